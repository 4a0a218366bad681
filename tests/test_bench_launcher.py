"""bench.py's own N > 1 path on the CPU: `python bench.py --gpus 2` must start two
ranks (children, rendezvous on 127.0.0.1), every rank runs `bench.run`, and rank 0
prints one JSON line with n_gpus == 2 and the SUM of both shards.  The ranks use
gloo and a toy oracle workload (tests/helpers/bench_dryrun_rank.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "helpers", "bench_dryrun_rank.py")


def _run(nproc, tmp_path, frames=("--frames-per-gpu", "2"), env=None):
    child_env = {"PCONV_DRYRUN_DIR": str(tmp_path)}
    child_env.update(env or {})
    code = ("import sys; sys.path.insert(0, %r); import bench; "
            "sys.exit(bench.launch_ranks(%d, ['--gpus', '%d', '--steps', '2', '--warmup', '1', '--prime', '0', '--full', "
            "%r, %r], script=%r, env=%r))"
            % (ROOT, nproc, nproc, frames[0], frames[1], WORKER, child_env))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_launcher_starts_two_ranks_and_reduces(tmp_path):
    two = _run(2, tmp_path)
    assert two["n_gpus"] == 2 and two["steps"] == 2 and two["scaling"] == "weak"
    assert two["config"]["frames_per_gpu"] == 2
    # weak scaling: twice the pixels of one rank's shard in the same number of steps
    pixels_per_rank_step = 2 * 256 * 1024
    assert abs(two["value"] * 1e6 * two["ms_per_step"] * 1e-3 - 2 * pixels_per_rank_step) / (2 * pixels_per_rank_step) < 0.01
    assert two["config"]["bpp"] > 0
    # every rank kept its own slice of the host cores (bench.pin_rank), before creating any thread
    allowed = sorted(os.sched_getaffinity(0))
    kept = [json.load(open(os.path.join(str(tmp_path), "affinity_r%d.json" % r))) for r in range(2)]
    if len(allowed) >= 2:
        assert not set(kept[0]["cpus"]) & set(kept[1]["cpus"])
        assert sorted(kept[0]["cpus"] + kept[1]["cpus"]) == allowed
        assert two["config"]["cores_per_rank"] == len(kept[0]["cpus"]) == kept[0]["torch_threads"]


@pytest.mark.timeout(1500)
def test_eight_ranks_on_one_host_share_the_quota(tmp_path):
    """BASELINE config #5's process model (one process per GPU on one host, test/trainDDP_Full.py:83-86,201-204)
    at its full width on the CPU: 8 gloo ranks of bench.run.  Every rank keeps a slice of its own of the host
    CPUs, the native engine of every rank sizes its host threads by quota / 8 (not by the affinity mask), and the
    ranks that would poll through the GPU part of a step never add up to more runnable spinners than the quota."""
    allowed = sorted(os.sched_getaffinity(0))
    quota = 16                                                  # the GPU box's container: 16 CPUs, shared by the ranks
    (tmp_path / "cpu.max").write_text("%d 100000" % (quota * 100000))
    out = _run(8, tmp_path, ("--frames-per-gpu", "1"), env={"PCONV_CGROUP_CPU_MAX": str(tmp_path / "cpu.max")})
    assert out["n_gpus"] == 8 and out["scaling"] == "weak"
    pixels = 8 * 256 * 1024
    assert abs(out["value"] * 1e6 * out["ms_per_step"] * 1e-3 - pixels) / pixels < 0.01
    kept = [json.load(open(os.path.join(str(tmp_path), "affinity_r%d.json" % r))) for r in range(8)]
    assert all(k["local_world"] == 8 for k in kept)
    if len(allowed) >= 8:
        seen = [c for k in kept for c in k["cpus"]]
        assert len(seen) == len(set(seen)) and sorted(seen) == allowed      # disjoint, covering
    for k in kept:
        assert k["engine_host_cpus"] == min(len(k["cpus"]), quota // 8)
        # 8 frames per rank = 8 decode threads + the caller on 2 CPUs: the workers block instead of polling
        assert k["engine_spin_us_8_frames"] == 60
    spinners = sum(8 for k in kept if k["engine_spin_us_8_frames"] > 60)
    assert spinners <= quota


@pytest.mark.timeout(1200)
def test_strong_scaling_mode_splits_a_fixed_batch(tmp_path):
    """--frames-total F (BASELINE config #5: batch 64 over N GPUs): rank r takes frames r::world"""
    two = _run(2, tmp_path, ("--frames-total", "5"))
    assert two["n_gpus"] == 2 and two["scaling"] == "strong" and two["config"]["frames_total"] == 5
    kept = [json.load(open(os.path.join(str(tmp_path), "affinity_r%d.json" % r))) for r in range(2)]
    assert [k["frames"] for k in kept] == [3, 2]
    pixels_step = 5 * 256 * 1024
    assert abs(two["value"] * 1e6 * two["ms_per_step"] * 1e-3 - pixels_step) / pixels_step < 0.01


def test_rank_cpu_slices_are_disjoint_and_cover():
    sys.path.insert(0, ROOT)
    import bench
    for ncpu, world in ((128, 8), (16, 8), (10, 4), (8, 8), (3, 8)):
        allowed = list(range(100, 100 + ncpu))
        parts = [bench.rank_cpus(r, world, allowed) for r in range(world)]
        if ncpu >= world:
            assert sorted(c for p in parts for c in p) == allowed
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
        else:
            assert all(p == allowed for p in parts)


def test_main_becomes_launcher_only_without_world_size(monkeypatch):
    """--gpus N with WORLD_SIZE set (the driver's torch.distributed.run) must NOT spawn again"""
    sys.path.insert(0, ROOT)
    import bench
    calls = []
    monkeypatch.setattr(bench, "launch_ranks", lambda n, argv, **kw: calls.append((n, list(argv))) or 0)
    monkeypatch.setattr(bench, "run", lambda args, **kw: calls.append(("run", args.gpus)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "4", "--steps", "1"])
    assert e.value.code == 0 and calls == [(4, ["--gpus", "4", "--steps", "1"])]
    calls.clear()
    monkeypatch.setenv("WORLD_SIZE", "4")
    bench.main(["--gpus", "4", "--steps", "1"])
    assert calls == [("run", 4)]
    calls.clear()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main(["--gpus", "1", "--steps", "1"])
    assert calls == [("run", 1)]


def test_plain_run_flags_and_dump_row_sample():
    """--full is off by default; --dump-outputs' row sample is the same from run to run, sorted, distinct, and
    within the budget (None when everything fits)"""
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not args.full and args.dump_outputs is None and args.steps == 3
    args = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert args.full and args.dump_outputs == "out"
    assert bench.row_sample(2048, 1000, 2048 * 1000) is None
    a, b = bench.row_sample(2048, 393216, bench.DUMP_BUDGET), bench.row_sample(2048, 393216, bench.DUMP_BUDGET)
    assert (a == b).all() and len(a) == bench.DUMP_BUDGET // 393216
    assert (a[1:] > a[:-1]).all() and a[0] >= 0 and a[-1] < 2048
    assert len(bench.row_sample(4, 10 ** 9, 100)) == 1
    assert bench.DUMP_BUDGET + 2 * 4096 < 64 * 10 ** 6


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench

    class Load(object):
        def outputs(self, budget):
            rows = bench.row_sample(64, budget // 8, budget)
            return {"x": np.arange(6, dtype=np.float32), "x_rows": rows.astype(np.float64)}

    assert bench.dump_outputs(Load(), str(tmp_path / "d")) == ["x", "x_rows"]
    x = np.load(str(tmp_path / "d" / "x.npy"))
    assert x.dtype == np.float32 and (x == np.arange(6)).all()
    assert np.load(str(tmp_path / "d" / "x_rows.npy")).shape == (8,)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_dumps_what_its_last_step_computed(tmp_path):
    """a plain `bench.py` run (no --full) on the HIP engine, two frames in two calls: one JSON line with the contract
    fields, and --dump-outputs holds both frames' bitstreams (as many bits as the line's bpp says) and the uint8
    images that reached host memory"""
    import numpy as np
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--prime", "0", "--height", "256", "--width", "512", "--frames-per-gpu", "2",
                        "--max-frames-per-call", "1", "--dump-outputs", out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert "cpu_baseline" not in line and "entropy" not in line and line["roofline"] is None
    lengths = np.load(os.path.join(out, "stream_lengths.npy"))
    streams = np.load(os.path.join(out, "streams.npy"))
    rec = np.load(os.path.join(out, "reconstruction.npy"))
    assert lengths.dtype == np.float64 and streams.dtype == rec.dtype == np.float32
    assert lengths.shape == (2,) and streams.size == lengths.sum()
    assert abs(lengths.sum() * 8 / (2 * 256 * 512) - line["config"]["bpp"]) < 1e-3
    assert ((streams >= 0) & (streams <= 255) & (streams == np.round(streams))).all()
    assert rec.shape == (2, 256, 512, 3) and ((rec >= 0) & (rec <= 255) & (rec == np.round(rec))).all()
    assert rec.std() > 1.0


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_dump_sample_truncation_and_reused_slots_on_the_engine(hip_backend):
    """bench.CodecWorkload.outputs on the HIP engine, three one-frame calls through one FramePipe (slots s, 1 - s, s: the
    first call's pinned images are overwritten by the third and come from its reconstruction instead), with a budget
    small enough to force the seeded row sample and the truncation of the streams, as at the headline shape: the
    sampled rows and the stream prefixes are those of the whole outputs, the host images are tensor2img of the
    reconstructions io="resident" returns, and a resident workload dumps the same reconstructions as float32"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--height", "256", "--width", "512", "--frames-per-gpu", "3", "--max-frames-per-call", "1"])
    load = bench.CodecWorkload(args, 0, 0, "cuda:0")
    for _ in range(2):
        load.step()
    torch.cuda.synchronize()
    slots = [c["slot"] for c in load.calls]
    assert slots[0] == slots[2] != slots[1]
    whole = load.outputs(bench.DUMP_BUDGET)
    assert "reconstruction_rows" not in whole and whole["reconstruction"].shape == (3, 256, 512, 3)
    lengths = whole["stream_lengths"].astype(np.int64)
    assert whole["streams"].size == lengths.sum()
    budget = 4 * 16 * int(lengths.min() // 2)               # room for half of the shortest stream, per stream
    small = load.outputs(budget)
    rows = small["reconstruction_rows"].astype(np.int64)
    assert 1 <= len(rows) < 256 and (rows == bench.row_sample(256, 3 * 512 * 3 * 4, budget - budget // 4)).all()
    assert (small["reconstruction"] == whole["reconstruction"][:, rows]).all()
    keep = budget // 16 // 3
    assert (small["stream_lengths"] == whole["stream_lengths"]).all() and small["streams"].size == 3 * keep
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    for i in range(3):
        assert (small["streams"][i * keep:(i + 1) * keep] == whole["streams"][starts[i]:starts[i] + keep]).all()
    assert small["streams"].nbytes <= budget // 4
    assert small["reconstruction"].nbytes <= max(budget - budget // 4, 3 * 512 * 3 * 4)
    # the images that reached host memory (slots 1 and the last 0) and the one rebuilt for the overwritten slot are
    # all tensor2img of the reconstructions the resident path returns
    load.io = "resident"
    res = load.outputs(bench.DUMP_BUDGET)["reconstruction"]
    assert res.shape == (3, 3, 256, 512) and res.dtype == np.float32
    assert (whole["reconstruction"] == (res * 255.0).transpose(0, 2, 3, 1).astype(np.uint8)).all()
    res_small = load.outputs(budget)
    assert (res_small["reconstruction"] == res[:, :, rows]).all()
