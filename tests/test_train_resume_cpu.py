"""train.py --resume on the CPU (the oracle backend, the shapes of tests/test_train_cpu.py): a run that is stopped and
resumed ends with the bits of the run that never stopped; what --resume refuses; the stop decision agreed between
ranks; the state file's atomic write."""
import os
import re
import sys

import pytest
import torch
import torch.multiprocessing as mp

import train_resume_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stop_and_resume(tmp_path, extra, stop_after):
    """(history of the straight run, of the stopped run, of the resumed run); directories a, b under tmp_path"""
    a, b = tmp_path / "a", tmp_path / "b"
    straight = R.job(a, extra)
    stopped = R.job(b, extra + ["--stop-after", str(stop_after)])
    st = R.state(b, extra)
    assert st["global_batch"] == stop_after
    resumed = R.job(b, extra + ["--resume"])
    return straight, stopped, resumed, st


@pytest.mark.timeout(900)
@pytest.mark.parametrize("extra, merges", [(["--base", "--optim", "torch"], None), (["--optim", "native"], None),
                                           (["--optim", "torch"], 2)],
                         ids=["base-torch", "full-native", "full-torch-merges"])
def test_stopped_mid_epoch_and_resumed_ends_with_the_bits_of_the_straight_run(oracle_backend, tmp_path, monkeypatch, extra, merges):
    """--stop-after 3 of 8 batches: mid-epoch, and in the middle of an accumulation window of 2.  merges: the
    quantiser merges its levels every 2 training calls, so one merge falls on each side of the stop"""
    if merges:
        R.quantiser_merges_every(monkeypatch, merges)
    straight, stopped, resumed, st = _stop_and_resume(tmp_path, extra, 3)
    assert (st["epoch"], st["next_batch"]) == (1, 3) and st["history"] == [] and len(stopped) == 1
    assert any(a.any() for a in st["acc"])                       # the half-filled window travels
    assert list(st["quant_calls"].values())[0] == {0: 3}
    R.assert_same_end(tmp_path / "a", tmp_path / "b", extra, straight, resumed)
    log = open(os.path.join(str(tmp_path / "b"), "save_models", R.prefix(extra) + "_logs_0.txt")).read()
    assert "resumed from" in log and "[3/8 (38%)]" in log          # a resumed epoch's lines keep the epoch's length
    assert ("optimiser step native" in log) == ("native" in extra)


@pytest.mark.timeout(900)
def test_stopped_at_an_epochs_end_resumes_into_the_next_epoch(oracle_backend, tmp_path):
    """the sampler's order of epoch 2 and the alternation of the two optimisers (epoch 2 trains the entropy model)
    are the straight run's"""
    extra = ["--optim", "native"]
    straight, stopped, resumed, st = _stop_and_resume(tmp_path, extra, 4)
    assert (st["epoch"], st["next_batch"]) == (2, 0) and len(st["history"]) == 1 and len(stopped) == 1
    assert len(st["optimizers"]["ent"]["state"]) == 0               # the entropy model's Adam has not stepped yet
    R.assert_same_end(tmp_path / "a", tmp_path / "b", extra, straight, resumed)
    assert len(R.state(tmp_path / "b", extra)["optimizers"]["ent"]["state"]) > 0


@pytest.mark.timeout(600)
def test_resume_refuses_another_trajectory_and_a_missing_file(oracle_backend, tmp_path):
    from pseudocylindrical_convolution_amd import optim, train
    extra = ["--base"]
    with pytest.raises(FileNotFoundError, match="no training state"):
        R.job(tmp_path, extra + ["--resume"])
    with pytest.raises(FileNotFoundError, match="elsewhere.pt"):
        R.job(tmp_path, extra + ["--resume", str(tmp_path / "elsewhere.pt")])
    R.job(tmp_path, extra + ["--stop-after", "1"])
    before = R.state(tmp_path, extra)
    for changed, name in ((["--batch-size", "2"], "--batch-size"), (["--seed", "5"], "--seed"), (["--loss", "ws"], "--loss")):
        with pytest.raises(ValueError, match="written with %s = " % name):
            R.job(tmp_path, extra + changed + ["--resume"])
    path = os.path.join(str(tmp_path), "save_models", R.prefix(extra) + "_state.pt")
    args = train.build_parser().parse_args(R.ARGS + ["--device", "cpu", "--dist-backend", "gloo"] + extra)
    with pytest.raises(ValueError, match="world size = 1, this run has 2"):
        optim.TrainState.load(path, args, 2, None, {}, None, None, torch.device("cpu"))
    assert R.difference(before, R.state(tmp_path, extra)) is None   # a refused resume writes nothing
    # ... and the arguments that do not shape the trajectory may change
    hist = R.job(tmp_path, extra + ["--resume", path, "--epochs", "1", "--verbose"])
    assert len(hist) == 1 and R.state(tmp_path, extra)["global_batch"] == 4


def test_a_state_file_cut_short_never_stands_under_the_final_name(tmp_path, monkeypatch):
    from pseudocylindrical_convolution_amd import optim, train
    from pseudocylindrical_convolution_amd.SphereDataset import MyDistributeSampler, SyntheticSphereDataSet
    args = train.build_parser().parse_args(R.ARGS)
    model = torch.nn.Linear(3, 2)
    sampler = MyDistributeSampler(SyntheticSphereDataSet(4, 16, 32, seed=1), 1, 0, 1)
    opts = {"other": torch.optim.Adam(model.parameters()), "ent": None}
    path = str(tmp_path / "state.pt")
    run = optim.TrainState()
    run.save(path, args, 1, model, opts, None, sampler, torch.device("cpu"))
    good = open(path, "rb").read()
    real = torch.save

    def cut_short(obj, f, *a, **k):
        real(obj, f, *a, **k)
        with open(f, "r+b") as fh:
            fh.truncate(100)
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", cut_short)
    run.global_batch = 7
    with pytest.raises(OSError, match="disk full"):
        run.save(path, args, 1, model, opts, None, sampler, torch.device("cpu"))
    assert open(path, "rb").read() == good and os.listdir(str(tmp_path)) == ["state.pt"]
    with pytest.raises(OSError):
        run.save(str(tmp_path / "fresh.pt"), args, 1, model, opts, None, sampler, torch.device("cpu"))
    assert os.listdir(str(tmp_path)) == ["state.pt"]
    monkeypatch.setattr(torch, "save", real)
    back = optim.TrainState.load(path, args, 1, model, opts, None, sampler, torch.device("cpu"))
    assert back.global_batch == 0


def _rank(rank, world, port, base_dir, ret):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from pseudocylindrical_convolution_amd.PCONV_operator import backend
    from oracle import pconv_cpu, coder_cpu
    backend.use(pconv_cpu, coder_cpu)
    pconv_cpu.set_detmath(True)
    torch.set_num_threads(2)
    from pseudocylindrical_convolution_amd import train
    trained = [0]
    real = train.forward_losses

    def counted(args, model, *a, **k):
        trained[0] += int(model.training)
        return real(args, model, *a, **k)

    train.forward_losses = counted
    args = train.build_parser().parse_args(
        R.ARGS + ["--device", "cpu", "--base", "--base-dir", base_dir, "--epochs", "100000", "--time-budget", "3"])
    hist = train.Job(rank, world, args)
    ret[rank] = (trained[0], len(hist))


@pytest.mark.timeout(300)
def test_two_ranks_agree_on_the_stop(tmp_path):
    """two gloo ranks under --time-budget 3 and far too many epochs: rank 0's decision is broadcast, so both leave
    after the same number of batches and meet in the checksum all-reduce (a rank-local deadline could hang here: this
    test's timeout would catch it)"""
    world, port = 2, 36000 + os.getpid() % 2000
    ret = mp.Manager().dict()
    mp.spawn(_rank, args=(world, port, str(tmp_path), ret), nprocs=world, join=True)
    assert ret[0] == ret[1] and ret[0][0] >= 1
    log = open(os.path.join(str(tmp_path), "save_models", "base_normal_16_8_16_logs_0.txt")).read()
    assert "time budget" in log
    spread = re.search(r"parameter checksum over 2 ranks: \S+, spread (\S+)", log)
    assert spread and float(spread.group(1)) == 0.0
    st = torch.load(os.path.join(str(tmp_path), "save_models", "base_normal_16_8_16_state.pt"), map_location="cpu")
    assert st["global_batch"] == ret[0][0] and st["fingerprint"]["world_size"] == 2
