"""What the stop-and-resume tests share (CPU: the oracle backend; GPU: the HIP backend): train.Job in this process at
the shapes of tests/test_train_cpu.py, and the comparison of two runs' final state files, log lines and histories."""
import math
import os
import re

import torch

# 8 frames of 256 x 512, 16 channels, 4 batches per epoch in accumulation windows of 2, two epochs: the first trains the
# transforms, the second (full model) the entropy model
ARGS = ["--synthetic", "8", "--height", "256", "--width", "512", "--batch-size", "1", "--test-batch-size", "1",
        "--acc-batch", "2", "--epochs", "2", "--valid-dim", "8", "--channels", "16", "--code-dim", "16",
        "--viewport_size", "24", "--lr", "0.001", "--mean", "1.0", "--workers", "0", "--no-opt", "--clip", "1.0",
        "--max-steps", "4", "--deterministic"]
_port = [34000 + os.getpid() % 2000]


def job(base_dir, extra, device="cpu"):
    """train.Job as the one rank of a run; returns its history"""
    import torch.distributed as dist
    from pseudocylindrical_convolution_amd import train
    _port[0] += 1
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port[0]), RANK="0", WORLD_SIZE="1")
    args = train.build_parser().parse_args(ARGS + ["--device", device, "--dist-backend", "gloo", "--base-dir", str(base_dir)]
                                           + list(extra))
    try:
        return train.Job(0, 1, args)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def quantiser_merges_every(monkeypatch, calls):
    """every quantiser op made from here on merges its levels every `calls` training calls (100 in the product)"""
    from pseudocylindrical_convolution_amd.PCONV_operator import ops
    real = ops.PseudoQUANTV2.__init__

    def init(self, *a, **k):
        real(self, *a, **k)
        for op in self.op.values():
            op.mod_ = calls

    monkeypatch.setattr(ops.PseudoQUANTV2, "__init__", init)


def prefix(extra):
    return "base_normal_16_8_16" if "--base" in extra else "ent_normal_16_8_16"


def state(base_dir, extra):
    return torch.load(os.path.join(str(base_dir), "save_models", prefix(extra) + "_state.pt"), map_location="cpu")


def batch_lines(base_dir, extra):
    """the per-batch lines of the log: epoch, position and the four loss figures as they were printed"""
    log = open(os.path.join(str(base_dir), "save_models", prefix(extra) + "_logs_0.txt")).read()
    return re.findall(r"^Train Epoch: .*$", log, flags=re.M)


def difference(a, b, where="state"):
    """None when a and b are the same, bit for bit in every tensor (a NaN float equals a NaN float); else where they
    differ first"""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)) or a.dtype != b.dtype or a.shape != b.shape:
            return where + ": tensors of another kind"
        if a.is_floating_point():
            view = {4: torch.int32, 8: torch.int64, 2: torch.int16}[a.element_size()]
            a, b = a.contiguous().view(view), b.contiguous().view(view)
        return None if torch.equal(a, b) else "%s: %d of %d entries differ" % (where, int((a != b).sum()), a.numel())
    if isinstance(a, dict) and isinstance(b, dict):
        if sorted(map(str, a)) != sorted(map(str, b)):
            return "%s: keys %s against %s" % (where, sorted(map(str, a)), sorted(map(str, b)))
        return next((d for d in (difference(a[k], b[k], "%s[%r]" % (where, k)) for k in a) if d), None)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        if len(a) != len(b):
            return "%s: %d entries against %d" % (where, len(a), len(b))
        return next((d for d in (difference(x, y, "%s[%d]" % (where, i)) for i, (x, y) in enumerate(zip(a, b))) if d), None)
    if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
        return None
    return None if a == b else "%s: %r against %r" % (where, a, b)


def assert_same_end(straight_dir, resumed_dir, extra, hist_straight, hist_resumed):
    """the resumed run ended where the straight one did: every parameter, every optimiser tensor and step count, the
    quantiser counters, best losses, sampler, random generators and history of the two final state files, the
    per-batch log lines (the resumed run's log is the stopped run's, appended to) and the returned histories"""
    a, b = state(straight_dir, extra), state(resumed_dir, extra)
    assert a["epoch"] == 3 and a["next_batch"] == 0 and a["global_batch"] == 8
    assert sum(1 for v in a["quant_calls"].values() for n in v.values() if n == 8) == 1
    diff = difference(a, b)
    assert diff is None, diff
    assert len(a["optimizers"]["other"]["state"]) > 10
    la, lb = batch_lines(straight_dir, extra), batch_lines(resumed_dir, extra)
    assert len(la) == 8 and la == lb
    assert difference(list(hist_straight), list(hist_resumed), "history") is None
    assert difference([[list(l), list(s)] for l, s in hist_straight], a["history"], "history in the file") is None
