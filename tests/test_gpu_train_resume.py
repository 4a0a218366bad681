"""GPU: train.py stopped and resumed on this project's kernels alone (--deterministic, the native convolutions, --optim
native) ends with the bits of the run that never stopped: all parameters, all optimiser state, the quantiser counters,
the log's loss figures and the history (tests/train_resume_cases.py)."""
import pytest
import torch

import train_resume_cases as R

pytestmark = pytest.mark.gpu


def _guard(*args, **kwargs):
    raise AssertionError("torch.nn.functional.conv2d was called under a native --conv")


def _straight_stopped_resumed(tmp_path, monkeypatch, extra):
    a, b = tmp_path / "a", tmp_path / "b"
    straight = R.job(a, extra, "cuda")
    # from the second run on no library convolution may be reached (the first shows what the patch would hide:
    # nothing -- the runs are compared bit for bit)
    monkeypatch.setattr(torch.nn.functional, "conv2d", _guard)
    stopped = R.job(b, extra + ["--stop-after", "3"], "cuda")
    st = R.state(b, extra)
    assert (st["epoch"], st["next_batch"], st["global_batch"]) == (1, 3, 3) and len(stopped) == 1
    assert st["rng"]["device"] is not None and any(x.any() for x in st["acc"])
    resumed = R.job(b, extra + ["--resume"], "cuda")
    R.assert_same_end(a, b, extra, straight, resumed)


@pytest.mark.timeout(600)
def test_base_stage_on_native_kernels_resumes_to_the_same_bits(hip_backend, tmp_path, monkeypatch):
    _straight_stopped_resumed(tmp_path, monkeypatch, ["--conv", "native", "--loss", "ws", "--base", "--optim", "native"])


@pytest.mark.timeout(600)
def test_full_model_on_native_kernels_resumes_to_the_same_bits_across_level_merges(hip_backend, tmp_path, monkeypatch):
    """the quantiser merges its levels every 2 training calls: a merge on each side of the stop"""
    R.quantiser_merges_every(monkeypatch, 2)
    _straight_stopped_resumed(tmp_path, monkeypatch, ["--conv", "native-all", "--optim", "native"])
