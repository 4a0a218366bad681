"""The ordered (atomic-free) backward, without a GPU: the host builders of the reverse lists against numpy
constructions from the forward tables; the proof that "the order" of include/pconv_hip.h is the oracle's -- a
float32 walk of the lists equals the oracle's sequential scatter bit for bit; the quantiser's numpy twin within the
bound the default form is held to; train.py --deterministic."""
import os

import numpy as np
import pytest
import torch

import backward_ordered_cases as B
from oracle import pconv_cpu as O
from ref_ops_cases import NPART, PHI, THETA, W16, WEIGHTS

SETS = ("W16", "WNOPT", "WFULL")
WIDTHS = (24, 40, 72, 128)
P = B.P


def call(*a):
    from pseudocylindrical_convolution_amd._native import call as c
    return c(*a)


@pytest.mark.parametrize("kind", ["slice", "uslice"])
@pytest.mark.parametrize("wset", SETS)
@pytest.mark.parametrize("width", WIDTHS)
def test_tap_reverse_is_the_forward_table_transposed_in_order(kind, wset, width):
    wd, col, coef = B.forward_taps(kind, WEIGHTS[wset], NPART, width)
    got, ref = B.host_tap_reverse(kind, wd, col, coef, width), B.numpy_tap_reverse(kind, wd, col, coef, width)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    start, src, rc = got
    nsrc = NPART * width if kind == "uslice" else int(np.minimum(wd, width).sum())
    assert start[0] == 0 and start[-1] == 4 * nsrc == len(src)
    # every forward coefficient is in exactly one list: the sums agree (float64 sums of the same float32 values)
    fwd = coef.reshape(NPART, width, 4)
    live = fwd if kind == "uslice" else np.concatenate([fwd[t, :min(int(wd[t]), width)] for t in range(NPART)])
    assert abs(rc.astype(np.float64).sum() - live.astype(np.float64).sum()) < 1e-9 * max(1.0, nsrc)
    if kind == "uslice":       # lists of dead columns are empty
        for t in range(NPART):
            assert start[t * width + int(wd[t])] == start[(t + 1) * width]
    if wset == "WNOPT" and width == 24 and kind == "uslice":
        assert wd[0] == 3     # a 3-column polar tile: one source column meets a destination twice, in tap order
        k0, k1 = start[0], start[1]
        assert max(np.bincount(src[k0:k1])) == 2


def test_tap_reverse_refuses_bad_arguments_before_writing():
    from pseudocylindrical_convolution_amd._native import PconvError
    width = 40
    for kind in ("slice", "uslice"):
        wd, col, coef = B.forward_taps(kind, WEIGHTS["WNOPT"], NPART, width)
        n = call("pconv_host_tap_reverse_size", P(wd), NPART, width, int(kind == "uslice"))
        start, src, rc = np.full(NPART * width + 1, -7, np.int32), np.full(n, -7, np.int32), np.full(n, -7, np.float32)
        args = [P(wd), NPART, width, P(col), P(coef), int(kind == "uslice"), P(start), P(src), P(rc)]
        for hole in (0, 3, 4, 6, 7, 8):
            with pytest.raises(PconvError, match="null pointer"):
                call("pconv_host_tap_reverse", *[None if i == hole else a for i, a in enumerate(args)])
        bad = col.copy()
        period = int(wd[NPART - 1]) if kind == "uslice" else width
        bad[(NPART - 1) * width + 1] = period          # one past the period, in the LAST tile: nothing before it may be written
        with pytest.raises(PconvError, match="outside its period"):
            call("pconv_host_tap_reverse", *(args[:3] + [P(bad)] + args[4:]))
        bad[(NPART - 1) * width + 1] = -1
        with pytest.raises(PconvError, match="outside its period"):
            call("pconv_host_tap_reverse", *(args[:3] + [P(bad)] + args[4:]))
        wide = wd.copy()
        wide[3] = width + 1
        with pytest.raises(PconvError):
            call("pconv_host_tap_reverse", *([P(wide)] + args[1:]))
        assert (start == -7).all() and (src == -7).all() and (rc == -7).all()
    with pytest.raises(PconvError, match="int32"):     # 4 * npart * width entries
        big = np.full(1 << 14, 1 << 16, np.int32)
        call("pconv_host_tap_reverse", P(big), 1 << 14, 1 << 16, 4096, 4096, 1, 4096, 4096, 4096)


@pytest.mark.parametrize("near", [False, True])
def test_project_reverse_is_a_stable_sort_of_the_forward_walk(near):
    hs, ws, ho, wo = 32, 64, 12, 18
    tf = B.project_table(THETA, PHI, 0.5, ho, wo, hs, ws)
    got = B.host_project_reverse(tf, len(THETA), ho * wo, hs, ws, near)
    ref = B.numpy_project_reverse(tf, len(THETA), ho * wo, hs, ws, near)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype and np.array_equal(g, r)
    start, smp, wgt = got
    assert start[-1] == len(THETA) * ho * wo * (1 if near else 4)
    reached = np.zeros(hs * ws, bool)
    t = tf.reshape(-1, 2)
    if near:
        reached[np.minimum(np.floor(t[:, 1].astype(np.float64) + 0.5), hs - 1).astype(int) * ws +
                np.floor(t[:, 0].astype(np.float64) + 0.5).astype(int) % ws] = True
    else:
        tw, th = np.floor(t[:, 0]).astype(int), np.floor(t[:, 1]).astype(int)
        for r, c in ((th, tw), (th, (tw + 1) % ws), (np.minimum(th + 1, hs - 1), tw), (np.minimum(th + 1, hs - 1), (tw + 1) % ws)):
            reached[r * ws + c] = True
    assert 0 < reached.sum() < hs * ws               # some pixels no sample reaches: their lists are empty
    assert np.array_equal(start[1:] > start[:-1], reached)


def test_project_reverse_holds_the_clamped_corners_of_the_last_row_twice():
    hs, ws = 8, 16
    # three samples of one view on the last row (floor(fy) == hs - 1: ph clamps onto th), one of them on the seam
    tf = np.array([3.25, 7.5, 15.5, 7.0, 9.75, 7.25, 4.5, 2.5], np.float32)
    got, ref = B.host_project_reverse(tf, 1, 4, hs, ws, False), B.numpy_project_reverse(tf, 1, 4, hs, ws, False)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    start, smp, wgt = got
    for s, (tw, pw) in enumerate([(3, 4), (15, 0), (9, 10)]):
        for col in (tw, pw):
            p = (hs - 1) * ws + col
            assert list(smp[start[p]:start[p + 1]]) == [s, s]
    fx, fy = np.float32(3.25), np.float32(7.5)
    tx, ty = np.float32(fx - np.float32(3)), np.float32(fy - np.float32(7))
    ntx, nty = np.float32(1.0 - float(tx)), np.float32(1.0 - float(ty))
    p = (hs - 1) * ws + 3
    assert list(wgt[start[p]:start[p + 1]]) == [np.float32(ntx * nty), np.float32(ntx * ty)]   # (th,tw) before (ph,tw)


def test_project_reverse_refuses_bad_arguments_before_writing():
    from pseudocylindrical_convolution_amd._native import PconvError
    hs, ws = 8, 16
    tf = np.array([3.25, 7.5, 15.5, 7.0, 9.75, 7.25, 4.5, 2.5], np.float32)
    start, smp, wgt = np.full(hs * ws + 1, -7, np.int32), np.full(16, -7, np.int32), np.full(16, -7, np.float32)
    args = [P(tf), 1, 4, hs, ws, 0, P(start), P(smp), P(wgt)]
    for hole in (0, 6, 7, 8):
        with pytest.raises(PconvError, match="null pointer"):
            call("pconv_host_project_reverse", *[None if i == hole else a for i, a in enumerate(args)])
    for x, y in ((16.5, 2.0), (-0.5, 2.0), (3.0, 8.0), (3.0, -1.0)):
        bad = tf.copy()
        bad[6:] = (x, y)                              # the LAST sample lies outside the frame
        with pytest.raises(PconvError, match="outside"):
            call("pconv_host_project_reverse", *([P(bad)] + args[1:]))
    with pytest.raises(PconvError, match="int32"):
        call("pconv_host_project_reverse", P(tf), 1 << 10, 1 << 20, hs, ws, 0, P(start), P(smp), P(wgt))
    with pytest.raises(PconvError, match="int32"):
        call("pconv_host_project_reverse", P(tf), 1, 4, 1 << 16, 1 << 16, 0, P(start), P(smp), P(wgt))
    assert (start == -7).all() and (smp == -7).all() and (wgt == -7).all()


# ---- the order is the oracle's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["slice", "uslice"])
@pytest.mark.parametrize("wset,width", [(s, w) for s in SETS for w in ((24, 40) if s == "WNOPT" else (40, 72))])
def test_walking_the_lists_is_the_oracles_scatter_bit_for_bit(kind, wset, width):
    weight = WEIGHTS[wset]
    g = torch.Generator().manual_seed(width + len(wset))
    for rows in (1, 2):
        wd, col, coef = B.forward_taps(kind, weight, rows * NPART, width)
        lists = B.host_tap_reverse(kind, wd, col, coef, width)
        for pad in (0, 1, 2):
            img, tiles = (2, 2, rows * NPART, width), (2 * NPART, 2, rows + 2 * pad, width + 2 * pad)
            if kind == "slice":
                op = O.SphereSliceOp(NPART, 0, pad, weight)
                op.forward(torch.randn(*img, generator=g))
                grad = torch.randn(*tiles, generator=g)
                want, got = op.backward(grad)[0], B.walk_slice(grad, wd, lists, rows, width, pad)
            else:
                op = O.SphereUsliceOp(NPART, 0, pad, weight)
                op.forward(torch.randn(*tiles, generator=g))
                grad = torch.randn(*img, generator=g)
                want, got = op.backward(grad)[0], B.walk_uslice(grad, wd, lists, rows, width, pad)
            assert torch.equal(got, want), (rows, pad, int((got != want).sum()))
            assert want.abs().sum() > 0


@pytest.mark.parametrize("near", [False, True])
def test_walking_the_viewport_lists_is_the_oracles_scatter_bit_for_bit(near):
    hs, ws, ho, wo = 32, 64, 12, 18
    g = torch.Generator().manual_seed(5)
    op = O.ProjectsOp(ho, wo, THETA, PHI, 0.5, near)
    y = op.forward(torch.randn(2, 3, hs, ws, generator=g))[0]
    grad = torch.randn(y.shape, generator=g)
    want, want_count = op.backward(grad)
    tf = B.project_table(THETA, PHI, 0.5, ho, wo, hs, ws)
    assert np.array_equal(tf, op.tf[(hs, ws)])
    lists = B.host_project_reverse(tf, len(THETA), ho * wo, hs, ws, near)
    got, got_count = B.walk_projects(grad, lists, len(THETA), ho * wo, (2, 3, hs, ws))
    assert torch.equal(got, want) and torch.equal(got_count, want_count)
    assert (want_count == 0).any() and (want_count > 0).any()


# ---- quantiser: the fixed-shape reduction keeps the bound of the default form -------------------------------------
@pytest.mark.parametrize("shape", [(16, 192, 2, 64), (16, 6, 3, 100)])
def test_quant_twin_is_within_the_default_forms_bound_of_the_oracle(shape):
    """the bound of tests/test_gpu_backward.py::test_quant_backward: 1e-4 of max(1, the largest gradient)"""
    O.set_detmath(True)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(*shape, generator=g) * 1.2 - 0.1
    c = shape[1]
    weight = torch.zeros(c, 8)
    weight[:, 0] = 1. / 9
    weight[:, 1:] = float(np.log(1. / 9))
    weight += torch.rand(c, 8, generator=g) * 0.05
    octx = O.PseudoContextOp(NPART, 20, W16)
    cop = O.PseudoQuantOp(c, 8, NPART, 0.9, 100, 1, 0.1, octx.addr())
    val = cop.forward(x, weight, torch.zeros(c, 8), False)[0]
    want = cop.backward([torch.randn(shape, generator=g)], x, val)[1]
    widths = O.widths_v3(W16, NPART, shape[2] * NPART, shape[3])
    got = B.quant_twin(x.numpy(), val.numpy(), cop.quant_.reshape(shape).astype(np.float32),
                       cop.tab_.reshape(c, 8), widths, NPART)
    scale = max(1.0, want.abs().max().item())
    assert (torch.from_numpy(got) - want).abs().max().item() <= 1e-4 * scale
    assert want.abs().max().item() > 0


# ---- the switch and train.py --deterministic ------------------------------------------------------------------------
def test_switch_returns_the_previous_value_and_restores_it():
    from pseudocylindrical_convolution_amd import PCONV
    assert PCONV.backward_is_ordered() is False                      # default: the atomic kernels
    assert PCONV.ordered_backward() == False and PCONV.backward_is_ordered() is False   # noqa: E712  (None: a read)
    with PCONV.ordered_backward(True) as previous:
        assert previous == False and PCONV.backward_is_ordered() is True   # noqa: E712
        with PCONV.ordered_backward(False):
            assert PCONV.backward_is_ordered() is False
        assert PCONV.backward_is_ordered() is True
    assert PCONV.backward_is_ordered() is False
    with pytest.raises(KeyError):
        with PCONV.ordered_backward(True):
            raise KeyError("inside")
    assert PCONV.backward_is_ordered() is False
    assert PCONV.ordered_backward(True) == False and PCONV.ordered_backward(False) == True   # noqa: E712
    assert PCONV.backward_is_ordered() is False


def test_train_deterministic_sets_the_switch_and_logs_it(oracle_backend, tmp_path):
    import torch.distributed as dist
    from pseudocylindrical_convolution_amd import PCONV, train
    assert train.build_parser().parse_args([]).deterministic is False
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(35000 + os.getpid() % 2000), RANK="0", WORLD_SIZE="1")
    args = train.build_parser().parse_args(
        ["--device", "cpu", "--procedural", "2", "--height", "256", "--width", "512", "--batch-size", "1",
         "--test-batch-size", "1", "--acc-batch", "1", "--epochs", "1", "--max-steps", "1", "--valid-dim", "8",
         "--channels", "16", "--code-dim", "16", "--viewport_size", "24", "--workers", "0", "--no-opt", "--mean", "0",
         "--base-dir", str(tmp_path), "--base", "--deterministic"])
    assert args.deterministic is True
    seen = []
    train_epoch = train.train
    before = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark, torch.are_deterministic_algorithms_enabled())

    def spy(*a, **k):
        seen.append((PCONV.backward_is_ordered(), torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark,
                     torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()))
        return train_epoch(*a, **k)

    train.train = spy
    try:
        train.Job(0, 1, args)
    finally:
        train.train = train_epoch
        if dist.is_initialized():
            dist.destroy_process_group()
    assert seen == [(True, True, False, True, True)]
    assert PCONV.backward_is_ordered() is False                      # put back when the Job ends
    assert before == (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark,
                      torch.are_deterministic_algorithms_enabled())
    log = open(os.path.join(str(tmp_path), "save_models", "base_normal_16_8_16_logs_0.txt")).read()
    assert "deterministic: ordered backward kernels on" in log
    assert "parameter checksum over 1 ranks" in log
