"""GPU: the HIP ops against the REFERENCE's own results (tests/golden/ref_ops_*.npz: the reference's kernels
compiled for the CPU and run on the stored inputs, tests/golden/gen_golden.py), under the stored masks of the
elements the reference never writes.  Reads tests/golden/ only.

Each op keeps the bound it already has against the oracle in tests/test_gpu_ops.py, tests/test_gpu_backward.py
and tests/test_gpu_codec_vs_oracle.py -- the right-hand side is now the reference, not our restatement of it:
torch.equal for index work and the forwards without transcendentals; 1e-5 of the result's scale for the backward
sums (LDS atomics / another order of the sum), 1e-4 for the float-atomic sums (projection, quantiser levels).
The erf / exp ops run the product's published polynomials where the reference calls libm (DESIGN.md section 2,
divergence 1), so they keep the bounds those tests hold against the libm oracle: CDF tables at most one count
apart in fewer than 2 % of the entries, the GMM gradients within 1e-4 of scale, quantised
values within 1e-5 with fewer than 1e-4 of the indices on the other side of a level boundary, the level table
after a training-mode merge within 1e-6.  One departure from the bounds those files hold: the GMM loss, 1e-5 there
between two sides that run the same erf, is held here to the per-row bound that follows from the polynomial's
published accuracy (ref_ops_cases.gmm_loss_bound) -- against libm's erf 1e-5 cannot hold on
rows whose probability is near 1e-7, for the oracle as for the kernel.

The masked 5x5 wavefront convolution (tests/golden/ref_ops_econv.npz: the reference's 128-thread blocks run on the
cooperative launcher of oracle/ref_shim/) sums in another order than the reference (divergence 2): the HIP op is
held to the reference's stored results under the bound derived in ref_ops_cases.econv_bound, to exact zeros wherever
the reference wrote nothing, and to the bits of the oracle's order 1 on the stored inputs.
"""
import os

import pytest
import torch

import ref_ops_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
_stored = {}
_stored_econv = {}


def stored(name):
    if not _stored:
        _stored.update(C.load_fixtures(GOLDEN))
    return _stored[name]


def under_mask(a, b, masks, key):
    a = a.detach().cpu()
    assert tuple(a.shape) == tuple(b.shape), (key, tuple(a.shape), tuple(b.shape))
    if key in masks:
        keep = ~torch.as_tensor(masks[key])
        return a[keep], b[keep]
    return a, b


def same(got, ref, masks, key):
    a, b = under_mask(got[key], ref[key], masks, key)
    assert torch.equal(a, b), "%s: max abs diff %g" % (key, (a.double() - b.double()).abs().max().item())


def close(got, ref, masks, key, tol):
    a, b = under_mask(got[key], ref[key], masks, key)
    scale = max(1.0, b.abs().max().item())
    worst = (a - b).abs().max().item()
    assert worst <= tol * scale, "%s: %g > %g" % (key, worst, tol * scale)


def run_product(hip_backend, name):
    case, ins, ref, masks = stored(name)
    got = C.run(hip_backend, case, ins, DEV, tables=False)
    keys = [k for k in ref if not k.startswith("table_") and k != "fill_param"]
    assert [k for k in got if k != "fill_param"] == keys
    return case, got, ref, masks


def names(*ops):
    return [n for n in C.FIXTURE_CASES if C.CASES[n]["op"] in ops]


@pytest.mark.parametrize("name", names("slice", "uslice"))
def test_slice_uslice(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    same(got, ref, masks, "y")
    close(got, ref, masks, "gx", 1e-5)
    if case["op"] == "slice":      # columns at or beyond the tile width are exactly zero, as the reference writes them
        p = case["pad"]
        y = got["y"][:, :, p:got["y"].shape[2] - p, p:got["y"].shape[3] - p]
        for t, v in enumerate(C.widths(case)):
            assert y[t::C.NPART, :, :, v:].abs().sum().item() == 0


@pytest.mark.parametrize("name", names("pad"))
def test_pseudo_pad(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    assert got["fill_param"].tolist() == ref["fill_param"].tolist()
    if case["fill"]:
        same(got, ref, masks, "filled")
    same(got, ref, masks, "y")
    close(got, ref, masks, "gx", 1e-5)


@pytest.mark.parametrize("name", names("epad"))
def test_entropy_pad(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    close(got, ref, masks, "y", 1e-6)
    close(got, ref, masks, "gx", 1e-5)


@pytest.mark.parametrize("name", names("fill", "dtow", "context_reshape", "mask", "wave"))
def test_index_work_is_bit_exact(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    for key in got:
        same(got, ref, masks, key)


@pytest.mark.parametrize("name", C.ECONV_FIXTURE_CASES)
def test_masked_convolution(hip_backend, name):
    """EntropyConv2Op, every entry point, stepped over the whole wavefront, past its end and restarted"""
    from oracle import pconv_cpu as O
    if not _stored_econv:
        _stored_econv.update(C.load_econv_fixtures(GOLDEN))
    case, ins, ref, masks = _stored_econv[name]
    assert not masks                       # the reference leaves nothing unwritten: zero reads "not written"
    got = C.run(hip_backend, case, ins, DEV, tables=False)
    assert list(got) == list(ref)
    # within the derived bound of the reference; exactly 0 wherever the reference's result is 0 (nothing written
    # early or outside the wavefront, the pad_out ring left alone); the flag and the restart result agree
    print(name, "worst difference / bound: %.3f" % C.econv_within_bound(case, ins, got, ref))
    # and the product's own order, bit for bit
    assert O.CONV_ORDER == 1
    want = C.run(O, case, ins)
    for key in ref:
        assert torch.equal(got[key], want[key]), "%s: max abs diff %g" % (key, (got[key] - want[key]).abs().max().item())


@pytest.mark.parametrize("name", names("quant"))
def test_quantiser(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    # level tables: exp by the published polynomial here, libm there -- agreeing to an ulp or two, so the values do;
    # an index may differ only for an input on a level boundary
    close(got, ref, masks, "val", 1e-5)
    assert (got["val"] - ref["val"]).abs().max().item() < 1e-5
    if "idx" in ref:
        assert (got["idx"] != ref["idx"]).float().mean().item() < 1e-4
        assert (got["dq"] - ref["dq"]).abs().max().item() < 1e-5
    assert (got["weight_after"] - ref["weight_after"]).abs().max().item() < 1e-6
    assert (got["count_after"] - ref["count_after"]).abs().max().item() < 1e-6
    close(got, ref, masks, "g_in", 1e-6)
    close(got, ref, masks, "g_weight", 1e-4)
    same(got, ref, masks, "histogram")
    for t, v in enumerate(C.widths(case)):
        assert got["g_in"][t::C.NPART, :, :, v:].abs().sum().item() == 0


def test_gmm_loss(hip_backend):
    case, got, ref, masks = run_product(hip_backend, "gmm_loss")
    # 1e-5 is the bound against the oracle running the same polynomials; against the reference's libm erf the loss
    # of a row moves with the conditioning of -log(p + 1e-7): the per-row bound derived from the polynomial's
    # published accuracy (ref_ops_cases.gmm_loss_bound), which is below 1e-5 wherever p > 0.04
    diff = (got["loss"].double() - ref["loss"].double()).abs()
    assert (diff <= C.gmm_loss_bound(ref["loss"])).all(), (diff / C.gmm_loss_bound(ref["loss"])).max().item()
    for key in ("g_weight", "g_delta", "g_mean", "g_label"):
        close(got, ref, masks, key, 1e-4)


@pytest.mark.parametrize("name", names("gmm_table", "gmm_table_batch"))
def test_gmm_table(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    rows = got["table"]
    assert (rows[:, 0] == 0).all() and (rows[:, 8] == 65536).all() and (rows[:, 1:] - rows[:, :-1] >= 1).all()
    diff = (rows - ref["table"]).abs()
    assert diff.max().item() <= 1 and (diff > 0).float().mean().item() < 0.02
    if name == "gmm_table":
        same(got, ref, masks, "delta_after")
        weights = (got["weight_after"], ref["weight_after"])
    else:
        assert torch.equal(got["data_after"][1:], ref["data_after"][1:])
        weights = (got["data_after"][0], ref["data_after"][0])
    # the softmax written in place: exp within 2 ulp (include/pconv_detmath.h), see check_detmath of the CPU tests
    bound = (2 + 2 + (case["ng"] - 1) + 1) * 2.0 ** -23
    assert ((weights[0] - weights[1]).abs() / weights[1].abs().clamp_min(1e-30)).max().item() <= bound


@pytest.mark.parametrize("name", names("projects"))
def test_projects(hip_backend, name):
    case, got, ref, masks = run_product(hip_backend, name)
    same(got, ref, masks, "y")
    close(got, ref, masks, "gx", 1e-4)      # float atomics: the order of the sums is not defined
    close(got, ref, masks, "count", 1e-4)
