"""GPU: the wide entropy nets (valid_dim 112 / 192: 28 / 48 channel groups, pseudo_codec.py:37-40) on the matrix
cores.  The encoder's hidden layers (84 -> 84 and 144 -> 144 channels) take the four-block form of
csrc/entropy_mfma.hip; its streams must be byte for byte the vector kernel's (PCONV_EE_BULK=valu) and the oracle's.

  * forms: which kernel each layer of an engine reports (pconv_ee_encoder_form);
  * streams of the matrix form == streams of the vector kernel on block shapes with remainders (symbol rows 10 / 5 per
    tile, widths that are not a multiple of 16), 1 / 3 / 8 frames per call and 1 / 3 / 4 encode step ranges, and they
    decode back to the symbols;
  * the oracle at 512 x 1024: the engine codes the oracle's symbols into the oracle's bytes and decodes them back, the
    HIP synthesis of the symbols is within 1e-4 of the oracle's image, quantiser ties counted;
  * the per-op wavefront ops (DInput2, EntropyCtxPadRun2, EntropyConv2, EntropyAdd, DExtract2) against the oracle at
    28 and 48 groups.  Tie counts go to wide_models_ties.json in the
    directory PCONV_TEST_REPORT_DIR names, when it is set."""
import json
import os

import pytest
import torch

from oracle import pconv_cpu as O

pytestmark = pytest.mark.gpu

VECTOR, MFMA16, FOUR_BLOCK = 0, 1, 2


@pytest.fixture(autouse=True)
def _detmath():
    O.set_detmath(True)
    yield


def _ent(vd, seed=17, scale=0.03):
    """an encoder's entropy net with small random weights (the wide-model test of test_gpu_engine.py)"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    torch.manual_seed(4321)
    enc = PC.PseudoEncoder(vd, 0).eval()
    g = torch.Generator().manual_seed(seed)
    enc.ent.load_state_dict({k: torch.randn(v.shape, generator=g) * scale for k, v in enc.ent.state_dict().items()})
    return enc.ent


def _engine(ent, h, w, nimg):
    from pseudocylindrical_convolution_amd.engine import EntropyEngine
    return EntropyEngine(ent, h, w, nimg, "cuda:0")


def _symbols(ent, nimg, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    sym = torch.randint(0, 8, (nimg * ent.npart, ent.ngroup, h, w), generator=g).float().cuda()
    return ent.fill(sym).contiguous()


# ---- a. forms ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("vd", [112, 192])
def test_wide_engine_forms(vd, hip_backend, monkeypatch):
    monkeypatch.delenv("PCONV_EE_BULK", raising=False)
    ent = _ent(vd)
    assert ent.ngroup == vd // 4
    # even width: the hidden and output layers on the four-block form, the input layer on the vector kernel
    assert _engine(ent, 10, 64, 1).encoder_forms == (VECTOR,) + (FOUR_BLOCK,) * 11
    assert _engine(ent, 5, 40, 1).encoder_forms == (VECTOR,) + (FOUR_BLOCK,) * 11
    # odd width: the vector kernel everywhere
    assert _engine(ent, 10, 65, 1).encoder_forms == (VECTOR,) * 12
    monkeypatch.setenv("PCONV_EE_BULK", "valu")
    assert _engine(ent, 10, 64, 1).encoder_forms == (VECTOR,) * 12


def test_14_group_engine_forms_unchanged(hip_backend, monkeypatch):
    for knob in ("PCONV_EE_BULK", "PCONV_EE_BULK0", "PCONV_EE_MFMA_FORM", "PCONV_EE_MFMA_WSRC", "PCONV_EE_MFMA_NT",
                 "PCONV_EE_MFMA_WAVES"):
        monkeypatch.delenv(knob, raising=False)
    ent = _ent(56)
    eng = _engine(ent, 4, 128, 1)
    assert eng.encoder_forms == (MFMA16,) + (FOUR_BLOCK,) * 11
    monkeypatch.setenv("PCONV_EE_MFMA_FORM", "16x4")
    assert _engine(ent, 4, 128, 1).encoder_forms == (MFMA16,) * 12
    monkeypatch.setenv("PCONV_EE_BULK", "valu")
    assert _engine(ent, 4, 128, 1).encoder_forms == (VECTOR,) * 12
    # a bad layer: a negative value and the reason
    assert eng.lib.pconv_ee_encoder_form(eng.handle, 12) < 0
    assert b"ee_encoder_form" in (eng.lib.pconv_last_error() or b"")


# ---- b. same streams as the vector kernel ------------------------------------------------------------------------

def _encode(eng, sym, ranges):
    if ranges is None:
        return eng.encode(sym)
    eng.encode_begin(sym, ranges)
    return eng.encode_end()


# (frames, symbol rows per tile, width, encode ranges): rows 10 and 5 (block rows 2 and 1 of the four-tile block),
# widths 70 and 40 (not multiples of 16), 1 / 3 / 8 frames, one piece and 3 / 4 step ranges
SHAPES = [(1, 10, 70, 1), (3, 5, 40, 3), (8, 10, 40, 4), (1, 4, 128, None)]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("vd", [112, 192])
def test_wide_streams_equal_vector_kernel(vd, hip_backend, monkeypatch):
    ent = _ent(vd)
    for k, (nimg, h, w, ranges) in enumerate(SHAPES):
        sym = _symbols(ent, nimg, h, w, seed=100 + k)
        monkeypatch.delenv("PCONV_EE_BULK", raising=False)
        eng = _engine(ent, h, w, nimg)
        assert eng.encoder_forms[1:] == (FOUR_BLOCK,) * 11
        fast = _encode(eng, sym, ranges)
        monkeypatch.setenv("PCONV_EE_BULK", "valu")
        ref_eng = _engine(ent, h, w, nimg)
        assert ref_eng.encoder_forms == (VECTOR,) * 12
        ref = _encode(ref_eng, sym, ranges)
        assert len(fast) == nimg
        for i in range(nimg):
            assert fast[i] == ref[i], "vd %d, shape %s, frame %d: %d vs %d bytes" % (
                vd, (nimg, h, w, ranges), i, len(fast[i]), len(ref[i]))
        assert torch.equal(eng.decode(fast), sym), "vd %d, shape %s: decoded symbols differ" % (vd, (nimg, h, w, ranges))
        del eng, ref_eng


# ---- c. oracle parity at 512 x 1024 ------------------------------------------------------------------------------

H, W = 512, 1024


def _codec(vd):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    torch.manual_seed(1234)
    enc, dec = PC.PseudoEncoder(vd, 0).eval(), PC.PseudoDecoder(vd, 0).eval()
    g = torch.Generator().manual_seed(7 + vd)
    sd = {k: torch.randn(v.shape, generator=g) * 0.05 for k, v in enc.ent.state_dict().items()}
    enc.ent.load_state_dict(sd)
    dec.ent.load_state_dict(sd)
    dec.quant.weight.data.copy_(enc.quant.weight.data)
    return enc, dec


def _frame(seed):
    x = torch.rand(1, 3, H, W, generator=torch.Generator().manual_seed(seed))
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    return (0.5 + 0.3 * torch.sin(6.28318 * 3 * xx) * torch.cos(3.14159 * 2 * yy) + 0.2 * (x - 0.5)).clamp_(0, 1).contiguous()


def _oracle(vd, x, tmp_path):
    from pseudocylindrical_convolution_amd.PCONV_operator import backend
    from oracle import coder_cpu
    backend.use(O, coder_cpu)
    threads = torch.get_num_threads()
    torch.set_num_threads(O.set_num_threads())
    try:
        enc, dec = _codec(vd)
        sym = enc.ent.fill(enc.symbols(x)).clone()
        path = str(tmp_path / ("oracle_%d.bin" % vd))
        enc.ent.start(path)
        enc.ent(sym)
        with open(path, "rb") as f:
            data = f.read()
        rec = dec.reconstruct(sym).clone()
    finally:
        backend.reset()
        torch.set_num_threads(threads)
    return sym, data, rec


def _report(key, value):
    out = os.environ.get("PCONV_TEST_REPORT_DIR")
    if not out:
        return
    path = os.path.join(out, "wide_models_ties.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        report = {}
        if os.path.exists(path):
            with open(path) as f:
                report = json.load(f)
        report[key] = value
        with open(path, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
    except (OSError, ValueError):
        pass


@pytest.mark.timeout(1500)
@pytest.mark.parametrize("vd", [112, 192])
def test_wide_models_against_the_oracle(vd, hip_backend, tmp_path, monkeypatch):
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    monkeypatch.delenv("PCONV_EE_BULK", raising=False)
    x = _frame(vd)
    csym, cbytes, crec = _oracle(vd, x, tmp_path)
    assert len(csym.unique()) >= 4, "this draw does not exercise the alphabet"
    enc, dec = _codec(vd)
    eng = CodecEngine(vd, 0, enc, dec)
    h2, w2 = 2 * (H // 256), 2 * (W // 16)
    gsym = eng.symbols(x.cuda()).cpu()
    ties = int((gsym != csym).sum())
    assert ties <= 8, "%d of %d symbols differ from the oracle's" % (ties, csym.numel())
    ee = eng._engine("enc", h2, w2, 1)
    assert ee.encoder_forms == (VECTOR,) + (FOUR_BLOCK,) * 11
    streams = ee.encode(csym.cuda().contiguous())
    assert streams[0] == cbytes, "engine stream %d bytes, oracle %d" % (len(streams[0]), len(cbytes))
    if ties == 0:
        assert eng.encode(x.cuda())[0] == cbytes
    back = eng._engine("dec", h2, w2, 1).decode([cbytes]).cpu()
    assert torch.equal(back, csym), "decoded symbols differ from the oracle's"
    rec = eng.decode([cbytes], H, W).cpu()
    err = (rec - crec).abs().max().item()
    assert err < 1e-4, "reconstruction differs from the oracle by %g" % err
    _report("vd%d" % vd, {"ties": ties, "symbols": csym.numel(), "bytes": len(cbytes),
                          "bpp": round(len(cbytes) * 8.0 / H / W, 4), "recon_max_abs_err": err})


# ---- d. the per-op wavefront ops against the oracle at 28 / 48 groups ------------------------------------------

@pytest.mark.timeout(900)
@pytest.mark.parametrize("nimg,h,w,ngroup", [(1, 1, 32, 28), (1, 1, 24, 48)])
def test_wide_wavefront_ops_bit_exact(nimg, h, w, ngroup):
    from test_gpu_ops import P, W16, _wavefront_net
    g = _wavefront_net(P(), nimg, h, w, ngroup, seed=23)
    c = _wavefront_net(O, nimg, h, w, ngroup, seed=23)
    assert g["counts"] == c["counts"]
    assert sum(g["counts"]) == int((g["data"].shape[1] * h * nimg) * sum(int(x) for x in O.widths_v3(W16, 16, 16 * h, w)))
    for k in ("ctx", "y1", "y2", "y3"):
        assert torch.equal(g[k], c[k]), k
    for tg, tc in zip(g["tables"], c["tables"]):
        assert torch.equal(tg, tc)
