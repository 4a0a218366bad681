"""GPU: rate without coding (pconv_ee_rate, EntropyEngine.rate, CodecEngine.rate / evaluate, pseudo_codec --rd).

The code length of a symbol is 16 - log2(c[s+1] - c[s]) of the row the coder gets (rate.py).  Checked here:
  1. against the rows the per-op path hands to the coder (a recording wrapper around ent.mcoder), totals, per
     (tile, group) and per latent position;
  2. the stream bracket (test_rate_cpu.py) against the engine's own streams, valid_dim 56 / 112 / 192;
  3. a frame's figures are the same bits alone, in a batch, on a second run and with another chunking;
  4. evaluate() = (rate(), decode(encode())) without coder or decoder, codable and non-codable sizes;
  5. the engine codes and decodes after rate() as before, rate() during a pending encode_begin is refused;
  6. an invalid label makes exactly its (frame, tile, group) entry and its map entry NaN;
  7. --rd end to end against --enc / --test on the same image.
Shapes: 256x512 (2 x 64 symbols per tile), 512x528 (4 rows, 66 columns: a ragged last block), 300x500 (not codable)."""
import os
import re

import numpy as np
import pytest
import torch

from test_rate_cpu import RecordingCoder, bracket

pytestmark = pytest.mark.gpu

FOUR_BLOCK = 2


def _codec(vd=56, scale=0.05):
    """tests/test_gpu_engine.py::_codec, any valid_dim and weight scale (0.3: most rows have one-count bins)"""
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    torch.manual_seed(1234)
    enc, dec = PC.PseudoEncoder(vd, 0), PC.PseudoDecoder(vd, 0)
    g = torch.Generator().manual_seed(7)
    sd = {k: torch.randn(v.shape, generator=g) * scale for k, v in enc.ent.state_dict().items()}
    enc.ent.load_state_dict(sd)
    dec.ent.load_state_dict(sd)
    dec.quant.weight.data.copy_(enc.quant.weight.data)
    return enc, dec


def _engine(vd=56, scale=0.05):
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    enc, dec = _codec(vd, scale)
    return CodecEngine(vd, 0, enc, dec)


def _frames(n, h, w, seed=1):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed)).cuda()


# ---- 1. against the rows the coder gets ----------------------------------------------------------------------------

def _per_op_rows(enc, x, path):
    """the HIP per-op encoder on x: (rows, labels, tile*ngroup + group, latent position) of every coded symbol, in
    coding order.  The ids come from two more DExtract2(label=True) run in lock-step with the encoder's own over
    tensors that hold them."""
    from pseudocylindrical_convolution_amd.PCONV_operator import DExtract2
    sym = enc.symbols(x)
    npart, ngroup = enc.ent.npart, enc.ent.ngroup
    h, w = sym.shape[2], sym.shape[3]
    tile = torch.arange(npart).view(npart, 1, 1, 1)
    group = torch.arange(ngroup).view(1, ngroup, 1, 1)
    row = torch.arange(h).view(1, 1, h, 1)
    col = torch.arange(w).view(1, 1, 1, w)
    shape = (npart, ngroup, h, w)
    id_tg = (tile * ngroup + group).expand(shape).float().contiguous().cuda()
    id_pos = ((tile * h + row) * w + col).expand(shape).float().contiguous().cuda()   # (< 2^24: exact in float32)
    ext_tg = DExtract2(npart, ngroup, True, enc.ent.ctx2, device=0)
    ext_pos = DExtract2(npart, ngroup, True, enc.ent.ctx2, device=0)
    got_tg, got_pos = [], []

    def on_step(num):
        got_tg.append(ext_tg(id_tg)[0].reshape(-1)[:num].to(torch.int64).cpu().numpy())
        got_pos.append(ext_pos(id_pos)[0].reshape(-1)[:num].to(torch.int64).cpu().numpy())

    enc.ent.start(path)
    ext_tg.restart()
    ext_pos.restart()
    rec = enc.ent.mcoder = RecordingCoder(enc.ent.mcoder, on_step)
    enc.ent(sym)
    tables, labels = rec.rows()
    return tables, labels, np.concatenate(got_tg), np.concatenate(got_pos), (npart, ngroup, h, w)


@pytest.mark.parametrize("height,width", [(256, 512), (512, 528)])
def test_rate_equals_the_rows_the_coder_gets(height, width, hip_backend, tmp_path):
    from pseudocylindrical_convolution_amd import rate
    eng = _engine()
    x = _frames(1, height, width, seed=3)
    tables, labels, tg, pos, (npart, ngroup, h, w) = _per_op_rows(eng.enc, x, str(tmp_path / "per_op.bin"))
    m = eng._engine("enc", h, w, 1).symbols_per_image
    assert len(labels) == m and (m == 23408 or (height, width) != (256, 512))
    ref = rate.row_bits(tables, labels)
    assert np.isfinite(ref).all()
    # every (tile, group) and every live position exactly once per group
    assert np.array_equal(np.bincount(pos, minlength=npart * h * w).reshape(npart, h, w).sum((1, 2)) // ngroup,
                          np.bincount(tg, minlength=npart * ngroup).reshape(npart, ngroup)[:, 0])
    ref_tg = np.bincount(tg, weights=ref, minlength=npart * ngroup).reshape(npart, ngroup)
    ref_pos = np.bincount(pos, weights=ref, minlength=npart * h * w).reshape(npart * h, w)
    live = np.bincount(pos, minlength=npart * h * w).reshape(npart * h, w) > 0

    bits, pmap = eng.rate(x, rate_map=True)
    assert bits.dtype == torch.float64 and tuple(bits.shape) == (1, npart, ngroup) and bits.is_cuda
    assert pmap.dtype == torch.float32 and tuple(pmap.shape) == (1, npart * h, w) and pmap.is_cuda
    bits, pmap = bits[0].cpu().numpy(), pmap[0].cpu().numpy()
    total_err = abs(bits.sum() - ref.sum()) / ref.sum()
    table_err = np.max(np.abs(bits - ref_tg) / ref_tg)
    map_err = np.max(np.abs(pmap[live].astype(np.float64) - ref_pos[live]) / ref_pos[live])
    tile_sum = pmap.astype(np.float64).reshape(npart, -1).sum(1)
    tile_err = np.max(np.abs(tile_sum - bits.sum(1)) / bits.sum(1))
    print("%dx%d: %d symbols, %.3f bits (%.4f per symbol); relative error: total %.3g, (tile, group) %.3g, map %.3g, "
          "map per tile %.3g" % (height, width, m, bits.sum(), bits.sum() / m, total_err, table_err, map_err, tile_err))
    # float64 sums of fewer than 1e5 terms of at most 16 bits; 1-ulp log2 differences stay below 1e-11
    assert total_err <= 1e-9
    assert table_err <= 1e-9
    assert map_err <= 1e-6
    assert (pmap[~live] == 0).all() and (~live).any()
    # every map entry is a non-negative float64 sum rounded once to float32 (relative error <= 2^-24), so the
    # float64 sum of a tile's entries is within 2^-24 of the tile's bits (+ the float64 summation error)
    assert tile_err <= 2.0 ** -24 + 1e-12


# ---- 2. the stream bracket against the engine's own streams --------------------------------------------------------

def _check_bracket(eng, x, what):
    streams = eng.encode(x)
    bits = eng.rate(x)
    sym = eng.symbols(x[:1])
    m = eng._engine("enc", sym.shape[2], sym.shape[3], 1).symbols_per_image
    per_frame = bits.reshape(bits.shape[0], -1).sum(1).cpu().numpy()
    assert np.isfinite(per_frame).all()
    gaps = []
    for i, s in enumerate(streams):
        gap, lo, hi = bracket(len(s), per_frame[i], m)
        gaps.append((gap, lo, hi))
        print("%s frame %d: %d symbols, %d bytes, %.3f bits in rows (%.4f per symbol), gap %.3f in [%.3f, %.3f]"
              % (what, i, m, len(s), per_frame[i], per_frame[i] / m, gap, lo, hi))
    for gap, lo, hi in gaps:
        assert lo <= gap <= hi
    return per_frame / m


@pytest.mark.parametrize("scale", [0.05, 0.3])
def test_stream_bracket_three_frames(scale, hip_backend):
    eng = _engine(56, scale)
    per_symbol = _check_bracket(eng, _frames(3, 256, 512, seed=5), "valid_dim 56, scale %g" % scale)
    assert (per_symbol > 0).all() and (per_symbol <= 16).all()


@pytest.mark.parametrize("vd", [112, 192])
def test_stream_bracket_matrix_core_forms(vd, hip_backend, monkeypatch):
    monkeypatch.delenv("PCONV_EE_BULK", raising=False)
    eng = _engine(vd)
    x = _frames(1, 256, 512, seed=vd)
    _check_bracket(eng, x, "valid_dim %d" % vd)
    sym = eng.symbols(x)
    assert eng._engine("enc", sym.shape[2], sym.shape[3], 1).encoder_forms[1:] == (FOUR_BLOCK,) * 11


# ---- 3. reproducibility --------------------------------------------------------------------------------------------

def test_rate_is_the_same_bits_alone_in_a_batch_and_on_every_run(hip_backend, monkeypatch):
    from pseudocylindrical_convolution_amd.engine import CodecEngine
    eng = _engine()
    x = _frames(3, 256, 512, seed=5)
    bits, pmap = eng.rate(x, rate_map=True)
    assert tuple(bits.shape) == (3, 16, 14) and tuple(pmap.shape) == (3, 32, 64)
    assert torch.isfinite(bits).all() and len({float(bits[i].sum()) for i in range(3)}) == 3
    for i in range(3):
        b1, m1 = eng.rate(x[i:i + 1], rate_map=True)
        assert torch.equal(b1[0], bits[i]) and torch.equal(m1[0], pmap[i])
    again, pmap_again = eng.rate(x, rate_map=True)
    assert torch.equal(again, bits) and torch.equal(pmap_again, pmap)
    assert torch.equal(eng.rate(x), bits)   # (without the map)
    monkeypatch.setattr(CodecEngine, "ENCODE_CHUNK", 1)
    one, pmap_one = eng.rate(x, rate_map=True)
    assert torch.equal(one, bits) and torch.equal(pmap_one, pmap)


# ---- 4. evaluate ---------------------------------------------------------------------------------------------------

def test_evaluate_is_rate_and_decode_of_encode(hip_backend):
    from pseudocylindrical_convolution_amd import rate
    eng = _engine()
    x = _frames(2, 256, 512, seed=9)
    bits, rec = eng.evaluate(x)
    assert torch.equal(rec, eng.decode(eng.encode(x), 256, 512))
    assert torch.equal(bits, eng.rate(x))
    b3, r3, m3 = eng.evaluate(x, rate_map=True)
    b2, m2 = eng.rate(x, rate_map=True)
    assert torch.equal(b3, bits) and torch.equal(r3, rec) and torch.equal(m3, m2) and torch.equal(b2, bits)
    # a size the codec does not take as it is: padded to 512x512, cropped back, the rate counts 300 x 500 pixels
    y = _frames(1, 300, 500, seed=11)
    ybits, yrec = eng.evaluate(y)
    assert tuple(yrec.shape) == (1, 3, 300, 500)
    ystreams = eng.encode(y)
    assert torch.equal(yrec, eng.decode(ystreams, 300, 500))
    assert torch.equal(ybits, eng.rate(y)) and tuple(ybits.shape) == (1, 16, 14)
    bpp = rate.bpp(ybits, 300, 500)
    assert bpp.is_cuda and bpp[0].item() == ybits.sum().item() / (300 * 500)
    m = eng._engine("enc", 4, 64, 1).symbols_per_image   # coded at 512x512: 4 symbol rows per tile, 64 columns
    gap, lo, hi = bracket(len(ystreams[0]), ybits.sum().item(), m)
    print("300x500: %.5f bpp from the rows, %.5f bpp in the stream, gap %.3f bits" %
          (bpp[0].item(), len(ystreams[0]) * 8 / 150000.0, gap))
    assert lo <= gap <= hi


# ---- 5. engine state -----------------------------------------------------------------------------------------------

def test_engine_codes_as_before_after_rate_and_refuses_rate_during_an_encode(hip_backend):
    from pseudocylindrical_convolution_amd._native import PconvError
    eng = _engine()
    x = _frames(2, 256, 512, seed=13)
    sym = eng.symbols(x).contiguous()
    e = eng._engine("enc", sym.shape[2], sym.shape[3], 2)
    before = e.encode(sym)
    bits = e.rate(sym)
    assert e.encode(sym) == before
    assert torch.equal(e.decode(before), sym)
    assert torch.equal(e.rate(sym), bits)
    e.encode_begin(sym)
    try:
        with pytest.raises(PconvError, match="has not been ended"):
            e.rate(sym)
    finally:
        pending = e.encode_end()
    assert pending == before
    assert torch.equal(e.rate(sym), bits)
    assert eng.encode(x) == before


# ---- 6. invalid label ----------------------------------------------------------------------------------------------

def test_an_invalid_label_makes_exactly_its_entries_nan(hip_backend):
    eng = _engine()
    x = _frames(2, 256, 512, seed=17)
    sym = eng.symbols(x).contiguous()
    h, w = sym.shape[2], sym.shape[3]
    e = eng._engine("enc", h, w, 2)
    good, good_map = e.rate(sym, rate_map=True)
    assert torch.isfinite(good).all() and torch.isfinite(good_map).all()
    frame, tile, group, row, col = 1, 5, 3, 1, 7
    assert good_map[frame, tile * h + row, col] > 0   # a live position
    bad = sym.clone()
    bad[frame * 16 + tile, group, row, col] = 9.0
    bits, pmap = e.rate(bad, rate_map=True)
    expect = torch.zeros_like(bits, dtype=torch.bool)
    expect[frame, tile, group] = True
    assert torch.equal(torch.isnan(bits), expect) and torch.isfinite(bits[~expect]).all()
    expect_map = torch.zeros_like(pmap, dtype=torch.bool)
    expect_map[frame, tile * h + row, col] = True
    assert torch.equal(torch.isnan(pmap), expect_map) and torch.isfinite(pmap[~expect_map]).all()
    assert torch.equal(bits[0], good[0]) and torch.equal(pmap[0], good_map[0])   # the other frame: untouched
    # the engine is none the worse for it
    gbits, gmap = e.rate(sym, rate_map=True)
    assert torch.equal(gbits, good) and torch.equal(gmap, good_map)


# ---- 7. --rd end to end --------------------------------------------------------------------------------------------

def test_cli_rd_against_enc_and_test(hip_backend, tmp_path, monkeypatch, capsys):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    from test_cli import _models, _write_png
    monkeypatch.chdir(tmp_path)
    _models(tmp_path, "cuda:0")
    H, W, m = 256, 512, 23408
    common = ["--ssim", "--model-idx", "3", "--height", str(H), "--width", str(W)]
    _write_png("img.png", H, W, 0)
    PC.main(["--enc", "--img-list", "img.png", "--code-list", "code.bin"] + common)
    PC.main(["--test", "--ws", "--img-list", "img.png", "--code-list", "code.bin"] + common)
    tested = capsys.readouterr().out
    rows = PC.rate_distortion(["img.png"], 3, False, 0, H, W, ws=True)
    capsys.readouterr()
    PC.main(["--rd", "--ws", "--img-list", "img.png"] + common)
    out = capsys.readouterr().out
    print(tested + out)
    line = re.search(r"Estimating img\.png \n Bitrate:([0-9.]+)bpp \(tables\), PSNR:([0-9.]+)dB, SSIM:([0-9.]+)", out)
    assert line, out
    # the returned rate is inside the bracket of the file --enc wrote; the printed one is that figure to three
    # decimals (a thousandth of a bpp is 131 bits at this size: the print cannot carry the bracket itself)
    nbytes = os.path.getsize("code.bin")
    gap, lo, hi = bracket(nbytes, rows[0][0] * H * W, m)
    print("--rd: %.6f bpp from the rows, file %d bytes (%.6f bpp), gap %.3f bits" % (rows[0][0], nbytes, nbytes * 8 / float(H * W), gap))
    assert lo <= gap <= hi
    assert line.group(1) == "%.3f" % rows[0][0]
    assert abs(float(line.group(1)) * H * W - 8 * nbytes) <= max(-lo, hi) + 0.0005 * H * W
    # distortion: the figures --test prints for that file, viewport and WS
    ref = re.search(r"Bitrate:[0-9.]+bpp, PSNR:([0-9.]+)dB, SSIM:([0-9.]+)\n WS-PSNR:([0-9.]+)dB, WS-SSIM:([0-9.]+)", tested)
    got = re.search(r"PSNR:([0-9.]+)dB, SSIM:([0-9.]+)\n WS-PSNR:([0-9.]+)dB, WS-SSIM:([0-9.]+)", out)
    assert ref and got and ref.groups() == got.groups()
    assert line.groups()[1:] == ref.groups()[:2]
    test_rows = PC.decoding_and_test(["code.bin"], ["img.png"], 3, False, 0, H, W, ws=True)
    assert tuple(rows[0][1:]) == tuple(test_rows[0][1:])
    assert "Average Performance" in out and len(rows[0]) == 5
    with pytest.raises(AssertionError):
        PC.main(["--rd", "--enc", "--img-list", "img.png", "--code-list", "code.bin"] + common)
