"""Rate without coding, the parts that need no GPU: rate.row_bits (the code-length definition of
include/pconv_hip.h in numpy float64) against streams the reference coder wrote, its NaN rule, rate.bpp, the
oracle per-op encoder's own file, and the command line's --rd exclusivity.

The stream bracket.  For a frame of m coded symbols, 8 * len(stream) - sum(code lengths) lies in
[-2 - m * 2^-13, 10 + m * 2^-13]: the 10 covers the final bit, byte padding and interval slack, the 2^-13 per
symbol the drift of the coder's integer range split (at most 1.44 / (2^14 f) bits per symbol for a 32-bit state and
total 65536)."""
import glob
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def bracket(stream_bytes, bits_sum, m):
    """(gap, lower bound, upper bound) of the stream bracket"""
    slack = m * 2.0 ** -13
    return 8 * stream_bytes - bits_sum, -2 - slack, 10 + slack


class RecordingCoder(object):
    """wraps an arithmetic coder module object (ent.mcoder): passes every call through and keeps the rows and
    labels of each encodes()"""

    def __init__(self, inner, on_step=None):
        self.inner, self.tables, self.labels, self.on_step = inner, [], [], on_step

    def encodes(self, table, ncode, symbols, num):
        assert ncode == 8
        self.tables.append(table.reshape(-1, 9)[:num].clone().numpy())
        self.labels.append(symbols.reshape(-1)[:num].clone().numpy())
        if self.on_step is not None:
            self.on_step(num)   # (once per wavefront step: keeps a second extractor in lock-step)
        return self.inner.encodes(table, ncode, symbols, num)

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def rows(self):
        return np.concatenate(self.tables, 0), np.concatenate(self.labels, 0)


def _stored_vectors():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLD, "coder_*.npz"))):
        d = np.load(path)
        out.append((os.path.basename(path), d["tables"], d["symbols"], d["stream"]))
    d = np.load(os.path.join(GOLD, "ref_coder_live.npz"))
    k = 0
    while "stream_%d" % k in d.files:
        out.append(("ref_coder_live[%d]" % k, d["tables_%d" % k], d["symbols_%d" % k], d["stream_%d" % k]))
        k += 1
    return out


def test_stored_reference_streams_are_inside_the_bracket():
    from pseudocylindrical_convolution_amd import rate
    cases = _stored_vectors()
    assert len(cases) >= 9
    for name, tables, symbols, stream in cases:
        bits = rate.row_bits(tables, symbols)
        assert bits.dtype == np.float64 and bits.shape == (len(symbols),) and np.isfinite(bits).all()
        gap, lo, hi = bracket(len(stream), bits.sum(), len(symbols))
        print("%s: %d symbols, %d bytes, gap %.3f bits" % (name, len(symbols), len(stream), gap))
        assert lo <= gap <= hi, "%s: gap %.3f outside [%.3f, %.3f]" % (name, gap, lo, hi)


def test_row_bits_values_and_nan_rule():
    from pseudocylindrical_convolution_amd import rate
    row = [0, 1, 3, 3, 1027, 32768, 65533, 65534, 65536]
    tables = np.array([row] * 10, dtype=np.int32)
    labels = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, -1], dtype=np.int32)
    bits = rate.row_bits(tables, labels)
    freq = np.diff(np.array(row, dtype=np.float64))
    for s in (0, 1, 3, 4, 5, 6, 7):
        assert bits[s] == 16.0 - np.log2(freq[s])
    assert bits[0] == 16.0 and bits[1] == 15.0 and bits[3] == 6.0 and bits[6] == 16.0 and bits[7] == 15.0
    assert np.isnan(bits[2])                        # zero-frequency label
    assert np.isnan(bits[8]) and np.isnan(bits[9])  # labels 8 and -1
    assert np.isfinite(bits[[0, 1, 3, 4, 5, 6, 7]]).all()
    assert rate.row_bits(np.zeros((0, 9), np.int32), np.zeros((0,), np.int32)).shape == (0,)
    with pytest.raises(ValueError):
        rate.row_bits(tables, labels[:3])


def test_bpp_arithmetic():
    from pseudocylindrical_convolution_amd import rate
    bits = torch.arange(2 * 16 * 14, dtype=torch.float64).reshape(2, 16, 14)
    out = rate.bpp(bits, 300, 500)
    assert out.dtype == torch.float64 and tuple(out.shape) == (2,)
    assert out[0].item() == float(sum(range(224))) / 150000.0
    assert out[1].item() == float(sum(range(224, 448))) / 150000.0
    assert np.array_equal(rate.bpp(bits.numpy(), 300, 500), out.numpy())
    nan = bits.clone()
    nan[1, 3, 5] = float("nan")
    got = rate.bpp(nan, 256, 512)
    assert torch.isfinite(got[0]) and torch.isnan(got[1])


def test_oracle_per_op_encoder_file_is_inside_the_bracket(oracle_backend, tmp_path):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC, rate
    torch.manual_seed(1234)
    enc = PC.PseudoEncoder(56, 0)
    g = torch.Generator().manual_seed(7)
    enc.ent.load_state_dict({k: torch.randn(v.shape, generator=g) * 0.05 for k, v in enc.ent.state_dict().items()})
    x = torch.rand(1, 3, 256, 512, generator=torch.Generator().manual_seed(1))
    path = str(tmp_path / "code.bin")
    sym = enc.symbols(x)
    enc.ent.start(path)
    rec = enc.ent.mcoder = RecordingCoder(enc.ent.mcoder)
    enc.ent(sym)
    tables, labels = rec.rows()
    m = 23408   # 14 groups x 2 rows x the valid widths of the 16 tiles at 64 columns
    assert tables.shape == (m, 9) and labels.shape == (m,)
    bits = rate.row_bits(tables, labels)
    assert np.isfinite(bits).all()
    gap, lo, hi = bracket(os.path.getsize(path), bits.sum(), m)
    print("oracle per-op encoder, 256x512, valid_dim 56: %.1f bits in rows, %d bytes, gap %.3f bits"
          % (bits.sum(), os.path.getsize(path), gap))
    assert lo <= gap <= hi


def test_rd_excludes_the_other_modes(tmp_path, monkeypatch):
    from pseudocylindrical_convolution_amd import pseudo_codec as PC
    monkeypatch.chdir(tmp_path)
    for other in (["--enc", "--code-list", "x.bin"], ["--dec", "--code-list", "x.bin", "--out-list", "x.png"],
                  ["--test", "--code-list", "x.bin"]):
        with pytest.raises(AssertionError, match="--rd excludes"):
            PC.main(["--rd", "--img-list", "x.png"] + other)
