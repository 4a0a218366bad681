"""Rate without coding: the code length of a symbol from its integer CDF row (include/pconv_hip.h, pconv_ee_rate).

For a coded symbol let c[0..8] be the integer CDF row the engine hands to the coder (8 symbols, c[0] = 0,
c[8] = 65536) and s its label.  Its code length is 16 - log2(c[s+1] - c[s]) bits in float64.  A label outside 0 .. 7
or a row whose label has zero frequency -- what the coder refuses -- has no code length: NaN.

`row_bits` is the definition in numpy, the CPU mirror of the HIP kernel (csrc/entropy_engine.hip,
ee_rate_bulk_kernel) as erp_size.coded_size mirrors its C rule; `bpp` turns the kernel's (frame, tile, group) sums
into the rate of a frame.  EntropyEngine.rate / CodecEngine.rate / CodecEngine.evaluate (engine.py) run the kernel.
"""
import numpy as np

NSYMBOL = 8
TOTAL_BITS = 16   # rows sum to 65536 = 2^16


def row_bits(tables, labels):
    """int CDF rows (m, 9) and labels (m,) -> code lengths (m,) float64, NaN where the coder would refuse"""
    tables = np.asarray(tables).reshape(-1, NSYMBOL + 1).astype(np.int64)
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if tables.shape[0] != labels.shape[0]:
        raise ValueError("row_bits: %d rows for %d labels" % (tables.shape[0], labels.shape[0]))
    valid = (labels >= 0) & (labels < NSYMBOL)
    s = np.where(valid, labels, 0)
    idx = np.arange(labels.shape[0])
    freq = tables[idx, s + 1] - tables[idx, s]
    valid &= freq > 0
    out = np.full(labels.shape[0], np.nan, dtype=np.float64)
    out[valid] = TOTAL_BITS - np.log2(freq[valid].astype(np.float64))
    return out


def bpp(bits, height, width):
    """rate in bits per pixel of every frame of a `bits` tensor (n, npart, ngroup) -- torch or numpy -- for frames
    of height x width AS GIVEN (a frame coded at a padded size counts its own pixels, as pseudo_codec.bitrate does)"""
    return bits.reshape(bits.shape[0], -1).sum(1) / float(int(height) * int(width))
