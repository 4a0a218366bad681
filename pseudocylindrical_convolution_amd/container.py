"""Bitstream container of the codec files.

The reference writes the raw arithmetic-coder bytes and nothing else
(coder/coder.h:20-24), so a file cannot be decoded without knowing the image
size, the model and its valid_dim out of band (pseudo_codec.py:206,209,229-234
hard-code them).  This container puts a 16-byte header in front of the same
payload -- the payload itself is byte for byte the reference-format stream:

    offset  size  field
    0       4     magic  b"PCVC"
    4       1     version (1)
    5       1     flags: bit 0 = model from the VSSIM list (--ssim), else VMSE
    6       1     model index inside its list
    7       1     ngroup = valid_dim / 4   (14, 28 or 48)
    8       2     ERP height / 16, little endian
    10      2     ERP width / 16, little endian
    12      4     payload length in bytes, little endian

Version 2 (20 bytes) carries an ERP size the codec does not take as it is -- any h x w, coded at
erp_size.coded_size(h, w) under the pole / seam padding rule of erp_size.py, the decoder crops back:

    0       4     magic  b"PCVC"
    4       1     version (2)
    5..7          flags, model index, ngroup as in version 1
    8       4     exact ERP height, little endian
    12      4     exact ERP width, little endian
    16      4     payload length in bytes, little endian

Version 3 (28 bytes) carries, beside the size of the coded content, the size of the source the content was resized
from (erp_resample.py: --code-size); the decoder resizes its picture back to it:

    0       4     magic  b"PCVC"
    4       1     version (3)
    5..7          flags, model index, ngroup as in version 1
    8       4     exact ERP height of the coded content, little endian
    12      4     exact ERP width of the coded content, little endian
    16      4     source height, little endian
    20      4     source width, little endian
    24      4     payload length in bytes, little endian

`pack` writes version 1 only; `pack_any` writes version 1 (the same bytes as `pack`) for a codable size and
version 2 otherwise, and version 3 only when `source=(hs, ws)` is given and differs from (height, width).
`unpack`, `sniff` and `read` take all three and return the same dict: height / width are the size of the coded
content before its padding; a version-3 header adds source_height / source_width.

The command line writes the reference's headerless files unless `--container` is given;
decoding recognises a container by `sniff` (magic, version and a payload length that
matches the file), so headerless files produced by the reference decode as before.
"""
import os
import struct

MAGIC = b"PCVC"
VERSION = 1
HEADER_BYTES = 16
_FMT = "<4sBBBBHHI"
VERSION_ANY = 2
HEADER_BYTES_ANY = 20
_FMT_ANY = "<4sBBBBIII"
VERSION_SOURCE = 3
HEADER_BYTES_SOURCE = 28
_FMT_SOURCE = "<4sBBBBIIIII"


class ContainerError(ValueError):
    pass


def pack(payload, height, width, model_idx, ssim, valid_dim):
    """header + payload"""
    if height % 16 or width % 16 or not (0 < height // 16 < 65536 and 0 < width // 16 < 65536):
        raise ContainerError("ERP size %dx%d does not fit the header (multiples of 16, < 2^20)" % (width, height))
    if valid_dim % 4 or not 0 < valid_dim // 4 < 256:
        raise ContainerError("valid_dim %d does not fit the header" % valid_dim)
    if not 0 <= model_idx < 256:
        raise ContainerError("model index %d does not fit the header" % model_idx)
    if len(payload) >= 1 << 32:
        raise ContainerError("payload too long")
    head = struct.pack(_FMT, MAGIC, VERSION, 1 if ssim else 0, model_idx, valid_dim // 4, height // 16, width // 16,
                       len(payload))
    return head + bytes(payload)


def pack_any(payload, height, width, model_idx, ssim, valid_dim, source=None):
    """header + payload for an ERP of any size: `pack` (version 1) when the codec takes height x width as it
    is, else version 2 with the exact size (coded at erp_size.coded_size under the padding rule).
    source=(hs, ws) != (height, width): version 3, which also records the size the content was resized from"""
    from .erp_size import codable
    if source is not None and (int(source[0]), int(source[1])) == (height, width):
        source = None
    if source is None and codable(height, width):
        return pack(payload, height, width, model_idx, ssim, valid_dim)
    if source is not None and not (2 <= int(source[0]) <= 1 << 20 and 2 <= int(source[1]) <= 1 << 20):
        raise ContainerError("source size %dx%d does not fit the header (2 .. 2^20 per side)" % (source[1], source[0]))
    if not (2 <= height <= 1 << 20 and 2 <= width <= 1 << 20):
        raise ContainerError("ERP size %dx%d does not fit the header (2 .. 2^20 per side)" % (width, height))
    if valid_dim % 4 or not 0 < valid_dim // 4 < 256:
        raise ContainerError("valid_dim %d does not fit the header" % valid_dim)
    if not 0 <= model_idx < 256:
        raise ContainerError("model index %d does not fit the header" % model_idx)
    if len(payload) >= 1 << 32:
        raise ContainerError("payload too long")
    if source is not None:
        head = struct.pack(_FMT_SOURCE, MAGIC, VERSION_SOURCE, 1 if ssim else 0, model_idx, valid_dim // 4, height,
                           width, int(source[0]), int(source[1]), len(payload))
        return head + bytes(payload)
    head = struct.pack(_FMT_ANY, MAGIC, VERSION_ANY, 1 if ssim else 0, model_idx, valid_dim // 4, height, width,
                       len(payload))
    return head + bytes(payload)


def _parse(head, size):
    """(fields dict, header bytes) of a header whose file (header + payload) is `size` bytes, or a reason string"""
    if len(head) < HEADER_BYTES:
        return "file shorter than the %d-byte header" % HEADER_BYTES
    if head[:4] != MAGIC:
        return "no container magic: a headerless reference-format stream?"
    version = head[4]
    source = None
    if version == VERSION:
        magic, version, flags, model_idx, ngroup, h16, w16, n = struct.unpack(_FMT, head[:HEADER_BYTES])
        nhead, height, width = HEADER_BYTES, h16 * 16, w16 * 16
    elif version == VERSION_ANY:
        if len(head) < HEADER_BYTES_ANY:
            return "file shorter than the %d-byte version-2 header" % HEADER_BYTES_ANY
        magic, version, flags, model_idx, ngroup, height, width, n = struct.unpack(_FMT_ANY, head[:HEADER_BYTES_ANY])
        nhead = HEADER_BYTES_ANY
        if not (2 <= height <= 1 << 20 and 2 <= width <= 1 << 20):
            return "ERP size %dx%d in the header is out of range" % (width, height)
    elif version == VERSION_SOURCE:
        if len(head) < HEADER_BYTES_SOURCE:
            return "file shorter than the %d-byte version-3 header" % HEADER_BYTES_SOURCE
        magic, version, flags, model_idx, ngroup, height, width, hs, ws, n = struct.unpack(
            _FMT_SOURCE, head[:HEADER_BYTES_SOURCE])
        nhead = HEADER_BYTES_SOURCE
        if not (2 <= height <= 1 << 20 and 2 <= width <= 1 << 20):
            return "ERP size %dx%d in the header is out of range" % (width, height)
        if not (2 <= hs <= 1 << 20 and 2 <= ws <= 1 << 20):
            return "source size %dx%d in the header is out of range" % (ws, hs)
        source = (hs, ws)
    else:
        return "container version %d, this build reads %d, %d and %d" % (version, VERSION, VERSION_ANY, VERSION_SOURCE)
    if size - nhead != n:
        return "payload is %d bytes, header says %d" % (size - nhead, n)
    if not (height and width and ngroup):
        return "empty field in the header"
    fields = {"height": height, "width": width, "model_idx": model_idx, "ssim": bool(flags & 1),
              "valid_dim": ngroup * 4}
    if source is not None:
        fields["source_height"], fields["source_width"] = source
    return fields, nhead


def unpack(data):
    """-> (dict(height, width, model_idx, ssim, valid_dim[, source_height, source_width]), payload bytes);
    version 1, 2 or 3"""
    got = _parse(bytes(data[:HEADER_BYTES_SOURCE]), len(data))
    if isinstance(got, str):
        raise ContainerError(got)
    head, nhead = got
    return head, bytes(data[nhead:])


def _sniff(path):
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(HEADER_BYTES_SOURCE)
    except OSError:
        return "unreadable"
    return _parse(head, size)


def sniff(path):
    """header dict when the file is a well-formed container (version 1, 2 or 3), else None (a headerless stream).
    A raw arithmetic-coded stream passes for a container only if its first bytes happen to spell the magic,
    a version and its own length: 2^-72 for random bytes."""
    got = _sniff(path)
    return None if isinstance(got, str) else got[0]


def header_bytes(path):
    """16, 20 or 28 when `path` is a well-formed container, else 0"""
    got = _sniff(path)
    return 0 if isinstance(got, str) else got[1]


def read(path):
    with open(path, "rb") as f:
        return unpack(f.read())


def write(path, payload, **fields):
    with open(path, "wb") as f:
        f.write(pack(payload, **fields))


def write_any(path, payload, **fields):
    with open(path, "wb") as f:
        f.write(pack_any(payload, **fields))
