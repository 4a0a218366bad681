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
import collections
import os
import struct

MAGIC = b"PCVC"
VERSION, VERSION_ANY, VERSION_SOURCE = 1, 2, 3
# per version: the struct format (magic, version, flags, model index, ngroup, sizes ..., payload length), what one
# count of the height / width fields stands for, and whether a source size follows them
_Layout = collections.namedtuple("_Layout", "fmt unit source")
_LAYOUT = {VERSION: _Layout("<4sBBBBHHI", 16, False),
           VERSION_ANY: _Layout("<4sBBBBIII", 1, False),
           VERSION_SOURCE: _Layout("<4sBBBBIIIII", 1, True)}
HEADER_BYTES, HEADER_BYTES_ANY, HEADER_BYTES_SOURCE = (struct.calcsize(_LAYOUT[v].fmt) for v in sorted(_LAYOUT))


class ContainerError(ValueError):
    pass


def _misfit(version, height, width, source, model_idx, valid_dim, nbytes):
    """why the fields do not fit a header of `version`, or None: the one check of pack, pack_any and _parse"""
    side = lambda v: 2 <= v <= 1 << 20
    if source is not None and not (side(source[0]) and side(source[1])):
        return "source size %dx%d does not fit the header (2 .. 2^20 per side)" % (source[1], source[0])
    if _LAYOUT[version].unit == 16:
        if height % 16 or width % 16 or not (0 < height // 16 < 65536 and 0 < width // 16 < 65536):
            return "ERP size %dx%d does not fit the header (multiples of 16, < 2^20)" % (width, height)
    elif not (side(height) and side(width)):
        return "ERP size %dx%d does not fit the header (2 .. 2^20 per side)" % (width, height)
    if valid_dim % 4 or not 0 < valid_dim // 4 < 256:
        return "valid_dim %d does not fit the header" % valid_dim
    if not 0 <= model_idx < 256:
        return "model index %d does not fit the header" % model_idx
    if nbytes >= 1 << 32:
        return "payload too long"
    return None


def _pack(version, payload, height, width, model_idx, ssim, valid_dim, source=None):
    why = _misfit(version, height, width, source, model_idx, valid_dim, len(payload))
    if why:
        raise ContainerError(why)
    layout = _LAYOUT[version]
    sizes = (height // layout.unit, width // layout.unit) + (tuple(source) if layout.source else ())
    return struct.pack(layout.fmt, MAGIC, version, 1 if ssim else 0, model_idx, valid_dim // 4, *sizes,
                       len(payload)) + bytes(payload)


def pack(payload, height, width, model_idx, ssim, valid_dim):
    """header + payload, version 1"""
    return _pack(VERSION, payload, height, width, model_idx, ssim, valid_dim)


def pack_any(payload, height, width, model_idx, ssim, valid_dim, source=None):
    """header + payload for an ERP of any size: `pack` (version 1) when the codec takes height x width as it
    is, else version 2 with the exact size (coded at erp_size.coded_size under the padding rule).
    source=(hs, ws) != (height, width): version 3, which also records the size the content was resized from"""
    from .erp_size import codable
    if source is not None:
        source = (int(source[0]), int(source[1]))
    if source is None or source == (height, width):
        return _pack(VERSION if codable(height, width) else VERSION_ANY, payload, height, width, model_idx, ssim,
                     valid_dim)
    return _pack(VERSION_SOURCE, payload, height, width, model_idx, ssim, valid_dim, source)


def _parse(head, size):
    """(fields dict, header bytes) of a header whose file (header + payload) is `size` bytes, or a reason string"""
    if len(head) < HEADER_BYTES:
        return "file shorter than the %d-byte header" % HEADER_BYTES
    if head[:4] != MAGIC:
        return "no container magic: a headerless reference-format stream?"
    version = head[4]
    if version not in _LAYOUT:
        return "container version %d, this build reads %d, %d and %d" % (version, VERSION, VERSION_ANY, VERSION_SOURCE)
    layout = _LAYOUT[version]
    nhead = struct.calcsize(layout.fmt)
    if len(head) < nhead:
        return "file shorter than the %d-byte version-%d header" % (nhead, version)
    _, _, flags, model_idx, ngroup, h, w, *source, n = struct.unpack(layout.fmt, head[:nhead])
    fields = {"height": h * layout.unit, "width": w * layout.unit, "model_idx": model_idx, "ssim": bool(flags & 1),
              "valid_dim": ngroup * 4}
    why = _misfit(version, fields["height"], fields["width"], source or None, model_idx, ngroup * 4, size - nhead)
    if why:
        return why
    if size - nhead != n:
        return "payload is %d bytes, header says %d" % (size - nhead, n)
    if source:
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
