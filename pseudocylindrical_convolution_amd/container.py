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

Version 4 (40 bytes) carries, beside the two sizes, the orientation the picture was coded in (erp_rotate.py: --rotate):
yaw, pitch and roll in units of 2^-16 degree, in the ranges of the sphere-rotation SEI of HEVC / VVC (yaw and roll
-180*2^16 .. 180*2^16 - 1, pitch -90*2^16 .. 90*2^16); the decoder rotates its picture back last.  The source size is
always present and equals the size of the coded content when nothing was resized:

    0       4     magic  b"PCVC"
    4       1     version (4)
    5..7          flags, model index, ngroup as in version 1
    8       4     exact ERP height of the coded content, little endian
    12      4     exact ERP width of the coded content, little endian
    16      4     source height, little endian
    20      4     source width, little endian
    24      4     yaw, signed, little endian
    28      4     pitch, signed, little endian
    32      4     roll, signed, little endian
    36      4     payload length in bytes, little endian

Version 5 (48 bytes) carries a cube picture (cube.py: --projection): version 4's fields -- the sizes are those of the ERP
frame the codec saw, cube.erp_size(face size); the angles may all be zero -- followed by the projection:

    0..35         as in version 4
    36      1     kind: 1 CMP, 2 EAC
    37      1     layout of the cube picture: 0 faces (6a x a), 1 6x1, 2 3x2
    38      2     zero
    40      4     face size a, little endian
    44      4     payload length in bytes, little endian

`pack` writes version 1 only; `pack_any` writes version 1 (the same bytes as `pack`) for a codable size and
version 2 otherwise, version 3 only when `source=(hs, ws)` is given and differs from (height, width), and version 4
only when `rotation=(yaw, pitch, roll)` is given and not all zeros, and version 5 only when `projection=(kind, layout,
face size)` is given.
`unpack`, `sniff` and `read` take all five and return the same dict: height / width are the size of the coded
content before its padding; a version-3 header adds source_height / source_width, a version-4 header adds them only
where they differ from height / width, and `rotation`, the integer triple; a version-5 header adds `projection`, the
triple (kind, layout, face size) with the names of cube.py ("cmp" / "eac"; "faces" / "6x1" / "3x2"), and `rotation` only
when it is not all zeros.

The command line writes the reference's headerless files unless `--container` is given;
decoding recognises a container by `sniff` (magic, version and a payload length that
matches the file), so headerless files produced by the reference decode as before.
"""
import collections
import operator
import os
import struct

MAGIC = b"PCVC"
VERSION, VERSION_ANY, VERSION_SOURCE, VERSION_ROTATED, VERSION_PROJECTED = 1, 2, 3, 4, 5
# per version: the struct format (magic, version, flags, model index, ngroup, sizes ..., [angles,] [projection,] payload
# length), what one count of the height / width fields stands for, whether a source size follows them, whether three
# angles follow that, and whether the projection (kind, layout, zero, face size) follows those
_Layout = collections.namedtuple("_Layout", "fmt unit source rotation projection")
_LAYOUT = {VERSION: _Layout("<4sBBBBHHI", 16, False, False, False),
           VERSION_ANY: _Layout("<4sBBBBIII", 1, False, False, False),
           VERSION_SOURCE: _Layout("<4sBBBBIIIII", 1, True, False, False),
           VERSION_ROTATED: _Layout("<4sBBBBIIIIiiiI", 1, True, True, False),
           VERSION_PROJECTED: _Layout("<4sBBBBIIIIiiiBBHII", 1, True, True, True)}
HEADER_BYTES, HEADER_BYTES_ANY, HEADER_BYTES_SOURCE, HEADER_BYTES_ROTATED, HEADER_BYTES_PROJECTED = \
    (struct.calcsize(_LAYOUT[v].fmt) for v in sorted(_LAYOUT))
HEADER_BYTES_MAX = max(struct.calcsize(layout.fmt) for layout in _LAYOUT.values())   # what sniff has to read
PROJECTION_KINDS = {1: "cmp", 2: "eac"}                  # cube.KINDS, by code
PROJECTION_LAYOUTS = {0: "faces", 1: "6x1", 2: "3x2"}    # cube.LAYOUTS, by code
PROJECTION_MAX_FACE = 9453                               # cube.MAX_FACE
_ANGLES = (("yaw", -180 << 16, (180 << 16) - 1), ("pitch", -90 << 16, 90 << 16), ("roll", -180 << 16, (180 << 16) - 1))


class ContainerError(ValueError):
    pass


def _projection_codes(projection):
    """(kind code, layout code, zero, face size) of (kind, layout, face size), names or codes; unknown names stay as
    they are for _misfit to name"""
    try:
        kind, layout, face = projection
    except (TypeError, ValueError):
        raise ContainerError("projection must be (kind, layout, face size), got %r" % (projection,))
    kind = {v: k for k, v in PROJECTION_KINDS.items()}.get(kind, kind)
    layout = {v: k for k, v in PROJECTION_LAYOUTS.items()}.get(layout, layout)
    try:
        face = operator.index(face)
    except TypeError:
        pass
    return kind, layout, 0, face


def _misfit(version, height, width, source, model_idx, valid_dim, nbytes, rotation=None, projection=None):
    """why the fields do not fit a header of `version`, or None: the one check of pack, pack_any and _parse"""
    side = lambda v: 2 <= v <= 1 << 20
    if projection is not None:
        kind, layout, zero, face = projection
        if kind not in PROJECTION_KINDS:
            return "projection kind %r is none of %s" % (kind, sorted(PROJECTION_KINDS.items()))
        if layout not in PROJECTION_LAYOUTS:
            return "projection layout %r is none of %s" % (layout, sorted(PROJECTION_LAYOUTS.items()))
        if zero != 0:
            return "the projection's reserved bytes are %r, not zero" % (zero,)
        if not isinstance(face, int) or not 2 <= face <= PROJECTION_MAX_FACE:
            return "projection face size %r is outside 2 .. %d" % (face, PROJECTION_MAX_FACE)
        if source is not None and tuple(source) != (2 * face, 4 * face):
            return "projection face size %d does not go with a source of %dx%d (the ERP frame of a cube picture is %dx%d)" \
                % (face, source[1], source[0], 4 * face, 2 * face)
    if rotation is not None:
        for (name, lo, hi), v in zip(_ANGLES, rotation):
            if not lo <= v <= hi:
                return "%s %d does not fit the header (%d .. %d, units of 2^-16 degree)" % (name, v, lo, hi)
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


def _pack(version, payload, height, width, model_idx, ssim, valid_dim, source=None, rotation=None, projection=None):
    why = _misfit(version, height, width, source, model_idx, valid_dim, len(payload), rotation, projection)
    if why:
        raise ContainerError(why)
    layout = _LAYOUT[version]
    sizes = (height // layout.unit, width // layout.unit) + (tuple(source) if layout.source else ()) + \
        (tuple(rotation) if layout.rotation else ()) + (tuple(projection) if layout.projection else ())
    return struct.pack(layout.fmt, MAGIC, version, 1 if ssim else 0, model_idx, valid_dim // 4, *sizes,
                       len(payload)) + bytes(payload)


def pack(payload, height, width, model_idx, ssim, valid_dim):
    """header + payload, version 1"""
    return _pack(VERSION, payload, height, width, model_idx, ssim, valid_dim)


def pack_any(payload, height, width, model_idx, ssim, valid_dim, source=None, rotation=None, projection=None):
    """header + payload for an ERP of any size: `pack` (version 1) when the codec takes height x width as it
    is, else version 2 with the exact size (coded at erp_size.coded_size under the padding rule).
    source=(hs, ws) != (height, width): version 3, which also records the size the content was resized from.
    rotation=(yaw, pitch, roll) in units of 2^-16 degree, not all zeros: version 4, which records the orientation
    as well (and always a source size); None or zeros: the bytes of versions 1 to 3.
    projection=(kind, layout, face size) of a cube picture (cube.py): version 5, whatever the other fields are; the
    source size must be cube.erp_size(face size).  None: the bytes of versions 1 to 4"""
    from .erp_size import codable
    if source is not None:
        source = (int(source[0]), int(source[1]))
    if rotation is not None:
        try:
            rotation = tuple(int(v) for v in rotation)
            if len(rotation) != 3:
                raise ValueError
        except (TypeError, ValueError):
            raise ContainerError("rotation must be three integers (yaw, pitch, roll) in units of 2^-16 degree")
    if projection is not None:
        return _pack(VERSION_PROJECTED, payload, height, width, model_idx, ssim, valid_dim,
                     (height, width) if source is None else source, rotation or (0, 0, 0), _projection_codes(projection))
    if rotation is not None and any(rotation):
        return _pack(VERSION_ROTATED, payload, height, width, model_idx, ssim, valid_dim,
                     (height, width) if source is None else source, rotation)
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
        return "container version %d, this build reads %s" % (version, ", ".join(str(v) for v in sorted(_LAYOUT)))
    layout = _LAYOUT[version]
    nhead = struct.calcsize(layout.fmt)
    if len(head) < nhead:
        return "file shorter than the %d-byte version-%d header" % (nhead, version)
    _, _, flags, model_idx, ngroup, h, w, *more, n = struct.unpack(layout.fmt, head[:nhead])
    source, rotation, projection = tuple(more[:2]), tuple(more[2:5]), tuple(more[5:])
    fields = {"height": h * layout.unit, "width": w * layout.unit, "model_idx": model_idx, "ssim": bool(flags & 1),
              "valid_dim": ngroup * 4}
    why = _misfit(version, fields["height"], fields["width"], source or None, model_idx, ngroup * 4, size - nhead,
                  rotation or None, projection or None)
    if why:
        return why
    if size - nhead != n:
        return "payload is %d bytes, header says %d" % (size - nhead, n)
    if source and (not layout.rotation or source != (fields["height"], fields["width"])):
        fields["source_height"], fields["source_width"] = source
    if rotation and (not layout.projection or any(rotation)):
        fields["rotation"] = rotation
    if projection:
        fields["projection"] = (PROJECTION_KINDS[projection[0]], PROJECTION_LAYOUTS[projection[1]], projection[3])
    return fields, nhead


def unpack(data):
    """-> (dict(height, width, model_idx, ssim, valid_dim[, source_height, source_width][, rotation][, projection]),
    payload bytes); version 1, 2, 3, 4 or 5"""
    got = _parse(bytes(data[:HEADER_BYTES_MAX]), len(data))
    if isinstance(got, str):
        raise ContainerError(got)
    head, nhead = got
    return head, bytes(data[nhead:])


def _sniff(path):
    try:
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(HEADER_BYTES_MAX)
    except OSError:
        return "unreadable"
    return _parse(head, size)


def sniff(path):
    """header dict when the file is a well-formed container (version 1 to 5), else None (a headerless stream).
    A raw arithmetic-coded stream passes for a container only if its first bytes happen to spell the magic,
    a version and its own length: 2^-72 for random bytes."""
    got = _sniff(path)
    return None if isinstance(got, str) else got[0]


def header_bytes(path):
    """16, 20, 28, 40 or 48 when `path` is a well-formed container, else 0"""
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
