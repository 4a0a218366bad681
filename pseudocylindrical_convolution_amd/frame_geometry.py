"""One frame geometry: (cube picture ->) source -> (rotate) -> (resize) -> content size -> (pad) -> coded size, and the
way back.

source is the picture the user holds; content what is coded before its padding (the container's height / width: the
source unless code_size / --code-size asks for another size); coded = erp_size.coded_size(content), what the transforms
and the entropy engine see.  rotation is the orientation the picture is coded in (erp_rotate.py: yaw, pitch, roll in
units of 2^-16 degree, or None).  The rules stay erp_rotate.py's (rotation, clamped to [0, 1]), erp_resample.py's
(resize, clamped to [0, 1]) and erp_size.py's (pole / seam pad, crop); this module only says which of them a frame
needs, for the engine, the file codec, the command line and the container header alike.  A step that is the identity
is not run: the tensor itself comes back.

projection is the cube.Spec of a picture that is a cubemap (cube.py: kind and layout), or None for an ERP picture.  The
source is then the ERP frame the codec sees, cube.erp_size(face size): the conversion cube -> ERP comes first on the way
in and ERP -> cube last on the way out, both clamped to [0, 1]; `picture` is the size of what the user holds.
"""
import collections

from . import cube, erp_resample, erp_rotate, erp_size
from ._native import PconvError


class FrameGeometry(collections.namedtuple("FrameGeometry", "source content coded top resized padded rotation projection")):
    """immutable; sizes are (height, width), `top` rows of the coded frame lie above the content, resized = source and
    content differ, padded = content and coded differ, rotation = the integer triple of erp_rotate.units or None (all
    zeros count as None), projection = the cube.Spec of a cube picture or None.  Sizes outside 2 .. 2^20 per side are
    erp_size.coded_size's ValueError, angles out of range erp_rotate.check's PconvError, a projection whose source is
    not cube.erp_size of a face size cube's PconvError"""
    __slots__ = ()

    def __new__(cls, source, content=None, rotation=None, projection=None):
        source = (int(source[0]), int(source[1]))
        if projection is not None:
            projection = cube.spec(projection)
            if source[1] % 4 or cube.erp_size(source[1] // 4) != source:
                raise PconvError("frame geometry: the ERP frame of a cube picture is 2a x 4a, a in 2 .. %d, not %dx%d"
                                 % (cube.MAX_FACE, source[1], source[0]))
        content = source if content is None else (int(content[0]), int(content[1]))
        if source != content:
            erp_size.coded_size(*source)   # (only its range check)
        hc, wc, top = erp_size.coded_size(*content)
        return super(FrameGeometry, cls).__new__(cls, source, content, (hc, wc), top, source != content,
                                                 (hc, wc) != content, erp_rotate.check(rotation), projection)

    @classmethod
    def for_picture(cls, size, content=None, rotation=None, projection=None):
        """from the size of the picture the user holds: an ERP frame, or with `projection` (a cube.Spec) a cube picture
        in its layout"""
        if projection is None:
            return cls(size, content, rotation)
        projection = cube.spec(projection)
        return cls(cube.erp_size(cube.face_size_of(size, projection.layout)), content, rotation, projection)

    @classmethod
    def for_raw(cls, height, width):
        """a headerless stream: the size comes from the caller and nothing was resized"""
        return cls((height, width))

    @classmethod
    def from_header(cls, head):
        """from the dict container.unpack / sniff / read return"""
        content = (head["height"], head["width"])
        source = (head["source_height"], head["source_width"]) if "source_height" in head else content
        projection = head.get("projection")
        if projection is not None:
            if cube.erp_size(projection[2]) != source:
                raise PconvError("frame geometry: a face size of %d does not go with a source of %dx%d"
                                 % (projection[2], source[1], source[0]))
            projection = cube.spec(*projection[:2])
        return cls(source, content, head.get("rotation"), projection)

    def header_fields(self):
        """the size arguments of container.pack_any / write_any (which picks version 1 to 5 from them); the
        `rotation` key only when rotated, the `projection` key only for a cube picture"""
        fields = dict(height=self.content[0], width=self.content[1], source=self.source)
        if self.rotated:
            fields["rotation"] = self.rotation
        if self.projected:
            fields["projection"] = (self.projection.kind, self.projection.layout, self.face)
        return fields

    @property
    def projected(self):
        """the picture is a cubemap"""
        return self.projection is not None

    @property
    def face(self):
        """the face size of a cube picture (None for an ERP picture)"""
        return self.source[1] // 4 if self.projected else None

    @property
    def picture(self):
        """the size of the picture the user holds: the source, or the cube picture in its layout"""
        return cube.picture_size(self.face, self.projection.layout) if self.projected else self.source

    @property
    def rotated(self):
        """the picture is coded in another orientation than the source's"""
        return self.rotation is not None

    @property
    def pixels(self):
        """what a bitrate is divided by: the pixels of the picture the user holds (the source's, or the cube picture's
        6 a^2), whatever size was coded"""
        return self.picture[0] * self.picture[1]

    def to_coded(self, frames):
        """float32 (n, C, *picture) -> (n, C, *coded)"""
        if self.projected:
            frames = cube.to_erp(frames, self.source, self.projection, clamp=True)
        if self.rotated:
            frames = erp_rotate.rotate(frames, self.rotation, clamp=True)
        if self.resized:
            frames = erp_resample.resize(frames, self.content[0], self.content[1], clamp=True)
        return erp_size.pad(frames) if self.padded else frames

    def from_coded(self, rec, to_source=True):
        """(n, C, *coded) -> (n, C, *picture); to_source=False stops at the content size, in the coded orientation (no
        resize back, no rotation back, no conversion back to a cube picture); to_source="erp" goes back to the source
        ERP frame and stops in front of the conversion"""
        if self.padded:
            rec = erp_size.crop(rec, *self.content)
        if self.resized and to_source:
            rec = erp_resample.resize(rec, self.source[0], self.source[1], clamp=True)
        if self.rotated and to_source:
            rec = erp_rotate.rotate(rec, self.rotation, inverse=True, clamp=True)
        if self.projected and to_source is True:
            rec = cube.from_erp(rec, self.face, self.projection, clamp=True)
        return rec
