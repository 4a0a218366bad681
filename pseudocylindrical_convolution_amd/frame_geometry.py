"""One frame geometry: source -> (rotate) -> (resize) -> content size -> (pad) -> coded size, and the way back.

source is the picture the user holds; content what is coded before its padding (the container's height / width: the
source unless code_size / --code-size asks for another size); coded = erp_size.coded_size(content), what the transforms
and the entropy engine see.  rotation is the orientation the picture is coded in (erp_rotate.py: yaw, pitch, roll in
units of 2^-16 degree, or None).  The rules stay erp_rotate.py's (rotation, clamped to [0, 1]), erp_resample.py's
(resize, clamped to [0, 1]) and erp_size.py's (pole / seam pad, crop); this module only says which of them a frame
needs, for the engine, the file codec, the command line and the container header alike.  A step that is the identity
is not run: the tensor itself comes back.
"""
import collections

from . import erp_resample, erp_rotate, erp_size


class FrameGeometry(collections.namedtuple("FrameGeometry", "source content coded top resized padded rotation")):
    """immutable; sizes are (height, width), `top` rows of the coded frame lie above the content, resized = source and
    content differ, padded = content and coded differ, rotation = the integer triple of erp_rotate.units or None (all
    zeros count as None).  Sizes outside 2 .. 2^20 per side are erp_size.coded_size's ValueError, angles out of range
    erp_rotate.check's PconvError"""
    __slots__ = ()

    def __new__(cls, source, content=None, rotation=None):
        source = (int(source[0]), int(source[1]))
        content = source if content is None else (int(content[0]), int(content[1]))
        if source != content:
            erp_size.coded_size(*source)   # (only its range check)
        hc, wc, top = erp_size.coded_size(*content)
        return super(FrameGeometry, cls).__new__(cls, source, content, (hc, wc), top, source != content,
                                                 (hc, wc) != content, erp_rotate.check(rotation))

    @classmethod
    def for_raw(cls, height, width):
        """a headerless stream: the size comes from the caller and nothing was resized"""
        return cls((height, width))

    @classmethod
    def from_header(cls, head):
        """from the dict container.unpack / sniff / read return"""
        content = (head["height"], head["width"])
        return cls((head["source_height"], head["source_width"]) if "source_height" in head else content, content,
                   head.get("rotation"))

    def header_fields(self):
        """the size arguments of container.pack_any / write_any (which picks version 1, 2, 3 or 4 from them); the
        `rotation` key only when rotated"""
        fields = dict(height=self.content[0], width=self.content[1], source=self.source)
        if self.rotated:
            fields["rotation"] = self.rotation
        return fields

    @property
    def rotated(self):
        """the picture is coded in another orientation than the source's"""
        return self.rotation is not None

    @property
    def pixels(self):
        """what a bitrate is divided by: the source's pixels, whatever size was coded"""
        return self.source[0] * self.source[1]

    def to_coded(self, frames):
        """float32 (n, C, *source) -> (n, C, *coded)"""
        if self.rotated:
            frames = erp_rotate.rotate(frames, self.rotation, clamp=True)
        if self.resized:
            frames = erp_resample.resize(frames, self.content[0], self.content[1], clamp=True)
        return erp_size.pad(frames) if self.padded else frames

    def from_coded(self, rec, to_source=True):
        """(n, C, *coded) -> (n, C, *source); to_source=False stops at the content size, in the coded orientation (no
        resize back, no rotation back)"""
        if self.padded:
            rec = erp_size.crop(rec, *self.content)
        if self.resized and to_source:
            rec = erp_resample.resize(rec, self.source[0], self.source[1], clamp=True)
        if self.rotated and to_source:
            rec = erp_rotate.rotate(rec, self.rotation, inverse=True, clamp=True)
        return rec
