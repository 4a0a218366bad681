"""One frame geometry: source size -> (resize) -> content size -> (pad) -> coded size, and the way back.

source is the picture the user holds; content what is coded before its padding (the container's height / width: the
source unless code_size / --code-size asks for another size); coded = erp_size.coded_size(content), what the transforms
and the entropy engine see.  The rules stay erp_resample.py's (resize, clamped to [0, 1]) and erp_size.py's (pole / seam
pad, crop); this module only says which of them a frame needs, for the engine, the file codec, the command line and the
container header alike.  A step that is the identity is not run: the tensor itself comes back.
"""
import collections

from . import erp_resample, erp_size


class FrameGeometry(collections.namedtuple("FrameGeometry", "source content coded top resized padded")):
    """immutable; sizes are (height, width), `top` rows of the coded frame lie above the content, resized = source and
    content differ, padded = content and coded differ.  Sizes outside 2 .. 2^20 per side are
    erp_size.coded_size's ValueError"""
    __slots__ = ()

    def __new__(cls, source, content=None):
        source = (int(source[0]), int(source[1]))
        content = source if content is None else (int(content[0]), int(content[1]))
        if source != content:
            erp_size.coded_size(*source)   # (only its range check)
        hc, wc, top = erp_size.coded_size(*content)
        return super(FrameGeometry, cls).__new__(cls, source, content, (hc, wc), top, source != content,
                                                 (hc, wc) != content)

    @classmethod
    def for_raw(cls, height, width):
        """a headerless stream: the size comes from the caller and nothing was resized"""
        return cls((height, width))

    @classmethod
    def from_header(cls, head):
        """from the dict container.unpack / sniff / read return"""
        content = (head["height"], head["width"])
        return cls((head["source_height"], head["source_width"]) if "source_height" in head else content, content)

    def header_fields(self):
        """the size arguments of container.pack_any / write_any (which picks version 1, 2 or 3 from them)"""
        return dict(height=self.content[0], width=self.content[1], source=self.source)

    @property
    def pixels(self):
        """what a bitrate is divided by: the source's pixels, whatever size was coded"""
        return self.source[0] * self.source[1]

    def to_coded(self, frames):
        """float32 (n, C, *source) -> (n, C, *coded)"""
        if self.resized:
            frames = erp_resample.resize(frames, self.content[0], self.content[1], clamp=True)
        return erp_size.pad(frames) if self.padded else frames

    def from_coded(self, rec, to_source=True):
        """(n, C, *coded) -> (n, C, *source); to_source=False stops at the content size (no resize back)"""
        if self.padded:
            rec = erp_size.crop(rec, *self.content)
        if self.resized and to_source:
            rec = erp_resample.resize(rec, self.source[0], self.source[1], clamp=True)
        return rec
