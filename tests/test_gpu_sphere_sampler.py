"""GPU: the one sphere sampler (csrc/sphere_sampler.h) behind its three callers.  The sphere rotation (erp_remap_f32),
the viewport renderer at ss = 1 (viewport_render_f32) and the sphere points (sphere_points_sample_f32) read the same
records to the same bits, and those are the bits of the torch twin (erp_rotate.sample_torch) run on the CPU; the nearest
mode is held to its own twin, and one ss = 2 view to render_torch.

Records: the rotation map at pitch 90 degrees (both poles inside the frame) and at (30, 20, 10) degrees, and a hand-made
list of every pair of INT_MIN, INT_MAX, -1, 0, 255, 256, -256 and 256 w - 1 (64 records).  erp_remap_f32 takes a map
of the frame's own size, so a list of another length goes through it in pieces of h w records, the last padded.
Frames:
  (1, 1, 2, 2), (2, 3, 3, 5)   w < 6: taps coincide and the wrap runs more than once; odd w: the half turn is floored;
                                the pole rule and the clamp both act
  (1, 2, 6, 7)                  the footprint just fits
  (2, 3, 37, 70)                two 64-column tiles, h no multiple of the 4-row tile
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2, 2), (2, 3, 3, 5), (1, 2, 6, 7), (2, 3, 37, 70)]
RECORDS = ["pitch90", "rot30_20_10", "edges"]
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1

_cache = {}


def _frames(n, c, h, w):
    g = torch.Generator().manual_seed(977 * h + w)
    return torch.randint(0, 256, (n, c, h, w), generator=g).float() / 255. * 1.5 - 0.25   # some of it outside [0, 1]


def _edges(w):
    """int32 (64, 2): every pair of the eight edge values"""
    vals = torch.tensor([INT_MIN, INT_MAX, -1, 0, 255, 256, -256, 256 * w - 1], dtype=torch.int32)
    return torch.stack([vals.repeat_interleave(8), vals.repeat(8)], dim=1).contiguous()


def _records(kind, h, w):
    """the records of a case as a grid (a, b, 2), a and b >= 2, on the GPU, made once"""
    from pseudocylindrical_convolution_amd import PCONV, erp_rotate
    key = (kind, h, w)
    if key not in _cache:
        if kind == "edges":
            _cache[key] = _edges(w).view(8, 8, 2).cuda()
        else:
            angles = (0, 90, 0) if kind == "pitch90" else (30, 20, 10)
            _cache[key] = PCONV.erp_rotation_map(h, w, erp_rotate.units(*angles))
    return _cache[key]


def _twin(kind, shape, interp):
    """the CPU twin on the case's records, computed once: (n, C, a, b)"""
    from pseudocylindrical_convolution_amd import erp_rotate, sphere_points
    key = (kind, shape, interp)
    if key not in _cache:
        n, c, h, w = shape
        m = _records(kind, h, w).cpu()
        x = _frames(*shape)
        if interp == "lanczos":
            _cache[key] = erp_rotate.sample_torch(x, m)
        else:
            _cache[key] = sphere_points.sample_torch(x, m.view(-1, 2), "nearest").view(n, c, m.shape[0], m.shape[1])
    return _cache[key]


def _remap_in_pieces(x, m):
    """erp_remap_f32 at every record of the grid m: pieces of h w records, the last padded with the first records"""
    from pseudocylindrical_convolution_amd import PCONV
    n, c, h, w = x.shape
    flat = m.view(-1, 2)
    count = flat.shape[0]
    pieces = []
    for at in range(0, count, h * w):
        idx = torch.arange(at, at + h * w, device=flat.device) % count
        pieces.append(PCONV.erp_remap_f32(x, flat[idx].view(h, w, 2).contiguous()).view(n, c, h * w))
    return torch.cat(pieces, dim=2)[:, :, :count].reshape(n, c, m.shape[0], m.shape[1])


def _same(got, want, what):
    got = got.cpu()
    assert got.shape == want.shape, what
    diff = got.view(torch.int32) != want.view(torch.int32)
    assert not diff.any().item(), "%s: %d of %d values differ in bits, first at %s: %r vs %r" % (
        what, diff.sum(), diff.numel(), diff.nonzero()[:1].tolist(), got[diff][:1].tolist(), want[diff][:1].tolist())


@pytest.mark.parametrize("kind", RECORDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_three_callers_read_the_same_bits(hip_backend, shape, kind):
    from pseudocylindrical_convolution_amd import PCONV
    n, c, h, w = shape
    x = _frames(*shape).cuda()
    m = _records(kind, h, w)
    a, b = m.shape[:2]
    want = _twin(kind, shape, "lanczos")
    assert torch.isfinite(want).all()
    _same(_remap_in_pieces(x, m), want, "erp_remap_f32")
    _same(PCONV.viewport_render_f32(x, m, a, b, 1)[:, 0], want, "viewport_render_f32")
    _same(PCONV.sphere_points_sample_f32(x, m.view(-1, 2)).view(n, c, a, b), want, "sphere_points_sample_f32")
    _same(PCONV.sphere_points_sample_f32(x, m.view(-1, 2), "nearest").view(n, c, a, b), _twin(kind, shape, "nearest"),
          "sphere_points_sample_f32 nearest")


def test_two_by_two_records_of_edges_are_render_torch(hip_backend):
    from pseudocylindrical_convolution_amd import PCONV, viewport
    shape = (2, 3, 3, 5)
    x = _frames(*shape)
    m2 = _edges(5)[:60].view(6, 10, 2).contiguous()
    want = viewport.render_torch(x, m2, 3, 5, 2)
    _same(PCONV.viewport_render_f32(x.cuda(), m2.cuda(), 3, 5, 2)[:, 0], want, "viewport_render_f32 ss = 2")
