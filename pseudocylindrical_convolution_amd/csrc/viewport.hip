// Rectilinear viewports of ERP frames (the definition is in include/pconv_hip.h, pconv_viewport_map /
// pconv_viewport_render_f32): float32 (n, C, h, w) -> n frames of (C, vh, vw), the gnomonic view of the sphere in a given
// orientation and field of view, ss x ss samples averaged per pixel.  Split like the sphere rotation (erp_rotate.hip):
//   viewport_map_kernel         one lane per grid sample: its direction (1, a, b), the rotation and the two tangents
//                               (eleven doubles, kernel arguments), two atan2 -- all in fp64 -- and the record (qu, qv)
//                               in 1/256 pixel of the source, one 8-byte store.
//   viewport_render_f32_kernel  a workgroup takes a tile of kTileH rows x kTileW columns of the VIEW; a lane owns one
//                               pixel.  Loop order: planes outermost, then the pixel's ss x ss records (p outer, t
//                               inner), then the 6 x 6 footprint: one accumulator whatever C is, and a plane's pixel is
//                               finished -- scaled, clamped, stored -- before the next plane begins.  The records are
//                               read again for every plane (8 bytes beside the 144 of the footprint they address, from
//                               L1 / L2: neighbouring lanes read neighbouring runs of ss records) and are NOT staged in
//                               LDS: at ss = 4 a tile's records are 32 KB, which would hold a CU to four workgroups for
//                               one load in 37.  The phase table (6 KB) is in LDS, staged by the workgroup.
// The renderer reduces every record to a position inside the frame (columns modulo w, rows by the pole rule and the
// clamp), so no map content makes it read outside `in`; each lane stores only its own pixel.
#include <math.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPhases = PCONV_ERP_ROTATE_PHASES;
constexpr int kTaps = PCONV_ERP_ROTATE_TAPS;
constexpr int kTileW = 64, kTileH = kBlock / kTileW;  // the renderer's tile: one wave per row
constexpr double kPi = 3.14159265358979323846;

struct Basis {
  double m[9], tx, ty;
};

__global__ __launch_bounds__(kBlock) void viewport_map_kernel(Basis B, int2 *__restrict__ map, int h, int w, int gh,
                                                              int gw, int tiles) {
  const int r = blockIdx.x / tiles;
  const int q = (blockIdx.x - r * tiles) * kBlock + threadIdx.x;
  if (q >= gw) return;
  const double a = (2.0 * (q + 0.5) / gw - 1.0) * B.tx;
  const double b = (1.0 - 2.0 * (r + 0.5) / gh) * B.ty;
  const double sx = B.m[0] + B.m[1] * a + B.m[2] * b;
  const double sy = B.m[3] + B.m[4] * a + B.m[5] * b;
  const double sz = B.m[6] + B.m[7] * a + B.m[8] * b;
  const double u = (atan2(sy, sx) / (2.0 * kPi) + 0.5) * w - 0.5;
  const double v = (0.5 - atan2(sz, hypot(sx, sy)) / kPi) * h - 0.5;
  const long long period = (long long)w * kPhases;
  long long qu = (long long)rint(u * kPhases) % period;  // |u| < w + 1: the conversion is exact
  if (qu < 0) qu += period;
  const int qv = (int)rint(v * kPhases);
  map[(long long)r * gw + q] = make_int2((int)qu, qv);
}

// one sample of the sampler of erp_remap_f32_kernel: the 6 x 6 footprint of `rec` on the plane `src`
__device__ __forceinline__ float sample(const float *__restrict__ src, int2 rec, const float *table, int h, int w) {
  // floor division and the non-negative remainder by 256, for a negative qv as well (two's complement)
  const int row0 = (rec.y >> 8) - 2;
  const float *wx = table + (rec.x & (kPhases - 1)) * kTaps;
  const float *wy = table + (rec.y & (kPhases - 1)) * kTaps;
  const int half = w / 2;
  float fx[kTaps], fy[kTaps];
  unsigned col[kTaps], turned[kTaps], row[kTaps];
  bool crossed[kTaps];
  int cb = ((rec.x >> 8) - 2) % w;  // the one division: the following columns wrap by comparison
  if (cb < 0) cb += w;
#pragma unroll
  for (int b = 0; b < kTaps; b++) {
    fx[b] = wx[b];
    fy[b] = wy[b];
    col[b] = cb;
    turned[b] = cb + half >= w ? cb + half - w : cb + half;
    cb = cb + 1 == w ? 0 : cb + 1;
    int r = row0 + b;
    crossed[b] = r < 0 || r >= h;
    if (r < 0) r = -1 - r;
    else if (r >= h) r = 2 * h - 1 - r;
    row[b] = min(max(r, 0), h - 1) * w;
  }
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < kTaps; a++) {
    // (src is the same for every lane: unsigned 32-bit offsets from it, not 36 addresses of 64 bits)
    float s = __fmul_rn(fx[0], src[row[a] + (crossed[a] ? turned[0] : col[0])]);
#pragma unroll
    for (int b = 1; b < kTaps; b++) s = __fadd_rn(s, __fmul_rn(fx[b], src[row[a] + (crossed[a] ? turned[b] : col[b])]));
    const float m = __fmul_rn(fy[a], s);
    acc = a == 0 ? m : __fadd_rn(acc, m);
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void viewport_render_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                     const int2 *__restrict__ map,
                                                                     const float *__restrict__ phases, int C, int h, int w,
                                                                     int vh, int vw, int ss, int tiles,
                                                                     long long out_frame_stride, float scale, int clamp) {
  __shared__ float table[kPhases * kTaps];
  for (int k = threadIdx.x; k < kPhases * kTaps; k += kBlock) table[k] = phases[k];
  __syncthreads();
  const int ty = blockIdx.x / tiles;
  const int i = (blockIdx.x - ty * tiles) * kTileW + (threadIdx.x % kTileW);
  const int j = ty * kTileH + threadIdx.x / kTileW;
  if (i >= vw || j >= vh) return;
  const int gw = vw * ss;                                // the map is below 2^31 bytes: below 2^28 records
  const int2 *recs = map + ((j * ss) * gw + i * ss);     // the pixel's first record: sample (j*ss, i*ss)
  const long long plane = (long long)h * w, vplane = (long long)vh * vw;
  const float *src = in + (long long)blockIdx.y * C * plane;
  float *dst = out + (long long)blockIdx.y * out_frame_stride + (j * vw + i);
  for (int c = 0; c < C; c++, src += plane, dst += vplane) {
    float acc = 0.f;
    for (int p = 0; p < ss; p++)
      for (int t = 0; t < ss; t++) {
        const float s = sample(src, recs[p * gw + t], table, h, w);
        acc = (p | t) == 0 ? s : __fadd_rn(acc, s);
      }
    if (ss > 1) acc = __fmul_rn(acc, scale);
    if (clamp) acc = fminf(fmaxf(acc, 0.f), 1.f);
    *dst = acc;
  }
}

int fov_ok(const char *what, int hfov, int vfov) {
  const int lo = 1 << 16, hi = 170 << 16;
  PCONV_REQUIRE(hfov >= lo && hfov <= hi && vfov >= lo && vfov <= hi,
                "%s: field of view (%d, %d) out of range: hfov and vfov 1*2^16 .. 170*2^16", what, hfov, vfov);
  return PCONV_OK;
}

int source_ok(const char *what, int h, int w) {
  PCONV_REQUIRE(h >= 2 && w >= 2 && h <= (1 << 20) && w <= (1 << 20), "%s: a source side of %dx%d is outside 2 .. 2^20", what,
                w, h);
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a source plane of %dx%d float32 is 2^31 bytes or more", what, w, h);
  return PCONV_OK;
}

}  // namespace

extern "C" int pconv_host_viewport_basis(int yaw, int pitch, int roll, int hfov, int vfov, double *out) {
  PCONV_REQUIRE(out, "host_viewport_basis: null pointer");
  if (fov_ok("host_viewport_basis", hfov, vfov) != PCONV_OK) return PCONV_EINVAL;
  if (pconv_host_erp_rotation_matrix(yaw, pitch, roll, 0, out) != PCONV_OK) return PCONV_EINVAL;  // angles out of range
  const double half_unit = kPi / 180.0 / 65536.0 / 2.0;
  out[9] = tan(hfov * half_unit);
  out[10] = tan(vfov * half_unit);
  return PCONV_OK;
}

extern "C" int pconv_viewport_map(int32_t *map, int h, int w, int gh, int gw, int yaw, int pitch, int roll, int hfov,
                                  int vfov, void *stream) {
  PCONV_REQUIRE(map, "viewport_map: null pointer");
  if (source_ok("viewport_map", h, w) != PCONV_OK) return PCONV_EINVAL;
  const int side = PCONV_VIEWPORT_MAX_SS << 20;
  PCONV_REQUIRE(gh >= 2 && gw >= 2 && gh <= side && gw <= side, "viewport_map: a grid side of %dx%d is outside 2 .. %d * 2^20",
                gw, gh, PCONV_VIEWPORT_MAX_SS);
  PCONV_REQUIRE(8LL * gh * gw < (1LL << 31), "viewport_map: a map of %dx%d records is 2^31 bytes or more", gw, gh);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(map) & 7) == 0, "viewport_map: the map must be 8-byte aligned");
  Basis B;
  double basis[11];
  if (pconv_host_viewport_basis(yaw, pitch, roll, hfov, vfov, basis) != PCONV_OK) return PCONV_EINVAL;
  for (int k = 0; k < 9; k++) B.m[k] = basis[k];
  B.tx = basis[9];
  B.ty = basis[10];
  const int tiles = (gw + kBlock - 1) / kBlock;  // gh * tiles < 2^28 / 256 + 2^22
  hipLaunchKernelGGL(viewport_map_kernel, dim3((unsigned)gh * tiles), dim3(kBlock), 0, as_stream(stream), B,
                     reinterpret_cast<int2 *>(map), h, w, gh, gw, tiles);
  PCONV_LAUNCH_CHECK("viewport_map");
  return PCONV_OK;
}

extern "C" int pconv_viewport_render_f32(const float *in, float *out, const int32_t *map, const float *phases, int n, int c,
                                         int h, int w, int vh, int vw, int ss, long long out_frame_stride, int clamp,
                                         void *stream) {
  PCONV_REQUIRE(in && out && map && phases, "viewport_render_f32: null pointer");
  PCONV_REQUIRE(n > 0 && c > 0 && (long long)n * c <= 65535,
                "viewport_render_f32: n * C = %lld planes, the grid takes 1 .. 65535", (long long)n * c);
  if (source_ok("viewport_render_f32", h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(vh >= 2 && vw >= 2 && vh <= (1 << 20) && vw <= (1 << 20),
                "viewport_render_f32: a view side of %dx%d is outside 2 .. 2^20", vw, vh);
  PCONV_REQUIRE(ss >= 1 && ss <= PCONV_VIEWPORT_MAX_SS, "viewport_render_f32: ss = %d supersampling is outside 1 .. %d", ss,
                PCONV_VIEWPORT_MAX_SS);
  PCONV_REQUIRE(8LL * ss * ss * vh * vw < (1LL << 31), "viewport_render_f32: a map of %dx%d records is 2^31 bytes or more",
                vw * ss, vh * ss);
  const long long frame = (long long)c * vh * vw;
  PCONV_REQUIRE(4LL * frame < (1LL << 31), "viewport_render_f32: an output frame of %d planes of %dx%d float32 is 2^31 bytes "
                "or more", c, vw, vh);
  PCONV_REQUIRE(out_frame_stride >= frame, "viewport_render_f32: the output frame stride %lld is below C * vh * vw = %lld",
                out_frame_stride, frame);
  const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out),
                  am = reinterpret_cast<uintptr_t>(map), ap = reinterpret_cast<uintptr_t>(phases);
  PCONV_REQUIRE(((ai | ao | ap) & 3) == 0 && (am & 7) == 0,
                "viewport_render_f32: the tensors must be 4-byte aligned, the map 8-byte aligned");
  PCONV_REQUIRE(in != out, "viewport_render_f32: in and out must be distinct (every output reads 36 inputs per sample)");
  const int tiles = (vw + kTileW - 1) / kTileW;
  const long long groups = (long long)tiles * ((vh + kTileH - 1) / kTileH);  // below 2^29 / 256 + 2^20 / 4 + 2^20 / 64 + 1
  hipLaunchKernelGGL(viewport_render_f32_kernel, dim3((unsigned)groups, n), dim3(kBlock), 0, as_stream(stream), in, out,
                     reinterpret_cast<const int2 *>(map), phases, c, h, w, vh, vw, ss, tiles, out_frame_stride,
                     (float)(1.0 / (ss * ss)), clamp);
  PCONV_LAUNCH_CHECK("viewport_render_f32");
  return PCONV_OK;
}
