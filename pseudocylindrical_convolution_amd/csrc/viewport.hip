// Rectilinear viewports of ERP frames (the definition is in include/pconv_hip.h, pconv_viewport_map /
// pconv_viewport_render_f32): float32 (n, C, h, w) -> n frames of (C, vh, vw), the gnomonic view of the sphere in a given
// orientation and field of view, ss x ss samples averaged per pixel.  Split like the sphere rotation (erp_rotate.hip):
//   viewport_map_kernel         one lane per grid sample: its direction (1, a, b), the rotation and the two tangents
//                               (eleven doubles, kernel arguments) -- all in fp64 -- and its record on the source
//                               (sphere_sampler.h), one 8-byte store.
//   viewport_render_f32_kernel  a workgroup takes a tile of kTileH rows x kTileW columns of the VIEW; a lane owns one
//                               pixel.  Loop order: planes outermost, then the pixel's ss x ss records (p outer, t
//                               inner), then the 6 x 6 footprint: one accumulator whatever C is, and a plane's pixel is
//                               finished -- scaled, clamped, stored -- before the next plane begins.  The records are
//                               read again for every plane (8 bytes beside the 144 of the footprint they address, from
//                               L1 / L2: neighbouring lanes read neighbouring runs of ss records) and are NOT staged in
//                               LDS: at ss = 4 a tile's records are 32 KB, which would hold a CU to four workgroups for
//                               one load in 37.  The phase table (6 KB) is in LDS, staged by the workgroup.
// The sampler itself is sphere_sampler.h; each lane stores only its own pixel.
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = kBlock / kTileW;  // the renderer's tile: one wave per row

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
  map[(long long)r * gw + q] = record_of_direction(sx, sy, sz, h, w);
}

__global__ __launch_bounds__(kBlock) void viewport_render_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                     const int2 *__restrict__ map,
                                                                     const float *__restrict__ phases, int C, int h, int w,
                                                                     int vh, int vw, int ss, int tiles,
                                                                     long long out_frame_stride, float scale, int clamp) {
  __shared__ float table[kPhases * kTaps];
  stage_phase_table<kBlock>(table, phases);
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
        const float s = sample_lanczos(src, recs[p * gw + t], table, h, w);
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
  if (frame_ok("viewport_map", "source ", h, w) != PCONV_OK) return PCONV_EINVAL;
  const int side = PCONV_VIEWPORT_MAX_SS << 20;
  PCONV_REQUIRE(gh >= 2 && gw >= 2 && gh <= side && gw <= side, "viewport_map: a grid side of %dx%d is outside 2 .. %d * 2^20",
                gw, gh, PCONV_VIEWPORT_MAX_SS);
  PCONV_REQUIRE(8LL * gh * gw < (1LL << 31), "viewport_map: a map of %dx%d records is 2^31 bytes or more", gw, gh);
  if (aligned8_ok("viewport_map", addr(map), "the map") != PCONV_OK) return PCONV_EINVAL;
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
  if (planes_ok("viewport_render_f32", n, c) != PCONV_OK || frame_ok("viewport_render_f32", "source ", h, w) != PCONV_OK ||
      side_ok("viewport_render_f32", "view ", vh, vw) != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(ss >= 1 && ss <= PCONV_VIEWPORT_MAX_SS, "viewport_render_f32: ss = %d supersampling is outside 1 .. %d", ss,
                PCONV_VIEWPORT_MAX_SS);
  PCONV_REQUIRE(8LL * ss * ss * vh * vw < (1LL << 31), "viewport_render_f32: a map of %dx%d records is 2^31 bytes or more",
                vw * ss, vh * ss);
  const long long frame = (long long)c * vh * vw;
  PCONV_REQUIRE(4LL * frame < (1LL << 31), "viewport_render_f32: an output frame of %d planes of %dx%d float32 is 2^31 bytes "
                "or more", c, vw, vh);
  PCONV_REQUIRE(out_frame_stride >= frame, "viewport_render_f32: the output frame stride %lld is below C * vh * vw = %lld",
                out_frame_stride, frame);
  if (aligned_ok("viewport_render_f32", addr(in) | addr(out) | addr(phases), "the tensors", addr(map), "the map") != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(in != out, "viewport_render_f32: in and out must be distinct (every output reads 36 inputs per sample)");
  const int tiles = (vw + kTileW - 1) / kTileW;
  const long long groups = (long long)tiles * ((vh + kTileH - 1) / kTileH);  // below 2^29 / 256 + 2^20 / 4 + 2^20 / 64 + 1
  hipLaunchKernelGGL(viewport_render_f32_kernel, dim3((unsigned)groups, n), dim3(kBlock), 0, as_stream(stream), in, out,
                     reinterpret_cast<const int2 *>(map), phases, c, h, w, vh, vw, ss, tiles, out_frame_stride,
                     (float)(1.0 / (ss * ss)), clamp);
  PCONV_LAUNCH_CHECK("viewport_render_f32");
  return PCONV_OK;
}
