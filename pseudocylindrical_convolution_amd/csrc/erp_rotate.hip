// Sphere rotation of ERP frames (the definition is in include/pconv_hip.h, pconv_erp_rotation_map /
// pconv_erp_remap_f32): float32 (n, C, h, w) -> (n, C, h, w), the same sphere seen in a rotated orientation.
// The work is split in a map and a sampler, so that the trigonometry is paid once per (size, rotation, direction)
// and not once per frame and plane:
//   erp_rotation_map_kernel  one lane per output pixel: its direction, the rotation (nine doubles, kernel arguments)
//                            -- all in fp64 -- and its record (sphere_sampler.h), one 8-byte store.
//   erp_remap_f32_kernel     the direct form.  A workgroup takes a tile of kTileH rows x kTileW columns of the output;
//                            a lane owns one pixel, reads its record once, decodes its footprint once (the phase
//                            table is in LDS, 6 KB, staged by the workgroup) and applies it to the C planes of its
//                            frame: 36 four-byte loads per plane, neighbouring lanes on neighbouring addresses wherever
//                            the map is smooth; the overlap of the footprints is left to L1 / L2.
// The sampler itself is sphere_sampler.h; each lane stores only its own pixel.
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64, kTileH = kBlock / kTileW;  // the sampler's tile: one wave per row

struct Mat9 {
  double m[9];
};

__global__ __launch_bounds__(kBlock) void erp_rotation_map_kernel(Mat9 M, int2 *__restrict__ map, int h, int w,
                                                                  int tiles) {
  const int j = blockIdx.x / tiles;
  const int i = (blockIdx.x - j * tiles) * kBlock + threadIdx.x;
  if (i >= w) return;
  const double theta = ((i + 0.5) / w - 0.5) * (2.0 * kPi);
  const double phi = (0.5 - (j + 0.5) / h) * kPi;
  const double cp = cos(phi), sp = sin(phi);
  const double dx = cp * cos(theta), dy = cp * sin(theta), dz = sp;
  const double sx = M.m[0] * dx + M.m[1] * dy + M.m[2] * dz;
  const double sy = M.m[3] * dx + M.m[4] * dy + M.m[5] * dz;
  const double sz = M.m[6] * dx + M.m[7] * dy + M.m[8] * dz;
  map[(long long)j * w + i] = record_of_direction(sx, sy, sz, h, w);
}

__global__ __launch_bounds__(kBlock) void erp_remap_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                               const int2 *__restrict__ map,
                                                               const float *__restrict__ phases, int C, int h, int w,
                                                               int tiles, int clamp) {
  __shared__ float table[kPhases * kTaps];
  stage_phase_table<kBlock>(table, phases);
  const int ty = blockIdx.x / tiles;
  const int i = (blockIdx.x - ty * tiles) * kTileW + (threadIdx.x % kTileW);
  const int j = ty * kTileH + threadIdx.x / kTileW;
  if (i >= w || j >= h) return;
  const int pixel = j * w + i;  // a plane is below 2^31 bytes: below 2^29 floats
  const Footprint foot = footprint_of(map[pixel], table, h, w);
  const long long plane = (long long)h * w;
  const float *src = in + (long long)blockIdx.y * C * plane;
  float *dst = out + (long long)blockIdx.y * C * plane + pixel;
  for (int c = 0; c < C; c++, src += plane, dst += plane) {
    float acc = apply(foot, src);
    if (clamp) acc = fminf(fmaxf(acc, 0.f), 1.f);
    *dst = acc;
  }
}

int angles_ok(const char *what, int yaw, int pitch, int roll) {
  const int half = 180 << 16, quarter = 90 << 16;
  PCONV_REQUIRE(yaw >= -half && yaw < half && pitch >= -quarter && pitch <= quarter && roll >= -half && roll < half,
                "%s: angles (%d, %d, %d) out of range: yaw and roll -180*2^16 .. 180*2^16 - 1, pitch -90*2^16 .. 90*2^16",
                what, yaw, pitch, roll);
  return PCONV_OK;
}

void mul3(const double *a, const double *b, double *c) {
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) c[3 * r + k] = a[3 * r] * b[k] + a[3 * r + 1] * b[3 + k] + a[3 * r + 2] * b[6 + k];
}

}  // namespace

extern "C" int pconv_host_erp_rotation_matrix(int yaw, int pitch, int roll, int inverse, double *m) {
  PCONV_REQUIRE(m, "host_erp_rotation_matrix: null pointer");
  if (angles_ok("host_erp_rotation_matrix", yaw, pitch, roll) != PCONV_OK) return PCONV_EINVAL;
  const double unit = kPi / 180.0 / 65536.0;
  const double cy = cos(yaw * unit), sy = sin(yaw * unit);
  const double cq = cos(-pitch * unit), sq = sin(-pitch * unit);
  const double cr = cos(roll * unit), sr = sin(roll * unit);
  const double rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1};
  const double ry[9] = {cq, 0, sq, 0, 1, 0, -sq, 0, cq};
  const double rx[9] = {1, 0, 0, 0, cr, -sr, 0, sr, cr};
  double zy[9], full[9];
  mul3(rz, ry, zy);
  mul3(zy, rx, full);
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) m[3 * r + k] = inverse ? full[3 * k + r] : full[3 * r + k];
  return PCONV_OK;
}

extern "C" int pconv_host_lanczos_phases(float *weights) {
  PCONV_REQUIRE(weights, "host_lanczos_phases: null pointer");
  for (int p = 0; p < kPhases; p++) {
    double raw[kTaps], sum = 0.0;
    for (int t = 0; t < kTaps; t++) {
      const int k = t - 2;
      if (p == 0) {
        raw[t] = k == 0 ? 1.0 : 0.0;  // the zeros of L at the integers, set and not evaluated
      } else {
        const double x = kPi * ((double)p / kPhases - k);
        raw[t] = 3.0 * sin(x) * sin(x / 3.0) / (x * x);
      }
      sum += raw[t];
    }
    for (int t = 0; t < kTaps; t++) weights[p * kTaps + t] = (float)(raw[t] / sum);
  }
  return PCONV_OK;
}

extern "C" int pconv_erp_rotation_map(int32_t *map, int h, int w, int yaw, int pitch, int roll, int inverse,
                                      void *stream) {
  PCONV_REQUIRE(map, "erp_rotation_map: null pointer");
  if (frame_ok("erp_rotation_map", "", h, w) != PCONV_OK) return PCONV_EINVAL;
  if (aligned8_ok("erp_rotation_map", addr(map), "the map") != PCONV_OK) return PCONV_EINVAL;
  Mat9 M;
  if (pconv_host_erp_rotation_matrix(yaw, pitch, roll, inverse, M.m) != PCONV_OK) return PCONV_EINVAL;
  const int tiles = (w + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(erp_rotation_map_kernel, dim3((unsigned)h * tiles), dim3(kBlock), 0, as_stream(stream), M,
                     reinterpret_cast<int2 *>(map), h, w, tiles);
  PCONV_LAUNCH_CHECK("erp_rotation_map");
  return PCONV_OK;
}

extern "C" int pconv_erp_remap_f32(const float *in, float *out, const int32_t *map, const float *phases, int n, int c,
                                   int h, int w, int clamp, void *stream) {
  PCONV_REQUIRE(in && out && map && phases, "erp_remap_f32: null pointer");
  if (planes_ok("erp_remap_f32", n, c) != PCONV_OK || frame_ok("erp_remap_f32", "", h, w) != PCONV_OK) return PCONV_EINVAL;
  if (aligned_ok("erp_remap_f32", addr(in) | addr(out) | addr(phases), "the tensors", addr(map), "the map") != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(in != out, "erp_remap_f32: in and out must be distinct (every output reads 36 inputs)");
  const int tiles = (w + kTileW - 1) / kTileW;
  const long long groups = (long long)tiles * ((h + kTileH - 1) / kTileH);  // below 2^29 / 256 + 2^20 / 4 + 2^20 / 64 + 1
  hipLaunchKernelGGL(erp_remap_f32_kernel, dim3((unsigned)groups, n), dim3(kBlock), 0, as_stream(stream), in, out,
                     reinterpret_cast<const int2 *>(map), phases, c, h, w, tiles, clamp);
  PCONV_LAUNCH_CHECK("erp_remap_f32");
  return PCONV_OK;
}
