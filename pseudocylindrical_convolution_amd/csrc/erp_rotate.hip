// Sphere rotation of ERP frames (the definition is in include/pconv_hip.h, pconv_erp_rotation_map /
// pconv_erp_remap_f32): float32 (n, C, h, w) -> (n, C, h, w), the same sphere seen in a rotated orientation.
// The work is split in a map and a sampler, so that the trigonometry is paid once per (size, rotation, direction)
// and not once per frame and plane:
//   erp_rotation_map_kernel  one lane per output pixel: its direction, the rotation (nine doubles, kernel arguments),
//                            two atan2 -- all in fp64 -- and the record (qu, qv) in 1/256 pixel, one 8-byte store.
//   erp_remap_f32_kernel     the direct form.  A workgroup takes a tile of kTileH rows x kTileW columns of the output;
//                            a lane owns one pixel, reads its record once, takes its two weight rows from the phase
//                            table in LDS (6 KB, staged by the workgroup) and walks the C planes of its frame: 36
//                            four-byte loads per plane, neighbouring lanes on neighbouring addresses wherever the map
//                            is smooth; the overlap of the footprints is left to L1 / L2.  Sums a-ascending over
//                            b-ascending row sums, one fp32 rounding per product and per addition.
// The sampler reduces every record to a position inside the frame (columns modulo w, rows by the pole rule and the
// clamp), so no map content makes it read outside `in`; each lane stores only its own pixel.
#include <math.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPhases = PCONV_ERP_ROTATE_PHASES;
constexpr int kTaps = PCONV_ERP_ROTATE_TAPS;
constexpr int kTileW = 64, kTileH = kBlock / kTileW;  // the sampler's tile: one wave per row
constexpr double kPi = 3.14159265358979323846;

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
  const double u = (atan2(sy, sx) / (2.0 * kPi) + 0.5) * w - 0.5;
  const double v = (0.5 - atan2(sz, hypot(sx, sy)) / kPi) * h - 0.5;
  const long long period = (long long)w * kPhases;
  long long qu = (long long)rint(u * kPhases) % period;  // |u| < w + 1: the conversion is exact
  if (qu < 0) qu += period;
  const int qv = (int)rint(v * kPhases);
  map[(long long)j * w + i] = make_int2((int)qu, qv);
}

__device__ __forceinline__ int pmod(int a, int m) {
  const int r = a % m;
  return r < 0 ? r + m : r;
}

__global__ __launch_bounds__(kBlock) void erp_remap_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                               const int2 *__restrict__ map,
                                                               const float *__restrict__ phases, int C, int h, int w,
                                                               int tiles, int clamp) {
  __shared__ float table[kPhases * kTaps];
  for (int k = threadIdx.x; k < kPhases * kTaps; k += kBlock) table[k] = phases[k];
  __syncthreads();
  const int ty = blockIdx.x / tiles;
  const int i = (blockIdx.x - ty * tiles) * kTileW + (threadIdx.x % kTileW);
  const int j = ty * kTileH + threadIdx.x / kTileW;
  if (i >= w || j >= h) return;
  const int pixel = j * w + i;  // a plane is below 2^31 bytes: below 2^29 floats
  const int2 rec = map[pixel];
  // floor division and the non-negative remainder by 256, for a negative qv as well (two's complement)
  const int col0 = (rec.x >> 8) - 2, row0 = (rec.y >> 8) - 2;
  const float *wx = table + (rec.x & (kPhases - 1)) * kTaps;
  const float *wy = table + (rec.y & (kPhases - 1)) * kTaps;
  const int half = w / 2;
  float fx[kTaps], fy[kTaps];
  unsigned col[kTaps], turned[kTaps], row[kTaps];
  bool crossed[kTaps];
#pragma unroll
  for (int b = 0; b < kTaps; b++) {
    fx[b] = wx[b];
    fy[b] = wy[b];
    const int cb = pmod(col0 + b, w);
    col[b] = cb;
    turned[b] = cb + half >= w ? cb + half - w : cb + half;
    int r = row0 + b;
    crossed[b] = r < 0 || r >= h;
    if (r < 0) r = -1 - r;
    else if (r >= h) r = 2 * h - 1 - r;
    row[b] = min(max(r, 0), h - 1) * w;
  }
  const long long plane = (long long)h * w;
  const float *src = in + (long long)blockIdx.y * C * plane;
  float *dst = out + (long long)blockIdx.y * C * plane + pixel;
  for (int c = 0; c < C; c++, src += plane, dst += plane) {
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

int frame_ok(const char *what, int h, int w) {
  PCONV_REQUIRE(h >= 2 && w >= 2 && h <= (1 << 20) && w <= (1 << 20), "%s: a side of %dx%d is outside 2 .. 2^20", what, w, h);
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a plane of %dx%d float32 is 2^31 bytes or more", what, w, h);
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
  if (frame_ok("erp_rotation_map", h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(map) & 7) == 0, "erp_rotation_map: the map must be 8-byte aligned");
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
  PCONV_REQUIRE(n > 0 && c > 0 && (long long)n * c <= 65535, "erp_remap_f32: n * C = %lld planes, the grid takes 1 .. 65535",
                (long long)n * c);
  if (frame_ok("erp_remap_f32", h, w) != PCONV_OK) return PCONV_EINVAL;
  const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out),
                  am = reinterpret_cast<uintptr_t>(map), ap = reinterpret_cast<uintptr_t>(phases);
  PCONV_REQUIRE(((ai | ao | ap) & 3) == 0 && (am & 7) == 0,
                "erp_remap_f32: the tensors must be 4-byte aligned, the map 8-byte aligned");
  PCONV_REQUIRE(in != out, "erp_remap_f32: in and out must be distinct (every output reads 36 inputs)");
  const int tiles = (w + kTileW - 1) / kTileW;
  const long long groups = (long long)tiles * ((h + kTileH - 1) / kTileH);  // below 2^29 / 256 + 2^20 / 4 + 2^20 / 64 + 1
  hipLaunchKernelGGL(erp_remap_f32_kernel, dim3((unsigned)groups, n), dim3(kBlock), 0, as_stream(stream), in, out,
                     reinterpret_cast<const int2 *>(map), phases, c, h, w, tiles, clamp);
  PCONV_LAUNCH_CHECK("erp_remap_f32");
  return PCONV_OK;
}
