// Sphere-sampled metrics (the definition is in include/pconv_hip.h, pconv_sphere_points_*): two ERP
// pictures of any two sizes are read at the same points of the sphere and the squared error is summed over the points.
//   sphere_points_records_kernel  one lane per point: (t, p) -> the 1/256-pixel record of a picture of h x w.  Four
//                                 fp64 operations per coordinate and a rint, no transcendental: the host evaluates
//                                 the same expression to the same bits.
//   sphere_points_sample_kernel   one lane per point, blockIdx.y a frame, the C planes walked by the lane: the footprint
//                                 of erp_rotate.hip's sampler (6 x 6 Lanczos-3) or the nearest pixel, one 4-byte store.
//   sphere_points_mse_kernel      the fused form.  A workgroup takes one chunk of 1024 points of one plane; a lane
//                                 samples both pictures at its four points, squares the difference in fp32 and adds it
//                                 in fp64; an LDS tree leaves the chunk's partial in the workspace.
//   sphere_points_sum_kernel      one workgroup per plane adds its partials in the same lane / tree order.
// The gather does nothing about the order of the points: an icosphere's order is not coherent in the picture, a CPP
// grid's is; both are left to L1 / L2 (DESIGN.md §4i says what that costs).  Every record is reduced to a position
// inside its frame (columns modulo w, rows by the pole rule and the clamp), so no record content makes a kernel read
// outside a picture; each lane stores only its own element.
#include <math.h>
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPhases = PCONV_ERP_ROTATE_PHASES;
constexpr int kTaps = PCONV_ERP_ROTATE_TAPS;
constexpr int kChunk = PCONV_SPHERE_POINTS_CHUNK;
constexpr int kPerLane = kChunk / kBlock;
constexpr long long kMaxPoints = (1LL << 28) - 1;
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;

__global__ __launch_bounds__(kBlock) void sphere_points_records_kernel(const double2 *__restrict__ points,
                                                                       int2 *__restrict__ records, long long P, int h,
                                                                       int w) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P) return;
  const double2 tp = points[k];
  const double u = ((tp.x / kTwoPi) + 0.5) * (double)w - 0.5;
  const double v = (0.5 - (tp.y / kPi)) * (double)h - 0.5;
  double ru = rint(u * (double)kPhases), rv = rint(v * (double)kPhases);
  // a point outside the stated ranges (or a NaN) gets a record all the same: the conversions below stay defined
  const double lim = 2147483000.0;
  ru = ru >= -lim && ru <= lim ? ru : 0.0;
  rv = rv >= -lim && rv <= lim ? rv : 0.0;
  const long long period = (long long)w * kPhases;
  long long qu = (long long)ru % period;
  if (qu < 0) qu += period;
  records[k] = make_int2((int)qu, (int)rv);
}

__device__ __forceinline__ int pmod(int a, int m) {
  const int r = a % m;
  return r < 0 ? r + m : r;
}

// the sampler of erp_remap_f32_kernel at one record: `table` is the phase table in LDS
__device__ __forceinline__ float sample_lanczos(const float *__restrict__ src, int2 rec, const float *table, int h, int w) {
  // floor division and the non-negative remainder by 256, for a negative record as well (two's complement)
  const int col0 = (rec.x >> 8) - 2, row0 = (rec.y >> 8) - 2;
  const float *wx = table + (rec.x & (kPhases - 1)) * kTaps;
  const float *wy = table + (rec.y & (kPhases - 1)) * kTaps;
  const int half = w / 2;
  float fx[kTaps];
  unsigned col[kTaps], turned[kTaps];
#pragma unroll
  for (int b = 0; b < kTaps; b++) {
    fx[b] = wx[b];
    const int cb = pmod(col0 + b, w);
    col[b] = cb;
    turned[b] = cb + half >= w ? cb + half - w : cb + half;
  }
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < kTaps; a++) {
    int r = row0 + a;
    const bool crossed = r < 0 || r >= h;
    if (r < 0) r = -1 - r;
    else if (r >= h) r = 2 * h - 1 - r;
    const unsigned row = (unsigned)(min(max(r, 0), h - 1)) * (unsigned)w;  // a plane is below 2^29 floats
    float s = __fmul_rn(fx[0], src[row + (crossed ? turned[0] : col[0])]);
#pragma unroll
    for (int b = 1; b < kTaps; b++) s = __fadd_rn(s, __fmul_rn(fx[b], src[row + (crossed ? turned[b] : col[b])]));
    const float m = __fmul_rn(wy[a], s);
    acc = a == 0 ? m : __fadd_rn(acc, m);
  }
  return acc;
}

__device__ __forceinline__ float sample_nearest(const float *__restrict__ src, int2 rec, int h, int w) {
  // floor((q + 128) / 256) without the addition's overflow for a record near INT_MAX
  int c = pmod((rec.x >> 8) + ((rec.x & (kPhases - 1)) >= kPhases / 2 ? 1 : 0), w);
  int r = (rec.y >> 8) + ((rec.y & (kPhases - 1)) >= kPhases / 2 ? 1 : 0);
  const bool crossed = r < 0 || r >= h;
  if (r < 0) r = -1 - r;
  else if (r >= h) r = 2 * h - 1 - r;
  r = min(max(r, 0), h - 1);
  if (crossed) c = c + w / 2 >= w ? c + w / 2 - w : c + w / 2;
  return src[(unsigned)r * (unsigned)w + (unsigned)c];
}

template <int MODE>
__device__ __forceinline__ float sample_at(const float *__restrict__ src, int2 rec, const float *table, int h, int w) {
  if (MODE == PCONV_SPHERE_POINTS_NEAREST) return sample_nearest(src, rec, h, w);
  return sample_lanczos(src, rec, table, h, w);
}

__device__ __forceinline__ void stage_table(float *table, const float *__restrict__ phases) {
  for (int k = threadIdx.x; k < kPhases * kTaps; k += kBlock) table[k] = phases[k];
  __syncthreads();
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void sphere_points_sample_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                      const int2 *__restrict__ records,
                                                                      const float *__restrict__ phases, int C, int h,
                                                                      int w, long long P) {
  __shared__ float table[kPhases * kTaps];
  if (MODE == PCONV_SPHERE_POINTS_LANCZOS) stage_table(table, phases);
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P) return;
  const int2 rec = records[k];
  const long long plane = (long long)h * w;
  const float *src = in + (long long)blockIdx.y * C * plane;
  float *dst = out + (long long)blockIdx.y * C * P + k;
  for (int c = 0; c < C; c++, src += plane, dst += P) *dst = sample_at<MODE>(src, rec, table, h, w);
}

// lane l < s takes lane[l] + lane[l + s], s = 128 .. 1: the tree of the header; the result is in part[0]
__device__ __forceinline__ void tree_sum(double *part, double mine) {
  part[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll
  for (int s = kBlock / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + s];
    __syncthreads();
  }
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void sphere_points_mse_kernel(const float *__restrict__ x, int h1, int w1,
                                                                   const int2 *__restrict__ rec_x,
                                                                   const float *__restrict__ y, int h2, int w2,
                                                                   const int2 *__restrict__ rec_y,
                                                                   const float *__restrict__ phases, long long P,
                                                                   long long chunks, double *__restrict__ partials) {
  __shared__ float table[kPhases * kTaps];
  __shared__ double part[kBlock];
  if (MODE == PCONV_SPHERE_POINTS_LANCZOS) stage_table(table, phases);
  const float *px = x + (long long)blockIdx.y * h1 * w1;
  const float *py = y + (long long)blockIdx.y * h2 * w2;
  const long long first = (long long)blockIdx.x * kChunk + threadIdx.x;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < kPerLane; i++) {
    const long long k = first + (long long)i * kBlock;
    if (k < P) {
      const float a = sample_at<MODE>(px, rec_x[k], table, h1, w1);
      const float b = sample_at<MODE>(py, rec_y[k], table, h2, w2);
      const float d = __fsub_rn(a, b);
      sum = sum + (double)__fmul_rn(d, d);
    }
  }
  tree_sum(part, sum);
  if (threadIdx.x == 0) partials[(long long)blockIdx.y * chunks + blockIdx.x] = part[0];
}

__global__ __launch_bounds__(kBlock) void sphere_points_sum_kernel(const double *__restrict__ partials, long long chunks,
                                                                   long long P, double *__restrict__ out) {
  __shared__ double part[kBlock];
  const double *mine = partials + (long long)blockIdx.x * chunks;
  double sum = 0.0;
  for (long long q = threadIdx.x; q < chunks; q += kBlock) sum = sum + mine[q];
  tree_sum(part, sum);
  if (threadIdx.x == 0) out[blockIdx.x] = part[0] / (double)P;
}

int frame_ok(const char *what, int h, int w) {
  PCONV_REQUIRE(h >= 2 && w >= 2 && h <= (1 << 20) && w <= (1 << 20), "%s: a side of %dx%d is outside 2 .. 2^20", what, w, h);
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a plane of %dx%d float32 is 2^31 bytes or more", what, w, h);
  return PCONV_OK;
}

int count_ok(const char *what, int n, int c, long long P) {
  PCONV_REQUIRE(n > 0 && c > 0 && (long long)n * c <= 65535, "%s: n * C = %lld planes, the grid takes 1 .. 65535", what,
                (long long)n * c);
  PCONV_REQUIRE(P >= 1 && P <= kMaxPoints, "%s: %lld points, 1 .. 2^28 - 1 expected", what, P);
  return PCONV_OK;
}

int mode_ok(const char *what, int mode) {
  PCONV_REQUIRE(mode == PCONV_SPHERE_POINTS_LANCZOS || mode == PCONV_SPHERE_POINTS_NEAREST,
                "%s: unknown mode %d (PCONV_SPHERE_POINTS_LANCZOS = 0, PCONV_SPHERE_POINTS_NEAREST = 1)", what, mode);
  return PCONV_OK;
}

inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, long long na, const void *b, long long nb) {
  return addr(a) < addr(b) + (uintptr_t)nb && addr(b) < addr(a) + (uintptr_t)na;
}

}  // namespace

extern "C" int pconv_sphere_points_records(const double *points, int32_t *records, long long P, int h, int w,
                                           void *stream) {
  PCONV_REQUIRE(points && records, "sphere_points_records: null pointer");
  if (frame_ok("sphere_points_records", h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(P >= 1 && P <= kMaxPoints, "sphere_points_records: %lld points, 1 .. 2^28 - 1 expected", P);
  PCONV_REQUIRE(((addr(points) | addr(records)) & 7) == 0, "sphere_points_records: the points and the records must be 8-byte aligned");
  PCONV_REQUIRE(!overlap(points, 16 * P, records, 8 * P), "sphere_points_records: the records overlap the points");
  const long long blocks = (P + kBlock - 1) / kBlock;  // below 2^20
  hipLaunchKernelGGL(sphere_points_records_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream),
                     reinterpret_cast<const double2 *>(points), reinterpret_cast<int2 *>(records), P, h, w);
  PCONV_LAUNCH_CHECK("sphere_points_records");
  return PCONV_OK;
}

extern "C" int pconv_sphere_points_sample_f32(const float *in, float *out, const int32_t *records, const float *phases,
                                              int n, int c, int h, int w, long long P, int mode, void *stream) {
  PCONV_REQUIRE(in && out && records && phases, "sphere_points_sample_f32: null pointer");
  if (count_ok("sphere_points_sample_f32", n, c, P) != PCONV_OK) return PCONV_EINVAL;
  if (frame_ok("sphere_points_sample_f32", h, w) != PCONV_OK) return PCONV_EINVAL;
  if (mode_ok("sphere_points_sample_f32", mode) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(((addr(in) | addr(out) | addr(phases)) & 3) == 0 && (addr(records) & 7) == 0,
                "sphere_points_sample_f32: the tensors must be 4-byte aligned, the records 8-byte aligned");
  PCONV_REQUIRE(!overlap(in, 4LL * n * c * h * w, out, 4LL * n * c * P),
                "sphere_points_sample_f32: in and out must be distinct");
  const dim3 grid((unsigned)((P + kBlock - 1) / kBlock), (unsigned)n);
  const int2 *rec = reinterpret_cast<const int2 *>(records);
  if (mode == PCONV_SPHERE_POINTS_NEAREST)
    hipLaunchKernelGGL(sphere_points_sample_kernel<PCONV_SPHERE_POINTS_NEAREST>, grid, dim3(kBlock), 0, as_stream(stream),
                       in, out, rec, phases, c, h, w, P);
  else
    hipLaunchKernelGGL(sphere_points_sample_kernel<PCONV_SPHERE_POINTS_LANCZOS>, grid, dim3(kBlock), 0, as_stream(stream),
                       in, out, rec, phases, c, h, w, P);
  PCONV_LAUNCH_CHECK("sphere_points_sample_f32");
  return PCONV_OK;
}

extern "C" long long pconv_sphere_points_mse_workspace_bytes(int n, int c, long long P) {
  if (count_ok("sphere_points_mse_workspace_bytes", n, c, P) != PCONV_OK) return PCONV_EINVAL;
  return 8LL * n * c * ((P + kChunk - 1) / kChunk);
}

extern "C" int pconv_sphere_points_mse_f32(const float *x, int h1, int w1, const int32_t *rec_x, const float *y, int h2,
                                           int w2, const int32_t *rec_y, const float *phases, int n, int c, long long P,
                                           int mode, void *workspace, double *out, void *stream) {
  PCONV_REQUIRE(x && y && rec_x && rec_y && phases && workspace && out, "sphere_points_mse_f32: null pointer");
  if (count_ok("sphere_points_mse_f32", n, c, P) != PCONV_OK) return PCONV_EINVAL;
  if (frame_ok("sphere_points_mse_f32", h1, w1) != PCONV_OK || frame_ok("sphere_points_mse_f32", h2, w2) != PCONV_OK)
    return PCONV_EINVAL;
  if (mode_ok("sphere_points_mse_f32", mode) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(((addr(x) | addr(y) | addr(phases)) & 3) == 0 && ((addr(rec_x) | addr(rec_y) | addr(workspace) | addr(out)) & 7) == 0,
                "sphere_points_mse_f32: the tensors must be 4-byte aligned, the records, the workspace and out 8-byte aligned");
  const long long planes = (long long)n * c, chunks = (P + kChunk - 1) / kChunk;
  const long long bx = 4LL * planes * h1 * w1, by = 4LL * planes * h2 * w2, bw = 8LL * planes * chunks, bo = 8LL * planes;
  PCONV_REQUIRE(!overlap(out, bo, x, bx) && !overlap(out, bo, y, by) && !overlap(workspace, bw, x, bx) &&
                    !overlap(workspace, bw, y, by) && !overlap(workspace, bw, out, bo),
                "sphere_points_mse_f32: out and the workspace must not alias an input or each other");
  const dim3 grid((unsigned)chunks, (unsigned)planes);  // chunks below 2^18
  const int2 *rx = reinterpret_cast<const int2 *>(rec_x), *ry = reinterpret_cast<const int2 *>(rec_y);
  double *partials = static_cast<double *>(workspace);
  if (mode == PCONV_SPHERE_POINTS_NEAREST)
    hipLaunchKernelGGL(sphere_points_mse_kernel<PCONV_SPHERE_POINTS_NEAREST>, grid, dim3(kBlock), 0, as_stream(stream), x,
                       h1, w1, rx, y, h2, w2, ry, phases, P, chunks, partials);
  else
    hipLaunchKernelGGL(sphere_points_mse_kernel<PCONV_SPHERE_POINTS_LANCZOS>, grid, dim3(kBlock), 0, as_stream(stream), x,
                       h1, w1, rx, y, h2, w2, ry, phases, P, chunks, partials);
  PCONV_LAUNCH_CHECK("sphere_points_mse_f32");
  hipLaunchKernelGGL(sphere_points_sum_kernel, dim3((unsigned)planes), dim3(kBlock), 0, as_stream(stream), partials, chunks,
                     P, out);
  PCONV_LAUNCH_CHECK("sphere_points_mse_f32");
  return PCONV_OK;
}
