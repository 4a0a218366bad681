// Sphere-sampled metrics (the definition is in include/pconv_hip.h, pconv_sphere_points_*): two ERP
// pictures of any two sizes are read at the same points of the sphere and the squared error is summed over the points.
//   sphere_points_records_kernel  one lane per point: (t, p) -> the 1/256-pixel record of a picture of h x w.  Four
//                                 fp64 operations per coordinate and a rint, no transcendental: the host evaluates
//                                 the same expression to the same bits.
//   sphere_points_sample_kernel   one lane per point, blockIdx.y a frame, the C planes walked by the lane: the sampler
//                                 of sphere_sampler.h (6 x 6 Lanczos-3) or its nearest pixel, one 4-byte store.
//   sphere_points_mse_kernel      the fused form.  A workgroup takes one chunk of 1024 points of one plane; a lane
//                                 samples both pictures at its four points, squares the difference in fp32 and adds it
//                                 in fp64; an LDS tree leaves the chunk's partial in the workspace.
//   sphere_points_sum_kernel      one workgroup per plane adds its partials in the same lane / tree order.
// The gather does nothing about the order of the points: an icosphere's order is not coherent in the picture, a CPP
// grid's is; both are left to L1 / L2 (DESIGN.md §4i says what that costs).  Each lane stores only its own element.
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = PCONV_SPHERE_POINTS_CHUNK;
constexpr int kPerLane = kChunk / kBlock;
constexpr long long kMaxPoints = (1LL << 28) - 1;

__global__ __launch_bounds__(kBlock) void sphere_points_records_kernel(const double2 *__restrict__ points,
                                                                       int2 *__restrict__ records, long long P, int h,
                                                                       int w) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= P) return;
  const double2 tp = points[k];
  const double u = ((tp.x / (2.0 * kPi)) + 0.5) * (double)w - 0.5;
  const double v = (0.5 - (tp.y / kPi)) * (double)h - 0.5;
  double ru = rint(u * (double)kPhases), rv = rint(v * (double)kPhases);
  // a point outside the stated ranges (or a NaN) gets a record all the same: the conversions below stay defined
  const double lim = 2147483000.0;
  ru = ru >= -lim && ru <= lim ? ru : 0.0;
  rv = rv >= -lim && rv <= lim ? rv : 0.0;
  records[k] = make_int2((int)wrap_record((long long)ru, w), (int)rv);
}

template <int MODE>
__device__ __forceinline__ float sample_at(const float *__restrict__ src, int2 rec, const float *table, int h, int w) {
  if (MODE == PCONV_SPHERE_POINTS_NEAREST) return sample_nearest(src, rec, h, w);
  return sample_lanczos(src, rec, table, h, w);
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void sphere_points_sample_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                                      const int2 *__restrict__ records,
                                                                      const float *__restrict__ phases, int C, int h,
                                                                      int w, long long P) {
  __shared__ float table[kPhases * kTaps];
  if (MODE == PCONV_SPHERE_POINTS_LANCZOS) stage_phase_table<kBlock>(table, phases);
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
  if (MODE == PCONV_SPHERE_POINTS_LANCZOS) stage_phase_table<kBlock>(table, phases);
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

int count_ok(const char *what, int n, int c, long long P) {
  if (planes_ok(what, n, c) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(P >= 1 && P <= kMaxPoints, "%s: %lld points, 1 .. 2^28 - 1 expected", what, P);
  return PCONV_OK;
}

int mode_ok(const char *what, int mode) {
  PCONV_REQUIRE(mode == PCONV_SPHERE_POINTS_LANCZOS || mode == PCONV_SPHERE_POINTS_NEAREST,
                "%s: unknown mode %d (PCONV_SPHERE_POINTS_LANCZOS = 0, PCONV_SPHERE_POINTS_NEAREST = 1)", what, mode);
  return PCONV_OK;
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, long long na, const void *b, long long nb) {
  return addr(a) < addr(b) + (uintptr_t)nb && addr(b) < addr(a) + (uintptr_t)na;
}

}  // namespace

extern "C" int pconv_sphere_points_records(const double *points, int32_t *records, long long P, int h, int w,
                                           void *stream) {
  PCONV_REQUIRE(points && records, "sphere_points_records: null pointer");
  if (frame_ok("sphere_points_records", "", h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(P >= 1 && P <= kMaxPoints, "sphere_points_records: %lld points, 1 .. 2^28 - 1 expected", P);
  if (aligned8_ok("sphere_points_records", addr(points) | addr(records), "the points and the records") != PCONV_OK)
    return PCONV_EINVAL;
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
  if (frame_ok("sphere_points_sample_f32", "", h, w) != PCONV_OK) return PCONV_EINVAL;
  if (mode_ok("sphere_points_sample_f32", mode) != PCONV_OK) return PCONV_EINVAL;
  if (aligned_ok("sphere_points_sample_f32", addr(in) | addr(out) | addr(phases), "the tensors", addr(records),
                 "the records") != PCONV_OK)
    return PCONV_EINVAL;
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
  if (frame_ok("sphere_points_mse_f32", "", h1, w1) != PCONV_OK || frame_ok("sphere_points_mse_f32", "", h2, w2) != PCONV_OK)
    return PCONV_EINVAL;
  if (mode_ok("sphere_points_mse_f32", mode) != PCONV_OK) return PCONV_EINVAL;
  if (aligned_ok("sphere_points_mse_f32", addr(x) | addr(y) | addr(phases), "the tensors",
                 addr(rec_x) | addr(rec_y) | addr(workspace) | addr(out), "the records, the workspace and out") != PCONV_OK)
    return PCONV_EINVAL;
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
