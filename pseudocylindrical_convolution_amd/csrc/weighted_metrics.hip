// Weighted squared error over a per-pixel weight plane (the definition is in include/pconv_hip.h,
// pconv_weighted_mse_*): out[f][c] = (sum over the pixels p of w_p * (x - y)^2) / W, the weights a float64 (H, W) plane
// shared by all frames and channels.  The cube's solid-angle weights are its first user; a mask or a region of interest
// is the same call.
//   weighted_mse_kernel           a workgroup takes one chunk of 1024 pixels of one plane; lane l reads the pixels l,
//                                 l + 256, l + 512, l + 768 of the chunk (4-byte loads of x and y, 8-byte loads of the
//                                 weights, each a run of consecutive addresses over the workgroup), squares the difference
//                                 in fp32 and adds w * e in fp64; the tree of sphere_points.hip leaves the chunk's partial
//                                 in the workspace.  LOAD says how a pixel is read: float32 planes or interleaved uint8.
//   weighted_sum_kernel           one workgroup per plane adds its partials in the same lane / tree order and divides by W.
//   weighted_mse_backward_kernel  one lane per four pixels: k = ((2 g) w) / W in fp64, rounded once, times (y - x) in fp32.
//                                 WIDE: the four pixels are consecutive and move as 16-byte loads and one 16-byte store;
//                                 otherwise the lane takes the forward's four pixels with 4-byte accesses.  An element's
//                                 arithmetic does not depend on which lane holds it, so the two forms give the same bits.
//   weighted_ssim_kernel          the SSIM map weighed by the plane (pconv_weighted_ssim_f32): a workgroup takes one tile of 32
//                                 rows x 64 columns of one plane through the tile passes of ssim_tile.h -- the passes, and so
//                                 the map bits, of sphere_metrics.hip's ms_forward_kernel -- then every lane reads the weights of
//                                 its 8 rows of one column straight from global memory (a wave reads 64 consecutive doubles per
//                                 row; nothing of the plane is staged, so the workgroup keeps the 80 KB of LDS that lets two
//                                 share a CU) and adds w * map in fp64; a wave butterfly and the four waves in order give the
//                                 tile's partial.  weighted_sum_kernel adds a plane's tile partials as it adds chunk partials.
//   pconv_weighted_ssim_backward_f32  the gradient of that figure has no kernel here: the checks are below, the kernel is
//                                 sphere_metrics.hip's ms_backward_kernel with its per-pixel factor (launch_plane_backward).
// The tree's last six steps stay inside wave 0 (lane l and lane l + s, s <= 32, are both lanes of it), so they are register
// exchanges of the same fp64 additions in the same order: two LDS steps and two barriers instead of eight.
#include "sphere_sampler.h"
#include "ssim_tile.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = PCONV_SPHERE_POINTS_CHUNK;
constexpr int kPerLane = kChunk / kBlock;
static_assert(kPerLane == 4, "a lane takes four pixels of a chunk");

// lane l < s takes lane[l] + lane[l + s], s = 128 .. 1: the tree of the header; the result is in lane 0
__device__ __forceinline__ double tree_sum(double *part, double mine) {
  const int l = threadIdx.x;
  part[l] = mine;
  __syncthreads();
  if (l < 128) part[l] = part[l] + part[l + 128];
  __syncthreads();
  double v = 0.0;
  if (l < 64) {
    v = part[l] + part[l + 64];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, 64);   // lanes >= s hold values nobody reads
  }
  return v;
}

struct LoadF32 {
  const float *x, *y;
  __device__ __forceinline__ LoadF32(const void *px, const void *py, long long plane, int c_count, long long pixels)
      : x(static_cast<const float *>(px) + plane * pixels), y(static_cast<const float *>(py) + plane * pixels) {}
  __device__ __forceinline__ float a(long long p) const { return x[p]; }
  __device__ __forceinline__ float b(long long p) const { return y[p]; }
};

// uint8 (n, H, W, 3): plane (f, c) is every third byte of frame f from byte c on; float(u8) / 255.f, correctly rounded,
// as pconv_frames_u8_to_f32 and pconv_ws_metrics_u8
struct LoadU8 {
  const uint8_t *x, *y;
  int C;
  __device__ __forceinline__ LoadU8(const void *px, const void *py, long long plane, int c_count, long long pixels) : C(c_count) {
    const long long f = plane / c_count, c = plane - f * c_count;
    x = static_cast<const uint8_t *>(px) + f * pixels * c_count + c;
    y = static_cast<const uint8_t *>(py) + f * pixels * c_count + c;
  }
  __device__ __forceinline__ float a(long long p) const { return __fdiv_rn((float)x[p * C], 255.f); }
  __device__ __forceinline__ float b(long long p) const { return __fdiv_rn((float)y[p * C], 255.f); }
};

template <typename LOAD>
__global__ __launch_bounds__(kBlock) void weighted_mse_kernel(const void *__restrict__ x, const void *__restrict__ y,
                                                              const double *__restrict__ weights, int C, long long pixels,
                                                              long long chunks, double *__restrict__ partials) {
  __shared__ double part[kBlock];
  const LOAD in(x, y, blockIdx.y, C, pixels);
  const long long first = (long long)blockIdx.x * kChunk + threadIdx.x;
  // all twelve loads are issued before the first is used: a pixel that does not exist reads pixel 0 and adds nothing
  float a[kPerLane], b[kPerLane];
  double wt[kPerLane];
#pragma unroll
  for (int i = 0; i < kPerLane; i++) {
    const long long p = first + (long long)i * kBlock, q = p < pixels ? p : 0;
    a[i] = in.a(q), b[i] = in.b(q), wt[i] = weights[q];
  }
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < kPerLane; i++) {
    const float d = __fsub_rn(a[i], b[i]);
    const double term = __dmul_rn(wt[i], (double)__fmul_rn(d, d));
    if (first + (long long)i * kBlock < pixels) sum = sum + term;
  }
  const double total = tree_sum(part, sum);
  if (threadIdx.x == 0) partials[(long long)blockIdx.y * chunks + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void weighted_sum_kernel(const double *__restrict__ partials, long long chunks,
                                                              double W, double *__restrict__ out) {
  __shared__ double part[kBlock];
  const double *mine = partials + (long long)blockIdx.x * chunks;
  double sum = 0.0;
  for (long long q = threadIdx.x; q < chunks; q += kBlock) sum = sum + mine[q];
  const double total = tree_sum(part, sum);
  if (threadIdx.x == 0) out[blockIdx.x] = total / W;
}

// one workgroup per (tile, plane).  Lane (column col, row group rg) adds w * map of its rows rg .. rg + 7 that lie in the
// plane, ascending, from +0; the 64 columns of a row group by the butterfly m = 32 .. 1 (v + partner: every lane of the
// wave ends with the same bits); the four row groups ascending.  G.c is 1: blockIdx.y counts planes
__global__ __launch_bounds__(ssim::kBlock, 2) void weighted_ssim_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                       const double *__restrict__ weights, ssim::WsGeom G,
                                                                       double *__restrict__ partials) {
  using namespace ssim;
  __shared__ __attribute__((aligned(16))) float sx[kInRows * kLd];
  __shared__ __attribute__((aligned(16))) float sy[kInRows * kLd];
  __shared__ __attribute__((aligned(16))) float mom[5][kPlane];
  __shared__ double red[kWaves];
  const int tid = threadIdx.x, tile = blockIdx.x, plane = blockIdx.y;
  const int ty = tile / G.tiles_x;
  const int r0 = ty * kTileRows, c0 = (tile - ty * G.tiles_x) * kTileCols;
  const int col = tid & 63, rg = (tid >> 6) * kRowsPerLane;
  stage_tile(plane_of(x, G, plane, 0), plane_of(y, G, plane, 0), G, 0, r0, c0, sx, sy);
  float acc[kRowsPerLane][5];
  tile_moments(sx, sy, mom, G, rg, col, acc);
  // the eight weights are asked for before the first is used: a pixel outside the plane reads none and adds nothing
  double wt[kRowsPerLane];
#pragma unroll
  for (int o = 0; o < kRowsPerLane; o++) {
    const int r = r0 + rg + o;
    wt[o] = r < G.h && c0 + col < G.w ? weights[(unsigned)(r * G.w + c0 + col)] : 0.0;
  }
  double sum = 0.0;
#pragma unroll
  for (int o = 0; o < kRowsPerLane; o++)
    if (r0 + rg + o < G.h && c0 + col < G.w) sum = sum + __dmul_rn(wt[o], (double)ssim_map<true>(acc[o]));
  sum = wave_sum(sum);
  if (col == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) {
    double s = red[0];
#pragma unroll
    for (int k = 1; k < kWaves; k++) s = s + red[k];
    partials[(long long)plane * G.tiles + tile] = s;
  }
}

__device__ __forceinline__ float grad_of(double g2, double w, double W, float x, float y) {
  const float k = (float)(__dmul_rn(g2, w) / W);
  return __fmul_rn(k, __fsub_rn(y, x));
}

template <bool WIDE>
__global__ __launch_bounds__(kBlock) void weighted_mse_backward_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                                       const double *__restrict__ weights,
                                                                       const double *__restrict__ gout, double W,
                                                                       long long pixels, float *__restrict__ grad) {
  const long long base = (long long)blockIdx.y * pixels;
  const double g2 = __dmul_rn(2.0, gout[blockIdx.y]);
  if (WIDE) {  // pixels is a multiple of 4 and every pointer 16-byte aligned: so is every plane and every group of four
    const long long p = ((long long)blockIdx.x * kBlock + threadIdx.x) * kPerLane;
    if (p >= pixels) return;
    const float4 a = *reinterpret_cast<const float4 *>(x + base + p), b = *reinterpret_cast<const float4 *>(y + base + p);
    const double2 w0 = *reinterpret_cast<const double2 *>(weights + p), w1 = *reinterpret_cast<const double2 *>(weights + p + 2);
    float4 r;
    r.x = grad_of(g2, w0.x, W, a.x, b.x);
    r.y = grad_of(g2, w0.y, W, a.y, b.y);
    r.z = grad_of(g2, w1.x, W, a.z, b.z);
    r.w = grad_of(g2, w1.y, W, a.w, b.w);
    *reinterpret_cast<float4 *>(grad + base + p) = r;
  } else {
    const long long first = (long long)blockIdx.x * kChunk + threadIdx.x;
    float a[kPerLane], b[kPerLane];
    double wt[kPerLane];
#pragma unroll
    for (int i = 0; i < kPerLane; i++) {  // (a pixel that does not exist reads pixel 0 and stores nothing)
      const long long p = first + (long long)i * kBlock, q = p < pixels ? p : 0;
      a[i] = x[base + q], b[i] = y[base + q], wt[i] = weights[q];
    }
#pragma unroll
    for (int i = 0; i < kPerLane; i++) {
      const long long p = first + (long long)i * kBlock;
      if (p < pixels) grad[base + p] = grad_of(g2, wt[i], W, a[i], b[i]);
    }
  }
}

// [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void *a, long long na, const void *b, long long nb) {
  return addr(a) < addr(b) + (uintptr_t)nb && addr(b) < addr(a) + (uintptr_t)na;
}

int shape_ok(const char *what, int n, int c, int h, int w, double W) {
  if (planes_ok(what, n, c) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(h >= 1 && w >= 1 && h <= (1 << 20) && w <= (1 << 20), "%s: a side of %dx%d is outside 1 .. 2^20", what, w, h);
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a plane of %dx%d float32 is 2^31 bytes or more", what, w, h);
  PCONV_REQUIRE(W > 0.0 && W <= 1.79769313486231570e308, "%s: the weights' total %g is not a positive finite number", what, W);
  return PCONV_OK;
}

// the checks every forward shares; per_plane: the partials of one plane in the workspace
int forward_ok(const char *what, bool u8, const void *x, const void *y, const double *weights, double W, int n, int c, int h,
               int w, const void *workspace, const double *out, long long per_plane) {
  PCONV_REQUIRE(x && y && weights && workspace && out, "%s: null pointer", what);
  if (shape_ok(what, n, c, h, w, W) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(!u8 || c == 3, "%s: uint8 frames are (n, H, W, 3): C = %d", what, c);
  if (aligned_ok(what, u8 ? 0 : addr(x) | addr(y), "x and y", addr(weights) | addr(workspace) | addr(out),
                 "the weights, the workspace and out") != PCONV_OK)
    return PCONV_EINVAL;
  const long long pixels = (long long)h * w, planes = (long long)n * c;
  const long long bin = (u8 ? 1LL : 4LL) * planes * pixels, bwt = 8LL * pixels, bw = 8LL * planes * per_plane, bo = 8LL * planes;
  PCONV_REQUIRE(!overlap(out, bo, x, bin) && !overlap(out, bo, y, bin) && !overlap(out, bo, weights, bwt) &&
                    !overlap(workspace, bw, x, bin) && !overlap(workspace, bw, y, bin) && !overlap(workspace, bw, weights, bwt) &&
                    !overlap(workspace, bw, out, bo),
                "%s: out and the workspace must not alias an input or each other", what);
  return PCONV_OK;
}

int forward(const char *what, bool u8, const void *x, const void *y, const double *weights, double W, int n, int c, int h, int w,
            void *workspace, double *out, void *stream) {
  const long long pixels = (long long)h * w, planes = (long long)n * c, chunks = (pixels + kChunk - 1) / kChunk;
  if (forward_ok(what, u8, x, y, weights, W, n, c, h, w, workspace, out, chunks) != PCONV_OK) return PCONV_EINVAL;
  const dim3 grid((unsigned)chunks, (unsigned)planes);  // chunks <= 2^19
  double *partials = static_cast<double *>(workspace);
  if (u8)
    hipLaunchKernelGGL(weighted_mse_kernel<LoadU8>, grid, dim3(kBlock), 0, as_stream(stream), x, y, weights, c, pixels, chunks,
                       partials);
  else
    hipLaunchKernelGGL(weighted_mse_kernel<LoadF32>, grid, dim3(kBlock), 0, as_stream(stream), x, y, weights, c, pixels, chunks,
                       partials);
  PCONV_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(weighted_sum_kernel, dim3((unsigned)planes), dim3(kBlock), 0, as_stream(stream), partials, chunks, W, out);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

// tiles of 32 x 64 across and down a plane of h x w (both at most 2^20, the plane below 2^29 pixels: below 2^26 tiles)
inline int tiles_across(int w) { return (w + ssim::kTileCols - 1) / ssim::kTileCols; }
inline long long tiles_of(int h, int w) { return (long long)tiles_across(w) * ((h + ssim::kTileRows - 1) / ssim::kTileRows); }

}  // namespace

extern "C" long long pconv_weighted_mse_workspace_bytes(int n, int c, int h, int w) {
  if (shape_ok("weighted_mse_workspace_bytes", n, c, h, w, 1.0) != PCONV_OK) return PCONV_EINVAL;
  return 8LL * n * c * (((long long)h * w + kChunk - 1) / kChunk);
}

extern "C" int pconv_weighted_mse_f32(const float *x, const float *y, const double *weights, double total, int n, int c, int h,
                                      int w, void *workspace, double *out, void *stream) {
  return forward("weighted_mse_f32", false, x, y, weights, total, n, c, h, w, workspace, out, stream);
}

extern "C" int pconv_weighted_mse_u8(const uint8_t *x, const uint8_t *y, const double *weights, double total, int n, int c,
                                     int h, int w, void *workspace, double *out, void *stream) {
  return forward("weighted_mse_u8", true, x, y, weights, total, n, c, h, w, workspace, out, stream);
}

extern "C" int pconv_weighted_mse_backward_f32(const float *x, const float *y, const double *weights, double total,
                                               const double *gout, int n, int c, int h, int w, float *grad, void *stream) {
  const char *what = "weighted_mse_backward_f32";
  PCONV_REQUIRE(x && y && weights && gout && grad, "%s: null pointer", what);
  if (shape_ok(what, n, c, h, w, total) != PCONV_OK) return PCONV_EINVAL;
  if (aligned_ok(what, addr(x) | addr(y) | addr(grad), "x, y and the gradient", addr(weights) | addr(gout),
                 "the weights and gout") != PCONV_OK)
    return PCONV_EINVAL;
  const long long pixels = (long long)h * w, planes = (long long)n * c;
  const long long bin = 4LL * planes * pixels;
  PCONV_REQUIRE(!overlap(grad, bin, x, bin) && !overlap(grad, bin, y, bin) && !overlap(grad, bin, weights, 8LL * pixels) &&
                    !overlap(grad, bin, gout, 8LL * planes),
                "%s: the gradient must not alias an input", what);
  const bool wide = pixels % kPerLane == 0 && ((addr(x) | addr(y) | addr(grad) | addr(weights)) & 15) == 0;
  const dim3 grid((unsigned)((pixels + kChunk - 1) / kChunk), (unsigned)planes);
  if (wide)
    hipLaunchKernelGGL(weighted_mse_backward_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), x, y, weights, gout, total,
                       pixels, grad);
  else
    hipLaunchKernelGGL(weighted_mse_backward_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), x, y, weights, gout, total,
                       pixels, grad);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

extern "C" long long pconv_weighted_ssim_workspace_bytes(int n, int c, int h, int w) {
  if (shape_ok("weighted_ssim_workspace_bytes", n, c, h, w, 1.0) != PCONV_OK) return PCONV_EINVAL;
  return 8LL * n * c * tiles_of(h, w);
}

extern "C" int pconv_weighted_ssim_f32(const float *x, const float *y, const double *weights, double total, int n, int c, int h,
                                       int w, void *workspace, double *out, void *stream) {
  const char *what = "weighted_ssim_f32";
  PCONV_REQUIRE(x && y && weights && workspace && out, "%s: null pointer", what);
  if (shape_ok(what, n, c, h, w, total) != PCONV_OK) return PCONV_EINVAL;  // (before tiles_of: no count of a refused size)
  const long long tiles = tiles_of(h, w), planes = (long long)n * c;
  if (forward_ok(what, false, x, y, weights, total, n, c, h, w, workspace, out, tiles) != PCONV_OK) return PCONV_EINVAL;
  ssim::WsGeom G = {};
  G.c = 1, G.h = h, G.w = w, G.tiles_x = tiles_across(w), G.tiles = (int)tiles;
  ssim::gaussian_taps(G.g);
  double *partials = static_cast<double *>(workspace);
  hipLaunchKernelGGL(weighted_ssim_kernel, dim3((unsigned)tiles, (unsigned)planes), dim3(ssim::kBlock), 0, as_stream(stream), x, y,
                     weights, G, partials);
  PCONV_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(weighted_sum_kernel, dim3((unsigned)planes), dim3(kBlock), 0, as_stream(stream), partials, tiles, total, out);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

// the gradient of the weighted SSIM: the checks here, the kernel in sphere_metrics.hip (the ERP backward's passes with a
// per-pixel factor read from the plane: ssim_tile.h, launch_plane_backward)
extern "C" int pconv_weighted_ssim_backward_f32(const float *x, const float *y, const double *weights, double total,
                                                const double *gout, int n, int c, int h, int w, float *grad_y, void *stream) {
  const char *what = "weighted_ssim_backward_f32";
  PCONV_REQUIRE(x && y && weights && gout && grad_y, "%s: null pointer", what);
  if (shape_ok(what, n, c, h, w, total) != PCONV_OK) return PCONV_EINVAL;
  if (aligned_ok(what, addr(x) | addr(y) | addr(grad_y), "x, y and the gradient", addr(weights) | addr(gout),
                 "the weights and gout") != PCONV_OK)
    return PCONV_EINVAL;
  const long long pixels = (long long)h * w, planes = (long long)n * c;
  const long long bin = 4LL * planes * pixels;
  PCONV_REQUIRE(!overlap(grad_y, bin, x, bin) && !overlap(grad_y, bin, y, bin) && !overlap(grad_y, bin, weights, 8LL * pixels) &&
                    !overlap(grad_y, bin, gout, 8LL * planes),
                "%s: the gradient must not alias an input", what);
  return ssim::launch_plane_backward(what, x, y, weights, total, gout, (int)planes, h, w, grad_y, stream);
}
