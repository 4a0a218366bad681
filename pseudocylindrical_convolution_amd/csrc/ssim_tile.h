// The tile passes of the SSIM map, shared by the kernels that weigh the map by a row cosine (sphere_metrics.hip,
// ms_forward_kernel) and by a per-pixel weight plane (weighted_metrics.hip, weighted_ssim_kernel): the same operations in
// the same order, so the same map bits.  A workgroup of 256 lanes takes a tile of 32 rows x 64 columns of one plane:
//   stage_tile    the 42 x 74 tile with its halo of 5 into LDS (zeros outside the plane), all loads before the first store
//   tile_moments  the horizontal pass, 4 adjacent outputs per lane from four float4 reads, into five moment planes (mu_x,
//                 mu_y, x², y², xy: 42 x 64 each, in LDS), then the vertical pass, 8 rows of one column per lane
//   ssim_map      the map of one pixel from its five moments
// Every 11-tap sum runs k-ascending as fmaf(g[k], v, acc) from acc = 0, the horizontal pass first.
#pragma once
#include <math.h>

#include "common.h"

namespace ssim {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileRows = 32, kTileCols = 64;
constexpr int kHalo = 5, kTaps = 2 * kHalo + 1;
constexpr int kInRows = kTileRows + 2 * kHalo;  // 42
constexpr int kInCols = kTileCols + 2 * kHalo;  // 74
constexpr int kLd = 76;                         // staged row stride: 16-byte rows, the last float4 read ends at 75
constexpr int kQuads = kTileCols / 4;           // horizontal pass: 4 adjacent outputs per lane
constexpr int kRowsPerLane = 8;                 // vertical pass: 8 rows of one column per lane
constexpr int kStage = (kInRows * kInCols + kBlock - 1) / kBlock;  // staged elements per lane and input
constexpr int kPlane = kInRows * kTileCols;
static_assert(kBlock == kTileCols * (kTileRows / kRowsPerLane), "vertical pass: one lane per (column, row group)");
static_assert(4 * (kQuads - 1) + 16 <= kLd, "horizontal pass: the last float4 read stays inside the staged row");

struct WsGeom {
  int c, h, w, tiles_x, tiles, uniform;
  float g[kTaps];  // the normalised 1-D Gaussian in fp32
};

// The backward of the map has one kernel, sphere_metrics.hip's ms_backward_kernel (passes A-E, 154 KB of LDS): this launches
// its weight-plane form for weighted_metrics.hip, which checks the arguments of pconv_weighted_ssim_backward_f32 first.
// `planes` = n * C; gout one double per plane and the weights (h, w), both on the device
int launch_plane_backward(const char *what, const float *x, const float *y, const double *weights, double total,
                          const double *gout, int planes, int h, int w, float *grad_y, void *stream);

// pytorch_ssim.gaussian(11, 1.5): exp(-(k - 5)² / (2·1.5²)) in double, normalised; here in fp32
inline void gaussian_taps(float *out) {
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; k++) sum += g[k] = exp(-(double)((k - kHalo) * (k - kHalo)) / (2.0 * 1.5 * 1.5));
  for (int k = 0; k < kTaps; k++) out[k] = (float)(g[k] / sum);
}

// the frame's plane (f, ch) as a uniform base, a pixel as a 32-bit offset from it (a plane is below 2^31 bytes)
__device__ __forceinline__ const float *plane_of(const float *__restrict__ p, const WsGeom &G, int f, int ch) {
  return p + ((long long)f * G.c + ch) * G.h * G.w;
}
__device__ __forceinline__ float load_px(const float *__restrict__ plane, const WsGeom &G, int ch, int r, int col) {
  return plane[(unsigned)(r * G.w + col)];
}

// uint8 (n, h, w, 3): the frame as the base; float(u8) / 255.f, correctly rounded, as pconv_frames_u8_to_f32
__device__ __forceinline__ const uint8_t *plane_of(const uint8_t *__restrict__ p, const WsGeom &G, int f, int) {
  return p + (long long)f * G.h * G.w * 3;
}
__device__ __forceinline__ float load_px(const uint8_t *__restrict__ frame, const WsGeom &G, int ch, int r, int col) {
  return __fdiv_rn((float)frame[(unsigned)((r * G.w + col) * 3 + ch)], 255.f);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// the tile at (r0, c0) of the planes xp / yp with its halo, into sx / sy (kInRows x kLd floats each).  The first barrier
// lets the previous user of sx / sy / the moment planes finish; the tile is visible after the second
template <typename T>
__device__ __forceinline__ void stage_tile(const T *__restrict__ xp, const T *__restrict__ yp, const WsGeom &G, int ch, int r0,
                                           int c0, float *sx, float *sy) {
  const int tid = threadIdx.x;
  float xv[kStage], yv[kStage];
#pragma unroll
  for (int k = 0; k < kStage; k++) {
    const int e = tid + k * kBlock;
    const int rr = e / kInCols, cc = e - rr * kInCols;
    const int gr = r0 - kHalo + rr, gc = c0 - kHalo + cc;
    const bool in = e < kInRows * kInCols && gr >= 0 && gr < G.h && gc >= 0 && gc < G.w;
    xv[k] = in ? load_px(xp, G, ch, gr, gc) : 0.f;
    yv[k] = in ? load_px(yp, G, ch, gr, gc) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kStage; k++) {
    const int e = tid + k * kBlock;
    if (e < kInRows * kInCols) {
      const int rr = e / kInCols, o = rr * kLd + (e - rr * kInCols);
      sx[o] = xv[k];
      sy[o] = yv[k];
    }
  }
  __syncthreads();
}

// the five moments of the rows rg .. rg + 7 of column col of the staged tile: acc[o] = mu_x, mu_y, blur(x²), blur(y²),
// blur(xy) at tile row rg + o.  mom: five planes of kPlane floats
__device__ __forceinline__ void tile_moments(const float *sx, const float *sy, float (*mom)[kPlane], const WsGeom &G, int rg,
                                             int col, float (&acc)[kRowsPerLane][5]) {
  const int tid = threadIdx.x;
  // horizontal pass: 4 adjacent outputs of one staged row per lane, from 14 inputs read as four float4
  for (int u = tid; u < kInRows * kQuads; u += kBlock) {
    const int rr = u / kQuads, q = u - rr * kQuads;
    float a[16], b[16];
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const float4 av = *reinterpret_cast<const float4 *>(sx + rr * kLd + 4 * q + 4 * v);
      const float4 bv = *reinterpret_cast<const float4 *>(sy + rr * kLd + 4 * q + 4 * v);
      a[4 * v] = av.x, a[4 * v + 1] = av.y, a[4 * v + 2] = av.z, a[4 * v + 3] = av.w;
      b[4 * v] = bv.x, b[4 * v + 1] = bv.y, b[4 * v + 2] = bv.z, b[4 * v + 3] = bv.w;
    }
    float m[5][4];
#pragma unroll
    for (int o = 0; o < 4; o++) {
#pragma unroll
      for (int t = 0; t < 5; t++) m[t][o] = 0.f;
#pragma unroll
      for (int k = 0; k < kTaps; k++) {
        const float p = a[o + k], s = b[o + k], g = G.g[k];
        m[0][o] = fmaf(g, p, m[0][o]);
        m[1][o] = fmaf(g, s, m[1][o]);
        m[2][o] = fmaf(g, p * p, m[2][o]);
        m[3][o] = fmaf(g, s * s, m[3][o]);
        m[4][o] = fmaf(g, p * s, m[4][o]);
      }
    }
#pragma unroll
    for (int t = 0; t < 5; t++)
      *reinterpret_cast<float4 *>(&mom[t][rr * kTileCols + 4 * q]) = make_float4(m[t][0], m[t][1], m[t][2], m[t][3]);
  }
  __syncthreads();
  // vertical pass: rows rg..rg+7 of column col, from moment rows rg..rg+17
#pragma unroll
  for (int o = 0; o < kRowsPerLane; o++)
#pragma unroll
    for (int t = 0; t < 5; t++) acc[o][t] = 0.f;
#pragma unroll
  for (int i = 0; i < kRowsPerLane + 2 * kHalo; i++) {
    float v[5];
#pragma unroll
    for (int t = 0; t < 5; t++) v[t] = mom[t][(rg + i) * kTileCols + col];
#pragma unroll
    for (int o = 0; o < kRowsPerLane; o++) {
      if (i - o >= 0 && i - o < kTaps) {
#pragma unroll
        for (int t = 0; t < 5; t++) acc[o][t] = fmaf(G.g[i - o], v[t], acc[o][t]);
      }
    }
  }
}

// FULL: the map l·cs = ((2 mu_x mu_y + C1)(2 s_xy + C2)) / ((mu_x² + mu_y² + C1)(s_x² + s_y² + C2)); otherwise cs alone,
// (2 s_xy + C2) / (s_x² + s_y² + C2).  C1 = 0.01², C2 = 0.03², sigma² = blur(x²) - mu²
template <bool FULL>
__device__ __forceinline__ float ssim_map(const float (&m)[5]) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1 = m[0], mu2 = m[1];
  const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
  const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu1_mu2;
  if (FULL) return ((2.f * mu1_mu2 + C1) * (2.f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
  return (2.f * s12 + C2) / (s1 + s2 + C2);
}

}  // namespace ssim
