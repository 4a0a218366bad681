// WS-PSNR / WS-SSIM of ERP frames (include/pconv_hip.h).  Every row j of an h-row frame is weighted
// by the area it covers on the sphere, w_j = cos(((j + 0.5)/h - 0.5)·pi) (or 1: "uniform"); the two per-frame sums
//   Σ_c Σ_j Σ_i w_j·(x - y)²   and   Σ_c Σ_j Σ_i w_j·ssim_map
// come out of one fused kernel that reads each frame once.  The SSIM map is pytorch_ssim's: 11-tap Gaussian
// (sigma 1.5) as the window g⊗g, zero padding of 5 on all four borders (the seam is not wrapped), C1 = 0.01²,
// C2 = 0.03², sigma² = blur(x²) - mu².  It is computed in fp32 with a separable filter; every sum is fp64.
//
// One workgroup per (tile of 32 rows x 64 columns, frame).  Per channel it stages the 42 x 74 tile with its halo in
// LDS (zeros outside the frame), runs the horizontal pass into five moment planes (mu_x, mu_y, x², y², xy: 42 x 64
// each, in LDS), then the vertical pass, 8 rows x 1 column per lane, evaluates the map and adds w_j·map and
// w_j·(x - y)² into two fp64 registers.  A wave butterfly and a fixed-order sum over the four waves give the tile's
// partials, stored to partials[frame][tile].  No atomics: a second launch adds each frame's partials in a fixed
// order, so a frame gives the same bits alone, in any batch and on every run.
#include "ws_common.h"

namespace {


template <typename T>
__global__ __launch_bounds__(kBlock, 2) void ws_metrics_kernel(const T *__restrict__ x, const T *__restrict__ y,
                                                            double *__restrict__ partials, WsGeom G) {
  __shared__ __attribute__((aligned(16))) float sx[kInRows * kLd];
  __shared__ __attribute__((aligned(16))) float sy[kInRows * kLd];
  __shared__ __attribute__((aligned(16))) float mom[5][kPlane];
  __shared__ double wrow[kTileRows];
  __shared__ double red[2][kWaves];
  const int tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y;
  const int ty = tile / G.tiles_x;
  const int r0 = ty * kTileRows, c0 = (tile - ty * G.tiles_x) * kTileCols;
  if (tid < kTileRows) wrow[tid] = G.uniform ? 1.0 : row_weight(min(r0 + tid, G.h - 1), G.h);
  const int col = tid & 63, rg = (tid >> 6) * kRowsPerLane;  // vertical pass: column, first row of the group
  double acc_e = 0.0, acc_s = 0.0;
  for (int ch = 0; ch < G.c; ch++) {
    const T *xp = plane_of(x, G, f, ch), *yp = plane_of(y, G, f, ch);
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
    __syncthreads();  // the previous channel's vertical pass has read sx / sy / mom
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
    float acc[kRowsPerLane][5];
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
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
    for (int o = 0; o < kRowsPerLane; o++) {
      const int r = rg + o;
      if (r0 + r < G.h && c0 + col < G.w) {
        const float mu1 = acc[o][0], mu2 = acc[o][1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
        const float s1 = acc[o][2] - mu1_sq, s2 = acc[o][3] - mu2_sq, s12 = acc[o][4] - mu1_mu2;
        const float map = ((2.f * mu1_mu2 + C1) * (2.f * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        const int centre = (r + kHalo) * kLd + col + kHalo;
        const float d = sx[centre] - sy[centre];
        const float e2 = d * d;
        acc_e += wrow[r] * (double)e2;
        acc_s += wrow[r] * (double)map;
      }
    }
  }
  acc_e = wave_sum(acc_e);
  acc_s = wave_sum(acc_s);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = acc_e;
    red[1][tid >> 6] = acc_s;
  }
  __syncthreads();
  if (tid < 2) {
    double s = red[tid][0];
#pragma unroll
    for (int k = 1; k < kWaves; k++) s += red[tid][k];
    partials[((long long)f * G.tiles + tile) * 2 + tid] = s;
  }
}

// one workgroup per frame: its tiles' partials and Σ_j w_j, each in a fixed order, then the normalisation
__global__ __launch_bounds__(kBlock) void ws_metrics_sum_kernel(const double *__restrict__ partials,
                                                                double *__restrict__ out, WsGeom G) {
  __shared__ double red[3][kBlock];
  const int f = blockIdx.x, tid = threadIdx.x;
  const double *p = partials + (long long)f * G.tiles * 2;
  double se = 0.0, ss = 0.0, sw = 0.0;
  for (int b = tid; b < G.tiles; b += kBlock) {
    se += p[2 * b];
    ss += p[2 * b + 1];
  }
  for (int j = tid; j < G.h; j += kBlock) sw += G.uniform ? 1.0 : row_weight(j, G.h);
  red[0][tid] = se;
  red[1][tid] = ss;
  red[2][tid] = sw;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int t = 0; t < 3; t++) red[t][tid] += red[t][tid + s];
    }
    __syncthreads();
  }
  if (tid < 2) out[2 * f + tid] = red[tid][0] / ((double)G.c * (double)G.w * red[2][0]);
}


template <typename T>
int ws_metrics(const char *what, const T *x, const T *y, int n, int c, int h, int w, int weighting, void *workspace,
               double *out, void *stream) {
  PCONV_REQUIRE(x && y && workspace && out, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                "%s: workspace and out must be 8-byte aligned", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(x) % sizeof(T)) == 0 && (reinterpret_cast<uintptr_t>(y) % sizeof(T)) == 0,
                "%s: misaligned frames", what);
  WsGeom G;
  if (ws_geom(what, n, c, h, w, weighting, &G) != PCONV_OK) return PCONV_EINVAL;
  double *partials = static_cast<double *>(workspace);
  hipLaunchKernelGGL(ws_metrics_kernel<T>, dim3(G.tiles, n), dim3(kBlock), 0, as_stream(stream), x, y, partials, G);
  PCONV_LAUNCH_CHECK(what);
  hipLaunchKernelGGL(ws_metrics_sum_kernel, dim3(n), dim3(kBlock), 0, as_stream(stream), partials, out, G);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

// ---- backward of WS-MSE + WS-SSIM with respect to y (include/pconv_hip.h states the definition) ----
// A gather: one workgroup per (32 x 64 output tile, frame, channel), every output element stored exactly once.
//   A  stage x and y with a halo of 10 (52 x 84, zeros outside the frame)
//   B  horizontal pass -> the five moment planes on 52 rows x 74 columns
//   C  vertical pass -> the moments on the tile + a halo of 5 (42 x 74); from them ks·a, ks·b, ks·c, zero outside the
//      frame, into three planes of their own
//   D  horizontal pass of these three planes -> 42 rows x 64 columns, over the moment planes (dead after C)
//   E  vertical pass -> blur(ks·a), blur(ks·b), blur(ks·c) on the tile, the four-term sum, one store per element
// Every 11-tap sum runs k-ascending as fmaf(g[k], v, acc) from acc = 0, the horizontal pass first.  No atomics, no
// workspace; the upstream gradients are read from device memory.

__global__ __launch_bounds__(kBBlock) void ws_metrics_backward_kernel(const float *__restrict__ x,
                                                                    const float *__restrict__ y,
                                                                    const double *__restrict__ gout,
                                                                    float *__restrict__ gy, WsGeom G, double norm) {
  __shared__ __attribute__((aligned(16))) float sx[kBRows * kBLd];
  __shared__ __attribute__((aligned(16))) float sy[kBRows * kBLd];
  __shared__ __attribute__((aligned(16))) float mom[5 * kBRows * kMLd];
  __shared__ __attribute__((aligned(16))) float abc[3][kPRows * kMLd];
  __shared__ float ks_row[kPRows], km_row[kTileRows];
  float *const q = mom;  // pass D's three 42 x 64 planes
  const int tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y, ch = blockIdx.z;
  const int ty = tile / G.tiles_x;
  const int r0 = ty * kTileRows, c0 = (tile - ty * G.tiles_x) * kTileCols;
  // ks_j = gs·w_j / N and km_j = 2·gm·w_j / N in fp64, each rounded once to fp32; ks = 0 on rows outside the frame
  if (tid < kPRows) {
    const int gr = r0 - kHalo + tid;
    const bool in = gr >= 0 && gr < G.h;
    const double wj = G.uniform ? 1.0 : row_weight(in ? gr : 0, G.h);
    ks_row[tid] = in ? (float)(gout[2 * f + 1] * wj / norm) : 0.f;
  } else if (tid >= 64 && tid < 64 + kTileRows) {
    const int gr = min(r0 + tid - 64, G.h - 1);
    const double wj = G.uniform ? 1.0 : row_weight(gr, G.h);
    km_row[tid - 64] = (float)(2.0 * gout[2 * f] * wj / norm);
  }
  const float *xp = plane_of(x, G, f, ch), *yp = plane_of(y, G, f, ch);
  // A: stage the inputs
#pragma unroll
  for (int k = 0; k < kBStage; k++) {
    const int e = tid + k * kBBlock;
    if (e < kBRows * kBLd) {
      const int rr = e / kBLd, cc = e - rr * kBLd;
      const int gr = r0 - kBHalo + rr, gc = c0 - kBHalo + cc;
      const bool in = gr >= 0 && gr < G.h && gc >= 0 && gc < G.w;
      sx[e] = in ? load_px(xp, G, ch, gr, gc) : 0.f;
      sy[e] = in ? load_px(yp, G, ch, gr, gc) : 0.f;
    }
  }
  __syncthreads();
  // B: horizontal pass, 4 adjacent outputs of one staged row per lane (as ws_metrics_kernel)
  for (int u = tid; u < kBRows * kMQuads; u += kBBlock) {
    const int rr = u / kMQuads, qd = u - rr * kMQuads;
    float a[16], b[16];
#pragma unroll
    for (int v = 0; v < 4; v++) {
      const float4 av = *reinterpret_cast<const float4 *>(sx + rr * kBLd + 4 * qd + 4 * v);
      const float4 bv = *reinterpret_cast<const float4 *>(sy + rr * kBLd + 4 * qd + 4 * v);
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
      *reinterpret_cast<float4 *>(mom + (t * kBRows + rr) * kMLd + 4 * qd) = make_float4(m[t][0], m[t][1], m[t][2], m[t][3]);
  }
  __syncthreads();
  // C: vertical pass, rows rg..rg+6 of one column per lane from moment rows rg..rg+16; then the three derivatives
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  for (int u = tid; u < (kPRows / kCRowsPerLane) * kMLd; u += kBBlock) {
    const int grp = u / kMLd, col = u - grp * kMLd, rg = grp * kCRowsPerLane;
    float acc[kCRowsPerLane][5];
#pragma unroll
    for (int o = 0; o < kCRowsPerLane; o++)
#pragma unroll
      for (int t = 0; t < 5; t++) acc[o][t] = 0.f;
#pragma unroll
    for (int i = 0; i < kCRowsPerLane + 2 * kHalo; i++) {
      float v[5];
#pragma unroll
      for (int t = 0; t < 5; t++) v[t] = mom[(t * kBRows + rg + i) * kMLd + col];
#pragma unroll
      for (int o = 0; o < kCRowsPerLane; o++) {
        if (i - o >= 0 && i - o < kTaps) {
#pragma unroll
          for (int t = 0; t < 5; t++) acc[o][t] = fmaf(G.g[i - o], v[t], acc[o][t]);
        }
      }
    }
    const int gc = c0 - kHalo + col;
#pragma unroll
    for (int o = 0; o < kCRowsPerLane; o++) {
      const int r = rg + o, gr = r0 - kHalo + r;
      const bool in = gr >= 0 && gr < G.h && gc >= 0 && gc < G.w;
      const float mux = acc[o][0], muy = acc[o][1];
      const float mux_sq = mux * mux, muy_sq = muy * muy, mux_muy = mux * muy;
      const float s1 = acc[o][2] - mux_sq, s2 = acc[o][3] - muy_sq, s12 = acc[o][4] - mux_muy;
      const float A1 = 2.f * mux_muy + C1, A2 = 2.f * s12 + C2, B1 = mux_sq + muy_sq + C1, B2 = s1 + s2 + C2;
      const float D = B1 * B2;
      const float S = (A1 * A2) / D;
      const float db = -S / B2;
      const float dc = (2.f * A1) / D;
      const float da = (2.f * mux) * A2 / D - (2.f * muy) * S / B1 - mux * dc - (2.f * muy) * db;
      const float ks = ks_row[r];
      abc[0][r * kMLd + col] = in ? ks * da : 0.f;
      abc[1][r * kMLd + col] = in ? ks * db : 0.f;
      abc[2][r * kMLd + col] = in ? ks * dc : 0.f;
    }
  }
  __syncthreads();  // the moment planes are dead: pass D writes over them
  // D: horizontal pass of the three planes, 4 adjacent outputs per lane
  for (int u = tid; u < kPRows * kQuads; u += kBBlock) {
    const int rr = u / kQuads, qd = u - rr * kQuads;
#pragma unroll
    for (int t = 0; t < 3; t++) {
      float a[16];
#pragma unroll
      for (int v = 0; v < 4; v++) {
        const float4 av = *reinterpret_cast<const float4 *>(&abc[t][rr * kMLd + 4 * qd + 4 * v]);
        a[4 * v] = av.x, a[4 * v + 1] = av.y, a[4 * v + 2] = av.z, a[4 * v + 3] = av.w;
      }
      float m[4];
#pragma unroll
      for (int o = 0; o < 4; o++) {
        m[o] = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; k++) m[o] = fmaf(G.g[k], a[o + k], m[o]);
      }
      *reinterpret_cast<float4 *>(q + (t * kPRows + rr) * kTileCols + 4 * qd) = make_float4(m[0], m[1], m[2], m[3]);
    }
  }
  __syncthreads();
  // E: vertical pass, rows rg..rg+3 of one column per lane, then
  //   gy = ((blur(ks·a) + (2·y)·blur(ks·b)) + x·blur(ks·c)) + km·(y - x)
  float *gp = gy + ((long long)f * G.c + ch) * G.h * G.w;
  for (int u = tid; u < (kTileRows / kERowsPerLane) * kTileCols; u += kBBlock) {
    const int col = u & (kTileCols - 1), rg = (u / kTileCols) * kERowsPerLane;
    float acc[kERowsPerLane][3];
#pragma unroll
    for (int o = 0; o < kERowsPerLane; o++)
#pragma unroll
      for (int t = 0; t < 3; t++) acc[o][t] = 0.f;
#pragma unroll
    for (int i = 0; i < kERowsPerLane + 2 * kHalo; i++) {
      float v[3];
#pragma unroll
      for (int t = 0; t < 3; t++) v[t] = q[(t * kPRows + rg + i) * kTileCols + col];
#pragma unroll
      for (int o = 0; o < kERowsPerLane; o++) {
        if (i - o >= 0 && i - o < kTaps) {
#pragma unroll
          for (int t = 0; t < 3; t++) acc[o][t] = fmaf(G.g[i - o], v[t], acc[o][t]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < kERowsPerLane; o++) {
      const int r = rg + o;
      if (r0 + r < G.h && c0 + col < G.w) {
        const int centre = (r + kBHalo) * kBLd + col + kBHalo;
        const float xv = sx[centre], yv = sy[centre];
        gp[(unsigned)((r0 + r) * G.w + c0 + col)] =
            ((acc[o][0] + (2.f * yv) * acc[o][1]) + xv * acc[o][2]) + km_row[r] * (yv - xv);
      }
    }
  }
}

}  // namespace

extern "C" int pconv_ws_metrics_backward_f32(const float *x, const float *y, const double *gout, int n, int c, int h,
                                             int w, int weighting, float *grad_y, void *stream) {
  const char *what = "ws_metrics_backward_f32";
  PCONV_REQUIRE(x && y && gout && grad_y, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(grad_y) & 3) == 0 && (reinterpret_cast<uintptr_t>(gout) & 7) == 0,
                "%s: misaligned tensors", what);
  WsGeom G;
  if (ws_geom(what, n, c, h, w, weighting, &G) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a %dx%d plane has 2^31 bytes or more", what, w, h);
  // N = C · w · Σ_j w_j: the sum j-ascending in double on the host, so that every workgroup divides by the same bits
  double sw = 0.0;
  for (int j = 0; j < h; j++) sw += G.uniform ? 1.0 : row_weight(j, h);
  const double norm = (double)c * (double)w * sw;
  hipLaunchKernelGGL(ws_metrics_backward_kernel, dim3(G.tiles, n, c), dim3(kBBlock), 0, as_stream(stream), x, y, gout,
                     grad_y, G, norm);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

extern "C" long long pconv_ws_metrics_workspace_bytes(int n, int h, int w) {
  PCONV_REQUIRE(n >= 1 && n <= 65535, "ws_metrics_workspace_bytes: bad frame count %d", n);
  PCONV_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "ws_metrics_workspace_bytes: bad frame size %dx%d",
                w, h);
  const long long tiles = (long long)((w + kTileCols - 1) / kTileCols) * ((h + kTileRows - 1) / kTileRows);
  return (long long)n * tiles * 2 * (long long)sizeof(double);
}

extern "C" int pconv_ws_metrics_f32(const float *x, const float *y, int n, int c, int h, int w, int weighting,
                                    void *workspace, double *out, void *stream) {
  return ws_metrics("ws_metrics_f32", x, y, n, c, h, w, weighting, workspace, out, stream);
}

extern "C" int pconv_ws_metrics_u8(const uint8_t *x, const uint8_t *y, int n, int c, int h, int w, int weighting,
                                   void *workspace, double *out, void *stream) {
  PCONV_REQUIRE(c == 3, "ws_metrics_u8: interleaved (n, h, w, 3) frames have 3 channels, got %d", c);
  return ws_metrics("ws_metrics_u8", x, y, n, c, h, w, weighting, workspace, out, stream);
}
