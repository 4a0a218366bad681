// Sphere-weighted quality of ERP frames, forward and backward: WS-PSNR / WS-SSIM and WS-MS-SSIM (DESIGN.md §4b;
// include/pconv_hip.h states the definitions).  Every row j of an h-row frame is weighted by the area it covers on the
// sphere, w_j = cos(((j + 0.5)/h - 0.5)·pi) (or 1: "uniform").  The SSIM map is pytorch_ssim's: 11-tap Gaussian
// (sigma 1.5) as the window g⊗g, zero padding of 5 on all four borders (the seam is not wrapped), C1 = 0.01²,
// C2 = 0.03², sigma² = blur(x²) - mu².  It is computed in fp32 with a separable filter; every sum is fp64.
// WS-MS-SSIM: five scales s = 0..4 of h >> s rows and w >> s columns, each the 2x2 mean of the one before; per scale
// the sphere-weighted mean of the contrast-structure map cs (s < 4) or of the full SSIM map l·cs (s = 4), with the row
// weights of an (h >> s)-row frame; WS-MS-SSIM = Π_s max(v_s, 0)^β_s.  WS-SSIM is the same chain with one scale, which
// is both the first (Σ w·(x - y)² is added) and the last (the full map): every kernel below serves both metrics.
//
// Forward: one launch of ms_forward_kernel per scale, one workgroup per (tile of 32 rows x 64 columns, frame).  Per
// channel it stages the 42 x 74 tile with its halo in LDS (zeros outside the frame), runs the horizontal pass into five
// moment planes (mu_x, mu_y, x², y², xy: 42 x 64 each, in LDS), then the vertical pass, 8 rows x 1 column per lane,
// evaluates the map and adds w_j·map (at the first scale also w_j·(x - y)²) into fp64 registers.  A wave butterfly and
// a fixed-order sum over the four waves give the tile's partials, stored to partials[frame][tile].  From the staged
// tile (the staging, the two passes and the map are the device functions of ssim_tile.h, which the weighted SSIM of
// weighted_metrics.hip calls too) it also writes the tile's 16 x 32 block of the next scale of x and of y: tile origins are even, so a 2x2 block
// never straddles tiles, and the pyramid costs no second read of the frame.  No atomics: ms_close_kernel, one workgroup
// per frame, adds each scale's partials in a fixed order and normalises, so a frame gives the same bits alone, in any
// batch and on every run.
//
// Backward: one launch of ms_backward_kernel per scale, coarse to fine: a gather (halo 10, five passes in LDS, every
// output stored once) with a compile-time switch between the cs-only and the full coefficients, the fused
// + 0.25f·g_{s+1}[r >> 1][q >> 1] read and, at scale 0, + km·(y - x).  The same kernel with a per-pixel factor read from
// a float64 weight plane is the backward of the weighted SSIM (pconv_weighted_ssim_backward_f32; launch_plane_backward).
#include "ssim_tile.h"

namespace {

// the tile, its constants, the staging and the two filter passes: ssim_tile.h, shared with weighted_metrics.hip
using namespace ssim;

constexpr int kMaxSide = 1 << 20;

__host__ __device__ inline double row_weight(int j, int h) {
  // ((j + 0.5)/h - 0.5)·pi with an exact integer numerator: rows j and h-1-j get the same weight bit for bit
  return cos((double)(2 * j + 1 - h) / (2.0 * h) * M_PI);
}

constexpr int kScales = 5;
constexpr int kOutCols = kScales + 2;  // v_0..v_4, WS-MSE, WS-MS-SSIM
__constant__ const double kBetaDev[kScales] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};  // Wang, Simoncelli, Bovik 2003

// the range checks of every entry; a chain of `scales` scales needs 1 << (scales - 1) pixels a side, or its last
// scale has none
int ws_sizes(const char *what, int scales, int n, int c, int h, int w) {
  const int min_side = 1 << (scales - 1);
  PCONV_REQUIRE(n >= 1 && n <= 65535, "%s: bad frame count %d", what, n);
  PCONV_REQUIRE(c >= 1 && c <= 4096, "%s: bad channel count %d", what, c);
  PCONV_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "%s: bad frame size %dx%d", what, w, h);
  PCONV_REQUIRE(h >= min_side && w >= min_side, "%s: h and w must be at least %d, got %dx%d", what, min_side, w, h);
  return PCONV_OK;
}

// f32_planes: the entry writes float32 planes (a pyramid, a gradient) that are addressed by 32-bit byte offsets
int ws_geom(const char *what, int scales, int n, int c, int h, int w, int weighting, bool f32_planes, WsGeom *G) {
  if (ws_sizes(what, scales, n, c, h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(3LL * h * w < (1LL << 31), "%s: a %dx%d frame exceeds 2^31 bytes per plane", what, w, h);
  PCONV_REQUIRE(weighting == PCONV_WS_WEIGHT_SPHERE || weighting == PCONV_WS_WEIGHT_UNIFORM,
                "%s: unknown weighting %d", what, weighting);
  PCONV_REQUIRE(!f32_planes || 4LL * h * w < (1LL << 31), "%s: a %dx%d plane has 2^31 bytes or more", what, w, h);
  G->c = c, G->h = h, G->w = w;
  G->tiles_x = (w + kTileCols - 1) / kTileCols;
  G->tiles = G->tiles_x * ((h + kTileRows - 1) / kTileRows);
  G->uniform = weighting == PCONV_WS_WEIGHT_UNIFORM;
  gaussian_taps(G->g);
  return PCONV_OK;
}

// ---- the backward kernel's tile: inputs with a halo of 10, see ms_backward_kernel ----
constexpr int kBHalo = 2 * kHalo;                 // 10: halo of the staged inputs
constexpr int kBBlock = 512;                      // two waves per SIMD: the 154 KB of LDS allow one workgroup per CU
constexpr int kBRows = kTileRows + 2 * kBHalo;    // 52 staged rows (of 84 columns) = rows of the horizontal moments
constexpr int kBLd = 88;                          // staged row stride: the last float4 read of pass B ends at 87
constexpr int kMLd = 76;                          // row stride of the 74 moment columns: 19 quads (74, 75 computed, unused)
constexpr int kMQuads = kMLd / 4;
constexpr int kPRows = kInRows;                   // 42 rows of ks·a, ks·b, ks·c
constexpr int kCRowsPerLane = 7;                  // pass C: 7 rows of one column per lane, 42 = 6 x 7
constexpr int kERowsPerLane = kTileRows * kTileCols / kBBlock;  // pass E: 4 rows of one column per lane
constexpr int kBStage = (kBRows * kBLd + kBBlock - 1) / kBBlock;
static_assert(kBBlock >= 64 + kTileRows && kTileRows % kERowsPerLane == 0, "pass E covers the tile in whole groups");
static_assert(kPRows % kCRowsPerLane == 0, "pass C covers the 42 rows in whole groups");
static_assert(4 * (kMQuads - 1) + 16 <= kBLd, "pass B: the last float4 read stays inside the staged row");
static_assert(4 * (kQuads - 1) + 16 <= kMLd, "pass D: the last float4 read stays inside the plane's row");
static_assert(3 * kPRows * kTileCols <= 5 * kBRows * kMLd, "pass D writes over the moment planes");

inline WsGeom scale_geom(const WsGeom &G0, int s) {
  WsGeom G = G0;
  G.h = G0.h >> s, G.w = G0.w >> s;
  G.tiles_x = (G.w + kTileCols - 1) / kTileCols;
  G.tiles = G.tiles_x * ((G.h + kTileRows - 1) / kTileRows);
  return G;
}

// N = C · w · Σ_j w_j: the sum j-ascending in double on the host, so that every workgroup divides by the same bits
inline double ws_norm(const WsGeom &G) {
  double sw = 0.0;
  for (int j = 0; j < G.h; j++) sw += G.uniform ? 1.0 : row_weight(j, G.h);
  return (double)G.c * (double)G.w * sw;
}

// the forward's workspace for a chain of `scales` scales: the pyramid x_1, y_1, ... (none for one scale), then the
// tiles' partials
struct MsLayout {
  long long level[kScales];     // floats from the workspace's start to x_s (s >= 1); y_s follows x_s
  long long partials[kScales];  // doubles from the partials' start to scale s
  long long pyramid_floats;     // all of x_1.. and y_1..
  long long partial_doubles;
  int tiles[kScales];
};

inline MsLayout ms_layout(int scales, int n, int c, int h, int w) {
  MsLayout L = {};
  long long fl = 0, db = 0;
  for (int s = 0; s < scales; s++) {
    const int hs = h >> s, ws = w >> s;
    L.tiles[s] = ((ws + kTileCols - 1) / kTileCols) * ((hs + kTileRows - 1) / kTileRows);
    L.level[s] = fl;
    if (s > 0) fl += 2LL * n * c * hs * ws;
    L.partials[s] = db;
    db += 2LL * n * L.tiles[s];
  }
  L.pyramid_floats = fl;  // even: the partials behind it stay 8-byte aligned
  L.partial_doubles = db;
  return L;
}

// FIRST: scale 0 (T may be uint8; Σ w·(x - y)² is accumulated).  FINAL: the last scale (the full map, no next scale).
// WS-SSIM is both at once.
template <typename T, bool FIRST, bool FINAL>
__global__ __launch_bounds__(kBlock, 2) void ms_forward_kernel(const T *__restrict__ x, const T *__restrict__ y,
                                                            float *__restrict__ nx, float *__restrict__ ny,
                                                            double *__restrict__ partials, WsGeom G, int h2, int w2) {
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
    stage_tile(xp, yp, G, ch, r0, c0, sx, sy);  // (its first barrier: the previous channel's vertical pass has read sx / sy / mom)
    // the next scale: the tile's 16 x 32 block of 2x2 means, ((p00 + p01) + (p10 + p11))·0.25f, from the staged tile.
    // A block inside the next scale lies inside this frame (2·(h >> 1) <= h) and inside this tile (even origin)
    if (!FINAL) {
      float *nxp = nx + ((long long)f * G.c + ch) * h2 * w2, *nyp = ny + ((long long)f * G.c + ch) * h2 * w2;
      for (int u = tid; u < (kTileRows / 2) * (kTileCols / 2); u += kBlock) {
        const int pj = u / (kTileCols / 2), pi = u - pj * (kTileCols / 2);
        const int gj = (r0 >> 1) + pj, gi = (c0 >> 1) + pi;
        if (gj < h2 && gi < w2) {
          const int o = (2 * pj + kHalo) * kLd + 2 * pi + kHalo;
          nxp[(unsigned)(gj * w2 + gi)] = ((sx[o] + sx[o + 1]) + (sx[o + kLd] + sx[o + kLd + 1])) * 0.25f;
          nyp[(unsigned)(gj * w2 + gi)] = ((sy[o] + sy[o + 1]) + (sy[o + kLd] + sy[o + kLd + 1])) * 0.25f;
        }
      }
    }
    float acc[kRowsPerLane][5];
    tile_moments(sx, sy, mom, G, rg, col, acc);
#pragma unroll
    for (int o = 0; o < kRowsPerLane; o++) {
      const int r = rg + o;
      if (r0 + r < G.h && c0 + col < G.w) {
        const float map = ssim_map<FINAL>(acc[o]);
        acc_s += wrow[r] * (double)map;
        if (FIRST) {
          const int centre = (r + kHalo) * kLd + col + kHalo;
          const float d = sx[centre] - sy[centre];
          const float e2 = d * d;
          acc_e += wrow[r] * (double)e2;
        }
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

struct MsClose {
  long long partials[kScales];  // doubles from the partials' start to scale s
  int tiles[kScales];
  int c, h, w, uniform;
};

// one workgroup per frame: per scale its tiles' partials and Σ_j w_j, each in a fixed order, then the normalisation.
// SCALES == kScales: out (n, 7) = v_0..v_4, WS-MSE, and the product, formed by thread 0.  SCALES == 1: out (n, 2) =
// WS-MSE, WS-SSIM, and no product
template <int SCALES>
__global__ __launch_bounds__(kBlock) void ms_close_kernel(const double *__restrict__ partials,
                                                          double *__restrict__ out, MsClose M) {
  __shared__ double red[3][kBlock];
  __shared__ double v[SCALES];
  constexpr int cols = SCALES == 1 ? 2 : kOutCols, mse_col = SCALES == 1 ? 0 : SCALES, v_col = SCALES == 1 ? 1 : 0;
  const int f = blockIdx.x, tid = threadIdx.x;
  for (int s = 0; s < SCALES; s++) {
    const int hs = M.h >> s, ws = M.w >> s, tiles = M.tiles[s];
    const double *p = partials + M.partials[s] + (long long)f * tiles * 2;
    double se = 0.0, ss = 0.0, sw = 0.0;
    for (int b = tid; b < tiles; b += kBlock) {
      se += p[2 * b];
      ss += p[2 * b + 1];
    }
    for (int j = tid; j < hs; j += kBlock) sw += M.uniform ? 1.0 : row_weight(j, hs);
    red[0][tid] = se;
    red[1][tid] = ss;
    red[2][tid] = sw;
    __syncthreads();
    for (int k = kBlock / 2; k > 0; k >>= 1) {
      if (tid < k) {
#pragma unroll
        for (int t = 0; t < 3; t++) red[t][tid] += red[t][tid + k];
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double norm = (double)M.c * (double)ws * red[2][0];
      v[s] = red[1][0] / norm;
      out[(long long)cols * f + v_col + s] = v[s];
      if (s == 0) out[(long long)cols * f + mse_col] = red[0][0] / norm;
    }
    __syncthreads();  // red is reused by the next scale
  }
  if (SCALES > 1 && tid == 0) {
    double ms = 1.0;
    for (int s = 0; s < SCALES; s++) ms *= pow(fmax(v[s], 0.0), kBetaDev[s]);
    out[(long long)cols * f + SCALES + 1] = ms;
  }
}

// A gather: one workgroup per (32 x 64 output tile, frame, channel), every output element stored exactly once.
//   A  stage x and y with a halo of 10 (52 x 84, zeros outside the frame)
//   B  horizontal pass -> the five moment planes on 52 rows x 74 columns
//   C  vertical pass -> the moments on the tile + a halo of 5 (42 x 74); from them k·a, k·b, k·c, zero outside the
//      frame, into three planes of their own
//   D  horizontal pass of these three planes -> 42 rows x 64 columns, over the moment planes (dead after C)
//   E  vertical pass -> blur(k·a), blur(k·b), blur(k·c) on the tile, the sum, one store per element
// Every 11-tap sum runs k-ascending as fmaf(g[k], v, acc) from acc = 0, the horizontal pass first.  No atomics; the
// upstream gradients are read from device memory.
// FULL: the last scale, the coefficients of the full map and no coarser gradient.  Otherwise the cs-only coefficients
// and + 0.25f·coarse[r >> 1][q >> 1].  FIRST: scale 0, + km·(y - x).  MULTI: the per-frame factor is u_s = gs·β_s·MS /
// v_s, formed in fp64 from the forward's saved values; otherwise (WS-SSIM, one scale) it is gs and `values` is not read.
// PLANE: the weighted SSIM over a weight plane (pconv_weighted_ssim_backward_f32): blockIdx.y counts planes (G.c is 1),
// gout holds one value per plane, `norm` is the plane's total W, and pass C takes its factor per pixel, k_p = gout·w_p / W,
// the weights of its 7 rows of one column read straight from global memory before the vertical pass starts (consecutive
// lanes read consecutive doubles of a row; nothing of the plane is staged: the 154 KB of LDS are taken).  No row factors.
template <bool FULL, bool FIRST, bool MULTI, bool PLANE = false>
__global__ __launch_bounds__(kBBlock) void ms_backward_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            const double *__restrict__ values,
                                                            const double *__restrict__ gout,
                                                            const float *__restrict__ coarse, float *__restrict__ gy,
                                                            WsGeom G, double norm, int scale, int h2, int w2,
                                                            const double *__restrict__ weights) {
  static_assert(!PLANE || (FULL && !FIRST && !MULTI), "the weight plane: one scale, the full map, no squared-error term");
  __shared__ __attribute__((aligned(16))) float sx[kBRows * kBLd];
  __shared__ __attribute__((aligned(16))) float sy[kBRows * kBLd];
  __shared__ __attribute__((aligned(16))) float mom[5 * kBRows * kMLd];
  __shared__ __attribute__((aligned(16))) float abc[3][kPRows * kMLd];
  __shared__ float ks_row[kPRows], km_row[kTileRows];
  float *const q = mom;  // pass D's three 42 x 64 planes
  const int tid = threadIdx.x, tile = blockIdx.x, f = blockIdx.y, ch = blockIdx.z;
  const int ty = tile / G.tiles_x;
  const int r0 = ty * kTileRows, c0 = (tile - ty * G.tiles_x) * kTileCols;
  // k_j = u_s·w_j / N_s with u_s = gs·β_s·MS / v_s (0 when any v_t <= 0; gs alone for one scale), and km_j =
  // 2·gm·w_j / N_0: fp64, each rounded once to fp32; k = 0 on rows outside the frame
  if (PLANE) {
    // the factor is per pixel: pass C forms it
  } else if (tid < kPRows) {
    const int gr = r0 - kHalo + tid;
    const bool in = gr >= 0 && gr < G.h;
    const double wj = G.uniform ? 1.0 : row_weight(in ? gr : 0, G.h);
    double u = gout[2 * f + 1];
    if (MULTI) {
      const double *v = values + (long long)kOutCols * f;
      bool positive = true;
#pragma unroll
      for (int t = 0; t < kScales; t++) positive = positive && v[t] > 0.0;
      u = positive ? u * kBetaDev[scale] * v[kScales + 1] / v[scale] : 0.0;
    }
    ks_row[tid] = in ? (float)(u * wj / norm) : 0.f;
  } else if (FIRST && tid >= 64 && tid < 64 + kTileRows) {
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
  // B: horizontal pass, 4 adjacent outputs of one staged row per lane
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
    // PLANE: the seven weights are asked for before the vertical pass; a pixel outside the plane reads none
    double wt[kCRowsPerLane];
    if (PLANE) {
#pragma unroll
      for (int o = 0; o < kCRowsPerLane; o++) {
        const int gr = r0 - kHalo + rg + o, gc = c0 - kHalo + col;
        const bool in = gr >= 0 && gr < G.h && gc >= 0 && gc < G.w;
        wt[o] = in ? weights[(unsigned)(gr * G.w + gc)] : 0.0;
      }
    }
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
      const float A2 = 2.f * s12 + C2, B2 = s1 + s2 + C2;
      float da, db, dc;
      if (FULL) {
        const float A1 = 2.f * mux_muy + C1, B1 = mux_sq + muy_sq + C1;
        const float D = B1 * B2;
        const float S = (A1 * A2) / D;
        db = -S / B2;
        dc = (2.f * A1) / D;
        da = (2.f * mux) * A2 / D - (2.f * muy) * S / B1 - mux * dc - (2.f * muy) * db;
      } else {
        const float S = A2 / B2;
        db = -S / B2;
        dc = 2.f / B2;
        da = (-mux * dc) - (2.f * muy) * db;
      }
      const float ks = PLANE ? (float)(__dmul_rn(gout[f], wt[o]) / norm) : ks_row[r];
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
  //   g = (blur(k·a) + (2·y)·blur(k·b)) + x·blur(k·c), + 0.25f·coarse[r >> 1][q >> 1] inside the coarser scale,
  //   + km·(y - x) at scale 0
  float *gp = gy + ((long long)f * G.c + ch) * G.h * G.w;
  const float *cp = FULL ? nullptr : coarse + ((long long)f * G.c + ch) * h2 * w2;
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
      const int r = rg + o, gr = r0 + r, gc = c0 + col;
      if (gr < G.h && gc < G.w) {
        const int centre = (r + kBHalo) * kBLd + col + kBHalo;
        const float xv = sx[centre], yv = sy[centre];
        float g = (acc[o][0] + (2.f * yv) * acc[o][1]) + xv * acc[o][2];
        if (!FULL) {
          const int cr = gr >> 1, cq = gc >> 1;
          if (cr < h2 && cq < w2) g = g + 0.25f * cp[(unsigned)(cr * w2 + cq)];
        }
        if (FIRST) g = g + km_row[r] * (yv - xv);
        gp[(unsigned)(gr * G.w + gc)] = g;
      }
    }
  }
}

// ---- host side: every entry is the chain of `scales` scales, 1 for WS-SSIM and kScales for WS-MS-SSIM ----

template <typename T>
int ws_forward(const char *what, int scales, const T *x, const T *y, int n, int c, int h, int w, int weighting,
               void *workspace, double *out, void *stream) {
  PCONV_REQUIRE(x && y && workspace && out, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
                "%s: workspace and out must be 8-byte aligned", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(x) % sizeof(T)) == 0 && (reinterpret_cast<uintptr_t>(y) % sizeof(T)) == 0,
                "%s: misaligned frames", what);
  WsGeom G0;
  if (ws_geom(what, scales, n, c, h, w, weighting, scales > 1, &G0) != PCONV_OK) return PCONV_EINVAL;
  const MsLayout L = ms_layout(scales, n, c, h, w);
  float *pyr = static_cast<float *>(workspace);
  double *partials = reinterpret_cast<double *>(pyr + L.pyramid_floats);
  hipStream_t st = as_stream(stream);
  for (int s = 0; s < scales; s++) {
    const WsGeom G = scale_geom(G0, s);
    const long long plane = (long long)n * c * G.h * G.w;
    const int h2 = G.h >> 1, w2 = G.w >> 1;
    const bool last = s + 1 == scales;
    float *nx = last ? nullptr : pyr + L.level[s + 1];
    float *ny = last ? nullptr : nx + (long long)n * c * h2 * w2;
    const float *xs = pyr + L.level[s], *ys = xs + plane;  // read at s > 0
    double *part = partials + L.partials[s];
    const dim3 grid(G.tiles, n), block(kBlock);
    if (s == 0 && last)
      hipLaunchKernelGGL((ms_forward_kernel<T, true, true>), grid, block, 0, st, x, y, nx, ny, part, G, h2, w2);
    else if (s == 0)
      hipLaunchKernelGGL((ms_forward_kernel<T, true, false>), grid, block, 0, st, x, y, nx, ny, part, G, h2, w2);
    else if (!last)
      hipLaunchKernelGGL((ms_forward_kernel<float, false, false>), grid, block, 0, st, xs, ys, nx, ny, part, G, h2, w2);
    else
      hipLaunchKernelGGL((ms_forward_kernel<float, false, true>), grid, block, 0, st, xs, ys, nx, ny, part, G, h2, w2);
    PCONV_LAUNCH_CHECK(what);
  }
  MsClose M = {};
  for (int s = 0; s < scales; s++) M.partials[s] = L.partials[s], M.tiles[s] = L.tiles[s];
  M.c = c, M.h = h, M.w = w, M.uniform = G0.uniform;
  if (scales == 1)
    hipLaunchKernelGGL(ms_close_kernel<1>, dim3(n), dim3(kBlock), 0, st, partials, out, M);
  else
    hipLaunchKernelGGL(ms_close_kernel<kScales>, dim3(n), dim3(kBlock), 0, st, partials, out, M);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

// pyr, values and grads (the forward's workspace and result, the coarser scales' gradients) are read at scales > 1
int ws_backward(const char *what, int scales, const float *x, const float *y, const float *pyr, const double *values,
                const double *gout, int n, int c, int h, int w, int weighting, int swapped, float *grads, float *grad_y,
                void *stream) {
  WsGeom G0;
  if (ws_geom(what, scales, n, c, h, w, weighting, true, &G0) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(swapped == 0 || swapped == 1, "%s: swapped must be 0 or 1, got %d", what, swapped);
  const MsLayout L = ms_layout(scales, n, c, h, w);
  hipStream_t st = as_stream(stream);
  for (int s = scales - 1; s >= 0; s--) {
    const WsGeom G = scale_geom(G0, s);
    const long long plane = (long long)n * c * G.h * G.w;
    const double norm = ws_norm(G);
    // the forward's workspace holds (first, second) of the forward call; swapped: y was its first picture
    const float *first = pyr + L.level[s], *second = first + plane;
    const float *xs = s == 0 ? x : (swapped ? second : first), *ys = s == 0 ? y : (swapped ? first : second);
    float *gs = s == 0 ? grad_y : grads + L.level[s] / 2;
    const float *coarse = s + 1 < scales ? grads + L.level[s + 1] / 2 : nullptr;
    const int h2 = G.h >> 1, w2 = G.w >> 1;
    const dim3 grid(G.tiles, n, c), block(kBBlock);
    if (scales == 1)
      hipLaunchKernelGGL((ms_backward_kernel<true, true, false>), grid, block, 0, st, xs, ys, values, gout, coarse, gs, G,
                         norm, s, h2, w2, nullptr);
    else if (s == scales - 1)
      hipLaunchKernelGGL((ms_backward_kernel<true, false, true>), grid, block, 0, st, xs, ys, values, gout, coarse, gs, G,
                         norm, s, h2, w2, nullptr);
    else if (s > 0)
      hipLaunchKernelGGL((ms_backward_kernel<false, false, true>), grid, block, 0, st, xs, ys, values, gout, coarse, gs, G,
                         norm, s, h2, w2, nullptr);
    else
      hipLaunchKernelGGL((ms_backward_kernel<false, true, true>), grid, block, 0, st, xs, ys, values, gout, coarse, gs, G,
                         norm, s, h2, w2, nullptr);
    PCONV_LAUNCH_CHECK(what);
  }
  return PCONV_OK;
}

}  // namespace

// the launch of pconv_weighted_ssim_backward_f32 (weighted_metrics.hip, which has checked every argument): the backward
// kernel above with its per-pixel factor, one workgroup per (tile, plane)
int ssim::launch_plane_backward(const char *what, const float *x, const float *y, const double *weights, double total,
                                const double *gout, int planes, int h, int w, float *grad_y, void *stream) {
  WsGeom G = {};
  G.c = 1, G.h = h, G.w = w;
  G.tiles_x = (w + kTileCols - 1) / kTileCols;
  G.tiles = G.tiles_x * ((h + kTileRows - 1) / kTileRows);  // a plane is below 2^29 pixels: below 2^26 tiles
  gaussian_taps(G.g);
  hipLaunchKernelGGL((ms_backward_kernel<true, false, false, true>), dim3(G.tiles, planes, 1), dim3(kBBlock), 0,
                     as_stream(stream), x, y, nullptr, gout, nullptr, grad_y, G, total, 0, 0, 0, weights);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

extern "C" long long pconv_ws_metrics_workspace_bytes(int n, int h, int w) {
  if (ws_sizes("ws_metrics_workspace_bytes", 1, n, 1, h, w) != PCONV_OK) return PCONV_EINVAL;
  return ms_layout(1, n, 1, h, w).partial_doubles * (long long)sizeof(double);
}

extern "C" int pconv_ws_metrics_f32(const float *x, const float *y, int n, int c, int h, int w, int weighting,
                                    void *workspace, double *out, void *stream) {
  return ws_forward("ws_metrics_f32", 1, x, y, n, c, h, w, weighting, workspace, out, stream);
}

extern "C" int pconv_ws_metrics_u8(const uint8_t *x, const uint8_t *y, int n, int c, int h, int w, int weighting,
                                   void *workspace, double *out, void *stream) {
  PCONV_REQUIRE(c == 3, "ws_metrics_u8: interleaved (n, h, w, 3) frames have 3 channels, got %d", c);
  return ws_forward("ws_metrics_u8", 1, x, y, n, c, h, w, weighting, workspace, out, stream);
}

extern "C" int pconv_ws_metrics_backward_f32(const float *x, const float *y, const double *gout, int n, int c, int h,
                                             int w, int weighting, float *grad_y, void *stream) {
  const char *what = "ws_metrics_backward_f32";
  PCONV_REQUIRE(x && y && gout && grad_y, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(grad_y) & 3) == 0 && (reinterpret_cast<uintptr_t>(gout) & 7) == 0,
                "%s: misaligned tensors", what);
  return ws_backward(what, 1, x, y, nullptr, nullptr, gout, n, c, h, w, weighting, 0, nullptr, grad_y, stream);
}

extern "C" long long pconv_ws_msssim_workspace_bytes(int n, int c, int h, int w) {
  if (ws_sizes("ws_msssim_workspace_bytes", kScales, n, c, h, w) != PCONV_OK) return PCONV_EINVAL;
  const MsLayout L = ms_layout(kScales, n, c, h, w);
  return L.pyramid_floats * (long long)sizeof(float) + L.partial_doubles * (long long)sizeof(double);
}

extern "C" int pconv_ws_msssim_f32(const float *x, const float *y, int n, int c, int h, int w, int weighting,
                                   void *workspace, double *out, void *stream) {
  return ws_forward("ws_msssim_f32", kScales, x, y, n, c, h, w, weighting, workspace, out, stream);
}

extern "C" int pconv_ws_msssim_u8(const uint8_t *x, const uint8_t *y, int n, int c, int h, int w, int weighting,
                                  void *workspace, double *out, void *stream) {
  PCONV_REQUIRE(c == 3, "ws_msssim_u8: interleaved (n, h, w, 3) frames have 3 channels, got %d", c);
  return ws_forward("ws_msssim_u8", kScales, x, y, n, c, h, w, weighting, workspace, out, stream);
}

extern "C" long long pconv_ws_msssim_backward_workspace_bytes(int n, int c, int h, int w) {
  if (ws_sizes("ws_msssim_backward_workspace_bytes", kScales, n, c, h, w) != PCONV_OK) return PCONV_EINVAL;
  return ms_layout(kScales, n, c, h, w).pyramid_floats / 2 * (long long)sizeof(float);
}

extern "C" int pconv_ws_msssim_backward_f32(const float *x, const float *y, const void *workspace, const double *values,
                                            const double *gout, int n, int c, int h, int w, int weighting, int swapped,
                                            void *backward_workspace, float *grad_y, void *stream) {
  const char *what = "ws_msssim_backward_f32";
  PCONV_REQUIRE(x && y && workspace && values && gout && backward_workspace && grad_y, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0 && (reinterpret_cast<uintptr_t>(y) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(grad_y) & 3) == 0 && (reinterpret_cast<uintptr_t>(gout) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(values) & 7) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(backward_workspace) & 3) == 0,
                "%s: misaligned tensors", what);
  return ws_backward(what, kScales, x, y, static_cast<const float *>(workspace), values, gout, n, c, h, w, weighting,
                     swapped, static_cast<float *>(backward_workspace), grad_y, stream);
}
