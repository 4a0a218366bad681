// Shared by sphere_metrics.hip and ws_msssim.hip: the tile geometry, the row weight, the pixel loads and the host
// checks of the sphere metrics.  Everything here has internal linkage.
#pragma once
#include <math.h>

#include "common.h"

namespace {

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
constexpr int kMaxSide = 1 << 20;
static_assert(kBlock == kTileCols * (kTileRows / kRowsPerLane), "vertical pass: one lane per (column, row group)");
static_assert(4 * (kQuads - 1) + 16 <= kLd, "horizontal pass: the last float4 read stays inside the staged row");

struct WsGeom {
  int c, h, w, tiles_x, tiles, uniform;
  float g[kTaps];  // the normalised 1-D Gaussian in fp32
};

__host__ __device__ inline double row_weight(int j, int h) {
  // ((j + 0.5)/h - 0.5)·pi with an exact integer numerator: rows j and h-1-j get the same weight bit for bit
  return cos((double)(2 * j + 1 - h) / (2.0 * h) * M_PI);
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

int ws_geom(const char *what, int n, int c, int h, int w, int weighting, WsGeom *G) {
  PCONV_REQUIRE(n >= 1 && n <= 65535, "%s: bad frame count %d", what, n);
  PCONV_REQUIRE(c >= 1 && c <= 4096, "%s: bad channel count %d", what, c);
  PCONV_REQUIRE(h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide, "%s: bad frame size %dx%d", what, w, h);
  PCONV_REQUIRE(3LL * h * w < (1LL << 31), "%s: a %dx%d frame exceeds 2^31 bytes per plane", what, w, h);
  PCONV_REQUIRE(weighting == PCONV_WS_WEIGHT_SPHERE || weighting == PCONV_WS_WEIGHT_UNIFORM,
                "%s: unknown weighting %d", what, weighting);
  G->c = c, G->h = h, G->w = w;
  G->tiles_x = (w + kTileCols - 1) / kTileCols;
  G->tiles = G->tiles_x * ((h + kTileRows - 1) / kTileRows);
  G->uniform = weighting == PCONV_WS_WEIGHT_UNIFORM;
  // pytorch_ssim.gaussian(11, 1.5): exp(-(k - 5)² / (2·1.5²)) in double, normalised; here in fp32
  double g[kTaps], sum = 0.0;
  for (int k = 0; k < kTaps; k++) sum += g[k] = exp(-(double)((k - kHalo) * (k - kHalo)) / (2.0 * 1.5 * 1.5));
  for (int k = 0; k < kTaps; k++) G->g[k] = (float)(g[k] / sum);
  return PCONV_OK;
}

// ---- the backward kernels' tile: inputs with a halo of 10, see sphere_metrics.hip ----
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

}  // namespace
