// The sphere sampler (the definition is in include/pconv_hip.h, pconv_erp_remap_f32): an ERP plane of h x w read at a
// record (qu, qv) in 1/256 pixel through the 6 x 6 Lanczos-3 footprint of the phase table.  This header is the one
// place where the rule is written; the sphere rotation, the viewport renderer, the sphere points, the host's reverse
// lists and the pole rule of the resize all call it.
//   record      qu = the column * 256 modulo w * 256, qv = the row * 256 (any int): floor(q / 256) is the footprint's
//               centre tap (tap 2 of 6), q mod 256 the phase, whose row of the table holds the six weights.
//   columns     modulo w (wrap_col).
//   rows        the pole rule (pole_row): r < 0 -> -1 - r, r >= h -> 2h - 1 - r, then clamped to 0 .. h - 1; a row that
//               crossed a pole (judged before the clamp) reads its columns half a turn on (half_turn).
//   sums        b ascending inside a ascending, one fp32 rounding per product and per addition (apply).
// Every record is reduced to positions inside the plane, so no record content makes a caller read outside it.
#pragma once
#include <math.h>
#include "common.h"

constexpr int kPhases = PCONV_ERP_ROTATE_PHASES;
constexpr int kTaps = PCONV_ERP_ROTATE_TAPS;
constexpr double kPi = 3.14159265358979323846;
static_assert(kPi == 3.141592653589793 && 2.0 * kPi == 6.283185307179586, "one double, however many digits spell it");

// ---- the index rule: host and device ----

__host__ __device__ inline int wrap_col(int c, int w) {  // c mod w, non-negative
  const int r = c % w;
  return r < 0 ? r + w : r;
}

__host__ __device__ inline int half_turn(int c, int w) {  // 0 <= c < w
  const int t = c + w / 2;
  return t >= w ? t - w : t;
}

__host__ __device__ inline int pole_row(int r, int h, bool *crossed) {  // |r| < 2^30
  *crossed = r < 0 || r >= h;
  if (r < 0) r = -1 - r;
  else if (r >= h) r = 2 * h - 1 - r;
  return r < 0 ? 0 : r > h - 1 ? h - 1 : r;
}

// floor division and the non-negative remainder by 256, for a negative q as well (two's complement)
__host__ __device__ inline int record_tap0(int q) { return (q >> 8) - 2; }
__host__ __device__ inline int record_phase(int q) { return q & (kPhases - 1); }
// floor((q + 128) / 256) without the addition's overflow for a record near INT_MAX
__host__ __device__ inline int record_nearest(int q) { return (q >> 8) + (record_phase(q) >= kPhases / 2 ? 1 : 0); }

// the pixel of the plane that tap (a, b) of the record reads
__host__ __device__ inline long long tap_pixel(int qu, int qv, int a, int b, int h, int w) {
  bool crossed;
  const int r = pole_row(record_tap0(qv) + a, h, &crossed);
  const int c = wrap_col(record_tap0(qu) + b, w);
  return (long long)r * w + (crossed ? half_turn(c, w) : c);
}

// ---- records: device ----

__device__ __forceinline__ long long wrap_record(long long q, int w) {  // q mod w * 256, non-negative
  const long long period = (long long)w * kPhases;
  q %= period;
  return q < 0 ? q + period : q;
}

// source coordinates in pixels -> the record; |u| < w + 1, so the conversion of rint is exact
__device__ __forceinline__ int2 pack_record(double u, double v, int w) {
  return make_int2((int)wrap_record((long long)rint(u * kPhases), w), (int)rint(v * kPhases));
}

__device__ __forceinline__ int2 record_of_direction(double sx, double sy, double sz, int h, int w) {
  const double u = (atan2(sy, sx) / (2.0 * kPi) + 0.5) * w - 0.5;
  const double v = (0.5 - atan2(sz, hypot(sx, sy)) / kPi) * h - 0.5;
  return pack_record(u, v, w);
}

// ---- the sampler: device ----

// the cooperative copy of the phase table to LDS, by a workgroup of BLOCK lanes
template <int BLOCK>
__device__ __forceinline__ void stage_phase_table(float *table, const float *__restrict__ phases) {
  for (int k = threadIdx.x; k < kPhases * kTaps; k += BLOCK) table[k] = phases[k];
  __syncthreads();
}

// a record decoded for a plane of h x w: what `apply` needs and no plane has a part in.  The offsets are unsigned 32-bit
// (a plane is below 2^29 floats): the plane's base is the same for every lane, so 36 addresses of 64 bits are not kept
struct Footprint {
  float fx[kTaps], fy[kTaps];
  unsigned col[kTaps], turned[kTaps], row[kTaps];
  bool crossed[kTaps];
};

__device__ __forceinline__ Footprint footprint_of(int2 rec, const float *table, int h, int w) {
  Footprint f;
  const float *wx = table + record_phase(rec.x) * kTaps;
  const float *wy = table + record_phase(rec.y) * kTaps;
  const int row0 = record_tap0(rec.y);
  int cb = wrap_col(record_tap0(rec.x), w);  // the one division: the following columns wrap by comparison
#pragma unroll
  for (int b = 0; b < kTaps; b++) {
    f.fx[b] = wx[b];
    f.fy[b] = wy[b];
    f.col[b] = cb;
    f.turned[b] = half_turn(cb, w);
    cb = cb + 1 == w ? 0 : cb + 1;
    f.row[b] = (unsigned)pole_row(row0 + b, h, &f.crossed[b]) * (unsigned)w;
  }
  return f;
}

__device__ __forceinline__ float apply(const Footprint &f, const float *__restrict__ src) {
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < kTaps; a++) {
    float s = __fmul_rn(f.fx[0], src[f.row[a] + (f.crossed[a] ? f.turned[0] : f.col[0])]);
#pragma unroll
    for (int b = 1; b < kTaps; b++)
      s = __fadd_rn(s, __fmul_rn(f.fx[b], src[f.row[a] + (f.crossed[a] ? f.turned[b] : f.col[b])]));
    const float m = __fmul_rn(f.fy[a], s);
    acc = a == 0 ? m : __fadd_rn(acc, m);
  }
  return acc;
}

__device__ __forceinline__ float sample_lanczos(const float *__restrict__ src, int2 rec, const float *table, int h, int w) {
  return apply(footprint_of(rec, table, h, w), src);
}

__device__ __forceinline__ float sample_nearest(const float *__restrict__ src, int2 rec, int h, int w) {
  bool crossed;
  const int r = pole_row(record_nearest(rec.y), h, &crossed);
  const int c = wrap_col(record_nearest(rec.x), w);
  return src[(unsigned)r * (unsigned)w + (unsigned)(crossed ? half_turn(c, w) : c)];
}

// ---- the refusals the entry points share: host.  `what` is the entry point's name ----

inline uintptr_t addr(const void *p) { return reinterpret_cast<uintptr_t>(p); }

// kind: "" (a frame), "source " or "view "
inline int side_ok(const char *what, const char *kind, int h, int w) {
  PCONV_REQUIRE(h >= 2 && w >= 2 && h <= (1 << 20) && w <= (1 << 20), "%s: a %sside of %dx%d is outside 2 .. 2^20", what, kind,
                w, h);
  return PCONV_OK;
}

inline int frame_ok(const char *what, const char *kind, int h, int w) {
  if (side_ok(what, kind, h, w) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(4LL * h * w < (1LL << 31), "%s: a %splane of %dx%d float32 is 2^31 bytes or more", what, kind, w, h);
  return PCONV_OK;
}

inline int planes_ok(const char *what, int n, int c) {
  PCONV_REQUIRE(n > 0 && c > 0 && (long long)n * c <= 65535, "%s: n * C = %lld planes, the grid takes 1 .. 65535", what,
                (long long)n * c);
  return PCONV_OK;
}

// four / eight: the addresses that must be 4-byte / 8-byte aligned, or-ed together; fours / eights: what they are
inline int aligned_ok(const char *what, uintptr_t four, const char *fours, uintptr_t eight, const char *eights) {
  PCONV_REQUIRE((four & 3) == 0 && (eight & 7) == 0, "%s: %s must be 4-byte aligned, %s 8-byte aligned", what, fours, eights);
  return PCONV_OK;
}

inline int aligned8_ok(const char *what, uintptr_t eight, const char *eights) {
  PCONV_REQUIRE((eight & 7) == 0, "%s: %s must be 8-byte aligned", what, eights);
  return PCONV_OK;
}
