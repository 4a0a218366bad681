// Sphere-aware Lanczos-3 resize of ERP frames (the definition is in include/pconv_hip.h,
// pconv_host_lanczos_taps / pconv_erp_resample_f32): float32 (n, C, h, w) -> (n, C, h2, w2), separable, the seam
// wrapped in the horizontal pass, the poles continued (mirrored row, longitude + half a turn) in the vertical one.
// The tap tables are computed on the host, in double, by the one function below; the two kernels only apply them,
// t-ascending, one fp32 rounding per product and per addition.
//   rows pass:    in (n*C*h rows of w) -> mid (rows of w2).  A workgroup takes R consecutive rows x one tile of
//                 kTile output columns: the source span of the tile, with its wrapped halo, is staged in LDS
//                 (16-byte loads where the rows are 16-byte multiples), then lane l produces outputs l, l + 256,
//                 l + 512, l + 768 of the tile for each of the R rows (neighbouring lanes read LDS addresses
//                 w/w2 dwords apart; the stores of a wave are 256 contiguous bytes).  A weight row is read once
//                 for the R rows, from the table's first period (rows repeat bit for bit with period w2 / gcd).
//   columns pass: mid (n*C, h, w2) -> out (n*C, h2, w2).  A lane owns 4 adjacent columns of one output row and walks
//                 the row's taps (row index and weight are wave-uniform): 16-byte loads where w2 % 4 == 0, for rows
//                 that crossed a pole only where floor(w2/2) % 4 == 0 as well, else 4-byte loads.
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 4 * kBlock;       // output columns of one workgroup, both passes
constexpr int kMaxLdsBytes = 64 * 1024;  // rows pass: R rows of the staged span

// Floats of LDS one staged row needs for a tile of kTile outputs: the span first[i0 + kTile - 1] + T - first[i0] is at
// most floor((kTile - 1) * n_in / n_out) + 1 + T (first advances by floor or ceil of n_in / n_out per output), plus 3
// for the base rounded down to a quad, rounded up to a quad.
inline int span_floats(int n_in, int n_out, int T) {
  const long long s = ((long long)(kTile - 1) * n_in) / n_out + 2 + T + 3;
  return (int)((s + 3) & ~3LL);
}

template <int R>
__global__ __launch_bounds__(kBlock) void erp_resample_rows_kernel(const float *__restrict__ in, float *__restrict__ mid,
                                                                   const int *__restrict__ first,
                                                                   const float *__restrict__ wgt, int T, int period,
                                                                   long long rows, int w, int w2, int S, int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long long row0 = (long long)blockIdx.x * R;
  const int i0 = blockIdx.y * kTile;
  const int i1 = min(i0 + kTile, w2);
  int base = first[i0];
  if (vec) base &= ~3;  // two's complement: rounds a negative base down as well
  const int span = min(first[i1 - 1] + T - base, S);
#pragma unroll
  for (int r = 0; r < R; r++) {
    if (row0 + r >= rows) break;
    const float *src = in + (row0 + r) * w;
    float *dst = lds + r * S;
    if (vec) {  // w % 4 == 0, base % 4 == 0, rows 16-byte aligned: a quad never straddles the seam
      for (int q = threadIdx.x; 4 * q < span; q += kBlock) {
        int c = base + 4 * q;
        if (c < 0 || c >= w) c = wrap_col(c, w);
        *reinterpret_cast<float4 *>(dst + 4 * q) = *reinterpret_cast<const float4 *>(src + c);
      }
    } else {
      for (int s = threadIdx.x; s < span; s += kBlock) {
        int c = base + s;
        if (c < 0 || c >= w) c = wrap_col(c, w);
        dst[s] = src[c];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int i = i0 + j * kBlock + threadIdx.x;
    if (i >= i1) break;
    const int off = first[i] - base;
    const float *wr = wgt + (long long)(i % period) * T;
    float acc[R];
    {
      const float wt = wr[0];
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = __fmul_rn(wt, lds[r * S + off]);
    }
    for (int t = 1; t < T; t++) {
      const float wt = wr[t];
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = __fadd_rn(acc[r], __fmul_rn(wt, lds[r * S + off + t]));
    }
#pragma unroll
    for (int r = 0; r < R; r++)
      if (row0 + r < rows) mid[(row0 + r) * w2 + i] = acc[r];
  }
}

// vec: 0 = 4-byte accesses; 1 = 16-byte loads on rows that did not cross a pole and 16-byte stores; 2 = on all rows
__global__ __launch_bounds__(kBlock) void erp_resample_cols_kernel(const float *__restrict__ mid, float *__restrict__ out,
                                                                   const int *__restrict__ first,
                                                                   const float *__restrict__ wgt, int T, int h, int h2,
                                                                   int w2, int clamp, int vec) {
  const int j = blockIdx.x, p = blockIdx.z;
  const int x0 = blockIdx.y * kTile + 4 * threadIdx.x;
  if (x0 >= w2) return;
  const int nx = min(4, w2 - x0);  // 4 wherever vec != 0
  const int half = w2 / 2;
  const float *plane = mid + (long long)p * h * w2;
  const float *wr = wgt + (long long)j * T;
  const int r0 = first[j];
  int xf[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    xf[k] = min(x0 + k, w2 - 1) + half;
    if (xf[k] >= w2) xf[k] -= w2;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; t++) {
    bool flip;
    const int r = pole_row(r0 + t, h, &flip);
    const float *src = plane + (long long)r * w2;
    float v[4];
    if (vec == 2 || (vec == 1 && !flip)) {
      const float4 q = *reinterpret_cast<const float4 *>(src + (flip ? xf[0] : x0));
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = src[flip ? xf[k] : min(x0 + k, w2 - 1)];
    }
    const float wt = wr[t];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float m = __fmul_rn(wt, v[k]);
      acc[k] = t == 0 ? m : __fadd_rn(acc[k], m);
    }
  }
  if (clamp) {
#pragma unroll
    for (int k = 0; k < 4; k++) acc[k] = fminf(fmaxf(acc[k], 0.f), 1.f);
  }
  float *dst = out + ((long long)p * h2 + j) * w2 + x0;
  if (vec) {
    *reinterpret_cast<float4 *>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < nx) dst[k] = acc[k];
  }
}

inline long long floor_div(long long a, long long b) {  // b > 0
  long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

inline long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b, b = t;
  }
  return a;
}

int axis_ok(const char *what, int n_in, int n_out) {
  PCONV_REQUIRE(n_in >= 2 && n_out >= 2 && n_in <= (1 << 20) && n_out <= (1 << 20),
                "%s: a side of %d -> %d is outside 2 .. 2^20", what, n_in, n_out);
  PCONV_REQUIRE((long long)n_in <= 8LL * n_out, "%s: %d -> %d shrinks by more than 8:1", what, n_in, n_out);
  return PCONV_OK;
}

// first tap of output i and the number of taps: all k with |N(i, k)| < 3D, N = 2*n_out*k - (2i+1)*n_in + n_out
inline void tap_range(long long n_in, long long n_out, long long D, long long i, long long *k0, int *count) {
  const long long c = (2 * i + 1) * n_in - n_out;             // N = 2*n_out*k - c
  const long long lo = floor_div(c - 3 * D, 2 * n_out) + 1;   // smallest k with N > -3D
  const long long hi = floor_div(c + 3 * D - 1, 2 * n_out);   // largest k with N < 3D
  *k0 = lo;
  *count = (int)(hi - lo + 1);
}

}  // namespace

extern "C" int pconv_host_lanczos_taps(int n_in, int n_out, int32_t *first, float *weights, int *taps) {
  PCONV_REQUIRE(taps, "host_lanczos_taps: null pointer");
  PCONV_REQUIRE((first == nullptr) == (weights == nullptr), "host_lanczos_taps: first and weights go together");
  if (axis_ok("host_lanczos_taps", n_in, n_out) != PCONV_OK) return PCONV_EINVAL;
  const long long D = 2LL * (n_in > n_out ? n_in : n_out);
  int T = 0;
  for (long long i = 0; i < n_out; i++) {
    long long k0;
    int count;
    tap_range(n_in, n_out, D, i, &k0, &count);
    if (count > T) T = count;
  }
  *taps = T;
  if (!first) return PCONV_OK;
  double raw[64];  // T <= 48: the open interval |N| < 3D holds fewer than 6 * 8 + 1 integers k
  for (long long i = 0; i < n_out; i++) {
    long long k0;
    int count;
    tap_range(n_in, n_out, D, i, &k0, &count);
    double sum = 0.0;
    for (int t = 0; t < count; t++) {
      const long long N = 2LL * n_out * (k0 + t) - (2 * i + 1) * n_in + n_out;
      double r;
      if (N == 0) {
        r = 1.0;
      } else if (N % D == 0) {
        r = 0.0;
      } else {
        const double x = kPi * (double)(N < 0 ? -N : N) / (double)D;
        r = 3.0 * sin(x) * sin(x / 3.0) / (x * x);
      }
      raw[t] = r;
      sum += r;
    }
    first[i] = (int32_t)k0;
    for (int t = 0; t < T; t++) weights[i * T + t] = t < count ? (float)(raw[t] / sum) : 0.0f;
  }
  return PCONV_OK;
}

extern "C" long long pconv_erp_resample_workspace_bytes(int n, int c, int h, int w, int h2, int w2) {
  if (n <= 0 || c <= 0 || (long long)n * c > 65535 || h < 2 || w < 2 || h2 < 2 || w2 < 2 || h > (1 << 20) ||
      w > (1 << 20) || h2 > (1 << 20) || w2 > (1 << 20)) {
    pconv_set_error("erp_resample_workspace_bytes: bad shape (%d, %d, %d, %d) -> %dx%d", n, c, h, w, w2, h2);
    return PCONV_EINVAL;
  }
  return 4LL * n * c * h * w2;  // the horizontal pass's picture, rounded to float32
}

extern "C" int pconv_erp_resample_f32(const float *in, float *out, void *workspace, const int32_t *first_x,
                                      const float *wx, int tx, const int32_t *first_y, const float *wy, int ty, int n,
                                      int c, int h, int w, int h2, int w2, int clamp, void *stream) {
  PCONV_REQUIRE(in && out && workspace && first_x && wx && first_y && wy, "erp_resample_f32: null pointer");
  if (planes_ok("erp_resample_f32", n, c) != PCONV_OK) return PCONV_EINVAL;
  if (axis_ok("erp_resample_f32", w, w2) != PCONV_OK || axis_ok("erp_resample_f32", h, h2) != PCONV_OK) return PCONV_EINVAL;
  int want_tx = 0, want_ty = 0;
  if (pconv_host_lanczos_taps(w, w2, nullptr, nullptr, &want_tx) != PCONV_OK ||
      pconv_host_lanczos_taps(h, h2, nullptr, nullptr, &want_ty) != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(tx == want_tx && ty == want_ty, "erp_resample_f32: tap counts %d, %d are not those of the tables (%d, %d)",
                tx, ty, want_tx, want_ty);
  const uintptr_t ai = reinterpret_cast<uintptr_t>(in), ao = reinterpret_cast<uintptr_t>(out),
                  am = reinterpret_cast<uintptr_t>(workspace);
  PCONV_REQUIRE(((ai | ao | am) & 3) == 0, "erp_resample_f32: the tensors must be 4-byte aligned");
  float *mid = static_cast<float *>(workspace);
  const long long rows = (long long)n * c * h;
  const int S = span_floats(w, w2, tx);
  const int R = 4 * S * 4 <= kMaxLdsBytes ? 4 : (2 * S * 4 <= kMaxLdsBytes ? 2 : 1);
  PCONV_REQUIRE(S * 4 <= kMaxLdsBytes, "erp_resample_f32: a tile's source span of %d floats exceeds LDS", S);
  const long long groups = (rows + R - 1) / R;
  PCONV_REQUIRE(groups <= 0x7fffffffLL, "erp_resample_f32: %lld rows exceed the grid", rows);
  const int tiles = (w2 + kTile - 1) / kTile;
  const int period = (int)(w2 / gcd_ll(w, w2));
  const int vec_rows = (w % 4 == 0 && (ai & 15) == 0) ? 1 : 0;
  const dim3 grid_rows((unsigned)groups, tiles);
  const size_t lds = (size_t)R * S * 4;
  hipStream_t st = as_stream(stream);
  if (R == 4)
    hipLaunchKernelGGL(erp_resample_rows_kernel<4>, grid_rows, dim3(kBlock), lds, st, in, mid, first_x, wx, tx, period, rows,
                       w, w2, S, vec_rows);
  else if (R == 2)
    hipLaunchKernelGGL(erp_resample_rows_kernel<2>, grid_rows, dim3(kBlock), lds, st, in, mid, first_x, wx, tx, period, rows,
                       w, w2, S, vec_rows);
  else
    hipLaunchKernelGGL(erp_resample_rows_kernel<1>, grid_rows, dim3(kBlock), lds, st, in, mid, first_x, wx, tx, period, rows,
                       w, w2, S, vec_rows);
  PCONV_LAUNCH_CHECK("erp_resample_f32 (rows)");
  int vec_cols = 0;
  if (w2 % 4 == 0 && ((ao | am) & 15) == 0) vec_cols = (w2 / 2) % 4 == 0 ? 2 : 1;
  hipLaunchKernelGGL(erp_resample_cols_kernel, dim3(h2, tiles, n * c), dim3(kBlock), 0, st, mid, out, first_y, wy, ty, h,
                     h2, w2, clamp, vec_cols);
  PCONV_LAUNCH_CHECK("erp_resample_f32 (columns)");
  return PCONV_OK;
}
