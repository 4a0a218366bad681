// Ordered backward of the sphere-aware Lanczos-3 resize (the definition is in include/pconv_hip.h,
// pconv_erp_resample_backward_f32): gx = Ax^T Ay^T g, the adjoint of the two passes of erp_resample.hip, taken in the
// opposite order.  Both passes are gathers over the transposed tap tables of pconv_host_lanczos_reverse (below: a CSR
// list per source index, entry e = i * T + t, so that the weight of an entry is weights[e] of the forward's own table):
// a list is walked front to back by one lane, the first product starts the chain, every further term is one __fmul_rn
// and one __fadd_rn.  No atomics, no allocation, no memset.
//   columns pass: g (n*C, h2, w2) -> gmid (n*C, h, w2), the mirror of erp_resample_cols_kernel.  The list of a gmid row
//                 is wave-uniform (blockIdx.x is the row); a lane owns 4 adjacent columns and walks it: 16-byte loads
//                 where w2 % 4 == 0, for entries that crossed a pole only where floor(w2/2) % 4 == 0 as well, else
//                 4-byte loads.  An entry that crossed a pole reads g at column (c - floor(w2/2)) mod w2.
//   rows pass:    gmid (n*C*h rows of w2) -> gx (rows of w), the mirror of erp_resample_rows_kernel.  A workgroup takes
//                 R consecutive rows x one tile of kTile source columns: the span of gmid columns the tile's lists reach,
//                 wrapped modulo w2, is staged in LDS, then lane l walks the lists of columns l, l + 256, l + 512,
//                 l + 768 of the tile, each entry decoded once for the R rows.
// Every index read from a list is reduced to one inside the table (an entry outside 0 .. n_out*T - 1 is skipped, a start
// outside it clamped) and every staged column to one inside the span, so no list content makes a kernel read outside
// its buffers; each lane stores only its own elements.
#include <vector>
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 4 * kBlock;        // destination columns of one workgroup, both passes
constexpr int kMaxLdsBytes = 64 * 1024;  // rows pass: R rows of the staged span

__host__ __device__ inline long long ceil_div(long long a, long long b) {  // b > 0
  const long long q = a / b;
  return (a % b != 0 && a > 0) ? q + 1 : q;
}

// Floats of LDS one staged row needs for a tile of kTile source columns.  Output i reaches the (unwrapped) source
// columns first(i) .. first(i) + T - 1, first(i) = floor(((2i + 1) n_in - n_out - 3D) / (2 n_out)) + 1 non-decreasing in
// i, so the outputs that reach c0 .. c0 + kTile - 1 are those with c0 - T + 1 <= first(i) <= c0 + kTile - 1: at most
// floor((kTile + T - 1) n_out / n_in) + 2 of them, plus 3 for the base rounded down to a quad, rounded up to a quad;
// never more than the whole row.
inline int span_floats(int n_in, int n_out, int T) {
  long long s = ((long long)(kTile + T - 1) * n_out) / n_in + 2 + 3;
  if (s > n_out) s = n_out;
  return (int)((s + 3) & ~3LL);
}

// vec: 0 = 4-byte accesses; 1 = 16-byte loads for entries that did not cross a pole and 16-byte stores; 2 = for all
__global__ __launch_bounds__(kBlock) void erp_resample_cols_backward_kernel(
    const float *__restrict__ g, float *__restrict__ gmid, const float *__restrict__ wgt, const int32_t *__restrict__ start,
    const int32_t *__restrict__ entry, const uint8_t *__restrict__ cross, int T, int h, int h2, int w2, int vec) {
  const int r = blockIdx.x, p = blockIdx.z;
  const int x0 = blockIdx.y * kTile + 4 * threadIdx.x;
  if (x0 >= w2) return;
  const int nx = min(4, w2 - x0);  // 4 wherever vec != 0
  const int half = w2 / 2;
  const int total = h2 * T;  // h2 <= 2^20, T <= 48
  const int lo = min(max(start[r], 0), total), hi = min(max(start[r + 1], 0), total);
  const float *plane = g + (long long)p * h2 * w2;
  int xf[4];  // (c - half) mod w2: the column of g whose half-turned read is column c of gmid
#pragma unroll
  for (int k = 0; k < 4; k++) {
    xf[k] = min(x0 + k, w2 - 1) - half;
    if (xf[k] < 0) xf[k] += w2;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  bool started = false;
  for (int at = lo; at < hi; at++) {
    const int e = entry[at];
    if ((unsigned)e >= (unsigned)total) continue;
    const bool flip = cross[at] != 0;
    const float *src = plane + (long long)(e / T) * w2;
    float v[4];
    if (vec == 2 || (vec == 1 && !flip)) {
      const float4 q = *reinterpret_cast<const float4 *>(src + (flip ? xf[0] : x0));
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = src[flip ? xf[k] : min(x0 + k, w2 - 1)];
    }
    const float wt = wgt[e];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const float m = __fmul_rn(wt, v[k]);
      acc[k] = started ? __fadd_rn(acc[k], m) : m;
    }
    started = true;
  }
  float *dst = gmid + ((long long)p * h + r) * w2 + x0;
  if (vec) {
    *reinterpret_cast<float4 *>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < nx) dst[k] = acc[k];
  }
}

// magic: floor(2^32 / T) + 1, so that __umulhi(e, magic) == e / T for every e < 2^26 (T < 64)
template <int R>
__global__ __launch_bounds__(kBlock) void erp_resample_rows_backward_kernel(
    const float *__restrict__ gmid, float *__restrict__ gx, const float *__restrict__ wgt, const int32_t *__restrict__ start,
    const int32_t *__restrict__ entry, int T, unsigned magic, long long rows, int w, int w2, int S, int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const long long row0 = (long long)blockIdx.x * R;
  const int c0 = blockIdx.y * kTile;
  const int c1 = min(c0 + kTile, w);
  const int total = w2 * T;
  // the outputs whose taps reach the tile, unwrapped: c0 - T + 1 <= first(i) <= c1 - 1 (span_floats above)
  const long long D = 2LL * max(w, w2), fix = 3 * D + w2 - w;
  const long long ia = ceil_div(2LL * w2 * (c0 - T) + fix, 2LL * w);
  const long long ib = ceil_div(2LL * w2 * (c1 - 1) + fix, 2LL * w) - 1;
  const int wrapped = wrap_col((int)(ia % w2), w2);
  int base = vec ? wrapped & ~3 : wrapped;
  long long count = ib - ia + 1 + (wrapped - base);
  if (count >= w2) base = 0, count = w2;  // every column of the row: staged once, in place
  const int span = (int)min(count, (long long)S);
#pragma unroll
  for (int r = 0; r < R; r++) {
    if (row0 + r >= rows) break;
    const float *src = gmid + (row0 + r) * w2;
    float *dst = lds + r * S;
    if (vec) {  // w2 % 4 == 0, base % 4 == 0, rows 16-byte aligned: a quad never straddles the seam
      for (int q = threadIdx.x; 4 * q < span; q += kBlock) {
        int c = base + 4 * q;
        if (c >= w2) c -= w2;
        *reinterpret_cast<float4 *>(dst + 4 * q) = *reinterpret_cast<const float4 *>(src + c);
      }
    } else {
      for (int s = threadIdx.x; s < span; s += kBlock) {
        int c = base + s;
        if (c >= w2) c -= w2;
        dst[s] = src[c];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int c = c0 + j * kBlock + threadIdx.x;
    if (c >= c1) break;
    const int lo = min(max(start[c], 0), total), hi = min(max(start[c + 1], 0), total);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.f;
    bool started = false;
    for (int at = lo; at < hi; at++) {
      const int e = entry[at];
      if ((unsigned)e >= (unsigned)total) continue;
      int s = (int)__umulhi((unsigned)e, magic) - base;  // column e / T of gmid, relative to the staged span
      if (s < 0) s += w2;
      if (s >= span) continue;
      const float wt = wgt[e];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const float m = __fmul_rn(wt, lds[r * S + s]);
        acc[r] = started ? __fadd_rn(acc[r], m) : m;
      }
      started = true;
    }
#pragma unroll
    for (int r = 0; r < R; r++)
      if (row0 + r < rows) gx[(row0 + r) * w + c] = acc[r];
  }
}

int shape_ok(const char *what, int n, int c, int h, int w, int h2, int w2, int *tx, int *ty) {
  if (planes_ok(what, n, c) != PCONV_OK) return PCONV_EINVAL;
  if (pconv_host_lanczos_taps(w, w2, nullptr, nullptr, tx) != PCONV_OK ||
      pconv_host_lanczos_taps(h, h2, nullptr, nullptr, ty) != PCONV_OK)
    return PCONV_EINVAL;  // a side outside 2 .. 2^20, a shrink beyond 8:1: the message is the tap function's
  return PCONV_OK;
}

}  // namespace

extern "C" long long pconv_host_lanczos_reverse_size(int n_in, int n_out) {
  int T = 0;
  if (pconv_host_lanczos_taps(n_in, n_out, nullptr, nullptr, &T) != PCONV_OK) return PCONV_EINVAL;
  return (long long)n_out * T;  // at most 2^20 * 48
}

// Transpose of the tap table of one axis as a CSR list per source index (the ordered backward of the resize): the
// forward walk -- output i ascending, then tap t = 0 .. T - 1, the padded taps of weight +0.0 included -- sorted by the
// source index the tap reads with a stable counting sort.  pole == 0 (the horizontal pass): tap (i, t) reads
// (first[i] + t) mod n_in.  pole != 0 (the vertical pass): it reads r = first[i] + t through the pole rule (r < 0 ->
// -1 - r; r >= n_in -> 2 n_in - 1 - r), then clamped to [0, n_in - 1], and crossed[k] says whether entry k crossed a
// pole (judged before the clamp).  rev_start: n_in + 1 ints; rev_entry: pconv_host_lanczos_reverse_size entries e = i * T
// + t, ascending within each list; crossed: as many bytes, required for pole != 0 and ignored otherwise.  Returns the
// number of entries; nothing is written unless every argument passes.
extern "C" int pconv_host_lanczos_reverse(int n_in, int n_out, int pole, int32_t *rev_start, int32_t *rev_entry,
                                          uint8_t *crossed) {
  PCONV_REQUIRE(rev_start && rev_entry && (crossed || !pole), "host_lanczos_reverse: null pointer");
  const long long total = pconv_host_lanczos_reverse_size(n_in, n_out);
  if (total < 0) return PCONV_EINVAL;
  const int T = (int)(total / n_out);
  std::vector<int32_t> first(n_out);
  std::vector<float> weights((size_t)total);
  int taps = 0;
  if (pconv_host_lanczos_taps(n_in, n_out, first.data(), weights.data(), &taps) != PCONV_OK) return PCONV_EINVAL;
  std::vector<int32_t> fill((size_t)n_in + 1, 0);
  for (int pass = 0; pass < 2; pass++) {
    for (int i = 0; i < n_out; i++)
      for (int t = 0; t < T; t++) {
        bool flip = false;  // |first[i] + t| < 2^24: a side is at most 2^20 and a shrink at most 8:1
        const int r = pole ? pole_row(first[i] + t, n_in, &flip) : wrap_col(first[i] + t, n_in);
        if (pass == 0) {
          fill[(size_t)r + 1]++;
        } else {
          const int32_t k = fill[(size_t)r]++;
          rev_entry[k] = i * T + t;
          if (pole) crossed[k] = flip ? 1 : 0;
        }
      }
    if (pass == 0) {
      for (int k = 0; k < n_in; k++) fill[k + 1] += fill[k];
      for (int k = 0; k <= n_in; k++) rev_start[k] = fill[k];
    }
  }
  return (int)total;
}

extern "C" long long pconv_erp_resample_backward_workspace_bytes(int n, int c, int h, int w, int h2, int w2) {
  if (n <= 0 || c <= 0 || (long long)n * c > 65535 || h < 2 || w < 2 || h2 < 2 || w2 < 2 || h > (1 << 20) ||
      w > (1 << 20) || h2 > (1 << 20) || w2 > (1 << 20)) {
    pconv_set_error("erp_resample_backward_workspace_bytes: bad shape (%d, %d, %d, %d) -> %dx%d", n, c, h, w, w2, h2);
    return PCONV_EINVAL;
  }
  return 4LL * n * c * h * w2;  // the vertical adjoint's picture (gmid), rounded to float32
}

extern "C" int pconv_erp_resample_backward_f32(const float *gout, float *gin, void *workspace, const float *wx, int tx,
                                               const int32_t *rev_start_x, const int32_t *rev_entry_x, const float *wy,
                                               int ty, const int32_t *rev_start_y, const int32_t *rev_entry_y,
                                               const uint8_t *rev_crossed_y, int n, int c, int h, int w, int h2, int w2,
                                               void *stream) {
  PCONV_REQUIRE(gout && gin && workspace && wx && wy, "erp_resample_backward_f32: null pointer");
  PCONV_REQUIRE(rev_start_x && rev_entry_x && rev_start_y && rev_entry_y && rev_crossed_y,
                "erp_resample_backward_f32: null list pointer");
  int want_tx = 0, want_ty = 0;
  if (shape_ok("erp_resample_backward_f32", n, c, h, w, h2, w2, &want_tx, &want_ty) != PCONV_OK) return PCONV_EINVAL;
  PCONV_REQUIRE(tx == want_tx && ty == want_ty,
                "erp_resample_backward_f32: tap counts %d, %d are not those of the tables (%d, %d)", tx, ty, want_tx, want_ty);
  PCONV_REQUIRE(tx >= 2 && tx < 64, "erp_resample_backward_f32: %d taps per output are outside 2 .. 63", tx);
  PCONV_REQUIRE(gin != gout, "erp_resample_backward_f32: gin and gout must be distinct");
  const uintptr_t ag = reinterpret_cast<uintptr_t>(gout), ai = reinterpret_cast<uintptr_t>(gin),
                  am = reinterpret_cast<uintptr_t>(workspace);
  PCONV_REQUIRE(((ag | ai | am | reinterpret_cast<uintptr_t>(wx) | reinterpret_cast<uintptr_t>(wy) |
                  reinterpret_cast<uintptr_t>(rev_start_x) | reinterpret_cast<uintptr_t>(rev_entry_x) |
                  reinterpret_cast<uintptr_t>(rev_start_y) | reinterpret_cast<uintptr_t>(rev_entry_y)) & 3) == 0,
                "erp_resample_backward_f32: the tensors, tables and lists must be 4-byte aligned");
  const long long rows = (long long)n * c * h;
  const int S = span_floats(w, w2, tx);
  PCONV_REQUIRE((long long)S * 4 <= kMaxLdsBytes,
                "erp_resample_backward_f32: a tile's span of %d gradient columns (%d -> %d) exceeds LDS", S, w, w2);
  const int R = 4 * S * 4 <= kMaxLdsBytes ? 4 : (2 * S * 4 <= kMaxLdsBytes ? 2 : 1);
  const long long groups = (rows + R - 1) / R;
  PCONV_REQUIRE(groups <= 0x7fffffffLL, "erp_resample_backward_f32: %lld rows exceed the grid", rows);
  float *gmid = static_cast<float *>(workspace);
  hipStream_t st = as_stream(stream);
  int vec_cols = 0;
  if (w2 % 4 == 0 && ((ag | am) & 15) == 0) vec_cols = (w2 / 2) % 4 == 0 ? 2 : 1;
  hipLaunchKernelGGL(erp_resample_cols_backward_kernel, dim3(h, (w2 + kTile - 1) / kTile, n * c), dim3(kBlock), 0, st, gout,
                     gmid, wy, rev_start_y, rev_entry_y, rev_crossed_y, ty, h, h2, w2, vec_cols);
  PCONV_LAUNCH_CHECK("erp_resample_backward_f32 (columns)");
  const int vec_rows = (w2 % 4 == 0 && (am & 15) == 0) ? 1 : 0;
  const unsigned magic = (unsigned)((1ULL << 32) / (unsigned)tx) + 1u;
  const dim3 grid_rows((unsigned)groups, (w + kTile - 1) / kTile);
  const size_t lds = (size_t)R * S * 4;
  if (R == 4)
    hipLaunchKernelGGL(erp_resample_rows_backward_kernel<4>, grid_rows, dim3(kBlock), lds, st, gmid, gin, wx, rev_start_x,
                       rev_entry_x, tx, magic, rows, w, w2, S, vec_rows);
  else if (R == 2)
    hipLaunchKernelGGL(erp_resample_rows_backward_kernel<2>, grid_rows, dim3(kBlock), lds, st, gmid, gin, wx, rev_start_x,
                       rev_entry_x, tx, magic, rows, w, w2, S, vec_rows);
  else
    hipLaunchKernelGGL(erp_resample_rows_backward_kernel<1>, grid_rows, dim3(kBlock), lds, st, gmid, gin, wx, rev_start_x,
                       rev_entry_x, tx, magic, rows, w, w2, S, vec_rows);
  PCONV_LAUNCH_CHECK("erp_resample_backward_f32 (rows)");
  return PCONV_OK;
}
