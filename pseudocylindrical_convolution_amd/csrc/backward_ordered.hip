// Ordered (atomic-free) forms of the four backward kernels that sum with float atomics in their default
// form (backward.hip: slice / uslice; pointwise.hip: projects, quantiser).  Every destination element has ONE
// fp32 accumulator that starts at +0 and receives its terms -- each one fp32 product rounded on its own, then one
// fp32 add -- in the order include/pconv_hip.h defines ("the order"): the order in which the oracle's sequential
// scatter reaches the element.  The result therefore does not depend on the grid, the workgroup or the batch, and
// slice / uslice / projects equal the oracle bit for bit.
//   * slice / uslice: a workgroup stages the source gradient rows of one (frame, channel, group of tile rows) in
//     LDS; a lane owns one (row, destination column) and walks the column's reverse list (pconv_host_tap_reverse)
//     out of LDS.  A list is never split over lanes.
//   * projects: a lane owns one ERP pixel, reads its list (pconv_host_project_reverse) once and walks up to four
//     planes with it; pixels no sample reaches get 0 -- there is no memset.
//   * quantiser: g_in is elementwise as in the default form; bins[c][q] is a two-stage fp64 reduction of fixed
//     shape (one workgroup per plane, lane l takes elements l, l + 256, ...; a fixed tree over the lanes; then
//     the planes in ascending order).
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxRows = 16;
constexpr size_t kLdsTarget = 32 * 1024;  // rows are added to a workgroup up to this much LDS: 5 workgroups per CU
constexpr int kPlanes = 4;                // planes one lane of the projects kernel carries
constexpr int kMaxLevels = 32;            // quantiser levels: 256 lanes x levels fp64 accumulators in LDS (64 KB)

// rows of one tile a workgroup takes: the largest divisor of the tile's rows that fits kLdsTarget (one row always
// fits: the entry points refuse rows above 64 KB).  A function of the shape alone, and the sums do not depend on it.
int rows_per_block(int tile_rows, int width) {
  int rb = 1;
  for (int r = 2; r <= kMaxRows && r <= tile_rows; r++)
    if (tile_rows % r == 0 && (size_t)r * width * 4 <= kLdsTarget) rb = r;
  return rb;
}

// the ordered sum of one destination column over the staged row: acc from +0, product rounded, then add
__device__ __forceinline__ float walk(const float *row, const int32_t *__restrict__ rev_src,
                                      const float *__restrict__ rev_coef, int k0, int k1) {
  float acc = 0.f;
  for (int k = k0; k < k1; k++) acc = __fadd_rn(acc, __fmul_rn(row[rev_src[k]], rev_coef[k]));
  return acc;
}

// grad of the tile stack (n*npart, c, h/npart + 2 pad, w + 2 pad) -> grad of the ERP image (n, c, height, width)
__global__ __launch_bounds__(kBlock) void slice_backward_ordered_kernel(
    const float *__restrict__ gout, float *__restrict__ gin, const int32_t *__restrict__ widths,
    const int32_t *__restrict__ rev_start, const int32_t *__restrict__ rev_src, const float *__restrict__ rev_coef,
    int c, int height, int width, int npart, int pad, int rb, long long ngroups) {
  extern __shared__ float lds[];
  const int th_tile = height / npart;
  const int oh = th_tile + 2 * pad, ow = width + 2 * pad;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long long row0 = g * rb;  // first ERP row of the group, over (frame, channel, row)
    const int ph = (int)(row0 % height);
    const long long nc = row0 / height;
    const int pt = ph / th_tile;
    const int th = ph - pt * th_tile;
    const long long pn = nc / c;
    const int pc = (int)(nc % c);
    const int valid = min(widths[pt], width);
    const float *src = gout + (((size_t)(pn * npart + pt) * c + pc) * oh + th + pad) * ow + pad;
    __syncthreads();
    for (int i = threadIdx.x; i < rb * valid; i += kBlock) {
      const int r = i / valid, tw = i - r * valid;
      lds[r * width + tw] = src[(size_t)r * ow + tw];
    }
    __syncthreads();
    float *dst = gin + (size_t)row0 * width;
    const int32_t *start = rev_start + (size_t)pt * width;
    for (int i = threadIdx.x; i < rb * width; i += kBlock) {
      const int r = i / width, j = i - r * width;
      dst[i] = walk(lds + r * width, rev_src, rev_coef, start[j], start[j + 1]);
    }
  }
}

// grad of the ERP image (n, c, h*npart, w) -> grad of the tile stack (n*npart, c, h + 2 pad, w + 2 pad); the
// kernel writes every element of the stack: the ring and the dead columns as zero
__global__ __launch_bounds__(kBlock) void uslice_backward_ordered_kernel(
    const float *__restrict__ gout, float *__restrict__ gin, const int32_t *__restrict__ widths,
    const int32_t *__restrict__ rev_start, const int32_t *__restrict__ rev_src, const float *__restrict__ rev_coef,
    int c, int h, int width, int npart, int pad, int rb, long long ngroups) {
  extern __shared__ float lds[];
  const int h_out = h * npart;
  const int ih = h + 2 * pad, iw = width + 2 * pad;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long long row0 = g * rb;  // first ERP row of the group, over (frame, channel, row)
    const int th = (int)(row0 % h_out);
    const long long nc = row0 / h_out;
    const int pb = th / h;
    const int ph = th - pb * h;
    const long long pn = nc / c;
    const int pc = (int)(nc % c);
    const int valid = min(widths[pb], width);
    const float *src = gout + (size_t)row0 * width;
    __syncthreads();
    for (int i = threadIdx.x; i < rb * width; i += kBlock) lds[i] = src[i];
    __syncthreads();
    float *plane = gin + ((size_t)(pn * npart + pb) * c + pc) * ih * iw;
    float *dst = plane + (size_t)(ph + pad) * iw;
    const int32_t *start = rev_start + (size_t)pb * width;
    // a polar tile has few columns and long lists: the (row, column) pairs of all rows share the lanes
    for (int i = threadIdx.x; i < rb * valid; i += kBlock) {
      const int r = i / valid, col = i - r * valid;
      dst[(size_t)r * iw + pad + col] = walk(lds + r * width, rev_src, rev_coef, start[col], start[col + 1]);
    }
    const int dead = iw - valid;  // columns of a row outside the valid interior
    for (int i = threadIdx.x; i < rb * dead; i += kBlock) {
      const int r = i / dead, d = i - r * dead;
      dst[(size_t)r * iw + (d < pad ? d : d + valid)] = 0.f;
    }
    if (ph == 0)  // the first group of a tile also clears the ring rows above it, the last those below
      for (int i = threadIdx.x; i < pad * iw; i += kBlock) plane[i] = 0.f;
    if (ph + rb == h)
      for (int i = threadIdx.x; i < pad * iw; i += kBlock) plane[(size_t)(h + pad) * iw + i] = 0.f;
  }
}

// gout (nview, planes, inner) -> gin, count (planes, hs*ws); blockIdx.y picks the group of kPlanes planes
__global__ __launch_bounds__(kBlock) void project_backward_ordered_kernel(
    const float *__restrict__ gout, const int32_t *__restrict__ rev_start, const int32_t *__restrict__ rev_sample,
    const float *__restrict__ rev_wgt, float *__restrict__ gin, float *__restrict__ count, int inner, long long hw,
    int planes) {
  const int p0 = blockIdx.y * kPlanes;
  const int np = min(kPlanes, planes - p0);
  for (long long pix = (long long)blockIdx.x * kBlock + threadIdx.x; pix < hw; pix += (long long)gridDim.x * kBlock) {
    float acc[kPlanes] = {0.f, 0.f, 0.f, 0.f};
    float cnt = 0.f;
    const int k1 = rev_start[pix + 1];
    for (int k = rev_start[pix]; k < k1; k++) {
      const int s = rev_sample[k];
      const float w = rev_wgt[k];
      const int tb = s / inner;
      const float *g = gout + ((size_t)tb * planes + p0) * inner + (s - tb * inner);
      cnt = __fadd_rn(cnt, w);
#pragma unroll
      for (int p = 0; p < kPlanes; p++)
        if (p < np) acc[p] = __fadd_rn(acc[p], __fmul_rn(w, g[(size_t)p * inner]));
    }
#pragma unroll
    for (int p = 0; p < kPlanes; p++)
      if (p < np) {
        gin[(size_t)(p0 + p) * hw + pix] = acc[p];
        count[(size_t)(p0 + p) * hw + pix] = cnt;
      }
  }
}

// stage one of the quantiser's level sums, fused with the elementwise g_in (the expressions of
// quant_backward_kernel, pointwise.hip).  One workgroup per (tile-image, channel) plane: lane l adds the
// differences val - x (one fp32 rounding each) of the live elements l, l + 256, ... of the plane, ascending, to
// one fp64 accumulator per level; then, per level, the tree a[l] += a[l + s] for s = 128, 64, ..., 1 leaves the
// plane's partial in a[0].  partials: (planes, levels) fp64.
__global__ __launch_bounds__(kBlock) void quant_backward_ordered_kernel(
    const float *__restrict__ x, const float *__restrict__ val, const float *__restrict__ idx,
    const float *__restrict__ g_val, const float *__restrict__ g_idx, const float *__restrict__ tab,
    float *__restrict__ g_in, double *__restrict__ partials, const int32_t *__restrict__ widths, float alpha, int c,
    int hw, int w, int levels, int npart, long long nplanes) {
  extern __shared__ double sums[];  // [level][lane]
  for (long long plane = blockIdx.x; plane < nplanes; plane += gridDim.x) {
    const int pc = (int)(plane % c);
    const int pg = (int)((plane / c) % npart);
    const int valid = widths[pg];
    const float *lv = tab + pc * levels;
    __syncthreads();
    for (int q = 0; q < levels; q++) sums[q * kBlock + threadIdx.x] = 0.0;
    for (int e = threadIdx.x; e < hw; e += kBlock) {
      const size_t i = (size_t)plane * hw + e;
      float g = 0.f;
      if (e % w < valid) {
        const float xv = x[i], tv = val[i];
        const int q = (int)idx[i];
        if ((unsigned)q < (unsigned)levels) {  // (a level outside the table would leave the LDS block)
          double *a = sums + q * kBlock + threadIdx.x;
          *a = __dadd_rn(*a, (double)__fsub_rn(tv, xv));
        }
        g = g_val[i];
        if (g_idx) {
          float beta;
          if (tv < xv) {
            beta = q < levels - 1 ? lv[q + 1] : 10000.f;
          } else if (tv > xv) {
            beta = q > 0 ? lv[q] : 10000.f;
          } else if (q == 0) {
            beta = lv[1];
          } else if (q < levels - 1) {
            beta = (lv[q] + lv[q + 1]) / 2.0;
          } else {
            beta = lv[q];
          }
          if (beta < 0.001) beta = 0.001;
          g = g + alpha * g_idx[i] / beta;
        }
      }
      g_in[i] = g;
    }
    for (int s = kBlock / 2; s > 0; s >>= 1) {
      __syncthreads();
      for (int i = threadIdx.x; i < levels * s; i += kBlock) {
        const int q = i / s, l = i - q * s;
        sums[q * kBlock + l] = __dadd_rn(sums[q * kBlock + l], sums[q * kBlock + l + s]);
      }
    }
    __syncthreads();
    if (threadIdx.x < levels) partials[(size_t)plane * levels + threadIdx.x] = sums[threadIdx.x * kBlock];
  }
}

// stage two: bins[c][q] = the partials of the channel's planes, tile-image ascending, added in fp64 from +0 and
// rounded once to fp32
__global__ __launch_bounds__(kBlock) void quant_bins_ordered_kernel(const double *__restrict__ partials,
                                                                    float *__restrict__ bins, int tn, int c, int levels) {
  const int i = blockIdx.x * kBlock + threadIdx.x;  // channel * levels + level
  if (i >= c * levels) return;
  const int ch = i / levels, q = i - ch * levels;
  double acc = 0.0;
  for (int t = 0; t < tn; t++) acc = __dadd_rn(acc, partials[((size_t)t * c + ch) * levels + q]);
  bins[i] = (float)acc;
}

std::atomic<unsigned long long> g_quant_lds{0};

}  // namespace

extern "C" int pconv_sphere_slice_backward_ordered(const float *gout, float *gin, const int32_t *widths,
                                                   const int32_t *rev_start, const int32_t *rev_src,
                                                   const float *rev_coef, int n, int c, int height, int width,
                                                   int npart, int pad, void *stream) {
  PCONV_REQUIRE(gout && gin && widths && rev_start && rev_src && rev_coef, "sphere_slice_backward_ordered: null pointer");
  PCONV_REQUIRE(n > 0 && c > 0 && npart > 0 && height > 0 && width > 0 && height % npart == 0 && pad >= 0,
                "sphere_slice_backward_ordered: bad shape");
  PCONV_REQUIRE((size_t)width * 4 <= 64 * 1024, "sphere_slice_backward_ordered: width %d exceeds LDS row", width);
  const int rb = rows_per_block(height / npart, width);
  const long long ngroups = (long long)n * c * height / rb;
  const unsigned grid = (unsigned)(ngroups < 256 * 16 ? ngroups : 256 * 16);
  hipLaunchKernelGGL(slice_backward_ordered_kernel, dim3(grid), dim3(kBlock), (size_t)rb * width * 4, as_stream(stream),
                     gout, gin, widths, rev_start, rev_src, rev_coef, c, height, width, npart, pad, rb, ngroups);
  PCONV_LAUNCH_CHECK("sphere_slice_backward_ordered");
  return PCONV_OK;
}

extern "C" int pconv_sphere_uslice_backward_ordered(const float *gout, float *gin, const int32_t *widths,
                                                    const int32_t *rev_start, const int32_t *rev_src,
                                                    const float *rev_coef, int n, int c, int h, int width, int npart,
                                                    int pad, void *stream) {
  PCONV_REQUIRE(gout && gin && widths && rev_start && rev_src && rev_coef, "sphere_uslice_backward_ordered: null pointer");
  PCONV_REQUIRE(n > 0 && c > 0 && npart > 0 && h > 0 && width > 0 && pad >= 0, "sphere_uslice_backward_ordered: bad shape");
  PCONV_REQUIRE((size_t)width * 4 <= 64 * 1024, "sphere_uslice_backward_ordered: width %d exceeds LDS row", width);
  const int rb = rows_per_block(h, width);
  const long long ngroups = (long long)n * c * h * npart / rb;
  const unsigned grid = (unsigned)(ngroups < 256 * 16 ? ngroups : 256 * 16);
  hipLaunchKernelGGL(uslice_backward_ordered_kernel, dim3(grid), dim3(kBlock), (size_t)rb * width * 4, as_stream(stream),
                     gout, gin, widths, rev_start, rev_src, rev_coef, c, h, width, npart, pad, rb, ngroups);
  PCONV_LAUNCH_CHECK("sphere_uslice_backward_ordered");
  return PCONV_OK;
}

extern "C" int pconv_project_backward_ordered(const float *gout, const int32_t *rev_start, const int32_t *rev_sample,
                                              const float *rev_wgt, float *gin, float *count, int n, int c, int height,
                                              int width, int nview, int h_out, int w_out, void *stream) {
  PCONV_REQUIRE(gout && rev_start && rev_sample && rev_wgt && gin && count, "project_backward_ordered: null pointer");
  PCONV_REQUIRE(n > 0 && c > 0 && nview > 0 && height > 0 && width > 0 && h_out > 0 && w_out > 0,
                "project_backward_ordered: bad shape");
  const long long planes = (long long)n * c, hw = (long long)height * width;
  PCONV_REQUIRE((planes + kPlanes - 1) / kPlanes <= 65535 && (long long)nview * h_out * w_out * 4 <= INT32_MAX &&
                    hw < INT32_MAX,
                "project_backward_ordered: shape exceeds the launch or the int32 lists");
  hipLaunchKernelGGL(project_backward_ordered_kernel, dim3(pconv_grid(hw), (unsigned)((planes + kPlanes - 1) / kPlanes)),
                     dim3(kBlock), 0, as_stream(stream), gout, rev_start, rev_sample, rev_wgt, gin, count,
                     h_out * w_out, hw, (int)planes);
  PCONV_LAUNCH_CHECK("project_backward_ordered");
  return PCONV_OK;
}

extern "C" long long pconv_quant_backward_ordered_workspace_bytes(int tn, int c, int levels) {
  PCONV_REQUIRE(tn > 0 && c > 0 && levels > 1, "quant_backward_ordered_workspace_bytes: bad shape");
  return (long long)tn * c * levels * (long long)sizeof(double);
}

extern "C" int pconv_quant_backward_ordered(const float *x, const float *val, const float *idx, const float *g_val,
                                            const float *g_idx, const float *level_tab, float *g_in, float *g_weight,
                                            float *bins, void *workspace, const int32_t *widths, float top_alpha,
                                            int tn, int c, int h, int w, int levels, int npart, void *stream) {
  PCONV_REQUIRE(x && val && idx && g_val && level_tab && g_in && g_weight && bins && workspace && widths,
                "quant_backward_ordered: null pointer");
  PCONV_REQUIRE(tn > 0 && c > 0 && h > 0 && w > 0 && levels > 1 && npart > 0, "quant_backward_ordered: bad shape");
  PCONV_REQUIRE(levels <= kMaxLevels, "quant_backward_ordered: %d levels exceed the %d the LDS accumulators hold", levels,
                kMaxLevels);
  PCONV_REQUIRE((long long)h * w < INT32_MAX && (long long)c * levels < INT32_MAX, "quant_backward_ordered: plane too large");
  const size_t lds = (size_t)levels * kBlock * sizeof(double);
  if (lds > 48 * 1024) {
    int rc = pconv_raise_lds(quant_backward_ordered_kernel, lds, g_quant_lds, "quant_backward_ordered");
    if (rc < 0) return rc;
  }
  const long long nplanes = (long long)tn * c;
  const unsigned grid = (unsigned)(nplanes < 256 * 16 ? nplanes : 256 * 16);
  hipLaunchKernelGGL(quant_backward_ordered_kernel, dim3(grid), dim3(kBlock), lds, as_stream(stream), x, val, idx, g_val,
                     g_idx, level_tab, g_in, static_cast<double *>(workspace), widths, top_alpha, c, h * w, w, levels,
                     npart, nplanes);
  hipLaunchKernelGGL(quant_bins_ordered_kernel, dim3((c * levels + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     as_stream(stream), static_cast<const double *>(workspace), bins, tn, c, levels);
  PCONV_LAUNCH_CHECK("quant_backward_ordered");
  return pconv_launch_quant_weight_grad(bins, level_tab, g_weight, c, levels, as_stream(stream));
}
