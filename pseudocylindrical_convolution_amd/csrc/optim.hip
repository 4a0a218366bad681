// The optimiser step of training on this project's arithmetic (optim.Adam, train.py --optim native): the global
// gradient norm, the clip coefficient and the Adam update of a whole parameter list in three launches, every
// operation and the order of the one reduction as include/pconv_hip.h defines them ("THE ORDER" of the optimiser
// step).  No atomics, no host synchronisation, nothing allocated: a device table of one record per tensor, a segment
// table (4096 elements of one tensor per workgroup) and a workspace that keeps total, norm and coef on the device.
//   * sqnorm: a workgroup owns one segment; lane l of 256 squares quads l, l + 256, ... of the step gradient in
//     fp64 and a fixed tree leaves the segment's partial.  A closing workgroup adds the partials in the same shape
//     and writes total, norm = sqrt(total) and coef.
//   * adam: element-wise, fp32, nothing contracted (-ffp-contract=off, and the operations are spelled __f*_rn); reads
//     p, grad, acc, m, v once and writes p, m, v and the zeroed acc once: 44 bytes per element with the norm pass.
// Both kernels move a quad as one 16-byte access where every pointer of the tensor is 16-byte aligned, and as 4-byte
// accesses in the same order where one is not.
#include "common.h"
#include <math.h>

namespace {

constexpr int kBlock = 256;
constexpr int kSegment = 4096;             // elements per workgroup: four quads per lane
constexpr size_t kHeader = 32;             // workspace: double total, double norm, float coef, 12 bytes unused
static_assert(sizeof(pconv_optim_tensor) == 72, "pconv_optim_tensor is nine 8-byte words");

struct Workspace {
  double total, norm;
  float coef;
  float unused[3];
};
static_assert(sizeof(Workspace) == kHeader, "workspace header");

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// for s = 128 ... 1: a[l] += a[l + s] for l < s; every lane returns a[0]
__device__ __forceinline__ double tree(double *a, double mine) {
  const int l = threadIdx.x;
  a[l] = mine;
  __syncthreads();
  for (int s = kBlock / 2; s >= 1; s >>= 1) {
    if (l < s) a[l] = a[l] + a[l + s];
    __syncthreads();
  }
  return a[0];
}

// elements [e0, e0 + cnt) of a tensor's segment: one 16-byte load for a full quad of an aligned tensor
__device__ __forceinline__ void load_quad(const float *__restrict__ src, int e0, int cnt, bool vec, float out[4]) {
  if (vec && cnt == 4) {
    const float4 t = *reinterpret_cast<const float4 *>(src + e0);
    out[0] = t.x, out[1] = t.y, out[2] = t.z, out[3] = t.w;
  } else {
    for (int j = 0; j < 4; j++) out[j] = j < cnt ? src[e0 + j] : 0.f;
  }
}

__device__ __forceinline__ void store_quad(float *__restrict__ dst, int e0, int cnt, bool vec, const float in[4]) {
  if (vec && cnt == 4) {
    *reinterpret_cast<float4 *>(dst + e0) = make_float4(in[0], in[1], in[2], in[3]);
  } else {
    for (int j = 0; j < cnt; j++) dst[e0 + j] = in[j];
  }
}

struct Segment {
  pconv_optim_tensor t;
  long long off;
  int len;
};

__device__ __forceinline__ Segment segment_of(const pconv_optim_tensor *__restrict__ rec,
                                              const int32_t *__restrict__ seg, int s) {
  Segment S;
  S.t = rec[seg[2 * s]];
  S.off = (long long)seg[2 * s + 1] * kSegment;
  const long long left = S.t.n - S.off;
  S.len = (int)(left < kSegment ? left : kSegment);
  return S;
}

__global__ __launch_bounds__(kBlock) void optim_sqnorm_kernel(const pconv_optim_tensor *__restrict__ rec,
                                                              const int32_t *__restrict__ seg,
                                                              double *__restrict__ partials) {
  __shared__ double a[kBlock];
  const Segment S = segment_of(rec, seg, blockIdx.x);
  const float *grad = S.t.grad + S.off;
  const float *acc = S.t.acc ? S.t.acc + S.off : nullptr;
  const bool vec = aligned16(grad) && aligned16(acc);
  double sum = 0.0;
  for (int e0 = 4 * threadIdx.x; e0 < S.len; e0 += 4 * kBlock) {
    const int cnt = S.len - e0 < 4 ? S.len - e0 : 4;
    float g[4], ac[4];
    load_quad(grad, e0, cnt, vec, g);
    if (acc) {
      load_quad(acc, e0, cnt, vec, ac);
      for (int j = 0; j < 4; j++) g[j] = __fadd_rn(ac[j], g[j]);
    }
    for (int j = 0; j < cnt; j++) sum = sum + (double)g[j] * (double)g[j];
  }
  const double total = tree(a, sum);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void optim_close_kernel(const double *__restrict__ partials, int nsegment,
                                                             float clip, Workspace *__restrict__ ws) {
  __shared__ double a[kBlock];
  double sum = 0.0;
  for (int i = threadIdx.x; i < nsegment; i += kBlock) sum = sum + partials[i];
  const double total = tree(a, sum);
  if (threadIdx.x == 0) {
    const double norm = sqrt(total);
    double coef = 1.0;
    if (clip > 0.f) {
      const double c = (double)clip / (norm + 1e-6);
      coef = c < 1.0 ? c : (c != c ? c : 1.0);  // min(1, c) that keeps a NaN
    }
    ws->total = total;
    ws->norm = norm;
    ws->coef = (float)coef;
  }
}

__global__ __launch_bounds__(kBlock) void optim_adam_kernel(const pconv_optim_tensor *__restrict__ rec,
                                                            const int32_t *__restrict__ seg,
                                                            const Workspace *__restrict__ ws) {
  const Segment S = segment_of(rec, seg, blockIdx.x);
  const float coef = ws->coef;
  float *p = S.t.p + S.off, *m = S.t.m + S.off, *v = S.t.v + S.off;
  const float *grad = S.t.grad + S.off;
  float *acc = S.t.acc ? S.t.acc + S.off : nullptr;
  const bool vec = aligned16(p) && aligned16(m) && aligned16(v) && aligned16(grad) && aligned16(acc);
  const float step_size = S.t.step_size, bc2_sqrt = S.t.bc2_sqrt, eps = S.t.eps;
  const float omb1 = S.t.one_minus_beta1, beta2 = S.t.beta2, omb2 = S.t.one_minus_beta2;
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e0 = 4 * threadIdx.x; e0 < S.len; e0 += 4 * kBlock) {
    const int cnt = S.len - e0 < 4 ? S.len - e0 : 4;
    float g[4], ac[4], pv[4], mv[4], vv[4];
    load_quad(grad, e0, cnt, vec, g);
    if (acc) {
      load_quad(acc, e0, cnt, vec, ac);
      for (int j = 0; j < 4; j++) g[j] = __fadd_rn(ac[j], g[j]);
    }
    load_quad(p, e0, cnt, vec, pv);
    load_quad(m, e0, cnt, vec, mv);
    load_quad(v, e0, cnt, vec, vv);
    for (int j = 0; j < 4; j++) {
      const float gj = __fmul_rn(g[j], coef);
      mv[j] = __fadd_rn(mv[j], __fmul_rn(omb1, __fsub_rn(gj, mv[j])));
      vv[j] = __fadd_rn(__fmul_rn(beta2, vv[j]), __fmul_rn(omb2, __fmul_rn(gj, gj)));
      const float den = __fadd_rn(__fdiv_rn(sqrtf(vv[j]), bc2_sqrt), eps);
      pv[j] = __fsub_rn(pv[j], __fmul_rn(step_size, __fdiv_rn(mv[j], den)));
    }
    store_quad(p, e0, cnt, vec, pv);
    store_quad(m, e0, cnt, vec, mv);
    store_quad(v, e0, cnt, vec, vv);
    if (acc) store_quad(acc, e0, cnt, vec, zero);
  }
}

// segments of `ntensor` tensors of counts[t] elements, or -1 for a negative count or more than INT32_MAX segments
long long count_segments(const long long *counts, int ntensor) {
  long long total = 0;
  for (int t = 0; t < ntensor; t++) {
    if (counts[t] < 0) return -1;
    total += (counts[t] + kSegment - 1) / kSegment;
    if (total > INT32_MAX) return -1;
  }
  return total;
}

int check_tables(const char *what, const void *records, const int32_t *segments, const long long *counts, int ntensor,
                 int nsegment, const void *workspace) {
  PCONV_REQUIRE(records && segments && counts && workspace, "%s: null pointer", what);
  PCONV_REQUIRE(ntensor > 0 && nsegment > 0, "%s: bad counts (%d tensors, %d segments)", what, ntensor, nsegment);
  const long long expect = count_segments(counts, ntensor);
  PCONV_REQUIRE(expect >= 0, "%s: negative element count, or more than 2^31 - 1 segments", what);
  PCONV_REQUIRE(expect == nsegment, "%s: the segment table has %d entries, the element counts need %lld", what, nsegment,
                expect);
  return PCONV_OK;
}

}  // namespace

extern "C" long long pconv_host_optim_segments(const long long *counts, int ntensor, int32_t *segments) {
  PCONV_REQUIRE(counts && ntensor > 0, "host_optim_segments: null pointer or no tensor");
  const long long total = count_segments(counts, ntensor);
  PCONV_REQUIRE(total >= 0, "host_optim_segments: negative element count, or more than 2^31 - 1 segments");
  if (segments) {
    long long s = 0;
    for (int t = 0; t < ntensor; t++)
      for (long long i = 0; i * kSegment < counts[t]; i++, s++) segments[2 * s] = t, segments[2 * s + 1] = (int32_t)i;
  }
  return total;
}

extern "C" long long pconv_optim_workspace_bytes(int ntensor, int nsegment) {
  PCONV_REQUIRE(ntensor > 0 && nsegment > 0, "optim_workspace_bytes: bad counts");
  return (long long)kHeader + (long long)nsegment * (long long)sizeof(double);
}

extern "C" int pconv_optim_sqnorm(const pconv_optim_tensor *records, const int32_t *segments, const long long *counts,
                                  int ntensor, int nsegment, float clip, void *workspace, void *stream) {
  int rc = check_tables("optim_sqnorm", records, segments, counts, ntensor, nsegment, workspace);
  if (rc < 0) return rc;
  double *partials = reinterpret_cast<double *>(static_cast<char *>(workspace) + kHeader);
  hipLaunchKernelGGL(optim_sqnorm_kernel, dim3((unsigned)nsegment), dim3(kBlock), 0, as_stream(stream), records, segments,
                     partials);
  hipLaunchKernelGGL(optim_close_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), partials, nsegment, clip,
                     static_cast<Workspace *>(workspace));
  PCONV_LAUNCH_CHECK("optim_sqnorm");
  return PCONV_OK;
}

extern "C" int pconv_optim_adam(const pconv_optim_tensor *records, const int32_t *segments, const long long *counts,
                                int ntensor, int nsegment, const void *workspace, void *stream) {
  int rc = check_tables("optim_adam", records, segments, counts, ntensor, nsegment, workspace);
  if (rc < 0) return rc;
  hipLaunchKernelGGL(optim_adam_kernel, dim3((unsigned)nsegment), dim3(kBlock), 0, as_stream(stream), records, segments,
                     static_cast<const Workspace *>(workspace));
  PCONV_LAUNCH_CHECK("optim_adam");
  return PCONV_OK;
}
