// Ordered backward of "6 x 6 sampler over a map plus ss x ss average" (the definition is in
// include/pconv_hip.h, pconv_remap_backward_f32): the gradient of the viewport renderer (viewport.hip) and, with ss = 1
// and the frame as the grid, of the sphere rotation (erp_rotate.hip), with respect to the source frames.
//   remap_backward_f32_kernel  a gather: a lane owns one source pixel of one frame and walks that pixel's list of
//                              pconv_host_remap_reverse once, front to back, for up to kPlanes planes at a time (one
//                              accumulator per plane: the decoding of an entry, its record and its two weights are
//                              shared by the planes, the sums are not).  A list is never split across lanes, so the
//                              order of a sum is the list's order whatever the grid is.  No atomics, no workspace.
//                              The phase table (6 KB) is staged in LDS -- but only by a workgroup that has a list to
//                              walk: most source pixels of a view have none (a 90 degree view covers a sixth of the
//                              sphere), and a workgroup of such pixels reads its starts, votes and leaves (storing
//                              +0 first when it does not accumulate).
// Every index read from a list is reduced to one inside the map (an entry outside 0 .. 36 gh gw - 1 is skipped, a start
// outside it clamped), so no list content makes the kernel read outside `map` or `gout`; each lane stores only its own
// pixel.
#include "sphere_sampler.h"

namespace {

constexpr int kBlock = 256;
constexpr int kFoot = kTaps * kTaps;  // entries per grid sample
constexpr int kPlanes = 4;            // planes a lane carries through one walk of its list
constexpr int kAhead = 4;             // entries of a list whose loads are in flight together

__global__ __launch_bounds__(kBlock) void remap_backward_f32_kernel(
    const float *__restrict__ gout, float *__restrict__ gin, const int2 *__restrict__ map, const float *__restrict__ phases,
    const int32_t *__restrict__ rev_start, const int32_t *__restrict__ rev_entry, int C, int hw, int vw, int gw, int ss,
    int total, long long vplane, long long gout_frame_stride, float inv, int accumulate) {
  __shared__ float table[kPhases * kTaps];
  const int d = blockIdx.x * kBlock + threadIdx.x;  // h * w < 2^29
  int lo = 0, hi = 0;
  if (d < hw) {
    lo = min(max(rev_start[d], 0), total);
    hi = min(max(rev_start[d + 1], 0), total);
  }
  const int groups = (C + kPlanes - 1) / kPlanes;
  const int frame = blockIdx.y / groups, c0 = (blockIdx.y - frame * groups) * kPlanes;
  const int planes = min(kPlanes, C - c0);
  float *dst = gin + ((long long)frame * C + c0) * hw + d;
  if (!__syncthreads_or(lo < hi)) {  // no list in this workgroup
    if (!accumulate && d < hw)
      for (int k = 0; k < planes; k++) dst[(long long)k * hw] = 0.f;
    return;
  }
  stage_phase_table<kBlock>(table, phases);
  if (d >= hw || (accumulate && lo >= hi)) return;
  const float *g = gout + (long long)frame * gout_frame_stride + (long long)c0 * vplane;
  float acc[kPlanes];
#pragma unroll
  for (int k = 0; k < kPlanes; k++) acc[k] = accumulate && k < planes ? dst[(long long)k * hw] : 0.f;
  // kAhead entries at a time: their loads (entry -> record -> weights and gradient values, a chain of three) are
  // issued together, the additions then made one entry after the other, in the list's order
  for (int at = lo; at < hi; at += kAhead) {
    float term[kAhead][kPlanes];
    bool live[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; u++) {
      const int e = at + u < hi ? rev_entry[at + u] : -1;
      live[u] = (unsigned)e < (unsigned)total;
      const int s = live[u] ? e / kFoot : 0, tap = live[u] ? e - s * kFoot : 0;
      const int a = tap / kTaps, b = tap - a * kTaps;
      const int2 rec = map[s];
      const float wy = table[record_phase(rec.y) * kTaps + a];
      const float wx = table[record_phase(rec.x) * kTaps + b];
      const int r = s / gw, q = s - r * gw;
      const float *gp = g + ((long long)(r / ss) * vw + q / ss);
#pragma unroll
      for (int k = 0; k < kPlanes; k++) {
        float v = k < planes ? gp[(long long)k * vplane] : 0.f;
        if (ss > 1) v = __fmul_rn(v, inv);
        term[u][k] = __fmul_rn(__fmul_rn(v, wy), wx);
      }
    }
#pragma unroll
    for (int u = 0; u < kAhead; u++)
      if (live[u]) {
#pragma unroll
        for (int k = 0; k < kPlanes; k++) acc[k] = __fadd_rn(acc[k], term[u][k]);
      }
  }
#pragma unroll
  for (int k = 0; k < kPlanes; k++)
    if (k < planes) dst[(long long)k * hw] = acc[k];
}

}  // namespace

extern "C" int pconv_remap_backward_f32(const float *gout, float *gin, const int32_t *map, const float *phases,
                                        const int32_t *rev_start, const int32_t *rev_entry, int n, int c, int h, int w, int vh,
                                        int vw, int ss, long long gout_frame_stride, int accumulate, void *stream) {
  PCONV_REQUIRE(gout && gin && map && phases, "remap_backward_f32: null pointer");
  PCONV_REQUIRE(rev_start && rev_entry, "remap_backward_f32: null list pointer");
  if (planes_ok("remap_backward_f32", n, c) != PCONV_OK || frame_ok("remap_backward_f32", "source ", h, w) != PCONV_OK ||
      side_ok("remap_backward_f32", "view ", vh, vw) != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(ss >= 1 && ss <= PCONV_VIEWPORT_MAX_SS, "remap_backward_f32: ss = %d supersampling is outside 1 .. %d", ss,
                PCONV_VIEWPORT_MAX_SS);
  PCONV_REQUIRE(8LL * ss * ss * vh * vw < (1LL << 31), "remap_backward_f32: a map of %dx%d records is 2^31 bytes or more",
                vw * ss, vh * ss);
  const long long total = pconv_host_remap_reverse_size(vh * ss, vw * ss);
  PCONV_REQUIRE(total > 0, "remap_backward_f32: the %lld list entries of a %dx%d grid do not fit int32",
                36LL * ss * ss * vh * vw, vw * ss, vh * ss);
  const long long frame = (long long)c * vh * vw;
  PCONV_REQUIRE(4LL * frame < (1LL << 31), "remap_backward_f32: a gradient frame of %d planes of %dx%d float32 is 2^31 bytes "
                "or more", c, vw, vh);
  PCONV_REQUIRE(gout_frame_stride >= frame, "remap_backward_f32: the gradient frame stride %lld is below C * vh * vw = %lld",
                gout_frame_stride, frame);
  if (aligned_ok("remap_backward_f32", addr(gout) | addr(gin) | addr(phases) | addr(rev_start) | addr(rev_entry),
                 "the tensors and lists", addr(map), "the map") != PCONV_OK)
    return PCONV_EINVAL;
  PCONV_REQUIRE(gin != gout, "remap_backward_f32: gin and gout must be distinct");
  const int hw = h * w;
  const int groups = (c + kPlanes - 1) / kPlanes;  // n * groups <= n * C <= 65535
  hipLaunchKernelGGL(remap_backward_f32_kernel, dim3((unsigned)((hw + kBlock - 1) / kBlock), (unsigned)(n * groups)),
                     dim3(kBlock), 0, as_stream(stream), gout, gin, reinterpret_cast<const int2 *>(map), phases, rev_start,
                     rev_entry, c, hw, vw, vw * ss, ss, (int)total, (long long)vh * vw, gout_frame_stride,
                     (float)(1.0 / (ss * ss)), accumulate ? 1 : 0);
  PCONV_LAUNCH_CHECK("remap_backward_f32");
  return PCONV_OK;
}
