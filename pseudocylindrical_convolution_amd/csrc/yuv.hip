// Planar 4:2:0 YCbCr frames in and out of the codec (include/pconv_hip.h, "YUV 4:2:0 frames"): the colour conversion
// fused with the pole / seam pad on the way in and with the crop on the way out.  Formats: yuv420p and nv12 (uint8),
// yuv420p10le (uint16, samples modulo 1024).  Every operation of the definition is one fp32 rounding, written with
// __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn so that nothing is contracted; pseudocylindrical_convolution_amd/
// yuv.py states the same arithmetic in torch and the tests compare the two bit for bit.
//
// Ingest: one workgroup per (frame, coded row).  The source luma row and the two chroma rows it blends are staged in
// LDS (aligned dwords on the body, bytes at ragged ends: stage_row_bytes); the vertical blend is done once per chroma
// column, kept as the integer Ca + 3*Cb (<= 4092; 0.25f*Ca + 0.75f*Cb is that integer times 0.25f, exactly, and the
// horizontal mean 0.5f*(V[i] + V[i+1]) the sum of two of them times 0.125f, exactly); each lane then converts 4
// adjacent coded pixels per plane -- the rule's gather is applied to each pixel's SOURCE column, whose parity decides
// between the co-sited and the interpolated chroma -- and stores three float4s.
// Egress: one workgroup per (frame, chroma row) = two luma rows.  float4 loads; luma is quantised and packed at once,
// the full-resolution cb / cr row means go to LDS, the 3-tap wrap filter reads them, and the packed rows leave in
// dwords aligned to the destination, bytes at the ends.
#include "common.h"
#include "erp_rule.h"

namespace {

constexpr int kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;

struct YuvCoef {
  float yo, ys, co, cs, qmax;       // range: offsets, scales, 2^d - 1
  float kr, kg, kb, a, b, c, dd;    // matrix: the seven floats of the definition
};

__host__ __device__ inline int round4(int v) { return (v + 3) & ~3; }

template <typename T>
__device__ __forceinline__ int code(T v) {
  return sizeof(T) == 2 ? (int)v & 1023 : (int)v;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// LDS of the ingest kernel: the luma row, 4 planar (or 2 interleaved) chroma rows, each with room for its source's
// misalignment, then the two rows of blended sums (uint16)
template <typename T, bool NV12>
__host__ __device__ inline void ingest_layout(int w, int *luma_bytes, int *chroma_bytes, int *total) {
  *luma_bytes = round4(w * (int)sizeof(T) + 3);
  *chroma_bytes = round4((NV12 ? w : w / 2) * (int)sizeof(T) + 3);
  *total = *luma_bytes + (NV12 ? 2 : 4) * *chroma_bytes + 2 * round4(w);   // 2 x (w/2) uint16
}

template <typename T>
__device__ __forceinline__ const T *staged(const uint8_t *lds, const T *src) {
  return reinterpret_cast<const T *>(lds + (reinterpret_cast<uintptr_t>(src) & 3));
}

template <typename T, bool NV12>
__global__ __launch_bounds__(kBlock) void frames_yuv420_to_f32_kernel(const T *__restrict__ in, float *__restrict__ out,
                                                                      ErpGeom g, YuvCoef k) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int yc = blockIdx.x, f = blockIdx.y;
  bool flip;
  const int y = erp_src_row(g, yc, flip);
  const int w2 = g.w >> 1, h2 = g.h >> 1, j = y >> 1;
  // luma row 2j blends chroma rows max(j-1, 0) and j, row 2j+1 rows j and min(j+1, h/2-1): 1/4 of `jo`, 3/4 of `j`
  const int jo = (y & 1) ? min(j + 1, h2 - 1) : max(j - 1, 0);
  const long long luma = (long long)g.h * g.w;
  const T *frame = in + (long long)f * (luma + 2LL * h2 * w2);
  int lb, cb_bytes, total;
  ingest_layout<T, NV12>(g.w, &lb, &cb_bytes, &total);
  const T *ysrc = frame + (long long)y * g.w;
  uint8_t *crow = lds + lb;
  const T *csrc[4];
  if (NV12) {
    csrc[0] = frame + luma + (long long)j * g.w, csrc[1] = frame + luma + (long long)jo * g.w;
    csrc[2] = csrc[0], csrc[3] = csrc[1];
  } else {
    const T *u = frame + luma, *v = u + (long long)h2 * w2;
    csrc[0] = u + (long long)j * w2, csrc[1] = u + (long long)jo * w2;
    csrc[2] = v + (long long)j * w2, csrc[3] = v + (long long)jo * w2;
  }
  stage_row_bytes(reinterpret_cast<const uint8_t *>(ysrc), g.w * (int)sizeof(T), lds);
#pragma unroll
  for (int r = 0; r < (NV12 ? 2 : 4); r++)
    stage_row_bytes(reinterpret_cast<const uint8_t *>(csrc[r]), (NV12 ? g.w : w2) * (int)sizeof(T), crow + r * cb_bytes);
  __syncthreads();
  uint16_t *su = reinterpret_cast<uint16_t *>(crow + (NV12 ? 2 : 4) * cb_bytes), *sv = su + round4(g.w) / 2;
  {
    const T *c0 = staged(crow, csrc[0]), *c1 = staged(crow + cb_bytes, csrc[1]);
    const T *c2 = NV12 ? c0 : staged(crow + 2 * cb_bytes, csrc[2]), *c3 = NV12 ? c1 : staged(crow + 3 * cb_bytes, csrc[3]);
    for (int i = threadIdx.x; i < w2; i += kBlock) {
      const int iu = NV12 ? 2 * i : i, iv = NV12 ? 2 * i + 1 : i;
      su[i] = (uint16_t)(code(c1[iu]) + 3 * code(c0[iu]));
      sv[i] = (uint16_t)(code(c3[iv]) + 3 * code(c2[iv]));
    }
  }
  __syncthreads();
  const T *yrow = staged(lds, ysrc);
  const long long plane = (long long)g.H * g.W;
  float *dst = out + (long long)f * 3 * plane + (long long)yc * g.W;
  for (int q = threadIdx.x; q < g.W / 4; q += kBlock) {
    float v[3][4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int x = erp_src_col(g, 4 * q + p, flip), i = x >> 1;
      float cu, cv;
      if (x & 1) {
        const int i1 = i + 1 == w2 ? 0 : i + 1;   // the seam wraps
        cu = __fmul_rn(0.125f, (float)((int)su[i] + (int)su[i1]));
        cv = __fmul_rn(0.125f, (float)((int)sv[i] + (int)sv[i1]));
      } else {
        cu = __fmul_rn(0.25f, (float)su[i]);
        cv = __fmul_rn(0.25f, (float)sv[i]);
      }
      const float yy = __fdiv_rn(__fsub_rn((float)code(yrow[x]), k.yo), k.ys);
      const float cb = __fdiv_rn(__fsub_rn(cu, k.co), k.cs), cr = __fdiv_rn(__fsub_rn(cv, k.co), k.cs);
      v[0][p] = clamp01(__fadd_rn(yy, __fmul_rn(k.a, cr)));
      v[1][p] = clamp01(__fsub_rn(__fsub_rn(yy, __fmul_rn(k.b, cb)), __fmul_rn(k.c, cr)));
      v[2][p] = clamp01(__fadd_rn(yy, __fmul_rn(k.dd, cb)));
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      *reinterpret_cast<float4 *>(dst + ch * plane + 4 * q) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
  }
}

// q = clamp(floor((p*scale + offset) + 0.5f), 0, 2^d - 1)
__device__ __forceinline__ unsigned quantise(float p, float scale, float offset, float qmax) {
  const float q = floorf(__fadd_rn(__fadd_rn(__fmul_rn(p, scale), offset), 0.5f));
  return (unsigned)fminf(fmaxf(q, 0.f), qmax);
}

// 4 samples, the first in the lowest bits, into one (uint8) or two (uint16) dwords at sample index 4 * q4
template <typename T>
__device__ __forceinline__ void pack4(uint32_t *row, int q4, const unsigned s[4]) {
  if (sizeof(T) == 1) {
    row[q4] = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
  } else {
    row[2 * q4] = s[0] | (s[1] << 16);
    row[2 * q4 + 1] = s[2] | (s[3] << 16);
  }
}

// LDS bytes [0, nbytes) (from an aligned dword on) -> dst (any alignment): dwords aligned to dst on the body, each
// put together from two LDS dwords, bytes at the two ragged ends.  The LDS row has one dword beyond round4(nbytes).
__device__ __forceinline__ void store_row_bytes(uint8_t *__restrict__ dst, int nbytes, const uint32_t *lds) {
  const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
  const int i0 = (4 - a) & 3;
  const int nd = nbytes > i0 ? (nbytes - i0) >> 2 : 0;
  uint32_t *body = reinterpret_cast<uint32_t *>(dst + i0);
  for (int t = threadIdx.x; t < nd; t += kBlock) {
    const int i = i0 + 4 * t;
    const uint32_t lo = lds[i >> 2], hi = (i & 3) ? lds[(i >> 2) + 1] : 0u;
    body[t] = __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(i & 3));
  }
  const uint8_t *bytes = reinterpret_cast<const uint8_t *>(lds);
  const int tail0 = i0 + 4 * nd, ragged = i0 + (nbytes - tail0);
  for (int t = threadIdx.x; t < ragged; t += kBlock) {
    const int i = t < i0 ? t : tail0 + (t - i0);
    if (i < nbytes) dst[i] = bytes[i];
  }
}

// LDS of the egress kernel, in dwords: two packed luma rows, the packed chroma (two planar rows or one interleaved),
// each with the lookahead dword of store_row_bytes, then the cb and cr row means (float, w rounded up to 4)
template <typename T, bool NV12>
__host__ __device__ inline void egress_layout(int w, int *luma_dw, int *chroma_dw, int *total_bytes) {
  *luma_dw = round4(w * (int)sizeof(T)) / 4 + 1;
  *chroma_dw = NV12 ? round4(2 * round4(w / 2)) / 4 + 1 : round4(round4(w / 2) * (int)sizeof(T)) / 4 + 1;
  *total_bytes = 4 * (round4(2 * *luma_dw + (NV12 ? 1 : 2) * *chroma_dw) + 2 * round4(w));   // the floats 16-byte aligned
}

template <typename T, bool NV12>
__global__ __launch_bounds__(kBlock) void frames_f32_to_yuv420_kernel(const float *__restrict__ in, T *__restrict__ out,
                                                                      ErpGeom g, YuvCoef k) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int j = blockIdx.x, f = blockIdx.y;
  const int w2 = g.w >> 1, h2 = g.h >> 1;
  int ld, cd, total;
  egress_layout<T, NV12>(g.w, &ld, &cd, &total);
  uint32_t *lrow = reinterpret_cast<uint32_t *>(lds);          // [2][ld]
  uint32_t *crow = lrow + 2 * ld;                              // [2][cd] planar, [cd] interleaved
  float *mcb = reinterpret_cast<float *>(lrow + round4(2 * ld + (NV12 ? 1 : 2) * cd)), *mcr = mcb + round4(g.w);
  const long long plane = (long long)g.H * g.W;
  const float *src = in + (long long)f * 3 * plane + (long long)(g.top + 2 * j) * g.W;
  const int nq = (g.w + 3) / 4;  // 4q + 3 < W: the last quad's extra columns are read, never written out
  for (int q = threadIdx.x; q < nq; q += kBlock) {
    float cb[2][4], cr[2][4];
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const float *s = src + r * g.W + 4 * q;
      const float4 R4 = *reinterpret_cast<const float4 *>(s), G4 = *reinterpret_cast<const float4 *>(s + plane),
                   B4 = *reinterpret_cast<const float4 *>(s + 2 * plane);
      const float R[4] = {R4.x, R4.y, R4.z, R4.w}, G[4] = {G4.x, G4.y, G4.z, G4.w}, B[4] = {B4.x, B4.y, B4.z, B4.w};
      unsigned yq[4];
#pragma unroll
      for (int p = 0; p < 4; p++) {
        const float rr = clamp01(R[p]), gg = clamp01(G[p]), bb = clamp01(B[p]);
        const float yy = __fadd_rn(__fadd_rn(__fmul_rn(k.kr, rr), __fmul_rn(k.kg, gg)), __fmul_rn(k.kb, bb));
        cb[r][p] = __fdiv_rn(__fsub_rn(bb, yy), k.dd);
        cr[r][p] = __fdiv_rn(__fsub_rn(rr, yy), k.a);
        yq[p] = quantise(yy, k.ys, k.yo, k.qmax);
      }
      pack4<T>(lrow + r * ld, q, yq);
    }
    float mb[4], mr[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      mb[p] = __fmul_rn(0.5f, __fadd_rn(cb[0][p], cb[1][p]));
      mr[p] = __fmul_rn(0.5f, __fadd_rn(cr[0][p], cr[1][p]));
    }
    *reinterpret_cast<float4 *>(mcb + 4 * q) = make_float4(mb[0], mb[1], mb[2], mb[3]);
    *reinterpret_cast<float4 *>(mcr + 4 * q) = make_float4(mr[0], mr[1], mr[2], mr[3]);
  }
  __syncthreads();
  // C[i] = (0.25f*v[(2i-1) mod w] + 0.5f*v[2i]) + 0.25f*v[2i+1], 4 chroma columns per lane
  for (int q = threadIdx.x; q < (w2 + 3) / 4; q += kBlock) {
    unsigned uq[4], vq[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int i = 4 * q + p;
      uq[p] = vq[p] = 0;
      if (i < w2) {
        const int xm = i == 0 ? g.w - 1 : 2 * i - 1;
        const float cu = __fadd_rn(__fadd_rn(__fmul_rn(0.25f, mcb[xm]), __fmul_rn(0.5f, mcb[2 * i])), __fmul_rn(0.25f, mcb[2 * i + 1]));
        const float cv = __fadd_rn(__fadd_rn(__fmul_rn(0.25f, mcr[xm]), __fmul_rn(0.5f, mcr[2 * i])), __fmul_rn(0.25f, mcr[2 * i + 1]));
        uq[p] = quantise(cu, k.cs, k.co, k.qmax);
        vq[p] = quantise(cv, k.cs, k.co, k.qmax);
      }
    }
    if (NV12) {
      crow[2 * q] = uq[0] | (vq[0] << 8) | (uq[1] << 16) | (vq[1] << 24);
      crow[2 * q + 1] = uq[2] | (vq[2] << 8) | (uq[3] << 16) | (vq[3] << 24);
    } else {
      pack4<T>(crow, q, uq);
      pack4<T>(crow + cd, q, vq);
    }
  }
  __syncthreads();
  const long long luma = (long long)g.h * g.w;
  T *frame = out + (long long)f * (luma + 2LL * h2 * w2);
  const int lbytes = g.w * (int)sizeof(T);
  store_row_bytes(reinterpret_cast<uint8_t *>(frame + (long long)(2 * j) * g.w), lbytes, lrow);
  store_row_bytes(reinterpret_cast<uint8_t *>(frame + (long long)(2 * j + 1) * g.w), lbytes, lrow + ld);
  if (NV12) {
    store_row_bytes(reinterpret_cast<uint8_t *>(frame + luma + (long long)j * g.w), lbytes, crow);
  } else {
    T *u = frame + luma + (long long)j * w2;
    store_row_bytes(reinterpret_cast<uint8_t *>(u), w2 * (int)sizeof(T), crow);
    store_row_bytes(reinterpret_cast<uint8_t *>(u + (long long)h2 * w2), w2 * (int)sizeof(T), crow + cd);
  }
}

int yuv_coef(const char *what, int fmt, int matrix, int range, YuvCoef *k) {
  PCONV_REQUIRE(fmt == PCONV_YUV_420P || fmt == PCONV_YUV_NV12 || fmt == PCONV_YUV_420P10LE, "%s: unknown pixel format %d",
                what, fmt);
  PCONV_REQUIRE(matrix == PCONV_YUV_BT709 || matrix == PCONV_YUV_BT601, "%s: unknown matrix %d", what, matrix);
  PCONV_REQUIRE(range == PCONV_YUV_LIMITED || range == PCONV_YUV_FULL, "%s: unknown range %d", what, range);
  const int d = fmt == PCONV_YUV_420P10LE ? 10 : 8;
  const double s = (double)(1 << (d - 8)), peak = (double)((1 << d) - 1);
  const double Kr = matrix == PCONV_YUV_BT709 ? 0.2126 : 0.299, Kb = matrix == PCONV_YUV_BT709 ? 0.0722 : 0.114;
  const double Kg = 1.0 - Kr - Kb;
  const double a = 2 * (1 - Kr);
  const double dd = 2 * (1 - Kb);
  const double b = Kb * dd / Kg;
  const double c = Kr * a / Kg;
  k->kr = (float)Kr, k->kg = (float)Kg, k->kb = (float)Kb, k->a = (float)a, k->b = (float)b, k->c = (float)c, k->dd = (float)dd;
  if (range == PCONV_YUV_LIMITED) {
    k->yo = (float)(16 * s), k->ys = (float)(219 * s), k->co = (float)(128 * s), k->cs = (float)(224 * s);
  } else {
    k->yo = 0.f, k->ys = (float)peak, k->co = (float)(1 << (d - 1)), k->cs = (float)peak;
  }
  k->qmax = (float)peak;
  return PCONV_OK;
}

int yuv_geom(const char *what, const void *samples, const float *tensor, int n, int h, int w, int fmt, ErpGeom *g) {
  PCONV_REQUIRE(samples && tensor, "%s: null pointer", what);
  PCONV_REQUIRE(n > 0 && n <= 65535, "%s: bad frame count %d", what, n);
  PCONV_REQUIRE(h >= 2 && w >= 2 && h % 2 == 0 && w % 2 == 0, "%s: a 4:2:0 frame needs even sides of at least 2, got %dx%d",
                what, w, h);
  PCONV_REQUIRE(w <= PCONV_YUV_MAX_WIDTH, "%s: width %d exceeds the %d columns the LDS staging holds", what, w,
                PCONV_YUV_MAX_WIDTH);
  PCONV_REQUIRE(pconv_erp_coded_size(h, w, &g->H, &g->W, &g->top) == PCONV_OK, "%s: bad ERP size %dx%d", what, w, h);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(tensor) & 15) == 0, "%s: the float tensor must be 16-byte aligned", what);
  PCONV_REQUIRE(fmt != PCONV_YUV_420P10LE || (reinterpret_cast<uintptr_t>(samples) & 1) == 0,
                "%s: 16-bit samples must be 2-byte aligned", what);
  g->h = h, g->w = w;
  g->m = (g->W - w + 1) / 2;
  g->half = w / 2;
  return PCONV_OK;
}

// kernels that need more than the default 64 KiB of dynamic LDS (wide frames) have the limit raised once per device
template <typename Kernel>
int lds_limit(Kernel kernel, int bytes, std::atomic<unsigned long long> &raised, const char *what) {
  PCONV_REQUIRE(bytes <= kLdsMax, "%s: the row needs %d bytes of LDS, above %d", what, bytes, kLdsMax);
  return bytes > kLdsDefault ? pconv_raise_lds(kernel, (size_t)kLdsMax, raised, what) : PCONV_OK;
}

template <typename T, bool NV12>
int launch_ingest(const void *in, float *out, int n, const ErpGeom &g, const YuvCoef &k, void *stream) {
  static std::atomic<unsigned long long> raised{0};
  int lb, cb, total;
  ingest_layout<T, NV12>(g.w, &lb, &cb, &total);
  auto kernel = frames_yuv420_to_f32_kernel<T, NV12>;
  if (int rc = lds_limit(kernel, total, raised, "frames_yuv420_to_f32")) return rc;
  hipLaunchKernelGGL(kernel, dim3(g.H, n), dim3(kBlock), (size_t)((total + 15) & ~15), as_stream(stream),
                     static_cast<const T *>(in), out, g, k);
  PCONV_LAUNCH_CHECK("frames_yuv420_to_f32");
  return PCONV_OK;
}

template <typename T, bool NV12>
int launch_egress(const float *in, void *out, int n, const ErpGeom &g, const YuvCoef &k, void *stream) {
  static std::atomic<unsigned long long> raised{0};
  int ld, cd, total;
  egress_layout<T, NV12>(g.w, &ld, &cd, &total);
  auto kernel = frames_f32_to_yuv420_kernel<T, NV12>;
  if (int rc = lds_limit(kernel, total, raised, "frames_f32_to_yuv420")) return rc;
  hipLaunchKernelGGL(kernel, dim3(g.h / 2, n), dim3(kBlock), (size_t)((total + 15) & ~15), as_stream(stream), in,
                     static_cast<T *>(out), g, k);
  PCONV_LAUNCH_CHECK("frames_f32_to_yuv420");
  return PCONV_OK;
}

}  // namespace

extern "C" int pconv_frames_yuv420_to_f32(const void *in, float *out, int n, int h, int w, int fmt, int matrix, int range,
                                          void *stream) {
  YuvCoef k;
  ErpGeom g;
  if (yuv_coef("frames_yuv420_to_f32", fmt, matrix, range, &k) != PCONV_OK) return PCONV_EINVAL;
  if (yuv_geom("frames_yuv420_to_f32", in, out, n, h, w, fmt, &g) != PCONV_OK) return PCONV_EINVAL;
  switch (fmt) {
    case PCONV_YUV_420P: return launch_ingest<uint8_t, false>(in, out, n, g, k, stream);
    case PCONV_YUV_NV12: return launch_ingest<uint8_t, true>(in, out, n, g, k, stream);
    default: return launch_ingest<uint16_t, false>(in, out, n, g, k, stream);
  }
}

extern "C" int pconv_frames_f32_to_yuv420(const float *in, void *out, int n, int h, int w, int fmt, int matrix, int range,
                                          void *stream) {
  YuvCoef k;
  ErpGeom g;
  if (yuv_coef("frames_f32_to_yuv420", fmt, matrix, range, &k) != PCONV_OK) return PCONV_EINVAL;
  if (yuv_geom("frames_f32_to_yuv420", out, in, n, h, w, fmt, &g) != PCONV_OK) return PCONV_EINVAL;
  switch (fmt) {
    case PCONV_YUV_420P: return launch_egress<uint8_t, false>(in, out, n, g, k, stream);
    case PCONV_YUV_NV12: return launch_egress<uint8_t, true>(in, out, n, g, k, stream);
    default: return launch_egress<uint16_t, false>(in, out, n, g, k, stream);
  }
}
