// Panoramas of any size: the pole / seam padding of an h x w ERP frame to the coded size H x W (DESIGN.md §4,
// "Any ERP size").  The rule is a pure gather (include/pconv_hip.h, pconv_erp_coded_size):
//   y = y' - top; rows above / below the image continue across the pole (mirrored row, longitude + w/2);
//   columns x' >= w: the left half of the pad repeats column w-1, the right half column 0 (the seam's wrap).
// Three kernels apply it at the PCIe boundary and on the device: uint8 (n,h,w,3) -> padded float32 (n,3,H,W) with
// img2tensor's division, float32 (n,3,h,w) -> (n,3,H,W), and the decoder's crop float32 (n,3,H,W) -> uint8 (n,h,w,3)
// with tensor2img's cast.  One workgroup per (frame, row); the interleaved uint8 row (3w bytes, any alignment, any w)
// goes through LDS so that the global side moves aligned dwords, bytes only at the row's two ragged ends.
#include "common.h"
#include "erp_rule.h"

namespace {

constexpr int kMaxRowBytes = 65536 - 32;  // LDS of one row: 3w + 12 bytes, at most 64 KiB per workgroup

// uint8 (n, h, w, 3) -> float32 (n, 3, H, W) = float(u8) / 255.f (correctly rounded) under the padding rule
__global__ __launch_bounds__(kBlock) void frames_u8_to_f32_erp_pad_kernel(const uint8_t *__restrict__ in,
                                                                          float *__restrict__ out, ErpGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t row[];
  const int yc = blockIdx.x, f = blockIdx.y;
  bool flip;
  const int y = erp_src_row(g, yc, flip);
  const uint8_t *src = in + ((long long)f * g.h + y) * (3LL * g.w);
  stage_row_bytes(src, 3 * g.w, row);
  __syncthreads();
  const uint8_t *px = row + (reinterpret_cast<uintptr_t>(src) & 3);
  const long long plane = (long long)g.H * g.W;
  float *dst = out + (long long)f * 3 * plane + (long long)yc * g.W;
  for (int q = threadIdx.x; q < g.W / 4; q += kBlock) {
    float v[3][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint8_t *p = px + 3 * erp_src_col(g, 4 * q + j, flip);
#pragma unroll
      for (int ch = 0; ch < 3; ch++) v[ch][j] = __fdiv_rn((float)p[ch], 255.f);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
      *reinterpret_cast<float4 *>(dst + ch * plane + 4 * q) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
  }
}

// float32 (n, 3, h, w) -> (n, 3, H, W) under the padding rule.  Source rows have any width (no 16-byte alignment):
// 4-byte loads, consecutive lanes on consecutive columns; the coded rows are 64-byte aligned: 16-byte stores.
__global__ __launch_bounds__(kBlock) void erp_pad_f32_kernel(const float *__restrict__ in, float *__restrict__ out,
                                                             ErpGeom g) {
  const int yc = blockIdx.x, f = blockIdx.y;
  bool flip;
  const int y = erp_src_row(g, yc, flip);
  const long long splane = (long long)g.h * g.w, plane = (long long)g.H * g.W;
  const float *src = in + (long long)f * 3 * splane + (long long)y * g.w;
  float *dst = out + (long long)f * 3 * plane + (long long)yc * g.W;
  for (int q = threadIdx.x; q < g.W / 4; q += kBlock) {
    int x[4];
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = erp_src_col(g, 4 * q + j, flip);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float *s = src + ch * splane;
      *reinterpret_cast<float4 *>(dst + ch * plane + 4 * q) = make_float4(s[x[0]], s[x[1]], s[x[2]], s[x[3]]);
    }
  }
}

__device__ __forceinline__ unsigned to_u8_like_numpy(float v) { return (unsigned)(int)(v * 255.f) & 255u; }

// float32 (n, 3, H, W) rows top..top+h-1, columns 0..w-1 -> uint8 (n, h, w, 3) = (uint8)(int)(x * 255.f).  A lane
// converts 4 pixels (three 16-byte loads) into three packed dwords at LDS byte 12q; the row then leaves in dwords
// aligned to the OUTPUT's address (v_alignbyte of two LDS dwords), bytes only at the ragged ends.
__global__ __launch_bounds__(kBlock) void frames_f32_to_u8_crop_kernel(const float *__restrict__ in,
                                                                       uint8_t *__restrict__ out, ErpGeom g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t row[];
  const int y = blockIdx.x, f = blockIdx.y;
  const long long plane = (long long)g.H * g.W;
  const float *src = in + (long long)f * 3 * plane + (long long)(g.top + y) * g.W;
  uint32_t *lds = reinterpret_cast<uint32_t *>(row);
  const int nq = (g.w + 3) / 4;  // 4q + 3 < W: the last quad's extra columns are read, not written
  for (int q = threadIdx.x; q < nq; q += kBlock) {
    unsigned px[4][3];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float4 v = *reinterpret_cast<const float4 *>(src + ch * plane + 4 * q);
      px[0][ch] = to_u8_like_numpy(v.x), px[1][ch] = to_u8_like_numpy(v.y);
      px[2][ch] = to_u8_like_numpy(v.z), px[3][ch] = to_u8_like_numpy(v.w);
    }
    lds[3 * q] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
    lds[3 * q + 1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
    lds[3 * q + 2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
  }
  __syncthreads();
  const int nbytes = 3 * g.w;
  uint8_t *dst = out + ((long long)f * g.h + y) * nbytes;
  const int a = (int)(reinterpret_cast<uintptr_t>(dst) & 3);
  const int i0 = (4 - a) & 3;
  const int nd = nbytes > i0 ? (nbytes - i0) >> 2 : 0;
  uint32_t *body = reinterpret_cast<uint32_t *>(dst + i0);
  for (int k = threadIdx.x; k < nd; k += kBlock) {
    const int i = i0 + 4 * k;  // output bytes i..i+3 = LDS bytes i..i+3: dwords i/4 and i/4 + 1, shifted by i & 3
    const uint32_t lo = lds[i >> 2], hi = (i & 3) ? lds[(i >> 2) + 1] : 0u;
    body[k] = __builtin_amdgcn_alignbyte(hi, lo, (unsigned)(i & 3));
  }
  const int tail0 = i0 + 4 * nd, ragged = i0 + (nbytes - tail0);
  for (int k = threadIdx.x; k < ragged; k += kBlock) {
    const int i = k < i0 ? k : tail0 + (k - i0);
    if (i < nbytes) dst[i] = row[i];
  }
}

int erp_geom(const char *what, int n, int h, int w, ErpGeom *g) {
  PCONV_REQUIRE(n > 0 && n <= 65535, "%s: bad frame count %d", what, n);
  PCONV_REQUIRE(pconv_erp_coded_size(h, w, &g->H, &g->W, &g->top) == PCONV_OK, "%s: bad ERP size %dx%d", what, w, h);
  PCONV_REQUIRE(3 * w <= kMaxRowBytes, "%s: width %d exceeds the %d bytes of a staged row", what, w, kMaxRowBytes);
  g->h = h, g->w = w;
  g->m = (g->W - w + 1) / 2;
  g->half = w / 2;
  return PCONV_OK;
}

// 3w bytes + up to 3 of misalignment (staging) or of the last quad's 12 bytes (crop) + the crop's lookahead dword
inline size_t row_lds_bytes(int w) { return (size_t)((3 * w + 12 + 15) & ~15); }

}  // namespace

extern "C" int pconv_erp_coded_size(int h, int w, int *H, int *W, int *top) {
  PCONV_REQUIRE(H && W && top, "erp_coded_size: null pointer");
  PCONV_REQUIRE(h >= 2 && w >= 2, "erp_coded_size: the ERP size %dx%d is below 2x2", w, h);
  PCONV_REQUIRE(h <= (1 << 20) && w <= (1 << 20), "erp_coded_size: the ERP size %dx%d exceeds 2^20", w, h);
  const int hc = 256 * ((h + 255) / 256), wc = 16 * ((w + 15) / 16);
  *H = hc;
  *W = wc;
  *top = (hc - h) / 2;
  return PCONV_OK;
}

extern "C" int pconv_frames_u8_to_f32_erp(const uint8_t *in, float *out, int n, int height, int width, void *stream) {
  PCONV_REQUIRE(in && out, "frames_u8_to_f32_erp: null pointer");
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0, "frames_u8_to_f32_erp: the tensor must be 16-byte aligned");
  ErpGeom g;
  if (erp_geom("frames_u8_to_f32_erp", n, height, width, &g) != PCONV_OK) return PCONV_EINVAL;
  hipLaunchKernelGGL(frames_u8_to_f32_erp_pad_kernel, dim3(g.H, n), dim3(kBlock), row_lds_bytes(width),
                     as_stream(stream), in, out, g);
  PCONV_LAUNCH_CHECK("frames_u8_to_f32_erp");
  return PCONV_OK;
}

extern "C" int pconv_erp_pad_f32(const float *in, float *out, int n, int height, int width, void *stream) {
  PCONV_REQUIRE(in && out, "erp_pad_f32: null pointer");
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(in) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                "erp_pad_f32: the input must be 4-byte aligned, the output 16-byte aligned");
  ErpGeom g;
  if (erp_geom("erp_pad_f32", n, height, width, &g) != PCONV_OK) return PCONV_EINVAL;
  hipLaunchKernelGGL(erp_pad_f32_kernel, dim3(g.H, n), dim3(kBlock), 0, as_stream(stream), in, out, g);
  PCONV_LAUNCH_CHECK("erp_pad_f32");
  return PCONV_OK;
}

extern "C" int pconv_frames_f32_to_u8_crop(const float *in, uint8_t *out, int n, int height, int width, void *stream) {
  PCONV_REQUIRE(in && out, "frames_f32_to_u8_crop: null pointer");
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(in) & 15) == 0, "frames_f32_to_u8_crop: the tensor must be 16-byte aligned");
  ErpGeom g;
  if (erp_geom("frames_f32_to_u8_crop", n, height, width, &g) != PCONV_OK) return PCONV_EINVAL;
  hipLaunchKernelGGL(frames_f32_to_u8_crop_kernel, dim3(height, n), dim3(kBlock), row_lds_bytes(width),
                     as_stream(stream), in, out, g);
  PCONV_LAUNCH_CHECK("frames_f32_to_u8_crop");
  return PCONV_OK;
}
