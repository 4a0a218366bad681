// The pole / seam rule of ERP frames of any size (include/pconv_hip.h, pconv_erp_coded_size) as the frame kernels
// apply it: the geometry of one launch, the source row / column of a coded pixel, and the staging of one row of
// samples of any alignment through LDS.  Shared by csrc/erp_size.hip and csrc/yuv.hip.
#pragma once
#include "common.h"

namespace {

constexpr int kBlock = 256;

struct ErpGeom {
  int h, w, H, W, top, m, half;
};

__device__ __forceinline__ int erp_src_row(const ErpGeom &g, int yc, bool &flip) {
  int y = yc - g.top;
  flip = false;
  if (y < 0) {
    y = -1 - y;
    flip = true;
  } else if (y >= g.h) {
    y = 2 * g.h - 1 - y;
    flip = true;
  }
  return min(max(y, 0), g.h - 1);
}

__device__ __forceinline__ int erp_src_col(const ErpGeom &g, int xc, bool flip) {
  int x = xc < g.w ? xc : (xc - g.w < g.m ? g.w - 1 : 0);
  if (flip) {
    x += g.half;
    if (x >= g.w) x -= g.w;
  }
  return x;
}

// bytes [0, nbytes) of `src` (any alignment) -> lds[a + i], a = src & 3: the row's whole dwords are read as dwords
// and land on aligned LDS dwords, the head and tail bytes one by one
__device__ __forceinline__ void stage_row_bytes(const uint8_t *__restrict__ src, int nbytes, uint8_t *lds) {
  const int a = (int)(reinterpret_cast<uintptr_t>(src) & 3);
  const int i0 = (4 - a) & 3;  // first byte of the row on a dword boundary
  const int nd = nbytes > i0 ? (nbytes - i0) >> 2 : 0;
  const uint32_t *body = reinterpret_cast<const uint32_t *>(src + i0);
  uint32_t *lds_body = reinterpret_cast<uint32_t *>(lds + a + i0);
  for (int k = threadIdx.x; k < nd; k += kBlock) lds_body[k] = body[k];
  const int tail0 = i0 + 4 * nd, ragged = i0 + (nbytes - tail0);
  for (int k = threadIdx.x; k < ragged; k += kBlock) {
    const int i = k < i0 ? k : tail0 + (k - i0);
    if (i < nbytes) lds[a + i] = src[i];
  }
}

}  // namespace
