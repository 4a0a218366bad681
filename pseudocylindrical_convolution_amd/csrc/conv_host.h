// Host side shared by the tile convolutions (conv.hip, wino.hip / wino_flat.hip, wino42.hip): the
// strided tensor view, the Winograd epilogue and the argument checks of the Winograd entry points.
// A kernel file adds its own tile arithmetic and launch.
#pragma once
#include "common.h"

// conv.hip: floats of the [red_pad][cout_pad] slab a (cout, cin, k, k) weight packs to, k in {1, 3, 5}: cout padded to
// the widest workgroup tile, cin to whole LDS stages.  64-bit: the caller checks the range.
long long pconv_conv_packed_floats(int cout, int cin, int k, int *cout_pad, int *red_pad);

// (anonymous like the kernels that take these structs by value: every translation unit has its own)
namespace {

// element strides of a (tile, channel, row, column) tensor whose columns are contiguous:
// lets a convolution read from / write into the interior of a padded buffer
struct ConvView {
  long long ts, cs;
  int rs;
};
using WView = ConvView;  // the Winograd kernels' name for it

struct WEpilogue {
  const float *bias, *slope, *residual;
  const int32_t *col_limit;
  int npart, act, trim, d2w;
  WView vres;
};

inline ConvView dense_view(int c, int h, int w) { return {(long long)c * h * w, (long long)h * w, w}; }

// views[3*i .. 3*i+2] = (tile, channel, row) strides of tensor i, or a dense view when views is null
inline ConvView view_at(const long long *views, int i, int c, int h, int w) {
  if (!views) return dense_view(c, h, w);
  return {views[3 * i], views[3 * i + 1], (int)views[3 * i + 2]};
}

inline bool view_ok(const ConvView &v, int c, int h, int w) {
  return v.rs >= w && v.cs >= (long long)(h - 1) * v.rs + w && v.ts >= (long long)(c - 1) * v.cs + (long long)(h - 1) * v.rs + w;
}

// rows of a view start on even element offsets from an 8-byte aligned base (float2 / float4 accesses)
inline bool view_aligned8(const ConvView &v, const void *base) {
  return v.rs % 2 == 0 && v.cs % 2 == 0 && v.ts % 2 == 0 && (reinterpret_cast<uintptr_t>(base) & 7) == 0;
}

// Argument checks of a Winograd 3x3 stride-1 entry point `name`, and the views / epilogue its kernel takes.
// supported: the kernel's own shape predicate; kc: input channels per stage (the span of a 32-bit byte offset);
// d2w_any_alignment: the depth-to-width store of the kernel does not need 8-byte aligned output rows.
inline int wino_check_args(const char *name, int (*supported)(int, int, int, int, int), int kc, bool d2w_any_alignment,
                           const float *in, const float *packed_u, const float *bias, float *out, int cin, int h, int w,
                           int cout, int act, const float *slope, const int32_t *col_limit, int npart,
                           const float *residual, int trim, int d2w, const long long *views, WView *vin, WView *vout,
                           WEpilogue *ep) {
  PCONV_REQUIRE(in && packed_u && out, "%s: null pointer", name);
  PCONV_REQUIRE(supported(cin, h, w, cout, d2w), "%s: unsupported shape %d x %d x %d -> %d", name, cin, h, w, cout);
  PCONV_REQUIRE(act == 0 || (act == 1 && slope), "%s: bad activation %d", name, act);
  PCONV_REQUIRE(!d2w || (!residual && !trim), "%s: depth-to-width takes no residual / trim", name);
  PCONV_REQUIRE(!col_limit || npart > 0, "%s: col_limit needs npart", name);
  PCONV_REQUIRE(!trim || col_limit, "%s: trim needs col_limit", name);
  PCONV_REQUIRE(residual != out, "%s: residual must not alias the output", name);
  const int ho = h - 2, wo = w - 2;
  const int oc = d2w ? cout / 4 : cout, oh = d2w ? 2 * ho : ho, ow = d2w ? 2 * wo : wo;
  *vin = view_at(views, 0, cin, h, w), *vout = view_at(views, 1, oc, oh, ow);
  *ep = {bias, slope, residual, col_limit, npart, act, trim, d2w, view_at(views, 2, cout, ho, wo)};
  PCONV_REQUIRE(view_ok(*vin, cin, h, w) && view_ok(*vout, oc, oh, ow) && (!residual || view_ok(ep->vres, cout, ho, wo)),
                "%s: strides overlap", name);
  PCONV_REQUIRE(((long long)(kc - 1) * vin->cs + (long long)(h - 1) * vin->rs + w) * 4 < (1LL << 32),
                "%s: input channel stride too large for 32-bit byte offsets inside a chunk", name);
  PCONV_REQUIRE((d2w && d2w_any_alignment) || view_aligned8(*vout, out), "%s: output rows must be 8-byte aligned", name);
  PCONV_REQUIRE(!residual || view_aligned8(ep->vres, residual), "%s: residual rows must be 8-byte aligned", name);
  return PCONV_OK;
}

}  // namespace
