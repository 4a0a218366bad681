/*
 * pconv_hip.h -- C ABI of libpconv_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the reference's native module `PCONV`
 * (reference: extension/main.cpp:4-137).  The reference binds 21 C++ op classes
 * with pybind11; a maintainer replacing it binds the flat entry points below
 * instead (see INTEGRATION.md for the ctypes / pybind stub).  No torch types
 * cross this boundary: plain device pointers, dims and a hipStream_t.
 *
 * Conventions
 *   - every tensor is fp32, NCHW, contiguous; the tile-batch index is
 *     n*npart + tile (reference: sphere_slice_cuda.cu:98-99).
 *   - `stream` is a hipStream_t passed as void*; kernels are launched on it and
 *     never synchronise.
 *   - device functions return 0 on success, a negative PCONV_E* code otherwise;
 *     pconv_last_error() returns a thread-local message.  (The reference only
 *     printf()s on failure, caffe_cuda_macro.h:21-33; the Python shim raises.)
 *   - "host" functions touch no GPU state; they build the integer/float tables
 *     the kernels consume and are bit-exact restatements of the reference's
 *     one-off table kernels, with element offsets kept as integers (the
 *     reference stores them in fp32, pseudo_context_cuda.cu:97-99).
 */
#ifndef PCONV_HIP_H
#define PCONV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCONV_OK 0
#define PCONV_EINVAL (-1)  /* bad argument / shape            */
#define PCONV_ELAUNCH (-2) /* hip launch or runtime error     */
#define PCONV_ENOMEM (-3)

const char *pconv_last_error(void);
int pconv_abi_version(void);
/* number of devices visible to the HIP runtime (0 if none) */
int pconv_device_count(void);

/* ------------------------------------------------------------------------
 * Host-side geometry (replaces math_cuda.cu:177-253 and the one-off table
 * kernels of sphere_slice / sphere_uslice / pseudo_context / entropy_context)
 * ---------------------------------------------------------------------- */

/* Valid width of every latitude tile at tensor width `width`.
 * replaces sphere_cal_npart_hw_v3 (math_cuda.cu:223-253) and the width half of
 * sphere_cal_npart_hw_v2 (math_cuda.cu:177-221).  widths[npart]. */
int pconv_host_tile_widths(const float *weight, int npart, int height, int width,
                           int32_t *widths);
/* The same for SphereSlice, by sphere_cal_npart_hw_v2's rule: the fixed widths apply from a weight total of
 * 3 * npart on, where the function above (_v3) switches only above it.  widths[npart]. */
int pconv_host_slice_widths(const float *weight, int npart, int height, int width,
                            int32_t *widths);

/* Catmull-Rom tap table of SphereSlice: for tile t, output column i < widths[t]
 * the first source column tap_col[t*width+i] and 4 coefficients.
 * replaces init_slice_param_kernel (sphere_slice_cuda.cu:13-32). */
int pconv_host_slice_taps(const int32_t *widths, int npart, int width,
                          int32_t *tap_col, float *tap_coef /* [npart*width*4] */);

/* Tap table of SphereUslice (up-resample from widths[t] to width).
 * replaces init_uslice_param_kernel (sphere_uslice_cuda.cu:13-30). */
int pconv_host_uslice_taps(const int32_t *widths, int npart, int width,
                           int32_t *tap_col, float *tap_coef);

/* Vertical-halo gather table of PseudoPad for tiles of `height` rows, `pad`
 * halo rows.  Entry e = ((t*2+side)*pad+r), side 0 = rows above, 1 = below.
 *   src_tile[e], src_row[e]      source tile / row inside that tile
 *   col[e*width+i], wgt[e*width+i]  first source column and its lerp weight
 * replaces pseudo_context_forward_kernel (pseudo_context_cuda.cu:51-104). */
int pconv_host_pad_table(const int32_t *widths, int npart, int height, int width, int pad,
                         int32_t *src_tile, int32_t *src_row, int32_t *col, float *wgt);

/* Wavefront schedule of the entropy model: positions (row*width+col) of the
 * npart stacked tiles sorted by plane row+col, valid columns only.
 * order[height*npart*width] (only plane_start[nplane] entries used),
 * plane_start[height*npart+width]  (nplane = height*npart+width-1, +1 end).
 * replaces entropy_context::reshape_hw (entropy_context_cuda.cu:13-45). */
int pconv_host_wavefront(const int32_t *widths, int npart, int height, int width,
                         int32_t *order, int32_t *plane_start);

/* Causal halo lists of the entropy model, one list per plane, deterministic
 * order.  Offsets are element offsets inside ONE image's channel-0 plane of the
 * padded tensor (npart, C, height+2*pad, width+2*pad), i.e. tile stride =
 * C*(height+2pad)*(width+2pad).
 *   entry k: dst[k], src0[k] (-1 = reads as zero), src1[k] (-2 = plain copy of
 *   src0), wgt[k], entry_plane[k];  plane_start[height*npart+width+pad] prefix
 *   offsets (nplane = height*npart+width+pad-1, +1 end).
 * Returns the number of entries, or <0.  Call with dst == NULL to size.
 * replaces entropy_context_kernel + step1/step2 + the CPU compaction
 * (entropy_context_cuda.cu:64-165,187-204). */
int pconv_host_causal_halo(const int32_t *widths, int npart, int channel, int height,
                           int width, int pad, int32_t *dst, int32_t *src0, int32_t *src1,
                           float *wgt, int32_t *entry_plane, int32_t *plane_start);

/* The same causal halo as a dense lookup table for kernels that compute halo
 * taps on the fly instead of reading stored ones: entry ((t*2+side)*pad+r)*width+i
 * = first source column (-1: only column 0 with weight 1-wgt; -2: no value, reads
 * as zero) and its weight. */
int pconv_host_causal_table(const int32_t *widths, int npart, int height, int width, int pad,
                            int32_t *col, float *wgt);

/* Viewport sampling table of MultiProject: tf[14*h_out*w_out*2] = (x, y) source
 * coordinates in an ERP of (height, width).
 * replaces projects_opt::init/update (projects_cuda.cu:7-165). */
int pconv_host_project_table(const float *theta, const float *phi, int nview, float fov,
                             int h_out, int w_out, int height, int width, float *tf);

/* ------------------------------------------------------------------------
 * Device kernels -- transform path
 * ---------------------------------------------------------------------- */

/* SphereSliceOp.forward  (sphere_slice_cuda.cu:87-146)
 * in (n, c, height, width) -> out (n*npart, c, height/npart + 2*pad, width + 2*pad);
 * only the interior is written when pad > 0, as in the reference. */
int pconv_sphere_slice(const float *in, float *out, const int32_t *widths,
                       const int32_t *tap_col, const float *tap_coef, int n, int c,
                       int height, int width, int npart, int pad, void *stream);

/* SphereUsliceOp.forward  (sphere_uslice_cuda.cu:73-126)
 * in (n*npart, c, h + 2*pad, width + 2*pad) -> out (n, c, h*npart, width) */
int pconv_sphere_uslice(const float *in, float *out, const int32_t *widths,
                        const int32_t *tap_col, const float *tap_coef, int n, int c, int h,
                        int width, int npart, int pad, void *stream);

/* PseudoPadOp.forward, the reference's three launches fused in one pass
 * (pseudo_pad.cu:39-125).  in (tn, c, h, w) -> out (tn, c, h+2p, w+2p). */
int pconv_pseudo_pad(const float *in, float *out, const int32_t *widths,
                     const int32_t *src_tile, const int32_t *src_row, const int32_t *col,
                     const float *wgt, int tn, int c, int h, int w, int pad, int npart,
                     void *stream);

/* The same when the producer has already written the tensor into the interior of
 * a padded buffer (pconv_conv2d / pconv_gdn with an output view): buf (tn, c,
 * h + 2*store, w + 2*store) holds the data at offset (store, store); only the ring
 * of the pad-p view (p <= store, origin (store - p, store - p)) is computed, in
 * place.  Tables as for pconv_pseudo_pad with the same pad. */
int pconv_pseudo_pad_ring(float *buf, const int32_t *widths, const int32_t *src_tile,
                          const int32_t *src_row, const int32_t *col, const float *wgt, int tn,
                          int c, int h, int w, int pad, int store, int npart, void *stream);

/* PseudoFillOp.forward, in place  (pseudo_fill_cuda.cu:28-62) */
int pconv_pseudo_fill(float *data, const int32_t *widths, int tn, int c, int h, int w,
                      int npart, int pad, int trim, float fvalue, void *stream);

/* DtowOp.forward  (dtow_cuda.cu:38-103); d2w != 0: (n,c,h,w)->(n,c/s^2,h*s,w*s) */
int pconv_dtow(const float *in, float *out, int n, int c, int h, int w, int stride, int d2w,
               void *stream);

/* PseudoQuantOp.forward (eval)  (pseudo_quant_cuda.cu:37-94,157-194)
 * weight (c, levels) raw parameter; level_tab (c, levels) scratch written here;
 * out_val / out_idx (idx as float, may be NULL); count (c, levels) histogram,
 * may be NULL. */
int pconv_quant(const float *x, const float *weight, float *level_tab, float *out_val,
                float *out_idx, float *count, const int32_t *widths, int tn, int c, int h,
                int w, int levels, int npart, void *stream);

/* ClipData.forward (model_zoo_v2.py:8-26), in place on n floats: x * 0.01 below 0, 1 + (x - 1) * 0.01 above 1,
 * x otherwise -- the same three roundings as the reference's masked assignments, in one pass. */
int pconv_leaky_clip(float *x, long long n, void *stream);

/* Frame I/O at the PCIe boundary: the device side of img2tensor / tensor2img (pseudo_codec.py:215-221).
 * u8_to_f32: in = n interleaved uint8 images (n, height, width, 3) ON THE DEVICE (copied there as they come from the
 * image file), out = float32 (n, 3, height, width) = float(u8) / 255.f, correctly rounded (the reference's numpy
 * float32 division).  f32_to_u8: out = (uint8)(int)(x * 255.f), numpy's float32 -> uint8 cast of tensor2img (truncation,
 * low byte kept).  width % 4 == 0; image 4-byte aligned, tensor 16-byte aligned. */
int pconv_frames_u8_to_f32(const uint8_t *in, float *out, int n, int height, int width, void *stream);
int pconv_frames_f32_to_u8(const float *in, uint8_t *out, int n, int height, int width, void *stream);

/* Panoramas of any size (csrc/erp_size.hip).  An h x w ERP frame (h, w >= 2) is coded at H = 256*ceil(h/256),
 * W = 16*ceil(w/16), padded by a pure gather: with top = (H - h) / 2 and m = (W - w + 1) / 2, coded pixel (y', x')
 * reads the image at
 *     y = y' - top; flip = 0;
 *     if (y < 0)       { y = -1 - y;        flip = 1; }   across the north pole
 *     else if (y >= h) { y = 2*h - 1 - y;   flip = 1; }   across the south pole
 *     y = clamp(y, 0, h - 1);                             only when the pad exceeds h
 *     x = x' < w ? x' : (x' - w < m ? w - 1 : 0);         seam: left half repeats column w-1, right half column 0
 *     if (flip) x = (x + w / 2) % w;                      half-turn of longitude across a pole
 * and the decoder crops rows top..top+h-1, columns 0..w-1.  A codable size (h % 256 == 0, w % 16 == 0) maps to
 * itself.  pconv_erp_coded_size is the single definition of (H, W, top): host only, 0 or PCONV_EINVAL (h or w
 * below 2 or above 2^20).  The three kernels take any width (w <= 21834) and any uint8 byte alignment:
 *   frames_u8_to_f32_erp: uint8 (n, h, w, 3) -> float32 (n, 3, H, W), float(u8) / 255.f as pconv_frames_u8_to_f32;
 *   erp_pad_f32:          float32 (n, 3, h, w) -> float32 (n, 3, H, W);
 *   frames_f32_to_u8_crop: float32 (n, 3, H, W) -> uint8 (n, h, w, 3), the crop with pconv_frames_f32_to_u8's cast.
 * Float tensors of the coded size 16-byte aligned; n <= 65535. */
int pconv_erp_coded_size(int h, int w, int *H, int *W, int *top);
int pconv_frames_u8_to_f32_erp(const uint8_t *in, float *out, int n, int h, int w, void *stream);
int pconv_erp_pad_f32(const float *in, float *out, int n, int h, int w, void *stream);
int pconv_frames_f32_to_u8_crop(const float *in, uint8_t *out, int n, int h, int w, void *stream);

/* YUV 4:2:0 frames (csrc/yuv.hip; pseudocylindrical_convolution_amd/yuv.py states the same definition in torch).
 * Formats.  A frame is one contiguous buffer, as a raw .yuv file holds it; h and w are even and at least 2:
 *   PCONV_YUV_420P      uint8.  Y (h, w), then U (h/2, w/2), then V (h/2, w/2).
 *   PCONV_YUV_NV12      uint8.  Y (h, w), then interleaved UV (h/2, w/2, 2).
 *   PCONV_YUV_420P10LE  uint16 (host little-endian).  The planes of 420P, values 0..1023; a sample above 1023 is
 *                       taken modulo 1024.
 * d is the bit depth (8 or 10), s = 2^(d-8).
 * Range.   PCONV_YUV_LIMITED: yo = 16s, ys = 219s, co = 128s, cs = 224s.
 *          PCONV_YUV_FULL:    yo = 0, ys = 2^d - 1, co = 2^(d-1), cs = 2^d - 1.
 * Matrix.  PCONV_YUV_BT709: Kr = 0.2126, Kb = 0.0722.  PCONV_YUV_BT601: Kr = 0.299, Kb = 0.114.  In double, in
 *          this order: Kg = 1.0 - Kr - Kb, a = 2*(1 - Kr), dd = 2*(1 - Kb), b = Kb*dd/Kg, c = Kr*a/Kg; each of Kr,
 *          Kg, Kb, a, b, c, dd is then rounded once to float32.
 * Chroma siting is H.26x type 0: a chroma sample is co-sited with the even luma columns and sits midway between
 * luma rows 2j and 2j+1.  The longitude seam wraps, the poles clamp.  All arithmetic is fp32, one rounding per
 * operation (no contraction), divisions correctly rounded.
 * Ingest (yuv420_to_f32): float32 RGB (n, 3, H, W) at the coded size of pconv_erp_coded_size(h, w).
 *   chroma up, vertical first:  luma row 2j   reads 0.25f*C[max(j-1, 0)] + 0.75f*C[j],
 *                               luma row 2j+1 reads 0.75f*C[j] + 0.25f*C[min(j+1, h/2-1)];
 *   then horizontal:            column 2i is V[i], column 2i+1 is 0.5f*(V[i] + V[(i+1) % (w/2)])
 *                               (for code values up to 1023 every intermediate is exact);
 *   normalise:  y = (Y - yo)/ys, cb = (Cb_up - co)/cs, cr = (Cr_up - co)/cs;
 *   matrix:     R = y + a*cr, G = (y - b*cb) - c*cr, B = y + dd*cb, each clamped to [0, 1];
 *   pad:        coded pixel (y', x') is the converted pixel at the source row and column of the pole / seam rule
 *               above (the rule's gather applied to converted pixels); a codable size maps to itself.
 * Egress (f32_to_yuv420): float32 RGB (n, 3, H, W) at the coded size -> the frame buffers of h x w.
 *   crop rows top..top+h-1, columns 0..w-1; clamp to [0, 1];
 *   y = (Kr*R + Kg*G) + Kb*B, cb = (B - y)/dd, cr = (R - y)/a;
 *   chroma down: v = 0.5f*(p[2j] + p[2j+1]) per column, then
 *                C[i] = (0.25f*v[(2i-1) mod w] + 0.5f*v[2i]) + 0.25f*v[2i+1]  (the seam wraps);
 *   quantise:    q = clamp(floorf((p*scale + offset) + 0.5f), 0, 2^d - 1), (ys, yo) for luma, (cs, co) for chroma.
 * Both refuse on the host, before any launch, with PCONV_EINVAL: null pointers, odd h or w or a side below 2,
 * w > PCONV_YUV_MAX_WIDTH (the row staging in LDS), n > 65535, unknown enums, a float tensor that is not 16-byte
 * aligned.  The sample buffers take any alignment their element size allows. */
#define PCONV_YUV_420P 0
#define PCONV_YUV_NV12 1
#define PCONV_YUV_420P10LE 2
#define PCONV_YUV_BT709 0
#define PCONV_YUV_BT601 1
#define PCONV_YUV_LIMITED 0
#define PCONV_YUV_FULL 1
#define PCONV_YUV_MAX_WIDTH 11520
int pconv_frames_yuv420_to_f32(const void *in, float *out, int n, int h, int w, int fmt, int matrix, int range,
                               void *stream);
int pconv_frames_f32_to_yuv420(const float *in, void *out, int n, int h, int w, int fmt, int matrix, int range,
                               void *stream);

/* Sphere-weighted quality of ERP frames (csrc/sphere_metrics.hip): WS-PSNR / WS-SSIM (Sun, Lu, Yu, IEEE SPL 2017).
 * x and y are n frames of h x w (h, w >= 1, any size, smaller than the SSIM window included):
 *   _f32: float32 (n, c, h, w), contiguous, 4-byte aligned, values as they are (nominally [0, 1], not clamped);
 *   _u8:  uint8 (n, h, w, 3) interleaved, c must be 3, each value read as float(u8) / 255.f like
 *         pconv_frames_u8_to_f32 (the same image gives the same bits in both forms).
 * Row j of h weighs w_j = cos(((j + 0.5)/h - 0.5)·pi) in double (weighting PCONV_WS_WEIGHT_SPHERE) or 1
 * (PCONV_WS_WEIGHT_UNIFORM: plain PSNR / SSIM over the ERP grid).  Per frame, with the sums over channels, rows
 * and columns in fp64 and N = c · w · Σ_j w_j:
 *   out[2f]     = Σ w_j·(x - y)² / N            the WS-MSE (difference and square in fp32); WS-PSNR = 10·log10(1/out)
 *   out[2f + 1] = Σ w_j·ssim_map / N            the WS-SSIM
 * ssim_map is pytorch_ssim's: 11-tap Gaussian (sigma 1.5) window g⊗g, zero padding of 5 on all four borders (the
 * seam is not wrapped), C1 = 0.01², C2 = 0.03², sigma² = blur(x²) - mu²; computed in fp32 with a separable filter.
 * workspace: device memory of pconv_ws_metrics_workspace_bytes(n, h, w) bytes (one fp64 pair per tile and frame),
 * 8-byte aligned; out: n x 2 doubles on the device.  The entry points allocate nothing.  No atomics: each frame's
 * partials are added in a fixed order, so a frame gives the same bits alone, inside any batch and on every run.
 * n <= 65535, h, w <= 2^20; PCONV_EINVAL otherwise (workspace_bytes: a negative value). */
#define PCONV_WS_WEIGHT_SPHERE 0
#define PCONV_WS_WEIGHT_UNIFORM 1
long long pconv_ws_metrics_workspace_bytes(int n, int h, int w);
int pconv_ws_metrics_f32(const float *x, const float *y, int n, int c, int h, int w, int weighting, void *workspace,
                         double *out, void *stream);
int pconv_ws_metrics_u8(const uint8_t *x, const uint8_t *y, int n, int c, int h, int w, int weighting,
                        void *workspace, double *out, void *stream);

/* Backward of the two sphere metrics (csrc/sphere_metrics.hip; sphere_metrics.backward_torch states the same in torch).
 * For one frame and channel of x (the other picture) and y (the picture that receives the gradient), with blur the
 * window g⊗g above (symmetric, and with its zero padding its own transpose on the h x w grid), per pixel:
 *   mux = blur(x)  muy = blur(y)  sx2 = blur(x·x) - mux²  sy2 = blur(y·y) - muy²  sxy = blur(x·y) - mux·muy
 *   A1 = 2·mux·muy + C1   A2 = 2·sxy + C2   B1 = mux² + muy² + C1   B2 = sx2 + sy2 + C2   D = B1·B2   S = A1·A2 / D
 *   b = -S / B2                                                  (dS/dblur(y²))
 *   c = 2·A1 / D                                                 (dS/dblur(xy))
 *   a = 2·mux·A2 / D - 2·muy·S / B1 - mux·c - 2·muy·b            (dS/dmuy, the sigma terms included)
 * gout holds the upstream gradients (gm of the frame's WS-MSE, gs of its WS-SSIM) as n fp64 pairs ON THE DEVICE:
 *   ks_j = gs·w_j / N   km_j = 2·gm·w_j / N   (N = c·w·Σ_j w_j, the sum j-ascending; fp64, rounded once to fp32)
 *   grad_y = blur(ks·a) + 2·y·blur(ks·b) + x·blur(ks·c) + km·(y - x)      (ks·a, ks·b, ks·c are zero outside the frame)
 * Both metrics are symmetric in their arguments: the gradient with respect to x is the same call with x and y swapped.
 * Arithmetic: fp32 without contraction apart from ks and km.  Every 11-tap sum runs k-ascending as
 * acc = fmaf(g[k], v, acc) from acc = 0, the horizontal pass before the vertical one; x·x, y·y and x·y are rounded
 * before they are filtered; a = (((2·mux)·A2 / D - (2·muy)·S / B1) - mux·c) - (2·muy)·b; the final sum is
 * ((blur(ks·a) + (2·y)·blur(ks·b)) + x·blur(ks·c)) + km·(y - x).  A pixel's result depends on nothing but its frame
 * and the frame's pair: the same bits alone, inside any batch and on every run.
 * One launch, a gather: every element of grad_y (float32 (n, c, h, w)) is stored exactly once.  No atomics, no
 * workspace, no allocation, no copy to or from the host.  Any h, w >= 1.  Refused on the host, before any launch,
 * with PCONV_EINVAL: null pointers, n, c, h or w outside pconv_ws_metrics_f32's ranges (n <= 65535, c <= 4096), an
 * unknown weighting, a plane of 2^31 bytes or more. */
int pconv_ws_metrics_backward_f32(const float *x, const float *y, const double *gout, int n, int c, int h, int w,
                                  int weighting, float *grad_y, void *stream);

/* WS-MS-SSIM of ERP frames, forward and backward (csrc/sphere_metrics.hip: the kernels of the entries above, launched
 * once per scale; sphere_metrics.ms_scales_torch and ms_backward_torch state the same in torch).  Frames as for
 * pconv_ws_metrics_f32 / _u8, with h >= 16 and w >= 16 (the fifth scale of a smaller frame would have no pixel).
 * x_0 = x, y_0 = y.
 * Pyramid.  Scale s = 0..4 has h_s = h >> s rows and w_s = w >> s columns;
 *   x_{s+1}[j][i] = ((x_s[2j][2i] + x_s[2j][2i+1]) + (x_s[2j+1][2i] + x_s[2j+1][2i+1])) · 0.25f   in fp32, in this order,
 * and y_{s+1} likewise.  An odd last row or column of a scale belongs to no 2x2 block and is dropped; it still counts in
 * that scale's own mean.
 * Per scale.  Window, zero padding of 5, C1, C2 and the moments are those of the WS-SSIM above, applied to (x_s, y_s) on
 * the h_s x w_s grid:  cs = (2·sxy + C2) / (sx2 + sy2 + C2),  l = (2·mux·muy + C1) / (mux² + muy² + C1).  The row weights
 * are those of an h_s-row frame, w_j = cos(((j + 0.5)/h_s - 0.5)·pi) or 1, and N_s = c · w_s · Σ_j w_j.  Every map is fp32,
 * every sum over pixels fp64:
 *   v_s = Σ w_j·cs / N_s  for s = 0..3,     v_4 = Σ w_j·(l·cs) / N_4  (the full SSIM map, evaluated as pconv_ws_metrics
 *   evaluates it: ((2·mux·muy + C1)·(2·sxy + C2)) / ((mux² + muy² + C1)·(sx2 + sy2 + C2))).
 * WS-MS-SSIM = Π_s max(v_s, 0)^β_s,  β = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) (Wang, Simoncelli, Bovik 2003), the
 * product in fp64 for s = 0..4 ascending.  Identical frames give 1; a frame with any v_s <= 0 gives 0.
 *   out[7f + s] = v_s (s = 0..4)   out[7f + 5] = WS-MSE, with the bits of pconv_ws_metrics   out[7f + 6] = WS-MS-SSIM
 * Forward: one launch per scale (one workgroup per 32 x 64 tile and frame, fp64 partials per tile, no atomics), each of
 * which also writes its tile's 16 x 32 block of the next scale from the tile it has staged, and one closing launch.
 * workspace: pconv_ws_msssim_workspace_bytes(n, c, h, w) bytes of device memory, 8-byte aligned: x_1, y_1, ..., x_4, y_4 as
 * float32 (n, c, h_s, w_s) each (one third of the two inputs), then the partials.  It is kept for the backward.
 * Gradient, with respect to y (x the other picture), gout = n fp64 pairs (gm of WS-MSE, gs of WS-MS-SSIM) and values = the
 * forward's out, both ON THE DEVICE:
 *   u_s = gs·β_s·MS / v_s when every v_t > 0, else u_s = 0 for all s (never a NaN or inf): fp64, on the device
 *   k_j = u_s·w_j / N_s   (fp64, rounded once to fp32; N_s with the sum j-ascending)
 *   own_s = (blur(k·a) + (2·y_s)·blur(k·b)) + x_s·blur(k·c)
 *   s = 4: a, b, c exactly those of pconv_ws_metrics_backward_f32, in the same operation order
 *   s < 4: B2 = sx2 + sy2 + C2,  S = A2 / B2,  b = -S / B2,  c = 2 / B2,  a = (-mux·c) - (2·muy)·b
 *   g_4 = own_4;  for s = 3..0:  g_s[r][q] = own_s[r][q] + 0.25f·g_{s+1}[r >> 1][q >> 1] where (r >> 1, q >> 1) lies
 *   inside scale s+1, else own_s[r][q];   grad_y = g_0 + km·(y - x),  km as in pconv_ws_metrics_backward_f32.
 * Rounding as there: 11-tap sums k-ascending with fmaf from 0, horizontal pass first, products rounded before they are
 * filtered, no contraction.  Everything is symmetric in x and y: the gradient of x is the same call with x and y
 * exchanged and swapped = 1, which says that the workspace was filled by the forward of (y, x).
 * Backward: one gather launch per scale, coarse to fine, every element stored once, no atomics.  backward_workspace:
 * pconv_ws_msssim_backward_workspace_bytes(n, c, h, w) bytes, 4-byte aligned: g_1..g_4 (one third of one input).
 * No entry point allocates, synchronises or copies to the host.  Refused on the host, before any launch, with
 * PCONV_EINVAL (the _bytes queries: a negative value): null or misaligned pointers, n, c, h, w or the weighting outside
 * pconv_ws_metrics_backward_f32's ranges, "h and w must be at least 16". */
long long pconv_ws_msssim_workspace_bytes(int n, int c, int h, int w);
int pconv_ws_msssim_f32(const float *x, const float *y, int n, int c, int h, int w, int weighting, void *workspace,
                        double *out, void *stream);
int pconv_ws_msssim_u8(const uint8_t *x, const uint8_t *y, int n, int c, int h, int w, int weighting, void *workspace,
                       double *out, void *stream);
long long pconv_ws_msssim_backward_workspace_bytes(int n, int c, int h, int w);
int pconv_ws_msssim_backward_f32(const float *x, const float *y, const void *workspace, const double *values,
                                 const double *gout, int n, int c, int h, int w, int weighting, int swapped,
                                 void *backward_workspace, float *grad_y, void *stream);

/* Sphere-aware resize of ERP frames (csrc/erp_resample.hip; pseudocylindrical_convolution_amd/erp_resample.py states
 * the same definition in torch).  Separable Lanczos-3 on float32 (n, C, h, w) -> (n, C, h2, w2); pixel centres sit at
 * (j + 1/2) / size on both grids; the kernel is stretched by max(1, in / out) when an axis shrinks.
 * Tap table of one axis, n_in -> n_out (pconv_host_lanczos_taps: host only, in double, the single source of the bits):
 *   D = 2 * max(n_in, n_out);  N(i, k) = 2*n_out*k - (2*i + 1)*n_in + n_out in exact 64-bit integers: source sample k
 *   lies N / D kernel units from output sample i.
 *   raw weight r = 1 if N == 0;  0 if N != 0 and D divides N (the exact zeros of sinc: equal sizes are a bit-exact
 *   identity);  otherwise, with x = pi * |N| / D,  r = 3 * sin(x) * sin(x / 3) / (x * x).
 *   The taps of output i are all k with |N| < 3*D; first[i] is the smallest (it may be negative or run past the
 *   axis).  Weights are divided by their sum (taken in ascending k, in double) and rounded once to float32.  T is
 *   the largest tap count over i (6 when enlarging, 12 at 2:1, at most 48 at 8:1); shorter rows are padded with
 *   +0.0f.  weights is (n_out, T) row-major.  The table repeats every n_out / gcd(n_in, n_out) outputs: first advances
 *   by n_in / gcd and the weights repeat bit for bit.  With first == weights == NULL only *taps is written.
 * Horizontal pass first:  mid[y][i] = sum_t wx[i][t] * x[y][(first_x[i] + t) mod w]  (the mathematical modulo: the
 *   seam wraps).
 * Vertical pass on mid:  source row r = first_y[j] + t goes through the pole rule of pconv_erp_coded_size:
 *   r < 0 -> -1 - r;  r >= h -> 2*h - 1 - r;  then clamp to [0, h - 1];  a row that crossed a pole is read at column
 *   (i + floor(w2 / 2)) mod w2, the half turn of longitude applied to the intermediate picture.
 * Rounding: both sums run t-ascending; every product and every addition is one fp32 rounding, never contracted; the
 *   first product starts the chain; mid is float32.  clamp != 0: the result is min(max(v, 0), 1) (Lanczos overshoots:
 *   a unit step gives -0.031 .. 1.031).  Non-finite inputs: unspecified.
 * pconv_erp_resample_f32: first_x / wx (w2 rows of tx) and first_y / wy (h2 rows of ty) are DEVICE copies of the
 *   tables; workspace is device memory of pconv_erp_resample_workspace_bytes(...) bytes (mid).  All tensors 4-byte
 *   aligned (16-byte alignment enables the wide accesses); no allocation, no atomics.  Refused on the host, before
 *   any launch, with PCONV_EINVAL: null pointers, a side outside 2 .. 2^20, n_in > 8 * n_out on an axis, n * C
 *   outside 1 .. 65535, tap counts that are not those of the two axes (workspace_bytes: a negative value). */
int pconv_host_lanczos_taps(int n_in, int n_out, int32_t *first, float *weights, int *taps);
long long pconv_erp_resample_workspace_bytes(int n, int c, int h, int w, int h2, int w2);
int pconv_erp_resample_f32(const float *in, float *out, void *workspace, const int32_t *first_x, const float *wx, int tx,
                           const int32_t *first_y, const float *wy, int ty, int n, int c, int h, int w, int h2, int w2,
                           int clamp, void *stream);

/* Ordered backward of the resize (csrc/erp_resample_backward.hip; erp_resample.py states the same definition in torch:
 * resize_backward_torch).  The forward, clamp aside, is mid[r][i] = sum_t wx[i][t] * x[r][(fx[i] + t) mod w] and
 * out[j][i] = sum_t wy[j][t] * mid[rho(fy[j] + t)][kappa], rho the pole rule followed by the clamp to [0, h - 1], kappa =
 * i, or (i + floor(w2 / 2)) mod w2 for a tap row that crossed a pole (judged before the clamp).  The backward is the
 * adjoint of that linear map, gx = Ax^T Ay^T g, in THIS ORDER:
 * Vertical adjoint, g (h2, w2) -> gmid (h, w2).  Destination gmid[r][c]: one fp32 accumulator.  Its terms: every table
 *   entry (j, t), 0 <= t < T_y, with rho(fy[j] + t) = r -- the padded entries of weight +0.0 included: the table is the
 *   data, not a tap count.  Term: wy[j][t] * g[j][i], i = c for an entry that did not cross a pole, i = (c - floor(w2 / 2))
 *   mod w2 for one that did.  Order: j ascending, then t ascending; taps of one j that the pole rule or the clamp sends to
 *   the same row are terms of their own.
 * Horizontal adjoint, gmid -> gx (h, w).  Destination gx[r][c]; its terms: every entry (i, t), 0 <= t < T_x, with
 *   (fx[i] + t) mod w = c (several t of one i coincide when w < T_x).  Term: wx[i][t] * gmid[r][i].  Order: i ascending,
 *   then t ascending.
 * Arithmetic, as in the forward: one __fmul_rn per term; the first product starts the chain; one __fadd_rn per further
 *   term, never contracted; a destination with no term gets +0; gmid is rounded to float32 between the passes, as mid
 *   is.  The clamp of the forward is the caller's: g is replaced by +0 where the unclamped value lay outside [0, 1]
 *   before it comes here (torch.clamp's gradient).  Nothing depends on the launch grid, the workgroup, the batch or the
 *   neighbours: one form, no float atomics.
 * pconv_host_lanczos_reverse_size(n_in, n_out): n_out * T, the number of list entries of one axis; negative for a side
 *   or a shrink pconv_host_lanczos_taps refuses.
 * pconv_host_lanczos_reverse (host): the transposed table of one axis as CSR per source index, built from the very table
 *   pconv_host_lanczos_taps returns: rev_start n_in + 1 int32, rev_entry n_out * T int32, entry e = i * T + t (so that
 *   its weight is weights[e]), ascending within each list: a stable counting sort of the forward walk (i ascending, then
 *   t) by destination, (first[i] + t) mod n_in for pole == 0, rho for pole != 0; crossed: n_out * T bytes, 1 where the
 *   entry crossed a pole, written for pole != 0 only (it may be NULL otherwise).  Returns the entry count.  Refused,
 *   before anything is written: null pointers, a side outside 2 .. 2^20, n_in > 8 * n_out.
 * pconv_erp_resample_backward_f32: gout (n, C, h2, w2) -> gin (n, C, h, w); wx / wy are the DEVICE copies of the
 *   forward's weight tables, the lists device copies of pconv_host_lanczos_reverse(w, w2, 0) and (h, h2, 1); workspace
 *   is device memory of pconv_erp_resample_backward_workspace_bytes(...) bytes (gmid).  Two gathers of 256 lanes; a list
 *   is never split across lanes; plain vector stores, 64-bit flat indices, no atomics, no allocation, no memset.  All
 *   tensors 4-byte aligned (16-byte alignment enables the wide accesses).  An entry outside 0 .. n_out*T - 1 is skipped
 *   and a start outside it clamped, so no list content makes a kernel read outside its buffers.  Refused on the host,
 *   before any launch, with PCONV_EINVAL: what pconv_erp_resample_f32 refuses, null list pointers, gin == gout, tap
 *   counts that are not the tables', and an enlargement so large (beyond about 15:1 in width) that the gradient columns
 *   one tile of 1024 source columns gathers from exceed 64 KiB of LDS. */
long long pconv_host_lanczos_reverse_size(int n_in, int n_out);
int pconv_host_lanczos_reverse(int n_in, int n_out, int pole, int32_t *rev_start, int32_t *rev_entry, uint8_t *crossed);
long long pconv_erp_resample_backward_workspace_bytes(int n, int c, int h, int w, int h2, int w2);
int pconv_erp_resample_backward_f32(const float *gout, float *gin, void *workspace, const float *wx, int tx,
                                    const int32_t *rev_start_x, const int32_t *rev_entry_x, const float *wy, int ty,
                                    const int32_t *rev_start_y, const int32_t *rev_entry_y, const uint8_t *rev_crossed_y,
                                    int n, int c, int h, int w, int h2, int w2, void *stream);

/* Sphere rotation of ERP frames (csrc/erp_rotate.hip; pseudocylindrical_convolution_amd/erp_rotate.py states the same
 * definition in torch and numpy): float32 (n, C, h, w) -> (n, C, h, w), the picture of the same sphere in a rotated
 * orientation.  A map says where on the source each output pixel lies; a sampler reads the source there.
 * Angles (the units and ranges of the sphere-rotation SEI of HEVC / VVC): int32 in units of 2^-16 degree,
 *   yaw in [-180*2^16, 180*2^16 - 1], pitch in [-90*2^16, 90*2^16], roll in [-180*2^16, 180*2^16 - 1].
 * Directions: pixel (row j, column i) of an h x w frame has longitude t = ((i + 1/2)/w - 1/2)*2*pi and latitude
 *   p = (1/2 - (j + 1/2)/h)*pi; its direction is d = (cos p cos t, cos p sin t, sin p).
 * Matrix (pconv_host_erp_rotation_matrix: host, in double, row-major m[9]): M = Rz(yaw) * Ry(-pitch) * Rx(roll), the
 *   right-handed axis rotations Rz(a) = [c -s 0; s c 0; 0 0 1], Ry(a) = [c 0 s; 0 1 0; -s 0 c], Rx(a) = [1 0 0; 0 c -s;
 *   0 s c].  Output pixel d reads the source at s = M * d: the source point at longitude yaw, latitude pitch lands in
 *   the centre of the rotated picture and roll turns the picture about that centre.  inverse != 0 gives the transpose
 *   of M, entry for entry: the way back.
 * Source coordinates, all in fp64:  u = (atan2(s_y, s_x)/(2*pi) + 1/2)*w - 1/2,
 *   v = (1/2 - atan2(s_z, hypot(s_x, s_y))/pi)*h - 1/2.
 * Map record (pconv_erp_rotation_map: (h, w, 2) int32 on the device), P = PCONV_ERP_ROTATE_PHASES = 256 phases per pixel:
 *   map[j][i][0] = qu = rint(u*P) reduced modulo w*P (the mathematical modulo, 0 <= qu < w*P);  map[j][i][1] = qv =
 *   rint(v*P) (it may be negative).  rint rounds halves to even.  Column and phase: floor(qu / P), qu mod P; row and
 *   phase: floor(qv / P), qv mod P (floor division, the phase never negative).  A position is thus quantised to 1/256
 *   pixel.  The trigonometry runs in fp64 on the device: the map equals a float64 evaluation on the host except where
 *   u*P or v*P lies within the evaluation error (about 1e-10) of a rounding boundary.
 * Phase table (pconv_host_lanczos_phases: host, in double; weights is P rows of PCONV_ERP_ROTATE_TAPS = 6 floats): row p,
 *   f = p / P, weighs the source samples base - 2 .. base + 3 with L(f - k), k = -2 .. 3, L(x) = 3 sin(pi x) sin(pi x/3)
 *   / (pi x)^2, L(0) = 1; each row is divided by its sum (ascending k, in double) and rounded once to float32.  Row 0 is
 *   exactly (0, 0, 1, 0, 0, 0): the zeros of L at the integers are set, not evaluated.
 * Sampler (pconv_erp_remap_f32), with (column, fx) and (row, fy) of the pixel's record, wx = row fx and wy = row fy of
 *   the table:  tap row r_a = row - 2 + a goes through the pole rule of pconv_erp_coded_size: r < 0 -> -1 - r;
 *   r >= h -> 2*h - 1 - r; then clamp to [0, h - 1].  Tap column c_b = (column - 2 + b) mod w; in a tap row that
 *   crossed a pole, (c_b + floor(w / 2)) mod w.
 *   out = sum_a wy[a] * (sum_b wx[b] * x[r_a][c_b]): both sums ascending, every product and every addition one fp32
 *   rounding, never contracted; the first product starts each chain; the inner sum of a row is finished before the
 *   outer sum takes it.  clamp != 0: min(max(v, 0), 1).  Non-finite inputs: unspecified.  The sampler reduces whatever
 *   the map holds to a position inside the frame (columns modulo w, rows by the pole rule), so no map content makes it
 *   read outside `in`.
 * pconv_erp_remap_f32: in / out (n, C, h, w), distinct; map (h, w, 2) int32 and phases (P x 6 float32) on the device.
 *   Tensors 4-byte aligned, the map 8-byte aligned; no allocation, no atomics, no workspace.  Refused on the host, before
 *   any launch, with PCONV_EINVAL: null pointers, a side outside 2 .. 2^20, a plane of 2^31 bytes or more, n * C
 *   outside 1 .. 65535, angles out of range, misaligned tensors, in == out. */
#define PCONV_ERP_ROTATE_PHASES 256
#define PCONV_ERP_ROTATE_TAPS 6
int pconv_host_erp_rotation_matrix(int yaw, int pitch, int roll, int inverse, double *m);
int pconv_host_lanczos_phases(float *weights);
int pconv_erp_rotation_map(int32_t *map, int h, int w, int yaw, int pitch, int roll, int inverse, void *stream);
int pconv_erp_remap_f32(const float *in, float *out, const int32_t *map, const float *phases, int n, int c, int h, int w,
                        int clamp, void *stream);

/* Rectilinear viewports of ERP frames (csrc/viewport.hip; pseudocylindrical_convolution_amd/viewport.py states the same
 * definition in torch and numpy): float32 (n, C, h, w) -> n frames of (C, vh, vw), what a pinhole camera at the centre
 * of the sphere sees.  A map says where on the source each sample of the view lies; a renderer reads the source there
 * and averages ss x ss samples per pixel.
 * View: five int32 in units of 2^-16 degree.  yaw, pitch, roll: the meaning and ranges of the sphere rotation above;
 *   hfov, vfov (the full horizontal and vertical field of view) in [1*2^16, 170*2^16].
 *   M = pconv_host_erp_rotation_matrix(yaw, pitch, roll, 0).  pconv_host_viewport_basis (host, in double) returns
 *   out[0..8] = M row-major, out[9] = tan(hfov/2), out[10] = tan(vfov/2), the angles as k * (pi / 180 / 65536) / 2.
 * Grid: a view of vh x vw pixels with supersampling ss in {1, 2, 3, 4} has gh = vh*ss rows and gw = vw*ss columns of
 *   samples.  Sample (row r, column q) looks along d = (1, a, b), all in fp64:
 *   a = (2*(q + 1/2)/gw - 1) * tan(hfov/2),  b = (1 - 2*(r + 1/2)/gh) * tan(vfov/2):  right is +y and up is +z, the
 *   picture centre is direction (1, 0, 0), as in the ERP convention above.  It reads the source at s = M * d (not
 *   normalised: u and v below depend on the direction alone).
 * Map record (pconv_viewport_map: (gh, gw, 2) int32 on the device): u, v and (qu, qv) are those of pconv_erp_rotation_map
 *   for the source size h x w: u = (atan2(s_y, s_x)/(2*pi) + 1/2)*w - 1/2, v = (1/2 - atan2(s_z, hypot(s_x, s_y))/pi)*h
 *   - 1/2, qu = rint(u*P) reduced modulo w*P, qv = rint(v*P), P = 256, rint rounds halves to even.
 * Sample: the sampler of pconv_erp_remap_f32, word for word: 6 x 6 Lanczos-3 from the phase table of
 *   pconv_host_lanczos_phases, columns wrapped, rows by the pole rule with the half turn, both sums ascending, one fp32
 *   rounding per product and per addition, never contracted.
 * Pixel (j, i): the sum of its ss*ss samples (j*ss + p, i*ss + t) in the order p outer, t inner, in fp32 additions, the
 *   first sample starting the chain; then one fp32 multiplication by (float)(1.0 / (ss*ss)), skipped for ss = 1; then,
 *   with clamp != 0, min(max(v, 0), 1).  A box average over the pixel: no wider reconstruction filter.
 * pconv_viewport_render_f32: in (n, C, h, w); out holds n frames of (C, vh, vw), out_frame_stride floats apart (at least
 *   C*vh*vw: one view can be written into slot k of an (n, V, C, vh, vw) tensor); map (vh*ss, vw*ss, 2) int32 and phases
 *   (P x 6 float32) on the device.  Every record is reduced to a position inside the frame, so no map content makes the
 *   renderer read outside `in`; each lane stores only its own pixel.  Tensors 4-byte aligned, the map 8-byte aligned; no
 *   allocation, no atomics, no workspace.  Refused on the host, before any launch, with PCONV_EINVAL: null pointers or
 *   misalignment, a source or view side outside 2 .. 2^20, a source plane, a map or an output frame of 2^31 bytes or
 *   more, ss outside 1 .. 4, n * C outside 1 .. 65535, a stride below C*vh*vw, in == out, angles out of range. */
#define PCONV_VIEWPORT_MAX_SS 4
int pconv_host_viewport_basis(int yaw, int pitch, int roll, int hfov, int vfov, double *out);
int pconv_viewport_map(int32_t *map, int h, int w, int gh, int gw, int yaw, int pitch, int roll, int hfov, int vfov,
                       void *stream);
int pconv_viewport_render_f32(const float *in, float *out, const int32_t *map, const float *phases, int n, int c, int h,
                              int w, int vh, int vw, int ss, long long out_frame_stride, int clamp, void *stream);

/* Cubemap panoramas, CMP and EAC (csrc/cube.hip; pseudocylindrical_convolution_amd/cube.py states the same definition in
 * torch and numpy).  A cube conversion is two maps for pconv_viewport_render_f32 and one kernel that continues a face
 * across its edges; the sampler is the one above, word for word.
 * Axes: those of the sphere rotation: the picture centre is (1, 0, 0), right is +y, up is +z.
 * Faces, in this order, each with forward, right and up:
 *     index  face  forward      right        up
 *     0      F     ( 1, 0, 0)   ( 0, 1, 0)   ( 0, 0, 1)
 *     1      R     ( 0, 1, 0)   (-1, 0, 0)   ( 0, 0, 1)
 *     2      B     (-1, 0, 0)   ( 0,-1, 0)   ( 0, 0, 1)
 *     3      L     ( 0,-1, 0)   ( 1, 0, 0)   ( 0, 0, 1)
 *     4      U     ( 0, 0, 1)   ( 0, 1, 0)   (-1, 0, 0)
 *     5      D     ( 0, 0,-1)   ( 0, 1, 0)   ( 1, 0, 0)
 *   F, R, B, L: up = +z, right = the forward of the next face in yaw order.  U and D: the edge shared with F is U's
 *   bottom edge and D's top edge.  right x up = forward on every face.
 * Face coordinates of a face of a x a pixels: s, t in [-1, 1], at the centre of pixel (row r, column c)
 *   s = 2*(c + 1/2)/a - 1,  t = 1 - 2*(r + 1/2)/a.  Plane coordinates: PCONV_CUBE_CMP p = s;  PCONV_CUBE_EAC
 *   p = tan(pi/4 * s), inverse s = (4/pi)*atan(p).  Direction d = forward + p_s*right + p_t*up, all in fp64.
 * Face of a direction (x, y, z): the axis of largest magnitude; ties in the order x, y, z:
 *   |x| >= |y| and |x| >= |z| -> x >= 0 ? F : B;  else |y| >= |z| -> y >= 0 ? R : L;  else z >= 0 ? U : D
 *   (pconv_host_cube_face_of: the rule on the host).  A tie is the one place where host and device could disagree by a
 *   whole face: a direction within rounding of an edge or corner of the cube may land on either side.
 *   Position on face g: p_s = (d . right_g)/(d . forward_g), p_t = (d . up_g)/(d . forward_g), s and t through the
 *   inverse above, u' = (s + 1)*a/2 - 1/2, v' = (1 - t)*a/2 - 1/2 (pixels; the centre of pixel (r, c) is (c, r)).
 * The canonical picture is the face stack (n, C, 6*a, a), face f in rows f*a .. f*a + a - 1.  Other layouts are index
 *   permutations made above this interface.  a in 2 .. PCONV_CUBE_MAX_FACE, the largest a whose padded stack (below)
 *   stays under 2^31 bytes.
 * ERP -> cube.  pconv_cube_from_erp_map: map (6*a*ss, a*ss, 2) int32 on the device.  With gs = a*ss, sample (row R, column
 *   Q) belongs to face R / gs; its face coordinates are those of the sample grid of that face, as in pconv_viewport_map:
 *   s = 2*(Q + 1/2)/gs - 1, t = 1 - 2*((R mod gs) + 1/2)/gs.  The record is that of pconv_erp_rotation_map for the
 *   direction d and the source size h x w.  The picture is pconv_viewport_render_f32 on that map: source h x w, "view"
 *   6*a x a, ss in 1 .. 4; an ss x ss block never leaves its face.
 * Cube -> ERP.  A face is first continued by PCONV_CUBE_PAD = 3 pixels on every side (the footprint reaches 2 pixels
 *   before and 3 after its centre tap), A = a + 6.
 *   pconv_cube_pad_f32: in (n, C, 6*a, a) -> out (n, C, 6*A, A), distinct.  Interior: out[f*A + 3 + r][3 + c] =
 *   in[f*a + r][c], a copy.  Ring pixel (face f, padded row R, padded column Q, r = R - 3 or c = Q - 3 outside 0 .. a-1):
 *   its value is the bilinear read of face g at (qu, qv) in 1/256 pixel, (g, qu, qv) its record in `table`:
 *     x0 = qu >> 8, fx = (float)(qu & 255)/256, x1 = min(x0 + 1, a - 1); y0, fy, y1 from qv alike;
 *     top = x[y0][x0] + fx*(x[y0][x1] - x[y0][x0]);  bot = x[y1][x0] + fx*(x[y1][x1] - x[y1][x0]);
 *     out = top + fy*(bot - top);  every subtraction, product and addition one fp32 rounding, never contracted.
 *   That form returns the constant for a constant face.  One level deep: the ring reads original faces only.
 *   table: int32 (6*(A*A - a*a), 3) on the device, face after face, within a face in ring order: the pixels of the padded
 *   face outside its interior, row after row, column after column (12*a + 36 per face).  It is built on the host in
 *   float64 (cube.pad_table): ring pixel (R, Q) lies on f's extended plane at the s, t of its centre by the same
 *   formulas, |s| or |t| > 1, EAC through tan as well (|s| and |t| held at 7/4 there, before the plane's horizon at 2:
 *   only faces of a <= 6 reach it); its direction falls on face g; u', v' there are
 *   clamped to [0, a - 1] and quantised, qu = rint(u'*256), halves to even.  The corners follow the same rule.  The kernel
 *   reduces whatever the table holds to a face 0 .. 5 and a position inside it, so no table content makes it read
 *   outside `in`.
 *   pconv_cube_to_erp_map: map (h*ss, w*ss, 2) int32 on the device.  Sample (row j, column i) of the gh x gw = h*ss x w*ss
 *   grid has the direction of pixel (j, i) of a gh x gw ERP frame (the sphere rotation above); that gives face g and u', v',
 *   clamped to [-1/2, a - 1/2].  The record addresses the padded stack seen as one plane of 6*A x A:
 *     qu = rint((u' + 3)*256),  qv = rint((v' + 3 + g*A)*256).
 *   Every footprint then stays inside its own padded face; the sampler's wrap and pole rule never fire, but still
 *   guarantee that no record reads outside the plane.  The picture is pconv_viewport_render_f32 with the padded stack
 *   as the source (6*A x A) and the ERP frame as the view.
 * Both maps run their trigonometry in fp64 on the device: they equal a float64 evaluation on the host except where
 *   u*256 or v*256 lies within the evaluation error of a rounding boundary, or a direction within it of a face tie.
 * Tensors and the table 4-byte aligned, maps 8-byte aligned; no allocation, no atomics, no workspace.  Refused on the host,
 *   before any launch, with PCONV_EINVAL: null or misaligned pointers, a kind outside {CMP, EAC}, a outside
 *   2 .. PCONV_CUBE_MAX_FACE, an ERP side outside 2 .. 2^20 or an ERP plane or a map of 2^31 bytes or more, n * C outside
 *   1 .. 65535, ss outside 1 .. 4, in == out.
 * A continuation of any depth.  pconv_cube_pad_depth_f32 is pconv_cube_pad_f32 with `depth` in 1 .. PCONV_CUBE_MAX_DEPTH
 *   in the place of 3: A = a + 2*depth, the interior at rows and columns depth .. depth + a - 1 of every padded face, the
 *   table int32 (6*(A*A - a*a), 3) in the same ring order (4*depth*(a + depth) pixels per face), built by the same rule
 *   (cube.pad_table(kind, a, depth)).  The bilinear read and the reduction of every record to a face and a position
 *   inside it are word for word those above, so depth = 3 gives the bits of pconv_cube_pad_f32 on the same table.  One
 *   level deep at every depth: the ring reads original faces only, and for EAC |s| and |t| of a ring pixel are still held
 *   at 7/4; the outermost ring pixel lies at 1 + (2*depth - 1)/a, beyond 7/4 for a < 4*(2*depth - 1)/3 (depth 3: a <= 6;
 *   depth 5: a <= 11).  cube.ws_ssim uses depth 5, the radius of the SSIM window.  Refused besides the above: a depth
 *   outside 1 .. PCONV_CUBE_MAX_DEPTH, and an a whose padded stack 24*A*A would reach 2^31 bytes. */
#define PCONV_CUBE_CMP 1
#define PCONV_CUBE_EAC 2
#define PCONV_CUBE_PAD 3
#define PCONV_CUBE_MAX_DEPTH 8
#define PCONV_CUBE_MAX_FACE 9453
int pconv_host_cube_face_of(double x, double y, double z);
int pconv_cube_from_erp_map(int32_t *map, int kind, int a, int ss, int h, int w, void *stream);
int pconv_cube_pad_f32(const float *in, float *out, const int32_t *table, int n, int c, int a, void *stream);
int pconv_cube_pad_depth_f32(const float *in, float *out, const int32_t *table, int n, int c, int a, int depth, void *stream);
int pconv_cube_to_erp_map(int32_t *map, int kind, int a, int h, int w, int ss, void *stream);

/* Ordered backward of the face continuation (csrc/cube.hip; cube.pad_backward_torch states the same definition in torch).
 * The forward above, as a function of real numbers, copies every interior pixel and writes ring pixel i (row i of the
 * table: face after face, in ring order) as a convex combination of four pixels of face g: with px = qu & 255, py = qv & 255
 *   (y0, x0) weighs (256 - px)*(256 - py)/65536,  (y0, x1) px*(256 - py)/65536,
 *   (y1, x0) (256 - px)*py/65536,                 (y1, x1) px*py/65536,
 * g, x0, x1, y0, y1 reduced and clamped exactly as the forward does it.  The backward is the adjoint of that linear map,
 * gin = A^T gout, gout (n, C, 6*A, A) -> gin (n, C, 6*a, a), in THIS ORDER:
 * Destination: pixel (face f, row r, column c) of plane (n, c): one fp32 accumulator that starts from the gradient of the
 *   pixel's own interior copy, gout[f*A + depth + r][depth + c].
 * Entry e = 4*i + corner: ring pixel i, corner 0 .. 3 = (y0, x0), (y0, x1), (y1, x0), (y1, x1).
 * Term: cx = (corner & 1) ? px : 256 - px;  cy = (corner & 2) ? py : 256 - py;  coef = (float)(cx*cy) * 2^-16, exact in
 *   fp32 since cx*cy <= 2^16;  term = __fmul_rn(g_ring, coef), g_ring the value of gout at ring pixel i;  then one
 *   __fadd_rn into the accumulator.  Never contracted.
 * Order of the terms of a destination: e ascending.  Where x1 == x0 or y1 == y0 (the clamp at a - 1) the corners that
 *   coincide stay entries of their own, added one after the other; a corner whose coefficient is 0 stays an entry too.  A
 *   destination no ring reads (most of a face) is the copy alone.  Nothing depends on the launch grid or the batch.
 * pconv_host_cube_pad_reverse_size(a, depth) = 24*(A*A - a*a), four entries per ring pixel of six faces; with 24*A*A below
 *   2^31 (the padded stack's own bound) this always fits int32.  A negative value when a or depth is refused.
 * pconv_host_cube_pad_reverse (host): the lists as CSR per pixel of the face stack from a host copy of the table the forward
 *   reads: rev_start 6*a*a + 1 int32, rev_entry 24*(A*A - a*a) int32, ascending within each list (a stable counting sort of
 *   the walk i ascending, corner ascending).  Returns the entry count; nothing is written unless every argument passes.
 * pconv_cube_pad_backward_f32: gout, gin, table and the two lists on the device, 4-byte aligned.  A gather: a lane owns one
 *   destination and walks its list once, for up to four planes at a time (the decoding of an entry is shared by the planes,
 *   the sums are not); a list is never split.  Every element of gin is stored exactly once.  No atomics, no workspace, no
 *   allocation.  An entry outside 0 .. 24*(A*A - a*a) - 1 is skipped and a start outside it clamped, and the ring pixel of
 *   an entry is always a pixel of the padded stack, so no list or table content makes the kernel read outside `table` or
 *   `gout`; each lane stores only its own pixel.  Refused on the host, before any launch, with PCONV_EINVAL: what
 *   pconv_cube_pad_depth_f32 refuses, null list pointers, gin == gout. */
long long pconv_host_cube_pad_reverse_size(int a, int depth);
int pconv_host_cube_pad_reverse(const int32_t *table, int a, int depth, int32_t *rev_start, int32_t *rev_entry);
int pconv_cube_pad_backward_f32(const float *gout, float *gin, const int32_t *table, const int32_t *rev_start,
                                const int32_t *rev_entry, int n, int c, int a, int depth, void *stream);

/* Sphere-sampled metrics: S-PSNR-NN, S-PSNR-I, CPP-PSNR (csrc/sphere_points.hip; pseudocylindrical_convolution_amd/
 * sphere_points.py states the same definition in torch and numpy).  Two ERP pictures of ANY two sizes are read at the
 * same points of the sphere and the squared error is summed over the points; neither picture is resampled onto the
 * other's grid.  The point sets (an icosphere, the pixels of a Craster parabolic picture, a file) are built on the host
 * by sphere_points.py; 360Lib's own point file is not part of this project, so equality of the figures with 360Lib's is
 * not claimed.
 * Point: a direction given as two doubles, longitude t in [-pi, pi] and latitude p in [-pi/2, pi/2], in the ERP
 *   convention of the sphere rotation above.  A point set is float64 (P, 2) of (t, p) in a fixed order, 1 <= P < 2^28.
 * Record of a point for a picture of h x w (pconv_sphere_points_records: (P, 2) int32 on the device), all in fp64, in
 *   THIS ORDER, every operation one rounding, never contracted, no transcendental:
 *     u = ((t / TWO_PI) + 0.5) * w - 0.5        TWO_PI = 6.283185307179586 (the double nearest 2*pi)
 *     v = (0.5 - (p / PI)) * h - 0.5            PI = 3.141592653589793
 *     qu = rint(u * 256) reduced modulo w * 256 (the mathematical modulo, 0 <= qu < w * 256);  qv = rint(v * 256)
 *   rint rounds halves to even.  These are the records of pconv_erp_rotation_map without the trigonometry, so the
 *   kernel and a float64 evaluation on the host in the same order give EQUAL records, with no exception near a rounding
 *   boundary.  A position is quantised to 1/256 pixel BEFORE the nearest / Lanczos choice below.
 * Sample, mode PCONV_SPHERE_POINTS_LANCZOS (S-PSNR-I, CPP-PSNR): the sampler of pconv_erp_remap_f32, word for word, at
 *   the record: 6 x 6 Lanczos-3 from the phase table of pconv_host_lanczos_phases, columns wrapped, rows by the pole rule
 *   with the half turn and then clamped, both sums ascending, one fp32 rounding per product and per addition, never
 *   contracted, no clamp of the value.  This is this project's interpolator, not 360Lib's.
 * Sample, mode PCONV_SPHERE_POINTS_NEAREST (S-PSNR-NN): column = floor((qu + 128) / 256) mod w; row = floor((qv + 128)
 *   / 256), then through the pole rule (r < 0 -> -1 - r; r >= h -> 2*h - 1 - r); a row that crossed a pole takes
 *   (column + floor(w / 2)) mod w; then the row is clamped to [0, h - 1].  The value is the pixel itself, no arithmetic.
 * pconv_sphere_points_sample_f32: in (n, C, h, w) -> out (n, C, P), out[f][c][k] the sample of plane (f, c) at record
 *   k.  It reads a panorama at arbitrary directions and is public in its own right.
 * Error of a point (pconv_sphere_points_mse_f32), a the sample of picture x (h1 x w1) at rec_x[k], b the sample of
 *   picture y (h2 x w2) at rec_y[k]:  d = a - b in fp32;  e_k = d * d in fp32, widened to double.
 * Sum, per plane (f, c), in fp64, in THIS ORDER, which depends on P alone (not on the batch, the grid or the device):
 *   chunks of PCONV_SPHERE_POINTS_CHUNK = 1024 consecutive points, chunk q = points 1024*q .. 1024*q + 1023 (the last
 *   one partial).  Lane l of 256 starts at +0 and adds e of the points l, l + 256, l + 512, l + 768 of its chunk that
 *   exist, ascending.  Tree: for s = 128, 64, 32, 16, 8, 4, 2, 1: lane l < s takes lane[l] + lane[l + s].  Lane 0 holds
 *   the chunk's partial, stored in the workspace (one double per plane and chunk).  A second launch sums a plane's
 *   partials the same way: lane l of 256 starts at +0 and adds the partials l, l + 256, l + 512, ... ascending, then
 *   the same tree; out[f][c] = SSE / P.  No atomics, no allocation; nothing of size P * n * C is written.
 *   A figure is 10 * log10(1 / mean over the channels of out[f]); RGB channels are thus averaged where 360Lib reports Y,
 *   U and V, and out keeps the per-channel values for a caller with planar data.
 * Tensors 4-byte aligned; points, records, workspace and out 8-byte aligned; phases (256 x 6 float32) on the device in
 *   both modes.  Every record is reduced to a position inside its frame, so no record content makes a kernel read outside
 *   a picture.  Refused on the host, before any launch, with PCONV_EINVAL (workspace_bytes: a negative value): null or
 *   misaligned pointers, a side outside 2 .. 2^20, a plane of 2^31 bytes or more, n * C outside 1 .. 65535, P outside
 *   1 .. 2^28 - 1, an unknown mode, in == out (sample), out or the workspace inside x or y (mse).  x == y is allowed. */
#define PCONV_SPHERE_POINTS_LANCZOS 0
#define PCONV_SPHERE_POINTS_NEAREST 1
#define PCONV_SPHERE_POINTS_CHUNK 1024
int pconv_sphere_points_records(const double *points, int32_t *records, long long P, int h, int w, void *stream);
int pconv_sphere_points_sample_f32(const float *in, float *out, const int32_t *records, const float *phases, int n, int c,
                                   int h, int w, long long P, int mode, void *stream);
long long pconv_sphere_points_mse_workspace_bytes(int n, int c, long long P);
int pconv_sphere_points_mse_f32(const float *x, int h1, int w1, const int32_t *rec_x, const float *y, int h2, int w2,
                                const int32_t *rec_y, const float *phases, int n, int c, long long P, int mode,
                                void *workspace, double *out, void *stream);

/* Points of the sphere on a cube picture (csrc/cube.hip; cube.point_records_numpy states the same definition in numpy):
 * the record that lets pconv_sphere_points_sample_f32 / pconv_sphere_points_mse_f32 read a cube picture, on either side,
 * with no conversion to ERP in between.  The picture they are given is the padded stack of pconv_cube_pad_f32, seen as
 * one plane of 6*A x A, A = a + 6.
 * dirs: float64 (P, 3) on the device, d = (cos p * cos t, cos p * sin t, sin p) of the point (t, p), built on the host:
 *   kernel and host twin read the same array, so no device trigonometry enters for CMP.
 * Record of a point (pconv_cube_points_records: (P, 2) int32 on the device), all in fp64, in THIS ORDER, every operation one
 *   rounding, never contracted:
 *     g = the face of d by the rule above (ties x, y, z with >=);
 *     along = d . forward_g;  ps = (d . right_g) / along;  pt = (d . up_g) / along   (the dot products have two zero terms);
 *     s = ps for CMP, (4/pi) * atan(ps) for EAC;  t from pt alike;
 *     u' = ((s + 1) * a) / 2 - 0.5;  v' = ((1 - t) * a) / 2 - 0.5;  both clamped to [-0.5, a - 0.5 - 1/256];
 *     qu = rint((u' + 3) * 256);  qv = rint((v' + 3 + g*A) * 256).
 *   The upper clamp is 1/256 tighter than pconv_cube_to_erp_map's, so that one record serves both modes: the nearest rule
 *   (floor((q + 128) / 256)) always lands on a pixel of face g itself, never on its ring, and the Lanczos footprint stays
 *   inside g's own padded face.  CMP records equal the host twin's with no exception; EAC records are equal except where
 *   u'*256 or v'*256 lies within the evaluation error of atan (about 1e-10) of a rounding boundary; a direction within
 *   rounding of a face tie lands on the same face on both sides, since both read the same doubles.
 * dirs and records 8-byte aligned; no allocation, no atomics, no workspace, one store per point.  Refused on the host, before
 *   any launch, with PCONV_EINVAL: null or misaligned pointers, a kind outside {CMP, EAC}, a outside 2 .. PCONV_CUBE_MAX_FACE,
 *   P outside 1 .. 2^28 - 1, records that overlap dirs. */
int pconv_cube_points_records(const double *dirs, int32_t *records, long long P, int kind, int a, void *stream);

/* Weighted squared error over a weight plane (csrc/weighted_metrics.hip; pseudocylindrical_convolution_amd/
 * weighted_metrics.py states the same definition in torch).  WS-PSNR is defined for every projection by its area weights:
 * the weights of a cube picture are the solid angles of its pixels (cube.area_weights); a mask of inactive regions, a half
 * sphere or a region of interest is the same call.
 * Inputs: x and y float32 (n, C, H, W), contiguous, 4-byte aligned (pconv_weighted_mse_f32), or uint8 (n, H, W, 3)
 *   interleaved, each value read as float(u8) / 255.f, correctly rounded (pconv_weighted_mse_u8, C = 3): the same image
 *   gives the same bits in both forms, as in pconv_ws_metrics_u8.
 * Weights: a float64 (H, W) plane on the device, 8-byte aligned, shared by all frames and channels; `total` is W, the
 *   plane's total, which the HOST supplies (weighted_metrics.WeightPlane: math.fsum of the plane, the exactly rounded sum,
 *   which has no order to state).  The kernels never sum the weights.
 * Error of pixel p (the row-major index in the plane): d = x - y in fp32; e = d * d in fp32, widened to double; the term
 *   is w_p * e, one fp64 product.
 * Sum, per plane (f, c), in fp64, in the order stated above for pconv_sphere_points_mse_f32 with "point" read as "pixel":
 *   chunks of PCONV_SPHERE_POINTS_CHUNK = 1024 consecutive pixels; lane l of 256 starts at +0 and adds the terms of the
 *   pixels l, l + 256, l + 512, l + 768 of its chunk that exist, ascending; the tree s = 128 .. 1, lane l < s taking
 *   lane[l] + lane[l + s]; one partial per plane and chunk in the workspace; a second launch adds a plane's partials the same
 *   way (lane l adds the partials l, l + 256, ... ascending, then the tree); out[f][c] = sum / W.  The order depends on H*W
 *   alone: not on the batch, the grid, or the alignment of the pointers.
 * Backward (pconv_weighted_mse_backward_f32): of sum over (f, c) of gout[f][c] * out[f][c], with respect to y.  gout is n*C
 *   doubles on the device.  k = ((2 * gout[f][c]) * w_p) / W in fp64, rounded once to fp32; grad[f][c][p] = k * (y - x), the
 *   difference and the product in fp32.  One launch, every element stored exactly once, no atomics, no workspace.  Where all
 *   four pointers are 16-byte aligned and H*W is a multiple of 4 the kernel moves 16 bytes per access; elsewhere 4; the bits
 *   are the same.  The gradient with respect to x is the same call with x and y swapped.
 * pconv_weighted_mse_workspace_bytes(n, c, h, w) = 8 * n * c * ceil(h*w / 1024) (a negative value when refused); the entry
 *   points allocate nothing.  Refused on the host, before any launch, with PCONV_EINVAL: null or misaligned pointers, a side
 *   outside 1 .. 2^20, a float32 plane of 2^31 bytes or more, n * C outside 1 .. 65535 (u8: C other than 3), a total that is
 *   not finite or not positive, out or the workspace inside an input or each other, a gradient inside an input.  x == y is
 *   allowed. */
long long pconv_weighted_mse_workspace_bytes(int n, int c, int h, int w);
int pconv_weighted_mse_f32(const float *x, const float *y, const double *weights, double total, int n, int c, int h, int w,
                           void *workspace, double *out, void *stream);
int pconv_weighted_mse_u8(const uint8_t *x, const uint8_t *y, const double *weights, double total, int n, int c, int h, int w,
                          void *workspace, double *out, void *stream);
int pconv_weighted_mse_backward_f32(const float *x, const float *y, const double *weights, double total, const double *gout,
                                    int n, int c, int h, int w, float *grad, void *stream);

/* SSIM weighted by a weight plane (csrc/weighted_metrics.hip, the tile passes in csrc/ssim_tile.h; weighted_metrics.
 * ssim_torch states the same definition in float64 torch).  WS-SSIM for any projection whose weights are data: what
 * pconv_ws_metrics_f32 computes with the cosine of an ERP row, with the weight of every pixel read from a plane.  A
 * window knows nothing of the projection: the caller lays the picture out so that a window's neighbourhood in the plane
 * is its neighbourhood on the sphere wherever the weight is not zero (cube.ws_ssim: every face continued by 5 pixels,
 * the ring weighted zero).
 * Inputs: x and y float32 (n, C, H, W), contiguous, 4-byte aligned; weights a float64 (H, W) plane on the device, 8-byte
 *   aligned, shared by all frames and channels; `total` is W, the plane's total, supplied by the host as above.  There is no
 *   uint8 form.
 * map_p, per plane (f, c): exactly the SSIM map of pconv_ws_metrics_f32 for that plane: the 11-tap Gaussian of sigma 1.5
 *   in fp32 applied as g (x) g, zero padding of 5 on the four borders of the H x W plane, C1 = 0.01^2, C2 = 0.03^2, fp32,
 *   separable, the horizontal pass first, every 11-tap sum k-ascending as fmaf(g[k], v, acc) from acc = 0, sigma^2 =
 *   blur(x^2) - mu^2, and the quotient grouped ((2 mu_x mu_y + C1) * (2 s_xy + C2)) / ((mu_x^2 + mu_y^2 + C1) * (s_x^2 +
 *   s_y^2 + C2)).  The two kernels run the same device functions.
 * out[f][c] = (sum over the pixels p of w_p * (double)map_p) / W, float64 (n, C): per plane, as pconv_weighted_mse_f32, not
 *   per frame.  Each term is one fp64 product.
 * Sum, per plane, in fp64, in THIS ORDER, which depends on (H, W) alone (not on the batch, the grid or the alignment of
 *   the pointers): tiles of 32 rows x 64 columns from the plane's origin, row-major, the last of a row or column partial.
 *   Within a tile, 256 lanes: lane (column c = l mod 64, row group q = l / 64) starts at +0 and adds the terms of the rows
 *   8*q .. 8*q + 7 of column c that exist, ascending.  The 64 lanes of a row group: for m = 32, 16, 8, 4, 2, 1 every lane
 *   takes its value + that of lane (c xor m), so all 64 end with the same bits.  The tile's partial is ((q0 + q1) + q2) +
 *   q3, stored in the workspace (one double per plane and tile).  A second launch adds a plane's partials as stated for
 *   pconv_sphere_points_mse_f32: lane l of 256 starts at +0 and adds the partials l, l + 256, ... ascending, then the tree
 *   s = 128 .. 1; out = sum / W.  No atomics, no allocation.
 * pconv_weighted_ssim_workspace_bytes(n, c, h, w) = 8 * n * c * ceil(h / 32) * ceil(w / 64) (a negative value when
 *   refused).  Refused on the host, before any launch, with PCONV_EINVAL: what pconv_weighted_mse_f32 refuses, so also out or
 *   the workspace inside x, y, the weights or each other.  x == y is allowed.  Non-finite inputs: unspecified.
 * Backward (pconv_weighted_ssim_backward_f32; weighted_metrics.ssim_backward_torch states the same in torch): the gradient of
 *   sum over (f, c) of gout[f][c] * out[f][c] with respect to y, x the other picture.  It is the definition of
 *   pconv_ws_metrics_backward_f32 with the per-row factor replaced by a per-pixel one: gout is n*C doubles on the device, one
 *   per plane, and
 *     k_p = (gout[f][c] * w_p) / W  in fp64, rounded once to fp32 (as the squared error's backward forms its factor); zero
 *     outside the plane;
 *     grad_y = (blur(k*a) + (2*y)*blur(k*b)) + x*blur(k*c),
 *   a, b, c exactly those of pconv_ws_metrics_backward_f32, in the same operation order and with its rounding rules (fp32, no
 *   contraction, 11-tap sums k-ascending with fmaf from 0, the horizontal pass first).  There is no km term.  The passes are
 *   those of the ERP entry's kernel (one kernel template, the factor of pass C read from the plane in global memory: nothing
 *   of the plane is staged in LDS).  One launch, a gather: every element of grad_y (float32 (n, C, H, W)) is stored exactly
 *   once; no atomics, no workspace, no allocation.  A pixel's result depends on its plane and that plane's gout alone.  The
 *   gradient with respect to x is the same call with x and y swapped.  The map is fp32, so the gradient agrees with a
 *   float64 evaluation to a bound, not to the bit.  Refused on the host, before any launch, with PCONV_EINVAL: null or
 *   misaligned pointers (x, y, grad_y 4-byte, weights and gout 8-byte), the sizes and the total that the forward refuses,
 *   grad_y inside x, y, the weights or gout. */
long long pconv_weighted_ssim_workspace_bytes(int n, int c, int h, int w);
int pconv_weighted_ssim_f32(const float *x, const float *y, const double *weights, double total, int n, int c, int h, int w,
                            void *workspace, double *out, void *stream);
int pconv_weighted_ssim_backward_f32(const float *x, const float *y, const double *weights, double total, const double *gout,
                                     int n, int c, int h, int w, float *grad_y, void *stream);

/* Ordered backward of the renderer and of the sphere rotation (csrc/remap_backward.hip, csrc/geometry.cpp; viewport.py
 * states the same definition in torch: render_backward_torch).  The forward of view pixel (j, i) of plane (n, c) is the
 * one above without the clamp: S = sum_a wy[a] * (sum_b wx[b] * x[r_a][c_b]) at each of the ss*ss records (j*ss + p,
 * i*ss + t), the ss*ss results summed and multiplied by inv = (float)(1.0 / (ss*ss)) (no factor for ss = 1).  The sphere
 * rotation is the case ss = 1 with the frame as the grid (gh = vh = h, gw = vw = w).  The backward is the adjoint of
 * that linear map, gin = A^T gout, in THIS ORDER:
 * Destination: source pixel (row, column) of plane (n, c): one fp32 accumulator, starting at +0, or, with accumulate
 *   != 0, at the value gin already holds.
 * Term: ((g' * wy[a]) * wx[b]), g' = gout[j][i] for ss = 1, else gout[j][i] * inv, (j, i) = (floor(r / ss), floor(q /
 *   ss)) of grid sample (r, q); every product one fp32 rounding (__fmul_rn), then one __fadd_rn into the accumulator;
 *   never contracted.
 * Order of the terms of a destination: the order in which a sequential walk of the forward reaches it: grid sample
 *   s = r*gw + q ascending, then tap row a = 0 .. 5, then tap column b = 0 .. 5.
 * Which destination a tap (s, a, b) has: the sampler's rule, word for word: column = floor(qu / P), row = floor(qv / P)
 *   of the record map[s]; tap row row - 2 + a through the pole rule (r < 0 -> -1 - r; r >= h -> 2*h - 1 - r), then
 *   clamped to [0, h - 1]; tap column (column - 2 + b) mod w, and in a tap row that crossed a pole (before the clamp)
 *   (c_b + floor(w / 2)) mod w; the mathematical modulo and floor for whatever the map holds.  wy = row (qv mod P) and
 *   wx = row (qu mod P) of the phase table.
 * Taps that coincide (w < 6; an h small enough that the pole rule or the clamp sends two tap rows to one) are terms of
 *   their own, all added, in order.  A destination no term reaches gets +0, or with accumulate != 0 is left untouched.
 *   Nothing depends on the launch grid, the workgroup or the neighbours in the batch: one form, no float atomics.
 * pconv_host_remap_reverse_size(gh, gw): 36*gh*gw, the number of list entries; negative where that exceeds int32.
 * pconv_host_remap_reverse (host): the lists as CSR per source pixel from the map the forward read (a host copy of it):
 *   rev_start h*w + 1 int32, rev_entry 36*gh*gw int32 (144 bytes per grid sample), entry e = s*36 + a*6 + b, ascending
 *   within each list: a stable counting sort of the forward walk by destination.  Returns the entry count.  Refused,
 *   before anything is written: null pointers, a source side outside 2 .. 2^20 or a plane of 2^31 bytes or more, a grid
 *   side outside 2 .. 4*2^20 or a map of 2^31 bytes or more, more entries than int32 holds.
 * pconv_remap_backward_f32: gout holds n frames of (C, vh, vw), gout_frame_stride floats apart (at least C*vh*vw: slot k
 *   of an (n, V, C, vh, vw) gradient is read in place); gin (n, C, h, w); map, phases and the two lists on the device.  A
 *   gather: a lane owns one destination and walks its list; a list is never split.  No atomics, no allocation, no
 *   memset, 64-bit flat indices.  An entry outside 0 .. 36*gh*gw - 1 is skipped and a start outside it clamped, so no
 *   list content makes the kernel read outside `map` or `gout`.  Refused on the host, before any launch, with
 *   PCONV_EINVAL: what pconv_viewport_render_f32 refuses, and gin == gout, null list pointers, lists beyond int32. */
long long pconv_host_remap_reverse_size(int gh, int gw);
int pconv_host_remap_reverse(const int32_t *map, int gh, int gw, int h, int w, int32_t *rev_start, int32_t *rev_entry);
int pconv_remap_backward_f32(const float *gout, float *gin, const int32_t *map, const float *phases, const int32_t *rev_start,
                             const int32_t *rev_entry, int n, int c, int h, int w, int vh, int vw, int ss,
                             long long gout_frame_stride, int accumulate, void *stream);

/* PseudoDQuantOp.forward  (pseudo_dquant_cuda.cu:24-70)
 * weight (wc, levels) raw parameter, level_tab (wc, levels) scratch */
int pconv_dquant(const float *x, const float *weight, float *level_tab, float *out,
                 const int32_t *widths, int tn, int c, int h, int w, int wc, int levels,
                 int npart, void *stream);

/* ProjectsOp.forward  (projects_cuda.cu:181-255)
 * in (n, c, height, width) -> out (nview*n, c, h_out, w_out), viewport-major */
int pconv_project(const float *in, const float *tf, float *out, int n, int c, int height,
                  int width, int nview, int h_out, int w_out, int nearest, void *stream);

/* ContextReshapeOp.forward (context_reshape_cuda.cu:30-60)
 * (n, g*cpg, h, w) -> (n*g*h*w, cpg) */
int pconv_context_reshape(const float *in, float *out, int n, int c, int h, int w, int ngroup,
                          void *stream);

/* ---- backward (transposed) forms of the linear geometry ops: training path, SURVEY 8f-4 ---- */

/* ContextReshapeOp.backward (context_reshape_cuda.cu:63-95): (n*g*h*w, cpg) -> (n, g*cpg, h, w) */
int pconv_context_reshape_backward(const float *top, float *bottom, int n, int c, int h, int w,
                                   int ngroup, void *stream);

/* SphereSliceOp.backward (sphere_slice_cuda.cu:191-244): grad of the tile stack
 * (n*npart, c, height/npart + 2*pad, width + 2*pad) -> grad of the image (n, c, height, width).
 * Same tap tables as the forward call. */
int pconv_sphere_slice_backward(const float *gout, float *gin, const int32_t *widths,
                                const int32_t *tap_col, const float *tap_coef, int n, int c,
                                int height, int width, int npart, int pad, void *stream);

/* SphereUsliceOp.backward (sphere_uslice_cuda.cu:128-200): grad of the image (n, c, h*npart, width)
 * -> grad of the tile stack (n*npart, c, h + 2*pad, width + 2*pad), zero outside the valid interior */
int pconv_sphere_uslice_backward(const float *gout, float *gin, const int32_t *widths,
                                 const int32_t *tap_col, const float *tap_coef, int n, int c, int h,
                                 int width, int npart, int pad, void *stream);

/* Reverse of pconv_host_pad_table: CSR over interior elements (tile*height + row)*width + col ->
 * halo entries that read the element, (destination tile << 24 | padded row*width + column, weight).
 * rev_start: npart*height*width + 1 ints; rev_dst / rev_wgt: up to 4*npart*pad*width records.
 * Returns the number of records.  Replaces pseudo_context_backward_kernel
 * (pseudo_context_cuda.cu:106-138), whose atomics-built lists have no defined order. */
int pconv_host_pad_reverse(const int32_t *widths, int npart, int height, int width, int pad,
                           int32_t *rev_start, int32_t *rev_dst, float *rev_wgt);

/* PseudoPadOp.backward (pseudo_pad.cu:127-235): grad (tn, c, h+2p, w+2p) -> (tn, c, h, w); gout is
 * not modified (the reference folds the wrap columns into its argument in place) */
int pconv_pseudo_pad_backward(const float *gout, float *gin, const int32_t *widths,
                              const int32_t *rev_start, const int32_t *rev_dst, const float *rev_wgt,
                              int tn, int c, int h, int w, int pad, int npart, void *stream);

/* PseudoEntropyPadOp.forward / backward (pseudo_entropy_pad_cuda.cu:39-241): the causal pad of the
 * training-time entropy net -- halo rows through pconv_host_causal_table, right wrap only, no pole
 * mirror.  in (tn, c, h, w) <-> out (tn, c, h+2p, w+2p). */
int pconv_entropy_pad(const float *in, float *out, const int32_t *widths, const int32_t *col,
                      const float *wgt, int tn, int c, int h, int w, int pad, int npart, void *stream);
int pconv_host_entropy_pad_table(const int32_t *widths, int npart, int height, int width, int pad,
                                 int version, int32_t *col, float *wgt);
int pconv_host_causal_reverse(const int32_t *widths, int npart, int height, int width, int pad,
                              int version, int32_t *rev_start, int32_t *rev_dst, float *rev_wgt);
int pconv_entropy_pad_backward(const float *gout, float *gin, const int32_t *widths,
                               const int32_t *rev_start, const int32_t *rev_dst, const float *rev_wgt,
                               int tn, int c, int h, int w, int pad, int npart, void *stream);

/* ProjectsOp.backward (projects_cuda.cu:257-329): gout (n*nview, c, h_out, w_out) -> gin and count
 * (n, c, height, width); count = the sampling weights each source pixel received. */
int pconv_project_backward(const float *gout, const float *tf, float *gin, float *count, int n, int c,
                           int height, int width, int nview, int h_out, int w_out, int nearest,
                           void *stream);

/* PseudoQuantOp.backward (pseudo_quant_cuda.cu:197-311).  x / val / idx: input and the two outputs
 * of the forward call, level_tab: the table that call filled; g_val / g_idx (may be NULL): gradients
 * of the outputs.  g_in (tn,c,h,w), g_weight (c,levels); bins: scratch of c*levels floats. */
int pconv_quant_backward(const float *x, const float *val, const float *idx, const float *g_val,
                         const float *g_idx, const float *level_tab, float *g_in, float *g_weight,
                         float *bins, const int32_t *widths, float top_alpha, int tn, int c, int h,
                         int w, int levels, int npart, void *stream);

/* ---- ordered (atomic-free) forms of the four backward calls above that sum with float atomics ----
 *
 * THE ORDER.  For all four: one fp32 accumulator per destination element, starting at +0; every term is one
 * fp32 product rounded on its own (__fmul_rn), then one fp32 add (__fadd_rn); the terms come in the order given
 * here, which is the order in which the sequential scatter of oracle/pconv_oracle.c reaches the element.  The
 * result does not depend on grid size, workgroup size or batch neighbours.
 *
 *   slice     destination: ERP pixel (frame, channel, row, column j).  The tile columns tw of that row's tile pt,
 *             ascending over tw < widths[pt]; within one tw the taps -1, 0, +1, +2 whose column
 *             (tap_col + tap) mod width is j.  Term: gout[tw] * coef.
 *   uslice    destination: valid tile column i of (tile, channel, row).  The ERP columns tw of that row,
 *             ascending; within one tw the taps -1, 0, +1, +2 whose column (tap_col + tap) mod wl is i, wl the
 *             tile's valid width (wl < 4: one tw meets a column twice, both terms are added, in tap order).
 *             Term: gout[tw] * coef.  The kernel writes every element outside the valid interior as zero.
 *   projects  destination: ERP pixel of a plane.  Viewport pixel ps ascending, then view tb ascending; within a
 *             sample the corners (th,tw), (th,pw), (ph,tw), (ph,pw) (the pole clamp makes ph == th on the last
 *             row: both terms are added).  With tx = fx - tw, ntx = 1. - tx (a double subtraction rounded to
 *             float) and ty, nty alike, the corner weights are the float products ntx*nty, tx*nty, ntx*ty, tx*ty
 *             and the term is weight * g.  nearest: one term 1 * g per sample.  `count` is the same ordered sum
 *             of the weights.  A pixel no sample reaches gets 0 and count 0.
 *   quant     g_in is elementwise (as pconv_quant_backward).  bins[c][q] = sum of val - x (each difference one
 *             fp32 rounding, then widened to fp64) over the live elements of channel c at level q, in a fixed
 *             shape:  (1) per (tile-image t, channel c) plane of h*w elements, lane l = e mod 256 of 256 adds
 *             the plane's live elements e = l, l + 256, ... (e = row*w + column, ascending) to one fp64
 *             accumulator a[q][l], from +0;  (2) per level the tree  for s = 128, 64, ..., 1:
 *             a[q][l] = a[q][l] + a[q][l + s] for l < s  leaves the plane's partial in a[q][0];  (3) bins[c][q]
 *             = the partials of planes t = 0 .. tn-1 of channel c, ascending, added in fp64 from +0, rounded
 *             once to fp32.  g_weight is the suffix sum over q of pconv_quant_backward, unchanged.
 */

/* Entries pconv_host_tap_reverse writes: 4 per forward output of a row (slice: the tiles' valid columns;
 * uslice: npart * width). */
long long pconv_host_tap_reverse_size(const int32_t *widths, int npart, int width, int uslice);

/* Transpose of the tap table of pconv_host_slice_taps (uslice = 0) / pconv_host_uslice_taps (uslice = 1) as a
 * CSR list per (tile, destination column), entries (source column, coefficient) in THE ORDER: rev_start
 * npart*width + 1 ints, rev_src / rev_coef pconv_host_tap_reverse_size entries.  The lists do not depend on
 * the row.  Refuses -- before it writes anything -- null pointers, widths outside 1..width, entry counts beyond
 * int32 and tap columns outside their period (width, or the tile's width for uslice).  Returns the number of
 * entries. */
int pconv_host_tap_reverse(const int32_t *widths, int npart, int width, const int32_t *tap_col,
                           const float *tap_coef, int uslice, int32_t *rev_start, int32_t *rev_src,
                           float *rev_coef);

/* Entries pconv_host_project_reverse writes: nview * inner samples, 4 corners each (1 when nearest). */
long long pconv_host_project_reverse_size(int nview, int inner, int nearest);

/* Transpose of the viewport sampling of pconv_host_project_table's table tf (nview, inner = h_out*w_out, 2)
 * as a CSR list per ERP pixel, entries (sample index tb*inner + ps, weight) in THE ORDER, built by a stable
 * counting sort of the forward walk: rev_start height*width + 1 ints, rev_sample / rev_wgt
 * pconv_host_project_reverse_size entries.  Refuses -- before it writes anything -- null pointers, sizes whose
 * entry count or pixel count does not fit int32 and samples outside the frame.  Returns the number of entries. */
int pconv_host_project_reverse(const float *tf, int nview, int inner, int height, int width, int nearest,
                               int32_t *rev_start, int32_t *rev_sample, float *rev_wgt);

/* pconv_sphere_slice_backward / pconv_sphere_uslice_backward in THE ORDER, through the lists of
 * pconv_host_tap_reverse; shapes and the 64 KB row limit as there.  The uslice form writes all of gin. */
int pconv_sphere_slice_backward_ordered(const float *gout, float *gin, const int32_t *widths,
                                        const int32_t *rev_start, const int32_t *rev_src,
                                        const float *rev_coef, int n, int c, int height, int width,
                                        int npart, int pad, void *stream);
int pconv_sphere_uslice_backward_ordered(const float *gout, float *gin, const int32_t *widths,
                                         const int32_t *rev_start, const int32_t *rev_src,
                                         const float *rev_coef, int n, int c, int h, int width,
                                         int npart, int pad, void *stream);

/* pconv_project_backward in THE ORDER, through the lists of pconv_host_project_reverse (which hold the
 * nearest / bilinear choice); writes all of gin and count. */
int pconv_project_backward_ordered(const float *gout, const int32_t *rev_start, const int32_t *rev_sample,
                                   const float *rev_wgt, float *gin, float *count, int n, int c,
                                   int height, int width, int nview, int h_out, int w_out, void *stream);

/* pconv_quant_backward with the level sums in THE ORDER; workspace: device memory of
 * pconv_quant_backward_ordered_workspace_bytes(tn, c, levels) bytes (one fp64 per plane and level).
 * levels <= 32. */
long long pconv_quant_backward_ordered_workspace_bytes(int tn, int c, int levels);
int pconv_quant_backward_ordered(const float *x, const float *val, const float *idx, const float *g_val,
                                 const float *g_idx, const float *level_tab, float *g_in, float *g_weight,
                                 float *bins, void *workspace, const int32_t *widths, float top_alpha,
                                 int tn, int c, int h, int w, int levels, int npart, void *stream);

/* MaskConstrainOp.forward, in place on a conv weight (nout, cin, k, k)
 * (mask_constrain_cuda.cu:19-88); constrain in {1,2,5,6} */
int pconv_mask_constrain(float *weight, int nout, int cin, int k, int ngroup, int constrain,
                         void *stream);

/* EntropyGmmOp.forward (entropy_gmm_cuda.cu:36-92): loss (m) plus the four
 * gradient buffers the reference keeps for backward (may be NULL). */
int pconv_gmm_loss(const float *weight, const float *delta, const float *mean,
                   const float *label, float *loss, float *d_weight, float *d_delta,
                   float *d_mean, float *d_label, int m, int ng, void *stream);

/* Dense per-tile convolution, implicit GEMM on fp32 MFMA (the nn.Conv2d call
 * sites of model_zoo_v2.py:41-45,83-86,100-105,119,143,158-164,181,205; cuDNN in
 * the reference).  in (tn, cin, h, w); packed_w from pconv_conv_pack_weight;
 * out (tn, cout, ho, wo), ho = (h - k)/stride + 1, no implicit padding.
 * k in {1,3}, stride in {1,2}.  act: 0 none, 1 PReLU(slope[cout]), 4 sigmoid.
 * col_limit (may be NULL): per latitude tile (t % npart) the first dead output
 * column; 64-column tiles starting at or beyond it are written as zeros without
 * being computed.
 * Every output is one k-ascending fp32 fmaf chain from 0 (k = (ci*k + kh)*k + kw),
 * then + bias, then the activation; then, each optional and in this order,
 * * gate[.], + residual[.] (both shaped like out, may be NULL: the attention
 * product and the residual sum that follow the convolution in
 * model_zoo_v2.py:53,76,93,114,175) and, with trim != 0, zero from col_limit on
 * (the PseudoFill that ends every block).
 * d2w != 0: DtowOp(2, d2w) (dtow_cuda.cu:38-75) applied by the store -- out is
 * (tn, cout/4, 2*ho, 2*wo); only with act 0/1 and no gate / residual / trim.
 * views (may be NULL = all dense NCHW): 12 element strides, (tile, channel, row)
 * for in, out, residual, gate in this order; columns are always contiguous.
 * Lets a convolution write the interior of a padded buffer (whose ring
 * pconv_pseudo_pad_ring then fills) and read such interiors.
 * Number range: the chain is IEEE over all of fp32 -- subnormal inputs, weights,
 * products, partial sums and results are kept, never flushed (the matrix
 * instructions run under the kernel's default denormal mode); the chain starts
 * at +0, so an all-zero sum is +0 whatever the signs of its terms, and -0
 * appears only where IEEE gives it (a later product, bias, PReLU or residual);
 * overflow goes to +-Inf and Inf - Inf to NaN in chain order.  The same holds
 * for pconv_gdn (x*x may underflow or overflow on its own), for the entropy
 * model's kernels in all three forms, for pconv_expf (its results below 2^-126
 * are correctly scaled subnormals) and for the quantiser.  Measured on the
 * MI355X against the CPU restatement, bit for bit incl. the sign of zero
 * (tests/test_gpu_fp32_edges.py).  The Winograd kernels promise exact
 * power-of-two scaling in the normal range, no bit equality below it.  NaN
 * INPUTS stay unspecified beyond what single entries state. */
int pconv_conv_packed_size(int cout, int cin, int k, int *cout_pad, int *red_pad);
int pconv_conv_pack_weight(const float *w, float *packed, int cout, int cin, int k,
                           void *stream);
int pconv_conv2d(const float *in, const float *packed_w, const float *bias, float *out,
                 int tn, int cin, int h, int w, int cout, int k, int stride, int act,
                 const float *slope, const int32_t *col_limit, int npart,
                 const float *residual, const float *gate, int trim, int d2w,
                 const long long *views, void *stream);

/* Backward of pconv_conv2d's layers in a defined order (csrc/conv_backward.hip): k in {1,3}, stride in {1,2},
 * no padding, dense NCHW fp32: in (tn, cin, h, w), w (cout, cin, k, k), gout (tn, cout, ho, wo).  Stream-ordered;
 * no atomics, no allocation and no memset inside a call: the caller brings the workspaces.  Null pointers,
 * unsupported k / stride and shapes beyond int32 are refused before any launch.  Results do not depend on the
 * grid, the device's CU count, an option or the workspace's size.
 *
 * Data gradient: gin (tn, cin, h, w) = pconv_conv2d, stride 1, no bias, no activation, of the PREPARED gradient
 * with the flipped, transposed weights wT[ci][co][kh'][kw'] = w[co][ci][k-1-kh'][k-1-kw']
 * (pconv_conv_pack_weight_transposed writes them in pconv_conv_pack_weight's layout:
 * pconv_conv_packed_size(cin, cout, k) floats).  The prepared gradient (tn, cout, h + k - 1, w + k - 1) holds
 * element (y, x) of a gout plane at (k-1 + stride*y, k-1 + stride*x) and +0 everywhere else: zero-stuffed to the
 * stride, padded by k - 1 on every side, with (h-k) % stride / (w-k) % stride further zero rows / columns at the
 * bottom / right.  pconv_conv_grad_prepare writes all of it in one pass (16-byte aligned buffer).  Every gin
 * element is therefore ONE fp32 fmaf chain from +0 over (co, kh', kw') ascending, in which stuffed and padded
 * positions enter as products with +0.  pconv_conv2d_dgrad chains prepare and pconv_conv2d; workspace: device
 * memory of pconv_conv2d_dgrad_workspace_bytes(...) bytes (0 for k = 1, stride 1, where the prepared gradient
 * is gout itself and workspace may be NULL).
 *
 * Weight gradient: for every tile t a partial P_t[co][ci][kh][kw] = ONE fp32 fmaf chain from +0 over the tile's
 * output pixels, y ascending then x ascending: acc = fmaf(gout[t,co,y,x], in[t,ci,stride*y+kh,stride*x+kw], acc)
 * (v_mfma_f32_32x32x2_f32: M = couts, N = (ci, kh, kw), K = pixels).  The pixels are taken in runs of up to 64
 * of one output row, [64 j, 64 j + 64) for j = 0 .. (wo-1)/64; a run of odd length -- a function of wo alone --
 * is followed by one step fmaf(-0, +0, acc), which returns acc for every acc (-0, Inf and NaN included), so the
 * chain has no zero-product step that could turn a -0 into +0.  Then gw = (((P_0 + P_1) + P_2) + ...), fp32
 * round-to-nearest adds, t ascending.
 * Bias gradient: gb[co] = the two-stage reduction of pconv_quant_backward_ordered: per plane (t, co), lane l of
 * 256 adds elements l, l + 256, ... ascending in fp64 from +0; the tree a[l] += a[l + s], s = 128 .. 1; then the
 * planes t ascending in fp64 from +0; one rounding to fp32.
 * pconv_conv2d_wgrad writes gw and gb (either may be NULL: not computed; in may be NULL without gw);
 * workspace: 16-byte aligned device memory of pconv_conv2d_wgrad_workspace_bytes(tn, cin, cout, k) bytes (the
 * partials, then one fp64 per plane; without gw the planes alone: tn * cout * 8 bytes suffice).
 *
 * Number range: as for pconv_conv2d -- subnormal operands, products and sums are kept, never flushed, and every
 * chain starts at +0 -- with one exception: Inf / NaN in gout are UNSPECIFIED for the data gradient, whose
 * stuffed and padded zeros multiply them (0 * Inf = NaN reaches gin elements the value has no part in).  The
 * weight and bias gradients carry Inf / NaN in chain order. */
int pconv_conv_pack_weight_transposed(const float *w, float *packed, int cout, int cin, int k,
                                      void *stream);
long long pconv_conv2d_dgrad_workspace_bytes(int tn, int cout, int h, int w, int k, int stride);
int pconv_conv_grad_prepare(const float *gout, float *prepared, int tn, int cout, int h, int w,
                            int k, int stride, void *stream);
int pconv_conv2d_dgrad(const float *gout, const float *packed_wt, float *gin, void *workspace,
                       int tn, int cin, int h, int w, int cout, int k, int stride, void *stream);
long long pconv_conv2d_wgrad_workspace_bytes(int tn, int cin, int cout, int k);
int pconv_conv2d_wgrad(const float *in, const float *gout, float *gw, float *gb, void *workspace,
                       int tn, int cin, int h, int w, int cout, int k, int stride, void *stream);

/* The 5x5 convolution of the entropy model's masked layers under training (MaskConstrain.py:24-38: MaskConv2 /
 * MaskConv3 call nn.functional.conv2d on the masked weight), forward and backward: stride 1, no padding, dense NCHW
 * fp32: in (tn, cin, h, w), w (cout, cin, 5, 5), out / gout (tn, cout, h - 4, w - 4).  Entry points of their own:
 * pconv_conv2d, pconv_conv_pack_weight[_transposed], pconv_conv2d_dgrad and pconv_conv2d_wgrad keep refusing k = 5.
 * THE ORDERS ARE THE SAME as those defined above for pconv_conv2d and its backward, taken at k = 5, stride 1:
 *   forward: every output is one fp32 fmaf chain from +0 over (ci, kh, kw) ascending, then + bias (may be NULL).
 *     EVERY tap is a step of the chain, also a tap whose weight is zero: the kernels do not know the causal mask
 *     (fmaf(x, +0, acc) differs from acc for acc = -0 and for x not finite), the definition is the dense chain on
 *     the masked weight;
 *   data gradient: pconv_conv5 of the prepared gradient -- gout padded by 4 with +0 on every side, (tn, cout,
 *     h + 4, w + 4); there is no stuffing at stride 1 -- with the flipped, transposed weights
 *     wT[ci][co][kh'][kw'] = w[co][ci][4-kh'][4-kw'] (pconv_conv5_pack_weight_transposed, pconv_conv5_packed_size(cin,
 *     cout) floats): one fmaf chain from +0 over (co, kh', kw') ascending per gin element;
 *   weight gradient: per tile t the partial P_t[co][ci][kh][kw] = one fmaf chain from +0 over the tile's output
 *     pixels, y then x ascending, on v_mfma_f32_32x32x2_f32, in runs of up to 64 pixels of one output row, a run of
 *     odd length followed by the step fmaf(-0, +0, acc); then gw = (((P_0 + P_1) + P_2) + ...) in fp32, t ascending;
 *   bias gradient: the fixed-shape two-stage fp64 reduction of pconv_conv2d_wgrad.
 * No atomics, no allocation and no memset inside a call; 64-bit flat indices; subnormals are kept; results do not
 * depend on the grid, the CU count, an option or the workspace's size; null pointers, h or w below 5, shapes beyond
 * int32 and a missing or misaligned workspace are refused before any launch.  Inf / NaN in gout are unspecified
 * for the data gradient only (its padded zeros multiply them).
 * Packed weights: pconv_conv5_packed_size(cout, cin) floats, 16-byte aligned ([red_pad][cout_pad], cin padded to
 * 2, cout to 32 / 96 / 192; negative when the weight exceeds int32).  Workspaces, 16-byte aligned device memory:
 *   pconv_conv5_dgrad_workspace_bytes(tn, cout, h, w) = tn * cout * (h + 4) * (w + 4) * 4 (h, w: the INPUT's);
 *   pconv_conv5_wgrad_workspace_bytes(tn, cin, cout) = tn * cout * cin * 25 * 4 rounded up to 16, + tn * cout * 8
 *   (the partials, then one fp64 per plane; without gw the planes alone: tn * cout * 8 bytes suffice).
 * pconv_conv5_wgrad writes gw and gb (either may be NULL: not computed; in may be NULL without gw). */
int pconv_conv5_packed_size(int cout, int cin, int *cout_pad, int *red_pad);
int pconv_conv5_pack_weight(const float *w, float *packed, int cout, int cin, void *stream);
int pconv_conv5_pack_weight_transposed(const float *w, float *packed, int cout, int cin, void *stream);
int pconv_conv5(const float *in, const float *packed_w, const float *bias, float *out, int tn, int cin,
                int h, int w, int cout, void *stream);
long long pconv_conv5_dgrad_workspace_bytes(int tn, int cout, int h, int w);
int pconv_conv5_dgrad(const float *gout, const float *packed_wt, float *gin, void *workspace, int tn,
                      int cin, int h, int w, int cout, void *stream);
long long pconv_conv5_wgrad_workspace_bytes(int tn, int cin, int cout);
int pconv_conv5_wgrad(const float *in, const float *gout, float *gw, float *gb, void *workspace, int tn,
                      int cin, int h, int w, int cout, void *stream);

/* The same convolution for k = 3, stride 1 by Winograd F(2x2, 3x3) on the fp32 matrix cores
 * (csrc/wino.hip): 4 instead of 9 multiply-adds per input channel, output channel and pixel -- the
 * algorithm cuDNN runs the reference's fp32 3x3 nn.Conv2d layers with (model_zoo_v2.py:41-45,83-86,
 * 158-164).  Results differ from pconv_conv2d's fmaf chain by rounding (~1e-6 relative).
 * packed_u from pconv_wino_pack_weight (pconv_wino_packed_size floats).  Arguments as pconv_conv2d
 * without k / stride / gate; act 0 or 1; views: 9 strides (in, out, residual) or NULL.  Takes the
 * layers pconv_wino_supported(...) accepts -- the single source of truth: cin % 16 == 0 (no ragged
 * channel path), cout >= 32, h, w >= 4, even output size, cout % 4 == 0 with d2w -- and returns
 * PCONV_EINVAL for anything else; rows of out / residual must start on 8-byte boundaries.  Input
 * views whose KC-channel chunk spans 4 GiB or more are refused (the LDS-DMA addresses a chunk as a
 * 64-bit uniform base + a 32-bit byte offset per lane); pconv_conv2d does the same for its 16-channel
 * chunks. */
long long pconv_wino_packed_size(int cout, int cin);
int pconv_wino_pack_weight(const float *w, float *packed, int cout, int cin, void *stream);
int pconv_wino_supported(int cin, int h, int w, int cout, int d2w);
int pconv_conv3x3_wino(const float *in, const float *packed_u, const float *bias, float *out,
                       int tn, int cin, int h, int w, int cout, int act, const float *slope,
                       const int32_t *col_limit, int npart, const float *residual, int trim,
                       int d2w, const long long *views, void *stream);
/* The same convolution with a 2-row x 128-column workgroup tile instead of 4 x 64 (csrc/wino_flat.hip): for launches of
 * TWO output rows (the remainders of PCONV.tile_conv2d's row split); same arguments, same packed weights, same bits per
 * output as pconv_conv3x3_wino. */
int pconv_conv3x3_wino_flat(const float *in, const float *packed_u, const float *bias, float *out,
                       int tn, int cin, int h, int w, int cout, int act, const float *slope,
                       const int32_t *col_limit, int npart, const float *residual, int trim,
                       int d2w, const long long *views, void *stream);

/* The same layers by Winograd F(4x2, 3x3) (csrc/wino42.hip): F(4, 3) vertically, F(2, 3) horizontally --
 * 3 instead of 4 (direct: 9) multiply-adds per input channel, output channel and pixel.  Same arguments and
 * epilogues as pconv_conv3x3_wino; takes the layers pconv_wino42_supported(...) accepts: cin % 24 == 0,
 * cout >= 32, at least 4 output rows, output width even (d2w: cout % 4 == 0).  Results differ from
 * pconv_conv2d's fmaf chain by rounding (~3e-6 relative; model_zoo_v2.py:41-45,83-86,158-164 are fp32
 * nn.Conv2d layers cuDNN runs with Winograd as well). */
long long pconv_wino42_packed_size(int cout, int cin);
int pconv_wino42_pack_weight(const float *w, float *packed, int cout, int cin, void *stream);
int pconv_wino42_supported(int cin, int h, int w, int cout, int d2w);
int pconv_conv3x3_wino42(const float *in, const float *packed_u, const float *bias, float *out,
                       int tn, int cin, int h, int w, int cout, int act, const float *slope,
                       const int32_t *col_limit, int npart, const float *residual, int trim,
                       int d2w, const long long *views, void *stream);

/* PseudoGDNV2.forward (PseudoContextV2.py:133-216) in one launch on the same
 * kernel: out = in / sqrt(beta + gamma * in^2) over channels (inverse: in * sqrt),
 * zeros from each tile's col_limit on (the reference's mask).  in, out
 * (tn, ch, h, w), distinct; packed_gamma = pconv_conv_pack_weight of the effective
 * (re-parametrised) gamma viewed as a (ch, ch, 1, 1) weight; beta (ch) effective. */
int pconv_gdn(const float *in, const float *packed_gamma, const float *beta, float *out,
              int tn, int ch, int h, int w, int inverse, const int32_t *col_limit, int npart,
              const float *residual /* added inside the valid columns, may be NULL */,
              const long long *views /* 9 strides: in, out, residual; may be NULL */,
              void *stream);

/* ------------------------------------------------------------------------
 * Device kernels -- entropy wavefront (one call = one step of one op)
 * `order`/`plane_start` come from pconv_host_wavefront; lo/hi = the range of
 * schedule entries handled by this step (plane_start[st] .. plane_start[end]).
 * ---------------------------------------------------------------------- */

/* DInput2Op.forward body (d_input_cuda_v2.cu:32-52): scatter packed symbols
 * (+bias) of the previous step into ctx (rep*nimg*npart, ngroup, h+2p, w+2p) */
int pconv_dinput2(const float *packed, float *ctx, const int32_t *order, int lo, int len,
                  int nimg, int ngroup, int npart, int h, int w, int pad, int psum,
                  float bias, int rep, void *stream);

/* EntropyCtxPadRun2Op.forward body, in place (entropy_ctx_pad_run2_cuda.cu:33-65).
 * list arrays from pconv_host_causal_halo; entry_plane[k] = plane of entry k. */
int pconv_ctx_pad_run2(float *data, const int32_t *dst, const int32_t *src0,
                       const int32_t *src1, const float *wgt, const int32_t *entry_plane,
                       int lo, int len, int nimg, int cpn, int channel, int npart, int h, int w,
                       int pad, int psum, void *stream);

/* EntropyConv2Op.forward{,_act,_batch,_act_batch} body
 * (entropy_conv_cuda_v2.cu:61-459).  x (nimg*npart, cin, h+2pi, w+2pi),
 * weight (nset, cout, cin, 5, 5), bias (nset, cout), slope NULL = no PReLU,
 * y (nimg*npart, cout, h+2po, w+2po) persistent.  nimg = images incl. replicas,
 * per_set = nimg / nset.  The step covers planes [first_plane, first_plane+nplane)
 * of the schedule (`plane_start` is the device copy of pconv_host_wavefront's
 * prefix array, max_plane_len the longest of those planes); the output group of
 * plane p is psum - p.
 * residual (may be NULL, same shape as y): added after the activation, i.e.
 * EntropyAddOp folded into the epilogue.
 * widths / vh_col / vh_wgt (may be NULL): pconv_host_causal_table of the input;
 * when given, halo taps are computed on the fly from tile interiors and the
 * stored halo of x is never read (no EntropyCtxPadRun2 needed). */
int pconv_entropy_conv(const float *x, const float *weight, const float *bias,
                       const float *slope, float *y, const int32_t *order,
                       const int32_t *plane_start, int first_plane, int nplane, int max_plane_len,
                       int nimg, int per_set, int cin, int cout, int ngroup, int k, int constrain,
                       int npart, int h, int w, int pad_in, int pad_out, int psum,
                       const float *residual, const int32_t *widths, const int32_t *vh_col,
                       const float *vh_wgt, void *stream);

/* EntropyAddOp.forward body, in place y += x (entropy_add_cuda.cu:25-44) */
int pconv_entropy_add(float *y, const float *x, const int32_t *order, int lo, int len,
                      int nimg, int channel, int ngroup, int npart, int h, int w, int pad,
                      int psum, void *stream);

/* DExtract2Op.forward body (d_extract_cuda_v2.cu:34-52): gather to packed list
 * out[(img*len + l)*cpn + ci] */
int pconv_dextract2(const float *x, float *out, const int32_t *order, int lo, int len,
                    int nimg, int channel, int cpn, int npart, int h, int w, int psum,
                    void *stream);

/* DExtract2Op.forward_batch body (d_extract_cuda_v2.cu:110-132): three packed
 * sections at distance `section_stride` */
int pconv_dextract2_batch(const float *x, float *out, const int32_t *order, int lo, int len,
                          int nimg, int channel, int cpn, int npart, int h, int w, int psum,
                          int nout, long long section_stride, void *stream);

/* EntropyGmmTableOp.forward_batch / forward (entropy_gmm_table_cuda.cu:29-185).
 * weight/delta/mean are (tn, ng) each, modified in place like the reference
 * (softmax / relu+beta); table (tn, nstep+1) holds integers as floats.
 * batch_arith != 0 selects forward_batch's mixed float/double accumulation
 * (:136-153), 0 the all-float accumulation of forward (:59-80). */
int pconv_gmm_table(float *weight, float *delta, const float *mean, float *table, int tn,
                    int ng, int nstep, float bias, float total, float beta, int batch_arith,
                    void *stream);

/* Engine step: DExtract2Batch + EntropyBatchGmmTable (+ the label DExtract2) in
 * one launch, integer output.  y (3*nimg*npart, 3*ngroup, h, w) = last layer;
 * table int32 [nimg*len][nstep+1]; symbols (nimg*npart, ngroup, h, w) / labels
 * int32 [nimg*len] may both be NULL. */
int pconv_step_tables(const float *y, const float *symbols, int32_t *table, int32_t *labels,
                      const int32_t *order, int lo, int len, int nimg, int ngroup, int npart, int h,
                      int w, int psum, int nstep, float bias, float total, float beta, void *stream);

/* encoder side of DInput2: scatter ALL symbols at once, ctx (rep*tn, c, h+2p, w+2p)
 * interior = symbol + bias inside the valid width (the buffer must be zeroed) */
int pconv_symbols_to_ctx(const float *symbols, float *ctx, const int32_t *widths, int tn, int c,
                         int h, int w, int pad, int npart, float bias, int rep, void *stream);

/* decoded symbols out of the padded context tensor (tn, c, h+2p, w+2p):
 * out (tn, c, h, w) = interior + bias inside each tile's valid width, 0 elsewhere
 * (pseudo_codec.py:159-160) */
int pconv_ctx_to_symbols(const float *ctx, float *out, const int32_t *widths, int tn, int c, int h,
                         int w, int pad, int npart, float bias, void *stream);

/* ------------------------------------------------------------------------
 * Native entropy engine: the EntEncoder / EntDecoder loops
 * (pseudo_codec.py:97-114,145-160) as one C++ host loop over the step kernels
 * above, `nimg` frames in lock-step, one arithmetic-coded stream per frame.
 * The streams are byte-identical to what the per-op path writes.
 * ---------------------------------------------------------------------- */
typedef struct pconv_entropy_engine pconv_entropy_engine;

/* h, w: rows per tile and columns of the symbol tensor (after Dtow);
 * tile_weight[npart] as for pconv_host_tile_widths; bias = (levels-1)/2. */
pconv_entropy_engine *pconv_ee_create(int npart, int ngroup, int h, int w, int nimg,
                                      const float *tile_weight, float bias, int nlevels, float total,
                                      float beta);
void pconv_ee_destroy(pconv_entropy_engine *e);
/* A non-blocking HIP stream on the current device, created directly (not out of a framework's stream pool): the
 * copy streams of the frame pipe (host <-> HBM beside the compute).  The caller destroys it. */
int pconv_stream_create(void **stream);
int pconv_stream_destroy(void *stream);
/* layer 0..11 = net.0.conv, net.1.conv1.conv, net.1.conv2.conv, ..., net.6.conv;
 * device pointers: weight (3, 3G, cin, 5, 5), bias (3, 3G), slope (3, 3G) or NULL.
 * The weight is copied (re-packed) on `stream`; bias and slope are borrowed. */
int pconv_ee_set_layer(pconv_entropy_engine *e, int layer, const float *weight, const float *bias,
                       const float *slope, void *stream);
long long pconv_ee_symbols_per_image(const pconv_entropy_engine *e);
int pconv_ee_steps(const pconv_entropy_engine *e);
/* Host side of the engine (no reference counterpart: the reference drives its loop from one Python
 * thread, pseudo_codec.py:145-160; its only multi-process code is one process per GPU,
 * test/trainDDP_Full.py:83-86,201-204).  pconv_ee_host_cpus: CPUs this rank's host threads can count
 * on = min(affinity mask, cgroup CPU quota / LOCAL_WORLD_SIZE).  pconv_ee_spin_us: microseconds an
 * idle decode worker polls before it blocks when a call runs `call_threads` host threads (one per
 * frame): 2000 (through the GPU part of a step) only if call_threads + 1 <= pconv_ee_host_cpus(),
 * else 60; PCONV_ENGINE_SPIN_US overrides.  Neither touches the GPU.  Like pconv_ee_host_plan they read the
 * environment when they are called; an engine keeps what pconv_ee_create read (pconv_option). */
int pconv_ee_host_cpus(void);
int pconv_ee_spin_us(int call_threads);
/* How an engine of `nimg` frames lays out its host side here (any pointer may be NULL): lock-step groups (= decoder
 * chains = driver threads), threads that arithmetic-decode a group's frames (0 = one per frame), queued-ahead (1)
 * or host-driven (0) chain, waits that sleep instead of spinning.  With nimg + 1 <= pconv_ee_host_cpus(): the
 * measured best of profiles/round3_decode_groups.txt; otherwise (a rank with a small share of the host) at most
 * one group per CPU, one decoding thread per group, host-driven chain, sleeping waits (blocking events)
 * (profiles/round5_host_share.txt).  PCONV_ENGINE_GROUPS / _WORKERS / _CHAIN / _BLOCKING_SYNC override. */
int pconv_ee_host_plan(int nimg, int *groups, int *group_threads, int *queued_chain, int *blocking_sync);
/* How the host threads of THIS engine wait for the GPU: 0 = the runtime's default (spinning) stream waits, 1 = sleeping
 * waits on blocking events (hipEventBlockingSync; the plan's blocking_sync, fixed at pconv_ee_create).  No device-wide
 * schedule flag is set either way. */
int pconv_ee_wait_mode(const pconv_entropy_engine *e);
/* Which kernel THIS engine's encoder runs for `layer` (0 .. 11), decided at pconv_ee_create: 0 = the vector kernel,
 * 1 = the 16x16x4 matrix-core form, 2 = the four-block matrix-core form (v_mfma_f32_16x16x1_4b_f32).  Matrix forms
 * need an even width and 14, 28 or 48 groups (28 / 48: hidden layers 1 .. 11 only); PCONV_EE_BULK=valu keeps the
 * vector kernel everywhere.  PCONV_EINVAL (pconv_last_error) for a bad layer. */
int pconv_ee_encoder_form(const pconv_entropy_engine *e, int layer);
/* The tuning options of the library (PCONV_* environment variables; every one, its default and the measurement
 * behind it: DESIGN.md, "What runs by default").  Two lifetimes: an ENGINE keeps the options pconv_ee_create read
 * (PCONV_ENGINE_*, PCONV_EE_*) -- no later call of that engine looks at the environment -- and a stateless entry
 * point (pconv_conv2d, pconv_gdn: PCONV_CONV*; pconv_sphere_slice / _uslice: PCONV_RESAMPLE_ROWS; the host queries
 * above) reads its options when it is called.  pconv_option stores in *value what engine `e` holds for the
 * variable `name`, or with e == NULL (and for the per-call options) what a create or call made now would read;
 * PCONV_EINVAL (pconv_last_error) for an unknown name.  Values are the integers the code branches on:
 *   numbers as written (atoi): PCONV_EE_BLOCK, _PPW (<= 0: by frame count), _JOINT, _CONTIG, _XCD, _FUSE_PPW,
 *     _MFMA_WAVES, _MFMA_NT, PCONV_ENGINE_ENCODE_RANGES, PCONV_CONV1X1_STAGGER (< 0: none), PCONV_CONV_XCD,
 *     PCONV_RESAMPLE_ROWS;
 *   numbers, or PCONV_OPTION_AUTO when unset (the host plan / pconv_ee_spin_us decides): PCONV_ENGINE_GROUPS,
 *     _WORKERS, _SPIN_US, _BLOCKING_SYNC (0 / 1), _CHAIN (1 queued: anything but h..., 0 host-driven);
 *   0 / 1 switches: PCONV_ENGINE_ROWS (1 = int32), _STEPWISE_ENCODER and _TIMING (1 = set at all),
 *     _CLEAR_EVERY_CALL, _ENCODE_INTERLEAVE, _RATE_STREAMS (1 = group), PCONV_EE_BULK and _BULK0 (1 = valu),
 *     _MFMA_FORM (1 = 16x4), _MFMA_WSRC (1 = ring), _FUSE_TABLES, PCONV_CONV_SMALL (0 = off);
 *   PCONV_CONV1X1: 0 auto, 1 tiled, 2 resident; PCONV_CONV1X1_WAYOUT: 0 quads, 1 pipe, 2 batch;
 *   PCONV_ENGINE_ALLOC_FILL: -1 unset, else the byte 0 .. 255 (decimal or 0x..) that pconv_ee_create writes over every
 *     device and pinned-host buffer of a group right after allocating it (a diagnostic: no result of the engine may
 *     depend on what fresh memory held; the context / activation buffers are then zeroed by the first call as always);
 *   PCONV_ENGINE_CU_MASK=first:count is reported under the two names PCONV_ENGINE_CU_MASK_FIRST and _COUNT. */
#define PCONV_OPTION_AUTO (-2147483647 - 1)
int pconv_option(const pconv_entropy_engine *e, const char *name, int *value);
/* Explicit, process-wide opt-in: hipSetDeviceFlags(hipDeviceScheduleBlockingSync) on the current device (enable != 0),
 * then the flag is read back: returns 1 when every runtime wait on the device now sleeps, 0 when it does not (not asked
 * for, or refused by the runtime on a live context -- the engine's blocking events still apply then).  Never called by
 * the library itself. */
int pconv_device_blocking_sync(int enable);
/* symbols: device float (nimg*npart, ngroup, h, w), dead columns zero */
int pconv_ee_encode(pconv_entropy_engine *e, const float *symbols, void *stream);
/* the same in two halves: begin queues the GPU part IN `stream` and starts the host thread that
 * arithmetic-codes the frames as their tables arrive, then returns; end joins that thread.
 * `symbols` must stay alive until end.  Between the two the caller may queue other GPU work in
 * `stream` (the transforms of the next frames): it runs while the CPU codes. */
int pconv_ee_encode_begin(pconv_entropy_engine *e, const float *symbols, void *stream);
/* The last group of an encode call is evaluated in `nrange` wavefront step ranges (1 .. 8; 0 = the default: 4, or
 * PCONV_ENGINE_ENCODE_RANGES), each range's CDF rows copied to the host as soon as they exist, so that the
 * arithmetic coder starts before the GPU has finished the group.  A caller that pipelines several encode calls
 * (engine.CodecEngine.encode: chunk k is coded on the CPU under chunk k + 1's GPU work) asks for 1 on all but the
 * last: ranges re-evaluate the blocks on their boundaries.  Same streams for every value. */
int pconv_ee_set_encode_ranges(pconv_entropy_engine *e, int nrange);
int pconv_ee_encode_end(pconv_entropy_engine *e, void *stream);
/* frame `img`'s byte stream of the last encode: *nbytes bytes; whatever the engine's buffer holds beyond them is
 * undefined and must not be read. */
const uint8_t *pconv_ee_stream(const pconv_entropy_engine *e, int img, size_t *nbytes);
int pconv_ee_decode(pconv_entropy_engine *e, const uint8_t *const *streams, const size_t *nbytes,
                    float *symbols_out, void *stream);
/* Rate without coding.  For a coded symbol let c[0..8] be the integer CDF row the engine hands to the coder for it
 * (8 symbols, c[0] = 0, c[8] = 65536) and s its label.  Its CODE LENGTH is 16 - log2(c[s+1] - c[s]) bits, evaluated
 * in float64.
 *   bits_dev (nimg, npart, ngroup) float64: bits[n][tile][group] = the sum of the code lengths of the symbols of frame
 *     n, latitude tile `tile`, channel group `group`, over the positions the coder receives (the engine's schedule:
 *     pconv_ee_symbols_per_image symbols per frame; dead columns are not symbols);
 *   map_dev_or_null (nimg, npart*h, w) float32: map[n][tile*h + row][col] = the float64 sum over the groups of that
 *     position in group order 0 .. ngroup - 1, rounded once; 0 at dead positions;
 *   invalid input -- a label outside 0 .. 7, or a row whose label has zero frequency: what the coder refuses -- makes
 *     the bits entry it belongs to and its map entry NaN, and nothing else;
 *   the rate of a frame in bits per pixel is the sum of bits[n] over height * width of the frame as given (a frame
 *     padded to its coded size counts its own pixels).
 * The sums are taken in a fixed order without atomics: a frame's figures are the same bits alone, in any batch and
 * on every run.  symbols as for pconv_ee_encode.  The call is stream-ordered: it queues the encoder's network and
 * the rate kernels behind `stream` and returns; no row is stored, nothing is copied to the host, no coder runs.
 * Refused while an encode_begin is pending and for engines whose rows are not 8 symbols of total 65536. */
int pconv_ee_rate(pconv_entropy_engine *e, const float *symbols, double *bits_dev, float *map_dev_or_null, void *stream);

/* ------------------------------------------------------------------------
 * The optimiser step of training (optim.Adam, train.py --optim native): global gradient norm, clip
 * coefficient and Adam update of a list of T dense fp32 tensors in three launches.  No reference
 * counterpart: the reference calls clip_grad_norm_ and torch.optim.Adam (trainDDP_Full.py:43-47).
 * ---------------------------------------------------------------------- */

/* One record per tensor, in device memory: nine 8-byte words (the Python side builds the table as int64).  acc may be
 * NULL (no accumulator).  step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t), both computed by the
 * caller in fp64 and rounded once to fp32, t the tensor's own step count after the increment: tensors of one list
 * may differ in lr and in t. */
typedef struct pconv_optim_tensor {
  float *p;
  const float *grad;
  float *acc;
  float *m;
  float *v;
  long long n;
  float step_size, bc2_sqrt, eps, one_minus_beta1, beta2, one_minus_beta2;
} pconv_optim_tensor;

/* THE ORDER of the optimiser step.
 *
 *   segments  Tensor t is cut into segments of 4096 elements, the last may be shorter; segments are numbered
 *             tensor-ascending, then offset-ascending.  A quad is four consecutive elements of a segment, the last
 *             may be short.  The segment table holds two int32 per segment: (tensor, segment within the tensor).
 *   gradient  g = grad where the tensor has no accumulator, else g = acc + grad, one fp32 rounding (__fadd_rn):
 *             what AccGrad.copy_back leaves in grad.
 *   sqnorm    (1) per segment, lane l of 256 adds (double)g * (double)g to one fp64 accumulator, from +0: quads
 *             q = l, l + 256, ... ascending, the elements of a quad ascending;  (2) the tree  for s = 128, 64, ..., 1:
 *             a[l] = a[l] + a[l + s] for l < s  leaves the segment's partial in a[0];  (3) one closing workgroup adds
 *             the partials in the same shape: lane l takes partials l, l + 256, ... ascending from +0, then the tree:
 *             `total`;  (4) norm = sqrt(total) in fp64;  (5) coef = 1 when clip <= 0, else
 *             min(1, clip / (norm + 1e-6)) in fp64 (clip_grad_norm_'s formula), rounded once to fp32.  A NaN norm gives
 *             a NaN coef (the minimum does not drop it), an infinite norm coef 0.
 *   adam      element-wise, fp32, every operation rounded on its own (nothing contracted), / and sqrt correctly
 *             rounded:
 *               g   = g * coef
 *               m'  = m + one_minus_beta1 * (g - m)
 *               v'  = (beta2 * v) + one_minus_beta2 * (g * g)
 *               den = sqrtf(v') / bc2_sqrt + eps
 *               p'  = p - step_size * (m' / den)
 *               acc = +0                                   (where the tensor has an accumulator)
 *             grad is not written.
 * The result of a tensor does not depend on the grid or, with clip <= 0, on the other tensors of the list.  The quad
 * mapping lets a tensor whose pointers are all 16-byte aligned move as 16-byte accesses; any other takes 4-byte
 * accesses in the same order.
 *
 * Workspace (device memory of pconv_optim_workspace_bytes bytes): double total at byte 0, double norm at byte 8,
 * float coef at byte 16, the segment partials (double) from byte 32.  They stay on the device; nothing is copied to
 * the host and no call synchronises.  The entry points allocate nothing and are stream-ordered. */

/* The segment table of tensors of counts[t] elements (host): returns the number of segments and, where `segments` is
 * not NULL, writes 2 int32 per segment.  Refuses -- before it writes -- a NULL counts, ntensor < 1, a negative count
 * and more than 2^31 - 1 segments. */
long long pconv_host_optim_segments(const long long *counts, int ntensor, int32_t *segments);
long long pconv_optim_workspace_bytes(int ntensor, int nsegment);
/* records (ntensor) and segments (2 * nsegment int32) are device tables, counts (ntensor) the host array the segment
 * table was built from.  pconv_optim_sqnorm: steps (1) - (5) into the workspace.  pconv_optim_adam: the update, with
 * the coef the workspace holds.  Both return PCONV_EINVAL before anything is written or launched for a NULL pointer,
 * ntensor or nsegment < 1, a negative count, or counts that do not give nsegment segments. */
int pconv_optim_sqnorm(const pconv_optim_tensor *records, const int32_t *segments, const long long *counts,
                       int ntensor, int nsegment, float clip, void *workspace, void *stream);
int pconv_optim_adam(const pconv_optim_tensor *records, const int32_t *segments, const long long *counts,
                     int ntensor, int nsegment, const void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PCONV_HIP_H */
