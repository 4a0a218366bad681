// Backward of the dense per-tile convolution (conv.hip) in a defined order: the data gradient, the weight
// gradient and the bias gradient of pconv_conv2d's layers (k in {1, 3}, stride in {1, 2}) and of pconv_conv5's (the
// masked 5x5 stride-1 convolutions of the entropy model); no padding, dense NCHW fp32.  No atomics, no allocation and
// no memset: what a call needs comes from the caller as a workspace.  The orders are part of the contract
// (include/pconv_hip.h) and the CPU twin of the tests restates them.  The two families have entry points of their own
// (pconv_conv2d_* / pconv_conv_*, pconv_conv5_*): each checks the (k, stride) it accepts and calls the one host
// routine of its step (run_*), which takes k and stride as arguments.
//
//   data gradient    = the forward convolution, stride 1, of the PREPARED output gradient (zero-stuffed to the
//                      stride, padded by k - 1) with the flipped, transposed weights.  New here: the transposed pack
//                      and the prepare kernel; the convolution itself is conv.hip's (pconv_conv2d, at k = 5
//                      pconv_conv5), so every gin element is one fmaf chain from +0 over (co, kh', kw') ascending.
//   weight gradient  = per tile t a GEMM over the tile's pixels on v_mfma_f32_32x32x2_f32:
//                        P_t[co][n] = sum_p gout[t][co][p] * in[t][ci][s y + kh][s x + kw],  n = (ci*k + kh)*k + kw
//                      M = couts (A operand), N = the (ci, kh, kw) columns (B operand, gathered from an LDS patch of
//                      input rows), K = the pixels p = (y, x), y ascending then x ascending.  A workgroup of four
//                      waves owns (t, 96 couts, 128 columns); a wave three accumulators of 32 x 32: all 96 couts of
//                      32 columns (96 divides the codec's 96 / 192 / 768 couts, and two workgroups fit a CU's LDS on
//                      the 3x3 stride-1 layers).  The pixels come
//                      in chunks of up to 64 of one output row; per chunk the gout slab [96][64] and the input patch
//                      go to LDS by LDS-DMA (global_load_lds, double buffered: the next chunk's DMA is issued in front
//                      of the chunk's matrix loop), and the chunks continue the chain in the same accumulators.  A
//                      chunk of odd length ends with one step whose product is -0 (A = -0, B = +0):
//                      fmaf(-0, +0, acc) = acc for EVERY acc, -0 and NaN included, so the pad is not part of the
//                      arithmetic.  Then a second kernel adds the partials, t ascending.  At k = 5 the patch is 5 input
//                      rows of 68 (+ 1: bank spread) columns for each of the <= 7 channels that 128 consecutive
//                      (ci, kh, kw) columns of 25 taps touch, 35 KB per stage.
//   bias gradient    = the fixed-shape two-stage fp64 reduction of quant_backward_ordered_kernel.
#include "conv_host.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_ptr_t;
typedef const __attribute__((address_space(1))) void glb_ptr_t;
typedef const __attribute__((address_space(1))) char glb_bytes_t;

constexpr int kBlock = 256;

// ---- data gradient: transposed pack and the prepared gradient -------------------------------------------------

// w (cout, cin, k, k) -> the [red_pad][cout_pad] slab pconv_conv_pack_weight would write for
// wT[ci][co][kh'][kw'] = w[co][ci][k-1-kh'][k-1-kw']: reduction entry kk = (co*k + kh')*k + kw', row ci
__global__ void pack_weight_transposed_kernel(const float *__restrict__ w, float *__restrict__ packed, int cout, int cin,
                                              int k, int row_pad, int red_pad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= row_pad * red_pad) return;
  const int ci = i % row_pad, kk = i / row_pad;
  float v = 0.f;
  if (ci < cin && kk < cout * k * k) {
    const int kw = kk % k, kh = (kk / k) % k, co = kk / (k * k);
    v = w[(((size_t)co * cin + ci) * k + (k - 1 - kh)) * k + (k - 1 - kw)];
  }
  packed[i] = v;
}

// prepared (planes, hp, wp): element (y, x) of a gout plane at (k-1 + s y, k-1 + s x), +0 everywhere else.  One
// pass, four consecutive floats per lane and store.
__global__ __launch_bounds__(kBlock) void conv_grad_prepare_kernel(const float *__restrict__ gout,
                                                                    float *__restrict__ prepared, long long total,
                                                                    int hp, int wp, int ho, int wo, int k, int s) {
  const long long quads = (total + 3) / 4;
  for (long long q = (long long)blockIdx.x * kBlock + threadIdx.x; q < quads; q += (long long)gridDim.x * kBlock) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const long long i = q * 4 + j;
      v[j] = 0.f;
      if (i < total) {
        const int X = (int)(i % wp) - (k - 1), Y = (int)((i / wp) % hp) - (k - 1);
        const long long plane = i / ((long long)wp * hp);
        if (X >= 0 && Y >= 0 && X % s == 0 && Y % s == 0 && X / s < wo && Y / s < ho)
          v[j] = gout[(size_t)plane * ho * wo + (size_t)(Y / s) * wo + X / s];
      }
    }
    if (q * 4 + 3 < total) {
      *reinterpret_cast<float4 *>(prepared + q * 4) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
      for (int j = 0; q * 4 + j < total; j++) prepared[q * 4 + j] = v[j];
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------

constexpr int kSeg = 64;          // pixels of one output row per chunk
constexpr int kMT = 3;            // 32 x 32 accumulators of a wave, along the couts
constexpr int kBM = 32 * kMT;     // couts per workgroup: 96 divides the codec's 96 / 192 / 768 without a remainder
constexpr int kBN = 128;          // (ci, kh, kw) columns per workgroup: 32 per wave
constexpr int kAStride = kSeg + 1;  // LDS row of the gout slab: lane = cout reads bank (cout + pixel) % 64

template <int KS, int S>
struct WgradCfg {
  static constexpr int KK = KS * KS;
  // sampling step of the staged patch (a strided 1x1 only needs every S-th pixel), as conv.hip's Patch
  static constexpr int PS = (KS == 1) ? S : 1;
  static constexpr int Q = S / PS;  // LDS step between neighbouring output pixels
  static constexpr int PC = (kSeg - 1) * Q + KS;
  // patch row in LDS: the next length that is KS modulo 64 (1 for 1x1, 3 for 3x3, 5 for 5x5), so that the 32 columns
  // a half wave reads -- consecutive n = (ci*KS + kh)*KS + kw, at (ci*KS + kh) * PCS + kw -- fall into 32 different banks
  static constexpr int PCS = (KS == 1) ? PC + 1 : PC + (S == 1 ? 1 : 2);
  static constexpr int NCI = (KS == 1) ? kBN : (kBN - 1) / KK + 2;  // input channels 128 consecutive columns can touch
  static constexpr int ASZ = kBM * kAStride;
  static constexpr int BOFF = (ASZ + 63) / 64 * 64;  // the patch starts on a wave's 64-dword boundary
  static constexpr int BSZ = NCI * KS * PCS;
  static constexpr int STAGE = BOFF + (BSZ + 63) / 64 * 64;
  static constexpr int ALD = (ASZ + kBlock - 1) / kBlock;  // LDS-DMA dwords per thread
  static constexpr int BLD = (BSZ + kBlock - 1) / kBlock;
  static_assert(PCS >= PC && PCS % 64 == KS, "patch rows spread the columns over the banks");
  static_assert(2 * STAGE * 4 <= 160 * 1024, "two stages fit the CU's LDS");
  // workgroups per CU the kernel is compiled for: two where two stage pairs fit the LDS (the 3x3 and 5x5 stride-1 layers)
  static constexpr int WGS = (2 * 2 * STAGE * 4 <= 160 * 1024) ? 2 : 1;
};

__device__ __forceinline__ float wg_lds_read(unsigned addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}

// partial (tn, cout, cin*KS*KS): the tile's chain, see the head of the file
template <int KS, int S>
__global__ __launch_bounds__(kBlock, (WgradCfg<KS, S>::WGS)) void conv_wgrad_kernel(
    const float *__restrict__ in, const float *__restrict__ gout, float *__restrict__ partial, int cin, int h, int w,
    int cout, int ho, int wo, int nblocks, int cblocks) {
  using C = WgradCfg<KS, S>;
  extern __shared__ float lds[];
  int b = blockIdx.x;
  const int nb = b % nblocks;
  b /= nblocks;
  const int cb = b % cblocks;
  const int t = b / cblocks;
  const int ncol = cin * C::KK;
  const int n0 = nb * kBN, cout0 = cb * kBM, ci0 = n0 / C::KK;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // (uniform: LDS-DMA bases stay in scalar registers)
  const int l31 = lane & 31, half = lane >> 5;

  // uniform 64-bit bases + a 32-bit byte offset per lane (the host checks that a block's span fits)
  const float *gt = gout + ((size_t)t * cout + cout0) * ho * wo;
  const float *it = in + ((size_t)t * cin + ci0) * h * w;

  // chunk-invariant parts of the DMA sources.  Couts past cout / channels past cin read the last real one: they
  // only reach accumulator rows / columns that are never stored.
  unsigned arow[C::ALD], brow[C::BLD];
  int apx[C::ALD], bpc[C::BLD];
#pragma unroll
  for (int j = 0; j < C::ALD; j++) {
    int e = tid + j * kBlock;
    e = e < C::ASZ ? e : 0;
    int co = cout0 + e / kAStride;
    co = (co < cout ? co : cout - 1) - cout0;
    arow[j] = (unsigned)co * (unsigned)(ho * wo);
    apx[j] = e % kAStride;
  }
#pragma unroll
  for (int j = 0; j < C::BLD; j++) {
    int e = tid + j * kBlock;
    e = e < C::BSZ ? e : 0;
    const int r = (e / C::PCS) % KS;
    int ci = ci0 + e / (C::PCS * KS);
    ci = (ci < cin ? ci : cin - 1) - ci0;
    brow[j] = (unsigned)ci * (unsigned)(h * w) + (unsigned)(r * w);
    bpc[j] = (e % C::PCS) * C::PS;
  }

  const int nseg = (wo + kSeg - 1) / kSeg;
  const int nchunk = ho * nseg;

  auto stage = [&](int chunk, int buf) {
    const int y = chunk / nseg, c0 = (chunk % nseg) * kSeg;
    float *as = lds + buf * C::STAGE, *bs = as + C::BOFF;
    const unsigned abase = (unsigned)(y * wo), bbase = (unsigned)(y * S * w);
#pragma unroll
    for (int j = 0; j < C::ALD; j++) {
      if (tid + j * kBlock < C::ASZ) {
        int col = c0 + apx[j];
        col = col < wo ? col : wo - 1;
        unsigned off = (arow[j] + abase + (unsigned)col) * 4u;
        asm volatile("" : "+v"(off));
        __builtin_amdgcn_global_load_lds((glb_ptr_t *)((glb_bytes_t *)gt + off), (lds_ptr_t *)(as + j * kBlock + wave * 64),
                                         4, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < C::BLD; j++) {
      if (tid + j * kBlock < C::BSZ) {
        int col = c0 * S + bpc[j];
        col = col < w ? col : w - 1;
        unsigned off = (brow[j] + bbase + (unsigned)col) * 4u;
        asm volatile("" : "+v"(off));
        __builtin_amdgcn_global_load_lds((glb_ptr_t *)((glb_bytes_t *)it + off), (lds_ptr_t *)(bs + j * kBlock + wave * 64),
                                         4, 0, 0);
      }
    }
  };

  // per-lane LDS byte addresses of the operands of pixel `half` of a chunk in buffer 0
  const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>(lds);  // low half of the flat address = LDS offset
  // (every wave reads all 96 couts of the slab and its own 32 columns of the patch)
  unsigned aaddr[kMT], baddr;
#pragma unroll
  for (int m = 0; m < kMT; m++) aaddr[m] = lds0 + (unsigned)((m * 32 + l31) * kAStride + half) * 4u;
  {
    int col = n0 + wave * 32 + l31;
    col = col < ncol ? col : ncol - 1;
    const int ci = col / C::KK - ci0, kh = (col % C::KK) / KS, kw = col % KS;
    baddr = lds0 + (unsigned)(C::BOFF + (ci * KS + kh) * C::PCS + kw + half * C::Q) * 4u;
  }

  f32x16 acc[kMT];
#pragma unroll
  for (int m = 0; m < kMT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[m][r] = 0.f;

  stage(0, 0);
  __syncthreads();  // (also waits for the DMA: vmcnt(0))

  for (int chunk = 0; chunk < nchunk; chunk++) {
    // the other buffer's last readers finished before the barrier that ended the previous iteration
    if (chunk + 1 < nchunk) stage(chunk + 1, (chunk & 1) ^ 1);
    const int c0 = (chunk % nseg) * kSeg;
    const int valid = wo - c0 < kSeg ? wo - c0 : kSeg;
    const int npair = (valid + 1) >> 1;
    const unsigned bufoff = (chunk & 1) ? (unsigned)(C::STAGE * 4) : 0u;
    static_assert(kMT == 3, "the operand reads are written out for three cout tiles");
    float an[kMT], bn;  // the operands of the next pixel pair, read while this pair's MFMAs run
    an[0] = wg_lds_read(aaddr[0] + bufoff), an[1] = wg_lds_read(aaddr[1] + bufoff), an[2] = wg_lds_read(aaddr[2] + bufoff);
    bn = wg_lds_read(baddr + bufoff);
    for (int j = 0; j < npair; j++) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(an[0]), "+v"(an[1]), "+v"(an[2]), "+v"(bn));
      float a[kMT] = {an[0], an[1], an[2]}, bb = bn;
      if (j + 1 < npair) {
        const unsigned ao = bufoff + (unsigned)(j + 1) * 8u, bo = bufoff + (unsigned)(j + 1) * (unsigned)(8 * C::Q);
        an[0] = wg_lds_read(aaddr[0] + ao), an[1] = wg_lds_read(aaddr[1] + ao), an[2] = wg_lds_read(aaddr[2] + ao);
        bn = wg_lds_read(baddr + bo);
      }
      if (half && 2 * j + 1 >= valid) {
        // the pad step of an odd chunk: product -0, which leaves every accumulator as it is
        a[0] = a[1] = a[2] = __int_as_float((int)0x80000000u);
        bb = 0.f;
      }
#pragma unroll
      for (int m = 0; m < kMT; m++) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], bb, acc[m], 0, 0, 0);
    }
    __syncthreads();
  }

  // reg r of a 32 x 32 tile: cout row (r&3) + 8*(r>>2) + 4*half, column l31
  float *pt = partial + (size_t)t * cout * ncol;
  const int col = n0 + wave * 32 + l31;
#pragma unroll
  for (int m = 0; m < kMT; m++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int co = cout0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      if (co < cout && col < ncol) pt[(size_t)co * ncol + col] = acc[m][r];
    }
}

// gw = (((P_0 + P_1) + P_2) + ...), fp32 round-to-nearest adds, t ascending
__global__ __launch_bounds__(kBlock) void conv_wgrad_sum_kernel(const float *__restrict__ partial, float *__restrict__ gw,
                                                                 int tn, long long n) {
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
    float acc = partial[i];
    for (int t = 1; t < tn; t++) acc = __fadd_rn(acc, partial[(size_t)t * n + i]);
    gw[i] = acc;
  }
}

// ---- bias gradient ------------------------------------------------------------------------------------------------

// stage one: one workgroup per (t, co) plane; lane l adds the elements l, l + 256, ... of the plane, ascending, in
// fp64 from +0; then the tree a[l] += a[l + s], s = 128 ... 1.  partials: (tn, cout) fp64.
__global__ __launch_bounds__(kBlock) void conv_bgrad_plane_kernel(const float *__restrict__ gout, double *__restrict__ partials,
                                                                   long long hw, long long nplanes) {
  __shared__ double sums[kBlock];
  for (long long plane = blockIdx.x; plane < nplanes; plane += gridDim.x) {
    const float *g = gout + (size_t)plane * hw;
    double a = 0.0;
    for (long long e = threadIdx.x; e < hw; e += kBlock) a = __dadd_rn(a, (double)g[e]);
    __syncthreads();  // (the previous plane's tree has been read)
    sums[threadIdx.x] = a;
    for (int s = kBlock / 2; s > 0; s >>= 1) {
      __syncthreads();
      if (threadIdx.x < s) sums[threadIdx.x] = __dadd_rn(sums[threadIdx.x], sums[threadIdx.x + s]);
    }
    if (threadIdx.x == 0) partials[plane] = sums[0];
  }
}

// stage two: the planes of a cout, t ascending, in fp64 from +0; one rounding to fp32
__global__ __launch_bounds__(kBlock) void conv_bgrad_sum_kernel(const double *__restrict__ partials, float *__restrict__ gb,
                                                                 int tn, int cout) {
  const int co = blockIdx.x * kBlock + threadIdx.x;
  if (co >= cout) return;
  double acc = 0.0;
  for (int t = 0; t < tn; t++) acc = __dadd_rn(acc, partials[(size_t)t * cout + co]);
  gb[co] = (float)acc;
}

template <int KS, int S>
int launch_wgrad(const float *in, const float *gout, float *partial, int tn, int cin, int h, int w, int cout, int ho,
                 int wo, hipStream_t stream) {
  using C = WgradCfg<KS, S>;
  const int nblocks = (cin * C::KK + kBN - 1) / kBN, cblocks = (cout + kBM - 1) / kBM;
  const long long grid = (long long)tn * nblocks * cblocks;
  PCONV_REQUIRE(grid > 0 && grid <= 0x7fffffffLL, "conv2d_wgrad: grid %lld out of range", grid);
  const size_t smem = (size_t)2 * C::STAGE * sizeof(float);
  auto kern = conv_wgrad_kernel<KS, S>;
  static std::atomic<unsigned long long> raised{0};
  if (int rc = pconv_raise_lds(kern, smem, raised, "conv2d_wgrad")) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(kBlock), smem, stream, in, gout, partial, cin, h, w, cout, ho, wo,
                     nblocks, cblocks);
  return PCONV_OK;
}

// ---- host: one routine per step, for every (k, stride) -------------------------------------------------------------
// An entry point (at the end of the file) checks the shape against the kernel sizes and strides IT accepts, then calls
// the routine of its step with its own name `what` for the messages.  The routines make every other check -- pointers,
// alignment, the int32 ranges -- so that a check exists once, for both families.

constexpr int kK5 = 5;  // the kernel size of the pconv_conv5_* entries (their stride is 1)
constexpr unsigned kSizes13 = (1u << 1) | (1u << 3), kSize5 = 1u << kK5;  // sets of kernel sizes: bit k

// ksizes: the kernel sizes the caller accepts; stride in {1, 2} (the 5x5 entries pass their 1)
inline bool conv_shape_ok(unsigned ksizes, int tn, int cin, int h, int w, int cout, int k, int stride) {
  return tn > 0 && cin > 0 && cout > 0 && k > 0 && k < 32 && ((ksizes >> k) & 1) && h >= k && w >= k &&
         (stride == 1 || stride == 2);
}

inline bool fits_int32(long long v) { return v >= 0 && v <= 0x7fffffffLL; }

inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

int run_pack_transposed(const char *what, const float *w, float *packed, int cout, int cin, int k, void *stream) {
  PCONV_REQUIRE(w && packed, "%s: null pointer", what);
  int rowp, redp;  // the transposed layer has cin output and cout input channels
  const long long total = pconv_conv_packed_floats(cin, cout, k, &rowp, &redp);
  PCONV_REQUIRE(fits_int32(total), "%s: weight exceeds int32", what);
  hipLaunchKernelGGL(pack_weight_transposed_kernel, dim3(((int)total + kBlock - 1) / kBlock), dim3(kBlock), 0,
                     as_stream(stream), w, packed, cout, cin, k, rowp, redp);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

long long dgrad_workspace_bytes(int tn, int cout, int h, int w, int k, int stride) {
  if (k == 1 && stride == 1) return 0;  // the prepared gradient is gout itself
  return (long long)tn * cout * (h + k - 1) * (w + k - 1) * (long long)sizeof(float);
}

int run_prepare(const char *what, const float *gout, float *prepared, int tn, int cout, int h, int w, int k, int stride,
                void *stream) {
  PCONV_REQUIRE(gout && prepared, "%s: null pointer", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 15) == 0, "%s: the prepared gradient must be 16-byte aligned", what);
  const int ho = (h - k) / stride + 1, wo = (w - k) / stride + 1, hp = h + k - 1, wp = w + k - 1;
  PCONV_REQUIRE(fits_int32((long long)hp * wp) && fits_int32((long long)tn * cout), "%s: plane exceeds int32", what);
  const long long total = (long long)tn * cout * hp * wp;
  hipLaunchKernelGGL(conv_grad_prepare_kernel, dim3(pconv_grid((total + 3) / 4, kBlock)), dim3(kBlock), 0, as_stream(stream),
                     gout, prepared, total, hp, wp, ho, wo, k, stride);
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

int run_dgrad(const char *what, const float *gout, const float *packed_wt, float *gin, void *workspace, int tn, int cin, int h,
              int w, int cout, int k, int stride, void *stream) {
  PCONV_REQUIRE(gout && packed_wt && gin, "%s: null pointer", what);
  PCONV_REQUIRE(fits_int32((long long)tn * cin) && fits_int32((long long)cout * cin * k * k), "%s: shape exceeds int32", what);
  const float *prepared = gout;
  if (k != 1 || stride != 1) {
    PCONV_REQUIRE(workspace, "%s: null workspace", what);
    if (int rc = run_prepare(what, gout, static_cast<float *>(workspace), tn, cout, h, w, k, stride, stream)) return rc;
    prepared = static_cast<const float *>(workspace);
  }
  // (tn, cout, h + k - 1, w + k - 1) * wT (cin, cout, k, k), stride 1 -> (tn, cin, h, w)
  if (k == 5) return pconv_conv5(prepared, packed_wt, nullptr, gin, tn, cout, h + k - 1, w + k - 1, cin, stream);
  return pconv_conv2d(prepared, packed_wt, nullptr, gin, tn, cout, h + k - 1, w + k - 1, cin, k, 1, 0, nullptr, nullptr, 0,
                      nullptr, nullptr, 0, 0, nullptr, stream);
}

long long wgrad_workspace_bytes(int tn, int cin, int cout, int k) {
  // the partials P_t (tn, cout, cin, k, k) fp32, then the bias planes (tn, cout) fp64
  return align_up((long long)tn * cout * cin * k * k * (long long)sizeof(float), 16) + (long long)tn * cout * (long long)sizeof(double);
}

// the weight and bias gradient: checks that depend on the sizes alone, then the launches
int run_wgrad(const char *what, const float *in, const float *gout, float *gw, float *gb, void *workspace, int tn, int cin,
              int h, int w, int cout, int k, int stride, void *stream) {
  PCONV_REQUIRE(gout && (gw || gb) && (in || !gw), "%s: null pointer", what);
  PCONV_REQUIRE(workspace, "%s: null workspace", what);
  PCONV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: the workspace must be 16-byte aligned", what);
  const int ho = (h - k) / stride + 1, wo = (w - k) / stride + 1;
  const long long ncol = (long long)cin * k * k, nw = (long long)cout * ncol;
  PCONV_REQUIRE(fits_int32(nw) && fits_int32((long long)h * w) && fits_int32((long long)tn * cout), "%s: shape exceeds int32",
                what);
  // a workgroup addresses its 96 couts of gout / its <= 128 channels of the input as a 64-bit uniform base + a
  // 32-bit byte offset per lane
  PCONV_REQUIRE((long long)kBM * ho * wo * 4 < (1LL << 32) && (long long)kBN * h * w * 4 < (1LL << 32),
                "%s: plane too large for 32-bit byte offsets inside a block", what);
  hipStream_t s = as_stream(stream);
  float *partial = static_cast<float *>(workspace);
  // (without gw there are no partials: the planes start the workspace)
  double *planes = reinterpret_cast<double *>(static_cast<char *>(workspace) + (gw ? align_up(tn * nw * (long long)sizeof(float), 16) : 0));
  if (gw) {
    int rc;
    if (k == 5)
      rc = launch_wgrad<5, 1>(in, gout, partial, tn, cin, h, w, cout, ho, wo, s);
    else if (k == 3 && stride == 1)
      rc = launch_wgrad<3, 1>(in, gout, partial, tn, cin, h, w, cout, ho, wo, s);
    else if (k == 3)
      rc = launch_wgrad<3, 2>(in, gout, partial, tn, cin, h, w, cout, ho, wo, s);
    else if (stride == 1)
      rc = launch_wgrad<1, 1>(in, gout, partial, tn, cin, h, w, cout, ho, wo, s);
    else
      rc = launch_wgrad<1, 2>(in, gout, partial, tn, cin, h, w, cout, ho, wo, s);
    if (rc != PCONV_OK) return rc;
    hipLaunchKernelGGL(conv_wgrad_sum_kernel, dim3(pconv_grid(nw, kBlock)), dim3(kBlock), 0, s, partial, gw, tn, nw);
  }
  if (gb) {
    const long long nplanes = (long long)tn * cout;
    const unsigned grid = (unsigned)(nplanes < 256 * 16 ? nplanes : 256 * 16);
    hipLaunchKernelGGL(conv_bgrad_plane_kernel, dim3(grid), dim3(kBlock), 0, s, gout, planes, (long long)ho * wo, nplanes);
    hipLaunchKernelGGL(conv_bgrad_sum_kernel, dim3((cout + kBlock - 1) / kBlock), dim3(kBlock), 0, s, planes, gb, tn, cout);
  }
  PCONV_LAUNCH_CHECK(what);
  return PCONV_OK;
}

}  // namespace

// ---- entry points: k in {1, 3}, stride in {1, 2} -------------------------------------------------------------------

extern "C" int pconv_conv_pack_weight_transposed(const float *w, float *packed, int cout, int cin, int k, void *stream) {
  PCONV_REQUIRE(cout > 0 && cin > 0 && (k == 1 || k == 3), "conv_pack_weight_transposed: bad argument");
  return run_pack_transposed("conv_pack_weight_transposed", w, packed, cout, cin, k, stream);
}

extern "C" long long pconv_conv2d_dgrad_workspace_bytes(int tn, int cout, int h, int w, int k, int stride) {
  PCONV_REQUIRE(conv_shape_ok(kSizes13, tn, 1, h, w, cout, k, stride), "conv2d_dgrad_workspace_bytes: bad shape");
  return dgrad_workspace_bytes(tn, cout, h, w, k, stride);
}

extern "C" int pconv_conv_grad_prepare(const float *gout, float *prepared, int tn, int cout, int h, int w, int k,
                                       int stride, void *stream) {
  PCONV_REQUIRE(conv_shape_ok(kSizes13, tn, 1, h, w, cout, k, stride), "conv_grad_prepare: unsupported k=%d stride=%d or bad shape",
                k, stride);
  return run_prepare("conv_grad_prepare", gout, prepared, tn, cout, h, w, k, stride, stream);
}

extern "C" int pconv_conv2d_dgrad(const float *gout, const float *packed_wt, float *gin, void *workspace, int tn, int cin,
                                  int h, int w, int cout, int k, int stride, void *stream) {
  PCONV_REQUIRE(conv_shape_ok(kSizes13, tn, cin, h, w, cout, k, stride), "conv2d_dgrad: unsupported k=%d stride=%d or bad shape",
                k, stride);
  return run_dgrad("conv2d_dgrad", gout, packed_wt, gin, workspace, tn, cin, h, w, cout, k, stride, stream);
}

extern "C" long long pconv_conv2d_wgrad_workspace_bytes(int tn, int cin, int cout, int k) {
  PCONV_REQUIRE(conv_shape_ok(kSizes13, tn, cin, k, k, cout, k, 1), "conv2d_wgrad_workspace_bytes: bad shape");
  return wgrad_workspace_bytes(tn, cin, cout, k);
}

extern "C" int pconv_conv2d_wgrad(const float *in, const float *gout, float *gw, float *gb, void *workspace, int tn,
                                  int cin, int h, int w, int cout, int k, int stride, void *stream) {
  PCONV_REQUIRE(conv_shape_ok(kSizes13, tn, cin, h, w, cout, k, stride), "conv2d_wgrad: unsupported k=%d stride=%d or bad shape",
                k, stride);
  return run_wgrad("conv2d_wgrad", in, gout, gw, gb, workspace, tn, cin, h, w, cout, k, stride, stream);
}

// ---- entry points: 5x5, stride 1 (the masked convolutions of the entropy model) ------------------------------------

extern "C" int pconv_conv5_pack_weight_transposed(const float *w, float *packed, int cout, int cin, void *stream) {
  PCONV_REQUIRE(cout > 0 && cin > 0, "conv5_pack_weight_transposed: bad shape");
  return run_pack_transposed("conv5_pack_weight_transposed", w, packed, cout, cin, kK5, stream);
}

extern "C" long long pconv_conv5_dgrad_workspace_bytes(int tn, int cout, int h, int w) {
  PCONV_REQUIRE(conv_shape_ok(kSize5, tn, 1, h, w, cout, kK5, 1), "conv5_dgrad_workspace_bytes: bad shape");
  return dgrad_workspace_bytes(tn, cout, h, w, kK5, 1);
}

extern "C" int pconv_conv5_dgrad(const float *gout, const float *packed_wt, float *gin, void *workspace, int tn, int cin,
                                 int h, int w, int cout, void *stream) {
  PCONV_REQUIRE(conv_shape_ok(kSize5, tn, cin, h, w, cout, kK5, 1), "conv5_dgrad: bad shape (%d, %d, %d, %d) -> %d: h and w >= 5",
                tn, cin, h, w, cout);
  return run_dgrad("conv5_dgrad", gout, packed_wt, gin, workspace, tn, cin, h, w, cout, kK5, 1, stream);
}

extern "C" long long pconv_conv5_wgrad_workspace_bytes(int tn, int cin, int cout) {
  PCONV_REQUIRE(conv_shape_ok(kSize5, tn, cin, kK5, kK5, cout, kK5, 1), "conv5_wgrad_workspace_bytes: bad shape");
  return wgrad_workspace_bytes(tn, cin, cout, kK5);
}

extern "C" int pconv_conv5_wgrad(const float *in, const float *gout, float *gw, float *gb, void *workspace, int tn, int cin,
                                 int h, int w, int cout, void *stream) {
  PCONV_REQUIRE(conv_shape_ok(kSize5, tn, cin, h, w, cout, kK5, 1), "conv5_wgrad: bad shape (%d, %d, %d, %d) -> %d: h and w >= 5",
                tn, cin, h, w, cout);
  return run_wgrad("conv5_wgrad", in, gout, gw, gb, workspace, tn, cin, h, w, cout, kK5, 1, stream);
}
