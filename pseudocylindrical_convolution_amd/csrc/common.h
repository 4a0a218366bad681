// Shared helpers of libpconv_hip.so: error reporting and launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include "../../include/pconv_hip.h"

void pconv_set_error(const char *fmt, ...);

#define PCONV_REQUIRE(cond, ...)     \
  do {                               \
    if (!(cond)) {                   \
      pconv_set_error(__VA_ARGS__);  \
      return PCONV_EINVAL;           \
    }                                \
  } while (0)

#define PCONV_LAUNCH_CHECK(name)                                          \
  do {                                                                    \
    hipError_t e__ = hipGetLastError();                                   \
    if (e__ != hipSuccess) {                                              \
      pconv_set_error("%s: %s", name, hipGetErrorString(e__));            \
      return PCONV_ELAUNCH;                                               \
    }                                                                     \
  } while (0)

// MI355X: 256 CUs.  Memory-bound grid-stride kernels are capped at 8 blocks of
// 256 threads per CU so the grid stays resident and the tail is short.
static inline unsigned pconv_grid(long long work_items, int block = 256) {
  long long blocks = (work_items + block - 1) / block;
  const long long cap = 256LL * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

static inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }

// pointwise.hip: the suffix sum over the quantiser's level bins, shared by both forms of its backward
int pconv_launch_quant_weight_grad(const float *bins, const float *tab, float *g_w, int c, int levels, hipStream_t stream);

// The dynamic-LDS limit is a per-device attribute of the function: raise it once on every device
// this process launches `kernel` on (one process may drive several GPUs: nn.DataParallel replicas
// of BaseOpModule).  `raised` is the caller's static mask of that kernel instantiation, one bit
// per device; `what` prefixes the error text.
template <typename Kernel>
static inline int pconv_raise_lds(Kernel kernel, size_t bytes, std::atomic<unsigned long long> &raised, const char *what) {
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) device = 0;
  const unsigned long long bit = 1ULL << (device & 63);
  if (!(raised.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
      pconv_set_error("%s: cannot raise dynamic LDS to %zu: %s", what, bytes, hipGetErrorString(e));
      return PCONV_ELAUNCH;
    }
    raised.fetch_or(bit, std::memory_order_release);
  }
  return PCONV_OK;
}
