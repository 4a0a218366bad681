// TEST INFRASTRUCTURE -- stand-in for the CUDA runtime header, so that the reference's extension/*.cu compile as
// ordinary C++ for the CPU (oracle/ref_ops.py).  A kernel is a plain function that runs as the only thread of the
// only block: every kernel but the masked convolution is a grid-stride loop, which one thread walks in index order.
// Atomics are serial; the few cuBLAS calls are plain loops.  The masked convolution's kernels need 128 cooperating
// threads (shared memory, __syncthreads, warp shuffles): its file alone is compiled with -DSHIM_COOPERATIVE and
// gets per-thread indices, a warp of 32, a real barrier and a real shuffle from coop_launch.h instead.
#pragma once
#include <algorithm>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __inline__ inline
#define __shared__
#ifdef SHIM_COOPERATIVE
// blocks of cooperating threads; the dynamic shared array "extern __shared__ int __smem[]" is the launcher's
#include "coop_launch.h"
extern int __smem[];
#else
// Dynamic shared memory, "extern __shared__ int __smem[]" inside a function of the masked convolution's file: in a
// one-thread file an extern array that nobody reads.  Declared weak at namespace scope first (a block-scope
// declaration cannot carry the attribute).
extern int __smem[] __attribute__((weak));

struct shim_dim3 { unsigned x, y, z; };
static const shim_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
static const int warpSize = 1;
inline void __syncthreads() {}
template <class T> inline T __shfl_down_sync(unsigned, T v, int) { return v; }
#endif

typedef void *cudaStream_t;
typedef void *cudaEvent_t;
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaMemcpyDefault };
inline cudaError_t cudaGetLastError() { return cudaSuccess; }
inline const char *cudaGetErrorString(cudaError_t) { return "cpu shim"; }
inline cudaError_t cudaMemset(void *p, int v, size_t n) { memset(p, v, n); return cudaSuccess; }
inline cudaError_t cudaMemcpy(void *d, const void *s, size_t n, int) { memmove(d, s, n); return cudaSuccess; }
inline cudaError_t cudaSetDevice(int) { return cudaSuccess; }
inline cudaError_t cudaEventCreate(cudaEvent_t *e) { *e = nullptr; return cudaSuccess; }
inline cudaError_t cudaEventRecord(cudaEvent_t, int) { return cudaSuccess; }
inline cudaError_t cudaEventSynchronize(cudaEvent_t) { return cudaSuccess; }
inline cudaError_t cudaEventElapsedTime(float *ms, cudaEvent_t, cudaEvent_t) { *ms = 0; return cudaSuccess; }

// CUDA's atomicAdd is an overload set, not a template: a call such as atomicAdd(float *, 1.) converts the addend
inline int atomicAdd(int *p, int v) { int o = *p; *p = o + v; return o; }
inline unsigned atomicAdd(unsigned *p, unsigned v) { unsigned o = *p; *p = o + v; return o; }
inline float atomicAdd(float *p, float v) { float o = *p; *p = o + v; return o; }
inline double atomicAdd(double *p, double v) { double o = *p; *p = o + v; return o; }

typedef void *cublasHandle_t;
typedef int cublasStatus_t;
enum { CUBLAS_STATUS_SUCCESS = 0, CUBLAS_STATUS_NOT_INITIALIZED, CUBLAS_STATUS_ALLOC_FAILED, CUBLAS_STATUS_INVALID_VALUE,
       CUBLAS_STATUS_ARCH_MISMATCH, CUBLAS_STATUS_MAPPING_ERROR, CUBLAS_STATUS_EXECUTION_FAILED,
       CUBLAS_STATUS_INTERNAL_ERROR, CUBLAS_STATUS_NOT_SUPPORTED, CUBLAS_STATUS_LICENSE_ERROR };
enum cublasOperation_t { CUBLAS_OP_N, CUBLAS_OP_T, CUBLAS_OP_C };
inline cublasStatus_t cublasCreate(cublasHandle_t *h) { *h = nullptr; return CUBLAS_STATUS_SUCCESS; }
inline cublasStatus_t cublasSetStream(cublasHandle_t, cudaStream_t) { return CUBLAS_STATUS_SUCCESS; }
template <class T> inline cublasStatus_t shim_dot(int n, const T *x, const T *y, T *out) {
  T s = 0;
  for (int i = 0; i < n; i++) s += x[i] * y[i];
  *out = s;
  return CUBLAS_STATUS_SUCCESS;
}
// column-major A (m x n, leading dimension lda), y = a op(A) x + b y
template <class T> inline cublasStatus_t shim_gemv(cublasOperation_t op, int m, int n, T a, const T *A, int lda, const T *x, T b, T *y) {
  const bool plain = op == CUBLAS_OP_N;
  const int ny = plain ? m : n, nx = plain ? n : m;
  for (int i = 0; i < ny; i++) {
    T s = 0;
    for (int j = 0; j < nx; j++) s += (plain ? A[i + (size_t)j * lda] : A[j + (size_t)i * lda]) * x[j];
    y[i] = a * s + b * y[i];
  }
  return CUBLAS_STATUS_SUCCESS;
}
inline cublasStatus_t cublasSdot(cublasHandle_t, int n, const float *x, int, const float *y, int, float *o) { return shim_dot(n, x, y, o); }
inline cublasStatus_t cublasDdot(cublasHandle_t, int n, const double *x, int, const double *y, int, double *o) { return shim_dot(n, x, y, o); }
inline cublasStatus_t cublasSgemv(cublasHandle_t, cublasOperation_t t, int m, int n, const float *a, const float *A, int lda, const float *x, int, const float *b, float *y, int) { return shim_gemv(t, m, n, *a, A, lda, x, *b, y); }
inline cublasStatus_t cublasDgemv(cublasHandle_t, cublasOperation_t t, int m, int n, const double *a, const double *A, int lda, const double *x, int, const double *b, double *y, int) { return shim_gemv(t, m, n, *a, A, lda, x, *b, y); }
inline cublasStatus_t cublasSscal(cublasHandle_t, int n, const float *a, float *x, int) { for (int i = 0; i < n; i++) x[i] *= *a; return CUBLAS_STATUS_SUCCESS; }
inline cublasStatus_t cublasDscal(cublasHandle_t, int n, const double *a, double *x, int) { for (int i = 0; i < n; i++) x[i] *= *a; return CUBLAS_STATUS_SUCCESS; }

// Every tensor the ops allocate "on the device" is a CPU tensor.  This header is read after torch's own headers
// (the reference includes torch first; ref_ops_bind.cpp does too), so only the reference's text sees the rename.
#define kCUDA kCPU
