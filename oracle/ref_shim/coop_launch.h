// TEST INFRASTRUCTURE -- cooperative-block launcher for the CPU build of the reference's masked convolution
// (oracle/ref_ops.py gives it to that one translation unit, and to our self-check kernels, with -DSHIM_COOPERATIVE).
// A launch `kernel<<<grid, block, smem, stream>>>(args);` is rewritten by the recipe into
// `shim_coop::launch(grid, block, smem, stream, [&] { kernel(args); });`.  The blocks run one after another; inside
// a block the `block` threads are fibers of one OS thread, resumed round-robin in thread order, so a run is
// deterministic.  __syncthreads() and the two halves of a shuffle are the only switch points: a fiber runs until it
// reaches one or returns, then the next one runs.  Every live thread therefore stands at the same barrier before
// any of them goes on -- real barrier semantics -- and the launcher aborts when the threads of a block do not all
// wait in the same kind of switch point in one round (a barrier some threads skip is undefined in CUDA too).
#pragma once
#include <cstddef>
#include <cstring>

struct shim_dim3 { unsigned x, y, z; };
// per thread: the launcher sets them before it resumes a fiber
extern shim_dim3 threadIdx, blockIdx, blockDim, gridDim;
static const int warpSize = 32;

namespace shim_coop {
enum { MAX_BLOCK = 1024, SMEM_BYTES = 48 * 1024 };
void launch_raw(unsigned grid, unsigned block, size_t smem, void (*body)(void *), void *arg);
void barrier();
// 8 bytes of the calling thread's value in, the value of thread `lane + delta` of the same 32-lane warp out; a
// lane whose source would be lane 32 or above keeps its own.  Threads that do not call (returned, or outside the
// branch) take no part; their slots keep whatever they last held.
void shfl_down(void *value, size_t size, unsigned delta);
template <class F> void body_of(void *f) { (*static_cast<F *>(f))(); }
template <class F> void launch(unsigned grid, unsigned block, size_t smem, void *, F f) {
  launch_raw(grid, block, smem, &body_of<F>, &f);
}
template <class F> void launch(unsigned grid, unsigned block, F f) { launch_raw(grid, block, 0, &body_of<F>, &f); }
}  // namespace shim_coop

inline void __syncthreads() { shim_coop::barrier(); }
template <class T> inline T __shfl_down_sync(unsigned, T v, int delta) {
  static_assert(sizeof(T) <= 8, "shuffle of at most 8 bytes");
  shim_coop::shfl_down(&v, sizeof(T), (unsigned)delta);
  return v;
}
