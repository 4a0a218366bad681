// TEST INFRASTRUCTURE -- stand-in for ATen's CUDA context: no device to select, one null stream
#pragma once
#include <cuda_runtime.h>
namespace at { namespace cuda {
inline void set_device(int) {}
struct ShimStream { cudaStream_t stream() const { return nullptr; } };
inline ShimStream getCurrentCUDAStream() { return ShimStream(); }
}}
