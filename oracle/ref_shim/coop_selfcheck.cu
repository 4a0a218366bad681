// TEST INFRASTRUCTURE -- kernels of our own that check the cooperative-block launcher (coop_launch.h) before the
// reference's masked convolution is trusted to it.  Written as CUDA, taken through the same recipe as that file
// (oracle/ref_ops.py rewrites the launches and compiles with -DSHIM_COOPERATIVE), bound in ref_ops_bind.cpp and
// run by tests/test_reference_ops_cpu.py.
#include <cuda_runtime.h>

#include <vector>

// every thread publishes a value and reads its right-hand neighbour's: wrong for all but the last thread when the
// barrier does not hold the readers back until every writer is done
__global__ void selfcheck_neighbour(float *out, int seed) {
  extern __shared__ int __smem[];
  float *sdata = (float *)__smem;
  const int t = threadIdx.x, n = blockDim.x;
  sdata[t] = (float)(seed + 1000 * (int)blockIdx.x + 3 * t + 1);
  __syncthreads();
  out[blockIdx.x * n + t] = sdata[(t + 1) % n];
}

// 128 values to one: halves 128 -> 64 -> 32 through shared memory, then shuffle-down 16 .. 1 inside the first warp
__global__ void selfcheck_tree(const float *in, float *out) {
  extern __shared__ int __smem[];
  float *sdata = (float *)__smem;
  const int t = threadIdx.x;
  float v = in[blockIdx.x * 128 + t];
  sdata[t] = v;
  __syncthreads();
  if (t < 64) sdata[t] = v = v + sdata[t + 64];
  __syncthreads();
  if (t < 32) {
    v += sdata[t + 32];
    for (int offset = warpSize / 2; offset > 0; offset /= 2) v += __shfl_down_sync(0xffffffff, v, offset);
  }
  if (t == 0) out[blockIdx.x] = v;
}

// the first warp alone shuffles (the others have returned by then); every stage of every lane is recorded
__global__ void selfcheck_shuffle(const float *in, float *out) {
  const int t = threadIdx.x, n = blockDim.x;
  float v = in[blockIdx.x * n + t];
  int stage = 0;
  for (int offset = 16; offset > 0; offset /= 2, stage++) {
    if (t >= 32) {
      out[(blockIdx.x * 5 + stage) * n + t] = v;
      continue;
    }
    v = __shfl_down_sync(0xffffffff, v, offset);
    out[(blockIdx.x * 5 + stage) * n + t] = v;
  }
}

// `launches` launches in a row of `blocks` blocks of `n` threads, each with its own seed
std::vector<float> coop_neighbour(int n, int blocks, int launches) {
  std::vector<float> out((size_t)n * blocks * launches, -1.0f);
  for (int l = 0; l < launches; l++)
    selfcheck_neighbour<<<blocks, n, n * sizeof(float), 0>>>(out.data() + (size_t)l * n * blocks, 100000 * l);
  return out;
}

std::vector<float> coop_tree(std::vector<float> in) {
  const int blocks = (int)(in.size() / 128);
  std::vector<float> out(blocks, -1.0f);
  selfcheck_tree<<<blocks, 128, 128 * sizeof(float), 0>>>(in.data(), out.data());
  return out;
}

std::vector<float> coop_shuffle(std::vector<float> in, int n) {
  const int blocks = (int)(in.size() / n);
  std::vector<float> out((size_t)blocks * 5 * n, -1.0f);
  selfcheck_shuffle<<<blocks, n>>>(in.data(), out.data());
  return out;
}
