// TEST INFRASTRUCTURE -- the cooperative-block launcher declared in coop_launch.h.
//
// Fibers: each thread slot of a block owns a stack, entered once with makecontext / setcontext and from then on
// switched with _setjmp / _longjmp, which leave the signal mask alone (swapcontext makes a system call per switch:
// about 700 switches per block of the masked convolution).  A fiber is a loop: park, run the kernel body once,
// mark itself done, park again; so the stacks are made once per process and reused by every block and launch.
// The fortified longjmp refuses to jump to a frame on another stack, hence the #undef before any header.
#undef _FORTIFY_SOURCE
#include <setjmp.h>
#include <ucontext.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "coop_launch.h"

shim_dim3 threadIdx{0, 0, 0}, blockIdx{0, 0, 0}, blockDim{1, 1, 1}, gridDim{1, 1, 1};
// the one dynamic shared array of the block that is running ("extern __shared__ int __smem[]" in the kernels)
int __smem[shim_coop::SMEM_BYTES / sizeof(int)];

namespace shim_coop {
namespace {

enum Wait { RUNNING, BARRIER, SHFL_WRITTEN, SHFL_READ };
const size_t STACK_BYTES = 64 * 1024;

struct Fiber {
  jmp_buf env;
  ucontext_t uc;
  char *stack;
  unsigned tid;
  int wait;
  bool done;
  unsigned char slot[8];
};

Fiber *fibers[MAX_BLOCK];
unsigned nfibers = 0;          // stacks made so far
unsigned nthreads = 0;         // threads of the running block; 0 outside a launch
Fiber *current = nullptr;
jmp_buf scheduler;
void (*body)(void *) = nullptr;
void *body_arg = nullptr;

void die(const char *what) {
  std::fprintf(stderr, "shim_coop: %s\n", what);
  std::abort();
}

// (own frames for the two _setjmp calls: no local of a caller changes between the call and the jump back)
__attribute__((noinline)) void park(Fiber *f, int wait) {
  f->wait = wait;
  if (!_setjmp(f->env)) _longjmp(scheduler, 1);
}

__attribute__((noinline)) void resume(Fiber *f) {
  current = f;
  threadIdx.x = f->tid;
  if (!_setjmp(scheduler)) _longjmp(f->env, 1);
  current = nullptr;
}

void fiber_main() {
  Fiber *f = current;
  for (;;) {
    park(f, RUNNING);
    body(body_arg);
    f->done = true;
  }
}

void make_fiber(unsigned tid) {
  Fiber *f = static_cast<Fiber *>(std::calloc(1, sizeof(Fiber)));
  if (!f || !(f->stack = static_cast<char *>(std::malloc(STACK_BYTES)))) die("out of memory");
  f->tid = tid;
  f->done = true;
  if (getcontext(&f->uc)) die("getcontext");
  f->uc.uc_stack.ss_sp = f->stack;
  f->uc.uc_stack.ss_size = STACK_BYTES;
  f->uc.uc_link = nullptr;
  makecontext(&f->uc, fiber_main, 0);
  fibers[tid] = f;
  current = f;
  if (!_setjmp(scheduler)) setcontext(&f->uc);       // runs fiber_main up to its first park
  current = nullptr;
}

}  // namespace

void launch_raw(unsigned grid, unsigned block, size_t smem, void (*fn)(void *), void *arg) {
  if (nthreads) die("a launch inside a kernel");
  if (block == 0 || block > MAX_BLOCK) die("block size out of range");
  if (smem > SMEM_BYTES) die("more dynamic shared memory than the launcher holds");
  while (nfibers < block) make_fiber(nfibers++);
  body = fn;
  body_arg = arg;
  nthreads = block;
  blockDim = shim_dim3{block, 1, 1};
  gridDim = shim_dim3{grid, 1, 1};
  for (unsigned b = 0; b < grid; b++) {
    blockIdx = shim_dim3{b, 0, 0};
    std::memset(__smem, 0xff, smem);                 // a block sees no value of the block before: NaN patterns
    for (unsigned t = 0; t < block; t++) {
      fibers[t]->done = false;
      std::memset(fibers[t]->slot, 0xff, sizeof(fibers[t]->slot));
    }
    for (unsigned live = block; live;) {
      int kind = RUNNING;
      for (unsigned t = 0; t < block; t++) {
        Fiber *f = fibers[t];
        if (f->done) continue;
        resume(f);
        if (f->done) {
          live--;
        } else if (kind == RUNNING) {
          kind = f->wait;
        } else if (kind != f->wait) {
          die("the threads of a block wait at different kinds of synchronisation");
        }
      }
    }
  }
  nthreads = 0;
  threadIdx = blockIdx = shim_dim3{0, 0, 0};
  blockDim = gridDim = shim_dim3{1, 1, 1};
}

void barrier() {
  if (!current) die("__syncthreads outside a launch");
  park(current, BARRIER);
}

void shfl_down(void *value, size_t size, unsigned delta) {
  Fiber *f = current;
  if (!f) die("shuffle outside a launch");
  std::memcpy(f->slot, value, size);
  park(f, SHFL_WRITTEN);                             // every taking-part lane has written its slot
  const unsigned lane = f->tid % 32, src = f->tid + delta;
  if (lane + delta < 32 && src < nthreads) std::memcpy(value, fibers[src]->slot, size);
  park(f, SHFL_READ);                                // every lane has read before a slot is written again
}

}  // namespace shim_coop
