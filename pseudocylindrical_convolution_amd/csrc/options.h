// Tuning options of libpconv_hip.so: every PCONV_ variable the native library reads, read HERE and nowhere else.
//
// THE RULE: an engine keeps the options it was created with (pconv_ee_create reads EngineOptions once and stores
// them; encode, decode, rate and the launchers they call never look at the environment again), and a stateless
// entry point reads its options when it is called (pconv_conv2d, pconv_gdn, pconv_sphere_slice / _uslice, and the
// host-side queries pconv_ee_host_cpus / _spin_us / _host_plan).  Nothing is cached per process.
//
// One row per option: X(variable, field, default, value of a set variable `s`).  The struct, the reader and
// pconv_option's lookup are generated from the rows; the codes are documented beside pconv_option
// (include/pconv_hip.h) and the defaults, with the measurements that decided them, in DESIGN.md ("What runs by
// default").
#pragma once
#include <limits.h>
#include <stdlib.h>

struct pconv_entropy_engine;

constexpr int kOptionAuto = INT_MIN;  // PCONV_OPTION_AUTO: not set, the library decides (host_plan, step_pool_spin_us)

// launch shapes of the entropy kernels (ee_kernels.h: ee_conv, ee_conv_tables, ee_conv_bulk_mfma, ee_mfma_block_shape)
#define PCONV_EE_LAUNCH_OPTIONS(X)                                                                                   \
  X("PCONV_EE_BLOCK", block, 256, atoi(s))         /* step kernel: threads per workgroup (256 / 512 / 1024) */       \
  X("PCONV_EE_PPW", ppw, 0, atoi(s))               /* ... positions a wave walks; <= 0: 2 for one frame, else 8 */   \
  X("PCONV_EE_JOINT", joint, 2, atoi(s))           /* ... positions per loop body (1 or 2) */                        \
  X("PCONV_EE_CONTIG", contig, 1, atoi(s))         /* ... 0 interleaved, 1 contiguous shares, 2 + neighbour pairs */ \
  X("PCONV_EE_XCD", xcd, 0, atoi(s))               /* ... 1: the 1-D XCD-major workgroup order */                    \
  X("PCONV_EE_FUSE_PPW", fuse_ppw, 4, atoi(s))     /* fused last layer + tables: positions per wave */               \
  X("PCONV_EE_MFMA_WSRC", mfma_ring, 0, s[0] == 'r') /* matrix-core encoder: weights through the LDS ring */         \
  X("PCONV_EE_MFMA_WAVES", mfma_waves, 4, atoi(s)) /* ... waves per workgroup (8, else 4) */                         \
  X("PCONV_EE_MFMA_NT", mfma_nt, 1, atoi(s))       /* ... rows per wave (1, else 2 where the rows are even) */

// the rest of an engine: host plan overrides, row format, encoder forms, diagnostics
#define PCONV_ENGINE_OPTIONS(X)                                                                                      \
  X("PCONV_ENGINE_GROUPS", groups, kOptionAuto, atoi(s))                                                             \
  X("PCONV_ENGINE_WORKERS", workers, kOptionAuto, atoi(s))                                                           \
  X("PCONV_ENGINE_CHAIN", chain, kOptionAuto, s[0] != 'h')             /* 1 queued, 0 host-driven */                 \
  X("PCONV_ENGINE_BLOCKING_SYNC", blocking_sync, kOptionAuto, atoi(s) != 0)                                          \
  X("PCONV_ENGINE_SPIN_US", spin_us, kOptionAuto, atoi(s))                                                           \
  X("PCONV_ENGINE_ROWS", rows_int32, 0, s[0] == 'i')                   /* int32 rows + labels across PCIe */         \
  X("PCONV_ENGINE_STEPWISE_ENCODER", stepwise_encoder, 0, 1)           /* set at all: the debugging encoder */       \
  X("PCONV_ENGINE_CLEAR_EVERY_CALL", clear_every_call, 0, atoi(s) != 0)                                              \
  X("PCONV_ENGINE_ALLOC_FILL", alloc_fill, -1, (int)(strtol(s, nullptr, 0) & 255)) /* byte over new buffers (tests) */ \
  X("PCONV_ENGINE_ENCODE_RANGES", encode_ranges, 4, atoi(s))           /* step ranges of a call's last group */      \
  X("PCONV_ENGINE_ENCODE_INTERLEAVE", encode_interleave, 1, atoi(s) != 0)                                            \
  X("PCONV_ENGINE_RATE_STREAMS", rate_group_streams, 0, s[0] == 'g')   /* rate(): each group on its own stream */    \
  X("PCONV_ENGINE_TIMING", timing, 0, 1)                               /* set at all: one stderr line per call */    \
  X("PCONV_EE_BULK", bulk_valu, 0, s[0] == 'v')                        /* vector kernel for the whole encoder */     \
  X("PCONV_EE_BULK0", bulk0_valu, 0, s[0] == 'v')                      /* ... for its input layer only */            \
  X("PCONV_EE_MFMA_FORM", mfma_16x4, 0, s[0] == '1')                   /* 16x16x4 form instead of the four-block */  \
  X("PCONV_EE_FUSE_TABLES", fuse_tables, 0, atoi(s) != 0)              /* decoder: last layer + tables, 1 launch */

// pconv_conv2d / pconv_gdn, read at the top of every call
#define PCONV_CONV_OPTIONS(X)                                                                                        \
  X("PCONV_CONV1X1", conv1x1, 0, s[0] == 't' ? 1 : s[0] == 'r' ? 2 : 0) /* 0 auto, 1 tiled, 2 resident */            \
  X("PCONV_CONV1X1_STAGGER", stagger, -1, atoi(s))                      /* resident form; < 0: 0 */                  \
  X("PCONV_CONV1X1_WAYOUT", wayout, 0, s[0] == 'p' ? 1 : s[0] == 'b' ? 2 : 0) /* 0 quads, 1 pipe, 2 batch */         \
  X("PCONV_CONV_SMALL", small_cout, 1, s[0] != '0')                     /* <= 16 couts on the 16x16x4 kernel */      \
  X("PCONV_CONV_XCD", xcd, 0, atoi(s))                                  /* 1: XCD-grouped workgroup order (3x3) */

// pconv_sphere_slice / _uslice, read at the top of every call
#define PCONV_RESAMPLE_OPTIONS(X) X("PCONV_RESAMPLE_ROWS", rows, 2, atoi(s)) /* rows a workgroup stages (1 / 2 / 4) */

#define PCONV_OPTION_FIELD(name, field, def, parse) int field = def;
struct EeLaunchOptions {
  PCONV_EE_LAUNCH_OPTIONS(PCONV_OPTION_FIELD)
  static EeLaunchOptions from_env();
};
struct EngineOptions {
  PCONV_ENGINE_OPTIONS(PCONV_OPTION_FIELD)
  int cu_first = 0, cu_count = 0;  // PCONV_ENGINE_CU_MASK=first:count (count 0: no mask)
  EeLaunchOptions launch;
  static EngineOptions from_env();
};
struct ConvOptions {
  PCONV_CONV_OPTIONS(PCONV_OPTION_FIELD)
  static ConvOptions from_env();
};
struct ResampleOptions {
  PCONV_RESAMPLE_OPTIONS(PCONV_OPTION_FIELD)
  static ResampleOptions from_env();
};
#undef PCONV_OPTION_FIELD

// PCONV_CGROUP_CPU_MAX: another cpu.max-format file for the host-share queries (tests), or null
const char *option_cgroup_cpu_max();
// the options `e` was created with (engine.cpp)
const EngineOptions &engine_options(const pconv_entropy_engine *e);
