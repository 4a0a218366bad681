// The one reader of the library's PCONV_ variables (options.h) and the query that shows what it read.
#include "options.h"
#include <stdio.h>
#include <string.h>
#include "common.h"

// ((void)s: a variable that counts by being set does not look at its value)
#define PCONV_OPTION_READ(name, field, def, parse) \
  if (const char *s = getenv(name)) o.field = ((void)s, (parse));

EeLaunchOptions EeLaunchOptions::from_env() {
  EeLaunchOptions o;
  PCONV_EE_LAUNCH_OPTIONS(PCONV_OPTION_READ)
  return o;
}

EngineOptions EngineOptions::from_env() {
  EngineOptions o;
  PCONV_ENGINE_OPTIONS(PCONV_OPTION_READ)
  if (const char *s = getenv("PCONV_ENGINE_CU_MASK")) (void)sscanf(s, "%d:%d", &o.cu_first, &o.cu_count);
  o.launch = EeLaunchOptions::from_env();
  return o;
}

ConvOptions ConvOptions::from_env() {
  ConvOptions o;
  PCONV_CONV_OPTIONS(PCONV_OPTION_READ)
  return o;
}

ResampleOptions ResampleOptions::from_env() {
  ResampleOptions o;
  PCONV_RESAMPLE_OPTIONS(PCONV_OPTION_READ)
  return o;
}

const char *option_cgroup_cpu_max() { return getenv("PCONV_CGROUP_CPU_MAX"); }

extern "C" int pconv_option(const pconv_entropy_engine *e, const char *name, int *value) {
  PCONV_REQUIRE(name && value, "option: null pointer");
  const EngineOptions engine = e ? engine_options(e) : EngineOptions::from_env();
  const ConvOptions conv = ConvOptions::from_env();
  const ResampleOptions resample = ResampleOptions::from_env();
#define PCONV_OPTION_FIND(n, field, def, parse) \
  if (strcmp(name, n) == 0) return *value = o.field, PCONV_OK;
  {
    const EngineOptions &o = engine;
    PCONV_ENGINE_OPTIONS(PCONV_OPTION_FIND)
    PCONV_OPTION_FIND("PCONV_ENGINE_CU_MASK_FIRST", cu_first, , )
    PCONV_OPTION_FIND("PCONV_ENGINE_CU_MASK_COUNT", cu_count, , )
  }
  {
    const EeLaunchOptions &o = engine.launch;
    PCONV_EE_LAUNCH_OPTIONS(PCONV_OPTION_FIND)
  }
  {
    const ConvOptions &o = conv;
    PCONV_CONV_OPTIONS(PCONV_OPTION_FIND)
  }
  {
    const ResampleOptions &o = resample;
    PCONV_RESAMPLE_OPTIONS(PCONV_OPTION_FIND)
  }
#undef PCONV_OPTION_FIND
  pconv_set_error("option: unknown name %s", name);
  return PCONV_EINVAL;
}
