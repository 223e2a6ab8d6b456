// Shared by the parts of msm_impl.h: includes, cdiv for grid sizes and the register-cap attributes of the tail kernels.
#pragma once
#include "ec_dev.h"
#include "engine.h"
#include "fpr_dev.h"
#include "host_ec.h"
#include "params_gen.h"
#include "tuning.h"
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace mg {

static inline u32 cdiv(size_t a, size_t b) { return (u32)((a + b - 1) / b); }

// Register caps of the tail kernels (merge, bucket reduce; msm_reduce.h): none for the scan kernels and the cooperative ones
#define MG_TAIL_ATTR
#define MG_TAIL_COOP_ATTR
// serial_reduce holds three points (acc, sum, the loaded item): 266 VGPRs left alone = one wavefront per SIMD; capped at
// 256 (30 spilled) two fit, and the big first level (2^19 buckets at c = 20) runs at the issue rate of two wavefronts
#define MG_SERIAL_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))

} // namespace mg
