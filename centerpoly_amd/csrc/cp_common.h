// Shared helpers for libcenterpoly_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "centerpoly_hip.h"

#define CP_WAVE 64

#define CP_CHECK_ARG(cond) \
  do {                     \
    if (!(cond)) return CP_EINVAL; \
  } while (0)

static inline int cp_launch_status() {
  return hipGetLastError() == hipSuccess ? CP_OK : CP_EHIP;
}

static inline size_t cp_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Wave-wide sum (64 lanes) through DPP/shuffles.
__device__ __forceinline__ float cp_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double cp_wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The result writers' vertex, int(float("%.2f" % v)), without text: two decimals round |v| up to the next integer
// exactly when its fraction is above 0.995 (a float32 fraction is never the tie itself); the sign is kept, as int()
// truncates towards zero.
__device__ __forceinline__ int cp_vertex_int(float v) {
  const double a = fabs((double)v);
  if (!(a < 2147483520.0)) return a != a ? 0 : (v < 0 ? INT32_MIN : INT32_MAX);   // NaN, infinities, beyond int32
  const double f = floor(a);
  const double r = f + ((a - f) > 0.995 ? 1.0 : 0.0);
  return v < 0 ? -(int)r : (int)r;
}
