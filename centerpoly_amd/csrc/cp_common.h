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

// The library's one ReLU, as torch.relu computes it: v where v is a NaN, fmaxf(v, 0.f) otherwise.  fmaxf alone
// (v_max_f32) returns the operand that is not a NaN, so it turned a NaN into 0.  IEEE 754-2019 maximum is one
// instruction on gfx950 (v_maximum3_f32 v, 0, 0) and gives every other value, -0, denormals and the infinities included,
// the bits of fmaxf(v, 0.f); `v != v ? v : fmaxf(v, 0.f)` is a compare and a select more and cost the inference step
// 0.6 %.  Both claims rest on the compiler's lowering of the builtin: the guard is
// test_relu_keeps_the_bits_of_every_other_value (tests/test_nonfinite.py), a sweep of float32 bit patterns on the device.
__device__ __forceinline__ float cp_relu(float v) { return __builtin_elementwise_maximum(v, 0.f); }

__device__ __forceinline__ f32x4 cp_relu(f32x4 v) {
  return f32x4{cp_relu(v[0]), cp_relu(v[1]), cp_relu(v[2]), cp_relu(v[3])};
}

// torch.clamp(v, lo, hi) for lo <= hi: a NaN stays a NaN, every other value takes fminf(fmaxf(v, lo), hi).
__device__ __forceinline__ float cp_clamp(float v, float lo, float hi) { return v != v ? v : fminf(fmaxf(v, lo), hi); }

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

// cv::warpAffine's in-place inversion of the forward 2x3 map (float64, host): trans src -> dst, M dst -> src.
static inline void cp_invert_affine(const double* trans, double* M) {
  for (int i = 0; i < 6; ++i) M[i] = trans[i];
  double D = M[0] * M[4] - M[1] * M[3];
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
}

// cvRound(v * 2^10), saturated to int: the fixed-point source coordinate of cv::warpAffine.
__device__ __forceinline__ long long cp_round_fix(double v) {
  const double s = v * 1024.0;
  if (s >= 2147483647.0) return 2147483647ll;
  if (s <= -2147483648.0) return -2147483648ll;
  return (long long)__double2int_rn(s);                      // round half to even
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
