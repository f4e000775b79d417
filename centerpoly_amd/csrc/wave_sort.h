// A bitonic sort of 128 float32 values held two per lane across one 64-lane wave, through wave shuffles: what the
// wave form of the scan line (scanline.h) orders a row's crossing list with.
#pragma once
#include <hip/hip_runtime.h>

// one compare-exchange step of the bitonic network on element `v` of this lane against lane ^ j
__device__ __forceinline__ float bitonic_step(float v, int lane, int j, bool ascending) {
  const float o = __shfl_xor(v, j, 64);
  const bool lower = (lane & j) == 0;
  return lower == ascending ? fminf(v, o) : fmaxf(v, o);
}

// sorts the 128 values (a of lane l = element l, b of lane l = element 64 + l) ascending across the wave
__device__ __forceinline__ void wave_sort128(float& a, float& b, int lane) {
#pragma unroll
  for (int k = 2; k <= 128; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j == 64) {                                                      // k == 128: element l against 64 + l
        const float lo = fminf(a, b), hi = fmaxf(a, b);
        a = lo; b = hi;
      } else {
        a = bitonic_step(a, lane, j, (lane & k) == 0);
        b = bitonic_step(b, lane, j, ((lane + 64) & k) == 0);
      }
    }
  }
}
