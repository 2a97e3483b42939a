// Log-add-exp helpers shared by the kernels that read the recognizer (ctc_decode.hip, ctc_beam.hip).
#pragma once
#include "sg_common.h"

__device__ __forceinline__ float dec_lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float dec_lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}
