// The uint8 Y plane of an image, as the metrics and the NIQE kernels read it (the rules are stated at the head of tgsr_metrics.hip):
// quantise_u8 is tgsr_to_uint8's rule, y_of_rgb the reference's rgb2y byte for byte, load_u8 one byte of a uint8 or float32 image.
#pragma once
#include "tgsr_common.h"

namespace tgsr {

__device__ __forceinline__ uint8_t quantise_u8(float v) {
  const float t = __fmul_rn(__fadd_rn(v, 1.0f), 127.5f);
  return (uint8_t)(int)rintf(fminf(255.f, fmaxf(0.f, t)));
}

// The reference's rgb2y on one pixel (see the head of tgsr_metrics.hip); every operation is rounded on its own.
__device__ __forceinline__ uint8_t y_of_rgb(uint8_t r, uint8_t g, uint8_t b) {
  const float fr = __fdiv_rn((float)r, 255.0f), fg = __fdiv_rn((float)g, 255.0f), fb = __fdiv_rn((float)b, 255.0f);
  double y = __dmul_rn((double)fr, 65.481 / 255.0);
  y = __dadd_rn(y, __dmul_rn((double)fg, 128.553 / 255.0));
  y = __dadd_rn(y, __dmul_rn((double)fb, 24.966 / 255.0));
  y = __dadd_rn(y, 16 / 255.0);
  return (uint8_t)(int)__dadd_rn(__dmul_rn(y, 255.0), 0.5);
}

template <bool F32>
__device__ __forceinline__ uint8_t load_u8(const void* __restrict__ p, int64_t i) {
  if (F32) return quantise_u8(static_cast<const float*>(p)[i]);
  return static_cast<const uint8_t*>(p)[i];
}

}  // namespace tgsr
