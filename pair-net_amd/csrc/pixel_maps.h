// Per-axis source-index arithmetic of the image / mask pipelines, ONE definition each, so that
// the test-time front end (preprocess.hip), the loss-side mask preparation (loss.hip) and the
// train-time pipeline (augment.hip) round alike wherever they restate the same library call.
#pragma once
#include "common.h"

// OpenCV INTER_LINEAR for 8-bit images: source index and the two 11-bit coefficients of
// destination index d (half-pixel centres; `scale` = src / dst in double, as cv::resize
// computes it; the horizontal pass clamps the index, the vertical pass clamps the row later).
__device__ __forceinline__ void lin_coef(int d, double scale, int n, int& s, int& a0, int& a1,
                                         bool horizontal) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  s = (int)floorf(f);
  f -= (float)s;
  if (horizontal) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
}

// ... and its fixed-point blend of the four source bytes (p<row><column>): integer horizontal
// pass, vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2, saturated.
__device__ __forceinline__ int lin_blend_u8(int p00, int p01, int p10, int p11, int ax0, int ax1,
                                            int by0, int by1) {
  const int h0 = p00 * ax0 + p01 * ax1;
  const int h1 = p10 * ax0 + p11 * ax1;
  const int v = (((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2;
  return min(max(v, 0), 255);
}

// Normalize of one resized byte: (u - mean) * (1 / std), two separately rounded operations
// (numpy float32 arithmetic; no fused multiply-add)
__device__ __forceinline__ float normalize_u8(int u, float mean, float stdinv) {
  return __fmul_rn(__fsub_rn((float)u, mean), stdinv);
}

// ATen's legacy nearest source index (F.interpolate(mode="nearest") with an output size):
// min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out
__device__ __forceinline__ int aten_nearest(int dst, float scale, int in) {
  return min((int)floorf((float)dst * scale), in - 1);
}

// OpenCV INTER_NEAREST source index: min(floor(dst * ifx), src - 1) in doubles, where
// ifx = 1.0 / ((double)dst_size / src_size) -- NOT src / dst: the two differ (6 -> 34, dst 17)
__device__ __forceinline__ int cv_nearest(int dst, double ifx, int src) {
  return min((int)floor((double)dst * ifx), src - 1);
}

// panopticapi rgb2id of one pixel of the RGB panoptic PNG
__device__ __forceinline__ int rgb2id_px(const uint8_t* p) {
  return (int)p[0] + 256 * (int)p[1] + 65536 * (int)p[2];
}
