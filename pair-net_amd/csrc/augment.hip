// Train-time input pipeline on the device (configs/mask2former/pairnet.py:234-306):
// RandomFlip -> AutoAugment[ Resize | Resize -> RelRandomCrop -> Resize ] -> Normalize -> Pad ->
// RelsFormatBundle -> collate, then the ground-truth mask preparation of `PSGTr.forward_train`
// (frameworks/psgtr.py:126-141).  The random draws and the <= 256 boxes are host work
// (train_pipeline.py); the per-pixel work is three kernels:
//
//   k_augment_image        the LAST Resize (OpenCV fixed-point INTER_LINEAR, the arithmetic of
//                          k_preprocess) of the optionally flipped source -> Normalize -> zero Pad,
//                          written into the image's slot of the collated [k][3][Hmax][Wmax] batch;
//   k_augment_resize_crop  policy 2's FIRST Resize, evaluated on the crop window only: the second
//                          Resize interpolates bytes the first one has rounded, so this uint8
//                          intermediate has to exist -- but only its [ch][cw] window;
//   k_augment_masks        every mask stage composed: flip, cv2 INTER_NEAREST, crop, cv2
//                          INTER_NEAREST, pad to the batch tensor, ATen nearest to half size are
//                          all gathers, so one index map per axis takes an output pixel of the
//                          [Gk][Hb/2][Wb/2] masks the loss consumes back to a pixel of the
//                          panoptic PNG.  No mask at an intermediate size is ever written.
#include "pixel_maps.h"

__global__ __launch_bounds__(256) void k_augment_image(const uint8_t* __restrict__ img, int H,
                                                       int W, int flip, float* __restrict__ out,
                                                       int Hn, int Wn, int Hmax, int Wmax,
                                                       float m0, float m1, float m2, float s0,
                                                       float s1, float s2, int to_rgb) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t plane = (int64_t)Hmax * Wmax;
  if (e >= plane) return;
  const int oy = (int)(e / Wmax), ox = (int)(e - (int64_t)oy * Wmax);
  if (oy >= Hn || ox >= Wn) {          // Pad and collate: zeros AFTER normalisation
    out[e] = 0.f;
    out[plane + e] = 0.f;
    out[2 * plane + e] = 0.f;
    return;
  }
  int sx, ax0, ax1, sy, by0, by1;
  lin_coef(ox, (double)W / (double)Wn, W, sx, ax0, ax1, true);
  lin_coef(oy, (double)H / (double)Hn, H, sy, by0, by1, false);
  int x1 = min(sx + 1, W - 1);
  if (flip) {                          // columns of the flipped image: a pure permutation
    sx = W - 1 - sx;
    x1 = W - 1 - x1;
  }
  const int y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
  const uint8_t* r0 = img + (int64_t)y0 * W * 3;
  const uint8_t* r1 = img + (int64_t)y1 * W * 3;
  const float mean[3] = {m0, m1, m2}, stdinv[3] = {s0, s1, s2};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int u = lin_blend_u8(r0[sx * 3 + c], r0[x1 * 3 + c], r1[sx * 3 + c], r1[x1 * 3 + c],
                               ax0, ax1, by0, by1);
    const int oc = to_rgb ? 2 - c : c;       // BGR -> RGB; mean / std are in OUTPUT order
    out[oc * plane + e] = normalize_u8(u, mean[oc], stdinv[oc]);
  }
}

extern "C" int pn_augment_image_u8_f32(const uint8_t* img, int H, int W, int flip, float* out,
                                       int64_t batch_stride, int slot, int Hn, int Wn, int Hmax,
                                       int Wmax, const float* mean3, const float* stdinv3,
                                       int to_rgb, void* stream) {
  if (!img || !out || !mean3 || !stdinv3 || H <= 0 || W <= 0 || Hn <= 0 || Wn <= 0 ||
      Hmax < Hn || Wmax < Wn || slot < 0 || batch_stride < 3 * (int64_t)Hmax * Wmax ||
      ((uintptr_t)out & 3))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_augment_image, dim3(pn_cdiv((int64_t)Hmax * Wmax, 256)), dim3(256), 0,
                     (hipStream_t)stream, img, H, W, flip ? 1 : 0, out + slot * batch_stride, Hn,
                     Wn, Hmax, Wmax, mean3[0], mean3[1], mean3[2], stdinv3[0], stdinv3[1],
                     stdinv3[2], to_rgb);
  return PN_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void k_augment_resize_crop(const uint8_t* __restrict__ img,
                                                             int H, int W, int flip, int H1,
                                                             int W1, int oy, int ox,
                                                             uint8_t* __restrict__ out, int ch,
                                                             int cw) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)ch * cw) return;
  const int y = (int)(e / cw), x = (int)(e - (int64_t)y * cw);
  int sx, ax0, ax1, sy, by0, by1;
  lin_coef(x + ox, (double)W / (double)W1, W, sx, ax0, ax1, true);
  lin_coef(y + oy, (double)H / (double)H1, H, sy, by0, by1, false);
  int x1 = min(sx + 1, W - 1);
  if (flip) {
    sx = W - 1 - sx;
    x1 = W - 1 - x1;
  }
  const int y0 = min(max(sy, 0), H - 1), y1 = min(max(sy + 1, 0), H - 1);
  const uint8_t* r0 = img + (int64_t)y0 * W * 3;
  const uint8_t* r1 = img + (int64_t)y1 * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c)
    out[e * 3 + c] = (uint8_t)lin_blend_u8(r0[sx * 3 + c], r0[x1 * 3 + c], r1[sx * 3 + c],
                                           r1[x1 * 3 + c], ax0, ax1, by0, by1);
}

extern "C" int pn_augment_resize_crop_u8(const uint8_t* img, int H, int W, int flip, int H1,
                                         int W1, int oy, int ox, uint8_t* out, int ch, int cw,
                                         void* stream) {
  if (!img || !out || H <= 0 || W <= 0 || H1 <= 0 || W1 <= 0 || ch <= 0 || cw <= 0 || oy < 0 ||
      ox < 0 || (int64_t)oy + ch > H1 || (int64_t)ox + cw > W1)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_augment_resize_crop, dim3(pn_cdiv((int64_t)ch * cw, 256)), dim3(256), 0,
                     (hipStream_t)stream, img, H, W, flip ? 1 : 0, H1, W1, oy, ox, out, ch, cw);
  return PN_LAUNCH_CHECK();
}

// The composed map of one axis, right to left through the pipeline.  Returns the PNG index, or
// -1 where the half-size pixel looks at the padding of the batch tensor.
struct AxisMap {
  float half;      // ATen: (float)Nb / (float)(Nb / 2)
  double inv2;     // cv2, second Resize: 1.0 / ((double)N2 / nc)   (1.0 for policy 1)
  double inv1;     // cv2, first Resize:  1.0 / ((double)N1 / N0)
  int Nb, N2, nc, off, N0;
};
__device__ __forceinline__ int axis_src(int d, const AxisMap& m) {
  const int b = aten_nearest(d, m.half, m.Nb);       // pixel of the padded batch tensor
  if (b >= m.N2) return -1;                          // Pad / collate: zeros
  const int c = cv_nearest(b, m.inv2, m.nc);         // pixel of the crop window
  return cv_nearest(c + m.off, m.inv1, m.N0);        // pixel of the (flipped) PNG
}

// HBM-bound byte work like k_pan_masks: a thread owns four consecutive pixels of the flattened
// [Ho * Wo] plane (they may wrap to the next row) and does one 32-bit store per segment; where
// the plane size is no multiple of 4 the planes of odd segments are misaligned and the thread
// stores bytes.  The <= 256 ids sit in LDS.
#define AUG_MAX_SEGMENTS 256
__global__ __launch_bounds__(256) void k_augment_masks(const uint8_t* __restrict__ png,
                                                       const int* __restrict__ ids, const int G,
                                                       const int flip, const AxisMap my,
                                                       const AxisMap mx, const int Ho,
                                                       const int Wo, uint8_t* __restrict__ out) {
  __shared__ int s_id[AUG_MAX_SEGMENTS];
  for (int g = threadIdx.x; g < G; g += 256) s_id[g] = ids[g];
  __syncthreads();
  const int64_t HW = (int64_t)Ho * Wo;
  const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (p0 >= HW) return;
  int y = (int)(p0 / Wo), x = (int)(p0 - (int64_t)y * Wo);
  int sy = axis_src(y, my);
  int id[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    id[j] = -1;                                      // (no segment id is negative)
    if (p0 + j < HW) {
      int sx = axis_src(x, mx);
      if (sy >= 0 && sx >= 0) {
        if (flip) sx = mx.N0 - 1 - sx;
        id[j] = rgb2id_px(png + ((int64_t)sy * mx.N0 + sx) * 3);
      }
      if (++x == Wo) {
        x = 0;
        ++y;
        if (y < Ho) sy = axis_src(y, my);
      }
    }
  }
  const bool whole = p0 + 4 <= HW && !(HW & 3);      // (every plane of `out` 4-aligned)
  for (int g = 0; g < G; ++g) {
    const int want = s_id[g];
    const unsigned m0 = id[0] == want, m1 = id[1] == want, m2 = id[2] == want, m3 = id[3] == want;
    uint8_t* dst = out + (int64_t)g * HW + p0;
    if (whole) {
      *reinterpret_cast<unsigned*>(dst) = m0 | (m1 << 8) | (m2 << 16) | (m3 << 24);
    } else {
      const unsigned m[4] = {m0, m1, m2, m3};
      for (int j = 0; j < 4; ++j)
        if (p0 + j < HW) dst[j] = (uint8_t)m[j];
    }
  }
}

extern "C" int pn_augment_masks_u8(const uint8_t* png, int H0, int W0, const int* ids, int Gk,
                                   int flip, int H1, int W1, int oy, int ox, int ch, int cw,
                                   int H2, int W2, int Hb, int Wb, uint8_t* out, void* stream) {
  if (!png || !ids || !out || H0 <= 0 || W0 <= 0 || Gk <= 0 || Gk > AUG_MAX_SEGMENTS || H1 <= 0 ||
      W1 <= 0 || ch <= 0 || cw <= 0 || H2 <= 0 || W2 <= 0 || oy < 0 || ox < 0 ||
      (int64_t)oy + ch > H1 || (int64_t)ox + cw > W1 || Hb < H2 || Wb < W2 || Hb < 2 || Wb < 2)
    return PN_BAD_ARG;
  if (((uintptr_t)png | (uintptr_t)out | (uintptr_t)ids) & 3) return PN_BAD_ARG;
  const int Ho = Hb / 2, Wo = Wb / 2;
  AxisMap my, mx;
  my.half = (float)Hb / (float)Ho;
  my.inv2 = 1.0 / ((double)H2 / (double)ch);
  my.inv1 = 1.0 / ((double)H1 / (double)H0);
  my.Nb = Hb, my.N2 = H2, my.nc = ch, my.off = oy, my.N0 = H0;
  mx.half = (float)Wb / (float)Wo;
  mx.inv2 = 1.0 / ((double)W2 / (double)cw);
  mx.inv1 = 1.0 / ((double)W1 / (double)W0);
  mx.Nb = Wb, mx.N2 = W2, mx.nc = cw, mx.off = ox, mx.N0 = W0;
  hipLaunchKernelGGL(k_augment_masks, dim3(pn_cdiv(pn_cdiv((int64_t)Ho * Wo, 4), 256)), dim3(256),
                     0, (hipStream_t)stream, png, ids, Gk, flip ? 1 : 0, my, mx, Ho, Wo, out);
  return PN_LAUNCH_CHECK();
}
