// The body of the lane-per-channel deformable-attention backward, shared by the atomic kernel
// (csrc/msda.hip: k_msda_bwd_lanes) and the deterministic pipeline (csrc/msda_grad.hip): ONE
// device function, so that grad_sampling_loc / grad_attn_weight of the two entries are the same
// arithmetic bit for bit, and one tap geometry, so that every pass of the deterministic pipeline
// finds the same in-map taps.
#pragma once
#include "common.h"

// The four bilinear taps of one sampling point, mmcv's ms_deform_attn_col2im_bilinear: tap t in
// the order (ya,xa), (ya,xb), (yb,xa), (yb,xb); tok[t] is the level-local pixel index (clamped
// into the map), in[t] says whether the tap lies inside it.
struct MsdaBwdTaps {
  bool inside;          // the point itself is inside (-1, H) x (-1, W)
  bool in[4];
  int tok[4];           // ya * W + xa, ... (every one inside [0, H * W))
  float lh, lw, hh, hw;
  float w[4];           // hh*hw, hh*lw, lh*hw, lh*lw
};

__device__ __forceinline__ MsdaBwdTaps msda_bwd_taps(const float2 lc, const int Hl, const int Wl) {
  MsdaBwdTaps t;
  const float h_im = lc.y * (float)Hl - 0.5f, w_im = lc.x * (float)Wl - 0.5f;
  t.inside = h_im > -1.f && w_im > -1.f && h_im < (float)Hl && w_im < (float)Wl;
  // (inside: floor() lies in [-1, H - 1] x [-1, W - 1], the int conversion cannot overflow; NaN
  // locations fail the test)
  const float fy = t.inside ? floorf(h_im) : 0.f, fx = t.inside ? floorf(w_im) : 0.f;
  const int y0 = (int)fy, x0 = (int)fx;
  t.lh = h_im - fy; t.lw = w_im - fx; t.hh = 1.f - t.lh; t.hw = 1.f - t.lw;
  const bool yin0 = y0 >= 0, yin1 = y0 + 1 <= Hl - 1, xin0 = x0 >= 0, xin1 = x0 + 1 <= Wl - 1;
  const int ya = max(y0, 0), yb = min(y0 + 1, Hl - 1), xa = max(x0, 0), xb = min(x0 + 1, Wl - 1);
  t.tok[0] = ya * Wl + xa; t.tok[1] = ya * Wl + xb; t.tok[2] = yb * Wl + xa; t.tok[3] = yb * Wl + xb;
  t.in[0] = t.inside && yin0 && xin0; t.in[1] = t.inside && yin0 && xin1;
  t.in[2] = t.inside && yin1 && xin0; t.in[3] = t.inside && yin1 && xin1;
  t.w[0] = t.hh * t.hw; t.w[1] = t.hh * t.lw; t.w[2] = t.lh * t.hw; t.w[3] = t.lh * t.lw;
  return t;
}

// Workgroup = one (batch, query), 512 threads: a wave owns one head and two points at a time, its
// 32-lane halves each cover ONE 128-byte value row per tap.  grad_sampling_loc and
// grad_attn_weight are written; grad_value's contributions are
//   COUNT = false: added with hardware fp32 atomics (the atomic entry);
//   COUNT = true : not added; the half's first lane counts every in-map tap into
//                  cnt[(b * 8 + head) * N + token] instead (pass 1 of the deterministic entry).
//                  A token outside [0, N) (a level_start_index that does not match N) is not
//                  counted, and is skipped in the same way by the fill pass.
template <int L, bool COUNT>
__device__ __forceinline__ void msda_bwd_lanes_body(
    const float* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ starts, const float* __restrict__ loc,
    const float* __restrict__ aw, const float* __restrict__ gout, float* __restrict__ gvalue,
    float* __restrict__ gloc, float* __restrict__ gaw, int* __restrict__ cnt, const int N,
    const int Nq, const int64_t ldv) {
  const int tid = threadIdx.x;
  const int b = blockIdx.y, q = blockIdx.x;
  constexpr int LP = L * 4;
  const int c = tid & 31, half = (tid >> 5) & 1, head = tid >> 6;
  const float g = gout[((int64_t)b * Nq + q) * 256 + head * 32 + c];
  const float* vb = value + (int64_t)b * N * ldv + head * 32 + c;
  float* gvb = gvalue + (int64_t)b * N * ldv + head * 32 + c;
#pragma unroll
  for (int l = 0; l < L; ++l) {
    const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
    const int64_t base = starts[l];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
      const int pt = pp * 2 + half;
      const int64_t slot = (((int64_t)b * Nq + q) * 8 + head) * LP + l * 4 + pt;
      const float2 lc = *reinterpret_cast<const float2*>(loc + 2 * slot);
      const float a = aw[slot];
      const MsdaBwdTaps t = msda_bwd_taps(lc, Hl, Wl);
      float ga = 0.f, gx = 0.f, gy = 0.f;
      if (t.inside) {                                           // (uniform in the half)
        const float lh = t.lh, lw = t.lw, hh = t.hh, hw = t.hw;
        const int64_t r1 = (base + t.tok[0]) * ldv, r2 = (base + t.tok[1]) * ldv;
        const int64_t r3 = (base + t.tok[2]) * ldv, r4 = (base + t.tok[3]) * ldv;
        const bool in1 = t.in[0], in2 = t.in[1], in3 = t.in[2], in4 = t.in[3];
        float v1, v2, v3, v4;
        if (COUNT) {
          // the deterministic entry tests what the atomic one trusts: rows outside [0, N) are
          // neither read nor counted
          const bool ok1 = in1 && base + t.tok[0] >= 0 && base + t.tok[0] < N;
          const bool ok2 = in2 && base + t.tok[1] >= 0 && base + t.tok[1] < N;
          const bool ok3 = in3 && base + t.tok[2] >= 0 && base + t.tok[2] < N;
          const bool ok4 = in4 && base + t.tok[3] >= 0 && base + t.tok[3] < N;
          v1 = ok1 ? vb[r1] : 0.f; v2 = ok2 ? vb[r2] : 0.f;
          v3 = ok3 ? vb[r3] : 0.f; v4 = ok4 ? vb[r4] : 0.f;
          if (c == 0) {
            int* cb = cnt + (int64_t)(b * 8 + head) * N + base;
            if (ok1) atomicAdd(cb + t.tok[0], 1);
            if (ok2) atomicAdd(cb + t.tok[1], 1);
            if (ok3) atomicAdd(cb + t.tok[2], 1);
            if (ok4) atomicAdd(cb + t.tok[3], 1);
          }
        } else {
          v1 = vb[r1]; v2 = vb[r2]; v3 = vb[r3]; v4 = vb[r4];
          v1 = in1 ? v1 : 0.f; v2 = in2 ? v2 : 0.f; v3 = in3 ? v3 : 0.f; v4 = in4 ? v4 : 0.f;
        }
        const float w1 = t.w[0], w2 = t.w[1], w3 = t.w[2], w4 = t.w[3];
        const float tg = g * a;                               // top_grad * attn_weight
        const float gh = -hw * v1 - lw * v2 + hw * v3 + lw * v4;
        const float gw = -hh * v1 - lh * v3 + hh * v2 + lh * v4;
        ga = g * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
        gx = (float)Wl * gw * tg;
        gy = (float)Hl * gh * tg;
        if (!COUNT) {
          if (in1) unsafeAtomicAdd(gvb + r1, w1 * tg);
          if (in2) unsafeAtomicAdd(gvb + r2, w2 * tg);
          if (in3) unsafeAtomicAdd(gvb + r3, w3 * tg);
          if (in4) unsafeAtomicAdd(gvb + r4, w4 * tg);
        }
      }
      // sum over the point's 32 channels: the half's lanes (fixed order: deterministic)
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
        ga += __shfl_xor(ga, o, 64);
        gx += __shfl_xor(gx, o, 64);
        gy += __shfl_xor(gy, o, 64);
      }
      if (c == 0) {
        gaw[slot] = ga;
        *reinterpret_cast<float2*>(gloc + 2 * slot) = make_float2(gx, gy);
      }
    }
  }
}
