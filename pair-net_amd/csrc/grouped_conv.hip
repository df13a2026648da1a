// Grouped 3x3 convolution, pad 1, stride 1 or 2, channel-last fp32: conv2 of the ResNeXt
// bottlenecks (configs/deformable_detr/pairnet_rnext101_vg.py:9-21 -> mmdet's ResNeXt, third party,
// restated from memory, unpinned), folded BatchNorm as the bias, optional ReLU.
//
//   out[b][oy][ox][g*Cg + co] = act(sum_{ky,kx,ci} in[b][oy*s+ky-1][ox*s+kx-1][g*Cg + ci]
//                                   * Wg[g][co][(ky*3+kx)*Cg + ci] + bias[g*Cg + co])
//
// One workgroup (4 waves) owns GC_TH x 16 output pixels x 64 consecutive channels:
//   * the halo patch those pixels read ((TH-1)s+3 rows x (16-1)s+3 columns x 64 channels) is
//     staged in LDS ONCE and serves all nine taps (zero outside the image and past channel C);
//   * wave w owns output channels [16w, 16w+16) of the 64 and contracts them with
//     v_mfma_f32_16x16x4_f32: D[16 pixels of one output row][16 channels].  Its B operand -- the
//     weights of its 16 channels, 9*CE/4 registers per lane, CE = max(Cg, 16) -- is loaded once
//     and stays in registers; the A operand is one ds_read_b32 per MFMA at a compile-time offset
//     from one per-lane base (pixel = lane & 15, channel = 16j + 4 (lane >> 4) + i);
//   * Cg = 8: a 16-channel tile spans two groups; the B operand is block-diagonal over the 16
//     input channels of both (half the products are exact zeros, see labnotes/r31.md);
//   * four output rows are contracted together (four independent accumulator chains share every
//     weight register), taps ascending, within a tap the channels in the order the float4 weight
//     fetch gives (16j + i, + 4, + 8, + 12 per MFMA): ONE chain of 9*Cg products per output, then
//     the bias.  No atomics, no split: bitwise reproducible.
// LDS row stride: 16 pixels x 2 channel-quads of a ds_read_b32 lane group must hit 32 distinct banks:
// s * LD = 2 (mod 32) -> 66 at stride 1, 65 at stride 2.
#include "common.h"

typedef float f32x4v __attribute__((ext_vector_type(4)));

#define GC_TW 16   // output columns per tile (the MFMA's 16 rows)
#define GC_CW 64   // channels per workgroup

template <int S> struct GcTile {
  static constexpr int TH = S == 1 ? 8 : 4;            // output rows per tile
  static constexpr int PR = (TH - 1) * S + 3;          // patch rows
  static constexpr int PW = (GC_TW - 1) * S + 3;       // patch columns
  static constexpr int LD = S == 1 ? 66 : 65;          // floats per patch pixel
};

template <int CG, int S>
__global__ __launch_bounds__(256) void k_conv3x3_grouped(const float* __restrict__ in,
                                                         const float* __restrict__ Wg,
                                                         const float* __restrict__ bias,
                                                         float* __restrict__ out, int H, int W,
                                                         int Ho, int Wo, int C, int tiles_x,
                                                         int tiles_per_img, int ntiles, int relu) {
  typedef GcTile<S> T;
  constexpr int CE = CG < 16 ? 16 : CG;   // input channels one 16-channel output tile contracts
  constexpr int NJ = CE / 4;              // MFMAs per tap
  constexpr int NK = 9 * NJ;
  __shared__ float patch[T::PR * T::PW * T::LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, q = lane >> 4;
  const int cb = blockIdx.x / ntiles, t = blockIdx.x - cb * ntiles;
  const int b = t / tiles_per_img, rt = t - b * tiles_per_img;
  const int ty = rt / tiles_x, tx = rt - ty * tiles_x;
  const int oy0 = T::TH * ty, ox0 = GC_TW * tx, c0 = GC_CW * cb;

  // ---- this lane's B operand, fetched as float4 (64 contiguous bytes of a weight row per four
  // lanes): MFMA kk = tap * NJ + 4 j + i contracts the window's channels 16 j + 4 q + i, q = 0..3
  // (lane >> 4) -- element i of the float4 at channel 16 j + 4 q ----
  const int co = c0 + 16 * wave + li;
  const bool live = co < C;
  float wf[NK];
  {
    const float* wr = Wg + (int64_t)min(co, C - 1) * (9 * CG);   // Wg is [G][Cg][9 Cg] = [C][9 Cg]
#pragma unroll
    for (int k4 = 0; k4 < NK / 4; ++k4) {
      const int tap = k4 / (NJ / 4), c = 16 * (k4 % (NJ / 4)) + 4 * q;
      // Cg = 8: the window holds two groups, this channel's own is the half li >> 3
      const bool own = CG >= 16 || (c >> 3) == (li >> 3);
      const float4 v = ld4(wr + tap * CG + (c & (CG - 1)));
      wf[4 * k4 + 0] = live && own ? v.x : 0.f;
      wf[4 * k4 + 1] = live && own ? v.y : 0.f;
      wf[4 * k4 + 2] = live && own ? v.z : 0.f;
      wf[4 * k4 + 3] = live && own ? v.w : 0.f;
    }
  }
  const float bv = bias[min(co, C - 1)];

  // ---- stage the patch: 16 float4 per pixel, zero outside the image / past channel C; four
  // loads per thread in flight at a time (all of them at once measured slower at Cg 8 / 16:
  // labnotes/r31.md R31.5) ----
  {
    constexpr int NE = T::PR * T::PW * (GC_CW / 4);
    const int c4 = 4 * (tid & 15);
    const bool cok = c0 + c4 < C;
    for (int e0 = 0; e0 < NE; e0 += 4 * 256) {
      float4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + 256 * j + tid;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < NE) {
          const int pix = e >> 4, pr = pix / T::PW, pc = pix - pr * T::PW;
          const int iy = oy0 * S - 1 + pr, ix = ox0 * S - 1 + pc;
          if (cok && iy >= 0 && iy < H && ix >= 0 && ix < W)
            v[j] = ld4(in + ((b * H + iy) * W + ix) * C + c0 + c4);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = e0 + 256 * j + tid;
        if (e < NE) {
          float* d = patch + (e >> 4) * T::LD + c4;
          d[0] = v[j].x; d[1] = v[j].y; d[2] = v[j].z; d[3] = v[j].w;
        }
      }
    }
  }
  __syncthreads();

  // ---- contract: four output rows at a time, 9 * CE / 4 MFMAs each ----
  const int cin0 = (16 * wave / CE) * CE;   // the window's first channel within the 64
  const float* ap = patch + li * S * T::LD + cin0 + 4 * q;
  const int ox = ox0 + 4 * q;               // D: channel = lane & 15, pixel = 4 (lane >> 4) + reg
  for (int r0 = 0; r0 < T::TH; r0 += 4) {
    if (oy0 + r0 >= Ho) break;
    const float* ar = ap + r0 * S * T::PW * T::LD;
    f32x4v acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) {
      const int tap = kk / NJ, ky = tap / 3, kx = tap - 3 * ky;
      const int j = 16 * ((kk % NJ) / 4) + (kk % NJ) % 4;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(
            ar[((i * S + ky) * T::PW + kx) * T::LD + j], wf[kk], acc[i], 0, 0, 0);
    }
    if (live) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int oy = oy0 + r0 + i;
        if (oy < Ho) {
          float* ob = out + ((b * Ho + oy) * Wo) * C + co;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float v = acc[i][r] + bv;
            if (ox + r < Wo) ob[(ox + r) * C] = relu ? fmaxf(v, 0.f) : v;
          }
        }
      }
    }
  }
}

template <int CG, int S>
static int gc_launch(const float* in, const float* Wg, const float* bias, float* out, int B, int H,
                     int W, int C, int relu, hipStream_t st) {
  typedef GcTile<S> T;
  const int Ho = (H - 1) / S + 1, Wo = (W - 1) / S + 1;
  const int tiles_x = pn_cdiv(Wo, GC_TW), tiles_y = pn_cdiv(Ho, T::TH);
  const int64_t ntiles = (int64_t)B * tiles_x * tiles_y;
  const int64_t grid = ntiles * pn_cdiv(C, GC_CW);
  if (grid >= ((int64_t)1 << 31)) return PN_BAD_ARG;
  hipLaunchKernelGGL((k_conv3x3_grouped<CG, S>), dim3((unsigned)grid), dim3(256), 0, st, in, Wg,
                     bias, out, H, W, Ho, Wo, C, tiles_x, tiles_x * tiles_y, (int)ntiles, relu);
  return PN_LAUNCH_CHECK();
}

// Wg [G][Cg][9 Cg]: the PyTorch weight [G Cg][Cg][3][3] with each row permuted to (ky, kx, ci).
extern "C" int pn_conv2d_grouped_nhwc_f32(const float* in, const float* Wg, const float* bias,
                                          float* out, int B, int H, int W, int G, int Cg, int KH,
                                          int KW, int stride, int flags, void* stream) {
  if (!in || !Wg || !bias || !out || B <= 0 || H <= 0 || W <= 0 || G <= 0) return PN_BAD_ARG;
  if (Cg != 8 && Cg != 16 && Cg != 32 && Cg != 64) return PN_BAD_ARG;
  if (KH != 3 || KW != 3 || (stride != 1 && stride != 2)) return PN_BAD_ARG;
  if (flags & ~PN_GEMM_RELU) return PN_BAD_ARG;
  if (((uintptr_t)in & 15) || ((uintptr_t)out & 3) || ((uintptr_t)Wg & 15) || ((uintptr_t)bias & 3))
    return PN_BAD_ARG;
  // the kernel indexes both maps with int32
  const int64_t C = (int64_t)G * Cg;
  if (C >= ((int64_t)1 << 31) || (int64_t)B * H * W * C >= ((int64_t)1 << 31)) return PN_BAD_ARG;
  const hipStream_t st = (hipStream_t)stream;
  const int relu = flags & PN_GEMM_RELU;
#define GC_CASE(CG)                                                                        \
  case CG:                                                                                 \
    return stride == 1 ? gc_launch<CG, 1>(in, Wg, bias, out, B, H, W, (int)C, relu, st)    \
                       : gc_launch<CG, 2>(in, Wg, bias, out, B, H, W, (int)C, relu, st);
  switch (Cg) {
    GC_CASE(8)
    GC_CASE(16)
    GC_CASE(32)
    GC_CASE(64)
  }
#undef GC_CASE
  return PN_BAD_ARG;
}
