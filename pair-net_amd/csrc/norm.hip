// Row / group normalisations (HBM-bound; one pass over the data each, fp32 I/O).
#include "common.h"

// One wave per 256-channel row: lane holds one float4.  Two-pass moments in
// registers (mean, then centred variance), like torch's CPU LayerNorm.
__global__ __launch_bounds__(256) void k_layernorm256(const float* __restrict__ x,
                                                       const float* __restrict__ g,
                                                       const float* __restrict__ b,
                                                       float* __restrict__ y,
                                                       int64_t rows, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4 v = ld4(x + row * 256 + lane * 4);
  const float4 gg = ld4(g + lane * 4), bb = ld4(b + lane * 4);
  st4(y + row * 256 + lane * 4, ln256_row(v, gg, bb, eps));
}

extern "C" int pn_layernorm_f32(const float* x, const float* gamma, const float* beta,
                                float* y, int64_t rows, int C, float eps, void* stream) {
  if (!x || !gamma || !beta || !y || C != 256 || rows <= 0) return PN_BAD_ARG;
  hipLaunchKernelGGL(k_layernorm256, dim3(pn_cdiv(rows, 4)), dim3(256), 0,
                     (hipStream_t)stream, x, gamma, beta, y, rows, eps);
  return PN_LAUNCH_CHECK();
}

// ---- GroupNorm, channel-last, C == 256 (64 float4 lanes per pixel) ----
// Pass 1: each block reduces GN_PIX pixels x 256 channels to per-group (sum, sumsq)
// in fp64 (exact enough that E[x^2]-E[x]^2 is safe) and writes them to `partials`.
// Pass 2: every block re-reduces the (small) partials of its image in a fixed order
// -> mean / rstd per group, then normalises its own pixels.  Deterministic.
// 16 waves per block: a 66 800-pixel map is only 261 blocks (about one per CU), so the
// block itself has to supply the memory-level parallelism.
#define GN_PIX 256
#define GN_SUB 16   // waves per block = pixel sub-lanes

extern "C" int pn_groupnorm_nblk(int64_t HW) { return pn_cdiv(HW, GN_PIX); }

__global__ __launch_bounds__(64 * GN_SUB) void k_gn_partial(const float* __restrict__ x,
                                                            double* __restrict__ partials,
                                                            int64_t HW, int G, int64_t xbs) {
  __shared__ double red[GN_SUB][64][2];
  const int tid = threadIdx.x, c4 = tid & 63, sub = tid >> 6;
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * GN_PIX;
  const float* xb = x + (int64_t)b * xbs;
  // all loads first, unconditional (clamped; hipcc serialises predicated loads)
  constexpr int NP = GN_PIX / GN_SUB;
  float4 v[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j)
    v[j] = ld4(xb + min(p0 + sub + j * GN_SUB, HW - 1) * 256 + c4 * 4);
  double s = 0.0, ss = 0.0;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (p0 + sub + j * GN_SUB < HW) {
      s += ((double)v[j].x + (double)v[j].y) + ((double)v[j].z + (double)v[j].w);
      ss += ((double)v[j].x * v[j].x + (double)v[j].y * v[j].y) +
            ((double)v[j].z * v[j].z + (double)v[j].w * v[j].w);
    }
  }
  red[sub][c4][0] = s;
  red[sub][c4][1] = ss;
  __syncthreads();
  // group g owns channels [g*cpg, (g+1)*cpg) = float4 lanes [g*cpg/4, ...)
  const int lanes_per_group = (256 / G) / 4;
  if (tid < G * 2) {
    const int g = tid >> 1, which = tid & 1;
    double t = 0.0;
    for (int l = 0; l < lanes_per_group; ++l)
      for (int k = 0; k < GN_SUB; ++k) t += red[k][g * lanes_per_group + l][which];
    partials[(((int64_t)b * gridDim.x + blockIdx.x) * G + g) * 2 + which] = t;
  }
}

__global__ __launch_bounds__(64 * GN_SUB) void k_gn_apply(const float* __restrict__ x,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta,
                                                          float* __restrict__ y,
                                                          const double* __restrict__ partials,
                                                          int64_t HW, int G, float eps, int relu,
                                                          int64_t xbs, int64_t ybs) {
  __shared__ double acc[GN_SUB][64];
  __shared__ float stat[64][2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nblk = gridDim.x;
  {  // reduce partials of image b: 2G columns, 4 row-strided lanes each
    const int col = tid & 63, part = tid >> 6;
    double t = 0.0;
    if (col < 2 * G)
      for (int i = part; i < nblk; i += GN_SUB)
        t += partials[((int64_t)b * nblk + i) * G * 2 + col];
    acc[part][col] = t;
  }
  __syncthreads();
  if (tid < G) {
    const double n = (double)HW * (256 / G);
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < GN_SUB; ++k) {
      s += acc[k][2 * tid];
      ss += acc[k][2 * tid + 1];
    }
    const double mean = s / n;
    double var = ss / n - mean * mean;
    if (var < 0.0) var = 0.0;
    stat[tid][0] = (float)mean;
    stat[tid][1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  const int c4 = tid & 63, sub = tid >> 6;
  const int g = (c4 * 4) / (256 / G);
  const float mean = stat[g][0], rstd = stat[g][1];
  const float4 gg = ld4(gamma + c4 * 4), bb = ld4(beta + c4 * 4);
  const int64_t p0 = (int64_t)blockIdx.x * GN_PIX;
  const float* xb = x + (int64_t)b * xbs;
  float* yb = y + (int64_t)b * ybs;
  constexpr int NP = GN_PIX / GN_SUB;
  float4 v[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j)
    v[j] = ld4(xb + min(p0 + sub + j * GN_SUB, HW - 1) * 256 + c4 * 4);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int64_t pix = p0 + sub + j * GN_SUB;
    float4 o = make_float4((v[j].x - mean) * rstd * gg.x + bb.x, (v[j].y - mean) * rstd * gg.y + bb.y,
                           (v[j].z - mean) * rstd * gg.z + bb.z, (v[j].w - mean) * rstd * gg.w + bb.w);
    if (relu) {
      o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f);
      o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    }
    if (pix < HW) st4(yb + pix * 256 + c4 * 4, o);
  }
}

extern "C" int pn_groupnorm_nhwc_f32(const float* x, const float* gamma, const float* beta,
                                     float* y, double* partials, int B, int64_t HW, int C,
                                     int G, float eps, int relu, int64_t x_bstride,
                                     int64_t y_bstride, void* stream) {
  if (!x || !gamma || !beta || !y || !partials) return PN_BAD_ARG;
  if (C != 256 || G <= 0 || G > 32 || 256 % G || (256 / G) % 4 || B <= 0 || HW <= 0)
    return PN_BAD_ARG;
  if ((x_bstride | y_bstride) & 3) return PN_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(pn_groupnorm_nblk(HW), B);
  hipLaunchKernelGGL(k_gn_partial, grid, dim3(64 * GN_SUB), 0, s, x, partials, HW, G, x_bstride);
  hipLaunchKernelGGL(k_gn_apply, grid, dim3(64 * GN_SUB), 0, s, x, gamma, beta, y, partials, HW, G,
                     eps, relu, x_bstride, y_bstride);
  return PN_LAUNCH_CHECK();
}

// k_gn_apply (no ReLU) + the accumulate pass of k_bilinear_nhwc (resize.hip) in one pass over
// the map: y = GN(x) + bilinear-up(coarse), the FPN's top-down add.  The same operations in the
// same order as the two kernels -- the normalised value is rounded to fp32 exactly as k_gn_apply
// stores it, the sample exactly as k_bilinear_nhwc forms it, then one add -- so the result is bit
// for bit theirs; the two values pass through empty asm statements so that the compiler cannot
// contract anything across the add that the two-kernel form could not.
#define GN_UP_CH 4   // pixels per thread whose loads are in flight together
__global__ __launch_bounds__(64 * GN_SUB) void k_gn_apply_up(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ y, const double* __restrict__ partials, const float* __restrict__ coarse,
    int64_t HW, int Wf, int hc, int wc, int Hf, int G, float eps, int64_t xbs, int64_t ybs,
    int64_t cbs) {
  __shared__ double acc[GN_SUB][64];
  __shared__ float stat[64][2];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int nblk = gridDim.x;
  {  // reduce partials of image b (k_gn_apply's order)
    const int col = tid & 63, part = tid >> 6;
    double t = 0.0;
    if (col < 2 * G)
      for (int i = part; i < nblk; i += GN_SUB)
        t += partials[((int64_t)b * nblk + i) * G * 2 + col];
    acc[part][col] = t;
  }
  __syncthreads();
  if (tid < G) {
    const double n = (double)HW * (256 / G);
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < GN_SUB; ++k) {
      s += acc[k][2 * tid];
      ss += acc[k][2 * tid + 1];
    }
    const double mean = s / n;
    double var = ss / n - mean * mean;
    if (var < 0.0) var = 0.0;
    stat[tid][0] = (float)mean;
    stat[tid][1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
  const int c4 = tid & 63, sub = tid >> 6;
  const int g = (c4 * 4) / (256 / G);
  const float mean = stat[g][0], rstd = stat[g][1];
  const float4 gg = ld4(gamma + c4 * 4), bb = ld4(beta + c4 * 4);
  const int64_t p0 = (int64_t)blockIdx.x * GN_PIX;
  const float* xb = x + (int64_t)b * xbs;
  float* yb = y + (int64_t)b * ybs;
  const float* ib = coarse + (int64_t)b * cbs + c4 * 4;
  const int64_t rs = (int64_t)wc * 256, cs = 256;
  constexpr int NP = GN_PIX / GN_SUB;
#pragma unroll
  for (int j0 = 0; j0 < NP; j0 += GN_UP_CH) {
    float4 v[GN_UP_CH], v00[GN_UP_CH], v01[GN_UP_CH], v10[GN_UP_CH], v11[GN_UP_CH];
    Tap tys[GN_UP_CH], txs[GN_UP_CH];
#pragma unroll
    for (int j = 0; j < GN_UP_CH; ++j) {   // all loads first, unconditional (clamped)
      const int pix = (int)min(p0 + sub + (j0 + j) * GN_SUB, HW - 1);
      const int oy = pix / Wf, ox = pix - oy * Wf;
      const Tap ty = make_tap(oy, hc, Hf), tx = make_tap(ox, wc, Wf);
      tys[j] = ty; txs[j] = tx;
      v[j] = ld4(xb + (int64_t)pix * 256 + c4 * 4);
      v00[j] = ld4(ib + ty.i0 * rs + tx.i0 * cs); v01[j] = ld4(ib + ty.i0 * rs + tx.i1 * cs);
      v10[j] = ld4(ib + ty.i1 * rs + tx.i0 * cs); v11[j] = ld4(ib + ty.i1 * rs + tx.i1 * cs);
    }
#pragma unroll
    for (int j = 0; j < GN_UP_CH; ++j) {
      const int64_t pix = p0 + sub + (j0 + j) * GN_SUB;
      const Tap ty = tys[j], tx = txs[j];
      // Written out as the fmaf chains the two kernels compile to (which product of a sum the
      // compiler folds into the fma decides the rounding): GN = fma(gamma, (x - mean) rstd, beta);
      // sample: top = fma(l1x, v01, l0x v00), bottom = fma(l0x, v10, l1x v11),
      // r = fma(l0y, top, l1y bottom).  The test compares against the pair bit for bit.
#define GN_O(c) fmaf((v[j].c - mean) * rstd, gg.c, bb.c)
#define UP_R(c) fmaf(ty.l0, fmaf(tx.l1, v01[j].c, tx.l0 * v00[j].c), \
                     ty.l1 * fmaf(tx.l0, v10[j].c, tx.l1 * v11[j].c))
      float4 o = make_float4(GN_O(x), GN_O(y), GN_O(z), GN_O(w));
      float4 r = make_float4(UP_R(x), UP_R(y), UP_R(z), UP_R(w));
#undef GN_O
#undef UP_R
      asm volatile("" : "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w));
      asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
      if (pix < HW) st4(yb + pix * 256 + c4 * 4, add4(o, r));
    }
  }
}

extern "C" int pn_groupnorm_upadd_nhwc_f32(const float* x, const float* gamma, const float* beta,
                                           float* y, double* partials, const float* coarse, int B,
                                           int H, int W, int hc, int wc, int C, int G, float eps,
                                           int64_t x_bstride, int64_t y_bstride,
                                           int64_t coarse_bstride, void* stream) {
  if (!x || !gamma || !beta || !y || !partials || !coarse) return PN_BAD_ARG;
  if (C != 256 || G <= 0 || G > 32 || 256 % G || (256 / G) % 4 || B <= 0 || B > 65535 || H <= 0 ||
      W <= 0 || hc <= 0 || wc <= 0)
    return PN_BAD_ARG;
  if ((x_bstride | y_bstride | coarse_bstride) & 3) return PN_BAD_ARG;
  const int64_t HW = (int64_t)H * W;
  if (HW >= ((int64_t)1 << 31)) return PN_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid(pn_groupnorm_nblk(HW), B);
  hipLaunchKernelGGL(k_gn_partial, grid, dim3(64 * GN_SUB), 0, s, x, partials, HW, G, x_bstride);
  hipLaunchKernelGGL(k_gn_apply_up, grid, dim3(64 * GN_SUB), 0, s, x, gamma, beta, y, partials,
                     coarse, HW, W, hc, wc, H, G, eps, x_bstride, y_bstride, coarse_bstride);
  return PN_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void k_l2norm256(const float* __restrict__ x,
                                                   float* __restrict__ y, int64_t rows,
                                                   float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float4 v = ld4(x + row * 256 + lane * 4);
  const float n = sqrtf(wave_sum((v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w)));
  const float d = fmaxf(n, eps);
  st4(y + row * 256 + lane * 4, make_float4(v.x / d, v.y / d, v.z / d, v.w / d));
}

extern "C" int pn_l2normalize_f32(const float* x, float* y, int64_t rows, int C, float eps,
                                  void* stream) {
  if (!x || !y || C != 256 || rows <= 0) return PN_BAD_ARG;
  hipLaunchKernelGGL(k_l2norm256, dim3(pn_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                     x, y, rows, eps);
  return PN_LAUNCH_CHECK();
}
