// Backward of the pixel decoder's FPN branch (pair-net_amd/seg_grad.py: SegPixelDecoderGrad): the
// adjoint of the channel-last bilinear upsampling and a GroupNorm (+ReLU) backward blocked for
// the H/4 x W/4 map.  No float atomics: every sum runs in an order that the shapes alone decide.
#include "common.h"

// ---- adjoint of k_bilinear_nhwc (resize.hip), gather form.  thread = (coarse pixel, float4
// channel group).  The fine rows / columns that can tap coarse index i are those with
// src = scale (dst + 0.5) - 0.5 in (i - 1, i + 1): dst in (((2i - 1) out - in) / (2 in),
// ((2i + 3) out - in) / (2 in)), inverted in integers and widened by one on each side (make_tap
// rounds src in fp32).  Membership and weights are make_tap's own, per candidate: i0 == i gives
// l0, i1 == i gives l1, and at the clamped last index (i0 == i1) both land here and are added.
// So this is the transpose of the forward's fp32 tap matrix; columns ascending inside a row
// (fmaf chain), rows ascending (one fmaf per row).
__device__ __forceinline__ int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ void adj_window(int i, int in, int outn, int* lo, int* hi) {
  const int64_t a = ((int64_t)2 * i - 1) * outn - in, b = ((int64_t)2 * i + 3) * outn - in;
  // integers inside the open interval: floor(lo) + 1 .. ceil(hi) - 1; one more on each side
  const int64_t l = floor_div(a, (int64_t)2 * in);
  const int64_t h = floor_div(b + (int64_t)2 * in - 1, (int64_t)2 * in);
  *lo = (int)(l < 0 ? 0 : l);
  *hi = (int)(h > outn - 1 ? outn - 1 : h);
}
__device__ __forceinline__ bool adj_weight(int dst, int i, int in, int outn, float* wgt) {
  const Tap t = make_tap(dst, in, outn);
  float w = 0.f;
  if (t.i0 == i) w = t.l0;
  if (t.i1 == i) w = (t.i0 == i) ? t.l0 + t.l1 : t.l1;
  *wgt = w;
  return t.i0 == i || t.i1 == i;
}

__global__ __launch_bounds__(256) void k_bilinear_nhwc_bwd(const float* __restrict__ dout,
                                                           float* __restrict__ din, int hi, int wi,
                                                           int ho, int wo, int C4, int accumulate,
                                                           int64_t obs, int64_t ibs) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_img = (int64_t)hi * wi * C4;
  if (e >= per_img) return;
  const int b = blockIdx.y;
  const int c4 = (int)(e % C4);
  const int pix = (int)(e / C4);
  const int iy = pix / wi, ix = pix - iy * wi;
  int y0, y1, x0, x1;
  adj_window(iy, hi, ho, &y0, &y1);
  adj_window(ix, wi, wo, &x0, &x1);
  const float* gb = dout + (int64_t)b * obs + c4 * 4;
  const int64_t rs = (int64_t)wo * C4 * 4, cs = (int64_t)C4 * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int oy = y0; oy <= y1; ++oy) {
    float wy;
    if (!adj_weight(oy, iy, hi, ho, &wy)) continue;
    float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ox = x0; ox <= x1; ++ox) {
      float wx;
      if (!adj_weight(ox, ix, wi, wo, &wx)) continue;
      const float4 g = ld4(gb + oy * rs + ox * cs);
      row.x = fmaf(wx, g.x, row.x); row.y = fmaf(wx, g.y, row.y);
      row.z = fmaf(wx, g.z, row.z); row.w = fmaf(wx, g.w, row.w);
    }
    acc.x = fmaf(wy, row.x, acc.x); acc.y = fmaf(wy, row.y, acc.y);
    acc.z = fmaf(wy, row.z, acc.z); acc.w = fmaf(wy, row.w, acc.w);
  }
  float* o = din + (int64_t)b * ibs + (int64_t)pix * C4 * 4 + c4 * 4;
  if (accumulate) acc = add4(ld4(o), acc);
  st4(o, acc);
}

extern "C" int pn_bilinear_nhwc_bwd_f32(const float* dout, float* din, int B, int hi, int wi,
                                        int ho, int wo, int C, int accumulate,
                                        int64_t dout_bstride, int64_t din_bstride, void* stream) {
  if (!dout || !din || B <= 0 || B > 65535 || hi <= 0 || wi <= 0 || ho <= 0 || wo <= 0 ||
      C <= 0 || (C & 3))
    return PN_BAD_ARG;
  if (ho < hi || wo < wi) return PN_BAD_ARG;          // the adjoint of an UPsampling only
  if ((dout_bstride | din_bstride) & 3) return PN_BAD_ARG;
  if ((int64_t)ho * wo * C > 2147483647) return PN_BAD_ARG;   // (pixel indices are 32-bit)
  const int64_t per_img = (int64_t)hi * wi * (C / 4);
  hipLaunchKernelGGL(k_bilinear_nhwc_bwd, dim3(pn_cdiv(per_img, 256), B), dim3(256), 0,
                     (hipStream_t)stream, dout, din, hi, wi, ho, wo, C / 4, accumulate,
                     dout_bstride, din_bstride);
  return PN_LAUNCH_CHECK();
}

// ---- GroupNorm (+ReLU) backward over channel-last x[b][HW][256] on the forward's own blocking
// (norm.hip: GNB_PIX pixels per workgroup, 16 waves, a float4 channel group per lane), for maps
// where one workgroup per (image, group) leaves most of the chip idle.  With gate = relu ?
// (y > 0) : 1 and g = gamma dy gate:
//   pass 1  per (image, block, group) double partials of (sum x, sum x^2, sum g, sum g x)
//   pass 2  per (image, group): blocks added in ascending order -> (mean, rstd, m1, m2),
//           m1 = mean(g), m2 = mean(g xhat) = rstd (sum g x - mean sum g) / n
//   pass 3  dx = rstd (g - m1 - xhat m2); per-block column partials of dy gate xhat and dy gate
//   pass 4  the column partials added in a fixed order -> d gamma, d beta (optionally += )
#define GNB_PIX 256
#define GNB_SUB 16
#define GNB_CH 4      // pixels per thread in flight together (x, dy, y: 12 float4)

__device__ __forceinline__ float4 gate4(const float4 d, const float4 y, const int relu) {
  if (!relu) return d;
  return make_float4(y.x > 0.f ? d.x : 0.f, y.y > 0.f ? d.y : 0.f, y.z > 0.f ? d.z : 0.f,
                     y.w > 0.f ? d.w : 0.f);
}

__global__ __launch_bounds__(64 * GNB_SUB) void k_gnact_bwd_partial(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ gamma, double* __restrict__ partials, int64_t HW, int G, int relu,
    int64_t xbs, int64_t dbs) {
  __shared__ double red[GNB_SUB][64][4];
  const int tid = threadIdx.x, c4 = tid & 63, sub = tid >> 6;
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * GNB_PIX;
  const float* xb = x + (int64_t)b * xbs + c4 * 4;
  const float* db = dy + (int64_t)b * dbs + c4 * 4;
  const float* yb = relu ? y + (int64_t)b * HW * 256 + c4 * 4 : nullptr;
  const float4 gg = ld4(gamma + c4 * 4);
  double s = 0.0, ss = 0.0, sg = 0.0, sgx = 0.0;
  constexpr int NP = GNB_PIX / GNB_SUB;
  for (int j0 = 0; j0 < NP; j0 += GNB_CH) {
    float4 xv[GNB_CH], dv[GNB_CH], yv[GNB_CH];
#pragma unroll
    for (int j = 0; j < GNB_CH; ++j) {        // all loads first, unconditional (clamped)
      const int64_t pix = min(p0 + sub + (int64_t)(j0 + j) * GNB_SUB, HW - 1);
      xv[j] = ld4(xb + pix * 256);
      dv[j] = ld4(db + pix * 256);
      yv[j] = relu ? ld4(yb + pix * 256) : xv[j];
    }
#pragma unroll
    for (int j = 0; j < GNB_CH; ++j) {
      if (p0 + sub + (int64_t)(j0 + j) * GNB_SUB < HW) {
        const float4 d = gate4(dv[j], yv[j], relu);
        const double x0 = xv[j].x, x1 = xv[j].y, x2 = xv[j].z, x3 = xv[j].w;
        const double g0 = (double)gg.x * (double)d.x, g1 = (double)gg.y * (double)d.y;
        const double g2 = (double)gg.z * (double)d.z, g3 = (double)gg.w * (double)d.w;
        s += (x0 + x1) + (x2 + x3);
        ss += (x0 * x0 + x1 * x1) + (x2 * x2 + x3 * x3);
        sg += (g0 + g1) + (g2 + g3);
        sgx += (g0 * x0 + g1 * x1) + (g2 * x2 + g3 * x3);
      }
    }
  }
  red[sub][c4][0] = s; red[sub][c4][1] = ss; red[sub][c4][2] = sg; red[sub][c4][3] = sgx;
  __syncthreads();
  const int lanes_per_group = (256 / G) / 4;
  if (tid < G * 4) {
    const int g = tid >> 2, which = tid & 3;
    double t = 0.0;
    for (int l = 0; l < lanes_per_group; ++l)
      for (int k = 0; k < GNB_SUB; ++k) t += red[k][g * lanes_per_group + l][which];
    partials[(((int64_t)b * gridDim.x + blockIdx.x) * G + g) * 4 + which] = t;
  }
}

__global__ __launch_bounds__(64) void k_gnact_bwd_finalize(const double* __restrict__ partials,
                                                           float* __restrict__ stats, int64_t HW,
                                                           int G, int nblk, float eps) {
  const int g = threadIdx.x, b = blockIdx.x;
  if (g >= G) return;
  double s = 0.0, ss = 0.0, sg = 0.0, sgx = 0.0;
  for (int i = 0; i < nblk; ++i) {
    const double* p = partials + (((int64_t)b * nblk + i) * G + g) * 4;
    s += p[0]; ss += p[1]; sg += p[2]; sgx += p[3];
  }
  const double n = (double)HW * (double)(256 / G);
  const double mean = s / n;
  const double var = fmax(ss / n - mean * mean, 0.0);
  const double rstd = 1.0 / sqrt(var + (double)eps);
  float* st = stats + ((int64_t)b * G + g) * 4;
  st[0] = (float)mean; st[1] = (float)rstd;
  st[2] = (float)(sg / n); st[3] = (float)(rstd * (sgx - mean * sg) / n);
}

__global__ __launch_bounds__(64 * GNB_SUB) void k_gnact_bwd_apply(
    const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
    const float* __restrict__ gamma, const float* __restrict__ stats, float* __restrict__ dx,
    float* __restrict__ colpart, int64_t HW, int G, int relu, int64_t xbs, int64_t dbs) {
  __shared__ float4 red[GNB_SUB][64][2];
  const int tid = threadIdx.x, c4 = tid & 63, sub = tid >> 6;
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * GNB_PIX;
  const float* xb = x + (int64_t)b * xbs + c4 * 4;
  const float* db = dy + (int64_t)b * dbs + c4 * 4;
  const float* yb = relu ? y + (int64_t)b * HW * 256 + c4 * 4 : nullptr;
  float* ob = dx + (int64_t)b * HW * 256 + c4 * 4;
  const float4 gg = ld4(gamma + c4 * 4);
  const float4 st = ld4(stats + ((int64_t)b * G + (c4 * 4) / (256 / G)) * 4);
  const float mean = st.x, rstd = st.y, m1 = st.z, m2 = st.w;
  float4 sgx = make_float4(0.f, 0.f, 0.f, 0.f), sd = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int NP = GNB_PIX / GNB_SUB;
  for (int j0 = 0; j0 < NP; j0 += GNB_CH) {
    float4 xv[GNB_CH], dv[GNB_CH], yv[GNB_CH];
#pragma unroll
    for (int j = 0; j < GNB_CH; ++j) {
      const int64_t pix = min(p0 + sub + (int64_t)(j0 + j) * GNB_SUB, HW - 1);
      xv[j] = ld4(xb + pix * 256);
      dv[j] = ld4(db + pix * 256);
      yv[j] = relu ? ld4(yb + pix * 256) : xv[j];
    }
#pragma unroll
    for (int j = 0; j < GNB_CH; ++j) {
      const int64_t pix = p0 + sub + (int64_t)(j0 + j) * GNB_SUB;
      if (pix < HW) {
        const float4 d = gate4(dv[j], yv[j], relu);
        float4 o;
#define GNB_ONE(c)                                              \
        {                                                       \
          const float xh = (xv[j].c - mean) * rstd;             \
          o.c = rstd * (gg.c * d.c - m1 - xh * m2);             \
          sgx.c += d.c * xh;                                    \
          sd.c += d.c;                                          \
        }
        GNB_ONE(x) GNB_ONE(y) GNB_ONE(z) GNB_ONE(w)
#undef GNB_ONE
        st4(ob + pix * 256, o);
      }
    }
  }
  red[sub][c4][0] = sgx;
  red[sub][c4][1] = sd;
  __syncthreads();
  if (tid < 128) {
    const int l = tid & 63, which = tid >> 6;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < GNB_SUB; ++k) t = add4(t, red[k][l][which]);
    st4(colpart + (((int64_t)b * gridDim.x + blockIdx.x) * 2 + which) * 256 + l * 4, t);
  }
}

// colpart rows [image][block][d gamma | d beta][256]: column c of `which` summed over the rows in
// ascending order on four interleaved lanes (double), the lanes added 0..3.
__global__ __launch_bounds__(256) void k_gnact_bwd_colreduce(const float* __restrict__ colpart,
                                                             float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta,
                                                             int64_t rows, int accumulate) {
  __shared__ double red[4][64];
  const int col = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;   // col < 512
  const int which = col >> 8, c = col & 255;
  double t = 0.0;
  for (int64_t r = part; r < rows; r += 4) t += (double)colpart[(r * 2 + which) * 256 + c];
  red[part][threadIdx.x & 63] = t;
  __syncthreads();
  if (part == 0) {
    const int l = threadIdx.x & 63;
    const float v = (float)(((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]);
    float* o = (which ? dbeta : dgamma) + c;
    *o = accumulate ? *o + v : v;
  }
}

extern "C" int pn_groupnorm_act_nhwc_bwd_f32(const float* x, const float* dy, const float* y,
                                             const float* gamma, float* dx, float* dgamma,
                                             float* dbeta, float* stats, double* partials,
                                             float* colpart, int B, int64_t HW, int G, float eps,
                                             int relu, int accumulate, int64_t x_bstride,
                                             int64_t dy_bstride, void* stream) {
  if (!x || !dy || !gamma || !dx || !dgamma || !dbeta || !stats || !partials || !colpart ||
      (relu && !y) || B <= 0 || B > 65535 || HW <= 0 || HW > 2147483647 || G <= 0 || 256 % G)
    return PN_BAD_ARG;
  // the forward's blocking: a float4 channel group lies inside one group
  if (G > 32 || (256 / G) % 4 || ((x_bstride | dy_bstride) & 3)) return PN_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = pn_cdiv(HW, GNB_PIX);
  dim3 grid(nblk, B);
  hipLaunchKernelGGL(k_gnact_bwd_partial, grid, dim3(64 * GNB_SUB), 0, s, x, dy, y, gamma,
                     partials, HW, G, relu, x_bstride, dy_bstride);
  hipLaunchKernelGGL(k_gnact_bwd_finalize, dim3(B), dim3(64), 0, s, partials, stats, HW, G, nblk,
                     eps);
  hipLaunchKernelGGL(k_gnact_bwd_apply, grid, dim3(64 * GNB_SUB), 0, s, x, dy, y, gamma, stats, dx,
                     colpart, HW, G, relu, x_bstride, dy_bstride);
  hipLaunchKernelGGL(k_gnact_bwd_colreduce, dim3(8), dim3(256), 0, s, colpart, dgamma, dbeta,
                     (int64_t)B * nblk, accumulate);
  return PN_LAUNCH_CHECK();
}
