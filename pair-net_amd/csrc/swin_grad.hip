// Backward kernels of the Swin backbone's trainable last stage (configs/mask2former/
// pairnet_swinb.py:201-240 with frozen_stages=3: the two blocks of stages.3 and norm3 train;
// [3P] mmdet 2.25.1 SwinBlock / ShiftWindowMSA / WindowMSA).  pair-net_amd/grad.py
// SwinBackboneGrad composes them with pn_gemm_f32 (the linear layers' dX / dW), pn_colsum_f32
// (bias / norm / bias-table reductions) and pn_scale_rows_f32 (drop path):
//   k_ln_rows_bwd        LayerNorm backward over rows of any width C % 4 == 0, C <= 3072
//   k_gelu / k_gelu_bwd  exact (erf) GELU and its derivative
//   k_window_attn_bwd    (shifted-)window attention backward: dq / dk / dv over the padded,
//                        un-shifted token grid and per-(image, window, head) partials of the
//                        relative-position-bias-table gradient
//   k_patch_merge_ln_bwd  backward of the fused 2x2 gather + LayerNorm(4C) of patch merging
//                        (pn_patch_merge_ln_f32): dx over the un-merged map, per-workgroup
//                        partials of d gamma / d beta (grad.py SwinStagesGrad: every stage trains)
// All sums run in a fixed order (no atomics): the gradients are bitwise reproducible.
#include "common.h"

#define LNB_MAXV 12  // float4 per lane: C <= 64 * 4 * 12 = 3072

// ---- LayerNorm backward, one wave per row.  y = xhat gamma + beta, xhat = (x - mean) rstd with
// the moments recomputed from the saved input as k_ln_rows (swin.hip) computes them:
//   dx = rstd (g - mean(g) - xhat mean(g xhat)),  g = dy gamma;   gxhat = dy xhat
__global__ __launch_bounds__(256) void k_ln_rows_bwd(const float* __restrict__ dy, int64_t lddy,
                                                     const float* __restrict__ x, int64_t ldx,
                                                     const float* __restrict__ gamma,
                                                     float* __restrict__ dx, int64_t lddx,
                                                     float* __restrict__ gxhat, int64_t ldg,
                                                     int64_t rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int nv = (C + 255) >> 8;
  float4 v[LNB_MAXV], d[LNB_MAXV];
#pragma unroll
  for (int i = 0; i < LNB_MAXV; ++i) {
    const int c = i * 256 + lane * 4;
    v[i] = d[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nv && c < C) {
      v[i] = ld4(x + row * ldx + c);
      d[i] = ld4(dy + row * lddy + c);
    }
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LNB_MAXV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mean = wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < LNB_MAXV; ++i) {
    const int c = i * 256 + lane * 4;
    if (i < nv && c < C) {
      v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
      ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    }
  }
  const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)C + eps);
  float m1 = 0.f, m2 = 0.f;
#pragma unroll
  for (int i = 0; i < LNB_MAXV; ++i) {
    const int c = i * 256 + lane * 4;
    if (i < nv && c < C) {
      const float4 g = ld4(gamma + c);
      v[i] = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);   // xhat
      const float4 gd = make_float4(d[i].x * g.x, d[i].y * g.y, d[i].z * g.z, d[i].w * g.w);
      st4(gxhat + row * ldg + c, make_float4(d[i].x * v[i].x, d[i].y * v[i].y, d[i].z * v[i].z,
                                             d[i].w * v[i].w));
      d[i] = gd;
      m1 += (gd.x + gd.y) + (gd.z + gd.w);
      m2 += (gd.x * v[i].x + gd.y * v[i].y) + (gd.z * v[i].z + gd.w * v[i].w);
    }
  }
  m1 = wave_sum(m1) / (float)C;
  m2 = wave_sum(m2) / (float)C;
#pragma unroll
  for (int i = 0; i < LNB_MAXV; ++i) {
    const int c = i * 256 + lane * 4;
    if (i < nv && c < C)
      st4(dx + row * lddx + c, make_float4(rstd * (d[i].x - m1 - v[i].x * m2),
                                           rstd * (d[i].y - m1 - v[i].y * m2),
                                           rstd * (d[i].z - m1 - v[i].z * m2),
                                           rstd * (d[i].w - m1 - v[i].w * m2)));
  }
}

extern "C" int pn_layernorm_rows_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                                         const float* gamma, float* dx, int64_t lddx, float* gxhat,
                                         int64_t ldg, int64_t rows, int C, float eps, void* stream) {
  if (!dy || !x || !gamma || !dx || !gxhat || rows <= 0 || C <= 0 || (C & 3) ||
      C > 256 * LNB_MAXV || lddy < C || ldx < C || lddx < C || ldg < C ||
      ((lddy | ldx | lddx | ldg) & 3))
    return PN_BAD_ARG;
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)gxhat) & 15)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_ln_rows_bwd, dim3(pn_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, dy,
                     lddy, x, ldx, gamma, dx, lddx, gxhat, ldg, rows, C, eps);
  return PN_LAUNCH_CHECK();
}

// ---- patch merging: backward of the fused gather + LayerNorm (k_ln_rows<MERGE>, swin.hip) -------
// Merged row (b, y2, x2) = [x(2y2, 2x2) | x(2y2, 2x2+1) | x(2y2+1, 2x2) | x(2y2+1, 2x2+1)], zeros
// beyond an odd map's edge; gamma in the same neighbour-major order.  Every token of the H x W
// map belongs to exactly one merged row, so the adjoint of the gather is a permutation: the wave
// that owns a merged row writes the (up to) four C-runs of dx it was gathered from, each exactly
// once, and nothing else does.  The [rows][4C] gathered input is never formed: the row is
// re-gathered from x into registers and its moments recomputed as the forward computes them.  A
// padding position's xhat = -mean rstd is NOT zero: it stays in the row's two backward sums and
// in d gamma / d beta, only its dx has nowhere to go and is dropped.
// One wave per merged row at a time, NV float4 per lane (4C <= 256 NV); a workgroup's four waves
// walk rows blockIdx.x * 4 + wave, + 4 gridDim.x, ... and keep their sums of dy xhat and dy in
// registers.  At the end the waves are added in the order ((0 + 1) + 2) + 3 through LDS and the
// workgroup writes ONE partial row [2][4C] (dy xhat | dy): pn_colsum_f32 over the [nblocks] rows
// gives d gamma | d beta in a fixed order.  Row reductions are cross-lane (wave_sum), no LDS.
struct MergeBP { int H, W, H2, W2, C; };

template <int NV>
__global__ __launch_bounds__(256) void k_patch_merge_ln_bwd(const float* __restrict__ dy,
                                                            const float* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            float* dx, float* __restrict__ part,
                                                            int64_t rows, MergeBP mp, float eps,
                                                            int accumulate) {
  extern __shared__ __attribute__((aligned(16))) float red[];     // [2][4C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C4 = 4 * mp.C;
  const int64_t per = (int64_t)mp.H2 * mp.W2;
  float4 ag[NV], ab[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) ag[i] = ab[i] = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t img = row / per;
    const int r = (int)(row - img * per);
    const int y2 = r / mp.W2, x2 = r - y2 * mp.W2;
    // element offset of this lane's i-th float4 in x / dx, -1: padding (or past the row)
    auto src = [&](int c) -> int64_t {
      const int q = c / mp.C, cc = c - q * mp.C;
      const int yy = 2 * y2 + (q >> 1), xx = 2 * x2 + (q & 1);
      return (yy < mp.H && xx < mp.W) ? ((img * mp.H + yy) * mp.W + xx) * mp.C + cc : -1;
    };
    float4 v[NV], d[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
      v[i] = d[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < C4) {
        const int64_t o = src(c);
        if (o >= 0) v[i] = ld4(x + o);
        d[i] = ld4(dy + row * C4 + c);
      }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) / (float)C4;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
      if (c < C4) {
        v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
        ss += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
      }
    }
    const float rstd = 1.f / sqrtf(wave_sum(ss) / (float)C4 + eps);
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
      if (c < C4) {
        const float4 g = ld4(gamma + c);
        v[i] = make_float4(v[i].x * rstd, v[i].y * rstd, v[i].z * rstd, v[i].w * rstd);   // xhat
        ag[i].x += d[i].x * v[i].x; ag[i].y += d[i].y * v[i].y;
        ag[i].z += d[i].z * v[i].z; ag[i].w += d[i].w * v[i].w;
        ab[i] = add4(ab[i], d[i]);
        d[i] = make_float4(d[i].x * g.x, d[i].y * g.y, d[i].z * g.z, d[i].w * g.w);
        m1 += (d[i].x + d[i].y) + (d[i].z + d[i].w);
        m2 += (d[i].x * v[i].x + d[i].y * v[i].y) + (d[i].z * v[i].z + d[i].w * v[i].w);
      }
    }
    m1 = wave_sum(m1) / (float)C4;
    m2 = wave_sum(m2) / (float)C4;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = i * 256 + lane * 4;
      const int64_t o = c < C4 ? src(c) : -1;
      if (o >= 0) {
        float4 t = make_float4(rstd * (d[i].x - m1 - v[i].x * m2), rstd * (d[i].y - m1 - v[i].y * m2),
                               rstd * (d[i].z - m1 - v[i].z * m2), rstd * (d[i].w - m1 - v[i].w * m2));
        if (accumulate) t = add4(ld4(dx + o), t);
        st4(dx + o, t);
      }
    }
  }

  // the four waves' sums in the order ((0 + 1) + 2) + 3; wave 3 writes the workgroup's partial
  // (every wave reaches every barrier: the row loop has no early exit)
  float* out = part + (int64_t)blockIdx.x * 2 * C4;
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        if (c < C4) {
          float4 a = ag[i], b = ab[i];
          if (w > 0) {
            a = add4(ld4(red + c), a);
            b = add4(ld4(red + C4 + c), b);
          }
          st4((w < 3 ? red : out) + c, a);
          st4((w < 3 ? red : out) + C4 + c, b);
        }
      }
    }
    __syncthreads();
  }
}

extern "C" int pn_patch_merge_ln_bwd_f32(const float* dy, const float* x, const float* gamma,
                                         float* dx, float* part, int nblocks, int B, int H, int W,
                                         int C, float eps, int accumulate, void* stream) {
  if (!dy || !x || !gamma || !dx || !part || B <= 0 || H < 1 || W < 1 || C <= 0 || (C & 3) ||
      4 * C > 256 * LNB_MAXV || nblocks < 1 || nblocks > 65535)
    return PN_BAD_ARG;
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)part) & 15)
    return PN_BAD_ARG;
  const MergeBP mp{H, W, (H + 1) / 2, (W + 1) / 2, C};
  const int64_t rows = (int64_t)B * mp.H2 * mp.W2;
  const int nv = (4 * C + 255) >> 8;
  const size_t lds = (size_t)8 * C * sizeof(float);
  const dim3 grid(nblocks), block(256);
  hipStream_t s = (hipStream_t)stream;
#define PMB_LAUNCH(NV)                                                                          \
  hipLaunchKernelGGL(k_patch_merge_ln_bwd<NV>, grid, block, lds, s, dy, x, gamma, dx, part, rows, \
                     mp, eps, accumulate)
  if (nv <= 2) PMB_LAUNCH(2);
  else if (nv <= 3) PMB_LAUNCH(3);
  else if (nv <= 4) PMB_LAUNCH(4);
  else if (nv <= 6) PMB_LAUNCH(6);
  else if (nv <= 8) PMB_LAUNCH(8);
  else PMB_LAUNCH(12);
#undef PMB_LAUNCH
  return PN_LAUNCH_CHECK();
}

// ---- exact GELU (nn.GELU(), the Swin FFN's activation: mmcv FFN act_cfg=dict(type='GELU')) ---
// y = x Phi(x), dy/dx = Phi(x) + x phi(x); the same expression as the GEMM epilogue's GELU
// (gemm_common.h), so the taped hidden rows equal the fused forward's
__global__ __launch_bounds__(256) void k_gelu(const float* __restrict__ x, float* __restrict__ y,
                                              int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    y[i] = 0.5f * v * (1.f + erff(v * 0.70710678118654752f));
  }
}

__global__ __launch_bounds__(256) void k_gelu_bwd(const float* dy, const float* __restrict__ x,
                                                  float* dx, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
    const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
    dx[i] = dy[i] * (cdf + v * pdf);
  }
}

extern "C" int pn_gelu_f32(const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n <= 0 || n > ((int64_t)1 << 38)) return PN_BAD_ARG;
  hipLaunchKernelGGL(k_gelu, dim3(pn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
  if (!dy || !x || !dx || n <= 0 || n > ((int64_t)1 << 38)) return PN_BAD_ARG;
  hipLaunchKernelGGL(k_gelu_bwd, dim3(pn_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dy, x,
                     dx, n);
  return PN_LAUNCH_CHECK();
}

// ---- (shifted-)window attention backward, head dim 32 -----------------------------------------
// Workgroup = (window, head, image) as k_window_attn; thread t < N = ws^2 owns window token t,
// first as a query, then as a key.  Token t of window (wy, wx) sits at (y, x) = (wy ws + py,
// wx ws + px) of the padded, rolled map, i.e. at padded-grid position ((y + shift) mod Hp,
// (x + shift) mod Wp): that position's row of dqkv [B Hp Wp][3C] is written by exactly one
// (window, token), so every row of the padded grid (padding included) is written once per head.
// A position outside the H x W map is padding: its q / k / v are the qkv bias (the reference
// pads before the qkv Linear) and its dO is zero.  LDS:
//   A  [N][32]  K rows (phase 1), then Q rows (phase 2)
//   V  [N][32]  V rows (phase 1), then dO rows (phase 2)
//   dS [N][N|1] scores -> exp -> dS = P (dP - D), the gradient of the pre-softmax scores
//   the head's bias row, per-query max / 1/sum, per-token metadata
// Phase 1 (thread = query i): S_i. = scale q_i K^T + bias + mask, softmax statistics, D_i =
//   dO_i . O_i, dS_i. and dq_i = scale dS_i. K.
// Phase 2 (thread = key j): P_.j recomputed from the saved statistics, dv_j = P_.j^T dO,
//   dk_j = scale dS_.j^T Q.
// Phase 3 (thread = relative-position bin r): d table[head][r] = sum of dS over the pairs of
//   offset r, queries in row-major order -- one partial per (image, window, head), reduced by
//   the caller with pn_colsum_f32 (fixed order).
// Plain fp32 FMA: 6 x 32 FMA per (query, key) pair and head.
#define WB_MAXN 169  // ws <= 13

struct WinBP {
  const float* qkv; const float* qkv_bias; const float* table; const float* dout; const float* out;
  float* dqkv; float* dtable;
  int64_t ldqkv, lddo, ldo, lddqkv;
  int H, W, Hp, Wp, C, heads, ws, shift, nwx, nwin;
  float scale;
};

__device__ __forceinline__ float wb_dot32(const float (&a)[32], const float* __restrict__ b) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 v = ld4(b + 4 * u);
    s += a[4 * u] * v.x;
    s += a[4 * u + 1] * v.y;
    s += a[4 * u + 2] * v.z;
    s += a[4 * u + 3] * v.w;
  }
  return s;
}

__global__ __launch_bounds__(256) void k_window_attn_bwd(const WinBP p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int ws = p.ws, N = ws * ws, Ns = N | 1;
  const int nrel = (2 * ws - 1) * (2 * ws - 1);
  float* A = smem;                        // [N][32]
  float* Vs = A + N * 32;                 // [N][32]
  float* dS = Vs + N * 32;                // [N][Ns]
  float* tab = dS + N * Ns;               // [nrel]
  float* rmax = tab + nrel;               // [N]
  float* rinv = rmax + N;                 // [N]
  int* meta = reinterpret_cast<int*>(rinv + N);   // [N]

  const int tid = threadIdx.x, nthreads = blockDim.x;
  const int win = blockIdx.x, head = blockIdx.y, b = blockIdx.z;
  const int wy = win / p.nwx, wx = win - wy * p.nwx;
  const int C = p.C;

  // window token t -> source row of the H x W map (-1: padding), padded-grid row, metadata
  // (relative-position key term | region label << 16, as k_window_attn)
  auto token = [&](int t, int& src, int64_t& prow) -> int {
    const int py = t / ws, px = t - py * ws;
    const int y = wy * ws + py, x = wx * ws + px;
    int ys = y + p.shift, xs = x + p.shift;
    if (ys >= p.Hp) ys -= p.Hp;
    if (xs >= p.Wp) xs -= p.Wp;
    int label = 0;
    if (p.shift > 0) {
      const int rh = (y >= p.Hp - ws) + (y >= p.Hp - p.shift);
      const int rw = (x >= p.Wp - ws) + (x >= p.Wp - p.shift);
      label = rh * 3 + rw;
    }
    src = (ys < p.H && xs < p.W) ? (b * p.H + ys) * p.W + xs : -1;
    prow = ((int64_t)b * p.Hp + ys) * p.Wp + xs;
    return (py * (2 * ws - 1) + px) | (label << 16);
  };
  auto qkv_row = [&](int src) -> const float* {
    return (src >= 0 ? p.qkv + (int64_t)src * p.ldqkv : p.qkv_bias) + head * 32;
  };

  // ---- prologue: K / V rows, the bias row, metadata
  for (int e = tid; e < N * 8; e += nthreads) {
    const int t = e >> 3, c = (e & 7) * 4;
    int src;
    int64_t prow;
    token(t, src, prow);
    const float* r = qkv_row(src);
    st4(A + t * 32 + c, ld4(r + C + c));
    st4(Vs + t * 32 + c, ld4(r + 2 * C + c));
  }
  for (int r = tid; r < nrel; r += nthreads) tab[r] = p.table[(int64_t)head * nrel + r];
  const bool own = tid < N;
  int src = -1, mymeta = 0;
  int64_t prow = 0;
  if (own) {
    mymeta = token(tid, src, prow);
    meta[tid] = mymeta;
  }
  float q[32], g[32];                     // this thread's query row, its dO row
  {
    const float* qr = qkv_row(src);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), d = a;
      if (own) a = ld4(qr + 4 * u);
      if (own && src >= 0) d = ld4(p.dout + (int64_t)src * p.lddo + head * 32 + 4 * u);
      q[4 * u] = a.x; q[4 * u + 1] = a.y; q[4 * u + 2] = a.z; q[4 * u + 3] = a.w;
      g[4 * u] = d.x; g[4 * u + 1] = d.y; g[4 * u + 2] = d.z; g[4 * u + 3] = d.w;
    }
  }
  const bool shifted = p.shift > 0;
  const float scale = p.scale;
  const int off = (ws - 1) * (2 * ws - 1) + (ws - 1);
  __syncthreads();

  // ---- phase 1: query rows
  if (own) {
    const int qlabel = mymeta >> 16, qbase = (mymeta & 0xffff) + off;
    float* srow = dS + tid * Ns;
    float m = -INFINITY;
    for (int j = 0; j < N; ++j) {
      const int km = meta[j];
      float s = wb_dot32(q, A + j * 32) * scale + tab[qbase - (km & 0xffff)];
      if (shifted && (km >> 16) != qlabel) s += -100.f;
      srow[j] = s;
      m = fmaxf(m, s);
    }
    float l = 0.f;
    float o[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) o[c] = 0.f;
    for (int j = 0; j < N; ++j) {
      const float e = expf(srow[j] - m);
      srow[j] = e;
      l += e;
      if (!p.out) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float4 v = ld4(Vs + j * 32 + 4 * u);
          o[4 * u] += e * v.x; o[4 * u + 1] += e * v.y;
          o[4 * u + 2] += e * v.z; o[4 * u + 3] += e * v.w;
        }
      }
    }
    const float inv = 1.f / l;
    float D = 0.f;
    if (src >= 0) {
      if (p.out) {
        D = wb_dot32(g, p.out + (int64_t)src * p.ldo + head * 32);
      } else {
#pragma unroll
        for (int c = 0; c < 32; ++c) D += g[c] * (o[c] * inv);
      }
    }
    rmax[tid] = m;
    rinv[tid] = inv;
    float dq[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) dq[c] = 0.f;
    for (int j = 0; j < N; ++j) {
      const float P = srow[j] * inv;
      const float ds = P * (wb_dot32(g, Vs + j * 32) - D);
      srow[j] = ds;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 k = ld4(A + j * 32 + 4 * u);
        dq[4 * u] += ds * k.x; dq[4 * u + 1] += ds * k.y;
        dq[4 * u + 2] += ds * k.z; dq[4 * u + 3] += ds * k.w;
      }
    }
    float* dst = p.dqkv + prow * p.lddqkv + head * 32;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      st4(dst + 4 * u, make_float4(dq[4 * u] * scale, dq[4 * u + 1] * scale,
                                   dq[4 * u + 2] * scale, dq[4 * u + 3] * scale));
  }
  __syncthreads();
  // this thread's key row out of A before A is overwritten with the query rows
  float kr[32];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 k = own ? ld4(A + tid * 32 + 4 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
    kr[4 * u] = k.x; kr[4 * u + 1] = k.y; kr[4 * u + 2] = k.z; kr[4 * u + 3] = k.w;
  }
  __syncthreads();
  if (own) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      st4(A + tid * 32 + 4 * u, make_float4(q[4 * u], q[4 * u + 1], q[4 * u + 2], q[4 * u + 3]));
      st4(Vs + tid * 32 + 4 * u, make_float4(g[4 * u], g[4 * u + 1], g[4 * u + 2], g[4 * u + 3]));
    }
  }
  __syncthreads();

  // ---- phase 2: key rows (the scores recomputed exactly as phase 1 formed them)
  if (own) {
    const int klabel = mymeta >> 16, kpos = mymeta & 0xffff;
    float dk[32], dv[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) dk[c] = dv[c] = 0.f;
    for (int i = 0; i < N; ++i) {
      const int qm = meta[i];
      // (dot(q_i, k_j) with the query operand first, as in phase 1)
      float s = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 a = ld4(A + i * 32 + 4 * u);
        s += a.x * kr[4 * u];
        s += a.y * kr[4 * u + 1];
        s += a.z * kr[4 * u + 2];
        s += a.w * kr[4 * u + 3];
      }
      s = s * scale + tab[(qm & 0xffff) + off - kpos];
      if (shifted && (qm >> 16) != klabel) s += -100.f;
      const float P = expf(s - rmax[i]) * rinv[i];
      const float ds = dS[i * Ns + tid];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 a = ld4(A + i * 32 + 4 * u), d = ld4(Vs + i * 32 + 4 * u);
        dk[4 * u] += ds * a.x; dk[4 * u + 1] += ds * a.y;
        dk[4 * u + 2] += ds * a.z; dk[4 * u + 3] += ds * a.w;
        dv[4 * u] += P * d.x; dv[4 * u + 1] += P * d.y;
        dv[4 * u + 2] += P * d.z; dv[4 * u + 3] += P * d.w;
      }
    }
    float* dst = p.dqkv + prow * p.lddqkv + head * 32;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      st4(dst + C + 4 * u, make_float4(dk[4 * u] * scale, dk[4 * u + 1] * scale,
                                       dk[4 * u + 2] * scale, dk[4 * u + 3] * scale));
      st4(dst + 2 * C + 4 * u, make_float4(dv[4 * u], dv[4 * u + 1], dv[4 * u + 2], dv[4 * u + 3]));
    }
  }

  // ---- phase 3: the bias-table bins (dS is final since the first barrier after phase 1)
  const int w2 = 2 * ws - 1;
  float* part = p.dtable + (((int64_t)b * p.nwin + win) * p.heads + head) * nrel;
  for (int r = tid; r < nrel; r += nthreads) {
    const int dy = r / w2 - (ws - 1), dx = r - (r / w2) * w2 - (ws - 1);
    const int y0 = max(0, dy), y1 = min(ws, ws + dy), x0 = max(0, dx), x1 = min(ws, ws + dx);
    float s = 0.f;
    for (int qy = y0; qy < y1; ++qy)
      for (int qx = x0; qx < x1; ++qx)
        s += dS[(qy * ws + qx) * Ns + (qy - dy) * ws + (qx - dx)];
    part[r] = s;
  }
}

static int window_attention_bwd_lds_bytes(int ws) {
  if (ws < 2 || ws * ws > WB_MAXN) return -1;
  const int N = ws * ws;
  return (2 * N * 32 + N * (N | 1) + (2 * ws - 1) * (2 * ws - 1) + 3 * N) * 4;
}

extern "C" int pn_window_attention_bwd_f32(const float* qkv, int64_t ldqkv, const float* qkv_bias,
                                           const float* bias_table, const float* dout, int64_t lddo,
                                           const float* out, int64_t ldo, float* dqkv,
                                           int64_t lddqkv, float* dtable_part, int B, int H, int W,
                                           int C, int heads, int ws, int shift, float scale,
                                           void* stream) {
  if (!qkv || !qkv_bias || !bias_table || !dout || !dqkv || !dtable_part || B <= 0 || H <= 0 ||
      W <= 0 || heads <= 0 || C != heads * 32 || ws < 2 || ws * ws > WB_MAXN || shift < 0 ||
      shift >= ws || ldqkv < 3 * C || lddo < C || lddqkv < 3 * C || (out && ldo < C) ||
      ((ldqkv | lddo | lddqkv | (out ? ldo : 0)) & 3))
    return PN_BAD_ARG;
  if (((uintptr_t)qkv | (uintptr_t)qkv_bias | (uintptr_t)dout | (uintptr_t)out |
       (uintptr_t)dqkv) & 15)
    return PN_BAD_ARG;
  const int Hp = (H + ws - 1) / ws * ws, Wp = (W + ws - 1) / ws * ws;
  if ((int64_t)B * Hp * Wp >= (1ll << 31)) return PN_BAD_ARG;
  const int lds = window_attention_bwd_lds_bytes(ws);
  int dev = 0, max_lds = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
    return PN_BAD_ARG;
  if (lds > max_lds) return PN_BAD_ARG;
  WinBP p{};
  p.qkv = qkv; p.qkv_bias = qkv_bias; p.table = bias_table; p.dout = dout; p.out = out;
  p.dqkv = dqkv; p.dtable = dtable_part;
  p.ldqkv = ldqkv; p.lddo = lddo; p.ldo = ldo; p.lddqkv = lddqkv;
  p.H = H; p.W = W; p.Hp = Hp; p.Wp = Wp; p.C = C; p.heads = heads; p.ws = ws; p.shift = shift;
  p.nwx = Wp / ws; p.nwin = (Hp / ws) * p.nwx;
  p.scale = scale;
  const int threads = (ws * ws + 63) / 64 * 64;
  hipLaunchKernelGGL(k_window_attn_bwd, dim3(p.nwin, heads, B), dim3(threads), lds,
                     (hipStream_t)stream, p);
  return PN_LAUNCH_CHECK();
}
