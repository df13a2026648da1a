// Unmasked multi-head attention backward with the keys split into fixed chunks across workgroups
// (8 heads x 32 channels): the relation decoder's cross-attentions of the sibling head
// (baseline.py:372-386: 100 relation queries against a memory level's 1 050 - 16 700 keys, no
// attention mask).  Same mathematics as pn_mha_bwd_f32 (csrc/grad.hip) with bits = NULL, but the
// probabilities P and dS = P (dP - delta) never leave the chip: a workgroup owns KS_CHUNK keys of
// one (image, head), one key per thread with its k / v rows and its dk / dv accumulators in
// registers, and walks the queries in tiles of KS_QTILE.  HBM scratch holds only
//   stat [B][8][Nq][6]            the softmax's row maximum M and the row term delta (doubles),
//                                 1 / L; one float unused,
//   part [B][8][Nq][chunks][32]   per-chunk partials of dq (their first six floats hold the
//                                 chunk's (m, l, t), three doubles, between the first two passes).
// Four launches: per-chunk statistics; their combination in ascending chunk order (the forward tape
// keeps no log-sum-exp); the main pass (dk, dv final, dq partials); the sum of the dq partials in
// ascending chunk order.
//
// pn_mha_bwd_keysplit_masked_f32 is the same backward UNDER the forward's packed boolean mask (bits /
// rowall exactly as pn_mask_pack writes them: bits [B * Nq][(Nk + 31) / 32], a set bit = the key is
// not attendable, shared by the 8 heads; a row with rowall == 1 ignores its bits, as pn_mha_bwd_f32
// and the forward do): the nine masked decoder layers' cross-attentions.  The kernels are the same
// templates with MASKED = true: a tile's mask words (KS_QTILE queries x KS_CHUNK / 32 words; the
// chunk starts at a multiple of 32 keys, so the words line up) are staged in LDS beside the
// query-side rows and every thread tests its own key's bit.  A masked (query, key) pair has P = 0
// and dS = 0 exactly and adds nothing to dq, dk or dv; a key masked in every row gets zero dk / dv
// rows, which are still written.  New with a mask: a chunk whose keys are ALL masked for a row has
// the chunk maximum m = -inf (l = t = 0).  No exponential is taken of (-inf) - (-inf): the
// statistics pass measures the distances from 0 in that case (every e is exp(-inf) = 0), and the
// combination gives such a chunk the weight w_c = 0 without evaluating exp.  With bits == NULL the
// masked entry launches the MASKED = false kernels: the bits of pn_mha_bwd_keysplit_f32.
//
// Where float64 is used, and why (measured under a peaked softmax, q scaled by 8; labnotes R23):
//  * The logits' dot products, and the softmax on their distance from the row maximum,
//    exp(|scale| (d - max d)).  An fp32 dot of 32 products of size 5 is off by ~1e-5, and that
//    error goes into every probability as a RELATIVE error.
//  * dP = dO . v, the row term delta = sum_j P_ij dP_ij (double exponentials and double sums in the
//    statistics pass) and the difference dP - delta, which is rounded to fp32 once.  dS = P (dP -
//    delta) is a product with a DIFFERENCE: a key's dk row is led by the one query that attends to
//    it most, and where that query's dP happens to lie within 0.1 of its delta (one key in a
//    hundred), an fp32 dP of size 5 -- good to 5e-7 at best -- leaves the whole row with a relative
//    error of 1e-5.  That is what kept dk at 241 x 2^-24 with float64 logits alone, and
//    pn_mha_bwd_f32 at 654 (dv 95).  The row term is therefore not taken as dO . O from a saved
//    output either.
// dk / dv / dq are accumulated in fp32.  No atomics: every sum has a fixed order that depends on the
// shapes only (within a thread in index order, across lanes by a butterfly, over chunks in
// ascending order), so two launches give equal bits.
#include "common.h"

#define KS_CHUNK 256   // keys per workgroup = threads per workgroup (one key each)
#define KS_QTILE 8     // queries per tile: KS_QTILE * 32 = KS_CHUNK threads in the dq phase
#define KS_KLD 36      // LDS row stride of the key chunk (floats; 16-byte aligned rows)
#define KS_STAT 6      // floats per row of `stat`
#define KS_MW (KS_CHUNK / 32)   // mask words per (query, chunk)

// The tile's mask words -> sMask (threads 0 .. KS_QTILE * KS_MW - 1, one word each): 0 (nothing
// masked) past the last query, past the row's last word and for a row whose rowall is set.
__device__ __forceinline__ void ks_stage_mask(uint32_t (*sMask)[KS_MW],
                                              const uint32_t* __restrict__ bits,
                                              const int32_t* __restrict__ rowall, int b, int c,
                                              int t0, int Nq, int Nk, int tid) {
  if (tid < KS_QTILE * KS_MW) {
    const int mq = tid / KS_MW, mw = tid % KS_MW;
    const int i = t0 + mq, nw = (Nk + 31) >> 5, wi = c * KS_MW + mw;
    uint32_t word = 0u;
    if (i < Nq && wi < nw) {
      const int64_t row = (int64_t)b * Nq + i;
      if (!rowall[row]) word = bits[row * nw + wi];
    }
    sMask[mq][mw] = word;
  }
}

// A query-side row (q times the sign of `scale`, or dO; float64 in LDS: the same address in every
// lane, a broadcast) against this thread's key-side row (k or v, float64 in registers) over one
// head's 32 channels.  Both passes call this, so the dots they see are the same bits.
__device__ __forceinline__ double ks_dot_d(const double* __restrict__ qs, const double (&kd)[32]) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int d = 0; d < 32; d += 4) {
    a0 = fma(qs[d], kd[d], a0);
    a1 = fma(qs[d + 1], kd[d + 1], a1);
    a2 = fma(qs[d + 2], kd[d + 2], a2);
    a3 = fma(qs[d + 3], kd[d + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// exp(ascale * diff) in fp32, diff <= 0 a float64 distance from a maximum: the argument as a float
// plus its remainder, exp(xh + xl) = exp(xh) (1 + xl).
__device__ __forceinline__ float ks_exp(double ascale, double diff) {
  const double x = ascale * diff;
  const float xh = (float)x;
  if (!(xh > -INFINITY)) return 0.f;
  const float xl = (float)(x - (double)xh);
  const float e = expf(xh);
  return fmaf(e, xl, e);
}

__device__ __forceinline__ double ks_wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ void ks_load_row_d(const float* __restrict__ p, double (&r)[32]) {
#pragma unroll
  for (int d = 0; d < 8; ++d) {
    const float4 x = ld4(p + 4 * d);
    r[4 * d] = x.x;
    r[4 * d + 1] = x.y;
    r[4 * d + 2] = x.z;
    r[4 * d + 3] = x.w;
  }
}

// ---- pass 1: m = max_j d_ij, l = sum_j e_ij, t = sum_j e_ij dP_ij with e_ij = exp(|scale| (d_ij -
// m)) of every (query, chunk), all in float64 ----
template <bool MASKED>
__global__ __launch_bounds__(KS_CHUNK) void k_ks_stats(const float* __restrict__ q, int64_t ldq,
                                                        const float* __restrict__ k, int64_t ldk,
                                                        const float* __restrict__ v, int64_t ldv,
                                                        const float* __restrict__ dout, int64_t ldo,
                                                        float* __restrict__ part, int Nq, int Nk,
                                                        int nch, float scale,
                                                        const uint32_t* __restrict__ bits,
                                                        const int32_t* __restrict__ rowall) {
  __shared__ uint32_t sMask[MASKED ? KS_QTILE : 1][KS_MW];
  __shared__ __attribute__((aligned(16))) double sQd[KS_QTILE][32];
  __shared__ __attribute__((aligned(16))) double sDOd[KS_QTILE][32];
  __shared__ double sS[KS_QTILE][KS_CHUNK];
  __shared__ double sDP[KS_QTILE][KS_CHUNK];
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int j = c * KS_CHUNK + tid;
  const bool valid = j < Nk;
  double kd[32], vd[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) kd[d] = vd[d] = 0.0;
  if (valid) {
    ks_load_row_d(k + ((int64_t)b * Nk + j) * ldk + h * 32, kd);
    ks_load_row_d(v + ((int64_t)b * Nk + j) * ldv + h * 32, vd);
  }
  const int ti = tid >> 5, td = tid & 31, wave = tid >> 6, lane = tid & 63;
  const double sgn = scale < 0.f ? -1.0 : 1.0, ascale = fabs((double)scale);
  for (int t0 = 0; t0 < Nq; t0 += KS_QTILE) {
    {
      const int i = t0 + ti;
      const int64_t row = (int64_t)b * Nq + i;
      sQd[ti][td] = i < Nq ? sgn * (double)q[row * ldq + h * 32 + td] : 0.0;
      sDOd[ti][td] = i < Nq ? (double)dout[row * ldo + h * 32 + td] : 0.0;
    }
    if constexpr (MASKED) ks_stage_mask(sMask, bits, rowall, b, c, t0, Nq, Nk, tid);
    __syncthreads();
#pragma unroll 1
    for (int qq = 0; qq < KS_QTILE; ++qq) {
      bool live = valid;
      if constexpr (MASKED) live = valid && !((sMask[qq][tid >> 5] >> (tid & 31)) & 1u);
      sS[qq][tid] = live ? ks_dot_d(sQd[qq], kd) : -(double)INFINITY;
      sDP[qq][tid] = ks_dot_d(sDOd[qq], vd);
    }
    __syncthreads();
    // a wave reduces two of the tile's queries over the chunk's 256 keys
#pragma unroll
    for (int r = 0; r < KS_QTILE / 4; ++r) {
      const int qq = wave * (KS_QTILE / 4) + r, i = t0 + qq;
      const double s0 = sS[qq][lane], s1 = sS[qq][lane + 64], s2 = sS[qq][lane + 128],
                   s3 = sS[qq][lane + 192];
      // (unmasked, key c * 256 is valid and m is finite; under a mask every key of the chunk may
      // be masked for this row: m = -inf, and the distances are then taken from 0, so that every
      // e is exp(-inf) = 0 and l = t = 0)
      const double m = ks_wave_max_d(fmax(fmax(s0, s1), fmax(s2, s3)));
      double mm = m;
      if constexpr (MASKED) mm = m > -(double)INFINITY ? m : 0.0;
      const double e0 = exp(ascale * (s0 - mm)), e1 = exp(ascale * (s1 - mm)),
                   e2 = exp(ascale * (s2 - mm)), e3 = exp(ascale * (s3 - mm));
      const double l = wave_sum_d((e0 + e1) + (e2 + e3));
      const double t = wave_sum_d((e0 * sDP[qq][lane] + e1 * sDP[qq][lane + 64]) +
                                  (e2 * sDP[qq][lane + 128] + e3 * sDP[qq][lane + 192]));
      if (lane == 0 && i < Nq) {
        double* p = reinterpret_cast<double*>(
            part + ((((int64_t)b * 8 + h) * Nq + i) * nch + c) * 32);
        p[0] = m;
        p[1] = l;
        p[2] = t;
      }
    }
    // (the next tile's sQd / sDOd are written while other waves may still reduce sS / sDP:
    // different arrays; sS / sDP are written again only behind the next barrier)
  }
}

// ---- pass 2: M = max_c m_c, L = sum_c l_c w_c, delta = sum_c t_c w_c / L with w_c = exp(|scale|
// (m_c - M)), chunks ascending -> stat = (M, delta, 1 / L) ----
template <bool MASKED>
__global__ __launch_bounds__(256) void k_ks_combine(const float* __restrict__ part,
                                                     float* __restrict__ stat, int64_t rows,
                                                     int nch, float scale) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double* p = reinterpret_cast<const double*>(part + r * nch * 32);   // 16 doubles per chunk
  const double ascale = fabs((double)scale);
  double M = p[0];
  for (int c = 1; c < nch; ++c) M = fmax(M, p[(int64_t)c * 16]);
  double L = 0.0, T = 0.0;
  for (int c = 0; c < nch; ++c) {
    const double mc = p[(int64_t)c * 16];
    double w;
    if constexpr (MASKED) {
      // a chunk with every key masked for this row (m_c = -inf, l_c = t_c = 0) weighs nothing
      w = mc > -(double)INFINITY ? exp(ascale * (mc - M)) : 0.0;
    } else {
      w = exp(ascale * (mc - M));
    }
    L += p[(int64_t)c * 16 + 1] * w;
    T += p[(int64_t)c * 16 + 2] * w;
  }
  float* st = stat + KS_STAT * r;
  if constexpr (MASKED) {
    // (bits that mask a whole row whose rowall is not set -- pn_mask_pack writes none -- leave
    // L = 0: such a row gets zero probabilities, not NaNs)
    const bool some = L > 0.0;
    reinterpret_cast<double*>(st)[0] = some ? M : 0.0;
    reinterpret_cast<double*>(st)[1] = some ? T / L : 0.0;
    st[4] = some ? (float)(1.0 / L) : 0.f;
  } else {
    reinterpret_cast<double*>(st)[0] = M;
    reinterpret_cast<double*>(st)[1] = T / L;
    st[4] = (float)(1.0 / L);
  }
  st[5] = 0.f;
}

// ---- pass 3: dk, dv of the chunk's keys (final) and the chunk's share of dq ----
template <bool MASKED>
__global__ __launch_bounds__(KS_CHUNK) void k_ks_main(
    const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
    const float* __restrict__ v, int64_t ldv, const float* __restrict__ dout, int64_t ldo,
    float* __restrict__ dk, int64_t lddk, float* __restrict__ dv, int64_t lddv,
    const float* __restrict__ stat, float* __restrict__ part, int Nq, int Nk, int nch,
    float scale, const uint32_t* __restrict__ bits, const int32_t* __restrict__ rowall) {
  __shared__ uint32_t sMask[MASKED ? KS_QTILE : 1][KS_MW];
  __shared__ __attribute__((aligned(16))) float sK[KS_CHUNK][KS_KLD];
  __shared__ __attribute__((aligned(16))) float sDS[KS_QTILE][KS_CHUNK];
  __shared__ __attribute__((aligned(16))) double sQd[KS_QTILE][32];
  __shared__ __attribute__((aligned(16))) double sDOd[KS_QTILE][32];
  __shared__ __attribute__((aligned(16))) float sQ[KS_QTILE][32];
  __shared__ __attribute__((aligned(16))) float sDO[KS_QTILE][32];
  __shared__ double sM[KS_QTILE], sDelta[KS_QTILE];
  __shared__ float sInv[KS_QTILE];
  const int c = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int j = c * KS_CHUNK + tid;
  const bool valid = j < Nk;
  double kd[32], vd[32];
  float4 ak[8], av[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) ak[d] = av[d] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int d = 0; d < 32; ++d) kd[d] = vd[d] = 0.0;
  if (valid) {
    ks_load_row_d(k + ((int64_t)b * Nk + j) * ldk + h * 32, kd);
    ks_load_row_d(v + ((int64_t)b * Nk + j) * ldv + h * 32, vd);
  }
#pragma unroll
  for (int d = 0; d < 8; ++d)
    *reinterpret_cast<float4*>(&sK[tid][4 * d]) = make_float4(
        (float)kd[4 * d], (float)kd[4 * d + 1], (float)kd[4 * d + 2], (float)kd[4 * d + 3]);
  const int ti = tid >> 5, td = tid & 31;
  const int64_t bh = (int64_t)b * 8 + h;
  const double sgn = scale < 0.f ? -1.0 : 1.0, ascale = fabs((double)scale);
  for (int t0 = 0; t0 < Nq; t0 += KS_QTILE) {
    {
      const int i = t0 + ti;
      const int64_t row = (int64_t)b * Nq + i;
      const float qv = i < Nq ? q[row * ldq + h * 32 + td] : 0.f;
      const float dov = i < Nq ? dout[row * ldo + h * 32 + td] : 0.f;
      sQ[ti][td] = qv;
      sQd[ti][td] = sgn * (double)qv;
      sDO[ti][td] = dov;
      sDOd[ti][td] = (double)dov;
      const float* st = stat + KS_STAT * (bh * Nq + i);
      if (td == 0) sM[ti] = i < Nq ? reinterpret_cast<const double*>(st)[0] : 0.0;
      if (td == 1) sDelta[ti] = i < Nq ? reinterpret_cast<const double*>(st)[1] : 0.0;
      if (td == 2) sInv[ti] = i < Nq ? st[4] : 0.f;   // (0 past the last query: the row adds nothing)
    }
    if constexpr (MASKED) ks_stage_mask(sMask, bits, rowall, b, c, t0, Nq, Nk, tid);
    __syncthreads();
    // phase 1: this thread's key against the tile's queries
#pragma unroll 1
    for (int qq = 0; qq < KS_QTILE; ++qq) {
      const double sd = ks_dot_d(sQd[qq], kd);
      bool live = valid;
      if constexpr (MASKED) live = valid && !((sMask[qq][tid >> 5] >> (tid & 31)) & 1u);
      const float p = live ? ks_exp(ascale, sd - sM[qq]) * sInv[qq] : 0.f;
      const float ds = p * (float)(ks_dot_d(sDOd[qq], vd) - sDelta[qq]);
      sDS[qq][tid] = ds;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        const float4 qv = *reinterpret_cast<const float4*>(&sQ[qq][4 * d]);
        const float4 dov = *reinterpret_cast<const float4*>(&sDO[qq][4 * d]);
        ak[d].x = fmaf(ds, qv.x, ak[d].x);
        ak[d].y = fmaf(ds, qv.y, ak[d].y);
        ak[d].z = fmaf(ds, qv.z, ak[d].z);
        ak[d].w = fmaf(ds, qv.w, ak[d].w);
        av[d].x = fmaf(p, dov.x, av[d].x);
        av[d].y = fmaf(p, dov.y, av[d].y);
        av[d].z = fmaf(p, dov.z, av[d].z);
        av[d].w = fmaf(p, dov.w, av[d].w);
      }
    }
    __syncthreads();
    // phase 2: thread (query ti, channel td) sums dS k over the chunk's keys in key order
    {
      float acc = 0.f;
#pragma unroll 4
      for (int jj = 0; jj < KS_CHUNK; jj += 4) {
        const float4 d4 = *reinterpret_cast<const float4*>(&sDS[ti][jj]);
        acc = fmaf(d4.x, sK[jj][td], acc);
        acc = fmaf(d4.y, sK[jj + 1][td], acc);
        acc = fmaf(d4.z, sK[jj + 2][td], acc);
        acc = fmaf(d4.w, sK[jj + 3][td], acc);
      }
      const int i = t0 + ti;
      if (i < Nq) part[((bh * Nq + i) * nch + c) * 32 + td] = acc;
    }
    // (the next tile writes the query-side arrays, mask words and statistics, which nobody reads
    // in phase 2, and writes sDS only behind its first barrier)
  }
  if (valid) {
    float* dkp = dk + ((int64_t)b * Nk + j) * lddk + h * 32;
    float* dvp = dv + ((int64_t)b * Nk + j) * lddv + h * 32;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      st4(dkp + 4 * d, make_float4(scale * ak[d].x, scale * ak[d].y, scale * ak[d].z,
                                   scale * ak[d].w));
      st4(dvp + 4 * d, av[d]);
    }
  }
}

// ---- pass 4: dq = scale * sum_c part, chunks ascending ----
__global__ __launch_bounds__(256) void k_ks_dq(const float* __restrict__ part,
                                                float* __restrict__ dq, int64_t lddq, int B, int Nq,
                                                int nch, float scale) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;   // ((b * Nq + i) * 8 + h) * 32 + d
  if (t >= (int64_t)B * Nq * 256) return;
  const int d = (int)(t & 31), h = (int)((t >> 5) & 7);
  const int64_t row = t >> 8;                                  // b * Nq + i
  const int64_t b = row / Nq, i = row - b * Nq;
  const float* p = part + (((b * 8 + h) * Nq + i) * nch) * 32 + d;
  float acc = 0.f;
  for (int c = 0; c < nch; ++c) acc += p[(int64_t)c * 32];
  dq[row * lddq + h * 32 + d] = scale * acc;
}

extern "C" int pn_mha_keysplit_chunk(void) { return KS_CHUNK; }

extern "C" int64_t pn_mha_bwd_keysplit_scratch_floats(int B, int Nq, int Nk) {
  if (B <= 0 || Nq <= 0 || Nk <= 0) return 0;
  const int64_t nch = (Nk + KS_CHUNK - 1) / KS_CHUNK;
  return (int64_t)B * 8 * Nq * (KS_STAT + 32 * nch);
}

template <bool MASKED>
static void ks_launch(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                      int64_t ldv, const float* dout, int64_t ldo, float* dq, int64_t lddq,
                      float* dk, int64_t lddk, float* dv, int64_t lddv, float* scratch, int B,
                      int Nq, int Nk, float scale, const uint32_t* bits, const int32_t* rowall,
                      hipStream_t s) {
  const int nch = pn_cdiv(Nk, KS_CHUNK);
  const int64_t rows = (int64_t)B * 8 * Nq;
  float* stat = scratch;
  float* part = scratch + KS_STAT * rows;
  hipLaunchKernelGGL(k_ks_stats<MASKED>, dim3(nch, 8, B), dim3(KS_CHUNK), 0, s, q, ldq, k, ldk, v,
                     ldv, dout, ldo, part, Nq, Nk, nch, scale, bits, rowall);
  hipLaunchKernelGGL(k_ks_combine<MASKED>, dim3(pn_cdiv(rows, 256)), dim3(256), 0, s, part, stat,
                     rows, nch, scale);
  hipLaunchKernelGGL(k_ks_main<MASKED>, dim3(nch, 8, B), dim3(KS_CHUNK), 0, s, q, ldq, k, ldk, v,
                     ldv, dout, ldo, dk, lddk, dv, lddv, stat, part, Nq, Nk, nch, scale, bits,
                     rowall);
  hipLaunchKernelGGL(k_ks_dq, dim3(pn_cdiv(rows * 32, 256)), dim3(256), 0, s, part, dq, lddq, B,
                     Nq, nch, scale);
}

// bits / rowall: pn_mask_pack's outputs, or both NULL (no mask: the kernels and bits of
// pn_mha_bwd_keysplit_f32); one without the other is refused before any launch.
extern "C" int pn_mha_bwd_keysplit_masked_f32(
    const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
    const float* dout, int64_t ldo, float* dq, int64_t lddq, float* dk, int64_t lddk, float* dv,
    int64_t lddv, float* scratch, int64_t scratch_floats, int B, int Nq, int Nk, float scale,
    const uint32_t* bits, const int32_t* rowall, void* stream) {
  if (!q || !k || !v || !dout || !dq || !dk || !dv || !scratch || B <= 0 || Nq <= 0 ||
      Nk <= 0 || B > 65535 || (bits == nullptr) != (rowall == nullptr))
    return PN_BAD_ARG;
  if ((ldq | ldk | ldv | ldo | lddq | lddk | lddv) % 4 || ldq < 256 || ldk < 256 ||
      ldv < 256 || ldo < 256 || lddq < 256 || lddk < 256 || lddv < 256)
    return PN_BAD_ARG;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout |
       (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)scratch) & 15)
    return PN_BAD_ARG;
  if (((uintptr_t)bits | (uintptr_t)rowall) & 3) return PN_BAD_ARG;
  if (scratch_floats < pn_mha_bwd_keysplit_scratch_floats(B, Nq, Nk)) return PN_BAD_ARG;
  if (bits)
    ks_launch<true>(q, ldq, k, ldk, v, ldv, dout, ldo, dq, lddq, dk, lddk, dv, lddv, scratch, B,
                    Nq, Nk, scale, bits, rowall, (hipStream_t)stream);
  else
    ks_launch<false>(q, ldq, k, ldk, v, ldv, dout, ldo, dq, lddq, dk, lddk, dv, lddv, scratch, B,
                     Nq, Nk, scale, nullptr, nullptr, (hipStream_t)stream);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_mha_bwd_keysplit_f32(const float* q, int64_t ldq, const float* k, int64_t ldk,
                                       const float* v, int64_t ldv, const float* dout,
                                       int64_t ldo, float* dq, int64_t lddq, float* dk,
                                       int64_t lddk, float* dv, int64_t lddv, float* scratch,
                                       int64_t scratch_floats, int B, int Nq, int Nk, float scale,
                                       void* stream) {
  if (!q || !k || !v || !dout || !dq || !dk || !dv || !scratch || B <= 0 || Nq <= 0 ||
      Nk <= 0 || B > 65535)
    return PN_BAD_ARG;
  if ((ldq | ldk | ldv | ldo | lddq | lddk | lddv) % 4 || ldq < 256 || ldk < 256 ||
      ldv < 256 || ldo < 256 || lddq < 256 || lddk < 256 || lddv < 256)
    return PN_BAD_ARG;
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout |
       (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)scratch) & 15)
    return PN_BAD_ARG;
  if (scratch_floats < pn_mha_bwd_keysplit_scratch_floats(B, Nq, Nk)) return PN_BAD_ARG;
  ks_launch<false>(q, ldq, k, ldk, v, ldv, dout, ldo, dq, lddq, dk, lddk, dv, lddv, scratch, B, Nq,
                   Nk, scale, nullptr, nullptr, (hipStream_t)stream);
  return PN_LAUNCH_CHECK();
}
