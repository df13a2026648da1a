// Backward of PSGTrHead2's three class heads (psgtr_head2.py:309-324): sub_cls_embed, obj_cls_embed
// and rel_cls_embed are three Linear layers on the SAME normalised rows qn [N][256] (N = B * Q), with
// output widths C + 1, C + 1 and Cr + 1 (134, 134, 57 in psgtr_r50_psg_plus.py: none a multiple of 4).
// From the loss's logit gradients, read as the loss wrote them (contiguous, no padding):
//
//   dqn[n][:]  = (add ? dqn[n][:] : 0) + sum_j dsub[n][j] Wsub[j][:] + sum_j dobj[n][j] Wobj[j][:]
//                                      + sum_j drel[n][j] Wrel[j][:]
//   dW_h[j][:] = sum_n d_h[n][j] qn[n][:]        db_h[j] = sum_n d_h[n][j]        h in {sub, obj, rel}
//
// Two launches, both on v_mfma_f32_32x32x2_f32 (fp32 operands and accumulation, a k-ordered fmaf
// chain), no float atomics, a fixed summation order: the same inputs give the same bits.  Ragged
// edges are predicated in the kernels: an operand outside its matrix enters as an exact zero (its
// load goes to a clamped address inside the matrix), and no store leaves a matrix.
#include "common.h"

#define TG_CH 256        // channels of qn / the weights' rows
#define TG_MAX_N 4096
#define TG_MAX_C1 256
#define TG_MAX_CR1 64

#define TG_U 16           // MFMAs per batch of operand loads (32 contraction steps)

// Operands of one batch: lane half h supplies step k = k0 + 2 u + h.  Every load is unconditional
// from an address clamped into the matrix (k -> K - 1); what lies outside enters as an exact zero.
__device__ __forceinline__ void tg_load(const float* __restrict__ a_base, int64_t a_stride, bool a_ok,
                                        const float* __restrict__ b_base, int K, int k0, int half,
                                        float (&a)[TG_U], float (&b)[TG_U]) {
#pragma unroll
  for (int u = 0; u < TG_U; ++u) {
    const int k = k0 + 2 * u + half;
    const int kc = k < K ? k : K - 1;
    const float av = a_base[(int64_t)kc * a_stride];
    const float bv = b_base[(int64_t)kc * TG_CH];
    a[u] = (a_ok && k < K) ? av : 0.f;
    b[u] = k < K ? bv : 0.f;
  }
}

// acc += A B over k = 0 .. K - 1 ascending, A[i][k] = a_base[k * a_stride] of lane i (zero unless
// a_ok), B[k][j] = b_base[k * 256] of lane j; the next batch's loads are in flight while this batch's
// MFMAs run.  SUM: lanes 0 .. 31 also add their A operands, step k then step k + 1, into `s`.
template <bool SUM>
__device__ __forceinline__ f32x16 tg_chain(const float* __restrict__ a_base, int64_t a_stride,
                                           bool a_ok, const float* __restrict__ b_base, int K,
                                           int half, f32x16 acc, float& s) {
  float a[TG_U], b[TG_U], an[TG_U], bn[TG_U];
  tg_load(a_base, a_stride, a_ok, b_base, K, 0, half, a, b);
  for (int k0 = 0; k0 < K; k0 += 2 * TG_U) {
    const bool more = k0 + 2 * TG_U < K;         // (uniform)
    if (more) tg_load(a_base, a_stride, a_ok, b_base, K, k0 + 2 * TG_U, half, an, bn);
#pragma unroll
    for (int u = 0; u < TG_U; ++u) {
      if (k0 + 2 * u < K) {                      // (uniform)
        acc = mfma32(a[u], b[u], acc);
        if (SUM) {
          const float other = __shfl_xor(a[u], 32, 64);
          s = (s + a[u]) + other;
        }
      }
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < TG_U; ++u) a[u] = an[u], b[u] = bn[u];
    }
  }
  return acc;
}

// Row-tile kernel.  Workgroup = (32 rows, 128 channels); wave w owns channels 128 y + 32 w .. + 31.
// A[i][k] = d_h[n0 + i][k] (a lane walks along its own row), B[k][j] = W_h[k][c0 + j] (128
// contiguous bytes per lane half).  The contraction runs over sub, obj, rel in this order, each
// ascending.
__global__ __launch_bounds__(256) void k_tri_heads_dqn(
    const float* __restrict__ dsub, const float* __restrict__ dobj, const float* __restrict__ drel,
    const float* __restrict__ Wsub, const float* __restrict__ Wobj, const float* __restrict__ Wrel,
    float* __restrict__ dqn, int N, int C1, int Cr1, int add) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
  const int n0 = blockIdx.x * 32, c = (blockIdx.y * 4 + w) * 32 + j;
  const int n = n0 + j;
  const bool row_ok = n < N;
  const int nc = row_ok ? n : N - 1;             // (a row inside the matrix: its values are dropped)
  float* out = dqn + (int64_t)n0 * TG_CH + c;
  f32x16 acc = {0};
  if (add) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = mfma32_row(r, half);
      if (n0 + row < N) acc[r] = out[(int64_t)row * TG_CH];
    }
  }
  float unused = 0.f;
  acc = tg_chain<false>(dsub + (int64_t)nc * C1, 1, row_ok, Wsub + c, C1, half, acc, unused);
  acc = tg_chain<false>(dobj + (int64_t)nc * C1, 1, row_ok, Wobj + c, C1, half, acc, unused);
  acc = tg_chain<false>(drel + (int64_t)nc * Cr1, 1, row_ok, Wrel + c, Cr1, half, acc, unused);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, half);
    if (n0 + row < N) out[(int64_t)row * TG_CH] = acc[r];
  }
}

// Column-tile kernel.  Workgroup = (32 output rows j of ONE head, 128 channels); wave w owns channels
// 128 y + 32 w .. + 31.  A[i = j][k = n] = d[n][j0 + i]: the lanes of a half run along contiguous
// columns of one row n, the halves read rows k and k + 1; B[k = n][c] = qn[n][c].  n ascending.  The
// wave of channels 0 .. 31 also sums its A operands, row k then row k + 1, into db.
__global__ __launch_bounds__(256) void k_tri_heads_dw(
    const float* __restrict__ dsub, const float* __restrict__ dobj, const float* __restrict__ drel,
    const float* __restrict__ qn, float* __restrict__ dWsub, float* __restrict__ dbsub,
    float* __restrict__ dWobj, float* __restrict__ dbobj, float* __restrict__ dWrel,
    float* __restrict__ dbrel, int N, int C1, int Cr1, int tiles_c) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
  int t = blockIdx.x;
  const float* d;
  float *dW, *db;
  int width;
  if (t < tiles_c) {
    d = dsub, dW = dWsub, db = dbsub, width = C1;
  } else if (t < 2 * tiles_c) {
    d = dobj, dW = dWobj, db = dbobj, width = C1, t -= tiles_c;
  } else {
    d = drel, dW = dWrel, db = dbrel, width = Cr1, t -= 2 * tiles_c;
  }
  const int j0 = t * 32, col = j0 + j;
  const bool col_ok = col < width;
  const int cc = col_ok ? col : width - 1;       // (a column inside the matrix: its values are dropped)
  const int c = (blockIdx.y * 4 + w) * 32 + j;
  const bool bias = blockIdx.y == 0 && w == 0;   // (wave-uniform)
  f32x16 acc = {0};
  float s = 0.f;
  if (bias)
    acc = tg_chain<true>(d + cc, width, col_ok, qn + c, N, half, acc, s);
  else
    acc = tg_chain<false>(d + cc, width, col_ok, qn + c, N, half, acc, s);
  float* out = dW + (int64_t)j0 * TG_CH + c;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, half);
    if (j0 + row < width) out[(int64_t)row * TG_CH] = acc[r];
  }
  if (bias && half == 0 && col_ok) db[col] = s;
}

extern "C" int pn_triplet_heads_bwd_f32(const float* dsub, const float* dobj, const float* drel,
                                        const float* qn, const float* Wsub, const float* Wobj,
                                        const float* Wrel, float* dqn, float* dWsub, float* dbsub,
                                        float* dWobj, float* dbobj, float* dWrel, float* dbrel, int N,
                                        int channels, int C1, int Cr1, int add, void* stream) {
  if (channels != TG_CH || N <= 0 || N > TG_MAX_N || C1 <= 0 || C1 > TG_MAX_C1 || Cr1 <= 0 ||
      Cr1 > TG_MAX_CR1 || (add != 0 && add != 1) || !dsub || !dobj || !drel || !qn || !Wsub ||
      !Wobj || !Wrel || !dqn || !dWsub || !dbsub || !dWobj || !dbobj || !dWrel || !dbrel)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_tri_heads_dqn, dim3((N + 31) / 32, 2), dim3(256), 0, (hipStream_t)stream,
                     dsub, dobj, drel, Wsub, Wobj, Wrel, dqn, N, C1, Cr1, add);
  int e = PN_LAUNCH_CHECK();
  if (e) return e;
  const int tiles_c = (C1 + 31) / 32, tiles_r = (Cr1 + 31) / 32;
  hipLaunchKernelGGL(k_tri_heads_dw, dim3(2 * tiles_c + tiles_r, 2), dim3(256), 0,
                     (hipStream_t)stream, dsub, dobj, drel, qn, dWsub, dbsub, dWobj, dbobj, dWrel,
                     dbrel, N, C1, Cr1, tiles_c);
  return PN_LAUNCH_CHECK();
}
