// The two products behind the mask logits' backward.  The mask logits of every decoder layer are
//   mask[l][b][q][p] = sum_c me[l][b][q][c] * MF[b][p][c]
// (`einsum("bqc,bchw->bqhw")`, pairnet_head.py:236-243 / baseline.py:254-296), and the segmentation
// loss hands their gradient back COMPACT: G [M][P] holds the rows of the matched queries only
// (P = h * w), mask_rows [M] their row index into the L * B * Q rows of `me`, -1 where the assignment
// failed (seg_losses.py).  Row m = l * Ml + m_off[b] + j (layer-major, then image, then the image's
// n_b = min(Q, G_b) rows), so which rows belong to which image is known on the host from shapes alone.
//
//   pn_mask_embed_grad_f32     dme[m][c]    = sum_p G[m][p] * MF[b(m)][p][c]             [M][256]
//   pn_mask_feature_grad_f32   dMF[b][p][c] = sum_{m of image b} G[m][p] * me[mask_rows[m]][c]
//
// Both run on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulation: a k-ordered fmaf chain), in
// a fixed summation order without floating-point atomics -- two launches on the same inputs give the
// same bits -- and write their WHOLE output.  A row with mask_rows[m] < 0 contributes an exact zero
// and its G row is never read (it may hold NaN).
//
// The table (int32, built by the host from L, B and n_b): [img_off (B + 1) | order (M) | tiles (2 T)]
//   order     the rows m grouped by image: image b owns order[img_off[b] .. img_off[b + 1]), its L
//             runs in layer order;
//   tiles     kernel 1's row tiles: (image, offset into `order` of the tile's first row); a tile is
//             up to 32 consecutive entries of ONE image's part of `order`.
// Every table entry is range-checked on the device before it becomes an address.
#include "common.h"

#define MG_KSLICE 2048   // pixels per split-K slice of pn_mask_embed_grad_f32 (a function of P alone)
#define MG_KC 64         // pixels per staged chunk of G
#define MG_LDA 66        // LDS row stride of the chunk: 2 mod 64, so the two lane halves of an A read
                         // (rows 0..31 at column k and at column k + 1) fall on even / odd banks
#define MG_KB 1024       // k entries of pn_mask_feature_grad_f32 staged per block

// ---------------------------------------------------------------------------------------------------
// Kernel 1.  Workgroup = (row tile t, slice s): 32 rows x 256 channels over the slice's pixels, wave w
// owns channels 64 w .. 64 w + 63 (two 32x32 accumulators).  A[i][k] = G[m_i][k] is K-contiguous in
// memory and goes through LDS (coalesced row reads, conflict-free operand reads); B[k][j] = MF[b][k][j]
// is N-contiguous and is read straight into the operand register (lane halves read two consecutive
// pixel rows, 128 contiguous bytes each).  Partial sums go to scratch [S][T * 32][256].
template <bool GUARD>
__device__ __forceinline__ void mg_chunk(const float* __restrict__ sA, const float* __restrict__ mf,
                                         int64_t k0, int64_t k_end, int half, int j, f32x16& acc0,
                                         f32x16& acc1) {
#pragma unroll 8
  for (int kk = 0; kk < MG_KC; kk += 2) {
    const float a = sA[j * MG_LDA + kk + half];
    const int64_t p = k0 + kk + half;
    float b0 = 0.f, b1 = 0.f;
    if (!GUARD || p < k_end) {
      b0 = mf[p * 256];
      b1 = mf[p * 256 + 32];
    }
    acc0 = mfma32(a, b0, acc0);
    acc1 = mfma32(a, b1, acc1);
  }
}

__global__ __launch_bounds__(256) void k_mask_embed_grad(
    const float* __restrict__ G, const float* __restrict__ MF, const int64_t* __restrict__ mask_rows,
    const int32_t* __restrict__ img_off, const int32_t* __restrict__ order,
    const int32_t* __restrict__ tiles, int M, int B, int T, int64_t P, int S,
    float* __restrict__ scratch) {
  __shared__ float sA[32 * MG_LDA];
  __shared__ int sm[32];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
  const int t = blockIdx.x / S, s = blockIdx.x % S;
  int b = tiles[2 * t], start = tiles[2 * t + 1];
  const bool okb = b >= 0 && b < B && start >= 0;
  if (!okb) b = 0;
  int end = okb ? img_off[b + 1] : 0;
  if (end > M) end = M;
  if (tid < 32) {
    int m = -1;
    if (okb && start + tid < end) {
      m = order[start + tid];
      if (m < 0 || m >= M || mask_rows[m] < 0) m = -1;
    }
    sm[tid] = m;
  }
  const int64_t k_begin = (int64_t)s * MG_KSLICE;
  const int64_t k_end = k_begin + MG_KSLICE < P ? k_begin + MG_KSLICE : P;
  const float* mf = MF + (int64_t)b * P * 256 + w * 64 + j;
  f32x16 acc0 = {0}, acc1 = {0};
  for (int64_t k0 = k_begin; k0 < k_end; k0 += MG_KC) {
    __syncthreads();      // the previous chunk's operand reads are done (first pass: sm is written)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = tid + 256 * e, row = idx >> 6, kk = idx & 63;
      const int m = sm[row];
      const int64_t k = k0 + kk;
      sA[row * MG_LDA + kk] = (m >= 0 && k < k_end) ? G[(int64_t)m * P + k] : 0.f;
    }
    __syncthreads();
    if (k0 + MG_KC <= k_end)
      mg_chunk<false>(sA, mf, k0, k_end, half, j, acc0, acc1);
    else
      mg_chunk<true>(sA, mf, k0, k_end, half, j, acc0, acc1);
  }
  float* out = scratch + (((int64_t)s * T + t) * 32) * 256 + w * 64 + j;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, half);
    out[row * 256] = acc0[r];
    out[row * 256 + 32] = acc1[r];
  }
}

// dme[m] = slice 0 + slice 1 + ... in ascending order; a failed row is an exact zero row
__global__ __launch_bounds__(256) void k_mask_embed_grad_reduce(
    const float* __restrict__ scratch, const int64_t* __restrict__ mask_rows,
    const int32_t* __restrict__ img_off, const int32_t* __restrict__ order,
    const int32_t* __restrict__ tiles, int M, int B, int T, int S, float* __restrict__ dme) {
  const int t = blockIdx.x >> 5, i = blockIdx.x & 31, c = threadIdx.x;
  const int b = tiles[2 * t], start = tiles[2 * t + 1];
  if (b < 0 || b >= B || start < 0) return;
  int end = img_off[b + 1];
  if (end > M) end = M;
  if (start + i >= end) return;
  const int m = order[start + i];
  if (m < 0 || m >= M) return;
  float v = 0.f;
  if (mask_rows[m] >= 0) {
    const float* p = scratch + ((int64_t)t * 32 + i) * 256 + c;
    v = p[0];
    for (int s = 1; s < S; ++s) v += p[(int64_t)s * T * 32 * 256];
  }
  dme[(int64_t)m * 256 + c] = v;
}

// ---------------------------------------------------------------------------------------------------
// Kernel 2.  Workgroup = (64 pixels, image b) x 256 channels, wave w owns channels 64 w .. 64 w + 63
// for both 32-pixel halves (four 32x32 accumulators).  A[i = pixel][k = m] is G read down its columns:
// the lanes of a half run along contiguous pixels of ONE row m (128 contiguous bytes), the two halves
// read rows k and k + 1.  B[k = m][j = c] is the `me` row gathered through mask_rows.  The contraction
// runs over the image's rows in `order` (ascending layer, then row); the row numbers are staged once
// per MG_KB entries so that the loop's loads depend on LDS only.
__global__ __launch_bounds__(256) void k_mask_feature_grad(
    const float* __restrict__ G, const float* __restrict__ me, const int64_t* __restrict__ mask_rows,
    const int32_t* __restrict__ img_off, const int32_t* __restrict__ order, int M, int64_t P,
    int64_t me_rows, float* __restrict__ dMF) {
  __shared__ int s_m[MG_KB];
  __shared__ int s_r[MG_KB];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, half = lane >> 5, j = lane & 31;
  const int b = blockIdx.y;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  int start = img_off[b], end = img_off[b + 1];
  if (start < 0) start = 0;
  if (end > M) end = M;
  const int K = end > start ? end - start : 0;
  const int64_t pa0 = p0 + j, pa1 = p0 + 32 + j;
  const bool in0 = pa0 < P, in1 = pa1 < P;
  const float* mec = me + w * 64 + j;
  f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};
  for (int kb = 0; kb < K; kb += MG_KB) {
    const int n = K - kb < MG_KB ? K - kb : MG_KB;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      int m = order[start + kb + i], r = -1;
      if (m >= 0 && m < M) {
        const int64_t rr = mask_rows[m];
        if (rr >= 0 && rr < me_rows) r = (int)rr;
      }
      s_m[i] = r < 0 ? -1 : m;
      s_r[i] = r < 0 ? 0 : r;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < n; kk += 2) {
      const int i = kk + half;
      const int m = i < n ? s_m[i] : -1;
      float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
      if (m >= 0) {
        const float* g = G + (int64_t)m * P;
        const float* mr = mec + (int64_t)s_r[i] * 256;
        if (in0) a0 = g[pa0];
        if (in1) a1 = g[pa1];
        b0 = mr[0];
        b1 = mr[32];
      }
      acc00 = mfma32(a0, b0, acc00);
      acc01 = mfma32(a0, b1, acc01);
      acc10 = mfma32(a1, b0, acc10);
      acc11 = mfma32(a1, b1, acc11);
    }
  }
  float* out = dMF + ((int64_t)b * P + p0) * 256 + w * 64 + j;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = mfma32_row(r, half);
    if (p0 + row < P) {
      out[(int64_t)row * 256] = acc00[r];
      out[(int64_t)row * 256 + 32] = acc01[r];
    }
    if (p0 + 32 + row < P) {
      out[(int64_t)(32 + row) * 256] = acc10[r];
      out[(int64_t)(32 + row) * 256 + 32] = acc11[r];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
static inline int mg_slices(int64_t P) { return (int)((P + MG_KSLICE - 1) / MG_KSLICE); }

extern "C" int pn_mask_grad_kslice(void) { return MG_KSLICE; }

extern "C" int64_t pn_mask_embed_grad_scratch_floats(int T, int64_t P) {
  if (T <= 0 || P <= 0) return 0;
  return (int64_t)mg_slices(P) * T * 32 * 256;
}

extern "C" int pn_mask_embed_grad_f32(const float* G, const float* MF, const int64_t* mask_rows,
                                      const int32_t* table, int64_t table_len, int M, int B, int T,
                                      int64_t P, float* scratch, int64_t scratch_floats, float* dme,
                                      void* stream) {
  if (M < 0 || M > 65535 || B <= 0 || B > 65535 || T < 0 || P <= 0 || P > ((int64_t)1 << 31) - 64 ||
      table_len != (int64_t)B + 1 + M + 2 * (int64_t)T || !table)
    return PN_BAD_ARG;
  if (M == 0) return T == 0 ? 0 : PN_BAD_ARG;
  const int S = mg_slices(P);
  if (!G || !MF || !mask_rows || !scratch || !dme || T <= 0 || (int64_t)T * 32 < M ||
      (int64_t)T * S > 0x7fffffff / 32 || scratch_floats < (int64_t)S * T * 32 * 256)
    return PN_BAD_ARG;
  const int32_t *img_off = table, *order = table + B + 1, *tiles = order + M;
  hipLaunchKernelGGL(k_mask_embed_grad, dim3(T * S), dim3(256), 0, (hipStream_t)stream, G, MF,
                     mask_rows, img_off, order, tiles, M, B, T, P, S, scratch);
  int e = PN_LAUNCH_CHECK();
  if (e) return e;
  hipLaunchKernelGGL(k_mask_embed_grad_reduce, dim3(T * 32), dim3(256), 0, (hipStream_t)stream,
                     scratch, mask_rows, img_off, order, tiles, M, B, T, S, dme);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_mask_feature_grad_f32(const float* G, const float* me, const int64_t* mask_rows,
                                        const int32_t* table, int64_t table_len, int M, int B,
                                        int64_t P, int64_t me_rows, float* dMF, void* stream) {
  if (M < 0 || M > 65535 || B <= 0 || B > 65535 || P <= 0 || P > ((int64_t)1 << 31) - 64 ||
      me_rows < 0 || me_rows > ((int64_t)1 << 22) || !table || table_len < (int64_t)B + 1 + M ||
      !dMF || (M > 0 && (!G || !me || !mask_rows)))
    return PN_BAD_ARG;
  const int32_t *img_off = table, *order = table + B + 1;
  hipLaunchKernelGGL(k_mask_feature_grad, dim3((unsigned)((P + 63) / 64), B), dim3(256), 0,
                     (hipStream_t)stream, G, me, mask_rows, img_off, order, M, P, me_rows, dMF);
  return PN_LAUNCH_CHECK();
}
