// The Mask2Former segmentation losses on device outputs: per-decoder-layer loss_cls / loss_mask /
// loss_dice with Hungarian matching per (layer, image), importance-sampled mask points and deep
// supervision -- values and d loss / d logits, no host wait.  What the reference computes with
// torch ops + scipy in panoptic_heads/mask2former_head.py:157-324 with
// maskformer_head.py:181-240,305-354 and panoptic_heads/point_sample.py:32-88 (word for word again
// in relation_heads/baseline.py:588-653).  The assignment itself is pn_lsa_f32 (csrc/assign.hip) on
// costs from pn_point_sample_f32 / pn_mask_match_cost_f32 (csrc/loss.hip); this file holds what is
// new: the counter-based uniform draws, the targets' bookkeeping, the per-mask point machinery
// (selection of the k most uncertain candidates, per-row point sampling, the per-mask sums and their
// derivative) and the transpose of the bilinear sample.  Everything is fp32 in the reference's
// formulas, with fixed-order reductions and no floating-point atomics: two launches on the same
// inputs give the same bits.
#include "common.h"

#define SEG_EPS32 1.1920928955078125e-07f    // torch.finfo(torch.float32).eps (weight_reduce_loss)
#define SEG_MAX_ROWS 4096
#define SEG_MAX_LAYERS 64

__device__ __forceinline__ float seg_block_sum(float v, float* red) {   // <= 1024 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < nw; ++w) t += red[w];      // every thread, wave order: deterministic
  return t;
}

// ---- Philox4x32-10 (Salmon et al., SC'11), the construction of csrc/dropout.hip ----
__device__ __forceinline__ void seg_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// out[s][i] = (word >> 8) * 2^-24 in [0, 1): word i % 4 of the block at counter
// (i / 4, rank, site + s * site_stride, step), key (seed & 0xffffffff, seed >> 32).
__global__ __launch_bounds__(256) void k_uniform(float* __restrict__ out, int64_t n, uint32_t key0,
                                                 uint32_t key1, uint32_t rank, uint32_t step,
                                                 uint32_t site, uint32_t site_stride) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const int64_t i0 = (int64_t)j * 4;
  if (i0 >= n) return;
  uint32_t w[4];
  seg_philox(j, rank, site + blockIdx.y * site_stride, step, key0, key1, w);
  float* o = out + (int64_t)blockIdx.y * n;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n) o[i0 + k] = (float)(w[k] >> 8) * 5.9604644775390625e-08f;
}

extern "C" int pn_uniform_f32(float* out, int64_t n, int nsites, uint32_t site_stride,
                              uint64_t seed, uint32_t rank, uint32_t step, uint32_t site,
                              void* stream) {
  if (!out || n <= 0 || n > ((int64_t)1 << 34) || nsites <= 0 || nsites > 65535) return PN_BAD_ARG;
  const int64_t blocks = ((n + 3) / 4 + 255) / 256;      // (int64: n / 4 exceeds int above 2^33)
  hipLaunchKernelGGL(k_uniform, dim3((unsigned)blocks, nsites), dim3(256), 0,
                     (hipStream_t)stream, out, n, (uint32_t)(seed & 0xffffffffu),
                     (uint32_t)(seed >> 32), rank, step, site, site_stride);
  return PN_LAUNCH_CHECK();
}

// ---- targets of every (layer, image) from the batched assignment (mask2former_head.py:205-221
// with MaskPseudoSampler: positives in ascending query order) ----
// One workgroup walks the P = L * B problems in order.  A problem whose assignment failed, or
// whose indices / labels are out of range, keeps its fills: labels = num_classes, matched rows -1.
__global__ __launch_bounds__(256) void k_seg_targets(
    const int64_t* __restrict__ table, const int32_t* __restrict__ row_ind,
    const int32_t* __restrict__ col_ind, const int32_t* __restrict__ lsa_status,
    int nlsa, const int64_t* __restrict__ gt_labels, int64_t gt_len, int64_t out_len, int L, int B,
    int Q, int C, int64_t Mtot, int64_t* __restrict__ labels, int64_t* __restrict__ matched,
    int32_t* __restrict__ mcount, int32_t* __restrict__ status) {
  __shared__ int bad;
  const int tid = threadIdx.x;
  int acc = 0;
  for (int l = tid; l < L; l += 256) mcount[l] = 0;
  for (int p = 0; p < L * B; ++p) {
    const int64_t* t = table + (int64_t)p * 6;
    const int64_t li = t[0], off = t[1], n = t[2], goff = t[3], G = t[4], dst = t[5];
    if (tid == 0) bad = 0;
    for (int q = tid; q < Q; q += 256) labels[(int64_t)p * Q + q] = C;
    int st = (li >= 0 && li < nlsa) ? lsa_status[li] : 0;
    if (li >= nlsa || n < 0 || n > Q || off < 0 || off + n > out_len || dst < 0 || dst + n > Mtot || goff < 0 ||
        G < 0 || goff + G > gt_len)
      st |= 8;
    if (st & 8) { acc |= st; continue; }             // (uniform: every thread read the same row)
    for (int64_t i = tid; i < n; i += 256)
#pragma unroll
      for (int k = 0; k < 4; ++k) matched[(dst + i) * 4 + k] = -1;
    __syncthreads();
    if (st == 0) {
      for (int64_t i = tid; i < n; i += 256) {
        const int q = row_ind[off + i], g = col_ind[off + i];
        bool ok = q >= 0 && q < Q && g >= 0 && g < G;
        if (ok) { const int64_t y = gt_labels[goff + g]; ok = y >= 0 && y < C; }
        if (!ok) atomicOr(&bad, 4);
      }
    }
    __syncthreads();
    st |= bad;
    if (st == 0) {
      for (int64_t i = tid; i < n; i += 256) {
        const int q = row_ind[off + i], g = col_ind[off + i];
        labels[(int64_t)p * Q + q] = gt_labels[goff + g];
        int64_t* m = matched + (dst + i) * 4;
        m[0] = p / B, m[1] = p % B, m[2] = q, m[3] = goff + g;
      }
      if (tid == 0) mcount[p / B] += (int)n;
    }
    acc |= st;
    __syncthreads();
  }
  if (tid == 0) status[0] = acc;
}

extern "C" int pn_seg_targets(const int64_t* table, const int32_t* row_ind, const int32_t* col_ind,
                              const int32_t* lsa_status, int nlsa, const int64_t* gt_labels,
                              int64_t gt_len, int64_t out_len, int L, int B, int Q, int C, int64_t Mtot,
                              int64_t* labels, int64_t* matched, int32_t* mcount, int32_t* status,
                              void* stream) {
  if (!table || !row_ind || !col_ind || !lsa_status || !gt_labels || !labels || !mcount || !status ||
      (!matched && Mtot > 0) || L <= 0 || L > SEG_MAX_LAYERS || B <= 0 || Q <= 0 || C <= 0 ||
      Mtot < 0 || gt_len < 0 || out_len < 0 || nlsa < 0 || (int64_t)L * B > 65536)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_seg_targets, dim3(1), dim3(256), 0, (hipStream_t)stream, table, row_ind,
                     col_ind, lsa_status, nlsa, gt_labels, gt_len, out_len, L, B, Q, C, Mtot,
                     labels, matched, mcount, status);
  return PN_LAUNCH_CHECK();
}

// ---- mmcv point_sample's arithmetic, as k_point_sample (csrc/loss.hip) states it:
// F.grid_sample(input, 2 p - 1, bilinear, zeros padding, align_corners=False) ----
struct SegTaps { int x0, y0; float nw, ne, sw, se; };
__device__ __forceinline__ SegTaps seg_taps(float px, float py, int h, int w) {
  const float cx = 2.f * px - 1.f, cy = 2.f * py - 1.f;
  const float ix = ((cx + 1.f) * (float)w - 1.f) / 2.f, iy = ((cy + 1.f) * (float)h - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  SegTaps t;
  t.x0 = (int)fminf(fmaxf(fx, -2.f), (float)w), t.y0 = (int)fminf(fmaxf(fy, -2.f), (float)h);
  const float x1f = fx + 1.f, y1f = fy + 1.f;
  t.nw = (x1f - ix) * (y1f - iy), t.ne = (ix - fx) * (y1f - iy);
  t.sw = (x1f - ix) * (iy - fy), t.se = (ix - fx) * (iy - fy);
  return t;
}
template <typename T>
__device__ __forceinline__ float seg_sample(const T* __restrict__ m, int h, int w, float px,
                                            float py) {
  const SegTaps t = seg_taps(px, py, h, w);
  auto at = [&](int y, int x) -> float {
    return (x >= 0 && x < w && y >= 0 && y < h) ? (float)m[(int64_t)y * w + x] : 0.f;
  };
  float v = 0.f;       // accumulated in ATen's order: nw, ne, sw, se
  v += at(t.y0, t.x0) * t.nw;
  v += at(t.y0, t.x0 + 1) * t.ne;
  v += at(t.y0 + 1, t.x0) * t.sw;
  v += at(t.y0 + 1, t.x0 + 1) * t.se;
  return v;
}

// ---- get_uncertain_point_coords_with_randomness (point_sample.py:32-88) for one matched mask
// per workgroup: sample the S candidates, keep the k with the smallest |logit| (what
// torch.topk(-|x|, k) keeps; ties to the lower candidate index), append the tail points.
// The keys |x| as fp32 bit patterns go to a global scratch row [S] (150 KB at S = 37 632: it
// stays in L2 between the passes; LDS holds only the 256-bin histogram, so occupancy is not
// bound by it): an 8-bit radix select over four passes finds the k-th key, one more pass
// compacts the kept candidates in ascending candidate order.
__global__ __launch_bounds__(1024) void k_uncertain_points(
    const float* __restrict__ maps, int64_t nmaps, const int64_t* __restrict__ matched, int B, int Q,
    int h, int w, const float* __restrict__ cand, const float* __restrict__ tail, int S, int k, int Np,
    uint32_t* __restrict__ keys, float* __restrict__ pts) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_prefix, s_remaining;
  __shared__ unsigned weq[16], wsel[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = blockIdx.x;
  const int64_t* row = matched + m * 4;
  const int64_t l = row[0], r = (l * B + row[1]) * Q + row[2];
  float2* out = reinterpret_cast<float2*>(pts) + m * Np;
  uint32_t* key = keys + m * S;
  if (l < 0 || row[1] < 0 || row[1] >= B || row[2] < 0 || row[2] >= Q || r >= nmaps) {
    // (uniform) an unassigned row: zeros
    for (int i = tid; i < Np; i += 1024) out[i] = make_float2(0.f, 0.f);
    for (int i = tid; i < S; i += 1024) key[i] = 0u;
    return;
  }
  const float* map = maps + r * (int64_t)h * w;
  const float2* c = reinterpret_cast<const float2*>(cand) + m * S;
  for (int i = tid; i < S; i += 1024) {
    const float2 p = c[i];
    key[i] = __float_as_uint(fabsf(seg_sample(map, h, w, p.x, p.y)));
  }
  for (int i = tid; i < Np - k; i += 1024)
    out[k + i] = reinterpret_cast<const float2*>(tail)[m * (Np - k) + i];
  if (k == 0) return;
  __syncthreads();
  unsigned prefix = 0, remaining = (unsigned)k;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass ? (0xffffffffu << (shift + 8)) : 0u;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < S; i += 1024) {
      const unsigned v = key[i];
      if ((v & himask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned cum = 0, b = 0;
      for (; b < 255; ++b) {
        if (cum + hist[b] >= remaining) break;
        cum += hist[b];
      }
      s_prefix = prefix | (b << shift);
      s_remaining = remaining - cum;
    }
    __syncthreads();
    prefix = s_prefix, remaining = s_remaining;
  }
  // keys below `prefix` are kept, and the first `remaining` of those equal to it
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned run_eq = 0, run_sel = 0;
  for (int base = 0; base < S; base += 1024) {
    const int i = base + tid;
    const unsigned v = i < S ? key[i] : 0xffffffffu;
    const bool lt = i < S && v < prefix, eq = i < S && v == prefix;
    const unsigned long long beq = __ballot(eq);
    if (lane == 0) weq[wave] = (unsigned)__popcll(beq);
    __syncthreads();
    unsigned eq_before = run_eq + (unsigned)__popcll(beq & below), eq_all = 0;
    for (int x = 0; x < 16; ++x) {
      if (x < wave) eq_before += weq[x];
      eq_all += weq[x];
    }
    const bool sel = lt || (eq && eq_before < remaining);
    const unsigned long long bsel = __ballot(sel);
    if (lane == 0) wsel[wave] = (unsigned)__popcll(bsel);
    __syncthreads();
    unsigned pos = run_sel + (unsigned)__popcll(bsel & below), sel_all = 0;
    for (int x = 0; x < 16; ++x) {
      if (x < wave) pos += wsel[x];
      sel_all += wsel[x];
    }
    if (sel && pos < (unsigned)k) out[pos] = c[i];
    run_eq += eq_all, run_sel += sel_all;
  }
}

extern "C" int pn_uncertain_points_f32(const float* maps, int64_t nmaps, const int64_t* matched,
                                       int64_t M, int B, int Q, int h, int w, const float* cand,
                                       const float* tail, int S, int k, int Np, uint32_t* keys,
                                       float* pts, void* stream) {
  if (!maps || !matched || !cand || !keys || !pts || M <= 0 || M > 0x7fffffff || B <= 0 || Q <= 0 ||
      h <= 0 || w <= 0 || S <= 0 || k < 0 || k > Np || k > S || Np <= 0 || (!tail && k < Np) ||
      nmaps <= 0 || (((uintptr_t)cand | (uintptr_t)tail | (uintptr_t)pts) & 7))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_uncertain_points, dim3((unsigned)M), dim3(1024), 0, (hipStream_t)stream, maps,
                     nmaps, matched, B, Q, h, w, cand, tail, S, k, Np, keys, pts);
  return PN_LAUNCH_CHECK();
}

// ---- point_sample with a point set PER ROW (mask2former_head.py:300-306): row m reads map
// idx[m] (idx < 0: zeros); maps fp32 logits or uint8 0/1 targets; pts [M][Np][2]; out [M][Np].
template <typename T>
__global__ __launch_bounds__(256) void k_point_sample_rows(const T* __restrict__ maps,
                                                           const int64_t* __restrict__ idx,
                                                           int64_t nmaps,
                                                           const float* __restrict__ pts,
                                                           float* __restrict__ out, int h, int w,
                                                           int Np) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t m = blockIdx.y;
  if (i >= Np) return;
  const int64_t r = idx[m];
  float v = 0.f;
  if (r >= 0 && r < nmaps) {
    const float2 p = reinterpret_cast<const float2*>(pts)[m * Np + i];
    v = seg_sample(maps + r * (int64_t)h * w, h, w, p.x, p.y);
  }
  out[m * Np + i] = v;
}

extern "C" int pn_point_sample_rows_f32(const void* maps, int maps_are_u8, int64_t nmaps,
                                        const int64_t* idx, const float* pts, float* out, int64_t M,
                                        int h, int w, int Np, void* stream) {
  if (!maps || !idx || !pts || !out || nmaps <= 0 || M <= 0 || M > 65535 || h <= 0 || w <= 0 ||
      Np <= 0 || ((uintptr_t)pts & 7))
    return PN_BAD_ARG;
  const dim3 grid(pn_cdiv(Np, 256), (unsigned)M);
  if (maps_are_u8)
    hipLaunchKernelGGL(k_point_sample_rows<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)maps, idx, nmaps, pts, out, h, w, Np);
  else
    hipLaunchKernelGGL(k_point_sample_rows<float>, grid, dim3(256), 0, (hipStream_t)stream,
                       (const float*)maps, idx, nmaps, pts, out, h, w, Np);
  return PN_LAUNCH_CHECK();
}

// ---- loss_mask (sigmoid CrossEntropyLoss) and loss_dice (DiceLoss: use_sigmoid, activate,
// naive_dice) over the sampled points of the matched masks (mask2former_head.py:308-322):
//   per mask m: sums[m] = { sum_p BCE(x, t), a = sum_p s t, b = sum_p s, c = sum_p t }, s = sigmoid(x)
//   loss_mask[l] = w_mask * sum_m sums[m][0] / (N_l * Np + eps32)
//   loss_dice[l] = w_dice * sum_m (1 - (2 a + eps) / (b + c + eps)) / (N_l + eps32)
// N_l = num_total_masks: the argument when > 0, else max(#assigned rows of the layer, 1).
__global__ __launch_bounds__(256) void k_mask_point_sums(const float* __restrict__ x,
                                                         const float* __restrict__ t,
                                                         const int64_t* __restrict__ matched,
                                                         float* __restrict__ sums, int Np) {
  __shared__ float red[8];
  const int64_t m = blockIdx.x;
  float bce = 0.f, a = 0.f, b = 0.f, c = 0.f;
  if (matched[m * 4] >= 0) {                         // (uniform)
    for (int i = threadIdx.x; i < Np; i += 256) {
      const float xv = x[m * Np + i], tv = t[m * Np + i];
      const float s = 1.f / (1.f + expf(-xv));
      bce += (fmaxf(xv, 0.f) - xv * tv) + log1pf(expf(-fabsf(xv)));
      a += s * tv, b += s, c += tv;
    }
  }
  bce = seg_block_sum(bce, red), a = seg_block_sum(a, red);
  b = seg_block_sum(b, red), c = seg_block_sum(c, red);
  if (threadIdx.x == 0) {
    float* o = sums + m * 4;
    o[0] = bce, o[1] = a, o[2] = b, o[3] = c;
  }
}

// thread l sums layer l's rows in table order; out [4L] = loss_mask | loss_dice | the two
// denominators (read by k_mask_point_coef)
__global__ __launch_bounds__(64) void k_mask_point_finish(const float* __restrict__ sums,
                                                          const int64_t* __restrict__ matched,
                                                          float* __restrict__ out, int L, int Ml,
                                                          int Np, float w_mask, float w_dice,
                                                          float eps, float ntm) {
  const int l = threadIdx.x;
  if (l >= L) return;
  float bce = 0.f, dice = 0.f;
  int cnt = 0;
  for (int64_t m = (int64_t)l * Ml; m < (int64_t)(l + 1) * Ml; ++m) {
    if (matched[m * 4] < 0) continue;
    const float* s = sums + m * 4;
    bce += s[0];
    dice += 1.f - (2.f * s[1] + eps) / ((s[2] + s[3]) + eps);
    ++cnt;
  }
  const float N = ntm > 0.f ? ntm : (float)(cnt > 1 ? cnt : 1);
  const float den_mask = N * (float)Np + SEG_EPS32, den_dice = N + SEG_EPS32;
  out[l] = w_mask * (bce / den_mask);
  out[L + l] = w_dice * (dice / den_dice);
  out[2 * L + l] = den_mask;
  out[3 * L + l] = den_dice;
}

// d (loss_mask[l] + loss_dice[l]) / d x[m][p]:
//   w_mask (s - t) / den_mask + w_dice / den_dice * ((2 a + eps) - 2 t (b + c + eps)) / (b + c + eps)^2 * s (1 - s)
__global__ __launch_bounds__(256) void k_mask_point_coef(const float* __restrict__ x,
                                                         const float* __restrict__ t,
                                                         const int64_t* __restrict__ matched,
                                                         const float* __restrict__ sums,
                                                         const float* __restrict__ out,
                                                         float* __restrict__ coef, int L, int Np,
                                                         float w_mask, float w_dice, float eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int64_t m = blockIdx.y;
  if (i >= Np) return;
  const int64_t l = matched[m * 4];
  float g = 0.f;
  if (l >= 0) {
    const float xv = x[m * Np + i], tv = t[m * Np + i];
    const float s = 1.f / (1.f + expf(-xv));
    const float* sm = sums + m * 4;
    const float num = 2.f * sm[1] + eps, den = (sm[2] + sm[3]) + eps;
    const float gm = w_mask * ((s - tv) / out[2 * L + l]);
    const float gd = (w_dice / out[3 * L + l]) * (((num - 2.f * tv * den) / (den * den)) * (s * (1.f - s)));
    g = gm + gd;
  }
  coef[m * Np + i] = g;
}

extern "C" int pn_mask_point_loss_f32(const float* x, const float* t, const int64_t* matched,
                                      int64_t M, int Np, int L, int Ml, float w_mask, float w_dice,
                                      float dice_eps, float num_total_masks, float* sums, float* out,
                                      float* coef, void* stream) {
  if (!x || !t || !matched || !sums || !out || M <= 0 || M > 65535 || Np <= 0 || L <= 0 ||
      L > SEG_MAX_LAYERS || Ml <= 0 || (int64_t)L * Ml != M)
    return PN_BAD_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mask_point_sums, dim3((unsigned)M), dim3(256), 0, s, x, t, matched, sums, Np);
  hipLaunchKernelGGL(k_mask_point_finish, dim3(1), dim3(64), 0, s, sums, matched, out, L, Ml, Np,
                     w_mask, w_dice, dice_eps, num_total_masks);
  if (coef)
    hipLaunchKernelGGL(k_mask_point_coef, dim3(pn_cdiv(Np, 256), (unsigned)M), dim3(256), 0, s, x, t,
                       matched, sums, out, coef, L, Np, w_mask, w_dice, dice_eps);
  return PN_LAUNCH_CHECK();
}

// ---- the transpose of the bilinear sample: coef [M][Np] at pts [M][Np][2] -> grad [M][h][w],
// grad[m][y][x] = sum over the points p whose tap falls on (y, x) of coef[m][p] * weight.
// No floating-point atomics (sums of them differ from run to run): an inverted index.  One
// workgroup per mask sorts the mask's points by the pixel of their top-left tap -- a counting sort
// over the (h + 1) x (w + 1) possible top-left pixels (-1 .. h-1, -1 .. w-1), made stable by ranking
// every point among the points of its bin by point index -- and every output pixel then sums the
// up-to-four bins that reach it, bin by bin and point by point in that order.  Taps outside the map
// are dropped, as the forward drops them; a point with no tap inside is in no bin.
// scratch per mask: nb + 1 bin ends, Np unordered slots, Np ordered slots (int32).
__device__ __forceinline__ int seg_bin(const SegTaps& t, int h, int w) {
  return (t.x0 >= -1 && t.x0 <= w - 1 && t.y0 >= -1 && t.y0 <= h - 1)
             ? (t.y0 + 1) * (w + 1) + (t.x0 + 1) : -1;
}

__global__ __launch_bounds__(1024) void k_point_scatter_grad(const float* __restrict__ coef,
                                                             const float* __restrict__ pts,
                                                             float* __restrict__ grad,
                                                             int* __restrict__ scratch, int Np,
                                                             int h, int w) {
  __shared__ int wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m = blockIdx.x;
  const int nb = (h + 1) * (w + 1);
  int* cnt = scratch + m * ((int64_t)nb + 2 * (int64_t)Np);
  int* seg = cnt + nb;
  int* order = seg + Np;
  const float2* p2 = reinterpret_cast<const float2*>(pts) + m * Np;
  const float* cf = coef + m * Np;
  for (int j = tid; j < nb; j += 1024) cnt[j] = 0;
  __syncthreads();
  for (int i = tid; i < Np; i += 1024) {
    const float2 p = p2[i];
    const int b = seg_bin(seg_taps(p.x, p.y, h, w), h, w);
    if (b >= 0) atomicAdd(&cnt[b], 1);
  }
  __syncthreads();
  // exclusive scan of the counts: a contiguous chunk per thread, a block scan of the chunk sums
  const int chunk = (nb + 1023) / 1024, j0 = tid * chunk, j1 = min(j0 + chunk, nb);
  int local = 0;
  for (int j = j0; j < j1; ++j) local += cnt[j];
  int incl = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int start = incl - local;
  for (int x = 0; x < wave; ++x) start += wtot[x];
  for (int j = j0; j < j1; ++j) {
    const int c = cnt[j];
    cnt[j] = start;
    start += c;
  }
  __syncthreads();
  // unordered placement: afterwards cnt[b] is the END of bin b (its begin: cnt[b - 1], or 0)
  for (int i = tid; i < Np; i += 1024) {
    const float2 p = p2[i];
    const int b = seg_bin(seg_taps(p.x, p.y, h, w), h, w);
    if (b >= 0) seg[atomicAdd(&cnt[b], 1)] = i;
  }
  __syncthreads();
  // stable order: the rank of a point among its bin's points is the number with a smaller index
  for (int i = tid; i < Np; i += 1024) {
    const float2 p = p2[i];
    const int b = seg_bin(seg_taps(p.x, p.y, h, w), h, w);
    if (b < 0) continue;
    const int beg = b ? cnt[b - 1] : 0, end = cnt[b];
    int r = 0;
    for (int j = beg; j < end; ++j) r += seg[j] < i;
    order[beg + r] = i;
  }
  __syncthreads();
  float* g = grad + m * (int64_t)h * w;
  for (int px = tid; px < h * w; px += 1024) {
    const int y = px / w, x = px - y * w;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // bin (y + dy, x + dx) holds the points whose top-left tap is (y + dy - 1, x + dx - 1)
      const int dy = q >> 1, dx = q & 1;
      const int b = (y + dy) * (w + 1) + (x + dx);
      const int beg = b ? cnt[b - 1] : 0, end = cnt[b];
      for (int j = beg; j < end; ++j) {
        const int i = order[j];
        const float2 p = p2[i];
        const SegTaps t = seg_taps(p.x, p.y, h, w);
        const float wt = dy ? (dx ? t.nw : t.ne) : (dx ? t.sw : t.se);
        s += cf[i] * wt;
      }
    }
    g[px] = s;
  }
}

extern "C" int64_t pn_point_scatter_scratch_ints(int64_t M, int Np, int h, int w) {
  if (M <= 0 || Np <= 0 || h <= 0 || w <= 0) return 0;
  return M * ((int64_t)(h + 1) * (w + 1) + 2 * (int64_t)Np);
}

extern "C" int pn_point_scatter_grad_f32(const float* coef, const float* pts, float* grad,
                                         int32_t* scratch, int64_t M, int Np, int h, int w,
                                         void* stream) {
  if (!coef || !pts || !grad || !scratch || M <= 0 || M > 0x7fffffff || Np <= 0 || h <= 0 ||
      w <= 0 || (int64_t)(h + 1) * (w + 1) > (1 << 28) || ((uintptr_t)pts & 7))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_point_scatter_grad, dim3((unsigned)M), dim3(1024), 0, (hipStream_t)stream,
                     coef, pts, grad, scratch, Np, h, w);
  return PN_LAUNCH_CHECK();
}

// ---- loss_cls: mmdet CrossEntropyLoss (softmax, class weights) with
// avg_factor = class_weight[labels].sum() (mask2former_head.py:273-276):
//   out[l] = loss_weight * sum_r cw[y_r] (lse(x_r) - x_r[y_r]) / (sum_r cw[y_r] + eps32)
// k_ce_mean's row layout (csrc/loss.hip); one workgroup per layer, rows = B * Q summed in row order.
__global__ __launch_bounds__(256) void k_ce_avg(const float* __restrict__ logits,
                                                const int64_t* __restrict__ target,
                                                const float* __restrict__ cw,
                                                float* __restrict__ out, int rows, int C,
                                                float loss_weight) {
  __shared__ float per_row[SEG_MAX_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (int64_t)blockIdx.x * rows * C;
  const int64_t* tg = target + (int64_t)blockIdx.x * rows;
  for (int r = wave; r < rows; r += 4) {
    const int64_t y = tg[r];
    const float* xr = x + (int64_t)r * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
    m = wave_max(m);
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d += expf(xr[c] - m);
    d = wave_sum(d);
    if (lane == 0) per_row[r] = ((logf(d) + m) - xr[y]) * cw[y];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f, den = 0.f;
    for (int r = 0; r < rows; ++r) { s += per_row[r]; den += cw[tg[r]]; }
    out[blockIdx.x] = loss_weight * (s / (den + SEG_EPS32));
  }
}

//   g[r][c] = loss_weight * cw[y_r] / (sum_r cw[y_r] + eps32) * (softmax(x_r)[c] - [c == y_r])
__global__ __launch_bounds__(256) void k_ce_avg_grad(const float* __restrict__ logits,
                                                     const int64_t* __restrict__ target,
                                                     const float* __restrict__ cw,
                                                     float* __restrict__ grad, int rows, int C,
                                                     float loss_weight) {
  __shared__ float s_den;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (int64_t)blockIdx.x * rows * C;
  float* gx = grad + (int64_t)blockIdx.x * rows * C;
  const int64_t* tg = target + (int64_t)blockIdx.x * rows;
  if (threadIdx.x == 0) {
    float den = 0.f;
    for (int r = 0; r < rows; ++r) den += cw[tg[r]];
    s_den = den + SEG_EPS32;
  }
  __syncthreads();
  const float scale = loss_weight / s_den;
  for (int r = wave; r < rows; r += 4) {
    const int64_t y = tg[r];
    const float* xr = x + (int64_t)r * C;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, xr[c]);
    m = wave_max(m);
    float d = 0.f;
    for (int c = lane; c < C; c += 64) d += expf(xr[c] - m);
    d = wave_sum(d);
    const float wy = scale * cw[y];
    for (int c = lane; c < C; c += 64)
      gx[(int64_t)r * C + c] = wy * (expf(xr[c] - m) / d - (c == (int)y ? 1.f : 0.f));
  }
}

// targets outside [0, C) would index the class weights out of bounds: they are the caller's
// contract (here C = num_classes + 1 logits; pn_seg_targets, whose own C is num_classes, writes only
// ground-truth labels it has range-checked against [0, num_classes), or num_classes = this C - 1)
extern "C" int pn_ce_avg_f32(const float* logits, const int64_t* target, const float* class_weight,
                             float* out, int L, int rows, int C, float loss_weight, void* stream) {
  if (!logits || !target || !class_weight || !out || L <= 0 || L > 65535 || rows <= 0 ||
      rows > SEG_MAX_ROWS || C <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_ce_avg, dim3(L), dim3(256), 0, (hipStream_t)stream, logits, target,
                     class_weight, out, rows, C, loss_weight);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_ce_avg_grad_f32(const float* logits, const int64_t* target,
                                  const float* class_weight, float* grad, int L, int rows, int C,
                                  float loss_weight, void* stream) {
  if (!logits || !target || !class_weight || !grad || L <= 0 || L > 65535 || rows <= 0 ||
      rows > SEG_MAX_ROWS || C <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_ce_avg_grad, dim3(L), dim3(256), 0, (hipStream_t)stream, logits, target,
                     class_weight, grad, rows, C, loss_weight);
  return PN_LAUNCH_CHECK();
}
