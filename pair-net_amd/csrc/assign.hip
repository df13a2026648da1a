// Loss targets on the device: the two Hungarian assignments of `_get_target_single`
// (pairnet_head.py:645-718; `linear_sum_assignment(cost.cpu())` in approaches/matcher.py:262-264 and
// [3P] mmdet mask_hungarian_assigner.py) and the index bookkeeping behind them, so that a training
// step never waits for the host.
//
//   pn_lsa_f32       P rectangular assignment problems per launch, one wavefront each.  scipy's
//                    algorithm (Crouse's shortest augmenting paths, float64 duals) step for step,
//                    so that row_ind / col_ind EQUAL scipy's, ties included.
//   pn_loss_targets  query_of_gt, the importance target, r_labels / sub_ids / obj_ids and SeesawLoss's
//                    label histogram from the assignments, for the whole batch.
//
// Every loop has a static bound (rows, columns, path length); there is no spin, no flag and no
// atomic: the kernels end on any input, NaN and infinities included.
#include <math.h>

#include "common.h"

#define LSA_MAX_SIDE 1024
#define LSA_LDS_CELLS 24576        // cost entries staged in LDS (96 KB) beside 48 KB of state

// (value, tie key) argmin over the wave.  The tie key reproduces scipy's scan rule
//   if (shortest[j] < lowest || (shortest[j] == lowest && row4col[j] == -1)) take j
// over scan positions it = 0 .. num_remaining-1: among equal minima the LAST unassigned column
// in scan order wins, otherwise the FIRST column.  key = -it-1 for an unassigned column, it for an
// assigned one; the smallest (value, key) is scipy's choice.
__device__ __forceinline__ void wave_argmin(double& s, int& k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double s2 = __shfl_xor(s, o, 64);
    const int k2 = __shfl_xor(k, o, 64);
    if (s2 < s || (s2 == s && k2 < k)) { s = s2; k = k2; }
  }
}

__global__ __launch_bounds__(64) void k_lsa(const float* __restrict__ cost, int64_t cost_len,
                                            const int64_t* __restrict__ table,
                                            int32_t* __restrict__ row_ind,
                                            int32_t* __restrict__ col_ind, int64_t out_len,
                                            int32_t* __restrict__ status, int lds_cells) {
  extern __shared__ __attribute__((aligned(16))) float c_lds[];
  __shared__ double u[LSA_MAX_SIDE], v[LSA_MAX_SIDE], shortest[LSA_MAX_SIDE];
  __shared__ int path[LSA_MAX_SIDE], remaining[LSA_MAX_SIDE], col4row[LSA_MAX_SIDE],
      row4col[LSA_MAX_SIDE], sr[LSA_MAX_SIDE], sc[LSA_MAX_SIDE];
  const int lane = threadIdx.x, p = blockIdx.x;
  const int64_t off = table[4 * p], rows64 = table[4 * p + 1], cols64 = table[4 * p + 2],
                ooff = table[4 * p + 3];
  // a descriptor that points outside the operands: nothing is read or written but the status
  if (rows64 < 0 || cols64 < 0 || rows64 > LSA_MAX_SIDE || cols64 > LSA_MAX_SIDE || off < 0 ||
      ooff < 0 || off + rows64 * cols64 > cost_len || ooff + min(rows64, cols64) > out_len) {
    if (lane == 0) status[p] = 3;
    return;
  }
  const int rows = (int)rows64, cols = (int)cols64, n = min(rows, cols);
  if (n == 0) {
    if (lane == 0) status[p] = 0;
    return;
  }
  const bool transposed = cols < rows;
  const int nr = n, nc = max(rows, cols);
  const float* __restrict__ C = cost + off;
  const int cells = rows * cols;
  const bool staged = cells <= lds_cells;

  // scipy refuses NaN and -inf entries before it solves; the same pass stages the matrix
  // (transposed when cols < rows, so that c_lds[i * nc + j] is the solver's cost[i][j])
  bool bad = false;
  for (int idx = lane; idx < cells; idx += 64) {
    const float x = C[idx];
    bad |= (x != x) || (x == -INFINITY);
    if (staged) {
      if (transposed) {
        const int r = idx / cols, c = idx - r * cols;
        c_lds[c * nc + r] = x;
      } else {
        c_lds[idx] = x;
      }
    }
  }
  int32_t* __restrict__ ro = row_ind + ooff;
  int32_t* __restrict__ co = col_ind + ooff;
  if (__ballot(bad) != 0ull) {
    for (int k = lane; k < n; k += 64) { ro[k] = -1; co[k] = -1; }
    if (lane == 0) status[p] = 1;
    return;
  }
  for (int k = lane; k < nc; k += 64) {
    v[k] = 0.0; row4col[k] = -1; path[k] = -1;
    if (k < nr) { u[k] = 0.0; col4row[k] = -1; }
  }
  __syncthreads();

  for (int cur = 0; cur < nr; ++cur) {
    for (int k = lane; k < nc; k += 64) { shortest[k] = INFINITY; remaining[k] = nc - 1 - k; }
    __syncthreads();
    int num_remaining = nc, i = cur, nsr = 0, nsc = 0, sink = -1;
    double min_val = 0.0;
    for (int scan = 0; scan < nc && sink < 0; ++scan) {
      if (lane == 0) sr[nsr] = i;
      ++nsr;
      const double ui = u[i];
      double bs = INFINITY;
      int bk = INT_MAX;
      for (int it = lane; it < num_remaining; it += 64) {
        const int j = remaining[it];
        const double cij = staged ? (double)c_lds[i * nc + j]
                                  : (double)(transposed ? C[(int64_t)j * cols + i]
                                                        : C[(int64_t)i * cols + j]);
        const double r = min_val + cij - ui - v[j];
        double sj = shortest[j];
        if (r < sj) { path[j] = i; shortest[j] = r; sj = r; }
        const int k = row4col[j] == -1 ? -it - 1 : it;
        if (sj < bs || (sj == bs && k < bk)) { bs = sj; bk = k; }
      }
      wave_argmin(bs, bk);
      min_val = bs;
      if (bs == INFINITY) {                       // no finite edge left: infeasible
        for (int k = lane; k < n; k += 64) { ro[k] = -1; co[k] = -1; }
        if (lane == 0) status[p] = 2;
        return;
      }
      const int it = bk < 0 ? -bk - 1 : bk;
      const int j = remaining[it], last = remaining[num_remaining - 1];
      const int owner = row4col[j];
      __syncthreads();
      if (lane == 0) { sc[nsc] = j; remaining[it] = last; }
      ++nsc;
      --num_remaining;
      if (owner == -1) sink = j; else i = owner;
      __syncthreads();
    }
    if (sink < 0) {                               // (unreachable for nr <= nc; keeps path[] indexed)
      for (int k = lane; k < n; k += 64) { ro[k] = -1; co[k] = -1; }
      if (lane == 0) status[p] = 2;
      return;
    }
    // dual update
    if (lane == 0) u[cur] += min_val;
    for (int k = 1 + lane; k < nsr; k += 64) {
      const int r = sr[k];
      u[r] += min_val - shortest[col4row[r]];
    }
    for (int k = lane; k < nsc; k += 64) {
      const int j = sc[k];
      v[j] -= min_val - shortest[j];
    }
    __syncthreads();
    // augment back from the sink (every lane walks the path; lane 0 writes: a row of the path is
    // read before it is written and never again)
    int j = sink;
    for (int step = 0; step <= nr; ++step) {
      const int r = path[j];
      const int prev = col4row[r];
      if (lane == 0) { row4col[j] = r; col4row[r] = j; }
      j = prev;
      if (r == cur) break;
    }
    __syncthreads();
  }

  if (!transposed) {
    for (int k = lane; k < nr; k += 64) { ro[k] = k; co[k] = col4row[k]; }
  } else {
    // the pairs sorted by original row (scipy: argsort(col4row)): the assigned columns of the
    // transposed problem in ascending order, compacted 64 at a time
    int base = 0;
    for (int k0 = 0; k0 < nc; k0 += 64) {
      const int k = k0 + lane;
      const int r = k < nc ? row4col[k] : -1;
      const unsigned long long m = __ballot(r != -1);
      if (r != -1) {
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        ro[pos] = k;
        co[pos] = r;
      }
      base += __popcll(m);
    }
  }
  if (lane == 0) status[p] = 0;
}

extern "C" int pn_lsa_f32(const float* cost, int64_t cost_len, const int64_t* table, int P,
                          int64_t max_cells, int32_t* row_ind, int32_t* col_ind, int64_t out_len,
                          int32_t* status, void* stream) {
  if (!cost || !table || !row_ind || !col_ind || !status || P <= 0 || P > 65535 || cost_len <= 0 ||
      out_len <= 0 || max_cells < 0)
    return PN_BAD_ARG;
  const int lds_cells = (int)min((int64_t)LSA_LDS_CELLS, max_cells);
  hipLaunchKernelGGL(k_lsa, dim3(P), dim3(64), (size_t)lds_cells * sizeof(float),
                     (hipStream_t)stream, cost, cost_len, table, row_ind, col_ind, out_len, status,
                     lds_cells);
  return PN_LAUNCH_CHECK();
}

// ---- the bookkeeping of `_get_target_single` (pairnet_head.py:645-718) and SeesawLoss's label
// counts for a batch, from the assignments above.  One workgroup walks the images in order (B is a
// per-GPU batch: a handful), so the counts are added in a fixed order.
//   lsa_table [2B][4]  pn_lsa_f32's table: problem 2b = image b's Q x G mask assignment, 2b+1 its
//                      R x T triplet assignment
//   tgt_table [B][4]   {offset of gt_labels [G], offset of gt_rels [T][3], G, T}, offsets into gt
// status bits: pn_lsa_f32's (1 invalid entry, 2 infeasible, 3 descriptor) ORed over the problems, 4:
// a ground-truth index outside its range.  A non-zero status leaves the fills (importance 0, labels
// -1) and the counts untouched.
__global__ __launch_bounds__(256) void k_loss_targets(
    const int64_t* __restrict__ lsa_table, const int32_t* __restrict__ row_ind,
    const int32_t* __restrict__ col_ind, const int32_t* __restrict__ lsa_status,
    const int64_t* __restrict__ tgt_table, const int64_t* __restrict__ gt, int64_t gt_len, int B,
    int Q, int R, int C, float* __restrict__ importance, int64_t* __restrict__ labels,
    float* __restrict__ cum, int32_t* __restrict__ batch_status) {
  __shared__ int qog[LSA_MAX_SIDE];
  const int tid = threadIdx.x;
  int st = 0;
  for (int k = 0; k < 2 * B; ++k) st |= lsa_status[k];
  int bad = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t gl_off = tgt_table[4 * b], rel_off = tgt_table[4 * b + 1], G = tgt_table[4 * b + 2],
                  T = tgt_table[4 * b + 3];
    if (G < 0 || T < 0 || G > LSA_MAX_SIDE || gl_off < 0 || rel_off < 0 || gl_off + G > gt_len ||
        rel_off + 3 * T > gt_len || lsa_table[8 * b + 1] != Q || lsa_table[8 * b + 2] != G ||
        lsa_table[8 * b + 5] != R || lsa_table[8 * b + 6] != T) {
      bad = 1;
      continue;
    }
    for (int64_t t = tid; t < T; t += 256) {
      const int64_t s = gt[rel_off + 3 * t], o = gt[rel_off + 3 * t + 1], r = gt[rel_off + 3 * t + 2];
      bad |= s < 0 || s >= G || o < 0 || o >= G || r < 0 || r > C + 1;
    }
  }
  if (__syncthreads_or(bad)) st |= 4;
  const int64_t nimp = (int64_t)B * Q * Q, nlab = (int64_t)3 * B * R;
  for (int64_t k = tid; k < nimp; k += 256) importance[k] = 0.f;
  for (int64_t k = tid; k < nlab; k += 256) labels[k] = -1;
  __syncthreads();
  if (st != 0) {
    if (tid == 0) batch_status[0] = st;
    return;
  }
  int64_t* __restrict__ r_lab = labels;
  int64_t* __restrict__ s_ids = labels + (int64_t)B * R;
  int64_t* __restrict__ o_ids = labels + (int64_t)2 * B * R;
  for (int b = 0; b < B; ++b) {
    const int64_t gl_off = tgt_table[4 * b], rel_off = tgt_table[4 * b + 1];
    const int G = (int)tgt_table[4 * b + 2], T = (int)tgt_table[4 * b + 3];
    const int64_t o1 = lsa_table[8 * b + 3], o2 = lsa_table[8 * b + 7];
    // ground-truth object -> its matched query; unmatched ones keep the reference's 1
    // (`torch.ones_like`, pairnet_head.py:648)
    for (int g = tid; g < G; g += 256) qog[g] = 1;
    __syncthreads();
    for (int k = tid; k < min(Q, G); k += 256) qog[col_ind[o1 + k]] = row_ind[o1 + k];
    __syncthreads();
    float* __restrict__ imp = importance + (int64_t)b * Q * Q;
    for (int t = tid; t < T; t += 256)            // duplicates stay 1 (:660)
      imp[(int64_t)qog[gt[rel_off + 3 * t]] * Q + qog[gt[rel_off + 3 * t + 1]]] = 1.f;
    for (int k = tid; k < min(R, T); k += 256) {
      const int r = row_ind[o2 + k], t = col_ind[o2 + k];
      r_lab[(int64_t)b * R + r] = gt[rel_off + 3 * t + 2] - 1;
      s_ids[(int64_t)b * R + r] = gt[gl_off + gt[rel_off + 3 * t]];
      o_ids[(int64_t)b * R + r] = gt[gl_off + gt[rel_off + 3 * t + 1]];
    }
    __syncthreads();
  }
  // SeesawLoss accumulates this batch's kept labels before it weighs (seesaw_loss.py forward);
  // counts are whole numbers, exact in fp32 like the host's one-by-one additions (below 2^24)
  if (tid <= C) {
    int cnt = 0;
    for (int64_t k = 0; k < (int64_t)B * R; ++k) cnt += r_lab[k] == tid;
    if (cnt) cum[tid] += (float)cnt;
  }
  if (tid == 0) batch_status[0] = 0;
}

extern "C" int pn_loss_targets(const int64_t* lsa_table, const int32_t* row_ind,
                               const int32_t* col_ind, const int32_t* lsa_status,
                               const int64_t* tgt_table, const int64_t* gt, int64_t gt_len, int B,
                               int Q, int R, int C, float* importance, int64_t* labels,
                               float* cum_samples, int32_t* batch_status, void* stream) {
  if (!lsa_table || !row_ind || !col_ind || !lsa_status || !tgt_table || !gt || !importance ||
      !labels || !cum_samples || !batch_status || gt_len <= 0 || B <= 0 || B > 4096 || Q < 2 ||
      Q > LSA_MAX_SIDE || R <= 0 || R > LSA_MAX_SIDE || C <= 0 || C > 254)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_loss_targets, dim3(1), dim3(256), 0, (hipStream_t)stream, lsa_table, row_ind,
                     col_ind, lsa_status, tgt_table, gt, gt_len, B, Q, R, C, importance, labels,
                     cum_samples, batch_status);
  return PN_LAUNCH_CHECK();
}
