// The relation terms of the sibling head's loss (relation_heads/baseline.py:655-694, 828-907 with
// OldIdMatcher, approaches/matcher.py:279-351, and MultilabelCrossEntropy, losses/seg_losses.py:47-57,
// under configs/mask2former/baseline_r50_psg.py:336-350, 373-378): the id match cost of every image in
// one launch, the targets' bookkeeping behind the Hungarian assignment (pn_lsa_f32, csrc/assign.hip)
// and the filtered multilabel cross entropy of the subject / object id scores -- values and
// d loss / d scores.  r_loss_cls itself is pn_ce_avg_f32 / pn_ce_avg_grad_f32 (csrc/seg_loss.hip) on
// the labels written here.  The data are tiny (B x 100 x 100 scores, a few dozen relations per image):
// the cost is launches and dependent loads, so every kernel covers the whole batch and their number
// does not grow with B.  fp32 in the reference's formulas, fixed-order reductions, no floating-point
// atomics: two launches on the same inputs give the same bits.
//
// The per-image table `tab` [B][8] int64 (built on the host from shapes alone):
//   {offset of the image's R x Gr cost block in `cost`, Gr, offset of its rows in gt_rels [.][3],
//    offset of its last-layer rows in `matched`, their number n = min(Q, G), offset of its objects
//    in the batch's concatenated ground truth (what matched[.][3] counts from), G,
//    offset of its P = min(R, Gr) entries in row_ind / col_ind / pos / row_loss}
#include "common.h"

#define REL_MAX_SIDE 1024     // Q, R and the objects of one image (LDS maps)

struct RelTab { int64_t coff, Gr, roff, moff, n, goff, G, poff; };

__device__ __forceinline__ RelTab rel_tab(const int64_t* __restrict__ tab, int b) {
  const int64_t* t = tab + (int64_t)b * 8;
  RelTab r;
  r.coff = t[0], r.Gr = t[1], r.roff = t[2], r.moff = t[3], r.n = t[4], r.goff = t[5], r.G = t[6],
  r.poff = t[7];
  return r;
}

// every offset the kernels below add to a pointer, checked against the buffers' lengths
__device__ __forceinline__ bool rel_tab_ok(const RelTab& t, int R, int Q, int64_t cost_len,
                                           int64_t rel_len, int64_t Mtot, int64_t pos_len) {
  if (t.Gr <= 0 || t.Gr > ((int64_t)1 << 24) || t.n < 0 || t.n > Q || t.G < 0 || t.G > REL_MAX_SIDE ||
      t.coff < 0 || t.roff < 0 || t.moff < 0 || t.poff < 0 || t.goff < 0)
    return false;
  const int64_t P = t.Gr < R ? t.Gr : R;
  return t.coff + (int64_t)R * t.Gr <= cost_len && t.roff + t.Gr <= rel_len &&
         t.moff + t.n <= Mtot && t.poff + P <= pos_len;
}

// softmax statistics of one row over a wavefront: max and the sum of exp(x - max), any length
__device__ __forceinline__ void rel_row_stats(const float* __restrict__ x, int n, int lane, float& m,
                                              float& d) {
  m = -INFINITY;
  for (int c = lane; c < n; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  d = 0.f;
  for (int c = lane; c < n; c += 64) d += expf(x[c] - m);
  d = wave_sum(d);
}

// ---- the id match cost (OldIdMatcher.assign, matcher.py:323-330: ClassificationCost three times)
//   cost[r][k] = (-w_s softmax(sub[r])[a[s_k]] - w_o softmax(obj[r])[a[o_k]]) - w_r softmax(rel[r])[p_k]
// a: ground-truth object -> its matched query of the last decoder layer, 1 for the rest
// (`torch.ones_like`, baseline.py:829-830).  grid (ceil(R / 4), B): a wavefront owns a relation-query
// row, forms the three denominators, then its lanes walk k.  An image whose last-layer segmentation
// assignment failed (matched rows -1) gets a cost block of zeros; pn_rel_targets skips it.
__global__ __launch_bounds__(256) void k_rel_id_cost(
    const float* __restrict__ rel, const float* __restrict__ sub, const float* __restrict__ obj,
    const int64_t* __restrict__ gt_rels, int64_t rel_len, const int64_t* __restrict__ matched,
    int64_t Mtot, const int64_t* __restrict__ tab, float* __restrict__ cost, int64_t cost_len, int R,
    int Q, int C1, float w_s, float w_o, float w_r) {
#pragma clang fp contract(off)
  __shared__ int a_q[REL_MAX_SIDE];
  __shared__ int seg_ok;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RelTab t = rel_tab(tab, b);
  if (!rel_tab_ok(t, R, Q, cost_len, rel_len, Mtot, (int64_t)1 << 62)) return;   // (uniform)
  for (int g = tid; g < t.G; g += 256) a_q[g] = 1;
  if (tid == 0) seg_ok = 1;
  __syncthreads();
  for (int i = tid; i < t.n; i += 256) {
    const int64_t* m = matched + (t.moff + i) * 4;
    const int64_t q = m[2], g = m[3] - t.goff;
    if (m[0] < 0 || q < 0 || q >= Q || g < 0 || g >= t.G) seg_ok = 0;
    else a_q[g] = (int)q;
  }
  __syncthreads();
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  float* crow = cost + t.coff + (int64_t)r * t.Gr;
  if (!seg_ok) {
    for (int64_t k = lane; k < t.Gr; k += 64) crow[k] = 0.f;
    return;
  }
  const float* xs = sub + ((int64_t)b * R + r) * Q;
  const float* xo = obj + ((int64_t)b * R + r) * Q;
  const float* xr = rel + ((int64_t)b * R + r) * C1;
  float ms, ds, mo, dob, mr, dr;
  rel_row_stats(xs, Q, lane, ms, ds);
  rel_row_stats(xo, Q, lane, mo, dob);
  rel_row_stats(xr, C1, lane, mr, dr);
  for (int64_t k = lane; k < t.Gr; k += 64) {
    const int64_t* g = gt_rels + (t.roff + k) * 3;
    const int64_t s = g[0], o = g[1], p = g[2];
    float v = 0.f;      // (an index out of range: pn_rel_targets reports it)
    if (s >= 0 && s < t.G && o >= 0 && o < t.G && p >= 0 && p < C1) {
      const int sq = a_q[s], oq = a_q[o];
      if (sq < Q && oq < Q) {
        const float ps = expf(xs[sq] - ms) / ds, po = expf(xo[oq] - mo) / dob;
        const float pr = expf(xr[p] - mr) / dr;
        v = ((-ps) * w_s + (-po) * w_o) + (-pr) * w_r;
      }
    }
    crow[k] = v;
  }
}

extern "C" int pn_rel_id_cost_f32(const float* rel, const float* sub, const float* obj,
                                  const int64_t* gt_rels, int64_t rel_len, const int64_t* matched,
                                  int64_t Mtot, const int64_t* tab, float* cost, int64_t cost_len,
                                  int B, int R, int Q, int C1, float w_s, float w_o, float w_r,
                                  void* stream) {
  if (!rel || !sub || !obj || !gt_rels || !matched || !tab || !cost || rel_len <= 0 || Mtot <= 0 ||
      cost_len <= 0 || B <= 0 || B > 65535 || R <= 0 || R > REL_MAX_SIDE || Q <= 0 ||
      Q > REL_MAX_SIDE || C1 <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_rel_id_cost, dim3((R + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, rel,
                     sub, obj, gt_rels, rel_len, matched, Mtot, tab, cost, cost_len, R, Q, C1, w_s,
                     w_o, w_r);
  return PN_LAUNCH_CHECK();
}

// ---- the targets behind the assignment (baseline.py:866-907 with MaskPseudoSampler: positives in
// ascending row order).  One workgroup walks the B images in order.  An image with a non-zero status
// keeps its fills: r_labels 0, pos rows -1.
__global__ __launch_bounds__(256) void k_rel_targets(
    const int64_t* __restrict__ tab, const int32_t* __restrict__ row_ind,
    const int32_t* __restrict__ col_ind, int64_t out_len, const int32_t* __restrict__ lsa_status,
    const int64_t* __restrict__ gt_rels, int64_t rel_len, const int64_t* __restrict__ matched,
    int64_t Mtot, int B, int R, int Q, int C1, int64_t* __restrict__ r_labels,
    int32_t* __restrict__ pos, int32_t* __restrict__ status) {
  __shared__ int a_q[REL_MAX_SIDE];
  __shared__ int pos_of_q[REL_MAX_SIDE];
  __shared__ int bad;
  const int tid = threadIdx.x;
  int acc = 0;
  for (int b = 0; b < B; ++b) {
    const RelTab t = rel_tab(tab, b);
    for (int r = tid; r < R; r += 256) r_labels[(int64_t)b * R + r] = 0;
    if (!rel_tab_ok(t, R, Q, (int64_t)1 << 62, rel_len, Mtot, out_len)) { acc |= 8; continue; }
    const int P = (int)(t.Gr < R ? t.Gr : R);
    for (int i = tid; i < 4 * P; i += 256) pos[t.poff * 4 + i] = -1;
    if (tid == 0) bad = 0;
    for (int g = tid; g < t.G; g += 256) a_q[g] = 1;
    for (int q = tid; q < Q; q += 256) pos_of_q[q] = -1;
    __syncthreads();
    for (int i = tid; i < t.n; i += 256) {
      const int64_t* m = matched + (t.moff + i) * 4;
      const int64_t q = m[2], g = m[3] - t.goff;
      if (m[0] < 0) atomicOr(&bad, 32);
      else if (q < 0 || q >= Q || g < 0 || g >= t.G) atomicOr(&bad, 4);
      else { a_q[g] = (int)q; pos_of_q[q] = i; }
    }
    __syncthreads();
    int st = bad;
    if (st == 0) st = lsa_status[b];
    if (st == 0) {
      for (int i = tid; i < P; i += 256) {
        const int r = row_ind[t.poff + i], k = col_ind[t.poff + i];
        if (r < 0 || r >= R || k < 0 || k >= t.Gr) { atomicOr(&bad, 4); continue; }
        const int64_t* g = gt_rels + (t.roff + k) * 3;
        const int64_t s = g[0], o = g[1], p = g[2];
        if (s < 0 || s >= t.G || o < 0 || o >= t.G || p < 0 || p >= C1) { atomicOr(&bad, 4); continue; }
        // (od_pos_inds == id).nonzero() of an id that is no matched query: the reference raises
        const int sq = a_q[s], oq = a_q[o];
        if (sq >= Q || oq >= Q || pos_of_q[sq] < 0 || pos_of_q[oq] < 0) atomicOr(&bad, 16);
      }
    }
    __syncthreads();
    st |= bad;
    if (st == 0) {
      for (int i = tid; i < P; i += 256) {
        const int r = row_ind[t.poff + i], k = col_ind[t.poff + i];
        const int64_t* g = gt_rels + (t.roff + k) * 3;
        r_labels[(int64_t)b * R + r] = g[2];
        int32_t* o = pos + (t.poff + i) * 4;
        o[0] = b, o[1] = r, o[2] = pos_of_q[a_q[g[0]]], o[3] = pos_of_q[a_q[g[1]]];
      }
    }
    acc |= st;
    __syncthreads();
  }
  if (tid == 0) status[0] = acc;
}

extern "C" int pn_rel_targets(const int64_t* tab, const int32_t* row_ind, const int32_t* col_ind,
                              int64_t out_len, const int32_t* lsa_status, const int64_t* gt_rels,
                              int64_t rel_len, const int64_t* matched, int64_t Mtot, int B, int R,
                              int Q, int C1, int64_t* r_labels, int32_t* pos, int32_t* status,
                              void* stream) {
  if (!tab || !row_ind || !col_ind || !lsa_status || !gt_rels || !matched || !r_labels || !pos ||
      !status || out_len <= 0 || rel_len <= 0 || Mtot <= 0 || B <= 0 || B > 65535 || R <= 0 ||
      R > REL_MAX_SIDE || Q <= 0 || Q > REL_MAX_SIDE || C1 <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_rel_targets, dim3(1), dim3(256), 0, (hipStream_t)stream, tab, row_ind,
                     col_ind, out_len, lsa_status, gt_rels, rel_len, matched, Mtot, B, R, Q, C1,
                     r_labels, pos, status);
  return PN_LAUNCH_CHECK();
}

// ---- loss_subject_match / loss_object_match (baseline.py:655-682, 883-902): MultilabelCrossEntropy
// with a one-hot target on scores[pos_inds][:, od_pos_inds],
//   row_loss[i][t] = lse over the n matched columns of x - x[target column]
//   out[t] = (1 / B) sum_b w_t * (sum_i row_loss[i][t] / P_b)
//   grad_t[b][r][c] = w_t / (B P_b) * (softmax over the matched columns - onehot), 0 elsewhere.
// grid (ceil(R / 4), B): a wavefront owns a row of the image and writes (or zeroes) the whole row of
// both gradients, so the caller clears nothing.
__global__ __launch_bounds__(256) void k_id_ce(
    const float* __restrict__ sub, const float* __restrict__ obj,
    const int64_t* __restrict__ matched, int64_t Mtot, const int64_t* __restrict__ tab,
    const int32_t* __restrict__ pos, int64_t pos_len, int B, int R, int Q, float w_s, float w_o,
    float* __restrict__ row_loss, float* __restrict__ g_sub, float* __restrict__ g_obj) {
#pragma clang fp contract(off)
  __shared__ int colpos[REL_MAX_SIDE];   // query -> its position among the matched columns, or -1
  __shared__ int rowpos[REL_MAX_SIDE];   // relation row -> its entry of the image's pos rows, or -1
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const RelTab t = rel_tab(tab, b);
  const bool ok = rel_tab_ok(t, R, Q, (int64_t)1 << 62, (int64_t)1 << 62, Mtot, pos_len);
  const int P = ok ? (int)(t.Gr < R ? t.Gr : R) : 0;
  for (int q = tid; q < Q; q += 256) colpos[q] = -1;
  for (int r = tid; r < R; r += 256) rowpos[r] = -1;
  __syncthreads();
  if (ok) {
    for (int i = tid; i < t.n; i += 256) {
      const int64_t* m = matched + (t.moff + i) * 4;
      if (m[0] >= 0 && m[2] >= 0 && m[2] < Q) colpos[m[2]] = i;
    }
    for (int i = tid; i < P; i += 256) {
      const int32_t* p = pos + (t.poff + i) * 4;
      if (p[0] == b && p[1] >= 0 && p[1] < R && p[2] >= 0 && p[2] < t.n && p[3] >= 0 && p[3] < t.n)
        rowpos[p[1]] = i;
    }
  }
  __syncthreads();
  const int r = blockIdx.x * 4 + wave;
  if (r >= R) return;
  const int i = rowpos[r];
  for (int side = 0; side < 2; ++side) {
    const float* x = (side ? obj : sub) + ((int64_t)b * R + r) * Q;
    float* g = side ? g_obj : g_sub;
    if (g) g += ((int64_t)b * R + r) * Q;
    const int tcol = i < 0 ? -1 : pos[(t.poff + i) * 4 + 2 + side];
    const int64_t qt = i < 0 ? -1 : matched[(t.moff + tcol) * 4 + 2];
    if (qt < 0 || qt >= Q) {      // not a positive row (or a target that is no matched column)
      if (g) for (int c = lane; c < Q; c += 64) g[c] = 0.f;
      if (i >= 0 && lane == 0) row_loss[(t.poff + i) * 2 + side] = 0.f;
      continue;
    }
    float m = -INFINITY;
    for (int c = lane; c < Q; c += 64) if (colpos[c] >= 0) m = fmaxf(m, x[c]);
    m = wave_max(m);
    float d = 0.f;
    for (int c = lane; c < Q; c += 64) if (colpos[c] >= 0) d += expf(x[c] - m);
    d = wave_sum(d);
    if (lane == 0) row_loss[(t.poff + i) * 2 + side] = (logf(d) + m) - x[qt];
    if (g) {
      const float scale = (side ? w_o : w_s) / (float)((int64_t)B * P);
      for (int c = lane; c < Q; c += 64) {
        const int j = colpos[c];
        g[c] = j >= 0 ? scale * (expf(x[c] - m) / d - (j == tcol ? 1.f : 0.f)) : 0.f;
      }
    }
  }
}

// the two scalars: per image in ascending row, then the images in ascending order (thread 0 the
// subject term, thread 1 the object term); an image whose pos rows are -1 adds nothing
__global__ __launch_bounds__(64) void k_id_ce_finish(const int64_t* __restrict__ tab,
                                                     const int32_t* __restrict__ pos, int64_t pos_len,
                                                     const float* __restrict__ row_loss, int B, int R,
                                                     float w_s, float w_o, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int side = threadIdx.x;
  if (side >= 2) return;
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    const RelTab t = rel_tab(tab, b);
    if (t.Gr <= 0 || t.poff < 0) continue;
    const int P = (int)(t.Gr < R ? t.Gr : R);
    if (t.poff + P > pos_len || pos[t.poff * 4] < 0) continue;
    float s = 0.f;
    for (int i = 0; i < P; ++i) s += row_loss[(t.poff + i) * 2 + side];
    total += (side ? w_o : w_s) * (s / (float)P);
  }
  out[side] = total / (float)B;
}

extern "C" int pn_id_ce_f32(const float* sub, const float* obj, const int64_t* matched, int64_t Mtot,
                            const int64_t* tab, const int32_t* pos, int64_t pos_len, int B, int R,
                            int Q, float w_s, float w_o, float* row_loss, float* out, float* g_sub,
                            float* g_obj, void* stream) {
  if (!sub || !obj || !matched || !tab || !pos || !row_loss || !out || Mtot <= 0 || pos_len <= 0 ||
      B <= 0 || B > 65535 || R <= 0 || R > REL_MAX_SIDE || Q <= 0 || Q > REL_MAX_SIDE ||
      (g_sub == nullptr) != (g_obj == nullptr))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_id_ce, dim3((R + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, sub, obj,
                     matched, Mtot, tab, pos, pos_len, B, R, Q, w_s, w_o, row_loss, g_sub, g_obj);
  int e = PN_LAUNCH_CHECK();
  if (e) return e;
  hipLaunchKernelGGL(k_id_ce_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, tab, pos, pos_len,
                     row_loss, B, R, w_s, w_o, out);
  return PN_LAUNCH_CHECK();
}
