// Evaluator feed, part 4: the no-graph-constraint ranking of SGRecall.calculate_recall
// (pairnet/evaluation/sgg_metrics.py:254-343, `detection_method != "pan_seg"`): every
// (pair, predicate) is a candidate scored obj_score_sub * obj_score_obj * rel_score (:256-257),
// each pair keeps its `nogc_num` best predicates (:258-264), the survivors are ranked
// (`argsort_desc`) and only the best 100 are counted (:306-308, :314, :333, :339).
//
// A sibling of the radix-select kernels of ppn.hip, one workgroup per image: the products are
// formed in registers (never stored), turned into 48-bit unique keys -- (order-preserving float
// bits << 16) | (0xFFFF - flat index), flat index = r * (C1 - 1) + (c - 1) -- so "larger key" ==
// larger score, ties -> smaller (r, c); the per-row cut counts, for every candidate, the entries
// of its row that beat it ((C1 - 1)^2 compares per row); an MSB-first 8-bit radix select finds
// the key of the k-th largest survivor; the k survivors are compacted into LDS and ordered by
// rank counting.  Integer LDS atomics only, nothing on floats: the result does not depend on any
// order of execution.
//
// Ties: numpy's default sort leaves their order unspecified, so the rule above (inside a row and
// in the global ranking the smaller (r, c) wins; -0 == +0) is this library's documented choice,
// not a parity claim.  Scores are finite (NaN is not ordered by the reference either).
#include "common.h"

#define PN_NOGC_MAX_K 100
#define PN_NOGC_SEL 128

__device__ __forceinline__ unsigned long long nogc_key(float v, int idx) {
  uint32_t u = __float_as_uint(v + 0.0f);  // -0 -> +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 16) | (unsigned long long)(0xFFFF - idx);
}

// (s_sub * s_obj) * rel: two separately rounded fp32 products in this order, as numpy's
// `obj_scores[pred_rel_inds].prod(1)[:, None] * rel_scores[:, 1:]` forms them.  Plain operators
// under the pragma (the *_rn intrinsics are inline header functions that carry the header's own
// mode into the caller).
__device__ __forceinline__ float nogc_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

__device__ __forceinline__ int nogc_row(const int32_t* __restrict__ table, int r, int rows) {
  return min(max(table[r], 0), rows - 1);  // (never index past det / labels)
}

// KPT = keys per thread held in registers (n <= 1024 * KPT); key 0 = no candidate here, or cut.
template <int KPT>
__global__ __launch_bounds__(1024) void k_nogc_triplets(
    const float* __restrict__ det, int ld, const int64_t* __restrict__ labels,
    const float* __restrict__ rel, const int32_t* __restrict__ sub_row,
    const int32_t* __restrict__ obj_row, int R, int C1, int t, int k, int K,
    int32_t* __restrict__ trip, int32_t* __restrict__ srow_out, int32_t* __restrict__ orow_out,
    float* __restrict__ score_out, int32_t* __restrict__ count_out) {
  __shared__ int hist[256];
  __shared__ unsigned long long sel[PN_NOGC_SEL];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_remaining, s_count, s_done;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P1 = C1 - 1, n = R * P1;
  unsigned long long key[KPT];
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int i = tid + 1024 * j;
    key[j] = 0ull;
    if (i < n) {
      const int r = i / P1, c = i - r * P1 + 1;
      const float* x = rel + (int64_t)r * C1;
      const float pair = nogc_mul(det[(int64_t)nogc_row(sub_row, r, 2 * R) * ld + 4],
                                  det[(int64_t)nogc_row(obj_row, r, 2 * R) * ld + 4]);
      const float v = nogc_mul(pair, x[c]);
      bool keep = true;
      if (t < P1) {  // the per-row cut: fewer than t entries of the row beat this one
        int beat = 0;
        for (int c2 = 1; c2 <= P1; ++c2) {
          const float v2 = nogc_mul(pair, x[c2]);
          beat += (v2 > v || (v2 == v && c2 < c)) ? 1 : 0;
        }
        keep = beat < t;
      }
      if (keep) key[j] = nogc_key(v, i);
    }
  }
  if (tid == 0) { s_prefix = 0ull; s_remaining = k; s_count = 0; s_done = 0; }
  __syncthreads();
  for (int pass = 0; pass < 6; ++pass) {
    const int shift = 40 - 8 * pass;
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = s_prefix;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      if (key[j] != 0ull && (pass == 0 || (key[j] >> (shift + 8)) == (prefix >> (shift + 8))))
        atomicAdd(&hist[(int)((key[j] >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (wave == 0) {
      const int remaining = s_remaining;
      const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1];
      const int h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
      const int s = (h0 + h1) + (h2 + h3);
      int suf = s;  // inclusive suffix sum over lanes >= this one
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_down(suf, o, 64);
        if (lane + o < 64) suf += up;
      }
      const int above = suf - s;
      if (above < remaining && remaining <= suf) {
        int cum = above, digit, hb[4] = {h0, h1, h2, h3};
        digit = 4 * lane;
#pragma unroll
        for (int bq = 3; bq >= 0; --bq) {
          if (cum + hb[bq] >= remaining) { digit = 4 * lane + bq; break; }
          cum += hb[bq];
        }
        s_prefix = prefix | ((unsigned long long)digit << shift);
        s_remaining = remaining - cum;
        // the whole bucket of this digit is taken: every key >= the prefix (lower bits zero)
        // is selected and nothing remains to refine
        if (hb[digit & 3] == remaining - cum) s_done = 1;
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  const unsigned long long kth = s_prefix;  // (>= 2^47: a finite score's key; never 0)
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    if (key[j] != 0ull && key[j] >= kth) {
      const int slot = atomicAdd(&s_count, 1);
      if (slot < PN_NOGC_SEL) sel[slot] = key[j];
    }
  }
  __syncthreads();
  // order: the keys are unique, so the rank of a selected key = the number of selected keys
  // above it; thread i counts for key i and writes its row of the output at that rank.  The
  // score is formed again from the operands (the key has lost the sign of a zero).
  if (tid < K) {
    if (tid < k) {
      const unsigned long long mine = sel[tid];
      int rank = 0;
      for (int j = 0; j < k; ++j) rank += sel[j] > mine ? 1 : 0;
      const int idx = 0xFFFF - (int)(mine & 0xFFFFull);
      const int r = min(idx / P1, R - 1), c = min(idx - r * P1 + 1, P1);  // (never index past)
      const int a = nogc_row(sub_row, r, 2 * R), b = nogc_row(obj_row, r, 2 * R);
      trip[3 * rank + 0] = (int32_t)labels[a];
      trip[3 * rank + 1] = c;
      trip[3 * rank + 2] = (int32_t)labels[b];
      srow_out[rank] = a;
      orow_out[rank] = b;
      score_out[rank] = nogc_mul(nogc_mul(det[(int64_t)a * ld + 4], det[(int64_t)b * ld + 4]),
                                 rel[(int64_t)r * C1 + c]);
    } else {  // rows past count
      trip[3 * tid + 0] = trip[3 * tid + 1] = trip[3 * tid + 2] = -1;
      srow_out[tid] = orow_out[tid] = -1;
      score_out[tid] = 0.f;
    }
  }
  if (tid == 0) count_out[0] = k;
}

extern "C" int pn_nogc_triplets_f32(const float* det, int ld, const int64_t* labels,
                                    const float* rel_dists, const int32_t* sub_row,
                                    const int32_t* obj_row, int R, int C1, int per_row, int K,
                                    int32_t* triplets, int32_t* sub_rows, int32_t* obj_rows,
                                    float* scores, int32_t* count, void* stream) {
  if (!det || !labels || !rel_dists || !sub_row || !obj_row || !triplets || !sub_rows ||
      !obj_rows || !scores || !count || ld < 5 || R <= 0 || C1 < 2)
    return PN_BAD_ARG;
  const int64_t n = (int64_t)R * (C1 - 1);
  if (n > 65536 || K <= 0 || K > PN_NOGC_MAX_K || per_row < 1 || per_row > C1 - 1)
    return PN_BAD_ARG;
  const int64_t kept = (int64_t)R * per_row;
  const int k = (int)(kept < K ? kept : K);
#define PN_NOGC(KPT)                                                                          \
  hipLaunchKernelGGL(k_nogc_triplets<KPT>, dim3(1), dim3(1024), 0, (hipStream_t)stream, det,  \
                     ld, labels, rel_dists, sub_row, obj_row, R, C1, per_row, k, K, triplets, \
                     sub_rows, obj_rows, scores, count)
  if (n <= 1024 * 8) PN_NOGC(8);
  else if (n <= 1024 * 24) PN_NOGC(24);
  else PN_NOGC(64);
#undef PN_NOGC
  return PN_LAUNCH_CHECK();
}

// ---- the box IoU statistic --------------------------------------------------------------
// `SGObjectIOU.calculate_iou` -> `_compute_iou_bbox` (sgg_metrics.py:1025-1028, :1133-1178), the
// box form of evaluate.hip's k_eval_iou_best: one thread per (side, ground-truth OBJECT) --
// objects, not relations.  Side 0 walks the subject predictions [0, R), side 1 the object
// predictions [R, 2R).  (The reference hard-codes the split at 100; this splits at R, identical
// at the only R any config uses.)  `max(iou_row)` is Python's max over the float32 row: the
// first value, replaced by a later one only when that is greater.  IoU = box_iou_f32 of
// common.h, the function the box triplet match uses, so the bits agree with it; stored as the
// exact float64 of that float32.
__global__ __launch_bounds__(256) void k_box_iou_best(
    const float* __restrict__ pbox, int ldp, const int64_t* __restrict__ pred_labels, int R,
    const float* __restrict__ gbox, int ldg, const int32_t* __restrict__ gt_labels, int n_obj,
    uint8_t* __restrict__ valid, double* __restrict__ best_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * n_obj) return;
  const int side = e / n_obj, o = e - side * n_obj;
  const int64_t cls = gt_labels[o];
  const float* g = gbox + (int64_t)o * ldg;
  const float g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3];
  bool any = false;
  float best = 0.f;
  for (int p = side * R; p < (side + 1) * R; ++p) {
    if (pred_labels[p] != cls) continue;
    const float* b = pbox + (int64_t)p * ldp;
    const float v = box_iou_f32(g0, g1, g2, g3, b[0], b[1], b[2], b[3]);
    if (!any || v > best) best = v;
    any = true;
  }
  valid[e] = any ? 1 : 0;
  best_out[e] = (double)best;
}

extern "C" int pn_eval_iou_best_boxes(const float* pred_boxes, int ld_pred,
                                      const int64_t* pred_labels, int R, const float* gt_boxes,
                                      int ld_gt, const int32_t* gt_labels, int n_obj,
                                      uint8_t* valid, double* best, void* stream) {
  if (!pred_boxes || !pred_labels || !gt_boxes || !gt_labels || !valid || !best || R <= 0 ||
      n_obj <= 0 || ld_pred < 4 || ld_gt < 4)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_box_iou_best, dim3(pn_cdiv(2 * (int64_t)n_obj, 256)), dim3(256), 0,
                     (hipStream_t)stream, pred_boxes, ld_pred, pred_labels, R, gt_boxes, ld_gt,
                     gt_labels, n_obj, valid, best);
  return PN_LAUNCH_CHECK();
}
