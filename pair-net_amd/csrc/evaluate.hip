// Evaluator feed, part 3: what the dataset-level metrics need of one image, left on the device
// as a small integer record (pairnet/evaluation/sgg_metrics.py:95-99 recall@K, :741-766
// SGMeanRecall._collect_single, :1087-1131 _compute_iou_panseg), so that the test loop never
// waits for a match matrix on the host (pairnet_amd.evaluation.StreamingEvaluator).
#include "common.h"

#define PN_EVAL_MAX_K 8
#define PN_EVAL_MAX_REL 256

// One workgroup per mode (0: sgdet, 1: phrdet).  A ground-truth relation g is hit at k when
// the FIRST prediction that matches it has index < k (the union of pred_to_gt[:k] contains g):
// one walk down column g of the match matrix -- consecutive threads read consecutive bytes --
// then integer LDS histograms over the predicate ids, so no result depends on an order.
__global__ __launch_bounds__(256) void k_eval_record(
    const uint8_t* __restrict__ match_sgdet, const uint8_t* __restrict__ match_phrdet, int R,
    int G, const int32_t* __restrict__ gt_pred, const int32_t* __restrict__ ks, int nk,
    int num_rel, int32_t* __restrict__ hits, int32_t* __restrict__ counts) {
  __shared__ int hist[PN_EVAL_MAX_K + 1][PN_EVAL_MAX_REL];
  const int mode = blockIdx.x;
  const uint8_t* __restrict__ match = mode == 0 ? match_sgdet : match_phrdet;
  for (int i = threadIdx.x; i < (PN_EVAL_MAX_K + 1) * PN_EVAL_MAX_REL; i += 256)
    (&hist[0][0])[i] = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += 256) {
    int first = 0x7fffffff;                          // (never matched: below no k, also k > R)
    for (int p = 0; p < R; ++p)
      if (match[(int64_t)p * G + g]) { first = p; break; }
    const int n = gt_pred[g];
    const bool in_range = n >= 1 && n < num_rel;     // (the caller has checked; never index past)
    for (int j = 0; j < nk; ++j)
      if (first < ks[j]) {
        atomicAdd(&hist[j][0], 1);
        if (in_range) atomicAdd(&hist[j][n], 1);
      }
    if (mode == 0) {
      atomicAdd(&hist[PN_EVAL_MAX_K][0], 1);
      if (in_range) atomicAdd(&hist[PN_EVAL_MAX_K][n], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nk * num_rel; i += 256) {
    const int j = i / num_rel, n = i - j * num_rel;
    hits[((int64_t)mode * nk + j) * num_rel + n] = hist[j][n];
  }
  if (mode == 0)
    for (int n = threadIdx.x; n < num_rel; n += 256) counts[n] = hist[PN_EVAL_MAX_K][n];
}

extern "C" int pn_eval_record(const uint8_t* match_sgdet, const uint8_t* match_phrdet, int R,
                              int G, const int32_t* gt_predicates, const int32_t* ks, int nk,
                              int num_rel, int32_t* hits, int32_t* counts, void* stream) {
  if (!match_sgdet || !match_phrdet || !gt_predicates || !ks || !hits || !counts || R <= 0 ||
      G <= 0 || nk <= 0 || nk > PN_EVAL_MAX_K || num_rel < 2 || num_rel > PN_EVAL_MAX_REL)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_eval_record, dim3(2), dim3(256), 0, (hipStream_t)stream, match_sgdet,
                     match_phrdet, R, G, gt_predicates, ks, nk, num_rel, hits, counts);
  return PN_LAUNCH_CHECK();
}

// One thread per (side, ground-truth relation): side 0 = subject, 1 = object.  The walk over
// the P predictions in index order is the reference's loop, `best = max(v, best)` with
// Python's max: the FIRST argument is returned unless the second is greater, so a NaN v
// (0 / 0: an empty prediction on an empty ground-truth mask) replaces best, and a NaN best is
// replaced by the next v.  float64 division of the exact integer counts, as mask_iou does.
__global__ __launch_bounds__(256) void k_eval_iou_best(
    const int32_t* __restrict__ inter, const int32_t* __restrict__ area_p,
    const int32_t* __restrict__ area_g, int P, int n_obj, const int64_t* __restrict__ pred_labels,
    const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ gt_sub_row,
    const int32_t* __restrict__ gt_obj_row, int G, uint8_t* __restrict__ valid,
    double* __restrict__ best_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * G) return;
  const int side = e / G, g = e - side * G;
  const int o = side == 0 ? gt_sub_row[g] : gt_obj_row[g];
  bool any = false;
  double best = 0.0;
  if (o >= 0 && o < n_obj) {
    const int64_t cls = gt_labels[o];
    const int ag = area_g[o];
    for (int p = 0; p < P; ++p) {
      if (pred_labels[p] != cls) continue;
      any = true;
      const int it = inter[(int64_t)p * n_obj + o];
      const double v = (double)it / (double)(area_p[p] + ag - it);
      best = (best > v) ? best : v;
    }
  }
  valid[e] = any ? 1 : 0;
  best_out[e] = best;
}

extern "C" int pn_eval_iou_best(const int32_t* inter, const int32_t* area_pred,
                                const int32_t* area_gt, int P, int n_obj,
                                const int64_t* pred_labels, const int32_t* gt_labels,
                                const int32_t* gt_sub_row, const int32_t* gt_obj_row, int G,
                                uint8_t* valid, double* best, void* stream) {
  if (!inter || !area_pred || !area_gt || !pred_labels || !gt_labels || !gt_sub_row ||
      !gt_obj_row || !valid || !best || P <= 0 || n_obj <= 0 || G <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_eval_iou_best, dim3(pn_cdiv(2 * (int64_t)G, 256)), dim3(256), 0,
                     (hipStream_t)stream, inter, area_pred, area_gt, P, n_obj, pred_labels,
                     gt_labels, gt_sub_row, gt_obj_row, G, valid, best);
  return PN_LAUNCH_CHECK();
}
