// The box head's object assignment cost (pairnet_bbox_head.py:863-865: `self.bbox_assigner.assign`,
// [3P] mmdet HungarianAssigner with FocalLossCost + BBoxL1Cost(xywh) + IoUCost(giou),
// configs/deformable_detr/cross_r101_vg.py:158-163): every image's Q x G cost block in one launch,
// written where pn_lsa_f32's table (csrc/assign.hip) expects it.  pn_rel_id_cost_f32
// (csrc/rel_loss.hip) does the same for the sibling head.  The data are tiny (100 queries, a few
// dozen boxes per image): one cell per lane, every cell from its own operands alone, fp32 in the
// reference's operation order without fused multiply-adds, no reductions across lanes and no
// atomics -- two launches on the same inputs give the same bits.
//
// The per-image table `tab` [B][4] int64 (built on the host from shapes alone):
//   {offset of the image's Q x G block in `cost`, G, offset of its labels in gt_labels,
//    offset of its boxes in gt_bboxes [.][4] (in boxes)}
#include "common.h"

#define BOX_MAX_SIDE 1024     // Q and the boxes of one image (pn_lsa_f32's limit)
#define BOX_MAX_CLASSES 256

// v^gamma as torch's `pow` gives it: the square is one product
__device__ __forceinline__ float box_pow(float v, float gamma) {
  return gamma == 2.f ? v * v : powf(v, gamma);
}

// grid (ceil(max_cells / 256), B): thread -> cell (q, g) = (cell / G, cell % G) of image b.
// An image whose table row points outside a buffer is left untouched (pn_lsa_f32 then solves
// whatever the block held; the host builds the table from the same shapes it allocates by).  A label
// outside [0, nc) gives a NaN cell, which pn_lsa_f32 reports as status 1.
__global__ __launch_bounds__(256) void k_box_match_cost(
    const float* __restrict__ cls, const float* __restrict__ box,
    const int64_t* __restrict__ gt_labels, int64_t labels_len, const float* __restrict__ gt_bboxes,
    int64_t boxes_len, const float* __restrict__ factor, const int64_t* __restrict__ tab,
    float* __restrict__ cost, int64_t cost_len, int Q, int nc, float w_cls, float w_reg,
    float w_iou, float alpha, float gamma, float eps, float iou_eps) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const int64_t* t = tab + (int64_t)b * 4;
  const int64_t coff = t[0], G = t[1], loff = t[2], boff = t[3];
  if (G <= 0 || G > BOX_MAX_SIDE || coff < 0 || loff < 0 || boff < 0 ||
      coff + (int64_t)Q * G > cost_len || loff + G > labels_len || boff + G > boxes_len)
    return;                                                     // (uniform)
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)Q * G) return;
  const int q = (int)(cell / G), g = (int)(cell - (int64_t)q * G);
  const int64_t label = gt_labels[loff + g];
  const float* gb = gt_bboxes + (boff + g) * 4;
  const float* pb = box + ((int64_t)b * Q + q) * 4;
  const float* f = factor + (int64_t)b * 4;
  float* out = cost + coff + cell;
  if (label < 0 || label >= nc) {
    *out = NAN;
    return;
  }
  // FocalLossCost: pos_cost[:, gt] - neg_cost[:, gt] on sigmoid(cls_pred)
  const float x = cls[((int64_t)b * Q + q) * nc + label];
  const float p = 1.f / (1.f + expf(-x));
  const float neg = ((-logf((1.f - p) + eps)) * (1.f - alpha)) * box_pow(p, gamma);
  const float pos = ((-logf(p + eps)) * alpha) * box_pow(1.f - p, gamma);
  const float cls_cost = (pos - neg) * w_cls;
  // BBoxL1Cost(xywh): cdist(p = 1) of the predicted cxcywh and cxcywh(gt / factor)
  const float gx1 = gb[0], gy1 = gb[1], gx2 = gb[2], gy2 = gb[3];
  const float nx1 = gx1 / f[0], ny1 = gy1 / f[1], nx2 = gx2 / f[2], ny2 = gy2 / f[3];
  const float cx = pb[0], cy = pb[1], bw = pb[2], bh = pb[3];
  const float d0 = fabsf(cx - (nx1 + nx2) / 2.f), d1 = fabsf(cy - (ny1 + ny2) / 2.f);
  const float d2 = fabsf(bw - (nx2 - nx1)), d3 = fabsf(bh - (ny2 - ny1));
  const float reg_cost = (((d0 + d1) + d2) + d3) * w_reg;
  // IoUCost(giou): bbox_overlaps of xyxy(pred) * factor and the ground truth in pixels
  const float px1 = (cx - 0.5f * bw) * f[0], py1 = (cy - 0.5f * bh) * f[1];
  const float px2 = (cx + 0.5f * bw) * f[2], py2 = (cy + 0.5f * bh) * f[3];
  const float area1 = (px2 - px1) * (py2 - py1), area2 = (gx2 - gx1) * (gy2 - gy1);
  const float iw = fmaxf(fminf(px2, gx2) - fmaxf(px1, gx1), 0.f);
  const float ih = fmaxf(fminf(py2, gy2) - fmaxf(py1, gy1), 0.f);
  const float overlap = iw * ih;
  const float uni = fmaxf((area1 + area2) - overlap, iou_eps);
  const float ew = fmaxf(fmaxf(px2, gx2) - fminf(px1, gx1), 0.f);
  const float eh = fmaxf(fmaxf(py2, gy2) - fminf(py1, gy1), 0.f);
  const float enclose = fmaxf(ew * eh, iou_eps);
  const float giou = overlap / uni - (enclose - uni) / enclose;
  const float iou_cost = (-giou) * w_iou;
  *out = (cls_cost + reg_cost) + iou_cost;
}

extern "C" int pn_box_match_cost_f32(const float* cls, const float* box, const int64_t* gt_labels,
                                     int64_t labels_len, const float* gt_bboxes, int64_t boxes_len,
                                     const float* factor, const int64_t* tab, float* cost,
                                     int64_t cost_len, int64_t max_cells, int B, int Q, int nc,
                                     float w_cls, float w_reg, float w_iou, float alpha, float gamma,
                                     float eps, float iou_eps, void* stream) {
  if (!cls || !box || !gt_labels || !gt_bboxes || !factor || !tab || !cost || labels_len <= 0 ||
      boxes_len <= 0 || cost_len <= 0 || max_cells <= 0 ||
      max_cells > (int64_t)BOX_MAX_SIDE * BOX_MAX_SIDE || B <= 0 || B > 65535 || Q < 2 ||
      Q > BOX_MAX_SIDE || nc <= 0 || nc > BOX_MAX_CLASSES)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_box_match_cost, dim3(pn_cdiv(max_cells, 256), B), dim3(256), 0,
                     (hipStream_t)stream, cls, box, gt_labels, labels_len, gt_bboxes, boxes_len,
                     factor, tab, cost, cost_len, Q, nc, w_cls, w_reg, w_iou, alpha, gamma, eps,
                     iou_eps);
  return PN_LAUNCH_CHECK();
}
