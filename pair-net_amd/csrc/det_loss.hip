// The plain Deformable-DETR detector's loss and box results (configs/deformable_detr/od_r101_vg.py:
// 3-96; [3P] mmdet `DETRHead.loss_single` / `_get_bboxes_single`, whose in-tree statement is the
// commented text at pairnet_bbox_head.py:596-642): the Hungarian match cost of all (L + 1) * B
// problems in one launch, the focal term of every decoder layer and of the per-token proposals in
// one streaming launch, the L1 / GIoU terms over the matched pairs, and the ranked detections.
// Composed in det_losses.py / det_head.py.  fp32 in mmdet's operation order, no fused multiply-adds
// where values are compared with mmdet's; reductions in fixed orders (per-workgroup partials, then
// one workgroup per term), no float atomics: two launches on the same inputs give the same bits.
#include "common.h"

#define DET_MAX_ROWS 65536      // rows of one match problem (the trunk's token limit)
#define DET_MAX_G 1024          // ground-truth boxes of one image
#define DET_MAX_CLASSES 256
#define DET_MAX_TERMS 16
#define DET_FOCAL_V4 4          // float4 per lane of k_det_focal
#define DET_FOCAL_WG_ELEMS (256 * 4 * DET_FOCAL_V4)

__device__ __forceinline__ float det_pow(float v, float gamma) {
  return gamma == 2.f ? v * v : powf(v, gamma);
}

// ---------------------------------------------------------------------------- match cost
// pn_box_match_cost_f32's cell (csrc/box_loss.hip), statement for statement, for P problems with
// their own row counts.  tab [P][6] int64 = {offset of the rows x G block in `cost`, rows, G, offset
// of the labels, offset of the boxes (in boxes), offset of the problem's first row in cls / box};
// factor [P][4].  grid (ceil(max_cells / 256), P): thread -> cell (q, g) = (cell / G, cell % G).
__global__ __launch_bounds__(256) void k_det_match_cost(
    const float* __restrict__ cls, const float* __restrict__ box, int64_t rows_len,
    const int64_t* __restrict__ gt_labels, int64_t labels_len, const float* __restrict__ gt_bboxes,
    int64_t boxes_len, const float* __restrict__ factor, const int64_t* __restrict__ tab,
    float* __restrict__ cost, int64_t cost_len, int nc, float w_cls, float w_reg, float w_iou,
    float alpha, float gamma, float eps, float iou_eps) {
#pragma clang fp contract(off)
  const int p = blockIdx.y;
  const int64_t* t = tab + (int64_t)p * 6;
  const int64_t coff = t[0], Q = t[1], G = t[2], loff = t[3], boff = t[4], roff = t[5];
  if (Q <= 0 || Q > DET_MAX_ROWS || G <= 0 || G > DET_MAX_G || coff < 0 || loff < 0 || boff < 0 ||
      roff < 0 || coff + Q * G > cost_len || loff + G > labels_len || boff + G > boxes_len ||
      roff + Q > rows_len)
    return;                                                     // (uniform)
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= Q * G) return;
  const int64_t q = cell / G;
  const int g = (int)(cell - q * G);
  const int64_t label = gt_labels[loff + g];
  const float* gb = gt_bboxes + (boff + g) * 4;
  const float* pb = box + (roff + q) * 4;
  const float* f = factor + (int64_t)p * 4;
  float* out = cost + coff + cell;
  if (label < 0 || label >= nc) {
    *out = NAN;
    return;
  }
  // FocalLossCost: pos_cost[:, gt] - neg_cost[:, gt] on sigmoid(cls_pred)
  const float x = cls[(roff + q) * nc + label];
  const float pr = 1.f / (1.f + expf(-x));
  const float neg = ((-logf((1.f - pr) + eps)) * (1.f - alpha)) * det_pow(pr, gamma);
  const float pos = ((-logf(pr + eps)) * alpha) * det_pow(1.f - pr, gamma);
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

extern "C" int pn_det_match_cost_f32(const float* cls, const float* box, int64_t rows_len,
                                     const int64_t* gt_labels, int64_t labels_len,
                                     const float* gt_bboxes, int64_t boxes_len, const float* factor,
                                     const int64_t* tab, float* cost, int64_t cost_len,
                                     int64_t max_cells, int P, int nc, float w_cls, float w_reg,
                                     float w_iou, float alpha, float gamma, float eps,
                                     float iou_eps, void* stream) {
  if (!cls || !box || !gt_labels || !gt_bboxes || !factor || !tab || !cost || rows_len <= 0 ||
      rows_len * (int64_t)(nc > 4 ? nc : 4) >= ((int64_t)1 << 40) || labels_len <= 0 ||
      boxes_len <= 0 || cost_len <= 0 || max_cells <= 0 ||
      max_cells > (int64_t)DET_MAX_ROWS * DET_MAX_G || P <= 0 || P > 65535 || nc <= 0 ||
      nc > DET_MAX_CLASSES)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_det_match_cost, dim3(pn_cdiv(max_cells, 256), P), dim3(256), 0,
                     (hipStream_t)stream, cls, box, rows_len, gt_labels, labels_len, gt_bboxes,
                     boxes_len, factor, tab, cost, cost_len, nc, w_cls, w_reg, w_iou, alpha, gamma,
                     eps, iou_eps);
  return PN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------- focal term
// One element of mmdet's `py_sigmoid_focal_loss` and its derivative.  With z = x for a negative
// and z = -x for the positive (the column that equals the row's label), q = sigmoid(z) is the
// probability of the wrong answer (mmdet's `pt`) and softplus(z) its BCE-with-logits in the stable
// form; both come from ONE e = exp(-|z|), so no 1 - p is formed:
//   loss = a softplus(z) q^gamma,  a = alpha (positive) / 1 - alpha (negative)
//   d loss / d x = +-a q^gamma (q + gamma softplus(z) (1 - q))       (+ negative, - positive)
struct DetFocal { float loss, grad; };
__device__ __forceinline__ DetFocal det_focal_elem(float x, bool positive, float alpha,
                                                   float gamma) {
  const float z = positive ? -x : x;
  const float e = expf(-fabsf(z));
  const float den = 1.f + e;
  const float q = (z >= 0.f ? 1.f : e) / den;
  const float omq = (z >= 0.f ? e : 1.f) / den;                // 1 - q without the subtraction
  const float bce = fmaxf(z, 0.f) + log1pf(e);
  const float a = positive ? alpha : 1.f - alpha;
  const float aq = a * det_pow(q, gamma);
  DetFocal r;
  r.loss = bce * aq;
  const float d = aq * (q + (gamma * bce) * omq);
  r.grad = positive ? -d : d;
  return r;
}

// x / grad [rows][C] contiguous, 16-byte aligned: the block is walked as rows * C / 4 float4 (an
// element's row is its flat index / C, so C need not be a multiple of 4) and the last
// (rows * C) % 4 elements one by one.  labels [rows] int32 (C = background; outside [0, C]: the
// row's loss and gradient are NaN), term [rows] int32 in [0, T) (outside: the row counts for no
// term and its gradient is 0).  Workgroup w owns the elements [w, w + 1) * DET_FOCAL_WG_ELEMS and
// writes partial[w][0 .. T): every lane adds its elements in index order into its own LDS slot of
// the element's term, then per term the 256 slots are summed by a fixed butterfly.
__global__ __launch_bounds__(256) void k_det_focal(
    const float* __restrict__ x, const int32_t* __restrict__ labels,
    const int32_t* __restrict__ term, const float* __restrict__ avg, float* __restrict__ grad,
    float* __restrict__ partial, uint32_t total, uint32_t C, int T, float w_cls, float alpha,
    float gamma) {
  __shared__ float s_acc[DET_MAX_TERMS * 256];
  __shared__ float s_wave[DET_MAX_TERMS * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < T * 256; i += 256) s_acc[i] = 0.f;
  // (own slots only: no barrier needed before the lane's own read-modify-writes below, but the
  // zero fill above strides across lanes)
  __syncthreads();
  const uint32_t wg_base = blockIdx.x * (uint32_t)DET_FOCAL_WG_ELEMS;
  const uint32_t n4 = total & ~3u;
  int cur = -1;
  float acc = 0.f, scale = 0.f;
#pragma unroll
  for (int v = 0; v < DET_FOCAL_V4; ++v) {
    const uint32_t e0 = wg_base + ((uint32_t)v * 256u + (uint32_t)tid) * 4u;
    if (e0 >= total) break;
    const bool vec = e0 < n4;
    const int cnt = vec ? 4 : (int)(total - e0);
    float in[4] = {0.f, 0.f, 0.f, 0.f}, out[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      const float4 t4 = ld4(x + e0);
      in[0] = t4.x, in[1] = t4.y, in[2] = t4.z, in[3] = t4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < cnt) in[j] = x[e0 + j];
    }
    uint32_t row = e0 / C, col = e0 - row * C;
    int lab = labels[row], tm = term[row];
    if (tm < 0 || tm >= T) tm = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < cnt) {
        if (tm != cur) {                       // a new term: bank what the old one collected
          if (cur >= 0) s_acc[cur * 256 + tid] += acc;
          cur = tm;
          acc = 0.f;
          scale = cur >= 0 ? w_cls / avg[cur] : 0.f;
        }
        DetFocal r = det_focal_elem(in[j], (int)col == lab, alpha, gamma);
        if (lab < 0 || lab > (int)C) r.loss = r.grad = NAN;
        if (cur >= 0) acc += r.loss;
        out[j] = cur >= 0 ? scale * r.grad : 0.f;
        if (++col == C && j + 1 < cnt) {
          col = 0;
          ++row;
          lab = labels[row], tm = term[row];
          if (tm < 0 || tm >= T) tm = -1;
        }
      }
    }
    if (vec) {
      st4(grad + e0, make_float4(out[0], out[1], out[2], out[3]));
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (j < cnt) grad[e0 + j] = out[j];
    }
  }
  if (cur >= 0) s_acc[cur * 256 + tid] += acc;
  __syncthreads();
  for (int t = 0; t < T; ++t) {
    const float s = wave_sum(s_acc[t * 256 + tid]);
    if (lane == 0) s_wave[t * 4 + wave] = s;
  }
  __syncthreads();
  if (tid < T)
    partial[(int64_t)blockIdx.x * T + tid] =
        ((s_wave[tid * 4] + s_wave[tid * 4 + 1]) + s_wave[tid * 4 + 2]) + s_wave[tid * 4 + 3];
}

// grid T: out[t] = w_cls * (sum_w partial[w][t] / avg[t]); lane i adds workgroups i, i + 256, ...
// in order, then the same butterfly.
__global__ __launch_bounds__(256) void k_det_focal_final(const float* __restrict__ partial,
                                                         const float* __restrict__ avg,
                                                         float* __restrict__ out, int nwg, int T,
                                                         float w_cls) {
#pragma clang fp contract(off)
  __shared__ float s_wave[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  float acc = 0.f;
  for (int w = tid; w < nwg; w += 256) acc += partial[(int64_t)w * T + t];
  acc = wave_sum(acc);
  if ((tid & 63) == 0) s_wave[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    out[t] = w_cls * ((((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3]) / avg[t]);
}

extern "C" int64_t pn_det_focal_partials(int64_t rows, int C, int T) {
  if (rows <= 0 || C <= 0 || C > DET_MAX_CLASSES || T <= 0 || T > DET_MAX_TERMS ||
      rows * C >= ((int64_t)1 << 31))
    return 0;
  return (int64_t)pn_cdiv(rows * C, DET_FOCAL_WG_ELEMS) * T;
}

extern "C" int pn_det_focal_f32(const float* x, const int32_t* labels, const int32_t* term,
                                const float* avg, float* grad, float* partial,
                                int64_t partial_len, float* out, int64_t rows, int C, int T,
                                float w_cls, float alpha, float gamma, void* stream) {
  const int64_t need = pn_det_focal_partials(rows, C, T);
  if (!x || !labels || !term || !avg || !grad || !partial || !out || need == 0 ||
      partial_len < need || ((uintptr_t)x & 15) || ((uintptr_t)grad & 15))
    return PN_BAD_ARG;
  const int nwg = (int)(need / T);
  hipLaunchKernelGGL(k_det_focal, dim3(nwg), dim3(256), 0, (hipStream_t)stream, x, labels, term,
                     avg, grad, partial, (uint32_t)(rows * C), (uint32_t)C, T, w_cls, alpha, gamma);
  hipLaunchKernelGGL(k_det_focal_final, dim3(T), dim3(256), 0, (hipStream_t)stream, partial, avg,
                     out, nwg, T, w_cls);
  return PN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------- L1 / GIoU terms
// pairs [M][4] int32 = {row of the prediction in box / grad, ground-truth box, row of `factor`,
// term}, grouped by term: term t owns pairs [term_off[t], term_off[t + 1]).  grid T, one workgroup
// per term: lane i takes the term's pairs i, i + 256, ... in order.  out[t][0] = w_bbox sum|d| /
// avg[t], out[t][1] = w_iou sum(1 - GIoU) / avg[t]; the gradients w.r.t. the predicted cxcywh go
// to grad[row] (each matched row belongs to one pair: plain stores into the zeroed buffer).  A pair
// whose indices leave their buffers poisons the term's sums with NaN and writes nothing.
__global__ __launch_bounds__(256) void k_det_box_loss(
    const float* __restrict__ box, int64_t rows_len, const float* __restrict__ gt_bboxes,
    int64_t boxes_len, const float* __restrict__ factor, int64_t factor_len,
    const int32_t* __restrict__ pairs, const int32_t* __restrict__ term_off, int64_t M,
    const float* __restrict__ avg, float* __restrict__ grad, float* __restrict__ out, float w_bbox,
    float w_iou, float iou_eps) {
#pragma clang fp contract(off)
  __shared__ float s_wave[2][4];
  const int t = blockIdx.x, tid = threadIdx.x;
  int lo = term_off[t], hi = term_off[t + 1];
  const bool bad_range = lo < 0 || hi < lo || hi > M;
  if (bad_range) lo = hi = 0;
  const float a = avg[t];
  const float sb = w_bbox / a, si = w_iou / a;
  float l1 = 0.f, gl = 0.f;
  for (int i = lo + tid; i < hi; i += 256) {
    const int32_t* pr = pairs + (int64_t)i * 4;
    const int r = pr[0], g = pr[1], fi = pr[2];
    if (r < 0 || r >= rows_len || g < 0 || g >= boxes_len || fi < 0 || fi >= factor_len) {
      l1 = gl = NAN;
      continue;
    }
    const float* pb = box + (int64_t)r * 4;
    const float* gb = gt_bboxes + (int64_t)g * 4;
    const float* f = factor + (int64_t)fi * 4;
    const float f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    const float cx = pb[0], cy = pb[1], bw = pb[2], bh = pb[3];
    // bbox_targets = bbox_xyxy_to_cxcywh(gt / factor)
    const float nx1 = gb[0] / f0, ny1 = gb[1] / f1, nx2 = gb[2] / f2, ny2 = gb[3] / f3;
    const float tcx = (nx1 + nx2) / 2.f, tcy = (ny1 + ny2) / 2.f, tw = nx2 - nx1, th = ny2 - ny1;
    const float e0 = cx - tcx, e1 = cy - tcy, e2 = bw - tw, e3 = bh - th;
    l1 += ((fabsf(e0) + fabsf(e1)) + fabsf(e2)) + fabsf(e3);
    // bboxes = bbox_cxcywh_to_xyxy(.) * factor on both sides
    const float px1 = (cx - 0.5f * bw) * f0, py1 = (cy - 0.5f * bh) * f1;
    const float px2 = (cx + 0.5f * bw) * f2, py2 = (cy + 0.5f * bh) * f3;
    const float gx1 = (tcx - 0.5f * tw) * f0, gy1 = (tcy - 0.5f * th) * f1;
    const float gx2 = (tcx + 0.5f * tw) * f2, gy2 = (tcy + 0.5f * th) * f3;
    const float pw = px2 - px1, ph = py2 - py1;
    const float area1 = pw * ph, area2 = (gx2 - gx1) * (gy2 - gy1);
    const float iwr = fminf(px2, gx2) - fmaxf(px1, gx1), ihr = fminf(py2, gy2) - fmaxf(py1, gy1);
    const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
    const float overlap = iw * ih;
    const float unr = (area1 + area2) - overlap;
    const float uni = fmaxf(unr, iou_eps);
    const float ewr = fmaxf(px2, gx2) - fminf(px1, gx1), ehr = fmaxf(py2, gy2) - fminf(py1, gy1);
    const float ew = fmaxf(ewr, 0.f), eh = fmaxf(ehr, 0.f);
    const float enr = ew * eh;
    const float enclose = fmaxf(enr, iou_eps);
    const float giou = overlap / uni - (enclose - uni) / enclose;
    gl += 1.f - giou;
    // d giou = d(ov / un) + d(un / en):  autograd's rules for min / max / clamp
    const float g_ov = 1.f / uni;                                        // d giou / d overlap
    const float g_un = (unr > iou_eps ? 1.f : 0.f) *
                       (1.f / enclose - overlap / (uni * uni));          // d giou / d union
    const float g_en = (enr > iou_eps ? 1.f : 0.f) * (-uni / (enclose * enclose));
    const float g_ovt = g_ov - g_un;                 // union = area1 + area2 - overlap
    const float g_iw = (iwr >= 0.f ? 1.f : 0.f) * (g_ovt * ih);
    const float g_ih = (ihr >= 0.f ? 1.f : 0.f) * (g_ovt * iw);
    const float g_ew = (ewr >= 0.f ? 1.f : 0.f) * (g_en * eh);
    const float g_eh = (ehr >= 0.f ? 1.f : 0.f) * (g_en * ew);
    // per corner: area1, the intersection side where the prediction's corner is the inner one,
    // the enclosing side where it is the outer one
    const float dx2 = g_un * ph + (px2 < gx2 ? g_iw : 0.f) + (px2 > gx2 ? g_ew : 0.f);
    const float dx1 = -(g_un * ph) - (px1 > gx1 ? g_iw : 0.f) - (px1 < gx1 ? g_ew : 0.f);
    const float dy2 = g_un * pw + (py2 < gy2 ? g_ih : 0.f) + (py2 > gy2 ? g_eh : 0.f);
    const float dy1 = -(g_un * pw) - (py1 > gy1 ? g_ih : 0.f) - (py1 < gy1 ? g_eh : 0.f);
    const float a1 = dx1 * f0, a2 = dx2 * f2, b1 = dy1 * f1, b2 = dy2 * f3;
    float* go = grad + (int64_t)r * 4;
    go[0] = sb * (e0 > 0.f ? 1.f : (e0 < 0.f ? -1.f : 0.f)) - si * (a1 + a2);
    go[1] = sb * (e1 > 0.f ? 1.f : (e1 < 0.f ? -1.f : 0.f)) - si * (b1 + b2);
    go[2] = sb * (e2 > 0.f ? 1.f : (e2 < 0.f ? -1.f : 0.f)) - si * (0.5f * (a2 - a1));
    go[3] = sb * (e3 > 0.f ? 1.f : (e3 < 0.f ? -1.f : 0.f)) - si * (0.5f * (b2 - b1));
  }
  if (bad_range) l1 = gl = NAN;
  l1 = wave_sum(l1);
  gl = wave_sum(gl);
  if ((tid & 63) == 0) s_wave[0][tid >> 6] = l1, s_wave[1][tid >> 6] = gl;
  __syncthreads();
  if (tid < 2) {
    const float s = ((s_wave[tid][0] + s_wave[tid][1]) + s_wave[tid][2]) + s_wave[tid][3];
    out[t * 2 + tid] = (tid == 0 ? w_bbox : w_iou) * (s / a);
  }
}

extern "C" int pn_det_box_loss_f32(const float* box, int64_t rows_len, const float* gt_bboxes,
                                   int64_t boxes_len, const float* factor, int64_t factor_len,
                                   const int32_t* pairs, const int32_t* term_off, int64_t M, int T,
                                   const float* avg, float* grad, float* out, float w_bbox,
                                   float w_iou, float iou_eps, void* stream) {
  // (M == 0 is legal: no image of the batch has ground truth; `pairs` / `gt_bboxes` may then be
  // NULL and every term is 0)
  if (!box || !factor || !term_off || !avg || !grad || !out || rows_len <= 0 ||
      rows_len >= ((int64_t)1 << 31) || factor_len <= 0 || M < 0 || M >= ((int64_t)1 << 29) ||
      T <= 0 || T > DET_MAX_TERMS || (M > 0 && (!pairs || !gt_bboxes || boxes_len <= 0)) ||
      boxes_len < 0 || boxes_len >= ((int64_t)1 << 31) || factor_len >= ((int64_t)1 << 31))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_det_box_loss, dim3(T), dim3(256), 0, (hipStream_t)stream, box, rows_len,
                     gt_bboxes, boxes_len, factor, factor_len, pairs, term_off, M, avg, grad, out,
                     w_bbox, w_iou, iou_eps);
  return PN_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------- box results
// mmdet `DETRHead._get_bboxes_single` behind the ranking: idx [B][K] are flat indices into the
// image's Q * C logits, best first.  meta [B][6] = {img_h, img_w, scale_factor[0..3]}.
//   label = idx % C, query = idx / C, score = sigmoid(logit)
//   box   = clamp(cxcywh_to_xyxy(bbox_pred[query]) * (w, h, w, h), 0, (w, h, w, h)) [/ scale_factor]
// det [B][K][5] = (x1, y1, x2, y2, score), labels [B][K] int64; an index outside [0, Q * C) gives
// a NaN row and label -1.  One lane per (b, k); every output element is written.
__global__ __launch_bounds__(256) void k_det_results(
    const float* __restrict__ cls, const float* __restrict__ box, const int64_t* __restrict__ idx,
    const float* __restrict__ meta, float* __restrict__ det, int64_t* __restrict__ labels, int B,
    int Q, int C, int K, int rescale) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * K) return;
  const int b = i / K;
  const int64_t id = idx[i];
  float* d = det + (int64_t)i * 5;
  if (id < 0 || id >= (int64_t)Q * C) {
    d[0] = d[1] = d[2] = d[3] = d[4] = NAN;
    labels[i] = -1;
    return;
  }
  const int q = (int)(id / C);
  labels[i] = id - (int64_t)q * C;
  const float* m = meta + (int64_t)b * 6;
  const float h = m[0], w = m[1];
  const float* pb = box + ((int64_t)b * Q + q) * 4;
  const float cx = pb[0], cy = pb[1], bw = pb[2], bh = pb[3];
  float x1 = (cx - 0.5f * bw) * w, y1 = (cy - 0.5f * bh) * h;
  float x2 = (cx + 0.5f * bw) * w, y2 = (cy + 0.5f * bh) * h;
  x1 = fminf(fmaxf(x1, 0.f), w), x2 = fminf(fmaxf(x2, 0.f), w);
  y1 = fminf(fmaxf(y1, 0.f), h), y2 = fminf(fmaxf(y2, 0.f), h);
  if (rescale) x1 = x1 / m[2], y1 = y1 / m[3], x2 = x2 / m[4], y2 = y2 / m[5];
  d[0] = x1, d[1] = y1, d[2] = x2, d[3] = y2;
  d[4] = 1.f / (1.f + expf(-cls[(int64_t)b * Q * C + id]));
}

extern "C" int pn_det_results_f32(const float* cls, const float* box, const int64_t* idx,
                                  const float* meta, float* det, int64_t* labels, int B, int Q,
                                  int C, int K, int rescale, void* stream) {
  if (!cls || !box || !idx || !meta || !det || !labels || B <= 0 || Q <= 0 || C <= 0 || K <= 0 ||
      C > DET_MAX_CLASSES || (int64_t)Q * C > 65536 || K > (int64_t)Q * C ||
      (int64_t)B * K >= ((int64_t)1 << 24) || (int64_t)B * Q * C >= ((int64_t)1 << 31))
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_det_results, dim3(pn_cdiv((int64_t)B * K, 256)), dim3(256), 0,
                     (hipStream_t)stream, cls, box, idx, meta, det, labels, B, Q, C, K, rescale);
  return PN_LAUNCH_CHECK();
}
