// The triplet matching of PSGTrHead2's loss on device outputs: MaskHTriMatcher's cost for every
// image of the batch and the bookkeeping behind the assignment -- what the reference computes with
// torch ops + scipy per image in relation_heads/psgtr_head2.py:879-1018 (`_get_target_single`) and
// approaches/matcher.py:29-102 (`MaskHTriMatcher.assign`).  The assignment itself is pn_lsa_f32
// (csrc/assign.hip); the loss terms behind it reuse csrc/seg_loss.hip as it is.
//
// The mask and dice terms of a (query, relation) cell depend only on (query, subject object) and
// (query, object object), and relations reuse objects freely, so the mask work is done once per
// (side, query, OBJECT) and gathered per relation: five launches per call, whatever B, sum R_b or
// sum G_b are.  fp32 in the reference's formulas, fixed-order reductions, no floating-point atomics:
// two calls on the same inputs give the same bits.
#include "common.h"

#define TRI_TQ 4          // query maps per workgroup of k_tri_pair
#define TRI_TG 16         // objects per register group of k_tri_pair
#define TRI_MAX_SPLITS 16 // point splits of k_tri_pair

// table row of image b (int64 [B][8]): see include/pairnet_hip.h
struct TriRow { int64_t coff, R, roff, goff, G, ooff; };
__device__ __forceinline__ TriRow tri_row(const int64_t* __restrict__ tab, int b) {
  const int64_t* t = tab + (int64_t)b * 8;
  TriRow r;
  r.coff = t[0], r.R = t[1], r.roff = t[2], r.goff = t[3], r.G = t[4], r.ooff = t[5];
  return r;
}

__device__ __forceinline__ float tri_block_sum(float v, float* red) {   // 256 threads
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];      // every thread, wave order: deterministic
}

// ---- mmcv point_sample's arithmetic, word for word as seg_taps / seg_sample state it
// (csrc/seg_loss.hip): F.grid_sample(input, 2 p - 1, bilinear, zeros padding, align_corners=False).
// The four taps of a point are computed once and serve every map sampled at it.
struct TriTaps { int o[4]; float wt[4]; };          // offset into the map (-1: outside), weight
__device__ __forceinline__ TriTaps tri_taps(float px, float py, int h, int w) {
  const float cx = 2.f * px - 1.f, cy = 2.f * py - 1.f;
  const float ix = ((cx + 1.f) * (float)w - 1.f) / 2.f, iy = ((cy + 1.f) * (float)h - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)w), y0 = (int)fminf(fmaxf(fy, -2.f), (float)h);
  const float x1f = fx + 1.f, y1f = fy + 1.f;
  TriTaps t;
  t.wt[0] = (x1f - ix) * (y1f - iy), t.wt[1] = (ix - fx) * (y1f - iy);
  t.wt[2] = (x1f - ix) * (iy - fy), t.wt[3] = (ix - fx) * (iy - fy);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + (k & 1), y = y0 + (k >> 1);
    t.o[k] = (x >= 0 && x < w && y >= 0 && y < h) ? y * w + x : -1;
  }
  return t;
}
template <typename T>
__device__ __forceinline__ float tri_sample(const T* __restrict__ m, const TriTaps& t) {
  float v = 0.f;       // accumulated in ATen's order: nw, ne, sw, se
#pragma unroll
  for (int k = 0; k < 4; ++k) v += (t.o[k] >= 0 ? (float)m[t.o[k]] : 0.f) * t.wt[k];
  return v;
}

// ---- (a) ground-truth samples: t[g][i] = object g's mask at its image's point i, and sum_i t[g][i].
// One workgroup per (object of the image, image); the masks are uint8 0/1 on their own grid.
__global__ __launch_bounds__(256) void k_tri_gt_samples(
    const uint8_t* __restrict__ gt, int hg, int wg, const float* __restrict__ pts,
    const int64_t* __restrict__ tab, int64_t SG, int Np, float* __restrict__ t,
    float* __restrict__ tsum) {
  __shared__ float red[4];
  const int b = blockIdx.y;
  const TriRow r = tri_row(tab, b);
  if (r.goff < 0 || r.G < 0 || r.goff + r.G > SG || (int64_t)blockIdx.x >= r.G) return;   // (uniform)
  const int64_t g = r.goff + blockIdx.x;
  const uint8_t* m = gt + g * (int64_t)hg * wg;
  const float2* p2 = reinterpret_cast<const float2*>(pts) + (int64_t)b * Np;
  float s = 0.f;
  for (int i = threadIdx.x; i < Np; i += 256) {
    const float2 p = p2[i];
    const float v = tri_sample(m, tri_taps(p.x, p.y, hg, wg));
    t[g * Np + i] = v;
    s += v;
  }
  s = tri_block_sum(s, red);
  if (threadIdx.x == 0) tsum[g] = s;
}

// ---- row statistics of the three logit blocks, once per query: stats[k][row] = (max, sum exp(x - max)),
// k = 0 sub, 1 obj, 2 rel; one wave per (block, row).
__global__ __launch_bounds__(192) void k_tri_row_stats(const float* __restrict__ sub,
                                                       const float* __restrict__ obj,
                                                       const float* __restrict__ rel, int rows, int C1,
                                                       int Cr1, float2* __restrict__ stats) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6, row = blockIdx.x;
  const int n = k == 2 ? Cr1 : C1;
  const float* x = (k == 0 ? sub : k == 1 ? obj : rel) + (int64_t)row * n;
  float m = -INFINITY;
  for (int c = lane; c < n; c += 64) m = fmaxf(m, x[c]);
  m = wave_max(m);
  float d = 0.f;
  for (int c = lane; c < n; c += 64) d += expf(x[c] - m);
  d = wave_sum(d);
  if (lane == 0) stats[(int64_t)k * rows + row] = make_float2(m, d);
}

// ---- (b) pair sums: for side s (0 subject masks, 1 object masks), query q and object g of image b
//   sum_p x t, sum_p s t (per pair) and sum_p BCE(x, 0), sum_p s (per query),  s = sigmoid(x),
// with x = the query's mask logits sampled at the image's points.  Grid (ceil(Q / 4), 2 B, splits),
// 256 threads: workgroup z owns a contiguous run of the 256-point chunks, a thread the points
// chunk * 256 + tid of that run; the taps of a point are computed once for the tile's 4 maps, the
// predictions are sampled on the fly (x [Q][Np] never goes to memory); the image's objects pass in
// groups of 16 (one pass over the points for up to 16 objects) with the 2 x 64 (query, object) sums
// and the 2 x 4 per-query sums in registers.  Per group: wave butterflies, one LDS pass, thread
// (a, j) adds the four waves in wave order and writes the split's partial sums.
__global__ __launch_bounds__(256) void k_tri_pair(
    const float* __restrict__ sub_maps, const float* __restrict__ obj_maps,
    const float* __restrict__ pts, const float* __restrict__ t, const int64_t* __restrict__ tab,
    float2* __restrict__ part_pair, float2* __restrict__ part_q, int64_t SG, int B, int Q, int h,
    int w, int Np, int ns) {
  __shared__ float red[4][2 * TRI_TQ * TRI_TG + 2 * TRI_TQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = blockIdx.x * TRI_TQ, b = blockIdx.y >> 1, side = blockIdx.y & 1, split = blockIdx.z;
  const TriRow r = tri_row(tab, b);
  if (r.goff < 0 || r.G <= 0 || r.goff + r.G > SG) return;                 // (uniform)
  const int G = (int)r.G;
  const int64_t hw = (int64_t)h * w;
  const float* maps = (side ? obj_maps : sub_maps) + (int64_t)b * Q * hw;
  const float* qm[TRI_TQ];
#pragma unroll
  for (int a = 0; a < TRI_TQ; ++a) qm[a] = maps + (int64_t)min(q0 + a, Q - 1) * hw;
  const float2* p2 = reinterpret_cast<const float2*>(pts) + (int64_t)b * Np;
  const int chunks = (Np + 255) / 256, per = (chunks + ns - 1) / ns;
  const int i0 = split * per * 256 + tid, i1 = min((split + 1) * per * 256, Np);
  for (int g0 = 0; g0 < G; g0 += TRI_TG) {
    float xt[TRI_TQ][TRI_TG], st[TRI_TQ][TRI_TG], sneg[TRI_TQ], ssig[TRI_TQ];
#pragma unroll
    for (int a = 0; a < TRI_TQ; ++a) {
      sneg[a] = ssig[a] = 0.f;
#pragma unroll
      for (int j = 0; j < TRI_TG; ++j) xt[a][j] = st[a][j] = 0.f;
    }
    const float* tg[TRI_TG];
#pragma unroll
    for (int j = 0; j < TRI_TG; ++j) tg[j] = t + (r.goff + min(g0 + j, G - 1)) * Np;
    for (int i = i0; i < i1; i += 256) {
      const float2 p = p2[i];
      const TriTaps tp = tri_taps(p.x, p.y, h, w);
      float tv[TRI_TG];
#pragma unroll
      for (int j = 0; j < TRI_TG; ++j) tv[j] = tg[j][i];
#pragma unroll
      for (int a = 0; a < TRI_TQ; ++a) {
        const float v = tri_sample(qm[a], tp);
        const float s = 1.f / (1.f + expf(-v));
        if (g0 == 0) {                                                      // (uniform)
          sneg[a] += fmaxf(v, 0.f) + log1pf(expf(-fabsf(v)));     // BCE-with-logits against target 0
          ssig[a] += s;
        }
#pragma unroll
        for (int j = 0; j < TRI_TG; ++j) {
          xt[a][j] = fmaf(v, tv[j], xt[a][j]);
          st[a][j] = fmaf(s, tv[j], st[a][j]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < TRI_TQ; ++a)
#pragma unroll
      for (int j = 0; j < TRI_TG; ++j) {
        const float u = wave_sum(xt[a][j]), v = wave_sum(st[a][j]);
        if (lane == 0) {
          red[wave][a * TRI_TG + j] = u;
          red[wave][TRI_TQ * TRI_TG + a * TRI_TG + j] = v;
        }
      }
    if (g0 == 0) {
#pragma unroll
      for (int a = 0; a < TRI_TQ; ++a) {
        const float u = wave_sum(sneg[a]), v = wave_sum(ssig[a]);
        if (lane == 0) {
          red[wave][2 * TRI_TQ * TRI_TG + a] = u;
          red[wave][2 * TRI_TQ * TRI_TG + TRI_TQ + a] = v;
        }
      }
    }
    __syncthreads();
    if (tid < TRI_TQ * TRI_TG) {
      const int a = tid / TRI_TG, j = tid % TRI_TG;
      if (q0 + a < Q && g0 + j < G) {
        const int k = a * TRI_TG + j, k2 = TRI_TQ * TRI_TG + k;
        const float sxt = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        const float sst = ((red[0][k2] + red[1][k2]) + red[2][k2]) + red[3][k2];
        part_pair[(((int64_t)side * SG + r.goff + g0 + j) * Q + q0 + a) * ns + split] =
            make_float2(sxt, sst);
      }
    }
    if (g0 == 0 && tid >= 64 && tid < 64 + TRI_TQ && q0 + tid - 64 < Q) {
      const int a = tid - 64, k = 2 * TRI_TQ * TRI_TG + a, k2 = k + TRI_TQ;
      const float sn = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
      const float sg = ((red[0][k2] + red[1][k2]) + red[2][k2]) + red[3][k2];
      part_q[(((int64_t)side * B + b) * Q + q0 + a) * ns + split] = make_float2(sn, sg);
    }
    __syncthreads();                       // (red is written again by the next group)
  }
}

// The splits' partial sums added in ascending split order, then the two pair terms
//   pair[s][g][q] = { (sum_p BCE(x, 0) - sum_p x t) / Np * w_mask,
//                     (1 - (2 sum_p s t + eps) / (sum_p s + sum_p t + eps)) * w_dice }
// (BCE(x, 1) - BCE(x, 0) = -x, as k_mask_match_cost of csrc/loss.hip uses it).  One workgroup per
// (object of the image, image, side), a thread per query.
__global__ __launch_bounds__(128) void k_tri_pair_finish(
    const float2* __restrict__ part_pair, const float2* __restrict__ part_q,
    const float* __restrict__ tsum, const int64_t* __restrict__ tab, float2* __restrict__ pair,
    int64_t SG, int B, int Q, int Np, int ns, float ws_mask, float ws_dice, float ws_eps,
    float wo_mask, float wo_dice, float wo_eps) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, side = blockIdx.z;
  const TriRow r = tri_row(tab, b);
  if (r.goff < 0 || r.G < 0 || r.goff + r.G > SG || (int64_t)blockIdx.x >= r.G) return;   // (uniform)
  const int64_t g = r.goff + blockIdx.x;
  const float w_mask = side ? wo_mask : ws_mask, w_dice = side ? wo_dice : ws_dice;
  const float eps = side ? wo_eps : ws_eps;
  for (int q = threadIdx.x; q < Q; q += 128) {
    const float2* pp = part_pair + (((int64_t)side * SG + g) * Q + q) * ns;
    const float2* pq = part_q + (((int64_t)side * B + b) * Q + q) * ns;
    float sxt = 0.f, sst = 0.f, sn = 0.f, sg = 0.f;
    for (int s = 0; s < ns; ++s) {
      sxt += pp[s].x, sst += pp[s].y;
      sn += pq[s].x, sg += pq[s].y;
    }
    const float c_mask = (sn - sxt) / (float)Np * w_mask;
    const float c_dice = (1.f - (2.f * sst + eps) / (sg + tsum[g] + eps)) * w_dice;
    pair[((int64_t)side * SG + g) * Q + q] = make_float2(c_mask, c_dice);
  }
}

// ---- (c) compose: one lane per (query, relation) cell of image b's row-major Q x R_b block,
//   cost = s_cls + s_mask + s_dice + o_cls + o_mask + o_dice + r_cls, added left to right
// (approaches/matcher.py:75-83), x_cls = -softmax(logits[q])[label] * weight (ClassificationCost).
// A relation whose objects, predicate or labels are out of range gives NaN cells (pn_lsa_f32
// status 1: the image keeps its fills; pn_tri_targets names the cause).
__global__ __launch_bounds__(256) void k_tri_compose(
    const float* __restrict__ sub, const float* __restrict__ obj, const float* __restrict__ rel,
    const float2* __restrict__ stats, const float2* __restrict__ pair,
    const int64_t* __restrict__ gt_rels, int64_t rel_len, const int64_t* __restrict__ gt_labels,
    int64_t SG, const int64_t* __restrict__ tab, float* __restrict__ cost, int64_t cost_len, int B,
    int Q, int C1, int Cr1, float w_s, float w_o, float w_r) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const TriRow r = tri_row(tab, b);
  if (r.R <= 0 || r.coff < 0 || r.coff + (int64_t)Q * r.R > cost_len ||
      r.roff < 0 || r.roff + r.R > rel_len || r.goff < 0 || r.G < 0 || r.goff + r.G > SG)
    return;                                                                 // (uniform)
  const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= (int64_t)Q * r.R) return;
  const int q = (int)(cell / r.R), k = (int)(cell % r.R);
  const int64_t* gr = gt_rels + (r.roff + k) * 3;
  const int64_t so = gr[0], oo = gr[1], pr = gr[2];
  float c = __builtin_nanf("");
  if (so >= 0 && so < r.G && oo >= 0 && oo < r.G && pr >= 1 && pr < Cr1) {
    const int64_t ls = gt_labels[r.goff + so], lo = gt_labels[r.goff + oo];
    if (ls >= 0 && ls < C1 - 1 && lo >= 0 && lo < C1 - 1) {
      const int64_t rows = (int64_t)B * Q, row = (int64_t)b * Q + q;
      const float2 ss = stats[row], os = stats[rows + row], rs = stats[2 * rows + row];
      const float ps = expf(sub[row * C1 + ls] - ss.x) / ss.y;
      const float po = expf(obj[row * C1 + lo] - os.x) / os.y;
      const float pp = expf(rel[row * Cr1 + pr] - rs.x) / rs.y;
      const float2 sp = pair[(r.goff + so) * Q + q], op = pair[(SG + r.goff + oo) * Q + q];
      c = -ps * w_s;
      c += sp.x;
      c += sp.y;
      c += -po * w_o;
      c += op.x;
      c += op.y;
      c += -pp * w_r;
    }
  }
  cost[r.coff + cell] = c;
}

// point splits of k_tri_pair: enough workgroups to fill the device, whole 256-point chunks per split
static int tri_pair_splits(int B, int Q, int Np) {
  const int chunks = pn_cdiv(Np, 256), wgs = pn_cdiv(Q, TRI_TQ) * B * 2;
  int ns = 512 / wgs;
  ns = ns < 1 ? 1 : ns;
  ns = ns > chunks ? chunks : ns;
  return ns > TRI_MAX_SPLITS ? TRI_MAX_SPLITS : ns;
}

extern "C" int pn_tri_pair_splits(int B, int Q, int Np) {
  return (B <= 0 || Q <= 0 || Np <= 0) ? 0 : tri_pair_splits(B, Q, Np);
}

extern "C" int pn_tri_match_cost_f32(
    const float* sub_cls, const float* obj_cls, const float* rel_cls, const float* sub_maps,
    const float* obj_maps, const uint8_t* gt_masks, const float* pts, const int64_t* gt_rels,
    int64_t rel_len, const int64_t* gt_labels, int64_t SG, const int64_t* tab, int B, int Q, int C1,
    int Cr1, int h, int w, int hg, int wg, int Np, int max_G, int64_t max_cells, const float* weights,
    float* t, float* tsum, float* stats, float* pair, float* part, int64_t part_floats, float* cost,
    int64_t cost_len, void* stream) {
  if (!sub_cls || !obj_cls || !rel_cls || !sub_maps || !obj_maps || !gt_masks || !pts || !gt_rels ||
      !gt_labels || !tab || !weights || !t || !tsum || !stats || !pair || !part || !cost || B <= 0 ||
      B > 32767 || Q <= 0 || C1 < 2 || Cr1 < 2 || h <= 0 || w <= 0 || hg <= 0 ||
      wg <= 0 || Np <= 0 || SG <= 0 || rel_len <= 0 || max_G <= 0 || max_G > SG || max_cells <= 0 ||
      max_cells > ((int64_t)1 << 31) || cost_len <= 0 || (int64_t)h * w > 0x7fffffff ||
      (int64_t)hg * wg > 0x7fffffff ||
      (((uintptr_t)pts | (uintptr_t)stats | (uintptr_t)pair | (uintptr_t)part) & 7))
    return PN_BAD_ARG;
  const int ns = tri_pair_splits(B, Q, Np);
  if (part_floats < 4 * (SG + B) * (int64_t)Q * ns) return PN_BAD_ARG;
  float2* part_pair = reinterpret_cast<float2*>(part);
  float2* part_q = part_pair + 2 * SG * (int64_t)Q * ns;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_tri_gt_samples, dim3(max_G, B), dim3(256), 0, s, gt_masks, hg, wg, pts, tab, SG,
                     Np, t, tsum);
  hipLaunchKernelGGL(k_tri_row_stats, dim3(B * Q), dim3(192), 0, s, sub_cls, obj_cls, rel_cls, B * Q,
                     C1, Cr1, reinterpret_cast<float2*>(stats));
  hipLaunchKernelGGL(k_tri_pair, dim3(pn_cdiv(Q, TRI_TQ), 2 * B, ns), dim3(256), 0, s, sub_maps,
                     obj_maps, pts, t, tab, part_pair, part_q, SG, B, Q, h, w, Np, ns);
  hipLaunchKernelGGL(k_tri_pair_finish, dim3(max_G, B, 2), dim3(128), 0, s, part_pair, part_q, tsum,
                     tab, reinterpret_cast<float2*>(pair), SG, B, Q, Np, ns, weights[1], weights[2],
                     weights[7], weights[4], weights[5], weights[8]);
  hipLaunchKernelGGL(k_tri_compose, dim3(pn_cdiv(max_cells, 256), B), dim3(256), 0, s, sub_cls, obj_cls,
                     rel_cls, reinterpret_cast<const float2*>(stats),
                     reinterpret_cast<const float2*>(pair), gt_rels, rel_len, gt_labels, SG, tab, cost,
                     cost_len, B, Q, C1, Cr1, weights[0], weights[3], weights[6]);
  return PN_LAUNCH_CHECK();
}

// ---- targets of every image from the batched assignment (psgtr_head2.py:967-997 with
// MaskPseudoSampler: positives in ascending query order).  One workgroup walks the B images in
// order.  An image whose assignment failed, or whose relations / labels / indices are out of range,
// keeps its fills: labels C | C | Cr, its matched rows -1.
__global__ __launch_bounds__(256) void k_tri_targets(
    const int64_t* __restrict__ tab, const int32_t* __restrict__ row_ind,
    const int32_t* __restrict__ col_ind, int64_t out_len, const int32_t* __restrict__ lsa_status,
    const int64_t* __restrict__ gt_rels, int64_t rel_len, const int64_t* __restrict__ gt_labels,
    int64_t SG, int B, int Q, int C, int Cr, int64_t M, int64_t* __restrict__ labels,
    int64_t* __restrict__ matched, int64_t* __restrict__ side_rows, int64_t* __restrict__ rel_idx,
    int32_t* __restrict__ mcount, int32_t* __restrict__ status) {
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int64_t rows = (int64_t)B * Q;
  int acc = 0, cnt = 0;
  for (int b = 0; b < B; ++b) {
    const TriRow r = tri_row(tab, b);
    if (tid == 0) bad = 0;
    for (int q = tid; q < Q; q += 256) {
      labels[(int64_t)b * Q + q] = C;
      labels[rows + (int64_t)b * Q + q] = C;
      labels[2 * rows + (int64_t)b * Q + q] = Cr;
    }
    int st = lsa_status[b];
    const int64_t n = r.R < Q ? r.R : Q;
    if (r.R <= 0 || r.roff < 0 || r.roff + r.R > rel_len || r.goff < 0 ||
        r.G < 0 || r.goff + r.G > SG || r.ooff < 0 || r.ooff + n > out_len || r.ooff + n > M)
      st |= 8;
    if (st & 8) { acc |= st; continue; }             // (uniform: every thread read the same row)
    for (int64_t i = tid; i < n; i += 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        matched[(r.ooff + i) * 4 + k] = side_rows[(r.ooff + i) * 4 + k] =
            side_rows[(M + r.ooff + i) * 4 + k] = -1;
      rel_idx[r.ooff + i] = -1;
    }
    __syncthreads();
    for (int64_t k = tid; k < r.R; k += 256) {       // the device-side range check of gt_rels
      const int64_t* gr = gt_rels + (r.roff + k) * 3;
      bool ok = gr[0] >= 0 && gr[0] < r.G && gr[1] >= 0 && gr[1] < r.G && gr[2] >= 1 && gr[2] <= Cr;
      if (ok) {
        const int64_t ls = gt_labels[r.goff + gr[0]], lo = gt_labels[r.goff + gr[1]];
        ok = ls >= 0 && ls < C && lo >= 0 && lo < C;
      }
      if (!ok) atomicOr(&bad, 4);
    }
    if (st == 0) {
      for (int64_t i = tid; i < n; i += 256) {
        const int q = row_ind[r.ooff + i], k = col_ind[r.ooff + i];
        if (!(q >= 0 && q < Q && k >= 0 && k < r.R)) atomicOr(&bad, 4);
      }
    }
    __syncthreads();
    st |= bad;
    if (st == 0) {
      for (int64_t i = tid; i < n; i += 256) {
        const int q = row_ind[r.ooff + i], k = col_ind[r.ooff + i];
        const int64_t* gr = gt_rels + (r.roff + k) * 3;
        const int64_t so = r.goff + gr[0], oo = r.goff + gr[1];
        labels[(int64_t)b * Q + q] = gt_labels[so];
        labels[rows + (int64_t)b * Q + q] = gt_labels[oo];
        labels[2 * rows + (int64_t)b * Q + q] = gr[2];
        int64_t* m = matched + (r.ooff + i) * 4;
        m[0] = b, m[1] = q, m[2] = so, m[3] = oo;
        int64_t* s0 = side_rows + (r.ooff + i) * 4;
        int64_t* s1 = side_rows + (M + r.ooff + i) * 4;
        s0[0] = 0, s0[1] = b, s0[2] = q, s0[3] = so;
        s1[0] = 0, s1[1] = b, s1[2] = q, s1[3] = oo;
        rel_idx[r.ooff + i] = k;
      }
      cnt += (int)n;
    }
    acc |= st;
    __syncthreads();
  }
  if (tid == 0) { status[0] = acc; mcount[0] = cnt; }
}

extern "C" int pn_tri_targets(const int64_t* tab, const int32_t* row_ind, const int32_t* col_ind,
                              int64_t out_len, const int32_t* lsa_status, const int64_t* gt_rels,
                              int64_t rel_len, const int64_t* gt_labels, int64_t SG, int B, int Q,
                              int C, int Cr, int64_t M, int64_t* labels, int64_t* matched,
                              int64_t* side_rows, int64_t* rel_idx, int32_t* mcount, int32_t* status,
                              void* stream) {
  if (!tab || !row_ind || !col_ind || !lsa_status || !gt_rels || !gt_labels || !labels || !matched ||
      !side_rows || !rel_idx || !mcount || !status || B <= 0 || B > 65535 || Q <= 0 || C <= 0 ||
      Cr <= 0 || M <= 0 || out_len <= 0 || rel_len <= 0 || SG <= 0)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_tri_targets, dim3(1), dim3(256), 0, (hipStream_t)stream, tab, row_ind, col_ind,
                     out_len, lsa_status, gt_rels, rel_len, gt_labels, SG, B, Q, C, Cr, M, labels,
                     matched, side_rows, rel_idx, mcount, status);
  return PN_LAUNCH_CHECK();
}
