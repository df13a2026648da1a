// Panoptic quality (PQ / SQ / RQ) of one image from its panoptic map, on the device: what the
// reference's `--eval PQ` computes on the host (pairnet/datasets/psg.py:309-335 -> [3P] mmdet's
// panoptic evaluation over the map `pairnet_head.py:882` writes; restated from memory, unpinned:
// INTEGRATION.md 3a-2 is the specification).  pairnet_amd.evaluation.PanopticQuality drives it.
//
//   pn_pq_confusion: ONE pass over the pixels -> the joint histogram N[gt row][pred column]
//   pn_pq_record:    one workgroup: areas, the IoU > 0.5 matching, the (tp, fp, fn, iou) record
//
// Integer counts only in the pass over the pixels, so N does not depend on any order of
// execution; the float64 IoU sums of the record are added by one thread in ascending
// ground-truth id.
#include "common.h"

#define PQ_COLS 257        // column s = predicted segment s (< 256), column 256 = void
#define PQ_VOID 256
#define PQ_THREADS 512
#define PQ_LDS_MAX_G 61    // (G + 1) * 257 + 256 + G int32 <= 64 KB  <=>  G <= 61
#define PQ_MAX_G 255
#define PQ_MAX_CLASSES 999

__global__ __launch_bounds__(256) void k_pq_init(int32_t* __restrict__ N, int64_t n,
                                                 int32_t* __restrict__ col_cat,
                                                 int32_t* __restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) N[i] = 0;
  if (i < 256) col_cat[i] = -1;
  if (i == 0) status[0] = 0;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Every thread takes 4 consecutive pixels per step: 12 bytes of RGB = three aligned dwords, 32
// bytes of predictions = two 16-byte loads.  key = row * 257 + column, -1 for a flagged pixel.
// Segments are large, so nearly always the whole wavefront holds ONE key: then the counts are
// summed over the wave and one lane adds them (instead of 256 adds to one LDS word, which
// serialise); otherwise every lane adds its own runs of equal keys.
// Both lookups keep the last hit per thread: the 64-bit division of the predicted value and
// the binary search of the sorted id table run only where the value changes.
// LDS (dynamic): [256 column categories | G ids | (G + 1) * 257 bins when LDS_TABLE].
template <bool LDS_TABLE, bool PLAIN>
__global__ __launch_bounds__(PQ_THREADS) void k_pq_confusion(
    const int64_t* __restrict__ pred, const uint8_t* __restrict__ rgb, int64_t npix,
    const int32_t* __restrict__ gt_ids, int G, int num_classes, int offset,
    int32_t* __restrict__ N, int32_t* __restrict__ col_cat, int32_t* __restrict__ status) {
  extern __shared__ int32_t pq_smem[];
  int32_t* const cat = pq_smem;
  int32_t* const ids = pq_smem + 256;
  int32_t* const tab = pq_smem + 256 + G;
  const int nbins = (G + 1) * PQ_COLS;
  for (int i = threadIdx.x; i < 256; i += PQ_THREADS) cat[i] = -1;
  for (int i = threadIdx.x; i < G; i += PQ_THREADS) ids[i] = gt_ids[i];
  if (LDS_TABLE)
    for (int i = threadIdx.x; i < nbins; i += PQ_THREADS) tab[i] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int64_t ngroups = (npix + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * PQ_THREADS;
  unsigned st = 0;
  int64_t last_v = -1;                       // (a negative value is flagged before the compare)
  int last_col = -1;
  uint32_t last_id = 0;                      // id 0 is void: row 0
  int last_row = 0;
  const uint32_t* __restrict__ rgb32 = reinterpret_cast<const uint32_t*>(rgb);

  // `base` depends on the wave only: all 64 lanes stay in the loop together (ballots below)
  for (int64_t base = (int64_t)blockIdx.x * PQ_THREADS + (threadIdx.x & ~63); base < ngroups;
       base += stride) {
    const int64_t grp = base + lane;
    int64_t v[4];
    uint32_t id[4];
    int n = 0;
    if (grp < ngroups) {
      const int64_t p0 = grp << 2;
      n = (npix - p0 >= 4) ? 4 : (int)(npix - p0);
      if (n == 4) {
        const uint32_t w0 = rgb32[grp * 3], w1 = rgb32[grp * 3 + 1], w2 = rgb32[grp * 3 + 2];
        id[0] = w0 & 0xffffffu;
        id[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        id[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
        id[3] = w2 >> 8;
        const longlong2 a = *reinterpret_cast<const longlong2*>(pred + p0);
        const longlong2 b = *reinterpret_cast<const longlong2*>(pred + p0 + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
      } else {                               // the last, partial group: bytes, never past the end
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = j < n;
          const int64_t p = in ? p0 + j : p0;
          id[j] = (uint32_t)rgb[p * 3] | ((uint32_t)rgb[p * 3 + 1] << 8) |
                  ((uint32_t)rgb[p * 3 + 2] << 16);
          v[j] = pred[p];
        }
      }
    }
    int key[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      key[j] = -1;
      if (j < n) {
        int col;
        if (v[j] < 0) {
          st |= 1u;
          col = -1;
        } else if (v[j] == last_v) {
          col = last_col;
        } else {
          const int64_t s = v[j] / offset;
          const int c = (int)(v[j] - s * offset);
          col = -1;
          if (c > num_classes) st |= 1u;
          if (s >= 256) st |= 2u;
          if (c <= num_classes && s < 256) {
            if (c == num_classes) {
              col = PQ_VOID;
            } else {
              col = (int)s;
              const int old = atomicMax(&cat[col], c);
              if (old >= 0 && old != c) st |= 4u;
            }
          }
          last_v = v[j];
          last_col = col;
        }
        if (col >= 0) {
          int row;
          if (id[j] == last_id) {
            row = last_row;
          } else {
            int lo = 0, hi = G;              // first index with ids[i] >= id
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if ((uint32_t)ids[mid] < id[j]) lo = mid + 1; else hi = mid;
            }
            row = (id[j] != 0 && lo < G && (uint32_t)ids[lo] == id[j]) ? lo + 1 : 0;
            last_id = id[j];
            last_row = row;
          }
          key[j] = row * PQ_COLS + col;      // < (G + 1) * 257
        }
      }
    }
    if (PLAIN) {                             // one add per pixel (the form measured against)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (key[j] >= 0) atomicAdd(LDS_TABLE ? &tab[key[j]] : &N[key[j]], 1);
      continue;
    }
    int cnt = 0, kmax = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cnt += key[j] >= 0;
      kmax = key[j] > kmax ? key[j] : kmax;
    }
    bool single = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) single = single && (key[j] < 0 || key[j] == kmax);
    const unsigned long long active = __ballot(cnt > 0);
    if (active == 0ull) continue;
    const int lead = __ffsll((long long)active) - 1;
    const int kw = __shfl(kmax, lead, 64);
    const unsigned long long same = __ballot(cnt == 0 || (single && kmax == kw));
    if (same == ~0ull) {
      const int total = wave_sum_i(cnt);
      if (lane == lead) atomicAdd(LDS_TABLE ? &tab[kw] : &N[kw], total);
    } else {
      int cur = -1, run = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (key[j] < 0) continue;
        if (key[j] == cur) {
          ++run;
        } else {
          if (run) atomicAdd(LDS_TABLE ? &tab[cur] : &N[cur], run);
          cur = key[j];
          run = 1;
        }
      }
      if (run) atomicAdd(LDS_TABLE ? &tab[cur] : &N[cur], run);
    }
  }
  __syncthreads();
  if (LDS_TABLE)
    for (int i = threadIdx.x; i < nbins; i += PQ_THREADS) {
      const int c = tab[i];
      if (c) atomicAdd(&N[i], c);
    }
  // the maximum is the same whatever the order; of two different categories under one segment
  // the one that arrives second sees the other, here or in the LDS table above
  for (int i = threadIdx.x; i < 256; i += PQ_THREADS) {
    const int c = cat[i];
    if (c >= 0) {
      const int old = atomicMax(&col_cat[i], c);
      if (old >= 0 && old != c) st |= 4u;
    }
  }
  if (st) atomicOr(status, (int)st);
}

extern "C" int pn_pq_confusion(const int64_t* pred, const uint8_t* gt_rgb, int H, int W,
                               const int32_t* gt_ids, int G, int num_classes,
                               int instance_offset, int flags, int32_t* N, int32_t* col_cat,
                               int32_t* status, void* stream) {
  if (!pred || !gt_rgb || !gt_ids || !N || !col_cat || !status || H <= 0 || W <= 0 ||
      (int64_t)H * W >= ((int64_t)1 << 31) || G < 0 || G > PQ_MAX_G || num_classes < 1 ||
      num_classes > PQ_MAX_CLASSES || instance_offset <= num_classes ||
      ((uintptr_t)pred & 15) || ((uintptr_t)gt_rgb & 3) || (flags & ~PN_PQ_PLAIN))
    return PN_BAD_ARG;
  const int64_t npix = (int64_t)H * W, nbins = (int64_t)(G + 1) * PQ_COLS;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_pq_init, dim3(pn_cdiv(nbins, 256)), dim3(256), 0, s, N, nbins, col_cat,
                     status);
  // two steps per thread at the least: a workgroup's table is zeroed and flushed once
  int64_t blocks = ((npix + 3) / 4 + 2 * PQ_THREADS - 1) / (2 * PQ_THREADS);
  blocks = blocks < 1 ? 1 : (blocks > 256 ? 256 : blocks);
  const bool lds = G <= PQ_LDS_MAX_G, plain = (flags & PN_PQ_PLAIN) != 0;
  const size_t smem = (size_t)(256 + G + (lds ? nbins : 0)) * sizeof(int32_t);
#define PQ_LAUNCH(L, P)                                                                         \
  hipLaunchKernelGGL((k_pq_confusion<L, P>), dim3((unsigned)blocks), dim3(PQ_THREADS), smem, s, \
                     pred, gt_rgb, npix, gt_ids, G, num_classes, instance_offset, N, col_cat,   \
                     status)
  if (lds && plain) PQ_LAUNCH(true, true);
  else if (lds) PQ_LAUNCH(true, false);
  else if (plain) PQ_LAUNCH(false, true);
  else PQ_LAUNCH(false, false);
#undef PQ_LAUNCH
  return PN_LAUNCH_CHECK();
}

// One workgroup.  Rows: 0 = void, g = 1..G the ground-truth segments in ascending id.
__global__ __launch_bounds__(256) void k_pq_record(
    const int32_t* __restrict__ N, const int32_t* __restrict__ col_cat,
    const int32_t* __restrict__ gt_cat, const int32_t* __restrict__ gt_crowd, int G,
    int num_classes, int32_t* __restrict__ area_gt, int32_t* __restrict__ area_pred,
    int32_t* __restrict__ match, int32_t* __restrict__ rec, double* __restrict__ iou,
    int32_t* __restrict__ status) {
  __shared__ int ap[PQ_COLS], ag[PQ_MAX_G + 1], pcat[256], pmatched[256], gmatch[PQ_MAX_G + 1];
  __shared__ int srec[PQ_MAX_CLASSES * 3];
  __shared__ double siou[PQ_MAX_CLASSES];
  // the tables and every row's matched (N, union) in LDS: the serial walk below then never waits
  // for global memory
  __shared__ int scat[PQ_MAX_G + 1], scrowd[PQ_MAX_G + 1], gn[PQ_MAX_G + 1];
  __shared__ long long gu[PQ_MAX_G + 1];
  const int t = threadIdx.x;
  if (t < G) {
    scat[t + 1] = gt_cat[t];
    scrowd[t + 1] = gt_crowd[t];
  }
  for (int i = t; i < num_classes * 3; i += 256) srec[i] = 0;
  for (int i = t; i < num_classes; i += 256) siou[i] = 0.0;
  pmatched[t] = 0;
  pcat[t] = col_cat[t];
  for (int p = t; p < PQ_COLS; p += 256) {
    int a = 0;
    for (int g = 0; g <= G; ++g) a += N[g * PQ_COLS + p];
    ap[p] = a;
  }
  for (int g = t; g <= G; g += 256) {
    int a = 0;
    for (int p = 0; p < PQ_COLS; ++p) a += N[g * PQ_COLS + p];
    ag[g] = a;
    gmatch[g] = -1;
  }
  __syncthreads();
  // iou > 0.5 decided in integers; at most one pair per row and per column satisfies it
  for (int g = 1 + t; g <= G; g += 256) {
    const int c = scat[g];
    if (scrowd[g] || c < 0 || c >= num_classes) continue;
    for (int p = 0; p < 256; ++p) {
      if (pcat[p] != c) continue;
      const int n = N[g * PQ_COLS + p];
      if (n <= 0) continue;
      const int64_t uni = (int64_t)ap[p] + ag[g] - n - N[p];
      if (2 * (int64_t)n > uni) {
        gmatch[g] = p;
        gn[g] = n;
        gu[g] = uni;
        pmatched[p] = 1;
      }
    }
  }
  __syncthreads();
  if (t == 0) {                              // float64 sums in ascending ground-truth id
    unsigned st = 0;
    for (int g = 1; g <= G; ++g) {
      const int c = scat[g];
      if (c < 0 || c >= num_classes) { st |= 8u; continue; }
      if (scrowd[g]) continue;
      if (gmatch[g] >= 0) {
        srec[c * 3] += 1;
        siou[c] += (double)gn[g] / (double)gu[g];
      } else {
        srec[c * 3 + 2] += 1;
      }
    }
    if (st) atomicOr(status, (int)st);
  }
  {                                          // false positives: thread t = column t
    const int c = pcat[t];
    if (c >= 0 && c < num_classes && !pmatched[t] && ap[t] > 0) {
      int64_t absorbed = N[t];               // void row + the crowd rows of this category
      for (int g = 1; g <= G; ++g)
        if (scrowd[g] && scat[g] == c) absorbed += N[g * PQ_COLS + t];
      if (!(2 * absorbed > (int64_t)ap[t])) atomicAdd(&srec[c * 3 + 1], 1);
    }
  }
  __syncthreads();
  for (int i = t; i < num_classes * 3; i += 256) rec[i] = srec[i];
  for (int i = t; i < num_classes; i += 256) iou[i] = siou[i];
  for (int p = t; p < PQ_COLS; p += 256) area_pred[p] = ap[p];
  for (int g = t; g <= G; g += 256) {
    area_gt[g] = ag[g];
    match[g] = gmatch[g];
  }
}

extern "C" int pn_pq_record(const int32_t* N, const int32_t* col_cat, const int32_t* gt_cat,
                            const int32_t* gt_crowd, int G, int num_classes, int32_t* area_gt,
                            int32_t* area_pred, int32_t* match, int32_t* rec, double* iou,
                            int32_t* status, void* stream) {
  if (!N || !col_cat || !gt_cat || !gt_crowd || !area_gt || !area_pred || !match || !rec ||
      !iou || !status || G < 0 || G > PQ_MAX_G || num_classes < 1 ||
      num_classes > PQ_MAX_CLASSES)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_pq_record, dim3(1), dim3(256), 0, (hipStream_t)stream, N, col_cat, gt_cat,
                     gt_crowd, G, num_classes, area_gt, area_pred, match, rec, iou, status);
  return PN_LAUNCH_CHECK();
}
