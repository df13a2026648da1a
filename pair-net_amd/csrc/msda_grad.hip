// Deformable-attention backward with a bitwise reproducible grad_value (pn_msda_bwd_det_f32):
// no floating-point atomics.  The atomic entry (csrc/msda.hip: pn_msda_bwd_f32) adds every
// bilinear tap's 128-byte contribution row into grad_value in arrival order; here an inverted
// index per destination (batch, token, head) is built and each destination is summed by ONE
// owner in a fixed order (include/pairnet_hip.h states the order).  A contribution is
// coef x grad_output row, so the index stores 8-byte records {id, coef}, not rows.
//
//   1 k_msda_bwd_count  grad_sampling_loc / grad_attn_weight (the atomic kernel's body without
//                       its adds: msda_bwd_body.h) and one integer atomicAdd per in-map tap on
//                       cnt[(b*8 + head)*N + token]
//   2 k_scan_*          exclusive scan of the B*8*N counts -> start[]; cnt[] is zeroed again and
//                       becomes the fill cursor
//   3 k_msda_bwd_fill   taps recomputed; rec[start[bin] + atomicAdd(&cnt[bin], 1)] = {id, coef}
//                       (arbitrary order inside a bin)
//   4 k_msda_bwd_sum    a 32-lane half-wave per bin, lane = channel: the bin's records are sorted
//                       by id (a bitonic network, all compare-exchanges ascending, so that a
//                       length that is no power of two needs no padding) and summed in that
//                       order; a record costs one 128-byte grad_output row.
// Integer atomics only: counts do not depend on arrival order, and the order inside a bin is
// removed by the sort (ids are unique), so every launch computes the same bits.
#include "common.h"
#include "msda_bwd_body.h"

template <int L>
__global__ __launch_bounds__(512) void k_msda_bwd_count(const float* __restrict__ value,
                                                        const int64_t* __restrict__ shapes,
                                                        const int64_t* __restrict__ starts,
                                                        const float* __restrict__ loc,
                                                        const float* __restrict__ aw,
                                                        const float* __restrict__ gout,
                                                        float* __restrict__ gloc,
                                                        float* __restrict__ gaw,
                                                        int* __restrict__ cnt, const int N,
                                                        const int Nq, const int64_t ldv) {
  msda_bwd_lanes_body<L, true>(value, shapes, starts, loc, aw, gout, nullptr, gloc, gaw, cnt, N, Nq,
                               ldv);
}

// ---- exclusive scan of n int32 counts, 2048 per workgroup of 256 threads (8 consecutive per
// thread): block sums, a one-workgroup scan of the block sums, then every block scans its own
// 2048 again from its offset.
#define SCAN_TILE 2048

__device__ __forceinline__ int wave_incl_scan(int v, const int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(256) void k_scan_block_sums(const int* __restrict__ cnt,
                                                         int* __restrict__ bsum, const int n) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x;
  const int64_t j0 = (int64_t)blockIdx.x * SCAN_TILE + tid * 8;
  int s = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += (j0 + e < n) ? cnt[j0 + e] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) wtot[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) bsum[blockIdx.x] = (wtot[0] + wtot[1]) + (wtot[2] + wtot[3]);
}

// one workgroup: bsum[i] <- sum of bsum[0 .. i), 1024 at a time with a running carry
__global__ __launch_bounds__(1024) void k_scan_top(int* __restrict__ bsum, const int nblk) {
  __shared__ int wtot[16];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int j0 = 0; j0 < nblk; j0 += 1024) {
    const int j = j0 + tid;
    const int v = j < nblk ? bsum[j] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int off = carry;
    for (int x = 0; x < wave; ++x) off += wtot[x];
    if (j < nblk) bsum[j] = off + incl - v;
    if (tid == 1023) carry_s = off + incl;
    __syncthreads();
    carry = carry_s;
  }
}

__global__ __launch_bounds__(256) void k_scan_finish(int* __restrict__ cnt,
                                                     const int* __restrict__ bsum,
                                                     int* __restrict__ start, const int n) {
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * SCAN_TILE + tid * 8;
  int v[8], s = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] = (j0 + e < n) ? cnt[j0 + e] : 0;
    s += v[e];
  }
  const int incl = wave_incl_scan(s, lane);
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int off = bsum[blockIdx.x] + incl - s;
  for (int x = 0; x < wave; ++x) off += wtot[x];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (j0 + e < n) {
      start[j0 + e] = off;
      cnt[j0 + e] = 0;            // the fill pass's cursor
    }
    off += v[e];
  }
}

// ---- fill: one thread per (b, q, head, l, p), the count pass's taps again (msda_bwd_taps and
// the same token test), a record per in-map tap.  A slot at or past `cap` (it cannot be one while
// count and fill see the same inputs) is dropped, not written.
template <int L>
__global__ __launch_bounds__(256) void k_msda_bwd_fill(const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ starts,
                                                       const float* __restrict__ loc,
                                                       const float* __restrict__ aw,
                                                       const int* __restrict__ start,
                                                       int* __restrict__ cur,
                                                       int2* __restrict__ rec, const int cap,
                                                       const int N, const int Nq) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;        // ((q * 8 + head) * L + l) * 4 + p
  if (i >= Nq * 8 * L * 4) return;
  const int p = i & 3, l = (i >> 2) % L, qh = (i >> 2) / L, head = qh & 7, q = qh >> 3;
  const int64_t slot = (int64_t)b * Nq * 8 * L * 4 + i;
  const int Hl = (int)shapes[2 * l], Wl = (int)shapes[2 * l + 1];
  const int64_t base = starts[l];
  const float2 lc = *reinterpret_cast<const float2*>(loc + 2 * slot);
  const float a = aw[slot];
  const MsdaBwdTaps t = msda_bwd_taps(lc, Hl, Wl);
  const int id0 = ((q * L + l) * 4 + p) * 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t tok = base + t.tok[k];
    if (t.in[k] && tok >= 0 && tok < N) {
      const int64_t bin = (int64_t)(b * 8 + head) * N + tok;
      const int s = start[bin] + atomicAdd(&cur[bin], 1);
      if (s >= 0 && s < cap) rec[s] = make_int2(id0 + k, __float_as_int(t.w[k] * a));
    }
  }
}

// ---- order and sum.  Workgroup = 128 threads = 4 half-waves, a half-wave per bin.
// Bins of up to SUM_CAP = 1024 records are sorted in the half's 8 KB of LDS; LONGER BINS (the slow
// path starts at 1025 records; offsets can send every query to one pixel, up to Nq*L*16 records)
// are sorted in place in the record array with the same network and a device-scope fence per
// step.  Either way the cost is n log^2 n / 64 compare-exchanges per lane, never quadratic.
#define SUM_CAP 1024

// Bitonic sorting network in which EVERY compare-exchange puts the smaller id at the lower
// index: stage k merges blocks of k, its first step pairs i with i ^ (k - 1) (the mirrored
// partner), the later steps i with i ^ j.  Indices at and past len stand for +infinity, which
// such a network never moves, so pairs that reach past len are skipped.
template <bool GLOBAL>
__device__ __forceinline__ void half_sort(int2* buf, const int len, const int c) {
  // (unsigned: a list may hold up to 2^31 - 1 records, its padded length is then 2^31)
  const unsigned n = (unsigned)len;
  for (unsigned k = 2; k != 0 && (k >> 1) < n; k <<= 1) {
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      const unsigned mask = (j == (k >> 1)) ? (k - 1) : j;
      for (unsigned t = (unsigned)c;; t += 32) {
        const unsigned i = ((t & ~(j - 1)) << 1) | (t & (j - 1));   // t-th index with bit j clear
        if (i >= n) break;
        const unsigned p = i ^ mask;                                // > i
        if (p < n) {
          const int2 x = buf[i], y = buf[p];
          if (x.x > y.x) { buf[i] = y; buf[p] = x; }
        }
      }
      // the half's lanes run in lockstep; make the step's stores visible to the next step's loads
      if (GLOBAL) {
        __threadfence();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

template <int L>
__device__ __forceinline__ float half_sum(const int2* buf, const int len,
                                          const float* __restrict__ gb, const int Nq) {
  float acc = 0.f;
#pragma unroll 4
  for (int k = 0; k < len; ++k) {
    const int2 r = buf[k];
    const int q = min((int)((unsigned)r.x >> 4) / L, Nq - 1);   // (ids are ours; clamped all the same)
    acc = __fmaf_rn(__int_as_float(r.y), gb[(int64_t)q * 256], acc);
  }
  return acc;
}

template <int L>
__global__ __launch_bounds__(128) void k_msda_bwd_sum(const float* __restrict__ gout,
                                                      float* __restrict__ gvalue,
                                                      const int* __restrict__ start,
                                                      const int* __restrict__ cnt,
                                                      int2* rec, const int cap, const int nbins,
                                                      const int N, const int Nq,
                                                      const int64_t ldv) {
  __shared__ int2 seg[4][SUM_CAP];
  const int c = threadIdx.x & 31, h = threadIdx.x >> 5;
  const int bin = blockIdx.x * 4 + h;
  if (bin >= nbins) return;
  const int beg = start[bin];
  int len = cnt[bin];
  // (beg / len come from this entry's own passes; clamped so that a corrupted scratch cannot
  // send the loops outside the record array)
  if (beg < 0 || beg >= cap || len <= 0) return;
  len = min(len, cap - beg);
  const int bh = bin / N, token = bin - bh * N, b = bh >> 3, head = bh & 7;
  const float* gb = gout + (int64_t)b * Nq * 256 + head * 32 + c;
  float acc;
  if (len <= SUM_CAP) {
    for (int k = c; k < len; k += 32) seg[h][k] = rec[beg + k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    half_sort<false>(seg[h], len, c);
    acc = half_sum<L>(seg[h], len, gb, Nq);
  } else {
    half_sort<true>(rec + beg, len, c);
    acc = half_sum<L>(rec + beg, len, gb, Nq);
  }
  float* gv = gvalue + ((int64_t)b * N + token) * ldv + head * 32 + c;
  *gv = *gv + acc;
}

static inline int64_t a16(int64_t x) { return (x + 15) & ~(int64_t)15; }

struct DetLayout {
  int64_t nbins, nblk, nrec;
  int64_t off_start, off_bsum, off_rec, total;   // cnt sits at offset 0
};

static bool det_layout(int B, int N, int Nq, int L, DetLayout* d) {
  if (B <= 0 || N <= 0 || Nq <= 0 || L <= 0 || L > 4) return false;
  const int64_t lim = 0x7fffffff;
  if ((int64_t)Nq * L * 16 > lim) return false;
  d->nrec = (int64_t)B * Nq * 8 * L * 16;
  d->nbins = (int64_t)B * 8 * N;
  if (d->nrec > lim || d->nbins > lim) return false;
  d->nblk = (d->nbins + SCAN_TILE - 1) / SCAN_TILE;
  d->off_start = a16(d->nbins * 4);
  d->off_bsum = d->off_start + a16(d->nbins * 4);
  d->off_rec = d->off_bsum + a16(d->nblk * 4);
  d->total = d->off_rec + d->nrec * 8;
  return true;
}

extern "C" int64_t pn_msda_bwd_det_scratch_bytes(int B, int N, int Nq, int L) {
  DetLayout d;
  return det_layout(B, N, Nq, L, &d) ? d.total : 0;
}

extern "C" int pn_msda_bwd_det_f32(const float* value, int64_t ld_value,
                                   const int64_t* spatial_shapes, const int64_t* level_start_index,
                                   const float* sampling_locations, const float* attention_weights,
                                   const float* grad_output, float* grad_value,
                                   float* grad_sampling_loc, float* grad_attn_weight, void* scratch,
                                   int64_t scratch_bytes, int B, int N, int Nq, int L, void* stream) {
  if (!value || !spatial_shapes || !level_start_index || !sampling_locations ||
      !attention_weights || !grad_output || !grad_value || !grad_sampling_loc ||
      !grad_attn_weight || B <= 0 || N <= 0 || Nq <= 0 || L <= 0 || L > 4)
    return PN_BAD_ARG;
  if (ld_value < 256 || (ld_value & 3) || ((uintptr_t)value & 15) || ((uintptr_t)grad_value & 15) ||
      ((uintptr_t)grad_output & 15) || ((uintptr_t)sampling_locations & 7) ||
      ((uintptr_t)grad_sampling_loc & 7))
    return PN_BAD_ARG;
  DetLayout d;
  if (!det_layout(B, N, Nq, L, &d)) return PN_BAD_ARG;
  if (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < d.total) return PN_BAD_ARG;
  if (B > 65535) return PN_BAD_ARG;                       // (grid.y)
  char* sb = static_cast<char*>(scratch);
  int* cnt = reinterpret_cast<int*>(sb);
  int* start = reinterpret_cast<int*>(sb + d.off_start);
  int* bsum = reinterpret_cast<int*>(sb + d.off_bsum);
  int2* rec = reinterpret_cast<int2*>(sb + d.off_rec);
  const int nbins = (int)d.nbins, nblk = (int)d.nblk, cap = (int)d.nrec;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(cnt, 0, (size_t)d.nbins * 4, s) != hipSuccess) return (int)hipGetLastError();
  const dim3 gq(Nq, B), gf(pn_cdiv((int64_t)Nq * 8 * L * 4, 256), B);
#define PN_DET_COUNT(LL)                                                                         \
  hipLaunchKernelGGL(k_msda_bwd_count<LL>, gq, dim3(512), 0, s, value, spatial_shapes,           \
                     level_start_index, sampling_locations, attention_weights, grad_output,      \
                     grad_sampling_loc, grad_attn_weight, cnt, N, Nq, ld_value)
#define PN_DET_FILL(LL)                                                                          \
  hipLaunchKernelGGL(k_msda_bwd_fill<LL>, gf, dim3(256), 0, s, spatial_shapes, level_start_index, \
                     sampling_locations, attention_weights, start, cnt, rec, cap, N, Nq)
#define PN_DET_SUM(LL)                                                                           \
  hipLaunchKernelGGL(k_msda_bwd_sum<LL>, dim3(pn_cdiv(nbins, 4)), dim3(128), 0, s, grad_output,  \
                     grad_value, start, cnt, rec, cap, nbins, N, Nq, ld_value)
  switch (L) {
    case 1: PN_DET_COUNT(1); break;
    case 2: PN_DET_COUNT(2); break;
    case 3: PN_DET_COUNT(3); break;
    default: PN_DET_COUNT(4); break;
  }
  hipLaunchKernelGGL(k_scan_block_sums, dim3(nblk), dim3(256), 0, s, cnt, bsum, nbins);
  hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, bsum, nblk);
  hipLaunchKernelGGL(k_scan_finish, dim3(nblk), dim3(256), 0, s, cnt, bsum, start, nbins);
  switch (L) {
    case 1: PN_DET_FILL(1); PN_DET_SUM(1); break;
    case 2: PN_DET_FILL(2); PN_DET_SUM(2); break;
    case 3: PN_DET_FILL(3); PN_DET_SUM(3); break;
    default: PN_DET_FILL(4); PN_DET_SUM(4); break;
  }
#undef PN_DET_COUNT
#undef PN_DET_FILL
#undef PN_DET_SUM
  return PN_LAUNCH_CHECK();
}
