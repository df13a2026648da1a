// Training-mode dropout of the Relation Fusion decoder's FFN (mmcv FFN.layers: nn.Dropout(ffn_drop)
// after the ReLU and after the second Linear; configs/mask2former/pairnet.py:121-129 sets
// ffn_drop=0.1 for the relation decoder and 0.0 everywhere else).  Stateless and counter-based:
// no mask is stored and no generator state lives on the device.  An element's keep bit is a pure
// function of (seed, subseq, step, site, element index) through Philox4x32-10 (Salmon et al.,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11), so the backward pass regenerates the
// forward's mask by running the same launch on the gradient, and a step is reproducible from its
// number.
//
//   block j = i / 4 covers elements 4j .. 4j+3: counter = (j, subseq, site, step),
//   key = (seed & 0xffffffff, seed >> 32); element 4j + k reads output word k;
//   keep <=> word >= T, T = (uint32)((double)p * 2^32); s = (float)(1 / (1 - (double)p));
//   kept: y = x s (or fmaf(x, s, res)); dropped: y = 0 (or res).
//
// A latency-sized pass (0.8 MB at [100, 2048]): one thread per Philox block, one float4 load and
// one float4 store per thread, a scalar tail for n % 4.
#include "common.h"

struct PhiloxArgs {
  uint32_t key0, key1, subseq, site, step, thresh;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
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

template <bool RES>
__global__ __launch_bounds__(256) void k_dropout(const float* x, const float* __restrict__ res,
                                                 float* y, int64_t n, float s, PhiloxArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const int64_t i0 = (int64_t)j * 4;
  if (i0 >= n) return;
  uint32_t w[4];
  philox4x32_10(j, a.subseq, a.site, a.step, a.key0, a.key1, w);
  if (i0 + 4 <= n) {
    const float4 v = *reinterpret_cast<const float4*>(x + i0);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (RES) r = *reinterpret_cast<const float4*>(res + i0);
    float4 o;
    o.x = w[0] >= a.thresh ? (RES ? fmaf(v.x, s, r.x) : v.x * s) : r.x;
    o.y = w[1] >= a.thresh ? (RES ? fmaf(v.y, s, r.y) : v.y * s) : r.y;
    o.z = w[2] >= a.thresh ? (RES ? fmaf(v.z, s, r.z) : v.z * s) : r.z;
    o.w = w[3] >= a.thresh ? (RES ? fmaf(v.w, s, r.w) : v.w * s) : r.w;
    *reinterpret_cast<float4*>(y + i0) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (i0 + k >= n) break;
      const float v = x[i0 + k], r = RES ? res[i0 + k] : 0.f;
      y[i0 + k] = w[k] >= a.thresh ? (RES ? fmaf(v, s, r) : v * s) : r;
    }
  }
}

__global__ __launch_bounds__(256) void k_dropout_keep(uint8_t* __restrict__ keep, int64_t n,
                                                      PhiloxArgs a) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  const int64_t i0 = (int64_t)j * 4;
  if (i0 >= n) return;
  uint32_t w[4];
  philox4x32_10(j, a.subseq, a.site, a.step, a.key0, a.key1, w);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (i0 + k < n) keep[i0 + k] = w[k] >= a.thresh ? 1 : 0;
}

static bool dropout_args(int64_t n, float p, uint64_t seed, uint32_t subseq, uint32_t step,
                         uint32_t site, PhiloxArgs* a) {
  if (n <= 0 || n > ((int64_t)1 << 34) || !(p >= 0.f && p < 1.f)) return false;
  a->key0 = (uint32_t)(seed & 0xffffffffu);
  a->key1 = (uint32_t)(seed >> 32);
  a->subseq = subseq, a->site = site, a->step = step;
  a->thresh = (uint32_t)((double)p * 4294967296.0);
  return true;
}

extern "C" int pn_dropout_f32(const float* x, const float* res, float* y, int64_t n, float p,
                              uint64_t seed, uint32_t subseq, uint32_t step, uint32_t site,
                              void* stream) {
  PhiloxArgs a;
  if (!x || !y || !dropout_args(n, p, seed, subseq, step, site, &a)) return PN_BAD_ARG;
  if (((uintptr_t)x | (uintptr_t)res | (uintptr_t)y) & 15) return PN_BAD_ARG;
  const float s = (float)(1.0 / (1.0 - (double)p));
  const dim3 grid(pn_cdiv(pn_cdiv(n, 4), 256));
  if (res)
    hipLaunchKernelGGL(k_dropout<true>, grid, dim3(256), 0, (hipStream_t)stream, x, res, y, n, s, a);
  else
    hipLaunchKernelGGL(k_dropout<false>, grid, dim3(256), 0, (hipStream_t)stream, x, res, y, n, s,
                       a);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_dropout_keep_u8(uint8_t* keep, int64_t n, float p, uint64_t seed,
                                  uint32_t subseq, uint32_t step, uint32_t site, void* stream) {
  PhiloxArgs a;
  if (!keep || !dropout_args(n, p, seed, subseq, step, site, &a)) return PN_BAD_ARG;
  hipLaunchKernelGGL(k_dropout_keep, dim3(pn_cdiv(pn_cdiv(n, 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, keep, n, a);
  return PN_LAUNCH_CHECK();
}
