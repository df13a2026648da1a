// The training log on the device (reference: mmcv's TextLoggerHook over LogBuffer.average behind
// `log_config = dict(interval=50, ...)`, configs/_base_/custom_runtime.py; the values are what
// mmdet's `_parse_losses` puts into `log_vars`).  mmcv calls `.item()` on every term of every
// iteration; here a training step's scalars never leave the device until a window is complete:
//   pn_train_log_row_f32     ONE launch per step: the step's T separate 0-dim scalars (their
//                            pointers travel BY VALUE in the kernel arguments), the sum of the
//                            loss terms, the status word and the skipped flag -> one ring row;
//   pn_train_log_window_f32  one launch per window: every column's mean in row order, the count
//                            of skipped steps and the OR of the status words -> one record.
// One wave each.  Plain vector stores, no atomics, no LDS; every sum is a serial fp32 chain in a
// fixed order, so a window's record is a function of the rows alone.
#include "common.h"

#define LOG_MAX_T 32

struct LogPtrs { const float* p[LOG_MAX_T]; };

// ring row (32-bit words): [0, T) the scalars | [T] loss | [T + 1] status (int32) | [T + 2] skipped
__global__ __launch_bounds__(64) void k_train_log_row(const LogPtrs src, int T, uint32_t loss_mask,
                                                      const int32_t* __restrict__ status0,
                                                      const int32_t* __restrict__ status1,
                                                      float* __restrict__ row) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  // lane i reads scalar i (static indices only: the pointer table stays in the argument segment)
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < LOG_MAX_T; ++i)
    if (i < T && i == lane) v = *src.p[i];
  if (lane < T) row[lane] = v;
  // `sum(v for k, v in losses.items() if "loss" in k)`: 0 + v_a + v_b + ... in dict order
  float loss = 0.f;
#pragma unroll
  for (int i = 0; i < LOG_MAX_T; ++i) {
    const float vi = __shfl(v, i, 64);
    if (i < T && ((loss_mask >> i) & 1u)) loss += vi;
  }
  if (lane == 0) {
    const int32_t st = (status0 ? *status0 : 0) | (status1 ? *status1 : 0);
    row[T] = loss;
    reinterpret_cast<int32_t*>(row)[T + 1] = st;
    row[T + 2] = st != 0 ? 1.f : 0.f;
  }
}

// record (32-bit words): [0, T] the means of the T scalars and of `loss` (float) |
// [T + 1] skipped steps (int32) | [T + 2] OR of the status words (int32) | [T + 3] n (int32)
__global__ __launch_bounds__(64) void k_train_log_window(const float* __restrict__ ring, int ld,
                                                         int n, int T, float* __restrict__ rec) {
#pragma clang fp contract(off)
  const int c = threadIdx.x;
  if (c <= T) {                         // (((v0 + v1) + ...) + v_{n-1}) / n
    float s = ring[c];
    for (int r = 1; r < n; ++r) s += ring[(int64_t)r * ld + c];
    rec[c] = s / (float)n;
  } else if (c == T + 1) {
    int32_t k = 0;
    for (int r = 0; r < n; ++r) k += ring[(int64_t)r * ld + T + 2] != 0.f ? 1 : 0;
    reinterpret_cast<int32_t*>(rec)[T + 1] = k;
  } else if (c == T + 2) {
    int32_t st = 0;
    for (int r = 0; r < n; ++r) st |= reinterpret_cast<const int32_t*>(ring)[(int64_t)r * ld + T + 1];
    reinterpret_cast<int32_t*>(rec)[T + 2] = st;
  } else if (c == T + 3) {
    reinterpret_cast<int32_t*>(rec)[T + 3] = n;
  }
}

extern "C" int pn_train_log_row_f32(const float* const* scalars, int T, uint32_t loss_mask,
                                    const int32_t* status0, const int32_t* status1, float* ring,
                                    int rows, int ld, int row, void* stream) {
  if (!scalars || !ring || T < 1 || T > LOG_MAX_T || rows < 1 || ld < T + 3 || row < 0 ||
      row >= rows)
    return PN_BAD_ARG;
  LogPtrs src;
  for (int i = 0; i < LOG_MAX_T; ++i) {
    if (i < T && !scalars[i]) return PN_BAD_ARG;
    src.p[i] = i < T ? scalars[i] : nullptr;
  }
  hipLaunchKernelGGL(k_train_log_row, dim3(1), dim3(64), 0, (hipStream_t)stream, src, T,
                     loss_mask, status0, status1, ring + (int64_t)row * ld);
  return PN_LAUNCH_CHECK();
}

extern "C" int pn_train_log_window_f32(const float* ring, int rows, int ld, int n, int T,
                                       float* record, void* stream) {
  if (!ring || !record || T < 1 || T > LOG_MAX_T || rows < 1 || ld < T + 3 || n < 1 || n > rows)
    return PN_BAD_ARG;
  hipLaunchKernelGGL(k_train_log_window, dim3(1), dim3(64), 0, (hipStream_t)stream, ring, ld, n, T,
                     record);
  return PN_LAUNCH_CHECK();
}
