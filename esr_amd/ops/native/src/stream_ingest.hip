// Multi-stream serving ingest kernels for gfx950.
//
// MultiStreamESR (engine/multistream.py) keeps the sliding windows of S
// independent event streams in ONE static buffer [seqn, S, 2, kH, kW] (the
// model's frame-major input) and replays one captured graph per tick.  The
// two kernels here are the part of that graph that makes the streams
// independent: a per-stream window shift / reset and a ragged splat of the
// tick's concatenated events into each stream's newest frame.
//
// Capture-safe by construction: no allocation, no host synchronisation, and
// every per-tick decision (which stream shifts, which resets, where a
// stream's events start and end) is read from device tensors, so the launch
// geometry depends only on static shapes.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <limits>
#include "esr_common.h"

namespace {

template <typename V> ESR_INLINE V zero_of();
template <> ESR_INLINE float zero_of<float>() { return 0.f; }
template <> ESR_INLINE float4 zero_of<float4>() {
  return make_float4(0.f, 0.f, 0.f, 0.f);
}

// buf: [seqn, S, P] (P = 2*kH*kW) viewed as columns of V; one thread owns
// one column of one stream across all frames, so the shift f <- f+1 has no
// cross-thread hazard.  ctrl: [3, S] rows has_window, ready, reset.
template <typename V>
__global__ void stream_window_advance_kernel(long long n, int seqn, int S,
                                             long long cols,
                                             const int* __restrict__ ctrl,
                                             V* __restrict__ buf) {
  const long long fstride = (long long)S * cols;
  ESR_KERNEL_LOOP(i, n) {
    const int s = (int)(i / cols);
    const bool reset = ctrl[2 * S + s] != 0;
    const bool shift = ctrl[s] != 0;
    if (!reset && !shift) continue;
    V* col = buf + i;                       // (frame 0, stream s, column)
    const V zero = zero_of<V>();
    if (reset) {
      // a reset stream's frames are all zero, shifted or not
      for (int f = 0; f < seqn; ++f) col[f * fstride] = zero;
    } else {
      for (int f = 0; f + 1 < seqn; ++f)
        col[f * fstride] = col[(f + 1) * fstride];
      col[(long long)(seqn - 1) * fstride] = zero;
    }
  }
}

// events: [cap, 4] (x, y, t, p) in LR pixels, the streams' windows
// concatenated; stream s owns rows offsets[s]..offsets[s+1].  Adds |p| into
// buf[seqn-1, s, p>0 ? 0 : 1, floor(y)*scale, floor(x)*scale].
__global__ void stream_splat_ragged_kernel(int cap, int S, int lrH, int lrW,
                                           int scale,
                                           const float4* __restrict__ events,
                                           const int* __restrict__ offsets,
                                           const int* __restrict__ ctrl,
                                           float* __restrict__ last) {
  int total = offsets[S];
  total = total < cap ? total : cap;        // never read past the buffer
  const int kH = lrH * scale, kW = lrW * scale;
  ESR_KERNEL_LOOP(i, total) {
    // branch-free segment search: the number of segment ends at or before
    // row i (empty segments share an end and are stepped over together)
    int s = 0;
    for (int k = 1; k < S; ++k) s += (int)i >= offsets[k] ? 1 : 0;
    const float4 e = events[i];
    const float fx = floorf(e.x);
    const float fy = floorf(e.y);
    // range test on the LR grid in float: equal to testing xi, yi against
    // the HR grid, and immune to int overflow of a wild coordinate (NaN
    // fails every comparison)
    if (e.w == 0.f || !(fx >= 0.f && fx < (float)lrW) ||
        !(fy >= 0.f && fy < (float)lrH) || ctrl[s] == 0)
      continue;
    const int xi = (int)fx * scale;
    const int yi = (int)fy * scale;
    const int ch = e.w > 0.f ? 0 : 1;
    atomicAdd(&last[(((long long)s * 2 + ch) * kH + yi) * kW + xi],
              fabsf(e.w));
  }
}

}  // namespace

void stream_window_advance(at::Tensor& buf, const at::Tensor& ctrl) {
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == at::kFloat &&
              buf.is_contiguous() && buf.dim() == 5 && buf.size(2) == 2,
              "stream_window_advance: contiguous fp32 [seqn,S,2,kH,kW] "
              "required");
  const int seqn = buf.size(0), S = buf.size(1);
  TORCH_CHECK(ctrl.is_cuda() && ctrl.scalar_type() == at::kInt &&
              ctrl.is_contiguous() && ctrl.dim() == 2 && ctrl.size(0) == 3 &&
              ctrl.size(1) == S && ctrl.get_device() == buf.get_device(),
              "stream_window_advance: contiguous int32 [3,S] ctrl required");
  const long long P = 2LL * buf.size(3) * buf.size(4);
  if (seqn == 0 || S == 0 || P == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  float* p = buf.data_ptr<float>();
  const int* c = ctrl.data_ptr<int>();
  if (P % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0) {
    const long long cols = P / 4, n = (long long)S * cols;
    hipLaunchKernelGGL(stream_window_advance_kernel<float4>,
                       dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream, n, seqn,
                       S, cols, c, reinterpret_cast<float4*>(p));
  } else {
    const long long n = (long long)S * P;
    hipLaunchKernelGGL(stream_window_advance_kernel<float>,
                       dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream, n, seqn,
                       S, P, c, p);
  }
}

void stream_splat_ragged(const at::Tensor& events, const at::Tensor& offsets,
                         const at::Tensor& ctrl, at::Tensor& buf,
                         int64_t scale) {
  TORCH_CHECK(buf.is_cuda() && buf.scalar_type() == at::kFloat &&
              buf.is_contiguous() && buf.dim() == 5 && buf.size(2) == 2,
              "stream_splat_ragged: contiguous fp32 [seqn,S,2,kH,kW] "
              "required");
  const int seqn = buf.size(0), S = buf.size(1);
  const int64_t kH = buf.size(3), kW = buf.size(4);
  TORCH_CHECK(scale >= 1 && kH % scale == 0 && kW % scale == 0,
              "stream_splat_ragged: kH, kW must be multiples of scale");
  TORCH_CHECK(events.is_cuda() && events.scalar_type() == at::kFloat &&
              events.is_contiguous() && events.dim() == 2 &&
              events.size(1) == 4 &&
              events.size(0) <= std::numeric_limits<int>::max() &&
              reinterpret_cast<uintptr_t>(events.data_ptr<float>()) % 16 == 0 &&
              events.get_device() == buf.get_device(),
              "stream_splat_ragged: contiguous fp32 [cap,4] events required");
  TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == at::kInt &&
              offsets.is_contiguous() && offsets.dim() == 1 &&
              offsets.size(0) == S + 1 &&
              offsets.get_device() == buf.get_device(),
              "stream_splat_ragged: contiguous int32 [S+1] offsets required");
  TORCH_CHECK(ctrl.is_cuda() && ctrl.scalar_type() == at::kInt &&
              ctrl.is_contiguous() && ctrl.dim() == 2 && ctrl.size(0) == 3 &&
              ctrl.size(1) == S && ctrl.get_device() == buf.get_device(),
              "stream_splat_ragged: contiguous int32 [3,S] ctrl required");
  const int cap = events.size(0);
  if (cap == 0 || seqn == 0 || S == 0 || kH == 0 || kW == 0) return;
  float* last = buf.data_ptr<float>() + (int64_t)(seqn - 1) * S * 2 * kH * kW;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(stream_splat_ragged_kernel, dim3(esr_grid(cap)),
                     dim3(ESR_BLOCK), 0, stream, cap, S, (int)(kH / scale),
                     (int)(kW / scale), (int)scale,
                     reinterpret_cast<const float4*>(events.data_ptr<float>()),
                     offsets.data_ptr<int>(), ctrl.data_ptr<int>(), last);
}
