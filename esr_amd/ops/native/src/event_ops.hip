// Event-stream splatting kernels for gfx950.
//
// GPU-resident replacements for the reference's per-event Python/Cython
// CPU loops (ESR:dataloader/encodings.py:243-304, :204-240): batched event
// clouds [B, N, 4] (x, y, t, p) are splatted straight into count maps /
// stacks on the device with one float4 load per event and device-scope
// atomicAdd (scatter is uncoalesced by nature — guide Appendix B: rely on
// L2; events from one emitter are temporally clustered so neighbouring
// threads hit nearby lines).
//
// Zero-padded entries (p == 0) contribute nothing, matching the
// zero-padding convention of the collate (ESR:dataloader/h5dataloader.py:248).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "esr_common.h"

namespace {

// events: [B, N, 4]; out: [B, 2, H, W] (ch0 pos counts, ch1 neg counts)
__global__ void splat_count_kernel(long long n, int N, int H, int W,
                                   const float4* __restrict__ events,
                                   float* __restrict__ out) {
  ESR_KERNEL_LOOP(i, n) {
    const float4 e = events[i];
    const int b = i / N;
    const int xi = (int)e.x;
    const int yi = (int)e.y;
    if (e.w == 0.f || xi < 0 || xi >= W || yi < 0 || yi >= H) continue;
    const int ch = e.w > 0.f ? 0 : 1;
    const float wgt = fabsf(e.w);  // count magnitude (p = +/-1 -> 1 per event)
    atomicAdd(&out[(((long long)b * 2 + ch) * H + yi) * W + xi], wgt);
  }
}

// events: [B, N, 4] with t normalized to [0,1]; out: [B, TB, H, W] signed
__global__ void splat_stack_kernel(long long n, int N, int TB, int H, int W,
                                   const float4* __restrict__ events,
                                   float t0, float t1,
                                   float* __restrict__ out) {
  const float dt = t1 - t0 + 1e-6f;
  ESR_KERNEL_LOOP(i, n) {
    const float4 e = events[i];
    const int b = i / N;
    const int xi = (int)e.x;
    const int yi = (int)e.y;
    if (e.w == 0.f || xi < 0 || xi >= W || yi < 0 || yi >= H) continue;
    int bin = (int)((e.z - t0) / dt * TB);
    bin = bin < 0 ? 0 : (bin >= TB ? TB - 1 : bin);
    atomicAdd(&out[((((long long)b * TB) + bin) * H + yi) * W + xi], e.w);
  }
}

}  // namespace

// Work items one launch of a capped grid-stride kernel covers before any
// thread takes a second iteration (tests size their wrap cases from it).
int64_t grid_cap() { return (int64_t)ESR_MAX_BLOCKS * ESR_BLOCK; }

at::Tensor splat_count(const at::Tensor& events, int64_t H, int64_t W) {
  TORCH_CHECK(events.is_cuda() && events.scalar_type() == at::kFloat &&
              events.is_contiguous() && events.size(-1) == 4,
              "splat_count: contiguous fp32 [B,N,4] required");
  const int B = events.size(0), N = events.size(1);
  auto out = at::zeros({B, 2, H, W}, events.options());
  long long n = (long long)B * N;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(splat_count_kernel, dim3(esr_grid(n)), dim3(ESR_BLOCK),
                     0, stream, n, N, (int)H, (int)W,
                     reinterpret_cast<const float4*>(events.data_ptr<float>()),
                     out.data_ptr<float>());
  return out;
}

at::Tensor splat_stack(const at::Tensor& events, int64_t TB, int64_t H,
                       int64_t W, double t0, double t1) {
  TORCH_CHECK(events.is_cuda() && events.scalar_type() == at::kFloat &&
              events.is_contiguous() && events.size(-1) == 4);
  const int B = events.size(0), N = events.size(1);
  auto out = at::zeros({B, TB, H, W}, events.options());
  long long n = (long long)B * N;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(splat_stack_kernel, dim3(esr_grid(n)), dim3(ESR_BLOCK),
                     0, stream, n, N, (int)TB, (int)H, (int)W,
                     reinterpret_cast<const float4*>(events.data_ptr<float>()),
                     (float)t0, (float)t1, out.data_ptr<float>());
  return out;
}
