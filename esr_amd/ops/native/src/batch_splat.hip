// Batched training-feed splat for gfx950.
//
// DeviceSequenceLoader (data/device_loader.py) keeps every stored sequence on
// the device as one packed word per event and turns a training batch into a
// table of jobs; this kernel splats all of a batch's windows, input and GT,
// into their count-map planes in one launch.
//
// Capture-safe by construction: no allocation, no host synchronisation; which
// rows a job covers and how it is flipped are read from the `jobs` tensor on
// the device, so the launch geometry depends only on static shapes.
//
// The arithmetic is the CPU dataset's, bit for bit (data/dataset.py:
// _augment_events -> normalize_events -> scaled_count_encoding ->
// _mask_and_flatten), so training sees the same tensors from either loader.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <limits>
#include "esr_common.h"

namespace {

// events one block walks: ESR_BLOCK lanes x 4 coalesced dwords each
constexpr int BSPLAT_CHUNK = 4 * ESR_BLOCK;

constexpr int FLAG_HFLIP = 1, FLAG_VFLIP = 2, FLAG_PFLIP = 4, FLAG_GT = 8;

// LR pixel -> HR pixel the way normalize_events and scaled_count_encoding do
// it: an fp32 divide, then an fp32 multiply, each rounded on its own, then
// truncation toward zero.  Not v * scale: at lrW = 43, kW = 86 the column 15
// lands on 29.
ESR_INLINE int scaled_coord(int v, float lr, float hr) {
  return (int)__fmul_rn(__fdiv_rn((float)v, lr), hr);
}

// packed: [E] one word per event, x in bits 0-14, y in bits 15-29, bit 31 set
// for polarity -1.  jobs: [J] rows {begin, end, flags, reserved}.  Block
// (j, c) adds events begin + c*CHUNK .. of job j into plane out[j] ([2,kH,kW]).
__global__ __launch_bounds__(ESR_BLOCK) void evs_batch_splat_kernel(
    int E, int kH, int kW, int lrH, int lrW,
    const int* __restrict__ packed, const int4* __restrict__ jobs,
    float* __restrict__ out) {
  const int4 job = jobs[blockIdx.x];          // block-uniform
  // a row range is clipped to the event buffer, never trusted
  const int begin = job.x > 0 ? job.x : 0;
  const int end = job.y < E ? job.y : E;
  const int first = (int)blockIdx.y * BSPLAT_CHUNK;
  if (end <= begin || first >= end - begin) return;
  const int len = end - begin;
  const int stop = len - first < BSPLAT_CHUNK ? len : first + BSPLAT_CHUNK;

  const int flags = job.z;
  const bool gt = (flags & FLAG_GT) != 0;
  // the flip mirrors the grid the events were recorded on
  const int srcH = gt ? kH : lrH, srcW = gt ? kW : lrW;
  const float flH = (float)lrH, flW = (float)lrW;
  const float fkH = (float)kH, fkW = (float)kW;
  const long long plane = (long long)kH * kW;
  float* dst = out + (long long)blockIdx.x * 2 * plane;

  for (int i = first + (int)threadIdx.x; i < stop; i += ESR_BLOCK) {
    const unsigned w = (unsigned)packed[begin + i];
    int x = (int)(w & 0x7FFFu);
    int y = (int)((w >> 15) & 0x7FFFu);
    bool neg = (w >> 31) != 0;
    if (flags & FLAG_HFLIP) x = srcW - 1 - x;
    if (flags & FLAG_VFLIP) y = srcH - 1 - y;
    if (flags & FLAG_PFLIP) neg = !neg;
    if (!gt) {
      x = scaled_coord(x, flW, fkW);
      y = scaled_coord(y, flH, fkH);
    }
    if (x < 0 || x >= kW || y < 0 || y >= kH) continue;
    unsafeAtomicAdd(dst + (neg ? plane : 0) + (long long)y * kW + x, 1.0f);
  }
}

}  // namespace

int64_t evs_batch_splat_chunk() { return BSPLAT_CHUNK; }

void evs_batch_splat(const at::Tensor& packed, const at::Tensor& jobs,
                     at::Tensor& out, int64_t lrH, int64_t lrW,
                     int64_t max_job_len) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat &&
              out.is_contiguous() && out.dim() == 4 && out.size(1) == 2,
              "evs_batch_splat: contiguous fp32 [J,2,kH,kW] out required");
  const int64_t J = out.size(0), kH = out.size(2), kW = out.size(3);
  TORCH_CHECK(packed.is_cuda() && packed.scalar_type() == at::kInt &&
              packed.is_contiguous() && packed.dim() == 1 &&
              packed.size(0) <= std::numeric_limits<int>::max() &&
              packed.get_device() == out.get_device(),
              "evs_batch_splat: contiguous int32 [E] packed events required");
  TORCH_CHECK(jobs.is_cuda() && jobs.scalar_type() == at::kInt &&
              jobs.is_contiguous() && jobs.dim() == 2 && jobs.size(0) == J &&
              jobs.size(1) == 4 &&
              reinterpret_cast<uintptr_t>(jobs.data_ptr<int>()) % 16 == 0 &&
              jobs.get_device() == out.get_device(),
              "evs_batch_splat: contiguous 16-byte aligned int32 [J,4] jobs "
              "required");
  TORCH_CHECK(lrH >= 1 && lrW >= 1 && kH % lrH == 0 && kW % lrW == 0 &&
              kH / lrH == kW / lrW && kH < (1 << 15) && kW < (1 << 15),
              "evs_batch_splat: kH, kW must be the same multiple of lrH, lrW "
              "and below 32768");
  TORCH_CHECK(max_job_len >= 0, "evs_batch_splat: max_job_len is negative");
  const int64_t chunks = (max_job_len + BSPLAT_CHUNK - 1) / BSPLAT_CHUNK;
  TORCH_CHECK(J <= std::numeric_limits<int>::max() && chunks <= 65535,
              "evs_batch_splat: J or max_job_len exceeds the grid limit");
  if (J == 0 || chunks == 0 || packed.size(0) == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(evs_batch_splat_kernel, dim3((unsigned)J, (unsigned)chunks),
                     dim3(ESR_BLOCK), 0, stream, (int)packed.size(0), (int)kH,
                     (int)kW, (int)lrH, (int)lrW, packed.data_ptr<int>(),
                     reinterpret_cast<const int4*>(jobs.data_ptr<int>()),
                     out.data_ptr<float>());
}
