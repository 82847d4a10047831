// Flat-buffer Adam/AdamW with device-side dynamic loss scaling for gfx950.
//
// The whole optimizer phase of a training step is at most three launches,
// independent of the number of parameter tensors, and takes every
// data-dependent decision on the device so it can be recorded into a
// hipGraph:
//
//   flat_grad_finite_check  grid-stride pass over the flat gradient; raises
//                           found_inf when any element is inf/NaN
//   flat_adam_step          if found_inf: no-op.  Otherwise un-scale the
//                           gradient and apply torch.optim.Adam/AdamW math
//   flat_scale_update       one wave: torch.amp.GradScaler scale/tracker
//                           update, step counter, bias corrections of the
//                           next step; leaves found_inf cleared
//
// All data buffers are flat contiguous fp32 of length n (16-byte aligned):
// float4 body + scalar tail for n % 4, 256-thread blocks,
// grid = min(ceil(n / 1024), 2048) with a grid-stride loop, no LDS.
//
// Device state (fp32[FA_STATE_SIZE], integers are exact below 2^24):
//   [0] scale          [1] growth_tracker   [2] found_inf   [3] step
//   [4] lr             [5] skipped_steps
//   [6] 1 - beta1^(step+1)        bias correction 1 of the NEXT step
//   [7] sqrt(1 - beta2^(step+1))  sqrt of bias correction 2 of the NEXT step
// The bias corrections are produced in fp64 by the single-thread update
// kernel (1 - 0.999^t cancels badly in fp32) so the bandwidth kernel reads
// them instead of evaluating two pow() per thread.  flat_scale_update is the
// only writer of scale/step and runs after flat_adam_step in stream order,
// so no block of the step kernel can see a half-updated state.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "esr_common.h"

namespace {

constexpr int FA_SCALE = 0, FA_TRACKER = 1, FA_FOUND_INF = 2, FA_STEP = 3,
              FA_LR = 4, FA_SKIPPED = 5, FA_BC1 = 6, FA_BC2_SQRT = 7,
              FA_STATE_SIZE = 8;

ESR_INLINE bool fa_nonfinite(float x) {
  return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
}

// grid for n fp32 elements handled 4 per thread
inline int fa_grid(long long n) { return esr_grid(n, ESR_BLOCK * 4); }

__global__ void __launch_bounds__(ESR_BLOCK)
flat_grad_finite_check_kernel(long long n, const float* __restrict__ grad,
                              float* __restrict__ state) {
  const long long n4 = n >> 2;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad);
  bool bad = false;
  ESR_KERNEL_LOOP(i, n4) {
    const float4 g = g4[i];
    bad |= fa_nonfinite(g.x) | fa_nonfinite(g.y) | fa_nonfinite(g.z) |
           fa_nonfinite(g.w);
  }
  // scalar tail (n % 4 elements) on the first lanes of block 0
  const long long t = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) bad |= fa_nonfinite(grad[t]);
  // every detecting lane stores the same value: a benign race
  if (bad) state[FA_FOUND_INF] = 1.0f;
}

// 1 - beta is formed in fp64 on the host (as torch does) and rounded once:
// 1.0f - 0.999f would carry a 6e-5 relative error into exp_avg_sq
struct FaHyper {
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
};

template <bool AMSGRAD, bool DECOUPLED>
ESR_INLINE void fa_update(float& p, float g, float& m, float& v, float& vmax,
                          const FaHyper h, float inv_scale, float lr,
                          float step_size, float bc2_sqrt) {
  g *= inv_scale;
  if (h.weight_decay != 0.f) {
    if (DECOUPLED) p *= 1.0f - lr * h.weight_decay;
    else g += h.weight_decay * p;
  }
  m += (g - m) * h.one_minus_beta1;             // exp_avg.lerp_(g, 1-b1)
  v = v * h.beta2 + h.one_minus_beta2 * g * g;  // mul_(b2).addcmul_(g, g)
  float vv = v;
  if (AMSGRAD) {
    vmax = fmaxf(vmax, v);
    vv = vmax;
  }
  const float denom = sqrtf(vv) / bc2_sqrt + h.eps;
  p -= step_size * (m / denom);
}

template <bool AMSGRAD, bool DECOUPLED>
__global__ void __launch_bounds__(ESR_BLOCK)
flat_adam_step_kernel(long long n, float* __restrict__ param,
                      const float* __restrict__ grad,
                      float* __restrict__ exp_avg,
                      float* __restrict__ exp_avg_sq,
                      float* __restrict__ max_exp_avg_sq,
                      const float* __restrict__ state, const FaHyper h) {
  // overflow step: leave every buffer untouched
  if (state[FA_FOUND_INF] != 0.f) return;
  const float inv_scale = 1.0f / state[FA_SCALE];
  const float lr = state[FA_LR];
  const float step_size = lr / state[FA_BC1];
  const float bc2_sqrt = state[FA_BC2_SQRT];

  const long long n4 = n >> 2;
  float4* __restrict__ p4 = reinterpret_cast<float4*>(param);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad);
  float4* __restrict__ m4 = reinterpret_cast<float4*>(exp_avg);
  float4* __restrict__ v4 = reinterpret_cast<float4*>(exp_avg_sq);
  float4* __restrict__ x4 = reinterpret_cast<float4*>(max_exp_avg_sq);
  ESR_KERNEL_LOOP(i, n4) {
    float4 p = p4[i], m = m4[i], v = v4[i];
    const float4 g = g4[i];
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (AMSGRAD) x = x4[i];
    fa_update<AMSGRAD, DECOUPLED>(p.x, g.x, m.x, v.x, x.x, h, inv_scale, lr,
                                  step_size, bc2_sqrt);
    fa_update<AMSGRAD, DECOUPLED>(p.y, g.y, m.y, v.y, x.y, h, inv_scale, lr,
                                  step_size, bc2_sqrt);
    fa_update<AMSGRAD, DECOUPLED>(p.z, g.z, m.z, v.z, x.z, h, inv_scale, lr,
                                  step_size, bc2_sqrt);
    fa_update<AMSGRAD, DECOUPLED>(p.w, g.w, m.w, v.w, x.w, h, inv_scale, lr,
                                  step_size, bc2_sqrt);
    p4[i] = p;
    m4[i] = m;
    v4[i] = v;
    if (AMSGRAD) x4[i] = x;
  }
  const long long t = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float p = param[t], m = exp_avg[t], v = exp_avg_sq[t];
    float x = AMSGRAD ? max_exp_avg_sq[t] : 0.f;
    fa_update<AMSGRAD, DECOUPLED>(p, grad[t], m, v, x, h, inv_scale, lr,
                                  step_size, bc2_sqrt);
    param[t] = p;
    exp_avg[t] = m;
    exp_avg_sq[t] = v;
    if (AMSGRAD) max_exp_avg_sq[t] = x;
  }
}

__global__ void __launch_bounds__(64)
flat_scale_update_kernel(float* __restrict__ state, int scaling,
                         float growth_factor, float backoff_factor,
                         float growth_interval, double beta1, double beta2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state[FA_FOUND_INF] != 0.f) {
    state[FA_SCALE] *= backoff_factor;
    state[FA_TRACKER] = 0.f;
    state[FA_SKIPPED] += 1.0f;
  } else {
    const float step = state[FA_STEP] + 1.0f;
    state[FA_STEP] = step;
    const double next = (double)step + 1.0;
    state[FA_BC1] = (float)(1.0 - pow(beta1, next));
    state[FA_BC2_SQRT] = (float)sqrt(1.0 - pow(beta2, next));
    if (scaling) {
      float tracker = state[FA_TRACKER] + 1.0f;
      if (tracker >= growth_interval) {
        // GradScaler keeps the scale when growing it would overflow
        const float grown = state[FA_SCALE] * growth_factor;
        if (!fa_nonfinite(grown)) state[FA_SCALE] = grown;
        tracker = 0.f;
      }
      state[FA_TRACKER] = tracker;
    }
  }
  state[FA_FOUND_INF] = 0.f;
}

void fa_check_flat(const at::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat &&
              t.is_contiguous() && t.dim() == 1 && t.numel() == n,
              "flat_adam: ", name, " must be a contiguous 1-D fp32 CUDA "
              "tensor of length ", n);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr<float>()) % 16 == 0,
              "flat_adam: ", name, " must be 16-byte aligned");
}

void fa_check_state(const at::Tensor& state) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kFloat &&
              state.is_contiguous() && state.numel() == FA_STATE_SIZE,
              "flat_adam: state must be a contiguous fp32 CUDA tensor of ",
              FA_STATE_SIZE, " elements");
}

}  // namespace

void flat_grad_finite_check(const at::Tensor& grad, at::Tensor& state) {
  const int64_t n = grad.numel();
  fa_check_flat(grad, n, "grad");
  fa_check_state(state);
  TORCH_CHECK(state.device() == grad.device());
  if (n == 0) return;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(flat_grad_finite_check_kernel, dim3(fa_grid(n)),
                     dim3(ESR_BLOCK), 0, stream, (long long)n,
                     grad.data_ptr<float>(), state.data_ptr<float>());
}

void flat_adam_step(at::Tensor& param, const at::Tensor& grad,
                    at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                    const c10::optional<at::Tensor>& max_exp_avg_sq,
                    const at::Tensor& state, double beta1, double beta2,
                    double eps, double weight_decay, bool decoupled) {
  const int64_t n = param.numel();
  fa_check_flat(param, n, "param");
  fa_check_flat(grad, n, "grad");
  fa_check_flat(exp_avg, n, "exp_avg");
  fa_check_flat(exp_avg_sq, n, "exp_avg_sq");
  const bool amsgrad = max_exp_avg_sq.has_value();
  if (amsgrad) fa_check_flat(*max_exp_avg_sq, n, "max_exp_avg_sq");
  fa_check_state(state);
  TORCH_CHECK(grad.device() == param.device() &&
              exp_avg.device() == param.device() &&
              exp_avg_sq.device() == param.device() &&
              state.device() == param.device(),
              "flat_adam: all buffers must be on one device");
  if (n == 0) return;
  const FaHyper h{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                  (float)eps, (float)weight_decay};
  float* vmax = amsgrad ? max_exp_avg_sq->data_ptr<float>() : nullptr;
  auto stream = at::hip::getCurrentHIPStream();
  const dim3 grid(fa_grid(n)), block(ESR_BLOCK);
#define FA_LAUNCH(A, D)                                                     \
  hipLaunchKernelGGL((flat_adam_step_kernel<A, D>), grid, block, 0, stream, \
                     (long long)n, param.data_ptr<float>(),                 \
                     grad.data_ptr<float>(), exp_avg.data_ptr<float>(),     \
                     exp_avg_sq.data_ptr<float>(), vmax,                    \
                     state.data_ptr<float>(), h)
  if (amsgrad) {
    if (decoupled) FA_LAUNCH(true, true);
    else FA_LAUNCH(true, false);
  } else {
    if (decoupled) FA_LAUNCH(false, true);
    else FA_LAUNCH(false, false);
  }
#undef FA_LAUNCH
}

void flat_scale_update(at::Tensor& state, bool scaling, double growth_factor,
                       double backoff_factor, int64_t growth_interval,
                       double beta1, double beta2) {
  fa_check_state(state);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(flat_scale_update_kernel, dim3(1), dim3(64), 0, stream,
                     state.data_ptr<float>(), scaling ? 1 : 0,
                     (float)growth_factor, (float)backoff_factor,
                     (float)growth_interval, beta1, beta2);
}
