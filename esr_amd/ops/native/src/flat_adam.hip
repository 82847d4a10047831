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
// With gradient-norm clipping the finite check is replaced by a pass that
// also sums the squares, and one small launch is added:
//
//   flat_grad_stats         the finite check's pass over the flat gradient,
//                           which also leaves one fp64 partial sum of g^2
//                           per block in a scratch tensor
//   flat_clip_finish        one block: adds the partials, writes the
//                           un-scaled L2 norm and the clip coefficient
//   flat_adam_step          the clipped variant multiplies the un-scaled
//                           gradient by the coefficient
//
// The sum of squares is deterministic and atomic-free: fixed grid-stride
// order per thread, a fixed shuffle tree over the lanes, LDS across the
// waves in wave order, one plain store per block (eval_metrics.hip's idiom).
// (double)g * (double)g is exact for fp32 g and cannot overflow.
//
// All data buffers are flat contiguous fp32 of length n (16-byte aligned):
// float4 body + scalar tail for n % 4, 256-thread blocks,
// grid = min(ceil(n / 1024), 2048) with a grid-stride loop; only the two
// clipping kernels use LDS (one double per wave).
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
//
// Clip scalars (fp32[FA_CLIP_SIZE], a tensor of their own so the layout
// above stays as it is):
//   [0] grad_norm      un-scaled L2 norm of the last gradient
//   [1] clip_coef      min(1, max_norm / (grad_norm + 1e-6))
//   [2] clipped_steps  steps taken with clip_coef < 1
// flat_clip_finish is their only writer.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "esr_common.h"

namespace {

constexpr int FA_SCALE = 0, FA_TRACKER = 1, FA_FOUND_INF = 2, FA_STEP = 3,
              FA_LR = 4, FA_SKIPPED = 5, FA_BC1 = 6, FA_BC2_SQRT = 7,
              FA_STATE_SIZE = 8;
constexpr int FA_GRAD_NORM = 0, FA_CLIP_COEF = 1, FA_CLIPPED = 2,
              FA_CLIP_SIZE = 3;
constexpr int FA_WAVES = ESR_BLOCK / 64;

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

// Sum over the block in a fixed order: shuffle tree over the lanes, then the
// waves in wave order through `red`.  Every thread returns the block's sum.
ESR_INLINE double fa_block_sum(double v, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < FA_WAVES; ++w) s += red[w];
  return s;
}

// The finite check's pass, which also leaves the block's sum of g^2 in
// partial[blockIdx.x].  found_inf comes from the bit test, never from the sum.
__global__ void __launch_bounds__(ESR_BLOCK)
flat_grad_stats_kernel(long long n, const float* __restrict__ grad,
                       float* __restrict__ state,
                       double* __restrict__ partial) {
  __shared__ double red[FA_WAVES];
  const long long n4 = n >> 2;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad);
  bool bad = false;
  double sum = 0.0;
  ESR_KERNEL_LOOP(i, n4) {
    const float4 g = g4[i];
    bad |= fa_nonfinite(g.x) | fa_nonfinite(g.y) | fa_nonfinite(g.z) |
           fa_nonfinite(g.w);
    const double x = g.x, y = g.y, z = g.z, w = g.w;
    sum += x * x;
    sum += y * y;
    sum += z * z;
    sum += w * w;
  }
  const long long t = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float g = grad[t];
    bad |= fa_nonfinite(g);
    sum += (double)g * (double)g;
  }
  if (bad) state[FA_FOUND_INF] = 1.0f;
  const double s = fa_block_sum(sum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One block.  Thread t adds partials t, t + 256, ... in that order, then the
// block sums in fa_block_sum's fixed order.  fp64 until the final rounding.
__global__ void __launch_bounds__(ESR_BLOCK)
flat_clip_finish_kernel(int nparts, const double* __restrict__ partial,
                        const float* __restrict__ state,
                        float* __restrict__ clip, double max_norm) {
  __shared__ double red[FA_WAVES];
  double sum = 0.0;
  for (int i = (int)threadIdx.x; i < nparts; i += ESR_BLOCK)
    sum += partial[i];
  const double s = fa_block_sum(sum, red);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(s) / (double)state[FA_SCALE];
  const double coef = max_norm / (norm + 1e-6);
  const bool clips = coef < 1.0;  // false for a NaN norm
  clip[FA_GRAD_NORM] = (float)norm;
  clip[FA_CLIP_COEF] = clips ? (float)coef : 1.0f;
  // once per launch, so a graph replay counts its own step and no other
  if (clips && state[FA_FOUND_INF] == 0.f) clip[FA_CLIPPED] += 1.0f;
}

// 1 - beta is formed in fp64 on the host (as torch does) and rounded once:
// 1.0f - 0.999f would carry a 6e-5 relative error into exp_avg_sq
struct FaHyper {
  float one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
};

// CLIP: a second, separate multiply, so that un-scaling by a power of two
// stays exact; weight decay is added after it, as torch's clip_grad_norm_
// sees the raw gradients
template <bool AMSGRAD, bool DECOUPLED, bool CLIP = false>
ESR_INLINE void fa_update(float& p, float g, float& m, float& v, float& vmax,
                          const FaHyper h, float inv_scale, float lr,
                          float step_size, float bc2_sqrt,
                          float clip_coef = 1.0f) {
  g *= inv_scale;
  if (CLIP) g *= clip_coef;
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

// flat_adam_step_kernel with the clip coefficient that flat_clip_finish left
// behind.  A copy, not a shared body: sharing one changed the instructions
// the compiler emits for the unclipped kernels, and that path must launch
// exactly what it did before clipping existed.
template <bool AMSGRAD, bool DECOUPLED>
__global__ void __launch_bounds__(ESR_BLOCK)
flat_adam_clip_step_kernel(long long n, float* __restrict__ param,
                           const float* __restrict__ grad,
                           float* __restrict__ exp_avg,
                           float* __restrict__ exp_avg_sq,
                           float* __restrict__ max_exp_avg_sq,
                           const float* __restrict__ state,
                           const float* __restrict__ clip, const FaHyper h) {
  // overflow step: leave every buffer untouched
  if (state[FA_FOUND_INF] != 0.f) return;
  const float inv_scale = 1.0f / state[FA_SCALE];
  const float lr = state[FA_LR];
  const float step_size = lr / state[FA_BC1];
  const float bc2_sqrt = state[FA_BC2_SQRT];
  const float coef = clip[FA_CLIP_COEF];

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
    fa_update<AMSGRAD, DECOUPLED, true>(p.x, g.x, m.x, v.x, x.x, h, inv_scale,
                                        lr, step_size, bc2_sqrt, coef);
    fa_update<AMSGRAD, DECOUPLED, true>(p.y, g.y, m.y, v.y, x.y, h, inv_scale,
                                        lr, step_size, bc2_sqrt, coef);
    fa_update<AMSGRAD, DECOUPLED, true>(p.z, g.z, m.z, v.z, x.z, h, inv_scale,
                                        lr, step_size, bc2_sqrt, coef);
    fa_update<AMSGRAD, DECOUPLED, true>(p.w, g.w, m.w, v.w, x.w, h, inv_scale,
                                        lr, step_size, bc2_sqrt, coef);
    p4[i] = p;
    m4[i] = m;
    v4[i] = v;
    if (AMSGRAD) x4[i] = x;
  }
  const long long t = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float p = param[t], m = exp_avg[t], v = exp_avg_sq[t];
    float x = AMSGRAD ? max_exp_avg_sq[t] : 0.f;
    fa_update<AMSGRAD, DECOUPLED, true>(p, grad[t], m, v, x, h, inv_scale, lr,
                                        step_size, bc2_sqrt, coef);
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

void fa_check_clip(const at::Tensor& clip) {
  TORCH_CHECK(clip.is_cuda() && clip.scalar_type() == at::kFloat &&
              clip.is_contiguous() && clip.numel() == FA_CLIP_SIZE,
              "flat_adam: clip must be a contiguous fp32 CUDA tensor of ",
              FA_CLIP_SIZE, " elements");
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

namespace {

// clip == nullptr: the unclipped kernels with the arguments they always had
void fa_launch_step(at::Tensor& param, const at::Tensor& grad,
                    at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                    const c10::optional<at::Tensor>& max_exp_avg_sq,
                    const at::Tensor& state, const float* clip, double beta1,
                    double beta2, double eps, double weight_decay,
                    bool decoupled) {
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
  if (clip == nullptr)                                                      \
    hipLaunchKernelGGL((flat_adam_step_kernel<A, D>), grid, block, 0,       \
                       stream, (long long)n, param.data_ptr<float>(),       \
                       grad.data_ptr<float>(), exp_avg.data_ptr<float>(),   \
                       exp_avg_sq.data_ptr<float>(), vmax,                  \
                       state.data_ptr<float>(), h);                         \
  else                                                                      \
    hipLaunchKernelGGL((flat_adam_clip_step_kernel<A, D>), grid, block, 0,  \
                       stream, (long long)n, param.data_ptr<float>(),       \
                       grad.data_ptr<float>(), exp_avg.data_ptr<float>(),   \
                       exp_avg_sq.data_ptr<float>(), vmax,                  \
                       state.data_ptr<float>(), clip, h)
  if (amsgrad) {
    if (decoupled) { FA_LAUNCH(true, true); }
    else { FA_LAUNCH(true, false); }
  } else {
    if (decoupled) { FA_LAUNCH(false, true); }
    else { FA_LAUNCH(false, false); }
  }
#undef FA_LAUNCH
}

}  // namespace

// The finite check and the sum of squares in one pass, then the one-block
// finish.  `partial` is the optimizer's fp64 scratch (>= one per block).
void flat_grad_stats(const at::Tensor& grad, at::Tensor& state,
                     at::Tensor& partial, at::Tensor& clip, double max_norm) {
  const int64_t n = grad.numel();
  fa_check_flat(grad, n, "grad");
  fa_check_state(state);
  fa_check_clip(clip);
  const int blocks = fa_grid(n);
  TORCH_CHECK(partial.is_cuda() && partial.scalar_type() == at::kDouble &&
              partial.is_contiguous() && partial.numel() >= blocks,
              "flat_adam: partial must be a contiguous fp64 CUDA tensor of "
              "at least ", blocks, " elements");
  TORCH_CHECK(state.device() == grad.device() &&
              partial.device() == grad.device() &&
              clip.device() == grad.device(),
              "flat_adam: all buffers must be on one device");
  TORCH_CHECK(max_norm > 0.0, "flat_adam: max_norm must be positive");
  auto stream = at::hip::getCurrentHIPStream();
  // n == 0 still launches: one block writes a zero partial
  hipLaunchKernelGGL(flat_grad_stats_kernel, dim3(blocks), dim3(ESR_BLOCK), 0,
                     stream, (long long)n, grad.data_ptr<float>(),
                     state.data_ptr<float>(), partial.data_ptr<double>());
  hipLaunchKernelGGL(flat_clip_finish_kernel, dim3(1), dim3(ESR_BLOCK), 0,
                     stream, blocks, partial.data_ptr<double>(),
                     state.data_ptr<float>(), clip.data_ptr<float>(),
                     max_norm);
}

void flat_adam_step(at::Tensor& param, const at::Tensor& grad,
                    at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                    const c10::optional<at::Tensor>& max_exp_avg_sq,
                    const at::Tensor& state, double beta1, double beta2,
                    double eps, double weight_decay, bool decoupled) {
  fa_launch_step(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, state,
                 nullptr, beta1, beta2, eps, weight_decay, decoupled);
}

void flat_adam_step_clipped(at::Tensor& param, const at::Tensor& grad,
                            at::Tensor& exp_avg, at::Tensor& exp_avg_sq,
                            const c10::optional<at::Tensor>& max_exp_avg_sq,
                            const at::Tensor& state, const at::Tensor& clip,
                            double beta1, double beta2, double eps,
                            double weight_decay, bool decoupled) {
  fa_check_clip(clip);
  TORCH_CHECK(clip.device() == param.device(),
              "flat_adam: all buffers must be on one device");
  fa_launch_step(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, state,
                 clip.data_ptr<float>(), beta1, beta2, eps, weight_decay,
                 decoupled);
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
