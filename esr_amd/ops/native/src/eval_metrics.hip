// Fused restoration metrics for gfx950: one pass over a pair of maps.
//
// restoration_metrics(pred, tgt, data_range) -> double [P, 5]; per plane
//   0  sum |p - t|      1  sum (p - t)^2      2  max t      3  min t
//   4  sum of SSIM over the (H-6)(W-6) valid 7x7 window positions
// SSIM is loss/metrics.py::_ssim_single: uniform 7x7 window, valid border,
// covariances times 49/48, K1 = 0.01, K2 = 0.03, C = (K * data_range)^2.
//
// A block owns a METRIC_TH x METRIC_TW tile of pixels and stages p and t into
// LDS with a 6-pixel halo on the right and bottom: every window is anchored at
// its top-left pixel, so the halo is one-sided.  The five window sums and the
// SSIM value are formed in fp64 by a direct 49-tap sum; the inputs are fp32,
// so every product is exact in fp64 and only the additions round.
//
// Deterministic two-stage reduction, no atomics: lane shuffles in a fixed
// order, LDS across the waves in wave order, one plain store of five partials
// per block into [P, tiles, 5]; a second kernel adds the tiles of a plane in
// index order.  Two launches on the same inputs are bitwise equal.
//
// Capture-safe: no host synchronisation, geometry from static shapes only.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <limits>
#include "esr_common.h"

namespace {

constexpr int METRIC_WIN = 7;
constexpr int METRIC_HALO = METRIC_WIN - 1;
// 256 lanes as 32 columns x 8 rows; a lane walks 4 rows 8 apart
constexpr int METRIC_TW = 32;
constexpr int METRIC_TH = 32;
constexpr int METRIC_ROWS_PER_LANE = METRIC_TH / (ESR_BLOCK / METRIC_TW);
constexpr int METRIC_LW = METRIC_TW + METRIC_HALO;     // 38 staged columns
constexpr int METRIC_LH = METRIC_TH + METRIC_HALO;     // 38 staged rows
// Row stride in dwords, padded from 38.  The tile is 32 wide so that a
// half-wave (the group LDS banking is decided in) reads 32 consecutive dwords
// of ONE row for every tap: conflict-free on the 32 dword banks whatever the
// stride (a 16-wide tile would put two rows in a half-wave and need
// stride % 32 == 16).  The pad to 40 keeps row starts 32-byte aligned.
constexpr int METRIC_LS = 40;
constexpr int METRIC_WAVES = ESR_BLOCK / 64;
constexpr int METRIC_COLS = 5;

static_assert(ESR_BLOCK % METRIC_TW == 0 &&
              METRIC_TH % (ESR_BLOCK / METRIC_TW) == 0, "tile / block shape");

template <typename Op>
ESR_INLINE double wave_reduce(double v, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_down(v, off, 64));
  return v;                                   // lane 0 holds the result
}

struct OpAdd { ESR_INLINE double operator()(double a, double b) const { return a + b; } };
struct OpMax { ESR_INLINE double operator()(double a, double b) const { return a > b ? a : b; } };
struct OpMin { ESR_INLINE double operator()(double a, double b) const { return a < b ? a : b; } };

// grid (tilesX * tilesY, P); partial: [P, tiles, 5]
__global__ __launch_bounds__(ESR_BLOCK) void restoration_metrics_tile_kernel(
    int H, int W, int tilesX, double C1, double C2,
    const float* __restrict__ pred, const float* __restrict__ tgt,
    double* __restrict__ partial) {
  // No fused multiply-add here: for p == t the numerator and the denominator
  // must round alike (ux*ux + uy*uy == 2*ux*uy, bit for bit) so that SSIM is
  // exactly 1; fma(ux, ux, uy*uy) rounds once less and gives 1 + 2^-52.
#pragma clang fp contract(off)
  __shared__ float sp[METRIC_LH * METRIC_LS];
  __shared__ float st[METRIC_LH * METRIC_LS];
  __shared__ double red[METRIC_COLS][METRIC_WAVES];

  const int tile = (int)blockIdx.x;
  const int y0 = (tile / tilesX) * METRIC_TH;
  const int x0 = (tile % tilesX) * METRIC_TW;
  const long long base = (long long)blockIdx.y * H * W;
  const float* p = pred + base;
  const float* t = tgt + base;

  // stage; pixels outside the plane read as 0 and no valid window sees them
  for (int i = (int)threadIdx.x; i < METRIC_LH * METRIC_LW; i += ESR_BLOCK) {
    const int r = i / METRIC_LW, c = i % METRIC_LW;
    const int y = y0 + r, x = x0 + c;
    const bool in = y < H && x < W;
    const long long g = (long long)y * W + x;
    sp[r * METRIC_LS + c] = in ? p[g] : 0.0f;
    st[r * METRIC_LS + c] = in ? t[g] : 0.0f;
  }
  __syncthreads();

  const int tx = (int)threadIdx.x % METRIC_TW;
  const int ty = (int)threadIdx.x / METRIC_TW;
  const double inv_n = 1.0 / (METRIC_WIN * METRIC_WIN);
  const double cov_norm = (double)(METRIC_WIN * METRIC_WIN) /
                          (double)(METRIC_WIN * METRIC_WIN - 1);

  double s_abs = 0.0, s_sq = 0.0, s_ssim = 0.0;
  double t_max = -std::numeric_limits<double>::infinity();
  double t_min = std::numeric_limits<double>::infinity();

#pragma unroll 1
  for (int k = 0; k < METRIC_ROWS_PER_LANE; ++k) {
    const int r = ty + k * (ESR_BLOCK / METRIC_TW);
    const int y = y0 + r, x = x0 + tx;
    if (y >= H || x >= W) continue;
    const float* rp = sp + r * METRIC_LS + tx;
    const float* rt = st + r * METRIC_LS + tx;
    const double pv = (double)rp[0], tv = (double)rt[0];
    const double d = pv - tv;
    s_abs += fabs(d);
    s_sq += d * d;
    t_max = tv > t_max ? tv : t_max;
    t_min = tv < t_min ? tv : t_min;
    if (y > H - METRIC_WIN || x > W - METRIC_WIN) continue;

    // row-major 49-tap sums; a*b is exact for fp32 a, b
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int dy = 0; dy < METRIC_WIN; ++dy) {
#pragma unroll
      for (int dx = 0; dx < METRIC_WIN; ++dx) {
        const double a = (double)rp[dy * METRIC_LS + dx];
        const double b = (double)rt[dy * METRIC_LS + dx];
        sx += a;
        sy += b;
        sxx += a * a;
        syy += b * b;
        sxy += a * b;
      }
    }
    const double ux = sx * inv_n, uy = sy * inv_n;
    const double uxx = sxx * inv_n, uyy = syy * inv_n, uxy = sxy * inv_n;
    const double vx = cov_norm * (uxx - ux * ux);
    const double vy = cov_norm * (uyy - uy * uy);
    const double vxy = cov_norm * (uxy - ux * uy);
    const double num = (2.0 * ux * uy + C1) * (2.0 * vxy + C2);
    const double den = (ux * ux + uy * uy + C1) * (vx + vy + C2);
    s_ssim += num / den;
  }

  // lanes -> wave (fixed shuffle order) -> block (wave order)
  const double w0 = wave_reduce(s_abs, OpAdd());
  const double w1 = wave_reduce(s_sq, OpAdd());
  const double w2 = wave_reduce(t_max, OpMax());
  const double w3 = wave_reduce(t_min, OpMin());
  const double w4 = wave_reduce(s_ssim, OpAdd());
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = w0;
    red[1][wave] = w1;
    red[2][wave] = w2;
    red[3][wave] = w3;
    red[4][wave] = w4;
  }
  __syncthreads();
  if (threadIdx.x < METRIC_COLS) {
    const int c = (int)threadIdx.x;
    double v = red[c][0];
    for (int w = 1; w < METRIC_WAVES; ++w) {
      const double o = red[c][w];
      v = c == 2 ? (o > v ? o : v) : c == 3 ? (o < v ? o : v) : v + o;
    }
    partial[((long long)blockIdx.y * gridDim.x + tile) * METRIC_COLS + c] = v;
  }
}

// one lane per (plane, column): the tiles of a plane in index order
__global__ __launch_bounds__(ESR_BLOCK) void restoration_metrics_finish_kernel(
    int P, int tiles, const double* __restrict__ partial,
    double* __restrict__ out) {
  const int q = (int)blockIdx.x * ESR_BLOCK + (int)threadIdx.x;
  if (q >= P * METRIC_COLS) return;
  const int plane = q / METRIC_COLS, c = q % METRIC_COLS;
  const double* src = partial + (long long)plane * tiles * METRIC_COLS + c;
  double v = src[0];
  for (int i = 1; i < tiles; ++i) {
    const double o = src[(long long)i * METRIC_COLS];
    v = c == 2 ? (o > v ? o : v) : c == 3 ? (o < v ? o : v) : v + o;
  }
  out[q] = v;
}

}  // namespace

std::vector<int64_t> restoration_metrics_tile() {
  return {METRIC_TH, METRIC_TW};
}

at::Tensor restoration_metrics(const at::Tensor& pred, const at::Tensor& tgt,
                               double data_range) {
  TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == at::kFloat &&
              pred.is_contiguous() && pred.dim() == 3,
              "restoration_metrics: contiguous fp32 [P,H,W] pred required");
  TORCH_CHECK(tgt.is_cuda() && tgt.scalar_type() == at::kFloat &&
              tgt.is_contiguous() && tgt.sizes() == pred.sizes() &&
              tgt.get_device() == pred.get_device(),
              "restoration_metrics: tgt must match pred (contiguous fp32, "
              "same shape and device)");
  const int64_t P = pred.size(0), H = pred.size(1), W = pred.size(2);
  TORCH_CHECK(H >= METRIC_WIN && W >= METRIC_WIN,
              "restoration_metrics: H, W >= 7 required for the 7x7 SSIM "
              "window, got ", H, "x", W);
  TORCH_CHECK(H < (1 << 15) && W < (1 << 15),
              "restoration_metrics: H, W must be below 32768");
  const int64_t tilesX = (W + METRIC_TW - 1) / METRIC_TW;
  const int64_t tilesY = (H + METRIC_TH - 1) / METRIC_TH;
  const int64_t tiles = tilesX * tilesY;
  TORCH_CHECK(P <= 65535 && P * METRIC_COLS <= std::numeric_limits<int>::max(),
              "restoration_metrics: P exceeds the grid limit");
  auto opts = pred.options().dtype(at::kDouble);
  at::Tensor out = at::empty({P, METRIC_COLS}, opts);
  if (P == 0) return out;
  at::Tensor partial = at::empty({P, tiles, METRIC_COLS}, opts);
  const double C1 = (0.01 * data_range) * (0.01 * data_range);
  const double C2 = (0.03 * data_range) * (0.03 * data_range);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(restoration_metrics_tile_kernel,
                     dim3((unsigned)tiles, (unsigned)P), dim3(ESR_BLOCK), 0,
                     stream, (int)H, (int)W, (int)tilesX, C1, C2,
                     pred.data_ptr<float>(), tgt.data_ptr<float>(),
                     partial.data_ptr<double>());
  hipLaunchKernelGGL(restoration_metrics_finish_kernel,
                     dim3((unsigned)((P * METRIC_COLS + ESR_BLOCK - 1) /
                                     ESR_BLOCK)),
                     dim3(ESR_BLOCK), 0, stream, (int)P, (int)tiles,
                     partial.data_ptr<double>(), out.data_ptr<double>());
  return out;
}
