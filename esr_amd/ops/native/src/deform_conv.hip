// Modulated deformable convolution (DCNv2) for gfx950 / CDNA4.
//
// MI355X-native re-design of the op the reference implements in CUDA
// (ESR:models/DCNv2/src/cuda/dcn_v2_im2col_cuda.cu:125-327, host glue
// ESR:models/DCNv2/src/cuda/dcn_v2_cuda.cu:20-216).  Differences:
//   * batched end to end — one im2col + one batched GEMM (hipBLASLt via
//     at::bmm) for forward, and a fully batched backward; the reference
//     loops the backward per sample.
//   * grid-stride launches sized for 256 CUs / 8 XCDs, 256-thread blocks
//     (multiples of the 64-wide wavefront).
//   * fp32 compute; offsets/masks are read once per (group, tap, pixel)
//     and broadcast across the group's channels via the thread mapping
//     (channel is the slowest index, so the offset reads of neighbouring
//     threads coalesce and hit L2 for the channel repeats).
//   * backward: where a deformable group's input-grad planes fit in LDS
//     (cpg*H*W*4 B <= 64 KiB) one fused kernel, dcn_bwd_fused_kernel, sums
//     the input grad on chip and writes the offset and mask grads in the
//     same pass: no global atomics, no fp32 scratch, no cast.  Larger
//     planes keep the split path: col2im with global fp32 atomics
//     (LDS-tiled for fp32 3x3/s1/p1) + cast + col2im_coord.
//   * the forward can hand its im2col columns to the backward
//     (deform_conv2d_forward_cols / deform_conv2d_backward_cols), so the
//     weight-grad GEMM does not rebuild them.
//
// Layout (same convention as the reference kernels):
//   offset [B, dg*2*K, Ho, Wo]  (per group: 2k = h-offset, 2k+1 = w-offset)
//   mask   [B, dg*K,   Ho, Wo]
//   columns [B, C*K, Ho*Wo], column row = c*K + k.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "esr_common.h"

namespace {

// The four integer neighbours of a sample point, zero outside the image.
// This and the three functions below are the one definition of the
// boundary rules; every kernel in this file samples through them.
struct DcnCorners { float v00, v01, v10, v11; };

template <typename T>
ESR_INLINE DcnCorners load_corners(const T* __restrict__ im, int H, int W,
                                   int h0, int w0) {
  // Every corner is loaded, from index 0 where it lies outside, and
  // selected afterwards: a load under its own branch makes hipcc wait for
  // it before the next one is issued, and a kernel that samples per
  // channel then runs at one memory latency per corner.
  const bool top = h0 >= 0, bot = h0 + 1 < H;
  const bool lft = w0 >= 0, rgt = w0 + 1 < W;
  const int at = h0 * W + w0;
  const float a00 = esr_to_f32(im[top && lft ? at : 0]);
  const float a01 = esr_to_f32(im[top && rgt ? at + 1 : 0]);
  const float a10 = esr_to_f32(im[bot && lft ? at + W : 0]);
  const float a11 = esr_to_f32(im[bot && rgt ? at + W + 1 : 0]);
  DcnCorners v;
  v.v00 = top && lft ? a00 : 0.f;
  v.v01 = top && rgt ? a01 : 0.f;
  v.v10 = bot && lft ? a10 : 0.f;
  v.v11 = bot && rgt ? a11 : 0.f;
  return v;
}

// lh, lw: fractional parts of the sample coordinates
ESR_INLINE float bilinear_sample(const DcnCorners& v, float lh, float lw) {
  float hh = 1.f - lh, hw = 1.f - lw;
  return hh * hw * v.v00 + hh * lw * v.v01 + lh * hw * v.v10 + lh * lw * v.v11;
}

// gradient of bilinear_sample wrt the sample coordinates
ESR_INLINE float coord_grad_h(const DcnCorners& v, float lw) {
  return (v.v10 - v.v00) * (1.f - lw) + (v.v11 - v.v01) * lw;
}

ESR_INLINE float coord_grad_w(const DcnCorners& v, float lh) {
  return (v.v01 - v.v00) * (1.f - lh) + (v.v11 - v.v10) * lh;
}

// a sample at (h, w) touches the image at all
ESR_INLINE bool sample_in_range(float h, float w, int H, int W) {
  return h > -1 && w > -1 && h < H && w < W;
}

template <typename T>
ESR_INLINE float bilinear_sample(const T* __restrict__ im, int H, int W,
                                 float h, float w) {
  // zero-padded bilinear; caller guarantees sample_in_range(h, w, H, W)
  int h0 = (int)floorf(h);
  int w0 = (int)floorf(w);
  return bilinear_sample(load_corners(im, H, W, h0, w0), h - h0, w - w0);
}

template <typename T>
ESR_INLINE float coord_grad_h(const T* __restrict__ im, int H, int W,
                              float h, float w) {
  if (h <= -1 || w <= -1 || h >= H || w >= W) return 0.f;
  int h0 = (int)floorf(h);
  int w0 = (int)floorf(w);
  return coord_grad_h(load_corners(im, H, W, h0, w0), w - w0);
}

template <typename T>
ESR_INLINE float coord_grad_w(const T* __restrict__ im, int H, int W,
                              float h, float w) {
  if (h <= -1 || w <= -1 || h >= H || w >= W) return 0.f;
  int h0 = (int)floorf(h);
  int w0 = (int)floorf(w);
  return coord_grad_w(load_corners(im, H, W, h0, w0), h - h0);
}

struct DcnGeom {
  int B, C, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, dg, Ho, Wo;
};

// ---------------------------------------------------------------- im2col
template <typename T>
__global__ void dcn_im2col_kernel(
    long long n, const T* __restrict__ im,
    const T* __restrict__ offset, const T* __restrict__ mask,
    DcnGeom g, T* __restrict__ cols) {
  const int K = g.kh * g.kw;
  const int HoWo = g.Ho * g.Wo;
  const int cpg = g.C / g.dg;  // channels per deformable group
  ESR_KERNEL_LOOP(index, n) {
    // index -> (b, c, ho, wo); spatial fastest for coalesced col writes
    const int wo = index % g.Wo;
    const int ho = (index / g.Wo) % g.Ho;
    const int c = (index / HoWo) % g.C;
    const int b = index / ((long long)HoWo * g.C);
    const int grp = c / cpg;

    const T* im_p = im + ((long long)b * g.C + c) * g.H * g.W;
    const T* off_p = offset +
        ((long long)b * g.dg + grp) * 2 * K * HoWo;
    const T* msk_p = mask + ((long long)b * g.dg + grp) * K * HoWo;
    T* col_p = cols + (((long long)b * g.C + c) * K * HoWo)
        + ho * g.Wo + wo;

    const int h_in = ho * g.sh - g.ph;
    const int w_in = wo * g.sw - g.pw;
    const int pix = ho * g.Wo + wo;

    #pragma unroll 3
    for (int i = 0; i < g.kh; ++i) {
      for (int j = 0; j < g.kw; ++j) {
        const int k = i * g.kw + j;
        const float off_h = esr_to_f32(off_p[(2 * k) * HoWo + pix]);
        const float off_w = esr_to_f32(off_p[(2 * k + 1) * HoWo + pix]);
        const float m = esr_to_f32(msk_p[k * HoWo + pix]);
        const float h_im = h_in + i * g.dh + off_h;
        const float w_im = w_in + j * g.dw + off_w;
        // sampled without a branch (at the origin when the point is
        // outside), so the taps' loads can overlap
        const bool ok = sample_in_range(h_im, w_im, g.H, g.W);
        const float s = bilinear_sample(im_p, g.H, g.W, ok ? h_im : 0.f,
                                        ok ? w_im : 0.f);
        const float val = ok ? s : 0.f;
        col_p[(long long)k * HoWo] = esr_from_f32<T>(val * m);
      }
    }
  }
}

// --------------------------------------------------- col2im (LDS-tiled)
// grad wrt input for the 3x3/stride1/pad1 shape: one block per
// (b, c, 16x16 output tile).  Corner contributions that land inside the
// tile's input region (+/- HALO) accumulate via LDS float atomics and are
// flushed once per block (one global atomic per covered input pixel —
// ~16x fewer HBM atomics than the per-contribution kernel below); corners
// pushed outside by large learned offsets fall back to device-scope
// global atomics, so correctness never depends on the offset magnitude.
constexpr int C2I_TILE = 16;
constexpr int C2I_HALO = 4;
constexpr int C2I_EDGE = C2I_TILE + 2 * C2I_HALO;   // 24

template <typename T>
__global__ __launch_bounds__(256)
void dcn_col2im_tiled_kernel(
    const T* __restrict__ col_grad, const T* __restrict__ offset,
    const T* __restrict__ mask, DcnGeom g, float* __restrict__ grad_im) {
  const int K = g.kh * g.kw;            // 9
  const int HoWo = g.Ho * g.Wo;
  const int cpg = g.C / g.dg;

  const int tiles_x = (g.Wo + C2I_TILE - 1) / C2I_TILE;
  const int tiles_y = (g.Ho + C2I_TILE - 1) / C2I_TILE;
  const int tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C2I_TILE;
  const int tx0 = (tile % tiles_x) * C2I_TILE;
  const int c = blockIdx.y;
  const int b = blockIdx.z;
  const int grp = c / cpg;

  __shared__ float acc[C2I_EDGE * C2I_EDGE];
  for (int i = threadIdx.x; i < C2I_EDGE * C2I_EDGE; i += 256)
    acc[i] = 0.f;
  __syncthreads();

  const int px_local = threadIdx.x;                 // 256 = 16x16 tile
  const int ho = ty0 + px_local / C2I_TILE;
  const int wo = tx0 + px_local % C2I_TILE;
  float* gim = grad_im + ((long long)b * g.C + c) * g.H * g.W;

  if (ho < g.Ho && wo < g.Wo) {
    const int pix = ho * g.Wo + wo;
    const T* off_p = offset + ((long long)b * g.dg + grp) * 2 * K * HoWo;
    const T* msk_p = mask + ((long long)b * g.dg + grp) * K * HoWo;
    const T* cg_p = col_grad + (((long long)b * g.C + c) * K) * HoWo + pix;
    #pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int i = k / 3, j = k % 3;
      const float off_h = esr_to_f32(off_p[(2 * k) * HoWo + pix]);
      const float off_w = esr_to_f32(off_p[(2 * k + 1) * HoWo + pix]);
      const float m = esr_to_f32(msk_p[k * HoWo + pix]);
      const float h_im = ho - 1 + i + off_h;
      const float w_im = wo - 1 + j + off_w;
      if (h_im <= -1 || w_im <= -1 || h_im >= g.H || w_im >= g.W) continue;
      const float gval = esr_to_f32(cg_p[(long long)k * HoWo]) * m;
      const int h0 = (int)floorf(h_im);
      const int w0 = (int)floorf(w_im);
      const float lh = h_im - h0, lw = w_im - w0;
      const float wgt[4] = {(1 - lh) * (1 - lw), (1 - lh) * lw,
                            lh * (1 - lw), lh * lw};
      #pragma unroll
      for (int corner = 0; corner < 4; ++corner) {
        const int hh = h0 + (corner >> 1);
        const int ww = w0 + (corner & 1);
        if (hh < 0 || hh >= g.H || ww < 0 || ww >= g.W) continue;
        const int ly = hh - (ty0 - C2I_HALO);
        const int lx = ww - (tx0 - C2I_HALO);
        if (ly >= 0 && ly < C2I_EDGE && lx >= 0 && lx < C2I_EDGE)
          atomicAdd(&acc[ly * C2I_EDGE + lx], wgt[corner] * gval);
        else  // large-offset outlier: device-scope fallback
          atomicAdd(&gim[hh * g.W + ww], wgt[corner] * gval);
      }
    }
  }
  __syncthreads();
  // cooperative flush: one global atomic per covered input pixel.
  // Element order is permuted so consecutive LANES write addresses ~16
  // pixels apart — same-line atomics from one instruction serialize in L2
  // (measured 70-87%% of the conv wgrad kernel before the same fix).
  constexpr int NE = C2I_EDGE * C2I_EDGE;            // 576
  constexpr int COLS = NE / 16;                      // 36
  for (int i = threadIdx.x; i < NE; i += 256) {
    const int e = (i % COLS) * 16 + i / COLS;        // bijective remap
    const float v = acc[e];
    if (v != 0.f) {
      const int hh = ty0 - C2I_HALO + e / C2I_EDGE;
      const int ww = tx0 - C2I_HALO + e % C2I_EDGE;
      if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W)
        atomicAdd(&gim[hh * g.W + ww], v);
    }
  }
}

// ------------------------------------------------------------- col2im
// grad wrt input: distribute each column grad over its <=4 integer
// neighbours with bilinear weights; atomicAdd into grad_im (device scope).
template <typename T>
__global__ void dcn_col2im_kernel(
    long long n, const T* __restrict__ col_grad,
    const T* __restrict__ offset, const T* __restrict__ mask,
    DcnGeom g, float* __restrict__ grad_im) {
  const int K = g.kh * g.kw;
  const int HoWo = g.Ho * g.Wo;
  const int cpg = g.C / g.dg;
  ESR_KERNEL_LOOP(index, n) {
    // index -> (b, c, k, ho, wo)
    const int wo = index % g.Wo;
    const int ho = (index / g.Wo) % g.Ho;
    const int k = (index / HoWo) % K;
    const int c = (index / ((long long)HoWo * K)) % g.C;
    const int b = index / ((long long)HoWo * K * g.C);
    const int grp = c / cpg;
    const int i = k / g.kw, j = k % g.kw;
    const int pix = ho * g.Wo + wo;

    const T* off_p = offset + ((long long)b * g.dg + grp) * 2 * K * HoWo;
    const float off_h = esr_to_f32(off_p[(2 * k) * HoWo + pix]);
    const float off_w = esr_to_f32(off_p[(2 * k + 1) * HoWo + pix]);
    const float m =
        esr_to_f32(mask[(((long long)b * g.dg + grp) * K + k) * HoWo + pix]);

    const float h_im = ho * g.sh - g.ph + i * g.dh + off_h;
    const float w_im = wo * g.sw - g.pw + j * g.dw + off_w;
    if (h_im <= -1 || w_im <= -1 || h_im >= g.H || w_im >= g.W) continue;

    const float gval =
        esr_to_f32(col_grad[(((long long)b * g.C + c) * K + k) * HoWo + pix])
        * m;
    const int h0 = (int)floorf(h_im);
    const int w0 = (int)floorf(w_im);
    const float lh = h_im - h0, lw = w_im - w0;
    float* gim = grad_im + ((long long)b * g.C + c) * g.H * g.W;
    if (h0 >= 0 && w0 >= 0)
      atomicAdd(&gim[h0 * g.W + w0], (1 - lh) * (1 - lw) * gval);
    if (h0 >= 0 && w0 + 1 < g.W)
      atomicAdd(&gim[h0 * g.W + w0 + 1], (1 - lh) * lw * gval);
    if (h0 + 1 < g.H && w0 >= 0)
      atomicAdd(&gim[(h0 + 1) * g.W + w0], lh * (1 - lw) * gval);
    if (h0 + 1 < g.H && w0 + 1 < g.W)
      atomicAdd(&gim[(h0 + 1) * g.W + w0 + 1], lh * lw * gval);
  }
}

// -------------------------------------------------------- col2im_coord
// grad wrt offsets and mask: per (b, grp, k, ho, wo) reduce over the
// group's channels; plain stores (no atomics).
template <typename T>
__global__ void dcn_col2im_coord_kernel(
    long long n, const T* __restrict__ col_grad,
    const T* __restrict__ im, const T* __restrict__ offset,
    const T* __restrict__ mask, DcnGeom g,
    T* __restrict__ grad_offset, T* __restrict__ grad_mask) {
  const int K = g.kh * g.kw;
  const int HoWo = g.Ho * g.Wo;
  const int cpg = g.C / g.dg;
  ESR_KERNEL_LOOP(index, n) {
    // index -> (b, grp, k, ho, wo)
    const int wo = index % g.Wo;
    const int ho = (index / g.Wo) % g.Ho;
    const int k = (index / HoWo) % K;
    const int grp = (index / ((long long)HoWo * K)) % g.dg;
    const int b = index / ((long long)HoWo * K * g.dg);
    const int i = k / g.kw, j = k % g.kw;
    const int pix = ho * g.Wo + wo;

    const T* off_p = offset + ((long long)b * g.dg + grp) * 2 * K * HoWo;
    const float off_h = esr_to_f32(off_p[(2 * k) * HoWo + pix]);
    const float off_w = esr_to_f32(off_p[(2 * k + 1) * HoWo + pix]);
    const float m =
        esr_to_f32(mask[(((long long)b * g.dg + grp) * K + k) * HoWo + pix]);

    const float h_im = ho * g.sh - g.ph + i * g.dh + off_h;
    const float w_im = wo * g.sw - g.pw + j * g.dw + off_w;

    float gh = 0.f, gw = 0.f, gm = 0.f;
    const bool in_range = (h_im > -1 && w_im > -1 && h_im < g.H && w_im < g.W);
    for (int cc = 0; cc < cpg; ++cc) {
      const int c = grp * cpg + cc;
      const float cg =
          esr_to_f32(col_grad[(((long long)b * g.C + c) * K + k) * HoWo + pix]);
      const T* im_p = im + ((long long)b * g.C + c) * g.H * g.W;
      if (in_range) {
        gh += cg * m * coord_grad_h(im_p, g.H, g.W, h_im, w_im);
        gw += cg * m * coord_grad_w(im_p, g.H, g.W, h_im, w_im);
        gm += cg * bilinear_sample(im_p, g.H, g.W, h_im, w_im);
      }
    }
    T* goff = grad_offset + ((long long)b * g.dg + grp) * 2 * K * HoWo;
    goff[(2 * k) * HoWo + pix] = esr_from_f32<T>(gh);
    goff[(2 * k + 1) * HoWo + pix] = esr_from_f32<T>(gw);
    grad_mask[(((long long)b * g.dg + grp) * K + k) * HoWo + pix] =
        esr_from_f32<T>(gm);
  }
}

// ------------------------------------------- fused backward (LDS planes)
// grad wrt input, offsets and mask in one pass over col_grad: one block
// per (b, deformable group).  The group's cpg input-grad planes live in
// LDS as fp32 (cpg*H*W*4 B, dynamic, zeroed here), so every contribution
// is an add into LDS (lds_add_f32) and no global atomic is issued.  The
// plane is the whole image: no halo, no outlier fallback, any stride /
// dilation / kernel size.  Each (tap, pixel) decodes its offset, mask and
// bilinear weights once and reuses them for the group's channels; lanes
// run along wo, so smooth offsets give consecutive LDS addresses per add.
constexpr int DCN_BWD_FUSED_LDS_MAX = 64 * 1024;

// Float add into LDS by an integer compare-and-swap loop.  Measured on
// MI355X (profiles/README.md, DCN backward): the DS float add retires one
// lane at a time, about 204 G lane-adds/s over the whole chip whatever the
// addresses, which is slower than global float atomics; integer DS
// atomics run 32x faster.  The loop repeats only for lanes that lost a
// race for their address, so smooth offsets pass in one round.
ESR_INLINE void lds_add_f32(float* p, float v) {
  unsigned int* pi = reinterpret_cast<unsigned int*>(p);
  unsigned int seen = __hip_atomic_load(pi, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_WORKGROUP);
  unsigned int expect;
  do {
    expect = seen;
    seen = atomicCAS(pi, expect, __float_as_uint(__uint_as_float(expect) + v));
  } while (seen != expect);
}

template <typename T>
__global__ __launch_bounds__(256)
void dcn_bwd_fused_kernel(
    const T* __restrict__ col_grad, const T* __restrict__ im,
    const T* __restrict__ offset, const T* __restrict__ mask, DcnGeom g,
    T* __restrict__ grad_im, T* __restrict__ grad_offset,
    T* __restrict__ grad_mask) {
  extern __shared__ __attribute__((aligned(16))) float dcn_planes[];
  const int K = g.kh * g.kw;
  const int HoWo = g.Ho * g.Wo;
  const int HW = g.H * g.W;
  const int cpg = g.C / g.dg;
  const int plane_n = cpg * HW;
  // blockIdx.x = b * dg + grp; a group's channels are adjacent in memory
  const long long bg = blockIdx.x;

  for (int i = threadIdx.x; i < plane_n; i += 256) dcn_planes[i] = 0.f;
  __syncthreads();

  const T* off_p = offset + bg * 2 * K * HoWo;
  const T* msk_p = mask + bg * K * HoWo;
  const T* im_g = im + bg * plane_n;
  const T* cg_g = col_grad + bg * cpg * K * HoWo;
  T* goff = grad_offset + bg * 2 * K * HoWo;
  T* gmsk = grad_mask + bg * K * HoWo;

  for (int it = threadIdx.x; it < K * HoWo; it += 256) {
    const int k = it / HoWo, pix = it % HoWo;
    const int ho = pix / g.Wo, wo = pix % g.Wo;
    const int i = k / g.kw, j = k % g.kw;
    const float off_h = esr_to_f32(off_p[(2 * k) * HoWo + pix]);
    const float off_w = esr_to_f32(off_p[(2 * k + 1) * HoWo + pix]);
    const float m = esr_to_f32(msk_p[it]);
    const float h_im = ho * g.sh - g.ph + i * g.dh + off_h;
    const float w_im = wo * g.sw - g.pw + j * g.dw + off_w;

    float gh = 0.f, gw = 0.f, gm = 0.f;
    if (sample_in_range(h_im, w_im, g.H, g.W)) {
      const int h0 = (int)floorf(h_im);
      const int w0 = (int)floorf(w_im);
      const float lh = h_im - h0, lw = w_im - w0;
      const bool top = h0 >= 0, bot = h0 + 1 < g.H;
      const bool lft = w0 >= 0, rgt = w0 + 1 < g.W;
      const float w00 = (1 - lh) * (1 - lw), w01 = (1 - lh) * lw;
      const float w10 = lh * (1 - lw), w11 = lh * lw;
      const int at = h0 * g.W + w0;
      const T* cg_p = cg_g + k * HoWo + pix;
      // DCN_BWD_CH channels at a time: all their loads are issued before
      // the first LDS add (the adds sit under lane-divergent branches,
      // which loads are not moved across), so a chunk costs one memory
      // latency, not one per channel.  A chunk's tail past cpg re-reads
      // the last channel and is not used.
      constexpr int DCN_BWD_CH = 4;
      for (int c0 = 0; c0 < cpg; c0 += DCN_BWD_CH) {
        float cg[DCN_BWD_CH];
        DcnCorners v[DCN_BWD_CH];
        #pragma unroll
        for (int u = 0; u < DCN_BWD_CH; ++u) {
          const int cc = min(c0 + u, cpg - 1);
          cg[u] = esr_to_f32(cg_p[(long long)cc * K * HoWo]);
          v[u] = load_corners(im_g + cc * HW, g.H, g.W, h0, w0);
        }
        #pragma unroll
        for (int u = 0; u < DCN_BWD_CH; ++u) {
          if (c0 + u >= cpg) break;
          const float gval = cg[u] * m;
          float* pl = dcn_planes + (c0 + u) * HW + at;
          if (top && lft) lds_add_f32(&pl[0], w00 * gval);
          if (top && rgt) lds_add_f32(&pl[1], w01 * gval);
          if (bot && lft) lds_add_f32(&pl[g.W], w10 * gval);
          if (bot && rgt) lds_add_f32(&pl[g.W + 1], w11 * gval);
          gh += gval * coord_grad_h(v[u], lw);
          gw += gval * coord_grad_w(v[u], lh);
          gm += cg[u] * bilinear_sample(v[u], lh, lw);
        }
      }
    }
    goff[(2 * k) * HoWo + pix] = esr_from_f32<T>(gh);
    goff[(2 * k + 1) * HoWo + pix] = esr_from_f32<T>(gw);
    gmsk[it] = esr_from_f32<T>(gm);
  }
  __syncthreads();
  // one rounding from the fp32 sum, plain coalesced stores
  T* gi = grad_im + bg * plane_n;
  for (int i = threadIdx.x; i < plane_n; i += 256)
    gi[i] = esr_from_f32<T>(dcn_planes[i]);
}

// the rule of esr_amd/ops/dcn.py:dcn_bwd_fused_applicable
bool dcn_bwd_fused_fits(const DcnGeom& g) {
  return g.C % g.dg == 0 &&
         (long long)(g.C / g.dg) * g.H * g.W * 4 <= DCN_BWD_FUSED_LDS_MAX;
}

DcnGeom make_geom(const at::Tensor& input, const at::Tensor& weight,
                  int sh, int sw, int ph, int pw, int dh, int dw, int dg) {
  DcnGeom g;
  g.B = input.size(0); g.C = input.size(1);
  g.H = input.size(2); g.W = input.size(3);
  g.Cout = weight.size(0); g.kh = weight.size(2); g.kw = weight.size(3);
  g.sh = sh; g.sw = sw; g.ph = ph; g.pw = pw; g.dh = dh; g.dw = dw; g.dg = dg;
  g.Ho = (g.H + 2 * ph - (dh * (g.kh - 1) + 1)) / sh + 1;
  g.Wo = (g.W + 2 * pw - (dw * (g.kw - 1) + 1)) / sw + 1;
  return g;
}

// fp32, bf16 or fp16 (fp32 compute inside either way)
#define DISPATCH_DCN_DTYPE(TEN, ...)                                   \
  [&] {                                                                \
    if ((TEN).scalar_type() == at::kFloat) {                           \
      using scalar_t = float;                                          \
      return __VA_ARGS__();                                            \
    }                                                                  \
    if ((TEN).scalar_type() == at::kHalf) {                            \
      using scalar_t = __half;                                         \
      return __VA_ARGS__();                                            \
    }                                                                  \
    TORCH_CHECK((TEN).scalar_type() == at::kBFloat16,                  \
                "deform_conv2d: fp32, bf16 or fp16 required");         \
    using scalar_t = __hip_bfloat16;                                   \
    return __VA_ARGS__();                                              \
  }()

at::Tensor dcn_im2col(const at::Tensor& input, const at::Tensor& offset,
                      const at::Tensor& mask, const DcnGeom& g) {
  auto cols = at::empty({g.B, g.C * g.kh * g.kw, g.Ho * g.Wo},
                        input.options());
  long long n = (long long)g.B * g.C * g.Ho * g.Wo;
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_DCN_DTYPE(input, [&] {
    hipLaunchKernelGGL((dcn_im2col_kernel<scalar_t>), dim3(esr_grid(n)),
                       dim3(ESR_BLOCK), 0, stream, n,
                       (const scalar_t*)input.data_ptr(),
                       (const scalar_t*)offset.data_ptr(),
                       (const scalar_t*)mask.data_ptr(), g,
                       (scalar_t*)cols.data_ptr());
    return 0;
  });
  return cols;
}

// grad wrt input on the split path (global fp32 atomics; LDS-tiled variant
// for the 3x3/s1/p1 shape; ESR_DCN_TILED=0/1 forces either kernel for A/B
// timing).  Default is dtype-dependent: fp32 measured 3.0x faster TILED
// (r1 microbench); bf16 measured faster UNTILED (whole-step A/B, +1.8%:
// the bf16 col-grad reads halve the per-contribution kernel's traffic
// while the tiled kernel stays LDS-atomic-bound).  fp16 has bf16's element
// size and takes the same (untiled) default; not measured separately.
at::Tensor dcn_col2im_split(const at::Tensor& input, const at::Tensor& offset,
                            const at::Tensor& mask, const at::Tensor& col_grad,
                            const DcnGeom& g) {
  static const int tiled_env = [] {
    const char* e = getenv("ESR_DCN_TILED");
    return e == nullptr ? -1 : (e[0] != '0');
  }();
  const bool use_tiled = tiled_env >= 0
      ? tiled_env != 0 : input.scalar_type() == at::kFloat;
  const int K = g.kh * g.kw;
  auto stream = at::hip::getCurrentHIPStream();
  // atomics accumulate in fp32 regardless of the op dtype
  auto grad_input_f = at::zeros(input.sizes(), input.options()
                                                   .dtype(at::kFloat));
  DISPATCH_DCN_DTYPE(input, [&] {
    if (use_tiled && g.kh == 3 && g.kw == 3 && g.sh == 1 && g.sw == 1 &&
        g.ph == 1 && g.pw == 1 && g.dh == 1 && g.dw == 1) {
      const int tiles = ((g.Ho + C2I_TILE - 1) / C2I_TILE) *
                        ((g.Wo + C2I_TILE - 1) / C2I_TILE);
      hipLaunchKernelGGL((dcn_col2im_tiled_kernel<scalar_t>),
                         dim3(tiles, g.C, g.B), dim3(256), 0, stream,
                         (const scalar_t*)col_grad.data_ptr(),
                         (const scalar_t*)offset.data_ptr(),
                         (const scalar_t*)mask.data_ptr(), g,
                         grad_input_f.data_ptr<float>());
    } else {
      long long n = (long long)g.B * g.C * K * g.Ho * g.Wo;
      hipLaunchKernelGGL((dcn_col2im_kernel<scalar_t>), dim3(esr_grid(n)),
                         dim3(ESR_BLOCK), 0, stream, n,
                         (const scalar_t*)col_grad.data_ptr(),
                         (const scalar_t*)offset.data_ptr(),
                         (const scalar_t*)mask.data_ptr(), g,
                         grad_input_f.data_ptr<float>());
    }
    return 0;
  });
  return input.scalar_type() == at::kFloat
      ? grad_input_f : grad_input_f.to(input.scalar_type());
}

bool dcn_dtype_ok(const at::Tensor& t) {
  return t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16 ||
         t.scalar_type() == at::kHalf;
}

// the kernels reinterpret every operand as input's element type
void dcn_check_same_dtype(const at::Tensor& input, const at::Tensor& offset,
                          const at::Tensor& mask, const at::Tensor& weight) {
  TORCH_CHECK(offset.scalar_type() == input.scalar_type() &&
              mask.scalar_type() == input.scalar_type() &&
              weight.scalar_type() == input.scalar_type(),
              "deform_conv2d: input/offset/mask/weight dtypes differ (",
              input.scalar_type(), ", ", offset.scalar_type(), ", ",
              mask.scalar_type(), ", ", weight.scalar_type(), ")");
}

}  // namespace

// deform_conv_fused.hip
bool dcn_fused_applicable(const at::Tensor&, const at::Tensor&, int64_t,
                          int64_t, int64_t, int64_t, int64_t, int64_t,
                          int64_t);
at::Tensor deform_conv2d_forward_fused(
    const at::Tensor&, const at::Tensor&, const at::Tensor&,
    const at::Tensor&, const c10::optional<at::Tensor>&, int64_t);

// conv2d.hip
std::vector<at::Tensor> bias_grad(const at::Tensor&, bool);

namespace {

DcnGeom dcn_forward_geom(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    const at::Tensor& weight, int sh, int sw, int ph, int pw, int dh, int dw,
    int dg) {
  TORCH_CHECK(input.is_cuda() && dcn_dtype_ok(input),
              "deform_conv2d: fp32/bf16/fp16 CUDA tensors required, got ",
              input.scalar_type());
  dcn_check_same_dtype(input, offset, mask, weight);
  TORCH_CHECK(input.is_contiguous() && offset.is_contiguous() &&
              mask.is_contiguous() && weight.is_contiguous());
  auto g = make_geom(input, weight, sh, sw, ph, pw, dh, dw, dg);
  TORCH_CHECK(offset.size(1) == g.dg * 2 * g.kh * g.kw, "offset channels");
  TORCH_CHECK(mask.size(1) == g.dg * g.kh * g.kw, "mask channels");
  TORCH_CHECK(g.C % g.dg == 0, "C % deformable_groups != 0");
  return g;
}

}  // namespace

// im2col + GEMM forward that also hands back the columns [B, C*K, Ho*Wo]:
// the weight-grad GEMM of the backward needs exactly these, so a caller
// that keeps them saves the backward a second im2col.
std::vector<at::Tensor> deform_conv2d_forward_cols(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    const at::Tensor& weight, const c10::optional<at::Tensor>& bias,
    int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
    int64_t dg) {
  auto g = dcn_forward_geom(input, offset, mask, weight, sh, sw, ph, pw, dh,
                            dw, dg);
  auto cols = dcn_im2col(input, offset, mask, g);
  // one batched GEMM: [B, Cout, C*K] x [B, C*K, HoWo]
  auto w2d = weight.reshape({g.Cout, g.C * g.kh * g.kw});
  auto out = at::matmul(w2d, cols);  // broadcasts over B -> [B, Cout, HoWo]
  out = out.reshape({g.B, g.Cout, g.Ho, g.Wo});
  if (bias.has_value() && bias->defined())
    out = out + bias->reshape({1, g.Cout, 1, 1});
  return {out, cols};
}

at::Tensor deform_conv2d_forward(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    const at::Tensor& weight, const c10::optional<at::Tensor>& bias,
    int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
    int64_t dg) {
  dcn_forward_geom(input, offset, mask, weight, sh, sw, ph, pw, dh, dw, dg);

  // Measured on gfx950 at the flagship shape (tools/bench_dcn.py,
  // profiles/README.md): split im2col + hipBLASLt GEMM 0.46 ms vs fused
  // im2col+MFMA 0.52 ms — the fused kernel's on-the-fly sampling is not
  // hidden behind its MFMAs (hipcc drains the sampling loads at their
  // immediate use).  Default to the faster split path; ESR_DCN_FUSED=1
  // selects the fused kernel (numerics-equal, no column buffer in HBM).
  static const bool use_fused = [] {
    const char* e = getenv("ESR_DCN_FUSED");
    return e != nullptr && e[0] == '1';
  }();
  if (use_fused && input.scalar_type() == at::kFloat &&
      dcn_fused_applicable(input, weight, sh, sw, ph, pw, dh, dw, dg))
    return deform_conv2d_forward_fused(input, offset, mask, weight, bias, dg);

  return deform_conv2d_forward_cols(input, offset, mask, weight, bias, sh, sw,
                                    ph, pw, dh, dw, dg)[0];
}

// Backward.  `cols` are the forward's columns when the caller kept them
// (deform_conv2d_forward_cols); without them the im2col runs again.
// `path` picks the kernels for the input / offset / mask grads:
//   "fused"  dcn_bwd_fused_kernel; an error where the group's planes do
//            not fit in LDS (dcn_bwd_fused_fits)
//   "split"  col2im (atomics) + fp32 scratch + cast + col2im_coord
//   "auto"   fused where it fits, else split
// Measured at the flagship shape (bf16, B=768, C=64, 32x32, dg=8): see
// profiles/README.md, DCN backward.
std::vector<at::Tensor> deform_conv2d_backward_cols(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    const at::Tensor& weight, const at::Tensor& grad_out,
    const c10::optional<at::Tensor>& cols_saved,
    int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
    int64_t dg, const std::string& path) {
  TORCH_CHECK(input.is_contiguous() && offset.is_contiguous() &&
              mask.is_contiguous() && weight.is_contiguous() &&
              grad_out.is_contiguous(),
              "deform_conv2d_backward: contiguous tensors required");
  TORCH_CHECK(input.is_cuda() && dcn_dtype_ok(input),
              "deform_conv2d_backward: fp32/bf16/fp16 CUDA tensors required, "
              "got ", input.scalar_type());
  dcn_check_same_dtype(input, offset, mask, weight);
  TORCH_CHECK(grad_out.scalar_type() == input.scalar_type(),
              "deform_conv2d_backward: grad_out is ", grad_out.scalar_type(),
              " but input is ", input.scalar_type());
  auto g = make_geom(input, weight, sh, sw, ph, pw, dh, dw, dg);
  const int K = g.kh * g.kw;
  auto stream = at::hip::getCurrentHIPStream();

  auto go2d = grad_out.reshape({g.B, g.Cout, g.Ho * g.Wo});
  auto w2d = weight.reshape({g.Cout, g.C * K});

  TORCH_CHECK(g.C % g.dg == 0, "C % deformable_groups != 0");
  TORCH_CHECK(path == "auto" || path == "fused" || path == "split",
              "deform_conv2d_backward: path must be auto, fused or split, "
              "got '", path, "'");
  const bool fits = dcn_bwd_fused_fits(g);
  TORCH_CHECK(path != "fused" || fits,
              "deform_conv2d_backward: the fused path keeps a deformable "
              "group's input-grad planes in LDS and needs (C/dg)*H*W*4 B <= ",
              DCN_BWD_FUSED_LDS_MAX, "; got ",
              (long long)(g.C / g.dg) * g.H * g.W * 4,
              " B (use path=auto or split)");
  const bool use_fused = path == "fused" || (path == "auto" && fits);

  // grad wrt columns: [B, C*K, HoWo] = W^T [C*K, Cout] x go2d (batched)
  auto col_grad = at::matmul(w2d.t(), go2d).contiguous();

  at::Tensor grad_input;
  auto grad_offset = at::empty_like(offset);
  auto grad_mask = at::empty_like(mask);
  if (use_fused) {
    grad_input = at::empty_like(input);
    const size_t lds = (size_t)(g.C / g.dg) * g.H * g.W * sizeof(float);
    DISPATCH_DCN_DTYPE(input, [&] {
      hipLaunchKernelGGL((dcn_bwd_fused_kernel<scalar_t>),
                         dim3(g.B * g.dg), dim3(256), lds, stream,
                         (const scalar_t*)col_grad.data_ptr(),
                         (const scalar_t*)input.data_ptr(),
                         (const scalar_t*)offset.data_ptr(),
                         (const scalar_t*)mask.data_ptr(), g,
                         (scalar_t*)grad_input.data_ptr(),
                         (scalar_t*)grad_offset.data_ptr(),
                         (scalar_t*)grad_mask.data_ptr());
      return 0;
    });
  } else {
    grad_input = dcn_col2im_split(input, offset, mask, col_grad, g);
    DISPATCH_DCN_DTYPE(input, [&] {
      long long n = (long long)g.B * g.dg * K * g.Ho * g.Wo;
      hipLaunchKernelGGL((dcn_col2im_coord_kernel<scalar_t>),
                         dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream, n,
                         (const scalar_t*)col_grad.data_ptr(),
                         (const scalar_t*)input.data_ptr(),
                         (const scalar_t*)offset.data_ptr(),
                         (const scalar_t*)mask.data_ptr(), g,
                         (scalar_t*)grad_offset.data_ptr(),
                         (scalar_t*)grad_mask.data_ptr());
      return 0;
    });
  }

  // grad weight / bias via batched GEMM (the reference loops per sample,
  // ESR:models/DCNv2/src/cuda/dcn_v2_cuda.cu:150)
  at::Tensor cols;
  if (cols_saved.has_value() && cols_saved->defined()) {
    cols = *cols_saved;
    TORCH_CHECK(cols.is_contiguous() && cols.dim() == 3 &&
                cols.size(0) == g.B && cols.size(1) == g.C * K &&
                cols.size(2) == g.Ho * g.Wo &&
                cols.scalar_type() == input.scalar_type(),
                "deform_conv2d_backward: saved columns do not match");
  } else {
    cols = dcn_im2col(input, offset, mask, g);
  }
  auto grad_weight = at::bmm(go2d, cols.transpose(1, 2)).sum(0)
                         .reshape(weight.sizes());
  // 16-bit: the conv bias-grad kernels (conv2d.hip, deterministic two-stage
  // sum); fp32 keeps torch's reduction
  const bool g16 = grad_out.scalar_type() == at::kBFloat16 ||
                   grad_out.scalar_type() == at::kHalf;
  auto grad_bias = g16 ? bias_grad(grad_out.contiguous(), false)[0]
                       : grad_out.sum(at::IntArrayRef{0, 2, 3});

  return {grad_input, grad_offset, grad_mask, grad_weight, grad_bias};
}

std::vector<at::Tensor> deform_conv2d_backward(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    const at::Tensor& weight, const at::Tensor& grad_out,
    int64_t sh, int64_t sw, int64_t ph, int64_t pw, int64_t dh, int64_t dw,
    int64_t dg) {
  return deform_conv2d_backward_cols(input, offset, mask, weight, grad_out,
                                     c10::nullopt, sh, sw, ph, pw, dh, dw, dg,
                                     "auto");
}

at::Tensor deform_im2col_debug(
    const at::Tensor& input, const at::Tensor& offset, const at::Tensor& mask,
    int64_t kh, int64_t kw, int64_t sh, int64_t sw, int64_t ph, int64_t pw,
    int64_t dh, int64_t dw, int64_t dg) {
  auto weight = at::empty({1, input.size(1), kh, kw}, input.options());
  auto g = make_geom(input, weight, sh, sw, ph, pw, dh, dw, dg);
  return dcn_im2col(input, offset, mask, g);
}
