// Hand-written gfx950 (CDNA4) direct convolution kernels, bf16/fp16 NCHW.
//
// Replaces the MIOpen conv + NCHW<->NHWC batched_transpose + autocast cast
// chain for the shapes ESRNet actually runs (3x3 s1/s2 p1 and 1x1 convs at
// C in {2..192}, reference ConvLayer ESR:models/submodules.py:159-200 and
// ConvGRU convs :474-514): 16-bit-native in/out, fp32 accumulate, fused
// bias + ReLU/sigmoid/tanh epilogues, no layout round trips.
//
// Element types: the forward kernels, act_grad and the fragment probe are
// templated on a small trait (ElemBf16 / ElemFp16: 16-bit load -> float,
// float -> 16-bit store, MFMA builtin).  Storage is raw 16-bit either way,
// so tiles, LDS layout and vector stores are shared; the host wrappers
// dispatch on x.scalar_type() and reject mixed bf16/fp16 operands.  The
// backward-only kernels (dgrad_s2, wgrad) are bf16-only and say so.
//
// Forward paths, picked by the host by shape:
//   * MFMA implicit GEMM (mfma_f32_16x16x32_bf16 / _f16): M = Cout tile (32/64),
//     N = 64 output pixels (2 rows x 32 cols), K = Cin in chunks of 32,
//     3x3 taps looped outside K.  The input patch is staged in LDS in a
//     pixel-major / channel-contiguous layout (40-short slots = 80 B so
//     ds_read_b128 lane groups hit distinct banks; guide §2/G4), weights
//     are read as packed [tap][Cout_p][Cin_p] fragments straight from L2.
//   * VALU direct kernel for bandwidth-bound small-channel shapes
//     (Cin small or Cout < 16 where MFMA tiles would idle).
//
//   * stride-1 deep class (3x3 / 1x1, >= 32 channels in and out): the
//     8x32-tile core conv2d_s1_core_kernel, forward and input grad.
//
// Backward: the stride-1 input-grad IS the forward with the weights read
// flipped and transposed (by the core's pack kernel; for Cin < 32 by the
// VALU kernel on a host-side copy); stride-2 input-grad has a dedicated
// scatter-form VALU kernel; stride-1 weight-grad is the MFMA kernel with
// a DETERMINISTIC two-stage reduction (conv2d_wgrad_s1_kernel below) whose
// second stage writes dW [Cout, Cin, k, k] bf16, stride-2 weight-grad the
// older per-row-tile variant with transposed line-parallel atomics.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include "esr_common.h"

namespace {

using s16x8 = __attribute__((ext_vector_type(8))) short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int TW = 32;    // output-pixel tile cols
constexpr int TH = 2;     // output-pixel tile rows
constexpr int CIK = 32;   // input channels per K chunk
constexpr int SLOT = 40;  // shorts per pixel slot (32 ci + 8 pad = 80 B:
                          // 20-dword stride, gcd(20,64)=4 -> the 16-lane
                          // ds_read_b128 groups see 16 distinct banks)

template <int ACT> ESR_INLINE float apply_act(float v);
template <> ESR_INLINE float apply_act<0>(float v) { return v; }
template <> ESR_INLINE float apply_act<1>(float v) { return v > 0.f ? v : 0.f; }
template <> ESR_INLINE float apply_act<2>(float v) { return esr_sigmoid(v); }
template <> ESR_INLINE float apply_act<3>(float v) { return tanhf(v); }

ESR_INLINE float bf16u_to_f(ushort u) {
  unsigned int x = (unsigned int)u << 16;
  return __uint_as_float(x);
}
ESR_INLINE ushort f_to_bf16u(float f) {
  // round-to-nearest-even, matching torch's float->bf16 cast
  unsigned int x = __float_as_uint(f);
  unsigned int lsb = (x >> 16) & 1;
  x += 0x7fffu + lsb;
  return (ushort)(x >> 16);
}

// Element traits: storage is raw 16-bit (ushort) for both types, so the LDS
// slot layout, staging loops and vector stores are shared; only the
// load/store conversions and the MFMA builtin differ.  The C/D fragment
// layout of mfma_f32_16x16x32 is dtype-independent (guide §3).
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;

struct ElemBf16 {
  static ESR_INLINE float to_f(ushort u) { return bf16u_to_f(u); }
  static ESR_INLINE ushort from_f(float f) { return f_to_bf16u(f); }
  static ESR_INLINE f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

struct ElemFp16 {
  static ESR_INLINE float to_f(ushort u) {
    return (float)__builtin_bit_cast(_Float16, u);
  }
  static ESR_INLINE ushort from_f(float f) {
    // v_cvt_f16_f32: round-to-nearest-even, overflow -> +/-inf, subnormals
    // kept — the same result as torch's float->half cast
    return __builtin_bit_cast(ushort, (_Float16)f);
  }
  static ESR_INLINE f32x4 mfma(s16x8 a, s16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(
        __builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
        0, 0, 0);
  }
};

// ---------------------------------------------------------------------------
// MFMA forward: one block = [32*MREP cout] x [64 pixels] for one frame.
// Wave grid 2(M) x 2(N); per wave MREP m-frags x 2 n-frags of 16x16.
// ---------------------------------------------------------------------------

template <typename E, int KS, int STRIDE, int ACT, int MREP>
__global__ __launch_bounds__(256)
void conv2d_fwd_mfma_kernel(
    const ushort* __restrict__ x,      // [B, Cin, H, W] bf16/fp16
    const ushort* __restrict__ wp,     // [KS*KS, Cout_p, Cin_p] packed, same
    const float* __restrict__ bias,    // [Cout] fp32 or nullptr
    ushort* __restrict__ y,            // [B, Cout, Ho, Wo] same as x
    int Cin, int H, int W, int Cout, int Ho, int Wo,
    int Cin_p, int Cout_p, int ntx) {
  constexpr int PH = STRIDE * TH + (KS - 1);
  constexpr int PW = STRIDE * TW + (KS - 1);
  constexpr int PAD = KS / 2;
  __shared__ ushort patch[PH * PW * SLOT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  const int ty0 = (blockIdx.x / ntx) * TH;
  const int tx0 = (blockIdx.x % ntx) * TW;
  const int b = blockIdx.y;
  const int co0 = blockIdx.z * (32 * MREP);

  const long long x_b = (long long)b * Cin * H * W;
  const long long plane = (long long)H * W;
  const int in_y0 = ty0 * STRIDE - PAD;
  const int in_x0 = tx0 * STRIDE - PAD;

  f32x4 acc[MREP][2] = {};

  const int kgrp = (lane >> 4) * 8;  // k-offset of this lane's fragment rows
  const int nchunks = Cin_p / CIK;
  for (int ck = 0; ck < nchunks; ++ck) {
    const int ci0 = ck * CIK;
    if (ck) __syncthreads();
    // ---- stage: thread <-> patch pixel; 32 plane-strided reads per pixel
    // are wave-coalesced (consecutive threads read consecutive ix of the
    // same channel plane); 4x ds_write_b128 per pixel, conflict-free slots.
    for (int p = tid; p < PH * PW; p += 256) {
      const int py = p / PW, px = p % PW;
      const int iy = in_y0 + py, ix = in_x0 + px;
      ushort vals[CIK];
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
        const ushort* src = x + x_b + ci0 * plane + (long long)iy * W + ix;
        const int cmax = Cin - ci0;  // >= 1 here (ci0 < Cin or full pad)
#pragma unroll
        for (int c = 0; c < CIK; ++c)
          vals[c] = (c < cmax) ? src[c * plane] : (ushort)0;
      } else {
#pragma unroll
        for (int c = 0; c < CIK; ++c) vals[c] = 0;
      }
#pragma unroll
      for (int v = 0; v < CIK / 8; ++v)
        *reinterpret_cast<s16x8*>(&patch[p * SLOT + v * 8]) =
            *reinterpret_cast<const s16x8*>(&vals[v * 8]);
    }
    __syncthreads();

    // ---- MFMA: 9 (or 1) taps x MREP x 2 fragments per wave per chunk
#pragma unroll
    for (int tap = 0; tap < KS * KS; ++tap) {
      const int ky = tap / KS, kx = tap % KS;
      s16x8 a[MREP];
#pragma unroll
      for (int m = 0; m < MREP; ++m) {
        // the last cout block may reach past Cout_p (216 -> 224 packed
        // rows, blocks of 64): clamp, or the load runs off the end of wp;
        // those rows' results are dropped by the co >= Cout test below
        int row = co0 + wm * 16 * MREP + m * 16 + (lane & 15);
        row = row < Cout_p ? row : Cout_p - 1;
        a[m] = *reinterpret_cast<const s16x8*>(
            &wp[((long long)tap * Cout_p + row) * Cin_p + ci0 + kgrp]);
      }
#pragma unroll
      for (int nf = 0; nf < 2; ++nf) {
        const int pidx = wn * 32 + nf * 16 + (lane & 15);
        const int py = (pidx >> 5) * STRIDE + ky;
        const int px = (pidx & 31) * STRIDE + kx;
        const s16x8 bfrag = *reinterpret_cast<const s16x8*>(
            &patch[(py * PW + px) * SLOT + kgrp]);
#pragma unroll
        for (int m = 0; m < MREP; ++m)
          acc[m][nf] = E::mfma(a[m], bfrag, acc[m][nf]);
      }
    }
  }

  // ---- epilogue: bias + activation fused, 16-bit stores
  // D layout (guide §3): col = lane&15 (pixel), row = (lane>>4)*4 + j (cout)
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
#pragma unroll
    for (int nf = 0; nf < 2; ++nf) {
      const int pidx = wn * 32 + nf * 16 + (lane & 15);
      const int oy = ty0 + (pidx >> 5), ox = tx0 + (pidx & 31);
      if (oy >= Ho || ox >= Wo) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = co0 + wm * 16 * MREP + m * 16 + (lane >> 4) * 4 + j;
        if (co >= Cout) continue;
        float v = acc[m][nf][j];
        if (bias) v += bias[co];
        v = apply_act<ACT>(v);
        y[(((long long)b * Cout + co) * Ho + oy) * Wo + ox] = E::from_f(v);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Stride-1 MFMA core for the deep class (3x3 pad 1 and 1x1, K >= 32 input
// and M >= 32 output channels): the stride-1 input grad, and offered to the
// forward (conv2d_s1 below).
//
//   block tile: 8 rows x 32 cols of output pixels x up to 16*MC channels,
//   wave grid 2 (channel halves) x 2 (rows 0-3 / 4-7); the MFMA's M rows are
//   PIXELS and its N columns output channels, so one lane ends up with four
//   neighbouring pixels of one channel.
//
// Against conv2d_fwd_mfma_kernel:
//   * staging reads 16 bytes along W (8 pixels) per load, 8 channels per
//     thread, and transposes the 8x8 block in registers into the same
//     pixel-major 80-byte slots; rows that are not 16-byte aligned
//     (W % 8 != 0) and partial groups take element loads.  The two halo
//     columns are staged by otherwise idle threads (160 + 80 of 256 busy at
//     3x3), and the 10-row patch is read once for ALL output channels of the
//     block (halo amplification 1.25x, no re-staging per 64-channel block;
//     M is split over blockIdx.z only above 128 channels, where the
//     accumulators no longer fit);
//   * two patch buffers: the global loads of chunk k+1 are issued before the
//     MFMAs of chunk k and written to the other buffer after them, one
//     barrier per chunk, 72*MC MFMAs per wave between barriers (36 before);
//   * the epilogue swaps 8 bytes between lane pairs 16 apart and stores 16
//     bytes (8 pixels) per lane, 64-byte runs per channel row.
// Accumulation order per output element (chunk-major, then tap, then the
// MFMA's own 32 channels) is that of conv2d_fwd_mfma_kernel.
// Weights: conv2d_pack_w_kernel writes [tap][Mp][Kp] once per call, zero
// padded to the block grid (no row clamp here); for the input grad it reads
// w[co][ci][KS-1-ky][KS-1-kx] in place, so no flipped or transposed copy is
// made on the host side.
// ---------------------------------------------------------------------------

constexpr int C_TH = 8;   // output rows per block tile

ESR_INLINE float apply_act_rt(float v, int act) {
  switch (act) {   // uniform across the grid
    case 1: return apply_act<1>(v);
    case 2: return apply_act<2>(v);
    case 3: return apply_act<3>(v);
    default: return v;
  }
}

__global__ void conv2d_pack_w_kernel(
    long long n, const ushort* __restrict__ w,   // [O, I, KS, KS]
    ushort* __restrict__ wp,                     // [KS*KS, Mp, Kp]
    int O, int I, int KS, int Mp, int Kp, int dgrad) {
  ESR_KERNEL_LOOP(i, n) {
    const int k = (int)(i % Kp);
    const int m = (int)((i / Kp) % Mp);
    const int tap = (int)(i / ((long long)Kp * Mp));
    const int ky = tap / KS, kx = tap % KS;
    const int o = dgrad ? k : m, ci = dgrad ? m : k;
    const int sy = dgrad ? KS - 1 - ky : ky, sx = dgrad ? KS - 1 - kx : kx;
    wp[i] = (o < O && ci < I)
        ? w[(((long long)o * I + ci) * KS + sy) * KS + sx] : (ushort)0;
  }
}

template <typename E, int KS, int MC>
__global__ __launch_bounds__(256, 2)   // 2 waves/SIMD: two blocks per CU
void conv2d_s1_core_kernel(
    const ushort* __restrict__ x,      // [B, Cin, H, W]
    const ushort* __restrict__ wp,     // [KS*KS, Mp, Kp] from conv2d_pack_w
    const float* __restrict__ bias,    // [Cout] fp32 or nullptr
    ushort* __restrict__ y,            // [B, Cout, H, W]
    int Cin, int H, int W, int Cout, int Kp, int Mp, int ntx, int act,
    int valign) {   // valign: W % 8 == 0 and both bases 16-byte aligned
  constexpr int PAD = KS / 2;
  constexpr int PH = C_TH + 2 * PAD;       // patch rows
  constexpr int PWC = TW + 2 * PAD;        // patch cols
  constexpr int MCW = MC / 2;              // channel fragments per wave
  constexpr int BUF = PH * PWC * SLOT;     // shorts per patch buffer
  constexpr int NV = PH * 4 * 4;           // 8ch x 8px vector staging units
  constexpr int NHALO = PAD ? PH * 4 * 2 : 0;  // 8ch x 1px halo units
  static_assert(NV + NHALO <= 256, "one staging unit per thread");
  __shared__ __attribute__((aligned(16))) ushort patch[2 * BUF];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l15 = lane & 15, lg = lane >> 4;

  const int ty0 = (blockIdx.x / ntx) * C_TH;
  const int tx0 = (blockIdx.x % ntx) * TW;
  const int b = blockIdx.y;
  const int co0 = blockIdx.z * (16 * MC);

  const long long plane = (long long)H * W;
  const ushort* xb = x + (long long)b * Cin * plane;

  // this thread's staging unit (fixed over the chunks)
  const bool is_vec = tid < NV;
  const bool is_halo = !is_vec && tid < NV + NHALO;
  int u_row, u_cg, u_px;   // patch row, 8-channel group, first pixel (global)
  int u_col;               // patch column of the unit's first pixel
  if (is_vec) {
    const int g = tid & 3;
    u_row = (tid >> 2) % PH;
    u_cg = tid / (4 * PH);
    u_px = tx0 + g * 8;
    u_col = PAD + g * 8;
  } else {
    const int h = tid - NV;
    const int side = h & 1;
    u_row = (h >> 1) % PH;
    u_cg = (h >> 1) / PH;
    u_px = side ? tx0 + TW : tx0 - 1;
    u_col = side ? PWC - 1 : 0;
  }
  const int u_iy = ty0 - PAD + u_row;
  const bool u_row_ok = u_iy >= 0 && u_iy < H;
  const bool u_vec_ok = valign && u_px + 8 <= W;
  const ushort* u_src = xb + (long long)u_iy * W + u_px;

  s16x8 pre[8];   // vector unit: pre[channel][pixel]; halo unit: pre[0][ch]

  auto load_chunk = [&](int ci0) {
    if (is_vec) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ci0 + u_cg * 8 + j;
        s16x8 v = {};
        if (c < Cin && u_row_ok) {
          const ushort* src = u_src + c * plane;
          if (u_vec_ok) {
            v = *reinterpret_cast<const s16x8*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              v[e] = (u_px + e < W) ? (short)src[e] : (short)0;
          }
        }
        pre[j] = v;
      }
    } else if (is_halo) {
      s16x8 v = {};
      if (u_row_ok && u_px >= 0 && u_px < W) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int c = ci0 + u_cg * 8 + j;
          v[j] = (c < Cin) ? (short)u_src[c * plane] : (short)0;
        }
      }
      pre[0] = v;
    }
  };

  auto store_chunk = [&](ushort* buf) {
    ushort* dst = buf + (u_row * PWC + u_col) * SLOT + u_cg * 8;
    if (is_vec) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        s16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = pre[j][e];
        *reinterpret_cast<s16x8*>(dst + e * SLOT) = v;
      }
    } else if (is_halo) {
      *reinterpret_cast<s16x8*>(dst) = pre[0];
    }
  };

  f32x4 acc[8][MCW] = {};
  const int kgrp = lg * 8;
  const int nchunks = Kp / CIK;

  load_chunk(0);
  store_chunk(patch);
  for (int ck = 0; ck < nchunks; ++ck) {
    // one barrier per chunk: buffer ck&1 is complete, and every wave is done
    // reading the other one (its MFMAs of chunk ck-1 precede this barrier)
    __syncthreads();
    const ushort* cur = patch + (ck & 1) * BUF;
    const bool more = ck + 1 < nchunks;
    if (more) load_chunk((ck + 1) * CIK);   // in flight under the MFMAs

    const int ci0 = ck * CIK;
    // ky stays a loop: fully unrolled, the compiler hoists the fragment
    // reads of all nine taps and the kernel drops to one wave per SIMD
#pragma unroll 1
    for (int ky = 0; ky < KS; ++ky)
#pragma unroll
    for (int kx = 0; kx < KS; ++kx) {
      const int tap = ky * KS + kx;
      s16x8 wf[MCW];
#pragma unroll
      for (int m = 0; m < MCW; ++m) {
        const int row = co0 + (wm * MCW + m) * 16 + l15;   // < Mp (padded)
        wf[m] = *reinterpret_cast<const s16x8*>(
            &wp[((long long)tap * Mp + row) * Kp + ci0 + kgrp]);
      }
#pragma unroll
      for (int nf = 0; nf < 8; ++nf) {
        const int r = wn * 4 + (nf >> 1);
        const int col = (nf & 1) * 16 + l15;
        const s16x8 pf = *reinterpret_cast<const s16x8*>(
            &cur[((r + ky) * PWC + col + kx) * SLOT + kgrp]);
#pragma unroll
        for (int m = 0; m < MCW; ++m)
          acc[nf][m] = E::mfma(pf, wf[m], acc[nf][m]);
      }
    }
    if (more) store_chunk(patch + ((ck + 1) & 1) * BUF);
  }

  // ---- epilogue.  D (guide §3): row = pixel (lane>>4)*4 + j of the
  // fragment's 16, col = channel lane&15.  Fragments 2r and 2r+1 are the two
  // halves of tile row r: a lane with lg even keeps its four pixels of the
  // left half and takes the next four from lane+16; a lane with lg odd does
  // the same on the right half with lane-16.  Every lane then holds 8
  // neighbouring pixels: lg 0 -> cols 0-7, 2 -> 8-15, 1 -> 16-23, 3 -> 24-31.
  const bool odd = lg & 1;
  const int ox0 = tx0 + (odd ? 16 : 0) + (lg >> 1) * 8;
#pragma unroll
  for (int m = 0; m < MCW; ++m) {
    const int co = co0 + (wm * MCW + m) * 16 + l15;
    const float bv = (bias && co < Cout) ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      unsigned int p[2][2];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const ushort lo =
              E::from_f(apply_act_rt(acc[2 * r + h][m][2 * q] + bv, act));
          const ushort hi =
              E::from_f(apply_act_rt(acc[2 * r + h][m][2 * q + 1] + bv, act));
          p[h][q] = (unsigned int)lo | ((unsigned int)hi << 16);
        }
      // all 64 lanes take part in the exchange: no branch above this point
      const unsigned int s0 = odd ? p[0][0] : p[1][0];
      const unsigned int s1 = odd ? p[0][1] : p[1][1];
      const unsigned int r0 = (unsigned int)__shfl_xor((int)s0, 16, 64);
      const unsigned int r1 = (unsigned int)__shfl_xor((int)s1, 16, 64);
      unsigned int o[4];
      o[0] = odd ? r0 : p[0][0];
      o[1] = odd ? r1 : p[0][1];
      o[2] = odd ? p[1][0] : r0;
      o[3] = odd ? p[1][1] : r1;
      const int oy = ty0 + wn * 4 + r;
      if (co < Cout && oy < H && ox0 < W) {
        ushort* dst = y + (((long long)b * Cout + co) * H + oy) * W + ox0;
        if (valign && ox0 + 8 <= W) {
          *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (ox0 + e < W)
              dst[e] = (ushort)(o[e >> 1] >> ((e & 1) * 16));
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// VALU direct forward: grid-stride over outputs; for bandwidth-bound
// small-channel shapes (head/tail/attention convs).  Neighbouring lanes
// read neighbouring ix -> coalesced; weights broadcast through K$/L1.
// ---------------------------------------------------------------------------

template <typename E, int KS, int STRIDE, int ACT>
__global__ void conv2d_fwd_valu_kernel(
    long long n, const ushort* __restrict__ x,
    const ushort* __restrict__ w,      // [Cout, Cin, KS, KS] (unpacked)
    const float* __restrict__ bias, ushort* __restrict__ y,
    int Cin, int H, int W, int Cout, int Ho, int Wo) {
  constexpr int PAD = KS / 2;
  ESR_KERNEL_LOOP(i, n) {
    const int ox = (int)(i % Wo);
    long long t = i / Wo;
    const int oy = (int)(t % Ho); t /= Ho;
    const int co = (int)(t % Cout);
    const int b = (int)(t / Cout);
    const long long plane = (long long)H * W;
    const ushort* xb = x + (long long)b * Cin * plane;
    const ushort* wc = w + (long long)co * Cin * KS * KS;
    float acc = bias ? bias[co] : 0.f;
    const int iy0 = oy * STRIDE - PAD, ix0 = ox * STRIDE - PAD;
    for (int ci = 0; ci < Cin; ++ci) {
      const ushort* xp = xb + ci * plane;
      const ushort* wk = wc + ci * KS * KS;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int iy = iy0 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const int ix = ix0 + kx;
          if (ix < 0 || ix >= W) continue;
          acc += E::to_f(xp[(long long)iy * W + ix]) *
                 E::to_f(wk[ky * KS + kx]);
        }
      }
    }
    y[i] = E::from_f(apply_act<ACT>(acc));
  }
}

// ---------------------------------------------------------------------------
// VALU forward v2 for the tiny-channel shapes (head 2->8, enc1 8->16,
// tail 8->2 at 256x256): each thread computes an 8-wide output strip for
// up to 8 cout at once — input row segments live in registers and are
// reused across cout and taps, weights broadcast from LDS.  The v1
// per-output kernel was instruction-bound (one bounds-checked scalar load
// per MAC); this one does ~18 loads per 1152 MACs on the head shape.
// ---------------------------------------------------------------------------

template <typename E, int KS, int STRIDE, int ACT, int COCH>
__global__ __launch_bounds__(256)
void conv2d_fwd_valu2_kernel(
    const ushort* __restrict__ x,   // [B, Cin, H, W] bf16/fp16
    const ushort* __restrict__ w,   // [Cout, Cin, KS, KS] same
    const float* __restrict__ bias, ushort* __restrict__ y,
    int Cin, int H, int W, int Cout, int Ho, int Wo,
    long long nstrips, int nsx) {
  constexpr int PAD = KS / 2;
  constexpr int VEC = 8;                       // outputs per thread strip
  constexpr int NPX = VEC * STRIDE + KS - 1;   // input px per row segment
  __shared__ ushort wl[COCH * 32 * KS * KS];   // this co-chunk x <=32ci

  // ---- preload this co-chunk's weights once per block
  const int co0 = blockIdx.z * COCH;
  const int nw = COCH * Cin * KS * KS;
  for (int i = threadIdx.x; i < nw; i += 256) {
    const int co = i / (Cin * KS * KS);
    wl[i] = (co0 + co < Cout)
        ? w[((long long)(co0 + co) * Cin) * KS * KS + (i % (Cin * KS * KS))]
        : (ushort)0;
  }
  __syncthreads();

  for (long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
       s < nstrips; s += (long long)gridDim.x * blockDim.x) {
    const int sx = (int)(s % nsx);
    const int oy = (int)((s / nsx) % Ho);
    const int b = (int)(s / ((long long)nsx * Ho));
    const int ox0 = sx * VEC;
    const long long plane = (long long)H * W;
    const ushort* xb = x + (long long)b * Cin * plane;

    float acc[COCH][VEC];   // compile-time indexed everywhere (rule 20)
#pragma unroll
    for (int c = 0; c < COCH; ++c)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[c][j] = 0.f;

    const int ix0 = ox0 * STRIDE - PAD;
    const bool interior = ix0 >= 0 && ix0 + NPX <= W;
    for (int ci = 0; ci < Cin; ++ci) {
      const ushort* xp = xb + ci * plane;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int iy = oy * STRIDE + ky - PAD;
        float seg[NPX];
        if (iy >= 0 && iy < H) {
          const ushort* row = xp + (long long)iy * W;
          if (interior) {
#pragma unroll
            for (int e = 0; e < NPX; ++e)
              seg[e] = E::to_f(row[ix0 + e]);
          } else {
#pragma unroll
            for (int e = 0; e < NPX; ++e) {
              const int ix = ix0 + e;
              seg[e] = (ix >= 0 && ix < W) ? E::to_f(row[ix]) : 0.f;
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < NPX; ++e) seg[e] = 0.f;
        }
        const ushort* wrow = &wl[(ci * KS + ky) * KS];
#pragma unroll
        for (int c = 0; c < COCH; ++c) {
          float wk[KS];
#pragma unroll
          for (int kx = 0; kx < KS; ++kx)
            wk[kx] = E::to_f(wrow[c * Cin * KS * KS + kx]);
#pragma unroll
          for (int j = 0; j < VEC; ++j) {
            float v = acc[c][j];
#pragma unroll
            for (int kx = 0; kx < KS; ++kx)
              v = fmaf(seg[j * STRIDE + kx], wk[kx], v);
            acc[c][j] = v;
          }
        }
      }
    }

    // ---- epilogue: bias + act, vector 16-bit stores per cout row
    const int nvalid = Wo - ox0 < VEC ? Wo - ox0 : VEC;
#pragma unroll
    for (int c = 0; c < COCH; ++c) {
      const int co = co0 + c;
      if (co >= Cout) break;
      ushort packed[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float v = acc[c][j];
        if (bias) v += bias[co];
        packed[j] = E::from_f(apply_act<ACT>(v));
      }
      ushort* dst = y + (((long long)b * Cout + co) * Ho + oy) * Wo + ox0;
      // vector store only when the row base is 16B-aligned (Wo % 8 != 0
      // leaves interior strips misaligned)
      if (nvalid == VEC && (((unsigned long long)(uintptr_t)dst) & 15) == 0) {
        *reinterpret_cast<s16x8*>(dst) =
            *reinterpret_cast<const s16x8*>(packed);
      } else {
        for (int j = 0; j < nvalid; ++j) dst[j] = packed[j];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Stride-2 input-grad (scatter form as a gather): dx[iy][ix] sums the <=4
// taps whose (iy + PAD - ky) is even, over all Cout.
// ---------------------------------------------------------------------------

template <int KS>
__global__ void conv2d_dgrad_s2_valu_kernel(
    long long n, const ushort* __restrict__ dy,  // [B, Cout, Ho, Wo]
    const ushort* __restrict__ w,                // [Cout, Cin, KS, KS]
    ushort* __restrict__ dx,                     // [B, Cin, H, W]
    int Cin, int H, int W, int Cout, int Ho, int Wo) {
  constexpr int PAD = KS / 2;
  ESR_KERNEL_LOOP(i, n) {
    const int ix = (int)(i % W);
    long long t = i / W;
    const int iy = (int)(t % H); t /= H;
    const int ci = (int)(t % Cin);
    const int b = (int)(t / Cin);
    float acc = 0.f;
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
      const int ty = iy + PAD - ky;
      if (ty < 0 || (ty & 1)) continue;
      const int oy = ty >> 1;
      if (oy >= Ho) continue;
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const int tx = ix + PAD - kx;
        if (tx < 0 || (tx & 1)) continue;
        const int ox = tx >> 1;
        if (ox >= Wo) continue;
        for (int co = 0; co < Cout; ++co) {
          acc += bf16u_to_f(dy[(((long long)b * Cout + co) * Ho + oy) * Wo + ox]) *
                 bf16u_to_f(w[(((long long)co * Cin + ci) * KS + ky) * KS + kx]);
        }
      }
    }
    dx[i] = f_to_bf16u(acc);
  }
}

// ---------------------------------------------------------------------------
// MFMA weight-grad v1 (kept for STRIDE 2), split-K over output pixels.
// dW[co][ci][ky][kx] = sum_pix dpre[co][oy][ox] * X[ci][oy*s+ky-1][ox*s+kx-1]
//   A = dpre, pre-shifted per kx (3 small scalar-staged copies, halo'd)
//   B = X, one aligned vector-staged copy [ci][ky-row][u-chunk]
// Each wave owns its own LDS tiles and an independent slice of output
// rows; the flush reduces the 4 waves through LDS then issues atomics in
// the TRANSPOSED [Cin_p][Cout_p] scratch (lanes span cachelines).
// ---------------------------------------------------------------------------

constexpr int WG_PW = 40;  // padded 32-px rows, same bank math as SLOT

template <int KS, int STRIDE>
__global__ __launch_bounds__(256)
void conv2d_wgrad_mfma_kernel(
    const ushort* __restrict__ x,     // [B, Cin, H, W]
    const ushort* __restrict__ dpre,  // [B, Cout, Ho, Wo]
    float* __restrict__ dwp,          // TRANSPOSED [Cin_p, Cout_p, KS, KS]
    int Cin, int H, int W, int Cout, int Ho, int Wo,
    int Cin_p, int Cout_p, int rows_per_blk) {
  constexpr int PAD = KS / 2;
  constexpr int NTAP = KS * KS;
  // per-wave LDS: X [16ci][KS rows][WG_PW] + dpre shifted copies [KS][16co][WG_PW]
  __shared__ ushort xs_all[4][16 * KS * WG_PW];
  __shared__ ushort dp_all[4][KS * 16 * WG_PW];
  __shared__ float red[16 * 16];  // cross-wave reduction buffer (per tap)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  ushort* xs = xs_all[wave];
  ushort* dp = dp_all[wave];

  const int co0 = blockIdx.z * 16;
  const int ci0 = blockIdx.y * 16;
  const long long nslab = blockIdx.x;
  const int uw = (W + TW - 1) / TW;        // u-chunks per input row
  const int b = (int)(nslab / ((Ho + rows_per_blk - 1) / rows_per_blk * uw));
  const int rslab = (int)(nslab % ((Ho + rows_per_blk - 1) / rows_per_blk * uw));
  const int r0 = (rslab / uw) * rows_per_blk;
  const int ux0 = (rslab % uw) * TW;

  const long long xplane = (long long)H * W;
  const long long dplane = (long long)Ho * Wo;
  const ushort* xb = x + (long long)b * Cin * xplane;
  const ushort* db = dpre + (long long)b * Cout * dplane;

  f32x4 acc[NTAP] = {};
  const int kgrp = (lane >> 4) * 8;

  for (int oy = r0 + wave; oy < min(r0 + rows_per_blk, Ho); oy += 4) {
    // ---- stage X rows iy = oy*s + ky - PAD at u in [ux0, ux0+32), aligned
    // lane <-> (ci, ky, u-chunk-of-8): 16*KS*4 units
    for (int u = lane; u < 16 * KS * 4; u += 64) {
      const int ci = u / (KS * 4);
      const int ky = (u / 4) % KS;
      const int c8 = u % 4;
      const int iy = oy * STRIDE + ky - PAD;
      ushort vals[8];
      const int gci = ci0 + ci;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ix = ux0 + c8 * 8 + e;
        vals[e] = (gci < Cin && iy >= 0 && iy < H && ix < W)
            ? xb[gci * xplane + (long long)iy * W + ix] : (ushort)0;
      }
      *reinterpret_cast<s16x8*>(&xs[(ci * KS + ky) * WG_PW + c8 * 8]) =
          *reinterpret_cast<const s16x8*>(&vals[0]);
    }
    // ---- stage dpre shifted per kx: dp[kx][co][j] = dpre[co][oy][ox(u)]
    // u = ux0 + j; ox = (u + PAD - kx) / STRIDE when divisible, else 0
    for (int u = lane; u < KS * 16 * 4; u += 64) {
      const int kx = u / (16 * 4);
      const int co = (u / 4) % 16;
      const int c8 = u % 4;
      const int gco = co0 + co;
      ushort vals[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int uu = ux0 + c8 * 8 + e;
        const int tx = uu + PAD - kx;
        ushort v = 0;
        if (gco < Cout && tx >= 0 && (STRIDE == 1 || (tx & 1) == 0)) {
          const int ox = tx / STRIDE;
          if (ox < Wo)
            v = db[gco * dplane + (long long)oy * Wo + ox];
        }
        vals[e] = v;
      }
      *reinterpret_cast<s16x8*>(&dp[(kx * 16 + co) * WG_PW + c8 * 8]) =
          *reinterpret_cast<const s16x8*>(&vals[0]);
    }
    // wave-synchronous: the same wave wrote and now reads its own LDS
    // slices, but the writer/reader LANES differ, so the compiler's
    // per-thread scoreboard can't see the dependency — drain the LDS queue
    // explicitly (no barrier needed: wave64 executes in lockstep)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- 2 K-subchunks of 16 pixels... K = 32 pixels of this row chunk
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const s16x8 a = *reinterpret_cast<const s16x8*>(
            &dp[(kx * 16 + (lane & 15)) * WG_PW + kgrp]);
        const s16x8 bf = *reinterpret_cast<const s16x8*>(
            &xs[((lane & 15) * KS + ky) * WG_PW + kgrp]);
        acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, bf, acc[ky * KS + kx], 0, 0, 0);
      }
    }
  }

  // ---- flush: D col = ci = lane&15, row = co = (lane>>4)*4 + j.
  // 4-wave partials meet in LDS (4-way atomic contention max), then one
  // global fp32 atomic per dW element per block (guide G12).
  for (int tap = 0; tap < NTAP; ++tap) {
    const int ky = tap / KS, kx = tap % KS;
    red[tid] = 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j)
      atomicAdd(&red[((lane >> 4) * 4 + j) * 16 + (lane & 15)], acc[tap][j]);
    __syncthreads();
    if (tid < 256) {
      // consecutive threads vary ci -> distinct lines in the transposed
      // [Cin_p][Cout_p] scratch
      const int co = tid >> 4, ci = tid & 15;
      atomicAdd(&dwp[(((long long)(ci0 + ci) * Cout_p + co0 + co) * KS + ky)
                     * KS + kx], red[tid]);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// MFMA weight-grad v2, stride-1 (3x3 p1 and 1x1): block-wide staged tiles,
// all staging as aligned b128 vectors, kx-shifts resolved by REGISTER
// shuffles of adjacent aligned fragments (no shifted LDS copies, no
// unaligned ds_read — guide G17).
//
//   block tile: [64 co] x [32 ci] x taps;  wave w owns co slice w*16.
//   A = dpre rows (halo'd u-domain), B = X rows; D[row=co][col=ci].
//   K = output pixels, chunked 32 per output row; fp32 atomics out.
// ---------------------------------------------------------------------------

constexpr int WGV2_DPW = 56;  // dp row stride in shorts (112 B: 28-dword
                              // stride, gcd(28,64)=4 -> conflict-free b128)
constexpr int WGV2_XW = 40;   // x row stride (same bank math as SLOT)

template <int KS>
__global__ __launch_bounds__(256)
void conv2d_wgrad_s1_kernel(
    const ushort* __restrict__ x,     // [B, Cin, H, W]
    const ushort* __restrict__ dpre,  // [B, Cout, H, W] (stride 1: Ho=H)
    float* __restrict__ dwp,          // partial tiles [g][32ci][64co][NTAP]
    int Cin, int H, int W, int Cout,
    int Cin_p, int Cout_p, int uw, int B, int fpb, int abl) {
  // abl (ablation, tools/bench_conv.py --wgrad): 0 = full, 1 = skip the
  // flush, 2 = skip MFMA (staging only; flush still runs)
  constexpr int PAD = KS / 2;
  constexpr int NTAP = KS * KS;
  constexpr int RB = 4;                       // output rows per barrier pair
  __shared__ ushort dp[RB * 64 * WGV2_DPW];   // px domain [-8, 48) per row
  __shared__ ushort xs[32 * (RB + 2) * WGV2_XW];  // rolling 6-row window

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const int b0 = (blockIdx.x / uw) * fpb;
  const int ux0 = (blockIdx.x % uw) * TW;
  const int ci0 = blockIdx.y * 32;
  const int co0 = blockIdx.z * 64;

  const long long plane = (long long)H * W;

  f32x4 acc[NTAP][2] = {};
  const int kgrp = (lane >> 4) * 8;
  constexpr int NSLOT = RB + 2;

  // stage one X row (iy) into rolling slot (iy mod NSLOT); zeros when oob
  auto stage_x_row = [&](const ushort* xb, int iy) {
    const int slot = ((iy % NSLOT) + NSLOT) % NSLOT;
    for (int u = tid; u < 32 * 4; u += 256) {
      const int ci = u >> 2, blk = u & 3;
      const int gci = ci0 + ci;
      const int px0 = ux0 + blk * 8;
      ushort vals[8] = {};
      if (gci < Cin && iy >= 0 && iy < H) {
        const ushort* src = xb + gci * plane + (long long)iy * W;
        if (px0 + 8 <= W) {
          *reinterpret_cast<s16x8*>(vals) =
              *reinterpret_cast<const s16x8*>(src + px0);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            vals[e] = (px0 + e < W) ? src[px0 + e] : (ushort)0;
        }
      }
      *reinterpret_cast<s16x8*>(&xs[(ci * NSLOT + slot) * WGV2_XW + blk * 8]) =
          *reinterpret_cast<const s16x8*>(vals);
    }
  };

  for (int bf = 0; bf < fpb && b0 + bf < B; ++bf) {
    const int b = b0 + bf;
    const ushort* xb = x + (long long)b * Cin * plane;
    const ushort* db = dpre + (long long)b * Cout * plane;

    // prologue: window rows -1, 0 (zeros via oob for -1)
    __syncthreads();
    if (KS == 3) {
      stage_x_row(xb, -1);
      stage_x_row(xb, 0);
    }

    for (int oy0 = 0; oy0 < H; oy0 += RB) {
      // ---- stage RB dp rows [64 co] at px [-8, 48): 7 b128 per row
      // (the kx=0 fragment at kgrp=24 reaches one pixel past the chunk)
      for (int u = tid; u < RB * 64 * 7; u += 256) {
        const int r = u / (64 * 7);
        const int co = (u / 7) % 64, blk = u % 7;
        const int gco = co0 + co;
        const int oy = oy0 + r;
        const int px0 = ux0 - 8 + blk * 8;
        ushort vals[8] = {};
        if (gco < Cout && oy < H) {
          const ushort* src = db + gco * plane + (long long)oy * W;
          if (px0 >= 0 && px0 + 8 <= W) {
            *reinterpret_cast<s16x8*>(vals) =
                *reinterpret_cast<const s16x8*>(src + px0);
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int px = px0 + e;
              vals[e] = (px >= 0 && px < W) ? src[px] : (ushort)0;
            }
          }
        }
        *reinterpret_cast<s16x8*>(&dp[(r * 64 + co) * WGV2_DPW + blk * 8]) =
            *reinterpret_cast<const s16x8*>(vals);
      }
      // ---- stage the RB new X rows of the sliding window
#pragma unroll
      for (int r = 0; r < RB; ++r)
        stage_x_row(xb, KS == 3 ? oy0 + r + 1 : oy0 + r);
      __syncthreads();

      if (abl != 2) {
        // ---- compute: wave w covers co rows [co0+w*16, +16)
#pragma unroll
        for (int r = 0; r < RB; ++r) {
          const int oy = oy0 + r;
          const ushort* dprow = &dp[((r * 64) + wave * 16 + (lane & 15))
                                    * WGV2_DPW + 8 + kgrp];
          const s16x8 a_0 = *reinterpret_cast<const s16x8*>(dprow);
          s16x8 afrag[NTAP == 1 ? 1 : 3];
          if (KS == 1) {
            afrag[0] = a_0;
          } else {
            const s16x8 a_m = *reinterpret_cast<const s16x8*>(dprow - 8);
            const s16x8 a_p = *reinterpret_cast<const s16x8*>(dprow + 8);
            // dp index = u + PAD - kx: kx=0 -> +1, kx=1 -> 0, kx=2 -> -1
            afrag[0] =
                __builtin_shufflevector(a_0, a_p, 1, 2, 3, 4, 5, 6, 7, 8);
            afrag[1] = a_0;
            afrag[2] =
                __builtin_shufflevector(a_m, a_0, 7, 8, 9, 10, 11, 12, 13, 14);
          }
#pragma unroll
          for (int ky = 0; ky < KS; ++ky) {
            const int slot = KS == 1 ? oy % NSLOT
                : (((oy + ky - PAD) % NSLOT) + NSLOT) % NSLOT;
#pragma unroll
            for (int nci = 0; nci < 2; ++nci) {
              const s16x8 bfrag = *reinterpret_cast<const s16x8*>(
                  &xs[((nci * 16 + (lane & 15)) * NSLOT + slot) * WGV2_XW
                      + kgrp]);
#pragma unroll
              for (int kx = 0; kx < KS; ++kx)
                acc[ky * KS + kx][nci] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        afrag[kx], bfrag, acc[ky * KS + kx][nci], 0, 0, 0);
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- flush: plain coalesced stores of this block's partial tile into
  // scratch [g][32ci][64co][NTAP]; a second kernel reduces over g.  No
  // atomics (an atomic flood here measured 70-87% of the kernel) and the
  // reduction order is DETERMINISTIC.
  if (abl == 1) return;
  float* part = dwp + ((((long long)blockIdx.x * gridDim.y + blockIdx.y)
                        * gridDim.z + blockIdx.z) * (32 * 64 * NTAP));
#pragma unroll
  for (int tap = 0; tap < NTAP; ++tap) {
#pragma unroll
    for (int nci = 0; nci < 2; ++nci) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = wave * 16 + (lane >> 4) * 4 + j;
        const int ci = nci * 16 + (lane & 15);
        part[((long long)ci * 64 + co) * NTAP + tap] = acc[tap][nci][j];
      }
    }
  }
}

// reduce the per-block partials: dwp[ci][co][tap] = sum_g part[g][...]
template <int NTAP>
__global__ void conv2d_wgrad_reduce_kernel(
    long long n, const float* __restrict__ part, int ng, int ciblks,
    int coblks, int Cin_p, int Cout_p, float* __restrict__ dwp) {
  ESR_KERNEL_LOOP(i, n) {  // i -> (ci, co, tap) over the PADDED dW
    const int tap = (int)(i % NTAP);
    const int co = (int)((i / NTAP) % Cout_p);
    const int ci = (int)(i / ((long long)NTAP * Cout_p));
    const int cib = ci / 32, cob = co / 64;
    const long long base =
        ((long long)cib * coblks + cob) * (32 * 64 * NTAP)
        + (((long long)(ci % 32) * 64 + (co % 64)) * NTAP + tap);
    const long long gstride = (long long)ciblks * coblks * (32 * 64 * NTAP);
    float v = 0.f;
    for (int g = 0; g < ng; ++g) v += part[g * gstride + base];
    dwp[i] = v;
  }
}

// The same stage 2, writing the weight's own layout and dtype: i runs over
// dW [Cout, Cin, k, k] bf16, each element the fp32 sum over g (same order as
// above) rounded once.  Longest chain of dependent fp32 additions behind one
// dW element, unchanged by this kernel:
//   n = 32 (one MFMA product) + fpb*H (MFMAs per block) + ng (partials),
//   ng = ceil(B/fpb) * ceil(W/32), fpb from the host's grid rule
// (B768 128->64 32x32: fpb 2, ng 384, n = 480; B384 32->64 64x64: fpb 1,
// ng 768, n = 864; both under the 2^11 of tests/bound_rules.py).
template <int NTAP>
__global__ void conv2d_wgrad_reduce_out_kernel(
    long long n, const float* __restrict__ part, int ng, int coblks,
    int Cin, int Cout, ushort* __restrict__ dw) {
  // i runs over one partial tile set [cib][cob][32ci][64co][tap], so the
  // reads of every g are contiguous; the (small) dW is written scattered
  ESR_KERNEL_LOOP(i, n) {
    const int tap = (int)(i % NTAP);
    const int co64 = (int)((i / NTAP) % 64);
    const int ci32 = (int)((i / (NTAP * 64)) % 32);
    const int blk = (int)(i / (NTAP * 64 * 32));
    const int ci = (blk / coblks) * 32 + ci32;
    const int co = (blk % coblks) * 64 + co64;
    if (ci >= Cin || co >= Cout) continue;
    float v = 0.f;
    for (int g = 0; g < ng; ++g) v += part[g * n + i];
    dw[((long long)co * Cin + ci) * NTAP + tap] = f_to_bf16u(v);
  }
}

// ---------------------------------------------------------------------------
// Activation backward: dpre = dy * act'(y) elementwise, bf16 or fp16.
// ---------------------------------------------------------------------------

// dy * act'(y) in fp32, act' written in the activated value y; the one
// expression both act_grad_kernel and act_grad_bias_kernel evaluate
template <int ACT> ESR_INLINE float act_grad_value(float g, float v) {
  if (ACT == 0) return g;
  if (ACT == 1) return v > 0.f ? g : 0.f;
  if (ACT == 2) return g * v * (1.f - v);
  return g * (1.f - v * v);  // tanh
}

// One dpre element, 16-bit in and out.  The empty asm keeps d an fp32 value
// of its own: without it hipcc folds the last multiply and the fp16 store
// conversion into one v_fma_mixlo_f16 in some loops (one rounding of the
// exact product) and keeps v_mul_f32 + v_cvt_f16_f32 in others (two
// roundings, the unrolled body of act_grad_kernel), and about one fp16
// element in 2^14 then differs in its last bit between two kernels, or
// between the unrolled body and the remainder loop of one kernel.  With it
// every path rounds the fp32 result once, as the file header says.
template <typename E, int ACT>
ESR_INLINE ushort act_grad_elem(ushort dy, ushort y) {
  float d = act_grad_value<ACT>(E::to_f(dy), E::to_f(y));
  asm("" : "+v"(d));
  return E::from_f(d);
}

template <typename E, int ACT>
__global__ void act_grad_kernel(long long n, const ushort* __restrict__ dy,
                                const ushort* __restrict__ y,
                                ushort* __restrict__ dpre) {
  ESR_KERNEL_LOOP(i, n) {
    dpre[i] = act_grad_elem<E, ACT>(dy[i], y[i]);
  }
}

// ---------------------------------------------------------------------------
// Activation backward fused with the conv bias gradient, and the bias
// gradient alone (ACT == 0, no store): one pass over NCHW [B,C,H,W].
//
//   dpre = dy * act'(y)             (act_grad_kernel's arithmetic and rounding)
//   db[c] = sum_{b,h,w} dpre[b,c,h,w]   over the ROUNDED dpre, i.e. exactly
//                                       what the dW / dx kernels consume
//
// Work item: channel c's B planes laid end to end are a row of L = B*H*W
// elements, cut into chunks of BG_CHUNK = 256 threads x BG_VPT x 8 elements;
// item = (c, chunk), P = ceil(L / BG_CHUNK) chunks per channel.  A chunk may
// cover part of one plane or several planes of its channel.  With H*W % 8 == 0
// every plane is 16-byte aligned and an 8-element group never straddles two
// planes: 16-byte loads/stores.  Otherwise (5x33: plane 1 starts 330 B in) a
// scalar path walks the same chunk element by element.  Items past the grid
// cap are taken by a grid-stride loop.
//
// Deterministic two-stage reduction, no atomics.  Stage 1 writes one fp32
// partial per item, part[c*P + chunk]; bias_grad_reduce_kernel (one block per
// channel) adds a channel's P partials in a fixed order and rounds once.
// Longest chain of dependent fp32 additions behind one db element:
//   stage 1: 8*BG_VPT per lane + 6 shuffle levels + 3 (4 wave sums in LDS)
//   stage 2: ceil(P/256) per lane + 6 shuffle levels + 3
//   n = 8*BG_VPT + 18 + ceil(P/256)
// (34 + ceil(P/256) at BG_VPT = 2; B768 C64 64x64: P = 768, n = 37).  The host
// refuses shapes with n > 2^11, the chain cap tests/bound_rules.py assumes.
// ---------------------------------------------------------------------------

constexpr int BG_VPT = 2;                        // 16-byte groups per thread
constexpr int BG_CHUNK = ESR_BLOCK * BG_VPT * 8; // elements per work item

// sum over the block's 256 threads in a fixed order; result valid in thread 0
ESR_INLINE float bg_block_sum(float v, float* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // red may still be read from the previous item
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

template <typename E, int ACT, bool STORE>
__global__ __launch_bounds__(ESR_BLOCK)
void act_grad_bias_kernel(int C, unsigned int HW, unsigned int L,
                          unsigned int P, bool vec,
                          const ushort* __restrict__ dy,
                          const ushort* __restrict__ y,
                          ushort* __restrict__ dpre,
                          float* __restrict__ part) {
  __shared__ float red[ESR_BLOCK / 64];
  const long long nitem = (long long)C * P;
  for (long long item = blockIdx.x; item < nitem; item += gridDim.x) {
    const int c = (int)(item / P);
    const unsigned int e0 = (unsigned int)(item % P) * BG_CHUNK;
    float acc = 0.f;
    if (vec) {
#pragma unroll
      for (int k = 0; k < BG_VPT; ++k) {
        const unsigned int e = e0 + (k * ESR_BLOCK + threadIdx.x) * 8;
        if (e < L) {  // L % 8 == 0: a group is all inside or all outside
          const unsigned int b = e / HW;
          const long long a = ((long long)b * C + c) * HW + (e - b * HW);
          s16x8 g8 = *(const s16x8*)(dy + a);
          if (ACT != 0) {
            const s16x8 y8 = *(const s16x8*)(y + a);
#pragma unroll
            for (int j = 0; j < 8; ++j)
              g8[j] = (short)act_grad_elem<E, ACT>((ushort)g8[j],
                                                   (ushort)y8[j]);
          }
          if (STORE) *(s16x8*)(dpre + a) = g8;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc += E::to_f((ushort)g8[j]);
        }
      }
    } else {
      for (int k = 0; k < BG_VPT * 8; ++k) {
        const unsigned int e = e0 + k * ESR_BLOCK + threadIdx.x;
        if (e < L) {
          const unsigned int b = e / HW;
          const long long a = ((long long)b * C + c) * HW + (e - b * HW);
          ushort d = dy[a];
          if (ACT != 0)
            d = act_grad_elem<E, ACT>(d, y[a]);
          if (STORE) dpre[a] = d;
          acc += E::to_f(d);
        }
      }
    }
    const float s = bg_block_sum(acc, red);
    if (threadIdx.x == 0) part[item] = s;
  }
}

// stage 2: block c adds part[c*P .. c*P+P) in index order (lane t takes
// t, t+256, ...; then the same tree as stage 1) and rounds the sum once to
// the bias dtype; sum32 (may be null) receives the fp32 sum for the tests
template <typename E>
__global__ __launch_bounds__(ESR_BLOCK)
void bias_grad_reduce_kernel(unsigned int P, const float* __restrict__ part,
                             float* __restrict__ sum32,
                             ushort* __restrict__ db) {
  __shared__ float red[ESR_BLOCK / 64];
  const float* p = part + (long long)blockIdx.x * P;
  float acc = 0.f;
  for (unsigned int i = threadIdx.x; i < P; i += ESR_BLOCK) acc += p[i];
  const float s = bg_block_sum(acc, red);
  if (threadIdx.x == 0) {
    if (sum32) sum32[blockIdx.x] = s;
    db[blockIdx.x] = E::from_f(s);
  }
}

// ---------------------------------------------------------------------------
// 16x16x32 GEMM probe: C[16,16] = A[16,32] @ B[32,16] — verifies the MFMA
// fragment maps this file assumes (guide §3; asymmetric-B testable).
// ---------------------------------------------------------------------------

template <typename E>
__global__ void gemm16_probe_kernel(const ushort* __restrict__ A,
                                    const ushort* __restrict__ B,
                                    float* __restrict__ C) {
  const int lane = threadIdx.x & 63;
  s16x8 a, b;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    a[j] = (short)A[(lane & 15) * 32 + (lane >> 4) * 8 + j];
    b[j] = (short)B[((lane >> 4) * 8 + j) * 16 + (lane & 15)];
  }
  f32x4 acc = {};
  acc = E::mfma(a, b, acc);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    C[((lane >> 4) * 4 + j) * 16 + (lane & 15)] = acc[j];
}

}  // namespace

// ===========================================================================
// Host wrappers
// ===========================================================================

#define DISPATCH_ACT(ACT, ...)                              \
  [&] {                                                     \
    switch (ACT) {                                          \
      case 0: { constexpr int kAct = 0; return __VA_ARGS__(); } \
      case 1: { constexpr int kAct = 1; return __VA_ARGS__(); } \
      case 2: { constexpr int kAct = 2; return __VA_ARGS__(); } \
      default: { constexpr int kAct = 3; return __VA_ARGS__(); } \
    }                                                       \
  }()

#define DISPATCH_KS_STRIDE(KS, STRIDE, ...)                                  \
  [&] {                                                                      \
    if (KS == 3 && STRIDE == 1) { constexpr int kKS = 3, kST = 1; return __VA_ARGS__(); } \
    if (KS == 3 && STRIDE == 2) { constexpr int kKS = 3, kST = 2; return __VA_ARGS__(); } \
    if (KS == 1 && STRIDE == 1) { constexpr int kKS = 1, kST = 1; return __VA_ARGS__(); } \
    TORCH_CHECK(false, "unsupported (ks, stride) = (", KS, ", ", STRIDE, ")"); \
    constexpr int kKS = 3, kST = 1; return __VA_ARGS__();                    \
  }()

// element-type dispatch for the forward kernels / act_grad / probe
#define DISPATCH_ELEM(TYPE, ...)                                        \
  [&] {                                                                 \
    if ((TYPE) == at::kHalf) { using elem_t = ElemFp16; return __VA_ARGS__(); } \
    using elem_t = ElemBf16; return __VA_ARGS__();                      \
  }()

// backward-only kernels (dgrad_s2, wgrad) are bf16-only: an fp16 tensor
// must fail here, not have its bits read as bf16
static void check_bf16_4d(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 &&
              t.is_contiguous(), name,
              ": contiguous bf16 CUDA tensor required (this kernel is "
              "bf16-only), got ", t.scalar_type());
}

static void check_16bit(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              (t.scalar_type() == at::kBFloat16 ||
               t.scalar_type() == at::kHalf), name,
              ": contiguous bf16 or fp16 CUDA tensor required, got ",
              t.scalar_type());
}

// all 16-bit operands of one call share one dtype
static void check_same_dtype(const at::Tensor& a, const at::Tensor& b,
                             const char* what) {
  TORCH_CHECK(a.scalar_type() == b.scalar_type(), what,
              ": operand dtypes differ (", a.scalar_type(), " vs ",
              b.scalar_type(), "); bf16 and fp16 cannot be mixed in one call");
}

static const float* bias_ptr_f32(const c10::optional<at::Tensor>& bias,
                                 const at::Tensor& x) {
  if (!bias.has_value()) return nullptr;
  TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->is_contiguous() &&
              bias->device() == x.device(),
              "bias: contiguous fp32 tensor on x's device required, got ",
              bias->scalar_type());
  return bias->data_ptr<float>();
}

// x [B,Cin,H,W] bf16|fp16, wp [ntap, Cout_p, Cin_p] same dtype,
// bias [Cout] fp32 | none; output has x's dtype
at::Tensor conv2d_fwd_mfma(const at::Tensor& x, const at::Tensor& wp,
                           const c10::optional<at::Tensor>& bias,
                           int64_t Cout, int64_t ks, int64_t stride,
                           int64_t act) {
  check_16bit(x, "conv2d_fwd_mfma: x");
  check_16bit(wp, "conv2d_fwd_mfma: wp");
  check_same_dtype(x, wp, "conv2d_fwd_mfma: x / wp");
  TORCH_CHECK(x.dim() == 4 && wp.dim() == 3,
              "x [B,Cin,H,W], wp: packed [ntap,Cop,Cip]");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const int Cout_p = wp.size(1), Cin_p = wp.size(2);
  TORCH_CHECK(wp.size(0) == ks * ks && Cin_p % CIK == 0 && Cout_p % 16 == 0);
  const int Ho = (H + 2 * (int)(ks / 2) - (int)ks) / (int)stride + 1;
  const int Wo = (W + 2 * (int)(ks / 2) - (int)ks) / (int)stride + 1;
  auto y = at::empty({B, Cout, Ho, Wo}, x.options());
  const float* bias_ptr = bias_ptr_f32(bias, x);
  const int mrep = (Cout > 32 && Cout_p % 32 == 0) ? 2 : 1;
  const int ntx = (Wo + TW - 1) / TW, nty = (Ho + TH - 1) / TH;
  dim3 grid(ntx * nty, B, (Cout_p + 32 * mrep - 1) / (32 * mrep));
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(x.scalar_type(), [&] {
  DISPATCH_KS_STRIDE((int)ks, (int)stride, [&] {
    DISPATCH_ACT((int)act, [&] {
      if (mrep == 2)
        hipLaunchKernelGGL((conv2d_fwd_mfma_kernel<elem_t, kKS, kST, kAct, 2>),
                           grid, dim3(256), 0, stream,
                           (const ushort*)x.data_ptr(), (const ushort*)wp.data_ptr(),
                           bias_ptr, (ushort*)y.data_ptr(),
                           Cin, H, W, (int)Cout, Ho, Wo, Cin_p, Cout_p, ntx);
      else
        hipLaunchKernelGGL((conv2d_fwd_mfma_kernel<elem_t, kKS, kST, kAct, 1>),
                           grid, dim3(256), 0, stream,
                           (const ushort*)x.data_ptr(), (const ushort*)wp.data_ptr(),
                           bias_ptr, (ushort*)y.data_ptr(),
                           Cin, H, W, (int)Cout, Ho, Wo, Cin_p, Cout_p, ntx);
      return 0;
    });
    return 0;
  });
  return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

// Stride-1 core (conv2d_s1_core_kernel): 3x3 pad 1 or 1x1.
//   dgrad == false: y = act(conv(x, w) + bias), x [B,I,H,W], w [O,I,ks,ks]
//   dgrad == true:  dx = conv_transpose(x = dpre [B,O,H,W], w [O,I,ks,ks]),
//                   bias none, act 0
// Two launches: the weight pack and the core.  No host sync, scratch from
// at::empty (capture-safe).
at::Tensor conv2d_s1(const at::Tensor& x, const at::Tensor& w,
                     const c10::optional<at::Tensor>& bias, int64_t act,
                     bool dgrad) {
  check_16bit(x, "conv2d_s1: x");
  check_16bit(w, "conv2d_s1: w");
  check_same_dtype(x, w, "conv2d_s1: x / w");
  TORCH_CHECK(x.dim() == 4 && w.dim() == 4 && w.size(2) == w.size(3),
              "conv2d_s1: x [B,C,H,W], w [O,I,k,k]");
  const int ks = w.size(2);
  TORCH_CHECK(ks == 1 || ks == 3, "conv2d_s1: 3x3 or 1x1 only, got ", ks);
  TORCH_CHECK(act >= 0 && act <= 3, "conv2d_s1: act id ", act);
  TORCH_CHECK(!dgrad || (!bias.has_value() && act == 0),
              "conv2d_s1: the input grad takes no bias or activation");
  const int O = w.size(0), I = w.size(1);
  const int B = x.size(0), K = x.size(1), H = x.size(2), W = x.size(3);
  const int M = dgrad ? I : O;
  TORCH_CHECK(K == (dgrad ? O : I), "conv2d_s1: x has ", K,
              " channels, w wants ", dgrad ? O : I);
  TORCH_CHECK(B <= 65535, "conv2d_s1: batch above the grid's y limit");
  // channel fragments of 16 per block: at most 8 (128 accumulator VGPRs),
  // an even count (two wave rows); M above 128 is split over blockIdx.z
  const int mfr = (M + 15) / 16;
  const int nsplit = (mfr + 7) / 8;
  const int mc = ((mfr + nsplit - 1) / nsplit + 1) / 2 * 2;
  const int Mp = nsplit * mc * 16;
  const int Kp = (K + CIK - 1) / CIK * CIK;
  const float* bias_ptr = bias_ptr_f32(bias, x);
  if (bias_ptr) TORCH_CHECK(bias->numel() == M, "conv2d_s1: bias size");
  auto wp = at::empty({ks * ks, Mp, Kp}, w.options());
  auto y = at::empty({B, M, H, W}, x.options());
  const int valign = W % 8 == 0 && (uintptr_t)x.data_ptr() % 16 == 0 &&
                     (uintptr_t)y.data_ptr() % 16 == 0;
  const int ntx = (W + TW - 1) / TW, nty = (H + C_TH - 1) / C_TH;
  dim3 grid(ntx * nty, B, nsplit);
  auto stream = at::hip::getCurrentHIPStream();
  const long long npack = (long long)ks * ks * Mp * Kp;
  hipLaunchKernelGGL(conv2d_pack_w_kernel, dim3(esr_grid(npack)),
                     dim3(ESR_BLOCK), 0, stream, npack,
                     (const ushort*)w.data_ptr(), (ushort*)wp.data_ptr(),
                     O, I, ks, Mp, Kp, (int)dgrad);
  DISPATCH_ELEM(x.scalar_type(), [&] {
    auto launch = [&](auto kern) {
      hipLaunchKernelGGL(kern, grid, dim3(256), 0, stream,
                         (const ushort*)x.data_ptr(),
                         (const ushort*)wp.data_ptr(), bias_ptr,
                         (ushort*)y.data_ptr(), K, H, W, M, Kp, Mp, ntx,
                         (int)act, valign);
    };
    auto by_mc = [&](auto ks_tag) {
      constexpr int kKS = decltype(ks_tag)::value;
      switch (mc) {
        case 2: launch(conv2d_s1_core_kernel<elem_t, kKS, 2>); break;
        case 4: launch(conv2d_s1_core_kernel<elem_t, kKS, 4>); break;
        case 6: launch(conv2d_s1_core_kernel<elem_t, kKS, 6>); break;
        default: launch(conv2d_s1_core_kernel<elem_t, kKS, 8>); break;
      }
    };
    if (ks == 3) by_mc(std::integral_constant<int, 3>{});
    else by_mc(std::integral_constant<int, 1>{});
    return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

// x [B,Cin,H,W] bf16|fp16, w [Cout,Cin,ks,ks] same dtype (unpacked),
// bias fp32 | none
at::Tensor conv2d_fwd_valu(const at::Tensor& x, const at::Tensor& w,
                           const c10::optional<at::Tensor>& bias,
                           int64_t stride, int64_t act) {
  check_16bit(x, "conv2d_fwd_valu: x");
  check_16bit(w, "conv2d_fwd_valu: w");
  check_same_dtype(x, w, "conv2d_fwd_valu: x / w");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const int Cout = w.size(0), ks = w.size(2);
  const int Ho = (H + 2 * (ks / 2) - ks) / (int)stride + 1;
  const int Wo = (W + 2 * (ks / 2) - ks) / (int)stride + 1;
  auto y = at::empty({B, Cout, Ho, Wo}, x.options());
  const float* bias_ptr = bias_ptr_f32(bias, x);
  const long long n = (long long)B * Cout * Ho * Wo;
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(x.scalar_type(), [&] {
  DISPATCH_KS_STRIDE(ks, (int)stride, [&] {
    DISPATCH_ACT((int)act, [&] {
      hipLaunchKernelGGL((conv2d_fwd_valu_kernel<elem_t, kKS, kST, kAct>),
                         dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream,
                         n, (const ushort*)x.data_ptr(), (const ushort*)w.data_ptr(),
                         bias_ptr, (ushort*)y.data_ptr(), Cin, H, W, Cout, Ho, Wo);
      return 0;
    });
    return 0;
  });
  return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

// v2 strip kernel for tiny-channel shapes (see kernel comment)
at::Tensor conv2d_fwd_valu2(const at::Tensor& x, const at::Tensor& w,
                            const c10::optional<at::Tensor>& bias,
                            int64_t stride, int64_t act) {
  check_16bit(x, "conv2d_fwd_valu2: x");
  check_16bit(w, "conv2d_fwd_valu2: w");
  check_same_dtype(x, w, "conv2d_fwd_valu2: x / w");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const int Cout = w.size(0), ks = w.size(2);
  TORCH_CHECK(Cin <= 32, "valu2 is for tiny-channel shapes (Cin <= 32)");
  const int Ho = (H + 2 * (ks / 2) - ks) / (int)stride + 1;
  const int Wo = (W + 2 * (ks / 2) - ks) / (int)stride + 1;
  auto y = at::empty({B, Cout, Ho, Wo}, x.options());
  const float* bias_ptr = bias_ptr_f32(bias, x);
  const int coch = Cout >= 8 || Cout > 2 ? 8 : 2;
  const int nsx = (Wo + 7) / 8;
  const long long nstrips = (long long)B * Ho * nsx;
  dim3 grid(esr_grid(nstrips), 1, (Cout + coch - 1) / coch);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(x.scalar_type(), [&] {
  DISPATCH_KS_STRIDE(ks, (int)stride, [&] {
    DISPATCH_ACT((int)act, [&] {
      if (coch == 8)
        hipLaunchKernelGGL((conv2d_fwd_valu2_kernel<elem_t, kKS, kST, kAct, 8>),
                           grid, dim3(256), 0, stream,
                           (const ushort*)x.data_ptr(),
                           (const ushort*)w.data_ptr(), bias_ptr,
                           (ushort*)y.data_ptr(), Cin, H, W, Cout, Ho, Wo,
                           nstrips, nsx);
      else
        hipLaunchKernelGGL((conv2d_fwd_valu2_kernel<elem_t, kKS, kST, kAct, 2>),
                           grid, dim3(256), 0, stream,
                           (const ushort*)x.data_ptr(),
                           (const ushort*)w.data_ptr(), bias_ptr,
                           (ushort*)y.data_ptr(), Cin, H, W, Cout, Ho, Wo,
                           nstrips, nsx);
      return 0;
    });
    return 0;
  });
  return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return y;
}

at::Tensor conv2d_dgrad_s2(const at::Tensor& dy, const at::Tensor& w,
                           int64_t H, int64_t W) {
  check_bf16_4d(dy, "conv2d_dgrad_s2: dy");
  check_bf16_4d(w, "conv2d_dgrad_s2: w");
  const int B = dy.size(0), Cout = dy.size(1), Ho = dy.size(2), Wo = dy.size(3);
  const int Cin = w.size(1), ks = w.size(2);
  TORCH_CHECK(ks == 3, "dgrad_s2 supports 3x3 only");
  auto dx = at::empty({B, Cin, H, W}, dy.options());
  const long long n = (long long)B * Cin * H * W;
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((conv2d_dgrad_s2_valu_kernel<3>),
                     dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream,
                     n, (const ushort*)dy.data_ptr(), (const ushort*)w.data_ptr(),
                     (ushort*)dx.data_ptr(), Cin, (int)H, (int)W, Cout, Ho, Wo);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dx;
}

// stage 1 of the stride-1 weight grad: per-block partial tiles
// [ng][ciblks][coblks][32ci][64co][ntap] fp32
static at::Tensor wgrad_s1_stage1(const at::Tensor& x, const at::Tensor& dpre,
                                  int ks, int Cin_p, int Cout_p, int* ng_out) {
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const int Cout = dpre.size(1);
  const int uw = (W + TW - 1) / TW;
  const int ciblks = (Cin_p + 31) / 32, coblks = (Cout_p + 63) / 64;
  // frames-per-block: accumulate several frames in registers before the
  // flush (partial traffic / fpb) while keeping the grid >= ~1024
  long long nb = (long long)B * uw * ciblks * coblks;
  int fpb = 1;
  while (fpb < 32 && fpb * 2 <= B && nb / (fpb * 2) >= 1024) fpb *= 2;
  static const int abl = [] {
    const char* e = getenv("ESR_WGRAD_ABL");
    return e ? atoi(e) : 0;
  }();
  const int bblks = (B + fpb - 1) / fpb;
  const int ng = bblks * uw;
  const int ntap = ks * ks;
  dim3 grid((unsigned)ng, ciblks, coblks);
  auto part = at::empty({(long long)ng * ciblks * coblks * 32 * 64 * ntap},
                        x.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
  if (ks == 3)
    hipLaunchKernelGGL((conv2d_wgrad_s1_kernel<3>), grid, dim3(256), 0,
                       stream, (const ushort*)x.data_ptr(),
                       (const ushort*)dpre.data_ptr(),
                       part.data_ptr<float>(),
                       Cin, H, W, Cout, Cin_p, Cout_p, uw, B, fpb, abl);
  else
    hipLaunchKernelGGL((conv2d_wgrad_s1_kernel<1>), grid, dim3(256), 0,
                       stream, (const ushort*)x.data_ptr(),
                       (const ushort*)dpre.data_ptr(),
                       part.data_ptr<float>(),
                       Cin, H, W, Cout, Cin_p, Cout_p, uw, B, fpb, abl);
  *ng_out = ng;
  return part;
}

// Stride-1 weight grad, both stages: dW [Cout, Cin, ks, ks] bf16, each
// element the fp32 sum of its partials (stage 2 adds them in block order)
// rounded once.  No zero fill, no padded fp32 result, no permute or cast
// afterwards: two launches.
at::Tensor conv2d_wgrad_s1(const at::Tensor& x, const at::Tensor& dpre,
                           int64_t ks) {
  check_bf16_4d(x, "conv2d_wgrad_s1: x");
  check_bf16_4d(dpre, "conv2d_wgrad_s1: dpre");
  TORCH_CHECK(ks == 1 || ks == 3, "conv2d_wgrad_s1: 3x3 or 1x1 only");
  TORCH_CHECK(x.size(0) == dpre.size(0) && x.size(2) == dpre.size(2) &&
              x.size(3) == dpre.size(3), "conv2d_wgrad_s1: x / dpre shapes");
  const int Cin = x.size(1), Cout = dpre.size(1);
  const int Cin_p = (Cin + 15) / 16 * 16, Cout_p = (Cout + 15) / 16 * 16;
  const int ciblks = (Cin_p + 31) / 32, coblks = (Cout_p + 63) / 64;
  int ng = 0;
  auto part = wgrad_s1_stage1(x, dpre, (int)ks, Cin_p, Cout_p, &ng);
  auto dw = at::empty({Cout, Cin, ks, ks}, x.options());
  // elements of one partial tile set
  const long long n = (long long)ciblks * coblks * 32 * 64 * ks * ks;
  auto stream = at::hip::getCurrentHIPStream();
  if (ks == 3)
    hipLaunchKernelGGL((conv2d_wgrad_reduce_out_kernel<9>),
                       dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream, n,
                       part.data_ptr<float>(), ng, coblks, Cin, Cout,
                       (ushort*)dw.data_ptr());
  else
    hipLaunchKernelGGL((conv2d_wgrad_reduce_out_kernel<1>),
                       dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream, n,
                       part.data_ptr<float>(), ng, coblks, Cin, Cout,
                       (ushort*)dw.data_ptr());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dw;
}

// returns padded fp32 dW [Cout_p, Cin_p, ks, ks]
at::Tensor conv2d_wgrad_mfma(const at::Tensor& x, const at::Tensor& dpre,
                             int64_t ks, int64_t stride,
                             int64_t Cin_p, int64_t Cout_p) {
  check_bf16_4d(x, "conv2d_wgrad: x");
  check_bf16_4d(dpre, "conv2d_wgrad: dpre");
  const int B = x.size(0), Cin = x.size(1), H = x.size(2), W = x.size(3);
  const int Cout = dpre.size(1), Ho = dpre.size(2), Wo = dpre.size(3);
  TORCH_CHECK(Cin_p % 16 == 0 && Cout_p % 16 == 0);
  // TRANSPOSED result [Cin_p, Cout_p, ks, ks]; the python layer permutes
  // back when slicing
  auto dwp = at::zeros({Cin_p, Cout_p, ks, ks},
                       x.options().dtype(at::kFloat));
  const int uw = (W + TW - 1) / TW;
  auto stream = at::hip::getCurrentHIPStream();
  if (stride == 1) {
    const int ciblks = (Cin_p + 31) / 32, coblks = (Cout_p + 63) / 64;
    const int ntap = (int)(ks * ks);
    int ng = 0;
    auto part = wgrad_s1_stage1(x, dpre, (int)ks, (int)Cin_p, (int)Cout_p,
                                &ng);
    const long long nred = (long long)Cin_p * Cout_p * ntap;
    if (ks == 3)
      hipLaunchKernelGGL((conv2d_wgrad_reduce_kernel<9>),
                         dim3(esr_grid(nred)), dim3(ESR_BLOCK), 0, stream,
                         nred, part.data_ptr<float>(), ng, ciblks, coblks,
                         (int)Cin_p, (int)Cout_p, dwp.data_ptr<float>());
    else
      hipLaunchKernelGGL((conv2d_wgrad_reduce_kernel<1>),
                         dim3(esr_grid(nred)), dim3(ESR_BLOCK), 0, stream,
                         nred, part.data_ptr<float>(), ng, ciblks, coblks,
                         (int)Cin_p, (int)Cout_p, dwp.data_ptr<float>());
  } else {
    const int rows_per_blk = 16;
    const long long nslab =
        (long long)B * ((Ho + rows_per_blk - 1) / rows_per_blk) * uw;
    dim3 grid((unsigned)nslab, Cin_p / 16, Cout_p / 16);
    TORCH_CHECK(ks == 3, "stride-2 wgrad supports 3x3 only");
    hipLaunchKernelGGL((conv2d_wgrad_mfma_kernel<3, 2>),
                       grid, dim3(256), 0, stream,
                       (const ushort*)x.data_ptr(), (const ushort*)dpre.data_ptr(),
                       dwp.data_ptr<float>(), Cin, H, W, Cout, Ho, Wo,
                       (int)Cin_p, (int)Cout_p, rows_per_blk);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dwp;
}

at::Tensor act_grad(const at::Tensor& dy, const at::Tensor& y, int64_t act) {
  check_16bit(dy, "act_grad: dy");
  check_16bit(y, "act_grad: y");
  check_same_dtype(dy, y, "act_grad: dy / y");
  TORCH_CHECK(dy.numel() == y.numel(), "act_grad: dy and y sizes differ");
  auto dpre = at::empty_like(dy);
  const long long n = dy.numel();
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(dy.scalar_type(), [&] {
  DISPATCH_ACT((int)act, [&] {
    if (kAct == 0) { dpre.copy_(dy); return 0; }
    hipLaunchKernelGGL((act_grad_kernel<elem_t, kAct>),
                       dim3(esr_grid(n)), dim3(ESR_BLOCK), 0, stream,
                       n, (const ushort*)dy.data_ptr(),
                       (const ushort*)y.data_ptr(), (ushort*)dpre.data_ptr());
    return 0;
  });
  return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dpre;
}

int64_t bias_grad_chunk() { return BG_CHUNK; }

// longest chain of dependent fp32 additions behind one db element of
// act_grad_bias / bias_grad for a [B,C,H,W] gradient (formula: see
// act_grad_bias_kernel)
int64_t bias_grad_chain(int64_t B, int64_t H, int64_t W) {
  const int64_t P = (B * H * W + BG_CHUNK - 1) / BG_CHUNK;
  return 8 * BG_VPT + 18 + (P + ESR_BLOCK - 1) / ESR_BLOCK;
}

// shared body: dy [B,C,H,W] bf16|fp16 (y likewise when act != 0).  Returns
// {dpre (only when store), db [C] in dy's dtype, and with want_f32 the fp32
// sums [C] before the rounding}.  No host sync; scratch from at::empty
// (capture-safe).  A shape past the limits below is an error, not a
// fall-back to torch's sum.
static std::vector<at::Tensor> bias_grad_impl(const at::Tensor& dy,
                                              const at::Tensor* y,
                                              int64_t act, bool store,
                                              bool want_f32,
                                              const char* name) {
  check_16bit(dy, name);
  TORCH_CHECK(dy.dim() == 4, name, ": [B,C,H,W] tensor required");
  TORCH_CHECK(act >= 0 && act <= 3, name, ": act id ", act);
  if (act != 0) {
    check_16bit(*y, name);
    check_same_dtype(dy, *y, name);
    TORCH_CHECK(dy.sizes() == y->sizes(), name, ": dy and y sizes differ");
  }
  const int64_t B = dy.size(0), C = dy.size(1), HW = dy.size(2) * dy.size(3);
  const int64_t L = B * HW;
  TORCH_CHECK(L > 0 && C > 0, name, ": empty tensor");
  TORCH_CHECK(L < (1LL << 31) - BG_CHUNK, name,
              ": B*H*W per channel must stay below 2^31, got ", L);
  TORCH_CHECK(bias_grad_chain(B, dy.size(2), dy.size(3)) <= 2048, name,
              ": fp32 summation chain above 2^11");
  const int64_t P = (L + BG_CHUNK - 1) / BG_CHUNK;
  at::Tensor dpre;
  if (store) dpre = at::empty_like(dy);
  auto f32 = dy.options().dtype(at::kFloat);
  auto part = at::empty({C * P}, f32);
  at::Tensor sum32;
  if (want_f32) sum32 = at::empty({C}, f32);
  auto db = at::empty({C}, dy.options());
  const ushort* yp = act != 0 ? (const ushort*)y->data_ptr() : nullptr;
  ushort* dp = store ? (ushort*)dpre.data_ptr() : nullptr;
  // 16-byte path: planes 16-byte aligned relative to 16-byte aligned bases
  const bool vec = HW % 8 == 0 && (uintptr_t)dy.data_ptr() % 16 == 0 &&
                   (uintptr_t)yp % 16 == 0 && (uintptr_t)dp % 16 == 0;
  const long long nitem = C * P;
  const int grid = (int)(nitem < ESR_MAX_BLOCKS ? nitem : ESR_MAX_BLOCKS);
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(dy.scalar_type(), [&] {
    DISPATCH_ACT((int)act, [&] {
      auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(ESR_BLOCK), 0, stream,
                           (int)C, (unsigned int)HW, (unsigned int)L,
                           (unsigned int)P, vec,
                           (const ushort*)dy.data_ptr(), yp, dp,
                           part.data_ptr<float>());
      };
      if (store) launch(act_grad_bias_kernel<elem_t, kAct, true>);
      else launch(act_grad_bias_kernel<elem_t, kAct, false>);
      return 0;
    });
    hipLaunchKernelGGL(bias_grad_reduce_kernel<elem_t>, dim3((int)C),
                       dim3(ESR_BLOCK), 0, stream, (unsigned int)P,
                       part.data_ptr<float>(),
                       want_f32 ? sum32.data_ptr<float>() : nullptr,
                       (ushort*)db.data_ptr());
    return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  std::vector<at::Tensor> out;
  if (store) out.push_back(dpre);
  out.push_back(db);
  if (want_f32) out.push_back(sum32);
  return out;
}

// {dpre, db[, fp32 sums]}: dpre bit-equal to act_grad(dy, y, act), db its
// per-channel sum
std::vector<at::Tensor> act_grad_bias(const at::Tensor& dy,
                                      const at::Tensor& y, int64_t act,
                                      bool want_f32) {
  TORCH_CHECK(act != 0, "act_grad_bias: act 0 has no dpre to write, "
              "use bias_grad");
  return bias_grad_impl(dy, &y, act, true, want_f32, "act_grad_bias");
}

// {db[, fp32 sums]} of a conv without activation: read-only pass over dy
std::vector<at::Tensor> bias_grad(const at::Tensor& dy, bool want_f32) {
  return bias_grad_impl(dy, nullptr, 0, false, want_f32, "bias_grad");
}

at::Tensor gemm16_probe(const at::Tensor& A, const at::Tensor& B) {
  check_16bit(A, "gemm16_probe: A");
  check_16bit(B, "gemm16_probe: B");
  check_same_dtype(A, B, "gemm16_probe: A / B");
  TORCH_CHECK(A.sizes() == at::IntArrayRef({16, 32}) &&
              B.sizes() == at::IntArrayRef({32, 16}),
              "probe: A[16,32] B[32,16]");
  auto C = at::empty({16, 16}, A.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
  DISPATCH_ELEM(A.scalar_type(), [&] {
    hipLaunchKernelGGL(gemm16_probe_kernel<elem_t>, dim3(1), dim3(64), 0,
                       stream, (const ushort*)A.data_ptr(),
                       (const ushort*)B.data_ptr(), C.data_ptr<float>());
    return 0;
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return C;
}
