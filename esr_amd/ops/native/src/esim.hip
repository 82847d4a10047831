// Log frames -> event rows on gfx950: the device form of
// data/simulate.py's simulate_events_log (the oracle; the two agree bit for
// bit, order included).  data/simulate_device.py drives the stages below.
//
// The work is parallel over pixels and sequential in time: one thread walks
// one pixel through the intervals of a slab [S, H, W] of float64 log frames
// with l0, ref and t_last in registers.  Per-pixel state (ref, t_last:
// float64 [H*W]) stays on the device between calls.
//
//   esim_count   the walk on a private copy of the state: events per pixel,
//                and into stats the largest crossing count of one pixel and
//                interval and the bad-input flag.  No side effect on the
//                state, so the caller may repeat it over fewer intervals
//                when the total does not fit its chunk.
//   esim_scan    int64 hipCUB ExclusiveSum of the counts; stats[0] = total.
//   esim_emit    the same walk, committing ref and t_last; writes t and the
//                tie-break key (k_local, pol, i, pixel) at the pixel's offset.
//   esim_sort    0: SortPairs by the tie-break key on the bits in use;
//                   then the pack_events word (x | y << 15 | sign << 31) is
//                   made from each key;
//                1: stable SortPairs by t (float64 keys), carrying the words.
//                Together: the oracle's order (t, k, + before -, i, y, x).
//   esim_unpack  the four typed columns (uint16 x, y; float64 t; int8 p).
//
// Arithmetic: float64, one rounding per operation and nothing contracted into
// an fma (es_add / es_sub / es_mul / es_div below), in numpy's order.
//
// Bounds: no index or loop bound depends on an unclamped value.  Crossings
// per pixel and interval are clamped to 65535 and a non-finite dl counts as
// zero crossings; either raises the flag.  Every slot is checked against the
// capacity of the chunk before it is written.  The keys index nothing.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hipcub/hipcub.hpp>
#include <limits>
#include "esr_common.h"

// The oracle rounds every operation.  The __dadd_rn / __dmul_rn intrinsics do
// not guarantee that here: their bodies in the compiler's header are plain
// operators compiled with contraction allowed, and `__dadd_rn(a,
// __dmul_rn(b, c))` comes out as one v_fmac_f64 (checked in the ISA).  Plain
// operators with contraction switched off for this file give v_mul_f64 and
// v_add_f64; the division is the IEEE sequence either way.
#pragma clang fp contract(off)

namespace {

ESR_INLINE double es_add(double a, double b) { return a + b; }
ESR_INLINE double es_sub(double a, double b) { return a - b; }
ESR_INLINE double es_mul(double a, double b) { return a * b; }
ESR_INLINE double es_div(double a, double b) { return a / b; }

constexpr int ES_MAX_DIM = 32767;
constexpr int ES_MAX_CROSS = 65535;
constexpr int ES_MAX_INTERVALS = 4096;       // 4096 * 65535 < 2^31 per pixel
constexpr long long ES_MAX_CAPACITY = 1ll << 30;

// stats layout (int64)
constexpr int ST_TOTAL = 0, ST_MAX_CROSS = 1, ST_BAD = 2, ST_LEN = 3;

// floor(m / c) for m >= 0 finite and c > 0, clamped to ES_MAX_CROSS
ESR_INLINE int es_crossings(double m, double c, bool& bad) {
  const double q = es_div(m, c);
  // compared as doubles: q may be +inf or far outside the int range
  if (!(q < (double)(ES_MAX_CROSS + 1))) {
    bad = true;
    return ES_MAX_CROSS;
  }
  return (int)floor(q);                      // 0 <= q < 65536
}

struct EsWalk {
  long long npix;
  const double* logf;    // [S, npix]
  const double* ts;      // [S]
  int k0, nint;          // intervals k0+1 .. k0+nint of the slab
  double cp, cn, refractory;
};

// One pixel through the walk's intervals.  EMIT = false counts on a private
// copy of the state; EMIT = true writes the events and commits the state.
template <bool EMIT>
__global__ void esim_walk_kernel(EsWalk w, double* __restrict__ ref_state,
                                 double* __restrict__ tl_state,
                                 int* __restrict__ counts,
                                 unsigned long long* __restrict__ stats,
                                 const long long* __restrict__ offs,
                                 long long capacity, int pix_bits, int i_bits,
                                 unsigned long long* __restrict__ keys,
                                 double* __restrict__ tv) {
  const bool use_ref = w.refractory > 0.0;
  ESR_KERNEL_LOOP(p, w.npix) {
    double ref = ref_state[p], tl = tl_state[p];
    double l0 = w.logf[(long long)w.k0 * w.npix + p];
    const long long base = EMIT ? offs[p] : 0;
    int cnt = 0, max_cross = 0;
    bool bad = false;
    for (int j = 1; j <= w.nint; ++j) {
      const double l1 = w.logf[(long long)(w.k0 + j) * w.npix + p];
      const double t0 = w.ts[w.k0 + j - 1], t1 = w.ts[w.k0 + j];
      const double dl = es_sub(l1, ref);
      int n_pos = 0, n_neg = 0;
      if (!isfinite(dl)) {
        bad = true;
      } else {
        n_pos = es_crossings(dl > 0.0 ? dl : 0.0, w.cp, bad);
        n_neg = es_crossings(dl < 0.0 ? -dl : 0.0, w.cn, bad);
      }
      // dl has one sign: at most one of the two is non-zero
      const int n = n_pos > n_neg ? n_pos : n_neg;
      max_cross = n > max_cross ? n : max_cross;
      if (n > 0 && !EMIT && !use_ref) {
        cnt += n;
      } else if (n > 0) {
        const bool neg = n_neg > 0;
        const double step = neg ? -w.cn : w.cp;          // pol * C
        const double den = es_sub(l1, l0);
        const bool moving = fabs(den) > 1e-12;
        const double dt = es_sub(t1, t0);
        for (int i = 1; i <= n; ++i) {
          const double target = es_add(ref, es_mul(step, (double)i));
          double frac = moving ? es_div(es_sub(target, l0), den) : 0.5;
          frac = frac < 0.0 ? 0.0 : frac;
          frac = frac > 1.0 ? 1.0 : frac;
          const double t = es_add(t0, es_mul(frac, dt));
          // tl = -inf until the pixel's first event: the gap is then +inf
          if (use_ref && !(es_sub(t, tl) >= w.refractory)) continue;
          tl = t;
          if (EMIT) {
            const long long slot = base + cnt;
            if (slot >= 0 && slot < capacity) {
              keys[slot] =
                  ((unsigned long long)(j - 1) << (pix_bits + i_bits + 1)) |
                  ((unsigned long long)(neg ? 1 : 0) << (pix_bits + i_bits)) |
                  ((unsigned long long)i << pix_bits) | (unsigned long long)p;
              tv[slot] = t;
            }
          }
          ++cnt;
        }
      }
      ref = es_sub(es_add(ref, es_mul((double)n_pos, w.cp)),
                   es_mul((double)n_neg, w.cn));
      l0 = l1;
    }
    if (EMIT) {
      ref_state[p] = ref;
      tl_state[p] = tl;
    } else {
      counts[p] = cnt;
      if (max_cross > 0)
        atomicMax(&stats[ST_MAX_CROSS], (unsigned long long)max_cross);
      if (bad) atomicOr(&stats[ST_BAD], 1ull);
    }
  }
}

struct EsWiden {
  __host__ __device__ long long operator()(int v) const { return v; }
};
using EsWidenIt = hipcub::TransformInputIterator<long long, EsWiden, const int*>;

__global__ void esim_total_kernel(long long npix, const int* __restrict__ counts,
                                  const long long* __restrict__ offs,
                                  long long* __restrict__ stats) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  stats[ST_TOTAL] = offs[npix - 1] + counts[npix - 1];
}

// tie-break keys in sorted order -> pack_events words
__global__ void esim_word_kernel(long long total, int W, int pix_bits,
                                 int i_bits,
                                 const unsigned long long* __restrict__ keys,
                                 unsigned* __restrict__ words) {
  const unsigned long long pix_mask = (1ull << pix_bits) - 1ull;
  ESR_KERNEL_LOOP(r, total) {
    const unsigned long long key = keys[r];
    const unsigned long long pix = key & pix_mask;
    const unsigned x = (unsigned)(pix % (unsigned long long)W) & 0x7fffu;
    const unsigned y = (unsigned)(pix / (unsigned long long)W) & 0x7fffu;
    const unsigned neg = (unsigned)((key >> (pix_bits + i_bits)) & 1ull);
    words[r] = x | (y << 15) | (neg << 31);
  }
}

__global__ void esim_unpack_kernel(long long total, long long rows,
                                   const double* __restrict__ tv,
                                   const unsigned* __restrict__ words,
                                   unsigned short* __restrict__ xs,
                                   unsigned short* __restrict__ ys,
                                   double* __restrict__ ts,
                                   signed char* __restrict__ ps) {
  ESR_KERNEL_LOOP(r, total) {
    if (r >= rows) continue;                  // the chunk is never overrun
    const unsigned p = words[r];
    xs[r] = (unsigned short)(p & 0x7fffu);
    ys[r] = (unsigned short)((p >> 15) & 0x7fffu);
    ts[r] = tv[r];
    ps[r] = (p >> 31) ? (signed char)-1 : (signed char)1;
  }
}

size_t es_scan_bytes(long long npix) {
  size_t bytes = 0;
  EsWidenIt in(nullptr, EsWiden());
  hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, (long long*)nullptr,
                                   (int)npix, (hipStream_t)0);
  return bytes;
}

size_t es_key_sort_bytes(long long n) {
  size_t bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(
      nullptr, bytes, (const unsigned long long*)nullptr,
      (unsigned long long*)nullptr, (const double*)nullptr, (double*)nullptr,
      (int)n, 0, 64, (hipStream_t)0);
  return bytes;
}

size_t es_time_sort_bytes(long long n) {
  size_t bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(
      nullptr, bytes, (const double*)nullptr, (double*)nullptr,
      (const unsigned*)nullptr, (unsigned*)nullptr, (int)n, 0, 64,
      (hipStream_t)0);
  return bytes;
}

// A chunk sorts `total` <= capacity items and the library picks its method
// by size: take the largest need over capacity, capacity/2, ...; esim_sort
// checks the need of the size it sorts against what was allocated.
size_t es_sort_bytes(long long capacity) {
  size_t need = 0;
  for (long long n = capacity; n > 0; n >>= 1) {
    const size_t a = es_key_sort_bytes(n), b = es_time_sort_bytes(n);
    need = a > need ? a : need;
    need = b > need ? b : need;
  }
  return need;
}

void es_check_sizes(int64_t npix, int64_t capacity) {
  TORCH_CHECK(npix >= 1 && npix <= (int64_t)ES_MAX_DIM * ES_MAX_DIM,
              "esim: the pixel count must lie in [1, 32767^2]");
  TORCH_CHECK(capacity >= 1 && capacity <= ES_MAX_CAPACITY,
              "esim: capacity must lie in [1, 2^30]");
}

bool es_on(const at::Tensor& t, int dev, at::ScalarType st) {
  return t.is_cuda() && t.get_device() == dev && t.scalar_type() == st &&
         t.is_contiguous();
}

// scratch = {counts int32 [>= npix], offsets int64 [>= npix], keys int64
// [2, capacity], t float64 [2, capacity], words int32 [2, capacity], hipCUB
// temporary storage uint8}; returns the capacity.
int64_t es_check_scratch(const std::vector<at::Tensor>& s, int dev,
                         int64_t npix) {
  TORCH_CHECK(s.size() == 6 && es_on(s[0], dev, at::kInt) &&
              es_on(s[1], dev, at::kLong) && es_on(s[2], dev, at::kLong) &&
              es_on(s[3], dev, at::kDouble) && es_on(s[4], dev, at::kInt) &&
              es_on(s[5], dev, at::kByte) && s[2].dim() == 2 &&
              s[2].size(0) == 2,
              "esim: scratch must come from esim_scratch on this device");
  const int64_t capacity = s[2].size(1);
  es_check_sizes(npix, capacity);
  TORCH_CHECK(s[0].numel() >= npix && s[1].numel() >= npix &&
              s[3].numel() == 2 * capacity && s[4].numel() == 2 * capacity &&
              (size_t)s[5].numel() >= es_scan_bytes(npix),
              "esim: scratch does not fit this frame size (esim_scratch)");
  return capacity;
}

EsWalk es_check_walk(const at::Tensor& logf, const at::Tensor& ts,
                     const at::Tensor& ref, const at::Tensor& t_last,
                     int64_t k0, int64_t nint, double cp, double cn,
                     double refractory) {
  TORCH_CHECK(logf.is_cuda() && logf.scalar_type() == at::kDouble &&
              logf.is_contiguous() && logf.dim() == 3,
              "esim: contiguous float64 [S,H,W] log frames required");
  const int dev = logf.get_device();
  const int64_t S = logf.size(0), H = logf.size(1), W = logf.size(2);
  TORCH_CHECK(H >= 1 && W >= 1 && H <= ES_MAX_DIM && W <= ES_MAX_DIM,
              "esim: H and W must lie in [1, 32767]");
  const int64_t npix = H * W;
  TORCH_CHECK(es_on(ts, dev, at::kDouble) && ts.dim() == 1 &&
              ts.size(0) == S,
              "esim: ts must be float64 [S] on the frames' device");
  TORCH_CHECK(es_on(ref, dev, at::kDouble) && ref.numel() == npix &&
              es_on(t_last, dev, at::kDouble) && t_last.numel() == npix,
              "esim: ref and t_last must be float64 [H,W] on the frames' "
              "device");
  TORCH_CHECK(nint >= 1 && nint <= ES_MAX_INTERVALS && k0 >= 0 &&
              k0 + nint <= S - 1,
              "esim: intervals k0+1..k0+nint must lie in the slab, at most ",
              ES_MAX_INTERVALS, " of them");
  TORCH_CHECK(cp > 0.0 && cn > 0.0 && refractory >= 0.0,
              "esim: cp, cn > 0 and refractory >= 0 required");
  EsWalk w;
  w.npix = npix;
  w.logf = logf.data_ptr<double>();
  w.ts = ts.data_ptr<double>();
  w.k0 = (int)k0;
  w.nint = (int)nint;
  w.cp = cp;
  w.cn = cn;
  w.refractory = refractory;
  return w;
}

}  // namespace

// Scratch for frames of up to `npix` pixels and chunks of up to `capacity`
// events, allocated once by the caller (layout: es_check_scratch).
std::vector<at::Tensor> esim_scratch(const at::Tensor& like, int64_t npix,
                                     int64_t capacity) {
  TORCH_CHECK(like.is_cuda(), "esim_scratch: a device tensor is required");
  es_check_sizes(npix, capacity);
  auto opt = like.options();
  const size_t a = es_scan_bytes(npix), b = es_sort_bytes(capacity);
  const long long tmp = (long long)(a > b ? a : b);
  return {at::zeros({npix}, opt.dtype(at::kInt)),
          at::zeros({npix}, opt.dtype(at::kLong)),
          at::zeros({2, capacity}, opt.dtype(at::kLong)),
          at::zeros({2, capacity}, opt.dtype(at::kDouble)),
          at::zeros({2, capacity}, opt.dtype(at::kInt)),
          at::zeros({tmp > 0 ? tmp : 1}, opt.dtype(at::kByte))};
}

// Events per pixel over intervals k0+1..k0+nint of the slab, from the state
// but without changing it.  stats int64 [3] = {total (esim_scan), largest
// crossing count of one pixel and interval, bad-input flag} is reset first.
void esim_count(const at::Tensor& logf, const at::Tensor& ts,
                const at::Tensor& ref, const at::Tensor& t_last, int64_t k0,
                int64_t nint, double cp, double cn, double refractory,
                const std::vector<at::Tensor>& scratch, at::Tensor& stats) {
  EsWalk w = es_check_walk(logf, ts, ref, t_last, k0, nint, cp, cn,
                           refractory);
  const int dev = logf.get_device();
  es_check_scratch(scratch, dev, w.npix);
  TORCH_CHECK(es_on(stats, dev, at::kLong) && stats.dim() == 1 &&
              stats.size(0) == ST_LEN, "esim: stats must be int64 [3]");
  auto stream = at::hip::getCurrentHIPStream();
  C10_HIP_CHECK(hipMemsetAsync(stats.data_ptr(), 0, ST_LEN * sizeof(int64_t),
                               stream));
  hipLaunchKernelGGL(esim_walk_kernel<false>, dim3(esr_grid(w.npix)),
                     dim3(ESR_BLOCK), 0, stream, w,
                     (double*)ref.data_ptr<double>(),
                     (double*)t_last.data_ptr<double>(),
                     scratch[0].data_ptr<int>(),
                     (unsigned long long*)stats.data_ptr<int64_t>(),
                     (const long long*)nullptr, 0ll, 0, 0,
                     (unsigned long long*)nullptr, (double*)nullptr);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// Offsets of the first `npix` counts and stats[0] = their total.
void esim_scan(int64_t npix, const std::vector<at::Tensor>& scratch,
               at::Tensor& stats) {
  TORCH_CHECK(stats.is_cuda(), "esim: stats must be on the device");
  const int dev = stats.get_device();
  es_check_scratch(scratch, dev, npix);
  TORCH_CHECK(es_on(stats, dev, at::kLong) && stats.dim() == 1 &&
              stats.size(0) == ST_LEN, "esim: stats must be int64 [3]");
  auto stream = at::hip::getCurrentHIPStream();
  const int* counts = scratch[0].data_ptr<int>();
  long long* offs = (long long*)scratch[1].data_ptr<int64_t>();
  size_t bytes = es_scan_bytes(npix);
  EsWidenIt in(counts, EsWiden());
  C10_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(scratch[5].data_ptr(), bytes,
                                                 in, offs, (int)npix, stream));
  hipLaunchKernelGGL(esim_total_kernel, dim3(1), dim3(64), 0, stream,
                     (long long)npix, counts, offs,
                     (long long*)stats.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// The walk esim_count made, now writing (key, t) at each pixel's offset and
// committing ref and t_last.  max_cross is what esim_count reported; it sets
// the width of the key's i field.  Returns {pix_bits, i_bits, key_bits}.
std::vector<int64_t> esim_emit(const at::Tensor& logf, const at::Tensor& ts,
                               at::Tensor& ref, at::Tensor& t_last, int64_t k0,
                               int64_t nint, double cp, double cn,
                               double refractory, int64_t max_cross,
                               const std::vector<at::Tensor>& scratch) {
  EsWalk w = es_check_walk(logf, ts, ref, t_last, k0, nint, cp, cn,
                           refractory);
  const int64_t capacity = es_check_scratch(scratch, logf.get_device(), w.npix);
  TORCH_CHECK(max_cross >= 0 && max_cross <= ES_MAX_CROSS,
              "esim: max_cross must lie in [0, 65535]");
  int pix_bits = 0, i_bits = 0, k_bits = 0;
  for (long long v = w.npix - 1; v > 0; v >>= 1) ++pix_bits;
  for (long long v = max_cross; v > 0; v >>= 1) ++i_bits;
  for (long long v = nint - 1; v > 0; v >>= 1) ++k_bits;
  const int key_bits = pix_bits + i_bits + 1 + k_bits;   // <= 30+16+1+12
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(esim_walk_kernel<true>, dim3(esr_grid(w.npix)),
                     dim3(ESR_BLOCK), 0, stream, w, ref.data_ptr<double>(),
                     t_last.data_ptr<double>(), (int*)nullptr,
                     (unsigned long long*)nullptr,
                     (const long long*)scratch[1].data_ptr<int64_t>(),
                     (long long)capacity, pix_bits, i_bits,
                     (unsigned long long*)scratch[2].data_ptr<int64_t>(),
                     scratch[3].data_ptr<double>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {pix_bits, i_bits, key_bits};
}

// which = 0: sort the first `total` (key, t) pairs by key on bits
// [0, key_bits) and make the words; which = 1: sort (t, word) stably by t.
void esim_sort(int64_t which, int64_t total, int64_t W, int64_t pix_bits,
               int64_t i_bits, int64_t key_bits,
               const std::vector<at::Tensor>& scratch) {
  TORCH_CHECK(scratch.size() == 6 && scratch[2].is_cuda(),
              "esim: scratch must come from esim_scratch");
  const int64_t capacity = es_check_scratch(scratch, scratch[2].get_device(), 1);
  TORCH_CHECK(total >= 1 && total <= capacity,
              "esim_sort: total must lie in [1, capacity]");
  TORCH_CHECK(W >= 1 && W <= ES_MAX_DIM && pix_bits >= 0 && pix_bits <= 30 &&
              i_bits >= 0 && i_bits <= 16 && key_bits >= pix_bits + i_bits + 1 &&
              key_bits <= 64, "esim_sort: key layout out of range");
  auto stream = at::hip::getCurrentHIPStream();
  unsigned long long* keys = (unsigned long long*)scratch[2].data_ptr<int64_t>();
  double* tv = scratch[3].data_ptr<double>();
  unsigned* words = (unsigned*)scratch[4].data_ptr<int>();
  size_t bytes = (size_t)scratch[5].numel();
  TORCH_CHECK(which == 0 || which == 1, "esim_sort: which is 0 or 1");
  TORCH_CHECK((which == 0 ? es_key_sort_bytes(total)
                          : es_time_sort_bytes(total)) <= bytes,
              "esim_sort: temporary storage too small (esim_scratch)");
  if (which == 0) {
    C10_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
        scratch[5].data_ptr(), bytes, (const unsigned long long*)keys,
        keys + capacity, (const double*)tv, tv + capacity, (int)total, 0,
        (int)key_bits, stream));
    hipLaunchKernelGGL(esim_word_kernel, dim3(esr_grid(total)),
                       dim3(ESR_BLOCK), 0, stream, (long long)total, (int)W,
                       (int)pix_bits, (int)i_bits, keys + capacity, words);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    C10_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
        scratch[5].data_ptr(), bytes, (const double*)(tv + capacity), tv,
        (const unsigned*)words, words + capacity, (int)total, 0, 64, stream));
  }
}

// The first `total` sorted (t, word) pairs -> cols = {xs uint16, ys uint16,
// ts float64, ps int8}, each [rows], rows >= total.
void esim_unpack(int64_t total, const std::vector<at::Tensor>& scratch,
                 const std::vector<at::Tensor>& cols) {
  TORCH_CHECK(scratch.size() == 6 && scratch[2].is_cuda(),
              "esim: scratch must come from esim_scratch");
  const int dev = scratch[2].get_device();
  const int64_t capacity = es_check_scratch(scratch, dev, 1);
  TORCH_CHECK(cols.size() == 4 && es_on(cols[0], dev, at::kUInt16) &&
              es_on(cols[1], dev, at::kUInt16) &&
              es_on(cols[2], dev, at::kDouble) && es_on(cols[3], dev, at::kChar),
              "esim_unpack: cols must be xs uint16, ys uint16, ts float64, "
              "ps int8 on the scratch's device");
  const int64_t rows = cols[0].numel();
  for (const auto& c : cols)
    TORCH_CHECK(c.dim() == 1 && c.numel() == rows,
                "esim_unpack: the four columns must have one length");
  TORCH_CHECK(total >= 1 && total <= capacity && total <= rows,
              "esim_unpack: total must lie in [1, min(capacity, rows)]");
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(esim_unpack_kernel, dim3(esr_grid(total)),
                     dim3(ESR_BLOCK), 0, stream, (long long)total,
                     (long long)rows, scratch[3].data_ptr<double>(),
                     (const unsigned*)scratch[4].data_ptr<int>() + capacity,
                     (unsigned short*)cols[0].data_ptr(),
                     (unsigned short*)cols[1].data_ptr(),
                     cols[2].data_ptr<double>(),
                     (signed char*)cols[3].data_ptr<int8_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}
