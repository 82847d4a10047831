// Count map -> event rows for a FILE, on gfx950: the emission stage of
// engine/superresolve.py.  One call turns one predicted window [2, kH, kW]
// into rows appended to a chunk of the four typed EVS columns, fully on the
// device: no allocation, no host synchronisation, so the call records into
// a hipGraph.  redistribute.hip stays the serving path's conversion; what
// differs here and why:
//
//   * counts are clamped to [0, cell_cap] in the FIRST kernel (NaN -> 0,
//     +inf -> cell_cap); nothing later reads the prediction again, so no
//     index or loop bound ever depends on an unclamped value;
//   * offsets are an int64 scan (2 * 32767^2 cells of 65535 overflow int32);
//   * the sort key is an integer phase q in [0, Q], Q = 2^20, not an fp32
//     timestamp: order and ties are the same on any machine, and the
//     timestamp is rebuilt from q in float64 on the recording's own clock;
//   * the payload is the pack_events word (15-bit x and y, sign in bit 31);
//   * rows are appended at a device-side cursor and the window's
//     total / emitted / dropped are written next to it: overflow is counted.
//
// Semantics (the torch oracle is emit_window_torch, engine/superresolve.py;
// the two agree bit for bit):
//   cell   c = (ch*kH + y)*kW + x,  n_c = isnan(v) ? 0 : clamp(rint(v), 0, cap)
//   slot   o_c + j (o = exclusive int64 sum of n), kept iff slot < capacity
//   phase  linear: n_c == 1 ? 0 : j*Q / (n_c-1);  random: hash % (Q+1)
//   order  stable sort of the kept slots by q
//   ts     min(max(t0 + (t1-t0) * (double(Q + 99q) / double(100Q)), t0), t1),
//          every operation rounded once (no fma contraction)
//
// Pipeline: counts -> hipCUB ExclusiveSum -> emit (one thread per cell, as
// redist_scatter_kernel) -> hipCUB SortPairs on bits 0..21 (bit 21 marks the
// unused tail of the capacity, which therefore sorts last) -> append -> tail.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hipcub/hipcub.hpp>
#include <limits>
#include "esr_common.h"

namespace {

constexpr int SR_Q_BITS = 20;
constexpr long long SR_Q = 1ll << SR_Q_BITS;
constexpr unsigned SR_PAD_KEY = 1u << (SR_Q_BITS + 1);   // above every phase
constexpr int SR_SORT_BITS = SR_Q_BITS + 2;
constexpr int SR_MAX_DIM = 32767;
constexpr int SR_MAX_CELL_CAP = 65535;
constexpr long long SR_MAX_CAPACITY = 1ll << 30;

// cursor_stats layout (int64)
constexpr int CS_CURSOR = 0, CS_TOTAL = 1, CS_EMITTED = 2, CS_DROPPED = 3,
              CS_WINDOW = 4, CS_LEN = 5;

ESR_INLINE int sr_cell_count(float v, int cell_cap) {
  if (v != v) return 0;                       // NaN
  const float r = rintf(v);                   // halves to even, +-inf stay
  // compared as floats: r may be +-inf or far outside the int range
  if (!(r > 0.0f)) return 0;
  if (r >= (float)cell_cap) return cell_cap;
  return (int)r;                              // 0 < r < cell_cap <= 65535
}

__global__ void sr_counts_kernel(long long n, const float* __restrict__ pred,
                                 int cell_cap, int* __restrict__ counts) {
  ESR_KERNEL_LOOP(i, n) counts[i] = sr_cell_count(pred[i], cell_cap);
}

struct SrWiden {
  __host__ __device__ long long operator()(int v) const { return v; }
};

// murmur3's 32-bit finaliser
ESR_INLINE unsigned sr_fmix(unsigned h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// phase of event j of cell c in window `widx`; all arithmetic modulo 2^32
ESR_INLINE unsigned sr_hash_phase(unsigned seed, unsigned widx, unsigned c,
                                  unsigned j) {
  unsigned h = sr_fmix(seed + widx * 0x9e3779b9u);
  h = sr_fmix(h ^ c);
  h = sr_fmix(h + j * 0x9e3779b9u);
  return h % (unsigned)(SR_Q + 1);
}

ESR_INLINE long long sr_total(long long ncells, const int* counts,
                              const long long* offs) {
  return offs[ncells - 1] + counts[ncells - 1];
}

// One thread per cell writes the cell's kept slots; the same grid then marks
// the slots past the window's events, so the sort sees `capacity` keys.
__global__ void sr_emit_kernel(long long ncells, int kH, int kW,
                               const int* __restrict__ counts,
                               const long long* __restrict__ offs,
                               long long capacity, int mode, unsigned seed,
                               const long long* __restrict__ cursor_stats,
                               unsigned* __restrict__ keys,
                               unsigned* __restrict__ payload) {
  const unsigned widx = (unsigned)cursor_stats[CS_WINDOW];
  const long long plane = (long long)kH * kW;
  ESR_KERNEL_LOOP(i, ncells) {
    const int n = counts[i];
    if (!n) continue;
    const long long base = offs[i];
    if (base >= capacity) continue;
    const long long r = i % plane;
    const unsigned x = (unsigned)(r % kW), y = (unsigned)(r / kW);
    const unsigned pay = x | (y << 15) | (i >= plane ? 0x80000000u : 0u);
    const long long keep = capacity - base < n ? capacity - base : n;
    for (long long j = 0; j < keep; ++j) {
      unsigned q;
      if (mode == 0) {
        q = n == 1 ? 0u : (unsigned)((j * SR_Q) / (n - 1));
      } else {
        q = sr_hash_phase(seed, widx, (unsigned)i, (unsigned)j);
      }
      keys[base + j] = q;
      payload[base + j] = pay;
    }
  }
  const long long total = sr_total(ncells, counts, offs);
  ESR_KERNEL_LOOP(s, capacity) {
    if (s >= total) {
      keys[s] = SR_PAD_KEY;
      payload[s] = 0u;
    }
  }
}

ESR_INLINE double sr_timestamp(double t0, double t1, unsigned q) {
  // __d*_rn: one rounding per operation, never contracted into an fma
  const double frac = __ddiv_rn((double)(SR_Q + 99ll * (long long)q),
                                (double)(100ll * SR_Q));
  double t = __dadd_rn(t0, __dmul_rn(__dsub_rn(t1, t0), frac));
  t = t < t0 ? t0 : t;
  t = t > t1 ? t1 : t;
  return t;
}

__global__ void sr_append_kernel(long long ncells, long long capacity,
                                 long long rows,
                                 const int* __restrict__ counts,
                                 const long long* __restrict__ offs,
                                 const unsigned* __restrict__ keys,
                                 const unsigned* __restrict__ payload,
                                 const double* __restrict__ win,
                                 const long long* __restrict__ cursor_stats,
                                 unsigned short* __restrict__ xs,
                                 unsigned short* __restrict__ ys,
                                 double* __restrict__ ts,
                                 signed char* __restrict__ ps) {
  const long long total = sr_total(ncells, counts, offs);
  const long long emitted = total < capacity ? total : capacity;
  const long long cursor = cursor_stats[CS_CURSOR];
  const double t0 = win[0], t1 = win[1];
  ESR_KERNEL_LOOP(i, emitted) {
    const long long row = cursor + i;
    if (row < 0 || row >= rows) continue;     // the chunk is never overrun
    const unsigned p = payload[i];
    xs[row] = (unsigned short)(p & 0x7fffu);
    ys[row] = (unsigned short)((p >> 15) & 0x7fffu);
    ts[row] = sr_timestamp(t0, t1, keys[i]);
    ps[row] = (p >> 31) ? (signed char)-1 : (signed char)1;
  }
}

__global__ void sr_tail_kernel(long long ncells, long long capacity,
                               const int* __restrict__ counts,
                               const long long* __restrict__ offs,
                               long long* __restrict__ cursor_stats) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const long long total = sr_total(ncells, counts, offs);
  const long long emitted = total < capacity ? total : capacity;
  cursor_stats[CS_CURSOR] += emitted;
  cursor_stats[CS_TOTAL] = total;
  cursor_stats[CS_EMITTED] = emitted;
  cursor_stats[CS_DROPPED] = total - emitted;
  cursor_stats[CS_WINDOW] += 1;
}

using WidenIt = hipcub::TransformInputIterator<long long, SrWiden, const int*>;

size_t sr_scan_bytes(long long ncells) {
  size_t bytes = 0;
  WidenIt in(nullptr, SrWiden());
  hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in, (long long*)nullptr,
                                   (int)ncells, (hipStream_t)0);
  return bytes;
}

size_t sr_sort_bytes(long long capacity) {
  size_t bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(
      nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
      (const unsigned*)nullptr, (unsigned*)nullptr, (int)capacity, 0,
      SR_SORT_BITS, (hipStream_t)0);
  return bytes;
}

void sr_check_sizes(int64_t ncells, int64_t capacity) {
  TORCH_CHECK(ncells >= 1 && ncells <= std::numeric_limits<int>::max(),
              "sr_emit: cell count must lie in [1, 2^31)");
  TORCH_CHECK(capacity >= 1 && capacity <= SR_MAX_CAPACITY,
              "sr_emit: capacity must lie in [1, 2^30]");
}

}  // namespace

// Scratch of sr_emit_window for maps of `ncells` cells and `capacity` kept
// events, allocated once by the caller: {counts int32 [ncells], offsets
// int64 [ncells], keys int32 [2, capacity], payload int32 [2, capacity],
// hipCUB temporary storage uint8}.
std::vector<at::Tensor> sr_emit_scratch(const at::Tensor& like, int64_t ncells,
                                        int64_t capacity) {
  TORCH_CHECK(like.is_cuda(), "sr_emit_scratch: a device tensor is required");
  sr_check_sizes(ncells, capacity);
  auto opt = like.options();
  const size_t a = sr_scan_bytes(ncells), b = sr_sort_bytes(capacity);
  const long long tmp = (long long)(a > b ? a : b);
  return {at::zeros({ncells}, opt.dtype(at::kInt)),
          at::zeros({ncells}, opt.dtype(at::kLong)),
          at::zeros({2, capacity}, opt.dtype(at::kInt)),
          at::zeros({2, capacity}, opt.dtype(at::kInt)),
          at::zeros({tmp > 0 ? tmp : 1}, opt.dtype(at::kByte))};
}

// The counts stage alone (test hook): pred fp32 [...] -> int32 counts.
at::Tensor sr_emit_counts(const at::Tensor& pred, int64_t cell_cap) {
  TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == at::kFloat &&
              pred.is_contiguous(), "sr_emit_counts: contiguous fp32 required");
  TORCH_CHECK(cell_cap >= 1 && cell_cap <= SR_MAX_CELL_CAP,
              "sr_emit: cell_cap must lie in [1, 65535]");
  auto counts = at::empty(pred.sizes(), pred.options().dtype(at::kInt));
  const long long n = pred.numel();
  if (n == 0) return counts;
  hipLaunchKernelGGL(sr_counts_kernel, dim3(esr_grid(n)), dim3(ESR_BLOCK), 0,
                     at::hip::getCurrentHIPStream(), n, pred.data_ptr<float>(),
                     (int)cell_cap, counts.data_ptr<int>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return counts;
}

// pred fp32 [2, kH, kW]; win float64 [2] = (t0, t1); cols = {xs uint16,
// ys uint16, ts float64, ps int8}, each [rows]; cursor_stats int64 [5] =
// {append cursor, total, emitted, dropped, window index}: the call reads the
// cursor and the window index, appends the window's rows at the cursor, adds
// `emitted` to the cursor, writes the three counts and adds 1 to the window
// index.  mode 0 = linear, 1 = random.  scratch from sr_emit_scratch.
void sr_emit_window(const at::Tensor& pred, const at::Tensor& win,
                    const std::vector<at::Tensor>& cols,
                    at::Tensor& cursor_stats, int64_t capacity,
                    int64_t cell_cap, int64_t mode, int64_t seed,
                    const std::vector<at::Tensor>& scratch) {
  TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == at::kFloat &&
              pred.is_contiguous() && pred.dim() == 3 && pred.size(0) == 2,
              "sr_emit_window: contiguous fp32 [2,kH,kW] pred required");
  const int64_t kH = pred.size(1), kW = pred.size(2);
  TORCH_CHECK(kH >= 1 && kW >= 1 && kH <= SR_MAX_DIM && kW <= SR_MAX_DIM,
              "sr_emit_window: kH and kW must lie in [1, 32767]");
  const int64_t ncells = 2 * kH * kW;
  sr_check_sizes(ncells, capacity);
  TORCH_CHECK(cell_cap >= 1 && cell_cap <= SR_MAX_CELL_CAP,
              "sr_emit: cell_cap must lie in [1, 65535]");
  TORCH_CHECK(mode == 0 || mode == 1, "sr_emit_window: mode is 0 or 1");
  const int dev = pred.get_device();
  auto on_dev = [dev](const at::Tensor& t, at::ScalarType st) {
    return t.is_cuda() && t.get_device() == dev && t.scalar_type() == st &&
           t.is_contiguous();
  };
  TORCH_CHECK(on_dev(win, at::kDouble) && win.dim() == 1 && win.size(0) == 2,
              "sr_emit_window: win must be float64 [2] on pred's device");
  TORCH_CHECK(on_dev(cursor_stats, at::kLong) && cursor_stats.dim() == 1 &&
              cursor_stats.size(0) == CS_LEN,
              "sr_emit_window: cursor_stats must be int64 [5]");
  TORCH_CHECK(cols.size() == 4 && on_dev(cols[0], at::kUInt16) &&
              on_dev(cols[1], at::kUInt16) && on_dev(cols[2], at::kDouble) &&
              on_dev(cols[3], at::kChar),
              "sr_emit_window: cols must be xs uint16, ys uint16, ts float64, "
              "ps int8 on pred's device");
  const int64_t rows = cols[0].numel();
  for (const auto& c : cols)
    TORCH_CHECK(c.dim() == 1 && c.numel() == rows,
                "sr_emit_window: the four columns must have one length");
  TORCH_CHECK(scratch.size() == 5 && on_dev(scratch[0], at::kInt) &&
              scratch[0].numel() == ncells && on_dev(scratch[1], at::kLong) &&
              scratch[1].numel() == ncells && on_dev(scratch[2], at::kInt) &&
              scratch[2].numel() == 2 * capacity &&
              on_dev(scratch[3], at::kInt) &&
              scratch[3].numel() == 2 * capacity &&
              on_dev(scratch[4], at::kByte),
              "sr_emit_window: scratch does not fit this map and capacity "
              "(sr_emit_scratch)");
  size_t scan_bytes = sr_scan_bytes(ncells);
  size_t sort_bytes = sr_sort_bytes(capacity);
  TORCH_CHECK((size_t)scratch[4].numel() >= scan_bytes &&
              (size_t)scratch[4].numel() >= sort_bytes,
              "sr_emit_window: temporary storage too small (sr_emit_scratch)");

  auto stream = at::hip::getCurrentHIPStream();
  int* counts = scratch[0].data_ptr<int>();
  long long* offs = (long long*)scratch[1].data_ptr<int64_t>();
  unsigned* keys = (unsigned*)scratch[2].data_ptr<int>();
  unsigned* pay = (unsigned*)scratch[3].data_ptr<int>();
  unsigned* keys_out = keys + capacity;
  unsigned* pay_out = pay + capacity;
  void* tmp = scratch[4].data_ptr();
  const long long* cs = (const long long*)cursor_stats.data_ptr<int64_t>();

  hipLaunchKernelGGL(sr_counts_kernel, dim3(esr_grid(ncells)), dim3(ESR_BLOCK),
                     0, stream, (long long)ncells, pred.data_ptr<float>(),
                     (int)cell_cap, counts);
  WidenIt in(counts, SrWiden());
  C10_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, in, offs,
                                                 (int)ncells, stream));
  const long long work = ncells > capacity ? ncells : capacity;
  hipLaunchKernelGGL(sr_emit_kernel, dim3(esr_grid(work)), dim3(ESR_BLOCK), 0,
                     stream, (long long)ncells, (int)kH, (int)kW, counts, offs,
                     (long long)capacity, (int)mode, (unsigned)seed, cs, keys,
                     pay);
  C10_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
      tmp, sort_bytes, (const unsigned*)keys, keys_out, (const unsigned*)pay,
      pay_out, (int)capacity, 0, SR_SORT_BITS, stream));
  hipLaunchKernelGGL(sr_append_kernel, dim3(esr_grid(capacity)),
                     dim3(ESR_BLOCK), 0, stream, (long long)ncells,
                     (long long)capacity, (long long)rows, counts, offs,
                     keys_out, pay_out, win.data_ptr<double>(), cs,
                     (unsigned short*)cols[0].data_ptr(),
                     (unsigned short*)cols[1].data_ptr(),
                     cols[2].data_ptr<double>(),
                     (signed char*)cols[3].data_ptr<int8_t>());
  hipLaunchKernelGGL(sr_tail_kernel, dim3(1), dim3(64), 0, stream,
                     (long long)ncells, (long long)capacity, counts, offs,
                     (long long*)cursor_stats.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------
// sr_emit_lanes: S predicted windows [S, 2, kH, kW] -> rows appended to S
// independent chunks in one call (engine/superresolve.py,
// super_resolve_stores).  Per active lane the result is sr_emit_window's for
// (pred[s], win[s], capacity_s, cursor_stats[s]), bit for bit; an inactive
// lane is not read and nothing of it is written.  What is shared between the
// lanes is the launch count, not the data:
//
//   * one int64 ExclusiveSum runs over all S * ncells counts (an inactive
//     lane's counts are 0); a lane's offsets are the scan minus the scan
//     value at the lane's first cell, its total comes from its last cell;
//   * one SortPairs runs over S * capacity_max keys, key = lane << 22 | q on
//     22 + ceil(log2 S) bits.  Every lane owns exactly capacity_max slots and
//     its unused ones carry the pad key under the lane's own bits, so lane
//     s's kept events come out, in phase order, at the head of slots
//     [s * capacity_max, (s + 1) * capacity_max);
//   * capacity_s is read from lane_ctl on the device and clamped to
//     [0, capacity_max] there, so no index depends on an unchecked value.

namespace {

constexpr int LC_ACTIVE = 0, LC_CAPACITY = 1, LC_LEN = 2;
constexpr int SR_MAX_LANES = 1 << (31 - SR_SORT_BITS);      // lane bits 22..30
constexpr unsigned SR_Q_MASK = (1u << SR_SORT_BITS) - 1u;

ESR_INLINE bool sr_lane_active(const long long* lane_ctl, long long s) {
  return lane_ctl[s * LC_LEN + LC_ACTIVE] != 0;
}

ESR_INLINE long long sr_lane_capacity(const long long* lane_ctl, long long s,
                                      long long capacity_max) {
  const long long c = lane_ctl[s * LC_LEN + LC_CAPACITY];
  return c < 0 ? 0 : (c < capacity_max ? c : capacity_max);
}

ESR_INLINE long long sr_lane_total(long long ncells, long long s,
                                   const int* counts, const long long* offs) {
  const long long last = (s + 1) * ncells - 1;
  return offs[last] + counts[last] - offs[s * ncells];
}

ESR_INLINE long long sr_lane_emitted(long long ncells, long long s,
                                     const int* counts, const long long* offs,
                                     const long long* lane_ctl,
                                     long long capacity_max) {
  const long long total = sr_lane_total(ncells, s, counts, offs);
  const long long cap = sr_lane_capacity(lane_ctl, s, capacity_max);
  return total < cap ? total : cap;
}

__global__ void sr_lanes_counts_kernel(long long n, long long ncells,
                                       const float* __restrict__ pred,
                                       int cell_cap,
                                       const long long* __restrict__ lane_ctl,
                                       int* __restrict__ counts) {
  ESR_KERNEL_LOOP(i, n) {
    counts[i] = sr_lane_active(lane_ctl, i / ncells)
                    ? sr_cell_count(pred[i], cell_cap) : 0;
  }
}

// sr_emit_kernel per lane: cell i of the [S, 2, kH, kW] stack belongs to lane
// i / ncells, hashes as the lane's own cell and window index, and writes into
// the lane's capacity_max slots.
__global__ void sr_lanes_emit_kernel(long long S, long long ncells, int kH,
                                     int kW, const int* __restrict__ counts,
                                     const long long* __restrict__ offs,
                                     const long long* __restrict__ lane_ctl,
                                     long long capacity_max, int mode,
                                     unsigned seed,
                                     const long long* __restrict__ cursor_stats,
                                     unsigned* __restrict__ keys,
                                     unsigned* __restrict__ payload) {
  const long long plane = (long long)kH * kW;
  ESR_KERNEL_LOOP(i, S * ncells) {
    const int n = counts[i];
    if (!n) continue;
    const long long s = i / ncells, c = i - s * ncells;
    const long long capacity = sr_lane_capacity(lane_ctl, s, capacity_max);
    const long long base = offs[i] - offs[s * ncells];
    if (base >= capacity) continue;
    const unsigned widx = (unsigned)cursor_stats[s * CS_LEN + CS_WINDOW];
    const unsigned lane = (unsigned)s << SR_SORT_BITS;
    const long long r = c % plane;
    const unsigned x = (unsigned)(r % kW), y = (unsigned)(r / kW);
    const unsigned pay = x | (y << 15) | (c >= plane ? 0x80000000u : 0u);
    const long long keep = capacity - base < n ? capacity - base : n;
    const long long slot = s * capacity_max + base;
    for (long long j = 0; j < keep; ++j) {
      unsigned q;
      if (mode == 0) {
        q = n == 1 ? 0u : (unsigned)((j * SR_Q) / (n - 1));
      } else {
        q = sr_hash_phase(seed, widx, (unsigned)c, (unsigned)j);
      }
      keys[slot + j] = lane | q;
      payload[slot + j] = pay;
    }
  }
  ESR_KERNEL_LOOP(t, S * capacity_max) {
    const long long s = t / capacity_max, k = t - s * capacity_max;
    if (k >= sr_lane_emitted(ncells, s, counts, offs, lane_ctl,
                             capacity_max)) {
      keys[t] = ((unsigned)s << SR_SORT_BITS) | SR_PAD_KEY;
      payload[t] = 0u;
    }
  }
}

__global__ void sr_lanes_append_kernel(long long S, long long ncells,
                                       long long capacity_max, long long rows,
                                       const int* __restrict__ counts,
                                       const long long* __restrict__ offs,
                                       const long long* __restrict__ lane_ctl,
                                       const unsigned* __restrict__ keys,
                                       const unsigned* __restrict__ payload,
                                       const double* __restrict__ win,
                                       const long long* __restrict__ cursor_stats,
                                       unsigned short* __restrict__ xs,
                                       unsigned short* __restrict__ ys,
                                       double* __restrict__ ts,
                                       signed char* __restrict__ ps) {
  ESR_KERNEL_LOOP(t, S * capacity_max) {
    const long long s = t / capacity_max, k = t - s * capacity_max;
    if (k >= sr_lane_emitted(ncells, s, counts, offs, lane_ctl, capacity_max))
      continue;                               // an inactive lane emits 0
    const long long row = cursor_stats[s * CS_LEN + CS_CURSOR] + k;
    if (row < 0 || row >= rows) continue;     // the chunk is never overrun
    const long long at = s * rows + row;
    const unsigned p = payload[t];
    xs[at] = (unsigned short)(p & 0x7fffu);
    ys[at] = (unsigned short)((p >> 15) & 0x7fffu);
    ts[at] = sr_timestamp(win[2 * s], win[2 * s + 1], keys[t] & SR_Q_MASK);
    ps[at] = (p >> 31) ? (signed char)-1 : (signed char)1;
  }
}

__global__ void sr_lanes_tail_kernel(long long S, long long ncells,
                                     long long capacity_max,
                                     const int* __restrict__ counts,
                                     const long long* __restrict__ offs,
                                     const long long* __restrict__ lane_ctl,
                                     long long* __restrict__ cursor_stats) {
  ESR_KERNEL_LOOP(s, S) {
    if (!sr_lane_active(lane_ctl, s)) continue;
    const long long total = sr_lane_total(ncells, s, counts, offs);
    const long long emitted = sr_lane_emitted(ncells, s, counts, offs,
                                              lane_ctl, capacity_max);
    long long* cs = cursor_stats + s * CS_LEN;
    cs[CS_CURSOR] += emitted;
    cs[CS_TOTAL] = total;
    cs[CS_EMITTED] = emitted;
    cs[CS_DROPPED] = total - emitted;
    cs[CS_WINDOW] += 1;
  }
}

int sr_lanes_sort_bits(int64_t S) {
  int bits = SR_SORT_BITS;
  while ((1ll << (bits - SR_SORT_BITS)) < S) ++bits;
  return bits;
}

size_t sr_lanes_sort_bytes(int64_t S, long long slots) {
  size_t bytes = 0;
  hipcub::DeviceRadixSort::SortPairs(
      nullptr, bytes, (const unsigned*)nullptr, (unsigned*)nullptr,
      (const unsigned*)nullptr, (unsigned*)nullptr, (int)slots, 0,
      sr_lanes_sort_bits(S), (hipStream_t)0);
  return bytes;
}

void sr_lanes_check_sizes(int64_t S, int64_t ncells, int64_t capacity_max) {
  TORCH_CHECK(S >= 1 && S <= SR_MAX_LANES,
              "sr_emit_lanes: the lane count must lie in [1, ", SR_MAX_LANES,
              "]");
  TORCH_CHECK(ncells >= 1 &&
              ncells <= std::numeric_limits<int>::max() / S,
              "sr_emit_lanes: lanes * cells must lie in [1, 2^31)");
  TORCH_CHECK(capacity_max >= 1 && capacity_max <= SR_MAX_CAPACITY / S,
              "sr_emit_lanes: lanes * capacity_max must lie in [1, 2^30]");
}

}  // namespace

// Scratch of sr_emit_lanes for S maps of `ncells` cells and at most
// `capacity_max` kept events per lane: sr_emit_scratch's layout with S times
// the cells and slots.
std::vector<at::Tensor> sr_emit_lanes_scratch(const at::Tensor& like,
                                              int64_t S, int64_t ncells,
                                              int64_t capacity_max) {
  TORCH_CHECK(like.is_cuda(),
              "sr_emit_lanes_scratch: a device tensor is required");
  sr_lanes_check_sizes(S, ncells, capacity_max);
  auto opt = like.options();
  const long long cells = S * ncells, slots = S * capacity_max;
  const size_t a = sr_scan_bytes(cells), b = sr_lanes_sort_bytes(S, slots);
  const long long tmp = (long long)(a > b ? a : b);
  return {at::zeros({cells}, opt.dtype(at::kInt)),
          at::zeros({cells}, opt.dtype(at::kLong)),
          at::zeros({2, slots}, opt.dtype(at::kInt)),
          at::zeros({2, slots}, opt.dtype(at::kInt)),
          at::zeros({tmp > 0 ? tmp : 1}, opt.dtype(at::kByte))};
}

// pred fp32 [S, 2, kH, kW]; win float64 [S, 2] = (t0, t1) per lane; cols =
// {xs uint16, ys uint16, ts float64, ps int8}, each [S, rows]; cursor_stats
// int64 [S, 5], sr_emit_window's layout per lane; lane_ctl int64 [S, 2] =
// {active, capacity_s}, 1 <= capacity_s <= capacity_max.  An active lane gets
// what sr_emit_window does for it alone; of an inactive lane (active == 0)
// nothing is read but lane_ctl and nothing is written.  scratch from
// sr_emit_lanes_scratch.
void sr_emit_lanes(const at::Tensor& pred, const at::Tensor& win,
                   const std::vector<at::Tensor>& cols,
                   at::Tensor& cursor_stats, const at::Tensor& lane_ctl,
                   int64_t capacity_max, int64_t cell_cap, int64_t mode,
                   int64_t seed, const std::vector<at::Tensor>& scratch) {
  TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == at::kFloat &&
              pred.is_contiguous() && pred.dim() == 4 && pred.size(0) >= 1 &&
              pred.size(1) == 2,
              "sr_emit_lanes: contiguous fp32 [S,2,kH,kW] pred required");
  const int64_t S = pred.size(0), kH = pred.size(2), kW = pred.size(3);
  TORCH_CHECK(kH >= 1 && kW >= 1 && kH <= SR_MAX_DIM && kW <= SR_MAX_DIM,
              "sr_emit_lanes: kH and kW must lie in [1, 32767]");
  const int64_t ncells = 2 * kH * kW;
  sr_lanes_check_sizes(S, ncells, capacity_max);
  TORCH_CHECK(cell_cap >= 1 && cell_cap <= SR_MAX_CELL_CAP,
              "sr_emit: cell_cap must lie in [1, 65535]");
  TORCH_CHECK(mode == 0 || mode == 1, "sr_emit_lanes: mode is 0 or 1");
  const int dev = pred.get_device();
  auto on_dev = [dev](const at::Tensor& t, at::ScalarType st) {
    return t.is_cuda() && t.get_device() == dev && t.scalar_type() == st &&
           t.is_contiguous();
  };
  TORCH_CHECK(on_dev(win, at::kDouble) && win.dim() == 2 &&
              win.size(0) == S && win.size(1) == 2,
              "sr_emit_lanes: win must be float64 [S,2] on pred's device");
  TORCH_CHECK(on_dev(cursor_stats, at::kLong) && cursor_stats.dim() == 2 &&
              cursor_stats.size(0) == S && cursor_stats.size(1) == CS_LEN,
              "sr_emit_lanes: cursor_stats must be int64 [S,5]");
  TORCH_CHECK(on_dev(lane_ctl, at::kLong) && lane_ctl.dim() == 2 &&
              lane_ctl.size(0) == S && lane_ctl.size(1) == LC_LEN,
              "sr_emit_lanes: lane_ctl must be int64 [S,2]");
  TORCH_CHECK(cols.size() == 4 && on_dev(cols[0], at::kUInt16) &&
              on_dev(cols[1], at::kUInt16) && on_dev(cols[2], at::kDouble) &&
              on_dev(cols[3], at::kChar),
              "sr_emit_lanes: cols must be xs uint16, ys uint16, ts float64, "
              "ps int8 on pred's device");
  TORCH_CHECK(cols[0].dim() == 2, "sr_emit_lanes: the columns must be "
              "[S, rows]");
  const int64_t rows = cols[0].size(1);
  for (const auto& c : cols)
    TORCH_CHECK(c.dim() == 2 && c.size(0) == S && c.size(1) == rows,
                "sr_emit_lanes: the four columns must all be [S, rows]");
  const long long cells = S * ncells, slots = S * capacity_max;
  TORCH_CHECK(scratch.size() == 5 && on_dev(scratch[0], at::kInt) &&
              scratch[0].numel() == cells && on_dev(scratch[1], at::kLong) &&
              scratch[1].numel() == cells && on_dev(scratch[2], at::kInt) &&
              scratch[2].numel() == 2 * slots &&
              on_dev(scratch[3], at::kInt) &&
              scratch[3].numel() == 2 * slots &&
              on_dev(scratch[4], at::kByte),
              "sr_emit_lanes: scratch does not fit these lanes, map and "
              "capacity (sr_emit_lanes_scratch)");
  size_t scan_bytes = sr_scan_bytes(cells);
  size_t sort_bytes = sr_lanes_sort_bytes(S, slots);
  TORCH_CHECK((size_t)scratch[4].numel() >= scan_bytes &&
              (size_t)scratch[4].numel() >= sort_bytes,
              "sr_emit_lanes: temporary storage too small "
              "(sr_emit_lanes_scratch)");

  auto stream = at::hip::getCurrentHIPStream();
  int* counts = scratch[0].data_ptr<int>();
  long long* offs = (long long*)scratch[1].data_ptr<int64_t>();
  unsigned* keys = (unsigned*)scratch[2].data_ptr<int>();
  unsigned* pay = (unsigned*)scratch[3].data_ptr<int>();
  unsigned* keys_out = keys + slots;
  unsigned* pay_out = pay + slots;
  void* tmp = scratch[4].data_ptr();
  const long long* cs = (const long long*)cursor_stats.data_ptr<int64_t>();
  const long long* lc = (const long long*)lane_ctl.data_ptr<int64_t>();

  hipLaunchKernelGGL(sr_lanes_counts_kernel, dim3(esr_grid(cells)),
                     dim3(ESR_BLOCK), 0, stream, cells, (long long)ncells,
                     pred.data_ptr<float>(), (int)cell_cap, lc, counts);
  WidenIt in(counts, SrWiden());
  C10_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp, scan_bytes, in, offs,
                                                 (int)cells, stream));
  const long long work = cells > slots ? cells : slots;
  hipLaunchKernelGGL(sr_lanes_emit_kernel, dim3(esr_grid(work)),
                     dim3(ESR_BLOCK), 0, stream, (long long)S,
                     (long long)ncells, (int)kH, (int)kW, counts, offs, lc,
                     (long long)capacity_max, (int)mode, (unsigned)seed, cs,
                     keys, pay);
  C10_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(
      tmp, sort_bytes, (const unsigned*)keys, keys_out, (const unsigned*)pay,
      pay_out, (int)slots, 0, sr_lanes_sort_bits(S), stream));
  hipLaunchKernelGGL(sr_lanes_append_kernel, dim3(esr_grid(slots)),
                     dim3(ESR_BLOCK), 0, stream, (long long)S,
                     (long long)ncells, (long long)capacity_max,
                     (long long)rows, counts, offs, lc, keys_out, pay_out,
                     win.data_ptr<double>(), cs,
                     (unsigned short*)cols[0].data_ptr(),
                     (unsigned short*)cols[1].data_ptr(),
                     cols[2].data_ptr<double>(),
                     (signed char*)cols[3].data_ptr<int8_t>());
  hipLaunchKernelGGL(sr_lanes_tail_kernel, dim3(esr_grid(S)), dim3(ESR_BLOCK),
                     0, stream, (long long)S, (long long)ncells,
                     (long long)capacity_max, counts, offs, lc,
                     (long long*)cursor_stats.data_ptr<int64_t>());
  C10_HIP_KERNEL_LAUNCH_CHECK();
}
