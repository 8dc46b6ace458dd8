// tm_declick.hip — the de-click stage on the device.
//
// The reference's step 2.2, src/declick_inpaint.py, restated as streaming kernels:
//   dmax[i] = max_c |x[i+1,c] - x[i,c]|            :64-66   -> k_dc_dmax_*
//   sigma   = (median(|dmax - median(dmax)|) + 1e-12) / 0.6745   (mad_sigma :7-11)
//                                                           -> k_dc_sel_* (exact radix
//                                                              select), scalars on the host
//   hit     = dmax > k * sigma                     :68-69   -> k_dc_tile_hits
//   mask / merge_runs / length filter              :78-94   -> k_dc_link, k_dc_tile_heads,
//                                                              k_dc_offsets, k_dc_filter
//   inpaint_linear                                 :26-46   -> k_dc_inpaint
//
// Everything is decided on bit patterns, so the stage is bit-exact: no FFT, no
// transcendental, float32 arithmetic with -ffp-contract=off (the unit's build),
// exact order statistics.  The host forms only the file's scalars (even-count
// mean, + 1e-12, / 0.6745, k * sigma) from the selected bit patterns.
//
// Layout (HBM-bound streaming work; wave64, 256-thread workgroups):
//  * dmax stays resident (4 B per frame): it is read by six select passes and
//    three segment passes, each of which would otherwise re-read 4*C B per frame.
//  * select: the values are >= +0 and not NaN, so their float32 bit patterns
//    order as unsigned integers.  Three digit passes (11 + 11 + 10 bits), each a
//    grid-stride sweep with 16-byte lane-contiguous loads into per-workgroup LDS
//    histograms (integer LDS atomics), merged into a global u32 histogram with
//    integer atomics; one small workgroup walks the digit and re-zeroes the
//    histogram.  Two ranks are carried at once (the two middle order statistics
//    of an even count); a second histogram is used only once their prefixes
//    differ.  The MAD pass forms its keys on the fly as |d - med|.
//  * segments: with D = 2*pad + 1 + gap, consecutive hits i < j lie in one
//    segment iff j - i <= D.  A hit is a cluster HEAD when its previous hit is
//    more than D away (or absent) and a TAIL when its next hit is; the k-th head
//    and the k-th tail bound the k-th raw segment [max(0, a-pad), min(N, b+1+pad)).
//    Tiles of 4096 differences: per-tile first / last hit, one workgroup links
//    the tiles (running max / min over tiles), the tiles count their heads and
//    tails, one workgroup scans the counts, the tiles write the bounds in order,
//    one workgroup filters by length in order.  Nothing sized by the hit count
//    exists: dense hits (a square wave) are one cluster and cost nothing extra.
//  * inpaint: one wave per kept segment, lanes over (frame, channel).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"

namespace {

typedef long long i64;

constexpr int kT = 256;               // threads per streaming workgroup
constexpr int kPer = 16;              // differences per thread of a tile
constexpr int kTile = kT * kPer;      // differences per tile
constexpr int kBins = 2048;           // widest digit (11 bits)
constexpr int kScanT = 1024;          // threads of the single-workgroup scans
constexpr int kStateWords = 16;       // SelState, padded
constexpr int kTileArrays = 9;        // int64 arrays of one entry per tile
constexpr i64 kNone = LLONG_MAX;      // "no hit after"

int dc_fail(hipError_t e) { return e == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP; }
int dc_launch() { return dc_fail(hipGetLastError()); }

// workgroups of a grid-stride sweep over `groups` 256-thread groups of work:
// eight per CU at the most
int dc_grid(i64 groups) {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  const i64 cap = (i64)cus * 8;
  return (int)(groups < 1 ? 1 : (groups < cap ? groups : cap));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

i64 n_tiles(i64 n) { return n < 1 ? 1 : (n + kTile - 1) / kTile; }

struct OpAdd {
  template <typename T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <typename T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct OpMin {
  template <typename T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};

// Scan over the NT threads of the workgroup in thread order: *excl = op over
// the threads before this one (ident for thread 0), *total = op over all.
// sm: NT / 64 slots, free again on return.
template <typename T, typename Op, int NT>
__device__ __forceinline__ void block_scan(T v, T ident, Op op, T* sm, T* excl, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, t);
  }
  T e = __shfl_up(v, 1, 64);
  if (lane == 0) e = ident;
  if (lane == 63) sm[w] = v;
  __syncthreads();
  T pre = ident, tot = ident;
  for (int i = 0; i < NT / 64; ++i) {
    const T s = sm[i];
    if (i < w) pre = op(pre, s);
    tot = op(tot, s);
  }
  __syncthreads();
  *excl = op(pre, e);
  *total = tot;
}

// The same from the last thread down: *excl = op over the threads after this one.
template <typename T, typename Op, int NT>
__device__ __forceinline__ void block_scan_rev(T v, T ident, Op op, T* sm, T* excl, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_down(v, o, 64);
    if (lane + o < 64) v = op(v, t);
  }
  T e = __shfl_down(v, 1, 64);
  if (lane == 63) e = ident;
  if (lane == 0) sm[w] = v;
  __syncthreads();
  T post = ident, tot = ident;
  for (int i = 0; i < NT / 64; ++i) {
    const T s = sm[i];
    if (i > w) post = op(post, s);
    tot = op(tot, s);
  }
  __syncthreads();
  *excl = op(post, e);
  *total = tot;
}

__device__ __forceinline__ float4 ld4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}

// ---------------------------------------------------------------------------
// dmax[i] = max_c |x[i+1][c] - x[i][c]|, i < n - 1
// ---------------------------------------------------------------------------
__device__ __forceinline__ float adiff(float b, float a) { return fabsf(__fsub_rn(b, a)); }

// C = 1 / 2, x and d 16-byte aligned: four differences per thread from 16-byte loads
template <int C>
__global__ __launch_bounds__(kT) void k_dc_dmax_vec(const float* __restrict__ x, i64 n,
                                                     float* __restrict__ d) {
  const i64 nd = n - 1, G = nd >> 2;
  for (i64 q = (i64)blockIdx.x * kT + threadIdx.x; q < G; q += (i64)gridDim.x * kT) {
    float4 o;
    if constexpr (C == 1) {
      const float4 a = ld4(x + 4 * q);
      const float b = x[4 * q + 4];  // frame 4q+4 <= n-1
      o = make_float4(adiff(a.y, a.x), adiff(a.z, a.y), adiff(a.w, a.z), adiff(b, a.w));
    } else {
      const float4 a = ld4(x + 8 * q), b = ld4(x + 8 * q + 4);
      const float2 c = *reinterpret_cast<const float2*>(x + 8 * q + 8);
      o = make_float4(fmaxf(adiff(a.z, a.x), adiff(a.w, a.y)),
                      fmaxf(adiff(b.x, a.z), adiff(b.y, a.w)),
                      fmaxf(adiff(b.z, b.x), adiff(b.w, b.y)),
                      fmaxf(adiff(c.x, b.z), adiff(c.y, b.w)));
    }
    *reinterpret_cast<float4*>(d + 4 * q) = o;
  }
  const i64 i = 4 * G + threadIdx.x;  // ragged tail: fewer than four differences
  if (blockIdx.x == 0 && i < nd) {
    float m = 0.0f;
    for (int c = 0; c < C; ++c) m = fmaxf(m, adiff(x[(i + 1) * C + c], x[i * C + c]));
    d[i] = m;
  }
}

// any channel count: a plain loop over the channels
__global__ __launch_bounds__(kT) void k_dc_dmax_any(const float* __restrict__ x, i64 n, int ch,
                                                     float* __restrict__ d) {
  const i64 nd = n - 1;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < nd; i += (i64)gridDim.x * kT) {
    float m = 0.0f;
    for (int c = 0; c < ch; ++c) m = fmaxf(m, adiff(x[(i + 1) * ch + c], x[i * ch + c]));
    d[i] = m;
  }
}

// ---------------------------------------------------------------------------
// exact selection of two ranks over many workgroups
// ---------------------------------------------------------------------------
struct SelState {
  uint32_t prefix[2];  // key bits decided so far (lower bits zero)
  uint32_t rank[2];    // rank among the keys that share the prefix
};

__host__ __device__ inline int sel_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ inline uint32_t sel_himask(int pass) {
  return pass == 0 ? 0u : (pass == 1 ? 0xFFE00000u : 0xFFFFFC00u);
}
__host__ __device__ inline int sel_bins(int pass) { return pass == 2 ? 1024 : 2048; }

__global__ __launch_bounds__(kT) void k_dc_sel_init(SelState* st, uint32_t* gh, uint32_t r0,
                                                     uint32_t r1) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i < 2 * kBins) gh[i] = 0u;
  if (i == 0) {
    st->prefix[0] = st->prefix[1] = 0u;
    st->rank[0] = r0;
    st->rank[1] = r1;
  }
}

template <bool CENTER>
__global__ __launch_bounds__(kT) void k_dc_sel_hist(const float* __restrict__ v, i64 n, int vec,
                                                     float center, const SelState* st,
                                                     uint32_t* gh, int pass) {
  __shared__ uint32_t h[2 * kBins];
  for (int i = threadIdx.x; i < 2 * kBins; i += kT) h[i] = 0u;
  __syncthreads();
  const uint32_t p0 = st->prefix[0], p1 = st->prefix[1];
  const bool same = p0 == p1;
  const uint32_t mh = sel_himask(pass), bm = (uint32_t)sel_bins(pass) - 1u;
  const int sh = sel_shift(pass);
  auto add = [&](float f) {
    if constexpr (CENTER) f = fabsf(__fsub_rn(f, center));
    const uint32_t k = __float_as_uint(f), hi = k & mh, b = (k >> sh) & bm;
    if (hi == p0) atomicAdd(&h[b], 1u);
    if (!same && hi == p1) atomicAdd(&h[kBins + b], 1u);
  };
  const i64 G = vec ? (n >> 2) : 0;
  for (i64 q = (i64)blockIdx.x * kT + threadIdx.x; q < G; q += (i64)gridDim.x * kT) {
    const float4 a = ld4(v + 4 * q);
    add(a.x);
    add(a.y);
    add(a.z);
    add(a.w);
  }
  for (i64 i = 4 * G + (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT)
    add(v[i]);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kBins; i += kT) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&gh[i], c);
  }
}

// one workgroup: walk the digit for both ranks, re-zero the histograms
__global__ __launch_bounds__(kT) void k_dc_sel_pick(SelState* st, uint32_t* gh, int pass,
                                                     uint32_t* out) {
  __shared__ uint32_t sm[kT / 64];
  __shared__ uint32_t np[2], nr[2];
  const uint32_t p[2] = {st->prefix[0], st->prefix[1]};
  const uint32_t r[2] = {st->rank[0], st->rank[1]};
  const bool same = p[0] == p[1];
  const int per = sel_bins(pass) / kT, sh = sel_shift(pass);
  if (threadIdx.x < 2) {
    np[threadIdx.x] = p[threadIdx.x];
    nr[threadIdx.x] = 0u;
  }
  __syncthreads();
  for (int j = 0; j < 2; ++j) {
    const uint32_t* h = gh + ((j == 1 && !same) ? kBins : 0);
    const int b0 = threadIdx.x * per;
    uint32_t s = 0u;
    for (int k = 0; k < per; ++k) s += h[b0 + k];
    uint32_t ex, tot;
    block_scan<uint32_t, OpAdd, kT>(s, 0u, OpAdd{}, sm, &ex, &tot);
    if (r[j] >= ex && r[j] - ex < s) {
      uint32_t c = ex;
      for (int k = 0; k < per; ++k) {
        const uint32_t w = h[b0 + k];
        if (r[j] - c < w) {
          np[j] = p[j] | ((uint32_t)(b0 + k) << sh);
          nr[j] = r[j] - c;
          break;
        }
        c += w;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * kBins; i += kT) gh[i] = 0u;
  if (threadIdx.x < 2) {
    st->prefix[threadIdx.x] = np[threadIdx.x];
    st->rank[threadIdx.x] = nr[threadIdx.x];
    if (pass == 2) out[threadIdx.x] = np[threadIdx.x];
  }
}

// ---------------------------------------------------------------------------
// hits -> clusters -> segments
// ---------------------------------------------------------------------------
// Hit bits of this thread's 16 consecutive differences [tb + 16 t, +16) of the
// tile at tb: 16-byte lane-contiguous loads, nibbles regrouped through LDS.
__device__ __forceinline__ uint32_t tile_mask(const float* __restrict__ d, i64 n, i64 tb, float thr,
                                              int vec, uint8_t* nib) {
  for (int j = 0; j < kPer / 4; ++j) {
    const int g = j * kT + threadIdx.x;
    const i64 e = tb + 4 * (i64)g;
    uint32_t b = 0u;
    if (vec && e + 4 <= n) {
      const float4 a = ld4(d + e);
      b = (a.x > thr ? 1u : 0u) | (a.y > thr ? 2u : 0u) | (a.z > thr ? 4u : 0u) |
          (a.w > thr ? 8u : 0u);
    } else {
      for (int k = 0; k < 4; ++k)
        if (e + k < n && d[e + k] > thr) b |= 1u << k;
    }
    nib[g] = (uint8_t)b;
  }
  __syncthreads();
  const uint32_t w = reinterpret_cast<const uint32_t*>(nib)[threadIdx.x];
  __syncthreads();
  return (w & 0xFu) | ((w >> 4) & 0xF0u) | ((w >> 8) & 0xF00u) | ((w >> 12) & 0xF000u);
}

// per tile: first hit, last hit (global indices; kNone / -1 when none), hit count
__global__ __launch_bounds__(kT) void k_dc_tile_hits(const float* __restrict__ d, i64 n, float thr,
                                                      int vec, i64* first, i64* last, i64* cnt) {
  __shared__ __attribute__((aligned(16))) uint8_t nib[kTile / 4];
  __shared__ int sm[kT / 64];
  const i64 tb = (i64)blockIdx.x * kTile;
  const uint32_t m = tile_mask(d, n, tb, thr, vec, nib);
  const int r0 = threadIdx.x * kPer;
  const int lf = m ? r0 + __builtin_ctz(m) : INT_MAX;
  const int ll = m ? r0 + 31 - __builtin_clz(m) : -1;
  int ex, f, l, c;
  block_scan<int, OpMin, kT>(lf, INT_MAX, OpMin{}, sm, &ex, &f);
  block_scan<int, OpMax, kT>(ll, -1, OpMax{}, sm, &ex, &l);
  block_scan<int, OpAdd, kT>(__builtin_popcount(m), 0, OpAdd{}, sm, &ex, &c);
  if (threadIdx.x == 0) {
    first[blockIdx.x] = c ? tb + f : kNone;
    last[blockIdx.x] = c ? tb + l : -1;
    cnt[blockIdx.x] = c;
  }
}

// one workgroup: for every tile the last hit before it and the first hit after
// it; counts[0] = hits
__global__ __launch_bounds__(kScanT) void k_dc_link(i64 nb, const i64* first, const i64* last,
                                                     const i64* cnt, i64* prev_last,
                                                     i64* next_first, i64* counts) {
  __shared__ i64 sm[kScanT / 64];
  i64 carry = -1, mine = 0, ex, tot;
  for (i64 base = 0; base < nb; base += kScanT) {
    const i64 i = base + threadIdx.x;
    const i64 v = i < nb ? last[i] : -1;
    if (i < nb) mine += cnt[i];
    block_scan<i64, OpMax, kScanT>(v, (i64)-1, OpMax{}, sm, &ex, &tot);
    if (i < nb) prev_last[i] = carry > ex ? carry : ex;
    carry = carry > tot ? carry : tot;
  }
  carry = kNone;
  for (i64 base = ((nb - 1) / kScanT) * kScanT; base >= 0; base -= kScanT) {
    const i64 i = base + threadIdx.x;
    const i64 v = i < nb ? first[i] : kNone;
    block_scan_rev<i64, OpMin, kScanT>(v, kNone, OpMin{}, sm, &ex, &tot);
    if (i < nb) next_first[i] = carry < ex ? carry : ex;
    carry = carry < tot ? carry : tot;
  }
  block_scan<i64, OpAdd, kScanT>(mine, (i64)0, OpAdd{}, sm, &ex, &tot);
  if (threadIdx.x == 0) counts[0] = tot;
}

// per tile: WRITE = false counts the cluster heads and tails; WRITE = true
// writes starts (bounds[0, cap)) and ends (bounds[cap, 2 cap)) at their ordinals
template <bool WRITE>
__global__ __launch_bounds__(kT) void k_dc_tile_heads(
    const float* __restrict__ d, i64 n, float thr, int vec, i64 D, const i64* prev_last,
    const i64* next_first, i64* hcnt, i64* tcnt, const i64* hoff, const i64* toff, i64* bounds,
    i64 cap, i64 pad, i64* counts) {
  __shared__ __attribute__((aligned(16))) uint8_t nib[kTile / 4];
  __shared__ int sm[kT / 64];
  const i64 tb = (i64)blockIdx.x * kTile;
  const uint32_t m = tile_mask(d, n, tb, thr, vec, nib);
  const int r0 = threadIdx.x * kPer;
  const int lf = m ? r0 + __builtin_ctz(m) : INT_MAX;
  const int ll = m ? r0 + 31 - __builtin_clz(m) : -1;
  int pl, nf, tot;
  block_scan<int, OpMax, kT>(ll, -1, OpMax{}, sm, &pl, &tot);
  block_scan_rev<int, OpMin, kT>(lf, INT_MAX, OpMin{}, sm, &nf, &tot);
  i64 p = pl >= 0 ? tb + pl : prev_last[blockIdx.x];
  const i64 after = nf != INT_MAX ? tb + nf : next_first[blockIdx.x];
  uint32_t hm = 0u, tm = 0u;
  for (uint32_t mm = m; mm; mm &= mm - 1) {
    const int k = __builtin_ctz(mm);
    const i64 i = tb + r0 + k;
    const uint32_t up = mm & (mm - 1);
    const i64 nx = up ? tb + r0 + __builtin_ctz(up) : after;
    if (p < 0 || i - p > D) hm |= 1u << k;
    if (nx == kNone || nx - i > D) tm |= 1u << k;
    p = i;
  }
  int ex;
  block_scan<int, OpAdd, kT>(__builtin_popcount(hm) | (__builtin_popcount(tm) << 16), 0, OpAdd{},
                             sm, &ex, &tot);
  if constexpr (!WRITE) {
    if (threadIdx.x == 0) {
      hcnt[blockIdx.x] = tot & 0xFFFF;
      tcnt[blockIdx.x] = tot >> 16;
    }
  } else {
    const i64 N = n + 1;
    i64 hp = hoff[blockIdx.x] + (ex & 0xFFFF), tp = toff[blockIdx.x] + (ex >> 16);
    bool over = false;
    for (uint32_t mm = hm; mm; mm &= mm - 1, ++hp) {
      const i64 s = tb + r0 + __builtin_ctz(mm) - pad;
      if (hp < cap) bounds[hp] = s < 0 ? 0 : s;
      else over = true;
    }
    for (uint32_t mm = tm; mm; mm &= mm - 1, ++tp) {
      const i64 e = tb + r0 + __builtin_ctz(mm) + 1 + pad;
      if (tp < cap) bounds[cap + tp] = e > N ? N : e;
      else over = true;
    }
    if (over) counts[3] = 1;  // more clusters than the caller's raw count
  }
}

// one workgroup: exclusive sums of the per-tile head / tail counts;
// counts[1] = raw segments
__global__ __launch_bounds__(kScanT) void k_dc_offsets(i64 nb, const i64* hcnt, const i64* tcnt,
                                                        i64* hoff, i64* toff, i64* counts) {
  __shared__ i64 sm[kScanT / 64];
  i64 hc = 0, tc = 0, ex, tot;
  for (i64 base = 0; base < nb; base += kScanT) {
    const i64 i = base + threadIdx.x;
    block_scan<i64, OpAdd, kScanT>(i < nb ? hcnt[i] : 0, (i64)0, OpAdd{}, sm, &ex, &tot);
    if (i < nb) hoff[i] = hc + ex;
    hc += tot;
    block_scan<i64, OpAdd, kScanT>(i < nb ? tcnt[i] : 0, (i64)0, OpAdd{}, sm, &ex, &tot);
    if (i < nb) toff[i] = tc + ex;
    tc += tot;
  }
  if (threadIdx.x == 0) {
    counts[1] = hc;
    if (hc != tc) counts[3] = 2;  // cannot happen: every cluster has one head and one tail
  }
}

// one workgroup: the raw segments no longer than max_fix, in order;
// counts[2] = kept
__global__ __launch_bounds__(kScanT) void k_dc_filter(const i64* bounds, i64 raw, i64 max_fix,
                                                       i64* segs, i64* counts) {
  __shared__ i64 sm[kScanT / 64];
  i64 kept = 0, ex, tot;
  for (i64 base = 0; base < raw; base += kScanT) {
    const i64 i = base + threadIdx.x;
    i64 s = 0, e = 0;
    bool keep = false;
    if (i < raw) {
      s = bounds[i];
      e = bounds[raw + i];
      keep = e - s <= max_fix;
    }
    block_scan<i64, OpAdd, kScanT>(keep ? 1 : 0, (i64)0, OpAdd{}, sm, &ex, &tot);
    if (keep) {  // kept + ex < raw: segs holds raw pairs
      segs[2 * (kept + ex)] = s;
      segs[2 * (kept + ex) + 1] = e;
    }
    kept += tot;
  }
  if (threadIdx.x == 0) counts[2] = kept;
}

// ---------------------------------------------------------------------------
// linear inpainting: one wave per kept segment
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kT) void k_dc_inpaint(const float* __restrict__ x,
                                                    float* __restrict__ y, i64 N, int ch,
                                                    const i64* __restrict__ segs, i64 nseg) {
  const i64 w = (i64)blockIdx.x * (kT / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nseg) return;
  const i64 s = segs[2 * w], e = segs[2 * w + 1];
  if (s < 0 || e > N || s >= e) return;
  const i64 s0 = s > 0 ? s - 1 : 0, e0 = e < N - 1 ? e : N - 1;
  if (s0 >= e0) return;
  const i64 L = e0 - s0;
  const double step = 1.0 / (double)L;  // np.linspace(0, 1, L + 1): i * step in double
  const i64 cnt = (e - s) * ch;
  for (i64 q = lane; q < cnt; q += 64) {
    const i64 fr = s + q / ch;
    const int c = (int)(q % ch);
    const i64 i = fr - s0;
    const float t = i == L ? 1.0f : (float)((double)i * step);
    const float left = x[s0 * ch + c], right = x[e0 * ch + c];
    y[fr * ch + c] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, t), left), __fmul_rn(t, right));
  }
}

// workspace carve: two histograms, the select state, the per-tile arrays
struct Work {
  uint32_t* gh;
  SelState* st;
  i64* tile[kTileArrays];
};

Work carve(uint32_t* work, i64 nb) {
  Work w;
  w.gh = work;
  w.st = reinterpret_cast<SelState*>(work + 2 * kBins);
  i64* t = reinterpret_cast<i64*>(work + 2 * kBins + kStateWords);
  for (int a = 0; a < kTileArrays; ++a) w.tile[a] = t + a * nb;
  return w;
}

float bits_float(uint32_t b) {
  union {
    uint32_t u;
    float f;
  } c;
  c.u = b;
  return c.f;
}

}  // namespace

extern "C" {

int64_t tomatis_declick_work_words(int64_t n_frames) {
  if (n_frames < 0) return 0;
  return 2 * kBins + kStateWords + 2 * (int64_t)kTileArrays * n_tiles(n_frames);
}

int tomatis_declick_dmax(const float* x, int64_t n_frames, int32_t ch, float* dmax, void* hs) {
  if (!x || n_frames < 0 || ch < 1 || ch > 128) return TOMATIS_E_ARG;
  if (n_frames < 2) return TOMATIS_OK;
  if (!dmax) return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  const i64 nd = n_frames - 1;
  if (ch <= 2 && aligned16(x) && aligned16(dmax)) {
    const dim3 g(dc_grid(((nd >> 2) + kT - 1) / kT));
    if (ch == 1) hipLaunchKernelGGL(k_dc_dmax_vec<1>, g, dim3(kT), 0, s, x, (i64)n_frames, dmax);
    else hipLaunchKernelGGL(k_dc_dmax_vec<2>, g, dim3(kT), 0, s, x, (i64)n_frames, dmax);
  } else {
    hipLaunchKernelGGL(k_dc_dmax_any, dim3(dc_grid((nd + kT - 1) / kT)), dim3(kT), 0, s, x,
                       (i64)n_frames, (int)ch, dmax);
  }
  return dc_launch();
}

int tomatis_declick_select(const float* v, int64_t n, int32_t centered, float center,
                           int64_t rank_lo, int64_t rank_hi, uint32_t* work, uint32_t* out_bits,
                           void* hs) {
  if (!v || !work || !out_bits || n < 1 || rank_lo < 0 || rank_hi < rank_lo || rank_hi >= n)
    return TOMATIS_E_ARG;
  if (n > (int64_t)UINT32_MAX) return TOMATIS_E_UNSUPPORTED;  // u32 histogram counts
  hipStream_t s = (hipStream_t)hs;
  Work w = carve(work, 1);
  const int vec = aligned16(v) ? 1 : 0;
  const dim3 g(dc_grid(((n >> 2) + kT - 1) / kT));
  hipLaunchKernelGGL(k_dc_sel_init, dim3(2 * kBins / kT), dim3(kT), 0, s, w.st, w.gh,
                     (uint32_t)rank_lo, (uint32_t)rank_hi);
  for (int pass = 0; pass < 3; ++pass) {
    if (centered)
      hipLaunchKernelGGL(k_dc_sel_hist<true>, g, dim3(kT), 0, s, v, (i64)n, vec, center, w.st,
                         w.gh, pass);
    else
      hipLaunchKernelGGL(k_dc_sel_hist<false>, g, dim3(kT), 0, s, v, (i64)n, vec, center, w.st,
                         w.gh, pass);
    hipLaunchKernelGGL(k_dc_sel_pick, dim3(1), dim3(kT), 0, s, w.st, w.gh, pass, out_bits);
  }
  return dc_launch();
}

int tomatis_declick_hits(const float* dmax, int64_t n, uint32_t thr_bits, int64_t pad, int64_t gap,
                         uint32_t* work, int64_t* counts, void* hs) {
  if (!dmax || !work || !counts || n < 1 || pad < 0 || gap < 0) return TOMATIS_E_ARG;
  if (n > ((int64_t)1 << 40) || pad > ((int64_t)1 << 40) || gap > ((int64_t)1 << 40))
    return TOMATIS_E_UNSUPPORTED;
  hipStream_t s = (hipStream_t)hs;
  const i64 nb = n_tiles(n), D = 2 * pad + 1 + gap;
  Work w = carve(work, n_tiles(n + 1));
  const float thr = bits_float(thr_bits);
  const int vec = aligned16(dmax) ? 1 : 0;
  int rc = dc_fail(hipMemsetAsync(counts, 0, 4 * sizeof(int64_t), s));
  if (rc != TOMATIS_OK) return rc;
  hipLaunchKernelGGL(k_dc_tile_hits, dim3((unsigned)nb), dim3(kT), 0, s, dmax, (i64)n, thr, vec,
                     w.tile[0], w.tile[1], w.tile[2]);
  hipLaunchKernelGGL(k_dc_link, dim3(1), dim3(kScanT), 0, s, nb, w.tile[0], w.tile[1], w.tile[2],
                     w.tile[3], w.tile[4], (i64*)counts);
  hipLaunchKernelGGL(k_dc_tile_heads<false>, dim3((unsigned)nb), dim3(kT), 0, s, dmax, (i64)n, thr,
                     vec, D, w.tile[3], w.tile[4], w.tile[5], w.tile[6], (const i64*)nullptr,
                     (const i64*)nullptr, (i64*)nullptr, (i64)0, (i64)pad, (i64*)counts);
  hipLaunchKernelGGL(k_dc_offsets, dim3(1), dim3(kScanT), 0, s, nb, w.tile[5], w.tile[6],
                     w.tile[7], w.tile[8], (i64*)counts);
  return dc_launch();
}

int tomatis_declick_segments(const float* dmax, int64_t n, uint32_t thr_bits, int64_t pad,
                             int64_t gap, int64_t max_fix, uint32_t* work, int64_t raw,
                             int64_t* bounds, int64_t* segs, int64_t* counts, void* hs) {
  if (!dmax || !work || !counts || n < 1 || pad < 0 || gap < 0 || raw < 0) return TOMATIS_E_ARG;
  if (n > ((int64_t)1 << 40) || pad > ((int64_t)1 << 40) || gap > ((int64_t)1 << 40))
    return TOMATIS_E_UNSUPPORTED;
  if (raw == 0) return TOMATIS_OK;
  if (!bounds || !segs) return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  const i64 nb = n_tiles(n), D = 2 * pad + 1 + gap;
  Work w = carve(work, n_tiles(n + 1));
  const float thr = bits_float(thr_bits);
  const int vec = aligned16(dmax) ? 1 : 0;
  hipLaunchKernelGGL(k_dc_tile_heads<true>, dim3((unsigned)nb), dim3(kT), 0, s, dmax, (i64)n, thr,
                     vec, D, w.tile[3], w.tile[4], (i64*)nullptr, (i64*)nullptr, w.tile[7],
                     w.tile[8], (i64*)bounds, (i64)raw, (i64)pad, (i64*)counts);
  hipLaunchKernelGGL(k_dc_filter, dim3(1), dim3(kScanT), 0, s, (const i64*)bounds, (i64)raw,
                     (i64)max_fix, (i64*)segs, (i64*)counts);
  return dc_launch();
}

int tomatis_declick_inpaint(const float* x, float* y, int64_t n_frames, int32_t ch,
                            const int64_t* segs, int64_t n_segs, void* hs) {
  if (n_frames < 0 || ch < 1 || ch > 128 || n_segs < 0) return TOMATIS_E_ARG;
  if (n_segs == 0) return TOMATIS_OK;
  if (!x || !y || !segs) return TOMATIS_E_ARG;
  if (n_segs > ((int64_t)1 << 31)) return TOMATIS_E_UNSUPPORTED;
  const int wpb = kT / 64;
  hipLaunchKernelGGL(k_dc_inpaint, dim3((unsigned)((n_segs + wpb - 1) / wpb)), dim3(kT), 0,
                     (hipStream_t)hs, x, y, (i64)n_frames, (int)ch, (const i64*)segs,
                     (i64)n_segs);
  return dc_launch();
}

}  // extern "C"
