// tm_align.hip — delay estimation on the device.
//
// find_delay_by_corr of the reference's workflow scripts
// (src/layer2_analyze_eq.py:17-52, src/calibrate_to_baseline_v2.py:46-82) as
// three kernel groups, each behind its own entry point:
//   power_mono + resample_poly(e, up, down) + "-= mean"  :31-33,43-45 -> k_al_envelope,
//                                                           k_al_sum, k_al_center
//   fftconvolve(mt_ds, mb_ds[::-1], "valid")             :47      -> k_al_xcorr
//   np.argmax                                            :48      -> k_al_argmax, k_al_decode
// and two pieces of src/compare_audio.py (row f7; its correlation is tm_fftcorr.hip):
//   power_mono, resample_poly(m - m.mean(), up, down)    :7-10,33-34 -> k_al_pm_sum, k_al_means,
//                                                           k_al_envelope<., true, ., .>
//   rms_db of power_mono(b) and of power_mono(b - g c)   :96-98   -> k_al_residual, k_al_means
// and the time-domain sums of src/compare_to_baseline.py's compute_metrics:
//   sum mb^2, sum mc^2, sum (mb - g mc)^2                :140-146,182-184 -> k_al_mono_sums,
//                                                           k_al_means
// One kernel decimates, for every ratio 1 <= up < down (48 kHz: 1 / 24, 44.1 kHz: 20 / 441,
// 192 kHz: 1 / 96), both mean orders, stereo or 1-D input.  al_envelope launches it with
// the sums of either order, and the three envelope entry points are argument checks in
// front of al_envelope: tomatis_align_envelope[_mean_first] pass channels = 2 and up = 1.
//
// Layout (wave64, 256-thread workgroups):
//  * envelope: polyphase, a resident grid over tiles of T outputs with the
//    samples and the taps of a tile in LDS; described at k_al_envelope.
//  * mean: a fixed grid of at most kSumGroups workgroups writes float64
//    partial sums (grid-stride, fixed order), every workgroup of the centring
//    pass adds them up in index order: the same mean in every workgroup and in
//    every run, no float atomics.
//  * correlation: direct float32 FMA.  A lane owns kR = 16 consecutive outputs
//    and slides a 32-word register window of t over the template: 16 new words
//    (four 16-byte LDS reads) and 16 template words (uniform LDS reads) feed
//    256 FMAs.  The workgroup's kT * kR outputs walk the template in blocks of
//    kJB taps staged in LDS (t window and template block, zero-filled past the
//    ends, so the inner loop has no bounds); sums run over kSB taps at a time
//    and are added to the running total in tap order, which keeps the float32
//    rounding of a 50 000-tap sum near sqrt(kSB) + sqrt(nb / kSB) ulps and the
//    result identical from run to run.  The t window is stored with four words
//    of padding after every 16 (lane stride 80 B): the 16-byte reads of the 16
//    lanes of one LDS group start on distinct multiples of four banks.
//  * argmax: 64-bit keys (order-preserving value bits << 32 | ~index): the
//    integer maximum is the largest value at the lowest index (np.argmax's
//    rule; NaN ranks above everything, as numpy's first NaN).  Per-lane keys,
//    wave and workgroup maxima, one integer atomic per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int kT = 256;                   // threads per workgroup
constexpr int kSumGroups = TOMATIS_ALIGN_MEAN_DOUBLES - 1;  // partial sums of the mean
constexpr int kMaxDown = 64;
constexpr int kR = 16;                    // outputs per lane of the correlation
constexpr int kOut = kT * kR;             // outputs per workgroup
constexpr int kJB = 1024;                 // template block staged in LDS
constexpr int kSB = 256;                  // taps per float32 partial sum
constexpr int kWin = kOut + kJB;          // t words staged per block
constexpr int kWinPad = kWin / 16 * 20;   // with 4 words of padding per 16

int al_fail(hipError_t e) { return e == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP; }
int al_launch() { return al_fail(hipGetLastError()); }

int al_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  return cus;
}

// workgroups of a fixed-order float64 sum over n items: min(ceil(n / kT), kSumGroups)
int sum_groups(i64 n) {
  const i64 want = (n + kT - 1) / kT;
  return (int)(want < kSumGroups ? want : kSumGroups);
}

// ---------------------------------------------------------------------------
// envelope: e = sqrt(0.5 (l l + r r) + 1e-12) in float32, and the sums behind its mean
// ---------------------------------------------------------------------------
__device__ __forceinline__ float power_mono(float l, float r) {
  const float p = __fmul_rn(0.5f, __fadd_rn(__fmul_rn(l, l), __fmul_rn(r, r)));
  return sqrtf(__fadd_rn(p, 1e-12f));
}

// Sum over the workgroup in a fixed order; the result in every thread.  sm: kT / 64 slots.
__device__ __forceinline__ double block_sum(double v, double* sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < kT / 64; ++i) s += sm[i];
  __syncthreads();
  return s;
}

// part[g] = float64 sum of y[i], i = g kT + t (mod G kT), G = gridDim.x
__global__ __launch_bounds__(kT) void k_al_sum(const float* __restrict__ y, i64 n,
                                                double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  double s = 0.0;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT)
    s += (double)y[i];
  s = block_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// part[g] = float64 sum of power_mono(x[i]), i = g kT + t (mod G kT), G = gridDim.x
template <bool VEC>
__global__ __launch_bounds__(kT) void k_al_pm_sum(const float* __restrict__ x, i64 n,
                                                   double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  double s = 0.0;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT) {
    if constexpr (VEC) {
      const float2 v = *reinterpret_cast<const float2*>(x + 2 * i);
      s += (double)power_mono(v.x, v.y);
    } else {
      s += (double)power_mono(x[2 * i], x[2 * i + 1]);
    }
  }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[r] = sum(part[r * stride + i], i < n_part) / n, r < n_res: one workgroup
__global__ __launch_bounds__(kT) void k_al_means(const double* __restrict__ part, int n_part,
                                                  int stride, int n_res, i64 n,
                                                  double* __restrict__ out) {
  __shared__ double sm[kT / 64];
  for (int r = 0; r < n_res; ++r) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_part; i += kT) s += part[r * stride + i];
    s = block_sum(s, sm);
    if (threadIdx.x == 0) out[r] = s / (double)n;
  }
}

// compare_audio.py:96-99: part[g] = float64 sum of power_mono(b)^2, part[kSumGroups + g] of
// power_mono(b - gain c)^2, squares in float32 as rms_db's x * x
template <bool VEC>
__global__ __launch_bounds__(kT) void k_al_residual(const float* __restrict__ b,
                                                     const float* __restrict__ c, i64 n,
                                                     float gain, double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  double sb = 0.0, sr = 0.0;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT) {
    float bl, br, cl, cr;
    if constexpr (VEC) {
      const float2 u = *reinterpret_cast<const float2*>(b + 2 * i);
      const float2 v = *reinterpret_cast<const float2*>(c + 2 * i);
      bl = u.x, br = u.y, cl = v.x, cr = v.y;
    } else {
      bl = b[2 * i], br = b[2 * i + 1], cl = c[2 * i], cr = c[2 * i + 1];
    }
    const float pb = power_mono(bl, br);
    const float pr = power_mono(__fsub_rn(bl, __fmul_rn(gain, cl)),
                                __fsub_rn(br, __fmul_rn(gain, cr)));
    sb += (double)__fmul_rn(pb, pb);
    sr += (double)__fmul_rn(pr, pr);
  }
  sb = block_sum(sb, sm);
  sr = block_sum(sr, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = sb;
    part[kSumGroups + blockIdx.x] = sr;
  }
}

// compare_to_baseline.py:140-146, :182-184: part[g], part[kSumGroups + g] and
// part[2 kSumGroups + g] = float64 sums of mb^2, mc^2 and (mb - gain mc)^2 for the float32
// power monos mb, mc; product, difference and squares in float32 as numpy forms them
template <bool VEC>
__global__ __launch_bounds__(kT) void k_al_mono_sums(const float* __restrict__ b,
                                                      const float* __restrict__ c, i64 n,
                                                      float gain, double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  double sb = 0.0, sc = 0.0, sr = 0.0;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT) {
    float bl, br, cl, cr;
    if constexpr (VEC) {
      const float2 u = *reinterpret_cast<const float2*>(b + 2 * i);
      const float2 v = *reinterpret_cast<const float2*>(c + 2 * i);
      bl = u.x, br = u.y, cl = v.x, cr = v.y;
    } else {
      bl = b[2 * i], br = b[2 * i + 1], cl = c[2 * i], cr = c[2 * i + 1];
    }
    const float mb = power_mono(bl, br), mc = power_mono(cl, cr);
    const float r = __fsub_rn(mb, __fmul_rn(mc, gain));
    sb += (double)__fmul_rn(mb, mb);
    sc += (double)__fmul_rn(mc, mc);
    sr += (double)__fmul_rn(r, r);
  }
  sb = block_sum(sb, sm);
  sc = block_sum(sc, sm);
  sr = block_sum(sr, sm);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = sb;
    part[kSumGroups + blockIdx.x] = sc;
    part[2 * kSumGroups + blockIdx.x] = sr;
  }
}

// y -= float32(sum(part) / n); mean[0] = sum(part) / n
__global__ __launch_bounds__(kT) void k_al_center(float* __restrict__ y, i64 n,
                                                   const double* __restrict__ part, int n_part,
                                                   double* __restrict__ mean) {
  __shared__ double sm[kT / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += kT) s += part[i];
  const double m = block_sum(s, sm) / (double)n;
  const float mf = (float)m;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT)
    y[i] = __fsub_rn(y[i], mf);
  if (blockIdx.x == 0 && threadIdx.x == 0) mean[0] = m;
}

// ---------------------------------------------------------------------------
// "valid" correlation c[k] = sum_j t[k + j] b[j]
// ---------------------------------------------------------------------------
__device__ __forceinline__ int win_at(int i) { return (i >> 4) * 20 + (i & 15); }

// 16 taps: outputs r = 0..15 read window words (OFF + r + u) mod 32
template <int OFF>
__device__ __forceinline__ void taps16(float (&acc)[kR], const float (&w)[32],
                                       const float* __restrict__ bb) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float4 h = *reinterpret_cast<const float4*>(bb + 4 * v);
    const float hh[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int r = 0; r < kR; ++r) acc[r] = fmaf(w[(OFF + r + 4 * v + k) & 31], hh[k], acc[r]);
    }
  }
}

template <int OFF>
__device__ __forceinline__ void load16(float (&w)[32], const float* __restrict__ p) {
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float4 a = *reinterpret_cast<const float4*>(p + 4 * v);
    w[OFF + 4 * v] = a.x;
    w[OFF + 4 * v + 1] = a.y;
    w[OFF + 4 * v + 2] = a.z;
    w[OFF + 4 * v + 3] = a.w;
  }
}

__global__ __launch_bounds__(kT) void k_al_xcorr(const float* __restrict__ t, i64 nt,
                                                  const float* __restrict__ b, i64 nb,
                                                  float* __restrict__ c, i64 nc) {
  __shared__ __attribute__((aligned(16))) float win[kWinPad];
  __shared__ __attribute__((aligned(16))) float tb[kJB];
  const int tid = threadIdx.x;
  const i64 kb = (i64)blockIdx.x * kOut;
  float tot[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) tot[r] = 0.0f;
  for (i64 j0 = 0; j0 < nb; j0 += kJB) {
    __syncthreads();  // the previous block's reads
    for (int i = tid; i < kWin; i += kT) {
      const i64 g = kb + j0 + i;
      win[win_at(i)] = g < nt ? t[g] : 0.0f;
    }
    for (int i = tid; i < kJB; i += kT) tb[i] = j0 + i < nb ? b[j0 + i] : 0.0f;
    __syncthreads();
    const i64 left = nb - j0;
    const int nsub = left >= kJB ? kJB / kSB : (int)((left + kSB - 1) / kSB);
    for (int sbi = 0; sbi < nsub; ++sbi) {
      const int s0 = sbi * kSB;
      float acc[kR], w[32];
#pragma unroll
      for (int r = 0; r < kR; ++r) acc[r] = 0.0f;
      // word i of this lane's window is t[kb + j0 + kR tid + i]: 16-word row tid + i / 16
      const float* row = win + (tid + s0 / 16) * 20;
      load16<0>(w, row);
#pragma unroll 1
      for (int s = 0; s < kSB; s += 32) {
        load16<16>(w, row + (s / 16 + 1) * 20);
        taps16<0>(acc, w, tb + s0 + s);
        load16<0>(w, row + (s / 16 + 2) * 20);
        taps16<16>(acc, w, tb + s0 + s + 16);
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) tot[r] += acc[r];
    }
  }
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const i64 k = kb + (i64)tid * kR + r;
    if (k < nc) c[k] = tot[r];
  }
}

// ---------------------------------------------------------------------------
// argmax, the lowest index on ties
// ---------------------------------------------------------------------------
__device__ __forceinline__ u64 arg_key(float v, i64 i) {
  uint32_t u;
  if (v != v) {
    u = 0xFFFFFFFFu;  // NaN: above everything
  } else {
    u = __float_as_uint(v == 0.0f ? 0.0f : v);  // -0 == +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((u64)u << 32) | (u64)(0xFFFFFFFFu - (uint32_t)i);
}

__global__ __launch_bounds__(kT) void k_al_argmax(const float* __restrict__ c, i64 n, u64* best) {
  __shared__ u64 sm[kT / 64];
  u64 m = 0;
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < n; i += (i64)gridDim.x * kT) {
    const u64 k = arg_key(c[i], i);
    m = k > m ? k : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const u64 v = __shfl_xor(m, o, 64);
    m = v > m ? v : m;
  }
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kT / 64; ++i) m = sm[i] > m ? sm[i] : m;
    atomicMax(best, m);
  }
}

__global__ void k_al_decode(const float* __restrict__ c, i64* index, float* value) {
  const u64 k = *reinterpret_cast<const u64*>(index);
  const i64 i = (i64)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFu));
  *index = i;
  *value = c[i];
}

bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1u)) == 0; }

// ---------------------------------------------------------------------------
// the decimator: resample_poly(e, up, down), 1 <= up < down
// ---------------------------------------------------------------------------
// With c = down j + half, p = c mod up and ih = c / up, output j is
//   y[j] = sum_v taps[p + up (K - 1 - v)] e[ih - (K - 1) + v],  v < K = ceil(n_taps / up)
// (a tap index >= n_taps counts as a zero tap; for up == 1 this is y[j] =
// sum_u taps[n_taps - 1 - u] e[down j - half + u]).  e is formed from 8-byte
// stereo loads as it is staged (the PCM is read once; the halo of neighbouring
// tiles comes from L2), less float32(mu[0]) inside the range in the mean-first
// order (SUB; compare_audio.py:33-34 removes the mean before it decimates),
// and is zero outside the range.  A workgroup of kT threads owns
// T consecutive outputs, S = kT / T threads each: thread (o, si) = (tid % T,
// tid / T) sums the terms v in [si C, (si + 1) C) of output j0 + o in four
// chains joined pairwise (up > 1: by v mod 4; up == 1: by the place in a row
// of down samples, the tail of a row on the first chain); the S partial sums
// are added in the order of si.  T, S and C depend on (up, down, n_taps)
// alone, and a tile's result does not depend on the workgroup that computes
// it: the workgroups are resident and walk the tiles, so each builds its tap
// table once.  With the reference's 20 down + 1 taps, up == 1 runs 256 x 1 up
// to down = 53 (48 kHz: 24, 96 kHz: 48), 128 x 2 up to 95, 64 x 4 from 96 (192 kHz) on.
//   stage: the W samples from g0 = ih(j0) - (K - 1) on; sample g0 + i at word
//          i + pad (i / down).  pad = 1 for up == 1 and an even down: lane o
//          then starts at o (down + 1), an odd stride over the 32 banks of a
//          4-byte read, where o down would put the 32 lanes of a half wave on
//          gcd(down, 32) times fewer banks (one bank at 192 kHz, down = 96).
//          For up > 1 the starts floor((p0 + down o) / up) step by a fraction
//          and a pad would break at another v in every lane; pad = 0, and the
//          441 family (22.05, 44.1, 88.2 words per lane) reads 2-way
//          conflicted (DESIGN.md §7f has the count per ratio).
//   tab:   the taps by phase, tab[p Ks + v] = taps[p + up (K - 1 - v)]: a
//          thread's taps are consecutive words.  up > 1 reads them four at a
//          time; Ks / 4 is odd, so the rows of 16 phases start on 16 distinct
//          16-byte slots of the 64 banks.  up == 1 has one row, every lane
//          reads the same word (a broadcast).  Where that row would leave
//          room for fewer than 64 outputs' samples (down above 150) the taps
//          are read from global memory instead and tab is empty.
//   red:   the kT partial sums.
constexpr int kRatMaxDown = 512;
constexpr int kRatMaxUp = 64;
constexpr int kEnvLdsBytes = 64 * 1024;

struct EnvPlan {
  int up, down, n_taps, K, Ks, T, C, W, pad, stage_words, tab_words;
};

__device__ __forceinline__ float env_join(float a0, float a1, float a2, float a3) {
  return (a0 + a1) + (a2 + a3);
}

// up == 1, the terms v in [v, v1) row by row of down samples: tap v is h[v] (REV: h[-v]),
// sample v lies at sp[v + pad (v / down)]
template <bool REV>
__device__ __forceinline__ float env_rows(const float* __restrict__ h, const float* sp, int v,
                                          int v1, int down, int pad) {
  float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
  while (v < v1) {
    const int q = v / down;
    const int ve = min(v1, (q + 1) * down);
    const float* col = sp + q * pad;
    for (; v + 4 <= ve; v += 4) {
      a0 = fmaf(REV ? h[-v] : h[v], col[v], a0);
      a1 = fmaf(REV ? h[-v - 1] : h[v + 1], col[v + 1], a1);
      a2 = fmaf(REV ? h[-v - 2] : h[v + 2], col[v + 2], a2);
      a3 = fmaf(REV ? h[-v - 3] : h[v + 3], col[v + 3], a3);
    }
    for (; v < ve; ++v) a0 = fmaf(REV ? h[-v] : h[v], col[v], a0);
  }
  return env_join(a0, a1, a2, a3);
}

// TAPS: 0 up > 1, the phase table in LDS; 1 up == 1, taps from global memory;
// 2 up == 1, the reversed taps in LDS
template <bool VEC, bool SUB, bool MONO, int TAPS>
__global__ __launch_bounds__(kT) void k_al_envelope(const float* __restrict__ x, i64 len,
                                                         const float* __restrict__ taps,
                                                         EnvPlan pl, float* __restrict__ out,
                                                         i64 n_out, int tiles,
                                                         const double* __restrict__ mu) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* stage = lds;
  float* tab = lds + pl.stage_words;
  float* red = tab + pl.tab_words;
  float mf = 0.0f;
  if constexpr (SUB) mf = (float)mu[0];
  const int tid = threadIdx.x, T = pl.T, up = pl.up, down = pl.down, K = pl.K;
  if constexpr (TAPS != 1) {  // once per workgroup; the first barrier of the loop publishes it
    for (int i = tid; i < pl.tab_words; i += kT) {
      const int p = i / pl.Ks, v = i - p * pl.Ks;
      const int m = p + up * (K - 1 - v);
      tab[i] = (v < K && m < pl.n_taps) ? taps[m] : 0.0f;
    }
  }
  const int si = tid / T, o = tid - si * T;
  const int v0 = si * pl.C, v1 = min(K, v0 + pl.C);
  // a workgroup walks the tiles of T outputs blockIdx.x, blockIdx.x + gridDim.x, ...
  for (i64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const i64 j0 = (i64)tile * T;
    const i64 c0 = (i64)down * j0 + (pl.n_taps - 1) / 2;
    const i64 ih0 = c0 / up;
    const int p0 = (int)(c0 - ih0 * up);
    const i64 g0 = ih0 - (K - 1);
    __syncthreads();  // the previous tile's reads of stage and red
    for (int i0 = tid; i0 < pl.W; i0 += 4 * kT) {
      float2 raw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {  // four loads in flight, from addresses clamped into the range
        i64 g = g0 + i0 + k * kT;
        g = g < 0 ? 0 : (g < len ? g : len - 1);
        if constexpr (MONO) raw[k] = make_float2(x[g], 0.0f);
        else if constexpr (VEC) raw[k] = *reinterpret_cast<const float2*>(x + 2 * g);
        else raw[k] = make_float2(x[2 * g], x[2 * g + 1]);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * kT;
        const i64 g = g0 + i;
        float e = 0.0f;  // the sub-range is a signal of its own: zeros outside it
        if (g >= 0 && g < len) {
          if constexpr (MONO) e = raw[k].x; else e = power_mono(raw[k].x, raw[k].y);
          if constexpr (SUB) e = __fsub_rn(e, mf);
        }
        if (i < pl.W) {
          if constexpr (TAPS != 0) stage[i + pl.pad * (i / down)] = e; else stage[i] = e;
        }
      }
    }
    __syncthreads();
    const i64 j = j0 + o;
    float part = 0.0f;
    if (j < n_out && v0 < v1) {
      if constexpr (TAPS != 0) {
        const float* sp = stage + o * (down + pl.pad);  // sample o down
        if constexpr (TAPS == 1)
          part = env_rows<true>(taps + (pl.n_taps - 1), sp, v0, v1, down, pl.pad);
        else
          part = env_rows<false>(tab, sp, v0, v1, down, pl.pad);
      } else {
        const int xo = p0 + down * o, ao = xo / up, p = xo - ao * up;
        const float* sp = stage + ao;
        const float* h = tab + p * pl.Ks;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        int v = v0;
#pragma unroll 4
        for (; v + 4 <= v1; v += 4) {
          const float4 t = *reinterpret_cast<const float4*>(h + v);
          a0 = fmaf(t.x, sp[v], a0);
          a1 = fmaf(t.y, sp[v + 1], a1);
          a2 = fmaf(t.z, sp[v + 2], a2);
          a3 = fmaf(t.w, sp[v + 3], a3);
        }
        for (; v < v1; ++v) a0 = fmaf(h[v], sp[v], a0);
        part = env_join(a0, a1, a2, a3);
      }
    }
    if (T == kT) {
      if (j < n_out) out[j] = part;
    } else {
      red[tid] = part;  // [si][o]
      __syncthreads();
      if (tid < T && j < n_out) {
        float s = red[o];
        for (int k = 1; k < kT / T; ++k) s += red[k * T + o];
        out[j] = s;
      }
    }
  }
}

// the largest T = 256, 128, ... 1 outputs per workgroup whose staging fits beside the tap
// table (lds_taps) or alone (up == 1 only)
bool env_plan_for(int up, int down, int n_taps, bool lds_taps, EnvPlan* pl) {
  pl->up = up, pl->down = down, pl->n_taps = n_taps;
  pl->K = (n_taps + up - 1) / up;
  pl->Ks = 4 * (((pl->K + 3) / 4) | 1);
  pl->pad = (up == 1 && (down & 1) == 0) ? 1 : 0;
  pl->tab_words = lds_taps ? up * pl->Ks : 0;
  for (int T = kT;; T >>= 1) {
    const int S = kT / T;
    pl->T = T;
    pl->C = ((pl->K + S - 1) / S + 3) / 4 * 4;
    pl->W = (up - 1 + down * (T - 1)) / up + pl->K;
    pl->stage_words = (pl->W + pl->pad * (pl->W / down + 1) + 3) / 4 * 4;
    const size_t bytes = sizeof(float) * ((size_t)pl->stage_words + pl->tab_words + kT);
    if (bytes <= (size_t)kEnvLdsBytes) return true;
    if (T == 1) return false;
  }
}

bool env_plan(int up, int down, int n_taps, EnvPlan* pl) {
  if (env_plan_for(up, down, n_taps, true, pl) && (up > 1 || pl->T >= 64)) return true;
  return up == 1 && env_plan_for(up, down, n_taps, false, pl);
}

// the decimator's launch; mu: the mean to remove first (mean-first order) or null
int al_decimate(const float* xs, i64 len, bool mono, const float* taps, const EnvPlan& pl,
                float* out, i64 n_out, const double* mu, hipStream_t s) {
  const size_t lds = sizeof(float) * ((size_t)pl.stage_words + pl.tab_words + kT);
  const i64 tiles = (n_out + pl.T - 1) / pl.T;
  if (tiles > 0x7FFFFFFF) return TOMATIS_E_UNSUPPORTED;
  const i64 cap = (i64)al_cus() * 4;  // resident workgroups, each builds its phase table once
  const unsigned groups = (unsigned)(tiles < cap ? tiles : cap);
  const bool vec = !mono && aligned(xs, 8);
#define TM_AL_ENV(V, S, M, U)                                                               \
  hipLaunchKernelGGL((k_al_envelope<V, S, M, U>), dim3(groups), dim3(kT), lds, s, xs, len, \
                     taps, pl, out, n_out, (int)tiles, mu)
#define TM_AL_ENV_U(V, S, M)                             \
  do {                                                   \
    if (pl.up > 1) TM_AL_ENV(V, S, M, 0);                \
    else if (pl.tab_words == 0) TM_AL_ENV(V, S, M, 1);   \
    else TM_AL_ENV(V, S, M, 2);                          \
  } while (0)
#define TM_AL_ENV_S(V, M) \
  do { if (mu) TM_AL_ENV_U(V, true, M); else TM_AL_ENV_U(V, false, M); } while (0)
  if (mono) TM_AL_ENV_S(false, true);
  else if (vec) TM_AL_ENV_S(true, false);
  else TM_AL_ENV_S(false, false);
#undef TM_AL_ENV_S
#undef TM_AL_ENV_U
#undef TM_AL_ENV
  return TOMATIS_OK;
}

// The envelope of one range with its mean removed, out_mean[0] the mean, out_mean[1..] the
// partial sums.  Mean first: the float64 mean of e, then the decimator on e - float32(mean).
// Mean last: the decimator, then the float64 mean of its output, then the centring pass.
int al_envelope(const float* xs, i64 len, int channels, int up, int down, const float* taps,
                int n_taps, bool mean_first, float* out, double* out_mean, hipStream_t s) {
  EnvPlan pl;
  if (!env_plan(up, down, n_taps, &pl)) return TOMATIS_E_UNSUPPORTED;
  const bool mono = channels == 1;
  const i64 n_out = (len * up + down - 1) / down;
  double* part = out_mean + 1;
  int rc;
  if (mean_first) {
    const int G = sum_groups(len);
    if (mono)
      hipLaunchKernelGGL(k_al_sum, dim3(G), dim3(kT), 0, s, xs, len, part);
    else if (aligned(xs, 8))
      hipLaunchKernelGGL(k_al_pm_sum<true>, dim3(G), dim3(kT), 0, s, xs, len, part);
    else
      hipLaunchKernelGGL(k_al_pm_sum<false>, dim3(G), dim3(kT), 0, s, xs, len, part);
    hipLaunchKernelGGL(k_al_means, dim3(1), dim3(kT), 0, s, (const double*)part, G, 0, 1, len,
                       out_mean);
    rc = al_decimate(xs, len, mono, taps, pl, out, n_out, out_mean, s);
    return rc != TOMATIS_OK ? rc : al_launch();
  }
  rc = al_decimate(xs, len, mono, taps, pl, out, n_out, nullptr, s);
  if (rc != TOMATIS_OK) return rc;
  const int G = sum_groups(n_out);
  hipLaunchKernelGGL(k_al_sum, dim3(G), dim3(kT), 0, s, (const float*)out, n_out, part);
  const i64 want = (n_out + kT - 1) / kT, cap = (i64)al_cus() * 8;
  hipLaunchKernelGGL(k_al_center, dim3((unsigned)(want < cap ? want : cap)), dim3(kT), 0, s, out,
                     n_out, (const double*)part, G, out_mean);
  return al_launch();
}

// tomatis_align_envelope[_mean_first]: stereo, up == 1, down <= kMaxDown
int al_env_args(const float* x, int64_t n_total, int64_t start, int64_t len, int32_t down,
                const float* taps, int32_t n_taps, float* out, double* out_mean) {
  if (!x || !taps || !out || !out_mean || n_total < 0 || start < 0 || len < 1 ||
      len > n_total - start || down < 2 || n_taps < 1 || (n_taps & 1) == 0)
    return TOMATIS_E_ARG;
  if (down > kMaxDown || n_taps > 20 * down + 1) return TOMATIS_E_UNSUPPORTED;
  return TOMATIS_OK;
}

}  // namespace

extern "C" {

int tomatis_align_envelope_rational(const float* x, int64_t n_total, int64_t start, int64_t len,
                                    int32_t channels, int32_t up, int32_t down,
                                    const float* taps, int32_t n_taps, int32_t mean_first,
                                    float* out, double* out_mean, void* hs) {
  if (!x || !taps || !out || !out_mean || n_total < 0 || start < 0 || len < 1 ||
      len > n_total - start || (channels != 1 && channels != 2) || up < 1 || up >= down ||
      n_taps < 1 || (n_taps & 1) == 0)
    return TOMATIS_E_ARG;
  if (down > kRatMaxDown || up > kRatMaxUp || n_taps > 20 * down + 1 ||
      len > (int64_t)1 << 55)
    return TOMATIS_E_UNSUPPORTED;
  return al_envelope(x + (i64)channels * start, (i64)len, (int)channels, (int)up, (int)down, taps,
                     (int)n_taps, mean_first != 0, out, out_mean, (hipStream_t)hs);
}

int tomatis_align_envelope_mean_first(const float* x, int64_t n_total, int64_t start, int64_t len,
                                      int32_t down, const float* taps, int32_t n_taps, float* out,
                                      double* out_mean, void* hs) {
  const int rc = al_env_args(x, n_total, start, len, down, taps, n_taps, out, out_mean);
  if (rc != TOMATIS_OK) return rc;
  return al_envelope(x + 2 * start, (i64)len, 2, 1, (int)down, taps, (int)n_taps, true, out,
                     out_mean, (hipStream_t)hs);
}

int tomatis_align_envelope(const float* x, int64_t n_total, int64_t start, int64_t len,
                           int32_t down, const float* taps, int32_t n_taps, float* out,
                           double* out_mean, void* hs) {
  const int rc = al_env_args(x, n_total, start, len, down, taps, n_taps, out, out_mean);
  if (rc != TOMATIS_OK) return rc;
  return al_envelope(x + 2 * start, (i64)len, 2, 1, (int)down, taps, (int)n_taps, false, out,
                     out_mean, (hipStream_t)hs);
}

int tomatis_compare_residual(const float* b, const float* c, int64_t n, float gain, double* out,
                             void* hs) {
  if (!b || !c || !out || n < 1) return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  const int G = sum_groups((i64)n);
  if (aligned(b, 8) && aligned(c, 8))
    hipLaunchKernelGGL(k_al_residual<true>, dim3(G), dim3(kT), 0, s, b, c, (i64)n, gain, out + 2);
  else
    hipLaunchKernelGGL(k_al_residual<false>, dim3(G), dim3(kT), 0, s, b, c, (i64)n, gain, out + 2);
  hipLaunchKernelGGL(k_al_means, dim3(1), dim3(kT), 0, s, (const double*)(out + 2), G, kSumGroups,
                     2, (i64)n, out);
  return al_launch();
}

int tomatis_cmp_mono_sums(const float* b, const float* c, int64_t n, float gain, double* out,
                          void* hs) {
  if (!b || !c || !out || n < 1) return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  const int G = sum_groups((i64)n);
  if (aligned(b, 8) && aligned(c, 8))
    hipLaunchKernelGGL(k_al_mono_sums<true>, dim3(G), dim3(kT), 0, s, b, c, (i64)n, gain, out + 3);
  else
    hipLaunchKernelGGL(k_al_mono_sums<false>, dim3(G), dim3(kT), 0, s, b, c, (i64)n, gain,
                       out + 3);
  // the sums themselves: k_al_means with a count of one
  hipLaunchKernelGGL(k_al_means, dim3(1), dim3(kT), 0, s, (const double*)(out + 3), G, kSumGroups,
                     3, (i64)1, out);
  return al_launch();
}

int tomatis_align_xcorr(const float* t, int64_t nt, const float* b, int64_t nb, float* out,
                        void* hs) {
  if (!t || !b || !out || nb < 1 || nt < nb) return TOMATIS_E_ARG;
  const i64 nc = nt - nb + 1;
  const i64 groups = (nc + kOut - 1) / kOut;
  if (groups > 0x7FFFFFFF) return TOMATIS_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_al_xcorr, dim3((unsigned)groups), dim3(kT), 0, (hipStream_t)hs, t, (i64)nt,
                     b, (i64)nb, out, nc);
  return al_launch();
}

int tomatis_align_argmax(const float* c, int64_t n, int64_t* out_index, float* out_value,
                         void* hs) {
  if (!c || !out_index || !out_value || n < 1) return TOMATIS_E_ARG;
  if (n > (int64_t)0xFFFFFFFF) return TOMATIS_E_UNSUPPORTED;  // 32-bit index in the key
  hipStream_t s = (hipStream_t)hs;
  const int rc = al_fail(hipMemsetAsync(out_index, 0, sizeof(int64_t), s));
  if (rc != TOMATIS_OK) return rc;
  const i64 want = (n + kT - 1) / kT, cap = (i64)al_cus() * 8;
  hipLaunchKernelGGL(k_al_argmax, dim3((unsigned)(want < cap ? want : cap)), dim3(kT), 0, s, c,
                     (i64)n, reinterpret_cast<u64*>(out_index));
  hipLaunchKernelGGL(k_al_decode, dim3(1), dim3(1), 0, s, c, (i64*)out_index, out_value);
  return al_launch();
}

}  // extern "C"
