// tm_analysis.hip — analysis spectra on the device (SURVEY.md §8 rows f3/f4,
// f8, f9, f11).
//
// The reference's validators and calibration tools run the same framing + real
// FFT as the processors, then reduce over bins or frames:
//   compare_audio.stft_mag_avg                 src/compare_audio.py:12-24
//       mean over frames of |rfft(win * x)|    -> k_an_spec_pair<MAG>, k_an_frame_mean
//   layer2_analyze_eq.stft_logpower_median     src/layer2_analyze_eq.py:54-88
//       frames with rms_dbfs(power_mono) > music_dbfs, median over frames of
//       10 log10(|rfft(win * power_mono)|^2 + EPS)
//                                              -> k_an_frame_r, k_an_select,
//                                                 k_an_spec_pair<LOGPOW>, median kernels
//   validate_layer1.compute_conditional_spectrum  src/validate_layer1.py:261-389
//       stable C1/C2 frames with level >= threshold, median over frames of
//       mean_c|Y_c| / max(mean_c|X_c|, 1e-10)  -> k_an_frame_r, k_an_select,
//                                                 k_an_verify (rows, no anchor),
//                                                 median kernels
//   calibrate_to_baseline_v2.stft_band_tilt    src/calibrate_to_baseline_v2.py:17-31
//       per frame two band sums of |rfft(win * power_mono)|^2  -> k_an_band_pair
//   compare_to_baseline.avg_spectrum_db        src/compare_to_baseline.py:105-122
//       mean over frames, in float64, of 10 log10(|rfft(win * power_mono)|^2 + EPS)
//                                              -> k_an_spec_mean, k_an_spec_mean_fold
//   verify_tomatis_15db_v2 (the acceptance validator)  src/verify_tomatis_15db_v2.py
//       :307-354 ratio rows divided by their mean over an anchor band, :451-470
//       band energies of input and output, :90 the DC mean
//                                              -> k_an_verify, k_an_sum_part / _fold
//   reverse_engineer_params / verify_tilt_amplitude (parameter recovery, row f11)
//       src/reverse_engineer_params.py:118-143, src/verify_tilt_amplitude.py:74-99
//       per frame the dB difference of the output's and the input's power-mono
//       spectra, reduced to two band means or to a mean row over a frame list
//                                              -> k_an_pair_tilt, k_an_pair_diff_mean
//
// Frames: f = 0 .. F-1 start at f*hop, F = frame_count (every frame lies inside
// the signal, as in all the reference loops).
//
// Layout and kernels (HBM-bound streaming work, no MFMA):
//  * The six spectrum kernels share one frame front end (below, "The frame
//    front end"): one 256-thread workgroup stages two real signals as a + ib in
//    LDS (coalesced loads of the hop-strided PCM) -- a frame PAIR of one signal
//    (k_an_spec_pair, k_an_band_pair, k_an_spec_mean) or one frame of an
//    input/output pair (k_an_verify per channel, k_an_pair_tilt,
//    k_an_pair_diff_mean) -- runs one complex FFT and splits it with
//    Z[k] +- conj(Z[n-k]).  Stockham autosort FFT in LDS (one radix-2 stage when
//    log2 n is odd, then radix-4 stages; every stage reads its butterflies into
//    registers, barrier, writes, barrier), twiddles from a float table built in
//    double precision once per size.  Any n_fft >= 16 (as np.fft.rfft): powers
//    of two up to 16384 directly, other lengths up to 8192 by Bluestein's
//    chirp-z over M = 2^k >= 2n - 1 in the same LDS buffer (tlds::lds_dft,
//    tables per n from tm_host_dsp.h).  Each kernel holds its own arithmetic
//    and little else; sums over bins and frames are fixed-order (block_sums,
//    slab_sums): no atomics, the same bits in every run.
//  * k_an_frame_r: numpy's pairwise mean of m^2 per frame, restated exactly
//    (128-sample leaves of 8 sequential chains, fixed 8-chain tree, perfect tree
//    over leaves; correctly rounded sqrtf, -ffp-contract=off) so level gating is
//    decided on the bit pattern of r, like the processors' gate.  Other frame
//    lengths take k_an_frame_r_pw: numpy's tree for that length (leaves +
//    postfix program, NPY_BUFSIZE chunks) built on the host.
//  * median: per-bin radix select over the frame axis on order-preserving u32
//    keys, 8-bit digits, 4 passes (+1 min pass for even counts); each pass is a
//    grid of (64-bin group x frame split) workgroups building LDS histograms
//    (digit-major, lane = bin: conflict-free) flushed with global atomics, then
//    a per-bin pick.  numpy's even-count rule: fl32(fl32(v_lo + v_hi) / 2).
//  * k_an_frame_mean: per-bin sequential float32 sum over frames then / F —
//    numpy's axis-0 reduction order of np.stack(rows).mean(axis=0).
//  * Host: every entry point checks its own arguments, then frame_count,
//    bands_ok, a SpecArgs filled by name and completed by spec_args (M and the
//    tables, cached per device by cached()), and a launch through dispatch_m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <limits>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/tomatis_hip.h"
#include "tm_host_dsp.h"
#include "tm_lds_fft.h"

namespace {

constexpr int kT = 256;                // threads per spectrum workgroup
constexpr int kMaxTreeN = 8192;        // k_an_frame_r: powers of two in [256, 8192]
constexpr int kMaxM = 16384;           // largest FFT in LDS (128 KiB of float2)
constexpr int kMinN = 16;              // smallest spectrum n_fft
constexpr int kPwMax = 512;            // k_an_frame_r_pw leaves (windows <= 65536)
constexpr int kLevelPowerMean = 2;     // k_an_frame_r_pw only: tomatis_an_frame_power_mean's term
constexpr int kMaxMeanWin = 65536;     // tomatis_an_frame_power_mean
constexpr float kEps = 1e-12f;

int an_fail(hipError_t e) { return e == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP; }
int an_launch() { return an_fail(hipGetLastError()); }

bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// FFT size in LDS for a length-n DFT (0: unsupported)
int dft_m(int n) {
  if (n < kMinN) return 0;
  const int M = is_pow2(n) ? n : thost::bluestein_m(n);
  return M <= kMaxM ? M : 0;
}

// ---------------------------------------------------------------------------
// twiddle table tw[t] = exp(-2 pi i t / n), computed in double, cached per n
// ---------------------------------------------------------------------------
__global__ void k_an_twiddle(float2* tw, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  double s, c;
  sincospi(-2.0 * (double)t / (double)n, &s, &c);
  tw[t] = make_float2((float)c, (float)s);
}

// Device tables are built once per (device, n) and kept for the life of the
// process: cached() looks one up under the lock and, where it is missing, keeps
// what build(&v) made (build frees whatever it allocated before it fails).
template <typename V>
using Cache = std::map<std::pair<int, int>, V>;
std::mutex g_cache_mu;

template <typename V, typename B>
int cached(Cache<V>& cache, int n, V* out, B&& build) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TOMATIS_E_HIP;
  std::lock_guard<std::mutex> lk(g_cache_mu);
  auto it = cache.find({dev, n});
  if (it == cache.end()) {
    V v{};
    const int rc = build(&v);
    if (rc != TOMATIS_OK) return rc;
    it = cache.emplace(std::make_pair(dev, n), v).first;
  }
  *out = it->second;
  return TOMATIS_OK;
}

template <typename T>
int upload(const std::vector<T>& v, T** out) {
  T* p = nullptr;
  if (hipMalloc(&p, sizeof(T) * v.size()) != hipSuccess) return TOMATIS_E_NOMEM;
  if (hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return TOMATIS_E_HIP;
  }
  *out = p;
  return TOMATIS_OK;
}

template <typename T, typename U>  // both tables or neither
int upload2(const std::vector<T>& a, T** pa, const std::vector<U>& b, U** pb) {
  int rc = upload(a, pa);
  if (rc == TOMATIS_OK && (rc = upload(b, pb)) != TOMATIS_OK) (void)hipFree(*pa);
  return rc;
}

struct Chirp {  // Bluestein tables for one n (tm_host_dsp.h bluestein_tables)
  float2* b = nullptr;
  float2* h = nullptr;
};

int chirp_tables(int n, int M, Chirp* out) {
  static Cache<Chirp> cache;
  return cached(cache, n, out, [&](Chirp* c) -> int {
    std::vector<float2> bf, hf;
    thost::bluestein_tables(n, M, bf, hf);
    return upload2(bf, &c->b, hf, &c->h);
  });
}

struct PwProg {  // numpy's pairwise tree over one frame length
  int2* leaf = nullptr;
  int16_t* prog = nullptr;
  int n_leaf = 0, n_prog = 0;
};

int pw_program(int n, PwProg* out) {
  static Cache<PwProg> cache;
  return cached(cache, n, out, [&](PwProg* q) -> int {
    std::vector<int2> lv;
    std::vector<int16_t> prog;
    thost::pw_program(n, lv, prog);
    if ((int)lv.size() > kPwMax) return TOMATIS_E_UNSUPPORTED;
    q->n_leaf = (int)lv.size();
    q->n_prog = (int)prog.size();
    return upload2(lv, &q->leaf, prog, &q->prog);
  });
}

int twiddles(int n, hipStream_t s, const float2** out) {
  static Cache<const float2*> cache;
  return cached(cache, n, out, [&](const float2** tw) -> int {
    float2* p = nullptr;
    if (hipMalloc(&p, sizeof(float2) * n) != hipSuccess) return TOMATIS_E_NOMEM;
    hipLaunchKernelGGL(k_an_twiddle, dim3((n + 255) / 256), dim3(256), 0, s, p, n);
    int rc = an_launch();
    if (rc == TOMATIS_OK) rc = an_fail(hipStreamSynchronize(s));  // visible to every stream
    if (rc != TOMATIS_OK) (void)hipFree(p);
    else *tw = p;
    return rc;
  });
}

// ---------------------------------------------------------------------------
// per-sample mono values
// ---------------------------------------------------------------------------
// validate_layer1.py:304-306 / process_tomatis.py:369-371:
//   mono = sqrt(mean(frame**2, axis=1)); rms uses mono*mono
template <int CH>
__device__ __forceinline__ float m2_chmean(const float* __restrict__ x, int64_t p, float sc) {
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const float v = x[p * CH + c] * sc;
    acc = acc + v * v;
  }
  const float mean = (CH == 1) ? acc : acc * 0.5f;
  const float m = sqrtf(mean);
  return m * m;
}
// compare_audio.py:7-10 / layer2_analyze_eq.py:71:
//   power_mono = sqrt(0.5 * (L**2 + R**2) + EPS)
__device__ __forceinline__ float power_mono(const float* __restrict__ x, int64_t p, float sc) {
  const float2 u = reinterpret_cast<const float2*>(x)[p];
  const float l = u.x * sc, r = u.y * sc;
  const float s = l * l + r * r;
  return sqrtf(0.5f * s + kEps);
}

// ---------------------------------------------------------------------------
// per-frame r (numpy pairwise mean, restated exactly)
// ---------------------------------------------------------------------------
template <int MODE, int CH>  // MODE: TOMATIS_AN_LEVEL_CHMEAN / _POWER_MONO
__global__ __launch_bounds__(256) void k_an_frame_r(const float* __restrict__ x, int n_fft,
                                                    int hop, int n_frames, float sc,
                                                    float* __restrict__ r_out) {
  __shared__ float lv[4][kMaxTreeN / 128];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int f = blockIdx.x * 4 + w;
  const bool live = f < n_frames;  // wave-uniform
  const int64_t p0 = (int64_t)f * hop;
  const int nl = n_fft >> 7;
  const int b = lane >> 3, c = lane & 7;
  for (int g = 0; g < nl; g += 8) {
    const int L = g + b;
    float acc = 0.f;
    if (live && L < nl) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int64_t p = p0 + 128 * L + c + 8 * t;
        float m2;
        if constexpr (MODE == TOMATIS_AN_LEVEL_POWER_MONO) {
          const float m = power_mono(x, p, sc);
          m2 = m * m;
        } else {
          m2 = m2_chmean<CH>(x, p, sc);
        }
        acc = (t == 0) ? m2 : acc + m2;
      }
    }
    // numpy's 8-chain tree ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); IEEE add commutes
    acc = acc + __shfl_xor(acc, 1, 64);
    acc = acc + __shfl_xor(acc, 2, 64);
    acc = acc + __shfl_xor(acc, 4, 64);
    if (c == 0 && L < nl) lv[w][L] = acc;
  }
  __syncthreads();
  if (live && lane == 0) {
    float* t = lv[w];
    for (int width = nl; width > 1; width >>= 1)
      for (int i = 0; i < width / 2; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    r_out[f] = sqrtf(t[0] / (float)n_fft + kEps);
  }
}

// any frame length: numpy's pairwise tree from the host program (leaf >= 0
// pushes that leaf's sum, -1 adds the top two); leaves follow numpy's block rule
// (sequential below 8, else 8 accumulators + fixed tree + sequential remainder)
template <int MODE, int CH>
__device__ __forceinline__ float m2_at(const float* __restrict__ x, int64_t p, float sc) {
  if constexpr (MODE == TOMATIS_AN_LEVEL_POWER_MONO) {
    const float m = power_mono(x, p, sc);
    return m * m;
  } else if constexpr (MODE == kLevelPowerMean) {
    // find_main_segment.py:8: (l l + r r) * 0.5, every operation rounded (sc unused)
    const float l = x[2 * p], r = x[2 * p + 1];
    return __fmul_rn(__fadd_rn(__fmul_rn(l, l), __fmul_rn(r, r)), 0.5f);
  } else {
    return m2_chmean<CH>(x, p, sc);
  }
}

// MODE kLevelPowerMean writes the mean itself (np.mean(p), :9), the others r
template <int MODE, int CH>
__global__ __launch_bounds__(256) void k_an_frame_r_pw(const float* __restrict__ x, int n_fft,
                                                       int hop, float sc,
                                                       const int2* __restrict__ leaf, int n_leaf,
                                                       const int16_t* __restrict__ prog,
                                                       int n_prog, float* __restrict__ r_out) {
  __shared__ float ls[kPwMax];
  const int f = blockIdx.x;
  const int64_t p0 = (int64_t)f * hop;
  for (int l = threadIdx.x; l < n_leaf; l += blockDim.x) {
    const int2 lf = leaf[l];
    const int64_t q = p0 + lf.x;
    const int len = lf.y;
    float res;
    if (len < 8) {
      res = 0.f;
      for (int i = 0; i < len; ++i) res = res + m2_at<MODE, CH>(x, q + i, sc);
    } else {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = m2_at<MODE, CH>(x, q + j, sc);
      int i = 8;
      for (; i < len - (len % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + m2_at<MODE, CH>(x, q + i + j, sc);
      }
      res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; i < len; ++i) res = res + m2_at<MODE, CH>(x, q + i, sc);
    }
    ls[l] = res;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float stk[32];
    int sp = 0;
    for (int i = 0; i < n_prog; ++i) {
      const int op = prog[i];
      if (op >= 0) {
        stk[sp++] = ls[op];
      } else {
        const float b = stk[--sp];
        stk[sp - 1] = stk[sp - 1] + b;
      }
    }
    if constexpr (MODE == kLevelPowerMean) r_out[f] = __fdiv_rn(stk[0], (float)n_fft);
    else r_out[f] = sqrtf(stk[0] / (float)n_fft + kEps);
  }
}

// ---------------------------------------------------------------------------
// frame selection on r bit patterns (exact level predicates, dsp.gate_bits)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_an_select(const float* __restrict__ r, int n_frames,
                                                   uint32_t thr, uint4 exc, int n_exc,
                                                   int keep_above, const int8_t* __restrict__ cls,
                                                   int cls_want, uint8_t* __restrict__ mask,
                                                   int32_t* __restrict__ count) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (f < n_frames) {
    const float rv = r[f];
    const uint32_t b = __float_as_uint(rv);
    const uint32_t e[4] = {exc.x, exc.y, exc.z, exc.w};
    bool hit = false;
    for (int i = 0; i < n_exc; ++i) hit |= (b == e[i]);
    if (rv == rv) {
      // keep_above: level >= T  <=> (b >= thr) xor exc     (gate "on" form)
      // else:       level >  T  <=> !((b <= thr) xor exc)  (not the "off" form)
      keep = keep_above ? ((b >= thr) != hit) : !((b <= thr) != hit);
    }
    if (cls) keep = keep && (cls[f] == cls_want);
    mask[f] = keep ? 1 : 0;
  }
  const unsigned long long bal = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (int32_t)__popcll(bal));
}

using tlds::cadd;
using tlds::cmul;
using tlds::csub;
using tlds::lds_dft;

// ---------------------------------------------------------------------------
// spectra
// ---------------------------------------------------------------------------
struct SpecArgs {  // filled by name, then completed by spec_args (host side below)
  const float* x = nullptr;
  const float* y = nullptr;
  const float* win = nullptr;
  const float2* tw = nullptr;  // exp(-2 pi i t / M)
  const float2* bb = nullptr;  // Bluestein chirp b (n_fft), BLUE kernels only
  const float2* bh = nullptr;  // Bluestein kernel spectrum H (M)
  float* out = nullptr;
  int n_fft = 0, M = 0, hop = 0, n_frames = 0, n_bins = 0;
  float sc = 1.0f;
  int band[4] = {0, 0, 0, 0};  // bins [band0, band1) and [band2, band3)
};

template <int SIG>  // TOMATIS_AN_SIG_RAW (ch 1) / TOMATIS_AN_SIG_POWER_MONO (ch 2)
__device__ __forceinline__ float sig_at(const float* __restrict__ x, int64_t p, float sc) {
  if constexpr (SIG == TOMATIS_AN_SIG_POWER_MONO) return power_mono(x, p, sc);
  else return x[p] * sc;
}

// ---------------------------------------------------------------------------
// The frame front end: what every spectrum kernel does around its own
// arithmetic.  A kernel stages two real signals as a + ib (stage_pair),
// transforms (lds_dft), and walks the bins it owns (owned_bins), taking both
// spectra of a bin from split_pair; sums over bins go through block_sums.  The
// helpers fix every order a result depends on: a thread's bins ascending, the
// shuffle offsets 32 -> 1, the waves 0..3, float64 adds of float32 values.
// ---------------------------------------------------------------------------
template <int M>
constexpr int kMaxUB = (M / 2 + 1 + kT - 1) / kT;  // bins per thread (n/2+1 <= M/2+1)

// fn(u, k) for the bins k = t, t + kT, ... below n_bins; u counts them from 0
template <int M, typename F>
__device__ __forceinline__ void owned_bins(int n_bins, F&& fn) {
#pragma unroll
  for (int u = 0; u < kMaxUB<M>; ++u) {
    const int k = threadIdx.x + u * kT;
    // k < n_bins, with the uniform part of it on the scalar side
    if ((int)threadIdx.x < n_bins - u * kT) fn(u, k);
  }
}

__device__ __forceinline__ bool in_range(int k, int lo, int hi) { return k >= lo && k < hi; }
__device__ __forceinline__ float power(float2 z) { return z.x * z.x + z.y * z.y; }
// 10 log10(re^2 + im^2 + EPS), float32 (layer2_analyze_eq.py:78-79)
__device__ __forceinline__ float logpow_db(float2 z) { return 10.0f * log10f(power(z) + kEps); }

// DFT bin mirrored for the two-real-signals split: (n - k) mod n
__device__ __forceinline__ int mirror(int k, int n) { return k == 0 ? 0 : n - k; }

// bin k of both spectra of Z = dft(a + ib):
//   A = (Z[k] + conj Z[n-k]) / 2, B = (Z[k] - conj Z[n-k]) / 2i
struct BinPair {
  float2 a, b;
};
__device__ __forceinline__ BinPair split_pair(const float2* buf, int k, int n) {
  const float2 zk = buf[k], zm = buf[mirror(k, n)];
  return {make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y)),
          make_float2(0.5f * (zk.y + zm.y), -0.5f * (zk.x - zm.x))};
}

// Fixed-order block sums of J values per thread: a shuffle tree inside each wave,
// lane 0 writes red[wave][j], barrier; wave_total then adds waves 0..3 in order.
// No atomics: the same bits in every run.
template <int J, typename T>
__device__ __forceinline__ void block_sums(const T (&acc)[J], T (*red)[J]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    T v = acc[j];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) red[wv][j] = v;
  }
  __syncthreads();
}
template <int J, typename T>
__device__ __forceinline__ T wave_total(const T (*red)[J], int j) {
  T v = 0;
  for (int i = 0; i < kT / 64; ++i) v += red[i][j];
  return v;
}

// buf[i] = (a_of(i) * win[i], has_b ? b_of(i) * win[i] : 0) for i < n, then a
// barrier.  REAL64 also leaves in red the float64 sums of the windowed samples
// with signs +1 and (-1)^i, that is the two real-valued bins 0 and (n even)
// n / 2 of both signals: (a, bin 0), (a, n/2), (b, 0), (b, n/2).  A real bin
// passes through zero, where a logarithm turns the transform's rounding
// (relative to the frame's largest bin) into decibels, and a positive signal
// such as the power mono puts n / 2 some 50 dB under bin 0; kernels that take
// logarithms of such signals read these bins from real_bins instead.
template <bool REAL64, typename FA, typename FB>
__device__ __forceinline__ void stage_pair(float2* buf, double (*red)[4], int n,
                                           const float* __restrict__ win, FA&& a_of, FB&& b_of,
                                           bool has_b = true) {
  double re[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < n; i += kT) {
    const float w = win[i];
    const float a = a_of(i) * w;
    const float b = has_b ? b_of(i) * w : 0.f;
    buf[i] = make_float2(a, b);
    if constexpr (REAL64) {
      re[0] += (double)a;
      re[1] += (i & 1) ? -(double)a : (double)a;
      re[2] += (double)b;
      re[3] += (i & 1) ? -(double)b : (double)b;
    }
  }
  if constexpr (REAL64) block_sums(re, red);
  else __syncthreads();
}

// which real bin k is of a length-n transform: 0 (bin 0), 1 (bin n / 2), else -1
__device__ __forceinline__ int real_bin(int k, int n) { return k == 0 ? 0 : 2 * k == n ? 1 : -1; }
// stage_pair<true>'s real bin j of (a, b): the float64 sums, rounded once
__device__ __forceinline__ float2 real_bins(const double (*red)[4], int j) {
  return make_float2((float)wave_total(red, j), (float)wave_total(red, 2 + j));
}

// frames f0 and f0 + 1 of x packed as a + ib; past the last frame b = 0
template <bool REAL64, int SIG>
__device__ __forceinline__ void stage_frames(const SpecArgs& A, int n, int f0, bool has1,
                                             float2* buf, double (*red)[4]) {
  const int64_t p0 = (int64_t)f0 * A.hop, p1 = (int64_t)(f0 + 1) * A.hop;
  stage_pair<REAL64>(
      buf, red, n, A.win, [&](int i) { return sig_at<SIG>(A.x, p0 + i, A.sc); },
      [&](int i) { return sig_at<SIG>(A.x, p1 + i, A.sc); }, has1);
}

// A float64 mean over many frames: a workgroup owns per_slab consecutive items
// (a constant of the source: neither the device nor the grid changes a bit of
// the result) and walks them in order; a thread keeps one float64 accumulator
// per bin it owns (registers: the LDS holds the transform) and item(e, acc) adds
// item e's values.  The slab's sums go to work[slab][bin]; k_an_spec_mean_fold
// adds the slabs in ascending order.
template <int M, typename F>
__device__ __forceinline__ void slab_sums(int per_slab, int n_items, int n_bins,
                                          double* __restrict__ work, F&& item) {
  double acc[kMaxUB<M>];
#pragma unroll
  for (int u = 0; u < kMaxUB<M>; ++u) acc[u] = 0.0;
  const int e0 = blockIdx.x * per_slab, e1 = min(e0 + per_slab, n_items);
  for (int e = e0; e < e1; ++e) {
    item(e, acc);
    __syncthreads();  // the item's LDS is written again for the next one
  }
  double* o = work + (int64_t)blockIdx.x * n_bins;
  owned_bins<M>(n_bins, [&](int u, int k) { o[k] = acc[u]; });
}

// MAG / LOGPOW: workgroup per frame pair (2g, 2g+1)
template <int KIND, int SIG, int M, bool BLUE>
__global__ __launch_bounds__(kT) void k_an_spec_pair(SpecArgs A) {
  __shared__ float2 buf[M];
  const int f0 = blockIdx.x * 2;
  const bool has1 = f0 + 1 < A.n_frames;
  const int n = BLUE ? A.n_fft : M;  // constant for powers of two
  stage_frames<false, SIG>(A, n, f0, has1, buf, nullptr);
  lds_dft<M, BLUE>(buf, n, A.tw, A.bb, A.bh);
  float* o0 = A.out + (int64_t)f0 * A.n_bins;
  float* o1 = o0 + A.n_bins;
  owned_bins<M>(A.n_bins, [&](int, int k) {
    const BinPair z = split_pair(buf, k, n);
    if constexpr (KIND == TOMATIS_AN_MAG) {
      o0[k] = hypotf(z.a.x, z.a.y);
      if (has1) o1[k] = hypotf(z.b.x, z.b.y);
    } else {
      o0[k] = logpow_db(z.a);
      if (has1) o1[k] = logpow_db(z.b);
    }
  });
}

// Mean log-power spectrum (avg_spectrum_db, compare_to_baseline.py:105-122): the
// LOGPOW value of k_an_spec_pair, summed over frames in float64 instead of
// stored: slab_sums over kSlabPairs frame pairs, frame 2g added, then frame
// 2g + 1 where it exists; the two real bins from the float64 sums.
constexpr int kSlabPairs = 8;

struct MeanArgs {
  SpecArgs S;
  double* work;  // [slabs][n_bins]
};

template <int SIG, int M, bool BLUE>
__global__ __launch_bounds__(kT) void k_an_spec_mean(MeanArgs B) {
  __shared__ float2 buf[M];
  __shared__ double red[kT / 64][4];
  const SpecArgs& A = B.S;
  const int n = BLUE ? A.n_fft : M;  // constant for powers of two
  slab_sums<M>(kSlabPairs, (A.n_frames + 1) / 2, A.n_bins, B.work, [&](int g, auto& acc) {
    const int f0 = 2 * g;
    const bool has1 = f0 + 1 < A.n_frames;
    stage_frames<true, SIG>(A, n, f0, has1, buf, red);
    lds_dft<M, BLUE>(buf, n, A.tw, A.bb, A.bh);
    owned_bins<M>(A.n_bins, [&](int u, int k) {
      BinPair z = split_pair(buf, k, n);
      if (const int j = real_bin(k, n); j >= 0) {
        const float2 r = real_bins(red, j);
        z = {make_float2(r.x, 0.f), make_float2(r.y, 0.f)};
      }
      acc[u] += (double)logpow_db(z.a);
      // an odd count's last frame has no partner: nothing is added for it
      if (has1) acc[u] += (double)logpow_db(z.b);
    });
  });
}

// out[k] = (work[0][k] + work[1][k] + ...) / max(n_frames, 1): one chain per bin
// in ascending slab order, its loads a batch ahead as in k_an_frame_mean
__global__ __launch_bounds__(64) void k_an_spec_mean_fold(const double* __restrict__ work,
                                                           int n_slabs, int n_bins, int n_frames,
                                                           double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_bins) return;
  constexpr int kB = 16;
  double v[kB];
  double s = 0.0;
  for (int s0 = 0; s0 < n_slabs; s0 += kB) {
#pragma unroll
    for (int u = 0; u < kB; ++u) v[u] = work[(int64_t)min(s0 + u, n_slabs - 1) * n_bins + k];
#pragma unroll
    for (int u = 0; u < kB; ++u)
      if (s0 + u < n_slabs) s += v[u];
  }
  out[k] = s / (double)max(n_frames, 1);
}

// BAND (stft_band_tilt, calibrate_to_baseline_v2.py:17-31): per frame of the
// pair the float32 power re^2 + im^2 of rfft(win * power_mono) summed over two
// bin ranges, each on its own (the reference takes any two masks: the ranges
// may overlap or be empty); workgroup per frame pair as k_an_spec_pair.
template <int M, bool BLUE>
__global__ __launch_bounds__(kT) void k_an_band_pair(SpecArgs A) {
  __shared__ float2 buf[M];
  __shared__ float red[kT / 64][4];
  const int n = BLUE ? A.n_fft : M;  // constant for powers of two
  const int f0 = blockIdx.x * 2;
  const bool has1 = f0 + 1 < A.n_frames;
  stage_frames<false, TOMATIS_AN_SIG_POWER_MONO>(A, n, f0, has1, buf, nullptr);
  lds_dft<M, BLUE>(buf, n, A.tw, A.bb, A.bh);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // (frame a, band lo), (a, hi), (b, lo), (b, hi)
  owned_bins<M>(A.n_bins, [&](int, int k) {
    const bool lo = in_range(k, A.band[0], A.band[1]), hi = in_range(k, A.band[2], A.band[3]);
    if (!lo && !hi) return;
    const BinPair z = split_pair(buf, k, n);
    const float pa = power(z.a), pb = power(z.b);
    if (lo) {
      acc[0] += pa;
      acc[2] += pb;
    }
    if (hi) {
      acc[1] += pa;
      acc[3] += pb;
    }
  });
  block_sums(acc, red);
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    const float v = wave_total(red, j);
    if (j < 2 || has1) A.out[(int64_t)f0 * 2 + j] = v;  // out[F][2]: j >= 2 is frame f0 + 1
  }
}


// Gate-calibration grid (calibrate_to_baseline_v2.py:84-109 simulate_state,
// :241-265 the search): one lane per candidate runs the standard automaton
// (hysteresis + up-delay on frame starts) over the fitted frames and counts
// mismatches against the target states and state switches.  Levels are
// float32 and compared with the float32 thresholds exactly as numpy compares
// an np.float32 level with a Python float (NEP 50: in float32).
__global__ __launch_bounds__(256) void k_cal_gate_grid(const float* __restrict__ levels,
                                                       int n_fit,
                                                       const int64_t* __restrict__ starts,
                                                       const int32_t* __restrict__ target,
                                                       const TomatisGateCand* __restrict__ cands,
                                                       int n_cand, int32_t* __restrict__ out,
                                                       uint8_t* __restrict__ states) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cand) return;  // no barriers below
  const TomatisGateCand C = cands[c];
  const float* lv = levels + (int64_t)C.level_row * n_fit;
  int state = 1, prev = 1, mism = 0, sw = 0;
  bool pend = false;
  int64_t pending = 0;
  for (int i = 0; i < n_fit; ++i) {
    const float l = lv[i];
    const int64_t st = starts[i];
    if (state == 1) {
      if (l >= C.t_on) {
        if (!pend) {
          pend = true;
          pending = st + C.up_delay;
        }
      } else {
        pend = false;
      }
      if (pend && st >= pending) {
        state = 2;
        pend = false;
      }
    } else if (l <= C.t_off) {
      state = 1;
      pend = false;
    }
    if (states) states[(int64_t)c * n_fit + i] = (uint8_t)state;
    if (target) mism += state != target[i];
    sw += (i > 0) & (state != prev);
    prev = state;
  }
  out[2 * c] = mism;
  out[2 * c + 1] = sw;
}

// Input/output pairs, one workgroup per frame and one transform of x_c + i y_c
// per channel: TOMATIS_AN_RATIO (compute_conditional_spectrum) and the per-frame
// work of sections C and D of the acceptance validator v2
// (verify_tomatis_15db_v2.py).
//   ROWS  (:307-354)  ratio[k] = mean_c|Y_c| / max(mean_c|X_c|, 1e-10).  With
//     ANCHOR, g = mean(ratio[a0:a1]) and the row is stored as ratio / g when g > 0,
//     else as it is (the reference's np.mean of an empty slice is NaN, and
//     NaN > 0 is false).  The host leaves ANCHOR out where the range is empty:
//     the row is stored as it is without the reduction and its barrier.
//   BANDS (:451-470)  P_x[k] = mean_c |X_c[k]|^2 (re^2 + im^2 in float32), P_y
//     likewise; bands[f] = (sum P_x[lo), sum P_x[hi), sum P_y[lo), sum P_y[hi)),
//     the two ranges independent and possibly empty as in k_an_band_pair.
// The row stays in registers after the split; the anchor sum and the four band
// sums go through one block_sums: the same bits in every run, and the same bits
// whether a launch forms the rows, the bands or both.
struct VerArgs {
  SpecArgs S;    // out = rows [F][n_bins] (ROWS), band = lo0, lo1, hi0, hi1 (BANDS)
  float* bands;  // [F][4]
  int a0, a1;    // anchor bins [a0, a1)
};

template <int CH, int M, bool BLUE, bool ROWS, bool BANDS, bool ANCHOR>
__global__ __launch_bounds__(kT) void k_an_verify(VerArgs V) {
  static_assert((ROWS || BANDS) && (ROWS || !ANCHOR), "ANCHOR scales the rows");
  __shared__ float2 buf[M];
  __shared__ float red[kT / 64][5];
  const SpecArgs& A = V.S;
  constexpr int kUR = ROWS ? kMaxUB<M> : 1, kUP = BANDS ? kMaxUB<M> : 1;
  const int f = blockIdx.x;
  const int n = BLUE ? A.n_fft : M;  // constant for powers of two
  const int64_t p0 = (int64_t)f * A.hop;
  float ax[kUR], ay[kUR], px[kUP], py[kUP];
#pragma unroll
  for (int u = 0; u < kUR; ++u) ax[u] = ay[u] = 0.f;
#pragma unroll
  for (int u = 0; u < kUP; ++u) px[u] = py[u] = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    stage_pair<false>(
        buf, nullptr, n, A.win, [&](int i) { return A.x[(p0 + i) * CH + c]; },
        [&](int i) { return A.y[(p0 + i) * CH + c]; });
    lds_dft<M, BLUE>(buf, n, A.tw, A.bb, A.bh);
    owned_bins<M>(A.n_bins, [&](int u, int k) {
      const BinPair z = split_pair(buf, k, n);
      if constexpr (ROWS) {
        ax[u] = ax[u] + hypotf(z.a.x, z.a.y);  // X += |rfft(x_c * win)|
        ay[u] = ay[u] + hypotf(z.b.x, z.b.y);
      }
      if constexpr (BANDS) {
        px[u] = px[u] + power(z.a);  // X += |rfft(x_c * win)|**2
        py[u] = py[u] + power(z.b);
      }
    });
    __syncthreads();  // buf reused by the next channel
  }
  float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};  // anchor, (x, lo), (x, hi), (y, lo), (y, hi)
  owned_bins<M>(A.n_bins, [&](int u, int k) {
    if constexpr (ROWS) {
      float X = (CH == 1) ? ax[u] : ax[u] * 0.5f;  // X /= ch
      const float Y = (CH == 1) ? ay[u] : ay[u] * 0.5f;
      X = fmaxf(X, 1e-10f);                        // np.maximum(X, 1e-10)
      ax[u] = Y / X;
      if constexpr (ANCHOR) {
        if (in_range(k, V.a0, V.a1)) acc[0] = acc[0] + ax[u];
      }
    }
    if constexpr (BANDS) {
      const float PX = (CH == 1) ? px[u] : px[u] * 0.5f;
      const float PY = (CH == 1) ? py[u] : py[u] * 0.5f;
      if (in_range(k, A.band[0], A.band[1])) {
        acc[1] = acc[1] + PX;
        acc[3] = acc[3] + PY;
      }
      if (in_range(k, A.band[2], A.band[3])) {
        acc[2] = acc[2] + PX;
        acc[4] = acc[4] + PY;
      }
    }
  });
  if constexpr (ANCHOR || BANDS) block_sums(acc, red);
  if constexpr (BANDS) {
    if (threadIdx.x < 4) V.bands[(int64_t)f * 4 + threadIdx.x] = wave_total(red, 1 + threadIdx.x);
  }
  if constexpr (ROWS) {
    float g = 0.f;
    if constexpr (ANCHOR) g = wave_total(red, 0) / (float)(V.a1 - V.a0);
    const bool scale = ANCHOR && g > 0.f;  // anchor_gain > 0 (NaN: false)
    float* o = A.out + (int64_t)f * A.n_bins;
    owned_bins<M>(A.n_bins, [&](int u, int k) { o[k] = scale ? ax[u] / g : ax[u]; });
  }
}

// ---------------------------------------------------------------------------
// Parameter recovery (reverse_engineer_params.py:118-143,
// verify_tilt_amplitude.py:74-92): per frame and bin
//   d[k] = 20 log10(|B_k| + EPS) - 20 log10(|A_k| + EPS),   float32,
// A = rfft(win * power_mono(x)), B = rfft(win * power_mono(y)).  Both spectra
// come from one transform of a + ib, the magnitudes are hypotf as
// TOMATIS_AN_MAG's; both signals are power monos, so the two real bins are
// stage_pair's float64 sums.
//
// pair_diff stages frame f, transforms, splits and hands every bin the thread
// owns to use(u, k, d).  It leaves buf and red in use: a caller that stages
// another frame puts a barrier in between.
// ---------------------------------------------------------------------------
template <int M, bool BLUE, typename U>
__device__ __forceinline__ void pair_diff(const SpecArgs& A, int f, float2* buf,
                                          double (*red)[4], U&& use) {
  const int n = BLUE ? A.n_fft : M;  // constant for powers of two
  const int64_t p0 = (int64_t)f * A.hop;
  stage_pair<true>(
      buf, red, n, A.win, [&](int i) { return power_mono(A.x, p0 + i, 1.0f); },
      [&](int i) { return power_mono(A.y, p0 + i, 1.0f); });
  lds_dft<M, BLUE>(buf, n, A.tw, A.bb, A.bh);
  owned_bins<M>(A.n_bins, [&](int u, int k) {
    float ma, mb;
    if (const int j = real_bin(k, n); j >= 0) {
      const float2 r = real_bins(red, j);
      ma = fabsf(r.x);
      mb = fabsf(r.y);
    } else {
      const BinPair z = split_pair(buf, k, n);
      ma = hypotf(z.a.x, z.a.y);
      mb = hypotf(z.b.x, z.b.y);
    }
    use(u, k, 20.0f * log10f(mb + kEps) - 20.0f * log10f(ma + kEps));
  });
}

// compute_tilt_index's two band means of d (reverse_engineer_params.py:62-76),
// one workgroup per frame: means[f] = (mean d[lo0:lo1], mean d[hi0:hi1]) as
// float64, each a float64 block_sums of the float32 values over the bin count;
// an empty range gives 0 / 0 = NaN, numpy's mean of an empty slice.  The row is
// stored where rows is given; the sums do not depend on it.
struct TiltArgs {
  SpecArgs S;     // out = rows [F][n_bins] or null, band = lo0, lo1, hi0, hi1
  double* means;  // [F][2]
};

template <int M, bool BLUE>
__global__ __launch_bounds__(kT) void k_an_pair_tilt(TiltArgs T) {
  __shared__ float2 buf[M];
  __shared__ double red[kT / 64][4];
  __shared__ double sums[kT / 64][2];
  const SpecArgs& A = T.S;
  const int f = blockIdx.x;
  float* o = A.out ? A.out + (int64_t)f * A.n_bins : nullptr;
  double acc[2] = {0.0, 0.0};
  pair_diff<M, BLUE>(A, f, buf, red, [&](int, int k, float d) {
    if (o) o[k] = d;
    if (in_range(k, A.band[0], A.band[1])) acc[0] += (double)d;
    if (in_range(k, A.band[2], A.band[3])) acc[1] += (double)d;
  });
  block_sums(acc, sums);
  if (threadIdx.x < 2) {
    const int j = threadIdx.x;
    T.means[(int64_t)f * 2 + j] =
        wave_total(sums, j) / (double)(A.band[2 * j + 1] - A.band[2 * j]);
  }
}

// np.mean(diffs, axis=0) over a list of frames (verify_tilt_amplitude.py:98-99),
// in float64: slab_sums over kSlabFrames consecutive list entries, then
// k_an_spec_mean_fold divides by the list's length.  frames == null: the list
// is 0, 1, 2, ...
constexpr int kSlabFrames = 16;

struct DiffMeanArgs {
  SpecArgs S;
  const int32_t* frames;  // [n_sel] or null
  int n_sel;
  double* work;  // [slabs][n_bins]
};

template <int M, bool BLUE>
__global__ __launch_bounds__(kT) void k_an_pair_diff_mean(DiffMeanArgs D) {
  __shared__ float2 buf[M];
  __shared__ double red[kT / 64][4];
  const SpecArgs& A = D.S;
  slab_sums<M>(kSlabFrames, D.n_sel, A.n_bins, D.work, [&](int e, auto& acc) {
    const int f = D.frames ? D.frames[e] : e;
    pair_diff<M, BLUE>(A, f, buf, red, [&](int u, int, float d) { acc[u] += (double)d; });
  });
}


__global__ void k_an_fill_f64(double* __restrict__ out, int n, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

// ---------------------------------------------------------------------------
// float64 sum of a float32 buffer (np.mean(y) of check_engineering,
// verify_tomatis_15db_v2.py:90): kSumGroups partial sums over a fixed grid (a
// constant of the source, not of the device), element i in group (i / kT) mod
// kSumGroups, each folded by a shuffle tree and the four waves in order; then the
// partial sums in index order.  The same bits in every run.
// ---------------------------------------------------------------------------
constexpr int kSumGroups = 1024;

__global__ __launch_bounds__(kT) void k_an_sum_part(const float* __restrict__ x, int64_t n,
                                                    double* __restrict__ part) {
  __shared__ double sm[kT / 64];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)kSumGroups * kT)
    s += (double)x[i];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < kT / 64; ++i) t += sm[i];
    part[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void k_an_sum_fold(const double* __restrict__ part,
                                                     double* __restrict__ out) {
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < kSumGroups; ++i) s += part[i];
    out[0] = s;
  }
}

// ---------------------------------------------------------------------------
// reductions over frames
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_an_frame_mean(const float* __restrict__ spec,
                                                       int n_frames, int n_bins,
                                                       float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_bins) return;
  // The sum is one dependent chain per bin (numpy's order); its loads are not:
  // batches of kB frames are loaded one batch ahead so the chain never waits on
  // HBM latency (indices clamped: the last batch re-reads valid rows).
  constexpr int kB = 32;
  float cur[kB], nxt[kB];
  const int last = n_frames - 1;
#pragma unroll
  for (int u = 0; u < kB; ++u) cur[u] = spec[(int64_t)min(u, last) * n_bins + k];
  float s = 0.f;  // numpy's add.reduce starts from the identity (-0 sums to +0)
  for (int f0 = 0; f0 < n_frames; f0 += kB) {
#pragma unroll
    for (int u = 0; u < kB; ++u) nxt[u] = spec[(int64_t)min(f0 + kB + u, last) * n_bins + k];
#pragma unroll
    for (int u = 0; u < kB; ++u)
      if (f0 + u < n_frames) s = s + cur[u];
#pragma unroll
    for (int u = 0; u < kB; ++u) cur[u] = nxt[u];
  }
  out[k] = s / (float)n_frames;
}

__device__ __forceinline__ uint32_t fkey(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fval(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

struct MedState {  // per bin
  uint32_t prefix;  // key bits fixed so far
  uint32_t rank;    // rank still to find inside the current prefix
  uint32_t cnt;     // elements equal to the selected key (after the last pass)
  uint32_t key2;    // min key > prefix (even counts)
};

__global__ void k_an_med_init(MedState* __restrict__ st, int n_bins, uint32_t k1) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < n_bins) st[b] = MedState{0u, k1, 0u, 0xFFFFFFFFu};
}

// pass p (0..3): histogram of digit (key >> (24 - 8p)) & 255 over selected
// frames whose higher digits equal the prefix; p == 4: min key > prefix
__global__ __launch_bounds__(256) void k_an_med_hist(const float* __restrict__ spec,
                                                     int n_frames, int n_bins,
                                                     const uint8_t* __restrict__ mask,
                                                     const MedState* __restrict__ st,
                                                     uint32_t* __restrict__ ghist, int pass,
                                                     int per_split) {
  __shared__ uint32_t h[256 * 64];  // [digit][lane]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + lane;
  const int fa = blockIdx.y * per_split;
  const int fb = min(n_frames, fa + per_split);
  const bool vb = b < n_bins;
  const uint32_t prefix = vb ? st[b].prefix : 0u;
  const int shift = 24 - 8 * pass;
  if (pass < 4) {
    for (int i = threadIdx.x; i < 256 * 64; i += 256) h[i] = 0u;
    __syncthreads();
    const uint32_t hm = pass == 0 ? 0u : (0xFFFFFFFFu << (32 - 8 * pass));
    if (vb) {
      for (int f = fa + w; f < fb; f += 4) {
        if (mask && !mask[f]) continue;
        const uint32_t key = fkey(spec[(int64_t)f * n_bins + b]);
        if ((key & hm) == prefix) atomicAdd(&h[((key >> shift) & 255u) * 64 + lane], 1u);
      }
    }
    __syncthreads();
    if (vb) {
      for (int d = w; d < 256; d += 4) {
        const uint32_t c = h[d * 64 + lane];
        if (c) atomicAdd(&ghist[(int64_t)b * 256 + d], c);
      }
    }
  } else {
    uint32_t m = 0xFFFFFFFFu;
    if (vb) {
      for (int f = fa + w; f < fb; f += 4) {
        if (mask && !mask[f]) continue;
        const uint32_t key = fkey(spec[(int64_t)f * n_bins + b]);
        if (key > prefix) m = min(m, key);
      }
    }
    h[w * 64 + lane] = m;
    __syncthreads();
    if (w == 0 && vb) {
      m = min(min(h[lane], h[64 + lane]), min(h[128 + lane], h[192 + lane]));
      if (m != 0xFFFFFFFFu) atomicMin(&ghist[(int64_t)b * 256], m);
    }
  }
}

__global__ void k_an_med_pick(MedState* __restrict__ st, const uint32_t* __restrict__ ghist,
                              int n_bins, int pass) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_bins) return;
  MedState s = st[b];
  const uint32_t* hh = ghist + (int64_t)b * 256;
  if (pass < 4) {
    uint32_t r = s.rank, d = 0, c = 0;
    for (; d < 256; ++d) {
      c = hh[d];
      if (r < c) break;
      r -= c;
    }
    s.prefix |= (d & 255u) << (24 - 8 * pass);
    s.rank = r;
    s.cnt = c;
  } else {
    s.key2 = hh[0];
  }
  st[b] = s;
}

__global__ void k_an_med_final(const MedState* __restrict__ st, int n_bins, int even,
                               float* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_bins) return;
  const MedState s = st[b];
  const float v1 = fval(s.prefix);
  // np.median = mean of the middle element(s): add.reduce from the identity 0
  if (!even) {
    out[b] = 0.f + v1;
    return;
  }
  // the upper middle equals v1 if another copy of v1 follows it
  const float v2 = (s.rank + 1 < s.cnt) ? v1 : fval(s.key2);
  out[b] = ((0.f + v1) + v2) / 2.0f;
}

// F = the frames that lie inside n samples, 0 where there is none (the caller
// then has nothing to do and returns TOMATIS_OK)
int frame_count(int64_t n, int n_fft, int hop, int* F) {
  *F = 0;
  if (n < n_fft) return TOMATIS_OK;
  const int64_t f = 1 + (n - n_fft) / hop;
  if (f > INT32_MAX) return TOMATIS_E_UNSUPPORTED;
  *F = (int)f;
  return TOMATIS_OK;
}

bool range_ok(int nb, int lo, int hi) { return lo >= 0 && hi >= lo && hi <= nb; }
bool bands_ok(int nb, int lo0, int lo1, int hi0, int hi1) {
  return range_ok(nb, lo0, lo1) && range_ok(nb, hi0, hi1);
}

// Completes a SpecArgs whose signals, window, output, scale and bands the caller
// has set by name: the framing, M, the twiddles of M and, for a length that is
// no power of two, the Bluestein tables.
int spec_args(int n_fft, int hop, int F, hipStream_t s, SpecArgs* A) {
  A->n_fft = n_fft;
  A->hop = hop;
  A->n_frames = F;
  A->n_bins = n_fft / 2 + 1;
  A->M = dft_m(n_fft);
  if (A->M == 0) return TOMATIS_E_UNSUPPORTED;
  int rc = twiddles(A->M, s, &A->tw);
  if (rc != TOMATIS_OK || A->M == n_fft) return rc;
  Chirp c;
  if ((rc = chirp_tables(n_fft, A->M, &c)) != TOMATIS_OK) return rc;
  A->bb = c.b;
  A->bh = c.h;
  return TOMATIS_OK;
}

void set_bands(SpecArgs* A, int lo0, int lo1, int hi0, int hi1) {
  A->band[0] = lo0;
  A->band[1] = lo1;
  A->band[2] = hi0;
  A->band[3] = hi1;
}


// calls f(integral_constant<M>, bool_constant<BLUE>) for the args' FFT size
// (M = 16 .. 16384; Bluestein sizes start at M = 32 since n_fft >= 16)
template <int M, typename L>
void launch_m(bool blue, L& f) {
  if constexpr (M >= 32) {
    if (blue) {
      f(std::integral_constant<int, M>{}, std::true_type{});
      return;
    }
  }
  f(std::integral_constant<int, M>{}, std::false_type{});
}

template <typename L>
int dispatch_m(const SpecArgs& A, L&& f) {
  const bool blue = A.M != A.n_fft;
  switch (A.M) {
    case 16: launch_m<16>(blue, f); break;
    case 32: launch_m<32>(blue, f); break;
    case 64: launch_m<64>(blue, f); break;
    case 128: launch_m<128>(blue, f); break;
    case 256: launch_m<256>(blue, f); break;
    case 512: launch_m<512>(blue, f); break;
    case 1024: launch_m<1024>(blue, f); break;
    case 2048: launch_m<2048>(blue, f); break;
    case 4096: launch_m<4096>(blue, f); break;
    case 8192: launch_m<8192>(blue, f); break;
    case 16384: launch_m<16384>(blue, f); break;
    default: return TOMATIS_E_UNSUPPORTED;
  }
  return an_launch();
}

template <int V>
constexpr std::integral_constant<int, V> ic{};

// calls f(integral_constant<MODE>, integral_constant<CH>) for a validated level
// mode and channel count (k_an_frame_r and k_an_frame_r_pw)
template <typename L>
void dispatch_level(int level_mode, int ch, L&& f) {
  if (level_mode == TOMATIS_AN_LEVEL_POWER_MONO) f(ic<TOMATIS_AN_LEVEL_POWER_MONO>, ic<2>);
  else if (ch == 1) f(ic<TOMATIS_AN_LEVEL_CHMEAN>, ic<1>);
  else f(ic<TOMATIS_AN_LEVEL_CHMEAN>, ic<2>);
}

// calls f(integral_constant<CH>, ROWS, BANDS, ANCHOR as bool_constants) for
// k_an_verify: rows without an anchor, anchored rows, bands, or anchored rows
// and bands
template <int CH, typename L>
void verify_variant(bool rows, bool bands, bool anchor, L& f) {
  constexpr std::true_type T{};
  constexpr std::false_type N{};
  if (!bands) anchor ? f(ic<CH>, T, N, T) : f(ic<CH>, T, N, N);
  else if (!rows) f(ic<CH>, N, T, N);
  else f(ic<CH>, T, T, T);
}
template <typename L>
void dispatch_verify(int ch, bool rows, bool bands, bool anchor, L&& f) {
  if (ch == 1) verify_variant<1>(rows, bands, anchor, f);
  else verify_variant<2>(rows, bands, anchor, f);
}

// one launch of k_an_verify over F frames of the pair (V.S.x, V.S.y): the rows
// where V.S.out is given, the bands where V.bands is; an empty anchor leaves the
// rows as they are (TOMATIS_AN_RATIO)
int launch_verify(VerArgs& V, int ch, int n_fft, int hop, int F, hipStream_t s) {
  const int rc = spec_args(n_fft, hop, F, s, &V.S);
  if (rc != TOMATIS_OK) return rc;
  return dispatch_m(V.S, [&](auto m, auto b) {
    dispatch_verify(ch, V.S.out != nullptr, V.bands != nullptr, V.a1 > V.a0, [&](auto c, auto r, auto bd, auto an) {
      hipLaunchKernelGGL((k_an_verify<decltype(c)::value, decltype(m)::value, decltype(b)::value,
                                      decltype(r)::value, decltype(bd)::value,
                                      decltype(an)::value>),
                         dim3((unsigned)F), dim3(kT), 0, s, V);
    });
  });
}

// the checks of the three pair entry points
int an_verify(const float* x, const float* y, int64_t n, int32_t ch, int32_t n_fft, int32_t hop,
              int32_t a0, int32_t a1, int32_t lo0, int32_t lo1, int32_t hi0, int32_t hi1,
              const float* win, float* rows, float* bands, void* hs) {
  if (!x || !y || !win || (!rows && !bands) || hop < 1 || ch < 1 || n_fft < 1 || n < 0)
    return TOMATIS_E_ARG;
  if (ch != 1 && ch != 2) return TOMATIS_E_UNSUPPORTED;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  const int nb = n_fft / 2 + 1;
  if (!range_ok(nb, a0, a1) || !bands_ok(nb, lo0, lo1, hi0, hi1)) return TOMATIS_E_ARG;
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  VerArgs V{{}, bands, a0, a1};
  V.S.x = x;
  V.S.y = y;
  V.S.win = win;
  V.S.out = rows;
  set_bands(&V.S, lo0, lo1, hi0, hi1);
  return launch_verify(V, ch, n_fft, hop, F, (hipStream_t)hs);
}

}  // namespace

extern "C" {

int tomatis_an_frame_r(const float* x, int64_t n, int32_t ch, int32_t n_fft, int32_t hop,
                       int32_t level_mode, float scale, float* r_out, void* hs) {
  if (!x || !r_out || hop < 1 || ch < 1 || n_fft < 1) return TOMATIS_E_ARG;
  if (n_fft > kMaxM) return TOMATIS_E_UNSUPPORTED;
  if (level_mode == TOMATIS_AN_LEVEL_POWER_MONO) {
    if (ch != 2) return TOMATIS_E_ARG;
  } else if (level_mode == TOMATIS_AN_LEVEL_CHMEAN) {
    if (ch != 1 && ch != 2) return TOMATIS_E_UNSUPPORTED;
  } else {
    return TOMATIS_E_ARG;
  }
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  hipStream_t s = (hipStream_t)hs;
  if (is_pow2(n_fft) && n_fft >= 256 && n_fft <= kMaxTreeN) {
    // perfect tree over 128-sample leaves, four frames per workgroup
    dispatch_level(level_mode, ch, [&](auto mode, auto c) {
      hipLaunchKernelGGL((k_an_frame_r<decltype(mode)::value, decltype(c)::value>),
                         dim3((unsigned)((F + 3LL) / 4)), dim3(256), 0, s, x, n_fft, hop, F, scale,
                         r_out);
    });
    return an_launch();
  }
  PwProg q;
  if ((rc = pw_program(n_fft, &q)) != TOMATIS_OK) return rc;
  dispatch_level(level_mode, ch, [&](auto mode, auto c) {
    hipLaunchKernelGGL((k_an_frame_r_pw<decltype(mode)::value, decltype(c)::value>),
                       dim3((unsigned)F), dim3(256), 0, s, x, n_fft, hop, scale, q.leaf, q.n_leaf,
                       q.prog, q.n_prog, r_out);
  });
  return an_launch();
}


int tomatis_an_frame_power_mean(const float* x, int64_t n, int32_t win, int32_t hop, float* out,
                                void* hs) {
  if (!x || !out || n < 0 || win < 1 || hop < 1) return TOMATIS_E_ARG;
  if (win > kMaxMeanWin) return TOMATIS_E_UNSUPPORTED;
  int F;
  int rc = frame_count(n, win, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  PwProg q;
  if ((rc = pw_program(win, &q)) != TOMATIS_OK) return rc;
  hipLaunchKernelGGL((k_an_frame_r_pw<kLevelPowerMean, 2>), dim3((unsigned)F), dim3(256), 0,
                     (hipStream_t)hs, x, win, hop, 1.0f, q.leaf, q.n_leaf, q.prog, q.n_prog, out);
  return an_launch();
}

int tomatis_an_select(const float* r, int32_t n_frames, uint32_t thr_bits,
                      const uint32_t* exc_host, int32_t n_exc, int32_t keep_above,
                      const int8_t* cls, int32_t cls_want, uint8_t* mask, int32_t* count,
                      void* hs) {
  if (!r || !mask || !count || n_frames < 0 || n_exc < 0 || n_exc > 4 || (n_exc && !exc_host))
    return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  int rc = an_fail(hipMemsetAsync(count, 0, sizeof(int32_t), s));
  if (rc != TOMATIS_OK || n_frames == 0) return rc;
  uint32_t e[4] = {0u, 0u, 0u, 0u};
  for (int i = 0; i < n_exc; ++i) e[i] = exc_host[i];
  hipLaunchKernelGGL(k_an_select, dim3((n_frames + 255) / 256), dim3(256), 0, s, r, n_frames,
                     thr_bits, make_uint4(e[0], e[1], e[2], e[3]), n_exc, keep_above, cls,
                     cls_want, mask, count);
  return an_launch();
}

int tomatis_an_spectra(const float* x, const float* y, int64_t n, int32_t ch, int32_t n_fft,
                       int32_t hop, int32_t kind, int32_t sig_mode, float scale,
                       const float* win, float* out, void* hs) {
  if (!x || !win || !out || hop < 1 || ch < 1 || n_fft < 1) return TOMATIS_E_ARG;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  if (kind == TOMATIS_AN_RATIO) {
    if (!y) return TOMATIS_E_ARG;
    if (ch != 1 && ch != 2) return TOMATIS_E_UNSUPPORTED;
  } else if (kind == TOMATIS_AN_MAG || kind == TOMATIS_AN_LOGPOW) {
    if (sig_mode == TOMATIS_AN_SIG_RAW) {
      if (ch != 1) return TOMATIS_E_ARG;
    } else if (sig_mode == TOMATIS_AN_SIG_POWER_MONO) {
      if (ch != 2) return TOMATIS_E_ARG;
    } else {
      return TOMATIS_E_ARG;
    }
  } else {
    return TOMATIS_E_ARG;
  }
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  hipStream_t s = (hipStream_t)hs;
  SpecArgs A;
  A.x = x;
  A.y = y;
  A.win = win;
  A.out = out;
  A.sc = scale;
  if (kind == TOMATIS_AN_RATIO) {  // the verify rows with an empty anchor (scale unused)
    VerArgs V{A, nullptr, 0, 0};
    return launch_verify(V, ch, n_fft, hop, F, s);
  }
  if ((rc = spec_args(n_fft, hop, F, s, &A)) != TOMATIS_OK) return rc;
  const dim3 g((unsigned)((F + 1LL) / 2));
  const bool raw = sig_mode == TOMATIS_AN_SIG_RAW;
  return dispatch_m(A, [&](auto m, auto b) {
    constexpr int MM = decltype(m)::value;
    constexpr bool BL = decltype(b)::value;
    constexpr int MAG = TOMATIS_AN_MAG, LOGP = TOMATIS_AN_LOGPOW;
    constexpr int RAW = TOMATIS_AN_SIG_RAW, PM = TOMATIS_AN_SIG_POWER_MONO;
    if (kind == MAG && raw) hipLaunchKernelGGL((k_an_spec_pair<MAG, RAW, MM, BL>), g, dim3(kT), 0, s, A);
    else if (kind == MAG) hipLaunchKernelGGL((k_an_spec_pair<MAG, PM, MM, BL>), g, dim3(kT), 0, s, A);
    else if (raw) hipLaunchKernelGGL((k_an_spec_pair<LOGP, RAW, MM, BL>), g, dim3(kT), 0, s, A);
    else hipLaunchKernelGGL((k_an_spec_pair<LOGP, PM, MM, BL>), g, dim3(kT), 0, s, A);
  });
}

int tomatis_an_band_energy(const float* x, int64_t n, int32_t n_fft, int32_t hop,
                           int32_t lo0, int32_t lo1, int32_t hi0, int32_t hi1,
                           const float* win, float* out, void* hs) {
  if (!x || !win || !out || hop < 1 || n_fft < 1) return TOMATIS_E_ARG;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  if (!bands_ok(n_fft / 2 + 1, lo0, lo1, hi0, hi1)) return TOMATIS_E_ARG;
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  hipStream_t s = (hipStream_t)hs;
  SpecArgs A;
  A.x = x;
  A.win = win;
  A.out = out;
  set_bands(&A, lo0, lo1, hi0, hi1);
  if ((rc = spec_args(n_fft, hop, F, s, &A)) != TOMATIS_OK) return rc;
  return dispatch_m(A, [&](auto m, auto b) {
    hipLaunchKernelGGL((k_an_band_pair<decltype(m)::value, decltype(b)::value>),
                       dim3((unsigned)((F + 1LL) / 2)), dim3(kT), 0, s, A);
  });
}

int tomatis_an_anchored_ratio(const float* x, const float* y, int64_t n, int32_t ch,
                              int32_t n_fft, int32_t hop, int32_t a0, int32_t a1,
                              const float* win, float* rows, void* hs) {
  if (!rows) return TOMATIS_E_ARG;
  return an_verify(x, y, n, ch, n_fft, hop, a0, a1, 0, 0, 0, 0, win, rows, nullptr, hs);
}

int tomatis_an_pair_band_energy(const float* x, const float* y, int64_t n, int32_t ch,
                                int32_t n_fft, int32_t hop, int32_t lo0, int32_t lo1,
                                int32_t hi0, int32_t hi1, const float* win, float* bands,
                                void* hs) {
  if (!bands) return TOMATIS_E_ARG;
  return an_verify(x, y, n, ch, n_fft, hop, 0, 0, lo0, lo1, hi0, hi1, win, nullptr, bands, hs);
}

int tomatis_an_verify_pair(const float* x, const float* y, int64_t n, int32_t ch, int32_t n_fft,
                           int32_t hop, int32_t a0, int32_t a1, int32_t lo0, int32_t lo1,
                           int32_t hi0, int32_t hi1, const float* win, float* rows, float* bands,
                           void* hs) {
  if (!rows || !bands) return TOMATIS_E_ARG;
  return an_verify(x, y, n, ch, n_fft, hop, a0, a1, lo0, lo1, hi0, hi1, win, rows, bands, hs);
}

int tomatis_sum_f64(const float* x, int64_t n, double* out, void* hs) {
  if (!x || !out || n < 0) return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  double* part = out + 1;
  hipLaunchKernelGGL(k_an_sum_part, dim3(kSumGroups), dim3(kT), 0, s, x, n, part);
  hipLaunchKernelGGL(k_an_sum_fold, dim3(1), dim3(64), 0, s, (const double*)part, out);
  return an_launch();
}

int64_t tomatis_an_spectrum_mean_work_doubles(int64_t n_frames, int32_t n_bins) {
  if (n_frames < 1 || n_frames > INT32_MAX || n_bins < 1) return 0;
  const int64_t pairs = (n_frames + 1) / 2;
  return (pairs + kSlabPairs - 1) / kSlabPairs * (int64_t)n_bins;
}

int tomatis_an_spectrum_mean(const float* x, int64_t n, int32_t ch, int32_t n_fft, int32_t hop,
                             int32_t sig_mode, float scale, const float* win, double* work,
                             double* out, void* hs) {
  if (!x || !win || !work || !out || hop < 1 || ch < 1 || n_fft < 1) return TOMATIS_E_ARG;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  if (sig_mode == TOMATIS_AN_SIG_RAW) {
    if (ch != 1) return TOMATIS_E_ARG;
  } else if (sig_mode == TOMATIS_AN_SIG_POWER_MONO) {
    if (ch != 2) return TOMATIS_E_ARG;
  } else {
    return TOMATIS_E_ARG;
  }
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  hipStream_t s = (hipStream_t)hs;
  MeanArgs B{{}, work};
  B.S.x = x;
  B.S.win = win;
  B.S.sc = scale;
  if ((rc = spec_args(n_fft, hop, F, s, &B.S)) != TOMATIS_OK) return rc;
  const int nb = B.S.n_bins;
  const int slabs = (int)(((F + 1LL) / 2 + kSlabPairs - 1) / kSlabPairs);
  const dim3 g((unsigned)slabs);
  const bool raw = sig_mode == TOMATIS_AN_SIG_RAW;
  rc = dispatch_m(B.S, [&](auto m, auto b) {
    constexpr int MM = decltype(m)::value;
    constexpr bool BL = decltype(b)::value;
    if (raw)
      hipLaunchKernelGGL((k_an_spec_mean<TOMATIS_AN_SIG_RAW, MM, BL>), g, dim3(kT), 0, s, B);
    else
      hipLaunchKernelGGL((k_an_spec_mean<TOMATIS_AN_SIG_POWER_MONO, MM, BL>), g, dim3(kT), 0, s,
                         B);
  });
  if (rc != TOMATIS_OK) return rc;
  hipLaunchKernelGGL(k_an_spec_mean_fold, dim3((nb + 63) / 64), dim3(64), 0, s,
                     (const double*)work, slabs, nb, F, out);
  return an_launch();
}

int tomatis_an_pair_tilt(const float* x, const float* y, int64_t n, int32_t n_fft, int32_t hop,
                         int32_t lo0, int32_t lo1, int32_t hi0, int32_t hi1, const float* win,
                         float* rows, double* band_means, void* hs) {
  if (!x || !y || !win || !band_means || hop < 1 || n_fft < 1 || n < 0) return TOMATIS_E_ARG;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  if (!bands_ok(n_fft / 2 + 1, lo0, lo1, hi0, hi1)) return TOMATIS_E_ARG;
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  hipStream_t s = (hipStream_t)hs;
  TiltArgs T{{}, band_means};
  T.S.x = x;
  T.S.y = y;
  T.S.win = win;
  T.S.out = rows;
  set_bands(&T.S, lo0, lo1, hi0, hi1);
  if ((rc = spec_args(n_fft, hop, F, s, &T.S)) != TOMATIS_OK) return rc;
  return dispatch_m(T.S, [&](auto m, auto b) {
    hipLaunchKernelGGL((k_an_pair_tilt<decltype(m)::value, decltype(b)::value>),
                       dim3((unsigned)F), dim3(kT), 0, s, T);
  });
}

int64_t tomatis_an_pair_diff_mean_work_doubles(int64_t n_sel, int32_t n_bins) {
  if (n_sel < 1 || n_sel > INT32_MAX || n_bins < 1) return 0;
  const int64_t slabs = (n_sel + kSlabFrames - 1) / kSlabFrames;
  return slabs * (int64_t)n_bins + (n_sel + 1) / 2;  // the partial sums, then the list
}

int tomatis_an_pair_diff_mean(const float* x, const float* y, int64_t n, int32_t n_fft,
                              int32_t hop, const float* win, const int32_t* frames,
                              int32_t n_sel, double* work, double* out, void* hs) {
  if (!x || !y || !win || !out || (!work && n_sel > 0) || hop < 1 || n_fft < 1 || n < 0 ||
      n_sel < 0)
    return TOMATIS_E_ARG;
  if (dft_m(n_fft) == 0) return TOMATIS_E_UNSUPPORTED;
  int F;
  int rc = frame_count(n, n_fft, hop, &F);
  if (rc != TOMATIS_OK || F == 0) return rc;
  if (!frames && n_sel != F) return TOMATIS_E_ARG;
  if (frames) {  // host memory: checked here, before anything is launched
    for (int32_t e = 0; e < n_sel; ++e)
      if (frames[e] < 0 || frames[e] >= F || (e && frames[e] <= frames[e - 1]))
        return TOMATIS_E_ARG;
  }
  hipStream_t s = (hipStream_t)hs;
  const int nb = n_fft / 2 + 1;
  if (n_sel == 0) {  // numpy's mean over no rows
    hipLaunchKernelGGL(k_an_fill_f64, dim3((nb + 255) / 256), dim3(256), 0, s, out, nb,
                       std::numeric_limits<double>::quiet_NaN());
    return an_launch();
  }
  const int slabs = (n_sel + kSlabFrames - 1) / kSlabFrames;
  const int32_t* list = nullptr;
  if (frames) {
    int32_t* dl = reinterpret_cast<int32_t*>(work + (int64_t)slabs * nb);
    rc = an_fail(hipMemcpyAsync(dl, frames, sizeof(int32_t) * (size_t)n_sel,
                                hipMemcpyHostToDevice, s));
    if (rc != TOMATIS_OK) return rc;
    list = dl;
  }
  DiffMeanArgs D{{}, list, n_sel, work};
  D.S.x = x;
  D.S.y = y;
  D.S.win = win;
  if ((rc = spec_args(n_fft, hop, F, s, &D.S)) != TOMATIS_OK) return rc;
  rc = dispatch_m(D.S, [&](auto m, auto b) {
    hipLaunchKernelGGL((k_an_pair_diff_mean<decltype(m)::value, decltype(b)::value>),
                       dim3((unsigned)slabs), dim3(kT), 0, s, D);
  });
  if (rc != TOMATIS_OK) return rc;
  hipLaunchKernelGGL(k_an_spec_mean_fold, dim3((nb + 63) / 64), dim3(64), 0, s,
                     (const double*)work, slabs, nb, n_sel, out);
  return an_launch();
}

int tomatis_cal_gate_grid(const float* levels, int32_t n_fit, const int64_t* starts,
                          const int32_t* target, const TomatisGateCand* cands, int32_t n_cand,
                          int32_t* out, uint8_t* states, void* hs) {
  if (n_fit < 0 || n_cand < 0 || (n_cand && (!cands || !out)) || (n_fit && (!levels || !starts)))
    return TOMATIS_E_ARG;
  if (n_cand == 0) return TOMATIS_OK;
  hipLaunchKernelGGL(k_cal_gate_grid, dim3((n_cand + 255) / 256), dim3(256), 0,
                     (hipStream_t)hs, levels, n_fit, starts, target, cands, n_cand, out, states);
  return an_launch();
}

int tomatis_an_frame_mean(const float* spec, int32_t n_frames, int32_t n_bins, float* out,
                          void* hs) {
  if (!spec || !out || n_frames < 1 || n_bins < 1) return TOMATIS_E_ARG;
  // one wave per 64 bins: spread the (latency-bound) chains over many CUs
  hipLaunchKernelGGL(k_an_frame_mean, dim3((n_bins + 63) / 64), dim3(64), 0,
                     (hipStream_t)hs, spec, n_frames, n_bins, out);
  return an_launch();
}

int64_t tomatis_an_median_work_words(int32_t n_bins) {
  return n_bins < 1 ? 0 : (int64_t)n_bins * (4 + 256);
}

int tomatis_an_frame_median(const float* spec, int32_t n_frames, int32_t n_bins,
                            const uint8_t* mask, int32_t n_sel, uint32_t* work, float* out,
                            void* hs) {
  if (!spec || !out || !work || n_frames < 1 || n_bins < 1 || n_sel < 1 || n_sel > n_frames)
    return TOMATIS_E_ARG;
  hipStream_t s = (hipStream_t)hs;
  MedState* st = reinterpret_cast<MedState*>(work);
  uint32_t* gh = work + (int64_t)n_bins * 4;
  const int even = (n_sel % 2) == 0;
  const uint32_t k1 = even ? (uint32_t)(n_sel / 2 - 1) : (uint32_t)(n_sel / 2);
  const dim3 gb((n_bins + 255) / 256);
  hipLaunchKernelGGL(k_an_med_init, gb, dim3(256), 0, s, st, n_bins, k1);
  // frame splits: enough workgroups to cover the chip, >= 1024 frames each
  const int groups = (n_bins + 63) / 64;
  int splits = (n_frames + 1023) / 1024;
  splits = std::max(1, std::min(splits, std::max(1, 2048 / groups)));
  const int per = (n_frames + splits - 1) / splits;
  const size_t gh_bytes = sizeof(uint32_t) * (size_t)n_bins * 256;
  for (int pass = 0; pass < 4 + even; ++pass) {
    int rc = (pass < 4) ? an_fail(hipMemsetAsync(gh, 0, gh_bytes, s))
                        : an_fail(hipMemsetAsync(gh, 0xFF, gh_bytes, s));
    if (rc != TOMATIS_OK) return rc;
    hipLaunchKernelGGL(k_an_med_hist, dim3(groups, splits), dim3(256), 0, s, spec, n_frames,
                       n_bins, mask, st, gh, pass, per);
    hipLaunchKernelGGL(k_an_med_pick, gb, dim3(256), 0, s, st, gh, n_bins, pass);
    rc = an_launch();
    if (rc != TOMATIS_OK) return rc;
  }
  hipLaunchKernelGGL(k_an_med_final, gb, dim3(256), 0, s, st, n_bins, even, out);
  return an_launch();
}

}  // extern "C"
