// tm_resample.hip — the audio resampler (workflow step 2.1).
//
// scipy.signal.resample_poly(x, up, down, axis=0) for interleaved multichannel
// float32 PCM, the call the reference makes wherever it changes a rate, as one
// polyphase pass: tomatis_resample_poly -> k_rs_poly.
//
// With half = (n_taps - 1) / 2, c = down j + half, p = c mod up, ih = c / up and
// K = ceil(n_taps / up), output frame j of channel ch is
//   y[j][ch] = sum_v taps[p + up (K - 1 - v)] x[start + ih - (K - 1) + v][ch],  v < K,
// a tap index >= n_taps counting as a zero tap and a frame outside
// [start, start + len) as a zero sample (the formula of §7f with
// the envelope replaced by the samples of one channel).
//
// Regime: K is 21 (160 / 147) to 161 (1 / 8) terms per output and the output is
// about as large as the input, so the pass is meant to move bytes: unlike
// k_al_envelope no output is split over threads and nothing is reduced.
//
// Layout (wave64, 256-thread workgroups, resident grid walking the tiles):
//  * a workgroup owns T consecutive output frames, T ch (frame, channel)
//    elements; thread t takes the elements t, t + 256, ...: element e is
//    channel e mod ch of frame e / ch, so the stores of a wave are consecutive
//    words of out.
//  * stage: the W = floor((up - 1 + down (T - 1)) / up) + K4 input frames the
//    tile reads (K4 = K rounded up to four), interleaved as in x.  The words are
//    fetched with 16-byte loads from the 16-byte boundary below the first one,
//    four loads in flight per thread; a load that crosses an end of the range
//    (or x not 16-byte aligned) is done by words, zeros outside the range.
//    Neighbouring elements start down / up frames apart: the 4-byte reads of a
//    wave are near-consecutive words.
//  * tab: the taps by phase, tab[p Ks + v] = taps[p + up (K - 1 - v)], zero for
//    v >= K; Ks >= K4 and Ks / 4 is odd, so the 16-byte reads of 16 phases start
//    on 16 distinct 16-byte slots of the 64 banks.  Built once per workgroup.
//    For up == 1 there is one row and every lane reads the same words.
//  * arithmetic: four float32 FMA chains over v mod 4 (K4 / 4 steps, the zero
//    taps of the padding add +0), joined as (a0 + a1) + (a2 + a3).  The order is
//    a function of (up, down, n_taps) and the phase alone: an output's bits do
//    not depend on start, len, the tile, the channel count or the run.
// T is the largest power of two <= 1024 whose stage and table fit 64 KiB; it
// depends on (up, down, n_taps, channels) alone (resample.outputs_per_workgroup).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"

namespace {

typedef long long i64;

constexpr int kT = 256;             // threads per workgroup
constexpr int kMaxTile = 1024;      // output frames per workgroup, at most
constexpr int kLdsBytes = 64 * 1024;
constexpr int kMaxRatio = 512;      // max(up, down)
constexpr int kMaxDecim = 8;        // down <= kMaxDecim up
constexpr int kMaxCh = 8;
constexpr int kInFlight = 4;        // 16-byte loads in flight per thread while staging

struct RsPlan {
  int up, down, n_taps, ch, K, K4, Ks, T, W, stage_words, tab_words;
};

int rs_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  return cus;
}

bool rs_plan(int up, int down, int n_taps, int ch, RsPlan* pl) {
  pl->up = up, pl->down = down, pl->n_taps = n_taps, pl->ch = ch;
  pl->K = (n_taps + up - 1) / up;
  pl->K4 = (pl->K + 3) / 4 * 4;
  pl->Ks = 4 * (((pl->K + 3) / 4) | 1);
  pl->tab_words = up * pl->Ks;
  for (int T = kMaxTile; T >= 1; T >>= 1) {
    pl->T = T;
    pl->W = (int)(((i64)up - 1 + (i64)down * (T - 1)) / up) + pl->K4;
    pl->stage_words = (3 + pl->W * ch + 3) / 4 * 4;  // up to 3 words before the first frame
    if (sizeof(float) * ((size_t)pl->stage_words + pl->tab_words) <= (size_t)kLdsBytes)
      return true;
  }
  return false;
}

// CH: the channel count where it is 1 or 2, else 0 (pl.ch at run time)
template <int CH>
__global__ __launch_bounds__(kT) void k_rs_poly(const float* __restrict__ x, i64 start, i64 len,
                                                const float* __restrict__ taps, RsPlan pl,
                                                float* __restrict__ out, i64 n_out, int tiles,
                                                int vec) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* stage = lds;
  float* tab = lds + pl.stage_words;
  const int tid = threadIdx.x, up = pl.up, down = pl.down, K = pl.K;
  const int ch = CH ? CH : pl.ch;
  // once per workgroup; the first barrier of the loop publishes it
  for (int i = tid; i < pl.tab_words; i += kT) {
    const int p = i / pl.Ks, v = i - p * pl.Ks;
    const int m = p + up * (K - 1 - v);
    tab[i] = (v < K && m < pl.n_taps) ? taps[m] : 0.0f;
  }
  const i64 lo = start * ch, hi = (start + len) * ch;  // the live words of x
  const int n_el = pl.T * ch, steps = pl.K4 / 4;
  for (i64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const i64 j0 = tile * pl.T;
    const i64 c0 = (i64)down * j0 + (pl.n_taps - 1) / 2;
    const i64 ih0 = c0 / up;
    const int p0 = (int)(c0 - ih0 * up);
    const i64 w0 = (start + ih0 - (K - 1)) * ch;  // first word of the span; may lie below 0
    const i64 a0 = w0 & ~(i64)3;
    const int shift = (int)(w0 - a0);
    const int nq = (shift + pl.W * ch + 3) / 4;   // 16-byte pieces; 4 nq <= stage_words
    __syncthreads();  // the previous tile's reads of stage
    for (int q0 = tid; q0 < nq; q0 += kInFlight * kT) {
      float4 r[kInFlight];
#pragma unroll
      for (int k = 0; k < kInFlight; ++k) {
        const int q = q0 + k * kT;
        const i64 a = a0 + 4 * (i64)q;
        r[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q < nq) {
          if (vec && a >= lo && a + 4 <= hi) {
            r[k] = *reinterpret_cast<const float4*>(x + a);
          } else {  // an end of the range: by words, zeros outside it
            if (a >= lo && a < hi) r[k].x = x[a];
            if (a + 1 >= lo && a + 1 < hi) r[k].y = x[a + 1];
            if (a + 2 >= lo && a + 2 < hi) r[k].z = x[a + 2];
            if (a + 3 >= lo && a + 3 < hi) r[k].w = x[a + 3];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < kInFlight; ++k) {
        const int q = q0 + k * kT;
        if (q < nq) *reinterpret_cast<float4*>(stage + 4 * q) = r[k];
      }
    }
    __syncthreads();
    for (int e = tid; e < n_el; e += kT) {
      const int o = e / ch, c = e - o * ch;
      if (j0 + o >= n_out) break;  // e grows with o
      const int xo = p0 + down * o, ao = xo / up, p = xo - ao * up;
      const float* sp = stage + shift + ao * ch + c;
      const float* h = tab + p * pl.Ks;
      float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
      for (int i = 0; i < steps; ++i) {
        const float4 t = *reinterpret_cast<const float4*>(h + 4 * i);
        s0 = fmaf(t.x, sp[0], s0);
        s1 = fmaf(t.y, sp[ch], s1);
        s2 = fmaf(t.z, sp[2 * ch], s2);
        s3 = fmaf(t.w, sp[3 * ch], s3);
        sp += 4 * ch;
      }
      out[j0 * ch + e] = (s0 + s1) + (s2 + s3);
    }
  }
}

}  // namespace

extern "C" {

int tomatis_resample_poly(const float* x, int64_t n_total, int64_t start, int64_t len,
                          int32_t channels, int32_t up, int32_t down, const float* taps,
                          int32_t n_taps, float* out, void* hs) {
  if (!x || !taps || !out || n_total < 0 || start < 0 || len < 1 || len > n_total - start ||
      n_taps < 1 || (n_taps & 1) == 0 || up < 1 || down < 1 || up == down || channels < 1 ||
      channels > kMaxCh)
    return TOMATIS_E_ARG;
  for (int a = up, b = down;;) {  // gcd(up, down) == 1
    const int r = a % b;
    if (r == 0) {
      if (b != 1) return TOMATIS_E_ARG;
      break;
    }
    a = b, b = r;
  }
  const int big = up > down ? up : down;
  if (big > kMaxRatio || (i64)down > (i64)kMaxDecim * up || n_taps > 20 * big + 1 ||
      n_total > (int64_t)1 << 48)
    return TOMATIS_E_UNSUPPORTED;
  RsPlan pl;
  if (!rs_plan((int)up, (int)down, (int)n_taps, (int)channels, &pl)) return TOMATIS_E_UNSUPPORTED;
  const i64 n_out = ((i64)len * up + down - 1) / down;
  const i64 tiles = (n_out + pl.T - 1) / pl.T;
  if (tiles > 0x7FFFFFFF) return TOMATIS_E_UNSUPPORTED;
  const i64 cap = (i64)rs_cus() * 4;  // resident workgroups, each builds its phase table once
  const unsigned groups = (unsigned)(tiles < cap ? tiles : cap);
  const size_t lds = sizeof(float) * ((size_t)pl.stage_words + pl.tab_words);
  const int vec = ((uintptr_t)x & 15u) == 0;
  hipStream_t s = (hipStream_t)hs;
#define TM_RS(CH)                                                                          \
  hipLaunchKernelGGL((k_rs_poly<CH>), dim3(groups), dim3(kT), lds, s, x, (i64)start, (i64)len, \
                     taps, pl, out, n_out, (int)tiles, vec)
  if (channels == 1) TM_RS(1);
  else if (channels == 2) TM_RS(2);
  else TM_RS(0);
#undef TM_RS
  return hipGetLastError() == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP;
}

}  // extern "C"
