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
//
// Every index below (the plan, the argument rule, what a tile and an element
// compute, the table's source) is a function of tm_resample_plan.h, host and
// device, which tools/resample_plan_check.cpp checks on the CPU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"
#include "tm_resample_plan.h"

namespace {

using namespace tm_rs;

int rs_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 1)
    cus = 256;
  return cus;
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
  const int tid = threadIdx.x;
  const int ch = CH ? CH : pl.ch;
  // once per workgroup; the first barrier of the loop publishes it
  for (int i = tid; i < pl.tab_words; i += kT) {
    const int m = rs_tab_src(pl, i);
    tab[i] = m >= 0 ? taps[m] : 0.0f;
  }
  const i64 lo = start * ch, hi = (start + len) * ch;  // the live words of x
  const int n_el = pl.T * ch, steps = pl.K4 / 4;
  for (i64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const RsTile tl = rs_tile(pl, ch, start, tile);
    const i64 j0 = tl.j0, a0 = tl.a0;
    const int p0 = tl.p0, shift = tl.shift, nq = tl.nq;  // 4 nq <= stage_words
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
      const RsElem el = rs_elem(pl, ch, p0, e);
      if (j0 + el.o >= n_out) break;  // e grows with o
      const float* sp = stage + rs_first_word(shift, ch, el);
      const float* h = tab + rs_tab_row(pl, el.p);
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
  RsPlan pl;
  i64 n_out = 0, tiles = 0;
  switch (rs_check_args(x != nullptr, taps != nullptr, out != nullptr, n_total, start, len,
                        channels, up, down, n_taps, &pl, &n_out, &tiles)) {
    case kRsOk: break;
    case kRsArg: return TOMATIS_E_ARG;
    default: return TOMATIS_E_UNSUPPORTED;
  }
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
