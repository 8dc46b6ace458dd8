// tm_layout.h — plain types and constants shared by the plan (tm_plan.cpp, host
// only), the kernels (tm_kernels.hip) and the fused transform (tm_transform.hip):
// the work items the plan lays out and the kernels walk.  No device code: it
// compiles with a plain host compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"

namespace tdsp {
struct cf {  // complex float (the kernels' register arithmetic on it: tm_common.h)
  float x, y;
};
}  // namespace tdsp

namespace tshared {
struct Run {          // main-kernel work item: emit frames [ka, kb) of stream s
  int32_t s;
  int32_t last;       // bit 0: kb is the stream's last frame + 1; bit 1: kRunInterior
  int64_t ka, kb;
};
// interior run: frames [max(0, ka - rmax + 1), kb) all read full frames and every
// emitted hop block is a full interior block (fast loop of the fused kernel)
constexpr int32_t kRunInterior = 2;

constexpr int kGateLookback = 512;       // look-back limit of a run that cannot chain
constexpr int kGateLookbackMax = 4096;   // chained runs: frames back to the previous run's start
constexpr int kGateChainStates = 1024;   // chaining needs gate_D + 2 <= this (transfer tables)
constexpr int kGateChained = -2;         // k_gate_carry -> k_gate_chain marker

// Any-size path (any n_fft in [2, kMaxNfft], any hop, 1..kMaxCh channels): per
// (frame, channel pair) a Stockham FFT of length M (n_fft when it is a power
// of two, else Bluestein's power of two >= 2 n_fft - 1) in LDS (M <= kLdsMaxM)
// or in per-block HBM buffers, windowed frames to scratch float
// [frame][n_fft][ch], then a per-position gather in frame order.
constexpr int kMaxNfft = 1 << 16;
constexpr int kMaxCh = 128;
constexpr int kLdsMaxM = 16384;

// n_fft 2048 register kernels (P = 64) run the single-exchange FFT (tm_fft.h
// fftx_*; its bin layout in the gain rows, its output scales in winS); the
// two-exchange form stays for n_fft 4096 and for -DTM_DEV_NOFX A/B builds
#ifdef TM_DEV_NOFX
constexpr bool kFftX = false;
#else
constexpr bool kFftX = true;
#endif

int transform_wg(int P, int NR);  // workgroup size of the fused kernel
int transform_slots_per_cu(int P, int NR);  // resident sequences per CU
int dev_opt(int key, int dflt);  // tomatis_set_dev_option (default when unset)

}  // namespace tshared

// Internal linkage, as before these moved here from tm_kernels.hip: the
// kernels' symbol names carry the struct types below.
namespace {

constexpr int kSeg = 1024;           // gate segment length (frames)
// xfade alpha segment length (frames): each segment's alpha recurrence is one
// lane's latency chain (k_alpha_sync / k_alpha_prefix), so short segments, many
// waves (C5x: 3.5 k segments of 128 frames instead of 440 of 1024)
constexpr int kASeg = 128;
constexpr int kLevelLds = 12288;     // floats of LDS for the levels span
constexpr int kMaxGateStates = 65535;  // uint16 state ids (transfer tables)
constexpr int kPwMaxLeaves = 2048;   // k_levels_any: leaf sums held in LDS

struct LvlBlock {     // levels work item
  int32_t s;
  int32_t nf;
  int64_t k0;
};
struct GateSeg {      // gate segment
  int32_t s;
  int32_t nf;
  int64_t k0;         // first frame (stream-local)
};

struct GSum {         // run-scan gate: segment summary (k_gate_sum)
  int all_on;  // every frame on
  int not_on;  // last not-on frame
  int l_end;   // last frame of the leading on-run (kNI if the first frame is not on)
  int e_int;   // last entry after the first not-on frame
  int off;     // last off frame
};
struct GCarry {       // run-scan gate: carry into a segment (k_gate_carry)
  int a, e, f;
};

constexpr int kMhLdsTf = 8192;        // (segment, start state) transfer entries held in LDS
constexpr int kMhLdsSym = 4096;       // symbol words held in LDS (65536 frames)

// Segment length (frames, a multiple of 16 = one symbol word): at least 256,
// few enough segments that the (segment, start) transfer table fits in LDS and
// the final pass's segment starts fit its 4096-entry table.  Host and device.
__host__ __device__ inline int64_t mh_seg_len(int64_t F, int ns) {
  int64_t seg = 256;
  const int64_t a = (F * ns + kMhLdsTf - 1) / kMhLdsTf, b = (F + 4095) / 4096;
  seg = a > seg ? a : seg;
  seg = b > seg ? b : seg;
  return (seg + 15) & ~(int64_t)15;
}

struct MhBisect {     // speculative bisection state per stream (k_mh_init / k_mh_probe)
  double lo, hi, best_T, best_diff;
  int32_t it, done, arrive, pad;
};
constexpr int kMhProbes = 7;
constexpr int kMhSlots = kMhProbes + 1;  // the probes + best_T (k_mh_probe)

struct ChunkDesc {    // limiter work item (k_limiter)
  int32_t s, c;
  int64_t p0, p1;  // output-relative sample range [p0, p1)
};

}  // namespace
