// tm_plan.h — the processor plan (tomatis_plan_s): stream table, work
// decompositions and the device buffers it owns.  Built by tm_plan.cpp (host
// only: no kernel, no device header), read by the launches of tm_kernels.hip.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "tm_layout.h"

namespace tshared {
inline int hipfail(hipError_t e) { return e == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP; }

// Device memory with one owner: pointer + element count, freed with it.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { return std::swap(p_, o.p_), std::swap(n_, o.n_), *this; }
  ~DevBuf() { (void)alloc(0); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  int n() const { return (int)n_; }  // (of a work-item list: a grid size)
  int alloc(size_t n) {  // n uninitialised elements (none: empty, get() == nullptr)
    if (p_) (void)hipFree(p_);
    p_ = nullptr, n_ = 0;
    if (n == 0) return TOMATIS_OK;
    if (hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)) != hipSuccess) {
      p_ = nullptr;
      return TOMATIS_E_NOMEM;
    }
    n_ = n;
    return TOMATIS_OK;
  }
  int ensure(size_t n) { return n > n_ ? alloc(n) : TOMATIS_OK; }  // grows only, contents dropped
  int upload(const std::vector<T>& v) {
    const int rc = alloc(v.size());
    if (rc || v.empty()) return rc;
    return hipfail(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  int zero() { return p_ ? hipfail(hipMemset(p_, 0, n_ * sizeof(T))) : TOMATIS_OK; }
 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// output scales of the register FFT's NR-point DFT through plan W (tm_common.h
// splan<NR, W>().sig; NR 16 or 32); defined next to the kernels
const double* register_fft_scales(int NR, int W);

}  // namespace tshared

struct tomatis_plan_s {
  template <typename T>
  using DevBuf = tshared::DevBuf<T>;
  using Run = tshared::Run;
  TomatisPlanDesc d{};
  int32_t n_streams = 0;
  int64_t total_frames = 0;
  int32_t total_chunks = 0;
  int P = 0, NR = 32, SH = 0, rmax = 1;
  bool generic = false;
  bool fx = false;  // fused kernel runs the single-exchange FFT (tm_fft.h fftx_*)
  bool lds = false;        // any-size path (k_stft_lds + k_ola_gather_lds)
  std::vector<TomatisStream> hs;
  DevBuf<TomatisStream> st;
  // runs of the fused kernel
  DevBuf<Run> runs;
  std::vector<Run> hruns;  // host copy of the runs
  int64_t run_slots = 0;   // resident sequences of the fused kernel
  // output position prefix per stream (gather kernels)
  DevBuf<int64_t> pos_base;
  int64_t total_out = 0;
  struct Levels {  // k_levels / k_levels_any / k_leaves + k_frame_r
    int nf = 0;    // frames per level block
    DevBuf<LvlBlock> blocks;
    // streaming levels (hop % 128 == 0): per-stream 8-block groups and leaves
    bool leaf_path = false;
    int64_t n_groups = 0;
    int64_t max_groups = 0;          // most groups of one stream (k_leaves grid x)
    DevBuf<int64_t> grp_base, leaf_base;
    DevBuf<double> leaves;           // (k_leaves<float> writes floats into it)
    // levels for any n_fft (k_levels_any): numpy pairwise leaves + postfix program
    bool any = false;
    DevBuf<int2> pw_leaf;
    DevBuf<int16_t> pw_prog;
  } lvl;
  struct Gate {  // k_gate_* / k_alpha_*, and the fused kernel's in-kernel gate
    DevBuf<GateSeg> segs;
    DevBuf<int32_t> seg_first, seg_count;
    DevBuf<GateSeg> asegs;        // xfade alpha segments (kASeg frames)
    DevBuf<int32_t> aseg_first, aseg_count;
    DevBuf<uint16_t> tf, seg_start;
    // run-scan gate (exclusive on/off predicates)
    bool excl = false;
    DevBuf<GSum> gsum;
    DevBuf<GCarry> gcarry;
    DevBuf<GCarry> gcarry_in;     // time shards: carry-in per stream
    DevBuf<int32_t> aq;           // xfade alpha passes: sync frame per gate segment
    DevBuf<double> afin, acin;    //   alpha at the segment end (when synced) / carry-in alpha
    // in-kernel levels + gate (tomatis_stft_ola_gated): per-run carry-in
    DevBuf<int32_t> carry;
    DevBuf<uint16_t> run_tf;      // chained runs' transfer tables [run][D + 2]
    DevBuf<double> acarry;        // cross-fade: alpha before each run's first frame
    // not owned: the caller's per-frame alpha array (tomatis_plan_set_gate_alpha)
    double* aout = nullptr;
    // not owned: the input the carries belong to (nullptr: no look-back yet)
    const float* gl_x = nullptr;
  } gate;
  struct MinHold {  // k_minhold / k_mh_*
    DevBuf<uint16_t> tf;
    DevBuf<int32_t> cnt;
    DevBuf<int64_t> off;
    DevBuf<uint32_t> sym;
    DevBuf<int64_t> soff;
    DevBuf<MhBisect> bs;     // speculative bisection state per stream
    int serial = 0;          // TOMATIS_OPT_MINHOLD_SERIAL
    DevBuf<int32_t> pc;      // probe counts [stream][kMhProbes]
    DevBuf<uint16_t> gtf;    // probe tables [stream][kMhSlots][nseg * ns]
    DevBuf<int32_t> gcnt;
    DevBuf<int64_t> goff;
    DevBuf<int32_t> arr;     // probe arrival counters [stream][kMhSlots]
    int parts = 1;           // workgroups per probe
  } mh;
  struct Limiter {  // k_limiter and the fused limiter
    DevBuf<ChunkDesc> chunks;
    int64_t max_chunk = 0;
    DevBuf<uint32_t> need, done;
    DevBuf<int64_t> rng;
    DevBuf<uint32_t> err;
    int fuse_span = 0;     // max runs contributing to one chunk
    int edge_mask = 0;     // set for one tomatis_stft_ola_limited_edges call
    int fuse_enabled = 1;  // TOMATIS_OPT_FUSE_LIMITER
    int spin = 1 << 18;    // TOMATIS_OPT_LIMITER_SPIN: fused-limiter wait bound (polls)
  } lim;
  struct Tables {  // the register transform kernels
    DevBuf<float> win;
    DevBuf<float> winS;  // synthesis window x the register FFT's inverse output scales
    DevBuf<float> win2, winv;
    DevBuf<tdsp::cf> twN, twP;
    DevBuf<float> scratch;  // generic hop: cf per position; any-size path: ch floats
    DevBuf<float> gperm;    // permuted gain rows, grown to the most rows of a call
  } tab;
  struct AnySize {  // k_stft_lds: FFT length M (= n_fft, or Bluestein's power of two)
    int M = 0;
    bool blue = false;
    DevBuf<float2> tw;      // exp(-2 pi i t / M)
    DevBuf<float2> blue_b;  // chirp exp(i pi n^2 / N), n < N
    DevBuf<float2> blue_h;  // FFT_M of the chirp filter / M
    DevBuf<float2> work;    // M > kLdsMaxM: per-block ping-pong buffers in HBM
    int work_blocks = 0;
  } any;
  // pipelined batches (tomatis_stft_ola_gated_pipelined): per run the previous
  // batch's blocks to rescale in the frame loop (k_r2_plan output)
  struct Pipeline {
    DevBuf<uint32_t> pieces;
    int max_pieces = 0;
  } pipe;
};

// level blocks of nf frames over every stream (k_levels work items)
inline std::vector<LvlBlock> level_blocks(const tomatis_plan_s* p, int nf) {
  std::vector<LvlBlock> lb;
  for (int s = 0; s < p->n_streams; ++s)
    for (int64_t a = 0, F = p->hs[s].n_frames; a < F; a += nf)
      lb.push_back(LvlBlock{s, (int32_t)std::min<int64_t>(nf, F - a), a});
  return lb;
}
