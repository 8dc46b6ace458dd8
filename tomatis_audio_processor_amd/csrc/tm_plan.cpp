// tm_plan.cpp — plan creation for the STFT-gate-OLA engine: stream validation,
// kernel-path selection and the layout of every work decomposition (runs of
// the fused kernel, limiter accounting, level blocks, gate / alpha segments,
// chunk descriptors, min-hold workspace), uploaded into buffers the plan owns.
// Host code only: it launches no kernel and compiles with a plain C++ compiler
// (tools/plan_check.cpp links it against a fake runtime and checks the layout).
#include "tm_plan.h"

#include <cmath>
#include <new>

#include "tm_host_dsp.h"

using namespace tshared;
using tdsp::cf;

namespace tshared {
// development overrides (tomatis_set_dev_option); -1 = the default
constexpr int kDevKeys = 16;
static int g_dev[kDevKeys] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
int dev_opt(int key, int dflt) {
  const int v = (key > 0 && key < kDevKeys) ? g_dev[key] : -1;
  return v < 0 ? dflt : v;
}
}  // namespace tshared

namespace {

int cu_count() {
  int dev = 0, ncu = 256;
  if (hipGetDevice(&dev) == hipSuccess)
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  return std::max(1, ncu);
}

// no float32 bit pattern can satisfy both gate predicates (run-scan gate valid)
bool gate_exclusive(const TomatisStream& S) {
  auto in = [](uint32_t b, const uint32_t* e, int n) {
    for (int i = 0; i < n; ++i)
      if (e[i] == b) return true;
    return false;
  };
  auto on = [&](uint32_t b) { return (b >= S.on_bits) != in(b, S.on_exc, S.n_on_exc); };
  auto off = [&](uint32_t b) { return (b <= S.off_bits) != in(b, S.off_exc, S.n_off_exc); };
  if (S.n_on_exc < 0 || S.n_on_exc > 4 || S.n_off_exc < 0 || S.n_off_exc > 4) return false;
  if (S.on_bits <= S.off_bits) return false;
  for (int i = 0; i < S.n_on_exc; ++i)
    if (on(S.on_exc[i]) && off(S.on_exc[i])) return false;
  for (int i = 0; i < S.n_off_exc; ++i)
    if (on(S.off_exc[i]) && off(S.off_exc[i])) return false;
  return true;
}

// Runs of the fused kernel (once per plan; the fused-limiter accounting that
// depends on them: limiter_accounting).
int build_runs(tomatis_plan_s* p) {
  const TomatisPlanDesc& d = p->d;
  const int N = d.n_fft, hop = d.hop, P = p->P;
  const int ns = p->n_streams;
  const int64_t tf_total = std::max<int64_t>(1, p->total_frames);
  // Runs.  Per stream, the emitted frames [e_lo, e_hi) whose run can take the
  // fused kernel's interior loop (full frame loads back to the warm-up frames,
  // full interior output blocks, not the stream's last frame) are cut into
  // equal runs; the few edge frames before/after form one generic run each.
  // One run per resident sequence slot of the fused kernel (a single wave of
  // blocks, every wave busy to the end), at least 48 frames per interior run
  // so the rmax-1 warm-up frames per run stay a few percent.
  const int rmax_ = (N + hop - 1) / hop;
  const bool fast_ok = !p->generic && P == 64 && dev_opt(TOMATIS_DEV_FAST_LOOP, 1) != 0;
  std::vector<int64_t> e_lo(ns, 0), e_hi(ns, 0);
  int64_t fast_total = 0, n_edge = 0;
  for (int s = 0; s < ns; ++s) {
    const TomatisStream& S = p->hs[s];
    const int64_t F = S.n_frames;
    int64_t lo = F, hi = F;
    if (fast_ok && F > 0) {
      auto ceil_div = [](int64_t a_, int64_t b_) { return a_ >= 0 ? (a_ + b_ - 1) / b_ : -((-a_) / b_); };
      lo = rmax_ - 1;                                                   // not an edge frame
      lo = std::max(lo, ceil_div(S.out_begin - S.first_start, hop));     // s_k >= out_begin
      lo = std::max(lo, ceil_div(-S.first_start, hop) + rmax_ - 1);      // warm-up frames load fully
      // s_k + hop <= out_end, s_k + N <= n, k <= F - 2
      hi = F - 1;
      const int64_t out_end = S.out_begin + S.out_len;
      auto fdiv = [](int64_t a_, int64_t b_) { return a_ >= 0 ? a_ / b_ : -((-a_ + b_ - 1) / b_); };
      hi = std::min(hi, fdiv(out_end - hop - S.first_start, hop) + 1);
      hi = std::min(hi, fdiv(S.n - N - S.first_start, hop) + 1);
      lo = std::max<int64_t>(0, lo);
      if (hi - lo < 48) lo = hi = F;  // too short: all generic
      else n_edge += (lo > 0) + (hi < F);
    }
    e_lo[s] = lo;
    e_hi[s] = hi;
    fast_total += hi - lo;
  }
  // resident sequence slots of the fused kernel
  int64_t slots = (int64_t)cu_count() * (p->generic ? 8 : transform_slots_per_cu(P, p->NR));
  const int dslots = dev_opt(TOMATIS_DEV_SLOTS, 0);  // tests: long runs on small inputs
  if (dslots > 0) slots = dslots;
  p->run_slots = slots;
  // Runs the in-kernel gate may take (tomatis_stft_ola_gated: standard mode at
  // n_fft 2048) are at most kGateLookbackMax frames, so every run's look-back
  // can chain to its predecessor's carry (k_gate_carry): a batch larger than
  // slots x kGateLookbackMax frames gets more rounds of runs instead of longer
  // runs, and a stream hovering inside the hysteresis band never sends the
  // pass back to the two-pass chain (src/process_tomatis.py:373-385 has no
  // horizon either)
  const bool gate_runs = d.alpha_mode == 0 && N == 2048 && P == 64 && !p->generic && !p->lds;
  // rounds: the runs fill the slots this many times over, in stream/position
  // order, so (in-order dispatch) early streams and chunks complete while later
  // runs still compute, and their limiter rescale overlaps that compute
  // (adaptive: every stream is one limiter chunk, measured 1.4 ms faster on C3
  // with 2 rounds; standard 10 s chunks gain nothing and pay warm-up frames)
  int rounds = std::max(1, dev_opt(TOMATIS_DEV_RUN_ROUNDS, (d.alpha_mode == 2 && ns > 1) ? 2 : 1));
  int T = dev_opt(TOMATIS_DEV_RUN_FRAMES, 0);
  if (T <= 0) {
    // generic streams and the edge runs take slots first
    int64_t gen_frames = 0;
    for (int s = 0; s < ns; ++s)
      if (e_lo[s] == e_hi[s]) gen_frames += p->hs[s].n_frames;
    const int64_t work = fast_total + gen_frames;
    if (gate_runs) {  // enough rounds that runs stay within the chained look-back
      const int64_t per_round = std::max<int64_t>(1, slots - n_edge) * (int64_t)(kGateLookbackMax - 64);
      rounds = (int)std::max<int64_t>(rounds, (work + per_round - 1) / per_round);
    }
    const int64_t avail = std::max<int64_t>(1, rounds * slots - n_edge);
    T = (int)std::max<int64_t>(rounds > 1 ? 32 : 48, (work + avail - 1) / avail);
    auto count = [&](int64_t t) {
      int64_t c = n_edge;
      for (int s = 0; s < ns; ++s) {
        const int64_t len = (e_lo[s] == e_hi[s]) ? p->hs[s].n_frames : e_hi[s] - e_lo[s];
        c += (len + t - 1) / t;
      }
      return c;
    };
    while (count(T) > rounds * slots && T < tf_total) T += std::max(1, T / 64);
  }
  T = std::min(T, 1 << 20);  // interior buffer resources stay far below 4 GB
  if (gate_runs) T = std::min(T, kGateLookbackMax);
  std::vector<Run> runs;
  auto add_runs = [&](int s, int64_t a0, int64_t a1, int32_t flags) {
    // equal cuts of [a0, a1) into ceil(len / T) runs
    const int64_t len = a1 - a0;
    if (len <= 0) return;
    const int64_t nr = (len + T - 1) / T;
    for (int64_t j = 0; j < nr; ++j) {
      Run r;
      r.s = s;
      r.ka = a0 + len * j / nr;
      r.kb = a0 + len * (j + 1) / nr;
      r.last = flags | ((r.kb == p->hs[s].n_frames) ? 1 : 0);
      runs.push_back(r);
    }
  };
  for (int s = 0; s < ns; ++s) {
    const int64_t F = p->hs[s].n_frames;
    if (e_lo[s] == e_hi[s]) {
      add_runs(s, 0, F, 0);
      continue;
    }
    if (e_lo[s] > 0) add_runs(s, 0, e_lo[s], 0);
    add_runs(s, e_lo[s], e_hi[s], kRunInterior);
    if (e_hi[s] < F) add_runs(s, e_hi[s], F, 0);
  }
  p->hruns = runs;
  return p->runs.upload(runs);
}

// Fused-limiter accounting over the plan's runs: flushes expected per chunk
// (host mirror of the kernel's frame-indexed chunk walk) and the largest run
// span of a chunk.
int limiter_accounting(tomatis_plan_s* p) {
  if (p->generic || p->total_chunks <= 0) return TOMATIS_OK;
  const int HOP = p->d.hop, wpr = p->P / 64;
  const std::vector<Run>& runs = p->hruns;
  std::vector<uint32_t> need(p->total_chunks, 0);
  std::vector<int32_t> first_run(p->total_chunks, -1), last_run(p->total_chunks, -1);
  for (int ri = 0; ri < (int)runs.size(); ++ri) {
    const Run& R = runs[ri];
    const TomatisStream& S = p->hs[R.s];
    const int64_t s_ka = S.first_start + R.ka * HOP;
    int cid = 0;
    if (S.n_chunks > 1 && s_ka >= S.chunk_first)
      cid = (int)std::min<int64_t>(1 + (s_ka - S.chunk_first) / S.chunk_len, S.n_chunks - 1);
    int64_t next_k = INT64_MAX;
    if (S.n_chunks > 1 && cid < S.n_chunks - 1)
      next_k = (S.chunk_first + (int64_t)cid * S.chunk_len - S.first_start) / HOP;
    const int64_t step = S.n_chunks > 1 ? S.chunk_len / HOP : 0;
    auto mark = [&](int c) {
      const int g = S.chunk_base + c;
      need[g] += wpr;
      if (first_run[g] < 0) first_run[g] = ri;
      last_run[g] = ri;
    };
    while (next_k < R.kb) {
      if (next_k >= R.ka) {
        mark(cid);
        ++cid;
        next_k = (cid < S.n_chunks - 1) ? next_k + step : INT64_MAX;
      } else {
        break;  // cannot happen: next chunk starts after the run's first frame
      }
    }
    mark(cid);
  }
  int span = 0;
  for (int g = 0; g < p->total_chunks; ++g)
    if (first_run[g] >= 0) span = std::max(span, last_run[g] - first_run[g] + 1);
  p->lim.fuse_span = span;
  return p->lim.need.upload(need);
}

int build_levels(tomatis_plan_s* p) {
  const TomatisPlanDesc& d = p->d;
  const int N = d.n_fft, hop = d.hop, ns = p->n_streams;
  tomatis_plan_s::Levels& L = p->lvl;
  int rc;
  // --- levels: any n_fft (numpy pairwise program) ---
  // k_levels holds a block's span in LDS (f64: half as many samples); frames
  // that do not fit, and every n_fft that is not a power of two >= 256, take
  // k_levels_any
  const bool pow2 = (N & (N - 1)) == 0;
  const int cap32 = ((kLevelLds + 256) * 128) / 132 - 8;
  const int cap64 = ((kLevelLds / 2 + 256) * 128) / 132 - 8;
  L.any = !pow2 || N < 256 || N > cap32;
  if (L.any || N > cap64) {
    std::vector<int2> lv;
    std::vector<int16_t> prog;
    thost::pw_program(N, lv, prog);
    if ((int)lv.size() > kPwMaxLeaves) return TOMATIS_E_UNSUPPORTED;
    if ((rc = L.pw_leaf.upload(lv))) return rc;
    if ((rc = L.pw_prog.upload(prog))) return rc;
  }
  // --- levels blocks ---
  if (!L.any) {
    const int arr_f32 = kLevelLds + 256;  // matches k_levels<float> LDS
    const int cap = (arr_f32 * 128) / 132 - 8;
    L.nf = std::max(1, (cap - N) / hop + 1);
    const int nleaf = N >> 7;
    L.nf = std::min(L.nf, 1024 / nleaf);
    if ((rc = L.blocks.upload(level_blocks(p, L.nf)))) return rc;
  }
  // --- streaming levels: leaves of 128 samples aligned to first_start ---
  L.leaf_path = (hop % 128 == 0) && N >= 256 && N <= 4096 && (N & (N - 1)) == 0 &&
                (d.ch == 1 || d.ch == 2) && dev_opt(TOMATIS_DEV_LEVELS_LEGACY, 0) == 0;
  if (L.leaf_path) {
    std::vector<int64_t> gb(ns + 1, 0), lbase(ns + 1, 0);
    for (int s = 0; s < ns; ++s) {
      const int64_t F = p->hs[s].n_frames;
      const int64_t nblk = F > 0 ? ((F - 1) * hop + N) / 128 : 0;
      lbase[s + 1] = lbase[s] + nblk;
      gb[s + 1] = gb[s] + (nblk + 7) / 8;
      L.max_groups = std::max<int64_t>(L.max_groups, (nblk + 7) / 8);
    }
    L.n_groups = gb[ns];
    if ((rc = L.grp_base.upload(gb))) return rc;
    if ((rc = L.leaf_base.upload(lbase))) return rc;
    if ((rc = L.leaves.alloc((size_t)std::max<int64_t>(1, lbase[ns])))) return rc;
  }
  return TOMATIS_OK;
}

int build_gate_segments(tomatis_plan_s* p) {
  const TomatisPlanDesc& d = p->d;
  const int ns = p->n_streams;
  tomatis_plan_s::Gate& G = p->gate;
  int rc;
  std::vector<GateSeg> sg;
  std::vector<int32_t> first(ns), count(ns);
  auto segment = [&](int len) {
    sg.clear();
    for (int s = 0; s < ns; ++s) {
      const int64_t F = p->hs[s].n_frames;
      first[s] = (int32_t)sg.size();
      for (int64_t a = 0; a < F; a += len) {
        GateSeg g;
        g.s = s;
        g.k0 = a;
        g.nf = (int)std::min<int64_t>(len, F - a);
        sg.push_back(g);
      }
      count[s] = (int32_t)sg.size() - first[s];
    }
  };
  if (d.alpha_mode == 1) {
    segment(kASeg);
    if ((rc = G.asegs.upload(sg))) return rc;
    if ((rc = G.aseg_first.upload(first))) return rc;
    if ((rc = G.aseg_count.upload(count))) return rc;
  }
  segment(kSeg);
  if ((rc = G.segs.upload(sg))) return rc;
  G.excl = dev_opt(TOMATIS_DEV_GATE_TF, 0) == 0;
  for (int s = 0; s < ns; ++s) G.excl = G.excl && gate_exclusive(p->hs[s]);
  if ((rc = G.gsum.alloc(G.segs.n()))) return rc;
  if ((rc = G.gcarry.alloc(G.segs.n()))) return rc;
  if ((rc = G.seg_first.upload(first))) return rc;
  if ((rc = G.seg_count.upload(count))) return rc;
  const int nstate = d.up_delay_frames + 2;
  if ((rc = G.tf.alloc((size_t)G.segs.n() * nstate))) return rc;
  return G.seg_start.alloc(G.segs.n());
}

int build_tables(tomatis_plan_s* p, const float* window) {
  const TomatisPlanDesc& d = p->d;
  const int N = d.n_fft, hop = d.hop, P = p->P;
  int rc;
  std::vector<float> w(window, window + N), w2(N);
  for (int i = 0; i < N; ++i) w2[i] = w[i] * w[i];
  std::vector<float> winv(hop);
  for (int m = 0; m < hop; ++m) {
    // frames covering an interior position with hop-offset m, ascending frame order
    const int Rm = (N - m + hop - 1) / hop;
    float acc = 0.f;
    for (int j = Rm - 1; j >= 0; --j) acc = acc + w2[m + j * hop];
    const float den = (d.norm_mode == TOMATIS_NORM_MAX) ? std::max(acc, 1e-8f) : (acc + 1e-12f);
    winv[m] = 1.0f / den;
  }
  p->rmax = (N + hop - 1) / hop;
  if (!p->lds) {  // register kernels only (NR = 16 or 32)
    const int NRr = p->NR;
    // scaled-DIF output scales of the register FFT (tm_common.h): the step-2
    // table absorbs the forward NR-point DFT's, the synthesis window the
    // inverse's (whose inputs carry 1 / the forward's)
    const double* sigF = register_fft_scales(NRr, 0);
    const double* sigI = register_fft_scales(NRr, 2);
    const double* sigX = register_fft_scales(32, 1);
    // n_fft 4096 single-exchange FFT (tm_fft.h fftx128_*): wave 1 (lanes >= 64)
    // holds k2 rotated by 16 in register r: its step-2 row r twiddles
    // k2 = (r + 16) mod 32, and both its windows carry (-1)^n2
    const bool fx = p->fx, rot = fx && P == 128;
    std::vector<cf> twN((size_t)NRr * P), twP(P);
    for (int r = 0; r < NRr; ++r)
      for (int n1 = 0; n1 < P; ++n1) {
        const int k2 = (rot && n1 >= 64) ? (r + 16) % 32 : r;
        const double ang = -2.0 * M_PI * (double)((int64_t)n1 * k2 % N) / (double)N;
        twN[((size_t)(r >> 1) * P + n1) * 2 + (r & 1)] = {(float)(cos(ang) * sigF[r]),
                                                         (float)(sin(ang) * sigF[r])};
      }
    std::vector<float> winS(N);
    // single-exchange FFTs (fftx_inv / fftx128_inv): lane m's first-DFT output scale too
    for (int t = 0; t < N; ++t) {
      const double sgn = (rot && (t % P) >= 64 && ((t / P) & 1)) ? -1.0 : 1.0;
      winS[t] = (float)(sgn * (double)w[t] * sigI[t / P] *
                        (fx ? sigX[(t % P) & 31] : 1.0));
      if (rot && sgn < 0) w[t] = -w[t];  // analysis window (w2 / winv are built above)
    }
    for (int m = 0; m < P; ++m) {
      const double ang = -2.0 * M_PI * (double)m / (double)P;
      twP[m] = {(float)cos(ang), (float)sin(ang)};
    }
    if ((rc = p->tab.winS.upload(winS))) return rc;
    if ((rc = p->tab.twN.upload(twN))) return rc;
    if ((rc = p->tab.twP.upload(twP))) return rc;
  }
  if ((rc = p->tab.win.upload(w))) return rc;
  if ((rc = p->tab.win2.upload(w2))) return rc;
  if ((rc = p->tab.winv.upload(winv))) return rc;
  if (p->lds) {
    const int M = p->any.M;
    std::vector<float2> tl(M);
    for (int t = 0; t < M; ++t) {
      const double ang = -2.0 * M_PI * (double)t / (double)M;
      tl[t] = make_float2((float)cos(ang), (float)sin(ang));
    }
    if ((rc = p->any.tw.upload(tl))) return rc;
    if (p->any.blue) {
      std::vector<float2> bf, hf;
      thost::bluestein_tables(N, M, bf, hf);
      if ((rc = p->any.blue_b.upload(bf))) return rc;
      if ((rc = p->any.blue_h.upload(hf))) return rc;
    }
    if (M > kLdsMaxM && p->total_frames > 0) {
      const int64_t items = p->total_frames * ((d.ch + 1) / 2);
      // one 1024-thread block per CU keeps the chip busy; each owns two
      // M-element buffers (2 MiB at M = 131072)
      p->any.work_blocks = (int)std::min<int64_t>(items, cu_count());
      if ((rc = p->any.work.alloc((size_t)p->any.work_blocks * 2 * M))) return rc;
    }
  }
  return TOMATIS_OK;
}

// limiter chunk descriptors, output prefix, fused-limiter accounting
int build_limiter_chunks(tomatis_plan_s* p) {
  const int ns = p->n_streams;
  int rc;
  std::vector<ChunkDesc> cd;
  std::vector<int64_t> pb(ns);
  int64_t tot = 0, mx = 0;
  for (int s = 0; s < ns; ++s) {
    const TomatisStream& S = p->hs[s];
    pb[s] = tot;
    tot += S.out_len;
    const int64_t ob = S.out_begin, oe = S.out_begin + S.out_len;
    for (int c = 0; c < S.n_chunks; ++c) {
      int64_t b0 = (c == 0) ? INT64_MIN / 4 : S.chunk_first + (int64_t)(c - 1) * S.chunk_len;
      int64_t b1 = (c == S.n_chunks - 1) ? INT64_MAX / 4 : S.chunk_first + (int64_t)c * S.chunk_len;
      b0 = std::max(b0, ob);
      b1 = std::min(b1, oe);
      if (b1 <= b0) continue;
      ChunkDesc C;
      C.s = s;
      C.c = c;
      C.p0 = b0 - ob;
      C.p1 = b1 - ob;
      mx = std::max(mx, b1 - b0);
      cd.push_back(C);
    }
  }
  p->lim.max_chunk = mx;
  p->total_out = tot;
  if ((rc = p->lim.chunks.upload(cd))) return rc;
  if ((rc = p->pos_base.upload(pb))) return rc;
  // fused limiter: chunk output ranges (the per-run accounting: limiter_accounting)
  if (!p->generic && p->total_chunks > 0) {
    std::vector<int64_t> rng(2 * (size_t)p->total_chunks, 0);
    for (const ChunkDesc& C : cd) {
      rng[2 * (p->hs[C.s].chunk_base + C.c)] = C.p0;
      rng[2 * (p->hs[C.s].chunk_base + C.c) + 1] = C.p1;
    }
    if ((rc = p->lim.rng.upload(rng))) return rc;
    if ((rc = p->lim.done.alloc(p->total_chunks))) return rc;
  }
  if ((rc = limiter_accounting(p))) return rc;
  if ((rc = p->lim.err.alloc(1))) return rc;
  return p->lim.err.zero();
}

// generic-hop scratch
int build_scratch(tomatis_plan_s* p) {
  if (!p->generic || p->total_frames <= 0) return TOMATIS_OK;
  // register generic path: cf per position (L, R); any-size path: ch floats
  const size_t per = p->lds ? (size_t)std::max(2, (int)p->d.ch) : sizeof(cf) / sizeof(float);
  return p->tab.scratch.alloc((size_t)p->total_frames * p->d.n_fft * per);
}

// min-hold workspace (used when a stream's tables exceed the kernel's LDS)
int build_minhold(tomatis_plan_s* p) {
  const TomatisPlanDesc& d = p->d;
  const int ns = p->n_streams;
  tomatis_plan_s::MinHold& H = p->mh;
  int rc;
  const int nsm = 2 * (d.min_hold_frames + 1);
  std::vector<int64_t> off(ns + 1, 0), soff(ns + 1, 0);
  for (int s = 0; s < ns; ++s) {
    const int64_t F = p->hs[s].n_frames;
    const int64_t nseg = (F + mh_seg_len(F, nsm) - 1) / mh_seg_len(F, nsm);
    off[s + 1] = off[s] + (nseg * nsm > kMhLdsTf ? nseg * nsm : 0);
    soff[s + 1] = soff[s] + (((F + 15) >> 4) > kMhLdsSym ? (F + 15) >> 4 : 0);
  }
  if ((rc = H.off.upload(off))) return rc;
  if ((rc = H.soff.upload(soff))) return rc;
  if ((rc = H.tf.alloc(off[ns]))) return rc;
  if ((rc = H.cnt.alloc(off[ns]))) return rc;
  if ((rc = H.sym.alloc(soff[ns]))) return rc;
  if (ns > 0 && off[ns] == 0 && soff[ns] == 0) {  // speculative path: tables fit
    if ((rc = H.bs.alloc(ns))) return rc;
    if ((rc = H.pc.alloc((size_t)ns * kMhProbes))) return rc;
    std::vector<int64_t> goff(ns + 1, 0);
    int max_nseg = 1;
    for (int s = 0; s < ns; ++s) {
      const int64_t F = p->hs[s].n_frames;
      const int64_t nseg = F > 0 ? (F + mh_seg_len(F, nsm) - 1) / mh_seg_len(F, nsm) : 0;
      goff[s + 1] = goff[s] + kMhSlots * nseg * nsm;
      max_nseg = std::max(max_nseg, (int)nseg);
    }
    // workgroups per probe: a few segments each (one pass of the block's
    // threads over their (segment, start) pairs), at most 8
    H.parts = std::max(1, std::min(8, (max_nseg * nsm + 767) / 768));
    if (const int e = dev_opt(TOMATIS_DEV_MH_PARTS, 0)) H.parts = std::max(1, std::min(32, e));
    if ((rc = H.goff.upload(goff))) return rc;
    if ((rc = H.gtf.alloc(goff[ns]))) return rc;
    if ((rc = H.gcnt.alloc(goff[ns]))) return rc;
    if ((rc = H.arr.alloc((size_t)ns * kMhSlots))) return rc;
    if ((rc = H.arr.zero())) return rc;
  }
  return TOMATIS_OK;
}

int plan_build(tomatis_plan_s* p, const float* window) {
  int rc;
  if ((rc = p->st.upload(p->hs))) return rc;
  if ((rc = build_runs(p))) return rc;
  if ((rc = build_levels(p))) return rc;
  if ((rc = build_gate_segments(p))) return rc;
  if ((rc = build_tables(p, window))) return rc;
  if ((rc = build_limiter_chunks(p))) return rc;
  if ((rc = build_scratch(p))) return rc;
  return build_minhold(p);
}

// (lanes P, registers NR) per transform: 2048 = 128 x 16, 4096 = 128 x 32
// n_fft 2048: one wave per frame (P = 64, 32 registers, wave-local exchanges)
// unless TOMATIS_P64=0; otherwise two waves per frame (P = 128)
// register kernels: n_fft 2048 / 4096 with <= 2 channels (L + iR); every
// other n_fft or more channels: the any-size path (Stockham FFT of length M,
// Bluestein when n_fft is not a power of two)
void select_path(tomatis_plan_s* p, const TomatisStream* streams) {
  const int N = p->d.n_fft, hop = p->d.hop;
  p->lds = !(N == 2048 || N == 4096) || p->d.ch > 2 || dev_opt(TOMATIS_DEV_FORCE_LDS, 0) != 0;
  if (p->lds) {
    p->any.blue = (N & (N - 1)) != 0;
    int M = 1;
    while (M < (p->any.blue ? 2 * N - 1 : N)) M <<= 1;
    p->any.M = M;
  }
  p->P = p->lds ? 64 : ((N == 2048 && dev_opt(TOMATIS_DEV_P64, 1)) ? 64 : 128);
  p->NR = N / p->P;
  p->SH = (!p->lds && hop % p->P == 0) ? hop / p->P : 0;
  p->generic = p->lds || (p->NR == 16 ? !(p->SH == 2 || p->SH == 4 || p->SH == 8)
                                      : !(p->SH == 4 || p->SH == 8 || p->SH == 16));
  for (int i = 0; i < p->n_streams && !p->generic; ++i) {
    const TomatisStream& s = streams[i];
    if (s.n_chunks > 1 && (((s.chunk_first - s.first_start) % hop) != 0 || (s.chunk_len % hop) != 0))
      p->generic = true;  // chunk boundaries not on emit blocks: per-sample gather path
  }
  // n_fft 2048 fused kernels: the single-exchange FFT (its bin layout and scales)
  p->fx = kFftX && !p->generic && (p->P == 64 || p->P == 128) && p->NR == 32;
}

// checks every stream and assigns its frame_base / chunk_base
int validate_streams(tomatis_plan_s* p, TomatisStream* streams) {
  const int N = p->d.n_fft, hop = p->d.hop;
  int64_t fb = 0;
  int32_t cb = 0;
  for (int i = 0; i < p->n_streams; ++i) {
    TomatisStream& s = streams[i];
    bool bad = s.n < 0 || s.n_frames < 0 || s.out_len < 0 || s.n_chunks < 1 ||
               (s.n_chunks > 1 && s.chunk_len <= 0);
    if (!bad && s.n_frames > 0 && s.out_begin + s.out_len > s.first_start + (s.n_frames - 1) * hop + N)
      bad = true;  // output beyond the last frame end is never produced
    if (!bad && s.n_frames == 0 && s.out_len > 0) bad = true;
    if (bad) return TOMATIS_E_ARG;
    s.frame_base = fb;
    s.chunk_base = cb;
    fb += s.n_frames;
    cb += s.n_chunks;
  }
  p->total_frames = fb;
  p->total_chunks = cb;
  p->hs.assign(streams, streams + p->n_streams);
  return TOMATIS_OK;
}

}  // namespace

extern "C" {

int tomatis_abi_version(void) { return TOMATIS_ABI_VERSION; }

const char* tomatis_status_string(int s) {
  switch (s) {
    case TOMATIS_OK: return "ok";
    case TOMATIS_E_ARG: return "invalid argument";
    case TOMATIS_E_UNSUPPORTED: return "configuration not supported by the gfx950 kernels";
    case TOMATIS_E_HIP: return "HIP runtime error";
    case TOMATIS_E_NOMEM: return "device allocation failed";
    default: return "unknown status";
  }
}

int tomatis_plan_destroy(tomatis_plan_t p) {
  delete p;
  return TOMATIS_OK;
}

int64_t tomatis_plan_total_frames(tomatis_plan_t p) { return p ? p->total_frames : -1; }
int32_t tomatis_plan_total_chunks(tomatis_plan_t p) { return p ? p->total_chunks : -1; }
int32_t tomatis_plan_gate_segments(tomatis_plan_t p) { return p ? p->gate.segs.n() : -1; }

int tomatis_plan_create(tomatis_plan_t* out, const TomatisPlanDesc* desc, const float* window,
                        TomatisStream* streams, int32_t n_streams) {
  if (!out || !desc || !window || (!streams && n_streams > 0) || n_streams < 0) return TOMATIS_E_ARG;
  *out = nullptr;
  const TomatisPlanDesc d = *desc;
  if (d.n_fft < 2 || d.n_fft > kMaxNfft) return TOMATIS_E_UNSUPPORTED;
  if (d.ch < 1 || d.ch > kMaxCh) return TOMATIS_E_UNSUPPORTED;
  if (d.hop < 1 || d.hop > d.n_fft) return TOMATIS_E_ARG;
  if (d.up_delay_frames < 0 || d.up_delay_frames + 2 > kMaxGateStates) return TOMATIS_E_UNSUPPORTED;
  if (d.min_hold_frames < 0 || 2 * (d.min_hold_frames + 1) > 65535) return TOMATIS_E_UNSUPPORTED;
  if (d.norm_mode != TOMATIS_NORM_EPS && d.norm_mode != TOMATIS_NORM_MAX) return TOMATIS_E_ARG;
  auto* p = new (std::nothrow) tomatis_plan_s();
  if (!p) return TOMATIS_E_NOMEM;
  p->d = d;
  p->n_streams = n_streams;
  select_path(p, streams);
  int rc = validate_streams(p, streams);
  if (!rc) rc = plan_build(p, window);
  if (rc != TOMATIS_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return TOMATIS_OK;
}

int tomatis_plan_update_streams(tomatis_plan_t p, const TomatisStream* streams, void* hs) {
  if (!p || !streams) return TOMATIS_E_ARG;
  for (int i = 0; i < p->n_streams; ++i) {  // geometry is fixed at plan creation
    const TomatisStream &a = streams[i], &b = p->hs[i];
    if (a.in_off != b.in_off || a.out_off != b.out_off || a.n != b.n ||
        a.first_start != b.first_start || a.n_frames != b.n_frames ||
        a.out_begin != b.out_begin || a.out_len != b.out_len || a.chunk_first != b.chunk_first ||
        a.chunk_len != b.chunk_len || a.n_chunks != b.n_chunks)
      return TOMATIS_E_ARG;
  }
  bool excl = dev_opt(TOMATIS_DEV_GATE_TF, 0) == 0;
  for (int i = 0; i < p->n_streams; ++i) {
    TomatisStream s = streams[i];
    s.frame_base = p->hs[i].frame_base;
    s.chunk_base = p->hs[i].chunk_base;
    p->hs[i] = s;
    excl = excl && gate_exclusive(s);
  }
  p->gate.excl = excl;
  if (p->n_streams == 0) return TOMATIS_OK;
  return hipfail(hipMemcpyAsync(p->st.get(), p->hs.data(), p->hs.size() * sizeof(TomatisStream),
                                hipMemcpyHostToDevice, (hipStream_t)hs));
}

int tomatis_plan_set_option(tomatis_plan_t p, int32_t option, int64_t value) {
  if (!p) return TOMATIS_E_ARG;
  switch (option) {
    case TOMATIS_OPT_FUSE_LIMITER: p->lim.fuse_enabled = value != 0; return TOMATIS_OK;
    case TOMATIS_OPT_LIMITER_SPIN:
      if (value < 0 || value > (1 << 24)) return TOMATIS_E_ARG;
      p->lim.spin = (int)value;
      return TOMATIS_OK;
    case TOMATIS_OPT_MINHOLD_SERIAL: p->mh.serial = value != 0; return TOMATIS_OK;
    default: return TOMATIS_E_ARG;
  }
}

int tomatis_set_dev_option(int32_t key, int32_t value) {
  if (key <= 0 || key >= tshared::kDevKeys) return TOMATIS_E_ARG;
  tshared::g_dev[key] = value < 0 ? -1 : value;
  return TOMATIS_OK;
}

int32_t tomatis_get_dev_option(int32_t key) {
  if (key <= 0 || key >= tshared::kDevKeys) return -1;
  return tshared::g_dev[key];
}

}  // extern "C"
