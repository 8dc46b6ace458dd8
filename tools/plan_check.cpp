// plan_check.cpp -- CPU-only check of the processor plan's layout and ownership
// (csrc/tm_plan.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer
// by tests/test_plan_layout.py.  Nothing here touches a GPU: the few runtime
// calls the plan unit makes are defined below over malloc, so the "device"
// buffers a plan uploads are host memory this program reads back.
//
// For every plan (families x stream geometries x resident slots, below):
//   * runs: per stream contiguous, ascending, covering [0, n_frames) once, streams
//     in order; bit 0 of `last` exactly when kb == n_frames; a run flagged
//     kRunInterior satisfies, frame by frame, what the fused kernel's interior
//     loop assumes; gate-run plans keep every run within kGateLookbackMax;
//   * limiter accounting: chunk_need and fuse_span against a brute-force count
//     over every emitted frame with the kernel's own rule (chunk_of,
//     tm_transform.hip); chunk descriptors, chunk_rng, max_chunk, total_out and
//     pos_base against each other;
//   * coverage: level blocks, gate and alpha segments, leaf / group prefixes,
//     min-hold workspace offsets and sizes;
//   * ownership: nothing stays allocated after tomatis_plan_destroy; creation
//     with the k-th allocation failing, for every k, returns TOMATIS_E_NOMEM
//     with *out == nullptr and nothing allocated; invalid streams return
//     TOMATIS_E_ARG the same way.  LeakSanitizer checks the rest at exit.
// Exit status 0 = clean ("failures 0" on stderr).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../tomatis_audio_processor_amd/csrc/tm_plan.h"

using namespace tshared;

// ---------------------------------------------------------------------------
// fake runtime: device memory is host memory; allocations are counted and the
// g_fail_at-th (1-based, 0: none) fails
// ---------------------------------------------------------------------------
namespace {
long g_live = 0, g_allocs = 0, g_fail_at = 0;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
  ++g_allocs;
  *p = (g_fail_at && g_allocs == g_fail_at) ? nullptr : malloc(n ? n : 1);
  if (!*p) return hipErrorOutOfMemory;
  ++g_live;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) --g_live;
  free(p);
  return hipSuccess;
}
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) {
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
  memcpy(d, s, n);
  return hipSuccess;
}
hipError_t hipMemset(void* d, int v, size_t n) {
  memset(d, v, n);
  return hipSuccess;
}
hipError_t hipGetDevice(int* d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) {
  *v = a == hipDeviceAttributeMultiprocessorCount ? 256 : 0;
  return hipSuccess;
}
}  // extern "C"

namespace tshared {
// the device units' side of the plan: fixed answers
int transform_slots_per_cu(int P, int) { return 512 / P; }
const double* register_fft_scales(int, int) {
  static const std::vector<double> ones(64, 1.0);
  return ones.data();
}
}  // namespace tshared

namespace {

int g_fail = 0;
long g_plans = 0, g_nomem = 0;
std::string g_ctx;

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (g_fail++ < 20) {                                 \
        fprintf(stderr, "FAIL [%s] %s: ", g_ctx.c_str(), #cond); \
        fprintf(stderr, __VA_ARGS__);                      \
        fprintf(stderr, "\n");                             \
      }                                                    \
    }                                                      \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int64_t in(int64_t lo, int64_t hi) { return lo + (int64_t)(next() % (uint64_t)(hi - lo + 1)); }
};

int64_t pymod(int64_t a, int64_t b) { return ((a % b) + b) % b; }
int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }  // a >= 0

TomatisStream blank_stream() {
  TomatisStream s;
  memset(&s, 0, sizeof(s));
  s.n_chunks = 1;
  s.chunk_len = 1;
  s.in_scale = s.out_scale = 1.f;
  s.on_bits = 0x3f000000u;   // exclusive predicates: on >= 0.5, off <= 0.25
  s.off_bits = 0x3e800000u;
  return s;
}

// a stream of N samples as engine.GatePipeline lays it (dsp.std_schedule,
// dsp.std_flush_bounds)
TomatisStream std_stream(int64_t N, int n_fft, int hop, int64_t flush = 240000) {
  const int64_t pad = n_fft / 2;
  const int64_t pad_end = pymod(hop - pymod(N - n_fft, hop), hop);
  const int64_t total = pad + N + pad_end;
  const int64_t F = total >= n_fft ? (total - n_fft) / hop + 1 : 0, s0 = -pad;
  std::vector<int64_t> b{s0};
  if (F) {
    const int64_t k1 = std::max<int64_t>(0, cdiv(flush + n_fft, hop) - 1);
    if (k1 <= F - 1) {
      int64_t pos = s0 + (k1 + 1) * hop - n_fft;
      const int64_t step = cdiv(flush, hop);
      for (int64_t k = k1; k <= F - 1; k += step, pos += step * hop) b.push_back(pos);
    }
    const int64_t end = s0 + (F - 1) * hop + n_fft;
    if (end > b.back()) b.push_back(end);
  }
  TomatisStream s = blank_stream();
  s.n = N;
  s.first_start = s0;
  s.n_frames = F;
  s.out_len = F ? std::min(N, s0 + (F - 1) * hop + n_fft) : 0;
  s.n_chunks = (int32_t)std::max<size_t>(1, b.size() - 1);
  s.chunk_first = b.size() > 2 ? b[1] : 0;
  s.chunk_len = b.size() > 3 ? b[2] - b[1] : std::max<int64_t>(1, b.size() > 2 ? b.back() - b[1] : 1);
  return s;
}

// a stream as engine.AdaptivePipeline lays it: the frames that start inside
// the input, one limiter chunk
TomatisStream adaptive_stream(int64_t N, int n_fft, int hop) {
  const int64_t pad = n_fft / 2, k0 = cdiv(pad, hop);
  TomatisStream s = blank_stream();
  s.n = N;
  s.first_start = k0 * hop - pad;
  s.n_frames = N > s.first_start ? cdiv(N - s.first_start, hop) : 0;
  s.out_len = s.n_frames ? N : 0;
  return s;
}

// a time shard: frames [k0, k0 + F) of a long standard stream, output from the
// shard's first hop-aligned position on
TomatisStream shard_stream(int64_t N, int n_fft, int hop, int64_t k0, int64_t F) {
  TomatisStream s = std_stream(N, n_fft, hop);
  s.first_start += k0 * hop;
  s.n_frames = F;
  s.out_begin = s.first_start + n_fft - hop;
  s.out_len = (F - 1) * hop - (n_fft - hop) + hop;
  s.n_chunks = 3;
  s.chunk_first = s.first_start + 40 * (int64_t)hop;
  s.chunk_len = 64 * (int64_t)hop;
  return s;
}

// a random stream valid under tomatis_plan_create's checks
TomatisStream random_stream(Rng& r, int n_fft, int hop, bool on_grid) {
  TomatisStream s = blank_stream();
  s.n = r.in(0, 400000);
  s.first_start = r.in(-n_fft, n_fft);
  s.n_frames = r.next() % 8 == 0 ? 0 : r.in(1, 900);
  if (s.n_frames > 0) {
    const int64_t end = s.first_start + (s.n_frames - 1) * hop + n_fft;
    s.out_begin = r.in(s.first_start - hop, s.first_start + 3 * (int64_t)hop);
    s.out_len = r.in(0, std::max<int64_t>(0, end - s.out_begin));
  }
  s.n_chunks = (int32_t)r.in(1, 5);
  if (s.n_chunks > 1) {
    s.chunk_len = hop * r.in(1, 200) + (on_grid ? 0 : r.in(1, hop - 1));
    s.chunk_first = s.first_start + hop * r.in(1, 300);
  }
  return s;
}

struct Family {
  std::string name;
  TomatisPlanDesc d;
  std::vector<TomatisStream> st;
  bool expect_generic = false;  // chunk boundaries off the hop grid
  int64_t interior = -1;        // frames expected in interior runs (-1: not pinned)
};

TomatisPlanDesc desc(int n_fft, int hop, int ch, int alpha_mode = 0, int xfade = 0, int min_hold = 0) {
  TomatisPlanDesc d;
  memset(&d, 0, sizeof(d));
  d.n_fft = n_fft;
  d.hop = hop;
  d.ch = ch;
  d.norm_mode = alpha_mode == 2 ? TOMATIS_NORM_MAX : TOMATIS_NORM_EPS;
  d.up_delay_frames = 3;
  d.min_hold_frames = min_hold;
  d.xfade_frames = xfade;
  d.alpha_mode = alpha_mode;
  return d;
}

// the kernel's chunk of an output position (chunk_of, tm_transform.hip)
int chunk_of(int64_t p, const TomatisStream& S) {
  if (S.n_chunks <= 1 || p < S.chunk_first) return 0;
  return (int)std::min<int64_t>(1 + (p - S.chunk_first) / S.chunk_len, S.n_chunks - 1);
}

template <typename Seg>
void check_cover(const char* what, const Seg* seg, size_t n, const std::vector<TomatisStream>& st,
                 int max_nf, const int32_t* first, const int32_t* count) {
  size_t i = 0;
  for (size_t s = 0; s < st.size(); ++s) {
    const size_t i0 = i;
    int64_t k = 0;
    while (i < n && seg[i].s == (int32_t)s) {
      CHECK(seg[i].k0 == k && seg[i].nf >= 1 && seg[i].nf <= max_nf, "%s %zu of stream %zu", what, i, s);
      k += seg[i].nf;
      ++i;
    }
    CHECK(k == st[s].n_frames, "%s cover %lld of %lld frames of stream %zu", what, (long long)k,
          (long long)st[s].n_frames, s);
    if (first) CHECK(first[s] == (int32_t)i0 && count[s] == (int32_t)(i - i0), "%s index of stream %zu", what, s);
  }
  CHECK(i == n, "%s: %zu items, %zu in stream order", what, n, i);
}

void check_plan(const Family& f, const tomatis_plan_s* p) {
  const TomatisPlanDesc& d = f.d;
  const int N = d.n_fft, hop = d.hop, ns = (int)f.st.size();
  const std::vector<TomatisStream>& st = p->hs;
  CHECK((int)st.size() == ns && p->n_streams == ns, "stream count");
  CHECK(ns == 0 || memcmp(p->st.get(), st.data(), ns * sizeof(TomatisStream)) == 0, "stream table upload");
  CHECK(p->generic || !f.expect_generic, "off-grid chunk boundaries must take the generic path");
  // ---- runs ----
  const Run* runs = p->runs.get();
  const int nr = p->runs.n();
  CHECK((size_t)nr == p->runs.size() && (size_t)nr == p->hruns.size(), "run count");
  CHECK(nr == 0 || memcmp(runs, p->hruns.data(), nr * sizeof(Run)) == 0, "run upload");
  const int rmax = (N + hop - 1) / hop;
  CHECK(p->rmax == rmax, "rmax %d", p->rmax);
  const bool gate_runs = d.alpha_mode == 0 && N == 2048 && p->P == 64 && !p->generic;
  {
    int i = 0;
    for (int s = 0; s < ns; ++s) {
      const TomatisStream& S = st[s];
      int64_t k = 0;
      for (; i < nr && runs[i].s == s; ++i) {
        const Run& R = runs[i];
        CHECK(R.ka == k && R.kb > R.ka && R.kb <= S.n_frames, "run %d [%lld, %lld)", i, (long long)R.ka,
              (long long)R.kb);
        CHECK(((R.last & 1) != 0) == (R.kb == S.n_frames), "run %d last flag %d", i, R.last);
        CHECK((R.last & ~(1 | kRunInterior)) == 0, "run %d flags %d", i, R.last);
        if (gate_runs) CHECK(R.kb - R.ka <= kGateLookbackMax, "run %d: %lld frames", i, (long long)(R.kb - R.ka));
        if (R.last & kRunInterior) {
          CHECK(!p->generic && p->P == 64, "interior run %d on a plan without the interior loop", i);
          CHECK(R.kb <= S.n_frames - 1, "interior run %d holds the last frame", i);
          for (int64_t j = std::max<int64_t>(0, R.ka - (rmax - 1)); j < R.kb; ++j) {
            const int64_t sj = S.first_start + j * hop;
            CHECK(sj >= 0 && sj + N <= S.n, "interior run %d: frame %lld loads outside the input", i, (long long)j);
            if (j >= R.ka)
              CHECK(sj >= S.out_begin && sj + hop <= S.out_begin + S.out_len,
                    "interior run %d: frame %lld emits outside the output", i, (long long)j);
          }
        }
        k = R.kb;
      }
      CHECK(k == S.n_frames, "runs cover %lld of %lld frames of stream %d", (long long)k, (long long)S.n_frames, s);
    }
    CHECK(i == nr, "%d runs, %d in stream order", nr, i);
    int64_t fast = 0;
    for (int j = 0; j < nr; ++j) fast += (runs[j].last & kRunInterior) ? runs[j].kb - runs[j].ka : 0;
    if (f.interior >= 0 && dev_opt(TOMATIS_DEV_FAST_LOOP, 1))
      CHECK(fast == f.interior, "%lld frames in interior runs, expected %lld", (long long)fast, (long long)f.interior);
  }
  // ---- limiter chunk descriptors, output prefix ----
  const ChunkDesc* cd = p->lim.chunks.get();
  const int ncd = p->lim.chunks.n();
  CHECK((size_t)ncd == p->lim.chunks.size(), "chunk descriptor count");
  {
    int i = 0;
    int64_t tot = 0, mx = 0;
    for (int s = 0; s < ns; ++s) {
      CHECK(p->pos_base.get()[s] == tot, "pos_base[%d]", s);
      tot += st[s].out_len;
      int64_t pos = 0;
      int c_prev = -1;
      for (; i < ncd && cd[i].s == s; ++i) {
        CHECK(cd[i].c > c_prev && cd[i].c < st[s].n_chunks && cd[i].p0 == pos && cd[i].p1 > cd[i].p0,
              "chunk descriptor %d", i);
        for (int64_t q : {cd[i].p0, cd[i].p1 - 1})
          CHECK(chunk_of(q + st[s].out_begin, st[s]) == cd[i].c, "chunk descriptor %d vs chunk_of", i);
        pos = cd[i].p1;
        c_prev = cd[i].c;
        mx = std::max(mx, cd[i].p1 - cd[i].p0);
      }
      CHECK(pos == st[s].out_len, "chunk descriptors cover %lld of %lld samples of stream %d", (long long)pos,
            (long long)st[s].out_len, s);
    }
    CHECK(i == ncd, "%d chunk descriptors, %d in stream order", ncd, i);
    CHECK(p->total_out == tot && p->lim.max_chunk == mx, "total_out / max_chunk");
  }
  int tc = 0;
  int64_t tfr = 0;
  for (int s = 0; s < ns; ++s) {
    CHECK(st[s].chunk_base == tc && st[s].frame_base == tfr, "bases of stream %d", s);
    tc += st[s].n_chunks;
    tfr += st[s].n_frames;
  }
  CHECK(p->total_chunks == tc && p->total_frames == tfr, "totals");
  CHECK(p->lim.err.size() == 1 && *p->lim.err.get() == 0, "error word");
  // ---- fused-limiter accounting, by brute force over the emitted frames ----
  if (!p->generic && tc > 0) {
    CHECK(p->lim.rng.size() == 2 * (size_t)tc && p->lim.done.size() == (size_t)tc &&
              p->lim.need.size() == (size_t)tc, "fused limiter buffer sizes");
    std::vector<int64_t> rng(2 * (size_t)tc, 0);
    for (int i = 0; i < ncd; ++i) {
      rng[2 * (st[cd[i].s].chunk_base + cd[i].c)] = cd[i].p0;
      rng[2 * (st[cd[i].s].chunk_base + cd[i].c) + 1] = cd[i].p1;
    }
    CHECK(memcmp(rng.data(), p->lim.rng.get(), rng.size() * 8) == 0, "chunk_rng vs descriptors");
    std::vector<uint32_t> need(tc, 0);
    std::vector<int> first(tc, -1), last(tc, -1);
    for (int i = 0; i < nr; ++i) {
      const TomatisStream& S = st[runs[i].s];
      std::set<int> cs;
      for (int64_t k = runs[i].ka; k < runs[i].kb; ++k) cs.insert(chunk_of(S.first_start + k * hop, S));
      for (int c : cs) {
        const int g = S.chunk_base + c;
        need[g] += p->P / 64;
        if (first[g] < 0) first[g] = i;
        last[g] = i;
      }
    }
    int span = 0;
    for (int g = 0; g < tc; ++g) {
      CHECK(p->lim.need.get()[g] == need[g], "chunk_need[%d] = %u, %u by frames", g, p->lim.need.get()[g], need[g]);
      if (first[g] >= 0) span = std::max(span, last[g] - first[g] + 1);
    }
    CHECK(p->lim.fuse_span == span, "fuse_span %d, %d by frames", p->lim.fuse_span, span);
  } else {
    CHECK(!p->lim.need.get() && !p->lim.done.get() && !p->lim.rng.get() && p->lim.fuse_span == 0,
          "no fused-limiter state on this path");
  }
  // ---- levels ----
  if (!p->lvl.any) {
    CHECK(p->lvl.nf >= 1, "level block frames %d", p->lvl.nf);
    check_cover("level block", p->lvl.blocks.get(), p->lvl.blocks.size(), st, p->lvl.nf, nullptr, nullptr);
  } else {
    CHECK(p->lvl.blocks.size() == 0 && p->lvl.pw_leaf.n() > 0 && p->lvl.pw_prog.n() > 0, "pairwise program");
  }
  CHECK(p->lvl.pw_leaf.size() == (size_t)p->lvl.pw_leaf.n() && p->lvl.pw_prog.size() == (size_t)p->lvl.pw_prog.n(),
        "pairwise program upload");
  if (p->lvl.leaf_path) {
    int64_t lb = 0, gb = 0, mg = 0;
    for (int s = 0; s < ns; ++s) {
      CHECK(p->lvl.leaf_base.get()[s] == lb && p->lvl.grp_base.get()[s] == gb, "leaf / group base of stream %d", s);
      const int64_t F = st[s].n_frames, nblk = F > 0 ? ((F - 1) * hop + N) / 128 : 0;
      lb += nblk;
      gb += (nblk + 7) / 8;
      mg = std::max(mg, (nblk + 7) / 8);
    }
    CHECK(p->lvl.leaf_base.size() == (size_t)ns + 1 && p->lvl.leaf_base.get()[ns] == lb, "leaf total");
    CHECK(p->lvl.grp_base.size() == (size_t)ns + 1 && p->lvl.grp_base.get()[ns] == gb, "group total");
    CHECK(p->lvl.n_groups == gb && p->lvl.max_groups == mg, "group counts");
    CHECK(p->lvl.leaves.size() == (size_t)std::max<int64_t>(1, lb), "leaf buffer");
  }
  // ---- gate and alpha segments ----
  const tomatis_plan_s::Gate& G = p->gate;
  CHECK(G.segs.size() == (size_t)G.segs.n() && G.gsum.size() == G.segs.size() && G.gcarry.size() == G.segs.size() &&
            G.seg_start.size() == G.segs.size() && G.tf.size() == G.segs.size() * (d.up_delay_frames + 2),
        "gate buffer sizes");
  CHECK(G.seg_first.size() == (size_t)ns && G.seg_count.size() == (size_t)ns, "gate index sizes");
  check_cover("gate segment", G.segs.get(), G.segs.size(), st, kSeg, G.seg_first.get(), G.seg_count.get());
  if (d.alpha_mode == 1) {
    CHECK(G.asegs.size() == (size_t)G.asegs.n() && G.aseg_first.size() == (size_t)ns, "alpha buffer sizes");
    check_cover("alpha segment", G.asegs.get(), G.asegs.size(), st, kASeg, G.aseg_first.get(), G.aseg_count.get());
  } else {
    CHECK(G.asegs.size() == 0 && G.asegs.n() == 0, "alpha segments without a cross-fade");
  }
  CHECK(G.excl, "exclusive gate predicates");
  // ---- min-hold workspace ----
  {
    const tomatis_plan_s::MinHold& H = p->mh;
    const int nsm = 2 * (d.min_hold_frames + 1);
    int64_t off = 0, soff = 0, goff = 0;
    CHECK(H.off.size() == (size_t)ns + 1 && H.soff.size() == (size_t)ns + 1, "min-hold offset tables");
    for (int s = 0; s <= ns; ++s) {
      CHECK(H.off.get()[s] == off && H.soff.get()[s] == soff, "min-hold offsets of stream %d", s);
      if (s == ns) break;
      const int64_t F = st[s].n_frames, seg = mh_seg_len(F, nsm), nseg = (F + seg - 1) / seg;
      CHECK(seg >= 256 && seg % 16 == 0 && nseg <= 4096, "min-hold segments of stream %d", s);
      off += nseg * nsm > kMhLdsTf ? nseg * nsm : 0;
      soff += ((F + 15) >> 4) > kMhLdsSym ? (F + 15) >> 4 : 0;
      goff += kMhSlots * nseg * nsm;
    }
    CHECK(H.tf.size() == (size_t)off && H.cnt.size() == (size_t)off && H.sym.size() == (size_t)soff,
          "min-hold workspace sizes");
    if (ns > 0 && off == 0 && soff == 0) {
      CHECK(H.bs.size() == (size_t)ns && H.pc.size() == (size_t)ns * kMhProbes && H.goff.size() == (size_t)ns + 1 &&
                H.goff.get()[ns] == goff && H.gtf.size() == (size_t)goff && H.gcnt.size() == (size_t)goff &&
                H.arr.size() == (size_t)ns * kMhSlots && H.parts >= 1 && H.parts <= 8,
            "speculative min-hold state");
      for (size_t i = 0; i < H.arr.size(); ++i) CHECK(H.arr.get()[i] == 0, "arrival counter %zu", i);
    } else {
      CHECK(!H.bs.get() && !H.gtf.get(), "speculative min-hold state on a spilling plan");
    }
  }
  // ---- tables and scratch ----
  CHECK(p->tab.win.size() == (size_t)N && p->tab.win2.size() == (size_t)N && p->tab.winv.size() == (size_t)hop,
        "window tables");
  if (p->lds) {
    CHECK(p->generic && p->any.M >= N && (p->any.M & (p->any.M - 1)) == 0 && p->any.tw.size() == (size_t)p->any.M,
          "any-size FFT length %d", p->any.M);
    CHECK(p->any.blue == ((N & (N - 1)) != 0) && p->any.blue_b.size() == (p->any.blue ? (size_t)N : 0) &&
              p->any.blue_h.size() == (p->any.blue ? (size_t)p->any.M : 0), "Bluestein tables");
    const bool glb = p->any.M > kLdsMaxM && tfr > 0;
    CHECK(p->any.work.size() == (glb ? (size_t)p->any.work_blocks * 2 * p->any.M : 0) &&
              (!glb || (p->any.work_blocks >= 1 && p->any.work_blocks <= 256)), "per-block work buffers");
  } else {
    CHECK(p->tab.winS.size() == (size_t)N && p->tab.twN.size() == (size_t)N && p->tab.twP.size() == (size_t)p->P,
          "register FFT tables");
  }
  const size_t per = p->lds ? (size_t)std::max(2, (int)d.ch) : 2;
  CHECK(p->tab.scratch.size() == (p->generic ? (size_t)tfr * N * per : 0), "generic-hop scratch");
}

// creates the plan (streams are copied: create fills their bases); returns rc
int create(const Family& f, tomatis_plan_t* out) {
  std::vector<TomatisStream> st = f.st;
  static std::vector<float> win;
  win.assign(f.d.n_fft, 0.5f);
  return tomatis_plan_create(out, &f.d, win.data(), st.data(), (int32_t)st.size());
}

// one family under the current dev options: layout, then every allocation failing
void run_family(const Family& f, const char* opts, bool nomem_sweep) {
  g_ctx = f.name + " " + opts;
  tomatis_plan_t p = nullptr;
  g_fail_at = 0;
  g_allocs = 0;
  const int rc = create(f, &p);
  const long n_alloc = g_allocs;
  CHECK(rc == TOMATIS_OK && p, "create: %s", tomatis_status_string(rc));
  if (!p) return;
  ++g_plans;
  check_plan(f, p);
  CHECK(tomatis_plan_total_frames(p) == p->total_frames && tomatis_plan_gate_segments(p) == p->gate.segs.n(),
        "plan getters");
  CHECK(tomatis_plan_destroy(p) == TOMATIS_OK && g_live == 0, "%ld allocations alive after destroy", g_live);
  for (long k = 1; nomem_sweep && k <= n_alloc; ++k) {
    g_fail_at = k;
    g_allocs = 0;
    p = reinterpret_cast<tomatis_plan_t>(&g_fail);
    const int rk = create(f, &p);
    CHECK(rk == TOMATIS_E_NOMEM && p == nullptr && g_live == 0,
          "allocation %ld of %ld failing: rc %d, %ld alive", k, n_alloc, rk, g_live);
    ++g_nomem;
  }
  g_fail_at = 0;
}

void bad_streams(const Family& base) {
  g_ctx = "invalid streams";
  const TomatisStream ok = std_stream(40000, base.d.n_fft, base.d.hop);
  auto expect_arg = [&](const char* what, TomatisStream s) {
    Family f = base;
    f.st = {ok, s};
    tomatis_plan_t p = reinterpret_cast<tomatis_plan_t>(&g_fail);
    const int rc = create(f, &p);
    CHECK(rc == TOMATIS_E_ARG && p == nullptr && g_live == 0, "%s: rc %d, %ld alive", what, rc, g_live);
  };
  TomatisStream s = ok;
  s.n = -1;
  expect_arg("n < 0", s);
  s = ok, s.n_frames = -1;
  expect_arg("n_frames < 0", s);
  s = ok, s.out_len = -1;
  expect_arg("out_len < 0", s);
  s = ok, s.n_chunks = 0;
  expect_arg("n_chunks < 1", s);
  s = ok, s.n_chunks = 2, s.chunk_len = 0;
  expect_arg("chunk_len <= 0", s);
  s = ok, s.out_len = s.first_start + (s.n_frames - 1) * base.d.hop + base.d.n_fft - s.out_begin + 1;
  expect_arg("output beyond the last frame", s);
  s = ok, s.n_frames = 0, s.out_len = 1;
  expect_arg("output without a frame", s);
}

std::vector<Family> families() {
  std::vector<Family> fs;
  // interior-eligible frames of a 2048-point standard stream of hop x m
  // samples: m - 7 at hop 512, m - 15 at hop 256; 0, 1, 47, 48 and 49 of them
  // (under 48 the stream has no interior run)
  const int eligible[5] = {0, 1, 47, 48, 49};
  for (int hop : {512, 256}) {
    Family f{"std 2048/" + std::to_string(hop), desc(2048, hop, 2), {}};
    for (int e : eligible) f.st.push_back(std_stream((int64_t)hop * (e + (hop == 512 ? 7 : 15)), 2048, hop));
    f.st.push_back(std_stream(750001, 2048, hop));  // four limiter chunks
    fs.push_back(f);
    for (size_t i = 0; i < f.st.size(); ++i) {  // and each alone
      fs.push_back(Family{f.name + " stream " + std::to_string(i), f.d, {f.st[i]}});
      if (i < 5) fs.back().interior = eligible[i] >= 48 ? eligible[i] : 0;
    }
  }
  // ragged batch of three odd lengths; no stream; a stream without a frame
  fs.push_back(Family{"std 2048/512 ragged", desc(2048, 512, 2),
                      {std_stream(480001, 2048, 512), std_stream(77777, 2048, 512), std_stream(1234567, 2048, 512)}});
  fs.push_back(Family{"std 2048/512 mono empty", desc(2048, 512, 1), {}});
  fs.push_back(Family{"std 2048/512 tiny", desc(2048, 512, 1), {std_stream(0, 2048, 512), std_stream(5, 2048, 512)}});
  // kGateLookbackMax cap: with one resident slot, more than 4096 frames
  fs.push_back(Family{"std 2048/512 long", desc(2048, 512, 2), {std_stream(512 * 5000 + 17, 2048, 512)}});
  // chunks of 7 and 5 frames: every run crosses several boundaries, and run ends
  // fall on every offset from one
  {
    Family f{"std 2048/512 short chunks", desc(2048, 512, 2), {std_stream(512 * 3000, 2048, 512), std_stream(512 * 777, 2048, 512)}};
    for (int i = 0; i < 2; ++i) {
      f.st[i].chunk_first = f.st[i].first_start + (50 + i) * 512;
      f.st[i].chunk_len = (7 - 2 * i) * 512;
      f.st[i].n_chunks = 300 - 200 * i;
    }
    fs.push_back(f);
  }
  // time shard: out_begin > 0
  fs.push_back(Family{"std 2048/512 shard", desc(2048, 512, 2),
                      {shard_stream(4000000, 2048, 512, 3000, 700), shard_stream(4000000, 2048, 512, 3600, 300)}});
  for (int xf : {0, 5})
    fs.push_back(Family{"xfade 4096/1024 xf " + std::to_string(xf), desc(4096, 1024, 2, 1, xf),
                        {std_stream(750001, 4096, 1024), std_stream(99999, 4096, 1024)}});
  fs.push_back(Family{"std 4096/2048", desc(4096, 2048, 2), {std_stream(750001, 4096, 2048), std_stream(4096, 4096, 2048)}});
  fs.push_back(Family{"adaptive 2048/512", desc(2048, 512, 2, 2, 4, 6),
                      {adaptive_stream(480000, 2048, 512), adaptive_stream(77777, 2048, 512), adaptive_stream(3, 2048, 512)}});
  // (tables past the kernel's LDS: the HBM workspace instead of the speculative state)
  fs.push_back(Family{"adaptive 2048/512 spill", desc(2048, 512, 2, 2, 4, 6),
                      {adaptive_stream(512 * 200000, 2048, 512), adaptive_stream(480000, 2048, 512)}});
  fs.push_back(Family{"generic hop 2048/300", desc(2048, 300, 2), {std_stream(750001, 2048, 300), std_stream(33333, 2048, 300)}});
  {
    Family f{"off-grid chunks 2048/512", desc(2048, 512, 2), {std_stream(750001, 2048, 512)}, true};
    f.st[0].chunk_first += 7;
    fs.push_back(f);
  }
  fs.push_back(Family{"any-size 1000/250 x3", desc(1000, 250, 3), {std_stream(48000, 1000, 250), std_stream(999, 1000, 250)}});
  fs.push_back(Family{"any-size 20000/5000", desc(20000, 5000, 2), {std_stream(100000, 20000, 5000)}});
  // seeded random geometries, on and off the hop grid
  Rng r{20240917};
  for (int i = 0; i < 40; ++i) {
    const int nf = i % 4 == 3 ? 4096 : 2048, hop = i % 4 == 3 ? 1024 : (i % 4 == 2 ? 300 : (i % 4 ? 256 : 512));
    Family f{"random " + std::to_string(i), desc(nf, hop, 1 + i % 2, i % 4 == 3 ? 1 : 0, 5), {}, false};
    const bool on_grid = i % 5 != 4;
    for (int s = 0, n = (int)r.in(1, 4); s < n; ++s) f.st.push_back(random_stream(r, nf, hop, on_grid));
    if (!on_grid) {
      f.expect_generic = false;
      for (const TomatisStream& s : f.st) f.expect_generic |= s.n_chunks > 1;
    }
    fs.push_back(f);
  }
  return fs;
}

}  // namespace

int main() {
  const std::vector<Family> fs = families();
  // resident slots: 1 and 8 (many rounds, the kGateLookbackMax cap) and the
  // device's own (256 CUs x the slots per CU above)
  for (int slots : {1, 8, 0}) {
    tomatis_set_dev_option(TOMATIS_DEV_SLOTS, slots);
    const std::string o = "slots " + std::to_string(slots);
    for (const Family& f : fs) run_family(f, o.c_str(), slots == 0 || f.st.size() <= 1);
  }
  // development options on the first shape
  struct Opt { int key, value; };
  for (Opt o : {Opt{TOMATIS_DEV_RUN_FRAMES, 48}, Opt{TOMATIS_DEV_RUN_FRAMES, 131}, Opt{TOMATIS_DEV_RUN_FRAMES, 1000},
                Opt{TOMATIS_DEV_FAST_LOOP, 0}, Opt{TOMATIS_DEV_RUN_ROUNDS, 2}}) {
    tomatis_set_dev_option(o.key, o.value);
    const std::string s = "option " + std::to_string(o.key) + " = " + std::to_string(o.value);
    for (int slots : {8, 0}) {
      tomatis_set_dev_option(TOMATIS_DEV_SLOTS, slots);
      run_family(fs[0], s.c_str(), false);
    }
    tomatis_set_dev_option(o.key, -1);
    CHECK(tomatis_get_dev_option(o.key) == -1, "dev option reset");
  }
  tomatis_set_dev_option(TOMATIS_DEV_SLOTS, 0);
  bad_streams(fs[0]);
  CHECK(tomatis_abi_version() == TOMATIS_ABI_VERSION, "ABI version");
  fprintf(stderr, "plans %ld, failed-allocation creations %ld, failures %d\n", g_plans, g_nomem, g_fail);
  return g_fail ? 1 : 0;
}
