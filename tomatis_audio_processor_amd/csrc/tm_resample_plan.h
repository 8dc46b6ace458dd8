// tm_resample_plan.h — the index arithmetic of the audio resampler
// (tm_resample.hip k_rs_poly): the tile plan, the entry point's
// argument rule and what the kernel computes per tile and per element.
//
// Host and device: plain C++ with no HIP header, so tools/resample_plan_check.cpp
// compiles it with the host compiler and checks, on the CPU, every index the
// kernel forms against the statement of tm_resample.hip's header.  The kernel
// and the entry point use these functions and no arithmetic of their own.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TM_HD __host__ __device__
#else
#define TM_HD
#endif

namespace tm_rs {

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

// K terms per output, K4 the four-chain loop's count, Ks the table's row (an odd
// number of 16-byte slots); T the largest power of two whose stage and table fit.
TM_HD inline bool rs_plan(int up, int down, int n_taps, int ch, RsPlan* pl) {
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

// ---- the entry point's arguments ------------------------------------------

enum RsArgs { kRsOk = 0, kRsArg = 1, kRsUnsupported = 2 };

TM_HD inline i64 rs_n_out(i64 len, int up, int down) { return (len * up + down - 1) / down; }
TM_HD inline i64 rs_tiles(i64 n_out, int T) { return (n_out + T - 1) / T; }

// x, taps, out: whether the pointer is non-null.  On kRsOk the plan, the output
// frames and the tiles of the launch are filled in.
inline RsArgs rs_check_args(bool x, bool taps, bool out, int64_t n_total, int64_t start,
                            int64_t len, int32_t channels, int32_t up, int32_t down,
                            int32_t n_taps, RsPlan* pl, i64* n_out, i64* tiles) {
  if (!x || !taps || !out || n_total < 0 || start < 0 || len < 1 || len > n_total - start ||
      n_taps < 1 || (n_taps & 1) == 0 || up < 1 || down < 1 || up == down || channels < 1 ||
      channels > kMaxCh)
    return kRsArg;
  for (int a = up, b = down;;) {  // gcd(up, down) == 1
    const int r = a % b;
    if (r == 0) {
      if (b != 1) return kRsArg;
      break;
    }
    a = b, b = r;
  }
  const int big = up > down ? up : down;
  if (big > kMaxRatio || (i64)down > (i64)kMaxDecim * up || n_taps > 20 * big + 1 ||
      n_total > (int64_t)1 << 48)
    return kRsUnsupported;
  if (!rs_plan((int)up, (int)down, (int)n_taps, (int)channels, pl)) return kRsUnsupported;
  *n_out = rs_n_out((i64)len, up, down);
  *tiles = rs_tiles(*n_out, pl->T);
  if (*tiles > 0x7FFFFFFF) return kRsUnsupported;
  return kRsOk;
}

// ---- the phase table --------------------------------------------------------

// tab[p Ks + v] <- taps[p + up (K - 1 - v)]: the tap index of table word i, or
// -1 where the word is a zero (v >= K, or an index past the filter)
TM_HD inline int rs_tab_src(const RsPlan& pl, int i) {
  const int p = i / pl.Ks, v = i - p * pl.Ks;
  const int m = p + pl.up * (pl.K - 1 - v);
  return (v < pl.K && m < pl.n_taps) ? m : -1;
}

TM_HD inline int rs_tab_row(const RsPlan& pl, int p) { return p * pl.Ks; }

// ---- per tile ---------------------------------------------------------------

struct RsTile {
  i64 j0;     // first output frame
  i64 c0;     // down j0 + half
  i64 ih0;    // c0 / up
  int p0;     // c0 mod up
  i64 w0;     // first word of the span in x; may lie below 0
  i64 a0;     // the 16-byte boundary at or below w0
  int shift;  // w0 - a0
  int nq;     // 16-byte pieces staged; 4 nq <= stage_words
};

TM_HD inline RsTile rs_tile(const RsPlan& pl, int ch, i64 start, i64 tile) {
  RsTile t;
  t.j0 = tile * pl.T;
  t.c0 = (i64)pl.down * t.j0 + (pl.n_taps - 1) / 2;
  t.ih0 = t.c0 / pl.up;
  t.p0 = (int)(t.c0 - t.ih0 * pl.up);
  t.w0 = (start + t.ih0 - (pl.K - 1)) * ch;
  t.a0 = t.w0 & ~(i64)3;
  t.shift = (int)(t.w0 - t.a0);
  t.nq = (t.shift + pl.W * ch + 3) / 4;
  return t;
}

// ---- per element ------------------------------------------------------------

struct RsElem {
  int o;   // output frame inside the tile
  int c;   // channel
  int ao;  // first staged frame of the element's K4 terms
  int p;   // phase
};

TM_HD inline RsElem rs_elem(const RsPlan& pl, int ch, int p0, int e) {
  RsElem r;
  r.o = e / ch, r.c = e - r.o * ch;
  const int xo = p0 + pl.down * r.o;
  r.ao = xo / pl.up, r.p = xo - r.ao * pl.up;
  return r;
}

// the stage word of the element's term v = 0; term v is v ch words further
TM_HD inline int rs_first_word(int shift, int ch, const RsElem& r) {
  return shift + r.ao * ch + r.c;
}

}  // namespace tm_rs
