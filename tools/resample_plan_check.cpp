// resample_plan_check.cpp -- CPU-only check of the audio resampler's index
// arithmetic (csrc/tm_resample_plan.h, used by tm_resample.hip k_rs_poly and
// tomatis_resample_poly), built with AddressSanitizer and
// UndefinedBehaviorSanitizer by tests/test_resample_plan.py.  No HIP, no GPU.
//
// 1. The whole supported domain: every reduced (up, down) with max <= 512,
//    down <= 8 up, up != down, n_taps = 20 max + 1, 1 to 8 channels.  A plan
//    exists; stage and table fit 64 KiB; T is a power of two <= 1024 and 2 T
//    would not fit; Ks >= K4, Ks % 4 == 0, Ks / 4 odd; and with the extreme values
//    (they are monotone in the output frame) for every tile-start phase and every
//    shift: staging stays inside `stage`, the highest stage word an element reads
//    is below shift + W ch, the highest table word below tab_words, and every
//    16-byte table read starts on a 16-byte boundary of the LDS.
// 2. Element by element, for a list of plans (custom tap counts among them) and
//    the tiles 0, 1, the last of a 3.5-tile range and the last of a range just
//    under the 2^31 - 1 tile limit: the LDS is emulated as an exactly sized heap
//    array of word origins (which word of x, a zero, or "not staged"), the
//    kernel's reads are replayed through the header's functions, and the set of
//    (tap index, input frame) pairs each element consumes must equal the
//    statement's, formed here in 64-bit integers from the output frame alone:
//      c = down j + half, phase c mod up, frame c / up,
//      terms (phase + up t, frame - t), t < K, tap < n_taps, 0 <= frame < len.
//    Every padded term (v >= K) must meet a zero tap and every word read must
//    have been staged for that tile.
// 3. The argument rule of the entry point against the expectations of
//    tests/test_gpu_resample.py::test_entry_point_guards.
// Prints "plan up down n_taps ch T W stage_words tab_words" per listed plan and
// ends with "failures N" on stdout; details of a failure go to stderr.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../tomatis_audio_processor_amd/csrc/tm_resample_plan.h"

using namespace tm_rs;

namespace {

long g_fail = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_fail <= 40) {                       \
        fprintf(stderr, "FAIL %s: ", #cond);      \
        fprintf(stderr, __VA_ARGS__);             \
        fprintf(stderr, "\n");                    \
      }                                           \
    }                                             \
  } while (0)

int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// ---------------------------------------------------------------------------
// 1. the whole domain
// ---------------------------------------------------------------------------
long whole_domain() {
  long plans = 0;
  for (int up = 1; up <= kMaxRatio; ++up)
    for (int down = 1; down <= kMaxRatio; ++down) {
      if (up == down || gcd(up, down) != 1 || down > kMaxDecim * up) continue;
      const int n_taps = 20 * (up > down ? up : down) + 1;
      for (int ch = 1; ch <= kMaxCh; ++ch) {
        RsPlan pl;
        const bool ok = rs_plan(up, down, n_taps, ch, &pl);
        CHECK(ok, "no plan %d/%d ch %d", up, down, ch);
        if (!ok) continue;
        ++plans;
        const long before = g_fail;
        CHECK(4 * ((i64)pl.stage_words + pl.tab_words) <= 65536, "LDS");
        CHECK(pl.T >= 1 && pl.T <= 1024 && (pl.T & (pl.T - 1)) == 0, "T %d", pl.T);
        if (pl.T < 1024) {  // the next size does not fit
          const i64 W2 = ((i64)up - 1 + (i64)down * (2 * pl.T - 1)) / up + pl.K4;
          const i64 st2 = (3 + W2 * ch + 3) / 4 * 4;
          CHECK(4 * (st2 + pl.tab_words) > 65536, "2 T fits");
        }
        CHECK(pl.K == (n_taps + up - 1) / up && pl.K4 >= pl.K && pl.K4 < pl.K + 4 &&
                  pl.K4 % 4 == 0, "K %d K4 %d", pl.K, pl.K4);
        CHECK(pl.Ks >= pl.K4 && pl.Ks % 4 == 0 && (pl.Ks / 4) % 2 == 1, "Ks %d", pl.Ks);
        CHECK(pl.tab_words == up * pl.Ks && pl.stage_words % 4 == 0, "words");
        // the table: the last row's last read, and the alignment of every row
        CHECK(rs_tab_row(pl, up - 1) + pl.K4 - 1 < pl.tab_words, "table read");
        for (int p = 0; p < up; ++p)
          for (int i = 0; i < pl.K4 / 4; ++i)
            CHECK((pl.stage_words + rs_tab_row(pl, p) + 4 * i) % 4 == 0, "table alignment");
        // the stage: the tile's last element at every start phase and shift
        const int e_last = pl.T * ch - 1;
        for (int p0 = 0; p0 < up; ++p0) {
          const RsElem el = rs_elem(pl, ch, p0, e_last);
          CHECK(el.o == pl.T - 1 && el.c == ch - 1 && el.p >= 0 && el.p < up, "last element");
          for (int shift = 0; shift < 4; ++shift) {
            const int nq = (shift + pl.W * ch + 3) / 4;
            CHECK(4 * nq <= pl.stage_words, "nq %d", nq);
            const int hi = rs_first_word(shift, ch, el) + (pl.K4 - 1) * ch;
            CHECK(hi < shift + pl.W * ch, "stage read %d W %d p0 %d", hi, pl.W, p0);
          }
        }
        if (g_fail != before && g_fail <= 40)
          fprintf(stderr, "  at %d/%d ch %d: T %d W %d K %d K4 %d Ks %d stage %d tab %d\n", up,
                  down, ch, pl.T, pl.W, pl.K, pl.K4, pl.Ks, pl.stage_words, pl.tab_words);
      }
    }
  return plans;
}

// ---------------------------------------------------------------------------
// 2. element by element
// ---------------------------------------------------------------------------
constexpr i64 kZero = -1, kUnstaged = -2;  // origins of an LDS word that is no word of x

typedef std::vector<std::pair<i64, i64>> Pairs;  // (tap index, frame of the range)

void check_tile(const RsPlan& pl, i64 start, i64 len, i64 n_out, i64 tile) {
  const int ch = pl.ch;
  const size_t n_lds = (size_t)pl.stage_words + pl.tab_words;
  i64* lds = new i64[n_lds];  // exactly sized: a read or write past it is ASan's
  i64* stage = lds;
  i64* tab = lds + pl.stage_words;
  for (size_t i = 0; i < n_lds; ++i) lds[i] = kUnstaged;
  for (int i = 0; i < pl.tab_words; ++i) tab[i] = rs_tab_src(pl, i);
  // the kernel's staging: nq 16-byte pieces from a0, zeros outside the live words
  const i64 lo = start * ch, hi = (start + len) * ch;
  const RsTile t = rs_tile(pl, ch, start, tile);
  CHECK(t.a0 <= t.w0 && t.w0 - t.a0 < 4 && (t.a0 & 3) == 0 && t.shift == (int)(t.w0 - t.a0),
        "a0 %lld w0 %lld", t.a0, t.w0);
  CHECK(t.p0 >= 0 && t.p0 < pl.up && t.c0 == t.ih0 * pl.up + t.p0, "p0");
  CHECK(4 * t.nq <= pl.stage_words, "nq");
  for (int q = 0; q < t.nq; ++q)
    for (int k = 0; k < 4; ++k) {
      const i64 a = t.a0 + 4 * (i64)q + k;
      stage[4 * q + k] = (a >= lo && a < hi) ? a : kZero;
    }
  const i64 half = (pl.n_taps - 1) / 2;
  Pairs got, want;
  for (int e = 0; e < pl.T * ch; ++e) {
    const RsElem el = rs_elem(pl, ch, t.p0, e);
    if (t.j0 + el.o >= n_out) break;
    CHECK(el.p >= 0 && el.p < pl.up && el.c >= 0 && el.c < ch, "element");
    const int first = rs_first_word(t.shift, ch, el);
    const int row = rs_tab_row(pl, el.p);
    got.clear(), want.clear();
    for (int v = 0; v < pl.K4; ++v) {
      const int sw = first + v * ch;
      CHECK(sw >= t.shift && sw < t.shift + pl.W * ch && sw < 4 * t.nq, "stage word %d", sw);
      const i64 m = tab[row + v], g = stage[sw];
      CHECK(g != kUnstaged && m != kUnstaged, "unstaged word");
      if (v >= pl.K) CHECK(m == kZero, "padded term meets tap %lld", m);
      if (m >= 0 && g >= 0) {
        CHECK(g % ch == el.c, "channel");
        got.push_back(std::make_pair(m, g / ch - start));
      }
    }
    // the statement, from the output frame alone
    const i64 j = tile * pl.T + el.o;
    const i64 c = (i64)pl.down * j + half, ph = c % pl.up, ih = c / pl.up;
    for (i64 tt = pl.K - 1; tt >= 0; --tt) {
      const i64 m = ph + pl.up * tt, i = ih - tt;
      if (m < pl.n_taps && i >= 0 && i < len) want.push_back(std::make_pair(m, i));
    }
    if (got != want) {
      std::sort(got.begin(), got.end());
      std::sort(want.begin(), want.end());
      CHECK(got == want, "terms of output %lld ch %d (%d/%d n_taps %d ch %d tile %lld start %lld)",
            j, el.c, pl.up, pl.down, pl.n_taps, ch, tile, start);
    }
  }
  delete[] lds;
}

void elementwise(int up, int down, int n_taps, int ch) {
  if (n_taps == 0) n_taps = 20 * (up > down ? up : down) + 1;
  const i64 starts[2] = {0, 13};
  for (int s = 0; s < 2; ++s) {
    const i64 start = starts[s];
    for (int big = 0; big < 2; ++big) {
      RsPlan pl0;
      if (!rs_plan(up, down, n_taps, ch, &pl0)) {
        CHECK(false, "no plan %d/%d n_taps %d ch %d", up, down, n_taps, ch);
        return;
      }
      // 3.5 tiles, or tiles just under the limit
      const i64 want_out = big ? ((i64)0x7FFFFFFF - 1) * pl0.T + pl0.T / 2 : 7 * (i64)pl0.T / 2;
      const i64 len = (want_out * down + up - 1) / up;
      RsPlan pl;
      i64 n_out = 0, tiles = 0;
      const RsArgs r = rs_check_args(true, true, true, start + len + 29, start, len, ch, up, down,
                                     n_taps, &pl, &n_out, &tiles);
      CHECK(r == kRsOk, "args %d/%d n_taps %d ch %d len %lld: %d", up, down, n_taps, ch, len,
            (int)r);
      if (r != kRsOk) continue;
      CHECK(n_out * down >= len * up && (n_out - 1) * down < len * up &&
                (tiles - 1) * pl.T < n_out && tiles * pl.T >= n_out, "n_out %lld", n_out);
      if (big) {
        CHECK(tiles > (i64)0x7FFFFFFF - 8 && tiles <= 0x7FFFFFFF, "tiles %lld", tiles);
        check_tile(pl, start, len, n_out, tiles - 1);
      } else {
        CHECK(tiles == 4 && n_out % pl.T != 0, "tiles %lld", tiles);
        check_tile(pl, start, len, n_out, 0);
        check_tile(pl, start, len, n_out, 1);
        check_tile(pl, start, len, n_out, tiles - 1);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// 3. the guards (tests/test_gpu_resample.py::test_entry_point_guards)
// ---------------------------------------------------------------------------
struct Call {
  bool x = true, h = true, out = true;
  int64_t n_total = 64, start = 0, ln = 64;
  int32_t ch = 2, up = 1, down = 2, n_taps = 41;
};

RsArgs classify(const Call& c) {
  RsPlan pl;
  i64 n_out, tiles;
  return rs_check_args(c.x, c.h, c.out, c.n_total, c.start, c.ln, c.ch, c.up, c.down, c.n_taps,
                       &pl, &n_out, &tiles);
}

void guards() {
  Call b;
  CHECK(classify(b) == kRsOk, "base call");
  std::vector<Call> bad(18);
  bad[0].x = false, bad[1].h = false, bad[2].out = false, bad[3].start = -1, bad[4].ln = 0;
  bad[5].start = 1, bad[6].ln = 65, bad[7].n_total = -1, bad[8].n_taps = 40, bad[9].n_taps = 0;
  bad[10].up = 2, bad[10].down = 2;
  bad[11].up = 1, bad[11].down = 1;
  bad[12].up = 2, bad[12].down = 4;
  bad[13].up = 6, bad[13].down = 4;
  bad[14].up = 0, bad[15].down = 0, bad[16].ch = 0, bad[17].ch = 9;
  for (size_t i = 0; i < bad.size(); ++i) CHECK(classify(bad[i]) == kRsArg, "bad_arg %zu", i);
  std::vector<Call> uns(6);
  uns[0].up = 513, uns[0].down = 512, uns[0].n_taps = 41;
  uns[1].up = 1, uns[1].down = 9;
  uns[2].up = 3, uns[2].down = 25;
  uns[3].up = 512, uns[3].down = 513, uns[3].n_taps = 41;
  uns[4].n_taps = 43;
  uns[5].up = 160, uns[5].down = 147, uns[5].n_taps = 3203;
  for (size_t i = 0; i < uns.size(); ++i)
    CHECK(classify(uns[i]) == kRsUnsupported, "unsupported %zu", i);
  std::vector<Call> ok(3);
  ok[0].up = 512, ok[0].down = 511, ok[0].n_taps = 10241;
  ok[1].up = 1, ok[1].down = 8, ok[1].n_taps = 161;
  ok[2].ch = 8, ok[2].n_total = 16, ok[2].ln = 16;
  for (size_t i = 0; i < ok.size(); ++i) CHECK(classify(ok[i]) == kRsOk, "ok %zu", i);
  // the limits themselves
  Call c;
  c.n_total = ((int64_t)1 << 48) + 1, c.ln = 1;
  CHECK(classify(c) == kRsUnsupported, "n_total past 2^48");
  c = Call();  // one tile more than 2^31 - 1: 1 / 2 mono, T = 1024
  c.ch = 1, c.ln = 2 * (((int64_t)0x7FFFFFFF) * 1024 + 1), c.n_total = c.ln;
  CHECK(classify(c) == kRsUnsupported, "tiles past 2^31 - 1");
  c.ln -= 2, c.n_total = c.ln;
  CHECK(classify(c) == kRsOk, "2^31 - 1 tiles");
}

void print_plan(int up, int down, int n_taps, int ch) {
  if (n_taps == 0) n_taps = 20 * (up > down ? up : down) + 1;
  RsPlan pl;
  if (!rs_plan(up, down, n_taps, ch, &pl)) {
    CHECK(false, "no plan %d/%d n_taps %d ch %d", up, down, n_taps, ch);
    return;
  }
  printf("plan %d %d %d %d %d %d %d %d\n", up, down, n_taps, ch, pl.T, pl.W, pl.stage_words,
         pl.tab_words);
}

}  // namespace

int main() {
  const long plans = whole_domain();
  printf("whole domain: %ld plans\n", plans);

  // (up, down, n_taps; 0: the default 20 max + 1)
  static const int kElem[][3] = {{160, 147, 0}, {1, 2, 0},  {1, 8, 0},       {512, 511, 0},
                                 {4, 7, 0},     {2, 3, 0},  {3, 2, 1},       {3, 2, 5},
                                 {5, 3, 3},     {2, 3, 15}, {160, 147, 159}, {160, 147, 161},
                                 {7, 5, 13},    {1, 2, 7}};
  static const int kElemCh[] = {1, 2, 3, 8};
  for (const auto& r : kElem)
    for (int ch : kElemCh) elementwise(r[0], r[1], r[2], ch);
  printf("element by element: %zu plans x 4 channel counts\n", sizeof kElem / sizeof kElem[0]);

  guards();

  // the plans the GPU tests take a length from: every default-filter ratio of
  // tests/test_gpu_resample.py and tests/test_gpu_resample_paths.py at 1 to 8
  // channels, and the custom filters of the latter
  static const int kDefault[][2] = {{160, 147}, {80, 147}, {40, 147}, {1, 2},     {1, 4},
                                    {3, 2},     {2, 1},    {320, 147}, {6, 1},    {3, 1},
                                    {512, 511}, {1, 8},    {4, 7},     {2, 3}};
  for (const auto& r : kDefault)
    for (int ch = 1; ch <= kMaxCh; ++ch) print_plan(r[0], r[1], 0, ch);
  static const int kCustom[][3] = {{3, 2, 1},  {3, 2, 5},      {5, 3, 3},      {7, 5, 13},
                                   {1, 2, 7},  {2, 3, 15},     {160, 147, 159}, {160, 147, 161},
                                   {1, 2, 41}, {160, 147, 3201}};
  for (const auto& r : kCustom)
    for (int ch : kElemCh) print_plan(r[0], r[1], r[2], ch);

  printf("failures %ld\n", g_fail);
  return g_fail ? 1 : 0;
}
