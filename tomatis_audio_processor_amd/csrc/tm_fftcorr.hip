// tm_fftcorr.hip — "full" cross-correlation through a large FFT (SURVEY.md §8
// row f7): compare_audio.find_delay_by_corr of the reference
// (src/compare_audio.py:30-42) correlates whole envelopes,
//   corr = fftconvolve(c, b[::-1], mode="full")                       :37
// nc + nb - 1 lags, which the direct kernel of tm_align.hip cannot pay for at
// file length.  Two entry points:
//   tomatis_fft_pow2          complex FFT of L = 2^p points in global memory
//   tomatis_align_xcorr_full  :37 as pack -> FFT -> C conj(B) -> inverse FFT
//
// The transform (float32, p = 4 .. 25):
//  * p <= kRowLog (8192 points, 64 KiB): one workgroup, the Stockham FFT of
//    tm_lds_fft.h in LDS.
//  * above: six-step, L = N1 N2 with N1 = 2^ceil(p/2), N2 = 2^floor(p/2), the
//    input index n = n1 N2 + n2, the output index k = k1 + N1 k2:
//      1 transpose  [N1][N2] -> [N2][N1]                   in   -> out
//      2 rows: FFT_N1 over n1, times W_L^(n2 k1)           out  in place
//      3 transpose  [N2][N1] -> [N1][N2]                   out  -> work
//      4 rows: FFT_N2 over n2                              work in place
//      5 transpose  [N1][N2] -> [N2][N1]                   work -> out
//    Every pass reads and writes whole 256-byte row segments; the transposes
//    go through a padded 32 x 32 LDS tile, a row pass holds one row per
//    workgroup in LDS.
//  * twiddles: the tables of the row FFTs (exp(-2 pi i t / N)) and the
//    inter-pass factors W_L^(n2 k1) are evaluated as sincospi in float64 on
//    the device and rounded once to float32: the argument n2 k1 / L is exact
//    (L is a power of two, n2 k1 < L), so the values are those of a float64
//    host table without its L entries.
//  * inverse: conj(FFT(conj x)) / L, the conjugations and the scale folded into
//    the first load and the last store.
// No atomics: the same bits in every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tomatis_hip.h"
#include "tm_lds_fft.h"

namespace {

typedef long long i64;

constexpr int kT = 256;
constexpr int kMinLog = TOMATIS_FFT_MIN_LOG2;  // 16 points
constexpr int kMaxLog = TOMATIS_FFT_MAX_LOG2;  // 2^25
constexpr int kRowLog = 13;                    // one row FFT: 8192 points, 64 KiB of LDS
constexpr int kRowMax = 1 << kRowLog;
constexpr int kTile = 32;                      // transpose tile
constexpr int kConjIn = 1, kConjOut = 2, kTwiddle = 4;

int fc_launch() { return hipGetLastError() == hipSuccess ? TOMATIS_OK : TOMATIS_E_HIP; }

// tw[t] = exp(-2 pi i t / n), float64 rounded once
__global__ __launch_bounds__(kT) void k_fc_table(float2* __restrict__ tw, int n) {
  const int t = blockIdx.x * kT + threadIdx.x;
  if (t >= n) return;
  double s, c;
  sincospi(-2.0 * (double)t / (double)n, &s, &c);
  tw[t] = make_float2((float)c, (float)s);
}

// One N-point FFT per workgroup over row blockIdx.x of in -> the same row of
// out (in == out allowed: a workgroup reads its row before it writes it).
// kTwiddle: times exp(-2 pi i row col / L), inv_L = 1 / L.
template <int N>
__global__ __launch_bounds__(kT) void k_fc_rows(const float2* __restrict__ in,
                                                float2* __restrict__ out,
                                                const float2* __restrict__ tw, int flags,
                                                double inv_L, float scale) {
  __shared__ __attribute__((aligned(16))) float2 buf[N];
  const int tid = threadIdx.x;
  const i64 row = blockIdx.x;
  const float2* src = in + row * N;
  float2* dst = out + row * N;
  for (int i = tid; i < N; i += kT) {
    float2 v = src[i];
    if (flags & kConjIn) v.y = -v.y;
    buf[i] = v;
  }
  __syncthreads();
  tlds::lds_fft<N, kT>(buf, tw);  // ends on a barrier
  for (int i = tid; i < N; i += kT) {
    float2 v = buf[i];
    if (flags & kTwiddle) {
      double s, c;
      sincospi(-2.0 * (double)(row * i) * inv_L, &s, &c);
      v = tlds::cmul(v, make_float2((float)c, (float)s));
    }
    if (flags & kConjOut) v.y = -v.y;
    dst[i] = make_float2(v.x * scale, v.y * scale);
  }
}

// out[c][r] = in[r][c] for in of R rows and C columns, both multiples of kTile
__global__ __launch_bounds__(kT) void k_fc_transpose(const float2* __restrict__ in,
                                                     float2* __restrict__ out, int R, int C,
                                                     int flags, float scale) {
  __shared__ float2 tile[kTile][kTile + 1];
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
  const i64 c0 = (i64)blockIdx.x * kTile, r0 = (i64)blockIdx.y * kTile;
  for (int r = ty; r < kTile; r += kT / kTile) {
    float2 v = in[(r0 + r) * C + c0 + tx];
    if (flags & kConjIn) v.y = -v.y;
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < kTile; r += kT / kTile) {
    float2 v = tile[tx][r];
    if (flags & kConjOut) v.y = -v.y;
    out[(c0 + r) * R + r0 + tx] = make_float2(v.x * scale, v.y * scale);
  }
}

template <int N>
void rows_n(unsigned rows, const float2* in, float2* out, const float2* tw, int flags,
            double inv_L, float scale, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_rows<N>, dim3(rows), dim3(kT), 0, s, in, out, tw, flags, inv_L, scale);
}

void rows(int logn, unsigned n_rows, const float2* in, float2* out, const float2* tw, int flags,
          double inv_L, float scale, hipStream_t s) {
  switch (logn) {
#define TM_FC_ROWS(P) \
  case P: rows_n<(1 << P)>(n_rows, in, out, tw, flags, inv_L, scale, s); break;
    TM_FC_ROWS(4) TM_FC_ROWS(5) TM_FC_ROWS(6) TM_FC_ROWS(7) TM_FC_ROWS(8) TM_FC_ROWS(9)
    TM_FC_ROWS(10) TM_FC_ROWS(11) TM_FC_ROWS(12) TM_FC_ROWS(13)
#undef TM_FC_ROWS
  }
}

void table(float2* tw, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_fc_table, dim3((n + kT - 1) / kT), dim3(kT), 0, s, tw, n);
}

void transpose(const float2* in, float2* out, int R, int C, int flags, float scale,
               hipStream_t s) {
  hipLaunchKernelGGL(k_fc_transpose, dim3(C / kTile, R / kTile), dim3(kT), 0, s, in, out, R, C,
                     flags, scale);
}

i64 fft_work_bytes(int p) {
  return 2 * (i64)kRowMax * (i64)sizeof(float2) + (p > kRowLog ? ((i64)sizeof(float2) << p) : 0);
}

// in != out, p in [kMinLog, kMaxLog]
int fft_run(const float2* in, float2* out, int p, bool inverse, void* work, hipStream_t s) {
  float2* tw1 = (float2*)work;
  float2* tw2 = tw1 + kRowMax;
  float2* tmp = tw2 + kRowMax;
  const float scale = inverse ? (float)(1.0 / (double)((i64)1 << p)) : 1.0f;  // exact
  const int cin = inverse ? kConjIn : 0, cout = inverse ? kConjOut : 0;
  if (p <= kRowLog) {
    table(tw1, 1 << p, s);
    rows(p, 1, in, out, tw1, cin | cout, 0.0, scale, s);
    return fc_launch();
  }
  const int p1 = (p + 1) / 2, p2 = p / 2;
  const int N1 = 1 << p1, N2 = 1 << p2;
  table(tw1, N1, s);
  if (p2 != p1) table(tw2, N2, s);
  transpose(in, out, N1, N2, cin, 1.0f, s);
  rows(p1, N2, out, out, tw1, kTwiddle, 1.0 / (double)((i64)1 << p), 1.0f, s);
  transpose(out, tmp, N2, N1, 0, 1.0f, s);
  rows(p2, N1, tmp, tmp, p2 != p1 ? tw2 : tw1, 0, 0.0, 1.0f, s);
  transpose(tmp, out, N1, N2, cout, scale, s);
  return fc_launch();
}

// ---------------------------------------------------------------------------
// full correlation
// ---------------------------------------------------------------------------
// z = c + i b, zero-padded to L
__global__ __launch_bounds__(kT) void k_fc_pack(const float* __restrict__ c, i64 nc,
                                                const float* __restrict__ b, i64 nb,
                                                float2* __restrict__ z, i64 L) {
  for (i64 i = (i64)blockIdx.x * kT + threadIdx.x; i < L; i += (i64)gridDim.x * kT)
    z[i] = make_float2(i < nc ? c[i] : 0.0f, i < nb ? b[i] : 0.0f);
}

// Z = FFT(c + i b): C[k] = (Z[k] + conj Z[L - k]) / 2, B[k] = (Z[k] - conj Z[L - k]) / 2i;
// p[k] = C[k] conj(B[k])
__global__ __launch_bounds__(kT) void k_fc_cross(const float2* __restrict__ z,
                                                 float2* __restrict__ p, i64 L) {
  for (i64 k = (i64)blockIdx.x * kT + threadIdx.x; k < L; k += (i64)gridDim.x * kT) {
    const float2 u = z[k], v = z[(L - k) & (L - 1)];
    const float2 C = make_float2(0.5f * (u.x + v.x), 0.5f * (u.y - v.y));
    const float2 B = make_float2(0.5f * (u.y + v.y), 0.5f * (v.x - u.x));
    p[k] = tlds::cmul_conj(C, B);
  }
}

// out[k] = Re r[(k - (nb - 1)) mod L]
__global__ __launch_bounds__(kT) void k_fc_lags(const float2* __restrict__ r, i64 L, i64 nb,
                                                float* __restrict__ out, i64 n_out) {
  for (i64 k = (i64)blockIdx.x * kT + threadIdx.x; k < n_out; k += (i64)gridDim.x * kT)
    out[k] = r[(k - (nb - 1)) & (L - 1)].x;
}

int full_log2(i64 nc, i64 nb) {  // -1: over the cap
  const i64 n = nc + nb - 1;
  int p = kMinLog;
  while (p <= kMaxLog && ((i64)1 << p) < n) ++p;
  return p <= kMaxLog ? p : -1;
}

unsigned grid_for(i64 n) {
  const i64 want = (n + kT - 1) / kT, cap = 256 * 16;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace

extern "C" {

int64_t tomatis_fft_pow2_work_bytes(int32_t log2n) {
  if (log2n < kMinLog || log2n > kMaxLog) return 0;
  return fft_work_bytes(log2n);
}

int tomatis_fft_pow2(const float* in, float* out, int32_t log2n, int32_t inverse, void* work,
                     void* hs) {
  if (!in || !out || !work || in == out) return TOMATIS_E_ARG;
  if (log2n < kMinLog || log2n > kMaxLog) return TOMATIS_E_UNSUPPORTED;
  return fft_run((const float2*)in, (float2*)out, log2n, inverse != 0, work, (hipStream_t)hs);
}

int64_t tomatis_align_xcorr_full_work_bytes(int64_t nc, int64_t nb) {
  if (nc < 1 || nb < 1) return 0;
  const int p = full_log2(nc, nb);
  if (p < 0) return 0;
  return 2 * ((int64_t)sizeof(float2) << p) + fft_work_bytes(p);
}

int tomatis_align_xcorr_full(const float* c, int64_t nc, const float* b, int64_t nb, float* out,
                             void* work, void* hs) {
  if (!c || !b || !out || !work || nc < 1 || nb < 1) return TOMATIS_E_ARG;
  if (nc > ((int64_t)1 << kMaxLog) || nb > ((int64_t)1 << kMaxLog)) return TOMATIS_E_UNSUPPORTED;
  const int p = full_log2(nc, nb);
  if (p < 0) return TOMATIS_E_UNSUPPORTED;
  hipStream_t s = (hipStream_t)hs;
  const i64 L = (i64)1 << p;
  float2* z = (float2*)work;
  float2* f = z + L;
  void* fw = f + L;
  hipLaunchKernelGGL(k_fc_pack, dim3(grid_for(L)), dim3(kT), 0, s, c, (i64)nc, b, (i64)nb, z, L);
  int rc = fft_run(z, f, p, false, fw, s);
  if (rc != TOMATIS_OK) return rc;
  hipLaunchKernelGGL(k_fc_cross, dim3(grid_for(L)), dim3(kT), 0, s, (const float2*)f, z, L);
  rc = fft_run(z, f, p, true, fw, s);
  if (rc != TOMATIS_OK) return rc;
  const i64 n_out = nc + nb - 1;
  hipLaunchKernelGGL(k_fc_lags, dim3(grid_for(n_out)), dim3(kT), 0, s, (const float2*)f, L,
                     (i64)nb, out, n_out);
  return fc_launch();
}

}  // extern "C"
