// mel_nnls.h -- the mel inversion kernel's tables and arithmetic (mel_nnls.hip): per frame column the non-negative least
// squares problem  min_{p >= 0} || M p - m ||^2  for a mel filterbank M (n_mels, F), by n_iter projected-gradient steps
//   r = M y - m;   p+ = max(y - eta M^T r, 0);   y = p+ + beta_k (p+ - p);   p = p+          (p = y = 0 at the start)
// with M kept SPARSE: a triangular bank has 2 .. 53 non-zeros per row, all contiguous, and at most 2 rows over any bin.
// Plain C++ like cfp_fft.h / fft_core.h: tests/native/mel_nnls_harness.cpp compiles the same functions for the host and
// runs the NT threads of a tile one after the other -- tables, index arithmetic and summation order are tested without a
// GPU.
//
// The table blob (32-bit words; built on the host by build_tables, copied to LDS by the kernel):
//   [0 .. 4)            n_act, nnz, F, n_mels
//   rows   4 n_act      per ACTIVE row c (a row with at least one non-zero, in the bank's order): start, length, offset of
//                       its weights in w, its row index in the bank (where its mel value is read)
//   bins   F            per bin one word: first active row over it (bits 0 .. 8), how many (9 .. 11), offset in tw (12 ..)
//   w      nnz floats   the rows' weights, row after row            (M y:   one (row, frame) walks its support)
//   tw     nnz floats   the same weights, bin after bin             (M^T r: one (bin, frame) gathers <= MAX_COVER terms)
// Rows without a non-zero (a bank with more filters than bins has them) take no part: their residual is -m whatever p is,
// and they reach no bin.  With the active rows' starts and stops non-decreasing, the rows over a bin are consecutive.
//
// Arithmetic: the iterate lives in FLOAT64 -- p and y in registers, the y and residual tiles in LDS, every sum and
// product -- and is rounded to float32 once, when p ** (1 / power) is stored.  A float32 iterate is not good enough here:
// each step rounds y at eps |y|, the row sums carry that into r and g at the scale of the LOUD bins of a row, and a quiet
// bin beside them (p 1e-4 of its neighbours) takes an absolute error of their size; ** (1 / 2) divides it by 2 sqrt p.
// Measured with the float32 version of this header on the GPU suite's inputs: 101 of 102 cases within 1.9 x the float32
// oracle's error, one at 4.6 x (one bin, p = 2e-5 beside 0.26) -- the float32 oracle draws from the same tail, so the
// ratio of two maxima is a lottery.  In float64 the error is the output rounding.  gfx950 runs v_fma_f64 at half the
// float32 rate and the tiles are twice as wide; DESIGN.md 3.17 has what that costs.
//
// A tile is TF consecutive frames of one clip, NT threads:
//   row walk   32 lanes per active row: lane = phase * TF + frame, KP = 32 / TF phases; phase ph sums the row's non-zeros
//              ph, ph + KP, ..; the phases are added by a butterfly over the lanes (xor TF, 2 TF, ..).  The y tile is
//              (F, TF) doubles, bin stride TF unpadded: the 32 lanes of a row read KP consecutive bins x TF frames = 32
//              consecutive doubles, 256 bytes: one per bank pair of ds_read_b64.  Rows are dealt round-robin to the 16 half waves (row c to half wave
//              c % 16), so that the long rows at the top of the bank are spread over all waves.
//   update     thread tid owns frame tid % TF of bins tid / TF + i NT / TF, i < NE: p and y of its elements stay in
//              registers over all iterations; y is written to the tile for the next row walk.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MELNNLS_HD __host__ __device__ __forceinline__
#else
#define MELNNLS_HD inline
#endif

namespace melnnls {

constexpr int NT = 512;          // threads of a workgroup
constexpr int ROW_LANES = 32;    // lanes of one row in the row walk: a half wave
constexpr int MAX_MELS = 256;
constexpr int MAX_F = 2049;      // n_fft <= 4096
// Rows over one bin.  A triangular bank needs 2; 4 leaves room for banks whose filters overlap their second neighbours
// (wider-than-critical triangles), keeps the gather a loop of a few terms, and bounds nnz <= MAX_COVER F: that bound is
// what makes the worst case below fit the LDS.  A dense bank (gammatone, a trained mel_basis) has n_mels rows over every
// bin: the composition of torch operators serves it.
constexpr int MAX_COVER = 4;
constexpr int HEADER_WORDS = 4;
constexpr int ROW_WORDS = 4;

// frames of a tile: as many as keep the (F, TF) float64 tile of y at 64 KB, beside the tables: 16 up to n_fft 1024, 8 up
// to 2048, 4 above
constexpr int tile_frames(int F) { return F <= 513 ? 16 : F <= 1025 ? 8 : 4; }
// bins a thread owns: ceil(F / (NT / TF)); the kernel is instantiated for NE = 9, 17
constexpr int elements_per_thread(int F, int TF) { return (F + NT / TF - 1) / (NT / TF); }
constexpr int MAX_NE = 17;
static_assert(elements_per_thread(513, 16) == MAX_NE && elements_per_thread(1025, 8) == MAX_NE &&
              elements_per_thread(MAX_F, 4) == MAX_NE, "register slots");

constexpr long table_words(int n_act, int F, int nnz) { return HEADER_WORDS + (long)ROW_WORDS * n_act + F + 2L * nnz; }
// words the tables take in LDS: an even number, so that the float64 tiles behind them are aligned
constexpr long table_words_lds(long words) { return (words + 1) / 2 * 2; }
// LDS of a workgroup: the tables, the y tile (F, TF) and the residual tile (n_act, TF) in float64, the mel tile (n_act, TF)
constexpr long lds_bytes(int F, int n_act, int nnz, int TF) {
  return 4 * table_words_lds(table_words(n_act, F, nnz)) + 8L * F * TF + 12L * n_act * TF;
}
constexpr long LDS_LIMIT = 160 * 1024;
static_assert(lds_bytes(513, MAX_MELS, MAX_COVER * 513, tile_frames(513)) <= LDS_LIMIT, "LDS, 16-frame tiles");
static_assert(lds_bytes(1025, MAX_MELS, MAX_COVER * 1025, tile_frames(1025)) <= LDS_LIMIT, "LDS, 8-frame tiles");
static_assert(lds_bytes(MAX_F, MAX_MELS, MAX_COVER * MAX_F, tile_frames(MAX_F)) <= LDS_LIMIT, "LDS, 4-frame tiles");
static_assert(MAX_MELS <= 512 && MAX_COVER <= 7 && MAX_COVER * MAX_F < (1 << 20), "the packing of a bin's word");

// what can be told from the sizes alone (mispec_mel_nnls_f32 sees the bank only as its tables)
constexpr bool served_shape(int n_mels, int F, int n_act, int nnz, float power) {
  return n_mels >= 1 && n_mels <= MAX_MELS && F >= 1 && F <= MAX_F && n_act >= 0 && n_act <= n_mels && nnz >= n_act &&
         nnz <= MAX_COVER * F && power > 0.f;
}

struct Sizes {
  int n_act, nnz;
};

// Scans a dense bank (n_mels rows of F floats, row_stride floats apart; HOST memory) and, when `blob` is not null, writes
// the table blob (table_words(n_act, F, nnz) words).  False when the bank is not served: a zero between two non-zeros of
// a row, active rows whose starts or stops decrease, more than MAX_COVER rows over a bin, or sizes beyond the caps.
inline bool build_tables(const float *M, long row_stride, int n_mels, int F, Sizes &sz, int32_t *blob) {
  sz.n_act = sz.nnz = 0;
  if (M == nullptr || n_mels < 1 || n_mels > MAX_MELS || F < 1 || F > MAX_F || row_stride < F) return false;
  int start[MAX_MELS], len[MAX_MELS], orig[MAX_MELS];
  int n_act = 0, nnz = 0;
  for (int r = 0; r < n_mels; ++r) {
    const float *row = M + (long)r * row_stride;
    int a = 0, b = F;
    while (a < F && row[a] == 0.f) ++a;
    if (a == F) continue;  // an empty row
    while (row[b - 1] == 0.f) --b;
    for (int k = a; k < b; ++k)
      if (row[k] == 0.f) return false;  // a gap inside the row
    if (n_act > 0 && (a < start[n_act - 1] || b < start[n_act - 1] + len[n_act - 1])) return false;
    start[n_act] = a;
    len[n_act] = b - a;
    orig[n_act] = r;
    ++n_act;
    nnz += b - a;
  }
  // rows over a bin: consecutive active rows (starts and stops are monotone); lo = the first row whose stop is beyond b
  int lo = 0, hi = 0;  // rows [lo, hi) cover the bin
  int first[MAX_F];
  unsigned char cnt[MAX_F];
  for (int b = 0; b < F; ++b) {
    while (hi < n_act && start[hi] <= b) ++hi;
    while (lo < hi && start[lo] + len[lo] <= b) ++lo;
    if (hi - lo > MAX_COVER) return false;
    first[b] = lo;
    cnt[b] = (unsigned char)(hi - lo);
  }
  if (nnz > MAX_COVER * F) return false;
  sz.n_act = n_act;
  sz.nnz = nnz;
  if (blob == nullptr) return true;
  blob[0] = n_act;
  blob[1] = nnz;
  blob[2] = F;
  blob[3] = n_mels;
  int32_t *rows = blob + HEADER_WORDS;
  uint32_t *bins = reinterpret_cast<uint32_t *>(rows + ROW_WORDS * n_act);
  float *w = reinterpret_cast<float *>(bins + F);
  float *tw = w + nnz;
  int off = 0;
  for (int c = 0; c < n_act; ++c) {
    rows[ROW_WORDS * c + 0] = start[c];
    rows[ROW_WORDS * c + 1] = len[c];
    rows[ROW_WORDS * c + 2] = off;
    rows[ROW_WORDS * c + 3] = orig[c];
    for (int k = 0; k < len[c]; ++k) w[off + k] = M[(long)orig[c] * row_stride + start[c] + k];
    off += len[c];
  }
  off = 0;
  for (int b = 0; b < F; ++b) {
    bins[b] = (uint32_t)first[b] | ((uint32_t)cnt[b] << 9) | ((uint32_t)off << 12);
    for (int j = 0; j < cnt[b]; ++j) tw[off + j] = M[(long)orig[first[b] + j] * row_stride + b];
    off += cnt[b];
  }
  return true;
}

inline bool served(const float *M, long row_stride, int n_mels, int F, float power) {
  Sizes sz;
  return power > 0.f && build_tables(M, row_stride, n_mels, F, sz, nullptr) &&
         served_shape(n_mels, F, sz.n_act, sz.nnz, power);
}

// the blob as the kernel reads it (n_act, nnz, F from the caller: the same numbers that sized the blob)
struct View {
  const int32_t *rows;
  const uint32_t *bins;
  const float *w, *tw;
  int n_act, F;
};

MELNNLS_HD View view(const int32_t *blob, int n_act, int F, int nnz) {
  View v;
  v.rows = blob + HEADER_WORDS;
  v.bins = reinterpret_cast<const uint32_t *>(v.rows + ROW_WORDS * n_act);
  v.w = reinterpret_cast<const float *>(v.bins + F);
  v.tw = v.w + nnz;
  v.n_act = n_act;
  v.F = F;
  return v;
}

// Row walk, lane `lane` (< ROW_LANES) of active row c: the sum over its phase of w y.  The row's (M y)[frame] is the sum of
// the KP lanes frame, frame + TF, ..: reduce_phases.
template <int TF>
MELNNLS_HD double row_partial(const View &v, const double *ytile, int c, int lane) {
  constexpr int KP = ROW_LANES / TF;
  const int t = lane % TF, ph = lane / TF;
  const int s = v.rows[ROW_WORDS * c], len = v.rows[ROW_WORDS * c + 1], off = v.rows[ROW_WORDS * c + 2];
  double acc = 0.0;
  for (int k = ph; k < len; k += KP) acc = fma((double)v.w[off + k], ytile[(s + k) * TF + t], acc);
  return acc;
}

// The butterfly over the phases: xchg(value, mask) returns the value of lane ^ mask.  Every lane ends with the row's sum.
template <int TF, class Xchg>
MELNNLS_HD double reduce_phases(double a, Xchg xchg) {
#pragma unroll
  for (int m = TF; m < ROW_LANES; m <<= 1) a += xchg(a, m);
  return a;
}

// (M^T r)[b] of frame t: the rows over bin b
template <int TF>
MELNNLS_HD double gradient(const View &v, const double *rtile, int b, int t) {
  const uint32_t info = v.bins[b];
  const int first = info & 511, cnt = (info >> 9) & 7, off = info >> 12;
  double g = 0.0;
  for (int j = 0; j < cnt; ++j) g = fma((double)v.tw[off + j], rtile[(first + j) * TF + t], g);
  return g;
}

// projection and momentum of one element
MELNNLS_HD void update(double &p, double &y, double g, double eta, double beta) {
  const double pn = fmax(fma(-eta, g, y), 0.0);
  y = fma(beta, pn - p, pn);
  p = pn;
}

// the one rounding to float32
MELNNLS_HD float finish(double p, float power) {
  if (power == 1.f) return (float)p;
  if (power == 2.f) return (float)sqrt(p);
  return p > 0.0 ? (float)pow(p, 1.0 / (double)power) : 0.f;
}

}  // namespace melnnls
