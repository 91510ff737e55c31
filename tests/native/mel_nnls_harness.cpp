// Host harness of nnaudio_amd/csrc/mel_nnls.h (tests/test_mel_inverse_cpu.py compiles and runs it): the sparse tables of
// real mel banks and the kernel's iteration, with the NT threads of a tile run one after the other, against the float64
// dense result the test computed with tests/_mel_nnls_oracle.py, under the suite's rule (4 x the float32 yardstick's
// error, max and RMS).  Also the served() rule on banks it must refuse.
//
// Usage: mel_nnls_harness CASE_FILE...      a case file (little endian):
//   int32 n_mels, F, T, n_iter;  float32 power;  float64 eta, yard_max, yard_rms;
//   float32 bank[n_mels F], mel[n_mels T], beta[n_iter];  float64 want[F T]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mel_nnls.h"

using namespace melnnls;

static int failures = 0;

#define EXPECT(cond, ...)          \
  do {                             \
    if (!(cond)) {                 \
      ++failures;                  \
      std::printf("FAIL: " __VA_ARGS__); \
      std::printf("\n");           \
    }                              \
  } while (0)

template <class T>
static bool read_n(std::FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

// the tables against the dense bank: every non-zero once in w and once in tw, supports inside the bank
static void check_tables(const char *name, const std::vector<float> &M, int n_mels, int F, const std::vector<int32_t> &blob,
                         const Sizes &sz) {
  const View v = view(blob.data(), sz.n_act, F, sz.nnz);
  std::vector<double> dense((size_t)n_mels * F, 0.0), dense_t((size_t)n_mels * F, 0.0);
  int prev_row = -1;
  for (int c = 0; c < sz.n_act; ++c) {
    const int s = v.rows[4 * c], len = v.rows[4 * c + 1], off = v.rows[4 * c + 2], r = v.rows[4 * c + 3];
    EXPECT(s >= 0 && len >= 1 && s + len <= F && off >= 0 && off + len <= sz.nnz && r > prev_row && r < n_mels,
           "%s: row %d of the tables (start %d len %d off %d orig %d)", name, c, s, len, off, r);
    prev_row = r;
    for (int k = 0; k < len; ++k) dense[(size_t)r * F + s + k] = v.w[off + k];
  }
  int total = 0;
  for (int b = 0; b < F; ++b) {
    const uint32_t info = v.bins[b];
    const int first = info & 511, cnt = (info >> 9) & 7, off = info >> 12;
    EXPECT(cnt <= MAX_COVER && first + cnt <= sz.n_act && off == total, "%s: bin %d of the tables", name, b);
    for (int j = 0; j < cnt; ++j) dense_t[(size_t)v.rows[4 * (first + j) + 3] * F + b] = v.tw[off + j];
    total += cnt;
  }
  EXPECT(total == sz.nnz, "%s: %d transposed weights, %d non-zeros", name, total, sz.nnz);
  size_t bad = 0;
  for (size_t i = 0; i < dense.size(); ++i) bad += dense[i] != (double)M[i] || dense_t[i] != (double)M[i];
  EXPECT(bad == 0, "%s: %zu elements of the bank differ from its tables", name, bad);
}

// what lane `lane` holds before the butterfly's step m (m = TF, 2 TF, ..): its partial, plus the partners of the steps before
template <int TF>
static double before_step(const double *a, int lane, int m) {
  return m == TF ? a[lane] : before_step<TF>(a, lane, m / 2) + before_step<TF>(a, lane ^ (m / 2), m / 2);
}

// all tiles of one clip, as the kernel runs them
template <int TF, int NE>
static void run(const std::vector<int32_t> &blob, const Sizes &sz, int F, int T, int n_iter, double eta, float power,
                const std::vector<float> &mel, const std::vector<float> &beta, std::vector<float> &out) {
  constexpr int BP = NT / TF;
  const View v = view(blob.data(), sz.n_act, F, sz.nnz);
  std::vector<double> ytile((size_t)F * TF), rtile((size_t)sz.n_act * TF);
  std::vector<float> mtile((size_t)sz.n_act * TF);
  std::vector<double> pv((size_t)NT * NE), yv((size_t)NT * NE);
  for (int t0 = 0; t0 < T; t0 += TF) {
    for (int i = 0; i < sz.n_act * TF; ++i) {
      const int c = i / TF, t = i % TF;
      mtile[i] = t0 + t < T ? mel[(size_t)v.rows[4 * c + 3] * T + t0 + t] : 0.f;
    }
    std::fill(ytile.begin(), ytile.end(), 0.0);
    std::fill(pv.begin(), pv.end(), 0.0);
    std::fill(yv.begin(), yv.end(), 0.0);
    for (int k = 0; k < n_iter; ++k) {
      for (int hw = 0; hw < NT / ROW_LANES; ++hw)
        for (int c = hw; c < sz.n_act; c += NT / ROW_LANES) {
          double a[ROW_LANES];
          for (int lane = 0; lane < ROW_LANES; ++lane) a[lane] = row_partial<TF>(v, ytile.data(), c, lane);
          // the header's butterfly, lane by lane: the partner's value before step m is computed on demand
          for (int lane = 0; lane < TF; ++lane) {
            const double sum = reduce_phases<TF>(a[lane], [&](double, int m) { return before_step<TF>(a, lane ^ m, m); });
            rtile[c * TF + lane] = sum - (double)mtile[c * TF + lane];
          }
        }
      for (int tid = 0; tid < NT; ++tid) {
        const int t = tid % TF, b0 = tid / TF;
        for (int i = 0; i < NE; ++i) {
          const int b = b0 + i * BP;
          if (b < F) {
            update(pv[(size_t)tid * NE + i], yv[(size_t)tid * NE + i], gradient<TF>(v, rtile.data(), b, t), eta, (double)beta[k]);
            ytile[b * TF + t] = yv[(size_t)tid * NE + i];
          }
        }
      }
    }
    for (int tid = 0; tid < NT; ++tid) {
      const int t = tid % TF, b0 = tid / TF;
      if (t0 + t >= T) continue;
      for (int i = 0; i < NE; ++i) {
        const int b = b0 + i * BP;
        if (b < F) out[(size_t)b * T + t0 + t] = finish(pv[(size_t)tid * NE + i], power);
      }
    }
  }
}

static void run_case(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) {
    EXPECT(false, "cannot open %s", path);
    return;
  }
  int32_t h[4];
  float power;
  double eta, yard[2];
  std::vector<float> M, mel, beta;
  std::vector<double> want;
  bool ok = std::fread(h, 4, 4, f) == 4 && std::fread(&power, 4, 1, f) == 1 && std::fread(&eta, 8, 1, f) == 1 && std::fread(yard, 8, 2, f) == 2;
  const int n_mels = h[0], F = h[1], T = h[2], n_iter = h[3];
  ok = ok && read_n(f, M, (size_t)n_mels * F) && read_n(f, mel, (size_t)n_mels * T) && read_n(f, beta, (size_t)n_iter) &&
       read_n(f, want, (size_t)F * T);
  std::fclose(f);
  EXPECT(ok, "%s: short file", path);
  if (!ok) return;

  EXPECT(served(M.data(), F, n_mels, F, power), "%s: the bank is not served", path);
  Sizes sz;
  if (!build_tables(M.data(), F, n_mels, F, sz, nullptr)) return;
  std::vector<int32_t> blob((size_t)table_words(sz.n_act, F, sz.nnz));
  build_tables(M.data(), F, n_mels, F, sz, blob.data());
  check_tables(path, M, n_mels, F, blob, sz);
  const int TF = tile_frames(F);
  EXPECT(lds_bytes(F, sz.n_act, sz.nnz, TF) <= LDS_LIMIT, "%s: LDS", path);
  EXPECT(elements_per_thread(F, TF) <= MAX_NE, "%s: register slots", path);

  std::vector<float> out((size_t)F * T, -1.f);
  if (TF == 16)
    run<16, MAX_NE>(blob, sz, F, T, n_iter, eta, power, mel, beta, out);
  else if (TF == 8)
    run<8, MAX_NE>(blob, sz, F, T, n_iter, eta, power, mel, beta, out);
  else
    run<4, MAX_NE>(blob, sz, F, T, n_iter, eta, power, mel, beta, out);
  double e_max = 0, e_sq = 0;
  for (size_t i = 0; i < out.size(); ++i) {
    const double d = (double)out[i] - want[i];
    e_max = std::fabs(d) > e_max ? std::fabs(d) : e_max;
    e_sq += d * d;
  }
  const double e_rms = std::sqrt(e_sq / (double)out.size());
  std::printf("%s: n_mels %d F %d T %d n_iter %d TF %d rows %d nnz %d: max %.3e (oracle f32 %.3e) rms %.3e (oracle f32 %.3e)\n",
              path, n_mels, F, T, n_iter, TF, sz.n_act, sz.nnz, e_max, yard[0], e_rms, yard[1]);
  if (yard[0] == 0.0) {
    EXPECT(e_max == 0.0, "%s: the yardstick is exact, the tile run is not", path);
  } else {
    EXPECT(e_max <= 4.0 * yard[0] && e_rms <= 4.0 * yard[1], "%s: beyond 4 x the float32 yardstick", path);
  }
  // bins no row covers: exactly 0
  const View v = view(blob.data(), sz.n_act, F, sz.nnz);
  for (int b = 0; b < F; ++b)
    if (((v.bins[b] >> 9) & 7) == 0)
      for (int t = 0; t < T; ++t) EXPECT(out[(size_t)b * T + t] == 0.f, "%s: uncovered bin %d is not 0", path, b);
}

static void refusals() {
  const int n = 8, F = 129;
  std::vector<float> tri((size_t)n * F, 0.f);
  for (int r = 0; r < n; ++r)
    for (int k = 0; k < 24; ++k) tri[(size_t)r * F + 12 * r + k] = 1.f + (float)k;
  EXPECT(served(tri.data(), F, n, F, 2.f), "a banded bank with two rows over a bin is refused");
  EXPECT(!served(tri.data(), F, n, F, 0.f) && !served(tri.data(), F, n, F, -1.f), "power <= 0 is served");
  std::vector<float> dense((size_t)n * F, 1.f);
  EXPECT(!served(dense.data(), F, n, F, 2.f), "a dense bank is served");
  std::vector<float> gap = tri;
  gap[(size_t)3 * F + 36 + 5] = 0.f;
  EXPECT(!served(gap.data(), F, n, F, 2.f), "a bank with a gap inside a row is served");
  std::vector<float> swapped = tri;
  for (int k = 0; k < F; ++k) std::swap(swapped[(size_t)2 * F + k], swapped[(size_t)5 * F + k]);
  EXPECT(!served(swapped.data(), F, n, F, 2.f), "a bank whose row starts decrease is served");
  std::vector<float> wide((size_t)2 * 4097, 0.f);
  wide[0] = wide[4097 + 1] = 1.f;
  EXPECT(!served(wide.data(), 4097, 2, 4097, 2.f), "F = 4097 is served");
  EXPECT(served(wide.data(), 4097, 2, 2049, 2.f), "F = 2049 is refused");
  std::vector<float> tall((size_t)257 * 300, 0.f);
  for (int r = 0; r < 257; ++r) tall[(size_t)r * 300 + r] = 1.f;
  EXPECT(!served(tall.data(), 300, 257, 300, 2.f), "n_mels = 257 is served");
  EXPECT(served(tall.data(), 300, 256, 300, 2.f), "n_mels = 256 is refused");
  // five rows over one bin: beyond MAX_COVER
  std::vector<float> five((size_t)5 * 16, 0.f);
  for (int r = 0; r < 5; ++r)
    for (int k = r; k < r + 6; ++k) five[(size_t)r * 16 + k] = 1.f;
  EXPECT(!served(five.data(), 16, 5, 16, 2.f), "five rows over a bin are served");
  EXPECT(served(five.data(), 16, 4, 16, 2.f), "four rows over a bin are refused");
  // an all-zero bank: no active row, served (the caller returns zeros: L == 0)
  std::vector<float> zero((size_t)4 * 16, 0.f);
  Sizes sz;
  EXPECT(build_tables(zero.data(), 16, 4, 16, sz, nullptr) && sz.n_act == 0 && sz.nnz == 0, "an all-zero bank");
}

int main(int argc, char **argv) {
  refusals();
  for (int i = 1; i < argc; ++i) run_case(argv[i]);
  std::printf(failures ? "%d FAILURES\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
