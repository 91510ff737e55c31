// Host harness of nnaudio_amd/csrc/cfp_fft.h: the NT threads of the CFP kernel's workgroup run one after the other
// (every thread's pass_load, then every thread's pass_store: the barrier between them), on the plans make_plan gives,
// and the results are compared with float64 DFTs:
//   1. the complex transform of every served N asked for;
//   2. the magnitudes of a real frame's transform;
//   3. two rectified (cut) sequences packed after even_part: real / imaginary part of the transform against the real
//      part of each sequence's own float64 DFT -- and the same WITHOUT it must be wrong (the test has teeth).
// Exit status 0 = all within tolerance.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cfp_fft.h"

using cfpfft::cf;
typedef std::complex<double> cd;

// (the register file sized for CAP: N <= HALF_N runs as the two-workgroups-per-CU kernel, the rest as the large one)
template <int R, int CAP>
static void run_pass_cap(std::vector<cf> &buf, int N, int s, const cf *tw) {
  typedef cf Regs[cfpfft::per_thread<R, CAP>()][R];
  std::vector<char> store(sizeof(Regs) * cfpfft::NT);
  Regs *regs = reinterpret_cast<Regs *>(store.data());
  for (int tid = 0; tid < cfpfft::NT; ++tid) cfpfft::pass_load<R, CAP>(buf.data(), N, tid, regs[tid]);
  for (int tid = 0; tid < cfpfft::NT; ++tid) cfpfft::pass_store<R, CAP>(buf.data(), N, s, tw, tid, regs[tid]);
}

template <int R>
static void run_pass(std::vector<cf> &buf, int N, int s, const cf *tw) {
  if (N <= cfpfft::HALF_N)
    run_pass_cap<R, cfpfft::HALF_CAP>(buf, N, s, tw);
  else
    run_pass_cap<R, cfpfft::MAX_N>(buf, N, s, tw);
}

static bool fft(std::vector<cf> &buf, int N, const std::vector<float> &tw) {
  cfpfft::Plan pl;
  if (!cfpfft::make_plan(N, pl)) return false;
  const cf *t = reinterpret_cast<const cf *>(tw.data());
  int s = 1;
  for (int i = 0; i < pl.n_pass; ++i) {
    switch (pl.radix[i]) {
      case 2: run_pass<2>(buf, N, s, t); break;
      case 4: run_pass<4>(buf, N, s, t); break;
      case 5: run_pass<5>(buf, N, s, t); break;
      case 8: run_pass<8>(buf, N, s, t); break;
      case 10: run_pass<10>(buf, N, s, t); break;
      case 16: run_pass<16>(buf, N, s, t); break;
      default: return false;
    }
    s *= pl.radix[i];
  }
  return s == N;
}

// float64 DFT by a table of the N roots
static std::vector<cd> dft64(const std::vector<cd> &x) {
  const int N = (int)x.size();
  std::vector<cd> w(N), y(N);
  for (int k = 0; k < N; ++k) w[k] = std::polar(1.0, -2.0 * M_PI * k / N);
  for (int k = 0; k < N; ++k) {
    cd acc = 0;
    long idx = 0;
    for (int n = 0; n < N; ++n) {
      acc += x[n] * w[idx];
      idx += k;
      if (idx >= N) idx -= N;
    }
    y[k] = acc;
  }
  return y;
}

static double rnd() { return (double)std::rand() / RAND_MAX * 2.0 - 1.0; }

static int failures = 0;
static void report(const char *what, int N, double err, double tol) {
  const bool ok = err <= tol;
  std::printf("%-34s N=%-6d err/peak %.3e (tol %.1e) %s\n", what, N, err, tol, ok ? "ok" : "FAIL");
  if (!ok) ++failures;
}

static void check_size(int N, bool packing) {
  cfpfft::Plan pl;
  if (!cfpfft::make_plan(N, pl)) {
    std::printf("no plan for N=%d FAIL\n", N);
    ++failures;
    return;
  }
  std::printf("N=%d plan:", N);
  for (int i = 0; i < pl.n_pass; ++i) std::printf(" %d", pl.radix[i]);
  std::printf("\n");
  std::vector<float> tw(2 * N);
  cfpfft::make_twiddles(N, tw.data());
  // fp32 FFT error ~ eps sqrt(log N) of the RMS output; bound it at 2e-6 of the peak
  {
    std::vector<cf> buf(N);
    std::vector<cd> x(N);
    for (int n = 0; n < N; ++n) {
      buf[n] = cf{(float)rnd(), (float)rnd()};
      x[n] = cd(buf[n].x, buf[n].y);
    }
    if (!fft(buf, N, tw)) {
      std::printf("fft failed FAIL\n");
      ++failures;
      return;
    }
    const std::vector<cd> y = dft64(x);
    double err = 0, peak = 0;
    for (int k = 0; k < N; ++k) {
      err = std::fmax(err, std::abs(cd(buf[k].x, buf[k].y) - y[k]));
      peak = std::fmax(peak, std::abs(y[k]));
    }
    report("complex transform", N, err / peak, 2e-6);
  }
  if (!packing) return;
  {  // a real frame (imaginary part zero): magnitudes of bins 0 .. N / 2
    std::vector<cf> buf(N);
    std::vector<cd> a(N);
    for (int n = 0; n < N; ++n) {
      buf[n] = cf{(float)rnd(), 0.f};
      a[n] = buf[n].x;
    }
    fft(buf, N, tw);
    const std::vector<cd> A = dft64(a);
    double err = 0, peak = 0;
    for (int k = 0; k <= N / 2; ++k) {
      err = std::fmax(err, std::fabs(cfpfft::magnitude(buf[k], 0.25f) - 0.25 * std::abs(A[k])));
      peak = std::fmax(peak, 0.25 * std::abs(A[k]));
    }
    report("real frame, magnitudes", N, err / peak, 2e-6);
  }
  for (int c : {N / 100 + 1, 0}) {  // rectified even sequences, packed; cutoff 0 zeroes everything
    std::vector<cf> buf(N), raw(N);
    std::vector<cd> a(N), b(N);
    for (int n = 0; n <= N / 2; ++n) {
      const int nn = n == 0 ? 0 : N - n;
      cf v = cf{(float)rnd(), (float)rnd()};  // an even sequence per component, both signs
      if (n == c) v = cf{std::fabs(v.x) + 0.1f, std::fabs(v.y) + 0.1f};  // (the bin at the cut's edge survives the relu)
      for (int k : {n, nn}) {
        const bool z = cfpfft::cut(k, N, c);
        buf[k] = cf{cfpfft::rectify(v.x, 0.6f, z), cfpfft::rectify(v.y, 0.6f, z)};
        a[k] = buf[k].x;
        b[k] = buf[k].y;
      }
    }
    raw = buf;
    for (int k = 1; 2 * k < N; ++k) buf[k] = buf[N - k] = cfpfft::even_part(buf[k], buf[N - k]);
    fft(buf, N, tw);
    fft(raw, N, tw);
    const std::vector<cd> A = dft64(a), B = dft64(b);
    double err = 0, err_raw = 0, peak = 0;
    for (int k = 0; k < N; ++k) {
      err = std::fmax(err, std::fmax(std::fabs(buf[k].x - A[k].real()), std::fabs(buf[k].y - B[k].real())));
      err_raw = std::fmax(err_raw, std::fmax(std::fabs(raw[k].x - A[k].real()), std::fabs(raw[k].y - B[k].real())));
      peak = std::fmax(peak, std::fmax(std::fabs(A[k].real()), std::fabs(B[k].real())));
    }
    if (c == 0) {
      report("cutoff 0: everything zero", N, err + peak, 0.0);
    } else {
      report("rectified even frames, packed", N, err / peak, 2e-6);
      if (!(err_raw > 100 * err)) {
        std::printf("the packing without the even part should be wrong (%.3e vs %.3e) FAIL\n", err_raw, err);
        ++failures;
      }
    }
  }
}

int main() {
  std::srand(1234);
  for (int N : {4000, 8000, 16000}) check_size(N, true);
  for (int N : {16, 20, 40, 50, 64, 80, 100, 160, 250, 320, 400, 512, 640, 1000, 1250, 2000, 2048, 3200, 6250, 10000, 12800})
    check_size(N, N <= 2048);
  // what is not served
  cfpfft::Plan pl;
  for (int N : {22050, 24, 7, 0}) {
    if (cfpfft::make_plan(N, pl)) {
      std::printf("make_plan accepted N=%d FAIL\n", N);
      ++failures;
    }
  }
  if (cfpfft::served(32000, 2049, 174, 3, false) || cfpfft::served(20000, 2049, 174, 3, false) ||
      cfpfft::served(8000, 8001, 174, 3, false) || cfpfft::served(8000, 2049, 300, 3, false) ||
      cfpfft::served(8000, 2049, 174, 1, false) || cfpfft::served(3125, 2049, 174, 3, false) ||
      cfpfft::served(8000, 2049, 174, 3, true) || !cfpfft::served(8000, 2049, 174, 3, false) ||
      !cfpfft::served(4000, 2049, 174, 2, false) || !cfpfft::served(16000, 2049, 174, 8, false)) {
    std::printf("served() FAIL\n");
    ++failures;
  }
  std::printf(failures ? "%d FAILURES\n" : "all ok\n", failures);
  return failures ? 1 : 0;
}
