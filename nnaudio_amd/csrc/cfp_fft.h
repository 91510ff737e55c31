// cfp_fft.h -- arithmetic of the CFP kernel (cfp.hip): a mixed-radix Stockham FFT of N = 2^a 5^b complex points in ONE
// N-point buffer, as NT threads run it ("read a pass's inputs into registers, barrier, write"), the rectifier, and the
// two-frames-per-transform packing of the transforms behind the first (the even part taken after the rectifier).
// Plain C++ like fft_core.h: tests/native/cfp_fft_harness.cpp compiles the same functions for the host, runs the NT
// threads one after the other and compares with a float64 DFT -- plans and index arithmetic are tested without a GPU.
//
// Pass of radix R at stride s (s = product of the radices before it, n = N / s points per sub-transform, m = n / R):
// butterfly i = p s + q  (q < s, p < m)  reads   x[i + j N / R],       j < R   (consecutive threads: consecutive words)
//                                        writes  y[q + s (R p + k)] = W_n^(p k) sum_j x_j W_R^(j k),  k < R
// and W_n^(p k) = W_N^(p k s) with p k s < N: one table of N twiddles, no modulo.  Decimation in frequency, natural
// order in and out after the last pass, any order of the radices.
#pragma once

#include <cmath>

#include "fft_core.h"

namespace cfpfft {

using fftcore::cf;
using fftcore::cmul;

// LDS of a workgroup: the N-point complex buffer and N / 2 + 1 floats (the first frame's magnitudes while the second
// frame is transformed): 10 N + 4 bytes.  MAX_N: what fits the 160 KB a workgroup can get; HALF_N: what fits twice.
constexpr int MAX_N = 16000;
constexpr int HALF_N = 8000;
// register slots of the HALF_N kernel are sized as for N = 10000 (one idle butterfly slot in the radix 2 / 4 / 8 passes):
// sized for 8000 exactly, hipcc 7 keeps the butterfly arrays in scratch (680 bytes per lane) instead of 113 VGPRs
constexpr int HALF_CAP = 10000;
constexpr long lds_bytes(int N) { return (long)N * 8 + ((long)N / 2 + 1) * 4; }
static_assert(lds_bytes(MAX_N) <= 160 * 1024 && 2 * lds_bytes(HALF_N) <= 160 * 1024, "LDS");
constexpr int MIN_N = 16;
constexpr int NT = 512;        // threads of a workgroup
constexpr int MAX_PASSES = 16;
constexpr int MAX_LAYERS = 8;

struct Plan {
  int n_pass;
  int radix[MAX_PASSES];
};

// N = 2^a 5^b -> radix passes: 10s while both primes are left, then 5s; the remaining 2s as 16 / 8 / 4 / 2 with as few
// passes as possible; the powers of two first.  False for any other N (or more than MAX_PASSES passes).
// N <= HALF_N (the kernel with two workgroups per CU and 128 registers) does without radix 16: 16 -> 4.4, 16.8 -> 8.4.4.
inline bool make_plan(int N, Plan &pl) {
  pl.n_pass = 0;
  if (N < 1) return false;
  const bool small = N <= HALF_N;
  int a = 0, b = 0;
  while (N % 2 == 0) N /= 2, ++a;
  while (N % 5 == 0) N /= 5, ++b;
  if (N != 1) return false;
  const int tens = a < b ? a : b;
  a -= tens;
  b -= tens;
  int twos[MAX_PASSES], n2 = 0;
  while (a > 0) {
    int e = a >= 7 || a == 4 ? 4 : a >= 5 ? 3 : a;  // 5 -> 8.4, 6 -> 8.8, 7 -> 16.8
    if (small && e == 4) e = a == 4 ? 2 : 3;
    if (n2 == MAX_PASSES) return false;
    twos[n2++] = 1 << e;
    a -= e;
  }
  if (n2 + tens + b > MAX_PASSES) return false;
  for (int i = 0; i < n2; ++i) pl.radix[pl.n_pass++] = twos[i];
  for (int i = 0; i < tens; ++i) pl.radix[pl.n_pass++] = 10;
  for (int i = 0; i < b; ++i) pl.radix[pl.n_pass++] = 5;
  return true;
}

// What the kernel serves: see mispec_cfp_served (include/mispec.h).  N even: frame counts as torch.stft has them.
// Not served: a layer with g == 0 (the log rectifier).  Its slope of 1e8 at 0 turns the kernel's rounding -- the partner
// frame's included -- into 14 x (max) / 6 x (RMS) the error the reference's own float32 run has on the fixture with such
// a layer; until that is understood the composition of torch operators keeps it.
inline bool served(int N, int window_size, int n_out, int n_layers, bool log_layer) {
  Plan pl;
  return !log_layer && N >= MIN_N && N <= MAX_N && N % 2 == 0 && make_plan(N, pl) && window_size >= 1 && window_size <= N &&
         n_out >= 1 && 2 * n_out <= NT && n_layers >= 2 && n_layers <= MAX_LAYERS;
}

// exp(-2 pi i k / N), evaluated in float64 and rounded once (host: the table the kernel reads)
inline void make_twiddles(int N, float *dst) {
  const double step = -2.0 * 3.14159265358979323846 / N;
  for (int k = 0; k < N; ++k) {
    dst[2 * k] = (float)std::cos(step * k);
    dst[2 * k + 1] = (float)std::sin(step * k);
  }
}

// ---- DFT_5 and DFT_10 on registers (2, 4, 8, 16: fft_core.h)
FFT_HD void dft5(cf (&v)[5]) {
  constexpr float c1 = 0.30901699437494742f, c2 = -0.80901699437494742f;  // cos(2 pi / 5), cos(4 pi / 5)
  constexpr float s1 = 0.95105651629515357f, s2 = 0.58778525229247313f;   // sin(2 pi / 5), sin(4 pi / 5)
  const cf a1 = v[1] + v[4], b1 = v[1] - v[4], a2 = v[2] + v[3], b2 = v[2] - v[3];
  const cf x0 = v[0];
  const cf r1 = x0 + a1 * c1 + a2 * c2, r2 = x0 + a1 * c2 + a2 * c1;
  const cf i1 = b1 * s1 + b2 * s2, i2 = b1 * s2 - b2 * s1;
  v[0] = x0 + a1 + a2;
  v[1] = cf{r1.x + i1.y, r1.y - i1.x};  // r1 - i (i1)
  v[4] = cf{r1.x - i1.y, r1.y + i1.x};
  v[2] = cf{r2.x + i2.y, r2.y - i2.x};
  v[3] = cf{r2.x - i2.y, r2.y + i2.x};
}

FFT_HD void dft10(cf (&v)[10]) {
  cf e[5] = {v[0], v[2], v[4], v[6], v[8]}, o[5] = {v[1], v[3], v[5], v[7], v[9]};
  dft5(e);
  dft5(o);
  // W_10^k, k = 1 .. 4: (cos, -sin) of pi k / 5
  constexpr float c1 = 0.80901699437494742f, s1 = 0.58778525229247313f, c2 = 0.30901699437494742f, s2 = 0.95105651629515357f;
  const cf w[5] = {cf{1.f, 0.f}, cf{c1, -s1}, cf{c2, -s2}, cf{-c2, -s2}, cf{-c1, -s1}};
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const cf t = k == 0 ? o[0] : cmul(o[k], w[k]);
    v[k] = e[k] + t;
    v[k + 5] = e[k] - t;
  }
}

template <int R>
FFT_HD void dft(cf (&v)[R]) {
  static_assert(R == 2 || R == 4 || R == 5 || R == 8 || R == 10 || R == 16, "radix");
  if constexpr (R == 5)
    dft5(v);
  else if constexpr (R == 10)
    dft10(v);
  else
    fftcore::dft<R>(v);
}

// butterflies a thread holds between the two halves of a pass of radix R, for N up to CAP (the kernel is compiled for
// two caps: HALF_N, where two workgroups share a CU and the registers must stay under 128, and MAX_N)
template <int R, int CAP>
constexpr int per_thread() {
  return (CAP / R + NT - 1) / NT;
}

// First half of a pass, thread `tid`: the inputs of its butterflies tid, tid + NT, ... into registers.
template <int R, int CAP>
FFT_HD void pass_load(const cf *buf, int N, int tid, cf (&v)[per_thread<R, CAP>()][R]) {
  const int nbf = N / R;
#pragma unroll
  for (int b = 0; b < per_thread<R, CAP>(); ++b) {
    const int i = tid + b * NT;
    if (i < nbf) {
#pragma unroll
      for (int j = 0; j < R; ++j) v[b][j] = buf[i + j * nbf];
    }
  }
}

// Second half (after every thread has finished the first): DFT_R, twiddles, outputs to their Stockham positions.
// tw: the N-entry table of make_twiddles.  A pass with m = 1 (the last one) has no twiddles.
template <int R, int CAP>
FFT_HD void pass_store(cf *buf, int N, int s, const cf *tw, int tid, cf (&v)[per_thread<R, CAP>()][R]) {
  const int nbf = N / R;
  const bool twiddled = nbf > s;  // m = N / (s R) > 1
#pragma unroll
  for (int b = 0; b < per_thread<R, CAP>(); ++b) {
    const int i = tid + b * NT;
    if (i < nbf) {
      const int p = i / s, q = i - p * s;
      dft<R>(v[b]);
      cf *dst = buf + q + s * R * p;
      dst[0] = v[b][0];
      const int step = p * s;
#pragma unroll
      for (int k = 1; k < R; ++k) dst[s * k] = twiddled ? cmul(v[b][k], tw[step * k]) : v[b][k];
    }
  }
}

// |z| scale: a bin of the magnitude spectrum (the frame's transform has the conjugate symmetry of a real input, so
// the kernel computes bins 0 .. N / 2 and mirrors them: s0[k] == s0[N - k] exactly)
FFT_HD float magnitude(cf z, float scale) { return sqrtf(z.x * z.x + z.y * z.y) * scale; }

// whether the rectifier zeroes bin k: the first c and the last c bins; c == 0: all (the reference's X[..., -0:] = 0)
FFT_HD bool cut(int k, int N, int c) { return c <= 0 || k < c || k >= N - c; }

FFT_HD float power_law(float x, float g) { return g == 1.f ? x : powf(x, g); }

// nl(X, g, c) of one value (X already divided by sqrt(N)), g != 0
FFT_HD float rectify(float x, float g, bool zeroed) {
  if (zeroed) return 0.f;
  return power_law(x > 0.f ? x : 0.f, g);
}

// ---- two frames per complex transform, from the second transform on
// Only the REAL part of those transforms is kept, and Re DFT(x) = DFT(even part of x), which is real.  So two frames packed
// as even(x_a) + i even(x_b) come out as real part = frame a's result, imaginary part = frame b's, nothing discarded.
// The rectifier's output is even only approximately (rounding of the transform before it, amplified without bound by
// ** g and log at 0) and not at all at the edge of the cut (bin c survives, its mirror N - c does not): the even part is
// TAKEN, (x[k] + x[N - k]) / 2 written to both bins, per component.  Packing without it puts frame b's odd part into
// frame a's result: measured 9 x the reference's own float32 error on tfrLF, and 1e-2 of the peak from the cut's edge.
FFT_HD cf even_part(cf xk, cf xnk) { return (xk + xnk) * 0.5f; }

}  // namespace cfpfft
