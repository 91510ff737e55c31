// pcen.h -- the arithmetic of per-channel energy normalisation (pcen.hip; Wang et al. 2017, librosa.pcen with max_size = 1):
// for a non-negative row S[0 .. T) of a spectrogram
//   M[-1] = S[0] (or a given state);   M[t] = a M[t-1] + b S[t],  a = 1 - b
//   out[t] = (S[t] (eps + M[t])^(-gain) + bias)^power - bias^power
// and its backward.  Plain C++ like mel_nnls.h / cfp_fft.h: the kernels and the host model (host_forward_row /
// host_backward_row: the 64 lanes of a wave run one after the other; mispec_pcen_host_f32 and
// tests/native/pcen_harness.cpp) call the same functions, so the order of every sum is tested without a GPU.
//
// The recurrence as a scan.  A wave owns a row and walks it in chunks of W = 64 frames, lane i on frame t0 + i:
//   v_i = b S_i;   six Kogge-Stone steps  v_i += a^(2^k) v_(i - 2^k)  (lanes i >= 2^k)   ->  v_i = sum_{j <= i} a^(i-j) b S_j
//   M_i = v_i + a^(i+1) carry,   carry = M of the frame before the chunk;   the next carry is M_63
// Every step is ONE fma (scan_step), on the device and on the host.  The factors a^(2^k) come from repeated squaring
// (Row::f) and a^n, 1 <= n <= 64, from the product of the squarings n's bits select, lowest bit first (lane_factor):
// products of a few numbers, never a power function, the same bits wherever they are computed.
// The backward runs the adjoint recurrence  lambda[t] = gM[t] + a lambda[t+1]  the same way from the last chunk to the
// first, lane i taking from lane i + 2^k, the carry entering as a^(64-i) lambda[t0 + 64].
//
// Arithmetic: FLOAT64 between the loads and the stores -- the scan, the two powers, M as the backward reads it -- and one
// rounding to float32 at each store.  The float32 form of these kernels (float32 scan, accurate powf) met the suite's
// rule, 4 x the error of a sequential float32 run, on every case of many elements and missed it at a row of two frames
// (12.6 x): with one or two elements the float32 yardstick is now and then exact to a tenth of an ulp, and only the
// correctly rounded result stays within 4 x of that.  DESIGN.md 3.18 has the figures and what float64 costs.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PCEN_HD __host__ __device__ __forceinline__
#else
#define PCEN_HD inline
#endif

namespace pcen {

constexpr int W = 64;      // frames of a chunk: the lanes of a wave
constexpr int STEPS = 6;   // log2 W

// what a row needs of its channel's parameters
struct Row {
  float gain, power, eps;
  double bias, b, a;
  double lb, bp, cb;    // ln bias, bias^power, power bias^(power - 1)   (bias = 0: 0, 0 and the limit of the last)
  double f[STEPS + 1];  // a^(2^k), k = 0 .. 6
};

// x^y for x >= 0 as exp(y ln x), with x^0 = 1 also at x = 0 (0 * -inf is not a number)
PCEN_HD double pow64(double x, double y) { return y == 0.0 ? 1.0 : ::exp(y * ::log(x)); }

PCEN_HD Row make_row(float b, float gain, float bias, float power, float eps) {
  Row r;
  r.b = (double)b;
  r.a = 1.0 - (double)b;
  r.gain = gain;
  r.bias = (double)bias;
  r.power = power;
  r.eps = eps;
  r.lb = bias > 0.0f ? ::log(r.bias) : 0.0;
  r.bp = bias > 0.0f ? ::exp((double)power * r.lb) : 0.0;
  r.cb = (double)power * pow64(r.bias, (double)power - 1.0);
  r.f[0] = r.a;
  for (int k = 1; k <= STEPS; ++k) r.f[k] = r.f[k - 1] * r.f[k - 1];
  return r;
}

// a^n for 1 <= n <= 64
PCEN_HD double lane_factor(const Row &r, int n) {
  double p = 1.0;
  for (int k = 0; k <= STEPS; ++k)
    if ((n >> k) & 1) p *= r.f[k];
  return p;
}

PCEN_HD double scan_input(const Row &r, float s) { return r.b * (double)s; }
// one Kogge-Stone step / the carry's entry: v + factor * other, one rounding
PCEN_HD double scan_step(double factor, double other, double v) { return ::fma(factor, other, v); }

// The pointwise part in float64, rounded once.  With P = S (eps + M)^(-gain) and x = P / bias
//   (P + bias)^power - bias^power = bias^power expm1(power log1p(x))
// which has no cancellation for P << bias and is exactly 0 at P = 0 (an all-zero input) by construction, not by two
// evaluations of a power agreeing in their last bit.  bias = 0 (the same for a whole row) is P^power.
PCEN_HD float output(const Row &r, float s, double m) {
  const double p = (double)s * ::exp(-(double)r.gain * ::log((double)r.eps + m));
  if (r.bias > 0.0) return (float)(r.bp * ::expm1((double)r.power * ::log1p(p / r.bias)));
  return (float)pow64(p, (double)r.power);
}

// The backward of one element for the output gradient g: the direct part of dS, the gradient that enters the adjoint
// recurrence at this frame (d out / d M) and the three pointwise parameter gradients, all float64.  With L = log1p(x),
// em = expm1((power - 1) L) and E = (1 + em)(1 + x) - 1 = expm1(power L):
//   c = power (P + bias)^(power - 1) = cb (1 + em)
//   d / d bias  = c - cb = cb em
//   d / d power = (P + bias)^power ln(P + bias) - bias^power ln bias = bias^power (E ln bias + (1 + E) L)
// again exactly 0 at P = 0.
struct Point {
  double ds, gm, dgain, dbias, dpower;
};

PCEN_HD Point backward_point(const Row &r, float s, double m, float g) {
  const double u = (double)r.eps + m, lu = ::log(u);
  const double q = ::exp(-(double)r.gain * lu);
  const double p = (double)s * q;
  double c, dbias, dpower;
  if (r.bias > 0.0) {
    const double x = p / r.bias, L = ::log1p(x);
    const double em = ::expm1(((double)r.power - 1.0) * L);
    const double E = ::fma(1.0 + em, x, em);
    c = ::fma(r.cb, em, r.cb);
    dbias = r.cb * em;
    dpower = r.bp * (E * r.lb + (1.0 + E) * L);
  } else {
    c = (double)r.power * pow64(p, (double)r.power - 1.0);
    dbias = c - r.cb;
    dpower = p > 0.0 ? pow64(p, (double)r.power) * ::log(p) : 0.0;
  }
  const double gc = (double)g * c;
  Point o;
  o.ds = gc * q;
  o.gm = -(double)r.gain * gc * p / u;
  o.dgain = -gc * p * lu;
  o.dbias = (double)g * dbias;
  o.dpower = (double)g * dpower;
  return o;
}

// ---- the host model: one row, the lanes of a chunk one after the other ---------------------------------------------

// s[0 .. T), out[0 .. T), m_out[0 .. T) or NULL; state: M[-1] or NULL (then S[0]); state_out: M[T-1] or NULL
inline void host_forward_row(const Row &r, const float *s, long long T, const float *state, float *out, double *m_out,
                             float *state_out) {
  double carry = state ? *state : s[0];
  double v[W];
  for (long long t0 = 0; t0 < T; t0 += W) {
    for (int i = 0; i < W; ++i) v[i] = scan_input(r, t0 + i < T ? s[t0 + i] : 0.0f);
    for (int k = 0; k < STEPS; ++k)
      for (int i = W - 1; i >= (1 << k); --i) v[i] = scan_step(r.f[k], v[i - (1 << k)], v[i]);  // (descending: old values)
    for (int i = 0; i < W; ++i) v[i] = scan_step(lane_factor(r, i + 1), carry, v[i]);
    for (int i = 0; i < W && t0 + i < T; ++i) {
      out[t0 + i] = output(r, s[t0 + i], v[i]);
      if (m_out) m_out[t0 + i] = v[i];
    }
    carry = v[W - 1];
  }
  if (state_out) *state_out = (float)v[(T - 1) % W];
}

// ds[0 .. T); sums[4] = db, dgain, dbias, dpower of the row; dstate: NULL when no state was given (then a lambda[0]
// goes to ds[0])
inline void host_backward_row(const Row &r, const float *s, const double *m, const float *g, long long T, const float *state,
                              float *ds, float *dstate, double sums[4]) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double carry = 0.0, lam[W], direct[W];
  const double first = state ? *state : s[0];
  for (long long t0 = (T - 1) / W * W; t0 >= 0; t0 -= W) {
    for (int i = 0; i < W; ++i) {
      lam[i] = direct[i] = 0.0;
      if (t0 + i < T) {
        const Point o = backward_point(r, s[t0 + i], m[t0 + i], g[t0 + i]);
        lam[i] = o.gm;
        direct[i] = o.ds;
        acc[1] += o.dgain;
        acc[2] += o.dbias;
        acc[3] += o.dpower;
      }
    }
    for (int k = 0; k < STEPS; ++k)
      for (int i = 0; i + (1 << k) < W; ++i) lam[i] = scan_step(r.f[k], lam[i + (1 << k)], lam[i]);  // (ascending: old values)
    for (int i = 0; i < W; ++i) lam[i] = scan_step(lane_factor(r, W - i), carry, lam[i]);
    for (int i = 0; i < W && t0 + i < T; ++i) {
      const long long t = t0 + i;
      const double prev = t > 0 ? m[t - 1] : first;
      acc[0] += lam[i] * ((double)s[t] - prev);
      double d = scan_step(r.b, lam[i], direct[i]);
      if (t == 0) {
        const double tail = r.a * lam[i];  // d / d M[-1]
        if (dstate)
          *dstate = (float)tail;
        else
          d += tail;
      }
      ds[t] = (float)d;
    }
    carry = lam[0];
  }
  for (int j = 0; j < 4; ++j) sums[j] = acc[j];
}
}  // namespace pcen
