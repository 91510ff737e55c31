// pcen.hip -- per-channel energy normalisation and its backward, one launch each: mispec_pcen_f32 / mispec_pcen_bwd_f32 /
// mispec_pcen_host_f32 of include/mispec.h, behind features.PCEN.  The arithmetic, the scan and the host model: pcen.h.
//
// The smoother is a first-order recurrence along time: as torch operators a loop of T launches.  Here ONE WAVE owns a row
// (clip, channel) and walks it in chunks of 64 frames, lane i on frame t0 + i -- every load and store of a wave is 256
// contiguous bytes -- and solves the recurrence inside the chunk by six shuffle steps, in float64 with one rounding at
// the store (pcen.h says why).  The next chunk's load is issued before the current chunk is scanned.  No LDS, no barrier, no atomics; a workgroup is ROWS_PER_BLOCK independent
// waves.  The backward walks the chunks from the last to the first with the adjoint recurrence, keeps the four parameter
// gradients per lane in float64 and reduces them over the wave once per row: lane 0 writes the row's four sums with one
// vector store to the (rows, 4) workspace, which the caller sums over the clips.
// Bounds: frame t of a row is touched only when t < T (every load and store below is predicated on it), rows only when
// row < n_clips * n_rows; offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "mispec.h"
#include "mispec_internal.h"
#include "pcen.h"

namespace {

using namespace pcen;

constexpr int ROWS_PER_BLOCK = 4;

struct PcenParams {
  const float *s;
  long long s_clip_stride, s_row_stride;
  const float *b, *gain, *bias, *power;
  float eps;
  int n_params, F;
  long long rows, T;
  const float *state_in;
  float *out;
  long long out_clip_stride, out_row_stride;
  double *m_out;
  float *state_out;
  // backward
  const double *m;
  const float *g;
  long long g_clip_stride, g_row_stride;
  float *ds;
  long long ds_clip_stride, ds_row_stride;
  float *dstate;
  double *sums;
};

__device__ __forceinline__ Row row_of(const PcenParams &p, int f) {
  const int c = p.n_params == 1 ? 0 : f;
  return make_row(p.b[c], p.gain[c], p.bias[c], p.power[c], p.eps);
}

__global__ __launch_bounds__(W *ROWS_PER_BLOCK) void pcen_fwd_kernel(const PcenParams p) {
  const int lane = threadIdx.x % W;
  const long long row = (long long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / W;
  if (row >= p.rows) return;  // (a whole wave: no barrier follows)
  const long long clip = row / p.F;
  const int f = (int)(row % p.F);
  const Row r = row_of(p, f);
  const float *s = p.s + clip * p.s_clip_stride + f * p.s_row_stride;
  float *out = p.out + clip * p.out_clip_stride + f * p.out_row_stride;
  double *m_out = p.m_out ? p.m_out + row * p.T : nullptr;
  const double up = lane_factor(r, lane + 1);

  double carry = p.state_in ? p.state_in[row] : s[0];
  float s_next = lane < p.T ? s[lane] : 0.0f;
  double m = 0.0;
  for (long long t0 = 0; t0 < p.T; t0 += W) {
    const long long t = t0 + lane;
    const float sv = s_next;
    s_next = t + W < p.T ? s[t + W] : 0.0f;
    double v = scan_input(r, sv);
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
      const double other = __shfl_up(v, 1u << k);
      if (lane >= (1 << k)) v = scan_step(r.f[k], other, v);
    }
    m = scan_step(up, carry, v);
    if (t < p.T) {
      out[t] = output(r, sv, m);
      if (m_out) m_out[t] = m;
    }
    carry = __shfl(m, W - 1);
  }
  if (p.state_out && lane == (int)((p.T - 1) % W)) p.state_out[row] = (float)m;
}

__global__ __launch_bounds__(W *ROWS_PER_BLOCK) void pcen_bwd_kernel(const PcenParams p) {
  const int lane = threadIdx.x % W;
  const long long row = (long long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / W;
  if (row >= p.rows) return;
  const long long clip = row / p.F;
  const int f = (int)(row % p.F);
  const Row r = row_of(p, f);
  const float *s = p.s + clip * p.s_clip_stride + f * p.s_row_stride;
  const float *g = p.g + clip * p.g_clip_stride + f * p.g_row_stride;
  const double *mrow = p.m + row * p.T;
  float *ds = p.ds + clip * p.ds_clip_stride + f * p.ds_row_stride;
  const double down = lane_factor(r, W - lane);
  const double first = p.state_in ? p.state_in[row] : s[0];

  double acc_b = 0.0, acc_gain = 0.0, acc_bias = 0.0, acc_power = 0.0;
  double carry = 0.0;
  long long t0 = (p.T - 1) / W * W;
  long long t = t0 + lane;
  float s_next = t < p.T ? s[t] : 0.0f, g_next = t < p.T ? g[t] : 0.0f;
  double m_next = t < p.T ? mrow[t] : 0.0;
  for (; t0 >= 0; t0 -= W) {
    t = t0 + lane;
    const float sv = s_next, gv = g_next;
    const double mv = m_next;
    if (t0 >= W) {  // (the chunks before the last one are whole)
      s_next = s[t - W];
      m_next = mrow[t - W];
      g_next = g[t - W];
    }
    double lam = 0.0, direct = 0.0;
    if (t < p.T) {
      const Point o = backward_point(r, sv, mv, gv);
      lam = o.gm;
      direct = o.ds;
      acc_gain += o.dgain;
      acc_bias += o.dbias;
      acc_power += o.dpower;
    }
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
      const double other = __shfl_down(lam, 1u << k);
      if (lane + (1 << k) < W) lam = scan_step(r.f[k], other, lam);
    }
    lam = scan_step(down, carry, lam);
    double prev = __shfl_up(mv, 1u);
    if (lane == 0) prev = t0 > 0 ? mrow[t0 - 1] : first;
    if (t < p.T) {
      acc_b += lam * ((double)sv - prev);
      double d = scan_step(r.b, lam, direct);
      if (t == 0) {
        const double tail = r.a * lam;  // d / d M[-1]
        if (p.dstate)
          p.dstate[row] = (float)tail;
        else
          d += tail;
      }
      ds[t] = (float)d;
    }
    carry = __shfl(lam, 0);
  }
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) {
    acc_b += __shfl_down(acc_b, d);
    acc_gain += __shfl_down(acc_gain, d);
    acc_bias += __shfl_down(acc_bias, d);
    acc_power += __shfl_down(acc_power, d);
  }
  if (lane == 0) *reinterpret_cast<double4 *>(p.sums + 4 * row) = make_double4(acc_b, acc_gain, acc_bias, acc_power);
}

const char *check(const mispec_pcen_args *a, bool backward) {
  if (a == nullptr) return "NULL argument block";
  if (a->struct_size != sizeof(mispec_pcen_args)) return "struct_size does not match this library's mispec_pcen_args";
  if (a->reserved != 0) return "reserved must be 0";
  if (!a->s || !a->b || !a->gain || !a->bias || !a->power) return "NULL pointer (s, b, gain, bias or power)";
  if (a->n_clips <= 0 || a->n_rows <= 0 || a->n_frames <= 0) return "non-positive size";
  if (a->n_params != 1 && a->n_params != a->n_rows) return "n_params must be 1 or n_rows";
  if (!(a->eps > 0.0f)) return "eps must be > 0";
  if (a->s_row_stride < a->n_frames || a->s_clip_stride < (int64_t)a->n_rows * a->s_row_stride)
    return "a stride of s shorter than its row";
  if (!backward) {
    if (!a->out) return "NULL pointer (out)";
    if (a->out_row_stride < a->n_frames || a->out_clip_stride < (int64_t)a->n_rows * a->out_row_stride)
      return "a stride of out shorter than its row";
  } else {
    if (!a->m || !a->grad_out || !a->grad_s || !a->sums) return "NULL pointer (m, grad_out, grad_s or sums)";
    if ((a->state_in == nullptr) != (a->grad_state == nullptr)) return "grad_state goes with state_in";
    if (a->grad_out_row_stride < a->n_frames || a->grad_out_clip_stride < (int64_t)a->n_rows * a->grad_out_row_stride ||
        a->grad_s_row_stride < a->n_frames || a->grad_s_clip_stride < (int64_t)a->n_rows * a->grad_s_row_stride)
      return "a stride of grad_out or grad_s shorter than its row";
  }
  return nullptr;
}

int fail(const char *fn, int code, const char *what) {
  static thread_local char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", fn, what);
  return mispec_fail_msg(code, msg);
}

PcenParams params_of(const mispec_pcen_args *a) {
  PcenParams p{};
  p.s = a->s;
  p.s_clip_stride = a->s_clip_stride;
  p.s_row_stride = a->s_row_stride;
  p.b = a->b;
  p.gain = a->gain;
  p.bias = a->bias;
  p.power = a->power;
  p.eps = a->eps;
  p.n_params = a->n_params;
  p.F = a->n_rows;
  p.rows = (long long)a->n_clips * a->n_rows;
  p.T = a->n_frames;
  p.state_in = a->state_in;
  p.out = a->out;
  p.out_clip_stride = a->out_clip_stride;
  p.out_row_stride = a->out_row_stride;
  p.m_out = a->m_out;
  p.state_out = a->state_out;
  p.m = a->m;
  p.g = a->grad_out;
  p.g_clip_stride = a->grad_out_clip_stride;
  p.g_row_stride = a->grad_out_row_stride;
  p.ds = a->grad_s;
  p.ds_clip_stride = a->grad_s_clip_stride;
  p.ds_row_stride = a->grad_s_row_stride;
  p.dstate = a->grad_state;
  p.sums = a->sums;
  return p;
}

int launch(const char *fn, const mispec_pcen_args *a, void *stream, bool backward) {
  if (const char *what = check(a, backward)) return fail(fn, MISPEC_E_INVALID, what);
  const PcenParams p = params_of(a);
  const long long blocks = (p.rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return fail(fn, MISPEC_E_UNSUPPORTED, "more than 2^33 rows in one call");
  hipLaunchKernelGGL(backward ? pcen_bwd_kernel : pcen_fwd_kernel, dim3((unsigned)blocks), dim3(W * ROWS_PER_BLOCK), 0,
                     static_cast<hipStream_t>(stream), p);
  if (hipGetLastError() != hipSuccess) return fail(fn, MISPEC_E_HIP, "launch failed");
  return MISPEC_OK;
}

}  // namespace

extern "C" {

int mispec_pcen_f32(const mispec_pcen_args *a, void *stream) { return launch("mispec_pcen_f32", a, stream, false); }

int mispec_pcen_bwd_f32(const mispec_pcen_args *a, void *stream) { return launch("mispec_pcen_bwd_f32", a, stream, true); }

int mispec_pcen_host_f32(const mispec_pcen_args *a) {
  if (const char *what = check(a, false)) return fail("mispec_pcen_host_f32", MISPEC_E_INVALID, what);
  const long long rows = (long long)a->n_clips * a->n_rows;
  for (long long row = 0; row < rows; ++row) {
    const long long clip = row / a->n_rows;
    const int f = (int)(row % a->n_rows);
    const int c = a->n_params == 1 ? 0 : f;
    const Row r = make_row(a->b[c], a->gain[c], a->bias[c], a->power[c], a->eps);
    host_forward_row(r, a->s + clip * a->s_clip_stride + f * a->s_row_stride, a->n_frames,
                     a->state_in ? a->state_in + row : nullptr, a->out + clip * a->out_clip_stride + f * a->out_row_stride,
                     a->m_out ? a->m_out + row * a->n_frames : nullptr, a->state_out ? a->state_out + row : nullptr);
  }
  return MISPEC_OK;
}

}  // extern "C"
