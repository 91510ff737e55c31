// cfp.hip -- Combined frequency and periodicity features (the reference's Combined_Frequency_Periodicity / CFP forward,
// cfp.py:129-176) in ONE launch: mispec_cfp_f32 of include/mispec.h.
//
// The reference runs, per frame of N = fs / fr samples (8000 by default), torch.stft, a power law, a full length-N FFT, a
// rectifier, another full length-N FFT and a rectifier, each over a (batch, frames, N) tensor in HBM, and then keeps
// 501 + 501 + 201 of the 3 N values for two small triangular filterbanks.  Here a workgroup takes TWO consecutive frames
// of a clip and keeps the whole chain in one N-point complex buffer in LDS (64 + 16 KB at N = 8000, 128 + 32 KB at 16000):
//
//   load      buf[n] = window[n] frame[n], one frame per transform       (global: hop + window_size samples are new)
//   FFT       mixed-radix Stockham passes from the host's plan (cfp_fft.h): every thread reads the inputs of its
//             butterflies into registers, barrier, writes the outputs -- one buffer, no ping-pong
//   s0        |Z[k]| / ||h|| of bins 0 .. N / 2, frame t's parked beside the buffer while frame t + 1 is transformed, then
//             both as (real, imaginary) of the buffer, mirrored to bins N - k
//   tfrL0     filterbank rows over s0[:f_cols] from LDS, one thread per (row, frame)
//   layer 0   spec = s0 ** g[0]
//   layer i   FFT of the packed pair: both sequences are real and even, so the real part of the transform is frame t's
//             result and the imaginary part frame t + 1's; rectifier in place; the filterbank of the LAST layer of each
//             parity (tfrLF: even, tfrLQ: odd) is taken right after it, into a register of the (row, frame) thread;
//             before the next transform the even part is taken, (x[k] + x[N - k]) / 2 (cfp_fft.h: even_part)
//   store     Z = tfrLF tfrLQ and, when asked for, tfrL0 / tfrLF / tfrLQ: 4 x n_out floats per frame leave the CU
//
// Twiddles: one table of N fp32 values rounded from float64 (mispec_cfp_twiddles_host), read through the caches.
// Bounds: every LDS index is < N by construction of the plan (cfp_fft.h), the signal is read only inside [0, n_samples),
// the filterbank supports are clamped to [0, cols] with cols <= N, outputs are written only for frames < n_frames.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "cfp_fft.h"
#include "mispec.h"
#include "mispec_internal.h"

namespace {

using cfpfft::cf;
constexpr int NT = cfpfft::NT;

struct CfpParams {
  const float *x;
  long long x_clip_stride;
  int n_samples, hop, N, window_size, left, half;
  const float *window;
  const cf *twiddle;
  float window_scale, inv_sqrt_n;
  int first_frame, n_frames, n_layers;
  float g[cfpfft::MAX_LAYERS];
  int cut_ceps, cut_spec;
  const float *fmat, *qmat;
  const int *f_support, *q_support;
  int f_cols, q_cols, n_out;
  float *z, *l0, *lf, *lq;
  long long out_clip_stride, out_row_stride;
  cfpfft::Plan plan;
};

template <int R, int CAP>
__device__ __forceinline__ void fft_pass(cf *buf, int N, int s, const cf *tw, int tid) {
  cf v[cfpfft::per_thread<R, CAP>()][R];
  cfpfft::pass_load<R, CAP>(buf, N, tid, v);
  __syncthreads();
  cfpfft::pass_store<R, CAP>(buf, N, s, tw, tid, v);
  __syncthreads();
}

// the N-point transform of buf, in place; entered and left with the buffer consistent (barrier behind it)
template <int CAP>
__device__ __forceinline__ void fft(cf *buf, const CfpParams &p, int tid) {
  int s = 1;
  for (int i = 0; i < p.plan.n_pass; ++i) {
    const int r = p.plan.radix[i];
    switch (r) {
      case 2: fft_pass<2, CAP>(buf, p.N, s, p.twiddle, tid); break;
      case 4: fft_pass<4, CAP>(buf, p.N, s, p.twiddle, tid); break;
      case 5: fft_pass<5, CAP>(buf, p.N, s, p.twiddle, tid); break;
      case 8: fft_pass<8, CAP>(buf, p.N, s, p.twiddle, tid); break;
      case 10: fft_pass<10, CAP>(buf, p.N, s, p.twiddle, tid); break;
      default:
        if constexpr (CAP > cfpfft::HALF_CAP) fft_pass<16, CAP>(buf, p.N, s, p.twiddle, tid);  // (make_plan: none below)
        break;
    }
    s *= r;
  }
}

// one filterbank row over the frame `j` (0: real parts, 1: imaginary parts) of buf[:cols]
__device__ __forceinline__ float band(const cf *buf, const float *mat, const int *support, int cols, int row, int j) {
  int a = support[2 * row], b = support[2 * row + 1];
  a = a < 0 ? 0 : a;
  b = b > cols ? cols : b;
  const float *m = mat + (long long)row * cols;
  float acc = 0.f;
  for (int k = a; k < b; ++k) acc += m[k] * (j ? buf[k].y : buf[k].x);
  return acc;
}

// CAP = HALF_CAP: N <= HALF_N = 8000, 80 KB of LDS at most and under 128 VGPRs -- two workgroups per CU, one transforming while the
// other waits at a barrier; CAP = MAX_N: one workgroup per CU
template <int CAP, int WAVES_PER_SIMD>
__global__ __launch_bounds__(NT, WAVES_PER_SIMD) void cfp_kernel(const CfpParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  cf *buf = reinterpret_cast<cf *>(smem);
  const int tid = threadIdx.x;
  const int N = p.N;
  const int clip = blockIdx.y;
  const int t0 = p.first_frame + 2 * (int)blockIdx.x;          // the pair's first frame
  const bool second = t0 + 1 < p.first_frame + p.n_frames;     // an odd count: the last pair's partner is zeros
  const float *x = p.x + (long long)clip * p.x_clip_stride;

  const int row = tid >> 1, j = tid & 1;
  const bool owner = row < p.n_out && (j == 0 || second);  // this thread's (row, frame) is stored
  const long long o = (long long)clip * p.out_clip_stride + (long long)row * p.out_row_stride + (t0 + j - p.first_frame);
  float *side = reinterpret_cast<float *>(buf + N);
  float lf = 0.f, lq = 0.f;
  // Stages 0 and 1: s0 of frames t0 and t0 + 1, one transform each (imaginary part zero): the window centred in the frame of
  // the zero-padded signal, FFT, magnitudes of bins 0 .. N / 2.  Frame t0's wait in `side` while frame t0 + 1 is
  // transformed; then both go into the buffer as (real, imaginary), mirrored to the upper half.
  // (Both frames in ONE transform, separated through Z[k] and conj Z[N - k], was measured and dropped: the separation
  // leaves eps |louder frame| in the quieter one, which ** 0.24 turns into 1e-2 of its output -- DESIGN.md 3.16.)
  // Stage s >= 2: layer i = s - 1 on the packed pair.  One loop, so that the transform is compiled once.
#pragma unroll 1
  for (int st = 0; st <= p.n_layers; ++st) {
    if (st < 2) {
      const bool live = st == 0 || second;  // (uniform; zeros for the missing partner of an odd count)
      for (int n = tid; n < N; n += NT) {
        float v = 0.f;
        const int wi = n - p.left;
        const long long i = (long long)(t0 + st) * p.hop + n - p.half;
        if (live && wi >= 0 && wi < p.window_size && i >= 0 && i < p.n_samples) v = p.window[wi] * x[i];
        buf[n] = cf{v, 0.f};
      }
    }
    __syncthreads();  // (the frame is loaded / the filterbank reads and the even part of the layer before are done)
    fft<CAP>(buf, p, tid);
    if (st == 0) {
      for (int k = tid; k <= N / 2; k += NT) side[k] = cfpfft::magnitude(buf[k], p.window_scale);
    } else if (st == 1) {
      // (a thread reads bin k <= N / 2 and writes bins k and N - k >= N / 2: nobody else's input)
      for (int k = tid; k <= N / 2; k += NT) {
        const cf m = cf{side[k], cfpfft::magnitude(buf[k], p.window_scale)};
        buf[k] = m;
        buf[k == 0 ? 0 : N - k] = m;
      }
      __syncthreads();
      if (owner && p.l0) p.l0[o] = band(buf, p.fmat, p.f_support, p.f_cols, row, j);
      __syncthreads();
      const float g0 = p.g[0];  // layer 0: spec = s0 ** g[0] (s0 >= 0: its relu is the identity), mirrored
      for (int k = tid; k <= N / 2; k += NT) {
        const cf m = buf[k];
        const cf v = cf{cfpfft::power_law(m.x, g0), cfpfft::power_law(m.y, g0)};
        buf[k] = v;
        buf[k == 0 ? 0 : N - k] = v;
      }
      if (p.n_layers < 3) {  // no later even layer: tfrLF is this one's
        __syncthreads();
        if (row < p.n_out) lf = band(buf, p.fmat, p.f_support, p.f_cols, row, j);
      }
    } else {
      const int i = st - 1;
      const bool odd = i & 1;
      const int c = odd ? p.cut_ceps : p.cut_spec;
      const float g = p.g[i];
      for (int k = tid; k < N; k += NT) {
        const cf v = buf[k] * p.inv_sqrt_n;
        const bool z = cfpfft::cut(k, N, c);
        buf[k] = cf{cfpfft::rectify(v.x, g, z), cfpfft::rectify(v.y, g, z)};
      }
      __syncthreads();
      if (i + 2 >= p.n_layers && row < p.n_out) {  // the last layer of this parity
        if (odd)
          lq = band(buf, p.qmat, p.q_support, p.q_cols, row, j);
        else
          lf = band(buf, p.fmat, p.f_support, p.f_cols, row, j);
      }
      if (i + 1 < p.n_layers) {  // another transform follows: its input is the even part (cfp_fft.h)
        __syncthreads();
        for (int k = tid + 1; 2 * k < N; k += NT) {
          const cf m = cfpfft::even_part(buf[k], buf[N - k]);
          buf[k] = m;
          buf[N - k] = m;
        }
      }
    }
  }
  if (owner) {
    p.z[o] = lf * lq;
    if (p.lf) p.lf[o] = lf;
    if (p.lq) p.lq[o] = lq;
  }
}

}  // namespace

extern "C" {

int mispec_cfp_served(int32_t n_fft, int32_t window_size, int32_t n_out, int32_t n_layers, int32_t log_layer) {
  return cfpfft::served(n_fft, window_size, n_out, n_layers, log_layer != 0) ? 1 : 0;
}

int mispec_cfp_twiddles_host(int32_t n_fft, float *dst) {
  cfpfft::Plan pl;
  if (dst == nullptr) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_twiddles_host: NULL pointer");
  if (n_fft < cfpfft::MIN_N || n_fft > cfpfft::MAX_N || !cfpfft::make_plan(n_fft, pl))
    return mispec_fail_msg(MISPEC_E_UNSUPPORTED, "mispec_cfp_twiddles_host: n_fft must be 2^a 5^b, 16 .. 16000");
  cfpfft::make_twiddles(n_fft, dst);
  return MISPEC_OK;
}

int mispec_cfp_f32(const mispec_cfp_args *a, void *stream) {
  if (a == nullptr) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: NULL argument block");
  if (a->struct_size != sizeof(mispec_cfp_args))
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: struct_size does not match this library's mispec_cfp_args");
  if (!a->x || !a->window || !a->twiddle || !a->fmat || !a->qmat || !a->f_support || !a->q_support || !a->z)
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: NULL device pointer");
  if (a->n_clips <= 0 || a->n_samples <= 0 || a->hop <= 0 || a->n_frames <= 0 || a->first_frame < 0 || a->n_fft <= 0 ||
      a->window_size <= 0 || a->n_out <= 0 || a->f_cols <= 0 || a->q_cols <= 0 || a->x_clip_stride < a->n_samples ||
      a->out_row_stride < a->n_frames || a->out_clip_stride < (int64_t)a->n_out * a->out_row_stride)
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: non-positive size or a stride shorter than its row");
  bool log_layer = false;
  for (int i = 0; i < a->n_layers && i < cfpfft::MAX_LAYERS; ++i) log_layer = log_layer || a->g[i] == 0.f;
  if (!cfpfft::served(a->n_fft, a->window_size, a->n_out, a->n_layers, log_layer))
    return mispec_fail_msg(MISPEC_E_UNSUPPORTED,
                           "mispec_cfp_f32: n_fft must be an even 2^a 5^b in 16 .. 16000, window_size <= n_fft, n_out <= 256, 2 .. 8 "
                           "layers, none of them with g == 0");
  if (a->f_cols > a->n_fft || a->q_cols > a->n_fft)
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: a filterbank has more columns than the frame has bins");
  // every frame asked for starts inside the padded signal, as torch.stft counts them
  const int64_t last_start = ((int64_t)a->first_frame + a->n_frames - 1) * a->hop;
  if (last_start + a->n_fft > (int64_t)a->n_samples + 2 * (a->n_fft / 2))
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_cfp_f32: more frames than the padded signal holds");
  if (a->n_clips > 65535) return mispec_fail_msg(MISPEC_E_UNSUPPORTED, "mispec_cfp_f32: more than 65535 clips in one call");

  CfpParams p;
  p.x = a->x;
  p.x_clip_stride = a->x_clip_stride;
  p.n_samples = a->n_samples;
  p.hop = a->hop;
  p.N = a->n_fft;
  p.window_size = a->window_size;
  p.left = (a->n_fft - a->window_size) / 2;
  p.half = a->n_fft / 2;
  p.window = a->window;
  p.twiddle = reinterpret_cast<const cf *>(a->twiddle);
  p.window_scale = a->window_scale;
  p.inv_sqrt_n = (float)(1.0 / std::sqrt((double)a->n_fft));
  p.first_frame = a->first_frame;
  p.n_frames = a->n_frames;
  p.n_layers = a->n_layers;
  for (int i = 0; i < cfpfft::MAX_LAYERS; ++i) p.g[i] = i < a->n_layers ? a->g[i] : 1.f;
  p.cut_ceps = a->cut_ceps;
  p.cut_spec = a->cut_spec;
  p.fmat = a->fmat;
  p.qmat = a->qmat;
  p.f_support = a->f_support;
  p.q_support = a->q_support;
  p.f_cols = a->f_cols;
  p.q_cols = a->q_cols;
  p.n_out = a->n_out;
  p.z = a->z;
  p.l0 = a->l0;
  p.lf = a->lf;
  p.lq = a->lq;
  p.out_clip_stride = a->out_clip_stride;
  p.out_row_stride = a->out_row_stride;
  cfpfft::make_plan(a->n_fft, p.plan);

  const size_t lds = (size_t)cfpfft::lds_bytes(a->n_fft);
  auto kern = a->n_fft <= cfpfft::HALF_N ? cfp_kernel<cfpfft::HALF_CAP, 4> : cfp_kernel<cfpfft::MAX_N, 2>;
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
        hipSuccess)
      return mispec_fail_msg(MISPEC_E_HIP, "hipFuncSetAttribute failed (cfp kernel)");
  }
  const dim3 grid((unsigned)((a->n_frames + 1) / 2), (unsigned)a->n_clips);
  hipLaunchKernelGGL(kern, grid, dim3(NT), lds, static_cast<hipStream_t>(stream), p);
  if (hipGetLastError() != hipSuccess) return mispec_fail_msg(MISPEC_E_HIP, "mispec_cfp_f32: launch failed");
  return MISPEC_OK;
}

}  // extern "C"
