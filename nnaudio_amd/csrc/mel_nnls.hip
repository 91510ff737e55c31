// mel_nnls.hip -- mel spectrogram -> magnitude (or power) spectrogram in ONE launch: mispec_mel_nnls_f32 of
// include/mispec.h, behind MelSpectrogram.to_stft / inverse.
//
// Per frame column the non-negative least squares problem min_{p >= 0} || M p - m ||^2 is solved by n_iter projected
// gradient steps with Nesterov momentum.  As torch operators every step is two dense (n_mels, F) GEMMs and five passes
// over a (B, F, T) tensor in HBM.  The frame columns are independent and the bank is ~8 KB when stored sparse, so here a
// workgroup takes TF consecutive frames of one clip, keeps the whole operator (mel_nnls.h: the table blob) and the tile
// in LDS, p and y in registers -- the iterate in float64, mel_nnls.h says why --, and runs ALL steps: HBM sees the mel input once and the spectrum once.
//
//   setup     tables -> LDS; mel tile (n_act, TF) -> LDS (frames beyond the clip: 0); y tile (F, TF) = 0
//   n_iter x  row walk:  r[c, t] = sum_k w[c, k] y[start_c + k, t] - m[c, t]      32 lanes per active row, the sum in float64
//                        (as everything between the mel tile and the store), residual tile
//             barrier
//             update:    g = sum_j tw[b, j] r[first_b + j, t];  p+ = max(y - eta g, 0);  y = p+ + beta_k (p+ - p)
//                        in registers, y written back to the tile
//             barrier
//   store     p ** (1 / power) of frames < T
//
// beta_k is the same for every lane: it is read from the table in global memory through the scalar cache, one load per
// step -- no LDS, no cap on n_iter.
// Bounds: the mel input is read only at frames < T and rows < n_mels (the tables' row indices), the output written only
// at frames < T and bins < F; every LDS index is inside its tile by construction of the tables (mel_nnls.h: start + len
// <= F, first + cnt <= n_act).  A bin no row covers has cnt = 0: g = 0 and p stays exactly 0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mel_nnls.h"
#include "mispec.h"
#include "mispec_internal.h"

namespace {

using namespace melnnls;

struct MelNnlsParams {
  const float *mel;
  long long mel_clip_stride, mel_row_stride;
  const int32_t *tables;
  int table_words, n_act, nnz, F, T, n_iter;
  const float *beta;
  double eta;
  float power;
  float *out;
  long long out_clip_stride, out_row_stride;
};

template <int TF, int NE>
__global__ __launch_bounds__(NT) void mel_nnls_kernel(const MelNnlsParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int BP = NT / TF;  // bins per pass of the update
  int32_t *blob = reinterpret_cast<int32_t *>(smem);
  double *ytile = reinterpret_cast<double *>(blob + table_words_lds(p.table_words));
  double *rtile = ytile + p.F * TF;
  float *mtile = reinterpret_cast<float *>(rtile + p.n_act * TF);
  const int tid = threadIdx.x;
  const int F = p.F, n_act = p.n_act;
  const int t0 = (int)blockIdx.x * TF;
  const float *mel = p.mel + (long long)blockIdx.y * p.mel_clip_stride;

  for (int i = tid; i < p.table_words; i += NT) blob[i] = p.tables[i];
  for (int i = tid; i < F * TF; i += NT) ytile[i] = 0.0;
  __syncthreads();
  const View v = view(blob, n_act, F, p.nnz);
  for (int i = tid; i < n_act * TF; i += NT) {
    const int c = i / TF, t = i % TF;
    mtile[i] = t0 + t < p.T ? mel[(long long)v.rows[ROW_WORDS * c + 3] * p.mel_row_stride + t0 + t] : 0.f;
  }
  __syncthreads();

  const int t = tid % TF, b0 = tid / TF;
  const int lane = tid % ROW_LANES, hw = tid / ROW_LANES;
  double pv[NE], yv[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) pv[i] = yv[i] = 0.0;

#pragma unroll 1
  for (int k = 0; k < p.n_iter; ++k) {
    for (int c = hw; c < n_act; c += NT / ROW_LANES) {
      double a = row_partial<TF>(v, ytile, c, lane);
      a = reduce_phases<TF>(a, [](double x, int m) { return __shfl_xor(x, m); });
      if (lane < TF) rtile[c * TF + lane] = a - (double)mtile[c * TF + lane];
    }
    __syncthreads();
    const double beta = (double)p.beta[k];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int b = b0 + i * BP;
      if (b < F) {
        update(pv[i], yv[i], gradient<TF>(v, rtile, b, t), p.eta, beta);
        ytile[b * TF + t] = yv[i];
      }
    }
    __syncthreads();
  }

  if (t0 + t < p.T) {
    float *out = p.out + (long long)blockIdx.y * p.out_clip_stride + t0 + t;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
      const int b = b0 + i * BP;
      if (b < F) out[(long long)b * p.out_row_stride] = finish(pv[i], p.power);
    }
  }
}

using Kernel = void (*)(const MelNnlsParams);

// register slots for the bins a thread owns: 9 or 17 (mel_nnls.h: elements_per_thread)
Kernel pick(int TF, int ne) {
  if (TF == 16) return ne <= 9 ? mel_nnls_kernel<16, 9> : mel_nnls_kernel<16, MAX_NE>;
  if (TF == 8) return ne <= 9 ? mel_nnls_kernel<8, 9> : mel_nnls_kernel<8, MAX_NE>;
  return ne <= 9 ? mel_nnls_kernel<4, 9> : mel_nnls_kernel<4, MAX_NE>;
}

}  // namespace

extern "C" {

int mispec_mel_nnls_served(const float *basis_host, int64_t row_stride, int32_t n_mels, int32_t n_bins, float power) {
  if (basis_host == nullptr) return 0;
  return served(basis_host, (long)row_stride, n_mels, n_bins, power) ? 1 : 0;
}

int mispec_mel_nnls_tables_host(const float *basis_host, int64_t row_stride, int32_t n_mels, int32_t n_bins, int32_t *dst,
                                int64_t dst_words, int32_t *sizes) {
  if (basis_host == nullptr || sizes == nullptr) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_tables_host: NULL pointer");
  if (n_mels <= 0 || n_bins <= 0 || row_stride < n_bins)
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_tables_host: non-positive size or a stride shorter than its row");
  Sizes sz;
  if (!build_tables(basis_host, (long)row_stride, n_mels, n_bins, sz, nullptr))
    return mispec_fail_msg(MISPEC_E_UNSUPPORTED,
                           "mispec_mel_nnls_tables_host: the bank needs contiguous rows with non-decreasing starts and stops, at "
                           "most 4 rows over a bin, n_mels <= 256 and n_bins <= 2049");
  sizes[0] = (int32_t)table_words(sz.n_act, n_bins, sz.nnz);
  sizes[1] = sz.n_act;
  sizes[2] = sz.nnz;
  if (dst == nullptr) return MISPEC_OK;
  if (dst_words < sizes[0]) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_tables_host: dst is shorter than the tables");
  build_tables(basis_host, (long)row_stride, n_mels, n_bins, sz, dst);
  return MISPEC_OK;
}

int mispec_mel_nnls_f32(const mispec_mel_nnls_args *a, void *stream) {
  if (a == nullptr) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: NULL argument block");
  if (a->struct_size != sizeof(mispec_mel_nnls_args))
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: struct_size does not match this library's mispec_mel_nnls_args");
  if (!a->mel || !a->tables || !a->out || (a->n_iter > 0 && !a->beta))
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: NULL device pointer");
  if (a->reserved != 0 || a->reserved2 != 0) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: reserved must be 0");
  if (a->n_clips <= 0 || a->n_frames <= 0 || a->n_mels <= 0 || a->n_bins <= 0 || a->n_iter < 0 ||
      a->mel_row_stride < a->n_frames || a->mel_clip_stride < (int64_t)a->n_mels * a->mel_row_stride ||
      a->out_row_stride < a->n_frames || a->out_clip_stride < (int64_t)a->n_bins * a->out_row_stride)
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: non-positive size or a stride shorter than its row");
  if (!served_shape(a->n_mels, a->n_bins, a->n_act, a->nnz, a->power))
    return mispec_fail_msg(MISPEC_E_UNSUPPORTED,
                           "mispec_mel_nnls_f32: n_mels <= 256, n_bins <= 2049, power > 0 and tables of at most 4 rows over a bin");
  if (a->table_words != table_words(a->n_act, a->n_bins, a->nnz))
    return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: table_words does not match n_act, n_bins and nnz");
  if (!(a->eta >= 0.0)) return mispec_fail_msg(MISPEC_E_INVALID, "mispec_mel_nnls_f32: eta must be >= 0");
  if (a->n_clips > 65535) return mispec_fail_msg(MISPEC_E_UNSUPPORTED, "mispec_mel_nnls_f32: more than 65535 clips in one call");

  MelNnlsParams p;
  p.mel = a->mel;
  p.mel_clip_stride = a->mel_clip_stride;
  p.mel_row_stride = a->mel_row_stride;
  p.tables = a->tables;
  p.table_words = a->table_words;
  p.n_act = a->n_act;
  p.nnz = a->nnz;
  p.F = a->n_bins;
  p.T = a->n_frames;
  p.n_iter = a->n_iter;
  p.beta = a->beta;
  p.eta = a->eta;
  p.power = a->power;
  p.out = a->out;
  p.out_clip_stride = a->out_clip_stride;
  p.out_row_stride = a->out_row_stride;

  const int TF = tile_frames(a->n_bins);
  const int ne = elements_per_thread(a->n_bins, TF);
  const size_t lds = (size_t)lds_bytes(a->n_bins, a->n_act, a->nnz, TF);
  const Kernel kern = pick(TF, ne);
  if (lds > 64 * 1024) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT) !=
        hipSuccess)
      return mispec_fail_msg(MISPEC_E_HIP, "hipFuncSetAttribute failed (mel_nnls kernel)");
  }
  const dim3 grid((unsigned)((a->n_frames + TF - 1) / TF), (unsigned)a->n_clips);
  hipLaunchKernelGGL(kern, grid, dim3(NT), lds, static_cast<hipStream_t>(stream), p);
  if (hipGetLastError() != hipSuccess) return mispec_fail_msg(MISPEC_E_HIP, "mispec_mel_nnls_f32: launch failed");
  return MISPEC_OK;
}

int32_t mispec_mel_nnls_tile_frames(int32_t n_bins) { return tile_frames(n_bins); }

}  // extern "C"
