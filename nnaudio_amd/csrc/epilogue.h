// epilogue.h -- the pointwise epilogue of one (bin, frame) pair: (re, im) -> the output format of `epilogue`.  ONE
// definition for the contraction kernels (mispec.hip), the chain kernel (cqt_chain.hip) and the host loops: CQT1992v2's
// "same bits as torch conv1d" rests on it.  P is any parameter block with the fields epilogue, eps and power.
// (stft_fft.inl's fft_epilogue takes its kind at compile time and octave_stream.hip's computes Power without an exponent:
// different functions on purpose.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mispec.h"

template <typename P>
__host__ __device__ __forceinline__ void epilogue_store(const P &p, float *__restrict__ dst, float re, float im) {
  switch (p.epilogue) {
    case MISPEC_EPI_COMPLEX: {
      float2 v = make_float2(re, im);
      *reinterpret_cast<float2 *>(dst) = v;
    } break;
    case MISPEC_EPI_MAGNITUDE:
      dst[0] = sqrtf(re * re + im * im + p.eps);
      break;
    case MISPEC_EPI_POWER: {
      float s = re * re + im * im + p.eps;
      float r;
      if (p.power == 2.0f && p.eps == 0.f)
        r = s;
      else if (p.power == 1.0f)
        r = sqrtf(s);
      else
        r = powf(sqrtf(s), p.power);
      dst[0] = r;
    } break;
    case MISPEC_EPI_PHASE_ATAN2:
      dst[0] = atan2f(im + 0.0f, re);
      break;
    case MISPEC_EPI_PHASE_COSSIN: {
      float a = atan2f(im, re);
      float2 v = make_float2(cosf(a), sinf(a));
      *reinterpret_cast<float2 *>(dst) = v;
    } break;
    default:
      dst[0] = re;
      break;
  }
}

// floats per (bin, frame) of the output
__host__ __device__ __forceinline__ int epilogue_width(int epi) {
  return (epi == MISPEC_EPI_COMPLEX || epi == MISPEC_EPI_PHASE_COSSIN) ? 2 : 1;
}
