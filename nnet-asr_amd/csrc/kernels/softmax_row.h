// softmax_row.h -- the row normaliser of the one-wave-per-row softmax, shared by softmax_xent_kernel (reduce.hip:
// tnetF_softmax, tnet_softmax_xent, tnet_softmax_xent_dense) and softmax_emit_kernel (feacat_emit.hip), so that a
// posterior formed inside the forward pass's emit is the one tnetF_softmax would have written, bit for bit.
#pragma once

#include "kcommon.h"

namespace tnetk {

constexpr int SX_MAXV4 = 16;  // row held in registers up to 16 float4 per lane = 4096 columns

// Passes 1 and 2 over one row of N columns at src, by one wave (every lane calls it):
//   m    = the row maximum (from -1e20f up, fmaxf: a NaN never becomes the maximum)
//   rsum = 1 / (float) sum_c exp(x_c - m)  (fp32 per lane, the 64 lane sums added in fp64) -- when `logits`
// cached (16-B aligned row, N % 4 == 0, N <= 4096): lane l holds columns j * 256 + 4 l .. + 3 in rv[j], which
// leave holding exp(x - m) where `logits`, x otherwise.  Not cached: the row is re-read, lane l taking columns
// l, l + 64, ...; the caller forms y = fast_exp(x - m) * rsum.
__device__ __forceinline__ void softmax_row_norm(const float* __restrict__ src, const int N, const int lane,
                                                 const bool cached, const bool logits, f32x4 (&rv)[SX_MAXV4],
                                                 float& m_out, float& rsum_out) {
  // ---- pass 1: max
  float m = -1e20f;
  if (cached) {
#pragma unroll
    for (int j = 0; j < SX_MAXV4; ++j) {
      const int c = j * 256 + lane * 4;
      f32x4 x = {-1e30f, -1e30f, -1e30f, -1e30f};
      if (c < N) x = *reinterpret_cast<const f32x4*>(src + c);
      rv[j] = x;
      m = fmaxf(m, fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
    }
  } else {
    for (int c = lane; c < N; c += 64) m = fmaxf(m, src[c]);
  }
  m = wave_max(m);

  // ---- pass 2: sum of exp (only when normalising logits)
  double dsum = 0.0;
  if (logits) {
    float s = 0.f;
    if (cached) {
#pragma unroll
      for (int j = 0; j < SX_MAXV4; ++j) {
        const int c = j * 256 + lane * 4;
        if (c < N) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float e = fast_exp(rv[j][k] - m);
            rv[j][k] = e;
            s += e;
          }
        }
      }
    } else {
      for (int c = lane; c < N; c += 64) s += fast_exp(src[c] - m);
    }
    dsum = wave_sum_d((double)s);
  }
  const float sum = (float)dsum;
  m_out = m;
  rsum_out = 1.f / sum;  // one division per row; y = e * (1/sum)
}

}  // namespace tnetk
