// softmax_block.hip -- <blocksoftmax>: several softmaxes side by side in one output layer (BlockSoftmax,
// TNetLib Activation.cc:55-133; the reference trains it on the CPU only), fused with the cross-entropy
// objective the way reduce.hip fuses the plain softmax.
//
// One wavefront per row, four rows a workgroup (softmax_xent_kernel's geometry, so the statistics take the same
// slots).  A row of up to 4096 columns is loaded once into 64 registers per lane -- 16 units of 256 columns, a
// lane's four values of a unit being 16 contiguous bytes where base, stride and width allow (V4) and four
// columns 64 apart otherwise.  The register layout follows the ROW, not the blocks, so block offsets need no
// alignment: the wave then walks the blocks, and for each one takes the maximum, the exponentials and the sum
// over the units the block touches (a wave-uniform skip of the others, by 1024 and by 256 columns), every lane
// masking its columns to [lo, hi).  One last sweep over the row writes Y and the masked error and takes the
// whole-row argmax, in column order.  Wider rows re-read the row block by block (softmax_xent_kernel's
// fallback).
//
// Every sum is a lane's fp32 sum in column order, combined by the fp64 butterfly of reduce.hip; with B == 1 the
// arithmetic is softmax_xent_kernel's operation for operation, and for 1025..4096 aligned columns
// softmax_xent_row4's (`quad`: four interleaved partial sums, one per wave of that kernel), so a one-block layer
// gives the plain kernel's bits.  The forward kernel and the fused kernel are one template.
#include <float.h>

#include "kcommon.h"

// y = e * (1/sum) is rounded before the error subtracts the target from it: the error is then the same bits
// whether it is formed here or by a later kernel that reads Y back (the three-call chain)
#pragma clang fp contract(off)

namespace tnetk {

constexpr int BS_UNITS = 16;          // 256-column units held in registers: 4096 columns
constexpr int BS_MAXN = BS_UNITS * 256;

__device__ __forceinline__ int bs_clamp(int v, int N) { return v < 0 ? 0 : (v > N ? N : v); }

// column of register q (0..3) of unit u on this lane
template <bool V4>
__device__ __forceinline__ int bs_col(int u, int q, int lane) {
  return V4 ? u * 256 + lane * 4 + q : u * 256 + q * 64 + lane;
}

// f(u, q, col) for every register of this lane whose column lies in [lo, hi); u and q are compile-time after
// unrolling, so the caller's register array stays in registers
template <bool V4, typename F>
__device__ __forceinline__ void bs_for_range(int lo, int hi, int lane, F&& f) {
#pragma unroll
  for (int g = 0; g < BS_UNITS / 4; ++g) {
    if (g * 1024 < hi && (g + 1) * 1024 > lo) {
#pragma unroll
      for (int uu = 0; uu < 4; ++uu) {
        const int u = g * 4 + uu;
        if (u * 256 < hi && (u + 1) * 256 > lo) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = bs_col<V4>(u, q, lane);
            if (c >= lo && c < hi) f(u, q, c);
          }
        }
      }
    }
  }
}

// the row's statistics: four rows a workgroup into slot (workgroup % slots), as softmax_xent_kernel; `quad`:
// every row on its own into slot (row % slots), as softmax_xent_row4.  Every wave of the workgroup calls it.
__device__ __forceinline__ void bs_stats(double* __restrict__ stats, bool quad, int row, bool live, double xent,
                                         bool hit) {
  __shared__ double red[2][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (quad) {
    if (live && lane == 0 && stats) {
      const int slot = row % TNET_STATS_SLOTS;
      atomicAdd(stats + 2 * slot, xent);
      atomicAdd(stats + 2 * slot + 1, hit ? 1.0 : 0.0);
    }
    return;
  }
  if (lane == 0) {
    red[0][wv] = live ? xent : 0.0;
    red[1][wv] = live && hit ? 1.0 : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0 && stats) {
    const int slot = blockIdx.x % TNET_STATS_SLOTS;
    atomicAdd(stats + 2 * slot, red[0][0] + red[0][1] + red[0][2] + red[0][3]);
    atomicAdd(stats + 2 * slot + 1, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

// XENT: labels, masked error and statistics; otherwise the forward pass alone (labels, E, stats unused)
template <bool V4, bool XENT>
__global__ __launch_bounds__(256) void block_softmax_kernel(const float* __restrict__ Z, TnetMatrixDim d,
                                                            const int* __restrict__ offsets, int B,
                                                            const int* __restrict__ labels, float* __restrict__ Y,
                                                            int strideY, float* __restrict__ E, int strideE,
                                                            double* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int N = d.cols;
  const bool quad = V4 && B == 1 && N > 1024;
  if (row >= d.rows) {
    if (XENT) bs_stats(stats, quad, row, false, 0.0, false);
    return;
  }
  const float* src = Z + (long)row * d.stride;
  int t = -1;
  if (XENT) {
    t = labels[row];
    if (t >= N) t = -1;
  }
  // ---- the row, once
  float rv[BS_UNITS * 4];
#pragma unroll
  for (int u = 0; u < BS_UNITS; ++u) {
    if (V4) {
      const int c = u * 256 + lane * 4;
      f32x4 x = {-1e30f, -1e30f, -1e30f, -1e30f};
      if (c < N) x = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
      for (int q = 0; q < 4; ++q) rv[u * 4 + q] = x[q];
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = u * 256 + q * 64 + lane;
        rv[u * 4 + q] = (u * 256 < N && c < N) ? src[c] : -1e30f;
      }
    }
  }
  // ---- block by block: maximum, exponentials, sum, normalisation -- all in the registers
  int tlo = 0, thi = 0;  // the label's block (empty: unlabeled row)
  for (int b = 0; b < B; ++b) {
    const int lo = bs_clamp(offsets[b], N), hi = bs_clamp(offsets[b + 1], N);
    if (hi <= lo) continue;
    if (t >= lo && t < hi) { tlo = lo; thi = hi; }
    float m = -1e20f;
    bs_for_range<V4>(lo, hi, lane, [&](int u, int q, int) { m = fmaxf(m, rv[u * 4 + q]); });
    m = wave_max(m);
    float s = 0.f, s4[4] = {0.f, 0.f, 0.f, 0.f};
    bs_for_range<V4>(lo, hi, lane, [&](int u, int q, int) {
      const float e = fast_exp(rv[u * 4 + q] - m);
      rv[u * 4 + q] = e;
      s += e;
      if (V4) s4[u & 3] += e;
    });
    double dsum;
    if (quad) {
      const double d0 = wave_sum_d((double)s4[0]), d1 = wave_sum_d((double)s4[1]);
      const double d2 = wave_sum_d((double)s4[2]), d3 = wave_sum_d((double)s4[3]);
      dsum = d0 + d1 + d2 + d3;
    } else {
      dsum = wave_sum_d((double)s);
    }
    const float rsum = 1.f / (float)dsum;  // one division per block; y = e * (1/sum)
    bs_for_range<V4>(lo, hi, lane, [&](int u, int q, int) { rv[u * 4 + q] *= rsum; });
  }
  // ---- the row again in column order: Y, the masked error, the whole-row argmax
  float* yrow = Y ? Y + (long)row * strideY : nullptr;
  float* erow = (XENT && E) ? E + (long)row * strideE : nullptr;
  ArgMax ay{-1e20f, 0x7fffffff};
  float ytl = 0.f;  // the y of column t, on the lane that owns it
#pragma unroll
  for (int u = 0; u < BS_UNITS; ++u) {
    if (u * 256 < N) {
      f32x4 yv, ev;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = bs_col<V4>(u, q, lane);
        const float y = rv[u * 4 + q];
        yv[q] = y;
        ev[q] = 0.f;
        if (c < N) {
          if (XENT) {
            if (y > ay.v) { ay.v = y; ay.i = c; }
            if (c == t) ytl = y;
            if (c >= tlo && c < thi) ev[q] = y - ((c == t) ? 1.f : 0.f);
          }
          if (!V4) {
            if (yrow) yrow[c] = y;
            if (erow) erow[c] = ev[q];
          }
        }
      }
      if (V4 && u * 256 + lane * 4 < N) {
        const int c = u * 256 + lane * 4;
        if (yrow) *reinterpret_cast<f32x4*>(yrow + c) = yv;
        if (erow) *reinterpret_cast<f32x4*>(erow + c) = ev;
      }
    }
  }
  if (XENT) {
    ay = wave_argmax(ay);
    const int des = t >= 0 ? t : 0;  // all-zero target row: first max of zeros is column 0
    const float yt = __shfl(ytl, t < 0 ? 0 : V4 ? (t & 255) >> 2 : t & 63, 64);
    double xent = 0.0;
    if (t >= 0) xent = -(double)logf(clamp_flt_min(yt));
    bs_stats(stats, quad, row, true, xent, ay.i == des);
  }
}

// rows wider than the register cache: every block read three times (maximum, sum, output)
template <bool XENT>
__global__ __launch_bounds__(256) void block_softmax_wide_kernel(const float* __restrict__ Z, TnetMatrixDim d,
                                                                 const int* __restrict__ offsets, int B,
                                                                 const int* __restrict__ labels,
                                                                 float* __restrict__ Y, int strideY,
                                                                 float* __restrict__ E, int strideE,
                                                                 double* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int N = d.cols;
  if (row >= d.rows) {
    if (XENT) bs_stats(stats, false, row, false, 0.0, false);
    return;
  }
  const float* src = Z + (long)row * d.stride;
  float* yrow = Y ? Y + (long)row * strideY : nullptr;
  float* erow = (XENT && E) ? E + (long)row * strideE : nullptr;
  int t = -1;
  if (XENT) {
    t = labels[row];
    if (t >= N) t = -1;
  }
  ArgMax ay{-1e20f, 0x7fffffff};
  float ytl = 0.f;
  int tlane = 0;
  for (int b = 0; b < B; ++b) {
    const int lo = bs_clamp(offsets[b], N), hi = bs_clamp(offsets[b + 1], N);
    if (hi <= lo) continue;
    const bool mine = t >= lo && t < hi;
    if (mine) tlane = (t - lo) & 63;
    float m = -1e20f;
    for (int c = lo + lane; c < hi; c += 64) m = fmaxf(m, src[c]);
    m = wave_max(m);
    float s = 0.f;
    for (int c = lo + lane; c < hi; c += 64) s += fast_exp(src[c] - m);
    const float rsum = 1.f / (float)wave_sum_d((double)s);
    for (int c = lo + lane; c < hi; c += 64) {
      const float y = fast_exp(src[c] - m) * rsum;
      if (yrow) yrow[c] = y;
      if (XENT) {
        if (y > ay.v) { ay.v = y; ay.i = c; }
        if (c == t) ytl = y;
        if (erow) erow[c] = mine ? y - ((c == t) ? 1.f : 0.f) : 0.f;
      }
    }
  }
  if (XENT) {
    ay = wave_argmax(ay);
    const int des = t >= 0 ? t : 0;
    const float yt = __shfl(ytl, tlane, 64);
    double xent = 0.0;
    if (t >= 0) xent = -(double)logf(clamp_flt_min(yt));
    bs_stats(stats, false, row, true, xent, ay.i == des);
  }
}

// the sum rule of BlockSoftmax::BackpropagateFnc; Ein and Eout may be one matrix (a lane writes only the
// columns it has read, after its block's sum is known)
template <bool V4>
__global__ __launch_bounds__(256) void block_softmax_bwd_kernel(const float* Ein, TnetMatrixDim d,
                                                                const int* __restrict__ offsets, int B, float* Eout,
                                                                int strideEout, int* __restrict__ invalid) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int N = d.cols;
  if (row >= d.rows) return;
  const float* src = Ein + (long)row * d.stride;
  float* dst = Eout + (long)row * strideEout;
  int bad = 0;
  if (N <= BS_MAXN) {
    float rv[BS_UNITS * 4];
#pragma unroll
    for (int u = 0; u < BS_UNITS; ++u) {
      if (V4) {
        const int c = u * 256 + lane * 4;
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (c < N) x = *reinterpret_cast<const f32x4*>(src + c);
#pragma unroll
        for (int q = 0; q < 4; ++q) rv[u * 4 + q] = x[q];
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = u * 256 + q * 64 + lane;
          rv[u * 4 + q] = (u * 256 < N && c < N) ? src[c] : 0.f;
        }
      }
    }
    for (int b = 0; b < B; ++b) {
      const int lo = bs_clamp(offsets[b], N), hi = bs_clamp(offsets[b + 1], N);
      if (hi <= lo) continue;
      float s = 0.f;
      bs_for_range<V4>(lo, hi, lane, [&](int u, int q, int) { s += rv[u * 4 + q]; });
      const float sum = (float)wave_sum_d((double)s);
      const bool keep = sum > -0.1f && sum < 0.1f;
      if (!keep) {
        if (!(sum > 0.9f && sum < 1.1f)) bad++;
        bs_for_range<V4>(lo, hi, lane, [&](int u, int q, int) { rv[u * 4 + q] = 0.f; });
      }
    }
#pragma unroll
    for (int u = 0; u < BS_UNITS; ++u) {
      if (u * 256 < N) {
        if (V4) {
          const int c = u * 256 + lane * 4;
          const f32x4 v = {rv[u * 4], rv[u * 4 + 1], rv[u * 4 + 2], rv[u * 4 + 3]};
          if (c < N) *reinterpret_cast<f32x4*>(dst + c) = v;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = u * 256 + q * 64 + lane;
            if (c < N) dst[c] = rv[u * 4 + q];
          }
        }
      }
    }
  } else {
    for (int b = 0; b < B; ++b) {
      const int lo = bs_clamp(offsets[b], N), hi = bs_clamp(offsets[b + 1], N);
      if (hi <= lo) continue;
      float s = 0.f;
      for (int c = lo + lane; c < hi; c += 64) s += src[c];
      const float sum = (float)wave_sum_d((double)s);
      const bool keep = sum > -0.1f && sum < 0.1f;
      if (!keep && !(sum > 0.9f && sum < 1.1f)) bad++;
      for (int c = lo + lane; c < hi; c += 64) dst[c] = keep ? src[c] : 0.f;
    }
  }
  if (invalid && bad && lane == 0) atomicAdd(invalid, bad);
}

static bool bs_v4ok(const void* p, int stride) { return ((uintptr_t)p & 15) == 0 && (stride & 3) == 0; }

template <bool XENT>
static int block_softmax_run(const float* Z, TnetMatrixDim dZ, const int* offsets, int B, const int* labels, float* Y,
                             int strideY, float* E, int strideE, double* stats, hipStream_t st) {
  if (dZ.rows < 0 || dZ.cols <= 0 || dZ.stride < dZ.cols || !Z || !offsets || B < 1 || B > dZ.cols) return TNET_ERR_ARG;
  if (Y && strideY < dZ.cols) return TNET_ERR_ARG;
  if (E && strideE < dZ.cols) return TNET_ERR_ARG;
  if (XENT && !labels) return TNET_ERR_ARG;
  if (!dZ.rows) return TNET_OK;
  const bool v4 = (dZ.cols & 3) == 0 && bs_v4ok(Z, dZ.stride) && (!Y || bs_v4ok(Y, strideY)) &&
                  (!E || bs_v4ok(E, strideE));
  const int grid = cdiv((long)dZ.rows * 64, 256);
  if (dZ.cols > BS_MAXN)
    block_softmax_wide_kernel<XENT><<<grid, 256, 0, st>>>(Z, dZ, offsets, B, labels, Y, strideY, E, strideE, stats);
  else if (v4)
    block_softmax_kernel<true, XENT><<<grid, 256, 0, st>>>(Z, dZ, offsets, B, labels, Y, strideY, E, strideE, stats);
  else
    block_softmax_kernel<false, XENT><<<grid, 256, 0, st>>>(Z, dZ, offsets, B, labels, Y, strideY, E, strideE, stats);
  TNET_LAUNCH_CHECK();
  return TNET_OK;
}

}  // namespace tnetk

using namespace tnetk;

extern "C" int tnetF_block_softmax(float* y, const float* x, TnetMatrixDim d, const int* offsets, int B,
                                   void* stream) {
  if (!y) return TNET_ERR_ARG;
  return block_softmax_run<false>(x, d, offsets, B, nullptr, y, d.stride, nullptr, 0, nullptr, (hipStream_t)stream);
}

extern "C" int tnet_block_softmax_xent(const float* Z, TnetMatrixDim dZ, const int* offsets, int B, const int* labels,
                                       float* Y, int strideY, float* E, int strideE, double* stats, void* stream) {
  return block_softmax_run<true>(Z, dZ, offsets, B, labels, Y, strideY, E, strideE, stats, (hipStream_t)stream);
}

extern "C" int tnet_block_softmax_bwd(const float* Ein, TnetMatrixDim dE, const int* offsets, int B, float* Eout,
                                      int strideEout, int* invalid, void* stream) {
  if (dE.rows < 0 || dE.cols <= 0 || dE.stride < dE.cols || !Ein || !Eout || strideEout < dE.cols || !offsets ||
      B < 1 || B > dE.cols)
    return TNET_ERR_ARG;
  if (!dE.rows) return TNET_OK;
  const bool v4 = (dE.cols & 3) == 0 && bs_v4ok(Ein, dE.stride) && bs_v4ok(Eout, strideEout);
  const int grid = cdiv((long)dE.rows * 64, 256);
  if (v4)
    block_softmax_bwd_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(Ein, dE, offsets, B, Eout, strideEout,
                                                                          invalid);
  else
    block_softmax_bwd_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(Ein, dE, offsets, B, Eout, strideEout,
                                                                           invalid);
  TNET_LAUNCH_CHECK();
  return TNET_OK;
}
