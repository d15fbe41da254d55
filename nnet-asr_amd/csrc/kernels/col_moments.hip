// col_moments.hip -- per-column first and second moments of a matrix, accumulated over many calls in fp64 on the
// device: the statistics loop of TNormCu (TNormCu.cc:262-282), which the reference runs element by element on one
// host thread after copying every transformed utterance back.
//
//   first[j]  += sum_i (double) X[i,j]
//   second[j] += sum_i (double)(X[i,j] * X[i,j])      the product an fp32 multiply, rounded to fp32 (TNormCu.cc:266
//                                                     squares in BaseFloat), then widened: no fp64 FMA, no double square
//
// Geometry.  One wavefront a workgroup, no LDS: a lane owns one column (scalar form) or four adjacent ones (16-byte
// loads, where the width and the stride are multiples of 4 and the base is 16-byte aligned -- the plain softmax
// kernel's condition), so a workgroup covers a chunk of 64 / 256 columns.  The rows are cut into slabs of
// TNET_COL_MOMENTS_ROWS; workgroup (s, c), s < min(slabs, TNET_COL_MOMENTS_SLOTS), walks the slabs s, s + SLOTS, ...
// of chunk c and adds every row into its lanes' fp64 registers in row order.  A full slab's loads are issued
// together, ahead of its adds.  A 100-row utterance of 598 columns is 7 slabs x 10 chunks = 70 workgroups.
//
// Accumulator.  SLOTS slots of [first[cols], second[cols]] doubles, then one word for the non-finite tag.  Workgroup
// (s, c) adds its registers to slot s with a plain load / add / store: every slot word has exactly one writer in a
// launch, launches on one stream are ordered, and no floating-point atomic exists anywhere -- the same sequence of
// calls (same shapes, same load form) gives the same bits every run.  tnet_col_moments_fetch adds the slots in index
// order.  An accumulator therefore belongs to ONE stream.
//
// Non-finite values.  The reference stops at the first utterance that makes an accumulator NaN / Inf.  With fp32
// inputs and fp64 sums that is exactly: some fp32 square is non-finite (a NaN or Inf input squares to one, and so
// does a finite |x| > ~1.8e19).  A lane that meets one records the launch's tag: the word keeps the SMALLEST tag as
// an integer atomicMax of its complement, so that the zeroed accumulator means "none".
#include <cstring>
#include <mutex>
#include <vector>

#include "kcommon.h"

#pragma clang fp contract(off)

namespace tnetk {

constexpr int CM_ROWS = TNET_COL_MOMENTS_ROWS;
constexpr int CM_SLOTS = TNET_COL_MOMENTS_SLOTS;

template <int W>
__device__ __forceinline__ void cm_add(const float (&x)[W], double (&s1)[W], double (&s2)[W], unsigned& bad) {
#pragma unroll
  for (int q = 0; q < W; ++q) {
    const float sq = x[q] * x[q];
    s1[q] += (double)x[q];
    s2[q] += (double)sq;
    bad |= (__float_as_uint(sq) & 0x7f800000u) == 0x7f800000u;
  }
}

template <bool V4>
__device__ __forceinline__ void cm_load(const float* p, float (&x)[V4 ? 4 : 1]) {
  if constexpr (V4) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = v[q];
  } else {
    x[0] = *p;
  }
}

template <bool V4>
__global__ __launch_bounds__(64) void col_moments_kernel(const float* __restrict__ X, TnetMatrixDim d,
                                                         double* __restrict__ acc, int slabs, unsigned tagkey) {
  constexpr int W = V4 ? 4 : 1;
  const int col = (blockIdx.x * 64 + threadIdx.x) * W;
  if (col >= d.cols) return;  // (V4: cols % 4 == 0, so the lane's four columns are all inside)
  double s1[W], s2[W];
#pragma unroll
  for (int q = 0; q < W; ++q) s1[q] = s2[q] = 0.0;
  unsigned bad = 0;
  for (int sl = blockIdx.y; sl < slabs; sl += gridDim.y) {
    const int r0 = sl * CM_ROWS;
    const float* p = X + (long)r0 * d.stride + col;
    if (r0 + CM_ROWS <= d.rows) {
      float x[CM_ROWS][W];
#pragma unroll
      for (int u = 0; u < CM_ROWS; ++u) cm_load<V4>(p + (long)u * d.stride, x[u]);
#pragma unroll
      for (int u = 0; u < CM_ROWS; ++u) cm_add<W>(x[u], s1, s2, bad);
    } else {
      for (int r = r0; r < d.rows; ++r, p += d.stride) {
        float x[W];
        cm_load<V4>(p, x);
        cm_add<W>(x, s1, s2, bad);
      }
    }
  }
  // slot blockIdx.y (= first slab % SLOTS: the grid has min(slabs, SLOTS) rows); this lane is the only writer of
  // these words in this launch
  double* a = acc + (long)blockIdx.y * 2 * d.cols + col;
#pragma unroll
  for (int q = 0; q < W; ++q) {
    a[q] = a[q] + s1[q];
    a[d.cols + q] = a[d.cols + q] + s2[q];
  }
  if (bad) atomicMax(reinterpret_cast<unsigned*>(acc + (long)CM_SLOTS * 2 * d.cols), tagkey);
}

// out[i] = sum over the slots, in index order, of word i of a slot (i < 2 cols: first, then second); out[2 cols] = the
// tag word
__global__ __launch_bounds__(64) void col_moments_fetch_kernel(const double* __restrict__ acc, int cols,
                                                               double* __restrict__ out) {
  const long n = 2L * cols;
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i < n) {
    double s = 0.0;
    for (int k = 0; k < CM_SLOTS; ++k) s += acc[k * n + i];
    out[i] = s;
  }
  if (i == 0) {
    const unsigned key = *reinterpret_cast<const unsigned*>(acc + CM_SLOTS * n);
    reinterpret_cast<unsigned long long*>(out)[n] = key;
  }
}

}  // namespace tnetk

using namespace tnetk;

extern "C" long tnet_col_moments_words(int cols) { return cols > 0 ? (long)CM_SLOTS * 2 * cols + 1 : 0; }

extern "C" int tnet_col_moments(const float* X, TnetMatrixDim d, double* acc, int tag, void* stream) {
  if (d.rows < 0 || d.cols <= 0 || d.stride < d.cols || tag < 0 || !acc || ((uintptr_t)acc & 7) ||
      ((uintptr_t)X & 3))
    return TNET_ERR_ARG;
  if (!d.rows) return TNET_OK;
  if (!X) return TNET_ERR_ARG;
  const int slabs = cdiv(d.rows, CM_ROWS);
  const int gy = slabs < CM_SLOTS ? slabs : CM_SLOTS;
  const unsigned tagkey = 0xFFFFFFFFu - (unsigned)tag;
  const bool v4 = (d.cols & 3) == 0 && (d.stride & 3) == 0 && ((uintptr_t)X & 15) == 0;
  if (v4)
    col_moments_kernel<true><<<dim3(cdiv(d.cols, 256), gy), 64, 0, (hipStream_t)stream>>>(X, d, acc, slabs, tagkey);
  else
    col_moments_kernel<false><<<dim3(cdiv(d.cols, 64), gy), 64, 0, (hipStream_t)stream>>>(X, d, acc, slabs, tagkey);
  TNET_LAUNCH_CHECK();
  return TNET_OK;
}

// the fetch's device staging buffer (2 cols + 1 doubles), kept per process and grown on demand; one fetch at a
// time (it waits for the stream anyway)
static std::mutex g_fetch_mu;
static double* g_fetch_buf = nullptr;
static long g_fetch_words = 0;

extern "C" int tnet_col_moments_fetch(const double* acc, int cols, double* first, double* second, int* bad_tag,
                                      void* stream) {
  if (!acc || cols <= 0 || ((uintptr_t)acc & 7)) return TNET_ERR_ARG;
  std::lock_guard<std::mutex> g(g_fetch_mu);
  const long n = 2L * cols;
  if (n + 1 > g_fetch_words) {
    if (g_fetch_buf) (void)hipFree(g_fetch_buf);
    g_fetch_buf = nullptr;
    g_fetch_words = 0;
    if (hipMalloc(&g_fetch_buf, (size_t)(n + 1) * sizeof(double)) != hipSuccess) return TNET_ERR_RUNTIME;
    g_fetch_words = n + 1;
  }
  hipStream_t st = (hipStream_t)stream;
  col_moments_fetch_kernel<<<cdiv(n, 64), 64, 0, st>>>(acc, cols, g_fetch_buf);
  TNET_LAUNCH_CHECK();
  std::vector<double> h((size_t)n + 1);
  if (hipMemcpyAsync(h.data(), g_fetch_buf, h.size() * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess)
    return TNET_ERR_RUNTIME;
  if (hipStreamSynchronize(st) != hipSuccess) return TNET_ERR_RUNTIME;
  for (int j = 0; j < cols; ++j) {
    if (first) first[j] = h[(size_t)j];
    if (second) second[j] = h[(size_t)cols + j];
  }
  if (bad_tag) {
    unsigned long long key;
    memcpy(&key, &h[(size_t)n], sizeof key);
    *bad_tag = key ? (int)(0xFFFFFFFFu - (unsigned)key) : -1;
  }
  return TNET_OK;
}
