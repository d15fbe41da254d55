// feacat_emit.hip -- the output stage of the forward pass (TFeaCatCu.cc:236-265) as one memory-bound launch:
// the rows a segment table selects (every utterance's context rows left out), GMMBYPASS / LOGPOSTERIOR in the
// reference's order, the byte order of the file, stored as dense C-word rows -- an utterance's file body as one
// contiguous range, whatever the stride of the matrix the network left.
//
//   feacat_emit_kernel   from the network's output Y.  A segment's output is contiguous across its rows, so it is
//                        indexed flat: one thread per 16-byte ALIGNED group of four output words (the group's
//                        position is taken from the output address, so C odd and destination offsets that are only
//                        4-byte aligned still store 16 bytes at a time; only the first and the last group of a
//                        segment can be partial, and store their words one by one).  16-byte loads where every
//                        group is four columns of one aligned source row (VEC), scalar loads otherwise.
//   softmax_emit_kernel  from the pre-softmax activations Z: softmax_row_norm (softmax_row.h, the normaliser of
//                        tnetF_softmax's kernel) per emitted row, one wave a row, then the same mode / swap /
//                        dense store -- the posterior matrix never reaches HBM.
//
// The segment table travels in the kernel arguments (FE_MAXSEG segments a launch): no device table to allocate,
// upload or keep alive, and the host arrays may be reused as soon as the call returns.
//
// The mode arithmetic is fp64 from the fp32 input, rounded once per step: the reference's lines call the C
// log(double) / sqrt(double) on a float and cast the result (tests/golden/feacat_ref.npz settles it: bit-equal).
#include <algorithm>
#include <vector>

#include "kcommon.h"
#include "softmax_row.h"

namespace tnetk {

constexpr int FE_MAXSEG = 64;

struct EmitSegs {
  int n;
  int src[FE_MAXSEG];        // first source row
  int first[FE_MAXSEG + 1];  // cumulative work items of the launch: 16-byte output groups (emit) / rows (softmax)
  long dst[FE_MAXSEG];       // first output word
  int words[FE_MAXSEG];      // rows * C
};

template <int MODE>
__device__ __forceinline__ float emit_fn(float y) {
  if (MODE & TNET_FEACAT_GMMBYPASS) y = (float)sqrt(-2.0 * log((double)y));
  if (MODE & TNET_FEACAT_LOGPOSTERIOR) y = (float)log((double)y);
  return y;
}
template <int MODE, bool SWAP>
__device__ __forceinline__ unsigned emit_word(float y) {
  const unsigned w = __float_as_uint(emit_fn<MODE>(y));
  return SWAP ? __builtin_bswap32(w) : w;
}

// the segment of work item g: the largest s with first[s] <= g (an empty segment is never the answer: its
// successor's `first` is the same)
__device__ __forceinline__ int emit_find(const EmitSegs& T, const int g) {
  int lo = 0, hi = T.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (T.first[mid] <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <int MODE, bool SWAP, bool VEC>
__global__ __launch_bounds__(256) void feacat_emit_kernel(const float* __restrict__ Y, const int C, const int stride,
                                                          const EmitSegs T, unsigned* __restrict__ out) {
  const int g = (int)(blockIdx.x * 256 + threadIdx.x);
  if (g >= T.first[T.n]) return;
  const int s = emit_find(T, g);
  const int k = g - T.first[s];
  const float* __restrict__ base = Y + (long)T.src[s] * stride;
  if (VEC) {  // every group is four columns of one 16-byte aligned source row, and 16-byte aligned in `out`
    const unsigned i = 4u * (unsigned)k, row = i / (unsigned)C, col = i - row * (unsigned)C;
    const f32x4 y = *reinterpret_cast<const f32x4*>(base + (long)row * stride + col);
    u32x4 w;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = emit_word<MODE, SWAP>(y[e]);
    *reinterpret_cast<u32x4*>(out + T.dst[s] + i) = w;
    return;
  }
  // the segment's first word sits `head` words into its first aligned group
  const int head = (int)((((uintptr_t)out >> 2) + (unsigned long)T.dst[s]) & 3);
  const int words = T.words[s];
  const int i0 = 4 * k - head;  // segment-relative index of the group's first word (< 0 in the first group)
  const int ib = i0 < 0 ? 0 : i0;
  unsigned row = (unsigned)ib / (unsigned)C, col = (unsigned)ib - row * (unsigned)C;
  const float* __restrict__ p = base + (long)row * stride;
  unsigned* __restrict__ o = out + T.dst[s] + i0;
  u32x4 w;
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = i0 + e;
    ok[e] = i >= 0 && i < words;
    w[e] = 0;
    if (ok[e]) {
      w[e] = emit_word<MODE, SWAP>(p[col]);
      if (++col == (unsigned)C) {
        col = 0;
        p += stride;
      }
    }
  }
  if (ok[0] && ok[3]) {
    *reinterpret_cast<u32x4*>(o) = w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ok[e]) o[e] = w[e];
  }
}

// one wave per emitted row, four rows a workgroup (softmax_xent_kernel's geometry)
template <int MODE, bool SWAP>
__global__ __launch_bounds__(256) void softmax_emit_kernel(const float* __restrict__ Z, const int C, const int stride,
                                                           const EmitSegs T, unsigned* __restrict__ out,
                                                           const int vec4) {
  const int lane = threadIdx.x & 63;
  const int g = (int)((blockIdx.x * 256 + threadIdx.x) >> 6);
  if (g >= T.first[T.n]) return;
  const int s = emit_find(T, g);
  const int r = g - T.first[s];
  const float* __restrict__ src = Z + (long)(T.src[s] + r) * stride;
  unsigned* __restrict__ o = out + T.dst[s] + (long)r * C;
  const bool cached = vec4 && C <= SX_MAXV4 * 256;
  f32x4 rv[SX_MAXV4];
  float m, rsum;
  softmax_row_norm(src, C, lane, cached, true, rv, m, rsum);
  if (cached) {
    const bool st16 = ((uintptr_t)o & 15) == 0;  // C % 4 == 0 here: every lane's four words are aligned or none is
#pragma unroll
    for (int j = 0; j < SX_MAXV4; ++j) {
      const int c = j * 256 + lane * 4;
      if (c < C) {
        u32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = emit_word<MODE, SWAP>(rv[j][e] * rsum);
        if (st16) {
          *reinterpret_cast<u32x4*>(o + c) = w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[c + e] = w[e];
        }
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) o[c] = emit_word<MODE, SWAP>(fast_exp(src[c] - m) * rsum);
  }
}

// Host side of both calls: the checks, and the table cut into launches of at most FE_MAXSEG segments.
// per_group: work items are 16-byte output groups (emit); otherwise rows (softmax).
struct EmitPlan {
  std::vector<EmitSegs> launches;
  bool all_aligned = true;  // every non-empty segment starts on a multiple of four words (relative to `out`)
};

static int emit_plan(TnetMatrixDim d, const int* src, const int* dst, const int* rows, int nseg, const void* in,
                     const void* out, bool per_group, EmitPlan& plan) {
  if (nseg < 0 || d.rows < 0 || d.cols <= 0 || d.stride < d.cols) return TNET_ERR_ARG;
  if (nseg > 0 && (!src || !dst || !rows)) return TNET_ERR_ARG;
  std::vector<std::pair<long, long>> ranges;  // destination rows [a, b) of the non-empty segments
  long total = 0;
  for (int s = 0; s < nseg; s++) {
    if (rows[s] < 0 || src[s] < 0 || dst[s] < 0 || (long)src[s] + rows[s] > d.rows) return TNET_ERR_ARG;
    if (rows[s]) ranges.emplace_back((long)dst[s], (long)dst[s] + rows[s]);
    total += rows[s];
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); i++)
    if (ranges[i].first < ranges[i - 1].second) return TNET_ERR_ARG;
  if (!total) return TNET_OK;
  if (!in || !out || ((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return TNET_ERR_ARG;
  const unsigned long obase = (uintptr_t)out >> 2;
  EmitSegs cur{};
  auto flush = [&]() {
    if (cur.n && cur.first[cur.n] > 0) plan.launches.push_back(cur);
    cur = EmitSegs{};
  };
  for (int s = 0; s < nseg; s++) {
    if (!rows[s]) continue;
    const long words = (long)rows[s] * d.cols;
    if (words >= (1L << 31)) return TNET_ERR_UNSUPPORTED;
    const long dw = (long)dst[s] * d.cols;
    const int head = (int)((obase + (unsigned long)dw) & 3);
    if (head) plan.all_aligned = false;
    const long items = per_group ? (head + words + 3) / 4 : (long)rows[s];
    if (cur.n == FE_MAXSEG || (long)cur.first[cur.n] + items >= (1L << 30)) flush();
    cur.src[cur.n] = src[s];
    cur.dst[cur.n] = dw;
    cur.words[cur.n] = (int)words;
    cur.first[cur.n + 1] = cur.first[cur.n] + (int)items;
    cur.n++;
  }
  flush();
  return TNET_OK;
}

template <int MODE, bool SWAP>
static void emit_launch(const float* Y, TnetMatrixDim d, const EmitSegs& T, bool vec, unsigned* out, hipStream_t st) {
  const unsigned grid = (unsigned)cdiv(T.first[T.n], 256);
  if (vec) feacat_emit_kernel<MODE, SWAP, true><<<grid, 256, 0, st>>>(Y, d.cols, d.stride, T, out);
  else feacat_emit_kernel<MODE, SWAP, false><<<grid, 256, 0, st>>>(Y, d.cols, d.stride, T, out);
}
template <int MODE, bool SWAP>
static void softmax_launch(const float* Z, TnetMatrixDim d, const EmitSegs& T, bool vec, unsigned* out,
                           hipStream_t st) {
  const unsigned grid = (unsigned)cdiv((long)T.first[T.n] * 64, 256);
  softmax_emit_kernel<MODE, SWAP><<<grid, 256, 0, st>>>(Z, d.cols, d.stride, T, out, vec ? 1 : 0);
}

typedef void (*EmitFn)(const float*, TnetMatrixDim, const EmitSegs&, bool, unsigned*, hipStream_t);
static EmitFn pick(bool softmax, int mode, bool swap) {
  static const EmitFn emit[8] = {emit_launch<0, false>, emit_launch<1, false>, emit_launch<2, false>,
                                 emit_launch<3, false>, emit_launch<0, true>,  emit_launch<1, true>,
                                 emit_launch<2, true>,  emit_launch<3, true>};
  static const EmitFn smax[8] = {softmax_launch<0, false>, softmax_launch<1, false>, softmax_launch<2, false>,
                                 softmax_launch<3, false>, softmax_launch<0, true>,  softmax_launch<1, true>,
                                 softmax_launch<2, true>,  softmax_launch<3, true>};
  return (softmax ? smax : emit)[(swap ? 4 : 0) + mode];
}

static int emit_run(bool softmax, const float* M, TnetMatrixDim d, const int* src, const int* dst, const int* rows,
                    int nseg, int mode, int swap, void* out, void* stream) {
  if (mode < 0 || mode > 3) return TNET_ERR_ARG;
  EmitPlan plan;
  const int rc = emit_plan(d, src, dst, rows, nseg, M, out, !softmax, plan);
  if (rc != TNET_OK) return rc;
  const bool src16 = (d.cols & 3) == 0 && (d.stride & 3) == 0 && ((uintptr_t)M & 15) == 0;
  // emit: 16-byte loads need every group to be four columns of one row; softmax: tnetF_softmax's own test
  const bool vec = softmax ? src16 : (src16 && plan.all_aligned);
  const EmitFn fn = pick(softmax, mode, swap != 0);
  for (const EmitSegs& T : plan.launches) {
    fn(M, d, T, vec, (unsigned*)out, (hipStream_t)stream);
    TNET_LAUNCH_CHECK();
  }
  return TNET_OK;
}

}  // namespace tnetk

using namespace tnetk;

extern "C" int tnet_feacat_emit(const float* Y, TnetMatrixDim dY, const int* seg_src_row, const int* seg_dst_row,
                                const int* seg_rows, int nseg, int mode, int swap, void* out, void* stream) {
  return emit_run(false, Y, dY, seg_src_row, seg_dst_row, seg_rows, nseg, mode, swap, out, stream);
}

extern "C" int tnet_softmax_emit(const float* Z, TnetMatrixDim dZ, const int* seg_src_row, const int* seg_dst_row,
                                 const int* seg_rows, int nseg, int mode, int swap, void* out, void* stream) {
  return emit_run(true, Z, dZ, seg_src_row, seg_dst_row, seg_rows, nseg, mode, swap, out, stream);
}
