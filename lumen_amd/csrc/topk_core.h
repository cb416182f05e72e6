// The workgroup body of the row top-k (topk.hip) as a device function, so the vocab sampler
// (sampler.hip) runs the very same scan, statistics and merge with a per-element transform in
// front and its own consumer of the winners behind.
//
// One 256-thread workgroup handles columns [part * chunk, min(N, (part + 1) * chunk)) of one
// row: every thread streams a strided slice keeping a sorted register list of its K best and an
// online (max, sum-exp); the block then merges by k rounds of a block arg-max over the list
// heads.  `xf(x, j)` maps the loaded value of column j before it is ranked and summed
// (TopkIdentity: nothing); `sink(r, v, i)` is called by EVERY thread with the r-th winner
// (TopkStore: thread 0 writes it to the output rows).
#pragma once
#include "common.h"

namespace lumen {

constexpr int TOPK_CHUNK = 4096;

// kSkipNegInf: the transform masks columns to -inf and the scan passes over those (the online
// sum-exp of a list that STARTS with -inf would be exp(-inf - -inf) = NaN); other transforms scan as before
struct TopkIdentity {
  static constexpr bool kSkipNegInf = false;
  __device__ __forceinline__ float operator()(const float x, const int) const { return x; }
};

struct TopkStore {
  float* out_v;
  int* out_i;
  int64_t obase;
  int index_offset;
  __device__ __forceinline__ void operator()(const int r, const float fv, const int fi) const {
    if (threadIdx.x == 0) {
      out_v[obase + r] = fv;
      out_i[obase + r] = fi < 0 ? -1 : fi + index_offset;
    }
  }
};

// Returns the row log-sum-exp in thread 0 (0 elsewhere, and when neither out_lse nor a merge /
// single-chunk statistic is computed); also stored to out_lse[row] when that is set.
template <int K, class XF, class Sink>
__device__ __forceinline__ float topk_block(const float* __restrict__ scores, int64_t ld, int N, int k, float scale,
                                            float* __restrict__ out_lse, const int* __restrict__ in_idx,
                                            const float* __restrict__ in_ml, int nparts, int chunk,
                                            float* __restrict__ out_ml, bool want_lse, const XF& xf, Sink& sink) {
  const int row = blockIdx.x, part = blockIdx.y, nblk = gridDim.y;
  const float* s = scores + (int64_t)row * ld;
  const int* ix = in_idx ? in_idx + (int64_t)row * ld : nullptr;
  const int j0 = part * chunk, j1 = min(N, j0 + chunk);
  float lse = 0.f;
  float v[K];
  int id[K];
#pragma unroll
  for (int i = 0; i < K; ++i) { v[i] = -INFINITY; id[i] = -1; }
  float m = -INFINITY, l = 0.f;
  auto take = [&](const float x, const int j) {
    if constexpr (XF::kSkipNegInf) {
      if (x == -INFINITY) return;   // never a candidate, adds nothing to the sum
    }
    if (!in_ml) {
      const float xs = x * scale;
      if (xs > m) { l = l * __expf(m - xs) + 1.f; m = xs; }
      else l += __expf(xs - m);
    }
    if (x > v[K - 1]) {
      v[K - 1] = x; id[K - 1] = j;
#pragma unroll
      for (int i = K - 1; i > 0; --i) {
        if (v[i] > v[i - 1]) {
          float tv = v[i]; v[i] = v[i - 1]; v[i - 1] = tv;
          int ti = id[i]; id[i] = id[i - 1]; id[i - 1] = ti;
        }
      }
    }
  };
  // 8 loads in flight per thread before any is consumed: a strided scalar loop paid one
  // dependent memory round trip per element (16 per thread on a 4096-column chunk)
  constexpr int LU = 8;
  for (int j = j0 + threadIdx.x; j < j1; j += 256 * LU) {
    float xv[LU];
    int iv[LU];
#pragma unroll
    for (int u = 0; u < LU; ++u) {
      const int jj = min(j + u * 256, j1 - 1);
      xv[u] = s[jj];
      iv[u] = ix ? ix[jj] : jj;
    }
#pragma unroll
    for (int u = 0; u < LU; ++u)
      if (j + u * 256 < j1) take(xf(xv[u], j + u * 256), iv[u]);
  }
  __shared__ float red_v[4];
  __shared__ int red_i[4];
  __shared__ float red_m[4], red_l[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // block log-sum-exp (or the merge of phase-1 partials)
  if (in_ml) {
    if (want_lse) {   // merge the phase-1 (max, sum-exp) partials: one per thread, then a block reduction
      const float* pm = in_ml + (int64_t)row * nparts * 2;
      float pmx = -INFINITY, pl = 0.f;
      for (int p = threadIdx.x; p < nparts; p += 256) {
        const float qm = pm[2 * p], ql = pm[2 * p + 1];
        if (qm == -INFINITY) continue;
        if (qm > pmx) { pl = pl * __expf(pmx - qm) + ql; pmx = qm; }
        else pl += ql * __expf(qm - pmx);
      }
      float mm = pmx;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
      float ll = pmx == -INFINITY ? 0.f : pl * __expf(pmx - mm);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ll += __shfl_xor(ll, o, 64);
      if (lane == 0) { red_m[w] = mm; red_l[w] = ll; }
      __syncthreads();
      if (threadIdx.x == 0) {
        const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        float L = 0.f;
        for (int i = 0; i < 4; ++i) L += red_m[i] == -INFINITY ? 0.f : red_l[i] * __expf(red_m[i] - M);
        lse = M + logf(L);
        if (out_lse) out_lse[row] = lse;
      }
    }
  } else {
    float mm = m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mm = fmaxf(mm, __shfl_xor(mm, o, 64));
    float ll = (m == -INFINITY) ? 0.f : l * __expf(m - mm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ll += __shfl_xor(ll, o, 64);
    if (lane == 0) { red_m[w] = mm; red_l[w] = ll; }
    __syncthreads();
    if (threadIdx.x == 0) {
      float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
      float L = 0.f;
      for (int i = 0; i < 4; ++i) L += red_m[i] == -INFINITY ? 0.f : red_l[i] * __expf(red_m[i] - M);
      if (out_ml) { out_ml[((int64_t)row * nblk + part) * 2] = M; out_ml[((int64_t)row * nblk + part) * 2 + 1] = L; }
      else if (want_lse) {
        lse = M + logf(L);
        if (out_lse) out_lse[row] = lse;
      }
    }
  }
  // K rounds of block arg-max over list heads
  for (int r = 0; r < k; ++r) {
    float bv = v[0];
    int bi = id[0], bt = threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      float ov = __shfl_xor(bv, o, 64);
      int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
      if (ov > bv || (ov == bv && oi >= 0 && (bi < 0 || oi < bi))) { bv = ov; bi = oi; bt = ot; }
    }
    __syncthreads();
    if (lane == 0) { red_v[w] = bv; red_i[w] = bi; red_l[w] = __int_as_float(bt); }
    __syncthreads();
    float fv = red_v[0];
    int fi = red_i[0], ft = __float_as_int(red_l[0]);
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (red_v[q] > fv || (red_v[q] == fv && red_i[q] >= 0 && (fi < 0 || red_i[q] < fi))) {
        fv = red_v[q]; fi = red_i[q]; ft = __float_as_int(red_l[q]);
      }
    }
    sink(r, fv, fi);
    if (threadIdx.x == ft) {  // pop the winner's head
#pragma unroll
      for (int i = 0; i < K - 1; ++i) { v[i] = v[i + 1]; id[i] = id[i + 1]; }
      v[K - 1] = -INFINITY; id[K - 1] = -1;
    }
  }
  return lse;
}

}  // namespace lumen
