// wae_nll_segments: the shifted cross-entropy of a packed list of utterances, per utterance (include/wae.h).
//
// The head kernels run on the packed rows of a list as ONE clip of `rows` steps (they are per column), so their nll takes the last
// row of item i against the first id of item i + 1.  Here, from that nll and the list's wae_glu_seg table: the last row of every item
// becomes 0 (what the item's own forward reports at t = T - 1), nll_sum[i] / count[i] are the item's masked sum and mask size, and
// out[0] the list's masked mean (vqwae_train.py:379 with the list as one batch).
// Deterministic by construction: one workgroup per item, thread j adds the rows j, j + 256, ... of the item in that order in fp64,
// the 64 lanes of a wave meet by a xor butterfly, the four waves are added in wave order; one thread then walks nll_sum in table
// order.  No atomics: an item's nll_sum depends on nothing but the item's rows.
#include "wae_common.hpp"

#define NLS_THREADS 256

__global__ void __launch_bounds__(NLS_THREADS) nll_segments_kernel(float* __restrict__ nll, const wae_glu_seg* __restrict__ segs,
                                                                   int rows, float* __restrict__ nll_sum, int32_t* __restrict__ count) {
  __shared__ double part[NLS_THREADS / 64];
  const wae_glu_seg seg = segs[blockIdx.x];
  // a record that does not fit the rows is skipped whole (uniform over the workgroup, in front of the barrier)
  if (seg.T < 1 || seg.row_off < 0 || (int64_t)seg.row_off + seg.T > rows) {
    if (threadIdx.x == 0) {
      nll_sum[blockIdx.x] = 0.f;
      count[blockIdx.x] = 0;
    }
    return;
  }
  float* r = nll + seg.row_off;
  double s = 0.0;
  for (int t = threadIdx.x; t < seg.T - 1; t += NLS_THREADS) s += (double)r[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < NLS_THREADS / 64; ++i) tot += part[i];
    nll_sum[blockIdx.x] = (float)tot;
    count[blockIdx.x] = seg.T - 1;
    r[seg.T - 1] = 0.f;      // no thread of this workgroup reads that row, and no other workgroup owns it
  }
}

__global__ void __launch_bounds__(64) nll_segments_total_kernel(const float* __restrict__ nll_sum, const int32_t* __restrict__ count,
                                                                int nsegs, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double tot = 0.0, cnt = 0.0;
  for (int i = 0; i < nsegs; ++i) {      // table order
    tot += (double)nll_sum[i];
    cnt += (double)count[i];
  }
  out[0] = cnt > 0.0 ? (float)(tot / cnt) : 0.f;
  out[1] = (float)cnt;
}

extern "C" int wae_nll_segments(float* nll, const wae_glu_seg* segs, int32_t nsegs, int32_t rows, int32_t first, float* nll_sum,
                                int32_t* count, float* out, void* stream) {
  WAE_REQUIRE(nll && segs && nll_sum && count && out, "nll_segments: null pointer argument");
  WAE_REQUIRE(nsegs > 0 && rows > 0 && first >= 0, "nll_segments: nsegs and rows must be > 0, first >= 0 (got %d, %d, %d)", nsegs, rows,
              first);
  hipStream_t st = as_stream(stream);
  // this group's entries of the list's nll_sum / count, then the mean over every entry so far (the whole list behind the last group)
  hipLaunchKernelGGL(nll_segments_kernel, dim3(nsegs), dim3(NLS_THREADS), 0, st, nll, segs, rows, nll_sum + first, count + first);
  if (int rc = wae_check_launch("nll_segments"); rc != WAE_OK) return rc;
  hipLaunchKernelGGL(nll_segments_total_kernel, dim3(1), dim3(64), 0, st, (const float*)nll_sum, (const int32_t*)count, first + nsegs,
                     out);
  return wae_check_launch("nll_segments (total)");
}
