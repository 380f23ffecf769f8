// wae_vq_stats_segments: the quantiser's commitment loss, perplexity and code histogram of a packed list of utterances, per utterance
// and for the list as one batch (include/wae.h).
//
// wae_vq_nearest on the packed latents of a list (B = 1, Tq = sum Tq_i) gives idx and quant per frame, but its two statistics are the
// aggregate of whatever was packed, and its squared error is a chain of float atomics in arrival order.  Here, from the latents, their
// quantised twins, the indices and a table of the items' columns: one workgroup per item counts the item's codes in LDS by integer
// atomics (exact, whatever the order) and adds its squared error in a fixed order in fp64 -- thread j takes the columns j, j + 256,
// ... and every channel of a column in turn, the 64 lanes of a wave meet by a xor butterfly, the four waves are added in wave order;
// one workgroup then adds the items' counts as integers and their squared errors in list order.  No floating-point atomics: an item's
// numbers depend on nothing but the item's columns, and the list's on nothing but the items' numbers and their order.
#include "vq_stats.hpp"

#define VQS_THREADS 256
#define VQS_MAX_K 8192      // 32 KiB of LDS for the counts

static_assert(VQS_THREADS == 256, "vq_perplexity is written for 256 threads");

__global__ void __launch_bounds__(VQS_THREADS) vq_stats_segments_kernel(const float* __restrict__ lat, const float* __restrict__ quant,
                                                                        const int64_t* __restrict__ idx,
                                                                        const wae_vq_seg* __restrict__ segs, int D, int pitch, int K,
                                                                        float c_loss, float* __restrict__ sqerr,
                                                                        int32_t* __restrict__ hist, float* __restrict__ item_stats) {
  extern __shared__ int32_t cnt[];      // K
  __shared__ double part[VQS_THREADS / 64];
  __shared__ float fpart[VQS_THREADS / 64];
  const wae_vq_seg seg = segs[blockIdx.x];
  int32_t* h = hist + (int64_t)blockIdx.x * K;
  // a record that does not fit the columns is skipped whole (uniform over the workgroup, in front of every barrier)
  if (seg.Tq < 1 || seg.q_off < 0 || (int64_t)seg.q_off + seg.Tq > pitch) {
    for (int k = threadIdx.x; k < K; k += VQS_THREADS) h[k] = 0;
    if (threadIdx.x == 0) {
      sqerr[blockIdx.x] = 0.f;
      item_stats[2 * blockIdx.x] = 0.f;
      item_stats[2 * blockIdx.x + 1] = 0.f;
    }
    return;
  }
  for (int k = threadIdx.x; k < K; k += VQS_THREADS) cnt[k] = 0;
  __syncthreads();
  const int64_t* ix = idx + seg.q_off;
  for (int t = threadIdx.x; t < seg.Tq; t += VQS_THREADS) {
    const int64_t c = ix[t];
    if (c >= 0 && c < K) atomicAdd(&cnt[(int)c], 1);      // an index outside the codebook is counted nowhere
  }
  double s = 0.0;
  for (int t = threadIdx.x; t < seg.Tq; t += VQS_THREADS) {      // adjacent lanes, adjacent columns
    const float* x = lat + seg.q_off + t;
    const float* q = quant + seg.q_off + t;
    for (int d = 0; d < D; ++d) {
      const double df = (double)q[(int64_t)d * pitch] - (double)x[(int64_t)d * pitch];
      s += df * df;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();      // the counts are complete behind it, too
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < VQS_THREADS / 64; ++i) tot += part[i];
    const float se = (float)tot;
    sqerr[blockIdx.x] = se;
    item_stats[2 * blockIdx.x] = c_loss * (se / ((float)seg.Tq * (float)D));
  }
  for (int k = threadIdx.x; k < K; k += VQS_THREADS) h[k] = cnt[k];
  const float perp = vq_perplexity(cnt, K, (float)seg.Tq, fpart);
  if (threadIdx.x == 0) item_stats[2 * blockIdx.x + 1] = perp;
}

// the list as one batch: counts added per code, squared errors and frame counts in list order.  An item's frame count is the sum of
// its counts (Tq_i for indices inside the codebook; 0 for a skipped record): the entry keeps no array of them between groups.
__global__ void __launch_bounds__(VQS_THREADS) vq_stats_total_kernel(const float* __restrict__ sqerr, const int32_t* __restrict__ hist,
                                                                     int n, int D, int K, float c_loss, float* __restrict__ out) {
  extern __shared__ int32_t cnt[];      // K
  __shared__ long long npart[VQS_THREADS / 64];
  __shared__ float fpart[VQS_THREADS / 64];
  long long mine = 0;
  for (int k = threadIdx.x; k < K; k += VQS_THREADS) {
    long long c = 0;
    for (int i = 0; i < n; ++i) c += hist[(int64_t)i * K + k];
    // one 32-bit count per code, as vq_stats_kernel reads them; a list of 2^31 frames of one code is beyond every buffer of this library
    cnt[k] = (int32_t)c;
    mine += c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
  if ((threadIdx.x & 63) == 0) npart[threadIdx.x >> 6] = mine;
  __syncthreads();
  long long frames = 0;
  for (int i = 0; i < VQS_THREADS / 64; ++i) frames += npart[i];      // integers: exact in any order
  const float perp = vq_perplexity(cnt, K, (float)frames, fpart);
  // the squared errors in list order by one thread, 256 at a time through LDS: one thread walking global memory waits out a load per
  // entry (a list of 2048 utterances in 52 groups spent 1.2 of its 9.4 ms there; the rest of this launch is the walk over the counts
  // above, n x K words through one workgroup, which grows with the entries so far: profiles/score_list.txt)
  __shared__ float stage[VQS_THREADS];
  double tot = 0.0;
  for (int i0 = 0; i0 < n; i0 += VQS_THREADS) {      // n is uniform over the workgroup: every thread meets every barrier
    const int m = min(VQS_THREADS, n - i0);
    if ((int)threadIdx.x < m) stage[threadIdx.x] = sqerr[i0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) tot += (double)stage[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool any = frames > 0;
    out[0] = any ? (float)((double)c_loss * tot / ((double)D * (double)frames)) : 0.f;
    out[1] = any ? perp : 0.f;
    out[2] = (float)frames;
    out[3] = (float)tot;
  }
}

extern "C" int wae_vq_stats_segments(const float* lat, const float* quant, const int64_t* idx, const wae_vq_seg* segs, int32_t nsegs,
                                     int32_t D, int32_t pitch, int32_t K, float c_loss, int32_t first, float* sqerr, int32_t* hist,
                                     float* item_stats, float* out, void* stream) {
  WAE_REQUIRE(lat && quant && idx && segs && sqerr && hist && item_stats && out, "vq_stats_segments: null pointer argument");
  WAE_REQUIRE(nsegs > 0 && D > 0 && K > 0 && pitch > 0 && first >= 0,
              "vq_stats_segments: nsegs, D, K and pitch must be > 0, first >= 0 (got %d, %d, %d, %d, %d)", nsegs, D, K, pitch, first);
  if (K > VQS_MAX_K) {
    wae_set_error("vq_stats_segments: K = %d codes; the counts of an item stay in LDS, at most %d", K, VQS_MAX_K);
    return WAE_EUNSUPPORTED;
  }
  hipStream_t st = as_stream(stream);
  const size_t lds = (size_t)K * sizeof(int32_t);
  // this group's entries of the list's per-item arrays, then the totals over every entry so far (the whole list behind the last group)
  hipLaunchKernelGGL(vq_stats_segments_kernel, dim3(nsegs), dim3(VQS_THREADS), lds, st, lat, quant, idx, segs, D, pitch, K, c_loss,
                     sqerr + first, hist + (int64_t)first * K, item_stats + 2 * (int64_t)first);
  if (int rc = wae_check_launch("vq_stats_segments"); rc != WAE_OK) return rc;
  hipLaunchKernelGGL(vq_stats_total_kernel, dim3(1), dim3(VQS_THREADS), lds, st, (const float*)sqerr, (const int32_t*)hist,
                     first + nsegs, D, K, c_loss, out);
  return wae_check_launch("vq_stats_segments (total)");
}
