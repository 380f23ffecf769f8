// The quantiser's perplexity from code counts, shared by vq_stats_kernel (csrc/misc.hip: one slice of a dense batch) and the list
// kernels (csrc/vq_list.hip: per utterance and for the list): one function, so the three values agree bit for bit on equal counts.
#pragma once
#include "wae_common.hpp"

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// exp(-sum_k p_k log(p_k + 1e-10)), p_k = hist[k] / n (vector_quantization.py:45-47), for a workgroup of 256 threads: thread j takes
// the codes j, j + 256, ..., the 64 lanes of a wave meet by a xor butterfly, the four waves are added in wave order.  Every thread of
// the workgroup calls it (one barrier inside) and every thread gets the value.  hist: K counts in global memory or in LDS, complete
// and visible before the call; n: the frame count as a float; part: 4 floats of LDS; on = false leaves the counts unread (the sum is
// 0, the value 1).
__device__ __forceinline__ float vq_perplexity(const int32_t* __restrict__ hist, int K, float n, float* part, bool on = true) {
  float s = 0.f;
  if (on)
    for (int k = threadIdx.x; k < K; k += 256) {
      const float pk = (float)hist[k] / n;
      s += pk * logf(pk + 1e-10f);
    }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  const float tot = part[0] + part[1] + part[2] + part[3];
  return expf(-tot);
}
