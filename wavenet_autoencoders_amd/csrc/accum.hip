// Gradient accumulation (engine.py: accumulate / apply_step): the two pieces of device code a window of micro-batches needs beside the
// kernels of a plain step.
//   wae_gproj_bwd_consume: wae_gproj_bwd (csrc/misc.hip) that zeroes the per-clip columns it has read.  The weight-gradient launches
//     add sum_t dz[b,t,row] of clip b into column ones_col + b of the layer's dW1 tile; the zb chain turns those columns into the
//     conv bias, conv1x1g and speaker-embedding gradients with THIS batch's speaker ids.  Inside a window the tiles are not cleared
//     between micro-batches, so the columns are consumed here: the next micro-batch's clip b starts from zero.
//   wae_accum_stats: the window's logged numbers, in a fixed order on one workgroup (no floating-point atomics).
#include "wae_common.hpp"
#include "vq_stats.hpp"

#define ACC_BMAX 32   // clips per launch: csrc/misc.hip GPROJ_BMAX (the sums of a group stay in LDS)

__device__ __forceinline__ int acc_checked_id(int v, int n) { return (unsigned)v >= (unsigned)n ? (v < 0 ? 0 : n - 1) : v; }

// Block = (layer, 32 gate rows), thread = (row, feature slice): the arithmetic of gproj_bwd_kernel statement for statement -- the same
// sums in the same order, so d_eff gets the same bits.  The one difference: the thread that stages c1[row][ones_col + B0 + b] stores
// 0.0f to the address it has just read (a plain vector store; no other thread of the grid touches that element).
// DET (wae_gproj_bwd_det): phase 2 stores its (layer, row block, clip, feature) sum to `parts` instead of adding it to the embedding row
// by an atomic (gproj_emb_finish_kernel adds them in a fixed order); CONSUME = false there leaves c1 as it is (a plain step).
template <bool CONSUME, bool DET>
__device__ __forceinline__ void gproj_bwd_consume_body(const float* __restrict__ eff, float* __restrict__ d_eff, int64_t wg_off,
                                                       int64_t bias_off, int64_t layer_stride, const int32_t* __restrict__ gid,
                                                       int64_t emb_off, const float* __restrict__ gvec, float* c1,
                                                       int64_t c_layer_stride, int64_t ld, int ones_col, int B0, int B, int G, int Hp,
                                                       int Cg, int n_speakers, float* __restrict__ parts) {
  extern __shared__ float ga_lds[];
  float* s_cl = ga_lds;                      // [32][ACC_BMAX]
  float* s_e = ga_lds + 32 * ACC_BMAX;       // [nb][Cg]
  __shared__ int s_sp[ACC_BMAX];
  const int l = blockIdx.x;
  const int H = G / 2;
  float* cl = c1 + (int64_t)l * c_layer_stride + ones_col;
  const bool proj = wg_off >= 0 && Cg > 0;
  const int nb = min(B - B0, ACC_BMAX);
  const int rr1 = threadIdx.x >> 3, r1 = blockIdx.y * 32 + rr1, cs = threadIdx.x & 7;
  const int half1 = r1 >= Hp, i1 = r1 - half1 * Hp;
  const bool live1 = r1 < 2 * Hp && i1 < H;
  const int ch1 = half1 * H + i1;
  float* dwg = d_eff + wg_off + (int64_t)l * layer_stride + (int64_t)ch1 * Cg;
  float* dbias = d_eff + bias_off + (int64_t)l * layer_stride + ch1;
  constexpr int PRE = 16;
  float pre[PRE], pre_b = 0.f;
  const bool use_pre = Cg <= 8 * PRE;
  if (live1) {
    if (cs == 0) pre_b = *dbias;
    if (proj && use_pre) {
#pragma unroll
      for (int k = 0; k < PRE; ++k) pre[k] = cs + 8 * k < Cg ? dwg[cs + 8 * k] : 0.f;
    }
  }
  for (int e = threadIdx.x; e < 32 * nb; e += 256) {
    const int rr = e / nb, b = e - rr * nb, r = blockIdx.y * 32 + rr;
    float v = 0.f;
    if (r < 2 * Hp) {
      float* p = cl + (int64_t)r * ld + B0 + b;
      v = *p;
      if constexpr (CONSUME) *p = 0.f;       // consumed
    }
    s_cl[rr * ACC_BMAX + b] = v;
  }
  if (gid && threadIdx.x < nb) s_sp[threadIdx.x] = acc_checked_id(gid[B0 + threadIdx.x], n_speakers);
  __syncthreads();
  if (proj)
    for (int e = threadIdx.x; e < nb * Cg; e += 256) {
      const int b = e / Cg, c = e - b * Cg;
      s_e[e] = gid ? eff[emb_off + (int64_t)s_sp[b] * Cg + c] : gvec[(int64_t)(B0 + b) * Cg + c];
    }
  __syncthreads();
  // phase 1: bias gradient and the row of dWg
  if (live1) {
    if (cs == 0) {
      float sb = 0.f;
      for (int b = 0; b < nb; ++b) sb += s_cl[rr1 * ACC_BMAX + b];
      *dbias = pre_b + sb;
    }
    if (proj) {
      if (use_pre) {
#pragma unroll
        for (int k = 0; k < PRE; ++k) {
          const int c = cs + 8 * k;
          if (c < Cg) {
            float a = 0.f;
            for (int b = 0; b < nb; ++b) a = fmaf(s_cl[rr1 * ACC_BMAX + b], s_e[b * Cg + c], a);
            dwg[c] = pre[k] + a;
          }
        }
      } else {
        for (int c = cs; c < Cg; c += 8) {
          float a = 0.f;
          for (int b = 0; b < nb; ++b) a = fmaf(s_cl[rr1 * ACC_BMAX + b], s_e[b * Cg + c], a);
          dwg[c] += a;
        }
      }
    }
  }
  // phase 2: embedding rows: thread per (clip, feature) reduces over this block's 32 gate rows -> one atomic each (as gproj_bwd_kernel)
  if (gid && proj) {
    for (int e = threadIdx.x; e < nb * Cg; e += 256) {
      const int b = e / Cg, c = e - b * Cg;
      float wv[32];
#pragma unroll
      for (int rr = 0; rr < 32; ++rr) {
        const int r = blockIdx.y * 32 + rr;
        const int half = r >= Hp, i = r - half * Hp;
        wv[rr] = (r < 2 * Hp && i < H) ? eff[wg_off + (int64_t)l * layer_stride + (int64_t)(half * H + i) * Cg + c] : 0.f;
      }
      float a = 0.f;
#pragma unroll
      for (int rr = 0; rr < 32; ++rr) a = fmaf(s_cl[rr * ACC_BMAX + b], wv[rr], a);
      if constexpr (DET) parts[((((int64_t)l * gridDim.y + blockIdx.y) * B) + B0 + b) * Cg + c] = a;
      else atomicAdd(d_eff + emb_off + (int64_t)s_sp[b] * Cg + c, a);
    }
  }
}
__global__ void __launch_bounds__(256) gproj_bwd_consume_kernel(const float* __restrict__ eff, float* __restrict__ d_eff, int64_t wg_off,
                                                                int64_t bias_off, int64_t layer_stride,
                                                                const int32_t* __restrict__ gid, int64_t emb_off,
                                                                const float* __restrict__ gvec, float* c1, int64_t c_layer_stride,
                                                                int64_t ld, int ones_col, int B0, int B, int G, int Hp, int Cg,
                                                                int n_speakers) {
  gproj_bwd_consume_body<true, false>(eff, d_eff, wg_off, bias_off, layer_stride, gid, emb_off, gvec, c1, c_layer_stride, ld, ones_col, B0,
                                      B, G, Hp, Cg, n_speakers, nullptr);
}
template <bool CONSUME>
__global__ void __launch_bounds__(256) gproj_bwd_det_kernel(const float* __restrict__ eff, float* __restrict__ d_eff, int64_t wg_off,
                                                            int64_t bias_off, int64_t layer_stride, const int32_t* __restrict__ gid,
                                                            int64_t emb_off, const float* __restrict__ gvec, float* c1,
                                                            int64_t c_layer_stride, int64_t ld, int ones_col, int B0, int B, int G,
                                                            int Hp, int Cg, int n_speakers, float* __restrict__ parts) {
  gproj_bwd_consume_body<CONSUME, true>(eff, d_eff, wg_off, bias_off, layer_stride, gid, emb_off, gvec, c1, c_layer_stride, ld, ones_col,
                                        B0, B, G, Hp, Cg, n_speakers, parts);
}
// The embedding rows from parts[layer][row block][clip][feature], one OWNER per (speaker, feature): the thread of (clip b, feature c)
// where b is the FIRST clip of its speaker adds, for the clips b' = b, b + 1, ... of that speaker in index order, the layers 0 .. L-1
// and inside a layer the row blocks 0 .. nblk-1 (started from zero), and adds the sum to the row with one plain read-modify-write.
__global__ void __launch_bounds__(256) gproj_emb_finish_kernel(const float* __restrict__ parts, const int32_t* __restrict__ gid,
                                                               float* __restrict__ d_eff, int64_t emb_off, int B, int L, int nblk, int Cg,
                                                               int n_speakers) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= B * Cg) return;
  const int b = e / Cg, c = e - b * Cg;
  const int sp = acc_checked_id(gid[b], n_speakers);
  for (int i = 0; i < b; ++i)
    if (acc_checked_id(gid[i], n_speakers) == sp) return;      // an earlier clip of the speaker owns the row
  float a = 0.f;
  for (int i = b; i < B; ++i) {
    if (acc_checked_id(gid[i], n_speakers) != sp) continue;
    for (int l = 0; l < L; ++l)
      for (int k = 0; k < nblk; ++k) a += parts[((((int64_t)l * nblk + k) * B) + i) * Cg + c];
  }
  float* dst = d_eff + emb_off + (int64_t)sp * Cg + c;
  *dst = *dst + a;
}

extern "C" int wae_gproj_bwd_consume(const float* eff, float* d_eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride,
                                     const int32_t* gid, int64_t emb_off, const float* gvec, float* c1, int64_t c_layer_stride,
                                     int64_t ld, int32_t ones_col, int32_t B, int32_t L, int32_t G, int32_t Hp, int32_t Cg,
                                     int32_t n_speakers, void* stream) {
  WAE_REQUIRE(eff && d_eff && c1 && B > 0 && L > 0 && G > 0 && G % 2 == 0, "gproj_bwd_consume: bad arguments");
  WAE_REQUIRE(!gid || n_speakers > 0, "gproj_bwd_consume: speaker ids need the size of the embedding table");
  WAE_REQUIRE(Hp >= G / 2 && ones_col >= 0 && ld >= (int64_t)ones_col + B && c_layer_stride >= (int64_t)2 * Hp * ld,
              "gproj_bwd_consume: the %d per-clip columns at %d do not fit rows of %lld floats (layer stride %lld)", B, ones_col,
              (long long)ld, (long long)c_layer_stride);
  const int64_t wg = (gid || gvec) ? wg_off : -1;
  const size_t lds = (32 * ACC_BMAX + (size_t)ACC_BMAX * (Cg > 0 ? Cg : 0)) * sizeof(float);
  WAE_REQUIRE(lds <= 64 * 1024, "gproj_bwd_consume: Cg = %d too wide for the staged form", Cg);
  for (int b0 = 0; b0 < B; b0 += ACC_BMAX) {
    hipLaunchKernelGGL(gproj_bwd_consume_kernel, dim3(L, (2 * Hp + 31) / 32), dim3(256), lds, as_stream(stream), eff, d_eff, wg,
                       bias_off, layer_stride, gid, emb_off, gvec, c1, c_layer_stride, ld, ones_col, b0, B, G, Hp, Cg, n_speakers);
  }
  return wae_check_launch("gproj_bwd_consume");
}

extern "C" int64_t wae_gproj_bwd_det_floats(int32_t B, int32_t L, int32_t Hp, int32_t Cg) {
  if (B <= 0 || L <= 0 || Hp <= 0 || Cg <= 0) return 0;
  return (int64_t)L * ((2 * Hp + 31) / 32) * B * Cg;
}
extern "C" int wae_gproj_bwd_det(const float* eff, float* d_eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride,
                                 const int32_t* gid, int64_t emb_off, const float* gvec, float* c1, int64_t c_layer_stride, int64_t ld,
                                 int32_t ones_col, int32_t B, int32_t L, int32_t G, int32_t Hp, int32_t Cg, int32_t n_speakers,
                                 int32_t consume, float* parts, int64_t parts_floats, void* stream) {
  WAE_REQUIRE(eff && d_eff && c1 && B > 0 && L > 0 && G > 0 && G % 2 == 0, "gproj_bwd_det: bad arguments");
  WAE_REQUIRE(!gid || n_speakers > 0, "gproj_bwd_det: speaker ids need the size of the embedding table");
  WAE_REQUIRE(Hp >= G / 2 && ones_col >= 0 && ld >= (int64_t)ones_col + B && c_layer_stride >= (int64_t)2 * Hp * ld,
              "gproj_bwd_det: the %d per-clip columns at %d do not fit rows of %lld floats (layer stride %lld)", B, ones_col,
              (long long)ld, (long long)c_layer_stride);
  const int64_t wg = (gid || gvec) ? wg_off : -1;
  const bool emb = gid && wg >= 0 && Cg > 0;
  WAE_REQUIRE(!emb || (parts && parts_floats >= wae_gproj_bwd_det_floats(B, L, Hp, Cg)),
              "gproj_bwd_det: the partials buffer is smaller than wae_gproj_bwd_det_floats says");
  const size_t lds = (32 * ACC_BMAX + (size_t)ACC_BMAX * (Cg > 0 ? Cg : 0)) * sizeof(float);
  WAE_REQUIRE(lds <= 64 * 1024, "gproj_bwd_det: Cg = %d too wide for the staged form", Cg);
  const int nblk = (2 * Hp + 31) / 32;
  for (int b0 = 0; b0 < B; b0 += ACC_BMAX) {
    if (consume)
      hipLaunchKernelGGL(gproj_bwd_det_kernel<true>, dim3(L, nblk), dim3(256), lds, as_stream(stream), eff, d_eff, wg, bias_off,
                         layer_stride, gid, emb_off, gvec, c1, c_layer_stride, ld, ones_col, b0, B, G, Hp, Cg, n_speakers, parts);
    else
      hipLaunchKernelGGL(gproj_bwd_det_kernel<false>, dim3(L, nblk), dim3(256), lds, as_stream(stream), eff, d_eff, wg, bias_off,
                         layer_stride, gid, emb_off, gvec, c1, c_layer_stride, ld, ones_col, b0, B, G, Hp, Cg, n_speakers, parts);
  }
  if (emb)
    hipLaunchKernelGGL(gproj_emb_finish_kernel, dim3((B * Cg + 255) / 256), dim3(256), 0, as_stream(stream), (const float*)parts, gid,
                       d_eff, emb_off, B, L, nblk, Cg, n_speakers);
  return wae_check_launch("gproj_bwd_det");
}

// ---- the window's statistics -------------------------------------------------------------------------------------------------
// sums (3 doubles): [0] = sum ce_weight_i * ce_i, [1] = sum vq_weight_i * vq_loss_i, [2] = micro-batches; counts (K int32): the code
// histograms added per code.  One workgroup; thread 0 alone touches the doubles, thread j the codes j, j + 256, ...
__global__ void __launch_bounds__(256) accum_stats_add_kernel(double* __restrict__ sums, int32_t* __restrict__ counts, int K,
                                                              const float* __restrict__ ce, double ce_weight,
                                                              const float* __restrict__ vq_loss, double vq_weight,
                                                              const int32_t* __restrict__ hist) {
  if (counts && hist)
    for (int k = threadIdx.x; k < K; k += 256) counts[k] += hist[k];
  if (threadIdx.x == 0) {
    if (ce) sums[0] += ce_weight * (double)ce[0];
    if (vq_loss) sums[1] += vq_weight * (double)vq_loss[0];
    sums[2] += 1.0;
  }
}

// out (5 floats): ce, vq_loss, ce + vq_loss, perplexity of the added counts with N = their sum (vq_perplexity: the arithmetic of the
// dense search's statistics and of wae_vq_stats_segments; 0 without counts), micro-batches
__global__ void __launch_bounds__(256) accum_stats_close_kernel(const double* __restrict__ sums, const int32_t* __restrict__ counts, int K,
                                                                float* __restrict__ out) {
  __shared__ float part[4];
  __shared__ int s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  int n = 0;
  if (counts)
    for (int k = threadIdx.x; k < K; k += 256) n += counts[k];
  if (n) atomicAdd(&s_n, n);                 // integers: any order gives the same sum
  __syncthreads();
  const int N = s_n;
  const float perp = vq_perplexity(counts, K, (float)N, part, counts != nullptr && N > 0);
  if (threadIdx.x == 0) {
    out[0] = (float)sums[0];
    out[1] = (float)sums[1];
    out[2] = (float)(sums[0] + sums[1]);
    out[3] = (counts && N > 0) ? perp : 0.f;
    out[4] = (float)sums[2];
  }
}

extern "C" int wae_accum_stats(double* sums, int32_t* counts, int32_t K, const float* ce, double ce_weight, const float* vq_loss,
                               double vq_weight, const int32_t* hist, float* out, void* stream) {
  WAE_REQUIRE(sums && K >= 0 && (!counts || K > 0), "accum_stats: bad arguments");
  if (out)
    hipLaunchKernelGGL(accum_stats_close_kernel, dim3(1), dim3(256), 0, as_stream(stream), sums, counts, K, out);
  else
    hipLaunchKernelGGL(accum_stats_add_kernel, dim3(1), dim3(256), 0, as_stream(stream), sums, counts, K, ce, ce_weight, vq_loss,
                       vq_weight, hist);
  return wae_check_launch("accum_stats");
}
