// The end of a train step's backward in one pass: packed weight-gradient tiles -> gradients of weight_g / weight_v and of the plain
// parameters in the reference layout, and the sum of their squares for the gradient clip.
//
// Before, the same values took four passes: scatter_multi_kernel added the tiles into d_eff (4-byte read-modify-writes a weight row
// apart, ~1 TB/s of useful bytes), weight_norm_bwd_kernel read d_eff and wrote grads, grad_sqnorm_kernel read grads again.  Here a row
// of the arena has ONE owner -- the 16-lane group of weight_norm_bwd_kernel (csrc/misc.hip) -- that GATHERS its dW from the tiles
// through an inverse map instead of waiting for a scatter: a row's slots are `base + pattern[i]` in the tile buffer, where the pattern
// (the row's slots relative to its first) is shared by every row of a tensor and every layer, so the map of C2's 10 M slots is a few
// KiB that stay in cache.  A group's gathers cover whole runs of the tile rows they touch (a convolution row reads k runs of R floats,
// a transposed dW_out row one float of every tile row, 16 neighbouring rows per workgroup), so the tile bytes are fetched once.
// The arithmetic of a row -- load order, the 16-lane butterfly, the formula -- is weight_norm_bwd_kernel's, statement for statement:
// grads are bit for bit what the three launches gave (tests/test_gpu_grad_finish.py).
//
// Rows whose dW other kernels leave in d_eff (conv1x1g and the conv bias from gproj_bwd, bias sums of the row-sum scatter) have no
// pattern (pat < 0) and read d_eff; plain parameters (g_off < 0) are passed through.  Every workgroup adds the squares of what it
// wrote -- fp32 products accumulated in double, as grad_sqnorm_kernel does -- with one fp64 atomic.
#include "wae_common.hpp"

#define GF_KMAX 16   // = WN_KMAX of csrc/misc.hip: rows of up to 1024 floats take the vector path
typedef __attribute__((ext_vector_type(4))) int i32x4;

__device__ __forceinline__ float gf_dot(const f32x4& a, const f32x4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float gf_group_sum(float x) {   // over the 16 lanes of a group
  x += __shfl_xor(x, 1);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 8);
  return x;
}
__device__ __forceinline__ double gf_sq(const f32x4& v) {
  return (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
}

__global__ void __launch_bounds__(256) grad_finish_kernel(const float* __restrict__ params, const float* __restrict__ tiles,
                                                          const int32_t* __restrict__ pats, const float* __restrict__ d_eff,
                                                          float* __restrict__ grads, const wae_finish_row* __restrict__ rows,
                                                          int nrows, double* __restrict__ acc) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int l = threadIdx.x & 15;
  double sq = 0.0;
  if (row < nrows) {
    const wae_finish_row r = rows[row];
    const int n = r.cols;
    const float* v = params + r.off;
    float* gv = grads + r.off;
    const int32_t* pt = r.pat >= 0 ? pats + r.pat : nullptr;      // (16-byte aligned: the host pads every pattern to four entries)
    const float* dw = pt ? tiles + r.base : d_eff + r.off;
    if (r.g_off < 0) {
      // a plain parameter: passed through, four loads in flight per lane (the host cuts plain runs into rows of 64 floats: one trip)
      for (int i0 = l; i0 < n; i0 += 64) {
        float x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + 16 * u;
          x[u] = i < n ? dw[pt ? pt[i] : i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + 16 * u;
          if (i < n) gv[i] = x[u];
          sq += (double)x[u] * x[u];
        }
      }
    } else {
      const float g = params[r.g_off];
      const bool vec = n >= 4 && n <= 64 * GF_KMAX && (n & 3) == 0 && (r.off & 3) == 0;   // wn_vec_ok of csrc/misc.hip
      if (vec) {
        f32x4 rv[GF_KMAX], rd[GF_KMAX];
#pragma unroll
        for (int k = 0; k < GF_KMAX; ++k)
          if (k * 64 < n) {
            const int i = min((l + 16 * k) * 4, n - 4);
            rv[k] = *(const f32x4*)(v + i);
            if (pt) {
              const i32x4 p = *(const i32x4*)(pt + i);
              rd[k].x = dw[p.x];
              rd[k].y = dw[p.y];
              rd[k].z = dw[p.z];
              rd[k].w = dw[p.w];
            } else {
              rd[k] = *(const f32x4*)(dw + i);
            }
          }
        float ss = 0.f, dv = 0.f;
#pragma unroll
        for (int k = 0; k < GF_KMAX; ++k)
          if (k * 64 < n) {
            const bool on = (l + 16 * k) * 4 < n;
            ss += on ? gf_dot(rv[k], rv[k]) : 0.f;
            dv += on ? gf_dot(rv[k], rd[k]) : 0.f;
          }
        ss = gf_group_sum(ss);
        dv = gf_group_sum(dv);
        const float inv = 1.0f / sqrtf(ss);
        const float gi = g * inv, c2 = dv * inv * inv;
#pragma unroll
        for (int k = 0; k < GF_KMAX; ++k)
          if ((l + 16 * k) * 4 < n) {
            const f32x4 o = (rd[k] - rv[k] * c2) * gi;
            *(f32x4*)(gv + (l + 16 * k) * 4) = o;
            sq += gf_sq(o);
          }
        if (l == 0) {
          const float dg = dv * inv;
          grads[r.g_off] = dg;
          sq += (double)dg * dg;
        }
      } else {
        float ss = 0.f, dv = 0.f;
        for (int i = l; i < n; i += 16) {
          ss += v[i] * v[i];
          dv += v[i] * dw[pt ? pt[i] : i];
        }
        ss = gf_group_sum(ss);
        dv = gf_group_sum(dv);
        const float inv = 1.0f / sqrtf(ss);
        for (int i = l; i < n; i += 16) {
          const float o = g * inv * (dw[pt ? pt[i] : i] - v[i] * dv * inv * inv);
          gv[i] = o;
          sq += (double)o * o;
        }
        if (l == 0) {
          const float dg = dv * inv;
          grads[r.g_off] = dg;
          sq += (double)dg * dg;
        }
      }
    }
  }
  if (acc == nullptr) return;       // (uniform over the launch)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
}

extern "C" int wae_grad_finish(const float* params, const float* tiles, const int32_t* pats, const float* d_eff, float* grads,
                               const wae_finish_row* rows, int32_t row_lo, int32_t row_hi, double* sqnorm_acc, void* stream) {
  WAE_REQUIRE(params && tiles && pats && d_eff && grads && rows, "grad_finish: null argument");
  WAE_REQUIRE(row_lo >= 0 && row_hi >= row_lo, "grad_finish: bad row range");
  const int nrows = row_hi - row_lo;
  if (nrows == 0) return WAE_OK;
  hipLaunchKernelGGL(grad_finish_kernel, dim3((nrows + 15) / 16), dim3(256), 0, as_stream(stream), params, tiles, pats, d_eff, grads,
                     rows + row_lo, nrows, sqnorm_acc);
  return wae_check_launch("grad_finish");
}
