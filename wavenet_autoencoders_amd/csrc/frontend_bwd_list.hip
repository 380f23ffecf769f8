// Backward of the low-rate front end over a LIST of utterances of unequal lengths (include/wae.h: wae_from_btc_list,
// wae_upsample_stage_bwd_list, wae_enc_conv_bwd_list) -- the list forms of csrc/frontend_bwd.hip, on the packed layout and the tables
// of their forward twins (csrc/ups_list.hip, csrc/enc_list.hip): an activation of the list is channel-major and packed along time,
// item i owning the columns [off_i, off_i + T_i) of a (C, pitch) fp32 array.  Every item is zero-padded at its own two ends: a tap
// outside the item contributes nothing and never reads the neighbour's column.  Plain fp32 VALU kernels, as the dense ones; the
// gradients they form are those of csrc/frontend_bwd.hip for every item as a batch of one, the weight gradients summed over the items.
// The kernels do not trust a table with memory: a record that does not fit its pitches, or contradicts the length formula, retires
// its workgroups (or is passed over by the weight gradient's owner) in front of every access.
#include "wae_common.hpp"

__device__ __forceinline__ float wave_sum_list(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The record of tile `bid` and the tile's index k inside its item (csrc/ups_list.hip: ups_find, with the bound of out_off
// handed in): false = the workgroup retires.  Uniform over the workgroup.
__device__ __forceinline__ bool upl_find(const wae_ups_seg* __restrict__ segs, int nsegs, int bid, int tile, int mul, int in_pitch,
                                         int out_bound, wae_ups_seg& seg, int& k, int& Tout) {
  int lo = 0, hi = nsegs - 1;
  while (lo < hi) {                      // the last record with tile0 <= bid
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].tile0 <= bid) lo = mid;
    else hi = mid - 1;
  }
  seg = segs[lo];
  const int next = segs[lo + 1].tile0;   // (the closing record for the last item)
  k = bid - seg.tile0;
  const int64_t To = (int64_t)seg.Tin * mul;
  if (seg.Tin < 1 || k < 0 || bid >= next || To >= (int64_t)1 << 31) return false;
  if ((int64_t)next - seg.tile0 != (To + tile - 1) / tile) return false;
  if (seg.in_off < 0 || (int64_t)seg.in_off + seg.Tin > in_pitch || seg.out_off < 0 || (int64_t)seg.out_off + To > out_bound) return false;
  Tout = (int)To;
  return true;
}

// ---- (rows, Cp) dtype -> (C, pitch) fp32, times scale: the inverse of to_btc_list_kernel, 64 rows of one item x 64 channels per block
template <typename E>
__global__ void __launch_bounds__(256) from_btc_list_kernel(const void* __restrict__ in, float* __restrict__ out,
                                                            const wae_ups_seg* __restrict__ segs, int nsegs, int pitch, int rows, int C,
                                                            int Cp, float scale) {
  __shared__ float tile[64][65];
  wae_ups_seg seg;
  int k, T;
  if (!upl_find(segs, nsegs, blockIdx.x, 64, 1, pitch, rows, seg, k, T)) return;
  const int t0 = k * 64, c0 = blockIdx.y * 64;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  for (int i = ly; i < 64; i += 4) {
    const int t = t0 + i, c = c0 + lx;
    tile[i][lx] = (t < T && c < C) ? (float)((const E*)in)[((int64_t)seg.out_off + t) * Cp + c] : 0.f;
  }
  __syncthreads();
  for (int i = ly; i < 64; i += 4) {
    const int c = c0 + i, t = t0 + lx;
    if (c < C && t < T) out[(int64_t)c * pitch + seg.in_off + t] = tile[lx][i] * scale;
  }
}

extern "C" int wae_from_btc_list(const void* in, float* out, const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t pitch,
                                 int32_t rows, int32_t C, int32_t Cp, int32_t dtype, float scale, void* stream) {
  WAE_REQUIRE(in && out && C > 0, "from_btc_list: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "from_btc_list: a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0 && pitch > 0 && rows > 0, "from_btc_list: ntiles, pitch and rows must be > 0 (got %d, %d, %d)", ntiles, pitch, rows);
  WAE_REQUIRE(Cp >= C, "from_btc_list: Cp %d < C %d", Cp, C);
  WAE_REQUIRE(wae_dtype_ok(dtype), "from_btc_list: bad dtype %d", dtype);
  if ((C + 63) / 64 > 65535) {
    wae_set_error("from_btc_list: C %d has no list kernel; run wae_from_btc_scaled per item", C);
    return WAE_EUNSUPPORTED;
  }
  const dim3 grid(ntiles, (C + 63) / 64);
  hipStream_t st = as_stream(stream);
  if (dtype == WAE_BF16) hipLaunchKernelGGL(from_btc_list_kernel<__bf16>, grid, dim3(256), 0, st, in, out, segs, nsegs, pitch, rows, C, Cp, scale);
  else if (dtype == WAE_F16) hipLaunchKernelGGL(from_btc_list_kernel<f16>, grid, dim3(256), 0, st, in, out, segs, nsegs, pitch, rows, C, Cp, scale);
  else hipLaunchKernelGGL(from_btc_list_kernel<float>, grid, dim3(256), 0, st, in, out, segs, nsegs, pitch, rows, C, Cp, scale);
  return wae_check_launch("from_btc_list");
}

// ---- upsample stage ------------------------------------------------------------------------------------------------------------
// A workgroup is one tile of the forward twin's table: WAE_UPS_LIST_TILE_CT output columns [k 256, (k+1) 256) of one item.  It owns
// the input frames q whose first output column q s lies in the tile -- [ceil(k 256 / s), ceil((k+1) 256 / s)) below Tin_i: every frame
// of the item belongs to exactly one tile, at most ceil(256 / s) of them -- and forms, for every channel,
//   din[q]  = sum_{d in [0, 3s)} coef[d] dout[q s - s + d]  (columns inside [0, Tout_i)),  coef as csrc/frontend_bwd.hip forms it;
//   dw[j]  += sum_r A[r][(r + j) / s],  A[r][o] = sum_q dout[q s + r] in[q - 1 + o]  (in[-1] = in[Tin_i] = 0: the item's own padding).
// Thread = (frame, channel lane): F = ceil(256 / s) frames by 256 / F channel lanes, a lane walking the channels c = lane,
// lane + 256 / F, ...  A workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (at most UPLB_MAXWG workgroups) and keeps its
// correlations across them: the tap sums leave as ONE float atomic per tap and workgroup, however many tiles the list has (the dense
// kernel's bound on the atomics that meet on the 2s+1 addresses; at 32 utterances of hps/vqwae.json it changed no step time).
// DET (wae_upsample_stage_bwd_list_det): the workgroup leaves its 2s+1 sums in parts[blockIdx.x][tap] with plain stores instead (every
// workgroup of the launch stores every tap once, a workgroup whose tiles were all refused its zeros: no clearing); a second launch adds
// the workgroups' sums in index order (ups_list_w_finish_kernel).  The DET launch hands `parts` in as the kernel's dw argument: one
// argument list for both instantiations.
#define UPLB_MAXWG 512
#define UPLB_MAXTAPS 33
#define UPLB_MAXS 16
template <int S, bool DET = false>
__global__ void __launch_bounds__(256) ups_stage_bwd_list_kernel(const float* __restrict__ dout, const float* __restrict__ in,
                                                                 const float* __restrict__ w, float* __restrict__ din,
                                                                 float* __restrict__ dw, const wae_ups_seg* __restrict__ segs, int nsegs,
                                                                 int ntiles, int in_pitch, int out_pitch, int C, int s_rt) {
  const int s = S > 0 ? S : s_rt;
  constexpr int NA = S > 0 ? S : UPLB_MAXS;
  __shared__ float coef[3 * UPLB_MAXS];
  __shared__ float part[4][UPLB_MAXTAPS];
  if ((int)threadIdx.x < 3 * s) {
    const int d = (int)threadIdx.x - s;
    float a = 0.f;
    for (int j = max(0, s - d); j <= min(2 * s, 2 * s - 1 - d); ++j) a += w[j];
    coef[threadIdx.x] = a;
  }
  __syncthreads();
  const int ntap = 2 * s + 1;
  const int F = (WAE_UPS_LIST_TILE_CT + s - 1) / s, G = 256 / F;
  const int f = threadIdx.x % F, lane = threadIdx.x / F;
  float A[NA][3];
#pragma unroll
  for (int r = 0; r < NA; ++r) A[r][0] = A[r][1] = A[r][2] = 0.f;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {      // (no barrier inside: a refused record passes the tile over)
    wae_ups_seg seg;
    int k, Tout;
    if (!upl_find(segs, nsegs, tile, WAE_UPS_LIST_TILE_CT, s, in_pitch, out_pitch, seg, k, Tout)) continue;
    const int Tin = seg.Tin;
    const int q_lo = (int)(((int64_t)k * WAE_UPS_LIST_TILE_CT + s - 1) / s);
    const int q_hi = (int)min((int64_t)Tin, ((int64_t)(k + 1) * WAE_UPS_LIST_TILE_CT + s - 1) / s);
    const int q = q_lo + f;
    const bool live = lane < G && q < q_hi;
    if (live) {
      for (int c = lane; c < C; c += G) {
        const float* dr = dout + (int64_t)c * out_pitch + seg.out_off;
        const float* ir = in + (int64_t)c * in_pitch + seg.in_off;
        float acc = 0.f;
        const int tb = q * s - s;
        for (int d = 0; d < 3 * s; ++d) {
          const int t = tb + d;
          if (t >= 0 && t < Tout) acc = fmaf(coef[d], dr[t], acc);
        }
        din[(int64_t)c * in_pitch + seg.in_off + q] = acc;
        const float i0 = q >= 1 ? ir[q - 1] : 0.f, i1 = ir[q], i2 = q + 1 < Tin ? ir[q + 1] : 0.f;
#pragma unroll
        for (int r = 0; r < NA; ++r)
          if (r < s) {
            const float g = dr[q * s + r];
            A[r][0] = fmaf(g, i0, A[r][0]);
            A[r][1] = fmaf(g, i1, A[r][1]);
            A[r][2] = fmaf(g, i2, A[r][2]);
          }
      }
    }
  }
  // dw[j] = sum_r A[r][(r + j) / s]: every index is known once the loops are unrolled (S > 0) or selected without a dynamic index
#pragma unroll
  for (int j = 0; j < 2 * NA + 1; ++j) {
    float v = 0.f;
#pragma unroll
    for (int r = 0; r < NA; ++r) {
      const int o = S > 0 ? (r + j) / NA : (r + j) / s;
      const float a = o == 0 ? A[r][0] : (o == 1 ? A[r][1] : A[r][2]);
      if (r < s && j < ntap) v += a;
    }
    if (j < ntap) {           // (uniform: every wave takes part in the butterfly)
      v = wave_sum_list(v);
      if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][j] = v;
    }
  }
  __syncthreads();
  if constexpr (DET) {
    if ((int)threadIdx.x < ntap)
      dw[blockIdx.x * UPLB_MAXTAPS + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
  } else {
    if ((int)threadIdx.x < ntap)
      atomicAdd(dw + threadIdx.x, part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
  }
}

extern "C" int wae_upsample_stage_bwd_list(const float* dout, const float* in, const float* w, float* din, float* dw,
                                           const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t in_pitch, int32_t out_pitch,
                                           int32_t C, int32_t s, void* stream) {
  WAE_REQUIRE(dout && in && w && din && dw && C > 0 && s > 0, "upsample_stage_bwd_list: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "upsample_stage_bwd_list: a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0, "upsample_stage_bwd_list: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "upsample_stage_bwd_list: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(s <= UPLB_MAXS, "upsample_stage_bwd_list: scale %d > %d is not supported", s, UPLB_MAXS);
  hipStream_t st = as_stream(stream);
  const dim3 grid(ntiles < UPLB_MAXWG ? ntiles : UPLB_MAXWG);
#define WAE_UPLB(S_) hipLaunchKernelGGL(ups_stage_bwd_list_kernel<S_>, grid, dim3(256), 0, st, dout, in, w, din, dw, segs, nsegs, ntiles, in_pitch, out_pitch, C, s)
  if (s == 4) WAE_UPLB(4);
  else if (s == 5) WAE_UPLB(5);
  else if (s == 8) WAE_UPLB(8);
  else if (s == 16) WAE_UPLB(16);
  else WAE_UPLB(0);
#undef WAE_UPLB
  return wae_check_launch("upsample_stage_bwd_list");
}

// The fixed-order form of the stage's backward: the same kernel with its tap sums stored to parts[workgroup][tap], and one small launch
// of one workgroup, thread = tap, that adds parts[0 .. nwg-1][tap] in index order from zero and then dw[tap] = dw[tap] + sum with one
// plain read-modify-write.  nwg <= UPLB_MAXWG rows of UPLB_MAXTAPS floats (66 KB) do not fit LDS whole: they pass through it in
// rounds of UPLBF_ROWS rows, coalesced (one thread per tap walking global memory would wait out a load per workgroup).
#define UPLBF_ROWS 128
__global__ void __launch_bounds__(256) ups_list_w_finish_kernel(const float* __restrict__ parts, int nwg, int ntap, float* __restrict__ dw) {
  __shared__ float sp[UPLBF_ROWS * UPLB_MAXTAPS];
  float v = 0.f;
  for (int r0 = 0; r0 < nwg; r0 += UPLBF_ROWS) {
    const int nr = min(UPLBF_ROWS, nwg - r0);
    __syncthreads();
    for (int i = threadIdx.x; i < nr * UPLB_MAXTAPS; i += 256) sp[i] = parts[(int64_t)r0 * UPLB_MAXTAPS + i];
    __syncthreads();
    if ((int)threadIdx.x < ntap)
      for (int i = 0; i < nr; ++i) v += sp[i * UPLB_MAXTAPS + threadIdx.x];
  }
  if ((int)threadIdx.x < ntap) dw[threadIdx.x] = dw[threadIdx.x] + v;
}
extern "C" int64_t wae_upsample_stage_bwd_list_det_floats(void) { return (int64_t)UPLB_MAXWG * UPLB_MAXTAPS; }
extern "C" int wae_upsample_stage_bwd_list_det(const float* dout, const float* in, const float* w, float* din, float* dw,
                                               const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t in_pitch,
                                               int32_t out_pitch, int32_t C, int32_t s, float* parts, int64_t parts_floats, void* stream) {
  WAE_REQUIRE(dout && in && w && din && dw && C > 0 && s > 0, "upsample_stage_bwd_list_det: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "upsample_stage_bwd_list_det: a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0, "upsample_stage_bwd_list_det: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "upsample_stage_bwd_list_det: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(s <= UPLB_MAXS, "upsample_stage_bwd_list_det: scale %d > %d is not supported", s, UPLB_MAXS);
  WAE_REQUIRE(parts && parts_floats >= (int64_t)UPLB_MAXWG * UPLB_MAXTAPS,
              "upsample_stage_bwd_list_det: the partials buffer is smaller than wae_upsample_stage_bwd_list_det_floats says");
  hipStream_t st = as_stream(stream);
  const int nwg = ntiles < UPLB_MAXWG ? ntiles : UPLB_MAXWG;
  const dim3 grid(nwg);
#define WAE_UPLB(S_) hipLaunchKernelGGL((ups_stage_bwd_list_kernel<S_, true>), grid, dim3(256), 0, st, dout, in, w, din, parts, segs, nsegs, ntiles, in_pitch, out_pitch, C, s)
  if (s == 4) WAE_UPLB(4);
  else if (s == 5) WAE_UPLB(5);
  else if (s == 8) WAE_UPLB(8);
  else if (s == 16) WAE_UPLB(16);
  else WAE_UPLB(0);
#undef WAE_UPLB
  hipLaunchKernelGGL(ups_list_w_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)parts, nwg, 2 * s + 1, dw);
  return wae_check_launch("upsample_stage_bwd_list_det");
}

// ---- Conv1d (+ReLU) (+residual) ------------------------------------------------------------------------------------------------
// dpre = dy * [relu ? (y - (residual ? x : 0)) > 0 : 1], as csrc/frontend_bwd.hip forms it; x (Cin, in_pitch), y / dy (Cout, out_pitch).
// One launch, a flat grid: the first ntiles * ceil(Cin / 32) workgroups form dx (absent where dx is NULL), the rest own the weight
// gradient.
#define ECL_T 32      // channels per block, both parts
#define ECL_CH 64     // output channels whose dpre window the input gradient stages per round
#define ECL_RT 4      // tiles staged per round of the weight gradient

struct EclTile {      // a validated tile: the item's columns, its lengths, the tile's first output
  int in_off, out_off, Tin, Tout, to0, ok;
};
template <int K, int S>
__device__ __forceinline__ EclTile ecl_tile(const wae_seg* __restrict__ segs, int nsegs, const int32_t* __restrict__ tiles, int t,
                                            int in_pitch, int out_pitch, int pad) {
  EclTile r = {0, 0, 0, 0, 0, 0};
  const int sg = tiles[2 * t];
  r.to0 = tiles[2 * t + 1];
  if (sg < 0 || sg >= nsegs) return r;
  const wae_seg seg = segs[sg];
  if (seg.Tin < 1 || seg.in_off < 0 || (int64_t)seg.in_off + seg.Tin > in_pitch || seg.out_off < 0 ||
      (int64_t)seg.out_off + seg.Tout > out_pitch || (int64_t)seg.Tin + 2 * pad < K ||
      seg.Tout != (int)(((int64_t)seg.Tin + 2 * pad - K) / S + 1) || r.to0 < 0 || r.to0 >= seg.Tout)
    return r;
  r.in_off = seg.in_off, r.out_off = seg.out_off, r.Tin = seg.Tin, r.Tout = seg.Tout, r.ok = 1;
  return r;
}
__device__ __forceinline__ float ecl_dpre(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                          int64_t yi, int64_t xi, int relu, int residual) {
  float g = dy[yi];
  if (relu) {
    const float act = residual ? y[yi] - x[xi] : y[yi];
    if (!(act > 0.f)) g = 0.f;
  }
  return g;
}

// dx[ci][ti] = sum_{co, j} w[co][ci][j] dpre[co][(ti + pad - j) / S] over the whole steps inside [0, Tout_i) (+ dy[ci][ti], residual).
// The tile (item, to0) of the forward's table owns the item's input steps [to0 S, (to0 + ET) S), the item's last tile everything up to
// Tin_i: the tiles of an item start at multiples of ET and cover [0, Tout_i), so these ranges cover [0, Tin_i) once.  Block = 32 input
// channels of one tile; thread = (channel, one step in 8); dpre windows of ECL_CH output channels go through LDS.
template <int K, int S, int ET>
__device__ __forceinline__ void ecl_dx_body(float* __restrict__ sm, const float* __restrict__ x, const float* __restrict__ w,
                                            const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                            const wae_seg* __restrict__ segs, int nsegs, const int32_t* __restrict__ tiles, int in_pitch,
                                            int out_pitch, int Cin, int Cout, int pad, int relu, int residual, int tile, int cblk) {
  constexpr int NI = ET * S + K - 1;            // the most input steps of a tile: (ET - 1) S + K + S - 1 - 2 pad for an item's last one
  constexpr int MAXI = (NI + 7) / 8;
  constexpr int TW = ET + 2 * K + 2;            // the most output steps they reach
  const EclTile tl = ecl_tile<K, S>(segs, nsegs, tiles, tile, in_pitch, out_pitch, pad);
  if (!tl.ok) return;
  const int ti0 = tl.to0 * S;
  const int ti1 = tl.to0 + ET >= tl.Tout ? tl.Tin : min(tl.Tin, (tl.to0 + ET) * S);
  if (ti0 >= ti1 || ti1 - ti0 > NI) return;     // (a tile that is no multiple of ET into its item: nothing of it is ours)
  const int to_lo = max(ti0 + pad - (K - 1), 0) / S, to_hi = min((ti1 - 1 + pad) / S, tl.Tout - 1);
  const int nto = to_hi - to_lo + 1;
  if (nto > TW) return;
  const int col = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int ci = cblk * ECL_T + col;
  float acc[MAXI];
#pragma unroll
  for (int i = 0; i < MAXI; ++i) acc[i] = 0.f;
  const float* xb = x + tl.in_off;
  const float* yb = y ? y + tl.out_off : nullptr;
  const float* dyb = dy + tl.out_off;
  for (int c0 = 0; c0 < Cout; c0 += ECL_CH) {
    const int nc = min(ECL_CH, Cout - c0);
    __syncthreads();
    for (int i = threadIdx.x; i < nc * nto; i += 256) {
      const int co = i / nto, tw = i - co * nto, to = to_lo + tw;
      sm[co * TW + tw] = ecl_dpre(dyb, yb, xb, (int64_t)(c0 + co) * out_pitch + to, (int64_t)(c0 + co) * in_pitch + to, relu, residual);
    }
    __syncthreads();
    if (ci < Cin)
      for (int co = 0; co < nc; ++co) {
        float wv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) wv[j] = w[((int64_t)(c0 + co) * Cin + ci) * K + j];
        const float* gr = sm + co * TW - to_lo;
#pragma unroll
        for (int i = 0; i < MAXI; ++i) {
          const int ti = ti0 + sub + 8 * i;
          if (ti < ti1)
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const int num = ti + pad - j;
              if (num >= 0 && num % S == 0 && num / S <= to_hi) acc[i] = fmaf(wv[j], gr[num / S], acc[i]);
            }
        }
      }
  }
  if (ci < Cin)
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int ti = ti0 + sub + 8 * i;
      if (ti < ti1) {
        float v = acc[i];
        if (residual) v += dyb[(int64_t)ci * out_pitch + ti];
        dx[(int64_t)ci * in_pitch + tl.in_off + ti] = v;
      }
    }
}

// dw[co][ci][j] += sum over the tiles of the table, in table order, of sum_to dpre[co][to] x[ci][to S + j - pad] (+ dbias[co] += sum dpre):
// block = 32 output x 32 input channels over every tile, the only owner of its outputs (a plain read-modify-write at the end); thread =
// (co, 4 input channels); ECL_RT tiles are staged per round -- the dpre tile [32 co][ET] and the x window [32 ci][(ET - 1) S + K], zeros
// outside the item.  A tile whose record is refused contributes nothing.  The arithmetic per staged tile is conv_bwd_w_tiled_body's.
template <int K, int S, int ET>
__device__ __forceinline__ void ecl_dw_body(float* __restrict__ sm, const float* __restrict__ x, const float* __restrict__ y,
                                            const float* __restrict__ dy, float* __restrict__ dw, float* __restrict__ dbias,
                                            const wae_seg* __restrict__ segs, int nsegs, const int32_t* __restrict__ tiles, int ntiles,
                                            int in_pitch, int out_pitch, int Cin, int Cout, int pad, int relu, int residual, int bx, int by) {
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3, GP = ET + 4;
  constexpr int GSZ = ECL_T * GP, XSZ = ECL_T * WP;
  __shared__ EclTile meta[ECL_RT];
  const int co0 = bx * ECL_T, ci0 = by * ECL_T;
  const int col = threadIdx.x & 31, cg = threadIdx.x >> 5;
  float acc[4][K];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int j = 0; j < K; ++j) acc[c][j] = 0.f;
  float accb = 0.f;
  for (int r0 = 0; r0 < ntiles; r0 += ECL_RT) {
    const int nr = min(ECL_RT, ntiles - r0);
    __syncthreads();
    if ((int)threadIdx.x < nr) meta[threadIdx.x] = ecl_tile<K, S>(segs, nsegs, tiles, r0 + threadIdx.x, in_pitch, out_pitch, pad);
    __syncthreads();
    for (int i = threadIdx.x; i < nr * ECL_T * ET; i += 256) {
      const int r = i / (ECL_T * ET), e = i - r * (ECL_T * ET);
      const int tl = e % ET, cl = e / ET;
      const EclTile m = meta[r];
      const int to = m.to0 + tl, co = co0 + cl;
      sm[r * (GSZ + XSZ) + cl * GP + tl] =
          (m.ok && co < Cout && to < m.Tout)
              ? ecl_dpre(dy + m.out_off, y ? y + m.out_off : nullptr, x + m.in_off, (int64_t)co * out_pitch + to, (int64_t)co * in_pitch + to,
                         relu, residual)
              : 0.f;
    }
    for (int i = threadIdx.x; i < nr * XSZ; i += 256) {
      const int r = i / XSZ, e = i - r * XSZ;
      const int cl = e / WP, wv = e - cl * WP;
      const EclTile m = meta[r];
      const int ci = ci0 + cl;
      const int64_t ti = (int64_t)m.to0 * S - pad + wv;
      sm[r * (GSZ + XSZ) + GSZ + e] = (m.ok && wv < WIN && ci < Cin && ti >= 0 && ti < m.Tin) ? x[(int64_t)ci * in_pitch + m.in_off + ti] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
      const float* gs = sm + r * (GSZ + XSZ);
      const float* xs = gs + GSZ;
      float g[ET];
#pragma unroll
      for (int q = 0; q < ET / 4; ++q) {
        const f32x4 v = *(const f32x4*)(gs + col * GP + 4 * q);
        g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
        accb += (v.x + v.y) + (v.z + v.w);
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4* xr4 = (const f32x4*)(xs + (cg * 4 + c) * WP);
        float xw[WP];
#pragma unroll
        for (int q = 0; q < WP / 4; ++q) {
          const f32x4 v = xr4[q];
          xw[4 * q] = v.x; xw[4 * q + 1] = v.y; xw[4 * q + 2] = v.z; xw[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
          for (int t = 0; t < ET; ++t) acc[c][j] = fmaf(g[t], xw[t * S + j], acc[c][j]);
      }
    }
  }
  const int co = co0 + col;
  if (co < Cout) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int ci = ci0 + cg * 4 + c;
      if (ci < Cin)
#pragma unroll
        for (int j = 0; j < K; ++j) dw[((int64_t)co * Cin + ci) * K + j] += acc[c][j];
    }
    if (dbias && cg == 0 && by == 0) dbias[co] += accb;
  }
}

template <int K, int S, int ET>
struct EclLds {
  static constexpr int WIN = (ET - 1) * S + K;
  static constexpr int WP = (WIN + 3) & ~3;
  static constexpr int DW = ECL_RT * (ECL_T * (ET + 4) + ECL_T * WP);
  static constexpr int DX = ECL_CH * (ET + 2 * K + 2);
  static constexpr int N = DW > DX ? DW : DX;
};
static_assert(EclLds<5, 2, 32>::N * sizeof(float) <= 60 * 1024, "the staging of the largest instantiation fits static LDS");

template <int K, int S, int ET>
__global__ void __launch_bounds__(256) enc_conv_bwd_list_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ y, const float* __restrict__ dy,
                                                                float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ dbias,
                                                                const wae_seg* __restrict__ segs, int nsegs,
                                                                const int32_t* __restrict__ tiles, int ntiles, int in_pitch, int out_pitch,
                                                                int Cin, int Cout, int pad, int relu, int residual, int nx, int nwx) {
  __shared__ __attribute__((aligned(16))) float sm[EclLds<K, S, ET>::N];
  const int id = blockIdx.x;
  if (id < nx) {
    ecl_dx_body<K, S, ET>(sm, x, w, y, dy, dx, segs, nsegs, tiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual, id % ntiles,
                          id / ntiles);
  } else {
    const int iw = id - nx;
    ecl_dw_body<K, S, ET>(sm, x, y, dy, dw, dbias, segs, nsegs, tiles, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual,
                          iw % nwx, iw / nwx);
  }
}

struct EclArgs {
  const float *x, *w, *y, *dy;
  float *dx, *dw, *dbias;
  const wae_seg* segs;
  const int32_t* tiles;
  int nsegs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual;
};
template <int K, int S, int ET>
static void launch_ecl_et(const EclArgs& a, hipStream_t st) {
  const int ncb = (a.Cin + ECL_T - 1) / ECL_T, nwx = (a.Cout + ECL_T - 1) / ECL_T;
  const int nx = a.dx ? a.ntiles * ncb : 0;
  hipLaunchKernelGGL((enc_conv_bwd_list_kernel<K, S, ET>), dim3(nx + nwx * ncb), dim3(256), 0, st, a.x, a.w, a.y, a.dy, a.dx, a.dw,
                     a.dbias, a.segs, a.nsegs, a.tiles, a.ntiles, a.in_pitch, a.out_pitch, a.Cin, a.Cout, a.pad, a.relu, a.residual, nx,
                     nwx);
}
template <int K, int S>
static void launch_ecl(const EclArgs& a, int et, hipStream_t st) {
  if (et == 8) launch_ecl_et<K, S, 8>(a, st);
  else if (et == 16) launch_ecl_et<K, S, 16>(a, st);
  else launch_ecl_et<K, S, 32>(a, st);
}

extern "C" int wae_enc_conv_bwd_list(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* dbias,
                                     const wae_seg* segs, int32_t nsegs, const int32_t* tiles, int32_t ntiles, int32_t et,
                                     int32_t in_pitch, int32_t out_pitch, int32_t Cin, int32_t Cout, int32_t k, int32_t stride,
                                     int32_t pad, int32_t relu, int32_t residual, void* stream) {
  WAE_REQUIRE(x && w && dy && dw && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "enc_conv_bwd_list: bad arguments");
  WAE_REQUIRE(!relu || y, "enc_conv_bwd_list: relu needs the forward output y");
  WAE_REQUIRE(segs && nsegs > 0, "enc_conv_bwd_list: a segment table of nsegs > 0 records (got %d)", nsegs);
  WAE_REQUIRE(tiles && ntiles > 0, "enc_conv_bwd_list: a tile table of ntiles > 0 pairs (got %d)", ntiles);
  WAE_REQUIRE(et == 8 || et == 16 || et == 32, "enc_conv_bwd_list: et %d is not 8, 16 or 32", et);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "enc_conv_bwd_list: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(!residual || (stride == 1 && Cin == Cout && 2 * pad == k - 1), "enc_conv_bwd_list: residual needs a same-shape conv");
  WAE_REQUIRE((int64_t)ntiles * ((Cin + ECL_T - 1) / ECL_T) + (int64_t)((Cout + ECL_T - 1) / ECL_T) * ((Cin + ECL_T - 1) / ECL_T) < ((int64_t)1 << 31),
              "enc_conv_bwd_list: the grid does not fit 31 bits");
  const EclArgs a = {x, w, y, dy, dx, dw, dbias, segs, tiles, nsegs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual};
  hipStream_t st = as_stream(stream);
  if (k == 1 && stride == 1) launch_ecl<1, 1>(a, et, st);
  else if (k == 3 && stride == 1) launch_ecl<3, 1>(a, et, st);
  else if (k == 5 && stride == 2) launch_ecl<5, 2>(a, et, st);
  else if (k == 5 && stride == 1) launch_ecl<5, 1>(a, et, st);
  else {
    wae_set_error("enc_conv_bwd_list: (k, stride) = (%d, %d) has no list kernel ((1,1), (3,1), (5,2), (5,1) have); "
                  "run wae_enc_conv_bwd per utterance", k, stride);
    return WAE_EUNSUPPORTED;
  }
  return wae_check_launch("enc_conv_bwd_list");
}
