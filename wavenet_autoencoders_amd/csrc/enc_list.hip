// Encoder block over a LIST of utterances of unequal lengths (include/wae.h: wae_enc_conv_fwd_list; vqvae_model.py:17-23, :48-51).
//
// The activations of the list are channel-major and packed along time: x is (Cin, in_pitch), utterance i owns the columns
// [in_off_i, in_off_i + Tin_i); y is (Cout, out_pitch) with out_off_i, Tout_i.  A workgroup looks its (segment, first output step) up
// in the tile table and then does, for that tile of that utterance, what enc_conv_fwd_tiled_kernel (csrc/misc.hip) does for a tile of
// a batch-1 call: the value of one output is the same sequence of operations -- input-channel chunks of EC_CH, the thread's slice
// [ca, cb) of the chunk in order, the taps in order, all by fmaf; then bias + the EC_NS slice partials in the order q = 0..7 -- and
// nothing in that sequence depends on ET, on the tile's position, on the other utterances or on the pitches.  Every utterance of the
// list therefore gets the bytes of its own batch-1 wae_enc_conv_fwd.  A tap outside [0, Tin_i) reads 0, never the neighbour's column.
//
// The per-tile body below MIRRORS csrc/misc.hip, enc_conv_fwd_tiled_kernel (the lines between `extern __shared__ float sm[]` and the
// kernel's closing brace): the same constants, staging, weight batches, accumulation and epilogue.  What differs is addressing only:
// the row pitch of x (in_pitch for Tin) and of y (out_pitch for Tout), the segment's column offsets, and where the tile comes from.
// It is a copy and not a shared header so that csrc/misc.hip and its built ISA stay untouched; a change to either copy's arithmetic
// belongs in both (tests/test_gpu_encode_list.py compares them bit for bit).
#include "wae_common.hpp"

#define EC_T 32     // outputs per block along channels          (csrc/misc.hip: the same four constants)
#define EC_NS 8     // reduction slices
#define EC_CH 256   // input channels staged per chunk
#define EC_WB 8     // channels whose weights a thread requests together

template <int K, int S, int ET>
__global__ void __launch_bounds__(256) enc_conv_fwd_list_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                const wae_seg* __restrict__ segs, int nsegs,
                                                                const int32_t* __restrict__ tiles, int in_pitch, int out_pitch, int Cin,
                                                                int Cout, int pad, int relu, int residual) {
  extern __shared__ float sm[];
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;   // LDS row pitch: whole 16-byte reads
  // the tile: uniform over the workgroup, so a record that does not fit its buffers retires the whole workgroup before any barrier
  // and before any access (the host builds the tables -- packing.encode_list_plan -- but the kernel does not trust them with memory)
  const int sg = tiles[2 * blockIdx.x], to0 = tiles[2 * blockIdx.x + 1];
  if (sg < 0 || sg >= nsegs) return;
  const wae_seg seg = segs[sg];
  const int Tin = seg.Tin, Tout = seg.Tout;
  if (Tin < 1 || seg.in_off < 0 || (int64_t)seg.in_off + Tin > in_pitch || seg.out_off < 0 || (int64_t)seg.out_off + Tout > out_pitch ||
      Tout != (Tin + 2 * pad - K) / S + 1 || Tin + 2 * pad < K || to0 < 0 || to0 >= Tout)
    return;
  const int co0 = blockIdx.y * EC_T;
  const int ti0 = to0 * S - pad;
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int co = co0 + col;
  float acc[ET];
#pragma unroll
  for (int i = 0; i < ET; ++i) acc[i] = 0.f;
  const float* xb = x + seg.in_off;
  for (int c0 = 0; c0 < Cin; c0 += EC_CH) {
    const int nc = min(EC_CH, Cin - c0);
    __syncthreads();
    // staged in batches of 16 independent loads per thread; zeros outside the SEGMENT (ti < 0 or ti >= Tin)
    for (int i0 = threadIdx.x; i0 < nc * WP; i0 += 256 * 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = i0 + u * 256;
        const int ci = i / WP, wv = i - ci * WP, ti = ti0 + wv;
        v[u] = (i < nc * WP && wv < WIN && ti >= 0 && ti < Tin) ? xb[(int64_t)(c0 + ci) * in_pitch + ti] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (i0 + u * 256 < nc * WP) sm[i0 + u * 256] = v[u];
    }
    __syncthreads();
    const int per = (nc + EC_NS - 1) / EC_NS;
    const int ca = sl * per, cb = min(nc, ca + per);
    if (co < Cout) {
      // the weights of a thread (row co, channels [ca, cb)) in batches of EC_WB channels, the NEXT batch requested while this one is used
      const float* wrow = w + ((int64_t)co * Cin + c0) * K;
      float wv[EC_WB][K], wn[EC_WB][K];
      auto fetch = [&](float (&dst)[EC_WB][K], int cc) {
#pragma unroll
        for (int u = 0; u < EC_WB; ++u)
#pragma unroll
          for (int j = 0; j < K; ++j) dst[u][j] = cc + u < cb ? wrow[(cc + u) * K + j] : 0.f;
      };
      if (ca < cb) fetch(wv, ca);
      for (int cc = ca; cc < cb; cc += EC_WB) {
        if (cc + EC_WB < cb) fetch(wn, cc + EC_WB);
#pragma unroll
        for (int u = 0; u < EC_WB; ++u) {
          // the channel's input window moves LDS -> registers once (16-byte broadcast reads) and serves every tap
          const f32x4* xr4 = (const f32x4*)(sm + min(cc + u, cb - 1) * WP);
          float xw[WP];
#pragma unroll
          for (int q = 0; q < WP / 4; ++q) {
            const f32x4 v = xr4[q];
            xw[4 * q] = v.x; xw[4 * q + 1] = v.y; xw[4 * q + 2] = v.z; xw[4 * q + 3] = v.w;
          }
#pragma unroll
          for (int j = 0; j < K; ++j)
#pragma unroll
            for (int t = 0; t < ET; ++t) acc[t] = fmaf(wv[u][j], xw[t * S + j], acc[t]);
        }
#pragma unroll
        for (int u = 0; u < EC_WB; ++u)
#pragma unroll
          for (int j = 0; j < K; ++j) wv[u][j] = wn[u][j];
      }
    }
  }
  __syncthreads();
  float* red = sm;   // [slice][t][33]
#pragma unroll
  for (int t = 0; t < ET; ++t) red[(sl * ET + t) * 33 + col] = acc[t];
  __syncthreads();
  float* yb = y + seg.out_off;
  for (int o = threadIdx.x; o < ET * EC_T; o += 256) {
    const int tl = o % ET, cl = o / ET;
    const int oc = co0 + cl, ot = to0 + tl;
    if (oc >= Cout || ot >= Tout) continue;
    float v = bias ? bias[oc] : 0.f;
#pragma unroll
    for (int q = 0; q < EC_NS; ++q) v += red[(q * ET + tl) * 33 + cl];
    if (relu) v = fmaxf(v, 0.f);
    if (residual) v += xb[(int64_t)oc * in_pitch + ot];      // a same-shape conv: Tout == Tin, column ot of the segment
    yb[(int64_t)oc * out_pitch + ot] = v;
  }
}

struct EncListArgs {
  const float *x, *w, *bias;
  float* y;
  const wae_seg* segs;
  const int32_t* tiles;
  int nsegs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual;
};

template <int K, int S, int ET>
static int launch_enc_list_et(const EncListArgs& a, hipStream_t st) {
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;
  const size_t in = (size_t)(a.Cin < EC_CH ? a.Cin : EC_CH) * WP, r = (size_t)EC_NS * ET * 33;
  const size_t lds = (in > r ? in : r) * sizeof(float);
  static WaeLdsCache cache;
  if (int rc = wae_ensure_lds((const void*)enc_conv_fwd_list_kernel<K, S, ET>, cache, lds, "enc_conv_fwd_list"); rc != WAE_OK) return rc;
  hipLaunchKernelGGL((enc_conv_fwd_list_kernel<K, S, ET>), dim3(a.ntiles, (a.Cout + EC_T - 1) / EC_T), dim3(256), lds, st, a.x, a.w, a.bias,
                     a.y, a.segs, a.nsegs, a.tiles, a.in_pitch, a.out_pitch, a.Cin, a.Cout, a.pad, a.relu, a.residual);
  return WAE_OK;
}
template <int K, int S>
static int launch_enc_list(const EncListArgs& a, int et, hipStream_t st) {
  if (et == 8) return launch_enc_list_et<K, S, 8>(a, st);
  if (et == 16) return launch_enc_list_et<K, S, 16>(a, st);
  return launch_enc_list_et<K, S, 32>(a, st);
}

extern "C" int wae_enc_conv_fwd_list(const float* x, const float* w, const float* bias, float* y, const wae_seg* segs, int32_t nsegs,
                                     const int32_t* tiles, int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin,
                                     int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, int32_t residual, void* stream) {
  WAE_REQUIRE(x && w && y && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "enc_conv_fwd_list: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "enc_conv_fwd_list: a segment table of nsegs > 0 records (got %d)", nsegs);
  WAE_REQUIRE(tiles && ntiles > 0, "enc_conv_fwd_list: a tile table of ntiles > 0 pairs (got %d)", ntiles);
  WAE_REQUIRE(et == 8 || et == 16 || et == 32, "enc_conv_fwd_list: et %d is not 8, 16 or 32", et);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "enc_conv_fwd_list: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(!residual || (stride == 1 && Cin == Cout && 2 * pad == k - 1), "enc_conv_fwd_list: residual needs a same-shape conv");
  const EncListArgs a = {x, w, bias, y, segs, tiles, nsegs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual};
  hipStream_t st = as_stream(stream);
  int rc;
  if (k == 1 && stride == 1) rc = launch_enc_list<1, 1>(a, et, st);
  else if (k == 3 && stride == 1) rc = launch_enc_list<3, 1>(a, et, st);
  else if (k == 5 && stride == 2) rc = launch_enc_list<5, 2>(a, et, st);
  else if (k == 5 && stride == 1) rc = launch_enc_list<5, 1>(a, et, st);
  else {
    wae_set_error("enc_conv_fwd_list: (k, stride) = (%d, %d) has no list kernel ((1,1), (3,1), (5,2), (5,1) have); "
                  "run wae_enc_conv_fwd per utterance", k, stride);
    return WAE_EUNSUPPORTED;
  }
  if (rc != WAE_OK) return rc;
  return wae_check_launch("enc_conv_fwd_list");
}
