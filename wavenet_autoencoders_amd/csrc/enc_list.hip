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
// The per-tile body below (enc_tile) MIRRORS csrc/misc.hip, enc_conv_fwd_tiled_kernel (the lines between `extern __shared__ float sm[]`
// and the kernel's closing brace): the same constants, staging, weight batches, accumulation and epilogue.  What differs is addressing
// only: the row pitch of x (in_pitch for Tin) and of y (out_pitch for Tout), the clip's column offsets, and where the tile comes from.
// It is a copy of misc.hip's and not a shared header so that csrc/misc.hip and its built ISA stay untouched; a change to either copy's
// arithmetic belongs in both (tests/test_gpu_encode_list.py compares them bit for bit).  Inside this file there is ONE body: the list
// entry (tiles at multiples of ET below the segment's Tout) and the ranges entry (wae_enc_conv_fwd_ranges: tiles counted from a
// record's t_lo, valid outputs stopping at its t_hi; the clips of an encode session whose features still arrive) launch two
// instantiations of one kernel template, which differ in where the tile comes from and where its valid outputs stop.
#include "wae_common.hpp"

#define EC_T 32     // outputs per block along channels          (csrc/misc.hip: the same four constants)
#define EC_NS 8     // reduction slices
#define EC_CH 256   // input channels staged per chunk
#define EC_WB 8     // channels whose weights a thread requests together

// ONE kernel template for both entries: the tile's SOURCE is a template parameter, the per-tile body below it is shared text.
//   RANGES = false (wae_enc_conv_fwd_list): table = wae_seg records, n of them; tiles = (segment, to0) pairs, tiles at multiples of ET
//     below the segment's Tout.
//   RANGES = true (wae_enc_conv_fwd_ranges): table = n wae_enc_range records and a closing one, tiles unused.  A record names the
//     input columns that are valid NOW (Tin) and the outputs [t_lo, t_hi) to compute, in the clip's own numbering; its tiles count from
//     t_lo.  The record of blockIdx.x is found by the workgroup-uniform binary search of csrc/ups_list.hip (the last record with
//     tile0 <= blockIdx.x; the closing record holds the tile count).  The kernel carries no "open" flag: the host keeps t_hi within
//     the outputs whose taps all lie below Tin while the clip is open (packing.enc_feed_plan), so the zero a tap at or beyond Tin reads
//     is only ever the clip's true right-hand padding.
// Either way the source yields: the clip's first column of x (in_off) and its valid input columns (Tin; a tap outside [0, Tin) reads
// 0), the tile's first output (to0), where the valid outputs stop (t_end), and the column of y (y_off) that receives output t_org.
// Nothing in an output's value depends on to0, on t_end or on ET, so a tile at any origin writes the bytes of the dense call.
// The source is uniform over the workgroup and runs in front of every barrier and every access: a record that does not fit its
// buffers retires the whole workgroup (the host builds the tables, but the kernel does not trust them with memory).
// Why a kernel template and not a __device__ function called from two kernels: with the body in an inlined function the compiler
// allocated the strided list kernels differently (k 5, stride 2, ET 16: 250 -> 260 VGPRs, two waves per SIMD -> one, and 51 % more
// time; ET 32 14 % more).  With RANGES = false this template is the list kernel's text as it was: its instantiations keep the
// registers, the occupancy and -- up to a few moves and scalar instructions of the prologue -- the instruction counts they had
// (profiles/enc_list_ab.txt; tools/ab_enc_list.py times two builds against each other).
template <int K, int S, int ET, bool RANGES>
__global__ void __launch_bounds__(256) enc_conv_fwd_tile_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                const void* __restrict__ table, int n,
                                                                const int32_t* __restrict__ tiles, int in_pitch, int out_pitch, int Cin,
                                                                int Cout, int pad, int relu, int residual) {
  extern __shared__ float sm[];
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;   // LDS row pitch: whole 16-byte reads
  int in_off, y_off, Tin, to0, t_end, t_org;
  if constexpr (!RANGES) {
    const int sg = tiles[2 * blockIdx.x];
    to0 = tiles[2 * blockIdx.x + 1];
    if (sg < 0 || sg >= n) return;
    const wae_seg seg = ((const wae_seg*)table)[sg];
    Tin = seg.Tin;
    const int Tout = seg.Tout;
    if (Tin < 1 || seg.in_off < 0 || (int64_t)seg.in_off + Tin > in_pitch || seg.out_off < 0 || (int64_t)seg.out_off + Tout > out_pitch ||
        Tout != (Tin + 2 * pad - K) / S + 1 || Tin + 2 * pad < K || to0 < 0 || to0 >= Tout)
      return;
    in_off = seg.in_off, y_off = seg.out_off, t_end = Tout, t_org = 0;
  } else {
    const wae_enc_range* recs = (const wae_enc_range*)table;
    const int bid = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) {                      // the last record with tile0 <= bid
      const int mid = (lo + hi + 1) >> 1;
      if (recs[mid].tile0 <= bid) lo = mid;
      else hi = mid - 1;
    }
    const wae_enc_range rec = recs[lo];
    const int next = recs[lo + 1].tile0;   // (the closing record for the last one)
    const int j = bid - rec.tile0;
    if (rec.Tin < 1 || j < 0 || bid >= next || rec.t_lo < 0 || rec.t_lo >= rec.t_hi) return;
    if ((int64_t)rec.Tin + 2 * pad < K || rec.t_hi > ((int64_t)rec.Tin + 2 * pad - K) / S + 1) return;
    const int64_t cnt = (int64_t)rec.t_hi - rec.t_lo;
    if ((int64_t)next - rec.tile0 != (cnt + ET - 1) / ET) return;
    if (rec.in_off < 0 || (int64_t)rec.in_off + rec.Tin > in_pitch || rec.out_col < 0 || (int64_t)rec.out_col + cnt > out_pitch) return;
    in_off = rec.in_off, y_off = rec.out_col, Tin = rec.Tin, t_end = rec.t_hi, t_org = rec.t_lo;
    to0 = rec.t_lo + j * ET;               // < t_hi by the tile count
  }
  __builtin_assume(Tin >= 1 && to0 >= 0);  // (both sources have checked it; it lets the staging test ti against [0, Tin) in one compare)
  const int co0 = blockIdx.y * EC_T;
  const int ti0 = to0 * S - pad;
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int co = co0 + col;
  float acc[ET];
#pragma unroll
  for (int i = 0; i < ET; ++i) acc[i] = 0.f;
  const float* xb = x + in_off;
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
  float* yb = y + y_off;
  for (int o = threadIdx.x; o < ET * EC_T; o += 256) {
    const int tl = o % ET, cl = o / ET;
    const int oc = co0 + cl, ot = to0 + tl;
    if (oc >= Cout || ot >= t_end) continue;
    float v = bias ? bias[oc] : 0.f;
#pragma unroll
    for (int q = 0; q < EC_NS; ++q) v += red[(q * ET + tl) * 33 + cl];
    if (relu) v = fmaxf(v, 0.f);
    if (residual) v += xb[(int64_t)oc * in_pitch + ot];      // a same-shape conv: column ot of the clip
    yb[(int64_t)oc * out_pitch + (ot - t_org)] = v;
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
  if (int rc = wae_ensure_lds((const void*)enc_conv_fwd_tile_kernel<K, S, ET, false>, cache, lds, "enc_conv_fwd_list"); rc != WAE_OK)
    return rc;
  hipLaunchKernelGGL((enc_conv_fwd_tile_kernel<K, S, ET, false>), dim3(a.ntiles, (a.Cout + EC_T - 1) / EC_T), dim3(256), lds, st, a.x,
                     a.w, a.bias, a.y, a.segs, a.nsegs, a.tiles, a.in_pitch, a.out_pitch, a.Cin, a.Cout, a.pad, a.relu, a.residual);
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

struct EncRangeArgs {
  const float *x, *w, *bias;
  float* y;
  const wae_enc_range* recs;
  int nrecs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual;
};

template <int K, int S, int ET>
static int launch_enc_ranges_et(const EncRangeArgs& a, hipStream_t st) {
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;
  const size_t in = (size_t)(a.Cin < EC_CH ? a.Cin : EC_CH) * WP, r = (size_t)EC_NS * ET * 33;
  const size_t lds = (in > r ? in : r) * sizeof(float);
  static WaeLdsCache cache;
  if (int rc = wae_ensure_lds((const void*)enc_conv_fwd_tile_kernel<K, S, ET, true>, cache, lds, "enc_conv_fwd_ranges"); rc != WAE_OK)
    return rc;
  hipLaunchKernelGGL((enc_conv_fwd_tile_kernel<K, S, ET, true>), dim3(a.ntiles, (a.Cout + EC_T - 1) / EC_T), dim3(256), lds, st, a.x,
                     a.w, a.bias, a.y, a.recs, a.nrecs, (const int32_t*)nullptr, a.in_pitch, a.out_pitch, a.Cin, a.Cout, a.pad, a.relu,
                     a.residual);
  return WAE_OK;
}
template <int K, int S>
static int launch_enc_ranges(const EncRangeArgs& a, int et, hipStream_t st) {
  if (et == 8) return launch_enc_ranges_et<K, S, 8>(a, st);
  if (et == 16) return launch_enc_ranges_et<K, S, 16>(a, st);
  return launch_enc_ranges_et<K, S, 32>(a, st);
}

extern "C" int wae_enc_conv_fwd_ranges(const float* x, const float* w, const float* bias, float* y, const wae_enc_range* recs,
                                       int32_t nrecs, int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin,
                                       int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, int32_t residual,
                                       void* stream) {
  WAE_REQUIRE(x && w && y && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "enc_conv_fwd_ranges: bad arguments");
  WAE_REQUIRE(recs && nrecs > 0, "enc_conv_fwd_ranges: a table of nrecs > 0 records and a closing one (got %d)", nrecs);
  WAE_REQUIRE(ntiles > 0, "enc_conv_fwd_ranges: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(et == 8 || et == 16 || et == 32, "enc_conv_fwd_ranges: et %d is not 8, 16 or 32", et);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "enc_conv_fwd_ranges: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(!residual || (stride == 1 && Cin == Cout && 2 * pad == k - 1), "enc_conv_fwd_ranges: residual needs a same-shape conv");
  const EncRangeArgs a = {x, w, bias, y, recs, nrecs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual};
  hipStream_t st = as_stream(stream);
  int rc;
  if (k == 1 && stride == 1) rc = launch_enc_ranges<1, 1>(a, et, st);
  else if (k == 3 && stride == 1) rc = launch_enc_ranges<3, 1>(a, et, st);
  else if (k == 5 && stride == 2) rc = launch_enc_ranges<5, 2>(a, et, st);
  else if (k == 5 && stride == 1) rc = launch_enc_ranges<5, 1>(a, et, st);
  else {
    wae_set_error("enc_conv_fwd_ranges: (k, stride) = (%d, %d) has no ranges kernel ((1,1), (3,1), (5,2), (5,1) have)", k, stride);
    return WAE_EUNSUPPORTED;
  }
  if (rc != WAE_OK) return rc;
  return wae_check_launch("enc_conv_fwd_ranges");
}
