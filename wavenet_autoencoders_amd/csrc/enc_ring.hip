// Encoder block over COLUMN RANGES of utterances that live in RINGS (include/wae.h: wae_enc_conv_fwd_rings): the
// open utterances of a windowed encode session.  wae_enc_conv_fwd_ranges (csrc/enc_list.hip) addresses column u of a clip at
// in_off + u; here a clip holds the last in_period of its Tin input columns and column u lies at in_off + u % in_period, and output
// t goes to out_off + t % out_period (out_period 0: linear, out_off receives t_lo -- lin's packed new latents).
//
// The per-tile body MIRRORS csrc/enc_list.hip, enc_conv_fwd_tile_kernel (itself the mirror of csrc/misc.hip,
// enc_conv_fwd_tiled_kernel): the same constants, staging batches, weight batches, accumulation and epilogue.  The ring enters in
// three places only, all of them addresses: where the staging loop reads x, where the epilogue reads the residual and where it writes
// y.  The tile's window in LDS is the clip's columns ti0 .. ti0 + WIN - 1 in the clip's own order, so the per-output fmaf sequence is
// the ranges kernel's and the dense kernel's: every output is theirs bit for bit, whatever the periods.  It is a copy in a
// translation unit of its own so that csrc/enc_list.hip and the ISA of its instantiations stay untouched (enc_list.hip explains why
// its register allocation is fragile); a change to the arithmetic of one copy belongs in all three
// (tests/test_gpu_session_window.py compares them bit for bit).
#include "wae_common.hpp"

#define EC_T 32     // outputs per block along channels          (csrc/enc_list.hip: the same four constants)
#define EC_NS 8     // reduction slices
#define EC_CH 256   // input channels staged per chunk
#define EC_WB 8     // channels whose weights a thread requests together

// table = n wae_enc_ring records and a closing one; the record of blockIdx.x is found by the workgroup-uniform binary search of
// csrc/ups_list.hip.  The search and every test of the record run in front of every barrier and every access: a record that does not
// fit its buffers, or whose first tap is a column the ring no longer holds, retires the whole workgroup.
template <int K, int S, int ET>
__global__ void __launch_bounds__(256) enc_conv_fwd_ring_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                const wae_enc_ring* __restrict__ recs, int n, int in_pitch,
                                                                int out_pitch, int Cin, int Cout, int pad, int relu, int residual) {
  extern __shared__ float sm[];
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;   // LDS row pitch: whole 16-byte reads
  const int bid = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {                      // the last record with tile0 <= bid
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].tile0 <= bid) lo = mid;
    else hi = mid - 1;
  }
  const wae_enc_ring rec = recs[lo];
  const int next = recs[lo + 1].tile0;   // (the closing record for the last one)
  const int j = bid - rec.tile0;
  if (rec.Tin < 1 || j < 0 || bid >= next || rec.t_lo < 0 || rec.t_lo >= rec.t_hi) return;
  if ((int64_t)rec.Tin + 2 * pad < K || rec.t_hi > ((int64_t)rec.Tin + 2 * pad - K) / S + 1) return;
  const int64_t cnt = (int64_t)rec.t_hi - rec.t_lo;
  if ((int64_t)next - rec.tile0 != (cnt + ET - 1) / ET) return;
  if (rec.in_period < 1 || rec.in_off < 0 || (int64_t)rec.in_off + rec.in_period > in_pitch) return;
  if (rec.out_period < 0 || rec.out_off < 0) return;
  if ((int64_t)rec.out_off + (rec.out_period ? (int64_t)rec.out_period : cnt) > out_pitch || (rec.out_period && cnt > rec.out_period)) return;
  // the first tap of t_lo is the oldest column the record reads (the residual's column t is the same or later): a column older than
  // Tin - in_period is gone, and its slot holds a newer one
  if ((int64_t)rec.t_lo * S - pad < (int64_t)rec.Tin - rec.in_period) return;
  const int Tin = rec.Tin, t_end = rec.t_hi, t_org = rec.t_lo, in_period = rec.in_period, out_period = rec.out_period;
  const int to0 = rec.t_lo + j * ET;     // < t_hi by the tile count
  __builtin_assume(Tin >= 1 && to0 >= 0 && in_period >= 1);
  const int co0 = blockIdx.y * EC_T;
  const int ti0 = to0 * S - pad;
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int co = co0 + col;
  float acc[ET];
#pragma unroll
  for (int i = 0; i < ET; ++i) acc[i] = 0.f;
  const float* xb = x + rec.in_off;
  for (int c0 = 0; c0 < Cin; c0 += EC_CH) {
    const int nc = min(EC_CH, Cin - c0);
    __syncthreads();
    // staged in batches of 16 independent loads per thread; zeros outside the CLIP (ti < 0 or ti >= Tin); column ti from its ring slot
    for (int i0 = threadIdx.x; i0 < nc * WP; i0 += 256 * 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = i0 + u * 256;
        const int ci = i / WP, wv = i - ci * WP, ti = ti0 + wv;
        v[u] = (i < nc * WP && wv < WIN && ti >= 0 && ti < Tin) ? xb[(int64_t)(c0 + ci) * in_pitch + (unsigned)ti % (unsigned)in_period] : 0.f;
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
  float* yb = y + rec.out_off;
  for (int o = threadIdx.x; o < ET * EC_T; o += 256) {
    const int tl = o % ET, cl = o / ET;
    const int oc = co0 + cl, ot = to0 + tl;
    if (oc >= Cout || ot >= t_end) continue;
    float v = bias ? bias[oc] : 0.f;
#pragma unroll
    for (int q = 0; q < EC_NS; ++q) v += red[(q * ET + tl) * 33 + cl];
    if (relu) v = fmaxf(v, 0.f);
    if (residual) v += xb[(int64_t)oc * in_pitch + (unsigned)ot % (unsigned)in_period];      // a same-shape conv: column ot of the clip
    yb[(int64_t)oc * out_pitch + (out_period ? ot % out_period : ot - t_org)] = v;
  }
}

struct EncRingArgs {
  const float *x, *w, *bias;
  float* y;
  const wae_enc_ring* recs;
  int nrecs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual;
};

template <int K, int S, int ET>
static int launch_enc_rings_et(const EncRingArgs& a, hipStream_t st) {
  constexpr int WIN = (ET - 1) * S + K;
  constexpr int WP = (WIN + 3) & ~3;
  const size_t in = (size_t)(a.Cin < EC_CH ? a.Cin : EC_CH) * WP, r = (size_t)EC_NS * ET * 33;
  const size_t lds = (in > r ? in : r) * sizeof(float);
  static WaeLdsCache cache;
  if (int rc = wae_ensure_lds((const void*)enc_conv_fwd_ring_kernel<K, S, ET>, cache, lds, "enc_conv_fwd_rings"); rc != WAE_OK) return rc;
  hipLaunchKernelGGL((enc_conv_fwd_ring_kernel<K, S, ET>), dim3(a.ntiles, (a.Cout + EC_T - 1) / EC_T), dim3(256), lds, st, a.x, a.w,
                     a.bias, a.y, a.recs, a.nrecs, a.in_pitch, a.out_pitch, a.Cin, a.Cout, a.pad, a.relu, a.residual);
  return WAE_OK;
}
template <int K, int S>
static int launch_enc_rings(const EncRingArgs& a, int et, hipStream_t st) {
  if (et == 8) return launch_enc_rings_et<K, S, 8>(a, st);
  if (et == 16) return launch_enc_rings_et<K, S, 16>(a, st);
  return launch_enc_rings_et<K, S, 32>(a, st);
}

extern "C" int wae_enc_conv_fwd_rings(const float* x, const float* w, const float* bias, float* y, const wae_enc_ring* recs,
                                      int32_t nrecs, int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin,
                                      int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, int32_t residual,
                                      void* stream) {
  WAE_REQUIRE(x && w && y && Cin > 0 && Cout > 0 && k > 0 && stride > 0 && pad >= 0, "enc_conv_fwd_rings: bad arguments");
  WAE_REQUIRE(recs && nrecs > 0, "enc_conv_fwd_rings: a table of nrecs > 0 records and a closing one (got %d)", nrecs);
  WAE_REQUIRE(ntiles > 0, "enc_conv_fwd_rings: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(et == 8 || et == 16 || et == 32, "enc_conv_fwd_rings: et %d is not 8, 16 or 32", et);
  WAE_REQUIRE(in_pitch > 0 && out_pitch > 0, "enc_conv_fwd_rings: pitches must be > 0 (got %d, %d)", in_pitch, out_pitch);
  WAE_REQUIRE(!residual || (stride == 1 && Cin == Cout && 2 * pad == k - 1), "enc_conv_fwd_rings: residual needs a same-shape conv");
  const EncRingArgs a = {x, w, bias, y, recs, nrecs, ntiles, in_pitch, out_pitch, Cin, Cout, pad, relu, residual};
  hipStream_t st = as_stream(stream);
  int rc;
  if (k == 1 && stride == 1) rc = launch_enc_rings<1, 1>(a, et, st);
  else if (k == 3 && stride == 1) rc = launch_enc_rings<3, 1>(a, et, st);
  else if (k == 5 && stride == 2) rc = launch_enc_rings<5, 2>(a, et, st);
  else if (k == 5 && stride == 1) rc = launch_enc_rings<5, 1>(a, et, st);
  else {
    wae_set_error("enc_conv_fwd_rings: (k, stride) = (%d, %d) has no rings kernel ((1,1), (3,1), (5,2), (5,1) have)", k, stride);
    return WAE_EUNSUPPORTED;
  }
  if (rc != WAE_OK) return rc;
  return wae_check_launch("enc_conv_fwd_rings");
}
