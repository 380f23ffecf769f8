// Upsampling stage over ROW RANGES of clips that live in RINGS (include/wae.h: wae_upsample_stage_fwd_rings): the
// ring-addressed twin of wae_upsample_stage_fwd_ranges (csrc/ups_list.hip).  A clip holds the last in_period of its Tin input frames,
// frame u at in_off + u % in_period, and output t goes to column (or, time-major, row) out_off + t % out_period.
//
// The ring is an ADDRESS and nothing else: both kernels first copy the frames an output needs into a linear piece of the clip -- LDS
// for the time-major tile, three registers for a channel-major output -- and then call the per-output functions of csrc/ups_fir.hpp,
// unchanged, on that copy.  The fmaf sequence of an output is therefore the ranges kernels' and the dense kernels', bit for bit,
// whatever the periods.
#include "wae_common.hpp"
#include "ups_fir.hpp"

static_assert(UPT == WAE_UPS_LIST_TILE_BTC, "the time-major tile is the dense last stage's");
#define UPR_CT WAE_UPS_LIST_TILE_CT
#define UPR_CPB 8   // channel rows per block of the channel-major stage (csrc/ups_list.hip: UPL_CPB)

template <typename E>
__device__ __forceinline__ void ups_ring_store(void* p, int64_t i, float v) { ((E*)p)[i] = (E)v; }

// The record of the tile blockIdx.x and the tile's first row; false: the workgroup retires, nothing read and nothing written (uniform
// over the workgroup, in front of every barrier and every access).  ups_find_range's tests with the pitch tests rewritten for rings;
// out_extent is the output's pitch (channel-major) or rows (time-major).  The first frame the record reads is that of t_lo's first
// tap, max(t_lo - s, 0) / s: a frame older than Tin - in_period is gone, and its slot holds a newer one.
__device__ __forceinline__ bool ups_find_ring(const wae_ups_ring* __restrict__ recs, int nrecs, int tile, int s, int in_pitch,
                                              int out_extent, wae_ups_ring& rec, int& t0, int& Tout) {
  const int bid = blockIdx.x;
  int lo = 0, hi = nrecs - 1;
  while (lo < hi) {                      // the last record with tile0 <= bid
    const int mid = (lo + hi + 1) >> 1;
    if (recs[mid].tile0 <= bid) lo = mid;
    else hi = mid - 1;
  }
  rec = recs[lo];
  const int next = recs[lo + 1].tile0;   // (the closing record for the last one)
  const int k = bid - rec.tile0;
  const int64_t To = (int64_t)rec.Tin * s;
  if (rec.Tin < 1 || k < 0 || bid >= next || To >= (int64_t)1 << 31) return false;
  if (rec.t_lo < 0 || rec.t_lo >= rec.t_hi || rec.t_hi > To) return false;
  const int64_t cnt = (int64_t)rec.t_hi - rec.t_lo;
  if ((int64_t)next - rec.tile0 != (cnt + tile - 1) / tile) return false;
  if (rec.in_period < 1 || rec.in_off < 0 || (int64_t)rec.in_off + rec.in_period > in_pitch) return false;
  if (rec.out_period < 1 || rec.out_off < 0 || (int64_t)rec.out_off + rec.out_period > out_extent || cnt > rec.out_period) return false;
  if (max(rec.t_lo - s, 0) / s < rec.Tin - rec.in_period) return false;
  Tout = (int)To;
  t0 = rec.t_lo + k * tile;              // < t_hi by the tile count
  return true;
}

// channel-major stage: grid (tiles, ceil(C / UPR_CPB)), thread = one output column of UPR_CPB channel rows in turn.  The taps of
// output t touch the frames f - 1, f, f + 1 (f = t / s) and no other; they are read from their ring slots into fr[] -- frame fb + i in
// fr[i], fb = max(f - 1, 0), 0 beyond Tin (never read: the walk stops at Tout) -- and the walk runs on that copy with the clip's
// origin moved to frame fb: t - fb s, Tout - fb s.  For fb > 0, t >= s, so the walk starts at tap 0 in both numberings, and (u / s,
// u % s) move by (fb, 0): the same taps of the same frames in the same order.
__global__ void __launch_bounds__(256) ups_stage_rings_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                              float* __restrict__ out, const wae_ups_ring* __restrict__ recs, int nrecs,
                                                              int in_pitch, int out_pitch, int C, int s) {
  wae_ups_ring rec;
  int t0, Tout;
  if (!ups_find_ring(recs, nrecs, UPR_CT, s, in_pitch, out_pitch, rec, t0, Tout)) return;
  const int t = t0 + threadIdx.x;
  if (t >= rec.t_hi) return;
  const int fb = max(t / s - 1, 0);
  int slot[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) slot[i] = fb + i < rec.Tin ? rec.in_off + (fb + i) % rec.in_period : -1;
  const int64_t o = (int64_t)rec.out_off + t % rec.out_period;
  for (int c = blockIdx.y * UPR_CPB; c < min(C, (blockIdx.y + 1) * UPR_CPB); ++c) {
    float fr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) fr[i] = slot[i] >= 0 ? in[(int64_t)c * in_pitch + slot[i]] : 0.f;
    out[(int64_t)c * out_pitch + o] = ups_fir_walk(w, fr, t - fb * s, s, Tout - fb * s);
  }
}

// csrc/ups_list.hip, ups_last_ranges_kernel, with the ring mapped where the tile's frames are staged in LDS and where a row is stored
template <typename E>
__global__ void __launch_bounds__(256) ups_last_rings_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                             void* __restrict__ out, const wae_ups_ring* __restrict__ recs, int nrecs,
                                                             int in_pitch, int rows, int C, int s, int Cp, int nfp) {
  extern __shared__ float sm[];              // [Cp][nfp] input frames, then [2s+1] taps, then [3][s] summed taps
  wae_ups_ring rec;
  int t0, Tout;
  if (!ups_find_ring(recs, nrecs, UPT, s, in_pitch, rows, rec, t0, Tout)) return;
  const int t1 = min(t0 + UPT, rec.t_hi);
  // frames of the CLIP that the rows [t0, t1) touch: fh < Tin; at most (UPT + 2s - 1) / s + 2 <= nfp of them; fl >= the record's first
  const int fl = max(t0 - s, 0) / s, fh = min(t1 - 1 + s, Tout - 1) / s, nf = fh - fl + 1;
  float* taps = sm + Cp * nfp;
  for (int i = threadIdx.x; i < Cp * nf; i += 256) {
    const int c = i / nf, f = i - c * nf;
    sm[c * nfp + f] = c < C ? in[(int64_t)c * in_pitch + rec.in_off + (fl + f) % rec.in_period] : 0.f;
  }
  if (threadIdx.x <= 2 * s) taps[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  float* co3 = taps + 2 * s + 1;
  if (threadIdx.x < 3 * s) co3[threadIdx.x] = ups_co3_entry(taps, threadIdx.x, s);
  __syncthreads();
  const int c = threadIdx.x % Cp, tl = threadIdx.x / Cp, tstep = 256 / Cp;
  const float* r = sm + c * nfp - fl;
  for (int t = t0 + tl; t < t1; t += tstep) {
    float acc = 0.f;
    if (c < C) {
      if (sizeof(E) == 2 && t >= s && t + s < Tout)   // interior: the same answer against Tin * s now and against the clip's final length
        acc = ups_fir_sum3(co3, r, t, s);
      else
        acc = ups_fir_walk(taps, r, t, s, Tout);
    }
    ups_ring_store<E>(out, ((int64_t)rec.out_off + t % rec.out_period) * Cp + c, acc);
  }
}

extern "C" int wae_upsample_stage_fwd_rings(const float* in, const float* w, void* out, const wae_ups_ring* recs, int32_t nrecs,
                                            int32_t ntiles, int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s,
                                            int32_t out_btc, int32_t Cp, int32_t dtype, void* stream) {
  WAE_REQUIRE(in && w && out && C > 0 && s > 0, "upsample_stage_fwd_rings: bad arguments");
  WAE_REQUIRE(recs && nrecs > 0, "upsample_stage_fwd_rings: a table of nrecs > 0 records and a closing one (got %d)", nrecs);
  WAE_REQUIRE(ntiles > 0, "upsample_stage_fwd_rings: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(in_pitch > 0 && out_pitch_or_rows > 0, "upsample_stage_fwd_rings: pitches must be > 0 (got %d, %d)", in_pitch,
              out_pitch_or_rows);
  hipStream_t st = as_stream(stream);
  if (!out_btc) {
    if ((C + UPR_CPB - 1) / UPR_CPB > 65535) {
      wae_set_error("upsample_stage_fwd_rings: C %d has no rings kernel", C);
      return WAE_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(ups_stage_rings_kernel, dim3(ntiles, (C + UPR_CPB - 1) / UPR_CPB), dim3(256), 0, st, in, w, (float*)out, recs,
                       nrecs, in_pitch, out_pitch_or_rows, C, s);
    return wae_check_launch("upsample_stage_fwd_rings");
  }
  WAE_REQUIRE(Cp >= C, "upsample_stage_fwd_rings: Cp %d < C %d", Cp, C);
  WAE_REQUIRE(wae_dtype_ok(dtype), "upsample_stage_fwd_rings: bad dtype %d", dtype);
  const int nfp = (UPT / s + 5) | 1;         // as the list's last stage
  const size_t lds = ((size_t)Cp * nfp + 2 * s + 1 + 3 * s) * sizeof(float);
  if (Cp > 256 || 256 % Cp != 0 || 3 * s > 256 || lds > 65536) {
    wae_set_error("upsample_stage_fwd_rings: the time-major rings kernel takes Cp dividing 256, 3 s <= 256 and 64 KiB of LDS "
                  "(got Cp %d, s %d, %zu bytes)", Cp, s, lds);
    return WAE_EUNSUPPORTED;
  }
  const dim3 grid(ntiles);
  if (dtype == WAE_BF16)
    hipLaunchKernelGGL(ups_last_rings_kernel<__bf16>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows, C,
                       s, Cp, nfp);
  else if (dtype == WAE_F16)
    hipLaunchKernelGGL(ups_last_rings_kernel<f16>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows, C, s,
                       Cp, nfp);
  else
    hipLaunchKernelGGL(ups_last_rings_kernel<float>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows, C,
                       s, Cp, nfp);
  return wae_check_launch("upsample_stage_fwd_rings");
}
