// Upsampling network over a LIST of utterances of unequal lengths (include/wae.h: wae_upsample_stage_fwd_list, wae_to_btc_list;
// upsample.py:12-85, forward, inference) -- the decode side's counterpart of csrc/enc_list.hip -- and over ROW RANGES of clips that
// are still growing (wae_upsample_stage_fwd_ranges, at the end of this file).
//
// The activations of the list are channel-major and packed along time: (C, pitch) fp32, item i owning the columns [off_i, off_i + T_i).
// The last launch of a chain writes the time-major operand (rows, Cp) the list and span decode kernels read, item i at the rows
// [out_off_i, out_off_i + Tout_i) -- any rows: the caller's order.  A workgroup is one tile of one item.  It finds the item by a
// binary search of its block index in the records' tile0 (a running sum with a closing record), uniform over the workgroup, and then
// does for that tile what the dense kernels of csrc/misc.hip do for a tile of a batch-1 call: the per-output arithmetic is the SAME
// functions (csrc/ups_fir.hpp), called with the item's own channel row and the item's own Tout.  In particular the choice between the
// three summed taps and the tap walk of a 16-bit last stage is taken against the item's length, never the packed one.
#include "wae_common.hpp"
#include "ups_fir.hpp"

static_assert(UPT == WAE_UPS_LIST_TILE_BTC, "the time-major tile is the dense last stage's");
#define UPL_CT WAE_UPS_LIST_TILE_CT

template <typename E>
__device__ __forceinline__ void ups_store(void* p, int64_t i, float v) { ((E*)p)[i] = (E)v; }

// The record of the tile blockIdx.x and the tile's index k inside its item; false: the workgroup retires (a block index the table
// does not cover, an item without frames, a tile count that contradicts Tout = Tin * mul, an input range outside the pitch).  Uniform
// over the workgroup, in front of every barrier and every access.  The host builds the table (packing.upsample_list_plan), but the
// kernel does not trust it with memory; the caller checks the output range, which differs per form.
__device__ __forceinline__ bool ups_find(const wae_ups_seg* __restrict__ segs, int nsegs, int tile, int mul, int in_pitch,
                                         wae_ups_seg& seg, int& k, int& Tout) {
  const int bid = blockIdx.x;
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
  if (seg.in_off < 0 || (int64_t)seg.in_off + seg.Tin > in_pitch || seg.out_off < 0) return false;
  Tout = (int)To;
  return true;
}

// channel-major stage: grid (tiles, ceil(C / UPL_CPB)), thread = one output column of UPL_CPB channel rows in turn (the search for the
// item is paid once per UPL_CPB x 256 outputs; which block computes a row does not enter its value)
#define UPL_CPB 8
__global__ void __launch_bounds__(256) ups_stage_list_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                             float* __restrict__ out, const wae_ups_seg* __restrict__ segs, int nsegs,
                                                             int in_pitch, int out_pitch, int C, int s) {
  wae_ups_seg seg;
  int k, Tout;
  if (!ups_find(segs, nsegs, UPL_CT, s, in_pitch, seg, k, Tout)) return;
  if ((int64_t)seg.out_off + Tout > out_pitch) return;
  const int t = k * UPL_CT + threadIdx.x;
  if (t >= Tout) return;
  for (int c = blockIdx.y * UPL_CPB; c < min(C, (blockIdx.y + 1) * UPL_CPB); ++c) {
    const float* r = in + (int64_t)c * in_pitch + seg.in_off;
    // ups_fir_taps' fmaf sequence (the same taps of the same frames in the same order) without its division per tap
    out[(int64_t)c * out_pitch + seg.out_off + t] = ups_fir_walk(w, r, t, s, Tout);
  }
}

// Last stage, time-major output: a block = UPT output steps of one item; csrc/misc.hip, upsample_last_kernel, with the item's record in
// the place of (blockIdx.y, Tin) and the pitches in the place of the dense strides.
template <typename E>
__global__ void __launch_bounds__(256) ups_last_list_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                            void* __restrict__ out, const wae_ups_seg* __restrict__ segs, int nsegs,
                                                            int in_pitch, int rows, int C, int s, int Cp, int nfp) {
  extern __shared__ float sm[];              // [Cp][nfp] input frames, then [2s+1] taps, then [3][s] summed taps
  wae_ups_seg seg;
  int k, Tout;
  if (!ups_find(segs, nsegs, UPT, s, in_pitch, seg, k, Tout)) return;
  if ((int64_t)seg.out_off + Tout > rows) return;
  const int t0 = k * UPT;
  const int fl = max(t0 - s, 0) / s, fh = min(t0 + UPT - 1 + s, Tout - 1) / s, nf = fh - fl + 1;   // frames of the ITEM: fh < Tin
  float* taps = sm + Cp * nfp;
  for (int i = threadIdx.x; i < Cp * nf; i += 256) {
    const int c = i / nf, f = i - c * nf;
    sm[c * nfp + f] = c < C ? in[(int64_t)c * in_pitch + seg.in_off + fl + f] : 0.f;
  }
  if (threadIdx.x <= 2 * s) taps[threadIdx.x] = w[threadIdx.x];
  __syncthreads();
  float* co3 = taps + 2 * s + 1;
  if (threadIdx.x < 3 * s) co3[threadIdx.x] = ups_co3_entry(taps, threadIdx.x, s);
  __syncthreads();
  const int c = threadIdx.x % Cp, tl = threadIdx.x / Cp, tstep = 256 / Cp;
  const float* r = sm + c * nfp - fl;
  for (int t = t0 + tl; t < min(t0 + UPT, Tout); t += tstep) {
    float acc = 0.f;
    if (c < C) {
      if (sizeof(E) == 2 && t >= s && t + s < Tout)   // interior OF THE ITEM (Tout is the item's)
        acc = ups_fir_sum3(co3, r, t, s);
      else
        acc = ups_fir_walk(taps, r, t, s, Tout);
    }
    ups_store<E>(out, ((int64_t)seg.out_off + t) * Cp + c, acc);
  }
}

// (C, in_pitch) fp32 -> (rows, Cp) dtype, 64 steps of one item x 64 channels per block through the LDS tile of to_btc_kernel
template <typename E>
__global__ void __launch_bounds__(256) to_btc_list_kernel(const float* __restrict__ in, void* __restrict__ out,
                                                          const wae_ups_seg* __restrict__ segs, int nsegs, int in_pitch, int C, int Cp) {
  __shared__ float tile[64][65];
  wae_ups_seg seg;
  int k, T;
  if (!ups_find(segs, nsegs, 64, 1, in_pitch, seg, k, T)) return;
  const int t0 = k * 64, c0 = blockIdx.y * 64;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  for (int i = ly; i < 64; i += 4) {
    const int c = c0 + i, t = t0 + lx;
    tile[i][lx] = (c < C && t < T) ? in[(int64_t)c * in_pitch + seg.in_off + t] : 0.f;
  }
  __syncthreads();
  for (int i = ly; i < 64; i += 4) {
    const int t = t0 + i, c = c0 + lx;
    if (t < T && c < Cp) ups_store<E>(out, ((int64_t)seg.out_off + t) * Cp + c, tile[lx][i]);
  }
}

// ---- row ranges of items (wae_upsample_stage_fwd_ranges): the clips of a decode session whose frames arrive while they decode.
// A record names the input columns that are valid NOW (Tin) and the output rows [t_lo, t_hi) to compute; the tiles of a record count
// from t_lo.  The per-output functions are called with Tout = Tin * s: for the rows the host may ask for (t_hi <= (Tin - 1) * s while
// the clip is open) every tap lies below Tout, so the walk and the interior test do what they will do against the clip's final length.
// The record and the tile's first row; false: the workgroup retires (as ups_find: nothing read, nothing written).
__device__ __forceinline__ bool ups_find_range(const wae_ups_range* __restrict__ recs, int nrecs, int tile, int s, int in_pitch,
                                               wae_ups_range& rec, int& t0, int& Tout) {
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
  if ((int64_t)next - rec.tile0 != ((int64_t)rec.t_hi - rec.t_lo + tile - 1) / tile) return false;
  if (rec.in_off < 0 || (int64_t)rec.in_off + rec.Tin > in_pitch || rec.out_off < 0) return false;
  Tout = (int)To;
  t0 = rec.t_lo + k * tile;              // < t_hi by the tile count
  return true;
}

__global__ void __launch_bounds__(256) ups_stage_ranges_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                               float* __restrict__ out, const wae_ups_range* __restrict__ recs, int nrecs,
                                                               int in_pitch, int out_pitch, int C, int s) {
  wae_ups_range rec;
  int t0, Tout;
  if (!ups_find_range(recs, nrecs, UPL_CT, s, in_pitch, rec, t0, Tout)) return;
  if ((int64_t)rec.out_off + rec.t_hi > out_pitch) return;
  const int t = t0 + threadIdx.x;
  if (t >= rec.t_hi) return;
  for (int c = blockIdx.y * UPL_CPB; c < min(C, (blockIdx.y + 1) * UPL_CPB); ++c) {
    const float* r = in + (int64_t)c * in_pitch + rec.in_off;
    out[(int64_t)c * out_pitch + rec.out_off + t] = ups_fir_walk(w, r, t, s, Tout);
  }
}

// ups_last_list_kernel on the rows [t0, min(t0 + UPT, t_hi)) of a record; t0 is any row, as is a dense tile's against the scale
template <typename E>
__global__ void __launch_bounds__(256) ups_last_ranges_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                              void* __restrict__ out, const wae_ups_range* __restrict__ recs, int nrecs,
                                                              int in_pitch, int rows, int C, int s, int Cp, int nfp) {
  extern __shared__ float sm[];              // [Cp][nfp] input frames, then [2s+1] taps, then [3][s] summed taps
  wae_ups_range rec;
  int t0, Tout;
  if (!ups_find_range(recs, nrecs, UPT, s, in_pitch, rec, t0, Tout)) return;
  if ((int64_t)rec.out_off + rec.t_hi > rows) return;
  const int t1 = min(t0 + UPT, rec.t_hi);
  // frames of the CLIP that the rows [t0, t1) touch: fh < Tin; at most (UPT + 2s - 1) / s + 2 <= nfp of them
  const int fl = max(t0 - s, 0) / s, fh = min(t1 - 1 + s, Tout - 1) / s, nf = fh - fl + 1;
  float* taps = sm + Cp * nfp;
  for (int i = threadIdx.x; i < Cp * nf; i += 256) {
    const int c = i / nf, f = i - c * nf;
    sm[c * nfp + f] = c < C ? in[(int64_t)c * in_pitch + rec.in_off + fl + f] : 0.f;
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
    ups_store<E>(out, ((int64_t)rec.out_off + t) * Cp + c, acc);
  }
}

extern "C" int wae_upsample_stage_fwd_list(const float* in, const float* w, void* out, const wae_ups_seg* segs, int32_t nsegs,
                                           int32_t ntiles, int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s,
                                           int32_t out_btc, int32_t Cp, int32_t dtype, void* stream) {
  WAE_REQUIRE(in && w && out && C > 0 && s > 0, "upsample_stage_fwd_list: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "upsample_stage_fwd_list: a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0, "upsample_stage_fwd_list: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(in_pitch > 0 && out_pitch_or_rows > 0, "upsample_stage_fwd_list: pitches must be > 0 (got %d, %d)", in_pitch,
              out_pitch_or_rows);
  hipStream_t st = as_stream(stream);
  if (!out_btc) {
    if ((C + UPL_CPB - 1) / UPL_CPB > 65535) {
      wae_set_error("upsample_stage_fwd_list: C %d has no list kernel; run wae_upsample_stage_fwd per item", C);
      return WAE_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(ups_stage_list_kernel, dim3(ntiles, (C + UPL_CPB - 1) / UPL_CPB), dim3(256), 0, st, in, w, (float*)out, segs,
                       nsegs, in_pitch, out_pitch_or_rows, C, s);
    return wae_check_launch("upsample_stage_fwd_list");
  }
  WAE_REQUIRE(Cp >= C, "upsample_stage_fwd_list: Cp %d < C %d", Cp, C);
  WAE_REQUIRE(wae_dtype_ok(dtype), "upsample_stage_fwd_list: bad dtype %d", dtype);
  const int nfp = (UPT / s + 5) | 1;         // frames per channel row, odd pitch against bank conflicts (as the dense last stage)
  const size_t lds = ((size_t)Cp * nfp + 2 * s + 1 + 3 * s) * sizeof(float);
  if (Cp > 256 || 256 % Cp != 0 || 3 * s > 256 || lds > 65536) {
    wae_set_error("upsample_stage_fwd_list: the time-major list kernel takes Cp dividing 256, 3 s <= 256 and 64 KiB of LDS "
                  "(got Cp %d, s %d, %zu bytes); run wae_upsample_stage_fwd per item", Cp, s, lds);
    return WAE_EUNSUPPORTED;
  }
  const dim3 grid(ntiles);
  if (dtype == WAE_BF16)
    hipLaunchKernelGGL(ups_last_list_kernel<__bf16>, grid, dim3(256), lds, st, in, w, out, segs, nsegs, in_pitch, out_pitch_or_rows, C,
                       s, Cp, nfp);
  else if (dtype == WAE_F16)
    hipLaunchKernelGGL(ups_last_list_kernel<f16>, grid, dim3(256), lds, st, in, w, out, segs, nsegs, in_pitch, out_pitch_or_rows, C, s,
                       Cp, nfp);
  else
    hipLaunchKernelGGL(ups_last_list_kernel<float>, grid, dim3(256), lds, st, in, w, out, segs, nsegs, in_pitch, out_pitch_or_rows, C,
                       s, Cp, nfp);
  return wae_check_launch("upsample_stage_fwd_list");
}

extern "C" int wae_to_btc_list(const float* in, void* out, const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t in_pitch,
                               int32_t C, int32_t Cp, int32_t dtype, void* stream) {
  WAE_REQUIRE(in && out && C > 0, "to_btc_list: bad arguments");
  WAE_REQUIRE(segs && nsegs > 0, "to_btc_list: a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0 && in_pitch > 0, "to_btc_list: ntiles and in_pitch must be > 0 (got %d, %d)", ntiles, in_pitch);
  WAE_REQUIRE(Cp >= C, "to_btc_list: Cp %d < C %d", Cp, C);
  WAE_REQUIRE(wae_dtype_ok(dtype), "to_btc_list: bad dtype %d", dtype);
  if ((Cp + 63) / 64 > 65535) {
    wae_set_error("to_btc_list: Cp %d has no list kernel; run wae_to_btc per item", Cp);
    return WAE_EUNSUPPORTED;
  }
  const dim3 grid(ntiles, (Cp + 63) / 64);
  hipStream_t st = as_stream(stream);
  if (dtype == WAE_BF16) hipLaunchKernelGGL(to_btc_list_kernel<__bf16>, grid, dim3(256), 0, st, in, out, segs, nsegs, in_pitch, C, Cp);
  else if (dtype == WAE_F16) hipLaunchKernelGGL(to_btc_list_kernel<f16>, grid, dim3(256), 0, st, in, out, segs, nsegs, in_pitch, C, Cp);
  else hipLaunchKernelGGL(to_btc_list_kernel<float>, grid, dim3(256), 0, st, in, out, segs, nsegs, in_pitch, C, Cp);
  return wae_check_launch("to_btc_list");
}

extern "C" int wae_upsample_stage_fwd_ranges(const float* in, const float* w, void* out, const wae_ups_range* recs, int32_t nrecs,
                                             int32_t ntiles, int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s,
                                             int32_t out_btc, int32_t Cp, int32_t dtype, void* stream) {
  WAE_REQUIRE(in && w && out && C > 0 && s > 0, "upsample_stage_fwd_ranges: bad arguments");
  WAE_REQUIRE(recs && nrecs > 0, "upsample_stage_fwd_ranges: a table of nrecs > 0 records and a closing one (got %d)", nrecs);
  WAE_REQUIRE(ntiles > 0, "upsample_stage_fwd_ranges: ntiles must be > 0 (got %d)", ntiles);
  WAE_REQUIRE(in_pitch > 0 && out_pitch_or_rows > 0, "upsample_stage_fwd_ranges: pitches must be > 0 (got %d, %d)", in_pitch,
              out_pitch_or_rows);
  hipStream_t st = as_stream(stream);
  if (!out_btc) {
    if ((C + UPL_CPB - 1) / UPL_CPB > 65535) {
      wae_set_error("upsample_stage_fwd_ranges: C %d has no ranges kernel", C);
      return WAE_EUNSUPPORTED;
    }
    hipLaunchKernelGGL(ups_stage_ranges_kernel, dim3(ntiles, (C + UPL_CPB - 1) / UPL_CPB), dim3(256), 0, st, in, w, (float*)out, recs,
                       nrecs, in_pitch, out_pitch_or_rows, C, s);
    return wae_check_launch("upsample_stage_fwd_ranges");
  }
  WAE_REQUIRE(Cp >= C, "upsample_stage_fwd_ranges: Cp %d < C %d", Cp, C);
  WAE_REQUIRE(wae_dtype_ok(dtype), "upsample_stage_fwd_ranges: bad dtype %d", dtype);
  const int nfp = (UPT / s + 5) | 1;         // as the list's last stage
  const size_t lds = ((size_t)Cp * nfp + 2 * s + 1 + 3 * s) * sizeof(float);
  if (Cp > 256 || 256 % Cp != 0 || 3 * s > 256 || lds > 65536) {
    wae_set_error("upsample_stage_fwd_ranges: the time-major ranges kernel takes Cp dividing 256, 3 s <= 256 and 64 KiB of LDS "
                  "(got Cp %d, s %d, %zu bytes)", Cp, s, lds);
    return WAE_EUNSUPPORTED;
  }
  const dim3 grid(ntiles);
  if (dtype == WAE_BF16)
    hipLaunchKernelGGL(ups_last_ranges_kernel<__bf16>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows,
                       C, s, Cp, nfp);
  else if (dtype == WAE_F16)
    hipLaunchKernelGGL(ups_last_ranges_kernel<f16>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows, C,
                       s, Cp, nfp);
  else
    hipLaunchKernelGGL(ups_last_ranges_kernel<float>, grid, dim3(256), lds, st, in, w, out, recs, nrecs, in_pitch, out_pitch_or_rows,
                       C, s, Cp, nfp);
  return wae_check_launch("upsample_stage_fwd_ranges");
}
