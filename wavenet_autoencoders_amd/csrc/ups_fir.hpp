// The per-output arithmetic of one upsample stage (upsample.py:19-21 nearest stretch + :39-46 shared FIR, zero padded at both ends),
// compiled by the dense kernels (csrc/misc.hip: upsample_stage_kernel, upsample_last_kernel) AND by the list kernels
// (csrc/ups_list.hip): an output of a clip is the same sequence of operations wherever the clip lies, by construction.
// `r` is the clip's channel row indexed by the clip's own frame number, `Tout` the clip's own output length: nothing here knows a
// pitch, a batch or a neighbour.
#pragma once

#define UPT 64      // output steps of one time-major tile (include/wae.h: WAE_UPS_LIST_TILE_BTC)

// tap by tap, every j tested: acc = fmaf(w[j], r[u / s], acc) for j = 0..2s with u = t + j - s inside [0, Tout)
__device__ __forceinline__ float ups_fir_taps(const float* w, const float* r, int t, int s, int Tout) {
  float acc = 0.f;
  for (int j = 0; j <= 2 * s; ++j) {
    const int u = t + j - s;
    if (u >= 0 && u < Tout) acc = fmaf(w[j], r[u / s], acc);
  }
  return acc;
}

// the same taps in the same order, walked with an incremental (u / s, u % s) from the first tap with u >= 0
__device__ __forceinline__ float ups_fir_walk(const float* taps, const float* r, int t, int s, int Tout) {
  float acc = 0.f;
  int j0 = max(0, s - t), u = t + j0 - s;      // first tap with u >= 0
  int q = u / s, rem = u - q * s;
  for (int j = j0; j <= 2 * s && u < Tout; ++j, ++u) {
    acc = fmaf(taps[j], r[q], acc);
    if (++rem == s) { rem = 0; ++q; }
  }
  return acc;
}

// An output step whose 2s + 1 taps all fall inside the clip touches three input frames f - 1, f, f + 1 (f = t / s) with the taps
// summed per frame: A[r] = sum_{j < s - r} w[j], B[r] = the next s taps, C[r] = the rest (r = t % s).  ups_co3_entry(i) is entry i of
// the [3][s] table (i < 3s), summed in tap order; ups_fir_sum3 is the three FMAs.  Valid for s <= t and t + s < Tout OF THE CLIP only.
__device__ __forceinline__ float ups_co3_entry(const float* taps, int i, int s) {
  const int which = i / s, rr = i - which * s;
  const int ja = which == 0 ? 0 : (which == 1 ? s - rr : 2 * s - rr), jb = which == 0 ? s - rr : (which == 1 ? 2 * s - rr : 2 * s + 1);
  float a = 0.f;
  for (int j = ja; j < jb; ++j) a += taps[j];
  return a;
}
__device__ __forceinline__ float ups_fir_sum3(const float* co3, const float* r, int t, int s) {
  const int f = t / s, rr = t - f * s;
  float acc = co3[rr] * r[f - 1];
  acc = fmaf(co3[s + rr], r[f], acc);
  acc = fmaf(co3[2 * s + rr], r[f + 1], acc);
  return acc;
}
