// wae_glu_layer_fwd_list: one ResidualConv1dGLU layer over a LIST of utterances of unequal lengths, teacher-forced, inference
// (include/wae.h) -- the list instantiations of the generic fused-layer kernel template (csrc/glu_fwd_kernel.hpp, LIST = true).
//
// A translation unit of its own: it builds beside csrc/glu_fwd.hip, and that file's ISA (obj/glu_fwd.s) holds the dense kernels alone.
// Shapes: bf16 / fp16 on 8 waves (tiles of 256 time columns), fp32 on 4 waves (128 columns); every (NP, NPH) of glu_fwd.hip's
// dispatch_np.  No CG = 2 and no 4-wave 16-bit shape, no z save, no separate convolution operand.  The 16-bit instantiations take
// their operand requests as inline-asm loads retired by counted waits, so they must not spill (a fragment group spilled between its
// request and the wait is saved before it has landed): tests/test_forward_list_cpu.py reads that off the kernels' metadata.
#include "wae_common.hpp"
#include "glu_fwd_kernel.hpp"

template <typename E, int NP, int NPH, bool EXACT>
static int launch_glu_list(GluListArgs a, int ntiles, hipStream_t st) {
  constexpr int NW = sizeof(E) == 2 ? 8 : 4;
  constexpr int CHB = 2 * NPH * 4 * 1024;
  size_t fixed;
  const int nslot = glu_ring_slots(NW, CHB, false, a.Rp, a.Hp, &fixed);
  if (nslot < 2) {
    wae_set_error("glu_fwd_list: needs %zu bytes of LDS: Hp=%d with Rp=%d is not supported", fixed + 2 * CHB, NP * 32, a.Rp);
    return WAE_EUNSUPPORTED;
  }
  a.nslot = nslot;
  const size_t lds = fixed + (size_t)nslot * CHB;
  static WaeLdsCache lds_cache;
  if (int rc = wae_ensure_lds((const void*)glu_fwd_kernel<E, NP, NPH, EXACT, NW, 1, true>, lds_cache, lds, "glu_fwd_list"); rc != WAE_OK)
    return rc;
  hipLaunchKernelGGL((glu_fwd_kernel<E, NP, NPH, EXACT, NW, 1, true>), dim3(ntiles), dim3(NW * 64), lds, st, a);
  return wae_check_launch("glu_fwd_list");
}

template <typename E, bool EXACT>
static int dispatch_np_list(int np, const GluListArgs& a, int ntiles, hipStream_t st) {
  switch (np) {
    // (NP, NPH) as csrc/glu_fwd.hip: dispatch_np -- the packed weights are the same stream
    case 1: return launch_glu_list<E, 1, 1, EXACT>(a, ntiles, st);
    case 2: return launch_glu_list<E, 2, 1, EXACT>(a, ntiles, st);
    case 3: return launch_glu_list<E, 3, 3, EXACT>(a, ntiles, st);
    case 4: return launch_glu_list<E, 4, 4, EXACT>(a, ntiles, st);
    case 6: return launch_glu_list<E, 6, 3, EXACT>(a, ntiles, st);
    case 8: return launch_glu_list<E, 8, 4, EXACT>(a, ntiles, st);
    default:
      wae_set_error("glu_fwd_list: unsupported Hp=%d (Hp/32 must be 1,2,3,4,6 or 8)", np * 32);
      return WAE_EUNSUPPORTED;
  }
}

extern "C" int32_t wae_glu_list_tile(int32_t dtype) {
  WAE_REQUIRE(wae_dtype_ok(dtype), "glu_list_tile: bad dtype %d", dtype);
  return wae_is16(dtype) ? 256 : 128;
}

extern "C" int wae_glu_layer_fwd_list(const wae_glu_desc* d, const wae_glu_seg* segs, int32_t nsegs, int32_t ntiles, int32_t rows,
                                      const void* x_in, void* x_out, const void* c_up, void* u_out, int64_t u_stride, const float* zb,
                                      int64_t zb_stride, const void* w_packed, const float* bias_out, void* stream) {
  int rc = glu_validate_shape(d);
  if (rc != WAE_OK) return rc;
  WAE_REQUIRE(x_in && u_out && zb && w_packed, "glu (list): null pointer argument");
  WAE_REQUIRE(segs && nsegs > 0, "glu (list): a table of nsegs > 0 records and a closing one (got %d)", nsegs);
  WAE_REQUIRE(ntiles > 0 && rows > 0, "glu (list): ntiles and rows must be > 0 (got %d, %d)", ntiles, rows);
  WAE_REQUIRE(u_stride >= d->Hp, "glu (list): u_stride (%lld) < Hp", (long long)u_stride);
  WAE_REQUIRE((d->flags & WAE_GLU_NO_OUT) || (x_out && bias_out), "glu (list): x_out/bias_out null but WAE_GLU_NO_OUT is not set");
  WAE_REQUIRE(d->Ccp == 0 || c_up, "glu (list): Ccp > 0 but c_up is null");
  if (d->flags & WAE_GLU_SAVE_Z) {
    wae_set_error("glu (list): WAE_GLU_SAVE_Z: the list form is inference only (no z save, no dropout operand)");
    return WAE_EUNSUPPORTED;
  }
  GluListArgs a;
  a.x_in = (const char*)x_in; a.x_conv = (const char*)x_in; a.x_out = (char*)x_out; a.c_up = (const char*)c_up; a.u_out = (char*)u_out;
  a.zb = zb; a.z_save = nullptr; a.w = (const char*)w_packed; a.bias_out = bias_out; a.zb_stride = zb_stride; a.u_stride = u_stride;
  a.B = d->B; a.T = 0; a.Rp = d->Rp; a.Ccp = d->Ccp; a.Hp = d->Hp; a.ktaps = d->ktaps; a.dilation = d->dilation;
  a.flags = d->flags & (WAE_GLU_NO_OUT | WAE_GLU_PAIR);
  a.nslot = 0; a.stamps = nullptr;
  a.segs = segs; a.nsegs = nsegs; a.rows = rows;
  hipStream_t st = as_stream(stream);
  if (d->dtype == WAE_BF16) return dispatch_np_list<__bf16, false>(d->Hp / 32, a, ntiles, st);
  if (d->dtype == WAE_F16) return dispatch_np_list<f16, false>(d->Hp / 32, a, ntiles, st);
  return dispatch_np_list<float, true>(d->Hp / 32, a, ntiles, st);
}
