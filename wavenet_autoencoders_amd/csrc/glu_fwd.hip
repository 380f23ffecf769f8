// wae_glu_layer_fwd: one ResidualConv1dGLU layer, fused (reference: modules.py:115-163).
//
//   z[2Hp, t] = zb + W1[2Hp, k*Rp + Ccp] . [x[t-(k-1)d] ; ... ; x[t] ; c[t]]      (GEMM 1, MFMA)
//   u[Hp, t]  = tanh(z_a) * sigmoid(z_b)                                           (registers) -> stored (B,T,*)
//   y[Rp, t]  = b_out + W_out[Rp, Hp] . u                                          (GEMM 2, MFMA; u never leaves
//   x'[t]     = (y + x[t]) * sqrt(.5)                                               the register file)
//
// The skip path (conv1x1_skip, modules.py:157, and `skips += h`, wavenet.py:204-207) is NOT accumulated here:
// every layer stores its gated activation u_l once, and the head kernel contracts all of them in ONE GEMM
//   skips = sum_l (W_skip_l . u_l + b_skip_l) = [W_skip_0 ... W_skip_{L-1}] . [u_0 ; ... ; u_{L-1}] + sum_l b_skip_l
// -- same arithmetic (fp32 accumulation over K = L*Hp inside the MFMA) without L read-modify-write passes over
// a (B,T,S) fp32 buffer: per sample and layer the kernel reads R+Cc and writes R+H elements instead of
// reading R+Cc+2S and writing R+2S.
//
// Work decomposition: one workgroup = NW*32 consecutive time steps of one clip, NW waves, each wave owns 32 time
// columns and ALL channels of its columns, so the gate and the second GEMM need no cross-wave exchange: the 32x32
// accumulator tiles of GEMM 1 (column = time on the lane, rows = channels in the registers) are converted in place
// into the B operand of GEMM 2 (cdna_hip_programming.md section 3, "An accumulator tile as the next MFMA's operand").
// GEMM 1 runs in NPASS passes over the gate channels (pass p = tanh rows and sigmoid rows of channels
// [p*NPH*32, (p+1)*NPH*32)), so only 2*NPH accumulator tiles are live: a wave fits in 256 registers and TWO waves
// share each SIMD -- one wave's DMA issue, operand loads, gate VALU work and store epilogues run under the other's
// MFMAs (measured with s_memtime stamps before this split: at one wave per SIMD the MFMA pipe idled for 2/3 of a
// workgroup's life).  The price is that the activation operand is read NPASS times (L2 hits).
// Weights arrive pre-packed in A-fragment order and are streamed through a double-buffered LDS ring by LDS-DMA,
// shared by the NW waves; the activation (B) operand is read straight from HBM/L2 as 16-byte fragments (time-major
// rows, channels innermost), zero-filled before t=0 (causal pad).  Outputs leave through a wave-private swizzled
// LDS tile so that every global store is a full-row 16-B access.
#include "wae_common.hpp"
#include "glu_fwd_kernel.hpp"

// Diagnostics (tools/stamps_glu.py, tools/time_glu.py) exist only in a `make EXTRA=-DWAE_DEBUG_KNOBS` build: the product
// library has no process-global switches (include/wae.h: every entry is re-entrant; shapes are chosen by descriptor flags).
#ifdef WAE_DEBUG_KNOBS
static unsigned long long* g_stamps = nullptr;
extern "C" void wae_debug_set_stamps(unsigned long long* dev_buf) { g_stamps = dev_buf; }
static int g_glu_slots = 0;  // 0 = as many ring slots as fit (<= 4)
extern "C" void wae_debug_set_glu_slots(int n) { g_glu_slots = n; }
#else
static constexpr unsigned long long* g_stamps = nullptr;
static constexpr int g_glu_slots = 0;
#endif

// waves per workgroup: 8 (one 256-step workgroup per CU) or 4 (two workgroups per CU).  With the XCD-contiguous tile order and
// the tap-interleaved chunk stream the 8-wave shape measures 2-5 % faster at C2 (59.8 vs 61.2 us inference, 67.4 vs 71.1 us
// with z saved; A/B on one box, WAE_GLU_WAVES=4|8); before those two changes the 4-wave shape was the faster one.
// The caller picks the shape per launch with WAE_GLU_WAVES4 in wae_glu_desc.flags (default: 8 waves).

template <typename E, int NP, int NPH, bool EXACT, int NW, int CG>
static int launch_glu_nw(GluArgs a, hipStream_t st) {
  constexpr int CHB = 2 * NPH * 4 * 1024;
  size_t fixed;
  int nslot = glu_ring_slots(NW, CHB, NW == 4 && sizeof(E) == 2 && CG == 1, a.Rp, a.Hp, &fixed);   // 16-bit, NW == 4, CG == 1: two workgroups share a CU
  if (g_glu_slots >= 2 && g_glu_slots < nslot) nslot = g_glu_slots;
  if (nslot < 2) {
    wae_set_error("glu_fwd: needs %zu bytes of LDS: Hp=%d with Rp=%d is not supported", fixed + 2 * CHB, NP * 32, a.Rp);
    return WAE_EUNSUPPORTED;
  }
  a.nslot = nslot;
  const size_t lds = fixed + (size_t)nslot * CHB;
  static WaeLdsCache lds_cache;
  if (int rc = wae_ensure_lds((const void*)glu_fwd_kernel<E, NP, NPH, EXACT, NW, CG>, lds_cache, lds, "glu_fwd"); rc != WAE_OK) return rc;
  const int tiles = (a.T + NW * 32 * CG - 1) / (NW * 32 * CG);
  hipLaunchKernelGGL((glu_fwd_kernel<E, NP, NPH, EXACT, NW, CG>), dim3(a.B * tiles), dim3(NW * 64), lds, st, a);
  return wae_check_launch("glu_fwd");
}

template <typename E, int NP, int NPH, bool EXACT>
static int launch_glu(const GluArgs& a, hipStream_t st) {
  // fp32 (the parity mode) keeps 4 waves with 512 registers each: its operand fragments are twice as many
  if constexpr (sizeof(E) == 2) {
    // WAE_GLU_CG2: 4 waves x 64 columns, one wave per SIMD, every A fragment feeds two MFMAs
    if (a.flags & WAE_GLU_CG2) return launch_glu_nw<E, NP, NPH, EXACT, 4, 2>(a, st);
    // two 4-wave workgroups per CU need a two-slot ring in 80 KiB each; wider layers take the whole CU with 8 waves
    const bool fits4 = 4 * 4096 + (size_t)(a.Rp + 2 * a.Hp) * 4 + 2 * (2 * NPH * 4096) <= 80 * 1024;
    if (!(a.flags & WAE_GLU_WAVES4) || !fits4) return launch_glu_nw<E, NP, NPH, EXACT, 8, 1>(a, st);
  }
  return launch_glu_nw<E, NP, NPH, EXACT, 4, 1>(a, st);
}

template <typename E, bool EXACT>
static int dispatch_np(int np, const GluArgs& a, hipStream_t st) {
  switch (np) {
    // (NP, NPH): gate-channel tiles, tiles per pass -- packing.py: glu_pass_tiles() must agree
    case 1: return launch_glu<E, 1, 1, EXACT>(a, st);
    case 2: return launch_glu<E, 2, 1, EXACT>(a, st);
    case 3: return launch_glu<E, 3, 3, EXACT>(a, st);
    case 4: return launch_glu<E, 4, 4, EXACT>(a, st);   // Hp = 128 (hps/vqwae.json): all 8 gate tiles in ONE pass
    case 6: return launch_glu<E, 6, 3, EXACT>(a, st);
    case 8: return launch_glu<E, 8, 4, EXACT>(a, st);
    default:
      wae_set_error("glu_fwd: unsupported Hp=%d (Hp/32 must be 1,2,3,4,6 or 8)", np * 32);
      return WAE_EUNSUPPORTED;
  }
}

static int glu_validate(const wae_glu_desc* d) {
  WAE_REQUIRE(d != nullptr, "glu: null desc");
  WAE_REQUIRE(d->T > 0, "glu: B,T must be positive");
  return glu_validate_shape(d);
}

extern "C" int64_t wae_glu_packed_bytes(const wae_glu_desc* d) {
  if (glu_validate(d) != WAE_OK) return WAE_EINVAL;
  const int ck = wae_is16(d->dtype) ? 64 : 32;
  const int np = d->Hp / 32, nph = (np == 3 || np == 4) ? np : (np % 2 == 0 ? np / 2 : np);
  const int mt2 = (wae_is16(d->dtype) ? 4 : 2) * nph / np;
  const int64_t chb = (int64_t)2 * nph * 4 * 1024;
  const int64_t nq1 = (int64_t)d->ktaps * (d->Rp / ck) + d->Ccp / ck;
  const int64_t nq2 = (d->Rp / 32) / mt2;
  return ((np / nph) * nq1 + nq2) * chb;
}

extern "C" int wae_glu_layer_fwd_drop(const wae_glu_desc* d, const void* x_in, const void* x_conv, void* x_out, const void* c_up,
                                      void* u_out, int64_t u_stride, const float* zb, int64_t zb_stride, void* z_save,
                                      const void* w_packed, const float* bias_out, void* stream);
extern "C" int wae_glu_layer_fwd(const wae_glu_desc* d, const void* x_in, void* x_out, const void* c_up, void* u_out,
                                 int64_t u_stride, const float* zb, int64_t zb_stride, void* z_save, const void* w_packed,
                                 const float* bias_out, void* stream) {
  return wae_glu_layer_fwd_drop(d, x_in, x_in, x_out, c_up, u_out, u_stride, zb, zb_stride, z_save, w_packed, bias_out, stream);
}

extern "C" int wae_glu_layer_fwd_drop(const wae_glu_desc* d, const void* x_in, const void* x_conv, void* x_out, const void* c_up,
                                      void* u_out, int64_t u_stride, const float* zb, int64_t zb_stride, void* z_save,
                                      const void* w_packed, const float* bias_out, void* stream) {
  int rc = glu_validate(d);
  if (rc != WAE_OK) return rc;
  WAE_REQUIRE(x_in && x_conv && u_out && zb && w_packed, "glu: null pointer argument");
  WAE_REQUIRE(u_stride >= d->Hp, "glu: u_stride (%lld) < Hp", (long long)u_stride);
  WAE_REQUIRE((d->flags & WAE_GLU_NO_OUT) || (x_out && bias_out), "glu: x_out/bias_out null but WAE_GLU_NO_OUT is not set");
  WAE_REQUIRE(d->Ccp == 0 || c_up, "glu: Ccp > 0 but c_up is null");
  WAE_REQUIRE(!(d->flags & WAE_GLU_SAVE_Z) || z_save, "glu: WAE_GLU_SAVE_Z without z_save");
  GluArgs a;
  a.x_in = (const char*)x_in; a.x_conv = (const char*)x_conv; a.x_out = (char*)x_out; a.c_up = (const char*)c_up; a.u_out = (char*)u_out; a.zb = zb;
  a.z_save = (char*)z_save; a.w = (const char*)w_packed; a.bias_out = bias_out; a.zb_stride = zb_stride;
  a.u_stride = u_stride; a.B = d->B; a.T = d->T; a.Rp = d->Rp; a.Ccp = d->Ccp; a.Hp = d->Hp; a.ktaps = d->ktaps;
  a.dilation = d->dilation; a.flags = d->flags; a.stamps = g_stamps;
  hipStream_t st = as_stream(stream);
#ifndef WAE_GLU_ABLATE
  // the benchmarked 16-bit geometries run on their static-schedule instantiations (glu_fwd_static.hip; bit-identical results);
  // the shape flags and WAE_GLU_GENERIC select this file's kernel
  if (!(d->flags & (WAE_GLU_GENERIC | WAE_GLU_CG2 | WAE_GLU_WAVES4))) {
    bool handled = false;
    rc = wae_glu_static_launch(a, d->dtype, st, &handled);
    if (handled || rc != WAE_OK) return rc;
  }
#endif
  if (d->dtype == WAE_BF16) return dispatch_np<__bf16, false>(d->Hp / 32, a, st);
  if (d->dtype == WAE_F16) return dispatch_np<f16, false>(d->Hp / 32, a, st);
  return dispatch_np<float, true>(d->Hp / 32, a, st);
}
