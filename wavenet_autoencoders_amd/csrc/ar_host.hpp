// Host side of the autoregressive decode entries (csrc/ar_fwd.hip, csrc/ar_coop.hip): the network operands as one block, the
// refusals every wae_ar_generate* entry makes before it launches, and the one launch with dynamic LDS.  Host code only.
#pragma once
#include "wae_common.hpp"

// The 15 network arguments every entry takes behind its descriptor (include/wae.h; _lib.py: _AR), in the entries' order.
struct ArNet {
  const int32_t* dilations; const int64_t* ring_off; float* ring; int64_t ring_total;
  const void* w_layers; int64_t layer_stride_bytes, w2_off_bytes;
  const float *bias2, *zb, *first_tab, *first_bias; const void* w_head; const float* head_bias;
  const void* c_up; int32_t c_dtype;
};
// ... built once per entry from its positional arguments, which every entry names alike
#define AR_NET_OF_ARGS \
  ArNet { dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes, bias2, zb, first_tab, first_bias, w_head, head_bias, c_up, c_dtype }

// the fields ArArgs (csrc/ar_fwd.hip) and ArcArgs (csrc/ar_coop.hip) share by name
template <typename A>
static void ar_fill_net(A& a, const wae_ar_desc* d, const ArNet& n) {
  a.dtype = d->dtype; a.B = d->B; a.T = d->T; a.L = d->L; a.R = d->R; a.G = d->G; a.S = d->S; a.O = d->O; a.Cc = d->Cc;
  a.Ccp = d->Ccp; a.Hp = d->Hp; a.ktaps = d->ktaps; a.mode = d->mode; a.Rp = d->Rp; a.scale = d->scale; a.dil = n.dilations;
  a.ring_off = n.ring_off; a.ring = n.ring; a.ring_total = n.ring_total; a.w_layers = (const char*)n.w_layers;
  a.layer_stride = n.layer_stride_bytes; a.w2_off = n.w2_off_bytes; a.bias2 = n.bias2; a.zb = n.zb; a.first_tab = n.first_tab;
  a.first_bias = n.first_bias; a.w_head = (const char*)n.w_head; a.head_bias = n.head_bias; a.c_up = (const char*)n.c_up;
  a.c_dtype = n.c_dtype; a.t0 = d->t0;
}

// steps of this launch that consume the forced inputs (wavenet.py:300-305): all T unless 0 < n_forced < T; none without inputs
static inline int ar_n_forced(const wae_ar_desc* d, const void* forced) {
  return forced ? (d->n_forced > 0 && d->n_forced < d->T ? d->n_forced : d->T) : 0;
}
static inline bool ar_forced_all(const wae_ar_desc* d, const void* forced) { return forced && (d->n_forced <= 0 || d->n_forced >= d->T); }

// How C members share one utterance: hc gate channels and sc skip rows each; NV values per member and exchange.  C >= 1.
struct ArSplit { int hc, sc, NV; };
static inline ArSplit ar_split(const wae_ar_desc* d, int C) {
  const int hc = (d->G / 2 + C - 1) / C, sc = (d->S + C - 1) / C;
  return {hc, sc, hc > sc ? hc : sc};
}

// ---- the refusals: every function takes the entry's name (`who`) and returns WAE_OK or the code it has set the error text for ----------
#define AR_REFUSE(code, cond, fmt, ...)                \
  do {                                                 \
    if (cond) {                                        \
      wae_set_error("%s: " fmt, who, ##__VA_ARGS__);   \
      return code;                                     \
    }                                                  \
  } while (0)
#define AR_REQUIRE(cond, ...) AR_REFUSE(WAE_EINVAL, !(cond), __VA_ARGS__)
#define AR_UNSUPPORTED(cond, ...) AR_REFUSE(WAE_EUNSUPPORTED, cond, __VA_ARGS__)
#define AR_TRY(call) do { if (int rc_ = (call); rc_ != WAE_OK) return rc_; } while (0)

// The network and its sizes.  others: the entry's own required pointers (out_idx, ...), all non-null.  per_launch: B and T come from the
// descriptor (a work list takes them from its items).  cap > 0: the cooperative kernels' limit on R, S and O.  Who says what about
// sizes: the one-CU entries (cap 0) "bad sizes"; wae_ar_generate_coop / _coop_fused / _coop_scalar (per_launch, cap) "bad sizes (R, S, O
// <= cap)" for either fault; wae_ar_generate_coop_list (cap, not per_launch) "R, S and O <= cap (got ...)" over the cap, else "bad sizes".
static int ar_check_net(const char* who, const wae_ar_desc* d, const ArNet& n, bool others, bool per_launch, int cap) {
  AR_REQUIRE(d && n.dilations && n.ring_off && n.ring && n.w_layers && n.bias2 && n.zb && n.first_tab && n.first_bias && n.w_head &&
                 n.head_bias && others, "null pointer argument");
  AR_REQUIRE(wae_dtype_ok(d->dtype), "bad dtype");
  const bool capped = cap <= 0 || (d->R <= cap && d->S <= cap && d->O <= cap);
  if (!per_launch) AR_REQUIRE(capped, "R, S and O <= %d (got %d, %d, %d)", cap, d->R, d->S, d->O);
  const bool sizes = (!per_launch || (d->B > 0 && d->T > 0)) && d->L > 0 && d->R > 0 && d->G > 0 && d->G % 2 == 0 && d->S > 0 && d->O > 0;
  if (cap > 0 && per_launch) AR_REQUIRE(sizes && capped, "bad sizes (R, S, O <= %d)", cap);
  AR_REQUIRE(sizes, "bad sizes");
  AR_REQUIRE(d->Cc <= 0 || n.c_up, "Cc > 0 but c_up is null");
  return WAE_OK;
}

// Class-id decoding: the mode (0 .. max_mode), what it needs, and the start class.  list: a work list (forced prefixes and start classes
// are per item).  scalar_entry: where a scalar-input decoder goes instead.
static int ar_check_class_ids(const char* who, const wae_ar_desc* d, const int32_t* inputs, const float* uniforms, const float* out_logits,
                              int max_mode, bool list, const char* scalar_entry) {
  AR_UNSUPPORTED(list && d->scalar_input, "list decoding covers class-id decoders; scalar-input decoders go through %s", scalar_entry);
  AR_UNSUPPORTED(list && (d->mode == 3 || d->mode == 4), "modes 3 / 4 (dense feedback) are not list-decoded; use wae_ar_generate");
  AR_REQUIRE(d->mode >= 0 && d->mode <= max_mode, "mode must be 0 (logits), 1 (argmax)%s",
             max_mode > 2 ? ", 2 (sample), 3 (feed probabilities back) or 4 (feed logits back)" : " or 2 (sample)");
  AR_REQUIRE(d->mode != 2 || uniforms, "sample mode needs uniforms");
  AR_REQUIRE(d->mode != 0 || (list ? inputs != nullptr : ar_forced_all(d, inputs)), "mode 0 needs inputs for every step");
  AR_REQUIRE(d->mode < 3 || out_logits, "modes 3 / 4 return their vectors through out_logits");
  AR_REQUIRE(!d->scalar_input, "scalar-input decoders go through %s", scalar_entry);
  // the start class indexes the first-conv table: wavenet.py:288 sets class 127, an IndexError there when O <= 127
  AR_REQUIRE(list || inputs || (d->init_idx >= 0 && d->init_idx < d->O), "init_idx %d is not a class (O = %d)", d->init_idx, d->O);
  return WAE_OK;
}

// The operands of a scalar draw.  dist 0: mixture of logistics (u_mix and draws = u_log, together); dist 1: mixture of Gaussians (draws =
// z; u_mix where there is more than one).  moded: the entry reads wae_ar_desc.mode (0 teacher-forced parameters, 2 sample); the one-CU
// entries do not: there a decode samples where it has its draws and is teacher-forced throughout where it has none.  list: a work list
// (always moded; the forced prefix is per item, so mode 0 asks for inputs_f only, and d->T / d->n_forced are not read).
struct ArDraw { const float *inputs_f, *u_mix, *draws; float *out_samples, *out_params; };
static int ar_check_mixture(const char* who, const wae_ar_desc* d, int dist, const ArDraw& w, bool moded, bool list = false) {
  AR_REQUIRE(d->scalar_input, "needs a scalar-input decoder (class ids go through %s)",
             list ? "wae_ar_generate_list / wae_ar_generate_coop_list" : "wae_ar_generate / wae_ar_generate_coop");
  AR_REQUIRE(dist == 0 || dist == 1, "dist must be 0 (mixture of logistics) or 1 (mixture of Gaussians)");
  AR_REQUIRE(dist != 0 || (d->O > 0 && d->O % 3 == 0), "the mixture of logistics has 3M output channels (got %d)", d->O);
  AR_REQUIRE(dist != 1 || d->O == 2 || (d->O > 0 && d->O % 3 == 0), "the mixture of Gaussians has 2 or 3M output channels (got %d)", d->O);
  const char* names = dist == 0 ? "u_mix and u_log" : "z";
  const bool sampled = dist == 0 ? (w.u_mix && w.draws) : w.draws != nullptr;
  AR_REQUIRE(!moded || d->mode == 0 || d->mode == 2, "mode must be 0 (teacher-forced parameters) or 2 (sample)");
  AR_REQUIRE(dist != 0 || !w.u_mix == !w.draws, "u_mix and u_log come together");
  AR_REQUIRE(!moded || d->mode != 2 || sampled, "sample mode needs its draws (%s)", names);
  AR_REQUIRE(dist != 1 || !sampled || d->O <= 3 || w.u_mix, "%d mixtures need the uniforms u_mix", d->O / 3);
  if (list) AR_REQUIRE(d->mode != 0 || w.inputs_f, "mode 0 needs teacher-forced inputs for every step");
  else if (moded) AR_REQUIRE(d->mode != 0 || ar_forced_all(d, w.inputs_f), "mode 0 needs teacher-forced inputs for every step");
  else AR_REQUIRE(sampled || ar_forced_all(d, w.inputs_f), "needs teacher-forced inputs for every step or its draws (%s)", names);
  AR_REQUIRE(!w.out_samples || sampled, "samples need the draws");
  AR_REQUIRE(w.out_samples || w.out_params, "no output requested");
  return WAE_OK;
}

// wae_ar_desc.t0 > 0 (a launch that continues an earlier launch's decode from the caller's ring).  The first step of a continuation is
// forced -- the previous launch's last output comes in as inputs[b][0] -- so a continuation without inputs (n_forced resolving to 0) has
// nothing to start from.  A work list is not continued at all.
static int ar_check_t0(const char* who, const wae_ar_desc* d, const void* forced, bool list) {
  if (list) AR_REQUIRE(d->t0 == 0, "t0 %d: a list decode cannot be continued", d->t0);
  AR_REQUIRE(d->t0 >= 0, "t0 %d is negative", d->t0);
  AR_REQUIRE(d->T <= 0 || d->t0 <= INT32_MAX - d->T, "t0 + T (%d + %d) does not fit int32_t", d->t0, d->T);
  AR_REQUIRE(d->t0 == 0 || forced, "a continuation (t0 > 0) needs inputs: its first step is forced (n_forced >= 1)");
  return WAE_OK;
}

// The queue of a work list.  max_slots > 0: the bound on `slots` (teams, one XCD each).  what: the records' name ("item"; "span" for
// the *_spans entries, whose records are wae_ar_span).
static int ar_check_queue(const char* who, const void* items, const int32_t* next, int n_items, const char* slots_name, int n_slots,
                          int max_slots, const char* what = "item") {
  AR_REQUIRE(items && next, "the %s array and the queue counter are required", what);
  AR_REQUIRE(n_items >= 1, "n_%ss %d < 1", what, n_items);
  if (max_slots > 0) AR_REQUIRE(n_slots >= 1 && n_slots <= max_slots, "%s %d outside 1..%d (one XCD each)", slots_name, n_slots, max_slots);
  else AR_REQUIRE(n_slots >= 1, "%s %d < 1", slots_name, n_slots);
  return WAE_OK;
}

// The cooperative split: the exchange buffers, C members of at most `threads` threads each, and 32-bit ring offsets.  more: the entry
// that takes more than 8 utterances per launch (null for a work list, whose teams the queue check bounds).
static int ar_check_split(const char* who, const wae_ar_desc* d, int C, int cmax, int threads, int64_t ring_total, bool exchange,
                          const char* more) {
  AR_REQUIRE(exchange, "the exchange buffers msg, acc and error are required");
  if (more) AR_REQUIRE(d->B > 0 && d->B <= 8, "1..8 utterances per launch (one XCD each); use %s for more", more);
  AR_REQUIRE(C >= 1 && C <= cmax, "C %d outside 1..%d cooperating workgroups per %s", C, cmax, more ? "utterance" : "team");
  const ArSplit s = ar_split(d, C);
  AR_REQUIRE(2 * s.hc <= threads && s.sc <= threads, "too few workgroups for G=%d, S=%d", d->G, d->S);
  AR_REQUIRE(ring_total < (int64_t)1 << 31, "ring_total %lld does not fit 32-bit offsets", (long long)ring_total);
  return WAE_OK;
}

// The exchange sequence numbers of a work list on cooperative teams run on across a team's items: at most L per step (the x' sums), one
// per step for the skip sum and each of the head's gathers, two messages per item taken or refused -- all below
// (total + n_items + 1) * (L + 4), which must fit 31 bits.  (A scalar draw adds workgroup barriers, not exchanges.)
static int ar_check_sequence(const char* who, const wae_ar_desc* d, int64_t total, int n_items) {
  AR_REQUIRE(total >= 0 && (total + n_items + 1) <= (((int64_t)1 << 31) - 1) / (d->L + 4),
             "%lld steps in %d items on %d layers: the exchange sequence numbers would not fit 31 bits", (long long)total, n_items, d->L);
  return WAE_OK;
}

// A work list of spans (wae_ar_generate_spans and its kin): every record carries its own t0, so the descriptor's stays 0.
static int ar_check_span_t0(const char* who, const wae_ar_desc* d) {
  AR_REQUIRE(d->t0 == 0, "t0 %d: every span carries its own t0; the descriptor's must be 0", d->t0);
  return WAE_OK;
}

// ---- the launch ------------------------------------------------------------------------------------------------------------------------
// Raises the kernel's dynamic-LDS limit where this device has not granted `lds` yet (wae_ensure_lds: one cache per kernel instantiation;
// a refusal is WAE_EHIP), then launches.
template <typename K, typename A>
static int ar_launch_dyn(K kernel, WaeLdsCache& cache, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A& args, const char* who) {
  AR_TRY(wae_ensure_lds((const void*)kernel, cache, lds, who));
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, args);
  return wae_check_launch(who);
}
// `return ar_launch_dyn(...)` with the instantiation's own cache: the static belongs to the enclosing function (template instantiation)
#define AR_LAUNCH(kernel, grid, block, lds, stream, args, who)                   \
  do {                                                                           \
    static WaeLdsCache cache_;                                                   \
    return ar_launch_dyn((kernel), cache_, grid, block, lds, stream, args, who); \
  } while (0)

// One dtype switch: f(ArElem<E>()) with the element type of storage dtype `dtype`.
template <typename E>
struct ArElem { using type = E; };
template <typename F>
static int ar_by_dtype(int dtype, F&& f) {
  return dtype == WAE_BF16 ? f(ArElem<__bf16>()) : dtype == WAE_F16 ? f(ArElem<f16>()) : f(ArElem<float>());
}
