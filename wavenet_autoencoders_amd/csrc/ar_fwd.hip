// wae_ar_generate: autoregressive (sample-by-sample) decoding, the MI355X replacement of
// Conv1d.incremental_forward (conv.py:17-62) + WaveNet.incremental_forward (wavenet.py:218-346).
//
// One persistent workgroup (512 threads) per utterance runs the whole T-step loop on the device: no per-sample
// launches, no per-layer launches.  The reference shifts a (1+(k-1)d, R) buffer by one row per layer per sample
// (an O(d) copy, conv.py:39); here every layer owns a ring of (k-1)d+1 rows in HBM/L2 that is written once and
// read at two fixed lags -- O(1) per sample.  Per layer and sample the work is two matrix-vector products
// (z = W1 [x taps ; c] + zb, [x' ; skip] = W2 u + b) streamed from L2 in a k-blocked, row-interleaved layout
// [k/EPL][row][EPL] so that consecutive lanes read consecutive 16-byte weight packets; the k range is split over
// NS thread slices whose partial sums meet in LDS.  Sampling (argmax / inverse-CDF categorical) is fused.
// Utterances are independent: a batch runs as B workgroups (replicas only; no collective).
#include "wae_common.hpp"

#define AR_THREADS 512

struct ArArgs {
  int dtype, B, T, L, R, G, S, O, Cc, Ccp, Hp, ktaps, mode, Rp;
  float scale;
  const int32_t* dil;
  const int64_t* ring_off;  // L+1 offsets (floats) into one utterance's ring arena
  float* ring;
  int64_t ring_total;
  const char* w_layers;
  int64_t layer_stride;  // bytes
  int64_t w2_off;        // bytes from a layer's base to its second matrix
  const float* bias2;    // (L, R+S)
  const float* zb;       // (B, L, 2Hp)
  const float* first_tab;   // (O, Rp)
  const float* first_bias;  // (Rp)
  const char* w_head;       // [S x S | O x S] blocked
  const float* head_bias;   // [S | O]
  const char* c_up;         // (B, T, Ccp) dtype_c
  int c_dtype;
  const int32_t* inputs;  // (B, T) teacher-forced class ids or null
  int n_forced;           // steps t < n_forced consume inputs[t] / inputs_f[t] (wavenet.py:300-305); 0 without inputs
  int init_idx;
  const float* uniforms;  // (B, T) or null
  int32_t* out_idx;       // (B, T)
  float* out_logits;      // (B, O, T) or null
  // scalar-input decoders (wavenet.py:284-285,325-333): the fed-back quantity is a float, drawn from the mixture of logistics
  int scalar;
  const float* inputs_f;  // (B, T) teacher-forced samples or null
  const float* u_mix;     // (B, T, M) uniforms of the mixture pick, or null (then inputs_f must cover every step)
  const float* u_log;     // (B, T) uniforms of the logistic draw
  float* out_f;           // (B, T) drawn samples, or null
  float log_scale_min;
  int clamp_log_scale;
  // output_distribution of the scalar draw: 0 mixture of logistics (u_mix, u_log), 1 mixture of Gaussians (u_mix, z)
  int dist;
  const float* z;         // (B, T) standard normal draws of the Gaussian (dist 1), or null
  int psum_floats;        // max over the matrix-vector products of slices x padded rows (>= AR_THREADS)
  int t0;                 // absolute index of this launch's first step (wae_ar_desc.t0): the ring holds the rows of steps [0, t0)
};

template <typename E>
__device__ __forceinline__ void load_w(const char* p, float (&w)[ET<E>::EPL]);
template <>
__device__ __forceinline__ void load_w<float>(const char* p, float (&w)[4]) {
  const f32x4 v = *(const f32x4*)p;
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
}
template <>
__device__ __forceinline__ void load_w<__bf16>(const char* p, float (&w)[8]) {
  // bf16 -> fp32 is a 16-bit shift; even elements sit in the low halves of the four dwords
  const f32x4 raw = *(const f32x4*)p;
  const unsigned r[4] = {__float_as_uint(raw.x), __float_as_uint(raw.y), __float_as_uint(raw.z), __float_as_uint(raw.w)};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[2 * i] = __uint_as_float(r[i] << 16);
    w[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u);
  }
}

// y[r] = sum_k W[r][k] v[k] for r < rows; W blocked [k/EPL][rows_pad][EPL]; v in LDS (K padded to EPL, zero filled).
// Threads are laid out as (row = tid % RW, slice = tid / RW); partials go to psum[slice][row] (row pitch rows_pad); caller
// barriers and sums.  More rows than threads (R + S = 1024 at C5): NS = 1 and a thread walks rows tid, tid + RW, ...
template <typename E>
__device__ __forceinline__ void gemv_partial(const char* __restrict__ W, const float* v, float* psum, int rows_pad, int K, int RW,
                                             int NS) {
  constexpr int EPL = ET<E>::EPL;
  const int r0 = threadIdx.x % RW, s = threadIdx.x / RW;
  if (s >= NS) return;
  const int nkb = (K + EPL - 1) / EPL;
  const int per = (nkb + NS - 1) / NS;
  const int kb0 = s * per, kb1 = min(nkb, kb0 + per);
  for (int r = r0; r < rows_pad; r += RW) {
  float acc = 0.f;
  const char* wp = W + ((int64_t)kb0 * rows_pad + r) * 16;
  const int64_t step = (int64_t)rows_pad * 16;
  int kb = kb0;
  for (; kb + 4 <= kb1; kb += 4) {
    float w0[EPL], w1[EPL], w2[EPL], w3[EPL];
    load_w<E>(wp, w0); load_w<E>(wp + step, w1); load_w<E>(wp + 2 * step, w2); load_w<E>(wp + 3 * step, w3);
    wp += 4 * step;
    const float* vv = v + kb * EPL;
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc = fmaf(w0[j], vv[j], acc);
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc = fmaf(w1[j], vv[EPL + j], acc);
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc = fmaf(w2[j], vv[2 * EPL + j], acc);
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc = fmaf(w3[j], vv[3 * EPL + j], acc);
  }
  for (; kb < kb1; ++kb) {
    float w0[EPL];
    load_w<E>(wp, w0);
    wp += step;
#pragma unroll
    for (int j = 0; j < EPL; ++j) acc = fmaf(w0[j], v[kb * EPL + j], acc);
  }
  psum[s * rows_pad + r] = acc;
  }
}

__device__ __forceinline__ float psum_total(const float* psum, int r, int rows_pad, int NS) {
  float a = 0.f;
  for (int s = 0; s < NS; ++s) a += psum[s * rows_pad + r];
  return a;
}

__device__ __forceinline__ void layout_rows(int rows, int& rows_pad, int& RW, int& NS) {
  rows_pad = (rows + 63) & ~63;
  RW = rows_pad > AR_THREADS ? AR_THREADS : rows_pad;
  NS = AR_THREADS / RW;
  if (NS < 1) NS = 1;
}

template <>
__device__ __forceinline__ void load_w<f16>(const char* p, float (&w)[8]) {
  const f16x8 v = *(const f16x8*)p;
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = (float)v[i];
}

// What one utterance adds to the launch's arguments: its ring slot, its zb row, its first step in the per-step operands (c_up,
// inputs, uniforms, out_idx, ...; out_logits holds its (O, T) block at base * O) and its own length, forced prefix and start class.
// ar_kernel decodes utterance blockIdx.x (base = b * T); ar_list_kernel one queue item after another; ar_span_kernel one queue span
// after another, each in its clip's own ring from its own t0.
struct ArUtt {
  float* ring;
  const float* zb;
  int64_t base;
  int T, n_forced, init_idx;
  int t0;   // absolute index of the first step (wae_ar_desc.t0; a span's own): the ring holds the rows of steps [0, t0)
};

// One utterance from its first step to its last, by the whole workgroup.  Every LDS word the steps read is written here first, and a
// ring row is read only behind its write in this very decode (the `tt >= 0` test below; a layer's (k-1)d+1 rows cover exactly the
// steps t-(k-1)d .. t), so a workgroup may run this again and again in the same LDS and the same ring slot.  With ut.t0 > 0 the rows
// behind the first step are those an earlier call left in ut.ring (an earlier launch's: wae_ar_desc.t0, or an earlier span's).
template <typename E>
__device__ __forceinline__ void ar_decode(const ArArgs& p, const ArUtt& ut, float* sm) {
  constexpr int EPL = ET<E>::EPL;
  const int tid = threadIdx.x;
  const int H = p.G / 2;
  const int K1 = p.ktaps * p.R + (p.Cc > 0 ? p.Cc : 0);
  const int K1p = (K1 + EPL - 1) / EPL * EPL;
  const int Hk = (H + EPL - 1) / EPL * EPL;
  const int Sk = (p.S + EPL - 1) / EPL * EPL;
  // LDS carve (floats)
  float* vbuf = sm;                       // K1p
  float* xbuf = vbuf + K1p;               // R
  float* ubuf = xbuf + p.R;               // Hk
  float* skipb = ubuf + Hk;               // Sk   (also the head's h0)
  float* hbuf = skipb + Sk;               // Sk   (h1)
  float* lbuf = hbuf + Sk;                // O    logits
  float* psum = lbuf + ((p.O + 3) & ~3);  // p.psum_floats
  int* ibuf = (int*)(psum + p.psum_floats);     // [0] = current input id

  float* ring = ut.ring;
  const float* zb_b = ut.zb;
  int gp, gRW, gNS, wp_, wRW, wNS, sp_, sRW, sNS, op_, oRW, oNS;
  layout_rows(p.G, gp, gRW, gNS);
  layout_rows(p.R + p.S, wp_, wRW, wNS);
  layout_rows(p.S, sp_, sRW, sNS);
  layout_rows(p.O, op_, oRW, oNS);

  for (int i = tid; i < K1p; i += AR_THREADS) vbuf[i] = 0.f;
  for (int i = tid; i < Hk; i += AR_THREADS) ubuf[i] = 0.f;
  for (int i = tid; i < Sk; i += AR_THREADS) { skipb[i] = 0.f; hbuf[i] = 0.f; }
  float* fcur = (float*)(ibuf + 1);   // scalar input: the current input value
  if (tid == 0) {
    ibuf[0] = (p.inputs && ut.n_forced > 0) ? p.inputs[ut.base] : ut.init_idx;
    fcur[0] = (p.inputs_f && ut.n_forced > 0) ? p.inputs_f[ut.base] : 0.f;     // wavenet.py:284-285: the start value is zero
  }
  __syncthreads();

  for (int t = 0; t < ut.T; ++t) {
    // ---- first conv: one-hot input == column gather (wavenet.py:311); scalar input: w * x + b ----------------
    const int cur = ibuf[0];
    if (cur < 0) {
      // dense feedback (quantize=False, wavenet.py:335-338 skipped): the previous step's probability / logit vector, still in
      // lbuf, is the decoder input -- first_conv on a dense (1, O) row (wavenet.py:311)
      for (int r = tid; r < p.R; r += AR_THREADS) {
        float acc = p.first_bias[r];
        for (int o = 0; o < p.O; ++o) acc = fmaf(p.first_tab[(int64_t)o * p.Rp + r], lbuf[o], acc);
        xbuf[r] = acc;
      }
    } else {
      for (int r = tid; r < p.R; r += AR_THREADS)
        xbuf[r] = p.scalar ? fmaf(p.first_tab[r], fcur[0], p.first_bias[r])
                           : p.first_tab[(int64_t)cur * p.Rp + r] + p.first_bias[r];
    }
    for (int cc = AR_THREADS - 1 - tid; cc < p.Cc; cc += AR_THREADS) {   // local conditioning of this step -> tail of the operand vector
      const int64_t ci = (ut.base + t) * p.Ccp + cc;
      vbuf[p.ktaps * p.R + cc] = p.c_dtype == WAE_BF16 ? (float)((const __bf16*)p.c_up)[ci] : (p.c_dtype == WAE_F16 ? (float)((const f16*)p.c_up)[ci] : ((const float*)p.c_up)[ci]);
    }
    for (int i = tid; i < p.S; i += AR_THREADS) skipb[i] = 0.f;
    __syncthreads();

    for (int l = 0; l < p.L; ++l) {
      const int d = p.dil[l];
      const int64_t roff = p.ring_off[l];
      const int rlen = (p.ktaps - 1) * d + 1;
      float* rl = ring + roff;
      const int ta = ut.t0 + t;                // the step's absolute index: ring rows and the start of the clip count from the first launch
      // ---- assemble [x[t-(k-1)d] .. x[t]] and push x[t] into the layer's ring (conv.py:35-44, O(1)) -------
      for (int i = tid; i < p.ktaps * p.R; i += AR_THREADS) {
        const int tap = i / p.R, ch = i - tap * p.R;
        const int tt = ta - (p.ktaps - 1 - tap) * d;
        float v;
        if (tap == p.ktaps - 1) {
          v = xbuf[ch];
          rl[(int64_t)(ta % rlen) * p.R + ch] = v;
        } else {
          v = tt >= 0 ? rl[(int64_t)(tt % rlen) * p.R + ch] : 0.f;   // zero history before the clip starts
        }
        vbuf[i] = v;
      }
      __syncthreads();
      const char* wl = p.w_layers + (int64_t)l * p.layer_stride;
      gemv_partial<E>(wl, vbuf, psum, gp, K1, gRW, gNS);
      __syncthreads();
      // ---- gate (modules.py:138-154): thread h owns channel h ------------------------------------------------
      for (int hh = tid; hh < H; hh += AR_THREADS) {
        const float* zbl = zb_b + (int64_t)l * 2 * p.Hp;
        const float a = psum_total(psum, hh, gp, gNS) + zbl[hh];
        const float g = psum_total(psum, H + hh, gp, gNS) + zbl[p.Hp + hh];
        ubuf[hh] = tanhf(a) * (1.f / (1.f + expf(-g)));
      }
      __syncthreads();
      gemv_partial<E>(wl + p.w2_off, ubuf, psum, wp_, H, wRW, wNS);
      __syncthreads();
      // ---- residual + skip (modules.py:157-162, wavenet.py:315) ------------------------------------------------
      const float* b2 = p.bias2 + (int64_t)l * (p.R + p.S);
      for (int i = tid; i < p.R + p.S; i += AR_THREADS) {
        const float y = psum_total(psum, i, wp_, wNS) + b2[i];
        if (i < p.R) xbuf[i] = (y + xbuf[i]) * 0.70710678118654752440f;
        else skipb[i - p.R] += y;
      }
      __syncthreads();
    }
    // ---- head (wavenet.py:316-322) ------------------------------------------------------------------------------
    for (int i = tid; i < p.S; i += AR_THREADS) skipb[i] = fmaxf(skipb[i] * p.scale, 0.f);
    __syncthreads();
    gemv_partial<E>(p.w_head, skipb, psum, sp_, p.S, sRW, sNS);
    __syncthreads();
    for (int i = tid; i < p.S; i += AR_THREADS) hbuf[i] = fmaxf(psum_total(psum, i, sp_, sNS) + p.head_bias[i], 0.f);
    __syncthreads();
    gemv_partial<E>(p.w_head + (int64_t)((p.S + EPL - 1) / EPL) * sp_ * 16, hbuf, psum, op_, p.S, oRW, oNS);
    __syncthreads();
    for (int i = tid; i < p.O; i += AR_THREADS) {
      const float y = psum_total(psum, i, op_, oNS) + p.head_bias[p.S + i];
      lbuf[i] = y;
      if (p.out_logits && p.mode != 3) p.out_logits[(ut.base * p.O + (int64_t)i * ut.T) + t] = y;
    }
    __syncthreads();
    if (p.mode == 3) {
      // softmax=True, quantize=False: the probability vector is the step's output and the next step's input
      float mx = -INFINITY, den = 0.f;
      for (int i = 0; i < p.O; ++i) mx = fmaxf(mx, lbuf[i]);
      for (int i = 0; i < p.O; ++i) den += expf(lbuf[i] - mx);
      __syncthreads();
      for (int i = tid; i < p.O; i += AR_THREADS) {
        const float pr = expf(lbuf[i] - mx) / den;
        lbuf[i] = pr;
        if (p.out_logits) p.out_logits[(ut.base * p.O + (int64_t)i * ut.T) + t] = pr;
      }
      __syncthreads();
    }
    // ---- next input: teacher forcing / greedy / categorical draw (wavenet.py:300-338) -------------------------
    if (tid == 0 && p.scalar && p.dist == 0) {
      // sample_from_discretized_mix_logistic (mixture.py:118-156) on caller-supplied uniforms: Gumbel-max mixture pick,
      // logistic draw, clamp to [-1, 1] -- the arithmetic of dmol_sample_kernel (csrc/loss.hip)
      float xs = 0.f;
      if (p.u_mix) {
        const int M = p.O / 3;
        const float* um = p.u_mix + (ut.base + t) * M;
        float best = -INFINITY;
        int arg = 0;
        for (int i = 0; i < M; ++i) {
          const float v = lbuf[i] - logf(-logf(um[i]));
          if (v > best) { best = v; arg = i; }
        }
        const float mu = lbuf[M + arg];
        float ls = lbuf[2 * M + arg];
        if (p.clamp_log_scale) ls = fmaxf(ls, p.log_scale_min);
        const float u = p.u_log[ut.base + t];
        xs = fminf(fmaxf(mu + expf(ls) * (logf(u) - logf(1.f - u)), -1.f), 1.f);
        if (p.out_f) p.out_f[ut.base + t] = xs;
      }
      fcur[0] = (p.inputs_f && t + 1 < ut.n_forced) ? p.inputs_f[ut.base + t + 1] : xs;
    }
    if (tid == 0 && p.scalar && p.dist == 1) {
      // sample_from_mix_gaussian (mixture.py:225-270) on caller-supplied draws: Gumbel-max mixture pick when M > 1, mu + exp(log s) z
      // (log s unclamped, as there), clamp to [-1, 1] -- the arithmetic of mog_sample_kernel (csrc/loss.hip).  O == 2: [mu | log s];
      // otherwise [logit pi | mu | log s] with M = O / 3 (O == 3: one Gaussian, the logit ignored)
      float xs = 0.f;
      if (p.z) {
        const int M = p.O == 2 ? 1 : p.O / 3;
        const int mu0 = p.O == 2 ? 0 : M, ls0 = p.O == 2 ? 1 : 2 * M;
        int arg = 0;
        if (M > 1) {
          const float* um = p.u_mix + (ut.base + t) * M;
          float best = -INFINITY;
          for (int i = 0; i < M; ++i) {
            const float v = lbuf[i] - logf(-logf(um[i]));
            if (v > best) { best = v; arg = i; }
          }
        }
        xs = fminf(fmaxf(lbuf[mu0 + arg] + expf(lbuf[ls0 + arg]) * p.z[ut.base + t], -1.f), 1.f);
        if (p.out_f) p.out_f[ut.base + t] = xs;
      }
      fcur[0] = (p.inputs_f && t + 1 < ut.n_forced) ? p.inputs_f[ut.base + t + 1] : xs;
    }
    if (tid == 0 && !p.scalar) {
      int nxt;
      float mx = -INFINITY;
      int am = 0;
      for (int i = 0; i < p.O; ++i)
        if (lbuf[i] > mx) { mx = lbuf[i]; am = i; }
      int produced = am;
      if (p.mode == 2) {
        // softmax in fp32 (F.softmax), then inverse CDF over a double cumulative sum
        float den = 0.f;
        for (int i = 0; i < p.O; ++i) den += expf(lbuf[i] - mx);
        double tot = 0.0;
        for (int i = 0; i < p.O; ++i) tot += (double)(expf(lbuf[i] - mx) / den);
        const double thr = (double)p.uniforms[ut.base + t] * tot;
        double c = 0.0;
        int cnt = 0;
        for (int i = 0; i < p.O; ++i) {
          c += (double)(expf(lbuf[i] - mx) / den);
          if (c < thr) ++cnt;
        }
        produced = min(cnt, p.O - 1);
      }
      p.out_idx[ut.base + t] = produced;
      if (p.inputs && t + 1 < ut.n_forced) nxt = p.inputs[ut.base + t + 1];
      else nxt = p.mode >= 3 ? -1 : produced;
      ibuf[0] = nxt;
    }
    __syncthreads();
  }
}

template <typename E>
__global__ void __launch_bounds__(AR_THREADS) ar_kernel(ArArgs p) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int b = blockIdx.x;
  const ArUtt ut = {p.ring + (int64_t)b * p.ring_total, p.zb + (int64_t)b * p.L * 2 * p.Hp, (int64_t)b * p.T, p.T, p.n_forced, p.init_idx, p.t0};
  ar_decode<E>(p, ut, sm);
}

// wae_ar_generate_list / wae_ar_generate_scalar_list: n_slots persistent workgroups empty a queue of utterances of any lengths.
// Thread 0 takes the next item index with one returning atomic add on the caller-zeroed counter and hands it to the workgroup through
// LDS; the workgroup decodes that item to its end in its own ring slot (blockIdx.x) and comes back for the next.  No workgroup ever
// waits for another.
struct ArListArgs {
  ArArgs a;
  const wae_ar_item* items;
  int32_t* next;
  int n_items;
  int qword;   // float index of the queue word in dynamic LDS, behind everything ar_decode carves
};

template <typename E>
__global__ void __launch_bounds__(AR_THREADS) ar_list_kernel(ArListArgs q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const ArArgs& p = q.a;
  int* taken = (int*)sm + q.qword;
  float* ring = p.ring + (int64_t)blockIdx.x * p.ring_total;
  for (;;) {
    if (threadIdx.x == 0) *taken = atomicAdd(q.next, 1);
    __syncthreads();
    const int it = *taken;
    if (it >= q.n_items) return;   // the same word for every thread: the workgroup leaves together
    const wae_ar_item w = q.items[it];
    if (w.T > 0) {
      // mode 0 is teacher-forced throughout; a start class outside the table would read beyond first_tab.  A scalar item
      // (wae_ar_generate_scalar_list) takes its forced prefix from inputs_f and has no start class: its start value is 0
      const bool forced = p.scalar ? p.inputs_f != nullptr : p.inputs != nullptr;
      const int nf = !forced ? 0 : (p.mode == 0 ? w.T : min(max(w.n_forced, 0), w.T));
      const ArUtt ut = {ring, p.zb + (int64_t)w.row * p.L * 2 * p.Hp, w.off, w.T, nf, p.scalar ? 0 : min(max(w.init_idx, 0), p.O - 1), p.t0};
      ar_decode<E>(p, ut, sm);
    }
    __syncthreads();               // every thread has read the word before thread 0 writes the next
  }
}

// wae_ar_generate_spans / wae_ar_generate_scalar_spans: the queue of ar_list_kernel over spans -- runs of consecutive steps of clips that
// live longer than a launch.  A span is decoded in ITS CLIP'S ring (p.ring + span.ring), not in a ring of the slot, from its own t0: ring
// rows and the "before the clip starts" test use span.t0 + t (ar_decode, as under wae_ar_desc.t0), the per-step operands are indexed from
// span.off.  Nothing is cleared: a history row is read only behind its own write, by absolute index, in this span or an earlier one.  A
// continuation's first step is forced (its input is the previous span's last output, put at inputs[off] by the caller).
struct ArSpanArgs {
  ArArgs a;
  const wae_ar_span* spans;
  int32_t* next;
  int n_spans;
  int qword;   // as ArListArgs
};

template <typename E>
__global__ void __launch_bounds__(AR_THREADS) ar_span_kernel(ArSpanArgs q) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const ArArgs& p = q.a;
  int* taken = (int*)sm + q.qword;
  for (;;) {
    if (threadIdx.x == 0) *taken = atomicAdd(q.next, 1);
    __syncthreads();
    const int it = *taken;
    if (it >= q.n_spans) return;   // the same word for every thread: the workgroup leaves together
    const wae_ar_span w = q.spans[it];
    if (w.T > 0) {
      const int t0 = max(w.t0, 0);
      const bool forced = p.scalar ? p.inputs_f != nullptr : p.inputs != nullptr;
      int nf = !forced ? 0 : (p.mode == 0 ? w.T : min(max(w.n_forced, 0), w.T));
      if (forced && t0 > 0 && nf < 1) nf = 1;
      const ArUtt ut = {p.ring + w.ring, p.zb + (int64_t)w.row * p.L * 2 * p.Hp, w.off, w.T, nf, p.scalar ? 0 : min(max(w.init_idx, 0), p.O - 1),
                        t0};
      ar_decode<E>(p, ut, sm);
    }
    __syncthreads();               // every thread has read the word before thread 0 writes the next
  }
}

#include "ar_host.hpp"

struct ArList {   // the list entries' own arguments (who: the entry's name); spans: the records of a *_spans entry instead of items
  const wae_ar_item* items;
  int32_t* next;
  int n_items, n_slots;
  const char* who;
  const wae_ar_span* spans;
};

// The operands of one form of the decode; whatever a form does not have stays null / zero.  Class ids: inputs, uniforms, out_idx, and
// out_logits.  A scalar draw: inputs_f, u_mix, u_log (dist 0) or z (dist 1), out_f, and the mixture parameters through out_logits.
struct ArOps {
  const int32_t* inputs;
  const float* uniforms;
  int32_t* out_idx;
  float *out_logits, *out_f;
  const float *inputs_f, *u_mix, *u_log, *z;
  float log_scale_min;
  int clamp_log_scale, dist;
};

static int ar_launch(const wae_ar_desc* d, const ArNet& net, const ArOps& o, void* stream, const ArList* list = nullptr) {
  ArArgs a = {};
  ar_fill_net(a, d, net);
  a.inputs = o.inputs; a.init_idx = d->init_idx; a.n_forced = ar_n_forced(d, o.inputs ? (const void*)o.inputs : (const void*)o.inputs_f);
  a.uniforms = o.uniforms; a.out_idx = o.out_idx; a.out_logits = o.out_logits; a.scalar = d->scalar_input ? 1 : 0;
  a.inputs_f = o.inputs_f; a.u_mix = o.u_mix; a.u_log = o.u_log; a.out_f = o.out_f; a.log_scale_min = o.log_scale_min;
  a.clamp_log_scale = o.clamp_log_scale; a.dist = o.dist; a.z = o.z;
  const int epl = wae_is16(d->dtype) ? 8 : 4;
  const int H = d->G / 2;
  auto ru = [](int x, int m) { return (x + m - 1) / m * m; };
  int psz = AR_THREADS;
  for (int rows : {d->G, d->R + d->S, d->S, d->O}) psz = psz > ru(rows, 64) ? psz : ru(rows, 64);
  a.psum_floats = psz;
  const size_t lds = sizeof(float) * (size_t)(ru(d->ktaps * d->R + (d->Cc > 0 ? d->Cc : 0), epl) + d->R + ru(H, epl) +
                                              2 * ru(d->S, epl) + ru(d->O, 4) + psz + 4);
  hipStream_t st = as_stream(stream);
  if (list && list->spans) {
    const ArSpanArgs q = {a, list->spans, list->next, list->n_items, (int)(lds / sizeof(float))};
    return ar_by_dtype(d->dtype, [&](auto e) {
      AR_LAUNCH(ar_span_kernel<typename decltype(e)::type>, dim3(list->n_slots), dim3(AR_THREADS), lds + 16, st, q, list->who);
    });
  }
  if (list) {
    // the queue word sits behind ar_decode's carve; per-utterance B, T, n_forced and init_idx come from the items
    const ArListArgs q = {a, list->items, list->next, list->n_items, (int)(lds / sizeof(float))};
    return ar_by_dtype(d->dtype, [&](auto e) {
      AR_LAUNCH(ar_list_kernel<typename decltype(e)::type>, dim3(list->n_slots), dim3(AR_THREADS), lds + 16, st, q, list->who);
    });
  }
  return ar_by_dtype(d->dtype, [&](auto e) {
    AR_LAUNCH(ar_kernel<typename decltype(e)::type>, dim3(d->B), dim3(AR_THREADS), lds, st, a, "ar_generate");
  });
}

extern "C" int wae_ar_generate(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                               int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                               const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                               const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                               const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits,
                               void* stream) {
  const char* who = "ar_generate";
  const ArNet net = AR_NET_OF_ARGS;
  AR_TRY(ar_check_net(who, d, net, out_idx != nullptr, true, 0));
  AR_TRY(ar_check_class_ids(who, d, inputs, uniforms, out_logits, 4, false, "wae_ar_generate_scalar"));
  AR_TRY(ar_check_t0(who, d, inputs, false));
  AR_REQUIRE(d->t0 == 0 || d->mode < 3, "a continuation (t0 > 0) cannot resume modes 3 / 4: the vector they feed back stays on chip");
  ArOps o = {};
  o.inputs = inputs; o.uniforms = uniforms; o.out_idx = out_idx; o.out_logits = out_logits; o.log_scale_min = -7.0f;
  return ar_launch(d, net, o, stream);
}

extern "C" int wae_ar_generate_list(const wae_ar_desc* d, int32_t n_items, int32_t n_slots, const wae_ar_item* items, int32_t* next,
                                    const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                                    const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                                    const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                                    const float* head_bias, const void* c_up, int32_t c_dtype, const int32_t* inputs,
                                    const float* uniforms, int32_t* out_idx, float* out_logits, void* stream) {
  const char* who = "ar_generate_list";
  const ArNet net = AR_NET_OF_ARGS;
  AR_TRY(ar_check_net(who, d, net, out_idx != nullptr, false, 0));
  AR_TRY(ar_check_queue(who, items, next, n_items, "n_slots", n_slots, 0));
  AR_TRY(ar_check_class_ids(who, d, inputs, uniforms, out_logits, 2, true, "wae_ar_generate_scalar_list"));
  AR_TRY(ar_check_t0(who, d, inputs, true));
  ArOps o = {};
  o.inputs = inputs; o.uniforms = uniforms; o.out_idx = out_idx; o.out_logits = out_logits; o.log_scale_min = -7.0f;
  const ArList list = {items, next, n_items, n_slots, who, nullptr};
  return ar_launch(d, net, o, stream, &list);
}

// A work list of spans of class-id clips on the one-CU kernel (include/wae.h): wae_ar_generate_list's checks and operands, ar_span_kernel.
extern "C" int wae_ar_generate_spans(const wae_ar_desc* d, int32_t n_spans, int32_t n_slots, const wae_ar_span* spans, int32_t* next,
                                     const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                                     const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                                     const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                                     const float* head_bias, const void* c_up, int32_t c_dtype, const int32_t* inputs,
                                     const float* uniforms, int32_t* out_idx, float* out_logits, void* stream) {
  const char* who = "ar_generate_spans";
  const ArNet net = AR_NET_OF_ARGS;
  AR_TRY(ar_check_net(who, d, net, out_idx != nullptr, false, 0));
  AR_TRY(ar_check_queue(who, spans, next, n_spans, "n_slots", n_slots, 0, "span"));
  AR_TRY(ar_check_class_ids(who, d, inputs, uniforms, out_logits, 2, true, "wae_ar_generate_scalar_spans"));
  AR_TRY(ar_check_span_t0(who, d));
  ArOps o = {};
  o.inputs = inputs; o.uniforms = uniforms; o.out_idx = out_idx; o.out_logits = out_logits; o.log_scale_min = -7.0f;
  const ArList list = {nullptr, next, n_spans, n_slots, who, spans};
  return ar_launch(d, net, o, stream, &list);
}

// the two scalar entries: dist 0 draws from (u_mix, u_log), dist 1 from (u_mix, z)
static int ar_generate_scalar(const char* who, const wae_ar_desc* d, const ArNet& net, int dist, const ArDraw& w, float log_scale_min,
                              int clamp_log_scale, void* stream) {
  AR_TRY(ar_check_net(who, d, net, true, true, 0));
  AR_TRY(ar_check_mixture(who, d, dist, w, false));
  AR_TRY(ar_check_t0(who, d, w.inputs_f, false));
  ArOps o = {};
  o.out_logits = w.out_params; o.inputs_f = w.inputs_f; o.u_mix = w.u_mix; (dist == 0 ? o.u_log : o.z) = w.draws; o.out_f = w.out_samples;
  o.log_scale_min = log_scale_min; o.clamp_log_scale = clamp_log_scale; o.dist = dist;
  return ar_launch(d, net, o, stream);
}

extern "C" int wae_ar_generate_scalar(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                                      int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                                      const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                                      const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                                      const float* inputs_f, const float* u_mix, const float* u_log, float log_scale_min,
                                      int32_t clamp_log_scale, float* out_samples, float* out_params, void* stream) {
  return ar_generate_scalar("ar_generate_scalar", d, AR_NET_OF_ARGS, 0, {inputs_f, u_mix, u_log, out_samples, out_params}, log_scale_min,
                            clamp_log_scale, stream);
}

extern "C" int wae_ar_generate_scalar_mog(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                                          int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                                          const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                                          const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                                          const float* inputs_f, const float* u_mix, const float* z, float log_scale_min,
                                          float* out_samples, float* out_params, void* stream) {
  return ar_generate_scalar("ar_generate_scalar_mog", d, AR_NET_OF_ARGS, 1, {inputs_f, u_mix, z, out_samples, out_params}, log_scale_min, 0,
                            stream);
}

// A work list of scalar-input utterances on the one-CU kernel: ar_list_kernel over scalar items (the same ar_decode as ar_kernel, so an
// item is bit for bit its wae_ar_generate_scalar / _scalar_mog decode).  The entry reads wae_ar_desc.mode: 0 forces every step of every
// item from inputs_f, 2 samples behind item.n_forced forced steps.
extern "C" int wae_ar_generate_scalar_list(const wae_ar_desc* d, int32_t dist, int32_t n_items, int32_t n_slots, const wae_ar_item* items,
                                           int32_t* next, const int32_t* dilations, const int64_t* ring_off, float* ring,
                                           int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                                           const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                                           const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                                           const float* inputs_f, const float* u_mix, const float* draws, float log_scale_min,
                                           int32_t clamp_log_scale, float* out_samples, float* out_params, void* stream) {
  const char* who = "ar_generate_scalar_list";
  const ArNet net = AR_NET_OF_ARGS;
  const ArDraw w = {inputs_f, u_mix, draws, out_samples, out_params};
  AR_TRY(ar_check_net(who, d, net, true, false, 0));
  AR_TRY(ar_check_mixture(who, d, dist, w, true, true));
  AR_TRY(ar_check_queue(who, items, next, n_items, "n_slots", n_slots, 0));
  AR_TRY(ar_check_t0(who, d, inputs_f, true));
  const bool sampled = dist == 0 ? (u_mix && draws) : draws != nullptr;
  ArOps o = {};
  o.out_logits = out_params; o.inputs_f = inputs_f; o.u_mix = sampled ? u_mix : nullptr; (dist == 0 ? o.u_log : o.z) = draws;
  o.out_f = out_samples; o.log_scale_min = log_scale_min; o.clamp_log_scale = dist == 0 ? clamp_log_scale : 0; o.dist = dist;
  const ArList list = {items, next, n_items, n_slots, who, nullptr};
  return ar_launch(d, net, o, stream, &list);
}

// ... and of spans of scalar-input clips: wae_ar_generate_scalar_list's checks and operands, ar_span_kernel.
extern "C" int wae_ar_generate_scalar_spans(const wae_ar_desc* d, int32_t dist, int32_t n_spans, int32_t n_slots, const wae_ar_span* spans,
                                            int32_t* next, const int32_t* dilations, const int64_t* ring_off, float* ring,
                                            int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                                            const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                                            const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                                            const float* inputs_f, const float* u_mix, const float* draws, float log_scale_min,
                                            int32_t clamp_log_scale, float* out_samples, float* out_params, void* stream) {
  const char* who = "ar_generate_scalar_spans";
  const ArNet net = AR_NET_OF_ARGS;
  const ArDraw w = {inputs_f, u_mix, draws, out_samples, out_params};
  AR_TRY(ar_check_net(who, d, net, true, false, 0));
  AR_TRY(ar_check_mixture(who, d, dist, w, true, true));
  AR_TRY(ar_check_queue(who, spans, next, n_spans, "n_slots", n_slots, 0, "span"));
  AR_TRY(ar_check_span_t0(who, d));
  const bool sampled = dist == 0 ? (u_mix && draws) : draws != nullptr;
  ArOps o = {};
  o.out_logits = out_params; o.inputs_f = inputs_f; o.u_mix = sampled ? u_mix : nullptr; (dist == 0 ? o.u_log : o.z) = draws;
  o.out_f = out_samples; o.log_scale_min = log_scale_min; o.clamp_log_scale = dist == 0 ? clamp_log_scale : 0; o.dist = dist;
  const ArList list = {nullptr, next, n_spans, n_slots, who, spans};
  return ar_launch(d, net, o, stream, &list);
}
