/*
 * wae.h -- C ABI of libwae_hip.so: the MI355X (gfx950) kernels behind the WaveNet-autoencoder hot path.
 *
 * The reference (MingjieChen/wavenet_autoencoders) has no FFI: its hot path is plain PyTorch modules.
 * Each entry point below replaces the ATen op sequence of the cited reference lines; the Python host
 * (wavenet_autoencoders_amd/) mirrors the reference's module API and binds these with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless the name ends in _host
 *   - nothing here allocates, frees, synchronises or owns memory; kernels are enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream)
 *   - returns WAE_OK (0) or a negative error code; wae_last_error() gives a thread-local message
 *   - dtype: WAE_F32 (fp32 storage, exact-fp32 MFMA 32x32x2), WAE_BF16 (bf16 storage, MFMA 32x32x16, fp32 accumulate) or
 *     WAE_F16 (fp16 storage, MFMA 32x32x16 f16, fp32 accumulate; same packing as bf16; backward on loss-scaled gradients:
 *     the caller folds the scale into inv_count / ext_dy and 1/scale into the alpha of the weight-gradient tables).
 *     Skip accumulators, biases, losses and the encoder/VQ are always fp32.
 *   - activation layout inside the decoder stack is time-major rows, channels innermost:
 *     x[b][t][Cp] with Cp = channels padded to a multiple of 128 (64 for c; pad channels are zero).  The
 *     reference's (B,C,T) tensors enter/leave through wae_to_btc / wae_from_btc, the first-conv gather
 *     and the head (which writes (B,O,T) logits).
 *   - packed weights are in MFMA A-fragment order produced by wae_pack_gather from index maps the host
 *     builds once (wavenet_autoencoders_amd/packing.py documents the order).
 */
#ifndef WAE_H
#define WAE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAE_OK 0
#define WAE_EINVAL (-1)
#define WAE_EUNSUPPORTED (-2)
#define WAE_EHIP (-3)

#define WAE_F32 0
#define WAE_BF16 1
#define WAE_F16 2   /* fp16 storage, MFMA 32x32x16 f16, fp32 accumulate (BASELINE config C5); same packing as WAE_BF16 */

/* flags of wae_glu_desc.flags */
#define WAE_GLU_SAVE_Z 2    /* also store the pre-activation z (B,T,2Hp) for backward */
#define WAE_GLU_NO_OUT 4    /* do not compute/store x' (last layer: the reference's x' is dead, wavenet.py:205-207) */
#define WAE_GLU_CG2 16      /* 16-bit dtypes: 4 waves x 64 time columns (one wave per SIMD), every weight fragment read from LDS feeds
                               two MFMAs -- half the LDS read traffic of the default shape; same results bit for bit */
#define WAE_GLU_PAIR 32     /* GEMM 1 meets at a workgroup barrier on every SECOND weight chunk (four ring slots, weights two chunks ahead): the
                               waves of a SIMD drift by up to one chunk, so one wave's chunk bookkeeping runs under the other's MFMAs;
                               same results bit for bit */
#define WAE_GLU_WAVES4 8    /* bf16: 128-step tiles, 4 waves, two workgroups per CU instead of one 256-step / 8-wave workgroup
                               (same results bit for bit; an A/B switch per launch, not process state) */
#define WAE_GLU_GENERIC 64   /* 16-bit dtypes: run the run-time-scheduled kernel (csrc/glu_fwd.hip) even where a static-schedule
                               instantiation (csrc/glu_fwd_static.hip) exists for the geometry; same results bit for bit */

const char* wae_version(void);
const char* wae_last_error(void);

/* ---- K14 weight norm (modules.py:18, upsample.py:44): w = g * v / ||v|| per output row --------------
 * Parameters live in one flat fp32 arena.  eff <- copy of params, then for every weight-normed row r:
 * eff[v_off[r] .. +cols[r]) = params[g_off[r]] * v / ||v||.  Tables are int64 device arrays of nrows, rows SORTED by v_off and
 * not overlapping (the kernels copy what lies between consecutive rows through instead of copying the whole arena first). */
int wae_weight_norm_fwd(const float* params, float* eff, int64_t n_params, const int64_t* v_off,
                        const int64_t* g_off, const int32_t* cols, int32_t nrows, void* stream);
/* backward: given d_eff (grad wrt effective weights, same layout) accumulate into grads:
 * grads[v] = g/||v|| * (dw - v * (dw.v)/||v||^2), grads[g] = (dw.v)/||v||; every other slot: grads = d_eff. */
int wae_weight_norm_bwd(const float* params, const float* d_eff, float* grads, int64_t n_params,
                        const int64_t* v_off, const int64_t* g_off, const int32_t* cols, int32_t nrows,
                        void* stream);
/* the same over the arena slice [lo, hi) and the weight-normed rows [row_lo, row_hi) that lie inside it: data-parallel
 * training hands the decoder layers' gradients to the all-reduce while the front end's backward is still running
 * (replaces the one-shot gather / reduce of vqwae_train.py:698-706) */
int wae_weight_norm_bwd_range(const float* params, const float* d_eff, float* grads, int64_t lo, int64_t hi,
                              const int64_t* v_off, const int64_t* g_off, const int32_t* cols, int32_t row_lo,
                              int32_t row_hi, void* stream);

/* dst[i + b*dst_stride] = (dtype) (map[i] < 0 ? 0 : src[map[i] + b*src_stride]),  i < n, b < nbatch */
int wae_pack_gather(const float* src, const int32_t* map, void* dst, int64_t n, int32_t nbatch,
                    int64_t src_stride, int64_t dst_stride, int32_t dtype, void* stream);
/* inverse (gradients): dst[map[i] + b*dst_stride] += src[s(i) + b*src_stride] (fp32 atomics; several i may share a
 * slot unless unique == 1, which promises one source per slot and uses plain adds); s(i) = i, or with src_cols > 0 the
 * element (i / src_cols, i % src_cols) of a row-major tile of pitch src_ld.  unique == 2: every row of the tile feeds the
 * one slot map[row * src_cols] (bias gradients from the per-clip ones columns): the row is summed and added once. */
int wae_unpack_scatter_add(const float* src, const int32_t* map, float* dst, int64_t n, int32_t nbatch,
                           int64_t src_stride, int64_t dst_stride, int32_t src_cols, int64_t src_ld, int32_t unique,
                           void* stream);

/* Several of either in ONE launch (a train step packs / scatters eleven families; the reference holds weights in one layout and
 * needs neither).  jobs_host: HOST array of at most WAE_MULTI_MAX jobs, copied into the kernel arguments; the fields mean what
 * the arguments of the single-job entries mean.  The scatter jobs of one call must write disjoint slots when unique != 0.
 * A gather job with map == NULL is a FILL: n fp32 zeros at dst (16-byte aligned; src / strides / nbatch unused) -- the backward's two
 * gradient accumulators are cleared by the launch that packs its weights (round 6). */
#define WAE_MULTI_MAX 16
typedef struct wae_gather_job {
  const float* src;
  const int32_t* map;
  void* dst;
  int64_t n, src_stride, dst_stride;
  int32_t nbatch, dtype;
} wae_gather_job;
typedef struct wae_scatter_job {
  const float* src;
  const int32_t* map;
  float* dst;
  int64_t n, src_stride, dst_stride, src_ld;
  int32_t nbatch, src_cols, unique, pad_;
} wae_scatter_job;
int wae_pack_gather_multi(const wae_gather_job* jobs_host, int32_t njobs, void* stream);
int wae_unpack_scatter_add_multi(const wae_scatter_job* jobs_host, int32_t njobs, void* stream);

/* ---- a1 encoder block (vqvae_model.py:17-23): y = relu(conv1d(x,w,b,stride,pad=k/2)) (+x) ; fp32 (B,C,T)
 * relu/residual/pad selectable so the same entry serves Encoder.lin (vqvae_model.py:50, k=1) and the
 * upsample net's conv_in (upsample.py:77-78: k = 2*cin_pad+1, pad 0, no bias).  Tout = (Tin+2*pad-k)/stride+1 */
int wae_enc_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t Cin,
                     int32_t Tin, int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu,
                     int32_t residual, void* stream);

/* ---- a1 over a LIST of utterances of unequal lengths (vqvae_model.py:17-23,48-51: the same block and Encoder.forward's chain of
 * blocks + lin, for every utterance of a list in one launch per layer).  The reference encodes one dense (B,C,T) batch; zero-padding
 * unequal utterances to a common length is NOT the same function (behind the first block bias + ReLU make the pad frames non-zero and
 * the next k = 3 / k = 5 block reads them into the last valid frames), so a list is otherwise a loop of batch-1 calls.
 * Packed layout: an activation of the list is channel-major and packed along time -- x (Cin, in_pitch) fp32, utterance i owning the
 * columns [in_off_i, in_off_i + Tin_i); y (Cout, out_pitch) with out_off_i and Tout_i = (Tin_i + 2*pad - k)/stride + 1.  Every
 * utterance is zero-padded at its own two ends: a tap outside [0, Tin_i) reads 0, never the neighbour's column.
 * Tables (DEVICE arrays the host builds -- packing.encode_list_plan; nothing here allocates or synchronises): segs, nsegs records
 * wae_seg; tiles, ntiles pairs (segment, to0): the workgroup (tile, channel block) computes outputs [to0, to0 + et) of that segment
 * for 32 output channels.  The tiles of a segment start at multiples of et and cover [0, Tout_i) once.  Grid (ntiles, ceil(Cout/32)).
 * et: 8, 16 or 32, the tile length the table was built for; the result does not depend on it.
 * Every utterance's columns are, bit for bit, what wae_enc_conv_fwd writes for that utterance alone (B = 1): the value of an output
 * is the same fixed sequence of fmaf and adds in both kernels (csrc/enc_list.hip), whatever else is in the list.  residual reads x at
 * (oc, in_off_i + ot).  Columns of y that no segment owns are not written.
 * Returns WAE_EINVAL for null x / w / y / segs / tiles, sizes < 1, nsegs or ntiles < 1, et outside {8, 16, 32}, a pitch < 1, or
 * residual on a conv that is not same-shape (stride 1, Cin == Cout, 2*pad == k-1), as wae_enc_conv_fwd; WAE_EUNSUPPORTED for a
 * (k, stride) other than (1,1), (3,1), (5,2), (5,1) -- the caller then loops wae_enc_conv_fwd.  A tile whose record does not fit the
 * pitches, names no segment or contradicts the Tout formula is skipped by the kernel: nothing is read or written for it.
 * The quantiser needs no list entry: wae_vq_nearest / wae_vq_slice with B = 1, Dtot = Cc, Tq = sum of Tq_i on the packed latents
 * (Cc, sum Tq_i) -- the row of (b = 0, t) is the packed column t; idx and quant are per row (so per utterance, bit for bit the
 * batch-1 call's), stats are the LIST's aggregate loss and perplexity; per utterance, and for the list in a fixed order, they come
 * from wae_vq_stats_segments below. */
typedef struct wae_seg { int32_t in_off, Tin, out_off, Tout; } wae_seg;
int wae_enc_conv_fwd_list(const float* x, const float* w, const float* bias, float* y, const wae_seg* segs, int32_t nsegs,
                          const int32_t* tiles, int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin,
                          int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu, int32_t residual, void* stream);

/* ---- a1 over COLUMN RANGES of utterances that are still growing (an encode session's open clips: EncodeSession.open / feed / end).
 * wae_enc_conv_fwd_list computes every output of every utterance; this entry computes the outputs [t_lo, t_hi) of every record, from
 * the input columns that are valid NOW.  Output t of a block (k, stride s, pad p = k/2) reads the inputs t s - p .. t s - p + k - 1
 * and nothing else, so with n input columns of a clip final, the outputs t <= (n - k + p) / s -- floor((n - k + p) / s) + 1 of them, 0
 * where n - k + p < 0 -- are final whatever arrives later: none of their taps reaches column n.  Once the clip has ended, all
 * (n + 2p - k) / s + 1 outputs are final, the taps at or beyond n being the clip's own zero padding.  Through ENCODER_BLOCKS and lin,
 * F feature frames make max(0, (F - 13) / 4) latent frames final while the clip is open and (F + 3) / 4 once it has ended.  The kernel
 * carries no "open" flag; the HOST guarantees t_hi <= the open count while a clip is open and t_hi <= Tout once it has ended
 * (packing.enc_feed_plan).  Inside that bound no tap of an open clip reaches Tin, and a tap outside [0, Tin) reads 0.
 * Record wae_enc_range {in_off, Tin, out_col, t_lo, t_hi, tile0}: in_off, Tin -- the clip's input columns [in_off, in_off + Tin) of
 * x (Cin, in_pitch) fp32 that are valid now; t_lo, t_hi -- the outputs to compute, in the clip's own numbering; out_col -- the column
 * of y (Cout, out_pitch) that receives t_lo (a per-clip arena: base + t_lo; a packed buffer of this call's new columns: its running
 * offset); tile0 -- the index of the record's first tile.  nrecs records and ONE closing record whose tile0 is the tile count, a
 * DEVICE array.  Tile j of a record is the outputs [t_lo + j et, min(t_lo + (j + 1) et, t_hi)); a workgroup finds its record by the
 * workgroup-uniform binary search of the upsampling list kernels.  Grid (ntiles, ceil(Cout/32)); et: 8, 16 or 32.
 * Every output is, bit for bit, what wae_enc_conv_fwd writes for the whole clip (B = 1): the value of an output is the same fixed
 * sequence of fmaf and adds (csrc/enc_list.hip: one kernel template, which the list entry launches too), and nothing in it depends on the tile's
 * origin or length.  residual reads x at (oc, in_off + ot).  Columns of y outside every range are not written.
 * The kernel does not trust the table with memory: a record with Tin < 1, t_lo < 0, t_lo >= t_hi, t_hi > (Tin + 2 pad - k) / stride + 1,
 * a tile count other than ceil((t_hi - t_lo) / et), in_off < 0, in_off + Tin > in_pitch, out_col < 0 or out_col + (t_hi - t_lo) >
 * out_pitch is skipped as a whole, nothing read or written for it.  Returns WAE_EINVAL / WAE_EUNSUPPORTED exactly where
 * wae_enc_conv_fwd_list does, before any launch; nothing allocates or synchronises. */
typedef struct wae_enc_range { int32_t in_off, Tin, out_col, t_lo, t_hi, tile0; } wae_enc_range;
int wae_enc_conv_fwd_ranges(const float* x, const float* w, const float* bias, float* y, const wae_enc_range* recs, int32_t nrecs,
                            int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin, int32_t Cout, int32_t k,
                            int32_t stride, int32_t pad, int32_t relu, int32_t residual, void* stream);

/* ---- a1 over column ranges of utterances that live in RINGS (a windowed encode session: EncodeSession(window=W)).
 * The ring-addressed twin of wae_enc_conv_fwd_ranges: the same ranges, the same guarantee asked of the host, the same bits.  What
 * differs is where a column lies.  Record wae_enc_ring {in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0}:
 * Tin -- as in wae_enc_range, the clip's input columns that are valid now, in the clip's own numbering; only the last in_period of
 * them are held, column u at in_off + u % in_period of x (Cin, in_pitch).  A tap with u < 0 or u >= Tin is the clip's zero padding.
 * Output t goes to column out_off + t % out_period of y (Cout, out_pitch); out_period == 0 means a linear output, out_off
 * receiving t_lo (a packed buffer of this call's new columns).  t_lo, t_hi, tile0, the closing record, the binary search, the grid
 * and et are wae_enc_conv_fwd_ranges'.  The ring is mapped where a tile's input window is staged, at the residual read and at the
 * store, and nowhere in the arithmetic: every output is, bit for bit, what wae_enc_conv_fwd writes for the whole clip (B = 1),
 * whatever the periods (csrc/enc_ring.hip).
 * The kernel does not trust the table with memory: it is skipped as a whole, nothing read or written for it, a record that
 * wae_enc_conv_fwd_ranges would skip for its Tin, t_lo, t_hi or tile count, and one with in_period < 1, in_off < 0,
 * in_off + in_period > in_pitch, out_period < 0, out_off < 0, out_off + out_period (out_period == 0: out_off + (t_hi - t_lo)) >
 * out_pitch, t_hi - t_lo > out_period > 0, or -- aliasing -- a first tap t_lo * stride - pad older than Tin - in_period: that column is
 * gone and its slot holds a newer one.  Returns WAE_EINVAL / WAE_EUNSUPPORTED exactly where wae_enc_conv_fwd_ranges does,
 * before any launch; nothing allocates or synchronises. */
typedef struct wae_enc_ring { int32_t in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0; } wae_enc_ring;
int wae_enc_conv_fwd_rings(const float* x, const float* w, const float* bias, float* y, const wae_enc_ring* recs, int32_t nrecs,
                           int32_t ntiles, int32_t et, int32_t in_pitch, int32_t out_pitch, int32_t Cin, int32_t Cout, int32_t k,
                           int32_t stride, int32_t pad, int32_t relu, int32_t residual, void* stream);

/* ---- a2 VectorQuantize.forward (vector_quantization.py:21-49) -----------------------------------------
 * lat (B,D,Tq) fp32, emb (K,D).  idx int64 (B*Tq) first-minimum of ||e||^2+||x||^2-2x.e; quant (B,D,Tq);
 * stats[0] = vq_loss = (beta+1)*mean((q-x)^2) forward value, stats[1] = perplexity; hist: (K+1) int32 scratch. */
int wae_vq_nearest(const float* lat, const float* emb, int64_t* idx, float* quant, float* stats, int32_t* hist,
                   int32_t B, int32_t D, int32_t Tq, int32_t K, float beta, void* stream);

/* ---- section 8(f) rank 3: the sliced / EMA quantizers (vector_quantization.py:51-128, :132-235, :239-306) -----------
 * wae_vq_slice: the search above on channels [d0, d0+D) of a (B,Dtot,Tq) tensor against that slice's own codebook
 * emb (K,D); quant is the (B,Dtot,Tq) output (only the slice is written).  mode 0: search + gather (:84-110),
 * 1: search only (idx, hist, stats[1]), 2: gather with the idx given (the EMA classes gather from the codebook AFTER
 * its update, :217-218,:292).  stats[0] = c_loss * mean((q-x)^2) over the slice, stats[1] = slice perplexity
 * (the sliced classes ADD the slice perplexities, :125-127).  hist: (K+1) int32 scratch; its K counts feed
 * wae_vq_ema_update.
 * wae_vq_ema_update (training branch, :190-215 / :275-290): cluster_size = decay*cluster_size + (1-decay)*counts,
 * Laplace smoothing (+1e-5, K*1e-5), ema_w = decay*ema_w + (1-decay)*sum of the latents assigned to each code,
 * emb = ema_w / cluster_size.  All three buffers are updated in place.
 * wae_vq_slice_bwd: dlat = dquant + c_lat*(x-q); demb[idx] += c_emb*(q-x) (demb NULL for EMA codebooks). */
int wae_vq_slice(const float* lat, const float* emb, int64_t* idx, float* quant, float* stats, int32_t* hist, int32_t B,
                 int32_t Dtot, int32_t d0, int32_t D, int32_t Tq, int32_t K, float c_loss, int32_t mode, void* stream);
int wae_vq_ema_update(const float* lat, const int64_t* idx, const int32_t* hist, float* ema_cluster_size, float* ema_w,
                      float* emb, int32_t B, int32_t Dtot, int32_t d0, int32_t D, int32_t Tq, int32_t K, float decay,
                      void* stream);
int wae_vq_slice_bwd(const float* lat, const float* quant, const int64_t* idx, const float* dquant, float* dlat,
                     float* demb, int32_t B, int32_t Dtot, int32_t d0, int32_t D, int32_t Tq, float c_lat, float c_emb,
                     void* stream);

/* ---- every slice of a sliced quantiser in ONE search launch (csrc/misc.hip) -----------------------------------------
 * wae_vq_search_slices: wae_vq_slice for nslices slices of one (B,Dtot,Tq) tensor at once.  recs_host: a HOST array of nslices
 * records {emb (K,D) device pointer, d0, D, K, c_loss}; they travel as a kernel argument by value -- no table upload, no
 * allocation, no synchronisation.  Per slice s the semantics are exactly wae_vq_slice's: mode 0 search + gather, 1 search only,
 * 2 gather from the idx given; first minimum wins; stats[s] = {c_loss_s * mean((q-x)^2) over the slice, slice perplexity}.
 * idx: (nslices, B*Tq) int64, row s the slice's indices; quant: (B,Dtot,Tq), channels no slice covers are not written (may be NULL in
 * mode 1); stats: (nslices, 2).  scratch: wae_vq_search_slices_scratch(recs, nslices) = sum K_s + nslices int32 entries -- the slices'
 * counts back to back (slice s at offset sum of K_r, r < s: the `hist` wae_vq_ema_update reads), then nslices float cells of squared
 * error.  A call is ONE memset (mode 2: the float cells only, the counts stay), ONE search launch on a (B*Tq, nslices) grid and ONE
 * statistics launch, whatever nslices is.
 * idx, quant, the counts and stats[s][1] are bit for bit what wae_vq_slice gives for slice s alone (the two kernels share the
 * per-vector function); stats[s][0] is the same sum of float atomics in arrival order, so not bitwise: wae_vq_loss_det per slice
 * makes it reproducible.
 * WAE_EINVAL before any launch: a null lat / recs / idx / stats / scratch / emb, quant null outside mode 1, nslices outside
 * 1..WAE_VQ_MAX_SLICES, a slice with D < 1, K < 1 or not inside [0, Dtot), two slices that overlap, a mode outside 0..2, B, Dtot
 * or Tq < 1.  WAE_EUNSUPPORTED: a slice wider than 15872 channels (LDS).  The scratch query returns WAE_EINVAL for the same record
 * errors (it does not know Dtot or the pointers). */
#define WAE_VQ_MAX_SLICES 8
typedef struct wae_vq_slice_rec { const float* emb; int32_t d0, D, K; float c_loss; } wae_vq_slice_rec;
int64_t wae_vq_search_slices_scratch(const wae_vq_slice_rec* recs_host, int32_t nslices);
int wae_vq_search_slices(const float* lat, const wae_vq_slice_rec* recs_host, int32_t nslices, int64_t* idx, float* quant,
                         float* stats, int32_t* scratch, int32_t B, int32_t Dtot, int32_t Tq, int32_t mode, void* stream);

/* ---- the quantiser's statistics of a packed list, per utterance and for the list as one batch (vector_quantization.py:41-47 for
 * every item as a batch of one; csrc/vq_list.hip).  wae_vq_nearest on the packed latents of a list (B = 1, Tq = pitch) gives idx and
 * quant per frame; its stats are the aggregate of whatever was packed, and its squared error a chain of float atomics in arrival order.
 * lat, quant: channel-major (D, pitch) fp32; idx: (pitch) int64; segs: a device array of nsegs records wae_vq_seg {q_off, Tq}, item
 * i owning the columns [q_off, q_off + Tq).  Written for this call's items, entries first .. first + nsegs - 1 of the list's arrays:
 *   hist[i] (K int32): the counts of the item's idx -- LDS integer atomics, exact; an idx outside [0, K) is counted nowhere;
 *   sqerr[i]: sum over the item's columns and every d < D of (quant - lat)^2, each difference and the sum in fp64 in a fixed order
 *     (thread j of 256 takes the columns j, j + 256, ..., the channels of a column in turn; a xor butterfly over the 64 lanes, the
 *     four waves in wave order), rounded to fp32 once;
 *   item_stats[i] (2 floats): [0] = c_loss * (sqerr[i] / ((float)Tq * (float)D)), the item's vq_loss for c_loss = beta + 1;
 *     [1] = the perplexity of the item's counts, bit for bit the stats[1] of the search entry above, mode 1, on the item alone.
 * out (4 floats), over the entries [0, first + nsegs) in list order: [0] = c_loss * sum sqerr / (D * sum Tq), [1] = the perplexity of
 * the counts added per code with N = sum Tq (what the dense search reports for the packed latents as one clip), [2] = sum Tq,
 * [3] = sum sqerr; the sums of sqerr in fp64.  Tq of an entry is read back as the sum of its counts (the entry keeps no array of
 * them between groups: equal to Tq for indices inside the codebook); all four are 0 when no entry has a frame.
 * Deterministic: no floating-point atomics; an item's numbers depend on the item's columns alone, the list's on the items' numbers
 * and their order.  Two launches on `stream`; nothing allocates or synchronises.
 * A record with Tq < 1, q_off < 0 or q_off + Tq > pitch gets sqerr = 0, K zero counts and zero stats; nothing is read for it.
 * first: a list that runs as consecutive groups (each with its own packed arrays and table) keeps ONE sqerr / hist / item_stats of
 * all its items; one group: first = 0.
 * WAE_EINVAL before any launch for a null pointer, nsegs < 1, D < 1, K < 1, pitch < 1 or first < 0; WAE_EUNSUPPORTED for K > 8192
 * (the counts of an item live in 32 KiB of LDS). */
typedef struct wae_vq_seg { int32_t q_off, Tq; } wae_vq_seg;
int wae_vq_stats_segments(const float* lat, const float* quant, const int64_t* idx, const wae_vq_seg* segs, int32_t nsegs, int32_t D,
                          int32_t pitch, int32_t K, float c_loss, int32_t first, float* sqerr, int32_t* hist, float* item_stats,
                          float* out, void* stream);

/* ---- a3 one upsample stage (upsample.py:19-21 stretch + :39-46 FIR) ------------------------------------
 * in (B,C,Tin) fp32 -> nearest-stretch by s, FIR w[2s+1] zero-padded.  If out_btc != 0 the result is written
 * time-major (B,Tin*s,Cp) in `dtype` (pad channels zeroed), else (B,C,Tin*s) fp32. */
int wae_upsample_stage_fwd(const float* in, const float* w, void* out, int32_t B, int32_t C, int32_t Tin,
                           int32_t s, int32_t out_btc, int32_t Cp, int32_t dtype, void* stream);

/* ---- a3 over a LIST of utterances of unequal lengths (upsample.py:12-85, forward, inference: the upsampling network for every
 * item of a decode list in one launch per stage).  The reference upsamples one dense (B,C,T) batch; a list is otherwise a loop of
 * batch-1 chains -- a conv_in launch, one launch per stage and as many allocations per item, in front of the ONE launch that decodes
 * the list (wae_ar_generate_list and its kin read every item's rows of one packed time-major c_up).
 * Packed layout: an activation of the list is channel-major and packed along time, as in wae_enc_conv_fwd_list -- (C, pitch) fp32,
 * item i owning the columns [off_i, off_i + T_i).  The final operand is time-major (rows, Cp) in `dtype`, item i owning the rows
 * [out_off_i, out_off_i + Tout_i); its pad channels [C, Cp) are written as zeros, as wae_to_btc and the dense last stage do.  An
 * item's row offset is free (the caller's order; not monotone in in_off).  Every item is zero-padded at its own two ends: a tap
 * outside [0, Tout_i) contributes nothing, it never reads the neighbour's column.
 * Table (a DEVICE array the host builds -- packing.upsample_list_plan; nothing here allocates or synchronises): nsegs records
 * wae_ups_seg {in_off, Tin, out_off, tile0}, tile0 = the index of the item's first tile, and ONE closing record whose tile0 is the
 * tile count (nsegs + 1 records in all).  The grid is the tile count; a workgroup finds its item by a workgroup-uniform binary search
 * on tile0, so the table follows the number of items, not of samples.  A tile is WAE_UPS_LIST_TILE_BTC output steps of one item in
 * the time-major forms, WAE_UPS_LIST_TILE_CT output columns (of 8 channel rows in turn) in the channel-major form, masked at the item's Tout_i.
 * wae_upsample_stage_fwd_list, one stage by the scale s (Tout_i = Tin_i * s, w[2s+1]):
 *   out_btc = 0: in (C, in_pitch) -> out (C, out_pitch_or_rows) fp32, tap by tap as wae_upsample_stage_fwd -- acc = fmaf(w[j], r[u / s], acc)
 *     for j = 0..2s with u = t + j - s inside [0, Tout_i), the frame index kept incrementally (Cp and dtype unused);
 *   out_btc = 1: the last stage, in (C, in_pitch) -> out (out_pitch_or_rows, Cp) in `dtype`, the input frames of a tile staged in LDS.
 *     16-bit outputs use the three summed taps on the interior steps s <= t, t + s < Tout_i OF THE ITEM and the tap form on the s
 *     steps at either end of every item; fp32 output uses the tap form everywhere -- exactly wae_upsample_stage_fwd's rule, taken
 *     against the item's own length.
 * wae_to_btc_list: in (C, in_pitch) fp32 -> out (rows, Cp) in `dtype` through the 64x64 LDS tile of wae_to_btc, rows
 *   [out_off_i, out_off_i + Tin_i) <- columns [in_off_i, in_off_i + Tin_i); for the chains whose last stage does not write the operand
 *   itself (an upsample_activation; the plain UpsampleNetwork, whose trim the host folds into in_off / Tin) and for conditioning that
 *   arrives upsampled.  (This entry is not told the rows of out: the host's offsets are the bound of out_off_i + Tin_i.)
 * Every item's rows are, bit for bit, what wae_upsample_stage_fwd / wae_to_btc write for that item alone (B = 1): both compile the
 * same per-output functions (csrc/ups_fir.hpp).  Rows and columns that no item owns are not written.
 * Returns WAE_EINVAL for null in / w / out / segs, C, s, nsegs, ntiles or a pitch < 1, Cp < C or a bad dtype (time-major forms);
 * WAE_EUNSUPPORTED for the time-major stage with Cp > 256, 256 % Cp != 0, 3 s > 256 or more than 64 KiB of LDS -- the caller then
 * loops wae_upsample_stage_fwd.  Every refusal returns before any launch.  A record that does not fit the pitches, or whose tile
 * count contradicts Tout_i = Tin_i * s, is skipped by the kernel: nothing is read or written for it. */
#define WAE_UPS_LIST_TILE_BTC 64
#define WAE_UPS_LIST_TILE_CT 256
typedef struct wae_ups_seg { int32_t in_off, Tin, out_off, tile0; } wae_ups_seg;
int wae_upsample_stage_fwd_list(const float* in, const float* w, void* out, const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles,
                                int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s, int32_t out_btc, int32_t Cp,
                                int32_t dtype, void* stream);
int wae_to_btc_list(const float* in, void* out, const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t in_pitch,
                    int32_t C, int32_t Cp, int32_t dtype, void* stream);

/* ---- a3 over ROW RANGES of clips that are still growing (a decode session's open clips: DecodeSession.open / feed / end).
 * wae_upsample_stage_fwd_list computes every row of every item; this entry computes the rows [t_lo, t_hi) of every record, from the
 * input columns that are valid NOW.  Output row t of a stage reads the input frames t/s - 1 .. t/s + 1 and nothing else, so with Tin
 * frames of a clip final, rows t < (Tin - 1) * s are final whatever arrives later: for them every tap u = t + j - s lies below Tin * s,
 * and the per-output functions (csrc/ups_fir.hpp), called with Tout = Tin * s, run the operations they will run against the clip's
 * true, longer Tout -- the tap walk stops at 2s either way and the 16-bit interior test s <= t && t + s < Tout gives the same answer.
 * Once a clip has ended, Tin * s IS its Tout and all rows are final.  The kernels carry no "open" flag; the HOST guarantees
 * t_hi <= (Tin - 1) * s while a clip is open and t_hi <= Tin * s once it has ended (packing.session_feed_plan).
 * Record wae_ups_range {in_off, Tin, out_off, t_lo, t_hi, tile0}: in_off, Tin -- the clip's input columns [in_off, in_off + Tin) of
 * `in` (C, in_pitch) fp32 that are valid now; out_off -- the column (out_btc = 0: out (C, out_pitch_or_rows) fp32) or the row
 * (out_btc = 1: out (out_pitch_or_rows, Cp) in `dtype`) of the clip's output row 0; t_lo, t_hi -- the rows to compute, in the clip's
 * own numbering; tile0 -- the index of the record's first tile.  nrecs records and ONE closing record whose tile0 is the tile count,
 * a DEVICE array.  The tiles of a record count from t_lo: tile k is the rows [t_lo + k * tile, min(t_lo + (k + 1) * tile, t_hi)),
 * tile = WAE_UPS_LIST_TILE_CT (channel-major) or WAE_UPS_LIST_TILE_BTC (time-major); a workgroup finds its record by the
 * workgroup-uniform binary search of the list kernels.  Both forms are the list entry's: tap by tap in fp32 channel-major; the
 * time-major last stage with a tile's frames staged in LDS, pad channels [C, Cp) written as zeros and the three summed taps on the
 * interior steps of 16-bit outputs.  Rows outside every [t_lo, t_hi) are not written.
 * The kernel does not trust the table with memory: a record with Tin < 1, t_lo < 0, t_lo >= t_hi, t_hi > Tin * s, a tile count other
 * than ceil((t_hi - t_lo) / tile), in_off + Tin beyond in_pitch or out_off + t_hi beyond out_pitch_or_rows is skipped, nothing read or
 * written for it.  Returns WAE_EINVAL / WAE_EUNSUPPORTED exactly where wae_upsample_stage_fwd_list does, before any launch; nothing
 * allocates or synchronises. */
typedef struct wae_ups_range { int32_t in_off, Tin, out_off, t_lo, t_hi, tile0; } wae_ups_range;
int wae_upsample_stage_fwd_ranges(const float* in, const float* w, void* out, const wae_ups_range* recs, int32_t nrecs, int32_t ntiles,
                                  int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s, int32_t out_btc, int32_t Cp,
                                  int32_t dtype, void* stream);

/* ---- a3 over row ranges of clips that live in RINGS: the ring-addressed twin of wae_upsample_stage_fwd_ranges.
 * Record wae_ups_ring {in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0}: Tin -- as in wae_ups_range, the clip's input
 * frames that are valid now; only the last in_period are held, frame u at column in_off + u % in_period of `in` (C, in_pitch).
 * Output row t goes to the column (out_btc = 0) or the row (out_btc = 1) out_off + t % out_period, out_period >= 1.  Everything else
 * -- ranges, tiles, the closing record, the binary search, both forms, the guarantee t_hi <= (Tin - 1) * s asked of the host while a
 * clip is open -- is wae_upsample_stage_fwd_ranges'.  The ring is an address only: the time-major last stage maps it where it stages
 * a tile's frames in LDS, the channel-major stage reads the three frames t/s - 1 .. t/s + 1 of an output into registers, and both
 * then run the per-output functions of csrc/ups_fir.hpp on that linear copy: every row is the ranges entry's and the dense stage's,
 * bit for bit, whatever the periods (csrc/ups_ring.hip).
 * The kernel does not trust the table with memory: it is skipped as a whole, nothing read or written for it, a record that
 * wae_upsample_stage_fwd_ranges would skip for its Tin, t_lo, t_hi or tile count, and one with in_period < 1, in_off < 0,
 * in_off + in_period > in_pitch, out_period < 1, out_off < 0, out_off + out_period > out_pitch_or_rows, t_hi - t_lo > out_period,
 * or -- aliasing -- a first frame max(t_lo - s, 0) / s older than Tin - in_period: that frame is gone and its slot holds a newer one.
 * Returns WAE_EINVAL / WAE_EUNSUPPORTED exactly where wae_upsample_stage_fwd_ranges does, before any launch; nothing allocates or
 * synchronises. */
typedef struct wae_ups_ring { int32_t in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0; } wae_ups_ring;
int wae_upsample_stage_fwd_rings(const float* in, const float* w, void* out, const wae_ups_ring* recs, int32_t nrecs, int32_t ntiles,
                                 int32_t in_pitch, int32_t out_pitch_or_rows, int32_t C, int32_t s, int32_t out_btc, int32_t Cp,
                                 int32_t dtype, void* stream);

/* ---- a4/K5 hoisted global conditioning: zb[b][l][2Hp] = bias_l + Wg_l . g_b  (modules.py:148-152) ------
 * g_b = eff[emb_off + gid[b]*Cg ..] (Embedding lookup, wavenet.py:185-190) when gid != NULL, else gvec[b*Cg ..]
 * (external features); both NULL or wg_off < 0 = no global conditioning.  Layer l reads its conv bias at
 * eff[bias_off + l*layer_stride] and its conv1x1g weight (G,Cg) at eff[wg_off + l*layer_stride]. */
int wae_gproj_fwd(const float* eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride, const int32_t* gid,
                  int64_t emb_off, const float* gvec, float* zb, int32_t B, int32_t L, int32_t G, int32_t Hp,
                  int32_t Cg, int32_t n_speakers, int32_t* err, void* stream);

/* backward of wae_gproj_fwd.  c1: the per-layer dW1 tiles of wae_gemm_tn_tiles (L x 2Hp x ld fp32) whose columns
 * ones_col + b hold sum_t dz[b,t,row] = d loss / d zb[b][l][row]; adds into d_eff: conv bias, conv1x1g weight and
 * (gid != NULL) the embedding rows. */
int wae_gproj_bwd(const float* eff, float* d_eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride,
                  const int32_t* gid, int64_t emb_off, const float* gvec, const float* c1, int64_t c_layer_stride,
                  int64_t ld, int32_t ones_col, int32_t B, int32_t L, int32_t G, int32_t Hp, int32_t Cg,
                  int32_t n_speakers, void* stream);

/* ---- gradient accumulation (csrc/accum.hip; engine.py: accumulate / apply_step) ---------------------------
 * wae_gproj_bwd that CONSUMES what it reads: wae_gproj_bwd's arguments and, statement for statement, its arithmetic -- d_eff gets
 * the same bits from the same tiles -- and every element c1[l][row][ones_col + b], row < 2Hp, b < B, is 0.0f afterwards (a plain
 * store by the thread that read it; nothing else of c1 is written).  Inside an accumulation window the weight-gradient tiles are
 * not cleared between micro-batches: those columns are per CLIP (clip b's sum_t dz, chained here into conv1x1g and the embedding row
 * of speaker gid[b]), so clip b of the next micro-batch must start from zero; every other tile element is a sum over clips and
 * simply keeps growing.  One launch per 32 clips, no pass over the tiles.
 * WAE_EINVAL before any launch for wae_gproj_bwd's refusals and for columns that do not fit: ld < ones_col + B, or
 * c_layer_stride < 2Hp * ld. */
int wae_gproj_bwd_consume(const float* eff, float* d_eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride,
                          const int32_t* gid, int64_t emb_off, const float* gvec, float* c1, int64_t c_layer_stride,
                          int64_t ld, int32_t ones_col, int32_t B, int32_t L, int32_t G, int32_t Hp, int32_t Cg,
                          int32_t n_speakers, void* stream);

/* The logged numbers of an accumulation window, kept on the device.  sums (3 doubles): [0] = sum_i ce_weight_i * ce_i,
 * [1] = sum_i vq_weight_i * vq_loss_i, [2] = the number of micro-batches; counts (K int32, or NULL without a quantiser): the
 * micro-batches' code histograms added per code.  The caller zeroes both when it opens the window.
 * out == NULL: one micro-batch is added -- ce / vq_loss (one float each on the device, NULL = absent) times their weights in
 * double, hist (K counts, what wae_vq_nearest leaves) into counts.
 * out != NULL (5 floats): the window is closed -- out = [ce, vq_loss, ce + vq_loss, perplexity, micro-batches]; the perplexity is
 * that of the added counts with N = their sum, by the one function the dense search and wae_vq_stats_segments use
 * (csrc/vq_stats.hpp): bit for bit what the search reports for the concatenated batch.  0 without counts.
 * One workgroup, one launch, a fixed order of additions and no floating-point atomics: the same numbers from run to run. */
int wae_accum_stats(double* sums, int32_t* counts, int32_t K, const float* ce, double ce_weight, const float* vq_loss,
                    double vq_weight, const int32_t* hist, float* out, void* stream);

/* ---- the fixed-order forms of the small float sums of a train step (EngineOptions.deterministic) ----------------
 * Each entry below takes its default twin's arguments (plus a partials buffer where it needs one) and computes the same quantity
 * with every sum that more than one workgroup feeds formed in a FIXED ORDER: one owner per output, or partials finished by a second
 * small launch in index order.  No floating-point atomics, no workgroup waits for another; partials are stored before they are read,
 * by plain stores, so no buffer needs clearing.  The same operands give the same bits on the same device model and build; the bits
 * are not the default twin's (another order of fp32 additions).  A partials buffer too small: WAE_EINVAL before any launch.
 *
 * wae_gproj_bwd_det: wae_gproj_bwd (consume = 0) or wae_gproj_bwd_consume (consume = 1).  Conv bias and conv1x1g rows have one owner
 *   in both forms.  The embedding rows: launch 1 stores, per (layer l, block k of 32 gate rows, clip b, feature c), the block's sum
 *   to parts[l][k][b][c] (wae_gproj_bwd_det_floats(B, L, Hp, Cg) = L * ceil(2Hp / 32) * B * Cg floats); launch 2, one thread per
 *   (speaker, feature): the clips of that speaker in index order, per clip the layers 0 .. L-1, per layer the blocks in order, all added
 *   one after another from zero, then d_eff[row] = d_eff[row] + sum.
 * wae_upsample_stage_bwd_det: wae_upsample_stage_bwd; din as there; the FIR's weight gradient: block i of the nbw = min(B * C, 256)
 *   weight blocks stores its 2s+1 tap sums to parts[i][tap] (wae_upsample_stage_bwd_det_floats() floats); one workgroup adds, per tap,
 *   the blocks 0 .. nbw-1 in order (from block 0's sum) and then dw[tap] = dw[tap] + sum.
 * wae_upsample_stage_bwd_list_det: wae_upsample_stage_bwd_list (the arguments, the table and the refusals of that entry; further down
 *   in this file); din as there; the FIR's weight gradient: workgroup i of the grid = min(ntiles, 512) workgroups walks the tiles
 *   i, i + grid, ... in that order, forms its 2s+1 tap sums as the default twin does (per thread over its tiles and channels, a xor
 *   butterfly over the 64 lanes, the four waves added in wave order) and stores them to parts[i][tap], rows of 33 floats
 *   (wae_upsample_stage_bwd_list_det_floats() = 512 * 33 floats); one workgroup, thread = tap, adds parts[0 .. grid-1][tap] in index
 *   order from zero and then dw[tap] = dw[tap] + sum.  A workgroup whose records were all refused stores zeros.  The result depends
 *   on the table's order (which tiles a workgroup walks); din does not.  parts NULL or short: WAE_EINVAL before any launch.
 * wae_vq_slice_bwd_det / wae_vq_bwd_det: wae_vq_slice_bwd / wae_vq_bwd with K, the number of codes; dlat as there; the codebook
 *   gradient by one workgroup per code: the frames in row order b * Tq + t whose idx is the code add -c_emb * (lat - quant) in turn
 *   (from zero), then demb[code] = demb[code] + sum; a code that no frame uses is not written.  D <= 1024.
 * wae_vq_loss_det: stats[0] of wae_vq_slice (modes 0, 2) / wae_vq_nearest again from lat and quant: c_loss * (sum / ((float)(B * Tq) *
 *   (float)D)), the sum of (quant - lat)^2 over the slice in fp64 by ONE workgroup -- thread j of 256 takes the elements j, j + 256, ...
 *   in (b, channel, t) order, a xor butterfly over the 64 lanes, the four waves in wave order -- rounded to fp32 once.
 * wae_clip_adam_ema_det: wae_clip_adam_ema; the squared norm: workgroup i of grid = min(1024, ceil(n / 1024)) sums its elements as
 *   there (thread by thread, xor butterfly, four waves in order) and stores the fp64 sum to parts[1 + i]; one thread adds parts[1 ..
 *   grid] in index order into parts[0], which the clip + Adam + EMA launch reads.  parts: at least 1025 doubles. */
int64_t wae_gproj_bwd_det_floats(int32_t B, int32_t L, int32_t Hp, int32_t Cg);
int wae_gproj_bwd_det(const float* eff, float* d_eff, int64_t wg_off, int64_t bias_off, int64_t layer_stride,
                      const int32_t* gid, int64_t emb_off, const float* gvec, float* c1, int64_t c_layer_stride, int64_t ld,
                      int32_t ones_col, int32_t B, int32_t L, int32_t G, int32_t Hp, int32_t Cg, int32_t n_speakers,
                      int32_t consume, float* parts, int64_t parts_floats, void* stream);
int64_t wae_upsample_stage_bwd_det_floats(void);
int wae_upsample_stage_bwd_det(const float* dout, const float* in, const float* w, float* din, float* dw, float* parts,
                               int64_t parts_floats, int32_t B, int32_t C, int32_t Tin, int32_t s, void* stream);
int64_t wae_upsample_stage_bwd_list_det_floats(void);
int wae_upsample_stage_bwd_list_det(const float* dout, const float* in, const float* w, float* din, float* dw,
                                    const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t in_pitch, int32_t out_pitch,
                                    int32_t C, int32_t s, float* parts, int64_t parts_floats, void* stream);
int wae_vq_slice_bwd_det(const float* lat, const float* quant, const int64_t* idx, const float* dquant, float* dlat,
                         float* demb, int32_t B, int32_t Dtot, int32_t d0, int32_t D, int32_t Tq, int32_t K, float c_lat,
                         float c_emb, void* stream);
int wae_vq_bwd_det(const float* lat, const float* quant, const int64_t* idx, const float* dquant, float* dlat, float* demb,
                   int32_t B, int32_t D, int32_t Tq, int32_t K, float beta, float loss_scale, void* stream);
int wae_vq_loss_det(const float* lat, const float* quant, float* stats, int32_t B, int32_t Dtot, int32_t d0, int32_t D,
                    int32_t Tq, float c_loss, void* stream);
int wae_clip_adam_ema_det(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* shadow, int64_t n,
                          double* parts, int64_t parts_doubles, float* grad_norm_out, int32_t step, double lr, double beta1,
                          double beta2, double eps, double weight_decay, double clip_thresh, double ema_decay, void* stream);

/* ---- a5 first_conv on one-hot input = column gather + bias (wavenet.py:119-122,203) --------------------
 * idx (B*T) int32 class ids; table (O,Rp) fp32 = W^T ; x0 (B,T,Rp) dtype.  scalar mode: xs (B*T) fp32,
 * table (1,Rp). */
int wae_first_conv_fwd(const int32_t* idx, const float* xs, const float* table, const float* bias, void* x0,
                       int64_t BT, int32_t Rp, int32_t O, int32_t dtype, int32_t* err, void* stream);

/* One-hot rows of the class ids: out (n, width) dtype, out[i][ids[i]] = 1 (ids outside [0, width): a zero row).  The operand that
 * turns the first conv's weight gradient (autograd of wavenet.py:203: dW[:, class] = sum of dx0 rows whose input is `class`) into a
 * P^T Q contraction of wae_gemm_tn_static. */
int wae_onehot_rows(const int32_t* ids, void* out, int64_t n, int32_t width, int32_t dtype, void* stream);

/* Ids that index tables (class ids -> first-conv table / targets, speaker ids -> embedding rows): the reference raises
 * IndexError (nn.Embedding, wavenet.py:185-190; one-hot encoding, vqwae_train.py:511).  The kernels clamp an id outside its
 * table -- no access leaves it -- and OR a WAE_ERR_* bit into the caller's sticky device word `err` (nullable); wae_check_ids
 * does the same for any id array (e.g. the CE targets) against [lo, hi).  The host raises when it next reads the word. */
#define WAE_ERR_CLASS_ID 1
#define WAE_ERR_SPEAKER_ID 2
#define WAE_ERR_TARGET_ID 4
int wae_check_ids(const int32_t* ids, int64_t n, int32_t lo, int32_t hi, int32_t* err, int32_t code, void* stream);
/* One-hot (B, C, T) fp32 input -> class ids (B, T).  wavenet.py:203 applies first_conv to any (B, C, T) float tensor; the kernels
 * gather weight rows by class id, the same arithmetic for one-hot columns only.  A column that is not exactly one 1.0 among zeros
 * ORs `code` (WAE_ERR_NOT_ONEHOT) into `err`: the host refuses dense inputs instead of arg-maxing them.  Strides in elements. */
#define WAE_ERR_NOT_ONEHOT 8
int wae_onehot_to_ids(const float* x, int32_t B, int32_t C, int32_t T, int64_t stride_b, int64_t stride_c, int64_t stride_t,
                      int32_t* ids, int32_t* err, int32_t code, void* stream);

/* ---- two chains of layer launches (round 6) ------------------------------------------------------------------
 * Every workgroup of a layer launch stores its outputs at the same time (forward: z, u, x' -- 106 MB at BASELINE C2, ~20 us of a 55-us
 * launch in which nothing computes).  One launch cannot be de-phased against itself, two CHAINS of launches can: the host runs the
 * gated stack (and the backward sweep) as two half-batch chains on two streams -- the same entry points with B / 2 clips and offset
 * pointers; every array of this ABI is clip-major -- and starts the second chain `us` microseconds late with this call: one wave that
 * sleeps on the wall clock.  Results are bit for bit those of one chain (no clip reads another clip's rows). */
int wae_stream_delay(double us, void* stream);

/* ---- a6 ResidualConv1dGLU._forward (modules.py:115-163) -------------------------------------------------
 * One fused layer: dilated causal conv + 1x1(c) + hoisted 1x1(g) + gate + 1x1 out + residual.  The skip 1x1
 * (modules.py:157) and `skips += h` (wavenet.py:204-207) are deferred: the layer stores its gated activation
 * u_l = tanh(a)*sigmoid(b) and wae_head_fwd contracts all layers' u against [W_skip_0 .. W_skip_{L-1}] at once. */
typedef struct wae_glu_desc {
  int32_t dtype;
  int32_t B, T;
  int32_t Rp, Ccp, Hp; /* padded: Rp % 128 == 0, Ccp % 64 == 0 (may be 0), Hp % 32 == 0, Hp <= 192 */
  int32_t ktaps;       /* kernel_size */
  int32_t dilation;
  int32_t flags;
} wae_glu_desc;
/* x_in,x_out (B,T,Rp) dtype; c_up (B,T,Ccp) dtype; u_out: this layer's Hp columns inside a (B,T,u_stride) dtype
 * buffer (pointer already offset to the layer's first column); zb (B,2Hp) fp32 for THIS layer (row stride
 * zb_stride floats) = conv bias + hoisted global conditioning; z_save (B,T,2Hp) dtype or NULL;
 * w_packed = [W1 chunks | W_out chunks] in fragment order; bias_out (Rp) fp32. */
int wae_glu_layer_fwd(const wae_glu_desc* d, const void* x_in, void* x_out, const void* c_up, void* u_out,
                      int64_t u_stride, const float* zb, int64_t zb_stride, void* z_save, const void* w_packed,
                      const float* bias_out, void* stream);
/* The same layer in TRAINING with dropout > 0 (modules.py:127-128: F.dropout in front of the dilated convolution only; the
 * residual path keeps the layer's input): x_conv = wae_dropout_fwd(x_in) is the operand of the convolution taps, x_in that
 * of the residual add.  wae_glu_layer_fwd is this entry with x_conv = x_in. */
int wae_glu_layer_fwd_drop(const wae_glu_desc* d, const void* x_in, const void* x_conv, void* x_out, const void* c_up, void* u_out,
                           int64_t u_stride, const float* zb, int64_t zb_stride, void* z_save, const void* w_packed,
                           const float* bias_out, void* stream);
/* xd[i] = keep(seed, i) ? x[i] / (1 - p) : 0 over n elements of `dtype`; keep = a counter-based hash of (seed, i) whose top 24
 * bits are >= p * 2^24 (restated by the oracle).  Backward of the convolution input through the same mask, fused with the
 * residual add of modules.py:161: out[i] = alpha * (g_next[i] + (keep ? acc[i] / (1 - p) : 0)), acc = the tap contraction
 * W1^T dz (wae_gemm_tm mode 0); the weight gradient dW1 contracts dz against xd. */
int wae_dropout_fwd(const void* x, void* xd, int64_t n, uint64_t seed, float p, int32_t dtype, void* stream);
int wae_dropout_bwd(const void* acc, const void* g_next, void* out, int64_t n, uint64_t seed, float p, float alpha, int32_t dtype,
                    void* stream);
int64_t wae_glu_packed_bytes(const wae_glu_desc* d);

/* ---- a6 over a LIST of utterances of unequal lengths (teacher-forced, inference): one launch per layer for the whole list.
 * The activations of a list are time-major and packed along time -- x_in, x_out (rows, Rp), c_up (rows, Ccp), u_out (rows, u_stride)
 * in `dtype` -- item i owning the rows [row_off_i, row_off_i + T_i): the operand wae_upsample_stage_fwd_list writes.
 * Table (a DEVICE array the host builds -- packing.glu_list_plan; nothing here allocates or synchronises): nsegs records
 * wae_glu_seg {row_off, T, zb_row, tile0} and ONE closing record whose tile0 is the tile count (the pattern of wae_ups_seg).  zb_row
 * is the item's row of zb (B rows of zb_stride floats: d->B counts the rows of zb, d->T is not read).  The grid is ntiles; a workgroup
 * finds its record by the workgroup-uniform binary search of the other list kernels; tile j of a record is the item's columns
 * [j * TW, min((j + 1) * TW, T_i)), TW = wae_glu_list_tile(dtype) (128 for fp32, 256 for bf16 / fp16).
 * The kernel is wae_glu_layer_fwd's generic kernel template (csrc/glu_fwd_kernel.hpp) compiled with the item's record in the place of
 * (b, d->T): the causal zero fill, the row clamp of the operand requests, the valid rows of both epilogues and the residual read are
 * taken against the item's own T_i and row_off_i.  A tap before the item's t = 0 reads zero, never the previous item's rows, and the
 * per-column instruction sequence is the dense kernel's: every item's rows of x_out and u_out are, bit for bit, what
 * wae_glu_layer_fwd writes for that item alone (B = 1), static-schedule instantiations included (bit-identical by their own
 * contract).  Rows no record owns are not written.
 * Inference only: WAE_GLU_SAVE_Z returns WAE_EUNSUPPORTED, and there is no x_conv (dropout) form; WAE_GLU_CG2 / WAE_GLU_WAVES4 are
 * ignored (the list has the 8-wave 16-bit and the 4-wave fp32 shapes only); WAE_GLU_NO_OUT and WAE_GLU_PAIR are honoured.
 * The kernel does not trust the table with memory: a record with T < 1, row_off < 0, row_off + T > rows, zb_row outside [0, B) or a
 * tile count other than ceil(T / TW) is skipped whole, nothing read or written for it.  WAE_EINVAL / WAE_EUNSUPPORTED come back
 * before any launch for the argument errors of wae_glu_layer_fwd, and WAE_EINVAL for a null table, nsegs, ntiles or rows < 1. */
typedef struct wae_glu_seg { int32_t row_off, T, zb_row, tile0; } wae_glu_seg;
int32_t wae_glu_list_tile(int32_t dtype);      /* the tile width the table must be built for; WAE_EINVAL for a bad dtype */
int wae_glu_layer_fwd_list(const wae_glu_desc* d, const wae_glu_seg* segs, int32_t nsegs, int32_t ntiles, int32_t rows,
                           const void* x_in, void* x_out, const void* c_up, void* u_out, int64_t u_stride, const float* zb,
                           int64_t zb_stride, const void* w_packed, const float* bias_out, void* stream);

/* ---- the shifted CE of a packed list, per utterance (vqwae_train.py:363-379,:764 for every item as a batch of one).
 * The head kernels are per column: on the packed rows they run as B = 1, T = rows, and wae_head_fwd's nll (rows) then takes the last
 * row of item i against the first id of item i + 1.  This entry, from that nll and the list's wae_glu_seg table (zb_row and tile0 are
 * not read): zeroes nll[row_off_i + T_i - 1] in place (what the item's own forward reports at t = T_i - 1), writes
 * nll_sum[first + i] = sum of the item's rows t < T_i - 1 and count[first + i] = T_i - 1, and out[0] = sum nll_sum / sum count (defined as 0 when the
 * total count is 0: a list of one-sample items has no shifted target), out[1] = sum_i count[i] as a float.
 * Deterministic: one workgroup per item adds its rows in a fixed order by a fixed tree (an item's nll_sum depends on nothing but the
 * item's rows), and one workgroup then walks nll_sum in table order; no floating-point atomics.  Two launches on `stream`.
 * A record with T < 1, row_off < 0 or row_off + T > rows gets nll_sum = 0, count = 0 and nothing of nll is touched for it.
 * first: a list that runs as consecutive groups (each with its own packed arrays and table) keeps ONE nll_sum / count of all its items;
 * the group whose items are first .. first + nsegs - 1 of the list writes those entries, and out is taken over the entries
 * [0, first + nsegs): behind the last group it is the whole list's mean, walked in list order.  One group: first = 0.
 * WAE_EINVAL for a null pointer, nsegs < 1, rows < 1 or first < 0. */
int wae_nll_segments(float* nll, const wae_glu_seg* segs, int32_t nsegs, int32_t rows, int32_t first, float* nll_sum, int32_t* count,
                     float* out, void* stream);

/* ---- a7+a8+a9 skip sum + head (wavenet.py:204-214) + MaskedCrossEntropyLoss (vqwae_train.py:363-379,:764) ---
 * skips = sum_l (W_skip_l u_l + b_skip_l);  h0 = relu(skips * scale);  h1 = relu(W1 h0 + b1);  logits = W3 h1 + b3.
 * u (B,T,Ku) dtype holds all layers' gated activations, Ku = L*Hp rounded up to 64 (pad columns zero).
 * bias = [sum_l b_skip_l (Sp) | b1 (Sp) | b3 (Op)] fp32.  logits (B,O,T) fp32 or NULL.
 * If target != NULL: nll[b*T+t] = logsumexp(logits[:,t]) - logits[target[b*T+t+1], t] for t < T-1
 * (the reference's one-step shift), 0 at t = T-1; lse (B,T) or NULL receives logsumexp(logits[:,t]).
 * h0_save/h1_save (B,T,Sp) dtype or NULL (for backward). */
typedef struct wae_head_desc {
  int32_t dtype;
  int32_t B, T;
  int32_t Ku;     /* columns of u, multiple of 64 */
  int32_t Sp, Op; /* padded to multiples of 128 */
  int32_t O;      /* true class count */
  float scale;    /* sqrt(1/L) */
} wae_head_desc;
int wae_head_fwd(const wae_head_desc* d, const void* u, const void* w_packed, const float* bias, float* logits,
                 const int32_t* target, float* nll, float* lse, void* h0_save, void* h1_save, void* stream);

/* The second half of wae_head_fwd -- GEMM 1, GEMM 2, logits and / or the fused cross-entropy (wavenet.py:208-214,
 * vqwae_train.py:363-379,:764) -- from a stored h0 = relu(sqrt(1/L) (sum_l b_skip_l + W_skip u)) (B,T,Sp) dtype, for callers that ran
 * the skip contraction as a wae_gemm_tm launch (mode 3, the first Ku/CK chunks of the same packed stream as its weights).  w_tail =
 * w_packed + (Ku / CK) * (Sp / 32) * 4096 bytes (CK = 64 for 16-bit, 32 for fp32); bias as in wae_head_fwd (first Sp entries unread). */
int wae_head_fwd_from_h0(const wae_head_desc* d, const void* h0, const void* w_tail, const float* bias, float* logits,
                         const int32_t* target, float* nll, float* lse, void* h1_save, void* stream);
/* backward of the head down to dskip (csrc/head_bwd.hip).  CE mode (ext_dy == NULL): logits are recomputed from h1,
 * dy = (softmax - onehot(target[t+1])) * [t < len-1] * inv_count with the forward's lse (B,T); DMoL mode: ext_dy
 * (B,T,Op) dtype is the loss gradient.  Outputs, all time-major dtype: dy_out (B,T,Op), dh1_out (B,T,Sp) (pre-ReLU
 * gradient of h1), dskip_out (B,T,Sp) = d loss / d skips.  w_packed = [W3 first-order | W3^T | W1^T second-order]. */
int wae_head_bwd(const wae_head_desc* d, const void* h0, const void* h1, const void* w_packed, const float* b3,
                 const float* lse, const int32_t* target, const int32_t* lengths, float inv_count, const void* ext_dy,
                 void* dy_out, void* dh1_out, void* dskip_out, void* stream);
int64_t wae_head_bwd_packed_bytes(const wae_head_desc* d);
/* The training head in one launch (csrc/head_train.hip): wae_head_fwd_from_h0 with h1_save, the masked mean of its nll and wae_head_bwd
 * in CE mode, for 16-bit storage with Sp == Op in {128, 256} (wae_head_train_supported; anything else: WAE_EINVAL).  The logits stay in
 * registers between the forward's GEMM 2 and the softmax gradient, and the relu masks are kept as bits: one GEMM and two reloads less
 * than the two launches.  w_tail as for wae_head_fwd_from_h0; w_bwd_packed as for wae_head_bwd (its first-order W3 chunks are skipped).
 * dy_factor is wae_head_bwd's inv_count.  nll and lse (lse may be NULL) are bit for bit wae_head_fwd_from_h0's; dy / dh1 / dskip add the
 * same products as wae_head_bwd with the dy operand taken from the accumulators.  loss[0] = sum_{b, t < len[b]-1} nll / count and
 * loss[1] = count as wae_masked_mean writes them: per-workgroup partials in double, summed in index order by the workgroup that finishes
 * last, so the value does not depend on the order of arrival.  red_ws: wae_head_train_ws_bytes(d) bytes of device memory whose first
 * 16 are ZERO before the first launch (the launch leaves them zero); one launch at a time per red_ws. */
int wae_head_train_supported(int32_t dtype, int32_t Sp, int32_t Op);
int64_t wae_head_train_ws_bytes(const wae_head_desc* d);
int wae_head_train_from_h0(const wae_head_desc* d, const void* h0, const void* w_tail, const void* w_bwd_packed, const float* bias,
                           const int32_t* target, const int32_t* lengths, float dy_factor, float* nll, float* lse, void* h1_save,
                           void* dy_out, void* dh1_out, void* dskip_out, void* red_ws, float* loss, void* stream);
int64_t wae_head_packed_bytes(const wae_head_desc* d);

/* out[i] = sum_{l<L} src[off + l*stride + i] for i < n, 0 for n <= i < n_pad  (sum of the skip biases) */
int wae_sum_rows(const float* src, int64_t off, int64_t stride, int32_t L, int32_t n, int32_t n_pad, float* out,
                 void* stream);

/* masked mean of per-sample losses: out[0] = sum_{b,t<len[b]-1} nll / sum mask  (vqwae_train.py:379) */
int wae_masked_mean(const float* nll, const int32_t* lengths, float* out, int32_t B, int32_t T, void* stream);
/* The criterion object of vqwae_train.py:363-379 on EXPLICIT logits (the drop-in MaskedCrossEntropyLoss; training proper uses
 * the CE fused into wae_head_fwd): logits (B,C,T) fp32, target (B,T) int64 -> nll (B,T), lse (B,T); backward
 * dlogits = (softmax - onehot) * w[b,t].  A target outside [0, C) is clamped and flagged in err (WAE_ERR_TARGET_ID).
 * wae_weighted_mean: out[0] = sum(v*m) / sum(m), out[1] = sum(m) for any mask m (:374-379). */
int wae_ce_logits_fwd(const float* logits, const int64_t* target, float* nll, float* lse, int32_t B, int32_t C, int32_t T,
                      int32_t* err, void* stream);
int wae_ce_logits_bwd(const float* logits, const int64_t* target, const float* lse, const float* w, float* dlogits, int32_t B,
                      int32_t C, int32_t T, void* stream);
int wae_weighted_mean(const float* v, const float* m, int64_t n, float* out, void* stream);

/* ---- a10 discretized mixture of logistics (mixture.py:26-106; wrapper vqwae_train.py:382-401, shift :766) --
 * y_hat (B,3M,T) fp32 = [logit pi | mu | log s]; y (B,T) fp32 in [-1,1].  nll[b,t] = -log p(y[b,t+shift] | y_hat[b,:,t])
 * (0 where t+shift >= T); dy_hat (B,3M,T) or NULL = d nll[b,t] / d y_hat[b,:,t]. */
int wae_dmol_loss_fwd(const float* y_hat, const float* y, float* nll, float* dy_hat, int32_t B, int32_t M,
                      int32_t T, int32_t num_classes, float log_scale_min, int32_t shift, void* stream);
/* ---- a11 sample_from_discretized_mix_logistic (mixture.py:118-156) with caller-supplied U(1e-5,1-1e-5) draws:
 * y (B,3M,Tn), u_mix (B,Tn,M), u_log (B,Tn) -> out (B,Tn) in [-1,1]. */
int wae_dmol_sample(const float* y, const float* u_mix, const float* u_log, float* out, int32_t B, int32_t M,
                    int32_t Tn, float log_scale_min, int32_t clamp_log_scale, void* stream);

/* ---- mixture of Gaussians, output_distribution "Normal" (mixture.py:161-222; wrapper MixtureGaussianLoss vqwae_train.py:404-422,
 * shift :766) -- replaces mix_gaussian_loss(y_hat, y, log_scale_min, reduce=False) and its autograd backward.
 * y_hat (B,C,T) fp32: C == 2 one Gaussian [mu | log s]; otherwise M = C/3 (<= 32) as [logit pi | mu | log s], C == 3 being one
 * Gaussian whose logit row is ignored (gradient 0).  log s is clamped from below at log_scale_min (zero gradient under the clamp).
 * nll[b,t] = -log p(y[b,t+shift] | y_hat[b,:,t]) (0 where t+shift >= T); dy_hat (B,C,T) or NULL = d nll[b,t] / d y_hat[b,:,t]. */
int wae_mog_loss_fwd(const float* y_hat, const float* y, float* nll, float* dy_hat, int32_t B, int32_t C, int32_t T,
                     float log_scale_min, int32_t shift, void* stream);
/* ---- sample_from_mix_gaussian (mixture.py:225-270) with caller-supplied draws: Gumbel-max mixture pick on u_mix (B,Tn,M) in
 * (1e-5, 1-1e-5) when M > 1 (NULL allowed when M == 1), mu + exp(log s) z with z (B,Tn) ~ N(0,1), clamp to [-1,1] -> out (B,Tn).
 * As in the reference, log s is not clamped here. */
int wae_mog_sample(const float* y, const float* u_mix, const float* z, float* out, int32_t B, int32_t C, int32_t Tn, void* stream);

/* ---- a15 clip_grad_norm_ + Adam + EMA over the flat arena (vqwae_train.py:776-787, :339-350) ---------------
 * coef = min(1, clip/(||g||+1e-6)) (clip <= 0: off); torch.optim.Adam update with bias correction for the
 * 1-based `step`; shadow -= (1-ema_decay)*(shadow-p) when shadow != NULL.  scratch: one double.
 * grad_norm_out (1 float) or NULL receives the pre-clip global L2 norm. */
int wae_clip_adam_ema(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* shadow, int64_t n,
                      double* scratch, float* grad_norm_out, int32_t step, double lr, double beta1, double beta2,
                      double eps, double weight_decay, double clip_thresh, double ema_decay, void* stream);

/* the same step where `sqnorm` already holds the sum of the squares of all of grads (the wae_grad_finish launches added them while
 * they wrote grads; the caller cleared it before those): no memset and no pass over grads for the norm are enqueued. */
int wae_clip_adam_ema_summed(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* shadow, int64_t n,
                             const double* sqnorm, float* grad_norm_out, int32_t step, double lr, double beta1, double beta2,
                             double eps, double weight_decay, double clip_thresh, double ema_decay, void* stream);

/* ---- gradient finish (csrc/grad_finish.hip): packed weight-gradient tiles -> grads in one pass.  A row is `cols` consecutive arena
 * elements at `off`, owned by one 16-lane group: element i of its dW is tiles[base + pats[pat + i]] (pat >= 0, a multiple of 4:
 * the inverse of the scatter maps, the pattern shared by the rows of a tensor) or d_eff[off + i] (pat < 0).  g_off >= 0: a
 * weight-normed row -- grads[off..] = dv, grads[g_off] = dg, arithmetic of wae_weight_norm_bwd; g_off < 0: a plain parameter,
 * passed through.  sqnorm_acc (or NULL): receives += the sum of the squares of everything written, in double.
 * Rows [row_lo, row_hi) of the table are done; rows are disjoint, so any split of the table into calls gives the same grads. */
typedef struct wae_finish_row {
  int64_t off, g_off, base;
  int32_t cols, pat;
} wae_finish_row;
int wae_grad_finish(const float* params, const float* tiles, const int32_t* pats, const float* d_eff, float* grads,
                    const wae_finish_row* rows, int32_t row_lo, int32_t row_hi, double* sqnorm_acc, void* stream);

/* ---- softmax over the channel dimension of (B, C, T) fp32 logits: WaveNet.forward(softmax=True) / VQVAE.forward(softmax=True)
 * (wavenet.py:214, vqvae_model.py:79-80: F.softmax(x, dim=1)) and its backward dx = p (dp - sum_c p dp).  p may alias x; dx may alias dp. */
int wae_softmax_bct_fwd(const float* x, float* p, int32_t B, int32_t C, int32_t T, void* stream);
int wae_softmax_bct_bwd(const float* p, const float* dp, float* dx, int32_t B, int32_t C, int32_t T, void* stream);

/* C[n] = alpha * A[n] (M x K, row stride lda) B[n] (K x N, ldb), fp32, n < nbatch with the given batch strides: the per-layer products
 * sqrt(.5) W1_cur[l] W_out[l-1] a caller of wae_ar_generate_coop_fused forms once per weight update (engine.py: _pack_ar_fused). */
int wae_bmm_f32(const float* a, const float* b, float* c, int32_t nbatch, int32_t M, int32_t K, int32_t N, int64_t lda, int64_t ldb,
                int64_t ldc, int64_t stride_a, int64_t stride_b, int64_t stride_c, float alpha, void* stream);

/* ---- a12 incremental (autoregressive) decoding: Conv1d.incremental_forward (conv.py:17-62) and
 * WaveNet.incremental_forward (wavenet.py:218-346) as ONE persistent launch, one workgroup per utterance ------
 * mode 0: teacher-forced (the reference's test_inputs, softmax=False, quantize=False): logits out, inputs consumed
 * mode 1: greedy, the argmax class is fed back          mode 2: categorical draw by inverse CDF from uniforms[b,t]
 * mode 3 / 4 (wae_ar_generate only; quantize=False, wavenet.py:335-338 skipped): the softmax probabilities / the raw logits
 *   of step t are the dense decoder input of step t+1 (first_conv on a (1, O) row) and the step's row of out_logits
 * Partial teacher forcing (test_inputs shorter than T, wavenet.py:300-305): desc.n_forced.
 * Weights are blocked [k/EPL][rows padded to 64][EPL] (EPL = 8 bf16 / 4 fp32), per layer [W1 (G x (k*R+Cc)) | W2
 * ((R+S) x H)] with layer_stride_bytes between layers; head = [S x S | O x S].  ring: B x ring_total floats of
 * per-layer history, ring_off[l] = float offset of layer l ((k-1)*d_l+1 rows of R).  zb as in wae_gproj_fwd.
 * first_tab (O, Rp) / first_bias as in wae_first_conv_fwd; c_up (B,T,Ccp) already upsampled (wavenet.py:276-280).
 * inputs (B,T) int32 class ids or NULL (then init_idx starts every utterance, wavenet.py:288). */
typedef struct wae_ar_desc {
  int32_t dtype;
  int32_t B, T;
  int32_t L, R, Rp, G, Hp, S, O, Cc, Ccp, ktaps;
  int32_t mode;
  int32_t init_idx;
  int32_t scalar_input; /* 0: wae_ar_generate / wae_ar_generate_coop; 1: wae_ar_generate_scalar[_mog] / wae_ar_generate_coop_scalar / the two *_scalar_list entries
                         * 2: a scalar-input decoder, as 1, that asks for the constant-size scalar kernels ("scalar sized"; the struct keeps
                         *    its size and its last field t0, so the request travels in this field).  Read by the scalar cooperative
                         *    entries only (wae_ar_generate_coop_scalar, _coop_scalar_list, _coop_scalar_spans); every other entry reads 2 as 1
                         *    and a class-id descriptor (0) has no such request: class-id entries ignore it.
                         *    1: the any-shape kernel, always (the routing before the value existed).
                         *    2: the constant-size scalar kernels (csrc/ar_coop.hip: ar_coop_fast_body<.., SCALAR>, two hand-overs per layer)
                         *    where C == 32, R = G = S = 256, 3 taps, Cc <= 256, ring_total % 4 == 0, !coop_generic, O <= 256 and the (dtype,
                         *    packets per thread) pair has one -- with resident_lds / resident_regs honoured as by wae_ar_generate_coop -- and
                         *    silently the any-shape kernel otherwise.  The members then share ONE ring of ring_total floats
                         *    (wae_ar_coop_ring_floats), which the launch clears when t0 == 0.
                         *    The three entries dispatch by this one rule and run one device function, so a clip's items and spans are
                         *    bit for bit its single decode at the same value; values 1 and 2 agree to rounding, not bitwise (the sums are
                         *    split differently).  There is no one-hand-over (wae_ar_generate_coop_fused) scalar form and no constant-size kernel
                         *    for C != 32 or other widths. */
  float scale;          /* sqrt(1/L) */
  int32_t n_forced;     /* with inputs: steps t < n_forced consume inputs[t], later steps the fed-back output
                           (test_inputs shorter than T, wavenet.py:300-305); <= 0 or >= T: every step is forced */
  /* wae_ar_generate_coop only (the library reads no environment variable; rounds 4-5 had three): */
  int32_t coop_generic;  /* 1: the any-shape cooperative kernel also where the reference's geometry has one with its sizes as constants */
  int32_t resident_lds;  /* layers whose weight packets the fast kernel keeps in LDS: 0 = as many as fit, n > 0 = n, < 0 = none */
  int32_t resident_regs; /* ... and in registers (accumulation registers, then hand-allocated arch VGPRs): 0 = all that fit, n > 0 = n,
                            < 0 = none.  Where the packets wait is not arithmetic: results are bitwise the same for every split. */
  /* Streaming (every wae_ar_generate* entry).  The reference keeps each layer's input window between incremental_forward calls
   * (conv.py:17-62: input_buffer is shifted by one row per call and survives the call) until clear_buffer drops it
   * (wavenet.py:348-356).  Here that window is the caller's `ring`, and t0 says how much of it is filled:
   * t0 == 0: a fresh decode, exactly as without the field (the ring counts as empty; the cooperative kernels zero-fill it).
   * t0 > 0: a continuation.  t0 is the absolute index of this launch's first step; `ring` holds what earlier launches -- same geometry,
   *   weights, dtype, C, kernel form and residency split -- wrote for steps [0, t0).  The launch does not zero-fill the ring and writes
   *   only the rows of its own steps; ring rows, ring cursors and every "history before the clip starts" test use t0 + t.  The per-step
   *   operands (inputs, inputs_f, uniforms, u_mix, u_log / z / draws, c_up, out_idx, out_samples, out_logits, out_params) are indexed
   *   from this launch's step 0 with row length T, and n_forced counts from this launch's step 0.  The first step of a continuation is
   *   always forced: the caller puts the previous launch's last output (or the teacher-forced value) in inputs[b][0] / inputs_f[b][0].
   *   msg, acc and error are zeroed by the caller per launch, as ever: the exchange sequence numbers restart.
   * Refused before any launch: t0 < 0; t0 + T beyond int32_t; t0 > 0 without inputs / inputs_f; t0 > 0 in modes 3 / 4 (the vector they
   * feed back lives on chip); t0 > 0 with wae_ar_generate_coop_fused's w_fused (the one-hand-over form has no resume prologue). */
  int32_t t0;
} wae_ar_desc;
int wae_ar_generate(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                    int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                    const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                    const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                    const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits, void* stream);

/* Scalar-input decoders (first_conv has one input channel; wavenet.py:284-285,325-333): the fed-back quantity is the
 * float drawn by sample_from_discretized_mix_logistic (mixture.py:118-156) from the step's 3M mixture parameters, on
 * caller-supplied uniforms u_mix (B,T,M), u_log (B,T) in (1e-5, 1-1e-5).  inputs_f (B,T) teacher-forces the inputs
 * (step t consumes inputs_f[t]; the start value is 0 without it).  out_samples (B,T) and/or out_params (B,3M,T). */
int wae_ar_generate_scalar(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                           int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                           const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                           const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                           const float* inputs_f, const float* u_mix, const float* u_log, float log_scale_min,
                           int32_t clamp_log_scale, float* out_samples, float* out_params, void* stream);
/* The same decoding for output_distribution "Normal" (wavenet.py:329-331: sample_from_mix_gaussian, mixture.py:225-270, in place of
 * the logistic draw): the persistent kernel of wae_ar_generate_scalar with a Gaussian draw per step on the caller's u_mix (B,T,M)
 * (NULL allowed when M == 1) and z (B,T) standard normals.  O == 2 ([mu | log s]) or O = 3M; log_scale_min is accepted and unused,
 * as in the reference's sampler.  out_samples (B,T) and/or out_params (B,O,T); inputs_f teacher-forces as above. */
int wae_ar_generate_scalar_mog(const wae_ar_desc* d, const int32_t* dilations, const int64_t* ring_off, float* ring,
                               int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                               const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                               const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                               const float* inputs_f, const float* u_mix, const float* z, float log_scale_min,
                               float* out_samples, float* out_params, void* stream);

/* A work list of utterances of unequal lengths in ONE launch (csrc/ar_fwd.hip: ar_list_kernel): n_slots persistent workgroups, each
 * running the one-CU kernel's per-utterance body (the same device function, so an item's results are wae_ar_generate's for that
 * utterance alone, bit for bit, whichever slot decodes it and in whatever order).  A workgroup takes the next item index with one
 * returning atomic add on `next` (one int32_t the caller zeroes before the launch), decodes that item to its end, and leaves when the
 * index reaches n_items; no workgroup waits for another.  Items are taken in array order: put the longest first to keep the tail of
 * the launch short.
 * The per-step operands are packed item after item: c_up (total, Ccp), inputs / uniforms / out_idx (total), out_logits one (O, T)
 * block per item at float offset off * O, with total = the sum of the items' T; item.off is the item's first step there (with
 * off = b * T and row = b this is wae_ar_generate's (B, T) layout).  zb holds one (L, 2Hp) row per value of item.row (wae_gproj_fwd).
 * ring: n_slots x ring_total floats, never zero-filled: a decode reads a history row only behind its own write of that row.
 * item.n_forced: the first n_forced steps consume inputs[off + t] (clamped to [0, T]; 0, or inputs == NULL: the item starts from
 * item.init_idx, which is clamped to a class); mode 0 forces every step.  d->B, d->T, d->n_forced and d->init_idx are not read.
 * Class-id decoders in modes 0 / 1 / 2.  Refused before any launch: d->scalar_input and modes 3 / 4 (WAE_EUNSUPPORTED); t0 != 0,
 * n_items < 1, n_slots < 1, NULL items or next, mode 0 without inputs, mode 2 without uniforms (WAE_EINVAL). */
typedef struct wae_ar_item {
  int64_t off;      /* first step of the item in the packed per-step operands */
  int32_t T;        /* steps to decode (an item with T <= 0 is skipped) */
  int32_t n_forced;
  int32_t init_idx;
  int32_t row;      /* the item's row of zb */
} wae_ar_item;
int wae_ar_generate_list(const wae_ar_desc* d, int32_t n_items, int32_t n_slots, const wae_ar_item* items, int32_t* next,
                         const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                         const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                         const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                         const float* head_bias, const void* c_up, int32_t c_dtype, const int32_t* inputs,
                         const float* uniforms, int32_t* out_idx, float* out_logits, void* stream);

/* The same decoding with ONE utterance spread over C cooperating workgroups / CUs (csrc/ar_coop.hip): every layer is
 * split by gate channels; the members all-reduce their shares of x' once per layer and of the skip vector once per
 * sample through `acc` (B x wae_ar_coop_acc_floats(d) floats), `msg` ((B, 2, C, NV) 8-byte granules, NV =
 * wae_ar_coop_msg_values(d, C)) carries the start-up handshake; each member keeps its own copy of the history rings:
 * ring is (B, C, ring_total).  B <= 8, C <= 32, R, S and O <= 256.  The caller zeroes msg, acc and error (>= 64 ints) before
 * the launch; error[0] != 0 afterwards means a wait timed out (the output is then invalid).  No atomics: every share is one
 * stored {sequence number, fp32} granule and the members add them in a fixed order -- results are bitwise reproducible.  The
 * reference's geometry (R = G = S = O = 256, 3 taps, Cc <= 256) on C = 32 runs a kernel with those sizes as constants
 * (wae_ar_desc.coop_generic = 1 keeps the any-shape kernel); both zero-fill / overwrite `ring` themselves when t0 == 0 (the caller should still hand
 * over a zeroed ring: the fast kernel's members zero-fill their shares only when they sit on one XCD).  That kernel's
 * 32 members share ONE history ring per utterance (member 0's region of the (B, C, ring_total) allocation: every member writes every
 * row, the same bits) and, in 16-bit storage, keep every layer's weight packets on chip for the whole clip -- 6 layers in LDS, 11 in
 * the accumulation registers, 3 in hand-allocated arch VGPRs at the reference's 20 layers; deeper stacks stream the rest from L2.
 * wae_ar_desc.resident_lds / resident_regs override the number of layers kept in LDS / in registers (-1 -1: the streaming form;
 * results are bitwise the same for every split, tests/test_gpu_ar.py). */
int64_t wae_ar_coop_acc_floats(const wae_ar_desc* d);
int wae_ar_coop_msg_values(const wae_ar_desc* d, int32_t C);
int wae_ar_generate_coop(const wae_ar_desc* d, int32_t C, const int32_t* dilations, const int64_t* ring_off, float* ring,
                         int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                         const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                         const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                         const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits,
                         uint64_t* msg, float* acc, int32_t* error, void* stream);
/* A work list of utterances of unequal lengths on cooperative teams, in ONE launch (csrc/ar_coop.hip: the LIST forms): n_teams teams of
 * C workgroups -- the grid is wae_ar_generate_coop's 8 * C workgroups, team = blockIdx.x & 7, teams >= n_teams leave at once -- empty the
 * queue of wae_ar_generate_list: thread 0 of a team's member 0 takes the next item index with one returning atomic add on `next` (one
 * int32_t the caller zeroes), the index reaches the team-mates through one {sequence, value} exchange on msg, the team decodes that
 * item to its end on the kernels of wae_ar_generate_coop and comes back for the next; all members leave together when the index
 * reaches n_items, an item with T <= 0 is skipped by the whole team.  No team waits for another.  An item's results are
 * wae_ar_generate_coop's for that utterance alone (same C, same kernel form; w_fused = NULL), bit for bit, whichever team decodes it
 * and in whatever order.  Items, the packed per-step operands (c_up (total, Ccp), inputs / uniforms / out_idx (total), out_logits one
 * (O, T) block per item at float offset off * O), item.n_forced / init_idx / row and zb are wae_ar_generate_list's; `total` is the
 * sum of the items' T (the length of the packed operands).  ring: (n_teams, C, ring_total) floats; the kernels do not depend on its
 * contents (the constant-size kernels clear the team's shared ring before every item, the first included; the any-shape kernel reads a
 * history row only behind its own write of it).  msg: (n_teams, 2, C, NV) granules, acc: n_teams x wae_ar_coop_acc_floats(d) floats,
 * error: >= 64 ints; the caller zeroes msg, acc, error and next before the launch.  The exchange sequence numbers run on across a
 * team's items (nothing is re-zeroed inside the launch).  error[0] != 0 afterwards: a wait timed out in some team and every team left
 * at its next poll (the output is then invalid); error[1] = the placement word of team 0.
 * d->B, d->T, d->n_forced and d->init_idx are not read; coop_generic, resident_lds and resident_regs select the kernel as for
 * wae_ar_generate_coop: the reference's geometry on C = 32 takes the constant-size kernels with the same residency rules (the weight
 * packets stay on chip across items; only the two zb words of a resident layer are rewritten per item), everything else the
 * any-shape kernel.  Class-id decoders in modes 0 / 1 / 2, two hand-overs per layer (there is no list form of
 * wae_ar_generate_coop_fused).  Refused before any launch: d->scalar_input and modes 3 / 4 (WAE_EUNSUPPORTED); t0 != 0, n_items < 1,
 * n_teams outside 1..8, C outside 1..32, R, S or O > 256, NULL items, next, msg, acc or error, mode 0 without inputs, mode 2 without
 * uniforms, and a list with (total + n_items + 1) * (L + 4) >= 2^31, whose sequence numbers could wrap (WAE_EINVAL). */
int wae_ar_generate_coop_list(const wae_ar_desc* d, int32_t C, int32_t n_items, int32_t n_teams, const wae_ar_item* items,
                              int32_t* next, int64_t total, const int32_t* dilations, const int64_t* ring_off, float* ring,
                              int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                              const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                              const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                              const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits,
                              uint64_t* msg, float* acc, int32_t* error, void* stream);
/* The same call with one more operand for the reference's geometry on 32 members: w_fused = (L, G, Hp) row-major in the model's element
 * type, row block l = sqrt(.5) * W1_cur[l] . W_out[l-1] (the current-tap columns of layer l's dilated convolution times the previous
 * layer's conv1x1_out; block 0 unused) -- formed once per weight update by the caller (a plain matrix product).  Because
 * z_l = W1_cur[l] x_l + .. and x_l = sqrt(.5) (W_out[l-1] u_{l-1} + b_{l-1} + x_{l-1}), a member's 4 channels of u_{l-1} give its share of
 * all gate rows of layer l directly: ONE reduce-scatter per layer stays on the critical path instead of the all-reduce's two hand-overs
 * (csrc/ar_coop.hip: FUSED).  w_fused = NULL, or any other geometry: exactly wae_ar_generate_coop. */
int wae_ar_generate_coop_fused(const wae_ar_desc* d, int32_t C, const int32_t* dilations, const int64_t* ring_off, float* ring,
                         int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                         const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                         const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                         const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits,
                         uint64_t* msg, float* acc, int32_t* error, const void* w_fused, void* stream);
/* Scalar-input decoders on C cooperating workgroups: the network, split and exchanges of wae_ar_generate_coop (its weight, ring, zb,
 * c_up, msg, acc and error arguments, with the same sizes and the same zeroing by the caller) with the first conv and the draw of
 * wae_ar_generate_scalar / wae_ar_generate_scalar_mog (wavenet.py:284-285, 325-333): the current input is a float, w * x + b is the
 * first conv, and after the all-gather of the step's parameters every member runs the same draw on the same bits -- dist 0:
 * sample_from_discretized_mix_logistic (mixture.py:118-156) on u_mix (B,T,M) and draws = u_log (B,T), O = 3M, log scale clamped to
 * log_scale_min when clamp_log_scale != 0; dist 1: sample_from_mix_gaussian (mixture.py:225-270) on u_mix (B,T,M) (NULL allowed when
 * M == 1) and draws = z (B,T), O == 2 or 3M, log scale unclamped (log_scale_min and clamp_log_scale unused).  It is the arithmetic of
 * wae_dmol_sample / wae_mog_sample on the returned parameters, bit for bit.  mode 0: inputs_f (B,T) teacher-forces every step;
 * mode 2: the draws are required, inputs_f (optional) forces steps t < desc.n_forced and the start value is inputs_f[0] (0 without
 * it).  out_samples (B,T) and/or out_params (B,O,T), written by member 0.  B <= 8, C in 1..32, R, S and O <= 256.  The any-shape kernel
 * unless wae_ar_desc.scalar_input = 2 and the shape select the constant-size scalar kernels (see the field; t0 > 0 continuations go
 * through their resume prologue); the split of the sums differs from the one-CU kernel's and between the two kernel forms, so these
 * agree to rounding, not bitwise; error[0] != 0 afterwards means a wait timed out. */
int wae_ar_generate_coop_scalar(const wae_ar_desc* d, int32_t C, int32_t dist, const int32_t* dilations, const int64_t* ring_off,
                                float* ring, int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes,
                                int64_t w2_off_bytes, const float* bias2, const float* zb, const float* first_tab,
                                const float* first_bias, const void* w_head, const float* head_bias, const void* c_up,
                                int32_t c_dtype, const float* inputs_f, const float* u_mix, const float* draws,
                                float log_scale_min, int32_t clamp_log_scale, float* out_samples, float* out_params,
                                uint64_t* msg, float* acc, int32_t* error, void* stream);
/* Work lists of scalar-input utterances: the queue of wae_ar_generate_list / wae_ar_generate_coop_list (items, `next`, slots or teams,
 * rings never zero-filled, longest first) with the first conv and the draw of the scalar entries (wavenet.py:284-285, 300-305, 325-333;
 * mixture.py:118-156, 225-270).  dist as for wae_ar_generate_coop_scalar: 0 = mixture of logistics on u_mix and draws = u_log, O = 3M,
 * log scale clamped to log_scale_min when clamp_log_scale != 0; 1 = mixture of Gaussians on draws = z and u_mix (NULL allowed when
 * M == 1), O == 2 or 3M, log scale unclamped.  The per-step operands are packed item after item by item.off: inputs_f, draws and
 * out_samples (total), u_mix (total, M), out_params one (O, T) block per item at float offset off * O, c_up (total, Ccp); zb holds one
 * (L, 2Hp) row per value of item.row.  Both entries read d->mode.  mode 0: teacher-forced parameters, inputs_f forces every step of
 * every item.  mode 2: sample; the first item.n_forced steps (clamped to [0, T]; 0 with inputs_f == NULL) consume inputs_f[off + t], the
 * rest the fed-back sample; an item whose step 0 is not forced starts from the value 0 (wavenet.py:284-285).  item.init_idx is not read,
 * nor are d->B, d->T, d->n_forced and d->init_idx.
 * wae_ar_generate_scalar_list (csrc/ar_fwd.hip: ar_list_kernel over scalar items): n_slots workgroups, ring n_slots x ring_total; an
 * item's samples and parameters are wae_ar_generate_scalar's / wae_ar_generate_scalar_mog's for that utterance alone, bit for bit (the
 * same device function), whichever slot decodes it and in whatever order.
 * wae_ar_generate_coop_scalar_list (csrc/ar_coop.hip: ar_coop_scalar_list_kernel, the any-shape kernel, or with
 * wae_ar_desc.scalar_input = 2 at the reference's shape the LIST forms of the constant-size scalar kernels): n_teams teams of C
 * workgroups; ring (n_teams, C, ring_total), msg (n_teams, 2, C, NV), acc n_teams x wae_ar_coop_acc_floats(d), error >= 64 ints, the
 * caller zeroes msg, acc, error and next; `total` is the sum of the items' T; error[0] != 0 afterwards: a wait timed out (the output is
 * then invalid).  An item's results are wae_ar_generate_coop_scalar's for that utterance alone at the same C and the same
 * scalar_input value, bit for bit.
 * Refused before any launch (WAE_EINVAL): a class-id decoder; a mode other than 0 / 2; dist outside {0, 1} or O not matching it; mode 2
 * without its draws; u_mix without u_log or the reverse (dist 0); more than one Gaussian without u_mix; mode 0 without inputs_f;
 * out_samples without draws; no output requested; t0 != 0; n_items < 1; n_slots < 1 / n_teams outside 1..8; NULL items or next; and for
 * the cooperative entry C outside 1..32, R, S or O > 256, NULL msg, acc or error, (total + n_items + 1) * (L + 4) >= 2^31. */
int wae_ar_generate_scalar_list(const wae_ar_desc* d, int32_t dist, int32_t n_items, int32_t n_slots, const wae_ar_item* items,
                                int32_t* next, const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                                const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                                const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                                const float* head_bias, const void* c_up, int32_t c_dtype, const float* inputs_f,
                                const float* u_mix, const float* draws, float log_scale_min, int32_t clamp_log_scale,
                                float* out_samples, float* out_params, void* stream);
int wae_ar_generate_coop_scalar_list(const wae_ar_desc* d, int32_t C, int32_t dist, int32_t n_items, int32_t n_teams,
                                     const wae_ar_item* items, int32_t* next, int64_t total, const int32_t* dilations,
                                     const int64_t* ring_off, float* ring, int64_t ring_total, const void* w_layers,
                                     int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2, const float* zb,
                                     const float* first_tab, const float* first_bias, const void* w_head, const float* head_bias,
                                     const void* c_up, int32_t c_dtype, const float* inputs_f, const float* u_mix,
                                     const float* draws, float log_scale_min, int32_t clamp_log_scale, float* out_samples,
                                     float* out_params, uint64_t* msg, float* acc, int32_t* error, void* stream);

/* Work lists of SPANS: the list entries' queue over clips that live longer than a launch (csrc/ar_fwd.hip: ar_span_kernel;
 * csrc/ar_coop.hip: the LIST forms, branching once per record).  A span is a run of consecutive steps of one clip; a clip is decoded
 * as a sequence of spans, in any chunking, over any number of launches, on whichever slot or team takes each span, and its spans'
 * outputs, concatenated, are bit for bit the single decode of that clip -- wae_ar_generate, wae_ar_generate_scalar or
 * wae_ar_generate_scalar_mog on the slots, wae_ar_generate_coop at the same C and kernel form on the teams (the same device
 * functions).  What carries a clip from one span to the next is its own history ring, which belongs to the clip and not to a slot:
 * `ring` is the base of the caller's ring storage and span.ring the float offset of the clip's ring in it (a multiple of 4).
 * Ring per clip: ring_total floats on the one-CU kernels and on the constant-size cooperative kernels, C * ring_total on the
 * any-shape cooperative kernel (wae_ar_coop_ring_floats says which for a cooperative launch).
 * The queue is the list entries': `next` is one int32_t the caller zeroes, taken with one returning atomic add; spans are taken in
 * array order (put the longest first) and no slot or team waits for another.  Ring rows, ring cursors and every "before the clip
 * starts" test use span.t0 + t, exactly as under wae_ar_desc.t0; d->t0 itself must be 0.  The per-step operands of THIS launch
 * (c_up, inputs / inputs_f, uniforms, u_mix, draws, out_idx, out_samples; out_logits / out_params one (O, span.T) block per span at
 * float offset off * O) are indexed from span.off; zb holds one (L, 2Hp) row per value of span.row.
 * The first step of a continuation (t0 > 0) is forced: the caller puts the previous span's last output, or the teacher-forced value,
 * at inputs[off] / inputs_f[off]; a record with t0 > 0 and n_forced < 1 is read as n_forced = 1.  span.n_forced counts from the span's
 * first step (clamped to [0, T]; mode 0 forces every step); span.init_idx is read only when t0 == 0 and nothing is forced.
 * THE CALLER'S CONTRACT, which the entries cannot check because the records live in device memory: one launch holds at most one span
 * of any clip (two spans of a clip in one launch could run at the same time on two slots); a span with t0 > 0 continues in the ring
 * the clip's earlier spans -- same geometry, weights, dtype, C, kernel form -- left for steps [0, t0); span.reserved is 0.
 * One-CU kernels and the any-shape cooperative kernel: nothing is cleared; a history row is read only behind its own write, by
 * absolute index.  Constant-size cooperative kernels: a span with t0 == 0 gets the list form's clearing of its clip's ring (drain,
 * rendezvous A -- which here also hands the team the span index --, clear, rendezvous B); a span with t0 > 0 keeps its rows and starts
 * from the single decode's continuation prologue (cursors at t0 mod ring length, the first step's two history taps read from the
 * ring); the weight packets stay on chip across spans and only the resident layers' two zb words are rewritten per span.  The
 * exchange sequence numbers run on across a team's spans, as across items.
 * wae_ar_generate_spans: class ids on n_slots one-CU workgroups, modes 0 / 1 / 2, the operands of wae_ar_generate_list.
 * wae_ar_generate_scalar_spans: dist 0 / 1 on n_slots one-CU workgroups, modes 0 / 2, the operands of wae_ar_generate_scalar_list.
 * wae_ar_generate_coop_spans: class ids on n_teams <= 8 teams of C workgroups, modes 0 / 1 / 2, the operands of
 *   wae_ar_generate_coop_list (msg, acc, error and next zeroed by the caller per launch; error[0] != 0 afterwards: a wait timed out).
 * wae_ar_generate_coop_scalar_spans: dist 0 / 1 on n_teams <= 8 teams of C workgroups, modes 0 / 2, the operands of
 *   wae_ar_generate_coop_scalar_list with wae_ar_span records (msg, acc, error and next zeroed by the caller per launch); it
 *   dispatches as its list twin does (wae_ar_desc.scalar_input), and a clip's spans, concatenated, are bit for bit
 *   wae_ar_generate_coop_scalar's decode of that clip at the same C and the same scalar_input value.
 * Refused before any launch: whatever the list twin refuses (WAE_EUNSUPPORTED / WAE_EINVAL as there), d->t0 != 0 among it; the
 * cooperative entries also (total + n_spans + 1) * (L + 4) >= 2^31, total being the length of the packed operands.
 * Rates (profiles/ar_session.txt, all measured, bf16 at the reference's geometry): 8 clips on 8 teams in spans of 1600 steps 30.7 kHz per
 * clip against 31 kHz in one launch, 16 clips on 8 teams 15.3 kHz per clip, a relaunch with its packing ~0.45 ms per round on the
 * teams; scalar team sessions on the constant-size kernels (profiles/ar_scalar_fast.txt, bf16): 8 clips 31.7 kHz per clip in spans of
 * 1600 steps, 16 clips 15.9 kHz per clip; fp32 sessions have not been measured. */
typedef struct wae_ar_span {
  int64_t off;       /* first step of the span in THIS launch's packed per-step operands (as wae_ar_item.off) */
  int64_t ring;      /* float offset of the clip's own history ring inside `ring` */
  int32_t T;         /* steps of the span (<= 0: skipped) */
  int32_t t0;        /* absolute index of the span's first step in its clip; the ring holds steps [0, t0) */
  int32_t n_forced;  /* span-relative, as wae_ar_desc.n_forced under streaming: a span with t0 > 0 forces at least its first step */
  int32_t init_idx;  /* read only when t0 == 0 and nothing is forced */
  int32_t row;       /* row of zb */
  int32_t reserved;  /* 0 */
} wae_ar_span;       /* 40 bytes */
int wae_ar_generate_spans(const wae_ar_desc* d, int32_t n_spans, int32_t n_slots, const wae_ar_span* spans, int32_t* next,
                          const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                          const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                          const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                          const float* head_bias, const void* c_up, int32_t c_dtype, const int32_t* inputs,
                          const float* uniforms, int32_t* out_idx, float* out_logits, void* stream);
int wae_ar_generate_scalar_spans(const wae_ar_desc* d, int32_t dist, int32_t n_spans, int32_t n_slots, const wae_ar_span* spans,
                                 int32_t* next, const int32_t* dilations, const int64_t* ring_off, float* ring, int64_t ring_total,
                                 const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2,
                                 const float* zb, const float* first_tab, const float* first_bias, const void* w_head,
                                 const float* head_bias, const void* c_up, int32_t c_dtype, const float* inputs_f,
                                 const float* u_mix, const float* draws, float log_scale_min, int32_t clamp_log_scale,
                                 float* out_samples, float* out_params, void* stream);
int wae_ar_generate_coop_spans(const wae_ar_desc* d, int32_t C, int32_t n_spans, int32_t n_teams, const wae_ar_span* spans,
                               int32_t* next, int64_t total, const int32_t* dilations, const int64_t* ring_off, float* ring,
                               int64_t ring_total, const void* w_layers, int64_t layer_stride_bytes, int64_t w2_off_bytes,
                               const float* bias2, const float* zb, const float* first_tab, const float* first_bias,
                               const void* w_head, const float* head_bias, const void* c_up, int32_t c_dtype,
                               const int32_t* inputs, const float* uniforms, int32_t* out_idx, float* out_logits,
                               uint64_t* msg, float* acc, int32_t* error, void* stream);
int wae_ar_generate_coop_scalar_spans(const wae_ar_desc* d, int32_t C, int32_t dist, int32_t n_spans, int32_t n_teams,
                                      const wae_ar_span* spans, int32_t* next, int64_t total, const int32_t* dilations,
                                      const int64_t* ring_off, float* ring, int64_t ring_total, const void* w_layers,
                                      int64_t layer_stride_bytes, int64_t w2_off_bytes, const float* bias2, const float* zb,
                                      const float* first_tab, const float* first_bias, const void* w_head, const float* head_bias,
                                      const void* c_up, int32_t c_dtype, const float* inputs_f, const float* u_mix,
                                      const float* draws, float log_scale_min, int32_t clamp_log_scale, float* out_samples,
                                      float* out_params, uint64_t* msg, float* acc, int32_t* error, void* stream);
/* Floats of ONE clip's ring under wae_ar_generate_coop_spans / wae_ar_generate_coop_scalar_spans for this descriptor, C and ring_total:
 * ring_total where the launch takes the constant-size kernels (their members share one ring) -- for a scalar-input descriptor that
 * needs scalar_input = 2 --, C * ring_total on the any-shape kernel; < 0: bad arguments. */
int64_t wae_ar_coop_ring_floats(const wae_ar_desc* d, int32_t C, int64_t ring_total);

/* ---- backward data path of the gated stack: C[t][M] = sum_s W_s . X_s[t + shift_s] on time-major operands ----
 * (autograd of modules.py:115-163; see csrc/gemm_tm.hip).  mode 0: out (t, M) = acc.  mode 1 (residual):
 * out = alpha * (acc + aux[t]).  mode 2 (gate backward): acc = du over M = Hp rows, aux = z (t, 2Hp),
 * out (t, 2Hp) = [du*sigmoid(b)*(1-tanh(a)^2) | du*tanh(a)*sigmoid(b)*(1-sigmoid(b))].
 * The four *_host arguments are HOST arrays of nsrc entries (device pointers, strides, cols, shifts).
 * Sources: nsrc <= 4 time-major arrays (row stride in elements, cols a multiple of 64 bf16 / 32 fp32), row t+shift,
 * zero outside the clip.  w_packed: [sum cols / CK] chunks of (M/32) x 4 fragment blocks (first-GEMM order). */
typedef struct wae_tm_desc {
  int32_t dtype;
  int32_t B, T;
  int32_t M;    /* output rows, multiple of 32: M/32 in {1,2,3,4,6,8}, or (modes 0/1/3/4) any multiple of 128: the output is then
                   cut into equal slices of 8, 6 or 4 tiles and w_packed is [slice][chunk] (packing.py: first_gemm_map) */
  int32_t nsrc;
  int32_t mode;
  float alpha;
  int32_t flags; /* WAE_TM_INTERLEAVE: the chunk stream visits the (equally wide) sources round-robin per 128-byte column
                    block -- [block 0 of source 0, of source 1, ..., block 1 of source 0, ...] -- instead of source by source:
                    the dilated taps of one column block are then read back to back, while the tiles d and 2d rows away
                    fetch the same rows into the same L2 (w_packed follows the same order) */
} wae_tm_desc;
#define WAE_TM_INTERLEAVE 1
#define WAE_TM_ONE_WG 2   /* bf16 gate-backward / residual / ReLU-backward launches: one 4-wave workgroup per CU with the 8 KiB
                             staging tiles instead of two per CU (same results; an A/B switch per launch).  It also keeps a mode-1 / -2 / -3
                             launch on this generic kernel where csrc/gemm_tm8.hip (below) has an instantiation. */
/* Mode 3 with ONE source, no shift, 16-bit storage, M a multiple of 256 and an even chunk count (the head's skip contraction, the
 * wide head's h0 / h1 launches) runs on csrc/gemm_tm8.hip since round 6: 8 consumer + 4 loader waves per workgroup, 256 time columns,
 * both operands by LDS-DMA -- same packed stream, same accumulation order, bit-identical outputs (170 against 196 us at C2). */
/* Modes 1 (interleaved taps of ONE array, M a multiple of 256) and 2 (M = Hp in {256, 192, 128}) in 16-bit storage with an even chunk
 * count run on gemm_tm8x_kernel of the same file since round 6: 256 columns per workgroup, both operand streams by LDS-DMA, the
 * eight waves sharing the requests (csrc/glu_bwd8.hip's schedule); bit for bit the generic kernel's results. */
/* (flag value 4 was WAE_TM_BLDS, the 8-wave LDS-staged-operand shape of rounds 3-4: measured not faster, removed in round 5) */
int wae_gemm_tm(const wae_tm_desc* d, const void* const* src_host, const int64_t* src_stride_host,
                const int32_t* src_cols_host, const int32_t* src_shift_host, const void* w_packed, void* out,
                int64_t out_stride, const void* aux, int64_t aux_stride, void* stream);

/* Wide decoder head: skip / head widths above 256 (BASELINE config C5: R = S = 512) do not fit the register-chained
 * wae_head_fwd / wae_head_bwd; the same arithmetic (wavenet.py:204-214, vqwae_train.py:363-379 with the shift of :764)
 * then runs as launches of the kernel above with epilogues, h0 / h1 / dy / dh1 passing through HBM:
 *   mode 3: out = relu(alpha * (bias[m] + acc)), aux = fp32 bias (M floats, aux_stride ignored)
 *   mode 4: out = aux[t][m] > 0 ? alpha * acc : 0, aux = the saved activation (t, M) in the compute dtype
 *   mode 5 (wae_gemm_tm_ce): acc = bias + W3 h1 over M = Op in {128, 256} padded classes; ce->logits (B,O,T) fp32 and / or
 *           ce->nll[b,t] = lse - y[target[t+1]] (0 at t = T-1), ce->lse optional; `out` unused
 *   mode 6 (wae_gemm_tm_ce): out (t, Op) = (exp(bias + acc - ce->lse[t]) - onehot(target[t+1])) * w[t],
 *           w[t] = ce->inv_count if t + 1 < min(lengths[b], T) else 0 (lengths == NULL: T) */
typedef struct wae_tm_ce {
  float* logits;
  const int32_t* target;
  float* nll;
  float* lse;
  const int32_t* lengths;
  float inv_count;
  int32_t O;
} wae_tm_ce;
int wae_gemm_tm_ce(const wae_tm_desc* d, const void* const* src_host, const int64_t* src_stride_host,
                   const int32_t* src_cols_host, const int32_t* src_shift_host, const void* w_packed, void* out,
                   int64_t out_stride, const float* bias, const wae_tm_ce* ce, void* stream);

/* ---- weight gradients: C[m][n] += alpha * sum_{b,t} P[b,t][m] * Q[b,t+shift][n]  (csrc/gemm_tn.hip) ----------
 * The work is described as an array of 128x128 output tiles in DEVICE memory; one launch processes them all (the
 * several weight gradients of a layer share a launch).  P, Q: time-major dtype arrays, pointers already offset to the
 * tile's first column, of which the first m_valid / n_valid columns take part.  onehot != NULL: P[t][m] =
 * (onehot[b*T+t] == m0 + m) (first-conv gradient).  ones_col >= 0: a virtual all-ones Q column at that tile-local
 * index; clip b accumulates sum_t P[b,t][m] into C[m][ones_col + b] (bias / per-clip conditioning-bias gradients).
 * Each tile is contracted over the time range of one clip split `splits` ways; results are added with fp32 atomics
 * (not bitwise reproducible run to run).
 * Preconditions: P and Q are read in 16-byte pieces -- pointers 16-byte aligned, p_stride / q_stride multiples of 16 bytes, and
 * the piece that holds the last valid column is read whole (any 0 <= m_valid, n_valid <= 128 is permitted, odd ones included,
 * while the row is readable up to the next multiple of 16 bytes; what lies there never reaches C).  ones_col + B <= 128 and
 * shift == 0 with ones_col >= 0: under a shift the three launches disagree on which rows the sums cover.  ones_col < n_valid is
 * permitted here (not in the team launches): the stored Q column of that index is ignored, and C columns ones_col + 1 ..
 * ones_col + B - 1 then receive both their own contraction and a clip's sums.  splits may exceed ceil(T / 32) (it is then
 * ceil(T / 32)).  C rows from m_valid on and C columns outside [0, n_valid) and [ones_col, ones_col + B) are never written. */
typedef struct wae_tn_tile {
  const void* P;
  const void* Q;
  const int32_t* onehot;
  float* C;
  int64_t p_stride, q_stride, ldc;
  int32_t m_valid, n_valid;
  int32_t m0;
  int32_t shift;
  int32_t ones_col;
  float alpha;
} wae_tn_tile;
int wae_gemm_tn_tiles(int32_t dtype, const wae_tn_tile* tiles_dev, int32_t ntiles, int32_t B, int32_t T, int32_t splits,
                      void* stream);
/* The same contraction with its sums formed in a FIXED ORDER (the deterministic train step): two launches, no workgroup waits for
 * another, no floating-point atomics.  Tile records, preconditions and what is never written are wae_gemm_tn_tiles'.
 *   Launch 1: the workgroup of the logical (tile i, kr = clip b * nsp + split s) -- nsp = the splits the launch really makes, as in
 *     wae_gemm_tn_tiles -- stores alpha * (its MFMA sum over its time range) into slot (i, kr) of `partials`, a [ntiles][B * nsp][128][128]
 *     fp32 array.  Every element launch 2 reads is stored exactly once per launch (zeros for an empty time range), so the buffer
 *     needs no clearing and may be reused by the next call on the same stream.
 *   Launch 2: one thread per element (row, c) of a tile's window, row < m_valid.  THE ORDER BELOW IS THE DEFINITION OF THE RESULT:
 *       data = ((slot[0] + slot[1]) + slot[2]) + ... + slot[B * nsp - 1]   at [row][c]: clip-major, split-minor; taken when
 *              c < n_valid and c != ones_col;
 *       ones = (slot[b * nsp] + slot[b * nsp + 1]) + ... + slot[b * nsp + nsp - 1]   at [row][ones_col]: clip b's splits only; taken
 *              when c == ones_col + b for a clip 0 <= b < B;
 *       C[row][c] = C[row][c] + data, + ones, or + (data + ones) -- ONE plain read-modify-write of fp32 adds, started from the first
 *       partial (not from zero).  Ones columns at or beyond tile-local 128 are added the same way, each alone.
 * partials_floats < wae_gemm_tn_tiles_det_floats(ntiles, B, T, splits): WAE_EINVAL, nothing launched.
 * ordered = 0: one reduce launch over all tiles; the caller guarantees that no two tiles of the table touch the same element of C
 *   (windows and ones columns; backward.py: TileTable.finalize checks it on the host).
 * ordered = 1: one reduce launch per tile, in table order: tiles that share C are added one after another in that order.
 * Within one device model and build the result is a function of the operands, C's previous contents, B, T, splits and the table. */
int64_t wae_gemm_tn_tiles_det_floats(int32_t ntiles, int32_t B, int32_t T, int32_t splits);
int wae_gemm_tn_tiles_det(int32_t dtype, const wae_tn_tile* tiles_dev, int32_t ntiles, int32_t B, int32_t T, int32_t splits,
                          float* partials, int64_t partials_floats, int32_t ordered, void* stream);

/* ---- backward data path across one layer boundary, fused (csrc/glu_bwd.hip; autograd of modules.py:115-163) ----------
 *   dx_l-hat = alpha * (dx_{l+1}-hat + sum_tap W1_l,tap^T dz_l[t + (k-1-tap) d])   -> g_out (B,T,Rp), also kept in registers
 *   dz_{l-1} = gate'(z_{l-1}) * (W_out_{l-1}^T dx_l-hat + W_skip_{l-1}^T dskip)    -> dz_prev (B,T,dz_stride)
 * = wae_gemm_tm mode 1 for layer l followed by mode 2 for layer l-1, without re-reading dx_l-hat.  dz / dz_prev point at
 * the layers' 2Hp columns inside the (B,T,dz_stride) buffer; z_prev is (B,T,2Hp); w_x = the mode-1 weights of layer l,
 * w_uo = W_out_{l-1}^T in accumulator-row k order (packing.py: bwd_uo_map), w_us = the W_skip part of the mode-2 weights.
 * wae_glu_bwd_fused_supported(Rp, Hp) tells whether an fp32 instance exists (else use the two wae_gemm_tm launches),
 * wae_glu_bwd_fused_supported16 the same for 16-bit storage.  16-bit storage runs the two-workgroups-per-CU form of round 5
 * (csrc/glu_bwd.hip: glu_bwd_pair_kernel), which takes w_x in the INTERLEAVED chunk order of wae_gemm_tm mode 1 with
 * WAE_TM_INTERLEAVE (packing.py: bwd_x_map) -- dx_l-hat is then bitwise what that launch stores; fp32 takes w_x tap by tap. */
typedef struct wae_glu_bwd_desc {
  int32_t dtype, B, T, Rp, Hp, Sp, ktaps, dilation;
  float alpha;
} wae_glu_bwd_desc;
int wae_glu_bwd_fused_supported(int32_t Rp, int32_t Hp);
int wae_glu_bwd_fused_supported16(int32_t Rp, int32_t Hp);
int wae_glu_bwd_fused(const wae_glu_bwd_desc* d, const void* dz, int64_t dz_stride, const void* g_next, void* g_out,
                      const void* dskip, const void* z_prev, void* dz_prev, const void* w_x, const void* w_uo,
                      const void* w_us, void* stream);
/* 16-bit storage, three taps, Ccp = 64: the same launch with the conditioning gradient folded in (round 5).  dc = sum_l Wc_l^T dz_l
 * (the ONE K = L * 2Hp launch of wae_gemm_tm mode 0 that re-reads every layer's dz) rides on phase A's shift-0 tap, whose operand
 * fragments are dz_l[t]: w_c = layer l's 2Hp / 64 chunks (8 KiB each) of that launch's weight stream (packing.py: bwd_c_map), dc_acc =
 * the fp32 (B,T,64) running sum over the layers, dc_mode bit 0: add dc_acc's previous content (clear: the first launch of a sweep),
 * bit 1: write the sum in the storage dtype to dc_out (B,T,64) instead (the last launch of the sweep).  last = 1: layer 0 -- phase A +
 * its epilogue only (z_prev / dz_prev / w_uo / w_us are not used but must be valid pointers).
 * Rp = 256, Sp = 256, Hp in {128, 192} (BASELINE C2, hps/vqwae.json) run csrc/glu_bwd8.hip since round 6 -- 8 waves x 256 columns, one
 * workgroup per CU, weights AND activation operands through LDS (77.6 against 84 us per launch at C2), bitwise the 4-wave kernel's
 * results; dc_mode bit 2 keeps the 4-wave kernel (the A/B and parity handle of tests/ and tools/time_pair.py). */
int wae_glu_bwd_fused_dc(const wae_glu_bwd_desc* d, const void* dz, int64_t dz_stride, const void* g_next, void* g_out,
                         const void* dskip, const void* z_prev, void* dz_prev, const void* w_x, const void* w_uo,
                         const void* w_us, const void* w_c, float* dc_acc, void* dc_out, int32_t dc_mode, int32_t last,
                         void* stream);

/* ---- all weight-gradient contractions of a step in one launch (csrc/gemm_tn_stream.hip; bf16 operands only) ------
 * Same contraction as wae_gemm_tn_tiles, C[m][n] += alpha * sum_{b,t} P[b,t][m] * Q[b,t+shift][n], cut differently:
 * a job is one 384 x 256 output region over the whole batch; the (job, 32-row time slab) list is cut into one
 * contiguous share per workgroup (segments), so a launch of nwg ~ #CUs workgroups finishes all jobs together and adds
 * each region to C once per (workgroup, job) boundary.  jobs/segs/team_seg are device arrays built by the host
 * (backward.py: StreamTable).  team_size consecutive workgroups form a team that walks one segment list, member m on
 * job (segment job + m) -- the jobs of one layer share operands; team_seg has nteams + 1 prefix offsets into segs;
 * slabs are numbered b * ceil(T/32) + t / 32; a job with m_valid == 0 is skipped; nwg >= nteams * team_size.
 * m_valid <= 384, n_valid <= 256; n_valid % 8 == 0 when ones_col >= 0 (n_valid <= ones_col < 256).
 * Preconditions: operands move in 16-byte units -- P / Q pointers 16-byte aligned, p_stride / q_stride multiples of 8 elements,
 * m_valid and n_valid multiples of 8; ones_col + B <= 256 and shift == 0 with ones_col >= 0 (rows whose Q partner lies outside
 * the clip are dropped from the sums as well); B <= 64; every segment has job + team_size <= the number of job records and
 * 0 <= slab_begin <= slab_end <= B * ceil(T / 32) (an empty segment and a team without segments are permitted); each (job, slab)
 * pair is contracted once per segment that covers it. */
typedef struct wae_ts_job {
  const void* P;
  const void* Q;
  float* C;
  int64_t p_stride, q_stride, ldc;
  int32_t m_valid, n_valid;
  int32_t shift;
  int32_t ones_col;
  float alpha;
  int32_t pad_;
} wae_ts_job;
typedef struct wae_ts_seg {
  int32_t job, slab_begin, slab_end;
} wae_ts_seg;
/* pace: nteams x 8 int32, ZEROED by the caller before every launch (or NULL / window <= 0: no pacing): members [0, pace_from) of
 * a team (the full-size jobs: the taps) publish the slab position of their next request, and members [pace_from, team_size) (the
 * narrow jobs, which would run ahead) request no more than `window` slabs beyond the slowest of them, so that the operand slabs
 * the jobs of a layer share are fetched from HBM once and found in the XCD's L2 by the others.  Timing only: results do not
 * depend on it, and a wait that does not end switches it off (the launch can never hang). */
int wae_gemm_tn_stream(int32_t dtype /* WAE_BF16 or WAE_F16 */, const wae_ts_job* jobs_dev, const wae_ts_seg* segs_dev,
                       const int32_t* team_seg_dev, int32_t nteams, int32_t team_size, int32_t nwg, int32_t B, int32_t T,
                       int32_t* pace, int32_t window, int32_t pace_from, void* stream);

/* ---- the same launch on a static schedule (csrc/gemm_tn_static.hip; 16-bit operands; round 4) -----------------------
 * Replaces the autograd of modules.py:134-136 (dilated conv: kind TAPS, one job per tap), :141-145 (conv1x1c + the per-clip
 * sums of dz that feed the conv bias and conv1x1g: kind COND) and :157-160 (conv1x1_out AND conv1x1_skip, which contract the
 * same gated activations u: kind OUTSKIP, C0[h][r] += sum u[t][h] Ghat[t][r], C1[h][s] += sum u[t][h] dS[t][s], Cb[r] += sum
 * Ghat[t][r]) for geometries that fit one region: m_valid <= 384 (TAPS / COND) or 192 (OUTSKIP), n0_valid, n1_valid <= 256
 * (COND: <= 64), B <= 32, every operand clip below 2^30 bytes.  Teams, segments and slab numbering as wae_gemm_tn_stream.
 * Rows outside a clip (a tap's causal shift, T % 32 != 0) are zero-filled by the hardware through per-clip buffer
 * descriptors; OUTSKIP's outputs are TRANSPOSED relative to the reference's weight layout (rows = gated channel h).
 * The same kinds carry the rest of the step's weight gradients (one more group of jobs; backward.py: static_head): the head's
 * 1x1 convolutions (wavenet.py:136-141) as TAPS jobs with shift 0 (P = dy, Q0 = h1; P = dh1, Q0 = h0), their biases as COND jobs
 * WITHOUT a Q operand (Q0 = NULL, n0_valid = 0: only the per-clip column sums of P, at ones_col), first_conv (wavenet.py:119-122,
 * 203) as a TAPS job whose P is the one-hot operand of wae_onehot_rows, and -- the last layer's conv1x1_out gradient being dead
 * (wavenet.py:205-207) -- dS as Q0 of that layer's OUTSKIP job, whose Cb then is the skip bias gradient.  A record with
 * m_valid <= 0 is a null job (its team member skips the segment).
 * Preconditions: shift <= 0 on every job; m_valid, n0_valid, n1_valid multiples of 8, operand pointers 16-byte aligned and
 * strides multiples of 8 elements (16-byte requests; a partly valid unit would be zero-filled whole); COND's sums and OUTSKIP's Cb
 * are defined for shift == 0 only (the slabs a shift skips, and the rows t >= T it brings into range, would otherwise enter or
 * leave them); COND writes C0 columns [0, n0_valid) and [ones_col, ones_col + B), which must lie inside ldc0; n1_valid == 0 goes
 * with Q1 = C1 = NULL; segments as for wae_gemm_tn_stream. */
enum { WAE_TQ_TAPS = 0, WAE_TQ_COND = 1, WAE_TQ_OUTSKIP = 2 };
typedef struct wae_tq_job {
  const void* P;
  const void* Q0;
  const void* Q1;
  float* C0;
  float* C1;
  float* Cb;
  int64_t p_stride, q0_stride, q1_stride, ldc0, ldc1;
  int32_t m_valid, n0_valid, n1_valid;
  int32_t shift;
  int32_t ones_col;   /* COND: column of clip 0's sums in C0 (a multiple of 32, >= n0_valid); clip b adds into ones_col + b */
  int32_t kind;
  float alpha;
  int32_t pad_;
} wae_tq_job;
/* stamps: NULL, or (diagnostic builds, -DWAE_TQ_STAMPS) nwg x 16 x 4 int64 zeroed by the caller.
 * pace: nteams uint32, ZEROED by the caller before every launch (or NULL / window <= 0: no pacing): every tap member adds its
 * request progress (in 32-row slabs; a team's share must stay below 1000 slabs) to its 10-bit field, and every TAPS / COND member
 * requests no more than `window` slabs beyond the slowest other tap member, so that the dz half-slabs four jobs of a layer share
 * are fetched from HBM once and found in the XCD's L2 by the others (window_cond: the bound of the COND member; negative = it stays
 * that many slabs behind the slowest tap).  Timing only: results do not depend on it, and a wait that
 * does not end switches it off.
 * max_clip_bytes: the caller's statement of the largest operand clip of the job table, (T + the largest |shift| + 32) rows x the
 * widest p / q row in bytes; refused (WAE_EINVAL) at 2^30 or more, because rows outside a clip are zero-filled by the range check
 * of a per-clip buffer descriptor with 32-bit offsets. */
int wae_gemm_tn_static(int32_t dtype /* WAE_BF16 or WAE_F16 */, const wae_tq_job* jobs_dev, const wae_ts_seg* segs_dev,
                       const int32_t* team_seg_dev, int32_t nteams, int32_t team_size, int32_t nwg, int32_t B, int32_t T,
                       int64_t* stamps, uint32_t* pace, int32_t window, int32_t window_cond, int32_t ntaps, int64_t max_clip_bytes,
                       void* stream);

/* ---- backward of the front end (csrc/frontend_bwd.hip) -----------------------------------------------------
 * upsample stage: dout (B,C,Tin*s), in (B,C,Tin) -> din (B,C,Tin), dw[2s+1] += (atomics).
 * conv block: dpre = dy * [relu ? (y - (residual ? x : 0)) > 0 : 1]; dx (or NULL), dw +=, dbias += (or NULL).
 * VQ: dlat = dquant + loss_scale*2*beta*(x-q)/N; demb[idx] += loss_scale*2*(q-x)/N (straight-through estimator). */
int wae_upsample_stage_bwd(const float* dout, const float* in, const float* w, float* din, float* dw, int32_t B,
                           int32_t C, int32_t Tin, int32_t s, void* stream);
int wae_enc_conv_bwd(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw,
                     float* dbias, int32_t B, int32_t Cin, int32_t Tin, int32_t Cout, int32_t k, int32_t stride,
                     int32_t pad, int32_t relu, int32_t residual, void* stream);
int wae_vq_bwd(const float* lat, const float* quant, const int64_t* idx, const float* dquant, float* dlat, float* demb,
               int32_t B, int32_t D, int32_t Tq, float beta, float loss_scale, void* stream);

/* ---- backward of the front end over a LIST of utterances of unequal lengths (csrc/frontend_bwd_list.hip): the second half of a
 * ragged train step (WaeEngine.train_step_list).  The decoder needs no list form: in a right-padded batch a valid row reads nothing
 * to its right, and under a masked loss a pad row sends no gradient to its left.  What zero-padding changes is the front end, so its
 * forward runs on the packed list (wae_enc_conv_fwd_list, wae_upsample_stage_fwd_list) and these three entries are its backward.
 * Each takes the packed layout and the tables of its forward twin (packing.encode_list_plan / upsample_list_plan records serve
 * both ways), enqueues on `stream`, never allocates or synchronises, and returns WAE_EINVAL / WAE_EUNSUPPORTED before any launch.
 * No entry trusts a table with memory: a record that does not fit its pitches or contradicts the length formula is skipped whole,
 * nothing read or written for it.  Every item is zero-padded at its own two ends: a tap outside the item contributes nothing and
 * never reads the neighbour's column.  Per item the gradients are those of the dense entries above for that item as a batch of one;
 * weight gradients are the sums over the items, ADDED into what dw / dbias hold.  Not reproducible to the bit from run to run where
 * float atomics add (the stage's dw); there is no deterministic form.
 * The QUANTISER needs no list entry in either direction: wae_vq_nearest / wae_vq_search_slices, wae_vq_ema_update and wae_vq_bwd /
 * wae_vq_slice_bwd run on the packed latents (Cc, sum Tq_i) with B = 1, Tq = pitch; their mean over Cc * sum Tq_i is the
 * list-as-one-batch convention of wae_vq_stats_segments' `out`.  The latent buffer must then have NO GAP COLUMNS: pitch == sum Tq_i
 * (a gap column would be searched, counted and averaged like a frame).
 *
 * wae_from_btc_list, the inverse of wae_to_btc_list: rows [out_off_i, out_off_i + Tin_i) of the time-major `in` (rows, Cp) in
 *   `dtype` -> columns [in_off_i, in_off_i + Tin_i) of the channel-major `out` (C, pitch) fp32, every element times `scale` (the
 *   conditioning gradient dc -> the packed gradient, with 1 / grad_scale).  Records wae_ups_seg + the closing one, tiles of 64 rows
 *   (wae_to_btc_list's table); a record with out_off_i + Tin_i > rows or in_off_i + Tin_i > pitch is skipped.  Columns that no item
 *   owns are not written.  WAE_EINVAL: a null pointer, C, nsegs, ntiles, pitch or rows < 1, Cp < C, a bad dtype.
 * wae_upsample_stage_bwd_list, wae_upsample_stage_bwd for every item in one launch: dout (C, out_pitch), item i at the columns
 *   [out_off_i, out_off_i + Tin_i s); in (C, in_pitch) the stage's packed input; din (C, in_pitch) receives the item's columns;
 *   dw[2s+1] += the sum over all items (float atomics; wae_upsample_stage_bwd_list_det: in a fixed order).  Records wae_ups_seg + the closing one with tiles of WAE_UPS_LIST_TILE_CT
 *   output columns: the channel-major table of wae_upsample_stage_fwd_list.  WAE_EINVAL: a null pointer, C, s, nsegs, ntiles or a
 *   pitch < 1, s > 16 (as the dense entry).
 * wae_enc_conv_bwd_list, wae_enc_conv_bwd over wae_seg records and the (segment, to0) tile table of wae_enc_conv_fwd_list: x
 *   (Cin, in_pitch), y (or NULL without relu) and dy (Cout, out_pitch); dx (Cin, in_pitch) or NULL (the first block); dw += and
 *   dbias += (or NULL).  dpre = dy * [relu ? (y - (residual ? x : 0)) > 0 : 1], as the dense kernel forms it; a tap outside
 *   [0, Tin_i) reads 0.  The tile (i, to0) also stands for the item's input steps [to0 stride, (to0 + et) stride) -- the item's last
 *   tile for everything up to Tin_i -- so the table must hold the tiles enc_list_tables builds: multiples of et below Tout_i, each
 *   once.  Every (32 output x 32 input channel) block of dw has ONE owner, which walks the tiles in table order and adds its sum with
 *   a plain read-modify-write: for a given table the result is reproducible, and in exact arithmetic it does not depend on the
 *   table's order.  Serves the ten encoder blocks, lin and conv_in.  WAE_EINVAL as wae_enc_conv_fwd_list, and for relu without y;
 *   WAE_EUNSUPPORTED for a (k, stride) other than (1,1), (3,1), (5,2), (5,1). */
int wae_from_btc_list(const void* in, float* out, const wae_ups_seg* segs, int32_t nsegs, int32_t ntiles, int32_t pitch, int32_t rows,
                      int32_t C, int32_t Cp, int32_t dtype, float scale, void* stream);
int wae_upsample_stage_bwd_list(const float* dout, const float* in, const float* w, float* din, float* dw, const wae_ups_seg* segs,
                                int32_t nsegs, int32_t ntiles, int32_t in_pitch, int32_t out_pitch, int32_t C, int32_t s, void* stream);
int wae_enc_conv_bwd_list(const float* x, const float* w, const float* y, const float* dy, float* dx, float* dw, float* dbias,
                          const wae_seg* segs, int32_t nsegs, const int32_t* tiles, int32_t ntiles, int32_t et, int32_t in_pitch,
                          int32_t out_pitch, int32_t Cin, int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t relu,
                          int32_t residual, void* stream);

/* layout helpers: (B,C,T) fp32 <-> (B,T,Cp) dtype */
int wae_to_btc(const float* in, void* out, int32_t B, int32_t C, int32_t T, int32_t Cp, int32_t dtype, void* stream);
/* the same with the shifted loss mask and weight of vqwae_train.py:374-379,764-766 applied on the way: row t is multiplied by
 * `scale` while t + 1 < min(lengths[b], T) (lengths == NULL: T) and zeroed otherwise -- d loss / d y_hat of the masked mean
 * of a per-step loss (the discretized mixture of logistics, mixture.py:26-106) in the layout wae_head_bwd takes as ext_dy */
int wae_to_btc_masked(const float* in, void* out, int32_t B, int32_t C, int32_t T, int32_t Cp, int32_t dtype,
                      const int32_t* lengths, float scale, void* stream);
int wae_from_btc(const void* in, float* out, int32_t B, int32_t C, int32_t T, int32_t Cp, int32_t dtype, void* stream);
/* wae_from_btc with every element multiplied by `scale` (fp16 runs: undoes the loss scale where the conditioning gradient
 * leaves the 16-bit stack for the fp32 front end) */
int wae_from_btc_scaled(const void* in, float* out, int32_t B, int32_t C, int32_t T, int32_t Cp, int32_t dtype, float scale,
                        void* stream);
/* upsample_activation (upsample.py:44-46): the element-wise module the reference puts behind every stage's smoothing FIR --
 * kind 1 nn.ReLU, 2 nn.LeakyReLU(negative_slope = slope), 3 nn.Tanh, 4 nn.Sigmoid.  wae_act_fwd: x <- act(x) in place (fp32);
 * wae_act_bwd: d <- d * act'(.) formed from the activation's OUTPUT y. */
int wae_act_fwd(float* x, int64_t n, int32_t kind, float slope, void* stream);
int wae_act_bwd(const float* y, float* d, int64_t n, int32_t kind, float slope, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAE_H */
