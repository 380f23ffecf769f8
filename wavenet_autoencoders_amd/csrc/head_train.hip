// wae_head_train_from_h0: the training head in ONE launch -- the second half of the head's forward (head_fwd.hip, FROM_H0), the masked
// mean of the cross-entropy and the head's backward (head_bwd.hip) down to dskip, for 16-bit engines with Sp == Op:
//
//   h1 = relu(b1 + W1 h0)                                   GEMM 1   -> h1 stored (operand of the weight gradients)
//   y  = b3 + W3 h1                                         GEMM 2   logits stay in the accumulator registers
//   nll[t] = lse(y) - y[target[t+1]]                                 -> nll, lse; per-workgroup partial of the masked sum
//   dy  = (softmax(y) - onehot(target[t+1])) * w[t]                  -> dy stored,  w[t] = [t < len-1] * dy_factor
//   dh1 = (W3^T dy) * [h1 > 0]                              GEMM b   -> dh1 stored
//   dskip = (W1^T dh1) * [h0 > 0] * sqrt(1/L)               GEMM c   -> dskip stored
//
// head_bwd.hip recomputes y from the stored h1 (a fourth GEMM) and reloads h1 and h0 through the staging tile for the two relu masks;
// here the logits never leave the registers and the masks are kept as bits (NT*16 per lane and mask).  Schedule: head_fwd_kernel<FROM_H0>'s
// 8 waves x 256 columns, one workgroup per CU, the 4*NT/2 weight chunks through a three-slot LDS ring two chunks ahead under counted
// waits.  GEMM 1 / GEMM 2 chunks come from the forward's packed tail, W3^T / W1^T from the backward's packed stream (its second-order
// part); the ring runs across the hand-over.  nll and lse are, bit for bit, head_fwd_kernel's (same statements in the same order).
#include "wae_common.hpp"

struct HeadTrainArgs {
  const char* h0;
  const char* w_fwd;      // GEMM 1 | GEMM 2 chunks (head_fwd's packed tail)
  const char* w_bwd;      // W3^T | W1^T chunks (head_bwd's packed stream from its second-order part on)
  const float* bias;      // [Sp unread | Sp b1 | Op b3]
  const int32_t* target;
  const int32_t* lengths;
  float* nll;
  float* lse;
  char* h1;
  char* dy;
  char* dh1;
  char* dskip;
  double* partial;        // one per workgroup
  unsigned* counter;      // zero between launches
  float* loss;            // [mean, count]
  int B, T, Sp, O;
  float scale, dy_factor;
};

// gemm_chunk<..., KMAJOR = true> for accumulator tiles that start from zero: the first k-block of every tile takes the constant 0 as its
// C operand, so no register holds zeros while the previous GEMM's tiles are still being converted (wae_common.hpp: GemmChunkStep)
template <int I, int N, int NM, int PD, int NB, typename frag>
struct GemmChunkStepZ {
  static __device__ __forceinline__ void run(unsigned addr, frag (&a)[PD], const frag (&B)[NB], f32x16 (&acc)[NM]) {
    constexpr int remaining = N - 1 - I;
    constexpr int cnt = remaining < PD - 1 ? remaining : PD - 1;
    lds_wait<cnt>(a[I % PD]);
    if constexpr (I % NB == 0) {
      const f32x16 z = {};
      acc[I / NB] = z;
    }
    mma32(acc[I / NB], a[I % PD], B[I % NB]);
    if constexpr (I + PD < N) lds_read_async<(I + PD) * 1024>(a[I % PD], addr);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (I + 1 < N) GemmChunkStepZ<I + 1, N, NM, PD, NB, frag>::run(addr, a, B, acc);
  }
};
template <int N, int NM, int NB, int PDMAX = 8, typename frag>
__device__ __forceinline__ void gemm_chunk_zero(const char* buf, const frag (&B)[NB], f32x16 (&acc)[NM]) {
  constexpr int PD = N < PDMAX ? N : PDMAX;
  static_assert((N - 1) * 1024 < 65536, "ds_read offset field is 16 bits");
  const unsigned addr = (unsigned)(uintptr_t)(const __attribute__((address_space(3))) char*)buf;
  frag a[PD];
  __builtin_amdgcn_sched_barrier(0);
  GemmChunkPrologue<0, PD, frag>::run(addr, a);
  GemmChunkStepZ<0, N, NM, PD, NB, frag>::run(addr, a, B, acc);
}

// acc_to_frags (wae_common.hpp) with the conversions written pair by pair: one packed convert per register of the fragment.  Element by
// element hipcc converts all NT*16 values into a register each before it packs them, which at NT = 8 does not fit beside the tiles.
template <typename E>
__device__ __forceinline__ void acc_to_frags_pk(const f32x16& u, typename ET<E>::frag (&f)[2]) {
  typedef __attribute__((ext_vector_type(2))) E e2;
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2 v = {u[8 * s + 2 * j], u[8 * s + 2 * j + 1]};
      w[j] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, e2));
    }
    f[s] = __builtin_bit_cast(typename ET<E>::frag, w);
  }
}

#define HEAD_TRAIN_RED_SLOTS 4096     // partials the last workgroup sums per pass (the eight staging tiles: 32 KiB of doubles)

template <typename E, int NT>
__global__ void __launch_bounds__(512, 1) head_train_kernel(HeadTrainArgs p) {
  using T_ = ET<E>;
  using frag = typename T_::frag;
  static_assert(sizeof(E) == 2, "16-bit storage only");
  constexpr int NW = 8, NSL = 3;
  constexpr int CHB = NT * 4 * 1024;
  constexpr int ES = sizeof(E);
  constexpr int KBU = T_::KBU;
  constexpr int NKB = NT * KBU;
  constexpr int MT2 = 4 / KBU;
  constexpr int NQ = NT / MT2;                 // chunks per GEMM
  constexpr int NQT = 4 * NQ;
  constexpr int TW = NW * 32;
  constexpr int PPW = CHB / NW / 1024;         // LDS-DMA pieces per wave and chunk
  constexpr int STGW = 4096, SPITCH = STGW / 32;
  constexpr int NMW = (NT + 1) / 2;            // mask words: 16 bits per tile
  // A fragments in flight in GEMM 1 / GEMM 2, where all NT tiles and the operand fragments are live beside the log-sum-exp's state
  // (NT = 8: 6, which keeps the kernel inside the 256 registers of two waves per SIMD without scratch; 8 spills seven registers)
  constexpr int PD12 = NT == 8 ? 6 : 8;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 31, h = lane >> 5;
  const int tiles_per_b = (p.T + TW - 1) / TW;
  const int tile_id = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const int b = tile_id / tiles_per_b;
  const int t0w = (tile_id % tiles_per_b) * TW + wave * 32;
  const int t = t0w + n;
  const bool tvalid = t < p.T;
  const int rows_valid = min(max(p.T - t0w, 0), 32);
  const int64_t rowB = (int64_t)p.Sp * ES;
  const int64_t base_t = (int64_t)b * p.T + t0w;

  char* stg = smem + NSL * CHB + wave * STGW;
  float* bias_lds = (float*)(smem + NSL * CHB + NW * STGW);
  double* red = (double*)(smem + NSL * CHB + NW * STGW + 3 * p.Sp * 4);
  int* last_flag = (int*)(red + NW);
  // the relu masks wait in LDS between where they are formed and where they are applied (word w of mask k: [k * NMW + w][thread])
  auto mpark_of = [&]() {        // (formed anew where it is used: one add, not a register held across the GEMMs)
    unsigned tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    return (unsigned*)(last_flag + 4) + tid;
  };

  for (int i = threadIdx.x * 4; i < 3 * p.Sp; i += NW * 256) *(f32x4*)(bias_lds + i) = *(const f32x4*)(p.bias + i);
  // chunk qt -> slot qt % NSL, requested two chunks ahead; the wait in front of chunk qt leaves chunk qt + 1's pieces in flight (stores
  // issued in between only make it stricter), the one in front of the last chunk leaves nothing
  auto dma_tail = [&](int qt) {
    if (qt < NQT) {
      const char* src = qt < 2 * NQ ? p.w_fwd + (int64_t)qt * CHB : p.w_bwd + (int64_t)(qt - 2 * NQ) * CHB;
      dma_chunk<NW>(src, smem + (qt % NSL) * CHB, CHB, wave, lane);
    }
  };
  auto ring_step = [&](int qt) {
    if (qt == 0 || qt + 1 >= NQT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // (chunk 0: also the h0 rows, target, lengths)
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW) : "memory");
    __builtin_amdgcn_s_barrier();   // chunk qt visible; every wave is past its reads of chunk qt - 1, whose slot is refilled now
    dma_tail(qt + NSL - 1);
  };
  auto ring_buf = [&](int qt) { return smem + (qt % NSL) * CHB + lane * 16; };

  dma_tail(0);
  dma_tail(1);

  // the column's target and weight (head_bwd.hip's statements) -- requested here, retired by chunk 0's wait
  int tgt = -1, tgt_w = -1;
  float wt = 0.f;
  if (tvalid && t + 1 < p.T) {
    tgt = p.target[(int64_t)b * p.T + t + 1];
    const int len = p.lengths ? min(p.lengths[b], p.T) : p.T;
    if (t < len - 1) { wt = p.dy_factor; tgt_w = tgt; }
  }

  // ---- h0 rows of this wave's 32 columns -> accumulator layout -> mask bits and operand fragments ------------------------------
  f32x16 acc[NT];
  frag uf[NKB];
  unsigned m0[NMW], m1[NMW], mk[NMW];
#pragma unroll
  for (int m = 0; m < NT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  if (rows_valid > 0) stage_load_tiles<E, NT, SPITCH>(stg, acc, p.h0 + base_t * rowB, rowB, rows_valid, lane);
#pragma unroll
  for (int w = 0; w < NMW; ++w) m0[w] = m1[w] = 0u;
#pragma unroll
  for (int m = 0; m < NT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) m0[m >> 1] |= acc[m][r] > 0.f ? 1u << ((m & 1) * 16 + r) : 0u;
    frag tmp[KBU];
    acc_to_frags_pk<E>(acc[m], tmp);
#pragma unroll
    for (int s = 0; s < KBU; ++s) uf[m * KBU + s] = tmp[s];
  }
  // (the bits are formed HERE: without the pin hipcc sinks the compares to GEMM c's epilogue and keeps the NT*16 h0 values alive)
#pragma unroll
  for (int w = 0; w < NMW; ++w) {
    asm volatile("" : "+v"(m0[w]));
    mpark_of()[w * NW * 64] = m0[w];
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // the bias table is in LDS before the first barrier

  // ---- GEMM 1: h1 = relu(b1 + W1 . h0) ----------------------------------------------------------------------------------------------
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ring_step(q);
    f32x16(&y)[MT2] = *reinterpret_cast<f32x16(*)[MT2]>(&acc[q * MT2]);
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt) init_rows(y[mt], bias_lds + p.Sp + 32 * (q * MT2 + mt), h);
    gemm_chunk<MT2 * NKB, MT2, NKB, true, PD12>(ring_buf(q), uf, y);
  }
#pragma unroll
  for (int m = 0; m < NT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = fmaxf(acc[m][r], 0.f);
    frag tmp[KBU];
    acc_to_frags_pk<E>(acc[m], tmp);
#pragma unroll
    for (int s = 0; s < KBU; ++s) {
      uf[m * KBU + s] = tmp[s];
      // the mask of the STORED h1 (what head_bwd tests): a small positive value may round to zero in the storage type
#pragma unroll
      for (int j = 0; j < 8; ++j) m1[m >> 1] |= (float)tmp[s][j] > 0.f ? 1u << ((m & 1) * 16 + 8 * s + j) : 0u;
    }
  }
#pragma unroll
  for (int w = 0; w < NMW; ++w) {
    asm volatile("" : "+v"(m1[w]));
    mpark_of()[(NMW + w) * NW * 64] = m1[w];
  }
  if (rows_valid > 0) stage_store_tiles<E, NT, SPITCH>(stg, acc, p.h1 + base_t * rowB, rowB, rows_valid, lane);

  // ---- GEMM 2 into all NT tiles + online log-sum-exp (head_fwd.hip's statements, tile by tile) ------------------------------------
  float run_m = -INFINITY, run_s = 0.f, picked = 0.f;
  const float* b3 = bias_lds + 2 * p.Sp;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ring_step(NQ + q);
    f32x16(&y)[MT2] = *reinterpret_cast<f32x16(*)[MT2]>(&acc[q * MT2]);
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt) init_rows(y[mt], b3 + 32 * (q * MT2 + mt), h);
    gemm_chunk<MT2 * NKB, MT2, NKB, true, PD12>(ring_buf(NQ + q), uf, y);
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt) {
      const int gm = q * MT2 + mt;
      if (tvalid) {
        float tile_m = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cls = 32 * gm + (r & 3) + 8 * (r >> 2) + 4 * h;
          if (cls < p.O) {
            tile_m = fmaxf(tile_m, y[mt][r]);
            if (cls == tgt) picked = y[mt][r];
          }
        }
        if (tile_m > -INFINITY) {
          const float nm = fmaxf(run_m, tile_m);
          float s = run_s * __expf(run_m - nm);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int cls = 32 * gm + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (cls < p.O) s += __expf(y[mt][r] - nm);
          }
          run_m = nm;
          run_s = s;
        }
      }
    }
  }
  float lse;
  {
    // merge the two lane halves (rows 4h..4h+3 of every 8) of the same time column
    const float om = __shfl_xor(run_m, 32), os = __shfl_xor(run_s, 32), op = __shfl_xor(picked, 32);
    const float nm = fmaxf(run_m, om);
    float s = 0.f;
    if (run_m > -INFINITY) s += run_s * __expf(run_m - nm);
    if (om > -INFINITY) s += os * __expf(om - nm);
    float v = 0.f;
    if (tvalid && h == 0) {
      if (tgt >= 0) v = (nm + __logf(s)) - (picked + op);
      p.nll[(int64_t)b * p.T + t] = v;
      if (p.lse) p.lse[(int64_t)b * p.T + t] = nm + __logf(s);
    }
    lse = __shfl(nm + __logf(s), n);       // both halves take the stored value (lane n wrote it)
    // this wave's share of the masked sum, in double, by a fixed tree
    double d = (tvalid && h == 0 && tgt_w >= 0) ? (double)v : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    if (lane == 0) red[wave] = d;
  }

  // ---- dy in place (head_bwd.hip's statements) -----------------------------------------------------------------------------------------
#pragma unroll
  for (int m = 0; m < NT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int cls = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * h;
      float g = 0.f;
      if (cls < p.O) g = (expf(acc[m][r] - lse) - (cls == tgt_w ? 1.f : 0.f)) * wt;
      acc[m][r] = g;
    }
  if (rows_valid > 0) stage_store_tiles<E, NT, SPITCH>(stg, acc, p.dy + base_t * rowB, rowB, rows_valid, lane);
#pragma unroll
  for (int m = 0; m < NT; ++m) {
    frag tmp[KBU];
    acc_to_frags_pk<E>(acc[m], tmp);
#pragma unroll
    for (int s = 0; s < KBU; ++s) uf[m * KBU + s] = tmp[s];
  }

  // ---- GEMM b: dh1 = W3^T dy, masked by the h1 bits ------------------------------------------------------------------------------------
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ring_step(2 * NQ + q);
    f32x16(&y)[MT2] = *reinterpret_cast<f32x16(*)[MT2]>(&acc[q * MT2]);
    gemm_chunk_zero<MT2 * NKB, MT2, NKB>(ring_buf(2 * NQ + q), uf, y);
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int w = 0; w < NMW; ++w) mk[w] = mpark_of()[(NMW + w) * NW * 64];
#pragma unroll
  for (int m = 0; m < NT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = (mk[m >> 1] >> ((m & 1) * 16 + r)) & 1u ? acc[m][r] : 0.f;
  __builtin_amdgcn_sched_barrier(0);
  if (rows_valid > 0) stage_store_tiles<E, NT, SPITCH>(stg, acc, p.dh1 + base_t * rowB, rowB, rows_valid, lane);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int m = 0; m < NT; ++m) {
    frag tmp[KBU];
    acc_to_frags_pk<E>(acc[m], tmp);
#pragma unroll
    for (int s = 0; s < KBU; ++s) uf[m * KBU + s] = tmp[s];
  }

  // ---- GEMM c: dskip = (W1^T dh1), masked by the h0 bits, times sqrt(1/L) -----------------------------------------------------------
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    ring_step(3 * NQ + q);
    f32x16(&y)[MT2] = *reinterpret_cast<f32x16(*)[MT2]>(&acc[q * MT2]);
    gemm_chunk_zero<MT2 * NKB, MT2, NKB>(ring_buf(3 * NQ + q), uf, y);
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int w = 0; w < NMW; ++w) mk[w] = mpark_of()[w * NW * 64];
#pragma unroll
  for (int m = 0; m < NT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = (mk[m >> 1] >> ((m & 1) * 16 + r)) & 1u ? acc[m][r] * p.scale : 0.f;
  if (rows_valid > 0) stage_store_tiles<E, NT, SPITCH>(stg, acc, p.dskip + base_t * rowB, rowB, rows_valid, lane);

  // ---- the masked mean: this workgroup's partial; the workgroup that counts last sums all of them in index order ------------------
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += red[w];
    __hip_atomic_store(p.partial + blockIdx.x, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const unsigned seen = __hip_atomic_fetch_add(p.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    *last_flag = seen + 1 == gridDim.x;
  }
  __syncthreads();
  if (*last_flag) {
    __threadfence();
    double* buf = (double*)(smem + NSL * CHB);      // every wave is done with its staging tile
    double tot = 0.0;
    for (int base = 0; base < (int)gridDim.x; base += HEAD_TRAIN_RED_SLOTS) {
      const int cnt = min((int)gridDim.x - base, HEAD_TRAIN_RED_SLOTS);
      for (int i = threadIdx.x; i < cnt; i += NW * 64)
        buf[i] = __hip_atomic_load(p.partial + base + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      if (threadIdx.x == 0)
        for (int i = 0; i < cnt; ++i) tot += buf[i];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      double cnt = 0.0;
      for (int bb = 0; bb < p.B; ++bb) {
        const int len = p.lengths ? min(p.lengths[bb], p.T) : p.T;
        cnt += (double)max(len - 1, 0);
      }
      p.loss[0] = (float)(tot / cnt);
      p.loss[1] = (float)cnt;
      __hip_atomic_store(p.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch
    }
  }
}

template <typename E, int NT>
static int launch_head_train(const HeadTrainArgs& a, hipStream_t st) {
  constexpr int CHB = NT * 4 * 1024;
  // ring | staging tiles | biases | the eight waves' partial sums, the last-workgroup flag | the parked masks
  const size_t lds = (size_t)3 * CHB + 8 * 4096 + (size_t)3 * a.Sp * 4 + 8 * sizeof(double) + 16 + (size_t)2 * ((NT + 1) / 2) * 512 * 4;
  static WaeLdsCache lds_cache;
  auto kern = head_train_kernel<E, NT>;
  if (int rc = wae_ensure_lds((const void*)kern, lds_cache, lds, "head_train"); rc != WAE_OK) return rc;
  const int tiles = (a.T + 255) / 256;
  hipLaunchKernelGGL(kern, dim3(a.B * tiles), dim3(512), lds, st, a);
  return wae_check_launch("head_train");
}

extern "C" int wae_head_train_supported(int32_t dtype, int32_t Sp, int32_t Op) {
  return wae_is16(dtype) && Sp == Op && (Sp == 128 || Sp == 256);
}

extern "C" int64_t wae_head_train_ws_bytes(const wae_head_desc* d) {
  if (!d || d->B <= 0 || d->T <= 0) return WAE_EINVAL;
  return 16 + (int64_t)d->B * ((d->T + 255) / 256) * (int64_t)sizeof(double);
}

extern "C" int wae_head_train_from_h0(const wae_head_desc* d, const void* h0, const void* w_tail, const void* w_bwd_packed,
                                      const float* bias, const int32_t* target, const int32_t* lengths, float dy_factor, float* nll,
                                      float* lse, void* h1_save, void* dy_out, void* dh1_out, void* dskip_out, void* red_ws, float* loss,
                                      void* stream) {
  WAE_REQUIRE(d != nullptr, "head_train: null desc");
  WAE_REQUIRE(d->B > 0 && d->T > 0 && d->O > 0, "head_train: B,T,O must be positive");
  WAE_REQUIRE(wae_head_train_supported(d->dtype, d->Sp, d->Op), "head_train: 16-bit storage with Sp == Op in {128, 256} (got dtype %d, Sp %d, Op %d)",
              d->dtype, d->Sp, d->Op);
  WAE_REQUIRE(d->O <= d->Op, "head_train: O (%d) exceeds Op (%d)", d->O, d->Op);
  WAE_REQUIRE(h0 && w_tail && w_bwd_packed && bias && target && nll && h1_save && dy_out && dh1_out && dskip_out && red_ws && loss,
              "head_train: null pointer argument");
  HeadTrainArgs a;
  const int nt = d->Sp / 32;
  a.h0 = (const char*)h0; a.w_fwd = (const char*)w_tail;
  // head_bwd's stream: [W3 first-order: Sp / 64 chunks | W3^T | W1^T], every chunk Op / 32 * 4 KiB
  a.w_bwd = (const char*)w_bwd_packed + (int64_t)(d->Sp / 64) * nt * 4096;
  a.bias = bias; a.target = target; a.lengths = lengths; a.nll = nll; a.lse = lse; a.h1 = (char*)h1_save; a.dy = (char*)dy_out;
  a.dh1 = (char*)dh1_out; a.dskip = (char*)dskip_out;
  a.counter = (unsigned*)red_ws; a.partial = (double*)((char*)red_ws + 16); a.loss = loss;
  a.B = d->B; a.T = d->T; a.Sp = d->Sp; a.O = d->O; a.scale = d->scale; a.dy_factor = dy_factor;
  hipStream_t st = as_stream(stream);
  if (d->dtype == WAE_BF16) return nt == 4 ? launch_head_train<__bf16, 4>(a, st) : launch_head_train<__bf16, 8>(a, st);
  return nt == 4 ? launch_head_train<f16, 4>(a, st) : launch_head_train<f16, 8>(a, st);
}
