// The generic fused-layer kernel template (csrc/glu_fwd.hip: the dense instantiations; csrc/glu_fwd_list.hip: the list form).
#pragma once
#include <type_traits>
#include "glu_fwd.hpp"
#ifndef WAE_GLU_PD
#define WAE_GLU_PD 4      // A-fragment reads in flight per wave in GEMM 1 (5, 6, 8: the C2 instantiation is at 256 registers and spills)
#endif

// timing-only ablation bits (tools/ablate_glu.py): compiled in only with -DWAE_GLU_ABLATE (a run-time test of these
// bits inside the gate loop cost 2x on that phase); outputs are wrong when any is set
#define DBG_NO_DMA 0x100
#define DBG_NO_BLOAD 0x200
#define DBG_NO_EPI 0x400
#define DBG_NO_GATE 0x800
#ifdef WAE_GLU_ABLATE
#define ABL(flags, bit) ((flags) & (bit))
#else
#define ABL(flags, bit) false
#endif
#ifdef WAE_GLU_STAMPS
#define STAMP(i)                                                              \
  do {                                                                        \
    if (p.stamps) {                                                           \
      __builtin_amdgcn_sched_barrier(0);                                      \
      st_[i] = __builtin_amdgcn_s_memtime();                                  \
      __builtin_amdgcn_sched_barrier(0);                                      \
    }                                                                         \
  } while (0)
#else
#define STAMP(i) do { } while (0)
#endif

// s_waitcnt vmcnt(min(w, 15)) for a wave-uniform run-time w (the count is an immediate in the ISA)
__device__ __forceinline__ void wait_vmcnt_upto(int w) {
#define WAE_VMC(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (w < 15 ? w : 15) {
    WAE_VMC(0) WAE_VMC(1) WAE_VMC(2) WAE_VMC(3) WAE_VMC(4) WAE_VMC(5) WAE_VMC(6) WAE_VMC(7)
    WAE_VMC(8) WAE_VMC(9) WAE_VMC(10) WAE_VMC(11) WAE_VMC(12) WAE_VMC(13) WAE_VMC(14)
    default: asm volatile("s_waitcnt vmcnt(15)" ::: "memory"); break;
  }
#undef WAE_VMC
}

__device__ __forceinline__ float vmax_nocanon(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// NPH = gate-channel tiles per pass (per half); NW = waves per workgroup; CG = 32-column groups per wave.
// CG = 2 (bf16 / fp16, 4 waves, one per SIMD, up to 512 registers each): a wave owns 64 time columns, every A fragment it
// reads from LDS feeds two MFMAs.  Opt-in and slower than CG = 1 (the LDS port, measured at 256 B/clk, was never
// the limit; one wave per SIMD exposes every wait of that wave).
//
// LIST (include/wae.h: wae_glu_layer_fwd_list): a workgroup is one tile of one ITEM of a list packed along time.  It finds the item's
// record by a workgroup-uniform binary search of its tile index (csrc/ups_list.hip), and from there on the item's T and row_off stand
// wherever the dense form has p.T and b * p.T -- the causal zero fill, the row clamp of the requests, the valid rows of the epilogues,
// the residual read -- and zb comes from the record's row.  Everything else, the per-column arithmetic above all, is the same
// statements: a column of either GEMM does not depend on the tile it sits in, so an item's rows are bitwise the dense kernel's for
// that item alone.  The list form is inference only: the z save is compiled out of it.  Its arguments: the dense ones (B = rows of
// zb; T unused) and the list's table.
struct GluListArgs : GluArgs {
  const wae_glu_seg* segs;  // nsegs records and the closing one
  int nsegs;
  int rows;                 // rows of the packed arrays: no record may reach beyond them
};

template <typename E, int NP, int NPH, bool EXACT, int NW, int CG, bool LIST = false>
__global__ void __launch_bounds__(NW * 64, (NW == 4 && sizeof(E) == 2 && CG == 1) ? 2 : 1)
glu_fwd_kernel(std::conditional_t<LIST, GluListArgs, GluArgs> p) {
  using T_ = ET<E>;
  using frag = typename T_::frag;
  static_assert(NP % NPH == 0, "passes must tile the gate channels");
  constexpr int NPASS = NP / NPH;
  constexpr int NM = 2 * NPH;
  constexpr int CHB = NM * 4 * 1024;  // bytes per weight chunk
  constexpr int ES = sizeof(E);
  constexpr int KBU = T_::KBU;
  constexpr int NKB = NP * KBU;              // 16-B k-blocks of GEMM 2
  constexpr int MT2 = CHB / (NKB * 1024);    // GEMM-2 M-tiles per chunk
  static_assert(MT2 >= 1 && MT2 * NKB * 1024 == CHB, "GEMM-2 chunk must equal GEMM-1 chunk");
  constexpr int PITCH = 128, STG = 32 * PITCH;
  // The widest 16-bit list instantiation (Hp = 256) sits at the register limit and may not spill (csrc/glu_fwd_list.hip).  What it
  // spilled was a per-lane address term of the epilogue stores, hoisted to the top of the kernel and kept across both passes; it forms
  // those terms at the store instead, from a copy of the lane index the compiler cannot see through (251 registers, no spill).
  constexpr bool NARROW = LIST && NP == 8 && sizeof(E) == 2;

  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef WAE_GLU_STAMPS
  unsigned long long st_[16] = {};
  if (p.stamps) st_[14] = __builtin_amdgcn_s_memrealtime();
#endif
  STAMP(0);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = lane & 31, h = lane >> 5;
  constexpr int TW = NW * 32 * CG;
  const int tiles_per_b = LIST ? 1 : (p.T + TW - 1) / TW;
  const int tile_id = xcd_contiguous_tile(blockIdx.x, gridDim.x);
  const int b = tile_id / tiles_per_b;
  // The clip of this tile -- its steps, its first row in the time-major arrays, its row of zb, the tile's first column in it.  Dense:
  // clip b of the batch, in the expressions this kernel has always had (GLU_T, GLU_ROW0 and GLU_ZROW fold to them at compile time, so
  // the dense instantiations do not move).  LIST: the item's record, workgroup-uniform (scalar registers).
  int it_T = 0, it_row = 0, it_zrow = 0, it_tcol = 0;
#define GLU_T (LIST ? it_T : p.T)
#define GLU_ROW0 (LIST ? (int64_t)it_row : (int64_t)b * p.T)
#define GLU_ZROW (LIST ? it_zrow : b)
  if constexpr (LIST) {
    int lo = 0, hi = p.nsegs - 1;
    while (lo < hi) {                      // the last record with tile0 <= tile_id
      const int mid = (lo + hi + 1) >> 1;
      if (p.segs[mid].tile0 <= tile_id) lo = mid;
      else hi = mid - 1;
    }
    const wae_glu_seg seg = p.segs[lo];
    const int next = __builtin_amdgcn_readfirstlane(p.segs[lo + 1].tile0);   // (the closing record for the last item)
    const int row_off = __builtin_amdgcn_readfirstlane(seg.row_off);
    const int k = __builtin_amdgcn_readfirstlane(tile_id - seg.tile0);
    const int T = __builtin_amdgcn_readfirstlane(seg.T);
    const int zrow = __builtin_amdgcn_readfirstlane(seg.zb_row);
    // The table is not trusted with memory: a record that does not fit is skipped whole, in front of every barrier and every access
    // (uniform over the workgroup).
    if (T < 1 || k < 0 || tile_id >= next || row_off < 0 || (int64_t)row_off + T > p.rows || zrow < 0 || zrow >= p.B) return;
    if ((int64_t)next - seg.tile0 != ((int64_t)T + TW - 1) / TW) return;
    it_T = T;
    it_row = row_off;
    it_zrow = zrow;
    it_tcol = k * TW;                      // < T by the tile count
  }
  const int t0w = (LIST ? it_tcol : (tile_id % tiles_per_b) * TW) + wave * 32 * CG;   // first column of this wave; group c starts at t0w + 32 c
  const int t = t0w + n;                                                               // this lane's column in group 0 (group c: t + 32 c)

  const int cpr = p.Rp / T_::CK;  // chunks per tap
  const int nq_conv = p.ktaps * cpr;
  const int nq1 = nq_conv + p.Ccp / T_::CK;
  const int nq2 = (p.flags & WAE_GLU_NO_OUT) ? 0 : (p.Rp >> 5) / MT2;
  const int nq_total = NPASS * nq1 + nq2;

  const int64_t row_x = (int64_t)p.Rp * ES;
  const int64_t row_c = (int64_t)p.Ccp * ES;
  const char* xb = p.x_in + GLU_ROW0 * row_x;      // residual path: the layer's input itself (modules.py:126,161)
  const char* xcb = p.x_conv + GLU_ROW0 * row_x;   // convolution operand
  const char* cb = p.c_up ? p.c_up + GLU_ROW0 * row_c : nullptr;

  const bool dbg_dma = !ABL(p.flags, DBG_NO_DMA);
  // chunk -> (column block, tap) once per chunk in b_src / fix_B: q / ktaps as a multiply (exact for q < 65536 / ktaps)
  const unsigned kinv = (65536u + (unsigned)p.ktaps - 1u) / (unsigned)p.ktaps;
  // The activation operand is requested TWO chunks ahead into a rotating set of three fragment groups (an L2/HBM
  // round trip under load is longer than one chunk of MFMAs).  Loads are always issued (rows clamped into the clip)
  // so that the number of outstanding VMEM ops is known; columns outside [0, T) are zeroed at use (causal pad).
  frag S0[CG][4] = {}, S1[CG][4] = {}, S2[CG][4] = {};   // defined: the asm loads tie their destination to its previous register
  // per-lane address of this lane's first fragment of activation chunk q, column group c (its row clamped into the clip)
  auto b_src = [&](int q, int c) -> const char* {
    const char* base;
    int64_t rp;
    int ts = t + 32 * c;
    if (q < nq_conv) {
      // column block by column block, the taps of one block back to back: a tile reads x[t - d] right after x[t] while the
      // tile d rows earlier reads the same rows as its last tap -- they meet in L2 (packing.py: glu_w1_map, same order)
      const int cblk = (int)(((unsigned)q * kinv) >> 16), tap = q - cblk * p.ktaps;   // q / ktaps without the division sequence
      ts -= (p.ktaps - 1 - tap) * p.dilation;
      base = xcb + cblk * 128 + h * 16;
      rp = row_x;
    } else {
      base = cb + (q - nq_conv) * 128 + h * 16;
      rp = row_c;
    }
    return base + (int64_t)min(max(ts, 0), GLU_T - 1) * rp;
  };
  // bf16 / fp16 only: the fp32 (parity) instantiations spill a few registers, and a fragment group spilled between its request
  // and the counted wait would be saved before it has landed -- they keep plain loads and the compiler's own waits.
#ifdef WAE_GLU_PLAIN_LOADS   // tools/check_asm_loads.py: the same kernel with compiler-managed loads, for a bitwise comparison
  constexpr bool ASM_B = false;
#else
  constexpr bool ASM_B = sizeof(E) == 2;
#endif
  // Requests go out as inline-asm loads (gload_async) and are retired by the counted waits of chunk_top alone.  As plain
  // loads they made hipcc put s_waitcnt vmcnt(0) in front of the first use of every loop-carried fragment group (the zero
  // fill in fix_B, right after the barrier of each chunk) -- which drained the DMA pieces and operand requests of the NEXT
  // chunks: the ring and the two-chunks-ahead requests bought nothing, every variant of this kernel measured 60 +- 2 us.
  auto load_B = [&](int q, frag (&Bf)[CG][4]) {
    if (ABL(p.flags, DBG_NO_BLOAD)) return;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const char* src = b_src(q, c);
      if constexpr (ASM_B) {
        gload_async<0>(Bf[c][0], src); gload_async<32>(Bf[c][1], src); gload_async<64>(Bf[c][2], src); gload_async<96>(Bf[c][3], src);
      } else {
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) Bf[c][blk] = *(const frag*)(src + blk * 32);
      }
    }
  };
  auto fix_B = [&](int q, frag (&Bf)[CG][4]) {
    const int shift = q < nq_conv ? (p.ktaps - 1 - (q - (int)(((unsigned)q * kinv) >> 16) * p.ktaps)) * p.dilation : 0;
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const int tc = t + 32 * c;
      const bool ok = tc < GLU_T && tc - shift >= 0 && !ABL(p.flags, DBG_NO_BLOAD);
      if (__any(!ok)) {
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
          if (!ok) {
            frag zf = {};
            Bf[c][blk] = zf;
          }
      }
    }
  };

  // out bias and this clip's zb -> LDS once (read back with ds_read: keeps accumulator inits off vmcnt, where they
  // would drain the LDS-DMA queue)
  constexpr int PPW = CHB / NW / 1024;  // LDS-DMA instructions per wave and chunk
  constexpr int NBL = 4 * CG;           // operand loads per wave and chunk
  // WAE_GLU_PAIR: the workgroup barrier of GEMM 1 on even chunks only.  Safe with four ring slots and the weights TWO chunks ahead:
  //  * slot reuse: DMA(c + 2), issued during chunk c, overwrites the slot of chunk c - 2, which every wave left before the last
  //    barrier (top of c for even c, top of c - 1 for odd c); a wave that runs one chunk ahead reads slot c % 4 and writes
  //    slot (c + 2) % 4 while the others read slot (c - 1) % 4;
  //  * visibility: at an even top every wave waits until only its operand requests of the previous chunk are outstanding, i.e.
  //    its pieces of DMA(c) AND of DMA(c + 1) (issued ahead of those requests in the previous chunk's stream) have landed
  //    before anybody passes the barrier -- nobody meets again before reading chunk c + 1.
  const bool pair = CG == 1 && (p.flags & WAE_GLU_PAIR) && p.nslot == 4;
  const int D = pair ? 2 : p.nslot - 1;   // weight prefetch distance in chunks
  char* ring_end = smem + p.nslot * CHB;
  char* stg = ring_end + wave * STG;
  float* bias_lds = (float*)(ring_end + NW * STG);
  float* zb_lds = bias_lds + p.Rp;
  {
    const float* zbb = p.zb + (int64_t)GLU_ZROW * p.zb_stride;
    if (nq2 > 0)
      for (int i = threadIdx.x * 4; i < p.Rp; i += NW * 256) *(f32x4*)(bias_lds + i) = *(const f32x4*)(p.bias_out + i);
    for (int i = threadIdx.x * 4; i < 2 * p.Hp; i += NW * 256) *(f32x4*)(zb_lds + i) = *(const f32x4*)(zbb + i);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // table loads retired: from here on VMEM ops are counted by hand
  if (dbg_dma) dma_chunk<NW>(p.w, smem, CHB, wave, lane);
  load_B(0, S0);
  load_B(1, S1);
  STAMP(1);

  const bool no_epi = ABL(p.flags, DBG_NO_EPI);
  frag uf[CG][NKB];
  // ring bookkeeping: slot_c = slot of the current chunk, slot_n = slot the next DMA goes to (chunk qi + D)
  int slot_c = 0, slot_n = 1 % p.nslot;
  // Top of chunk qi: retire B(qi) and DMA(qi), meet the other waves.  The requests for later chunks -- the weights
  // D chunks ahead (PPW LDS-DMA pieces per wave) and the activations two chunks ahead (NBL loads) -- are then issued
  // BETWEEN the MFMAs of chunk qi (every SP-th step), pieces first: a burst of VMEM instructions per wave at the
  // chunk top queued at the CU's texture-address unit for ~1000 cycles per chunk with the matrix pipe idle.
  // Loads retire in order, so B(qi) -- the last thing issued in chunk qi-2 -- and everything older (DMA(qi) included,
  // D >= 2) have landed once at most w_next = (ops issued during chunk qi-1) VMEM ops are outstanding.  Stores issued
  // in between only make the wait stricter.  D == 1: DMA(qi) is itself part of chunk qi-1, only that chunk's B loads
  // may stay in flight.
  constexpr int NSTEP = 4 * NM * CG, NOPS = PPW + NBL, SP = NSTEP / NOPS >= 1 ? NSTEP / NOPS : 1;
  static_assert(NOPS * SP <= NSTEP + SP - 1 && NOPS <= NSTEP, "not enough MFMA steps to carry the chunk's VMEM issue");
  const int per_wave = CHB / NW;
  const char* w_lane = p.w + wave * per_wave + lane * 16;
  int w_next = ABL(p.flags, DBG_NO_BLOAD) ? 0 : NBL;  // the prologue's B(1)
  int nb_last = w_next;   // operand requests issued by the previous chunk's stream (they follow its DMA pieces)
  const char* dsrc = nullptr;  // this chunk's DMA request (wave-uniform validity), per-lane source
  char* ddst = nullptr;
  const char* bsrc[CG];        // this chunk's activation requests (null: none)
#pragma unroll
  for (int c = 0; c < CG; ++c) bsrc[c] = nullptr;
#ifdef WAE_GLU_STAMPS
  unsigned long long acc_wait = 0, acc_bar = 0, acc_issue = 0, acc_gemm = 0;
#define TICK() (__builtin_amdgcn_sched_barrier(0), __builtin_amdgcn_s_memtime())
#endif
  auto chunk_top = [&](int qi, int q_load) {
#ifdef WAE_GLU_STAMPS
    const unsigned long long c00 = TICK();
#endif
    // Bookkeeping of this chunk's requests first, the wait and the barrier after it (nothing here touches LDS or memory but the
    // chunk-0 burst, which goes to ring slots nobody has read yet).  Per-wave stamps (tools/stamps_glu.py, C2, eight waves): the
    // older wave of a SIMD gets the matrix pipe first, finishes its 24 MFMAs after ~1390 clocks and waits ~870 at the barrier;
    // the younger one needs ~2030, then ~300 for this bookkeeping and ~200 for the wait: 2630 clocks per chunk of 1536 MFMA
    // clocks.  Forming the NEXT chunk's requests inside the MFMA stream instead (built and measured, round 2) moved those 300
    // clocks into the stream one for one: the waves' instruction streams, not the matrix pipe, set the pace of a chunk.
    const int w_cur = w_next;
    int issued = 0;
    dsrc = nullptr;
    if (qi == 0) {
      for (int j = 1; j <= D; ++j)
        if (j < nq_total && dbg_dma) {
          dma_chunk<NW>(p.w + (int64_t)j * CHB, smem + slot_n * CHB, CHB, wave, lane);
          slot_n = slot_n + 1 == p.nslot ? 0 : slot_n + 1;
          issued += PPW;
        }
    } else if (qi + D < nq_total && dbg_dma) {
      dsrc = w_lane + (int64_t)(qi + D) * CHB;
      ddst = smem + slot_n * CHB + wave * per_wave;
      slot_n = slot_n + 1 == p.nslot ? 0 : slot_n + 1;
      issued += PPW;
    }
    const bool lb = q_load >= 0 && !ABL(p.flags, DBG_NO_BLOAD);
#pragma unroll
    for (int c = 0; c < CG; ++c) bsrc[c] = lb ? b_src(q_load, c) : nullptr;   // CG == 2: always a chunk of this pass
    const int nb = lb ? NBL : 0;
    // at chunk 1 DMA(1) -- the oldest chunk of chunk 0's burst -- must have landed as well
    w_next = D == 1 ? nb : (qi == 0 && issued > 0 ? issued - PPW + nb : issued + nb);
#ifdef WAE_GLU_STAMPS
    const unsigned long long c0 = TICK();
    acc_issue += c0 - c00;
#endif
    const bool meet = !pair || (qi & 1) == 0;
    int allow = qi == 0 ? w_cur + issued : w_cur;
    if (pair && meet && qi > 0) allow = min(allow, nb_last);   // DMA(qi + 1) too (see `pair` above)
    nb_last = nb;
    wait_vmcnt_upto(allow);
#ifdef WAE_GLU_STAMPS
    const unsigned long long c1 = TICK();
#endif
    // a bare s_barrier: __syncthreads() is fence + barrier, and hipcc lowers the fence to s_waitcnt vmcnt(0), which
    // would drain the very prefetch queue the counted wait above leaves in flight.  Every wave has retired its LDS
    // reads of the previous chunk (gemm_chunk exits with lgkmcnt(0)), and its own DMA pieces by the counted wait.
    if (meet) __builtin_amdgcn_s_barrier();
#ifdef WAE_GLU_STAMPS
    const unsigned long long c2 = TICK();
    acc_wait += c1 - c0;
    acc_bar += c2 - c1;
#endif
  };

#pragma unroll
  for (int ps = 0; ps < NPASS; ++ps) {
    // ---- accumulators start from zb = conv bias + hoisted global conditioning ---------------------------
    f32x16 acc[CG][NM];
    if (ps == 0) __syncthreads();  // zb/bias tables visible
#pragma unroll
    for (int m = 0; m < NM; ++m) {
      init_rows(acc[0][m], zb_lds + (m < NPH ? 32 * (ps * NPH + m) : p.Hp + 32 * (ps * NPH + m - NPH)), h);
      if constexpr (CG == 2) acc[1][m] = acc[0][m];
    }

    // ---- GEMM 1, pass ps -----------------------------------------------------------------------------------
    // Chunks run in statically unrolled triples so that the three fragment groups rotate without register moves
    // (a move of a group whose load is still in flight would stall on it): chunk q computes from group q % 3 while
    // chunk q + 2 is requested into group (q + 2) % 3.  Every pass restarts the rotation at group 0.
    {
      auto step = [&](int q, frag (&Bcur)[CG][4], frag (&Bload)[CG][4]) {
        // CG == 2 requests UNCONDITIONALLY (the last two chunks of a pass re-request their own rows, L2 hits, into the group
        // that is idle anyway): a request under its own branch gave its destination two reaching definitions, and with the
        // register pressure of 64 columns per wave hipcc then loads into a scratch register and copies it home after the join
        // -- before the data has landed (tools/check_asm_regs.py).  The pass end drains them (below).
        chunk_top(ps * nq1 + q, q + 2 < nq1 ? q + 2 : (CG == 2 ? q : -1));
        // the fragments of this chunk have landed (counted wait in chunk_top): every use comes after this point
        if constexpr (ASM_B) {
#pragma unroll
          for (int c = 0; c < CG; ++c) asm volatile("" : "+v"(Bcur[c][0]), "+v"(Bcur[c][1]), "+v"(Bcur[c][2]), "+v"(Bcur[c][3]));
        }
        fix_B(q, Bcur);
        const char* buf = smem + slot_c * CHB + lane * 16;
        auto filler = [&](auto ic) {
          constexpr int I = decltype(ic)::value;
          if constexpr (I % SP == 0 && I / SP < NOPS) {
            constexpr int k = I / SP;
            if constexpr (k < PPW) {
              if (dsrc) dma_piece(dsrc + k * 1024, ddst + k * 1024);
            } else {
              constexpr int c = (k - PPW) / 4, blk = (k - PPW) % 4;
              if (CG == 2 || bsrc[c]) {
                if constexpr (ASM_B) gload_async<blk * 32>(Bload[c][blk], bsrc[c]);
                else Bload[c][blk] = *(const frag*)(bsrc[c] + blk * 32);
              }
            }
          }
        };
#ifdef WAE_GLU_STAMPS
        const unsigned long long g0 = TICK();
#endif
        gemm_chunk_fill_cg<4 * NM, NM, 4, CG, false, WAE_GLU_PD>(buf, Bcur, acc, filler);
#ifdef WAE_GLU_STAMPS
        acc_gemm += TICK() - g0;
#endif
        slot_c = slot_c + 1 == p.nslot ? 0 : slot_c + 1;
      };
      int q = 0;
      for (; q + 3 <= nq1; q += 3) {
        step(q, S0, S2);
        step(q + 1, S1, S0);
        step(q + 2, S2, S1);
      }
      if (q < nq1) step(q, S0, S2);
      if (q + 1 < nq1) step(q + 1, S1, S0);
      if constexpr (CG == 2 && ASM_B) {
        // retire the re-requests of the pass's last two chunks before their registers can be given to anything else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int c = 0; c < CG; ++c) {
          asm volatile("" : "+v"(S0[c][0]), "+v"(S0[c][1]), "+v"(S0[c][2]), "+v"(S0[c][3]));
          asm volatile("" : "+v"(S1[c][0]), "+v"(S1[c][1]), "+v"(S1[c][2]), "+v"(S1[c][3]));
          asm volatile("" : "+v"(S2[c][0]), "+v"(S2[c][1]), "+v"(S2[c][2]), "+v"(S2[c][3]));
        }
      }
      if (ps + 1 < NPASS) {  // the next pass's first two chunks travel under the gate
        load_B(0, S0);
        load_B(1, S1);
        w_next = ABL(p.flags, DBG_NO_BLOAD) ? 0 : NBL;
        nb_last = w_next;
      }
    }
    if (ps == 0) STAMP(2);

#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const int rows_valid = min(max(GLU_T - (t0w + 32 * c), 0), 32);
      const int64_t row0 = GLU_ROW0 + t0w + 32 * c;
      // ---- optional z save (training): rows of 2Hp elements, a-half then b-half --------------------------
      if constexpr (!LIST) {
        if ((p.flags & WAE_GLU_SAVE_Z) && rows_valid > 0) {
          char* zr = p.z_save + (row0 * (2 * p.Hp) + ps * NPH * 32) * ES;
          stage_store_tiles<E, NPH, PITCH>(stg, &acc[c][0], zr, (int64_t)2 * p.Hp * ES, rows_valid, lane);
          stage_store_tiles<E, NPH, PITCH>(stg, &acc[c][NPH], zr + (int64_t)p.Hp * ES, (int64_t)2 * p.Hp * ES, rows_valid, lane);
        }
      }

      // ---- gate: u = tanh(a) * sigmoid(b); stored once for the head's skip GEMM, and converted in place to the
      //      operand fragments of GEMM 2 -------------------------------------------------------------------
#pragma unroll
      for (int pr = 0; pr < NPH; ++pr) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = acc[c][pr][r], g = acc[c][NPH + pr][r];
          float u;
          if (ABL(p.flags, DBG_NO_GATE)) {
            u = a * g;
          } else if constexpr (EXACT) {
            u = tanhf(a) * (1.0f / (1.0f + expf(-g)));
          } else {
            // tanh(a)*sigmoid(g) = (1-ea) / ((1+ea)(1+eg)), ea = e^-2a, eg = e^-g.  a is clamped from below so that
            // ea stays finite (tanh(-15) == -1 in fp32); eg = inf gives rcp(inf) = 0, the correct limit.
            const f32x2 sc = {-2.885390081777927f, -1.4426950408889634f};
            f32x2 ag = {vmax_nocanon(a, -15.0f), g};
            ag = ag * sc;
            const float ea = __builtin_amdgcn_exp2f(ag.x);
            const float eg = __builtin_amdgcn_exp2f(ag.y);
            const f32x2 one = {1.0f, 1.0f};
            const f32x2 e2 = {ea, eg};
            const f32x2 d = e2 + one;
            u = (1.0f - ea) * fast_rcp(d.x * d.y);
          }
          acc[c][pr][r] = u;
        }
        frag tmp[KBU];
        acc_to_frags(acc[c][pr], tmp);
#pragma unroll
        for (int s = 0; s < KBU; ++s) uf[c][(ps * NPH + pr) * KBU + s] = tmp[s];
        __builtin_amdgcn_sched_barrier(0);  // one tile at a time: keeps the gate's temporaries from piling up
      }
      if (!no_epi && rows_valid > 0) {
        char* ur = p.u_out + (row0 * p.u_stride + ps * NPH * 32) * ES;
        int lane_e = lane;
        if constexpr (NARROW) asm volatile("" : "+v"(lane_e));
        stage_store_tiles<E, NPH, PITCH>(stg, &acc[c][0], ur, p.u_stride * ES, rows_valid, lane_e);
      }
    }
  }
  STAMP(3);

  // ---- GEMM 2 + residual epilogue ------------------------------------------------------------------------
  // Each chunk = MT2 M-tiles (MT2*32 output channels = one staging pass per time row) against all of u.
  for (int q2 = 0; q2 < nq2; ++q2) {
    const int qi = NPASS * nq1 + q2;
    constexpr int NRES = ES == 2 ? 2 * MT2 : 4 * MT2;  // 16-byte fragments per lane (32 bytes of the row per pair)
    const bool dma_now = qi + D < nq_total && dbg_dma;
    // DMA(qi) was requested D chunks ago.  If that was before this phase's first drain (q2 == 0) nothing is pending
    // for it any more.  Otherwise (16-bit): every later chunk has issued its CG * NRES residual requests and its PPW pieces
    // (stores -- none for an all-padding tile -- only make the wait stricter), so DMA(qi) has landed once at most that many
    // operations are outstanding and the younger chunks' pieces stay in flight.  fp32: plain loads, drain.
    if (q2 == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (q2 - D >= 0) {
      if constexpr (ASM_B) {
        int younger = 0;
        for (int j = q2 - D + 1; j < q2; ++j) younger += CG * NRES + (j < nq2 - D && dbg_dma ? PPW : 0);
        wait_vmcnt_upto(younger);
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    __builtin_amdgcn_s_barrier();
    const char* buf = smem + slot_c * CHB + lane * 16;
    slot_c = slot_c + 1 == p.nslot ? 0 : slot_c + 1;
    const int gm0 = q2 * MT2;
    // residual x[t] for this chunk's channels, as operand-shaped 16-byte fragments (L2 hits: tap k-1 of GEMM 1
    // read the same bytes); requested FIRST (loads retire in order: the wait for them below then leaves this chunk's
    // DMA pieces in flight), consumed after the MFMAs
    frag res[CG][NRES];
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      const int tc = t + 32 * c;
      const char* rsrc = xb + (int64_t)(tc < GLU_T ? tc : 0) * row_x + (int64_t)gm0 * 32 * ES + h * 16;
      if constexpr (ASM_B) {
        gload_async_n<0, NRES>(res[c], rsrc);
      } else {
#pragma unroll
        for (int f = 0; f < NRES; ++f) res[c][f] = *(const frag*)(rsrc + f * 32);
      }
    }
    if (dma_now) {
      dma_chunk<NW>(p.w + (int64_t)(qi + D) * CHB, smem + slot_n * CHB, CHB, wave, lane);
      slot_n = slot_n + 1 == p.nslot ? 0 : slot_n + 1;
    }
    f32x16 y[CG][MT2];
#pragma unroll
    for (int mt = 0; mt < MT2; ++mt) {
      init_rows(y[0][mt], bias_lds + 32 * (gm0 + mt), h);
      if constexpr (CG == 2) y[1][mt] = y[0][mt];
    }
    NoFiller nf;
    gemm_chunk_fill_cg<MT2 * NKB, MT2, NKB, CG, true, 8>(buf, uf, y, nf);
    if (no_epi) {
      if (y[0][0][0] == 12345.678f && t < GLU_T) p.x_out[t] =(char)y[CG - 1][MT2 - 1][3];  // keep the MFMAs alive
      continue;
    }
    // x' = (y + x) * sqrt(.5) in the accumulator layout
    const f32x2 rs = {0.70710678118654752440f, 0.70710678118654752440f};
    if constexpr (ASM_B) {   // the residual fragments have landed once only this chunk's pieces (issued after them) are outstanding
      if (dma_now) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(PPW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int c = 0; c < CG; ++c)
#pragma unroll
        for (int f = 0; f < NRES; ++f) asm volatile("" : "+v"(res[c][f]));
    }
#pragma unroll
    for (int c = 0; c < CG; ++c) {
      residual_to_acc_layout(res[c]);
#pragma unroll
      for (int mt = 0; mt < MT2; ++mt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 r4 = residual_piece<E>(res[c], mt, g);
          f32x2 lo = {y[c][mt][4 * g + 0], y[c][mt][4 * g + 1]}, hi = {y[c][mt][4 * g + 2], y[c][mt][4 * g + 3]};
          const f32x2 rlo = {r4.x, r4.y}, rhi = {r4.z, r4.w};
          lo = (lo + rlo) * rs;
          hi = (hi + rhi) * rs;
          y[c][mt][4 * g + 0] = lo.x; y[c][mt][4 * g + 1] = lo.y; y[c][mt][4 * g + 2] = hi.x; y[c][mt][4 * g + 3] = hi.y;
        }
      }
      const int rows_valid = min(max(GLU_T - (t0w + 32 * c), 0), 32);
      if (rows_valid > 0) {
        char* orow = p.x_out + (GLU_ROW0 + t0w + 32 * c) * row_x + (int64_t)gm0 * 32 * ES;
        int lane_e = lane;
        if constexpr (NARROW) asm volatile("" : "+v"(lane_e));
        stage_store_tiles<E, MT2, PITCH>(stg, y[c], orow, row_x, rows_valid, lane_e);
      }
    }
  }
  STAMP(4);
#ifdef WAE_GLU_STAMPS
  if (p.stamps && lane == 0) {   // every wave: its own sums of the GEMM-1 chunk loop
    unsigned long long* o = p.stamps + (size_t)blockIdx.x * 64 + 16 + wave * 4;
    o[0] = acc_wait; o[1] = acc_bar; o[2] = acc_issue; o[3] = acc_gemm;
  }
  if (p.stamps && threadIdx.x == 0) {
    st_[5] = __builtin_amdgcn_s_memrealtime();
    st_[6] = acc_wait; st_[7] = acc_bar; st_[8] = acc_issue; st_[9] = acc_gemm;
#pragma unroll
    for (int i = 0; i < 16; ++i) p.stamps[(size_t)blockIdx.x * 64 + i] = st_[i];
  }
#endif
#undef GLU_T
#undef GLU_ROW0
#undef GLU_ZROW
}

// what both entries ask of a descriptor (the dense one asks for T > 0 as well; the list's lengths are in its table)
static inline int glu_validate_shape(const wae_glu_desc* d) {
  WAE_REQUIRE(d != nullptr, "glu: null desc");
  WAE_REQUIRE(wae_dtype_ok(d->dtype), "glu: bad dtype %d", d->dtype);
  WAE_REQUIRE(d->B > 0, "glu: B,T must be positive");
  WAE_REQUIRE(d->Rp > 0 && d->Rp % 128 == 0 && d->Ccp >= 0 && d->Ccp % 64 == 0,
              "glu: Rp must be a multiple of 128 and Ccp of 64 (got %d,%d)", d->Rp, d->Ccp);
  WAE_REQUIRE(d->Hp > 0 && d->Hp % 32 == 0 && d->Hp <= 256, "glu: Hp must be a multiple of 32, <= 256");
  WAE_REQUIRE(d->ktaps >= 1 && d->dilation >= 1, "glu: ktaps, dilation must be >= 1");
  return WAE_OK;
}

// LDS ring of a launch: `fixed` bytes (staging tiles, bias and zb tables) and as many weight-chunk slots as fit, four at the most
// (four slots -- weights three chunks ahead -- measure best once the requests really stay in flight: 57.2 us against 58.1 (3 slots)
// and 59.1 (5) at C2 inference, tools/time_glu.py); fewer than two: the geometry has no kernel
static inline int glu_ring_slots(int NW, int CHB, bool half_cu, int Rp, int Hp, size_t* fixed) {
  *fixed = (size_t)NW * 4096 + (size_t)(Rp + 2 * Hp) * 4;
  const size_t budget = (half_cu ? 80 : 160) * 1024;
  const int nslot = *fixed + 2 * (size_t)CHB <= budget ? (int)((budget - *fixed) / CHB) : 0;
  return nslot > 4 ? 4 : nslot;
}
