"""Backward pass of the decoder hot path (host orchestration; all arithmetic in libwae_hip.so).

Gradient flow (autograd of wavenet.py:164-216 + vqwae_train.py:758-766), with "hat" = gradient already carrying the
layer's sqrt(.5):
    head_bwd:   dy, dh1, dskip                                                    (csrc/head_bwd.hip)
    layer l = L-1 .. 0:
        du/dz:  dz_l  = gate'(z_l) * (W_out_l^T dxhat_{l+1} + W_skip_l^T dskip)   (wae_gemm_tm, GATE_BWD)
        wgrad:  dW1_l, dWc_l, dzb_l (ones columns), dW_out_l                      (wae_gemm_tn)
        dx:     dxhat_l = sqrt(.5) * (dxhat_{l+1} + sum_tap W1_tap^T dz_l[t+s])   (wae_gemm_tm, RESIDUAL)
    dc = sum_l Wc_l^T dz_l  (one GEMM over all layers),  dW_skip of all layers (one GEMM), head + first-conv weights,
    scatter into the gradient arena, gproj backward, weight-norm backward.
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L
from . import packing as P
from .frontend import encoder_convs
from .step_state import saved_for

RS = math.sqrt(0.5)


def _prepare_bwd(eng):
    if eng._bwd_ready:
        return
    g, dev, lay = eng.g, eng.device, eng.lay
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    # Which weight-gradient launches this engine uses follows from eng.opt (options.py: read once per engine): the arenas sized below, the
    # job tables of every (B, T) workspace and the scatter lists all follow from it.
    eng.opt_tn_stream = eng.dt in (L.WAE_BF16, L.WAE_F16) and eng.opt.tn_stream
    eng.opt_tn_static = eng.opt.tn_static
    eng.opt_tn_static_head = eng.opt.tn_static_head
    eng.m_bu = up(P.bwd_u_map(g, lay, eng.dt))
    eng.m_bx = up(P.bwd_x_map(g, lay, eng.dt))
    # K_X(l) + K_U(l-1) in one launch (csrc/glu_bwd.hip).  16-bit storage: the round-5 kernel (two workgroups per CU, the residual
    # launch's own weight stream and chunk order) is the DEFAULT where it has an instantiation -- 5.72 -> 5.52 ms per C2 train step once
    # its epilogues stopped reloading spilled addresses (profiles/EXPERIMENT_LOG.md); EngineOptions.bwd_fused "0" keeps the two launches.
    # fp32 keeps the two launches unless asked ("1"): its fused form is the round-1 kernel (118 us against 60 + 50).
    is16 = eng.dt in (L.WAE_BF16, L.WAE_F16)
    sup = eng.lib.wae_glu_bwd_fused_supported16(g.Rp, g.Hp) if is16 else eng.lib.wae_glu_bwd_fused_supported(g.Rp, g.Hp)
    want = eng.opt.bwd_fused == "1" or (eng.opt.bwd_fused == "auto" and is16)
    eng.fused_bwd = bool(sup) and g.Sp % (64 if is16 else 32) == 0 and want
    eng.m_bxf = eng.w_bxf = None
    if eng.fused_bwd:
        eng.m_buo = up(P.bwd_uo_map(g, lay, eng.dt))
        eng.n_buo = eng.m_buo.numel()
        eng.w_buo = torch.zeros(g.layers * eng.n_buo, dtype=eng.tdtype, device=dev)
        if not is16:
            eng.m_bxf = up(P.bwd_x_map(g, lay, eng.dt, interleave=False))     # the fp32 kernel walks the taps one by one
            eng.w_bxf = torch.zeros(g.layers * eng.m_bxf.numel(), dtype=eng.tdtype, device=dev)
    eng.m_bc = up(P.bwd_c_map(g, lay, eng.dt)) if g.Ccp else None
    eng.m_hb_w = up(P.head_bwd_map(g, lay, eng.dt)) if not eng.wide_head else torch.zeros(0, dtype=torch.int32, device=dev)
    eng.n_bu, eng.n_bx = eng.m_bu.numel(), eng.m_bx.numel()
    eng.w_bu = torch.zeros(g.layers * eng.n_bu, dtype=eng.tdtype, device=dev)
    eng.w_bx = torch.zeros(g.layers * eng.n_bx, dtype=eng.tdtype, device=dev)
    eng.w_bc = torch.zeros(eng.m_bc.numel(), dtype=eng.tdtype, device=dev) if g.Ccp else None
    eng.w_hb = torch.zeros(eng.m_hb_w.numel(), dtype=eng.tdtype, device=dev)
    sm = P.grad_scatter_maps(g, lay)
    eng.sm = {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in sm.items()}
    eng.d_eff = torch.zeros_like(eng.params)
    eng.grads = torch.zeros_like(eng.params)
    # the squared norm of the step's gradients as wae_grad_finish sums it (one double; cleared with the gradient accumulators)
    eng.gn_acc = torch.zeros(2, dtype=torch.float64, device=dev)
    # dense weight-gradient tiles (fp32), one allocation so a single memset clears them
    sizes = dict(c1=g.layers * 2 * g.Hp * sm["ld1"], co=g.layers * g.Rp * sm["ldo"], cs=g.Sp * sm["lds"],
                 c3=g.Op * sm["ldh"], c1h=g.Sp * sm["ldh"], ctab=P._ru(g.O, 128) * g.Rp, fb=g.Rp)
    if static_tn_geometry(eng):
        # wae_gemm_tn_static (kind OUTSKIP) writes dW_out / dW_skip of a layer transposed: rows = gated channel, and the out bias
        # as one more row; the skip bias (column sums of dS, the same for every layer) is the Cb of the LAST layer's OUTSKIP job, whose
        # first operand is dS (its conv1x1_out gradient is dead): a plain (Sp,) vector in the first floats of `cbs`
        sizes.update(coT=g.layers * sm["ldoT_rows"] * g.Rp, csT=g.layers * g.Hp * g.Sp, cbs=g.Sp * P.ONES_PAD)
    total = sum(sizes.values())
    eng.cbuf = torch.zeros(total, dtype=torch.float32, device=dev)
    eng.cview, off = {}, 0
    for k, n in sizes.items():
        eng.cview[k] = eng.cbuf[off:off + n]
        off += n
    eng._bwd_ready = True


def pack_bwd_weights(eng):
    _prepare_bwd(eng)
    lib, st, g, lay = eng.lib, eng.stream(), eng.g, eng.lay
    jobs = eng._pack_bwd_jobs
    if jobs is None:
        eff = eng.eff.data_ptr()
        J = lambda mp, dst, n, nb, ss, ds: L.GatherJob(eff, mp.data_ptr(), dst.data_ptr(), n, ss, ds, nb, eng.dt)
        lst = [J(eng.m_bu, eng.w_bu, eng.n_bu, g.layers, lay.layer_stride, eng.n_bu),
               J(eng.m_bx, eng.w_bx, eng.n_bx, g.layers, lay.layer_stride, eng.n_bx)]
        if eng.fused_bwd:
            lst.append(J(eng.m_buo, eng.w_buo, eng.n_buo, g.layers, lay.layer_stride, eng.n_buo))
            if eng.m_bxf is not None:
                lst.append(J(eng.m_bxf, eng.w_bxf, eng.n_bx, g.layers, lay.layer_stride, eng.n_bx))       # tap by tap (fp32)
        if g.Ccp:
            lst.append(J(eng.m_bc, eng.w_bc, eng.m_bc.numel(), 1, 0, 0))
        if eng.wide_head:
            lst += [J(eng.m_hwide[k], eng.w_hwide[k], eng.m_hwide[k].numel(), 1, 0, 0) for k in ("w3t", "w1t")]
        else:
            lst.append(J(eng.m_hb_w, eng.w_hb, eng.m_hb_w.numel(), 1, 0, 0))
        # ... and the step's two gradient accumulators cleared by the same launch (fill jobs: no map; round 5 cleared them with two
        # torch fills of 43 + 50 MB between launches, 19 us that this launch's idle store bandwidth absorbs)
        lst += [L.GatherJob(None, None, t_.data_ptr(), t_.numel(), 0, 0, 1, L.WAE_F32) for t_ in (eng.d_eff, eng.cbuf)]
        lst.append(L.GatherJob(None, None, eng.gn_acc.data_ptr(), 2 * eng.gn_acc.numel(), 0, 0, 1, L.WAE_F32))
        jobs = eng._pack_bwd_jobs = (L.GatherJob * len(lst))(*lst)
    L.check(lib.wae_pack_gather_multi(jobs, len(jobs), st), "pack backward weights + clear the gradient accumulators")


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _tm_srcs(srcs):
    """srcs: list of (device ptr int, row stride elems, cols, shift) -> the four arrays wae_gemm_tm / wae_gemm_tm_ce take"""
    return (_arr(ctypes.c_void_p, [s[0] for s in srcs]), _arr(ctypes.c_int64, [s[1] for s in srcs]),
            _arr(ctypes.c_int32, [s[2] for s in srcs]), _arr(ctypes.c_int32, [s[3] for s in srcs]))


def _tm(eng, B, T, M, mode, alpha, srcs, w_ptr, out_ptr, out_stride, aux_ptr=None, aux_stride=0, flags=0, st=None):
    """srcs: list of (device ptr int, row stride elems, cols, shift)"""
    d = L.TmDesc(eng.dt, B, T, M, len(srcs), mode, alpha, flags)
    L.check(eng.lib.wae_gemm_tm(ctypes.byref(d), *_tm_srcs(srcs), ctypes.c_void_p(w_ptr), ctypes.c_void_p(out_ptr),
                                out_stride, ctypes.c_void_p(aux_ptr) if aux_ptr else None, aux_stride, st if st is not None else eng.stream()), "gemm_tm")


def _tm_ce(eng, B, T, M, mode, srcs, w_ptr, out_ptr, out_stride, bias_ptr, ce):
    """wae_gemm_tm_ce (modes 5 / 6 of the wide head): ce is an L.TmCe"""
    d = L.TmDesc(eng.dt, B, T, M, len(srcs), mode, 1.0, 0)
    L.check(eng.lib.wae_gemm_tm_ce(ctypes.byref(d), *_tm_srcs(srcs), ctypes.c_void_p(w_ptr),
                                   ctypes.c_void_p(out_ptr) if out_ptr else None, out_stride, ctypes.c_void_p(bias_ptr),
                                   ctypes.byref(ce), eng.stream()), "gemm_tm_ce")


def _timed(eng, sink, fn):
    """fn() -- with a list `sink` (bench.py's event hooks), between a pair of HIP events on the current stream, appended to it"""
    if sink is None:
        return fn()
    cur = torch.cuda.current_stream(eng.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(cur)
    fn()
    e1.record(cur)
    sink.append((e0, e1))


def _await_packed_weights(eng):
    """The backward's packed weights and cleared gradient accumulators: train_step queued that launch on a side stream right behind
    weight norm (eng.flight.early_pack: wait for it); any other caller packs here."""
    early = eng.flight.take_early_pack()
    if early is not None:
        eng.join(early)
    else:
        pack_bwd_weights(eng)      # (also clears eng.d_eff and eng.cbuf)


def tn_tiles_overlap(tiles, B):
    """Do two tiles of a table add into the same fp32 element of C?  -> (i, j), the first such pair in address order, or None.
    A tile owns, in each of its m_valid rows, the columns [0, n_valid) and [ones_col, ones_col + B) behind its C pointer (include/wae.h);
    what wae_gemm_tn_tiles_det's single reduce launch (ordered = 0) needs is that no element has two owners."""
    spans = []                                          # (first byte, one past the last byte, tile)
    for i, t in enumerate(tiles):
        cols = [(0, t.n_valid)] if t.n_valid > 0 else []
        if t.ones_col >= 0:
            cols.append((t.ones_col, t.ones_col + B))
        if len(cols) == 2 and cols[1][0] <= cols[0][1]:    # the tile's own two ranges touch: one range (one thread per element adds both)
            cols = [(0, max(cols[0][1], cols[1][1]))]
        for c0, c1 in cols:
            first = (t.C or 0) + 4 * (np.arange(t.m_valid, dtype=np.int64) * t.ldc + c0)
            spans += [(int(a), int(a) + 4 * (c1 - c0), i) for a in first]
    spans.sort()
    end, owner = -1, -1
    for a, b, i in spans:
        if a < end and i != owner:
            return (min(owner, i), max(owner, i))
        if b > end:
            end, owner = b, i
    return None


class TileTable:
    """Host builder of a device array of wae_tn_tile (include/wae.h): each add() is one contraction
    C[M][N (+ones)] += alpha * P^T Q, cut into 128x128 output tiles."""

    def __init__(self, eng):
        self.eng, self.tiles = eng, []
        self.det_checked = None        # launch_det: the batch size the table's tiles were last found disjoint in C for

    def add(self, M, N, shift, ones_col, alpha, p_ptr, p_stride, q_ptr, q_stride, c_ptr, ldc, onehot_ptr=0):
        es = self.eng.w_glu.element_size()
        nmax = max(N, ones_col + 1) if ones_col >= 0 else N
        TN = 128                                     # csrc/gemm_tn.hip: 128 x 128 output tiles
        for mt in range((M + 127) // 128):
            for nt in range((nmax + TN - 1) // TN):
                oc = ones_col - TN * nt if (ones_col >= 0 and 0 <= ones_col - TN * nt < TN) else -1
                self.tiles.append(L.TnTile(
                    (p_ptr + mt * 128 * es) if p_ptr else None, q_ptr + nt * TN * es, onehot_ptr or None,
                    c_ptr + (mt * 128 * ldc + nt * TN) * 4, p_stride, q_stride, ldc,
                    min(128, M - 128 * mt), max(0, min(TN, N - TN * nt)), 128 * mt, shift, oc, alpha))

    def finalize(self, B):
        arr = (L.TnTile * len(self.tiles))(*self.tiles)
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.dev = host.to(self.eng.device)
        self.n = len(self.tiles)
        # measured on C2 (tools/ablate_tn.py): ~1200 workgroups (2-3 per slot) beat fewer, longer ones; keep >= 512 steps each
        self.splits = max(1, min(16, round(1200 / max(1, self.n * B))))
        return self

    def launch(self, B, T):
        eng = self.eng
        if eng.opt.deterministic:      # the engine's one partials buffer, reused by every table's launch on the one stream
            return self.launch_det(B, T, eng.det_buffer("tn", self.det_floats(B, T)))
        L.check(eng.lib.wae_gemm_tn_tiles(eng.dt, L.ptr(self.dev), self.n, B, T, self.splits, eng.stream()), "gemm_tn_tiles")

    def det_floats(self, B, T):
        """fp32 elements of the partials buffer launch_det needs for this table"""
        return int(self.eng.lib.wae_gemm_tn_tiles_det_floats(self.n, B, T, self.splits))

    def launch_det(self, B, T, partials):
        """The same contractions with their sums in a fixed order (wae_gemm_tn_tiles_det, one reduce launch): `partials` is an fp32
        tensor of at least det_floats(B, T) elements that no other stream uses meanwhile.  Raises if two tiles share an element of C."""
        eng = self.eng
        if self.det_checked != B:
            pair = tn_tiles_overlap(self.tiles, B)
            if pair is not None:
                raise ValueError(f"tiles {pair[0]} and {pair[1]} of the table add into the same element of C: the single reduce launch "
                                 "of wae_gemm_tn_tiles_det (ordered = 0) would add them in no defined order")
            self.det_checked = B
        L.check(eng.lib.wae_gemm_tn_tiles_det(eng.dt, L.ptr(self.dev), self.n, B, T, self.splits, L.ptr(partials), partials.numel(), 0,
                                              eng.stream()), "gemm_tn_tiles_det")


def _ncu(eng):
    return torch.cuda.get_device_properties(eng.device).multi_processor_count


class _TeamTable:
    """What the two team launches share: *groups* of equally many jobs, and the (group, 32-row time slab) list cut into equal
    contiguous shares, one per *team* of len(group) workgroups (packing.tn_team_shares)."""

    def __init__(self, eng, B, T):
        self.eng, self.B, self.T = eng, B, T
        self.groups = []          # list of lists of job records

    def begin_group(self):
        self.groups.append([])

    def _upload(self, job_type, n_groups, ncu, swap=False):
        """self.groups (swap: two variants of n_groups groups each) and their team shares on ncu CUs -> device arrays"""
        gs = len(self.groups[0])
        assert all(len(g) == gs for g in self.groups), "every layer must contribute the same list of jobs"
        sh = P.tn_team_shares(n_groups, self.B, self.T, gs, ncu or _ncu(self.eng), swap)
        self.team_size, self.nteams, self.nwg = gs, sh.nteams, sh.nwg
        jobs = [j for g in self.groups for j in g]
        segs = [L.TsSeg(*s) for s in sh.segs]
        dev = self.eng.device
        self.jobs_dev = torch.frombuffer(bytearray(bytes((job_type * len(jobs))(*jobs))), dtype=torch.uint8).to(dev)
        self.segs_dev = torch.frombuffer(bytearray(bytes((L.TsSeg * len(segs))(*segs))), dtype=torch.uint8).to(dev)
        self.team_seg_dev = torch.tensor(sh.team_seg, dtype=torch.int32, device=dev)


class StreamTable(_TeamTable):
    """Host builder for wae_gemm_tn_stream (csrc/gemm_tn_stream.hip): the weight-gradient contractions of every layer as
    ONE launch.  A *group* is the list of jobs of one layer (every dilated-conv tap, the conditioning 1x1 with the per-clip
    zb sums, conv1x1_out with its bias), each cut into 384 x 256 output regions; all groups have the same number of jobs."""
    RM, RN, KT = 384, 256, 32

    def __init__(self, eng, B, T):
        super().__init__(eng, B, T)
        self.lead_jobs = 0        # the first lead_jobs jobs of every group are full-size (the taps): the pacing reference

    def add(self, M, N, shift, ones_col, alpha, p_ptr, p_stride, q_ptr, q_stride, c_ptr, ldc):
        """C[M][N (+ B ones columns at ones_col)] += alpha * P^T Q ; p_ptr == 0: placeholder jobs that do nothing."""
        es = 2
        nmax = max(N, ones_col + self.B) if ones_col >= 0 else N
        for mt in range((M + self.RM - 1) // self.RM):
            for nt in range((nmax + self.RN - 1) // self.RN):
                nv = max(0, min(self.RN, N - self.RN * nt))
                oc = -1
                if ones_col >= 0 and 0 <= ones_col - self.RN * nt < self.RN:
                    oc = ones_col - self.RN * nt
                    assert oc + self.B <= self.RN and nv % 8 == 0 and oc >= nv, "ones columns must fit behind the region's data"
                if nv == 0 and oc < 0:
                    continue
                mv = min(self.RM, M - self.RM * mt) if p_ptr else 0
                self.groups[-1].append(L.TsJob((p_ptr + mt * self.RM * es) if p_ptr else None, q_ptr + nt * self.RN * es,
                                               c_ptr + (mt * self.RM * ldc + nt * self.RN) * 4, p_stride, q_stride, ldc,
                                               mv, nv, shift, oc, alpha, 0))

    def finalize(self):
        self._upload(L.TsJob, len(self.groups), None)
        # (the kernel's team pacing and equal-time shares -- rounds 2-3, measured slower: profiles/EXPERIMENT_LOG.md -- stay reachable
        #  through wae_gemm_tn_stream's own arguments; the product launches unpaced teams)
        self.pace = torch.zeros(self.nteams * 8, dtype=torch.int32, device=self.eng.device)
        self.window, self.pace_from = 0, self.lead_jobs
        return self

    def launch(self):
        eng = self.eng
        L.check(eng.lib.wae_gemm_tn_stream(eng.dt, L.ptr(self.jobs_dev), L.ptr(self.segs_dev), L.ptr(self.team_seg_dev), self.nteams,
                                           self.team_size, self.nwg, self.B, self.T, L.ptr(self.pace), self.window, self.pace_from, eng.stream()),
                "gemm_tn_stream")


def _cuts(n, cap, gran):
    """[0, n) in the fewest equal parts of at most `cap` columns, each a multiple of `gran` -> [(first column, width)]"""
    parts = -(-n // cap)
    w = -(-(-(-n // parts)) // gran) * gran
    out, c = [], 0
    while c < n:
        out.append((c, min(w, n - c)))
        c += w
    return out


def static_tn_geometry(eng):
    """The static-schedule weight-gradient launch (csrc/gemm_tn_static.hip): 16-bit operands, Ccp = 64.  A job of the kernel is one
    output region -- TAPS: dz (<= 384 columns) x x (<= 256), COND: dz (<= 384) x [c (64) | ones], OUTSKIP: u (<= 192) x [Ghat (<= 256) |
    dS (<= 256)] -- and a layer whose matrices are wider is cut into several jobs per kind (round 5: C5's 512-wide layers are 18 jobs
    in three groups of six; C2 and hps/vqwae.json stay at the five jobs of one region each).  WAE_TN_STATIC=0 keeps the any-shape
    stream-K kernel (csrc/gemm_tn_stream.hip)."""
    g = eng.g
    return (eng.dt in (L.WAE_BF16, L.WAE_F16) and eng.opt_tn_static and g.Ccp == 64 and (2 * g.Hp) % 64 == 0 and g.Rp % 128 == 0
            and g.Sp % 128 == 0)


def static_tn_split(eng):
    """Does a layer need more than one job per kind (see static_tn_geometry)?"""
    g = eng.g
    return 2 * g.Hp > 384 or g.Rp > 256 or g.Sp > 256 or g.Hp > 192


def static_tn_shape(eng, B, T):
    """... and shapes it can address: one ones column per clip inside one 32-column tile, every operand clip below 2^30 bytes
    (the per-clip buffer descriptors carry 32-bit offsets; rows before a clip wrap to offsets beyond num_records)."""
    g = eng.g
    # bytes per time row of the widest operand array (the head's dy and the first conv's one-hot operand ride in the launch too)
    return static_tn_geometry(eng) and use_stream_tn(eng) and B <= 32 and static_tn_clip_bytes(g, T) < (1 << 30)


def static_tn_clip_bytes(g, T):
    """The largest operand clip the static launch addresses, in bytes (what wae_gemm_tn_static takes as max_clip_bytes)."""
    widest = max(g.layers * 2 * g.Hp, g.Ku, g.Rp, g.Sp, g.Ccp, g.Op, P._ru(g.O, 128)) * 2
    return (T + (g.k - 1) * max(g.dilations) + 32) * widest


def static_head(eng, B, T):
    """The head's weight gradients (dW3 = dy^T h1, dW1 = dh1^T h0, their biases = column sums of dy / dh1) and -- class-id input -- the
    first conv's (onehot^T dx0) ride in the static launch as one more group of jobs when they fit its regions (P <= 384 columns,
    Q <= 256) and a layer is one group of at least five jobs (k >= 3, no cut matrices); otherwise they stay on the 128 x 128 tile
    launches (csrc/gemm_tn.hip)."""
    g = eng.g
    return (static_tn_shape(eng, B, T) and not static_tn_split(eng) and not eng.wide_head and g.k >= 3 and g.Op <= 384 and g.Sp <= 256
            and P._ru(g.O, 128) <= 384 and eng.opt_tn_static_head)


class StaticStreamTable(_TeamTable):
    """Host builder for wae_gemm_tn_static: per layer one job per dilated-conv tap (TAPS), one for conv1x1c + the per-clip sums of
    dz (COND) and one for conv1x1_out + conv1x1_skip (OUTSKIP).  Teams and segments as StreamTable."""

    def add(self, **kw):
        f = dict(P=None, Q0=None, Q1=None, C0=None, C1=None, Cb=None, p_stride=0, q0_stride=0, q1_stride=0, ldc0=0, ldc1=0,
                 m_valid=0, n0_valid=0, n1_valid=0, shift=0, ones_col=-1, kind=0, alpha=1.0, pad_=0)
        f.update(kw)
        assert f["shift"] <= 0 and f["m_valid"] % 8 == 0 and f["n0_valid"] % 8 == 0 and f["n1_valid"] % 8 == 0
        self.groups[-1].append(L.TqJob(*[f[n] for n, _ in L.TqJob._fields_]))

    def finalize(self, ncu=None):
        """ncu: the CUs this launch may count on (default: all) -- a launch that runs BESIDE an under-filled sweep takes the idle ones"""
        # The members of a team walk the same slabs, but a slab costs the out + skip member 704 operand columns (96 tiles), a tap member
        # 640 and the conditioning member 448 (36 tiles): by workgroup lives (tools/tq_member_lives.py, C2) 1 274 / 1 150-1 176 / 954 us,
        # and the launch ends with the slowest.  A member's job kind is a field of the job record, so the second half of every team's
        # share runs on a copy of the groups in which the last two slots have changed places: the two members each do half of both.
        # (One more segment per team = one more prologue + flush per member; the partial sums are added atomically either way.)
        ng, gs = len(self.groups), len(self.groups[0])
        swap = bool(self.eng.opt.tn_swap and gs >= 2)
        if swap:
            def swapped(grp):
                k = [j.kind if j.m_valid > 0 else -1 for j in grp]
                if k[-2:] == [L.TQ_COND, L.TQ_OUTSKIP]:
                    return grp[:-2] + [grp[-1], grp[-2]]
                return grp
            self.groups = self.groups + [swapped(grp) for grp in self.groups]
        self._upload(L.TqJob, ng, ncu, swap)
        self.stamps = None          # diagnostic builds (-DWAE_TQ_STAMPS): an int64 [nwg][16][4] tensor, zeroed before the launch
        # (team pacing of the tap members -- round 4: 6.7 -> 4.7 GB of HBM traffic at identical time, profiles/r04_tq_experiments.txt --
        #  stays reachable through wae_gemm_tn_static's own arguments; the product launches unpaced: window 0)
        self.ntaps = gs - 2
        self.window = self.window_cond = 0
        self.pace = torch.zeros(self.nteams, dtype=torch.int32, device=self.eng.device)
        return self

    def launch(self):
        eng = self.eng
        L.check(eng.lib.wae_gemm_tn_static(eng.dt, L.ptr(self.jobs_dev), L.ptr(self.segs_dev), L.ptr(self.team_seg_dev), self.nteams,
                                           self.team_size, self.nwg, self.B, self.T, L.ptr(self.stamps), L.ptr(self.pace), self.window,
                                           self.window_cond, self.ntaps, static_tn_clip_bytes(eng.g, self.T), eng.stream()),
                "gemm_tn_static")


def use_stream_tn(eng):
    """16-bit runs take every layer's weight gradients in one launch after the backward sweep (needs the residual-stream gradient
    of every layer kept); fp32 (the parity mode) keeps one wae_gemm_tn_tiles launch per layer."""
    _prepare_bwd(eng)
    return eng.opt_tn_stream


def bwd_workspace(eng, B, T):
    key = ("bwd", B, T)
    ws = eng._ws.get(key)
    if ws is None:
        g, dev, td = eng.g, eng.device, eng.tdtype
        ws = dict(dz=torch.zeros(B, T, g.layers * 2 * g.Hp, dtype=td, device=dev),
                  gx=[torch.zeros(B, T, g.Rp, dtype=td, device=dev) for _ in range(g.layers if use_stream_tn(eng) else 2)],
                  gzero=torch.zeros(B, T, g.Rp, dtype=td, device=dev),
                  gtmp=torch.zeros(B, T, g.Rp, dtype=td, device=dev) if eng.dropout > 0 else None,
                  dy=torch.zeros(B, T, g.Op, dtype=td, device=dev),
                  dh1=torch.zeros(B, T, g.Sp, dtype=td, device=dev),
                  dskip=torch.zeros(B, T, g.Sp, dtype=td, device=dev),
                  dc=torch.zeros(B, T, max(g.Ccp, 64), dtype=td, device=dev),
                  ids=torch.zeros(B, T, dtype=torch.int32, device=dev),
                  onehot=(torch.zeros(B, T, P._ru(g.O, 128), dtype=td, device=dev)
                          if static_head(eng, B, T) and not g.scalar_input else None),
                  # scalar input (first_conv is a 1x1 on one channel): operand [x | 1 | 0 ...] of its weight/bias gradient
                  xs1=torch.zeros(B, T, 64, dtype=td, device=dev) if g.scalar_input else None)
        _build_tile_tables(eng, ws, eng._ws[(B, T, True)], B, T)
        eng._ws[key] = ws
    return ws


def _layer_operands(eng, ws, fw, l):
    """Device addresses of layer l's weight-gradient operands: dz_l, the convolution's operand (dW1 contracts dz against it: the
    masked one under dropout), u_l, and the layer's dense dW1 | dWc | zb tile"""
    g, es, Z2 = eng.g, eng.w_glu.element_size(), 2 * eng.g.Hp
    xl = fw["xd"][l] if "xd" in fw else fw["x"][l]
    return (ws["dz"].data_ptr() + l * Z2 * es, xl.data_ptr(), fw["u"].data_ptr() + l * g.Hp * es,
            eng.cview["c1"].data_ptr() + l * Z2 * eng.sm["ld1"] * 4)


def _layer_contractions(eng, ws, fw, l, g_next):
    """packing.tn_layer_contractions of layer l of the stack (g_next: address of dx-hat of layer l + 1, None or 0: see there)"""
    g, sm = eng.g, eng.sm
    dz, x, u, c1l = _layer_operands(eng, ws, fw, l)
    return P.tn_layer_contractions(g, g.dilations[l], 1.0 / eng.grad_scale, dz, g.layers * 2 * g.Hp, x,
                                   fw["c_up"].data_ptr() if g.Ccp else 0, g_next, u, c1l, sm["ld1"],
                                   eng.cview["co"].data_ptr() + l * g.Rp * sm["ldo"] * 4, sm["ldo"])


def _static_layer_jobs(eng, ws, fw, l):
    """Layer l as job records of the static launch (StaticStreamTable.add's keywords): matrices wider than a region are cut"""
    g, sm = eng.g, eng.sm
    es, Z2, ia = eng.w_glu.element_size(), 2 * g.Hp, 1.0 / eng.grad_scale
    dzs, d = g.layers * Z2, g.dilations[l]
    dz_ptr, x_ptr, u_ptr, c1l = _layer_operands(eng, ws, fw, l)
    m_taps, n_taps = _cuts(Z2, 384, 64), _cuts(g.Rp, 256, 128)
    m_cond = _cuts(Z2, 384, 32)
    m_os, n_os0, n_os1 = _cuts(g.Hp, 192, 64), _cuts(g.Rp, 256, 128), _cuts(g.Sp, 256, 128)
    jobs = []
    for tap in range(g.k):
        for m0, mw in m_taps:
            for n0, nw in n_taps:
                jobs.append(dict(kind=L.TQ_TAPS, P=dz_ptr + m0 * es, p_stride=dzs, m_valid=mw, Q0=x_ptr + n0 * es,
                                 q0_stride=g.Rp, n0_valid=nw, shift=-(g.k - 1 - tap) * d,
                                 C0=c1l + (m0 * sm["ld1"] + tap * g.Rp + n0) * 4, ldc0=sm["ld1"], alpha=ia))
    for m0, mw in m_cond:
        jobs.append(dict(kind=L.TQ_COND, P=dz_ptr + m0 * es, p_stride=dzs, m_valid=mw, Q0=fw["c_up"].data_ptr(), q0_stride=g.Ccp,
                         n0_valid=g.Ccp, ones_col=g.Ccp, C0=c1l + (m0 * sm["ld1"] + g.k * g.Rp) * 4, ldc0=sm["ld1"], alpha=ia))
    has_out = l < g.layers - 1       # the last layer's x' is dead (wavenet.py:205-207): no conv1x1_out gradient
    coTl = eng.cview["coT"].data_ptr() + l * sm["ldoT_rows"] * g.Rp * 4
    csTl = eng.cview["csT"].data_ptr() + l * g.Hp * g.Sp * 4
    for m0, mw in m_os:
        if has_out:
            for i in range(max(len(n_os0), len(n_os1))):
                j = dict(kind=L.TQ_OUTSKIP, P=u_ptr + m0 * es, p_stride=g.Ku, m_valid=mw, alpha=ia)
                if i < len(n_os0):
                    n0, nw = n_os0[i]
                    j.update(Q0=ws["gx"][l + 1].data_ptr() + n0 * es, q0_stride=g.Rp, n0_valid=nw,
                             C0=coTl + (m0 * g.Rp + n0) * 4, ldc0=g.Rp)
                    if m0 == 0:          # the out bias: column sums of Ghat, formed by the job that holds rows 0..63 of u
                        j.update(Cb=coTl + (g.Hp * g.Rp + n0) * 4)
                if i < len(n_os1):
                    n1, nw1 = n_os1[i]
                    j.update(Q1=ws["dskip"].data_ptr() + n1 * es, q1_stride=g.Sp, n1_valid=nw1,
                             C1=csTl + (m0 * g.Sp + n1) * 4, ldc1=g.Sp)
                jobs.append(j)
        else:
            # ... which frees the job's first operand: dS takes its place, and the column sums the kernel forms of that operand
            # are the skip bias gradient (the same for every layer, modules.py:157-160)
            for n1, nw1 in n_os1:
                j = dict(kind=L.TQ_OUTSKIP, P=u_ptr + m0 * es, p_stride=g.Ku, m_valid=mw, Q0=ws["dskip"].data_ptr() + n1 * es,
                         q0_stride=g.Sp, n0_valid=nw1, C0=csTl + (m0 * g.Sp + n1) * 4, ldc0=g.Sp, alpha=ia)
                if m0 == 0:
                    j.update(Cb=eng.cview["cbs"].data_ptr() + n1 * 4)
                jobs.append(j)
    return jobs


def _static_head_group(eng, ws, fw, l0, l1):
    """The group of jobs that rides with layers [l0, l1) of the static launch (static_head): the head's with the top layer, the first
    conv's with the bottom one; [] when neither is in the range"""
    g, sm, ia = eng.g, eng.sm, 1.0 / eng.grad_scale
    gs = g.k + 2
    first = None
    if not g.scalar_input and l0 == 0:
        W1 = P._ru(g.O, 128)
        first = dict(kind=L.TQ_TAPS, P=ws["onehot"].data_ptr(), p_stride=W1, m_valid=W1, Q0=ws["gx"][0].data_ptr(),
                     q0_stride=g.Rp, n0_valid=g.Rp, C0=eng.cview["ctab"].data_ptr(), ldc0=g.Rp, alpha=ia / RS)
    if l1 < g.layers:
        return ([first] + [{}] * (gs - 1)) if first else []
    # the head: two contractions and two column-sum jobs (kind COND without a Q operand: per-clip sums of P's columns,
    # the layout the ones columns of the tile launches had); the first conv's takes the free third slot
    c3, c1h = eng.cview["c3"].data_ptr(), eng.cview["c1h"].data_ptr()
    dy, dh1 = ws["dy"].data_ptr(), ws["dh1"].data_ptr()
    return [dict(kind=L.TQ_TAPS, P=dy, p_stride=g.Op, m_valid=g.Op, Q0=fw["h1"].data_ptr(), q0_stride=g.Sp, n0_valid=g.Sp,
                 C0=c3, ldc0=sm["ldh"], alpha=ia),
            dict(kind=L.TQ_TAPS, P=dh1, p_stride=g.Sp, m_valid=g.Sp, Q0=fw["h0"].data_ptr(), q0_stride=g.Sp, n0_valid=g.Sp,
                 C0=c1h, ldc0=sm["ldh"], alpha=ia),
            first or {}] + [{}] * (gs - 5) + [
            dict(kind=L.TQ_COND, P=dy, p_stride=g.Op, m_valid=g.Op, ones_col=g.Sp, C0=c3, ldc0=sm["ldh"], alpha=ia),
            dict(kind=L.TQ_COND, P=dh1, p_stride=g.Sp, m_valid=g.Sp, ones_col=g.Sp, C0=c1h, ldc0=sm["ldh"], alpha=ia)]


def _build_stream_table(eng, ws, fw, B, T, l0, l1, ncu=None):
    """One team launch over the weight gradients of layers [l0, l1): dW1 taps, dWc + zb sums, dW_out + bias of every layer of the
    range -- the static launch where it can address the shape (static_tn_shape), else the any-shape stream-K launch.  Which ranges
    a step launches, and where: _tn_schedule."""
    g = eng.g
    if not static_tn_shape(eng, B, T):
        assert ncu is None, "a CU budget is a feature of the static launch"
        stt = StreamTable(eng, B, T)
        for l in range(l0, l1):
            stt.begin_group()
            for rec in _layer_contractions(eng, ws, fw, l, ws["gx"][l + 1].data_ptr() if l < g.layers - 1 else 0):
                stt.add(*rec)
        stt.lead_jobs = g.k
        return stt.finalize()
    stt = StaticStreamTable(eng, B, T)
    layers = [_static_layer_jobs(eng, ws, fw, l) for l in range(l0, l1)]
    # jobs that share operands (the cuts of one tap) stay side by side in their group
    ngrp, gsz = P.tn_job_groups(max(len(jobs) for jobs in layers))
    groups = [(jobs + [{}] * (ngrp * gsz - len(jobs)))[gi * gsz:(gi + 1) * gsz] for jobs in layers for gi in range(ngrp)]
    if static_head(eng, B, T):
        groups.append(_static_head_group(eng, ws, fw, l0, l1))
    for grp in groups:
        if grp:
            stt.begin_group()
            for j in grp:
                stt.add(**j)
    return stt.finalize(ncu)


def _build_tile_tables(eng, ws, fw, B, T):
    """All weight-gradient contractions of a step as two kinds of launches: one table per layer (dW1 taps, dWc + zb sums,
    dW_out + bias) and one global table (dW_skip of every layer + bias, head matrices + biases, first-conv table)."""
    g, sm = eng.g, eng.sm
    ia = 1.0 / eng.grad_scale       # fp16: the 16-bit gradients are loss-scaled, the fp32 weight gradients are not
    ws["tt_layer"] = []
    ws["stream"] = None
    if use_stream_tn(eng):
        ws["stream"] = _build_stream_table(eng, ws, fw, B, T, 0, g.layers)
    for l in range(g.layers if ws["stream"] is None else 0):
        tt = TileTable(eng)
        g_next = ws["gx"][(l + 1) % len(ws["gx"])].data_ptr() if l < g.layers - 1 else None
        for rec in _layer_contractions(eng, ws, fw, l, g_next):
            tt.add(*rec)
        ws["tt_layer"].append(tt.finalize(B))
    tt = TileTable(eng)
    c3, c1h, cs, ctab = eng.cview["c3"], eng.cview["c1h"], eng.cview["cs"], eng.cview["ctab"]
    ws["tt_head"] = ws["tt_first"] = None
    if not static_head(eng, B, T):
        tt.add(g.Op, g.Sp, 0, g.Sp, ia, ws["dy"].data_ptr(), g.Op, fw["h1"].data_ptr(), g.Sp, c3.data_ptr(), sm["ldh"])
        tt.add(g.Sp, g.Sp, 0, g.Sp, ia, ws["dh1"].data_ptr(), g.Sp, fw["h0"].data_ptr(), g.Sp, c1h.data_ptr(), sm["ldh"])
    if not static_tn_shape(eng, B, T):    # (static: dW_skip of every layer and the skip bias ride in the stream launch)
        tt.add(g.Sp, g.Ku, 0, g.Ku, ia, ws["dskip"].data_ptr(), g.Sp, fw["u"].data_ptr(), g.Ku, cs.data_ptr(), sm["lds"])
    if tt.tiles:
        ws["tt_head"] = tt.finalize(B)
    if static_head(eng, B, T) and not g.scalar_input:
        return
    tt = TileTable(eng)
    g0 = ws["gx"][0]                                    # dxhat_0 lands in gx[0 % 2]
    if g.scalar_input:     # rows 0 / 1 of the tile = d weight / d bias:  sum_t [x[t] | 1] (x) dx0[t]
        tt.add(64, g.Rp, 0, -1, ia / RS, ws["xs1"].data_ptr(), 64, g0.data_ptr(), g.Rp, ctab.data_ptr(), g.Rp)
    else:
        tt.add(g.O, g.Rp, 0, -1, ia / RS, 0, 0, g0.data_ptr(), g.Rp, ctab.data_ptr(), g.Rp, onehot_ptr=ws["ids"].data_ptr())
    ws["tt_first"] = tt.finalize(B)


def layer_segment(eng):
    """[lo, hi) of the flat arena that holds the gated layers and the head -- ~95 % of the parameters, and final as soon as the
    weight-gradient launches and gproj_bwd have run (first_conv sits in front of it, the speaker embedding, the upsampling
    network, the encoder and the codebook behind it)."""
    lay = eng.lay
    keys = list(lay.offsets)
    last = keys.index("wavenet.last_conv_layers.3.weight_v")
    hi = lay.offsets[keys[last + 1]] if last + 1 < len(keys) else lay.total
    return lay.off("wavenet.conv_layers.0.conv.bias"), hi


def layer_segment_mid(eng):
    """First arena element of layer L/2: [layer_segment lo, mid) = the lower half of the gated layers, [mid, hi) = the upper half
    and the head -- the slice a data-parallel backward hands to the all-reduce first."""
    return eng.lay.off("wavenet.conv_layers.0.conv.bias") + (eng.g.layers // 2) * eng.lay.layer_stride


def _wn_bwd_range(eng, lo, hi):
    """weight-norm backward (d_eff -> grads) of the arena slice [lo, hi)"""
    lay = eng.lay
    r0, r1 = int(np.searchsorted(lay.wn_v_off, lo)), int(np.searchsorted(lay.wn_v_off, hi))
    L.check(eng.lib.wae_weight_norm_bwd_range(L.ptr(eng.params), L.ptr(eng.d_eff), L.ptr(eng.grads), lo, hi, L.ptr(eng.wn_v),
                                              L.ptr(eng.wn_g), L.ptr(eng.wn_c), r0, r1, eng.stream()), "weight_norm_bwd")


@dataclasses.dataclass
class _Step:
    """The per-call quantities of one backward, handed from phase to phase.  A *part* is (b0, nb, stc): the clips of a chain and its
    stream -- every array of the sweep is clip-major, so a chain is the same call on its clips (engine.chain_plan); (0, B, None) = the
    whole batch on the current stream."""
    eng: object
    ws: dict
    fw: dict
    B: int
    T: int
    es: int                       # bytes of a storage element
    Z2: int                       # columns of one layer's z / dz
    dzs: int                      # row stride of dz: every layer's columns side by side
    us_off: int                   # bytes: the W_skip chunks follow the W_out chunks in the mode-2 stream
    seeds: Optional[list] = None  # dropout: the mask seeds of the train-mode forward
    fold_dc: bool = False
    tm_ev: Optional[dict] = None  # bench.py: {"gate": [(e0, e1), ...], "res": [...], "pair": [...], "sweep": [...]}
    tn_ev: Optional[list] = None  # bench.py: one (e0, e1) per weight-gradient launch
    plan: Optional[tuple] = None  # engine.chain_plan
    parts: tuple = ()
    gid32: Optional[torch.Tensor] = None
    use_gid: bool = False
    gvec: Optional[torch.Tensor] = None
    beside_done: Optional[list] = None
    finish: Optional[tuple] = None        # FinishPlan: the gather pass finishes the layers' gradients (_finish_layers); None: the split launches
    finish_acc: bool = False              # ... and sums their squares (not data parallel: the all-reduce changes them afterwards)
    small_done: Optional[list] = None     # completion events of those side launches, joined at the end of decoder_backward

    def sink(self, kind, stc=None):
        """the event list of a launch family (HIP events bracket the current stream's launches only)"""
        return None if self.tm_ev is None or stc is not None else self.tm_ev.setdefault(kind, [])


def _step(eng, B, T, seeds=None):
    g = eng.g
    is16 = eng.dt in (L.WAE_BF16, L.WAE_F16)
    # 16-bit fused sweep, three taps, 64 conditioning columns: dc = sum_l Wc_l^T dz_l is folded into the pair launches (phase A's
    # shift-0 tap already holds dz_l[t] as MFMA operand): an fp32 running sum over the layers, written in the storage dtype by the
    # launch of layer 0 (which runs the pair kernel's first half only) -- the K = L * 2Hp launch that re-read every dz is gone
    fold_dc = bool(eng.fused_bwd and seeds is None and is16 and g.k == 3 and g.Ccp == 64 and eng.opt.bwd_fold_dc)
    return _Step(eng, eng._ws[("bwd", B, T)], eng._ws[(B, T, True)], B, T, eng.w_glu.element_size(), 2 * g.Hp, g.layers * 2 * g.Hp,
                 (g.Rp // (64 if is16 else 32)) * g.NP * 4 * 1024, seeds, fold_dc, eng._tm_events, eng._tn_events,
                 parts=((0, B, None),))


def _k_u(cx, l, gn, part, flags=0):
    """du -> dz of layer l from gn = dx-hat of the layer above"""
    eng, g, ws, T, es, Z2, dzs = cx.eng, cx.eng.g, cx.ws, cx.T, cx.es, cx.Z2, cx.dzs
    b0, nb, stc = part
    r = b0 * T * es
    srcs, w = [(ws["dskip"].data_ptr() + r * g.Sp, g.Sp, g.Sp, 0)], eng.w_bu.data_ptr() + l * eng.n_bu * es
    if gn.data_ptr() == ws["gzero"].data_ptr():
        # the top layer: dx-hat above it is zero (its x' is dead), so W_out^T . 0 is left out -- the skip half of the weight stream
        # on dS alone: the same sums (+ 0 exactly), half the chunks, 32 MB of zeros not read
        w += cx.us_off
    else:
        srcs.insert(0, (gn.data_ptr() + r * g.Rp, g.Rp, g.Rp, 0))
    _timed(eng, cx.sink("gate", stc), lambda: _tm(eng, nb, T, g.Hp, 2, 1.0, srcs, w, ws["dz"].data_ptr() + l * Z2 * es + r * dzs, dzs,
                                                  cx.fw["z"][l].data_ptr() + r * Z2, Z2, flags=flags, st=stc))


def _k_x(cx, l, gn, gc, part, flags=0):
    """dx-hat of layer l into gc, from dz_l and gn = dx-hat of the layer above"""
    eng, g, ws, B, T, es, Z2, dzs = cx.eng, cx.eng.g, cx.ws, cx.B, cx.T, cx.es, cx.Z2, cx.dzs
    b0, nb, stc = part
    r = b0 * T * es
    srcs = [(ws["dz"].data_ptr() + l * Z2 * es + r * dzs, dzs, Z2, (g.k - 1 - tap) * g.dilations[l]) for tap in range(g.k)]
    w = eng.w_bx.data_ptr() + l * eng.n_bx * es
    if cx.seeds is None:
        _timed(eng, cx.sink("res", stc), lambda: _tm(eng, nb, T, g.Rp, 1, RS, srcs, w, gc.data_ptr() + r * g.Rp, g.Rp,
                                                     gn.data_ptr() + r * g.Rp, g.Rp, flags=P.TM_INTERLEAVE | flags, st=stc))
    else:
        # dropout: the tap contraction alone (mode 0), then out = sqrt(.5) * (g_next + keep * acc / (1 - p)) with the mask
        # the forward applied to this layer's convolution operand
        _tm(eng, B, T, g.Rp, 0, 1.0, srcs, w, ws["gtmp"].data_ptr(), g.Rp, flags=P.TM_INTERLEAVE)
        L.check(eng.lib.wae_dropout_bwd(L.ptr(ws["gtmp"]), L.ptr(gn), L.ptr(gc), B * T * g.Rp, cx.seeds[l], eng.dropout, RS, eng.dt,
                                        eng.stream()), "dropout_bwd")


def _k_pair(cx, l, g_next, g_cur):
    """K_X of layer l and K_U of layer l-1 in one launch per chain (csrc/glu_bwd.hip); layer 0 (fold_dc): K_X + the last dc term only"""
    eng, g, ws, T, es, Z2, dzs = cx.eng, cx.eng.g, cx.ws, cx.T, cx.es, cx.Z2, cx.dzs
    lib, lp = eng.lib, max(l - 1, 0)
    cbytes = (Z2 // 64) * 8192                # bytes of one layer's chunks in the dc weight stream (packing.bwd_c_map)
    for b0, nb, stc in cx.parts:
        d = L.GluBwdDesc(eng.dt, nb, T, g.Rp, g.Hp, g.Sp, g.k, g.dilations[l], RS)
        r = b0 * T * es
        args = [ctypes.byref(d), ctypes.c_void_p(ws["dz"].data_ptr() + l * Z2 * es + r * dzs), dzs,
                ctypes.c_void_p(g_next.data_ptr() + r * g.Rp), ctypes.c_void_p(g_cur.data_ptr() + r * g.Rp),
                ctypes.c_void_p(ws["dskip"].data_ptr() + r * g.Sp), ctypes.c_void_p(cx.fw["z"][lp].data_ptr() + r * Z2),
                ctypes.c_void_p(ws["dz"].data_ptr() + lp * Z2 * es + r * dzs),
                ctypes.c_void_p((eng.w_bxf if eng.w_bxf is not None else eng.w_bx).data_ptr() + l * eng.n_bx * es),
                ctypes.c_void_p(eng.w_buo.data_ptr() + lp * eng.n_buo * es),
                ctypes.c_void_p(eng.w_bu.data_ptr() + lp * eng.n_bu * es + cx.us_off)]
        sq = stc if stc is not None else eng.stream()
        if cx.fold_dc:
            mode = (0 if l == g.layers - 1 else 1) | (2 if l == 0 else 0) | (4 if eng.bwd_pair4 else 0)
            # (bit 2: keep the 4-wave kernel where the 8-wave one, csrc/glu_bwd8.hip, has an instantiation -- tests and tools)
            args += [ctypes.c_void_p(eng.w_bc.data_ptr() + l * cbytes), ctypes.c_void_p(ws["dc32"].data_ptr() + b0 * T * 64 * 4),
                     ctypes.c_void_p(ws["dc"].data_ptr() + r * ws["dc"].shape[-1]), mode, int(l == 0)]
            _timed(eng, cx.sink("pair", stc), lambda: L.check(lib.wae_glu_bwd_fused_dc(*args, sq), "glu_bwd_fused_dc"))
        else:
            _timed(eng, cx.sink("pair", stc), lambda: L.check(lib.wae_glu_bwd_fused(*args, sq), "glu_bwd_fused"))


class TnSchedule(NamedTuple):
    """Where a step's weight-gradient launches go, decided once per (B, T) workspace and situation (_tn_schedule):
        "tiles":  one tile launch per layer inside the sweep (fp32, WAE_TN_STREAM=0)
        "whole":  `end` = every layer in one team launch behind the sweep
        "split":  data parallel -- `mid` = layers [cut, L) and the head leave the sweep at layer cut, so that their slice of the
                  gradient arena reaches the all-reduce in the middle of backward; `end` = layers [0, cut) behind the sweep
        "beside": an under-filled sweep -- `mid` = layers [cut, L) start at layer cut on a side stream, sized for the idle CUs,
                  `end` = layers [0, cut) behind the sweep"""
    kind: str
    cut: int          # the layer of the sweep behind which `mid` is launched; -1: nothing leaves the sweep
    mid: object
    end: object


def _tn_schedule(cx, sync):
    """The TnSchedule of this workspace for `sync` (a data-parallel step) and dropout; builds the tables it names on first use."""
    eng, g, ws, fw, B, T = cx.eng, cx.eng.g, cx.ws, cx.fw, cx.B, cx.T
    key = ("tn_schedule", sync, cx.seeds is not None)
    sched = ws.get(key)
    if sched is not None:
        return sched
    if ws["stream"] is None:
        sched = TnSchedule("tiles", -1, None, None)
    elif sync and g.layers >= 4 and eng.opt.dp_split:       # (WAE_DP_SPLIT=0: one hand-over at the end)
        cut = g.layers // 2
        if "stream_hi" not in ws:
            ws["stream_hi"] = _build_stream_table(eng, ws, fw, B, T, cut, g.layers)
            ws["stream_lo"] = _build_stream_table(eng, ws, fw, B, T, 0, cut)
        sched = TnSchedule("split", cut, ws["stream_hi"], ws["stream_lo"])
    else:
        sched = TnSchedule("whole", -1, None, ws["stream"])
        # ---- an UNDER-FILLED sweep (hps/vqwae.json's shard: 160 workgroups per launch on 256 CUs): the weight gradients of the upper
        #      layers (+ the head's) run BESIDE the lower part of the sweep, as a launch sized for the idle CUs on a side stream; the lower
        #      layers' follow the sweep as before.  Measured at that shard (20 layers, 96 idle CUs; ms per train step, one box): 6 / 8 /
        #      10 / 12 / 14 layers beside the sweep 3.247 / 3.226-3.239 / 3.223-3.230 / 3.230 / 3.287 against 3.37-3.39 without.  The
        #      side launch runs a layer's share in ~114 us on 96 CUs (all 256: 31 -- its teams no longer sit on one XCD each, and the
        #      sweep's launches share L2 and HBM with it) and slows the sweep's launches by ~5 % (the rule: packing.tn_beside_split)
        ncu = _ncu(eng)
        up = P.tn_beside_split(g.layers, B, T, ncu)
        if up is not None and not sync and eng.opt.side and isinstance(ws["stream"], StaticStreamTable) and cx.seeds is None:
            if "stream_beside" not in ws:
                ws["stream_beside"] = _build_stream_table(eng, ws, fw, B, T, up[0], g.layers, ncu=up[1])
                # with an encoder in front, the front end's backward is a chain of ~20 small launches (~0.3 ms) that starts at the end of
                # the sweep on its own side stream (engine.backward): the lower layers' launch leaves it 32 CUs instead of taking
                # every SIMD's registers (0 / 32 / 48 / 64 CUs left: 3.20-3.21 / 3.08-3.14 / 3.10 / 3.11 ms per step at hps/vqwae.json)
                ws["stream_below"] = _build_stream_table(eng, ws, fw, B, T, 0, up[0], ncu=(ncu - 32) if g.has_encoder else None)
            sched = TnSchedule("beside", up[0], ws["stream_beside"], ws["stream_below"])
    ws[key] = sched
    return sched


def _fork(cx):
    """The sweep's parts from here on: the whole batch, or (engine.chain_plan) two chains, the second started late on a side stream"""
    if cx.plan is None:
        return ((0, cx.B, None),)
    side = cx.eng.chain_fork(cx.plan[1])
    return ((0, cx.plan[0], None), (cx.plan[0], cx.B - cx.plan[0], ctypes.c_void_p(side.cuda_stream)))


def _leave_sweep(cx, work):
    """The one place where launches that read the sweep's results start before its end: whatever work() enqueues (on the current
    stream or on streams ordered behind it) reads rows of BOTH chains, so the chains are joined first and forked again behind it."""
    if cx.plan is not None:
        cx.eng.chain_join()
    work()
    cx.parts = _fork(cx)


def _hand_over(cx, grad_sync, lo, hi):
    """data parallel: the arena slice [lo, hi) is final -> its weight-norm backward (the gather pass of _finish_layers has done it
    already), and its all-reduce starts"""
    if cx.finish is None:
        _wn_bwd_range(cx.eng, lo, hi)
    grad_sync.ready_range(lo, hi)


def _tn_mid_sweep(cx, sched, grad_sync):
    """dz, dx-hat and the saved activations of layers [sched.cut, L) are complete: their weight gradients start"""
    eng = cx.eng
    if sched.kind == "beside":           # on the idle CUs
        with eng.branch(1) as cx.beside_done:
            _timed(eng, cx.tn_ev, sched.mid.launch)
    else:                                # split: the head's and theirs into the arena, and the all-reduce of ~half the arena starts
        _timed(eng, cx.tn_ev, sched.mid.launch)           # while the lower half of the sweep still runs
        done = _finish_layers(cx, sched.cut, eng.g.layers, with_head=True)
        eng.join(done[0] if done else None)
        _hand_over(cx, grad_sync, layer_segment_mid(eng), layer_segment(eng)[1])


def _sweep(cx, sched, grad_sync):
    """The gated stack below the top layer's K_U, last layer first; dx-hat of layer 0 lands in gx[0]"""
    eng, g, ws = cx.eng, cx.eng.g, cx.ws
    ngx = len(ws["gx"])
    fused = eng.fused_bwd and cx.seeds is None
    g_next = ws["gzero"]                      # dxhat_{L} = 0: the last layer's x' is dead (wavenet.py:205-207)
    cx.parts = _fork(cx)
    for l in range(g.layers - 1, -1, -1):
        assert l == g.layers - 1 or g_next.data_ptr() == ws["gx"][(l + 1) % ngx].data_ptr()
        if sched.kind == "tiles":              # needs dz_l and dx_{l+1}-hat
            _timed(eng, cx.tn_ev, lambda: ws["tt_layer"][l].launch(cx.B, cx.T))
        g_cur = ws["gx"][l % ngx]
        if fused and (l > 0 or cx.fold_dc):
            _k_pair(cx, l, g_next, g_cur)
        else:
            for part in cx.parts:
                _k_x(cx, l, g_next, g_cur, part)
                if l > 0:
                    _k_u(cx, l - 1, g_cur, part)
        g_next = g_cur
        if l == sched.cut:
            _leave_sweep(cx, lambda: _tn_mid_sweep(cx, sched, grad_sync))
    if cx.plan is not None:
        eng.chain_join()
    assert g_next.data_ptr() == ws["gx"][0].data_ptr()


def _scatter_specs(cx, l0, l1, with_head):
    """What _finish_layers(l0, l1, with_head) moves from the weight-gradient tiles into the arena, one record per block:
    (tile buffer, map, rows, cols, ld, off, nb, ss, ds, unique, doff) -- names of eng.cview / eng.sm and the fields of wae_scatter_job
    (nb batch entries = layers, `ss` tile floats and `ds` arena floats apart, the first at tile float `off` and arena float `doff`)."""
    eng, g, sm, Z2 = cx.eng, cx.eng.g, cx.eng.sm, cx.Z2
    OP = P.ONES_PAD
    nb, ls = l1 - l0, eng.lay.layer_stride

    def spec(src, mp, rows, cols, ld, off=0, nb=1, ss=0, ds=0, unique=1, doff=0):
        return (src, mp, rows, cols, ld, off, nb, ss, ds, unique, doff)
    per = dict(nb=nb, ds=ls, doff=l0 * ls)     # one block per layer of the range
    static = isinstance(cx.ws["stream"], StaticStreamTable)
    lst = [spec("c1", "w1", Z2, sm["ncol1"], sm["ld1"], off=l0 * Z2 * sm["ld1"], ss=Z2 * sm["ld1"], **per)]
    if static:      # transposed dW_out (+ its bias row) and dW_skip blocks of the static stream launch, per layer
        rows = sm["ldoT_rows"]
        lst += [spec("coT", "woT", g.Hp, g.Rp, g.Rp, off=l0 * rows * g.Rp, ss=rows * g.Rp, **per),
                spec("coT", "boT", 1, g.Rp, g.Rp, off=l0 * rows * g.Rp + g.Hp * g.Rp, ss=rows * g.Rp, **per),
                spec("csT", "wsT", g.Hp, g.Sp, g.Sp, off=l0 * g.Hp * g.Sp, ss=g.Hp * g.Sp, **per),
                spec("cbs", "bsT", 1, g.Sp, g.Sp, ss=0, **per)]
    else:
        lst += [spec("co", "wo", g.Rp, g.Hp, sm["ldo"], off=l0 * g.Rp * sm["ldo"], ss=g.Rp * sm["ldo"], **per),
                spec("co", "bo", g.Rp, OP, sm["ldo"], off=l0 * g.Rp * sm["ldo"] + g.Hp, ss=g.Rp * sm["ldo"], unique=2, **per),
                spec("cs", "bs", g.Sp, OP, sm["lds"], off=g.Ku, ss=0, unique=2, **per)]
    if with_head:
        if not static:
            lst.append(spec("cs", "ws", g.Sp, g.Ku, sm["lds"]))
        lst += [spec("c3", "w3", g.Op, g.Sp, sm["ldh"]),
                spec("c3", "b3", g.Op, OP, sm["ldh"], off=g.Sp, unique=2),
                spec("c1h", "w1h", g.Sp, g.Sp, sm["ldh"]),
                spec("c1h", "b1h", g.Sp, OP, sm["ldh"], off=g.Sp, unique=2)]
    return lst


def _scatter_jobs(cx, l0, l1, with_head, which="all"):
    """The wae_scatter_job array of _finish_layers(l0, l1, with_head): built once per workspace and range.  which = "rowsum": the bias
    sums (unique == 2) alone -- what the gather pass (_finish_plan) leaves to the scatter; "tiles": the others; None if there are none."""
    eng = cx.eng
    lst = [L.ScatterJob(eng.cview[src].data_ptr() + off * 4, eng.sm[mp].data_ptr(), eng.d_eff.data_ptr() + doff * 4, rows * cols, ss, ds,
                        ld, nb, cols, unique, 0)
           for src, mp, rows, cols, ld, off, nb, ss, ds, unique, doff in _scatter_specs(cx, l0, l1, with_head)
           if which == "all" or (unique == 2) == (which == "rowsum")]
    return (L.ScatterJob * len(lst))(*lst) if lst else None


_FINISH_ROW = np.dtype([("off", "<i8"), ("g_off", "<i8"), ("base", "<i8"), ("cols", "<i4"), ("pat", "<i4")])    # wae_finish_row
_FINISH_PLAIN = 64         # floats of a plain parameter per row of the table: one trip of its 16-lane group, four loads per lane


class FinishPlan(NamedTuple):
    """The row tables of wae_grad_finish over backward.layer_segment (csrc/grad_finish.hip), built once per engine:
    `tile` = the rows whose dW the kernel gathers from the weight-gradient tiles (the inverse of the `unique == 1` scatter jobs),
    `rest` = the rows other kernels leave in d_eff (gproj_bwd: conv1x1g and the conv bias; the row-sum scatter: bias sums).
    Both sorted by arena offset (`*_off`, host), so an arena range is a row range.  `outer` = the rows of the arena outside the segment
    (first conv, speaker embedding, upsampling network, encoder, codebook: all from d_eff), finished in one launch by finish_grads."""
    tile: torch.Tensor
    tile_off: np.ndarray
    rest: torch.Tensor
    rest_off: np.ndarray
    pats: torch.Tensor
    outer: torch.Tensor
    outer_off: np.ndarray


def _finish_recs(lay, lo, hi, inv=None):
    """(off, g_off, cols) of the rows of wae_grad_finish that cover the arena range [lo, hi), sorted: its weight-normed rows, and what
    lies between them except the g scalars (the rows write those) in pieces of at most _FINISH_PLAIN -- cut, with `inv` (slot - lo ->
    tile float or -1), where the kind of source changes"""
    r0, r1 = int(np.searchsorted(lay.wn_v_off, lo)), int(np.searchsorted(lay.wn_v_off, hi))
    voff, goff, vcols = (np.asarray(a[r0:r1], dtype=np.int64) for a in (lay.wn_v_off, lay.wn_g_off, lay.wn_cols))
    edge = np.zeros(hi - lo + 1, dtype=np.int32)
    np.add.at(edge, voff - lo, 1)
    np.add.at(edge, voff - lo + vcols, -1)
    covered = np.cumsum(edge[:-1]) > 0
    gall = np.asarray(lay.wn_g_off, dtype=np.int64)
    covered[gall[(gall >= lo) & (gall < hi)] - lo] = True
    plain = np.flatnonzero(~covered)
    recs = [(int(o), int(go), int(c)) for o, go, c in zip(voff, goff, vcols)]
    if plain.size:
        brk = np.diff(plain) != 1
        if inv is not None:
            brk |= np.diff(inv[plain] >= 0) != 0
        cut = np.flatnonzero(brk) + 1
        for a, b in zip(np.concatenate(([0], cut)), np.concatenate((cut, [plain.size]))):
            for p0 in range(int(plain[a]), int(plain[b - 1]) + 1, _FINISH_PLAIN):
                recs.append((p0 + lo, -1, min(_FINISH_PLAIN, int(plain[b - 1]) + 1 - p0)))
    recs.sort()
    return recs


def _build_finish_plan(cx):
    """FinishPlan of this engine and kind of weight-gradient launch, or None where the gather pass has no form for the tiles: a slot
    fed by more than one tile element, or a row only partly covered by tiles (the split launches stay in charge then)."""
    eng, g, lay = cx.eng, cx.eng.g, cx.eng.lay
    lo, hi = layer_segment(eng)
    hm = P.grad_scatter_maps(g, lay)
    base0 = eng.cbuf.data_ptr()
    inv = np.full(hi - lo, -1, dtype=np.int64)          # arena slot of the segment -> float of eng.cbuf
    for src, mp, rows, cols, ld, off, nb, ss, ds, unique, doff in _scatter_specs(cx, 0, g.layers, True):
        if unique != 1:
            continue
        m = np.asarray(hm[mp], dtype=np.int64).reshape(-1)[:rows * cols]
        i = np.arange(rows * cols, dtype=np.int64)
        ok = m >= 0
        si = ((i // cols) * ld + i % cols)[ok] + off + (eng.cview[src].data_ptr() - base0) // 4
        m = m[ok] + doff - lo
        for b in range(nb):
            d = m + b * ds
            if d.size == 0:
                continue
            if d.min() < 0 or d.max() >= hi - lo or np.unique(d).size != d.size or (inv[d] >= 0).any():
                return None
            inv[d] = si + b * ss
    if inv.max() >= eng.cbuf.numel():
        return None
    recs = _finish_recs(lay, lo, hi, inv)
    pats, pat_at, pool, tile, rest = {}, 0, [], [], []
    for off, go, c in recs:
        sl = inv[off - lo:off - lo + c]
        if (sl < 0).all():
            rest.append((off, go, 0, c, -1))
            continue
        if (sl < 0).any():
            return None
        b0 = int(sl.min())
        rel = (sl - b0).astype(np.int32)
        key = rel.tobytes()
        at = pats.get(key)
        if at is None:
            at = pats[key] = pat_at
            pool.append(np.concatenate((rel, np.zeros(-c % 4, dtype=np.int32))))        # (16-byte aligned patterns)
            pat_at += pool[-1].size
        tile.append((off, go, b0, c, at))
    if not tile:
        return None

    def up(rows):
        a = np.array(rows, dtype=_FINISH_ROW) if rows else np.zeros(0, dtype=_FINISH_ROW)
        t = torch.from_numpy(a.view(np.uint8).copy()).to(eng.device) if rows else torch.zeros(32, dtype=torch.uint8, device=eng.device)
        return t, a["off"].copy()
    t_tile, o_tile = up(tile)
    t_rest, o_rest = up(rest)
    outer = [(off, go, 0, c, -1) for a, b in ((0, lo), (hi, lay.total)) if b > a for off, go, c in _finish_recs(lay, a, b)]
    t_outer, o_outer = up(outer)
    return FinishPlan(t_tile, o_tile, t_rest, o_rest, torch.from_numpy(np.concatenate(pool)).to(eng.device), t_outer, o_outer)


def _finish_plan(cx):
    """The FinishPlan that serves this step, or None: the split launches (EngineOptions.grad_finish off, or no form: _build_finish_plan)"""
    eng = cx.eng
    if not eng.opt.grad_finish:
        return None
    static = isinstance(cx.ws["stream"], StaticStreamTable)
    plans = eng._finish_plans
    if static not in plans:
        plans[static] = _build_finish_plan(cx)
    return plans[static]


def _finish_rows(eng, plan, lo, hi, which, acc):
    """wae_grad_finish over the rows of plan.tile / plan.rest (`which`) that start in the arena range [lo, hi); acc: their squares are
    added to eng.gn_acc"""
    rows, offs = {"tile": (plan.tile, plan.tile_off), "rest": (plan.rest, plan.rest_off), "outer": (plan.outer, plan.outer_off)}[which]
    r0, r1 = int(np.searchsorted(offs, lo)), int(np.searchsorted(offs, hi))
    if r1 > r0:
        L.check(eng.lib.wae_grad_finish(L.ptr(eng.params), L.ptr(eng.cbuf), L.ptr(plan.pats), L.ptr(eng.d_eff), L.ptr(eng.grads),
                                        L.ptr(rows), r0, r1, L.ptr(eng.gn_acc) if acc else None, eng.stream()), "grad_finish")


def _gproj_bwd(cx, l0, l1, consume=False):
    """the zb chain (conv bias + hoisted global conditioning, modules.py:148-152) of layers [l0, l1) into d_eff; consume (a
    micro-batch of an accumulation window): the entry that zeroes the per-clip columns it has read (csrc/accum.hip)"""
    eng, g, lay, sm = cx.eng, cx.eng.g, cx.eng.lay, cx.eng.sm
    wg_off = lay.off("wavenet.conv_layers.0.conv1x1g.weight_v") + l0 * lay.layer_stride if g.Cg > 0 else -1
    args = (L.ptr(eng.eff), L.ptr(eng.d_eff), wg_off, lay.off("wavenet.conv_layers.0.conv.bias") + l0 * lay.layer_stride,
            lay.layer_stride, L.ptr(cx.gid32) if cx.use_gid else None, lay.offsets.get("wavenet.embed_speakers.weight", 0),
            L.ptr(cx.gvec), ctypes.c_void_p(eng.cview["c1"].data_ptr() + l0 * cx.Z2 * sm["ld1"] * 4),
            cx.Z2 * sm["ld1"], sm["ld1"], g.k * g.Rp + g.Ccp, cx.B, l1 - l0, g.G, g.Hp, max(g.Cg, 0), int(g.n_speakers or 0))
    if eng.opt.deterministic:      # the embedding rows from partials in a fixed order (csrc/accum.hip)
        parts = eng.det_buffer("gproj", int(eng.lib.wae_gproj_bwd_det_floats(cx.B, l1 - l0, g.Hp, max(g.Cg, 0))))
        L.check(eng.lib.wae_gproj_bwd_det(*args, int(consume), L.ptr(parts), parts.numel(), eng.stream()), "gproj_bwd_det")
        return
    entry = eng.lib.wae_gproj_bwd_consume if consume else eng.lib.wae_gproj_bwd
    L.check(entry(*args, eng.stream()), "gproj_bwd_consume" if consume else "gproj_bwd")


def _finish_layers(cx, l0, l1, with_head, zb=True):
    """The weight gradients of layers [l0, l1) (and of the head) leave the dense tiles.  Split launches: scattered into the
    effective-weight arena d_eff, then the zb chain of those layers; disjoint slots, the tables never move -- the weight-norm
    backward and the norm follow in launches of their own (_hand_over, finish_grads, wae_clip_adam_ema).
    Gather pass (cx.finish, csrc/grad_finish.hip): ONE launch takes them from the tiles to eng.grads and sums their squares; the bias
    sums, the zb chain and the finish of the few rows those two produce run beside it on a side stream (each far too small to fill the
    machine, and none of them reads what the gather pass writes).  Returns that side work's completion event (a list, engine.branch)
    or None.  d_eff keeps zeros in the slots the gather pass serves: nothing reads them.
    zb=False (the close of an accumulation window): the zb chain has run, consuming, behind every micro-batch."""
    eng, ws, st = cx.eng, cx.ws, cx.eng.stream()
    plan = cx.finish
    key = ("scatter_jobs", l0, l1, with_head, plan is not None)
    if key not in ws:
        ws[key] = _scatter_jobs(cx, l0, l1, with_head, which="all" if plan is None else "rowsum")
    jobs = ws[key]
    if plan is None:
        L.check(eng.lib.wae_unpack_scatter_add_multi(jobs, len(jobs), st), "scatter layer and head gradients")
        if zb:
            _gproj_bwd(cx, l0, l1)
        return None
    ls, seg = eng.lay.layer_stride, layer_segment(eng)
    lo, hi = seg[0] + l0 * ls, (seg[1] if with_head else seg[0] + l1 * ls)

    def small():
        if jobs is not None:
            L.check(eng.lib.wae_unpack_scatter_add_multi(jobs, len(jobs), eng.stream()), "bias sums of the layer and head gradients")
        if zb:
            _gproj_bwd(cx, l0, l1)
        _finish_rows(eng, plan, lo, hi, "rest", cx.finish_acc)
    if not eng.opt.side:
        small()
        _finish_rows(eng, plan, lo, hi, "tile", cx.finish_acc)
        return None
    with eng.branch(1) as done:
        small()
    _finish_rows(eng, plan, lo, hi, "tile", cx.finish_acc)
    return done


def _tn_behind_sweep(cx, sched, grad_sync):
    """The weight-gradient launch behind the sweep (every layer's dW1 taps, dWc + zb sums, dW_out + bias in one launch, or the lower
    layers' when the upper ones' left the sweep: TnSchedule), the scatter into the arena, and the data-parallel hand-over."""
    eng = cx.eng
    if sched.end is not None:
        _timed(eng, cx.tn_ev, sched.end.launch)
    if sched.kind == "beside":           # (the upper layers' launch has been running beside the sweep)
        eng.join(cx.beside_done[0])
    fl = eng.flight
    fl.grads_done = None
    if fl.accum is not None:
        # a micro-batch of an accumulation window: the tiles keep adding up until finish_window -- nothing is scattered and nothing
        # reaches eng.grads.  The zb chain alone is per micro-batch (its columns are per clip, under this batch's speaker ids)
        _gproj_bwd(cx, 0, eng.g.layers, consume=True)
        return
    if sched.kind == "split":
        done = _finish_layers(cx, 0, sched.cut, with_head=False)
        eng.join(done[0] if done else None)
        seg = layer_segment(eng)
        fl.grads_done = seg
        _hand_over(cx, grad_sync, seg[0], layer_segment_mid(eng))
        return
    done = _finish_layers(cx, 0, eng.g.layers, with_head=True)
    if grad_sync is None:
        cx.small_done = done
        if cx.finish is not None:      # finish_grads has the rest of the arena left (and, with finish_acc, the rest of the norm)
            fl.grads_done = layer_segment(eng)
            fl.norm_summed = cx.finish_acc
    else:
        eng.join(done[0] if done else None)
        # data parallel without the split (too few layers, or the per-layer tile launches of fp32): the layers' + head's gradients
        # are final -> weight-norm backward of that slice, then the all-reduce starts on its side stream while the launches below
        # (and the front end's backward) still run
        seg = layer_segment(eng)
        fl.grads_done = seg
        _hand_over(cx, grad_sync, *seg)


def head_dy_factor(eng, B, T, lengths, loss_scale=1.0, dy_factor=None):
    """The factor on d loss / d logits of a (B, T) batch's masked cross-entropy: dy_factor where given (a window's micro-batch), else
    loss_scale * grad_scale / count over the shifted steps inside `lengths` (None: all).  ONE expression for train.step_run, which
    announces it to the forward's fused head, and decoder_backward, which skips wae_head_bwd where the two agree."""
    if dy_factor is not None:
        return dy_factor
    if lengths is None:
        count = B * (T - 1)
    else:
        count = int(torch.clamp(lengths.detach().to("cpu", torch.int64).clamp(max=T) - 1, min=0).sum())
    return loss_scale * eng.grad_scale / max(count, 1)


def head_fused_ok(eng) -> bool:
    """Does this engine have the one-launch training head (csrc/head_train.hip)?  16-bit split heads with Sp == Op."""
    g = eng.g
    return bool(eng.opt.head_fused and eng.split_head and not eng.wide_head and not g.scalar_input
                and eng.lib.wae_head_train_supported(eng.dt, g.Sp, g.Op))


def early_onehot(eng, x):
    """The first conv's one-hot operand depends on the ids alone: train.step_open writes it behind the backward's weight packing on
    that launch's side stream (decoder_backward waits for both at once) where the fused head has taken the launches around it off the
    main stream.  ws: the (B, T) backward workspace, made by the caller on the main stream."""
    B, T = x.shape
    ws = eng._ws.get(("bwd", B, T))
    if ws is None or ws["onehot"] is None:
        return
    L.check(eng.lib.wae_onehot_rows(L.ptr(x), L.ptr(ws["onehot"]), B * T, ws["onehot"].shape[-1], eng.dt, eng.stream()), "onehot_rows")
    eng.flight.onehot_early = (x.data_ptr(), B, T)
    eng.hold("onehot_early", x)


def _head_backward(cx, xi, tg, ln, inv_count, ext_dy, done=False):
    """dy, dh1, dskip (done: the forward's fused head launch wrote them); the head's tile launch and the first conv's one-hot operand
    where the static launch does not carry them"""
    eng, g, lib, ws, fw, B, T, st = cx.eng, cx.eng.g, cx.eng.lib, cx.ws, cx.fw, cx.B, cx.T, cx.eng.stream()
    b3 = ctypes.c_void_p(eng.b_head.data_ptr() + 2 * g.Sp * 4)
    if eng.wide_head:
        # the same three steps as csrc/head_bwd.hip, one wae_gemm_tm launch each (dy, dh1, dskip through HBM)
        if ext_dy is not None:
            ws["dy"].copy_(ext_dy)
        else:
            ce = L.TmCe(None, tg.data_ptr(), None, fw["lse"].data_ptr(), ln.data_ptr() if ln is not None else None, inv_count, g.O)
            _tm_ce(eng, B, T, g.Op, 6, [(fw["h1"].data_ptr(), g.Sp, g.Sp, 0)], eng.w_hwide["w3"].data_ptr(), ws["dy"].data_ptr(),
                   g.Op, b3.value, ce)
        _tm(eng, B, T, g.Sp, 4, 1.0, [(ws["dy"].data_ptr(), g.Op, g.Op, 0)], eng.w_hwide["w3t"].data_ptr(), ws["dh1"].data_ptr(),
            g.Sp, fw["h1"].data_ptr(), g.Sp)
        _tm(eng, B, T, g.Sp, 4, math.sqrt(1.0 / g.layers), [(ws["dh1"].data_ptr(), g.Sp, g.Sp, 0)], eng.w_hwide["w1t"].data_ptr(),
            ws["dskip"].data_ptr(), g.Sp, fw["h0"].data_ptr(), g.Sp)
    elif not done:
        hd = L.HeadDesc(eng.dt, B, T, g.Ku, g.Sp, g.Op, g.O, math.sqrt(1.0 / g.layers))
        L.check(lib.wae_head_bwd(ctypes.byref(hd), L.ptr(fw["h0"]), L.ptr(fw["h1"]), L.ptr(eng.w_hb), b3, L.ptr(fw["lse"]), L.ptr(tg),
                                 L.ptr(ln), inv_count, L.ptr(ext_dy), L.ptr(ws["dy"]), L.ptr(ws["dh1"]), L.ptr(ws["dskip"]), st),
                "head_bwd")
        if ext_dy is not None:
            ws["dy"].copy_(ext_dy)                # the tile table points at ws["dy"]
    if ws["tt_head"] is not None:
        ws["tt_head"].launch(B, T)
    early, eng.flight.onehot_early = eng.flight.onehot_early, None
    if ws["onehot"] is not None and early != (xi.data_ptr(), B, T):        # operand of the first conv's weight gradient (a job of the stream launch)
        L.check(lib.wae_onehot_rows(L.ptr(xi), L.ptr(ws["onehot"]), B * T, ws["onehot"].shape[-1], eng.dt, st), "onehot_rows")


def _first_conv_grads(cx, x_ids, xi, tile_only=False):
    """dW[r][class] = sum_t dx0[t][r] onehot(id[t])[class];  dx0 = dxhat_0 / sqrt(.5).  tile_only (a micro-batch of an accumulation
    window): the contraction into the tile alone; _first_conv_finish takes the tile to d_eff once, when the window closes."""
    eng, g, ws, B, T = cx.eng, cx.eng.g, cx.ws, cx.B, cx.T
    if g.scalar_input:
        ws["xs1"][:, :, 0] = x_ids.to(ws["xs1"].dtype)
        ws["xs1"][:, :, 1] = 1.0
        ws["tt_first"].launch(B, T)
    elif ws["tt_first"] is not None:
        ws["ids"].copy_(xi)
        ws["tt_first"].launch(B, T)
    if not tile_only:
        _first_conv_finish(cx)


def _first_conv_finish(cx):
    """the first conv's tile -> its bias gradient and both into d_eff"""
    eng, g, lib, ws, sm, st = cx.eng, cx.eng.g, cx.eng.lib, cx.ws, cx.eng.sm, cx.eng.stream()
    ctab, fb = eng.cview["ctab"], eng.cview["fb"]
    if g.scalar_input:
        fb.copy_(ctab[g.Rp:2 * g.Rp])            # row 1: bias gradient; row 0 (weight) is scattered below
    else:
        L.check(lib.wae_sum_rows(L.ptr(ctab), 0, g.Rp, g.O, g.Rp, g.Rp, L.ptr(fb), st), "first bias grad")
    jobs = ws.get("scatter_jobs_first")
    if jobs is None:
        def sjob(src, mp, rows, cols, ld):
            return L.ScatterJob(src.data_ptr(), mp.data_ptr(), eng.d_eff.data_ptr(), rows * cols, 0, 0, ld, 1, cols, 1, 0)
        lst = [sjob(ctab, sm["tab"], 1 if g.scalar_input else g.O, g.Rp, g.Rp), sjob(fb, sm["fb"], 1, g.Rp, g.Rp)]
        jobs = ws["scatter_jobs_first"] = (L.ScatterJob * len(lst))(*lst)
    L.check(lib.wae_unpack_scatter_add_multi(jobs, len(jobs), st), "scatter first-conv gradients")


def decoder_backward(eng, x_ids: torch.Tensor, targets: torch.Tensor, lengths: Optional[torch.Tensor],
                     gid: Optional[torch.Tensor], gvec: Optional[torch.Tensor] = None, ext_dy: Optional[torch.Tensor] = None,
                     loss_scale: float = 1.0, grad_sync=None, dy_factor: Optional[float] = None):
    """Backward of the last ``decoder_forward(..., train=True)`` with the same (B, T).  Fills ``eng.grads`` (flat arena,
    reference parameter layout incl. weight_g / weight_v) for every decoder parameter and returns dc (B,T,Ccp): the
    gradient wrt the upsampled local conditioning.  ``ext_dy`` (B,T,Op): external d loss / d logits (DMoL).
    ``grad_sync`` (distributed.GradSync): the layers' + head's slice of the gradient arena is finished (weight-norm backward
    of that slice) and handed to the all-reduce BEFORE the conditioning / first-conv / front-end gradients are computed, so
    the collective runs under them.
    ``dy_factor``: the factor on d loss / d logits, in place of loss_scale * grad_scale / count (a window's micro-batch: grad_scale over
    the WINDOW's count, formed once).
    Deferred finishing (``eng.flight.accum``, a step_state.Window): this backward is a micro-batch of an accumulation window.  The first
    one packs the backward's weights and clears the accumulators as a plain step does; from the second on that launch is skipped
    altogether (the weights, and so their packings, are the window's).  The sweep, the weight-gradient launches (`beside` included), the
    zb chain -- which consumes its per-clip columns -- and the first conv's contraction run as now; nothing is scattered from the tiles,
    eng.grads and the norm's accumulator are not touched.  finish_window does all that once."""
    B, T = x_ids.shape
    sv = saved_for(eng, B, T)
    _prepare_bwd(eng)
    g = eng.g
    win = eng.flight.accum
    if win is not None and grad_sync is not None:
        raise ValueError("a micro-batch of an accumulation window takes no grad_sync: the arena goes out once, in apply_step")
    bwd_workspace(eng, B, T)
    if win is None or win.n == 0:
        _await_packed_weights(eng)
    cx = _step(eng, B, T, sv.drop_seeds)
    ws = cx.ws
    factor = head_dy_factor(eng, B, T, lengths, loss_scale, dy_factor)
    xi = x_ids.to(torch.int32).contiguous() if not g.scalar_input else None
    tg = targets.to(torch.int32).contiguous() if targets is not None else None
    ln = lengths.to(torch.int32).to(eng.device).contiguous() if lengths is not None else None
    # (the forward's fused head ran the head's backward with the factor train.step_run announced: nothing to launch where it is this one)
    done = ext_dy is None and sv.head_done is not None and sv.head_done.serves(factor, targets, lengths)
    _head_backward(cx, xi, tg, ln, factor, ext_dy, done)
    cx.use_gid = gid is not None and "wavenet.embed_speakers.weight" in eng.lay.offsets
    cx.gid32 = gid.to(torch.int32).contiguous() if gid is not None else None
    cx.gvec = gvec
    sched = _tn_schedule(cx, grad_sync is not None)
    cx.finish = eng.flight.finish_used = _finish_plan(cx)
    cx.finish_acc = cx.finish is not None and grad_sync is None and not eng.opt.deterministic      # (its norm: train.clip_adam_ema)
    eng.flight.norm_summed = False
    if win is not None:
        win.static, win.shape = isinstance(ws["stream"], StaticStreamTable), (B, T)
    if cx.fold_dc and "dc32" not in ws:
        ws["dc32"] = torch.empty(B, T, 64, dtype=torch.float32, device=eng.device)
    eng.flight.grads_done = None
    # ---- gated stack, last layer first ---------------------------------------------------------------------------
    _k_u(cx, g.layers - 1, ws["gzero"], cx.parts[0])
    # two half-batch chains of the sweep's launches (engine.chain_plan), the second half a launch late; not with dropout (its mask
    # generator counts elements of the full batch) and not with per-layer weight-gradient launches (they read both chains' rows)
    cx.plan = eng.chain_plan(B, T, backward=True) if (cx.seeds is None and sched.kind != "tiles") else None
    _timed(eng, cx.sink("sweep"), lambda: _sweep(cx, sched, grad_sync))   # (bench.py: HIP events around both chains)
    if cx.fold_dc and eng.opt.side:
        # dc is complete: the front end's backward may start (engine.backward: a side stream).  Its launches then sit behind the
        # weight-gradient launch below, which fills every SIMD's registers, and run in that launch's ragged end (its workgroups finish
        # 60-90 us apart) and beside the scatters.  (Started behind the weight-gradient launch instead they ran beside the scatters
        # only, and both took longer: 54 us per step gained instead of 90.)
        eng.flight.ev_dc = torch.cuda.Event()
        eng.flight.ev_dc.record(torch.cuda.current_stream(eng.device))
    _tn_behind_sweep(cx, sched, grad_sync)
    # ---- local-conditioning gradient over all layers at once ---------------------------------------------------------
    if g.Ccp and not cx.fold_dc:
        _tm(eng, B, T, g.Ccp, 0, 1.0, [(ws["dz"].data_ptr(), cx.dzs, cx.dzs, 0)], eng.w_bc.data_ptr(), ws["dc"].data_ptr(), g.Ccp)
    _first_conv_grads(cx, x_ids, xi, tile_only=win is not None)          # (behind the gather pass, while the side stream's chain of small launches runs)
    eng.join(cx.small_done[0] if cx.small_done else None)
    eng.hold("bwd", xi, tg, ln, cx.gid32)
    return ws["dc"]


def layer_backward(eng, B, T, gx_hat, ds, gvec, lead=0):
    """Backward of ONE ResidualConv1dGLU layer (an engine of geometry layers == 1, wavenet_vocoder.modules.ResidualConv1dGLU) -- the
    autograd of modules.py:115-163 from the same kernels the stack uses, last train-mode forward of that (B, T):
        dz  = gate'(z) * (W_out^T gx_hat + W_skip^T ds)                   (wae_gemm_tm GATE_BWD)
        dx  = gx_hat + sum_tap W1_tap^T dz[t + (k-1-tap) d]               (wae_gemm_tm RESIDUAL, alpha 1: the true gradient)
        dc  = Wc^T dz                                                     (wae_gemm_tm PLAIN)
        dW1, dWc, per-clip sums of dz, dW_out + bias, dW_skip + bias      (wae_gemm_tn_tiles), gproj / weight-norm backward
    gx_hat (B,T,Rp) = sqrt(.5) * d loss / d x' (x' = (conv1x1_out(u) + x) sqrt(.5)), ds (B,T,Sp) = d loss / d s, both in the engine's
    storage dtype (times eng.grad_scale for fp16).  The dropout mask the forward applied to the convolution's operand (modules.py:127-128)
    is regenerated from the seed in eng.saved.  lead > 0: a causal=False layer run on a frame `lead` steps longer (modules.ResidualConv1dGLU):
    the convolution operand's rows [0, T - lead) are x, the residual operand's rows [lead, T) are x, so the residual path's gradient of
    x[t] is gx_hat[t + lead] (gx_hat must own `lead` readable rows behind its end) and dx is returned in the convolution operand's frame.
    Fills eng.grads (finish_grads) and returns (dx (B,T,Rp), dc (B,T,Ccp) | None)."""
    sv = saved_for(eng, B, T)
    drop_seed = sv.drop_seeds[0] if sv.drop_seeds else None
    _prepare_bwd(eng)
    g, lib, lay, st, sm = eng.g, eng.lib, eng.lay, eng.stream(), eng.sm
    assert g.layers == 1
    fw = eng._ws[(B, T, True)]
    Z2 = 2 * g.Hp
    key = ("lbwd", B, T)
    ws = eng._ws.get(key)
    ia = 1.0 / eng.grad_scale
    c1, co, cs = eng.cview["c1"], eng.cview["co"], eng.cview["cs"]
    if ws is None:
        dev, td = eng.device, eng.tdtype
        ws = dict(dz=torch.zeros(B, T, Z2, dtype=td, device=dev), gx=torch.zeros(B, T, g.Rp, dtype=td, device=dev),
                  gn=torch.zeros(B * T + lead, g.Rp, dtype=td, device=dev)[:B * T].view(B, T, g.Rp),
                  dskip=torch.zeros(B, T, g.Sp, dtype=td, device=dev),
                  dc=torch.zeros(B, T, max(g.Ccp, 64), dtype=td, device=dev))
        tt = TileTable(eng)
        # dW1 contracts dz against the convolution's operand: the masked one, the non-causal layer's [x ; 0], or x itself
        xop = fw["xd"][0] if "xd" in fw else (fw["xnc"] if lead else fw["x"][0])
        for rec in P.tn_layer_contractions(g, g.dilations[0], ia, ws["dz"].data_ptr(), Z2, xop.data_ptr(),
                                           fw["c_up"].data_ptr() if g.Ccp else 0, ws["gn"].data_ptr(), fw["u"].data_ptr(),
                                           c1.data_ptr(), sm["ld1"], co.data_ptr(), sm["ldo"]):
            tt.add(*rec)
        tt.add(g.Sp, g.Ku, 0, g.Ku, ia, ws["dskip"].data_ptr(), g.Sp, fw["u"].data_ptr(), g.Ku, cs.data_ptr(), sm["lds"])
        ws["tt"] = tt.finalize(B)
        eng._ws[key] = ws
    ws["gn"].copy_(gx_hat)
    ws["dskip"].copy_(ds)
    _await_packed_weights(eng)
    _tm(eng, B, T, g.Hp, 2, 1.0, [(ws["gn"].data_ptr(), g.Rp, g.Rp, 0), (ws["dskip"].data_ptr(), g.Sp, g.Sp, 0)], eng.w_bu.data_ptr(),
        ws["dz"].data_ptr(), Z2, fw["z"][0].data_ptr(), Z2)
    ws["tt"].launch(B, T)
    srcs = [(ws["dz"].data_ptr(), Z2, Z2, (g.k - 1 - tap) * g.dilations[0]) for tap in range(g.k)]
    if drop_seed is None and not lead:
        _tm(eng, B, T, g.Rp, 1, 1.0, srcs, eng.w_bx.data_ptr(), ws["gx"].data_ptr(), g.Rp, ws["gn"].data_ptr(), g.Rp,
            flags=P.TM_INTERLEAVE)
    else:
        # dropout and / or the non-causal frame: the tap contraction alone, then dx[t] = gx_hat[t + lead] + keep * acc[t] / (1 - p) with
        # the forward's mask (no dropout: p = 0 keeps everything)
        if "gtmp" not in ws:
            ws["gtmp"] = torch.zeros(B, T, g.Rp, dtype=eng.tdtype, device=eng.device)
        _tm(eng, B, T, g.Rp, 0, 1.0, srcs, eng.w_bx.data_ptr(), ws["gtmp"].data_ptr(), g.Rp, flags=P.TM_INTERLEAVE)
        gn_late = ctypes.c_void_p(ws["gn"].data_ptr() + lead * g.Rp * ws["gn"].element_size())
        L.check(lib.wae_dropout_bwd(L.ptr(ws["gtmp"]), gn_late, L.ptr(ws["gx"]), B * T * g.Rp, drop_seed or 0,
                                    eng.dropout if drop_seed is not None else 0.0, 1.0, eng.dt, st), "dropout_bwd")
    if g.Ccp:
        _tm(eng, B, T, g.Ccp, 0, 1.0, [(ws["dz"].data_ptr(), Z2, Z2, 0)], eng.w_bc.data_ptr(), ws["dc"].data_ptr(), g.Ccp)
    OP = P.ONES_PAD
    jobs = ws.get("scatter")
    if jobs is None:
        def sjob(src, mp, rows, cols, ld, off=0, unique=1):
            return L.ScatterJob(src.data_ptr() + off * 4, mp.data_ptr(), eng.d_eff.data_ptr(), rows * cols, 0, 0, ld, 1, cols, unique, 0)
        lst = [sjob(c1, sm["w1"], Z2, sm["ncol1"], sm["ld1"]), sjob(co, sm["wo"], g.Rp, g.Hp, sm["ldo"]),
               sjob(co, sm["bo"], g.Rp, OP, sm["ldo"], off=g.Hp, unique=2), sjob(cs, sm["ws"], g.Sp, g.Ku, sm["lds"]),
               sjob(cs, sm["bs"], g.Sp, OP, sm["lds"], off=g.Ku, unique=2)]
        jobs = ws["scatter"] = (L.ScatterJob * len(lst))(*lst)
    L.check(lib.wae_unpack_scatter_add_multi(jobs, len(jobs), st), "scatter layer gradients")
    wg_off = lay.off("wavenet.conv_layers.0.conv1x1g.weight_v") if (g.Cg > 0 and gvec is not None) else -1
    L.check(lib.wae_gproj_bwd(L.ptr(eng.eff), L.ptr(eng.d_eff), wg_off, lay.off("wavenet.conv_layers.0.conv.bias"), lay.layer_stride,
                              None, 0, L.ptr(gvec), L.ptr(c1), Z2 * sm["ld1"], sm["ld1"], g.k * g.Rp + g.Ccp, B, 1, g.G, g.Hp,
                              max(g.Cg, 0), 0, st), "gproj_bwd")
    eng.flight.grads_done = eng.flight.finish_used = None
    eng.flight.norm_summed = False
    finish_grads(eng)
    return ws["gx"], (ws["dc"] if g.Ccp else None)


def _debug_kernels(eng, B, T, l, flags_u=0, flags_x=0):
    """(du/dz launch, dx launch) of layer l as closures over the workspaces of the last train step (tools/ablate_tm.py,
    flags_*: extra wae_tm_desc flags (L.TM_ONE_WG)."""
    cx = _step(eng, B, T)
    cx.tm_ev = None
    ngx = len(cx.ws["gx"])
    gn, gc = cx.ws["gx"][(l + 1) % ngx], cx.ws["gx"][l % ngx]
    return (lambda: _k_u(cx, l, gn, cx.parts[0], flags_u)), (lambda: _k_x(cx, l, gn, gc, cx.parts[0], flags_x))


def window_kind(eng, B, T):
    """Which weight-gradient launch a (B, T) micro-batch fills the tiles with -- True: the static launch's transposed dW_out / dW_skip
    blocks.  The gather pass reads ONE layout, so a window holds micro-batches of one kind."""
    _prepare_bwd(eng)
    return bool(use_stream_tn(eng) and static_tn_shape(eng, B, T))


def finish_window(eng, win, grad_sync=None):
    """The close of an accumulation window: everything _finish_layers / finish_grads do for a plain step, ONCE, on the tiles and d_eff
    that the window's micro-batches added into -- the first conv's tile to d_eff, the bias row-sum scatter, the gather pass over tiles,
    rest and outer rows (or the split launches: scatter, weight-norm backward), and with the gather pass the norm.  The tables are
    those of the last micro-batch's workspace: they address engine-level buffers only.  -> eng.grads"""
    cx = _step(eng, *win.shape)
    fl = eng.flight
    cx.finish = fl.finish_used = _finish_plan(cx)
    cx.finish_acc = cx.finish is not None and grad_sync is None and not eng.opt.deterministic      # (its norm: train.clip_adam_ema)
    _first_conv_finish(cx)
    done = _finish_layers(cx, 0, eng.g.layers, with_head=True, zb=False)
    eng.join(done[0] if done else None)
    fl.grads_done, fl.norm_summed = None, False
    if cx.finish is not None:
        fl.grads_done, fl.norm_summed = layer_segment(eng), cx.finish_acc
    return finish_grads(eng)


def finish_grads(eng):
    """d_eff (gradient wrt effective weights) -> grads (wrt weight_g / weight_v and plain parameters); the slice that
    decoder_backward already finished for the all-reduce (eng.flight.grads_done) is left alone."""
    lay, fl = eng.lay, eng.flight
    done, plan = fl.grads_done, fl.finish_used
    if plan is not None and done is not None and tuple(done) == tuple(layer_segment(eng)):
        # the gather pass served the segment: the rest of the arena in ONE launch of the same kernel (its rows read d_eff), which adds
        # their squares to the norm's accumulator as well -- instead of two launches per side of the segment and a pass for the norm
        _finish_rows(eng, plan, 0, lay.total, "outer", fl.norm_summed)
        fl.grads_done = None
    elif done is None:
        _wn_bwd_range(eng, 0, lay.total)
    else:
        if done[0] > 0:
            _wn_bwd_range(eng, 0, done[0])
        if done[1] < lay.total:
            _wn_bwd_range(eng, done[1], lay.total)
        fl.grads_done = None
    return eng.grads


def _vq_backward(eng, sv, dq, B, Tq, loss_scale):
    """The quantiser's backward on the saved (B, Cc, Tq) record: dlat = dq + the commitment term (straight-through), the codebooks'
    gradients added into eng.d_eff.  A packed list (frontend_backward_list) is B = 1, Tq = sum Tq_i.  -> dlat"""
    g, lib, lay, st = eng.g, eng.lib, eng.lay, eng.stream()
    lat, quant, idx = sv.lat, sv.quant, sv.idx
    dlat = torch.empty_like(lat)
    en = "vq.embedding.weight"
    if g.vq != "plain":
        # the sliced / EMA kinds: every slice's rows of dlat, and its codebook's gradient where it has one (EMA codebooks: none --
        # their arena slice keeps the zero gradient under which the optimizer leaves them alone)
        _, c_lat, c_emb = P.vq_coeffs(g, sv.beta)
        scale = float(loss_scale) * 2.0 / (B * g.Cc * Tq)
        for s, (name, d0, Ds, K) in enumerate(P.vq_slice_specs(g)):
            demb = eng.d_eff[lay.off(name + ".weight"):] if c_emb is not None else None
            head = (L.ptr(lat), L.ptr(quant), L.ptr(idx[s] if g.vq_n > 1 else idx), L.ptr(dq), L.ptr(dlat), L.ptr(demb), B, g.Cc, d0, Ds, Tq)
            if eng.opt.deterministic:
                L.check(lib.wae_vq_slice_bwd_det(*head, K, scale * c_lat, scale * (c_emb or 0.0), st), "vq_slice_bwd_det")
            else:
                L.check(lib.wae_vq_slice_bwd(*head, scale * c_lat, scale * (c_emb or 0.0), st), "vq_slice_bwd")
    elif eng.opt.deterministic:      # the codebook gradient by one workgroup per code
        L.check(lib.wae_vq_bwd_det(L.ptr(lat), L.ptr(quant), L.ptr(idx), L.ptr(dq), L.ptr(dlat), L.ptr(eng.d_eff[lay.off(en):]), B,
                                   g.Cc, Tq, g.K, sv.beta, loss_scale, st), "vq_bwd_det")
    else:
        L.check(lib.wae_vq_bwd(L.ptr(lat), L.ptr(quant), L.ptr(idx), L.ptr(dq), L.ptr(dlat), L.ptr(eng.d_eff[lay.off(en):]), B, g.Cc,
                               Tq, sv.beta, loss_scale, st), "vq_bwd")
    return dlat


def frontend_backward(eng, dc: torch.Tensor, loss_scale: float = 1.0, stop_at_quant: bool = False):
    """dc (B,T,Ccp) -> upsample stages -> conv_in -> [VQ straight-through + vq_loss -> encoder]; adds the weight
    gradients into eng.d_eff.  Uses the activations kept by the last train-mode forward (eng.saved)."""
    g, lib, lay, st = eng.g, eng.lib, eng.lay, eng.stream()
    B, T = dc.shape[0], dc.shape[1]
    sv = saved_for(eng, B, T)
    dev = eng.device
    d = torch.empty(B, g.Cc, T, dtype=torch.float32, device=dev)
    L.check(lib.wae_from_btc_scaled(L.ptr(dc), L.ptr(d), B, g.Cc, T, g.Ccp, eng.dt, 1.0 / eng.grad_scale, st), "from_btc")
    acts = sv.up_acts                        # [conv_in input | None, stage-0 input, stage-1 input, ...]
    keep = [d]
    if not g.conv_in and g.cin_pad > 0:      # plain UpsampleNetwork: the forward trimmed `indent` samples at either end (upsample.py:64-65)
        trim = g.cin_pad * int(np.prod(g.upsample_scales))
        d = torch.nn.functional.pad(d, (trim, trim))
        keep.append(d)
    act = P.UP_ACT_KINDS.get(g.up_act, 0)
    for i in range(len(g.upsample_scales) - 1, -1, -1):
        s = g.upsample_scales[i]
        xin = acts[1 + i]
        name = P.up_stage_name(g, i) + ".weight_v"
        if act:        # through the stage's activation, whose output is the next stage's input (the last stage's: kept by the forward)
            yout = acts[2 + i] if i + 1 < len(g.upsample_scales) else sv.up_last
            d = d.contiguous()
            L.check(lib.wae_act_bwd(L.ptr(yout), L.ptr(d), d.numel(), act, float(g.up_act_slope), st), "upsample activation bwd")
        din = torch.empty_like(xin)
        if eng.opt.deterministic:
            parts = eng.det_buffer("ups", int(lib.wae_upsample_stage_bwd_det_floats()))
            L.check(lib.wae_upsample_stage_bwd_det(L.ptr(d), L.ptr(xin), L.ptr(eng.eff[lay.off(name):]), L.ptr(din),
                                                   L.ptr(eng.d_eff[lay.off(name):]), L.ptr(parts), parts.numel(), B, g.Cc, xin.shape[-1], s,
                                                   st), "upsample_stage_bwd_det")
        else:
            L.check(lib.wae_upsample_stage_bwd(L.ptr(d), L.ptr(xin), L.ptr(eng.eff[lay.off(name):]), L.ptr(din),
                                               L.ptr(eng.d_eff[lay.off(name):]), B, g.Cc, xin.shape[-1], s, st), "upsample_stage_bwd")
        d = din
        keep.append(d)
    if g.conv_in:
        cin = acts[0]
        kin = 2 * g.cin_pad + 1
        name = "wavenet.upsample_net.conv_in.weight"
        dq = torch.empty_like(cin)
        L.check(lib.wae_enc_conv_bwd(L.ptr(cin), L.ptr(eng.eff[lay.off(name):]), None, L.ptr(d), L.ptr(dq),
                                     L.ptr(eng.d_eff[lay.off(name):]), None, B, g.Cc, cin.shape[-1], g.Cc, kin, 1, 0, 0, 0, st), "conv_in bwd")
    else:
        dq = d                               # no conv_in: the stages' input gradient IS the gradient of the features
    keep.append(dq)
    eng.hold("fe", keep)      # (the list itself: the encoder's side below appends to it)
    if stop_at_quant:
        return dq
    if sv.lat is not None and g.has_encoder:
        lat = sv.lat
        Tq = lat.shape[-1]
        dlat = _vq_backward(eng, sv, dq, B, Tq, loss_scale)
        ea = sv.enc_acts                     # ea[i] = input of block i, ea[10] = output of block 9
        dx = torch.empty_like(ea[10])
        L.check(lib.wae_enc_conv_bwd(L.ptr(ea[10]), L.ptr(eng.eff[lay.off("encoder.lin.weight"):]), None, L.ptr(dlat), L.ptr(dx),
                                     L.ptr(eng.d_eff[lay.off("encoder.lin.weight"):]), L.ptr(eng.d_eff[lay.off("encoder.lin.bias"):]),
                                     B, g.encoder_hid, Tq, g.Cc, 1, 1, 0, 0, 0, st), "lin bwd")
        keep += [dlat, dx]
        dcur = dx
        for i in range(len(P.ENCODER_BLOCKS) - 1, -1, -1):
            k, s = P.ENCODER_BLOCKS[i]
            wn_, bn_ = f"encoder.net.{i}.conv.weight", f"encoder.net.{i}.conv.bias"
            co, ci, _ = lay.shapes[wn_]
            xin, yout = ea[i], ea[i + 1]
            dxi = torch.empty_like(xin) if i > 0 else None
            L.check(lib.wae_enc_conv_bwd(L.ptr(xin), L.ptr(eng.eff[lay.off(wn_):]), L.ptr(yout), L.ptr(dcur), L.ptr(dxi),
                                         L.ptr(eng.d_eff[lay.off(wn_):]), L.ptr(eng.d_eff[lay.off(bn_):]), B, ci, xin.shape[-1], co,
                                         k, s, k // 2, 1, int(s == 1 and ci == co), st), "enc block bwd")
            keep.append(dxi)
            dcur = dxi
    return dq


def frontend_backward_list(eng, dc: torch.Tensor, loss_scale: float = 1.0):
    """frontend_backward for the LIST front end of a ragged step (WaeEngine.train_step_list; include/wae.h: "backward of the front end
    over a LIST"): dc (B, Tmax, Ccp) of the dense decoder -> wae_from_btc_list (item b's rows [b Tmax, b Tmax + T_b) to the packed
    (Cc, sum T_i) gradient, times 1 / grad_scale) -> the stages -> conv_in -> the quantiser on the packed latents as one clip -> lin
    and the encoder blocks, one list launch each; adds the weight gradients into eng.d_eff as frontend_backward does.  Uses the
    packed activations and tables the list forward left in eng.saved.list_fe."""
    g, lib, lay, st, dev = eng.g, eng.lib, eng.lay, eng.stream(), eng.device
    B, T = dc.shape[0], dc.shape[1]
    sv = saved_for(eng, B, T)
    fe = sv.list_fe
    tp = fe.plan
    t_enc, t_ups, t_bwd = fe.tables
    total = int(tp.Ts.sum())
    d = torch.empty(g.Cc, total, dtype=torch.float32, device=dev)
    L.check(lib.wae_from_btc_list(L.ptr(dc), L.ptr(d), L.ptr(t_bwd[tp.fb_off:]), B, tp.fb_ntiles, total, B * T, g.Cc, g.Ccp, eng.dt,
                                  1.0 / eng.grad_scale, st), "from_btc_list")
    acts = fe.up_acts                     # [conv_in's packed input | None, stage-0 input, stage-1 input, ...]
    keep = [d]
    for i in range(len(g.upsample_scales) - 1, -1, -1):
        s = int(g.upsample_scales[i])
        name = P.up_stage_name(g, i) + ".weight_v"
        in_pitch, out_pitch = tp.stage_pitch[i]
        din = torch.empty(g.Cc, in_pitch, dtype=torch.float32, device=dev)
        args = (L.ptr(d), L.ptr(acts[1 + i]), L.ptr(eng.eff[lay.off(name):]), L.ptr(din), L.ptr(eng.d_eff[lay.off(name):]),
                L.ptr(t_bwd[tp.stage_off[i]:]), B, tp.stage_ntiles[i], in_pitch, out_pitch, g.Cc, s)
        if eng.opt.deterministic:
            parts = eng.det_buffer("ups_list", int(lib.wae_upsample_stage_bwd_list_det_floats()))
            L.check(lib.wae_upsample_stage_bwd_list_det(*args, L.ptr(parts), parts.numel(), st), "upsample_stage_bwd_list_det")
        else:
            L.check(lib.wae_upsample_stage_bwd_list(*args, st), "upsample_stage_bwd_list")
        d = din
        keep.append(d)
    if g.conv_in:
        ln = tp.ups.launches[0]
        name = "wavenet.upsample_net.conv_in.weight"
        dq = torch.empty_like(acts[0])
        L.check(lib.wae_enc_conv_bwd_list(L.ptr(acts[0]), L.ptr(eng.eff[lay.off(name):]), None, L.ptr(d), L.ptr(dq),
                                          L.ptr(eng.d_eff[lay.off(name):]), None, L.ptr(t_ups[ln.seg_off:]), ln.nsegs,
                                          L.ptr(t_ups[ln.tile_off:]), ln.ntiles, ln.et, ln.in_pitch, ln.out_pitch, g.Cc, g.Cc, ln.s, 1, 0, 0,
                                          0, st), "conv_in bwd (list)")
    else:
        dq = d
    keep.append(dq)
    eng.hold("fe", keep)
    if sv.lat is None or not g.has_encoder:
        return dq
    Tq = sv.lat.shape[-1]                    # the packed latents as ONE clip: (1, Cc, sum Tq_i), no gap columns
    dlat = _vq_backward(eng, sv, dq, 1, Tq, loss_scale)
    ea, layers = fe.enc_acts, tp.enc.layers        # ea[i]: the packed input of layer i (ten blocks, then lin)
    convs = encoder_convs(eng)
    dcur = dlat
    keep.append(dlat)
    for i in range(len(convs) - 1, -1, -1):
        (name, relu), ly = convs[i], layers[i]
        co, ci = lay.shapes[name + ".weight"][:2]
        dxi = torch.empty_like(ea[i]) if i > 0 else None
        res = int(bool(relu) and ly.stride == 1 and ci == co)
        L.check(lib.wae_enc_conv_bwd_list(L.ptr(ea[i]), L.ptr(eng.eff[lay.off(name + ".weight"):]), L.ptr(ea[i + 1]) if relu else None,
                                          L.ptr(dcur), L.ptr(dxi), L.ptr(eng.d_eff[lay.off(name + ".weight"):]),
                                          L.ptr(eng.d_eff[lay.off(name + ".bias"):]), L.ptr(t_enc[ly.seg_off:]), ly.nsegs,
                                          L.ptr(t_enc[ly.tile_off:]), ly.ntiles, ly.et, ly.in_pitch, ly.out_pitch, ci, co, ly.k, ly.stride,
                                          ly.pad, relu, res, st), "enc_conv_bwd_list")
        keep.append(dxi)
        dcur = dxi
    return dq
