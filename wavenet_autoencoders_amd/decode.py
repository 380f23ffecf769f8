"""Autoregressive decode, host side: every route from WaeEngine's decode methods to a wae_ar_generate* entry (include/wae.h).

Three forms of launch -- "batch" (incremental_forward / incremental_stream: B equal-length utterances), "list" (decode_list /
decode_list_scalar: a work list of ragged items in one launch) and "spans" (DecodeSession: the next span of every live clip) -- each
for class-id and scalar-input decoders, on one-CU workgroups or on cooperative teams.  They share ONE of each of: the descriptor
(ar_desc), the small routing rules (team_width, group_count, mixture, coop_sized / refuse_wide), the per-item checks (clip_intake),
the per-clip draws (clip_draws), the conditioning of a list (_list_cond), the list decode (decode_list) and the launch (ENTRIES,
ar_args, launch).  The functions take the engine as `eng`, like backward.py's; WaeEngine keeps the public methods, the packed weights and the helpers that read them (_ar_cond_rows,
_ar_speaker_rows, _ar_exchange, _ar_net_args, _ar_scalar_path, _ar_check_exchange).  What the routes do differently on purpose is
listed in DESIGN.md ("Decode host path").
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import types

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import frontend as F
from . import packing as P

# include/wae.h: wae_ar_item and wae_ar_span, as the host packs them
_AR_ITEM = np.dtype([("off", "<i8"), ("T", "<i4"), ("n_forced", "<i4"), ("init_idx", "<i4"), ("row", "<i4")])
_AR_SPAN = np.dtype([("off", "<i8"), ("ring", "<i8"), ("T", "<i4"), ("t0", "<i4"), ("n_forced", "<i4"), ("init_idx", "<i4"),
                     ("row", "<i4"), ("reserved", "<i4")])

# (form, scalar, coop) -> entry.  scalar: False (class ids), True, or "normal" for the one entry that has the distribution in its
# name instead of a `dist` argument: the one-CU batch decode of a "Normal" geometry.
ENTRIES = {
    ("batch", False, False): "wae_ar_generate",
    ("batch", False, True): "wae_ar_generate_coop_fused",
    ("batch", True, False): "wae_ar_generate_scalar",
    ("batch", "normal", False): "wae_ar_generate_scalar_mog",
    ("batch", True, True): "wae_ar_generate_coop_scalar",
    ("list", False, False): "wae_ar_generate_list",
    ("list", False, True): "wae_ar_generate_coop_list",
    ("list", True, False): "wae_ar_generate_scalar_list",
    ("list", True, True): "wae_ar_generate_coop_scalar_list",
    ("spans", False, False): "wae_ar_generate_spans",
    ("spans", False, True): "wae_ar_generate_coop_spans",
    ("spans", True, False): "wae_ar_generate_scalar_spans",
    ("spans", True, True): "wae_ar_generate_coop_scalar_spans",
}


def ar_args(key, d, net, operands, stream, *, C=1, dist=0, queue=(), total=0, exchange=(), w_fused=None):
    """The positional arguments of ENTRIES[key], by the rule above _lib._AR: the descriptor; C on the team entries; dist on the scalar
    entries that take one (all but the one-CU batch entries); a work list's `queue` = (n, slots or teams, records, next) and, on
    the team entries, `total`; the 15 network arguments `net`; the operands -- (inputs, uniforms, out, logits), or (inputs, u_mix, draws,
    log_scale_min, clamp, out, params), "normal" without the clamp --; on the team entries `exchange` = (msg, acc, err) and, batch
    class-id only, w_fused; the stream."""
    form, scalar, coop = key
    head = (C,) if coop else ()
    if scalar and (coop or form != "batch"):
        head += (dist,)
    if form != "batch":
        head += tuple(queue) + ((total,) if coop else ())
    if scalar == "normal":
        operands = operands[:4] + operands[5:]
    tail = (tuple(exchange) + ((w_fused,) if form == "batch" and not scalar else ())) if coop else ()
    return (ctypes.byref(d),) + head + tuple(net) + tuple(operands) + tail + (stream,)


def launch(eng, key, d, net, operands, *, hold=None, exchange=None, w_fused=None, **head):
    """One launch of ENTRIES[key] on the engine's stream; on a team entry (`exchange`: the (msg, acc, err) tensors, zeroed) the
    time-out word is then read back (eng._ar_check_exchange: one device read).  `hold`: called between the two, where the caller
    stores the launch's operands -- which frees the previous launch's while the kernel runs, not in front of it."""
    name = ENTRIES[key]
    ex = () if exchange is None else tuple(L.ptr(t) for t in exchange)
    L.check(getattr(eng.lib, name)(*ar_args(key, d, net, operands, eng.stream(), exchange=ex, w_fused=L.ptr(w_fused), **head)), name[4:])
    if hold is not None:
        hold()
    if key[2]:
        eng._ar_check_exchange(exchange[2], name[4:])


# ---- the small rules every route reads
def team_width(eng):
    """C: workgroups of one cooperative team (one utterance's gate rows over up to 32 CUs of an XCD)"""
    return max(1, min(eng.opt.ar_coop_c, 32, eng.g.H, eng.g.S))


def group_count(eng, coop, slots, teams):
    """Teams of a cooperative launch (`teams`, clamped to 1..8: one XCD each) or its one-CU workgroups (`slots`; default: one per CU)"""
    if coop:
        return max(1, min(8 if teams is None else int(teams), 8))
    return torch.cuda.get_device_properties(eng.device).multi_processor_count if slots is None else int(slots)


def mixture(g):
    """(normal, M): whether a scalar-input decoder draws from Gaussians, and its mixture count (0 for a class-id decoder)"""
    normal = g.scalar_input and g.output_distribution == "Normal"
    return normal, ((1 if (normal and g.O == 2) else g.O // 3) if g.scalar_input else 0)


def coop_sized(g):
    return max(g.R, g.S, g.O) <= 256


def refuse_wide(g, who, instead):
    if not coop_sized(g):
        raise ValueError(f"{who}(coop=True): the cooperative kernels take R, S and O <= 256 (got {g.R}, {g.S}, {g.O}); "
                         f"use the one-CU {instead} (coop=False)")


def ar_desc(eng, *, B, T, mode, init_idx, n_forced, coop):
    """THE wae_ar_desc of a decode.  The kernel-form triple (coop_generic, resident_lds, resident_regs) is read by the cooperative
    entries only: a class-id decoder passes the engine's own (ar_path), a scalar-input one what _ar_scalar_path() says, together with
    the request for the constant-size scalar kernels (scalar_input = 2) under ar_path(scalar_fast=True)."""
    g, path = eng.g, ()
    if coop:
        path = eng._ar_scalar_path() if g.scalar_input else (int(eng.ar_generic), eng.ar_resident[0], eng.ar_resident[1])
    d = L.ArDesc(eng.dt, B, T, g.layers, g.R, g.Rp, g.G, g.Hp, g.S, g.O, max(g.Cc, 0), g.Ccp, g.k, mode, int(init_idx),
                 int(g.scalar_input), math.sqrt(1.0 / g.layers), n_forced, *path)
    d.scalar_sized = int(bool(coop) and eng.ar_scalar_fast)
    return d


def _operands(g, inputs, uni, u_mix, draw, log_scale_min, clamp, out, logits):
    if g.scalar_input:
        return (L.ptr(inputs), L.ptr(u_mix), L.ptr(draw), log_scale_min, clamp, L.ptr(out), L.ptr(logits))
    return (L.ptr(inputs), L.ptr(uni), L.ptr(out), L.ptr(logits))


def _io(g):
    """(dtype of the inputs and outputs, the outputs' key in the result)"""
    return (torch.float32, "x") if g.scalar_input else (torch.int32, "idx")


def _wrong_draws(normal, u_log, z, at=""):
    if normal and u_log is not None:
        raise ValueError(f"{at}output_distribution 'Normal' draws from u_mix and z, not u_log")
    if not normal and z is not None:
        raise ValueError(f"{at}output_distribution 'Logistic' draws from u_mix and u_log, not z")


def scalar_draws(eng, T):
    g, dev = eng.g, eng.device
    normal, M = mixture(g)
    if normal:      # mixture.py:249 (the mixture pick, M > 1 only), then Normal(...).sample() (:266)
        u_mix = torch.rand(1, T, M, device=dev) * (1 - 2e-5) + 1e-5 if M > 1 else None
        return u_mix, torch.randn(1, T, device=dev)
    u_mix = torch.rand(1, T, M, device=dev) * (1 - 2e-5) + 1e-5          # mixture.py:138,151
    return u_mix, torch.rand(1, T, device=dev) * (1 - 2e-5) + 1e-5


# ---- one item of a list or a session
def clip_intake(g, device, mode, item, who, index=None, check_ids=True, open_clip=False):
    """Every check of one item (decode_list's / decode_list_scalar's mapping) for `mode` (0 "logits", 1 "argmax", 2 "sample"), before
    anything else is allocated -> (T, forced, n_forced, init_idx, given): the forced prefix on `device` (at most T values; None where
    there is none), the start class (0 where a prefix is forced, and for scalar-input decoders) and whether the item brings its own
    scalar draws.  check_ids=False leaves the class-id range of the prefix to the caller (decode_list reads its packed array once).
    open_clip (DecodeSession.open): the item has no T and no c yet -- T comes back None, the forced prefix whole, and what depends on
    T (the teacher-forced cover of mode "logits") is DecodeSession.end's to check."""
    at = f"{who}: " if index is None else f"{who}: item {index}: "
    T = None if open_clip else int(item["T"])
    if not open_clip and T < 1:
        raise ValueError(f"{at}every clip has at least one step (got {T})")
    if not open_clip and g.Ccp and item.get("c") is None:
        raise ValueError(f"{at}no conditioning c, the decoder has {g.Cc} conditioning channels")
    ti = item.get("test_inputs")
    if ti is not None:
        ti = torch.as_tensor(ti).reshape(-1).to(device, _io(g)[0])[:T]
    nf = 0 if ti is None else int(ti.numel())
    if not open_clip and mode == 0 and nf < T:
        raise ValueError(f"{at}mode 'logits' is teacher-forced: test_inputs must cover all {T} steps")
    init, given = 0, False
    if g.scalar_input:
        normal, M = mixture(g)
        um, ul, z = item.get("u_mix"), item.get("u_log"), item.get("z")
        _wrong_draws(normal, ul, z, at)
        if not normal and (um is None) != (ul is None):
            raise ValueError(f"{at}u_mix and u_log come together")
        if normal and z is not None and M > 1 and um is None:
            raise ValueError(f"{at}{M} Gaussians need u_mix beside z")
        given = (z if normal else ul) is not None
    else:
        init = item.get("init_idx")
        init = 127 if init is None else int(torch.as_tensor(init).reshape(-1)[0])
        if nf == 0 and not 0 <= init < g.O:
            # wavenet.py:288 writes a one at the start class of the start vector: the same IndexError when there are fewer classes
            raise IndexError(f"index {init} is out of bounds for dimension 2 with size {g.O}")
        if check_ids and nf and (int(ti.min()) < 0 or int(ti.max()) >= g.O):
            raise IndexError(f"{at}test_inputs hold a class id outside [0, {g.O})")
        init = init if nf == 0 else 0
    return T, (ti if nf else None), nf, init, given


def clip_draws(eng, item, T, given, at):
    """(uni, u_mix, draw) of one clip that samples, flat on the device: the item's own draws, or -- where it brings none -- what
    incremental_forward draws for that utterance alone, by the same expressions in the same order (torch.rand(1, T); scalar_draws)."""
    g, dev = eng.g, eng.device
    flat = lambda a: torch.as_tensor(a).reshape(-1).to(dev, torch.float32)  # noqa: E731
    if not g.scalar_input:
        u = item.get("uniforms")
        uni = (torch.rand(1, T, device=dev) if u is None else flat(u)).reshape(-1).contiguous()
        assert uni.numel() == T, f"{at}{uni.numel()} uniforms for {T} steps"
        return uni, None, None
    normal, M = mixture(g)
    um, dr = (item.get("u_mix"), item.get("z" if normal else "u_log")) if given else eng.scalar_draws(T)
    if not normal or M > 1:
        um = flat(um)
        assert um.numel() == T * M, f"{at}u_mix holds {um.numel()} values for {T} steps of {M} mixtures"
        um = um.view(T, M).contiguous()
    else:
        um = None
    dr = flat(dr).contiguous()
    assert dr.numel() == T, f"{at}{dr.numel()} draws for {T} steps"
    return None, um, dr


def _clip_cond(eng, item, T, c_is_upsampled, out, at):
    """the item's conditioning (one utterance of batch 1) -> out (T, Ccp), zeroed"""
    c = torch.as_tensor(item["c"]).to(eng.device, torch.float32)
    eng._ar_cond_rows((c if c.dim() == 3 else c[None]).contiguous(), out.view(1, T, eng.g.Ccp), c_is_upsampled, at)


def _list_cond(eng, items, Ts, c_is_upsampled, out, offsets, at):
    """The conditioning of a whole list -> the rows [offsets_i, offsets_i + T_i) of out (rows, Ccp) through ONE upsample_list
    (WaeEngine.upsample_list: a launch per stage for the list, not per item).  The length check of _ar_cond_rows runs here for every
    item, with at(i) in front, before the first launch."""
    g, cs = eng.g, [it["c"] if hasattr(it["c"], "shape") else torch.as_tensor(it["c"]) for it in items]
    direct = c_is_upsampled or not g.upsample_scales
    for i, (c, T) in enumerate(zip(cs, Ts)):
        shape = tuple(c.shape)
        shape = shape if len(shape) == 3 else (1,) + shape
        if direct:
            assert shape[-1] == T, f"{at(i)}c {shape} != T {T}"       # wavenet.py:278
        else:
            assert (shape[-1] - 2 * g.cin_pad) * int(np.prod(g.upsample_scales)) == T, f"{at(i)}c does not upsample to T"
    eng.upsample_list(cs, out=out, offsets=offsets, c_is_upsampled=c_is_upsampled)


def _gid32(eng, gids):
    return torch.tensor([int(torch.as_tensor(x).reshape(-1)[0]) for x in gids], dtype=torch.int32, device=eng.device)


# ---- batch: incremental_forward / incremental_stream
@dataclasses.dataclass
class _ArDecode:
    """One batch decode between ar_open and its launches (ar_launch): what does not depend on the chunk."""
    # geometry, mode, start class, ar_path() settings.  ONE descriptor for all launches: ar_launch overwrites d.T, d.n_forced and d.t0
    # with the chunk's before every call (the library reads it during the call, never later), so outside a launch those three are stale
    d: L.ArDesc
    n_forced: int               # steps of the clip that `forced` covers
    forced: Optional[torch.Tensor]
    c_up: Optional[torch.Tensor]
    zb: torch.Tensor
    gid32: Optional[torch.Tensor]   # (held only so that wae_gproj_fwd's operand outlives its launch)
    coop: bool
    C: int
    ring: torch.Tensor          # the decode's state: every launch continues in it
    normal: bool
    uni: Optional[torch.Tensor]
    u_mix: Optional[torch.Tensor]
    draw: Optional[torch.Tensor]    # u_log, or z of a "Normal" decoder
    sampled: bool
    want: bool
    log_scale_min: float
    clamp: int
    w_fused: Optional[torch.Tensor]
    exchange: Optional[tuple]       # (msg, acc, err) of a cooperative decode
    last: Optional[torch.Tensor] = None     # (B,) the previous launch's last output


def ar_open(eng, c, gid, T, *, mode, test_inputs, uniforms, init_idx, c_is_upsampled, want_logits, gvec, u_mix, u_log,
            log_scale_min, clamp_log_scale, n_forced, z):
    """What a decode of T steps fixes before its first launch, whatever its chunks (incremental_forward's arguments) -> the state
    ar_launch runs steps of: the packed weights, the start classes, the forced prefix, the upsampled conditioning, the speaker
    rows, the kernel path, the zeroed ring, the draws of all T steps and the exchange buffers."""
    g, dev = eng.g, eng.device
    if not eng._ar_packed or eng.weights_dirty:
        eng.pack_ar_weights()
    T = int(T)
    B = c.shape[0] if c is not None else (test_inputs.shape[0] if test_inputs is not None else 1)
    m = {"logits": 0, "argmax": 1, "sample": 2, "probs": 3, "raw": 4}[mode]
    if not isinstance(init_idx, int) and not g.scalar_input:
        ii = torch.as_tensor(init_idx).reshape(-1).to("cpu", torch.int64)
        if ii.numel() == 1:
            init_idx = int(ii[0])
        else:
            if ii.numel() != B:
                raise ValueError(f"init_idx: {ii.numel()} start classes for {B} utterances")
            if int(ii.min()) < 0 or int(ii.max()) >= g.O:
                raise IndexError(f"index {int(ii.max() if ii.max() >= g.O else ii.min())} is out of bounds for dimension 2 with size {g.O}")
            if test_inputs is None:     # (forced steps override the start class anyway: wavenet.py:300-302)
                test_inputs, n_forced = ii.to(dev, torch.int32).reshape(B, 1), 1
            init_idx = int(ii[0])
    nf = 0
    if test_inputs is not None:
        nf = int(test_inputs.shape[1]) if n_forced is None else int(n_forced)
        nf = max(0, min(nf, int(test_inputs.shape[1]), T))
        if nf == 0:
            test_inputs = None
    if m == 0 and nf < T:
        raise ValueError("mode 'logits' is teacher-forced: test_inputs must cover all T steps (use 'raw' to feed logits back)")
    if g.scalar_input and m not in (0, 2):
        raise ValueError("scalar-input decoders feed the drawn sample back: modes 'logits' and 'sample' only")
    c_up = None
    if g.Ccp:
        c_up = torch.zeros(B, T, g.Ccp, dtype=eng.tdtype, device=dev)
        eng._ar_cond_rows(c.contiguous().float(), c_up, c_is_upsampled)
    gid32 = gid.to(torch.int32).contiguous() if gid is not None else None
    zb = eng._ar_speaker_rows(B, gid32, gvec)
    # one utterance per XCD, its gate rows split over up to 32 CUs (csrc/ar_coop.hip); bigger batches run one
    # utterance per CU (csrc/ar_fwd.hip): better aggregate throughput, 3-4x lower speed per utterance
    # scalar-input decoders take that path on request only (ar_path(scalar_coop=True)), in the modes their kernel has
    coop = (B <= 8 and coop_sized(g) and m <= 2 and eng.opt.ar_coop and (not g.scalar_input or (eng.ar_scalar_coop and m in (0, 2))))
    C = team_width(eng) if coop else 1
    # zeros: the rows read as history before their first write (t - d, t - 2d of the first samples) are the causal pad; the
    # cooperative kernel zero-fills its ring itself, but only when its members share an XCD.  Every launch of the decode continues in it.
    ring = torch.zeros(B * C * eng.ar_ring_total, dtype=torch.float32, device=dev)
    normal, M = mixture(g)
    uni = um = draw = None
    if g.scalar_input:
        _wrong_draws(normal, u_log, z)
        if m == 2 and (z if normal else u_mix) is None:     # scalar_draws' expressions in its order, for B utterances at once
            u_mix = torch.rand(B, T, M, device=dev) * (1 - 2e-5) + 1e-5 if (M > 1 or not normal) else None
            if normal:
                z = torch.randn(B, T, device=dev)
            else:
                u_log = torch.rand(B, T, device=dev) * (1 - 2e-5) + 1e-5
        forced = test_inputs.to(dev, torch.float32).contiguous() if test_inputs is not None else None
        um = u_mix.to(dev, torch.float32).contiguous() if u_mix is not None else None
        draw = z if normal else u_log
        draw = draw.to(dev, torch.float32).contiguous() if draw is not None else None
        sampled = (draw if normal else um) is not None
        init_idx = 0
    else:
        forced = test_inputs.to(dev, torch.int32).contiguous() if test_inputs is not None else None
        if forced is None and not 0 <= int(init_idx) < g.O:
            # wavenet.py:288 writes a one at class 127 of the start vector: the same IndexError when there are fewer classes
            raise IndexError(f"index {int(init_idx)} is out of bounds for dimension 2 with size {g.O}")
        if m == 2 and uniforms is None:
            uniforms = torch.rand(B, T, device=dev)
        uni = uniforms.to(dev).float().contiguous() if uniforms is not None else None
        sampled = True
    d = ar_desc(eng, B=B, T=T, mode=m, init_idx=init_idx, n_forced=nf, coop=coop)
    # (not zeroed here: ar_launch zeroes them before every launch)
    exchange = eng._ar_exchange(d, C, B, torch.empty) if coop else None
    return _ArDecode(d=d, n_forced=nf, forced=forced, c_up=c_up, zb=zb, gid32=gid32, coop=coop, C=C, ring=ring, normal=normal,
                     uni=uni, u_mix=um, draw=draw, sampled=sampled, want=want_logits or m == 0 or m >= 3,
                     log_scale_min=float(log_scale_min), clamp=int(bool(clamp_log_scale)),
                     w_fused=eng.ar_wm if eng.ar_one_handover else None, exchange=exchange)


def ar_launch(eng, s, t0, n):
    """Steps [t0, t0 + n) of the decode `s` (ar_open) as one launch -> the dict incremental_forward returns, for those steps."""
    g, dev, d = eng.g, eng.device, s.d
    dt, key = _io(g)
    sl = lambda a: None if a is None else a[:, t0:t0 + n].contiguous()  # noqa: E731  (B == 1 or the whole clip: the slice itself, no copy)
    k = max(0, min(n, s.n_forced - t0))         # steps of this launch that the caller's inputs force
    if k > 0 or t0 > 0:
        if k == n:
            inp = sl(s.forced)
        else:                                   # the kernels index inputs as (B, n)
            inp = torch.zeros(d.B, n, dtype=dt, device=dev)
            if k > 0:
                inp[:, :k] = s.forced[:, t0:t0 + k]
            else:
                inp[:, 0] = s.last              # past the forced prefix a continuation starts from the previous launch's last output
        d.n_forced = max(1, k)
    else:
        inp, d.n_forced = None, 0
    d.T, d.t0 = n, t0
    cu, uc, um, dr = sl(s.c_up), sl(s.uni), sl(s.u_mix), sl(s.draw)
    logits = torch.empty(d.B, g.O, n, dtype=torch.float32, device=dev) if s.want else None
    out = torch.empty(d.B, n, dtype=dt, device=dev) if s.sampled else None
    if s.coop:
        for t in s.exchange:
            t.zero_()
    scalar = ("normal" if s.normal and not s.coop else True) if g.scalar_input else False
    launch(eng, ("batch", scalar, s.coop), d, eng._ar_net_args(s.ring, s.zb, cu),
           _operands(g, inp, uc, um, dr, s.log_scale_min, s.clamp, out, logits), C=s.C, dist=int(s.normal), exchange=s.exchange,
           w_fused=s.w_fused)
    s.last = out[:, -1] if out is not None else None
    eng._ar_keep = (s, cu, inp, uc, um, dr)     # the launch's operands (and the decode's: ring, zb, ...) live until the stream has run
    return {key: out, "logits": logits}


def ar_chunks(eng, s, chunks):
    """The launches of an open incremental_stream: chunk k runs steps [t0, t0 + n) with wae_ar_desc.t0 = t0."""
    t0, mine = 0, None
    try:
        for n in chunks:
            item = ar_launch(eng, s, t0, n)
            mine = eng._ar_keep
            t0 += n
            yield item
    finally:
        if eng._ar_keep is mine:
            eng._ar_keep = None    # closed (early or at the end): the ring and the operands go with the generator


# ---- list: decode_list / decode_list_scalar
def decode_list(eng, who, items, m, *, slots, want_logits, c_is_upsampled, coop, teams, log_scale_min=-7.0, clamp_log_scale=False):
    """WaeEngine.decode_list and decode_list_scalar behind their own refusals: `items` (not empty) in mode m, ONE launch.  Every item
    is checked before anything is drawn or allocated; what differs between class-id and scalar-input decoders is data -- the dtype
    of inputs and outputs, which draws there are, the operands and the result's key."""
    g, dev, n = eng.g, eng.device, len(items)
    (dt, key), (normal, M), scalar = _io(g), mixture(g), bool(g.scalar_input)
    Ts = [int(it["T"]) for it in items]
    plan = P.ar_list_plan(Ts, group_count(eng, coop, slots, teams))      # longest first; clamps slots / teams to the item count
    off, total = [int(o) for o in plan.offsets], plan.total
    gids = [it.get("gid") for it in items]
    if any(x is None for x in gids) and not all(x is None for x in gids):
        raise ValueError(f"{who}: give every item a gid, or none")
    took = [clip_intake(g, dev, m, it, who, i, check_ids=False) for i, it in enumerate(items)]
    forced, nfs, inits, given = ([t[k] for t in took] for k in (1, 2, 3, 4))
    if scalar and m == 0 and any(given) and not all(given):
        raise ValueError(f"{who}: mode 'logits': give every item its draws (then the samples come back too), or none")
    draws = m == 2 or (scalar and all(given))
    if not eng._ar_packed or eng.weights_dirty:
        eng.pack_ar_weights()
    inputs = None
    if any(nfs):        # the forced prefixes at their items' offsets, zeros behind them
        inputs = torch.zeros(total, dtype=dt, device=dev)
        for o, f, k in zip(off, forced, nfs):
            if k:
                inputs[o:o + k] = f
        if not scalar and (int(inputs.min()) < 0 or int(inputs.max()) >= g.O):
            raise IndexError(f"{who}: test_inputs hold a class id outside [0, {g.O})")
    c_up = None
    if g.Ccp:           # every item's conditioning rows at its offset
        c_up = torch.zeros(total, g.Ccp, dtype=eng.tdtype, device=dev)
        _list_cond(eng, items, Ts, c_is_upsampled, c_up, off, lambda i: f"item {i}: ")
    gid32 = _gid32(eng, gids) if gids[0] is not None else None
    zb = eng._ar_speaker_rows(n, gid32)         # one row per item, in the caller's order (item.row = the caller's index)
    uni = um_d = dr_d = None
    if draws:
        uni = torch.empty(total, dtype=torch.float32, device=dev) if not scalar else None
        um_d = torch.empty(total, M, dtype=torch.float32, device=dev) if scalar and (not normal or M > 1) else None
        dr_d = torch.empty(total, dtype=torch.float32, device=dev) if scalar else None
        for i, it in enumerate(items):      # item after item in the caller's order: a seeded list is a seeded loop
            for dst, src in zip((uni, um_d, dr_d), clip_draws(eng, it, Ts[i], given[i], f"item {i}: ")):
                if dst is not None:
                    dst[off[i]:off[i] + Ts[i]] = src
    rec = np.zeros(n, dtype=_AR_ITEM)           # in launch order
    assert rec.dtype.itemsize == ctypes.sizeof(L.ArItem)
    for k, i in enumerate(plan.order):
        rec[k] = (off[i], Ts[i], nfs[i], inits[i], int(i))
    items_d, nxt = torch.from_numpy(rec.view(np.uint8)).to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.empty(total, dtype=dt, device=dev) if draws or not scalar else None
    want = want_logits or m == 0
    logits = torch.empty(total * g.O, dtype=torch.float32, device=dev) if want else None
    d = ar_desc(eng, B=n, T=0, mode=m, init_idx=0, n_forced=0, coop=coop)
    # One ring per slot, or per member of every team.  Not zeroed: a decode reads a history row only behind its own write of it
    # (csrc/ar_fwd.hip: ar_decode; the any-shape cooperative kernel likewise, the constant-size ones clear it per item), in the first
    # item of a slot as in every later one.  The exchange buffers are allocated zeroed, for this one launch.
    C = team_width(eng) if coop else 1
    ring = torch.empty(plan.slots * C * eng.ar_ring_total, dtype=torch.float32, device=dev)
    exchange = eng._ar_exchange(d, C, plan.slots, torch.zeros) if coop else None

    def hold():     # the launch's operands live until the next decode
        eng._ar_keep = (items_d, nxt, ring, zb, gid32, c_up, inputs, uni, um_d, dr_d, exchange)
    launch(eng, ("list", scalar, bool(coop)), d, eng._ar_net_args(ring, zb, c_up),
           _operands(g, inputs, uni, um_d, dr_d, float(log_scale_min), int(bool(clamp_log_scale)), out, logits), hold=hold,
           C=C, dist=int(normal), queue=(n, plan.slots, L.ptr(items_d), L.ptr(nxt)), total=total, exchange=exchange)
    return [{key: None if out is None else out[o:o + T], "logits": logits[o * g.O:(o + T) * g.O].view(g.O, T) if want else None}
            for o, T in zip(off, Ts)]


# ---- spans: decode sessions
@dataclasses.dataclass
class _ArClip:
    """One clip of a DecodeSession between add() and its last step: what ar_open fixes once per decode, kept per clip."""
    T: int
    slot: int                       # the clip's ring and zb row in the session's tables
    c_up: Optional[torch.Tensor]    # (T, Ccp) conditioning rows of the whole clip
    forced: Optional[torch.Tensor]  # the forced prefix (class ids, or floats of a scalar-input decoder)
    n_forced: int
    init: int
    uni: Optional[torch.Tensor]     # (T,) uniforms of the categorical draw
    u_mix: Optional[torch.Tensor]   # (T, M) / (T,) draws of a scalar-input decoder
    draw: Optional[torch.Tensor]
    pos: int = 0                    # steps decoded so far = t0 of the next span
    last: Optional[torch.Tensor] = None     # (1,) the previous span's last output, on the device
    feed: Optional["_Feed"] = None  # a clip joined with open(): its conditioning arrives while it decodes


@dataclasses.dataclass
class _Feed:
    """What an open clip has beside _ArClip, whose T stays 0 until end() and whose c_up is a view of the session's c_up rows (bound
    again whenever the arenas move)."""
    base: int = 0                   # the clip's first column in stage 0's arena, in latent frames
    cap: int = 0                    # latent frames the clip has room for in the arenas
    frames: int = 0                 # latent frames fed so far
    planned: int = 0                # ... when the clip's ranges last ran
    ended: bool = False
    ended_planned: bool = False
    ready: int = 0                  # audio-rate rows of c_up that are final
    max_frames: Optional[int] = None
    given: Optional[bool] = None    # whether the draws come with the feeds (fixed by the first feed)
    drawn: int = 0                  # steps the draws cover
    slot: int = -1                  # a windowed session: the clip's ring in every arena (base = slot * window, cap = window)
    doff: int = 0                   # ... and the step of the first draw still held: uni / u_mix / draw are [doff, drawn)


class DecodeSession:
    """WaeEngine.decode_session: clips of any lengths that join at any time and decode in rounds, one launch per round (include/wae.h:
    the four wae_ar_generate*_spans entries).  add() does once per clip what a decode does once
    (the conditioning rows of the whole clip, the speaker row, the clip's own history ring, the draws of all its steps); step() decodes
    the next span of every live clip in one launch and returns the spans' outputs; a clip's outputs, concatenated over the rounds, are
    bit for bit its single decode (incremental_forward alone: on the one-CU kernel for coop=False, on the cooperative path for
    coop=True), whatever the chunking and whichever slot or team took which span.
    A clip may also join before its conditioning exists: open() / feed() / feed_list() / end() ("Clips that are fed while
    they decode").  step() then decodes min(chunk, ready - pos) steps of it, `ready` being the audio-rate conditioning rows that no
    later frame can change; its result dict carries `ready`, and `done` is true only once the clip has ended and pos == T.  The bits
    are those of the clip decoded whole, whatever the feeding.
    window=W (latent frames, at least packing.feed_window_min(scales)): the clips joined with open() live in constant memory
    (include/wae.h: wae_upsample_stage_fwd_rings).  Every open clip owns a RING of W * prod(scales[:i]) columns in
    stage i's arena and of W * prod(scales) c_up rows, column u at slot * period + u % period; nothing is copied when a clip grows,
    and the ring of any clip that left goes to the next one.  One call feeds a clip at most max_feed frames, and -- back-pressure --
    never rows that would overwrite c_up rows it has not decoded: room(h) says how many frames it can take now, and grows as step()
    advances.  The draws step() has consumed are dropped.  Clips joined with add / add_list are untouched.  The bits do not depend
    on the window: the ring is an address, never an operand."""

    def __init__(self, eng, mode="sample", coop=False, slots=None, teams=None, want_logits=False, c_is_upsampled=False,
                 log_scale_min=-7.0, clamp_log_scale=False, window=None):
        g = eng.g
        if g.scalar_input and coop and not eng.ar_scalar_coop:
            raise NotImplementedError("decode_session(coop=True): scalar-input decoders decode their sessions on the one-CU slots "
                                      "(coop=False); the team form of the scalar span list does not exist yet")
        if coop:
            refuse_wide(g, "decode_session", "slots")
        modes = {"logits": 0, "sample": 2} if g.scalar_input else {"logits": 0, "argmax": 1, "sample": 2}
        if mode not in modes:
            raise ValueError(f"decode_session: mode '{mode}' is not decoded in spans; use " + ", ".join(f"'{k}'" for k in modes))
        self.eng, self.mode, self.coop, self.want = eng, modes[mode], bool(coop), bool(want_logits) or modes[mode] == 0
        self.c_is_upsampled, self.log_scale_min, self.clamp = bool(c_is_upsampled), float(log_scale_min), int(bool(clamp_log_scale))
        self._slots, self._teams = slots, teams
        self.clips: Dict[int, _ArClip] = {}
        self._next_handle, self._gids, self._closed, self._open = 0, None, False, False
        self._keep = None
        # open clips (open / feed / end): per-stage channel-major arenas and the time-major c_up rows, in latent frames of room
        self._fa, self._fa_cup, self._fa_mul, self._fa_cap, self._fa_top, self._fa_pending = None, None, None, 0, 0, False
        self.window, self.max_feed, self._fa_free = None if window is None else int(window), None, []
        if self.window is not None:
            scales = self._feed_geometry("decode_session(window=)")
            if self.window < P.feed_window_min(scales):
                prod, look = P.feed_lookahead(scales)
                raise ValueError(f"decode_session: window {self.window} is below the minimum of {P.feed_window_min(scales)} latent frames "
                                 f"(the c_up ring holds the {look} rows an open clip holds back and at least one frame of {prod})")
            self.max_feed = P.feed_window_max_feed(scales, self.window)

    # ---- the session's device state: once, at the first add
    def _open_device(self):
        eng, g = self.eng, self.eng.g
        if not eng._ar_packed or eng.weights_dirty:
            eng.pack_ar_weights()
        if self._open:
            return
        dev = eng.device
        self.nslots = max(1, group_count(eng, self.coop, self._slots, self._teams))
        self.d = ar_desc(eng, B=0, T=0, mode=self.mode, init_idx=0, n_forced=0, coop=self.coop)
        self.C, per, self.exchange = 1, eng.ar_ring_total, None
        if self.coop:
            self.C = team_width(eng)
            per = int(eng.lib.wae_ar_coop_ring_floats(ctypes.byref(self.d), self.C, eng.ar_ring_total))
            assert per > 0, per
            self.exchange = eng._ar_exchange(self.d, self.C, self.nslots, torch.empty)      # zeroed before every launch
        self.ring_floats = (per + 3) // 4 * 4       # span.ring is a multiple of 4 floats
        self.cap, self.free = 0, []
        self.ring = torch.empty(0, dtype=torch.float32, device=dev)
        self.zb = torch.empty(0, g.layers, 2 * g.Hp, dtype=torch.float32, device=dev)
        self.normal, self.M = mixture(g)
        self._open = True

    def reserve(self, n):
        """Room for n clips at once in the ring and speaker-row tables (they grow on demand; growing copies the live clips' rings)."""
        self._open_device()
        n = int(n)
        if n <= self.cap:
            return
        # never zeroed: a span reads a history row only behind its own write of it, or -- the constant-size cooperative kernels -- behind
        # the clearing its clip's first span makes
        ring = torch.empty(n * self.ring_floats, dtype=torch.float32, device=self.eng.device)
        zb = torch.empty(n, *self.zb.shape[1:], dtype=torch.float32, device=self.eng.device)
        ring[:self.ring.numel()] = self.ring
        zb[:self.cap] = self.zb
        self.free += list(range(n - 1, self.cap - 1, -1))
        self.ring, self.zb, self.cap = ring, zb, n

    @property
    def live(self):
        """handles of the clips that still have steps to decode, in the order they were added"""
        return list(self.clips)

    def add(self, item):
        """A clip joins: `item` is decode_list's / decode_list_scalar's mapping (T, c, gid, test_inputs, uniforms or u_mix / u_log / z,
        init_idx).  Legal at any time between two step() calls.  Returns the clip's handle."""
        if self._closed:
            raise RuntimeError("decode_session: the session is closed")
        eng, g, dev, who = self.eng, self.eng.g, self.eng.device, "decode_session.add"
        gid = item.get("gid")
        if self._gids is not None and (gid is not None) != self._gids:
            raise ValueError(f"{who}: give every item a gid, or none")
        T, forced, nf, init, given = clip_intake(g, dev, self.mode, item, who)      # (class ids checked per clip: one device read each)
        self._open_device()
        c_up = None
        if g.Ccp:
            c_up = torch.zeros(T, g.Ccp, dtype=eng.tdtype, device=dev)
            _clip_cond(eng, item, T, self.c_is_upsampled, c_up, f"{who}: ")
        gid32 = _gid32(eng, [gid]) if gid is not None else None
        zb = eng._ar_speaker_rows(1, gid32)
        uni, um, dr = clip_draws(eng, item, T, given, f"{who}: ") if self.mode == 2 else (None, None, None)
        if not self.free:
            self.reserve(max(2 * self.cap, self.nslots, 8))
        slot = self.free.pop()
        self.zb[slot] = zb[0]
        self._gids = gid is not None
        h = self._next_handle
        self._next_handle += 1
        self.clips[h] = _ArClip(T=T, slot=slot, c_up=c_up, forced=forced, n_forced=nf, init=init, uni=uni, u_mix=um, draw=dr)
        eng.hold("session_add", gid32, zb)
        return h

    def add_list(self, items):
        """Clips join together: equivalent to [sess.add(it) for it in items] -- the same checks, the same draws in the same order, the
        same handles -- with the conditioning of all of them through ONE WaeEngine.upsample_list (a launch per stage for the list,
        where add() runs the upsampling network per clip) and their speaker rows through one projection.  Every item is checked before
        anything is launched or joins: a list with a bad item adds nothing.  Each clip keeps a row slice of the packed result: the
        slices keep the group's buffer alive until its last clip ends.  Legal at any time between two step() calls.  Returns the
        clips' handles in the items' order."""
        if self._closed:
            raise RuntimeError("decode_session: the session is closed")
        items = list(items)
        if not items:
            return []
        eng, g, dev, who = self.eng, self.eng.g, self.eng.device, "decode_session.add"
        gids = [it.get("gid") for it in items]
        for gid in gids:
            if (gid is not None) != (self._gids if self._gids is not None else gids[0] is not None):
                raise ValueError(f"{who}: give every item a gid, or none")
        took = [clip_intake(g, dev, self.mode, it, who) for it in items]
        self._open_device()
        Ts = [t[0] for t in took]
        offs, c_up = np.concatenate([[0], np.cumsum(Ts)]).astype(np.int64), None
        if g.Ccp:
            c_up = torch.empty(int(offs[-1]), g.Ccp, dtype=eng.tdtype, device=dev)      # every row is an item's: all written
            _list_cond(eng, items, Ts, self.c_is_upsampled, c_up, offs[:-1], lambda i: f"{who}: ")
        gid32 = _gid32(eng, gids) if gids[0] is not None else None
        zb = eng._ar_speaker_rows(len(items), gid32)
        # clip after clip in the items' order, as a loop of add() draws; before anything joins, since a count assert may refuse
        draws = [clip_draws(eng, it, t[0], t[4], f"{who}: ") if self.mode == 2 else (None, None, None) for it, t in zip(items, took)]
        need = len(items) - len(self.free)
        if need > 0:
            self.reserve(max(2 * self.cap, self.nslots, 8, self.cap + need))
        slots = [self.free.pop() for _ in items]
        self.zb[torch.tensor(slots, dtype=torch.int64, device=dev)] = zb
        self._gids = gids[0] is not None
        hs = []
        for i, ((T, forced, nf, init, _), (uni, um, dr)) in enumerate(zip(took, draws)):
            h = self._next_handle
            self._next_handle += 1
            self.clips[h] = _ArClip(T=T, slot=slots[i], c_up=None if c_up is None else c_up[int(offs[i]):int(offs[i + 1])],
                                    forced=forced, n_forced=nf, init=init, uni=uni, u_mix=um, draw=dr)
            hs.append(h)
        eng.hold("session_add", gid32, zb)
        return hs

    # ---- clips whose conditioning arrives while they decode
    def _avail(self, c):
        """steps of clip c that can be decoded now: all of a clip that was added whole, the final rows of an open one (in mode
        "logits" no further than its forced inputs)"""
        if c.feed is None:
            return c.T
        return min(c.feed.ready, c.n_forced) if self.mode == 0 else c.feed.ready

    def _feed_geometry(self, who):
        g = self.eng.g
        if self.c_is_upsampled:
            raise NotImplementedError(f"{who}: c_is_upsampled conditioning has no upsampling to extend; join the clip whole with add")
        if not g.Ccp or not g.upsample_scales:
            raise NotImplementedError(f"{who}: this decoder has no upsampling network to feed; join the clip whole with add")
        if g.cin_pad > 0:
            raise NotImplementedError(f"{who}: cin_pad {g.cin_pad} > 0 makes conv_in read neighbouring frames; join the clip whole with add")
        if g.up_act != "none":
            raise NotImplementedError(f"{who}: an upsample_activation ({g.up_act}) is not fed in pieces; join the clip whole with add")
        if not P.upsample_list_supported(g):
            raise NotImplementedError(f"{who}: the time-major ranges kernel takes Ccp dividing 256 and 3 s <= 256 (got Ccp {g.Ccp}, "
                                      f"last scale {g.upsample_scales[-1]}); join the clip whole with add")
        return [int(s) for s in g.upsample_scales]

    def reserve_frames(self, n):
        """Room for n latent frames of open clips in all: the per-stage channel-major arenas ((Cc, n * prod(scales[:i])) fp32, stage
        i's input) and the time-major c_up rows ((n * prod(scales), Ccp) in the model's dtype).  They grow on demand, geometrically;
        growing copies what the open clips have so far.  Retained intermediates are not trimmed."""
        scales = self._feed_geometry("decode_session.reserve_frames")
        self._open_device()
        n = int(n)
        if self.window is not None:     # whole rings: slot j is the frames [j W, (j + 1) W) of room
            n = -(-n // self.window) * self.window
        if n <= self._fa_cap:
            return
        eng, g, dev = self.eng, self.eng.g, self.eng.device
        mul = [int(np.prod(scales[:i])) for i in range(len(scales) + 1)]
        if n * mul[-1] >= 2 ** 31:
            raise ValueError(f"decode_session: {n} latent frames of open clips reach 2^31 rows")
        fa = [torch.empty(g.Cc, n * m, dtype=torch.float32, device=dev) for m in mul[:-1]]
        cup = torch.empty(n * mul[-1], g.Ccp, dtype=eng.tdtype, device=dev)
        if self._fa_cap:
            for new, old in zip(fa, self._fa):
                new[:, :old.shape[1]] = old
            cup[:self._fa_cup.shape[0]] = self._fa_cup
        if self.window is not None:
            self._fa_free += list(range(n // self.window - 1, self._fa_cap // self.window - 1, -1))
        self._fa, self._fa_cup, self._fa_cap, self._fa_mul = fa, cup, n, mul
        for c in self.clips.values():
            self._bind(c)

    @property
    def arena_bytes(self):
        """bytes of the arenas of the open clips (windowed: nslots rings, whatever the clips' lengths)"""
        return sum(a.numel() * a.element_size() for a in (self._fa or []) + ([self._fa_cup] if self._fa_cup is not None else []))

    def _ring(self, c):
        """a windowed session: the ring of clip c -- the one freed last, else the arenas grow by rings, geometrically"""
        if not self._fa_free:
            self.reserve_frames(max(2 * self._fa_cap, 4 * self.window))
        f = c.feed
        f.slot = self._fa_free.pop()
        f.base, f.cap = f.slot * self.window, self.window
        self._bind(c)

    def room(self, handle):
        """A windowed session: the latent frames the open clip can take in one call now -- at most max_feed, and no more than keep
        its final rows within window * prod(scales) of the rows it has decoded; grows as step() advances."""
        c = self.clips[handle]
        if c.feed is None or self.window is None:
            raise ValueError(f"decode_session.room: clip {handle} is not an open clip of a windowed session")
        prod, look = P.feed_lookahead(self._feed_geometry("decode_session.room"))
        f = c.feed      # the rows final after n frames: prod (frames + n - 1) - look <= pos + window prod
        return 0 if f.ended else max(0, min(self.max_feed, (c.pos + self.window * prod + look) // prod + 1 - f.frames))

    def cond_rows(self, handle, lo, hi):
        """A copy of the rows [lo, hi) of an open clip's conditioning (c_up) while they are held: rows that are final and, in a
        windowed session, not yet overwritten -- the last window * prod(scales) of them.  ValueError once they are not."""
        c = self.clips[handle]
        if c.feed is None:
            raise ValueError(f"decode_session.cond_rows: clip {handle} joined whole (add)")
        if self._fa_pending:
            self.feed_list({})
        lo, hi, ready = int(lo), int(hi), c.feed.ready
        period = c.c_up.shape[0]
        first = max(0, ready - period) if self.window is not None else 0
        if not first <= lo <= hi <= ready:
            raise ValueError(f"decode_session.cond_rows: clip {handle} holds the rows [{first}, {ready}), not [{lo}, {hi})")
        return self._cup_rows(c, lo, hi - lo).clone()

    def _cup_rows(self, c, lo, n):
        """rows [lo, lo + n) of clip c's conditioning: a slice, or -- a ring -- two pieces where they wrap"""
        if c.feed is None or self.window is None:
            return c.c_up[lo:lo + n]
        period = c.c_up.shape[0]
        a = lo % period
        if a + n <= period:
            return c.c_up[a:a + n]
        return torch.cat([c.c_up[a:], c.c_up[:a + n - period]])

    def _bind(self, c):
        if c.feed is not None and self._fa_cup is not None:
            P_ = self._fa_mul[-1]
            c.c_up = self._fa_cup[c.feed.base * P_:(c.feed.base + c.feed.cap) * P_]

    def _place(self, c, need):
        """room for `need` latent frames of clip c: where it lies if it fits (or is the last and can stretch), else at the top of the
        arenas with what it has so far copied there"""
        f = c.feed
        if need <= f.cap:
            return
        cap = need if f.max_frames is not None else max(2 * f.cap, need, 8)
        if f.max_frames is not None:
            cap = max(cap, f.max_frames)
        if f.cap and f.base + f.cap == self._fa_top:
            self._fa_top = f.base
        base, top = self._fa_top, self._fa_top + cap
        if top > self._fa_cap:
            self.reserve_frames(max(2 * self._fa_cap, top))
        if base != f.base and f.frames:
            for a, m in zip(self._fa, self._fa_mul):
                a[:, base * m:(base + f.frames) * m] = a[:, f.base * m:(f.base + f.frames) * m].clone()
            P_ = self._fa_mul[-1]
            self._fa_cup[base * P_:base * P_ + f.ready] = self._fa_cup[f.base * P_:f.base * P_ + f.ready].clone()
        f.base, f.cap, self._fa_top = base, cap, top
        self._bind(c)

    def open(self, item, max_T=None):
        """A clip joins before its conditioning exists: `item` is add's mapping (gid, init_idx, test_inputs) without T and without c.
        The latent frames come with feed() / feed_list(), the clip decodes the rows that are final (step), and end() fixes its length.
        max_T: the most steps the clip will have -- its room in the arenas is taken once, and a feed beyond it is refused.  Draws (a
        uniforms / u_mix / u_log / z entry of `item`) are refused here: they come with the feeds.  NotImplementedError, naming add:
        c_is_upsampled sessions, cin_pad > 0, an upsample_activation, a decoder without an upsampling network.  Returns the handle."""
        if self._closed:
            raise RuntimeError("decode_session: the session is closed")
        eng, g, dev, who = self.eng, self.eng.g, self.eng.device, "decode_session.open"
        scales = self._feed_geometry(who)
        if item.get("T") is not None or item.get("c") is not None:
            raise ValueError(f"{who}: an open clip has no T and no c yet (feed its frames; a whole clip joins with add)")
        if any(item.get(k) is not None for k in ("uniforms", "u_mix", "u_log", "z")):
            raise ValueError(f"{who}: the draws of an open clip come with its feeds")
        gid = item.get("gid")
        if self._gids is not None and (gid is not None) != self._gids:
            raise ValueError(f"{who}: give every item a gid, or none")
        prod = int(np.prod(scales))
        if max_T is not None and int(max_T) < prod:
            raise ValueError(f"{who}: max_T {int(max_T)} is less than one latent frame ({prod} steps)")
        _, forced, nf, init, _ = clip_intake(g, dev, self.mode, item, who, open_clip=True)
        self._open_device()
        gid32 = _gid32(eng, [gid]) if gid is not None else None
        zb = eng._ar_speaker_rows(1, gid32)
        if not self.free:
            self.reserve(max(2 * self.cap, self.nslots, 8))
        slot = self.free.pop()
        self.zb[slot] = zb[0]
        self._gids = gid is not None
        h = self._next_handle
        self._next_handle += 1
        c = _ArClip(T=0, slot=slot, c_up=None, forced=forced, n_forced=nf, init=init, uni=None, u_mix=None, draw=None,
                    feed=_Feed(max_frames=None if max_T is None else int(max_T) // prod))
        self.clips[h] = c
        if self.window is not None:
            self._ring(c)
        elif c.feed.max_frames is not None:
            self._place(c, c.feed.max_frames)
        eng.hold("session_add", gid32, zb)
        return h

    def feed(self, handle, c, uniforms=None, u_mix=None, u_log=None, z=None):
        """Appends the latent frames c (Cc, f) to one open clip: feed_list({handle: c}, ...) with this clip's draws."""
        one = lambda a: None if a is None else {handle: a}  # noqa: E731
        return self.feed_list({handle: c}, uniforms=one(uniforms), u_mix=one(u_mix), u_log=one(u_log), z=one(z))

    def end(self, handle):
        """The clip has all its frames: T = F * prod(scales), and the rows that waited for a next frame become final -- the closing
        ranges run with the next feed_list() or step().  ValueError: a clip that is not open, that has ended, that has no frames, whose
        supplied draws or -- mode "logits" -- forced inputs do not cover T."""
        who = "decode_session.end"
        c = self.clips[handle]
        f = c.feed
        if f is None:
            raise ValueError(f"{who}: clip {handle} joined whole (add); only open clips end")
        if f.ended:
            raise ValueError(f"{who}: clip {handle} has ended")
        if f.frames < 1:
            raise ValueError(f"{who}: clip {handle} has no frames: every clip has at least one step")
        T = f.frames * self._fa_mul[-1]
        if self.mode == 2 and f.given and f.drawn < T:
            raise ValueError(f"{who}: clip {handle} ends at {T} steps beyond the {f.drawn} draws supplied")
        if self.mode == 0 and c.n_forced < T:
            raise ValueError(f"{who}: mode 'logits' is teacher-forced: test_inputs must cover all {T} steps")
        if self.window is not None and T - c.pos > self.window * self._fa_mul[-1]:
            raise ValueError(f"{who}: clip {handle}: its {T} rows with {c.pos} decoded do not fit the {self.window * self._fa_mul[-1]} "
                             f"rows of its c_up ring: step first")
        f.ended, c.T, self._fa_pending = True, T, True

    def _feed_draws(self, who, h, c, frames, after, draws):
        """the draws that come with a feed of `frames` frames to clip h, flat on the device, checked against the rows final `after`
        it: (uni, u_mix, draw, steps they cover), or None where the engine draws.  The first feed that brings frames or draws fixes
        which of the two the clip does."""
        g, f = self.eng.g, c.feed
        uni, um, ul, z = (None if d is None else d.get(h) for d in draws)
        if self.mode != 2:
            if any(a is not None for a in (uni, um, ul, z)):
                raise ValueError(f"{who}: clip {h}: draws are for mode 'sample'")
            return None
        flat = lambda a: torch.as_tensor(a).reshape(-1).to(self.eng.device, torch.float32)  # noqa: E731
        if not g.scalar_input:
            if um is not None or ul is not None or z is not None:
                raise ValueError(f"{who}: clip {h}: a class-id decoder draws from uniforms")
            given, got = uni is not None, None if uni is None else (flat(uni), None, None)
        else:
            if uni is not None:
                raise ValueError(f"{who}: clip {h}: a scalar-input decoder draws from u_mix and u_log or z, not uniforms")
            _wrong_draws(self.normal, ul, z, f"{who}: clip {h}: ")
            dr = z if self.normal else ul
            if (not self.normal or self.M > 1) and (um is None) != (dr is None):
                raise ValueError(f"{who}: clip {h}: u_mix and {'z' if self.normal else 'u_log'} come together")
            given, got = dr is not None, None
            if given:
                dr, um = flat(dr), (flat(um) if um is not None and (not self.normal or self.M > 1) else None)
                if um is not None:
                    if um.numel() != dr.numel() * self.M:
                        raise ValueError(f"{who}: clip {h}: u_mix holds {um.numel()} values for {dr.numel()} steps of {self.M} mixtures")
                    um = um.view(-1, self.M)
                got = (None, um, dr)
        if f.given is not None and given != f.given and (frames or given):
            raise ValueError(f"{who}: clip {h}: the draws come with every feed of a clip, or with none")
        if not given:
            return None
        n = int((got[0] if got[0] is not None else got[2]).numel())
        if after > f.drawn + n:
            raise ValueError(f"{who}: clip {h}: this feed makes {after} steps final, beyond the {f.drawn + n} draws supplied")
        return got + (n,)

    def feed_list(self, feeds, uniforms=None, u_mix=None, u_log=None, z=None):
        """Latent frames for many open clips: `feeds` maps handle -> c (Cc, f) or (1, Cc, f), f >= 0, host or device.  ONE conv_in
        launch on the new frames (wae_enc_conv_fwd_list; pointwise at cin_pad 0), ONE wae_upsample_stage_fwd_ranges launch per stage
        and ONE table upload per call, however many clips are fed (packing.session_feed_plan); clips that have ended since the last
        call get their closing ranges in the same launches.  The rows a clip has final are, bit for bit, the rows upsample_forward
        writes for the whole clip, whatever the feeding.
        Draws of mode "sample": mappings handle -> draws, as add's item entries.  A clip brings draws with every feed or with none.
        With them, the clip decodes bit for bit as its single decode on the concatenated draws; a feed must not make more rows final
        than the draws supplied so far cover (f * prod(scales) draws with f frames always do).  Without them the engine's generator
        draws at feed time, clip after clip in the order of this call's plan (the session's order of joining), for the rows this feed
        makes final -- NOT add's order, which draws a clip's T steps at once: a seeded fed clip differs from the seeded added clip.
        Refused before anything is launched (ValueError): a handle that is not an open clip, a feed after end, frames that are not
        (Cc, f), a feed beyond max_T or beyond the draws supplied.  Returns {handle: ready} for the clips whose rows moved."""
        if self._closed:
            raise RuntimeError("decode_session: the session is closed")
        eng, g, dev, who = self.eng, self.eng.g, self.eng.device, "decode_session.feed"
        feeds, draws = dict(feeds), (uniforms, u_mix, u_log, z)
        for d in draws:
            for h in (d or {}):
                if h not in feeds:
                    raise ValueError(f"{who}: draws for clip {h}, which this call does not feed")
        scales = self._feed_geometry(who) if feeds else None
        prod, look = P.feed_lookahead(scales) if feeds else (0, 0)
        new, got = {}, {}
        for h, c in feeds.items():
            clip = self.clips.get(h)
            if clip is None or clip.feed is None:
                raise ValueError(f"{who}: clip {h} is not an open clip of this session")
            f = clip.feed
            if f.ended:
                raise ValueError(f"{who}: clip {h} has ended: no feed after end")
            shape = tuple(getattr(c, "shape", ()))
            shape = shape[1:] if len(shape) == 3 and shape[0] == 1 else shape
            if len(shape) != 2 or shape[0] != g.Cc:
                raise ValueError(f"{who}: clip {h}: frames of shape {tuple(getattr(c, 'shape', ()))}; a feed is (Cc, f) or (1, Cc, f) "
                                 f"with Cc = {g.Cc}")
            n = int(shape[1])
            if f.max_frames is not None and f.frames + n > f.max_frames:
                raise ValueError(f"{who}: clip {h}: {f.frames + n} frames are beyond max_T ({f.max_frames} frames)")
            if self.window is not None and n:
                if (f.frames + n) * prod >= 2 ** 31:
                    raise ValueError(f"{who}: clip {h}: {f.frames + n} frames reach 2^31 rows")
                if n > self.max_feed:
                    raise ValueError(f"{who}: clip {h}: a feed of {n} frames; a window of {self.window} admits max_feed = {self.max_feed} "
                                     f"per call")
                if n > self.room(h):
                    raise ValueError(f"{who}: clip {h}: a feed of {n} frames would overwrite conditioning rows it has not decoded "
                                     f"(room {self.room(h)}: {max(0, prod * (f.frames + n - 1) - look)} final rows, {clip.pos} decoded, a ring "
                                     f"of {self.window * prod}); step first")
            new[h] = n
            if self.mode == 2 or any(d is not None for d in draws):     # (the rows final after this feed: packing.feed_ready)
                got[h] = self._feed_draws(who, h, clip, n, max(0, prod * (f.frames + n - 1) - look), draws)
        # everything is checked: room, then the plan over every open clip with rows to run
        ring = self.window is not None
        for h, n in new.items():
            if n and not ring:
                self._place(self.clips[h], self.clips[h].feed.frames + n)
        todo = [(h, c) for h, c in self.clips.items() if c.feed is not None
                and (new.get(h, 0) or c.feed.frames != c.feed.planned or c.feed.ended != c.feed.ended_planned)]
        self._fa_pending = False
        if not todo:
            return {}
        scales = scales or self._feed_geometry(who)
        if eng.weights_dirty:
            eng.prepare_weights()
        if ring:    # the planner refuses what a ring cannot hold, before anything is launched
            plan = P.session_feed_plan_rings(scales, [(c.feed.slot, c.feed.planned, c.feed.ended_planned, c.feed.frames + new.get(h, 0),
                                                       c.feed.ended, c.pos) for h, c in todo], self.window)
        else:
            plan = P.session_feed_plan(scales, [(c.feed.base, c.feed.planned, c.feed.ended_planned, c.feed.frames + new.get(h, 0),
                                                 c.feed.ended) for h, c in todo])
        fed = [(h, self.clips[h]) for h, n in new.items() if n]
        parts, conv = [plan.table], None
        if fed:     # the new frames, packed in this call's order, and where they go in stage 0's arena
            ns = [new[h] for h, _ in fed]
            dst = [c.feed.base + c.feed.frames for _, c in fed]
            if ring:    # a feed that crosses its ring's end is two segments (conv_in is pointwise at cin_pad 0: any split, the same bytes)
                W, pieces = self.window, []
                for (_, c), n in zip(fed, ns):
                    a = c.feed.frames % W
                    first = min(n, W - a)
                    pieces += [(c.feed.base + a, first)] + ([(c.feed.base, n - first)] if n > first else [])
                dst, ns = [p[0] for p in pieces], [p[1] for p in pieces]
            segs, tiles, et, _ = P.enc_list_tables(ns, 1, 1, 0)
            segs[:, 2] = dst
            conv = types.SimpleNamespace(seg_off=plan.table.size, tile_off=plan.table.size + segs.size, nsegs=len(segs), ntiles=len(tiles),
                                         et=et, in_pitch=int(sum(ns)))      # (the record frontend.conv_list takes)
            parts += [segs.reshape(-1), tiles.reshape(-1)]
            if not g.conv_in:       # the plain network: the frames are stage 0's input as they are
                parts.append(np.concatenate([np.arange(o, o + n) for o, n in zip(segs[:, 2], ns)]).astype(np.int32))
        table = torch.from_numpy(np.concatenate(parts)).to(dev)        # ONE upload
        x = None
        if fed:
            x = F.pack_time(eng, [feeds[h] for h, _ in fed], g.Cc)
            if g.conv_in:
                conv.out_pitch = self._fa[0].shape[1]
                F.conv_list(eng, x, self._fa[0], table, conv, "wavenet.upsample_net.conv_in.weight", None, g.Cc, g.Cc, (1, 1, 0, 0, 0),
                            "conv_in (feed)")
            else:
                self._fa[0].index_copy_(1, table[conv.tile_off + 2 * conv.ntiles:].long(), x)
        for ln in plan.launches:
            w = eng.eff[eng.lay.off(P.up_stage_name(g, ln.stage) + ".weight_v"):]
            out = self._fa_cup if ln.last else self._fa[ln.stage + 1]
            entry = eng.lib.wae_upsample_stage_fwd_rings if ring else eng.lib.wae_upsample_stage_fwd_ranges
            L.check(entry(L.ptr(self._fa[ln.stage]), L.ptr(w), L.ptr(out), L.ptr(table[ln.rec_off:]), ln.nrecs, ln.ntiles,
                          self._fa[ln.stage].shape[1], out.shape[0] if ln.last else out.shape[1], g.Cc, ln.s, int(ln.last), g.Ccp, eng.dt,
                          eng.stream()), "upsample_stage (rings)" if ring else "upsample_stage (ranges)")
        eng.hold("session_feed", table, x)
        moved = {}
        for (h, c), ready in zip(todo, plan.ready):
            f, ready = c.feed, int(ready)
            f.frames += new.get(h, 0)
            f.planned, f.ended_planned = f.frames, f.ended
            if self.mode == 2:
                if f.given is None and (new.get(h, 0) or got.get(h) is not None):
                    f.given = got.get(h) is not None
                self._append_draws(c, got.get(h), ready)
            if ready != f.ready:
                moved[h] = ready
            f.ready = ready
        return moved

    def _append_draws(self, c, got, ready):
        """the clip's draws grow: by what came with the feed, or -- the engine's generator -- by clip_draws' expressions for the rows
        that became final"""
        f = c.feed
        if got is not None:
            uni, um, dr, n = got
        else:
            n = ready - f.drawn
            if f.given or n < 1:
                return
            uni, um, dr = clip_draws(self.eng, {}, n, False, "decode_session.feed: ")
        cat = lambda old, a: a if old is None or a is None else torch.cat([old, a])  # noqa: E731
        c.uni, c.u_mix, c.draw, f.drawn = cat(c.uni, uni), cat(c.u_mix, um), cat(c.draw, dr), f.drawn + n

    def _drop_draws(self, c):
        """a windowed clip's draws that step() has consumed go: uni / u_mix / draw keep [pos, drawn) -- copied out of the longer
        tensor once the consumed part outweighs the rest, so the memory held stays within twice the live draws"""
        f = c.feed
        gone = c.pos - f.doff
        if gone < max(f.drawn - c.pos, 256):
            return
        keep = lambda a: None if a is None else a[gone:].clone()  # noqa: E731
        c.uni, c.u_mix, c.draw, f.doff = keep(c.uni), keep(c.u_mix), keep(c.draw), c.pos

    def drop(self, handle):
        """Cancels a clip: it leaves the session and its ring is free for the next add."""
        c = self.clips.pop(handle)
        self.free.append(c.slot)
        if c.feed is not None and self.window is not None:
            self._fa_free.append(c.feed.slot)
        elif c.feed is not None:    # the clip's columns: the top of the arenas falls back where it was the last, and to 0 with the last open clip
            if c.feed.base + c.feed.cap == self._fa_top:
                self._fa_top = c.feed.base
            if not any(k.feed is not None for k in self.clips.values()):
                self._fa_top = 0

    def step(self, chunk):
        """One launch: the next min(chunk, remaining) steps of every live clip (`chunk`: an int, or a mapping from handle to steps -- a
        clip the mapping leaves out sits the round out).  Returns {handle: dict(idx | x, logits, done)} for the clips that decoded: the
        span's class ids (n,) int32 or samples (n,) fp32, its logits / mixture parameters (O, n) where asked for, and whether the clip
        has finished -- it has then left the session.  The forced first input of a continuation comes from the previous round's output
        on the device; only the team path reads one word back per launch (the time-out flag).
        A clip joined with open() decodes min(chunk, ready - pos) steps, `ready` being its conditioning rows that are final: with
        ready == pos it sits the round out (absent from the result, not done).  Its dict also carries `ready`, and `done` is true only
        once the clip has ended and pos == T.  Clips that ended since the last feed get their closing ranges first."""
        if self._closed:
            raise RuntimeError("decode_session: the session is closed")
        handles = list(self.clips)
        if not handles:
            return {}
        if self._fa_pending:        # clips that ended since the last feed: their closing ranges
            self.feed_list({})
        if not isinstance(chunk, (int, np.integer)):
            chunk = {handles.index(h): int(n) for h, n in dict(chunk).items()}
        clips = [self.clips[h] for h in handles]
        plan = P.ar_round_plan([self._avail(c) - c.pos for c in clips], [c.pos for c in clips], chunk, self.nslots)
        if plan.total == 0:
            return {}
        eng, g, dev = self.eng, self.eng.g, self.eng.device
        dt, key = _io(g)
        sel = [clips[int(i)] for i in plan.clips]
        ns, offs, total = [int(x) for x in plan.lengths], [int(x) for x in plan.offsets], plan.total
        # (the draws of a windowed clip start at its feed.doff: the consumed ones are dropped)
        at = lambda c: c.pos - (c.feed.doff if c.feed is not None else 0)  # noqa: E731
        cut = lambda name, on=True: torch.cat([getattr(c, name)[at(c):at(c) + n] for c, n in zip(sel, ns)]) if on else None  # noqa: E731
        c_up = torch.cat([self._cup_rows(c, c.pos, n) for c, n in zip(sel, ns)]) if g.Ccp else None
        # the forced steps: a clip's forced prefix where the span lies in it, else -- a continuation -- the previous span's last output
        nfs, inputs = [0] * len(sel), None
        if any(c.pos > 0 or c.n_forced > 0 for c in sel):
            inputs = torch.zeros(total, dtype=dt, device=dev)
            dst, src = [], []
            for j, (c, n, off) in enumerate(zip(sel, ns, offs)):
                k = max(0, min(n, c.n_forced - c.pos))
                if k > 0:
                    inputs[off:off + k] = c.forced[c.pos:c.pos + k]
                elif c.pos > 0:
                    dst.append(off)
                    src.append(c.last)
                    k = 1
                nfs[j] = k
            if dst:
                inputs.index_copy_(0, torch.tensor(dst, dtype=torch.int64, device=dev), torch.cat(src))
        rec = np.zeros(len(sel), dtype=_AR_SPAN)
        assert rec.dtype.itemsize == ctypes.sizeof(L.ArSpan)
        for k, j in enumerate(plan.order):
            c = sel[int(j)]
            rec[k] = (offs[j], c.slot * self.ring_floats, ns[j], c.pos, nfs[j], c.init, c.slot, 0)
        spans = torch.from_numpy(rec.view(np.uint8)).to(dev)
        nxt = torch.zeros(1, dtype=torch.int32, device=dev)
        logits = torch.empty(total * g.O, dtype=torch.float32, device=dev) if self.want else None
        sampled, scalar = self.mode == 2, bool(g.scalar_input)
        uni = cut("uni", sampled and not scalar)
        um, dr = cut("u_mix", sampled and scalar and (not self.normal or self.M > 1)), cut("draw", sampled and scalar)
        out = torch.empty(total, dtype=dt, device=dev) if sampled or not scalar else None
        for t in self.exchange or ():
            t.zero_()

        def hold():     # the launch's operands live until the next round's
            self._keep = (spans, nxt, c_up, inputs, out, logits, uni, um, dr)
        launch(eng, ("spans", scalar, self.coop), self.d, eng._ar_net_args(self.ring, self.zb, c_up),
               _operands(g, inputs, uni, um, dr, self.log_scale_min, self.clamp, out, logits), hold=hold, C=self.C, dist=int(self.normal),
               queue=(len(sel), plan.slots, L.ptr(spans), L.ptr(nxt)), total=total, exchange=self.exchange)
        res = {}
        for i, c, n, off in zip(plan.clips, sel, ns, offs):
            h = handles[int(i)]
            c.pos += n
            if self.window is not None and c.feed is not None:
                self._drop_draws(c)
            if out is not None:
                c.last = out[off + n - 1:off + n]
            done = c.pos >= c.T and (c.feed is None or c.feed.ended)
            res[h] = {key: None if out is None else out[off:off + n],
                      "logits": logits[off * g.O:(off + n) * g.O].view(g.O, n) if self.want else None, "done": done}
            if c.feed is not None:
                res[h]["ready"] = c.feed.ready
            if done:
                self.drop(h)
        return res

    def close(self):
        """Frees everything: the clips, their rings and the exchange buffers.  Results already returned stay valid."""
        self.clips.clear()
        self._closed = True
        self.ring = self.zb = self.exchange = self._keep = self._fa = self._fa_cup = None
        self._fa_free = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def list_rounds(sess, items, chunk):
    """The rounds of decode_list_stream: the session `sess` holding the fixed list `items`."""
    with sess:
        sess.reserve(len(items))
        hs = sess.add_list(items)
        while sess.live:
            n = chunk if isinstance(chunk, (int, np.integer)) else {hs[int(i)]: v for i, v in dict(chunk).items() if hs[int(i)] in sess.clips}
            res = sess.step(n)
            if not res:
                raise ValueError("decode_list_stream: the chunk mapping leaves every live clip out")
            yield [res.get(h) for h in hs]
