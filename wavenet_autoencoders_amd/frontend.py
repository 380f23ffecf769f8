"""The front end's host path: encoder, quantiser and upsampling network, dense and for a LIST of utterances of unequal lengths.
Functions that take the engine as `eng` (as backward.py and decode.py; nothing here imports engine.py): WaeEngine keeps the public
methods and their docstrings.  ONE of each: the packer of a list onto the device (pack_time), the encoder's layer list
(encoder_convs), its list chain (enc_list_chain), the upsampling list chain (ups_list_chain), the wae_enc_conv_fwd_list call
(conv_list).  Every helper reads eng.stream() when it launches: the callers run them under eng.branch(...) contexts."""
from __future__ import annotations

import functools

from typing import Optional

import numpy as np
import torch

from . import _lib as L
from . import packing as P
from .step_state import ListFrontEnd, Saved


def pack_time(eng, items, rows: int, dtype=torch.float32) -> torch.Tensor:
    """(rows, sum n_i) `dtype` on the device, the items side by side along time in the caller's order.  Items: (rows, n_i), (1, rows, n_i)
    or, rows 1, (n_i,) -- host arrays, CPU or device tensors, mixed: the host items go up in ONE upload, the device items join by one cat."""
    dev, flat = eng.device, (lambda t: t[0] if t.dim() == 3 else t)       # (cat along the last axis: no view per item)
    on_dev = [torch.is_tensor(c) and c.is_cuda for c in items]
    parts = [flat(c.to(dev, dtype)) if d else None for c, d in zip(items, on_dev)]
    host = [i for i, d in enumerate(on_dev) if not d]
    if host:
        up = torch.cat([flat(torch.as_tensor(items[i]).to(dtype)) for i in host], dim=-1).to(dev)
        if len(host) == len(items):
            return up.contiguous().reshape(rows, -1)
        at = 0
        for i in host:
            n = int(items[i].shape[-1])
            parts[i] = up[..., at:at + n]
            at += n
    return torch.cat(parts, dim=-1).contiguous().reshape(rows, -1)


_ENCODER_CONVS = [(f"encoder.net.{i}.conv", 1) for i in range(len(P.ENCODER_BLOCKS))] + [("encoder.lin", 0)]


def encoder_convs(eng) -> list:
    """[(parameter name, relu)] of the encoder's layers: the blocks, then lin.  Built once: every engine's encoder has these blocks."""
    return _ENCODER_CONVS


def conv_list(eng, x, y, table, ly, wname, bname, ci, co, conv, what):
    """THE wae_enc_conv_fwd_list call: x -> y through the weight `wname` (bias `bname` or None) of the effective arena, on the segment
    and tile records of the layer record ly in the device table.  conv = (k, stride, pad, relu, res)."""
    lay = eng.lay
    L.check(eng.lib.wae_enc_conv_fwd_list(L.ptr(x), L.ptr(eng.eff[lay.off(wname):]), L.ptr(eng.eff[lay.off(bname):]) if bname else None,
                                          L.ptr(y), L.ptr(table[ly.seg_off:]), ly.nsegs, L.ptr(table[ly.tile_off:]), ly.ntiles, ly.et,
                                          ly.in_pitch, ly.out_pitch, ci, co, *conv, eng.stream()), what)


def enc_list_chain(eng, x, plan, table, keep: bool):
    """The encoder on the packed (c_in, sum F_i) input x: one list launch per layer of plan (packing.encode_list_plan) on the device
    table.  keep=False (nothing is saved for a backward): two ping-pong (width, sum F_i) buffers carry the blocks; keep=True: every
    layer writes a fresh (co, out_pitch) tensor.  -> (lat (Cc, sum Tq_i), acts: None | [the packed input of every layer])."""
    g, dev = eng.g, eng.device
    convs = encoder_convs(eng)
    acts = [x]
    if not keep:
        width = max(eng.lay.shapes[name + ".weight"][0] for name, relu in convs if relu)
        pong = [torch.empty(width * plan.total_F, dtype=torch.float32, device=dev) for _ in range(2)]
        lat = torch.empty(g.Cc, plan.total_Tq, dtype=torch.float32, device=dev)
    for i, ((name, relu), ly) in enumerate(zip(convs, plan.layers)):
        co, ci = eng.lay.shapes[name + ".weight"][:2]
        if keep:
            y = torch.empty(co, ly.out_pitch, dtype=torch.float32, device=dev)
        else:
            y = pong[i & 1] if relu else lat
        res = int(bool(relu) and ly.stride == 1 and ci == co)
        conv_list(eng, x, y, table, ly, name + ".weight", name + ".bias", ci, co, (ly.k, ly.stride, ly.pad, relu, res), "enc_conv_fwd_list")
        x = y
        acts.append(y)
    return acts.pop(), (acts if keep else None)


def ups_list_chain(eng, x, plan, table, out, out_rows: int, act: int):
    """The upsampling network on the packed (Cc, sum Tc_i) input x: the launches of plan (packing.upsample_list_plan) on the device
    table -- conv_in, the stages (the activation launch behind each), the last stage or wae_to_btc_list into the time-major `out` of
    out_rows rows.  -> (the tensors the launches read by raw pointer, [conv_in's input | None, every stage's input])."""
    g, lib, dev = eng.g, eng.lib, eng.device
    keep, ups, stage = [table, x], [x if g.conv_in else None], 0
    for ln in plan.launches:
        if ln.kind == "conv_in":
            y = torch.empty(g.Cc, ln.out_pitch, dtype=torch.float32, device=dev)
            conv_list(eng, x, y, table, ln, "wavenet.upsample_net.conv_in.weight", None, g.Cc, g.Cc, (ln.s, 1, 0, 0, 0), "conv_in (list)")
        elif ln.kind == "to_btc":
            y = out
            L.check(lib.wae_to_btc_list(L.ptr(x), L.ptr(out), L.ptr(table[ln.seg_off:]), ln.nsegs, ln.ntiles, ln.in_pitch, g.Cc,
                                        g.Ccp, eng.dt, eng.stream()), "to_btc_list (c_up)")
        else:
            assert ln.kind in ("stage", "last"), ln.kind
            last = ln.kind == "last"
            ups.append(x)
            w = eng.eff[eng.lay.off(P.up_stage_name(g, stage) + ".weight_v"):]
            stage += 1
            y = out if last else torch.empty(g.Cc, ln.out_pitch, dtype=torch.float32, device=dev)
            L.check(lib.wae_upsample_stage_fwd_list(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(table[ln.seg_off:]), ln.nsegs, ln.ntiles,
                                                    ln.in_pitch, out_rows if last else ln.out_pitch, g.Cc, ln.s, int(last),
                                                    g.Ccp, eng.dt, eng.stream()), "upsample_stage (list)")
            if act:
                L.check(lib.wae_act_fwd(L.ptr(y), y.numel(), act, float(g.up_act_slope), eng.stream()), "upsample activation")
        if y is not out:
            keep.append(y)
        x = y
    return keep, ups


def encoder_forward(eng, c: torch.Tensor, save: Optional[Saved] = None) -> torch.Tensor:
    lib, st = eng.lib, eng.stream()
    x = c.contiguous().float()
    B, acts = x.shape[0], [x]
    for (name, relu), (k, s) in zip(encoder_convs(eng), list(P.ENCODER_BLOCKS) + [(1, 1)]):      # the blocks, then lin as a 1-tap conv
        co, ci = eng.lay.shapes[name + ".weight"][:2]
        Tin = x.shape[-1]
        y = torch.empty(B, co, (Tin + 2 * (k // 2) - k) // s + 1, dtype=torch.float32, device=eng.device)
        L.check(lib.wae_enc_conv_fwd(L.ptr(x), L.ptr(eng.eff[eng.lay.off(name + ".weight"):]), L.ptr(eng.eff[eng.lay.off(name + ".bias"):]),
                                     L.ptr(y), B, ci, Tin, co, k, s, k // 2, relu, int(bool(relu) and s == 1 and ci == co), st), name)
        x = y
        acts.append(x)
    lat = acts.pop()
    if save is not None:
        save.enc_acts = acts       # inputs of every block (+ the last block's output): backward needs them
    return lat


def vq_forward(eng, lat: torch.Tensor, beta: float = 0.25, update: bool = False):
    g = eng.g
    if g.vq != "plain":
        return _vq_forward_slices(eng, lat, float(beta), bool(update))
    B, D, Tq = lat.shape
    idx = torch.empty(B * Tq, dtype=torch.int64, device=eng.device)
    quant = torch.empty_like(lat)
    stats = torch.empty(2, dtype=torch.float32, device=eng.device)
    hist = eng._vq_hist = torch.empty(g.K + 1, dtype=torch.int32, device=eng.device)
    L.check(eng.lib.wae_vq_nearest(L.ptr(lat), L.ptr(eng.eff[eng.lay.off("vq.embedding.weight"):]), L.ptr(idx),
                                   L.ptr(quant), L.ptr(stats), L.ptr(hist), B, D, Tq, g.K, beta, eng.stream()), "vq_nearest")
    if eng.opt.deterministic:      # stats[0] again, from a fixed-order sum (the search adds its squared errors by float atomics)
        L.check(eng.lib.wae_vq_loss_det(L.ptr(lat), L.ptr(quant), L.ptr(stats), B, D, 0, D, Tq, beta + 1.0, eng.stream()), "vq_loss_det")
    return quant, idx, stats


def vq_slice_records(eng, beta: float):
    hit = eng._vq_recs.get(beta)
    if hit is None:
        g = eng.g
        c_loss = P.vq_coeffs(g, beta)[0]
        specs = [(name + ".weight", d0, D, K, c_loss * D / g.Cc) for name, d0, D, K in P.vq_slice_specs(g)]
        recs = (L.VqSliceRec * len(specs))(*[L.VqSliceRec(eng.eff.data_ptr() + 4 * eng.lay.off(name), d0, D, K, cl) for name, d0, D, K, cl in specs])
        words = int(eng.lib.wae_vq_search_slices_scratch(recs, len(specs)))
        if words < 1:
            raise L.WaeError(f"vq_search_slices_scratch: {eng.lib.wae_last_error().decode()}")
        hit = eng._vq_recs[beta] = (recs, specs, words)
    return hit


def _vq_forward_slices(eng, lat: torch.Tensor, beta: float, update: bool):
    """vq_forward of the sliced / EMA kinds: ONE wae_vq_search_slices call for all slices (two around the codebook update)."""
    g, lib, st, dev = eng.g, eng.lib, eng.stream(), eng.device
    B, D, Tq = lat.shape
    recs, specs, words = vq_slice_records(eng, beta)
    n, idx = len(specs), torch.empty(len(specs), B * Tq, dtype=torch.int64, device=dev)
    quant = torch.empty_like(lat)
    stats = torch.empty(n, 2, dtype=torch.float32, device=dev)
    scratch = eng._vq_hist = torch.empty(words, dtype=torch.int32, device=dev)
    call = lambda mode: L.check(lib.wae_vq_search_slices(L.ptr(lat), recs, n, L.ptr(idx), L.ptr(quant), L.ptr(stats), L.ptr(scratch),  # noqa: E731
                                                         B, D, Tq, mode, st), "vq_search_slices")
    if update and g.vq_ema:
        call(1)
        hoff = 0
        for s, (name, d0, Ds, K, _) in enumerate(specs):
            sfx = name[len("vq.embedding"):-len(".weight")]
            off = eng.lay.off(name)
            L.check(lib.wae_vq_ema_update(L.ptr(lat), L.ptr(idx[s]), L.ptr(scratch[hoff:]), L.ptr(eng.vq_buffers["vq.ema_cluster_size" + sfx]),
                                          L.ptr(eng.vq_buffers["vq.ema_w" + sfx]), L.ptr(eng.eff[off:]), B, D, d0, Ds, Tq, K,
                                          float(g.vq_decay), st), "vq_ema_update")
            # the codebook moved where the search reads it (the effective arena); the parameters are what state_dict, the next
            # weight norm pass and the optimizer read
            eng.params[off:off + K * Ds].copy_(eng.eff[off:off + K * Ds])
            hoff += K
        call(2)
    else:
        call(0)
    if eng.opt.deterministic:      # every slice's stats[0] again, from a fixed-order sum
        for s, (_, d0, Ds, _, cl) in enumerate(specs):
            L.check(lib.wae_vq_loss_det(L.ptr(lat), L.ptr(quant), L.ptr(stats[s]), B, D, d0, Ds, Tq, cl, st), "vq_loss_det")
    if g.vq_n == 1:
        return quant, idx[0], stats[0]
    tot = stats[0]
    for s in range(1, n):      # in slice order (element-wise adds: the same bits wherever the same slices' numbers are added)
        tot = tot + stats[s]
    return quant, idx, tot


def upsample_forward(eng, c: torch.Tensor, out: torch.Tensor, save: Optional[Saved] = None):
    g, lib, st = eng.g, eng.lib, eng.stream()
    B, Cc, Tc = c.shape
    c = c.contiguous()
    n, trim = len(g.upsample_scales), 0
    act = P.UP_ACT_KINDS.get(g.up_act, 0)          # upsample_activation behind every stage (upsample.py:44-46), 0 = none
    if g.conv_in:
        kin = 2 * g.cin_pad + 1
        Tin = Tc - 2 * g.cin_pad
        x = torch.empty(B, Cc, Tin, dtype=torch.float32, device=eng.device)
        L.check(lib.wae_enc_conv_fwd(L.ptr(c), L.ptr(eng.eff[eng.lay.off("wavenet.upsample_net.conv_in.weight"):]),
                                     None, L.ptr(x), B, Cc, Tc, Cc, kin, 1, 0, 0, 0, st), "conv_in")
        acts = [c, x]          # conv_in input, then every stage's input
    else:
        x, Tin = c, Tc
        trim = g.cin_pad * int(np.prod(g.upsample_scales))
        acts = [None, x]
    for i, s in enumerate(g.upsample_scales):
        w = eng.eff[eng.lay.off(P.up_stage_name(g, i) + ".weight_v"):]
        last = i == n - 1 and trim == 0 and not act    # the last stage writes the time-major operand itself, unless something follows
        assert not last or out.shape[1] == Tin * s, (out.shape, Tin * s)
        y = out if last else torch.empty(B, Cc, Tin * s, dtype=torch.float32, device=eng.device)
        L.check(lib.wae_upsample_stage_fwd(L.ptr(x), L.ptr(w), L.ptr(y), B, Cc, Tin, s, int(last), g.Ccp, eng.dt, st), "upsample_stage")
        x, Tin = y, Tin * s
        if act:
            L.check(lib.wae_act_fwd(L.ptr(x), x.numel(), act, float(g.up_act_slope), st), "upsample activation")
        if i < n - 1:
            acts.append(x)
    xt = None
    if trim or act:       # upsample.py:64-65: c[:, :, indent:-indent]
        assert out.shape[1] == Tin - 2 * trim, (out.shape, Tin, trim)
        xt = x[:, :, trim:Tin - trim].contiguous() if trim else x
        L.check(lib.wae_to_btc(L.ptr(xt), L.ptr(out), B, Cc, Tin - 2 * trim, g.Ccp, eng.dt, st), "to_btc (c_up)")
    if save is not None:
        save.up_acts, save.up_last, save.up_keep = acts, (x if act else None), xt
    return out


def encode_list(eng, feats, want_latents, want_idx, max_frames, beta):
    """encode_list (beta None) / encode_list_stats: the checks, the groups, the per-list arrays of the statistics"""
    from .train import list_items
    g, want_stats = eng.g, beta is not None
    if not g.has_encoder:
        raise ValueError("encode_list: this engine has no encoder (a decoder-only geometry: c_in is None)")
    _, Fs, feats, _ = list_items("encode_list", list(feats), g, "feats")
    cap = P.ENC_LIST_MAX_FRAMES if max_frames is None else int(max_frames)
    if cap < 1:
        raise ValueError(f"encode_list: max_frames {cap} < 1")
    if eng.weights_dirty:
        eng.prepare_weights()
    out, stats = [], None
    if want_stats:
        specs = [("vq.embedding.weight", 0, g.Cc, g.K, float(beta) + 1.0)] if g.vq == "plain" else vq_slice_records(eng, float(beta))[1]
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=eng.device)  # noqa: E731
        stats = dict(keep=[], specs=specs, slices=[dict(sqerr=z(len(feats)), hist=z(len(feats), K, dt=torch.int32), item=z(len(feats), 2),
                                                        out=z(4)) for _, _, _, K, _ in specs])
    for lo, hi in P.encode_list_groups(Fs, cap):
        out += _encode_group(eng, feats[lo:hi], want_latents, want_idx, stats, lo)
    if want_stats:
        _vq_list_stats_close(eng, stats)
        eng.last_list_stats = stats["out"]
        eng.hold("encode_list_stats", *stats["keep"])       # the tables passed by raw pointer, until the next list
        # the items' views by four unbind calls for the whole list: indexing per item cost more than the kernels (about 10 us an item)
        cols = (stats["sqerr"].unbind(0), stats["item"][:, 0].unbind(0), stats["item"][:, 1].unbind(0), stats["hist"].unbind(0))
        for r, sq, vq, pp, h in zip(out, *cols):
            r.update(sqerr=sq, vq_loss=vq, perp=pp, hist=h)
    return out


def _encode_group(eng, feats, want_latents, want_idx, stats=None, first=0):
    """one group of encode_list: pack, eleven list launches, one quantiser call; stats: encode_list's per-list arrays, whose
    entries first .. first + n - 1 this group fills with one more call per slice"""
    g, plan = eng.g, P.encode_list_plan([f.shape[1] for f in feats])
    tab, vq_off = plan.table, plan.table.size
    if stats is not None:
        # the statistics' records ride behind the layers' in the one upload: a copy of their own behind the quantiser's call would
        # make the host wait for the group's launches and the groups stop overlapping (0.4 ms a group)
        tab = np.concatenate([tab, P.vq_seg_table(plan.q_offsets, plan.Tq).reshape(-1)])
    x, table = pack_time(eng, feats, g.c_in), torch.from_numpy(tab).to(eng.device)
    lat = enc_list_chain(eng, x, plan, table, keep=False)[0]
    # the quantiser on the packed latents as ONE clip of sum Tq_i frames: rows are per frame, so idx and quant are per utterance
    # what vq_forward gives it alone; stats would be the list's aggregate and are not returned
    quant, idx, _ = vq_forward(eng, lat.view(1, g.Cc, plan.total_Tq))
    quant = quant[0]
    sl = [slice(int(o), int(o + t)) for o, t in zip(plan.q_offsets, plan.Tq)]
    res = [dict(quant=quant[:, s], idx=idx[..., s] if want_idx else None, latents=lat[:, s] if want_latents else None) for s in sl]
    if stats is not None:       # one call per slice, on the slice's rows of the packed arrays
        for s, ((_, d0, Ds, K, cl), a) in enumerate(zip(stats["specs"], stats["slices"])):
            L.check(eng.lib.wae_vq_stats_segments(L.ptr(lat[d0:]), L.ptr(quant[d0:]), L.ptr(idx[s] if idx.dim() == 2 else idx),
                                                  L.ptr(table[vq_off:]), len(feats), Ds, plan.total_Tq, K, cl, first, L.ptr(a["sqerr"]),
                                                  L.ptr(a["hist"]), L.ptr(a["item"]), L.ptr(a["out"]), eng.stream()), "vq_stats_segments")
        stats["keep"].append(table)
    return res


# the list statistics: wae_vq_stats_segments once per SLICE and group, on the slice's rows of the packed arrays (pointer offset
# d0 * pitch, D = D_s, the slice's idx row and K_s) with c_loss_s = c_loss * D_s / Dtot, so an item's vq_loss_s is
# c_loss sqerr_s / (Tq_i Dtot); the plain quantiser is the one slice of all Cc rows with c_loss = beta + 1.  Per item and for the list:
# vq_loss, perp and sqerr are the slices' numbers added in slice order, hist (n, max K_s) the slices' counts side by side, zero beyond K_s.
def _vq_list_stats_close(eng, stats):
    sl = stats["slices"]
    add = lambda key: functools.reduce(lambda x, y: x + y, [a[key] for a in sl])      # noqa: E731  (in slice order)
    stats["sqerr"], stats["item"] = add("sqerr"), add("item")
    out = stats["out"] = add("out")
    if len(sl) > 1:
        out[2] = sl[0]["out"][2]       # sum Tq: every slice counted the same frames
    hist = stats["hist"] = sl[0]["hist"]
    if eng.g.vq_n > 1:
        hist = stats["hist"] = torch.zeros(hist.shape[0], len(sl), max(a["hist"].shape[1] for a in sl), dtype=torch.int32, device=eng.device)
        for s, a in enumerate(sl):
            hist[:, s, :a["hist"].shape[1]] = a["hist"]


def upsample_list(eng, cs, out=None, offsets=None, c_is_upsampled=False, max_samples=None):
    g, dev, cs = eng.g, eng.device, list(cs)
    if not cs:
        raise ValueError("upsample_list: an empty list")
    if g.Cc <= 0:
        raise ValueError("upsample_list: this engine has no local conditioning (Cc <= 0)")
    Tcs = []
    for i, c in enumerate(cs):
        shape = tuple(getattr(c, "shape", ()))
        if len(shape) == 3 and shape[0] == 1:
            shape = shape[1:]
        if len(shape) != 2 or shape[0] != g.Cc:
            raise ValueError(f"upsample_list: item {i} has shape {tuple(getattr(c, 'shape', ()))}; every item is (Cc, Tc) or "
                             f"(1, Cc, Tc) with Cc = {g.Cc}")
        Tcs.append(int(shape[1]))
    cap = P.UPS_LIST_MAX_SAMPLES if max_samples is None else int(max_samples)
    if cap < 1:
        raise ValueError(f"upsample_list: max_samples {cap} < 1")
    whole = P.upsample_list_plan(Tcs, g, offsets, c_is_upsampled)       # the lengths, the rows and their refusals; not launched
    Ts, offs = [int(t) for t in whole.Ts], [int(o) for o in whole.offsets]
    if out is None:
        out = torch.empty(whole.rows, g.Ccp, dtype=eng.tdtype, device=dev)
    elif (out.dim() != 2 or out.shape[1] != g.Ccp or out.dtype != eng.tdtype or not out.is_contiguous() or not out.is_cuda
          or out.shape[0] < whole.rows):
        raise ValueError(f"upsample_list: out is {tuple(out.shape)} {out.dtype}; the items need a contiguous ({whole.rows}+, {g.Ccp}) "
                         f"{eng.tdtype} operand on {dev}")
    if eng.weights_dirty:
        eng.prepare_weights()
    if not P.upsample_list_supported(g, c_is_upsampled):
        for i, c in enumerate(cs):
            ci = torch.as_tensor(c).to(dev, torch.float32).reshape(1, g.Cc, Tcs[i]).contiguous()
            eng._ar_cond_rows(ci, out[offs[i]:offs[i] + Ts[i]].view(1, Ts[i], g.Ccp), c_is_upsampled, f"item {i}: ")
        return out, whole.offsets
    keep, groups = [], P.upsample_list_groups(Ts, cap)
    act = 0 if c_is_upsampled else P.UP_ACT_KINDS.get(g.up_act, 0)
    for lo, hi in groups:
        # one group: pack, one table, the chain's launches
        plan = whole if len(groups) == 1 else P.upsample_list_plan(Tcs[lo:hi], g, offs[lo:hi], c_is_upsampled)
        x = pack_time(eng, cs[lo:hi], g.Cc)
        keep += ups_list_chain(eng, x, plan, torch.from_numpy(plan.table).to(dev), out, out.shape[0], act)[0]
    eng.hold("upsample_list", *keep)       # the tables and intermediates, passed by raw pointer, until the next list
    return out, whole.offsets


def train_list_front(eng, tp, cs, beta):
    """The front half of a ragged step's train-mode forward (train.train_step_list; tp: packing.train_list_plan): the list front end,
    every layer's packed input kept for the backward (Saved.list_fe), into the zero-filled conditioning operand of the
    (B, Tmax, train) workspace.  -> (the forward's record, the quantiser's stats | None without an encoder)."""
    g, dev, B, T = eng.g, eng.device, tp.B, tp.Tmax
    sv = Saved(B, T)
    t_enc = torch.from_numpy(tp.enc.table).to(dev) if tp.enc is not None else None
    t_ups, t_bwd = torch.from_numpy(tp.ups.table).to(dev), torch.from_numpy(tp.bwd_table).to(dev)
    fe = sv.list_fe = ListFrontEnd(plan=tp, tables=(t_enc, t_ups, t_bwd))
    stats = None
    if g.has_encoder:
        lat, fe.enc_acts = enc_list_chain(eng, pack_time(eng, cs, g.c_in), tp.enc, t_enc, keep=True)
        lat = lat.view(1, g.Cc, tp.enc.total_Tq)       # no gap columns: the quantiser's mean is over Cc * sum Tq_i
        quant, idx, stats = vq_forward(eng, lat, beta, update=True)
        sv.lat, sv.quant, sv.idx, sv.beta = lat, quant, idx, beta
        xc = quant[0]
    else:
        xc = pack_time(eng, cs, g.Cc)
    c_up = eng.workspace(B, T, True)["c_up"]
    c_up.zero_()                              # the pad rows of every item: what the padded decoder reads there, and zero gradient back
    fe.up_acts = ups_list_chain(eng, xc, tp.ups, t_ups, c_up, B * T, 0)[1]
    return sv, stats
