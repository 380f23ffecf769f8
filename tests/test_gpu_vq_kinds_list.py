"""The sliced and EMA quantisers on the list and session paths: every item of encode_list, encode_list_stats, score_list and
forward_list is bit for bit the dense call on the utterance alone, for every order and grouping; session chunks concatenate to
encode_list's bytes and drive a decode session to incremental_forward's; one wae_vq_search_slices call per group / per feed_list
whatever the slices and the items, and one wae_vq_stats_segments call per slice."""
import functools

import numpy as np
import pytest
import torch

import vq_cases as V
from wavenet_autoencoders_amd import packing as P

pytestmark = pytest.mark.gpu

FS = (1, 5, 16, 17, 40)                              # feature frames: 1, 2, 4, 5 and 10 latent frames
ORDERS = ((0, 1, 2, 3, 4), (4, 2, 0, 3, 1))
GROUPINGS = (None, 24)                               # max_frames: one group; 40 | 16 + 5 + 1 ... by the caller's order
KINDS = sorted(V.LIST_KINDS)
HOP = 640


@functools.lru_cache(maxsize=None)
def _setup(kind, dtype="fp32"):
    """engine, the utterances and, per utterance, the dense calls' answer on it alone -- once per kind, left unchanged"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, _, _ = V.model_case(V.LIST_KINDS[kind])
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd)
    eng.prepare_weights()
    gen = torch.Generator().manual_seed(7)
    feats = [torch.randn(cfg["c_in"], F, generator=gen) * 1.7 for F in FS]
    xs = [torch.randint(0, cfg["O"], ((F + 3) // 4 * HOP,), generator=gen) for F in FS]
    alone = []
    for f in feats:
        lat = eng.encoder_forward(f[None].cuda())
        quant, idx, stats = eng.vq_forward(lat, V.BETA)
        n = len(V.slice_specs(cfg))
        assert tuple(idx.shape) == (n, lat.shape[-1])
        alone.append(dict(latents=lat[0].clone(), quant=quant[0].clone(), idx=idx.clone(), vq_loss=stats[0].clone(), perp=stats[1].clone()))
    torch.cuda.synchronize()
    return eng, cfg, feats, xs, alone


def _check_item(cfg, r, want, stats=False):
    assert torch.equal(r["quant"], want["quant"]) and torch.equal(r["idx"], want["idx"])
    if r.get("latents") is not None:
        assert torch.equal(r["latents"], want["latents"])
    if stats:
        assert torch.equal(r["perp"], want["perp"])
        vq, perp, hist, sq = V.list_stats_f64(cfg, want["latents"].cpu().numpy(), want["quant"].cpu().numpy(), want["idx"].cpu().numpy())
        assert tuple(r["hist"].shape) == hist.shape and r["hist"].dtype == torch.int32 and np.array_equal(r["hist"].cpu().numpy(), hist)
        # fp32 rounding: per slice the fp64 sum rounded once, a division and a product, then the slices added -- at most 8 roundings
        assert abs(float(r["vq_loss"]) - vq) <= 8 * 2.0 ** -24 * vq
        assert abs(float(r["sqerr"]) - sum(sq)) <= 8 * 2.0 ** -24 * sum(sq)
        assert abs(float(r["vq_loss"]) - float(want["vq_loss"])) <= 1e-5 * vq      # the dense call's loss: float atomics


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_list_items_are_bitwise_the_utterance_alone(kind, dtype):
    eng, cfg, feats, xs, alone = _setup(kind, dtype)
    specs = V.slice_specs(cfg)
    seen_vq, seen_tot = {}, []
    for order in ORDERS:
        for cap in GROUPINGS:
            fl = [feats[i] for i in order]
            for r, i in zip(eng.encode_list(fl, want_latents=True, max_frames=cap), order):
                _check_item(cfg, r, alone[i])
            res = eng.encode_list_stats(fl, beta=V.BETA, want_latents=True, max_frames=cap)
            tot = eng.last_list_stats.clone()
            for r, i in zip(res, order):
                _check_item(cfg, r, alone[i], stats=True)
                seen_vq.setdefault(i, r["vq_loss"].clone())
                assert torch.equal(r["vq_loss"], seen_vq[i])              # bitwise across orders and groupings
            # the list as one batch: packing.vq_list_totals per slice, added over the slices
            want_vq = want_perp = 0.0
            for s, (_, d0, D, K) in enumerate(specs):
                sq = [V.list_stats_f64(cfg, alone[i]["latents"].cpu().numpy(), alone[i]["quant"].cpu().numpy(),
                                       alone[i]["idx"].cpu().numpy())[3][s] for i in order]
                hist = np.stack([r["hist"].cpu().numpy()[s, :K] for r in res])
                vq_s, perp_s, frames, _ = P.vq_list_totals(sq, hist, D, V.coeffs(cfg["vq"])[0] * D / cfg["Cc"])
                want_vq, want_perp = want_vq + vq_s, want_perp + perp_s
            assert frames == 22 == int(tot[2])
            assert abs(float(tot[0]) - want_vq) <= 1e-6 * want_vq and abs(float(tot[1]) - want_perp) <= 1e-5 * want_perp
            seen_tot.append((cap, tot))
    # the totals of one order do not depend on the grouping (the squared errors are added in list order)
    assert torch.equal(seen_tot[0][1], seen_tot[1][1]) and torch.equal(seen_tot[2][1], seen_tot[3][1])
    # forward_list and score_list: the same items behind the decoder
    for order in ORDERS:
        items = [dict(x=xs[i], feats=feats[i], gid=i % 5) for i in order]
        res, loss = eng.forward_list(items, want_stats=True, beta=V.BETA)
        for r, i in zip(res, order):
            _check_item(cfg, r, alone[i], stats=False)
            assert torch.equal(r["perp"], alone[i]["perp"]) and torch.equal(r["vq_loss"], seen_vq[i])
        sres, totals = eng.score_list(items, beta=V.BETA)
        for r, i in zip(sres, order):
            assert torch.equal(r["quant"], alone[i]["quant"]) and torch.equal(r["idx"], alone[i]["idx"])
            assert torch.equal(r["perp"], alone[i]["perp"]) and torch.equal(r["vq_loss"], seen_vq[i])
        assert torch.equal(totals["vq_loss"], eng.last_list_stats[0]) and float(totals["frames"]) == 22
        assert torch.equal(totals["loss"], totals["ce"] + totals["vq_loss"])
    # one utterance through the dense forward: the list's logits are its bytes
    i = 1
    dense = eng.forward(xs[i][None].cuda(), feats[i][None].cuda(), torch.tensor([i % 5]).cuda(), targets=xs[i][None].cuda(), beta=V.BETA)
    res, _ = eng.forward_list([dict(x=xs[j], feats=feats[j], gid=j % 5) for j in (0, 1, 2)])
    assert torch.equal(res[1]["logits"], dense["logits"][0]) and torch.equal(res[1]["idx"], dense["idx"])


def _feeds(name, F):
    if name == "irregular":
        out, k = [], 0
        while sum(out) < F:
            out.append(min((3, 1, 7, 2, 11)[k % 5], F - sum(out)))
            k += 1
        return out
    n = int(name)
    return [n] * (F // n) + ([F % n] if F % n else [])


@pytest.mark.parametrize("window", [None, 32])
@pytest.mark.parametrize("sizes", ["1", "4", "irregular"])
@pytest.mark.parametrize("kind", KINDS)
def test_session_chunks_are_encode_list_of_the_whole_utterance(kind, sizes, window):
    eng, cfg, feats, _, alone = _setup(kind)
    plans = [_feeds(sizes, F) for F in FS]
    got = [dict(quant=[], idx=[], latents=[]) for _ in FS]
    with eng.encode_session(want_latents=True, window=window) as sess:
        hs = [sess.open() for _ in FS]
        fed = [0] * len(FS)
        for r in range(max(len(p) for p in plans)):
            feeds, ends = {}, []
            for i, p in enumerate(plans):
                if r < len(p):
                    feeds[hs[i]] = feats[i][:, fed[i]:fed[i] + p[r]]
                    fed[i] += p[r]
                    if r == len(p) - 1:
                        ends.append(hs[i])
            res = sess.feed_list(feeds, ended=ends)
            for i in range(len(FS)):
                out = res.get(hs[i])
                if out is not None:
                    assert out["idx"].shape == (len(V.slice_specs(cfg)), out["quant"].shape[1])
                    for key in got[i]:
                        got[i][key].append(out[key].clone())
    for i, want in enumerate(alone):
        for key in ("quant", "latents", "idx"):
            assert torch.equal(torch.cat(got[i][key], dim=1), want[key]), (FS[i], key)


def test_fed_features_decode_as_the_whole_clip(monkeypatch):
    """an encode session of a sliced quantiser drives a decode session (slots) to the bytes of incremental_forward on the whole clip"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    monkeypatch.setenv("WAE_AR_COOP", "0")
    cfg, sd, _, _ = V.model_case(V.LIST_KINDS["sliced2"])
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    gen = torch.Generator().manual_seed(23)
    F = 21
    Lq = (F + 3) // 4
    T = Lq * HOP
    feats = torch.randn(cfg["c_in"], F, generator=gen) * 1.7
    uni = torch.rand(T, generator=gen).cuda()
    quant = eng.encode_list([feats])[0]["quant"].contiguous()
    want = eng.incremental_forward(quant[None], torch.tensor([3]).cuda(), T, mode="sample", init_idx=31, uniforms=uni[None])["idx"][0].clone()
    parts, got = [], 0
    with eng.encode_session() as enc, eng.decode_session(mode="sample", coop=False, slots=2) as dec:
        e, h = enc.open(), dec.open(dict(gid=3, init_idx=31))
        for lo, hi, end in ((0, 9, False), (9, 21, False), (21, 21, True)):
            res = enc.end(e) if end else enc.feed(e, feats[:, lo:hi])
            n = res["quant"].shape[1]
            if n:
                dec.feed_list({h: res["quant"]}, uniforms={h: uni[got * HOP:(got + n) * HOP]})
                got += n
            if res["done"]:
                dec.end(h)
            while True:
                out = dec.step(1500).get(h)
                if out is None:
                    break
                parts.append(out["idx"].clone())
                if out["done"]:
                    break
    assert got == Lq and torch.equal(torch.cat(parts), want)


def test_one_search_call_per_group_and_per_feed():
    """exactly one wae_vq_search_slices call per group / per feed_list, for 2 and 4 slices and for 3 and 12 items alike; one
    wae_vq_stats_segments call per slice and group; no per-slice search entry"""
    counts = {}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            counts[name] = counts.get(name, 0) + 1
            return getattr(self._lib, name)

    VQ = ("wae_vq_search_slices", "wae_vq_stats_segments", "wae_vq_slice", "wae_vq_nearest")
    gen = torch.Generator().manual_seed(11)
    seen = {}
    for kind, n in (("sliced2", 2), ("sliced4", 4)):
        eng, cfg, _, _, _ = _setup(kind)
        real = eng.lib
        try:
            for items in (3, 12):
                fl = [torch.randn(cfg["c_in"], 5 + (7 * i) % 13, generator=gen).cuda() for i in range(items)]
                eng.lib = Counting(real)
                counts.clear()
                eng.encode_list(fl)
                a = {k: counts.get(k, 0) for k in VQ}
                counts.clear()
                eng.encode_list_stats(fl, beta=V.BETA)
                b = {k: counts.get(k, 0) for k in VQ}
                counts.clear()
                eng.encode_list_stats(fl, beta=V.BETA, max_frames=12)
                groups = len(P.encode_list_groups([f.shape[1] for f in fl], 12))
                c = {k: counts.get(k, 0) for k in VQ}
                eng.lib = real
                with eng.encode_session() as sess:
                    hs = [sess.open() for _ in fl]
                    sess.feed_list({h: f[:, :3] for h, f in zip(hs, fl)})
                    eng.lib = Counting(real)
                    counts.clear()
                    sess.feed_list({h: f[:, 3:] for h, f in zip(hs, fl)}, ended=hs)
                    d = {k: counts.get(k, 0) for k in VQ}
                    eng.lib = real
                assert a == dict(zip(VQ, (1, 0, 0, 0))) and b == dict(zip(VQ, (1, n, 0, 0))) and d == dict(zip(VQ, (1, 0, 0, 0)))
                assert groups > 1 and c == dict(zip(VQ, (groups, n * groups, 0, 0)))
                seen[(kind, items)] = (a, d)
        finally:
            eng.lib = real
    assert len({str(v) for v in seen.values()}) == 1
