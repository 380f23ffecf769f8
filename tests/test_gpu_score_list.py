"""List scoring in full on the GPU: wae_vq_stats_segments through raw ctypes (exact histograms, fixed-order squared errors against
float64, the perplexity bit for bit the dense search's, untouched neighbours, skipped records, determinism, groups), the engine's
encode_list_stats / score_list against the utterances alone, the mixture losses of scalar-input decoders over a list, and
vqwae_train.evaluate(packed=True) with the quantiser's numbers."""
import math
import types

import numpy as np
import pytest
import torch

from helpers import golden_model
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -2
TQS = [1, 2, 63, 64, 65, 255, 256, 257, 700]       # the wave, workgroup and stride edges
ONE_CODE, EXACT = 3, 5                             # the item that uses one code; the item whose quant equals its latents
SENTINEL, ISENTINEL = 7.0, -77
C_LOSS = 1.25
U24 = 2.0 ** -24


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------- the kernel
class Packed:
    """Packed latents of nine items with gaps between some, their indices and quantised twins.  The codes differ in channel 0 alone
    (a grid of spacing 1/4 around 0) and the latents are the codes plus a tenth of the spacing of noise: the dense search finds exactly
    `idx` again, which the per-item reference (the search entry, mode 1) needs.  Every array carries a margin in front and behind --
    NaN for the floats, so that a read outside an item's columns poisons its sum -- and so do the gaps: no table of these tests, the
    out-of-contract ones included, could take even a wrong kernel outside an allocation."""
    MARGIN = 1024

    def __init__(self, D, K, seed=0):
        from wavenet_autoencoders_amd import _lib as L
        self.L, self.lib, self.D, self.K = L, L.lib(), D, K
        gen = torch.Generator().manual_seed(4000 + 131 * D + K + seed)
        M, s = self.MARGIN, 0.25
        self.offs, at = [], 3
        for i, T in enumerate(TQS):
            self.offs.append(at)
            at += T + (i % 3) * 5
        self.pitch = pitch = at + 4
        emb = torch.zeros(K, D)
        emb[:, 0] = (torch.arange(K) - K // 2).float() * s
        if D > 1:
            emb[:, 1:] = torch.randn(D - 1, generator=gen)[None]
        idx = torch.randint(0, K, (pitch,), generator=gen)
        o = self.offs[ONE_CODE]
        idx[o:o + TQS[ONE_CODE]] = K // 3
        noise = (torch.rand(D, pitch, generator=gen) * 2 - 1) * (s / 10)
        o = self.offs[EXACT]
        noise[:, o:o + TQS[EXACT]] = 0.0
        quant = emb[idx].t().contiguous()
        lat = quant + noise
        owned = torch.zeros(pitch, dtype=torch.bool)
        for o, T in zip(self.offs, TQS):
            owned[o:o + T] = True
        lat[:, ~owned] = float("nan")
        quant[:, ~owned] = float("nan")
        self.emb = emb.cuda()
        self.lat_all = torch.full((2 * M + D * pitch,), float("nan"))
        self.quant_all = torch.full((2 * M + D * pitch,), float("nan"))
        self.lat_all[M:M + D * pitch] = lat.reshape(-1)
        self.quant_all[M:M + D * pitch] = quant.reshape(-1)
        self.lat_all, self.quant_all = self.lat_all.cuda(), self.quant_all.cuda()
        self.idx_all = torch.zeros(2 * M + pitch, dtype=torch.int64)
        self.idx_all[M:M + pitch] = idx
        self.idx_all = self.idx_all.cuda()
        self.lat = self.lat_all[M:M + D * pitch].view(D, pitch)
        self.quant = self.quant_all[M:M + D * pitch].view(D, pitch)
        self.idx = self.idx_all[M:M + pitch]
        self.table = np.stack([self.offs, TQS], axis=1).astype(np.int32)

    def outputs(self, n):
        """sqerr, hist, item_stats of n entries and out, prefilled with the sentinels"""
        return (torch.full((n,), SENTINEL, device="cuda"), torch.full((n, self.K), ISENTINEL, dtype=torch.int32, device="cuda"),
                torch.full((n, 2), SENTINEL, device="cuda"), torch.full((4,), SENTINEL, device="cuda"))

    def call(self, table, outs, first=0, nsegs=None, **kw):
        L = self.L
        tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 2)).cuda()
        a = dict(lat=L.ptr(self.lat), quant=L.ptr(self.quant), idx=L.ptr(self.idx), segs=L.ptr(tab), nsegs=len(tab) if nsegs is None else nsegs,
                 D=self.D, pitch=self.pitch, K=self.K, c_loss=C_LOSS, first=first, sqerr=L.ptr(outs[0]), hist=L.ptr(outs[1]),
                 item_stats=L.ptr(outs[2]), out=L.ptr(outs[3]))
        a.update(kw)
        rc = self.lib.wae_vq_stats_segments(a["lat"], a["quant"], a["idx"], a["segs"], a["nsegs"], a["D"], a["pitch"], a["K"], a["c_loss"],
                                            a["first"], a["sqerr"], a["hist"], a["item_stats"], a["out"], None)
        torch.cuda.synchronize()
        return rc

    def dense_perplexity(self, i):
        """the search entry, mode 1, on item i alone -> (idx it finds, stats[1])"""
        L, D, K = self.L, self.D, self.K
        o, T = self.offs[i], TQS[i]
        lat = self.lat[:, o:o + T].contiguous().view(1, D, T)
        idx = torch.full((T,), -1, dtype=torch.int64, device="cuda")
        stats = torch.full((2,), SENTINEL, device="cuda")
        hist = torch.zeros(K + 1, dtype=torch.int32, device="cuda")
        L.check(self.lib.wae_vq_slice(L.ptr(lat), L.ptr(self.emb), L.ptr(idx), None, L.ptr(stats), L.ptr(hist), 1, D, 0, D, T, K, C_LOSS, 1,
                                      None), "vq_slice")
        torch.cuda.synchronize()
        return idx, stats[1].clone()


def _perplexity64(hist, n):
    p = hist.double() / n
    return float(torch.exp(-(p * torch.log(p + 1e-10)).sum()))


@pytest.mark.parametrize("K", [1, 32, 257, 1000])
@pytest.mark.parametrize("D", [1, 16, 65])
def test_the_kernel_per_item(D, K):
    pk = Packed(D, K)
    n = len(TQS)
    outs = pk.outputs(n + 2)
    pk.L.check(pk.call(pk.table, outs), "vq_stats_segments")
    sqerr, hist, item, out = outs
    # entries behind this call's keep their sentinel
    assert bool((sqerr[n:] == SENTINEL).all()) and bool((hist[n:] == ISENTINEL).all()) and bool((item[n:] == SENTINEL).all())
    ppl_bound = 2 * math.log(max(K, 2)) * (13 + -(-K // 256)) * U24
    for i, (o, T) in enumerate(zip(pk.offs, TQS)):
        ix = pk.idx[o:o + T]
        assert torch.equal(hist[i].long(), torch.bincount(ix, minlength=K)), (D, K, T, "hist")
        ref = float(((pk.quant[:, o:o + T].double() - pk.lat[:, o:o + T].double()) ** 2).sum())
        got = float(sqerr[i])
        print(f"D {D} K {K} Tq {T}: sqerr {got:.9g} (float64 {ref:.9g}, rel {abs(got - ref) / max(ref, 1e-300):.2e})")
        assert abs(got - ref) <= 2.0 ** -23 * ref, (D, K, T, got, ref)            # fp64 accumulation, one rounding to fp32
        vq_ref = C_LOSS * ref / (T * D)
        assert abs(float(item[i, 0]) - vq_ref) <= 8 * U24 * vq_ref, (D, K, T, float(item[i, 0]), vq_ref)
        found, dense = pk.dense_perplexity(i)
        assert torch.equal(found, ix), (D, K, T, "the dense search does not find the indices this test packed")
        assert _same(item[i, 1], dense), (D, K, T, float(item[i, 1]), float(dense))
        p64 = _perplexity64(hist[i], T)
        print(f"D {D} K {K} Tq {T}: perplexity {float(item[i, 1]):.9g} (float64 {p64:.9g}, bound {ppl_bound:.2e})")
        assert abs(float(item[i, 1]) - p64) <= ppl_bound * p64, (D, K, T, float(item[i, 1]), p64)
    assert float(item[ONE_CODE, 1]) == 1.0                     # one code: p = 1, log 1 = 0, exp(-0) = 1
    assert float(sqerr[EXACT]) == 0.0 and float(item[EXACT, 0]) == 0.0
    # the list as one batch, against float64 of the per-item results
    from wavenet_autoencoders_amd import packing as P
    vq, perp, frames, tot = P.vq_list_totals(sqerr[:n].cpu().numpy(), hist[:n].cpu().numpy(), D, C_LOSS)
    assert frames == sum(TQS) == int(out[2]) and abs(float(out[3]) - tot) <= 2 * U24 * tot
    assert abs(float(out[0]) - vq) <= 4 * U24 * vq and abs(float(out[1]) - perp) <= ppl_bound * perp
    # two runs: the same bytes
    again = pk.outputs(n + 2)
    pk.L.check(pk.call(pk.table, again), "vq_stats_segments")
    assert all(torch.equal(a, b) if a.dtype == torch.int32 else _same(a, b) for a, b in zip(outs, again))


@pytest.mark.parametrize("D,K", [(16, 32), (65, 257)])
def test_groups_give_the_same_bytes_as_one_call(D, K):
    pk = Packed(D, K, seed=1)
    n, cut = len(TQS), 5
    one = pk.outputs(n + 2)
    pk.L.check(pk.call(pk.table, one), "one call")
    two = pk.outputs(n + 2)
    pk.L.check(pk.call(pk.table[:cut], two), "first group")
    head = [t.clone() for t in two]
    # behind the first group: its entries written, the others still the sentinel, out over the first group alone
    assert bool((two[0][cut:] == SENTINEL).all()) and bool((two[1][cut:] == ISENTINEL).all()) and bool((two[2][cut:] == SENTINEL).all())
    assert int(two[3][2]) == sum(TQS[:cut])
    pk.L.check(pk.call(pk.table[cut:], two, first=cut), "second group")
    for k in range(3):                                         # the second group touches the entries [cut, n) alone
        assert torch.equal(two[k][:cut], head[k][:cut])
    assert bool((two[0][n:] == SENTINEL).all()) and bool((two[1][n:] == ISENTINEL).all()) and bool((two[2][n:] == SENTINEL).all())
    assert _same(two[0], one[0]) and torch.equal(two[1], one[1]) and _same(two[2], one[2]) and _same(two[3], one[3])


def test_records_that_do_not_fit_give_zeros():
    """Out-of-contract records: zero results, nothing read (the latents around every item are NaN), no error.  Every record here keeps
    even a kernel that did NOT skip inside the allocations (Packed's margins)."""
    pk = Packed(16, 32, seed=2)
    good = [pk.offs[4], TQS[4]]
    ref = pk.outputs(1)
    pk.L.check(pk.call([good], ref), "good record")
    assert float(ref[0][0]) > 0.0
    for what, rec in (("Tq = 0", [400, 0]), ("Tq < 0", [400, -5]), ("q_off < 0", [-3, 100]), ("q_off + Tq > pitch", [pk.pitch - 50, 100])):
        outs = pk.outputs(3)
        pk.L.check(pk.call([good, rec], outs), what)
        assert _same(outs[0][0], ref[0][0]) and torch.equal(outs[1][0], ref[1][0]) and _same(outs[2][0], ref[2][0]), what
        assert float(outs[0][1]) == 0.0 and bool((outs[1][1] == 0).all()) and bool((outs[2][1] == 0.0).all()), what
        assert float(outs[0][2]) == SENTINEL and bool((outs[1][2] == ISENTINEL).all()), what
        assert _same(outs[3], ref[3]), what                   # a skipped record adds nothing to the list
        alone = pk.outputs(1)
        pk.L.check(pk.call([rec], alone), what)
        assert float(alone[0][0]) == 0.0 and bool((alone[1] == 0).all()) and bool((alone[2] == 0.0).all()), what
        assert bool((alone[3] == 0.0).all()), what              # a list without a frame: all four totals are 0


def test_argument_errors_launch_nothing():
    pk = Packed(16, 32, seed=3)
    outs = pk.outputs(len(TQS))
    for kw, code in ((dict(lat=None), EINVAL), (dict(quant=None), EINVAL), (dict(idx=None), EINVAL), (dict(segs=None), EINVAL),
                     (dict(sqerr=None), EINVAL), (dict(hist=None), EINVAL), (dict(item_stats=None), EINVAL), (dict(out=None), EINVAL),
                     (dict(nsegs=0), EINVAL), (dict(D=0), EINVAL), (dict(K=0), EINVAL), (dict(pitch=0), EINVAL), (dict(first=-1), EINVAL),
                     (dict(K=8193), EUNSUPPORTED)):
        assert pk.call(pk.table, outs, **kw) == code, kw
        assert pk.lib.wae_last_error().startswith(b"vq_stats_segments: ")
    assert bool((outs[0] == SENTINEL).all()) and bool((outs[1] == ISENTINEL).all()) and bool((outs[2] == SENTINEL).all())
    assert bool((outs[3] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- the engine
SMALL = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
             c_in=39, K=32, cin_pad=0)
FRAMES = [1, 5, 8, 20]


def _engine(cfg, sd, dtype):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd)
    return eng


class Counting:
    def __init__(self, lib, counts):
        self._lib, self._counts = lib, counts

    def __getattr__(self, name):
        self._counts[name] = self._counts.get(name, 0) + 1
        return getattr(self._lib, name)


def _clone(r):
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def test_encode_list_stats_are_the_utterances_alone():
    sd = O.make_state_dict(SMALL, 1)
    eng = _engine(SMALL, sd, "fp32")
    feats = [O.hash_fill((SMALL["c_in"], F), 40 + i, 1.7) for i, F in enumerate(FRAMES)]
    K, D = SMALL["K"], SMALL["Cc"]
    plain = [_clone(r) for r in eng.encode_list(feats, want_latents=True)]
    runs, totals = {}, {}
    from wavenet_autoencoders_amd import packing as P
    assert len(P.encode_list_groups(FRAMES, 16)) == 2
    for name, order, kw in (("given", [0, 1, 2, 3], {}), ("reversed", [3, 2, 1, 0], {}), ("groups", [0, 1, 2, 3], dict(max_frames=16))):
        res = eng.encode_list_stats([feats[i] for i in order], want_latents=True, **kw)
        torch.cuda.synchronize()
        runs[name] = {i: _clone(r) for r, i in zip(res, order)}
        totals[name] = eng.last_list_stats.clone()
    for i in range(len(FRAMES)):
        r = runs["given"][i]
        # the quantiser's outputs are what the call without statistics gives
        assert torch.equal(r["idx"], plain[i]["idx"]) and _same(r["quant"], plain[i]["quant"]) and _same(r["latents"], plain[i]["latents"])
        assert r["hist"].dtype == torch.int32 and r["hist"].shape == (K,) and r["perp"].dim() == 0 and r["vq_loss"].dim() == 0
        assert torch.equal(r["hist"].long(), torch.bincount(r["idx"], minlength=K))
        lat = r["latents"].contiguous()[None]
        N = lat.shape[2]
        _, idx1, stats = eng.vq_forward(lat)
        torch.cuda.synchronize()
        assert torch.equal(idx1, r["idx"])
        assert _same(r["perp"], stats[1]), (i, float(r["perp"]), float(stats[1]))
        # the dense value is a chain of fp32 atomics over non-negative terms, the less accurate side: 4 N + ceil(D / 256) + 12 roundings
        bound = (4 * N + -(-D // 256) + 12) * U24
        print(f"item {i}: vq_loss {float(r['vq_loss']):.9g}, vq_forward alone {float(stats[0]):.9g}, bound {bound:.2e}")
        assert abs(float(r["vq_loss"]) - float(stats[0])) <= bound * abs(float(stats[0]))
        ref = float(((r["quant"].double() - r["latents"].double()) ** 2).sum())
        assert abs(float(r["sqerr"]) - ref) <= 2.0 ** -23 * ref
        for name in ("reversed", "groups"):
            q = runs[name][i]
            assert all(_same(q[k], r[k]) for k in ("sqerr", "vq_loss", "perp")) and torch.equal(q["hist"], r["hist"]), (name, i)
            assert torch.equal(q["idx"], r["idx"]) and _same(q["quant"], r["quant"])
    assert _same(totals["given"], totals["groups"])
    # one group: the perplexity of the list is the dense search's on the packed latents
    packed = torch.cat([runs["given"][i]["latents"] for i in range(len(FRAMES))], dim=1).contiguous()[None]
    _, _, stats = eng.vq_forward(packed)
    torch.cuda.synchronize()
    assert _same(totals["given"][1], stats[1])
    vq, perp, frames, tot = P.vq_list_totals([float(runs["given"][i]["sqerr"]) for i in range(4)],
                                             torch.stack([runs["given"][i]["hist"] for i in range(4)]).cpu().numpy(), D, 1.25)
    t = totals["given"]
    assert int(t[2]) == frames == sum(-(-F // 4) for F in FRAMES)
    assert abs(float(t[0]) - vq) <= 4 * U24 * vq and abs(float(t[3]) - tot) <= 2 * U24 * tot


def test_the_statistics_cost_one_call_per_group():
    sd = O.make_state_dict(SMALL, 1)
    eng = _engine(SMALL, sd, "fp32")
    eng.prepare_weights()
    counts = {}
    eng.lib = Counting(eng.lib, counts)
    for n in (3, 12):
        feats = [O.hash_fill((SMALL["c_in"], 5 + 3 * i), 60 + i, 1.7) for i in range(n)]
        counts.clear()
        eng.encode_list(feats)
        base = dict(counts)
        assert "wae_vq_stats_segments" not in base and base["wae_vq_nearest"] == 1
        counts.clear()
        eng.encode_list_stats(feats)
        with_stats = dict(counts)
        assert with_stats.pop("wae_vq_stats_segments") == 1
        assert with_stats == base, (with_stats, base)          # one more call, and the launches in front of it as they were
        counts.clear()
        eng.encode_list_stats(feats, max_frames=12)
        from wavenet_autoencoders_amd import packing as P
        groups = len(P.encode_list_groups([5 + 3 * i for i in range(n)], 12))
        assert groups > 1 and counts["wae_vq_stats_segments"] == groups == counts["wae_vq_nearest"]
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- scalar decoders
DEC = dict(layers=10, stacks=1, R=32, G=32, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
DEC_T = [1, 129, 300, 257, 1100]
QC, LSM = 65536, -7.0


def _scalar_items(cfg, Ts, salt=0):
    return [dict(x=O.hash_fill((T,), 100 + salt + i), c=O.hash_fill((cfg["Cc"], T), 200 + salt + i, 1.0), gid=(2 * i + 1) % cfg["n_speakers"])
            for i, T in enumerate(Ts)]


def _alone(eng, it, dist):
    """decoder_forward of the item as a batch of one, then the dense loss entry on its logits with B = 1, shift = 1 ->
    (logits (O, T), nll (T,))"""
    from wavenet_autoencoders_amd import _lib as L
    lib = L.lib()
    x = it["x"][None].cuda().contiguous()
    T = x.shape[1]
    out = eng.decoder_forward(x, it["c"][None].cuda(), torch.tensor([it["gid"]]).cuda(), c_is_upsampled=True, want_logits=True)
    lg = out["logits"].clone()
    nll = torch.full((1, T), SENTINEL, device="cuda")
    Oc = lg.shape[1]
    if dist == "Normal":
        L.check(lib.wae_mog_loss_fwd(L.ptr(lg), L.ptr(x), L.ptr(nll), None, 1, Oc, T, LSM, 1, eng.stream()), "mog_loss")
    else:
        L.check(lib.wae_dmol_loss_fwd(L.ptr(lg), L.ptr(x), L.ptr(nll), None, 1, Oc // 3, T, QC, LSM, 1, eng.stream()), "dmol_loss")
    torch.cuda.synchronize()
    return lg[0], nll[0]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dist,Oc", [("Logistic", 30), ("Normal", 30), ("Normal", 2)])
def test_the_mixture_nll_of_a_list_is_the_utterances_alone(dist, Oc, dtype):
    """Scalar-input decoders under both output distributions: logits bit for bit decoder_forward of the item alone, nll bit for bit
    the dense loss entry on those logits.  (Before the list form had a mixture NLL these calls raised NotImplementedError.)"""
    cfg = dict(DEC, scalar_input=True, O=Oc, output_distribution=dist)
    sd = O.make_state_dict(cfg, salt=9, with_encoder=False)
    eng = _engine(cfg, sd, dtype)
    items = _scalar_items(cfg, DEC_T)
    single = [_alone(eng, it, dist) for it in items]
    runs = {}
    for name, order, kw in (("given", list(range(5)), {}), ("reversed", [4, 3, 2, 1, 0], {}), ("groups", list(range(5)), dict(max_rows=600))):
        res, loss = eng.decoder_forward_list([items[i] for i in order], c_is_upsampled=True, quantize_channels=QC, log_scale_min=LSM, **kw)
        torch.cuda.synchronize()
        eng.check_errors()
        sums = [None] * 5
        for r, i in zip(res, order):
            lg, nl = single[i]
            assert _same(r["logits"], lg), (dist, Oc, dtype, name, i, "logits")
            assert _same(r["nll"], nl), (dist, Oc, dtype, name, i, "nll")
            assert int(r["count"]) == DEC_T[i] - 1 and float(r["nll"][-1]) == 0.0
            ref = float(nl.double().sum())
            slack = 2.0 ** -23 * abs(ref) + 2.0 ** -40 * float(nl.double().abs().sum())      # MoG values change sign
            assert abs(float(r["nll_sum"]) - ref) <= slack, (dist, Oc, dtype, name, i, float(r["nll_sum"]), ref)
            sums[i] = r["nll_sum"].clone()
        runs[name] = torch.stack(sums)
        cnt = sum(T - 1 for T in DEC_T)
        refs = [float(single[i][1].double().sum()) for i in range(5)]
        mags = [float(single[i][1].double().abs().sum()) for i in range(5)]
        tot = sum(refs) / cnt
        print(f"{dist} O {Oc} {dtype} {name}: loss {float(loss):.7f}, float64 of the single forwards' nll {tot:.7f}")
        # every nll_sum within its own bound (above), their fp64 sum and quotient exact to 2^-53, one rounding to fp32
        assert abs(float(loss) - tot) <= (2.0 ** -23 * sum(abs(r) for r in refs) + 2.0 ** -40 * sum(mags)) / cnt + U24 * abs(tot)
    assert _same(runs["given"], runs["reversed"]) and _same(runs["given"], runs["groups"])
    assert float(runs["given"][0]) == 0.0                       # T = 1: nothing to predict
    # without the logits the numbers are the same (the parameters go through an internal buffer)
    res, _ = eng.decoder_forward_list(items, want_logits=False, c_is_upsampled=True, quantize_channels=QC, log_scale_min=LSM)
    torch.cuda.synchronize()
    assert all(r["logits"] is None and _same(r["nll"], s[1]) for r, s in zip(res, single))


def test_the_list_loss_of_golden_S_against_the_oracle():
    """Golden model S (scalar input, logistic mixture), fp32: the list loss of two utterances of unequal lengths against
    oracle.masked_dmol_loss of each alone, at the tolerance the dense path's tests use for that loss (tests/test_gpu_loss_optim.py,
    tests/test_gpu_mog.py: 1e-4 relative)."""
    cfg, sd, ins, z, ocfg = golden_model("S")
    eng = _engine(cfg, sd, "fp32")
    items, want, cnt = [], 0.0, 0
    for b, F in ((0, 8), (1, 4)):
        T = F // 4 * 640
        x, c, g = ins["x"][b, 0, :T].contiguous(), ins["c"][b, :, :F].contiguous(), ins["g"][b:b + 1]
        items.append(dict(x=x, feats=c, gid=int(g[0])))
        with torch.no_grad():
            y, _, _, _ = O.vqvae_forward(sd, ocfg, x[None, None], c[None], g)
            one = float(O.masked_dmol_loss(y, x[None, :, None], torch.full((1,), T), 65536, -7.0))
        want += one * (T - 1)
        cnt += T - 1
    want /= cnt
    res, loss = eng.forward_list(items, want_logits=False, quantize_channels=65536, log_scale_min=-7.0)
    torch.cuda.synchronize()
    got = float(loss)
    print(f"golden S: list loss {got:.7f}, oracle {want:.7f}, rel {abs(got - want) / abs(want):.2e}")
    assert abs(got - want) < 1e-4 * abs(want)
    own = sum(float(r["nll_sum"]) for r in res) / cnt
    assert abs(got - own) <= 1e-6 * abs(own)


# ---------------------------------------------------------------------------------------------------------------- evaluate
def _full_items(cfg, frames, scalar=False):
    items = []
    for i, F in enumerate(frames):
        T = -(-F // 4) * 640
        if scalar:
            x = O.hash_fill((T,), 50 + i)
        else:
            x = ((O.hash_fill((T,), 50 + i) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
        items.append(dict(x=x, feats=O.hash_fill((cfg["c_in"], F), 40 + i, 1.7), gid=(i + 1) % cfg["n_speakers"]))
    return items


def _padded(items, cfg):
    Fm, Tm = max(it["feats"].shape[1] for it in items), max(it["x"].numel() for it in items)
    c = torch.zeros(len(items), cfg["c_in"], Fm)
    x = torch.zeros(len(items), Tm, dtype=items[0]["x"].dtype)
    for i, it in enumerate(items):
        c[i, :, :it["feats"].shape[1]] = it["feats"]
        x[i, :it["x"].numel()] = it["x"]
    return x, c


def _batch(items, cfg):
    xp, cp = _padded(items, cfg)
    return [(xp, cp, torch.tensor([it["gid"] for it in items]), torch.tensor([it["x"].numel() for it in items]))]


def test_dev_packed_reports_the_quantisers_numbers():
    """The three-utterance batch of tests/test_gpu_forward_list.py::test_dev_packed_scores_the_utterances_alone: vq_loss and the
    perplexity (nan before the list form had them) are score_list's totals, and with packed_total the loss is ce + vq_loss."""
    import vqwae_train
    sd = O.make_state_dict(SMALL, 1)
    eng = _engine(SMALL, sd, "bf16")
    items = _full_items(SMALL, [4, 8, 20])
    hp = types.SimpleNamespace(max_time_steps=None, hop_size=160, cin_pad=0, quantize_channels=64, log_scale_min=-7.0)
    ce, vq, perp = vqwae_train.evaluate(eng, _batch(items, SMALL), "cuda:0", hp, packed=True)
    loss, vq2, perp2 = vqwae_train.evaluate(eng, _batch(items, SMALL), "cuda:0", hp, packed=True, packed_total=True)
    assert all(math.isfinite(v) for v in (ce, vq, perp, loss)) and vq > 0.0 and 1.0 <= perp <= SMALL["K"]
    res, t = eng.score_list(items, quantize_channels=64, log_scale_min=-7.0)
    torch.cuda.synchronize()
    assert set(t) == {"ce", "vq_loss", "perp", "loss", "count", "frames"} and all(v.dim() == 0 and v.is_cuda for v in t.values())
    assert (vq, perp) == (float(t["vq_loss"]), float(t["perp"])) == (vq2, perp2) and ce == float(t["ce"])
    assert loss == float(t["loss"]) == float(t["ce"] + t["vq_loss"])
    assert abs(loss - (ce + vq)) <= 4 * U24 * abs(loss)
    assert float(t["count"]) == sum(it["x"].numel() - 1 for it in items) and float(t["frames"]) == 1 + 2 + 5
    assert all(r["logits"] is None and r["latents"] is None and r["hist"].shape == (SMALL["K"],) for r in res)
    # the module-level door
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    assert callable(VQVAE.score_list)


def test_dev_packed_scores_a_scalar_input_model():
    """A scalar-input model under "Normal": three finite numbers, score_list's totals (this call used to raise NotImplementedError)."""
    import vqwae_train
    cfg = dict(SMALL, scalar_input=True, O=30, output_distribution="Normal")
    sd = O.make_state_dict(cfg, 1)
    eng = _engine(cfg, sd, "bf16")
    items = _full_items(cfg, [4, 8, 20], scalar=True)
    hp = types.SimpleNamespace(max_time_steps=None, hop_size=160, cin_pad=0, quantize_channels=65536, log_scale_min=-7.0)
    got = vqwae_train.evaluate(eng, _batch(items, cfg), "cuda:0", hp, packed=True, packed_total=True)
    print("--dev-packed, scalar input, Normal:", got)
    assert len(got) == 3 and all(math.isfinite(v) for v in got)
    _, t = eng.score_list(items, quantize_channels=65536, log_scale_min=-7.0)
    assert got[0] == float(t["loss"]) and got[1] == float(t["vq_loss"]) and got[2] == float(t["perp"])
