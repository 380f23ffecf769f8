"""The ragged conditioning upsampler on the GPU (wae_upsample_stage_fwd_list, wae_to_btc_list, WaeEngine.upsample_list,
decode_list / DecodeSession.add_list through it): every item's rows are BITWISE what the per-item path -- wae_upsample_stage_fwd /
wae_to_btc / upsample_forward with B = 1 -- writes for that item alone, whatever the order, the grouping and the neighbours.  The
segment lengths put an item below, at and one step past a tile edge and leave items without any interior step; neighbouring segments
differ by 1e3 in scale and the slack between them holds 1e6, so a read across an item boundary, or the three summed taps applied
against the packed length instead of the item's, cannot hide."""
import numpy as np
import pytest
import torch

from oracle import wae_oracle as O
from helpers import rel_err

pytestmark = pytest.mark.gpu
DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
SENT = -77.0


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _records(in_off, Tin, out_off, Tout, tile):
    from wavenet_autoencoders_amd import packing as PK
    rec, nt = PK.ups_list_records(np.asarray(in_off), np.asarray(Tin), np.asarray(out_off), np.asarray(Tout), tile)
    return torch.from_numpy(rec.reshape(-1)).cuda(), nt


def _packed_input(C, lens, gen, slack=3):
    """(C, pitch) with the segments `slack` columns apart, 1e6 in the slack, neighbouring segments 1e3 apart in scale"""
    offs, at = [], slack
    for n in lens:
        offs.append(at)
        at += n + slack
    x = torch.full((C, at), 1e6)
    for i, (o, n) in enumerate(zip(offs, lens)):
        x[:, o:o + n] = torch.randn(C, n, generator=gen) * (1e3 if i % 2 else 1.0)
    return x.cuda(), offs


def _scattered(lens, perm, gap=2):
    """offsets of the items in an output where they lie in the order `perm`, `gap` rows or columns apart; and the total"""
    offs, at = [0] * len(lens), gap
    for j in perm:
        offs[j] = at
        at += lens[j] + gap
    return offs, at


def _owned(offs, lens, total):
    m = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(offs, lens):
        assert not m[o:o + n].any()
        m[o:o + n] = True
    return m.cuda()


# ---- 1. the raw stage entry -------------------------------------------------------------------------------------------------------------
TINS = [1, 2, 3, 7, 13, 16, 17, 33]
PERM = [5, 0, 7, 2, 6, 1, 4, 3]


@pytest.mark.parametrize("C,Cp", [(1, 64), (16, 64), (64, 64), (80, 128), (200, 256)])
@pytest.mark.parametrize("s", [2, 4, 5, 8])
def test_stage_entry_is_the_dense_stage_per_segment(s, C, Cp):
    L, lib = _lib()
    gen = torch.Generator().manual_seed(100 * s + C)
    x, in_off = _packed_input(C, TINS, gen)
    w = torch.randn(2 * s + 1, generator=gen).cuda()
    Tout = [t * s for t in TINS]
    assert 16 * 4 == 64 and 8 * 8 == 64 and 13 * 5 == 65           # (the lengths the tile edges of s = 4, 8, 5 are chosen for)
    out_off, total = _scattered(Tout, PERM)
    owned = _owned(out_off, Tout, total)
    dense_in = [x[:, o:o + n].contiguous()[None] for o, n in zip(in_off, TINS)]
    # channel-major, fp32
    rec, nt = _records(in_off, TINS, out_off, Tout, 256)
    y = torch.full((C, total), SENT, device="cuda")
    L.check(lib.wae_upsample_stage_fwd_list(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rec), len(TINS), nt, x.shape[1], total, C, s, 0, Cp, 0,
                                            None), "stage list")
    for i, (xi, o, n) in enumerate(zip(dense_in, out_off, Tout)):
        ref = torch.empty(1, C, n, device="cuda")
        L.check(lib.wae_upsample_stage_fwd(L.ptr(xi), L.ptr(w), L.ptr(ref), 1, C, TINS[i], s, 0, Cp, 0, None), "stage")
        assert _same(y[:, o:o + n], ref[0]), ("channel-major", i)
    assert (y[:, ~owned] == SENT).all()
    # time-major, three storage types
    rec, nt = _records(in_off, TINS, out_off, Tout, 64)
    for name, (dt, td) in DT.items():
        y = torch.full((total, Cp), SENT, dtype=td, device="cuda")
        L.check(lib.wae_upsample_stage_fwd_list(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rec), len(TINS), nt, x.shape[1], total, C, s, 1, Cp,
                                                dt, None), "last stage list")
        for i, (xi, o, n) in enumerate(zip(dense_in, out_off, Tout)):
            ref = torch.full((1, n, Cp), SENT, dtype=td, device="cuda")
            L.check(lib.wae_upsample_stage_fwd(L.ptr(xi), L.ptr(w), L.ptr(ref), 1, C, TINS[i], s, 1, Cp, dt, None), "last stage")
            assert _same(y[o:o + n], ref[0]), (name, i, TINS[i])
            assert (y[o:o + n, C:] == 0).all() and bool(torch.isfinite(y[o:o + n].float()).all())
            assert float(y[o:o + n, :C].float().abs().max()) < 1e5          # nothing of the 1e6 slack
        assert (y[~owned] == SENT).all(), name


def test_stage_entry_skips_records_that_do_not_fit():
    """a record beyond the pitch, beyond the rows or with a tile count that contradicts Tout = Tin * s: nothing is written for it"""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(3)
    C, Cp, s, lens = 16, 64, 4, [5, 9, 20]
    x, in_off = _packed_input(C, lens, gen)
    w = torch.randn(2 * s + 1, generator=gen).cuda()
    Tout = [t * s for t in lens]
    out_off, total = _scattered(Tout, [2, 0, 1])
    good, nt = _records(in_off, lens, out_off, Tout, 64)
    want = torch.full((total, Cp), SENT, dtype=torch.bfloat16, device="cuda")
    L.check(lib.wae_upsample_stage_fwd_list(L.ptr(x), L.ptr(w), L.ptr(want), L.ptr(good), 3, nt, x.shape[1], total, C, s, 1, Cp, 1, None), "")
    for bad in ("in_off", "out_off", "tiles"):
        rec = good.clone().view(4, 4)
        if bad == "in_off":
            rec[1, 0] = x.shape[1] - 3                     # in_off + Tin > in_pitch
        elif bad == "out_off":
            rec[1, 2] = total - 5                          # out_off + Tout > rows
        else:
            rec[1, 1] = 40                                 # Tin * s needs 3 tiles, the table gives the item 1
        got = torch.full((total, Cp), SENT, dtype=torch.bfloat16, device="cuda")
        L.check(lib.wae_upsample_stage_fwd_list(L.ptr(x), L.ptr(w), L.ptr(got), L.ptr(rec), 3, nt, x.shape[1], total, C, s, 1, Cp, 1, None),
                "")
        torch.cuda.synchronize()
        o, n = out_off[1], Tout[1]
        assert (got[o:o + n] == SENT).all(), bad           # the bad record's item: untouched (it was the only writer of these rows)
        keep = torch.ones(total, dtype=torch.bool, device="cuda")
        keep[o:o + n] = False
        assert _same(got[keep], want[keep]), bad           # the others: as before


# ---- 2. wae_to_btc_list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C,Cp", [(16, 64), (80, 128)])
@pytest.mark.parametrize("trim", [0, 3])
def test_to_btc_list_is_to_btc_per_trimmed_segment(trim, C, Cp, dtype):
    L, lib = _lib()
    dt, td = DT[dtype]
    Ts = [1, 63, 64, 65, 130]
    gen = torch.Generator().manual_seed(7 + trim + C)
    x, in_off = _packed_input(C, [t + 2 * trim for t in Ts], gen)
    out_off, total = _scattered(Ts, [3, 1, 4, 0, 2])
    rec, nt = _records([o + trim for o in in_off], Ts, out_off, Ts, 64)      # the host folds the trim into in_off / Tin
    y = torch.full((total, Cp), SENT, dtype=td, device="cuda")
    L.check(lib.wae_to_btc_list(L.ptr(x), L.ptr(y), L.ptr(rec), len(Ts), nt, x.shape[1], C, Cp, dt, None), "to_btc_list")
    for i, (o, n) in enumerate(zip(out_off, Ts)):
        xi = x[:, in_off[i] + trim:in_off[i] + trim + n].contiguous()
        ref = torch.full((1, n, Cp), SENT, dtype=td, device="cuda")
        L.check(lib.wae_to_btc(L.ptr(xi), L.ptr(ref), 1, C, n, Cp, dt, None), "to_btc")
        assert _same(y[o:o + n], ref[0]), i
        assert (y[o:o + n, C:] == 0).all()
    assert (y[~_owned(out_off, Ts, total)] == SENT).all()


# ---- 3. WaeEngine.upsample_list ---------------------------------------------------------------------------------------------------------
NET = dict(layers=4, stacks=2, R=32, G=32, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
GEOMS = {
    "conv_in": dict(NET),
    "conv_in_cc64": dict(NET, Cc=64),
    "cin_pad_1": dict(NET, cin_pad=1),                                                     # model_P's network
    "cin_pad_2": dict(NET, cin_pad=2),
    "plain_trim": dict(NET, cin_pad=1, conv_in=False),                                     # model_U's
    "plain": dict(NET, conv_in=False),
    "leaky": dict(NET, up_act="LeakyReLU", up_act_slope=0.2),                              # model_V's four
    "tanh_plain": dict(NET, conv_in=False, up_act="Tanh"),
    "relu": dict(NET, up_act="ReLU"),
    "sigmoid": dict(NET, up_act="Sigmoid"),
}
FRAMES = [1, 2, 3, 5, 17]
_CACHE = {}


def _net(name, dtype):
    """(engine, items, every item's rows by upsample_forward alone): built once per (geometry, dtype) and left unchanged"""
    if (name, dtype) not in _CACHE:
        from wavenet_autoencoders_amd import Geometry
        from wavenet_autoencoders_amd.engine import WaeEngine
        cfg = GEOMS[name] if name in GEOMS else dict(NET, Cc=130)
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
        eng.load_state_dict(O.make_state_dict(dict(cfg), salt=11, with_encoder=False))
        eng.prepare_weights()
        gen = torch.Generator().manual_seed(len(name))
        cs = [torch.randn(cfg["Cc"], f + 2 * cfg["cin_pad"], generator=gen) * (1e3 if i % 2 else 1.0) for i, f in enumerate(FRAMES)]
        alone = []
        for c, f in zip(cs, FRAMES):
            o = torch.full((1, f * 640, eng.g.Ccp), SENT, dtype=eng.tdtype, device="cuda")
            eng.upsample_forward(c[None].cuda(), o)
            alone.append(o[0].clone())
        torch.cuda.synchronize()
        _CACHE[(name, dtype)] = (eng, cs, alone)
    return _CACHE[(name, dtype)]


def _rows(c_up, offs, alone):
    return [c_up[int(o):int(o) + a.shape[0]] for o, a in zip(offs, alone)]


CASES = [(n, d) for n in GEOMS for d in ("fp32", "bf16")] + [("conv_in", "fp16")]


@pytest.mark.parametrize("name,dtype", CASES, ids=[f"{n}-{d}" for n, d in CASES])
def test_upsample_list_is_the_loop_bit_for_bit(name, dtype):
    eng, cs, alone = _net(name, dtype)
    dev = [c.cuda() for c in cs]
    c_up, offs = eng.upsample_list(dev)
    assert c_up.shape == (sum(FRAMES) * 640, eng.g.Ccp) and c_up.dtype == eng.tdtype
    assert list(offs) == list(np.concatenate([[0], np.cumsum([f * 640 for f in FRAMES])[:-1]]))
    for i, (got, want) in enumerate(zip(_rows(c_up, offs, alone), alone)):
        assert _same(got, want), (name, dtype, "item", i)
    # another order
    perm = [3, 0, 4, 2, 1]
    c2, o2 = eng.upsample_list([dev[j] for j in perm])
    for k, j in enumerate(perm):
        assert _same(c2[int(o2[k]):int(o2[k]) + alone[j].shape[0]], alone[j]), ("shuffled", j)
    # three groups
    from wavenet_autoencoders_amd import packing as PK
    assert len(PK.upsample_list_groups([f * 640 for f in FRAMES], 5120)) == 3
    c3, o3 = eng.upsample_list(dev, max_samples=5120)
    assert all(_same(a, b) for a, b in zip(_rows(c3, o3, alone), alone)), "groups"
    # host arrays, CPU tensors, device tensors and (1, Cc, Tc) items, mixed
    mixed = [cs[0].numpy(), dev[1], cs[2][None], dev[3][None], cs[4]]
    c4, o4 = eng.upsample_list(mixed)
    assert all(_same(a, b) for a, b in zip(_rows(c4, o4, alone), alone)), "mixed"
    # the caller's operand and rows
    lens = [a.shape[0] for a in alone]
    offs5, total = _scattered(lens, [2, 4, 0, 3, 1], gap=5)
    out = torch.full((total, eng.g.Ccp), SENT, dtype=eng.tdtype, device="cuda")
    c5, o5 = eng.upsample_list(mixed, out=out, offsets=offs5, max_samples=5120)
    assert c5 is out and list(o5) == offs5
    assert all(_same(a, b) for a, b in zip(_rows(out, offs5, alone), alone)), "given rows"
    assert (out[~_owned(offs5, lens, total)] == SENT).all()
    with pytest.raises(ValueError, match="upsample_list: out is"):
        eng.upsample_list(dev, out=out[:100])


def test_upsample_list_against_the_oracle():
    eng, cs, alone = _net("cin_pad_1", "fp32")
    sd = O.make_state_dict(dict(GEOMS["cin_pad_1"]), salt=11, with_encoder=False)
    c_up, offs = eng.upsample_list(cs)
    for c, got in zip(cs, _rows(c_up, offs, alone)):
        with torch.no_grad():
            want = O.upsample_forward(sd, c[None], NET["upsample_scales"], cin_pad=1)[0]            # (Cc, T)
        assert rel_err(got[:, :NET["Cc"]].t().cpu(), want) < 1e-3


def test_unsupported_geometry_runs_the_loop_into_the_same_rows():
    eng, cs, alone = _net("cc130", "bf16")
    assert eng.g.Ccp == 192
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    real, eng.lib = eng.lib, Counting(eng.lib)
    try:
        c_up, offs = eng.upsample_list(cs)
    finally:
        eng.lib = real
    assert all(_same(a, b) for a, b in zip(_rows(c_up, offs, alone), alone))
    assert calls.count("wae_upsample_stage_fwd") == 4 * len(cs) and not [n for n in calls if n.endswith("_list")]


# ---- 4. / 5. decode_list and the sessions through it ------------------------------------------------------------------------------------
TINY = dict(layers=4, stacks=2, R=32, G=32, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[2, 3], cin_pad=0)
TINY_SCALAR = dict(TINY, O=30, scalar_input=True)
UPS = ("wae_enc_conv_fwd_list", "wae_upsample_stage_fwd_list", "wae_to_btc_list", "wae_act_fwd", "wae_enc_conv_fwd", "wae_to_btc")


def _decoder(cfg, dtype, monkeypatch, coop="0"):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    monkeypatch.setenv("WAE_AR_COOP", coop)
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(O.make_state_dict(dict(cfg), salt=5, with_encoder=False))
    return eng


def _latent_items(cfg, frames, seed=2):
    gen = torch.Generator().manual_seed(seed)
    items = []
    for i, f in enumerate(frames):
        T = f * 6
        it = dict(T=T, c=torch.randn(cfg["Cc"], f, generator=gen) * (30.0 if i % 2 else 1.0), gid=int(torch.randint(0, 5, (1,), generator=gen)))
        if cfg.get("scalar_input"):
            it.update(u_mix=torch.rand(T, cfg["O"] // 3, generator=gen).cuda() * (1 - 2e-5) + 1e-5,
                      u_log=torch.rand(T, generator=gen).cuda() * (1 - 2e-5) + 1e-5)
        else:
            it.update(uniforms=torch.rand(T, generator=gen).cuda(), init_idx=31)
        items.append(it)
    return items


def test_launches_do_not_grow_with_the_list(monkeypatch):
    eng = _decoder(TINY, "bf16", monkeypatch)
    counts = {}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            counts[name] = counts.get(name, 0) + 1
            return getattr(self._lib, name)

    eng.lib = Counting(eng.lib)
    per_list = []
    for n in (3, 12):
        counts.clear()
        eng.decode_list(_latent_items(TINY, [1 + (5 * i) % 7 for i in range(n)]), mode="sample")
        assert counts.get("wae_upsample_stage_fwd", 0) == 0 and counts.get("wae_ar_generate_list", 0) == 1
        per_list.append({k: counts.get(k, 0) for k in UPS})
    assert per_list[0] == per_list[1]
    assert sum(per_list[0].values()) == 1 + len(TINY["upsample_scales"])              # one group: conv_in and a launch per stage
    assert per_list[0]["wae_enc_conv_fwd_list"] == 1 and per_list[0]["wae_upsample_stage_fwd_list"] == 2


def _alone(eng, it, coop):
    """the item as a batch of one through incremental_forward, on the one-CU kernel (WAE_AR_COOP=0) or the cooperative path (=1)"""
    kw = {k: it[k][None] for k in ("uniforms", "u_mix", "u_log") if k in it}
    if "init_idx" in it:
        kw["init_idx"] = it["init_idx"]
    eng._ar_profile = None
    out = eng.incremental_forward(it["c"][None].cuda(), torch.tensor([it["gid"]]).cuda(), it["T"], mode="sample", want_logits=True, **kw)
    assert (eng._ar_profile is not None) == coop              # (the cooperative paths leave their error / profile words)
    key = "x" if eng.g.scalar_input else "idx"
    return out[key][0].clone(), out["logits"][0].clone()


FRAMES5 = [7, 1, 12, 3, 20]


@pytest.mark.parametrize("route", ["slots", "teams", "scalar_slots"])
def test_decode_list_items_are_their_single_decodes(route, monkeypatch):
    cfg = TINY_SCALAR if route == "scalar_slots" else TINY
    coop = route == "teams"
    eng = _decoder(cfg, "bf16", monkeypatch, coop="1" if coop else "0")
    items = _latent_items(cfg, FRAMES5)
    key = "x" if cfg.get("scalar_input") else "idx"
    fn = eng.decode_list_scalar if cfg.get("scalar_input") else eng.decode_list
    got = fn(items, mode="sample", want_logits=True, coop=coop)
    got = [(r[key].clone(), r["logits"].clone()) for r in got]
    for i, it in enumerate(items):
        a, b = _alone(eng, it, coop)
        assert _same(got[i][0], a) and _same(got[i][1], b), (route, i)
    # the length check keeps its type and wording, with the item's index, before any launch
    bad = [dict(items[0]), dict(items[1], T=items[1]["T"] + 1)]
    with pytest.raises(AssertionError, match="item 1: c does not upsample to T"):
        fn(bad, mode="sample", coop=coop)


def test_add_list_is_sequential_add_and_the_stream_is_the_list(monkeypatch):
    eng = _decoder(TINY, "bf16", monkeypatch)
    items = _latent_items(TINY, FRAMES5)
    want = eng.decode_list(items, mode="sample", want_logits=True)
    want = [(r["idx"].clone(), r["logits"].clone()) for r in want]

    def rounds(join):
        with eng.decode_session(mode="sample", want_logits=True) as sess:
            hs = join(sess)
            out = []
            while sess.live:
                res = sess.step(25)
                out.append({h: (r["idx"].clone(), r["logits"].clone(), r["done"]) for h, r in res.items()})
        return hs, out

    ha, a = rounds(lambda s: [s.add(it) for it in items])
    hb, b = rounds(lambda s: s.add_list(items))
    assert ha == hb == list(range(len(items))) and len(a) == len(b)
    for ra, rb in zip(a, b):
        assert ra.keys() == rb.keys()
        for h in ra:
            assert _same(ra[h][0], rb[h][0]) and _same(ra[h][1], rb[h][1]) and ra[h][2] == rb[h][2]
    for i, h in enumerate(hb):
        assert _same(torch.cat([r[h][0] for r in b if h in r]), want[i][0])
    # a second list joins between two rounds; a bad item adds nothing
    with eng.decode_session(mode="sample") as sess:
        first = sess.add_list(items[:2])
        sess.step(3)                                       # (the shortest clip has 6 steps: nobody leaves)
        assert sess.add_list(items[2:4]) == [2, 3] and sess.live == first + [2, 3]
        with pytest.raises(AssertionError, match="decode_session.add: c does not upsample to T"):
            sess.add_list([items[4], dict(items[0], T=5)])
        assert sess.live == [0, 1, 2, 3] and sess.add_list([]) == []
    # decode_list_stream runs on add_list
    got = [[] for _ in items]
    for res in eng.decode_list_stream(items, 40, mode="sample", want_logits=True):
        for i, r in enumerate(res):
            if r is not None:
                got[i].append((r["idx"].clone(), r["logits"].clone()))
    for i in range(len(items)):
        assert _same(torch.cat([g[0] for g in got[i]]), want[i][0])
        assert _same(torch.cat([g[1] for g in got[i]], dim=1), want[i][1])
