"""Clips whose conditioning arrives while they decode, on the GPU (wae_upsample_stage_fwd_ranges, DecodeSession.open / feed /
feed_list / end, synthesis.py --feed-frames): the rows of c_up that the session calls final, taken as they become final, are BITWISE
upsample_forward's rows of the whole clip, and a clip that is fed in pieces with step() between the feeds decodes BITWISE as
incremental_forward of the whole clip -- on the slots and on the teams, class ids and scalars.  Clips lie side by side 1e3 apart in
scale with 1e6 in the arenas' slack, so a read past a clip's valid columns cannot hide; the ranges start in the middle of a tile, end on
a tile edge and a step past one."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import golden_model
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
SENT = -77.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _records(rows, tile):
    """rows: (in_off, Tin, out_off, t_lo, t_hi) per record -> the device table with tile0 and the closing record, and the tile count"""
    rec, nt = [], 0
    for r in rows:
        rec.append(list(r) + [nt])
        nt += -(-(r[4] - r[3]) // tile)
    rec.append([0, 0, 0, 0, 0, nt])
    return torch.tensor(rec, dtype=torch.int32).reshape(-1).cuda(), nt


# ---- 1. the raw entry: rows of a prefix are the dense stage's rows of the whole clip ------------------------------------------------------
FULL = 80                                                  # frames of every whole clip
NOW = [70, 75, 80]                                         # frames valid now: two open clips and one that has ended


def _clips(C, gen, slack=3):
    """three clips of FULL frames side by side, `slack` columns apart, 1e3 apart in scale; only NOW[i] columns of clip i are valid,
    the rest of its place and the slack hold 1e6"""
    whole = [torch.randn(C, FULL, generator=gen) * sc for sc in (1e-3, 1.0, 1e3)]
    offs, at = [], slack
    for _ in whole:
        offs.append(at)
        at += FULL + slack
    x = torch.full((C, at), 1e6)
    for o, w, n in zip(offs, whole, NOW):
        x[:, o:o + n] = w[:, :n]
    return x.cuda(), offs, [w.cuda() for w in whole]


@pytest.mark.parametrize("C,Cp", [(16, 64), (80, 128)])
@pytest.mark.parametrize("s", [4, 5, 8])
def test_ranges_entry_rows_are_the_dense_stage_of_the_whole_clip(s, C, Cp):
    L, lib = _lib()
    gen = torch.Generator().manual_seed(10 * s + C)
    x, in_off, whole = _clips(C, gen)
    w = torch.randn(2 * s + 1, generator=gen).cuda()
    Tout = FULL * s
    out_off = [5, 5 + Tout + 7, 5 + 2 * (Tout + 7)]
    total = out_off[-1] + Tout + 4

    def ranges(tile):
        """clip 0: starts mid-tile and ends exactly on a tile edge (counted from t_lo); clip 1: a step past the edge, up to the last
        final row of an open clip; clip 2 (ended): a single row, and in a second record the rows up to the clip's end"""
        hi1 = (NOW[1] - 1) * s
        assert 7 + tile <= (NOW[0] - 1) * s and hi1 - (tile + 1) >= 0
        return [(in_off[0], NOW[0], out_off[0], 7, 7 + tile), (in_off[1], NOW[1], out_off[1], hi1 - (tile + 1), hi1),
                (in_off[2], NOW[2], out_off[2], 3, 4), (in_off[2], NOW[2], out_off[2], Tout - tile - 9, Tout)]

    def check(y, ref_of, rows, name):
        mask = torch.zeros(total, dtype=torch.bool, device="cuda")
        for (_, _, oo, lo, hi), i in zip(rows, (0, 1, 2, 2)):
            ref = ref_of(i)
            got = y[oo + lo:oo + hi] if y.shape[0] == total else y[:, oo + lo:oo + hi]
            want = ref[lo:hi] if y.shape[0] == total else ref[:, lo:hi]
            assert _same(got, want), (name, i, lo, hi)
            mask[oo + lo:oo + hi] = True
        rest = y[~mask] if y.shape[0] == total else y[:, ~mask]
        assert (rest == SENT).all(), name                  # rows outside every range: not written

    # channel-major, fp32
    rows = ranges(256)
    rec, nt = _records(rows, 256)
    y = torch.full((C, total), SENT, device="cuda")
    L.check(lib.wae_upsample_stage_fwd_ranges(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rec), len(rows), nt, x.shape[1], total, C, s, 0, Cp, 0,
                                              None), "stage ranges")
    dense = []
    for wh in whole:
        ref = torch.empty(1, C, Tout, device="cuda")
        L.check(lib.wae_upsample_stage_fwd(L.ptr(wh.contiguous()), L.ptr(w), L.ptr(ref), 1, C, FULL, s, 0, Cp, 0, None), "stage")
        dense.append(ref[0])
    check(y, lambda i: dense[i], rows, "channel-major")
    # time-major, three storage types
    rows = ranges(64)
    rec, nt = _records(rows, 64)
    for name, (dt, td) in DT.items():
        y = torch.full((total, Cp), SENT, dtype=td, device="cuda")
        L.check(lib.wae_upsample_stage_fwd_ranges(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(rec), len(rows), nt, x.shape[1], total, C, s, 1, Cp,
                                                  dt, None), "last stage ranges")
        dense = []
        for wh in whole:
            ref = torch.full((1, Tout, Cp), SENT, dtype=td, device="cuda")
            L.check(lib.wae_upsample_stage_fwd(L.ptr(wh.contiguous()), L.ptr(w), L.ptr(ref), 1, C, FULL, s, 1, Cp, dt, None), "last stage")
            dense.append(ref[0])
        check(y, lambda i: dense[i], rows, name)
        written = y[(y != SENT).any(dim=1)]
        assert (written[:, C:] == 0).all() and float(written[:, :C].float().abs().max()) < 1e5      # pad channels; nothing of the slack


def test_ranges_entry_skips_records_it_cannot_trust():
    """t_lo < 0, t_hi > Tin * s, a tile count that contradicts the range, columns beyond the pitch, rows beyond the output: nothing written"""
    L, lib = _lib()
    gen = torch.Generator().manual_seed(4)
    C, Cp, s = 16, 64, 4
    x, in_off, _ = _clips(C, gen)
    w = torch.randn(2 * s + 1, generator=gen).cuda()
    total = 3 * FULL * s
    rows = [(in_off[i], NOW[i], i * FULL * s, 10, 150) for i in range(3)]
    for form, shape, dt in ((1, (total, Cp), 1), (0, (C, total), 0)):
        tile = 64 if form else 256
        good, nt = _records(rows, tile)
        td = torch.bfloat16 if form else torch.float32
        want = torch.full(shape, SENT, dtype=td, device="cuda")
        L.check(lib.wae_upsample_stage_fwd_ranges(L.ptr(x), L.ptr(w), L.ptr(want), L.ptr(good), 3, nt, x.shape[1], total, C, s, form, Cp, dt,
                                                  None), "")
        for bad in ("t_lo", "t_hi", "tiles", "in_off", "out_off", "empty"):
            rec = good.clone().view(4, 6)
            if bad == "t_lo":
                rec[1, 3] = -40 if form else -106          # (the same tile count: only the sign is wrong)
            elif bad == "t_hi":
                rec[1, 1] = 30                             # t_hi 150 > Tin * s = 120
            elif bad == "tiles":
                rec[1, 4] = 150 + tile                     # one tile more than the table gives
            elif bad == "in_off":
                rec[1, 0] = x.shape[1] - 10
            elif bad == "out_off":
                rec[1, 2] = total - 100
            else:
                rec[1, 3] = 150
            got = torch.full(shape, SENT, dtype=td, device="cuda")
            L.check(lib.wae_upsample_stage_fwd_ranges(L.ptr(x), L.ptr(w), L.ptr(got), L.ptr(rec), 3, nt, x.shape[1], total, C, s, form, Cp,
                                                      dt, None), "")
            torch.cuda.synchronize()
            keep = torch.ones(total, dtype=torch.bool, device="cuda")
            keep[FULL * s:2 * FULL * s] = False
            mine, others = (got[~keep], got[keep]) if form else (got[:, ~keep], got[:, keep])
            assert (mine == SENT).all(), (form, bad)       # also where out_off moved the record: total - 100 + 150 > total
            assert _same(others, want[keep] if form else want[:, keep]), (form, bad)


# ---- 2. the session's c_up rows, as they become final -------------------------------------------------------------------------------------
NET = dict(layers=4, stacks=2, R=32, G=32, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
# per schedule three clips side by side: the frames fed per round and clip; 0: an empty feed; "end": the clip ends in a round of its
# own; (n, "end"): n frames and the end in the same round
SCHEDULES = {
    "1_2_3_frames": ([[(1, "end")], [2, "end"], [(3, "end")]]),
    "one_at_a_time": ([[1, 1, 1, 1, 1, 1, 1, "end"], [(3, "end")], [2, 0, 1, 4, "end"]]),
    "whole_and_trickle": ([[0, 0, 5, "end"], [1, 0, 0, 1, "end"], [2, 2, "end"]]),
}
_NETS = {}


def _net(dtype, cfg_name="conv_in"):
    if (dtype, cfg_name) not in _NETS:
        from wavenet_autoencoders_amd import Geometry
        from wavenet_autoencoders_amd.engine import WaeEngine
        cfg = dict(NET) if cfg_name == "conv_in" else dict(NET, conv_in=False)
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
        eng.load_state_dict(O.make_state_dict(dict(cfg), salt=11, with_encoder=False))
        eng.prepare_weights()
        _NETS[dtype, cfg_name] = eng
    return _NETS[dtype, cfg_name]


def _run_schedule(eng, sched, seed):
    gen = torch.Generator().manual_seed(seed)
    frames = lambda step: 0 if step == "end" else (step[0] if isinstance(step, tuple) else step)  # noqa: E731
    totals = [sum(frames(step) for step in s) for s in sched]
    cs = [torch.randn(NET["Cc"], F, generator=gen) * sc for F, sc in zip(totals, (1e-3, 1.0, 1e3))]
    alone = []
    for c, F in zip(cs, totals):
        o = torch.full((1, F * 640, eng.g.Ccp), SENT, dtype=eng.tdtype, device="cuda")
        eng.upsample_forward(c[None].cuda(), o)
        alone.append(o[0].clone())
    with eng.decode_session(mode="argmax") as sess:
        sess.reserve_frames(40)
        for a in sess._fa:
            a.fill_(1e6)                                   # the arenas' slack: a read past a clip's valid columns shows up
        sess._fa_cup.fill_(SENT)
        hs = [sess.open(dict(gid=1, init_idx=5)) for _ in sched]
        fa = [a.data_ptr() for a in sess._fa]
        at, got, ready = [0] * len(sched), [[] for _ in sched], [0] * len(sched)
        for r in range(max(len(s) for s in sched) + 1):
            feeds, ends = {}, []
            for i, s in enumerate(sched):
                if r < len(s) and s[r] != "end":            # (a feed of no frames is a feed)
                    n = frames(s[r])
                    feeds[hs[i]] = cs[i][:, at[i]:at[i] + n] if i % 2 else cs[i][:, at[i]:at[i] + n].cuda()
                    at[i] += n
                if r < len(s) and (s[r] == "end" or isinstance(s[r], tuple)):
                    ends.append(hs[i])
            moved = sess.feed_list(feeds)
            for i, h in enumerate(hs):
                f = sess.clips[h].feed
                want = _ready(f.frames, f.ended_planned)
                assert f.ready == want and (moved.get(h, ready[i]) == want)
                if f.ready > ready[i]:
                    got[i].append(sess.clips[h].c_up[ready[i]:f.ready].clone())     # taken as they become final
                    ready[i] = f.ready
            for h in ends:
                sess.end(h)
        assert [a.data_ptr() for a in sess._fa] == fa      # (nothing grew: the 1e6 is still the slack)
        for i, F in enumerate(totals):
            assert ready[i] == F * 640 and _same(torch.cat(got[i]), alone[i]), ("clip", i)
            assert (sess.clips[hs[i]].c_up[F * 640:] == SENT).all()                # behind the clip's last row: not written
        owned = torch.zeros(sess._fa_cup.shape[0], dtype=torch.bool, device="cuda")
        for h in hs:
            f = sess.clips[h].feed
            owned[f.base * 640:(f.base + f.cap) * 640] = True
        assert (sess._fa_cup[~owned] == SENT).all()


def _ready(F, ended):
    return F * 640 if ended else max(0, 640 * (F - 1) - 205)


@pytest.mark.parametrize("name", list(SCHEDULES))
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_session_rows_are_upsample_forward_of_the_whole_clip(dtype, name):
    # first ranges end at 435 + 640 k rows (51 past a tile edge), so every later range starts mid-tile; a range of one frame is 640 rows,
    # ten tiles exactly; the closing range is 845 rows, 13 past an edge
    _run_schedule(_net(dtype), SCHEDULES[name], seed=len(name))


def test_plain_network_and_growing_arenas():
    """UpsampleNetwork without conv_in (the frames are stage 0's input as they are), and arenas that grow while clips are open"""
    for cfg_name in ("plain", "conv_in"):
        eng = _net("bf16", cfg_name)
        gen = torch.Generator().manual_seed(3)
        cs = [torch.randn(NET["Cc"], F, generator=gen).cuda() * sc for F, sc in zip((21, 9, 12), (1.0, 1e3, 1e-3))]
        alone = []
        for c in cs:
            o = torch.empty(1, c.shape[1] * 640, eng.g.Ccp, dtype=eng.tdtype, device="cuda")
            eng.upsample_forward(c[None], o)
            alone.append(o[0].clone())
        with eng.decode_session(mode="argmax") as sess:
            hs = [sess.open(dict(gid=0, init_idx=5)) for _ in cs]
            at = [0, 0, 0]
            for step in (1, 2, 3, 5, 10):                  # clip 0 outgrows its 8 frames twice, the arenas their first size
                feeds = {}
                for i, c in enumerate(cs):
                    n = min(step, c.shape[1] - at[i])
                    if n:
                        feeds[hs[i]] = c[:, at[i]:at[i] + n]
                        at[i] += n
                sess.feed_list(feeds)
            assert at == [21, 9, 12]
            for h in hs:
                sess.end(h)
            sess.feed_list({})
            for i, h in enumerate(hs):
                assert sess.clips[h].feed.ready == alone[i].shape[0]
                assert _same(sess.clips[h].c_up[:alone[i].shape[0]], alone[i]), (cfg_name, i)


# ---- 3. decode, bit for bit ---------------------------------------------------------------------------------------------------------------
def _decoder(name, dtype, monkeypatch, coop):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, _, _, _ = golden_model(name)
    monkeypatch.setenv("WAE_AR_COOP", "1" if coop else "0")
    monkeypatch.setenv("WAE_AR_COOP_C", "8")
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    if coop and cfg.get("scalar_input"):
        eng.ar_path(scalar_coop=True)
    eng.load_state_dict(sd)
    return eng, cfg


def _draws(cfg, T, gen, mode):
    unit = lambda *s: (torch.rand(*s, generator=gen) * (1 - 2e-5) + 1e-5).cuda()  # noqa: E731
    if mode != "sample":
        return {}
    if cfg.get("scalar_input"):
        return dict(u_mix=unit(T, cfg["O"] // 3), u_log=unit(T))
    return dict(uniforms=torch.rand(T, generator=gen).cuda())


def _whole(eng, cfg, c, gid, T, mode, draws, coop):
    """incremental_forward of the whole clip alone, on the one-CU kernel or on the cooperative path"""
    kw = {k: v[None] for k, v in draws.items()}
    if not cfg.get("scalar_input"):
        kw["init_idx"] = 31
    eng._ar_profile = None
    out = eng.incremental_forward(c[None].cuda(), torch.tensor([gid]).cuda(), T, mode=mode, want_logits=True, **kw)
    torch.cuda.synchronize()
    assert (eng._ar_profile is not None) == coop
    key = "x" if cfg.get("scalar_input") else "idx"
    return out[key][0].clone(), out["logits"][0].clone()


ROUTES = [("B", "argmax", False), ("B", "sample", False), ("B", "argmax", True), ("B", "sample", True), ("S", "sample", False),
          ("S", "sample", True)]


@pytest.mark.parametrize("name,mode,coop", ROUTES, ids=[f"{n}-{m}-{'teams' if c else 'slots'}" for n, m, c in ROUTES])
def test_a_fed_clip_decodes_as_incremental_forward_of_the_whole_clip(name, mode, coop, monkeypatch):
    eng, cfg = _decoder(name, "bf16", monkeypatch, coop)
    hop = int(np.prod(cfg["upsample_scales"]))
    look = sum(int(np.prod(cfg["upsample_scales"][i:])) for i in range(1, len(cfg["upsample_scales"])))
    gen = torch.Generator().manual_seed(17)
    key = "x" if cfg.get("scalar_input") else "idx"
    F = 3
    T = F * hop
    c = torch.randn(cfg["Cc"], F, generator=gen)
    draws = _draws(cfg, T, gen, mode)
    closed = dict(T=hop, c=torch.randn(cfg["Cc"], 1, generator=gen) * 30.0, gid=2, **_draws(cfg, hop, gen, mode))
    item = dict(gid=3)
    if not cfg.get("scalar_input"):
        item["init_idx"], closed["init_idx"] = 31, 31
    want = _whole(eng, cfg, c, 3, T, mode, draws, coop)
    want_closed = _whole(eng, cfg, closed["c"], 2, hop, mode, {k: closed[k] for k in draws}, coop)
    piece = lambda a, b: {k: v[a * hop:b * hop] for k, v in draws.items()}  # noqa: E731  (the draws of the frames fed)
    parts, parts_closed, log = [], [], []
    with eng.decode_session(mode=mode, coop=coop, want_logits=True, **({"teams": 2} if coop else {"slots": 3})) as sess:
        h = sess.open(item)
        k = sess.add(closed)

        def step(n):
            res = sess.step(n)
            if h in res:
                parts.append((res[h][key].clone(), res[h]["logits"].clone()))
                assert res[h]["done"] == (h not in sess.live)
                assert res[h]["ready"] == (T if res[h]["done"] else sess.clips[h].feed.ready)
            if k in res:
                parts_closed.append((res[k][key].clone(), res[k]["logits"].clone()))
                assert "ready" not in res[k]
            log.append((int(res[h][key].shape[0]) if h in res else 0, int(res[k][key].shape[0]) if k in res else 0))

        step(100)                                          # nothing fed: the open clip sits the round out
        sess.feed(h, c[:, :1], **piece(0, 1))
        step(100)                                          # one frame makes no row final: it starves, the added clip decodes
        sess.feed(h, c[:, 1:2].cuda(), **piece(1, 2))
        assert sess.clips[h].feed.ready == hop - look
        step(hop - look - 40)
        step(100)                                          # 40 rows are left of what is final
        step(100)                                          # starves: ready == pos, absent from the result, not done
        assert h in sess.live and sess.clips[h].pos == hop - look
        sess.feed(h, c[:, 2:], **piece(2, 3))
        step(hop)
        sess.end(h)
        assert h in sess.live
        while sess.live:
            step(700)
    assert [n for n, _ in log[:6]] == [0, 0, hop - look - 40, 40, 0, hop] and log[0][1] == log[1][1] == 100
    assert sum(n for n, _ in log) == T and sum(n for _, n in log) == hop
    for i, nm in enumerate((key, "logits")):
        assert _same(torch.cat([p[i] for p in parts], -1), want[i]), (name, mode, coop, nm)
        assert _same(torch.cat([p[i] for p in parts_closed], -1), want_closed[i]), (name, mode, coop, "the added clip", nm)


def test_refusals_on_the_device_and_draws_of_the_engine(monkeypatch):
    eng, cfg = _decoder("B", "bf16", monkeypatch, False)
    hop = 320
    with eng.decode_session(mode="sample") as sess:
        h = sess.open(dict(gid=1, init_idx=3), max_T=2 * hop + 7)
        assert sess.clips[h].feed.max_frames == 2 and sess.clips[h].feed.cap == 2
        with pytest.raises(ValueError, match="clip 0 has no frames"):
            sess.end(h)
        assert sess.feed(h, torch.zeros(cfg["Cc"], 0)) == {}                   # an empty feed
        with pytest.raises(ValueError, match=r"3 frames are beyond max_T \(2 frames\)"):
            sess.feed(h, torch.zeros(cfg["Cc"], 3))
        with pytest.raises(ValueError, match="makes 215 steps final, beyond the 100 draws supplied"):
            sess.feed(h, torch.zeros(cfg["Cc"], 2), uniforms=torch.zeros(100))
        assert sess.clips[h].feed.frames == 0 and sess.step(10) == {}
        # the engine's generator draws at feed time for the rows that feed makes final
        torch.manual_seed(5)
        assert sess.feed(h, torch.randn(cfg["Cc"], 2)) == {h: 215}
        torch.manual_seed(5)
        assert torch.equal(sess.clips[h].uni, torch.rand(1, 215, device="cuda").reshape(-1))
        with pytest.raises(ValueError, match="with every feed of a clip, or with none"):
            sess.feed(h, torch.zeros(cfg["Cc"], 0), uniforms=torch.zeros(5))
        sess.end(h)
        with pytest.raises(ValueError, match="no feed after end"):
            sess.feed(h, torch.zeros(cfg["Cc"], 1))
        res = sess.step(10_000)                            # the closing ranges run in front of the round
        assert res[h]["ready"] == 640 and res[h]["idx"].shape[0] == 640 and res[h]["done"]
        assert sess.live == [] and sess._fa_top == 0


# ---- 4. launches, allocations and uploads do not grow with the clips fed ----------------------------------------------------------------
def test_feed_list_costs_the_same_for_2_and_16_clips(monkeypatch):
    eng = _net("bf16")
    counts = {}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            counts[name] = counts.get(name, 0) + 1
            return getattr(self._lib, name)

    uploads = []
    real_to = torch.Tensor.to

    def counting_to(self, *a, **kw):
        out = real_to(self, *a, **kw)
        if not self.is_cuda and out.is_cuda:
            uploads.append(tuple(self.shape))
        return out

    gen = torch.Generator().manual_seed(9)
    seen = []
    real_lib = eng.lib
    try:
        for n in (2, 16):
            with eng.decode_session(mode="argmax") as sess:
                sess.reserve(16)
                sess.reserve_frames(16 * 4)
                hs = [sess.open(dict(gid=i % 5, init_idx=5), max_T=4 * 640) for i in range(n)]
                first = {h: torch.randn(NET["Cc"], 2, generator=gen).cuda() for h in hs}
                sess.feed_list(first)                          # (every clip has rows at every stage from here on)
                feeds = {h: torch.randn(NET["Cc"], 1 + i % 2, generator=gen).cuda() for i, h in enumerate(hs)}
                torch.cuda.synchronize()
                counts.clear()
                uploads.clear()
                eng.lib = Counting(real_lib)
                monkeypatch.setattr(torch.Tensor, "to", counting_to)
                before = torch.cuda.memory_stats()["allocation.all.allocated"]
                sess.feed_list(feeds)
                allocs = torch.cuda.memory_stats()["allocation.all.allocated"] - before
                monkeypatch.setattr(torch.Tensor, "to", real_to)
                eng.lib = real_lib
                seen.append((dict(counts), allocs, len(uploads)))
    finally:
        eng.lib = real_lib
    assert seen[0] == seen[1], seen
    launches, allocs, ups = seen[0]
    assert launches == {"wae_enc_conv_fwd_list": 1, "wae_upsample_stage_fwd_ranges": 4}      # ONE conv_in, ONE launch per stage
    assert ups == 1                                            # ONE table upload (the frames were on the device)
    print(f"feed_list: {allocs} allocations per call for 2 and for 16 clips")


# ---- 5. synthesis.py ----------------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_feed_frames(tmp_path):
    from test_gpu_ar_stream import HP, _run, _tiny_dump_and_checkpoint
    dump, ckpt, preset = _tiny_dump_and_checkpoint(tmp_path)
    rng = np.random.default_rng(6)
    pairs = [("S0_0007", "V1")]
    for fid, frames, tar in (("0011", 28, "V2"), ("0012", 12, "V1")):
        utt = dump / "test" / f"S0_{fid}"
        utt.mkdir(parents=True)
        np.save(utt / "mfcc.norm.npy", rng.standard_normal((frames, 39)).astype(np.float32))
        pairs.append((f"S0_{fid}", tar))
    (tmp_path / "syn.txt").write_text("".join(f"test/{s} {t}\n" for s, t in pairs))
    (tmp_path / "spk.json").write_text(json.dumps({"V1": 2, "V2": 0}))
    outs = {}
    for dst, extra in (("rounds/", []), ("fed/", ["--feed-frames", "2"])):
        outs[dst] = _run([os.path.join(ROOT, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
                          "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7", "--batch-decode",
                          "--batch-stream", "700"] + extra, str(tmp_path))
    assert "first audio of all 3 clips after" in outs["fed/"]
    names = sorted(p.name for p in (tmp_path / "rounds" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    for n in names:
        a = (tmp_path / "rounds" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "fed" / "2019" / "english" / "test" / n).read_bytes()
        assert len(a) > 44 and a == b, n
