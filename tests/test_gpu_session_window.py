"""Sessions in constant memory on the GPU: the ring-addressed entries (wae_upsample_stage_fwd_rings, wae_enc_conv_fwd_rings) compute,
over clips that grow through rings far shorter than they are, BITWISE the rows of the dense call on the whole clip -- every range
compared right after its launch, before the ring turns again --, leave every slot they do not address at a sentinel and skip every
record they cannot trust; EncodeSession(window=W) hands out BITWISE encode_list of the whole utterance from arenas that never move,
gives the ring of an utterance that left to the next one, and costs the launches of the unwindowed session.  The rings' slack holds
1e6 in the inputs and a sentinel in the outputs; neighbouring clips differ by 1e3 in scale."""
import functools

import numpy as np
import pytest
import torch

from helpers import golden_model

pytestmark = pytest.mark.gpu
DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}
SENT, SLACK = -77.0, 3


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _records(rows, tile):
    """rows: (in_off, in_period, Tin, out_off, out_period, t_lo, t_hi) -> the device table with tile0 and the closing record, the tiles"""
    rec, nt = [], 0
    for r in rows:
        rec.append(list(r) + [nt])
        nt += -(-(r[6] - r[5]) // tile)
    rec.append([0] * 7 + [nt])
    return torch.tensor(rec, dtype=torch.int32).reshape(-1).cuda(), nt


def _ring_cols(off, period, lo, hi):
    return torch.tensor([off + t % period for t in range(lo, hi)], dtype=torch.int64, device="cuda")


# ---- 5. the upsampling entry against the dense stage of the whole clip ------------------------------------------------------------------
UPS_FULL, UPS_PERIOD, UPS_STEP = (80, 37), 8, 6


@pytest.mark.parametrize("C,Cp", [(16, 64), (80, 128)])
@pytest.mark.parametrize("s", [4, 5, 8])
def test_upsampling_rings_rows_are_the_dense_stage_of_the_whole_clip(s, C, Cp):
    L, lib = _lib()
    gen = torch.Generator().manual_seed(10 * s + C)
    rng = np.random.default_rng(s + C)
    whole = [(torch.randn(C, F, generator=gen) * sc).cuda() for F, sc in zip(UPS_FULL, (1.0, 1e3))]
    w = torch.randn(2 * s + 1, generator=gen).cuda()
    P, Po = UPS_PERIOD, s * UPS_PERIOD
    in_off = [SLACK, 2 * SLACK + P]
    out_off = [SLACK, 2 * SLACK + Po]
    in_pitch, total = 3 * SLACK + 2 * P, 3 * SLACK + 2 * Po
    dense = {"cm": []}
    for wh in whole:
        ref = torch.empty(1, C, wh.shape[1] * s, device="cuda")
        L.check(lib.wae_upsample_stage_fwd(L.ptr(wh.contiguous()), L.ptr(w), L.ptr(ref), 1, C, wh.shape[1], s, 0, Cp, 0, None), "stage")
        dense["cm"].append(ref[0])
    for name, (dt, td) in DT.items():
        dense[name] = []
        for wh in whole:
            ref = torch.full((1, wh.shape[1] * s, Cp), SENT, dtype=td, device="cuda")
            L.check(lib.wae_upsample_stage_fwd(L.ptr(wh.contiguous()), L.ptr(w), L.ptr(ref), 1, C, wh.shape[1], s, 1, Cp, dt, None), "last")
            dense[name].append(ref[0])
    x = torch.full((C, in_pitch), 1e6, device="cuda")
    y = {"cm": torch.full((C, total), SENT, device="cuda")}
    y.update({name: torch.full((total, Cp), SENT, dtype=td, device="cuda") for name, (_, td) in DT.items()})
    now, done, wraps, calls = [0, 0], [0, 0], 0, 0
    while done[0] < UPS_FULL[0] * s:
        rows = []
        for j, F in enumerate(UPS_FULL):
            if done[j] == F * s or (j == 1 and calls < 2):                   # the second clip joins two calls later: another phase
                continue
            n = min(F - now[j], UPS_STEP if calls % 3 == 0 else int(rng.integers(1, UPS_STEP + 1)))
            x[:, _ring_cols(in_off[j], P, now[j], now[j] + n)] = whole[j][:, now[j]:now[j] + n]
            now[j] += n
            hi = F * s if now[j] == F else (now[j] - 1) * s                  # (a clip whose last frame is there is run as ended)
            if hi > done[j]:
                rows.append((in_off[j], P, now[j], out_off[j], Po, done[j], hi, j))
                wraps += done[j] // Po != (hi - 1) // Po
        calls += 1
        if not rows:
            continue
        for form, tile in (("cm", 256), ("fp32", 64), ("bf16", 64), ("fp16", 64)):
            rec, nt = _records([r[:7] for r in rows], tile)
            btc = form != "cm"
            L.check(lib.wae_upsample_stage_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(y[form]), L.ptr(rec), len(rows), nt, in_pitch, total, C, s,
                                                     int(btc), Cp, DT[form][0] if btc else 0, None), "stage rings")
            for (_, _, _, oo, _, lo, hi, j) in rows:
                at = _ring_cols(oo, Po, lo, hi)
                got, want = (y[form][at], dense[form][j][lo:hi]) if btc else (y[form][:, at], dense[form][j][:, lo:hi])
                assert _same(got, want), (form, j, lo, hi)
        for r in rows:
            done[r[7]] = r[6]
    assert done == [F * s for F in UPS_FULL] and wraps >= 6                  # ranges that wrap inside a tile
    owned = torch.zeros(total, dtype=torch.bool, device="cuda")
    for oo in out_off:
        owned[oo:oo + Po] = True
    for form, out in y.items():
        rest = out[:, ~owned] if form == "cm" else out[~owned]
        assert (rest == SENT).all(), form                                    # slots never addressed keep the sentinel
        mine = out[:, owned] if form == "cm" else out[owned][:, :C]
        assert float(mine.float().abs().max()) < 1e5                         # nothing of the inputs' slack
        if form != "cm":
            assert (out[owned][:, C:] == 0).all()                            # pad channels


# ---- 6. the encoder entry against the dense call --------------------------------------------------------------------------------------------
ENC_TOUTS, ENC_STEP, ENC_OUT_PERIOD = [5, 65, 33], 7, 11


def _tin(tout, k, stride, pad):
    """the ODD input length under stride 2, else the only one, that gives tout outputs"""
    tin = (tout - 1) * stride + k - 2 * pad
    assert (tin + 2 * pad - k) // stride + 1 == tout and (stride == 1 or tin % 2 == 1)
    return tin


def _open_final(n, k, s, pad):
    return (n - k + pad) // s + 1 if n - k + pad >= 0 else 0


@pytest.mark.parametrize("et", [8, 16, 32])
@pytest.mark.parametrize("k,stride,pad", [(1, 1, 0), (3, 1, 1), (5, 2, 2), (5, 1, 2)])
def test_encoder_rings_over_growing_clips_are_the_dense_call_of_the_whole_clip(k, stride, pad, et):
    L, lib = _lib()
    dev = "cuda"
    gen = torch.Generator().manual_seed(1000 * k + 100 * stride + et)
    Tin = [_tin(t, k, stride, pad) for t in ENC_TOUTS]
    P, Po = k - 1 + ENC_STEP, ENC_OUT_PERIOD                 # the smallest ring the lag allows, plus the step
    in_off = [SLACK + j * (P + SLACK) for j in range(3)]
    out_off = [SLACK + j * (Po + SLACK) for j in range(3)]
    in_pitch, out_pitch = SLACK + 3 * (P + SLACK), SLACK + 3 * (Po + SLACK)
    shapes = [(39, 40, 0), (300, 64, 0)]
    if stride == 1 and 2 * pad == k - 1:
        shapes += [(64, 64, 1), (300, 300, 1)]
    for Cin, Cout, residual in shapes:
        whole = [(torch.randn(Cin, t, generator=gen) * (1e3 if j % 2 else 1.0)).to(dev) for j, t in enumerate(Tin)]
        w = (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).to(dev)
        b = torch.randn(Cout, generator=gen).to(dev)
        dense = []
        for j, t in enumerate(Tin):
            ref = torch.full((1, Cout, ENC_TOUTS[j]), SENT, device=dev)
            L.check(lib.wae_enc_conv_fwd(L.ptr(whole[j].contiguous()), L.ptr(w), L.ptr(b), L.ptr(ref), 1, Cin, t, Cout, k, stride, pad, 1,
                                         residual, None), "enc_conv_fwd")
            dense.append(ref[0])
        x = torch.full((Cin, in_pitch), 1e6, device=dev)
        y = torch.full((Cout, out_pitch), SENT, device=dev)
        now, done, wraps, mids, calls = [0] * 3, [0] * 3, 0, 0, 0
        while done != ENC_TOUTS:
            rows = []
            for j, t in enumerate(Tin):
                if done[j] == ENC_TOUTS[j] or calls < j:     # clip j joins at call j: three phases
                    continue
                n = min(ENC_STEP, t - now[j])
                x[:, _ring_cols(in_off[j], P, now[j], now[j] + n)] = whole[j][:, now[j]:now[j] + n]
                now[j] += n
                hi = ENC_TOUTS[j] if now[j] == t else _open_final(now[j], k, stride, pad)
                if hi > done[j]:
                    assert hi - done[j] <= Po and now[j] - max(done[j] * stride - pad, 0) <= P
                    rows.append((in_off[j], P, now[j], out_off[j], Po, done[j], hi, j))
                    wraps += done[j] // Po != (hi - 1) // Po
                    mids += done[j] % et != 0
            calls += 1
            if not rows:
                continue
            rec, nt = _records([r[:7] for r in rows], et)
            L.check(lib.wae_enc_conv_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(rec), len(rows), nt, et, in_pitch, out_pitch,
                                               Cin, Cout, k, stride, pad, 1, residual, None), "enc_conv_fwd_rings")
            # the same ranges into a linear output: this call's new columns packed (out_period 0)
            cnt = [r[6] - r[5] for r in rows]
            packed = SLACK + np.concatenate([[0], np.cumsum(cnt)[:-1]])
            lin = torch.full((Cout, int(sum(cnt)) + 2 * SLACK), SENT, device=dev)
            rec, nt = _records([(r[0], r[1], r[2], int(o), 0, r[5], r[6]) for r, o in zip(rows, packed)], et)
            L.check(lib.wae_enc_conv_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(lin), L.ptr(rec), len(rows), nt, et, in_pitch,
                                               lin.shape[1], Cin, Cout, k, stride, pad, 1, residual, None), "enc_conv_fwd_rings")
            for (_, _, _, oo, _, lo, hi, j), o in zip(rows, packed):
                assert torch.equal(y[:, _ring_cols(oo, Po, lo, hi)], dense[j][:, lo:hi]), (Cin, Cout, residual, j, lo, hi)
                assert torch.equal(lin[:, int(o):int(o) + hi - lo], dense[j][:, lo:hi]), (Cin, Cout, residual, j, lo, hi)
                done[j] = hi
            assert (lin[:, :SLACK] == SENT).all() and (lin[:, -SLACK:] == SENT).all()
        assert wraps >= 3 and mids > 0                       # rings that turned inside a range; ranges that start inside a tile
        owned = torch.zeros(out_pitch, dtype=torch.bool, device=dev)
        for oo in out_off:
            owned[oo:oo + Po] = True
        assert (y[:, ~owned] == SENT).all() and float(y[:, owned].abs().max()) < 1e5 * 1e3, (Cin, Cout, residual)
        assert float(dense[0].abs().max()) < 1e5 and float(y[:, out_off[0]:out_off[0] + Po].abs().max()) < 1e5      # not the 1e3 neighbour's


# ---- 7. records the kernels must skip -----------------------------------------------------------------------------------------------------
def test_entries_skip_the_records_they_cannot_trust():
    """Every bad record stays inside this test's own buffers even for a kernel that accepted it: the clips lie LINEAR in buffers with
    a spare row of channels in front and behind, so a missing check is a failed assertion here, never a fault."""
    L, lib = _lib()
    dev = "cuda"
    gen = torch.Generator().manual_seed(3)
    # -- the encoder entry: three clips of 129 columns, ranges [2, 20) in three tiles of 8
    Cin, Cout, k, s, pad, et, T = 39, 40, 5, 2, 2, 8, 129
    in_off, out_off, in_pitch, out_pitch = [4, 140, 280], [3, 75, 150], 420, 220
    xbuf = torch.full((Cin + 2, in_pitch), 1e6)
    for o in in_off:
        xbuf[1:-1, o:o + T] = torch.randn(Cin, T, generator=gen)
    xbuf = xbuf.to(dev)
    x, w, b = xbuf[1:-1], (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).to(dev), torch.randn(Cout, generator=gen).to(dev)
    rows = [(in_off[i], T, T, out_off[i], 64, 2, 20) for i in range(3)]

    def enc(rec, nt):
        ybuf = torch.full((Cout + 2, out_pitch), SENT, device=dev)
        rc = lib.wae_enc_conv_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(ybuf[1:-1]), L.ptr(rec), 3, nt, et, in_pitch, out_pitch, Cin,
                                        Cout, k, s, pad, 1, 0, None)
        torch.cuda.synchronize()
        assert rc == 0
        return ybuf

    good, nt = _records(rows, et)
    want = enc(good, nt)
    mine = torch.zeros(out_pitch, dtype=torch.bool, device=dev)
    mine[out_off[1]:out_off[1] + 64] = True
    assert nt == 9 and not (want[1:-1, out_off[1] + 2:out_off[1] + 20] == SENT).any() and (want[[0, -1]] == SENT).all()
    cases = {
        "aliasing": {1: 8},                          # the first tap of t_lo = 2 is column 2 < Tin - in_period = 121
        "aliasing_by_one": {1: T - 3},               # 2 * 2 - 2 = 2 < 129 - 126 = 3
        "range_longer_than_the_ring": {4: 17},       # 18 outputs into a ring of 17
        "in_period_0": None,
        "in_period_beyond_pitch": {1: in_pitch - in_off[1] + 1},
        "out_period_beyond_pitch": {4: out_pitch - out_off[1] + 1},
        "linear_beyond_pitch": {3: out_pitch - 17, 4: 0},
        "out_period_negative": {4: -64},
        "in_off_negative": {0: -1},
        "out_off_negative": {3: -1},
        "tile_count": {6: 28},                       # four tiles where the table gives three; 28 <= Tout
        "Tin_0": {2: 0},
        "t_hi_beyond_Tout": {2: 31},                 # t_hi 20 > (31 + 4 - 5) / 2 + 1 = 16
        "t_lo_at_t_hi": {5: 20},
    }
    for name, change in cases.items():
        if change is None:                           # (a period of 0 would divide by zero in a kernel without the check: not run)
            continue
        rec = good.clone().view(4, 8)
        for col, v in change.items():
            rec[1, col] = v
        got = enc(rec.reshape(-1), nt)
        assert (got[:, mine] == SENT).all() and (got[[0, -1]] == SENT).all(), name
        assert torch.equal(got[:, ~mine], want[:, ~mine]), name
    # -- the upsampling entry, both forms: three clips of 60 frames, rows [10, 150)
    C, Cp, s, F = 16, 64, 4, 60
    in_off, in_pitch, total = [3, 70, 140], 210, 3 * F * s
    xbuf = torch.full((C + 2, in_pitch), 1e6)
    for o in in_off:
        xbuf[1:-1, o:o + F] = torch.randn(C, F, generator=gen)
    xbuf = xbuf.to(dev)
    x, w = xbuf[1:-1], torch.randn(2 * s + 1, generator=gen).to(dev)
    rows = [(in_off[i], F, F, i * F * s, F * s, 10, 150) for i in range(3)]
    for form, dt, td, tile in ((1, 1, torch.bfloat16, 64), (0, 0, torch.float32, 256)):
        def ups(rec, nt):
            ybuf = torch.full((total + 2 * 64, Cp) if form else (C + 2, total), SENT, dtype=td, device=dev)
            out = ybuf[64:-64] if form else ybuf[1:-1]
            rc = lib.wae_upsample_stage_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(out), L.ptr(rec), 3, nt, in_pitch, total, C, s, form, Cp, dt,
                                                  None)
            torch.cuda.synchronize()
            assert rc == 0
            return ybuf, out

        good, nt = _records(rows, tile)
        wbuf, want = ups(good, nt)
        keep = torch.ones(total, dtype=torch.bool, device=dev)
        keep[F * s:2 * F * s] = False
        cases = {
            "aliasing": {1: 8},                      # the first frame of t_lo = 10 is frame 1 < Tin - in_period = 52
            "aliasing_by_one": {1: F - 2},           # 1 < 60 - 58
            "range_longer_than_the_ring": {4: 139},
            "in_period_beyond_pitch": {1: in_pitch - in_off[1] + 1},
            "out_period_beyond_rows": {4: total - F * s + 1},
            "out_period_0": None,
            "in_off_negative": {0: -1},
            "out_off_negative": {3: -1},
            "tile_count": {6: 150 + tile},
            "t_lo_negative": {5: -40 if form else -106},
            "t_hi_beyond_Tout": {2: 30},
            "empty": {5: 150},
        }
        for name, change in cases.items():
            if change is None:
                continue
            rec = good.clone().view(4, 8)
            for col, v in change.items():
                rec[1, col] = v
            gbuf, got = ups(rec.reshape(-1), nt)
            rest, others = (got[~keep], got[keep]) if form else (got[:, ~keep], got[:, keep])
            assert (rest == SENT).all(), (form, name)
            assert _same(others, want[keep] if form else want[:, keep]), (form, name)
            assert (gbuf[:64] == SENT).all() and (gbuf[-64:] == SENT).all() if form else (gbuf[[0, -1]] == SENT).all(), (form, name)
    # refused before any launch, as the ranges entries
    y = torch.full((Cout, out_pitch), SENT, device=dev)
    for kw, code in ((dict(nrecs=0), -1), (dict(ntiles=0), -1), (dict(et=12), -1), (dict(k=7, pad=3), -2)):
        a = dict(nrecs=3, ntiles=9, et=8, k=5, pad=2)
        a.update(kw)
        rc = lib.wae_enc_conv_fwd_rings(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(good), a["nrecs"], a["ntiles"], a["et"], in_pitch, out_pitch,
                                        C, Cout, a["k"], 2, a["pad"], 1, 0, None)
        torch.cuda.synchronize()
        assert rc == code and (y == SENT).all(), kw


# ---- 8. the encode session ----------------------------------------------------------------------------------------------------------------
FS = [129, 200, 7, 37]                                      # the fourth joins once the third -- the middle one -- has left


@functools.lru_cache(maxsize=None)
def _setup():
    """engine on the weights of golden_model("A") (the geometry of test_gpu_encode_session._setup), the utterances and encode_list's
    answer per utterance, once"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, _, _, _ = golden_model("A")
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    eng.prepare_weights()
    gen = torch.Generator().manual_seed(7)
    items = [torch.randn(cfg["c_in"], F, generator=gen) * (1e3 if i % 2 else 1.7) for i, F in enumerate(FS)]
    whole = []
    for it in items:
        r = eng.encode_list([it], want_latents=True)[0]
        whole.append({k: r[k].clone() for k in ("quant", "idx", "latents")})
    return eng, cfg, items, whole


def _chunks(name, F, max_feed, rng):
    if name in ("1", "3"):
        n = int(name)
        return [n] * (F // n) + ([F % n] if F % n else [])
    out = []
    while sum(out) < F:
        out.append(int(min(max_feed if name == "max_feed" else rng.integers(1, max_feed + 1), F - sum(out))))
    return out


@pytest.mark.parametrize("schedule", ["1", "3", "max_feed", "random"])
@pytest.mark.parametrize("window", [16, 32])
def test_windowed_session_chunks_are_encode_list_of_the_whole_utterance(window, schedule):
    from wavenet_autoencoders_amd import packing as PK
    eng, cfg, items, whole = _setup()
    rng = np.random.default_rng(window + len(schedule))
    got = [dict(quant=[], idx=[], latents=[]) for _ in FS]
    with eng.encode_session(want_latents=True, window=window) as sess:
        assert sess.max_feed == PK.enc_window_max_feed(window) == window - 8
        plans = [_chunks(schedule, F, sess.max_feed, rng) for F in FS]
        hs, fed, step, ended = {}, [0] * len(FS), [0] * len(FS), [False] * len(FS)
        arenas, r = None, 0
        while not all(ended):
            feeds, ends = {}, []
            for i, F in enumerate(FS):
                if i not in hs and (i < 3 and r == i or i == 3 and ended[2]):
                    hs[i] = sess.open(max_frames=F if i == 0 else None)
                    if i == 3:                               # the ring the middle utterance left, while its neighbours are open
                        assert sess.clips[hs[3]].slot == slot_of_2 and not ended[0] and not ended[1]
                if i not in hs or ended[i]:
                    continue
                if step[i] < len(plans[i]):
                    n = plans[i][step[i]]
                    piece = items[i][:, fed[i]:fed[i] + n]
                    feeds[hs[i]] = piece.cuda() if i % 2 == 0 else piece.numpy()
                    fed[i] += n
                    step[i] += 1
                    if fed[i] == F and i % 2 == 0:           # ends with its last frames; the others in a call of their own
                        ends.append(hs[i])
                else:
                    ends.append(hs[i])
            if 2 in hs and not ended[2]:
                slot_of_2 = sess.clips[hs[2]].slot
            res = sess.feed_list(feeds, ended=ends)
            if arenas is None:
                arenas = [(a.data_ptr(), tuple(a.shape)) for a in sess._ar]
            assert set(res) == set(feeds) | set(ends)
            for i in range(len(FS)):
                out = res.get(hs.get(i))
                if out is None:
                    continue
                done = hs[i] in ends
                assert out["done"] == done and out["final"] == PK.enc_ready(fed[i], done)
                for key in got[i]:
                    got[i][key].append(out[key].clone())
                ended[i] = done
            r += 1
        assert sess.live == []
        assert [(a.data_ptr(), tuple(a.shape)) for a in sess._ar] == arenas   # nothing moved, nothing grew: four rings from the first feed on
        chans = [eng.lay.shapes[f"encoder.net.{i}.conv.weight"][1] for i in range(10)] + [eng.lay.shapes["encoder.lin.weight"][1]]
        assert sess.arena_bytes == 4 * 4 * sum(c * p for c, p in zip(chans, PK.enc_ring_periods(window)))      # 4 rings x 4 bytes
        assert max(FS) > 4 * window                          # the rings turned many times
    for i, want in enumerate(whole):
        for key in ("quant", "latents"):
            assert torch.equal(torch.cat(got[i][key], dim=1), want[key]), (window, schedule, FS[i], key)
        assert torch.equal(torch.cat(got[i]["idx"]), want["idx"]), (window, schedule, FS[i])


def test_windowed_session_refusals_on_the_device_leave_it_as_it_was():
    eng, cfg, items, whole = _setup()
    x = items[FS.index(37)]
    with eng.encode_session(window=16) as sess:
        h = sess.open()
        a = sess.feed(h, x[:, :8])
        with pytest.raises(ValueError, match=r"a feed of 9 frames; a window of 16 admits max_feed = 8 per call"):
            sess.feed(h, x[:, 8:17])
        parts = [a] + [sess.feed(h, x[:, lo:lo + 8]) for lo in (8, 16, 24)] + [sess.feed_list({h: x[:, 32:]}, ended=(h,))[h]]
        assert parts[-1]["done"] and sess.live == []
        assert torch.equal(torch.cat([p["quant"] for p in parts], dim=1), whole[FS.index(37)]["quant"])
        assert torch.equal(torch.cat([p["idx"] for p in parts]), whole[FS.index(37)]["idx"])


# ---- 10. cost per call ---------------------------------------------------------------------------------------------------------------------
def test_windowed_feed_list_costs_the_same_for_2_and_16_clips_and_no_more_than_unwindowed(monkeypatch):
    eng, cfg, _, _ = _setup()
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
    seen = {}
    real_lib = eng.lib
    try:
        for window in (16, None):
            for n in (2, 16):
                with eng.encode_session(window=window) as sess:
                    if window is None:
                        sess.reserve_frames(16 * 24)
                    else:
                        sess.reserve_slots(16)
                    hs = [sess.open(max_frames=24) for _ in range(n)]
                    for lo in (0, 8, 16):                    # 20 frames each, within max_feed per call
                        sess.feed_list({h: torch.randn(cfg["c_in"], min(8, 20 - lo), generator=gen).cuda() for h in hs})
                    feeds = {h: torch.randn(cfg["c_in"], 1, generator=gen).cuda() for h in hs}   # 20 -> 21 frames: a new latent each
                    torch.cuda.synchronize()
                    counts.clear()
                    uploads.clear()
                    allocs = torch.cuda.memory_stats()["allocation.all.allocated"]
                    eng.lib = Counting(real_lib)
                    monkeypatch.setattr(torch.Tensor, "to", counting_to)
                    res = sess.feed_list(feeds)
                    monkeypatch.setattr(torch.Tensor, "to", real_to)
                    eng.lib = real_lib
                    allocs = torch.cuda.memory_stats()["allocation.all.allocated"] - allocs
                    assert all(r["quant"].shape[1] == 1 and r["final"] == 2 for r in res.values()) and len(res) == n
                    seen[window, n] = (dict(counts), len(uploads), allocs)
    finally:
        eng.lib = real_lib
    assert seen[16, 2] == seen[16, 16], seen
    launches, ups, allocs = seen[16, 2]
    assert launches == {"wae_enc_conv_fwd_rings": 11, "wae_vq_nearest": 1}       # one launch per layer, one quantiser call; no move
    assert ups == 1                                                              # ONE table upload (the frames were on the device)
    flat, flat_ups, flat_allocs = seen[None, 2]
    assert sum(launches.values()) <= sum(flat.values()) and ups <= flat_ups and allocs <= flat_allocs


# ---- 9. the decode session ------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(dtype, scales):
    """test_gpu_session_feed's NET with other scales"""
    from oracle import wae_oracle as O
    from test_gpu_session_feed import NET
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    if (dtype, tuple(scales)) not in _NETS:
        cfg = dict(NET, upsample_scales=list(scales))
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
        eng.load_state_dict(O.make_state_dict(dict(cfg), salt=11, with_encoder=False))
        eng.prepare_weights()
        _NETS[dtype, tuple(scales)] = eng
    return _NETS[dtype, tuple(scales)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("scales,F", [([2, 3], 30), ([4, 4, 8, 5], 12)], ids=["2x3", "4x4x8x5"])
def test_windowed_session_rows_are_upsample_forward_of_the_whole_clip(scales, F, dtype):
    from test_gpu_session_feed import NET
    from wavenet_autoencoders_amd import packing as PK
    eng, W = _net(dtype, scales), 4
    prod, look = PK.feed_lookahead(scales)
    gen = torch.Generator().manual_seed(F)
    rng = np.random.default_rng(F)
    cs = [torch.randn(NET["Cc"], n, generator=gen) * sc for n, sc in ((F, 1.0), (F - 5, 1e3))]
    alone = []
    for c in cs:
        o = torch.full((1, c.shape[1] * prod, eng.g.Ccp), SENT, dtype=eng.tdtype, device="cuda")
        eng.upsample_forward(c[None].cuda(), o)
        alone.append(o[0].clone())
    with eng.decode_session(mode="argmax", window=W) as sess:
        assert sess.max_feed == PK.feed_window_max_feed(scales, W) == 2
        sess.reserve_frames(2 * W)
        for a in sess._fa:
            a.fill_(1e6)                                     # a read of a slot that was never written shows up
        cup, bytes_ = sess._fa_cup.data_ptr(), sess.arena_bytes
        assert bytes_ == 2 * W * (4 * NET["Cc"] * sum(int(np.prod(scales[:i])) for i in range(len(scales)))
                                  + prod * eng.g.Ccp * sess._fa_cup.element_size())
        hs = [sess.open(dict(gid=1, init_idx=5)) for _ in cs]
        whole = sess.add(dict(T=prod, c=cs[0][:, :1], gid=2, init_idx=5))      # a clip joined whole shares the session
        at, ready, ended, rose, fell = [0, 0], [0, 0], [False, False], 0, 0
        while any(h in sess.live for h in hs):
            feeds = {}
            for i, h in enumerate(hs):
                if h not in sess.live or ended[i]:
                    continue
                room = sess.room(h)
                n = min(room, cs[i].shape[1] - at[i], int(rng.integers(1, 3)))
                if n:
                    feeds[h] = cs[i][:, at[i]:at[i] + n] if i else cs[i][:, at[i]:at[i] + n].cuda()
                    at[i] += n
            before = {h: sess.room(h) for h in feeds}
            sess.feed_list(feeds)
            assert all(sess.room(h) <= before[h] for h in feeds)         # a feed never makes room ...
            fell += sum(sess.room(h) < before[h] for h in feeds)         # ... and takes it once the backlog, not max_feed, bounds it
            for i, h in enumerate(hs):
                if h not in sess.live:
                    continue
                f, c = sess.clips[h].feed, sess.clips[h]
                if at[i] == cs[i].shape[1] and not f.ended and f.frames * prod - c.pos <= W * prod:
                    sess.end(h)
                    ended[i] = True
                r = f.frames * prod if f.ended else PK.feed_ready(f.frames, scales, False)
                if r > ready[i]:                             # every row, read while it is held
                    assert _same(sess.cond_rows(h, ready[i], r), alone[i][ready[i]:r]), (i, ready[i], r)
                    ready[i] = r
            rooms = {h: sess.room(h) for h in hs if h in sess.live}
            sess.step(prod)                                  # slower than the feeds: the backlog, not max_feed, comes to bound the room
            rose += sum(sess.room(h) > rooms[h] for h in rooms if h in sess.live)
        assert ready == [c.shape[1] * prod for c in cs] and rose > 3 and fell > 3 and whole not in sess.live
        assert sess._fa_cup.data_ptr() == cup and sess.arena_bytes == bytes_ and F >= 3 * W        # the rings turned at least three times
        # rows the ring has turned over are refused, and so is a feed beyond the room
        h = sess.open(dict(gid=1, init_idx=5))
        for _ in range(4):
            sess.feed(h, cs[0][:, :1])
            sess.step(10 ** 6)
        assert sess.room(h) > 0
        held = sess.clips[h].feed.ready
        state = (sess.clips[h].feed.frames, held, sess.clips[h].pos)
        with pytest.raises(ValueError, match="a feed of 3 frames; a window of 4 admits max_feed = 2"):
            sess.feed(h, cs[0][:, :3])
        sess.feed(h, cs[0][:, :2])
        sess.feed(h, cs[0][:, :2])
        with pytest.raises(ValueError, match="would overwrite conditioning rows it has not decoded"):
            sess.feed(h, cs[0][:, :2])
        assert sess.clips[h].feed.frames == state[0] + 4 and sess.clips[h].pos == state[2]      # the refused feed left it as it was
        with pytest.raises(ValueError, match="holds the rows"):
            sess.cond_rows(h, 0, 1) if sess.clips[h].feed.ready > W * prod else sess.cond_rows(h, 0, sess.clips[h].feed.ready + 1)


ROUTES = [("B", "argmax", False), ("B", "sample", False), ("B", "argmax", True), ("B", "sample", True), ("S", "sample", False),
          ("S", "sample", True)]         # test_gpu_session_feed.ROUTES


@pytest.mark.parametrize("name,mode,coop", ROUTES, ids=[f"{n}-{m}-{'teams' if c else 'slots'}" for n, m, c in ROUTES])
def test_windowed_fed_clips_decode_as_incremental_forward_of_the_whole_clip(name, mode, coop, monkeypatch):
    """the routes of test_gpu_session_feed.ROUTES, the open clip in a ring of 4 frames that turns twice"""
    from test_gpu_session_feed import ROUTES as THEIRS, _decoder, _draws, _whole
    from wavenet_autoencoders_amd import packing as PK
    assert ROUTES == THEIRS
    if True:
        eng, cfg = _decoder(name, "bf16", monkeypatch, coop)
        scales = cfg["upsample_scales"]
        hop = int(np.prod(scales))
        gen = torch.Generator().manual_seed(17)
        key = "x" if cfg.get("scalar_input") else "idx"
        F, W = 9, 4
        T = F * hop
        c = torch.randn(cfg["Cc"], F, generator=gen)
        draws = _draws(cfg, T, gen, mode)
        closed = dict(T=hop, c=torch.randn(cfg["Cc"], 1, generator=gen) * 30.0, gid=2, **_draws(cfg, hop, gen, mode))
        item = dict(gid=3)
        if not cfg.get("scalar_input"):
            item["init_idx"], closed["init_idx"] = 31, 31
        want = _whole(eng, cfg, c, 3, T, mode, draws, coop)
        want_closed = _whole(eng, cfg, closed["c"], 2, hop, mode, {k: closed[k] for k in draws}, coop)
        parts, parts_closed, fed, rounds = [], [], 0, 0
        with eng.decode_session(mode=mode, coop=coop, want_logits=True, window=W, **({"teams": 2} if coop else {"slots": 3})) as sess:
            assert W >= PK.feed_window_min(scales)
            h = sess.open(item)
            k = sess.add(closed)
            while h in sess.live:
                n = min(sess.room(h), F - fed, 1 + rounds % 2)
                if n:
                    sess.feed(h, c[:, fed:fed + n], **{kk: v[fed * hop:(fed + n) * hop] for kk, v in draws.items()})
                    fed += n
                f = sess.clips[h].feed
                if fed == F and not f.ended and T - sess.clips[h].pos <= W * hop:
                    sess.end(h)
                res = sess.step(hop // 2 + 7 * rounds)
                rounds += 1
                if h in res:
                    parts.append((res[h][key].clone(), res[h]["logits"].clone()))
                if k in res:
                    parts_closed.append((res[k][key].clone(), res[k]["logits"].clone()))
                if h in sess.live and mode == "sample":      # the draws step() has consumed are dropped
                    cl = sess.clips[h]
                    held = cl.draw if cfg.get("scalar_input") else cl.uni
                    assert held.shape[0] == cl.feed.drawn - cl.feed.doff and cl.feed.doff <= cl.pos
                    assert cl.pos - cl.feed.doff < max(cl.feed.drawn - cl.pos, 256)
            while sess.live:
                res = sess.step(700)
                if k in res:
                    parts_closed.append((res[k][key].clone(), res[k]["logits"].clone()))
        assert fed == F
        for i, nm in enumerate((key, "logits")):
            assert _same(torch.cat([p[i] for p in parts], -1), want[i]), (name, mode, coop, nm)
            assert _same(torch.cat([p[i] for p in parts_closed], -1), want_closed[i]), (name, mode, coop, "the added clip", nm)


def test_windowed_decode_feed_list_costs_the_same_for_2_and_16_clips_and_no_more_than_unwindowed(monkeypatch):
    from test_gpu_session_feed import NET
    eng = _net("bf16", [4, 4, 8, 5])
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
    seen = {}
    real_lib = eng.lib
    try:
        for window in (4, None):
            for n in (2, 16):
                with eng.decode_session(mode="argmax", window=window) as sess:
                    sess.reserve(16)
                    sess.reserve_frames(16 * 4)
                    hs = [sess.open(dict(gid=i % 5, init_idx=5), max_T=4 * 640) for i in range(n)]
                    sess.feed_list({h: torch.randn(NET["Cc"], 2, generator=gen).cuda() for h in hs})
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
                    seen[window, n] = (dict(counts), allocs, len(uploads))
    finally:
        eng.lib = real_lib
    assert seen[4, 2] == seen[4, 16], seen
    launches, allocs, ups = seen[4, 2]
    assert launches == {"wae_enc_conv_fwd_list": 1, "wae_upsample_stage_fwd_rings": 4}       # ONE conv_in, ONE launch per stage; no move
    flat, flat_allocs, flat_ups = seen[None, 2]
    assert ups == 1 and sum(launches.values()) <= sum(flat.values()) and allocs <= flat_allocs and ups <= flat_ups


# ---- 11. synthesis.py -----------------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_batch_window(tmp_path):
    import json
    import os
    from test_gpu_ar_stream import HP, _run, _tiny_dump_and_checkpoint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    for dst, extra in (("fed/", ["--feed-features", "5"]), ("ring/", ["--feed-features", "5", "--batch-window", "4"])):
        outs[dst] = _run([os.path.join(root, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
                          "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7", "--batch-decode",
                          "--batch-stream", "700"] + extra, str(tmp_path))
    assert "first audio of all 3 clips after" in outs["ring/"]
    names = sorted(p.name for p in (tmp_path / "fed" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    for n in names:
        a = (tmp_path / "fed" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "ring" / "2019" / "english" / "test" / n).read_bytes()
        assert len(a) > 44 and a == b, n
