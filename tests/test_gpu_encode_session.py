"""Encode sessions on the GPU (fp32): wae_enc_conv_fwd_ranges computes, over successive calls with a growing Tin and ranges that start
in the middle of a tile, BITWISE the columns wae_enc_conv_fwd writes for the whole clip, skips every record it cannot trust, and
EncodeSession's chunks, concatenated, are BITWISE encode_list of the whole utterance -- whatever the feeding, with arenas that grow
and clips that relocate; one call costs the same for 2 and for 16 clips; its `quant` chunks drive DecodeSession.feed_list to the
bits of incremental_forward on the whole clip; synthesis.py --feed-features writes the wavs of --batch-stream alone.  Neighbouring
clips differ by 1e3 in scale and the slack (and every column that has not arrived yet) holds 1e6 in x, a sentinel in y."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from helpers import golden_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL, SLACK = -12345.5, 5
TOUTS = [1, 9, 33, 65]
GROW = [1, 7, 20, 45, 100]                          # inputs valid at the successive calls (those below the clip's length), then the end


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _tin(tout, k, stride, pad):
    """the ODD input length under stride 2, else the only one, that gives tout outputs"""
    tin = (tout - 1) * stride + k - 2 * pad
    assert (tin + 2 * pad - k) // stride + 1 == tout and (stride == 1 or tin % 2 == 1)
    return tin


def _open_final(n, k, s, pad):
    return (n - k + pad) // s + 1 if n - k + pad >= 0 else 0


def _table(rows, et):
    """rows: (in_off, Tin, out_col, t_lo, t_hi) -> the device table with tile0 and the closing record, and the tile count"""
    rec, nt = [], 0
    for r in rows:
        rec.append(list(r) + [nt])
        nt += -(-(r[4] - r[3]) // et)
    rec.append([0, 0, 0, 0, 0, nt])
    return torch.tensor(rec, dtype=torch.int32).reshape(-1).cuda(), nt


# ---- 1. the raw entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("et", [8, 16, 32])
@pytest.mark.parametrize("k,stride,pad", [(1, 1, 0), (3, 1, 1), (5, 2, 2), (5, 1, 2)])
def test_ranges_over_growing_clips_are_the_dense_call_of_the_whole_clip(k, stride, pad, et):
    L, lib = _lib()
    dev = "cuda"
    gen = torch.Generator().manual_seed(1000 * k + 100 * stride + et)
    Tin = [_tin(t, k, stride, pad) for t in TOUTS]
    in_off = [SLACK + sum(Tin[:i]) + i * SLACK for i in range(len(Tin))]
    out_off = [SLACK + sum(TOUTS[:i]) + i * SLACK for i in range(len(Tin))]
    in_pitch, out_pitch = in_off[-1] + Tin[-1] + SLACK, out_off[-1] + TOUTS[-1] + SLACK
    shapes = [(39, 40, 0), (300, 64, 0)]
    if stride == 1 and 2 * pad == k - 1:
        shapes += [(64, 64, 1), (300, 300, 1)]
    steps = sorted({n for n in GROW if n < max(Tin)})
    for Cin, Cout, residual in shapes:
        whole = [torch.randn(Cin, t, generator=gen) * (1e3 if j % 2 else 1.0) for j, t in enumerate(Tin)]
        w = (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).to(dev)
        b = torch.randn(Cout, generator=gen).to(dev)
        y = torch.full((Cout, out_pitch), SENTINEL, device=dev)
        done = [0] * len(Tin)
        mids = 0
        for n in steps + [None]:                    # None: every clip has ended
            x = torch.full((Cin, in_pitch), 1e6)    # the slack, and every column that has not arrived
            rows = []
            for j, t in enumerate(Tin):
                now = t if n is None else min(n, t)
                ended = n is None or n >= t         # (a clip whose last column is there is run as ended: its Tout is known)
                x[:, in_off[j]:in_off[j] + now] = whole[j][:, :now]
                hi = TOUTS[j] if ended else _open_final(now, k, stride, pad)
                if hi > done[j]:
                    rows.append((in_off[j], now, out_off[j] + done[j], done[j], hi))
                    mids += done[j] % et != 0
                    done[j] = hi
            if not rows:
                continue
            rec, nt = _table(rows, et)
            L.check(lib.wae_enc_conv_fwd_ranges(L.ptr(x.to(dev)), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(rec), len(rows), nt, et, in_pitch,
                                                out_pitch, Cin, Cout, k, stride, pad, 1, residual, None), "enc_conv_fwd_ranges")
        assert done == TOUTS and mids > 0           # some range started in the middle of a tile
        owned = torch.zeros(out_pitch, dtype=torch.bool, device=dev)
        for j, t in enumerate(Tin):
            ref = torch.full((1, Cout, TOUTS[j]), SENTINEL, device=dev)
            L.check(lib.wae_enc_conv_fwd(L.ptr(whole[j].to(dev).contiguous()), L.ptr(w), L.ptr(b), L.ptr(ref), 1, Cin, t, Cout, k, stride,
                                         pad, 1, residual, None), "enc_conv_fwd")
            assert torch.equal(y[:, out_off[j]:out_off[j] + TOUTS[j]], ref[0]), (Cin, Cout, residual, j)
            assert float(ref.abs().max()) < 1e5 * (1e3 if j % 2 else 1.0)
            owned[out_off[j]:out_off[j] + TOUTS[j]] = True
        assert (y[:, ~owned] == SENTINEL).all(), (Cin, Cout, residual)


# ---- 2. records the kernel cannot trust ---------------------------------------------------------------------------------------------------
def test_entry_skips_untrusted_records_and_refuses_bad_arguments():
    L, lib = _lib()
    dev = "cuda"
    gen = torch.Generator().manual_seed(3)
    Cin, Cout, k, s, pad, et = 39, 40, 5, 2, 2, 8
    T, To = 129, 65
    in_off, out_off = [4, 140, 280], [3, 75, 150]
    in_pitch, out_pitch = 420, 220
    x = torch.full((Cin, in_pitch), 1e6)
    for o in in_off:
        x[:, o:o + T] = torch.randn(Cin, T, generator=gen)
    x, w, b = x.to(dev), (torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5).to(dev), torch.randn(Cout, generator=gen).to(dev)
    rows = [(in_off[i], T, out_off[i] + 2, 2, 20) for i in range(3)]         # three tiles each: [2, 10), [10, 18), [18, 20)

    def run(rec, nt, **kw):
        a = dict(x=x, w=w, y=torch.full((Cout, out_pitch), SENTINEL, device=dev), nrecs=3, ntiles=nt, et=et, in_pitch=in_pitch,
                 out_pitch=out_pitch, Cin=Cin, Cout=Cout, k=k, stride=s, pad=pad, residual=0)
        a.update(kw)
        rc = lib.wae_enc_conv_fwd_ranges(L.ptr(a["x"]), L.ptr(a["w"]), L.ptr(b), L.ptr(a["y"]), L.ptr(rec), a["nrecs"], a["ntiles"], a["et"],
                                         a["in_pitch"], a["out_pitch"], a["Cin"], a["Cout"], a["k"], a["stride"], a["pad"], 1, a["residual"], None)
        torch.cuda.synchronize()
        return rc, a["y"]

    good, nt = _table(rows, et)
    rc, want = run(good, nt)
    assert rc == 0 and nt == 9 and not (want[:, out_off[1] + 2:out_off[1] + 20] == SENTINEL).any()
    mine = torch.zeros(out_pitch, dtype=torch.bool, device=dev)
    mine[out_off[1] + 2:out_off[1] + 20] = True
    cases = {
        "Tin_0": {1: 0},
        "t_lo_negative": {3: -6, 4: 12},             # (the same tile count: only the sign is wrong)
        "t_lo_at_t_hi": {3: 20},
        "t_hi_beyond_Tout": {1: 31},                 # t_hi 20 > (31 + 4 - 5) / 2 + 1 = 16
        "tile_count": {4: 28},                       # four tiles where the table gives three; 28 <= Tout
        "in_off_negative": {0: -1},
        "in_off_beyond_pitch": {0: in_pitch - T + 1},
        "out_col_negative": {2: -1},
        "out_col_beyond_pitch": {2: out_pitch - 17},
    }
    for name, change in cases.items():
        rec = good.clone().view(4, 6)
        for col, v in change.items():
            rec[1, col] = v
        rc, got = run(rec.reshape(-1), nt)
        assert rc == 0, name
        assert (got[:, mine] == SENTINEL).all(), name
        assert torch.equal(got[:, ~mine], want[:, ~mine]), name
    # refused before any launch
    for kw, code in ((dict(x=None), -1), (dict(nrecs=0), -1), (dict(ntiles=0), -1), (dict(et=12), -1), (dict(out_pitch=0), -1),
                     (dict(residual=1), -1), (dict(k=7, pad=3), -2), (dict(k=3, stride=2, pad=1), -2)):
        rc, got = run(good, nt, **kw)
        assert rc == code and (got == SENTINEL).all(), kw


# ---- 3. the session against the whole clip ----------------------------------------------------------------------------------------------
FS = [1, 2, 4, 5, 12, 13, 16, 17, 20, 21, 37, 129]


@functools.lru_cache(maxsize=None)
def _setup():
    """engine on the weights of golden_model("A"), the utterances, and per utterance encode_list's and the dense calls' answer, once"""
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
        lat = eng.encoder_forward(it[None].cuda())
        quant, idx, _ = eng.vq_forward(lat)
        assert torch.equal(r["latents"], lat[0]) and torch.equal(r["quant"], quant[0]) and torch.equal(r["idx"], idx)
        whole.append({k: r[k].clone() for k in ("quant", "idx", "latents")})
    return eng, cfg, items, whole


def _chunks(name, F, rng):
    if name == "one_frame_per_call":
        return [1] * F
    if name == "all_in_one_call":
        return [F]
    out = []
    while sum(out) < F:
        out.append(int(min(rng.integers(1, 12), F - sum(out))))
    return out


@pytest.mark.parametrize("schedule", ["one_frame_per_call", "random_chunks", "all_in_one_call"])
def test_session_chunks_are_encode_list_of_the_whole_utterance(schedule):
    from wavenet_autoencoders_amd import packing as PK
    eng, cfg, items, whole = _setup()
    rng = np.random.default_rng(len(schedule))
    plans = [_chunks(schedule, F, rng) for F in FS]
    # "all at once" ends in the same call; otherwise alternate between ending with the last frames and in a call of its own
    same_call = [schedule == "all_in_one_call" or i % 2 == 0 for i in range(len(FS))]
    start = [i % 3 for i in range(len(FS))]                                  # the round at which the utterance joins
    got = [dict(quant=[], idx=[], latents=[]) for _ in FS]
    with eng.encode_session(want_latents=True) as sess:
        sess.reserve_frames(8)                                               # small: the arenas grow, clips relocate
        first_arena = sess._ar[0].data_ptr()
        hs, fed, step, ended = {}, [0] * len(FS), [0] * len(FS), [False] * len(FS)
        moved, r = 0, 0
        while not all(ended):
            feeds, ends = {}, []
            for i, F in enumerate(FS):
                if r == start[i]:
                    hs[i] = sess.open(max_frames=F if i % 4 == 0 else None)
                if r < start[i] or ended[i]:
                    continue
                if step[i] < len(plans[i]):
                    n = plans[i][step[i]]
                    piece = items[i][:, fed[i]:fed[i] + n]
                    feeds[hs[i]] = piece.cuda() if i % 3 == 0 else piece.numpy() if i % 3 == 1 else piece
                    fed[i] += n
                    step[i] += 1
                    if fed[i] == F and same_call[i]:
                        ends.append(hs[i])
                else:
                    ends.append(hs[i])
            bases = {h: c.base for h, c in sess.clips.items()}
            res = sess.feed_list(feeds, ended=ends)
            moved += sum(1 for h, c in sess.clips.items() if h in bases and bases[h] != c.base)
            assert set(res) == set(feeds) | set(ends)
            for i in range(len(FS)):
                out = res.get(hs.get(i))
                if out is None:
                    continue
                done = hs[i] in ends
                assert out["done"] == done and out["final"] == PK.enc_ready(fed[i], done)
                n = out["quant"].shape[1]
                assert out["idx"].shape == (n,) and out["latents"].shape == (cfg["Cc"], n) and out["idx"].dtype == torch.int64
                if FS[i] < 17 and not done:
                    assert n == 0                                            # nothing is final before the end
                for key in got[i]:
                    got[i][key].append(out[key].clone())
                assert sum(p.shape[1] for p in got[i]["quant"]) == out["final"]
                ended[i] = done
            r += 1
        assert sess.live == [] and sess._top == 0
        if schedule != "all_in_one_call":
            assert sess._ar[0].data_ptr() != first_arena and moved > 0       # the arenas grew and a clip moved
    for i, want in enumerate(whole):
        for key in ("quant", "latents"):
            assert torch.equal(torch.cat(got[i][key], dim=1), want[key]), (schedule, FS[i], key)
        assert torch.equal(torch.cat(got[i]["idx"]), want["idx"]), (schedule, FS[i])


def test_one_clip_forms_and_refusals_on_the_device():
    eng, cfg, items, whole = _setup()
    x = items[FS.index(37)]
    with eng.encode_session() as sess:
        h = sess.open(max_frames=37)
        a = sess.feed(h, x[:, :30])
        assert a["latents"] is None and a["final"] == 4 and not a["done"] and a["quant"].shape == (cfg["Cc"], 4)
        with pytest.raises(ValueError, match=r"38 frames are beyond max_frames \(37\)"):
            sess.feed(h, x[:, :8])
        empty = sess.feed(h, x[:, :0])
        assert empty["quant"].shape == (cfg["Cc"], 0) and empty["final"] == 4
        b = sess.feed(h, x[:, 30:].cuda())
        c = sess.end(h)
        assert c["done"] and c["final"] == 10 and sess.live == []
        assert torch.equal(torch.cat([a["quant"], b["quant"], c["quant"]], dim=1), whole[FS.index(37)]["quant"])
        assert torch.equal(torch.cat([a["idx"], b["idx"], c["idx"]]), whole[FS.index(37)]["idx"])
        with pytest.raises(ValueError, match="not an open utterance"):
            sess.feed(h, x[:, :1])
        k = sess.open()
        sess.feed(k, x[:, :20])
        sess.drop(k)
        assert sess.live == [] and sess._top == 0


def test_vqvae_module_session_equals_encode_list():
    from test_gpu_modules import _build
    _, cfg, items, whole = _setup()
    cfg_full, sd, _, _, _ = golden_model("A")
    model, _ = _build(cfg_full)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    x = items[FS.index(21)]
    with model.encode_session() as sess:
        h = sess.open()
        parts = [sess.feed(h, x[:, :17].cuda())["quant"], sess.feed_list({h: x[:, 17:].cuda()}, ended=(h,))[h]["quant"]]
    assert parts[0].shape[1] == 1 and torch.equal(torch.cat(parts, dim=1), model.encode_list([x.cuda()])[0])


# ---- 4. cost per call ---------------------------------------------------------------------------------------------------------------------
def test_feed_list_costs_the_same_for_2_and_16_clips(monkeypatch):
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
    seen = []
    real_lib = eng.lib
    try:
        for n in (2, 16):
            with eng.encode_session() as sess:
                sess.reserve_frames(16 * 24)
                hs = [sess.open(max_frames=24) for _ in range(n)]
                sess.feed_list({h: torch.randn(cfg["c_in"], 20, generator=gen).cuda() for h in hs})
                feeds = {h: torch.randn(cfg["c_in"], 1, generator=gen).cuda() for h in hs}       # 20 -> 21 frames: a new latent each
                torch.cuda.synchronize()
                counts.clear()
                uploads.clear()
                eng.lib = Counting(real_lib)
                monkeypatch.setattr(torch.Tensor, "to", counting_to)
                res = sess.feed_list(feeds)
                monkeypatch.setattr(torch.Tensor, "to", real_to)
                eng.lib = real_lib
                assert all(r["quant"].shape[1] == 1 and r["final"] == 2 for r in res.values()) and len(res) == n
                seen.append((dict(counts), len(uploads)))
    finally:
        eng.lib = real_lib
    assert seen[0] == seen[1], seen
    launches, ups = seen[0]
    assert launches == {"wae_enc_conv_fwd_ranges": 11, "wae_vq_nearest": 1}      # one launch per layer, one quantiser call
    assert ups == 1                                                              # ONE table upload (the frames were on the device)


# ---- 5. end to end: features in, audio out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coop", [False, True], ids=["slots", "one_team"])
def test_fed_features_decode_as_the_whole_clip(coop, monkeypatch):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.decode import coop_sized
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, _, _, _ = golden_model("A")
    monkeypatch.setenv("WAE_AR_COOP", "1" if coop else "0")
    monkeypatch.setenv("WAE_AR_COOP_C", "8")
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    assert coop_sized(eng.g)
    hop = int(np.prod(cfg["upsample_scales"]))
    gen = torch.Generator().manual_seed(23)
    F = 21                                                                   # the shortest clip with a latent frame to decode from before its end
    Lq = (F + 3) // 4
    T = Lq * hop
    feats = torch.randn(cfg["c_in"], F, generator=gen) * 1.7
    uni = torch.rand(T, generator=gen).cuda()
    quant = eng.encode_list([feats])[0]["quant"].contiguous()
    want = eng.incremental_forward(quant[None], torch.tensor([3]).cuda(), T, mode="sample", init_idx=31, uniforms=uni[None])["idx"][0].clone()
    parts, sizes, rounds, got = [], [], 0, 0
    with eng.encode_session() as enc, eng.decode_session(mode="sample", coop=coop, **({"teams": 1} if coop else {"slots": 2})) as dec:
        e, h = enc.open(), dec.open(dict(gid=3, init_idx=31))
        for lo, hi, end in ((0, 9, False), (9, 21, False), (21, 21, True)):      # nothing final; two latent frames; the end: four more
            res = enc.end(e) if end else enc.feed(e, feats[:, lo:hi])
            n = res["quant"].shape[1]
            assert n == (0, 2, 4)[len(sizes)]
            sizes.append(n)
            if n:
                dec.feed_list({h: res["quant"]}, uniforms={h: uni[got * hop:(got + n) * hop]})
                got += n
            if res["done"]:
                dec.end(h)
            while True:
                out = dec.step(1500).get(h)
                if out is None:
                    break
                parts.append(out["idx"].clone())
                rounds += 1
                if out["done"]:
                    break
            if len(sizes) == 2:
                assert rounds == 1 and parts[0].shape[0] == hop - 205        # decoded while the utterance was still open
    assert got == Lq and rounds >= 2
    assert torch.equal(torch.cat(parts), want)


# ---- 6. synthesis.py ----------------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_feed_features(tmp_path):
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
    for dst, extra in (("rounds/", []), ("fed/", ["--feed-features", "5"])):
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
