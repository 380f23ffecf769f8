"""Decode sessions on the one-CU slots on the GPU (wae_ar_generate_spans, wae_ar_generate_scalar_spans, WaeEngine.decode_session /
decode_list_stream, synthesis.py --batch-decode --batch-stream): the clips of a ragged list decode in rounds -- one launch per round,
every clip in its own history ring, on whichever slot takes its span -- and every clip's chunks, concatenated, are BITWISE
decode_list's result for it and incremental_forward's for the clip alone on the one-CU kernel (WAE_AR_COOP=0).  The 20-layer geometry
has dilations up to 512 (the longest ring: 1025 rows); the rounds [1, 7, 1024, 1025, 503] hold a one-step span, a span shorter than
the largest dilation and boundaries on both sides of a ring wrap, and clips end in the middle of a round."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from test_gpu_ar_stream import HP, SMALL, _engine, _run, _tiny_dump_and_checkpoint

pytestmark = pytest.mark.gpu
LENS = [1500, 37, 2300, 640, 1, 1100, 911]
ROUNDS = [1, 7, 1024, 1025, 503]
assert sum(ROUNDS) >= max(LENS)
START = SMALL["O"] // 2 - 1                                # (the default start class, 127, needs more than 127 classes)


def _items(cfg=SMALL, lens=LENS, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return [dict(T=T, c=torch.randn(cfg["Cc"], T, generator=gen).cuda(), gid=int(torch.randint(0, cfg["n_speakers"], (1,), generator=gen)),
                 uniforms=torch.rand(T, generator=gen).cuda(), test_inputs=torch.randint(0, cfg["O"], (T,), generator=gen).cuda(),
                 init_idx=START) for T in lens]


def _for_mode(items, mode):
    """mode "logits" is teacher-forced on every step; the other modes run free from the start class"""
    return items if mode == "logits" else [{k: v for k, v in it.items() if k != "test_inputs"} for it in items]


def _session(eng, items, rounds=ROUNDS, joins=None, drops=None, **kw):
    """the items through a session -> per item the concatenated chunks (idx | x, logits) and the chunk lengths.  joins: {round: item
    indices added in front of that round} (default: all in front of round 0); drops: {round: item indices dropped behind it}."""
    joins = joins if joins is not None else {0: list(range(len(items)))}
    drops = drops or {}
    parts, handle = {i: [] for i in range(len(items))}, {}
    with eng.decode_session(**kw) as sess:
        for r, n in enumerate(rounds):
            for i in joins.get(r, []):
                handle[i] = sess.add(items[i])
            res = sess.step(n)
            for i, h in handle.items():
                if h in res:
                    parts[i].append(res[h])
                    assert res[h]["done"] == (h not in sess.live)
            for i in drops.get(r, []):
                sess.drop(handle.pop(i))
        left = sess.live
    torch.cuda.synchronize()
    out = []
    for i in range(len(items)):
        key = "x" if "x" in parts[i][0] else "idx"
        lg = None if parts[i][0]["logits"] is None else torch.cat([p["logits"] for p in parts[i]], -1)
        val = None if parts[i][0][key] is None else torch.cat([p[key] for p in parts[i]])
        out.append((val, lg, [int(next(v for k, v in p.items() if k != "done" and v is not None).shape[-1]) for p in parts[i]]))
    return out, left


def _expected_chunks(T, rounds=ROUNDS, first=0):
    out, t = [], 0
    for n in rounds[first:]:
        if t < T:
            out.append(min(n, T - t))
            t += out[-1]
    return out


def _equal(got, want, what):
    assert len(got) == len(want)
    for i, (g_, w_) in enumerate(zip(got, want)):
        for name, a, b in (("out", g_[0], w_[0]), ("logits", g_[1], w_[1])):
            assert (a is None) == (b is None), (what, i, name)
            if a is not None:
                assert a.shape == b.shape and a.dtype == b.dtype, (what, i, name, a.shape, b.shape)
                assert torch.equal(a, b), (what, i, name, "first difference at", (a != b).nonzero()[:1].tolist())


_REF = {}


def _reference(dtype, mode, monkeypatch):
    """(engine, items, decode_list's results) of (dtype, mode): computed once, shared, never changed"""
    if (dtype, mode) not in _REF:
        eng = _engine(SMALL, dtype, monkeypatch, coop="0")
        items = _for_mode(_items(), mode)
        res = eng.decode_list(items, mode=mode, want_logits=True)
        torch.cuda.synchronize()
        _REF[dtype, mode] = (eng, items, [(r["idx"].clone(), r["logits"].clone()) for r in res])
    return _REF[dtype, mode]


def _alone(eng, it, mode):
    kw = dict(init_idx=it["init_idx"])
    if mode == "sample":
        kw["uniforms"] = it["uniforms"][None]
    if it.get("test_inputs") is not None:
        kw["test_inputs"] = it["test_inputs"][None]
    eng._ar_profile = None
    out = eng.incremental_forward(it["c"][None], torch.tensor([it["gid"]]).cuda(), it["T"], mode=mode, c_is_upsampled=True,
                                  want_logits=True, **kw)
    assert eng._ar_profile is None                         # the one-CU kernel
    return out["idx"][0].clone(), out["logits"][0].clone()


# ---- 1. every clip is its list decode and its single decode -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sample", "argmax", "logits"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_clip_is_its_list_decode_and_its_single_decode(dtype, mode, monkeypatch):
    eng, items, want = _reference(dtype, mode, monkeypatch)
    got, left = _session(eng, items, mode=mode, want_logits=True)
    assert left == [] and [g[2] for g in got] == [_expected_chunks(T) for T in LENS]
    _equal(got, want, (dtype, mode, "decode_list"))
    _equal(got, [_alone(eng, it, mode) for it in items], (dtype, mode, "incremental_forward alone"))
    if mode == "sample":
        assert int(torch.unique(torch.cat([g[0] for g in got])).numel()) > SMALL["O"] // 4      # real roll-outs, not a constant


def test_logits_only_on_request_and_results_outlive_the_session(monkeypatch):
    eng, items, want = _reference("fp32", "sample", monkeypatch)
    got, _ = _session(eng, items[:3], rounds=[700, 700, 700, 700], mode="sample")
    assert all(g[1] is None for g in got)
    _equal([(g[0], None) for g in got], [(w[0], None) for w in want[:3]], "without logits")


# ---- 2. a ring belongs to its clip, not to a slot ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mode", [("fp32", "sample"), ("bf16", "argmax")])
def test_two_slots_decode_seven_clips_in_turn(dtype, mode, monkeypatch):
    """slots=2: a slot decodes spans of different clips in turn, and a clip's spans run on either slot"""
    eng, items, want = _reference(dtype, mode, monkeypatch)
    got, _ = _session(eng, items, mode=mode, want_logits=True, slots=2)
    _equal(got, want, (dtype, mode, "two slots"))
    sub = [1, 3, 4, 6]                                     # one slot decodes every span of four clips, round after round
    got, _ = _session(eng, [items[i] for i in sub], rounds=[300] * 4, mode=mode, want_logits=True, slots=1)
    _equal(got, [want[i] for i in sub], (dtype, mode, "one slot, rounds of 300"))


# ---- 3. clips join and leave between rounds ------------------------------------------------------------------------------------------
def test_clips_join_mid_session_and_one_is_dropped(monkeypatch):
    eng, items, want = _reference("fp32", "sample", monkeypatch)
    more = _for_mode(_items(lens=[40], seed=77), "sample")          # the clip that is dropped behind round 1
    rounds = ROUNDS + ROUNDS[2:]
    got, left = _session(eng, items + more, rounds=rounds, joins={0: [0, 1, 2, 3, 7], 3: [4, 5, 6]}, drops={1: [7]}, mode="sample",
                         want_logits=True, slots=3)
    assert left == []
    _equal(got[:7], want, "joined behind round 2 / beside a dropped clip")
    assert [g[2] for g in got[4:7]] == [_expected_chunks(T, rounds, 3) for T in LENS[4:]]
    assert got[7][2] == [1, 7] and torch.equal(got[7][0], _alone(eng, more[0], "sample")[0][:8])
    # a chunk per handle: clip 0 alone, then clip 1 alone, then both
    with eng.decode_session(mode="sample") as sess:
        a, b = sess.add(items[3]), sess.add(items[1])
        r1, r2 = sess.step({a: 100}), sess.step({b: 30})
        assert list(r1) == [a] and list(r2) == [b] and sess.step({}) == {}
        r3 = sess.step(10_000)
        assert sess.live == [] and r3[a]["done"] and r3[b]["done"]
        assert torch.equal(torch.cat([r1[a]["idx"], r3[a]["idx"]]), want[3][0])
        assert torch.equal(torch.cat([r2[b]["idx"], r3[b]["idx"]]), want[1][0])


def test_decode_list_stream_yields_rounds_in_the_callers_order(monkeypatch):
    eng, items, want = _reference("fp32", "sample", monkeypatch)
    rounds = list(eng.decode_list_stream(items, 1024, mode="sample", want_logits=True))
    torch.cuda.synchronize()
    assert len(rounds) == 3 and all(len(r) == len(items) for r in rounds)
    assert [r is None for r in rounds[1]] == [T <= 1024 for T in LENS] and [r is None for r in rounds[2]] == [T <= 2048 for T in LENS]
    got = [(torch.cat([r[i]["idx"] for r in rounds if r[i] is not None]), torch.cat([r[i]["logits"] for r in rounds if r[i] is not None], -1))
           for i in range(len(items))]
    _equal(got, want, "decode_list_stream")
    # no uniforms given: a seeded stream equals the seeded list
    bare = [{k: v for k, v in it.items() if k != "uniforms"} for it in items[:4]]
    torch.manual_seed(21)
    one = [r["idx"].clone() for r in eng.decode_list(bare, mode="sample")]
    torch.manual_seed(21)
    rounds = list(eng.decode_list_stream(bare, 700, mode="sample"))
    for i in range(4):
        assert torch.equal(torch.cat([r[i]["idx"] for r in rounds if r[i] is not None]), one[i]), i


# ---- 4. start classes and forced prefixes per item -----------------------------------------------------------------------------------
def test_start_class_and_forced_prefix_per_item(monkeypatch):
    """forced prefixes that end inside a span (100: inside round 2), one step behind a boundary (1033: the forced first step of round 3 is
    the teacher's), on a boundary (8) and with the clip (640)"""
    eng = _engine(SMALL, "bf16", monkeypatch, coop="0")
    items = _for_mode(_items(), "sample")
    for it, s in zip(items, [3, 40, 62, 0, 63, 17, 31]):
        it["init_idx"] = s
    gen = torch.Generator().manual_seed(8)
    for i, F in ((0, 100), (2, 1033), (3, 640), (5, 8), (6, 1)):
        items[i]["test_inputs"] = torch.randint(0, SMALL["O"], (F,), generator=gen).cuda()
    want = [(r["idx"].clone(), r["logits"].clone()) for r in eng.decode_list(items, mode="sample", want_logits=True)]
    got, _ = _session(eng, items, mode="sample", want_logits=True, slots=3)
    _equal(got, want, "start classes and forced prefixes")
    _equal(got[:2], [_alone(eng, it, "sample") for it in items[:2]], "alone")
    with eng.decode_session(mode="argmax") as sess:
        with pytest.raises(IndexError):
            sess.add(dict(items[1], init_idx=SMALL["O"]))
        with pytest.raises(ValueError, match="gid"):
            sess.add(items[1])
            sess.add(dict(items[4], gid=None))
    with eng.decode_session(mode="logits") as sess:
        with pytest.raises(ValueError, match="teacher-forced"):
            sess.add(items[0])


# ---- 5. scalar-input decoders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,O_ch,dtype", [("Logistic", 30, "fp32"), ("Normal", 6, "bf16"), ("Normal", 2, "fp32")])
def test_scalar_input_clips_against_decode_list_scalar(dist, O_ch, dtype, monkeypatch):
    cfg = dict(SMALL, O=O_ch, scalar_input=True, output_distribution=dist)
    eng = _engine(cfg, dtype, monkeypatch, coop="0")
    gen = torch.Generator().manual_seed(11)
    M = 1 if O_ch == 2 else O_ch // 3
    unit = lambda *s: (torch.rand(*s, generator=gen) * (1 - 2e-5) + 1e-5).cuda()  # noqa: E731
    lens = [1100, 37, 1300, 1, 1026]
    items = []
    for T in lens:
        it = dict(T=T, c=torch.randn(cfg["Cc"], T, generator=gen).cuda(), gid=int(torch.randint(0, cfg["n_speakers"], (1,), generator=gen)))
        if dist == "Logistic" or M > 1:
            it["u_mix"] = unit(T, M)
        it.update(u_log=unit(T)) if dist == "Logistic" else it.update(z=torch.randn(T, generator=gen).cuda())
        items.append(it)
    items[0]["test_inputs"] = (torch.rand(600, generator=gen) * 2 - 1).cuda()      # a forced prefix that ends inside the fourth span
    want = [(r["x"].clone(), r["logits"].clone()) for r in eng.decode_list_scalar(items, mode="sample", want_logits=True, c_is_upsampled=True)]
    got, _ = _session(eng, items, rounds=[1, 7, 512, 513, 400], mode="sample", want_logits=True, c_is_upsampled=True, slots=2)
    _equal(got, want, (dist, O_ch, "sample"))
    assert float(torch.cat([g[0] for g in got]).std()) > 1e-3
    # teacher-forced parameters
    forced = [dict(T=it["T"], c=it["c"], gid=it["gid"], test_inputs=(torch.rand(it["T"], generator=gen) * 2 - 1).cuda()) for it in items[:3]]
    want = [(None, r["logits"].clone()) for r in eng.decode_list_scalar(forced, mode="logits", c_is_upsampled=True)]
    got, _ = _session(eng, forced, rounds=[1, 7, 512, 513, 400], mode="logits", c_is_upsampled=True)
    _equal(got, want, (dist, O_ch, "logits"))
    with pytest.raises(NotImplementedError):
        eng.decode_session(coop=True)


# ---- 6. against the reference's own vectors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("name", ["A", "B"])
def test_teacher_forced_logits_against_the_reference(name, dtype, tol):
    """tests/test_gpu_ar.py::test_teacher_forced_equals_reference through a session in rounds of 7 steps"""
    cfg, sd, ins, zm, ocfg = golden_model(name)
    z = load_npz("ar_" + name)
    eng = _engine(cfg, dtype, sd=sd)
    c_up = torch.from_numpy(z["c_up"]).cuda()
    B, _, Tar = c_up.shape
    x, g = ins["x"][:, :Tar].cuda(), ins["g"]
    items = [dict(T=Tar, c=c_up[b].contiguous(), gid=int(g[b]), test_inputs=x[b]) for b in range(B)]
    got, _ = _session(eng, items, rounds=[7] * ((Tar + 6) // 7), mode="logits", c_is_upsampled=True)
    err = rel_err(torch.stack([g_[1] for g_ in got]).cpu(), z["tf_logits"])
    print(f"session, model {name} {dtype}: teacher-forced logits rel err {err:.3e} (bound {tol})")
    assert err < tol


# ---- 7. synthesis.py -----------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_batch_stream(tmp_path, monkeypatch):
    dump, ckpt, preset = _tiny_dump_and_checkpoint(tmp_path)
    rng = np.random.default_rng(6)
    pairs = [("S0_0007", "V1")]
    for fid, frames, tar in (("0011", 28, "V2"), ("0012", 12, "V1"), ("0013", 20, "V3")):
        utt = dump / "test" / f"S0_{fid}"
        utt.mkdir(parents=True)
        np.save(utt / "mfcc.norm.npy", rng.standard_normal((frames, 39)).astype(np.float32))
        pairs.append((f"S0_{fid}", tar))
    (tmp_path / "syn.txt").write_text("".join(f"test/{s} {t}\n" for s, t in pairs))
    (tmp_path / "spk.json").write_text(json.dumps({"V1": 2, "V2": 0, "V3": 4}))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for dst, extra in (("list/", ["--batch-decode"]), ("rounds/", ["--batch-decode", "--batch-stream", "700"])):
        outs[dst] = _run([os.path.join(root, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
                          "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp_path))
    assert "first audio of all 4 clips after" in outs["rounds/"] and "first audio" not in outs["list/"]
    names = sorted(p.name for p in (tmp_path / "list" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    sizes = set()
    for n in names:
        a = (tmp_path / "list" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "rounds" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
        sizes.add(len(a))
    assert len(sizes) == len(names)                                    # four clips of four lengths, the longest in seven rounds
