"""Decode sessions on cooperative teams on the GPU (wae_ar_generate_coop_spans, WaeEngine.decode_session(coop=True), synthesis.py
--batch-decode --batch-coop --batch-stream): the clips of a ragged list decode in rounds on teams of C workgroups, every clip in its
own history ring, and every clip's chunks, concatenated, are BITWISE incremental_forward's result for the clip alone on the
cooperative path (WAE_AR_COOP=1, the same ar_path) -- on the any-shape kernel (members keep private rings; nothing is cleared) and on
the constant-size kernels in every residency split (one shared ring per clip: cleared by the clip's first span, kept by every later
one; only the resident layers' zb words change at a span boundary).  Every launch checks that no wait between team-mates timed out."""
import json
import os

import numpy as np
import pytest
import torch

from test_gpu_ar_session import LENS, ROUNDS, _equal, _expected_chunks
from test_gpu_ar_stream import HP, REF, SMALL, _engine, _run, _tiny_dump_and_checkpoint
from test_gpu_ar_team_list import _alone, _items

pytestmark = pytest.mark.gpu


def _session(eng, items, rounds=ROUNDS, joins=None, drops=None, **kw):
    """tests/test_gpu_ar_session.py's driver on teams: after every launch the team path left its error / profile words, and no wait
    timed out.  A round is a number of steps for every live clip, or a mapping from item index to steps."""
    joins = joins if joins is not None else {0: list(range(len(items)))}
    drops = drops or {}
    parts, handle = {i: [] for i in range(len(items))}, {}
    with eng.decode_session(coop=True, **kw) as sess:
        for r, n in enumerate(rounds):
            for i in joins.get(r, []):
                handle[i] = sess.add(items[i])
            eng._ar_profile = None
            res = sess.step(n if isinstance(n, int) else {handle[i]: v for i, v in n.items()})
            if res:
                assert eng._ar_profile is not None and int(eng._ar_profile[0]) == 0, (r, eng._ar_profile)
            for i, h in handle.items():
                if h in res:
                    parts[i].append(res[h])
            for i in drops.get(r, []):
                sess.drop(handle.pop(i))
        left = sess.live
    torch.cuda.synchronize()
    out = [(torch.cat([p["idx"] for p in parts[i]]), None if parts[i][0]["logits"] is None else torch.cat([p["logits"] for p in parts[i]], -1),
            [int(p["idx"].shape[0]) for p in parts[i]]) for i in range(len(items))]
    return out, left


# ---- 1. the any-shape kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("teams", [1, 3, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_any_shape_kernel_every_clip_is_its_single_cooperative_decode(dtype, teams, monkeypatch):
    eng = _engine(SMALL, dtype, monkeypatch)
    items = _items(SMALL)
    mode = "sample" if teams != 3 else "argmax"
    got, left = _session(eng, items, mode=mode, want_logits=True, teams=teams)
    assert left == [] and [g[2] for g in got] == [_expected_chunks(T) for T in LENS]
    _equal(got, [_alone(eng, it, mode) for it in items], (dtype, teams, mode))
    if mode == "sample":
        assert int(torch.unique(torch.cat([g[0] for g in got])).numel()) > SMALL["O"] // 4      # real roll-outs, not a constant


def test_any_shape_kernel_teacher_forced_and_forced_prefixes(monkeypatch):
    eng = _engine(SMALL, "bf16", monkeypatch, members=8)
    items = _items(SMALL, lens=[1500, 37, 1100, 1])
    gen = torch.Generator().manual_seed(8)
    for it in items:
        it["test_inputs"] = torch.randint(0, SMALL["O"], (it["T"],), generator=gen).cuda()
    got, _ = _session(eng, items, mode="logits", teams=2)
    _equal(got, [_alone(eng, it, "logits") for it in items], "logits")
    for it, F in zip(items, (100, 8, 1033, 1)):              # inside a span, on a boundary, one step behind a boundary
        it["test_inputs"] = it["test_inputs"][:F]
    got, _ = _session(eng, items, mode="sample", want_logits=True, teams=2)
    _equal(got, [_alone(eng, it, "sample") for it in items], "forced prefixes")


# ---- 2. the constant-size kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,split", [("bf16", {}), ("bf16", dict(reg_layers=11)), ("bf16", dict(lds_layers=0, reg_layers=0)), ("fp32", {})],
                         ids=["bf16_resident", "bf16_resident_without_vgpr_bank", "bf16_streaming", "fp32"])
def test_constant_size_kernels_every_clip_is_its_single_cooperative_decode(dtype, split, monkeypatch):
    """teams=2 with seven clips: inside one launch a team decodes a fresh clip, then a continuation of another clip, then a fresh clip
    again -- clearing for t0 == 0, no clearing for t0 > 0, and the zb rewrite for every span (every clip has its own speaker)"""
    eng = _engine(REF, dtype, monkeypatch, **split)
    items = _items(REF)
    for it, g in zip(items, [3, 150, 77, 0, 21, 9, 64]):
        it["gid"] = g
    # clips 0, 2 and 5 start in round 0; the others join in front of round 2, where the first three continue
    got, left = _session(eng, items, rounds=ROUNDS + [1024], joins={0: [0, 2, 5], 2: [1, 3, 4, 6]}, mode="sample", want_logits=True,
                         c_is_upsampled=True, teams=2)
    assert left == []
    assert [g[2] for g in got] == [_expected_chunks(T, ROUNDS + [1024], 0 if i in (0, 2, 5) else 2) for i, T in enumerate(LENS)]
    want = [_alone(eng, it, "sample") for it in items]
    _equal(got, want, (dtype, split))
    assert int(torch.unique(torch.cat([g[0] for g in got])).numel()) > REF["O"] // 4
    # ONE team, the second launch longest first: clip 1 fresh (900 of its 2300), clip 0 continued at step 600 (800), clip 3 fresh
    # (640): clear, keep, clear on the same team inside one launch
    sub = [items[0], items[2], items[3]]
    got, left = _session(eng, sub, rounds=[{0: 600}, {1: 900, 0: 800, 2: 700}, 4096], mode="sample", want_logits=True, c_is_upsampled=True,
                         teams=1)
    assert left == [] and [g[2] for g in got] == [[600, 800, 100], [900, 1400], [640]]
    _equal(got, [want[0], want[2], want[3]], (dtype, split, "fresh, continued, fresh on one team"))


# ---- 3. clips join and leave ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,dtype", [(SMALL, "fp32"), (REF, "bf16")], ids=["any_shape", "constant_size"])
def test_a_clip_joins_mid_session_and_a_clip_is_dropped(cfg, dtype, monkeypatch):
    eng = _engine(cfg, dtype, monkeypatch)
    items = _items(cfg, lens=[1500, 40, 1100, 37])
    rounds = [7, 1024, 1025]
    # clip 1 is dropped behind round 0 (its ring is free for clip 2, which joins in front of round 1, and for clip 3 in front of round 2)
    got, left = _session(eng, items, rounds=rounds, joins={0: [0, 1], 1: [2], 2: [3]}, drops={0: [1]}, mode="sample", want_logits=True,
                         c_is_upsampled=True, teams=2)
    assert left == [] and got[1][2] == [7]
    want = [_alone(eng, it, "sample") for it in items]
    _equal([got[0], got[2], got[3]], [want[0], want[2], want[3]], "beside a dropped clip")
    assert torch.equal(got[1][0], want[1][0][:7]) and torch.equal(got[1][1], want[1][1][:, :7])


def test_routing_of_the_team_session(monkeypatch):
    wide = dict(SMALL, O=300)
    eng = _engine(wide, "fp32", monkeypatch)
    with pytest.raises(ValueError, match="R, S and O <= 256"):
        eng.decode_session(coop=True)
    eng = _engine(SMALL, "fp32", monkeypatch)
    for mode in ("probs", "raw"):
        with pytest.raises(ValueError, match=f"mode '{mode}'"):
            eng.decode_session(mode=mode, coop=True)
    scalar = _engine(dict(SMALL, O=30, scalar_input=True, output_distribution="Logistic"), "fp32", monkeypatch)
    with pytest.raises(NotImplementedError, match="one-CU slots"):
        scalar.decode_session(coop=True)


# ---- 4. synthesis.py -----------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_batch_coop_and_batch_stream(tmp_path, monkeypatch):
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
    monkeypatch.delenv("WAE_AR_COOP", raising=False)
    monkeypatch.delenv("WAE_AR_COOP_C", raising=False)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    coop = ["--batch-decode", "--batch-coop", "--batch-teams", "2"]
    for dst, extra in (("teams/", coop), ("rounds/", coop + ["--batch-stream", "700"])):
        _run([os.path.join(root, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
              "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp_path))
    names = sorted(p.name for p in (tmp_path / "teams" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    for n in names:
        a = (tmp_path / "teams" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "rounds" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
