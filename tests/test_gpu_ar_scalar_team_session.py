"""GPU: decode sessions of scalar-input decoders on cooperative teams (wae_ar_generate_coop_scalar_spans,
WaeEngine.decode_session(coop=True) under ar_path(scalar_coop=True), synthesis.py --batch-decode --batch-coop --batch-stream on a "raw"
model), modelled on tests/test_gpu_ar_team_session.py: the clips of a ragged list decode in rounds on teams of C workgroups, every clip
in its own history ring, and every clip's chunks, concatenated, are BITWISE scalar incremental_forward's result for the clip alone on
the cooperative path at the same ar_path -- on the any-shape kernel (golden model S's sizes on 8 members; private rings, nothing
cleared) and, with scalar_fast=True, on the constant-size scalar kernels (one shared ring per clip: cleared by the clip's first span,
kept by every later one).  Every launch checks that no wait between team-mates timed out."""
import os

import pytest
import torch

from helpers import golden_model
from oracle import wae_oracle as O
from test_gpu_ar_scalar_fast import _cfg, _engine as _ref_engine
from test_gpu_ar_scalar_list import HP, _alone, _equal, _items, _run, raw_checkpoint  # noqa: F401  (raw_checkpoint: a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [48, 17, 33, 5, 1]
ROUNDS = [7, 1, 24, 64]


def _expected_chunks(T, rounds=ROUNDS, first=0):
    out, left = [], T
    for n in rounds[first:]:
        if left <= 0:
            break
        out.append(min(n, left))
        left -= out[-1]
    return out


def _small_engine(dtype, monkeypatch, dist="Logistic", O_ch=30, C=8):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, _, z, _ = golden_model("S")
    cfg = dict(cfg, output_distribution=dist)
    if O_ch != cfg["O"]:
        cfg["O"] = O_ch
        sd = O.make_state_dict(cfg, int(z["salt"]))
    monkeypatch.setenv("WAE_AR_COOP", "1")
    monkeypatch.setenv("WAE_AR_COOP_C", str(C))
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype).ar_path(scalar_coop=True)
    assert eng.opt.ar_coop and eng.opt.ar_coop_c == C
    eng.load_state_dict(sd)
    return eng, cfg


def _session(eng, items, rounds=ROUNDS, joins=None, drops=None, **kw):
    """tests/test_gpu_ar_team_session.py's driver for scalar clips: after every launch the team path left its error / profile words, and
    no wait timed out.  A round is a number of steps for every live clip, or a mapping from item index to steps."""
    joins = joins if joins is not None else {0: list(range(len(items)))}
    drops = drops or {}
    parts, handle = {i: [] for i in range(len(items))}, {}
    with eng.decode_session(coop=True, c_is_upsampled=True, **kw) as sess:
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
    cat = lambda ps, k, dim: None if ps[0][k] is None else torch.cat([p[k] for p in ps], dim)  # noqa: E731
    out = [(cat(parts[i], "x", 0), cat(parts[i], "logits", -1)) for i in range(len(items))]
    sizes = [[int((p["x"] if p["x"] is not None else p["logits"]).shape[-1]) for p in parts[i]] for i in range(len(items))]
    return out, sizes, left


# ---- 1. the any-shape kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("teams", [1, 3, 8])
@pytest.mark.parametrize("mode", ["sample", "logits"])
@pytest.mark.parametrize("dist,O_ch", [("Logistic", 30), ("Normal", 2)])
def test_any_shape_kernel_every_clip_is_its_single_cooperative_decode(dist, O_ch, mode, teams, monkeypatch):
    eng, cfg = _small_engine("fp32" if teams != 3 else "bf16", monkeypatch, dist, O_ch)
    items = _items(cfg, LENS)
    if mode == "logits":
        for i, it in enumerate(items):
            it["test_inputs"] = (O.hash_fill((it["T"],), 40 + i) * 0.9).cuda()
            for k in ("u_mix", "u_log", "z"):
                it.pop(k, None)
    got, sizes, left = _session(eng, items, mode=mode, want_logits=True, teams=teams)
    assert left == [] and sizes == [_expected_chunks(T) for T in LENS]
    _equal(got, [_alone(eng, it, mode, coop=True) for it in items], (dist, mode, teams))
    if mode == "sample":
        assert float(torch.cat([x for x, _ in got]).std()) > 0.0      # real roll-outs, not a constant


# ---- 2. the constant-size kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,split", [("bf16", {}), ("bf16", dict(lds_layers=0, reg_layers=0)), ("fp32", {})],
                         ids=["bf16_resident", "bf16_streaming", "fp32"])
def test_constant_size_kernels_every_clip_is_its_single_cooperative_decode(dtype, split, monkeypatch):
    """teams=2 with seven clips: inside one launch a team decodes a fresh clip, then a continuation of another clip, then a fresh clip
    again -- clearing for t0 == 0, no clearing for t0 > 0, and the zb rewrite for every span (every clip has its own speaker)"""
    cfg = _cfg(5)
    eng = _ref_engine(cfg, dtype, monkeypatch, **split)
    lens = LENS + [40, 26]
    items = _items(cfg, lens)
    for it, g in zip(items, [3, 5, 0, 6, 1, 2, 4]):
        it["gid"] = g
    rounds = ROUNDS + [64]
    # clips 0, 2 and 5 start in round 0; the others join in front of round 2, where the first three continue
    got, sizes, left = _session(eng, items, rounds=rounds, joins={0: [0, 2, 5], 2: [1, 3, 4, 6]}, mode="sample", want_logits=True, teams=2)
    assert left == []
    assert sizes == [_expected_chunks(T, rounds, 0 if i in (0, 2, 5) else 2) for i, T in enumerate(lens)]
    want = [_alone(eng, it, coop=True) for it in items]
    _equal(got, want, (dtype, split))
    assert float(torch.cat([x for x, _ in got]).std()) > 0.0
    # ONE team, the second launch longest first: clip 1 fresh (20 of its 40), clip 0 continued at step 12 (16), clip 2 fresh (17):
    # clear, keep, clear on the same team inside one launch
    sub = [items[0], items[5], items[1]]
    got, sizes, left = _session(eng, sub, rounds=[{0: 12}, {1: 20, 0: 16, 2: 17}, 64], mode="sample", want_logits=True, teams=1)
    assert left == [] and sizes == [[12, 16, 20], [20, 20], [17]]
    _equal(got, [want[0], want[5], want[1]], (dtype, split, "fresh, continued, fresh on one team"))


# ---- 3. clips join and leave ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["any_shape", "constant_size"])
def test_a_clip_joins_mid_session_and_a_clip_is_dropped(form, monkeypatch):
    if form == "any_shape":
        eng, cfg = _small_engine("fp32", monkeypatch)
    else:
        cfg = _cfg(5)
        eng = _ref_engine(cfg, "bf16", monkeypatch)
    items = _items(cfg, [48, 40, 33, 17])
    rounds = [7, 24, 64]
    # clip 1 is dropped behind round 0 (its ring is free for clip 2, which joins in front of round 1, and for clip 3 in front of round 2)
    got, sizes, left = _session(eng, items, rounds=rounds, joins={0: [0, 1], 1: [2], 2: [3]}, drops={0: [1]}, mode="sample",
                                want_logits=True, teams=2)
    assert left == [] and sizes[1] == [7]
    want = [_alone(eng, it, coop=True) for it in items]
    _equal([got[0], got[2], got[3]], [want[0], want[2], want[3]], "beside a dropped clip")
    assert torch.equal(got[1][0], want[1][0][:7]) and torch.equal(got[1][1], want[1][1][:, :7])


def test_team_session_of_a_scalar_decoder_needs_the_opt_in(monkeypatch):
    eng, _ = _small_engine("fp32", monkeypatch)
    eng.ar_path(scalar_coop=False)
    with pytest.raises(NotImplementedError, match="one-CU slots"):
        eng.decode_session(coop=True)


# ---- 4. synthesis.py ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["--coop-scalar", "--coop-scalar-fast"])
def test_synthesis_script_writes_the_same_wavs_with_batch_coop_and_batch_stream(flag, raw_checkpoint, monkeypatch):  # noqa: F811
    tmp, dump, ckpt, preset, pairs = raw_checkpoint
    monkeypatch.delenv("WAE_AR_COOP", raising=False)
    monkeypatch.delenv("WAE_AR_COOP_C", raising=False)
    coop = ["--batch-decode", "--batch-coop", "--batch-teams", "2", flag]
    tag = flag.strip("-").replace("-", "_")
    outs = {}
    for dst, extra in ((f"{tag}_teams/", coop), (f"{tag}_rounds/", coop + ["--batch-stream", "700"])):
        outs[dst] = _run([os.path.join(ROOT, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp / "syn.txt"), str(tmp / "spk.json"),
                          "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp))
    assert f"first audio of all {len(pairs)} clips after" in outs[f"{tag}_rounds/"]
    names = sorted(p.name for p in (tmp / f"{tag}_teams" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    for n in names:
        a = (tmp / f"{tag}_teams" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp / f"{tag}_rounds" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
