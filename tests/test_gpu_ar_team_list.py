"""A work list on cooperative teams on the GPU (wae_ar_generate_coop_list, WaeEngine.decode_list(coop=True), synthesis.py
--batch-coop): every item of a ragged list is BITWISE what incremental_forward returns for that utterance alone on the cooperative
path (WAE_AR_COOP=1, the same ar_path) -- on the any-shape kernel and on the constant-size kernels in every residency split, in
every mode and storage type, with and without conditioning, with per-item speakers, start classes and forced prefixes, whatever the
number of teams and the order of the list -- and the teacher-forced logits of the reference's own vectors keep the tolerances of
tests/test_gpu_ar.py.  The lengths lie below, around and beyond the longest history ring of the 20-layer geometry (2 * 512 + 1 rows),
and a team decodes several items in one launch: a 2300-step item is followed by items of 37, 2 and 1 steps on the same team."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from test_gpu_ar_stream import HP, REF, SMALL, _engine, _run, _tiny_dump_and_checkpoint

pytestmark = pytest.mark.gpu
LENS = [1500, 37, 2300, 640, 1, 1100, 911]
BARE = dict(SMALL, Cc=-1, Cg=-1, n_speakers=None)          # no local and no global conditioning


def _items(cfg, lens=LENS, seed=5):
    gen = torch.Generator().manual_seed(seed)
    cond = cfg["Cc"] > 0
    start = min(127, cfg["O"] // 2 - 1)                    # (the default start class, 127, needs more than 127 classes)
    return [dict(T=T, c=torch.randn(cfg["Cc"], T, generator=gen).cuda() if cond else None,
                 gid=int(torch.randint(0, cfg["n_speakers"], (1,), generator=gen)) if cond else None,
                 uniforms=torch.rand(T, generator=gen).cuda(), init_idx=start) for T in lens]


def _alone(eng, it, mode, want_logits=True):
    """the item as a batch of one through incremental_forward on the cooperative path (the engine was built with WAE_AR_COOP=1)"""
    kw = dict(init_idx=it["init_idx"])
    if mode == "sample":
        kw["uniforms"] = it["uniforms"][None]
    if it.get("test_inputs") is not None:
        kw["test_inputs"] = it["test_inputs"][None]
    eng._ar_profile = None
    out = eng.incremental_forward(it["c"][None] if it["c"] is not None else None,
                                  torch.tensor([it["gid"]]).cuda() if it["gid"] is not None else None, it["T"], mode=mode,
                                  c_is_upsampled=True, want_logits=want_logits, **kw)
    assert eng._ar_profile is not None                     # the cooperative path left its error / profile words: that path was taken
    return out["idx"][0].clone(), None if out["logits"] is None else out["logits"][0].clone()


def _equal(got, want, what):
    assert len(got) == len(want)
    for i, (g_, (idx, logits)) in enumerate(zip(got, want)):
        assert g_["idx"].shape == idx.shape and g_["idx"].dtype == torch.int32, (what, i)
        assert torch.equal(g_["idx"], idx), (what, i, "first difference at", (g_["idx"] != idx).nonzero()[:1].tolist())
        assert (g_["logits"] is None) == (logits is None), (what, i)
        if logits is not None:
            assert g_["logits"].shape == logits.shape, (what, i)
            assert torch.equal(g_["logits"], logits), (what, i, "first difference at", (g_["logits"] != logits).nonzero()[:1].tolist())


def _snapshot(res):
    return [(r["idx"].clone(), None if r["logits"] is None else r["logits"].clone()) for r in res]


def _as_dicts(snap):
    return [dict(idx=a, logits=b) for a, b in snap]


def _list(eng, items, mode, teams, **kw):
    eng._ar_profile = None
    got = eng.decode_list(items, mode=mode, coop=True, teams=teams, **kw)
    torch.cuda.synchronize()
    assert eng._ar_profile is not None and int(eng._ar_profile[0]) == 0      # the team launch ran and no wait timed out
    return got


# ---- 1. the any-shape kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["argmax", "sample"])
@pytest.mark.parametrize("cond", [True, False], ids=["c_and_gid", "unconditioned"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_any_shape_kernel_every_item_is_its_single_cooperative_decode(dtype, cond, mode, monkeypatch):
    cfg = SMALL if cond else BARE
    eng = _engine(cfg, dtype, monkeypatch)
    items = _items(cfg)
    got = _list(eng, items, mode, 3, want_logits=True)
    assert [r["idx"].shape[0] for r in got] == LENS and all(r["logits"].shape == (cfg["O"], T) for r, T in zip(got, LENS))
    got = _snapshot(got)
    _equal(_as_dicts(got), [_alone(eng, it, mode) for it in items], (dtype, cond, mode))
    if mode == "sample":
        assert int(torch.unique(torch.cat([a for a, _ in got])).numel()) > cfg["O"] // 4   # real roll-outs, not a constant
    assert all(r["logits"] is None for r in _list(eng, items[:3], mode, 3))                # logits only on request


# ---- 2. the constant-size kernels: per-item speakers against resident zb words -------------------------------------------------------
@pytest.mark.parametrize("dtype,split", [("bf16", {}), ("bf16", dict(reg_layers=11)), ("bf16", dict(lds_layers=0, reg_layers=0)), ("fp32", {})],
                         ids=["bf16_resident", "bf16_resident_without_vgpr_bank", "bf16_streaming", "fp32"])
def test_constant_size_kernels_every_item_is_its_single_cooperative_decode(dtype, split, monkeypatch):
    eng = _engine(REF, dtype, monkeypatch, **split)
    items = _items(REF, lens=[1500, 37, 2300, 1, 1100])
    for it, g in zip(items, [3, 150, 77, 0, 21]):          # every item its own speaker: its own zb row
        it["gid"] = g
    got = _snapshot(_list(eng, items, "sample", 2, want_logits=True, c_is_upsampled=True))
    _equal(_as_dicts(got), [_alone(eng, it, "sample") for it in items], (dtype, split))
    assert int(torch.unique(torch.cat([a for a, _ in got])).numel()) > REF["O"] // 4
    # the speaker matters: the same item under another speaker decodes differently
    other = _list(eng, [dict(items[0], gid=150)], "sample", 1, want_logits=True, c_is_upsampled=True)
    assert not torch.equal(other[0]["logits"], got[0][1])


# ---- 3. a reused team decodes as a fresh one -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,mode", [("fp32", "argmax"), ("bf16", "sample")])
def test_a_reused_team_decodes_as_a_fresh_one(dtype, mode, monkeypatch):
    """more items than teams: a team decodes one item after another in the same rings, with the same exchange buffers running on"""
    eng = _engine(SMALL, dtype, monkeypatch)
    items = _items(SMALL, lens=LENS + [1300, 2, 1026, 700])
    want = _snapshot(_list(eng, items, mode, 8, want_logits=True))
    _equal(_as_dicts(want[:4]), [_alone(eng, it, mode) for it in items[:4]], "eight teams")
    for teams in (1, 2, 3):
        _equal(_list(eng, items, mode, teams, want_logits=True), want, ("teams", teams))
    _equal(_list(eng, items, mode, 4096, want_logits=True), want, "teams beyond eight are clamped to eight")
    # one team, longest first: the 2300-step item directly followed by items of 37, 2 and 1 steps (stale history rows, wrong cursors)
    short = [items[2], items[1], items[8], items[4]]
    assert [it["T"] for it in short] == [2300, 37, 2, 1]
    _equal(_list(eng, short, mode, 1, want_logits=True), [want[2], want[1], want[8], want[4]], "one team, long then short")
    perm = [4, 2, 6, 0, 5, 1, 3, 10, 9, 7, 8]
    _equal(_list(eng, [items[j] for j in perm], mode, 3, want_logits=True), [want[j] for j in perm], "permuted")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_a_reused_team_of_the_constant_size_kernels(dtype, monkeypatch):
    """the shared ring of the constant-size kernels is cleared between items: long then short on ONE team equals eight teams"""
    eng = _engine(REF, dtype, monkeypatch)
    items = _items(REF, lens=[2300, 37, 2, 1, 1030])
    for it, g in zip(items, [5, 6, 7, 8, 9]):
        it["gid"] = g
    want = _snapshot(_list(eng, items, "sample", 8, want_logits=True, c_is_upsampled=True))
    _equal(_list(eng, items, "sample", 1, want_logits=True, c_is_upsampled=True), want, "one team")
    _equal(_as_dicts(want[1:4]), [_alone(eng, it, "sample") for it in items[1:4]], "alone")


# ---- 4. per-item start classes and forced prefixes -----------------------------------------------------------------------------------
def test_start_class_and_forced_prefix_per_item(monkeypatch):
    eng = _engine(SMALL, "bf16", monkeypatch)
    items = _items(SMALL)
    for it, s in zip(items, [3, 40, 62, 0, 63, 17, 31]):
        it["init_idx"] = s
    gen = torch.Generator().manual_seed(8)
    for i, F in ((0, 100), (2, 2300), (3, 640), (5, 1)):    # inside the item, and as long as the item
        items[i]["test_inputs"] = torch.randint(0, SMALL["O"], (F,), generator=gen).cuda()
    got = _snapshot(_list(eng, items, "sample", 2, want_logits=True))
    _equal(_as_dicts(got), [_alone(eng, it, "sample") for it in items], "start classes and forced prefixes")
    free = _list(eng, [{k: v for k, v in it.items() if k != "test_inputs"} for it in items], "sample", 2)
    assert not torch.equal(free[0]["idx"], got[0][0]) and torch.equal(free[1]["idx"], got[1][0])
    with pytest.raises(IndexError):
        eng.decode_list([dict(items[1], init_idx=SMALL["O"])], mode="argmax", coop=True)


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("name", ["A", "B"])
def test_teacher_forced_logits_against_the_reference(name, dtype, tol):
    """tests/test_gpu_ar.py::test_teacher_forced_equals_reference, its utterances as items among others of other lengths"""
    cfg, sd, ins, zm, ocfg = golden_model(name)
    z = load_npz("ar_" + name)
    eng = _engine(cfg, dtype, sd=sd)
    c_up = torch.from_numpy(z["c_up"]).cuda()
    B, _, Tar = c_up.shape
    x, g = ins["x"][:, :Tar].cuda(), ins["g"]
    item = lambda b, T: dict(T=T, c=c_up[b, :, :T].contiguous(), gid=int(g[b]), test_inputs=x[b, :T])  # noqa: E731
    items = [item(0, 5)] + [item(b, Tar) for b in range(B)] + [item(B - 1, Tar - 3), item(0, 1), item(B - 1, Tar // 2)]
    got = _list(eng, items, "logits", 2, c_is_upsampled=True)
    logits = torch.stack([got[1 + b]["logits"] for b in range(B)]).cpu()
    err = rel_err(logits, z["tf_logits"])
    print(f"team list, model {name} {dtype}: teacher-forced logits rel err {err:.3e} (bound {tol})")
    assert err < tol
    # the shorter items are prefixes of the same causal computation
    assert torch.equal(got[0]["logits"], got[1]["logits"][:, :5]) and torch.equal(got[-1]["logits"], got[B]["logits"][:, :Tar // 2])


# ---- 5. synthesis.py -----------------------------------------------------------------------------------------------------------------
def test_synthesis_script_writes_the_same_wavs_with_batch_coop(tmp_path, monkeypatch):
    """the set-up of tests/test_gpu_ar_list.py's script test with WAE_AR_COOP left at its default: the loop decodes cooperatively"""
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
    for dst, extra in (("loop/", []), ("teams/", ["--batch-decode", "--batch-coop", "--batch-teams", "2"])):
        _run([os.path.join(root, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
              "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp_path))
    names = sorted(p.name for p in (tmp_path / "loop" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    sizes = set()
    for n in names:
        a = (tmp_path / "loop" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "teams" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
        sizes.add(len(a))
    assert len(sizes) == len(names)                                    # four clips of four lengths
