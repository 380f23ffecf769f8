"""List decoding on the GPU (wae_ar_generate_list, WaeEngine.decode_list, synthesis.py --batch-decode): every item of a ragged list
is BITWISE what incremental_forward returns for that utterance alone on the one-CU kernel (WAE_AR_COOP=0) -- in every mode and
storage type, with and without conditioning, with per-item start classes and forced prefixes, whatever the number of slots and the
order of the list -- and the teacher-forced logits of the reference's own vectors keep the tolerances of tests/test_gpu_ar.py.
The lengths lie below, around and beyond the longest history ring of the 20-layer geometry (2 * 512 + 1 rows)."""
import json

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from test_gpu_ar_stream import HP, SMALL, _engine, _run, _tiny_dump_and_checkpoint

pytestmark = pytest.mark.gpu
LENS = [1500, 37, 2300, 640, 1, 1100, 911]
BARE = dict(SMALL, Cc=-1, Cg=-1, n_speakers=None)          # no local and no global conditioning
START = SMALL["O"] // 2 - 1                                # (the default start class, 127, needs more classes)


def _items(cfg, lens=LENS, seed=5):
    gen = torch.Generator().manual_seed(seed)
    cond = cfg["Cc"] > 0
    return [dict(T=T, c=torch.randn(cfg["Cc"], T, generator=gen).cuda() if cond else None,
                 gid=int(torch.randint(0, cfg["n_speakers"], (1,), generator=gen)) if cond else None,
                 uniforms=torch.rand(T, generator=gen).cuda(), init_idx=START) for T in lens]


def _alone(eng, it, mode, want_logits=True):
    """the item as a batch of one through incremental_forward (the engine was built with WAE_AR_COOP=0: the one-CU kernel)"""
    kw = dict(init_idx=it["init_idx"])
    if mode == "sample":
        kw["uniforms"] = it["uniforms"][None]
    if it.get("test_inputs") is not None:
        kw["test_inputs"] = it["test_inputs"][None]
    out = eng.incremental_forward(it["c"][None] if it["c"] is not None else None,
                                  torch.tensor([it["gid"]]).cuda() if it["gid"] is not None else None, it["T"], mode=mode,
                                  c_is_upsampled=True, want_logits=want_logits, **kw)
    assert getattr(eng, "_ar_profile", None) is None       # (the cooperative paths leave their error / profile words)
    return out["idx"][0].clone(), None if out["logits"] is None else out["logits"][0].clone()


def _equal(got, want, what):
    assert len(got) == len(want)
    for i, (g_, (idx, logits)) in enumerate(zip(got, want)):
        assert g_["idx"].shape == idx.shape and g_["idx"].dtype == torch.int32, (what, i)
        assert torch.equal(g_["idx"], idx), (what, i, "first difference at", (g_["idx"] != idx).nonzero()[:1].tolist())
        assert (g_["logits"] is None) == (logits is None), (what, i)
        if logits is not None:
            assert g_["logits"].shape == logits.shape and torch.equal(g_["logits"], logits), (what, i)


def _snapshot(res):
    return [(r["idx"].clone(), None if r["logits"] is None else r["logits"].clone()) for r in res]


@pytest.mark.parametrize("mode", ["argmax", "sample"])
@pytest.mark.parametrize("cond", [True, False], ids=["c_and_gid", "unconditioned"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_item_is_its_single_decode_bit_for_bit(dtype, cond, mode, monkeypatch):
    cfg = SMALL if cond else BARE
    eng = _engine(cfg, dtype, monkeypatch, coop="0")
    items = _items(cfg)
    got = eng.decode_list(items, mode=mode, want_logits=True)
    torch.cuda.synchronize()
    assert [r["idx"].shape[0] for r in got] == LENS and all(r["logits"].shape == (cfg["O"], T) for r, T in zip(got, LENS))
    got = _snapshot(got)
    _equal([dict(idx=a, logits=b) for a, b in got], [_alone(eng, it, mode) for it in items], (dtype, cond, mode))
    if mode == "sample":
        assert int(torch.unique(torch.cat([a for a, _ in got])).numel()) > cfg["O"] // 4   # real roll-outs, not a constant
    # logits only on request
    assert all(r["logits"] is None for r in eng.decode_list(items[:3], mode=mode))


def test_start_class_per_item(monkeypatch):
    eng = _engine(SMALL, "fp32", monkeypatch, coop="0")
    items = _items(SMALL)
    for it, s in zip(items, [3, 40, 62, 0, 63, 17, START]):
        it["init_idx"] = s
    got = _snapshot(eng.decode_list(items, mode="argmax", want_logits=True))
    _equal([dict(idx=a, logits=b) for a, b in got], [_alone(eng, it, "argmax") for it in items], "init_idx")
    same = eng.decode_list([dict(it, init_idx=START) for it in items], mode="argmax", want_logits=True)
    assert torch.equal(same[6]["idx"], got[6][0]) and torch.equal(same[6]["logits"], got[6][1])
    assert not torch.equal(same[0]["logits"][:, 0], got[0][1][:, 0])      # another start class, another first step
    with pytest.raises(IndexError):
        eng.decode_list([dict(items[1], init_idx=SMALL["O"])], mode="argmax")


def test_forced_prefix_shorter_than_the_item(monkeypatch):
    """items with a forced prefix (inside, and as long as, the item) beside items that run free from their start class"""
    eng = _engine(SMALL, "bf16", monkeypatch, coop="0")
    items = _items(SMALL)
    gen = torch.Generator().manual_seed(8)
    for i, F in ((0, 100), (2, 1500), (3, 640), (5, 1)):
        items[i]["test_inputs"] = torch.randint(0, SMALL["O"], (F,), generator=gen).cuda()
    got = _snapshot(eng.decode_list(items, mode="sample", want_logits=True))
    _equal([dict(idx=a, logits=b) for a, b in got], [_alone(eng, it, "sample") for it in items], "forced prefix")
    free = eng.decode_list([{k: v for k, v in it.items() if k != "test_inputs"} for it in items], mode="sample")
    assert not torch.equal(free[0]["idx"], got[0][0]) and torch.equal(free[1]["idx"], got[1][0])


@pytest.mark.parametrize("dtype,mode", [("fp32", "argmax"), ("bf16", "sample")])
def test_a_reused_slot_decodes_as_a_fresh_one(dtype, mode, monkeypatch):
    """more items than slots: a workgroup decodes one item after another in the same ring slot, which nobody clears in between"""
    eng = _engine(SMALL, dtype, monkeypatch, coop="0")
    items = _items(SMALL, lens=LENS + [1300, 2, 1026, 700])
    want = _snapshot(eng.decode_list(items, mode=mode, slots=len(items), want_logits=True))
    for slots in (2, 3, 1):
        got = eng.decode_list(items, mode=mode, slots=slots, want_logits=True)
        _equal(got, want, ("slots", slots))
    _equal(eng.decode_list(items, mode=mode, slots=4096, want_logits=True), want, "slots beyond the item count")


def test_the_order_of_the_list_does_not_matter(monkeypatch):
    eng = _engine(SMALL, "fp32", monkeypatch, coop="0")
    items = _items(SMALL)
    want = _snapshot(eng.decode_list(items, mode="sample", want_logits=True))
    perm = [4, 2, 6, 0, 5, 1, 3]
    got = eng.decode_list([items[j] for j in perm], mode="sample", slots=3, want_logits=True)
    _equal(got, [want[j] for j in perm], "permuted")


def test_draws_made_here_are_those_of_the_seeded_loop(monkeypatch):
    """no uniforms passed: item i's are torch.rand(1, T_i) in the caller's order -- with the seed reset per item, the loop's draws"""
    eng = _engine(SMALL, "fp32", monkeypatch, coop="0")
    items = [{k: v for k, v in it.items() if k != "uniforms"} for it in _items(SMALL, lens=[640, 37, 911])]
    torch.manual_seed(21)
    got = _snapshot(eng.decode_list(items, mode="sample"))
    torch.manual_seed(21)
    want = []
    for it in items:
        out = eng.incremental_forward(it["c"][None], torch.tensor([it["gid"]]).cuda(), it["T"], mode="sample", init_idx=START,
                                      c_is_upsampled=True)
        want.append((out["idx"][0].clone(), None))
    _equal([dict(idx=a, logits=b) for a, b in got], want, "seeded")


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
    got = eng.decode_list(items, mode="logits", slots=2, c_is_upsampled=True)
    torch.cuda.synchronize()
    logits = torch.stack([got[1 + b]["logits"] for b in range(B)]).cpu()
    assert rel_err(logits, z["tf_logits"]) < tol
    # the shorter items are prefixes of the same causal computation
    assert torch.equal(got[0]["logits"], got[1]["logits"][:, :5]) and torch.equal(got[-1]["logits"], got[B]["logits"][:, :Tar // 2])


def test_synthesis_script_writes_the_same_wavs_with_batch_decode(tmp_path, monkeypatch):
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
    monkeypatch.setenv("WAE_AR_COOP", "0")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dst, extra in (("loop/", []), ("list/", ["--batch-decode"])):
        _run([os.path.join(root, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"),
              "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp_path))
    names = sorted(p.name for p in (tmp_path / "loop" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    sizes = set()
    for n in names:
        a = (tmp_path / "loop" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp_path / "list" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
        sizes.add(len(a))
    assert len(sizes) == len(names)                                    # four clips of four lengths
