"""GPU: work lists of scalar-input utterances (wae_ar_generate_scalar_list, wae_ar_generate_coop_scalar_list,
WaeEngine.decode_list_scalar, synthesis.py --batch-decode on a "raw" model).  Every item of a ragged list is BITWISE what scalar
incremental_forward returns for that utterance alone -- on the one-CU kernel for the plain list, on the cooperative any-shape kernel at
the same C for the team list -- in both storage types, for the mixture of logistics and the mixture of Gaussians (O = 3M and O = 2),
with per-item speakers and forced prefixes, whatever the number of slots or teams and the order of the list.  Two geometries: golden
model S (4 layers, dilations 1 and 2: the longest ring has 5 rows; lengths below, at and beyond it) and a 20-layer geometry whose
longest ring has 2 * 512 + 1 rows (lengths around it).  Every cooperative run checks that the team launch really ran and that no wait
timed out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": 1e-4, "bf16": 5e-2}                      # tests/test_gpu_ar_scalar_coop.py
LENS_S = [1, 4, 5, 6, 40, 13, 64]
LENS_DEEP = [1100, 37, 1300, 640, 1, 1026]
DEEP = dict(layers=20, stacks=2, R=64, G=64, S=64, O=30, Cc=16, Cg=8, k=3, n_speakers=7, upsample_scales=None, cin_pad=0,
            scalar_input=True)
PATHS = [("one_cu", None), ("teams_C32", 32), ("teams_C3", 3)]


def _engine(geom, dtype, monkeypatch, C=None, dist="Logistic", O_ch=30):
    """C None: WAE_AR_COOP=0, every incremental_forward on the one-CU kernel; else the cooperative path on C members with the scalar
    opt-in (WAE_AR_COOP / WAE_AR_COOP_C are read when the engine is built)."""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    if geom == "S":
        cfg, sd, _, z, _ = golden_model("S")
        cfg = dict(cfg, output_distribution=dist)
        if O_ch != cfg["O"]:
            cfg["O"] = O_ch
            sd = O.make_state_dict(cfg, int(z["salt"]))
    else:
        cfg = dict(DEEP, output_distribution=dist, O=O_ch)
        sd = O.make_state_dict(dict(cfg), salt=7, with_encoder=False)
    monkeypatch.setenv("WAE_AR_COOP", "0" if C is None else "1")
    if C is not None:
        monkeypatch.setenv("WAE_AR_COOP_C", str(C))
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    if C is not None:
        eng.ar_path(scalar_coop=True)
        assert eng.opt.ar_coop and eng.opt.ar_coop_c == C
    eng.load_state_dict(sd)
    return eng, cfg


def _unit(shape, salt):
    return (O.hash_fill(shape, salt) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)


def _items(cfg, lens, salt=900):
    """conditioning, speaker and draws per item (O.hash_fill, the uniforms clamped to (1e-5, 1 - 1e-5))"""
    normal = cfg["output_distribution"] == "Normal"
    M = 1 if cfg["O"] == 2 else cfg["O"] // 3
    items = []
    for i, T in enumerate(lens):
        s = salt + 10 * i
        it = dict(T=T, c=O.hash_fill((cfg["Cc"], T), s + 1).cuda(), gid=(3 * i + 1) % cfg["n_speakers"])
        if not normal or M > 1:
            it["u_mix"] = _unit((T, M), s + 2).cuda()
        if normal:
            it["z"] = (O.hash_fill((T,), s + 3) * 1.7).cuda()
        else:
            it["u_log"] = _unit((T,), s + 4).cuda()
        items.append(it)
    return items


def _alone(eng, it, mode="sample", coop=False, want_logits=True):
    """the item as a batch of one through scalar incremental_forward, on the path the engine was built for"""
    kw = {k: it[k][None] for k in ("u_mix", "u_log", "z", "test_inputs") if it.get(k) is not None}
    if mode == "logits":
        kw = {k: v for k, v in kw.items() if k == "test_inputs"}
    eng._ar_profile = None
    out = eng.incremental_forward(it["c"][None], torch.tensor([it["gid"]]).cuda(), it["T"], mode=mode, c_is_upsampled=True,
                                  want_logits=want_logits, **kw)
    torch.cuda.synchronize()
    if coop:
        assert eng._ar_profile is not None, "the single decode fell back to the one-CU kernel"
        assert int(eng._ar_profile[0]) == 0
    else:
        assert eng._ar_profile is None, "the single decode took the cooperative path"
    return (None if out["x"] is None else out["x"][0].clone(), None if out["logits"] is None else out["logits"][0].clone())


def _list(eng, items, mode="sample", coop=False, **kw):
    eng._ar_profile = None
    got = eng.decode_list_scalar(items, mode=mode, coop=coop, c_is_upsampled=True, **kw)
    torch.cuda.synchronize()
    if coop:
        assert eng._ar_profile is not None, "the team launch did not run"
        assert int(eng._ar_profile[0]) == 0, eng._ar_profile[:8].tolist()
    else:
        assert eng._ar_profile is None
    return [(None if r["x"] is None else r["x"].clone(), None if r["logits"] is None else r["logits"].clone()) for r in got]


def _equal(got, want, what):
    assert len(got) == len(want)
    for i, ((x, p), (wx, wp)) in enumerate(zip(got, want)):
        for name, a, b in (("x", x, wx), ("logits", p, wp)):
            assert (a is None) == (b is None), (what, i, name)
            if a is not None:
                assert a.shape == b.shape and a.dtype == torch.float32, (what, i, name, a.shape, b.shape)
                assert torch.equal(a, b), (what, i, name, "first difference at", (a != b).nonzero()[:1].tolist())


# ---- 1. every item is its single decode, bit for bit --------------------------------------------------------------------------------
CASES = [("S", "Logistic", 30), ("S", "Normal", 30), ("S", "Normal", 2), ("deep", "Logistic", 30), ("deep", "Normal", 30)]


@pytest.mark.parametrize("path,C", PATHS, ids=[p for p, _ in PATHS])
@pytest.mark.parametrize("geom,dist,O_ch", CASES, ids=[f"{g}_{d}_O{o}" for g, d, o in CASES])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_item_is_its_single_decode(dtype, geom, dist, O_ch, path, C, monkeypatch):
    eng, cfg = _engine(geom, dtype, monkeypatch, C=C, dist=dist, O_ch=O_ch)
    lens = LENS_S if geom == "S" else LENS_DEEP
    items = _items(cfg, lens)
    coop = C is not None
    got = _list(eng, items, coop=coop, want_logits=True, **(dict(teams=3) if coop else dict(slots=4)))
    assert [x.shape for x, _ in got] == [(T,) for T in lens] and [p.shape for _, p in got] == [(O_ch, T) for T in lens]
    _equal(got, [_alone(eng, it, coop=coop) for it in items], (dtype, geom, dist, O_ch, path))
    xs = torch.cat([x for x, _ in got])
    assert float(xs.abs().max()) <= 1.0 and float(xs.std()) > 0.0                          # real roll-outs, not a constant
    assert all(p is None for _, p in _list(eng, items[:3], coop=coop))                      # parameters only on request


# ---- 2. a reused slot or team decodes as a fresh one ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dist", [("fp32", "Logistic"), ("bf16", "Normal")])
def test_a_reused_slot_decodes_as_a_fresh_one(dtype, dist, monkeypatch):
    """more items than slots: a workgroup decodes one item after another in the same ring slot, which nobody clears in between"""
    eng, cfg = _engine("deep", dtype, monkeypatch, dist=dist)
    items = _items(cfg, LENS_DEEP + [2, 1025])
    want = _list(eng, items, want_logits=True, slots=len(items))
    for slots in (1, 2, 3):
        _equal(_list(eng, items, want_logits=True, slots=slots), want, ("slots", slots))
    small, cfg_s = _engine("S", dtype, monkeypatch, dist=dist)
    its = _items(cfg_s, LENS_S)
    want = _list(small, its, want_logits=True, slots=len(its))
    for slots in (1, 2, 3):
        _equal(_list(small, its, want_logits=True, slots=slots), want, ("model S, slots", slots))


@pytest.mark.parametrize("dtype,dist", [("fp32", "Normal"), ("bf16", "Logistic")])
def test_a_reused_team_decodes_as_a_fresh_one(dtype, dist, monkeypatch):
    """more items than teams: a team decodes one item after another in the same rings, with the same exchange buffers running on"""
    eng, cfg = _engine("deep", dtype, monkeypatch, C=32, dist=dist)
    items = _items(cfg, LENS_DEEP + [2, 1025])
    want = _list(eng, items, coop=True, want_logits=True, teams=8)
    for teams in (1, 2):
        _equal(_list(eng, items, coop=True, want_logits=True, teams=teams), want, ("teams", teams))
    # one team, longest first: the 1300-step item directly followed by items of 37, 2 and 1 steps (stale history rows, wrong cursors)
    short = [items[2], items[1], items[6], items[4]]
    assert [it["T"] for it in short] == [1300, 37, 2, 1]
    _equal(_list(eng, short, coop=True, want_logits=True, teams=1), [want[2], want[1], want[6], want[4]], "one team, long then short")
    small, cfg_s = _engine("S", dtype, monkeypatch, C=3, dist=dist)
    its = _items(cfg_s, LENS_S)
    want = _list(small, its, coop=True, want_logits=True, teams=8)
    for teams in (1, 2):
        _equal(_list(small, its, coop=True, want_logits=True, teams=teams), want, ("model S, teams", teams))


# ---- 3. order ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,C", PATHS[:2], ids=[p for p, _ in PATHS[:2]])
def test_a_permuted_list_gives_permuted_results(path, C, monkeypatch):
    eng, cfg = _engine("deep", "fp32", monkeypatch, C=C)
    items = _items(cfg, LENS_DEEP)
    coop = C is not None
    want = _list(eng, items, coop=coop, want_logits=True)
    perm = [4, 2, 0, 5, 1, 3]
    how = dict(teams=2) if coop else dict(slots=3)
    _equal(_list(eng, [items[j] for j in perm], coop=coop, want_logits=True, **how), [want[j] for j in perm], "permuted")


# ---- 4. forced prefixes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,C", PATHS, ids=[p for p, _ in PATHS])
def test_forced_prefix_per_item(path, C, monkeypatch):
    """forced prefixes shorter than, and as long as, the item beside free-running items; mode "logits" on fully forced items"""
    eng, cfg = _engine("deep", "bf16", monkeypatch, C=C)
    coop = C is not None
    items = _items(cfg, LENS_DEEP)
    for i, F in ((0, 100), (2, 1300), (3, 1), (5, 1025)):
        items[i]["test_inputs"] = (O.hash_fill((F,), 950 + i) * 0.9).cuda()
    got = _list(eng, items, coop=coop, want_logits=True, **(dict(teams=2) if coop else dict(slots=3)))
    _equal(got, [_alone(eng, it, coop=coop) for it in items], "forced prefixes")
    free = _list(eng, [{k: v for k, v in it.items() if k != "test_inputs"} for it in items], coop=coop)
    assert not torch.equal(free[0][0], got[0][0]) and torch.equal(free[1][0], got[1][0])   # a free item differs from its forced twin
    # mode "logits": every item forced throughout; no draws, no samples
    forced = [dict(T=it["T"], c=it["c"], gid=it["gid"], test_inputs=(O.hash_fill((it["T"],), 970 + i) * 0.9).cuda())
              for i, it in enumerate(items)]
    tf = _list(eng, forced, mode="logits", coop=coop, **(dict(teams=2) if coop else dict(slots=3)))
    assert all(x is None for x, _ in tf)
    _equal(tf, [_alone(eng, it, mode="logits", coop=coop) for it in forced], "mode logits")
    with pytest.raises(ValueError, match="must cover all"):
        eng.decode_list_scalar([dict(forced[1], test_inputs=forced[1]["test_inputs"][:5])], mode="logits", coop=coop, c_is_upsampled=True)


# ---- 5. the reference's own vectors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,C", PATHS, ids=[p for p, _ in PATHS])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_teacher_forced_parameters_against_the_reference(dtype, path, C, monkeypatch):
    """the teacher-forced parameters of the golden ar_S utterances (tests/test_gpu_ar_scalar_coop.py: fp32 1e-4, bf16 5e-2), as items
    among others of other lengths; the shorter items are exact prefixes of the same causal computation"""
    eng, cfg = _engine("S", dtype, monkeypatch, C=C)
    _, _, ins, _, _ = golden_model("S")
    z = load_npz("ar_S")
    c_up = torch.from_numpy(z["c_up"]).cuda()
    B, _, Tar = c_up.shape
    x, g = ins["x"][:, 0, :Tar].cuda(), ins["g"]
    item = lambda b, T: dict(T=T, c=c_up[b, :, :T].contiguous(), gid=int(g[b]), test_inputs=x[b, :T].contiguous())  # noqa: E731
    items = [item(0, 5)] + [item(b, Tar) for b in range(B)] + [item(B - 1, Tar - 3), item(0, 1), item(B - 1, Tar // 2)]
    coop = C is not None
    got = _list(eng, items, mode="logits", coop=coop, **(dict(teams=2) if coop else dict(slots=2)))
    params = torch.stack([got[1 + b][1] for b in range(B)]).cpu()
    err = rel_err(params, z["params_tf"])
    print(f"scalar list {path} {dtype}: teacher-forced parameters rel err {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype]
    assert torch.equal(got[0][1], got[1][1][:, :5]) and torch.equal(got[-1][1], got[B][1][:, :Tar // 2])
    assert torch.equal(got[-3][1], got[B][1][:, :Tar - 3]) and torch.equal(got[-2][1], got[1][1][:, :1])


# ---- 6. the draw is the parameters' draw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,C", PATHS[:2], ids=[p for p, _ in PATHS[:2]])
@pytest.mark.parametrize("dist,O_ch", [("Logistic", 30), ("Normal", 30), ("Normal", 2)])
def test_draw_is_the_sampler_kernel_on_the_returned_parameters(dist, O_ch, path, C, monkeypatch):
    """wae_dmol_sample / wae_mog_sample on an item's returned parameters and its draws give its returned samples bit for bit"""
    from wavenet_autoencoders_amd import _lib as L
    eng, cfg = _engine("S", "fp32", monkeypatch, C=C, dist=dist, O_ch=O_ch)
    items = _items(cfg, LENS_S)
    M = 1 if O_ch == 2 else O_ch // 3
    got = _list(eng, items, coop=C is not None, want_logits=True)
    for it, (xs, params) in zip(items, got):
        T = it["T"]
        params, again = params.contiguous(), torch.empty(T, device="cuda")
        if dist == "Logistic":
            L.check(L.lib().wae_dmol_sample(L.ptr(params), L.ptr(it["u_mix"]), L.ptr(it["u_log"]), L.ptr(again), 1, M, T, -7.0, 0, None),
                    "dmol_sample")
        else:
            L.check(L.lib().wae_mog_sample(L.ptr(params), L.ptr(it["u_mix"]) if M > 1 else None, L.ptr(it["z"]), L.ptr(again), 1, O_ch, T,
                                           None), "mog_sample")
        torch.cuda.synchronize()
        assert torch.equal(again, xs), (T, float((again - xs).abs().max()))
    xs = torch.cat([x for x, _ in got])
    assert float(xs.abs().max()) <= 1.0 and float(xs.min()) < float(xs.max())


# ---- 7. draws made here ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["Logistic", "Normal"])
def test_draws_made_here_are_those_of_the_seeded_loop(dist, monkeypatch):
    """no draws passed: item i's are incremental_forward's expressions in the caller's order.  One seed in front of the list against
    one seed in front of the loop (the generator runs on from item to item), and the seed reset before every item (lists of one)."""
    eng, cfg = _engine("deep", "fp32", monkeypatch, dist=dist)
    items = [dict(T=it["T"], c=it["c"], gid=it["gid"]) for it in _items(cfg, [640, 37, 911])]
    alone = lambda it: eng.incremental_forward(it["c"][None], torch.tensor([it["gid"]]).cuda(), it["T"], mode="sample",  # noqa: E731
                                               c_is_upsampled=True)["x"][0].clone()
    torch.manual_seed(21)
    got = _list(eng, items, slots=2)
    torch.manual_seed(21)
    want = [(alone(it), None) for it in items]
    _equal(got, want, "one seed")
    assert not torch.equal(got[0][0][:37], got[1][0])
    per_item, loop = [], []
    for it in items:
        torch.manual_seed(33)
        per_item += _list(eng, [it])
        torch.manual_seed(33)
        loop.append((alone(it), None))
    _equal(per_item, loop, "seed reset per item")


def test_draws_of_the_wrong_kind_are_refused(monkeypatch):
    eng, cfg = _engine("S", "fp32", monkeypatch)
    it = _items(cfg, [8])[0]
    with pytest.raises(ValueError, match="not z"):
        eng.decode_list_scalar([dict(it, z=torch.zeros(8))], c_is_upsampled=True)
    with pytest.raises(ValueError, match="come together"):
        eng.decode_list_scalar([{k: v for k, v in it.items() if k != "u_log"}], c_is_upsampled=True)
    eng, cfg = _engine("S", "fp32", monkeypatch, dist="Normal")
    it = _items(cfg, [8])[0]
    with pytest.raises(ValueError, match="not u_log"):
        eng.decode_list_scalar([dict(it, u_log=torch.full((8,), 0.5))], c_is_upsampled=True)
    with pytest.raises(ValueError, match="need u_mix"):
        eng.decode_list_scalar([{k: v for k, v in it.items() if k != "u_mix"}], c_is_upsampled=True)


# ---- 8. synthesis.py ------------------------------------------------------------------------------------------------------------------
HP = ("layers=4,residual_channels=32,gate_channels=64,skip_out_channels=32,encoder_hid=32,cin_channels=16,gin_channels=8,"
      "n_speakers=5,batch_size=2,max_time_steps=2560,checkpoint_interval=1000,input_type=raw,out_channels=30,"
      "output_distribution=Normal,log_scale_min=-7.0")          # tests/test_gpu_mog.py


def _run(args, cwd, **env):
    p = subprocess.run([sys.executable] + args, cwd=cwd, env=dict(os.environ, PYTHONPATH=ROOT, **env), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.fixture(scope="module")
def raw_checkpoint(tmp_path_factory):
    """a tiny "raw" checkpoint (the dump and train step of tests/test_gpu_mog.py) and four test clips of four lengths"""
    tmp = tmp_path_factory.mktemp("scalar_list")
    rng = np.random.default_rng(6)
    dump, lines = tmp / "dump", []
    for u in range(3):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 40 + 4 * u
        np.save(d / "wave.npy", (0.3 * np.sin(np.arange(n * 160) * (0.05 + 0.01 * u)) + 0.05 * rng.standard_normal(n * 160))
                .astype(np.float32))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    preset = os.path.join(ROOT, "hps", "vqwae.json")
    _run([os.path.join(ROOT, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(tmp / "ck"), "--preset", preset,
          "--hparams", HP, "--max-steps", "1", "--dtype", "fp32"], str(tmp))
    pairs = []
    for fid, frames, tar in (("0007", 8, "V1"), ("0011", 16, "V2"), ("0012", 4, "V1"), ("0013", 12, "V3")):
        utt = dump / "test" / f"S0_{fid}"
        utt.mkdir(parents=True)
        np.save(utt / "mfcc.norm.npy", rng.standard_normal((frames, 39)).astype(np.float32))
        pairs.append((f"S0_{fid}", tar))
    (tmp / "syn.txt").write_text("".join(f"test/{s} {t}\n" for s, t in pairs))
    (tmp / "spk.json").write_text(json.dumps({"V1": 2, "V2": 0, "V3": 4}))
    return tmp, dump, tmp / "ck" / "checkpoint_latest.pth", preset, pairs


@pytest.mark.parametrize("loop,batch", [((dict(WAE_AR_COOP="0"), []), (dict(), ["--batch-decode"])),
                                        ((dict(), ["--coop-scalar"]), (dict(), ["--batch-decode", "--batch-coop", "--batch-teams", "2"]))],
                         ids=["batch_decode_is_the_one_cu_loop", "batch_coop_is_the_coop_scalar_loop"])
def test_synthesis_script_writes_the_loops_wavs(loop, batch, raw_checkpoint, monkeypatch):
    tmp, dump, ckpt, preset, pairs = raw_checkpoint
    monkeypatch.delenv("WAE_AR_COOP", raising=False)
    monkeypatch.delenv("WAE_AR_COOP_C", raising=False)
    tag = "coop" if "--coop-scalar" in loop[1] else "one_cu"
    for dst, (env, extra) in ((f"{tag}_loop/", loop), (f"{tag}_batch/", batch)):
        _run([os.path.join(ROOT, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp / "syn.txt"), str(tmp / "spk.json"), "english", "160",
              "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra, str(tmp), **env)
    names = sorted(p.name for p in (tmp / f"{tag}_loop" / "2019" / "english" / "test").iterdir())
    assert names == sorted(f"{t}_{s.split('_')[1]}.wav" for s, t in pairs)
    sizes = set()
    for n in names:
        a = (tmp / f"{tag}_loop" / "2019" / "english" / "test" / n).read_bytes()
        b = (tmp / f"{tag}_batch" / "2019" / "english" / "test" / n).read_bytes()
        assert a == b, n
        sizes.add(len(a))
    assert len(sizes) == len(names)                                    # four clips of four lengths
    from scipy.io import wavfile
    sr, y = wavfile.read(tmp / f"{tag}_batch" / "2019" / "english" / "test" / names[0])
    assert np.isfinite(y).all() and float(np.abs(y).max()) > 0
