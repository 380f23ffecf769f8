"""Ragged micro-batches in accumulation windows: WaeEngine.accumulate_list / train_step_list_accum, and the fixed-order tap gradient
of the list upsampling backward (wae_upsample_stage_bwd_list_det) with the deterministic ragged window it makes possible.

The window's definition is train_step_list on the concatenation of its groups: the same addends in another order, so the bounds are
tests/test_gpu_accum.py's _tol (gradients within 2e-5 / 2e-3 of max|g|, parameters within 1e-5 / 2e-3, losses within 1e-5 / 2e-3,
perplexity within 1e-6 relative; fp32 / 16-bit).  Against autograd through the oracle the bounds are tests/test_gpu_train_list.py's
(rel_err < 2e-3 per gradient tensor, ce within 1e-4, vq_loss within 1e-5).  The per-kernel cases are exact: integer operands whose
float64 sums of |terms| stay below 2^22, so fp32 arithmetic is exact in any order and the assertion is torch.equal.  In the
deterministic mode two engines agree in every bit."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frontend_list_ref as RL
from helpers import golden_model
from oracle import wae_oracle as O
from test_gpu_accum import W_CFG, _tol
from test_gpu_train_list import _items, _oracle, _per_tensor

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3
DEV = "cuda"
SPLITS = {"2+2": [[0, 1], [2, 3]], "1+3": [[3], [0, 1, 2]], "1+1+1+1": [[0], [1], [2], [3]]}


def _engine(cfg, sd, dtype, strict=True, **kw):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype, **kw)
    eng.load_state_dict(sd, strict=strict)
    eng.init_optimizer()
    return eng


def _numbers(res):
    return {k: float(v) for k, v in res.items() if k in ("loss", "ce", "vq_loss", "perp", "grad_norm")}


def _groups(items, split):
    return [[items[i] for i in grp] for grp in split]


def _step(eng, call):
    """one step through `call(eng, grad_hook)` -> (numbers, gradients, parameters, the step's dict)"""
    seen = {}
    res = call(eng, lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    eng.check_errors()
    return _numbers(res), seen["g"].cpu(), eng.params.cpu().clone(), res


def _close(got, ref, dtype, what=""):
    """item 1's bounds; prints every figure before it asserts"""
    tol = _tol(dtype)
    (n0, g0, p0), (n1, g1, p1) = got[:3], ref[:3]
    gerr, gmax, perr = float((g0 - g1).abs().max()), float(g1.abs().max()), float((p0 - p1).abs().max())
    lerr = {k: abs(n0[k] - n1[k]) for k in ("loss", "ce", "vq_loss") if k in n1}
    print(f"{what} {dtype}: grad err {gerr:.3e} of max|g| {gmax:.3e} ({gerr / gmax:.2e}), param err {perr:.3e}, losses {lerr}, "
          f"perp {n0.get('perp')} vs {n1.get('perp')}, grad_norm {n0['grad_norm']} vs {n1['grad_norm']}")
    assert gerr <= tol["g"] * gmax
    assert perr < tol["p"]
    assert all(v < tol["l"] for v in lerr.values()), lerr
    if "perp" in n1:
        assert abs(n0["perp"] - n1["perp"]) <= 1e-6 * n1["perp"]


_UNION, _WINDOW = {}, {}


def _union(dtype):
    """train_step_list on all four utterances; computed once per dtype"""
    if dtype not in _UNION:
        cfg, sd = golden_model("A")[:2]
        _UNION[dtype] = _step(_engine(cfg, sd, dtype), lambda e, hook: e.train_step_list(_items(cfg), lr=LR, grad_hook=hook))[:3]
    return _UNION[dtype]


def _window(dtype, split):
    """train_step_list_accum on the split (default mode); computed once per (dtype, split)"""
    if (dtype, split) not in _WINDOW:
        cfg, sd = golden_model("A")[:2]
        eng = _engine(cfg, sd, dtype)
        groups = _groups(_items(cfg), SPLITS[split])
        n, g, p, res = _step(eng, lambda e, hook: e.train_step_list_accum(groups, lr=LR, grad_hook=hook))
        assert res["micro_batches"] == len(groups) and eng.window is None and eng.opt_step == 1
        Ts = [[it["x"].shape[0] for it in grp] for grp in groups]
        assert res["rows"] == sum(len(t) * max(t) for t in Ts) and res["pad_rows"] == res["rows"] - 9600
        _WINDOW[(dtype, split)] = (n, g, p, eng.lay)
    return _WINDOW[(dtype, split)]


# ---------------------------------------------------------------- 1. the window against the union
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("split", list(SPLITS))
def test_window_equals_the_list_step_on_the_union(split, dtype):
    _close(_window(dtype, split), _union(dtype), dtype, f"A {split}")


# ---------------------------------------------------------------- 2. against the oracle
def test_window_against_autograd_through_the_oracle():
    cfg = golden_model("A")[0]
    ref, ce_o, vq_o = _oracle(_items(cfg))
    n, grads, _, lay = _window("fp32", "2+2")
    print(f"ce {n['ce']} (oracle {ce_o}), vq_loss {n['vq_loss']} (oracle {vq_o})")
    assert abs(n["ce"] - ce_o) < 1e-4 and abs(n["vq_loss"] - vq_o) < 1e-5
    errs = _per_tensor(lay, grads, ref)
    print({k: f"{e:.2e}" for k, e in errs.items() if e > 2e-4})
    bad = {k: e for k, e in errs.items() if not e < 2e-3}
    assert not bad, bad


# ---------------------------------------------------------------- 3. a dense and a ragged micro-batch in one window
def test_mixed_window_against_autograd_through_the_oracle():
    """accumulate (two clips of 8 frames) + accumulate_list (utterances of 12 and 4 frames) under accum_weights, fp32: the oracle's
    gradient of  sum_i w_ce_i ce_i + w_vq_i vq_i,  the dense micro-batch a batch of two, the ragged one utterance by utterance"""
    from wavenet_autoencoders_amd import packing as P
    from wavenet_autoencoders_amd import train as TR
    from wavenet_autoencoders_amd.distributed import accum_weights
    cfg, sd, _, _, ocfg = golden_model("A")
    gen = torch.Generator().manual_seed(77)
    x = torch.randint(0, cfg["O"], (2, 1280), generator=gen)
    c = torch.randn(2, cfg["c_in"], 8, generator=gen)
    g = torch.tensor([4, 1])
    items = _items(cfg)[1:3]
    eng = _engine(cfg, sd, "fp32")
    tp = P.train_list_plan(eng.g, [it["x"].shape[0] for it in items], [it["c"].shape[1] for it in items])
    metas = [(2, 1280, None, eng.latent_elements(2, 8)), TR.list_meta(eng.g, tp)]
    weights, N = accum_weights(metas)
    assert N == 2 * 1279 + 1919 + 639 and [m[3] for m in metas] == [2 * 16 * 2, 16 * 4]
    seen = {}
    eng.accumulate(x.cuda(), c.cuda(), g.cuda(), None, ce_weight=weights[0][0], vq_weight=weights[0][1], ce_count=N)
    r = eng.accumulate_list(items, ce_weight=weights[1][0], vq_weight=weights[1][1], ce_count=N)
    assert r["rows"] == 2 * 1920 and r["pad_rows"] == 1280 and eng.window.n == 2
    res = eng.apply_step(lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    eng.check_errors()
    assert res["micro_batches"] == 2 and eng.window is None and eng.opt_step == 1
    psd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xin = torch.nn.functional.one_hot(x, cfg["O"]).float().transpose(1, 2).contiguous()
    y, vq_d, _, _ = O.vqvae_forward(psd, ocfg, xin, c, g)
    ce_d = O.masked_ce_loss(y, x.unsqueeze(-1), torch.tensor([1280, 1280]))
    nll, n, vqs, tqs = 0.0, 0, [], []
    for it in items:
        T = it["x"].shape[0]
        xi = torch.nn.functional.one_hot(it["x"][None], cfg["O"]).float().transpose(1, 2).contiguous()
        yi, vq, _, _ = O.vqvae_forward(psd, ocfg, xi, it["c"][None], torch.tensor([it["gid"]]))
        nll = nll + O.masked_ce_loss(yi, it["x"][None].unsqueeze(-1), torch.tensor([T])) * (T - 1)
        n += T - 1
        vqs.append(vq)
        tqs.append(T // 640)
    ce_l, vq_l = nll / n, sum(v * (t / sum(tqs)) for v, t in zip(vqs, tqs))
    ce_o = weights[0][0] * ce_d + weights[1][0] * ce_l
    vq_o = weights[0][1] * vq_d + weights[1][1] * vq_l
    (ce_o + vq_o).backward()
    ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in psd.items()}
    print(f"ce {float(res['ce'])} (oracle {float(ce_o)}), vq_loss {float(res['vq_loss'])} (oracle {float(vq_o)})")
    assert abs(float(res["ce"]) - float(ce_o)) < 1e-4 and abs(float(res["vq_loss"]) - float(vq_o)) < 1e-5
    errs = _per_tensor(eng.lay, seen["g"].cpu(), ref)
    bad = {k: e for k, e in errs.items() if not e < 2e-3}
    assert not bad, bad


# ---------------------------------------------------------------- 4. the static weight-gradient launch
class _Counting:
    """the library with every entry that is looked up written down"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._lib, name)


def _items_w(tcs=(3, 2, 1, 3), seed=377):
    gen = torch.Generator().manual_seed(seed)
    return [dict(x=torch.randint(0, 256, (640 * tc,), generator=gen), c=torch.randn(W_CFG["Cc"], tc, generator=gen),
                 gid=int(torch.randint(0, W_CFG["n_speakers"], (1,), generator=gen))) for tc in tcs]


def test_window_on_the_static_launch_geometry():
    """W (10 layers, R = G = S = 256, decoder only), bf16, items c (Cc, Tc) with Tc = 3, 2, 1, 3: the window of 2 + 2 against the union;
    then a window whose second group (33 items: B > 32) takes the tile launches where the first took the static one"""
    from wavenet_autoencoders_amd import backward as BW
    sd = O.make_state_dict(dict(W_CFG), salt=9, with_encoder=False)
    items = _items_w()
    ref = _step(_engine(W_CFG, sd, "bf16", strict=False), lambda e, hook: e.train_step_list(items, lr=LR, grad_hook=hook))
    eng = _engine(W_CFG, sd, "bf16", strict=False)
    got = _step(eng, lambda e, hook: e.train_step_list_accum(_groups(items, SPLITS["2+2"]), lr=LR, grad_hook=hook))
    assert got[3]["micro_batches"] == 2 and got[3]["rows"] == 2 * 1920 + 2 * 1920 and got[3]["pad_rows"] == 640 + 1280
    assert "vq_loss" not in got[3] and eng.window is None and eng.opt_step == 1
    _close(got, ref, "bf16", "W 2+2")
    # another launch in the same window
    assert BW.window_kind(eng, 2, 1920) is True and BW.window_kind(eng, 33, 640) is False
    eng.accumulate_list(items[:2], ce_weight=0.5)
    torch.cuda.synchronize()
    snap = (eng.cbuf.clone(), eng.d_eff.clone(), eng.window.sums.clone())
    many = _items_w(tcs=(1,) * 33, seed=5)
    calls, real, drops, saved = [], eng.lib, eng.drop_calls, eng.saved
    eng.lib = _Counting(real, calls)
    try:
        with pytest.raises(ValueError, match="another weight-gradient launch"):
            eng.accumulate_list(many, ce_weight=0.5)
    finally:
        eng.lib = real
    torch.cuda.synchronize()
    assert calls == [] and eng.window is not None and eng.window.n == 1 and eng.saved is saved and eng.drop_calls == drops
    for a, b in zip(snap, (eng.cbuf, eng.d_eff, eng.window.sums)):
        assert torch.equal(a, b)
    eng.discard_step()


# ---------------------------------------------------------------- 5. window mechanics
def test_window_of_one_group_with_dropout_is_the_list_step():
    """dropout masks follow the engine's call counter: a window of ONE group draws train_step_list's masks"""
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    out = []
    for how in ("list", "window"):
        eng = _engine(cfg, sd, "bf16", dropout=0.05)
        if how == "list":
            out.append(_step(eng, lambda e, hook: e.train_step_list(items, lr=LR, grad_hook=hook)))
        else:
            out.append(_step(eng, lambda e, hook: e.train_step_list_accum([items], lr=LR, grad_hook=hook)))
        assert eng.drop_calls == 1
    _close(out[1], out[0], "bf16", "dropout")


def _state(eng):
    return dict(params=eng.params.clone(), exp_avg=eng.exp_avg.clone(), exp_avg_sq=eng.exp_avg_sq.clone(), shadow=eng.shadow.clone(),
                opt_step=eng.opt_step)


class _FailingAt:
    """the library whose entry `name` raises where it is looked up: a micro-batch that ends half-way"""

    def __init__(self, lib, name):
        self._lib, self._name = lib, name

    def __getattr__(self, name):
        if name == self._name:
            raise RuntimeError(f"{name}: refused for the test")
        return getattr(self._lib, name)


@pytest.mark.parametrize("how", ["discarded", "refused"])
def test_a_dropped_window_leaves_nothing_behind(how):
    """discard_step after one accumulate_list / a second micro-batch that fails in its backward (the window goes with it), then
    train_step_list(items): against a fresh engine's train_step_list(items)"""
    dtype = "bf16"
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    eng = _engine(cfg, sd, dtype, dropout=0.05)
    eng.accumulate_list(items[:2], ce_weight=0.5, vq_weight=0.5)
    assert eng.window is not None and eng.window.n == 1 and eng.drop_calls == 1
    if how == "discarded":
        eng.discard_step()
    else:
        real = eng.lib
        eng.lib = _FailingAt(real, "wae_from_btc_list")
        try:
            with pytest.raises(RuntimeError, match="refused for the test"):
                eng.accumulate_list(items[2:], ce_weight=0.5, vq_weight=0.5)
        finally:
            eng.lib = real
    torch.cuda.synchronize()
    assert eng.window is None and eng.opt_step == 0 and eng.drop_calls == 0 and eng.flight.accum is None
    assert float(eng.cbuf.abs().max()) == 0 and float(eng.d_eff.abs().max()) == 0
    with pytest.raises(RuntimeError, match="accumulate"):
        eng.apply_step()
    got = _step(eng, lambda e, hook: e.train_step_list(items, lr=LR, grad_hook=hook))
    ref = _step(_engine(cfg, sd, dtype, dropout=0.05), lambda e, hook: e.train_step_list(items, lr=LR, grad_hook=hook))
    _close(got, ref, dtype, how)


def test_refusals_come_before_any_launch():
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    calls = []

    class Sync:
        world = 1

    def refused(eng, exc, match, call):
        eng.prepare_weights()
        torch.cuda.synchronize()
        real, drops, saved = eng.lib, eng.drop_calls, eng.saved
        eng.lib = _Counting(real, calls)
        try:
            with pytest.raises(exc, match=match):
                call(eng)
        finally:
            eng.lib = real
        assert calls == [] and eng.window is None and eng.saved is saved and eng.drop_calls == drops and eng.opt_step == 0, (match, calls)

    eng = _engine(cfg, sd, "fp32", dropout=0.05)
    short = [dict(it) for it in items]
    short[2] = dict(short[2], x=short[2]["x"][:-1])
    refused(eng, ValueError, "item 2 has 639 samples", lambda e: e.accumulate_list(short))
    refused(eng, ValueError, "group 1.*item 0 has 639 samples", lambda e: e.train_step_list_accum([items[:2], short[2:]]))
    refused(eng, ValueError, "max_rows", lambda e: e.accumulate_list(items, max_rows=4 * 5760 - 1))
    refused(eng, ValueError, "empty", lambda e: e.accumulate_list([]))
    refused(eng, ValueError, "no groups", lambda e: e.train_step_list_accum([]))
    refused(eng, ValueError, "group 1.*empty", lambda e: e.train_step_list_accum([items, []]))
    refused(eng, NotImplementedError, "grad_sync", lambda e: e.train_step_list_accum([items], grad_sync=Sync()))
    for extra, match in ((dict(cin_pad=1), "cin_pad"), (dict(up_act="ReLU"), "upsample_activation"), (dict(vq="sliced", vq_slices=2), "quantiser")):
        e2 = WaeEngine(Geometry.from_cfg(dict(cfg, **extra)), dtype="fp32")
        e2.init_optimizer()
        refused(e2, NotImplementedError, match, lambda e: e.accumulate_list(items))
        refused(e2, NotImplementedError, match, lambda e: e.train_step_list_accum([items]))
    # inside an open window a whole step is refused, and the window stays
    eng.accumulate_list(items[:2], ce_weight=0.5, vq_weight=0.5)
    with pytest.raises(RuntimeError, match=r"apply_step\(\).*discard_step\(\)"):
        eng.train_step_list_accum([items])
    assert eng.window is not None and eng.window.n == 1
    eng.discard_step()


# ---------------------------------------------------------------- 6. the training script
def test_train_script_with_train_packed_and_accum_steps(tmp_path):
    """vqwae_train.py --train-packed --accum-steps 2 for two optimizer steps on the synthetic dump of
    tests/test_gpu_train_list.py::test_train_script_with_train_packed with five utterances, in ONE child process"""
    from test_gpu_scripts import HP
    rng = np.random.default_rng(5)
    dump = tmp_path / "dump"
    lines = []
    for u in range(5):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 41 + 4 * u
        np.save(d / "wave.npy", rng.integers(0, 256, n * 160).astype(np.int16))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    preset = json.load(open(os.path.join(ROOT, "hps", "vqwae.json")))
    preset["max_time_steps"] = None
    (tmp_path / "preset.json").write_text(json.dumps(preset))
    hp = ",".join(kv for kv in HP.split(",") if not kv.startswith("max_time_steps=")) + ",train_eval_interval=1000"
    ck = tmp_path / "ck"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(ck),
                        "--preset", str(tmp_path / "preset.json"), "--hparams", hp, "--max-steps", "2", "--dtype", "fp32",
                        "--train-packed", "--accum-steps", "2"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Finished" in p.stdout and "step 1 loss" in p.stdout
    assert "2 optimizer steps of 2 micro-batches: 4 batches consumed" in p.stdout
    saved = torch.load(ck / "checkpoint_latest.pth", map_location="cpu")
    assert saved["global_step"] == 2


# ---------------------------------------------------------------- 7. wae_upsample_stage_bwd_list_det alone
U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 22
SENT = 12288.0
UP_TINS = [1, 2, 3, 17, 65, 129]
UP_CASES = [(s, C) for s in (4, 5, 8, 16, 3) for C in (3, 16)]


def _ints(rng, *shape):
    return torch.from_numpy(rng.randint(-3, 4, size=shape).astype(np.float32))


def _prefill(rng, *shape):
    return torch.from_numpy(rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=shape))


def _gauss(rng, *shape):
    return torch.from_numpy(rng.randn(*shape).astype(np.float32))


def _up_operands(rng, tins, s, C, draw):
    Tin = np.asarray(tins)
    Tout = Tin * s
    in_off, in_pitch = RL.scattered_offsets(Tin, rng)
    out_off, out_pitch = RL.scattered_offsets(Tout, rng)
    ins = [draw(rng, C, int(t)) for t in Tin]
    douts = [draw(rng, C, int(t)) for t in Tout]
    return dict(Tin=Tin, Tout=Tout, in_off=in_off, in_pitch=in_pitch, out_off=out_off, out_pitch=out_pitch, ins=ins, douts=douts,
                w=draw(rng, 2 * s + 1), pre=_prefill(rng, 2 * s + 1), s=s, C=C)


def _call_up(op, det, order=None):
    """one call of the default or the fixed-order entry on fresh outputs -> (din (C, in_pitch), dw) on the host"""
    from wavenet_autoencoders_amd import _lib as L
    from wavenet_autoencoders_amd import packing as P
    lib = L.lib()
    order = np.arange(len(op["Tin"])) if order is None else np.asarray(order)
    recs, ntiles = P.ups_list_records(op["in_off"][order], op["Tin"][order], op["out_off"][order], op["Tout"][order], P.UPS_LIST_TILE_CT)
    rd = torch.from_numpy(recs).to(DEV)
    dout = RL.pack(op["douts"], op["out_off"], op["out_pitch"], RL.GAP_FILL).to(DEV)
    inp = RL.pack(op["ins"], op["in_off"], op["in_pitch"], RL.GAP_FILL).to(DEV)
    w, dw = op["w"].to(DEV), op["pre"].to(DEV)
    din = torch.full((op["C"], op["in_pitch"]), SENT, device=DEV)
    args = (L.ptr(dout), L.ptr(inp), L.ptr(w), L.ptr(din), L.ptr(dw), L.ptr(rd), len(recs) - 1, ntiles, op["in_pitch"], op["out_pitch"],
            op["C"], op["s"])
    if det:
        n = int(lib.wae_upsample_stage_bwd_list_det_floats())
        parts = torch.full((n,), float("nan"), device=DEV)          # (never cleared by the caller: every row read was stored before)
        L.check(lib.wae_upsample_stage_bwd_list_det(*args, L.ptr(parts), n, None), "upsample_stage_bwd_list_det")
    else:
        L.check(lib.wae_upsample_stage_bwd_list(*args, None), "upsample_stage_bwd_list")
    torch.cuda.synchronize()
    return din.cpu(), dw.cpu(), ntiles


def _exact_up(tins, s, C, seed):
    rng = np.random.RandomState(seed)
    op = _up_operands(rng, tins, s, C, _ints)
    ref = RL.upsample_list_grads(op["ins"], op["w"], op["douts"], s)
    A = RL.upsample_list_grads([x.abs() for x in op["ins"]], op["w"].abs(), [d.abs() for d in op["douts"]], s)
    top = max(float((op["pre"].abs().double() + A[1]).max()), max(float(a.max()) for a in A[0]))
    assert top < EXACT_LIMIT, f"sum of |terms| {top} leaves exact fp32 arithmetic"
    din, dw, ntiles = _call_up(op, det=True)
    din0, dw0, _ = _call_up(op, det=False)
    want_dw = (op["pre"].double() + ref[1]).float()
    assert torch.equal(dw, want_dw), (dw, want_dw)
    keep = torch.ones(op["in_pitch"], dtype=torch.bool)
    for i, (r, o) in enumerate(zip(ref[0], op["in_off"])):
        T = r.shape[1]
        keep[int(o):int(o) + T] = False
        assert torch.equal(din[:, int(o):int(o) + T], r.float()), f"din of item {i} (Tin {T})"
    assert bool((din[:, keep] == SENT).all()), "a column outside every item was written"
    assert torch.equal(dw, dw0) and torch.equal(din, din0), "the default entry's bits"
    return ntiles


@pytest.mark.parametrize("s,C", UP_CASES, ids=lambda v: str(v))
def test_upsample_stage_bwd_list_det_exact(s, C):
    _exact_up(UP_TINS, s, C, 6000 + 17 * s + C)


def test_upsample_stage_bwd_list_det_exact_when_workgroups_walk_several_tiles():
    """one item of Tin = 38 500 at s = 4, C = 3: 602 tiles for 512 workgroups"""
    assert _exact_up([38500], 4, 3, 6100) == 602 > 512


def test_upsample_stage_bwd_list_det_repeats_and_din_ignores_the_table_order():
    rng = np.random.RandomState(83)
    op = _up_operands(rng, UP_TINS + [700], 16, 16, _gauss)
    din, dw, _ = _call_up(op, det=True)
    din1, dw1, _ = _call_up(op, det=True)
    assert torch.equal(din, din1) and torch.equal(dw, dw1)
    din2, dw2, _ = _call_up(op, det=True, order=rng.permutation(len(op["Tin"])))
    assert torch.equal(din, din2)
    # (another table order hands a workgroup other tiles: dw within the bound of an fp32 sum in any order)
    ref = RL.upsample_list_grads(op["ins"], op["w"], op["douts"], 16)[1]
    A = RL.upsample_list_grads([x.abs() for x in op["ins"]], op["w"].abs(), [d.abs() for d in op["douts"]], 16)[1]
    bound = (16 * int(op["Tout"].sum()) + 5.0) * U * (op["pre"].abs().double() + A)
    for got in (dw, dw2):
        assert bool(((got.double() - (op["pre"].double() + ref)).abs() <= bound).all())


# ---------------------------------------------------------------- 8. deterministic windows
STATE = ("grads", "params", "exp_avg", "exp_avg_sq", "shadow", "grad_norm")


def _det_engine(cfg, sd, dtype, dropout=0.0):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype, dropout=dropout, drop_seed=0xD0D0)
    eng.load_state_dict(sd)
    return eng


def _snapshot(eng, res):
    torch.cuda.synchronize()
    out = {k: getattr(eng, k).clone() for k in STATE}
    out.update({"res:" + k: v.clone() if torch.is_tensor(v) else torch.tensor(v) for k, v in res.items()})
    return out


@pytest.mark.parametrize("dropout", [0.0, 0.05], ids=["plain", "dropout"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_deterministic_window_repeats_bitwise(dtype, dropout, monkeypatch):
    """train_step_list_accum on the 2 + 2 split, two engines, then once more on the updated weights"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd = golden_model("A")[:2]
    groups = _groups(_items(cfg), SPLITS["2+2"])
    engs = [_det_engine(cfg, sd, dtype, dropout) for _ in range(2)]
    assert all(e.opt.deterministic for e in engs)
    for step in range(2):
        a, b = [_snapshot(e, e.train_step_list_accum(groups, lr=LR)) for e in engs]
        assert a.keys() == b.keys() and {"res:ce", "res:vq_loss", "res:loss", "res:grad_norm"} <= a.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (f"{dtype} dropout {dropout} step {step}: {k} differs in {int((a[k] != b[k]).sum())} of "
                                             f"{a[k].numel()} elements")
            assert bool(torch.isfinite(a[k].double()).all()), k
        assert float(a["grads"].abs().max()) > 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_deterministic_window_equals_the_default_window(dtype, monkeypatch):
    ref = _window(dtype, "2+2")
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd = golden_model("A")[:2]
    eng = _engine(cfg, sd, dtype)
    assert eng.opt.deterministic
    groups = _groups(_items(cfg), SPLITS["2+2"])
    got = _step(eng, lambda e, hook: e.train_step_list_accum(groups, lr=LR, grad_hook=hook))
    _close(got, ref, dtype, "deterministic")


_DIGEST = """
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_train_list_accum as T
print("digest", T.digest_after_two_windows())
"""


def digest_after_two_windows():
    """model A, bf16, two ragged windows of 2 + 2 -> sha256 over the gradients, the updated state, the norm and the losses"""
    cfg, sd = golden_model("A")[:2]
    groups = _groups(_items(cfg), SPLITS["2+2"])
    eng = _det_engine(cfg, sd, "bf16")
    for _ in range(2):
        res = eng.train_step_list_accum(groups, lr=LR)
    h = hashlib.sha256()
    for t in list(_snapshot(eng, res).values()):
        h.update(t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_a_fresh_process_gives_the_same_bits(monkeypatch):
    """the same two windows in this process and in ONE fresh child process"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    here = os.path.dirname(os.path.abspath(__file__))
    torch.empty(3 << 20, device="cuda")            # (this process's allocator is not in a fresh state)
    mine = digest_after_two_windows()
    p = subprocess.run([sys.executable, "-c", _DIGEST.format(tests=here, root=os.path.dirname(here))], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert p.returncode == 0, p.stderr[-2000:]
    theirs = [l.split()[1] for l in p.stdout.splitlines() if l.startswith("digest ")]
    assert theirs == [mine]
