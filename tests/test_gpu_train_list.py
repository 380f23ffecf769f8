"""WaeEngine.train_step_list: one optimisation step on a list of unequal-length utterances -- the list front end (packed, unpadded)
in front of the dense right-padded decoder, the list forms of the front end's backward behind it.

The function it differentiates is  sum_i nll_sum_i / sum_i (T_i - 1) + sum_i (Tq_i / sum Tq) vq_i  with every utterance a batch of
one: the checker is autograd through the oracle of exactly that, on golden model A with utterances of 8, 12, 4 and 36
feature frames.  The bounds are those of tests/test_gpu_accum.py case 4 (rel_err < 2e-3 per gradient tensor, ce within 1e-4, vq_loss
within 1e-5).  train_step on the same utterances zero-padded differentiates another function (the pad frames' latents enter the
commitment mean and the conditioning of every utterance's end): it must MISS encoder.lin.weight by more than 0.1 (the oracle: 0.47).
"""
import numpy as np
import pytest
import torch

from helpers import golden_model, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
LR = 1e-3
FRAMES = (8, 12, 4, 36)


def _engine(cfg, sd, dtype, **kw):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype, **kw)
    eng.load_state_dict(sd)
    eng.init_optimizer()
    return eng


def _items(cfg, frames=FRAMES, seed=5, speakers=None):
    """host items of the given feature frames: x (160 F,), c (c_in, F), gid"""
    torch.manual_seed(seed)
    out = []
    for i, F in enumerate(frames):
        x = torch.randint(0, cfg["O"], (160 * F,))
        c = torch.randn(cfg["c_in"], F)
        out.append(dict(x=x, c=c, gid=i if speakers is None else speakers[i]))
    return out


def _padded(items, cfg):
    B, Tm, Fm = len(items), max(it["x"].shape[0] for it in items), max(it["c"].shape[1] for it in items)
    x, c = torch.zeros(B, Tm, dtype=torch.long), torch.zeros(B, cfg["c_in"], Fm)
    for b, it in enumerate(items):
        x[b, :it["x"].shape[0]] = it["x"]
        c[b, :, :it["c"].shape[1]] = it["c"]
    return x.cuda(), c.cuda(), torch.tensor([it["gid"] for it in items]).cuda(), torch.tensor([it["x"].shape[0] for it in items])


def _numbers(res):
    return {k: float(v) for k, v in res.items() if k in ("loss", "ce", "vq_loss", "perp", "grad_norm")}


def _list_step(cfg, sd, dtype, items, **kw):
    eng = _engine(cfg, sd, dtype)
    seen = {}
    res = eng.train_step_list(items, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()), **kw)
    torch.cuda.synchronize()
    eng.check_errors()
    return eng, res, seen["g"].cpu()


_ORACLE = {}


def _oracle(items):
    """autograd through the oracle, every utterance a batch of one -> (grads by name, ce, vq_loss); computed once"""
    if "A" not in _ORACLE:
        cfg, sd, _, _, ocfg = golden_model("A")
        psd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        nll, n, vqs, tqs = 0.0, 0, [], []
        for it in items:
            T = it["x"].shape[0]
            xin = torch.nn.functional.one_hot(it["x"][None], cfg["O"]).float().transpose(1, 2).contiguous()
            y, vq, _, aux = O.vqvae_forward(psd, ocfg, xin, it["c"][None], torch.tensor([it["gid"]]))
            nll = nll + O.masked_ce_loss(y, it["x"][None].unsqueeze(-1), torch.tensor([T])) * (T - 1)
            n += T - 1
            vqs.append(vq)
            tqs.append(T // 640)
        ce = nll / n
        vq = sum(v * (t / sum(tqs)) for v, t in zip(vqs, tqs))
        (ce + vq).backward()
        _ORACLE["A"] = ({k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in psd.items()}, float(ce.detach()),
                        float(vq.detach()))
    return _ORACLE["A"]


def _per_tensor(lay, grads, ref):
    return {k: (rel_err(grads[lay.off(k):lay.off(k) + lay.numel(k)].view(lay.shapes[k]), r) if float(r.abs().max()) > 0
                else float(grads[lay.off(k):lay.off(k) + lay.numel(k)].abs().max())) for k, r in ref.items()}


def test_list_step_against_autograd_through_the_oracle():
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    assert [it["x"].shape[0] for it in items] == [1280, 1920, 640, 5760]
    ref, ce_o, vq_o = _oracle(items)
    eng, res, grads = _list_step(cfg, sd, "fp32", items)
    print(f"ce {float(res['ce'])} (oracle {ce_o}), vq_loss {float(res['vq_loss'])} (oracle {vq_o}), rows {res['rows']}, pad {res['pad_rows']}")
    assert res["rows"] == 4 * 5760 and res["pad_rows"] == 4 * 5760 - 9600
    assert abs(float(res["ce"]) - ce_o) < 1e-4 and abs(float(res["vq_loss"]) - vq_o) < 1e-5
    errs = _per_tensor(eng.lay, grads, ref)
    print({k: f"{e:.2e}" for k, e in errs.items() if e > 2e-4})
    bad = {k: e for k, e in errs.items() if not e < 2e-3}
    assert not bad, bad


def test_padded_step_is_another_function():
    """train_step on the zero-padded batch against the same oracle: encoder.lin.weight off by more than 0.1"""
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    ref = _oracle(items)[0]
    eng = _engine(cfg, sd, "fp32")
    seen = {}
    x, c, g, lengths = _padded(items, cfg)
    res = eng.train_step(x, c, g, lengths=lengths, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    errs = _per_tensor(eng.lay, seen["g"].cpu(), ref)
    print(f"padded: vq_loss {float(res['vq_loss'])}, encoder.lin.weight {errs['encoder.lin.weight']:.3f}, "
          f"vq.embedding.weight {errs['vq.embedding.weight']:.3f}")
    assert errs["encoder.lin.weight"] > 0.1


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_list_step_against_the_fp32_list_step(dtype):
    """the bounds the 16-bit dense steps are held to against fp32 (tests/test_gpu_backward.py: the whole gradient within 5e-2 in norm;
    tests/test_gpu_fp16.py: ce within 5e-3, grad_norm within 5e-2, both relative)"""
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    _, r32, g32 = _list_step(cfg, sd, "fp32", items)
    _, r16, g16 = _list_step(cfg, sd, dtype, items)
    rel = float((g16 - g32).double().norm() / g32.double().norm())
    n16, n32 = _numbers(r16), _numbers(r32)
    print(f"{dtype}: gradient {rel:.3e}, {n16} vs {n32}")
    assert rel < 5e-2
    assert abs(n16["ce"] - n32["ce"]) < 5e-3 * n32["ce"] and abs(n16["grad_norm"] - n32["grad_norm"]) < 5e-2 * n32["grad_norm"]
    assert abs(n16["vq_loss"] - n32["vq_loss"]) < 1e-5 and n16["perp"] == n32["perp"]          # the front end's forward is fp32 in both


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_equal_lengths_equal_the_dense_step(dtype):
    """three items of one length: no pad, the same function as train_step on the dense batch -- tests/test_gpu_accum.py's _tol"""
    tol = dict(g=2e-5, p=1e-5, l=1e-5) if dtype == "fp32" else dict(g=2e-3, p=2e-3, l=2e-3)
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg, frames=(12, 12, 12), seed=9, speakers=(2, 0, 4))
    eng, res, g0 = _list_step(cfg, sd, dtype, items)
    assert res["pad_rows"] == 0
    p0 = eng.params.cpu().clone()
    ref = _engine(cfg, sd, dtype)
    seen = {}
    x, c, g, lengths = _padded(items, cfg)
    r1 = ref.train_step(x, c, g, lengths=lengths, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    g1, p1, n0, n1 = seen["g"].cpu(), ref.params.cpu(), _numbers(res), _numbers(r1)
    gerr, gmax, perr = float((g0 - g1).abs().max()), float(g1.abs().max()), float((p0 - p1).abs().max())
    print(f"{dtype}: grad err {gerr:.3e} of {gmax:.3e}, param err {perr:.3e}, {n0} vs {n1}")
    assert gerr <= tol["g"] * gmax and perr < tol["p"]
    assert all(abs(n0[k] - n1[k]) < tol["l"] for k in ("loss", "ce", "vq_loss"))
    assert abs(n0["perp"] - n1["perp"]) <= 1e-6 * n1["perp"]


def test_reported_numbers_are_score_lists():
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    eng = _engine(cfg, sd, "fp32")
    _, tot = eng.score_list([dict(it, feats=it["c"]) for it in items])
    tot = {k: float(v) for k, v in tot.items()}
    res = eng.train_step_list(items, lr=LR)
    n = _numbers(res)
    print(n, tot)
    assert n["perp"] == tot["perp"]
    assert abs(n["vq_loss"] - tot["vq_loss"]) <= 1e-6 * tot["vq_loss"]
    assert abs(n["ce"] - tot["ce"]) < 1e-5


def _state(eng):
    return dict(params=eng.params.clone(), exp_avg=eng.exp_avg.clone(), exp_avg_sq=eng.exp_avg_sq.clone(), shadow=eng.shadow.clone(),
                opt_step=eng.opt_step)


def test_a_list_step_leaves_nothing_behind():
    """a list step, then train_step(X): against a fresh engine that loaded the state behind the list step and ran train_step(X)"""
    dtype = "bf16"
    tol = dict(g=2e-3, p=2e-3, l=2e-3)
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    X = _padded(_items(cfg, frames=(36, 36), seed=23, speakers=(1, 2)), cfg)        # the list step's (B 4, T 5760) workspace is not X's...
    Y = _padded(_items(cfg, frames=(36, 30, 36, 20), seed=24), cfg)                  # ... and is Y's: its conditioning rows were list-written
    eng, _, _ = _list_step(cfg, sd, dtype, items)
    assert eng.window is None and eng.opt_step == 1
    state = _state(eng)
    fresh = _engine(cfg, sd, dtype)
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow"):
        getattr(fresh, k).copy_(state[k])
    fresh.opt_step = state["opt_step"]
    fresh.weights_dirty = True
    for batch in (X, Y):
        out = []
        for e in (eng, fresh):
            seen = {}
            x, c, g, lengths = batch
            res = e.train_step(x, c, g, lengths=lengths, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
            torch.cuda.synchronize()
            out.append((_numbers(res), seen["g"].cpu(), e.params.cpu().clone()))
        (n0, g0, p0), (n1, g1, p1) = out
        gerr, gmax, perr = float((g0 - g1).abs().max()), float(g1.abs().max()), float((p0 - p1).abs().max())
        print(f"grad err {gerr:.3e} of {gmax:.3e}, param err {perr:.3e}")
        assert gerr <= tol["g"] * gmax and perr < tol["p"]
        assert all(abs(n0[k] - n1[k]) < tol["l"] for k in ("loss", "ce", "vq_loss"))


def test_refusals_come_before_any_launch():
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd = golden_model("A")[:2]
    items = _items(cfg)
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    class Sync:
        world = 1

    def refused(eng, exc, match, its=items, **kw):
        eng.prepare_weights()
        torch.cuda.synchronize()
        real, drops, saved = eng.lib, eng.drop_calls, eng.saved
        eng.lib = Counting(real)
        try:
            with pytest.raises(exc, match=match):
                eng.train_step_list(its, **kw)
        finally:
            eng.lib = real
        assert calls == [] and eng.window is None and eng.saved is saved and eng.drop_calls == drops and eng.opt_step == 0, (match, calls)

    eng = _engine(cfg, sd, "fp32", dropout=0.05)
    short = [dict(it) for it in items]
    short[2] = dict(short[2], x=short[2]["x"][:-1])
    refused(eng, ValueError, "item 2 has 639 samples", short)
    nofr = [dict(it) for it in items]
    nofr[1] = dict(nofr[1], c=nofr[1]["c"][:, :0])
    refused(eng, ValueError, "item 1", nofr)
    refused(eng, ValueError, "max_rows", max_rows=4 * 5760 - 1)
    refused(eng, ValueError, "empty", [])
    refused(eng, NotImplementedError, "grad_sync", grad_sync=Sync())
    det = _engine(cfg, sd, "fp32")
    det.opt.deterministic = True
    refused(det, NotImplementedError, "deterministic")
    for extra, match in ((dict(cin_pad=1), "cin_pad"), (dict(up_act="ReLU"), "upsample_activation")):
        g2 = Geometry.from_cfg(dict(cfg, **extra))
        e2 = WaeEngine(g2, dtype="fp32")
        e2.init_optimizer()
        refused(e2, NotImplementedError, match)
    # inside an open accumulation window: train_step's refusal
    x, c, g, lengths = _padded(_items(cfg, frames=(8, 8), seed=3), cfg)
    eng.accumulate(x, c, g, lengths, ce_weight=1.0, vq_weight=1.0)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match=r"apply_step\(\).*discard_step\(\)"):
        eng.train_step_list(items)
    assert eng.window is not None and eng.window.n == 1
    eng.discard_step()



# ---------------------------------------------------------------- the sliced and EMA quantisers
@pytest.mark.parametrize("kind", ["sliced", "sliced_ema"])
def test_quantiser_kinds_against_float64_autograd(kind):
    """the oracle composed per utterance around ONE quantiser call (training mode) on the latents concatenated along time: gradients
    at the bounds above, the codebooks and EMA statistics after the step at 1e-5 (tests/test_gpu_vq_kinds.py's bound)"""
    import vq_cases as V
    cfg, sd, _, ocfg = V.model_case(V.KINDS[kind])
    items = _items(cfg)
    sd64 = {k: v.double() for k, v in sd.items()}
    keys = [k for k in sd64 if not V.is_buffer(k)]
    p = {k: (sd64[k].clone().requires_grad_(True) if k in keys else sd64[k].clone()) for k in sd64}
    lat = torch.cat([O.encoder_forward(p, it["c"][None].double()) for it in items], dim=2)
    q, vq, perp, idx, state = V.quantise(cfg, p, lat, training=True)
    nll, n, at = 0.0, 0, 0
    for it in items:
        T = it["x"].shape[0]
        xin = torch.nn.functional.one_hot(it["x"][None], cfg["O"]).double().transpose(1, 2).contiguous()
        y = O.wavenet_forward(p, ocfg, xin, q[:, :, at:at + T // 640], torch.tensor([it["gid"]]))
        nll = nll + O.masked_ce_loss(y, it["x"][None].unsqueeze(-1), torch.tensor([T])) * (T - 1)
        n, at = n + T - 1, at + T // 640
    ce = nll / n
    (ce + vq).backward()
    grads = {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])).detach() for k in keys}
    new = {k: v.detach().clone() for k, v in p.items()}
    if state is not None:
        new.update({k: v.detach().clone() for k, v in state.items()})
    params = {k: new[k] for k in keys}
    opt = dict(m={k: torch.zeros_like(sd64[k]) for k in keys}, v={k: torch.zeros_like(sd64[k]) for k in keys},
               shadow={k: sd64[k].clone() for k in keys})
    O.clip_adam_ema_step(params, grads, opt["m"], opt["v"], opt["shadow"], 1, LR, clip_thresh=100.0, ema_decay=0.9999)
    new.update(params)
    eng, res, g = _list_step(cfg, sd, "fp32", items, clip_thresh=100.0, ema_decay=0.9999)
    print(f"{kind}: ce {float(res['ce'])} ({float(ce.detach())}), vq_loss {float(res['vq_loss'])} ({float(vq.detach())}), perp {float(res['perp'])} ({float(perp)})")
    assert abs(float(res["ce"]) - float(ce.detach())) < 1e-4 and abs(float(res["vq_loss"]) - float(vq.detach())) < 1e-5
    errs = _per_tensor(eng.lay, g, grads)
    bad = {k: e for k, e in errs.items() if not e < 2e-3}
    assert not bad, bad
    got = eng.state_dict()
    for key in (k for k in sd if k.startswith("vq.")):
        assert rel_err(got[key].cpu(), new[key]) < 1e-5, key


# ---------------------------------------------------------------- other models
def _dense_vs_list(eng_of, items, batch, dtype="fp32"):
    """a list of equal lengths against train_step on the dense batch, fp32: gradients and losses at test_gpu_accum.py's _tol.  The
    parameters behind Adam are compared where the gradient is not rounding noise: the first Adam step is lr g / (|g| + eps), so an
    element with |g| >= 1e-3 max|g| moves by lr |dg| / |g| <= lr 2e-5 / 1e-3 more or less -- the bound below -- while an element whose
    gradient is itself of the size of the fp32 sums' reordering error may move by up to 2 lr either way (model A's equal-length test
    holds every parameter to 1e-5)."""
    tol = dict(g=2e-5, p=LR * 2e-5 / 1e-3, l=1e-5)
    out = []
    for how in ("list", "dense"):
        eng, seen = eng_of(), {}
        hook = lambda gr: seen.__setitem__("g", gr.clone())      # noqa: E731
        res = eng.train_step_list(items, lr=LR, grad_hook=hook) if how == "list" else eng.train_step(*batch[:3], lengths=batch[3], lr=LR,
                                                                                                     grad_hook=hook)
        torch.cuda.synchronize()
        out.append((_numbers(res), seen["g"].cpu(), eng.params.cpu().clone(), res))
    (n0, g0, p0, r0), (n1, g1, p1, _) = out
    gerr, gmax = float((g0 - g1).abs().max()), float(g1.abs().max())
    perr = float((p0 - p1).abs()[g1.abs() >= 1e-3 * gmax].max())
    print(f"grad err {gerr:.3e} of {gmax:.3e}, param err {perr:.3e}, {n0} vs {n1}")
    assert gerr <= tol["g"] * gmax and perr < tol["p"]
    assert all(abs(n0[k] - n1[k]) < tol["l"] for k in n1 if k != "grad_norm" and k != "perp")
    return r0


def test_scalar_input_model():
    """golden_model("S") (scalar input, the mixture loss through ext_dy): its two clips as a list equal the dense step; a ragged list runs"""
    cfg, sd, ins = golden_model("S")[:3]
    x, c, g = ins["x"][:, 0, :].contiguous(), ins["c"], ins["g"]
    T = x.shape[1]
    items = [dict(x=x[b], c=c[b], gid=int(g[b])) for b in range(x.shape[0])]
    r = _dense_vs_list(lambda: _engine(cfg, sd, "fp32"), items, (x.cuda(), c.cuda(), g.cuda(), torch.tensor([T] * x.shape[0])))
    assert r["pad_rows"] == 0
    hop = T // c.shape[2]
    ragged = [items[0], dict(items[1], x=x[1][:T - 4 * hop], c=c[1][:, :c.shape[2] - 4])]
    res = _engine(cfg, sd, "fp32").train_step_list(ragged, lr=LR)
    assert res["pad_rows"] == 4 * hop and np.isfinite(float(res["loss"])) and np.isfinite(float(res["grad_norm"]))


def test_decoder_only_engine():
    """an engine without an encoder takes c (Cc, Tc_i): equal lengths equal the dense step; a ragged list equals the dense step on the
    zero-padded conditioning only in the decoder's parameters' count of rows -- it runs, and reports its pad rows"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg = {k: v for k, v in golden_model("A")[0].items() if k not in ("c_in", "encoder_hid", "K")}
    sd = O.make_state_dict(dict(cfg), salt=7, with_encoder=False)

    def eng_of():
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
        eng.load_state_dict(sd)
        eng.init_optimizer()
        return eng

    gen = torch.Generator().manual_seed(41)
    x = torch.randint(0, cfg["O"], (2, 1920), generator=gen)
    c = torch.randn(2, cfg["Cc"], 3, generator=gen)
    g = torch.tensor([1, 3])
    items = [dict(x=x[b], c=c[b], gid=int(g[b])) for b in range(2)]
    r = _dense_vs_list(eng_of, items, (x.cuda(), c.cuda(), g.cuda(), torch.tensor([1920, 1920])))
    assert r["pad_rows"] == 0 and "vq_loss" not in r
    res = eng_of().train_step_list([items[0], dict(items[1], x=x[1][:640], c=c[1][:, :1])], lr=LR)
    assert res["pad_rows"] == 1280 and np.isfinite(float(res["loss"]))


# ---------------------------------------------------------------- the training script
def test_train_script_with_train_packed(tmp_path):
    """vqwae_train.py --train-packed for two steps on a synthetic dump whose utterances are no multiple of 4 frames, under a preset
    with max_time_steps null (modelled on tests/test_gpu_accum.py::test_train_script_with_accum_steps)"""
    import json
    import os
    import subprocess
    import sys
    from test_gpu_scripts import HP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(5)
    dump = tmp_path / "dump"
    lines = []
    for u in range(3):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 41 + 4 * u
        np.save(d / "wave.npy", rng.integers(0, 256, n * 160).astype(np.int16))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    preset = json.load(open(os.path.join(root, "hps", "vqwae.json")))
    preset["max_time_steps"] = None
    (tmp_path / "preset.json").write_text(json.dumps(preset))
    hp = ",".join(kv for kv in HP.split(",") if not kv.startswith("max_time_steps=")) + ",train_eval_interval=1000"
    ck = tmp_path / "ck"
    p = subprocess.run([sys.executable, os.path.join(root, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(ck),
                        "--preset", str(tmp_path / "preset.json"), "--hparams", hp, "--max-steps", "2", "--dtype", "fp32",
                        "--train-packed"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=root), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Finished" in p.stdout and "step 1 loss" in p.stdout
    saved = torch.load(ck / "checkpoint_latest.pth", map_location="cpu")
    assert saved["global_step"] == 2
    # without the preset's null the flag is refused
    q = subprocess.run([sys.executable, os.path.join(root, "vqwae_train.py"), "--synthetic", "--checkpoint-dir", str(tmp_path / "ck2"),
                        "--hparams", HP, "--max-steps", "1", "--train-packed"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=600)
    assert q.returncode != 0 and "max_time_steps" in q.stderr
