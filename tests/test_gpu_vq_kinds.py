"""The sliced and EMA quantisers inside the engine (Geometry.vq), on golden model A's geometry in fp32 unless said: forward and one
train step per kind against the oracle's composition encoder -> quantiser -> decoder (float64 autograd for the step), the EMA
kinds' carried state over two steps and an eval forward, the VQVAE module and a checkpoint round trip, the deterministic mode, and
the refusals before any launch."""
import pytest
import torch

import vq_cases as V
from helpers import rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL, BF16_TOL = 1e-3, 5e-2          # tests/test_gpu_parity.py
KINDS = sorted(V.KINDS)
LR = 4e-4


def _engine(cfg, sd, dtype="fp32"):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd)
    return eng


def _rows(idx):
    return list(idx) if idx.dim() == 2 else [idx]


@pytest.mark.parametrize("dtype,tol", [("fp32", FP32_TOL), ("bf16", BF16_TOL)])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_against_the_oracle(kind, dtype, tol):
    cfg, sd, ins, ocfg = V.model_case(V.KINDS[kind])
    with torch.no_grad():
        y_ref, vq_ref, perp_ref, aux = V.oracle_forward(cfg, sd, ocfg, ins["xin"], ins["c"], ins["g"])
    eng = _engine(cfg, sd, dtype)
    out = eng.forward(ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda(), targets=ins["x"].cuda())
    torch.cuda.synchronize()
    n = len(V.slice_specs(cfg))
    assert tuple(out["idx"].shape) == ((n, aux["idx"][0].numel()) if n > 1 else (aux["idx"][0].numel(),))
    for got, want in zip(_rows(out["idx"]), aux["idx"]):
        assert torch.equal(got.cpu(), want)
    assert rel_err(out["latents"].cpu(), aux["latents"]) < FP32_TOL            # encoder and quantiser are always fp32
    assert rel_err(out["quant"].cpu(), aux["quant"]) < 1e-5
    assert abs(float(out["vq_loss"]) - float(vq_ref)) < 1e-5 and abs(float(out["perp"]) - float(perp_ref)) < 1e-3
    assert rel_err(out["logits"].cpu(), y_ref) < tol
    # an eval forward of an EMA kind moves nothing
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in eng.state_dict().items())


def _oracle_step(cfg, sd64, ocfg, ins, opt, training=True):
    """one float64 train step through the oracle's composition: -> (numbers, grads, the state after clip + Adam + EMA shadow);
    opt: dict(m, v, shadow, step) carried between steps"""
    keys = [k for k in sd64 if not V.is_buffer(k)]
    p = {k: (sd64[k].clone().requires_grad_(True) if k in keys else sd64[k].clone()) for k in sd64}
    x, T = ins["x"], ins["x"].shape[1]
    y, vq, perp, aux = V.oracle_forward(cfg, p, ocfg, ins["xin"].double(), ins["c"].double(), ins["g"], training=training)
    ce = O.masked_ce_loss(y, x.unsqueeze(-1), torch.full((x.shape[0],), T))
    (ce + vq).backward()
    grads = {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])).detach() for k in keys}
    new = {k: v.detach().clone() for k, v in p.items()}
    if aux["state"] is not None:
        new.update({k: v.detach().clone() for k, v in aux["state"].items()})        # the moved codebooks and their statistics
    params = {k: new[k] for k in keys}
    opt["step"] += 1
    gn = O.clip_adam_ema_step(params, grads, opt["m"], opt["v"], opt["shadow"], opt["step"], LR, clip_thresh=100.0, ema_decay=0.9999)
    new.update(params)
    return dict(loss=float(ce + vq), vq_loss=float(vq), perp=float(perp), grad_norm=float(gn), idx=aux["idx"]), grads, new


def _opt_state(sd64):
    keys = [k for k in sd64 if not V.is_buffer(k)]
    return dict(m={k: torch.zeros_like(sd64[k]) for k in keys}, v={k: torch.zeros_like(sd64[k]) for k in keys},
                shadow={k: sd64[k].clone() for k in keys}, step=0)


def _arena(eng, arena, key):
    lay = eng.lay
    return arena[lay.off(key):lay.off(key) + lay.numel(key)].view(lay.shapes[key]).cpu()


@pytest.mark.parametrize("kind", KINDS)
def test_train_step_against_float64_autograd(kind):
    """the tolerances of tests/test_gpu_backward.py::test_full_train_step_against_golden"""
    cfg, sd, ins, ocfg = V.model_case(V.KINDS[kind])
    sd64 = {k: v.double() for k, v in sd.items()}
    opt = _opt_state(sd64)
    ref, grads, new = _oracle_step(cfg, sd64, ocfg, ins, opt)
    eng = _engine(cfg, sd)
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    res = eng.train_step(x, c, g, lengths=torch.tensor([T, T]), lr=LR, clip_thresh=100.0, ema_decay=0.9999)
    torch.cuda.synchronize()
    for got, want in zip(_rows(eng.saved.idx), ref["idx"]):
        assert torch.equal(got.cpu(), want)
    assert abs(float(res["loss"]) - ref["loss"]) < 1e-4
    assert abs(float(res["vq_loss"]) - ref["vq_loss"]) < 1e-5
    assert abs(float(res["grad_norm"]) - ref["grad_norm"]) < 1e-3 * ref["grad_norm"]
    ema_kind = cfg["vq"] in ("ema", "sliced_ema")
    for key in grads:
        if key.startswith("vq.embedding"):
            assert (float(grads[key].abs().max()) == 0.0) == ema_kind, key
        if float(grads[key].abs().max()) == 0.0:      # the top layer's residual output feeds nothing; an EMA codebook has no gradient
            assert float(_arena(eng, eng.grads, key).abs().max()) == 0.0, key
        else:
            assert rel_err(_arena(eng, eng.grads, key), grads[key]) < 2e-3, key
        assert rel_err(_arena(eng, eng.params, key), new[key]) < 5e-5, key
        assert rel_err(_arena(eng, eng.shadow, key), opt["shadow"][key]) < 1e-6, key
    got = eng.state_dict()
    for key in (k for k in sd if V.is_buffer(k)):
        assert rel_err(got[key].cpu(), new[key]) < 1e-5, key


@pytest.mark.parametrize("kind", ["ema", "sliced_ema"])
def test_ema_state_over_two_steps_and_an_eval_forward(kind):
    """codebooks, ema_cluster_size* and ema_w* against the oracle's carried state, at the tolerance of
    tests/test_gpu_modules.py::test_ema_quantizers_against_reference_vectors; forwards that must not update change no bit"""
    cfg, sd, ins, ocfg = V.model_case(V.KINDS[kind])
    sd64 = {k: v.double() for k, v in sd.items()}
    opt = _opt_state(sd64)
    eng = _engine(cfg, sd)
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    with pytest.raises(NotImplementedError, match="weight_decay"):
        eng.train_step(x, c, g, lengths=torch.tensor([T, T]), lr=LR, weight_decay=1e-4)
    assert eng.opt_step == 0 and eng.saved is None
    vq_keys = [k for k in sd if k.startswith("vq.")]
    for step in range(2):
        ref, _, sd64 = _oracle_step(cfg, sd64, ocfg, ins, opt)
        eng.train_step(x, c, g, lengths=torch.tensor([T, T]), lr=LR, clip_thresh=100.0, ema_decay=0.9999)
        got = eng.state_dict()
        for got_i, want in zip(_rows(eng.saved.idx), ref["idx"]):
            assert torch.equal(got_i.cpu(), want), step
        for key in vq_keys:
            assert rel_err(got[key].cpu(), sd64[key]) < 1e-5, (step, key)
    before = {k: v.clone() for k, v in eng.state_dict().items()}
    with torch.no_grad():
        y_ref, vq_ref, _, aux = V.oracle_forward(cfg, sd64, ocfg, ins["xin"].double(), ins["c"].double(), ins["g"])
    out = eng.forward(x, c, g, targets=x)
    for got_i, want in zip(_rows(out["idx"]), aux["idx"]):
        assert torch.equal(got_i.cpu(), want)
    assert rel_err(out["quant"].cpu(), aux["quant"]) < 1e-5 and abs(float(out["vq_loss"]) - float(vq_ref)) < 1e-5
    assert rel_err(out["logits"].cpu(), y_ref) < FP32_TOL
    eng.forward(x, c, g, targets=x, train=True, vq_update=False)
    torch.cuda.synchronize()
    after = eng.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    eng.forward(x, c, g, targets=x, train=False, vq_update=True)               # the reference updates on self.training, whatever the grad mode
    assert not torch.equal(eng.state_dict()[vq_keys[0]], before[vq_keys[0]])


def _module(cfg):
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    wn = WaveNet(out_channels=cfg["O"], layers=cfg["layers"], stacks=cfg["stacks"], residual_channels=cfg["R"],
                 gate_channels=cfg["G"], skip_out_channels=cfg["S"], kernel_size=cfg["k"], dropout=0.0, cin_channels=cfg["Cc"],
                 gin_channels=cfg["Cg"], n_speakers=cfg["n_speakers"], upsample_conditional_features=True,
                 upsample_params=dict(upsample_scales=cfg["upsample_scales"]), use_speaker_embedding=True)
    return VQVAE(c_in=cfg["c_in"], hid=cfg["Cc"], K=cfg["K"], wavenet=wn, encoder_hid=cfg["encoder_hid"], quantizer=cfg["vq"],
                 num_slices=cfg.get("vq_slices", 2), K1=cfg.get("K1"), beta=V.BETA, decay=cfg.get("vq_decay", 0.99))


@pytest.mark.parametrize("kind", KINDS)
def test_module_autograd_and_checkpoint_round_trip(kind, tmp_path):
    from wavenet_autoencoders_amd.checkpoint import load_checkpoint, save_checkpoint
    from wavenet_autoencoders_amd.hparams import hparams
    cfg, sd, ins, ocfg = V.model_case(V.KINDS[kind])
    model = _module(cfg)
    assert set(model.state_dict()) == set(sd)                                  # the reference's names (vq_cases.model_case)
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert {k for k, _ in model.named_buffers()} == {k for k in sd if V.is_buffer(k)}
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    y, vq, perp = model(ins["xin"].cuda(), c, g, False)
    ce = torch.nn.functional.cross_entropy(y[:, :, :-1], x[:, 1:], reduction="mean")
    (ce + vq).backward()
    # the engine's own backward of the same step, on a second engine
    eng = _engine(cfg, sd)
    eng.forward(x, c, g, targets=x, lengths=torch.tensor([T, T]), train=True, want_logits=False)
    grads = eng.backward(x, g, x, torch.tensor([T, T])).clone()
    torch.cuda.synchronize()
    for key, p in model.named_parameters():
        want = _arena(eng, grads, key)
        assert p.grad is not None and (float((p.grad.cpu() - want).abs().max()) <= 2e-3 * float(want.abs().max()) + 1e-12), key
    after = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    if cfg["vq"] in ("ema", "sliced_ema"):                                     # a training-mode forward moved codebooks and statistics alike
        assert all(not torch.equal(after[k], sd[k]) for k in sd if k.startswith("vq."))
        assert all(torch.equal(after[k], v.cpu()) for k, v in eng.state_dict().items() if k.startswith("vq."))
    # checkpoint round trip, plain and _ema twin: parameters and buffers come back bit for bit
    eng.init_optimizer()
    eng.shadow.mul_(0.5)
    save_checkpoint(eng, 3, 0, str(tmp_path), hparams)
    want = eng.state_dict()
    for name, scale in (("checkpoint_latest.pth", 1.0), ("checkpoint_latest_ema.pth", 0.5)):
        saved = torch.load(tmp_path / name, map_location="cpu")["state_dict"]
        assert set(saved) == set(sd)
        e2 = _engine(cfg, {k: torch.zeros_like(v) for k, v in sd.items()})
        load_checkpoint(str(tmp_path / name), e2, reset_optimizer=True)
        got = e2.state_dict()
        for k in want:
            assert torch.equal(got[k], want[k] if V.is_buffer(k) else want[k] * scale), (name, k)


@pytest.mark.parametrize("kind", KINDS)
def test_deterministic_mode_repeats_bitwise(kind, monkeypatch):
    """tests/test_gpu_deterministic.py's pattern: two fresh engines, the same inputs, every bit of two steps"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, ins, _ = V.model_case(V.KINDS[kind])
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    engs = [_engine(cfg, sd) for _ in range(2)]
    assert all(e.opt.deterministic for e in engs)
    for step in range(2):
        snaps = []
        for e in engs:
            res = e.train_step(x, c, g, lengths=torch.tensor([T, T - 137]), lr=2e-3)
            torch.cuda.synchronize()
            snap = {k: getattr(e, k).clone() for k in ("grads", "params", "exp_avg", "exp_avg_sq", "shadow", "grad_norm")}
            snap.update({"res:" + k: v.clone() for k, v in res.items()})
            snap.update({"sd:" + k: v for k, v in e.state_dict().items() if V.is_buffer(k)})
            snaps.append(snap)
        assert snaps[0].keys() == snaps[1].keys()
        for k in snaps[0]:
            assert torch.equal(snaps[0][k], snaps[1][k]), (kind, step, k)
            assert bool(torch.isfinite(snaps[0][k].double()).all()), (kind, step, k)


@pytest.mark.parametrize("kind", KINDS)
def test_refusals_come_before_any_launch(kind):
    cfg, sd, ins, _ = V.model_case(V.KINDS[kind])
    eng = _engine(cfg, sd)
    eng.prepare_weights()
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    class Sync:                      # a grad_sync is refused before anything of it is touched
        world = 2

    real, eng.lib = eng.lib, Counting(eng.lib)
    try:
        with pytest.raises(NotImplementedError, match="accumulation"):
            eng.accumulate(x, c, g)
        with pytest.raises(NotImplementedError, match="accumulation"):
            eng.train_step_accum([(x, c, g, None)])
        if cfg["vq"] in ("ema", "sliced_ema"):
            with pytest.raises(NotImplementedError, match="grad_sync"):
                eng.train_step(x, c, g, grad_sync=Sync())
            with pytest.raises(NotImplementedError, match="weight_decay"):
                eng.train_step(x, c, g, weight_decay=0.01)
    finally:
        eng.lib = real
    assert calls == [] and eng.window is None and eng.saved is None
