"""The hand-over between a train-mode forward and its backward (engine.saved, engine.flight): only a train-mode forward
replaces what backward reads, a backward without its forward is refused before any launch, and an abandoned step leaves nothing behind.

Geometry: golden model B (6 layers, ConvInUpsampleNetwork with scales 4,4,4,5), the one model of tests/test_gpu_modules.py whose hop
(320) allows T = one 256-step tile plus a partial one; B = 2, fp32."""
import pytest
import torch

from helpers import golden_model
from oracle import wae_oracle as O
from test_gpu_modules import _build

pytestmark = pytest.mark.gpu

B, F, T = 2, 4, 320          # 4 feature frames -> 1 latent frame -> 320 samples


def _inputs(cfg):
    c = O.hash_fill((B, cfg["c_in"], F), 21, 1.7).cuda()
    lat = O.hash_fill((B, cfg["Cc"], 1), 22, 1.2).cuda()
    x = ((O.hash_fill((B, T), 23) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1).cuda()
    g = torch.tensor([1, 3]).cuda()
    start = torch.zeros(B, 1, cfg["O"], device="cuda")
    start[:, :, cfg["O"] // 2 - 1] = 1
    return c, lat, x, g, start


def _models(which):
    cfg, sd, _, _, _ = golden_model("B")
    model, wn = _build(cfg)
    c, lat, x, g, start = _inputs(cfg)
    if which == "vqvae":            # _VQVAEFn: encoder -> VQ -> upsampling network -> decoder
        model.load_state_dict(sd)
        model = model.cuda()
        fwd = lambda cc: (lambda y, vq, perp: y.square().mean() + vq)(*model(x, cc, g, False))  # noqa: E731
        stream = lambda cc: model.incremental_stream(start, cc, g, T, True, True, None, -7.0, chunk=8)  # noqa: E731
        return model, fwd, stream, c
    wn.load_state_dict({k[len("wavenet."):]: v for k, v in sd.items() if k.startswith("wavenet.")})      # _DecoderFn, upsampling network
    wn = wn.cuda()
    fwd = lambda cc: wn(x, c=cc, g=g).square().mean()  # noqa: E731
    stream = lambda cc: wn.incremental_stream(start, c=cc, g=g, T=T, softmax=True, quantize=True, chunk=8)  # noqa: E731
    return wn, fwd, stream, lat


@pytest.mark.parametrize("which", ["vqvae", "decoder"])
def test_a_later_eval_forward_or_decode_does_not_change_the_gradients(which):
    """Run 1: train-mode forward, backward -> G1.  Run 2: train-mode forward, a no_grad forward and a decode of 8 steps on
    c' = 10 c + 1, then backward -> G2.  Run 3: run 1 again -> G3.  If G3 is bitwise G1 so must G2 be; otherwise
    max|G2 - G1| <= 1e-4 max|G1| per tensor (fp32 reordering noise of these sums is of order 1e-6 relative; activations scaled by ten
    move the upsampling and encoder gradients by order one).
    The decode: the upsampling network maps whole latent frames, so a decode through it spans all T = 320 steps; its first 8 steps are
    the first chunk of incremental_stream, which opens as incremental_forward does (the whole c' through the upsampling network)."""
    model, fwd, stream, c = _models(which)
    c2 = 10 * c + 1

    def disturb():
        with torch.no_grad():
            fwd(c2)
        model.eval()
        chunks = stream(c2)
        assert next(chunks).shape[-1] == 8
        chunks.close()
        model.train()

    def run(between=None):
        model.train().zero_grad(set_to_none=True)
        loss = fwd(c)
        if between is not None:
            between()
        loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    g1, g2, g3 = run(), run(disturb), run()
    assert len(g1) == len(list(model.parameters())) and g1.keys() == g2.keys() == g3.keys()
    bitwise = all(torch.equal(g1[n], g3[n]) for n in g1)
    worst = {n: (float((g2[n] - g1[n]).abs().max()), float(g1[n].abs().max())) for n in g1}
    off = {n: v for n, v in worst.items() if v[0] > 0}
    print(f"{which}: repeat bitwise {bitwise}; {len(off)} of {len(g1)} tensors differ; largest (diff, max|G1|):",
          sorted(off.items(), key=lambda kv: -kv[1][0] / max(kv[1][1], 1e-30))[:4])
    if bitwise:
        assert not off, off
    bad = {n: v for n, v in worst.items() if v[0] > 1e-4 * v[1]}
    assert not bad, bad


def _engine(cfg, sd):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    eng.init_optimizer()
    return eng


def _same_step(res, ref_res):
    """every entry of train_step's result (loss, ce, vq_loss, perp, grad_norm), bit for bit"""
    torch.cuda.synchronize()
    got, want = {k: float(v) for k, v in res.items()}, {k: float(v) for k, v in ref_res.items()}
    print("step:", got, "clean engine:", want)
    assert got == want


def test_backward_without_its_forward_is_refused():
    """engine.backward on a fresh engine, and after a train-mode forward of another (B, T): RuntimeError before any launch; the engine
    then runs a correct train_step -- the loss (and the rest of the result) of a second engine that saw only that step, bit for bit."""
    cfg, sd, _, _, _ = golden_model("B")
    c, _, x, g, _ = _inputs(cfg)
    eng = _engine(cfg, sd)
    assert eng.saved is None
    with pytest.raises(RuntimeError, match="no train-mode forward to differentiate"):
        eng.backward(x, g, x, None)
    eng.forward(x, c, g, targets=x, want_logits=False)                  # an eval forward saves nothing
    assert eng.saved is None
    with pytest.raises(RuntimeError, match="no train-mode forward to differentiate"):
        eng.backward(x, g, x, None)
    c_long = O.hash_fill((B, cfg["c_in"], 2 * F), 24, 1.7).cuda()
    x_long = torch.cat([x, x], dim=1)
    eng.forward(x_long, c_long, g, targets=x_long, want_logits=False, train=True)
    assert (eng.saved.B, eng.saved.T) == (B, 2 * T)
    with pytest.raises(RuntimeError, match=rf"\({B}, {T}\).*\({B}, {2 * T}\)"):
        eng.backward(x, g, x, None)
    res = eng.train_step(x, c, g)
    ref = _engine(cfg, sd)
    _same_step(res, ref.train_step(x, c, g))
    eng.check_errors()


def test_an_abandoned_step_leaves_nothing_behind():
    """A train_step refused half-way (conditioning that does not upsample to T: raised inside the forward, after the side-stream packing
    was queued) is followed by a good one whose result is a clean engine's, bit for bit.  Then the out-of-range id: the kernels clamp
    it and flag it, check_errors() refuses the step afterwards (its update has happened); the next good step equals that of an engine
    that starts clean from the state the refused step left."""
    cfg, sd, _, _, _ = golden_model("B")
    c, _, x, g, _ = _inputs(cfg)
    eng = _engine(cfg, sd)
    with pytest.raises(Exception, match="upsamples to"):
        eng.train_step(x, O.hash_fill((B, cfg["c_in"], 2 * F), 24, 1.7).cuda(), g)
    assert eng.flight.pack_done is None and eng.flight.early_pack is None and eng.saved is None
    res = eng.train_step(x, c, g)
    ref = _engine(cfg, sd)
    _same_step(res, ref.train_step(x, c, g))
    x_bad = x.clone()
    x_bad[0, 17] = cfg["O"] + 5
    eng.train_step(x_bad, c, g)
    with pytest.raises(IndexError, match="class id"):
        eng.check_errors()
    ref = _engine(cfg, eng.state_dict())
    for name in ("exp_avg", "exp_avg_sq", "shadow"):
        getattr(ref, name).copy_(getattr(eng, name))
    ref.opt_step = eng.opt_step
    _same_step(eng.train_step(x, c, g), ref.train_step(x, c, g))
    eng.check_errors()
