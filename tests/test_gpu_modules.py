"""Drop-in module surface on the GPU: reference state_dict keys, forward/backward through torch autograd
with an external loss, incremental_forward, and the no-CPU-fallback rule."""
import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu


def _build(cfg):
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    wn = WaveNet(out_channels=cfg["O"], layers=cfg["layers"], stacks=cfg["stacks"], residual_channels=cfg["R"],
                 gate_channels=cfg["G"], skip_out_channels=cfg["S"], kernel_size=cfg["k"], dropout=0.0, cin_channels=cfg["Cc"],
                 gin_channels=cfg["Cg"], n_speakers=cfg["n_speakers"], upsample_conditional_features=True,
                 upsample_params=dict(upsample_scales=cfg["upsample_scales"]), use_speaker_embedding=True)
    return VQVAE(c_in=cfg["c_in"], hid=cfg["Cc"], K=cfg["K"], wavenet=wn, encoder_hid=cfg["encoder_hid"]), wn


def test_state_dict_keys_and_forward_match_reference():
    cfg, sd, ins, z, ocfg = golden_model("A")
    model, wn = _build(cfg)
    assert set(model.state_dict().keys()) == set(sd.keys())
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    with torch.no_grad():
        y, vq, perp = model(ins["xin"].cuda(), ins["c"].cuda(), ins["g"].cuda(), False)
    assert rel_err(y.cpu(), z["y_hat"]) < 1e-3
    assert abs(float(vq) - float(z["vq_loss"])) < 1e-5 and abs(float(perp) - float(z["perp"])) < 1e-3
    # the Parameters alias the engine arena; a state_dict round trip reproduces the weights bit for bit
    sd2 = {k: v.cpu() for k, v in model.state_dict().items()}
    for k in sd:
        assert torch.equal(sd2[k], sd[k]), k
    q = model.encode(ins["c"].cuda())
    assert rel_err(q.cpu(), z["quant"]) < 1e-6


def test_autograd_with_external_loss_matches_oracle():
    """The reference computes the masked CE outside the model (vqwae_train.py:758-766); so can a user of the drop-in."""
    cfg, sd, ins, zm, ocfg = golden_model("A")
    z = load_npz("train_A")
    model, _ = _build(cfg)
    model.load_state_dict(sd)
    model = model.cuda().train()
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    y, vq, perp = model(ins["xin"].cuda(), c, g, False)
    ce = torch.nn.functional.cross_entropy(y[:, :, :-1], x[:, 1:], reduction="mean")
    (ce + vq).backward()
    assert abs(float(ce + vq) - float(z["loss"])) < 1e-4
    named = dict(model.named_parameters())
    for key in [k[5:] for k in z if k.startswith("grad:")]:
        assert rel_err(named[key].grad.cpu(), z["grad:" + key]) < 2e-3, key
    # a torch optimizer updates the arena through the aliased Parameters
    opt = torch.optim.Adam(model.parameters(), lr=4e-4, eps=1e-8)
    torch.nn.utils.clip_grad_norm_(model.parameters(), 100.0)
    opt.step()
    for key in [k[4:] for k in z if k.startswith("new:")]:
        assert rel_err(named[key].data.cpu(), z["new:" + key]) < 5e-5, key
    with torch.no_grad():
        y2, _, _ = model(ins["xin"].cuda(), c, g, False)
    assert float((y2 - y).abs().max()) > 0           # the engine saw the update


def test_wavenet_incremental_forward_module():
    cfg, sd, ins, zm, ocfg = golden_model("B")
    z = load_npz("ar_B")
    _, wn = _build(cfg)
    wn.load_state_dict({k[len("wavenet."):]: v for k, v in sd.items() if k.startswith("wavenet.")})
    wn = wn.cuda()
    with pytest.raises(RuntimeError):
        wn.train().incremental_forward(None, c=None, g=None, T=4)                       # conv.py:19-20
    wn.eval()
    c_up = torch.from_numpy(z["c_up"]).cuda()
    Tar = c_up.shape[-1]
    tf = wn.incremental_forward(None, c=c_up, g=ins["g"].cuda(), T=Tar, test_inputs=ins["xin"][:, :, :Tar].cuda(),
                                softmax=False, quantize=False)
    assert rel_err(tf.cpu(), z["tf_logits"]) < 1e-3
    # the default start vector has its one at class 127 (wavenet.py:288): an IndexError with 64 classes, there and here
    with pytest.raises(IndexError):
        wn.incremental_forward(None, c=c_up, g=ins["g"].cuda(), T=Tar, softmax=True, quantize=True)
    start = torch.zeros(2, 1, cfg["O"], device="cuda")
    start[:, :, cfg["O"] // 2 - 1] = 1
    smp = wn.incremental_forward(start, c=c_up, g=ins["g"].cuda(), T=Tar, softmax=True, quantize=True)
    assert smp.shape == (2, cfg["O"], Tar) and float(smp.sum()) == 2 * Tar
    assert wn.receptive_field == O.receptive_field_size(cfg["layers"], cfg["stacks"], cfg["k"])
    wn.clear_buffer(); wn.make_generation_fast_()


def test_cpu_call_fails_loudly():
    from wavenet_autoencoders_amd._lib import WaeError
    cfg, sd, ins, zm, ocfg = golden_model("A")
    model, _ = _build(cfg)
    with pytest.raises(WaeError):
        model(ins["xin"], ins["c"], ins["g"], False)


def test_mixture_module_functions():
    from wavenet_autoencoders_amd.wavenet_vocoder.mixture import (discretized_mix_logistic_loss,
                                                                  sample_from_discretized_mix_logistic)
    z = load_npz("dmol")
    y_hat = torch.from_numpy(z["y_hat"]).cuda().requires_grad_(True)
    y = torch.from_numpy(z["y"]).cuda()
    loss = discretized_mix_logistic_loss(y_hat, y, 256, -7.0, reduce=True)
    loss.backward()
    assert abs(float(loss) - float(z["loss_sum_7"])) < 1e-3 * abs(float(z["loss_sum_7"]))
    assert rel_err(y_hat.grad.cpu(), z["grad_7"]) < 1e-3
    el = discretized_mix_logistic_loss(y_hat.detach(), y, 256, -7.0, reduce=False)
    assert el.shape == y.shape and rel_err(el.cpu(), z["loss_el_7"]) < 1e-4
    s = sample_from_discretized_mix_logistic(y_hat.detach(), -7.0)
    assert s.shape == (2, 96) and float(s.abs().max()) <= 1.0
    from wavenet_autoencoders_amd.losses import DiscretizedMixturelogisticLoss, MaskedCrossEntropyLoss
    lengths = torch.tensor([96, 80]).cuda()
    got = DiscretizedMixturelogisticLoss(256, -7.0)(y_hat.detach(), y, lengths=lengths)
    mask = O.sequence_mask(lengths.cpu(), 96).unsqueeze(-1)
    want = (torch.from_numpy(z["loss_el_7"]) * mask).sum() / mask.sum()
    assert abs(float(got) - float(want)) < 1e-4 * abs(float(want))
    with pytest.raises(RuntimeError):
        MaskedCrossEntropyLoss()(y_hat, y)


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("d", [1, 2, 512])
def test_standalone_residual_conv1d_glu_against_golden(name, d):
    """wavenet_vocoder.modules.ResidualConv1dGLU (modules.py:71-169): forward against the reference's single-layer vectors,
    and incremental_forward step by step against forward."""
    from helpers import golden_model, load_npz, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model(name)
    z = load_npz("glu_" + name)
    layer = ResidualConv1dGLU(cfg["R"], cfg["G"], cfg["k"], skip_out_channels=cfg["S"], cin_channels=cfg["Cc"],
                              gin_channels=cfg["Cg"], dropout=0.0, dilation=d)
    pre = "wavenet.conv_layers.1."
    layer.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
    layer = layer.cuda().eval()
    T, B = int(z["T"]), 2
    x = O.hash_fill((B, cfg["R"], T), int(z["x_salt"]), float(z["x_scale"]))
    c = O.hash_fill((B, cfg["Cc"], T), int(z["c_salt"]), float(z["c_scale"]))
    gv = O.hash_fill((B, cfg["Cg"], 1), int(z["g_salt"]), float(z["g_scale"]))
    xo, so = layer(x.cuda(), c.cuda(), gv.cuda().expand(-1, -1, T))
    pt = torch.from_numpy(z["probe_t"])
    assert xo.shape == (B, cfg["R"], T) and so.shape == (B, cfg["S"], T)
    assert rel_err(xo.cpu()[:, :, pt], z[f"xo_d{d}_cg"]) < 1e-4
    assert rel_err(so.cpu()[:, :, pt], z[f"so_d{d}_cg"]) < 1e-4
    # incremental_forward: (B, 1, C) per step with the layer's own buffer (conv.py:17-46); compare 6 steps from a cleared buffer
    if d <= 2:
        layer.clear_buffer()
        n = 6
        xs, cs = x[:, :, :n].cuda(), c[:, :, :n].cuda()
        ref_x, ref_s = layer(xs, cs, gv.cuda().expand(-1, -1, n))
        for t in range(n):
            xi, si = layer.incremental_forward(xs[:, :, t:t + 1].transpose(1, 2), cs[:, :, t:t + 1].transpose(1, 2),
                                               gv.cuda().transpose(1, 2))
            assert xi.shape == (B, 1, cfg["R"]) and si.shape == (B, 1, cfg["S"])
            assert rel_err(xi[:, 0].cpu(), ref_x[:, :, t].cpu()) < 1e-5
            assert rel_err(si[:, 0].cpu(), ref_s[:, :, t].cpu()) < 1e-5
        layer.train()
        with pytest.raises(RuntimeError):
            layer.incremental_forward(xs[:, :, :1].transpose(1, 2))
        layer.eval()
        # (a gradient with respect to the global features: test_standalone_layer_with_time_varying_global_features)
        with torch.no_grad():
            layer.train()
            layer(xs, cs, gv.cuda().expand(-1, -1, n))          # train mode without autograd is an ordinary forward (dropout 0)
            layer.eval()


@pytest.mark.parametrize("name,d", [("A", 1), ("A", 4), ("B", 2)])
def test_standalone_residual_conv1d_glu_is_trainable(name, d):
    """modules.py:109-163 is an ordinary autograd module in the reference: gradients of a scalar function of (x', s) with respect to
    x, c and every parameter (weight_g / weight_v / bias of the five convolutions) against autograd through the oracle's layer."""
    from helpers import golden_model, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model(name)
    pre = "wavenet.conv_layers.1."
    lsd = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre)}
    layer = ResidualConv1dGLU(cfg["R"], cfg["G"], cfg["k"], skip_out_channels=cfg["S"], cin_channels=cfg["Cc"],
                              gin_channels=cfg["Cg"], dropout=0.0, dilation=d)
    layer.load_state_dict(lsd)
    layer = layer.cuda().train()
    B, T = 2, 300
    x = O.hash_fill((B, cfg["R"], T), 31, 0.8)
    c = O.hash_fill((B, cfg["Cc"], T), 32, 0.8)
    gv = O.hash_fill((B, cfg["Cg"], 1), 33, 0.8)
    wx, wsk = O.hash_fill((B, cfg["R"], T), 34), O.hash_fill((B, cfg["S"], T), 35)
    # oracle: autograd through the restated layer
    psd = {pre + k: v.clone().requires_grad_(True) for k, v in lsd.items()}
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    xo_r, so_r = O.glu_layer_forward(psd, pre, xr, cr, gv.expand(-1, -1, T), d)
    ((xo_r * wx).sum() + (so_r * wsk).sum()).backward()
    # the module on the GPU
    xg, cg = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    xo, so = layer(xg, cg, gv.cuda().expand(-1, -1, T))
    assert rel_err(xo.detach().cpu(), xo_r.detach()) < 1e-4 and rel_err(so.detach().cpu(), so_r.detach()) < 1e-4
    ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < 1e-4
    assert rel_err(cg.grad.cpu(), cr.grad) < 1e-4
    params = dict(layer.named_parameters())
    assert set(params) == set(lsd)
    for k, p_ in params.items():
        assert p_.grad is not None, k
        assert rel_err(p_.grad.cpu(), psd[pre + k].grad) < 2e-4, k
    # a second step on the same module: an optimizer that writes through the parameter aliases is seen by the next forward
    with torch.no_grad():
        for p_ in params.values():
            p_.add_(p_.grad, alpha=-1e-2)
            p_.grad = None
    with torch.no_grad():
        for k, v in psd.items():
            v.add_(v.grad, alpha=-1e-2)
    xo2, _ = layer(x.cuda(), c.cuda(), gv.cuda().expand(-1, -1, T))
    xo2_r, _ = O.glu_layer_forward({k: v.detach() for k, v in psd.items()}, pre, x, c, gv.expand(-1, -1, T), d)
    assert rel_err(xo2.detach().cpu(), xo2_r) < 1e-4


def _t(z):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in z.items()}


def test_sliced_vector_quantize_against_reference_vectors():
    """SlicedVectorQuantize (vector_quantization.py:51-128) forward + autograd backward."""
    from wavenet_autoencoders_amd.vector_quantization import SlicedVectorQuantize
    t = _t(load_npz("quantizers"))
    K, K1, D = t["e1"].shape[0], t["e2"].shape[0], t["lats"].shape[2]
    m = SlicedVectorQuantize(K, D, beta=0.25, K1=K1)
    assert set(m.state_dict().keys()) == {"embedding1.weight", "embedding2.weight"}
    m.load_state_dict({"embedding1.weight": t["e1"], "embedding2.weight": t["e2"]})
    m = m.cuda()
    x = t["lats"][0].cuda().requires_grad_(True)
    q, loss, perp = m(x)
    (q * t["w"].cuda()).sum().add(loss).backward()
    assert torch.equal(m.last_indices[0].cpu(), t["s_idx1"]) and torch.equal(m.last_indices[1].cpu(), t["s_idx2"])  # bit-exact
    assert rel_err(q.detach().cpu(), t["s_quant"]) < 1e-6
    assert abs(float(loss) - float(t["s_loss"])) < 1e-6 and abs(float(perp) - float(t["s_perp"])) < 1e-3
    assert rel_err(x.grad.cpu(), t["s_dlat"]) < 1e-5
    assert rel_err(m.embedding1.weight.grad.cpu(), t["s_demb1"]) < 1e-5
    assert rel_err(m.embedding2.weight.grad.cpu(), t["s_demb2"]) < 1e-5
    with pytest.raises(Exception):
        m(t["lats"][0])                                                     # no CPU fallback


@pytest.mark.parametrize("sliced", [False, True])
def test_ema_quantizers_against_reference_vectors(sliced):
    """VectorQuantizeEMA (vector_quantization.py:239-306) / SlicedVectorQuantizeEMA (:132-235): two training steps that move
    the codebook, then an eval step."""
    from wavenet_autoencoders_amd.vector_quantization import SlicedVectorQuantizeEMA, VectorQuantizeEMA
    t = _t(load_npz("quantizers"))
    K, D = t["ef"].shape
    if sliced:
        m = SlicedVectorQuantizeEMA(K, D, beta=0.25, decay=0.9)
        assert set(m.state_dict().keys()) == {"embedding1.weight", "embedding2.weight", "ema_cluster_size1", "ema_w1",
                                              "ema_cluster_size2", "ema_w2"}
        m.embedding1.weight.data.copy_(t["e1"])
        m.embedding2.weight.data.copy_(t["e2k"])
        p, sfx = "se", ("1", "2")
    else:
        m = VectorQuantizeEMA(K, D, beta=0.25, decay=0.9)
        assert set(m.state_dict().keys()) == {"embedding.weight", "ema_cluster_size", "ema_w"}
        m.embedding.weight.data.copy_(t["ef"])
        p, sfx = "e", ("",)
    m = m.cuda()
    for step in range(3):
        m.train(step < 2)
        x = t["lats"][step].cuda().requires_grad_(True)
        q, loss, perp = m(x)
        (q * t["w"].cuda()).sum().add(loss).backward()
        idx = m.last_indices if sliced else (m.last_indices,)
        for s, i in zip(sfx, idx):
            assert torch.equal(i.cpu(), t[f"{p}{step}_idx{s}"])             # bit-exact
            assert rel_err(getattr(m, "embedding" + s).weight.data.cpu(), t[f"{p}{step}_emb{s}"]) < 1e-5
            assert rel_err(getattr(m, "ema_cluster_size" + s).cpu(), t[f"{p}{step}_n{s}"]) < 1e-5
            assert rel_err(getattr(m, "ema_w" + s).cpu(), t[f"{p}{step}_w{s}"]) < 1e-5
            assert getattr(m, "embedding" + s).weight.grad is None
        assert rel_err(q.detach().cpu(), t[f"{p}{step}_quant"]) < 1e-5
        assert abs(float(loss) - float(t[f"{p}{step}_loss"])) < 1e-6 and abs(float(perp) - float(t[f"{p}{step}_perp"])) < 1e-3
        assert rel_err(x.grad.cpu(), t[f"{p}{step}_dlat"]) < 1e-5


def test_reference_default_constructor_and_eval_mode_dropout():
    """WaveNet() with the reference's own defaults (dropout = 1 - 0.95, wavenet.py:98-111) constructs; dropout is the identity in
    eval mode (modules.py:127-128), so its logits equal those of the same weights built with dropout = 0; in training mode the
    mask is active (different logits, still finite, gradients flow)."""
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    torch.manual_seed(3)
    kw = dict(out_channels=64, layers=4, stacks=2, residual_channels=32, gate_channels=48, skip_out_channels=32, cin_channels=-1,
              gin_channels=-1)
    a = WaveNet(**kw).cuda().eval()                       # dropout left at the reference default
    b = WaveNet(dropout=0.0, **kw).cuda().eval()
    b.load_state_dict(a.state_dict())
    assert abs(a.dropout - 0.05) < 1e-12
    x = torch.nn.functional.one_hot(torch.randint(0, 64, (2, 200)), 64).float().transpose(1, 2).contiguous().cuda()
    with torch.no_grad():
        ya, yb = a(x), b(x)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb)
    a.train()
    yt = a(x)
    yt.square().mean().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(yt).all()) and not torch.equal(yt.detach(), ya)
    gsum = sum(float(p.grad.abs().sum()) for p in a.parameters() if p.grad is not None)
    assert gsum > 0 and np.isfinite(gsum)


def test_backward_after_a_second_forward_raises():
    """the saved activations of the drop-in modules live in the engine's workspace: a backward through an older forward must
    fail loudly instead of using the newer forward's activations"""
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    torch.manual_seed(4)
    m = WaveNet(out_channels=64, layers=4, stacks=2, residual_channels=32, gate_channels=48, skip_out_channels=32, cin_channels=-1,
                gin_channels=-1, dropout=0.0).cuda().train()
    x1 = torch.nn.functional.one_hot(torch.randint(0, 64, (2, 200)), 64).float().transpose(1, 2).contiguous().cuda()
    x2 = torch.nn.functional.one_hot(torch.randint(0, 64, (2, 200)), 64).float().transpose(1, 2).contiguous().cuda()
    y1 = m(x1)
    y2 = m(x2)
    with pytest.raises(RuntimeError, match="overwritten"):
        y1.sum().backward()
    y2.sum().backward()                                   # the latest forward is fine


@pytest.mark.parametrize("name", ["A", "B"])
def test_masked_cross_entropy_module_on_explicit_logits(name):
    """losses.MaskedCrossEntropyLoss (vqwae_train.py:363-379) called the reference's way -- criterion(y_hat[:, :, :-1, :],
    y[:, 1:, :], mask=mask) -- runs wae_ce_logits_fwd / _bwd + wae_weighted_mean: value and d loss / d logits against the
    vectors the reference produced (ce_<name>.npz), and the (deferred) IndexError for a target outside the classes."""
    from wavenet_autoencoders_amd.losses import MaskedCrossEntropyLoss, sequence_mask
    cfg, sd, ins, zm, ocfg = golden_model(name)
    z = load_npz("ce_" + name)
    y_hat = torch.from_numpy(zm["y_hat"]).cuda().requires_grad_(True)
    y = ins["x"].unsqueeze(-1).cuda()
    lengths = torch.from_numpy(z["lengths"]).cuda()
    T = y.shape[1]
    mask = sequence_mask(lengths, T).unsqueeze(-1)[:, 1:, :]
    loss = MaskedCrossEntropyLoss()(y_hat.unsqueeze(-1)[:, :, :-1, :], y[:, 1:, :], mask=mask)
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss) - float(z["loss"])) < 1e-5 * float(z["loss"])
    assert rel_err(y_hat.grad.cpu()[:, :, ::29], z["dlogits_probe"]) < 1e-4
    bad = y[:, 1:, :].clone()
    bad[0, 3, 0] = cfg["O"]
    # an out-of-range target is clamped by the kernel and flagged in a sticky device word; the IndexError nn.CrossEntropyLoss raises
    # on the spot comes from check_target_errors() (or, at the latest, from the next loss call): no host sync per loss evaluation
    from wavenet_autoencoders_amd.losses import check_target_errors
    check_target_errors()                                       # the good call above left nothing behind
    MaskedCrossEntropyLoss()(y_hat.detach().unsqueeze(-1)[:, :, :-1, :], bad, mask=mask)
    with pytest.raises(IndexError):
        check_target_errors()
    MaskedCrossEntropyLoss()(y_hat.detach().unsqueeze(-1)[:, :, :-1, :], bad, mask=mask)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        MaskedCrossEntropyLoss()(y_hat.detach().unsqueeze(-1)[:, :, :-1, :], y[:, 1:, :], mask=mask)   # raised by the next call
    check_target_errors()                                       # cleared


def test_out_of_range_ids_raise_index_error():
    """The reference raises IndexError on the spot for a speaker id >= n_speakers (nn.Embedding, wavenet.py:185-187) or a class id
    outside [0, out_channels) (the one-hot encoder / CrossEntropyLoss).  The kernels clamp such ids and set a sticky flag;
    the module API turns it into the same IndexError at the end of the call, the engine API in check_errors()."""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, ins, z, ocfg = golden_model("A")
    model, wn = _build(cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    g_bad = ins["g"].clone()
    g_bad[1] = cfg["n_speakers"] + 3
    with torch.no_grad():
        with pytest.raises(IndexError, match="speaker id"):
            model(ins["xin"].cuda(), ins["c"].cuda(), g_bad.cuda(), False)
        model(ins["xin"].cuda(), ins["c"].cuda(), ins["g"].cuda(), False)       # the flag is cleared: a good call passes again
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="bf16")
    eng.load_state_dict(sd)
    eng.init_optimizer()
    x_bad = ins["x"].clone()
    x_bad[0, 17] = cfg["O"] + 5
    eng.train_step(x_bad.cuda(), ins["c"].cuda(), ins["g"].cuda())
    with pytest.raises(IndexError, match="class id"):
        eng.check_errors()
    eng.train_step(ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda())
    eng.check_errors()


def test_dense_decoder_input_is_refused_and_start_classes_are_per_utterance():
    """wavenet.py:203 applies first_conv as a dense 1x1 to any (B, C, T) float tensor; the teacher-forced kernels gather weight rows by
    class id, the same arithmetic for ONE-HOT columns only.  Soft labels are refused (NotImplementedError at the end of the call),
    never arg-maxed (round-5 finding); one-hot columns in either layout give the logits of the id path.  incremental_forward starts
    every utterance from its own row of initial_input (wavenet.py:283-297)."""
    cfg, sd, ins, z, ocfg = golden_model("A")
    model, wn = _build(cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    xin = ins["xin"].cuda()
    with torch.no_grad():
        y_ref, _, _ = model(xin, ins["c"].cuda(), ins["g"].cuda(), False)
        y_ids, _, _ = model(ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda(), False)         # (B, T) class ids
        assert torch.equal(y_ref, y_ids)
        soft = xin * 0.9 + 0.1 / cfg["O"]                        # label smoothing: columns still sum to one, argmax unchanged
        with pytest.raises(NotImplementedError, match="not one-hot"):
            model(soft, ins["c"].cuda(), ins["g"].cuda(), False)
        two = xin.clone()
        two[0, 5, 3] = 1.0                                        # a second one in one column
        if float(xin[0, 5, 3]) == 1.0:
            two[0, 6, 3] = 1.0
        with pytest.raises(NotImplementedError, match="not one-hot"):
            model(two, ins["c"].cuda(), ins["g"].cuda(), False)
        y_again, _, _ = model(xin, ins["c"].cuda(), ins["g"].cuda(), False)                   # the flag is cleared
        assert torch.equal(y_again, y_ref)
    # per-utterance start classes through the module API, against the oracle's restatement of the reference loop (greedy, fp32)
    za = load_npz("ar_A")
    T = 16
    c_up = torch.from_numpy(za["c_up"])[:, :, :T].contiguous()
    starts = [1, cfg["O"] - 3]
    init = torch.zeros(2, cfg["O"], 1)
    for b, s_ in enumerate(starts):
        init[b, s_, 0] = 1
    ref = O.incremental_forward(sd, ocfg, c_up, ins["g"], T, initial_input=init, mode="logits")    # logits fed back (quantize=False)
    _, wn3 = _build(cfg)
    wn3.load_state_dict({k[len("wavenet."):]: v for k, v in sd.items() if k.startswith("wavenet.")})
    wn3 = wn3.cuda().eval()
    got = wn3.incremental_forward(init.cuda(), c=c_up.cuda(), g=ins["g"].cuda(), T=T, softmax=False, quantize=False)
    assert rel_err(got.cpu(), ref) < 1e-3
    got_t = wn3.incremental_forward(init.transpose(1, 2).contiguous().cuda(), c=c_up.cuda(), g=ins["g"].cuda(), T=T, softmax=False,
                                    quantize=False)                                                  # (B, 1, C) start rows
    assert torch.equal(got_t, got)
    with pytest.raises(NotImplementedError, match="not one-hot"):
        wn3.incremental_forward(init.cuda() * 0.5, c=c_up.cuda(), g=ins["g"].cuda(), T=T, softmax=False, quantize=False)


@pytest.mark.parametrize("name,d,with_c", [("A", 2, True), ("B", 4, True), ("A", 1, False)])
def test_standalone_layer_with_time_varying_global_features(name, d, with_c):
    """modules.py:148-152 convolves whatever (B, gin_channels, T) tensor it is given; the reference's WaveNet hands it one speaker vector
    expanded over time, a caller of the stand-alone layer may hand it a time series and ask for its gradient.  Round 5: such a call
    switches the layer to Geometry.g_local (conv1x1g's columns behind conv1x1c's in the kernel's conditioning operand).  Outputs and the
    gradients of x, c, g and every parameter against autograd through the oracle's layer; a constant-over-time g through the same
    geometry afterwards gives the hoisted path's result."""
    from helpers import golden_model, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model(name)
    pre = "wavenet.conv_layers.1."
    lsd = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre) and (with_c or "conv1x1c" not in k)}
    layer = ResidualConv1dGLU(cfg["R"], cfg["G"], cfg["k"], skip_out_channels=cfg["S"], cin_channels=cfg["Cc"] if with_c else -1,
                              gin_channels=cfg["Cg"], dropout=0.0, dilation=d)
    layer.load_state_dict(lsd)
    layer = layer.cuda().train()
    B, T = 2, 300
    x = O.hash_fill((B, cfg["R"], T), 41, 0.8)
    c = O.hash_fill((B, cfg["Cc"], T), 42, 0.8) if with_c else None
    g = O.hash_fill((B, cfg["Cg"], T), 43, 0.8)                    # varies over time
    wx, wsk = O.hash_fill((B, cfg["R"], T), 44), O.hash_fill((B, cfg["S"], T), 45)
    psd = {pre + k: v.clone().requires_grad_(True) for k, v in lsd.items()}
    xr, gr = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    cr = c.clone().requires_grad_(True) if with_c else None
    xo_r, so_r = O.glu_layer_forward(psd, pre, xr, cr, gr, d)
    ((xo_r * wx).sum() + (so_r * wsk).sum()).backward()
    xg, gg = x.cuda().requires_grad_(True), g.cuda().requires_grad_(True)
    cg = c.cuda().requires_grad_(True) if with_c else None
    assert not layer.geom.g_local
    xo, so = layer(xg, cg, gg)
    assert layer.geom.g_local and layer.geom.Cx == (cfg["Cc"] if with_c else 0) + cfg["Cg"]
    assert rel_err(xo.detach().cpu(), xo_r.detach()) < 1e-4 and rel_err(so.detach().cpu(), so_r.detach()) < 1e-4
    ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < 1e-4
    assert rel_err(gg.grad.cpu(), gr.grad) < 1e-4
    if with_c:
        assert rel_err(cg.grad.cpu(), cr.grad) < 1e-4
    params = dict(layer.named_parameters())
    assert set(params) == set(lsd)
    for k, p_ in params.items():
        assert p_.grad is not None, k
        assert rel_err(p_.grad.cpu(), psd[pre + k].grad) < 2e-4, k
    # a constant-over-time g (B, Cg, 1) through the same geometry = the reference's expanded speaker vector
    layer.eval()
    gv = O.hash_fill((B, cfg["Cg"], 1), 46, 0.8)
    with torch.no_grad():
        xo2, so2 = layer(x.cuda(), c.cuda() if with_c else None, gv.cuda())
        xo2_r, so2_r = O.glu_layer_forward({k: v.detach() for k, v in psd.items()}, pre, x, c, gv.expand(-1, -1, T), d)
    assert rel_err(xo2.cpu(), xo2_r) < 1e-4 and rel_err(so2.cpu(), so2_r) < 1e-4


@pytest.mark.parametrize("p_drop", [0.05, 0.4])
def test_standalone_layer_trains_with_dropout(p_drop):
    """modules.py:127-128: the reference's constructor default is dropout = 0.05 and F.dropout is active in training mode.  The stand-alone
    layer now applies the engine's counter-based mask (one seed per forward call); torch's Philox stream cannot be reproduced, so parity is
    against the oracle under the SAME mask (oracle.wae_oracle.dropout_keep restates the hash): outputs, gradients of x, c and every
    parameter; two forwards draw different masks; eval mode is the identity."""
    from helpers import golden_model, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model("A")
    pre = "wavenet.conv_layers.1."
    lsd = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre)}
    d = 2
    layer = ResidualConv1dGLU(cfg["R"], cfg["G"], cfg["k"], skip_out_channels=cfg["S"], cin_channels=cfg["Cc"],
                              gin_channels=cfg["Cg"], dropout=p_drop, dilation=d)
    layer.load_state_dict(lsd)
    layer = layer.cuda().train()
    B, T = 2, 300
    x = O.hash_fill((B, cfg["R"], T), 51, 0.8)
    c = O.hash_fill((B, cfg["Cc"], T), 52, 0.8)
    gv = O.hash_fill((B, cfg["Cg"], 1), 53, 0.8)
    wx, wsk = O.hash_fill((B, cfg["R"], T), 54), O.hash_fill((B, cfg["S"], T), 55)
    outs = []
    for call in (1, 2):
        xg, cg = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
        for p_ in layer.parameters():
            p_.grad = None
        xo, so = layer(xg, cg, gv.cuda().expand(-1, -1, T))
        eng = layer._engine
        assert eng.drop_calls == call
        keep = O.dropout_keep(eng.layer_drop_seed(call, 0), B, cfg["R"], T, p_drop)
        assert abs(float(keep.float().mean()) - (1 - p_drop)) < 0.03
        psd = {pre + k: v.clone().requires_grad_(True) for k, v in lsd.items()}
        xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
        xo_r, so_r = O.glu_layer_forward(psd, pre, xr, cr, gv.expand(-1, -1, T), d, keep=keep, p=p_drop)
        ((xo_r * wx).sum() + (so_r * wsk).sum()).backward()
        assert rel_err(xo.detach().cpu(), xo_r.detach()) < 1e-4 and rel_err(so.detach().cpu(), so_r.detach()) < 1e-4
        ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
        assert rel_err(xg.grad.cpu(), xr.grad) < 1e-4
        assert rel_err(cg.grad.cpu(), cr.grad) < 1e-4
        for k, p_ in layer.named_parameters():
            assert rel_err(p_.grad.cpu(), psd[pre + k].grad) < 2e-4, k
        outs.append(xo.detach().clone())
    assert not torch.equal(outs[0], outs[1])               # another call, another mask
    layer.eval()
    with torch.no_grad():
        xe, _ = layer(x.cuda(), c.cuda(), gv.cuda().expand(-1, -1, T))
        xe_r, _ = O.glu_layer_forward({pre + k: v for k, v in lsd.items()}, pre, x, c, gv.expand(-1, -1, T), d)
    assert rel_err(xe.cpu(), xe_r) < 1e-4


def test_standalone_layer_without_biases():
    """modules.py:88-107 with bias=False: conv, conv1x1_out and conv1x1_skip have no bias (state_dict without the three keys); outputs and
    the gradients of x, c and every parameter against autograd through the oracle's layer on a state_dict without them."""
    from helpers import golden_model, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model("A")
    pre = "wavenet.conv_layers.1."
    lsd = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre) and not k.endswith(".bias")}
    layer = ResidualConv1dGLU(cfg["R"], cfg["G"], cfg["k"], skip_out_channels=cfg["S"], cin_channels=cfg["Cc"],
                              gin_channels=cfg["Cg"], dropout=0.0, dilation=2, bias=False)
    assert set(layer.state_dict()) == set(lsd) and not any(k.endswith(".bias") for k in layer.state_dict())
    layer.load_state_dict(lsd)
    layer = layer.cuda().train()
    B, T = 2, 300
    x = O.hash_fill((B, cfg["R"], T), 81, 0.8)
    c = O.hash_fill((B, cfg["Cc"], T), 82, 0.8)
    gv = O.hash_fill((B, cfg["Cg"], 1), 83, 0.8)
    wx, wsk = O.hash_fill((B, cfg["R"], T), 84), O.hash_fill((B, cfg["S"], T), 85)
    psd = {pre + k: v.clone().requires_grad_(True) for k, v in lsd.items()}
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    xo_r, so_r = O.glu_layer_forward(psd, pre, xr, cr, gv.expand(-1, -1, T), 2)
    ((xo_r * wx).sum() + (so_r * wsk).sum()).backward()
    xg, cg = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    xo, so = layer(xg, cg, gv.cuda().expand(-1, -1, T))
    assert rel_err(xo.detach().cpu(), xo_r.detach()) < 1e-4 and rel_err(so.detach().cpu(), so_r.detach()) < 1e-4
    ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
    assert rel_err(xg.grad.cpu(), xr.grad) < 1e-4 and rel_err(cg.grad.cpu(), cr.grad) < 1e-4
    for k, p_ in layer.named_parameters():
        assert p_.grad is not None and rel_err(p_.grad.cpu(), psd[pre + k].grad) < 2e-4, k


@pytest.mark.parametrize("d", [1, 8])
def test_standalone_layer_non_causal_against_reference_vectors(d):
    """modules.py:82-88 with causal=False (symmetric padding (k-1)//2 * d, nothing trimmed): outputs and the gradients of x, c and every
    parameter against the REFERENCE module's own forward and autograd (tests/golden/glu_noncausal.npz; the causal kernels on a frame
    shifted by d).  Then: a time-varying g with a gradient, training-mode dropout and bf16 against autograd through the oracle's layer;
    even kernel sizes and incremental_forward are refused."""
    from helpers import golden_model, load_npz, rel_err
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd.wavenet_vocoder.modules import ResidualConv1dGLU
    cfg, sd, ins, zm, ocfg = golden_model("A")
    z = load_npz("glu_noncausal")
    pre = "wavenet.conv_layers.1."
    lsd = {k[len(pre):]: v.clone() for k, v in sd.items() if k.startswith(pre)}
    B, T, sc = int(z["B"]), int(z["T"]), float(z["scale"])
    x, c = O.hash_fill((B, cfg["R"], T), int(z["x_salt"]), sc), O.hash_fill((B, cfg["Cc"], T), int(z["c_salt"]), sc)
    gv = O.hash_fill((B, cfg["Cg"], 1), int(z["g_salt"]), sc)
    wx, wsk = O.hash_fill((B, cfg["R"], T), int(z["wx_salt"])), O.hash_fill((B, cfg["S"], T), int(z["ws_salt"]))

    def make(**kw):
        lay = ResidualConv1dGLU(cfg["R"], cfg["G"], 3, skip_out_channels=cfg["S"], cin_channels=cfg["Cc"], gin_channels=cfg["Cg"],
                                dilation=d, causal=False, **kw)
        lay.load_state_dict(lsd)
        return lay.cuda()
    layer = make(dropout=0.0).train()
    xg, cg = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True)
    xo, so = layer(xg, cg, gv.cuda().expand(-1, -1, T))
    assert xo.shape == (B, cfg["R"], T) and so.shape == (B, cfg["S"], T)
    assert rel_err(xo.detach().cpu(), z[f"xo_d{d}"]) < 1e-4 and rel_err(so.detach().cpu(), z[f"so_d{d}"]) < 1e-4
    ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
    assert rel_err(xg.grad.cpu(), z[f"dx_d{d}"]) < 1e-4 and rel_err(cg.grad.cpu(), z[f"dc_d{d}"]) < 1e-4
    for k, p_ in layer.named_parameters():
        assert p_.grad is not None and rel_err(p_.grad.cpu(), z[f"grad_d{d}:{k}"]) < 2e-4, k
    with torch.no_grad():            # eval mode, no autograd: the same outputs
        xe, se = layer.eval()(x.cuda(), c.cuda(), gv.cuda().expand(-1, -1, T))
    assert rel_err(xe.cpu(), z[f"xo_d{d}"]) < 1e-4 and rel_err(se.cpu(), z[f"so_d{d}"]) < 1e-4
    # g as a time series with a gradient; training-mode dropout (the mask lives in the kernels' frame of T + d steps); bf16
    psd = {pre + k: v.clone().requires_grad_(True) for k, v in lsd.items()}
    gt = O.hash_fill((B, cfg["Cg"], T), 931, 0.7)
    xr, cr, gr = x.clone().requires_grad_(True), c.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    xo_r, so_r = O.glu_layer_forward(psd, pre, xr, cr, gr, d, causal=False)
    ((xo_r * wx).sum() + (so_r * wsk).sum()).backward()
    for dtype, tol in (("fp32", 1e-4), ("bf16", 4e-2)):
        lay = make(dropout=0.0).set_compute_dtype(dtype).train()
        xg, cg, gg = x.cuda().requires_grad_(True), c.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
        xo, so = lay(xg, cg, gg)
        assert rel_err(xo.detach().cpu(), xo_r.detach()) < tol and rel_err(so.detach().cpu(), so_r.detach()) < tol
        ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
        assert rel_err(xg.grad.cpu(), xr.grad) < tol and rel_err(cg.grad.cpu(), cr.grad) < tol and rel_err(gg.grad.cpu(), gr.grad) < tol
        for k, p_ in lay.named_parameters():
            assert rel_err(p_.grad.cpu(), psd[pre + k].grad) < 2 * tol, (dtype, k)
    pd = 0.3
    lay = make(dropout=pd).train()
    xg = x.cuda().requires_grad_(True)
    xo, so = lay(xg, c.cuda(), gv.cuda().expand(-1, -1, T))
    eng = lay.engine()
    keep = O.dropout_keep(eng.layer_drop_seed(eng.drop_calls, 0), B, cfg["R"], T + d, pd)[:, :, :T]     # the convolution operand's rows [0, T)
    xq = x.clone().requires_grad_(True)
    xo_q, so_q = O.glu_layer_forward({k: v.detach() for k, v in psd.items()}, pre, xq, c, gv.expand(-1, -1, T), d, keep=keep, p=pd, causal=False)
    assert rel_err(xo.detach().cpu(), xo_q.detach()) < 1e-4 and rel_err(so.detach().cpu(), so_q.detach()) < 1e-4
    ((xo * wx.cuda()).sum() + (so * wsk.cuda()).sum()).backward()
    ((xo_q * wx).sum() + (so_q * wsk).sum()).backward()
    assert rel_err(xg.grad.cpu(), xq.grad) < 1e-4
    with pytest.raises(NotImplementedError):
        ResidualConv1dGLU(cfg["R"], cfg["G"], 2, causal=False)
    with pytest.raises(NotImplementedError):
        layer.eval().incremental_forward(x[:, :, :1].transpose(1, 2).cuda())


def test_train_step_takes_the_speaker_ids_of_a_fresh_tensor_per_batch():
    """train_step keeps the int32 copy of the speaker ids while it is handed the SAME id tensor (a benchmark's fixture).  A data loader
    hands it a fresh int64 tensor per batch, freed before the next one is allocated -- which the caching allocator places at the same
    address, version 0: the cache holds the source tensor and compares by identity, so the second batch's ids are the ones used.
    Two steps on golden model A (fp32, one chain); the second step's loss against a fresh engine stepped once from the same
    parameters with the second ids (the same launches on the same weights: 1e-6 for the VQ term's atomically summed statistics)."""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, ins, z, ocfg = golden_model("A")
    x, c = ins["x"].cuda(), ins["c"].cuda()
    first = [int(v) for v in ins["g"]]
    second = [(v + 1 + i) % cfg["n_speakers"] for i, v in enumerate(first)]
    assert all(a != b_ for a, b_ in zip(first, second))

    def step(eng, ids):
        gid = torch.tensor(ids, dtype=torch.int64, device="cuda")      # built here, dropped on return
        return eng.train_step(x, c, gid, lr=1e-3)["loss"].detach().clone()

    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    eng.init_optimizer()
    step(eng, first)
    torch.cuda.synchronize()
    params = eng.params.clone()
    loss = float(step(eng, second))
    assert eng._gid32.dtype == torch.int32 and eng._gid32.tolist() == second
    ref = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    ref.load_state_dict(sd)
    ref.init_optimizer()
    ref.params.copy_(params)
    want = float(step(ref, second))
    print("second step's loss", loss, "fresh engine's", want)
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
