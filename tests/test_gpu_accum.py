"""Gradient accumulation (WaeEngine.accumulate / apply_step / discard_step / train_step_accum; backward.py: deferred finishing;
csrc/accum.hip): a window of micro-batches against the reference's golden step, against one step on the concatenated batch, against
autograd through the oracle for micro-batches of different shapes, and what a window leaves behind.

Geometries: A = golden_model("A") (4 layers, R 32, encoder + VQ, hop 640) with inputs of its own; W = the 10-layer R = G = S = 256
decoder without encoder of test_gpu_backward.py::test_weight_gradients_beside_an_underfilled_sweep (the static weight-gradient launch,
`beside`, the gather pass).
Bounds of "the same addends in another order of fp32 additions" (test_gpu_backward.py::test_side_streams_change_nothing): gradients
<= 2e-5 (fp32) / 2e-3 (16-bit) of max|g|, parameters < 1e-5 / 2e-3, losses < 1e-5 / 2e-3; the perplexity to 1e-6 relative."""
import ctypes
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
LR = 1e-3
W_CFG = dict(layers=10, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=11, upsample_scales=[4, 4, 8, 5], cin_pad=0)


def _tol(dtype):
    return dict(g=2e-5, p=1e-5, l=1e-5) if dtype == "fp32" else dict(g=2e-3, p=2e-3, l=2e-3)


def _engine(cfg, sd, dtype, strict=True):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd, strict=strict)
    eng.init_optimizer()
    return eng


def _batch_a(B=4, T=1280, lengths=(1280, 1063, 900, 641), speakers=(3, 0, 4, 1), seed=91):
    """own inputs for geometry A from a seeded generator: (x, c, g, lengths) on the device (lengths on the host)"""
    cfg = golden_model("A")[0]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, cfg["O"], (B, T), generator=gen)
    c = torch.randn(B, cfg["c_in"], T // 160, generator=gen)
    return x.cuda(), c.cuda(), torch.tensor(speakers).cuda(), torch.tensor(lengths)


def _batch_w():
    B, T, hop = 3, 1920, 640
    gen = torch.Generator().manual_seed(377)
    x = torch.randint(0, 256, (B, T), generator=gen).cuda()
    c = torch.randn(B, 64, T // hop, generator=gen).cuda()
    g = torch.randint(0, W_CFG["n_speakers"], (B,), generator=gen).cuda()
    return x, c, g, torch.tensor([T - 97 * i for i in range(B)])


def _parts(batch, split):
    x, c, g, lengths = batch
    out, lo = [], 0
    for n in split:
        out.append((x[lo:lo + n], c[lo:lo + n], g[lo:lo + n], lengths[lo:lo + n]))
        lo += n
    assert lo == x.shape[0]
    return out


def _numbers(res):
    return {k: float(v) for k, v in res.items() if k in ("loss", "ce", "vq_loss", "perp", "grad_norm")}


def _plain_step(cfg, sd, dtype, batch, strict=True):
    eng = _engine(cfg, sd, dtype, strict)
    seen = {}
    x, c, g, lengths = batch
    res = eng.train_step(x, c, g, lengths=lengths, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    out = (_numbers(res), seen["g"].cpu(), eng.params.cpu().clone())
    del eng
    torch.cuda.empty_cache()
    return out


def _window_step(cfg, sd, dtype, batch, split, strict=True, **opts):
    eng = _engine(cfg, sd, dtype, strict)
    for k, v in opts.items():          # launch-path switches (options.py), set before the first step builds its tables
        assert hasattr(eng.opt, k), k
        setattr(eng.opt, k, v)
    seen = {}
    res = eng.train_step_accum(_parts(batch, split), lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    assert res["micro_batches"] == len(split) and eng.window is None and eng.opt_step == 1
    out = (_numbers(res), seen["g"].cpu(), eng.params.cpu().clone())
    del eng
    torch.cuda.empty_cache()
    return out


def _close(got, ref, dtype, what=""):
    """case 2's bounds; prints every figure before it asserts"""
    tol = _tol(dtype)
    (n0, g0, p0), (n1, g1, p1) = got, ref
    gerr, gmax, perr = float((g0 - g1).abs().max()), float(g1.abs().max()), float((p0 - p1).abs().max())
    lerr = {k: abs(n0[k] - n1[k]) for k in ("loss", "ce", "vq_loss") if k in n1}
    print(f"{what} {dtype}: grad err {gerr:.3e} of max|g| {gmax:.3e} ({gerr / gmax:.2e}), param err {perr:.3e}, losses {lerr}, "
          f"perp {n0.get('perp')} vs {n1.get('perp')}, grad_norm {n0['grad_norm']} vs {n1['grad_norm']}")
    assert gerr <= tol["g"] * gmax
    assert perr < tol["p"]
    assert all(v < tol["l"] for v in lerr.values()), lerr
    if "perp" in n1:
        assert abs(n0["perp"] - n1["perp"]) <= 1e-6 * n1["perp"]


# ---------------------------------------------------------------- 1. against the reference
def test_window_of_the_golden_batch_against_the_reference():
    """The golden batch of train_A.npz, fp32, as a window of its two clips under accum_weights: loss, vq_loss, grad_norm, every
    gradient tensor, the post-Adam parameters and the EMA shadow to the tolerances of
    test_gpu_backward.py::test_full_train_step_against_golden (no grad_hook: the norm is the gather pass's sum)."""
    cfg, sd, ins, zm, ocfg = golden_model("A")
    z = load_npz("train_A")
    eng = _engine(cfg, sd, "fp32")
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    res = eng.train_step_accum(_parts((x, c, g, torch.tensor([T, T])), [1, 1]), lr=4e-4, clip_thresh=100.0, ema_decay=0.9999)
    torch.cuda.synchronize()
    print({k: (float(res[k]), float(z[k])) for k in ("loss", "vq_loss", "grad_norm", "perp")})
    assert res["micro_batches"] == 2
    assert abs(float(res["loss"]) - float(z["loss"])) < 1e-4
    assert abs(float(res["vq_loss"]) - float(z["vq_loss"])) < 1e-5
    assert abs(float(res["grad_norm"]) - float(z["grad_norm"])) < 1e-3 * float(z["grad_norm"])
    lay = eng.lay
    for key in [k[5:] for k in z if k.startswith("grad:")]:
        view = lambda a: a[lay.off(key):lay.off(key) + lay.numel(key)].view(lay.shapes[key]).cpu()  # noqa: E731
        assert rel_err(view(eng.grads), z["grad:" + key]) < 2e-3, key
        assert rel_err(view(eng.params), z["new:" + key]) < 5e-5, key
        assert rel_err(view(eng.shadow), z["ema:" + key]) < 1e-6, key


# ---------------------------------------------------------------- 2. against one step on the concatenated batch
_REF = {}


def _ref(name, dtype):
    if (name, dtype) not in _REF:
        if name == "A":
            cfg, sd = golden_model("A")[:2]
            _REF[(name, dtype)] = _plain_step(cfg, sd, dtype, _batch_a())
        else:
            sd = O.make_state_dict(dict(W_CFG), salt=9, with_encoder=False)
            _REF[(name, dtype)] = _plain_step(W_CFG, sd, dtype, _batch_w(), strict=False)
    return _REF[(name, dtype)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("split", [[1, 3], [2, 2], [1, 1, 2]])
def test_window_equals_one_step_on_the_concatenated_batch(split, dtype):
    """A: B = 4, T = 1280, ragged lengths, four speakers; fresh engines; gradients through grad_hook, parameters and losses after
    the step, the perplexity against the concatenated batch's."""
    cfg, sd = golden_model("A")[:2]
    _close(_window_step(cfg, sd, dtype, _batch_a(), split), _ref("A", dtype), dtype, f"A {split}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("split", [[1, 2], [1, 1, 1]])
def test_window_equals_one_step_on_the_wide_decoder(split, dtype):
    """W: B = 3, T = 1920 -- the static weight-gradient launch (with its `beside` form where the shape takes it) and the gather pass"""
    sd = O.make_state_dict(dict(W_CFG), salt=9, with_encoder=False)
    _close(_window_step(W_CFG, sd, dtype, _batch_w(), split, strict=False), _ref("W", dtype), dtype, f"W {split}")


@pytest.mark.parametrize("name,dtype", [("A", "fp32"), ("A", "bf16"), ("W", "bf16")])
@pytest.mark.parametrize("opts", [dict(grad_finish=False), dict(side=False)], ids=["split_finish", "one_stream"])
def test_window_under_the_other_finish_and_on_one_stream(opts, name, dtype):
    """The close of a window by the split launches (WAE_GRAD_FINISH=0: scatter of every block, weight-norm backward, a pass for the
    norm) and a window with every launch on one stream (WAE_SIDE=0), against the concatenated batch's step under the defaults."""
    if name == "A":
        cfg, sd = golden_model("A")[:2]
        got = _window_step(cfg, sd, dtype, _batch_a(), [1, 3], **opts)
    else:
        sd = O.make_state_dict(dict(W_CFG), salt=9, with_encoder=False)
        got = _window_step(W_CFG, sd, dtype, _batch_w(), [2, 1], strict=False, **opts)
    _close(got, _ref(name, dtype), dtype, f"{name} {opts}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_window_of_a_scalar_input_model(dtype):
    """golden_model("S") (scalar input, mixture-of-logistics loss through ext_dy, encoder + VQ): its batch as a window of its two clips
    with ragged lengths against the step on the batch."""
    cfg, sd, ins = golden_model("S")[:3]
    x, c, g = ins["x"][:, 0, :].contiguous().cuda(), ins["c"].cuda(), ins["g"].cuda()
    batch = (x, c, g, torch.tensor([x.shape[1], x.shape[1] - 97]))
    _close(_window_step(cfg, sd, dtype, batch, [1, 1]), _plain_step(cfg, sd, dtype, batch), dtype, "S [1, 1]")


def test_window_of_one_micro_batch_with_dropout_is_the_plain_step():
    """Dropout masks follow the engine's call counter and the batch's element count, so only a window of ONE micro-batch has a plain
    step with the same masks: the deferred order under dropout (tap contraction + wae_dropout_bwd in the sweep, no chains), and
    discard_step puts the counter back."""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd = golden_model("A")[:2]
    batch = _batch_a()
    out = []
    for how in ("plain", "window"):
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype="bf16", dropout=0.1)
        eng.load_state_dict(sd)
        eng.init_optimizer()
        seen = {}
        hook = lambda gr: seen.__setitem__("g", gr.clone())  # noqa: E731
        if how == "plain":
            res = eng.train_step(*batch[:3], lengths=batch[3], lr=LR, grad_hook=hook)
        else:
            eng.accumulate(*batch)
            eng.discard_step()
            assert eng.drop_calls == 0
            res = eng.train_step_accum([batch], lr=LR, grad_hook=hook)
        torch.cuda.synchronize()
        assert eng.drop_calls == 1
        out.append((_numbers(res), seen["g"].cpu(), eng.params.cpu().clone()))
    _close(out[1], out[0], "bf16", "dropout")


# ---------------------------------------------------------------- 3. speaker columns do not leak
def test_speaker_columns_do_not_leak_between_micro_batches():
    """Two micro-batches of one shape with disjoint speakers: the embedding rows of speakers in neither are exactly 0.0, and the rows
    of micro-batch 1's speakers are ce_weight_1 x their rows from a plain backward of micro-batch 1 alone."""
    from wavenet_autoencoders_amd.distributed import accum_weights
    cfg, sd = golden_model("A")[:2]
    x, c, g, lengths = _batch_a(speakers=(0, 1, 2, 3))          # n_speakers = 5: speaker 4 appears nowhere
    parts = _parts((x, c, g, lengths), [2, 2])
    eng = _engine(cfg, sd, "fp32")
    seen = {}
    eng.train_step_accum(parts, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    lay = eng.lay
    emb = lambda a: a[lay.off("wavenet.embed_speakers.weight"):][:lay.numel("wavenet.embed_speakers.weight")].view(5, cfg["Cg"]).cpu()  # noqa: E731
    got = emb(seen["g"])
    assert torch.equal(got[4], torch.zeros(cfg["Cg"]))
    metas = [(p[0].shape[0], p[0].shape[1], p[3], eng.latent_elements(p[0].shape[0], p[1].shape[-1])) for p in parts]
    (w1, v1), _ = accum_weights(metas)[0]
    one = _engine(cfg, sd, "fp32")
    x1, c1, g1, l1 = parts[0]
    one.forward(x1, c1, g1, targets=x1, lengths=l1, want_logits=False, train=True)
    ref = emb(one.backward(x1, g1, x1, l1, loss_scale=1.0, vq_scale=1.0)) * w1
    torch.cuda.synchronize()
    err, top = float((got[:2] - ref[:2]).abs().max()), float(ref[:2].abs().max())
    print(f"embedding rows of micro-batch 1: err {err:.3e} of {top:.3e}; rows of micro-batch 2 in the plain backward: "
          f"{float(ref[2:4].abs().max())}")
    assert top > 0 and err <= 2e-5 * top
    assert float(got[2:4].abs().max()) > 0 and float(ref[2:].abs().max()) == 0.0


def test_consuming_entry_is_bitwise_gproj_bwd_and_zeroes_its_columns():
    """wae_gproj_bwd_consume against wae_gproj_bwd on the same tiles, layer by layer (one layer and distinct speakers: an embedding
    slot then gets two addends, one per 32-row block, so its bits do not depend on the order of the atomics): d_eff bit for bit, the
    per-clip columns zero afterwards, nothing else of the tile touched."""
    from wavenet_autoencoders_amd import _lib as L
    from wavenet_autoencoders_amd import backward as BW
    cfg, sd = golden_model("A")[:2]
    eng = _engine(cfg, sd, "fp32")
    eng.prepare_weights()
    BW._prepare_bwd(eng)
    g, lay, sm = eng.g, eng.lay, eng.sm
    assert 2 * g.Hp <= 64
    B, Z2 = 3, 2 * g.Hp
    gen = torch.Generator().manual_seed(5)
    gid = torch.tensor([4, 0, 2], dtype=torch.int32).cuda()
    c1_0 = torch.randn(eng.cview["c1"].numel(), generator=gen).cuda()
    d0 = torch.randn(lay.total, generator=gen).cuda()
    e0, e1 = lay.off("wavenet.embed_speakers.weight"), lay.off("wavenet.embed_speakers.weight") + lay.numel("wavenet.embed_speakers.weight")
    d0[e0:e1] = 0
    ones_col = g.k * g.Rp + g.Ccp
    for l in range(g.layers):
        outs = []
        for name in ("wae_gproj_bwd", "wae_gproj_bwd_consume"):
            c1, d = c1_0.clone(), d0.clone()
            rc = getattr(eng.lib, name)(L.ptr(eng.eff), L.ptr(d), lay.off("wavenet.conv_layers.0.conv1x1g.weight_v") + l * lay.layer_stride,
                                        lay.off("wavenet.conv_layers.0.conv.bias") + l * lay.layer_stride, lay.layer_stride, L.ptr(gid),
                                        e0, None, ctypes.c_void_p(c1.data_ptr() + l * Z2 * sm["ld1"] * 4), Z2 * sm["ld1"], sm["ld1"],
                                        ones_col, B, 1, g.G, g.Hp, g.Cg, g.n_speakers, eng.stream())
            L.check(rc, name)
            torch.cuda.synchronize()
            outs.append((c1.cpu(), d.cpu()))
        (c_plain, d_plain), (c_cons, d_cons) = outs
        assert torch.equal(c_plain, c1_0.cpu())
        assert not torch.equal(d_plain, d0.cpu()) and torch.equal(d_plain, d_cons), l
        want = c1_0.cpu().view(g.layers, Z2, sm["ld1"]).clone()
        want[l, :, ones_col:ones_col + B] = 0
        assert torch.equal(c_cons.view(g.layers, Z2, sm["ld1"]), want), l
    # columns that do not fit the tile's rows are refused before any launch
    rc = eng.lib.wae_gproj_bwd_consume(L.ptr(eng.eff), L.ptr(d0), -1, lay.off("wavenet.conv_layers.0.conv.bias"), lay.layer_stride, None, 0,
                                       None, L.ptr(c1_0), Z2 * sm["ld1"], sm["ld1"], sm["ld1"] - 2, B, 1, g.G, g.Hp, g.Cg, 0, eng.stream())
    assert rc != 0


# ---------------------------------------------------------------- 4. different shapes in one window
def test_micro_batches_of_different_shapes_against_autograd_through_the_oracle():
    """A, fp32: (B 2, T 1280) and (B 1, T 1920) with ragged lengths in one window; every gradient tensor against the oracle's autograd
    of sum ce_weight_i masked_ce_i + sum vq_weight_i vq_loss_i (rel_err < 2e-3, the golden test's bound)."""
    from wavenet_autoencoders_amd.distributed import accum_weights
    cfg, sd, _, _, ocfg = golden_model("A")
    b1 = _batch_a(B=2, T=1280, lengths=(1280, 977), speakers=(2, 0), seed=17)
    b2 = _batch_a(B=1, T=1920, lengths=(1803,), speakers=(4,), seed=18)
    eng = _engine(cfg, sd, "fp32")
    metas = [(b[0].shape[0], b[0].shape[1], b[3], eng.latent_elements(b[0].shape[0], b[1].shape[-1])) for b in (b1, b2)]
    weights, N = accum_weights(metas)
    assert N == 1279 + 976 + 1802 and metas[0][3] == 2 * 16 * 2 and metas[1][3] == 16 * 3
    seen = {}
    res = eng.train_step_accum([b1, b2], lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    psd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    total, ce_o, vq_o = 0.0, 0.0, 0.0
    for (x, c, g, lengths), (wc, wv) in zip((b1, b2), weights):
        xin = torch.nn.functional.one_hot(x.cpu().long(), cfg["O"]).float().transpose(1, 2).contiguous()
        y, vq, _, _ = O.vqvae_forward(psd, ocfg, xin, c.cpu(), g.cpu())
        ce = O.masked_ce_loss(y, x.cpu().long().unsqueeze(-1), lengths)
        total = total + wc * ce + wv * vq
        ce_o, vq_o = ce_o + wc * float(ce.detach()), vq_o + wv * float(vq.detach())
    total.backward()
    print(f"ce {float(res['ce'])} (oracle {ce_o}), vq_loss {float(res['vq_loss'])} (oracle {vq_o})")
    assert abs(float(res["ce"]) - ce_o) < 1e-4 and abs(float(res["vq_loss"]) - vq_o) < 1e-5
    lay, grads, bad = eng.lay, seen["g"].cpu(), {}
    for k, v in psd.items():
        ref = v.grad if v.grad is not None else torch.zeros_like(v)
        got = grads[lay.off(k):lay.off(k) + lay.numel(k)].view(lay.shapes[k])
        if float(ref.abs().max()) == 0:
            assert float(got.abs().max()) == 0, k
            continue
        e = rel_err(got, ref)
        if not e < 2e-3:
            bad[k] = e
    assert not bad, bad


# ---------------------------------------------------------------- 5. nothing left behind
def _state(eng):
    return dict(params=eng.params.clone(), exp_avg=eng.exp_avg.clone(), exp_avg_sq=eng.exp_avg_sq.clone(), shadow=eng.shadow.clone(),
                opt_step=eng.opt_step)


def _fresh_from(cfg, sd, dtype, state):
    eng = _engine(cfg, sd, dtype)
    for k in ("params", "exp_avg", "exp_avg_sq", "shadow"):
        getattr(eng, k).copy_(state[k])
    eng.opt_step = state["opt_step"]
    eng.weights_dirty = True
    return eng


def _step_x(eng, batch):
    seen = {}
    x, c, g, lengths = batch
    res = eng.train_step(x, c, g, lengths=lengths, lr=LR, grad_hook=lambda gr: seen.__setitem__("g", gr.clone()))
    torch.cuda.synchronize()
    return _numbers(res), seen["g"].cpu(), eng.params.cpu().clone()


@pytest.mark.parametrize("how", ["applied", "discarded", "interleaved"])
def test_a_window_leaves_nothing_behind(how):
    """A window (applied; dropped by discard_step; applied with an eval forward and a decode_list of one short clip between its
    micro-batches), then train_step(X): against a fresh engine that loaded the state behind the window and ran train_step(X)."""
    dtype = "bf16"
    cfg, sd = golden_model("A")[:2]
    win, X = _batch_a(), _batch_a(B=2, T=1280, lengths=(1280, 1111), speakers=(1, 2), seed=23)
    parts = _parts(win, [2, 2])
    eng = _engine(cfg, sd, dtype)
    if how == "discarded":
        before = _state(eng)
        eng.accumulate(*parts[0], ce_weight=0.5, vq_weight=0.5)
        eng.discard_step()
        assert eng.window is None and eng.opt_step == 0 and float(eng.cbuf.abs().max()) == 0 and float(eng.d_eff.abs().max()) == 0
        state = before
    else:
        if how == "interleaved":
            x0, c0, g0, l0 = parts[0]
            eng.accumulate(x0, c0, g0, l0, ce_weight=0.5, vq_weight=0.5)
            acc = (eng.cbuf.clone(), eng.d_eff.clone())
            ev = eng.forward(x0, c0, g0, targets=x0, lengths=l0, want_logits=False, train=False)
            dec = eng.decode_list([dict(T=640, c=ev["quant"][0, :, :1].contiguous(), gid=1, init_idx=31)], mode="argmax")
            assert dec[0]["idx"].shape == (640,) and torch.isfinite(ev["loss"])
            assert eng.window is not None and eng.window.n == 1
            assert torch.equal(acc[0], eng.cbuf) and torch.equal(acc[1], eng.d_eff)        # the window is intact
            eng.accumulate(*parts[1], ce_weight=0.5, vq_weight=0.5)
            res = eng.apply_step(lr=LR)
            assert res["micro_batches"] == 2
        else:
            eng.train_step_accum(parts, lr=LR)
        assert eng.window is None and eng.opt_step == 1
        state = _state(eng)
    got = _step_x(eng, X)
    ref = _step_x(_fresh_from(cfg, sd, dtype, state), X)
    _close(got, ref, dtype, how)


# ---------------------------------------------------------------- 6. data parallel hand-over at world 1
def test_apply_step_with_grad_sync_at_world_one():
    from wavenet_autoencoders_amd.distributed import GradSync
    dtype = "bf16"
    cfg, sd = golden_model("A")[:2]
    parts = _parts(_batch_a(), [1, 3])
    out = {}
    for with_sync in (False, True):
        eng = _engine(cfg, sd, dtype)
        sync = GradSync(eng) if with_sync else None
        for p in parts:
            eng.accumulate(*p, ce_weight=0.5, vq_weight=0.5)
            if sync is not None:
                assert not any(sync.launched) and sync.n_collectives == 0 and not sync.handles     # nothing goes out inside a micro-batch
        res = eng.apply_step(lr=LR, grad_sync=sync)
        torch.cuda.synchronize()
        if sync is not None:
            assert not any(sync.launched) and not sync.handles          # finish() ran and reset the bucketer
        out[with_sync] = (_numbers(res), eng.grads.cpu().clone(), eng.params.cpu().clone())
        del eng
        torch.cuda.empty_cache()
    _close(out[True], out[False], dtype, "grad_sync")


# ---------------------------------------------------------------- 7. refusals
def test_refusals_come_before_any_launch():
    cfg, sd = golden_model("A")[:2]
    eng = _engine(cfg, sd, "fp32")
    x, c, g, lengths = _batch_a()
    with pytest.raises(RuntimeError, match="accumulate"):
        eng.apply_step()
    assert eng.opt_step == 0
    eng.accumulate(x[:2], c[:2], g[:2], lengths[:2], ce_weight=0.5, vq_weight=0.5)
    torch.cuda.synchronize()
    snap = (eng.cbuf.clone(), eng.d_eff.clone(), eng.gn_acc.clone(), eng.params.clone(), eng.window.sums.clone())
    calls = [lambda: eng.train_step(x, c, g, lengths=lengths),
             lambda: eng.forward(x, c, g, targets=x, lengths=lengths, want_logits=False, train=True),
             lambda: eng.decoder_forward(x, torch.zeros(4, 16, 2).cuda(), g, targets=x, train=True),
             lambda: eng.backward(x[:2], g[:2], x[:2], lengths[:2]),
             lambda: eng.load_state_dict(sd),
             lambda: setattr(eng, "weights_dirty", True),
             lambda: eng.train_step_accum([(x, c, g, lengths)])]
    for i, call in enumerate(calls):
        with pytest.raises(RuntimeError, match=r"apply_step\(\).*discard_step\(\)"):
            call()
        torch.cuda.synchronize()
        assert eng.window is not None and eng.window.n == 1 and eng.opt_step == 0 and not eng.weights_dirty, i
        for a, b in zip(snap, (eng.cbuf, eng.d_eff, eng.gn_acc, eng.params, eng.window.sums)):
            assert torch.equal(a, b), i
    # the window still closes
    eng.accumulate(x[2:], c[2:], g[2:], lengths[2:], ce_weight=0.5, vq_weight=0.5)
    res = eng.apply_step(lr=LR)
    assert res["micro_batches"] == 2 and eng.opt_step == 1 and eng.window is None and np.isfinite(float(res["loss"]))


# ---------------------------------------------------------------- 8. the training script
def test_train_script_with_accum_steps(tmp_path):
    """vqwae_train.py --accum-steps 2 for two optimizer steps on the synthetic dump of tests/test_gpu_scripts.py: global_step == 2,
    four batches consumed, a checkpoint that reloads."""
    from test_gpu_scripts import HP
    rng = np.random.default_rng(5)
    dump = tmp_path / "dump"
    lines = []
    for u in range(3):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 40 + 4 * u
        np.save(d / "wave.npy", rng.integers(0, 256, n * 160).astype(np.int16))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    preset = os.path.join(ROOT, "hps", "vqwae.json")
    ck = tmp_path / "ck"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(ck),
                        "--preset", preset, "--hparams", HP + ",train_eval_interval=1000", "--max-steps", "2", "--dtype", "fp32",
                        "--accum-steps", "2"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "Finished" in p.stdout and "step 1 loss" in p.stdout
    assert "2 optimizer steps of 2 micro-batches: 4 batches consumed" in p.stdout
    saved = torch.load(ck / "checkpoint_latest.pth", map_location="cpu")
    assert saved["global_step"] == 2
    from wavenet_autoencoders_amd.checkpoint import load_checkpoint
    hp = json.load(open(ck / "hparams.json"))
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    geom = Geometry(layers=hp["layers"], stacks=hp["stacks"], R=hp["residual_channels"], G=hp["gate_channels"], S=hp["skip_out_channels"],
                    O=hp["out_channels"], Cc=hp["cin_channels"], Cg=hp["gin_channels"], k=hp["kernel_size"], n_speakers=hp["n_speakers"],
                    upsample_scales=list(hp["upsample_params"]["upsample_scales"]), cin_pad=hp["cin_pad"], use_speaker_embedding=True,
                    c_in=hp["dim_in"], encoder_hid=hp["encoder_hid"], K=256)
    eng = WaeEngine(geom, dtype="fp32")
    step, _, _ = load_checkpoint(str(ck / "checkpoint_latest.pth"), eng, reset_optimizer=False)
    assert step == 2 and eng.opt_step == 2 and bool(torch.isfinite(eng.params).all())
