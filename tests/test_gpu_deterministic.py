"""The reproducible train step (WAE_DETERMINISTIC=1; options.py): two engines built from the same state take the same
steps and must agree in every bit -- the losses, every element of the gradients, the norm, and the parameters, both Adam moments and
the EMA shadow after the update -- for class-id and scalar-input decoders, with and without encoder, VQ and speaker ids, with dropout,
over ragged lengths, in fp32, bf16 and fp16, for train_step and for an accumulation window.  A fixed-order form that still hides a sum
in arrival order fails here (the default mode does: its weight gradients alone differ from run to run in every tensor).

Against the default mode the gradients are the tile launch's up to the order of fp32 additions (2e-4 of a tensor's range: the figure of
test_gpu_backward.test_stream_weight_gradients_match_per_layer_tiles for the same operands summed in another order), and in fp32 the
step passes the assertions of test_gpu_backward.test_full_train_step_against_golden."""
import json

import pytest
import torch

from helpers import golden_model, load_npz, rel_err

pytestmark = pytest.mark.gpu

LR = 2e-3
STATE = ("grads", "params", "exp_avg", "exp_avg_sq", "shadow", "grad_norm")


def _engine(cfg, sd, dtype, dropout=0.0):
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


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if not torch.equal(a[k], b[k]):
            d = (a[k].double() - b[k].double()).abs()
            raise AssertionError(f"{what}: {k} differs between the two engines in {int((a[k] != b[k]).sum())} of {a[k].numel()} elements "
                                 f"(largest difference {float(d.max()):.3e})")


def _batch_a(B, T, lengths, speakers, seed):
    cfg = golden_model("A")[0]
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(0, cfg["O"], (B, T), generator=gen)
    c = torch.randn(B, cfg["c_in"], T // 160, generator=gen)
    return x.cuda(), c.cuda(), torch.tensor(speakers).cuda(), torch.tensor(lengths)


def _case(name):
    """-> (cfg, sd, (x, c, g, lengths), dropout)"""
    if name in ("A", "A-dropout"):
        cfg, sd, ins, _, _ = golden_model("A")
        T = ins["x"].shape[1]
        return cfg, sd, (ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda(), torch.tensor([T, T - 137])), 0.05 if name == "A-dropout" else 0.0
    if name == "B":
        cfg, sd, ins, _, _ = golden_model("B")
        T = ins["x"].shape[1]
        return cfg, sd, (ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda(), torch.tensor([T, T - 137])), 0.0
    if name == "S":         # scalar input: the geometry of test_gpu_backward.test_scalar_input_train_step_runs_and_learns
        cfg, sd, ins, _, _ = golden_model("S")
        return cfg, sd, (ins["x"][:, 0, :].contiguous().cuda(), ins["c"].cuda(), ins["g"].cuda(), None), 0.0
    assert name == "A-ragged"      # B = 5 on model A's weights, seeded random inputs: ragged lengths, two clips of one speaker
    cfg, sd, _, _, _ = golden_model("A")
    T = 1280
    return cfg, sd, _batch_a(5, T, (T, T - 1, 801, 640, 333), (3, 0, 3, 1, 4), seed=5), 0.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["A", "B", "A-dropout", "S", "A-ragged"])
def test_train_step_repeats_bitwise(name, dtype, monkeypatch):
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, (x, c, g, lengths), dropout = _case(name)
    engs = [_engine(cfg, sd, dtype, dropout) for _ in range(2)]
    assert all(e.opt.deterministic and not e.opt.tn_stream and not e.opt.side and e.opt.chains == "1" for e in engs)
    for step in range(3):
        snaps = [_snapshot(e, e.train_step(x, c, g, lengths=lengths, lr=LR)) for e in engs]
        _same(snaps[0], snaps[1], f"{name} {dtype} step {step}")
        assert all(bool(torch.isfinite(v.double()).all()) for v in snaps[0].values()), f"{name} {dtype} step {step}: not finite"


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_accum_window_repeats_bitwise(dtype, monkeypatch):
    """train_step_accum on three micro-batches of different shapes, twice (two engines), then once more on the updated weights"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, _, _, _ = golden_model("A")
    parts = [_batch_a(2, 1280, (1280, 977), (2, 0), seed=17), _batch_a(1, 1920, (1803,), (4,), seed=18),
             _batch_a(3, 640, (640, 500, 333), (1, 1, 3), seed=19)]
    engs = [_engine(cfg, sd, dtype) for _ in range(2)]
    for step in range(2):
        snaps = [_snapshot(e, e.train_step_accum(parts, lr=LR)) for e in engs]
        _same(snaps[0], snaps[1], f"window {dtype} step {step}")


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_ragged_splits_repeat_bitwise(dtype, monkeypatch):
    """B = 5, T = 1000 with model A's weights and seeded random inputs: the time splits of the tile launches are ragged (1000 is no
    multiple of a split's 32-row slabs).  T = 1000 is no multiple of the 640 samples the encoder and the upsampling network make of a
    latent frame, so the decoder runs on upsampled conditioning (as test_gpu_backward.test_static_weight_gradient_launch_at_odd_shapes
    does): decoder_forward(train=True) + decoder_backward + finish_grads, twice -- the loss and every gradient."""
    from wavenet_autoencoders_amd import backward as BW
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, _, _, _ = golden_model("A")
    B, T = 5, 1000
    gen = torch.Generator().manual_seed(1000)
    x = torch.randint(0, cfg["O"], (B, T), generator=gen).cuda()
    c_up = torch.randn(B, cfg["Cc"], T, generator=gen).cuda()
    g = torch.tensor([3, 0, 3, 1, 4]).cuda()
    ln = torch.tensor([T, T - 1, 801, 640, 333])
    got = []
    for _ in range(2):
        eng = _engine(cfg, sd, dtype)
        out = eng.decoder_forward(x, c_up, g, targets=x, lengths=ln.cuda(), train=True, c_is_upsampled=True, want_logits=False)
        BW.decoder_backward(eng, x, x, ln, g)
        grads = BW.finish_grads(eng).clone()
        torch.cuda.synchronize()
        got.append((out["loss"].clone(), grads))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][1].abs().max()) > 0


def test_backward_alone_repeats_bitwise(monkeypatch):
    """forward(train=True) + backward() without the optimizer, bf16: eng.grads of two engines"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, (x, c, g, lengths), _ = _case("A")
    got = []
    for _ in range(2):
        eng = _engine(cfg, sd, "bf16")
        eng.forward(x, c, g, targets=x, lengths=lengths, want_logits=False, train=True)
        got.append(eng.backward(x, g, x, lengths).clone())
        torch.cuda.synchronize()
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_deterministic_gradients_are_the_tile_paths(dtype, monkeypatch):
    """against WAE_TN_STREAM=0 without the mode, model A: every gradient tensor within 2e-4 max|g| + 1e-7"""
    cfg, sd, (x, c, g, lengths), _ = _case("A")
    got = {}
    for mode in ("det", "tiles"):
        monkeypatch.setenv("WAE_TN_STREAM", "0")
        monkeypatch.setenv("WAE_DETERMINISTIC", "1" if mode == "det" else "0")
        eng = _engine(cfg, sd, dtype)
        assert eng.opt.deterministic == (mode == "det")
        eng.train_step(x, c, g, lengths=lengths, lr=LR)
        torch.cuda.synchronize()
        got[mode] = eng.grads.clone()
    lay, bad = eng.lay, {}
    for k in lay.offsets:
        a = got["tiles"][lay.off(k):lay.off(k) + lay.numel(k)]
        b = got["det"][lay.off(k):lay.off(k) + lay.numel(k)]
        err, ref = float((a - b).abs().max()), float(a.abs().max())
        if err > 2e-4 * ref + 1e-7:
            bad[k] = (err, ref)
    assert not bad, bad


def test_deterministic_train_step_against_golden(monkeypatch):
    """fp32: the assertions of test_gpu_backward.test_full_train_step_against_golden, with that test's tolerances, under the mode"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, ins, zm, ocfg = golden_model("A")
    z = load_npz("train_A")
    eng = _engine(cfg, sd, "fp32")
    x, c, g = ins["x"].cuda(), ins["c"].cuda(), ins["g"].cuda()
    T = x.shape[1]
    res = eng.train_step(x, c, g, lengths=torch.tensor([T, T]), lr=4e-4, clip_thresh=100.0, ema_decay=0.9999)
    torch.cuda.synchronize()
    assert abs(float(res["loss"]) - float(z["loss"])) < 1e-4
    assert abs(float(res["vq_loss"]) - float(z["vq_loss"])) < 1e-5
    assert abs(float(res["grad_norm"]) - float(z["grad_norm"])) < 1e-3 * float(z["grad_norm"])
    gsq = json.loads(str(z["grad_sq_by_key"]))
    lay, bad = eng.lay, {}
    for k, want in gsq.items():
        got = float((eng.grads[lay.off(k):lay.off(k) + lay.numel(k)].double() ** 2).sum())
        if abs(got - want) > 5e-3 * max(want, 1e-12) + 1e-14:
            bad[k] = (got, want)
    assert not bad, bad
    for key in [k[5:] for k in z if k.startswith("grad:")]:
        view = lambda a: a[lay.off(key):lay.off(key) + lay.numel(key)].view(lay.shapes[key]).cpu()  # noqa: E731
        assert rel_err(view(eng.grads), z["grad:" + key]) < 2e-3, key
        assert rel_err(view(eng.params), z["new:" + key]) < 5e-5, key
        assert rel_err(view(eng.shadow), z["ema:" + key]) < 1e-6, key


def test_grad_sync_is_refused(monkeypatch):
    """NotImplementedError before any launch: the engine has prepared nothing and saved nothing when it raises"""
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    cfg, sd, (x, c, g, lengths), _ = _case("B")
    eng = _engine(cfg, sd, "bf16")

    class Sync:
        world = 2

        def __getattr__(self, name):
            raise AssertionError(f"grad_sync.{name} was reached")

    for call in (lambda: eng.train_step(x, c, g, lengths=lengths, grad_sync=Sync()),
                 lambda: eng.train_step_accum([(x, c, g, lengths)], grad_sync=Sync()),
                 lambda: eng.backward(x, g, x, lengths, grad_sync=Sync())):
        with pytest.raises(NotImplementedError, match="deterministic"):
            call()
    assert eng.saved is None and eng.exp_avg is None and eng.window is None
    eng.train_step(x, c, g, lengths=lengths, grad_hook=lambda gr: None)       # grad_hook is allowed
    torch.cuda.synchronize()


_DIGEST = """
import hashlib, sys, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_deterministic as T
print("digest", T.digest_after_two_steps())
"""


def digest_after_two_steps():
    """model A, bf16, two train steps -> sha256 over the gradients, the updated state, the norm and the losses"""
    import hashlib
    cfg, sd, (x, c, g, lengths), _ = _case("A")
    eng = _engine(cfg, sd, "bf16")
    for _ in range(2):
        res = eng.train_step(x, c, g, lengths=lengths, lr=LR)
    h = hashlib.sha256()
    for t in list(_snapshot(eng, res).values()):
        h.update(t.cpu().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_a_fresh_process_gives_the_same_bits(monkeypatch):
    """the same two steps in this process and in ONE fresh child process (the test is about the process: nothing of the result may
    depend on addresses, on what ran before, or on the allocator's state)"""
    import os
    import subprocess
    import sys
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    here = os.path.dirname(os.path.abspath(__file__))
    torch.empty(3 << 20, device="cuda")            # (this process's allocator is not in a fresh state)
    mine = digest_after_two_steps()
    p = subprocess.run([sys.executable, "-c", _DIGEST.format(tests=here, root=os.path.dirname(here))], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert p.returncode == 0, p.stderr[-2000:]
    theirs = [l.split()[1] for l in p.stdout.splitlines() if l.startswith("digest ")]
    assert theirs == [mine]


@pytest.mark.parametrize("kind", ["VectorQuantize", "SlicedVectorQuantize", "SlicedVectorQuantizeEMA", "VectorQuantizeEMA"])
def test_quantiser_modules_repeat_bitwise(kind, monkeypatch):
    """the drop-in quantisers run without an engine and follow the switch on their own: forward (train mode, so the EMA ones move their
    codebooks) + backward of loss + sum(quant * w), three times from the same state: vq_loss, perplexity, quant, the input gradient, the
    codebook gradients and the EMA buffers bit for bit (3 x 397 frames: more waves add to the loss than one)"""
    import copy
    from wavenet_autoencoders_amd import vector_quantization as VQ
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    gen = torch.Generator().manual_seed(7)
    x0 = (torch.randn(3, 16, 397, generator=gen) * 0.05).cuda()
    w = torch.randn(3, 16, 397, generator=gen).cuda()
    torch.manual_seed(11)
    proto = getattr(VQ, kind)(24, 16).cuda().train()
    runs = []
    for _ in range(3):
        m = copy.deepcopy(proto)
        x = x0.clone().requires_grad_(True)
        quant, loss, perp = m(x)
        (loss + (quant * w).sum()).backward()
        torch.cuda.synchronize()
        out = [quant.detach(), loss.detach(), perp.detach(), x.grad] + [b.clone() for b in m.buffers()]
        out += [p.grad if p.grad is not None else p.detach().clone() for p in m.parameters()]
        runs.append(out)
    for r in runs[1:]:
        assert len(r) == len(runs[0])
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
