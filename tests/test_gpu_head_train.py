"""The training head in one launch (csrc/head_train.hip: wae_head_train_from_h0) against the launches it replaces --
wae_head_fwd_from_h0, wae_masked_mean, wae_head_bwd -- on the same buffers, and against a float64 restatement on the CPU.

Shapes are the smallest at which the kernel can go wrong, not the workload's: B = 2; T = 31 (one partial wave), 256 (an exact tile),
300 (a tile with one partial and six empty waves), 513 (three tiles); (Sp, Op, O) = (256, 256, 256), (256, 256, 250), (128, 128, 100).

  nll, lse, h1      bit for bit wae_head_fwd_from_h0's (the same statements in the same order);
  loss              wae_masked_mean of the same nll, or the fp32 value next to it (double sums in another order); three launches in a
                    row give the same bits (the counter resets itself); one case with a single workgroup;
  dy, dh1, dskip    e = max|out - ref| / max|ref| against float64 from the same stored h0 / weights / biases, for the fused launch and
                    for the two launches.  Both add the same products in another k order (the fused kernel's dy operand comes from the
                    accumulators, head_bwd's GEMM a reads stored rows), so they are not bitwise equal; the bound is
                    e_fused <= e_two_launch + half a unit of storage rounding at the tensor's maximum (2^-9 bf16, 2^-12 fp16): one
                    flipped rounding;
  poison            a NaN guard band behind every output stays NaN, rows < T are finite, rows with weight 0 (beyond len - 1, and
                    t = T - 1) have dy exactly 0.
Step level (tests/helpers.py's model A: Sp = Op = 128): a train step with the fused head against one with EngineOptions.head_fused off."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

GEOMS = {"256": (256, 256), "250": (256, 250), "100": (128, 100)}         # S, O  (Sp = Op = S)
TS = [31, 256, 300, 513]
B = 2
GUARD = 256          # poisoned rows behind every output
HALF_ULP = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12}
_engines = {}


def _engine(geom, dtype):
    """An engine whose head weights are this test's: zero-mean W1 and W3 (about half of h1 = relu(b1 + W1 h0) is zero for a
    non-negative h0), logits of a few units"""
    key = (geom, dtype)
    if key not in _engines:
        from wavenet_autoencoders_amd import Geometry
        from wavenet_autoencoders_amd import backward as BW
        from wavenet_autoencoders_amd.engine import WaeEngine
        S, Ocls = GEOMS[geom]
        cfg = dict(layers=2, stacks=1, R=64, G=128, S=S, O=Ocls, k=3, Cc=64, Cg=16, n_speakers=5, upsample_scales=[4, 4], cin_pad=0)
        sd = O.make_state_dict(dict(cfg), salt=5, with_encoder=False)
        gen = torch.Generator().manual_seed(1000 + S + Ocls)
        for name, rows, scale in (("wavenet.last_conv_layers.1", S, 1.4 / math.sqrt(S)), ("wavenet.last_conv_layers.3", Ocls, 2.5 / math.sqrt(S))):
            v = torch.randn(rows, S, 1, generator=gen)
            sd[name + ".weight_v"] = v
            sd[name + ".weight_g"] = v.flatten(1).norm(dim=1).view(rows, 1, 1) * scale         # effective weight = scale * v
            sd[name + ".bias"] = 0.1 * torch.randn(rows, generator=gen)
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
        eng.load_state_dict(sd, strict=False)
        eng.prepare_weights()
        BW.pack_bwd_weights(eng)
        torch.cuda.synchronize()
        g, lay = eng.g, eng.lay
        assert (g.Sp, g.Op, g.O) == (S, S, Ocls) and eng.split_head and not eng.wide_head
        eff = eng.eff.float().cpu()
        o1, o3 = lay.off("wavenet.last_conv_layers.1.weight_v"), lay.off("wavenet.last_conv_layers.3.weight_v")
        stored = lambda w: w.to(eng.tdtype).double()        # noqa: E731  (the packed streams hold the weights in the storage dtype)
        bh = eng.b_head.cpu().double()
        ref = dict(W1=stored(eff[o1:o1 + S * S].view(S, S)), W3=stored(eff[o3:o3 + Ocls * S].view(Ocls, S)), b1=bh[S:2 * S], b3=bh[2 * S:2 * S + Ocls])
        _engines[key] = (eng, ref)
    return _engines[key]


def _h0(eng, T, seed, nb=B):
    """(nb, T, Sp) in the storage dtype: about half zeros, the rest |N(0, 1)|"""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(nb, T, eng.g.Sp, generator=gen).abs() * (torch.rand(nb, T, eng.g.Sp, generator=gen) < 0.5)
    return v.to(eng.tdtype).cuda()


def _reference(ref, h0, tgt, lens, factor, scale, T, Ocls):
    """float64 on the CPU from the stored h0, weights and biases -> h1, dy, dh1, dskip (B, T, S / O) and the weight of every step"""
    x = h0.cpu().double()
    h1 = torch.relu(x @ ref["W1"].T + ref["b1"])
    y = h1 @ ref["W3"].T + ref["b3"]
    p = torch.softmax(y, dim=-1)
    onehot = torch.zeros_like(p)
    nxt = torch.roll(tgt.cpu().long(), -1, dims=1)
    onehot.scatter_(2, nxt.unsqueeze(-1), 1.0)
    t = torch.arange(T).view(1, T)
    w = ((t < (lens.view(B, 1).clamp(max=T) - 1)) & (t + 1 < T)).double() * factor
    dy = (p - onehot) * w.unsqueeze(-1)
    dh1 = (dy @ ref["W3"]) * (h1 > 0)
    dskip = (dh1 @ ref["W1"]) * (x > 0) * scale
    return h1, dy, dh1, dskip, w


class _Bufs:
    """One set of outputs with a NaN guard band behind each"""

    def __init__(self, eng, T, nb=B):
        S = eng.g.Sp
        self.nb, self.rows = nb, nb * T
        mk = lambda cols, dt: torch.full(((self.rows + GUARD) * cols,), float("nan"), dtype=dt, device="cuda")      # noqa: E731
        self.nll, self.lse = mk(1, torch.float32), mk(1, torch.float32)
        self.h1, self.dy, self.dh1, self.dskip = (mk(S, eng.tdtype) for _ in range(4))
        self.loss = torch.full((2 + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.S = S

    def view(self, name):
        t = getattr(self, name)
        cols = 1 if name in ("nll", "lse") else self.S
        return t[:self.rows * cols].view(self.nb, -1, cols) if cols > 1 else t[:self.rows].view(self.nb, -1)

    def guards_untouched(self):
        for name in ("nll", "lse", "h1", "dy", "dh1", "dskip"):
            cols = 1 if name in ("nll", "lse") else self.S
            if not bool(torch.isnan(getattr(self, name)[self.rows * cols:].float()).all()):
                return name
        return None if bool(torch.isnan(self.loss[2:]).all()) else "loss"


def _launch_fused(eng, h0, tgt, ln, factor, T, out, red):
    from wavenet_autoencoders_amd import _lib as L
    g = eng.g
    hd = L.HeadDesc(eng.dt, out.nb, T, g.Ku, g.Sp, g.Op, g.O, math.sqrt(1.0 / g.layers))
    tail = eng.w_head.data_ptr() + (g.Ku // 64) * (g.Sp // 32) * 4096
    L.check(eng.lib.wae_head_train_from_h0(ctypes.byref(hd), L.ptr(h0), ctypes.c_void_p(tail), L.ptr(eng.w_hb), L.ptr(eng.b_head), L.ptr(tgt),
                                           L.ptr(ln), factor, L.ptr(out.nll), L.ptr(out.lse), L.ptr(out.h1), L.ptr(out.dy), L.ptr(out.dh1),
                                           L.ptr(out.dskip), L.ptr(red), L.ptr(out.loss), eng.stream()), "head_train")


def _launch_two(eng, h0, tgt, ln, factor, T, out):
    from wavenet_autoencoders_amd import _lib as L
    g = eng.g
    hd = L.HeadDesc(eng.dt, out.nb, T, g.Ku, g.Sp, g.Op, g.O, math.sqrt(1.0 / g.layers))
    tail = eng.w_head.data_ptr() + (g.Ku // 64) * (g.Sp // 32) * 4096
    L.check(eng.lib.wae_head_fwd_from_h0(ctypes.byref(hd), L.ptr(h0), ctypes.c_void_p(tail), L.ptr(eng.b_head), None, L.ptr(tgt), L.ptr(out.nll),
                                         L.ptr(out.lse), L.ptr(out.h1), eng.stream()), "head_fwd_from_h0")
    L.check(eng.lib.wae_masked_mean(L.ptr(out.nll), L.ptr(ln), L.ptr(out.loss), out.nb, T, eng.stream()), "masked_mean")
    b3 = ctypes.c_void_p(eng.b_head.data_ptr() + 2 * g.Sp * 4)
    L.check(eng.lib.wae_head_bwd(ctypes.byref(hd), L.ptr(h0), L.ptr(out.h1), L.ptr(eng.w_hb), b3, L.ptr(out.lse), L.ptr(tgt), L.ptr(ln), factor, None,
                                 L.ptr(out.dy), L.ptr(out.dh1), L.ptr(out.dskip), eng.stream()), "head_bwd")


def _red(eng, T, nb=B):
    from wavenet_autoencoders_amd import _lib as L
    g = eng.g
    hd = L.HeadDesc(eng.dt, nb, T, g.Ku, g.Sp, g.Op, g.O, 1.0)
    return torch.zeros(int(eng.lib.wae_head_train_ws_bytes(ctypes.byref(hd))), dtype=torch.uint8, device="cuda")


def _adjacent(a, b):
    """two fp32 values: equal or neighbours"""
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, b) == b


def _cases(T, Ocls, seed):
    """(name, lengths | None, targets): random targets under every mask, and the last class everywhere"""
    gen = torch.Generator().manual_seed(seed)
    rnd = torch.randint(0, Ocls, (B, T), generator=gen, dtype=torch.int32)
    out = [("all", None, rnd), ("T,0", [T, 0], rnd), ("1,T-7", [1, T - 7], rnd), ("T/2,T", [T // 2, T], rnd),
           ("last class", None, torch.full((B, T), Ocls - 1, dtype=torch.int32))]
    return out


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_fused_launch_against_the_two_launches_and_float64(geom, dtype, T):
    eng, ref = _engine(geom, dtype)
    S, Ocls = GEOMS[geom]
    scale = math.sqrt(1.0 / eng.g.layers)
    h0 = _h0(eng, T, 7 * T + S)
    red = _red(eng, T)
    for name, lens, tgt in _cases(T, Ocls, T + Ocls):
        lens_t = torch.tensor(lens if lens is not None else [T] * B)
        count = int(torch.clamp(lens_t.clamp(max=T) - 1, min=0).sum())
        factor = (4096.0 if dtype == "fp16" else 1.0) / max(count, 1)
        ln = lens_t.to(torch.int32).cuda() if lens is not None else None
        tg = tgt.cuda()
        h1r, dyr, dh1r, dskr, w = _reference(ref, h0, tgt, lens_t, factor, scale, T, Ocls)
        # the masks are exercised: about half of h0 and of h1 is zero
        z0, z1 = float((h0.cpu().float() == 0).float().mean()), float((h1r == 0).double().mean())
        assert 0.3 <= z0 <= 0.7 and 0.3 <= z1 <= 0.7, (z0, z1)

        fu, two = _Bufs(eng, T), _Bufs(eng, T)
        _launch_fused(eng, h0, tg, ln, factor, T, fu, red)
        _launch_two(eng, h0, tg, ln, factor, T, two)
        torch.cuda.synchronize()
        tag = f"{geom} {dtype} T={T} {name}"
        # ---- poison: nothing behind the outputs, everything in front of it
        assert fu.guards_untouched() is None, (tag, fu.guards_untouched())
        for k in ("nll", "lse", "h1", "dy", "dh1", "dskip"):
            assert bool(torch.isfinite(fu.view(k).float()).all()), (tag, k)
        # ---- the forward's outputs: bit for bit
        for k in ("nll", "lse", "h1"):
            assert torch.equal(fu.view(k), two.view(k)), (tag, k)
        # ---- the loss: wae_masked_mean's value or its neighbour
        lf, lt = fu.loss[:2].cpu().numpy(), two.loss[:2].cpu().numpy()
        assert lf[1] == lt[1] == count, (tag, lf, lt)
        assert _adjacent(lf[0], lt[0]), (tag, lf[0], lt[0])
        # ---- rows without weight: dy exactly 0
        dead = (w == 0).cuda()
        assert bool((fu.view("dy")[dead].float() == 0).all()), tag
        # ---- dy, dh1, dskip against float64, no worse than the two launches by more than one flipped rounding
        for k, r, cols in (("dy", dyr, Ocls), ("dh1", dh1r, S), ("dskip", dskr, S)):
            a, b = fu.view(k).cpu().double(), two.view(k).cpu().double()
            assert bool((a[..., cols:] == 0).all()), (tag, k, "pad columns")
            top = float(r.abs().max())
            e_f, e_t = float((a[..., :cols] - r).abs().max()) / top, float((b[..., :cols] - r).abs().max()) / top
            print(f"{tag} {k}: e_fused {e_f:.3e} e_two_launch {e_t:.3e}")
            assert e_f <= e_t + HALF_ULP[dtype], (tag, k, e_f, e_t)


@pytest.mark.parametrize("Bc,T", [(2, 513), (1, 31)])
def test_loss_repeats_bit_for_bit(Bc, T):
    """Three launches in a row on one reduction workspace: the counter resets itself, and the partials are summed in index order
    whichever workgroup arrives last.  (1, 31): a single workgroup."""
    eng, _ = _engine("250", "bf16")
    h0 = _h0(eng, T, 99, Bc)
    tg = torch.randint(0, 250, (Bc, T), generator=torch.Generator().manual_seed(5), dtype=torch.int32).cuda()
    ln = torch.tensor([T - 3] * Bc, dtype=torch.int32).cuda()
    red = _red(eng, T, Bc)
    got = []
    for _ in range(3):
        out = _Bufs(eng, T, Bc)
        _launch_fused(eng, h0, tg, ln, 1.0 / (Bc * (T - 4)), T, out, red)
        torch.cuda.synchronize()
        got.append((out.loss[:2].cpu(), out.dy.cpu()))
        assert int(red[:4].view(torch.int32)[0]) == 0
    two = _Bufs(eng, T, Bc)
    _launch_two(eng, h0, tg, ln, 1.0 / (Bc * (T - 4)), T, two)
    torch.cuda.synchronize()
    for lo, dy in got[1:]:
        assert torch.equal(lo, got[0][0]) and torch.equal(dy.view(torch.int16), got[0][1].view(torch.int16))
    assert float(got[0][0][1]) == Bc * (T - 4) and _adjacent(float(got[0][0][0]), float(two.loss[0]))


def _step_engine(cfg, sd, fused):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="bf16")
    eng.opt.head_fused = fused
    eng.load_state_dict(sd)
    eng.init_optimizer()
    return eng


def test_train_step_with_and_without_the_fused_head():
    """One train step from the same state with the switch on and off: the loss equal or adjacent, every gradient tensor within the
    bf16 criterion of DESIGN section 4 (max|a - b| / max|b| <= 5e-2).  The fused step's saved record says that the head's backward is
    done; a decoder_forward(train=True) + backward pair outside a step still runs wae_head_bwd (no record)."""
    from helpers import golden_model
    cfg, sd, inp, _, _ = golden_model("A")
    x, c, g = inp["x"].cuda().to(torch.int32), inp["c"].cuda(), inp["g"].cuda()
    on, off = _step_engine(cfg, sd, True), _step_engine(cfg, sd, False)
    assert (on.g.Sp, on.g.Op) == (128, 128)
    r_on, r_off = on.train_step(x, c, g, lr=0.0), off.train_step(x, c, g, lr=0.0)
    torch.cuda.synchronize()
    assert on.saved.head_done is not None and on.saved.head_done.factor == 1.0 / (x.shape[0] * (x.shape[1] - 1))
    assert off.saved.head_done is None
    assert _adjacent(float(r_on["ce"]), float(r_off["ce"])), (float(r_on["ce"]), float(r_off["ce"]))
    bad = {}
    for k in on.lay.offsets:
        a, b = (t[on.lay.off(k):on.lay.off(k) + on.lay.numel(k)] for t in (on.grads, off.grads))
        err, top = float((a - b).abs().max()), float(b.abs().max())
        if err > 5e-2 * top + 1e-12:
            bad[k] = (err, top)
    assert not bad, bad
    assert abs(float(r_on["grad_norm"]) - float(r_off["grad_norm"])) <= 5e-2 * float(r_off["grad_norm"])

    # outside a step nobody announces a factor: the forward runs its own launches and the backward runs wae_head_bwd
    out = on.forward(x, c, g, targets=x, want_logits=False, train=True)
    assert on.saved.head_done is None and on.flight.head_factor is None
    on.backward(x, g, x, None)
    torch.cuda.synchronize()
    assert _adjacent(float(out["loss"]), float(r_off["ce"]))
    bad = {}
    for k in on.lay.offsets:
        a, b = (t[on.lay.off(k):on.lay.off(k) + on.lay.numel(k)] for t in (on.grads, off.grads))
        err, top = float((a - b).abs().max()), float(b.abs().max())
        if err > 1e-4 * top + 1e-7:          # (the same launches as the engine without the switch: the two-run tolerance of the atomic sums)
            bad[k] = (err, top)
    assert not bad, bad
