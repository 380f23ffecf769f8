"""The gather pass that finishes a step's gradients (csrc/grad_finish.hip, EngineOptions.grad_finish) against the split launches it
replaces -- scatter into d_eff, weight-norm backward, a pass over the arena for the norm -- ON THE SAME WEIGHT-GRADIENT TILES.

The tiles are fp32 atomic sums of the weight-gradient launch: two runs of a step differ in their last bits whatever finishes them
(tests/test_gpu_backward.py compares such runs at 1e-4).  So the yardstick runs on the engine state the gather pass has just read:
after a train step with the switch on (lr = 0), the test scatters the same tiles into d_eff (whose slots the gather pass leaves at
zero), runs wae_weight_norm_bwd_range over the layer segment and wae_clip_adam_ema over the arena, and compares
    grads       bit for bit (every slot has one contributing tile element: _build_finish_plan refuses anything else),
    grad_norm   to 1e-9 relative (the same fp32 squares summed in double in another order: n * 2^-53, n ~ 1e7; the norm is rounded
                to fp32 once, so this asks for the same float).
A second engine runs the whole step with the switch off: every tensor's gradient to the tolerance of two runs of the atomic sums --
the wiring of the switch (streams, joins, the rows left to gproj_bwd and the row-sum scatter) rather than the arithmetic."""
import numpy as np
import pytest
import torch

from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

_UP = dict(O=256, Cc=64, Cg=16, n_speakers=5, upsample_scales=[4, 4], cin_pad=0)
GEOMETRIES = {
    # padded gate rows (H = 184 -> 192: map entries < 0), three taps
    "k3_padded": (dict(layers=3, stacks=1, R=64, G=368, S=64, k=3, **_UP), False, 512),
    # two taps: another tap stride, a row length that is no multiple of 3
    "k2": (dict(layers=3, stacks=1, R=64, G=256, S=64, k=2, **_UP), False, 512),
    # C2's row of 256 x 3 floats
    "c2_rows": (dict(layers=2, stacks=1, R=256, G=368, S=256, k=3, **_UP), False, 512),
    # C5's row of 512 x 3 floats: beyond the 1024 floats of the vector path, so the scalar path of the kernel with a pattern
    "c5_rows": (dict(layers=2, stacks=1, R=512, G=512, S=512, k=3, **_UP), False, 512),
    # the encoder in front (C3 cut to two layers): the arena outside the layer segment (encoder, codebook, upsampling network) is
    # finished from d_eff by the `outer` rows of the same kernel, which add its share of the norm
    "encoder": (None, True, 2560),
}


def _case(name):
    import bench
    cfg, enc, T = GEOMETRIES[name]
    B = 2
    if enc:
        conf = dict(bench.CONFIGS["c3"], B=B, T=T)
        conf["cfg"] = dict(conf["cfg"], layers=2, stacks=2)
        sd = O.make_state_dict(dict(conf["cfg"]), salt=conf["salt"], with_encoder=True)
        x, c, g = bench.synth_inputs(0, torch.device("cuda:0"), conf)
        return conf["cfg"], sd, x, c, g
    hop = int(np.prod(cfg["upsample_scales"]))
    sd = O.make_state_dict(dict(cfg), salt=11, with_encoder=False)
    gen = torch.Generator().manual_seed(4242)
    x = torch.randint(0, cfg["O"], (B, T), generator=gen).cuda()
    c = torch.randn(B, cfg["Cc"], T // hop, generator=gen).cuda()
    g = torch.randint(0, cfg["n_speakers"], (B,), generator=gen).cuda()
    return cfg, sd, x, c, g


def _engine(cfg, sd, dtype, on):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.opt.grad_finish = on
    eng.load_state_dict(sd, strict=False)
    eng.init_optimizer()
    return eng


def _plan(eng):
    plans = [p for p in getattr(eng, "_finish_plans", {}).values() if p is not None]
    assert len(plans) == 1, "the gather pass did not serve this step"
    return plans[0]


def _split_launches_on_the_same_tiles(eng, B, T):
    """grads and grad_norm of the split launches from the tiles and d_eff slots the last step left behind"""
    from wavenet_autoencoders_amd import _lib as L
    from wavenet_autoencoders_amd import backward as BW
    cx = BW._step(eng, B, T)
    jobs = BW._scatter_jobs(cx, 0, eng.g.layers, True, which="tiles")
    L.check(eng.lib.wae_unpack_scatter_add_multi(jobs, len(jobs), eng.stream()), "scatter")
    lo, hi = BW.layer_segment(eng)
    for a, b in ((0, lo), (lo, hi), (hi, eng.lay.total)):       # (outside the segment d_eff holds what the gather pass read)
        if b > a:
            BW._wn_bwd_range(eng, a, b)
    L.check(eng.lib.wae_clip_adam_ema(L.ptr(eng.params), L.ptr(eng.grads), L.ptr(eng.exp_avg), L.ptr(eng.exp_avg_sq), L.ptr(eng.shadow),
                                      eng.lay.total, L.ptr(eng.opt_scratch), L.ptr(eng.grad_norm), eng.opt_step, 0.0, 0.9, 0.999, 1e-8,
                                      0.0, 100.0, 0.9999, eng.stream()), "clip_adam_ema")
    torch.cuda.synchronize()
    return eng.grads.clone(), float(eng.grad_norm[0])


def _unequal(lay, a, b):
    return [k for k in lay.offsets if not torch.equal(a[lay.off(k):lay.off(k) + lay.numel(k)], b[lay.off(k):lay.off(k) + lay.numel(k)])]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_gather_pass_is_the_split_launches(name, dtype):
    from wavenet_autoencoders_amd import backward as BW
    cfg, sd, x, c, g = _case(name)
    B, T = x.shape
    eng = _engine(cfg, sd, dtype, True)
    params0 = eng.params.clone()
    r1 = eng.train_step(x, c, g, lr=0.0)
    n1 = float(r1["grad_norm"])
    torch.cuda.synchronize()
    plan, (lo, hi), mid = _plan(eng), BW.layer_segment(eng), BW.layer_segment_mid(eng)
    assert plan.tile_off.size > 0 and plan.rest_off.size > 0 and plan.outer_off.size > 0
    assert torch.equal(eng.params, params0)
    g_on = eng.grads.clone()
    assert np.isfinite(n1) and n1 > 0 and float(g_on[lo:hi].abs().max()) > 0

    # ---- range calls: [lo, mid) and [mid, hi) against one call over [lo, hi), from the same tiles and d_eff slots
    acc = {}
    for cuts in ((lo, hi), (lo, mid, hi)):
        eng.grads[lo:hi].zero_()
        eng.gn_acc.zero_()
        for a, b in zip(cuts[:-1], cuts[1:]):       # (the two launches per range that _finish_layers enqueues, here on one stream)
            BW._finish_rows(eng, plan, a, b, "tile", True)
            BW._finish_rows(eng, plan, a, b, "rest", True)
        torch.cuda.synchronize()
        assert not _unequal(eng.lay, eng.grads, g_on), cuts
        acc[len(cuts)] = float(eng.gn_acc[0])
    print(f"{name} {dtype}: sum of squares over the segment: one call {acc[2]!r}, two calls {acc[3]!r}")
    assert acc[2] > 0 and abs(acc[2] - acc[3]) <= 2e-9 * acc[2]     # (of the squares: twice the norm's bound)

    # ---- the split launches on the same tiles
    g_off, n_off = _split_launches_on_the_same_tiles(eng, B, T)
    print(f"{name} {dtype}: grad_norm gather pass {n1!r}, split launches {n_off!r}")
    assert not _unequal(eng.lay, g_on, g_off)
    assert abs(n1 - n_off) <= 1e-9 * n_off

    # ---- the whole step with the switch off, on an engine of its own (other atomic sums: two-run tolerance)
    ref = _engine(cfg, sd, dtype, False)
    r0 = ref.train_step(x, c, g, lr=0.0)
    torch.cuda.synchronize()
    assert not getattr(ref, "_finish_plans", {})
    bad = {}
    for k in eng.lay.offsets:
        a, b = (t[eng.lay.off(k):eng.lay.off(k) + eng.lay.numel(k)] for t in (ref.grads, g_on))
        err, scale = float((a - b).abs().max()), float(a.abs().max())
        if err > 1e-4 * max(scale, 1e-6) + 1e-7:
            bad[k] = (err, scale)
    assert not bad, bad
    assert abs(float(r0["grad_norm"]) - n1) <= 1e-4 * n1
    assert float(r0["loss"]) == float(r1["loss"])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_steps_give_the_same_norm(dtype):
    """lr = 0: the second step sees the first step's weights and inputs.  An accumulator that is not cleared, or cleared in the wrong
    place, doubles (or loses) the layer segment's share of the norm: a factor of ~1.4 (or ~0.1).

    Two consecutive steps do NOT give the same float on either path: the weight-gradient tiles are fp32 atomic sums, nearly every
    gradient tensor differs in its last bits from step to step, and the split launches' own grad_norm of four consecutive steps of
    this case (bf16) read 0.15001560747623444, ...444, 0.15001562237739563, ...444 -- one fp32 ulp apart.  So the second step's norm
    is asked to be EXACTLY the split launches' norm of the second step's own tiles (same values, a deterministic yardstick), and to
    agree with the first step's within the two-run tolerance of the atomic sums that the suite uses for gradients (1e-4)."""
    cfg, sd, x, c, g = _case("k3_padded")
    B, T = x.shape
    eng = _engine(cfg, sd, dtype, True)
    norms = []
    for _ in range(2):
        norms.append(float(eng.train_step(x, c, g, lr=0.0)["grad_norm"]))
    torch.cuda.synchronize()
    _plan(eng)
    _, n_off = _split_launches_on_the_same_tiles(eng, B, T)
    print(f"{dtype}: grad_norm of two consecutive steps {norms!r}, split launches on the second step's tiles {n_off!r}")
    assert norms[1] == n_off
    assert abs(norms[1] - norms[0]) <= 1e-4 * norms[0]
