"""The fixed-order forms of the small float sums of a train step (include/wae.h: wae_upsample_stage_bwd_det, wae_vq_slice_bwd_det /
wae_vq_bwd_det, wae_vq_loss_det, wae_gproj_bwd_det, wae_clip_adam_ema_det), each called on its own through the C ABI at the smallest
shapes that reach its edges: more workgroups than one, a ragged last block, two clips of one speaker, a code no frame uses.

Integer-valued operands: bit for bit against the float64 references of tests/frontend_ref.py (or, where that file has none, against the
default entry, which is exact on such operands in any order).  Gaussian operands: the bound the default kernel's own test uses
(tests/test_gpu_frontend_bwd.py: (n + 4) 2^-24 A holds for a round-to-nearest fp32 sum of n terms in ANY order), and three runs
from the same prefill that must agree in every bit."""
import ctypes

import numpy as np
import pytest
import torch

import frontend_ref as R
import test_gpu_frontend_bwd as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL = -1


def _three_equal(run, what):
    a = run()
    for i in (1, 2):
        b = run()
        for x, y in zip(a, b):          # (bit patterns: an untouched NaN prefill equals itself)
            assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), \
                f"{what}: run {i} gave other bits than run 0"
    return a


# ================================================================================================ wae_upsample_stage_bwd_det
#          s, Tin, B, C: 320 rows on 256 blocks (a block walks two rows), 256 rows, 3 rows (three blocks), the generic template
UP_CASES = [(4, 513, 5, 64), (5, 257, 5, 64), (8, 256, 2, 128), (4, 1, 1, 3), (16, 257, 5, 64), (3, 256, 5, 64)]


def _run_up(case, seed, gauss, short=0):
    L, lib = F._lib()
    s, Tin, B, C = case
    rng = np.random.RandomState(seed)
    draw = F._gauss if gauss else F._ints
    inp, w, dout = draw(rng, B, C, Tin), draw(rng, 2 * s + 1), draw(rng, B, C, Tin * s)
    pre = F._prefill(rng, 2 * s + 1)
    need = lib.wae_upsample_stage_bwd_det_floats()
    ins = [F._dev(dout), F._dev(inp), F._dev(w)]

    def run():
        din, dw = F.Guarded(F._nan(B, C, Tin)), F.Guarded(pre)
        parts = F.Guarded(torch.full((need,), float("nan")))      # a partial that is read before it is stored shows as NaN
        rc = lib.wae_upsample_stage_bwd_det(*[L.ptr(t) for t in ins], L.ptr(din.t), L.ptr(dw.t), L.ptr(parts.t), need - short, B, C,
                                            Tin, s, None)
        torch.cuda.synchronize()
        parts.result()
        return rc, din.result(), dw.result()
    if short:
        rc, din, dw = run()
        assert rc == EINVAL and bool(torch.isnan(din).all()) and torch.equal(dw, pre)
        return
    rc, din, dw = run()
    L.check(rc, "upsample_stage_bwd_det")
    ref = R.upsample_stage_grads(inp, w, dout, s)
    A = R.upsample_stage_grads(inp.abs(), w.abs(), dout.abs(), s)
    for name, got, want, a, n in (("din", din, ref[0], A[0], s * (2 * s + 1)),
                                  ("dw", dw, pre.double() + ref[1], pre.abs().double() + A[1], B * C * Tin * s + 1)):
        if gauss:
            F._assert_bound(got, want, a, n, name, "wae_upsample_stage_bwd_det")
        else:
            F._assert_exact(got, want, a, name)
    if gauss:
        _three_equal(lambda: run()[1:], "upsample_stage_bwd_det")


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "s%d-T%d-B%dC%d" % c)
def test_upsample_stage_bwd_det_exact(case):
    _run_up(case, 2000 + UP_CASES.index(case), gauss=False)


@pytest.mark.parametrize("case", [(4, 513, 5, 64), (16, 257, 5, 64)], ids=lambda c: "s%d-T%d-B%dC%d" % c)
def test_upsample_stage_bwd_det_rounding_and_repeats(case):
    _run_up(case, 78, gauss=True)


def test_upsample_stage_bwd_det_refuses_a_short_buffer():
    _run_up((4, 1, 1, 3), 5, gauss=False, short=1)


# ============================================================================================ wae_vq_slice_bwd_det, wae_vq_bwd_det
def _run_vq(B, Dtot, d0, D, Tq, K, idx, c_lat, c_emb, seed, gauss, whole=None):
    L, lib = F._lib()
    rng = np.random.RandomState(seed)
    draw = F._gauss if gauss else F._ints
    lat, quant, dq = draw(rng, B, Dtot, Tq), draw(rng, B, Dtot, Tq), draw(rng, B, Dtot, Tq)
    out = torch.ones(Dtot, dtype=torch.bool)
    out[d0:d0 + D] = False
    lat[:, out] += 1000.0
    quant[:, out] -= 1000.0
    ref = R.vq_slice_bwd(lat, quant, idx, dq, d0, D, K, c_lat, c_emb)
    A = [a.abs() for a in R.vq_slice_bwd(lat.abs(), -quant.abs(), idx, dq.abs(), d0, D, K, c_lat, c_emb)]
    pre = F._prefill(rng, K, D)
    ins = [F._dev(lat), F._dev(quant), F._dev(idx), F._dev(dq)]

    def run():
        dlat, demb = F.Guarded(F._nan(B, Dtot, Tq)), F.Guarded(pre)
        args = [L.ptr(t) for t in ins] + [L.ptr(dlat.t), L.ptr(demb.t)]
        if whole is None:
            L.check(lib.wae_vq_slice_bwd_det(*args, B, Dtot, d0, D, Tq, K, c_lat, c_emb, None), "vq_slice_bwd_det")
        else:
            L.check(lib.wae_vq_bwd_det(*args, B, D, Tq, K, whole[0], whole[1], None), "vq_bwd_det")
        torch.cuda.synchronize()
        return dlat.result(), demb.result()
    got, demb = run()
    assert bool(torch.isnan(got[:, out]).all()), "dlat outside the slice was written"
    counts = torch.bincount(idx, minlength=K).double()
    unused = counts == 0
    assert bool(unused.any()) and torch.equal(demb[unused], pre[unused])          # a code no frame uses keeps its prefill
    quantum = min(1.0, c_lat, c_emb)
    for name, g, want, a, n in (("dlat", got[:, d0:d0 + D], ref[0], A[0], 3),
                                ("demb", demb, pre.double() + ref[1], pre.abs().double() + A[1], (2 * counts + 1)[:, None])):
        if gauss:
            F._assert_bound(g, want, a, n, name, "wae_vq_bwd_det")
        else:
            F._assert_exact(g, want, a / quantum, name)
    if gauss:
        _three_equal(run, "vq_bwd_det")


@pytest.mark.parametrize("case", ["slice", "one_code", "two_blocks"])
def test_vq_slice_bwd_det_exact(case):
    """channels [3, 8) of 12, c_lat = 1/2 and c_emb = 2: exact.  B Tq = 111 frames (one ragged block of the owner's walk), or 3 * 100 = 300
    (two blocks, the second ragged); codes 6..8 of the 9 stay unused; `one_code`: every frame names code 4"""
    B, Dtot, d0, D, K = 3, 12, 3, 5, 9
    Tq = 100 if case == "two_blocks" else 37
    rng = np.random.RandomState(31)
    idx = torch.full((B * Tq,), 4, dtype=torch.int64) if case == "one_code" else torch.from_numpy(rng.randint(0, 6, size=B * Tq))
    _run_vq(B, Dtot, d0, D, Tq, K, idx, 0.5, 2.0, 3000, gauss=False)


def test_vq_bwd_det_exact():
    B, D, Tq, K = 2, 16, 32, 8
    idx = torch.from_numpy(np.random.RandomState(32).randint(0, K - 1, size=B * Tq))
    c_lat, c_emb = R.vq_bwd_coefficients(B, D, Tq, 0.25, 1.0)
    _run_vq(B, D, 0, D, Tq, K, idx, c_lat, c_emb, 3100, gauss=False, whole=(0.25, 1.0))


def test_vq_bwd_det_rounding_and_repeats():
    B, D, Tq, K = 3, 64, 137, 32
    idx = torch.from_numpy(np.random.RandomState(33).randint(0, K - 1, size=B * Tq))
    c_lat, c_emb = R.vq_bwd_coefficients(B, D, Tq, 0.25, 1024.0)
    _run_vq(B, D, 0, D, Tq, K, idx, c_lat, c_emb, 3200, gauss=True, whole=(0.25, 1024.0))


# ================================================================================================================ wae_vq_loss_det
@pytest.mark.parametrize("gauss", [False, True], ids=["ints", "gauss"])
@pytest.mark.parametrize("B,Dtot,d0,D,Tq", [(3, 12, 3, 5, 37), (2, 64, 0, 64, 300), (1, 4, 1, 2, 1)])
def test_vq_loss_det(B, Dtot, d0, D, Tq, gauss):
    """stats[0] = c_loss * (fp32(sum) / (fp32(B Tq) * fp32(D))) with the sum of (quant - lat)^2 over the slice in float64: on integers the
    sum is exact and the three fp32 operations are restated here bit for bit; on Gaussian operands the fp64 sum is rounded once, so the
    value is within 2^-23 of the float64 expression (one rounding of the sum, one of the quotient, one of the product: 3 * 2^-24 < 2^-22);
    stats[1] keeps what it held."""
    L, lib = F._lib()
    rng = np.random.RandomState(9)
    draw = F._gauss if gauss else F._ints
    lat, quant = draw(rng, B, Dtot, Tq), draw(rng, B, Dtot, Tq)
    c_loss = 1.25
    s64 = float(((quant[:, d0:d0 + D].double() - lat[:, d0:d0 + D].double()) ** 2).sum())
    ins = [F._dev(lat), F._dev(quant)]

    def run():
        stats = F.Guarded(torch.tensor([float("nan"), 7.0]))
        L.check(lib.wae_vq_loss_det(L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(stats.t), B, Dtot, d0, D, Tq, c_loss, None), "vq_loss_det")
        torch.cuda.synchronize()
        return (stats.result(),)
    (st,) = _three_equal(run, "vq_loss_det")
    assert float(st[1]) == 7.0
    if gauss:
        want = c_loss * s64 / (B * Tq * D)
        assert abs(float(st[0]) - want) <= 2.0 ** -22 * abs(want), (float(st[0]), want)
    else:
        want = np.float32(c_loss) * (np.float32(s64) / (np.float32(B * Tq) * np.float32(D)))
        assert float(st[0]) == float(want), (float(st[0]), float(want))


# ============================================================================================================== wae_gproj_bwd_det
def _gproj_problem(rng, gauss, B, gid):
    """two layers of G = 40 gate channels in Hp = 32 (64 tile rows: two row blocks, the second ragged -- rows 52..63 are padding),
    Cg = 8 features, five speakers; c1 (L, 2Hp, ld) with the per-clip columns at 7"""
    Lr, G, Hp, Cg, nspk, ones = 2, 40, 32, 8, 5, 7
    stride, wg_off, bias_off, emb_off = 2000, 0, 400, 4000
    draw = F._gauss if gauss else F._ints
    eff = draw(rng, emb_off + nspk * Cg + 16)
    c1 = draw(rng, Lr, 2 * Hp, ones + B + 3)
    pre = F._prefill(rng, eff.numel())
    return dict(L=Lr, G=G, Hp=Hp, Cg=Cg, nspk=nspk, ones=ones, stride=stride, wg_off=wg_off, bias_off=bias_off, emb_off=emb_off, eff=eff,
                c1=c1, pre=pre, B=B, gid=torch.tensor(gid, dtype=torch.int32))


def _gproj_call(p, det, consume):
    L, lib = F._lib()
    eff, gid = F._dev(p["eff"]), F._dev(p["gid"])
    d_eff, c1 = F.Guarded(p["pre"]), F.Guarded(p["c1"])
    ld = p["c1"].shape[-1]
    args = (L.ptr(eff), L.ptr(d_eff.t), p["wg_off"], p["bias_off"], p["stride"], L.ptr(gid), p["emb_off"], None, L.ptr(c1.t),
            2 * p["Hp"] * ld, ld, p["ones"], p["B"], p["L"], p["G"], p["Hp"], p["Cg"], p["nspk"])
    if det:
        need = lib.wae_gproj_bwd_det_floats(p["B"], p["L"], p["Hp"], p["Cg"])
        assert need == p["L"] * 2 * p["B"] * p["Cg"]
        parts = F.Guarded(torch.full((need,), float("nan")))
        L.check(lib.wae_gproj_bwd_det(*args, consume, L.ptr(parts.t), need, None), "gproj_bwd_det")
        torch.cuda.synchronize()
        parts.result()
    else:
        L.check((lib.wae_gproj_bwd_consume if consume else lib.wae_gproj_bwd)(*args, None), "gproj_bwd")
        torch.cuda.synchronize()
    return d_eff.result(), c1.result()


def _emb_ref(p):
    """the embedding rows in float64: row gid[b] += sum_l sum_{gate channel} c1[l][row(channel)][ones + b] * Wg[l][channel][:]"""
    H, Hp, Cg = p["G"] // 2, p["Hp"], p["Cg"]
    out = torch.zeros(p["nspk"], Cg, dtype=torch.float64)
    for b, sp in enumerate(p["gid"].tolist()):
        for l in range(p["L"]):
            wg = p["eff"][p["wg_off"] + l * p["stride"]:][:p["G"] * Cg].view(p["G"], Cg).double()
            rows = torch.cat([torch.arange(H), Hp + torch.arange(H)])        # tile row of gate channel ch = half * H + i
            out[sp] += p["c1"][l, rows, p["ones"] + b].double() @ wg
    return out


@pytest.mark.parametrize("consume", [0, 1])
def test_gproj_bwd_det_exact(consume):
    """three clips, two of speaker 2: integer operands -- d_eff bit for bit the default entry's (every sum exact in any order), its
    embedding rows the float64 restatement; consume = 1 zeroes exactly the per-clip columns"""
    p = _gproj_problem(np.random.RandomState(41), False, 3, [2, 4, 2])
    d_det, c_det = _gproj_call(p, True, consume)
    d_def, c_def = _gproj_call(p, False, consume)
    assert torch.equal(d_det, d_def) and torch.equal(c_det, c_def)
    emb = d_det[p["emb_off"]:p["emb_off"] + p["nspk"] * p["Cg"]].view(p["nspk"], p["Cg"])
    pre = p["pre"][p["emb_off"]:p["emb_off"] + p["nspk"] * p["Cg"]].view(p["nspk"], p["Cg"])
    assert torch.equal(emb, (pre.double() + _emb_ref(p)).float())
    assert torch.equal(emb[[0, 1, 3]], pre[[0, 1, 3]])            # speakers without a clip keep their prefill
    want_c = p["c1"].clone()
    if consume:
        want_c[:, :, p["ones"]:p["ones"] + p["B"]] = 0.0
    assert torch.equal(c_det, want_c)


def test_gproj_bwd_det_repeats_and_is_close():
    """Gaussian operands, 35 clips (two launches of 32 and 3) over five speakers: three runs equal; the embedding rows within
    (n + 4) 2^-24 A of float64, n = the terms of a row's sum"""
    rng = np.random.RandomState(42)
    gid = rng.randint(0, 5, size=35).tolist()
    p = _gproj_problem(rng, True, 35, gid)
    d_det, _ = _three_equal(lambda: _gproj_call(p, True, 0), "gproj_bwd_det")
    sl = slice(p["emb_off"], p["emb_off"] + p["nspk"] * p["Cg"])
    pa = dict(p, eff=p["eff"].abs(), c1=p["c1"].abs())
    n = torch.bincount(torch.tensor(gid), minlength=p["nspk"]).double()[:, None] * (p["L"] * p["G"]) + 1
    F._assert_bound(d_det[sl].view(p["nspk"], p["Cg"]), p["pre"][sl].view(p["nspk"], p["Cg"]).double() + _emb_ref(p),
                    p["pre"][sl].view(p["nspk"], p["Cg"]).abs().double() + _emb_ref(pa), n, "embedding rows", "wae_gproj_bwd_det")
    d_def, _ = _gproj_call(p, False, 0)
    rest = torch.ones(d_det.numel(), dtype=torch.bool)
    rest[sl] = False
    assert torch.equal(d_det[rest], d_def[rest])        # conv bias and conv1x1g rows: one owner in both forms, the same statements


def test_gproj_bwd_det_refuses_a_short_buffer():
    L, lib = F._lib()
    p = _gproj_problem(np.random.RandomState(43), False, 3, [2, 4, 2])
    ptr = ctypes.c_void_p(0x1000)
    need = lib.wae_gproj_bwd_det_floats(3, 2, 32, 8)
    rc = lib.wae_gproj_bwd_det(ptr, ptr, 0, 400, 2000, ptr, 4000, None, ptr, 64 * 13, 13, 7, 3, 2, 40, 32, 8, 5, 0, ptr, need - 1, None)
    assert rc == EINVAL and b"partials buffer" in lib.wae_last_error()


# ========================================================================================================== wae_clip_adam_ema_det
@pytest.mark.parametrize("n", [5, 1024 * 3 + 5, 1024 * 1024 + 3001])
def test_clip_adam_ema_det(n):
    """integer gradients (the sum of squares is exact in fp64 in any order): norm, parameters, both moments and the shadow bit for bit
    wae_clip_adam_ema's, over one workgroup, several with a ragged tail, and more than the 1024 the grid stops at.  Gaussian gradients:
    three runs equal, the norm within 2^-22 of float64 (an fp64 sum of fp32 squares, then one square root and one rounding to fp32)."""
    L, lib = F._lib()
    rng = np.random.RandomState(n % 1000)
    state = [F._gauss(rng, n) for _ in range(2)] + [F._gauss(rng, n).abs()]          # params, exp_avg, exp_avg_sq

    def run(grads, det):
        p, m, v = (F._dev(t.clone()) for t in state)
        sh, g = p.clone(), F._dev(grads)
        norm = torch.zeros(1, device=DEV)
        tail = (3, 4e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.9999, None)
        if det:
            parts = F.Guarded(torch.full((1025,), float("nan")), dtype=torch.float64)
            L.check(lib.wae_clip_adam_ema_det(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(sh), n, L.ptr(parts.t), 1025, L.ptr(norm), *tail),
                    "clip_adam_ema_det")
            torch.cuda.synchronize()
            parts.result()
        else:
            scratch = torch.zeros(1, dtype=torch.float64, device=DEV)
            L.check(lib.wae_clip_adam_ema(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(sh), n, L.ptr(scratch), L.ptr(norm), *tail),
                    "clip_adam_ema")
            torch.cuda.synchronize()
        return [t.cpu() for t in (norm, p, m, v, sh)]
    ints = F._ints(rng, n)
    a, b = run(ints, True), run(ints, False)
    assert float(a[0]) == float(np.float32(np.sqrt(float((ints.double() ** 2).sum()))))
    for x, y, name in zip(a, b, ("norm", "params", "exp_avg", "exp_avg_sq", "shadow")):
        assert torch.equal(x, y), name
    gs = F._gauss(rng, n)
    got = _three_equal(lambda: run(gs, True), "clip_adam_ema_det")
    want = float(np.sqrt(float((gs.double() ** 2).sum())))
    assert abs(float(got[0]) - want) <= 2.0 ** -22 * want


def test_clip_adam_ema_det_refuses_a_short_buffer():
    L, lib = F._lib()
    ptr = ctypes.c_void_p(0x1000)
    rc = lib.wae_clip_adam_ema_det(ptr, ptr, ptr, ptr, ptr, 100, ptr, 1024, ptr, 1, 4e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.9999, None)
    assert rc == EINVAL
