"""tests/tn_ref.py (the float64 restatement of the weight-gradient contraction) against torch.autograd, and the exactness
precondition of every launch of tests/test_gpu_tn_kernels.py -- all on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tn_cases as C
import tn_ref as R
from wavenet_autoencoders_amd import packing as P


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max()) / scale
    assert err <= 1e-12, f"{what}: relative error {err}"


@pytest.mark.parametrize("cond", (0, 1))
@pytest.mark.parametrize("T", (7, 37))
@pytest.mark.parametrize("d", (1, 2, 5))
@pytest.mark.parametrize("k", (2, 3))
def test_layer_contractions_match_autograd(k, d, T, cond):
    """the records of packing.tn_layer_contractions, evaluated by the reference, are autograd's dW1 per tap, dWc, the per-clip sums
    of dz, dW_out and its bias on a ResidualConv1dGLU-shaped layer (modules.py:115-163) in float64"""
    torch.manual_seed(100 * k + 10 * d + T + cond)
    B, Rr, H, Cc, S, alpha = 2, 5, 3, 4, 6, 0.5
    g = P.Geometry(layers=1, stacks=1, R=Rr, G=2 * H, S=S, O=8, Cc=Cc if cond else -1, k=k, dilations_override=[d])
    Rp, Hp, Ccp = g.Rp, g.Hp, g.Ccp
    f64 = dict(dtype=torch.float64)
    x, c = torch.randn(B, Rr, T, **f64), torch.randn(B, Cc, T, **f64)
    W1, b1 = torch.randn(2 * H, Rr, k, **f64).requires_grad_(), torch.randn(2 * H, **f64).requires_grad_()
    Wc = torch.randn(2 * H, Cc, 1, **f64).requires_grad_()
    Wo, bo = torch.randn(Rr, H, 1, **f64).requires_grad_(), torch.randn(Rr, **f64).requires_grad_()
    Ws, bs = torch.randn(S, H, 1, **f64).requires_grad_(), torch.randn(S, **f64).requires_grad_()
    z = F.conv1d(F.pad(x, ((k - 1) * d, 0)), W1, b1, dilation=d)
    if cond:
        z = z + F.conv1d(c, Wc)
    z.retain_grad()
    u = torch.tanh(z[:, :H]) * torch.sigmoid(z[:, H:])
    out, skip = F.conv1d(u, Wo, bo), F.conv1d(u, Ws, bs)
    Gout, Gs = torch.randn_like(out), torch.randn_like(skip)
    ((out * Gout).sum() + (skip * Gs).sum()).backward()

    def tm(a, width, rows=None):        # (B, C, T) -> time-major (B, T, width), channel ch in column rows[ch]
        o = torch.zeros(B, T, width, **f64)
        o[:, :, list(rows if rows is not None else range(a.shape[1]))] = a.detach().transpose(1, 2)
        return o

    gate = list(range(H)) + [Hp + h for h in range(H)]          # where the test puts the 2H gate channels among the 2Hp columns
    DZ, X, CU, GN, U, C1, CO = 1 << 8, 2 << 8, 3 << 8, 4 << 8, 5 << 8, 1 << 20, 1 << 30      # stand-ins for device addresses
    arrays = {DZ: tm(z.grad, 2 * Hp, gate), X: tm(x, Rp), CU: tm(c, max(Ccp, 64)), GN: tm(Gout, Rp), U: tm(u, g.Ku)}
    ld1, ldo = k * Rp + Ccp + 64, Hp + 64
    tiles = {C1: torch.zeros(2 * Hp, ld1, **f64), CO: torch.zeros(Rp, ldo, **f64)}
    recs = list(P.tn_layer_contractions(g, d, alpha, DZ, 2 * Hp, X, CU if cond else 0, GN, U, C1, ld1, CO, ldo))
    assert len(recs) == k + cond + 1
    for M, N, shift, ones, a, pa, ps, qa, qs, ca, ldc in recs:
        assert arrays[pa].shape[2] == ps and arrays[qa].shape[2] == qs
        base = CO if ca >= CO else C1
        col0 = (ca - base) // 4
        assert (ca - base) % 4 == 0 and col0 < ldc == tiles[base].shape[1]
        o = R.tn_reference(R.TnSpec(B, T, M, N, shift, a, ones), arrays[pa], arrays[qa])["C"]
        tiles[base][:M, col0:col0 + o.update.shape[1]] += o.update
    c1, co = tiles[C1], tiles[CO]
    for tap in range(k):
        _close(c1[gate, tap * Rp:tap * Rp + Rr], alpha * W1.grad[:, :, tap], f"dW1 tap {tap}")
    zb0 = k * Rp + Ccp
    if cond:
        _close(c1[gate, k * Rp:k * Rp + Cc], alpha * Wc.grad[:, :, 0], "dWc")
    _close(c1[gate, zb0:zb0 + B], alpha * z.grad.sum(2).t(), "per-clip sums of dz")
    _close(c1[gate, zb0:zb0 + B].sum(1), alpha * b1.grad, "conv bias")
    _close(co[:Rr, :H], alpha * Wo.grad[:, :, 0], "dW_out")
    _close(co[:Rr, Hp:Hp + B].sum(1), alpha * bo.grad, "out bias")
    # nothing lands outside the weights' own rows and columns (the padded operand columns are zeros)
    assert float(c1.abs().sum()) > 0 and not bool(c1[[i for i in range(2 * Hp) if i not in gate]].any())
    assert not bool(co[Rr:].any()) and not bool(co[:, H:Hp].any())


@pytest.mark.parametrize("m0", (0, 128))
def test_onehot_form_matches_one_hot_matmul(m0):
    rng = np.random.RandomState(m0 + 1)
    B, T, n, classes = 3, 41, 24, 300
    ids = torch.from_numpy(rng.randint(-1, classes, size=(B, T)).astype(np.int32))
    ids[0, 0], ids[1, 3] = -1, m0 + 5
    dx0 = torch.from_numpy(rng.randn(B, T, n + 8))
    oh = F.one_hot(ids.long().clamp(min=0), classes).double() * (ids >= 0).double().unsqueeze(-1)
    for shift in (0, -3):
        want = torch.einsum("btc,btn->cn", oh[:, -shift:], dx0[:, :T + shift, 8:8 + n])
        o = R.tn_reference(R.TnSpec(B, T, 128, n, shift, -2.0, q_col=8, m0=m0), None, dx0, ids)["C"]
        _close(o.update, -2.0 * want[m0:m0 + 128], f"one-hot, m0 {m0}, shift {shift}")
        assert torch.equal(o.A, 2.0 * torch.einsum("btc,btn->cn", oh[:, -shift:], dx0[:, :T + shift, 8:8 + n].abs())[m0:m0 + 128])


def test_ones_columns_and_row_weights():
    """clip b's sums land in column ones_col + b; a row multiplicity scales that row's terms; |terms| and their count follow"""
    rng = np.random.RandomState(7)
    B, T = 3, 5
    Pa, Qa = torch.from_numpy(rng.randn(B, T, 20)), torch.from_numpy(rng.randn(B, T, 12))
    w = torch.tensor([[1, 1, 0, 0, 2]] * B, dtype=torch.float64)
    sp = R.TnSpec(B, T, 9, 4, 0, 0.5, ones_col=6, p_col=8, q_col=8)
    o = R.tn_reference(sp, Pa, Qa, rows=w)["C"]
    Pm, Qm = Pa[:, :, 8:17], Qa[:, :, 8:12]
    _close(o.update[:, :4], 0.5 * torch.einsum("bt,btm,btn->mn", w, Pm, Qm), "data columns")
    _close(o.update[:, 6:9], 0.5 * torch.einsum("bt,btm->mb", w, Pm), "ones columns")
    assert not bool(o.update[:, 4:6].any()) and o.update.shape == (9, 9)
    assert float(o.n[0, 0]) == 12 and float(o.n[0, 6]) == 4 and bool((o.A >= o.update.abs() - 1e-12).all())
    cb = R.tn_reference(R.TnSpec(B, T, 9, 4, 0, -2.0, p_col=8, q_col=8, n1_valid=3, q1_col=1, want_cb=True), Pa, Qa, None, Qa)
    _close(cb["Cb"].update, -2.0 * Qm.sum((0, 1)), "column sums")
    _close(cb["C1"].update, -2.0 * torch.einsum("btm,btn->mn", Pm, Qa[:, :, 1:4]), "second Q operand")


LISTS = dict(tiles=C.tile_cases, stream=C.stream_cases, taps=lambda: C.static_cases("TAPS"), cond=lambda: C.static_cases("COND"),
             outskip=lambda: C.static_cases("OUTSKIP"), group=lambda: C.static_cases("GROUP"),
             cross=lambda: [l for k in C.CROSS for l in C.cross_launches(k)])


@pytest.mark.parametrize("which", sorted(LISTS))
def test_gpu_cases_stay_exact_and_inside_the_entries_limits(which):
    """every exact GPU case: sum of |terms| below 2^22 with the integer operands, and the shapes the headers permit"""
    launches = LISTS[which]()
    assert len({l.name for l in launches}) == len(launches) >= 3
    for l in launches:
        prob = C.build_problem(l)
        assert C.max_A(prob) < C.EXACT_LIMIT, l.name
        spc = (l.T + 31) // 32
        for j in l.jobs:
            assert j.shift <= 0 and (j.ones < 0 or j.shift == 0) and (not j.cb or j.shift == 0), l.name
            if l.entry == "tiles":
                assert 1 <= j.m <= 128 and 0 <= j.n <= 128 and (j.ones < 0 or j.ones + l.B <= 128), l.name
                continue
            assert j.m % 8 == 0 and j.n % 8 == 0 and j.n1 % 8 == 0, l.name
            if j.m == 0:
                continue
            lim_m, lim_n = {C.TQ_TAPS: (384, 256), C.TQ_COND: (384, 64), C.TQ_OUTSKIP: (192, 256)}[j.kind] if l.entry == "static" else (384, 256)
            assert j.m <= lim_m and j.n <= lim_n and j.n1 <= 256, l.name
            if l.entry == "stream":
                assert j.ones < 0 or (j.n <= j.ones and j.ones + l.B <= 256), l.name
            elif j.kind == C.TQ_COND:
                assert j.ones % 32 == 0 and j.ones >= j.n and l.B <= 32, l.name
        if l.entry != "tiles":
            assert l.nwg >= l.nteams * l.team_size and len(l.team_seg) == l.nteams + 1 and l.team_seg[-1] == len(l.segs), l.name
            assert all(0 <= jb and jb + l.team_size <= len(l.jobs) and 0 <= a <= b <= l.B * spc for jb, a, b in l.segs), l.name


def test_case_lists_hold_the_axes_of_the_issue():
    tl, sl = C.tile_cases(), C.stream_cases()
    assert {l.T for l in tl} >= set(C.T_AXIS) and {l.T for l in sl} >= set(C.T_AXIS)
    assert {l.splits for l in tl} == {1, 2, 3, 16} and {j.onehot for l in tl for j in l.jobs} == {None, 0, 128}
    assert {l.team_size for l in sl} == {1, 3, 5} and {l.nteams for l in sl} >= {1, 2, 3, 7}
    assert any(l.nwg % 8 == 0 for l in sl) and any(l.B == 32 for l in sl) and any(j.m == 0 for l in sl for j in l.jobs)
    for kind, tq in (("TAPS", C.TQ_TAPS), ("COND", C.TQ_COND), ("OUTSKIP", C.TQ_OUTSKIP)):
        ls = C.static_cases(kind)
        assert all(j.kind == tq for l in ls for j in l.jobs) and {l.T for l in ls} >= set(C.T_AXIS)
    cond = C.static_cases("COND")
    assert {j.n for l in cond for j in l.jobs} == {0, 8, 32, 40, 64} and {l.B for l in cond} >= {1, 2, 31, 32}
    osk = C.static_cases("OUTSKIP")
    assert any(j.n1 == 0 for l in osk for j in l.jobs) and {j.cb for l in osk for j in l.jobs} == {True, False}
    grp = C.static_cases("GROUP")
    assert {l.team_size for l in grp} == {4, 5} and {l.nwg for l in grp} >= {16, 48}
    assert any(len(l.jobs) == 2 * l.team_size * 3 for l in grp)                      # swapped copies of three groups
    assert any(j.onehot == 0 and j.kind == C.TQ_TAPS for l in grp for j in l.jobs)   # the head group
    for ls in (C.static_cases("TAPS"), osk, grp):                                     # segments inside the skipped slabs
        hit = 0
        for l in ls:
            u_lo, spc = (-min(j.shift for j in l.jobs)) >> 5, (l.T + 31) // 32
            hit += any(a < b and a // spc == (b - 1) // spc and b - 1 - a // spc * spc < u_lo for _, a, b in l.segs)
        assert hit >= 2
