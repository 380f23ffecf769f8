"""tests/tm_ref.py (the float64 restatement of the backward data path's time-major contraction) against torch.autograd, the packed
streams of tests/tm_cases.py against their dense matrices, and the preconditions and coverage of every launch of
tests/test_gpu_tm_kernels.py / tests/test_gpu_bwd_pair_kernels.py -- all on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tm_cases as C
import tm_ref as R


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max()) / scale
    assert err <= 1e-12, f"{what}: relative error {err}"


def _tm(a):         # (B, C, T) -> time-major (B, T, C)
    return a.detach().transpose(1, 2).contiguous()


@pytest.mark.parametrize("T,d", ((7, 1), (37, 5), (6, 9)))
@pytest.mark.parametrize("k", (2, 3))
def test_modes_1_and_2_match_autograd(k, T, d):
    """a ResidualConv1dGLU-shaped layer in float64: z = dilated causal conv of x, u = tanh(a) sigmoid(b), out = alpha (W_out u + x),
    skip = W_skip u.  Mode 2 over [dout | dskip] is autograd's dz; mode 1 over the k taps of dz (tap j at t + (k - 1 - j) d) plus the
    residual gradient is autograd's dx.  Ragged T, and a dilation beyond T (every shifted tap is zeros)."""
    torch.manual_seed(100 * k + 10 * d + T)
    B, Rr, H, S, alpha = 2, 5, 3, 6, 0.5
    f64 = dict(dtype=torch.float64)
    x = torch.randn(B, Rr, T, **f64).requires_grad_()
    W1 = torch.randn(2 * H, Rr, k, **f64)
    Wo, Ws = torch.randn(Rr, H, 1, **f64), torch.randn(S, H, 1, **f64)
    z = F.conv1d(F.pad(x, ((k - 1) * d, 0)), W1, dilation=d)
    z.retain_grad()
    u = torch.tanh(z[:, :H]) * torch.sigmoid(z[:, H:])
    out, skip = alpha * (F.conv1d(u, Wo) + x), F.conv1d(u, Ws)
    Gout, Gs = torch.randn_like(out), torch.randn_like(skip)
    ((out * Gout).sum() + (skip * Gs).sum()).backward()
    Wu = torch.cat([alpha * Wo[:, :, 0].t(), Ws[:, :, 0].t()], dim=1)             # (H, R + S)
    got = R.tm_ref(2, Wu, [_tm(Gout), _tm(Gs)], [0, 0], 1.0, _tm(z), B, T)
    _close(got.out, _tm(z.grad), "dz (mode 2)")
    Wx = torch.cat([W1[:, :, j].t() for j in range(k)], dim=1)                    # (R, k * 2H) tap by tap
    shifts = [(k - 1 - j) * d for j in range(k)]
    dz = _tm(z.grad)
    got = R.tm_ref(1, Wx, [dz] * k, shifts, 1.0, alpha * _tm(Gout), B, T)
    _close(got.out, _tm(x.grad), "dx (mode 1)")
    assert bool((got.A >= got.out.abs() - 1e-12).all()) and got.n == k * 2 * H + 1
    half = R.tm_ref(1, Wx, [dz] * k, shifts, -2.0, alpha * _tm(Gout), B, T)
    _close(half.out, -2.0 * _tm(x.grad), "alpha")


def test_other_epilogues_and_shifts():
    rng = np.random.RandomState(3)
    B, T, M = 2, 9, 4
    X0, X1 = torch.from_numpy(rng.randn(B, T, 3)), torch.from_numpy(rng.randn(B, T, 2))
    W = torch.from_numpy(rng.randn(M, 5))
    acc = torch.zeros(B, T, M, dtype=torch.float64)
    for t in range(T):
        for X, s, k0 in ((X0, 2, 0), (X1, -3, 3)):
            if 0 <= t + s < T:
                acc[:, t] += X[:, t + s] @ W[:, k0:k0 + X.shape[2]].t()
    assert torch.allclose(R.tm_ref(0, W, [X0, X1], [2, -3], 1.0, None, B, T).out, acc, rtol=0, atol=1e-13)
    bias, aux = torch.from_numpy(rng.randn(M)), torch.from_numpy(rng.randn(B, T, M))
    aux[0, 0, 0] = 0.0
    assert torch.allclose(R.tm_ref(3, W, [X0, X1], [2, -3], -2.0, bias, B, T).out, torch.relu(-2.0 * (bias + acc)), rtol=0, atol=1e-13)
    assert torch.allclose(R.tm_ref(4, W, [X0, X1], [2, -3], 0.25, aux, B, T).out, torch.where(aux > 0, 0.25 * acc, torch.zeros(())), rtol=0, atol=1e-13)
    lg = R.tm_ref(5, W, [X0, X1], [2, -3], 1.0, bias, B, T, O=3)
    assert lg.out.shape == (B, 3, T) and torch.allclose(lg.out, (bias + acc)[:, :, :3].transpose(1, 2), rtol=0, atol=1e-13)
    for s in (T, T + 5, -T):
        assert not bool(R.shifted(X0, s, T).any())
    zero = R.tm_ref(2, W, [X0, X1], [0, 0], 1.0, torch.zeros(B, T, 2 * M), B, T)
    assert torch.equal(zero.out[:, :, :M], zero.acc / 2) and not bool(zero.out[:, :, M:].any())


@pytest.mark.parametrize("dc_mode,last", ((0, 0), (1, 0), (3, 0), (2, 1)))
def test_pair_ref_is_the_two_tm_ref_calls(dc_mode, last):
    rng = np.random.RandomState(5 + dc_mode)
    B, T, Rp, Hp, Sp, k, d, alpha = 2, 11, 6, 4, 5, 3, 2, 0.5
    r = lambda *s: torch.from_numpy(rng.randn(*s))    # noqa: E731
    Wx, Wuo, Wus, Wc = r(Rp, k * 2 * Hp), r(Hp, Rp), r(Hp, Sp), r(64, 2 * Hp)
    dz, gn, ds, zp, dcp = r(B, T, 2 * Hp), r(B, T, Rp), r(B, T, Sp), r(B, T, 2 * Hp), r(B, T, 64)
    rnd = lambda x: x.float().to(torch.bfloat16).double()      # noqa: E731
    got = R.pair_ref(Wx, Wuo, Wus, dz, gn, ds, zp, k, d, alpha, B, T, round_fn=rnd, W_c=Wc, dc_prev=dcp, dc_mode=dc_mode, last=last)
    a = R.tm_ref(1, Wx, [dz] * k, [2 * d, d, 0], alpha, gn, B, T)
    assert torch.equal(got.g_out.out, a.out) and torch.equal(got.handed, rnd(a.out))
    if last:
        assert got.dz_prev is None
    else:
        b = R.tm_ref(2, torch.cat([Wuo, Wus], 1), [rnd(a.out), ds], [0, 0], 1.0, zp, B, T)
        assert torch.equal(got.dz_prev.out, b.out)
    dc = R.tm_ref(0, Wc, [dz], [0], 1.0, None, B, T).out + (dcp if dc_mode & 1 else 0.0)
    assert torch.equal(got.dc.out, dc) and got.dc_to_out == bool(dc_mode & 2)
    own = R.pair_ref(Wx, Wuo, Wus, dz, gn, ds, zp, k, d, alpha, B, T, handed=gn)
    assert torch.equal(own.handed, gn) and own.dc is None


def test_interleaved_order_is_the_headers():
    """chunk q of an interleaved stream is column block q // nsrc of source q % nsrc; back to back otherwise"""
    for ck in (32, 64):
        p = C.stream_perm((128, 128, 128), True, ck)
        for q in range(3 * 128 // ck):
            assert list(p[q * ck:(q + 1) * ck]) == list(range((q % 3) * 128 + (q // 3) * ck, (q % 3) * 128 + (q // 3) * ck + ck))
    assert list(C.stream_perm((64, 128, 192), False, 64)) == list(range(384))


def test_every_dense_element_appears_exactly_once_in_its_stream():
    """pack round trip for every (M, K, dtype, interleave, slice count) of the case tables, w_uo / w_us / w_c included: the maps hold
    every index of the dense matrix once, and gathering then scattering gives the matrix back"""
    shapes = set()
    for c in C.tm_cases() + C.tm_rounding_cases():
        for dt in C.DTYPES:
            shapes.add(("first", c.M, c.cols, dt, c.interleave))
    for c in C.pair_cases() + C.pair_rounding_cases():
        for dt in C.pair_dtypes(c):
            shapes |= {("first", c.Rp, (2 * c.Hp,) * c.ktaps, dt, dt != "fp32"), ("second", c.Hp, (c.Rp,), dt, False),
                       ("first", c.Hp, (c.Sp,), dt, False), ("first", 64, (2 * c.Hp,), dt, False)}
    assert len(shapes) > 100 and {C.tm_slices(s[1])[1] for s in shapes if s[0] == "first"} >= {1, 2, 5}
    rng = np.random.RandomState(0)
    for form, M, cols, dt, il in sorted(shapes):
        K = sum(cols)
        idx = C.first_index(M, K, dt, C.stream_perm(cols, il, C.CK[dt])) if form == "first" else C.second_index(M, K, dt)
        assert idx.shape == (M * K,) and np.array_equal(np.sort(idx), np.arange(M * K)), (form, M, cols, dt, il)
        if M * K <= 128 * 384:
            W = torch.from_numpy(rng.randn(M, K).astype(np.float32))
            back = torch.zeros(M * K)
            back[torch.from_numpy(idx).long()] = C.gather(W, idx)
            assert torch.equal(back.view(M, K), W)


def _is_exact(x64, dt):
    return torch.equal(C.storage(x64, dt).double(), x64)


def _bf16_ties(x64):
    bits = x64.float().view(torch.int32)
    return int(((bits & 0xFFFF) == 0x8000).sum())


def test_tm_cases_stay_exact_representable_and_tied():
    """every exact wae_gemm_tm case: no output's sum of |terms| reaches 2^22; a "rep" case stores only values exact in bf16 and fp16; a
    dense case whose output is 16-bit holds at least one exact bf16 tie; mode 2 runs on z = 0"""
    cases = C.tm_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        prob = C.tm_problem(c, "bf16")
        assert float(prob.ref.A.max()) < C.EXACT_LIMIT, c.name
        assert float(prob.ref.out.abs().max()) > 0 or all(abs(sh) >= c.T for sh in c.shifts), c.name
        assert all(w % 64 == 0 for w in c.cols) and 1 <= len(c.cols) <= 4 and C.tm_path(c, "fp32") != "refused", c.name
        if c.mode == 2:
            assert torch.equal(prob.ref.out[:, :, :c.M], prob.ref.acc / 2) and not bool(prob.ref.out[:, :, c.M:].any()), c.name
        if c.mode == 4:
            a = prob.aux[:, :, C.COLS[0]:C.COLS[0] + c.M]
            assert bool((a > 0).any()) and bool((a < 0).any()) and bool((a == 0).any()), c.name
        if c.kind == "rep":
            assert _is_exact(prob.ref.out, "bf16") and _is_exact(prob.ref.out, "fp16"), c.name
            assert int((prob.W != 0).sum(1).max()) <= 8
        else:
            assert c.kind == "dense" and sum(c.cols) >= C.DENSE_MIN_K and bool((prob.W == 0).any()) and float(prob.W.abs().max()) == 3, c.name
            if c.mode != 5:         # (the logits are fp32)
                assert _bf16_ties(prob.ref.out) >= 1 and not _is_exact(prob.ref.out, "bf16"), c.name


def test_pair_cases_stay_exact_representable_and_tied():
    cases = C.pair_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        for dt in C.pair_dtypes(c):
            if C.pair_path(c, dt) == "refused":
                continue
            ref = C.pair_problem(c, dt).ref
            outs = [ref.g_out] + ([ref.dz_prev] if ref.dz_prev is not None else []) + ([ref.dc] if ref.dc is not None else [])
            assert all(float(o.A.max()) < C.EXACT_LIMIT for o in outs), c.name
            assert (ref.dz_prev is None) == bool(c.last) and (ref.dc is None) == (not c.dc), c.name
            stored = [ref.g_out.out] + ([ref.dz_prev.out] if ref.dz_prev is not None else []) + ([ref.dc.out] if ref.dc is not None and ref.dc_to_out else [])
            if c.kind == "rep":
                for x in stored + [ref.handed]:
                    assert _is_exact(x, "bf16") and _is_exact(x, "fp16"), (c.name, dt)
            elif dt == "bf16":
                assert sum(_bf16_ties(x) for x in stored) >= 1, c.name
                if (c.ktaps - 1) * c.dilation < c.T // 2:   # (taps beyond the clip leave too few terms) the hand-over really rounds
                    assert not torch.equal(ref.handed, ref.g_out.out), c.name


def test_every_path_is_reached_at_every_time_of_its_tile_set_in_both_forms():
    """the path of every (case, dtype) by the Python restatement of the dispatch; per path: every T of its tile set, B * tiles both a
    multiple of 8 and not; where a shape has two launch forms, both are in the table"""
    seen = {}
    for c in C.tm_cases():
        for dt in C.tm_dtypes(c):
            seen.setdefault(C.tm_path(c, dt), []).append((c, dt))
    assert set(seen) == set(C.TM_PATH_TILES), sorted(set(seen) ^ set(C.TM_PATH_TILES))
    for path, tiles in C.TM_PATH_TILES.items():
        tw = 256 if tiles is C.T256 else 128
        assert {c.T for c, _ in seen[path]} >= set(tiles), (path, sorted({c.T for c, _ in seen[path]}))
        assert {(c.B * ((c.T + tw - 1) // tw)) % 8 == 0 for c, _ in seen[path]} == {True, False}, path
        if not path.startswith("generic-one"):
            assert {dt for _, dt in seen[path]} == {"bf16", "fp16"}, path
            assert {c.kind for c, _ in seen[path]} == {"rep", "dense"}, path
            # the same shapes with WAE_TM_ONE_WG
            flagged = {c._replace(name="", one_wg=False, kind="") for c, _ in seen["generic-one/m" + path[-1]] if c.one_wg}
            assert {c.T for c, _ in seen[path] if c._replace(name="", kind="") in flagged} >= set(C.T128) & set(tiles), path
    assert {dt for _, dt in seen["generic-one/m0"]} == set(C.DTYPES)
    names = {c.name: c for c in C.tm_cases()}
    assert any(c.mode == 2 and c.M == 256 and not c.one_wg and C.tm_path(c, "bf16") == "generic-one/m2" for c in names.values())
    assert any(c.mode == 2 and c.M == 64 and C.tm_path(c, "bf16") == "generic-paired/m2" for c in names.values())
    assert {C.tm_slices(c.M) for c in names.values() if c.mode in (0, 1)} >= {(1, 1), (2, 1), (3, 1), (4, 1), (6, 1), (8, 1), (6, 2), (8, 2), (4, 5)}
    assert {len(c.cols) for c in names.values()} == {1, 2, 3, 4} and any(len(set(c.cols)) == 3 for c in names.values())
    assert {len(c.cols) for c in names.values() if c.interleave and c.one_array} == {2, 3, 4}
    assert any(c.interleave and not c.one_array for c in names.values())
    assert any(s < 0 for c in names.values() for s in c.shifts) and {c.B for c in names.values()} >= {1, 3, 8, 9}
    assert all(C.tm_path(c, dt) == "refused" for c in C.tm_refused_cases() for dt in C.DTYPES)
    for c in C.tm_rounding_cases():
        assert c.T <= 513
    assert {C.tm_path(c, dt) for c in C.tm_rounding_cases() for dt in C.DTYPES} == set(C.TM_PATH_TILES)

    seen = {}
    for c in C.pair_cases():
        for dt in C.pair_dtypes(c):
            seen.setdefault(C.pair_path(c, dt), []).append((c, dt))
    assert set(seen) == set(C.PAIR_PATH_TILES) | {"refused"}
    for path, tiles in C.PAIR_PATH_TILES.items():
        assert {c.T for c, _ in seen[path]} >= set(tiles), (path, sorted({c.T for c, _ in seen[path]}))
        assert {c.kind for c, _ in seen[path]} == {"rep", "dense"} and {c.B for c, _ in seen[path]} >= {1, 3}, path
    assert {(c.Rp, c.Hp) for c, _ in seen["fused-fp32"]} == {(256, 192), (256, 128), (128, 32), (128, 64), (128, 96), (128, 128)}
    assert {(c.Rp, c.Hp) for c, _ in seen["pair4"]} == {(256, 192), (256, 128), (128, 64), (128, 128)}
    assert {c.ktaps for c, _ in seen["pair4"]} == {2, 3, 4} and {(c.Rp, c.Hp) for c, _ in seen["refused"]} == {(128, 32), (128, 96)}
    for path in ("pair8", "pair4-fold"):
        assert {(c.dc_mode & 3, c.last) for c, _ in seen[path]} >= {(0, 0), (1, 0), (2, 0), (3, 0), (1, 1), (2, 1)}, path
    assert {c.Hp for c, _ in seen["pair8"]} == {128, 192} and (128, 64) in {(c.Rp, c.Hp) for c, _ in seen["pair4-fold"]}
    assert {C.pair_path(c, dt) for c in C.pair_rounding_cases() for dt in C.pair_dtypes(c)} == set(C.PAIR_PATH_TILES)


def test_rounding_cases_keep_their_exact_parts_exact():
    """mode 2 and the "gate" pair cases measure the gate derivative alone: their GEMM operands are integers and du stays exact"""
    for c in C.tm_rounding_cases():
        if c.mode == 2:
            prob = C.tm_problem(c, "bf16")
            assert float(prob.ref.A.max()) < C.EXACT_LIMIT and torch.equal(prob.ref.acc, prob.ref.acc.round()), c.name
            z = prob.aux[:, :, C.COLS[0]:C.COLS[0] + 2 * c.M]
            assert float(z.abs().max()) == 20.0 and float(z.abs().median()) < 3.0, c.name
    for c in C.pair_rounding_cases():
        if c.kind == "gate":
            for dt in C.pair_dtypes(c):
                ref = C.pair_reference(c, C.pair_problem(c, dt), dt)
                assert float(ref.g_out.A.max()) < C.EXACT_LIMIT and float(ref.dz_prev.A.max()) < C.EXACT_LIMIT, (c.name, dt)
                assert c.alpha == 0.5 and torch.equal(2 * ref.g_out.out, (2 * ref.g_out.out).round()), c.name
