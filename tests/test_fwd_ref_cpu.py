"""tests/fwd_ref.py (the float64 restatements of the forward layer, head and first conv) against float64 torch (conv1d, tanh and
sigmoid, cross_entropy), the packed streams of tests/fwd_cases.py against their dense matrices, and the preconditions and coverage of
every launch of tests/test_gpu_fwd_kernels.py -- all on the CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fwd_cases as C
import fwd_ref as R


def _close(got, want, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max()) / scale
    assert err <= 1e-12, f"{what}: relative error {err}"


@pytest.mark.parametrize("T,d", ((7, 1), (37, 5), (6, 9)))
@pytest.mark.parametrize("k,Cc", ((1, 0), (2, 3), (3, 4)))
def test_layer_ref_is_the_reference_layer(k, Cc, T, d):
    """ResidualConv1dGLU._forward in float64 torch: causal dilated conv1d + conv1x1c + bias, tanh * sigmoid, conv1x1_out, residual,
    sqrt(.5).  Ragged T, a dilation beyond T, clips with their own zb rows, and the dropout form (taps from x_conv, residual from x_in)"""
    torch.manual_seed(100 * k + 10 * d + T)
    B, Rr, H = 3, 5, 4
    f64 = dict(dtype=torch.float64)
    x, xc = torch.randn(B, Rr, T, **f64), torch.randn(B, Rr, T, **f64)
    c = torch.randn(B, Cc, T, **f64) if Cc else None
    W1, Wc, Wo = torch.randn(2 * H, Rr, k, **f64), (torch.randn(2 * H, Cc, 1, **f64) if Cc else None), torch.randn(Rr, H, 1, **f64)
    zb, bo = torch.randn(B, 2 * H, **f64), torch.randn(Rr, **f64)
    z = F.conv1d(F.pad(xc, ((k - 1) * d, 0)), W1, dilation=d) + zb.unsqueeze(-1)
    if Cc:
        z = z + F.conv1d(c, Wc)
    u = torch.tanh(z[:, :H]) * torch.sigmoid(z[:, H:])
    out = (F.conv1d(u, Wo, bo) + x) * np.sqrt(0.5)
    rows = lambda a: a.transpose(1, 2).reshape(B * T, -1)       # noqa: E731
    got = R.layer_ref(rows(x), rows(xc), rows(c) if Cc else None, zb, W1.permute(0, 2, 1), Wc[:, :, 0] if Cc else None, Wo[:, :, 0], bo, k, d,
                      [T] * B)
    _close(got.z, rows(z), "z")
    _close(got.u, rows(u), "u")
    _close(got.x_out, rows(out), "x_out")
    assert bool((got.zA >= got.z.abs() - 1e-12).all()) and bool((got.yA >= got.yx.abs() - 1e-12).all())
    assert got.n1 == 1 + k * Rr + Cc and got.n2 == H + 2
    # a list: every item is a clip of its own, with the zb row its record names
    Ts, zr = [T, 1, T + 2], [2, 0, 1]
    xs = [torch.randn(t, Rr, **f64) for t in Ts]
    cs = [torch.randn(t, Cc, **f64) for t in Ts] if Cc else None
    lst = R.layer_ref(torch.cat(xs), torch.cat(xs), torch.cat(cs) if Cc else None, zb, W1.permute(0, 2, 1), Wc[:, :, 0] if Cc else None,
                      Wo[:, :, 0], bo, k, d, Ts, zr)
    r0 = 0
    for i, t in enumerate(Ts):
        one = R.layer_ref(xs[i], xs[i], cs[i] if Cc else None, zb[zr[i]:zr[i] + 1], W1.permute(0, 2, 1), Wc[:, :, 0] if Cc else None, Wo[:, :, 0],
                          bo, k, d, [t])
        _close(lst.x_out[r0:r0 + t], one.x_out, f"item {i}: x_out")         # (a matrix product's order of additions depends on its row count)
        _close(lst.z[r0:r0 + t], one.z, f"item {i}: z")
        r0 += t


@pytest.mark.parametrize("T", (1, 2, 9))
def test_head_ref_is_the_reference_head(T):
    """wavenet.py:204-214 on the summed skips and the shifted, masked cross-entropy of vqwae_train.py:363-379,:764 in float64 torch"""
    torch.manual_seed(T)
    B, Ku, S, O, scale = 2, 6, 5, 7, 0.5
    f64 = dict(dtype=torch.float64)
    u, Ws, bs = torch.randn(B, T, Ku, **f64), torch.randn(S, Ku, **f64), torch.randn(S, **f64)
    W1, b1, W3, b3 = torch.randn(S, S, **f64), torch.randn(S, **f64), torch.randn(O, S, **f64), torch.randn(O, **f64)
    target = torch.randint(0, O, (B, T))
    skips = F.conv1d(u.transpose(1, 2), Ws.unsqueeze(-1), bs)
    h0 = torch.relu(skips * scale)
    h1 = torch.relu(F.conv1d(h0, W1.unsqueeze(-1), b1))
    y = F.conv1d(h1, W3.unsqueeze(-1), b3)
    got = R.head_ref(u, Ws, bs, W1, b1, W3, b3, scale, target)
    _close(got.logits, y, "logits")
    _close(got.h0, h0.transpose(1, 2), "h0")
    _close(got.h1, h1.transpose(1, 2), "h1")
    _close(got.lse, torch.logsumexp(y, 1), "lse")
    if T > 1:
        ce = F.cross_entropy(y[:, :, :-1], target[:, 1:], reduction="none")
        _close(got.nll[:, :-1], ce, "nll")
    assert not bool(got.nll[:, -1].any())
    again = R.head_ref(got.h0, None, None, W1, b1, W3, b3, scale, target, from_h0=True)
    assert torch.equal(again.logits, got.logits) and torch.equal(again.nll, got.nll) and again.A[0] is None
    rnd = lambda a: a.float().to(torch.bfloat16).double()       # noqa: E731
    handed = R.head_ref(u, Ws, bs, W1, b1, W3, b3, scale, target, handed0=rnd, handed1=rnd)
    assert torch.equal(handed.h0, rnd(got.h0)) and torch.equal(handed.h1, rnd(torch.relu(b1 + rnd(got.h0) @ W1.t())))


def test_first_conv_ref_is_a_conv_of_one_hot_columns():
    torch.manual_seed(0)
    Rr, O, BT = 6, 5, 11
    W, b = torch.randn(Rr, O, dtype=torch.float64), torch.randn(Rr, dtype=torch.float64)
    ids = torch.randint(0, O, (BT,))
    onehot = F.one_hot(ids, O).double().t().unsqueeze(0)
    got, bad = R.first_conv_ref(ids, None, W, b)
    _close(got, F.conv1d(onehot, W.unsqueeze(-1), b)[0].t(), "class ids")
    assert not bad
    ids2 = ids.clone()
    ids2[0], ids2[1] = -1, O
    got2, bad2 = R.first_conv_ref(ids2, None, W, b)
    assert bad2 and torch.equal(got2[0], W[:, 0] + b) and torch.equal(got2[1], W[:, O - 1] + b) and torch.equal(got2[2:], got[2:])
    xs = torch.randn(BT, dtype=torch.float64)
    gs, _ = R.first_conv_ref(None, xs, W[:, :1], b)
    _close(gs, F.conv1d(xs.view(1, 1, BT), W[:, :1].unsqueeze(-1), b)[0].t(), "scalar")


def _is_exact(x64, dt):
    return torch.equal(C.storage(x64, dt).double(), x64)


def test_layer_cases_keep_their_preconditions():
    """sat: every z is 64 n with |n| <= 17 in the a-half and n >= 2 in the b-half, exact in bf16 and fp16; the float64 gate of it is
    exactly -1, 0 or +1, each at least 10 % of u; y + x is an integer.  dense: z is an integer whose sum of |terms| stays below 2^22.
    Every case: operand pads as the kernels' contract has them, every exact sum below 2^22"""
    cases = C.layer_cases()
    assert len({c.name for c in cases}) == len(cases)
    kinds = set()
    for c in cases:
        for dt in {("fp32" if d == "fp32" else "bf16") if c.entry == "list" else "any" for d in c.dts}:
            dtype = "bf16" if dt == "any" else dt
            p = C.layer_problem(c, dtype)
            ref, own, H, Hp = p.ref, p.owned, c.H, c.Hp
            kinds.add((c.kind, c.entry))
            assert c.Rp % 128 == 0 and c.Ccp % 64 == 0 and 1 <= c.d and c.T <= 513 and (c.B <= 3 or c.entry == "list"), c.name
            assert not bool(p.x_in[..., c.R:].any()) and float(p.zb[:, 2 * Hp:].min()) == 1024.0, c.name
            assert not bool(p.zb[:, H:Hp].any()) and not bool(p.zb[:, Hp + H:2 * Hp].any()), c.name
            if c.Ccp > c.Cc > 0:
                assert bool((p.c_up[..., c.Cc:] != 0).all()), c.name
            if c.entry == "drop" and c.Rp > c.R:
                assert bool((p.x_conv[..., c.R:] != 0).all()), c.name
            if c.entry == "drop":
                assert not torch.equal(p.x_conv[..., :c.R], p.x_in[..., :c.R]), c.name
            assert bool(torch.isnan(ref.u[~own]).all()) and not bool(torch.isnan(ref.u[own]).any()), c.name
            z, u, yx = ref.z[own], ref.u[own], ref.yx[own]
            assert float(ref.zA[own].max()) < C.EXACT_LIMIT and float(ref.yA[own].max()) < C.EXACT_LIMIT, c.name
            assert not bool(z[:, H:Hp].any()) and not bool(z[:, Hp + H:].any()) and not bool(u[:, H:].any()) and not bool(yx[:, c.R:].any()), c.name
            if c.kind == "sat":
                n = z / 64.0
                assert torch.equal(n, n.round()) and float(n[:, :H].abs().max()) <= 17 and float(n[:, Hp:Hp + H].min()) >= 2, c.name
                assert _is_exact(z, "bf16") and _is_exact(z, "fp16"), c.name
                assert bool(((u == -1) | (u == 0) | (u == 1)).all()), c.name
                assert torch.equal(u[:, :H], torch.sign(z[:, :H])), c.name
                assert min(C._shares(u[:, :H])) >= C.SHARE, (c.name, C._shares(u[:, :H]))
                assert torch.equal(yx, yx.round()), c.name
                assert int((p.W1 != 0).sum((1, 2)).max()) + (int((p.Wc != 0).sum(1).max()) if c.Cc else 0) <= 16, c.name
                both = torch.cat([p.W1.reshape(2 * H, -1)] + ([p.Wc] if c.Cc else []), 1)
                assert int((both != 0).sum(1).max()) <= 8 and float(both.abs().max()) <= 2, c.name
                x0 = C.sat_x_out(yx, "bf16")
                assert not _is_exact(yx * R.SQRT_HALF, "fp32") and x0.shape == yx.shape, c.name
            else:
                assert c.kind == "dense" and torch.equal(z, z.round()), c.name
                both = torch.cat([p.W1.reshape(2 * H, -1)] + ([p.Wc] if c.Cc else []), 1)
                assert float(both.abs().max()) == 3 and bool((both == 0).any()), c.name
    assert kinds >= {(k, e) for k in ("sat", "dense") for e in ("fwd", "drop", "list")}


def test_head_cases_keep_their_preconditions():
    """every sum of an exact head case is exact in any order: the sum of |terms| over the smallest unit in play stays below 2^22; "ce":
    one class at least 128 above all others in every column, below the 4096 of the pad classes' bias; lse = max and nll = max - picked"""
    cases = C.head_cases()
    assert len({c.name for c in cases}) == len(cases)
    doms = {}
    for c in cases:
        for dt in c.dts:
            p = C.head_problem(c, dt)
            ref = p.ref
            assert c.scale in (1.0, 0.5, 0.25) and c.T <= 513 and c.B <= 3, c.name
            for A in ref.A:
                if A is not None:
                    assert float(A.max()) / p.unit < C.EXACT_LIMIT, (c.name, dt, float(A.max()), p.unit)
            for v in (ref.h0, ref.h1, ref.logits):
                assert torch.equal(v / p.unit, (v / p.unit).round()), c.name
            assert _is_exact(ref.h0, dt) and _is_exact(ref.h1, dt) and _is_exact(ref.logits, "fp32"), c.name
            assert bool((ref.h0 > 0).any()) and bool((ref.h1 > 0).any()), c.name
            x = p.x
            if c.entry == "head" and c.Ku > c.L * c.Hh:
                Hp = C._ru(c.Hh, 32)
                assert bool((x[:, :, c.L * Hp:] == 3).all()) and bool((x[:, :, :c.L * Hp].reshape(c.B, c.T, c.L, Hp)[..., c.Hh:] == 3).all()), c.name
            if c.entry == "from_h0" and c.Sp > c.S:
                assert bool((x[:, :, c.S:] == 3).all()), c.name
            tg = p.target.long()
            assert int(tg.min()) >= 0 and int(tg.max()) < c.O, c.name
            if c.kind == "ce":
                lg = ref.logits
                top2 = lg.topk(2, dim=1).values
                assert float((top2[:, 0] - top2[:, 1]).min()) >= C.CE_GAP and bool((lg.argmax(1) == c.dom).all()), c.name
                assert float(lg.max()) + C.CE_GAP <= C.PAD_B3, (c.name, float(lg.max()))
                assert torch.equal(ref.lse, top2[:, 0]), c.name            # float64 logsumexp of such a column is the maximum itself
                want = top2[:, 0, :-1] - torch.gather(lg[:, :, :-1], 1, tg[:, 1:].unsqueeze(1)).squeeze(1)
                assert torch.equal(ref.nll[:, :-1], want) and not bool(ref.nll[:, -1].any()), c.name
                assert bool((ref.nll[:, :-1] == 0).any()) and bool((ref.nll[:, :-1] >= C.CE_GAP).any()), c.name
                assert int(tg[0, 0]) != c.dom, c.name
                doms.setdefault(c.entry, set()).add((c.O, c.dom))
                picked = {int(t) for t in tg[:, 1:].reshape(-1)}
                assert picked >= {1, 5, 31, 32, 63, c.O - 1} & set(range(c.O)), c.name
    for entry in ("head", "from_h0"):
        d = doms[entry]
        assert {dom for O, dom in d} >= {1, 5, 31, 32, 63} and {dom == O - 1 for O, dom in d} == {True, False}, d
        assert {O for O, dom in d if dom == O - 1} >= {100, 128, 129, 257, 384}, d


def test_first_conv_cases():
    cases = C.fc_cases()
    assert {c.BT for c in cases} == {1, 255, 257} and {C._ru(c.R, 128) for c in cases} == {128, 512} and {c.O for c in cases} == {100, 256}
    for c in cases:
        p = C.fc_problem(c)
        tab, bias = C.fc_streams(c, p)
        Rp = C._ru(c.R, 128)
        assert tab.shape == ((1 if c.scalar else c.O), Rp) and torch.equal(tab[:, :c.R], p.W.t()) and not bool(tab[:, c.R:].any()), c.name
        assert torch.equal(bias[:c.R], p.bias) and not bool(bias[c.R:].any()), c.name
        assert p.flagged == c.bad and _is_exact(p.ref, "bf16") and _is_exact(p.ref, "fp16"), c.name
        if c.bad:
            assert int(p.ids.min()) == -1 and (c.BT == 1 or int(p.ids.max()) == c.O), c.name


def test_packed_streams_hold_every_dense_element_once():
    """the maps of the product, applied to the arena of a case: every nonzero dense weight appears exactly once in its stream, the
    arena's filler (every slot no map of the launch may point to) never, and the stream has the size the ABI states"""
    seen = set()
    for c in C.layer_cases():
        for dt in c.dts:
            key = (c.R, c.H, c.Cc, c.k, dt != "fp32")
            if key in seen or c.kind != "dense":
                continue
            seen.add(key)
            p = C.layer_problem(c, dt)
            w, bias = C.layer_streams(c, p, dt)
            assert not bool((w == C.ARENA_FILL).any()) and not bool((bias == C.ARENA_FILL).any()), c.name
            n1 = w.numel() - c.Rp * c.Hp
            dense1 = torch.cat([p.W1.reshape(2 * c.H, -1)] + ([p.Wc] if c.Cc else []), 1)
            for stream, dense in ((w[:n1], dense1), (w[n1:], p.W_out)):
                for v in (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0):
                    assert int((stream == v).sum()) == int((dense == v).sum()), (c.name, dt, v)
            assert torch.equal(bias[:c.R], p.b_out) and not bool(bias[c.R:].any()), c.name
    assert len(seen) >= 20
    seen = set()
    for c in C.head_cases():
        for dt in c.dts:
            key = (c.S, c.O, c.L, c.Hh, dt != "fp32")
            if key in seen or c.kind != "dense":
                continue
            seen.add(key)
            p = C.head_problem(c, dt)
            w, tail, bias = C.head_streams(c, p, dt)
            assert not bool((w == C.ARENA_FILL).any()) and tail == c.Ku * c.Sp, c.name
            for stream, dense in ((w[:tail], p.W_skip), (w[tail:tail + c.Sp * c.Sp], p.W1), (w[tail + c.Sp * c.Sp:], p.W3)):
                for v in (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0):
                    assert int((stream == v).sum()) == int((dense == v).sum()), (c.name, dt, v)
            assert torch.equal(bias[:c.S], p.b_skip) and torch.equal(bias[c.Sp:c.Sp + c.S], p.b1), c.name
            assert torch.equal(bias[2 * c.Sp:2 * c.Sp + c.O], p.b3) and bool((bias[2 * c.Sp + c.O:] == C.PAD_B3).all()), c.name
    assert len(seen) >= 10


def test_every_path_is_reached_at_every_time_of_its_tile_set():
    """the path of every (case, dtype) by the Python restatement of the dispatch; per path: every T of its tile set with and without
    the z save (WAE_GLU_SAVE_Z has kernels of its own on the static path), in every dtype the path exists in, in both exact kinds"""
    seen = {}
    for c in C.layer_cases():
        for dt in c.dts:
            seen.setdefault(C.fwd_path(c, dt), []).append((c, dt))
    assert set(seen) == set(C.FWD_PATH_DTYPES), sorted(set(seen) ^ set(C.FWD_PATH_DTYPES))
    for path, tiles in C.FWD_PATH_TILES.items():
        for dt in C.FWD_PATH_DTYPES[path]:
            for save in (C.SAVE_Z, 0):
                got = {c.T for c, d in seen[path] if d == dt and (c.flags & C.SAVE_Z) == save}
                assert got >= set(tiles), (path, dt, save, sorted(got))
        assert {c.kind for c, _ in seen[path]} == {"sat", "dense"} and max(c.B for c, _ in seen[path]) == 3, path
        assert {c.entry for c, _ in seen[path]} >= {"fwd", "drop"}, path
        big = [c for c, _ in seen[path] if c.B == 3 and c.T >= 257]
        assert big and {c.d for c in big} & {128, 512, 33, 2}, path
    for path in ("static/256x192", "static/256x128", "static/512x256"):
        at3 = [c for c, _ in seen[path] if c.B == 3]
        assert {c.T for c in at3} >= set(C.T256), path
        assert {c.d for c in at3 if c.T == 257} >= {1, 2, 31, 32, 33, 128, 512, 256, 257, 262}, path
    base = [c for c, _ in seen["generic-8x32"] + seen["fp32-4x32"]]
    assert {c.d for c in base if c.T == 33} >= {1, 2, 31, 32, 33, 128, 512, 38} and {c.k for c in base} >= {1, 2, 3, 5}
    assert {c.Ccp for c in base} >= {0, 64, 128} and {c.Hp // 32 for c in base} >= {1, 2, 3, 4, 6, 8} and {c.Rp for c in base} >= {128, 256, 512}
    assert any(c.H < c.Hp for c in base) and any(c.H == c.Hp for c in base) and any(c.R < c.Rp for c in base) and {c.B for c in base} >= {1, 2, 3}
    for flags in C._FLAG_AXIS:
        assert any(c.flags == flags for c, _ in seen["generic-8x32"] + seen["generic-4x64"] + seen["generic-4x32"]), flags
    assert {c.flags for c, _ in seen["static/256x128"]} >= {0, C.SAVE_Z, C.PAIR, C.PAIR | C.SAVE_Z, C.NO_OUT, C.NO_OUT | C.SAVE_Z}
    for path in ("list-8x32", "list-fp32-4x32"):
        ls = [c for c, _ in seen[path]]
        assert {i for c in ls for i in c.items} >= set(C.LIST_LENGTHS) and {len(c.items) for c in ls} >= {3, 4}, path
        assert any(c.flags & C.NO_OUT for c in ls) and any(c.flags & C.PAIR for c in ls) and {c.kind for c in ls if (0, 0) in c.items} == {"sat", "dense"}, path
        for c in ls:            # a malformed record owns rows and a tile of its own, which the launch must leave alone
            if (0, 0) in c.items:
                p = C.layer_problem(c, "fp32" if path == "list-fp32-4x32" else "bf16")
                assert int((~p.owned).sum()) == C.LIST_BAD_ROWS and p.ntiles == int(p.table[-1, 3]) == 1 + sum(
                    -(-T // C.list_tile("fp32" if path == "list-fp32-4x32" else "bf16")) for T in p.table[:-1, 1]), c.name
        assert any(c.zb_rows != tuple(range(len(c.items))) for c in ls) and {c.kind for c in ls} == {"sat", "dense"}, path
    assert {C.fwd_path(c, dt) for c in C.layer_rounding_cases() for dt in c.dts} == set(C.FWD_PATH_DTYPES)
    for c in C.layer_rounding_cases():
        for dt in c.dts:
            assert dt in C.FWD_PATH_DTYPES[C.fwd_path(c, dt)]
    assert C.fwd_path(C.layer_case(C.LAYER_REFUSED[0][0], "sat", C.DTYPES), "bf16") == "refused"

    seen = {}
    for c in C.head_cases():
        for dt in c.dts:
            seen.setdefault(C.head_path(c, dt), []).append((c, dt))
    assert set(seen) == set(C.HEAD_PATH_TILES)
    for path, tiles in C.HEAD_PATH_TILES.items():
        for dt in C.HEAD_PATH_DTYPES[path]:
            got = {c.T for c, d in seen[path] if d == dt}
            assert got >= set(tiles), (path, dt, sorted(got))
        assert {c.kind for c, _ in seen[path]} == {"rep", "dense", "ce"} and {c.B for c, _ in seen[path]} >= {1, 3}, path
        assert {c.Sp for c, _ in seen[path]} == {128, 256} and {c.Op for c, _ in seen[path]} == {128, 256, 384}, path
    h4 = [c for c, _ in seen["head4"]]
    assert {c.Ku // 64 for c in h4} >= {1, 2, 3, 4, 5, 9} and {c.O for c in h4} >= {100, 128, 129, 256, 257, 384} and {c.scale for c in h4} == {1.0, 0.5, 0.25}
    assert {c.nulls for c in h4} >= set(C._NULLS)
    assert {C.head_path(c, dt) for c in C.head_rounding_cases() for dt in c.dts} == set(C.HEAD_PATH_TILES)


def test_rounding_cases_are_what_they_say():
    """layer: z about N(0, 1.5) with a few entries at +-20; head: logits of spread about 3"""
    for c in C.layer_rounding_cases():
        p = C.layer_problem(c, c.dts[0])
        z = p.ref.z[p.owned][:, :c.H]
        # (N(0, 1.5) has median |z| = 1.01; the channels at +-20 are few)
        assert 0.6 < float(z.abs().median()) < 1.6 and float(z.abs().max()) > 15.0 and float((z.abs() > 10).double().mean()) < 0.1, (c.name, float(z.abs().median()))
        if c.kind == "gate":        # z is exact in fp32 in any order, and one rounding away from its stored value
            zz, A = p.ref.z[p.owned] / C.GATE_UNIT, p.ref.zA[p.owned] / C.GATE_UNIT
            assert torch.equal(zz, zz.round()) and float(A.max()) < C.EXACT_LIMIT and torch.equal(p.ref.z[p.owned].float().double(), p.ref.z[p.owned]), c.name
            for a in (p.x_in, p.c_up):
                assert _is_exact(a.double(), "bf16") and _is_exact(a.double(), "fp16"), c.name
            assert float(p.ref.yA[p.owned].max()) < C.EXACT_LIMIT, c.name
    assert {c.kind for c in C.layer_rounding_cases()} == {"gauss", "gate"}
    for c in C.head_rounding_cases():
        p = C.head_problem(c, "fp32")
        lg = C.head_reference(c, p, "fp32").logits
        assert 1.5 < float(lg.std()) < 6.0, (c.name, float(lg.std()))
