"""tests/frontend_ref.py (the float64 checkers of tests/test_gpu_frontend_bwd.py) against explicit-loop restatements of the same
formulas, each once at one tiny shape."""
import numpy as np
import torch

import frontend_ref as R


def _ints(rng, *shape):
    return torch.from_numpy(rng.randint(-3, 4, size=shape).astype(np.float64))


def test_conv_block_forward_and_grads_against_loops():
    rng = np.random.RandomState(0)
    B, Cin, Cout, Tin, k, stride, pad = 2, 3, 3, 7, 5, 2, 2
    Tout = R.conv_tout(Tin, k, stride, pad)
    assert Tout == 4
    for relu, residual, st, pd in ((1, 0, stride, pad), (0, 0, stride, pad), (1, 1, 1, 2)):
        To = R.conv_tout(Tin, k, st, pd)
        x, w, b, dy = _ints(rng, B, Cin, Tin), _ints(rng, Cout, Cin, k), _ints(rng, Cout), _ints(rng, B, Cout, To)
        y, mask = R.conv_block_forward(x, w, b, st, pd, relu, residual)
        want_y = torch.zeros(B, Cout, To, dtype=torch.float64)
        dx, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(b)
        for bb in range(B):
            for co in range(Cout):
                for to in range(To):
                    pre = float(b[co])
                    for ci in range(Cin):
                        for j in range(k):
                            ti = to * st + j - pd
                            if 0 <= ti < Tin:
                                pre += float(w[co, ci, j] * x[bb, ci, ti])
                    on = pre > 0 or not relu
                    want_y[bb, co, to] = (pre if on else 0.0) + (float(x[bb, co, to]) if residual else 0.0)
                    g = float(dy[bb, co, to]) if on else 0.0
                    db[co] += g
                    for ci in range(Cin):
                        for j in range(k):
                            ti = to * st + j - pd
                            if 0 <= ti < Tin:
                                dx[bb, ci, ti] += g * w[co, ci, j]
                                dw[co, ci, j] += g * x[bb, ci, ti]
                    if residual:
                        dx[bb, co, to] += dy[bb, co, to]
        assert torch.equal(y, want_y)
        assert torch.equal(R.relu_mask_from_output(y, x, residual) if relu else torch.ones_like(mask), mask)
        got = R.conv_block_grads(x, w, dy, st, pd, mask if relu else None, residual)
        assert torch.equal(got[0], dx) and torch.equal(got[1], dw) and torch.equal(got[2], db)


def test_upsample_stage_against_loops():
    rng = np.random.RandomState(1)
    B, C, Tin, s = 2, 2, 4, 3
    inp, w, dout = _ints(rng, B, C, Tin), _ints(rng, 2 * s + 1), _ints(rng, B, C, Tin * s)
    Tout = Tin * s
    out = torch.zeros(B, C, Tout, dtype=torch.float64)
    din, dw = torch.zeros_like(inp), torch.zeros_like(w)
    for b in range(B):
        for c in range(C):
            for t in range(Tout):
                for j in range(2 * s + 1):
                    u = t + j - s
                    if 0 <= u < Tout:
                        out[b, c, t] += w[j] * inp[b, c, u // s]
                        din[b, c, u // s] += w[j] * dout[b, c, t]
                        dw[j] += inp[b, c, u // s] * dout[b, c, t]
    assert torch.equal(R.upsample_stage_forward(inp, w, s), out)
    got = R.upsample_stage_grads(inp, w, dout, s)
    assert torch.equal(got[0], din) and torch.equal(got[1], dw)


def test_vq_slice_bwd_and_ema_update_against_loops():
    rng = np.random.RandomState(2)
    B, Dtot, d0, D, Tq, K = 2, 5, 1, 3, 4, 4
    lat, quant, dq = _ints(rng, B, Dtot, Tq), _ints(rng, B, Dtot, Tq), _ints(rng, B, Dtot, Tq)
    idx = torch.from_numpy(rng.randint(0, K - 1, size=B * Tq))            # code K-1 stays unused
    c_lat, c_emb = 0.5, 2.0
    dlat, demb = torch.zeros(B, D, Tq, dtype=torch.float64), torch.zeros(K, D, dtype=torch.float64)
    sums = torch.zeros(K, D, dtype=torch.float64)
    for b in range(B):
        for d in range(D):
            for t in range(Tq):
                x, q = lat[b, d0 + d, t], quant[b, d0 + d, t]
                dlat[b, d, t] = dq[b, d0 + d, t] + c_lat * (x - q)
                demb[idx[b * Tq + t], d] += c_emb * (q - x)
                sums[idx[b * Tq + t], d] += x
    got = R.vq_slice_bwd(lat, quant, idx, dq, d0, D, K, c_lat, c_emb)
    assert torch.equal(got[0], dlat) and torch.equal(got[1], demb)
    assert torch.equal(R.vq_slice_bwd(lat, quant, idx, None, d0, D, K, c_lat, c_emb)[0], dlat - dq[:, d0:d0 + D])
    assert R.vq_bwd_coefficients(2, 4, 8, 0.25, 1.0) == (2.0 * 0.25 / 64, 2.0 / 64)
    # EMA update
    hist = torch.bincount(idx, minlength=K)
    n0, w0 = torch.from_numpy(rng.rand(K) + 0.5), torch.from_numpy(rng.randn(K, D))
    decay = 0.5
    n1 = [decay * float(n0[k]) + (1 - decay) * int(hist[k]) for k in range(K)]
    tot = sum(n1)
    n, w, emb = R.vq_ema_update(lat, idx, hist, n0, w0, d0, D, decay)
    for k in range(K):
        nk = (n1[k] + 1e-5) / (tot + K * 1e-5) * tot
        assert abs(float(n[k]) - nk) < 1e-14
        for d in range(D):
            wk = decay * float(w0[k, d]) + (1 - decay) * float(sums[k, d])
            assert abs(float(w[k, d]) - wk) < 1e-14 and abs(float(emb[k, d]) - wk / nk) < 1e-13
    assert int(hist[K - 1]) == 0 and torch.equal(w[K - 1], decay * w0[K - 1])


def test_layout_and_activation_helpers_against_loops():
    rng = np.random.RandomState(3)
    B, C, Cp, T = 3, 2, 4, 5
    a = torch.from_numpy(rng.randn(B, T, Cp))
    got = R.from_btc_scaled(a, C, 0.25)
    assert got.shape == (B, C, T)
    for b in range(B):
        for c in range(C):
            for t in range(T):
                assert got[b, c, t] == a[b, t, c] * 0.25
    x = torch.from_numpy(rng.randn(B, C, T))
    for lengths in (None, [0, 2, T + 5]):
        got = R.to_btc_masked(x, Cp, lengths, 0.5)
        for b in range(B):
            n = T if lengths is None else min(lengths[b], T)
            for t in range(T):
                for c in range(Cp):
                    assert got[b, t, c] == (x[b, c, t] * 0.5 if c < C and t + 1 < n else 0.0)
    y = torch.tensor([-2.0, -0.5, 0.0, 0.25, 0.5])
    d = torch.tensor([3.0, -1.0, 2.0, 4.0, -2.0])
    assert R.act_bwd(y, d, 1, 0.25).tolist() == [0.0, 0.0, 0.0, 4.0, -2.0]
    assert R.act_bwd(y, d, 2, 0.25).tolist() == [0.75, -0.25, 0.5, 4.0, -2.0]
    assert R.act_bwd(y, d, 3, 0.0).tolist() == [3.0 * (1 - 4.0), -1.0 * 0.75, 2.0, 4.0 * (1 - 0.0625), -2.0 * 0.75]
    assert R.act_bwd(y, d, 4, 0.0).tolist() == [3.0 * -6.0, -1.0 * -0.75, 0.0, 4.0 * 0.1875, -2.0 * 0.25]
