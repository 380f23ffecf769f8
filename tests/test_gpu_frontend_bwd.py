"""The front end's backward kernels (csrc/frontend_bwd.hip) and the helpers around frontend_backward (csrc/misc.hip), each called
straight through the C ABI against the float64 restatements of tests/frontend_ref.py.

EXACT cases: every operand (x, w, dy, dout, in, the prefill of accumulated outputs) holds integers drawn uniformly from [-3, 3] and
stored as fp32, and y is the float64 forward of those integers.  Every product and partial sum is then an integer far below 2^24, so
fp32 FMAs, wave / LDS reductions and atomics are exact in ANY order, and the assertion is torch.equal with the float64 reference cast
to fp32 -- no tolerance: one missing, doubled or misplaced term fails.  Each case asserts, from the reference evaluated on absolute
values, that no output's sum of |terms| reaches 2^22.  Many y are exactly 0: the `!(act > 0)` side of the ReLU mask is exercised.
ROUNDING cases (one per entry, Gaussian operands, the entry's largest shape): per element |got - ref64| <= (n + 4) 2^-24 A, n the
number of terms of that output's sum, A the same reference on the absolute values of every operand: the bound of an fp32 sum in any
order, derived and not measured.  Largest err / bound observed on an MI355X: wae_enc_conv_bwd 0.022, wae_upsample_stage_bwd 0.0020,
wae_vq_bwd 0.28, wae_vq_ema_update 0.60 (printed by the tests; run with -s).
BUFFERS: every output sits in the middle of a larger buffer with 1024 sentinel floats on either side, which must stay untouched;
overwritten outputs (dx, din, dlat) start as NaN and must hold none afterwards, accumulated outputs (dw, dbias, demb, the stage's
dw[2s+1]) start from a nonzero integer prefill and must hold prefill + gradient.

Which case reaches which kernel of wae_enc_conv_bwd (CONV_CASES; the tile ET is chosen by Tin: <= 8 -> 8, <= 16 -> 16, else 32):

  (k, stride, pad)   ET = 8 (Tin)   ET = 16 (Tin)   ET = 32 (Tin)           kernel
  (1,1,0)            1, 8           9, 16           17, 33, 70              conv_bwd_xw_tiled_kernel<K,S,PAD,ET>  (dx = NULL:
  (3,1,1)            1, 8           9, 16           17, 32, 33, 70            conv_bwd_w_tiled_kernel<K,S,ET>, the Tin = 9 rows
  (3,1,0)            5, 8           9, 16           17, 33, 70                with 39 x 37 channels and (3,1,1) at Tin = 70)
  (5,2,2)            1, 8           9, 16           17, 32, 33, 70
  (5,1,2)            1, 8           9, 16           17, 33, 70
  (5,1,0)            5, 8           9, 16           17, 33, 70
  (3,2,1) (4,2,1) (7,1,3)   any Tin                                         conv_bwd_x_kernel + conv_bwd_w_kernel (generic)

  Tin = 9 runs B = 11 (eleven (clip, tile) pairs: weight-gradient rounds of 8 + 3; with dx where the block is residual), Tin = 70
  runs B = 3 (nine pairs where Tout = 70: 8 + 1), Cout = 300 (Tin = 16, 33) a second ECB_CH window of 44 channels, Cout = 3 (Tin = 5,
  17) reduction slices without a channel.
wae_upsample_stage_bwd (UP_CASES): s = 4, 5, 8 -> upsample_stage_bwd_kernel<4>, <5>, <8>; s = 1, 2, 3, 16 -> <0>; 320 rows: a block of
the weight gradient walks two rows.  wae_vq_slice_bwd / wae_vq_bwd: vq_bwd_kernel (VQ_CASES, test_vq_bwd_*).
"""
import numpy as np
import pytest
import torch

import frontend_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024            # floats of sentinel on either side of every output
SENT = 12288.0          # (representable in bf16 and fp16 as well)
U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 22


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


class Guarded:
    """A tensor in the middle of a larger buffer: [GUARD sentinels | the tensor, starting as `init` | GUARD sentinels]."""

    def __init__(self, init, dtype=torch.float32):
        n = init.numel()
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init.to(dtype))

    def result(self):
        """-> the tensor on the CPU, after asserting that both guard regions are untouched."""
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[b.numel() - GUARD:] == SENT).all()), "a guard region was written"
        return b[GUARD:b.numel() - GUARD].view(self.t.shape)


def _nan(*shape):
    return torch.full(shape, float("nan"))


def _ints(rng, *shape):
    return torch.from_numpy(rng.randint(-3, 4, size=shape).astype(np.float32))


def _prefill(rng, *shape):
    """nonzero integers in [-3, 3]"""
    return torch.from_numpy(rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=shape))


def _gauss(rng, *shape):
    return torch.from_numpy(rng.randn(*shape).astype(np.float32))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _assert_exact(got, ref, A, what):
    assert not bool(torch.isnan(got).any()), f"{what}: NaN left"
    assert float(A.max()) < EXACT_LIMIT, f"{what}: sum of |terms| {float(A.max())} leaves exact fp32 arithmetic"
    if not torch.equal(got, ref.float()):
        bad = (got != ref.float()).nonzero()
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {first}: got {float(got[first])}, "
                             f"want {float(ref[first])}")


def _assert_bound(got, ref, A, n, what, entry):
    """|got - ref| <= (n + 4) 2^-24 A per element (n: a number or a tensor broadcastable to ref)."""
    assert not bool(torch.isnan(got).any()), f"{what}: NaN left"
    err = (got.double() - ref).abs()
    bound = (torch.as_tensor(n, dtype=torch.float64) + 4.0) * U * A
    assert bool((err[bound == 0] == 0).all()), f"{what}: nonzero where every term is zero"
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    print(f"{entry} {what}: largest err / bound = {ratio:.3g} (largest err {float(err.max()):.3g})")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio}"


# ====================================================================================================== wae_enc_conv_bwd
def _cc(k, s, p, Tin, Cin, Cout, B=1, relu=1, res=0, ynull=0, dxnull=0, dbnull=0):
    return (k, s, p, Tin, Cin, Cout, B, relu, res, ynull, dxnull, dbnull)


TILED = [(1, 1, 0), (3, 1, 1), (3, 1, 0), (5, 2, 2), (5, 1, 2), (5, 1, 0)]
CONV_CASES = []
for _sig in TILED:
    CONV_CASES += [
        _cc(*_sig, 8, 39, 37),                          # ET = 8, the preset's c_in, channels no multiple of 32 or 4
        _cc(*_sig, 9, 39, 37, B=11, dxnull=1),          # ET = 16, the weight-only kernel, eleven (clip, tile) pairs: rounds of 8 + 3
        _cc(*_sig, 16, 33, 300),                        # ET = 16 full, a second ECB_CH window of 44 channels
        _cc(*_sig, 17, 3, 3),                           # ET = 32, two tiles, fewer output channels than reduction slices
        _cc(*_sig, 33, 33, 300, relu=0, ynull=1),       # ET = 32, one step into the second tile, the conv_in / lin form
        _cc(*_sig, 70, 39, 37, B=3),                    # three tiles x three clips: rounds of 8 + 1 where Tout = 70
    ]
CONV_CASES += [_cc(*_sig, 1, 39, 37) for _sig in ((1, 1, 0), (3, 1, 1), (5, 2, 2), (5, 1, 2))]       # Tin = 1 where Tout >= 1
CONV_CASES += [
    _cc(3, 1, 0, 5, 3, 3, relu=0, ynull=1, dbnull=1),   # Tout = 3
    _cc(5, 1, 0, 5, 3, 3),                              # Tout = 1
    _cc(3, 1, 1, 32, 39, 37, relu=0, ynull=1, dbnull=1),    # one full tile, conv_in's calling form (no y, no bias)
    _cc(5, 2, 2, 32, 39, 37),
    _cc(3, 1, 1, 70, 39, 37, B=3, dxnull=1),            # block 0 of the encoder: c_in = 39, dx = NULL
]
for _sig in ((1, 1, 0), (3, 1, 1), (5, 1, 2)):          # residual blocks (shape preserving, Cin == Cout)
    CONV_CASES += [_cc(*_sig, 70, 64, 64, B=3, res=1), _cc(*_sig, 9, 64, 64, B=11, res=1)]
CONV_CASES += [_cc(3, 1, 1, 33, 64, 64, relu=0, res=1, ynull=1)]
CONV_CASES += [                                         # every other shape: the one-thread-per-output kernels
    _cc(3, 2, 1, 1, 39, 37), _cc(3, 2, 1, 9, 39, 37, B=11), _cc(3, 2, 1, 33, 33, 300), _cc(3, 2, 1, 70, 3, 3, B=3, dxnull=1),
    _cc(4, 2, 1, 9, 39, 37, B=11), _cc(4, 2, 1, 17, 33, 300, relu=0, ynull=1), _cc(4, 2, 1, 70, 39, 37, B=3, dbnull=1),
    _cc(7, 1, 3, 1, 39, 37), _cc(7, 1, 3, 9, 64, 64, B=11, res=1), _cc(7, 1, 3, 70, 64, 64, B=3, res=1), _cc(7, 1, 3, 33, 33, 300),
]


def _conv_id(c):
    k, s, p, Tin, Cin, Cout, B, relu, res, ynull, dxnull, dbnull = c
    flags = "".join(f for f, on in (("-relu", relu), ("-res", res), ("-noy", ynull), ("-nodx", dxnull), ("-nodb", dbnull)) if on)
    return f"k{k}s{s}p{p}-T{Tin}-{Cin}x{Cout}-B{B}{flags}"


def test_conv_case_table_covers_every_instantiation():
    """the table of the docstring: each tiled signature at all three tiles, each generic shape, and the listed lengths"""
    for sig in TILED:
        tins = [c[3] for c in CONV_CASES if c[:3] == sig and not c[10]]
        assert any(t <= 8 for t in tins) and any(8 < t <= 16 for t in tins) and any(t > 16 for t in tins), sig
        assert any(c[:3] == sig and c[10] and c[6] > 8 for c in CONV_CASES)               # the weight-only kernel, two rounds
    for sig in ((3, 2, 1), (4, 2, 1), (7, 1, 3)):
        assert any(c[:3] == sig for c in CONV_CASES)
    assert {c[3] for c in CONV_CASES} == {1, 5, 8, 9, 16, 17, 32, 33, 70}
    assert all(R.conv_tout(c[3], c[0], c[1], c[2]) >= 1 for c in CONV_CASES)
    assert all(not c[8] or (c[4] == c[5] and R.conv_tout(c[3], c[0], c[1], c[2]) == c[3]) for c in CONV_CASES)
    assert len(CONV_CASES) <= 66 and len(set(CONV_CASES)) == len(CONV_CASES)


def _call_conv(x, w, y, dy, dx, dw, db, B, Cin, Tin, Cout, k, s, p, relu, res):
    L, lib = _lib()
    return lib.wae_enc_conv_bwd(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(dy), L.ptr(dx), L.ptr(dw), L.ptr(db), B, Cin, Tin, Cout, k, s, p,
                                relu, res, None)


def _run_conv(case, seed, gauss):
    k, s, p, Tin, Cin, Cout, B, relu, res, ynull, dxnull, dbnull = case
    assert not (relu and ynull)
    Tout = R.conv_tout(Tin, k, s, p)
    rng = np.random.RandomState(seed)
    draw = _gauss if gauss else _ints
    x, w, b, dy = draw(rng, B, Cin, Tin), draw(rng, Cout, Cin, k), draw(rng, Cout), draw(rng, B, Cout, Tout)
    y64, mask = R.conv_block_forward(x, w, b, s, p, relu, res)
    y = y64.float()
    if relu:
        stored = R.relu_mask_from_output(y, x, res)         # what the kernels are specified to form
        if gauss:
            mask = stored
        else:
            assert torch.equal(stored, mask)
    else:
        mask = None
    ref = R.conv_block_grads(x, w, dy, s, p, mask, res)
    A = R.conv_block_grads(x.abs(), w.abs(), dy.abs(), s, p, mask, res)
    pre_w, pre_b = _prefill(rng, Cout, Cin, k), _prefill(rng, Cout)
    dx = None if dxnull else Guarded(_nan(B, Cin, Tin))
    dw = Guarded(pre_w)
    db = None if dbnull else Guarded(pre_b)
    rc = _call_conv(_dev(x), _dev(w), None if ynull else _dev(y), _dev(dy), None if dx is None else dx.t, dw.t,
                    None if db is None else db.t, B, Cin, Tin, Cout, k, s, p, relu, res)
    _lib()[0].check(rc, "enc_conv_bwd")
    outs = [("dw", dw.result(), pre_w.double() + ref[1], pre_w.abs().double() + A[1], B * Tout + 1)]
    if dx is not None:
        outs.append(("dx", dx.result(), ref[0], A[0], Cout * k + res))
    if db is not None:
        outs.append(("dbias", db.result(), pre_b.double() + ref[2], pre_b.abs().double() + A[2], B * Tout + 1))
    for name, got, want, a, n in outs:
        if gauss:
            _assert_bound(got, want, a, n, name, "wae_enc_conv_bwd")
        else:
            _assert_exact(got, want, a, name)


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_enc_conv_bwd_exact(case):
    _run_conv(case, 1000 + CONV_CASES.index(case), gauss=False)


def test_enc_conv_bwd_rounding():
    """the largest shape of the table, Gaussian operands; the mask is the one the stored fp32 y gives"""
    _run_conv(_cc(5, 1, 2, 70, 33, 300, B=3), 77, gauss=True)


def test_enc_conv_bwd_refuses_relu_without_y():
    """WAE_REQUIRE(!relu || y) returns before any launch: a nonzero code, the message, and nothing written"""
    L, lib = _lib()
    rng = np.random.RandomState(5)
    B, Cin, Tin, Cout, k = 2, 8, 9, 8, 3
    x, w, dy = _ints(rng, B, Cin, Tin), _ints(rng, Cout, Cin, k), _ints(rng, B, Cout, Tin)
    pre_w, pre_b = _prefill(rng, Cout, Cin, k), _prefill(rng, Cout)
    dx, dw, db = Guarded(_nan(B, Cin, Tin)), Guarded(pre_w), Guarded(pre_b)
    rc = _call_conv(_dev(x), _dev(w), None, _dev(dy), dx.t, dw.t, db.t, B, Cin, Tin, Cout, k, 1, 1, 1, 0)
    assert rc != 0
    assert "relu needs the forward output y" in lib.wae_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.result()).all()) and torch.equal(dw.result(), pre_w) and torch.equal(db.result(), pre_b)


# ================================================================================================ wae_upsample_stage_bwd
#            s, Tin, B, C
UP_CASES = [(4, 255, 2, 128), (4, 1, 1, 3), (4, 513, 5, 64),
            (5, 257, 5, 64), (5, 2, 1, 3), (5, 256, 2, 128),
            (8, 256, 2, 128), (8, 513, 1, 3), (8, 1, 5, 64),
            (1, 513, 5, 64), (1, 1, 1, 3), (2, 257, 2, 128), (2, 255, 1, 3), (3, 256, 5, 64), (3, 1, 2, 128),
            (16, 513, 1, 3), (16, 2, 5, 64), (16, 255, 1, 3), (16, 257, 5, 64)]


def _call_up(dout, inp, w, din, dw, B, C, Tin, s):
    L, lib = _lib()
    return lib.wae_upsample_stage_bwd(L.ptr(dout), L.ptr(inp), L.ptr(w), L.ptr(din), L.ptr(dw), B, C, Tin, s, None)


def _run_up(case, seed, gauss):
    s, Tin, B, C = case
    rng = np.random.RandomState(seed)
    draw = _gauss if gauss else _ints
    inp, w, dout = draw(rng, B, C, Tin), draw(rng, 2 * s + 1), draw(rng, B, C, Tin * s)
    ref = R.upsample_stage_grads(inp, w, dout, s)
    A = R.upsample_stage_grads(inp.abs(), w.abs(), dout.abs(), s)
    pre = _prefill(rng, 2 * s + 1)
    din, dw = Guarded(_nan(B, C, Tin)), Guarded(pre)
    _lib()[0].check(_call_up(_dev(dout), _dev(inp), _dev(w), din.t, dw.t, B, C, Tin, s), "upsample_stage_bwd")
    for name, got, want, a, n in (("din", din.result(), ref[0], A[0], s * (2 * s + 1)),
                                  ("dw", dw.result(), pre.double() + ref[1], pre.abs().double() + A[1], B * C * Tin * s + 1)):
        if gauss:
            _assert_bound(got, want, a, n, name, "wae_upsample_stage_bwd")
        else:
            _assert_exact(got, want, a, name)


def test_upsample_case_table_covers_every_template():
    assert {c[0] for c in UP_CASES} == {4, 5, 8, 1, 2, 3, 16}
    assert {c[1] for c in UP_CASES} == {1, 2, 255, 256, 257, 513}
    assert {c[2:] for c in UP_CASES} == {(1, 3), (5, 64), (2, 128)}
    for s in (4, 5, 8):                                   # every template: a row count above, at and below the 256 blocks
        assert {c[2:] for c in UP_CASES if c[0] == s} == {(1, 3), (5, 64), (2, 128)}
    assert any(c[0] in (1, 2, 3, 16) and c[2:] == (5, 64) and c[1] > 256 for c in UP_CASES)      # generic form, two rows per block


@pytest.mark.parametrize("case", UP_CASES, ids=lambda c: "s%d-T%d-B%dC%d" % c)
def test_upsample_stage_bwd_exact(case):
    _run_up(case, 2000 + UP_CASES.index(case), gauss=False)


def test_upsample_stage_bwd_rounding():
    _run_up((16, 257, 5, 64), 78, gauss=True)


def test_upsample_stage_bwd_refuses_scale_17():
    """WAE_REQUIRE(2 s + 1 <= 33) returns before any launch"""
    L, lib = _lib()
    rng = np.random.RandomState(6)
    s, Tin, B, C = 17, 4, 1, 3
    inp, w, dout = _ints(rng, B, C, Tin), _ints(rng, 2 * s + 1), _ints(rng, B, C, Tin * s)
    pre = _prefill(rng, 2 * s + 1)
    din, dw = Guarded(_nan(B, C, Tin)), Guarded(pre)
    rc = _call_up(_dev(dout), _dev(inp), _dev(w), din.t, dw.t, B, C, Tin, s)
    assert rc != 0
    assert "scale 17" in lib.wae_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(din.result()).all()) and torch.equal(dw.result(), pre)


# ============================================================================================ wae_vq_slice_bwd, wae_vq_bwd
def _run_vq(B, Dtot, d0, D, Tq, K, idx, c_lat, c_emb, seed, gauss, with_demb=True, with_dquant=True, whole=None):
    """whole = (beta, loss_scale): through wae_vq_bwd (d0 = 0, D = Dtot), whose coefficients the entry forms itself."""
    L, lib = _lib()
    rng = np.random.RandomState(seed)
    draw = _gauss if gauss else _ints
    lat, quant, dq = draw(rng, B, Dtot, Tq), draw(rng, B, Dtot, Tq), draw(rng, B, Dtot, Tq)
    out = torch.ones(Dtot, dtype=torch.bool)
    out[d0:d0 + D] = False
    lat[:, out] += 1000.0                                  # outside the slice: values that would show if read
    quant[:, out] -= 1000.0
    dq[:, out] += 500.0
    ref = R.vq_slice_bwd(lat, quant, idx, dq if with_dquant else None, d0, D, K, c_lat, c_emb)
    A = [a.abs() for a in R.vq_slice_bwd(lat.abs(), -quant.abs(), idx, dq.abs() if with_dquant else None, d0, D, K, c_lat, c_emb)]
    pre = _prefill(rng, K, D)
    dlat = Guarded(_nan(B, Dtot, Tq))
    demb = Guarded(pre) if with_demb else None
    ins = [_dev(lat), _dev(quant), _dev(idx), _dev(dq) if with_dquant else None]      # (held until the results are read)
    args = [L.ptr(t) for t in ins] + [L.ptr(dlat.t), None if demb is None else L.ptr(demb.t)]
    if whole is None:
        L.check(lib.wae_vq_slice_bwd(*args, B, Dtot, d0, D, Tq, c_lat, c_emb, None), "vq_slice_bwd")
    else:
        L.check(lib.wae_vq_bwd(*args, B, D, Tq, whole[0], whole[1], None), "vq_bwd")
    got = dlat.result()
    assert bool(torch.isnan(got[:, out]).all()), "dlat outside the slice was written"
    counts = torch.bincount(idx, minlength=K).double()
    outs = [("dlat", got[:, d0:d0 + D], ref[0], A[0], 3)]
    if demb is not None:
        outs.append(("demb", demb.result(), pre.double() + ref[1], pre.abs().double() + A[1], (2 * counts + 1)[:, None]))
        unused = counts == 0
        assert torch.equal(outs[1][1][unused], pre[unused])          # rows of unused codes keep the prefill
    quantum = min(1.0, c_lat, c_emb)                                 # every value is an integer multiple of it
    for name, g, want, a, n in outs:
        if gauss:
            _assert_bound(g, want, a, n, name, "wae_vq_bwd")
        else:
            _assert_exact(g, want, a / quantum, name)


#            name: (idx of (B * Tq,) for K = 9, demb, dquant)
VQ_CASES = ["slice", "no_demb", "no_dquant", "one_code"]


@pytest.mark.parametrize("case", VQ_CASES)
def test_vq_slice_bwd_exact(case):
    """channels [3, 8) of 12, B D Tq = 3 * 5 * 37 = 555 (no multiple of 256), c_lat = 1/2 and c_emb = 2: exact.  Codes 6..8 of the 9
    stay unused; `one_code`: every frame names code 4, so every atomic of a column lands on one address."""
    B, Dtot, d0, D, Tq, K = 3, 12, 3, 5, 37, 9
    rng = np.random.RandomState(31)
    idx = torch.full((B * Tq,), 4, dtype=torch.int64) if case == "one_code" else torch.from_numpy(rng.randint(0, 6, size=B * Tq))
    _run_vq(B, Dtot, d0, D, Tq, K, idx, 0.5, 2.0, 3000 + VQ_CASES.index(case), gauss=False, with_demb=case != "no_demb",
            with_dquant=case != "no_dquant")


def test_vq_bwd_exact():
    """B D Tq = 2 * 16 * 32 = 2^10, beta = 1/4, loss_scale = 1: both coefficients are powers of two"""
    B, D, Tq, K = 2, 16, 32, 8
    idx = torch.from_numpy(np.random.RandomState(32).randint(0, K - 1, size=B * Tq))
    c_lat, c_emb = R.vq_bwd_coefficients(B, D, Tq, 0.25, 1.0)
    assert (c_lat, c_emb) == (2.0 ** -11, 2.0 ** -9)
    _run_vq(B, D, 0, D, Tq, K, idx, c_lat, c_emb, 3100, gauss=False, whole=(0.25, 1.0))


def test_vq_bwd_rounding():
    B, D, Tq, K = 3, 64, 37, 32
    idx = torch.from_numpy(np.random.RandomState(33).randint(0, K, size=B * Tq))
    c_lat, c_emb = R.vq_bwd_coefficients(B, D, Tq, 0.25, 1024.0)
    _run_vq(B, D, 0, D, Tq, K, idx, c_lat, c_emb, 3200, gauss=True, whole=(0.25, 1024.0))


# ==================================================================================== the helpers around frontend_backward
DTYPES = ["fp32", "bf16", "fp16"]
LAYOUT_T = (1, 63, 64, 65, 130)


def _dtype(name):
    L, _ = _lib()
    return dict(fp32=(torch.float32, L.WAE_F32), bf16=(torch.bfloat16, L.WAE_BF16), fp16=(torch.float16, L.WAE_F16))[name]


@pytest.mark.parametrize("C,Cp", [(64, 64), (39, 64), (80, 128)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_from_btc_scaled(dtype, C, Cp):
    L, lib = _lib()
    td, dt = _dtype(dtype)
    B, scale = 2, 1.0 / 1024
    rng = np.random.RandomState(41)
    for T in LAYOUT_T:
        inp = _gauss(rng, B, T, Cp).to(td)
        out, src = Guarded(_nan(B, C, T)), _dev(inp)
        L.check(lib.wae_from_btc_scaled(L.ptr(src), L.ptr(out.t), B, C, T, Cp, dt, scale, None), "from_btc_scaled")
        assert torch.equal(out.result(), R.from_btc_scaled(inp, C, scale).float()), T


@pytest.mark.parametrize("C,Cp", [(64, 64), (39, 64), (80, 128)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_to_btc_masked(dtype, C, Cp):
    L, lib = _lib()
    td, dt = _dtype(dtype)
    scale = 0.25
    rng = np.random.RandomState(42)
    for T in LAYOUT_T:
        for lengths in (None, [0, 1, 2, T, T + 5, max(T // 2, 1)]):
            B = 2 if lengths is None else len(lengths)
            inp = _gauss(rng, B, C, T)
            out, src = Guarded(_nan(B, T, Cp), td), _dev(inp)
            ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
            L.check(lib.wae_to_btc_masked(L.ptr(src), L.ptr(out.t), B, C, T, Cp, dt, L.ptr(ln), scale, None), "to_btc_masked")
            # (a power of two times an fp32 value: the float64 product IS the fp32 product)
            assert torch.equal(out.result(), R.to_btc_masked(inp, Cp, lengths, scale).float().to(td)), (T, lengths)


ACT_N = (1, 255, 256, 257, 4096 * 256 + 3)     # the last: one past the grid cap, so the grid-stride loop runs


@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_act_bwd(kind):
    L, lib = _lib()
    rng = np.random.RandomState(43 + kind)
    slope = 0.25
    for n in ACT_N:
        if kind <= 2:
            y, d0 = _ints(rng, n), _ints(rng, n)         # exact zeros and negatives in y
        else:
            z = _gauss(rng, n)
            y, d0 = (torch.tanh(z) if kind == 3 else torch.sigmoid(z)), _gauss(rng, n)
        d, yd = Guarded(d0), _dev(y)
        L.check(lib.wae_act_bwd(L.ptr(yd), L.ptr(d.t), n, kind, slope, None), "act_bwd")
        got, ref = d.result(), R.act_bwd(y, d0, kind, slope)
        if kind <= 2:
            assert torch.equal(got, ref.float()), n
        else:
            assert bool(((got.double() - ref).abs() <= 4 * U * ref.abs().clamp(min=1.0)).all()), n


@pytest.mark.parametrize("decay", [0.5, 0.99])
@pytest.mark.parametrize("K", [5, 300])
def test_vq_ema_update(K, decay):
    """channels [7, 77) of 80 (D = 70: more than the 64 lanes), 150 frames, codes with a zero count, in place on all three buffers"""
    L, lib = _lib()
    B, Dtot, d0, D, Tq = 3, 80, 7, 70, 50
    rng = np.random.RandomState(50 + K)
    lat = _gauss(rng, B, Dtot, Tq)
    idx = torch.from_numpy(rng.randint(0, K - 1, size=B * Tq))          # the last code (and at K = 300 many more) is never named
    counts = torch.bincount(idx, minlength=K)
    assert int((counts == 0).sum()) >= 1
    hist = torch.cat([counts, torch.zeros(1, dtype=torch.int64)]).to(torch.int32)
    n0, w0, e0 = torch.from_numpy((rng.rand(K) + 0.5).astype(np.float32)), _gauss(rng, K, D), _gauss(rng, K, D)
    dec = float(np.float32(decay))                                      # the value the entry receives
    ref = R.vq_ema_update(lat, idx, hist, n0, w0, d0, D, dec)
    A = R.vq_ema_update(lat.abs(), idx, hist, n0, w0.abs(), d0, D, dec)
    n, w, e = Guarded(n0), Guarded(w0), Guarded(e0)
    ins = [_dev(lat), _dev(idx), _dev(hist)]
    L.check(lib.wae_vq_ema_update(L.ptr(ins[0]), L.ptr(ins[1]), L.ptr(ins[2]), L.ptr(n.t), L.ptr(w.t), L.ptr(e.t), B, Dtot,
                                  d0, D, Tq, K, decay, None), "vq_ema_update")
    nmax = int(counts.max())
    for name, got, want, a in (("cluster_size", n.result(), ref[0], A[0]), ("ema_w", w.result(), ref[1], A[1]),
                               ("emb", e.result(), ref[2], A[2])):
        _assert_bound(got, want, a, nmax, name, "wae_vq_ema_update")


# ================================================================================================== one composition check
def test_frontend_backward_composed_every_element():
    """A train step of golden model A (fp32) at B = 3, F = 37 feature frames: the encoder blocks see 37, 37, 19 and 10 frames (no
    multiple of their tiles, odd lengths into both stride-2 blocks, weight-gradient rounds that are not full), and EVERY element of
    every front-end parameter gradient is compared with float64 autograd through the oracle (vqvae_forward: encoder_forward,
    vq_forward, upsample_forward, the teacher-forced stack; the same loss, masked CE + vq_loss) under the per-tensor rule of
    test_vqwae_full_geometry_train_step_fp32: 2e-3 of the tensor's largest gradient plus its floors.  No piece is left out: the
    oracle is differentiable end to end (the quantiser through its straight-through form)."""
    from helpers import golden_model
    from oracle import wae_oracle as O
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, ins, z, ocfg = golden_model("A")
    B, Fr = 3, 37
    Tq = R.conv_tout(R.conv_tout(Fr, 5, 2, 2), 5, 2, 2)
    assert Tq == 10
    T = Tq * int(np.prod(cfg["upsample_scales"]))
    c = O.hash_fill((B, cfg["c_in"], Fr), 9101, 1.7)
    x = ((O.hash_fill((B, T), 9102) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
    g = ((O.hash_fill((B,), 9103) * 0.5 + 0.5) * cfg["n_speakers"]).long().clamp(0, cfg["n_speakers"] - 1)
    lengths = torch.tensor([T, T - 137, T // 2 + 3])
    # float64 autograd through the oracle
    sd64 = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    xin = torch.nn.functional.one_hot(x, cfg["O"]).double().transpose(1, 2).contiguous()
    y_hat, vq_loss, perp, aux = O.vqvae_forward(sd64, dict(ocfg, beta=cfg.get("beta", 0.25)), xin, c.double(), g)
    ce = O.masked_ce_loss(y_hat, x.unsqueeze(-1), lengths)
    (ce + vq_loss).backward()
    ce, vq_loss = ce.detach(), vq_loss.detach()
    # the engine's step
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    eng.init_optimizer()
    seen = {}
    res = eng.train_step(x.cuda(), c.cuda(), g.cuda(), lengths=lengths.cuda(), lr=4e-4, clip_thresh=100.0, ema_decay=0.9999,
                         grad_hook=lambda gr: seen.update(g=gr.clone()))
    torch.cuda.synchronize()
    assert np.array_equal(eng.saved.idx.cpu().numpy().reshape(-1), aux["idx"].numpy().reshape(-1))
    assert abs(float(res["ce"]) - float(ce)) < 1e-4 * float(ce)
    assert abs(float(res["vq_loss"]) - float(vq_loss)) < 1e-5 * max(1.0, float(vq_loss))
    grads = seen["g"].cpu()
    front = [k for k in sd if k.startswith(("encoder.", "vq.", "wavenet.upsample_net."))]
    assert len(front) == 32
    bad = {}
    for k in front:
        o, n = eng.lay.off(k), eng.lay.numel(k)
        want = sd64[k].grad.reshape(-1)
        gmax = float(want.abs().max())
        assert gmax > 0, k
        err = (grads[o:o + n].double() - want).abs()
        floor = 1e-7 if k.endswith("weight_g") else 2e-8
        if float(err.max()) > 2e-3 * gmax + floor:
            bad[k] = (float(err.max()), gmax, int(err.argmax()))
    assert not bad, bad
