"""The list forms of the front end's backward (csrc/frontend_bwd_list.hip), each entry called alone through the C ABI against the
float64 references of tests/frontend_list_ref.py: frontend_ref.py's functions per item, the weight gradients summed over the items.

EXACT cases, as tests/test_gpu_frontend_bwd.py: every operand holds integers from [-3, 3], so every product and partial sum is an
integer far below 2^24, fp32 arithmetic is exact in any order (tile order, atomics, wave reductions), and the assertion is
torch.equal.  One list holds items of Tin = 1, 2, 7, 8, 9, 31, 32, 33, 65 (conv) or 1, 2, 3, 17, 65, 129 (upsample stage: Tin * s
crosses the 256-column tile).  The items lie in a shuffled order with gap columns between them (offsets not monotone); the gap columns
of every input hold 2^20, so a neighbour's column read in the place of an item's own zero padding shows in the element that read
it; every overwritten output is prefilled with a sentinel that must survive outside every item; accumulated outputs start from a
nonzero integer prefill.
ROUNDING cases, one per entry: Gaussian operands, |got - ref64| <= (n + 4) 2^-24 A per element -- n the number of terms of the
output's sum, A the reference on absolute values (the bound of an fp32 sum in any order, derived and not measured).
"""
import itertools

import numpy as np
import pytest
import torch

import frontend_list_ref as RL
import frontend_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 12288.0
U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 22
CONV_TINS = [1, 2, 7, 8, 9, 31, 32, 33, 65]
UP_TINS = [1, 2, 3, 17, 65, 129]


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


def _P():
    from wavenet_autoencoders_amd import packing
    return packing


def _ints(rng, *shape):
    return torch.from_numpy(rng.randint(-3, 4, size=shape).astype(np.float32))


def _prefill(rng, *shape):
    return torch.from_numpy(rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=shape))


def _gauss(rng, *shape):
    return torch.from_numpy(rng.randn(*shape).astype(np.float32))


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _check(got, ref, A, n, what, gauss, entry):
    assert not bool(torch.isnan(got).any()), f"{what}: NaN"
    if not gauss:
        assert float(A.max()) < EXACT_LIMIT, f"{what}: sum of |terms| {float(A.max())} leaves exact fp32 arithmetic"
        if not torch.equal(got, ref.float()):
            bad = (got != ref.float()).nonzero()
            first = tuple(bad[0].tolist())
            raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ, first at {first}: got {float(got[first])}, "
                                 f"want {float(ref[first])}")
        return
    err = (got.double() - ref).abs()
    bound = (torch.as_tensor(n, dtype=torch.float64) + 4.0) * U * A
    assert bool((err[bound == 0] == 0).all()), f"{what}: nonzero where every term is zero"
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    print(f"{entry} {what}: largest err / bound = {ratio:.3g} (largest err {float(err.max()):.3g})")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio}"


def _check_items(packed, refs, As, offs, pitch, n, what, gauss, entry, skip=()):
    """every item's columns of a packed output against its reference; the sentinel everywhere else (skipped items included)"""
    keep = torch.ones(pitch, dtype=torch.bool)
    for i, (ref, o) in enumerate(zip(refs, offs)):
        if i in skip:
            continue
        T = ref.shape[1]
        keep[int(o):int(o) + T] = False
        _check(packed[:, int(o):int(o) + T], ref, As[i], n, f"{what} of item {i} (T {T})", gauss, entry)
    assert bool((packed[:, keep] == SENT).all()), f"{what}: a column outside every item was written"


# ================================================================================================== wae_enc_conv_bwd_list
KS = [(1, 1), (3, 1), (5, 2), (5, 1)]
CHANS = [(5, 33), (32, 32), (39, 32)]
ETS = [8, 16, 32]
CONV_CASES = [(k, s, ci, co, et, (a + b + c) % 2, 0) for (a, (k, s)), (b, (ci, co)), (c, et)
              in itertools.product(enumerate(KS), enumerate(CHANS), enumerate(ETS))]
CONV_CASES += [(k, s, ci, co, et, 1 - relu, 0) for k, s, ci, co, et, relu, _ in CONV_CASES if et == 32 and (ci, co) != (5, 33)]
CONV_CASES += [(3, 1, 39, 32, 16, 1, 1)]       # dx = NULL: the encoder's first block


def _conv_id(c):
    k, s, ci, co, et, relu, dxnull = c
    return f"k{k}s{s}-{ci}x{co}-et{et}" + ("-relu" if relu else "") + ("-nodx" if dxnull else "")


def test_conv_case_table():
    for ks in KS:
        for ch in CHANS:
            mine = [c for c in CONV_CASES if c[:2] == ks and c[2:4] == ch]
            assert {c[4] for c in mine} == {8, 16, 32}
        assert {c[5] for c in CONV_CASES if c[:2] == ks and c[2:4] == (32, 32) and c[4] == 32} == {0, 1}
    assert sum(c[6] for c in CONV_CASES) == 1


def _conv_tables(Tin, k, s, pad, et, in_off, out_off, rng=None):
    segs, tiles, et, Tout = _P().enc_list_tables(Tin, k, s, pad, et)
    segs = segs.copy()
    segs[:, 0], segs[:, 2] = in_off, out_off
    if rng is not None:
        tiles = tiles[rng.permutation(len(tiles))]
    return segs, np.ascontiguousarray(tiles), Tout


def _call_conv(x, w, y, dy, dx, dw, db, segs, tiles, et, in_pitch, out_pitch, Cin, Cout, k, s, pad, relu, res):
    L, lib = _lib()
    sd, td = torch.from_numpy(segs).to(DEV), torch.from_numpy(tiles).to(DEV)
    rc = lib.wae_enc_conv_bwd_list(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(dy), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(sd), len(segs), L.ptr(td),
                                   len(tiles), et, in_pitch, out_pitch, Cin, Cout, k, s, pad, relu, res, None)
    torch.cuda.synchronize()
    return rc


def _run_conv(case, seed, gauss=False, pad=None, tins=CONV_TINS, bad=None, shuffle=True):
    k, s, Cin, Cout, et, relu, dxnull = case
    pad = k // 2 if pad is None else pad
    res = int(s == 1 and Cin == Cout and 2 * pad == k - 1)
    rng = np.random.RandomState(seed)
    draw = _gauss if gauss else _ints
    Tin = np.asarray(tins)
    Tout = (Tin + 2 * pad - k) // s + 1
    in_off, in_pitch = RL.scattered_offsets(Tin, rng)
    out_off, out_pitch = RL.scattered_offsets(Tout, rng)
    xs = [draw(rng, Cin, int(t)) for t in Tin]
    dys = [draw(rng, Cout, int(t)) for t in Tout]
    w, b = draw(rng, Cout, Cin, k), draw(rng, Cout)
    ys64, masks = RL.conv_list_forward(xs, w, b, s, pad, relu, res)
    ys = [y.float() for y in ys64]
    if relu:
        stored = [R.relu_mask_from_output(y[None], x[None], res)[0] for y, x in zip(ys, xs)]
        if gauss:
            masks = stored
        else:
            assert all(torch.equal(a, m) for a, m in zip(stored, masks))
    else:
        masks = None
    skip = () if bad is None else (bad,)
    ref = RL.conv_list_grads(xs, w, dys, s, pad, masks, res, skip)
    A = RL.conv_list_grads([x.abs() for x in xs], w.abs(), [d.abs() for d in dys], s, pad, masks, res, skip)
    segs, tiles, _ = _conv_tables(Tin, k, s, pad, et, in_off, out_off, rng if shuffle else None)
    if bad is not None:
        segs[bad, 0] = in_pitch - int(Tin[bad]) + 1        # one column beyond the pitch
    pre_w, pre_b = _prefill(rng, Cout, Cin, k), _prefill(rng, Cout)
    x, dy = _dev(RL.pack(xs, in_off, in_pitch, RL.GAP_FILL)), _dev(RL.pack(dys, out_off, out_pitch, RL.GAP_FILL))
    y = _dev(RL.pack(ys, out_off, out_pitch, RL.GAP_FILL)) if relu else None
    dx = None if dxnull else torch.full((Cin, in_pitch), SENT, device=DEV)
    dw, db = _dev(pre_w), _dev(pre_b)
    rc = _call_conv(x, _dev(w), y, dy, dx, dw, db, segs, tiles, et, in_pitch, out_pitch, Cin, Cout, k, s, pad, relu, res)
    _lib()[0].check(rc, "enc_conv_bwd_list")
    n_w = int(Tout.sum()) + 1
    _check(dw.cpu(), pre_w.double() + ref[1], pre_w.abs().double() + A[1], n_w, "dw", gauss, "wae_enc_conv_bwd_list")
    _check(db.cpu(), pre_b.double() + ref[2], pre_b.abs().double() + A[2], n_w, "dbias", gauss, "wae_enc_conv_bwd_list")
    if dx is not None:
        _check_items(dx.cpu(), ref[0], A[0], in_off, in_pitch, Cout * k + res, "dx", gauss, "wae_enc_conv_bwd_list", skip)


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_enc_conv_bwd_list_exact(case):
    _run_conv(case, 3000 + CONV_CASES.index(case))


@pytest.mark.parametrize("k", [3, 5])
def test_enc_conv_bwd_list_conv_in_form(k):
    """conv_in's calling form: pad 0, no ReLU, Cin == Cout, items of at least k frames (the last tile of an item owns the k - 1
    input steps beyond Tout * stride)"""
    _run_conv((k, 1, 16, 16, 16, 0, 0), 3100 + k, pad=0, tins=[5, 6, 7, 16, 17, 20, 21, 33, 40])


def test_enc_conv_bwd_list_tile_order_does_not_matter():
    """the same list with the tiles in table order and shuffled: the same integers"""
    _run_conv((5, 2, 39, 32, 8, 1, 0), 3200, shuffle=False)
    _run_conv((5, 2, 39, 32, 8, 1, 0), 3200, shuffle=True)


def test_enc_conv_bwd_list_rounding():
    _run_conv((5, 1, 39, 32, 32, 1, 0), 79, gauss=True)


def test_enc_conv_bwd_list_skips_a_bad_record():
    """an item whose columns end beyond in_pitch: nothing of it in dw / dbias, its dx columns keep the sentinel, the rest is whole"""
    _run_conv((3, 1, 32, 32, 16, 1, 0), 3300, bad=4)


def test_enc_conv_bwd_list_refusals():
    """every refusal returns before any launch: a nonzero code and nothing written"""
    L, lib = _lib()
    rng = np.random.RandomState(7)
    Cin = Cout = 8
    Tin = np.asarray([4, 9])
    segs, tiles, _ = _conv_tables(Tin, 3, 1, 1, 8, [0, 4], [0, 4])
    x, w, dy = _dev(_ints(rng, Cin, 13)), _dev(_ints(rng, Cout, Cin, 7)), _dev(_ints(rng, Cout, 13))
    pre = _prefill(rng, Cout, Cin, 7)
    for kw, msg in ((dict(y=None, relu=1), "relu needs"), (dict(k=7), "no list kernel"), (dict(k=3, s=2), "no list kernel"),
                    (dict(et=12), "et 12"), (dict(in_pitch=0), "pitches"), (dict(res=1, Cout=4), "residual"), (dict(ntiles=0), "tile table")):
        a = dict(y=x, relu=0, k=3, s=1, et=8, in_pitch=13, res=0, Cout=Cout, ntiles=len(tiles))
        a.update(kw)
        dx, dw, db = torch.full((Cin, 13), SENT, device=DEV), _dev(pre), torch.full((Cout,), SENT, device=DEV)
        sd, td = torch.from_numpy(segs).to(DEV), torch.from_numpy(tiles).to(DEV)
        rc = lib.wae_enc_conv_bwd_list(L.ptr(x), L.ptr(w), L.ptr(a["y"]), L.ptr(dy), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(sd), len(segs),
                                       L.ptr(td), a["ntiles"], a["et"], a["in_pitch"], 13, Cin, a["Cout"], a["k"], a["s"], a["k"] // 2,
                                       a["relu"], a["res"], None)
        assert rc != 0 and msg in lib.wae_last_error().decode(), (kw, rc, lib.wae_last_error().decode())
        torch.cuda.synchronize()
        assert bool((dx == SENT).all()) and bool((db == SENT).all()) and torch.equal(dw.cpu(), pre), kw


# ============================================================================================ wae_upsample_stage_bwd_list
UP_CASES = list(itertools.product([4, 5, 8, 16], [3, 16])) + [(1, 3), (3, 16)]


def _call_up(dout, inp, w, din, dw, recs, ntiles, in_pitch, out_pitch, C, s):
    L, lib = _lib()
    rd = torch.from_numpy(recs).to(DEV)
    rc = lib.wae_upsample_stage_bwd_list(L.ptr(dout), L.ptr(inp), L.ptr(w), L.ptr(din), L.ptr(dw), L.ptr(rd), len(recs) - 1, ntiles, in_pitch,
                                         out_pitch, C, s, None)
    torch.cuda.synchronize()
    return rc


def _run_up(s, C, seed, gauss=False, bad=None):
    P = _P()
    rng = np.random.RandomState(seed)
    draw = _gauss if gauss else _ints
    Tin = np.asarray(UP_TINS)
    Tout = Tin * s
    in_off, in_pitch = RL.scattered_offsets(Tin, rng)
    out_off, out_pitch = RL.scattered_offsets(Tout, rng)
    ins = [draw(rng, C, int(t)) for t in Tin]
    douts = [draw(rng, C, int(t)) for t in Tout]
    w = draw(rng, 2 * s + 1)
    skip = () if bad is None else (bad,)
    ref = RL.upsample_list_grads(ins, w, douts, s, skip)
    A = RL.upsample_list_grads([x.abs() for x in ins], w.abs(), [d.abs() for d in douts], s, skip)
    recs, ntiles = P.ups_list_records(in_off, Tin, out_off, Tout, P.UPS_LIST_TILE_CT)
    if bad is not None:
        recs = recs.copy()
        recs[bad, 2] = out_pitch - int(Tout[bad]) + 1      # one column beyond the pitch
    pre = _prefill(rng, 2 * s + 1)
    din, dw = torch.full((C, in_pitch), SENT, device=DEV), _dev(pre)
    rc = _call_up(_dev(RL.pack(douts, out_off, out_pitch, RL.GAP_FILL)), _dev(RL.pack(ins, in_off, in_pitch, RL.GAP_FILL)), _dev(w), din, dw,
                  recs, ntiles, in_pitch, out_pitch, C, s)
    _lib()[0].check(rc, "upsample_stage_bwd_list")
    _check(dw.cpu(), pre.double() + ref[1], pre.abs().double() + A[1], C * int(Tout.sum()) + 1, "dw", gauss, "wae_upsample_stage_bwd_list")
    _check_items(din.cpu(), ref[0], A[0], in_off, in_pitch, s * (2 * s + 1), "din", gauss, "wae_upsample_stage_bwd_list", skip)


@pytest.mark.parametrize("s,C", UP_CASES, ids=lambda v: str(v))
def test_upsample_stage_bwd_list_exact(s, C):
    _run_up(s, C, 4000 + 17 * s + C)


def test_upsample_stage_bwd_list_rounding():
    _run_up(16, 16, 80, gauss=True)


def test_upsample_stage_bwd_list_skips_a_bad_record():
    _run_up(5, 16, 4100, bad=3)


def test_upsample_stage_bwd_list_refusals():
    L, lib = _lib()
    P = _P()
    rng = np.random.RandomState(8)
    C, Tin = 3, np.asarray([2, 3])
    for s, kw, msg in ((17, {}, "scale 17"), (4, dict(ntiles=0), "ntiles"), (4, dict(out_pitch=0), "pitches"), (4, dict(nsegs=0), "table")):
        recs, ntiles = P.ups_list_records([0, 2], Tin, [0, 2 * s], Tin * s, P.UPS_LIST_TILE_CT)
        a = dict(ntiles=ntiles, out_pitch=5 * s, nsegs=2)
        a.update(kw)
        pre = _prefill(rng, 2 * s + 1)
        din, dw = torch.full((C, 5), SENT, device=DEV), _dev(pre)
        dout, inp, w, rd = _dev(_ints(rng, C, 5 * s)), _dev(_ints(rng, C, 5)), _dev(_ints(rng, 2 * s + 1)), torch.from_numpy(recs).to(DEV)
        rc = lib.wae_upsample_stage_bwd_list(L.ptr(dout), L.ptr(inp), L.ptr(w), L.ptr(din), L.ptr(dw), L.ptr(rd), a["nsegs"], a["ntiles"], 5,
                                             a["out_pitch"], C, s, None)
        assert rc != 0 and msg in lib.wae_last_error().decode(), (s, kw, lib.wae_last_error().decode())
        torch.cuda.synchronize()
        assert bool((din == SENT).all()) and torch.equal(dw.cpu(), pre), (s, kw)


# ====================================================================================================== wae_from_btc_list
FB_TS = [1, 63, 64, 65, 130]
DTYPES = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16), "fp16": (2, torch.float16)}


def _fb_setup(rng, C, Cp, tdt):
    P = _P()
    T = np.asarray(FB_TS)
    col_off, pitch = RL.scattered_offsets(T, rng)
    row_off, rows = RL.scattered_offsets(T, rng)
    src = torch.full((rows, Cp), RL.GAP_FILL if tdt == torch.float32 else 16384.0)
    own = RL.owned(row_off, T, rows)
    src[own] = _ints(rng, int(own.sum()), Cp)             # the pad channels hold values too: they must not be read into a channel
    recs, ntiles = P.ups_list_records(col_off, T, row_off, T, P.UPS_LIST_TILE_BTC)
    return T, col_off, pitch, row_off, rows, src.to(tdt), recs, ntiles


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("C,Cp", [(5, 8), (70, 96)], ids=["C5p8", "C70p96"])
def test_from_btc_list_exact_and_round_trip(dtype, C, Cp):
    L, lib = _lib()
    dt, tdt = DTYPES[dtype]
    rng = np.random.RandomState(5000 + dt + C)
    T, col_off, pitch, row_off, rows, src, recs, ntiles = _fb_setup(rng, C, Cp, tdt)
    want = RL.from_btc_list(src, row_off, T, C, 0.5)
    out = torch.full((C, pitch), SENT, device=DEV)
    sd, rd = _dev(src), torch.from_numpy(recs).to(DEV)
    L.check(lib.wae_from_btc_list(L.ptr(sd), L.ptr(out), L.ptr(rd), len(T), ntiles, pitch, rows, C, Cp, dt, 0.5, None), "from_btc_list")
    torch.cuda.synchronize()
    _check_items(out.cpu(), want, [w.abs() for w in want], col_off, pitch, 1, "out", False, "wae_from_btc_list")
    # back through wae_to_btc_list: the item's rows hold 0.5 * src in the channels, zero in the pad channels; other rows untouched
    back = torch.full((rows, Cp), 7.0, dtype=tdt, device=DEV)
    L.check(lib.wae_to_btc_list(L.ptr(out), L.ptr(back), L.ptr(rd), len(T), ntiles, pitch, C, Cp, dt, None), "to_btc_list")
    torch.cuda.synchronize()
    back = back.cpu().float()
    own = RL.owned(row_off, T, rows)
    assert bool((back[~own] == 7.0).all())
    assert torch.equal(back[own][:, :C], src.float()[own][:, :C] * 0.5) and bool((back[own][:, C:] == 0).all())


def test_from_btc_list_skips_a_bad_record_and_refuses():
    L, lib = _lib()
    rng = np.random.RandomState(5100)
    C, Cp = 5, 8
    T, col_off, pitch, row_off, rows, src, recs, ntiles = _fb_setup(rng, C, Cp, torch.float32)
    bad = 2
    recs = recs.copy()
    recs[bad, 2] = rows - int(T[bad]) + 1                  # one row beyond the operand
    want = RL.from_btc_list(src, row_off, T, C, 2.0)
    out = torch.full((C, pitch), SENT, device=DEV)
    sd, rd = _dev(src), torch.from_numpy(recs).to(DEV)
    L.check(lib.wae_from_btc_list(L.ptr(sd), L.ptr(out), L.ptr(rd), len(T), ntiles, pitch, rows, C, Cp, 0, 2.0, None), "from_btc_list")
    torch.cuda.synchronize()
    _check_items(out.cpu(), want, [w.abs() for w in want], col_off, pitch, 1, "out", False, "wae_from_btc_list", skip=(bad,))
    out.fill_(SENT)
    for kw, msg in ((dict(Cp=4), "Cp 4"), (dict(dt=3), "dtype"), (dict(rows=0), "rows"), (dict(ntiles=0), "ntiles"), (dict(nsegs=0), "table")):
        a = dict(Cp=Cp, dt=0, rows=rows, ntiles=ntiles, nsegs=len(T))
        a.update(kw)
        rc = lib.wae_from_btc_list(L.ptr(sd), L.ptr(out), L.ptr(rd), a["nsegs"], a["ntiles"], pitch, a["rows"], C, a["Cp"], a["dt"], 1.0, None)
        assert rc != 0 and msg in lib.wae_last_error().decode(), (kw, lib.wae_last_error().decode())
        torch.cuda.synchronize()
        assert bool((out == SENT).all()), kw


def test_from_btc_list_rounding():
    """Gaussian rows in fp32 times a scale that is no power of two: one product per element, held to the same (n + 4) 2^-24 A"""
    L, lib = _lib()
    rng = np.random.RandomState(81)
    C, Cp = 70, 96
    T, col_off, pitch, row_off, rows, src, recs, ntiles = _fb_setup(rng, C, Cp, torch.float32)
    own = RL.owned(row_off, T, rows)
    src[own] = _gauss(rng, int(own.sum()), Cp)
    scale = 1.0 / 3.0
    want = RL.from_btc_list(src, row_off, T, C, float(np.float32(scale)))
    out = torch.full((C, pitch), SENT, device=DEV)
    sd, rd = _dev(src), torch.from_numpy(recs).to(DEV)
    L.check(lib.wae_from_btc_list(L.ptr(sd), L.ptr(out), L.ptr(rd), len(T), ntiles, pitch, rows, C, Cp, 0, scale, None), "from_btc_list")
    torch.cuda.synchronize()
    _check_items(out.cpu(), want, [w.abs() for w in want], col_off, pitch, 1, "out", True, "wae_from_btc_list")
