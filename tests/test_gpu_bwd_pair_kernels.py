"""The fused layer-boundary launches of the backward data path -- wae_glu_bwd_fused (csrc/glu_bwd.hip: glu_bwd_fused_kernel in fp32,
glu_bwd_pair_kernel in 16 bits) and wae_glu_bwd_fused_dc (the same 4-wave kernel with the conditioning gradient folded in, and
csrc/glu_bwd8.hip: glu_bwd_pair8_kernel) -- each launch called straight through the C ABI, without an engine, against the float64
restatement of tests/tm_ref.py (pair_ref).  The launches are data (tests/tm_cases.py); w_x (interleaved in 16 bits, tap by tap in fp32),
w_uo (accumulator-row order), w_us and w_c are packed there from DENSE matrices with packing.first_gemm_map / second_gemm_map.

EXACT cases, operands, guards and kinds are those of tests/test_gpu_tm_kernels.py: integers in [-3, 3], alpha in {1, 0.5, -2, 0.25},
z_prev = 0 (dz_prev = [du / 2 | 0]), dc_acc prefilled with integers; torch.equal on the float values, the message names the first wrong
(b, t, column).  Phase A's result is handed to the second contraction ROUNDED to the storage dtype (csrc/glu_bwd.hip keeps dx-hat "as
stored": acc_to_frags converts the scaled accumulators to 16-bit fragments; fp32 hands the fp32 value over) and the reference does the
same, so a "dense" bf16 case checks that rounding too; a "rep" case hands over values exact in 16 bits.  dz_l and dz_{l-1} are column
slices of ONE (B, T, dz_stride) buffer, as in the sweep: dz_l's columns, the foreign columns and the 1024.0 margin rows must keep their
values; g_out, dc_acc and dc_out (no stride in the ABI) lie between 1024 sentinel elements and start as NaN where they must be written.
With last = 1 dz_{l-1} must stay untouched; with dc_mode bit 1 the sum goes to dc_out and dc_acc must stay untouched, else the reverse.
ROUNDING cases, one per kernel path and dtype, in two kinds:
  "gauss"  Gaussian dz, dx_{l+1}-hat, w_x and w_c: dx_l-hat and dc to |got - ref64| <= 2 (n + 4) 2^-24 A + h(ref64); phase B takes the kernel's
           own stored dx_l-hat as the reference's operand (phase A's error is not counted twice), its weights are integers, z is Gaussian
           with entries at +-20: |got - e| <= h(e) + k 2^-23 |du| + 2 (n + 4) 2^-24 A_du  (du is a rounded fp32 sum here; the gate factors are
           at most 1);
  "gate"   integer GEMM operands throughout (dx_l-hat must be exact, du is exact), the same z: |got - e| <= h(e) + k 2^-23 |du|, and the
           largest (|got - e| - h(e)) / (2^-23 |du|) is printed (run with -s).  k = 4 x the largest value observed on an MI355X against
           the float64 reference: observed 0.528 (bf16: 0.31 pair4, 0.53 pair4-fold, 0.46 pair8), 0.8552 (fp16: 0.79 / 0.77 / 0.86), 1.405
           (fp32) = K_OBSERVED below, hence k = 2.11, 3.42, 5.62 = K_GATE.  Phase A's largest err / bound: 0.86 (bf16), 0.54 (fp16), nearly
           all of it the storage rounding h; 0.0018 (fp32).

Which case reaches which kernel path (tests/tm_cases.py: pair_path restates dispatch_gb, the *_supported functions and
wae_glu_bwd8_launch; tests/test_tm_ref_cpu.py asserts the coverage):

  path         kernel                                            cases
  fused-fp32   glu_bwd_fused_kernel<float, Rp / 32, Hp / 32>     PAIR_AXES["fused"] in fp32: (Rp, Hp) in {(256, 192), (256, 128), (128, 32), (128, 64),
                                                                 (128, 96), (128, 128)}, taps 2 / 3 / 4, T in {1 .. 257}, B in {1, 3}
  pair4        glu_bwd_pair_kernel<E, .., FOLD = false>          the same cases in bf16 / fp16: (256, 192), (256, 128), (128, 64), (128, 128)
  refused      WAE_EUNSUPPORTED before any launch                (128, 32) and (128, 96) in 16 bits
  pair4-fold   glu_bwd_pair_kernel<E, .., FOLD = true>           PAIR_AXES["dc"] with dc_mode bit 2 (T in {1 .. 257}), (128, 64), Sp = 128
  pair8        glu_bwd_pair8_kernel<E, 4 / 6, 4>                 PAIR_AXES["dc"]: Rp 256, Sp 256, Hp in {128, 192}, T in {1, 33, 255, 256, 257, 513},
                                                                 dc_mode 0 .. 3, last 0 / 1
  dilations 1, 2, 32, 33, 128, T + 5 on every path."""
import ctypes

import pytest
import torch

import tm_cases as C
import tm_device as D

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# phase B, "gate" cases: largest (|got - e| - h(e)) / (2^-23 |du|) observed per dtype, and the bound's k = 4 x that
K_OBSERVED = {"bf16": 0.528, "fp16": 0.8552, "fp32": 1.405}
K_GATE = {dt: 4.0 * v for dt, v in K_OBSERVED.items()}


class Launched:
    pass


def _launch(c, prob, dtype, streams=None, dilation=None):
    """upload, launch ONCE -> the return code and the device buffers"""
    L, lib = D.lib()
    td = C.TORCH_DT[dtype]
    B, T, z2 = c.B, c.T, 2 * c.Hp
    c0, c1, stride = C.dz_cols(c)
    r = Launched()
    host = prob.dzbuf.clone()
    host[:, :, c1:c1 + z2] = float("nan")       # dz_{l-1}: every element must be written (or, with last = 1, none)
    r.margin = (c.ktaps - 1) * c.dilation + 64
    r.dz_host = host.to(td)
    r.dz = D.Rows(host, dtype, r.margin)
    r.g_next, r.dskip, r.z_prev = D.Rows(prob.g_next, dtype, 64), D.Rows(prob.dskip, dtype, 64), D.Rows(prob.z_prev, dtype, 64)
    r.g_out = D.Flat(torch.full((B * T, c.Rp), float("nan")), td)
    st = streams or {k: v[0] for k, v in C.pair_streams(c, prob, dtype).items()}
    w = {k: D.upload(v, dtype) for k, v in st.items()}
    desc = L.GluBwdDesc(C.DT[dtype], B, T, c.Rp, c.Hp, c.Sp, c.ktaps, c.dilation if dilation is None else dilation, c.alpha)
    vp = ctypes.c_void_p
    args = [ctypes.byref(desc), vp(r.dz.at(c0)), stride, vp(r.g_next.at()), vp(r.g_out.ptr()), vp(r.dskip.at()), vp(r.z_prev.at()), vp(r.dz.at(c1)),
            L.ptr(w["w_x"]), L.ptr(w["w_uo"]), L.ptr(w["w_us"])]
    if c.dc:
        r.dc_acc = D.Flat(prob.dc_prev.reshape(B * T, 64), torch.float32)
        r.dc_out = D.Flat(torch.full((B * T, 64), float("nan")), td)
        r.rc = lib.wae_glu_bwd_fused_dc(*args, L.ptr(w["w_c"]), vp(r.dc_acc.ptr()), vp(r.dc_out.ptr()), c.dc_mode, c.last, None)
    else:
        r.rc = lib.wae_glu_bwd_fused(*args, None)
    torch.cuda.synchronize()
    return r


def _dz_prev(c, r, what):
    """the dz_{l-1} window (B * T, 2Hp) as fp32, after checking that the margins, dz_l and the foreign columns kept every bit"""
    _, c1, stride = C.dz_cols(c)
    z2 = 2 * c.Hp
    b = r.dz.buf.cpu()
    rows = c.B * c.T
    assert bool((b[:r.margin] == C.MARGIN).all()) and bool((b[r.margin + rows:] == C.MARGIN).all()), f"{what}: a margin row of the dz buffer was written"
    mid = b[r.margin:r.margin + rows]
    keep = torch.ones(stride, dtype=torch.bool)
    keep[c1:c1 + z2] = False
    assert torch.equal(D._bits(mid[:, keep].contiguous()), D._bits(r.dz_host.view(rows, stride)[:, keep].contiguous())), f"{what}: dz_l or a foreign column was written"
    return mid[:, c1:c1 + z2].float()


def _describe(c, dtype):
    return (f"{c.name} [{dtype}, {C.pair_path(c, dtype)}] Rp {c.Rp}, Hp {c.Hp}, Sp {c.Sp}, taps {c.ktaps}, dilation {c.dilation}, B {c.B}, T {c.T}, "
            f"alpha {c.alpha}, dc_mode {c.dc_mode}, last {c.last}")


def _flat2(x):
    return x.reshape(-1, x.shape[-1])


def _check_dc_exact(c, r, ref, dtype, what):
    if not c.dc:
        return None
    if ref.dc_to_out:
        assert r.dc_acc.untouched(), f"{what}: dc_acc was written although dc_mode bit 1 sends the sum to dc_out"
        return D.first_difference(r.dc_out.result(what), C.storage(_flat2(ref.dc.out), dtype), c.T, what + " dc_out")
    assert r.dc_out.untouched(), f"{what}: dc_out was written without dc_mode bit 1"
    return D.first_difference(r.dc_acc.result(what), _flat2(ref.dc.out).float(), c.T, what + " dc_acc")


def _run_exact(c, dtype, **kw):
    """-> the first difference (a message) or None"""
    L, _ = D.lib()
    prob = C.pair_problem(c, dtype)
    ref, what = prob.ref, _describe(c, dtype)
    r = _launch(c, prob, dtype, **kw)
    L.check(r.rc, c.name)
    msgs = [D.first_difference(r.g_out.result(what), C.storage(_flat2(ref.g_out.out), dtype), c.T, what + " g_out")]
    dzp = _dz_prev(c, r, what)
    if c.last:
        assert bool(torch.isnan(dzp).all()), f"{what}: dz_prev was written with last = 1"
    else:
        msgs.append(D.first_difference(dzp, C.storage(_flat2(ref.dz_prev.out), dtype), c.T, what + " dz_prev"))
    msgs.append(_check_dc_exact(c, r, ref, dtype, what))
    msgs = [m for m in msgs if m]
    return "; ".join(msgs) if msgs else None


_CASES = [(c, dt) for c in C.pair_cases() for dt in C.pair_dtypes(c)]


@pytest.mark.parametrize("c,dtype", _CASES, ids=[f"{c.name}-{dt}" for c, dt in _CASES])
def test_pair_exact(c, dtype):
    _, lib = D.lib()
    path = C.pair_path(c, dtype)
    sup = lib.wae_glu_bwd_fused_supported(c.Rp, c.Hp) if dtype == "fp32" else lib.wae_glu_bwd_fused_supported16(c.Rp, c.Hp)
    assert bool(sup) == (path != "refused"), (c.name, dtype, sup)
    if path == "refused":           # WAE_EUNSUPPORTED (-2) before any launch: no output changes a bit
        prob = C.pair_problem(c, dtype)
        r = _launch(c, prob, dtype)
        assert r.rc == -2, (c.name, r.rc)
        assert r.g_out.untouched() and bool(torch.isnan(_dz_prev(c, r, c.name)).all()), c.name
        return
    msg = _run_exact(c, dtype)
    assert msg is None, msg


def _beyond(err, bound, c, what, got, e):
    bad = (~(err <= bound)).nonzero()       # (an element never written is NaN: beyond every bound)
    if len(bad):
        r, col = bad[0].tolist()
        raise AssertionError(f"{what}: {len(bad)} elements beyond the bound, first at (b {r // c.T}, t {r % c.T}, column {col}): got {float(got[r, col])}, "
                             f"want {float(e[r, col])}, bound {float(bound[r, col])}")


_ROUNDING = [(c, dt) for c in C.pair_rounding_cases() for dt in C.pair_dtypes(c)]


@pytest.mark.parametrize("c,dtype", _ROUNDING, ids=[f"{c.name}-{dt}" for c, dt in _ROUNDING])
def test_rounding_bound(c, dtype):
    """the bounds of the module docstring, per element"""
    L, _ = D.lib()
    prob = C.pair_problem(c, dtype)
    what = _describe(c, dtype)
    r = _launch(c, prob, dtype)
    L.check(r.rc, c.name)
    g = r.g_out.result(what)
    ref = C.pair_reference(c, prob, dtype, handed=g.double().view(c.B, c.T, c.Rp))      # phase B from the kernel's own stored dx-hat
    ea = _flat2(ref.g_out.out)
    if c.kind == "gate":
        msg = D.first_difference(g, C.storage(ea, dtype), c.T, what + " g_out (integer operands: exact)")
        assert msg is None, msg
    else:
        bound = 2.0 * (ref.g_out.n + 4.0) * U * _flat2(ref.g_out.A) + C.half_ulp(ea, dtype)
        err = (g.double() - ea).abs()
        print(f"{C.pair_path(c, dtype)} {dtype} phase A: largest err / (2 (n + 4) 2^-24 A + h) = {float((err / bound).max()):.4g}")
        _beyond(err, bound, c, what + " g_out", g, ea)
    if c.dc:
        ed = _flat2(ref.dc.out)
        to16 = ref.dc_to_out
        gd = (r.dc_out if to16 else r.dc_acc).result(what).double()
        bound = 2.0 * (ref.dc.n + 4.0) * U * _flat2(ref.dc.A) + (C.half_ulp(ed, dtype) if to16 else 0.0)
        _beyond((gd - ed).abs(), bound, c, what + " dc", gd, ed)
    eb = _flat2(ref.dz_prev.out)
    gb = _dz_prev(c, r, what).double()
    du = _flat2(ref.dz_prev.acc).abs()
    du = torch.cat([du, du], dim=1)
    h, unit = C.half_ulp(eb, dtype), 2.0 ** -23 * du
    err = (gb - eb).abs()
    bound = h + K_GATE[dtype] * unit
    if c.kind == "gate":
        live = du > 0
        worst = float(((err - h)[live] / unit[live]).max())
        print(f"{C.pair_path(c, dtype)} {dtype} phase B: largest (|got - e| - h(e)) / (2^-23 |du|) = {worst:.4g}")
    else:
        bound = bound + 2.0 * (ref.dz_prev.n + 4.0) * U * _flat2(ref.dz_prev.A)
    _beyond(err, bound, c, what + " dz_prev", gb, eb)
