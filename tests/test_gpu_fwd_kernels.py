"""The forward launches of the decoder -- wae_glu_layer_fwd / _drop / _list (csrc/glu_fwd.hip, glu_fwd_static.hip, glu_fwd_list.hip),
wae_head_fwd / wae_head_fwd_from_h0 (csrc/head_fwd.hip) and wae_first_conv_fwd (csrc/misc.hip) -- each called straight through the
C ABI, without an engine, ONCE, against the float64 restatements of tests/fwd_ref.py.  The launches are data (tests/fwd_cases.py); the
packed weight streams are gathered there from DENSE matrices through the product's own maps (packing.glu_w1_map, glu_w2_map,
glu_bias2_map, head_w_map, head_bias_map, first_conv_maps), so kernel and packing map are tested together against dense arithmetic.

EXACT comparisons are torch.equal on the float values -- no tolerance -- and a failure names the first wrong (b, t, column):
  layer "sat"    z_save, u_out and x_out.  x, x_conv, c and the a-half of zb are 64 {-1, 0, 1}, W1 / Wc rows hold at most 8 nonzeros of
                 +-1 / +-2, the b-half of zb is 64 * 18: every z is 64 n, exact in 16 bits, z_b >= 128, and the gate is exactly -1, 0 or
                 +1 (16 bits: exp2(-0) = 1 gives 1 - ea = 0; a >= 64 underflows ea and eg to 0; a <= -64 is clamped at -15, where
                 -ea rcp(ea) is -1 to within an fp32 ulp, which is -1 after the conversion; fp32: tanhf / expf saturate).  W_out is
                 dense from [-3, 3], so y + x is an exact integer and x_out = storage(fp32(y + x) * fp32(sqrt(.5))): one fp32 product.
  layer "dense"  z_save: operands and weights from [-3, 3] everywhere, the sums are integers below 2^22, one rounding to storage.
  head           h0_save = storage(relu(scale s)), h1_save = storage(relu(b1 + W1 h0)) and the fp32 logits, with u / h0 integers in
                 [-3, 3], scale a power of two and both hand-overs restated; "ce" cases (one class >= 128 above all others in every
                 column, b3's pad entries at +4096): __expf of every other term is 0, s = 1, __logf(1) = 0, so lse = max and
                 nll = max - logits[target[t + 1]] exactly, 0 at t = T - 1.
  first conv     integer table, bias and samples; ids -1 and O clamped, WAE_ERR_CLASS_ID OR-ed into a word preset to WAE_ERR_TARGET_ID.
OPERANDS: x_in, x_conv, c_up, u and h0 lie in larger allocations whose margin rows hold 1024.0; B >= 2 in most cases, so the rows
before t = 0 of a clip are another clip's; pad columns of x_conv, c_up, u and h0 hold nonzero values that only a zero of the packed
stream keeps out.  OUTPUTS: u_out is a column window of a wider prefilled array; every output starts as NaN between sentinel guards:
every element must be written, guards and foreign columns must keep their values, pad columns come back as zeros, rows no list
record owns -- those of a malformed record (T = 0), which is skipped whole -- stay NaN in u_out and x_out, and with WAE_GLU_NO_OUT
x_out keeps every bit.
ROUNDING bounds, against float64 and never against another kernel; U = 2^-24, h = half a unit in the last place of the storage type:
  z       |got - z64| <= 2 (n + 4) U A + h                     (the bound tests/test_gpu_tn_kernels.py derives; "dense" / "gate": exact)
  u       |got - gate64(z64)| <= h + k 2^-23 + (z's sum bound in the a-half + in the b-half: the gate's slope is at most 1)
  x_out   (u's bound carried through |W_out| + 2 (H + 6) U A_y) sqrt(.5) + h
  lse     |got - lse64| <= k_ce 2^-23 (1 + |lse64|) + the logits' sum bound;  nll: the same + the picked logit's bound + U |nll64| (the
          subtraction's own rounding), exactly 0 at t = T - 1.
  They hold u and x_out of the "dense" layer cases, the "gauss" cases (one per kernel path and dtype: Gaussian operands and weights
  rounded to storage, z about N(0, 1.5) with a few channels at +-20) and lse / nll of every head case that is not "ce".  A "gauss" head
  takes its float64 h1 from the kernel's own stored h0, its logits from the stored h1 and once more its lse / nll from the stored fp32
  logits, so that an earlier GEMM's error is not counted twice and no sum bound hides k_ce.  Under the z term of a "gauss" layer case
  (about 1e4 units of 2^-23) the gate's own error cannot be seen, so k is measured on the "gate" cases, one per path and dtype: x, c
  from [-3, 3] / 8, sparse W1, zb Gaussian in multiples of 2^-12 -- the same spread of z, but exact in fp32 in any order (z_save is
  compared bit for bit), so u's whole error is the gate's.
  k = 4 x the largest (|got - e| - h) / 2^-23 observed on an MI355X (printed; run with -s), and at least 0.5: the fp32 result's own
  rounding in front of the storage rounding (2^-24).  Observed on an MI355X (gfx950; profiles/fwd_kernels.txt has the run):
    gate   fp32 1.054 (fp32-4x32; 0.93 list, 0.89 on the "dense" cases: libm tanhf / expf); bf16 0.0 and fp16 -0.001 on every path: the
           exp2 / rcp gate's error never reached past h, the upper bound of the storage half unit -- hence k = 4.22 (fp32), 0.5 (16 bits)
    k_ce   0.747 (bf16), 0.770 (fp16), 0.708 (fp32) on Gaussian logits of spread 3, 0.487 on the exact logits of the "rep" / "dense"
           cases (any dtype) -- hence k_ce = 2.99, 3.08, 2.83
  Largest err / bound elsewhere: z of the "gauss" cases 0.92 (bf16), 0.68 (fp16) -- nearly all of it h -- and 0.013 (fp32); x_out 0.50 /
  0.43 / 0.030 ("dense"), 0.34 / 0.095 / 0.0002 ("gauss"); head h0 0.92 / 0.64 / 0.007, h1 0.97 / 0.81 / 0.011, logits 0.004 / 0.005 / 0.012.
  The saturation steps of the "sat" kind held on hardware in every dtype (fp32's tanhf(-64) is -1), so nothing was moved to a bound.

Which case reaches which kernel (tests/fwd_cases.py: fwd_path / head_path restate the dispatch; tests/test_fwd_ref_cpu.py asserts that
every path is reached at every T of its tile set, with and without the z save, in every dtype it exists in):
  static/256x192, /256x128, /512x256   glu_fwd_static(_z)_kernel: 16 bits, ktaps 3, Ccp 64, no shape flag; full T and dilation sweeps at B = 3
  generic-8x32 / -4x64 / -4x32         glu_fwd_kernel, 16 bits: default / WAE_GLU_CG2 / WAE_GLU_WAVES4 (where two workgroups fit a CU)
  fp32-4x32                            glu_fwd_kernel, fp32 (libm tanhf / expf)
  list-8x32, list-fp32-4x32            glu_fwd_kernel<LIST>: tables of 3 and 4 items, zb rows permuted, a malformed record skipped whole
  refused                              Hp / 32 = 5, Rp = 64, WAE_GLU_SAVE_Z without z_save or on the list form: return codes only
  head4, from_h0-4, from_h0-8          head_fwd_kernel: 4 waves x 128 columns; FROM_H0 fp32; FROM_H0 16 bits on 8 waves x 256 columns"""
import ctypes

import pytest
import torch

import fwd_cases as C
import fwd_ref as R
import tm_device as D

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# the gate: largest (|got - gate64(z64)| - h) / 2^-23 observed per dtype on an MI355X ("gate" cases), and the bound's k = 4 x that, at
# least 0.5 (the fp32 result's own rounding in front of the storage rounding)
K_OBSERVED = {"bf16": 0.0, "fp16": -0.001023, "fp32": 1.054}
K_GATE = {dt: max(4.0 * v, 0.5) for dt, v in K_OBSERVED.items()}
# lse / nll: largest (|got - ref64| - the other terms) / (2^-23 (1 + |lse64|)) observed per dtype, and k_ce = 4 x that
KCE_OBSERVED = {"bf16": 0.7471, "fp16": 0.7704, "fp32": 0.7076}
K_CE = {dt: 4.0 * v for dt, v in KCE_OBSERVED.items()}
U_COL = 8               # u_out: the layer's Hp columns from element 8 of a wider array
NAN = float("nan")


def _vp(x):
    return None if x is None else ctypes.c_void_p(x)


# ======================================================================================================================= layer
class LayerRun:
    """the buffers of one layer launch; run() launches ONCE"""

    def __init__(self, c, prob, dtype, streams=None, with_z=None):
        self.c, self.dtype = c, dtype
        td = C.TORCH_DT[dtype]
        self.rows = rows = prob.owned.numel()
        self.x_in = D.Rows(prob.x_in, dtype, 64)
        self.x_conv = D.Rows(prob.x_conv, dtype, 64) if c.entry == "drop" else None
        self.c_up = D.Rows(prob.c_up, dtype, 64) if c.Ccp else None
        w, bias = streams if streams is not None else C.layer_streams(c, prob, dtype)
        self.w, self.bias = D.upload(w, dtype), bias.float().to(D.DEV).contiguous()
        self.zb = prob.zb.float().to(D.DEV).contiguous()
        self.u = D.Window(rows, U_COL, c.Hp, td)
        self.x_out = D.Flat(torch.full((rows, c.Rp), NAN), td)
        want_z = bool(c.flags & C.SAVE_Z) if with_z is None else with_z
        self.z = D.Flat(torch.full((rows, 2 * c.Hp), NAN), td) if want_z else None
        self.table = torch.from_numpy(prob.table).to(D.DEV).contiguous() if prob.table is not None else None
        self.ntiles = prob.ntiles

    def run(self, **over):
        """-> rc; over: descriptor fields to override (the refusals)"""
        L, lib = D.lib()
        c = self.c
        f = dict(dtype=C.DT[self.dtype], B=c.B, T=c.T, Rp=c.Rp, Ccp=c.Ccp, Hp=c.Hp, ktaps=c.k, dilation=c.d, flags=c.flags)
        f.update(over)
        desc = L.GluDesc(*[f[n] for n in ("dtype", "B", "T", "Rp", "Ccp", "Hp", "ktaps", "dilation", "flags")])
        x_in, x_out, c_up = _vp(self.x_in.at()), _vp(self.x_out.ptr()), _vp(self.c_up.at() if self.c_up else None)
        u, z = _vp(self.u.ptr()), _vp(self.z.ptr() if self.z else None)
        common = (u, self.u.stride, L.ptr(self.zb), self.zb.shape[1])
        if c.entry == "list":
            rc = lib.wae_glu_layer_fwd_list(ctypes.byref(desc), L.ptr(self.table), len(c.items), self.ntiles, self.rows, x_in, x_out, c_up,
                                            *common, L.ptr(self.w), L.ptr(self.bias), None)
        elif c.entry == "drop":
            rc = lib.wae_glu_layer_fwd_drop(ctypes.byref(desc), x_in, _vp(self.x_conv.at()), x_out, c_up, *common, z, L.ptr(self.w),
                                            L.ptr(self.bias), None)
        else:
            rc = lib.wae_glu_layer_fwd(ctypes.byref(desc), x_in, x_out, c_up, *common, z, L.ptr(self.w), L.ptr(self.bias), None)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return self.u.untouched() and self.x_out.untouched() and (self.z is None or self.z.untouched())


def _describe(c, dtype):
    return (f"{c.name} [{dtype}, {C.fwd_path(c, dtype)}] {c.entry}, Rp {c.Rp} (R {c.R}), Hp {c.Hp} (H {c.H}), Ccp {c.Ccp}, ktaps {c.k}, dilation {c.d}, "
            f"B {c.B}, T {c.T or C.list_items(c, dtype)}, flags {c.flags}")


def _row_T(c, rows):
    return c.T if c.entry != "list" else rows       # (a list's rows are named as t of one clip: the packed row)


def _beyond(err, bound, got, want, T, what):
    bad = (~(err <= bound)).nonzero()          # (an element never written is NaN: beyond every bound)
    if len(bad):
        r, col = bad[0].tolist()
        return (f"{what}: {len(bad)} elements beyond the bound, first at (b {r // T}, t {r % T}, column {col}): got {float(got[r, col])}, "
                f"want {float(want[r, col])}, bound {float(bound[r, col])}")
    return None


def _unowned(got, owned, what):
    """the rows no record of a list owns (a malformed record's among them) must still hold the NaN they started with"""
    if bool(owned.all()) or bool(torch.isnan(got[~owned]).all()):
        return None
    r, col = (~torch.isnan(got) & ~owned.unsqueeze(1)).nonzero()[0].tolist()
    return f"{what}: row {r}, which no record owns, was written (column {col}: {float(got[r, col])})"


def _same(got, want, owned, T, what):
    """exact comparison over the owned rows, NaN kept in all others (tm_device.first_difference wants arrays without NaN on both sides)"""
    msg = _unowned(got, owned, what)
    if msg:
        return msg
    got, want = got.clone(), want.clone()
    got[~owned] = 0.0
    want[~owned] = 0.0
    return D.first_difference(got, want, T, what)


def _gate_bounds(c, prob, dtype, got_u, got_x, what, z_exact):
    """the bounds of the module docstring on u and x_out over the rows the launch owns -> (message or None, observed k of the gate,
    largest x_out err / bound)"""
    ref, own, H = prob.ref, prob.owned, c.H
    T = _row_T(c, own.numel())
    zt = torch.zeros_like(ref.u) if z_exact else 2.0 * (ref.n1 + 4.0) * U * (ref.zA[:, :c.Hp] + ref.zA[:, c.Hp:])
    hu = C.half_ulp(ref.u, dtype)
    unit = 2.0 ** -23
    err_u = (got_u.double() - ref.u).abs()
    k_seen = float(((err_u - hu - zt)[own] / unit).max())
    ub = hu + K_GATE[dtype] * unit + zt
    msg = _beyond(err_u[own], ub[own], got_u[own], ref.u[own], T, what + " u_out")
    x_seen = 0.0
    if got_x is not None and msg is None:
        carried = ub[:, :H] @ prob.W_out.double().abs().t()
        xb = torch.full_like(ref.x_out, NAN)
        xb[:, :c.R] = (carried + 2.0 * (ref.n2 + 4.0) * U * ref.yA[:, :c.R]) * R.SQRT_HALF
        xb[:, c.R:] = 0.0
        xb = xb + C.half_ulp(ref.x_out, dtype)
        err_x = (got_x.double() - ref.x_out).abs()
        live = own.unsqueeze(1) & (xb > 0)
        x_seen = float((err_x[live] / xb[live]).max())
        msg = _beyond(err_x[own], xb[own], got_x[own], ref.x_out[own], T, what + " x_out")
    return msg, k_seen, x_seen


def run_layer_case(c, dtype, streams=None):
    """-> None or what is wrong with the launch's outputs"""
    L, _ = D.lib()
    prob = C.layer_problem(c, dtype)
    run = LayerRun(c, prob, dtype, streams=streams)
    L.check(run.run(), c.name)
    what = _describe(c, dtype)
    ref, T = prob.ref, _row_T(c, prob.owned.numel())
    got_u = run.u.result(what + " u_out")
    if c.flags & C.NO_OUT:
        assert run.x_out.untouched(), f"{what}: WAE_GLU_NO_OUT, but x_out was written"
        got_x = None
    else:
        got_x = run.x_out.result(what + " x_out")
    own = prob.owned
    msg = _unowned(got_u, own, what + " u_out") or (_unowned(got_x, own, what + " x_out") if got_x is not None else None)
    if msg:
        return msg
    if run.z is not None and c.kind != "gauss":
        msg = _same(run.z.result(what + " z_save"), C.storage(ref.z, dtype), own, T, what + " z_save")
        if msg:
            return msg
    if c.kind == "sat":
        msg = _same(got_u, C.storage(ref.u, dtype), own, T, what + " u_out")
        if msg is None and got_x is not None:
            msg = _same(got_x, C.sat_x_out(ref.yx, dtype), own, T, what + " x_out")
        return msg
    if c.kind == "gauss" and run.z is not None:
        got_z = run.z.result(what + " z_save").double()
        zb = 2.0 * (ref.n1 + 4.0) * U * ref.zA + C.half_ulp(ref.z, dtype)
        own = prob.owned
        live = own.unsqueeze(1) & (zb > 0)
        print(f"{C.fwd_path(c, dtype)} {dtype}: largest z err / (2 (n + 4) 2^-24 A + h) = {float(((got_z - ref.z).abs()[live] / zb[live]).max()):.4g}")
        msg = _beyond((got_z - ref.z).abs()[own], zb[own], got_z[own], ref.z[own], T, what + " z_save")
        if msg:
            return msg
    # the pad columns are exact whatever the kind: zeros
    if bool(got_u[prob.owned][:, c.H:].any()) or (got_x is not None and bool(got_x[prob.owned][:, c.R:].any())):
        return f"{what}: a pad column of u_out or x_out is not zero"
    msg, k_seen, x_seen = _gate_bounds(c, prob, dtype, got_u, got_x, what, z_exact=c.kind in ("dense", "gate"))
    print(f"{C.fwd_path(c, dtype)} {dtype} {c.kind}: gate k observed {k_seen:.4g} (bound k {K_GATE[dtype]:.4g}); x_out err / bound {x_seen:.4g}")
    return msg


_LAYER = [(c, dt) for c in C.layer_cases() for dt in c.dts]


@pytest.mark.parametrize("c,dtype", _LAYER, ids=[f"{c.name[4:]}-{dt}" for c, dt in _LAYER])
def test_layer_exact(c, dtype):
    msg = run_layer_case(c, dtype)
    assert msg is None, msg


_LAYER_R = [(c, dt) for c in C.layer_rounding_cases() for dt in c.dts]


@pytest.mark.parametrize("c,dtype", _LAYER_R, ids=[f"{c.name[4:]}-{dt}" for c, dt in _LAYER_R])
def test_layer_rounding_bound(c, dtype):
    """Gaussian operands at the path's largest small shape: the bounds of the module docstring, per element"""
    msg = run_layer_case(c, dtype)
    assert msg is None, msg


_SAVE_Z_TWINS = [(C.layer_case(p, "dense", ()), dt) for p, dt in (
    (dict(T=257, B=3), "bf16"), (dict(T=129, B=3), "fp32"), (dict(T=257, flags=C.CG2), "fp16"), (dict(T=129, flags=C.WAVES4), "bf16"),
    (dict(**{**C.STATIC_BASE[(256, 192)], "T": 257}), "bf16"), (dict(**{**C.STATIC_BASE[(256, 128)], "T": 257}), "fp16"),
    (dict(**{**C.STATIC_BASE[(512, 256)], "T": 257}), "bf16"))]


@pytest.mark.parametrize("c,dtype", _SAVE_Z_TWINS, ids=[f"{C.fwd_path(c, dt)}-{dt}" for c, dt in _SAVE_Z_TWINS])
def test_z_save_changes_no_bit_of_u_and_x_out(c, dtype):
    """the same dense launch with and without WAE_GLU_SAVE_Z (on the static path: another kernel)"""
    L, _ = D.lib()
    prob = C.layer_problem(c, dtype)
    outs = []
    for flags in (c.flags | C.SAVE_Z, c.flags & ~C.SAVE_Z):
        run = LayerRun(c._replace(flags=flags), prob, dtype)
        L.check(run.run(), c.name)
        outs.append((run.u.result(c.name), run.x_out.result(c.name)))
    msg = D.first_difference(outs[1][0], outs[0][0], c.T, c.name + " u_out") or D.first_difference(outs[1][1], outs[0][1], c.T, c.name + " x_out")
    assert msg is None, msg


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("i", range(len(C.LAYER_REFUSED)), ids=("Hp160", "Rp64", "save_z-without-z_save", "save_z-on-the-list"))
def test_layer_refusals_leave_the_outputs_untouched(i, dtype):
    """return codes only: refused before any launch, every output keeps every bit"""
    p, over, want = C.LAYER_REFUSED[i]
    over = dict(over)
    c = C.layer_case(p, "sat", C.DTYPES)
    prob = C.layer_problem(c, dtype)
    # (no map packs Hp / 32 = 5: that launch gets a stream of zeros, which nothing reads)
    streams = (torch.zeros(4096), torch.zeros(c.Rp)) if C.fwd_path(c, dtype) == "refused" else None
    run = LayerRun(c, prob, dtype, streams=streams, with_z=not over.pop("no_z", False) and c.entry != "list")
    if "flags" in over:
        over["flags"] |= c.flags
    elif c.entry != "list":
        over["flags"] = c.flags | C.SAVE_Z
    rc = run.run(**over)
    assert rc == want, (c.name, over, rc)
    assert run.untouched(), c.name


# ======================================================================================================================== head
class HeadRun:
    def __init__(self, c, prob, dtype, streams=None):
        self.c, self.dtype = c, dtype
        td = C.TORCH_DT[dtype]
        self.es = 4 if dtype == "fp32" else 2
        self.x = D.Rows(prob.x, dtype, 64)
        w, self.tail, bias = streams if streams is not None else C.head_streams(c, prob, dtype)
        self.w, self.bias = D.upload(w, dtype), bias.float().to(D.DEV).contiguous()
        self.target = prob.target.to(torch.int32).to(D.DEV).contiguous()
        B, T = c.B, c.T
        mk = lambda name, shape, t: None if name in c.nulls else D.Flat(torch.full(shape, NAN), t)       # noqa: E731
        self.logits, self.nll, self.lse = mk("logits", (B, c.O, T), torch.float32), mk("nll", (B, T), torch.float32), mk("lse", (B, T), torch.float32)
        self.h0 = mk("h0", (B * T, c.Sp), td) if c.entry == "head" else None
        self.h1 = mk("h1", (B * T, c.Sp), td)

    def run(self, nothing=False, **over):
        L, lib = D.lib()
        c = self.c
        f = dict(dtype=C.DT[self.dtype], B=c.B, T=c.T, Ku=c.Ku, Sp=c.Sp, Op=c.Op, O=c.O, scale=c.scale)
        f.update(over)
        desc = L.HeadDesc(*[f[n] for n in ("dtype", "B", "T", "Ku", "Sp", "Op", "O", "scale")])
        p = lambda b: _vp(b.ptr() if b is not None else None)      # noqa: E731
        logits = None if nothing else p(self.logits)
        tgt, nll = (None, None) if (self.nll is None or nothing) else (L.ptr(self.target), p(self.nll))
        if c.entry == "head":
            rc = lib.wae_head_fwd(ctypes.byref(desc), _vp(self.x.at()), L.ptr(self.w), L.ptr(self.bias), logits, tgt, nll, p(self.lse), p(self.h0),
                                  p(self.h1), None)
        else:
            rc = lib.wae_head_fwd_from_h0(ctypes.byref(desc), _vp(self.x.at()), _vp(self.w.data_ptr() + self.tail * self.es), L.ptr(self.bias), logits,
                                          tgt, nll, p(self.lse), p(self.h1), None)
        torch.cuda.synchronize()
        return rc

    def outputs(self):
        return [b for b in (self.logits, self.nll, self.lse, self.h0, self.h1) if b is not None]


def _head_describe(c, dtype):
    return (f"{c.name} [{dtype}, {C.head_path(c, dtype)}] Sp {c.Sp} (S {c.S}), Op {c.Op} (O {c.O}), Ku {c.Ku}, B {c.B}, T {c.T}, scale {c.scale}, "
            f"null: {c.nulls}")


def _ce_bounds(c, dtype, run, ref, logit_bound, what):
    """lse / nll under the bound of the module docstring -> (message or None, the observed k_ce)"""
    unit = 2.0 ** -23 * (1.0 + ref.lse.abs())
    msg, seen = None, 0.0
    if run.lse is not None and run.nll is not None:
        got = run.lse.result(what + " lse").double()
        err = (got - ref.lse).abs()
        seen = max(seen, float(((err - logit_bound) / unit).max()))
        msg = _beyond(err, K_CE[dtype] * unit + logit_bound, got, ref.lse, c.T, what + " lse (named as (b = 0, t = clip, column = t))")
    if run.nll is not None and msg is None:
        got = run.nll.result(what + " nll").double()
        other = 2.0 * logit_bound + U * ref.nll.abs()
        other[:, -1] = 0.0
        err = (got - ref.nll).abs()
        seen = max(seen, float(((err - other) / unit)[:, :-1].max()) if c.T > 1 else 0.0)
        bound = K_CE[dtype] * unit + other
        bound[:, -1] = 0.0              # t = T - 1: exactly 0
        msg = _beyond(err, bound, got, ref.nll, c.T, what + " nll (named as (b = 0, t = clip, column = t))")
    return msg, seen


def _pad(a, width):
    return C._pad_cols(a, width)


def run_head_case(c, dtype, streams=None):
    L, _ = D.lib()
    prob = C.head_problem(c, dtype)
    run = HeadRun(c, prob, dtype, streams=streams)
    L.check(run.run(), c.name)
    what = _head_describe(c, dtype)
    B, T, S, Sp = c.B, c.T, c.S, c.Sp
    rows = lambda a: _pad(a.reshape(B * T, S), Sp)      # noqa: E731
    if c.kind == "gauss":
        return _head_rounding(c, dtype, prob, run, what)
    ref = prob.ref
    if run.h0 is not None:
        msg = D.first_difference(run.h0.result(what + " h0_save"), C.storage(rows(ref.h0), dtype), T, what + " h0_save")
        if msg:
            return msg
    if run.h1 is not None:
        msg = D.first_difference(run.h1.result(what + " h1_save"), C.storage(rows(ref.h1), dtype), T, what + " h1_save")
        if msg:
            return msg
    if run.logits is not None:
        got = run.logits.result(what + " logits")
        msg = D.first_difference(got.transpose(1, 2).reshape(B * T, c.O), ref.logits.float().transpose(1, 2).reshape(B * T, c.O), T, what + " logits")
        if msg:
            return msg
    if c.kind == "ce":
        for name, buf, want in (("lse", run.lse, ref.lse), ("nll", run.nll, ref.nll)):
            if buf is not None:
                msg = D.first_difference(buf.result(what + " " + name).reshape(B * T, 1), want.float().reshape(B * T, 1), T, what + " " + name)
                if msg:
                    return msg
        return None
    if run.nll is None:
        assert run.lse is None or bool(torch.isnan(run.lse.result(what)).all()), f"{what}: lse written without a target"
        return None
    msg, seen = _ce_bounds(c, dtype, run, ref, torch.zeros_like(ref.lse), what)
    print(f"{C.head_path(c, dtype)} {dtype} {c.kind}: k_ce observed {seen:.4g} (bound k {K_CE[dtype]:.4g})")
    return msg


def _head_rounding(c, dtype, prob, run, what):
    B, T, S, Sp = c.B, c.T, c.S, c.Sp
    def cut(buf, name):
        full = buf.result(what + " " + name).reshape(B, T, Sp)
        assert not bool(full[:, :, S:].any()) and not bool(torch.isnan(full[:, :, S:]).any()), f"{what}: a pad column of {name} is not zero"
        return full[:, :, :S].double()
    got_h1 = cut(run.h1, "h1_save")
    got_h0 = cut(run.h0, "h0_save") if c.entry == "head" else None
    ref = C.head_reference(c, prob, dtype, h0=got_h0, h1=got_h1)
    worst = {}
    if got_h0 is not None:
        plain = C.head_reference(c, prob, "fp32")         # (no rounding of the hand-overs: h0 is the plain float64 value)
        b = 2.0 * (plain.n[0] + 4.0) * U * plain.A[0] + C.half_ulp(plain.h0, dtype)
        err = (got_h0 - plain.h0).abs()
        worst["h0"] = float((err / b).max())
        msg = _beyond(err.reshape(B * T, S), b.reshape(B * T, S), got_h0.reshape(B * T, S), plain.h0.reshape(B * T, S), T, what + " h0_save")
        if msg:
            return msg
    one = C.head_reference(c, prob, "fp32", h0=got_h0 if got_h0 is not None else None)         # h1 from the h0 the kernel handed over
    b = 2.0 * (one.n[1] + 4.0) * U * one.A[1] + C.half_ulp(one.h1, dtype)
    err = (got_h1 - one.h1).abs()
    worst["h1"] = float((err / b).max())
    msg = _beyond(err.reshape(B * T, S), b.reshape(B * T, S), got_h1.reshape(B * T, S), one.h1.reshape(B * T, S), T, what + " h1_save")
    if msg:
        return msg
    lb = 2.0 * (ref.n[2] + 4.0) * U * ref.A[2]             # (B, T, O)
    got = run.logits.result(what + " logits").double().transpose(1, 2)
    want = ref.logits.transpose(1, 2)
    worst["logits"] = float(((got - want).abs() / lb).max())
    msg = _beyond((got - want).abs().reshape(B * T, c.O), lb.reshape(B * T, c.O), got.reshape(B * T, c.O), want.reshape(B * T, c.O), T, what + " logits")
    if msg:
        return msg
    msg, seen = _ce_bounds(c, dtype, run, ref, lb.max(dim=2).values, what)
    if msg is None:
        # the softmax alone: float64 lse / nll of the fp32 logits the kernel itself stored -- no sum bound hides k_ce here
        lse_own, nll_own = R.ce_ref(got.transpose(1, 2), prob.target)
        msg, seen = _ce_bounds(c, dtype, run, R.HeadOut(None, None, None, lse_own, nll_own, None, None), torch.zeros_like(lse_own),
                               what + " (against the float64 softmax of the stored logits)")
    print(f"{C.head_path(c, dtype)} {dtype} gauss: err / bound " + ", ".join(f"{k} {v:.4g}" for k, v in worst.items())
          + f"; k_ce observed {seen:.4g} (bound k {K_CE[dtype]:.4g})")
    return msg


_HEAD = [(c, dt) for c in C.head_cases() for dt in c.dts]


@pytest.mark.parametrize("c,dtype", _HEAD, ids=[f"{c.name[5:]}-{dt}" for c, dt in _HEAD])
def test_head_exact(c, dtype):
    msg = run_head_case(c, dtype)
    assert msg is None, msg


_HEAD_R = [(c, dt) for c in C.head_rounding_cases() for dt in c.dts]


@pytest.mark.parametrize("c,dtype", _HEAD_R, ids=[f"{c.name[5:]}-{dt}" for c, dt in _HEAD_R])
def test_head_rounding_bound(c, dtype):
    msg = run_head_case(c, dtype)
    assert msg is None, msg


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("entry", ("head", "from_h0"))
@pytest.mark.parametrize("over", C.HEAD_REFUSED, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_head_refusals_leave_the_outputs_untouched(over, entry, dtype):
    """WAE_EINVAL (-1) before any launch: Sp = 192, Op = 64, Ku = 96, and nothing to produce"""
    c = C.head_case(dict(entry=entry), "rep")
    run = HeadRun(c, C.head_problem(c, dtype), dtype)
    rc = run.run(**over)
    assert rc == -1, (c.name, over, rc)
    assert all(b.untouched() for b in run.outputs()), c.name


# ================================================================================================================== first conv
@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("c", C.fc_cases(), ids=lambda c: c.name[3:])
def test_first_conv_exact(c, dtype):
    L, lib = D.lib()
    prob = C.fc_problem(c)
    tab, bias = C.fc_streams(c, prob)
    Rp = tab.shape[1]
    tab_d, bias_d = tab.float().to(D.DEV).contiguous(), bias.float().to(D.DEV).contiguous()
    ids = prob.ids.to(D.DEV) if prob.ids is not None else None
    xs = prob.xs.float().to(D.DEV) if prob.xs is not None else None
    out = D.Flat(torch.full((c.BT, Rp), NAN), C.TORCH_DT[dtype])
    err = torch.full((1,), C.ERR_TARGET_ID, dtype=torch.int32, device=D.DEV)
    L.check(lib.wae_first_conv_fwd(L.ptr(ids), L.ptr(xs), L.ptr(tab_d), L.ptr(bias_d), _vp(out.ptr()), c.BT, Rp, c.O, C.DT[dtype], L.ptr(err), None),
            c.name)
    torch.cuda.synchronize()
    msg = D.first_difference(out.result(c.name), C.storage(prob.ref, dtype), c.BT, f"{c.name} [{dtype}] (b = 0, t = sample)")
    assert msg is None, msg
    assert int(err.item()) == C.ERR_TARGET_ID | (C.ERR_CLASS_ID if c.bad else 0), (c.name, int(err.item()))
