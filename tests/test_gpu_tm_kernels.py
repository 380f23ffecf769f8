"""The time-major GEMM of the backward data path -- wae_gemm_tm and wae_gemm_tm_ce mode 5 (csrc/gemm_tm.hip) and their 8-wave forms
(csrc/gemm_tm8.hip: gemm_tm8s_kernel, gemm_tm8x_kernel) -- each launch called straight through the C ABI, without an engine, against
the float64 restatement of tests/tm_ref.py.  The launches are data (tests/tm_cases.py); the packed weight stream of every launch is
built there from the DENSE matrix with packing.first_gemm_map in the K order include/wae.h states, so kernel and packing map are
tested together against dense arithmetic.

EXACT cases: operands are integers in [-3, 3] (exact in bf16, fp16 and fp32), alpha is 1, 0.5, -2 or 0.25, aux / bias / residual are
small integers (mode 4's aux has mixed signs and zeros), mode 2 runs on z = 0 (tanh = 0, sigmoid = 1/2: the result is [du / 2 | 0]).
Every sum is an integer far below 2^24, so the MFMA accumulation is exact in ANY order and the expectation is the float64 value cast
to fp32 and then to the storage dtype (round to nearest even, as the kernels' conversions); the assertion is torch.equal on the float
values -- no tolerance: one missing, doubled or misplaced term, a row read one off, a wrong zero fill or a slice with the other
slice's weights fails, and the message names the first wrong (b, t, column).  "rep" cases (sparse weights: 8 nonzeros of +-1 / +-2 per
row) store only values exact in 16 bits, so they do not depend on a rounding; "dense" cases (weights in [-3, 3] everywhere, K >= 512)
see every weight element, must round in bf16 and hold exact ties.  tests/test_tm_ref_cpu.py asserts these preconditions without a
device.  Every launch runs once.
OPERANDS: every source is a column slice (from element 8 or 64) of a wider array whose other columns hold the same kind of integers;
B >= 2 in most cases, so the rows next to a clip are another clip's; the array lies in a larger allocation whose margins
(max |shift| + 64 rows either side) hold 1024.0.  OUTPUT: a column window of a wider prefilled array between 1024 sentinel elements
either side; guards and foreign columns must keep their values and every element of the window must be written (it starts as NaN).
ROUNDING cases (one per kernel path and dtype, Gaussian operands rounded to the storage dtype, alpha = 0.70710678):
  modes 0 / 1 / 3 / 4 / 5:  |got - ref64| <= 2 (n + 4) 2^-24 A + h(ref64), n the number of terms, A the reference on absolute values (the
  bound tests/test_gpu_tn_kernels.py derives), h half a unit in the last place of the storage type;
  mode 2: integer GEMM operands (du exact), Gaussian z with a few entries at +-20 (the tanh clamp): |got - e| <= h(e) + k 2^-23 |du|.
  k = 4 x the largest (|got - e| - h(e)) / (2^-23 |du|) observed on an MI355X against the float64 reference (printed; run with -s):
  observed 0.6164 (bf16: 0.43 tm8x, 0.21 generic-one, 0.62 generic-paired), 1.101 (fp16: 0.80 / 0.86 / 1.10), 1.601 (fp32, libm tanhf /
  expf) = K_OBSERVED below, hence k = 2.47, 4.40, 6.40 = K_GATE.
  Largest err / bound of the other modes on an MI355X: 0.96 (bf16) and 0.74 (fp16), both mode 0 and nearly all of it the storage
  rounding h; fp32 0.0064 (mode 0), 0.0038 (mode 3), 0.0030 (mode 5's fp32 logits): the sums themselves are nowhere near their bound.

Which case reaches which kernel path (tests/tm_cases.py: tm_path restates the dispatch; tests/test_tm_ref_cpu.py asserts that every
path is reached at every T of its tile set, with B * tiles both a multiple of 8 and not, flagged and unflagged):

  path                 kernel                                                      cases
  generic-one/m0..m5   gemm_tm_kernel, one workgroup per CU: fp32 always; 16 bits    every mode's sweeps in fp32; modes 0 / 5; every
                       with WAE_TM_ONE_WG, odd tile counts, mode 2 at NT = 8       one_wg = 1 case; M / 32 in {1, 3}; mode 2 M = 256, w = 192
  generic-paired/m1-4  gemm_tm_kernel, two workgroups per CU, pairwise epilogue    16 bits: src = "3" / "uneq" / "ild3" / "il4", M = 64 ..
                                                                                   (mode 2: M = 64, 128 with nq odd), w = 192 (mode 3), mode 4
  tm8x/m1              gemm_tm8x_kernel, residual: interleaved taps of one array   16 bits: src = "il2" / "il3", M in {256, 512}, nq even >= 4
  tm8x/m2              gemm_tm8x_kernel, gate backward, M in {128, 192, 256}       16 bits: src = "1" / "2", nq even >= 4
  tm8s/m3              gemm_tm8s_kernel (8 consumer + 4 loader waves)              16 bits: one source, shift 0, M in {256, 512}, nq even >= 4
  refused              WAE_EUNSUPPORTED before any launch                          TM_REFUSED: M / 32 in {5, 10}, sliced mode 2, modes 3 / 4
                                                                                   below four tiles, mode 5 at 192 classes
  T in {1, 31, 32, 33, 97, 128, 129, 257} on the 128-row tiles, {1, 33, 255, 256, 257, 513} on the 256-row kernels; shifts 0, 1, 31, 32, 33,
  128, T - 1, T, T + 5, -1, -33 and mixed per source; M = 384 / 512 / 640 = 2 x 6, 2 x 8, 5 x 4 slices; B in {1, 2, 3, 8, 9}."""
import ctypes

import pytest
import torch

import tm_cases as C
import tm_device as D

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# mode 2, largest (|got - e| - h(e)) / (2^-23 |du|) observed per dtype, and the bound's k = 4 x that
K_OBSERVED = {"bf16": 0.6164, "fp16": 1.101, "fp32": 1.601}
K_GATE = {dt: 4.0 * v for dt, v in K_OBSERVED.items()}
OUT_COL = 8


def _launch(c, prob, dtype, stream=None, shifts=None):
    """upload, launch ONCE -> (rc, the output window or None, the logits (B * O, T) window or None)"""
    L, lib = D.lib()
    td = C.TORCH_DT[dtype]
    margin = prob.max_shift + 64
    ops = [D.Rows(a, dtype, margin) for a in prob.arrays]
    n = len(c.cols)
    ptrs = (ctypes.c_void_p * n)(*[ops[a].at(col0) for a, col0 in prob.src])
    strides = (ctypes.c_int64 * n)(*[ops[a].stride for a, _ in prob.src])
    cols = (ctypes.c_int32 * n)(*c.cols)
    sh = (ctypes.c_int32 * n)(*(shifts or c.shifts))
    w = D.upload(C.tm_stream(c, prob, dtype)[0] if stream is None else stream, dtype)
    flags = (C.TM_INTERLEAVE if c.interleave else 0) | (C.TM_ONE_WG if c.one_wg else 0)
    desc = L.TmDesc(C.DT[dtype], c.B, c.T, c.M, n, c.mode, c.alpha, flags)
    if c.mode == 5:
        bias = prob.aux.to(D.DEV)
        # the logits are (B, O, T) contiguous, the ABI has no stride for them: a plain array between the guards, NaN before the launch
        flat = torch.full((c.B * c.O * c.T + 2 * D.GUARD,), D.SENT, dtype=torch.float32, device=D.DEV)
        flat[D.GUARD:D.GUARD + c.B * c.O * c.T] = float("nan")
        ce = L.TmCe(flat.data_ptr() + 4 * D.GUARD, None, None, None, None, 0.0, c.O)
        rc = lib.wae_gemm_tm_ce(ctypes.byref(desc), ptrs, strides, cols, sh, L.ptr(w), None, 0, L.ptr(bias), ctypes.byref(ce), None)
        torch.cuda.synchronize()
        return rc, None, flat
    out = D.Window(c.B * c.T, OUT_COL, C.tm_out_width(c), td)
    aux_ptr, aux_stride, keep = None, 0, None
    if c.mode in (1, 2, 4):
        keep = D.Rows(prob.aux, dtype, 64)
        aux_ptr, aux_stride = ctypes.c_void_p(keep.at(C.COLS[0])), keep.stride
    elif c.mode == 3:
        keep = prob.aux.to(D.DEV)
        aux_ptr = L.ptr(keep)
    rc = lib.wae_gemm_tm(ctypes.byref(desc), ptrs, strides, cols, sh, L.ptr(w), ctypes.c_void_p(out.ptr()), out.stride, aux_ptr, aux_stride, None)
    torch.cuda.synchronize()
    return rc, out, None


def _logits(c, flat, what):
    b = flat.cpu()
    n = c.B * c.O * c.T
    assert bool((b[:D.GUARD] == D.SENT).all()) and bool((b[D.GUARD + n:] == D.SENT).all()), f"{what}: a guard region was written"
    return b[D.GUARD:D.GUARD + n].view(c.B, c.O, c.T)


def _got(c, prob, dtype, **kw):
    """-> the result as (B * T, columns) fp32 (mode 5: the logits brought to (B * T, O))"""
    L, _ = D.lib()
    rc, out, flat = _launch(c, prob, dtype, **kw)
    L.check(rc, c.name)
    if c.mode == 5:
        return _logits(c, flat, c.name).transpose(1, 2).reshape(c.B * c.T, c.O)
    return out.result(c.name)


def _want64(c, prob):
    ref = prob.ref.out
    return (ref.transpose(1, 2) if c.mode == 5 else ref).reshape(c.B * c.T, -1)


def _describe(c, dtype):
    return (f"{c.name} [{dtype}, {C.tm_path(c, dtype)}] mode {c.mode}, M {c.M}, cols {c.cols}, shifts {c.shifts}, interleave {c.interleave}, "
            f"B {c.B}, T {c.T}, alpha {c.alpha}")


def _run_exact(c, dtype, **kw):
    prob = C.tm_problem(c, dtype)
    assert float(prob.ref.A.max()) < C.EXACT_LIMIT, f"{c.name}: sum of |terms| {float(prob.ref.A.max())} leaves exact fp32 arithmetic"
    want = C.storage(_want64(c, prob), "fp32" if c.mode == 5 else dtype)
    return D.first_difference(_got(c, prob, dtype, **kw), want, c.T, _describe(c, dtype))


_CASES = [(c, dt) for c in C.tm_cases() for dt in C.tm_dtypes(c)]


@pytest.mark.parametrize("c,dtype", _CASES, ids=[f"{c.name[3:]}-{dt}" for c, dt in _CASES])
def test_tm_exact(c, dtype):
    msg = _run_exact(c, dtype)
    assert msg is None, msg


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("c", C.tm_refused_cases(), ids=lambda c: c.name[3:])
def test_refused_shapes_leave_the_output_untouched(c, dtype):
    """WAE_EUNSUPPORTED (-2) before any launch: the output keeps every bit"""
    prob = C.TmProblem(torch.zeros(c.M, sum(c.cols)), tuple(torch.zeros(c.B, c.T, C.COLS[s % 2] + w + C.PAD) for s, w in enumerate(c.cols)),
                       tuple((s, C.COLS[s % 2]) for s in range(len(c.cols))),
                       torch.zeros(c.M) if c.mode in (3, 5) else torch.zeros(c.B, c.T, C.COLS[0] + 2 * c.M + C.PAD), None, 0)
    assert C.tm_path(c, dtype) == "refused"
    rc, out, flat = _launch(c, prob, dtype, stream=torch.zeros(c.M * sum(c.cols)))
    assert rc == -2, (c.name, rc)
    if c.mode == 5:
        assert bool(torch.isnan(_logits(c, flat, c.name)).all())
    else:
        assert out.untouched(), c.name


_ROUNDING = [(c, dt) for c in C.tm_rounding_cases() for dt in C.DTYPES if not (c.one_wg and dt == "fp32")]


@pytest.mark.parametrize("c,dtype", _ROUNDING, ids=[f"{c.name[3:]}-{dt}" for c, dt in _ROUNDING])
def test_rounding_bound(c, dtype):
    """Gaussian operands at the path's largest small shape: the bounds of the module docstring, per element"""
    prob = C.tm_problem(c, dtype)
    got = _got(c, prob, dtype).double()
    e = _want64(c, prob)
    h = C.half_ulp(e, "fp32" if c.mode == 5 else dtype)
    err = (got - e).abs()
    path = C.tm_path(c, dtype)
    if c.mode == 2:
        du = prob.ref.acc.reshape(c.B * c.T, -1).abs()
        du = torch.cat([du, du], dim=1)
        unit = 2.0 ** -23 * du
        live = du > 0
        worst = float(((err - h)[live] / unit[live]).max())
        print(f"wae_gemm_tm mode 2 {dtype} {path}: largest (|got - e| - h(e)) / (2^-23 |du|) = {worst:.4g}")
        bound = h + K_GATE[dtype] * unit
    else:
        bound = 2.0 * (prob.ref.n + 4.0) * U * _want_A(c, prob) + h
        worst = float((err / bound).max())
        print(f"wae_gemm_tm mode {c.mode} {dtype} {path}: largest err / (2 (n + 4) 2^-24 A + h) = {worst:.4g}")
    bad = (~(err <= bound)).nonzero()       # (an element never written is NaN: beyond every bound)
    if len(bad):
        r, col = bad[0].tolist()
        raise AssertionError(f"{_describe(c, dtype)}: {len(bad)} elements beyond the bound, first at (b {r // c.T}, t {r % c.T}, column {col}): got "
                             f"{float(got[r, col])}, want {float(e[r, col])}, bound {float(bound[r, col])}")


def _want_A(c, prob):
    A = prob.ref.A
    A = (A.transpose(1, 2) if c.mode == 5 else A).reshape(c.B * c.T, -1)
    assert bool((A > 0).all())
    return A
