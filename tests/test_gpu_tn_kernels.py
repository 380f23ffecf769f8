"""The three weight-gradient entries -- wae_gemm_tn_tiles (csrc/gemm_tn.hip), wae_gemm_tn_stream (csrc/gemm_tn_stream.hip) and
wae_gemm_tn_static (csrc/gemm_tn_static.hip) -- each called straight through the C ABI, without an engine, against the float64
restatement of tests/tn_ref.py.  The launches are data (tests/tn_cases.py); job, tile and segment tables are built here from the
ctypes records of _lib.

EXACT cases: P and Q hold integers drawn uniformly from [-3, 3] (exact in bf16, fp16 and fp32), alpha is 1, 0.5 or -2, C / C1 / Cb
start from a nonzero integer prefill.  Every product and partial sum is then an integer (or a multiple of 0.5) far below 2^24, so
the MFMA accumulation, the VALU column sums and the fp32 atomics are exact in ANY order and the assertion is torch.equal with
(prefill + float64 update) cast to fp32 -- no tolerance: one missing, doubled or misplaced term fails, and the message names the
element.  Each case asserts that no output's sum of |terms| reaches 2^22 (tests/test_tn_ref_cpu.py asserts it without a device).
Every launch runs once.
OPERANDS: every job's columns are a slice (from element 8) of a wider array whose other columns hold the same kind of integers;
B >= 2 in most cases, so the rows around a clip are another clip's; the array lies in a larger allocation whose margins (at least
|shift| + 64 rows either side) hold 1024.0: a read that should have been a zero changes an output by a visible integer.
OUTPUTS: in the middle of guarded buffers (1024 sentinel floats either side, which must stay untouched); the columns between
n_valid and the ones columns, the columns left and right of the job's window and the rows from m_valid on lie inside ldc and must
keep their prefill.
ROUNDING cases (one per entry and dtype, the entry's largest shape, Gaussian operands rounded to the storage dtype, alpha =
0.70710678): per element |got - ref64| <= 2 (n + 4) 2^-24 A, with n the number of terms and A the reference on absolute values:
(n + 4) 2^-24 A bounds a round-to-nearest fp32 sum in any order, the factor 2 allows a faithfully rounding adder in the matrix pipe.
Largest err / bound observed on an MI355X (printed by the tests; run with -s): wae_gemm_tn_tiles 0.0011 (bf16), 0.0010 (fp16),
0.0017 (fp32); wae_gemm_tn_stream 0.0011 (bf16), 0.0012 (fp16); wae_gemm_tn_static 0.0017 (bf16), 0.0019 (fp16) -- nowhere near
0.5, so these sums give no sign of an adder that rounds other than to nearest.

Which case reaches which kernel path:

  path                                                    cases (tests/tn_cases.py)
  tile launch: 128 x 128 edges, odd m_valid / n_valid     TILE_AXES m, n in {1, 8, 31, 32, 33, 64, 127, 128}, all three dtypes
  tile launch: time splits, XCD-aware order               splits in {1, 2, 3, 16} (16 > ceil(T / 32)); B = 2, T = 97, splits = 16: gridDim.y = 8
  tile launch: ones column, one-hot operand               ones at 0 (inside n_valid), n_valid and 128 - B; m0 in {0, 128}, ids in [-1, 300)
  tile launch: tiles that share / do not share C          multi = "same" / "disjoint"
  stream: region edges, 1-KiB piece validity              STREAM_AXES m in {8 .. 384}, n in {8 .. 256}
  stream: clamped-row path, whole-slab path               every T that is no multiple of 32 / every shift < 0; T = 64, 32 with shift 0
  stream: slab skipping (t_lo), nothing useful            shift in {-32, -33, -64}; shift = -T, -(T + 5)
  stream: ones column moving with the clip                ones in {n, 256 - B}, B up to 32, one team (seg = "1")
  stream: teams, null job, both workgroup orders          ts in {1, 3, 5}, nullmid; seg = "x16" (nwg % 8 == 0) against "1", "2", "3", "7"
  stream / static: hand-written lists                     seg = "hand": one segment per slab, an empty segment, a team without segments
  static kind TAPS / COND / OUTSKIP alone                 static_cases("TAPS" / "COND" / "OUTSKIP"): team_size 1
  static: product groups                                  static_cases("GROUP"): k2, k3 (taps + COND + OUTSKIP), head (one-hot P from
                                                          wae_onehot_rows, COND with Q0 = NULL and n0_valid = 0)
  static: tile edges of a kind                            m in {8 .. 384} (OUTSKIP: .. 192), n0 / n1 in {8 .. 256} (COND: 0 .. 64), n1 = 0 with
                                                          Q1 = C1 = NULL, Cb present and NULL
  static: team mapping gridDim.x & 7 != 0                 seg = "1", "2", "3", "7", "hand", "skip"
  static: team mapping gridDim.x & 7 == 0                 seg = "x16" (team_size 5: every team made of XCD leftovers), "x48" (eight whole teams,
                                                          one leftover team, idle workgroups)
  static: swapped copy of the groups                      swap = 1 (k2, k3)
  static: skipped-slab segments                           seg = "skip" (SKIP_TS): segments wholly inside the slabs a tap skips, beginning
                                                          there, ending in the next clip's
  static: clip change inside a segment                    every seg = "1" launch with B > 1; COND at B = 3, 31, 32 moves its ones operand
  static: ragged tails through the descriptors            T in {1, 15, 17, 31, 33, 49, 65, 97, 130}; B = 32 at T = 17, 33
"""
import ctypes
import functools

import pytest
import torch

import tn_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 1024
SENT = 12288.0
U = 2.0 ** -24
DT = {"fp32": 0, "bf16": 1, "fp16": 2}      # include/wae.h: WAE_F32, WAE_BF16, WAE_F16


def _lib():
    from wavenet_autoencoders_amd import _lib as L
    return L, L.lib()


class Guarded:
    """An fp32 output in the middle of a larger buffer: [GUARD sentinels | the tensor, starting as `init` | GUARD sentinels]."""

    def __init__(self, init):
        n = init.numel()
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)

    def result(self, what):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == SENT).all()) and bool((b[b.numel() - GUARD:] == SENT).all()), f"{what}: a guard region was written"
        return b[GUARD:b.numel() - GUARD].view(self.t.shape)


class Operand:
    """A (B, T, stride) operand in the storage dtype inside a larger allocation whose margin rows hold 1024.0."""

    def __init__(self, values, dtype, margin_rows):
        B, T, stride = values.shape
        self.stride, self.es = stride, 4 if dtype == "fp32" else 2
        self.buf = torch.full((2 * margin_rows + B * T, stride), C.MARGIN, dtype=C.TORCH_DT[dtype], device=DEV)
        self.mid = self.buf[margin_rows:margin_rows + B * T]
        self.mid.copy_(values.view(B * T, stride).to(C.TORCH_DT[dtype]))

    def at(self, col):
        return self.mid.data_ptr() + col * self.es


def _table(records):
    arr = (type(records[0]) * len(records))(*records)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


@functools.lru_cache(maxsize=4)
def _built(l, gauss, dtype, seed_name):
    return C.build_problem(l, gauss, dtype, seed_name)


def _problem(l, gauss, dtype, seed_name=None):
    """(the integer operands are the same in every dtype: one reference per launch, shared by its dtypes)"""
    return _built(l, gauss, dtype if gauss else "any", seed_name)


def _launch(l, prob, dtype):
    """upload, build the tables, launch ONCE -> per output set {name: fp32 tensor on the CPU}"""
    L, lib = _lib()
    dt = DT[dtype]
    margin = prob.max_shift + 64
    Pd, Qd, Q1d = (Operand(a, dtype, margin) for a in (prob.P, prob.Q, prob.Q1))
    ids = prob.ids.to(DEV).contiguous().view(-1)
    OH = None
    if l.entry == "static" and any(j.onehot is not None for j in l.jobs):
        OH = Operand(torch.full((l.B, l.T, 128), 5.0), dtype, margin)       # every element overwritten by wae_onehot_rows
        L.check(lib.wae_onehot_rows(L.ptr(ids), ctypes.c_void_p(OH.at(0)), l.B * l.T, 128, dt, None), "onehot_rows")
    outs = [None if o is None else {k: Guarded(v[0]) for k, v in o.bufs.items()} for o in prob.outs]

    def cptr(i, name):
        o = outs[l.out[i]]
        if name not in o:
            return None
        return o[name].t.data_ptr() + (0 if name == "Cb" else C.COL * 4)

    def ldc(i, name):
        o = outs[l.out[i]]
        return o[name].t.shape[1] if name in o else 0

    recs = []
    for i, j in enumerate(l.jobs):
        if l.entry == "tiles":
            recs.append(L.TnTile(None if j.onehot is not None else Pd.at(C.COL), Qd.at(C.COL), L.ptr(ids) if j.onehot is not None else None,
                                 cptr(i, "C"), Pd.stride, Qd.stride, ldc(i, "C"), j.m, j.n, j.onehot or 0, j.shift, j.ones, j.alpha))
        elif j.m <= 0:              # a null job
            recs.append(L.TsJob() if l.entry == "stream" else L.TqJob())
        elif l.entry == "stream":
            recs.append(L.TsJob(Pd.at(C.COL), Qd.at(C.COL), cptr(i, "C"), Pd.stride, Qd.stride, ldc(i, "C"), j.m, j.n, j.shift, j.ones,
                                j.alpha, 0))
        else:
            p_ptr, p_stride = (OH.at(0), 128) if j.onehot is not None else (Pd.at(C.COL), Pd.stride)
            recs.append(L.TqJob(p_ptr, None if j.qnull else Qd.at(C.COL), Q1d.at(C.COL) if j.n1 else None, cptr(i, "C"), cptr(i, "C1"),
                                cptr(i, "Cb"), p_stride, 0 if j.qnull else Qd.stride, Q1d.stride if j.n1 else 0, ldc(i, "C"), ldc(i, "C1"),
                                j.m, j.n, j.n1, j.shift, j.ones, j.kind, j.alpha, 0))
    jobs_dev = _table(recs)
    if l.entry == "tiles":
        rc = lib.wae_gemm_tn_tiles(dt, L.ptr(jobs_dev), len(recs), l.B, l.T, l.splits, None)
    else:
        segs_dev = _table([L.TsSeg(*s) for s in (l.segs or ((0, 0, 0),))])
        team_seg = torch.tensor(l.team_seg, dtype=torch.int32, device=DEV)
        if l.entry == "stream":
            rc = lib.wae_gemm_tn_stream(dt, L.ptr(jobs_dev), L.ptr(segs_dev), L.ptr(team_seg), l.nteams, l.team_size, l.nwg, l.B, l.T,
                                        None, 0, 0, None)
        else:
            # max_clip_bytes as include/wae.h states it: (T + the largest |shift| + 32) rows x the widest p / q row in bytes
            clip_bytes = (l.T + prob.max_shift + 32) * 2 * max(Pd.stride, Qd.stride, Q1d.stride, 128)
            rc = lib.wae_gemm_tn_static(dt, L.ptr(jobs_dev), L.ptr(segs_dev), L.ptr(team_seg), l.nteams, l.team_size, l.nwg, l.B, l.T,
                                        None, None, 0, 0, max(l.team_size - 2, 0), clip_bytes, None)
    L.check(rc, l.name)
    torch.cuda.synchronize()
    return [None if o is None else {k: g.result(f"{l.name} set {s} {k}") for k, g in o.items()} for s, o in enumerate(outs)]


def _where(l, s, name, idx):
    jobs = [i for i in range(len(l.jobs)) if l.out[i] == s]
    j = l.jobs[jobs[0]]
    pos = f"Cb[{idx[0]}]" if name == "Cb" else f"{name}[row {idx[0]}][column {idx[1] - C.COL}]"
    return (f"{l.name}: table entries {jobs} (kind {j.kind}, m_valid {j.m}, n_valid {j.n}, n1_valid {j.n1}, shift {[l.jobs[i].shift for i in jobs]}, "
            f"ones_col {j.ones}, B {l.B}, T {l.T}) {pos}")


def _check_exact(l, prob, got):
    for s, o in enumerate(prob.outs):
        if o is None:
            continue
        for name, (pre, exp, A, n, win) in o.bufs.items():
            g = got[s][name]
            assert float(A.max()) < C.EXACT_LIMIT, f"{l.name} set {s} {name}: sum of |terms| {float(A.max())} leaves exact fp32 arithmetic"
            want = exp.float()
            if not torch.equal(g, want):
                bad = (g != want).nonzero()
                first = tuple(bad[0].tolist())
                raise AssertionError(f"{len(bad)} of {g.numel()} elements differ, first at {_where(l, s, name, first)}: got {float(g[first])}, "
                                     f"want {float(want[first])} (prefill {float(pre[first])})")


def _run_exact(l, dtype):
    prob = _problem(l, False, dtype)
    _check_exact(l, prob, _launch(l, prob, dtype))


TILE_CASES, STREAM_CASES = C.tile_cases(), C.stream_cases()
STATIC_CASES = {k: C.static_cases(k) for k in ("TAPS", "COND", "OUTSKIP", "GROUP")}
_id = dict(ids=lambda l: l.name.split("-", 1)[1].replace("None", "x"))


@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32"))
@pytest.mark.parametrize("l", TILE_CASES, **_id)
def test_tiles_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("l", STREAM_CASES, **_id)
def test_stream_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("l", STATIC_CASES["TAPS"], **_id)
def test_static_taps_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("l", STATIC_CASES["COND"], **_id)
def test_static_cond_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("l", STATIC_CASES["OUTSKIP"], **_id)
def test_static_outskip_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("l", STATIC_CASES["GROUP"], **_id)
def test_static_groups_exact(l, dtype):
    _run_exact(l, dtype)


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("kind", sorted(C.CROSS))
def test_same_contraction_through_all_three_entries(kind, dtype):
    """one spec per static kind through the tile, the stream and the static launch on the same operands and prefill: each exact, and
    therefore bit for bit the same C"""
    res = []
    for l in C.cross_launches(kind):
        prob = _problem(l, False, dtype, "cross-" + kind)
        got = _launch(l, prob, dtype)
        _check_exact(l, prob, got)
        res.append(got[0]["C"])
    assert res[0].shape == res[1].shape == res[2].shape
    assert torch.equal(res[0], res[1]) and torch.equal(res[0], res[2]), kind


ROUNDING = dict(tiles=(C.tile_launch, C.TILE_ROUNDING, ("bf16", "fp16", "fp32")), stream=(C.stream_launch, C.STREAM_ROUNDING, ("bf16", "fp16")),
                static=(C.static_launch, C.STATIC_ROUNDING, ("bf16", "fp16")))


@pytest.mark.parametrize("entry,dtype", [(e, d) for e, v in ROUNDING.items() for d in v[2]])
def test_rounding_bound(entry, dtype):
    """Gaussian operands at the entry's largest shape: |got - ref64| <= 2 (n + 4) 2^-24 A per element"""
    make, params, _ = ROUNDING[entry]
    l = make(params)
    prob = _problem(l, True, dtype)
    got = _launch(l, prob, dtype)
    worst = 0.0
    for s, o in enumerate(prob.outs):
        if o is None:
            continue
        for name, (pre, exp, A, n, win) in o.bufs.items():
            err = (got[s][name].double() - exp).abs()
            bound = 2.0 * (n + 4.0) * U * A
            assert bool((bound > 0).all())
            ratio = err / bound
            worst = max(worst, float(ratio.max()))
            if float(ratio.max()) > 1.0:
                first = tuple((ratio > 1.0).nonzero()[0].tolist())
                raise AssertionError(f"err / bound = {float(ratio[first])} at {_where(l, s, name, first)}: got {float(got[s][name][first])}, "
                                     f"want {float(exp[first])}")
    print(f"wae_gemm_tn_{entry} {dtype}: largest err / (2 (n + 4) 2^-24 A) = {worst:.3g}")
