"""wae_gemm_tn_tiles_det (csrc/gemm_tn.hip) -- the weight-gradient tile launch with its sums formed in a fixed order (partials, then an
ordered reduce; include/wae.h states the order) -- called straight through the C ABI on the launches of tests/tn_cases.py against the
float64 restatement of tests/tn_ref.py.  Operands, prefill, guards and the exact assertion are those of tests/test_gpu_tn_kernels.py
(its helper classes are imported, not restated).

The partials buffer lies between two 1024-float sentinel regions that must stay untouched and is itself pre-filled with the sentinel
(12288.0): an element the reduce reads and launch 1 forgot to store moves the result by a visible amount.

test_tiles_det_exact: all 97 launches of tn_cases.tile_cases() in three dtypes; the 13 whose three tiles share one C run with ordered = 1
(one reduce launch per tile in table order), the other 84 with ordered = 0.
test_tiles_det_repeats: 64 partials per element, Gaussian operands: five launches from one prefill give five equal results, each inside
|got - ref64| <= 2 (n + 4) 2^-24 A (test_gpu_tn_kernels.test_rounding_bound's bound: (n + 4) 2^-24 A bounds a round-to-nearest fp32 sum of n
terms in ANY order, so it holds for the MFMA sums of a split followed by the ordered sum of the splits).
"""
import pytest
import torch

import tn_cases as C
import test_gpu_tn_kernels as K

pytestmark = pytest.mark.gpu

EINVAL = -1
SLOT = 128 * 128


class Partials:
    """[GUARD sentinels | the buffer, pre-filled with the sentinel | GUARD sentinels]"""

    def __init__(self, floats):
        self.n = floats
        self.buf = torch.full((floats + 2 * K.GUARD,), K.SENT, dtype=torch.float32, device=K.DEV)
        self.t = self.buf[K.GUARD:K.GUARD + floats]

    def check_guards(self, what):
        b = self.buf
        assert bool((b[:K.GUARD] == K.SENT).all()) and bool((b[K.GUARD + self.n:] == K.SENT).all()), f"{what}: a guard of the partials buffer was written"


def _launch_tiles(l, prob, dtype, ordered=0, det=True, short_by=0):
    """upload, build the tile table, launch ONCE through wae_gemm_tn_tiles_det (det=False: wae_gemm_tn_tiles) -> (rc, per output set
    {name: fp32 tensor on the CPU}, the partials buffer)"""
    L, lib = K._lib()
    dt = K.DT[dtype]
    margin = prob.max_shift + 64
    Pd, Qd = (K.Operand(a, dtype, margin) for a in (prob.P, prob.Q))
    ids = prob.ids.to(K.DEV).contiguous().view(-1)
    outs = [{k: K.Guarded(v[0]) for k, v in o.bufs.items()} for o in prob.outs]
    recs = []
    for i, j in enumerate(l.jobs):
        c = outs[l.out[i]]["C"].t
        recs.append(L.TnTile(None if j.onehot is not None else Pd.at(C.COL), Qd.at(C.COL), L.ptr(ids) if j.onehot is not None else None,
                             c.data_ptr() + C.COL * 4, Pd.stride, Qd.stride, c.shape[1], j.m, j.n, j.onehot or 0, j.shift, j.ones, j.alpha))
    tiles = K._table(recs)
    part = None
    if det:
        need = lib.wae_gemm_tn_tiles_det_floats(len(recs), l.B, l.T, l.splits)
        nsp = min(l.splits, (l.T + 31) // 32)
        assert need >= len(recs) * l.B * SLOT and need % (len(recs) * l.B * SLOT) == 0 and need // (len(recs) * l.B * SLOT) <= nsp
        part = Partials(need)
        rc = lib.wae_gemm_tn_tiles_det(dt, L.ptr(tiles), len(recs), l.B, l.T, l.splits, L.ptr(part.t), need - short_by, ordered, None)
    else:
        rc = lib.wae_gemm_tn_tiles(dt, L.ptr(tiles), len(recs), l.B, l.T, l.splits, None)
    torch.cuda.synchronize()
    if part is not None:
        part.check_guards(l.name)
    return rc, [{k: g.result(f"{l.name} set {s} {k}") for k, g in o.items()} for s, o in enumerate(outs)], part


TILE_CASES = C.tile_cases()
SHARED = [l for l in TILE_CASES if len(set(l.out)) < len(l.out)]


def test_the_case_list_is_the_one_the_order_rule_was_written_for():
    assert len(TILE_CASES) == 97 and len(SHARED) == 13
    assert all("multisame" in l.name for l in SHARED)


@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32"))
@pytest.mark.parametrize("l", TILE_CASES, **K._id)
def test_tiles_det_exact(l, dtype):
    L, _ = K._lib()
    prob = K._problem(l, False, dtype)
    rc, got, _ = _launch_tiles(l, prob, dtype, ordered=int(l in SHARED))
    L.check(rc, l.name)
    K._check_exact(l, prob, got)


REPEAT = C.Launch("tiles-det-repeats", "tiles", 4, 2048, (C.Job(128, 128, -17, C.ALPHA_R), C.Job(128, 128, -17, C.ALPHA_R)), (0, 1), splits=16)


@pytest.mark.parametrize("dtype", ("bf16", "fp16", "fp32"))
def test_tiles_det_repeats(dtype):
    L, lib = K._lib()
    l = REPEAT
    assert lib.wae_gemm_tn_tiles_det_floats(2, l.B, l.T, l.splits) == 2 * 64 * SLOT        # 64 partials per element
    prob = K._problem(l, True, dtype)
    runs = []
    for _ in range(5):
        rc, got, _ = _launch_tiles(l, prob, dtype)
        L.check(rc, l.name)
        runs.append(got)
    worst = 0.0
    for s, o in enumerate(prob.outs):
        pre, exp, A, n, win = o.bufs["C"]
        for r in runs[1:]:
            assert torch.equal(r[s]["C"], runs[0][s]["C"]), f"{dtype} tile {s}: a repetition gave other bits"
        for r in runs:
            ratio = (r[s]["C"].double() - exp).abs() / (2.0 * (n + 4.0) * K.U * A)
            worst = max(worst, float(ratio.max()))
            assert float(ratio.max()) <= 1.0, f"err / bound = {float(ratio.max())} at {K._where(l, s, 'C', tuple((ratio > 1.0).nonzero()[0].tolist()))}"
    # for the record (no assertion): the atomic launch on the same problem
    base = [_launch_tiles(l, prob, dtype, det=False)[1] for _ in range(5)]
    moved = sum(any(not torch.equal(r[s]["C"], base[0][s]["C"]) for s in range(len(prob.outs))) for r in base[1:])
    print(f"wae_gemm_tn_tiles_det {dtype}: 5 of 5 runs equal, largest err / (2 (n + 4) 2^-24 A) = {worst:.3g}; "
          f"wae_gemm_tn_tiles: {moved} of 4 further runs differed from the first")


def test_tiles_det_refuses_a_short_buffer():
    L, lib = K._lib()
    l = C.tile_launch({**C.TILE_BASE, "multi": "disjoint"})
    prob = K._problem(l, False, "bf16")
    rc, got, part = _launch_tiles(l, prob, "bf16", short_by=1)
    assert rc == EINVAL and b"partials buffer" in lib.wae_last_error()
    assert bool((part.t == K.SENT).all()), "the refused call wrote into the partials buffer"
    for s, o in enumerate(prob.outs):
        assert torch.equal(got[s]["C"], o.bufs["C"][0]), "the refused call wrote into C"
