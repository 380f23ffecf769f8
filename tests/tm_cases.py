"""The launches of tests/test_gpu_tm_kernels.py (wae_gemm_tm, wae_gemm_tm_ce mode 5) and tests/test_gpu_bwd_pair_kernels.py
(wae_glu_bwd_fused, wae_glu_bwd_fused_dc) as data, their operands, packed weight streams and float64 expectations (tests/tm_ref.py) on
the host -- no device is touched here, so tests/test_tm_ref_cpu.py can assert every precondition of every case without one.

A case is ONE launch.  Case lists are one-factor-at-a-time sweeps around a base launch per mode (TM_BASE / TM_AXES) or per entry
(PAIR_BASE / PAIR_AXES), time sweeps per kernel path in both launch forms, and a few combined cases.  Every case has a KIND:
  "rep"    sparse weights (8 nonzeros of +-1 / +-2 per row at varying positions): every stored value and phase A's hand-over is exact in
           bf16 and fp16, so nothing depends on a rounding;
  "dense"  weights from [-3, 3] everywhere (K >= DENSE_MIN_K, so that 16-bit results must round and ties occur): every weight element
           of the packed stream takes part;
  "gauss"  the rounding cases: normal deviates rounded to the storage dtype (mode 2 / phase B: integer GEMM operands, Gaussian z).
Operands are integers in [-3, 3]; the dense matrices are packed HERE with packing.first_gemm_map / second_gemm_map in the K order
include/wae.h states (stream_perm), so the kernels and the packing maps are tested together against dense arithmetic.

tm_path / pair_path restate the dispatch conditions of csrc/gemm_tm8.hip (tm8x_covers, wae_gemm_tm8_launch), csrc/gemm_tm.hip (launch_tm,
tm_slicing, dispatch_nt), csrc/glu_bwd.hip (dispatch_gb, the *_supported functions) and csrc/glu_bwd8.hip (wae_glu_bwd8_launch): every case
names the kernel path it reaches in a dtype."""
import functools
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

import tm_ref as R
from wavenet_autoencoders_amd import packing as P

DT = {"fp32": 0, "bf16": 1, "fp16": 2}      # include/wae.h: WAE_F32, WAE_BF16, WAE_F16
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
CK = {"fp32": 32, "bf16": 64, "fp16": 64}
DTYPES = ("bf16", "fp16", "fp32")
TM_INTERLEAVE, TM_ONE_WG = 1, 2             # include/wae.h: WAE_TM_*
COLS = (8, 64)              # a source's columns start at element 8 or 64 of a wider array ...
PAD = 8                     # ... and at least this many foreign columns follow
MARGIN = 1024.0             # what the rows around an operand array hold
EXACT_LIMIT = 2.0 ** 22
ALPHA_R = 0.70710678
ALPHAS = (1.0, 0.5, -2.0, 0.25)
DENSE_MIN_K = 512           # below it a sum of K products of [-3, 3] integers hardly reaches 256, where bf16 begins to round

T128 = (1, 31, 32, 33, 97, 128, 129, 257)       # the 128-row tiles of the generic kernels (32 rows per wave)
T256 = (1, 33, 255, 256, 257, 513)              # the 256-row kernels of csrc/gemm_tm8.hip / csrc/glu_bwd8.hip
T_ALL = tuple(sorted(set(T128) | set(T256)))
D_AXIS = (0, 1, 31, 32, 33, 128, "T-1", "T", "T+5", -1, -33, "mixed")
MIXED = (33, -1, 0, 5)


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def storage(x64, dtype):
    """float64 -> fp32 -> the storage dtype, both round to nearest even (csrc/wae_common.hpp: the (__bf16) / from_f32x4 conversions),
    returned as fp32"""
    return x64.float().to(TORCH_DT[dtype]).float()


def half_ulp(e, dtype):
    """half a unit in the last place of the storage type at |e| (an upper bound: 2^-8 |e| bf16; 2^-11 |e|, at least 2^-25, fp16; 0 fp32)"""
    if dtype == "bf16":
        return 2.0 ** -8 * e.abs()
    if dtype == "fp16":
        return (2.0 ** -11 * e.abs()).clamp(min=2.0 ** -25)
    return torch.zeros_like(e)


# ------------------------------------------------------------------------------------------------------------- packed streams
def stream_perm(cols, interleave, ck):
    """stream K index -> column of the dense (M, sum cols) matrix [source 0 | source 1 | ...]: sources back to back, or with
    WAE_TM_INTERLEAVE chunk q = column_block * nsrc + source"""
    K = sum(cols)
    kk = np.arange(K)
    if not interleave:
        return kk
    n, w = len(cols), cols[0]
    assert all(c == w for c in cols)
    q = kk // ck
    return (q % n) * w + (q // n) * ck + kk % ck


def first_index(M, K, dtype, perm=None):
    """stream element -> flat index into the dense (M, K) matrix (first-GEMM order, [slice][chunk] above 256 rows), -1: a zero"""
    perm = np.arange(K) if perm is None else perm
    return P.first_gemm_map(M, K, DT[dtype], lambda row, kk: row * K + perm[kk])


def second_index(M, K, dtype):
    """the same in accumulator-row k order (w_uo)"""
    return P.second_gemm_map(M, K, DT[dtype], lambda row, kk: row * K + kk)


def gather(W, idx):
    flat = W.reshape(-1)
    return torch.where(torch.from_numpy(idx < 0), torch.zeros(()), flat[torch.from_numpy(np.maximum(idx, 0)).long()])


# ------------------------------------------------------------------------------------------------------------------ wae_gemm_tm
class TmCase(NamedTuple):
    name: str
    kind: str                       # "rep" | "dense" | "gauss"
    mode: int
    M: int
    cols: Tuple[int, ...]           # per source
    shifts: Tuple[int, ...]
    interleave: bool
    one_array: bool                 # the sources are taps of ONE array (same pointer, stride and width)
    B: int
    T: int
    alpha: float
    one_wg: bool
    O: int = 0                      # mode 5: classes


SRC = {"1": (1, False, False), "2": (2, False, False), "3": (3, False, False), "4": (4, False, False), "uneq": (3, False, False),
       "tap3": (3, False, True), "il2": (2, True, True), "il3": (3, True, True), "il4": (4, True, True), "ild3": (3, True, False)}

TM_BASE = {
    0: dict(mode=0, M=128, src="2", w=256, d=1, B=2, T=33, alpha=1.0, one_wg=0, O=0),
    1: dict(mode=1, M=256, src="il3", w=256, d=2, B=2, T=33, alpha=0.5, one_wg=0, O=0),
    2: dict(mode=2, M=128, src="2", w=256, d=0, B=2, T=33, alpha=1.0, one_wg=0, O=0),
    3: dict(mode=3, M=256, src="1", w=512, d=0, B=2, T=33, alpha=0.5, one_wg=0, O=0),
    4: dict(mode=4, M=128, src="1", w=512, d=0, B=2, T=33, alpha=0.5, one_wg=0, O=0),
    5: dict(mode=5, M=128, src="1", w=512, d=0, B=2, T=33, alpha=1.0, one_wg=0, O=100),
}
_M01 = (32, 64, 96, 128, 192, 256, 384, 512, 640)
_SRC01 = ("1", "2", "3", "4", "uneq", "tap3", "il2", "il3", "il4", "ild3")
TM_AXES = {
    0: dict(M=_M01, src=_SRC01, w=(64, 128, 192, 256), T=T128, B=(1, 2, 3, 8, 9), d=D_AXIS),
    1: dict(M=_M01, src=_SRC01, w=(64, 128, 192, 256), T=T_ALL, B=(1, 2, 3, 8, 9), d=D_AXIS, alpha=ALPHAS, one_wg=(0, 1)),
    2: dict(M=(32, 64, 96, 128, 192, 256), src=("1", "2", "3"), w=(64, 128, 192, 256), T=T_ALL, B=(1, 2, 3, 8, 9), d=D_AXIS, one_wg=(0, 1)),
    3: dict(M=(128, 192, 256, 512), src=("1", "2"), w=(64, 128, 192, 256, 384, 512), T=T_ALL, B=(1, 3, 8, 9), d=(0, 1, -1, "T"), alpha=ALPHAS,
            one_wg=(0, 1)),
    4: dict(M=(128, 192, 256, 512), src=("1", "2"), w=(64, 128, 384), T=T128, B=(1, 3, 8, 9), d=(0, 1, -33, "T+5"), alpha=ALPHAS,
            one_wg=(0, 1)),
    5: dict(M=(128, 256), src=("1", "2"), w=(64, 128, 384), T=T128, B=(1, 3, 8, 9), d=(0, 1, -1, "T-1"), O=(100, "M")),
}
# time sweeps beside the base's: the other launch form (WAE_TM_ONE_WG), and a shape of each mode that stays on the generic kernel's
# two-workgroups-per-CU instance in 16 bits (distinct arrays; M = 64: paired, never on csrc/gemm_tm8.hip; an odd chunk count)
TM_T_SWEEPS = {1: (dict(one_wg=1), dict(src="3", w=128), dict(src="3", w=128, one_wg=1)), 2: (dict(one_wg=1), dict(M=64), dict(M=64, one_wg=1)),
               3: (dict(one_wg=1), dict(w=192), dict(w=192, one_wg=1)), 4: (dict(one_wg=1),)}
TM_COMBINED = (
    dict(mode=1, M=512, src="il3", w=256, d=33, B=3, T=257, alpha=-2.0),           # two slices of 256 rows on the 8-wave kernel
    dict(mode=1, M=512, src="il3", w=256, d=33, B=3, T=257, alpha=-2.0, one_wg=1),
    dict(mode=1, M=384, src="ild3", w=192, d=-33, B=3, T=129, alpha=0.25),          # 2 x 6 tiles, distinct arrays, negative shifts
    dict(mode=1, M=640, src="il4", w=128, d=32, B=1, T=257, alpha=1.0),             # five slices of four tiles, nsrc = 4 interleaved
    dict(mode=1, src="3", w=128, B=8),                                              # B * tiles a multiple of 8 on the paired instances
    dict(mode=2, M=64, B=8),
    dict(mode=3, w=192, B=8),
    dict(mode=0, M=640, src="uneq", w=128, d=-33, B=3, T=129),
    dict(mode=0, M=512, src="4", w=192, d="mixed", B=9, T=97),
    dict(mode=0, M=384, src="il4", w=64, d=1, B=8, T=128),
    dict(mode=2, M=256, src="1", w=192, d=0, B=3, T=257),                           # NT = 8 without the flag: never paired, odd chunk count
    dict(mode=2, M=256, src="2", w=256, d=0, B=3, T=513),
    dict(mode=2, M=192, src="2", w=256, d="mixed", B=1, T=255),
    dict(mode=2, M=64, src="2", w=128, d=-1, B=9, T=129),
    dict(mode=3, M=512, src="1", w=384, d=0, B=1, T=513, alpha=0.25),
    dict(mode=3, M=512, src="2", w=192, d=1, B=3, T=129, alpha=-2.0),
    dict(mode=4, M=512, src="2", w=192, d=1, B=3, T=257, alpha=-2.0),
    dict(mode=4, M=192, src="1", w=384, d=-1, B=8, T=128, alpha=1.0, one_wg=1),
    dict(mode=5, M=256, src="2", w=192, d=1, B=3, T=129, O=201),
    dict(mode=5, M=256, src="1", w=384, d=0, B=8, T=128, O="M"),
)
# shapes the ABI refuses (WAE_EUNSUPPORTED): M / 32 = 5 or 10; a sliced gate launch; modes 3 / 4 below four tiles; mode 5 at 192 classes
TM_REFUSED = (dict(mode=0, M=160), dict(mode=1, M=320), dict(mode=2, M=512), dict(mode=3, M=64), dict(mode=4, M=96), dict(mode=5, M=192, O=100))


def _sweep(base, axes):
    out = [dict(base)]
    for k, vals in axes.items():
        out += [{**base, k: v} for v in vals if v != base[k]]
    return out


def tm_case(p, kind=None):
    p = dict(p)
    n, il, one = SRC[p["src"]]
    cols = (64, 128, 192) if p["src"] == "uneq" else (p["w"],) * n
    T = p["T"]
    d = {"T-1": T - 1, "T": T, "T+5": T + 5}.get(p["d"], p["d"])
    if d == "mixed":
        shifts = MIXED[:n]
    else:
        shifts = tuple((n - 1 - j) * d for j in range(n)) if n > 1 else (d,)
    O = p["M"] if p["O"] == "M" else p["O"]
    name = "tm-" + "-".join(f"{k}{v}" for k, v in p.items())
    if kind is None:
        kind = "rep"
    return TmCase(f"{name}-{kind}", kind, p["mode"], p["M"], cols, shifts, il, one, p["B"], T, p["alpha"], bool(p["one_wg"]), O)


def _dense_ok(c):
    """enough terms that reach into the clip, and enough outputs, for sums beyond 256"""
    live = sum(w * max(0, c.T - abs(s)) for w, s in zip(c.cols, c.shifts)) / c.T
    return live >= 0.9 * DENSE_MIN_K and c.B * c.T * c.M >= 8192


def _kinds(ps):
    """base first (both kinds); then dense and sparse weights by turns where K allows dense"""
    out = [tm_case(ps[0], "rep")]
    if _dense_ok(tm_case(ps[0])):
        out.append(tm_case(ps[0], "dense"))
    for i, p in enumerate(ps[1:]):
        out.append(tm_case(p, "dense" if (i % 2 == 0 and _dense_ok(tm_case(p))) else "rep"))
    return out


@functools.lru_cache(maxsize=None)
def tm_cases():
    out = []
    for mode, base in TM_BASE.items():
        ps = _sweep(base, TM_AXES[mode])
        for extra in TM_T_SWEEPS.get(mode, ()):
            ps += [{**base, **extra, "T": T} for T in (T128 if extra.get("one_wg") else T_ALL)]
        ps += [{**base, **c} for c in TM_COMBINED if c["mode"] == mode]
        out += _kinds(ps)
    seen, uniq = set(), []
    for c in out:
        if c[1:] not in seen:
            seen.add(c[1:])
            uniq.append(c)
    return tuple(uniq)


def tm_dtypes(c: TmCase):
    """a dense case in both 16-bit dtypes, a sparse one in one of them by turns; fp32 too, except under WAE_TM_ONE_WG (which changes
    nothing in fp32: the unflagged twin of the case is that launch)"""
    d16 = ("bf16", "fp16") if c.kind != "rep" else (("bf16", "fp16")[zlib.crc32(c.name.encode()) & 1],)
    return d16 if c.one_wg and c.mode in (1, 2, 3, 4) else d16 + ("fp32",)


@functools.lru_cache(maxsize=None)
def tm_refused_cases():
    return tuple(tm_case({**TM_BASE[c["mode"]], **c}) for c in TM_REFUSED)


# ROUNDING: one per kernel path (tm_path) and dtype that reaches it, at the path's largest small shape
TM_ROUNDING = (
    dict(mode=0, M=640, src="uneq", w=128, d=17, B=3, T=257),
    dict(mode=1, M=512, src="il3", w=384, d=17, B=2, T=513, alpha=ALPHA_R),
    dict(mode=1, M=256, src="il3", w=384, d=17, B=3, T=257, alpha=ALPHA_R, one_wg=1),
    dict(mode=1, M=256, src="3", w=384, d=17, B=3, T=257, alpha=ALPHA_R),
    dict(mode=2, M=256, src="2", w=256, d=0, B=3, T=513),
    dict(mode=2, M=256, src="2", w=256, d=0, B=3, T=257, one_wg=1),
    dict(mode=2, M=192, src="1", w=192, d=0, B=3, T=257),
    dict(mode=3, M=512, src="1", w=1152, d=0, B=2, T=513, alpha=ALPHA_R),
    dict(mode=3, M=256, src="1", w=1152, d=0, B=3, T=257, alpha=ALPHA_R, one_wg=1),
    dict(mode=3, M=256, src="1", w=960, d=0, B=3, T=257, alpha=ALPHA_R),
    dict(mode=4, M=256, src="1", w=1152, d=0, B=3, T=257, alpha=ALPHA_R),
    dict(mode=4, M=256, src="1", w=1152, d=0, B=3, T=257, alpha=ALPHA_R, one_wg=1),
    dict(mode=5, M=256, src="1", w=1152, d=0, B=3, T=257, O=201),
)


@functools.lru_cache(maxsize=None)
def tm_rounding_cases():
    return tuple(tm_case({**TM_BASE[c["mode"]], **c}, "gauss") for c in TM_ROUNDING)


def tm_slices(M):
    """csrc/gemm_tm.hip: tm_slicing -> (tiles per slice, slices) or None"""
    nt = M // 32
    if nt in (1, 2, 3, 4, 6, 8):
        return nt, 1
    for c in (8, 6, 4):
        if nt % c == 0:
            return c, nt // c
    return None


def tm_path(c: TmCase, dtype: str) -> str:
    """the kernel a launch reaches: "refused", "tm8s/m3", "tm8x/m1", "tm8x/m2", "generic-paired/m<mode>" (two workgroups per CU,
    pairwise epilogue) or "generic-one/m<mode>" """
    sl = tm_slices(c.M)
    if sl is None or (sl[1] > 1 and c.mode in (2, 5)):
        return "refused"
    nts = sl[0]
    if (c.mode == 5 and nts not in (4, 8)) or (c.mode in (3, 4) and nts not in (4, 6, 8)):
        return "refused"
    is16, n = dtype != "fp32", len(c.cols)
    if is16 and not c.one_wg:           # csrc/gemm_tm8.hip: wae_gemm_tm8_launch, tm8x_covers
        fits = c.T * (max(c.cols) + COLS[1] + PAD) * 2 < 2 ** 31
        if c.mode == 1 and c.interleave and n <= 3 and c.M % 256 == 0 and c.one_array:
            nq = n * (c.cols[0] // 64)
            if nq >= 4 and nq % 2 == 0 and fits:
                return "tm8x/m1"
        if c.mode == 2 and not c.interleave and n <= 2 and c.M in (256, 192, 128):
            nq = sum(c.cols) // 64
            if nq >= 4 and nq % 2 == 0 and fits:
                return "tm8x/m2"
        if c.mode == 3 and n == 1 and c.shifts[0] == 0 and c.M % 256 == 0:
            nq = c.cols[0] // 64
            if nq >= 4 and nq % 2 == 0 and fits:
                return "tm8s/m3"
    paired = is16 and nts % 2 == 0 and ((c.mode == 2 and nts <= 6) or c.mode in (1, 3, 4)) and not c.one_wg     # csrc/gemm_tm.hip: launch_tm
    return f"generic-{'paired' if paired else 'one'}/m{c.mode}"


TM_PATH_TILES = {"tm8s/m3": T256, "tm8x/m1": T256, "tm8x/m2": T256, **{f"generic-one/m{m}": T128 for m in range(6)},
                 **{f"generic-paired/m{m}": T128 for m in (1, 2, 3, 4)}}


class TmProblem(NamedTuple):
    W: torch.Tensor                 # (M, K) dense, fp32 copies of the stored values, columns [source 0 | source 1 | ...]
    arrays: Tuple[torch.Tensor, ...]        # (B, T, stride) each
    src: Tuple[Tuple[int, int], ...]        # per source: (array, first column)
    aux: Optional[torch.Tensor]     # modes 1 / 2 / 4: (B, T, COLS[0] + width + PAD), the operand from column COLS[0]; modes 3 / 5: bias (M,)
    ref: R.TmOut
    max_shift: int


def _ints(rng, shape, lo=-3, hi=3):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def _gauss(rng, shape, dtype, scale=1.0):
    return (torch.from_numpy(rng.randn(*shape).astype(np.float32)) * scale).to(TORCH_DT[dtype]).float()


def _wide(rng, B, T, col0, used, kind, dtype, zero_inside=False):
    """(B, T, col0 + used + PAD) whose columns outside [col0, col0 + used) hold the same kind of data and no zero"""
    shape = (B, T, col0 + used + PAD)
    if kind == "gauss":
        return _gauss(rng, shape, dtype)
    a = _ints(rng, shape)
    for foreign in (a[:, :, :col0], a[:, :, col0 + used:]):
        foreign[foreign == 0] = 3.0
    if zero_inside:
        a[:, :, col0:col0 + used] = 0.0
    return a


def _weights(rng, M, K, kind, dtype, ones_only=False):
    if kind == "dense":
        return _ints(rng, (M, K))
    if kind == "gauss":
        return _gauss(rng, (M, K), dtype, 1.0 / K ** 0.5)
    W = torch.zeros(M, K)
    vals = np.array([-1, 1] if ones_only else [-2, -1, 1, 2], np.float32)
    for m in range(M):
        pos = rng.choice(K, size=min(8, K), replace=False)
        W[m, torch.from_numpy(pos).long()] = torch.from_numpy(rng.choice(vals, size=len(pos)))
    return W


def _gate_z(rng, shape, dtype):
    """Gaussian pre-activations, a few at +-20 (the tanh clamp of the 16-bit kernels)"""
    z = _gauss(rng, shape, dtype, 1.5)
    flat = z.view(-1)
    pos = torch.from_numpy(rng.choice(flat.numel(), size=min(64, flat.numel()), replace=False)).long()
    flat[pos] = torch.from_numpy(rng.choice(np.array([-20.0, 20.0], np.float32), size=len(pos)))
    return z


def _build_tm(c: TmCase, dtype: str) -> TmProblem:
    rng = _rng(c.name)
    B, T, M, K = c.B, c.T, c.M, sum(c.cols)
    gemm_kind = "dense" if (c.kind == "gauss" and c.mode == 2) else c.kind      # mode 2 rounding: integer GEMM operands
    W = _weights(rng, M, K, gemm_kind, dtype)
    if c.one_array:
        col0 = COLS[1]
        arrays, src = (_wide(rng, B, T, col0, c.cols[0], gemm_kind, dtype),), tuple((0, col0) for _ in c.cols)
    else:
        arrays = tuple(_wide(rng, B, T, COLS[s % 2], w, gemm_kind, dtype) for s, w in enumerate(c.cols))
        src = tuple((s, COLS[s % 2]) for s in range(len(c.cols)))
    dense = [arrays[a][:, :, c0:c0 + w] for (a, c0), w in zip(src, c.cols)]
    aux, aux_dense = None, None
    if c.mode in (1, 4):
        aux = _wide(rng, B, T, COLS[0], M, c.kind, dtype)          # (mode 4: mixed signs and zeros)
        aux_dense = aux[:, :, COLS[0]:COLS[0] + M]
    elif c.mode == 2:
        aux = _wide(rng, B, T, COLS[0], 2 * M, c.kind, dtype, zero_inside=c.kind != "gauss")
        if c.kind == "gauss":
            aux[:, :, COLS[0]:COLS[0] + 2 * M] = _gate_z(rng, (B, T, 2 * M), dtype)
        aux_dense = aux[:, :, COLS[0]:COLS[0] + 2 * M]
    elif c.mode in (3, 5):
        aux = torch.from_numpy(rng.randn(M).astype(np.float32)) if c.kind == "gauss" else _ints(rng, (M,))
        aux_dense = aux
    ref = R.tm_ref(c.mode, W, dense, c.shifts, c.alpha, aux_dense, B, T, c.O)
    return TmProblem(W, arrays, src, aux, ref, max(abs(s) for s in c.shifts))


@functools.lru_cache(maxsize=8)
def _tm_cached(c, dtype):
    return _build_tm(c, dtype)


def tm_problem(c: TmCase, dtype: str) -> TmProblem:
    """(the integer operands are the same in every dtype: one reference per case, shared by its dtypes)"""
    return _tm_cached(c, dtype if c.kind == "gauss" else "any")


def tm_stream(c: TmCase, prob: TmProblem, dtype: str):
    """the packed weight stream of the launch (fp32 copies of its elements) and the map it was gathered through"""
    idx = first_index(c.M, sum(c.cols), dtype, stream_perm(c.cols, c.interleave, CK[dtype]))
    return gather(prob.W, idx), idx


def tm_out_width(c: TmCase):
    return 2 * c.M if c.mode == 2 else c.M


# ------------------------------------------------------------------------------------- wae_glu_bwd_fused / wae_glu_bwd_fused_dc
class PairCase(NamedTuple):
    name: str
    kind: str
    Rp: int
    Hp: int
    Sp: int
    ktaps: int
    dilation: int
    B: int
    T: int
    alpha: float
    dc: bool                        # wae_glu_bwd_fused_dc (16-bit storage only)
    dc_mode: int                    # bits 0, 1 as include/wae.h; bit 2 keeps the 4-wave kernel
    last: int


PAIR_BASE = {
    "fused": dict(Rp=128, Hp=64, Sp=128, k=3, d=2, B=3, T=33, alpha=0.5, dc=0, dc_mode=0, last=0),
    "dc": dict(Rp=256, Hp=128, Sp=256, k=3, d=2, B=3, T=33, alpha=0.5, dc=1, dc_mode=1, last=0),
}
_SHAPES = ((256, 192), (256, 128), (128, 32), (128, 64), (128, 96), (128, 128))       # 16 bits refuse (128, 32) and (128, 96)
_D_PAIR = (1, 2, 32, 33, 128, "T+5")
PAIR_AXES = {
    "fused": dict(shape=_SHAPES, k=(2, 3, 4), d=_D_PAIR, T=T128, B=(1, 3), alpha=ALPHAS, Sp=(64, 128, 256)),
    "dc": dict(Hp=(128, 192), d=_D_PAIR, T=T_ALL, B=(1, 3), alpha=ALPHAS, dc_mode=(0, 1, 2, 3, 4, 5, 6, 7), last=(0, 1)),
}
PAIR_COMBINED = (
    ("fused", dict(shape=(256, 192), k=4, d=33, T=129, B=1, alpha=-2.0)),
    ("fused", dict(shape=(256, 128), k=2, d="T+5", T=97, B=3, alpha=0.25, Sp=256)),
    ("fused", dict(shape=(128, 128), k=4, d=128, T=257, B=1, alpha=1.0)),
    ("dc", dict(Hp=192, d=33, T=513, B=1, dc_mode=3, last=0)),
    ("dc", dict(Hp=192, d=128, T=255, B=3, dc_mode=2, last=1)),
    ("dc", dict(Hp=192, d=32, T=257, B=3, dc_mode=7, last=0)),
    ("dc", dict(Hp=128, d=1, T=256, B=1, dc_mode=5, last=1)),
    ("dc", dict(Rp=128, Hp=64, Sp=128, d=2, T=129, B=3, dc_mode=1, last=0)),       # (128, 64): the 4-wave kernel only
    ("dc", dict(Rp=128, Hp=64, Sp=128, d=33, T=97, B=1, dc_mode=2, last=1)),
    ("dc", dict(Hp=128, Sp=128, d=2, T=129, B=3, dc_mode=3, last=0)),              # Sp != 256: the 4-wave kernel
)


def pair_case(entry, p, kind="rep"):
    p = dict(p)
    if "shape" in p:
        p["Rp"], p["Hp"] = p.pop("shape")
    p = {**PAIR_BASE[entry], **p}
    d = p["T"] + 5 if p["d"] == "T+5" else p["d"]
    name = f"{entry}-" + "-".join(f"{k}{v}" for k, v in p.items())
    return PairCase(f"{name}-{kind}", kind, p["Rp"], p["Hp"], p["Sp"], p["k"], d, p["B"], p["T"], p["alpha"], bool(p["dc"]), p["dc_mode"], p["last"])


@functools.lru_cache(maxsize=None)
def pair_cases():
    out = []
    for entry, base in PAIR_BASE.items():
        b = dict(base)
        if entry == "fused":
            b["shape"] = (b.pop("Rp"), b.pop("Hp"))
        ps = _sweep(b, PAIR_AXES[entry])
        if entry == "dc":           # the 4-wave kernel (dc_mode bit 2) over its own tile set
            ps += [{**b, "dc_mode": 5, "T": T} for T in T128]
        ps += [{**b, **c} for e, c in PAIR_COMBINED if e == entry]
        out += [pair_case(entry, ps[0], "rep"), pair_case(entry, ps[0], "dense")]
        out += [pair_case(entry, p, "dense" if i % 2 == 0 else "rep") for i, p in enumerate(ps[1:])]
    seen, uniq = set(), []
    for c in out:
        if c[1:] not in seen:
            seen.add(c[1:])
            uniq.append(c)
    return tuple(uniq)


PAIR_ROUNDING = (
    ("fused", dict(shape=(256, 192), k=3, d=17, T=257, B=3, alpha=ALPHA_R, Sp=256)),
    ("dc", dict(Hp=192, d=17, T=513, B=3, alpha=ALPHA_R, dc_mode=1)),
    ("dc", dict(Hp=192, d=17, T=257, B=3, alpha=ALPHA_R, dc_mode=5)),
)


@functools.lru_cache(maxsize=None)
def pair_rounding_cases():
    """per path: "gauss" (Gaussian phase A, the composite bound on phase B) and "gate" (integer GEMMs and alpha = 0.5, Gaussian z: dx-hat
    and du exact)"""
    return tuple(pair_case(e, {**p, "alpha": p["alpha"] if kind == "gauss" else 0.5}, kind) for e, p in PAIR_ROUNDING for kind in ("gauss", "gate"))


def pair_dtypes(c: PairCase):
    return ("bf16", "fp16") if c.dc else DTYPES


def pair_path(c: PairCase, dtype: str) -> str:
    """"refused", "fused-fp32" (glu_bwd_fused_kernel), "pair4" / "pair4-fold" (glu_bwd_pair_kernel without / with the conditioning
    gradient) or "pair8" (csrc/glu_bwd8.hip)"""
    x, u = c.Rp // 32, c.Hp // 32
    if dtype == "fp32":
        assert not c.dc
        return "fused-fp32" if (x == 8 and u in (6, 4)) or (x == 4 and 1 <= u <= 4) else "refused"
    if c.dc and not (c.dc_mode & 4) and x == 8 and c.ktaps == 3 and c.Sp == 256 and u in (6, 4):
        return "pair8"
    if (x == 8 and u in (6, 4)) or (x == 4 and u in (2, 4)):
        return "pair4-fold" if c.dc else "pair4"
    return "refused"


PAIR_PATH_TILES = {"fused-fp32": T128, "pair4": T128, "pair4-fold": T128, "pair8": T256}


class PairProblem(NamedTuple):
    W_x: torch.Tensor               # (Rp, ktaps * 2Hp) tap by tap
    W_uo: torch.Tensor              # (Hp, Rp)
    W_us: torch.Tensor              # (Hp, Sp)
    W_c: Optional[torch.Tensor]     # (64, 2Hp)
    dzbuf: torch.Tensor             # (B, T, stride): dz_l from column DZ_COL, dz_{l-1} (prefill) from column DZ_COL + 2Hp + PAD
    g_next: torch.Tensor            # (B, T, Rp)
    dskip: torch.Tensor             # (B, T, Sp)
    z_prev: torch.Tensor            # (B, T, 2Hp)
    dc_prev: Optional[torch.Tensor]         # (B, T, 64) integers
    ref: Optional[R.PairOut]        # None for "gauss" / "gate" in 16 bits until the kernel's own dx-hat is known: pair_reference


DZ_COL = COLS[0]


def dz_cols(c: PairCase):
    """(first column of dz_l, first column of dz_{l-1}, row stride) of the shared buffer"""
    z2 = 2 * c.Hp
    return DZ_COL, DZ_COL + z2 + PAD, DZ_COL + z2 + PAD + z2 + PAD


def _build_pair(c: PairCase, dtype: str) -> PairProblem:
    rng = _rng(c.name)
    B, T, Rp, Hp, Sp, k = c.B, c.T, c.Rp, c.Hp, c.Sp, c.ktaps
    z2 = 2 * Hp
    a_kind = {"gate": "dense"}.get(c.kind, c.kind)      # phase A's operands
    b_kind = {"gauss": "dense", "gate": "dense"}.get(c.kind, c.kind)    # phase B's weights: integers in every rounding case
    W_x = _weights(rng, Rp, k * z2, a_kind, dtype)
    Wb = _weights(rng, Hp, Rp + Sp, b_kind, dtype, ones_only=True)
    W_c = _weights(rng, 64, z2, a_kind, dtype) if c.dc else None
    c0, c1, stride = dz_cols(c)
    dzbuf = _wide(rng, B, T, c0, stride - c0 - PAD, a_kind, dtype)
    g_next = _gauss(rng, (B, T, Rp), dtype) if a_kind == "gauss" else _ints(rng, (B, T, Rp))
    dskip = _ints(rng, (B, T, Sp))
    z_prev = _gate_z(rng, (B, T, z2), dtype) if c.kind in ("gauss", "gate") else torch.zeros(B, T, z2)
    dc_prev = _ints(rng, (B, T, 64)) if c.dc else None
    prob = PairProblem(W_x, Wb[:, :Rp].contiguous(), Wb[:, Rp:].contiguous(), W_c, dzbuf, g_next, dskip, z_prev, dc_prev, None)
    if c.kind in ("rep", "dense"):
        prob = prob._replace(ref=pair_reference(c, prob, dtype))
    return prob


def pair_reference(c: PairCase, prob: PairProblem, dtype: str, handed=None) -> R.PairOut:
    c0, _, _ = dz_cols(c)
    dz = prob.dzbuf[:, :, c0:c0 + 2 * c.Hp]
    rnd = None if dtype == "fp32" else (lambda x: storage(x, dtype).double())
    return R.pair_ref(prob.W_x, prob.W_uo, prob.W_us, dz, prob.g_next, prob.dskip, prob.z_prev, c.ktaps, c.dilation, c.alpha, c.B, c.T,
                      round_fn=rnd, W_c=prob.W_c, dc_prev=prob.dc_prev, dc_mode=c.dc_mode, last=c.last, handed=handed)


@functools.lru_cache(maxsize=8)
def _pair_cached(c, dtype):
    return _build_pair(c, dtype)


def pair_problem(c: PairCase, dtype: str) -> PairProblem:
    """(exact cases: the hand-over rounds per dtype, so fp32 / bf16 / fp16 each get their own reference; a "rep" case's is the same)"""
    return _pair_cached(c, dtype)


def pair_streams(c: PairCase, prob: PairProblem, dtype: str):
    """{"w_x", "w_uo", "w_us", "w_c"} -> (stream, index map): w_x interleaved in 16 bits and tap by tap in fp32, w_uo in
    accumulator-row order, w_us = the skip part of the mode-2 stream, w_c as packing.bwd_c_map lays one layer out"""
    z2 = 2 * c.Hp
    perm = stream_perm((z2,) * c.ktaps, dtype != "fp32", CK[dtype])
    maps = dict(w_x=(prob.W_x, first_index(c.Rp, c.ktaps * z2, dtype, perm)), w_uo=(prob.W_uo, second_index(c.Hp, c.Rp, dtype)),
                w_us=(prob.W_us, first_index(c.Hp, c.Sp, dtype)))
    if c.dc:
        maps["w_c"] = (prob.W_c, first_index(64, z2, dtype))
    return {k: (gather(W, idx), idx) for k, (W, idx) in maps.items()}
