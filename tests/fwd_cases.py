"""The launches of tests/test_gpu_fwd_kernels.py (wae_glu_layer_fwd / _drop / _list, wae_head_fwd, wae_head_fwd_from_h0,
wae_first_conv_fwd) as data, their operands, dense weights, packed weight streams and float64 expectations (tests/fwd_ref.py) on the
host -- no device is touched here, so tests/test_fwd_ref_cpu.py can assert every precondition of every case without one.

A case is ONE launch.  Case lists are one-factor-at-a-time sweeps around a base launch (LAYER_BASE / LAYER_AXES, HEAD_BASE /
HEAD_AXES), time sweeps per kernel path with and without the z save, and a few combined cases.  The dense weights go into a small
fp32 parameter arena (packing.Geometry / ParamLayout, no weight norm; every other slot of the arena holds 7.0) and the streams are
gathered from it through the PRODUCT's maps -- packing.glu_w1_map, glu_w2_map, glu_bias2_map, head_w_map, head_bias_map,
first_conv_maps -- so kernel and packing map are tested together against dense arithmetic.

Layer KINDS:
  "sat"    x, x_conv, c and the a-half of zb are 64 {-1, 0, 1}; W1 / Wc rows hold 2, 4 or 8 nonzeros of +-1 / +-2 at varying taps and
           columns; the b-half of zb is 64 * 18.  Every z is 64 n (|n| <= 17 in the a-half, n >= 2 in the b-half): exact in bf16 and fp16,
           and the gate of such a z is exactly -1, 0 or +1.  W_out is dense from [-3, 3]: y + x is an integer and
           x_out = storage(fp32(y + x) * fp32(sqrt(.5))) -- one fp32 product, then the storage rounding.  z, u and x_out are all exact.
  "dense"  every GEMM-1 operand and weight from [-3, 3]: every element of the W1 stream takes part; z is exact (one rounding to
           storage), u and x_out are held to the rounding bounds.
  "gauss"  Gaussian operands and weights rounded to storage, z about N(0, 1.5) with a few channels at +-20: the rounding bounds.
  "gate"   the gate alone: x, c from [-3, 3] / 8, sparse W1 / Wc, zb Gaussian in multiples of 2^-12 with a few channels at +-20 -- z is
           about N(0, 1.5) AND exact in fp32 in any order (multiples of 2^-12 below 64), so u's error is the gate's own: the cases from
           which the bound's k is measured.
Head KINDS: "rep" (sparse weights) and "dense" (h0, h1 and the fp32 logits exact, with both hand-overs restated), "ce" (sparse
weights, one class at least 128 above all others in every column: lse and nll exact) and "gauss".

fwd_path / head_path restate the dispatch of csrc/glu_fwd.hip (launch_glu), csrc/glu_fwd_static.hip (wae_glu_static_launch,
dispatch_static), csrc/glu_fwd_list.hip and csrc/head_fwd.hip (launch_head): every case names the kernel it reaches in a dtype."""
import functools
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

import fwd_ref as R
from tm_cases import DT, DTYPES, EXACT_LIMIT, T128, T256, T_ALL, TORCH_DT, _rng, _sweep, gather, half_ulp, storage  # noqa: F401
from wavenet_autoencoders_amd import packing as P

SAVE_Z, NO_OUT, WAVES4, CG2, PAIR, GENERIC = 2, 4, 8, 16, 32, 64      # include/wae.h: WAE_GLU_*
ONLY16 = WAVES4 | CG2 | GENERIC                                      # flags that change nothing in fp32
ERR_CLASS_ID, ERR_TARGET_ID = 1, 4                                  # include/wae.h: WAE_ERR_*
D16 = ("bf16", "fp16")
ARENA_FILL = 7.0            # what every slot of the arena holds that no map of the launch may point to
ZB_PAD = 8                  # zb_stride = 2 Hp + ZB_PAD; the foreign columns hold 1024.0
STATIC = ((256, 192), (256, 128), (512, 256))
SHARE = 0.10                # "sat": each of -1, 0, +1 makes up at least this share of u
GATE_UNIT = 2.0 ** -12      # "gate": every z is a multiple of it


def _ru(x, m):
    return (x + m - 1) // m * m


# ========================================================================================================== the gated layer
class LayerCase(NamedTuple):
    name: str
    kind: str                       # "sat" | "dense" | "gauss" | "gate"
    entry: str                      # "fwd" | "drop" | "list"
    R: int
    H: int
    Cc: int                         # 0: no conditioning operand
    k: int
    d: int
    B: int                          # clips (list: rows of zb)
    T: int                          # (list: unused)
    flags: int
    items: Tuple[Tuple[int, int], ...] = ()     # list: the items' lengths as (a, b) = a * TW + b, TW the dtype's tile; T = 0: a malformed record
    zb_rows: Tuple[int, ...] = ()
    dts: Tuple[str, ...] = DTYPES

    @property
    def Rp(self):
        return _ru(self.R, 128)

    @property
    def Hp(self):
        return _ru(self.H, 32)

    @property
    def Ccp(self):
        return _ru(self.Cc, 64) if self.Cc > 0 else 0


LAYER_BASE = dict(entry="fwd", R=100, H=50, Cc=40, k=2, d=2, B=2, T=33, flags=SAVE_Z)
_FLAG_AXIS = tuple(f | s for f in (0, PAIR, GENERIC, GENERIC | PAIR, CG2, WAVES4, NO_OUT) for s in (SAVE_Z, 0))
_D_AXIS = (1, 2, 31, 32, 33, 128, 512, "T-1", "T", "T+5")
LAYER_AXES = dict(T=T_ALL, d=_D_AXIS, k=(1, 2, 3, 5), Cc=(0, 40, 64, 100, 128), H=(20, 32, 50, 64, 96, 128, 180, 192, 256),
                  R=(100, 128, 200, 256, 512), B=(1, 2, 3), flags=_FLAG_AXIS, entry=("fwd", "drop"))
STATIC_BASE = {
    (256, 192): dict(R=256, H=184, Cc=40, k=3, d=2, B=3, T=33, flags=SAVE_Z),      # (the benchmark's layer: G = 368)
    (256, 128): dict(R=200, H=128, Cc=64, k=3, d=2, B=3, T=33, flags=SAVE_Z),
    (512, 256): dict(R=512, H=256, Cc=40, k=3, d=2, B=3, T=33, flags=SAVE_Z),
}
# time sweeps per kernel path: (what differs from the base, the path's tile set, dtypes), each with and without the z save
LAYER_T_SWEEPS = (
    (dict(), T256, D16),                                   # generic-8x32
    (dict(), T128, ("fp32",)),                             # fp32-4x32
    (dict(flags=CG2), T256, D16),                          # generic-4x64
    (dict(flags=WAVES4), T128, D16),                       # generic-4x32
) + tuple((b, T256, D16) for b in STATIC_BASE.values())
LAYER_COMBINED = (
    dict(d=128, T=257, B=3), dict(d=512, T=513, B=2), dict(d=128, T=257, B=3, flags=CG2 | SAVE_Z), dict(d=33, T=129, B=3, flags=WAVES4),
    dict(d=128, T=257, B=3, flags=WAVES4 | SAVE_Z),
    dict(entry="drop", flags=CG2 | SAVE_Z, T=257, kind="dense"), dict(entry="drop", flags=WAVES4, T=129),
    dict(entry="drop", R=200, H=128, Cc=64, k=3, B=3, T=257, kind="dense"),
    dict(entry="drop", R=256, H=184, Cc=40, k=3, B=2, T=33, flags=0), dict(entry="drop", R=512, H=256, Cc=40, k=3, B=2, T=255),
    dict(R=256, H=184, Cc=40, k=3, d=2, B=2, T=257, flags=GENERIC | SAVE_Z),
    dict(R=512, H=256, Cc=40, k=3, d=32, B=1, T=257, flags=GENERIC | PAIR), dict(R=200, H=128, Cc=64, k=3, d=33, B=3, T=257, flags=CG2),
    dict(R=256, H=96, Cc=100, k=5, d=31, B=2, T=129, flags=WAVES4 | SAVE_Z), dict(R=256, H=180, Cc=0, k=3, d=2, B=3, T=129),
    dict(R=512, H=256, Cc=128, k=2, d=1, B=1, T=97, flags=NO_OUT | SAVE_Z), dict(R=200, H=128, Cc=64, k=3, d=2, B=2, T=33, flags=NO_OUT),
) + tuple(dict(R=200, H=128, Cc=64, k=3, d=2, B=2, T=33, flags=f) for f in _FLAG_AXIS)
# wae_glu_layer_fwd_list: items as (a, b) = a * TW + b; adjacent, no margin between them
_L3 = ((0, 1), (1, 1), (0, 33))
_L4 = ((0, 33), (2, 0), (0, 1), (1, -1))
LAYER_LISTS = (
    dict(items=_L3), dict(items=_L4, zb_rows=(2, 0, 3, 1)), dict(items=_L3, flags=NO_OUT), dict(items=_L4, flags=PAIR, zb_rows=(3, 2, 1, 0)),
    dict(items=((0, 33), (0, 0), (1, 1), (0, 5)), zb_rows=(1, 3, 0, 2)),                     # the second record is malformed (T = 0) ...
    dict(items=((0, 33), (0, 0), (1, 1), (0, 5)), zb_rows=(1, 3, 0, 2), kind="sat"),         # ... its neighbours compared exactly
    dict(items=((1, 1), (0, 0), (0, 33)), zb_rows=(2, 0, 1), kind="sat", flags=NO_OUT),
    dict(items=((2, 1), (1, 0), (0, 1)), R=200, H=128, Cc=64, k=3, d=33), dict(items=_L4, R=256, H=184, Cc=40, k=3, d=2, flags=PAIR),
    dict(items=_L3, R=128, H=256, Cc=0, k=2, d=1), dict(items=_L3, H=96, k=5, d=31), dict(items=_L4, H=20, k=1, Cc=128, zb_rows=(0, 0, 1, 1)),
)
LIST_LENGTHS = ((0, 1), (0, 33), (1, -1), (1, 0), (1, 1), (2, 1))        # what the list paths' items must cover between them
LAYER_ROUNDING = (
    (dict(R=256, H=184, Cc=40, k=3, d=17, B=2, T=513, flags=SAVE_Z), D16), (dict(R=200, H=128, Cc=64, k=3, d=17, B=2, T=513, flags=SAVE_Z), D16),
    (dict(R=512, H=256, Cc=40, k=3, d=17, B=2, T=513, flags=SAVE_Z), D16), (dict(R=512, H=256, Cc=40, k=3, d=17, B=2, T=513, flags=SAVE_Z | GENERIC), D16),
    (dict(R=256, H=184, Cc=40, k=3, d=17, B=2, T=513, flags=SAVE_Z | CG2), D16), (dict(R=256, H=96, Cc=40, k=3, d=17, B=2, T=257, flags=SAVE_Z | WAVES4), D16),
    (dict(R=256, H=184, Cc=40, k=3, d=17, B=2, T=257, flags=SAVE_Z), ("fp32",)),
    (dict(entry="list", items=((1, 1), (0, 33), (2, 0)), R=200, H=128, Cc=64, k=3, d=17, flags=0), DTYPES),
)


def layer_case(p, kind, dts):
    p = {**LAYER_BASE, **p}
    T = p["T"]
    d = {"T-1": max(T - 1, 1), "T": T, "T+5": T + 5}.get(p["d"], p["d"])
    items, zb_rows = tuple(p.get("items", ())), tuple(p.get("zb_rows", ()))
    if items:
        p["entry"] = "list"
        zb_rows = zb_rows or tuple(range(len(items)))
        p["B"], p["T"] = max(zb_rows) + 1, 0
        p["flags"] = p["flags"] & ~SAVE_Z
    if p["flags"] & ONLY16:
        dts = tuple(dt for dt in dts if dt != "fp32")
    name = "glu-" + "-".join(f"{k}{v}" for k, v in p.items() if k not in ("items", "zb_rows"))
    if items:
        name += "-items" + "_".join(f"{a}w{b:+d}" for a, b in items) + "-zb" + "".join(map(str, zb_rows))
    return LayerCase(f"{name}-{kind}", kind, p["entry"], p["R"], p["H"], p["Cc"], p["k"], d, p["B"], p["T"], p["flags"], items, zb_rows, tuple(dts))


def _layer_kinds(ps, dts_fn):
    """dense and sat by turns where the z save shows the exact z; sat (exact u and x_out) elsewhere"""
    out = []
    for i, p in enumerate(ps):
        flags = p.get("flags", LAYER_BASE["flags"])
        kind = p.get("kind") or ("dense" if (i % 2 == 0 and (flags & SAVE_Z or "items" in p)) else "sat")
        out.append(layer_case({k: v for k, v in p.items() if k != "kind"}, kind, dts_fn(p, i)))
    return out


@functools.lru_cache(maxsize=None)
def layer_cases():
    out = [layer_case(LAYER_BASE, "sat", DTYPES), layer_case(LAYER_BASE, "dense", DTYPES)]
    out += _layer_kinds(_sweep(LAYER_BASE, LAYER_AXES)[1:], lambda p, i: (D16[i & 1], "fp32"))
    for extra, tiles, dts in LAYER_T_SWEEPS:
        f = extra.get("flags", 0) & ~SAVE_Z
        for save in (SAVE_Z, 0):
            out += _layer_kinds([{**LAYER_BASE, **extra, "flags": f | save, "T": T} for T in tiles], lambda p, i: dts)
    for base in STATIC_BASE.values():           # the static shapes' dilation sweeps at B = 3
        out += _layer_kinds([{**base, "T": 257, "d": d} for d in _D_AXIS], lambda p, i: (D16[i & 1],))
    out += _layer_kinds([{**LAYER_BASE, **c} for c in LAYER_COMBINED], lambda p, i: (D16[i & 1], "fp32"))
    out += _layer_kinds([{**LAYER_BASE, "flags": 0, **c} for c in LAYER_LISTS], lambda p, i: DTYPES)
    seen, uniq = {}, []
    for c in out:           # one launch once: the same launch from two sweeps keeps the union of their dtypes
        key = c[1:-1]
        if key in seen:
            j = seen[key]
            uniq[j] = uniq[j]._replace(dts=tuple(dt for dt in DTYPES if dt in uniq[j].dts + c.dts))
        else:
            seen[key] = len(uniq)
            uniq.append(c)
    return tuple(uniq)


@functools.lru_cache(maxsize=None)
def layer_rounding_cases():
    """per path: "gauss" (the composite bounds) and "gate" (exact z: the gate's own error)"""
    return tuple(layer_case(p, kind, dts) for p, dts in LAYER_ROUNDING for kind in ("gauss", "gate"))


# refusals before any launch: (what differs from the base, a descriptor override, the return code)
LAYER_REFUSED = (
    (dict(H=160), {}, -2),                      # Hp / 32 = 5: WAE_EUNSUPPORTED
    (dict(), dict(Rp=64), -1),                  # Rp = 64: WAE_EINVAL
    (dict(), dict(no_z=True), -1),              # WAE_GLU_SAVE_Z without z_save
    (dict(items=_L3), dict(flags=SAVE_Z), -2),  # WAE_GLU_SAVE_Z on the list form
)


def list_tile(dtype):
    """include/wae.h: wae_glu_list_tile"""
    return 128 if dtype == "fp32" else 256


def list_items(c: LayerCase, dtype):
    """-> the items' lengths (0: the malformed record, which still owns LIST_BAD_ROWS rows and one tile of the grid)"""
    tw = list_tile(dtype)
    return tuple(a * tw + b for a, b in c.items)


LIST_BAD_ROWS = 5


def fwd_path(c: LayerCase, dtype: str) -> str:
    """the kernel a launch reaches: "refused", "static/256x192", "static/256x128", "static/512x256" (csrc/glu_fwd_static.hip),
    "generic-8x32" / "generic-4x64" / "generic-4x32" (csrc/glu_fwd.hip: waves x columns per wave), "fp32-4x32", "list-8x32" /
    "list-fp32-4x32" (csrc/glu_fwd_list.hip)"""
    Rp, Hp, Ccp = c.Rp, c.Hp, c.Ccp
    if Hp // 32 not in (1, 2, 3, 4, 6, 8):
        return "refused"
    if c.entry == "list":
        return "list-fp32-4x32" if dtype == "fp32" else "list-8x32"
    if dtype == "fp32":
        return "fp32-4x32"
    if not c.flags & (GENERIC | CG2 | WAVES4) and Ccp == 64 and c.k == 3 and (Rp, Hp) in STATIC and c.T * Rp * 2 < 2 ** 31:
        return f"static/{Rp}x{Hp}"
    if c.flags & CG2:
        return "generic-4x64"
    nph = P.glu_pass_tiles(Hp // 32)
    fits4 = 4 * 4096 + (Rp + 2 * Hp) * 4 + 2 * (2 * nph * 4096) <= 80 * 1024
    return "generic-4x32" if (c.flags & WAVES4 and fits4) else "generic-8x32"


FWD_PATH_TILES = {"static/256x192": T256, "static/256x128": T256, "static/512x256": T256, "generic-8x32": T256, "generic-4x64": T256,
                  "generic-4x32": T128, "fp32-4x32": T128}
FWD_PATH_DTYPES = {**{p: D16 for p in FWD_PATH_TILES}, "fp32-4x32": ("fp32",), "list-8x32": D16, "list-fp32-4x32": ("fp32",)}


class LayerProblem(NamedTuple):
    x_in: torch.Tensor              # (B, T, Rp); list: (1, rows, Rp)
    x_conv: Optional[torch.Tensor]  # the "drop" entry's convolution operand
    c_up: Optional[torch.Tensor]    # (.., Ccp)
    zb: torch.Tensor                # (B, 2 Hp + ZB_PAD)
    W1: torch.Tensor                # (2H, R, k)
    Wc: Optional[torch.Tensor]      # (2H, Cc)
    W_out: torch.Tensor             # (R, H)
    b_out: torch.Tensor             # (R)
    ref: R.LayerOut                 # in the padded layouts: z (rows, 2Hp) = [a | b], u (rows, Hp), x_out / yx (rows, Rp); rows no record owns: NaN
    owned: torch.Tensor             # (rows) bool
    table: Optional[np.ndarray]     # list: (n + 1, 4) int32 wae_glu_seg records
    ntiles: int


def _ints(rng, shape, lo=-3, hi=3):
    return torch.from_numpy(rng.randint(lo, hi + 1, size=shape).astype(np.float32))


def _gauss(rng, shape, dtype, scale=1.0):
    return (torch.from_numpy(rng.randn(*shape).astype(np.float32)) * scale).to(TORCH_DT[dtype]).float()


def _sparse_rows(rng, M, K, ones_only=False):
    """(M, K): row m holds 2, 4 or 8 nonzeros of +-1 / +-2 at varying positions"""
    W = torch.zeros(M, K)
    vals = np.array([-1, 1] if ones_only else [-2, -1, 1, 2], np.float32)
    for m in range(M):
        pos = rng.choice(K, size=min((2, 4, 8)[m % 3], K), replace=False)
        W[m, torch.from_numpy(pos).long()] = torch.from_numpy(rng.choice(vals, size=len(pos)))
    return W


def _pad_cols(a, width, fill=0.0):
    out = torch.full(a.shape[:-1] + (width,), fill, dtype=a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _layer_rows(c, dtype):
    """-> (Ts of the well-formed clips in row order, their zb rows, owned mask, table, ntiles, rows)"""
    if c.entry != "list":
        return [c.T] * c.B, list(range(c.B)), torch.ones(c.B * c.T, dtype=torch.bool), None, 0, c.B * c.T
    tw = list_tile(dtype)
    Ts, zrows, rec, owned, row, tile = [], [], [], [], 0, 0
    for T, zr in zip(list_items(c, dtype), c.zb_rows):
        rec.append((row, T, zr, tile))
        if T > 0:
            Ts.append(T)
            zrows.append(zr)
            owned += [True] * T
            row, tile = row + T, tile + (T + tw - 1) // tw
        else:
            owned += [False] * LIST_BAD_ROWS
            row, tile = row + LIST_BAD_ROWS, tile + 1
    rec.append((0, 0, 0, tile))
    if all(T > 0 for T in list_items(c, dtype)):        # the product's own planner builds the same table
        plan = P.glu_list_plan(list_items(c, dtype), tw, zb_rows=c.zb_rows)
        assert np.array_equal(plan.table, np.asarray(rec, np.int32)) and plan.ntiles == tile and plan.rows == row
    return Ts, zrows, torch.tensor(owned), np.asarray(rec, np.int32), tile, row


def _draw_layer(c, dtype, rng, rows, nzb):
    R_, H, Cc, k = c.R, c.H, c.Cc, c.k
    K = k * R_ + Cc
    if c.kind == "sat":
        tri = lambda *s: 64.0 * _ints(rng, s, -1, 1)       # noqa: E731
        x, xc, cu = tri(rows, R_), tri(rows, R_), tri(rows, max(Cc, 1))
        W = _sparse_rows(rng, 2 * H, K)
        za, zbh = tri(nzb, H), torch.full((nzb, H), 64.0 * 18)
        W_out, b_out = _ints(rng, (R_, H)), _ints(rng, (R_,))
        pad_fill = 64.0
    elif c.kind == "dense":
        x, xc, cu = _ints(rng, (rows, R_)), _ints(rng, (rows, R_)), _ints(rng, (rows, max(Cc, 1)))
        W = _ints(rng, (2 * H, K))
        za, zbh = _ints(rng, (nzb, H)), _ints(rng, (nzb, H))
        W_out, b_out = _ints(rng, (R_, H)), _ints(rng, (R_,))
        pad_fill = 3.0
    elif c.kind == "gate":
        x, xc, cu = (_ints(rng, (rows, n)) / 8.0 for n in (R_, R_, max(Cc, 1)))
        W = _sparse_rows(rng, 2 * H, K)
        zz = (torch.from_numpy(rng.randn(nzb, 2 * H).astype(np.float32)).clamp(-8, 8) * GATE_UNIT ** -1).round() * GATE_UNIT
        pos = rng.choice(2 * H, size=6, replace=False)
        zz[:, torch.from_numpy(pos).long()] = torch.from_numpy(rng.choice(np.array([-20.0, 20.0], np.float32), size=(nzb, 6)))
        za, zbh = zz[:, :H].contiguous(), zz[:, H:].contiguous()
        W_out, b_out = _ints(rng, (R_, H)), _ints(rng, (R_,))
        pad_fill = 0.375
    else:
        x, xc, cu = _gauss(rng, (rows, R_), dtype), _gauss(rng, (rows, R_), dtype), _gauss(rng, (rows, max(Cc, 1)), dtype)
        W = _gauss(rng, (2 * H, K), dtype, 1.5 / K ** 0.5)
        zz = torch.from_numpy(rng.randn(nzb, 2 * H).astype(np.float32)) * 0.3
        pos = rng.choice(2 * H, size=6, replace=False)
        zz[:, torch.from_numpy(pos).long()] = torch.from_numpy(rng.choice(np.array([-20.0, 20.0], np.float32), size=(nzb, 6)))
        za, zbh = zz[:, :H].contiguous(), zz[:, H:].contiguous()
        W_out, b_out = _gauss(rng, (R_, H), dtype, 1.0 / H ** 0.5), torch.from_numpy(rng.randn(R_).astype(np.float32))
        pad_fill = 1.0
    W1 = W[:, :k * R_].reshape(2 * H, R_, k).contiguous()
    Wc = W[:, k * R_:].contiguous() if Cc > 0 else None
    return x, xc, (cu[:, :Cc] if Cc > 0 else None), W1, Wc, za, zbh, W_out, b_out, pad_fill


def _shares(u):
    n = float(u.numel())
    return tuple(float((u == v).sum()) / n for v in (-1.0, 0.0, 1.0))


def _build_layer(c: LayerCase, dtype: str) -> LayerProblem:
    Ts, zrows, owned, table, ntiles, rows = _layer_rows(c, dtype)
    Rp, Hp, Ccp, H = c.Rp, c.Hp, c.Ccp, c.H
    for salt in range(16):          # "sat": the first draw in which -1, 0 and +1 each make up SHARE of u (asserted by the CPU test)
        rng = _rng(c.name + (f"#{salt}" if salt else ""))
        x, xc, cu, W1, Wc, za, zbh, W_out, b_out, pad_fill = _draw_layer(c, dtype, rng, rows, c.B)
        drop = c.entry == "drop"
        good = owned.nonzero().squeeze(1)
        ref = R.layer_ref(x[good], (xc if drop else x)[good], None if cu is None else cu[good], torch.cat([za, zbh], 1), W1.permute(0, 2, 1),
                          Wc, W_out, b_out, c.k, c.d, Ts, zrows)
        if c.kind != "sat" or min(_shares(ref.u)) >= SHARE:
            break

    def full(a, width, halves=False):
        out = torch.full((rows, width), float("nan"), dtype=torch.float64)
        if halves:
            out[good] = torch.cat([_pad_cols(a[:, :H], Hp), _pad_cols(a[:, H:], Hp)], 1)
        else:
            out[good] = _pad_cols(a, width)
        return out
    ref = R.LayerOut(full(ref.z, 2 * Hp, True), full(ref.u, Hp), full(ref.x_out, Rp), full(ref.yx, Rp), full(ref.zA, 2 * Hp, True),
                     full(ref.yA, Rp), ref.n1, ref.n2)
    lead = (1, rows) if c.entry == "list" else (c.B, c.T)
    # pad columns: x_in's are zeros (the residual adds them); the convolution operand of "drop" and the conditioning hold values there
    # that only a zero in the packed stream keeps out
    x_in = _pad_cols(x, Rp).view(*lead, Rp)
    x_conv = _pad_cols(xc, Rp, pad_fill).view(*lead, Rp) if drop else None
    c_up = _pad_cols(cu, Ccp, pad_fill).view(*lead, Ccp) if cu is not None else None
    zb = torch.full((c.B, 2 * Hp + ZB_PAD), 1024.0)
    zb[:, :2 * Hp] = torch.cat([_pad_cols(za, Hp), _pad_cols(zbh, Hp)], 1)
    return LayerProblem(x_in, x_conv, c_up, zb, W1, Wc, W_out, b_out, ref, owned, table, ntiles)


@functools.lru_cache(maxsize=6)
def _layer_cached(c, key):
    return _build_layer(c._replace(dts=()), key if key in DTYPES else "bf16")


def layer_problem(c: LayerCase, dtype: str) -> LayerProblem:
    """(integer operands are the same in every dtype; a list's rows depend on the dtype's tile, Gaussian values on its rounding)"""
    key = dtype if c.kind == "gauss" else (("fp32" if dtype == "fp32" else "bf16") if c.entry == "list" else "any")
    return _layer_cached(c._replace(dts=()), key)


@functools.lru_cache(maxsize=64)
def _layer_maps(R_, H, Cc, k, is16):
    g = P.Geometry(layers=1, stacks=1, R=R_, G=2 * H, S=128, O=128, Cc=Cc if Cc > 0 else -1, k=k)
    lay = P.ParamLayout(g)
    dt = P.BF16 if is16 else P.F32
    return g, lay, P.glu_w1_map(g, lay, dt), P.glu_w2_map(g, lay, dt), P.glu_bias2_map(g, lay)


def _arena(lay, tensors):
    a = torch.full((lay.total,), ARENA_FILL)
    for name, t in tensors.items():
        assert lay.numel(name) == t.numel(), (name, lay.shapes[name], t.shape)
        a[lay.off(name):lay.off(name) + t.numel()] = t.reshape(-1)
    return a


def layer_arena(c, prob, lay):
    p = "wavenet.conv_layers.0."
    t = {p + "conv.weight_v": prob.W1, p + "conv1x1_out.weight_v": prob.W_out, p + "conv1x1_out.bias": prob.b_out}
    if c.Cc > 0:
        t[p + "conv1x1c.weight_v"] = prob.Wc
    return _arena(lay, t)


def layer_streams(c: LayerCase, prob: LayerProblem, dtype: str, mutate=None):
    """-> (w_packed = [GEMM-1 stream | GEMM-2 stream] as fp32 copies of its elements, bias_out (Rp)); mutate: a function that alters
    the three maps first (a mutation check on a scratch copy: every such change must fail exact cases)"""
    g, lay, m1, m2, mb = _layer_maps(c.R, c.H, c.Cc, c.k, dtype != "fp32")
    assert (g.Rp, g.Hp, g.Ccp) == (c.Rp, c.Hp, c.Ccp)
    if mutate is not None:
        m1, m2, mb = mutate(g, lay, m1, m2, mb)
    a = layer_arena(c, prob, lay)
    w = torch.cat([gather(a, m1), gather(a, m2)])
    assert w.numel() == P.glu_packed_elems(g, DT[dtype])
    return w, gather(a, mb)


def sat_x_out(yx64, dtype):
    """the exact x_out of a "sat" case: ONE fp32 product of the integer y + x with fp32(sqrt(.5)), then the storage rounding"""
    y32 = yx64.float().numpy()
    assert np.array_equal(y32.astype(np.float64), yx64.numpy(), equal_nan=True)
    prod = (y32 * np.float32(R.SQRT_HALF)).astype(np.float32)
    return torch.from_numpy(prod).to(TORCH_DT[dtype]).float()


# ================================================================================================================ the head
class HeadCase(NamedTuple):
    name: str
    kind: str                       # "rep" | "dense" | "ce" | "gauss"
    entry: str                      # "head" | "from_h0"
    S: int
    O: int
    L: int                          # layers whose u the skip GEMM contracts
    Hh: int                         # gate channels per layer
    B: int
    T: int
    scale: float
    nulls: Tuple[str, ...]          # outputs not asked for: of "logits", "nll" (no target), "lse", "h0", "h1"
    dom: int = -1                   # "ce": the class that dominates every column
    dts: Tuple[str, ...] = DTYPES

    @property
    def Sp(self):
        return _ru(self.S, 128)

    @property
    def Op(self):
        return _ru(self.O, 128)

    @property
    def Ku(self):
        return _ru(self.L * _ru(self.Hh, 32), 64)


HEAD_BASE = dict(entry="head", S=128, O=100, L=4, Hh=20, B=3, T=33, scale=0.5, nulls=())
_NULLS = ((), ("logits",), ("nll",), ("lse",), ("h0",), ("h1",), ("logits", "lse"), ("h0", "h1", "lse"), ("nll", "h0", "h1"))
HEAD_AXES = dict(S=(100, 128, 200, 256), O=(100, 128, 129, 256, 257, 384), L=(2, 3, 4, 6, 8, 10, 18), Hh=(20, 32), B=(1, 3), T=T128,
                 scale=(1.0, 0.5, 0.25), nulls=_NULLS, entry=("head", "from_h0"))
HEAD_T_SWEEPS = ((dict(entry="from_h0"), T128, ("fp32",)), (dict(entry="from_h0"), T256, D16), (dict(entry="from_h0", S=256, O=257), T256, D16),
                 (dict(S=256, O=129, L=10), T128, DTYPES))
HEAD_COMBINED = (
    dict(S=256, O=384, L=18, B=1, T=129, scale=1.0), dict(S=200, O=257, L=3, B=3, T=97, scale=0.25), dict(entry="from_h0", S=256, O=100, B=3, T=257),
    dict(entry="from_h0", S=200, O=384, B=1, T=513, nulls=("logits",)), dict(entry="from_h0", nulls=("nll",)), dict(entry="from_h0", nulls=("h1", "lse")),
    dict(entry="from_h0", S=256, O=256, nulls=("logits", "h1")), dict(L=2, S=256, O=256, T=129), dict(L=10, T=128), dict(L=18, B=1, T=257),
)
# "ce": the dominant class over the lane halves (cls % 8 < 4 and >= 4), 31 and 32, the last class of a chunk (16 bits: 64 classes, fp32: 32), O - 1
HEAD_CE = tuple(dict(O=O, S=S, dom=dom, entry=e) for e in ("head", "from_h0") for O, S, doms in
                ((100, 128, (1, 5, 31, 32, 63, 99)), (128, 128, (127,)), (129, 256, (64, 128)), (257, 128, (255, 256)), (384, 256, (191, 383)))
                for dom in doms)
HEAD_ROUNDING = ((dict(S=256, O=257, L=18, B=2, T=257, scale=0.2357), DTYPES), (dict(entry="from_h0", S=256, O=257, B=2, T=513, scale=0.2357), DTYPES))
HEAD_REFUSED = (dict(Sp=192), dict(Op=64), dict(Ku=96), dict(nothing=True))          # WAE_EINVAL before any launch


def head_case(p, kind, dts=DTYPES):
    p = {**HEAD_BASE, **p}
    name = "head-" + "-".join(f"{k}{'+'.join(v) if k == 'nulls' else v}" for k, v in p.items())
    return HeadCase(f"{name}-{kind}", kind, p["entry"], p["S"], p["O"], p["L"], p["Hh"], p["B"], p["T"], p["scale"], tuple(p["nulls"]),
                    p.get("dom", -1), tuple(dts))


@functools.lru_cache(maxsize=None)
def head_cases():
    ps = _sweep(HEAD_BASE, HEAD_AXES)
    out = [head_case(ps[0], "rep"), head_case(ps[0], "dense")]
    out += [head_case(p, "dense" if i % 2 == 0 else "rep", (D16[i & 1], "fp32")) for i, p in enumerate(ps[1:])]
    for extra, tiles, dts in HEAD_T_SWEEPS:
        out += [head_case({**extra, "T": T}, "dense" if i % 2 == 0 else "rep", dts) for i, T in enumerate(tiles)]
    out += [head_case(p, "dense" if i % 2 == 0 else "rep", (D16[i & 1], "fp32")) for i, p in enumerate(HEAD_COMBINED)]
    out += [head_case({**p, "scale": 0.25}, "ce", (D16[i & 1], "fp32")) for i, p in enumerate(HEAD_CE)]
    seen, uniq = {}, []
    for c in out:
        key = c[1:-1]
        if key in seen:
            j = seen[key]
            uniq[j] = uniq[j]._replace(dts=tuple(dt for dt in DTYPES if dt in uniq[j].dts + c.dts))
        else:
            seen[key] = len(uniq)
            uniq.append(c)
    return tuple(uniq)


@functools.lru_cache(maxsize=None)
def head_rounding_cases():
    return tuple(head_case(p, "gauss", dts) for p, dts in HEAD_ROUNDING)


def head_path(c: HeadCase, dtype: str) -> str:
    """csrc/head_fwd.hip: launch_head -- "head4" (wae_head_fwd: 4 waves x 32 columns in every dtype), "from_h0-4" (fp32) and "from_h0-8"
    (16 bits: 8 waves, 256 columns, three-slot ring)"""
    if c.entry == "head":
        return "head4"
    return "from_h0-4" if dtype == "fp32" else "from_h0-8"


HEAD_PATH_TILES = {"head4": T128, "from_h0-4": T128, "from_h0-8": T256}
HEAD_PATH_DTYPES = {"head4": DTYPES, "from_h0-4": ("fp32",), "from_h0-8": D16}
PAD_B3 = 4096.0             # what the test writes into b3[O .. Op): a pad class that reaches the maximum or the sum is seen
CE_GAP = 128.0


class HeadProblem(NamedTuple):
    x: torch.Tensor                 # u (B, T, Ku) or h0 (B, T, Sp)
    W_skip: torch.Tensor            # (S, L, Hh)
    b_skip: torch.Tensor            # (S): the sum over the layers, as wae_sum_rows leaves it
    W1: torch.Tensor                # (S, S)
    b1: torch.Tensor
    W3: torch.Tensor                # (O, S)
    b3: torch.Tensor
    target: torch.Tensor            # (B, T) int32
    ref: Optional[R.HeadOut]        # (gauss: None -- the reference is taken from the kernel's own hand-overs, head_reference)
    unit: float                     # the smallest unit of the exact sums


def _head_dense_x(c, prob):
    """the operand over the true columns and the dense (S, Ku') skip matrix that goes with it"""
    Hp = _ru(c.Hh, 32)
    if c.entry == "from_h0":
        return prob.x[:, :, :c.S], None
    u = prob.x[:, :, :c.L * Hp].reshape(c.B, c.T, c.L, Hp)[:, :, :, :c.Hh].reshape(c.B, c.T, c.L * c.Hh)
    return u, prob.W_skip.reshape(c.S, c.L * c.Hh)


def head_reference(c: HeadCase, prob: HeadProblem, dtype: str, h0=None, h1=None) -> R.HeadOut:
    """the float64 head with both hand-overs rounded to the storage dtype; h0 / h1 (B, T, S): take these as handed over instead (a
    rounding case hands the kernel's own stored values on, so that an earlier GEMM's error is not counted twice)"""
    rnd = None if dtype == "fp32" else (lambda x: storage(x, dtype).double())
    x, Ws = _head_dense_x(c, prob)
    return R.head_ref(x, Ws, prob.b_skip, prob.W1, prob.b1, prob.W3, prob.b3, c.scale, None if "nll" in c.nulls else prob.target,
                      from_h0=c.entry == "from_h0", handed0=(lambda _: h0.double()) if h0 is not None else rnd,
                      handed1=(lambda _: h1.double()) if h1 is not None else rnd)


def _build_head(c: HeadCase, dtype: str) -> HeadProblem:
    rng = _rng(c.name)
    S, O, L, Hh, B, T = c.S, c.O, c.L, c.Hh, c.B, c.T
    Hp, Ku, Sp = _ru(Hh, 32), c.Ku, c.Sp
    kind = c.kind
    if kind == "gauss":
        W_skip = _gauss(rng, (S, L, Hh), dtype, 1.0 / (L * Hh) ** 0.5)
        W1, W3 = _gauss(rng, (S, S), dtype, (2.0 / S) ** 0.5), _gauss(rng, (O, S), dtype, 3.0 * (2.0 / S) ** 0.5)
        b_skip, b1, b3 = (torch.from_numpy(rng.randn(n).astype(np.float32)) * 0.5 for n in (S, S, O))
        u = _gauss(rng, (B, T, Ku), dtype, 1.0 / abs(c.scale))
        h0 = torch.relu(_gauss(rng, (B, T, Sp), dtype))
    else:
        sparse = kind in ("rep", "ce")
        mk = (lambda m, k: _sparse_rows(rng, m, k, ones_only=kind == "ce")) if sparse else (lambda m, k: _ints(rng, (m, k)))
        W_skip, W1, W3 = mk(S, L * Hh).view(S, L, Hh), mk(S, S), mk(O, S)
        b_skip, b1, b3 = _ints(rng, (S,)), _ints(rng, (S,)), _ints(rng, (O,))
        u = _ints(rng, (B, T, Ku))
        h0 = _ints(rng, (B, T, Sp), 0, 3)
    # pad columns of the operand (channels Hh .. Hp of a layer, columns beyond L Hp; h0: S .. Sp) hold values that only a zero in the
    # packed stream keeps out
    if c.entry == "from_h0":
        x = h0
        if kind != "gauss":
            x[:, :, S:] = 3.0
    else:
        x = u
        if kind != "gauss":
            v = x[:, :, :L * Hp].reshape(B, T, L, Hp)
            v[:, :, :, Hh:] = 3.0
            x[:, :, :L * Hp] = v.reshape(B, T, L * Hp)
            x[:, :, L * Hp:] = 3.0
    special = sorted({1, 5, 31, 32, 63, O - 1, max(c.dom, 0)} & set(range(O)))
    target = torch.from_numpy(rng.randint(0, O, size=(B, T)).astype(np.int32))
    target[:, ::2] = torch.tensor(special, dtype=torch.int32)[(torch.arange(0, T, 2) // 2) % len(special)]
    target[:, 0] = (max(c.dom, 0) + 2) % O          # (what a kernel would pick for t = T - 1 of the clip before, if it read on)
    prob = HeadProblem(x, W_skip, b_skip, W1, b1, W3, b3, target, None, 1.0)
    if kind == "gauss":
        return prob
    unit = 1.0 if c.entry == "from_h0" else min(1.0, abs(c.scale))
    if kind == "ce":
        plain = head_reference(c, prob, dtype).logits
        m = float(plain.abs().max())
        bump = float(np.ceil((2.0 * m + CE_GAP) / 64.0) * 64.0)
        b3 = b3.clone()
        b3[c.dom] += bump
        prob = prob._replace(b3=b3)
    return prob._replace(ref=head_reference(c, prob, dtype), unit=unit)


@functools.lru_cache(maxsize=6)
def _head_cached(c, dtype):
    return _build_head(c, dtype)


def head_problem(c: HeadCase, dtype: str) -> HeadProblem:
    """(the hand-overs round per dtype: every dtype has its own reference)"""
    return _head_cached(c._replace(dts=()), dtype)


@functools.lru_cache(maxsize=64)
def _head_maps(S, O, L, Hh, is16):
    g = P.Geometry(layers=L, stacks=1, R=128, G=2 * Hh, S=S, O=O, k=1)
    lay = P.ParamLayout(g)
    return g, lay, P.head_w_map(g, lay, P.BF16 if is16 else P.F32), P.head_bias_map(g, lay)


def head_streams(c: HeadCase, prob: HeadProblem, dtype: str, mutate=None):
    """-> (w_packed as fp32 copies, first element of GEMM 1's chunks (w_tail), bias = [skip-bias sum | b1 | b3 with PAD_B3 in its pads])"""
    g, lay, mw, mb = _head_maps(c.S, c.O, c.L, c.Hh, dtype != "fp32")
    assert (g.Sp, g.Op, g.Ku) == (c.Sp, c.Op, c.Ku) and mw.size == P.head_packed_elems(g, DT[dtype])
    if mutate is not None:
        mw, mb = mutate(g, lay, mw, mb)
    t = {f"wavenet.conv_layers.{l}.conv1x1_skip.weight_v": prob.W_skip[:, l, :] for l in range(c.L)}
    t.update({"wavenet.last_conv_layers.1.weight_v": prob.W1, "wavenet.last_conv_layers.1.bias": prob.b1,
              "wavenet.last_conv_layers.3.weight_v": prob.W3, "wavenet.last_conv_layers.3.bias": prob.b3})
    a = _arena(lay, t)
    bias = torch.cat([_pad_cols(prob.b_skip, c.Sp), gather(a, mb)])
    bias[2 * c.Sp + c.O:] = PAD_B3
    return gather(a, mw), c.Ku * c.Sp, bias


# ============================================================================================================ the first conv
class FcCase(NamedTuple):
    name: str
    BT: int
    R: int
    O: int
    scalar: bool
    bad: bool                       # ids -1 and O among the class ids


@functools.lru_cache(maxsize=None)
def fc_cases():
    out = []
    for BT in (1, 255, 257):
        for R_ in (100, 512):       # Rp = 128, 512
            for O in (100, 256):
                for scalar, bad in ((False, False), (False, True), (True, False)):
                    if scalar and O != 100:
                        continue
                    out.append(FcCase(f"fc-BT{BT}-R{R_}-O{O}-{'scalar' if scalar else 'ids'}{'-bad' if bad else ''}", BT, R_, O, scalar, bad))
    return tuple(out)


class FcProblem(NamedTuple):
    ids: Optional[torch.Tensor]     # (BT) int32
    xs: Optional[torch.Tensor]      # (BT) fp32
    W: torch.Tensor                 # (R, O) or (R, 1)
    bias: torch.Tensor              # (R)
    ref: torch.Tensor               # (BT, Rp) float64
    flagged: bool


@functools.lru_cache(maxsize=8)
def fc_problem(c: FcCase) -> FcProblem:
    rng = _rng(c.name)
    Rp = _ru(c.R, 128)
    W, bias = _ints(rng, (c.R, 1 if c.scalar else c.O)), _ints(rng, (c.R,))
    ids = xs = None
    if c.scalar:
        xs = _ints(rng, (c.BT,))
    else:
        ids = torch.from_numpy(rng.randint(0, c.O, size=(c.BT,)).astype(np.int32))
        ids[-1] = c.O - 1
        if c.bad:
            ids[0] = -1
            ids[c.BT // 2] = c.O if c.BT > 1 else -1
    ref, flagged = R.first_conv_ref(ids, xs, W, bias)
    return FcProblem(ids, xs, W, bias, _pad_cols(ref, Rp), flagged)


def fc_streams(c: FcCase, prob: FcProblem):
    """-> (table (O or 1, Rp), bias (Rp)) through packing.first_conv_maps"""
    g = P.Geometry(layers=1, stacks=1, R=c.R, G=64, S=128, O=c.O, k=1, scalar_input=c.scalar)
    lay = P.ParamLayout(g)
    tab, mb = P.first_conv_maps(g, lay)
    a = _arena(lay, {"wavenet.first_conv.weight_v": prob.W, "wavenet.first_conv.bias": prob.bias})
    return gather(a, tab).view(-1, g.Rp), gather(a, mb)
