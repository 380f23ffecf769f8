"""The launches of tests/test_gpu_tn_kernels.py as data, and their operands and float64 expectations (tests/tn_ref.py) on the host --
no device is touched here, so tests/test_tn_ref_cpu.py can assert the exactness precondition of every case without one.

A Launch is one call of wae_gemm_tn_tiles / wae_gemm_tn_stream / wae_gemm_tn_static: a flat job table (tiles; or the groups of a team
launch back to back), the segment lists of its teams, and for every table entry the output set it accumulates into (the swapped copy
of a static launch's groups, and tiles that write one C region, share a set).  Case lists are one-factor-at-a-time sweeps around a
base launch per entry or kind plus a fixed-seed random sample of 40 combinations each."""
import zlib
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

import tn_ref as R
from wavenet_autoencoders_amd import packing as P

TQ_TAPS, TQ_COND, TQ_OUTSKIP = 0, 1, 2     # include/wae.h: WAE_TQ_*
COL = 8                 # every job's columns start at element 8 of a wider array (16-byte aligned in every dtype) ...
PAD = 8                 # ... and at least this many foreign columns follow
EXTRA_ROWS = 3          # rows of C from m_valid on, inside the buffer: must keep their prefill
MARGIN = 1024.0         # what the rows around an operand array hold
EXACT_LIMIT = 2.0 ** 22
ALPHA_R = 0.70710678

T_AXIS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 97, 130)
SHIFTS = (0, -1, -15, -16, -17, -31, -32, -33, -64, "T-1", "T", "T+5")
ALPHAS = (1.0, 0.5, -2.0)


class Job(NamedTuple):
    m: int
    n: int
    shift: int = 0
    alpha: float = 1.0
    ones: int = -1
    kind: int = TQ_TAPS             # static launch only
    n1: int = 0                     # OUTSKIP: columns of Q1 (0: Q1 = C1 = NULL)
    cb: bool = False                # OUTSKIP: Cb requested
    onehot: Optional[int] = None    # tile launch: m0 of the one-hot form; static launch: P is the operand of wae_onehot_rows
    qnull: bool = False             # no Q operand at all (n == 0)


class Launch(NamedTuple):
    name: str
    entry: str                      # "tiles" | "stream" | "static"
    B: int
    T: int
    jobs: Tuple[Job, ...]
    out: Tuple[int, ...]            # table entry -> output set
    splits: int = 1
    team_size: int = 1
    nteams: int = 1
    nwg: int = 1
    segs: Tuple[Tuple[int, int, int], ...] = ()
    team_seg: Tuple[int, ...] = (0, 0)


def _ru(x, m):
    return (x + m - 1) // m * m


def _shift(s, T):
    return {"T-1": -(T - 1), "T": -T, "T+5": -(T + 5)}.get(s, s)


def _sweep(base, axes):
    out = [dict(base)]
    for k, vals in axes.items():
        out += [{**base, k: v} for v in vals if v != base[k]]
    return out


def _sample(base, axes, n, seed):
    rng = np.random.RandomState(seed)
    return [{**base, **{k: vals[rng.randint(len(vals))] for k, vals in axes.items()}} for _ in range(n)]


def _time_axis(p, big_b):
    """B = 32 runs at T = 17 and 33 only; symbolic shifts resolved against T"""
    p = dict(p)
    if p["B"] >= 31 and p["T"] not in (17, 33):
        p["T"] = 33 if p["T"] > 17 else 17
    assert big_b or p["B"] <= 3
    p["shift"] = _shift(p["shift"], p["T"])
    return p


def _unique(launches):
    seen, out = set(), []
    for l in launches:
        if l[1:] not in seen:
            seen.add(l[1:])
            out.append(l)
    return out


def _named(prefix, p):
    return prefix + "-" + "-".join(f"{k}{v}" for k, v in p.items())


# ------------------------------------------------------------------------------------------------------------ wae_gemm_tn_tiles
TILE_BASE = dict(B=2, T=33, shift=-1, m=33, n=31, splits=2, ones="no", onehot=None, alpha=1.0, multi="one")
TILE_AXES = dict(T=T_AXIS, B=(1, 2, 3), shift=SHIFTS, m=(1, 8, 31, 32, 33, 64, 127, 128), n=(1, 8, 31, 32, 33, 64, 127, 128),
                 splits=(1, 2, 3, 16), ones=("no", "0", "n", "end"), onehot=(None, 0, 128), alpha=ALPHAS,
                 multi=("one", "disjoint", "same"))


def tile_launch(p):
    p = _time_axis(p, big_b=False)
    B, T, m, n, shift = p["B"], p["T"], p["m"], p["n"], p["shift"]
    ones = -1
    if p["ones"] != "no":           # the ones columns are defined for shift 0 (include/wae.h)
        shift = 0
        n = min(n, 128 - B)
        ones = {"0": 0, "n": n, "end": 128 - B}[p["ones"]]
    j0 = Job(m, n, shift, p["alpha"], ones, onehot=p["onehot"])
    if p["multi"] == "disjoint":    # tiles of different shapes, each with a C of its own
        jobs, out = (j0, Job(8, 128, min(shift, -2), 0.5), Job(127, 1, 0, -2.0)), (0, 1, 2)
    elif p["multi"] == "same":      # the same C region from three tiles
        jobs, out = (j0, j0._replace(shift=0 if ones >= 0 else shift - 1), j0._replace(alpha=0.5)), (0, 0, 0)
    else:
        jobs, out = (j0,), (0,)
    return Launch(_named("tiles", p), "tiles", B, T, jobs, out, splits=p["splits"])


def tile_cases():
    ps = _sweep(TILE_BASE, TILE_AXES) + _sample(TILE_BASE, TILE_AXES, 40, 1)
    ps += [{**TILE_BASE, "T": 130, "splits": 16}, {**TILE_BASE, "T": 97, "splits": 3, "shift": -33},        # splits > ceil(T / 32), ragged splits
           {**TILE_BASE, "T": 97, "splits": 16, "multi": "disjoint"},       # gridDim.y = 8: the XCD-aware workgroup order
           {**TILE_BASE, "ones": "0", "B": 1}, {**TILE_BASE, "ones": "end", "B": 3, "m": 128, "n": 127},
           {**TILE_BASE, "onehot": 128, "m": 128, "n": 128, "T": 130, "B": 3}, {**TILE_BASE, "onehot": 0, "ones": "n"}]
    return _unique([tile_launch(p) for p in ps])


TILE_ROUNDING = dict(TILE_BASE, B=3, T=130, m=128, n=128, splits=3, alpha=ALPHA_R, shift=-17)


# ------------------------------------------------------------------------------------------------------ team launches: segments
def shares(n_groups, B, T, team_size, ncu, swap=False):
    sh = P.tn_team_shares(n_groups, B, T, team_size, ncu, swap)
    return dict(nteams=sh.nteams, nwg=sh.nwg, segs=tuple(sh.segs), team_seg=tuple(sh.team_seg))


def hand_segments(n_groups, B, T, team_size):
    """three teams: one segment per slab over the first half of every group and an empty segment; no segment at all; the rest"""
    per = B * ((T + 31) // 32)
    h = per // 2
    t0 = [(g * team_size, s, s + 1) for g in range(n_groups) for s in range(h)] + [(0, h, h)]
    t2 = [(g * team_size, h, per) for g in range(n_groups)]
    return dict(nteams=3, nwg=3 * team_size, segs=tuple(t0 + t2), team_seg=(0, len(t0), len(t0), len(t0) + len(t2)))


def skip_segments(B, T, shift, team_size):
    """two teams over one group; no cut at a clip boundary, cuts one slab into every clip and one slab behind its skipped slabs
    (slab < (-shift) >> 5): segments that lie wholly in the skipped slabs, begin there, and end in the next clip's"""
    spc = (T + 31) // 32
    per, u_lo = B * spc, (-shift) >> 5
    cuts = sorted({0, per} | {c for b in range(B) for c in (b * spc + 1, b * spc + u_lo + 1) if c < per})
    segs = [(0, a, b) for a, b in zip(cuts, cuts[1:])]
    t0, t1 = segs[0::2], segs[1::2]
    return dict(nteams=2, nwg=2 * team_size, segs=tuple(t0 + t1), team_seg=(0, len(t0), len(segs)))


def _segments(mode, n_groups, B, T, team_size, shift=0, swap=False):
    if mode == "hand":
        return hand_segments(n_groups, B, T, team_size)
    if mode == "skip":
        return skip_segments(B, T, shift, team_size)
    if mode in ("x16", "x48"):      # nwg % 8 == 0: the XCD-aware workgroup-to-team mapping
        return shares(n_groups, B, T, team_size, int(mode[1:]), swap)
    return shares(n_groups, B, T, team_size, int(mode) * team_size, swap)     # "1", "2", "3", "7": that many teams, nwg % 8 != 0 ...


def slab_rows(l: Launch):
    """table entry -> (B, T) multiplicity of every time row under the launch's segment lists (team t's member i walks job + i)"""
    spc = (l.T + 31) // 32
    w = torch.zeros(len(l.jobs), l.B * spc, dtype=torch.float64)
    for t in range(l.nteams):
        for job, sb, se in l.segs[l.team_seg[t]:l.team_seg[t + 1]]:
            assert 0 <= sb <= se <= l.B * spc
            for i in range(l.team_size):
                w[job + i, sb:se] += 1
    idx = (torch.arange(l.B).view(-1, 1) * spc + torch.arange(l.T).view(1, -1) // 32)
    return [w[j][idx] for j in range(len(l.jobs))]


# ----------------------------------------------------------------------------------------------------------- wae_gemm_tn_stream
STREAM_BASE = dict(B=2, T=33, shift=-1, m=72, n=40, ones="no", ts=1, groups=1, seg="2", nullmid=0, alpha=1.0)
STREAM_AXES = dict(T=T_AXIS, B=(1, 2, 3, 32), shift=SHIFTS, m=(8, 64, 72, 376, 384), n=(8, 32, 40, 128, 136, 248, 256),
                   ones=("no", "n", "end"), ts=(1, 3, 5), groups=(1, 3), seg=("1", "2", "3", "7", "x16", "hand"), nullmid=(0, 1),
                   alpha=ALPHAS)
STREAM_MATES = (Job(64, 40, -2, 0.5), Job(72, 8, 0, -2.0, ones=8), Job(8, 136, -33), Job(376, 248, -1, 0.5))


def stream_launch(p):
    p = _time_axis(p, big_b=True)
    B, T, m, n, shift, ts, ng = p["B"], p["T"], p["m"], p["n"], p["shift"], p["ts"], p["groups"]
    ones = -1
    if p["ones"] != "no":
        shift = 0
        n = min(n, 256 - B) // 8 * 8
        ones = n if p["ones"] == "n" else 256 - B
    jobs = []
    for g in range(ng):             # the jobs of a group share their operands; group g's taps reach g rows further back
        grp = [Job(m, n, shift if ones >= 0 else shift - g, p["alpha"], ones)] + [j._replace(shift=j.shift - g if j.ones < 0 else 0)
                                                                                  for j in STREAM_MATES[:ts - 1]]
        if p["nullmid"] and ts >= 3:
            grp[1] = Job(0, 0)      # a null job in the middle of the group
        jobs += grp
    sg = _segments(p["seg"], ng, B, T, ts)
    return Launch(_named("stream", p), "stream", B, T, tuple(jobs), tuple(range(len(jobs))), team_size=ts, **sg)


def stream_cases():
    ps = _sweep(STREAM_BASE, STREAM_AXES) + _sample(STREAM_BASE, STREAM_AXES, 40, 2)
    ps += [{**STREAM_BASE, "ts": 5, "groups": 3, "seg": s, "nullmid": 1, "T": 97} for s in ("3", "7", "x16", "hand")]
    ps += [{**STREAM_BASE, "ts": 3, "groups": 3, "seg": "x16", "B": 3, "T": 65}, {**STREAM_BASE, "B": 32, "T": 17, "ones": "end", "seg": "7"},
           {**STREAM_BASE, "m": 384, "n": 256, "T": 130, "B": 3, "shift": -33, "seg": "3"}]
    return _unique([stream_launch(p) for p in ps])


STREAM_ROUNDING = dict(STREAM_BASE, B=3, T=130, m=384, n=256, ts=5, groups=1, seg="3", alpha=ALPHA_R, shift=-17)


# ----------------------------------------------------------------------------------------------------------- wae_gemm_tn_static
SEG_MODES = ("1", "2", "3", "7", "x16", "hand")
TAPS_BASE = dict(form="TAPS", B=2, T=33, shift=-1, m=72, n=40, n1=0, ones=0, cb=0, groups=1, seg="2", swap=0, alpha=1.0)
TAPS_AXES = dict(T=T_AXIS, B=(1, 2, 3, 32), shift=SHIFTS, m=(8, 32, 40, 64, 72, 376, 384), n=(8, 32, 40, 128, 136, 248, 256),
                 groups=(1, 3), seg=SEG_MODES, alpha=ALPHAS)
COND_BASE = dict(TAPS_BASE, form="COND", shift=0, n=40, ones="min")
COND_AXES = dict(T=T_AXIS, B=(1, 2, 31, 32), m=(8, 32, 40, 64, 72, 376, 384), n=(0, 8, 32, 40, 64), ones=("min", 64, 96),
                 groups=(1, 3), seg=SEG_MODES, alpha=ALPHAS)
OUTSKIP_BASE = dict(TAPS_BASE, form="OUTSKIP", shift=0, m=72, n=136, n1=120, cb=1)
OUTSKIP_AXES = dict(T=T_AXIS, B=(1, 2, 3, 32), shift=SHIFTS, m=(8, 64, 72, 184, 192), n=(8, 120, 128, 136, 256),
                    n1=(0, 8, 120, 128, 136, 256), cb=(0, 1), groups=(1, 3), seg=SEG_MODES, alpha=ALPHAS)
GROUP_BASE = dict(TAPS_BASE, form="k3", shift=-2, m=72, n=136, n1=120, cb=1, seg="x16")
GROUP_AXES = dict(form=("k2", "k3", "head"), T=T_AXIS, B=(1, 2, 3, 32), shift=(0, -1, -2, -16, -17, -32, -33), m=(8, 64, 72, 184, 192),
                  n=(8, 128, 136, 256), groups=(1, 3), seg=("1", "2", "3", "7", "x16", "x48", "hand"), swap=(0, 1), alpha=ALPHAS)
SKIP_TS = ((130, -64), (97, -33), (65, -32), (130, -33), (130, -96))


def static_launch(p):
    p = _time_axis(p, big_b=True)
    form, B, T, m, n, n1, shift, a, ng = p["form"], p["B"], p["T"], p["m"], p["n"], p["n1"], p["shift"], p["alpha"], p["groups"]
    if form == "TAPS":
        grp = [Job(m, n, shift, a)]
    elif form == "COND":            # (its ones columns: shift 0)
        ones = _ru(n, 32) if p["ones"] == "min" else max(p["ones"], _ru(n, 32))
        grp = [Job(m, n, 0, a, ones, TQ_COND, qnull=n == 0)]
    elif form == "OUTSKIP":         # (its column sums: shift 0)
        grp = [Job(m, n, shift, a, kind=TQ_OUTSKIP, n1=n1, cb=bool(p["cb"]) and shift == 0)]
    elif form in ("k2", "k3"):      # a layer of the product: k taps of dilation -shift, COND, OUTSKIP (P narrower: u against dz)
        k = int(form[1])
        grp = [Job(m, n, (k - 1 - tap) * shift, a) for tap in range(k)]
        grp += [Job(m, 40, 0, a, 64, TQ_COND), Job(min(m, 192), n, 0, 0.5, kind=TQ_OUTSKIP, n1=n1, cb=bool(p["cb"]))]
    else:                           # backward._static_head_group: two TAPS, the one-hot TAPS, two column-sum COND jobs without Q
        grp = [Job(m, n, 0, a), Job(72, 40, 0, 0.5), Job(128, n, 0, a, onehot=0), Job(m, 0, 0, a, 256, TQ_COND, qnull=True),
               Job(72, 0, 0, -2.0, 64, TQ_COND, qnull=True)]
    ts = len(grp)
    seg, swap = p["seg"], bool(p["swap"]) and form in ("k2", "k3")
    if seg == "x48" and ts != 5:
        seg = "x16"
    jobs = [j._replace(shift=j.shift - g if (j.shift < 0 and form in ("TAPS", "OUTSKIP")) else j.shift) for g in range(ng) for j in grp]
    out = list(range(len(jobs)))
    if swap:                        # StaticStreamTable.finalize: a second copy of the groups, COND and OUTSKIP having changed places
        for g in range(ng):
            c = jobs[g * ts:(g + 1) * ts]
            jobs += c[:-2] + [c[-1], c[-2]]
            out += list(range(g * ts, (g + 1) * ts - 2)) + [(g + 1) * ts - 1, (g + 1) * ts - 2]
    if seg == "skip":
        assert ng == 1
        sg = skip_segments(B, T, min(j.shift for j in grp), ts)
    else:
        sg = _segments(seg, ng, B, T, ts, swap=swap)
    return Launch(_named("static", p), "static", B, T, tuple(jobs), tuple(out), team_size=ts, **sg)


def static_cases(kind):
    base, axes, seed = {"TAPS": (TAPS_BASE, TAPS_AXES, 3), "COND": (COND_BASE, COND_AXES, 4), "OUTSKIP": (OUTSKIP_BASE, OUTSKIP_AXES, 5),
                        "GROUP": (GROUP_BASE, GROUP_AXES, 6)}[kind]
    ps = _sweep(base, axes) + _sample(base, axes, 40, seed)
    if kind in ("TAPS", "OUTSKIP", "GROUP"):     # segments that begin inside the slabs a tap skips, end there, or lie wholly in them
        ps += [{**base, "T": T, "shift": s, "seg": "skip", "B": b, "cb": 0} for T, s in SKIP_TS for b in (2, 3)][:10 if kind != "GROUP" else 4]
    if kind == "COND":              # one team: its single segment changes clip B - 1 times
        ps += [{**base, "seg": "1", "B": b, "T": t, "n": nn} for b, t, nn in ((3, 65, 40), (32, 33, 0), (31, 17, 64), (3, 130, 8))]
    if kind == "GROUP":
        ps += [{**base, "form": f, "seg": s, "swap": w, "T": t, "B": 3} for f in ("k2", "k3") for s, w, t in (("x48", 1, 130), ("7", 1, 65), ("x16", 1, 33))]
        ps += [{**base, "form": "head", "seg": s, "T": t, "B": b} for s, t, b in (("x48", 130, 3), ("3", 33, 2), ("x16", 17, 32))]
    return _unique([static_launch(p) for p in ps])


STATIC_ROUNDING = dict(GROUP_BASE, form="k3", B=3, T=130, m=384, n=256, n1=256, cb=1, seg="x16", swap=1, alpha=ALPHA_R, shift=-17)

# one contraction that fits all three entries, per static kind (run through the entry named and compared bit for bit)
CROSS = dict(TAPS=dict(B=2, T=97, shift=-33, m=72, n=40, alpha=0.5), COND=dict(B=3, T=65, shift=0, m=64, n=32, alpha=-2.0),
             OUTSKIP=dict(B=2, T=49, shift=0, m=64, n=120, alpha=1.0))


def cross_launches(kind):
    """the spec of CROSS[kind] as a tile launch (one 128 x 128 tile), a stream launch and a static launch of that kind"""
    c = CROSS[kind]
    ones = "n" if kind == "COND" else "no"
    t = tile_launch({**TILE_BASE, **c, "ones": ones, "splits": 2})
    s = stream_launch({**STREAM_BASE, **c, "ones": ones, "seg": "3"})
    q = static_launch({**TAPS_BASE, **c, "form": kind, "ones": c["n"], "n1": 0, "cb": 0, "seg": "x16"})
    return t, s, q


def all_launches():
    out = tile_cases() + stream_cases()
    for kind in ("TAPS", "COND", "OUTSKIP", "GROUP"):
        out += static_cases(kind)
    out += [l for k in CROSS for l in cross_launches(k)]
    out += [tile_launch(TILE_ROUNDING), stream_launch(STREAM_ROUNDING), static_launch(STATIC_ROUNDING)]
    return out


# ---------------------------------------------------------------------------------------------------- operands and expectations
class OutSet(NamedTuple):
    """the buffers one job (or several that share them) accumulates into; each entry: name -> (prefill, expect64, A, n, window)"""
    bufs: dict


class Problem(NamedTuple):
    P: torch.Tensor                 # (B, T, p_stride) fp32 copies of the stored values
    Q: torch.Tensor
    Q1: torch.Tensor
    ids: torch.Tensor               # (B, T) int32
    specs: Tuple[R.TnSpec, ...]     # per table entry
    outs: Tuple[OutSet, ...]
    max_shift: int


TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def spec_of(l: Launch, j: Job) -> R.TnSpec:
    return R.TnSpec(l.B, l.T, j.m, j.n, j.shift, j.alpha, j.ones, COL, COL, j.onehot, j.n1, COL, j.cb)


def build_problem(l: Launch, gauss: bool = False, dtype: str = "bf16", seed_name: Optional[str] = None) -> Problem:
    """operands (integers in [-3, 3]; gauss: normal deviates rounded to the storage dtype) and, per output set, prefill and the
    float64 expectation prefill + sum of the updates of every table entry that points at it.  The draws are seeded by the launch's
    name (or seed_name: launches of equal shapes then get equal operands)"""
    rng = np.random.RandomState(zlib.crc32((seed_name or l.name).encode()) & 0x7fffffff)
    B, T = l.B, l.T

    def draw(used):
        """(B, T, COL + used rounded up to 8 + PAD); the columns no job of the launch owns hold no zero"""
        width = COL + _ru(used, 8) + PAD
        if gauss:
            return torch.from_numpy(rng.randn(B, T, width).astype(np.float32)).to(TORCH_DT[dtype]).float()
        a = torch.from_numpy(rng.randint(-3, 4, size=(B, T, width)).astype(np.float32))
        for foreign in (a[:, :, :COL], a[:, :, COL + used:]):
            foreign[foreign == 0] = 3.0
        return a

    live = [j for j in l.jobs if j.m > 0]
    Pa = draw(max([j.m for j in live if j.onehot is None] + [8]))
    Qa = draw(max(j.n for j in live))
    Q1a = draw(max(j.n1 for j in live))
    ids = torch.from_numpy(rng.randint(-1, 300, size=(B, T)).astype(np.int32))
    ids[0, 0] = -1
    rows = slab_rows(l) if l.entry != "tiles" else [None] * len(l.jobs)
    specs = tuple(spec_of(l, j) for j in l.jobs)
    sets = {}
    for i, (j, sp) in enumerate(zip(l.jobs, specs)):
        if j.m <= 0:
            continue
        ref = R.tn_reference(sp, Pa, Qa, ids, Q1a, rows[i])
        if l.out[i] not in sets:
            bufs = {}
            for name, o in ref.items():
                if name == "Cb":
                    shape, win = (j.n + PAD,), (slice(0, j.n),)
                else:
                    shape, win = (j.m + EXTRA_ROWS, COL + o.update.shape[1] + PAD), (slice(0, j.m), slice(COL, COL + o.update.shape[1]))
                pre = torch.from_numpy(rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), size=shape))
                bufs[name] = [pre, pre.double().clone(), pre.double().abs(), torch.ones(shape, dtype=torch.float64), win]
            sets[l.out[i]] = bufs
        for name, o in ref.items():
            pre, exp, A, n, win = sets[l.out[i]][name]
            assert exp[win].shape == o.update.shape, (l.name, i, name)
            exp[win] += o.update
            A[win] += o.A
            n[win] += o.n
    outs = tuple(OutSet({k: tuple(v) for k, v in sets[i].items()}) if i in sets else None for i in range(max(l.out) + 1))
    return Problem(Pa, Qa, Q1a, ids, specs, outs, max(abs(j.shift) for j in l.jobs))


def max_A(prob: Problem) -> float:
    return max(float(b[2].max()) for o in prob.outs if o is not None for b in o.bufs.values())
