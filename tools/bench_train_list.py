#!/usr/bin/env python
"""What a ragged train step costs (WaeEngine.train_step_list) against the way there was before it: train_step on the same utterances
zero-padded to the longest, with `lengths`.  Geometry: hps/vqwae.json.  The two ways differentiate DIFFERENT functions (the padded
batch's pad frames enter the commitment loss and the conditioning of every utterance's end: DESIGN.md), so this compares cost only.

usage: bench_train_list.py [--sizes 8,32] [--dtypes bf16,fp32] [--repeats 5] [--min-frames 100] [--max-frames 300] [--sorted]
Inputs: N utterances of --min-frames..--max-frames feature frames, multiples of 4, numpy default_rng(1234); inputs on the device.
One process, one engine per precision, warmed; the two ways alternate step by step, medians of --repeats (at least 5).  The decoder
runs on the same (N, Tmax) rows either way; what differs is the front end (packed list against padded batch: 1-2 % of a step) and the
host's packing.  Prints one line per measurement and one JSON line at the end.

usage: bench_train_list.py --accum 2,4,8 [--group 4] [--dtypes bf16,fp32] [--repeats 5]
What a ragged accumulation window saves (WaeEngine.train_step_list_accum): M groups of --group utterances as ONE window (M
accumulate_list micro-batches and one apply_step: one finish of the gradients, one optimizer pass) against M train_step_list calls on
the same groups (M finishes, M optimizer passes).  The two ways alternate in one process on one engine, medians of --repeats; then
the same window on an engine in the deterministic mode (EngineOptions.deterministic), timed alone.  The groups of a smaller M are
the first groups of the largest, so every shape's workspace is made once.  The two ways take DIFFERENT steps (one update against M):
cost only."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vqwae_train as VT  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402
from wavenet_autoencoders_amd.hparams import hparams  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_accum(args, geom, sd, hop, reps):
    """--accum: the window of M groups against M list steps, and the window in the deterministic mode"""
    Ms = sorted(int(m) for m in args.accum.split(","))
    rng = np.random.default_rng(1234)
    gen = torch.Generator().manual_seed(1234)
    groups = []
    for _ in range(Ms[-1]):
        Fs = [int(f) * 4 for f in rng.integers(args.min_frames // 4, args.max_frames // 4 + 1, args.group)]
        groups.append([dict(x=torch.randint(0, geom.O, (f * hop,), generator=gen).cuda(), c=torch.randn(geom.c_in, f, generator=gen).cuda(),
                            gid=int(i % geom.n_speakers)) for i, f in enumerate(Fs)])
    def time_mode(dtype, mode, t):
        """one engine's measurements into t; the engine and every workspace of its shapes go when this returns"""
        os.environ["WAE_DETERMINISTIC"] = "1" if mode == "deterministic" else "0"       # (read once, when the engine is created)
        eng = WaeEngine(geom, dtype=dtype)
        assert eng.opt.deterministic == (mode == "deterministic")
        eng.load_state_dict(sd, strict=False)
        eng.init_optimizer()
        for M in Ms:
            gs = groups[:M]

            def steps():
                for grp in gs:
                    eng.train_step_list(grp, lr=1e-4)
            ways = dict(window=lambda: eng.train_step_list_accum(gs, lr=1e-4))
            if mode == "default":
                ways["steps"] = steps
            for fn in ways.values():       # warm both ways: workspaces, tables, LDS opt-ins
                fn()
                fn()
            tm = {k: [] for k in ways}
            for _ in range(reps):
                for k, fn in ways.items():
                    tm[k].append(timed(fn))
            for k, v in tm.items():
                t[(M, k if mode == "default" else "det_window")] = [statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3]
            if mode == "default":
                res = eng.train_step_list_accum(gs, lr=1e-4)
                t[(M, "rows")] = (int(res["rows"]), int(res["pad_rows"]))

    out = []
    for dtype in args.dtypes.split(","):
        t = {}
        for mode in ("default", "deterministic"):
            time_mode(dtype, mode, t)
            gc.collect()
            torch.cuda.empty_cache()
        for M in Ms:
            rec = dict(dtype=dtype, M=M, group=args.group, rows=t[(M, "rows")][0], pad_rows=t[(M, "rows")][1], window_ms=t[(M, "window")],
                       steps_ms=t[(M, "steps")], det_window_ms=t[(M, "det_window")])
            rec["window_over_steps"] = rec["window_ms"][0] / rec["steps_ms"][0]
            rec["det_over_window"] = rec["det_window_ms"][0] / rec["window_ms"][0]
            out.append(rec)
            fmt = lambda v: f"{v[0]:.2f} [{v[1]:.2f}, {v[2]:.2f}]"      # noqa: E731
            print(f"{dtype} M={M} x {args.group}: rows {rec['rows']} ({rec['pad_rows']} pad), window {fmt(rec['window_ms'])} ms, "
                  f"{M} list steps {fmt(rec['steps_ms'])} ms, window / steps {rec['window_over_steps']:.3f}, deterministic window "
                  f"{fmt(rec['det_window_ms'])} ms ({rec['det_over_window']:.3f} x)")
    os.environ.pop("WAE_DETERMINISTIC", None)
    print(json.dumps(dict(bench="train_list_accum", results=out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--accum", default="", help="M1,M2,...: time a window of M groups against M list steps instead (and the window in "
                                                "the deterministic mode)")
    ap.add_argument("--group", type=int, default=4, help="--accum: utterances per group")
    ap.add_argument("--sizes", default="8,32")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-frames", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=300)
    ap.add_argument("--sorted", action="store_true", help="length-sorted lists (the pad rows are the same; the packing order differs)")
    args = ap.parse_args()
    reps = max(args.repeats, 5)
    with open(os.path.join(ROOT, "hps", "vqwae.json")) as f:
        hparams.parse_json(f.read())
    geom = VT.build_geometry(hparams)
    hop = hparams.hop_size
    from wavenet_autoencoders_amd.wavenet_vocoder._base import ArenaModel

    class _Init(ArenaModel):
        pass
    torch.manual_seed(1234)
    tmp = _Init()
    tmp._init_arena(geom, "")
    sd = {k: v.detach() for k, v in tmp.state_dict().items()}
    if args.accum:
        return bench_accum(args, geom, sd, hop, reps)
    out = []
    for dtype in args.dtypes.split(","):
        eng = WaeEngine(geom, dtype=dtype)
        eng.load_state_dict(sd, strict=False)
        eng.init_optimizer()
        for n in [int(s) for s in args.sizes.split(",")]:
            rng = np.random.default_rng(1234)
            gen = torch.Generator().manual_seed(1234)
            Fs = [int(f) * 4 for f in rng.integers(args.min_frames // 4, args.max_frames // 4 + 1, n)]
            if args.sorted:
                Fs.sort(reverse=True)
            items = [dict(x=torch.randint(0, geom.O, (f * hop,), generator=gen).cuda(), c=torch.randn(geom.c_in, f, generator=gen).cuda(),
                          gid=int(i % geom.n_speakers)) for i, f in enumerate(Fs)]
            Fm, Tm = max(Fs), max(Fs) * hop
            x, c = torch.zeros(n, Tm, dtype=torch.long, device="cuda"), torch.zeros(n, geom.c_in, Fm, device="cuda")
            for b, it in enumerate(items):
                x[b, :it["x"].shape[0]], c[b, :, :it["c"].shape[1]] = it["x"], it["c"]
            g = torch.tensor([it["gid"] for it in items]).cuda()
            lengths = torch.tensor([f * hop for f in Fs])
            ways = dict(list=lambda: eng.train_step_list(items, lr=1e-4, max_rows=n * Tm),
                        padded=lambda: eng.train_step(x, c, g, lengths=lengths, lr=1e-4))
            for fn in ways.values():       # warm both ways: workspaces, tables, LDS opt-ins
                fn()
                fn()
            t = {k: [] for k in ways}
            for _ in range(reps):
                for k, fn in ways.items():
                    t[k].append(timed(fn))
            res = eng.train_step_list(items, lr=1e-4, max_rows=n * Tm)
            rec = dict(dtype=dtype, n=n, rows=int(res["rows"]), pad_rows=int(res["pad_rows"]), frames=sum(Fs),
                       **{k + "_ms": [statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3] for k, v in t.items()})
            rec["list_over_padded"] = rec["list_ms"][0] / rec["padded_ms"][0]
            out.append(rec)
            print(f"{dtype} N={n}: rows {rec['rows']} ({rec['pad_rows']} pad), list {rec['list_ms'][0]:.2f} ms "
                  f"[{rec['list_ms'][1]:.2f}, {rec['list_ms'][2]:.2f}], padded {rec['padded_ms'][0]:.2f} ms "
                  f"[{rec['padded_ms'][1]:.2f}, {rec['padded_ms'][2]:.2f}], list / padded {rec['list_over_padded']:.3f}")
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(dict(bench="train_list", results=out)))


if __name__ == "__main__":
    main()
