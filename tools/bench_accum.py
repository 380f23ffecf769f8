#!/usr/bin/env python
"""What gradient accumulation (WaeEngine.accumulate / apply_step) costs and saves on one GPU, in one process, the contenders
alternating repeat by repeat after one warm-up each, medians of --repeats (at least 5) with the fastest and the slowest.

usage: bench_accum.py [--configs c2,c3] [--windows 2,4,8] [--repeats 5] [--ragged 32] [--min-frames 100] [--max-frames 1500]

Per sample: a window of M micro-batches plus apply_step against M plain train_step calls on the same batch (bench.py's c2: 8 x 8000,
c3: 8 x 5120 with the encoder, both bf16; learning rate 0, so every step starts from the same weights).  What a window leaves out per
micro-batch from the second on: weight norm, the forward's and the backward's weight packing with the clearing of the accumulators,
the gather pass, the weight-norm backward and clip + Adam + EMA.

Ragged: --ragged utterances of --min-frames .. --max-frames feature frames (160 samples each, rounded up to whole latent frames; drawn
with numpy.random.default_rng(1234) as tools/bench_forward_list.py draws them: a stand-in for the corpus) on the hps/vqwae.json
decoder: ONE zero-padded batch of all of them against length-sorted micro-batches of 8, each padded to its own longest clip, as one
window.  Rows computed and time.  A contender whose workspaces would not fit the device (about 50 KB per row of a 20-layer R = 256
train step, estimated on the host) is skipped and reported as such, never tried.
Prints one line per measurement and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the configurations and their synthetic inputs)
from oracle import wae_oracle as O  # closed-form weights only  # noqa: E402
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

RAGGED_CFG = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153, upsample_scales=[4, 4, 8, 5],
                  cin_pad=0)
HOP, PER_LATENT = 160, 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns, repeats):
    for f in fns.values():
        f()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def ms(t):
    return f"{t[0] * 1e3:9.3f} ms ({t[1] * 1e3:.3f} .. {t[2] * 1e3:.3f})"


def per_sample(name, windows, repeats, record):
    conf = bench.CONFIGS[name]
    sd = O.make_state_dict(dict(conf["cfg"]), salt=conf["salt"], with_encoder=conf["encoder"])
    eng = WaeEngine(Geometry.from_cfg(conf["cfg"]), dtype=conf["dtype"])
    eng.load_state_dict(sd, strict=False)
    eng.init_optimizer()
    x, c, g = bench.synth_inputs(0, "cuda:0", conf)
    B, T = x.shape
    for M in windows:
        def plain():
            for _ in range(M):
                eng.train_step(x, c, g, lr=0.0)

        def window():
            eng.train_step_accum([(x, c, g, None)] * M, lr=0.0)
        r = alternate(dict(plain=plain, window=window), repeats)
        n = M * B * T
        print(f"{name} {conf['dtype']} {B} x {T}, M = {M}: {M} train_step {ms(r['plain'])}, window + apply_step {ms(r['window'])}; "
              f"ns per sample {r['plain'][0] / n * 1e9:8.3f} -> {r['window'][0] / n * 1e9:8.3f}; window / plain "
              f"{r['window'][0] / r['plain'][0]:6.4f}", flush=True)
        record["runs"].append(dict(config=name, dtype=conf["dtype"], B=B, T=T, M=M, plain_ms=[t * 1e3 for t in r["plain"]],
                                   window_ms=[t * 1e3 for t in r["window"]], window_over_plain=r["window"][0] / r["plain"][0]))
    del eng
    torch.cuda.empty_cache()


def ragged(n, lo, hi, repeats, record):
    cfg = RAGGED_CFG
    rng = np.random.default_rng(1234)
    gen = torch.Generator().manual_seed(1234)
    Tqs = sorted(int(t) for t in -(-rng.integers(lo, hi + 1, n) // PER_LATENT))
    Ts = [t * PER_LATENT * HOP for t in Tqs]

    def batch(idx):
        Tm, Fm = max(Ts[i] for i in idx), max(Tqs[i] for i in idx)
        x = torch.zeros(len(idx), Tm, dtype=torch.int32)
        c = torch.zeros(len(idx), cfg["Cc"], Fm)
        for j, i in enumerate(idx):
            x[j, :Ts[i]] = torch.randint(0, cfg["O"], (Ts[i],), generator=gen, dtype=torch.int32)
            c[j, :, :Tqs[i]] = torch.randn(cfg["Cc"], Tqs[i], generator=gen)
        g = torch.randint(0, cfg["n_speakers"], (len(idx),), generator=gen)
        return x.cuda(), c.cuda(), g.cuda(), torch.tensor([Ts[i] for i in idx])
    groups = [list(range(a, min(a + 8, n))) for a in range(0, n, 8)]
    rows_valid, rows_padded, rows_micro = sum(Ts), n * max(Ts), sum(len(gr) * max(Ts[i] for i in gr) for gr in groups)
    per_row = 50 * 1024          # bytes of forward + backward workspace per row (docstring)
    free = torch.cuda.mem_get_info()[1] * 0.6
    # (the engine keeps a workspace per shape: the padded batch's and every micro-batch's are alive together)
    both = (rows_padded + rows_micro) * per_row < free
    fits = dict(padded=both, micro=both)
    sd = O.make_state_dict(dict(cfg), salt=7, with_encoder=False)
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="bf16")
    eng.load_state_dict(sd, strict=False)
    eng.init_optimizer()
    fns = {}
    if fits["padded"]:
        whole = batch(list(range(n)))
        fns["padded"] = lambda: eng.train_step(*whole[:3], lengths=whole[3], lr=0.0)
    if fits["micro"]:
        micro = [batch(gr) for gr in groups]
        fns["window"] = lambda: eng.train_step_accum(micro, lr=0.0)
    out = dict(utterances=n, frames=[lo, hi], rows_valid=rows_valid, rows_padded=rows_padded, rows_micro=rows_micro, fits=fits)
    line = (f"ragged {n} utterances of {lo}..{hi} frames: {rows_valid} valid rows; one padded batch {rows_padded} rows, "
            f"{len(groups)} length-sorted micro-batches {rows_micro} rows")
    if fns:
        r = alternate(fns, repeats)
        for k, t in r.items():
            line += f"; {k} {ms(t)}"
            out[k + "_ms"] = [v * 1e3 for v in t]
        if len(r) == 2:
            line += f"; window / padded {r['window'][0] / r['padded'][0]:6.4f} (rows {rows_micro / rows_padded:6.4f})"
    for k, ok in fits.items():
        if not ok:
            line += f"; {k}: not run, its workspaces would not fit the device"
    print(line, flush=True)
    record["runs"].append(out)
    del eng
    torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--windows", default="2,4,8")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ragged", type=int, default=32, help="utterances of the ragged case (0: skip it)")
    ap.add_argument("--min-frames", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=1500)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    record = dict(repeats=args.repeats, runs=[])
    for name in [s for s in args.configs.split(",") if s]:
        per_sample(name, [int(m) for m in args.windows.split(",") if m], args.repeats, record)
    if args.ragged > 0:
        ragged(args.ragged, args.min_frames, args.max_frames, args.repeats, record)
    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
