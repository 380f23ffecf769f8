#!/usr/bin/env python
"""What scoring whole utterances of unequal lengths costs three ways: the teacher-forced decoder of hps/vqwae.json (20 layers, R = G =
S = 256, 256 classes, 64 conditioning channels through the [4, 4, 8, 5] upsampling network, speaker embedding) with the shifted
cross-entropy, on lists of utterances.

usage: bench_forward_list.py [--sizes 16,64,256] [--dtypes bf16,fp32] [--repeats 5] [--min-frames 100] [--max-frames 1500]
    --sizes     utterances per list, one measurement each
    --repeats   timed repeats per measurement (at least 5); the median is reported with the fastest and the slowest
Lengths: feature frames drawn with numpy.random.default_rng(1234), uniform in [--min-frames, --max-frames], 160 samples each, rounded up
to whole latent frames (4 feature frames, 640 samples): the ZeroSpeech length distribution is not available to this tool, so the
lengths are a stand-in, not the corpus (the stand-in of tools/bench_encode_list.py).
Per list size and dtype three contenders alternate in this one process, repeat by repeat, device to device (inputs on the device,
results left there), after one warm-up each:
  list     WaeEngine.decoder_forward_list (want_logits=False): one launch per layer and group, no pad rows
  loop     decoder_forward per utterance (B = 1), what a caller without the list form does for exact per-utterance scores
  padded   zero-padded batches of 8 in length-sorted order with `lengths` (the case kindest to padding: the reference's similar-length
           sampler arranges this), what vqwae_train.evaluate does for presets with max_time_steps null
decoder_forward caches a workspace per (B, T); the loop and the padded batches meet a new T per call, so the cache is dropped after
every call (otherwise it grows by gigabytes per call): that allocation is part of what those two cost.
Last, what the generic list kernel costs per valid row against the dense path (static-schedule kernels where they apply): decoder_forward
on a dense 8 x 5120 batch against decoder_forward_list on 8 items of 5120, same process, alternating.
Prints one line per measurement and one JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import wae_oracle as O  # closed-form weights only  # noqa: E402
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

CFG = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153, upsample_scales=[4, 4, 8, 5], cin_pad=0)
HOP, PER_LATENT = 160, 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(fns, repeats):
    """the contenders alternating repeat by repeat, one warm-up each -> {name: (median, min, max)} in seconds"""
    for f in fns.values():
        f()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            ts[k].append(timed(f))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def make_items(Tqs, gen):
    items = []
    for Tq in Tqs:
        T = int(Tq) * PER_LATENT * HOP
        items.append(dict(x=torch.randint(0, CFG["O"], (T,), generator=gen, dtype=torch.int32).cuda(),
                          c=torch.randn(CFG["Cc"], int(Tq), generator=gen).cuda(), gid=int(torch.randint(0, CFG["n_speakers"], (1,), generator=gen))))
    return items


def contenders(eng, items):
    order = sorted(range(len(items)), key=lambda i: items[i]["x"].numel())
    batches = []
    for lo in range(0, len(order), 8):
        its = [items[i] for i in order[lo:lo + 8]]
        Tm, Fm = max(it["x"].numel() for it in its), max(it["c"].shape[1] for it in its)
        x = torch.zeros(len(its), Tm, dtype=torch.int32, device="cuda")
        c = torch.zeros(len(its), CFG["Cc"], Fm, device="cuda")
        for j, it in enumerate(its):
            x[j, :it["x"].numel()] = it["x"]
            c[j, :, :it["c"].shape[1]] = it["c"]
        batches.append((x, c, torch.tensor([it["gid"] for it in its]).cuda(), torch.tensor([it["x"].numel() for it in its]).cuda()))
    singles = [(it["x"][None], it["c"][None], torch.tensor([it["gid"]]).cuda()) for it in items]

    def run_list():
        return eng.decoder_forward_list(items, want_logits=False)[1]

    def run_loop():
        tot = []
        for x, c, g in singles:
            tot.append(eng.decoder_forward(x, c, g, targets=x, want_logits=False)["nll"].sum())
            eng._ws.clear()
        return tot

    def run_padded():
        tot = []
        for x, c, g, ln in batches:
            tot.append(eng.decoder_forward(x, c, g, targets=x, lengths=ln, want_logits=False)["loss"].clone())
            eng._ws.clear()
        return tot

    return dict(list=run_list, loop=run_loop, padded=run_padded)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-frames", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--no-dense", action="store_true", help="skip the dense 8 x 5120 comparison")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    record = dict(cfg="hps/vqwae.json decoder: 20 layers, R = G = S = 256, O 256, Cc 64, scales [4, 4, 8, 5]", repeats=args.repeats,
                  lengths=f"uniform {args.min_frames}..{args.max_frames} frames x {HOP} samples, numpy default_rng(1234) (a stand-in for "
                          "ZeroSpeech)", runs=[])
    print(record["cfg"] + "; " + record["lengths"], flush=True)
    sd = O.make_state_dict(dict(CFG), salt=7, with_encoder=False)
    for dtype in args.dtypes.split(","):
        eng = WaeEngine(Geometry.from_cfg(CFG), dtype=dtype)
        eng.load_state_dict(sd)
        eng.prepare_weights()
        rng = np.random.default_rng(1234)
        gen = torch.Generator().manual_seed(1234)
        for n in [int(s) for s in args.sizes.split(",") if s]:
            Tqs = -(-rng.integers(args.min_frames, args.max_frames + 1, n) // PER_LATENT)
            items = make_items(Tqs, gen)
            rows = int(sum(it["x"].numel() for it in items))
            pad_rows = sum(8 * max(it["x"].numel() for it in grp) for grp in
                           [sorted(items, key=lambda it: it["x"].numel())[lo:lo + 8] for lo in range(0, n, 8)])
            fns = contenders(eng, items)
            # the three agree on what they score: the list's mean against the loop's sums
            ref = float(torch.stack(fns["loop"]()).double().sum()) / (rows - n)
            got = float(fns["list"]())
            r = alternate(fns, args.repeats)
            li, lo, pa = r["list"], r["loop"], r["padded"]
            print(f"{dtype} {n:4d} utterances, {rows:9d} rows (padded batches of 8: {pad_rows:9d}): list {li[0] * 1e3:9.2f} ms "
                  f"({li[1] * 1e3:.2f} .. {li[2] * 1e3:.2f}), loop {lo[0] * 1e3:9.2f} ms ({lo[1] * 1e3:.2f} .. {lo[2] * 1e3:.2f}), padded "
                  f"{pa[0] * 1e3:9.2f} ms ({pa[1] * 1e3:.2f} .. {pa[2] * 1e3:.2f}); loop / list {lo[0] / li[0]:5.2f}, padded / list "
                  f"{pa[0] / li[0]:5.2f}; loss {got:.6f} (loop {ref:.6f})", flush=True)
            record["runs"].append(dict(dtype=dtype, utterances=n, rows=rows, padded_rows=int(pad_rows), list_ms=[t * 1e3 for t in li],
                                       loop_ms=[t * 1e3 for t in lo], padded_ms=[t * 1e3 for t in pa], loop_over_list=lo[0] / li[0],
                                       padded_over_list=pa[0] / li[0], loss_list=got, loss_loop=ref))
            del items, fns
            eng.hold("forward_list")
            eng.hold("upsample_list")
            torch.cuda.empty_cache()
        if not args.no_dense:
            items = make_items([5120 // (PER_LATENT * HOP)] * 8, gen)
            x = torch.stack([it["x"] for it in items])
            c = torch.stack([it["c"] for it in items])
            g = torch.tensor([it["gid"] for it in items]).cuda()
            r = alternate(dict(dense=lambda: eng.decoder_forward(x, c, g, targets=x, want_logits=False)["loss"],
                               list=lambda: eng.decoder_forward_list(items, want_logits=False)[1]), args.repeats)
            de, li = r["dense"], r["list"]
            print(f"{dtype} dense 8 x 5120: decoder_forward {de[0] * 1e3:8.3f} ms ({de[1] * 1e3:.3f} .. {de[2] * 1e3:.3f}), list of 8 x 5120 "
                  f"{li[0] * 1e3:8.3f} ms ({li[1] * 1e3:.3f} .. {li[2] * 1e3:.3f}); list / dense {li[0] / de[0]:5.2f}", flush=True)
            record["runs"].append(dict(dtype=dtype, dense_8x5120_ms=[t * 1e3 for t in de], list_8x5120_ms=[t * 1e3 for t in li],
                                       list_over_dense=li[0] / de[0]))
        del eng
        torch.cuda.empty_cache()
    print(json.dumps(record))
    return 0


if __name__ == "__main__":
    sys.exit(main())
