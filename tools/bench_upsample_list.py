#!/usr/bin/env python
"""What the per-item conditioning loop costs in front of a list decode and what the ragged upsampler (WaeEngine.upsample_list) saves:
the upsampling network of hps/vqwae.json (Cc 64, ConvInUpsampleNetwork, scales [4, 4, 8, 5], cin_pad 0) on lists of unequal lengths.

usage: bench_upsample_list.py [--sizes 8,64,256,1024] [--dtypes bf16,fp32] [--repeats 5] [--min-frames 13] [--max-frames 100]
                              [--session-clips 256] [--chunk 160]
    --sizes          clips per list, one measurement each and per dtype
    --repeats        timed repeats per measurement (at least 5); the median is reported with the fastest and the slowest
    --session-clips  clips of the second pair (0: skip it)
Latent frame counts are drawn with numpy.random.default_rng(1234), uniform in [--min-frames, --max-frames] (one frame = 640 samples:
8 000 to 64 000 samples).  Two pairs, each in this one process, warmed, the two sides alternating repeat by repeat:
  device to device   the loop decode_list ran before the list form -- _ar_cond_rows (upsample_forward, B = 1) per item into the item's
                     rows of the packed c_up -- against one upsample_list into the same rows; latents on the device, c_up left there
  first chunks       N x sess.add + sess.step(chunk) against sess.add_list + sess.step(chunk) on the decoder of hps/vqwae.json
                     (bf16, one-CU slots): the time until the first chunk of every clip is on the host's side of the launch
Prints one line per measurement and one JSON line at the end.  The list's rows are compared with the loop's bit for bit first."""
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

# hps/vqwae.json: the conditioning network; the decoder is not run in the first pair and is kept small there
NET = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=64, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
# hps/vqwae.json: the decoder of the second pair
DEC = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153, upsample_scales=[4, 4, 8, 5], cin_pad=0)
HOP = 640


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def pair(a, b, repeats):
    """a, b alternating, one warm-up each -> {side: (median, min, max)} in seconds"""
    a(), b()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(timed(a))
        tb.append(timed(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in (("loop", ta), ("list", tb))}


def engine(cfg, dtype):
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(O.make_state_dict(dict(cfg), salt=7, with_encoder=False))
    eng.prepare_weights()
    return eng


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="8,64,256,1024")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-frames", type=int, default=13)
    ap.add_argument("--max-frames", type=int, default=100)
    ap.add_argument("--session-clips", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=160)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    record = dict(cfg="hps/vqwae.json conditioning: Cc 64, ConvInUpsampleNetwork, scales [4, 4, 8, 5], cin_pad 0", repeats=args.repeats,
                  lengths=f"uniform {args.min_frames}..{args.max_frames} latent frames of {HOP} samples, numpy default_rng(1234)", runs=[])
    print(record["cfg"] + "; " + record["lengths"], flush=True)
    for dtype in args.dtypes.split(","):
        eng = engine(NET, dtype)
        rng = np.random.default_rng(1234)
        gen = torch.Generator().manual_seed(1234)
        for n in [int(s) for s in args.sizes.split(",")]:
            Fs = [int(f) for f in rng.integers(args.min_frames, args.max_frames + 1, n)]
            dev = [torch.randn(NET["Cc"], f, generator=gen).cuda() for f in Fs]
            Ts = [f * HOP for f in Fs]
            offs = [int(o) for o in np.concatenate([[0], np.cumsum(Ts)[:-1]])]
            total = sum(Ts)
            out_loop = torch.zeros(total, eng.g.Ccp, dtype=eng.tdtype, device="cuda")
            out_list = torch.zeros(total, eng.g.Ccp, dtype=eng.tdtype, device="cuda")

            def loop():
                for c, o, T in zip(dev, offs, Ts):
                    eng._ar_cond_rows(c[None], out_loop[o:o + T].view(1, T, eng.g.Ccp), False)

            def lst():
                eng.upsample_list(dev, out=out_list, offsets=offs)

            loop(), lst()
            torch.cuda.synchronize()
            same = bool(torch.equal(out_loop.view(torch.int16 if out_loop.element_size() == 2 else torch.int32),
                                    out_list.view(torch.int16 if out_list.element_size() == 2 else torch.int32)))
            r = pair(loop, lst, args.repeats)
            lo, li = r["loop"], r["list"]
            bar = li[2] < lo[1]          # the slowest list repeat against the fastest loop repeat
            print(f"{dtype} {n:5d} clips, {total:9d} samples, device to device: loop {lo[0] * 1e3:9.2f} ms ({lo[1] * 1e3:.2f} .. {lo[2] * 1e3:.2f}), "
                  f"upsample_list {li[0] * 1e3:9.2f} ms ({li[1] * 1e3:.2f} .. {li[2] * 1e3:.2f}), loop / list {lo[0] / li[0]:6.2f}; "
                  f"per clip {lo[0] / n * 1e6:8.1f} us against {li[0] / n * 1e6:8.1f} us; slowest list < fastest loop: {bar}; "
                  f"bit for bit: {same}", flush=True)
            record["runs"].append(dict(kind="d2d", dtype=dtype, clips=n, samples=total, loop_ms=[t * 1e3 for t in lo],
                                       list_ms=[t * 1e3 for t in li], ratio=lo[0] / li[0], slowest_list_below_fastest_loop=bool(bar),
                                       same=same))
            del out_loop, out_list, dev
            torch.cuda.empty_cache()
        del eng
    if args.session_clips > 0:
        n = args.session_clips
        eng = engine(DEC, "bf16")
        rng = np.random.default_rng(4321)
        gen = torch.Generator().manual_seed(4321)
        Fs = [int(f) for f in rng.integers(args.min_frames, args.max_frames + 1, n)]
        items = [dict(T=f * HOP, c=torch.randn(DEC["Cc"], f, generator=gen).cuda(), gid=int(rng.integers(0, DEC["n_speakers"])),
                      uniforms=torch.rand(f * HOP, generator=gen).cuda()) for f in Fs]
        first = {}

        def run(join, key):
            def go():
                with eng.decode_session(mode="sample") as sess:
                    hs = join(sess)
                    res = sess.step(args.chunk)
                    first[key] = torch.cat([res[h]["idx"] for h in hs]).clone()
            return go

        a = run(lambda s: [s.add(it) for it in items], "loop")
        b = run(lambda s: s.add_list(items), "list")
        r = pair(a, b, args.repeats)
        same = bool(torch.equal(first["loop"], first["list"]))
        lo, li = r["loop"], r["list"]
        print(f"bf16 {n:5d} clips, first chunks of {args.chunk} steps: {n} x add + step {lo[0] * 1e3:9.2f} ms ({lo[1] * 1e3:.2f} .. "
              f"{lo[2] * 1e3:.2f}), add_list + step {li[0] * 1e3:9.2f} ms ({li[1] * 1e3:.2f} .. {li[2] * 1e3:.2f}), loop / list "
              f"{lo[0] / li[0]:6.2f}; slowest list < fastest loop: {li[2] < lo[1]}; bit for bit: {same}", flush=True)
        record["runs"].append(dict(kind="first_chunks", dtype="bf16", clips=n, chunk=args.chunk, loop_ms=[t * 1e3 for t in lo],
                                   list_ms=[t * 1e3 for t in li], ratio=lo[0] / li[0],
                                   slowest_list_below_fastest_loop=bool(li[2] < lo[1]), same=same))
    print(json.dumps(record))
    return 0 if all(r["same"] for r in record["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
