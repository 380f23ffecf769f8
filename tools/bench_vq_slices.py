#!/usr/bin/env python
"""What the fused multi-slice search costs against the loop it replaces (include/wae.h: wae_vq_search_slices / wae_vq_slice), and
what a whole feed_list round of a sliced quantiser costs against the plain one's.

usage: bench_vq_slices.py [--frames 16,256,4096,65536] [--repeats 5]
Two measurements, one process, one warm-up, the two sides alternating, medians of --repeats (at least 5), device to device:
  search      64 latent channels as 2 x 32 and 4 x 16 slices, 256 codes per slice, mode 0 (search + gather), one clip of N frames:
              ONE wae_vq_search_slices call (one memset, one search launch, one statistics launch) against n wae_vq_slice calls (a
              memset and two launches each) on the same latents and codebooks.  idx and quant are compared bit for bit.
  feed round  EncodeSession.feed_list for 64 open utterances x 4 new frames each (hps/vqwae.json's encoder, fp32): an engine with
              the `sliced` quantiser (2 slices) against one with the plain quantiser -- the whole round, encoder launches included.
Sizes where the fused call is not faster are marked.  Prints one line per measurement and one JSON line at the end."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import wae_oracle as O  # closed-form weights only  # noqa: E402
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd import _lib as L  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

CFG = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=64, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0,
           c_in=39, encoder_hid=256, K=256)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return [statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3]


def search(args, record):
    lib = L.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(1234)
    for n in (2, 4):
        D = 64 // n
        embs = [(torch.rand(256, D, generator=gen) - 0.5).cuda() for _ in range(n)]
        recs = (L.VqSliceRec * n)(*[L.VqSliceRec(e.data_ptr(), s * D, D, 256, 1.25 * D / 64) for s, e in enumerate(embs)])
        words = int(lib.wae_vq_search_slices_scratch(recs, n))
        for N in [int(s) for s in args.frames.split(",")]:
            lat = (torch.rand(1, 64, N, generator=gen) - 0.5).cuda()
            fi, li = (torch.empty(n, N, dtype=torch.int64, device="cuda") for _ in range(2))
            fq, lq = torch.empty_like(lat), torch.empty_like(lat)
            fs, ls = (torch.empty(n, 2, device="cuda") for _ in range(2))
            scratch = torch.empty(words, dtype=torch.int32, device="cuda")
            hists = [torch.empty(257, dtype=torch.int32, device="cuda") for _ in range(n)]

            def fused():
                L.check(lib.wae_vq_search_slices(L.ptr(lat), recs, n, L.ptr(fi), L.ptr(fq), L.ptr(fs), L.ptr(scratch), 1, 64, N, 0, st),
                        "vq_search_slices")

            def loop():
                for s, e in enumerate(embs):
                    L.check(lib.wae_vq_slice(L.ptr(lat), L.ptr(e), L.ptr(li[s]), L.ptr(lq), L.ptr(ls[s]), L.ptr(hists[s]), 1, 64, s * D, D,
                                             N, 256, 1.25 * D / 64, 0, st), "vq_slice")

            fused(), loop()      # the warm-up
            tf, tl = [], []
            for _ in range(args.repeats):
                tf.append(timed(fused))
                tl.append(timed(loop))
            same = bool(torch.equal(fi, li)) and bool(torch.equal(fq, lq)) and bool(torch.equal(fs[:, 1], ls[:, 1]))
            f, a = stats(tf), stats(tl)
            print(f"search {n} x {D:2d} channels, K 256, {N:6d} frames: fused {f[0]:8.3f} ms ({f[1]:.3f} .. {f[2]:.3f}), "
                  f"{n} per-slice calls {a[0]:8.3f} ms ({a[1]:.3f} .. {a[2]:.3f}), loop / fused {a[0] / f[0]:5.2f}; "
                  f"fused not faster: {f[0] >= a[0]}; bit for bit: {same}", flush=True)
            record["runs"].append(dict(kind="search", slices=n, D=D, K=256, frames=N, fused_ms=f, loop_ms=a, ratio=a[0] / f[0],
                                       fused_not_faster=bool(f[0] >= a[0]), same=same))


def feed_round(args, record):
    gen = torch.Generator().manual_seed(77)
    clips, K = 64, 4
    rounds = args.repeats + 1
    xs = [torch.randn(CFG["c_in"], 40 + rounds * K, generator=gen).cuda() for _ in range(clips)]
    sd = O.make_state_dict(dict(CFG), salt=7)
    engs = {}
    for kind in ("plain", "sliced"):
        eng = WaeEngine(Geometry.from_cfg(dict(CFG, vq=kind)), dtype="fp32")
        if kind == "sliced":
            cb = sd["vq.embedding.weight"]
            sd_k = {k: v for k, v in sd.items() if k != "vq.embedding.weight"}
            sd_k.update({"vq.embedding1.weight": cb[:, :32].contiguous(), "vq.embedding2.weight": cb[:, 32:].contiguous()})
        else:
            sd_k = sd
        eng.load_state_dict(sd_k)
        eng.prepare_weights()
        engs[kind] = eng
    with engs["plain"].encode_session() as sp, engs["sliced"].encode_session() as ss:
        hp, hs = [sp.open() for _ in xs], [ss.open() for _ in xs]
        sp.feed_list({h: x[:, :40] for h, x in zip(hp, xs)})
        ss.feed_list({h: x[:, :40] for h, x in zip(hs, xs)})
        tp, ts, same = [], [], True
        for r in range(rounds):       # round 0 warms both sides
            lo = 40 + r * K
            a, b = {}, {}
            t1 = timed(lambda: a.update(ss.feed_list({h: x[:, lo:lo + K] for h, x in zip(hs, xs)})))
            t2 = timed(lambda: b.update(sp.feed_list({h: x[:, lo:lo + K] for h, x in zip(hp, xs)})))
            if r:
                ts.append(t1)
                tp.append(t2)
            same = same and all(a[x_]["quant"].shape == b[y_]["quant"].shape == (64, 1) for x_, y_ in zip(hs, hp))
    s, p = stats(ts), stats(tp)
    print(f"feed_list round, {clips} utterances x {K} frames: sliced (2 x 32) {s[0]:.3f} ms ({s[1]:.3f} .. {s[2]:.3f}), plain {p[0]:.3f} ms "
          f"({p[1]:.3f} .. {p[2]:.3f}); sliced / plain {s[0] / p[0]:.2f}", flush=True)
    record["runs"].append(dict(kind="feed_round", clips=clips, frames_per_feed=K, sliced_ms=s, plain_ms=p, ratio=s[0] / p[0], same=same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", default="16,256,4096,65536")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    record = dict(cfg="search: 64 channels, K 256, mode 0, fp32; feed round: hps/vqwae.json encoder (c_in 39, encoder_hid 256, Cc 64)",
                  repeats=args.repeats, runs=[])
    search(args, record)
    feed_round(args, record)
    print(json.dumps(record))
    return 0 if all(r["same"] for r in record["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
