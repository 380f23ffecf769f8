#!/usr/bin/env python
"""What feeding a decode session costs and what it buys (DecodeSession.open / feed / feed_list / end), on hps/vqwae.json's
conditioning network (Cc 64, ConvInUpsampleNetwork, scales [4, 4, 8, 5], cin_pad 0: one latent frame = 640 samples = 40 ms at 16 kHz).

usage: bench_session_feed.py [--sizes 8,64,256] [--repeats 5] [--min-frames 13] [--max-frames 100] [--clip-frames 50] [--chunk 160]
Two measurements, bf16, one process, warmed:
  first audio   one clip of --clip-frames latent frames on the decoder of hps/vqwae.json, one cooperative team.  ARRIVAL MODEL: the
                latent frames arrive in real time, frame k at k x 40 ms (frame 0 at t = 0).  Nothing sleeps: the compute parts are
                timed and the waiting is added from the model.  Fed clip: the second frame makes the first 435 rows final, so its
                first audio is on the host at 40 ms + [feed(frame 1) + step(chunk) + the copy to the host].  Added clip: add needs all
                frames, so at (frames - 1) x 40 ms + [add(clip) + step(chunk) + the copy to the host].  Both bracketed parts are
                measured (median of --repeats, fastest .. slowest).
  feed rounds   N open clips that already hold 13..100 frames each (numpy default_rng(1234)) get one frame each per round:
                feed_list (one conv_in launch, one ranges launch per stage, one table upload) against the naive alternative on the
                code path that existed before -- upsample_list over every clip's WHOLE prefix again.  Round by round alternating,
                the clips growing by a frame per round on both sides; the fed rows are compared bit for bit with the naive rows.
fp32 sessions, scalar-input decoders, feeds of more than one frame and clips on the one-CU slots: not measured.
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

NET = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=64, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
DEC = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153, upsample_scales=[4, 4, 8, 5], cin_pad=0)
HOP, FRAME_MS = 640, 40.0


def engine(cfg, dtype):
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(O.make_state_dict(dict(cfg), salt=7, with_encoder=False))
    eng.prepare_weights()
    return eng


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return [statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3]


def first_audio(args, record):
    eng = engine(DEC, "bf16")
    gen = torch.Generator().manual_seed(77)
    F = args.clip_frames
    c = torch.randn(DEC["Cc"], F, generator=gen).cuda()
    uni = torch.rand(F * HOP, generator=gen).cuda()
    fed, added, heard = [], [], {}

    def run_fed():
        with eng.decode_session(mode="sample", coop=True, teams=1) as sess:
            h = sess.open(dict(gid=3), max_T=F * HOP)
            sess.feed(h, c[:, :1], uniforms=uni[:HOP])

            def go():
                sess.feed(h, c[:, 1:2], uniforms=uni[HOP:2 * HOP])
                heard["fed"] = sess.step(args.chunk)[h]["idx"].cpu()
            return timed(go)

    def run_added():
        with eng.decode_session(mode="sample", coop=True, teams=1) as sess:
            def go():
                h = sess.add(dict(T=F * HOP, c=c, gid=3, uniforms=uni))
                heard["added"] = sess.step(args.chunk)[h]["idx"].cpu()
            return timed(go)

    run_fed(), run_added()
    for _ in range(args.repeats):
        fed.append(run_fed())
        added.append(run_added())
    same = bool(torch.equal(heard["fed"], heard["added"]))
    f, a = stats(fed), stats(added)
    print(f"bf16 first audio, 1 clip of {F} frames ({F * FRAME_MS / 1e3:.2f} s), one team, chunk {args.chunk}: "
          f"feed(frame 1) + step + copy {f[0]:.2f} ms ({f[1]:.2f} .. {f[2]:.2f}); add(clip) + step + copy {a[0]:.2f} ms ({a[1]:.2f} .. "
          f"{a[2]:.2f}); under the arrival model (frame k at k x 40 ms) first audio {FRAME_MS + f[0]:.1f} ms after the first frame when "
          f"fed against {(F - 1) * FRAME_MS + a[0]:.1f} ms when added; bit for bit: {same}", flush=True)
    record["runs"].append(dict(kind="first_audio", dtype="bf16", frames=F, chunk=args.chunk, feed_step_ms=f, add_step_ms=a,
                               modelled_fed_ms=FRAME_MS + f[0], modelled_added_ms=(F - 1) * FRAME_MS + a[0], same=same))


def feed_rounds(args, record):
    eng = engine(NET, "bf16")
    for n in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(1234)
        gen = torch.Generator().manual_seed(1234)
        rounds = args.repeats + 1
        Fs = [int(f) for f in rng.integers(args.min_frames, args.max_frames + 1, n)]
        cs = [torch.randn(NET["Cc"], f + rounds, generator=gen).cuda() for f in Fs]
        tf, tn = [], []
        with eng.decode_session(mode="argmax") as sess:
            sess.reserve(n)
            sess.reserve_frames(sum(Fs) + n * rounds)
            hs = [sess.open(dict(gid=0, init_idx=1), max_T=(f + rounds) * HOP) for f in Fs]
            sess.feed_list({h: c[:, :f] for h, c, f in zip(hs, cs, Fs)})
            for r in range(rounds):       # round 0 warms both sides
                have = [f + r for f in Fs]
                t1 = timed(lambda: sess.feed_list({h: c[:, k:k + 1] for h, c, k in zip(hs, cs, have)}))
                naive = {}
                t2 = timed(lambda: naive.update(out=eng.upsample_list([c[:, :k + 1] for c, k in zip(cs, have)])))
                if r:
                    tf.append(t1)
                    tn.append(t2)
            c_up, offs = naive["out"]
            same = True
            for h, o in zip(hs, offs):
                k = sess.clips[h].feed.ready
                a, b = sess.clips[h].c_up[:k], c_up[int(o):int(o) + k]
                same = same and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
        f, a = stats(tf), stats(tn)
        print(f"bf16 {n:4d} open clips holding {sum(Fs)} frames, one frame each per round: feed_list {f[0]:8.2f} ms ({f[1]:.2f} .. {f[2]:.2f}), "
              f"upsample_list over the whole prefixes {a[0]:8.2f} ms ({a[1]:.2f} .. {a[2]:.2f}), naive / feed {a[0] / f[0]:6.2f}; "
              f"feed slower than naive: {f[0] > a[0]}; final rows bit for bit: {same}", flush=True)
        record["runs"].append(dict(kind="feed_round", dtype="bf16", clips=n, frames_held=sum(Fs), feed_ms=f, naive_ms=a, ratio=a[0] / f[0],
                                   feed_slower=bool(f[0] > a[0]), same=same))
        torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="8,64,256")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-frames", type=int, default=13)
    ap.add_argument("--max-frames", type=int, default=100)
    ap.add_argument("--clip-frames", type=int, default=50)
    ap.add_argument("--chunk", type=int, default=160)
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    record = dict(cfg="hps/vqwae.json conditioning: Cc 64, ConvInUpsampleNetwork, scales [4, 4, 8, 5], cin_pad 0",
                  arrival_model="latent frame k arrives at k x 40 ms; nothing sleeps, waiting is added from the model", repeats=args.repeats,
                  runs=[])
    print(record["cfg"] + "; arrival model: " + record["arrival_model"], flush=True)
    first_audio(args, record)
    feed_rounds(args, record)
    print(json.dumps(record))
    return 0 if all(r["same"] for r in record["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
