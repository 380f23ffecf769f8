#!/usr/bin/env python
"""What feeding an encode session costs and what it buys (EncodeSession.open / feed_list / end), on the encoder and quantiser of
hps/vqwae.json (39 MFCC channels, encoder_hid 256, 64 latent channels, 256 codes; fp32; one feature frame = 10 ms, one latent = 40 ms).

usage: bench_encode_session.py [--sizes 1,8,64,256] [--feeds 1,4,16] [--repeats 5] [--min-frames 100] [--max-frames 1500]
                               [--clip-frames 200]
Two measurements, one process, warmed, the two sides alternating round by round, medians of --repeats (at least 5):
  feed rounds    N open utterances that already hold --min-frames..--max-frames feature frames each (numpy default_rng(1234), a
                 stand-in for a corpus) get K frames each per round: feed_list (one upload of the frames, one table upload, at most
                 eleven range launches, one quantiser call) against the only way there was before -- encode_list over every
                 utterance's WHOLE prefix again.  The utterances grow by K frames per round on both sides.  The session's new chunks
                 are compared bit for bit with the same columns of the prefix encoding (they are final, so the prefix has them right).
                 Inputs are on the device and outputs stay there.
  first latent   one utterance of --clip-frames feature frames.  ARRIVAL MODEL: feature frame k arrives at k x 10 ms (frame 0 at
                 t = 0).  Nothing sleeps: the compute parts are timed and the waiting is added from the model.  Session: latent
                 frame 0 needs 17 feature frames, so it is on the host at 160 ms + [feed(frame 16) + the copy to the host].  Whole
                 utterance: encode_list needs every frame, so at (frames - 1) x 10 ms + [encode_list + the copy to the host].  Both
                 bracketed parts are measured.
Frames that arrive from the host, 16-bit storage, sliced / EMA quantisers and a session that trims its intermediates: not measured.
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
from wavenet_autoencoders_amd import packing as P  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

# hps/vqwae.json: the encoder (dim_in 39, encoder_hid 256, cin_channels 64, K 256); the decoder is not run here and is kept small
CFG = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=64, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0,
           c_in=39, encoder_hid=256, K=256)
FRAME_MS = 10.0


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(v):
    return [statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3]


def feed_rounds(eng, args, record):
    for n in [int(s) for s in args.sizes.split(",")]:
        for K in [int(s) for s in args.feeds.split(",")]:
            rng = np.random.default_rng(1234)
            gen = torch.Generator().manual_seed(1234)
            rounds = args.repeats + 1
            Fs = [int(f) for f in rng.integers(args.min_frames, args.max_frames + 1, n)]
            xs = [torch.randn(CFG["c_in"], f + rounds * K, generator=gen).cuda() for f in Fs]
            tf, tn, same = [], [], True
            with eng.encode_session() as sess:
                sess.reserve_frames(sum(-(-(f + rounds * K) // 4) * 4 for f in Fs))
                hs = [sess.open(max_frames=f + rounds * K) for f in Fs]
                sess.feed_list({h: x[:, :f] for h, x, f in zip(hs, xs, Fs)})
                for r in range(rounds):       # round 0 warms both sides
                    have = [f + r * K for f in Fs]
                    got, naive = {}, {}
                    t1 = timed(lambda: got.update(sess.feed_list({h: x[:, k:k + K] for h, x, k in zip(hs, xs, have)})))
                    t2 = timed(lambda: naive.update(out=eng.encode_list([x[:, :k + K] for x, k in zip(xs, have)])))
                    if r:
                        tf.append(t1)
                        tn.append(t2)
                    for h, k, pre in zip(hs, have, naive["out"]):
                        lo, hi = P.enc_ready(k, False), P.enc_ready(k + K, False)
                        same = same and got[h]["final"] == hi and bool(torch.equal(got[h]["quant"], pre["quant"][:, lo:hi]))
                        same = same and bool(torch.equal(got[h]["idx"], pre["idx"][lo:hi]))
            f, a = stats(tf), stats(tn)
            print(f"fp32 {n:4d} open utterances holding {sum(Fs)} frames, {K:2d} frames each per round: feed_list {f[0]:8.2f} ms "
                  f"({f[1]:.2f} .. {f[2]:.2f}), encode_list over the whole prefixes {a[0]:8.2f} ms ({a[1]:.2f} .. {a[2]:.2f}), "
                  f"naive / feed {a[0] / f[0]:7.2f}; feed slower than naive: {f[0] > a[0]}; new latents bit for bit: {same}", flush=True)
            record["runs"].append(dict(kind="feed_round", dtype="fp32", clips=n, frames_per_feed=K, frames_held=sum(Fs), feed_ms=f,
                                       naive_ms=a, ratio=a[0] / f[0], feed_slower=bool(f[0] > a[0]), same=same))
            torch.cuda.empty_cache()


def window_rounds(eng, args, record):
    """--window W: a round of the windowed session (EncodeSession(window=W): rings, constant arenas) against the same round of the
    unwindowed one, alternating in one process, and the bytes of both sessions' arenas"""
    W = args.window
    for n in [int(s) for s in args.sizes.split(",")]:
        for K in [int(s) for s in args.feeds.split(",")]:
            rng = np.random.default_rng(1234)
            gen = torch.Generator().manual_seed(1234)
            rounds = args.repeats + 1
            Fs = [int(f) for f in rng.integers(args.min_frames, args.max_frames + 1, n)]
            xs = [torch.randn(CFG["c_in"], f + rounds * K, generator=gen).cuda() for f in Fs]
            tw, tf, same = [], [], True
            with eng.encode_session(window=W) as ring, eng.encode_session() as flat:
                if K > ring.max_feed:
                    print(f"fp32 {n:4d} utterances, {K} frames per round: beyond max_feed {ring.max_feed} of window {W}: not measured", flush=True)
                    continue
                ring.reserve_slots(n)
                flat.reserve_frames(sum(-(-(f + rounds * K) // 4) * 4 for f in Fs))
                hr, hf = [ring.open() for _ in Fs], [flat.open(max_frames=f + rounds * K) for f in Fs]
                flat.feed_list({h: x[:, :f] for h, x, f in zip(hf, xs, Fs)})
                for lo in range(0, max(Fs), ring.max_feed):      # the prefix, max_feed frames per call
                    ring.feed_list({h: x[:, lo:min(lo + ring.max_feed, f)] for h, x, f in zip(hr, xs, Fs) if lo < f})
                for r in range(rounds):       # round 0 warms both sides
                    have = [f + r * K for f in Fs]
                    a, b = {}, {}
                    t1 = timed(lambda: a.update(ring.feed_list({h: x[:, k:k + K] for h, x, k in zip(hr, xs, have)})))
                    t2 = timed(lambda: b.update(flat.feed_list({h: x[:, k:k + K] for h, x, k in zip(hf, xs, have)})))
                    if r:
                        tw.append(t1)
                        tf.append(t2)
                    for x_, y_ in zip(hr, hf):
                        same = same and bool(torch.equal(a[x_]["quant"], b[y_]["quant"])) and bool(torch.equal(a[x_]["idx"], b[y_]["idx"]))
                bytes_ring, bytes_flat = ring.arena_bytes, flat.arena_bytes
            w, f = stats(tw), stats(tf)
            print(f"fp32 {n:4d} open utterances holding {sum(Fs)} frames, {K:2d} frames each per round: window {W} {w[0]:8.2f} ms "
                  f"({w[1]:.2f} .. {w[2]:.2f}), no window {f[0]:8.2f} ms ({f[1]:.2f} .. {f[2]:.2f}); windowed slower than the unwindowed "
                  f"runs' slowest: {w[0] > f[2]}; arenas {bytes_ring} B against {bytes_flat} B; bit for bit: {same}", flush=True)
            record["runs"].append(dict(kind="window_round", dtype="fp32", clips=n, frames_per_feed=K, window=W, window_ms=w, flat_ms=f,
                                       slower=bool(w[0] > f[2]), arena_bytes=bytes_ring, flat_arena_bytes=bytes_flat, same=same))
            torch.cuda.empty_cache()


def first_latent(eng, args, record):
    gen = torch.Generator().manual_seed(77)
    F = args.clip_frames
    x = torch.randn(CFG["c_in"], F, generator=gen).cuda()
    heard = {}

    def run_fed():
        with eng.encode_session() as sess:
            h = sess.open(max_frames=F)
            for k in range(16):               # frames 0..15, one per call as they arrive: nothing is final yet
                assert sess.feed(h, x[:, k:k + 1])["final"] == 0

            def go():
                heard["fed"] = sess.feed(h, x[:, 16:17])["quant"].cpu()
            return timed(go)

    def run_whole():
        def go():
            heard["whole"] = eng.encode_list([x], want_idx=False)[0]["quant"].cpu()
        return timed(go)

    run_fed(), run_whole()
    fed, whole = [], []
    for _ in range(args.repeats):
        fed.append(run_fed())
        whole.append(run_whole())
    same = heard["fed"].shape[1] == 1 and bool(torch.equal(heard["fed"], heard["whole"][:, :1]))
    f, a = stats(fed), stats(whole)
    print(f"fp32 first quantised latent, 1 utterance of {F} frames ({F * FRAME_MS / 1e3:.2f} s): feed(frame 16) + copy {f[0]:.2f} ms "
          f"({f[1]:.2f} .. {f[2]:.2f}); encode_list(whole) + copy {a[0]:.2f} ms ({a[1]:.2f} .. {a[2]:.2f}); under the arrival model "
          f"(frame k at k x 10 ms) the first latent is on the host {16 * FRAME_MS + f[0]:.1f} ms after the first frame when fed "
          f"against {(F - 1) * FRAME_MS + a[0]:.1f} ms when encoded whole; bit for bit: {same}", flush=True)
    record["runs"].append(dict(kind="first_latent", dtype="fp32", frames=F, feed_ms=f, whole_ms=a, modelled_fed_ms=16 * FRAME_MS + f[0],
                               modelled_whole_ms=(F - 1) * FRAME_MS + a[0], same=same))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="1,8,64,256")
    ap.add_argument("--feeds", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-frames", type=int, default=100)
    ap.add_argument("--max-frames", type=int, default=1500)
    ap.add_argument("--clip-frames", type=int, default=200)
    ap.add_argument("--window", type=int, help="measure EncodeSession(window=W) against the unwindowed session instead")
    args = ap.parse_args(argv)
    if args.repeats < 5:
        ap.error("--repeats: at least 5")
    if args.clip_frames < 17:
        ap.error("--clip-frames: the first latent needs 17 frames")
    eng = WaeEngine(Geometry.from_cfg(CFG), dtype="fp32")
    eng.load_state_dict(O.make_state_dict(dict(CFG), salt=7))
    eng.prepare_weights()
    record = dict(cfg="hps/vqwae.json encoder: c_in 39, encoder_hid 256, Cc 64, K 256, fp32",
                  arrival_model="feature frame k arrives at k x 10 ms; nothing sleeps, waiting is added from the model",
                  lengths=f"uniform {args.min_frames}..{args.max_frames} frames, numpy default_rng(1234) (a stand-in for a corpus)",
                  repeats=args.repeats, runs=[])
    print(record["cfg"] + "; arrival model: " + record["arrival_model"], flush=True)
    if args.window is not None:
        window_rounds(eng, args, record)
    else:
        first_latent(eng, args, record)
        feed_rounds(eng, args, record)
    print(json.dumps(record))
    return 0 if all(r["same"] for r in record["runs"]) else 1


if __name__ == "__main__":
    sys.exit(main())
