#!/usr/bin/env python
"""Synthesis waveform from trained WaveNet autoencoder (entry point of the reference's synthesis.py:2-17).

usage: synthesis.py [options] <dump_root> <checkpoint> <dst_dir> <syn_list> <speaker2ind> <lan> <up_factor> <frame_rate> <start_ind>

options:
    --hparams=<parmas>       Hyper parameters [default: ].
    --preset=<json>          Path of preset parameters (json).
    --length=<T>             Accepted and, as in the reference (synthesis.py:327-329), overridden by frames * up_factor.
    --initial-value=<n>      Initial mu-law class id (default: mulaw_quantize(0) = 127).
    --dtype=<fp32|bf16>      Compute precision [default: fp32].
    --coop-scalar            Scalar-input models ("raw" / "mulaw"): decode on the cooperative kernel (up to 32 CUs per utterance)
                             instead of one CU.  No effect on class-id ("mulaw-quantize") models.
    --coop-scalar-fast       --coop-scalar on the constant-size scalar kernels where the model has the reference's decoder sizes
                             (WaeEngine.ar_path(scalar_fast=True); other sizes keep the any-shape kernel).  Implies --coop-scalar.
    --stream-chunk=<N>       Decode in resumable launches of N samples (WaeEngine.incremental_stream) and post-process every chunk as
                             it arrives; prints the wall time to the first chunk of audio.  The wav written is the same file.
    --seed=<n>               torch.manual_seed(n) before decoding: the same draws, hence the same wav, from run to run.
    --batch-decode           Read every pair of <syn_list> first and decode them all in one launch (WaeEngine.decode_list: one
                             utterance per CU, the next one as soon as a CU is free) instead of one after another.  The wavs
                             written are the same files (with --seed: byte for byte those of the loop on the one-CU kernel,
                             WAE_AR_COOP=0).  Scalar-input ("raw" / "mulaw") models go through WaeEngine.decode_list_scalar; with
                             --batch-coop their wavs are those of the loop run with --coop-scalar.  Not with --stream-chunk.
    --batch-stream=<N>       With --batch-decode: decode the list in rounds of N samples per clip (WaeEngine.decode_list_stream: one
                             launch per round, every clip keeps its own history between the launches) and post-process every chunk as
                             it arrives, as --stream-chunk does for one clip; prints the wall time until every clip has its first
                             chunk.  With or without --batch-coop; a scalar-input model streams on the one-CU slots, or with
                             --batch-coop and --coop-scalar[-fast] on cooperative teams.
                             The wavs written are the bytes of --batch-decode alone.
    --feed-frames=<K>        With --batch-decode --batch-stream: every clip joins the session open, without its conditioning, and gets
                             K latent frames in front of every round, as if the speech arrived while it is converted
                             (DecodeSession.open / feed_list / end); a round decodes the samples whose conditioning is final.  The
                             wavs written are the bytes of --batch-decode --batch-stream alone, also with --seed.
    --feed-features=<K>      With --batch-decode --batch-stream: every clip joins an encode session AND the decode session open and
                             gets K feature frames in front of every round (EncodeSession.open / feed_list); the latent frames that
                             call makes final go straight into DecodeSession.feed_list, and the clip ends in both sessions behind its
                             last frames -- the whole conversion fed incrementally.  The wavs written are the bytes of --batch-decode
                             --batch-stream alone, also with --seed.  Not with --feed-frames.
    --batch-window=<W>       With --feed-frames or --feed-features: the sessions run in constant memory, every clip in a ring of W
                             latent frames (DecodeSession(window=W); the encode session's window is 4 W feature frames plus what
                             its layers retain).  A clip gets no more frames per round than its ring has room for.  The wavs
                             written are the bytes of the same command without the flag.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from wavenet_autoencoders_amd.data import inv_mulaw, inv_mulaw_quantize  # noqa: E402
from wavenet_autoencoders_amd.hparams import hparams  # noqa: E402
from wavenet_autoencoders_amd.wavenet_vocoder.util import is_mulaw  # noqa: E402


def inv_preemphasis(x, coef=0.85):
    """audio.py inv_preemphasis: y[n] = x[n] + coef * y[n-1] (scipy.signal.lfilter([1], [1, -coef], x))."""
    from scipy import signal
    return signal.lfilter([1], [1, -coef], x)


def postprocess_indices(idx, quantize_channels, postprocess, global_gain_scale):
    """The tail of wavegen (synthesis.py:382-394): mu-law class ids -> inv_mulaw_quantize(., quantize_channels) ->
    getattr(audio, postprocess) (the presets name inv_preemphasis, coefficient 0.85, audio.py:64-65) -> / global_gain_scale."""
    return postprocess_wave(inv_mulaw_quantize(np.asarray(idx), quantize_channels), postprocess, global_gain_scale)


def postprocess_wave(y, postprocess, global_gain_scale):
    """The part of that tail every input type shares: getattr(audio, postprocess), then / global_gain_scale (synthesis.py:388-394)."""
    y = np.asarray(y, dtype=np.float64)
    if postprocess not in ("", None, "none"):
        if postprocess != "inv_preemphasis":
            raise NotImplementedError(f"postprocess={postprocess!r}: audio.py offers inv_preemphasis only")
        y = inv_preemphasis(y, 0.85)
    if global_gain_scale > 0:
        y = y / global_gain_scale
    return y.astype(np.float32)


class ChunkPostprocess:
    """postprocess_wave a chunk at a time: inv_preemphasis is a one-pole recursive filter, so a chunk continues from the filter state
    the previous chunk left (scipy.signal.lfilter's zi / zf); the gain is point-wise.  The chunks' outputs, concatenated, are the array
    postprocess_wave returns for the whole signal, bit for bit (the same float64 recurrence in the same order;
    tests/test_ar_stream_cpu.py)."""

    def __init__(self, postprocess, global_gain_scale, coef=0.85):
        if postprocess not in ("", None, "none", "inv_preemphasis"):
            raise NotImplementedError(f"postprocess={postprocess!r}: audio.py offers inv_preemphasis only")
        self.filter = postprocess == "inv_preemphasis"
        self.gain, self.coef = global_gain_scale, coef
        self.zi = np.zeros(1, dtype=np.float64)

    def __call__(self, y):
        y = np.asarray(y, dtype=np.float64)
        if self.filter:
            from scipy import signal
            y, self.zi = signal.lfilter([1], [1, -self.coef], y, zi=self.zi)
        if self.gain > 0:
            y = y / self.gain
        return y.astype(np.float32)


def decoded_wave(out):
    """A decode result of one utterance (WaeEngine.incremental_forward, or a chunk of incremental_stream) -> the float waveform before
    post-processing (synthesis.py:382-385): class ids through inv_mulaw_quantize; the samples of a scalar-input decoder as they are
    ("raw") or through inv_mulaw ("mulaw")."""
    if out.get("idx") is not None:
        return inv_mulaw_quantize(out["idx"][0].cpu().numpy(), hparams.quantize_channels)
    y = out["x"][0].cpu().numpy().astype(np.float64)
    return inv_mulaw(y, hparams.quantize_channels) if is_mulaw(hparams.input_type) else y


def wavegen(eng, length, c, g, initial_value=127, chunk=None, on_chunk=None):
    """wavegen (synthesis.py:295-396): c (Tc, D) features, g speaker id -> float waveform in [-1, 1].
    chunk: decode in resumable launches of that many samples (WaeEngine.incremental_stream) and post-process each chunk with the
    filter state carried over; on_chunk(t0, audio) is called with every chunk's float32 audio and its first sample's index as soon as
    it exists.  The waveform returned is the same array as without `chunk`, given the same random draws."""
    device = eng.device
    ct = torch.from_numpy(np.ascontiguousarray(c.T[None]).astype(np.float32)).to(device)      # (1, D, Tc)  :342
    gid = torch.tensor([g], dtype=torch.int64, device=device) if g is not None else None
    if eng.weights_dirty:
        eng.prepare_weights()
    lat = eng.encoder_forward(ct)
    quant, _, _ = eng.vq_forward(lat)
    # input_type "raw" / "mulaw": one draw of the model's output distribution per sample (logistic or Gaussian mixture,
    # wavenet.py:325-333); "mulaw-quantize": a categorical draw per sample, from the start class
    kw = dict(log_scale_min=hparams.log_scale_min) if eng.g.scalar_input else dict(init_idx=int(initial_value))
    if chunk is None:
        out = eng.incremental_forward(quant, gid, int(length), mode="sample", **kw)
        return postprocess_wave(decoded_wave(out), hparams.postprocess, hparams.global_gain_scale)
    post = ChunkPostprocess(hparams.postprocess, hparams.global_gain_scale)
    parts, t0 = [], 0
    for item in eng.incremental_stream(quant, gid, int(length), int(chunk), mode="sample", **kw):
        parts.append(post(decoded_wave(item)))
        if on_chunk is not None:
            on_chunk(t0, parts[-1])
        t0 += len(parts[-1])
    return np.concatenate(parts)


def read_features(args, src):
    """A source of <syn_list> -> (its path under the dump, file id, (Tc, D) features zero-padded to whole latent frames)
    (synthesis.py:475-486)."""
    if args.lan == "surprise":
        src = "test/" + src
    fid = src.split("_")[1]
    path = f"{args.dump_root}/{src}/mfcc.norm.npy"
    if not os.path.exists(path):
        raise FileNotFoundError(f"cant find con file in {path}")
    c = np.load(path)
    div = 100 // int(args.frame_rate)
    if c.shape[0] % div != 0:
        c = np.pad(c, [[0, div - c.shape[0] % div], [0, 0]], mode="constant", constant_values=0.0)
    return src, fid, c


def batch_decode(eng, args, pairs, sp2ind, out_dir):
    """--batch-decode: the loop of main() with its decodes gathered into one WaeEngine.decode_list call (decode_list_scalar for a
    scalar-input model: "raw" / "mulaw", whose loop under --batch-coop is the one run with --coop-scalar).  Per pair, in the list's
    order: the seed (if any) and the draws of all its samples -- the order in which the loop consumes the generator; the encoder and
    the quantizer, which draw nothing, run before that as one WaeEngine.encode_list over all pairs -- then one launch for all pairs,
    then the loop's post-processing and file names.  --batch-coop: that launch on cooperative teams (decode_list(coop=True), --batch-teams of them): the loop's bytes where the loop decodes on the cooperative path
    (WAE_AR_COOP=1, the default), as plain --batch-decode gives the loop's bytes under WAE_AR_COOP=0."""
    from scipy.io import wavfile
    device = eng.device
    if eng.weights_dirty:
        eng.prepare_weights()
    # every pair's features first, then ONE encoder + quantiser call for the whole list (WaeEngine.encode_list: per pair the bytes of
    # its own encoder_forward + vq_forward).  Neither draws random numbers, so the generator is consumed exactly as in the loop.
    read = []
    for src, tar in pairs:
        src, fid, c = read_features(args, src)
        if tar not in sp2ind:
            raise KeyError(f"cant find sp {tar} in sp2ind {args.speaker2ind}")
        read.append((tar, fid, c))
    feats = [np.ascontiguousarray(c.T).astype(np.float32) for _, _, c in read]
    # (--feed-features: the encoder runs inside the rounds, on the frames as they are fed)
    quants = [None] * len(read) if args.feed_features else [r["quant"] for r in eng.encode_list(feats, want_idx=False)]
    items, names = [], []
    for (tar, fid, c), quant in zip(read, quants):
        length = c.shape[0] * int(args.up_factor)
        if args.seed is not None:
            torch.manual_seed(args.seed)
        if eng.g.scalar_input:
            u_mix, draw = eng.scalar_draws(length)
            items.append(dict(c=None if quant is None else quant.contiguous(), gid=sp2ind[tar], T=length, u_mix=u_mix,
                              **{"z" if eng.g.output_distribution == "Normal" else "u_log": draw}))
        else:
            items.append(dict(c=None if quant is None else quant.contiguous(), gid=sp2ind[tar], T=length, init_idx=int(args.initial_value),
                              uniforms=torch.rand(1, length, device=device)))
        names.append(f"{out_dir}{tar}_{fid}.wav")
    how = dict(coop=True, teams=args.batch_teams) if args.batch_coop else {}
    if args.feed_features:
        return batch_feed_features(eng, args, items, feats, names, how)
    if args.feed_frames:
        return batch_feed(eng, args, items, names, how)
    if args.batch_stream:
        return batch_stream(eng, args, items, names, how)
    if eng.g.scalar_input:
        results = eng.decode_list_scalar(items, mode="sample", log_scale_min=hparams.log_scale_min, **how)
    else:
        results = eng.decode_list(items, mode="sample", **how)
    for out, res in zip(names, results):
        # decoded_wave takes a batch of one utterance
        y = postprocess_wave(decoded_wave({k: v[None] for k, v in res.items() if v is not None}), hparams.postprocess,
                             hparams.global_gain_scale)
        wavfile.write(out, hparams.sample_rate, y)
        print("Finished! Check out {} for generated audio samples.".format(out), flush=True)
    return 0


def batch_stream(eng, args, items, names, how):
    """--batch-decode --batch-stream=N: batch_decode's list in rounds of N samples (WaeEngine.decode_list_stream).  Every clip has its
    own ChunkPostprocess, so its chunks, concatenated, are the array batch_decode post-processes in one piece -- the same wav bytes."""
    import time
    from scipy.io import wavfile
    kw = dict(log_scale_min=hparams.log_scale_min) if eng.g.scalar_input else {}
    posts = [ChunkPostprocess(hparams.postprocess, hparams.global_gain_scale) for _ in items]
    parts = [[] for _ in items]
    t_start, first = time.perf_counter(), True
    for rnd in eng.decode_list_stream(items, int(args.batch_stream), mode="sample", **how, **kw):
        for i, res in enumerate(rnd):
            if res is not None:
                parts[i].append(posts[i](decoded_wave({k: v[None] for k, v in res.items() if k != "done" and v is not None})))
        if first:
            first = False
            print(f"first audio of all {len(items)} clips after {(time.perf_counter() - t_start) * 1e3:.1f} ms", flush=True)
    for out, p in zip(names, parts):
        wavfile.write(out, hparams.sample_rate, np.concatenate(p))
        print("Finished! Check out {} for generated audio samples.".format(out), flush=True)
    return 0


def batch_feed(eng, args, items, names, how):
    """--batch-decode --batch-stream=N --feed-frames=K: batch_stream's rounds with every clip OPEN -- it joins without its
    conditioning (DecodeSession.open) and gets K latent frames in front of every round (feed_list: one launch per upsampling stage for
    all clips), as if the speech arrived while it is converted; a clip ends with its last frame.  The draws batch_decode made go with
    the frames they belong to, so a clip decodes bit for bit as in batch_stream: the same wav bytes, also with --seed.
    --batch-window=W: the session holds every clip in a ring of W latent frames; a clip gets no more frames than it has room for
    (DecodeSession.room) and ends once its last rows fit -- other feeds, the same bytes."""
    import time
    from scipy.io import wavfile
    kw = dict(log_scale_min=hparams.log_scale_min) if eng.g.scalar_input else {}
    hop = int(np.prod(eng.g.upsample_scales))
    W = args.batch_window
    names_of = ("u_mix", "z" if eng.g.output_distribution == "Normal" else "u_log") if eng.g.scalar_input else ("uniforms",)
    posts = [ChunkPostprocess(hparams.postprocess, hparams.global_gain_scale) for _ in items]
    parts, fed = [[] for _ in items], [0] * len(items)
    t_start, first = time.perf_counter(), True
    with eng.decode_session(mode="sample", **how, **kw, **({} if W is None else {"window": W})) as sess:
        sess.reserve(len(items))
        sess.reserve_frames(len(items) * W if W else sum(int(it["c"].shape[-1]) for it in items))
        hs = [sess.open({k: it[k] for k in ("gid", "init_idx") if k in it}, max_T=it["T"]) for it in items]
        ends = []
        while sess.live:
            feeds, draws = {}, {k: {} for k in names_of}
            for i, (h, it) in enumerate(zip(hs, items)):
                F = int(it["c"].shape[-1])
                n = min(int(args.feed_frames), F - fed[i], sess.room(h) if W and fed[i] < F else F)
                if n > 0:
                    feeds[h] = it["c"][:, fed[i]:fed[i] + n]
                    for k in names_of:
                        if it.get(k) is not None:
                            draws[k][h] = it[k].reshape(it["T"], -1)[fed[i] * hop:(fed[i] + n) * hop]
                    fed[i] += n
                    if fed[i] == F:
                        ends.append((h, it["T"]))
            sess.feed_list(feeds, **{k: v for k, v in draws.items() if v})
            for h, T in ends:       # (a windowed clip ends once its last rows fit behind the rows it has decoded)
                if not W or T - sess.clips[h].pos <= W * hop:
                    sess.end(h)
            ends = [(h, T) for h, T in ends if not sess.clips[h].feed.ended]
            rnd = sess.step(int(args.batch_stream))
            for i, h in enumerate(hs):
                res = rnd.get(h)
                if res is not None:
                    parts[i].append(posts[i](decoded_wave({k: v[None] for k, v in res.items() if k in ("idx", "x") and v is not None})))
            if first and all(parts):
                first = False
                print(f"first audio of all {len(items)} clips after {(time.perf_counter() - t_start) * 1e3:.1f} ms", flush=True)
    for out, p in zip(names, parts):
        wavfile.write(out, hparams.sample_rate, np.concatenate(p))
        print("Finished! Check out {} for generated audio samples.".format(out), flush=True)
    return 0


def batch_feed_features(eng, args, items, feats, names, how):
    """--batch-decode --batch-stream=N --feed-features=K: batch_feed's rounds with the encoder inside them.  Every clip joins an encode
    session and the decode session open; a round feeds K feature frames per clip to the encode session (EncodeSession.feed_list: one
    launch per encoder layer for all clips), hands the quantised latents that call made final to DecodeSession.feed_list with the
    draws of their samples, and decodes; a clip ends in both sessions behind its last frames.  The latents are bit for bit
    encode_list's and the draws are batch_decode's, so the wavs are batch_stream's bytes, also with --seed.
    --batch-window=W: both sessions in constant memory -- the decode session with rings of W latent frames, the encode session with
    a window of 4 W feature frames plus what its layers retain.  Latent frames the decode session has no room for yet wait on the
    device for the next round; a clip ends once its last rows fit.  Other feeds, the same bytes."""
    import time
    import torch
    from scipy.io import wavfile
    from wavenet_autoencoders_amd import packing as PK
    kw = dict(log_scale_min=hparams.log_scale_min) if eng.g.scalar_input else {}
    hop = int(np.prod(eng.g.upsample_scales))
    W = args.batch_window
    enc_kw = {} if W is None else {"window": PK.ENC_ROOM * W + PK.enc_window_min() - PK.ENC_ROOM}
    names_of = ("u_mix", "z" if eng.g.output_distribution == "Normal" else "u_log") if eng.g.scalar_input else ("uniforms",)
    posts = [ChunkPostprocess(hparams.postprocess, hparams.global_gain_scale) for _ in items]
    parts, fed, got = [[] for _ in items], [0] * len(items), [0] * len(items)
    t_start, first = time.perf_counter(), True
    with eng.encode_session(**enc_kw) as enc, eng.decode_session(mode="sample", **how, **kw, **({} if W is None else {"window": W})) as sess:
        sess.reserve(len(items))
        sess.reserve_frames(len(items) * W if W else sum(it["T"] // hop for it in items))
        if W:
            enc.reserve_slots(len(feats))
        else:
            enc.reserve_frames(sum(-(-f.shape[1] // 4) * 4 for f in feats))
        hs = [sess.open({k: it[k] for k in ("gid", "init_idx") if k in it}, max_T=it["T"]) for it in items]
        es = [enc.open(max_frames=f.shape[1]) for f in feats]
        wait, ends = [None] * len(items), []        # windowed: latent frames the decode session has no room for yet
        while sess.live:
            feeds, last = {}, []
            for i, (e, f) in enumerate(zip(es, feats)):
                if fed[i] < f.shape[1]:
                    n = min(int(args.feed_features), f.shape[1] - fed[i], enc.max_feed if W else f.shape[1])
                    feeds[e] = f[:, fed[i]:fed[i] + n]
                    fed[i] += n
                    if fed[i] == f.shape[1]:
                        last.append(e)
            new = enc.feed_list(feeds, ended=last) if feeds else {}
            lat, draws = {}, {k: {} for k in names_of}
            for i, (h, e, it) in enumerate(zip(hs, es, items)):
                res = new.get(e)
                q = None if res is None or not res["quant"].shape[1] else res["quant"]
                if W and h in sess.clips and not sess.clips[h].feed.ended:
                    q = q if wait[i] is None else wait[i] if q is None else torch.cat([wait[i], q], dim=1)
                    n = 0 if q is None else min(int(q.shape[1]), sess.room(h))
                    wait[i] = None if q is None or n == q.shape[1] else q[:, n:]
                    q = None if not n else q[:, :n]
                n = 0 if q is None else int(q.shape[1])
                if n:
                    lat[h] = q
                    for k in names_of:
                        if it.get(k) is not None:
                            draws[k][h] = it[k].reshape(it["T"], -1)[got[i] * hop:(got[i] + n) * hop]
                    got[i] += n
                if res is not None and res["done"]:
                    ends.append((i, h, it["T"]))
            sess.feed_list(lat, **{k: v for k, v in draws.items() if v})
            for i, h, T in ends:    # (a windowed clip ends once all its frames are fed and its last rows fit)
                if not W or (wait[i] is None and T - sess.clips[h].pos <= W * hop):
                    sess.end(h)
            ends = [(i, h, T) for i, h, T in ends if not sess.clips[h].feed.ended]
            rnd = sess.step(int(args.batch_stream))
            for i, h in enumerate(hs):
                res = rnd.get(h)
                if res is not None:
                    parts[i].append(posts[i](decoded_wave({k: v[None] for k, v in res.items() if k in ("idx", "x") and v is not None})))
            if first and all(parts):
                first = False
                print(f"first audio of all {len(items)} clips after {(time.perf_counter() - t_start) * 1e3:.1f} ms", flush=True)
    for out, p in zip(names, parts):
        wavfile.write(out, hparams.sample_rate, np.concatenate(p))
        print("Finished! Check out {} for generated audio samples.".format(out), flush=True)
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for a in ("dump_root", "checkpoint", "dst_dir", "syn_list", "speaker2ind", "lan", "up_factor", "frame_rate", "start_ind"):
        ap.add_argument(a)
    ap.add_argument("--hparams", default="")
    ap.add_argument("--preset")
    ap.add_argument("--length", type=int)
    ap.add_argument("--initial-value", type=int, default=127)
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--coop-scalar", action="store_true")
    ap.add_argument("--coop-scalar-fast", action="store_true")
    ap.add_argument("--stream-chunk", type=int)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--batch-decode", action="store_true")
    ap.add_argument("--batch-coop", action="store_true")
    ap.add_argument("--batch-teams", type=int)
    ap.add_argument("--batch-stream", type=int)
    ap.add_argument("--feed-frames", type=int)
    ap.add_argument("--feed-features", type=int)
    ap.add_argument("--batch-window", type=int)
    args = ap.parse_args(argv)
    args.coop_scalar = args.coop_scalar or args.coop_scalar_fast
    if args.batch_stream is not None and not args.batch_decode:
        ap.error("--batch-stream sets the round length of --batch-decode: it needs --batch-decode")
    if args.batch_stream is not None and args.batch_stream < 1:
        ap.error("--batch-stream: a round has at least one sample")
    if args.feed_frames is not None and (args.batch_stream is None or args.feed_frames < 1):
        ap.error("--feed-frames feeds that many latent frames (>= 1) per round of --batch-decode --batch-stream: it needs both")
    if args.feed_features is not None and (args.batch_stream is None or args.feed_features < 1):
        ap.error("--feed-features feeds that many feature frames (>= 1) per round of --batch-decode --batch-stream: it needs both")
    if args.batch_window is not None and (args.batch_window < 1 or (args.feed_frames is None and args.feed_features is None)):
        ap.error("--batch-window holds the fed clips in rings of that many latent frames (>= 1): it needs --feed-frames or --feed-features")
    if args.feed_features is not None and args.feed_frames is not None:
        ap.error("--feed-features feeds the encoder, --feed-frames the decoder: they cannot be combined")
    if (args.batch_coop or args.batch_teams is not None) and not args.batch_decode:
        ap.error("--batch-coop / --batch-teams choose how --batch-decode runs its list: they need --batch-decode")
    if args.batch_coop and args.stream_chunk:
        ap.error("--batch-coop decodes the whole list in one launch: it cannot be combined with --stream-chunk")
    if args.batch_teams is not None and not args.batch_coop:
        ap.error("--batch-teams sets the teams of --batch-coop")
    if args.batch_decode and args.stream_chunk:
        ap.error("--batch-decode decodes the whole list in one launch: it cannot be combined with --stream-chunk")
    if args.preset:
        with open(args.preset) as f:
            hparams.parse_json(f.read())
    hparams.parse(args.hparams)
    from vqwae_train import build_geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(build_geometry(hparams), dtype=args.dtype)
    ck = torch.load(args.checkpoint, map_location="cpu")
    eng.load_state_dict(ck["state_dict"])
    if args.coop_scalar:
        eng.ar_path(scalar_coop=True, scalar_fast=args.coop_scalar_fast)
    with open(args.speaker2ind) as f:
        sp2ind = json.load(f)
    os.makedirs(args.dst_dir, exist_ok=True)
    up = int(args.up_factor)
    with open(args.syn_list) as f:
        pairs = [ln.split() for ln in f if ln.strip()][int(args.start_ind):]
    from scipy.io import wavfile
    out_dir = f"{args.dst_dir}2019/{args.lan}/test/"                                          # synthesis.py:521-522 (string concat)
    os.makedirs(out_dir, exist_ok=True)
    if args.batch_decode:
        return batch_decode(eng, args, pairs, sp2ind, out_dir)
    for src, tar in pairs:
        src, fid, c = read_features(args, src)
        if tar not in sp2ind:
            raise KeyError(f"cant find sp {tar} in sp2ind {args.speaker2ind}")
        length = c.shape[0] * up                                                              # overrides --length (:327-329)
        if args.seed is not None:
            torch.manual_seed(args.seed)
        if args.stream_chunk:
            import time
            t_start, first = time.perf_counter(), []

            def on_chunk(t0, audio):
                if not first:
                    first.append(time.perf_counter() - t_start)
                    print(f"first audio: {len(audio)} samples after {first[0] * 1e3:.1f} ms ({src} -> {tar})", flush=True)
            y = wavegen(eng, length, c, sp2ind[tar], args.initial_value, chunk=args.stream_chunk, on_chunk=on_chunk)
        else:
            y = wavegen(eng, length, c, sp2ind[tar], args.initial_value)
        out = f"{out_dir}{tar}_{fid}.wav"
        wavfile.write(out, hparams.sample_rate, y)
        print("Finished! Check out {} for generated audio samples.".format(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
