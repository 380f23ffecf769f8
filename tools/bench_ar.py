#!/usr/bin/env python
"""AR synthesis speed (BASELINE config C4): hps/vqwae.json decoder, B utterances, T samples.

usage: bench_ar.py [dtype] [B] [T] [--generic] [--scalar [--fast]] [--chunk N[,N...]]
    --generic   the class-id decode on the any-shape cooperative kernel (WaeEngine.ar_path(generic=True))
    --scalar    scalar-input decoders instead: the same decoder with a scalar head (O = 30 mixture of logistics, O = 2 "Normal"), the
                one-CU path (the default routing) against the cooperative path (ar_path(scalar_coop=True)) on the same draws, the two
                alternating, best of three decodes each
    --fast      with --scalar: three paths on the same clips in one process, alternating -- one-CU, the any-shape cooperative kernel
                and the constant-size cooperative kernels (ar_path(scalar_coop=True, scalar_fast=True)) -- and behind them the class-id
                constant-size decode of the same decoder, by the same procedure (one warm-up, best of three)
    --chunk N[,N...]  streaming (WaeEngine.incremental_stream): the one-shot decode against the same decode in launches of N steps, for
                every N listed, in one process -- kHz per utterance (best of three decodes each, after a warm-up) and the wall time from
                opening the stream to the first chunk's samples on the host.  Without a dtype argument both bf16 and fp32 run; T defaults
                to 16000 (one second at hps/vqwae.json's rate)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import wae_oracle as O  # closed-form weights only
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

CFG = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153,
           upsample_scales=[4, 4, 8, 5], cin_pad=0)
argv = sys.argv[1:]
chunk_sizes = None
if "--chunk" in argv:
    i = argv.index("--chunk")
    chunk_sizes = [int(n) for n in argv[i + 1].split(",")]
    del argv[i:i + 2]
flags = [a for a in argv if a.startswith("--")]
pos = [a for a in argv if not a.startswith("--")]
dtype = pos[0] if len(pos) > 0 else "bf16"
B = int(pos[1]) if len(pos) > 1 else 1
T = int(pos[2]) if len(pos) > 2 else 6400


def bench_scalar():
    lat = torch.randn(B, 64, T // 640, device="cuda")
    gid = torch.zeros(B, dtype=torch.int64, device="cuda")
    for dist, O_ch in (("Logistic", 30), ("Normal", 2)):
        cfg = dict(CFG, O=O_ch, scalar_input=True, output_distribution=dist)
        sd = O.make_state_dict(dict(cfg), salt=7, with_encoder=False)
        engs = {}
        for path in ("one-CU", "cooperative") + (("constant-size",) if "--fast" in flags else ()):
            engs[path] = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype).ar_path(scalar_coop=path != "one-CU",
                                                                                  scalar_fast=path == "constant-size")
            engs[path].load_state_dict(sd)
        M = 1 if O_ch == 2 else O_ch // 3
        gen = torch.Generator(device="cuda").manual_seed(11)
        u_mix = torch.rand(B, T, M, device="cuda", generator=gen) * (1 - 2e-5) + 1e-5
        kw = (dict(u_mix=u_mix, u_log=torch.rand(B, T, device="cuda", generator=gen) * (1 - 2e-5) + 1e-5) if dist == "Logistic"
              else dict(z=torch.randn(B, T, device="cuda", generator=gen)))
        best, xs = {}, {}
        for rep in range(4):                       # (the first pass warms both paths up)
            for path, e in engs.items():
                e._ar_profile = None
                t0 = time.perf_counter()
                out = e.incremental_forward(lat, gid, T, mode="sample", **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                assert (e._ar_profile is not None) == (path != "one-CU"), f"{path}: the other path ran"
                if rep > 0:
                    best[path] = min(best.get(path, dt), dt)
                xs[path] = out["x"]
        agree = float((xs["one-CU"] - xs["cooperative"]).abs().lt(1e-2).float().mean())
        for path, dt in best.items():
            print(f"AR scalar {dist} O={O_ch} {dtype} B={B} T={T} {path:11s}: {dt:.3f} s -> {T / dt / 1e3:.2f} kHz per utterance, "
                  f"{dt / T * 1e6:.1f} us/sample")
        print(f"  cooperative / one-CU = {best['one-CU'] / best['cooperative']:.2f}x; samples within 1e-2 of each other: {agree:.3f} "
              f"(free-running decodes part where a mixture pick ties)")
        if "constant-size" in best:
            print(f"  constant-size / any-shape cooperative = {best['cooperative'] / best['constant-size']:.2f}x "
                  f"({T / best['constant-size'] / 1e3:.2f} against {T / best['cooperative'] / 1e3:.2f} kHz per utterance)")
    if "--fast" in flags:      # the class-id decode of the same decoder on its constant-size kernels, in the same process
        eng = WaeEngine(Geometry.from_cfg(CFG), dtype=dtype)
        eng.load_state_dict(O.make_state_dict(dict(CFG), salt=7, with_encoder=False))
        uni = torch.rand(B, T, device="cuda")
        best = None
        for rep in range(4):
            t0 = time.perf_counter()
            eng.incremental_forward(lat, gid, T, mode="sample", uniforms=uni)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep > 0:
                best = dt if best is None else min(best, dt)
        print(f"AR class ids O=256 {dtype} B={B} T={T} constant-size: {best:.3f} s -> {T / best / 1e3:.2f} kHz per utterance, "
              f"{best / T * 1e6:.1f} us/sample")


def bench_stream():
    Ts = int(pos[2]) if len(pos) > 2 else 16000
    for dt_name in ([pos[0]] if pos else ["bf16", "fp32"]):
        eng = WaeEngine(Geometry.from_cfg(CFG), dtype=dt_name).ar_path(generic="--generic" in flags)
        eng.load_state_dict(O.make_state_dict(dict(CFG), salt=7, with_encoder=False))
        lat = torch.randn(B, 64, Ts // 640, device="cuda")
        gid = torch.zeros(B, dtype=torch.int64, device="cuda")
        uni = torch.rand(B, Ts, device="cuda")

        def one_shot():
            return eng.incremental_forward(lat, gid, Ts, mode="sample", uniforms=uni)["idx"]

        def streamed(n):
            first, parts = None, []
            t_open = time.perf_counter()
            for item in eng.incremental_stream(lat, gid, Ts, n, mode="sample", uniforms=uni):
                if first is None:
                    item["idx"].cpu()                       # the first chunk's samples on the host: what a player waits for
                    first = time.perf_counter() - t_open
                parts.append(item["idx"])
            return torch.cat(parts, dim=1), first

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            best, res = None, None
            for _ in range(3):
                t0 = time.perf_counter()
                res = fn()
                torch.cuda.synchronize()
                d = time.perf_counter() - t0
                best = d if best is None else min(best, d)
            return best, res
        d1, ref = timed(one_shot)
        print(f"AR stream {dt_name} B={B} T={Ts} one-shot          : {d1:.3f} s -> {Ts / d1 / 1e3:6.2f} kHz per utterance")
        for n in chunk_sizes:
            dn, (idx, first) = timed(lambda: streamed(n))
            same = bool(torch.equal(idx, ref))
            print(f"AR stream {dt_name} B={B} T={Ts} chunk {n:6d} ({-(-Ts // n):4d} launches): {dn:.3f} s -> {Ts / dn / 1e3:6.2f} kHz per utterance, "
                  f"{dn / d1:.3f}x the one-shot time, first chunk after {first * 1e3:.1f} ms, bitwise equal to the one-shot decode: {same}")
            assert same, f"chunk {n}: the streamed decode differs from the one-shot decode"


if chunk_sizes is not None:
    bench_stream()
    sys.exit(0)
if "--scalar" in flags:
    bench_scalar()
    sys.exit(0)
eng = WaeEngine(Geometry.from_cfg(CFG), dtype=dtype).ar_path(generic="--generic" in flags)
eng.load_state_dict(O.make_state_dict(dict(CFG), salt=7, with_encoder=False))
lat = torch.randn(B, 64, T // 640, device="cuda")
gid = torch.zeros(B, dtype=torch.int64, device="cuda")
for _ in range(2):
    eng.incremental_forward(lat, gid, T, mode="sample")
torch.cuda.synchronize()
t0 = time.perf_counter()
out = eng.incremental_forward(lat, gid, T, mode="sample")
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"AR {dtype} B={B} T={T}{' (any-shape cooperative kernel)' if '--generic' in flags else ''}: {dt:.3f} s -> {T / dt / 1e3:.2f} kHz per utterance, {B * T / dt / 1e3:.1f} kHz aggregate, "
      f"{dt / T * 1e6:.1f} us/sample")
prof = getattr(eng, "_ar_profile", None)
if prof is not None:
    f = int(prof[1])
    print("  XCC ids of the members:", prof[20:52].tolist())
    print(f"  cooperative path: same-XCD exchange = {f & 1}, XCC id of member 0 / last member = {(f >> 4) & 15} / {(f >> 8) & 15}")
if prof is not None and int(prof[2:].abs().sum()) != 0:
    import numpy as np
    pc = prof.cpu().numpy()[2:30].view(np.uint64)
    names = ["barrier after the GEMV", "gate + x' and skip shares", "-", "residual, next taps + barrier", "skip exchange", "head", "draw",
             "gate rows GEMV", "fused: x round-2 poll", "fused: vbuf writes + barrier", "exchange: stores + requests (weights, scalars, history)", "exchange: polling passes + sum"]
    print("  s_memtime ticks per sample (member 0):", {n: int(v // T) for n, v in zip(names, pc)})
