#!/usr/bin/env python
"""AR synthesis speed (BASELINE config C4): hps/vqwae.json decoder, B utterances, T samples.

usage: bench_ar.py [dtype] [B] [T] [--generic] [--scalar]
    --generic   the class-id decode on the any-shape cooperative kernel (WaeEngine.ar_path(generic=True))
    --scalar    scalar-input decoders instead: the same decoder with a scalar head (O = 30 mixture of logistics, O = 2 "Normal"), the
                one-CU path (the default routing) against the cooperative path (ar_path(scalar_coop=True)) on the same draws, the two
                alternating, best of three decodes each"""
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
flags = [a for a in sys.argv[1:] if a.startswith("--")]
pos = [a for a in sys.argv[1:] if not a.startswith("--")]
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
        for path in ("one-CU", "cooperative"):
            engs[path] = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype).ar_path(scalar_coop=path == "cooperative")
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
                assert (e._ar_profile is not None) == (path == "cooperative"), f"{path}: the other path ran"
                if rep > 0:
                    best[path] = min(best.get(path, dt), dt)
                xs[path] = out["x"]
        agree = float((xs["one-CU"] - xs["cooperative"]).abs().lt(1e-2).float().mean())
        for path, dt in best.items():
            print(f"AR scalar {dist} O={O_ch} {dtype} B={B} T={T} {path:11s}: {dt:.3f} s -> {T / dt / 1e3:.2f} kHz per utterance, "
                  f"{dt / T * 1e6:.1f} us/sample")
        print(f"  cooperative / one-CU = {best['one-CU'] / best['cooperative']:.2f}x; samples within 1e-2 of each other: {agree:.3f} "
              f"(free-running decodes part where a mixture pick ties)")


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
