#!/usr/bin/env python
"""Throughput of list decoding (WaeEngine.decode_list): hps/vqwae.json's decoder on a work list of unequal lengths.

usage: bench_ar_list.py [--items N] [--dtypes bf16,fp32] [--slots cu[,2cu,N...]] [--teams N[,N...]] [--loop K] [--min-len 8000]
                        [--max-len 64000] [--scalar [--fast] [--stream N[,N...]]]
       bench_ar_list.py --session [--session-clips 256]
    --items N     clips in the list (default 512); lengths are drawn with numpy.random.default_rng(1234), uniform in
                  [--min-len, --max-len] samples, and rounded to whole latent frames (640 samples: the conditioning is upsampled per clip)
    --dtypes      storage types to run (default bf16,fp32)
    --slots       workgroups to launch, one run each: "cu" = the device's CU count (decode_list's default), "2cu" twice that, or a number
    --teams N     also decode the list on N cooperative teams (decode_list(coop=True, teams=N); 1..8), one run each; "--slots none"
                  skips the one-CU list
    --loop K      also decode the first K clips one after another with incremental_forward (what synthesis.py does without
                  --batch-decode, on whatever kernel WAE_AR_COOP selects) and print that aggregate rate; 0 (default) skips it
    --scalar      the scalar-input decoder of tools/bench_ar.py --scalar instead (the same decoder with an O = 30 mixture-of-logistics
                  head) through WaeEngine.decode_list_scalar, on both list forms; --loop then runs twice: on the one-CU kernel and on
                  the cooperative kernel (ar_path(scalar_coop=True), what synthesis.py --coop-scalar selects)
    --fast        with --scalar: the team runs on the constant-size scalar kernels (ar_path(scalar_coop=True, scalar_fast=True), what
                  synthesis.py --coop-scalar-fast selects) instead of the any-shape kernel
    --stream N    with --scalar and --teams: also decode the list as a team session (decode_list_stream(coop=True)) in rounds of N
                  steps, one run per N and team count, every round's samples copied to the host; prints the aggregate kHz, the mean
                  per-clip kHz (a clip's steps / the time until its last chunk is on the host) and whether every clip equals the
                  team list bit for bit
    --session     decode sessions (WaeEngine.decode_session) against the list decode of the same clips, in bf16, in one run: 8 clips of
                  16 000 steps on 8 teams in rounds of 160 and of 1600 steps against decode_list(coop=True); 16 such clips on 8 teams
                  in rounds of 1600 (two clips per team); --session-clips clips of --min-len .. --max-len steps on the one-CU slots in
                  rounds of 1600 against decode_list.  Every round's outputs are copied to the host, as a service would.  Per run: the
                  aggregate kHz, the mean per-clip kHz (a clip's steps / the time from the start until its last chunk is on the
                  host) and the time until every clip has its first chunk on the host.
Prints, per run, the wall time of the whole decode_list call (packing the operands, upsampling, the launch, synchronised) and the
aggregate kHz = sum of lengths / time, beside the efficiency the launch plan predicts (packing.ar_list_plan), and one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import wae_oracle as O  # closed-form weights only  # noqa: E402
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402
from wavenet_autoencoders_amd.packing import ar_list_plan  # noqa: E402

CFG = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153,
           upsample_scales=[4, 4, 8, 5], cin_pad=0)
HOP = 640


def session_bench(args):
    dtype = "bf16"
    eng = WaeEngine(Geometry.from_cfg(CFG), dtype=dtype)
    eng.load_state_dict(O.make_state_dict(dict(CFG), salt=7, with_encoder=False))
    gen = torch.Generator(device="cuda").manual_seed(1234)
    mk = lambda lens: [dict(T=T, c=torch.randn(64, T // HOP, device="cuda", generator=gen), gid=i % CFG["n_speakers"],  # noqa: E731
                            uniforms=torch.rand(T, device="cuda", generator=gen)) for i, T in enumerate(lens)]
    record = dict(session=True, dtype=dtype, runs=[])

    def run_list(items, **how):
        total = sum(it["T"] for it in items)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.decode_list(items, mode="sample", **how)
        host = [r["idx"].cpu() for r in out]
        dt = time.perf_counter() - t0
        print(f"  decode_list({how}): {dt:.3f} s -> {total / dt / 1e3:.1f} kHz aggregate; first audio of every clip after {dt * 1e3:.0f} ms "
              f"(the whole launch)", flush=True)
        record["runs"].append(dict(kind="decode_list", how=str(how), clips=len(items), samples=total, seconds=dt, khz=total / dt / 1e3))
        return host

    def run_session(items, chunk, ref=None, **how):
        total = sum(it["T"] for it in items)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first, done_at, parts = None, {}, [[] for _ in items]
        for k, rnd in enumerate(eng.decode_list_stream(items, chunk, mode="sample", **how)):
            for i, r in enumerate(rnd):
                if r is not None:
                    parts[i].append(r["idx"].cpu())
                    if r["done"]:
                        done_at[i] = None
            now = time.perf_counter() - t0
            first = now if first is None else first
            done_at = {i: (now if v is None else v) for i, v in done_at.items()}
        dt = time.perf_counter() - t0
        per = float(np.mean([items[i]["T"] / done_at[i] for i in range(len(items))])) / 1e3
        same = "" if ref is None else ("; bit for bit the list" if all(torch.equal(torch.cat(p), r) for p, r in zip(parts, ref))
                                       else "; DIFFERS from the list")
        print(f"  decode_session({how}) rounds of {chunk}: {k + 1} launches, {dt:.3f} s -> {total / dt / 1e3:.1f} kHz aggregate, "
              f"{per:.2f} kHz per clip (mean); every clip's first chunk on the host after {first * 1e3:.1f} ms{same}", flush=True)
        record["runs"].append(dict(kind="decode_session", how=str(how), chunk=chunk, clips=len(items), samples=total, launches=k + 1,
                                   seconds=dt, khz=total / dt / 1e3, khz_per_clip=per, first_chunk_ms=first * 1e3))

    warm = mk([HOP] * 8)
    eng.decode_list(warm, mode="sample", coop=True)
    eng.decode_list(warm, mode="sample")
    list(eng.decode_list_stream(warm, 160, mode="sample", coop=True))
    list(eng.decode_list_stream(warm, 160, mode="sample"))
    torch.cuda.synchronize()
    eight, sixteen = mk([16000] * 8), mk([16000] * 16)
    print("8 clips of 16000 steps on 8 teams")
    ref = run_list(eight, coop=True, teams=8)
    run_session(eight, 160, ref, coop=True, teams=8)
    run_session(eight, 1600, ref, coop=True, teams=8)
    print("16 clips of 16000 steps on 8 teams (two clips per team)")
    ref = run_list(sixteen, coop=True, teams=8)
    run_session(sixteen, 1600, ref, coop=True, teams=8)
    rng = np.random.default_rng(1234)
    lens = rng.integers(args.min_len, args.max_len + 1, args.session_clips)
    lens = (np.maximum(1, np.rint(lens / HOP)).astype(np.int64) * HOP).tolist()
    many = mk(lens)
    print(f"{len(lens)} clips of {min(lens)} .. {max(lens)} steps on the one-CU slots")
    ref = run_list(many)
    run_session(many, 1600, ref)
    print(json.dumps(record))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--slots", default="cu")
    ap.add_argument("--teams", default="")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--min-len", type=int, default=8000)
    ap.add_argument("--max-len", type=int, default=64000)
    ap.add_argument("--scalar", action="store_true")
    ap.add_argument("--fast", action="store_true")
    ap.add_argument("--stream", default="")
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--session-clips", type=int, default=256)
    args = ap.parse_args()
    if args.session:
        return session_bench(args)
    if (args.fast or args.stream) and not args.scalar:
        ap.error("--fast and --stream belong to --scalar (class-id sessions: --session)")
    cfg = dict(CFG, O=30, scalar_input=True, output_distribution="Logistic") if args.scalar else CFG
    rng = np.random.default_rng(1234)
    lens = rng.integers(args.min_len, args.max_len + 1, args.items)
    lens = (np.maximum(1, np.rint(lens / HOP)).astype(np.int64) * HOP).tolist()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slot_runs = [] if args.slots == "none" else [cus if s == "cu" else 2 * cus if s == "2cu" else int(s) for s in args.slots.split(",")]
    team_runs = [int(t) for t in args.teams.split(",") if t]
    gen = torch.Generator(device="cuda").manual_seed(1234)
    unit = lambda *shape: torch.rand(*shape, device="cuda", generator=gen) * (1 - 2e-5) + 1e-5  # noqa: E731
    draws = (lambda T: dict(u_mix=unit(T, 10), u_log=unit(T))) if args.scalar else (lambda T: dict(uniforms=torch.rand(T, device="cuda", generator=gen)))
    items = [dict(T=T, c=torch.randn(64, T // HOP, device="cuda", generator=gen), gid=i % CFG["n_speakers"], **draws(T))
             for i, T in enumerate(lens)]
    # one latent frame of an item: the warm-up lists
    short = lambda it: dict({k: (v[:HOP] if k in ("uniforms", "u_mix", "u_log") else v) for k, v in it.items()}, T=HOP,  # noqa: E731
                            c=it["c"][:, :1].contiguous())
    what = "decode_list_scalar" if args.scalar else "decode_list"
    total = sum(lens)
    print(f"list: {len(lens)} clips, {total} samples, lengths {min(lens)} .. {max(lens)} (mean {total / len(lens):.0f}); {cus} CUs")
    record = dict(items=len(lens), samples=total, cus=cus, scalar=args.scalar, runs=[])
    sd = O.make_state_dict(dict(cfg), salt=7, with_encoder=False)
    for dtype in args.dtypes.split(","):
        eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
        if args.scalar:
            eng.ar_path(scalar_coop=True, scalar_fast=args.fast)      # (decode_list_scalar(coop=False) stays on the one-CU slots)
        eng.load_state_dict(sd)
        decode = eng.decode_list_scalar if args.scalar else eng.decode_list
        # what tells a real roll-out from a constant: the classes of clip 0, or the spread of its samples
        alive = ((lambda out: f"sample std of clip 0 {float(out[0]['x'].std()):.3f}") if args.scalar
                 else (lambda out: f"{int(torch.unique(out[0]['idx']).numel())} distinct classes in clip 0"))
        # warm-up: the kernels' code objects and the packed weights, on a list short enough not to matter
        decode([short(it) for it in items[:cus]])
        torch.cuda.synchronize()
        for slots in slot_runs:
            plan = ar_list_plan(lens, slots)
            t0 = time.perf_counter()
            out = decode(items, mode="sample", slots=slots)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{what} {dtype} slots={plan.slots}: {dt:.2f} s -> {total / dt / 1e3:.1f} kHz aggregate; plan efficiency "
                  f"{plan.efficiency:.3f} (busiest slot {plan.makespan} samples -> {plan.makespan / dt / 1e3:.2f} kHz per slot); "
                  f"{alive(out)}", flush=True)
            record["runs"].append(dict(kind=what, dtype=dtype, slots=plan.slots, seconds=dt, khz=total / dt / 1e3,
                                       plan_efficiency=plan.efficiency, makespan=plan.makespan))
            del out
        if team_runs:
            decode([short(it) for it in items[:8]], coop=True)
            torch.cuda.synchronize()
        for teams in team_runs:
            plan = ar_list_plan(lens, max(1, min(teams, 8)))
            t0 = time.perf_counter()
            out = decode(items, mode="sample", coop=True, teams=teams)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"{what}(coop=True) {dtype} teams={plan.slots}: {dt:.2f} s -> {total / dt / 1e3:.1f} kHz aggregate; plan efficiency "
                  f"{plan.efficiency:.3f} (busiest team {plan.makespan} samples -> {plan.makespan / dt / 1e3:.2f} kHz per team); "
                  f"{alive(out)}", flush=True)
            record["runs"].append(dict(kind=what + "_coop", dtype=dtype, teams=plan.slots, seconds=dt, khz=total / dt / 1e3,
                                       plan_efficiency=plan.efficiency, makespan=plan.makespan, fast=args.fast))
            for chunk in [int(n) for n in args.stream.split(",") if n]:
                ref = [r["x"].cpu() for r in out]
                list(eng.decode_list_stream([short(it) for it in items[:8]], chunk, mode="sample", coop=True, teams=teams))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                parts, done_at, k = [[] for _ in items], {}, 0
                for k, rnd in enumerate(eng.decode_list_stream(items, chunk, mode="sample", coop=True, teams=teams)):
                    for i, r in enumerate(rnd):
                        if r is not None:
                            parts[i].append(r["x"].cpu())
                            if r["done"]:
                                done_at[i] = time.perf_counter() - t0
                dt = time.perf_counter() - t0
                per = float(np.mean([lens[i] / done_at[i] for i in range(len(items))])) / 1e3
                same = all(torch.equal(torch.cat(p), r) for p, r in zip(parts, ref))
                print(f"decode_list_stream(coop=True) {dtype} teams={plan.slots} rounds of {chunk}: {k + 1} launches, {dt:.2f} s -> "
                      f"{total / dt / 1e3:.1f} kHz aggregate, {per:.2f} kHz per clip (mean); bit for bit the team list: {same}", flush=True)
                record["runs"].append(dict(kind="team_session", dtype=dtype, teams=plan.slots, chunk=chunk, launches=k + 1, seconds=dt,
                                           khz=total / dt / 1e3, khz_per_clip=per, equal=same, fast=args.fast))
            del out
        for scalar_coop in ((False, True) if args.scalar else (False,)) if args.loop > 0 else ():
            eng.ar_path(scalar_coop=scalar_coop, scalar_fast=args.fast)      # (no effect on class-id decoders)
            sub = items[:args.loop]
            first = sub[0]
            eng.incremental_forward(first["c"][None, :, :1].contiguous(), torch.tensor([0], device="cuda"), HOP, mode="sample")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for it in sub:
                eng._ar_profile = None
                eng.incremental_forward(it["c"][None], torch.tensor([it["gid"]], device="cuda"), it["T"], mode="sample",
                                        **{k: it[k][None] for k in ("uniforms", "u_mix", "u_log") if k in it})
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = sum(it["T"] for it in sub)
            kern = "one CU per clip" if getattr(eng, "_ar_profile", None) is None else "cooperative, one clip at a time"
            print(f"incremental_forward loop {dtype} first {len(sub)} clips ({n} samples; {kern}): {dt:.2f} s -> {n / dt / 1e3:.1f} kHz",
                  flush=True)
            record["runs"].append(dict(kind="loop", dtype=dtype, clips=len(sub), samples=n, seconds=dt, khz=n / dt / 1e3, kernel=kern))
    print(json.dumps(record))


if __name__ == "__main__":
    main()
