#!/usr/bin/env python
"""The host paths' library calls, as text: every call through eng.lib with its entry name and its scalar arguments (pointers as
null / ptr, the stream as s0, s1, ... in order of first use, descriptors by their scalar fields), for the train steps (plain, window,
ragged) and the list calls on golden model A's geometry (class ids) and S's (scalar input) at tiny shapes, then the dense steps again
under WAE_DETERMINISTIC=1 with a sha256 of the parameters.  Per scenario it prints the number of calls, a sha256 of their text and the
entries in order of first use with their counts; --full prints every call.  Two builds that print the same text make the same calls
with the same scalars in the same order.
usage: host_trace.py [--dtype bf16] [--full]   (T = 160 F: the dense batches are B = 2 at 8 and 4 feature frames, the lists 8, 12 and 20)"""
import argparse
import ctypes
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import wae_oracle as O  # noqa: E402  (the golden models' state dicts)
from wavenet_autoencoders_amd import Geometry  # noqa: E402
from wavenet_autoencoders_amd.engine import WaeEngine  # noqa: E402

A = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
         c_in=39, K=32, cin_pad=0)
MODELS = dict(A=(A, 1), S=(dict(A, G=64, O=30, scalar_input=True), 3))


class Trace:
    def __init__(self, lib):
        self.lib, self.streams, self.calls = lib, {}, []

    def show(self, a, last):
        if a is None or (isinstance(a, ctypes.c_void_p) and not a.value):
            return "null"
        if isinstance(a, ctypes.c_void_p):
            return f"s{self.streams.setdefault(a.value, len(self.streams))}" if last else "ptr"
        obj = getattr(a, "_obj", a)          # byref(descriptor): its scalar fields
        if isinstance(obj, ctypes.Structure):
            vals = [getattr(obj, f[0]) for f in obj._fields_]
            return "{" + ",".join(repr(v) for v in vals if isinstance(v, (int, float)) and not isinstance(v, bool)) + "}"
        return repr(a) if isinstance(a, (int, float, bytes)) else "ptr"

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("wae_"):
            return fn

        def call(*args):
            self.calls.append(" ".join([name] + [self.show(a, i == len(args) - 1) for i, a in enumerate(args)]))
            return fn(*args)
        return call


def run(name, dtype, det, full):
    cfg, salt = MODELS[name]
    os.environ["WAE_DETERMINISTIC"] = "1" if det else "0"
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(O.make_state_dict(cfg, salt))
    tr = eng.lib = Trace(eng.lib)
    gen = torch.Generator().manual_seed(3)
    xs = (lambda *s: torch.rand(*s, generator=gen) * 1.6 - 0.8) if cfg.get("scalar_input") else (lambda *s: torch.randint(0, cfg["O"], s, generator=gen))
    batch = lambda F: (xs(2, 160 * F).cuda(), torch.randn(2, 39, F, generator=gen).cuda(), torch.tensor([1, 3]).cuda())  # noqa: E731
    items = [dict(x=xs(160 * F), feats=torch.randn(39, F, generator=gen), gid=i) for i, F in enumerate((8, 12, 20))]
    b8, b4 = batch(8), batch(4)
    steps = [("train_step", lambda: eng.train_step(*b8, lr=1e-3))] * 3
    steps += [("accumulate", lambda: eng.accumulate(*b8)), ("accumulate", lambda: eng.accumulate(*b4)), ("apply_step", lambda: eng.apply_step(lr=1e-3)),
              ("train_step_accum", lambda: eng.train_step_accum([b8 + (None,), b4 + (None,)], lr=1e-3))]
    if not det:
        steps += [("train_step_list", lambda: eng.train_step_list(items, lr=1e-3))] * 2
        steps += [("encode_list_stats", lambda: eng.encode_list_stats([it["feats"] for it in items])),
                  ("upsample_list", lambda: eng.upsample_list([torch.randn(16, F, generator=gen) for F in (2, 3, 5)])),
                  ("forward_list", lambda: eng.forward_list(items)), ("score_list", lambda: eng.score_list(items))]
    for what, fn in steps:
        tr.calls = []
        fn()
        names = [c.split(" ", 1)[0] for c in tr.calls]
        print(f"== {name} {dtype} det={int(det)} {what}: {len(names)} calls, sha256 {hashlib.sha256(chr(10).join(tr.calls).encode()).hexdigest()[:16]}")
        print("\n".join(tr.calls) if full else "   " + " ".join(f"{n}x{names.count(n)}" for n in dict.fromkeys(names)))
    torch.cuda.synchronize()
    eng.check_errors()
    if det:
        print(f"== {name} {dtype} params sha256", hashlib.sha256(eng.params.cpu().numpy().tobytes()).hexdigest())


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--full", action="store_true", help="every call with its arguments, not the scenario's digest")
    args = ap.parse_args()
    for model in MODELS:
        for det in (False, True):
            run(model, args.dtype, det, args.full)
