#!/usr/bin/env python
"""A/B of wae_enc_conv_fwd_list between two builds of the library: the same launches on the same operands, alternating in one
process, 20 launches per timing, medians of 9 (fastest .. slowest); the outputs are compared bit for bit.

usage: ab_enc_list.py <other libwae_hip.so>
    the other build, e.g. the parent commit's (build it in a second checkout); this tree's library is the one _lib loads.
Cases: 256 channels, the blocks the list entry has, lists of short clips (tiles of 8 and 16 outputs) and of long ones (32)."""
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wavenet_autoencoders_amd import _lib as L  # noqa: E402
from wavenet_autoencoders_amd import packing as PK  # noqa: E402

new = L.lib()
if len(sys.argv) != 2:
    sys.exit(__doc__)
old = ctypes.CDLL(os.path.abspath(sys.argv[1]))
res, args = L.SIGNATURES["wae_enc_conv_fwd_list"]
old.wae_enc_conv_fwd_list.restype, old.wae_enc_conv_fwd_list.argtypes = res, args


def timed(fn, n=20):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


gen = torch.Generator().manual_seed(1)
for (k, s, pad), C, Tin, n, et in (((5, 2, 2), 256, 31, 512, 16), ((5, 2, 2), 256, 1001, 64, 32), ((5, 2, 2), 256, 15, 512, 8),
                                   ((3, 1, 1), 256, 16, 512, 16), ((3, 1, 1), 256, 1000, 64, 32), ((1, 1, 0), 256, 250, 256, 32),
                                   ((5, 1, 2), 256, 16, 512, 16)):
    segs, tiles, et, Tout = PK.enc_list_tables([Tin] * n, k, s, pad, et)
    x = torch.randn(C, Tin * n, generator=gen).cuda()
    w = (torch.randn(C, C, k, generator=gen) / (C * k) ** 0.5).cuda()
    b = torch.randn(C, generator=gen).cuda()
    sd, td = torch.from_numpy(segs).cuda(), torch.from_numpy(tiles).cuda()
    ys = {}
    for name, lib in (("old", old), ("new", new)):
        ys[name] = torch.empty(C, int(Tout.sum()), device="cuda")

    def run(lib, y):
        rc = lib.wae_enc_conv_fwd_list(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(sd), len(segs), L.ptr(td), len(tiles), et, x.shape[1],
                                       y.shape[1], C, C, k, s, pad, 1, 0, None)
        assert rc == 0, rc

    run(old, ys["old"]), run(new, ys["new"])
    to, tn = [], []
    for _ in range(9):
        to.append(timed(lambda: run(old, ys["old"])))
        tn.append(timed(lambda: run(new, ys["new"])))
    same = bool(torch.equal(ys["old"], ys["new"]))
    print(f"k{k} s{s} et{et} C{C} Tin{Tin} x{n}: other {statistics.median(to):8.1f} us ({min(to):.1f} .. {max(to):.1f}), "
          f"this tree {statistics.median(tn):8.1f} us ({min(tn):.1f} .. {max(tn):.1f}), same bits {same}", flush=True)
