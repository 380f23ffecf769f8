"""The quantiser kinds without a GPU: Geometry's new fields and their refusals, the parameter and buffer layout per kind (the default
one unchanged), the hparams keys, the C entry's declaration and binding, the float64 restatement of the sliced list statistics, and
the margin condition of the GPU tests' inputs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import vq_cases as V
from oracle import wae_oracle as O
from wavenet_autoencoders_amd import _lib
from wavenet_autoencoders_amd import packing as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
           c_in=39, K=32, cin_pad=0)


def test_default_geometry_and_param_specs_are_unchanged():
    g = P.Geometry.from_cfg(CFG)
    assert (g.vq, g.vq_slices, g.K1, g.vq_decay) == ("plain", 2, None, 0.99)
    specs = P.param_specs(g)
    assert specs[-1] == ("vq.embedding.weight", (32, 16), False)
    assert [n for n, _, _ in specs if n.startswith("vq.")] == ["vq.embedding.weight"]
    sd = O.make_state_dict(CFG, 1)                       # the reference's keys and shapes
    assert {n for n, _, _ in specs} == set(sd) and all(tuple(sd[n].shape) == s for n, s, _ in specs)
    # ... and its registration order, recorded from the reference's own VQVAE at hps/vqwae.json's geometry
    import json
    from helpers import load_npz
    full = P.Geometry(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, n_speakers=153, upsample_scales=[4, 4, 8, 5],
                      c_in=39, encoder_hid=256, K=256)
    assert [n for n, _, _ in P.param_specs(full)] == json.loads(str(load_npz("train_vqwae")["names"]))
    assert specs == P.param_specs(P.Geometry.from_cfg(dict(CFG, vq="plain", vq_slices=2, K1=None, vq_decay=0.99)))
    assert P.vq_buffer_specs(g) == []
    # a decoder-only geometry never looks at the quantiser's fields (Cc = -1 is no multiple of 2)
    assert P.Geometry(layers=4, stacks=2, R=32, G=48, S=32, O=64).vq == "plain"


@pytest.mark.parametrize("kind,extra,want,bufs", [
    ("ema", {}, [("vq.embedding.weight", (32, 16))], [("vq.ema_cluster_size", (32,)), ("vq.ema_w", (32, 16))]),
    ("sliced", {}, [("vq.embedding1.weight", (32, 8)), ("vq.embedding2.weight", (32, 8))], []),
    ("sliced", dict(K1=20), [("vq.embedding1.weight", (32, 8)), ("vq.embedding2.weight", (20, 8))], []),
    ("sliced", dict(vq_slices=4), [(f"vq.embedding{s}.weight", (32, 4)) for s in (1, 2, 3, 4)], []),
    ("sliced_ema", {}, [("vq.embedding1.weight", (32, 8)), ("vq.embedding2.weight", (32, 8))],
     [("vq.ema_cluster_size1", (32,)), ("vq.ema_w1", (32, 8)), ("vq.ema_cluster_size2", (32,)), ("vq.ema_w2", (32, 8))]),
    ("sliced_ema", dict(vq_slices=8), [(f"vq.embedding{s}.weight", (32, 2)) for s in range(1, 9)],
     [x for s in range(1, 9) for x in ((f"vq.ema_cluster_size{s}", (32,)), (f"vq.ema_w{s}", (32, 2)))]),
])
def test_keys_and_shapes_per_kind(kind, extra, want, bufs):
    g = P.Geometry.from_cfg(dict(CFG, vq=kind, **extra))
    specs = P.param_specs(g)
    base = P.param_specs(P.Geometry.from_cfg(CFG))
    assert specs[:len(base) - 1] == base[:-1]                                # everything in front of the quantiser is as before
    assert [(n, s) for n, s, _ in specs[len(base) - 1:]] == want and not any(v for _, _, v in specs[len(base) - 1:])
    assert P.vq_buffer_specs(g) == bufs
    lay = P.ParamLayout(g)
    assert [lay.shapes[n] for n, _ in want] == [s for _, s in want]
    assert [(d0, D, K) for _, d0, D, K in P.vq_slice_specs(g)] == [(d0, D, K) for _, d0, D, K in V.slice_specs(dict(CFG, vq=kind, **extra))]
    # the reference's names for its two-slice classes
    if kind == "sliced_ema" and not extra:
        from wavenet_autoencoders_amd.vector_quantization import SlicedVectorQuantizeEMA
        assert {"vq." + k for k in SlicedVectorQuantizeEMA(32, 16).state_dict()} == {n for n, _ in want + bufs}


@pytest.mark.parametrize("bad", [dict(vq="gumbel"), dict(vq="sliced", vq_slices=1), dict(vq="sliced_ema", vq_slices=9),
                                 dict(vq="sliced", vq_slices=3), dict(vq="sliced_ema", vq_slices=5), dict(vq="plain", K1=20),
                                 dict(vq="ema", K1=20), dict(vq="sliced_ema", K1=20), dict(vq="sliced", vq_slices=4, K1=20)])
def test_geometry_refuses(bad):
    with pytest.raises(ValueError):
        P.Geometry.from_cfg(dict(CFG, **bad))


def test_coefficients_are_the_modules():
    """what the three stand-alone modules of vector_quantization.py pass to the kernels"""
    g = lambda kind: P.Geometry.from_cfg(dict(CFG, vq=kind))  # noqa: E731
    assert P.vq_coeffs(g("sliced"), 0.25) == (1.25, 1.0, 0.25)                 # SlicedVectorQuantize.forward's spec
    assert P.vq_coeffs(g("ema"), 0.25) == P.vq_coeffs(g("sliced_ema"), 0.25) == (0.25, 0.25, None)
    assert P.vq_coeffs(g("plain"), 0.25) == (1.25, 0.25, 1.0)                  # wae_vq_nearest / wae_vq_bwd
    for kind in ("sliced", "ema", "sliced_ema"):
        assert P.vq_coeffs(g(kind), 0.4)[0] == V.coeffs(kind, 0.4)[0]


def test_hparams_keys_and_presets():
    from wavenet_autoencoders_amd.hparams import HParams, _DEFAULTS
    h = HParams(**_DEFAULTS)
    assert (h.quantizer, h.num_slices, h.vq_decay) == ("plain", 2, 0.99) and "quantizer" in h
    before = h.values()
    assert "quantizer" not in before                      # the registry a run saves stays the reference's until a key is used
    for preset in ("vqwae.json", "inae_hp.json"):
        hp = HParams(**_DEFAULTS).parse_json(open(os.path.join(ROOT, "hps", preset)).read())
        assert (hp.quantizer, hp.num_slices, hp.vq_decay) == ("plain", 2, 0.99) and hp.ema is False
    h.parse("quantizer=sliced_ema,num_slices=4,vq_decay=0.9")
    assert (h.quantizer, h.num_slices, h.vq_decay) == ("sliced_ema", 4, 0.9) and h.values()["num_slices"] == 4
    with pytest.raises(ValueError):
        HParams(**_DEFAULTS).parse("num_slices=2.5")
    h2 = HParams(**_DEFAULTS).parse_json('{"quantizer": "ema", "vq_decay": 0.5}')
    assert h2.quantizer == "ema" and h2.vq_decay == 0.5 and h2.num_slices == 2
    with pytest.raises(KeyError):
        HParams(**_DEFAULTS).parse_json('{"quantizer": "ema"}', strict=True)     # not a key of the reference's registry
    import vqwae_train as T
    hp = HParams(**_DEFAULTS).parse_json(open(os.path.join(ROOT, "hps", "vqwae.json")).read())
    g0 = T.build_geometry(hp)
    assert (g0.vq, g0.K) == ("plain", 256)
    hp.parse("quantizer=sliced,num_slices=4")
    g4 = T.build_geometry(hp)
    assert (g4.vq, g4.vq_n, g4.K) == ("sliced", 4, 256) and P.param_specs(g4)[-1] == ("vq.embedding4.weight", (256, 16), False)


def test_entry_is_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    m = re.search(r"\bint\s+wae_vq_search_slices\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 12 == len(_lib.SIGNATURES["wae_vq_search_slices"][1])
    m = re.search(r"\bint64_t\s+wae_vq_search_slices_scratch\s*\(([^)]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 2 == len(_lib.SIGNATURES["wae_vq_search_slices_scratch"][1])
    assert _lib.SIGNATURES["wae_vq_search_slices_scratch"][0] is ctypes.c_int64
    assert re.search(r"#define\s+WAE_VQ_MAX_SLICES\s+8\b", hdr) and _lib.VQ_MAX_SLICES == 8
    m = re.search(r"typedef struct wae_vq_slice_rec \{([^}]*)\}", hdr)
    names = re.findall(r"(\w+)\s*[,;]", m.group(1))
    assert names == [n for n, _ in _lib.VqSliceRec._fields_] and ctypes.sizeof(_lib.VqSliceRec) == 24
    lib = _lib.lib()
    recs = (_lib.VqSliceRec * 2)(_lib.VqSliceRec(None, 0, 8, 24, 1.0), _lib.VqSliceRec(None, 8, 8, 20, 1.0))
    assert lib.wae_vq_search_slices_scratch(recs, 2) == 46
    # argument checks return before any HIP call: they run without a GPU
    d = ctypes.c_void_p(0x1000)
    assert lib.wae_vq_search_slices(d, recs, 2, d, d, d, d, 1, 16, 1, 0, None) == -1          # null codebooks
    assert lib.wae_vq_search_slices(d, recs, 9, d, d, d, d, 1, 16, 1, 0, None) == -1
    assert b"vq_search_slices" in lib.wae_last_error()


def test_sliced_list_statistics_restated_in_float64():
    """per item: vq_loss = c_loss sum_s sqerr_s / (Tq Dtot), perp = sum_s perp_s, hist (n, max K_s) zero beyond K_s; the list's totals
    are packing.vq_list_totals per slice (c_loss_s = c_loss D_s / Dtot), added over the slices"""
    cfg = dict(CFG, vq="sliced", vq_slices=2, K1=20)
    rng = np.random.default_rng(0)
    specs = V.slice_specs(cfg)
    items, per_slice = [], [dict(sq=[], hist=[]) for _ in specs]
    for Tq in (1, 5, 9):
        lat, quant = rng.standard_normal((16, Tq)), rng.standard_normal((16, Tq))
        idx = np.stack([rng.integers(0, K, Tq) for _, _, _, K in specs])
        vq, perp, hist, sq = V.list_stats_f64(cfg, lat, quant, idx)
        assert hist.shape == (2, 32) and hist[1, 20:].sum() == 0 and (hist.sum(1) == Tq).all()
        assert abs(vq - 1.25 * ((quant - lat) ** 2).mean()) < 1e-12          # the slices' errors add up to the whole width's
        items.append((vq, perp, Tq))
        for s, (_, _, _, K) in enumerate(specs):
            per_slice[s]["sq"].append(sq[s])
            per_slice[s]["hist"].append(hist[s, :K])
    tot_vq = tot_perp = 0.0
    for (_, _, D, K), a in zip(specs, per_slice):
        vq, perp, frames, sq = P.vq_list_totals(a["sq"], np.stack(a["hist"]), D, 1.25 * D / 16)
        assert frames == 15
        tot_vq, tot_perp = tot_vq + vq, tot_perp + perp
    assert abs(tot_vq - sum(v * t for v, _, t in items) / 15) < 1e-12          # frame-weighted mean of the items' losses
    assert 2.0 <= tot_perp <= 32 + 20


@pytest.mark.parametrize("name", sorted({**V.KINDS, **V.LIST_KINDS}))
def test_margin_condition_of_the_gpu_inputs(name):
    """every frame's top-2 distance gap in every slice is at least 1e-4 of the slice's largest distance in float64 (fp32 rounding of
    a <= 64-term distance is below 5e-6 of it), and the fp32 and fp64 oracles agree on every index"""
    cfg, sd, ins, _ = V.model_case({**V.KINDS, **V.LIST_KINDS}[name])
    with torch.no_grad():
        lat = O.encoder_forward(sd, ins["c"])
        assert V.worst_margin(cfg, sd, lat) >= V.MARGIN
        if cfg.get("vq_slices", 2) == 2:
            sd64 = {k: v.double() for k, v in sd.items()}
            i32 = V.quantise(cfg, sd, lat)[3]
            i64 = V.quantise(cfg, sd64, O.encoder_forward(sd64, ins["c"].double()))[3]
            assert all(torch.equal(a, b) for a, b in zip(i32, i64))
