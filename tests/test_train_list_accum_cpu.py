"""Ragged micro-batches in accumulation windows without a GPU: a group's entry for distributed.accum_weights from its plan, the
fixed-order entry of the list upsampling backward (declared, bound, its size query and its refusals before any launch), the public
surface, and vqwae_train.py's checks on --train-packed with --accum-steps and --deterministic that run before an engine exists."""
import ctypes
import inspect
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PTR = ctypes.c_void_p(0x1000)
FRAMES = (8, 12, 4, 36)          # tests/test_gpu_train_list.py's utterances: 160 samples per feature frame


def _geometry():
    from helpers import golden_model
    from wavenet_autoencoders_amd import Geometry
    return Geometry.from_cfg(golden_model("A")[0])


def test_group_metas_and_weights_of_the_2_plus_2_split():
    from wavenet_autoencoders_amd import packing as P
    from wavenet_autoencoders_amd import train as TR
    from wavenet_autoencoders_amd.distributed import accum_weights
    g = _geometry()
    Ts = [160 * f for f in FRAMES]
    assert Ts == [1280, 1920, 640, 5760]
    metas = []
    for lo in (0, 2):
        tp = P.train_list_plan(g, Ts[lo:lo + 2], FRAMES[lo:lo + 2])
        B, Tmax, lengths, elems = TR.list_meta(g, tp)
        assert (B, Tmax) == (2, max(Ts[lo:lo + 2])) and lengths.tolist() == Ts[lo:lo + 2]
        metas.append((B, Tmax, lengths, elems))
    assert [m[3] for m in metas] == [g.Cc * 5, g.Cc * 10]
    weights, N = accum_weights(metas)
    assert N == 9596
    assert [w[0] * N for w in weights] == pytest.approx([3198, 6398], abs=1e-9)
    assert [w[1] for w in weights] == pytest.approx([5 / 15, 10 / 15], abs=1e-15)
    assert sum(w[0] for w in weights) == pytest.approx(1.0, abs=1e-15) and sum(w[1] for w in weights) == pytest.approx(1.0, abs=1e-15)


def test_a_decoder_only_group_has_no_latent_elements():
    from helpers import golden_model
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd import packing as P
    from wavenet_autoencoders_amd import train as TR
    cfg = {k: v for k, v in golden_model("A")[0].items() if k not in ("c_in", "encoder_hid", "K")}
    g = Geometry.from_cfg(cfg)
    tp = P.train_list_plan(g, [1920, 640], [3, 1])
    B, Tmax, lengths, elems = TR.list_meta(g, tp)
    assert (B, Tmax, lengths.tolist(), elems) == (2, 1920, [1920, 640], 0)


ENTRIES = {"wae_upsample_stage_bwd_list_det_floats": 0, "wae_upsample_stage_bwd_list_det": 15}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_entries_are_declared_and_bound(name):
    from wavenet_autoencoders_amd import _lib
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*?)\);", header, re.S)
    assert m, f"{name} is not declared in include/wae.h"
    nargs = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
    assert nargs == ENTRIES[name] == len(_lib.SIGNATURES[name][1])
    assert getattr(_lib.lib(), name).argtypes is not None


def test_the_header_states_the_order():
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    for word in ("wae_upsample_stage_bwd_list_det: wae_upsample_stage_bwd_list", "walks the tiles", "parts[0 .. grid-1][tap] in index",
                 "order from zero", "512 * 33 floats"):
        assert word in header, word


def test_the_size_query_and_the_refusals_before_any_launch():
    """(the pointers are not device memory and there may be no device)"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    n = 512 * 33
    assert lib.wae_upsample_stage_bwd_list_det_floats() == n
    ok = dict(dout=PTR, inp=PTR, w=PTR, din=PTR, dw=PTR, segs=PTR, nsegs=2, ntiles=3, in_pitch=40, out_pitch=160, C=3, s=4, parts=PTR, n=n)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.wae_upsample_stage_bwd_list_det(a["dout"], a["inp"], a["w"], a["din"], a["dw"], a["segs"], a["nsegs"], a["ntiles"],
                                                   a["in_pitch"], a["out_pitch"], a["C"], a["s"], a["parts"], a["n"], None)

    bad = [dict(parts=None), dict(n=n - 1), dict(n=0),
           # what the default twin refuses
           dict(dout=None), dict(inp=None), dict(w=None), dict(din=None), dict(dw=None), dict(segs=None), dict(nsegs=0), dict(ntiles=0),
           dict(in_pitch=0), dict(out_pitch=0), dict(C=0), dict(s=0), dict(s=17)]
    for kw in bad:
        assert call(**kw) == EINVAL, (kw, lib.wae_last_error())
        d = {k: v for k, v in dict(ok, **kw).items() if k not in ("parts", "n")}
        if "parts" not in kw and "n" not in kw:
            assert lib.wae_upsample_stage_bwd_list(d["dout"], d["inp"], d["w"], d["din"], d["dw"], d["segs"], d["nsegs"], d["ntiles"],
                                                   d["in_pitch"], d["out_pitch"], d["C"], d["s"], None) == EINVAL, kw


def test_the_public_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.accumulate_list)
    assert list(sig.parameters)[:2] == ["self", "items"]
    want = dict(ce_weight=1.0, vq_weight=1.0, ce_count=None, beta=0.25, quantize_channels=65536, log_scale_min=-7.0, max_rows=None)
    for k, v in want.items():
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters[k].default == v, k
    sig = inspect.signature(WaeEngine.train_step_list_accum)
    assert list(sig.parameters)[:2] == ["self", "groups"]
    for k in ("lr", "betas", "eps", "weight_decay", "clip_thresh", "ema_decay", "beta", "grad_hook", "max_rows", "grad_sync"):
        assert k in sig.parameters, k
    for fn in (WaeEngine.accumulate_list, WaeEngine.train_step_list_accum):
        assert fn.__doc__ and "deterministic" in fn.__doc__


def test_train_step_list_shares_its_intake_with_the_window():
    from wavenet_autoencoders_amd import train as TR
    for fn in (TR.train_step_list, TR.accumulate_list):
        src = inspect.getsource(fn)
        for word in ("list_refusals(", "list_intake(", "list_dense_inputs(", "list_forward("):
            assert word in src, (fn.__name__, word)


def _args(monkeypatch, argv):
    import vqwae_train
    for k in list(os.environ):
        if k.startswith("WAE_"):
            monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("WAE_DETERMINISTIC", "0")          # (monkeypatch restores what engine_switches sets)
    return vqwae_train, vqwae_train.parse_args(argv)


def test_the_script_takes_packed_windows_before_an_engine_exists(monkeypatch):
    hp, geom = types.SimpleNamespace(max_time_steps=None), types.SimpleNamespace(vq="plain")
    for argv in (["--train-packed", "--accum-steps", "2"], ["--train-packed", "--deterministic"],
                 ["--train-packed", "--accum-steps", "4", "--deterministic"], ["--train-packed"]):
        V, args = _args(monkeypatch, argv)
        V.refuse_combinations(args, hp, geom, 1, V.engine_switches(args))
    src = inspect.getsource(V.main)
    assert src.index("refuse_combinations(args, hp, geom, world, engine_switches(args))") < src.index("WaeEngine(geom")
    assert "train_step_list_accum(" in src


def test_the_script_still_refuses_what_no_ragged_step_covers(monkeypatch):
    hp, geom = types.SimpleNamespace(max_time_steps=None), types.SimpleNamespace(vq="plain")
    V, args = _args(monkeypatch, ["--train-packed", "--accum-steps", "2"])
    with pytest.raises(NotImplementedError, match="one GPU"):
        V.refuse_combinations(args, hp, geom, 2, V.engine_switches(args))
    V, args = _args(monkeypatch, ["--train-packed"])
    with pytest.raises(NotImplementedError, match="one GPU"):
        V.refuse_combinations(args, hp, geom, 2, V.engine_switches(args))
    with pytest.raises(ValueError, match="max_time_steps"):
        V.refuse_combinations(args, types.SimpleNamespace(max_time_steps=8000), geom, 1, V.engine_switches(args))
    V, args = _args(monkeypatch, ["--train-packed", "--accum-steps", "2"])
    with pytest.raises(NotImplementedError, match="plain quantiser"):
        V.refuse_combinations(args, hp, types.SimpleNamespace(vq="sliced"), 1, V.engine_switches(args))
    V, args = _args(monkeypatch, ["--train-packed", "--deterministic"])
    with pytest.raises(NotImplementedError, match="plain quantiser"):
        V.refuse_combinations(args, hp, types.SimpleNamespace(vq="sliced_ema"), 1, V.engine_switches(args))
    V, args = _args(monkeypatch, ["--deterministic"])
    with pytest.raises(NotImplementedError, match="data parallel"):
        V.refuse_combinations(args, hp, geom, 2, V.engine_switches(args))
