"""List decoding (wae_ar_generate_list, WaeEngine.decode_list, synthesis.py --batch-decode) without a GPU: the launch planner, the
symbol and its declaration, every refusal of the entry before any launch (raw ctypes calls with dummy pointers, as
tests/test_ar_stream_cpu.py), and the host-side refusals."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2


# ---- packing.ar_list_plan --------------------------------------------------------------------------------------------------------------
def test_plan_offsets_are_contiguous_in_the_callers_order():
    from wavenet_autoencoders_amd.packing import ar_list_plan
    rng = np.random.default_rng(3)
    n = rng.integers(1, 5000, 37)
    p = ar_list_plan(n, 8)
    assert p.total == int(n.sum())
    assert p.offsets[0] == 0 and np.array_equal(p.offsets[1:], np.cumsum(n)[:-1])
    assert int(p.offsets[-1] + n[-1]) == p.total
    assert p.offsets.dtype == np.int64


def test_plan_order_is_a_permutation_longest_first():
    from wavenet_autoencoders_amd.packing import ar_list_plan
    rng = np.random.default_rng(4)
    n = rng.integers(1, 5000, 101)
    p = ar_list_plan(n, 16)
    assert sorted(p.order.tolist()) == list(range(101))
    assert np.all(np.diff(n[p.order]) <= 0)


def test_plan_keeps_the_callers_order_among_equal_lengths():
    from wavenet_autoencoders_amd.packing import ar_list_plan
    p = ar_list_plan([7, 9, 7, 9, 9, 3, 7], 2)
    assert p.order.tolist() == [1, 3, 4, 0, 2, 6, 5]
    assert ar_list_plan([5] * 6, 4).order.tolist() == list(range(6))


def test_plan_clamps_slots_to_the_item_count_and_simulates_the_queue():
    from wavenet_autoencoders_amd.packing import ar_list_plan
    p = ar_list_plan([5, 9], 256)
    assert p.slots == 2 and p.makespan == 9 and p.efficiency == 14 / 18
    # two slots, items taken in launch order by whichever slot is free: 9 | 9, then 7 -> slot 0 (16), 5 -> slot 1 (14), 3 -> slot 1 (17)
    p = ar_list_plan([5, 9, 9, 3, 7], 2)
    assert p.slots == 2 and p.makespan == 17 and p.efficiency == 33 / 34
    assert ar_list_plan([4, 4, 4, 4], 1).makespan == 16
    for bad in (([], 4), ([3, 0], 4), ([3, 4], 0)):
        with pytest.raises(ValueError):
            ar_list_plan(*bad)


# ---- the symbol ------------------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wae_ar_generate_list\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index("int wae_ar_generate_list("):]
    decl = decl[:decl.index(";")]
    D, vp, i32, i64 = ctypes.POINTER(_lib.ArDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # d, n_items, n_slots, items, next, dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes, bias2, zb,
    # first_tab, first_bias, w_head, head_bias, c_up, c_dtype, inputs, uniforms, out_idx, out_logits, stream
    args = [D, i32, i32, vp, vp, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    res, bound = _lib.SIGNATURES["wae_ar_generate_list"]
    assert res is i32 and list(bound) == args
    assert list(_lib.lib().wae_ar_generate_list.argtypes) == args
    assert len(args) == decl.count(",") + 1
    # the item struct: the header's fields in the header's order, 24 bytes
    block = hdr[hdr.index("typedef struct wae_ar_item"):hdr.index("} wae_ar_item;")]
    names = [n for n, _ in _lib.ArItem._fields_]
    assert names == ["off", "T", "n_forced", "init_idx", "row"]
    pos = [block.index(f" {n};") for n in names]
    assert pos == sorted(pos) and "int64_t off;" in block
    assert ctypes.sizeof(_lib.ArItem) == 24 and _lib.ArItem.T.offset == 8 and _lib.ArItem.row.offset == 20


# ---- refusals of the entry, before any launch ------------------------------------------------------------------------------------------
def _desc(scalar=0, O=32, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, n_items=3, n_slots=2, items=P, nxt=P, inputs=P, uniforms=P):
    return lib.wae_ar_generate_list(ctypes.byref(d), n_items, n_slots, items, nxt, P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0,
                                    inputs, uniforms, P, P, None)


@pytest.mark.parametrize("case,code,text", [
    (dict(d=dict(scalar=1, O=30)), EUNSUPPORTED, b"class-id decoders"),
    (dict(d=dict(mode=3)), EUNSUPPORTED, b"modes 3 / 4"),
    (dict(d=dict(mode=4)), EUNSUPPORTED, b"modes 3 / 4"),
    (dict(d=dict(t0=5)), EINVAL, b"t0 5"),
    (dict(d=dict(t0=-1)), EINVAL, b"t0 -1"),
    (dict(n_items=0), EINVAL, b"n_items 0 < 1"),
    (dict(n_items=-2), EINVAL, b"n_items -2 < 1"),
    (dict(n_slots=0), EINVAL, b"n_slots 0 < 1"),
    (dict(items=None), EINVAL, b"item array"),
    (dict(nxt=None), EINVAL, b"queue counter"),
    (dict(d=dict(mode=0), inputs=None), EINVAL, b"mode 0 needs inputs"),
    (dict(d=dict(mode=2), uniforms=None), EINVAL, b"sample mode needs uniforms"),
], ids=["scalar_input", "mode3", "mode4", "t0", "t0_negative", "no_items", "negative_items", "no_slots", "null_items", "null_next",
        "mode0_without_inputs", "mode2_without_uniforms"])
def test_entry_refuses_before_any_launch(case, code, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    case = dict(case)
    d = _desc(**case.pop("d", {}))
    assert _call(lib, d, **case) == code
    err = lib.wae_last_error()
    assert b"ar_generate_list" in err and text in err, err


# ---- the host --------------------------------------------------------------------------------------------------------------------------
def test_decode_list_refuses_scalar_input_geometries_without_a_device():
    """the check comes before anything that needs the engine's device state: an engine object that never saw a GPU is enough"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
               scalar_input=True, output_distribution="Logistic")
    eng = object.__new__(WaeEngine)
    eng.g = Geometry.from_cfg(cfg)
    with pytest.raises(NotImplementedError, match="class-id decoders"):
        eng.decode_list([dict(c=None, gid=0, T=8)])
    eng.g = Geometry.from_cfg(dict(cfg, O=32, scalar_input=False))
    with pytest.raises(ValueError, match="empty list"):
        eng.decode_list([])
    with pytest.raises(ValueError, match="mode 'probs'"):
        eng.decode_list([dict(c=None, gid=0, T=8)], mode="probs")


def test_decode_list_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.decode_list)
    assert list(sig.parameters)[:5] == ["self", "items", "mode", "slots", "want_logits"]
    assert sig.parameters["mode"].default == "sample" and sig.parameters["slots"].default is None
    assert sig.parameters["want_logits"].default is False
    doc = WaeEngine.decode_list.__doc__
    assert "ar_path()" in doc and "WAE_AR_COOP" in doc


def test_synthesis_has_the_batch_option_and_refuses_it_with_stream_chunk(capsys):
    sys.path.insert(0, ROOT)
    import synthesis
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    assert "--batch-decode" in src and "decode_list" in src
    pos = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]
    with pytest.raises(SystemExit) as e:
        synthesis.main(pos + ["--batch-decode", "--stream-chunk", "700"])
    assert e.value.code == 2
    assert "--stream-chunk" in capsys.readouterr().err
