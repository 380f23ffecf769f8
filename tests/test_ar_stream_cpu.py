"""Streaming decode (wae_ar_desc.t0, incremental_stream, synthesis.py --stream-chunk) without a GPU: the descriptor field and its
declaration, every refusal of a continuation before any launch (raw ctypes calls with dummy pointers, as
tests/test_ar_scalar_coop_cpu.py), the public surface, and the chunked post-processing against the whole-signal one."""
import ctypes
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
INT32_MAX = 2 ** 31 - 1


def _desc(scalar=0, O=32, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_desc_has_a_trailing_t0_that_positional_constructions_leave_zero():
    from wavenet_autoencoders_amd import _lib
    names = [n for n, _ in _lib.ArDesc._fields_]
    assert names[-1] == "t0" and names[-2] == "resident_regs"
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 32, 0, 0, 3, 2, 0, 0, 0.5, 0)      # 18 positional arguments
    assert d.t0 == 0
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 32, 0, 0, 3, 2, 0, 0, 0.5, 0, 1, -1, -1)      # ... and the engine's 21
    assert d.t0 == 0 and d.resident_regs == -1
    assert ctypes.sizeof(_lib.ArDesc) == 4 * len(names)


def test_header_declares_the_field_and_cites_the_lines_it_replaces():
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    block = hdr[hdr.index("typedef struct wae_ar_desc"):hdr.index("} wae_ar_desc;")]
    assert "int32_t t0;" in block
    assert block.rindex("int32_t t0;") > block.index("int32_t resident_regs;")
    for ref in ("conv.py:17-62", "wavenet.py:348-356"):
        assert ref in block, ref


# one caller per decode entry: inputs / inputs_f is the operand a continuation needs
def _ar_generate(lib, d, inputs):
    return lib.wae_ar_generate(ctypes.byref(d), P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, P, None)


def _ar_generate_scalar(lib, d, inputs):
    return lib.wae_ar_generate_scalar(ctypes.byref(d), P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, -7.0, 0, P, P, None)


def _ar_generate_scalar_mog(lib, d, inputs):
    return lib.wae_ar_generate_scalar_mog(ctypes.byref(d), P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, -7.0, P, P, None)


def _ar_generate_coop(lib, d, inputs):
    return lib.wae_ar_generate_coop(ctypes.byref(d), 4, P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, None, P, P, P, None)


def _ar_generate_coop_fused(lib, d, inputs, w_fused=None):
    return lib.wae_ar_generate_coop_fused(ctypes.byref(d), 4, P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, None, P, P, P,
                                          w_fused, None)


def _ar_generate_coop_scalar(dist):
    def call(lib, d, inputs):
        return lib.wae_ar_generate_coop_scalar(ctypes.byref(d), 4, dist, P, P, P, 1, P, 1, 1, P, P, P, P, P, P, None, 0, inputs, P, P, -7.0, 0,
                                               P, P, P, P, P, None)
    return call


ENTRIES = [("ar_generate", _ar_generate, dict(scalar=0, O=32)),
           ("ar_generate_scalar", _ar_generate_scalar, dict(scalar=1, O=30)),
           ("ar_generate_scalar_mog", _ar_generate_scalar_mog, dict(scalar=1, O=30)),
           ("ar_generate_coop", _ar_generate_coop, dict(scalar=0, O=32)),
           ("ar_generate_coop", _ar_generate_coop_fused, dict(scalar=0, O=32)),
           ("ar_generate_coop_scalar", _ar_generate_coop_scalar(0), dict(scalar=1, O=30)),
           ("ar_generate_coop_scalar", _ar_generate_coop_scalar(1), dict(scalar=1, O=30))]


@pytest.mark.parametrize("name,call,kw", ENTRIES, ids=[e[1].__name__.lstrip("_") + str(i) for i, e in enumerate(ENTRIES)])
def test_every_entry_refuses_a_bad_continuation_before_any_launch(name, call, kw):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    err = lambda: lib.wae_last_error()  # noqa: E731
    # a negative start
    assert call(lib, _desc(t0=-1, **kw), P) == -1
    assert name.encode() + b": t0 -1 is negative" in err()
    # t0 + T beyond int32_t (T = 8)
    for t0 in (INT32_MAX, INT32_MAX - 7):
        assert call(lib, _desc(t0=t0, **kw), P) == -1
        assert name.encode() in err() and b"does not fit int32_t" in err()
    # a continuation without inputs: nothing to start from (n_forced resolves to 0)
    for n_forced in (0, 3):
        assert call(lib, _desc(t0=5, n_forced=n_forced, **kw), None) == -1
        assert name.encode() in err() and b"a continuation (t0 > 0) needs inputs" in err()


def test_modes_3_and_4_cannot_be_continued():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    for mode in (3, 4):
        assert _ar_generate(lib, _desc(mode=mode, t0=5), P) == -1
        assert b"cannot resume modes 3 / 4" in lib.wae_last_error()


def test_the_one_handover_form_cannot_be_continued():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ar_generate_coop_fused(lib, _desc(t0=5), P, w_fused=P) == -1
    err = lib.wae_last_error()
    assert b"ar_generate_coop_fused" in err and b"w_fused" in err and b"t0 > 0" in err


def test_decode_entries_bind_the_declared_argument_types():
    """The six wae_ar_generate* signatures, written out parameter by parameter from include/wae.h (not from the prefix _lib.py
    composes them from): the bound argtypes are these lists, element for element."""
    from wavenet_autoencoders_amd import _lib
    D, vp, i32, i64, f32 = ctypes.POINTER(_lib.ArDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    expected = {
        # d, dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes, bias2, zb, first_tab, first_bias,
        # w_head, head_bias, c_up, c_dtype, inputs, uniforms, out_idx, out_logits, stream
        "wae_ar_generate": [D, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp],
        # ... c_dtype, inputs_f, u_mix, u_log, log_scale_min, clamp_log_scale, out_samples, out_params, stream
        "wae_ar_generate_scalar": [D, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, i32, vp, vp, vp],
        # ... c_dtype, inputs_f, u_mix, z, log_scale_min, out_samples, out_params, stream
        "wae_ar_generate_scalar_mog": [D, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, vp, vp, vp],
        # d, C, ... c_dtype, inputs, uniforms, out_idx, out_logits, msg, acc, error, stream
        "wae_ar_generate_coop": [D, i32, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        # ... error, w_fused, stream
        "wae_ar_generate_coop_fused": [D, i32, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                       vp, vp],
        # d, C, dist, ... c_dtype, inputs_f, u_mix, draws, log_scale_min, clamp_log_scale, out_samples, out_params, msg, acc, error, stream
        "wae_ar_generate_coop_scalar": [D, i32, i32, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, i32,
                                        vp, vp, vp, vp, vp, vp],
    }
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    for name, args in expected.items():
        res, bound = _lib.SIGNATURES[name]
        assert res is i32 and list(bound) == args, name
        assert list(getattr(_lib.lib(), name).argtypes) == args, name
        decl = hdr[hdr.index("int " + name + "("):]
        assert len(args) == decl[:decl.index(";")].count(",") + 1, name      # one type per declared parameter


def test_incremental_stream_is_on_every_layer_of_the_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder.wavenet import WaveNet
    sig = inspect.signature(WaeEngine.incremental_stream)
    fwd = inspect.signature(WaeEngine.incremental_forward)
    assert list(sig.parameters)[:5] == ["self", "c", "gid", "T", "chunk"]
    # the keyword arguments of incremental_forward, with its defaults
    for name, par in fwd.parameters.items():
        assert name in sig.parameters and sig.parameters[name].default == par.default, name
    for cls in (WaveNet, VQVAE):
        sig, fwd = inspect.signature(cls.incremental_stream), inspect.signature(cls.incremental_forward)
        assert "chunk" in sig.parameters
        assert [n for n in sig.parameters if n != "chunk"] == list(fwd.parameters)
    assert "inside an open" in WaveNet.clear_buffer.__doc__ and "nothing persists between calls" not in WaveNet.clear_buffer.__doc__


def test_synthesis_has_the_stream_option():
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    assert "--stream-chunk" in src and "incremental_stream" in src
    import sys
    sys.path.insert(0, ROOT)
    import synthesis
    sig = inspect.signature(synthesis.wavegen)
    assert sig.parameters["chunk"].default is None and sig.parameters["on_chunk"].default is None


@pytest.mark.parametrize("postprocess,gain", [("inv_preemphasis", 0.55), ("inv_preemphasis", 0.0), ("none", 0.55)])
def test_chunked_postprocessing_equals_the_whole_signal(postprocess, gain):
    """inv_preemphasis is scipy.signal.lfilter([1], [1, -0.85], x): with the filter state carried from chunk to chunk (zi / zf) the
    recurrence runs the same float64 operations in the same order, so the chunks' float32 outputs are the whole signal's, exactly."""
    import sys
    sys.path.insert(0, ROOT)
    import synthesis
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.0, 1.0, 16000)
    whole = synthesis.postprocess_wave(x, postprocess, gain)
    assert whole.dtype == np.float32
    for chunks in ([1, 7, 1024, 1025, 16000 - 2057], [160] * 100, [16000]):
        post, parts, t = synthesis.ChunkPostprocess(postprocess, gain), [], 0
        for n in chunks:
            parts.append(post(x[t:t + n]))
            t += n
        got = np.concatenate(parts)
        assert got.dtype == np.float32 and np.array_equal(got, whole), (postprocess, gain, len(chunks))
