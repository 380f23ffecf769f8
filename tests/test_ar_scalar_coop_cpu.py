"""The cooperative decode entry of scalar-input decoders (wae_ar_generate_coop_scalar, csrc/ar_coop.hip) without a GPU: the library
exports it, include/wae.h declares it, the ctypes table binds it, and every refusal returns before any launch (raw ctypes calls with
dummy pointers, as tests/test_mog_cpu.py::test_new_entries_refuse_bad_arguments_before_any_launch)."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "wae_ar_generate_coop_scalar"


def test_symbol_is_exported_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    for ref in ("wavenet.py:284-285", "325-333", "mixture.py:118-156", "mixture.py:225-270"):      # the reference lines it replaces
        assert ref in hdr[hdr.index("Scalar-input decoders on C cooperating workgroups"):hdr.index("int " + NAME)], ref
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES
    # one argument type per parameter of the declaration
    decl = hdr[hdr.index("int " + NAME):]
    decl = decl[:decl.index(";")]
    assert len(_lib.SIGNATURES[NAME][1]) == decl.count(",") + 1


def test_engine_switch_is_an_argument_not_an_environment_variable():
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.ar_path)
    assert sig.parameters["scalar_coop"].default is False
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    assert "--coop-scalar" in src and "scalar_coop=True" in src


def _call(lib, d, C=32, dist=0, inputs_f=None, u_mix=None, draws=None, out_samples=None, out_params=None):
    p = ctypes.c_void_p(0x1000)
    return lib.wae_ar_generate_coop_scalar(ctypes.byref(d), C, dist, p, p, p, 1, p, 1, 1, p, p, p, p, p, p, None, 0,
                                           inputs_f, u_mix, draws, -7.0, 0, out_samples, out_params, p, p, p, None)


def _desc(**kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O   Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 30, 0, 0, 3, 2, 0, 1, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refusals_before_any_launch():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    err = lambda: lib.wae_last_error()  # noqa: E731
    ok = dict(u_mix=p, draws=p, out_samples=p)
    # a class-id decoder
    assert _call(lib, _desc(scalar_input=0), **ok) == -1 and b"scalar-input decoder" in err()
    # an output width the distribution cannot have
    assert _call(lib, _desc(O=31), **ok) == -1 and b"3M output channels" in err()
    assert _call(lib, _desc(O=2), dist=0, **ok) == -1 and b"3M output channels" in err()
    assert _call(lib, _desc(O=4), dist=1, **ok) == -1 and b"2 or 3M" in err()
    assert _call(lib, _desc(), dist=2, **ok) == -1 and b"dist must be" in err()
    # more utterances / members / channels than the cooperative kernel takes
    assert _call(lib, _desc(B=9), **ok) == -1 and b"1..8 utterances" in err()
    for C in (0, 33):
        assert _call(lib, _desc(), C=C, **ok) == -1 and b"1..32 cooperating" in err()
    for field in ("R", "S", "O"):
        assert _call(lib, _desc(**{field: 258}), **ok) == -1 and b"R, S, O <= 256" in err()
    # modes other than 0 and 2
    for mode in (1, 3, 4):
        assert _call(lib, _desc(mode=mode), **ok) == -1 and b"mode must be 0" in err()
    # a sampled decode without its draws
    assert _call(lib, _desc(), dist=0, out_params=p) == -1 and b"needs its draws" in err()
    assert _call(lib, _desc(), dist=0, u_mix=p, out_params=p) == -1 and b"come together" in err()
    assert _call(lib, _desc(), dist=1, u_mix=p, out_params=p) == -1 and b"needs its draws" in err()
    # the mixture pick of more than one Gaussian needs u_mix; one Gaussian does not (it gets past that check)
    assert _call(lib, _desc(), dist=1, draws=p, out_samples=p) == -1 and b"need the uniforms u_mix" in err()
    assert _call(lib, _desc(O=2), dist=1, draws=p) == -1 and b"no output requested" in err()
    # teacher-forced parameters need inputs for every step
    assert _call(lib, _desc(mode=0), out_params=p) == -1 and b"every step" in err()
    assert _call(lib, _desc(mode=0, n_forced=3), inputs_f=p, out_params=p) == -1 and b"every step" in err()
    # samples without draws, and no output at all
    assert _call(lib, _desc(mode=0), inputs_f=p, out_samples=p) == -1 and b"samples need the draws" in err()
    assert _call(lib, _desc(), u_mix=p, draws=p) == -1 and b"no output requested" in err()
    assert _call(lib, _desc(mode=0), inputs_f=p) == -1 and b"no output requested" in err()
    # the class-id entry points scalar decoders to this one
    assert lib.wae_ar_generate_coop(ctypes.byref(_desc()), 32, p, p, p, 1, p, 1, 1, p, p, p, p, p, p, None, 0, None, p, p, None, p, p, p,
                                    None) == -1
    assert NAME.encode() in err()
