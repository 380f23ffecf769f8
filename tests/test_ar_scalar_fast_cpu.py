"""Constant-size cooperative kernels and team sessions for scalar-input decoders (wae_ar_desc.scalar_input = 2 = ArDesc.scalar_sized,
wae_ar_generate_coop_scalar_spans, WaeEngine.ar_path(scalar_fast=), decode_session(coop=True) on a scalar engine, synthesis.py
--coop-scalar-fast) without a GPU, in the manner of tests/test_ar_session_cpu.py: the symbol and its binding, every refusal of the new
entry before any launch (raw ctypes calls with dummy pointers), the descriptor's size, wae_ar_coop_ring_floats on scalar descriptors,
the host's routing and the script's arguments."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL = -1
ENTRY, TWIN = "wae_ar_generate_coop_scalar_spans", "wae_ar_generate_coop_scalar_list"


# ---- the symbol, the header, the binding -----------------------------------------------------------------------------------------------
def test_entry_is_exported_declared_and_bound_as_its_list_twin():
    from wavenet_autoencoders_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {ENTRY}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {ENTRY}("):]
    decl = decl[:decl.index(";")]
    twin = hdr[hdr.index(f"int {TWIN}("):]
    twin = twin[:twin.index(";")]
    res, bound = _lib.SIGNATURES[ENTRY]
    assert res is ctypes.c_int32 and list(bound) == list(_lib.SIGNATURES[TWIN][1])
    assert list(getattr(_lib.lib(), ENTRY).argtypes) == list(bound)
    assert len(bound) == decl.count(",") + 1
    norm = lambda t: " ".join(t.split("(", 1)[1].split())  # noqa: E731
    assert norm(decl) == norm(twin).replace("int32_t n_items", "int32_t n_spans").replace("const wae_ar_item* items", "const wae_ar_span* spans")


def test_header_documents_the_field_and_no_longer_says_always_any_shape():
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    block = hdr[hdr.index("typedef struct wae_ar_desc"):hdr.index("} wae_ar_desc;")]
    field = block[block.index("int32_t scalar_input;"):block.index("float scale;")]
    assert "2: a scalar-input decoder" in field and "scalar sized" in field
    for word in ("Class-id entries ignore it", "bit for bit", "O <= 256", "ring_total % 4 == 0", "one-hand-over"):
        assert word.lower() in block.lower(), word
    assert "Always the any-shape kernel" not in hdr and "always the any-shape kernel" not in hdr


def _c_sizeof_desc(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "wae.h"\nint main(void) { printf("%zu\\n", sizeof(wae_ar_desc)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return int(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout)


def test_descriptor_mirror_has_the_headers_size_and_a_flag_that_defaults_to_zero(tmp_path):
    """the struct keeps its fields and its size (tests/test_ar_stream_cpu.py pins t0 as the last one): the request for the constant-size
    scalar kernels is the value 2 of scalar_input, which the mirror reads and writes as a flag of its own"""
    from wavenet_autoencoders_amd import _lib
    names = [n for n, _ in _lib.ArDesc._fields_]
    assert names[-1] == "t0" and "scalar_sized" not in names
    assert ctypes.sizeof(_lib.ArDesc) == 4 * len(names) == _c_sizeof_desc(tmp_path)
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    block = hdr[hdr.index("typedef struct wae_ar_desc"):hdr.index("} wae_ar_desc;")]
    fields = re.findall(r"^\s*(?:int32_t|float)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", block, flags=re.S), flags=re.M)
    assert [f.strip() for fs in fields for f in fs.split(",")] == names
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 30, 0, 0, 3, 2, 0, 1, 0.5, 0)
    assert d.scalar_sized == 0 and d.t0 == 0
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 30, 0, 0, 3, 2, 0, 1, 0.5, 0, 1, -1, -1, 7)      # ... up to and including t0
    assert d.scalar_sized == 0 and d.t0 == 7 and d.scalar_input == 1
    d.scalar_sized = 1
    assert d.scalar_sized == 1 and d.scalar_input == 2
    d.scalar_sized = 0
    assert d.scalar_sized == 0 and d.scalar_input == 1
    c = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, 32, 0, 0, 3, 2, 0, 0, 0.5, 0)      # class ids: no such request
    c.scalar_sized = 1
    assert c.scalar_sized == 0 and c.scalar_input == 0


# ---- refusals of the new entry, before any launch --------------------------------------------------------------------------------------
def _desc(scalar=1, O=30, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _net(w_layers=P, c_up=None, ring_total=4):
    return [P, P, P, ring_total, w_layers, 1, 1, P, P, P, P, P, P, c_up, 0]


def _call(name):
    def call(lib, d, C=8, dist=0, n=3, n_teams=2, recs=P, nxt=P, total=24, inputs_f=P, u_mix=P, draws=P, out_samples=P, out_params=P,
             msg=P, acc=P, error=P, **net):
        return getattr(lib, name)(ctypes.byref(d), C, dist, n, n_teams, recs, nxt, total, *_net(**net), inputs_f, u_mix, draws, -7.0, 0,
                                  out_samples, out_params, msg, acc, error, None)
    return call


# (name, arguments, text of the spans entry, text of the list twin where it words the record differently)
CASES = [
    ("class_id_decoder", dict(d=dict(scalar=0, O=32)), b"needs a scalar-input decoder", None),
    ("t0", dict(d=dict(t0=5)), b"t0 5", None),
    ("t0_negative", dict(d=dict(t0=-1)), b"t0 -1", None),
    ("mode1", dict(d=dict(mode=1)), b"mode must be 0 (teacher-forced parameters) or 2 (sample)", None),
    ("mode3", dict(d=dict(mode=3)), b"mode must be 0", None),
    ("mode4", dict(d=dict(mode=4)), b"mode must be 0", None),
    ("dist2", dict(dist=2), b"dist must be 0", None),
    ("logistic_O_not_3M", dict(d=dict(O=31)), b"3M output channels (got 31)", None),
    ("gaussian_O_4", dict(dist=1, d=dict(O=4)), b"2 or 3M output channels (got 4)", None),
    ("no_teams", dict(n_teams=0), b"n_teams 0 outside 1..8", None),
    ("nine_teams", dict(n_teams=9), b"n_teams 9 outside 1..8", None),
    ("no_members", dict(C=0), b"C 0 outside 1..32", None),
    ("too_many_members", dict(C=33), b"C 33 outside 1..32", None),
    ("wide_R", dict(d=dict(R=257)), b"R, S and O <= 256", None),
    ("wide_S", dict(d=dict(S=320)), b"R, S and O <= 256", None),
    ("wide_O", dict(d=dict(O=300)), b"R, S and O <= 256", None),
    ("no_records", dict(n=0), b"n_spans 0 < 1", b"n_items 0 < 1"),
    ("null_records", dict(recs=None), b"span array", b"item array"),
    ("null_next", dict(nxt=None), b"queue counter", None),
    ("null_msg", dict(msg=None), b"msg, acc and error", None),
    ("null_acc", dict(acc=None), b"msg, acc and error", None),
    ("null_error", dict(error=None), b"msg, acc and error", None),
    ("null_w_layers", dict(w_layers=None), b"null pointer", None),
    ("Cc_without_c_up", dict(d=dict(Cc=4, Ccp=4), c_up=None), b"c_up is null", None),
    ("sample_without_draws", dict(u_mix=None, draws=None, out_samples=None), b"sample mode needs its draws (u_mix and u_log)", None),
    ("gaussian_sample_without_z", dict(dist=1, draws=None, out_samples=None), b"sample mode needs its draws (z)", None),
    ("u_mix_without_u_log", dict(draws=None), b"u_mix and u_log come together", None),
    ("ten_gaussians_without_u_mix", dict(dist=1, u_mix=None), b"10 mixtures need the uniforms u_mix", None),
    ("mode0_without_inputs_f", dict(d=dict(mode=0), inputs_f=None), b"mode 0 needs teacher-forced inputs", None),
    ("samples_without_draws", dict(d=dict(mode=0), u_mix=None, draws=None), b"samples need the draws", None),
    ("no_output", dict(out_samples=None, out_params=None), b"no output requested", None),
    ("ring_total_beyond_32_bits", dict(ring_total=1 << 31), b"ring_total", None),
    # (total + n + 1) * (L + 4) must stay below 2^31: L = 2 -> 357 913 942 is the first total + n + 1 that does not
    ("sequence_overflow", dict(total=357913942 - 4), b"sequence numbers would not fit 31 bits", None),
    ("sequence_overflow_far", dict(total=1 << 40), b"sequence numbers would not fit 31 bits", None),
    ("negative_total", dict(total=-1), b"sequence numbers would not fit 31 bits", None),
]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("case,text,twin_text", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_span_entry_refuses_what_its_list_twin_refuses_under_its_own_name(case, text, twin_text, flag):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    for name, who, want in ((ENTRY, b"ar_generate_coop_scalar_spans: ", text), (TWIN, b"ar_generate_coop_scalar_list: ", twin_text or text)):
        args = dict(case)
        d = _desc(**dict(dict(scalar_sized=flag), **args.pop("d", {})))
        assert _call(name)(lib, d, **args) == EINVAL, name
        err = lib.wae_last_error()
        assert err.startswith(who) and want in err, err


def test_sequence_bound_is_thirty_one_bits_and_the_descriptor_is_not_read_per_clip():
    """the largest list the bound admits is not refused for its size (a later check trips on purpose: nothing launches)"""
    from wavenet_autoencoders_amd import _lib
    lib, call = _lib.lib(), _call(ENTRY)
    assert call(lib, _desc(), total=357913941 - 4, ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()
    assert call(lib, _desc(), total=357913942 - 4, ring_total=1 << 31) == EINVAL
    assert b"sequence numbers" in lib.wae_last_error()
    assert call(lib, _desc(B=-3, T=-9, n_forced=77, init_idx=-5), ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()


# ---- the ring of one clip --------------------------------------------------------------------------------------------------------------
REF = dict(R=256, G=256, S=256, Cc=64, Ccp=64, L=20)
RT = 1052672


def _ring(**kw):
    from wavenet_autoencoders_amd import _lib
    C = kw.pop("C", 32)
    return _lib.lib().wae_ar_coop_ring_floats(ctypes.byref(_desc(**dict(REF, **kw))), C, RT)


@pytest.mark.parametrize("dtype", [0, 1, 2], ids=["fp32", "bf16", "f16"])
@pytest.mark.parametrize("O", [30, 2, 256])
def test_ring_floats_of_a_scalar_clip(dtype, O):
    assert _ring(dtype=dtype, O=O, scalar_sized=1) == RT
    assert _ring(dtype=dtype, O=O, scalar_sized=1, Cc=0, Ccp=0) == RT
    assert _ring(dtype=dtype, O=O, scalar_sized=0) == 32 * RT
    assert _ring(dtype=dtype, O=O) == 32 * RT
    assert _ring(dtype=dtype, O=O, scalar_sized=1, R=128) == 32 * RT
    assert _ring(dtype=dtype, O=O, scalar_sized=1, C=16) == 16 * RT
    assert _ring(dtype=dtype, O=O, scalar_sized=1, coop_generic=1) == 32 * RT
    assert _ring(dtype=dtype, O=O, scalar_sized=1, ktaps=4) == 32 * RT


def test_ring_floats_of_a_class_id_clip_ignore_the_flag():
    for flag in (0, 1):
        assert _ring(scalar=0, dtype=1, O=256, scalar_sized=flag) == RT
        assert _ring(scalar=0, dtype=0, O=256, scalar_sized=flag) == RT
        assert _ring(scalar=0, dtype=1, O=256, scalar_sized=flag, coop_generic=1) == 32 * RT
        assert _ring(scalar=0, dtype=1, O=256, scalar_sized=flag, C=16) == 16 * RT
        assert _ring(scalar=0, dtype=1, O=30, scalar_sized=flag) == 32 * RT      # (no class-id kernel with O != 256)
    from wavenet_autoencoders_amd import _lib
    assert _lib.lib().wae_ar_coop_ring_floats(ctypes.byref(_desc()), 0, 1000) < 0


# ---- the host --------------------------------------------------------------------------------------------------------------------------
CFG = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
           scalar_input=True, output_distribution="Logistic")


def test_team_session_of_a_scalar_decoder_needs_the_engines_opt_in():
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import DecodeSession, WaeEngine
    eng = object.__new__(WaeEngine)
    eng.g = Geometry.from_cfg(CFG)
    with pytest.raises(NotImplementedError, match="scalar-input decoders.*one-CU slots.*does not exist yet"):
        eng.decode_session(coop=True)
    eng.ar_scalar_coop = False
    with pytest.raises(NotImplementedError, match="scalar-input decoders.*one-CU slots"):
        eng.decode_session(coop=True)
    eng.ar_scalar_coop = True
    for mode in ("sample", "logits"):
        sess = eng.decode_session(mode=mode, coop=True, teams=3)
        assert isinstance(sess, DecodeSession) and sess.coop and sess.live == [] and sess.step(7) == {}
    with pytest.raises(ValueError, match="mode 'argmax'"):
        eng.decode_session(mode="argmax", coop=True)
    eng.g = Geometry.from_cfg(dict(CFG, O=300))
    with pytest.raises(ValueError, match=r"R, S and O <= 256 \(got 32, 32, 300\)"):
        eng.decode_session(coop=True)


def test_ar_path_takes_scalar_fast_and_the_scalar_routes_read_it():
    from wavenet_autoencoders_amd.engine import DecodeSession, WaeEngine
    sig = inspect.signature(WaeEngine.ar_path)
    assert sig.parameters["scalar_fast"].default is False and sig.parameters["scalar_coop"].default is False
    eng = object.__new__(WaeEngine)
    eng.ar_one_handover = False
    assert eng.ar_path(scalar_fast=True) is eng
    assert eng.ar_scalar_fast is True and eng.ar_scalar_coop is False      # it implies nothing on its own
    assert eng._ar_scalar_path() == (0, 0, 0)
    eng.ar_path(scalar_coop=True, scalar_fast=True, lds_layers=2, reg_layers=0)
    assert eng.ar_scalar_coop and eng._ar_scalar_path() == (0, 2, -1)
    eng.ar_path(scalar_coop=True, generic=True, lds_layers=2)
    assert eng.ar_scalar_fast is False and eng._ar_scalar_path() == (0, 0, 0)      # without the flag: today's zeros
    # every scalar route reads it in ONE place -- decode.ar_desc, the only constructor of a decode's descriptor
    # (tests/test_decode_host_cpu.py: the structure on the sources, and the descriptor of every route on a device-less engine) -- and
    # the team session's entry is in the launch table, whose launcher checks the exchange of every team entry
    from wavenet_autoencoders_amd import Geometry, decode
    assert decode.ENTRIES[("spans", True, True)] == "wae_ar_generate_coop_scalar_spans"
    eng.g, eng.dt = Geometry.from_cfg(CFG), 1
    for coop, fast, want in ((True, True, 2), (True, False, 1), (False, True, 1)):
        eng.ar_path(scalar_coop=True, scalar_fast=fast, lds_layers=2)
        d = decode.ar_desc(eng, B=1, T=8, mode=2, init_idx=0, n_forced=0, coop=coop)
        assert d.scalar_input == want and d.resident_lds == (2 if want == 2 else 0), (coop, fast)
    assert DecodeSession is decode.DecodeSession
    seen, buf = [], type("Buf", (), {"data_ptr": lambda self: 0x1000})
    msg, acc, err = buf(), buf(), buf()
    eng.lib = type("Lib", (), {ENTRY: staticmethod(lambda *a: seen.append(len(a)) or 0)})()
    eng.stream = lambda: None
    eng._ar_check_exchange = lambda e, who: seen.append((e, who))
    decode.launch(eng, ("spans", True, True), d, [None] * 15, (None, None, None, -7.0, 0, None, None), C=32, dist=0,
                  queue=(1, 1, None, None), total=8, exchange=(msg, acc, err), hold=lambda: seen.append("hold"))
    # the entry first, with all its arguments; the operands are stored while it runs; then its exchange check
    assert seen == [34, "hold", (err, "ar_generate_coop_scalar_spans")]


# ---- synthesis.py ----------------------------------------------------------------------------------------------------------------------
POS = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]


class _Parsed(Exception):
    pass


@pytest.mark.parametrize("extra,coop,fast", [(["--coop-scalar-fast"], True, True), (["--coop-scalar"], True, False), ([], False, False),
                                             (["--batch-decode", "--batch-coop", "--batch-stream", "160", "--coop-scalar-fast"], True, True),
                                             (["--batch-decode", "--batch-coop", "--batch-teams", "2", "--batch-stream", "160",
                                               "--coop-scalar"], True, False)])
def test_synthesis_accepts_the_flag_and_the_team_session_combination(extra, coop, fast, monkeypatch):
    """the arguments parse and reach the engine as ar_path(scalar_coop=, scalar_fast=): the first thing main() does behind its
    argument checks is to read the preset, which is where this test stops it"""
    sys.path.insert(0, ROOT)
    import synthesis
    seen = {}

    def stop(self, text):
        raise _Parsed()
    monkeypatch.setattr(type(synthesis.hparams), "parse", stop)
    real = synthesis.argparse.ArgumentParser.parse_args

    def spy(self, argv=None):
        seen["args"] = real(self, argv)
        return seen["args"]
    monkeypatch.setattr(synthesis.argparse.ArgumentParser, "parse_args", spy)
    with pytest.raises(_Parsed):
        synthesis.main(POS + extra)
    assert seen["args"].coop_scalar is coop and seen["args"].coop_scalar_fast is fast
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    assert "eng.ar_path(scalar_coop=True, scalar_fast=args.coop_scalar_fast)" in src and "--coop-scalar-fast" in synthesis.__doc__
