"""Decode sessions (wae_ar_generate_spans, wae_ar_generate_scalar_spans, wae_ar_generate_coop_spans, WaeEngine.decode_session /
decode_list_stream, synthesis.py --batch-decode --batch-stream) without a GPU: the span record and the three symbols, every refusal of
the entries before any launch (raw ctypes calls with dummy pointers, as tests/test_ar_list_cpu.py), the round planner, the host-side
refusals and the script's argument errors."""
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
SLOTS, SCALAR, TEAMS = "wae_ar_generate_spans", "wae_ar_generate_scalar_spans", "wae_ar_generate_coop_spans"
TWIN = {SLOTS: "wae_ar_generate_list", SCALAR: "wae_ar_generate_scalar_list", TEAMS: "wae_ar_generate_coop_list"}


# ---- the record and the symbols --------------------------------------------------------------------------------------------------------
def test_span_record_is_forty_bytes_and_matches_the_packed_dtype():
    from wavenet_autoencoders_amd import _lib
    from wavenet_autoencoders_amd.decode import _AR_SPAN
    names = ["off", "ring", "T", "t0", "n_forced", "init_idx", "row", "reserved"]
    assert [n for n, _ in _lib.ArSpan._fields_] == names == list(_AR_SPAN.names)
    assert ctypes.sizeof(_lib.ArSpan) == 40 == _AR_SPAN.itemsize
    for n in names:
        f = getattr(_lib.ArSpan, n)
        assert f.offset == _AR_SPAN.fields[n][1] and f.size == _AR_SPAN.fields[n][0].itemsize, n
    assert [getattr(_lib.ArSpan, n).offset for n in names] == [0, 8, 16, 20, 24, 28, 32, 36]
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    block = hdr[hdr.index("typedef struct wae_ar_span"):hdr.index("} wae_ar_span;")]
    pos = [block.index(f" {n};") for n in names]
    assert pos == sorted(pos) and "int64_t off;" in block and "int64_t ring;" in block
    # the item record and its entries are untouched
    assert ctypes.sizeof(_lib.ArItem) == 24 and [n for n, _ in _lib.ArItem._fields_] == ["off", "T", "n_forced", "init_idx", "row"]


@pytest.mark.parametrize("entry", [SLOTS, SCALAR, TEAMS])
def test_entries_are_exported_declared_and_bound_as_their_list_twins(entry):
    from wavenet_autoencoders_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {entry}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {entry}("):]
    decl = decl[:decl.index(";")]
    twin = hdr[hdr.index(f"int {TWIN[entry]}("):]
    twin = twin[:twin.index(";")]
    res, bound = _lib.SIGNATURES[entry]
    assert res is ctypes.c_int32 and list(bound) == list(_lib.SIGNATURES[TWIN[entry]][1])
    assert list(getattr(_lib.lib(), entry).argtypes) == list(bound)
    assert len(bound) == decl.count(",") + 1
    # the operand list of the twin, with spans for items
    norm = lambda t: " ".join(t.split("(", 1)[1].split())  # noqa: E731
    assert norm(decl) == norm(twin).replace("int32_t n_items", "int32_t n_spans").replace("const wae_ar_item* items", "const wae_ar_span* spans")
    comment = hdr[:hdr.index("typedef struct wae_ar_span")]
    comment = comment[comment.rindex("/*"):]
    for word in ("bit for bit", "span.t0 + t", "d->t0 itself must be 0", "at most one span", "inputs[off]", "n_forced = 1", "rendezvous A",
                 "C * ring_total", "2^31", "zb words"):
        assert word in comment, word


# ---- refusals of the entries, before any launch ----------------------------------------------------------------------------------------
def _desc(scalar=0, O=32, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _net(w_layers=P, c_up=None, ring_total=4):
    return [P, P, P, ring_total, w_layers, 1, 1, P, P, P, P, P, P, c_up, 0]


def _call_slots(lib, d, n_spans=3, n_slots=2, spans=P, nxt=P, inputs=P, uniforms=P, out_idx=P, **net):
    return lib.wae_ar_generate_spans(ctypes.byref(d), n_spans, n_slots, spans, nxt, *_net(**net), inputs, uniforms, out_idx, P, None)


def _call_teams(lib, d, C=8, n_spans=3, n_teams=2, spans=P, nxt=P, total=24, inputs=P, uniforms=P, out_idx=P, msg=P, acc=P, error=P, **net):
    return lib.wae_ar_generate_coop_spans(ctypes.byref(d), C, n_spans, n_teams, spans, nxt, total, *_net(**net), inputs, uniforms, out_idx, P,
                                          msg, acc, error, None)


def _call_scalar(lib, d, dist=0, n_spans=3, n_slots=2, spans=P, nxt=P, inputs_f=P, u_mix=P, draws=P, out_samples=P, out_params=P, **net):
    return lib.wae_ar_generate_scalar_spans(ctypes.byref(d), dist, n_spans, n_slots, spans, nxt, *_net(**net), inputs_f, u_mix, draws, -7.0, 0,
                                            out_samples, out_params, None)


QUEUE = [
    ("t0", dict(d=dict(t0=5)), EINVAL, b"t0 5"),
    ("t0_negative", dict(d=dict(t0=-1)), EINVAL, b"t0 -1"),
    ("no_spans", dict(n_spans=0), EINVAL, b"n_spans 0 < 1"),
    ("negative_spans", dict(n_spans=-2), EINVAL, b"n_spans -2 < 1"),
    ("null_spans", dict(spans=None), EINVAL, b"span array"),
    ("null_next", dict(nxt=None), EINVAL, b"queue counter"),
]
FAULTS = [
    ("null_w_layers", dict(w_layers=None), EINVAL, b"null pointer"),
    ("dtype_7", dict(d=dict(dtype=7)), EINVAL, b"bad dtype"),
    ("odd_G", dict(d=dict(G=47)), EINVAL, b"bad sizes"),
    ("Cc_without_c_up", dict(d=dict(Cc=4, Ccp=4), c_up=None), EINVAL, b"c_up is null"),
]
CLASS_IDS = [
    ("scalar_input", dict(d=dict(scalar=1, O=30)), EUNSUPPORTED, b"class-id decoders"),
    ("mode3", dict(d=dict(mode=3)), EUNSUPPORTED, b"modes 3 / 4"),
    ("mode4", dict(d=dict(mode=4)), EUNSUPPORTED, b"modes 3 / 4"),
    ("mode5", dict(d=dict(mode=5)), EINVAL, b"mode must be 0"),
    ("mode0_without_inputs", dict(d=dict(mode=0), inputs=None), EINVAL, b"mode 0 needs inputs"),
    ("mode2_without_uniforms", dict(d=dict(mode=2), uniforms=None), EINVAL, b"sample mode needs uniforms"),
    ("null_out_idx", dict(out_idx=None), EINVAL, b"null pointer"),
]
SLOTS_ONLY = [("no_slots", dict(n_slots=0), EINVAL, b"n_slots 0 < 1"), ("negative_slots", dict(n_slots=-1), EINVAL, b"n_slots -1 < 1")]
TEAMS_ONLY = [
    ("no_teams", dict(n_teams=0), EINVAL, b"n_teams 0 outside 1..8"),
    ("nine_teams", dict(n_teams=9), EINVAL, b"n_teams 9 outside 1..8"),
    ("no_members", dict(C=0), EINVAL, b"C 0 outside 1..32"),
    ("too_many_members", dict(C=33), EINVAL, b"C 33 outside 1..32"),
    ("wide_R", dict(d=dict(R=257)), EINVAL, b"R, S and O <= 256"),
    ("wide_S", dict(d=dict(S=320)), EINVAL, b"R, S and O <= 256"),
    ("wide_O", dict(d=dict(O=300)), EINVAL, b"R, S and O <= 256"),
    ("null_msg", dict(msg=None), EINVAL, b"msg, acc and error"),
    ("null_acc", dict(acc=None), EINVAL, b"msg, acc and error"),
    ("null_error", dict(error=None), EINVAL, b"msg, acc and error"),
    ("ring_total_beyond_32_bits", dict(ring_total=1 << 31), EINVAL, b"ring_total"),
    # (total + n_spans + 1) * (L + 4) must stay below 2^31: L = 2 -> 357 913 942 is the first total + n_spans + 1 that does not
    ("sequence_overflow", dict(total=357913942 - 4), EINVAL, b"sequence numbers would not fit 31 bits"),
    ("sequence_overflow_far", dict(total=1 << 40), EINVAL, b"sequence numbers would not fit 31 bits"),
    ("negative_total", dict(total=-1), EINVAL, b"sequence numbers would not fit 31 bits"),
]
SCALAR_ONLY = [
    ("class_id_decoder", dict(d=dict(scalar=0, O=32)), EINVAL, b"needs a scalar-input decoder"),
    ("mode1", dict(d=dict(mode=1)), EINVAL, b"mode must be 0 (teacher-forced parameters) or 2 (sample)"),
    ("mode3", dict(d=dict(mode=3)), EINVAL, b"mode must be 0"),
    ("mode4", dict(d=dict(mode=4)), EINVAL, b"mode must be 0"),
    ("dist2", dict(dist=2), EINVAL, b"dist must be 0"),
    ("logistic_O_not_3M", dict(d=dict(O=31)), EINVAL, b"3M output channels (got 31)"),
    ("gaussian_O_4", dict(dist=1, d=dict(O=4)), EINVAL, b"2 or 3M output channels (got 4)"),
    ("sample_without_draws", dict(u_mix=None, draws=None, out_samples=None), EINVAL, b"sample mode needs its draws (u_mix and u_log)"),
    ("gaussian_sample_without_z", dict(dist=1, draws=None, out_samples=None), EINVAL, b"sample mode needs its draws (z)"),
    ("u_mix_without_u_log", dict(draws=None), EINVAL, b"u_mix and u_log come together"),
    ("ten_gaussians_without_u_mix", dict(dist=1, u_mix=None), EINVAL, b"10 mixtures need the uniforms u_mix"),
    ("mode0_without_inputs_f", dict(d=dict(mode=0), inputs_f=None), EINVAL, b"mode 0 needs teacher-forced inputs"),
    ("samples_without_draws", dict(d=dict(mode=0), u_mix=None, draws=None), EINVAL, b"samples need the draws"),
    ("no_output", dict(out_samples=None, out_params=None), EINVAL, b"no output requested"),
]


def _refused(call, name, case, code, text, **desc):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    case = dict(case)
    d = _desc(**dict(desc, **case.pop("d", {})))
    assert call(lib, d, **case) == code
    err = lib.wae_last_error()
    assert err.startswith(name + b": ") and text in err, err


def _cases(rows):
    return dict(argnames="case,code,text", argvalues=[r[1:] for r in rows], ids=[r[0] for r in rows])


@pytest.mark.parametrize(**_cases(CLASS_IDS + QUEUE + SLOTS_ONLY + FAULTS))
def test_slot_entry_refuses_before_any_launch(case, code, text):
    _refused(_call_slots, b"ar_generate_spans", case, code, text)


@pytest.mark.parametrize(**_cases(CLASS_IDS + QUEUE + TEAMS_ONLY + FAULTS))
def test_team_entry_refuses_before_any_launch(case, code, text):
    _refused(_call_teams, b"ar_generate_coop_spans", case, code, text)


@pytest.mark.parametrize(**_cases(SCALAR_ONLY + QUEUE + SLOTS_ONLY + FAULTS))
def test_scalar_entry_refuses_before_any_launch(case, code, text):
    _refused(_call_scalar, b"ar_generate_scalar_spans", case, code, text, scalar=1, O=30)


def test_sequence_bound_is_thirty_one_bits_and_the_descriptor_is_not_read_per_clip():
    """the largest list the bound admits is not refused for its size (a later check trips on purpose: nothing launches); d->B, d->T,
    d->n_forced and d->init_idx are not read"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _call_teams(lib, _desc(), total=357913941 - 4, ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()
    assert _call_teams(lib, _desc(), total=357913942 - 4, ring_total=1 << 31) == EINVAL
    assert b"sequence numbers" in lib.wae_last_error()
    assert _call_teams(lib, _desc(B=-3, T=-9, n_forced=77, init_idx=-5), ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()


def test_ring_floats_of_a_clip_on_the_teams():
    """one shared ring per clip where the launch takes the constant-size kernels, one per member on the any-shape kernel"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    ref = dict(R=256, G=256, S=256, O=256, Cc=64, Ccp=64, L=20)
    rt = 1052672
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc(dtype=1, **ref)), 32, rt) == rt
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc(dtype=0, **ref)), 32, rt) == rt
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc(dtype=1, coop_generic=1, **ref)), 32, rt) == 32 * rt
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc(dtype=1, **ref)), 16, rt) == 16 * rt
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc()), 8, 1000) == 8000
    assert lib.wae_ar_coop_ring_floats(ctypes.byref(_desc()), 0, 1000) < 0


# ---- packing.ar_round_plan -------------------------------------------------------------------------------------------------------------
def test_round_offsets_are_contiguous_in_the_callers_order():
    from wavenet_autoencoders_amd.packing import ar_round_plan
    rng = np.random.default_rng(3)
    rem = rng.integers(1, 5000, 37)
    pos = rng.integers(0, 9000, 37)
    p = ar_round_plan(rem, pos, 1600, 8)
    n = np.minimum(rem, 1600)
    assert p.clips.tolist() == list(range(37)) and np.array_equal(p.lengths, n) and np.array_equal(p.t0, pos)
    assert p.total == int(n.sum()) and p.offsets[0] == 0 and np.array_equal(p.offsets[1:], np.cumsum(n)[:-1])
    assert p.offsets.dtype == np.int64 and p.slots == 8


def test_round_order_is_longest_first_and_stable():
    from wavenet_autoencoders_amd.packing import ar_round_plan
    p = ar_round_plan([7, 9, 7, 9, 9, 3, 7], [0] * 7, 100, 2)
    assert p.order.tolist() == [1, 3, 4, 0, 2, 6, 5]
    p = ar_round_plan([5000] * 6, [0, 10, 20, 30, 40, 50], 160, 4)
    assert p.order.tolist() == list(range(6)) and p.lengths.tolist() == [160] * 6
    rng = np.random.default_rng(4)
    rem = rng.integers(1, 5000, 101)
    p = ar_round_plan(rem, np.zeros(101), 2000, 16)
    assert sorted(p.order.tolist()) == list(range(101)) and np.all(np.diff(p.lengths[p.order]) <= 0)


def test_round_gives_a_short_clip_what_is_left_and_leaves_finished_clips_out():
    from wavenet_autoencoders_amd.packing import ar_round_plan
    p = ar_round_plan([1500, 0, 37, 2300, 1, 0], [0, 37, 600, 1, 0, 9], 1024, 256)
    assert p.clips.tolist() == [0, 2, 3, 4] and p.lengths.tolist() == [1024, 37, 1024, 1] and p.t0.tolist() == [0, 600, 1, 0]
    assert p.offsets.tolist() == [0, 1024, 1061, 2085] and p.total == 2086
    assert p.order.tolist() == [0, 2, 1, 3] and p.slots == 4
    empty = ar_round_plan([0, 0], [5, 6], 7, 3)
    assert empty.total == 0 and empty.clips.size == 0 and empty.order.size == 0 and empty.slots == 1
    assert ar_round_plan([], [], 7, 3).total == 0


def test_round_honours_a_chunk_per_clip():
    from wavenet_autoencoders_amd.packing import ar_round_plan
    p = ar_round_plan([100, 100, 100, 5], [0, 0, 0, 0], {0: 10, 2: 300, 3: 7}, 8)
    assert p.clips.tolist() == [0, 2, 3] and p.lengths.tolist() == [10, 100, 5] and p.order.tolist() == [1, 0, 2]
    assert ar_round_plan([100, 100], [0, 0], {1: 0}, 8).total == 0
    for bad in (([3], [0, 1], 4, 1), ([3], [0], 0, 1), ([3], [0], 4, 0), ([3], [-1], 4, 1), ([3], [0], {1: 4}, 1)):
        with pytest.raises(ValueError):
            ar_round_plan(*bad)


# ---- the host --------------------------------------------------------------------------------------------------------------------------
CFG = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
           scalar_input=True, output_distribution="Logistic")


def test_decode_session_routes_and_refuses_without_a_device():
    """the routing checks come before anything that needs the engine's device state"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import DecodeSession, WaeEngine
    eng = object.__new__(WaeEngine)
    eng.g = Geometry.from_cfg(CFG)
    with pytest.raises(NotImplementedError, match="scalar-input decoders.*one-CU slots"):
        eng.decode_session(coop=True)
    for mode in ("argmax", "probs", "raw"):
        with pytest.raises(ValueError, match=f"mode '{mode}'"):
            eng.decode_session(mode=mode)
    assert isinstance(eng.decode_session(mode="logits"), DecodeSession)
    eng.g = Geometry.from_cfg(dict(CFG, O=32, scalar_input=False))
    for mode in ("probs", "raw"):
        for kw in (dict(), dict(coop=True)):
            with pytest.raises(ValueError, match=f"mode '{mode}'"):
                eng.decode_session(mode=mode, **kw)
    sess = eng.decode_session(mode="argmax", coop=True, teams=3)
    assert sess.live == [] and sess.step(7) == {}
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.step(7)
    with pytest.raises(RuntimeError, match="closed"):
        sess.add(dict(T=4, c=None, gid=0))
    eng.g = Geometry.from_cfg(dict(CFG, O=300, scalar_input=False))
    with pytest.raises(ValueError, match=r"R, S and O <= 256 \(got 32, 32, 300\)"):
        eng.decode_session(coop=True)
    with pytest.raises(ValueError, match="empty list"):
        eng.decode_list_stream([], 7)


def test_decode_session_surface():
    from wavenet_autoencoders_amd.engine import DecodeSession, WaeEngine
    sig = inspect.signature(WaeEngine.decode_session)
    assert list(sig.parameters)[:7] == ["self", "mode", "coop", "slots", "teams", "want_logits", "c_is_upsampled"]
    want = dict(mode="sample", coop=False, slots=None, teams=None, want_logits=False, c_is_upsampled=False)
    assert {k: sig.parameters[k].default for k in want} == want
    for name in ("add", "step", "drop", "close", "reserve", "__enter__", "__exit__"):
        assert callable(getattr(DecodeSession, name)), name
    assert list(inspect.signature(WaeEngine.decode_list_stream).parameters)[:3] == ["self", "items", "chunk"]
    for word in ("bit for bit", "NotImplementedError", "ar_path"):
        assert word in WaeEngine.decode_session.__doc__, word
    # the per-clip set-up and the round go through what every decode route shares (tests/test_decode_host_cpu.py checks that module's
    # structure): which functions of the module each method calls, read off its syntax tree
    import ast
    import textwrap
    from wavenet_autoencoders_amd import decode
    assert DecodeSession is decode.DecodeSession

    def calls(fn):
        tree = ast.parse(textwrap.dedent(inspect.getsource(fn)))
        return {ast.unparse(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)}
    assert {"clip_intake", "clip_draws", "_clip_cond", "eng._ar_speaker_rows", "self._open_device"} <= calls(DecodeSession.add)
    assert {"ar_desc", "team_width", "group_count", "mixture", "eng._ar_exchange"} <= calls(DecodeSession._open_device)
    assert {"P.ar_round_plan", "launch", "eng._ar_net_args", "_operands"} <= calls(DecodeSession.step)
    assert "refuse_wide" in calls(DecodeSession.__init__)
    for name in ("clip_intake", "clip_draws", "ar_desc", "team_width", "group_count", "mixture", "launch", "refuse_wide"):
        assert inspect.isfunction(getattr(decode, name)), name


# ---- synthesis.py ----------------------------------------------------------------------------------------------------------------------
POS = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]


@pytest.mark.parametrize("extra,word", [(["--batch-stream", "700"], "--batch-decode"),
                                        (["--batch-coop", "--batch-stream", "700"], "--batch-decode"),
                                        (["--batch-decode", "--batch-stream", "0"], "at least one sample"),
                                        (["--batch-decode", "--batch-stream", "-5"], "at least one sample"),
                                        (["--batch-decode", "--batch-stream", "700", "--stream-chunk", "700"], "--stream-chunk"),
                                        (["--batch-decode", "--stream-chunk", "700"], "--stream-chunk")],
                         ids=["stream_without_batch", "coop_stream_without_batch", "zero_round", "negative_round",
                              "batch_stream_with_stream_chunk", "batch_decode_with_stream_chunk_stays_refused"])
def test_synthesis_argument_errors(extra, word, capsys):
    sys.path.insert(0, ROOT)
    import synthesis
    with pytest.raises(SystemExit) as e:
        synthesis.main(POS + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_synthesis_streams_the_batch_through_decode_list_stream():
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    body = src[src.index("def batch_stream("):src.index("def main(")]
    assert "decode_list_stream(" in body and "ChunkPostprocess(" in body and "--batch-stream" in src
    assert "if args.batch_stream:" in src[src.index("def batch_decode("):src.index("def batch_stream(")]
