"""The work list on cooperative teams (wae_ar_generate_coop_list, WaeEngine.decode_list(coop=True), synthesis.py --batch-coop) without a
GPU: the symbol and its declaration, every refusal of the entry before any launch (raw ctypes calls with dummy pointers, as
tests/test_ar_list_cpu.py), and the host-side refusals."""
import ctypes
import inspect
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2


def test_entry_is_exported_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T wae_ar_generate_coop_list\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index("int wae_ar_generate_coop_list("):]
    decl = decl[:decl.index(";")]
    D, vp, i32, i64 = ctypes.POINTER(_lib.ArDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    # d, C, n_items, n_teams, items, next, total, dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes,
    # bias2, zb, first_tab, first_bias, w_head, head_bias, c_up, c_dtype, inputs, uniforms, out_idx, out_logits, msg, acc, error, stream
    args = [D, i32, i32, i32, vp, vp, i64, vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    res, bound = _lib.SIGNATURES["wae_ar_generate_coop_list"]
    assert res is i32 and list(bound) == args
    assert list(_lib.lib().wae_ar_generate_coop_list.argtypes) == args
    assert len(args) == decl.count(",") + 1
    for word in ("int32_t C", "int32_t n_items", "int32_t n_teams", "const wae_ar_item* items", "int32_t* next", "int64_t total",
                 "uint64_t* msg", "float* acc", "int32_t* error"):
        assert word in decl, word
    # the contract is stated next to the declaration
    comment = hdr[:hdr.index("int wae_ar_generate_coop_list(")]
    comment = comment[comment.rindex("/*"):]
    for word in ("n_teams", "bit for bit", "zeroes msg, acc, error and next", "WAE_EUNSUPPORTED", "WAE_EINVAL", "error[0]"):
        assert word in comment, word


def _desc(scalar=0, O=32, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(lib, d, C=8, n_items=3, n_teams=2, items=P, nxt=P, total=24, inputs=P, uniforms=P, msg=P, acc=P, error=P, ring_total=4):
    return lib.wae_ar_generate_coop_list(ctypes.byref(d), C, n_items, n_teams, items, nxt, total, P, P, P, ring_total, P, 1, 1, P, P, P, P, P, P,
                                         None, 0, inputs, uniforms, P, P, msg, acc, error, None)


@pytest.mark.parametrize("case,code,text", [
    (dict(d=dict(scalar=1, O=30)), EUNSUPPORTED, b"class-id decoders"),
    (dict(d=dict(mode=3)), EUNSUPPORTED, b"modes 3 / 4"),
    (dict(d=dict(mode=4)), EUNSUPPORTED, b"modes 3 / 4"),
    (dict(d=dict(t0=5)), EINVAL, b"t0 5"),
    (dict(d=dict(t0=-1)), EINVAL, b"t0 -1"),
    (dict(n_items=0), EINVAL, b"n_items 0 < 1"),
    (dict(n_items=-2), EINVAL, b"n_items -2 < 1"),
    (dict(n_teams=0), EINVAL, b"n_teams 0 outside 1..8"),
    (dict(n_teams=9), EINVAL, b"n_teams 9 outside 1..8"),
    (dict(C=0), EINVAL, b"C 0 outside 1..32"),
    (dict(C=33), EINVAL, b"C 33 outside 1..32"),
    (dict(d=dict(R=257)), EINVAL, b"R, S and O <= 256"),
    (dict(d=dict(S=320)), EINVAL, b"R, S and O <= 256"),
    (dict(d=dict(O=512)), EINVAL, b"R, S and O <= 256"),
    (dict(items=None), EINVAL, b"item array"),
    (dict(nxt=None), EINVAL, b"queue counter"),
    (dict(msg=None), EINVAL, b"msg, acc and error"),
    (dict(acc=None), EINVAL, b"msg, acc and error"),
    (dict(error=None), EINVAL, b"msg, acc and error"),
    (dict(d=dict(mode=0), inputs=None), EINVAL, b"mode 0 needs inputs"),
    (dict(d=dict(mode=2), uniforms=None), EINVAL, b"sample mode needs uniforms"),
    # (total + n_items + 1) * (L + 4) must stay below 2^31: L = 2 -> 357 913 942 is the first total + n_items + 1 that does not
    (dict(total=357913942 - 4), EINVAL, b"sequence numbers would not fit 31 bits"),
    (dict(total=1 << 40), EINVAL, b"sequence numbers would not fit 31 bits"),
    (dict(total=-1), EINVAL, b"sequence numbers would not fit 31 bits"),
], ids=["scalar_input", "mode3", "mode4", "t0", "t0_negative", "no_items", "negative_items", "no_teams", "nine_teams", "no_members",
        "too_many_members", "wide_R", "wide_S", "wide_O", "null_items", "null_next", "null_msg", "null_acc", "null_error",
        "mode0_without_inputs", "mode2_without_uniforms", "sequence_overflow", "sequence_overflow_far", "negative_total"])
def test_entry_refuses_before_any_launch(case, code, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    case = dict(case)
    d = _desc(**case.pop("d", {}))
    assert _call(lib, d, **case) == code
    err = lib.wae_last_error()
    assert b"ar_generate_coop_list" in err and text in err, err


def test_sequence_bound_is_thirty_one_bits():
    """the largest list the bound admits is not refused FOR ITS SIZE: with total + n_items + 1 = 357 913 941 on two layers the product
    with L + 4 is 2 147 483 646 < 2^31; the call is then refused by a LATER check this test trips on purpose (no launch either way)"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _call(lib, _desc(), total=357913941 - 4, ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()
    assert _call(lib, _desc(), total=357913942 - 4, ring_total=1 << 31) == EINVAL
    assert b"sequence numbers" in lib.wae_last_error()


def test_decode_list_coop_refuses_scalar_and_wide_geometries_without_a_device():
    """the checks come before anything that needs the engine's device state: an engine object that never saw a GPU is enough"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
               scalar_input=True, output_distribution="Logistic")
    eng = object.__new__(WaeEngine)
    eng.g = Geometry.from_cfg(cfg)
    with pytest.raises(NotImplementedError, match="class-id decoders"):
        eng.decode_list([dict(c=None, gid=0, T=8)], coop=True)
    for wide in (dict(R=512), dict(S=320), dict(O=1024)):
        eng.g = Geometry.from_cfg(dict(dict(cfg, O=32, scalar_input=False), **wide))
        with pytest.raises(ValueError, match="R, S and O <= 256"):
            eng.decode_list([dict(c=None, gid=0, T=8)], coop=True)
    eng.g = Geometry.from_cfg(dict(cfg, O=32, scalar_input=False))
    with pytest.raises(ValueError, match="empty list"):
        eng.decode_list([], coop=True)
    with pytest.raises(ValueError, match="mode 'probs'"):
        eng.decode_list([dict(c=None, gid=0, T=8)], mode="probs", coop=True, teams=2)


def test_decode_list_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.decode_list)
    assert list(sig.parameters)[:5] == ["self", "items", "mode", "slots", "want_logits"]      # the earlier arguments keep their places
    assert sig.parameters["coop"].default is False and sig.parameters["teams"].default is None
    doc = WaeEngine.decode_list.__doc__
    assert "coop=True" in doc and "bit for bit" in doc and "WAE_AR_COOP=1" in doc and "one_handover is ignored" in doc


@pytest.mark.parametrize("extra,word", [(["--batch-coop"], "--batch-decode"), (["--batch-teams", "2"], "--batch-decode"),
                                        (["--batch-decode", "--batch-coop", "--stream-chunk", "700"], "--stream-chunk"),
                                        (["--batch-decode", "--batch-teams", "2"], "--batch-coop")],
                         ids=["coop_without_batch", "teams_without_batch", "coop_with_stream_chunk", "teams_without_coop"])
def test_synthesis_refuses_batch_coop_where_it_cannot_apply(extra, word, capsys):
    sys.path.insert(0, ROOT)
    import synthesis
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    assert "--batch-coop" in src and "coop=True" in src
    pos = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]
    with pytest.raises(SystemExit) as e:
        synthesis.main(pos + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err
