"""List decoding of scalar-input decoders (wae_ar_generate_scalar_list, wae_ar_generate_coop_scalar_list,
WaeEngine.decode_list_scalar, synthesis.py --batch-decode on a "raw" / "mulaw" model) without a GPU: the symbols and their
declarations, every refusal of the two entries before any launch (raw ctypes calls with dummy pointers, as tests/test_ar_list_cpu.py),
the four broken-network faults of tests/test_ar_entries_cpu.py, and the host-side refusals."""
import ctypes
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2
ONE_CU, TEAMS = "wae_ar_generate_scalar_list", "wae_ar_generate_coop_scalar_list"


# ---- the symbols -----------------------------------------------------------------------------------------------------------------------
def _args(entry):
    from wavenet_autoencoders_amd import _lib
    D, vp, i32, i64, f32 = ctypes.POINTER(_lib.ArDesc), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    # dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes, bias2, zb, first_tab, first_bias, w_head,
    # head_bias, c_up, c_dtype
    net = [vp, vp, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, i32]
    # inputs_f, u_mix, draws, log_scale_min, clamp_log_scale, out_samples, out_params
    draw = [vp, vp, vp, f32, i32, vp, vp]
    if entry == ONE_CU:      # d, dist, n_items, n_slots, items, next | net | draw | stream
        return [D, i32, i32, i32, vp, vp] + net + draw + [vp]
    # d, C, dist, n_items, n_teams, items, next, total | net | draw | msg, acc, error, stream
    return [D, i32, i32, i32, i32, vp, vp, i64] + net + draw + [vp, vp, vp, vp]


@pytest.mark.parametrize("entry", [ONE_CU, TEAMS])
def test_entries_are_exported_declared_and_bound(entry):
    from wavenet_autoencoders_amd import _lib
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {entry}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {entry}("):]
    decl = decl[:decl.index(";")]
    args = _args(entry)
    res, bound = _lib.SIGNATURES[entry]
    assert res is ctypes.c_int32 and list(bound) == args
    assert list(getattr(_lib.lib(), entry).argtypes) == args
    assert len(args) == decl.count(",") + 1
    words = ["int32_t dist", "int32_t n_items", "const wae_ar_item* items", "int32_t* next", "const float* inputs_f", "const float* u_mix",
             "const float* draws", "float log_scale_min", "int32_t clamp_log_scale", "float* out_samples", "float* out_params"]
    words += ["int32_t n_slots"] if entry == ONE_CU else ["int32_t C", "int32_t n_teams", "int64_t total", "uint64_t* msg", "float* acc",
                                                          "int32_t* error"]
    for word in words:
        assert word in decl, word
    # the contract is stated next to the declarations: reference lines, layouts, refusals
    comment = hdr[:hdr.index(f"int {ONE_CU}(")]
    comment = comment[comment.rindex("/*"):]
    for word in ("wavenet.py:284-285", "mixture.py:118-156", "225-270", "bit for bit", "off * O", "(total, M)", "item.row",
                 "item.init_idx is not read", "d->mode", "WAE_EINVAL", "zeroes msg, acc, error and next", "error[0]", "2^31"):
        assert word in comment, word


# ---- refusals of the entries, before any launch ----------------------------------------------------------------------------------------
def _desc(scalar=1, O=30, mode=2, **kw):
    from wavenet_autoencoders_amd import _lib
    #             dtype B  T  L  R   Rp   G   Hp  S   O  Cc Ccp k  mode init scalar scale n_forced
    d = _lib.ArDesc(0, 1, 8, 2, 32, 128, 48, 32, 32, O, 0, 0, 3, mode, 0, scalar, 0.5, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _net(w_layers=P, c_up=None, ring_total=4):
    return [P, P, P, ring_total, w_layers, 1, 1, P, P, P, P, P, P, c_up, 0]


def _call_one(lib, d, dist=0, n_items=3, n_slots=2, items=P, nxt=P, inputs_f=P, u_mix=P, draws=P, out_samples=P, out_params=P, **net):
    return lib.wae_ar_generate_scalar_list(ctypes.byref(d), dist, n_items, n_slots, items, nxt, *_net(**net), inputs_f, u_mix, draws, -7.0, 0,
                                           out_samples, out_params, None)


def _call_teams(lib, d, C=8, dist=0, n_items=3, n_teams=2, items=P, nxt=P, total=24, inputs_f=P, u_mix=P, draws=P, out_samples=P,
                out_params=P, msg=P, acc=P, error=P, **net):
    return lib.wae_ar_generate_coop_scalar_list(ctypes.byref(d), C, dist, n_items, n_teams, items, nxt, total, *_net(**net), inputs_f, u_mix,
                                                draws, -7.0, 0, out_samples, out_params, msg, acc, error, None)


# what both entries refuse (include/wae.h); `slots` stands for n_slots / n_teams
SHARED = [
    ("class_id_decoder", dict(d=dict(scalar=0, O=32)), b"needs a scalar-input decoder"),
    ("mode1", dict(d=dict(mode=1)), b"mode must be 0 (teacher-forced parameters) or 2 (sample)"),
    ("mode3", dict(d=dict(mode=3)), b"mode must be 0"),
    ("mode_negative", dict(d=dict(mode=-1)), b"mode must be 0"),
    ("dist2", dict(dist=2), b"dist must be 0"),
    ("dist_negative", dict(dist=-1), b"dist must be 0"),
    ("logistic_O_not_3M", dict(d=dict(O=31)), b"3M output channels (got 31)"),
    ("logistic_O_2", dict(d=dict(O=2)), b"3M output channels (got 2)"),
    ("gaussian_O_4", dict(dist=1, d=dict(O=4)), b"2 or 3M output channels (got 4)"),
    ("sample_without_draws", dict(u_mix=None, draws=None, out_samples=None), b"sample mode needs its draws (u_mix and u_log)"),
    ("gaussian_sample_without_z", dict(dist=1, draws=None, out_samples=None), b"sample mode needs its draws (z)"),
    ("u_mix_without_u_log", dict(draws=None), b"u_mix and u_log come together"),
    ("u_log_without_u_mix", dict(u_mix=None), b"u_mix and u_log come together"),
    ("ten_gaussians_without_u_mix", dict(dist=1, u_mix=None), b"10 mixtures need the uniforms u_mix"),
    ("mode0_without_inputs_f", dict(d=dict(mode=0), inputs_f=None), b"mode 0 needs teacher-forced inputs"),
    ("samples_without_draws", dict(d=dict(mode=0), u_mix=None, draws=None), b"samples need the draws"),
    ("no_output", dict(out_samples=None, out_params=None), b"no output requested"),
    ("t0", dict(d=dict(t0=5)), b"t0 5"),
    ("t0_negative", dict(d=dict(t0=-1)), b"t0 -1"),
    ("no_items", dict(n_items=0), b"n_items 0 < 1"),
    ("negative_items", dict(n_items=-2), b"n_items -2 < 1"),
    ("null_items", dict(items=None), b"item array"),
    ("null_next", dict(nxt=None), b"queue counter"),
]
ONE_ONLY = [("no_slots", dict(n_slots=0), b"n_slots 0 < 1"), ("negative_slots", dict(n_slots=-1), b"n_slots -1 < 1")]
TEAMS_ONLY = [
    ("no_teams", dict(n_teams=0), b"n_teams 0 outside 1..8"),
    ("nine_teams", dict(n_teams=9), b"n_teams 9 outside 1..8"),
    ("no_members", dict(C=0), b"C 0 outside 1..32"),
    ("too_many_members", dict(C=33), b"C 33 outside 1..32"),
    ("wide_R", dict(d=dict(R=257)), b"R, S and O <= 256"),
    ("wide_S", dict(d=dict(S=320)), b"R, S and O <= 256"),
    ("wide_O", dict(d=dict(O=300)), b"R, S and O <= 256"),
    ("null_msg", dict(msg=None), b"msg, acc and error"),
    ("null_acc", dict(acc=None), b"msg, acc and error"),
    ("null_error", dict(error=None), b"msg, acc and error"),
    # (total + n_items + 1) * (L + 4) must stay below 2^31: L = 2 -> 357 913 942 is the first total + n_items + 1 that does not
    ("sequence_overflow", dict(total=357913942 - 4), b"sequence numbers would not fit 31 bits"),
    ("sequence_overflow_far", dict(total=1 << 40), b"sequence numbers would not fit 31 bits"),
    ("negative_total", dict(total=-1), b"sequence numbers would not fit 31 bits"),
]
# the four broken networks of tests/test_ar_entries_cpu.py
FAULTS = [
    ("null_w_layers", dict(w_layers=None), b"null pointer"),
    ("dtype_7", dict(d=dict(dtype=7)), b"bad dtype"),
    ("odd_G", dict(d=dict(G=47)), b"bad sizes"),
    ("Cc_without_c_up", dict(d=dict(Cc=4, Ccp=4), c_up=None), b"c_up is null"),
]


def _refused(call, name, case, text, code=EINVAL):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    case = dict(case)
    d = _desc(**case.pop("d", {}))
    assert call(lib, d, **case) == code
    err = lib.wae_last_error()
    assert err.startswith(name + b": ") and text in err, err


@pytest.mark.parametrize("case,text", [r[1:] for r in SHARED + ONE_ONLY + FAULTS], ids=[r[0] for r in SHARED + ONE_ONLY + FAULTS])
def test_one_cu_entry_refuses_before_any_launch(case, text):
    _refused(_call_one, b"ar_generate_scalar_list", case, text)


@pytest.mark.parametrize("case,text", [r[1:] for r in SHARED + TEAMS_ONLY + FAULTS], ids=[r[0] for r in SHARED + TEAMS_ONLY + FAULTS])
def test_team_entry_refuses_before_any_launch(case, text):
    _refused(_call_teams, b"ar_generate_coop_scalar_list", case, text)


def test_what_the_entries_do_not_read_or_do_allow():
    """d->B, d->T, d->n_forced and d->init_idx are not read (nonsense there trips nothing); a single Gaussian needs no u_mix, O == 2
    is a Gaussian geometry, mode 0 may come without draws.  Every call is still refused -- by a LATER check this test trips on
    purpose (a ring_total beyond 32-bit offsets on the team entry, t0 on the one-CU entry), so nothing launches."""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    for kw in (dict(d=dict(B=-3, T=-9, n_forced=77, init_idx=-5)), dict(dist=1, d=dict(O=3), u_mix=None), dict(dist=1, d=dict(O=2), u_mix=None),
               dict(d=dict(mode=0), u_mix=None, draws=None, out_samples=None), dict(d=dict(mode=2), inputs_f=None)):
        kw = dict(kw)
        fields = kw.pop("d", {})
        assert _call_teams(lib, _desc(**fields), ring_total=1 << 31, **kw) == EINVAL
        assert b"ring_total" in lib.wae_last_error(), lib.wae_last_error()
        assert _call_one(lib, _desc(t0=1, **fields), **kw) == EINVAL
        assert b"t0 1" in lib.wae_last_error(), lib.wae_last_error()


def test_sequence_bound_is_thirty_one_bits():
    """as tests/test_ar_team_list_cpu.py: the largest list the bound admits is not refused for its size"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _call_teams(lib, _desc(), total=357913941 - 4, ring_total=1 << 31) == EINVAL
    assert b"ring_total" in lib.wae_last_error()
    assert _call_teams(lib, _desc(), total=357913942 - 4, ring_total=1 << 31) == EINVAL
    assert b"sequence numbers" in lib.wae_last_error()


def test_class_id_list_entries_name_the_scalar_entries():
    import test_ar_list_cpu as one_cu_list
    import test_ar_team_list_cpu as team_list
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert one_cu_list._call(lib, one_cu_list._desc(scalar=1, O=30)) == EUNSUPPORTED
    assert b"class-id decoders" in lib.wae_last_error() and b"wae_ar_generate_scalar_list" in lib.wae_last_error()
    assert team_list._call(lib, team_list._desc(scalar=1, O=30)) == EUNSUPPORTED
    assert b"class-id decoders" in lib.wae_last_error() and b"wae_ar_generate_coop_scalar_list" in lib.wae_last_error()


# ---- the host --------------------------------------------------------------------------------------------------------------------------
CFG = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
           scalar_input=True, output_distribution="Logistic")


def test_decode_list_scalar_refuses_without_a_device():
    """the checks come before anything that needs the engine's device state: an engine object that never saw a GPU is enough"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = object.__new__(WaeEngine)
    one = [dict(c=None, gid=0, T=8)]
    eng.g = Geometry.from_cfg(dict(CFG, O=32, scalar_input=False))
    for kw in (dict(), dict(coop=True)):
        with pytest.raises(ValueError, match="decode_list_scalar: scalar-input decoders only.*decode_list"):
            eng.decode_list_scalar(one, **kw)
    eng.g = Geometry.from_cfg(CFG)
    for kw in (dict(), dict(coop=True)):
        with pytest.raises(ValueError, match="empty list"):
            eng.decode_list_scalar([], **kw)
        with pytest.raises(ValueError, match="mode 'argmax'"):
            eng.decode_list_scalar(one, mode="argmax", **kw)
    eng.g = Geometry.from_cfg(dict(CFG, O=300))
    with pytest.raises(ValueError, match=r"R, S and O <= 256 \(got 32, 32, 300\)"):
        eng.decode_list_scalar(one, coop=True)
    # decode_list keeps refusing scalar geometries, and says where they go
    eng.g = Geometry.from_cfg(CFG)
    with pytest.raises(NotImplementedError, match="class-id decoders.*decode_list_scalar"):
        eng.decode_list(one)


def test_decode_list_scalar_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.decode_list_scalar)
    assert list(sig.parameters) == ["self", "items", "mode", "slots", "want_logits", "c_is_upsampled", "coop", "teams", "log_scale_min",
                                    "clamp_log_scale"]
    want = dict(mode="sample", slots=None, want_logits=False, c_is_upsampled=False, coop=False, teams=None, log_scale_min=-7.0,
                clamp_log_scale=False)
    assert {k: sig.parameters[k].default for k in want} == want
    doc = WaeEngine.decode_list_scalar.__doc__
    for word in ("test_inputs", "u_mix", "u_log", "bit for bit", "torch.manual_seed", "scalar_coop"):
        assert word in doc, word
    # both lists are ONE function behind their own refusals (tests/test_decode_host_cpu.py checks the structure of that module)
    import ast
    import textwrap
    for fn in (WaeEngine.decode_list, WaeEngine.decode_list_scalar):
        ret = ast.parse(textwrap.dedent(inspect.getsource(fn))).body[0].body[-1]
        assert isinstance(ret, ast.Return) and ast.unparse(ret.value.func) == "D.decode_list", fn.__name__
        # nothing but refusals in front of it: no assignment reads an item, no loop, no launch
        assert not any(isinstance(n, (ast.For, ast.While, ast.ListComp)) for n in ast.walk(ast.parse(textwrap.dedent(inspect.getsource(fn)))))


def test_synthesis_routes_scalar_models_to_the_scalar_list():
    src = open(os.path.join(ROOT, "synthesis.py")).read()
    body = src[src.index("def batch_decode("):src.index("def main(")]
    assert "eng.g.scalar_input" in body and "decode_list_scalar(" in body and "eng.decode_list(" in body
    assert "scalar_draws(" in body and "how = dict(coop=True, teams=args.batch_teams)" in body
    assert body.index("scalar_input") < body.index("decode_list_scalar(")
