"""The decode host path (wavenet_autoencoders_amd/decode.py) without a GPU: its structure, read off the two sources with `ast` (one
descriptor constructor, one launch table); the descriptor of every route on a device-less engine; every key of the launch table
against the bound argument types; the per-item intake (clip_intake) on device="cpu"."""
import ast
import ctypes
import itertools
import os

import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavenet_autoencoders_amd")
PREFIX = "wae_ar_generate"
CFG = dict(layers=4, stacks=2, R=32, G=32, S=32, O=30, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=None, cin_pad=0,
           scalar_input=True, output_distribution="Logistic")
CLASS = dict(CFG, O=32, scalar_input=False)
CALLERS = ("decode_list", "decode_list_scalar", "decode_session.add")


def _tree(rel):
    with open(os.path.join(PKG, rel)) as f:
        return ast.parse(f.read(), rel)


def _inside(tree, pick):
    """the nodes below the top-level nodes that `pick` selects, and the nodes of the rest of the module"""
    inner = [n for top in tree.body if pick(top) for n in ast.walk(top)]
    ids = {id(n) for n in inner}
    return inner, [n for n in ast.walk(tree) if id(n) not in ids]


def _entry_names(nodes):
    return ([n.value for n in nodes if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value.startswith(PREFIX)]
            + [n.attr for n in nodes if isinstance(n, ast.Attribute) and n.attr.startswith(PREFIX)])


def _is_call_of(n, name):
    return isinstance(n, ast.Call) and (getattr(n.func, "id", None) == name or getattr(n.func, "attr", None) == name)


def _assigns(n, attr):
    targets = n.targets if isinstance(n, ast.Assign) else [n.target] if isinstance(n, (ast.AugAssign, ast.AnnAssign)) else []
    return any(isinstance(t, ast.Attribute) and t.attr == attr for top in targets for t in ast.walk(top))


# ---- structure -----------------------------------------------------------------------------------------------------------------------------
def test_one_descriptor_constructor():
    dec, eng = _tree("decode.py"), _tree("engine.py")
    in_desc, rest = _inside(dec, lambda n: isinstance(n, ast.FunctionDef) and n.name == "ar_desc")
    assert sum(_is_call_of(n, "ArDesc") for n in in_desc) == 1
    assert sum(_is_call_of(n, "_ar_scalar_path") for n in in_desc) == 1 and sum(_assigns(n, "scalar_sized") for n in in_desc) == 1
    for n in rest + list(ast.walk(eng)):
        assert not _is_call_of(n, "ArDesc") and not _is_call_of(n, "_ar_scalar_path") and not _assigns(n, "scalar_sized"), n.lineno


def test_entry_names_live_in_the_launch_table_only():
    assert _entry_names(ast.walk(_tree("engine.py"))) == []
    table, rest = _inside(_tree("decode.py"), lambda n: isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "ENTRIES")
    assert len(_entry_names(table)) == 13 and _entry_names(rest) == []


def test_decode_does_not_import_the_engine():
    for n in ast.walk(_tree("decode.py")):
        if isinstance(n, ast.ImportFrom):
            assert n.module != "engine" and all(a.name != "engine" for a in n.names), n.lineno
        if isinstance(n, ast.Import):
            assert all("engine" not in a.name for a in n.names), n.lineno
    from wavenet_autoencoders_amd import decode, engine
    assert engine.DecodeSession is decode.DecodeSession


def test_the_walkers_see_what_they_look_for():
    src = ("ENTRIES = {1: 'wae_ar_generate_x'}\n"
           "def ar_desc(eng):\n    d = L.ArDesc(1)\n    d.scalar_sized = eng._ar_scalar_path()\n    return d\n"
           "def f(eng, d):\n    d.scalar_sized = 1\n    eng.lib.wae_ar_generate_y(L.ArDesc(2), eng._ar_scalar_path(), 'see wae_ar_generate_z')\n")
    tree = ast.parse(src)
    _, rest = _inside(tree, lambda n: isinstance(n, ast.FunctionDef) and n.name == "ar_desc")
    assert sum(_is_call_of(n, "ArDesc") for n in rest) == 1 and sum(_is_call_of(n, "_ar_scalar_path") for n in rest) == 1
    assert sum(_assigns(n, "scalar_sized") for n in rest) == 1
    table, rest = _inside(tree, lambda n: isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "ENTRIES")
    assert _entry_names(table) == ["wae_ar_generate_x"] and _entry_names(rest) == ["wae_ar_generate_y"]


# ---- the descriptor ------------------------------------------------------------------------------------------------------------------------
def _engine(cfg, **path):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = object.__new__(WaeEngine)
    eng.g, eng.dt, eng.ar_one_handover = Geometry.from_cfg(cfg), 1, False
    return eng.ar_path(**path)


@pytest.mark.parametrize("cfg", [CFG, CLASS], ids=["scalar", "class_id"])
@pytest.mark.parametrize("coop,fast", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("path", [dict(), dict(generic=True), dict(lds_layers=2), dict(reg_layers=0), dict(generic=True, lds_layers=3, reg_layers=5)],
                         ids=["default", "generic", "lds", "regs", "all"])
def test_ar_desc_of_every_route(cfg, coop, fast, path):
    from wavenet_autoencoders_amd import decode
    eng = _engine(cfg, scalar_coop=True, scalar_fast=fast, **path)
    g, scalar = eng.g, cfg["scalar_input"]
    d = decode.ar_desc(eng, B=3, T=9, mode=2, init_idx=5, n_forced=4, coop=coop)
    assert (d.dtype, d.B, d.T, d.L, d.R, d.Rp, d.G, d.Hp, d.S, d.O, d.Cc, d.Ccp, d.ktaps) == (1, 3, 9, 4, 32, g.Rp, 32, g.Hp, 32, g.O, 16, g.Ccp, 3)
    assert (d.mode, d.init_idx, d.n_forced, d.t0) == (2, 5, 4, 0) and d.scale == pytest.approx(0.5)
    own = (int(eng.ar_generic), eng.ar_resident[0], eng.ar_resident[1])
    assert own == (int(path.get("generic", False)), path.get("lds_layers", 0), {None: 0, 0: -1, 5: 5}[path.get("reg_layers")])
    sized = bool(scalar and coop and fast)
    assert d.scalar_input == (2 if sized else int(scalar)) and d.scalar_sized == int(sized)
    triple = (d.coop_generic, d.resident_lds, d.resident_regs)
    if scalar:
        assert triple == (own if sized else (0, 0, 0))
    else:
        assert triple == (own if coop else (0, 0, 0))


# ---- the launch table ----------------------------------------------------------------------------------------------------------------------
def _keys():
    from wavenet_autoencoders_amd import decode
    return sorted(decode.ENTRIES, key=str)


def test_launch_table_is_the_entries_the_host_calls():
    from wavenet_autoencoders_amd import _lib, decode
    assert set(k[0] for k in decode.ENTRIES) == {"batch", "list", "spans"}
    plain = {k for k in decode.ENTRIES if k[1] in (False, True)}
    assert plain == set(itertools.product(("batch", "list", "spans"), (False, True), (False, True)))        # the twelve (form, scalar, coop)
    assert set(decode.ENTRIES) - plain == {("batch", "normal", False)}      # and the one-CU batch entry of "Normal" geometries
    names = list(decode.ENTRIES.values())
    assert len(set(names)) == len(names) == 13 and all(n in _lib.SIGNATURES for n in names)
    # every bound launch entry but the two-hand-over batch kernel's own (the host reaches it through wae_ar_generate_coop_fused)
    assert set(names) == {n for n in _lib.SIGNATURES if n.startswith(PREFIX)} - {"wae_ar_generate_coop"}
    assert decode.ENTRIES[("batch", "normal", False)] == "wae_ar_generate_scalar_mog"
    for (form, scalar, coop), name in decode.ENTRIES.items():
        assert ("coop" in name) == coop and ("scalar" in name) == bool(scalar) and (form in name) == (form != "batch"), name


def _dummies(key):
    """one value of its own per argument: pointers 0x1000 apart, so that a swap of any two shows"""
    from wavenet_autoencoders_amd import _lib
    vp = lambda k: ctypes.c_void_p(0x1000 * (k + 1))  # noqa: E731
    net = (vp(0), vp(1), vp(2), 1 << 33, vp(3), 1 << 34, 1 << 35) + tuple(vp(k) for k in range(4, 11)) + (1,)
    operands = (vp(11), vp(12), vp(13), -7.0, 9, vp(14), vp(15)) if key[1] else (vp(11), vp(12), vp(13), vp(14))
    return dict(d=_lib.ArDesc(), net=net, operands=operands, stream=vp(30), C=32, dist=7, queue=(5, 2, vp(20), vp(21)), total=1 << 36,
                exchange=(vp(22), vp(23), vp(24)), w_fused=vp(25))


def _same(a, b):
    return a.value == b.value if isinstance(a, ctypes.c_void_p) and isinstance(b, ctypes.c_void_p) else (a is b or a == b)


@pytest.mark.parametrize("key", _keys(), ids=lambda k: "-".join(map(str, k)))
def test_composed_arguments_fit_the_bound_signature(key):
    from wavenet_autoencoders_amd import _lib, decode
    v = _dummies(key)
    args = decode.ar_args(key, v["d"], v["net"], v["operands"], v["stream"], C=v["C"], dist=v["dist"], queue=v["queue"], total=v["total"],
                          exchange=v["exchange"], w_fused=v["w_fused"])
    argtypes = _lib.SIGNATURES[decode.ENTRIES[key]][1]
    assert len(args) == len(argtypes)
    for i, (a, t) in enumerate(zip(args, argtypes)):
        t.from_param(a)                                             # raises where the position takes another type
        assert (t is ctypes.c_void_p) == isinstance(a, ctypes.c_void_p), (i, a, t)      # pointers in pointer positions only
        assert (t is ctypes.c_float) == isinstance(a, float), (i, a, t)
    # no pointer twice, and the order of the groups: network arguments, operands, exchange (w_fused), stream
    ptrs = [a.value for a in args if isinstance(a, ctypes.c_void_p)]
    assert len(set(ptrs)) == len(ptrs)
    tail = [p for p in ptrs if p not in (0x1000 * 21, 0x1000 * 22)]         # (the queue's two pointers stand in front of the network's)
    assert tail == sorted(tail) and tail[-1] == 0x1000 * 31
    # the 64-bit positions hold what was passed as 64-bit values: nothing was shifted by one
    wide = [a for a, t in zip(args, argtypes) if t is ctypes.c_int64]
    assert wide == ([1 << 36] if key[2] and key[0] != "batch" else []) + [1 << 33, 1 << 34, 1 << 35]
    small = [a for a, t in zip(args, argtypes) if t is ctypes.c_int32]
    head = ([32] if key[2] else []) + ([7] if key[1] and (key[2] or key[0] != "batch") else []) + ([5, 2] if key[0] != "batch" else [])
    assert small == head + [1] + ([9] if key[1] is True else [])       # C, dist, (n, groups); c_dtype; the clamp


def test_composed_arguments_spelled_out():
    """the whole tuple of one entry per form (and of the entry without a clamp), written out by hand from include/wae.h"""
    from wavenet_autoencoders_amd import decode

    def check(key, want):
        v = _dummies(key)
        got = decode.ar_args(key, v["d"], v["net"], v["operands"], v["stream"], C=v["C"], dist=v["dist"], queue=v["queue"],
                             total=v["total"], exchange=v["exchange"], w_fused=v["w_fused"])
        want = want(v)
        assert ctypes.addressof(got[0]._obj) == ctypes.addressof(v["d"]) and len(got) == 1 + len(want)
        assert all(_same(a, b) for a, b in zip(got[1:], want)), (key, got, want)
    # wae_ar_generate_coop_fused(d, C, <net>, inputs, uniforms, out_idx, out_logits, msg, acc, error, w_fused, stream)
    check(("batch", False, True), lambda v: (v["C"],) + v["net"] + v["operands"] + v["exchange"] + (v["w_fused"], v["stream"]))
    # wae_ar_generate_scalar_mog(d, <net>, inputs_f, u_mix, z, log_scale_min, out_samples, out_params, stream): no clamp, no dist
    check(("batch", "normal", False), lambda v: v["net"] + v["operands"][:4] + v["operands"][5:] + (v["stream"],))
    # wae_ar_generate_coop_scalar(d, C, dist, <net>, inputs_f, u_mix, draws, log_scale_min, clamp, out_samples, out_params, msg, acc, error, stream)
    check(("batch", True, True), lambda v: (v["C"], v["dist"]) + v["net"] + v["operands"] + v["exchange"] + (v["stream"],))
    # wae_ar_generate_scalar_list(d, dist, n_items, n_slots, items, next, <net>, <scalar operands>, stream)
    check(("list", True, False), lambda v: (v["dist"],) + v["queue"] + v["net"] + v["operands"] + (v["stream"],))
    # wae_ar_generate_coop_spans(d, C, n_spans, n_teams, spans, next, total, <net>, inputs, uniforms, out_idx, out_logits, msg, acc, error, stream)
    check(("spans", False, True), lambda v: (v["C"],) + v["queue"] + (v["total"],) + v["net"] + v["operands"] + v["exchange"] + (v["stream"],))
    # wae_ar_generate_coop_scalar_spans(d, C, dist, n_spans, n_teams, spans, next, total, <net>, <scalar operands>, msg, acc, error, stream)
    check(("spans", True, True), lambda v: (v["C"], v["dist"]) + v["queue"] + (v["total"],) + v["net"] + v["operands"] + v["exchange"] + (v["stream"],))


# ---- the intake ----------------------------------------------------------------------------------------------------------------------------
def _g(cfg=CFG, **kw):
    from wavenet_autoencoders_amd import Geometry
    return Geometry.from_cfg(dict(cfg, **kw))


def _intake(g, mode, item, who="decode_list", index=None, **kw):
    from wavenet_autoencoders_amd import decode
    return decode.clip_intake(g, "cpu", mode, dict(dict(T=6, c=torch.zeros(16, 6), gid=1), **item), who, index, **kw)


U6 = torch.full((6,), 0.5)
REFUSALS = [
    # (geometry, mode, item, exception, words)
    ("no_steps", CFG, 2, dict(T=0), ValueError, "at least one step"),
    ("no_conditioning", CFG, 2, dict(c=None), ValueError, "no conditioning c, the decoder has 16 conditioning channels"),
    ("logits_without_inputs", CFG, 0, dict(), ValueError, "teacher-forced: test_inputs must cover all 6 steps"),
    ("logits_short_inputs", CFG, 0, dict(test_inputs=torch.zeros(5)), ValueError, "must cover all 6 steps"),
    ("logistic_with_z", CFG, 2, dict(z=U6), ValueError, "'Logistic' draws from u_mix and u_log, not z"),
    ("u_mix_alone", CFG, 2, dict(u_mix=torch.zeros(6, 10)), ValueError, "u_mix and u_log come together"),
    ("u_log_alone", CFG, 2, dict(u_log=U6), ValueError, "u_mix and u_log come together"),
    ("normal_with_u_log", dict(CFG, output_distribution="Normal"), 2, dict(u_log=U6), ValueError, "'Normal' draws from u_mix and z, not u_log"),
    ("gaussians_without_u_mix", dict(CFG, output_distribution="Normal"), 2, dict(z=U6), ValueError, "10 Gaussians need u_mix beside z"),
    ("class_logits_short_inputs", CLASS, 0, dict(test_inputs=[1, 2, 3]), ValueError, "must cover all 6 steps"),
    ("start_class_too_large", CLASS, 1, dict(init_idx=32), IndexError, "index 32 is out of bounds for dimension 2 with size 32"),
    ("start_class_negative", CLASS, 2, dict(init_idx=torch.tensor([-1])), IndexError, "index -1 is out of bounds"),
    ("forced_class_too_large", CLASS, 2, dict(test_inputs=[0, 32]), IndexError, "test_inputs hold a class id outside [0, 32)"),
    ("forced_class_negative", CLASS, 0, dict(test_inputs=[0, 1, 2, 3, 4, -1]), IndexError, "class id outside [0, 32)"),
]


@pytest.mark.parametrize("who", CALLERS)
@pytest.mark.parametrize("cfg,mode,item,exc,words", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_intake_refuses(who, cfg, mode, item, exc, words):
    for index, at in ((None, f"{who}: "), (3, f"{who}: item 3: ")):
        with pytest.raises(exc) as e:
            _intake(_g(cfg), mode, item, who, index)
        text = str(e.value)
        assert words in text and (text.startswith(at) or text.startswith("index ")), text     # (the IndexError of the start class is torch's own wording)


def test_intake_leaves_the_class_range_to_a_caller_that_asks():
    T, forced, nf, init, given = _intake(_g(CLASS), 2, dict(test_inputs=[0, 32], init_idx=99), check_ids=False)
    assert forced.tolist() == [0, 32] and (nf, init) == (2, 0)         # decode_list reads its packed array once; a forced prefix: no start class
    with pytest.raises(IndexError):
        _intake(_g(CLASS), 2, dict(init_idx=99), check_ids=False)      # the start class is not part of that switch


def test_intake_accepts():
    assert _intake(_g(CLASS, O=256), 2, dict()) == (6, None, 0, 127, False)            # init_idx default 127, n_forced == 0: forced is None
    assert _intake(_g(CLASS, O=256), 1, dict(init_idx=torch.tensor([200])))[3] == 200
    assert _intake(_g(CLASS, O=256), 1, dict(test_inputs=[]))[1:3] == (None, 0)
    T, forced, nf, init, given = _intake(_g(CLASS, O=256), 2, dict(test_inputs=torch.arange(9), init_idx=200))
    assert forced.dtype == torch.int32 and forced.device.type == "cpu" and forced.tolist() == list(range(6))      # truncated to T
    assert (T, nf, init, given) == (6, 6, 0, False)                                    # init_idx zeroed when a prefix is given
    assert _intake(_g(CLASS, O=256), 0, dict(test_inputs=torch.arange(6).reshape(1, 6)))[2] == 6
    # scalar-input decoders: float prefix, start class 0 always, `given` = the item brings its own draws
    g = _g()
    T, forced, nf, init, given = _intake(g, 2, dict(test_inputs=torch.linspace(-1, 1, 8).double(), init_idx=9))
    assert forced.dtype == torch.float32 and forced.shape == (6,) and (nf, init, given) == (6, 0, False)
    assert _intake(g, 2, dict())[1:] == (None, 0, 0, False)
    assert _intake(g, 2, dict(u_mix=torch.zeros(6, 10), u_log=U6))[4] is True
    assert _intake(g, 0, dict(test_inputs=torch.zeros(6), u_mix=torch.zeros(6, 10), u_log=U6))[4] is True
    normal = _g(output_distribution="Normal")
    assert _intake(normal, 2, dict(z=U6, u_mix=torch.zeros(6, 10)))[4] is True and _intake(normal, 2, dict(u_mix=torch.zeros(6, 10)))[4] is False
    assert _intake(_g(output_distribution="Normal", O=2), 2, dict(z=U6))[4] is True      # one Gaussian needs no u_mix
    assert _intake(_g(Cc=0), 2, dict(c=None))[0] == 6                                   # no conditioning channels, no c


def test_small_rules():
    from wavenet_autoencoders_amd import decode
    assert decode.mixture(_g()) == (False, 10) and decode.mixture(_g(output_distribution="Normal")) == (True, 10)
    assert decode.mixture(_g(output_distribution="Normal", O=2)) == (True, 1) and decode.mixture(_g(CLASS)) == (False, 0)
    eng = _engine(CFG)
    eng.opt = type("Opt", (), {"ar_coop_c": 32})()
    assert decode.team_width(eng) == min(32, eng.g.H, eng.g.S)
    eng.opt.ar_coop_c = 0
    assert decode.team_width(eng) == 1
    assert [decode.group_count(eng, True, 99, t) for t in (None, 0, 3, 8, 20)] == [8, 1, 3, 8, 8]
    assert decode.group_count(eng, False, 7, None) == 7
    assert decode.coop_sized(eng.g) and not decode.coop_sized(_g(O=300))
    decode.refuse_wide(eng.g, "decode_list", "list")
    for who, instead in (("decode_list", "list"), ("decode_list_scalar", "list"), ("decode_session", "slots")):
        with pytest.raises(ValueError, match=rf"^{who}\(coop=True\): .*R, S and O <= 256 \(got 32, 32, 300\); use the one-CU {instead}"):
            decode.refuse_wide(_g(O=300), who, instead)
