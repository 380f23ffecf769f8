"""The ragged conditioning upsampler (wae_upsample_stage_fwd_list, wae_to_btc_list, packing.upsample_list_plan,
WaeEngine.upsample_list, DecodeSession.add_list) without a GPU: the symbols, their declarations and bindings, the entries' refusals
before any launch (raw ctypes calls with dummy pointers, as tests/test_encode_list_cpu.py), the launch plan's tables and the surface."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2
STAGE, TOBTC = "wae_upsample_stage_fwd_list", "wae_to_btc_list"
F32, BF16 = 0, 1

STAGE_PARAMS = ["const float* in", "const float* w", "void* out", "const wae_ups_seg* segs", "int32_t nsegs", "int32_t ntiles",
                "int32_t in_pitch", "int32_t out_pitch_or_rows", "int32_t C", "int32_t s", "int32_t out_btc", "int32_t Cp",
                "int32_t dtype", "void* stream"]
TOBTC_PARAMS = ["const float* in", "void* out", "const wae_ups_seg* segs", "int32_t nsegs", "int32_t ntiles", "int32_t in_pitch",
                "int32_t C", "int32_t Cp", "int32_t dtype", "void* stream"]


# ---- the symbols -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,want", [(STAGE, STAGE_PARAMS), (TOBTC, TOBTC_PARAMS)])
def test_entries_are_exported_declared_and_bound(entry, want):
    from wavenet_autoencoders_amd import _lib
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {entry}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {entry}("):]
    decl = decl[:decl.index(";")]
    params = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert params == want
    args = [vp if "*" in p else i32 for p in params]
    res, bound = _lib.SIGNATURES[entry]
    assert res is i32 and list(bound) == args and len(bound) == decl.count(",") + 1
    assert list(getattr(_lib.lib(), entry).argtypes) == args
    assert "typedef struct wae_ups_seg { int32_t in_off, Tin, out_off, tile0; } wae_ups_seg;" in hdr
    comment = hdr[:hdr.index("typedef struct wae_ups_seg")]
    comment = comment[comment.rindex("/*"):]
    for word in ("upsample.py:12-85", "bit for bit", "never reads the neighbour's column", "OF THE ITEM", "closing record", "binary search",
                 "WAE_EUNSUPPORTED", "WAE_EINVAL", "before any launch", "pad channels", "B = 1", "is skipped by the kernel"):
        assert word in comment, word


def test_tile_constants_of_the_header_are_the_planners():
    from wavenet_autoencoders_amd import packing as PK
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    get = lambda name: int(re.search(rf"#define {name} (\d+)", hdr).group(1))  # noqa: E731
    assert get("WAE_UPS_LIST_TILE_BTC") == PK.UPS_LIST_TILE_BTC == 64         # UPT of the dense last stage
    assert get("WAE_UPS_LIST_TILE_CT") == PK.UPS_LIST_TILE_CT == 256
    fir = open(os.path.join(ROOT, "wavenet_autoencoders_amd", "csrc", "ups_fir.hpp")).read()
    assert "#define UPT 64" in fir
    # the default cap: the largest fp32 intermediate at Cc 64 and a last scale of 5 is 205 MiB, the one before it (scale 8) an eighth
    assert PK.UPS_LIST_MAX_SAMPLES == 1 << 22
    assert round(64 * PK.UPS_LIST_MAX_SAMPLES / 5 * 4 / 2 ** 20) == 205


def _stage(lib, inp=P, w=P, out=P, segs=P, nsegs=3, ntiles=5, in_pitch=100, rows=400, C=16, s=4, out_btc=1, Cp=64, dtype=BF16):
    return lib.wae_upsample_stage_fwd_list(inp, w, out, segs, nsegs, ntiles, in_pitch, rows, C, s, out_btc, Cp, dtype, None)


def _tobtc(lib, inp=P, out=P, segs=P, nsegs=3, ntiles=5, in_pitch=100, C=16, Cp=64, dtype=BF16):
    return lib.wae_to_btc_list(inp, out, segs, nsegs, ntiles, in_pitch, C, Cp, dtype, None)


STAGE_EINVAL = [
    ("null_in", dict(inp=None), b"bad arguments"),
    ("null_w", dict(w=None), b"bad arguments"),
    ("null_out", dict(out=None), b"bad arguments"),
    ("no_channels", dict(C=0), b"bad arguments"),
    ("scale_0", dict(s=0), b"bad arguments"),
    ("null_segs", dict(segs=None), b"nsegs > 0 records"),
    ("no_segs", dict(nsegs=0), b"(got 0)"),
    ("no_tiles", dict(ntiles=0), b"ntiles must be > 0 (got 0)"),
    ("negative_tiles", dict(ntiles=-3), b"ntiles must be > 0 (got -3)"),
    ("no_in_pitch", dict(in_pitch=0), b"pitches must be > 0 (got 0, 400)"),
    ("negative_rows", dict(rows=-1), b"pitches must be > 0 (got 100, -1)"),
    ("cp_below_c", dict(C=80, Cp=64), b"Cp 64 < C 80"),
    ("bad_dtype", dict(dtype=7), b"bad dtype 7"),
    ("channel_major_null_in", dict(inp=None, out_btc=0), b"bad arguments"),
    ("channel_major_no_pitch", dict(rows=0, out_btc=0), b"pitches must be > 0 (got 100, 0)"),
]


@pytest.mark.parametrize("case,text", [r[1:] for r in STAGE_EINVAL], ids=[r[0] for r in STAGE_EINVAL])
def test_stage_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _stage(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"upsample_stage_fwd_list: ") and text in err, err


@pytest.mark.parametrize("case", [dict(C=130, Cp=192), dict(C=300, Cp=320), dict(C=16, Cp=512), dict(s=86), dict(s=300),
                                  dict(C=200, Cp=256, s=1)],
                         ids=["cp_192", "cp_320", "cp_512", "3s_258", "s_300", "lds_beyond_64k"])
def test_stage_entry_names_what_the_time_major_kernel_takes(case):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _stage(lib, **case) == EUNSUPPORTED
    err = lib.wae_last_error()
    assert b"Cp dividing 256" in err and b"3 s <= 256" in err and b"wae_upsample_stage_fwd per item" in err, err


TOBTC_EINVAL = [
    ("null_in", dict(inp=None), b"bad arguments"),
    ("null_out", dict(out=None), b"bad arguments"),
    ("no_channels", dict(C=0), b"bad arguments"),
    ("null_segs", dict(segs=None), b"nsegs > 0 records"),
    ("no_segs", dict(nsegs=-1), b"(got -1)"),
    ("no_tiles", dict(ntiles=0), b"must be > 0 (got 0, 100)"),
    ("no_pitch", dict(in_pitch=0), b"must be > 0 (got 5, 0)"),
    ("cp_below_c", dict(C=65), b"Cp 64 < C 65"),
    ("bad_dtype", dict(dtype=-1), b"bad dtype -1"),
]


@pytest.mark.parametrize("case,text", [r[1:] for r in TOBTC_EINVAL], ids=[r[0] for r in TOBTC_EINVAL])
def test_to_btc_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _tobtc(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"to_btc_list: ") and text in err, err


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
BASE = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
TCS = [1, 2, 3, 5, 17, 4, 9]


def _geom(**kw):
    from wavenet_autoencoders_amd import Geometry
    return Geometry.from_cfg(dict(BASE, **kw))


def _run(x):
    return np.concatenate([[0], np.cumsum(x)[:-1]])


def _check_records(rec, ntiles, in_off, Tin, out_off, Tout, tile):
    """records {in_off, Tin, out_off, tile0} + the closing one: running tile0, every [0, Tout_i) covered once by the item's own tiles"""
    n = len(Tin)
    assert rec.shape == (n + 1, 4) and rec.dtype == np.int32
    assert np.array_equal(rec[:n, 0], in_off) and np.array_equal(rec[:n, 1], Tin) and np.array_equal(rec[:n, 2], out_off)
    per = [-(-int(t) // tile) for t in Tout]
    assert np.array_equal(rec[:, 3], np.concatenate([[0], np.cumsum(per)])) and rec[n, 3] == ntiles == sum(per)
    assert tuple(rec[n, :3]) == (0, 0, 0)
    cover = [np.zeros(int(t), dtype=np.int64) for t in Tout]
    for b in range(ntiles):                     # what the kernel's search does: the last record with tile0 <= b
        i = int(np.searchsorted(rec[:n, 3], b, side="right")) - 1
        k = b - rec[i, 3]
        assert 0 <= k * tile < Tout[i]
        cover[i][k * tile:(k + 1) * tile] += 1   # masked at the item's Tout: the slice stops there
    assert all((c == 1).all() for c in cover)


@pytest.mark.parametrize("pad", [0, 1, 2])
def test_plan_conv_in_chain(pad):
    from wavenet_autoencoders_amd import packing as PK
    g = _geom(cin_pad=pad)
    Tcs = np.array(TCS) + 2 * pad
    plan = PK.upsample_list_plan(Tcs, g)
    assert [ln.kind for ln in plan.launches] == ["conv_in", "stage", "stage", "stage", "last"] and not plan.closes_with_to_btc
    assert plan.table.dtype == np.int32 and plan.table.ndim == 1
    assert np.array_equal(plan.Ts, np.array(TCS) * 640) and np.array_equal(plan.offsets, _run(plan.Ts))
    assert np.array_equal(plan.in_offsets, _run(Tcs)) and plan.in_pitch == Tcs.sum() and plan.rows == plan.Ts.sum()
    ci = plan.launches[0]
    assert (ci.s, ci.nsegs, ci.in_pitch, ci.out_pitch, ci.seg_off) == (2 * pad + 1, len(TCS), Tcs.sum(), sum(TCS), 0)
    segs = plan.records(0)
    assert np.array_equal(segs[:, 1], Tcs) and np.array_equal(segs[:, 3], TCS) and np.array_equal(segs[:, 2], _run(TCS))
    end = ci.tile_off + 2 * ci.ntiles
    Tin = np.array(TCS)
    for i, s in enumerate(g.upsample_scales):
        ln = plan.launches[1 + i]
        last = i == 3
        assert ln.seg_off == end and ln.tile_off == -1 and ln.s == s and ln.in_pitch == Tin.sum()
        assert ln.out_pitch == (plan.rows if last else (Tin * s).sum())
        _check_records(plan.records(1 + i), ln.ntiles, _run(Tin), Tin, plan.offsets if last else _run(Tin * s), Tin * s,
                       PK.UPS_LIST_TILE_BTC if last else PK.UPS_LIST_TILE_CT)
        end += 4 * (ln.nsegs + 1)
        Tin = Tin * s
    assert end == plan.table.size                                           # every launch's records in ONE array: one upload


@pytest.mark.parametrize("act", ["none", "Tanh"])
@pytest.mark.parametrize("pad", [0, 1])
def test_plan_plain_network_with_trim_and_activation(pad, act):
    from wavenet_autoencoders_amd import packing as PK
    g = _geom(cin_pad=pad, conv_in=False, up_act=act)
    Tcs = np.array(TCS) + 2 * pad
    plan = PK.upsample_list_plan(Tcs, g)
    closing = pad > 0 or act != "none"
    assert [ln.kind for ln in plan.launches] == ["stage"] * 3 + (["stage", "to_btc"] if closing else ["last"])
    assert plan.closes_with_to_btc == closing
    assert np.array_equal(plan.Ts, np.array(TCS) * 640)                     # (Tc - 2 cin_pad) * prod(scales)
    if closing:
        ln = plan.launches[-1]
        full, trim = Tcs * 640, pad * 640
        assert ln.in_pitch == full.sum() and ln.out_pitch == plan.rows
        _check_records(plan.records(4), ln.ntiles, _run(full) + trim, plan.Ts, plan.offsets, plan.Ts, PK.UPS_LIST_TILE_BTC)
    # an activation behind ConvInUpsampleNetwork closes with to_btc too
    if act != "none" and pad == 0:
        kinds = [ln.kind for ln in PK.upsample_list_plan(TCS, _geom(up_act=act)).launches]
        assert kinds == ["conv_in"] + ["stage"] * 4 + ["to_btc"]


def test_plan_given_offsets_and_upsampled_conditioning():
    from wavenet_autoencoders_amd import packing as PK
    g = _geom()
    offs = np.array([5000, 0, 700, 9000, 20000, 3000, 40000])
    plan = PK.upsample_list_plan(TCS, g, offsets=offs)
    assert np.array_equal(plan.offsets, offs) and plan.rows == 40000 + 9 * 640
    assert np.array_equal(plan.records(4)[:-1, 2], offs)                    # free: the caller's order, not monotone in in_off
    direct = PK.upsample_list_plan([640, 1, 65], g, c_is_upsampled=True)
    assert [ln.kind for ln in direct.launches] == ["to_btc"] and direct.closes_with_to_btc and list(direct.Ts) == [640, 1, 65]
    _check_records(direct.records(0), direct.launches[0].ntiles, [0, 640, 641], [640, 1, 65], [0, 640, 641], [640, 1, 65], 64)
    none = PK.upsample_list_plan([7, 3], _geom(upsample_scales=None))
    assert [ln.kind for ln in none.launches] == ["to_btc"] and list(none.Ts) == [7, 3]


def test_plan_refusals_groups_and_support():
    from wavenet_autoencoders_amd import packing as PK
    g = _geom(cin_pad=1)
    with pytest.raises(ValueError, match="an empty list"):
        PK.upsample_list_plan([], g)
    with pytest.raises(ValueError, match=r"item 2 has no output frame \(2 frames under cin_pad 1\)"):
        PK.upsample_list_plan([3, 4, 2, 5], g)
    with pytest.raises(ValueError, match="item 1 has no output frame"):
        PK.upsample_list_plan([3, 0], _geom())
    with pytest.raises(ValueError, match="item 3: the packed list reaches 2\\^31 samples"):
        PK.upsample_list_plan([1000000] * 5, _geom())                       # 640e6 samples an item: the fourth crosses 2^31
    with pytest.raises(ValueError, match="offsets"):
        PK.upsample_list_plan([3, 4], _geom(), offsets=[0])
    assert PK.upsample_list_groups([5, 5, 5, 5], 10) == [(0, 2), (2, 4)]
    assert PK.upsample_list_groups([3, 40, 3, 3, 3], 8) == [(0, 1), (1, 2), (2, 4), (4, 5)]       # an oversize item is its own group
    assert PK.upsample_list_groups([640] * 3) == [(0, 3)]
    with pytest.raises(ValueError, match="max_samples 0"):
        PK.upsample_list_groups([1], 0)
    ok = PK.upsample_list_supported
    assert ok(_geom()) and ok(_geom(cin_pad=2)) and ok(_geom(Cc=64)) and ok(_geom(Cc=200))
    assert not ok(_geom(cin_pad=3)) and not ok(_geom(Cc=130)) and not ok(_geom(upsample_scales=[4, 86]))
    assert ok(_geom(Cc=130), c_is_upsampled=True) and ok(_geom(Cc=130, up_act="ReLU"))   # a closing to_btc takes any Ccp


# ---- the surface -----------------------------------------------------------------------------------------------------------------------
def test_surface():
    from wavenet_autoencoders_amd import decode as D
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.upsample_list)
    assert list(sig.parameters) == ["self", "cs", "out", "offsets", "c_is_upsampled", "max_samples"]
    assert [sig.parameters[k].default for k in ("out", "offsets", "c_is_upsampled", "max_samples")] == [None, None, False, None]
    for word in ("bit for bit", "max_samples", "205 MiB", "caller's order", "ValueError", "wae_upsample_stage_fwd_list", "wae_to_btc_list"):
        assert word in WaeEngine.upsample_list.__doc__, word
    assert list(inspect.signature(D.DecodeSession.add_list).parameters) == ["self", "items"]
    assert "keep the group's buffer alive until its last clip ends" in D.DecodeSession.add_list.__doc__
    assert "add_list(" in inspect.getsource(D.list_rounds) and "upsample_list(" in inspect.getsource(D._list_cond)
    assert "_list_cond(" in inspect.getsource(D.decode_list) and "_clip_cond(" not in inspect.getsource(D.decode_list)
    assert "import engine" not in inspect.getsource(D) and "from .engine" not in inspect.getsource(D)


def test_upsample_list_refuses_without_a_device():
    """the checks come before anything that needs the engine's device state: an engine object that never saw a GPU is enough"""
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = object.__new__(WaeEngine)
    eng.g, eng.device = _geom(cin_pad=1), "cpu"
    ok = np.zeros((16, 4), np.float32)
    with pytest.raises(ValueError, match="upsample_list: an empty list"):
        eng.upsample_list([])
    with pytest.raises(ValueError, match=r"item 1 has shape \(17, 4\); every item is \(Cc, Tc\) or \(1, Cc, Tc\) with Cc = 16"):
        eng.upsample_list([ok, np.zeros((17, 4), np.float32)])
    with pytest.raises(ValueError, match=r"item 0 has shape \(2, 16, 4\)"):
        eng.upsample_list([np.zeros((2, 16, 4), np.float32)])
    with pytest.raises(ValueError, match="item 2 has no output frame"):
        eng.upsample_list([ok, ok[None], np.zeros((16, 2), np.float32)])
    with pytest.raises(ValueError, match="max_samples 0 < 1"):
        eng.upsample_list([ok], max_samples=0)
