"""List encoding (wae_enc_conv_fwd_list, packing.encode_list_plan, WaeEngine.encode_list, inference_2019.py --batch) without a GPU:
the symbol, its declaration and its binding, the entry's refusals before any launch (raw ctypes calls with dummy pointers, as
tests/test_ar_list_cpu.py), the launch plan's tables, the host-side refusals and the script's batching."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2
ENTRY = "wae_enc_conv_fwd_list"
FS = [1, 2, 3, 4, 5, 37, 128, 129, 131]


# ---- the symbol ------------------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {ENTRY}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {ENTRY}("):]
    decl = decl[:decl.index(";")]
    # x, w, bias, y, segs | nsegs | tiles | ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu, residual | stream
    args = [vp] * 5 + [i32, vp] + [i32] * 11 + [vp]
    res, bound = _lib.SIGNATURES[ENTRY]
    assert res is i32 and list(bound) == args
    assert list(getattr(_lib.lib(), ENTRY).argtypes) == args
    assert len(args) == decl.count(",") + 1
    params = [p.strip() for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert params == ["const float* x", "const float* w", "const float* bias", "float* y", "const wae_seg* segs", "int32_t nsegs",
                      "const int32_t* tiles", "int32_t ntiles", "int32_t et", "int32_t in_pitch", "int32_t out_pitch", "int32_t Cin",
                      "int32_t Cout", "int32_t k", "int32_t stride", "int32_t pad", "int32_t relu", "int32_t residual", "void* stream"]
    # one ctypes type per declared parameter, pointer for pointer
    assert [a is vp for a in args] == ["*" in p for p in params]
    assert "typedef struct wae_seg { int32_t in_off, Tin, out_off, Tout; } wae_seg;" in hdr
    comment = hdr[:hdr.index("typedef struct wae_seg")]
    comment = comment[comment.rindex("/*"):]
    for word in ("vqvae_model.py:17-23,48-51", "bit for bit", "in_pitch", "never the neighbour's column", "WAE_EUNSUPPORTED", "WAE_EINVAL",
                 "(segment, to0)", "wae_vq_nearest", "B = 1", "aggregate"):
        assert word in comment, word


def _call(lib, x=P, w=P, bias=P, y=P, segs=P, nsegs=3, tiles=P, ntiles=5, et=16, in_pitch=100, out_pitch=100, Cin=39, Cout=64, k=3,
          stride=1, pad=1, relu=1, residual=0):
    return lib.wae_enc_conv_fwd_list(x, w, bias, y, segs, nsegs, tiles, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu,
                                     residual, None)


REFUSED = [
    ("null_x", dict(x=None), b"bad arguments"),
    ("null_w", dict(w=None), b"bad arguments"),
    ("null_y", dict(y=None), b"bad arguments"),
    ("no_channels", dict(Cin=0), b"bad arguments"),
    ("no_outputs", dict(Cout=0), b"bad arguments"),
    ("k0", dict(k=0), b"bad arguments"),
    ("stride0", dict(stride=0), b"bad arguments"),
    ("negative_pad", dict(pad=-1), b"bad arguments"),
    ("null_segs", dict(segs=None), b"segment table"),
    ("no_segs", dict(nsegs=0), b"nsegs > 0 records (got 0)"),
    ("null_tiles", dict(tiles=None), b"tile table"),
    ("no_tiles", dict(ntiles=0), b"ntiles > 0 pairs (got 0)"),
    ("negative_tiles", dict(ntiles=-4), b"ntiles > 0 pairs (got -4)"),
    ("et_0", dict(et=0), b"et 0 is not 8, 16 or 32"),
    ("et_24", dict(et=24), b"et 24 is not 8, 16 or 32"),
    ("et_64", dict(et=64), b"et 64 is not 8, 16 or 32"),
    ("no_in_pitch", dict(in_pitch=0), b"pitches must be > 0 (got 0, 100)"),
    ("negative_out_pitch", dict(out_pitch=-7), b"pitches must be > 0 (got 100, -7)"),
    ("residual_strided", dict(k=5, stride=2, pad=2, Cin=64, residual=1), b"residual needs a same-shape conv"),
    ("residual_other_width", dict(residual=1), b"residual needs a same-shape conv"),
    ("residual_unpadded", dict(Cin=64, pad=0, residual=1), b"residual needs a same-shape conv"),
]


@pytest.mark.parametrize("case,text", [r[1:] for r in REFUSED], ids=[r[0] for r in REFUSED])
def test_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _call(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"enc_conv_fwd_list: ") and text in err, err


@pytest.mark.parametrize("k,stride", [(7, 1), (3, 2), (1, 2), (5, 3), (2, 1)])
def test_entry_names_the_shapes_it_has(k, stride):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _call(lib, k=k, stride=stride, pad=k // 2) == EUNSUPPORTED
    err = lib.wae_last_error()
    assert f"(k, stride) = ({k}, {stride})".encode() in err and b"wae_enc_conv_fwd per utterance" in err, err


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def _single_call_chain(F):
    from wavenet_autoencoders_amd import packing as PK
    T, out = F, []
    for k, s in list(PK.ENCODER_BLOCKS) + [(1, 1)]:
        T = (T + 2 * (k // 2) - k) // s + 1          # engine.encoder_forward / include/wae.h: wae_enc_conv_fwd
        out.append(T)
    return out


@pytest.mark.parametrize("et", [None, 8, 16, 32])
def test_plan_tables(et):
    from wavenet_autoencoders_amd import packing as PK
    plan = PK.encode_list_plan(FS, et=et)
    assert len(plan.layers) == len(PK.ENCODER_BLOCKS) + 1
    assert plan.table.dtype == np.int32 and plan.table.ndim == 1
    assert plan.table.size == sum(4 * ly.nsegs + 2 * ly.ntiles for ly in plan.layers)        # all layers in one array: one upload
    want = np.array([_single_call_chain(F) for F in FS])                                      # (item, layer)
    Tin = np.array(FS)
    end = 0
    for i, (ly, (k, s)) in enumerate(zip(plan.layers, list(PK.ENCODER_BLOCKS) + [(1, 1)])):
        assert (ly.k, ly.stride, ly.pad) == (k, s, k // 2)
        assert ly.et in (8, 16, 32) and (et is None or ly.et == et)
        assert ly.seg_off == end and ly.tile_off == end + 4 * ly.nsegs                        # back to back in the one table
        end = ly.tile_off + 2 * ly.ntiles
        segs, tiles = plan.segs(i), plan.tiles(i)
        assert segs.shape == (len(FS), 4) and tiles.shape == (ly.ntiles, 2)
        assert np.array_equal(segs[:, 1], Tin)
        assert np.array_equal(segs[:, 3], want[:, i])                                         # the single-call formula
        assert np.array_equal(segs[:, 0], np.concatenate([[0], np.cumsum(Tin)[:-1]]))         # running sums
        assert np.array_equal(segs[:, 2], np.concatenate([[0], np.cumsum(want[:, i])[:-1]]))
        assert ly.in_pitch == Tin.sum() and ly.out_pitch == want[:, i].sum()
        assert ly.ntiles == sum(-(-int(t) // ly.et) for t in want[:, i])
        cover = [np.zeros(int(t), dtype=np.int64) for t in want[:, i]]
        for sg, to0 in tiles:
            assert 0 <= sg < len(FS) and 0 <= to0 < want[sg, i] and to0 % ly.et == 0
            cover[sg][to0:to0 + ly.et] += 1           # a tile belongs to ONE segment: the slice stops at that segment's Tout
        assert all((c == 1).all() for c in cover)
        # no tile starts in one segment and ends in another: in packed columns it stays inside its segment's span once masked by Tout
        for sg, to0 in tiles:
            lo = segs[sg, 2] + to0
            hi = segs[sg, 2] + min(to0 + ly.et, segs[sg, 3])
            assert segs[sg, 2] <= lo < hi <= segs[sg, 2] + segs[sg, 3]
        Tin = want[:, i]
    assert end == plan.table.size
    assert np.array_equal(plan.Tq, want[:, -1]) and plan.total_Tq == want[:, -1].sum() and plan.total_F == sum(FS)
    assert np.array_equal(plan.q_offsets, np.concatenate([[0], np.cumsum(want[:, -1])[:-1]]))
    assert np.array_equal(plan.in_offsets, np.concatenate([[0], np.cumsum(FS)[:-1]]))


def test_plan_tile_length_of_a_single_utterance_is_the_single_call_rule():
    """csrc/misc.hip, launch_enc_fwd_tiled: 8 up to 8 outputs, 16 up to 16, else 32"""
    from wavenet_autoencoders_amd import packing as PK
    for T in list(range(1, 70)) + [375, 1500]:
        _, _, et, _ = PK.enc_list_tables([T], 3, 1, 1)
        assert et == (8 if T <= 8 else 16 if T <= 16 else 32), T


def test_plan_refusals_and_groups():
    from wavenet_autoencoders_amd import packing as PK
    with pytest.raises(ValueError, match="empty list"):
        PK.encode_list_plan([])
    with pytest.raises(ValueError, match="at least one frame"):
        PK.encode_list_plan([4, 0, 9])
    with pytest.raises(ValueError, match="et 24"):
        PK.encode_list_plan([4, 9], et=24)
    assert PK.encode_list_groups([5, 5, 5, 5], 10) == [(0, 2), (2, 4)]
    assert PK.encode_list_groups([5, 5, 5], 100) == [(0, 3)]
    assert PK.encode_list_groups([3, 40, 3, 3, 3], 8) == [(0, 1), (1, 2), (2, 4), (4, 5)]     # a long utterance is never split
    assert PK.encode_list_groups([1], 1) == [(0, 1)]
    with pytest.raises(ValueError, match="max_frames 0"):
        PK.encode_list_groups([1], 0)
    # the default cap: two fp32 buffers of encoder_hid = 768 rows stay at 192 MiB
    assert 2 * 768 * 4 * PK.ENC_LIST_MAX_FRAMES == 192 << 20


# ---- the host --------------------------------------------------------------------------------------------------------------------------
CFG = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
           c_in=39, K=32, cin_pad=0)


def test_encode_list_surface():
    from wavenet_autoencoders_amd.engine import WaeEngine
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    sig = inspect.signature(WaeEngine.encode_list)
    assert list(sig.parameters) == ["self", "feats", "want_latents", "want_idx", "max_frames"]
    assert {k: sig.parameters[k].default for k in ("want_latents", "want_idx", "max_frames")} == dict(want_latents=False, want_idx=True,
                                                                                                      max_frames=None)
    doc = WaeEngine.encode_list.__doc__
    for word in ("bit for bit", "max_frames", "192 MiB", "caller's order", "ValueError", "wae_enc_conv_fwd_list"):
        assert word in doc, word
    assert list(inspect.signature(VQVAE.encode_list).parameters) == ["self", "xs"]


def test_encode_list_refuses_without_a_device():
    """the checks come before anything that needs the engine's device state: an engine object that never saw a GPU is enough"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = object.__new__(WaeEngine)
    eng.g = Geometry.from_cfg({k: v for k, v in CFG.items() if k not in ("c_in", "encoder_hid")})
    with pytest.raises(ValueError, match="encode_list: this engine has no encoder"):
        eng.encode_list([np.zeros((39, 4), np.float32)])
    eng.g = Geometry.from_cfg(CFG)
    with pytest.raises(ValueError, match="encode_list: an empty list"):
        eng.encode_list([])
    ok = np.zeros((39, 4), np.float32)
    with pytest.raises(ValueError, match=r"item 1 has shape \(40, 4\); every item is \(c_in, F\) = \(39, F\)"):
        eng.encode_list([ok, np.zeros((40, 4), np.float32)])
    with pytest.raises(ValueError, match=r"item 0 has shape \(1, 39, 4\)"):
        eng.encode_list([ok[None]])
    with pytest.raises(ValueError, match="item 2 has no frames"):
        eng.encode_list([ok, ok, np.zeros((39, 0), np.float32)])
    with pytest.raises(ValueError, match="max_frames 0 < 1"):
        eng.encode_list([ok], max_frames=0)


# ---- the script ------------------------------------------------------------------------------------------------------------------------
def test_inference_script_batch_option_and_grouping():
    import inference_2019 as inf
    pos = ["list.json", "mfcc.norm", "ckpt.pth", "out/"]
    assert inf.parse_args(pos).batch == 1                          # the default: the loop, one utterance at a time
    assert inf.parse_args(pos + ["--batch", "16"]).batch == 16
    assert inf.parse_args(["--batch=3"] + pos).batch == 3
    for bad in ("0", "-2", "x"):
        with pytest.raises(SystemExit):
            inf.parse_args(pos + ["--batch", bad])
    scp = [[f"u{i}", f"/a/b/lan/set/u{i}/"] for i in range(7)]
    got = inf.batches(scp, 3)
    assert [len(b) for b in got] == [3, 3, 1] and [e for b in got for e in b] == scp       # a short last one, the list's order
    assert inf.batches(scp, 7) == [scp] and inf.batches(scp, 100) == [scp] and inf.batches([], 4) == []
    assert [len(b) for b in inf.batches(scp, 1)] == [1] * 7
    with pytest.raises(ValueError):
        inf.batches(scp, 0)
    # --batch 1 stays the loop; N > 1 goes through process_batch / encode_features_list
    src = inspect.getsource(inf.main)
    assert "if args.batch > 1:" in src and "process_batch(" in src and "process_utterance(" in src
    assert "encode_list(" in inspect.getsource(inf.encode_features_list)


def test_inference_script_missing_feature_file_raises(tmp_path):
    import inference_2019 as inf
    base = str(tmp_path) + "/a/lan/set/utt/"
    with pytest.raises(FileNotFoundError, match="mfcc.norm.npy"):
        inf.process_batch([["utt", base]], "mfcc.norm", None, str(tmp_path) + "/out/")
