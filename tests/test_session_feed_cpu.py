"""Clips whose conditioning arrives while they decode (wae_upsample_stage_fwd_ranges, packing.session_feed_plan, DecodeSession.open /
feed / feed_list / end) without a GPU: the plan by brute force -- over every split of 1..6 frames into feeds the ranges tile [0, T)
once per stage, no open-clip range reaches past (Tin - 1) * s, `ready` is the closed form -- a float64 restatement of the stage that
shows the rows the plan calls final on a prefix to be the whole clip's, the entry's declaration, binding and refusals before any
launch (raw ctypes calls with dummy pointers, as tests/test_upsample_list_cpu.py), and the session's refusals."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2
ENTRY = "wae_upsample_stage_fwd_ranges"
PARAMS = ["const float* in", "const float* w", "void* out", "const wae_ups_range* recs", "int32_t nrecs", "int32_t ntiles",
          "int32_t in_pitch", "int32_t out_pitch_or_rows", "int32_t C", "int32_t s", "int32_t out_btc", "int32_t Cp", "int32_t dtype",
          "void* stream"]
SCALES = [[4, 4, 8, 5], [4, 4, 4, 5], [2, 3], [5]]


def _splits(F):
    """every way to cut F frames into feeds of >= 1 frame (compositions: 2^(F-1) of them, one frame at a time among them)"""
    for cuts in itertools.product([0, 1], repeat=F - 1):
        out, run = [], 1
        for c in cuts:
            if c:
                out.append(run)
                run = 1
            else:
                run += 1
        yield out + [run]


def _closed_form(F, scales, ended):
    prod = int(np.prod(scales))
    if ended:
        return F * prod
    return max(0, prod * (F - 1) - sum(int(np.prod(scales[i:])) for i in range(1, len(scales))))


def _drive(scales, feeds, base=3, end_with_last=False):
    """the plans of a clip fed `feeds` frames at a time and ended behind the last feed (the end as a plan of its own, or in the last
    feed's plan) -> per stage the list of (Tin, t_lo, t_hi, open) and the `ready` after every plan"""
    from wavenet_autoencoders_amd import packing as PK
    per_stage, ready, F = [[] for _ in scales], [], 0
    steps = [(n, False) for n in feeds] + [(0, True)]
    if end_with_last:
        steps = steps[:-2] + [(feeds[-1], True)]
    ended = False
    for n, end in steps:
        plan = PK.session_feed_plan(scales, [(base, F, ended, F + n, end)])
        F, ended = F + n, end
        ready.append(int(plan.ready[0]))
        mul = [int(np.prod(scales[:i])) for i in range(len(scales) + 1)]
        for i, ln in enumerate(plan.launches):
            rec = plan.records(i)
            assert rec.shape == (2, 6) and ln.nrecs == 1 and ln.s == scales[ln.stage] and ln.last == (ln.stage == len(scales) - 1)
            in_off, Tin, out_off, lo, hi, tile0 = (int(v) for v in rec[0])
            tile = PK.UPS_LIST_TILE_BTC if ln.last else PK.UPS_LIST_TILE_CT
            assert (in_off, out_off, tile0) == (base * mul[ln.stage], base * mul[ln.stage + 1], 0)
            assert lo < hi and int(rec[1, 5]) == ln.ntiles == -(-(hi - lo) // tile)          # no empty record; the closing one counts
            per_stage[ln.stage].append((Tin, lo, hi, not end))
    return per_stage, ready


@pytest.mark.parametrize("scales", SCALES, ids=[str(s) for s in SCALES])
def test_ranges_of_all_feeds_tile_the_clip_once_and_ready_is_the_closed_form(scales):
    from wavenet_autoencoders_amd import packing as PK
    for F in range(1, 7):
        T = F * int(np.prod(scales))
        for feeds in _splits(F):
            per_stage, ready = _drive(scales, feeds)
            for i, s in enumerate(scales):
                Ti = F * int(np.prod(scales[:i + 1]))
                at = 0
                for Tin, lo, hi, is_open in per_stage[i]:
                    assert lo == at, (scales, feeds, i)                                    # neither a gap nor a row twice
                    assert hi <= ((Tin - 1) * s if is_open else Tin * s), (scales, feeds, i)
                    assert Tin * int(np.prod(scales[i:])) <= T
                    at = hi
                assert at == Ti, (scales, feeds, i)
            fed = np.cumsum(feeds)
            assert ready == [_closed_form(int(f), scales, False) for f in fed] + [T], (scales, feeds)
            assert all(PK.feed_ready(int(f), scales, False) == r for f, r in zip(fed, ready))
            assert PK.feed_final_rows(F, scales, True)[-1] == PK.feed_ready(F, scales, True) == T
            per_stage, ready = _drive(scales, feeds, end_with_last=True)         # the last frames and the end in one plan
            for i in range(len(scales)):
                spans = [(lo, hi) for _, lo, hi, _ in per_stage[i]]
                assert spans[0][0] == 0 and spans[-1][1] == F * int(np.prod(scales[:i + 1]))
                assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (scales, feeds, i)
            assert ready[-1] == T
    assert [_closed_form(F, [4, 4, 8, 5], False) for F in (1, 2, 3)] == [0, 640 - 205, 1280 - 205]       # a lookahead of 845 samples


def _stage64(x, w, s):
    """one stage in float64: nearest stretch by s, zero pad of s at both ends, FIR of 2s + 1 taps"""
    up = np.repeat(x, s, axis=-1)
    pad = np.pad(up, [(0, 0), (s, s)])
    return np.stack([pad[:, t:t + 2 * s + 1] @ w for t in range(up.shape[-1])], axis=-1)


@pytest.mark.parametrize("scales", SCALES, ids=[str(s) for s in SCALES])
def test_rows_the_plan_calls_final_on_a_prefix_are_the_whole_clips(scales):
    from wavenet_autoencoders_amd import packing as PK
    rng = np.random.default_rng(len(scales))
    F, C = 6, 3
    x = rng.standard_normal((C, F))
    ws = [rng.standard_normal(2 * s + 1) for s in scales]
    whole = [x]
    for w, s in zip(ws, scales):
        whole.append(_stage64(whole[-1], w, s))
    for n in range(1, F + 1):
        final = PK.feed_final_rows(n, scales, False)
        cur = x[:, :n]
        for i, (w, s) in enumerate(zip(ws, scales)):
            nxt = _stage64(cur[:, :final[i]], w, s) if final[i] else np.zeros((C, 0))    # from the final input rows alone, zero-padded there
            k = final[i + 1]
            assert k <= nxt.shape[-1] and np.array_equal(nxt[:, :k], whole[i + 1][:, :k]), (scales, n, i)
            if final[i] < whole[i].shape[-1] and nxt.shape[-1] > k:        # (an input row is still to come)
                assert not np.array_equal(nxt[:, k], whole[i + 1][:, k])                  # the rule is tight: the next row is not final
            cur = nxt
    done = PK.feed_final_rows(F, scales, True)
    assert done == [a.shape[-1] for a in whole]


def test_plan_of_many_clips_leaves_empty_ranges_and_idle_stages_out():
    from wavenet_autoencoders_amd import packing as PK
    sc = [4, 4, 8, 5]
    # clip 0: first frame (nothing final yet at any stage), clip 1: an empty feed, clip 2: frames 2 -> 3, clip 3: ends
    plan = PK.session_feed_plan(sc, [(0, 0, False, 1, False), (10, 2, False, 2, False), (20, 2, False, 3, False), (30, 2, False, 2, True)])
    assert [ln.stage for ln in plan.launches] == [0, 1, 2, 3] and all(ln.nrecs == 2 for ln in plan.launches)
    assert list(plan.ready) == [0, 435, 1075, 1280]
    last = plan.records(3)
    assert last[:, 5].tolist() == [0, -(-640 // 64), -(-640 // 64) + -(-845 // 64)] and last[0, 3:5].tolist() == [435, 1075]
    assert last[1].tolist()[:5] == [30 * 128, 256, 30 * 640, 435, 1280]
    assert plan.table.dtype == np.int32 and plan.table.size == sum(6 * (ln.nrecs + 1) for ln in plan.launches)
    # only first frames and empty feeds: no stage has a record, nothing is launched
    idle = PK.session_feed_plan(sc, [(0, 0, False, 1, False), (10, 2, False, 2, False)])
    assert idle.launches == [] and idle.table.size == 0 and list(idle.ready) == [0, 435]
    # two frames at [2, 3]: both stages have rows; one frame: none
    part = PK.session_feed_plan([2, 3], [(0, 0, False, 2, False)])
    assert [ln.stage for ln in part.launches] == [0, 1] and list(part.ready) == [3]
    assert PK.session_feed_plan([2, 3], [(0, 0, False, 1, False)]).launches == []
    assert [ln.stage for ln in PK.session_feed_plan([4, 4], [(0, 1, False, 2, False)]).launches] == [0, 1]
    for bad, text in ((dict(scales=[], clips=[(0, 0, False, 1, False)]), "at least one stage"),
                      (dict(scales=sc, clips=[(0, 3, False, 2, False)]), "clip 0: frames 3 -> 2"),
                      (dict(scales=sc, clips=[(0, 1, False, 1, False), (0, 2, True, 3, True)]), "clip 1: frames 2 -> 3, ended True -> True"),
                      (dict(scales=sc, clips=[(0, 2, True, 2, False)]), "ended True -> False"),
                      (dict(scales=sc, clips=[(2 ** 22, 0, False, 1, False)]), "reach 2^31")):
        with pytest.raises(ValueError, match=text.replace("^", r"\^")):
            PK.session_feed_plan(**bad)


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------
def test_entry_is_exported_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert f" T {ENTRY}\n" in nm
    hdr = open(os.path.join(ROOT, "include", "wae.h")).read()
    decl = hdr[hdr.index(f"int {ENTRY}("):]
    decl = decl[:decl.index(";")]
    params = [" ".join(p.split()) for p in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
    assert params == PARAMS
    args = [vp if "*" in p else i32 for p in params]
    res, bound = _lib.SIGNATURES[ENTRY]
    assert res is i32 and list(bound) == args
    assert list(getattr(_lib.lib(), ENTRY).argtypes) == args
    assert "typedef struct wae_ups_range { int32_t in_off, Tin, out_off, t_lo, t_hi, tile0; } wae_ups_range;" in hdr
    comment = hdr[:hdr.index("typedef struct wae_ups_range")]
    comment = comment[comment.rindex("/*"):]
    for word in ("t_hi <= (Tin - 1) * s", "t_hi <= Tin * s", "count from t_lo", "closing record", "binary search", "pad channels",
                 "is skipped", "before any launch", "WAE_EINVAL", "WAE_EUNSUPPORTED", "no \"open\" flag"):
        assert word in comment, word


def _ranges(lib, inp=PTR, w=PTR, out=PTR, recs=PTR, nrecs=3, ntiles=5, in_pitch=100, rows=400, C=16, s=4, out_btc=1, Cp=64, dtype=1):
    return lib.wae_upsample_stage_fwd_ranges(inp, w, out, recs, nrecs, ntiles, in_pitch, rows, C, s, out_btc, Cp, dtype, None)


RANGES_EINVAL = [
    ("null_in", dict(inp=None), b"bad arguments"),
    ("null_w", dict(w=None), b"bad arguments"),
    ("null_out", dict(out=None), b"bad arguments"),
    ("no_channels", dict(C=0), b"bad arguments"),
    ("scale_0", dict(s=0), b"bad arguments"),
    ("null_recs", dict(recs=None), b"nrecs > 0 records"),
    ("no_recs", dict(nrecs=0), b"(got 0)"),
    ("no_tiles", dict(ntiles=0), b"ntiles must be > 0 (got 0)"),
    ("no_in_pitch", dict(in_pitch=0), b"pitches must be > 0 (got 0, 400)"),
    ("negative_rows", dict(rows=-1), b"pitches must be > 0 (got 100, -1)"),
    ("cp_below_c", dict(C=80, Cp=64), b"Cp 64 < C 80"),
    ("bad_dtype", dict(dtype=7), b"bad dtype 7"),
    ("channel_major_null_in", dict(inp=None, out_btc=0), b"bad arguments"),
    ("channel_major_no_pitch", dict(rows=0, out_btc=0), b"pitches must be > 0 (got 100, 0)"),
]


@pytest.mark.parametrize("case,text", [r[1:] for r in RANGES_EINVAL], ids=[r[0] for r in RANGES_EINVAL])
def test_ranges_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ranges(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"upsample_stage_fwd_ranges: ") and text in err, err


@pytest.mark.parametrize("case", [dict(C=130, Cp=192), dict(C=16, Cp=512), dict(s=86), dict(C=200, Cp=256, s=1)],
                         ids=["cp_192", "cp_512", "3s_258", "lds_beyond_64k"])
def test_ranges_entry_names_what_the_time_major_kernel_takes(case):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ranges(lib, **case) == EUNSUPPORTED
    err = lib.wae_last_error()
    assert b"Cp dividing 256" in err and b"3 s <= 256" in err, err


# ---- the session's refusals, before a device is touched --------------------------------------------------------------------------------
BASE = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)


class _Eng:
    """as much of WaeEngine as DecodeSession reads before it opens its device state"""
    ar_scalar_coop = False

    def __init__(self, **cfg):
        from wavenet_autoencoders_amd import Geometry
        self.g = Geometry.from_cfg(dict(BASE, **cfg))
        self.device = "cpu"


@pytest.mark.parametrize("cfg,kw,text", [
    (dict(cin_pad=1), {}, "cin_pad 1 > 0"),
    (dict(up_act="LeakyReLU", up_act_slope=0.2), {}, r"an upsample_activation \(LeakyReLU\)"),
    ({}, dict(c_is_upsampled=True), "c_is_upsampled conditioning"),
    (dict(upsample_scales=None), {}, "no upsampling network"),
    (dict(Cc=130), {}, "Ccp dividing 256"),
], ids=["cin_pad", "activation", "c_is_upsampled", "no_network", "ccp_192"])
def test_open_refuses_what_only_add_takes(cfg, kw, text):
    from wavenet_autoencoders_amd.decode import DecodeSession
    sess = DecodeSession(_Eng(**cfg), mode="argmax", **kw)
    for call in (lambda: sess.open(dict(gid=1)), lambda: sess.reserve_frames(8)):
        with pytest.raises(NotImplementedError, match=text) as e:
            call()
        assert "with add" in str(e.value)
    assert sess.clips == {} and not sess._open                     # nothing joined, no device state


def test_open_wants_no_T_no_c_and_no_draws():
    from wavenet_autoencoders_amd.decode import DecodeSession
    sess = DecodeSession(_Eng(), mode="sample")
    for item, text in ((dict(gid=1, T=640), "no T and no c yet"), (dict(gid=1, c=np.zeros((16, 1))), "no T and no c yet"),
                       (dict(gid=1, uniforms=np.zeros(640)), "come with its feeds"), (dict(gid=1), "max_T 100 is less than one latent frame")):
        with pytest.raises(ValueError, match=text):
            sess.open(item, max_T=100)
    assert sess.clips == {} and not sess._open


def _bare_session(mode="sample", **feed):
    """a session with one open clip put there by hand: what end() and the checks of feed_list() read, no device"""
    from wavenet_autoencoders_amd import decode as D
    sess = D.DecodeSession(_Eng(), mode=mode)
    sess._fa_mul = [1, 4, 16, 128, 640]
    sess.normal, sess.M = False, 0
    sess.clips[0] = D._ArClip(T=0, slot=0, c_up=None, forced=None, n_forced=0, init=0, uni=None, u_mix=None, draw=None, feed=D._Feed(**feed))
    sess.clips[1] = D._ArClip(T=640, slot=1, c_up=None, forced=None, n_forced=0, init=0, uni=None, u_mix=None, draw=None)
    return sess


def test_end_right_after_open_raises_and_feed_after_end_is_refused():
    sess = _bare_session()
    with pytest.raises(ValueError, match="clip 0 has no frames"):
        sess.end(0)
    with pytest.raises(ValueError, match=r"clip 1 joined whole \(add\)"):
        sess.end(1)
    sess = _bare_session(frames=2, planned=2, cap=8, given=True, drawn=1000)
    with pytest.raises(ValueError, match="ends at 1280 steps beyond the 1000 draws supplied"):
        sess.end(0)
    sess.clips[0].feed.drawn = 1280
    sess.end(0)
    assert sess.clips[0].T == 1280 and sess.clips[0].feed.ended and sess._fa_pending
    with pytest.raises(ValueError, match="clip 0 has ended$"):
        sess.end(0)
    with pytest.raises(ValueError, match="clip 0 has ended: no feed after end"):
        sess.feed(0, np.zeros((16, 1), dtype=np.float32))
    sess = _bare_session(mode="logits", frames=1, planned=1, cap=8)
    with pytest.raises(ValueError, match="teacher-forced: test_inputs must cover all 640 steps"):
        sess.end(0)


def test_feed_list_checks_every_feed_before_anything_is_launched():
    sess = _bare_session(frames=1, planned=1, cap=2, max_frames=2, given=True, drawn=640)
    one = np.zeros((16, 1), dtype=np.float32)
    for feeds, kw, err, text in (
            ({7: one}, {}, ValueError, "clip 7 is not an open clip"),
            ({1: one}, {}, ValueError, "clip 1 is not an open clip"),
            ({0: np.zeros((15, 1))}, {}, ValueError, r"a feed is \(Cc, f\) or \(1, Cc, f\) with Cc = 16"),
            ({0: np.zeros((16, 2))}, {}, ValueError, r"3 frames are beyond max_T \(2 frames\)"),
            ({0: one}, dict(uniforms={0: np.zeros(10)}), ValueError, "makes 435 steps final"),     # (the 640 from before cover them)
            ({0: one}, dict(uniforms={1: np.zeros(10)}), ValueError, "draws for clip 1, which this call does not feed"),
            ({0: one}, dict(u_log={0: np.zeros(640)}), ValueError, "a class-id decoder draws from uniforms"),
            ({0: one}, {}, ValueError, "with every feed of a clip, or with none")):
        if "makes 435" in text:
            sess.clips[0].feed.drawn = 0
        with pytest.raises(err, match=text):
            sess.feed_list(feeds, **kw)
        sess.clips[0].feed.drawn = 640
    f = sess.clips[0].feed
    assert (f.frames, f.planned, f.ready, f.drawn) == (1, 1, 0, 640) and sess.clips[0].uni is None
    # an argmax session takes no draws
    sess = _bare_session(mode="argmax", frames=1, planned=1, cap=2)
    with pytest.raises(ValueError, match="draws are for mode 'sample'"):
        sess.feed(0, one, uniforms=np.zeros(640))


def test_surface_and_documents():
    from wavenet_autoencoders_amd.decode import DecodeSession
    from wavenet_autoencoders_amd.engine import WaeEngine
    for name in ("open", "feed", "feed_list", "end", "reserve_frames"):
        assert callable(getattr(DecodeSession, name)), name
    doc = DecodeSession.feed_list.__doc__
    for word in ("ONE conv_in", "ONE table upload", "bit for bit", "NOT add's order", "beyond max_T", "beyond the draws supplied"):
        assert word in doc, word
    assert "open" in WaeEngine.decode_session.__doc__ and "feed_list" in WaeEngine.decode_session.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Clips that are fed while they decode" in design
    assert "arrives while a clip is decoding is out of scope" not in design
    assert "--feed-frames" in open(os.path.join(ROOT, "README.md")).read()
    assert "--feed-frames" in open(os.path.join(ROOT, "synthesis.py")).read()
