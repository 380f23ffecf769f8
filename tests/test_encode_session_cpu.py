"""Utterances whose features arrive while they are encoded (wae_enc_conv_fwd_ranges, packing.enc_feed_plan, EncodeSession) without a
GPU: the finality rule by brute force against a float64 restatement of ENCODER_BLOCKS + lin -- for every length 1..59 and every
prefix, the columns the rule calls final on the prefix are the whole clip's, and the next one is not --, the closed forms, the plan
over random feeding schedules (every layer's ranges tile [0, Tout) once, no open range reaches a tap at Tin, bases never overlap,
tile counts match the closing record), the entry's declaration, binding and refusals before any launch (raw ctypes calls with dummy
pointers, as tests/test_session_feed_cpu.py), and the session's refusals that need no device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2
ENTRY = "wae_enc_conv_fwd_ranges"
PARAMS = ["const float* x", "const float* w", "const float* bias", "float* y", "const wae_enc_range* recs", "int32_t nrecs",
          "int32_t ntiles", "int32_t et", "int32_t in_pitch", "int32_t out_pitch", "int32_t Cin", "int32_t Cout", "int32_t k",
          "int32_t stride", "int32_t pad", "int32_t relu", "int32_t residual", "void* stream"]
C_IN, HID, CC, FMAX = 3, 16, 4, 59


# ---- the rule against brute force -----------------------------------------------------------------------------------------------------
def _weights():
    from wavenet_autoencoders_amd import packing as PK
    rng = np.random.default_rng(1234)
    ws, ci = [], C_IN
    for k, _ in PK.ENCODER_BLOCKS:
        ws.append((rng.standard_normal((HID, ci, k)) / np.sqrt(ci * k), 0.3 * rng.standard_normal(HID)))
        ci = HID
    ws.append((rng.standard_normal((CC, HID, 1)) / np.sqrt(HID), 0.3 * rng.standard_normal(CC)))
    return ws


def _conv64(x, w, b, k, s):
    """conv1d(x, w, b, stride s, pad k // 2) in float64, tap by tap; an output's value does not depend on the clip's length"""
    p = k // 2
    Tout = (x.shape[1] + 2 * p - k) // s + 1
    xp = np.pad(x, [(0, 0), (p, p)])
    y = np.repeat(b[:, None], Tout, axis=1)
    for j in range(k):
        for c in range(x.shape[0]):
            y = y + w[:, c, j][:, None] * xp[c, j:j + (Tout - 1) * s + 1:s][None, :]
    return y


def _encode64(x, ws):
    """the input of every layer and the latents (12 arrays): y = relu(conv(x)) (+ x for a same-shape block), then lin"""
    from wavenet_autoencoders_amd import packing as PK
    acts = [x]
    for (k, s), (w, b) in zip(PK.ENCODER_BLOCKS, ws):
        y = np.maximum(_conv64(acts[-1], w, b, k, s), 0.0)
        if s == 1 and w.shape[0] == w.shape[1]:
            y = y + acts[-1]
        acts.append(y)
    acts.append(_conv64(acts[-1], ws[-1][0], ws[-1][1], 1, 1))
    return acts


@pytest.fixture(scope="module")
def encodings():
    """every prefix of one seeded clip of FMAX frames, encoded once: prefix n -> its 12 activations"""
    ws = _weights()
    x = np.random.default_rng(99).standard_normal((C_IN, FMAX))
    return {n: _encode64(x[:, :n], ws) for n in range(1, FMAX + 1)}


def test_final_columns_of_every_prefix_are_the_whole_clips_and_the_next_one_is_not(encodings):
    from wavenet_autoencoders_amd import packing as PK
    tight = 0
    for F in range(1, FMAX + 1):
        whole = encodings[F]
        assert PK.enc_final_rows(F, True) == [a.shape[1] for a in whole]
        assert PK.enc_ready(F, True) == whole[-1].shape[1]
        for n in range(1, F + 1):
            pre, final = encodings[n], PK.enc_final_rows(n, False)
            assert len(final) == 12 and final[0] == n and final[-1] == PK.enc_ready(n, False)
            for l in range(12):
                r = final[l]
                assert r <= pre[l].shape[1] and r <= whole[l].shape[1], (F, n, l)
                assert np.array_equal(pre[l][:, :r], whole[l][:, :r]), (F, n, l)
            r = final[-1]
            if n < F and r < pre[-1].shape[1] and r < whole[-1].shape[1]:        # both encodings have the column behind the final ones
                assert not np.array_equal(pre[-1][:, r], whole[-1][:, r]), (F, n)
                tight += 1
    assert tight > 100


def test_closed_forms():
    from wavenet_autoencoders_amd import packing as PK
    for F in range(1, 200):
        assert PK.enc_ready(F, False) == max(0, (F - 13) // 4) == PK.enc_final_rows(F, False)[-1]
        assert PK.enc_ready(F, True) == (F + 3) // 4 == PK.enc_final_rows(F, True)[-1]
    for q in range(0, 40):        # latent frame q needs 4 q + 17 feature frames
        assert PK.enc_ready(4 * q + 17, False) == q + 1 and PK.enc_ready(4 * q + 16, False) == q
    assert PK.enc_final_rows(0, False) == [0] * 12 and PK.enc_ready(0, False) == 0
    assert PK.ENC_ARENA_DIV == [1, 1, 1, 2, 4, 4, 4, 4, 4, 4, 4, 4] and PK.ENC_ROOM == 4
    # one cost model for the list's tables and the session's ranges
    for touts in ([1], [8], [9], [16], [17], [33], [5, 1], [9, 9, 40], [200, 3]):
        assert PK.enc_list_et(touts) == PK.enc_list_tables([t for t in touts], 1, 1, 0)[2]


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
def _open_bound(n, k, s):
    p = k // 2
    return (n - k + p) // s + 1 if n - k + p >= 0 else 0


def _drive(feeds, base=8, end_with_last=False):
    """the plans of one clip fed `feeds` frames at a time and ended behind the last feed (in a plan of its own, or in the last feed's)
    -> per layer the list of (Tin, t_lo, t_hi, open), the `ready` after every plan and the packed counts"""
    from wavenet_autoencoders_amd import packing as PK
    per_layer, ready, counts, F = [[] for _ in PK.ENC_LAYERS], [], [], 0
    steps = [(n, False) for n in feeds] + [(0, True)]
    if end_with_last:
        steps = steps[:-2] + [(feeds[-1], True)]
    for n, end in steps:
        plan = PK.enc_feed_plan([(base, F, False, F + n, end)])
        F += n
        ready.append(int(plan.ready[0]))
        counts.append(int(plan.q_cnt[0]))
        assert int(plan.q_off[0]) == 0 and plan.total_new == counts[-1]
        assert plan.table.dtype == np.int32 and plan.table.size == sum(6 * (ln.nrecs + 1) for ln in plan.launches)
        for i, ln in enumerate(plan.launches):
            rec = plan.records(i)
            k, s = PK.ENC_LAYERS[ln.layer]
            assert rec.shape == (2, 6) and ln.nrecs == 1 and (ln.k, ln.stride, ln.pad) == (k, s, k // 2) and ln.et in PK.ENC_LIST_ETS
            in_off, Tin, out_col, lo, hi, tile0 = (int(v) for v in rec[0])
            last = ln.layer == len(PK.ENC_LAYERS) - 1
            assert in_off == base // PK.ENC_ARENA_DIV[ln.layer] and tile0 == 0
            assert out_col == (0 if last else base // PK.ENC_ARENA_DIV[ln.layer + 1] + lo)
            assert lo < hi and int(rec[1, 5]) == ln.ntiles == -(-(hi - lo) // ln.et)         # no empty record; the closing one counts
            per_layer[ln.layer].append((Tin, lo, hi, not end))
    return per_layer, ready, counts


def _schedules(F, rng):
    yield [1] * F
    yield [F]
    for _ in range(3):
        out, left = [], F
        while left:
            n = int(rng.integers(1, min(left, 9) + 1))
            out.append(n)
            left -= n
        yield out


def test_ranges_of_all_feeds_tile_every_layer_once():
    from wavenet_autoencoders_amd import packing as PK
    rng = np.random.default_rng(5)
    for F in list(range(1, 40)) + [129]:
        Touts = PK.enc_final_rows(F, True)
        for feeds in _schedules(F, rng):
            for end_with_last in (False, True):
                per_layer, ready, counts = _drive(feeds, end_with_last=end_with_last)
                for l, (k, s) in enumerate(PK.ENC_LAYERS):
                    at = 0
                    for Tin, lo, hi, is_open in per_layer[l]:
                        assert lo == at, (F, feeds, l)                                     # neither a gap nor a column twice
                        assert hi <= (_open_bound(Tin, k, s) if is_open else (Tin + 2 * (k // 2) - k) // s + 1), (F, feeds, l)
                        assert Tin <= Touts[l]
                        at = hi
                    assert at == Touts[l + 1], (F, feeds, l)
                fed = np.cumsum(feeds)
                want = [PK.enc_ready(int(f), False) for f in fed]
                want = want[:-1] + [Touts[-1]] if end_with_last else want + [Touts[-1]]
                assert ready == want, (F, feeds)
                assert sum(counts) == Touts[-1] and counts == list(np.diff([0] + ready))


def test_plan_of_many_clips_packs_the_new_latents_and_leaves_idle_layers_out():
    from wavenet_autoencoders_amd import packing as PK
    # clip 0: its first frame (nothing final behind block 0's input), clip 1: an empty feed, clip 2: frames 20 -> 25, clip 3: ends at 5
    clips = [(0, 0, False, 1, False), (40, 30, False, 30, False), (80, 20, False, 25, False), (160, 5, False, 5, True)]
    plan = PK.enc_feed_plan(clips)
    assert list(plan.ready) == [0, 4, 3, 2] and list(plan.q_cnt) == [0, 0, 2, 2] and list(plan.q_off) == [0, 0, 0, 2]
    assert plan.total_new == 4 and [ln.layer for ln in plan.launches] == list(range(11))
    lin = plan.records(len(plan.launches) - 1)
    assert lin[:2, :5].tolist() == [[20, 3, 0, 1, 3], [40, 2, 2, 0, 2]]
    first = plan.records(0)       # block 0 (k = 3): 1 frame makes 0 columns final, 25 make 24, the ended clip all 5
    assert first[:, :5].tolist()[:3] == [[80, 25, 80 + 19, 19, 24], [160, 5, 160 + 4, 4, 5], [0, 0, 0, 0, 0]]
    # block 0's whole table by hand: records of clips 2 and 3 (5 and 1 columns -> one tile of 8 each), the closing record
    assert plan.launches[0] == PK.EncFeedLaunch(0, 3, 1, 1, 8, 2, 2, 0)
    assert plan.table[:18].tolist() == [80, 25, 99, 19, 24, 0, 160, 5, 164, 4, 5, 1, 0, 0, 0, 0, 0, 2]
    # a function of the counts alone: other bases move in_off and out_col by base / div and nothing else; another order of the clips
    # permutes the records and re-runs the tile0 and packed-latent sums, and changes no record's range
    moved = PK.enc_feed_plan([(b + 400, f0, e0, f1, e1) for b, f0, e0, f1, e1 in clips])
    assert moved.launches == plan.launches and list(moved.ready) == list(plan.ready) and list(moved.q_off) == list(plan.q_off)
    for i, ln in enumerate(plan.launches):
        d = plan.records(i).astype(np.int64)
        m = moved.records(i).astype(np.int64)
        last = ln.layer == 10
        assert np.array_equal(m[:, [1, 3, 4, 5]], d[:, [1, 3, 4, 5]])
        assert np.array_equal(m[:-1, 0], d[:-1, 0] + 400 // PK.ENC_ARENA_DIV[ln.layer])
        assert np.array_equal(m[:-1, 2], d[:-1, 2] + (0 if last else 400 // PK.ENC_ARENA_DIV[ln.layer + 1]))
    back = PK.enc_feed_plan(clips[::-1])
    assert [(ln.layer, ln.et, ln.nrecs, ln.ntiles) for ln in back.launches] == [(ln.layer, ln.et, ln.nrecs, ln.ntiles) for ln in plan.launches]
    assert list(back.ready) == list(plan.ready)[::-1] and list(back.q_cnt) == [2, 2, 0, 0] and list(back.q_off) == [0, 2, 4, 4]
    for i, ln in enumerate(plan.launches):
        d, r = plan.records(i)[:-1], back.records(i)[:-1]
        cols = [0, 1, 3, 4] if ln.layer == 10 else [0, 1, 2, 3, 4]          # (lin's out_col is the packed offset: it follows the order)
        assert np.array_equal(r[::-1][:, cols], d[:, cols])
        per = -(-(r[:, 4] - r[:, 3]) // ln.et)
        assert r[:, 5].tolist() == np.concatenate([[0], np.cumsum(per)[:-1]]).tolist()
    idle = PK.enc_feed_plan([(0, 0, False, 1, False), (40, 30, False, 30, False)])
    assert idle.launches == [] and idle.table.size == 0 and idle.total_new == 0 and list(idle.ready) == [0, 4]
    for bad, text in (([(0, 3, False, 2, False)], "clip 0: base 0, frames 3 -> 2"),
                      ([(0, 1, False, 1, False), (4, 2, True, 3, True)], "clip 1: base 4, frames 2 -> 3, ended True -> True"),
                      ([(0, 2, True, 2, False)], "ended True -> False"),
                      ([(2, 0, False, 1, False)], "clip 0: base 2"),
                      ([(0, 0, False, 0, True)], "clip 0: base 0, frames 0 -> 0"),
                      ([(2 ** 31 - 4, 0, False, 4, False)], "reach 2^31")):
        with pytest.raises(ValueError, match=text.replace("^", r"\^")):
            PK.enc_feed_plan(bad)


def test_bases_of_neighbouring_clips_never_overlap_at_any_layer():
    """the session's placement: rooms are multiples of ENC_ROOM frames, so at every layer a clip's columns end where the next begins"""
    from wavenet_autoencoders_amd import packing as PK
    from wavenet_autoencoders_amd.encode import _room
    rng = np.random.default_rng(11)
    for _ in range(50):
        caps = [_room(int(rng.integers(1, 70))) for _ in range(6)]
        bases = np.concatenate([[0], np.cumsum(caps)[:-1]])
        frames = [int(rng.integers(1, c + 1)) for c in caps]
        plan = PK.enc_feed_plan([(int(b), 0, False, f, True) for b, f in zip(bases, frames)])
        for i, ln in enumerate(plan.launches):
            rec = plan.records(i)[:-1]
            d_in, d_out = PK.ENC_ARENA_DIV[ln.layer], PK.ENC_ARENA_DIV[ln.layer + 1]
            for j in range(len(caps) - 1):
                assert rec[j, 0] + rec[j, 1] <= bases[j + 1] // d_in == rec[j + 1, 0]                 # input columns
                if ln.layer < 10:
                    assert rec[j, 2] - rec[j, 3] + rec[j, 4] <= bases[j + 1] // d_out                  # output columns
            assert PK.enc_final_rows(caps[0], True)[ln.layer] <= caps[0] // d_in


# ---- the entry ------------------------------------------------------------------------------------------------------------------------
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
    assert "typedef struct wae_enc_range { int32_t in_off, Tin, out_col, t_lo, t_hi, tile0; } wae_enc_range;" in hdr
    comment = hdr[:hdr.index("typedef struct wae_enc_range")]
    comment = comment[comment.rindex("/*"):]
    for word in ("floor((n - k + p) / s) + 1", "(n + 2p - k) / s + 1", "max(0, (F - 13) / 4)", "(F + 3) / 4", "closing record",
                 "binary search", "is skipped", "before any launch", "WAE_EINVAL", "WAE_EUNSUPPORTED", "no \"open\" flag", "bit for bit"):
        assert word in comment, word


def _ranges(lib, x=PTR, w=PTR, bias=PTR, y=PTR, recs=PTR, nrecs=3, ntiles=5, et=16, in_pitch=100, out_pitch=100, Cin=39, Cout=64,
            k=3, stride=1, pad=1, relu=1, residual=0):
    return lib.wae_enc_conv_fwd_ranges(x, w, bias, y, recs, nrecs, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu,
                                       residual, None)


RANGES_EINVAL = [
    ("null_x", dict(x=None), b"bad arguments"),
    ("null_w", dict(w=None), b"bad arguments"),
    ("null_y", dict(y=None), b"bad arguments"),
    ("no_channels", dict(Cin=0), b"bad arguments"),
    ("no_outputs", dict(Cout=0), b"bad arguments"),
    ("k_0", dict(k=0), b"bad arguments"),
    ("stride_0", dict(stride=0), b"bad arguments"),
    ("negative_pad", dict(pad=-1), b"bad arguments"),
    ("null_recs", dict(recs=None), b"nrecs > 0 records"),
    ("no_recs", dict(nrecs=0), b"(got 0)"),
    ("no_tiles", dict(ntiles=0), b"ntiles must be > 0 (got 0)"),
    ("et_12", dict(et=12), b"et 12 is not 8, 16 or 32"),
    ("no_in_pitch", dict(in_pitch=0), b"pitches must be > 0 (got 0, 100)"),
    ("negative_out_pitch", dict(out_pitch=-1), b"pitches must be > 0 (got 100, -1)"),
    ("residual_other_width", dict(residual=1), b"residual needs a same-shape conv"),
    ("residual_strided", dict(residual=1, Cin=64, k=5, stride=2, pad=2), b"residual needs a same-shape conv"),
]


@pytest.mark.parametrize("case,text", [r[1:] for r in RANGES_EINVAL], ids=[r[0] for r in RANGES_EINVAL])
def test_ranges_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ranges(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"enc_conv_fwd_ranges: ") and text in err, err


@pytest.mark.parametrize("case", [dict(k=7, pad=3), dict(k=3, stride=2), dict(k=1, stride=4, pad=0)], ids=["k7", "k3s2", "k1s4"])
def test_ranges_entry_names_the_blocks_it_has(case):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ranges(lib, **case) == EUNSUPPORTED
    assert b"(1,1), (3,1), (5,2), (5,1)" in lib.wae_last_error()


# ---- the session's refusals, before a device is touched ---------------------------------------------------------------------------------
class _Lay:
    def __init__(self, c_in, hid, cc):
        from wavenet_autoencoders_amd import packing as PK
        self.shapes, ci = {}, c_in
        for i, (k, _) in enumerate(PK.ENCODER_BLOCKS):
            self.shapes[f"encoder.net.{i}.conv.weight"] = (hid, ci, k)
            ci = hid
        self.shapes["encoder.lin.weight"] = (cc, hid)


class _Eng:
    """as much of WaeEngine as EncodeSession reads before its first launch"""

    def __init__(self, **cfg):
        from wavenet_autoencoders_amd import Geometry
        base = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0,
                    encoder_hid=32, c_in=39, K=32)
        self.g = Geometry.from_cfg(dict(base, **cfg))
        self.device = "cpu"
        self.lay = _Lay(39, 32, 16)


def test_session_refuses_an_engine_without_an_encoder():
    from wavenet_autoencoders_amd.encode import EncodeSession
    with pytest.raises(ValueError, match="no encoder"):
        EncodeSession(_Eng(c_in=None, encoder_hid=None))


def test_feed_list_checks_every_feed_before_anything_is_launched():
    from wavenet_autoencoders_amd.encode import EncodeSession
    sess = EncodeSession(_Eng())
    a, b = sess.open(max_frames=6), sess.open()
    assert (a, b) == (0, 1) and sess.live == [0, 1]
    assert sess.clips[a].cap == 8 and sess.clips[a].base == 0 and sess._top == 8 and sess._cap >= 8       # room in multiples of 4 frames
    assert [t.shape for t in sess._ar][:5] == [(39, sess._cap), (32, sess._cap), (32, sess._cap), (32, sess._cap // 2), (32, sess._cap // 4)]
    assert len(sess._ar) == 11
    one = np.zeros((39, 1), dtype=np.float32)
    for feeds, ended, text in (
            ({7: one}, (), "clip 7 is not an open utterance"),
            ({a: np.zeros((38, 1))}, (), r"a feed is \(c_in, f\) = \(39, f\)"),
            ({a: np.zeros((1, 39, 1))}, (), r"a feed is \(c_in, f\)"),
            ({a: np.zeros(39)}, (), r"a feed is \(c_in, f\)"),
            ({a: np.zeros((39, 7))}, (), r"7 frames are beyond max_frames \(6\)"),
            ({a: one}, (9,), "clip 9 is not an open utterance"),
            ({a: one}, (b,), "clip 1 ends without frames"),
            ({}, (a,), "clip 0 ends without frames"),
            ({b: np.zeros((39, 0))}, (b,), "clip 1 ends without frames")):
        with pytest.raises(ValueError, match=text):
            sess.feed_list(feeds, ended=ended)
    assert all(c.frames == 0 and c.final == 0 for c in sess.clips.values()) and sess.live == [0, 1]
    with pytest.raises(ValueError, match="max_frames 0 < 1"):
        sess.open(max_frames=0)
    assert sess.feed_list({}) == {}
    sess.drop(a)
    with pytest.raises(ValueError, match="clip 0 is not an open utterance"):
        sess.feed(a, one)
    for gone in (a, 7):
        with pytest.raises(ValueError, match=f"drop: clip {gone} is not an open utterance"):
            sess.drop(gone)
    sess.drop(b)
    assert sess._top == 0
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.open()
    with pytest.raises(RuntimeError, match="closed"):
        sess.feed_list({})
    with pytest.raises(RuntimeError, match="closed"):
        sess.drop(b)
    with pytest.raises(RuntimeError, match="closed"):
        sess.reserve_frames(8)
    sess.close()                                                             # closing twice is harmless


POS = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]


@pytest.mark.parametrize("extra,word", [(["--batch-decode", "--feed-features", "4"], "it needs both"),
                                        (["--feed-features", "4"], "it needs both"),
                                        (["--batch-decode", "--batch-stream", "700", "--feed-features", "0"], "feature frames (>= 1)"),
                                        (["--batch-decode", "--batch-stream", "700", "--feed-features", "4", "--feed-frames", "1"],
                                         "cannot be combined")],
                         ids=["without_stream", "without_batch", "zero_frames", "with_feed_frames"])
def test_synthesis_argument_errors(extra, word, capsys):
    sys.path.insert(0, ROOT)
    import synthesis
    with pytest.raises(SystemExit) as e:
        synthesis.main(POS + extra)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_surface_and_documents():
    from wavenet_autoencoders_amd.encode import EncodeSession
    from wavenet_autoencoders_amd.engine import WaeEngine
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    for name in ("open", "feed", "feed_list", "end", "drop", "close", "reserve_frames", "__enter__", "__exit__"):
        assert callable(getattr(EncodeSession, name)), name
    doc = EncodeSession.feed_list.__doc__
    for word in ("encode_list([whole])[0]", "beyond max_frames", "without frames", "final", "done"):
        assert word in doc, word
    assert "feed_list" in WaeEngine.encode_session.__doc__ and callable(VQVAE.encode_session)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.4.4" in design and "wae_enc_range" in design
    assert "encode_session" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "--feed-features" in open(os.path.join(ROOT, "README.md")).read()
    assert "--feed-features" in open(os.path.join(ROOT, "synthesis.py")).read()
