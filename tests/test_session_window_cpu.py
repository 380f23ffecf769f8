"""Sessions in constant memory (wae_enc_conv_fwd_rings, wae_upsample_stage_fwd_rings, packing.enc_feed_plan_rings,
EncodeSession(window=W)) without a GPU: a simulation of the rings -- every arena an array of "which column of which utterance does
this slot hold" tags, driven by the ring plans over random interleaved feeding schedules: every tap of every record hits a slot that
holds exactly that column, slots of two utterances never overlap, the ranges tile every layer once --, the closed forms against brute
force, the ring records against the ranges plan's, the entries' declaration, binding and refusals before any launch (raw ctypes calls
with dummy pointers) and the session's refusals that need no device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = ctypes.c_void_p(0x1000)
EINVAL, EUNSUPPORTED = -1, -2


# ---- 1. the rings, simulated ------------------------------------------------------------------------------------------------------------
class _EncRings:
    """the arenas of a windowed encode session as tags: arena l, column i -> (utterance, column) or None"""

    def __init__(self, window, nslots):
        from wavenet_autoencoders_amd import packing as PK
        self.PK, self.W = PK, window
        self.periods = PK.enc_ring_periods(window)
        self.tags = [[None] * (nslots * p) for p in self.periods]
        self.reads = 0

    def feed(self, clips):
        """clips: (name, slot, frames_before, frames, ended) -> the plan; asserts every read, then performs every write"""
        PK = self.PK
        plan = PK.enc_feed_plan_rings([(s, f0, False, f1, e) for _, s, f0, f1, e in clips], self.W)
        p0 = self.periods[0]
        for name, s, f0, f1, _ in clips:                     # the upload of the new frames
            for u in range(f0, f1):
                self.tags[0][s * p0 + u % p0] = (name, u)
        by_slot = {s: name for name, s, *_ in clips}
        ranges = {}
        for i, ln in enumerate(plan.launches):
            recs = PK.ring_records(plan, i)
            k, st = PK.ENC_LAYERS[ln.layer]
            assert (ln.k, ln.stride, ln.pad) == (k, st, k // 2) and ln.et in PK.ENC_LIST_ETS
            assert int(recs[-1, 7]) == ln.ntiles and recs.dtype == np.int32
            last = ln.layer == len(PK.ENC_LAYERS) - 1
            tile0 = 0
            for in_off, in_per, Tin, out_off, out_per, lo, hi, t0 in (tuple(int(v) for v in r) for r in recs[:-1]):
                assert in_per == self.periods[ln.layer] and in_off % in_per == 0 and lo < hi and t0 == tile0
                tile0 += -(-(hi - lo) // ln.et)
                name = by_slot[in_off // in_per]
                assert last == (out_per == 0)
                if not last:
                    assert out_per == self.periods[ln.layer + 1] and out_off == (in_off // in_per) * out_per
                for t in range(lo, hi):
                    for u in range(t * st - k // 2, t * st - k // 2 + k):
                        if 0 <= u < Tin:                     # (outside: the utterance's zero padding, no read)
                            assert self.tags[ln.layer][in_off + u % in_per] == (name, u), (ln.layer, name, t, u)
                            self.reads += 1
                if not last:
                    for t in range(lo, hi):
                        self.tags[ln.layer + 1][out_off + t % out_per] = (name, t)
                ranges[(name, ln.layer)] = (Tin, lo, hi, out_off)
            assert tile0 == ln.ntiles
        return plan, ranges


def _schedule(rng, window, rounds, names):
    """random interleaved lives: per round, who joins, who is fed how much, who ends (with or behind its frames), who is dropped"""
    from wavenet_autoencoders_amd import packing as PK
    max_feed = PK.enc_window_max_feed(window)
    live, nxt = {}, 0
    for _ in range(rounds):
        if nxt < names and len(live) < 4 and (len(live) < 2 or rng.random() < 0.3):
            live[nxt] = 0
            nxt += 1
        acts = []
        for name in list(live):
            r = rng.random()
            n = int(rng.choice([1, int(rng.integers(1, max_feed + 1)), max_feed]))
            if live[name] > 40 and r < 0.15:
                acts.append((name, n if r < 0.08 else 0, True, False))
                del live[name]
            elif r > 0.97:
                acts.append((name, 0, False, True))          # dropped
                del live[name]
            elif r > 0.2:
                acts.append((name, n, False, False))
                live[name] += n
        yield acts
    yield [(name, 0, True, False) for name in live if live[name] > 0]


@pytest.mark.parametrize("window", [16, 32])
def test_every_tap_of_every_record_hits_the_slot_that_holds_its_column(window):
    from wavenet_autoencoders_amd import packing as PK
    rng = np.random.default_rng(window)
    nslots = 4
    rings = _EncRings(window, nslots)
    free, slot, frames, at, ended_lens = list(range(nslots - 1, -1, -1)), {}, {}, {}, {}
    reused, used = 0, set()
    for acts in _schedule(rng, window, 400, 24):
        call = []
        for name, n, end, drop in acts:
            if name not in slot:
                assert free, "the schedule holds at most nslots utterances"
                slot[name], frames[name] = free.pop(), 0
                at[name] = [0] * len(PK.ENC_LAYERS)
                reused += slot[name] in used                 # a ring that another utterance left
                used.add(slot[name])
            if drop:
                free.append(slot.pop(name))
                continue
            if n or end:
                call.append((name, slot[name], frames[name], frames[name] + n, end))
        assert len(set(slot.values())) == len(slot) and not set(slot.values()) & set(free)       # two open utterances never share a ring
        if not call:
            continue
        plan, ranges = rings.feed(call)
        for j, (name, s, f0, f1, end) in enumerate(call):
            frames[name] = f1
            assert int(plan.ready[j]) == PK.enc_ready(f1, end)
            for l in range(len(PK.ENC_LAYERS)):
                final = PK.enc_final_rows(f1, end)[l + 1]
                if (name, l) in ranges:
                    Tin, lo, hi, _ = ranges[(name, l)]
                    assert lo == at[name][l] and hi == final and Tin == PK.enc_final_rows(f1, end)[l]      # neither a gap nor a column twice
                    at[name][l] = hi
                assert at[name][l] == final
            if end:
                ended_lens[name] = f1
                free.append(slot.pop(name))
    assert len(ended_lens) > 8 and max(ended_lens.values()) > 4 * window and reused > 4 and rings.reads > 10000


# ---- 2. the closed forms ------------------------------------------------------------------------------------------------------------------
def test_lag_tail_and_span_are_the_brute_force_maxima():
    from wavenet_autoencoders_amd import packing as PK
    L = PK.ENC_LAYERS
    forms = PK._enc_final_forms()
    lag, tail = [0] * len(L), [0] * len(L)
    for F in range(1, 201):
        op, en = PK.enc_final_rows(F, False), PK.enc_final_rows(F, True)
        for l, (k, s) in enumerate(L):
            assert op[l] == max(0, (F - forms[l][0]) // forms[l][1] + 1) and en[l] == (F - 1) // forms[l][1] + 1
            lag[l] = max(lag[l], op[l] - max(op[l + 1] * s - k // 2, 0))
            tail[l] = max(tail[l], en[l] - op[l])
    assert lag == PK.enc_window_lag() and tail == PK.enc_window_tail()
    assert forms[-1] == (17, 4)                                              # enc_ready: (F - 13) // 4 = (F - 17) // 4 + 1
    for n in (1, 2, 4, 5, 16, 17, 64):
        worst = 0
        for F in range(0, 201):
            b, a = PK.enc_final_rows(F, False), PK.enc_final_rows(F + n, False)
            worst = max(worst, max((a[l] - max(b[l + 1] * s - k // 2, 0)) * PK.ENC_ARENA_DIV[l] for l, (k, s) in enumerate(L)))
        assert worst == PK.enc_window_span(n), n
    assert PK.enc_window_min() == PK.enc_window_span(1) == max(d * g for d, g in zip(PK.ENC_ARENA_DIV, lag)) + PK.ENC_ROOM


@pytest.mark.parametrize("window", [12, 16, 32])
def test_max_feed_is_exact_and_the_window_is_tight(window, monkeypatch):
    from wavenet_autoencoders_amd import packing as PK
    mf, periods = PK.enc_window_max_feed(window), PK.enc_ring_periods(window)
    assert PK.enc_window_span(mf) <= window < PK.enc_window_span(mf + 1)
    assert periods == [window // d + t for d, t in zip(PK.ENC_ARENA_DIV, PK.enc_window_tail())]
    held = [0] * len(periods)
    for F in range(0, 130):
        for n in range(0, mf + 1):
            for end in (False, True):
                if F + n < 1:
                    continue
                PK.enc_feed_plan_rings([(1, F, False, F + n, end)], window)                  # never raises within max_feed
                b, a = PK.enc_final_rows(F, False), PK.enc_final_rows(F + n, end)
                for l, (k, s) in enumerate(PK.ENC_LAYERS):
                    held[l] = max(held[l], a[l] - max(b[l + 1] * s - k // 2, 0))
        with pytest.raises(ValueError, match=f"a feed of {mf + 1} frames; a window of {window} admits {mf} per call"):
            PK.enc_feed_plan_rings([(0, F, False, F + mf + 1, False)], window)
    assert all(h <= p for h, p in zip(held, periods)) and any(h == p for h, p in zip(held, periods))      # some ring is full at the worst
    if window > PK.enc_window_min():         # one ENC_ROOM less: the same feed is refused
        with pytest.raises(ValueError, match="admits"):
            PK.enc_feed_plan_rings([(0, 40, False, 40 + mf, False)], window - PK.ENC_ROOM)
    for bad in (window + 1, PK.enc_window_min() - PK.ENC_ROOM, 0):
        with pytest.raises(ValueError, match=f"at least {PK.enc_window_min()}"):
            PK.enc_ring_periods(bad)
    # the retention check itself, with the feed limit out of its way: the first feed it refuses, at the worst phase, is max_feed + 1
    monkeypatch.setattr(PK, "enc_window_max_feed", lambda w: 10 ** 6)
    first = None
    for n in range(1, 2 * window):
        try:
            for F in range(0, 60):
                PK.enc_feed_plan_rings([(0, F, False, F + n, True)], window)
        except ValueError as e:
            assert "would hold" in str(e) and "in a ring of" in str(e)
            first = n
            break
    assert first == mf + 1


# ---- 3. the records against the ranges plan ---------------------------------------------------------------------------------------------
def test_ring_records_of_a_window_that_holds_the_whole_clip_are_the_ranges_plans():
    from wavenet_autoencoders_amd import packing as PK
    window = 64
    mf = PK.enc_window_max_feed(window)
    periods = PK.enc_ring_periods(window)
    rng = np.random.default_rng(3)
    for _ in range(20):
        F = [0, 0, 0]
        while min(F) < 40:
            n = [int(rng.integers(0, min(mf, 12) + 1)) for _ in F]
            end = [f + k >= 40 for f, k in zip(F, n)]
            ring = PK.enc_feed_plan_rings([(i, f, False, f + k, e) for i, (f, k, e) in enumerate(zip(F, n, end))], window)
            flat = PK.enc_feed_plan([(i * 64, f, False, f + k, e) for i, (f, k, e) in enumerate(zip(F, n, end))])
            assert [ln[:7] for ln in ring.launches] == [ln[:7] for ln in flat.launches]      # (rec_off differs: records of 8)
            assert list(ring.ready) == list(flat.ready) and list(ring.q_off) == list(flat.q_off) and ring.total_new == flat.total_new
            for i, ln in enumerate(flat.launches):
                a, b = PK.ring_records(ring, i).astype(np.int64), flat.records(i).astype(np.int64)
                last = ln.layer == len(PK.ENC_LAYERS) - 1
                assert np.array_equal(a[:, [2, 5, 6, 7]], b[:, [1, 3, 4, 5]])             # Tin, t_lo, t_hi, tile0
                slot = a[:-1, 0] // periods[ln.layer]
                assert np.array_equal(slot * (64 // PK.ENC_ARENA_DIV[ln.layer]), b[:-1, 0])  # the same clip's columns
                assert (a[:-1, 6] <= periods[ln.layer + 1]).all() if not last else True      # no column wraps: u % period == u
                if last:
                    assert np.array_equal(a[:-1, 3], b[:-1, 2]) and (a[:-1, 4] == 0).all()   # the packed latents, linear
                else:                                                                        # out_off + t_lo % period against base + t_lo
                    assert np.array_equal(a[:-1, 3] + a[:-1, 5] - slot * periods[ln.layer + 1],
                                          b[:-1, 2] - slot * (64 // PK.ENC_ARENA_DIV[ln.layer + 1]))
            F = [40 if e else f + k for f, k, e in zip(F, n, end)]
            if all(end):
                break


# ---- 4. the entries -------------------------------------------------------------------------------------------------------------------------
ENC = ("wae_enc_conv_fwd_rings", "wae_enc_ring",
       ["const float* x", "const float* w", "const float* bias", "float* y", "const wae_enc_ring* recs", "int32_t nrecs", "int32_t ntiles",
        "int32_t et", "int32_t in_pitch", "int32_t out_pitch", "int32_t Cin", "int32_t Cout", "int32_t k", "int32_t stride", "int32_t pad",
        "int32_t relu", "int32_t residual", "void* stream"])
UPS = ("wae_upsample_stage_fwd_rings", "wae_ups_ring",
       ["const float* in", "const float* w", "void* out", "const wae_ups_ring* recs", "int32_t nrecs", "int32_t ntiles", "int32_t in_pitch",
        "int32_t out_pitch_or_rows", "int32_t C", "int32_t s", "int32_t out_btc", "int32_t Cp", "int32_t dtype", "void* stream"])


@pytest.mark.parametrize("entry,record,want", [ENC, UPS], ids=["encoder", "upsampling"])
def test_entries_are_exported_declared_and_bound(entry, record, want):
    from wavenet_autoencoders_amd import _lib
    from wavenet_autoencoders_amd import packing as PK
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
    assert res is i32 and list(bound) == args and list(getattr(_lib.lib(), entry).argtypes) == args
    struct = f"typedef struct {record} {{ int32_t in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0; }} {record};"
    assert struct in hdr                                                     # 8 x int32 = 32 bytes, the planner's row
    plan = PK.enc_feed_plan_rings([(0, 0, False, 20, True)], 32)
    assert PK.ring_records(plan, 0).shape[1] * plan.table.itemsize == 32
    comment = hdr[:hdr.index(f"typedef struct {record}")]
    comment = comment[comment.rindex("/*"):]
    for word in ("% in_period", "% out_period", "is skipped", "aliasing", "older than Tin - in_period", "before any launch", "WAE_EINVAL",
                 "WAE_EUNSUPPORTED", "bit for bit", "whatever the periods"):
        assert word in comment, word


def _enc(lib, x=PTR, w=PTR, bias=PTR, y=PTR, recs=PTR, nrecs=3, ntiles=5, et=16, in_pitch=100, out_pitch=100, Cin=39, Cout=64, k=3,
         stride=1, pad=1, relu=1, residual=0):
    return lib.wae_enc_conv_fwd_rings(x, w, bias, y, recs, nrecs, ntiles, et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu,
                                      residual, None)


ENC_EINVAL = [
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


@pytest.mark.parametrize("case,text", [r[1:] for r in ENC_EINVAL], ids=[r[0] for r in ENC_EINVAL])
def test_encoder_rings_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _enc(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"enc_conv_fwd_rings: ") and text in err, err


@pytest.mark.parametrize("case", [dict(k=7, pad=3), dict(k=3, stride=2), dict(k=1, stride=4, pad=0)], ids=["k7", "k3s2", "k1s4"])
def test_encoder_rings_entry_names_the_blocks_it_has(case):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _enc(lib, **case) == EUNSUPPORTED
    assert b"(1,1), (3,1), (5,2), (5,1)" in lib.wae_last_error()


def _ups(lib, inp=PTR, w=PTR, out=PTR, recs=PTR, nrecs=3, ntiles=5, in_pitch=100, rows=400, C=16, s=4, out_btc=1, Cp=64, dtype=1):
    return lib.wae_upsample_stage_fwd_rings(inp, w, out, recs, nrecs, ntiles, in_pitch, rows, C, s, out_btc, Cp, dtype, None)


UPS_EINVAL = [
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


@pytest.mark.parametrize("case,text", [r[1:] for r in UPS_EINVAL], ids=[r[0] for r in UPS_EINVAL])
def test_upsampling_rings_entry_refuses_before_any_launch(case, text):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ups(lib, **case) == EINVAL
    err = lib.wae_last_error()
    assert err.startswith(b"upsample_stage_fwd_rings: ") and text in err, err


@pytest.mark.parametrize("case", [dict(C=130, Cp=192), dict(C=16, Cp=512), dict(s=86), dict(C=200, Cp=256, s=1)],
                         ids=["cp_192", "cp_512", "3s_258", "lds_beyond_64k"])
def test_upsampling_rings_entry_names_what_the_time_major_kernel_takes(case):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _ups(lib, **case) == EUNSUPPORTED
    err = lib.wae_last_error()
    assert b"Cp dividing 256" in err and b"3 s <= 256" in err, err


# ---- the session's refusals, before a device is touched ---------------------------------------------------------------------------------
def _session(window):
    from test_encode_session_cpu import _Eng
    from wavenet_autoencoders_amd.encode import EncodeSession
    return EncodeSession(_Eng(), window=window)


def test_windowed_session_refuses_before_anything_is_launched():
    from wavenet_autoencoders_amd import packing as PK
    for bad in (8, 18, 0, -4):
        with pytest.raises(ValueError, match=r"a multiple of 4 feature frames, at least 12 \(the 8 the layers retain and 4 of feed\)"):
            _session(bad)
    sess = _session(16)
    assert sess.max_feed == 8 == PK.enc_window_max_feed(16) and sess.arena_bytes == 0
    a, b = sess.open(), sess.open(max_frames=100)
    periods = PK.enc_ring_periods(16)
    chans = [39] + [32] * 10
    assert [tuple(t.shape) for t in sess._ar] == [(c, 4 * p) for c, p in zip(chans, periods)]     # four rings to begin with
    assert sess.arena_bytes == 4 * 4 * sum(c * p for c, p in zip(chans, periods))
    assert (sess.clips[a].slot, sess.clips[b].slot) == (0, 1)
    before = [t.data_ptr() for t in sess._ar]
    for feeds, ended, text in (
            ({a: np.zeros((39, 9), dtype=np.float32)}, (), r"a feed of 9 frames; a window of 16 admits max_feed = 8 per call"),
            ({a: np.zeros((39, 8)), b: np.zeros((39, 9))}, (), r"clip 1: a feed of 9 frames"),
            ({b: np.zeros((39, 1))}, (a,), "clip 0 ends without frames"),
            ({a: np.zeros((38, 1))}, (), r"a feed is \(c_in, f\) = \(39, f\)")):
        with pytest.raises(ValueError, match=text):
            sess.feed_list(feeds, ended=ended)
    assert all(c.frames == 0 and c.final == 0 for c in sess.clips.values()) and sess.live == [0, 1]
    assert [t.data_ptr() for t in sess._ar] == before
    with pytest.raises(ValueError, match="reserves rings"):
        sess.reserve_frames(64)
    with pytest.raises(ValueError, match="reserves frames"):
        _session(None).reserve_slots(4)
    # a slot freed by ANY utterance goes to the next one; a fifth utterance at once doubles the rings
    c = sess.open()
    sess.drop(a)
    d = sess.open()
    assert sess.clips[d].slot == 0 and sess.clips[c].slot == 2 and sess._nslots == 4
    e, f = sess.open(), sess.open()
    assert (sess.clips[e].slot, sess.clips[f].slot) == (3, 4) and sess._nslots == 8
    assert sess.arena_bytes == 8 * 4 * sum(ch * p for ch, p in zip(chans, periods))
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.reserve_slots(2)


def test_surface_and_documents():
    from wavenet_autoencoders_amd.encode import EncodeSession
    from wavenet_autoencoders_amd.engine import WaeEngine
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    import inspect
    assert "window" in inspect.signature(WaeEngine.encode_session).parameters
    assert "window" in inspect.signature(VQVAE.encode_session).parameters
    assert "window" in inspect.signature(EncodeSession.__init__).parameters
    for word in ("window=W", "max_feed", "arena_bytes", "slot * period + u % period"):
        assert word in EncodeSession.__doc__, word
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "3.4.5" in design and "wae_enc_ring" in design and "wae_ups_ring" in design
    assert "window=" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "window=" in open(os.path.join(ROOT, "README.md")).read()


# ---- the decode side: packing.session_feed_plan_rings, DecodeSession(window=W) ----------------------------------------------------------
SCALES = [[4, 4, 8, 5], [2, 3], [4, 4, 4, 5]]


@pytest.mark.parametrize("scales", SCALES, ids=["4x4x8x5", "2x3", "4x4x4x5"])
def test_every_frame_every_stage_record_reads_is_in_its_slot(scales):
    """the encoder's simulation for the upsampling chain: stage arenas and the c_up ring as tags; a clip decodes (pos moves) between
    the feeds, feeds stay within room, and no row is overwritten before it is decoded"""
    from wavenet_autoencoders_amd import packing as PK
    W, nslots = 4, 3
    mul = [int(np.prod(scales[:i])) for i in range(len(scales) + 1)]
    prod, look = PK.feed_lookahead(scales)
    mf = PK.feed_window_max_feed(scales, W)
    tags = [[None] * (nslots * W * m) for m in mul]
    rng = np.random.default_rng(len(scales))
    free, clips, nxt, ended_n, reads = list(range(nslots - 1, -1, -1)), {}, 0, 0, 0
    for _ in range(300):
        if free and nxt < 12 and rng.random() < 0.5:
            clips[nxt] = dict(slot=free.pop(), planned=0, ep=False, frames=0, ended=False, pos=0, at=[0] * len(scales), decoded=0)
            nxt += 1
        call = []
        for name, c in list(clips.items()):
            if rng.random() < 0.03:                          # dropped
                free.append(clips.pop(name)["slot"])
                continue
            room = max(0, min(mf, (c["pos"] + W * prod + look) // prod + 1 - c["frames"]))
            n = 0 if c["ended"] else min(room, int(rng.integers(0, mf + 1)))
            if not c["ended"] and c["frames"] + n > 6 and rng.random() < 0.2 and (c["frames"] + n) * prod - c["pos"] <= W * prod:
                c["ended"] = True
            if n or c["ended"] != c["ep"]:
                for u in range(c["frames"], c["frames"] + n):
                    tags[0][c["slot"] * W + u % W] = (name, u)
                c["frames"] += n
                call.append(name)
        assert len({c["slot"] for c in clips.values()}) == len(clips) and not {c["slot"] for c in clips.values()} & set(free)
        if call:
            plan = PK.session_feed_plan_rings(scales, [(clips[n_]["slot"], clips[n_]["planned"], clips[n_]["ep"], clips[n_]["frames"],
                                                        clips[n_]["ended"], clips[n_]["pos"]) for n_ in call], W)
            by_slot = {clips[n_]["slot"]: n_ for n_ in call}
            for i, ln in enumerate(plan.launches):
                recs = PK.ring_records(plan, i)
                s = scales[ln.stage]
                tile = 64 if ln.last else 256
                assert ln.s == s and ln.last == (ln.stage == len(scales) - 1) and int(recs[-1, 7]) == ln.ntiles
                t0 = 0
                for in_off, in_per, Tin, out_off, out_per, lo, hi, tile0 in (tuple(int(v) for v in r) for r in recs[:-1]):
                    name = by_slot[in_off // in_per]
                    c = clips[name]
                    assert in_per == W * mul[ln.stage] and out_per == W * mul[ln.stage + 1] and in_off == c["slot"] * in_per
                    assert out_off == c["slot"] * out_per and tile0 == t0 and lo == c["at"][ln.stage] and lo < hi
                    assert hi <= (Tin * s if c["ended"] else (Tin - 1) * s)              # the guarantee the kernel asks of the host
                    t0 += -(-(hi - lo) // tile)
                    for t in range(lo, hi):
                        for f in range(max(t - s, 0) // s, min(t + s, Tin * s - 1) // s + 1):
                            assert tags[ln.stage][in_off + f % in_per] == (name, f), (ln.stage, name, t, f)
                            reads += 1
                    for t in range(lo, hi):
                        if ln.last:                          # never over a row the clip has not decoded
                            old = tags[-1][out_off + t % out_per]
                            assert old is None or old[0] != name or old[1] < c["pos"], (name, t, old, c["pos"])
                        tags[ln.stage + 1][out_off + t % out_per] = (name, t)
                    c["at"][ln.stage] = hi
            for j, n_ in enumerate(call):
                c = clips[n_]
                c["planned"], c["ep"] = c["frames"], c["ended"]
                assert int(plan.ready[j]) == PK.feed_ready(c["frames"], scales, c["ended"]) == c["at"][-1]
        for name, c in list(clips.items()):                  # a round of decoding: every row read is the clip's own
            ready = c["at"][-1]
            n = min(ready - c["pos"], int(rng.integers(0, 2 * prod)))
            for t in range(c["pos"], c["pos"] + n):
                assert tags[-1][c["slot"] * W * prod + t % (W * prod)] == (name, t)
            c["pos"] += n
            if c["ep"] and c["pos"] == c["frames"] * prod:
                ended_n += 1
                free.append(clips.pop(name)["slot"])
    assert ended_n > 5 and reads > 2000


@pytest.mark.parametrize("scales", SCALES + [[5], [1, 1], [8, 2]], ids=lambda s: "x".join(map(str, s)))
def test_decode_lag_and_max_feed_are_the_brute_force_values(scales):
    from wavenet_autoencoders_amd import packing as PK
    mul = [int(np.prod(scales[:i])) for i in range(len(scales) + 1)]
    lag = [0] * len(scales)
    for F in range(1, 201):
        r = PK.feed_final_rows(F, scales, False)
        for i, s in enumerate(scales):
            lag[i] = max(lag[i], r[i] - max(r[i + 1] // s - 1, 0))
    assert lag == PK.feed_window_lag(scales) == [2] * len(scales)
    for k in range(0, 7):
        worst = [0] * len(scales)
        for F in range(0, 40):
            for end in (False, True):
                if F + k >= 1:
                    b, a = PK.feed_final_rows(F, scales, False), PK.feed_final_rows(F + k, scales, end)
                    worst = [max(w, a[i] - max(b[i + 1] // s - 1, 0)) for i, (w, s) in enumerate(zip(worst, scales))]
        assert worst == PK.feed_window_held(scales, k)
    Wmin = PK.feed_window_min(scales)
    prod, look = PK.feed_lookahead(scales)
    assert PK.feed_window_max_feed(scales, Wmin) >= 1 and Wmin * prod >= look + prod
    assert PK.feed_window_max_feed(scales, Wmin - 1) < 1 or (Wmin - 1) * prod < look + prod          # tight: one frame less is refused
    with pytest.raises(ValueError, match=f"below the minimum of {Wmin} latent frames"):
        PK.session_feed_plan_rings(scales, [(0, 0, False, 1, False, 0)], Wmin - 1)
    for W in (Wmin, Wmin + 3):
        mf = PK.feed_window_max_feed(scales, W)
        for F in range(0, 12):
            for end in (False, True):
                PK.session_feed_plan_rings(scales, [(1, F, False, F + mf, end, 10 ** 9)], W)      # (pos far ahead: the stage rings alone)
        with pytest.raises(ValueError, match=f"would hold .*a window of {W} admits {mf} frames per call"):
            for F in range(0, 12):
                PK.session_feed_plan_rings(scales, [(1, F, False, F + mf + 1, True, 10 ** 9)], W)
    # back-pressure: final rows beyond pos + the ring
    W = Wmin + 1
    PK.session_feed_plan_rings(scales, [(0, 1, False, W, False, 0)], W + 8)
    with pytest.raises(ValueError, match="step first"):
        PK.session_feed_plan_rings(scales, [(0, 4, False, 5, False, 0)], Wmin) if PK.feed_ready(5, scales, False) > Wmin * prod \
            else PK.session_feed_plan_rings(scales, [(0, Wmin + 2, False, Wmin + 3, False, 0)], Wmin)


def test_decode_ring_records_of_a_window_that_holds_the_whole_clip_are_the_ranges_plans():
    from wavenet_autoencoders_amd import packing as PK
    scales, W = [4, 4, 8, 5], 32
    mul = [int(np.prod(scales[:i])) for i in range(len(scales) + 1)]
    rng = np.random.default_rng(8)
    F, ended = [0, 0, 0], [False] * 3
    while not all(ended):
        n = [0 if e else int(rng.integers(0, 7)) for e in ended]
        end = [e or (f + k >= 20) for e, f, k in zip(ended, F, n)]
        ring = PK.session_feed_plan_rings(scales, [(i, F[i], ended[i], F[i] + n[i], end[i], 0) for i in range(3)], W)
        flat = PK.session_feed_plan(scales, [(i * W, F[i], ended[i], F[i] + n[i], end[i]) for i in range(3)])
        assert [ln[:5] for ln in ring.launches] == [ln[:5] for ln in flat.launches] and list(ring.ready) == list(flat.ready)
        for i, ln in enumerate(flat.launches):
            a, b = PK.ring_records(ring, i).astype(np.int64), flat.records(i).astype(np.int64)
            assert np.array_equal(a[:, [0, 2, 3, 5, 6, 7]], b)               # no column wraps: the same columns, ranges and tiles
            assert (a[:-1, 1] == W * mul[ln.stage]).all() and (a[:-1, 4] == W * mul[ln.stage + 1]).all()
        F, ended = [f + k for f, k in zip(F, n)], end


def test_windowed_decode_session_refusals_need_no_device():
    from test_session_feed_cpu import _Eng
    from wavenet_autoencoders_amd.decode import DecodeSession
    import inspect
    from wavenet_autoencoders_amd.engine import WaeEngine
    with pytest.raises(ValueError, match=r"window 2 is below the minimum of 3 latent frames \(the c_up ring holds the 205 rows"):
        DecodeSession(_Eng(), mode="sample", window=2)
    sess = DecodeSession(_Eng(), mode="sample", window=4)
    assert sess.max_feed == 2 and sess.arena_bytes == 0 and not sess._open
    assert "window" in inspect.signature(WaeEngine.decode_session).parameters
    for name in ("room", "cond_rows", "arena_bytes"):
        assert hasattr(DecodeSession, name)
    for word in ("window=W", "max_feed", "room(h)", "slot * period + u % period", "back-pressure"):
        assert word in DecodeSession.__doc__, word


POS = ["dump", "ck.pth", "out/", "syn.txt", "spk.json", "english", "160", "25", "0"]


@pytest.mark.parametrize("extra", [["--batch-decode", "--batch-stream", "700", "--batch-window", "4"],
                                   ["--batch-decode", "--batch-stream", "700", "--feed-frames", "2", "--batch-window", "0"],
                                   ["--batch-window", "4"]], ids=["without_a_feed_flag", "zero", "alone"])
def test_batch_window_argument_errors(extra, capsys):
    import sys
    sys.path.insert(0, ROOT)
    import synthesis
    with pytest.raises(SystemExit) as e:
        synthesis.main(POS + extra)
    assert e.value.code == 2
    assert "--batch-window holds the fed clips in rings" in capsys.readouterr().err
