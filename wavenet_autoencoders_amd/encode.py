"""Encode sessions: utterances whose feature frames arrive while they are encoded (include/wae.h: wae_enc_conv_fwd_ranges;
DESIGN.md 3.4.4).  The counterpart of decode.DecodeSession.open / feed_list / end on the encoder's side: WaeEngine.encode_list needs
every utterance complete; a session takes the frames as they come and hands out, per call, the latent frames that no later feature
frame can change -- bit for bit encoder_forward + vq_forward of the whole utterance, whatever the feeding."""
import dataclasses
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import frontend as F
from . import packing as P


@dataclasses.dataclass
class _EncClip:
    """One open utterance of an EncodeSession."""
    base: int = 0                   # its first column in layer 0's arena, in feature frames (a multiple of P.ENC_ROOM)
    cap: int = 0                    # feature frames it has room for (a multiple of P.ENC_ROOM)
    frames: int = 0                 # feature frames fed so far
    final: int = 0                  # latent frames handed out so far
    max_frames: Optional[int] = None
    slot: int = -1                  # a windowed session: the clip's ring in every arena


def _room(n):
    return -(-int(n) // P.ENC_ROOM) * P.ENC_ROOM


class EncodeSession:
    """WaeEngine.encode_session: utterances join open (open), feature frames are appended as they arrive (feed / feed_list) and every
    call returns the latent frames -- with their codes and quantised latents -- that no later frame can change: max(0, (F - 13) // 4)
    of an utterance that is open with F frames, all (F + 3) // 4 once it has ended (packing.enc_ready).  One feed_list is one packed
    upload of the new frames, one table upload, at most eleven wae_enc_conv_fwd_ranges launches and one quantiser call, however many
    utterances it feeds.  Every layer's activations of the open utterances live in per-layer channel-major arenas (layer l's input:
    (C_l, room / ENC_ARENA_DIV[l]) fp32); they grow geometrically, copying what the open utterances have so far, and are not trimmed
    while an utterance is open -- about 4.25 columns of encoder_hid floats per feature frame.  An utterance's room is returned when it
    has ended and its last chunk has been handed out (or with drop).  Room is reused from the top only, as in DecodeSession: the
    columns of an utterance that ended or moved BELOW the top one stay unused until the utterances above it have left, and the top
    falls to 0 when the session is empty -- a session that always holds an old utterance keeps growing; close it and open another
    at a quiet moment, or give max_frames so that utterances never move.
    window=W (feature frames, a multiple of packing.ENC_ROOM, at least packing.enc_window_min()): a session in constant memory
    (include/wae.h: wae_enc_conv_fwd_rings).  Every open utterance owns a RING of packing.enc_ring_periods(W)[l]
    columns in layer l's arena -- W / ENC_ARENA_DIV[l] and the few columns the end of an utterance adds --, column u of the utterance
    at slot * period + u % period; old columns are overwritten once no output can read them, nothing is copied when an utterance
    grows, and the slot of any utterance that left goes to the next one.  The arenas hold nslots rings and grow, geometrically in
    slots, only when more utterances are open at once than ever before; arena_bytes does not depend on the utterances' lengths.  One
    call may feed an utterance at most max_feed = packing.enc_window_max_feed(W) frames.  The chunks are the bits of the unwindowed
    session's: the ring is an address, never an operand."""

    def __init__(self, eng, want_latents=False, window=None):
        if not eng.g.has_encoder:
            raise ValueError("encode_session: this engine has no encoder (a decoder-only geometry: c_in is None)")
        self.eng, self.want_latents = eng, bool(want_latents)
        self.clips: Dict[int, _EncClip] = {}
        self._next_handle, self._closed = 0, False
        self._ar, self._cap, self._top = None, 0, 0
        self._names = [name for name, _ in F.encoder_convs(eng)]
        self.window = None if window is None else int(window)
        self.max_feed, self._periods, self._nslots, self._free = None, None, 0, []
        if self.window is not None:
            if self.window % P.ENC_ROOM != 0 or self.window < P.enc_window_min():
                raise ValueError(f"encode_session: window {self.window}: a multiple of {P.ENC_ROOM} feature frames, at least "
                                 f"{P.enc_window_min()} (the {P.enc_window_min() - P.ENC_ROOM} the layers retain and {P.ENC_ROOM} of feed)")
            self.max_feed, self._periods = P.enc_window_max_feed(self.window), P.enc_ring_periods(self.window)

    @property
    def arena_bytes(self):
        """bytes of the session's arenas (windowed: 4 nslots sum_l C_l period_l, whatever the utterances' lengths)"""
        return sum(a.numel() * a.element_size() for a in self._ar or ())

    def _chans(self):
        return [self.eng.lay.shapes[name + ".weight"][1] for name in self._names]      # layer l's input channels

    def reserve_slots(self, n):
        """A windowed session: rings for n utterances open at once.  Grows on demand, geometrically; growing copies the rings."""
        if self._closed:
            raise RuntimeError("encode_session: the session is closed")
        if self.window is None:
            raise ValueError("encode_session.reserve_slots: a session without a window reserves frames (reserve_frames)")
        n = int(n)
        if n <= self._nslots:
            return
        if n * max(self._periods) >= 2 ** 31:
            raise ValueError(f"encode_session: {n} rings of {max(self._periods)} columns reach 2^31 columns")
        ar = [torch.empty(c, n * p, dtype=torch.float32, device=self.eng.device) for c, p in zip(self._chans(), self._periods)]
        for new, old in zip(ar, self._ar or ()):
            new[:, :old.shape[1]] = old
        self._free += list(range(n - 1, self._nslots - 1, -1))
        self._ar, self._nslots = ar, n

    # ---- room
    def reserve_frames(self, n):
        """Room for n feature frames of open utterances in all, in every layer's arena.  Grows on demand, geometrically; growing
        copies what the open utterances have so far."""
        if self._closed:
            raise RuntimeError("encode_session: the session is closed")
        if self.window is not None:
            raise ValueError("encode_session.reserve_frames: a windowed session reserves rings (reserve_slots)")
        n = _room(n)
        if n <= self._cap:
            return
        if n >= 2 ** 31:
            raise ValueError(f"encode_session: {n} feature frames of open utterances reach 2^31 columns")
        eng = self.eng
        ar = [torch.empty(c, n // d, dtype=torch.float32, device=eng.device) for c, d in zip(self._chans(), P.ENC_ARENA_DIV)]
        if self._cap:
            for new, old in zip(ar, self._ar):
                new[:, :old.shape[1]] = old
        self._ar, self._cap = ar, n

    def _place(self, c, need):
        """room for `need` feature frames of clip c: where it lies if it fits (or is the last and can stretch), else at the top of the
        arenas with what it has so far copied there"""
        if need <= c.cap:
            return
        cap = _room(need if c.max_frames is not None else max(2 * c.cap, need, 8))
        if c.max_frames is not None:
            cap = max(cap, _room(c.max_frames))
        if c.cap and c.base + c.cap == self._top:
            self._top = c.base
        base, top = self._top, self._top + cap
        if top > self._cap:
            self.reserve_frames(max(2 * self._cap, top))
        if base != c.base and c.frames:
            rows = P.enc_final_rows(c.frames, False)
            for a, d, n in zip(self._ar, P.ENC_ARENA_DIV, rows):
                if n:
                    a[:, base // d:base // d + n] = a[:, c.base // d:c.base // d + n].clone()
        c.base, c.cap, self._top = base, cap, top

    def _release(self, c):
        if self.window is not None:
            self._free.append(c.slot)
            return
        if c.base + c.cap == self._top:
            self._top = c.base
        if not self.clips:
            self._top = 0

    # ---- clips
    @property
    def live(self):
        """handles of the open utterances, in the order they joined"""
        return list(self.clips)

    def open(self, max_frames=None):
        """An utterance joins open.  max_frames: the most feature frames it will have -- its room is taken once, and a feed beyond
        it is refused.  Returns the handle."""
        if self._closed:
            raise RuntimeError("encode_session: the session is closed")
        if max_frames is not None and int(max_frames) < 1:
            raise ValueError(f"encode_session.open: max_frames {int(max_frames)} < 1")
        h = self._next_handle
        self._next_handle += 1
        c = _EncClip(max_frames=None if max_frames is None else int(max_frames))
        self.clips[h] = c
        if self.window is not None:     # a ring, whatever max_frames: the slot freed last, else the arenas grow by slots
            try:
                if not self._free:
                    self.reserve_slots(max(2 * self._nslots, 4))
            except Exception:
                del self.clips[h]
                raise
            c.slot = self._free.pop()
        elif c.max_frames is not None:
            try:
                self._place(c, c.max_frames)
            except Exception:
                del self.clips[h]
                raise
        return h

    def feed(self, handle, feats):
        """Appends the feature frames feats (c_in, f) to one open utterance: feed_list({handle: feats})[handle]."""
        return self.feed_list({handle: feats})[handle]

    def end(self, handle):
        """The utterance has all its frames: feed_list({}, ended=(handle,))[handle], its last latent frames."""
        return self.feed_list({}, ended=(handle,))[handle]

    def drop(self, handle):
        """Cancels an utterance: it leaves the session and its room is free.  ValueError: not an open utterance of this session."""
        if self._closed:
            raise RuntimeError("encode_session: the session is closed")
        if handle not in self.clips:
            raise ValueError(f"encode_session.drop: clip {handle} is not an open utterance of this session (unknown, ended or dropped)")
        self._release(self.clips.pop(handle))

    def feed_list(self, feeds, ended=()):
        """Feature frames for many open utterances: `feeds` maps handle -> feats (c_in, f), f >= 0, host or device; the handles in
        `ended` end behind their frames of this call.  Returns {handle: dict(quant (Cc, n), idx (n,) int64, latents (Cc, n) | None,
        final, done)} for every utterance that got frames or ended: the n latent frames this call made final (n = 0 allowed), `final`
        the utterance's latent frames so far, `done` true with its last chunk.  The chunks of an utterance, concatenated, are bit for
        bit encode_list([whole])[0].  The tensors are views of the call's packed (Cc, sum n) arrays.
        Refused before anything is launched (ValueError): a handle that is not an open utterance of this session, frames that are
        not (c_in, f), a feed beyond max_frames, the end of an utterance without frames, and -- a windowed session -- a feed of more
        than max_feed frames to one utterance."""
        if self._closed:
            raise RuntimeError("encode_session: the session is closed")
        eng, g, dev, who = self.eng, self.eng.g, self.eng.device, "encode_session.feed"
        feeds, ended = dict(feeds), list(dict.fromkeys(ended))
        new = {}
        for h, f in feeds.items():
            c = self.clips.get(h)
            if c is None:
                raise ValueError(f"{who}: clip {h} is not an open utterance of this session (unknown, ended or dropped)")
            shape = tuple(getattr(f, "shape", ()))
            if len(shape) != 2 or shape[0] != g.c_in:
                raise ValueError(f"{who}: clip {h}: frames of shape {shape}; a feed is (c_in, f) = ({g.c_in}, f)")
            n = int(shape[1])
            if c.max_frames is not None and c.frames + n > c.max_frames:
                raise ValueError(f"{who}: clip {h}: {c.frames + n} frames are beyond max_frames ({c.max_frames})")
            if self.window is not None and n > self.max_feed:
                raise ValueError(f"{who}: clip {h}: a feed of {n} frames; a window of {self.window} admits max_feed = {self.max_feed} "
                                 f"per call")
            new[h] = n
        for h in ended:
            c = self.clips.get(h)
            if c is None:
                raise ValueError(f"{who}: clip {h} is not an open utterance of this session (unknown, ended or dropped)")
            if c.frames + new.get(h, 0) < 1:
                raise ValueError(f"{who}: clip {h} ends without frames: every utterance has at least one")
        # everything is checked: room, then the plan over the clips of this call in the session's order of joining
        todo = [(h, c) for h, c in self.clips.items() if h in new or h in ended]
        if not todo:
            return {}
        ring = self.window is not None
        if ring:    # the planner refuses what a ring cannot hold, before anything is launched
            plan = P.enc_feed_plan_rings([(c.slot, c.frames, False, c.frames + new.get(h, 0), h in ended) for h, c in todo], self.window)
        else:
            for h, c in todo:
                if new.get(h, 0):
                    self._place(c, c.frames + new[h])
            plan = P.enc_feed_plan([(c.base, c.frames, False, c.frames + new.get(h, 0), h in ended) for h, c in todo])
        if eng.weights_dirty:
            eng.prepare_weights()
        fed = [(h, c) for h, c in todo if new.get(h, 0)]
        parts = [plan.table]
        if fed and ring:    # the ring columns of layer 0's arena that take the new frames, behind the records: ONE upload
            p0 = self._periods[0]
            parts.append(np.concatenate([c.slot * p0 + np.arange(c.frames, c.frames + new[h]) % p0 for h, c in fed]).astype(np.int32))
        elif fed:   # where the new frames go in layer 0's arena, behind the records: ONE upload
            parts.append(np.concatenate([np.arange(c.base + c.frames, c.base + c.frames + new[h]) for h, c in fed]).astype(np.int32))
        table = torch.from_numpy(np.concatenate(parts)).to(dev) if sum(p.size for p in parts) else None
        x = None
        if fed:
            x = F.pack_time(eng, [feeds[h] for h, _ in fed], g.c_in)
            self._ar[0].index_copy_(1, table[plan.table.size:].long(), x)
        lat = torch.empty(g.Cc, plan.total_new, dtype=torch.float32, device=dev)
        for ln in plan.launches:
            name = self._names[ln.layer]
            co, ci = eng.lay.shapes[name + ".weight"][:2]
            last = ln.layer == len(self._names) - 1
            xin, y = self._ar[ln.layer], (lat if last else self._ar[ln.layer + 1])
            res = int(not last and ln.stride == 1 and ci == co)
            entry = eng.lib.wae_enc_conv_fwd_rings if ring else eng.lib.wae_enc_conv_fwd_ranges
            L.check(entry(L.ptr(xin), L.ptr(eng.eff[eng.lay.off(name + ".weight"):]), L.ptr(eng.eff[eng.lay.off(name + ".bias"):]),
                          L.ptr(y), L.ptr(table[ln.rec_off:]), ln.nrecs, ln.ntiles, ln.et, xin.shape[1], y.shape[1], ci, co, ln.k,
                          ln.stride, ln.pad, int(not last), res, eng.stream()), "enc_conv_fwd_rings" if ring else "enc_conv_fwd_ranges")
        if plan.total_new:
            # the quantiser on this call's new latents as ONE clip: rows are per frame, so idx and quant are what vq_forward gives
            # the whole utterance (frontend._encode_group does the same with a list)
            quant, idx, _ = eng.vq_forward(lat.view(1, g.Cc, plan.total_new))
            quant = quant[0]
        else:
            quant = torch.empty_like(lat)
            idx = torch.empty((g.vq_n, 0) if g.vq_n > 1 else 0, dtype=torch.int64, device=dev)      # sliced kinds: a row per slice
        eng.hold("encode_session_feed", table, x)
        out = {}
        for (h, c), ready, o, n in zip(todo, plan.ready, plan.q_off, plan.q_cnt):
            s = slice(int(o), int(o + n))
            c.frames += new.get(h, 0)
            c.final = int(ready)
            done = h in ended
            out[h] = dict(quant=quant[:, s], idx=idx[..., s], latents=lat[:, s] if self.want_latents else None, final=c.final, done=done)
            if done:        # its last chunk is handed out: the room goes back
                del self.clips[h]
                self._release(c)
        return out

    def close(self):
        """Ends the session: every open utterance is dropped and the arenas are freed.  Closing twice is harmless; every other call
        on a closed session raises RuntimeError."""
        self.clips.clear()
        self._ar, self._cap, self._top, self._closed = None, 0, 0, True
        self._nslots, self._free = 0, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
