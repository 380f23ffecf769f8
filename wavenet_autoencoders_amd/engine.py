"""WaeEngine: host-side driver of the HIP hot path (encoder -> VQ -> upsample -> gated stack -> head -> loss).

PyTorch is used for device memory, streams and (elsewhere) torch.distributed only; every arithmetic step below
is a call into libwae_hip.so through the C ABI of include/wae.h.  There is no CPU fallback.

Reference call stack being replaced: VQVAE.forward (vqvae_model.py:66-72) -> Encoder.forward (:48-51),
VectorQuantize.forward (vector_quantization.py:21-49), WaveNet.forward (wavenet.py:164-216).
"""
from __future__ import annotations

import contextlib
import ctypes
import math

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import decode as D
from . import frontend as F
from . import packing as P
from . import train as TR
from .decode import DecodeSession  # noqa: F401  (re-exported)
from .encode import EncodeSession
from .options import two_chains
from .step_state import HeadDone, InFlight, Saved, Window


def _dt(dtype) -> int:
    if dtype in ("bf16", torch.bfloat16, L.WAE_BF16):
        return L.WAE_BF16
    if dtype in ("fp32", "f32", torch.float32, L.WAE_F32):
        return L.WAE_F32
    if dtype in ("fp16", "f16", "half", torch.float16, L.WAE_F16) and not isinstance(dtype, bool):
        return L.WAE_F16
    raise ValueError(f"unsupported compute dtype {dtype!r} (use 'fp32', 'bf16' or 'fp16')")


class WaeEngine:
    # the scalar cooperative opt-ins (ar_path), off on the class: an engine whose __init__ has not run routes as one that never opted in
    ar_scalar_coop = False
    ar_scalar_fast = False

    def __init__(self, geom: P.Geometry, dtype="bf16", device="cuda:0", dropout: float = 0.0, drop_seed: int = 0x5EED):
        """dtype: 'fp32' (exact, the parity mode), 'bf16' (default throughput mode) or 'fp16' (BASELINE config C5) storage of
        activations and packed weights; accumulation, biases, losses, gradients of parameters and the optimizer are fp32.
        dropout: probability of the F.dropout in front of every dilated convolution (modules.py:127-128); applied in
        train-mode forwards only, with a counter-based mask (seed, call number, layer) that backward regenerates."""
        if not 0.0 <= float(dropout) < 1.0:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")     # F.dropout's own check
        self.dropout, self.drop_seed, self.drop_calls = float(dropout), int(drop_seed), 0
        if not torch.cuda.is_available():
            raise L.WaeError("WaeEngine needs a ROCm GPU: the hot path has no CPU implementation")
        self.lib = L.lib()
        from .options import EngineOptions
        self.opt = EngineOptions.from_env().pinned()       # every launch-path switch, read once (options.py)
        # GLU_PAIR (barrier on every second weight chunk of the fused layer kernel; bit-identical): measured -2.3 % per launch without
        # the z save, nothing with it -- so inference launches take it by default
        self.glu_flags = L.GLU_PAIR if self.opt.glu_pair == "1" else 0
        self.glu_pair = self.opt.glu_pair
        self.g = geom
        self.dt = _dt(dtype)
        self.tdtype = {L.WAE_BF16: torch.bfloat16, L.WAE_F16: torch.float16, L.WAE_F32: torch.float32}[self.dt]
        # fp16 has 5 exponent bits: the backward pass runs on gradients multiplied by grad_scale (a power of two: exact), the
        # weight-gradient contractions carry 1/grad_scale in their alpha, so everything fp32 sees is unscaled.  Bounds: the
        # largest 16-bit gradient is |dy| <= grad_scale / count <= 4096 << 65504; at C5 (count 8e4) dy ~ 2e-4 stays normal.
        self.grad_scale = 4096.0 if self.dt == L.WAE_F16 else 1.0
        self.device = torch.device(device)
        self.lay = P.ParamLayout(geom)
        dev = self.device
        self.params = torch.zeros(self.lay.total, dtype=torch.float32, device=dev)
        self.eff = torch.zeros_like(self.params)
        self.wn_v = torch.from_numpy(self.lay.wn_v_off).to(dev)
        self.wn_g = torch.from_numpy(self.lay.wn_g_off).to(dev)
        self.wn_c = torch.from_numpy(self.lay.wn_cols).to(dev)
        g = geom
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.m_w1 = up(P.glu_w1_map(g, self.lay, self.dt))
        self.m_w2 = up(P.glu_w2_map(g, self.lay, self.dt))
        self.m_b2 = up(P.glu_bias2_map(g, self.lay))
        tab, fb = P.first_conv_maps(g, self.lay)
        self.m_tab, self.m_fb = up(tab), up(fb)
        # head: register-chained kernels up to 256 skip channels; wider heads as separate GEMM launches (csrc/gemm_tm.hip)
        self.wide_head = P.head_is_wide(g) or self.opt.head_wide
        # 16-bit dtypes: GEMM 0 of the head as its own wae_gemm_tm launch (decoder_forward); WAE_HEAD_SPLIT=0 keeps the one-kernel head
        self.split_head = not self.wide_head and self.dt in (L.WAE_BF16, L.WAE_F16) and g.Sp in (128, 256) and self.opt.head_split
        if self.wide_head:
            hm = P.head_wide_maps(g, self.lay, self.dt)
            self.m_hwide = {k: up(v) for k, v in hm.items()}
            self.w_hwide = {k: torch.zeros(v.numel(), dtype=self.tdtype, device=dev) for k, v in self.m_hwide.items()}
            self.m_hw = torch.zeros(0, dtype=torch.int32, device=dev)
        else:
            self.m_hw = up(P.head_w_map(g, self.lay, self.dt))
        self.m_hb = up(P.head_bias_map(g, self.lay))
        self.n_w1 = self.m_w1.numel()
        self.n_w2 = self.m_w2.numel()
        self.glu_elems = self.n_w1 + self.n_w2
        assert self.glu_elems == P.glu_packed_elems(g, self.dt)
        self.w_glu = torch.zeros(g.layers * self.glu_elems, dtype=self.tdtype, device=dev)
        self.b_glu = torch.zeros(g.layers * g.Rp, dtype=torch.float32, device=dev)
        self.first_tab = torch.zeros(self.m_tab.numel(), dtype=torch.float32, device=dev)
        self.first_bias = torch.zeros(g.Rp, dtype=torch.float32, device=dev)
        self.w_head = torch.zeros(self.m_hw.numel(), dtype=self.tdtype, device=dev)
        self.b_head = torch.zeros(2 * g.Sp + g.Op, dtype=torch.float32, device=dev)   # [sum skip bias | b1 | b3]
        self._ws: Dict[tuple, dict] = {}
        # which form of the cooperative decode kernel runs (ar_path(); arguments of the C ABI, not environment variables)
        self.ar_generic, self.ar_one_handover, self.ar_resident = False, False, (0, 0)
        self.ar_scalar_coop = False
        self.ar_scalar_fast = False
        self._param_gen, self._prep_gen, self._ar_gen = 1, 0, -1
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)      # sticky WAE_ERR_* bits set by the kernels (include/wae.h)
        # ---- step state: every attribute a later call creates or replaces starts here
        self.saved: Optional[Saved] = None      # the last train-mode forward's record; None: nothing to differentiate
        self.flight = InFlight()
        self.window: Optional[Window] = None    # an open accumulation window (accumulate .. apply_step / discard_step)
        self._vq_hist = None                    # the code counts of the last vq_forward (K + 1 int32; accumulate adds them to the window's)
        # the EMA quantisers' statistics (packing.vq_buffer_specs: vq.ema_cluster_size[s], vq.ema_w[s]): fp32 tensors of their own,
        # outside the parameter arena -- clipping, Adam and the EMA shadow never see them; empty for the other kinds
        self.vq_buffers: Dict[str, torch.Tensor] = {name: torch.zeros(shape, dtype=torch.float32, device=dev)
                                                    for name, shape in P.vq_buffer_specs(geom)}
        self._vq_recs: Dict[float, tuple] = {}  # vq_forward of the sliced / EMA kinds: the slices' records per beta (host array, c_loss_s)
        self._keep = {}                         # hold(): buffers passed by raw pointer, alive until their slot's next use
        # encode_list_stats: the list's quantiser totals over all its groups, (4,) fp32 on the device --
        # [vq_loss, perplexity, sum Tq, sum sqerr] (include/wae.h: wae_vq_stats_segments `out`); None before the first such call
        self.last_list_stats: Optional[torch.Tensor] = None
        self._side_streams, self._side_stream, self._ev_wn = {}, None, None
        self._pack_jobs = self._pack_bwd_jobs = None          # the packing launches' job tables (the pointers never change)
        self._bwd_ready, self._finish_plans = False, {}       # backward.py: _prepare_bwd, _finish_plan
        self._gid_src = self._gid_version = self._gid32 = None
        # hooks that bench.py, tools/ and tests set from outside
        self._layer_events = self._tn_events = self._tm_events = None
        self.chain_delay_us, self.bwd_pair4, self._ar_profile = None, False, None
        # the decode path's maps and packed weights (_prepare_ar, pack_ar_weights) and the last decode's operands
        self._ar_ready, self._ar_keep = False, None
        self.m_ar_layer = self.m_ar_b2 = self.m_ar_head = self.m_ar_hb = self.ar_ring_off = self.ar_dil = None
        self.ar_w = self.ar_b2 = self.ar_wh = self.ar_hb = self.ar_wm = None
        self.ar_w2_off = self.ar_layer_elems = self.ar_ring_total = 0
        # optimizer state (init_optimizer)
        self.exp_avg = self.exp_avg_sq = self.shadow = self.opt_scratch = self.grad_norm = None
        self.opt_step = 0
        # EngineOptions.deterministic: the partials of the fixed-order sums, each grown to its largest use and reused on the one stream
        # the mode runs on (det_buffer) -- "tn": wae_gemm_tn_tiles_det, "gproj": wae_gproj_bwd_det, "ups": wae_upsample_stage_bwd_det,
        # "ups_list": wae_upsample_stage_bwd_list_det (fp32), "norm": wae_clip_adam_ema_det (fp64)
        self._det_bufs: Dict[str, torch.Tensor] = {}

    def hold(self, slot: str, *tensors):
        self._keep[slot] = tensors

    def det_buffer(self, name: str, n: int, dtype=torch.float32) -> torch.Tensor:
        """The partials buffer `name` of the deterministic mode with at least n elements (never cleared: every user stores before it
        reads).  A larger request replaces it; the old one stays alive in hold() until the launches that use it have run."""
        buf = self._det_bufs.get(name)
        if buf is None or buf.numel() < n:
            if buf is not None:
                self.hold("det_" + name, buf)
            buf = self._det_bufs[name] = torch.empty(max(int(n), 1), dtype=dtype, device=self.device)
        return buf

    def _refuse_accum_vq(self):
        if self.g.has_encoder and self.g.vq != "plain":
            raise NotImplementedError(f"gradient accumulation with the {self.g.vq!r} quantiser: a window keeps one code histogram "
                                      "(wae_accum_stats); accumulation windows cover the plain quantiser")

    def _refuse_grad_sync(self, grad_sync):
        if grad_sync is not None and self.g.has_encoder and self.g.vq_ema:
            raise NotImplementedError(f"grad_sync with the {self.g.vq!r} quantiser: the codebooks move by each rank's EMA statistics, "
                                      "which would need an all-reduce of their own; data-parallel steps cover the plain and sliced kinds")
        if grad_sync is not None and self.opt.deterministic:
            raise NotImplementedError("EngineOptions.deterministic with grad_sync: the order in which the all-reduce adds the ranks' "
                                      "gradients is the collective library's; the mode covers one GPU")

    # Parameter generations.  Everything derived from the parameters -- the weight-normed arena and the fragment-packed buffers
    # (prepare_weights), the matrix-vector layout of the autoregressive kernels (pack_ar_weights) -- remembers the generation it was
    # made from.  `weights_dirty = True` (train_step, load_state_dict, the drop-in modules' parameter aliases, an EMA swap) starts a new
    # generation; a stale derivative is rebuilt where it is next needed.  (Round 3 kept two independent booleans: the decode weights
    # packed at the first in-training evaluation were reused by every later one.)
    @property
    def weights_dirty(self) -> bool:
        return self._prep_gen != self._param_gen

    @weights_dirty.setter
    def weights_dirty(self, dirty: bool):
        if dirty:
            self._refuse_in_window("a change of the parameters")
            self._param_gen += 1
        else:
            self._prep_gen = self._param_gen

    @property
    def _ar_packed(self) -> bool:
        return self._ar_gen == self._param_gen

    @_ar_packed.setter
    def _ar_packed(self, ok: bool):
        self._ar_gen = self._param_gen if ok else -1

    def _refuse_in_window(self, what: str):
        """Inside an accumulation window the weights, their packings and the gradient accumulators belong to the window: whatever would
        change them is refused here, before any launch."""
        if self.window is not None:
            raise RuntimeError(f"{what} while an accumulation window is open ({self.window.n} micro-batch(es) accumulated): close it "
                               "with apply_step() or drop it with discard_step() first")

    def check_errors(self):
        """Turn the kernels' sticky id-range flags into the IndexError the reference raises on the spot (nn.Embedding for a
        speaker id >= n_speakers, the one-hot encoder / CrossEntropyLoss for a class id outside [0, out_channels)).  Reads one
        device word (synchronises): the train script calls it where it already reads the logged scalars."""
        bits = int(self.err.item())
        if bits:
            self.err.zero_()
            if bits & L.ERR_NOT_ONEHOT:
                # wavenet.py:203 runs first_conv as a dense 1x1 on ANY (B, C, T) float tensor; the kernels gather rows of its weight by
                # class id -- identical for one-hot columns only.  Soft labels / probabilities are refused, not arg-maxed.
                raise NotImplementedError("decoder input (B, C, T) is not one-hot (every column exactly one 1.0 among zeros): dense inputs "
                                          "to first_conv are not implemented on the teacher-forced path; pass one-hot columns or (B, T) class ids")
            what = [n for b, n in ((L.ERR_CLASS_ID, f"input class id outside [0, {self.g.O})"),
                                   (L.ERR_SPEAKER_ID, f"speaker id outside [0, {self.g.n_speakers})"),
                                   (L.ERR_TARGET_ID, f"target class id outside [0, {self.g.O})")) if bits & b]
            raise IndexError("index out of range in self: " + "; ".join(what) + " (ids were clamped; results of that call are invalid)")

    def ids_from_onehot(self, x: torch.Tensor) -> torch.Tensor:
        """(B, C, T) one-hot floats (any strides: a transposed (B, T, C) view needs no copy) -> (B, T) int32 class ids.  A column that is
        not one-hot sets WAE_ERR_NOT_ONEHOT in the sticky error word; check_errors() raises (wae_onehot_to_ids, include/wae.h)."""
        x = x.to(self.device, torch.float32)
        B, C, T = x.shape
        ids = torch.empty(B, T, dtype=torch.int32, device=self.device)
        L.check(self.lib.wae_onehot_to_ids(L.ptr(x), B, C, T, x.stride(0), x.stride(1), x.stride(2), L.ptr(ids), L.ptr(self.err),
                                           L.ERR_NOT_ONEHOT, self.stream()), "onehot_to_ids")
        self.hold("onehot", x)
        return ids

    # ------------------------------------------------------------------ parameters
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ two chains of layer launches (include/wae.h: wae_stream_delay)
    def chain_plan(self, B: int, T: int, backward: bool = False):
        """None (one chain of full-batch launches), or (b_cut, delay_us): clips [0, b_cut) stay on the current stream, clips
        [b_cut, B) run as a second chain of the same launches on the engine's side stream, started delay_us late.
        Every workgroup of a layer launch stores its outputs at the same time -- at BASELINE C2 ~20 us of a 55-us forward launch and
        ~30 of a 77-us backward launch in which nothing computes -- and a launch with more workgroups than CUs (C5: 320) ends with a
        quarter-full second round.  One launch cannot be de-phased against itself (it ends with its late half: profiles/
        r06_pair8_experiments.txt); two chains of launches can, and two 160-workgroup launches side by side fill C5's machine.
        Measured on whole train steps (profiles/r06_chains.txt): C5 37.5 -> 33.4 ms (both directions), C2 5.26 -> 5.19 ms (the backward
        sweep only: `auto` leaves a forward stack of one round of workgroups on one chain); hps/vqwae.json's 160-workgroup launches gain
        nothing, so `auto` leaves them alone.  Same kernels, same arithmetic per clip: results are bit for bit those of one chain
        (tests/test_gpu_backward.py::test_two_chains_are_bitwise_one_chain)."""
        if not two_chains(self.opt.chains, self.dt in (L.WAE_BF16, L.WAE_F16), B, T, backward):      # (options.py: the rule and its numbers)
            return None
        g = self.g
        delay = self.chain_delay_us        # (tools)
        if delay is None:
            # The forward chains start together and stay in step (started half a launch apart they ran 64 us per layer at C2 until they
            # fell into step, 53 in step, 55.5 as one chain).  The backward sweep's second chain starts half a launch late: 35 us at
            # C2, scaled by the MFMA work of a workgroup.  Its launches then run 70-72 us per layer against 77 in step -- for about 14
            # layers, until the trailing chain (~3 us per launch faster) has caught up; holding it back with events on a third stream
            # costs more than it keeps (profiles/r06_chains.txt).
            work = (g.k * g.Rp + g.Ccp) * 2 * g.Hp + g.Hp * g.Rp
            delay = 35.0 * work / 368640.0 if backward else 0.0
        return (B + 1) // 2, float(delay)

    def side_stream(self, k: int = 0):
        if k not in self._side_streams:
            self._side_streams[k] = torch.cuda.Stream(self.device)
        return self._side_streams[k]

    @contextlib.contextmanager
    def branch(self, k: int, after=None):
        """Independent side work of a step: the body's launches go to side stream k, which first waits for `after` (an event of the
        main stream; default: everything enqueued on the current stream so far).  Yields a one-element list that holds the branch's
        completion event afterwards: `self.join(box[0])` where the main stream needs the results.  (The step's small launches --
        weight packing, the upsampling network, the front end's backward, scatters -- fill a fraction of the machine each and run
        one after the other on one stream: DESIGN 3.4.)"""
        side, cur = self.side_stream(k), torch.cuda.current_stream(self.device)
        if after is None:
            after = torch.cuda.Event()
            after.record(cur)
        side.wait_event(after)
        box = [None]
        with torch.cuda.stream(side):
            yield box
        box[0] = torch.cuda.Event()
        box[0].record(side)

    def join(self, ev):
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)

    def chain_fork(self, delay_us: float):
        """The side stream waits for everything enqueued on the current stream so far, then for delay_us; returns it."""
        self._side_stream = self.side_stream(0)
        side, cur = self._side_stream, torch.cuda.current_stream(self.device)
        ev = torch.cuda.Event()
        ev.record(cur)
        side.wait_event(ev)
        L.check(self.lib.wae_stream_delay(delay_us, ctypes.c_void_p(side.cuda_stream)), "stream_delay")
        return side

    def chain_join(self):
        """The current stream waits for the side stream's chain."""
        ev = torch.cuda.Event()
        ev.record(self._side_stream)
        torch.cuda.current_stream(self.device).wait_event(ev)

    def view(self, name: str) -> torch.Tensor:
        off = self.lay.off(name)
        return self.params[off:off + self.lay.numel(name)].view(self.lay.shapes[name])

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        self._refuse_in_window("load_state_dict")
        keys = list(self.lay.offsets) + list(self.vq_buffers)
        missing = [k for k in keys if k not in sd]
        extra = [k for k in sd if k not in self.lay.offsets and k not in self.vq_buffers]
        if strict and (missing or extra):
            raise KeyError(f"state_dict mismatch: missing {missing[:5]}, unexpected {extra[:5]}")
        for k, buf in self.vq_buffers.items():
            if k in sd:
                if tuple(sd[k].shape) != tuple(buf.shape):
                    raise ValueError(f"{k}: expected {tuple(buf.shape)}, got {tuple(sd[k].shape)}")
        host = torch.zeros(self.lay.total, dtype=torch.float32)
        for k in self.lay.offsets:
            if k in sd:
                t = sd[k].detach().to(torch.float32).cpu().reshape(-1)
                if t.numel() != self.lay.numel(k):
                    raise ValueError(f"{k}: expected {self.lay.shapes[k]}, got {tuple(sd[k].shape)}")
                host[self.lay.off(k):self.lay.off(k) + t.numel()] = t
        self.params.copy_(host.to(self.device))
        for k, buf in self.vq_buffers.items():
            if k in sd:
                buf.copy_(sd[k].detach().to(torch.float32))
        self.weights_dirty = True

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {k: self.view(k).detach().clone() for k in self.lay.offsets}
        sd.update({k: v.detach().clone() for k, v in self.vq_buffers.items()})
        return sd

    def prepare_weights(self, side: bool = False):
        """K14 weight norm + fragment packing; call after every parameter update.  side (train_step): the packing runs on a side stream
        behind weight norm -- what needs the effective weights only (an encoder, the upsampling network, the hoisted global
        conditioning) goes ahead on the main stream beside it; decoder_forward joins in front of the first launch that reads a packed
        array."""
        lib, st, g, lay = self.lib, self.stream(), self.g, self.lay
        L.check(lib.wae_weight_norm_fwd(L.ptr(self.params), L.ptr(self.eff), lay.total, L.ptr(self.wn_v), L.ptr(self.wn_g),
                                        L.ptr(self.wn_c), len(lay.wn_cols), st), "weight_norm_fwd")
        self._ev_wn = None
        if side and self.opt.side and self.device.type == "cuda":      # the effective weights exist: what only needs them may start
            self._ev_wn = torch.cuda.Event()
            self._ev_wn.record(torch.cuda.current_stream(self.device))
        with (self.branch(1, after=self._ev_wn) if self._ev_wn is not None else contextlib.nullcontext([None])) as self.flight.pack_done:
            self._pack_weights()
        self.weights_dirty = False

    def _pack_weights(self):
        lib, st, g, lay = self.lib, self.stream(), self.g, self.lay
        jobs = self._pack_jobs
        if jobs is None:       # the pointers never change: one host array, one launch for every family
            es = self.w_glu.element_size()
            eff = self.eff.data_ptr()
            J = lambda mp, dst, n, nb, ss, ds, dt: L.GatherJob(eff, mp.data_ptr(), dst, n, ss, ds, nb, dt)
            lst = [J(self.m_w1, self.w_glu.data_ptr(), self.n_w1, g.layers, lay.layer_stride, self.glu_elems, self.dt),
                   J(self.m_w2, self.w_glu.data_ptr() + self.n_w1 * es, self.n_w2, g.layers, lay.layer_stride, self.glu_elems, self.dt),
                   J(self.m_b2, self.b_glu.data_ptr(), g.Rp, g.layers, lay.layer_stride, g.Rp, L.WAE_F32),
                   J(self.m_tab, self.first_tab.data_ptr(), self.m_tab.numel(), 1, 0, 0, L.WAE_F32),
                   J(self.m_fb, self.first_bias.data_ptr(), g.Rp, 1, 0, 0, L.WAE_F32)]
            if self.wide_head:
                lst += [J(self.m_hwide[k], self.w_hwide[k].data_ptr(), self.m_hwide[k].numel(), 1, 0, 0, self.dt)
                        for k in ("skip", "w1", "w3")]
            else:
                lst.append(J(self.m_hw, self.w_head.data_ptr(), self.m_hw.numel(), 1, 0, 0, self.dt))
            lst.append(J(self.m_hb, self.b_head.data_ptr() + g.Sp * 4, g.Sp + g.Op, 1, 0, 0, L.WAE_F32))
            jobs = self._pack_jobs = (L.GatherJob * len(lst))(*lst)
        L.check(lib.wae_pack_gather_multi(jobs, len(jobs), st), "pack weights")
        L.check(lib.wae_sum_rows(L.ptr(self.eff), lay.off("wavenet.conv_layers.0.conv1x1_skip.bias"), lay.layer_stride,
                                 g.layers, g.S, g.Sp, L.ptr(self.b_head), st), "sum skip bias")

    # ------------------------------------------------------------------ workspaces
    def workspace(self, B: int, T: int, train: bool = False) -> dict:
        key = (B, T, train)
        ws = self._ws.get(key)
        if ws is None:
            g, dev, td = self.g, self.device, self.tdtype
            ws = dict(
                x=[torch.empty(B, T, g.Rp, dtype=td, device=dev) for _ in range((g.layers + 1) if train else 2)],
                u=torch.zeros(B, T, g.Ku, dtype=td, device=dev),      # all layers' gated activations (pad columns stay 0)
                zb=torch.empty(B, g.layers, 2 * g.Hp, dtype=torch.float32, device=dev),
                c_up=torch.zeros(B, T, g.Ccp, dtype=td, device=dev) if g.Ccp else None,
                nll=torch.zeros(B, T, dtype=torch.float32, device=dev),
                loss=torch.zeros(2, dtype=torch.float32, device=dev),
            )
            if train:
                ws["z"] = [torch.empty(B, T, 2 * g.Hp, dtype=td, device=dev) for _ in range(g.layers)]
                if self.dropout > 0:       # dropout(x_l): operand of layer l's convolution and of its weight gradient
                    ws["xd"] = [torch.empty(B, T, g.Rp, dtype=td, device=dev) for _ in range(g.layers)]
                ws["lse"] = torch.zeros(B, T, dtype=torch.float32, device=dev)
            if train or self.wide_head or self.split_head:   # the wide / split head pass h0 (and h1) through HBM in inference too
                ws["h0"] = torch.empty(B, T, g.Sp, dtype=td, device=dev)
            if train or self.wide_head:
                ws["h1"] = torch.empty(B, T, g.Sp, dtype=td, device=dev)
            self._ws[key] = ws
        return ws

    # ------------------------------------------------------------------ front end
    def encoder_forward(self, c: torch.Tensor, save: Optional[Saved] = None) -> torch.Tensor:
        """a1: c (B, c_in, F) fp32 -> latents (B, Cc, F')  (vqvae_model.py:48-51).  save: the train-mode forward's record, which
        takes the blocks' inputs; without it nothing outlives the call."""
        return F.encoder_forward(self, c, save)

    def vq_forward(self, lat: torch.Tensor, beta: float = 0.25, update: bool = False):
        """a2: -> (quant (B,Cc,Tq), idx int64 (B*Tq), stats[2] = (vq_loss, perplexity)).  The sliced kinds (Geometry.vq): idx
        (n, B*Tq), a row per slice; vq_loss and perplexity the sums over the slices (vector_quantization.py:113-127).
        update (EMA kinds): the training branch -- the codebooks move between the search and the gather."""
        return F.vq_forward(self, lat, beta, update)

    def vq_slice_records(self, beta: float):
        """The slices of the geometry's quantiser for wae_vq_search_slices: (host array of wae_vq_slice_rec -- codebook pointers into
        the effective arena, c_loss_s = c_loss * D_s / Dtot --, [(codebook name, d0, D, K, c_loss_s)], scratch entries).  Made once per
        beta: the arena never moves."""
        return F.vq_slice_records(self, beta)

    def encode_list(self, feats, want_latents: bool = False, want_idx: bool = True, max_frames: Optional[int] = None):
        """Encoder + quantiser for a LIST of utterances of unequal lengths (include/wae.h: wae_enc_conv_fwd_list): one launch per
        encoder block, one for lin and one quantiser call for the whole list, where encoder_forward takes equal lengths only, a loop
        over it is thirteen launches and two copies per utterance, and zero-padding to a common length gives other latents at the
        clip ends (the pad frames stop being zero behind the first block).

        feats: a sequence of (c_in, F_i) float tensors or arrays, on the host or on the device, F_i >= 1, lengths free.  They are
        packed along time in the caller's order into ONE (c_in, sum F_i) input (one upload when they come from the host); two
        ping-pong (encoder_hid, sum F_i) buffers carry the blocks, since nothing is saved for a backward; every layer's tables
        (packing.encode_list_plan) go up as one int32 array.
        max_frames: the most frames (sum F_i) of one group, by default packing.ENC_LIST_MAX_FRAMES = 32768, which keeps the two
        activation buffers at 192 MiB for encoder_hid = 768; a longer list runs as consecutive groups (an utterance longer than
        max_frames is a group of its own).  The bytes of every item are the same for every grouping and every order.
        Returns, in the caller's order, a list of dict(quant (Cc, Tq_i) fp32, idx (Tq_i,) int64 | None (want_idx=False),
        latents (Cc, Tq_i) fp32 | None (want_latents=False)); every item is, bit for bit, encoder_forward + vq_forward of that
        utterance alone.  The tensors of an item are views of its group's packed (Cc, sum Tq_i) arrays (not contiguous).
        The quantiser's statistics are not computed here: encode_list_stats is this call with them.
        ValueError, before any launch: an empty list, an item that is not (c_in, F_i) with F_i >= 1, an engine without an encoder."""
        return F.encode_list(self, feats, want_latents, want_idx, max_frames, None)

    def encode_list_stats(self, feats, beta: float = 0.25, want_latents: bool = False, want_idx: bool = True,
                          max_frames: Optional[int] = None):
        """encode_list with the quantiser's numbers besides (include/wae.h: wae_vq_stats_segments, one call per group behind the
        quantiser's, c_loss = beta + 1): the same launches in front of it, the same quant, idx and latents.  Every item's dict gains
        sqerr (sum of (quant - latents)^2), vq_loss (what vq_forward reports for the utterance alone, here from a fixed-order fp64 sum:
        reproducible to the bit), perp (bit for bit vq_forward's perplexity of the utterance alone) -- 0-d views -- and hist, a (K,)
        int32 view: how often the utterance used every code.  The list's totals over all groups go to self.last_list_stats, a (4,)
        device tensor [vq_loss, perplexity, sum Tq, sum sqerr] of the list as ONE batch: vq_loss = (beta + 1) sum sqerr / (Cc sum Tq),
        the perplexity that of the counts added per code -- what vq_forward reports on the packed latents.  All of it is the same
        for every grouping, and per item for every order.  ValueError as encode_list.
        Sliced / EMA quantisers (Geometry.vq): idx is (n, Tq_i), a row per slice; vq_loss = c_loss sum_s sqerr_s / (Tq_i Cc) with the
        kind's c_loss (packing.vq_coeffs), perp = sum_s perp_s, sqerr = sum_s sqerr_s, hist (n, max K_s) int32, zero beyond K_s; the
        totals follow the same rule (packing.vq_list_totals per slice, added over the slices)."""
        return F.encode_list(self, feats, want_latents, want_idx, max_frames, float(beta))

    def encode_session(self, want_latents: bool = False, window: Optional[int] = None) -> EncodeSession:
        """An encode session: encode_list for utterances whose feature frames still arrive (include/wae.h: wae_enc_conv_fwd_ranges).
        h = sess.open(max_frames=None) joins an open utterance; sess.feed_list({h: feats (c_in, f), ...}, ended=()) appends frames
        and returns, per utterance, the latent frames no later frame can change -- dict(quant, idx, latents | None, final, done); with
        F frames that is max(0, (F - 13) // 4) of them while the utterance is open, all (F + 3) // 4 once it has ended (sess.end(h), or
        its handle in `ended`).  One call is one upload of the new frames, one table upload, at most eleven range launches and one
        quantiser call, whatever the number of utterances.  An utterance's chunks, concatenated, are bit for bit
        encode_list([whole])[0]; the `quant` chunks are what DecodeSession.feed_list takes.  sess.drop(h) cancels, sess.close() (or
        leaving the `with` block) frees everything.  ValueError: an engine without an encoder.
        window=W (feature frames): a session in constant memory -- every open utterance lives in a ring of about W / ENC_ARENA_DIV[l]
        columns per layer (include/wae.h: wae_enc_conv_fwd_rings), nothing is copied when it grows, one call feeds
        an utterance at most sess.max_feed frames, and the chunks are the same bits.  ValueError: a window below the minimum."""
        return EncodeSession(self, want_latents=want_latents, window=window)

    def upsample_forward(self, c: torch.Tensor, out: torch.Tensor, save: Optional[Saved] = None):
        """a3: c (B,Cc,Tc) fp32 -> out (B, (Tc - 2 cin_pad) * prod(scales), Ccp) time-major compute dtype.  ConvInUpsampleNetwork
        (upsample.py:69-85): conv_in eats cin_pad frames at either end, then the stages; plain UpsampleNetwork (Geometry.conv_in False,
        upsample.py:29-66): the stages on all Tc frames, then cin_pad * prod(scales) samples trimmed at either end.
        save: the train-mode forward's record, which takes the stages' inputs; without it (eval, a decode) nothing outlives the call."""
        return F.upsample_forward(self, c, out, save)

    def upsample_list(self, cs, out: Optional[torch.Tensor] = None, offsets=None, c_is_upsampled: bool = False,
                      max_samples: Optional[int] = None):
        """The conditioning rows of a LIST of utterances of unequal lengths (include/wae.h: wae_upsample_stage_fwd_list,
        wae_to_btc_list): one launch for conv_in, one per stage and, where the last stage does not write the operand itself (an
        upsample_activation, the plain UpsampleNetwork's trim), one wae_to_btc_list -- per list, where a loop of upsample_forward is
        that many launches and allocations per item.  The launches, the allocations and the one table upload do not grow with the list.

        cs: a sequence of (Cc, Tc_i) or (1, Cc, Tc_i) arrays -- host arrays, CPU tensors or device tensors, mixed: the latent frames, or
        the (Cc, T_i) per-sample features when c_is_upsampled or the geometry has no upsampling network.  Host items are packed on the
        host and go up in one copy; device items are concatenated on the device.
        out: the packed time-major operand (rows, Ccp) in the model's dtype that the list and span decode kernels read, or None: a new
        one of sum T_i rows.  offsets: the first row of every item in `out` (free: the caller's order), or None: running sums.
        max_samples: the most output samples (sum T_i) of one group, by default packing.UPS_LIST_MAX_SAMPLES = 2^22, which keeps the
        largest fp32 intermediate at 205 MiB for Cc 64 and a last scale of 5; a longer list runs as consecutive groups (an item longer
        than max_samples is a group of its own).
        Returns (c_up, offsets).  Every item's rows [offsets_i, offsets_i + T_i), pad channels included, are bit for bit what
        upsample_forward (or wae_to_btc) writes for that item alone, for every order and every grouping.  Geometries the list kernels do
        not cover (conv_in with cin_pad > 2, a time-major last stage with Ccp not dividing 256 or 3 s > 256) run that loop into the same
        rows.  ValueError, before any launch and with the item's index: an empty list, an item that is not (Cc, Tc), an item with no
        output frame, rows outside `out`."""
        return F.upsample_list(self, cs, out, offsets, c_is_upsampled, max_samples)

    def _pack_cond_list(self, cs):
        """(Cc, sum Tc_i) fp32 on the device, the items side by side in order: the host items in one upload, the rest by one cat"""
        return F.pack_time(self, cs, self.g.Cc)

    def layer_drop_seed(self, call: int, layer: int) -> int:
        """64-bit seed of layer `layer`'s dropout mask in the call-th train-mode forward (csrc/misc.hip: dropout_keep)"""
        # distinct (drop_seed, call, layer) triples give distinct seeds; the kernel finalises the seed (dropout_key) before it meets
        # the element index, so neighbouring seeds give unrelated masks.  drop_seed should differ per data-parallel rank and
        # drop_calls follow the global step across a resume (vqwae_train.py does both).
        return ((self.drop_seed * 0x100000001B3 + call) * 1024 + layer) & 0xFFFFFFFFFFFFFFFF

    # ------------------------------------------------------------------ decoder
    def decoder_forward(self, x: torch.Tensor, c: Optional[torch.Tensor], gid: Optional[torch.Tensor],
                        targets: Optional[torch.Tensor] = None, lengths: Optional[torch.Tensor] = None,
                        want_logits: bool = True, train: bool = False, c_is_upsampled: bool = False,
                        gvec: Optional[torch.Tensor] = None, layer_events: Optional[list] = None, dropout_on: bool = True,
                        saved: Optional[Saved] = None, c_ready: bool = False):
        """WaveNet.forward (wavenet.py:164-216) on class ids.

        x: (B,T) int32 class ids (mulaw-quantize) or (B,T) fp32 scalars (scalar_input).
        c: (B,Cc,Tc) fp32 local conditioning (upsampled here) or, if c_is_upsampled, (B,Cc,T).
        gid: (B,) int32 speaker ids.  targets: (B,T) int32 -> fused shifted CE.
        train: the activations stay in the (B, T, True) workspace and this forward's record becomes self.saved once it is complete
        (saved: the record forward() began with the encoder's side; default: a new one).
        c_ready: the (B, T, Ccp) conditioning operand of the (B, T, train) workspace already holds this call's rows (train_step_list:
        the list front end wrote them, pad rows zero); c is not read.
        Returns dict(logits (B,O,T) | None, nll (B,T) | None, loss | None).
        """
        if train and self.flight.accum is None:
            self._refuse_in_window("a train-mode decoder_forward outside accumulate()")
        if self.weights_dirty:
            self.prepare_weights()
        g, lib, st = self.g, self.lib, self.stream()
        B, T = x.shape
        ws = self.workspace(B, T, train)
        sv = None
        if train:       # the launches below overwrite what the previous train-mode forward of this (B, T) saved
            self.saved, sv = None, (saved if saved is not None else Saved(B, T))
        # global conditioning folded with the conv bias (first: in a train step the launches below run beside the weight packing)
        if gid is not None:
            gid = gid.to(torch.int32).contiguous()
        self._ar_speaker_rows(B, gid, gvec, ws["zb"])
        # local conditioning
        if g.Ccp and not c_ready:
            if c is None:
                raise ValueError("model has local conditioning but c is None")
            if c_is_upsampled or not g.upsample_scales:
                if c.shape[-1] != T:
                    raise Exception(f"c {tuple(c.shape)} x T={T}")           # wavenet.py:198-200
                L.check(lib.wae_to_btc(L.ptr(c.contiguous().float()), L.ptr(ws["c_up"]), B, g.Cc, T, g.Ccp, self.dt, self.stream()), "to_btc")
            else:
                Tup = (c.shape[-1] - 2 * g.cin_pad) * int(np.prod(g.upsample_scales))
                if Tup != T:
                    raise Exception(f"c {tuple(c.shape)} upsamples to {Tup} != T={T}")  # wavenet.py:198-200
                self.upsample_forward(c.float(), ws["c_up"], sv)
        # (train_step: the packing of the weights runs on a side stream beside the launches above -- prepare_weights(side=True))
        self.join(self.flight.take_pack_done())
        # first conv
        if g.scalar_input:
            xs = x.contiguous().float()
            L.check(lib.wae_first_conv_fwd(None, L.ptr(xs), L.ptr(self.first_tab), L.ptr(self.first_bias), L.ptr(ws["x"][0]),
                                           B * T, g.Rp, 1, self.dt, None, st), "first_conv")
        else:
            xi = x.to(torch.int32).contiguous()
            L.check(lib.wae_first_conv_fwd(L.ptr(xi), None, L.ptr(self.first_tab), L.ptr(self.first_bias), L.ptr(ws["x"][0]),
                                           B * T, g.Rp, g.O, self.dt, L.ptr(self.err), st), "first_conv")
        # gated residual stack
        es = self.w_glu.element_size()
        # dropout (modules.py:127-128) only in a train-mode forward of a model in training mode; eval is the identity
        drop = self.dropout if (train and dropout_on) else 0.0
        if drop > 0:
            self.drop_calls += 1
            sv.drop_seeds = [self.layer_drop_seed(self.drop_calls, i) for i in range(g.layers)]
        if layer_events is not None:   # HIP events on the launch stream around the whole gated stack (bench.py)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream(self.device))
        # two half-batch chains of the same launches (chain_plan): not with dropout (its mask generator counts elements of the full batch)
        plan = self.chain_plan(B, T) if (drop == 0 and not (train and "xd" in ws)) else None

        parts = [(0, B, st)]
        if plan is not None:
            side = self.chain_fork(plan[1])
            parts = [(0, plan[0], st), (plan[0], B - plan[0], ctypes.c_void_p(side.cuda_stream))]
        for i, dil in enumerate(g.dilations):
            last = i == g.layers - 1
            flags = (L.GLU_SAVE_Z if train else 0) | (L.GLU_NO_OUT if last else 0) | self.glu_flags
            if not train and self.glu_pair == "inference":
                flags |= L.GLU_PAIR
            xin = ws["x"][i if train else i % 2]
            xout = ws["x"][(i + 1) if train else (i + 1) % 2]
            xconv = xin
            if drop > 0:
                xconv = ws["xd"][i]
                L.check(lib.wae_dropout_fwd(L.ptr(xin), L.ptr(xconv), B * T * g.Rp, sv.drop_seeds[i], drop, self.dt, st), "dropout")
            elif train and "xd" in ws:
                # an engine built with dropout > 0 running a train-mode forward of a model in eval mode: the weight-gradient
                # tables of this (B, T) point at xd, so it must hold the (undropped) operand
                L.check(lib.wae_dropout_fwd(L.ptr(xin), L.ptr(ws["xd"][i]), B * T * g.Rp, 0, 0.0, self.dt, st), "dropout (identity)")
            for b0, nb, stc in parts:      # every array is clip-major: a chain is the same call on its clips
                dd = L.GluDesc(self.dt, nb, T, g.Rp, g.Ccp, g.Hp, g.k, dil, flags)
                rx = b0 * T * g.Rp * es
                L.check(lib.wae_glu_layer_fwd_drop(ctypes.byref(dd), ctypes.c_void_p(xin.data_ptr() + rx), ctypes.c_void_p(xconv.data_ptr() + rx),
                                                   None if last else ctypes.c_void_p(xout.data_ptr() + rx),
                                                   ctypes.c_void_p(ws["c_up"].data_ptr() + b0 * T * g.Ccp * es) if ws["c_up"] is not None else None,
                                                   ctypes.c_void_p(ws["u"].data_ptr() + (b0 * T * g.Ku + i * g.Hp) * es), g.Ku,
                                                   ctypes.c_void_p(ws["zb"].data_ptr() + (b0 * g.layers + i) * 2 * g.Hp * 4),
                                                   g.layers * 2 * g.Hp,
                                                   ctypes.c_void_p(ws["z"][i].data_ptr() + b0 * T * 2 * g.Hp * es) if train else None,
                                                   ctypes.c_void_p(self.w_glu.data_ptr() + i * self.glu_elems * es),
                                                   ctypes.c_void_p(self.b_glu.data_ptr() + i * g.Rp * 4), stc), f"glu layer {i}")
        if plan is not None:
            self.chain_join()
        if layer_events is not None:
            e1.record(torch.cuda.current_stream(self.device))
            layer_events.append((e0, e1))
        # head (+ fused CE)
        logits = torch.empty(B, g.O, T, dtype=torch.float32, device=self.device) if want_logits else None
        tg = targets.to(torch.int32).contiguous() if targets is not None else None
        if tg is not None and tg.data_ptr() != (xi.data_ptr() if not g.scalar_input else 0):   # targets = inputs: already checked
            L.check(lib.wae_check_ids(L.ptr(tg), B * T, 0, g.O, L.ptr(self.err), L.ERR_TARGET_ID, st), "check targets")
        ln = lengths.to(self.device, torch.int32).contiguous() if (tg is not None and lengths is not None) else None
        # (a train step announced the factor of its backward: the head's launch may run the head's backward and the loss mean with it)
        factor = self.flight.take_head_factor()
        fused = self._head_fwd(ws, B, T, logits, tg, train, ln, factor if train else None)
        if fused:
            sv.head_done = HeadDone(factor, targets, lengths)
        out = dict(logits=logits, nll=None, loss=None)
        if tg is not None:
            if not fused:
                TR.masked_mean(self, ws["nll"], ln, ws["loss"])
            out["nll"] = ws["nll"]
            out["loss"] = ws["loss"][0]
        if train:
            self.saved = sv
        return out

    def _head_fwd(self, ws, B, T, logits, tg, train, ln=None, factor=None) -> bool:
        """wavenet.py:204-214 (+ the shifted CE against tg) on the (B, T) rows of ws["u"]: the head this engine runs -- wide, split or
        the one kernel; ws holds u and, where that head passes them through memory, h0 / h1, nll and lse.
        factor (with ln, the int32 device lengths): the factor on d loss / d logits that the caller's backward will use.  A split 16-bit
        head with Sp == Op in train mode then runs ONE launch from h0 (csrc/head_train.hip; EngineOptions.head_fused) that also writes
        ws["loss"] -- the masked mean -- and dy, dh1, dskip of the (B, T) backward workspace: -> True, and the caller records it."""
        g, lib, st = self.g, self.lib, self.stream()
        hd = L.HeadDesc(self.dt, B, T, g.Ku, g.Sp, g.Op, g.O, math.sqrt(1.0 / g.layers))
        if self.wide_head:
            self._head_fwd_wide(ws, B, T, logits, tg, train)
        elif self.split_head:
            # the skip contraction (K = Ku: 72 chunks at C2, its operand 590 MB of u) as a wae_gemm_tm launch -- 197 us against the ~210 us
            # the same loop takes inside the one-workgroup-per-CU head kernel -- then the rest from h0 (45 us)
            from . import backward as BW
            es = self.w_head.element_size()
            BW._tm(self, B, T, g.Sp, 3, math.sqrt(1.0 / g.layers), [(ws["u"].data_ptr(), g.Ku, g.Ku, 0)], self.w_head.data_ptr(),
                   ws["h0"].data_ptr(), g.Sp, self.b_head.data_ptr(), 0)
            ck = 64 if es == 2 else 32
            tail = self.w_head.data_ptr() + (g.Ku // ck) * (g.Sp // 32) * 4096
            if factor is not None and train and tg is not None and logits is None and BW.head_fused_ok(self) and self._bwd_weights_coming():
                bws = BW.bwd_workspace(self, B, T)
                red = ws.get("head_red")
                if red is None:
                    red = ws["head_red"] = torch.zeros(int(lib.wae_head_train_ws_bytes(ctypes.byref(hd))), dtype=torch.uint8, device=self.device)
                L.check(lib.wae_head_train_from_h0(ctypes.byref(hd), L.ptr(ws["h0"]), ctypes.c_void_p(tail), L.ptr(self.w_hb), L.ptr(self.b_head),
                                                   L.ptr(tg), L.ptr(ln), float(factor), L.ptr(ws["nll"]), L.ptr(ws["lse"]), L.ptr(ws["h1"]),
                                                   L.ptr(bws["dy"]), L.ptr(bws["dh1"]), L.ptr(bws["dskip"]), L.ptr(red), L.ptr(ws["loss"]), st),
                        "head (train, from h0)")
                return True
            L.check(lib.wae_head_fwd_from_h0(ctypes.byref(hd), L.ptr(ws["h0"]), ctypes.c_void_p(tail), L.ptr(self.b_head), L.ptr(logits),
                                             L.ptr(tg), L.ptr(ws["nll"]) if tg is not None else None,
                                             L.ptr(ws["lse"]) if (train and tg is not None) else None,
                                             L.ptr(ws["h1"]) if train else None, st), "head (from h0)")
        else:
            L.check(lib.wae_head_fwd(ctypes.byref(hd), L.ptr(ws["u"]), L.ptr(self.w_head), L.ptr(self.b_head), L.ptr(logits),
                                     L.ptr(tg), L.ptr(ws["nll"]) if tg is not None else None,
                                     L.ptr(ws["lse"]) if (train and tg is not None) else None,
                                     L.ptr(ws["h0"]) if train else None, L.ptr(ws["h1"]) if train else None, st), "head")
        return False

    def _bwd_weights_coming(self) -> bool:
        """The fused training head reads the backward's packed head weights during the forward.  True where they are this step's: the
        step's early packing (train.step_open) is in flight -- the current stream then waits for it here; decoder_backward still takes
        the event -- or an accumulation window's earlier micro-batch packed them for these same weights."""
        box = self.flight.early_pack
        if box is not None and box[0] is not None:
            self.join(box[0])
            return True
        win = self.flight.accum
        return win is not None and win.n > 0

    def _head_fwd_wide(self, ws, B, T, logits, tg, train):
        """wavenet.py:204-214 (+ the shifted CE of vqwae_train.py:363-379,:764) for skip widths above 256: three launches of
        wae_gemm_tm -- h0 = relu(sqrt(1/L) (sum_l b_skip_l + W_skip u)), h1 = relu(b1 + W1 h0), logits / nll from b3 + W3 h1."""
        from . import backward as BW
        g = self.g
        bh = self.b_head.data_ptr()
        BW._tm(self, B, T, g.Sp, 3, math.sqrt(1.0 / g.layers), [(ws["u"].data_ptr(), g.Ku, g.Ku, 0)],
               self.w_hwide["skip"].data_ptr(), ws["h0"].data_ptr(), g.Sp, bh, 0)
        BW._tm(self, B, T, g.Sp, 3, 1.0, [(ws["h0"].data_ptr(), g.Sp, g.Sp, 0)], self.w_hwide["w1"].data_ptr(),
               ws["h1"].data_ptr(), g.Sp, bh + g.Sp * 4, 0)
        ce = L.TmCe(logits.data_ptr() if logits is not None else None, tg.data_ptr() if tg is not None else None,
                    ws["nll"].data_ptr() if tg is not None else None,
                    ws["lse"].data_ptr() if (train and tg is not None) else None, None, 0.0, g.O)
        BW._tm_ce(self, B, T, g.Op, 5, [(ws["h1"].data_ptr(), g.Sp, g.Sp, 0)], self.w_hwide["w3"].data_ptr(), None, 0,
                  bh + 2 * g.Sp * 4, ce)
        self.hold("ce", logits, tg)

    # ------------------------------------------------------------------ teacher-forced forward of a list
    def decoder_forward_list(self, items, want_logits: bool = True, want_nll: bool = True, max_rows: Optional[int] = None,
                             c_is_upsampled: bool = False, quantize_channels: int = 65536, log_scale_min: float = -7.0):
        """WaveNet.forward (wavenet.py:164-216) for a LIST of utterances of unequal lengths (include/wae.h: wae_glu_layer_fwd_list,
        wae_nll_segments): logits and the shifted cross-entropy of every utterance, where decoder_forward takes one (B, T) batch, a
        loop of batch-1 forwards is 20+ launches, a workspace and a round trip per utterance, and a zero-padded batch computes every
        pad row of every layer.

        items: a sequence of mappings with `x` ((T_i,) class ids, or floats for a scalar-input decoder), `c` ((Cc, Tc_i) latent frames,
        upsampled here, or the (Cc, T_i) per-sample features when c_is_upsampled or the geometry has no upsampling network; None
        without local conditioning) and `gid` (speaker id or None; all items or none).  Host or device arrays.
        The activations are time-major and packed along time in the caller's order.  A group of the list runs as: wae_gproj_fwd with
        one zb row per item, upsample_list into the packed c_up, ONE wae_first_conv_fwd over all rows, ONE list launch per layer on two
        ping-pong x buffers, the head on the packed rows (it is per column: B = 1, T = rows) and wae_nll_segments.  The launches, the
        allocations and the table uploads (one for the stack, upsample_list's own) do not grow with the number of items.
        max_rows: the most rows (sum T_i) of one group, by default packing.FWD_LIST_MAX_ROWS = 2^20, which keeps the group's u buffer
        (rows x Ku) at 5 GiB in bf16 / 10 GiB in fp32 at hps/vqwae.json's geometry; a longer list runs as consecutive groups (an item
        longer than max_rows is a group of its own).  The bytes of every item are the same for every grouping and every order.
        Returns (results, loss): in the caller's order a list of dict(logits (O, T_i) fp32 | None, nll (T_i,) fp32 | None,
        nll_sum, count) -- views of the group's arrays; nll[t] is taken against x[t + 1], 0 at t = T_i - 1, nll_sum its sum and
        count = T_i - 1 -- and loss = sum nll_sum / sum count over the list (vqwae_train.py:379 with the list as one batch; None
        without want_nll).  logits and nll are, bit for bit, decoder_forward of that utterance alone.
        Scalar-input decoders: logits are the distribution's parameters and nll the mixture loss after the geometry's
        output_distribution, as scalar_loss_and_grad chooses it -- wae_mog_loss_fwd ("Normal") or wae_dmol_loss_fwd with
        quantize_channels, both with log_scale_min -- on the packed (1, O, rows) logits against the packed x with B = 1, T = rows,
        shift = 1 and no gradient.  Those kernels are per column too (T is an address stride and the t + shift >= T test), so every
        row but an item's last is the item's own value bit for bit, and wae_nll_segments zeroes the last rows as it does for the
        cross-entropy.  The logits buffer is internal when want_logits=False.
        ValueError, before any launch: an empty list, an item with T_i < 1, gid on some items only, a c that does not upsample to
        T_i."""
        g, who = self.g, "decoder_forward_list"
        items = list(items)
        Ts, Tcs, _, _ = TR.list_items(who, items, g, "c")
        if g.Ccp:
            Tup = P.upsample_list_plan(Tcs, g, None, c_is_upsampled).Ts       # refuses what upsample_list refuses; not launched
            for i, (a, b) in enumerate(zip(Tup, Ts)):
                if int(a) != b:
                    raise ValueError(f"{who}: item {i}: c {tuple(items[i]['c'].shape)} gives {int(a)} rows != T = {b}")
        cap = P.FWD_LIST_MAX_ROWS if max_rows is None else int(max_rows)
        if cap < 1:
            raise ValueError(f"{who}: max_rows {cap} < 1")
        if self.weights_dirty:
            self.prepare_weights()
        n = len(items)
        sums = torch.zeros(n, dtype=torch.float32, device=self.device) if want_nll else None
        counts = torch.zeros(n, dtype=torch.int32, device=self.device) if want_nll else None
        loss = torch.zeros(2, dtype=torch.float32, device=self.device) if want_nll else None
        out, keep = [], []
        for lo, hi in P.forward_list_groups(Ts, cap):
            out += self._forward_list_group(items[lo:hi], Ts[lo:hi], lo, want_logits, want_nll, c_is_upsampled, sums, counts, loss, keep,
                                            (int(quantize_channels), float(log_scale_min)))
        self.hold("forward_list", *keep)       # the tables and operands passed by raw pointer, until the next list
        return out, (loss[0] if want_nll else None)

    def _forward_list_group(self, items, Ts, first, want_logits, want_nll, c_is_upsampled, sums, counts, loss, keep,
                            mix=(65536, -7.0)):
        """one group of decoder_forward_list: its packed arrays, one table, the launches; -> the items' dicts.
        mix: (quantize_channels, log_scale_min) of a scalar-input decoder's mixture loss"""
        g, lib, st, dev, td = self.g, self.lib, self.stream(), self.device, self.tdtype
        n = len(items)
        plan = P.glu_list_plan(Ts, P.GLU_LIST_TILES[self.dt])
        rows = plan.rows
        table = torch.from_numpy(plan.table).to(dev)
        gid32 = None
        if items[0].get("gid") is not None:
            gid32 = torch.as_tensor(np.asarray([int(it["gid"]) for it in items], dtype=np.int32)).to(dev)
        zb = self._ar_speaker_rows(n, gid32)
        c_up = None
        if g.Ccp:
            c_up, _ = self.upsample_list([it["c"] for it in items], c_is_upsampled=c_is_upsampled)
        self.join(self.flight.take_pack_done())
        # the inputs side by side in order: the host items in one upload
        xi = F.pack_time(self, [it["x"] for it in items], 1, torch.float32 if g.scalar_input else torch.int32).view(-1)
        xs = [torch.empty(rows, g.Rp, dtype=td, device=dev) for _ in range(2)]
        u = torch.empty(rows, g.Ku, dtype=td, device=dev)       # all layers' gated activations
        if g.Ku > g.layers * g.Hp:
            u[:, g.layers * g.Hp:].zero_()                       # the pad columns the head's skip contraction reads
        if g.scalar_input:
            L.check(lib.wae_first_conv_fwd(None, L.ptr(xi), L.ptr(self.first_tab), L.ptr(self.first_bias), L.ptr(xs[0]), rows, g.Rp, 1,
                                           self.dt, None, st), "first_conv")
        else:
            L.check(lib.wae_first_conv_fwd(L.ptr(xi), None, L.ptr(self.first_tab), L.ptr(self.first_bias), L.ptr(xs[0]), rows, g.Rp, g.O,
                                           self.dt, L.ptr(self.err), st), "first_conv")
        es = self.w_glu.element_size()
        for i, dil in enumerate(g.dilations):
            last = i == g.layers - 1
            flags = (L.GLU_NO_OUT if last else 0) | self.glu_flags | (L.GLU_PAIR if self.glu_pair == "inference" else 0)
            dd = L.GluDesc(self.dt, n, 0, g.Rp, g.Ccp, g.Hp, g.k, dil, flags)
            L.check(lib.wae_glu_layer_fwd_list(ctypes.byref(dd), L.ptr(table), n, plan.ntiles, rows, L.ptr(xs[i % 2]),
                                               None if last else L.ptr(xs[(i + 1) % 2]), L.ptr(c_up),
                                               ctypes.c_void_p(u.data_ptr() + i * g.Hp * es), g.Ku,
                                               ctypes.c_void_p(zb.data_ptr() + i * 2 * g.Hp * 4), g.layers * 2 * g.Hp,
                                               ctypes.c_void_p(self.w_glu.data_ptr() + i * self.glu_elems * es),
                                               ctypes.c_void_p(self.b_glu.data_ptr() + i * g.Rp * 4), st), f"glu layer {i} (list)")
        # the head is per column: the packed rows as one clip of `rows` steps; its CE shift crosses the items' ends, wae_nll_segments
        # puts that right
        ws = dict(u=u)
        if self.wide_head or self.split_head:
            ws["h0"] = torch.empty(rows, g.Sp, dtype=td, device=dev)
        if self.wide_head:
            ws["h1"] = torch.empty(rows, g.Sp, dtype=td, device=dev)
        mixture = g.scalar_input and want_nll       # the head has no fused mixture loss: it runs into logits, the loss kernel behind it
        logits = torch.empty(1, g.O, rows, dtype=torch.float32, device=dev) if (want_logits or mixture) else None
        nll = None
        if want_nll:
            nll = ws["nll"] = torch.empty(rows, dtype=torch.float32, device=dev)
        self._head_fwd(ws, 1, rows, logits, xi if (want_nll and not mixture) else None, False)
        if mixture:
            # per column as the head's cross-entropy: row t against x[t + 1] of the packed rows, 0 at the last row of all
            TR.mixture_nll(self, g.output_distribution == "Normal", logits, xi, nll, None, mix, " (list)")
        if want_nll:
            L.check(lib.wae_nll_segments(L.ptr(nll), L.ptr(table), n, rows, first, L.ptr(sums), L.ptr(counts), L.ptr(loss), st),
                    "nll_segments")
        # the small operands passed by raw pointer stay until the next list; the group's activations (x, u, c_up, h0 / h1: gigabytes)
        # go back to the allocator here -- every launch above is on the current stream, and so is whatever takes their memory next
        keep += [table, zb, xi]
        res = []
        for i, (o, T) in enumerate(zip(plan.offsets, Ts)):
            o = int(o)
            res.append(dict(logits=logits[0, :, o:o + T] if want_logits else None, nll=nll[o:o + T] if want_nll else None,
                            nll_sum=sums[first + i] if want_nll else None, count=counts[first + i] if want_nll else None))
        return res

    def forward_list(self, items, want_logits: bool = True, want_nll: bool = True, max_rows: Optional[int] = None,
                     want_latents: bool = True, want_stats: bool = False, beta: float = 0.25, quantize_channels: int = 65536,
                     log_scale_min: float = -7.0):
        """VQVAE.forward (vqvae_model.py:66-72) in eval mode for a LIST of utterances of unequal lengths: encode_list, then
        decoder_forward_list on the quantised latents.  items: mappings with `x` ((T_i,) class ids, or floats for a scalar-input
        decoder), `feats` ((c_in, F_i) features) and `gid`.  Returns (results, loss) as decoder_forward_list, every dict with quant
        (Cc, Tq_i), idx (Tq_i,) and latents (Cc, Tq_i) | None (want_latents=False) besides.  Every item is, bit for bit, forward() of
        that utterance alone -- which a zero-padded batch is not at the utterance ends (encode_list, upsample_list).
        want_stats: every dict gains vq_loss, perp and hist as encode_list_stats(beta=beta) gives them, and the list's
        quantiser totals are in self.last_list_stats; loss stays the NLL mean.  quantize_channels, log_scale_min: the mixture loss of
        a scalar-input decoder (decoder_forward_list).  ValueError as the two list calls."""
        items = list(items)
        if not items:
            raise ValueError("forward_list: an empty list")
        feats = [it["feats"] for it in items]
        enc = (self.encode_list_stats(feats, beta=beta, want_latents=want_latents) if want_stats
               else self.encode_list(feats, want_latents=want_latents))
        dec, loss = self.decoder_forward_list([dict(x=it["x"], c=e["quant"], gid=it.get("gid")) for it, e in zip(items, enc)],
                                              want_logits=want_logits, want_nll=want_nll, max_rows=max_rows,
                                              quantize_channels=quantize_channels, log_scale_min=log_scale_min)
        for d, e in zip(dec, enc):
            d.update(quant=e["quant"], idx=e["idx"], latents=e["latents"])
            if want_stats:
                d.update(vq_loss=e["vq_loss"], perp=e["perp"], hist=e["hist"])
        return dec, loss

    def score_list(self, items, beta: float = 0.25, quantize_channels: int = 65536, log_scale_min: float = -7.0,
                   max_rows: Optional[int] = None):
        """What forward() reports for a batch -- loss, commitment loss, perplexity -- for a LIST of utterances of unequal lengths, per
        utterance and for the list as one batch: forward_list without logits and without latents, with the quantiser's statistics.
        items: as forward_list.  Returns (results, totals): results as forward_list(want_stats=True) (nll, nll_sum, count, quant, idx,
        vq_loss, perp, hist per utterance); totals, a dict of 0-d device tensors:
          ce      sum nll_sum / sum count, the masked mean of vqwae_train.py:379 with the list as one batch (cross-entropy, or the
                  mixture loss of a scalar-input decoder);
          vq_loss (beta + 1) sum sqerr / (Cc sum Tq);  perp: the perplexity of the code counts added over the list;
          loss    ce + vq_loss, the number the reference's dev phase logs;
          count   sum (T_i - 1);  frames: sum Tq_i (both as floats).
        Nothing synchronises: the numbers are read when the caller reads them."""
        res, ce = self.forward_list(items, want_logits=False, want_latents=False, want_stats=True, beta=beta, max_rows=max_rows,
                                    quantize_channels=quantize_channels, log_scale_min=log_scale_min)
        st = self.last_list_stats
        count = sum(int(r["nll"].shape[0]) - 1 for r in res)       # the lengths are host numbers: no read-back
        totals = dict(ce=ce, vq_loss=st[0], perp=st[1], loss=ce + st[0],
                      count=torch.tensor(float(count), dtype=torch.float32, device=self.device), frames=st[2])
        return res, totals

    # ------------------------------------------------------------------ autoregressive synthesis
    def _prepare_ar(self):
        if self._ar_ready:
            return
        g, dev = self.g, self.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        lm, w2_off = P.ar_layer_map(g, self.lay, self.dt)
        self.m_ar_layer, self.ar_w2_off, self.ar_layer_elems = up(lm), int(w2_off), int(lm.size)
        self.m_ar_b2 = up(P.ar_bias2_map(g, self.lay))
        self.m_ar_head = up(P.ar_head_map(g, self.lay, self.dt))
        self.m_ar_hb = up(P.ar_head_bias_map(g, self.lay))
        self.ar_w = torch.zeros(g.layers * self.ar_layer_elems, dtype=self.tdtype, device=dev)
        self.ar_b2 = torch.zeros(g.layers * (g.R + g.S), dtype=torch.float32, device=dev)
        self.ar_wh = torch.zeros(self.m_ar_head.numel(), dtype=self.tdtype, device=dev)
        self.ar_hb = torch.zeros(g.S + g.O, dtype=torch.float32, device=dev)
        roff = P.ar_ring_offsets(g)
        self.ar_ring_off, self.ar_ring_total = up(roff), int(roff[-1])
        self.ar_dil = torch.tensor(g.dilations, dtype=torch.int32, device=dev)
        self._ar_ready = True
        self._ar_packed = False

    def pack_ar_weights(self):
        """Effective (weight-normed) weights -> the matrix-vector layout of ar_fwd.hip; this is the engine's
        make_generation_fast_() (wavenet.py:358-364): weight norm is folded once, not per sample."""
        self._prepare_ar()
        if self.weights_dirty:
            self.prepare_weights()
        lib, st, g, lay = self.lib, self.stream(), self.g, self.lay
        L.check(lib.wae_pack_gather(L.ptr(self.eff), L.ptr(self.m_ar_layer), L.ptr(self.ar_w), self.ar_layer_elems, g.layers,
                                    lay.layer_stride, self.ar_layer_elems, self.dt, st), "pack AR layers")
        L.check(lib.wae_pack_gather(L.ptr(self.eff), L.ptr(self.m_ar_b2), L.ptr(self.ar_b2), g.R + g.S, g.layers,
                                    lay.layer_stride, g.R + g.S, L.WAE_F32, st), "pack AR bias2")
        L.check(lib.wae_pack_gather(L.ptr(self.eff), L.ptr(self.m_ar_head), L.ptr(self.ar_wh), self.m_ar_head.numel(), 1, 0, 0,
                                    self.dt, st), "pack AR head")
        L.check(lib.wae_pack_gather(L.ptr(self.eff), L.ptr(self.m_ar_hb), L.ptr(self.ar_hb), g.S + g.O, 1, 0, 0, L.WAE_F32, st),
                "pack AR head bias")
        self.ar_wm = self._pack_ar_fused()
        self._ar_packed = True

    def ar_path(self, generic: bool = False, one_handover: bool = False, lds_layers: Optional[int] = None,
                reg_layers: Optional[int] = None, scalar_coop: bool = False, scalar_fast: bool = False):
        """Selects the form of the cooperative decode kernel (csrc/ar_coop.hip) for this engine's next incremental_forward calls -- the
        A/B and test handles that rounds 4-5 read from the environment inside the library: `generic` = the any-shape kernel on the
        reference's geometry too; `one_handover` = one exchange per layer on host-formed W1_cur . W_out products (measured slower:
        23.9 against 31.4 kHz; wae_ar_generate_coop_fused); lds_layers / reg_layers = how many layers' weight packets stay in LDS / in
        registers (None: as many as fit, 0: none -- (0, 0) is the streaming form; results are bitwise the same for every split).
        `scalar_coop` = scalar-input decoders ("raw" / "mulaw" inputs) decode on the cooperative any-shape kernel too
        (wae_ar_generate_coop_scalar) where class-id decoders would (<= 8 utterances; R, S, O <= 256; WAE_AR_COOP on; modes "logits" /
        "sample"), else on the one-CU kernel as without it.  Opt-in: the split sums round differently from the one-CU kernel's, whose
        roll-out tests/test_gpu_mog.py pins bit for bit.  No effect on class-id decoders.
        `scalar_fast` = wherever a scalar cooperative decode is routed (incremental_forward / incremental_stream under scalar_coop,
        decode_list_scalar(coop=True), team sessions) it asks for the constant-size scalar kernels (wae_ar_desc.scalar_input = 2) and
        passes this call's generic / lds_layers / reg_layers along; geometries those kernels do not cover (anything but R = G = S = 256,
        3 taps, C = 32, O <= 256) keep the any-shape kernel.  It implies nothing on its own: incremental_forward still needs
        scalar_coop=True to leave the one-CU kernel.  Results differ from the any-shape kernel's by rounding (the sums are split
        differently) and are bitwise the same across single, streamed, list and session decodes at one setting."""
        enc = lambda v: 0 if v is None else (-1 if int(v) == 0 else int(v))  # noqa: E731  (wae_ar_desc: 0 = default, < 0 = none)
        if bool(one_handover) != self.ar_one_handover:
            self._ar_packed = False                    # the products are formed by pack_ar_weights
        self.ar_generic, self.ar_one_handover, self.ar_resident = bool(generic), bool(one_handover), (enc(lds_layers), enc(reg_layers))
        self.ar_scalar_coop, self.ar_scalar_fast = bool(scalar_coop), bool(scalar_fast)
        return self

    def _ar_scalar_path(self):
        """(coop_generic, resident_lds, resident_regs) of a scalar cooperative decode: the engine's own under ar_path(scalar_fast=True),
        else zeros (the any-shape kernel reads none of them).  The caller sets ArDesc.scalar_sized (wae_ar_desc.scalar_input = 2) beside it."""
        if self.ar_scalar_fast:
            return (int(self.ar_generic), self.ar_resident[0], self.ar_resident[1])
        return (0, 0, 0)

    def _pack_ar_fused(self):
        """include/wae.h: wae_ar_generate_coop_fused.  M_l = sqrt(.5) W1_cur[l] W_out[l-1] for the reference's own geometry (the one the
        cooperative kernel has with its sizes as constants), from the packed decode weights: one small matrix product per layer, once per
        weight update -- like make_generation_fast_ (wavenet.py:358-364) it is preparation, not the decode path.  Opt-in (ar_path(one_handover=True)):
        with the exchange's stores no longer waiting for their acknowledgement a hand-over costs ~1.3 k clocks, and the fused layer's
        longer window (its requests miss L2: 11.7 MB of weights cycle through a 4-MB L2 every sample) measures 19 kHz against 22.7."""
        g = self.g
        if not (g.R == 256 and g.S == 256 and g.O == 256 and g.G == 256 and g.k == 3 and g.layers >= 2 and not g.scalar_input
                and self.ar_one_handover):
            return None
        epl = 4 if self.dt == L.WAE_F32 else 8
        K1 = 3 * g.R + max(g.Cc, 0)
        nkb1, nkbh = (K1 + epl - 1) // epl, (g.H + epl - 1) // epl
        g_pad, w_pad = (g.G + 63) // 64 * 64, (g.R + g.S + 63) // 64 * 64
        w = self.ar_w.view(g.layers, self.ar_layer_elems).float()
        w1 = w[:, :nkb1 * g_pad * epl].view(g.layers, nkb1, g_pad, epl)                       # [l][k / epl][row][k % epl]
        w1c = w1[:, 2 * g.R // epl:3 * g.R // epl, :g.G].permute(0, 2, 1, 3).reshape(g.layers, g.G, g.R)      # current tap
        w2 = w[:, self.ar_w2_off:self.ar_w2_off + nkbh * w_pad * epl].view(g.layers, nkbh, w_pad, epl)
        wout = w2[:, :, :g.R].permute(0, 2, 1, 3).reshape(g.layers, g.R, nkbh * epl)[:, :, :g.H]
        wm = torch.zeros(g.layers, g.G, g.H, dtype=torch.float32, device=self.device)
        a, b = w1c[1:].contiguous(), wout[:-1].contiguous()        # (L-1, G, R), (L-1, R, H)
        L.check(self.lib.wae_bmm_f32(L.ptr(a), L.ptr(b), L.ptr(wm[1:]), g.layers - 1, g.G, g.R, g.H, g.R, g.H, g.H, g.G * g.R, g.R * g.H,
                                     g.G * g.H, math.sqrt(0.5), self.stream()), "bmm_f32")
        self.hold("fused", a, b)
        return wm.to(self.tdtype).contiguous()

    def incremental_forward(self, c: Optional[torch.Tensor], gid: Optional[torch.Tensor], T: int, mode: str = "sample",
                            test_inputs: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
                            init_idx: int = 127, c_is_upsampled: bool = False, want_logits: bool = False,
                            gvec: Optional[torch.Tensor] = None, u_mix: Optional[torch.Tensor] = None,
                            u_log: Optional[torch.Tensor] = None, log_scale_min: float = -7.0, clamp_log_scale: bool = False,
                            n_forced: Optional[int] = None, z: Optional[torch.Tensor] = None):
        """WaveNet.incremental_forward (wavenet.py:218-346) as one persistent launch.

        mode "logits": teacher-forced on test_inputs (B,T) class ids (softmax=False, quantize=False) -> logits (B,O,T);
        "argmax": greedy feedback; "sample": categorical draw from `uniforms` (B,T) in [0,1) (torch.rand if None).
        "probs" / "raw" (quantize=False, wavenet.py:335-338 skipped): the softmax probabilities / raw logits of a step are the
        dense input of the next; they come back as `logits` (B,O,T).
        n_forced: test_inputs covers only the first n_forced steps (default: its length), later steps run free in `mode`
        (wavenet.py:300-305).  init_idx: the class fed to step 0 when nothing is forced -- an int for every utterance (wavenet.py:288:
        127) or one id per utterance (wavenet.py:283-297 starts each batch item from its own row of initial_input); ids per utterance
        run as a forced first step.  Returns dict(idx (B,T) int32, logits (B,O,T) | None).
        Scalar-input decoders: test_inputs (B,T) fp32 teacher-forces the inputs (mode "logits" -> the mixture parameters
        (B,3M,T) as `logits`); mode "sample" draws every step from the mixture of logistics on the uniforms u_mix (B,T,M),
        u_log (B,T) (torch.rand in (1e-5, 1-1e-5) if None) -> dict(x (B,T) fp32, logits | None).  With geometry
        output_distribution "Normal" the draw is sample_from_mix_gaussian's (mixture.py:225-270) on u_mix (B,T,M) (M > 1 only) and
        standard normals z (B,T) (torch.rand / torch.randn if z is None); log_scale_min is unused there, as in the reference."""
        s = D.ar_open(self, c, gid, T, mode=mode, test_inputs=test_inputs, uniforms=uniforms, init_idx=init_idx,
                      c_is_upsampled=c_is_upsampled, want_logits=want_logits, gvec=gvec, u_mix=u_mix, u_log=u_log,
                      log_scale_min=log_scale_min, clamp_log_scale=clamp_log_scale, n_forced=n_forced, z=z)
        return D.ar_launch(self, s, 0, int(T))      # the one-chunk case of incremental_stream; _ar_keep holds the operands until the next decode

    def incremental_stream(self, c: Optional[torch.Tensor], gid: Optional[torch.Tensor], T: int, chunk, mode: str = "sample",
                           test_inputs: Optional[torch.Tensor] = None, uniforms: Optional[torch.Tensor] = None,
                           init_idx: int = 127, c_is_upsampled: bool = False, want_logits: bool = False,
                           gvec: Optional[torch.Tensor] = None, u_mix: Optional[torch.Tensor] = None,
                           u_log: Optional[torch.Tensor] = None, log_scale_min: float = -7.0, clamp_log_scale: bool = False,
                           n_forced: Optional[int] = None, z: Optional[torch.Tensor] = None):
        """incremental_forward in resumable launches: a generator over the clip's chunks.

        `chunk`: steps per launch (the last chunk takes what remains), or a sequence of chunk lengths that sums to T.  The other
        arguments are incremental_forward's.  Every item is the dict incremental_forward returns, restricted to the next chunk's steps:
        idx (B,n) / x (B,n), logits (B,O,n) when asked for; concatenated along time the items are the one-shot result of the same
        arguments bit for bit (wae_ar_desc.t0, include/wae.h: a launch with t0 > 0 continues from the history ring the earlier launches
        left, where the reference keeps each conv's input window between calls, conv.py:17-62).
        Opening the stream (this call) is the step incremental_forward opens with (_ar_open): what does not depend on the chunk, once --
        the weight packing, the conditioning upsample of the whole `c` (the encoder side is not causal), the speaker projection, the
        ring and -- where the caller passed none -- the random draws of all T steps, so that a seeded stream equals the seeded one-shot
        call.  The kernel path (cooperative or one CU, C, ar_path() settings) is fixed there too.  Every chunk is then the launch
        incremental_forward makes once for the whole clip (_ar_launch): the operands' time slices, the forced first input (the previous
        chunk's last output, or the teacher-forced value), the chunk-relative n_forced, the zeroed exchange buffers and the time-out
        check (one device read per chunk on the cooperative paths).  Closing the generator early is legal and frees the
        state; nothing of it outlives the generator.  ValueError before any launch: modes "probs" / "raw" (their fed-back vector stays
        on chip), ar_path(one_handover=True), a chunk < 1, chunk lengths that do not sum to T."""
        if mode in ("probs", "raw"):
            raise ValueError(f"incremental_stream: mode '{mode}' feeds a vector back that lives on chip; stream 'logits', 'argmax' or 'sample'")
        if self.ar_one_handover:
            raise ValueError("incremental_stream: the one-hand-over kernel (ar_path(one_handover=True)) cannot continue a decode")
        T = int(T)
        if isinstance(chunk, (int, np.integer)):
            if int(chunk) < 1:
                raise ValueError(f"incremental_stream: chunk {int(chunk)} < 1")
            chunks = [min(int(chunk), T - t) for t in range(0, T, int(chunk))]
        else:
            chunks = [int(n) for n in chunk]
            if not chunks or min(chunks) < 1:
                raise ValueError("incremental_stream: every chunk has at least one step")
            if sum(chunks) != T:
                raise ValueError(f"incremental_stream: the chunk lengths sum to {sum(chunks)}, not to T = {T}")
        s = D.ar_open(self, c, gid, T, mode=mode, test_inputs=test_inputs, uniforms=uniforms, init_idx=init_idx,
                      c_is_upsampled=c_is_upsampled, want_logits=want_logits, gvec=gvec, u_mix=u_mix, u_log=u_log,
                      log_scale_min=log_scale_min, clamp_log_scale=clamp_log_scale, n_forced=n_forced, z=z)
        return D.ar_chunks(self, s, chunks)

    # ---- the engine state every decode route reads (decode.py)
    def _ar_cond_rows(self, c, out, c_is_upsampled, who=""):
        """c (B, Cc, Tc) fp32, contiguous -> out (B, T, Ccp), zeroed, in the model's dtype: the per-sample features as they are
        (already upsampled, or a geometry without an upsampling network), else the latent frames through the upsampling network."""
        g, (B, T) = self.g, out.shape[:2]
        if c_is_upsampled or not g.upsample_scales:
            assert c.shape[-1] == T, f"{who}c {tuple(c.shape)} != T {T}"       # wavenet.py:278
            L.check(self.lib.wae_to_btc(L.ptr(c), L.ptr(out), B, g.Cc, T, g.Ccp, self.dt, self.stream()), "to_btc")
        else:
            assert (c.shape[-1] - 2 * g.cin_pad) * int(np.prod(g.upsample_scales)) == T, f"{who}c does not upsample to T"
            self.upsample_forward(c, out)

    def _ar_speaker_rows(self, n, gid32, gvec=None, zb=None):
        """zb (n, layers, 2Hp) fp32 (default: a new one): every layer's gate bias plus the projection of the speaker vector (gid32's
        embedding row or gvec)."""
        g = self.g
        if zb is None:
            zb = torch.empty(n, g.layers, 2 * g.Hp, dtype=torch.float32, device=self.device)
        wg_off = self.lay.off("wavenet.conv_layers.0.conv1x1g.weight_v") if g.Cg > 0 else -1
        use_gid = gid32 is not None and "wavenet.embed_speakers.weight" in self.lay.offsets
        L.check(self.lib.wae_gproj_fwd(L.ptr(self.eff), wg_off if (gid32 is not None or gvec is not None) else -1,
                                       self.lay.off("wavenet.conv_layers.0.conv.bias"), self.lay.layer_stride,
                                       L.ptr(gid32) if use_gid else None, self.lay.offsets.get("wavenet.embed_speakers.weight", 0),
                                       L.ptr(gvec) if gvec is not None else None, L.ptr(zb), n, g.layers, g.G, g.Hp, max(g.Cg, 0),
                                       int(g.n_speakers or 0), L.ptr(self.err), self.stream()), "gproj")
        return zb

    def _ar_exchange(self, d, C, groups, alloc):
        """(msg, acc, err) of `groups` utterances or teams of C workgroups from `alloc` (torch.zeros / torch.empty: a launch needs them
        zeroed).  err[0] = the time-out flag; the rest: profile counters of a -DWAE_ARC_PROFILE build."""
        nv = self.lib.wae_ar_coop_msg_values(ctypes.byref(d), C)
        return (alloc(groups * 2 * C * nv, dtype=torch.int64, device=self.device),
                alloc(groups * self.lib.wae_ar_coop_acc_floats(ctypes.byref(d)), dtype=torch.float32, device=self.device),
                alloc(64, dtype=torch.int32, device=self.device))

    def _ar_net_args(self, ring, zb, c_up):
        """The 15 network arguments every wae_ar_generate* entry takes behind its descriptor (_lib._AR[1:])."""
        es = self.ar_w.element_size()
        return (L.ptr(self.ar_dil), L.ptr(self.ar_ring_off), L.ptr(ring), self.ar_ring_total, L.ptr(self.ar_w), self.ar_layer_elems * es,
                self.ar_w2_off * es, L.ptr(self.ar_b2), L.ptr(zb), L.ptr(self.first_tab), L.ptr(self.first_bias), L.ptr(self.ar_wh),
                L.ptr(self.ar_hb), L.ptr(c_up), self.dt)

    def _ar_check_exchange(self, err, who):
        self._ar_profile = err
        if int(err[0].item()) != 0:     # synchronises, once per launch: generation is a blocking call for its callers anyway
            raise L.WaeError(f"{who}: an exchange between the cooperating workgroups timed out")

    def decode_list(self, items, mode: str = "sample", slots: Optional[int] = None, want_logits: bool = False,
                    c_is_upsampled: bool = False, coop: bool = False, teams: Optional[int] = None):
        """A work list of utterances of unequal lengths in ONE launch (include/wae.h: wae_ar_generate_list): `slots` persistent
        workgroups, one per CU, each decoding one item after another until the list is empty -- throughput decoding, where
        incremental_forward takes equal lengths only and a loop over it leaves most of the device idle.

        items: a sequence of mappings with `T` (steps), `c` ((Cc, Tc) conditioning or None: the latent frames, upsampled here as
        incremental_forward does, or the (Cc, T) per-sample features when c_is_upsampled or the geometry has no upsampling network),
        `gid` (speaker id or None; all items or none) and optionally `test_inputs` (class ids of the forced prefix, up to T of them),
        `uniforms` ((T,) draws in [0, 1) of mode "sample") and `init_idx` (the start class where nothing is forced; 127 by default).
        mode "logits" (teacher-forced on test_inputs of all T steps), "argmax" or "sample", as incremental_forward.  Where an item has
        no uniforms they are drawn as torch.rand(1, T) on the device, item after item in the caller's order: with the same
        torch.manual_seed before every item this is what a loop of incremental_forward draws.
        slots: workgroups (and ring slots of ar_ring_total floats each) to launch, by default min(len(items), CUs of the device); a
        workgroup's registers fill a CU, so more slots than CUs only queue.  The launch order is longest first (packing.ar_list_plan).
        Returns, in the caller's order, a list of dict(idx (T,) int32, logits (O, T) fp32 | None); every item is, bit for bit, what
        incremental_forward returns for that utterance alone on the one-CU kernel (WAE_AR_COOP=0).
        Always the list kernel: ar_path() and WAE_AR_COOP have no effect here.  Class-id decoders only: a scalar-input geometry
        raises NotImplementedError (its list is decode_list_scalar), an empty list ValueError, both before any launch.

        coop=True: the same list on cooperative teams (include/wae.h: wae_ar_generate_coop_list) -- `teams` teams (default
        min(len(items), 8); clamped to 1..8, one XCD each, and to the item count) of C = min(WAE_AR_COOP_C, 32, H, S) workgroups, each
        team decoding one item after another on the cooperative kernels, longest first (packing.ar_list_plan(Ts, teams)); `slots` is
        not used.  Every item is then, bit for bit, what incremental_forward returns for that utterance alone on the cooperative path
        (WAE_AR_COOP=1, the same ar_path, no one_handover).  ar_path(generic=, lds_layers=, reg_layers=) is honoured as there;
        one_handover is ignored (the one-hand-over kernel has no list form: the list runs two hand-overs per layer).  A wait between
        team-mates that times out raises WaeError after the launch; R, S or O > 256 raises ValueError before any launch."""
        g = self.g
        if g.scalar_input:
            raise NotImplementedError("decode_list: list decoding covers class-id decoders; scalar-input models: use decode_list_scalar "
                                      "(or incremental_forward one batch at a time)")
        if coop:
            D.refuse_wide(g, "decode_list", "list")
        items = list(items)
        if not items:
            raise ValueError("decode_list: an empty list")
        if mode not in ("logits", "argmax", "sample"):
            raise ValueError(f"decode_list: mode '{mode}' is not list-decoded; use 'logits', 'argmax' or 'sample'")
        return D.decode_list(self, "decode_list", items, {"logits": 0, "argmax": 1, "sample": 2}[mode], slots=slots,
                             want_logits=want_logits, c_is_upsampled=c_is_upsampled, coop=coop, teams=teams)

    def scalar_draws(self, T: int):
        """(u_mix (1, T, M) | None, u_log (1, T) or z (1, T)): the draws scalar incremental_forward makes for one utterance of T steps
        where the caller passes none, by the same expressions in the same order (_ar_open; mixture.py:138,151 and :249,266) -- after
        the same torch.manual_seed they are the same numbers."""
        return D.scalar_draws(self, int(T))

    def decode_list_scalar(self, items, mode: str = "sample", slots: Optional[int] = None, want_logits: bool = False,
                           c_is_upsampled: bool = False, coop: bool = False, teams: Optional[int] = None,
                           log_scale_min: float = -7.0, clamp_log_scale: bool = False):
        """decode_list for scalar-input decoders ("raw" / "mulaw" inputs; include/wae.h: wae_ar_generate_scalar_list and
        wae_ar_generate_coop_scalar_list): a work list of utterances of unequal lengths in ONE launch, each step's sample drawn from the
        mixture of logistics or, with geometry output_distribution "Normal", the mixture of Gaussians, as scalar incremental_forward.

        items: mappings with `T`, `c` and `gid` as in decode_list, and optionally `test_inputs` (the float forced prefix, up to T
        values), `u_mix` ((T, M)) together with `u_log` ((T,)) -- or, for "Normal" geometries, `z` ((T,)) and, where M > 1, `u_mix`.
        Draws of the wrong kind for the geometry raise ValueError, as in incremental_forward.  mode "logits": every item is
        teacher-forced on test_inputs of all T steps and its mixture parameters come back (its samples too where every item carries
        draws); mode "sample": the steps behind an item's forced prefix feed the drawn sample back.  Where an item has no draws they
        are made on the device item after item in the caller's order, with incremental_forward's expressions (Logistic:
        torch.rand(1, T, M) * (1 - 2e-5) + 1e-5, then torch.rand(1, T) * (1 - 2e-5) + 1e-5; Normal: the u_mix line when M > 1, then
        torch.randn(1, T)): with the same torch.manual_seed before every item this is what a loop of incremental_forward draws.
        slots / coop / teams: as decode_list.  coop=True is itself the opt-in to the cooperative kernel: ar_path(scalar_coop=) is not
        consulted.  Returns, in the caller's order, a list of dict(x (T,) fp32 | None, logits (O, T) fp32 | None) -- the keys of scalar
        incremental_forward.  With coop=False every item is, bit for bit, incremental_forward for that utterance alone on the one-CU
        kernel; with coop=True on the cooperative path (WAE_AR_COOP=1, ar_path(scalar_coop=True), the same C and the same
        ar_path(scalar_fast=): with it the constant-size scalar kernels where the geometry has them).  A wait between
        team-mates that times out raises WaeError after the launch.  ValueError before any launch: a class-id geometry (use
        decode_list), an empty list, a mode other than "logits" / "sample", coop=True with R, S or O > 256."""
        g, who = self.g, "decode_list_scalar"
        if not g.scalar_input:
            raise ValueError(f"{who}: scalar-input decoders only; a class-id decoder goes through decode_list")
        if coop:
            D.refuse_wide(g, who, "list")
        items = list(items)
        if not items:
            raise ValueError(f"{who}: an empty list")
        if mode not in ("logits", "sample"):
            raise ValueError(f"{who}: mode '{mode}': scalar-input decoders feed the drawn sample back: modes 'logits' and 'sample' only")
        return D.decode_list(self, who, items, {"logits": 0, "sample": 2}[mode], slots=slots, want_logits=want_logits,
                             c_is_upsampled=c_is_upsampled, coop=coop, teams=teams, log_scale_min=log_scale_min,
                             clamp_log_scale=clamp_log_scale)

    def decode_session(self, mode: str = "sample", coop: bool = False, slots: Optional[int] = None, teams: Optional[int] = None,
                       want_logits: bool = False, c_is_upsampled: bool = False, log_scale_min: float = -7.0,
                       clamp_log_scale: bool = False, window: Optional[int] = None) -> DecodeSession:
        """A decode session: decode_list's ragged clips, streamed (include/wae.h: the wae_ar_generate*_spans entries).  Clips join with
        sess.add(item) at any time between two rounds, sess.step(chunk) decodes the next `chunk` steps of every live clip in ONE launch
        and returns them per clip, sess.drop(handle) cancels a clip, sess.close() (or leaving the `with` block) frees everything.
        Every clip keeps its own history ring between the launches, so a span runs on whichever slot or team is free; a clip's chunks,
        concatenated, are bit for bit decode_list's result for it -- that is incremental_forward for the clip alone, on the one-CU
        kernel (coop=False) or on the cooperative path (coop=True, WAE_AR_COOP=1, the same ar_path; one_handover is ignored).
        mode, slots, teams, want_logits, c_is_upsampled: as decode_list; log_scale_min / clamp_log_scale: as decode_list_scalar.
        Class-id decoders decode on `slots` one-CU workgroups or, coop=True, on `teams` cooperative teams (ar_path(generic=,
        lds_layers=, reg_layers=) honoured as in decode_list).  Scalar-input decoders decode in modes "logits" / "sample" (in "logits"
        the mixture parameters come back and x is None): on the slots, or with coop=True on the teams once the engine has opted in with
        ar_path(scalar_coop=True) -- without that opt-in coop=True raises NotImplementedError -- on the any-shape kernel or, under
        ar_path(scalar_fast=True), the constant-size scalar kernels (wae_ar_generate_coop_scalar_spans).  ValueError: R, S or
        O > 256 with coop=True; a mode the matching list call does not take.
        A clip whose conditioning arrives while it decodes joins with h = sess.open(item) (add's mapping without T and c; optional
        max_T), gets latent frames with sess.feed(h, c) / sess.feed_list({h: c, ...}) -- one conv_in launch, one
        wae_upsample_stage_fwd_ranges launch per stage and one table upload per call -- and ends with sess.end(h); step() decodes the
        rows of it that no later frame can change (`ready` in its result).  Its bits are those of the clip decoded whole (DESIGN.md
        3.4.3); cin_pad > 0, an upsample_activation and c_is_upsampled sessions are refused there with NotImplementedError.  In mode
        "logits" an open clip decodes no further than its forced inputs, which must cover T by the time it ends.
        window=W (latent frames): the open clips in constant memory -- a ring of W frames per clip at every stage and of
        W * prod(scales) c_up rows (include/wae.h: wae_upsample_stage_fwd_rings), the same bits; a call feeds a clip
        at most sess.max_feed frames and never over rows it has not decoded (sess.room(h)); ValueError: a window below the minimum."""
        return DecodeSession(self, mode=mode, coop=coop, slots=slots, teams=teams, want_logits=want_logits, c_is_upsampled=c_is_upsampled,
                             log_scale_min=log_scale_min, clamp_log_scale=clamp_log_scale, window=window)

    def decode_list_stream(self, items, chunk, **kw):
        """decode_list / decode_list_scalar in rounds of `chunk` steps: a generator over the rounds of a decode_session(**kw) that holds
        the fixed list `items`.  Every round yields a list in the caller's order: the clip's dict(idx | x, logits, done) for this
        round, None for a clip that finished in an earlier round.  chunk: an int, or a mapping from list index to steps.  The draws of
        clips that bring none are made when the generator starts, clip after clip in the caller's order -- a seeded stream equals the
        seeded list.  Closing the generator early frees the session."""
        items = list(items)
        if not items:
            raise ValueError("decode_list_stream: an empty list")
        sess = self.decode_session(**kw)
        return D.list_rounds(sess, items, chunk)

    # ------------------------------------------------------------------ full autoencoder
    def forward(self, x: torch.Tensor, c: torch.Tensor, gid: Optional[torch.Tensor], targets=None, lengths=None,
                want_logits=True, train=False, beta: float = 0.25, dropout_on: bool = True, layer_events: Optional[list] = None,
                vq_update: Optional[bool] = None):
        """VQVAE.forward (vqvae_model.py:66-72) -> dict(logits, vq_loss, perp, latents, idx, quant, loss).
        vq_update (EMA quantisers): whether this forward moves the codebooks -- the reference's `self.training`, which is not its
        grad mode; default: train."""
        if train and self.flight.accum is None:
            self._refuse_in_window("a train-mode forward outside accumulate()")
        if self.weights_dirty:
            self.prepare_weights()
        sv = Saved(*x.shape) if train else None
        lat = self.encoder_forward(c, sv)
        if self.g.vq == "plain":
            quant, idx, stats = self.vq_forward(lat, beta)
        else:
            quant, idx, stats = self.vq_forward(lat, beta, update=train if vq_update is None else bool(vq_update))
        if train:
            sv.lat, sv.quant, sv.idx, sv.beta = lat, quant, idx, beta
        out = self.decoder_forward(x, quant, gid, targets, lengths, want_logits, train, dropout_on=dropout_on, layer_events=layer_events,
                                   saved=sv)
        out.update(latents=lat, quant=quant, idx=idx, vq_loss=stats[0], perp=stats[1])
        return out

    # ------------------------------------------------------------------ training step (vqwae_train.py:709-798)
    def init_optimizer(self, ema: bool = True):
        TR.init_optimizer(self, ema)

    def backward(self, x, gid, targets, lengths, gvec=None, loss_scale: float = 1.0, ext_dy=None, vq_scale: float = None,
                 grad_sync=None, dy_factor: Optional[float] = None):
        """Gradients of (masked CE or, with ext_dy (B,T,Op) = d loss / d logits, any output loss [+ vq_loss]) of the last
        train-mode forward -> self.grads (flat arena).  loss_scale multiplies the CE term, vq_scale (default: loss_scale) the
        vq_loss term; grad_sync, dy_factor: see backward.decoder_backward.  Inside accumulate() (flight.accum) the gradients stay in the
        accumulators and None is returned."""
        from . import backward as BW
        self._refuse_grad_sync(grad_sync)
        if self.flight.accum is None:
            self._refuse_in_window("backward outside accumulate()")
        self.flight.ev_dc = None
        # (a ragged step's forward left the list front end's record: its backward is the list form's)
        fe_bwd = BW.frontend_backward_list if (self.saved is not None and self.saved.list_fe is not None) else BW.frontend_backward
        dc = BW.decoder_backward(self, x, targets, lengths, gid, gvec, ext_dy=ext_dy, loss_scale=loss_scale, grad_sync=grad_sync,
                                 dy_factor=dy_factor)
        if self.g.Ccp and self.g.upsample_scales:
            if self.flight.ev_dc is not None:
                # dc was complete when the sweep ended (the event): the front end's backward runs on a side stream beside the scatter of
                # the layers' weight gradients that decoder_backward queued behind the sweep (disjoint slices of the gradient arena)
                with self.branch(0, after=self.flight.ev_dc) as tail:
                    fe_bwd(self, dc, loss_scale if vq_scale is None else vq_scale)
                self.join(tail[0])
            else:
                fe_bwd(self, dc, loss_scale if vq_scale is None else vq_scale)
        if self.flight.accum is not None:
            return None
        return BW.finish_grads(self)

    def dmol_loss_and_grad(self, y_hat: torch.Tensor, y: torch.Tensor, lengths, num_classes: int = 65536,
                           log_scale_min: float = -7.0, scale: float = 1.0, factor: Optional[float] = None):
        """DiscretizedMixturelogisticLoss (vqwae_train.py:382-401 with the shift of :766): y_hat (B,3M,T) fp32, y (B,T) fp32
        -> (masked mean loss, scale * d loss / d y_hat as (B,T,Op) in the compute dtype for decoder_backward's ext_dy).
        Per-step loss and its gradient: wae_dmol_loss_fwd; masked mean: wae_masked_mean; mask, 1/count and the transposition
        of the gradient: wae_to_btc_masked."""
        return TR.mixture_loss_and_grad(self, False, y_hat, y, lengths, (num_classes, log_scale_min), scale, factor)

    def mog_loss_and_grad(self, y_hat: torch.Tensor, y: torch.Tensor, lengths, log_scale_min: float = -7.0, scale: float = 1.0,
                          factor: Optional[float] = None):
        """MixtureGaussianLoss (vqwae_train.py:404-422 with the shift of :766): y_hat (B,C,T) fp32 (C = 2 or 3M), y (B,T) fp32
        -> (masked mean loss, scale * d loss / d y_hat as (B,T,Op) in the compute dtype for decoder_backward's ext_dy).
        Per-step loss and its gradient: wae_mog_loss_fwd; masked mean and transposition as in dmol_loss_and_grad."""
        return TR.mixture_loss_and_grad(self, True, y_hat, y, lengths, (0, log_scale_min), scale, factor)

    def scalar_loss_and_grad(self, y_hat, y, lengths, quantize_channels: int = 65536, log_scale_min: float = -7.0,
                             scale: float = 1.0, factor: Optional[float] = None):
        """The criterion of a scalar-input decoder after its output_distribution (vqwae_train.py:802-812)."""
        return TR.mixture_loss_and_grad(self, self.g.output_distribution == "Normal", y_hat, y, lengths, (quantize_channels, log_scale_min),
                                        scale, factor)

    def train_step(self, x, c, gid, lengths=None, lr: float = 4e-4, betas=(0.9, 0.999), eps: float = 1e-8,
                   weight_decay: float = 0.0, clip_thresh: float = 100.0, ema_decay: float = 0.9999, grad_hook=None,
                   quantize_channels: int = 65536, log_scale_min: float = -7.0, grad_sync=None, ce_scale: float = 1.0):
        """One optimisation step: forward (teacher forced, targets = x shifted by one), backward, [data parallel: grad_sync, a
        distributed.GradSync -- its all-reduce starts inside backward and is awaited here; or grad_hook(grads)],
        clip_grad_norm_ + Adam + EMA.  Returns dict(loss, ce, vq_loss, perp, grad_norm).
        ce_scale: factor on the CE gradient (ragged data-parallel shards: n_local * world / n_global, so that the rank mean is
        the gradient of the global masked mean of vqwae_train.py:374-379); vq_loss keeps weight 1 (rank mean, :759).
        Class-id input: masked cross-entropy; scalar input (hparams input_type "raw" / "mulaw"): discretized mixture of logistics,
        or mixture of Gaussians with geometry output_distribution "Normal"."""
        return TR.train_step(self, x, c, gid, lengths, (lr, betas, eps, weight_decay, clip_thresh, ema_decay), grad_hook,
                             (quantize_channels, log_scale_min), grad_sync, ce_scale)

    # ------------------------------------------------------------------ a ragged train step: list front end, dense decoder
    def train_step_list(self, items, lr: float = 4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                        clip_thresh: float = 100.0, ema_decay: float = 0.9999, beta: float = 0.25, grad_hook=None,
                        quantize_channels: int = 65536, log_scale_min: float = -7.0, max_rows: Optional[int] = None, grad_sync=None):
        """One optimisation step on a LIST of utterances of unequal lengths, none of them padded in front of the decoder.
        items: dicts x (T_i,) class ids (or scalars), c (c_in, F_i) features (or, forward_list's name, feats) -- an engine without an
        encoder: c (Cc, Tc_i) -- and gid.
        train_step on the zero-padded batch masks the cross-entropy only: behind the encoder's first block the pad frames are not zero,
        their latents enter the commitment mean, and the conditioning of every utterance's end reads them (DESIGN.md has the figures).
        Here the FRONT END runs on the packed list (encode_list's launches keeping every layer's input, ONE quantiser call on the
        packed latents, the upsampling list chain writing item b's rows of a zero-filled (B, Tmax, Ccp) operand) and the DECODER runs
        dense on the right-padded batch with `lengths`, forward and backward exactly as in train_step: a valid row reads nothing to
        its right, and under the masked loss a pad row sends no gradient to its left.  The list forms of the front end's backward
        (backward.frontend_backward_list) finish the gradients; the optimizer call is train_step's.
        ce = sum nll / sum (T_i - 1); vq_loss and perp are the packed quantiser call's, the list as one batch -- score_list's totals.
        EMA codebooks move once, on the list's packed latents.  Dropout as in train_step.
        Returns dict(loss, ce, vq_loss, perp, grad_norm, rows = B * Tmax, pad_rows = rows - sum T_i): length-sorted lists keep
        pad_rows low.
        ValueError before any launch and any RNG draw: an empty list, a malformed item, len(x_i) != prod(upsample_scales) * Tq_i,
        F_i < 1, B * Tmax > max_rows (default packing.FWD_LIST_MAX_ROWS; the caller splits longer lists).  NotImplementedError before
        any launch: EngineOptions.deterministic (train_step_list_accum runs under it), grad_sync, cin_pad > 0, an upsample_activation, a geometry without an upsampling
        network or one the upsampling list kernels do not cover.  RuntimeError inside an open accumulation window."""
        return TR.train_step_list(self, items, (lr, betas, eps, weight_decay, clip_thresh, ema_decay), beta, grad_hook,
                                  (quantize_channels, log_scale_min), max_rows, grad_sync)

    # ------------------------------------------------------------------ gradient accumulation: micro-batches into one optimizer step
    def latent_elements(self, B: int, frames: int) -> int:
        """Elements of the latents the encoder makes of (B, c_in, frames) features -- what one micro-batch's vq_loss is a mean over
        (distributed.accum_weights); 0 without an encoder."""
        return int(B) * self.g.Cc * P.enc_ready(frames, True) if self.g.has_encoder else 0

    def accumulate(self, x, c, gid, lengths=None, *, ce_weight: float = 1.0, vq_weight: float = 1.0, quantize_channels: int = 65536,
                   log_scale_min: float = -7.0, ce_count: Optional[float] = None):
        """One micro-batch of an accumulation window: train-mode forward and backward INTO the open window (the first call opens it);
        apply_step() closes it with one finish and one optimizer step, discard_step() drops it.  Returns the micro-batch's own numbers
        as device tensors, without a host sync: dict(ce) and, with an encoder, vq_loss and perp.
        ce_weight: the factor on this micro-batch's masked-mean CE (or mixture loss) and its gradient -- train_step's ce_scale;
        vq_weight: the factor on its vq_loss term -- backward's vq_scale.  distributed.accum_weights gives the pair under which the
        window's gradient is that of one step on the concatenated batch.
        ce_count: the window's count of loss positions N where ce_weight = n_i / N.  Given, the factor that reaches d loss / d logits
        is grad_scale / ce_count, formed in double and cast once -- the bits the concatenated batch's backward multiplies by -- instead
        of the product of ce_weight and grad_scale / n_i; ce_weight then only weights the logged loss.
        Micro-batches of one window may differ in B and T (the accumulators are the engine's, the workspaces per shape), but all take
        the same weight-gradient launch (16-bit: B <= 32 and the static launch's clip size, or neither).
        Deferred finishing (backward.decoder_backward): the first micro-batch packs the weights and clears the accumulators; later
        ones skip both; every one runs the sweep, the weight-gradient launches, the consuming zb chain and the front end's backward;
        nothing is scattered, finished or applied before apply_step."""
        return TR.accumulate(self, x, c, gid, lengths, ce_weight, vq_weight, (quantize_channels, log_scale_min), ce_count)

    def apply_step(self, lr: float = 4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                   clip_thresh: float = 100.0, ema_decay: float = 0.9999, grad_hook=None, grad_sync=None):
        """Closes the accumulation window: the finish of the gradients (backward.finish_window: what a plain step's _finish_layers and
        finish_grads do, once for the window), [data parallel: grad_sync.finish() -- the finished arena goes out here, once per
        window and never inside a micro-batch (DDP's no_sync); or grad_hook(grads)], clip_grad_norm_ + Adam + EMA.  opt_step advances
        by one.  Returns dict(loss, ce, grad_norm, micro_batches) and, with an encoder, vq_loss and perp -- 0-d device tensors but
        micro_batches: ce = sum ce_weight_i ce_i, vq_loss = sum vq_weight_i vq_loss_i, loss = ce + vq_loss, perp = the perplexity of
        the micro-batches' code counts added per code (score_list's convention: the concatenated batch's perplexity)."""
        return TR.apply_step(self, (lr, betas, eps, weight_decay, clip_thresh, ema_decay), grad_hook, grad_sync)

    def discard_step(self):
        """Drops an open accumulation window: the accumulators are cleared, the dropout counter goes back to where the window opened,
        nothing of its micro-batches reaches the gradients or the optimizer.  Without an open window: nothing."""
        TR.discard_step(self)

    def train_step_accum(self, batches, lr: float = 4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                         clip_thresh: float = 100.0, ema_decay: float = 0.9999, grad_hook=None, quantize_channels: int = 65536,
                         log_scale_min: float = -7.0, grad_sync=None, ce_scale: float = 1.0):
        """One optimisation step on a sequence of micro-batches (x, c, gid, lengths): the weights of distributed.accum_weights, an
        accumulate() per entry, apply_step().  Under them the step is the one train_step takes on the concatenated batch where the
        micro-batches share T; where they do not (each padded to its own longest clip) it is the step on the global masked mean over
        all loss positions and the mean over all latent elements.  grad_sync: the ranks meet once for the window's count and once in
        apply_step.  ce_scale: one more factor on the CE term.  Returns apply_step's dict."""
        return TR.train_step_accum(self, batches, (lr, betas, eps, weight_decay, clip_thresh, ema_decay), grad_hook,
                                   (quantize_channels, log_scale_min), grad_sync, ce_scale)

    # ------------------------------------------------------------------ ragged micro-batches in accumulation windows
    def accumulate_list(self, items, *, ce_weight: float = 1.0, vq_weight: float = 1.0, ce_count: Optional[float] = None,
                        beta: float = 0.25, quantize_channels: int = 65536, log_scale_min: float = -7.0, max_rows: Optional[int] = None):
        """One RAGGED micro-batch of an accumulation window: train_step_list's items, intake, plan and forward (the list front end in
        front of the dense right-padded decoder) and its backward INTO the open window, as accumulate() does for a dense batch; the
        first call opens the window.  Dense accumulate() calls and accumulate_list() calls may share one window; apply_step() closes
        it, discard_step() drops it.  ce_weight, vq_weight, ce_count: as accumulate's; train.list_meta gives the micro-batch's entry
        for distributed.accum_weights (n = sum_b (T_b - 1), e = Cc * sum Tq_b).  The list front end's backward adds its weight
        gradients into the engine's accumulators, which the window's one finish reads.
        Returns accumulate's dict (ce and, with an encoder, vq_loss and perp: device tensors, no host sync) plus rows and pad_rows.
        Runs under EngineOptions.deterministic (the FIR tap gradient through wae_upsample_stage_bwd_list_det; every other sum of the
        list forms has one owner or a fixed order).
        Before any launch -- ValueError: train_step_list's item and plan refusals; a (B, Tmax) that takes another weight-gradient
        launch than the window's earlier micro-batches (accumulate's rule).  NotImplementedError: train_step_list's geometry refusals;
        the sliced and EMA quantisers (windows cover the plain kind).  A micro-batch that fails half-way takes the window with it
        (discard_step)."""
        return TR.accumulate_list(self, items, ce_weight, vq_weight, ce_count, beta, (quantize_channels, log_scale_min), max_rows)

    def train_step_list_accum(self, groups, lr: float = 4e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                              clip_thresh: float = 100.0, ema_decay: float = 0.9999, beta: float = 0.25, grad_hook=None,
                              quantize_channels: int = 65536, log_scale_min: float = -7.0, max_rows: Optional[int] = None, grad_sync=None):
        """One optimisation step on a sequence of GROUPS, each a list of train_step_list's items: the weights of
        distributed.accum_weights over train.list_meta of every group, an accumulate_list() per group, apply_step().  The step is
        train_step_list on the concatenation of all groups, whose decoder would not fit in one batch: ce = sum nll / sum (T - 1),
        vq_loss and perp those of all latents as one batch (score_list's totals).  max_rows caps each group.  Returns apply_step's
        dict plus the summed rows and pad_rows.  Runs under EngineOptions.deterministic: the same weights, optimizer state, groups
        and dropout seed give the same bits.
        ValueError before any launch: no groups, an empty group, a malformed item in any group.  NotImplementedError: grad_sync
        (ragged steps cover one GPU) and accumulate_list's refusals.  RuntimeError inside an open window."""
        return TR.train_step_list_accum(self, groups, (lr, betas, eps, weight_decay, clip_thresh, ema_decay), beta, grad_hook,
                                        (quantize_channels, log_scale_min), max_rows, grad_sync)
