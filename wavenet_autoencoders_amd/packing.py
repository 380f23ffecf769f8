"""Host logic: parameter arena layout and the index maps that put weights into MFMA A-fragment order.

Everything here is numpy on the host and runs once per model geometry; the maps are uploaded and applied on
the device by ``wae_pack_gather`` (csrc/misc.hip) every time the weights change.

Fragment order (must match csrc/glu_fwd.hip and csrc/head_fwd.hip)
------------------------------------------------------------------
A *fragment block* is 64 lanes x 16 bytes = one A operand of a 32x32 MFMA tile: lane l = (i = l & 31, h = l >> 5)
holds, for output row ``32*m + i`` of M-tile m, EPL consecutive-in-k elements (EPL = 8 bf16 / 4 f32).

GEMM 1 stream ``[pass][q][blk][m][lane][j]`` (chunk q = one 128-byte slice of an activation row; pass p covers the
gate channels [p*NPH*32, (p+1)*NPH*32), NPH = glu_pass_tiles(NP); m < NPH: tanh rows, m >= NPH: sigmoid rows):
    q <  k*(Rp/CK): cblk = q // k, tap = q % k               -> conv weight (G, R, k)  (taps of a column block back to back)
    q >=          : c chunk                                   -> conv1x1c weight (G, Cc)
    channel = cblk*CK + blk*2*EPL + h*EPL + j          (CK = 64 bf16 / 32 f32 channels per chunk)
    gate-a row = 32*(p*NPH + m) + i, gate-b row = H + 32*(p*NPH + m - NPH) + i (reference row = half*H + i)
GEMM 2 stream ``[q2][mt][kb][lane][j]``: M-tile gm = q2*MT2 + mt over [out rows (Rp) | skip rows (Sp)],
    k index = row of u inside accumulator tile ut = kb // KBU, sub-block s = kb % KBU:
      bf16: u_row = 32*ut + 16*s + 8*(j >> 2) + 4*h + (j & 3)
      f32 : u_row = 32*ut +  8*s + 4*h + j
    (the register order in which a 32x32 accumulator tile is reused as the next MFMA's B operand).
"""
from __future__ import annotations

import heapq
import math
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

F32, BF16, F16 = 0, 1, 2    # include/wae.h WAE_F32 / WAE_BF16 / WAE_F16 (fp16 packs exactly like bf16)


def _ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


VQ_KINDS = ("plain", "sliced", "ema", "sliced_ema")


@dataclass
class Geometry:
    """Decoder/encoder sizes (reference ctor args: wavenet.py:98-111, vqvae_model.py:54) + padded sizes."""
    layers: int
    stacks: int
    R: int
    G: int
    S: int
    O: int
    Cc: int = -1
    Cg: int = -1
    k: int = 3
    n_speakers: Optional[int] = None
    upsample_scales: Optional[List[int]] = None
    cin_pad: int = 0
    scalar_input: bool = False
    use_speaker_embedding: bool = True
    # autoencoder front end (None = decoder only)
    c_in: Optional[int] = None
    encoder_hid: Optional[int] = None
    K: int = 256
    dilations_override: Optional[List[int]] = None   # standalone layers (wavenet_vocoder.modules.ResidualConv1dGLU)
    # upsample_net "ConvInUpsampleNetwork" (upsample.py:69-85: a Conv1d of 2 cin_pad + 1 taps without padding in front of the stages;
    # every preset) or, conv_in = False, the plain "UpsampleNetwork" (upsample.py:29-66: the stages alone, the output trimmed by
    # cin_pad * prod(scales) samples at either end) -- the same output length, other state_dict keys
    conv_in: bool = True
    # upsample_activation (upsample.py:44-46): "none" (every preset) or an element-wise torch.nn module behind every stage's FIR --
    # ReLU, LeakyReLU (up_act_slope = negative_slope), Tanh, Sigmoid are implemented (csrc/misc.hip: wae_act_fwd / _bwd).  With an
    # activation the ModuleList holds three modules per stage, so the FIRs sit at up_layers.{3 i + 1}.
    up_act: str = "none"
    up_act_slope: float = 0.01
    # Global features that VARY over time (modules.py:148-152 convolves any (B, Cg, T) tensor): conv1x1g then is one more 1x1 over a
    # time series, exactly what conv1x1c is -- its Cg columns ride behind the Cc columns of the local conditioning in the layer
    # kernel's operand ([c ; g] in c_up, [Wc | Wg] in the packed GEMM-1 stream), forward and backward; the hoisted per-clip projection
    # (gproj) is not used.  Set by the stand-alone layer module when it is handed such a tensor.
    g_local: bool = False
    # output_distribution (wavenet.py:109, hparams.py): the distribution a scalar-input decoder's outputs parameterise -- "Logistic"
    # (discretized mixture of logistics) or "Normal" (mixture of Gaussians, mixture.py:161-270).  Ignored for class-id decoders
    # (mulaw-quantize), as in the reference.
    output_distribution: str = "Logistic"
    # the quantiser between encoder and decoder (vector_quantization.py): "plain" VectorQuantize (:10-49), "sliced"
    # SlicedVectorQuantize (:51-128: vq_slices equal slices of the channel axis, a codebook each; K1: the second codebook's size, as
    # the constructor's K1, default K), "ema" VectorQuantizeEMA (:239-306) and "sliced_ema" SlicedVectorQuantizeEMA (:132-235), whose
    # codebooks move by exponential moving averages (vq_decay) instead of gradients
    vq: str = "plain"
    vq_slices: int = 2
    K1: Optional[int] = None
    vq_decay: float = 0.99

    def __post_init__(self):
        if self.vq not in VQ_KINDS:
            raise ValueError(f"quantiser kind {self.vq!r}: one of {VQ_KINDS}")
        if self.vq in ("sliced", "sliced_ema"):
            if not 2 <= int(self.vq_slices) <= 8:
                raise ValueError(f"vq_slices = {self.vq_slices}: a sliced quantiser has 2..8 slices")
            if self.Cc % int(self.vq_slices) != 0:
                raise ValueError(f"vq_slices = {self.vq_slices} does not divide the latent width Cc = {self.Cc}")
        if self.K1 is not None:
            if self.vq != "sliced":
                raise ValueError(f"K1 belongs to the 'sliced' quantiser (SlicedVectorQuantize(K1=)), not to {self.vq!r}")
            if self.vq_slices != 2:
                raise ValueError(f"K1 is the second of two codebooks: vq_slices = {self.vq_slices}")
        assert self.layers % self.stacks == 0                       # wavenet.py:117
        assert self.G % 2 == 0
        self.H = self.G // 2
        self.Rp = _ru(self.R, 128)
        self.Sp = _ru(self.S, 128)
        self.Op = _ru(self.O, 128)
        self.Ccp = _ru(self.Cc, 64) if self.Cc > 0 else 0
        self.Cx = max(self.Cc, 0)                     # conditioning columns of the layer kernel's operand
        if self.g_local:
            assert self.Cg > 0
            self.Cx += self.Cg
            self.Ccp = _ru(self.Cx, 64)
        self.Hp = _ru(self.H, 32)
        self.NP = self.Hp // 32
        self.Ku = _ru(self.layers * self.Hp, 64)       # columns of the (B,T,Ku) buffer of all layers' gated activations
        per = self.layers // self.stacks
        self.dilations = [2 ** (i % per) for i in range(self.layers)]   # wavenet.py:126
        if self.dilations_override is not None:
            assert len(self.dilations_override) == self.layers
            self.dilations = [int(d) for d in self.dilations_override]
        self.receptive_field = (self.k - 1) * sum(self.dilations) + 1   # wavenet.py:42-60
        self.has_encoder = self.c_in is not None
        self.vq_ema = self.vq in ("ema", "sliced_ema")                  # codebooks moved by EMA statistics, no gradient
        self.vq_n = int(self.vq_slices) if self.vq in ("sliced", "sliced_ema") else 1
        if self.scalar_input:
            if self.output_distribution not in ("Logistic", "Normal"):
                # vqwae_train.py:810-812
                raise RuntimeError(f"Not supported output distribution type: {self.output_distribution}")
            if self.output_distribution == "Normal" and not (self.O == 2 or self.O % 3 == 0):
                # mixture.py:178-182: [mean, log_scale] or nr_mix = C / 3
                raise ValueError(f"output_distribution 'Normal' needs out_channels 2 or a multiple of 3 (got {self.O})")
        if self.up_act == "LeakyReLU" and not self.up_act_slope >= 0.0:
            # wae_act_bwd forms act'(x) from the sign of the stored OUTPUT (csrc/misc.hip: act_bwd_kernel); with a negative slope the
            # output's sign no longer is the input's (torch accepts such slopes): refused, not differentiated wrongly
            raise NotImplementedError(f"upsample_activation LeakyReLU(negative_slope={self.up_act_slope}): negative slopes are not implemented")

    @staticmethod
    def from_cfg(cfg: dict) -> "Geometry":
        return Geometry(layers=cfg["layers"], stacks=cfg["stacks"], R=cfg["R"], G=cfg["G"], S=cfg["S"], O=cfg["O"],
                        Cc=cfg.get("Cc", -1), Cg=cfg.get("Cg", -1), k=cfg.get("k", 3), n_speakers=cfg.get("n_speakers"),
                        upsample_scales=cfg.get("upsample_scales"), cin_pad=cfg.get("cin_pad", 0),
                        scalar_input=bool(cfg.get("scalar_input")), c_in=cfg.get("c_in"),
                        encoder_hid=cfg.get("encoder_hid"), K=cfg.get("K", 256), conv_in=bool(cfg.get("conv_in", True)),
                        up_act=cfg.get("up_act", "none"), up_act_slope=float(cfg.get("up_act_slope", 0.01)),
                        output_distribution=cfg.get("output_distribution", "Logistic"), vq=cfg.get("vq", "plain"),
                        vq_slices=int(cfg.get("vq_slices", 2)), K1=cfg.get("K1"), vq_decay=float(cfg.get("vq_decay", 0.99)))


ENCODER_BLOCKS = [(3, 1), (3, 1), (5, 2), (5, 2), (3, 1), (3, 1), (1, 1), (1, 1), (1, 1), (1, 1)]  # vqvae_model.py:32-40


ENC_LIST_ETS = (8, 16, 32)     # tile lengths of the list kernel (include/wae.h: wae_enc_conv_fwd_list)
# Default cap on the frames of one group of WaeEngine.encode_list: the two ping-pong activation buffers of a group are
# 2 x encoder_hid x sum F_i fp32, so 32768 frames keep them at 192 MiB for encoder_hid = 768 (the width VQVAE defaults to,
# vqvae_model.py:54; 64 MiB at the 256 of hps/vqwae.json).
ENC_LIST_MAX_FRAMES = 32768


class EncListLayer(NamedTuple):
    """One layer of an EncListPlan: (k, stride, pad) of the conv; et, its tile length; nsegs / ntiles and the int32 offsets seg_off /
    tile_off of its segment records (nsegs x 4: in_off, Tin, out_off, Tout) and tile pairs (ntiles x 2: segment, to0) inside the plan's
    one table; in_pitch / out_pitch, the columns of the packed input and output."""
    k: int
    stride: int
    pad: int
    et: int
    nsegs: int
    ntiles: int
    seg_off: int
    tile_off: int
    in_pitch: int
    out_pitch: int


class EncListPlan(NamedTuple):
    """encode_list_plan's answer.  layers: ENCODER_BLOCKS in order, then lin; table: every layer's tables in ONE int32 array (one
    upload); Fs, Tq: frames and latent frames per utterance; in_offsets, q_offsets: the first column of every utterance in the packed
    input and in the packed latents (running sums, the caller's order); total_F, total_Tq: the two pitches."""
    layers: List[EncListLayer]
    table: np.ndarray
    Fs: np.ndarray
    Tq: np.ndarray
    in_offsets: np.ndarray
    q_offsets: np.ndarray
    total_F: int
    total_Tq: int

    def segs(self, i: int) -> np.ndarray:
        ly = self.layers[i]
        return self.table[ly.seg_off:ly.seg_off + 4 * ly.nsegs].reshape(ly.nsegs, 4)

    def tiles(self, i: int) -> np.ndarray:
        ly = self.layers[i]
        return self.table[ly.tile_off:ly.tile_off + 2 * ly.ntiles].reshape(ly.ntiles, 2)


def enc_list_et(Tout) -> int:
    """The tile length of least modelled cost for one launch whose clips (or ranges) have Tout outputs each:
    sum_i ceil(Tout_i / et) * (et + 32); ties go to the longer tile (enc_list_tables explains the model)."""
    Tout = np.asarray(Tout, dtype=np.int64).reshape(-1)
    return int(min(ENC_LIST_ETS, key=lambda e: (int((-(-Tout // e)).sum()) * (e + 32), -e)))


def enc_list_tables(Tin, k: int, stride: int, pad: int, et: Optional[int] = None):
    """Tables of ONE wae_enc_conv_fwd_list launch for utterances of Tin frames packed back to back, in the caller's order:
    -> (segs (n, 4) int32, tiles (ntiles, 2) int32, et, Tout (n,)).  The offsets are the running sums of Tin and of Tout, so the
    pitches are their totals.  The tiles of a segment start at 0, et, 2 et, ... below its Tout: they cover [0, Tout_i) exactly once and
    none reaches into another segment (a tile belongs to one segment; the kernel masks its tail beyond Tout_i).
    et None: the tile length of least modelled cost sum_i ceil(Tout_i / et) * (et + 32) -- a tile costs its et output columns plus a
    fixed part (staging the window, one pass over its 32 channels' weights) put at 32 columns, the value with which a single
    utterance gets exactly the rule of wae_enc_conv_fwd (8 up to 8 outputs, 16 up to 16, else 32); ties go to the longer tile.  A
    model, not a measurement; the choice changes no result."""
    Tin = np.asarray(Tin, dtype=np.int64).reshape(-1)
    if Tin.size < 1:
        raise ValueError("enc_list_tables: an empty list")
    if int(Tin.min()) < 1:
        raise ValueError(f"enc_list_tables: every utterance has at least one frame (got {int(Tin.min())})")
    Tout = (Tin + 2 * pad - k) // stride + 1
    if int(Tout.min()) < 1:
        raise ValueError(f"enc_list_tables: an utterance of {int(Tin[np.argmin(Tout)])} frames has no output under k={k}, pad={pad}")
    if max(int(Tin.sum()), int(Tout.sum())) >= 2 ** 31:
        raise ValueError("enc_list_tables: the packed list does not fit 32-bit columns")
    if et is None:
        et = enc_list_et(Tout)
    if et not in ENC_LIST_ETS:
        raise ValueError(f"enc_list_tables: et {et} is not one of {ENC_LIST_ETS}")
    in_off = np.concatenate([[0], np.cumsum(Tin)[:-1]])
    out_off = np.concatenate([[0], np.cumsum(Tout)[:-1]])
    segs = np.stack([in_off, Tin, out_off, Tout], axis=1).astype(np.int32)
    per = -(-Tout // et)                                           # tiles per segment
    seg_of = np.repeat(np.arange(Tin.size), per)
    first = np.concatenate([[0], np.cumsum(per)[:-1]])             # index of every segment's first tile
    to0 = (np.arange(int(per.sum())) - np.repeat(first, per)) * et
    tiles = np.stack([seg_of, to0], axis=1).astype(np.int32)
    return segs, tiles, int(et), Tout


def encode_list_plan(Fs, et: Optional[int] = None) -> EncListPlan:
    """Launch plan of WaeEngine.encode_list for utterances of Fs feature frames (>= 1 each), packed in the caller's order: the tables
    of every block of ENCODER_BLOCKS (pad k // 2, vqvae_model.py:17-23) and of lin (k = 1), each layer's output offsets being the next
    layer's input offsets.  et: force one tile length (8, 16 or 32) on every layer; None: enc_list_tables chooses per layer.
    Pure numpy: the plan is a function of the lengths alone."""
    Fs = np.asarray(Fs, dtype=np.int64).reshape(-1)
    if Fs.size < 1:
        raise ValueError("encode_list_plan: an empty list")
    if int(Fs.min()) < 1:
        raise ValueError(f"encode_list_plan: every utterance has at least one frame (got {int(Fs.min())})")
    layers, parts, off, T = [], [], 0, Fs
    for k, s in list(ENCODER_BLOCKS) + [(1, 1)]:
        segs, tiles, e, Tout = enc_list_tables(T, k, s, k // 2, et)
        layers.append(EncListLayer(k, s, k // 2, e, len(segs), len(tiles), off, off + segs.size, int(T.sum()), int(Tout.sum())))
        parts += [segs.reshape(-1), tiles.reshape(-1)]
        off += segs.size + tiles.size
        T = Tout
    zero = np.zeros(1, dtype=np.int64)
    return EncListPlan(layers, np.concatenate(parts).astype(np.int32), Fs, T, np.concatenate([zero, np.cumsum(Fs)[:-1]]),
                       np.concatenate([zero, np.cumsum(T)[:-1]]), int(Fs.sum()), int(T.sum()))


def encode_list_groups(Fs, max_frames: int) -> List[Tuple[int, int]]:
    """Consecutive groups [lo, hi) of a list of Fs frames whose sums stay within max_frames; an utterance longer than max_frames is a
    group of its own (an utterance is never split)."""
    if int(max_frames) < 1:
        raise ValueError(f"encode_list_groups: max_frames {int(max_frames)} < 1")
    out, lo, tot = [], 0, 0
    for i, f in enumerate(Fs):
        if i > lo and tot + int(f) > max_frames:
            out.append((lo, i))
            lo, tot = i, 0
        tot += int(f)
    out.append((lo, len(Fs)))
    return out


def vq_seg_table(q_offsets, Tq) -> np.ndarray:
    """(n, 2) int32 records {q_off, Tq} of wae_vq_stats_segments (include/wae.h: wae_vq_seg): item i owns the columns
    [q_off_i, q_off_i + Tq_i) of the packed latents -- encode_list_plan's q_offsets and Tq.  The entry takes no closing record.
    ValueError: an empty list, arrays of unequal sizes, an item with Tq < 1 (with its index), a negative offset, columns at or above
    2^31."""
    offs = np.asarray(q_offsets, dtype=np.int64).reshape(-1)
    Tq = np.asarray(Tq, dtype=np.int64).reshape(-1)
    if Tq.size < 1:
        raise ValueError("vq_seg_table: an empty list")
    if offs.size != Tq.size:
        raise ValueError(f"vq_seg_table: {offs.size} offsets for {Tq.size} items")
    if int(Tq.min()) < 1:
        raise ValueError(f"vq_seg_table: item {int(np.argmax(Tq < 1))} has Tq < 1")
    if int(offs.min()) < 0 or int((offs + Tq).max()) >= 2 ** 31:
        raise ValueError("vq_seg_table: one column offset in [0, 2^31) per item")
    return np.stack([offs, Tq], axis=1).astype(np.int32)


def vq_list_totals(sqerr, hist, D: int, c_loss: float):
    """float64 restatement of wae_vq_stats_segments' `out` from the per-item results (sqerr (n,), hist (n, K)): "the list as one
    batch", the quantiser's counterpart of loss = sum nll_sum / sum count.  -> (vq_loss = c_loss sum sqerr / (D sum Tq), perplexity of
    the counts added per code with N = sum Tq (vector_quantization.py:45-47), sum Tq, sum sqerr); Tq_i is the sum of item i's
    counts."""
    sq = np.asarray(sqerr, dtype=np.float64).reshape(-1)
    h = np.asarray(hist, dtype=np.int64).reshape(sq.size, -1)
    frames = int(h.sum())
    if frames < 1:
        return 0.0, 0.0, 0, 0.0
    p = h.sum(axis=0).astype(np.float64) / frames
    return float(c_loss) * float(sq.sum()) / (D * frames), float(np.exp(-np.sum(p * np.log(p + 1e-10)))), frames, float(sq.sum())


# ---- utterances whose features arrive while they are encoded (include/wae.h: wae_enc_conv_fwd_ranges; EncodeSession.open / feed)
ENC_LAYERS = list(ENCODER_BLOCKS) + [(1, 1)]       # the blocks, then lin: (k, stride), pad k // 2
# columns of a layer's INPUT per feature frame, as a divisor: cap frames of room are cap, cap, cap, ceil(cap / 2) and then
# ceil(cap / 4) columns (the two stride-2 blocks); the last entry is the latents'
ENC_ARENA_DIV = [int(np.prod([s for _, s in ENC_LAYERS[:i]])) for i in range(len(ENC_LAYERS) + 1)]
ENC_ROOM = ENC_ARENA_DIV[-1]       # a clip's room and base are multiples of this many frames, so base / div is exact at every layer


def _enc_final(n, ended, k: int, s: int):
    """output columns of a block (k, s, pad k // 2) that n final input columns make final (numpy arrays or ints): while open
    floor((n - k + p) / s) + 1, 0 where n - k + p < 0 -- output t reads inputs t s - p .. t s - p + k - 1, all below n; once ended
    (n + 2p - k) / s + 1, every output of the clip"""
    p = k // 2
    n = np.asarray(n, dtype=np.int64)
    opened = np.where(n - k + p >= 0, (n - k + p) // s + 1, 0)
    closed = np.where(n >= 1, (n + 2 * p - k) // s + 1, 0)
    return np.where(ended, closed, opened)


def enc_final_rows(frames: int, ended: bool) -> List[int]:
    """Columns of an utterance that are FINAL at the input of every layer of the encoder once `frames` feature frames have arrived:
    entry l is the input of ENC_LAYERS[l] (entry 0 the frames themselves), the last of the 12 entries the latents."""
    rows = [max(int(frames), 0)]
    for k, s in ENC_LAYERS:
        rows.append(int(_enc_final(rows[-1], bool(ended), k, s)))
    return rows


def enc_ready(frames: int, ended: bool) -> int:
    """enc_final_rows' last entry in closed form: max(0, (F - 13) // 4) latent frames while the utterance is open -- latent frame q
    needs 4 q + 17 feature frames -- and (F + 3) // 4 once it has ended."""
    f = max(int(frames), 0)
    return (f + 3) // 4 if ended else max(0, (f - 13) // 4)


class EncFeedLaunch(NamedTuple):
    """One wae_enc_conv_fwd_ranges launch of an EncFeedPlan: layer index into ENC_LAYERS, its (k, stride, pad), the tile length et,
    nrecs records {in_off, Tin, out_col, t_lo, t_hi, tile0} and a closing one at rec_off of the table, ntiles."""
    layer: int
    k: int
    stride: int
    pad: int
    et: int
    nrecs: int
    ntiles: int
    rec_off: int


class EncFeedPlan(NamedTuple):
    """enc_feed_plan's answer.  launches: the layers that have a record, in order (a layer without one is not launched); table: every
    launch's records in ONE int32 array (one upload); ready: latent frames final per clip after this feed; q_off, q_cnt: per clip,
    the first column and the count of its NEW latents in the call's packed output of total_new columns."""
    launches: List[EncFeedLaunch]
    table: np.ndarray
    ready: np.ndarray
    q_off: np.ndarray
    q_cnt: np.ndarray
    total_new: int

    def records(self, i: int) -> np.ndarray:
        ln = self.launches[i]
        return self.table[ln.rec_off:ln.rec_off + 6 * (ln.nrecs + 1)].reshape(ln.nrecs + 1, 6)


def enc_feed_plan(clips) -> EncFeedPlan:
    """The range records of one EncodeSession.feed_list for `clips`, each (base, frames_before, ended_before, frames, ended): base,
    the clip's first column in layer 0's arena, in feature frames and a multiple of ENC_ROOM -- its first column at layer l's input
    is base / ENC_ARENA_DIV[l]; frames_before / ended_before, the state its ranges last ran for; frames / ended, now.  Per layer and
    clip, the output columns this feed (or this end) makes final -- [final before, final now) of enc_final_rows -- computed from the
    input columns final now: while a clip is open no tap of such an output reaches Tin, the guarantee wae_enc_conv_fwd_ranges asks of
    the host.  A block writes at base / div + t_lo of the next layer's arena; lin writes this call's new latents packed, clip after
    clip in the order given.  Empty ranges are left out.  et per launch: enc_list_tables' cost model (enc_list_et) on the ranges' lengths.  Over
    the feeds of a clip the ranges of a layer tile [0, Tout) exactly once.  Pure numpy: a function of the counts alone.
    ValueError: a clip that shrinks or reopens, a base that is negative or no multiple of ENC_ROOM, columns at or above 2^31."""
    cols = np.asarray([tuple(c) for c in clips], dtype=np.int64).reshape(-1, 5)
    base, f0, e0, f1, e1 = (cols[:, j] for j in range(5))
    e0, e1 = e0 != 0, e1 != 0
    bad = (f1 < f0) | (f0 < 0) | (base < 0) | (base % ENC_ROOM != 0) | (e0 & (~e1 | (f1 != f0))) | (e1 & (f1 < 1))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"enc_feed_plan: clip {i}: base {int(base[i])}, frames {int(f0[i])} -> {int(f1[i])}, "
                         f"ended {bool(e0[i])} -> {bool(e1[i])}")
    over = base + np.maximum(f1, 1) >= 2 ** 31
    if over.any():
        raise ValueError(f"enc_feed_plan: clip {int(np.argmax(over))}: its columns reach 2^31")
    before, now = [f0], [f1]         # enc_final_rows for all clips at once
    for k, s in ENC_LAYERS:
        before.append(_enc_final(before[-1], e0, k, s))
        now.append(_enc_final(now[-1], e1, k, s))
    q_cnt = now[-1] - before[-1]
    q_off = _running(q_cnt)
    launches, parts, at = [], [], 0
    for l, (k, s) in enumerate(ENC_LAYERS):
        j = np.nonzero(now[l + 1] > before[l + 1])[0]
        if not j.size:
            continue
        lo, hi = before[l + 1][j], now[l + 1][j]
        et = enc_list_et(hi - lo)
        per = -(-(hi - lo) // et)
        last = l == len(ENC_LAYERS) - 1
        out_col = q_off[j] if last else base[j] // ENC_ARENA_DIV[l + 1] + lo
        rec = np.zeros((j.size + 1, 6), dtype=np.int64)
        rec[:-1] = np.stack([base[j] // ENC_ARENA_DIV[l], now[l][j], out_col, lo, hi, _running(per)], axis=1)
        rec[-1, 5] = int(per.sum())
        launches.append(EncFeedLaunch(l, k, s, k // 2, int(et), int(j.size), int(per.sum()), at))
        parts.append(rec.reshape(-1))
        at += rec.size
    table = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return EncFeedPlan(launches, table, now[-1], q_off, q_cnt, int(q_cnt.sum()))


# ---- the same utterances in RINGS of constant size (include/wae.h: wae_enc_conv_fwd_rings; EncodeSession(window=W))
def _enc_final_forms():
    """(A_l, D_l) per layer input l = 0..11 with enc_final_rows(F, False)[l] == max(0, (F - A_l) // D_l + 1): a block (k, s, pad k // 2)
    maps max(0, (F - A) // D + 1) final inputs to max(0, (F - A - D (k - k // 2 - 1)) // (D s) + 1) final outputs, floors of floors
    composing.  The last entry is enc_ready's (17, 4).  Once ended the counts are (F - 1) // D_l + 1: the form with A = 1."""
    forms = [(1, 1)]
    for k, s in ENC_LAYERS:
        A, D = forms[-1]
        forms.append((A + D * (k - k // 2 - 1), D * s))
    assert [D for _, D in forms] == ENC_ARENA_DIV
    return forms


def enc_window_lag() -> List[int]:
    """Columns of its INPUT that layer l of ENC_LAYERS must still hold between two feeds of an open utterance, at the worst phase:
    with n input columns final, the next output that is not is t = (n - k + p) // s + 1 and its first tap t s - p = n - (k - s) -
    (n - k + p) % s, so k - 1 columns at most -- [2, 2, 4, 4, 2, 2, 0, ...] for ENCODER_BLOCKS.  The residual's column t is the same
    or later."""
    return [k - 1 for k, _ in ENC_LAYERS]


def enc_window_tail() -> List[int]:
    """Columns that the END of an utterance adds at layer l's input beyond those final while it was open, at the worst phase:
    ((F - 1) // D + 1) - ((F - A) // D + 1) <= ceil((A - 1) / D) with _enc_final_forms' (A, D).  The closing ranges write them while
    the layer still reads its retained columns, so every ring has that many columns beyond its share of the window."""
    return [-(-(A - 1) // D) for A, D in _enc_final_forms()[:-1]]


def enc_window_span(n: int) -> int:
    """Feature frames of window that a feed of n frames to an OPEN utterance needs, at the worst phase and layer: layer l's input gains
    at most ceil(n / D_l) columns while its first enc_window_lag()[l] are still read -- max over l of D_l (ceil(n / D_l) + k_l - 1);
    for ENCODER_BLOCKS 4 ceil(n / 4) + 8."""
    n = int(n)
    return max(D * (-(-n // D) + lag) for D, lag in zip(ENC_ARENA_DIV, enc_window_lag()))


def enc_window_min() -> int:
    """The smallest window of an encode session, in feature frames: the retained columns of the worst layer and one ENC_ROOM of feed"""
    return max(D * lag for D, lag in zip(ENC_ARENA_DIV, enc_window_lag())) + ENC_ROOM


def enc_window_max_feed(window: int) -> int:
    """The most feature frames one call may feed an utterance of a session with this window: the largest n with enc_window_span(n) <=
    window (the span grows with n).  ValueError: a window that is no multiple of ENC_ROOM or below enc_window_min()."""
    W = int(window)
    if W % ENC_ROOM != 0 or W < enc_window_min():
        raise ValueError(f"encode window {W}: a multiple of {ENC_ROOM} feature frames, at least {enc_window_min()}")
    n = W
    while enc_window_span(n) > W:
        n -= 1
    return n


def enc_ring_periods(window: int) -> List[int]:
    """Columns of an utterance's ring at the input of every layer: window / ENC_ARENA_DIV[l] + enc_window_tail()[l]"""
    enc_window_max_feed(window)
    return [int(window) // D + t for D, t in zip(ENC_ARENA_DIV, enc_window_tail())]


def enc_feed_plan_rings(clips, window: int) -> EncFeedPlan:
    """enc_feed_plan for utterances that live in rings (EncodeSession(window=W)): `clips` are (slot, frames_before, ended_before,
    frames, ended).  The same ranges per layer and clip, in records of 8 (include/wae.h: wae_enc_ring) {in_off, in_period, Tin,
    out_off, out_period, t_lo, t_hi, tile0}: layer l's input ring of slot i is the columns [i P_l, (i + 1) P_l) of its arena,
    P = enc_ring_periods(window); lin's output is linear (out_period 0), this call's new latents packed.  EncFeedPlan.records
    does not apply: use ring_records(plan, i).
    The planner checks, not the caller: ValueError before anything is launched for a feed of more than enc_window_max_feed(window)
    frames, and for any layer where the columns final after this feed, less the first column its next output still reads (the first
    tap of the first output that was not final BEFORE this feed: this call's own records read from there), exceed the ring."""
    periods = enc_ring_periods(window)
    max_feed = enc_window_max_feed(window)
    cols = np.asarray([tuple(c) for c in clips], dtype=np.int64).reshape(-1, 5)
    slot, f0, e0, f1, e1 = (cols[:, j] for j in range(5))
    e0, e1 = e0 != 0, e1 != 0
    bad = (f1 < f0) | (f0 < 0) | (slot < 0) | (e0 & (~e1 | (f1 != f0))) | (e1 & (f1 < 1))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"enc_feed_plan_rings: clip {i}: slot {int(slot[i])}, frames {int(f0[i])} -> {int(f1[i])}, "
                         f"ended {bool(e0[i])} -> {bool(e1[i])}")
    if (f1 - f0 > max_feed).any():
        i = int(np.argmax(f1 - f0 > max_feed))
        raise ValueError(f"enc_feed_plan_rings: clip {i}: a feed of {int(f1[i] - f0[i])} frames; a window of {int(window)} admits "
                         f"{max_feed} per call")
    if ((slot + 1) * max(periods) >= 2 ** 31).any() or (f1 >= 2 ** 31).any():
        raise ValueError("enc_feed_plan_rings: columns reach 2^31")
    before, now = [f0], [f1]
    for k, s in ENC_LAYERS:
        before.append(_enc_final(before[-1], e0, k, s))
        now.append(_enc_final(now[-1], e1, k, s))
    for l, (k, s) in enumerate(ENC_LAYERS):
        held = now[l] - np.maximum(before[l + 1] * s - k // 2, 0)
        if (held > periods[l]).any():
            i = int(np.argmax(held > periods[l]))
            raise ValueError(f"enc_feed_plan_rings: clip {i}: layer {l} would hold {int(held[i])} columns in a ring of {periods[l]}")
    q_cnt = now[-1] - before[-1]
    q_off = _running(q_cnt)
    launches, parts, at = [], [], 0
    for l, (k, s) in enumerate(ENC_LAYERS):
        j = np.nonzero(now[l + 1] > before[l + 1])[0]
        if not j.size:
            continue
        lo, hi = before[l + 1][j], now[l + 1][j]
        et = enc_list_et(hi - lo)
        per = -(-(hi - lo) // et)
        last = l == len(ENC_LAYERS) - 1
        rec = np.zeros((j.size + 1, 8), dtype=np.int64)
        rec[:-1, 0], rec[:-1, 1], rec[:-1, 2] = slot[j] * periods[l], periods[l], now[l][j]
        rec[:-1, 3], rec[:-1, 4] = (q_off[j], 0) if last else (slot[j] * periods[l + 1], periods[l + 1])
        rec[:-1, 5], rec[:-1, 6], rec[:-1, 7] = lo, hi, _running(per)
        rec[-1, 7] = int(per.sum())
        launches.append(EncFeedLaunch(l, k, s, k // 2, int(et), int(j.size), int(per.sum()), at))
        parts.append(rec.reshape(-1))
        at += rec.size
    table = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return EncFeedPlan(launches, table, now[-1], q_off, q_cnt, int(q_cnt.sum()))


def ring_records(plan, i: int) -> np.ndarray:
    """the (nrecs + 1, 8) records of launch i of a ring plan (enc_feed_plan_rings, session_feed_plan_rings)"""
    ln = plan.launches[i]
    return plan.table[ln.rec_off:ln.rec_off + 8 * (ln.nrecs + 1)].reshape(ln.nrecs + 1, 8)


UP_ACT_KINDS = {"ReLU": 1, "LeakyReLU": 2, "Tanh": 3, "Sigmoid": 4}      # include/wae.h: wae_act_fwd


# ---- the upsampling network over a list (include/wae.h: wae_upsample_stage_fwd_list, wae_to_btc_list)
UPS_LIST_TILE_BTC = 64     # output steps of a time-major tile   (include/wae.h: WAE_UPS_LIST_TILE_BTC)
UPS_LIST_TILE_CT = 256     # output columns of a channel-major tile (include/wae.h: WAE_UPS_LIST_TILE_CT)
# Default cap on the output samples (sum T_i) of one group of WaeEngine.upsample_list: the intermediates of a group are fp32
# (Cc, samples / last scale) and smaller ones before it, so at the reference's geometry (Cc 64, last scale 5: hps/vqwae.json) 2^22
# samples keep the largest at 64 x 2^22 / 5 x 4 B = 205 MiB and the one before it at an eighth of that (scale 8).
UPS_LIST_MAX_SAMPLES = 1 << 22


class UpsListLaunch(NamedTuple):
    """One launch of an UpsListPlan.  kind: "conv_in" (wae_enc_conv_fwd_list with k = 2 cin_pad + 1, pad 0: seg_off / tile_off are
    its wae_seg records and (segment, to0) pairs, et its tile length), "stage" (wae_upsample_stage_fwd_list, channel-major), "last"
    (the same entry, time-major) or "to_btc" (wae_to_btc_list): for these three seg_off is the offset of nsegs + 1 wae_ups_seg records
    {in_off, Tin, out_off, tile0}, the last one closing (tile0 = ntiles), and tile_off is -1.  s: the stage's scale (conv_in: k;
    to_btc: 1).  in_pitch / out_pitch: columns of the packed input and output; out_pitch of "last" / "to_btc": the rows of c_up that
    the records may reach."""
    kind: str
    s: int
    et: int
    nsegs: int
    ntiles: int
    seg_off: int
    tile_off: int
    in_pitch: int
    out_pitch: int


class UpsListPlan(NamedTuple):
    """upsample_list_plan's answer.  launches: the chain in order; table: every launch's records in ONE int32 array (one upload);
    Tcs, Ts: conditioning frames and output rows per item; in_offsets: the first column of every item in the packed input (running
    sums, the caller's order); offsets: the first row of every item in c_up (running sums unless the caller gave them); rows: the rows
    of c_up the plan reaches (max offsets + Ts); in_pitch: sum Tcs; closes_with_to_btc: whether a to_btc launch closes the chain
    (an upsample_activation, the plain UpsampleNetwork's trim, conditioning that is already upsampled, no network)."""
    launches: List[UpsListLaunch]
    table: np.ndarray
    Tcs: np.ndarray
    Ts: np.ndarray
    in_offsets: np.ndarray
    offsets: np.ndarray
    rows: int
    in_pitch: int
    closes_with_to_btc: bool

    def records(self, i: int) -> np.ndarray:
        ln = self.launches[i]
        per = ln.nsegs + (0 if ln.kind == "conv_in" else 1)
        return self.table[ln.seg_off:ln.seg_off + 4 * per].reshape(per, 4)


def _running(x: np.ndarray) -> np.ndarray:
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(x)[:-1]])


def ups_list_records(in_off, Tin, out_off, Tout, tile: int) -> Tuple[np.ndarray, int]:
    """(n + 1, 4) int32 records {in_off, Tin, out_off, tile0} of one list launch whose items have Tout outputs in tiles of `tile`
    (tile0: running sums of ceil(Tout_i / tile); the closing record carries the tile count), and that count.  The tiles of an item
    are tile0_i + 0, 1, ...: they cover [0, Tout_i) once and a tile belongs to one item."""
    per = -(-np.asarray(Tout, dtype=np.int64) // tile)
    n = int(per.sum())
    rec = np.zeros((len(per) + 1, 4), dtype=np.int64)
    rec[:-1, 0], rec[:-1, 1], rec[:-1, 2], rec[:-1, 3] = in_off, Tin, out_off, _running(per)
    rec[-1, 3] = n
    return rec.astype(np.int32), n


def upsample_list_supported(g: Geometry, c_is_upsampled: bool = False) -> bool:
    """Whether the list kernels cover this geometry's conditioning chain; where not, WaeEngine.upsample_list loops upsample_forward.
    conv_in has list kernels for cin_pad <= 2 (k = 1, 3, 5); a last stage that writes the time-major operand itself needs Ccp dividing
    256, 3 s <= 256 and its frames in 64 KiB of LDS (csrc/ups_list.hip)."""
    if c_is_upsampled or not g.upsample_scales:
        return True
    if g.conv_in and g.cin_pad > 2:
        return False
    if (g.cin_pad == 0 or g.conv_in) and g.up_act == "none":       # the last stage is time-major
        s = int(g.upsample_scales[-1])
        nfp = (UPS_LIST_TILE_BTC // s + 5) | 1
        return g.Ccp <= 256 and 256 % g.Ccp == 0 and 3 * s <= 256 and (g.Ccp * nfp + 5 * s + 1) * 4 <= 65536
    return True


def upsample_list_plan(Tcs, g: Geometry, offsets=None, c_is_upsampled: bool = False) -> UpsListPlan:
    """Launch plan of WaeEngine.upsample_list for items of Tcs conditioning frames, packed along time in the caller's order: conv_in
    (ConvInUpsampleNetwork: it eats cin_pad frames at either end), one launch per stage -- the last one time-major straight into c_up
    unless something follows it --, and where something does (an upsample_activation, the plain UpsampleNetwork's trim of
    cin_pad * prod(scales) samples at either end, folded into the records' in_off / Tin) a closing to_btc launch.  c_is_upsampled, or
    a geometry without a network: the to_btc launch alone.  offsets: the first row of every item in c_up (free: the caller's order);
    None: running sums of the items' rows.  Pure numpy: the plan is a function of the lengths alone.
    ValueError, with the item's index: an empty list, an item with no output frame, totals at or above 2^31."""
    Tcs = np.asarray(Tcs, dtype=np.int64).reshape(-1)
    if Tcs.size < 1:
        raise ValueError("upsample_list_plan: an empty list")
    scales = [] if c_is_upsampled else [int(s) for s in (g.upsample_scales or [])]
    prod = int(np.prod(scales)) if scales else 1
    pad = g.cin_pad if scales else 0
    T0 = Tcs - 2 * pad
    if int(T0.min()) < 1:
        i = int(np.argmax(T0 < 1))
        raise ValueError(f"upsample_list_plan: item {i} has no output frame ({int(Tcs[i])} frames"
                         + (f" under cin_pad {pad})" if pad else ")"))
    Ts = T0 * prod
    full = Tcs * prod if (scales and not g.conv_in) else Ts       # columns of the last channel-major activation
    over = np.cumsum(np.maximum(full, Tcs)) >= 2 ** 31
    if over.any():
        raise ValueError(f"upsample_list_plan: item {int(np.argmax(over))}: the packed list reaches 2^31 samples; split it "
                         "(upsample_list_groups)")
    offs = _running(Ts) if offsets is None else np.asarray(offsets, dtype=np.int64).reshape(-1)
    if offs.size != Tcs.size or int(offs.min()) < 0 or int((offs + Ts).max()) >= 2 ** 31:
        raise ValueError("upsample_list_plan: offsets: one row offset in [0, 2^31) per item")
    rows = int((offs + Ts).max())
    launches, parts, at = [], [], 0

    def put(kind, s, et, nsegs, ntiles, arrays, in_pitch, out_pitch):
        nonlocal at
        tile_off = at + arrays[0].size if len(arrays) > 1 else -1
        launches.append(UpsListLaunch(kind, s, et, nsegs, ntiles, at, tile_off, in_pitch, out_pitch))
        for a in arrays:
            parts.append(a.reshape(-1))
            at += a.size

    in_off, Tin, in_pitch = _running(Tcs), Tcs, int(Tcs.sum())
    if scales and g.conv_in:
        k = 2 * g.cin_pad + 1
        segs, tiles, et, To = enc_list_tables(Tcs, k, 1, 0)
        put("conv_in", k, et, len(segs), len(tiles), [segs, tiles], in_pitch, int(To.sum()))
        in_off, Tin, in_pitch = _running(To), To, int(To.sum())
    act = g.up_act != "none"
    trim = 0 if (not scales or g.conv_in) else g.cin_pad * prod
    for i, s in enumerate(scales):
        To = Tin * s
        if i == len(scales) - 1 and trim == 0 and not act:
            rec, nt = ups_list_records(in_off, Tin, offs, To, UPS_LIST_TILE_BTC)
            put("last", s, 0, Tcs.size, nt, [rec], in_pitch, rows)
        else:
            out_off = _running(To)
            rec, nt = ups_list_records(in_off, Tin, out_off, To, UPS_LIST_TILE_CT)
            put("stage", s, 0, Tcs.size, nt, [rec], in_pitch, int(To.sum()))
            in_off, in_pitch = out_off, int(To.sum())
        Tin = To
    closes = not launches or launches[-1].kind != "last"
    if closes:
        rec, nt = ups_list_records(in_off + trim, Tin - 2 * trim, offs, Tin - 2 * trim, UPS_LIST_TILE_BTC)
        put("to_btc", 1, 0, Tcs.size, nt, [rec], in_pitch, rows)
    return UpsListPlan(launches, np.concatenate(parts).astype(np.int32), Tcs, Ts, _running(Tcs), offs, rows, int(Tcs.sum()), closes)


def upsample_list_groups(Ts, max_samples: int = UPS_LIST_MAX_SAMPLES) -> List[Tuple[int, int]]:
    """Consecutive groups [lo, hi) of a list of Ts output samples whose sums stay within max_samples; an item longer than max_samples
    is a group of its own (an item is never split)."""
    if int(max_samples) < 1:
        raise ValueError(f"upsample_list_groups: max_samples {int(max_samples)} < 1")
    return encode_list_groups(Ts, int(max_samples))


# ---- a ragged train step (WaeEngine.train_step_list): the list front end in front of the dense, right-padded decoder
class TrainListPlan(NamedTuple):
    """train_list_plan's answer.  enc: the encoder's list plan (None: an engine without an encoder); ups: the conditioning chain's,
    whose last launch writes item b at the rows [b * Tmax, b * Tmax + T_b) of the dense (B, Tmax, Ccp) operand; Ts: samples per item;
    B, Tmax: the dense decoder's shape; rows = B * Tmax; pad_rows = rows - sum T_i: the rows the decoder spends on padding.
    bwd_table: the records of the backward launches that the forward's tables do not hold, in ONE int32 array -- at fb_off the
    nsegs + 1 wae_ups_seg records of wae_from_btc_list (fb_ntiles tiles of 64 rows: rows b * Tmax + t -> columns of the packed
    (Cc, sum T_i) gradient), at stage_off[i] those of stage i's wae_upsample_stage_bwd_list (stage_ntiles[i] tiles of 256 output
    columns; stage_pitch[i] = (in_pitch, out_pitch), both running sums without gaps)."""
    enc: Optional[EncListPlan]
    ups: UpsListPlan
    Ts: np.ndarray
    B: int
    Tmax: int
    rows: int
    pad_rows: int
    bwd_table: np.ndarray
    fb_off: int
    fb_ntiles: int
    stage_off: List[int]
    stage_ntiles: List[int]
    stage_pitch: List[Tuple[int, int]]


def train_list_plan(g: Geometry, Ts, Fs, max_rows: Optional[int] = None) -> TrainListPlan:
    """Launch plan of WaeEngine.train_step_list for items of Ts samples and Fs feature frames (an engine without an encoder: Fs
    conditioning frames).  Pure numpy: a function of the lengths alone.  ValueError, with the item's index: an empty list, lists of
    unequal sizes, an item without a frame, an item whose samples are not prod(scales) * Tq_i (Tq_i: its latent frames; without an
    encoder its conditioning frames), B * Tmax above max_rows (default FWD_LIST_MAX_ROWS: the caller splits longer lists)."""
    Ts = np.asarray(Ts, dtype=np.int64).reshape(-1)
    Fs = np.asarray(Fs, dtype=np.int64).reshape(-1)
    if Ts.size < 1:
        raise ValueError("train_list_plan: an empty list")
    if Fs.size != Ts.size:
        raise ValueError(f"train_list_plan: {Ts.size} sample counts for {Fs.size} frame counts")
    if int(Fs.min()) < 1:
        raise ValueError(f"train_list_plan: item {int(np.argmax(Fs < 1))} has no frame (F >= 1)")
    if not g.upsample_scales or g.Cc <= 0:
        raise ValueError("train_list_plan: this geometry has no upsampling network in front of the decoder")
    enc = encode_list_plan(Fs) if g.has_encoder else None
    Tq = enc.Tq if enc is not None else Fs
    scales = [int(s) for s in g.upsample_scales]
    prod = int(np.prod(scales))
    wrong = Ts != prod * Tq
    if wrong.any():
        i = int(np.argmax(wrong))
        raise ValueError(f"train_list_plan: item {i} has {int(Ts[i])} samples for {int(Tq[i])} conditioning frames: "
                         f"len(x) == prod(upsample_scales) * Tq = {prod * int(Tq[i])}")
    B, Tmax = int(Ts.size), int(Ts.max())
    cap = FWD_LIST_MAX_ROWS if max_rows is None else int(max_rows)
    if B * Tmax > cap:
        raise ValueError(f"train_list_plan: {B} items padded to {Tmax} samples are {B * Tmax} rows > max_rows {cap}: split the list")
    ups = upsample_list_plan(Tq, g, offsets=np.arange(B, dtype=np.int64) * Tmax)
    parts, at = [], 0
    rec, fb_ntiles = ups_list_records(_running(Ts), Ts, np.arange(B, dtype=np.int64) * Tmax, Ts, UPS_LIST_TILE_BTC)
    fb_off = at
    parts.append(rec.reshape(-1))
    at += rec.size
    stage_off, stage_ntiles, stage_pitch, Tin = [], [], [], Tq
    for s in scales:
        To = Tin * s
        rec, nt = ups_list_records(_running(Tin), Tin, _running(To), To, UPS_LIST_TILE_CT)
        stage_off.append(at)
        stage_ntiles.append(nt)
        stage_pitch.append((int(Tin.sum()), int(To.sum())))
        parts.append(rec.reshape(-1))
        at += rec.size
        Tin = To
    return TrainListPlan(enc, ups, Ts, B, Tmax, B * Tmax, B * Tmax - int(Ts.sum()), np.concatenate(parts).astype(np.int32), fb_off,
                         fb_ntiles, stage_off, stage_ntiles, stage_pitch)


# ---- the teacher-forced gated stack over a list (include/wae.h: wae_glu_layer_fwd_list, wae_nll_segments)
GLU_LIST_TILES = {0: 128, 1: 256, 2: 256}      # dtype (WAE_F32, WAE_BF16, WAE_F16) -> time columns of a tile: wae_glu_list_tile()
# Default cap on the rows (sum T_i) of one group of WaeEngine.decoder_forward_list.  The largest array of a group is u, all layers'
# gated activations, (rows, Ku): at hps/vqwae.json's geometry (20 layers of Hp 128: Ku 2560) 2^20 rows keep it at 5 GiB in bf16 /
# fp16 and 10 GiB in fp32; the (O 256, rows) fp32 logits are 1 GiB beside it.  The reference's utterances are 16 000 .. 240 000
# samples, so a group holds four or more of them.
FWD_LIST_MAX_ROWS = 1 << 20


class GluListPlan(NamedTuple):
    """glu_list_plan's answer.  table: (n + 1, 4) int32 records {row_off, T, zb_row, tile0} (include/wae.h: wae_glu_seg), the last one
    closing (tile0 = ntiles); ntiles: the grid of a layer launch; offsets: the first row of every item; rows: the packed rows the
    records reach (max offsets + Ts); Ts: the lengths."""
    table: np.ndarray
    ntiles: int
    offsets: np.ndarray
    rows: int
    Ts: np.ndarray


def glu_list_plan(Ts, tile: int, offsets=None, zb_rows=None) -> GluListPlan:
    """The table of one list launch of the gated layer for items of Ts steps: item i owns the rows [offsets_i, offsets_i + T_i) of the
    packed time-major arrays (offsets None: running sums, the caller's order -- the rows upsample_list writes) and the tiles
    tile0_i + 0, 1, ..., tile j being its columns [j * tile, min((j + 1) * tile, T_i)); zb_rows: every item's row of zb (None: its
    index).  tile: WaeEngine's dtype decides it (GLU_LIST_TILES / wae_glu_list_tile).  Pure numpy, no loop per item.
    ValueError: an empty list, an item with T < 1 (with its index), a tile < 1, rows at or above 2^31."""
    Ts = np.asarray(Ts, dtype=np.int64).reshape(-1)
    if Ts.size < 1:
        raise ValueError("glu_list_plan: an empty list")
    if int(tile) < 1:
        raise ValueError(f"glu_list_plan: tile {tile} < 1")
    if int(Ts.min()) < 1:
        raise ValueError(f"glu_list_plan: item {int(np.argmax(Ts < 1))} has T < 1")
    offs = _running(Ts) if offsets is None else np.asarray(offsets, dtype=np.int64).reshape(-1)
    zrow = np.arange(Ts.size, dtype=np.int64) if zb_rows is None else np.asarray(zb_rows, dtype=np.int64).reshape(-1)
    if offs.size != Ts.size or zrow.size != Ts.size or int(offs.min()) < 0 or int(zrow.min()) < 0 or int((offs + Ts).max()) >= 2 ** 31:
        raise ValueError("glu_list_plan: one row offset in [0, 2^31) and one zb row >= 0 per item")
    per = -(-Ts // int(tile))
    rec = np.zeros((Ts.size + 1, 4), dtype=np.int64)
    rec[:-1, 0], rec[:-1, 1], rec[:-1, 2], rec[:-1, 3] = offs, Ts, zrow, _running(per)
    rec[-1, 3] = int(per.sum())
    return GluListPlan(rec.astype(np.int32), int(per.sum()), offs, int((offs + Ts).max()), Ts)


def forward_list_groups(Ts, max_rows: int = FWD_LIST_MAX_ROWS) -> List[Tuple[int, int]]:
    """Consecutive groups [lo, hi) of a list of Ts steps whose sums stay within max_rows; an item longer than max_rows is a group of
    its own (an item is never split).  The default keeps a group's u buffer at the size FWD_LIST_MAX_ROWS states."""
    if int(max_rows) < 1:
        raise ValueError(f"forward_list_groups: max_rows {int(max_rows)} < 1")
    return encode_list_groups(Ts, int(max_rows))


def nll_segments_restated(nll, table):
    """numpy restatement of wae_nll_segments (csrc/nll_list.hip) on a COPY of nll (rows,) fp32 and glu_list_plan's table (its closing
    record is not an item): thread j of 256 adds the item's rows j, j + 256, ... below T - 1 in fp64, the 64 lanes of a wave meet by a xor
    butterfly, the four waves add in order; the item's last row becomes 0; the list's mean walks nll_sum in table order and is 0 for
    a total count of 0.  -> (nll, nll_sum (n,) fp32, count (n,) int32, loss fp32)."""
    nll = np.array(nll, dtype=np.float32).reshape(-1)
    recs = np.asarray(table).reshape(-1, 4)[:-1]         # without the closing record
    sums, cnts = np.zeros(len(recs), dtype=np.float32), np.zeros(len(recs), dtype=np.int32)
    for i, (off, T, _, _) in enumerate(recs):
        if T < 1 or off < 0 or off + T > nll.size:
            continue
        lane = np.zeros(256, dtype=np.float64)
        body = nll[off:off + T - 1].astype(np.float64)
        full = (len(body) // 256) * 256
        for r in body[:full].reshape(-1, 256):           # one row of the strided walk at a time: every thread's own order
            lane += r
        lane[:len(body) - full] += body[full:]
        w = lane.reshape(4, 64)
        o = 32
        while o:                                         # s += shfl_xor(s, o): every lane ends with the same tree's sum
            w = w + w[:, np.arange(64) ^ o]
            o >>= 1
        tot = 0.0
        for k in range(4):
            tot += w[k, 0]
        sums[i], cnts[i] = np.float32(tot), T - 1
        nll[off + T - 1] = 0.0
    tot = cnt = 0.0
    for s, c in zip(sums, cnts):
        tot += float(s)
        cnt += float(c)
    return nll, sums, cnts, np.float32(tot / cnt) if cnt > 0 else np.float32(0.0)


# ---- clips whose conditioning arrives while they decode (include/wae.h: wae_upsample_stage_fwd_ranges; DecodeSession.open / feed)
def feed_final_rows(frames: int, scales, ended: bool) -> List[int]:
    """Rows of a clip that are FINAL at every level of the upsampling chain once `frames` latent frames have arrived: entry 0 is the
    frames themselves (stage 0's input), entry i + 1 the output of stage i, the last one audio-rate rows (`ready`).  Output row t of a
    stage by s reads its input frames t/s - 1 .. t/s + 1, so n final input rows make (n - 1) * s output rows final while the clip is
    open and n * s once it has ended."""
    rows = [max(int(frames), 0)]
    for s in scales:
        rows.append(rows[-1] * int(s) if ended else max(rows[-1] - 1, 0) * int(s))
    return rows


def feed_ready(frames: int, scales, ended: bool) -> int:
    """feed_final_rows' last entry in closed form: prod * (F - 1) - sum_{i >= 1} prod(scales[i:]) while open (0 where that is
    negative), prod * F once ended.  hps/vqwae.json's [4, 4, 8, 5]: 640 (F - 1) - 205, a lookahead of 845 samples."""
    prod, look = feed_lookahead(scales)
    return max(int(frames), 0) * prod if ended else max(0, prod * (int(frames) - 1) - look)


def feed_lookahead(scales) -> Tuple[int, int]:
    """(prod(scales), sum_{i >= 1} prod(scales[i:])): the audio-rate rows of a latent frame, and the rows beyond one frame that an
    open clip holds back"""
    sc = [int(s) for s in scales]
    return int(np.prod(sc)), sum(int(np.prod(sc[i:])) for i in range(1, len(sc)))


class FeedClip(NamedTuple):
    """One clip of a session_feed_plan.  base: the clip's first column in stage 0's arena, in latent frames -- its first column at
    stage i is base * prod(scales[:i]), its first c_up row base * prod(scales); frames_before / ended_before: the frames that had
    arrived, and whether the clip had ended, when its ranges last ran; frames / ended: now."""
    base: int
    frames_before: int
    ended_before: bool
    frames: int
    ended: bool


class FeedLaunch(NamedTuple):
    """One wae_upsample_stage_fwd_ranges launch of a FeedPlan: stage index and scale, last (time-major into c_up), nrecs records
    {in_off, Tin, out_off, t_lo, t_hi, tile0} and a closing one at rec_off of the table, ntiles."""
    stage: int
    s: int
    last: bool
    nrecs: int
    ntiles: int
    rec_off: int


class FeedPlan(NamedTuple):
    """session_feed_plan's answer.  launches: the stages that have a record, in order (a stage without one is not launched); table:
    every launch's records in ONE int32 array (one upload); ready: audio-rate rows final per clip after this feed."""
    launches: List[FeedLaunch]
    table: np.ndarray
    ready: np.ndarray

    def records(self, i: int) -> np.ndarray:
        ln = self.launches[i]
        return self.table[ln.rec_off:ln.rec_off + 6 * (ln.nrecs + 1)].reshape(ln.nrecs + 1, 6)


def session_feed_plan(scales, clips) -> FeedPlan:
    """The range records of one DecodeSession.feed_list for `clips` (FeedClip, or its five fields as a tuple, per open clip): per
    stage and clip, the output rows that this feed (or this end) makes final
    -- [final before, final now) of feed_final_rows -- computed from the input rows final now.  While a clip is open its record has
    t_hi = (Tin - 1) * s, once ended t_hi = Tin * s: the guarantee wae_upsample_stage_fwd_ranges asks of the host.  Records with empty
    ranges are left out.  Over the feeds of a clip the ranges of a stage tile [0, T) exactly once.  Pure numpy: a function of the
    counts alone.  ValueError: no scales, a clip that shrinks or reopens, columns or rows at or above 2^31."""
    sc = [int(s) for s in scales]
    if not sc or min(sc) < 1:
        raise ValueError(f"session_feed_plan: scales {sc}: at least one stage, every scale >= 1")
    cols = np.asarray([tuple(c) for c in clips], dtype=np.int64).reshape(-1, 5)
    base, f0, e0, f1, e1 = (cols[:, k] for k in range(5))
    e0, e1 = e0 != 0, e1 != 0
    mul = [int(np.prod(sc[:i])) for i in range(len(sc) + 1)]
    bad = (f1 < f0) | (f0 < 0) | (base < 0) | (e0 & (~e1 | (f1 != f0)))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"session_feed_plan: clip {i}: frames {int(f0[i])} -> {int(f1[i])}, ended {bool(e0[i])} -> {bool(e1[i])}")
    over = (base + np.maximum(f1, 1)) * mul[-1] >= 2 ** 31
    if over.any():
        raise ValueError(f"session_feed_plan: clip {int(np.argmax(over))}: its rows reach 2^31")
    before, now = [f0], [f1]         # feed_final_rows for all clips at once
    for s in sc:
        before.append(np.where(e0, before[-1], np.maximum(before[-1] - 1, 0)) * s)
        now.append(np.where(e1, now[-1], np.maximum(now[-1] - 1, 0)) * s)
    launches, parts, at = [], [], 0
    for i, s in enumerate(sc):
        last = i == len(sc) - 1
        tile = UPS_LIST_TILE_BTC if last else UPS_LIST_TILE_CT
        k = np.nonzero(now[i + 1] > before[i + 1])[0]
        if not k.size:
            continue
        lo, hi = before[i + 1][k], now[i + 1][k]
        per = -(-(hi - lo) // tile)
        rec = np.zeros((k.size + 1, 6), dtype=np.int64)
        rec[:-1] = np.stack([base[k] * mul[i], now[i][k], base[k] * mul[i + 1], lo, hi, _running(per)], axis=1)
        rec[-1, 5] = int(per.sum())
        launches.append(FeedLaunch(i, s, last, int(k.size), int(per.sum()), at))
        parts.append(rec.reshape(-1))
        at += rec.size
    table = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return FeedPlan(launches, table, now[-1])


# ---- the same clips in RINGS of constant size (include/wae.h: wae_upsample_stage_fwd_rings; DecodeSession(window=W))
def feed_window_lag(scales) -> List[int]:
    """Input frames that stage i must still hold between two feeds of an open clip: with n of them final the first output row that
    is not is (n - 1) s, which reads the frames n - 2 .. n -- two, at every stage."""
    return [2 for _ in scales]


def feed_window_held(scales, k: int) -> List[int]:
    """The most columns stage i's input ring holds during one call that feeds an open clip k frames and may end it, at the worst
    phase: the columns final after the call less the first one its records read.  Stage 0: the k new frames and the 2 retained.
    Stage i >= 1: its input grows by mul_i per frame, and the end adds the mul_i + look_i columns that waited for a next frame
    (look_i = sum_{1 <= j < i} prod(scales[j:i])): mul_i (k + 1) + look_i + 2."""
    sc = [int(s) for s in scales]
    mul = [int(np.prod(sc[:i])) for i in range(len(sc))]
    look = [sum(int(np.prod(sc[j:i])) for j in range(1, i)) for i in range(len(sc))]
    return [int(k) + 2] + [mul[i] * (int(k) + 1) + look[i] + 2 for i in range(1, len(sc))]


def feed_window_max_feed(scales, window: int) -> int:
    """The most latent frames one call may feed a clip of a decode session with this window (0: the window is too small): the largest
    k whose feed_window_held fits the rings of window * prod(scales[:i]) columns."""
    sc, W = [int(s) for s in scales], int(window)
    mul = [int(np.prod(sc[:i])) for i in range(len(sc))]
    k = max(W, 0)
    while k > 0 and any(h > W * m for h, m in zip(feed_window_held(sc, k), mul)):
        k -= 1
    return k


def feed_window_min(scales) -> int:
    """The smallest window of a decode session, in latent frames: one frame of feed at every stage, and c_up rows for the lookahead
    an open clip holds back plus one frame (feed_lookahead)."""
    prod, look = feed_lookahead(scales)
    W = -(-(look + prod) // prod)
    while feed_window_max_feed(scales, W) < 1:
        W += 1
    return W


def session_feed_plan_rings(scales, clips, window: int) -> FeedPlan:
    """session_feed_plan for clips that live in rings (DecodeSession(window=W)): `clips` are (slot, frames_before, ended_before,
    frames, ended, pos), pos being the audio-rate rows the clip has decoded.  The same ranges per stage and clip, in records of 8
    (include/wae.h: wae_ups_ring) {in_off, in_period, Tin, out_off, out_period, t_lo, t_hi, tile0}: stage i's input ring of slot j is
    the columns [j P_i, (j + 1) P_i) of its arena, P_i = window * prod(scales[:i]); the c_up ring, window * prod(scales) rows.
    FeedPlan.records does not apply: use ring_records(plan, i).
    The planner checks, not the caller -- ValueError before anything is launched: a window below feed_window_min, a stage whose
    columns final after this call, less the first frame its records read (input frame final_out / s - 1 of BEFORE this call), exceed
    its ring, and -- back-pressure -- c_up rows final after this call that would overwrite rows the clip has not decoded
    (ready - pos > window * prod(scales))."""
    sc, W = [int(s) for s in scales], int(window)
    if not sc or min(sc) < 1:
        raise ValueError(f"session_feed_plan_rings: scales {sc}: at least one stage, every scale >= 1")
    if W < feed_window_min(sc):
        raise ValueError(f"session_feed_plan_rings: window {W} is below the minimum of {feed_window_min(sc)} latent frames")
    cols = np.asarray([tuple(c) for c in clips], dtype=np.int64).reshape(-1, 6)
    slot, f0, e0, f1, e1, pos = (cols[:, k] for k in range(6))
    e0, e1 = e0 != 0, e1 != 0
    mul = [int(np.prod(sc[:i])) for i in range(len(sc) + 1)]
    bad = (f1 < f0) | (f0 < 0) | (slot < 0) | (pos < 0) | (e0 & (~e1 | (f1 != f0)))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"session_feed_plan_rings: clip {i}: frames {int(f0[i])} -> {int(f1[i])}, ended {bool(e0[i])} -> {bool(e1[i])}")
    over = (np.maximum(f1, 1) * mul[-1] >= 2 ** 31) | ((slot + 1) * W * mul[-1] >= 2 ** 31)
    if over.any():
        raise ValueError(f"session_feed_plan_rings: clip {int(np.argmax(over))}: its rows reach 2^31")
    before, now = [f0], [f1]
    for s in sc:
        before.append(np.where(e0, before[-1], np.maximum(before[-1] - 1, 0)) * s)
        now.append(np.where(e1, now[-1], np.maximum(now[-1] - 1, 0)) * s)
    for i, s in enumerate(sc):
        held = now[i] - np.maximum(before[i + 1] // s - 1, 0)
        if (held > W * mul[i]).any():
            j = int(np.argmax(held > W * mul[i]))
            raise ValueError(f"session_feed_plan_rings: clip {j}: stage {i} would hold {int(held[j])} columns in a ring of {W * mul[i]} "
                             f"(a window of {W} admits {feed_window_max_feed(sc, W)} frames per call)")
    full = now[-1] - pos > W * mul[-1]
    if full.any():
        j = int(np.argmax(full))
        raise ValueError(f"session_feed_plan_rings: clip {j}: {int(now[-1][j])} final rows with {int(pos[j])} decoded do not fit the "
                         f"{W * mul[-1]} rows of its c_up ring: step first")
    launches, parts, at = [], [], 0
    for i, s in enumerate(sc):
        last = i == len(sc) - 1
        tile = UPS_LIST_TILE_BTC if last else UPS_LIST_TILE_CT
        k = np.nonzero(now[i + 1] > before[i + 1])[0]
        if not k.size:
            continue
        lo, hi = before[i + 1][k], now[i + 1][k]
        per = -(-(hi - lo) // tile)
        rec = np.zeros((k.size + 1, 8), dtype=np.int64)
        rec[:-1] = np.stack([slot[k] * W * mul[i], np.full(k.size, W * mul[i]), now[i][k], slot[k] * W * mul[i + 1],
                             np.full(k.size, W * mul[i + 1]), lo, hi, _running(per)], axis=1)
        rec[-1, 7] = int(per.sum())
        launches.append(FeedLaunch(i, s, last, int(k.size), int(per.sum()), at))
        parts.append(rec.reshape(-1))
        at += rec.size
    table = np.concatenate(parts).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)
    return FeedPlan(launches, table, now[-1])


def up_stage_name(g: Geometry, i: int) -> str:
    """state_dict prefix of upsampling stage i's smoothing FIR: the ModuleList holds [Stretch2d, Conv2d] per stage (upsample.py:38-44),
    under `.upsample` when ConvInUpsampleNetwork wraps it (upsample.py:80-82)"""
    per = 2 if g.up_act == "none" else 3
    return f"wavenet.upsample_net.{'upsample.' if g.conv_in else ''}up_layers.{per * i + 1}"


def param_specs(g: Geometry) -> List[Tuple[str, Tuple[int, ...], bool]]:
    """(name, shape, is_weight_norm_v) in the reference's registration order (state_dict keys)."""
    out: List[Tuple[str, Tuple[int, ...], bool]] = []

    def wn(prefix, cout, cin, k, bias=True, conv2d=False):
        if bias:
            out.append((prefix + ".bias", (cout,), False))
        gs = (cout, 1, 1, 1) if conv2d else (cout, 1, 1)
        vs = (cout, cin, 1, k) if conv2d else (cout, cin, k)
        out.append((prefix + ".weight_g", gs, False))
        out.append((prefix + ".weight_v", vs, True))

    wn("wavenet.first_conv", g.R, 1 if g.scalar_input else g.O, 1)
    for i in range(g.layers):
        p = f"wavenet.conv_layers.{i}."
        wn(p + "conv", g.G, g.R, g.k)
        if g.Cc > 0:
            wn(p + "conv1x1c", g.G, g.Cc, 1, bias=False)
        if g.Cg > 0:
            wn(p + "conv1x1g", g.G, g.Cg, 1, bias=False)
        wn(p + "conv1x1_out", g.R, g.H, 1)
        wn(p + "conv1x1_skip", g.S, g.H, 1)
    wn("wavenet.last_conv_layers.1", g.S, g.S, 1)
    wn("wavenet.last_conv_layers.3", g.O, g.S, 1)
    if g.Cg > 0 and g.use_speaker_embedding and g.n_speakers:
        out.append(("wavenet.embed_speakers.weight", (g.n_speakers, g.Cg), False))
    if g.upsample_scales:
        if g.conv_in:
            out.append(("wavenet.upsample_net.conv_in.weight", (g.Cc, g.Cc, 2 * g.cin_pad + 1), False))
        for i, s in enumerate(g.upsample_scales):
            wn(up_stage_name(g, i), 1, 1, 2 * s + 1, bias=False, conv2d=True)
    if g.has_encoder:
        dims = [(g.c_in, g.encoder_hid)] + [(g.encoder_hid, g.encoder_hid)] * 9
        for i, ((ci, co), (kk, _)) in enumerate(zip(dims, ENCODER_BLOCKS)):
            out.append((f"encoder.net.{i}.conv.weight", (co, ci, kk), False))
            out.append((f"encoder.net.{i}.conv.bias", (co,), False))
        out.append(("encoder.lin.weight", (g.Cc, g.encoder_hid), False))
        out.append(("encoder.lin.bias", (g.Cc,), False))
        out += [(name + ".weight", (K, D), False) for name, _, D, K in vq_slice_specs(g)]
    return out


def vq_slice_specs(g: Geometry) -> List[Tuple[str, int, int, int]]:
    """(codebook module name, d0, D, K) per slice of the geometry's quantiser: the whole width under `vq.embedding` for "plain" and
    "ema"; vq_slices equal slices under `vq.embedding{1..n}` (the reference's names for n = 2, vector_quantization.py:62-65, :143-146)
    for the sliced kinds, the second of two with K1 codes where given."""
    if g.vq_n == 1:
        return [("vq.embedding", 0, g.Cc, g.K)]
    D = g.Cc // g.vq_n
    return [(f"vq.embedding{s + 1}", s * D, D, g.K1 if (s == 1 and g.K1 is not None) else g.K) for s in range(g.vq_n)]


def vq_coeffs(g: Geometry, beta: float) -> Tuple[float, float, Optional[float]]:
    """(c_loss, c_lat, c_emb) of the geometry's quantiser: vq_loss = c_loss * mse forward; d vq_loss / d latents carries c_lat and
    d / d codebook c_emb (None: no codebook gradient).  plain: (:41-43) the two terms' forward values are equal; sliced: weight 1 on
    the encoder-side term, beta on the codebook's (:113-118); EMA kinds: beta * mse(sg[q], x) alone (:220, :294)."""
    if g.vq_ema:
        return float(beta), float(beta), None
    if g.vq == "sliced":
        return 1.0 + float(beta), 1.0, float(beta)
    return float(beta) + 1.0, float(beta), 1.0


def vq_buffer_specs(g: Geometry) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the EMA kinds' statistics in the reference's registration order (vector_quantization.py:148-153, :251-253):
    vq.ema_cluster_size[s] (K,) and vq.ema_w[s] (K, D_s), the suffix absent for "ema", 1..n for "sliced_ema"."""
    if not (g.vq_ema and g.has_encoder):
        return []
    out = []
    for name, _, D, K in vq_slice_specs(g):
        sfx = name[len("vq.embedding"):]
        out += [("vq.ema_cluster_size" + sfx, (K,)), ("vq.ema_w" + sfx, (K, D))]
    return out


class ParamLayout:
    """Flat fp32 arena: name -> (offset, shape).  One contiguous buffer for parameters, one for gradients,
    one for the effective (weight-normed) weights: a single all-reduce / optimizer launch covers everything."""

    def __init__(self, g: Geometry):
        self.geom = g
        self.offsets: "OrderedDict[str, int]" = OrderedDict()
        self.shapes: Dict[str, Tuple[int, ...]] = {}
        off = 0
        v_off, g_off, cols = [], [], []
        for name, shape, is_v in param_specs(g):
            n = int(np.prod(shape))
            self.offsets[name] = off
            self.shapes[name] = shape
            off += _ru(n, 4)            # keep every tensor 16-byte aligned
        self.total = off
        for name, shape, is_v in param_specs(g):
            if is_v:
                rows = shape[0]
                c = int(np.prod(shape[1:]))
                gname = name[:-1] + "g"
                for r in range(rows):
                    v_off.append(self.offsets[name] + r * c)
                    g_off.append(self.offsets[gname] + r)
                    cols.append(c)
        self.wn_v_off = np.asarray(v_off, dtype=np.int64)
        self.wn_g_off = np.asarray(g_off, dtype=np.int64)
        self.wn_cols = np.asarray(cols, dtype=np.int32)
        if g.layers > 1:
            self.layer_stride = self.offsets["wavenet.conv_layers.1.conv.bias"] - self.offsets["wavenet.conv_layers.0.conv.bias"]
        else:
            self.layer_stride = 0

    def off(self, name: str) -> int:
        return self.offsets[name]

    def numel(self, name: str) -> int:
        return int(np.prod(self.shapes[name]))


def _traits(dtype: int):
    if dtype in (BF16, F16):
        return dict(EPL=8, CK=64, KBU=2, MT2=4, ES=2)
    return dict(EPL=4, CK=32, KBU=4, MT2=2, ES=4)


def u_row_index(dtype: int, kb: np.ndarray, h: np.ndarray, j: np.ndarray) -> np.ndarray:
    """k index (row of the previous accumulator tile stack) held by element j of lane-half h in k-block kb."""
    t = _traits(dtype)
    ut, s = kb // t["KBU"], kb % t["KBU"]
    if dtype in (BF16, F16):
        return 32 * ut + 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)
    return 32 * ut + 8 * s + 4 * h + j


def glu_pass_tiles(NP: int) -> int:
    """Gate-channel tiles per GEMM-1 pass (csrc/glu_fwd.hip dispatch_np must agree)."""
    if NP not in (1, 2, 3, 4, 6, 8):
        raise ValueError(f"gate_channels/2 padded to {32 * NP} is not supported by the fused layer kernel (Hp/32 must be 1,2,3,4,6,8)")
    return {1: 1, 2: 1, 3: 3, 4: 4, 6: 3, 8: 4}[NP]


def cond_weight_src(g: Geometry, lay: ParamLayout, row, cc):
    """arena offset (layer 0) of the 1x1 conditioning weight [gate row `row`][operand column `cc`], and its validity: columns
    [0, Cc) = conv1x1c; with g_local, [Cc, Cc + Cg) = conv1x1g (Geometry.g_local)."""
    Cc = max(g.Cc, 0)
    src = np.zeros(np.broadcast(row, cc).shape, dtype=np.int64)
    ok = np.zeros(src.shape, dtype=bool)
    if Cc > 0:
        c_off = lay.off("wavenet.conv_layers.0.conv1x1c.weight_v")
        isc = (cc >= 0) & (cc < Cc)
        src = np.where(isc, c_off + row * Cc + cc, src)
        ok |= isc
    if g.g_local:
        g_off = lay.off("wavenet.conv_layers.0.conv1x1g.weight_v")
        isg = (cc >= Cc) & (cc < Cc + g.Cg)
        src = np.where(isg, g_off + row * g.Cg + (cc - Cc), src)
        ok |= isg
    return src, ok


def glu_w1_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """int32 map (relative to arena start, layer 0) for the GEMM-1 stream of one GLU layer."""
    t = _traits(dtype)
    EPL, CK = t["EPL"], t["CK"]
    NPH = glu_pass_tiles(g.NP)
    NM = 2 * NPH
    cpr = g.Rp // CK
    nq_conv = g.k * cpr
    nq1 = nq_conv + g.Ccp // CK
    ps, q, blk, m, lane, j = np.meshgrid(np.arange(g.NP // NPH), np.arange(nq1), np.arange(4), np.arange(NM), np.arange(64),
                                         np.arange(EPL), indexing="ij")
    i, h = lane & 31, lane >> 5
    half = (m >= NPH).astype(np.int64)
    ig = 32 * (ps * NPH + m - half * NPH) + i
    row = half * g.H + ig
    is_conv = q < nq_conv
    tap = np.where(is_conv, q % g.k, 0)               # taps of one column block back to back (csrc/glu_fwd.hip: b_src)
    cblk = np.where(is_conv, q // g.k, q - nq_conv)
    ch = cblk * CK + blk * 2 * EPL + h * EPL + j
    conv_off = lay.off("wavenet.conv_layers.0.conv.weight_v")
    src_conv = conv_off + (row * g.R + ch) * g.k + tap
    valid_conv = (ig < g.H) & (ch < g.R)
    src_c, valid_c = cond_weight_src(g, lay, row, ch)
    valid_c = valid_c & (ig < g.H)
    out = np.where(is_conv, np.where(valid_conv, src_conv, -1), np.where(valid_c, src_c, -1))
    return out.astype(np.int32).reshape(-1)


def glu_w2_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """GEMM-2 stream of one layer: conv1x1_out rows only (the skip 1x1 is contracted in the head)."""
    t = _traits(dtype)
    EPL, KBU = t["EPL"], t["KBU"]
    NKB = g.NP * KBU
    n_mt = g.Rp // 32
    gm, kb, lane, j = np.meshgrid(np.arange(n_mt), np.arange(NKB), np.arange(64), np.arange(EPL), indexing="ij")
    i, h = lane & 31, lane >> 5
    ur = u_row_index(dtype, kb, h, j)
    r_out = 32 * gm + i
    src_out = lay.off("wavenet.conv_layers.0.conv1x1_out.weight_v") + r_out * g.H + ur
    out = np.where((r_out < g.R) & (ur < g.H), src_out, -1)
    return out.astype(np.int32).reshape(-1)


def glu_bias2_map(g: Geometry, lay: ParamLayout) -> np.ndarray:
    r = np.arange(g.Rp)
    o = lay.off("wavenet.conv_layers.0.conv1x1_out.bias")
    return np.where(r < g.R, o + r, -1).astype(np.int32)


def first_conv_maps(g: Geometry, lay: ParamLayout):
    """table (O or 1, Rp) with table[o][r] = W[r][o]; bias (Rp)."""
    nin = 1 if g.scalar_input else g.O
    o, r = np.meshgrid(np.arange(nin), np.arange(g.Rp), indexing="ij")
    tab = np.where(r < g.R, lay.off("wavenet.first_conv.weight_v") + r * nin + o, -1).astype(np.int32).reshape(-1)
    rr = np.arange(g.Rp)
    bias = np.where(rr < g.R, lay.off("wavenet.first_conv.bias") + rr, -1).astype(np.int32)
    return tab, bias


def head_w_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """[GEMM 0: all layers' conv1x1_skip, GEMM-1 order over K = (layer, u channel)] +
       [GEMM 1: last_conv_layers.1, GEMM-2 order] + [GEMM 2: last_conv_layers.3, GEMM-2 order]."""
    t = _traits(dtype)
    EPL, CK, KBU = t["EPL"], t["CK"], t["KBU"]
    NT = g.Sp // 32
    nq0 = g.Ku // CK
    q, blk, m, lane, j = np.meshgrid(np.arange(nq0), np.arange(4), np.arange(NT), np.arange(64), np.arange(EPL),
                                     indexing="ij")
    i, h = lane & 31, lane >> 5
    row = 32 * m + i
    kk = q * CK + blk * 2 * EPL + h * EPL + j
    layer, ch = kk // g.Hp, kk % g.Hp
    w0 = np.where((row < g.S) & (layer < g.layers) & (ch < g.H),
                  lay.off("wavenet.conv_layers.0.conv1x1_skip.weight_v") + layer * lay.layer_stride + row * g.H + ch, -1)
    NKB = NT * KBU

    def second_gemm(name, rows, rows_p):
        gm, kb, lane, j = np.meshgrid(np.arange(rows_p // 32), np.arange(NKB), np.arange(64), np.arange(EPL), indexing="ij")
        i, h = lane & 31, lane >> 5
        ur = u_row_index(dtype, kb, h, j)
        r = 32 * gm + i
        return np.where((r < rows) & (ur < g.S), lay.off(name) + r * g.S + ur, -1)

    w1 = second_gemm("wavenet.last_conv_layers.1.weight_v", g.S, g.Sp)
    w3 = second_gemm("wavenet.last_conv_layers.3.weight_v", g.O, g.Op)
    return np.concatenate([w0.reshape(-1), w1.reshape(-1), w3.reshape(-1)]).astype(np.int32)


def head_bias_map(g: Geometry, lay: ParamLayout) -> np.ndarray:
    """[b1 (Sp) | b3 (Op)] -- stored after the Sp-float skip-bias sum produced by wae_sum_rows."""
    r = np.arange(g.Sp + g.Op)
    b1 = lay.off("wavenet.last_conv_layers.1.bias")
    b3 = lay.off("wavenet.last_conv_layers.3.bias")
    return np.where(r < g.Sp, np.where(r < g.S, b1 + r, -1), np.where(r - g.Sp < g.O, b3 + r - g.Sp, -1)).astype(np.int32)


def glu_packed_elems(g: Geometry, dtype: int) -> int:
    t = _traits(dtype)
    nph = glu_pass_tiles(g.NP)
    chb = 2 * nph * 4 * 1024
    nq1 = g.k * (g.Rp // t["CK"]) + g.Ccp // t["CK"]
    mt2 = t["MT2"] * nph // g.NP
    nq2 = (g.Rp // 32) // mt2
    return ((g.NP // nph) * nq1 + nq2) * chb // t["ES"]


def head_packed_elems(g: Geometry, dtype: int) -> int:
    t = _traits(dtype)
    chb = (g.Sp // 32) * 4 * 1024
    mt2 = 4 // t["KBU"]
    return (g.Ku // t["CK"] + (g.Sp // 32) // mt2 + (g.Op // 32) // mt2) * chb // t["ES"]


# ---------------------------------------------------------------------------------------------------
# autoregressive kernel (csrc/ar_fwd.hip): matrix-vector layout [k/EPL][rows padded to 64][EPL]
# ---------------------------------------------------------------------------------------------------
def _ar_block(rows, rows_valid_fn, K, src_fn, EPL):
    """generic blocked map: element (kb, r, j) -> src_fn(r, kb*EPL + j) or -1"""
    rp = _ru(rows, 64)
    nkb = (K + EPL - 1) // EPL
    kb, r, j = np.meshgrid(np.arange(nkb), np.arange(rp), np.arange(EPL), indexing="ij")
    kk = kb * EPL + j
    ok = (r < rows) & (kk < K)
    return np.where(ok, src_fn(np.minimum(r, rows - 1), np.minimum(kk, K - 1)), -1).reshape(-1), nkb * rp * EPL


def ar_layer_map(g: Geometry, lay: ParamLayout, dtype: int):
    """-> (map of one layer [W1 | W2], element offset of W2).  W1: G x (k*R + Cc) with k ordered
    [tap 0 .. tap k-1 | c] (tap j multiplies x[t-(k-1-j)d], conv.py:51-62); W2: [conv1x1_out (R) ; conv1x1_skip (S)] x H."""
    EPL = _traits(dtype)["EPL"]
    Cc = max(g.Cc, 0)
    K1 = g.k * g.R + Cc
    conv = lay.off("wavenet.conv_layers.0.conv.weight_v")
    cw = lay.off("wavenet.conv_layers.0.conv1x1c.weight_v") if Cc else 0

    def src1(r, kk):
        tap, ch = kk // g.R, kk % g.R
        return np.where(kk < g.k * g.R, conv + (r * g.R + ch) * g.k + np.minimum(tap, g.k - 1),
                        cw + r * max(Cc, 1) + (kk - g.k * g.R))

    m1, n1 = _ar_block(g.G, None, K1, src1, EPL)
    out = lay.off("wavenet.conv_layers.0.conv1x1_out.weight_v")
    skp = lay.off("wavenet.conv_layers.0.conv1x1_skip.weight_v")

    def src2(r, kk):
        return np.where(r < g.R, out + r * g.H + kk, skp + (r - g.R) * g.H + kk)

    m2, n2 = _ar_block(g.R + g.S, None, g.H, src2, EPL)
    return np.concatenate([m1, m2]).astype(np.int32), n1


def ar_bias2_map(g: Geometry, lay: ParamLayout) -> np.ndarray:
    r = np.arange(g.R + g.S)
    return np.where(r < g.R, lay.off("wavenet.conv_layers.0.conv1x1_out.bias") + r,
                    lay.off("wavenet.conv_layers.0.conv1x1_skip.bias") + r - g.R).astype(np.int32)


def ar_head_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    EPL = _traits(dtype)["EPL"]
    w1 = lay.off("wavenet.last_conv_layers.1.weight_v")
    w3 = lay.off("wavenet.last_conv_layers.3.weight_v")
    m1, _ = _ar_block(g.S, None, g.S, lambda r, kk: w1 + r * g.S + kk, EPL)
    m3, _ = _ar_block(g.O, None, g.S, lambda r, kk: w3 + r * g.S + kk, EPL)
    return np.concatenate([m1, m3]).astype(np.int32)


def ar_head_bias_map(g: Geometry, lay: ParamLayout) -> np.ndarray:
    r = np.arange(g.S + g.O)
    return np.where(r < g.S, lay.off("wavenet.last_conv_layers.1.bias") + r,
                    lay.off("wavenet.last_conv_layers.3.bias") + r - g.S).astype(np.int32)


def ar_ring_offsets(g: Geometry) -> np.ndarray:
    """float offsets of each layer's history ring ((k-1)*d+1 rows of R) inside one utterance's arena; last = total"""
    off = [0]
    for d in g.dilations:
        off.append(off[-1] + ((g.k - 1) * d + 1) * g.R)
    return np.asarray(off, dtype=np.int64)


class ArListPlan(NamedTuple):
    """ar_list_plan's answer.  order: item indices in launch order; offsets[i]: first step of the caller's item i in the packed
    per-step operands (caller's order, contiguous); total: their sum of lengths; slots: workgroups to launch; makespan: steps of the
    busiest slot when every free slot takes the next item of `order` (what the kernel's queue does, all steps costing the same)."""
    order: np.ndarray
    offsets: np.ndarray
    total: int
    slots: int
    makespan: int

    @property
    def efficiency(self) -> float:
        """share of slots x makespan that decodes: sum T_i / (slots x longest slot load)"""
        return self.total / float(self.slots * self.makespan)


def ar_list_plan(lengths, slots: int) -> ArListPlan:
    """Launch plan of a list decode (include/wae.h: wae_ar_generate_list) for utterances of `lengths` steps on `slots` workgroups.
    Longest first, so that the tail of the launch -- slots idling while the last items finish -- is short; equal lengths keep the
    caller's order (a stable sort), so the plan is a function of the lengths alone.  slots is clamped to the item count."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size < 1:
        raise ValueError("ar_list_plan: an empty list")
    if int(n.min()) < 1:
        raise ValueError(f"ar_list_plan: every item has at least one step (got {int(n.min())})")
    if int(slots) < 1:
        raise ValueError(f"ar_list_plan: slots {int(slots)} < 1")
    slots = min(int(slots), int(n.size))
    order = np.argsort(-n, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)
    free = [0] * slots                      # a heap of the times at which the slots come back to the queue
    for i in order:
        heapq.heappush(free, heapq.heappop(free) + int(n[i]))
    return ArListPlan(order, offsets, int(n.sum()), slots, max(free))


class ArRoundPlan(NamedTuple):
    """ar_round_plan's answer: one span per clip that decodes in this round.  clips: the indices (into the planner's arguments) of those
    clips, in the caller's order; lengths / t0: steps and absolute first step of each clip's span; offsets: first step of each span in
    the round's packed per-step operands (contiguous, in `clips` order); order: positions in `clips` in launch order; total: the sum
    of the lengths (the length of the packed operands); slots: workgroups or teams to launch."""
    clips: np.ndarray
    lengths: np.ndarray
    t0: np.ndarray
    offsets: np.ndarray
    order: np.ndarray
    total: int
    slots: int


def ar_round_plan(remaining, positions, chunk, slots: int) -> ArRoundPlan:
    """One round of a decode session (include/wae.h: wae_ar_generate_spans): which clips get a span, how long, and in what order.
    remaining[i] / positions[i]: steps clip i still has to decode and the absolute index of its next step.  chunk: steps per clip and
    round -- an int for every clip, or a mapping from clip index to steps (a clip the mapping leaves out, or gives < 1, sits the round
    out).  A clip gets min(chunk, remaining) steps; a finished clip (remaining < 1) gets no span and is absent from the plan.  The
    launch order is longest span first, equal lengths in the caller's order (a stable sort, as ar_list_plan); slots is clamped to the
    number of spans (at least 1)."""
    rem = np.asarray(remaining, dtype=np.int64).reshape(-1)
    pos = np.asarray(positions, dtype=np.int64).reshape(-1)
    if rem.size != pos.size:
        raise ValueError(f"ar_round_plan: {rem.size} remaining lengths for {pos.size} positions")
    if int(slots) < 1:
        raise ValueError(f"ar_round_plan: slots {int(slots)} < 1")
    if pos.size and int(pos.min()) < 0:
        raise ValueError("ar_round_plan: a negative position")
    if isinstance(chunk, (int, np.integer)):
        if int(chunk) < 1:
            raise ValueError(f"ar_round_plan: chunk {int(chunk)} < 1")
        want = np.full(rem.size, int(chunk), dtype=np.int64)
    else:
        want = np.zeros(rem.size, dtype=np.int64)
        for i, n in dict(chunk).items():
            if not 0 <= int(i) < rem.size:
                raise ValueError(f"ar_round_plan: chunk names clip {int(i)} of {rem.size}")
            want[int(i)] = max(int(n), 0)
    n = np.minimum(want, np.maximum(rem, 0))
    clips = np.nonzero(n > 0)[0].astype(np.int64)
    n = n[clips]
    order = np.argsort(-n, kind="stable").astype(np.int64)
    offsets = (np.concatenate([[0], np.cumsum(n)[:-1]]) if n.size else np.zeros(0)).astype(np.int64)
    return ArRoundPlan(clips, n, pos[clips], offsets, order, int(n.sum()), max(1, min(int(slots), int(n.size))))


# ---------------------------------------------------------------------------------------------------
# backward: where the weight-gradient launches go (backward.py builds the tables; the rules are here,
# plain Python, so that they run without a device)
# ---------------------------------------------------------------------------------------------------
class TnShares(NamedTuple):
    """tn_team_shares' answer.  segs: (first job of the group, first slab, end slab) in team order; team t owns
    segs[team_seg[t]:team_seg[t + 1]]."""
    nteams: int
    nwg: int
    segs: List[Tuple[int, int, int]]
    team_seg: List[int]


def tn_team_shares(n_groups: int, B: int, T: int, team_size: int, ncu: int, swap: bool = False) -> TnShares:
    """The (group, 32-row time slab) list of a team launch (csrc/gemm_tn_stream.hip, csrc/gemm_tn_static.hip) cut into equal
    contiguous shares, one per team of team_size workgroups; ncu: the CUs the launch may count on.  Every member of a team sweeps
    the same slab range; shares are cut on the raw slab count (the slabs a member skips differ by tap).  swap: the second half of
    every team's share points at a second copy of the groups that follows the first (backward.StaticStreamTable: the copy in which
    the conditioning and the out + skip member have changed places)."""
    KT = 32
    per = B * ((T + KT - 1) // KT)            # slabs of one group
    nteams = max(1, ncu // team_size)
    nwg = ncu if ncu % 8 == 0 and ncu >= nteams * team_size else nteams * team_size
    total = n_groups * per
    segs, team_seg = [], [0]
    for t in range(nteams):
        lo, hi = total * t // nteams, total * (t + 1) // nteams
        mid = (lo + hi) // 2 if swap else hi
        for a, b, var in ((lo, mid, 0), (mid, hi, 1)):
            while a < b:
                grp = a // per
                end = min(b, (grp + 1) * per)
                segs.append(((var * n_groups + grp) * team_size, a - grp * per, end - grp * per))
                a = end
        team_seg.append(len(segs))
    return TnShares(nteams, nwg, segs, team_seg)


def tn_beside_split(layers: int, B: int, T: int, ncu: int) -> Optional[Tuple[int, int]]:
    """An under-filled backward sweep (B * ceil(T / 256) workgroups per launch on ncu CUs): None, or (first upper layer, idle CUs) --
    the weight gradients of layers [first, L) run beside the lower part of the sweep on the idle CUs.  What the side launch has not
    finished when the sweep ends runs beside the lower layers' launch, so the cut is not critical: L / (1 + ncu / (2 idle)) upper
    layers (measured: backward.py, _tn_schedule)."""
    idle = (ncu - B * ((T + 255) // 256)) // 8 * 8
    if idle < 64 or layers < 8:
        return None
    nup = int(layers / (1.0 + 0.5 * ncu / idle))
    return (layers - nup, idle) if nup >= 2 else None


def tn_job_groups(njobs: int) -> Tuple[int, int]:
    """(groups, jobs per group) of a layer's static weight-gradient jobs: one group (a team of that many workgroups walks the layer's
    slabs) up to six jobs; more are dealt into equal groups of at most six, the last padded with null jobs."""
    ngrp = -(-njobs // 6) if njobs > 6 else 1
    return ngrp, -(-njobs // ngrp)


def tn_layer_contractions(g: Geometry, d: int, alpha: float, dz: int, dz_stride: int, x: int, c_up: int, g_next: Optional[int],
                          u: int, c1: int, ld1: int, co: int, ldo: int):
    """The weight-gradient contractions C[M][N (+ ones)] += alpha * P^T Q of one gated layer of dilation d, as records
    (M, N, shift, ones_col, alpha, P, p_stride, Q, q_stride, C, ldc) -- the arguments of backward.TileTable.add / StreamTable.add:
    one per dilated-conv tap (dz against the convolution's operand x), the conditioning 1x1 with the zb sums in its ones columns (the
    last tap's without conditioning), conv1x1_out + bias (g_next = dx-hat of the layer above against u; None: no such contraction,
    0: a placeholder job).  Operands are device addresses; c1 / co: the layer's dense fp32 gradient tiles."""
    Z2 = 2 * g.Hp
    for tap in range(g.k):
        last = tap == g.k - 1 and not g.Ccp
        yield (Z2, g.Rp, -(g.k - 1 - tap) * d, (g.Rp if last else -1), alpha, dz, dz_stride, x, g.Rp, c1 + tap * g.Rp * 4, ld1)
    if g.Ccp:
        yield (Z2, g.Ccp, 0, g.Ccp, alpha, dz, dz_stride, c_up, g.Ccp, c1 + g.k * g.Rp * 4, ld1)
    if g_next is not None:
        yield (g.Rp, g.Hp, 0, g.Hp, alpha, g_next, g.Rp, u, g.Ku, co, ldo)


# ---------------------------------------------------------------------------------------------------
# backward: transposed weight streams (csrc/gemm_tm.hip, csrc/head_bwd.hip) and the scatter maps that
# bring the dense weight-gradient tiles of csrc/gemm_tn.hip back into the flat gradient arena
# ---------------------------------------------------------------------------------------------------
def tm_slicing(Mp: int) -> Tuple[int, int]:
    """(tiles per slice, slices) of an Mp-row output of wae_gemm_tm (csrc/gemm_tm.hip: tm_slicing must agree)."""
    nt = Mp // 32
    if nt in (1, 2, 3, 4, 6, 8):
        return nt, 1
    for c in (8, 6, 4):
        if nt % c == 0:
            return c, nt // c
    raise ValueError(f"wae_gemm_tm: unsupported output width {Mp}")


def first_gemm_map(Mp: int, Kp: int, dtype: int, src_fn) -> np.ndarray:
    """[slice][q][blk][m][lane][j] stream of an (Mp x Kp) matrix; src_fn(row, kk) -> arena offset or -1 (vectorised).
    Outputs wider than 256 rows are cut into slices of tm_slicing(Mp) tiles, each with its own chunk stream."""
    t = _traits(dtype)
    EPL, CK = t["EPL"], t["CK"]
    assert Mp % 32 == 0 and Kp % CK == 0, (Mp, Kp)
    nts, nsl = tm_slicing(Mp)
    sl, q, blk, m, lane, j = np.meshgrid(np.arange(nsl), np.arange(Kp // CK), np.arange(4), np.arange(nts), np.arange(64),
                                         np.arange(EPL), indexing="ij")
    row = 32 * (sl * nts + m) + (lane & 31)
    kk = q * CK + blk * 2 * EPL + (lane >> 5) * EPL + j
    return src_fn(row, kk).astype(np.int32).reshape(-1)


def second_gemm_map(Mp: int, Kp: int, dtype: int, src_fn) -> np.ndarray:
    """[gm][kb][lane][j] stream; k index follows the accumulator-tile row order (u_row_index)."""
    t = _traits(dtype)
    EPL, KBU = t["EPL"], t["KBU"]
    assert Mp % 32 == 0 and Kp % 32 == 0
    gm, kb, lane, j = np.meshgrid(np.arange(Mp // 32), np.arange(Kp // 32 * KBU), np.arange(64), np.arange(EPL), indexing="ij")
    row = 32 * gm + (lane & 31)
    kk = u_row_index(dtype, kb, lane >> 5, j)
    return src_fn(row, kk).astype(np.int32).reshape(-1)


def _gate_row(g: Geometry, c2):
    """padded gate column (0..2Hp) -> (reference row of the (G, ...) conv weight, valid)"""
    half = (c2 >= g.Hp).astype(np.int64)
    i = c2 - half * g.Hp
    return half * g.H + i, i < g.H


def bwd_u_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """du = W_out^T dx-hat + W_skip^T dskip: rows h (Hp), K = [Rp | Sp]."""
    o = lay.off("wavenet.conv_layers.0.conv1x1_out.weight_v")
    s = lay.off("wavenet.conv_layers.0.conv1x1_skip.weight_v")

    def src(h, kk):
        r, sk = kk, kk - g.Rp
        return np.where(kk < g.Rp, np.where((r < g.R) & (h < g.H), o + r * g.H + h, -1),
                        np.where((sk < g.S) & (h < g.H), s + sk * g.H + h, -1))
    return first_gemm_map(g.Hp, g.Rp + g.Sp, dtype, src)


def bwd_uo_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """W_out^T for the fused boundary kernel (csrc/glu_bwd.hip): rows h (Hp), K = Rp in accumulator-row order (the
    operand is the just-computed dx-hat tile stack)."""
    o = lay.off("wavenet.conv_layers.0.conv1x1_out.weight_v")
    return second_gemm_map(g.Hp, g.Rp, dtype, lambda h, r: np.where((r < g.R) & (h < g.H), o + r * g.H + h, -1))


TM_INTERLEAVE = 1    # include/wae.h: WAE_TM_INTERLEAVE


def bwd_x_map(g: Geometry, lay: ParamLayout, dtype: int, interleave: bool = True) -> np.ndarray:
    """dx = sum_tap W1_tap^T dz[t + (k-1-tap) d]: rows r (Rp), K = k sources of 2Hp gate columns, visited round-robin per
    128-byte column block (WAE_TM_INTERLEAVE): chunk q = cblk * k + tap; interleave=False: tap by tap (csrc/glu_bwd.hip)."""
    conv = lay.off("wavenet.conv_layers.0.conv.weight_v")
    CK = _traits(dtype)["CK"]

    def src(r, kk):
        q, within = kk // CK, kk % CK
        if interleave:
            tap, c2 = q % g.k, (q // g.k) * CK + within
        else:
            tap, c2 = kk // (2 * g.Hp), kk % (2 * g.Hp)
        row, ok = _gate_row(g, c2)
        return np.where(ok & (r < g.R), conv + (row * g.R + r) * g.k + tap, -1)
    return first_gemm_map(g.Rp, g.k * 2 * g.Hp, dtype, src)


def bwd_c_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    """dc = sum_l Wc_l^T dz_l: rows cc (Ccp), K = L * 2Hp (absolute offsets).  (g_local: rows [Cc, Cc + Cg) are conv1x1g's.)"""
    def src(cc, kk):
        l, c2 = kk // (2 * g.Hp), kk % (2 * g.Hp)
        row, ok = _gate_row(g, c2)
        off, okc = cond_weight_src(g, lay, row, cc)
        return np.where(ok & okc, off + l * lay.layer_stride, -1)
    return first_gemm_map(g.Ccp, g.layers * 2 * g.Hp, dtype, src)


def head_bwd_map(g: Geometry, lay: ParamLayout, dtype: int) -> np.ndarray:
    w3 = lay.off("wavenet.last_conv_layers.3.weight_v")
    w1 = lay.off("wavenet.last_conv_layers.1.weight_v")
    a = first_gemm_map(g.Op, g.Sp, dtype, lambda o, kk: np.where((o < g.O) & (kk < g.S), w3 + o * g.S + kk, -1))
    b = second_gemm_map(g.Sp, g.Op, dtype, lambda s, kk: np.where((s < g.S) & (kk < g.O), w3 + kk * g.S + s, -1))
    c = second_gemm_map(g.Sp, g.Sp, dtype, lambda s, kk: np.where((s < g.S) & (kk < g.S), w1 + kk * g.S + s, -1))
    return np.concatenate([a, b, c]).astype(np.int32)


def head_wide_maps(g: Geometry, lay: ParamLayout, dtype: int) -> Dict[str, np.ndarray]:
    """Weight streams of the wide head (Sp > 256; wae_gemm_tm modes 3-6), all in first-GEMM order:
    skip = all layers' conv1x1_skip over K = Ku (layer, gated channel); w1 / w3 = last_conv_layers.1 / .3;
    w3t / w1t = their transposes for the backward data path."""
    ws = lay.off("wavenet.conv_layers.0.conv1x1_skip.weight_v")
    w1 = lay.off("wavenet.last_conv_layers.1.weight_v")
    w3 = lay.off("wavenet.last_conv_layers.3.weight_v")

    def skip_src(row, kk):
        layer, ch = kk // g.Hp, kk % g.Hp
        return np.where((row < g.S) & (layer < g.layers) & (ch < g.H), ws + layer * lay.layer_stride + row * g.H + ch, -1)
    return dict(
        skip=first_gemm_map(g.Sp, g.Ku, dtype, skip_src),
        w1=first_gemm_map(g.Sp, g.Sp, dtype, lambda r, kk: np.where((r < g.S) & (kk < g.S), w1 + r * g.S + kk, -1)),
        w3=first_gemm_map(g.Op, g.Sp, dtype, lambda o, kk: np.where((o < g.O) & (kk < g.S), w3 + o * g.S + kk, -1)),
        w3t=first_gemm_map(g.Sp, g.Op, dtype, lambda s_, kk: np.where((s_ < g.S) & (kk < g.O), w3 + kk * g.S + s_, -1)),
        w1t=first_gemm_map(g.Sp, g.Sp, dtype, lambda s_, kk: np.where((s_ < g.S) & (kk < g.S), w1 + kk * g.S + s_, -1)),
    )


def head_is_wide(g: Geometry) -> bool:
    """The register-chained head kernels hold Sp/32 <= 8 accumulator tiles per wave; wider heads (or EngineOptions.head_wide, for
    tests) run as separate wae_gemm_tm launches."""
    return g.Sp > 256


ONES_PAD = 128   # spare C columns that receive the per-clip "ones column" sums (B <= 128)


def grad_scatter_maps(g: Geometry, lay: ParamLayout) -> dict:
    """C-buffer element -> gradient-arena offset (or -1).  Layer maps are relative to layer 0.  ``*_w`` maps cover the
    weight sub-tile (rows x cols, every slot written once: plain adds); ``*_b`` maps cover the ONES_PAD ones-columns
    (rows x ONES_PAD, every clip column adds into the same bias slot: atomics)."""
    out = {}
    ones = np.zeros((1, ONES_PAD), dtype=np.int64)
    # dW1 | dWc : rows = padded gate rows (2Hp), cols = [tap*Rp + r | k*Rp + cc]  (the ones columns feed gproj_bwd)
    ld1 = g.k * g.Rp + g.Ccp + ONES_PAD
    ncol1 = g.k * g.Rp + g.Ccp
    row, col = np.meshgrid(np.arange(2 * g.Hp), np.arange(ncol1), indexing="ij")
    grow, ok = _gate_row(g, row)
    conv = lay.off("wavenet.conv_layers.0.conv.weight_v")
    tap, r = col // g.Rp, col % g.Rp
    m = np.where(ok & (col < g.k * g.Rp) & (r < g.R), conv + (grow * g.R + r) * g.k + np.minimum(tap, g.k - 1), -1)
    if g.Ccp:
        cc = col - g.k * g.Rp
        off, okc = cond_weight_src(g, lay, grow, cc)
        m = np.where(ok & okc, off, m)
    out["w1"], out["ld1"], out["ncol1"] = m.astype(np.int32).reshape(-1), ld1, ncol1
    # dW_out: rows r (Rp), cols h (Hp) ; ones -> bias
    ldo = g.Hp + ONES_PAD
    row, col = np.meshgrid(np.arange(g.Rp), np.arange(g.Hp), indexing="ij")
    wo = lay.off("wavenet.conv_layers.0.conv1x1_out.weight_v")
    bo = lay.off("wavenet.conv_layers.0.conv1x1_out.bias")
    out["wo"], out["ldo"] = np.where((row < g.R) & (col < g.H), wo + row * g.H + col, -1).astype(np.int32).reshape(-1), ldo
    rowb = np.arange(g.Rp)[:, None] + ones
    out["bo"] = np.where(rowb < g.R, bo + rowb, -1).astype(np.int32).reshape(-1)
    # dW_skip of all layers: rows s (Sp), cols l*Hp + h ; ones -> skip bias (applied per layer separately)
    lds = g.Ku + ONES_PAD
    row, col = np.meshgrid(np.arange(g.Sp), np.arange(g.Ku), indexing="ij")
    ws = lay.off("wavenet.conv_layers.0.conv1x1_skip.weight_v")
    l, hh = col // g.Hp, col % g.Hp
    m = np.where((row < g.S) & (col < g.layers * g.Hp) & (hh < g.H), ws + l * lay.layer_stride + row * g.H + hh, -1)
    out["ws"], out["lds"] = m.astype(np.int32).reshape(-1), lds
    bs = lay.off("wavenet.conv_layers.0.conv1x1_skip.bias")
    rowb = np.arange(g.Sp)[:, None] + ones
    out["bs"] = np.where(rowb < g.S, bs + rowb, -1).astype(np.int32).reshape(-1)   # (Sp, ONES_PAD) ones columns, layer 0
    # The static weight-gradient launch (csrc/gemm_tn_static.hip, kind OUTSKIP) writes dW_out and dW_skip of a layer TRANSPOSED --
    # rows = gated channel h (Hp of them), columns = residual / skip channel -- and the out bias as ONE row behind the Hp rows.
    hrow, rcol = np.meshgrid(np.arange(g.Hp), np.arange(g.Rp), indexing="ij")
    out["woT"] = np.where((rcol < g.R) & (hrow < g.H), wo + rcol * g.H + hrow, -1).astype(np.int32).reshape(-1)
    rr = np.arange(g.Rp)
    out["boT"] = np.where(rr < g.R, bo + rr, -1).astype(np.int32)
    out["ldoT_rows"] = g.Hp + 8               # rows of a layer's block: Hp weight rows, the bias row, padding
    hrow, scol = np.meshgrid(np.arange(g.Hp), np.arange(g.Sp), indexing="ij")
    out["wsT"] = np.where((scol < g.S) & (hrow < g.H), ws + scol * g.H + hrow, -1).astype(np.int32).reshape(-1)   # layer 0
    ss_ = np.arange(g.Sp)
    out["bsT"] = np.where(ss_ < g.S, bs + ss_, -1).astype(np.int32)          # skip bias from a plain (Sp,) vector of sums, layer 0
    # head
    ldh = g.Sp + ONES_PAD
    row, col = np.meshgrid(np.arange(g.Op), np.arange(g.Sp), indexing="ij")
    w3, b3 = lay.off("wavenet.last_conv_layers.3.weight_v"), lay.off("wavenet.last_conv_layers.3.bias")
    out["w3"] = np.where((row < g.O) & (col < g.S), w3 + row * g.S + col, -1).astype(np.int32).reshape(-1)
    rowb = np.arange(g.Op)[:, None] + ones
    out["b3"] = np.where(rowb < g.O, b3 + rowb, -1).astype(np.int32).reshape(-1)
    row, col = np.meshgrid(np.arange(g.Sp), np.arange(g.Sp), indexing="ij")
    w1, b1 = lay.off("wavenet.last_conv_layers.1.weight_v"), lay.off("wavenet.last_conv_layers.1.bias")
    out["w1h"] = np.where((row < g.S) & (col < g.S), w1 + row * g.S + col, -1).astype(np.int32).reshape(-1)
    rowb = np.arange(g.Sp)[:, None] + ones
    out["b1h"] = np.where(rowb < g.S, b1 + rowb, -1).astype(np.int32).reshape(-1)
    out["ldh"] = ldh
    # first conv table gradient (O or 1, Rp) -> weight_v (R, O, 1)
    nin = 1 if g.scalar_input else g.O
    o, r = np.meshgrid(np.arange(nin), np.arange(g.Rp), indexing="ij")
    out["tab"] = np.where(r < g.R, lay.off("wavenet.first_conv.weight_v") + r * nin + o, -1).astype(np.int32).reshape(-1)
    rr = np.arange(g.Rp)
    out["fb"] = np.where(rr < g.R, lay.off("wavenet.first_conv.bias") + rr, -1).astype(np.int32)
    return out
