"""The two records of a training step's hand-overs on the host: `Saved` (what a train-mode forward leaves for its backward) and
`InFlight` (what the phases of one step hand to each other).  WaeEngine owns one of each: engine.saved, engine.flight."""
from __future__ import annotations

import dataclasses
import itertools

from typing import Optional

import torch


@dataclasses.dataclass
class ListFrontEnd:
    """What the LIST front end of a ragged step's forward (frontend.train_list_front) leaves for backward.frontend_backward_list, in
    place of Saved.up_acts / enc_acts; Saved.lat / quant / idx are then the packed (1, Cc, sum Tq_i) arrays."""
    plan: object                                # packing.TrainListPlan
    tables: tuple                               # the device tables (enc | None, ups, bwd)
    enc_acts: Optional[list] = None             # the packed input of every encoder layer (the blocks, then lin)
    up_acts: Optional[list] = None              # [conv_in's packed input | None, every stage's packed input]


@dataclasses.dataclass
class HeadDone:
    """The head's backward as the fused forward launch ran it: the factor on d loss / d logits, and the targets and lengths it masked
    with.  backward.decoder_backward skips wae_head_bwd only for the same three."""
    factor: float
    targets: object                             # the caller's targets and lengths objects themselves (lengths None: every step counts)
    lengths: object

    def serves(self, factor, targets, lengths) -> bool:
        return self.factor == factor and self.targets is targets and self.lengths is lengths


@dataclasses.dataclass
class Saved:
    """What ONE train-mode forward leaves for its backward beside the activations in the engine's (B, T, True) workspace.  Only a
    train-mode decoder_forward / forward -- and the stand-alone layer's train-mode run -- replaces WaeEngine.saved, each with a new
    `gen` (made here and nowhere else); an eval forward or a decode leaves it alone.  The autograd wrappers remember `gen` and refuse a backward
    through an older forward (wavenet_vocoder/_base.py: check_saved)."""
    B: int
    T: int
    gen: int = dataclasses.field(default_factory=itertools.count(1).__next__)
    drop_seeds: Optional[list] = None           # one mask seed per layer, where the forward applied dropout
    up_acts: Optional[list] = None              # upsampling network: [conv_in input | None, stage-0 input, stage-1 input, ...]
    up_last: Optional[torch.Tensor] = None      # ... the last stage's activated output: backward forms act' from it
    up_keep: Optional[torch.Tensor] = None      # ... the trimmed copy its last launch read
    enc_acts: Optional[list] = None             # encoder: the input of every block, then the last block's output
    lat: Optional[torch.Tensor] = None          # the VQ record (None: no encoder ran in front of the decoder)
    quant: Optional[torch.Tensor] = None
    idx: Optional[torch.Tensor] = None
    beta: float = 0.25
    list_fe: Optional[ListFrontEnd] = None      # the LIST front end of a ragged step (WaeEngine.train_step_list); None: a dense forward
    head_done: Optional["HeadDone"] = None      # the forward's head launch already wrote dy, dh1 and dskip (csrc/head_train.hip)


@dataclasses.dataclass
class Window:
    """An open accumulation window (WaeEngine.accumulate .. apply_step): micro-batches whose weight gradients add up in the engine's
    accumulators (backward.py: deferred finishing) until ONE finish and ONE optimizer step close it."""
    sums: torch.Tensor                          # (3,) fp64 on the device: sum w ce, sum w vq_loss, micro-batches (wae_accum_stats)
    counts: Optional[torch.Tensor]              # (K,) int32: the code histograms added per code; None without an encoder
    drop_calls: int                             # the engine's dropout counter when the window opened (discard_step puts it back)
    n: int = 0                                  # micro-batches accumulated
    static: Optional[bool] = None               # which weight-gradient launch fills the tiles (backward.static_tn_shape): one per window
    shape: Optional[tuple] = None               # (B, T) of the last micro-batch: its workspace's tables serve the finish


class InFlight:
    """What the phases of one step hand to each other.  pack_done / early_pack: the completion events (WaeEngine.branch boxes) of the
    forward's / the backward's weight packing on a side stream, each taken once by the phase that waits for it; ev_dc: recorded where
    the conditioning gradient is complete; grads_done: the arena slice decoder_backward finished itself; finish_used: the FinishPlan
    that did; norm_summed: the gather passes summed the squared norm.
    head_factor: the factor on d loss / d logits that the step's backward will use, announced by train.step_run before the forward and
    taken by the forward's head (engine._head_fwd: the fused training head); onehot_early: (ids address, B, T) of the one-hot rows that
    step_open already wrote on the packing's side stream.
    accum: the Window this backward adds a micro-batch to -- the accumulate-mode switch of decoder_backward (deferred finishing:
    no clearing from the second micro-batch on, nothing scattered, nothing written to the gradient arena); None: a plain step."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.pack_done = self.early_pack = self.ev_dc = None
        self.grads_done = self.finish_used = None
        self.norm_summed = False
        self.accum = None
        self.head_factor = self.onehot_early = None

    def abandon(self):
        """A refused input ended the step half-way: nothing of it may be taken for the next call's.  -> the event of the forward's
        weight packing, which may still run on its side stream: the caller's stream waits for it, as the forward would have."""
        ev = self.take_pack_done()
        self.reset()
        return ev

    def take_pack_done(self):
        box, self.pack_done = self.pack_done, None
        return box[0] if box else None

    def take_head_factor(self):
        f, self.head_factor = self.head_factor, None
        return f

    def take_early_pack(self):
        box, self.early_pack = self.early_pack, None
        return box[0] if box else None


def saved_for(eng, B, T) -> Saved:
    """eng.saved, the record of the train-mode forward that a backward of shape (B, T) differentiates -- or, before any launch, the
    RuntimeError that names what is missing"""
    sv = eng.saved
    if sv is None:
        raise RuntimeError("no train-mode forward to differentiate: run decoder_forward / forward with train=True (or train_step) first")
    if (sv.B, sv.T) != (B, T):
        raise RuntimeError(f"backward of shape (B, T) = ({B}, {T}), but the last train-mode forward ran ({sv.B}, {sv.T})")
    return sv
