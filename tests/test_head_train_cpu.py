"""Host side of the one-launch training head (csrc/head_train.hip; EngineOptions.head_fused) without a GPU: the ONE expression of the
factor on d loss / d logits that train.step_run announces and decoder_backward compares, the record the forward leaves, the switch,
and the built kernel's register file (no scratch, counted waits in front of every weight chunk)."""
import os
import re
import types

import pytest
import torch

from wavenet_autoencoders_amd import backward as BW
from wavenet_autoencoders_amd.options import EngineOptions
from wavenet_autoencoders_amd.step_state import HeadDone, InFlight, Saved


def _eng(grad_scale):
    return types.SimpleNamespace(grad_scale=grad_scale)


def _before(eng, B, T, lengths, loss_scale, dy_factor):
    """decoder_backward's expression before the helper existed"""
    if lengths is None:
        count = B * (T - 1)
    else:
        count = int(torch.clamp(lengths.detach().to("cpu", torch.int64).clamp(max=T) - 1, min=0).sum())
    return loss_scale * eng.grad_scale / max(count, 1) if dy_factor is None else dy_factor


@pytest.mark.parametrize("grad_scale", [1.0, 4096.0])
@pytest.mark.parametrize("lengths", [None, [300, 0], [1, 293], [150, 300], [400, 2], [0, 0]])
@pytest.mark.parametrize("loss_scale,dy_factor", [(1.0, None), (0.37, None), (1.0, 4096.0 / 577), (0.5, 0.0)])
def test_factor_helper_is_decoder_backwards_expression(grad_scale, lengths, loss_scale, dy_factor):
    B, T = 2, 300
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    eng = _eng(grad_scale)
    assert BW.head_dy_factor(eng, B, T, ln, loss_scale, dy_factor) == _before(eng, B, T, ln, loss_scale, dy_factor)


def test_factor_helper_counts():
    eng = _eng(1.0)
    assert BW.head_dy_factor(eng, 2, 300, None) == 1.0 / 598
    assert BW.head_dy_factor(eng, 2, 300, torch.tensor([300, 0])) == 1.0 / 299
    assert BW.head_dy_factor(eng, 2, 300, torch.tensor([1, 293])) == 1.0 / 292
    assert BW.head_dy_factor(eng, 2, 300, torch.tensor([400, 2])) == 1.0 / 300          # clamped to T
    assert BW.head_dy_factor(eng, 2, 300, torch.tensor([0, 1])) == 1.0                   # no step counts: max(count, 1)
    assert BW.head_dy_factor(eng, 2, 300, torch.tensor([7, 7]), 3.0, 0.125) == 0.125


def test_record_serves_only_the_same_factor_targets_and_lengths():
    x, ln = torch.zeros(2, 8, dtype=torch.int32), torch.tensor([8, 5])
    rec = HeadDone(0.25, x, ln)
    assert rec.serves(0.25, x, ln)
    assert not rec.serves(0.5, x, ln)
    assert not rec.serves(0.25, x.clone(), ln)
    assert not rec.serves(0.25, x, ln.clone())
    assert not rec.serves(0.25, x, None)
    assert HeadDone(0.25, x, None).serves(0.25, x, None)
    assert Saved(2, 8).head_done is None


def test_flight_record_hands_the_factor_over_once():
    fl = InFlight()
    assert fl.take_head_factor() is None
    fl.head_factor = 0.125
    assert fl.take_head_factor() == 0.125
    assert fl.take_head_factor() is None
    fl.head_factor, fl.onehot_early = 1.0, (1, 2, 3)
    fl.reset()
    assert fl.head_factor is None and fl.onehot_early is None


def test_switch(monkeypatch):
    assert EngineOptions().head_fused is True
    monkeypatch.delenv("WAE_HEAD_FUSED", raising=False)
    assert EngineOptions.from_env().head_fused is True
    monkeypatch.setenv("WAE_HEAD_FUSED", "0")
    assert EngineOptions.from_env().head_fused is False


def test_built_kernel_has_no_scratch_and_counted_waits():
    """csrc/obj/head_train.s (a by-product of the build): every instantiation fits two waves per SIMD (256 registers) without scratch,
    and in front of every weight chunk stands a hand-written wait -- vmcnt(0) for the first and the last chunk, a counted
    one for the 4 * NT / 2 - 2 between them (the next chunk's LDS-DMA pieces stay in flight)."""
    from wavenet_autoencoders_amd import _lib
    _lib.build()
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "obj", "head_train.s")
    text = open(path).read()
    meta = re.findall(r"\.name:\s+(_Z17head_train_kernel\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                      r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    assert len(meta) == 4, [m[0] for m in meta]
    for name, scratch, vgprs, spills in meta:
        assert int(scratch) == 0 and int(spills) == 0 and int(vgprs) <= 256, (name, scratch, vgprs, spills)
    for name, _, _, _ in meta:
        nt = 8 if "Li8E" in name else 4
        body = text.split(name + ":", 1)[1].split("s_endpgm", 1)[0]
        waits = re.findall(r";;#ASMSTART\s*\n\s*s_waitcnt vmcnt\((\d+)\)", body)       # (the kernel's only hand-written vmcnt waits)
        chunks = 4 * nt // 2
        assert len(waits) == chunks, (name, waits)
        pieces = str(nt * 4 // 8)
        assert waits[0] == "0" and waits[-1] == "0" and all(w == pieces for w in waits[1:-1]), (name, waits)
