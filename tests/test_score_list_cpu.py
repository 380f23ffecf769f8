"""List scoring in full, without a GPU: the table of wae_vq_stats_segments (packing.vq_seg_table), the definition of "the list as one
batch" for the quantiser's two numbers pinned on the oracle, the ABI of the new entry and its refusals before any launch, and the
host signatures that carry the mixture losses and the statistics through to the public interface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import wae_oracle as O
from wavenet_autoencoders_amd import packing as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
PTR = ctypes.c_void_p(0x1000)
SMALL = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
             c_in=39, K=32, cin_pad=0)


# ---------------------------------------------------------------------------------------------------------------- the table
def test_vq_seg_table_is_the_plans_offsets_and_lengths():
    plan = P.encode_list_plan([1, 5, 8, 20, 257])
    tab = P.vq_seg_table(plan.q_offsets, plan.Tq)
    assert tab.dtype == np.int32 and tab.shape == (5, 2) and tab.flags["C_CONTIGUOUS"]
    Tq = [1, 2, 2, 5, 65]
    assert list(tab[:, 1]) == Tq == list(plan.Tq)
    assert list(tab[:, 0]) == [sum(Tq[:i]) for i in range(5)]
    assert int(tab[-1].sum()) == plan.total_Tq
    free = P.vq_seg_table([100, 0, 40], [7, 3, 9])                 # the offsets are the caller's: gaps and any order
    assert free.tolist() == [[100, 7], [0, 3], [40, 9]]


@pytest.mark.parametrize("offs,Tq", [([], []), ([0, 3], [3, 0]), ([0, 3], [3, -2]), ([0], [3, 4]), ([-1, 3], [3, 4]),
                                     ([0, 2 ** 31 - 2], [3, 4])])
def test_vq_seg_table_refuses(offs, Tq):
    with pytest.raises(ValueError):
        P.vq_seg_table(offs, Tq)


def test_vq_seg_table_names_the_item_without_frames():
    with pytest.raises(ValueError, match="item 2 has Tq < 1"):
        P.vq_seg_table([0, 3, 5, 5], [3, 2, 0, 4])


# ---------------------------------------------------------------------------------------------------------------- the definition
def test_the_list_as_one_batch_is_the_concatenation_as_one_clip():
    """oracle.vq_forward on three utterances' latents side by side as ONE clip (B = 1): its vq_loss is (beta + 1) sum sqerr_i /
    (D sum Tq_i) and its perplexity that of sum hist_i, both from the per-utterance calls -- in float64, to 1e-12.  This is what
    wae_vq_stats_segments' `out` and WaeEngine.last_list_stats mean, pinned before any kernel runs."""
    sd = {k: v.double() for k, v in O.make_state_dict(SMALL, 1).items()}
    emb = sd["vq.embedding.weight"]
    K, D, beta = emb.shape[0], emb.shape[1], 0.25
    with torch.no_grad():
        lats = [O.encoder_forward(sd, O.hash_fill((SMALL["c_in"], F), 40 + i, 1.7).double()[None]) for i, F in enumerate((5, 8, 20))]
        assert all(lat.dtype == torch.float64 for lat in lats)
        sqerr, hist = [], []
        for lat in lats:
            quant, _, _, idx = O.vq_forward(emb, lat, beta)
            sqerr.append(float(((quant - lat) ** 2).sum()))
            hist.append(torch.bincount(idx.reshape(-1), minlength=K).numpy())
        _, vq_cat, perp_cat, idx_cat = O.vq_forward(emb, torch.cat(lats, dim=2), beta)
    Tq = [lat.shape[2] for lat in lats]
    assert torch.equal(idx_cat.reshape(-1), torch.cat([O.vq_forward(emb, lat, beta)[3].reshape(-1) for lat in lats]))
    vq, perp, frames, tot = P.vq_list_totals(sqerr, hist, D, beta + 1.0)
    assert frames == sum(Tq) and tot == pytest.approx(sum(sqerr), rel=1e-15)
    assert vq == pytest.approx((beta + 1.0) * sum(sqerr) / (D * sum(Tq)), rel=1e-15)
    assert abs(vq - float(vq_cat)) <= 1e-12 * abs(float(vq_cat)), (vq, float(vq_cat))
    assert abs(perp - float(perp_cat)) <= 1e-12 * abs(float(perp_cat)), (perp, float(perp_cat))
    # and it is NOT the mean of the utterances' own numbers: they weigh by frames
    own = [O.vq_forward(emb, lat, beta)[1:3] for lat in lats]
    assert abs(np.mean([float(o[0]) for o in own]) - vq) > 1e-3 * vq


def test_totals_of_a_list_without_frames_are_zero():
    assert P.vq_list_totals([0.0, 0.0], np.zeros((2, 7), dtype=np.int32), 16, 1.25) == (0.0, 0.0, 0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_entry_is_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    lib = _lib.lib()
    m = re.search(r"\bwae_vq_stats_segments\(([^;]*?)\);", header, re.S)
    assert m, "wae_vq_stats_segments is not declared in include/wae.h"
    assert len(m.group(1).split(",")) == 15 == len(_lib.SIGNATURES["wae_vq_stats_segments"][1])
    assert lib.wae_vq_stats_segments.argtypes is not None
    assert re.search(r"typedef struct wae_vq_seg \{ int32_t q_off, Tq; \} wae_vq_seg;", header)
    assert [f[0] for f in _lib.VqSeg._fields_] == ["q_off", "Tq"] and ctypes.sizeof(_lib.VqSeg) == 8
    for word in ("integer atomics", "fixed order", "no floating-point atomics", "WAE_EINVAL", "WAE_EUNSUPPORTED", "K > 8192",
                 "nothing is read for it", "first"):
        assert word in header, word


def _stats(lib, **kw):
    a = dict(lat=PTR, quant=PTR, idx=PTR, segs=PTR, nsegs=3, D=16, pitch=100, K=32, c_loss=1.25, first=0, sqerr=PTR, hist=PTR,
             item_stats=PTR, out=PTR)
    a.update(kw)
    return lib.wae_vq_stats_segments(a["lat"], a["quant"], a["idx"], a["segs"], a["nsegs"], a["D"], a["pitch"], a["K"], a["c_loss"],
                                     a["first"], a["sqerr"], a["hist"], a["item_stats"], a["out"], None)


@pytest.mark.parametrize("case,code", [
    (dict(lat=None), EINVAL), (dict(quant=None), EINVAL), (dict(idx=None), EINVAL), (dict(segs=None), EINVAL), (dict(sqerr=None), EINVAL),
    (dict(hist=None), EINVAL), (dict(item_stats=None), EINVAL), (dict(out=None), EINVAL), (dict(nsegs=0), EINVAL), (dict(nsegs=-4), EINVAL),
    (dict(D=0), EINVAL), (dict(K=0), EINVAL), (dict(pitch=0), EINVAL), (dict(first=-1), EINVAL),
    (dict(K=8193), EUNSUPPORTED), (dict(K=1 << 20), EUNSUPPORTED),
    (dict(K=8193, D=0), EINVAL),                        # a bad argument comes before an unsupported size
])
def test_the_entry_refuses_before_any_launch(case, code):
    """The pointers here are not device memory and this machine may have no device: a refusal that came after a launch would not
    return these codes."""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _stats(lib, **case) == code, lib.wae_last_error()
    assert lib.wae_last_error().startswith(b"vq_stats_segments: ")


# ---------------------------------------------------------------------------------------------------------------- the host
def test_the_host_signatures_carry_the_feature():
    import vqwae_train
    from wavenet_autoencoders_amd.engine import WaeEngine
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder.wavenet import WaveNet
    par = lambda f: inspect.signature(f).parameters      # noqa: E731
    # encode_list keeps its parameters (tests/test_encode_list_cpu.py pins them); the statistics have a door of their own
    assert list(par(WaeEngine.encode_list)) == ["self", "feats", "want_latents", "want_idx", "max_frames"]
    p = par(WaeEngine.encode_list_stats)
    assert list(p) == ["self", "feats", "beta", "want_latents", "want_idx", "max_frames"] and p["beta"].default == 0.25
    p = par(WaeEngine.decoder_forward_list)
    assert p["quantize_channels"].default == 65536 and p["log_scale_min"].default == -7.0 and p["want_nll"].default is True
    p = par(WaeEngine.forward_list)
    assert p["want_stats"].default is False and p["quantize_channels"].default == 65536 and p["log_scale_min"].default == -7.0
    p = par(WaeEngine.score_list)
    assert [k for k in p][1:] == ["items", "beta", "quantize_channels", "log_scale_min", "max_rows"]
    assert (p["beta"].default, p["quantize_channels"].default, p["log_scale_min"].default, p["max_rows"].default) == (0.25, 65536, -7.0, None)
    # the NLL of a list is on by default for every model, scalar-input ones included
    assert par(WaveNet.forward_list)["want_nll"].default is True and par(VQVAE.forward_list)["want_nll"].default is True
    assert callable(VQVAE.score_list)
    for fn in (WaeEngine.decoder_forward_list, vqwae_train.evaluate):
        assert "NotImplementedError" not in inspect.getsource(fn), fn.__name__
    assert "score_list" in inspect.getsource(vqwae_train.evaluate)
