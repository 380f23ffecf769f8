"""The host side of WaeEngine.train_step_list that needs no GPU: packing.train_list_plan (offsets, the b * Tmax rows, tile counts, the
length rule, the max_rows refusal) and the oracle-only figures that motivate the ragged step -- what zero-padding does to vq_loss."""
import numpy as np
import pytest
import torch

from helpers import golden_model
from oracle import wae_oracle as O


def _geom():
    from wavenet_autoencoders_amd import Geometry
    return Geometry.from_cfg(golden_model("A")[0])


def test_plan_of_the_four_utterances():
    from wavenet_autoencoders_amd import packing as P
    g = _geom()
    tp = P.train_list_plan(g, [1280, 1920, 640, 5760], [8, 12, 4, 36])
    assert (tp.B, tp.Tmax, tp.rows, tp.pad_rows) == (4, 5760, 23040, 23040 - 9600)
    assert tp.enc.Tq.tolist() == [2, 3, 1, 9] and tp.enc.total_Tq == 15 and tp.enc.q_offsets.tolist() == [0, 2, 5, 6]
    # the conditioning chain writes item b at the rows b * Tmax of the dense operand
    assert tp.ups.offsets.tolist() == [0, 5760, 11520, 17280] and tp.ups.rows == 17280 + 5760
    assert [ln.kind for ln in tp.ups.launches] == ["conv_in", "stage", "stage", "stage", "last"]
    last = tp.ups.records(4)
    assert last[:-1, 2].tolist() == [0, 5760, 11520, 17280] and last[:-1, 1].tolist() == [256, 384, 128, 1152]
    assert last[-1, 3] == sum(-(-t // P.UPS_LIST_TILE_BTC) for t in (1280, 1920, 640, 5760))
    # the backward's own records: rows b * Tmax + t -> the packed columns, then every stage on running sums without gaps
    fb = tp.bwd_table[tp.fb_off:tp.fb_off + 20].reshape(5, 4)
    assert fb[:-1, 0].tolist() == [0, 1280, 3200, 3840] and fb[:-1, 1].tolist() == [1280, 1920, 640, 5760]
    assert fb[:-1, 2].tolist() == [0, 5760, 11520, 17280] and fb[-1, 3] == tp.fb_ntiles == 20 + 30 + 10 + 90
    assert tp.stage_pitch == [(15, 60), (60, 240), (240, 1920), (1920, 9600)]
    Tin = np.asarray([2, 3, 1, 9])
    for i, s in enumerate(g.upsample_scales):
        rec = tp.bwd_table[tp.stage_off[i]:tp.stage_off[i] + 20].reshape(5, 4)
        To = Tin * s
        assert rec[:-1, 1].tolist() == Tin.tolist()
        assert rec[:-1, 0].tolist() == (np.cumsum(Tin) - Tin).tolist() and rec[:-1, 2].tolist() == (np.cumsum(To) - To).tolist()
        assert rec[-1, 3] == tp.stage_ntiles[i] == int((-(-To // P.UPS_LIST_TILE_CT)).sum())
        Tin = To
    assert Tin.tolist() == [1280, 1920, 640, 5760]


def test_plan_refusals():
    from wavenet_autoencoders_amd import packing as P
    g = _geom()
    with pytest.raises(ValueError, match="item 2 has 639 samples"):
        P.train_list_plan(g, [1280, 1920, 639, 5760], [8, 12, 4, 36])
    with pytest.raises(ValueError, match="item 1 has no frame"):
        P.train_list_plan(g, [1280, 0], [8, 0])
    with pytest.raises(ValueError, match="empty"):
        P.train_list_plan(g, [], [])
    with pytest.raises(ValueError, match="max_rows 23039"):
        P.train_list_plan(g, [1280, 1920, 640, 5760], [8, 12, 4, 36], max_rows=23039)
    assert P.train_list_plan(g, [1280, 1920, 640, 5760], [8, 12, 4, 36], max_rows=23040).rows == 23040
    # frames that are no multiple of 4: Tq = ceil(F / 4), and the samples must follow it
    assert P.train_list_plan(g, [1920], [9]).enc.Tq.tolist() == [3]
    with pytest.raises(ValueError, match="item 0 has 1440 samples"):
        P.train_list_plan(g, [1440], [9])


def test_zero_padding_changes_the_commitment_loss():
    """golden model A in float64, utterances of 8, 12, 4 and 36 frames (torch.manual_seed(5)): the padded batch reports vq_loss 1.454,
    the utterances one by one, combined as score_list does (weights Tq_i / sum Tq), 2.290 -- the pad frames' latents are inside the
    padded batch's commitment mean."""
    cfg, sd, _, _, ocfg = golden_model("A")
    sd = {k: v.double() for k, v in sd.items()}
    torch.manual_seed(5)
    F = [8, 12, 4, 36]
    items = [(torch.randint(0, cfg["O"], (1, 160 * f)), torch.randn(1, cfg["c_in"], f), torch.tensor([i])) for i, f in enumerate(F)]
    with torch.no_grad():
        vq_list = 0.0
        for _, c, g in items:
            lat = O.encoder_forward(sd, c.double())
            vq_list = vq_list + O.vq_forward(sd["vq.embedding.weight"], lat)[1] * (lat.shape[-1] / 15)
        cpad = torch.zeros(4, cfg["c_in"], 36, dtype=torch.float64)
        for i, (_, c, _) in enumerate(items):
            cpad[i, :, :c.shape[2]] = c[0]
        vq_pad = O.vq_forward(sd["vq.embedding.weight"], O.encoder_forward(sd, cpad))[1]
    assert abs(float(vq_list) - 2.290) < 1e-3, float(vq_list)
    assert abs(float(vq_pad) - 1.454) < 1e-3, float(vq_pad)
