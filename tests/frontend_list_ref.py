"""Float64 references of the list forms of the front end's backward (csrc/frontend_bwd_list.hip; include/wae.h:
wae_from_btc_list, wae_upsample_stage_bwd_list, wae_enc_conv_bwd_list): tests/frontend_ref.py's functions applied per item, each item
a batch of one, the weight gradients summed over the items -- and the packing helpers the tests share.  As in frontend_ref.py, the
same functions on the absolute values of the operands give every output's sum of |terms|."""
import numpy as np
import torch

import frontend_ref as R

GAP_FILL = float(2 ** 20)       # what the gap columns of every input hold: read as a neighbour's zero, it shows in a named element


def scattered_offsets(lengths, rng, gap=3):
    """First column of every item in a packed array whose items lie in a shuffled order with `gap` unowned columns in front of each
    and behind the last: offsets that are not monotone in the item index.  -> (offsets (n,), pitch)."""
    lengths = [int(t) for t in lengths]
    order = rng.permutation(len(lengths))
    offs, at = [0] * len(lengths), gap
    for i in order:
        offs[i] = at
        at += lengths[i] + gap
    return np.asarray(offs, dtype=np.int64), at


def pack(items, offsets, pitch, fill):
    """items: (C, T_i) tensors -> (C, pitch) float32, item i at the columns [offsets_i, offsets_i + T_i), `fill` everywhere else."""
    C = items[0].shape[0]
    out = torch.full((C, pitch), float(fill), dtype=torch.float32)
    for it, o in zip(items, offsets):
        out[:, int(o):int(o) + it.shape[1]] = it.float()
    return out


def owned(offsets, lengths, pitch):
    """(pitch,) bool: the columns some item owns."""
    m = torch.zeros(pitch, dtype=torch.bool)
    for o, t in zip(offsets, lengths):
        m[int(o):int(o) + int(t)] = True
    return m


def conv_list_forward(xs, w, b, stride, pad, relu, residual):
    """-> ([y_i (Cout, Tout_i) float64], [mask_i]) : frontend_ref.conv_block_forward per item as a batch of one."""
    ys, masks = [], []
    for x in xs:
        y, m = R.conv_block_forward(x[None], w, b, stride, pad, relu, residual)
        ys.append(y[0])
        masks.append(m[0])
    return ys, masks


def conv_list_grads(xs, w, dys, stride, pad, masks, residual, skip=()):
    """-> ([dx_i (Cin, Tin_i)], dw, dbias): frontend_ref.conv_block_grads per item, dw and dbias summed over the items.  masks None:
    no ReLU.  skip: item indices that contribute nothing (their dx is None)."""
    dxs, dw, db = [], 0.0, 0.0
    for i, (x, dy) in enumerate(zip(xs, dys)):
        if i in skip:
            dxs.append(None)
            continue
        gx, gw, gb = R.conv_block_grads(x[None], w, dy[None], stride, pad, None if masks is None else masks[i][None], residual)
        dxs.append(gx[0])
        dw, db = dw + gw, db + gb
    return dxs, dw, db


def upsample_list_grads(ins, w, douts, s, skip=()):
    """-> ([din_i (C, Tin_i)], dw (2s+1,)): frontend_ref.upsample_stage_grads per item, dw summed over the items."""
    dins, dw = [], 0.0
    for i, (x, d) in enumerate(zip(ins, douts)):
        if i in skip:
            dins.append(None)
            continue
        gi, gw = R.upsample_stage_grads(x[None], w, d[None], s)
        dins.append(gi[0])
        dw = dw + gw
    return dins, dw


def from_btc_list(rows, row_offsets, lengths, C, scale):
    """rows (R, Cp) of any float dtype -> [(C, T_i) float64]: item i's rows [row_offsets_i, + T_i), cropped to C channels, transposed,
    times scale (frontend_ref.from_btc_scaled per item)."""
    return [R.from_btc_scaled(rows[int(o):int(o) + int(t)][None], C, scale)[0] for o, t in zip(row_offsets, lengths)]
