"""Float64 restatements of the forward launches of the decoder (include/wae.h: wae_glu_layer_fwd / _drop / _list, wae_head_fwd,
wae_head_fwd_from_h0, wae_first_conv_fwd), written from the header's statements and the reference's formulas (modules.py:115-163,
wavenet.py:203-214, vqwae_train.py:363-379 with the shift of :764) -- plain torch on the CPU, DENSE matrices only: nothing here knows a
fragment order, a tile or the engine (tests/fwd_cases.py builds the packed streams with the product's maps).

Layer (time-major rows, clip i owning T_i consecutive rows; every clip starts from zeros before its t = 0):
    z[t]  = zb[clip] + sum_j W1[:, j, :] . x_conv[t - (k - 1 - j) d] + Wc . c[t]          (2H: a-half | b-half)
    u[t]  = tanh(z_a[t]) sigmoid(z_b[t])
    x'[t] = sqrt(.5) (b_out + W_out . u[t] + x_in[t])
Head:
    h0 = relu(scale (b_skip_sum + W_skip . u)),  h1 = relu(b1 + W1 . h0),  logits = b3 + W3 . h1          (B, O, T)
    lse[b, t] = logsumexp_o logits[b, o, t],  nll[b, t] = lse[b, t] - logits[b, target[b, t + 1], t] for t < T - 1, 0 at t = T - 1
    `handed` functions restate what a kernel hands from one GEMM to the next (the storage rounding of h0 and of h1).
Every sum comes with the same expression on absolute values (A) and its number of terms (n): what the exact cases (A < 2^22 units) and
the rounding bound 2 (n + 4) 2^-24 A need."""
from typing import Callable, NamedTuple, Optional, Sequence

import torch

SQRT_HALF = 0.70710678118654752440


def gate(z):
    """z = [a | b] (.., 2H) float64 -> tanh(a) sigmoid(b)"""
    H = z.shape[-1] // 2
    return torch.tanh(z[..., :H]) * torch.sigmoid(z[..., H:])


class LayerOut(NamedTuple):
    z: torch.Tensor         # (rows, 2H)
    u: torch.Tensor         # (rows, H)
    x_out: torch.Tensor     # (rows, R)
    yx: torch.Tensor        # (rows, R): b_out + W_out u + x_in, before the scale
    zA: torch.Tensor        # z on absolute values
    yA: torch.Tensor        # yx on absolute values
    n1: int                 # terms of a z sum
    n2: int                 # terms of a yx sum


def shifted_rows(x, shift, Ts):
    """x (rows, C) packed clip after clip -> x[t - shift] within each clip, zeros where t - shift < 0"""
    out = torch.zeros_like(x)
    r0 = 0
    for T in Ts:
        if shift < T:
            out[r0 + shift:r0 + T] = x[r0:r0 + T - shift]
        r0 += T
    assert r0 == x.shape[0]
    return out


def layer_ref(x_in, x_conv, c, zb, W1, Wc, W_out, b_out, k: int, dilation: int, Ts: Sequence[int], zb_rows: Optional[Sequence[int]] = None,
              u_fn: Optional[Callable] = None) -> LayerOut:
    """x_in, x_conv (rows, R); c (rows, Cc) or None; zb (B, 2H); W1 (2H, k, R); Wc (2H, Cc) or None; W_out (R, H); b_out (R);
    Ts: the clips' lengths in row order; zb_rows: every clip's row of zb (None: its index); u_fn: what GEMM 2 is handed for u"""
    f = lambda a: a.double()       # noqa: E731
    x_in, x_conv, zb, W1, W_out, b_out = f(x_in), f(x_conv), f(zb), f(W1), f(W_out), f(b_out)
    rows = x_in.shape[0]
    assert sum(Ts) == rows and W1.shape[1] == k
    zrow = list(range(len(Ts))) if zb_rows is None else list(zb_rows)
    z = torch.cat([zb[zrow[i]].expand(T, -1) for i, T in enumerate(Ts)], dim=0).clone()
    zA = z.abs()
    for j in range(k):
        xs = shifted_rows(x_conv, (k - 1 - j) * dilation, Ts)
        z += xs @ W1[:, j, :].t()
        zA += xs.abs() @ W1[:, j, :].abs().t()
    n1 = 1 + k * x_in.shape[1]
    if c is not None:
        z += f(c) @ f(Wc).t()
        zA += f(c).abs() @ f(Wc).abs().t()
        n1 += c.shape[1]
    u = gate(z)
    uh = u if u_fn is None else u_fn(u)
    yx = b_out + uh @ W_out.t() + x_in
    yA = b_out.abs() + uh.abs() @ W_out.abs().t() + x_in.abs()
    return LayerOut(z, u, yx * SQRT_HALF, yx, zA, yA, n1, W_out.shape[1] + 2)


class HeadOut(NamedTuple):
    h0: torch.Tensor        # (B, T, S) as handed to GEMM 1
    h1: torch.Tensor        # (B, T, S) as handed to GEMM 2
    logits: torch.Tensor    # (B, O, T)
    lse: torch.Tensor       # (B, T)
    nll: torch.Tensor       # (B, T)
    A: tuple                # the three sums on absolute values: skips (None from h0), h1's, the logits' (B, T, .)
    n: tuple                # their numbers of terms


def ce_ref(logits, target):
    """logits (B, O, T) float64, target (B, T) integers -> lse (B, T), nll (B, T) with the one-step shift, 0 at t = T - 1"""
    lse = torch.logsumexp(logits, dim=1)
    nll = torch.zeros_like(lse)
    T = logits.shape[2]
    if T > 1:
        pick = torch.gather(logits[:, :, :T - 1], 1, target[:, 1:].long().unsqueeze(1)).squeeze(1)
        nll[:, :T - 1] = lse[:, :T - 1] - pick
    return lse, nll


def head_ref(x, W_skip, b_skip_sum, W1, b1, W3, b3, scale, target, from_h0=False, handed0=None, handed1=None) -> HeadOut:
    """x: u (B, T, Ku) or, from_h0, h0 (B, T, S); W_skip (S, Ku); W1 (S, S); W3 (O, S); handed0 / handed1: the roundings of the two
    hand-overs (None: none)"""
    f = lambda a: a.double()       # noqa: E731
    x, W1, b1, W3, b3 = f(x), f(W1), f(b1), f(W3), f(b3)
    if from_h0:
        h0, A0, n0 = x, None, 0
    else:
        W_skip, b0 = f(W_skip), f(b_skip_sum)
        h0 = torch.relu(float(scale) * (b0 + x @ W_skip.t()))
        A0 = abs(float(scale)) * (b0.abs() + x.abs() @ W_skip.abs().t())
        n0 = W_skip.shape[1] + 1
        if handed0 is not None:
            h0 = handed0(h0)
    h1 = torch.relu(b1 + h0 @ W1.t())
    A1 = b1.abs() + h0.abs() @ W1.abs().t()
    if handed1 is not None:
        h1 = handed1(h1)
    logits, A2 = logits_ref(h1, W3, b3)
    lse, nll = ce_ref(logits, target) if target is not None else (torch.logsumexp(logits, dim=1), None)
    return HeadOut(h0, h1, logits, lse, nll, (A0, A1, A2), (n0, W1.shape[1] + 1, W3.shape[1] + 1))


def logits_ref(h1, W3, b3):
    """h1 (B, T, S) -> (logits (B, O, T), the same on absolute values (B, T, O))"""
    h1, W3, b3 = h1.double(), W3.double(), b3.double()
    return (b3 + h1 @ W3.t()).transpose(1, 2).contiguous(), b3.abs() + h1.abs() @ W3.abs().t()


def first_conv_ref(ids, xs, W, bias):
    """class-id mode: ids (BT) integers (outside [0, O): clamped to the nearest class), W (R, O) -> W[:, id] + bias;
    scalar mode (ids None): xs (BT), W (R, 1) -> W[:, 0] xs + bias.  Returns (x0 (BT, R), whether an id was outside its table)"""
    W, bias = W.double(), bias.double()
    if ids is not None:
        O = W.shape[1]
        ids = ids.long()
        bad = bool(((ids < 0) | (ids >= O)).any())
        return W.t()[ids.clamp(0, O - 1)] + bias, bad
    return xs.double().unsqueeze(1) * W[:, 0] + bias, False
