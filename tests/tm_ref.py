"""Float64 restatement of the backward data path's time-major contraction (include/wae.h: wae_gemm_tm, wae_gemm_tm_ce mode 5,
wae_glu_bwd_fused, wae_glu_bwd_fused_dc), written from the header's statement and not from the kernels -- plain torch on the CPU,
no engine, DENSE matrices only (nothing here knows a fragment order; tests/tm_cases.py builds the packed streams):

    acc[b,t,:] = sum_s W_s . X_s[b, t + shift_s, :]             rows t + shift_s outside [0, T) are zeros

  W is (M, K) with the sources' columns back to back, K = sum_s cols_s; X_s is (B, T, cols_s).  Epilogues:
  mode 0: acc                                      mode 1: alpha (acc + aux),           aux (B, T, M)
  mode 2: z = [a | b] = aux (B, T, 2M):            [du s(b) (1 - tanh(a)^2) | du tanh(a) s(b) (1 - s(b))],  du = acc, s = sigmoid
  mode 3: relu(alpha (bias + acc)), aux = bias (M) mode 4: aux > 0 ? alpha acc : 0,     aux (B, T, M)
  mode 5: bias + acc over the first O classes, laid out (B, O, T) (the logits; nll / lse are tests/test_gpu_wide.py's)

Every result comes as TmOut(out, A, n, acc): the float64 value, the same expression on absolute values (|alpha|, |aux| and |bias|
included, before any gate factor or mask) and the number of terms of each element's sum -- what the exact cases (A < 2^22) and the
rounding bound 2 (n + 4) 2^-24 A need -- and the bare contraction (mode 2's du)."""
from typing import NamedTuple, Optional

import torch


class TmOut(NamedTuple):
    out: torch.Tensor
    A: torch.Tensor
    n: int
    acc: torch.Tensor


def shifted(X, shift, T):
    """X[b, t + shift, :] as float64, zeros where t + shift leaves [0, T)"""
    B, _, cols = X.shape
    out = torch.zeros(B, T, cols, dtype=torch.float64)
    lo, hi = max(0, -shift), min(T, T - shift)
    if hi > lo:
        out[:, lo:hi] = X[:, lo + shift:hi + shift].double()
    return out


def contraction(W, sources, shifts, B, T):
    """-> (acc, the same on absolute values), both (B, T, M)"""
    W = W.double()
    assert len(sources) == len(shifts) and W.shape[1] == sum(x.shape[2] for x in sources), (W.shape, [x.shape for x in sources])
    acc = torch.zeros(B, T, W.shape[0], dtype=torch.float64)
    A = torch.zeros_like(acc)
    k0 = 0
    for X, s in zip(sources, shifts):
        assert X.shape[:2] == (B, T)
        Xs, Ws = shifted(X, s, T), W[:, k0:k0 + X.shape[2]]
        acc += torch.einsum("btk,mk->btm", Xs, Ws)
        A += torch.einsum("btk,mk->btm", Xs.abs(), Ws.abs())
        k0 += X.shape[2]
    return acc, A


def gate_bwd(du, z):
    """u = tanh(a) sigmoid(b), z = [a | b]: (du/da | du/db) scaled by du"""
    H = du.shape[-1]
    a, b = z[..., :H].double(), z[..., H:2 * H].double()
    th, sg = torch.tanh(a), torch.sigmoid(b)
    return torch.cat([du * sg * (1.0 - th * th), du * th * sg * (1.0 - sg)], dim=-1)


def tm_ref(mode, W, sources, shifts, alpha, aux, B, T, O: Optional[int] = None) -> TmOut:
    acc, A = contraction(W, sources, shifts, B, T)
    n = int(W.shape[1])
    a, aa = float(alpha), abs(float(alpha))
    if mode == 0:
        return TmOut(acc, A, n, acc)
    if mode == 1:
        r = aux.double()
        return TmOut(a * (acc + r), aa * (A + r.abs()), n + 1, acc)
    if mode == 2:
        return TmOut(gate_bwd(acc, aux), torch.cat([A, A], dim=-1), n, acc)
    if mode == 3:
        bias = aux.double().view(1, 1, -1)
        return TmOut(torch.relu(a * (bias + acc)), aa * (bias.abs() + A), n + 1, acc)
    if mode == 4:
        keep = (aux.double() > 0).double()
        return TmOut(keep * (a * acc), aa * A, n, acc)
    if mode == 5:
        bias = aux.double().view(1, 1, -1)
        return TmOut((bias + acc)[:, :, :O].transpose(1, 2).contiguous(), (bias.abs() + A)[:, :, :O].transpose(1, 2).contiguous(), n + 1, acc)
    raise ValueError(f"mode {mode}")


class PairOut(NamedTuple):
    g_out: TmOut                    # phase A: dx_l-hat (B, T, Rp), unrounded
    handed: torch.Tensor            # what phase B contracts: g_out rounded to the storage dtype (fp32: as it is)
    dz_prev: Optional[TmOut]        # phase B: (B, T, 2Hp); None with last = 1
    dc: Optional[TmOut]             # the running conditioning-gradient sum (B, T, 64) after this launch, unrounded; None without w_c
    dc_to_out: bool                 # dc_mode bit 1: the sum goes to dc_out in the storage dtype and dc_acc keeps its content


def pair_ref(W_x, W_uo, W_us, dz, g_next, dskip, z_prev, ktaps, dilation, alpha, B, T, round_fn=None, W_c=None, dc_prev=None,
             dc_mode=0, last=0, handed=None) -> PairOut:
    """wae_glu_bwd_fused / wae_glu_bwd_fused_dc across one layer boundary.
    W_x (Rp, ktaps * 2Hp) tap by tap, tap j against dz[t + (ktaps - 1 - j) dilation]; W_uo (Hp, Rp), W_us (Hp, Sp); W_c (64, 2Hp).
    round_fn: storage rounding of the hand-over (the 16-bit kernels keep dx_l-hat as stored); handed: take this array as phase B's
    operand instead (a rounding case hands the kernel's own stored dx_l-hat over, so that phase A's error is not counted twice)."""
    shifts = [(ktaps - 1 - j) * dilation for j in range(ktaps)]
    ga = tm_ref(1, W_x, [dz] * ktaps, shifts, alpha, g_next, B, T)
    if handed is None:
        handed = round_fn(ga.out) if round_fn is not None else ga.out
    dc = None
    if W_c is not None:
        c = tm_ref(0, W_c, [dz], [0], 1.0, None, B, T)
        if dc_mode & 1:
            dc = TmOut(c.out + dc_prev.double(), c.A + dc_prev.double().abs(), c.n + 1, c.acc)
        else:
            dc = c
    gb = None
    if not last:
        gb = tm_ref(2, torch.cat([W_uo.double(), W_us.double()], dim=1), [handed.double(), dskip], [0, 0], 1.0, z_prev, B, T)
    return PairOut(ga, handed, gb, dc, bool(dc_mode & 2))
