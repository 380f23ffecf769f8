"""Float64 restatement of the weight-gradient contraction (include/wae.h: wae_gemm_tn_tiles, wae_gemm_tn_stream, wae_gemm_tn_static),
written from the header's statement and not from the kernels -- plain torch on the CPU, no engine:

    C[m][n] += alpha * sum_{b,t} P[b,t][m] * Q[b,t+shift][n]          rows t + shift outside [0, T) are zeros

  * P[b,t][m] = P_array[b,t][p_col + m], or the one-hot operand (ids[b,t] == m0 + m);
  * ones_col >= 0: a virtual all-ones Q column at that output-local index -- clip b adds alpha * sum_t P[b,t][m] into
    C[m][ones_col + b]; a stored Q column of the same index is ignored (only the tile launch permits ones_col < n_valid);
  * OUTSKIP of the static launch: C1[m][n] from a second Q operand, Cb[n] += alpha * sum_{b,t} Q[b,t][n] (shift 0);
  * rows: an optional (B, T) multiplicity of every time row -- how often the segment lists of a team launch hand the 32-row slab
    of (b, t) to this job (1 everywhere for a launch that covers every slab once).

Every output comes as TnOut(update, A, n): the float64 update, the same expression on absolute values (|alpha| included) and the
number of terms of each element's sum -- what the exact cases (A < 2^22) and the rounding bound (n + 4) 2^-24 A need."""
from typing import NamedTuple, Optional

import torch


class TnSpec(NamedTuple):
    B: int
    T: int
    m_valid: int
    n_valid: int
    shift: int = 0
    alpha: float = 1.0
    ones_col: int = -1
    p_col: int = 0
    q_col: int = 0
    m0: Optional[int] = None      # not None: the one-hot form, P[b,t][m] = (ids[b,t] == m0 + m)
    n1_valid: int = 0             # OUTSKIP: columns of the second Q operand
    q1_col: int = 0
    want_cb: bool = False         # OUTSKIP: the column sums of Q


class TnOut(NamedTuple):
    update: torch.Tensor
    A: torch.Tensor
    n: torch.Tensor


def c_width(spec: TnSpec) -> int:
    """columns of the C window a job touches: the data columns, then (possibly after a gap) one ones column per clip"""
    return max(spec.n_valid, spec.ones_col + spec.B) if spec.ones_col >= 0 else spec.n_valid


def _shifted(Q, col, width, shift, T):
    """Q[b, t + shift][col : col + width] as float64, zeros where t + shift leaves [0, T)"""
    B = Q.shape[0]
    out = torch.zeros(B, T, width, dtype=torch.float64)
    lo, hi = max(0, -shift), min(T, T - shift)
    if hi > lo and width > 0:
        out[:, lo:hi] = Q[:, lo + shift:hi + shift, col:col + width].double()
    return out


def tn_reference(spec: TnSpec, P=None, Q=None, ids=None, Q1=None, rows=None):
    """-> {"C": TnOut (m_valid, c_width), "C1": TnOut (m_valid, n1_valid) if n1_valid, "Cb": TnOut (n_valid,) if want_cb}"""
    B, T, M, N = spec.B, spec.T, spec.m_valid, spec.n_valid
    if spec.m0 is not None:
        Pm = (ids.view(B, T, 1).long() == (spec.m0 + torch.arange(M)).view(1, 1, M)).double()
    else:
        Pm = P[:, :, spec.p_col:spec.p_col + M].double()
    assert Pm.shape == (B, T, M)
    w = torch.ones(B, T, dtype=torch.float64) if rows is None else rows.double()
    Pw, Pa = Pm * w.view(B, T, 1), Pm.abs() * w.view(B, T, 1)
    inside = torch.zeros(T, dtype=torch.float64)
    inside[max(0, -spec.shift):max(0, min(T, T - spec.shift))] = 1.0
    a, aa = float(spec.alpha), abs(float(spec.alpha))

    def against(Qarr, col, width, drop=-1):
        Qs = _shifted(Qarr, col, width, spec.shift, T) if width > 0 else torch.zeros(B, T, 0, dtype=torch.float64)
        if 0 <= drop < width:
            Qs[:, :, drop] = 0.0
        upd = a * torch.einsum("btm,btn->mn", Pw, Qs)
        A = aa * torch.einsum("btm,btn->mn", Pa, Qs.abs())
        n = torch.full((M, width), float((w * inside.view(1, T)).sum()), dtype=torch.float64)
        return upd, A, n

    W = c_width(spec)
    upd, A, n = (torch.zeros(M, W, dtype=torch.float64) for _ in range(3))
    u0, A0, n0 = against(Q, spec.q_col, N, spec.ones_col)
    upd[:, :N], A[:, :N], n[:, :N] = u0, A0, n0
    if spec.ones_col >= 0:
        assert spec.shift == 0, "the ones columns are defined for shift 0 only"
        for b in range(B):
            upd[:, spec.ones_col + b] += a * Pw[b].sum(0)
            A[:, spec.ones_col + b] += aa * Pa[b].sum(0)
            n[:, spec.ones_col + b] += float(w[b].sum())
    out = {"C": TnOut(upd, A, n)}
    if spec.n1_valid > 0:
        out["C1"] = TnOut(*against(Q1, spec.q1_col, spec.n1_valid))
    if spec.want_cb:
        assert spec.shift == 0, "the column sums are defined for shift 0 only"
        Qd = Q[:, :, spec.q_col:spec.q_col + N].double() * w.view(B, T, 1)
        out["Cb"] = TnOut(a * Qd.sum((0, 1)), aa * Qd.abs().sum((0, 1)), torch.full((N,), float(w.sum()), dtype=torch.float64))
    return out
