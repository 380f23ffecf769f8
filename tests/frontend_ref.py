"""Plain float64 restatements, in torch on the CPU, of what csrc/frontend_bwd.hip and the helpers around frontend_backward compute
(include/wae.h: "backward of the front end", the layout helpers, wae_act_bwd, wae_vq_ema_update) -- the checkers of
tests/test_gpu_frontend_bwd.py.  Every function takes tensors of any float dtype and works in float64; tests/test_frontend_ref_cpu.py
checks each of them once against an explicit-loop restatement.

Every gradient is linear in its operands once the ReLU mask is fixed, so the same functions evaluated on the ABSOLUTE values of the
operands (with the same mask) give, per output element, the sum of the absolute values of its terms: the `A` of the rounding bound
|got - ref| <= (n + 4) 2^-24 A of an fp32 sum of n terms in any order, and the proof that an integer-valued case stays in exact
fp32 arithmetic (A < 2^22)."""
import torch
import torch.nn.functional as F


def _d(t):
    return None if t is None else torch.as_tensor(t).detach().double()


# ---------------------------------------------------------------------------------------------- convolution block
def conv_tout(Tin, k, stride, pad):
    """Output length of the block (0 or less: the shape does not exist)."""
    return (Tin + 2 * pad - k) // stride + 1


def conv_block_forward(x, w, b, stride, pad, relu, residual):
    """y = conv1d(x, w, b, stride, pad), optionally through ReLU, optionally + x (vqvae_model.py:17-23).  -> (y, mask): mask is the
    0/1 derivative of the ReLU at this input (all ones without ReLU)."""
    x, w, b = _d(x), _d(w), _d(b)
    pre = F.conv1d(x, w, b, stride=stride, padding=pad)
    mask = (pre > 0).double() if relu else torch.ones_like(pre)
    y = pre * mask
    if residual:
        y = y + x
    return y, mask


def relu_mask_from_output(y, x, residual):
    """The mask as the kernels form it, from the STORED output: (y - (residual ? x : 0)) > 0.  (The sign of a floating-point
    difference is exact, so float64 on fp32 operands decides as fp32 does.)"""
    y, x = _d(y), _d(x)
    return ((y - x if residual else y) > 0).double()


def conv_block_grads(x, w, dy, stride, pad, mask, residual):
    """-> (dx, dw, dbias) of sum(dy * out), out = conv1d(x, w, b) * mask (+ x), by autograd in float64.  mask: (B, Cout, Tout) of 0 / 1
    (conv_block_forward's, or relu_mask_from_output's), None = no ReLU."""
    x, w, dy = _d(x).requires_grad_(True), _d(w).requires_grad_(True), _d(dy)
    b = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    out = F.conv1d(x, w, b, stride=stride, padding=pad)
    if mask is not None:
        out = out * _d(mask)
    if residual:
        out = out + x
    return torch.autograd.grad(out, (x, w, b), dy)


# ---------------------------------------------------------------------------------------------- upsample stage
def upsample_stage_forward(inp, w, s):
    """inp (B, C, Tin), w (2s+1,) -> (B, C, Tin*s): nearest stretch by s (upsample.py:19-21), then the correlation with the 2s+1 taps,
    zero padded by s (:39-46): out[t] = sum_j w[j] * up[t + j - s]."""
    B, C, Tin = inp.shape
    up = torch.repeat_interleave(inp, s, dim=-1)
    return F.conv1d(up.reshape(B * C, 1, Tin * s), w.reshape(1, 1, 2 * s + 1), padding=s).reshape(B, C, Tin * s)


def upsample_stage_grads(inp, w, dout, s):
    """-> (din, dw) of sum(dout * upsample_stage_forward(inp, w, s)), by autograd in float64."""
    inp, w, dout = _d(inp).requires_grad_(True), _d(w).requires_grad_(True), _d(dout)
    return torch.autograd.grad(upsample_stage_forward(inp, w, s), (inp, w), dout)


# ---------------------------------------------------------------------------------------------- quantiser
def vq_slice_bwd(lat, quant, idx, dquant, d0, D, K, c_lat, c_emb):
    """The two closed forms of include/wae.h on channels [d0, d0+D) of (B, Dtot, Tq) tensors:
    dlat = dquant + c_lat (x - q) -> (B, D, Tq) (the slice alone);  demb[idx] += c_emb (q - x) -> (K, D), from zero.
    idx (B*Tq,) int64; dquant None = zero."""
    lat, quant, dquant = _d(lat), _d(quant), _d(dquant)
    B, _, Tq = lat.shape
    x, q = lat[:, d0:d0 + D], quant[:, d0:d0 + D]
    dlat = c_lat * (x - q)
    if dquant is not None:
        dlat = dlat + dquant[:, d0:d0 + D]
    demb = torch.zeros(K, D, dtype=torch.float64)
    demb.index_add_(0, torch.as_tensor(idx).long().reshape(-1), (c_emb * (q - x)).permute(0, 2, 1).reshape(B * Tq, D))
    return dlat, demb


def vq_bwd_coefficients(B, D, Tq, beta, loss_scale):
    """wae_vq_bwd is wae_vq_slice_bwd on the whole tensor with c_lat = loss_scale 2 beta / N, c_emb = loss_scale 2 / N, N = B D Tq."""
    n = float(B * D * Tq)
    return loss_scale * 2.0 * beta / n, loss_scale * 2.0 / n


def vq_ema_update(lat, idx, hist, cluster_size, ema_w, d0, D, decay, eps=1e-5):
    """The three formulas of include/wae.h (vector_quantization.py:190-215): cluster_size = decay cluster_size + (1 - decay) counts,
    Laplace smoothing (n + eps) / (sum n + K eps) * sum n, ema_w = decay ema_w + (1 - decay) sum of the latents of each code,
    emb = ema_w / cluster_size.  -> (cluster_size (K,), ema_w (K, D), emb (K, D))."""
    lat, n0, w0 = _d(lat), _d(cluster_size), _d(ema_w)
    B, _, Tq = lat.shape
    K = n0.numel()
    n1 = decay * n0 + (1.0 - decay) * _d(hist)[:K]
    tot = n1.sum()
    n2 = (n1 + eps) / (tot + K * eps) * tot
    dw = torch.zeros(K, D, dtype=torch.float64)
    dw.index_add_(0, torch.as_tensor(idx).long().reshape(-1), lat[:, d0:d0 + D].permute(0, 2, 1).reshape(B * Tq, D))
    w1 = decay * w0 + (1.0 - decay) * dw
    return n2, w1, w1 / n2[:, None]


# ---------------------------------------------------------------------------------------------- helpers around frontend_backward
def from_btc_scaled(inp, C, scale):
    """inp (B, T, Cp) of any float dtype -> (B, C, T) float64: cropped to C columns, transposed, times scale."""
    return _d(inp)[:, :, :C].transpose(1, 2).contiguous() * scale


def to_btc_masked(inp, Cp, lengths, scale):
    """inp (B, C, T) -> (B, T, Cp) float64: row t holds scale * in while t + 1 < min(length, T) (lengths None: T), zero otherwise; the
    pad columns C..Cp are zero."""
    inp = _d(inp)
    B, C, T = inp.shape
    out = torch.zeros(B, T, Cp, dtype=torch.float64)
    for b in range(B):
        n = T if lengths is None else min(int(lengths[b]), T)
        rows = max(n - 1, 0)
        out[b, :rows, :C] = inp[b, :, :rows].t() * scale
    return out


def act_bwd(y, d, kind, slope):
    """d * act'(.) formed from the activation's OUTPUT y: kind 1 ReLU [y > 0], 2 LeakyReLU [y > 0 ? 1 : slope], 3 Tanh 1 - y^2,
    4 Sigmoid y (1 - y)."""
    y, d = _d(y), _d(d)
    if kind == 1:
        g = (y > 0).double()
    elif kind == 2:
        g = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    elif kind == 3:
        g = 1.0 - y * y
    else:
        assert kind == 4, kind
        g = y * (1.0 - y)
    return d * g
