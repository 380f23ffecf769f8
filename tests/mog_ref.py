"""Restatement of the mixture-of-Gaussians output distribution (output_distribution "Normal"; reference mixture.py:161-270 and
MixtureGaussianLoss, vqwae_train.py:404-422) in plain torch on the CPU -- the checker of the HIP kernels (wae_mog_loss_fwd,
wae_mog_sample, the Gaussian draw of wae_ar_generate_scalar_mog).  Pinned to the reference by tests/golden/mog.npz.

Layout of y (B, C, T): C == 2 is one Gaussian [mean | log scale]; otherwise M = C / 3 as [logit | mean | log scale], and C == 3 is
one Gaussian whose logit row is ignored."""
import math

import torch


def layout(C: int):
    """-> (M, row of the first mean, row of the first log scale)."""
    if C == 2:
        return 1, 0, 1
    assert C % 3 == 0, C
    M = C // 3
    return M, M, 2 * M


def mog_loss(y_hat: torch.Tensor, y: torch.Tensor, log_scale_min: float = -7.0, reduce: bool = True) -> torch.Tensor:
    """y_hat (B, C, T), y (B, T, 1) -> -sum log p (reduce) or (B, T, 1) per-step negative log-likelihoods."""
    M, mu0, ls0 = layout(y_hat.shape[1])
    p = y_hat.transpose(1, 2)                                            # (B, T, C)
    mu = p[..., mu0:mu0 + M]
    log_s = torch.clamp(p[..., ls0:ls0 + M], min=log_scale_min)
    scale = torch.exp(log_s)
    cen = y.expand_as(mu) - mu
    # Normal(0, scale).log_prob(cen), formed as torch.distributions forms it
    lp = -(cen ** 2) / (2 * scale ** 2) - scale.log() - math.log(math.sqrt(2 * math.pi))
    if M > 1:
        lp = lp + torch.log_softmax(p[..., :M], dim=-1)
        m = lp.max(-1, keepdim=True)[0]
        lp = m + torch.log(torch.exp(lp - m).sum(-1, keepdim=True))
    nll = -lp                                                            # (B, T, 1)
    return nll.sum() if reduce else nll


def masked_mog_loss(y_hat: torch.Tensor, y: torch.Tensor, lengths: torch.Tensor, log_scale_min: float = -7.0) -> torch.Tensor:
    """The training criterion: step t of y_hat predicts y[t+1] (vqwae_train.py:766), masked mean over the valid steps."""
    T = y_hat.shape[-1]
    mask = (torch.arange(T - 1).unsqueeze(0) < (lengths.view(-1, 1) - 1)).float().unsqueeze(-1)
    losses = mog_loss(y_hat[:, :, :-1], y[:, 1:, :], log_scale_min, reduce=False)
    return (losses * mask).sum() / mask.sum()


def mog_sample(y: torch.Tensor, u_mix, z: torch.Tensor) -> torch.Tensor:
    """y (B, C, T); u_mix (B, T, M) uniforms of the Gumbel-max pick (used when M > 1), z (B, T) standard normals -> (B, T) in [-1, 1].
    The log scales are not clamped (the reference's sampler ignores log_scale_min)."""
    M, mu0, ls0 = layout(y.shape[1])
    p = y.transpose(1, 2)
    if M > 1:
        pick = (p[..., :M] - torch.log(-torch.log(u_mix))).argmax(-1, keepdim=True)
    else:
        pick = torch.zeros(p.shape[0], p.shape[1], 1, dtype=torch.int64)
    mu = p[..., mu0:mu0 + M].gather(-1, pick).squeeze(-1)
    log_s = p[..., ls0:ls0 + M].gather(-1, pick).squeeze(-1)
    return torch.clamp(z * torch.exp(log_s) + mu, -1.0, 1.0)
