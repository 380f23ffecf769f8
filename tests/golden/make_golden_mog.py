#!/usr/bin/env python
"""Golden vectors of the mixture-of-Gaussians output distribution (output_distribution "Normal").  Runs ONLY where a checkout of
the reference project exists; it is never needed to build or test.

Imports the reference's own ``wavenet_vocoder/mixture.py`` (never copied, never shipped) and runs ``mix_gaussian_loss`` and
``sample_from_mix_gaussian`` on small closed-form inputs for C = 2, 3 and 30, then stores inputs and outputs in ``mog.npz`` next
to this script:

  y_hat_C (B,C,T), y_C (B,T,1)      inputs; log-scale rows reach below log_scale_min
  loss_C (B,T,1), sum_C ()          reduce=False / reduce=True
  grad_C (B,C,T)                    d sum_C / d y_hat_C by autograd
  samp_C (B,T)                      sampler output, with the draws that produced it: u_mix_C (B,T,M) (M > 1 only), z_C (B,T)

The sampler's draws are recovered by re-seeding and drawing again in the reference's order (the Gumbel uniforms, then the normal
draw); the script asserts that the restatement in tests/mog_ref.py reproduces the reference's samples, losses and gradients from
them before it writes anything.

    python tests/golden/make_golden_mog.py /path/to/reference      (or WAE_REFERENCE=/path/to/reference)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("WAE_REFERENCE")
if not REF or not os.path.isdir(os.path.join(REF, "wavenet_vocoder")):
    sys.exit("usage: make_golden_mog.py <reference checkout> (the directory that holds wavenet_vocoder/)")
sys.path.insert(0, REF)
sys.path.insert(0, TESTS)

from wavenet_vocoder import mixture as ref_mix  # noqa: E402

import mog_ref  # noqa: E402

B, T, LOG_SCALE_MIN = 2, 24, -7.0


def inputs(C, seed):
    gen = torch.Generator().manual_seed(seed)
    M = 1 if C == 2 else C // 3
    mu0, ls0 = (0, 1) if C == 2 else (M, 2 * M)
    y_hat = torch.randn(B, C, T, generator=gen)
    y_hat[:, mu0:mu0 + M] = torch.rand(B, M, T, generator=gen) * 2.4 - 1.2
    y_hat[:, ls0:ls0 + M] = torch.rand(B, M, T, generator=gen) * 8.5 - 9.0     # about a quarter below log_scale_min
    y = torch.rand(B, T, 1, generator=gen) * 2 - 1
    return y_hat, y, M


def main():
    out = {}
    for C in (2, 3, 30):
        y_hat, y, M = inputs(C, 100 + C)
        assert bool((y_hat < LOG_SCALE_MIN).any())
        loss = ref_mix.mix_gaussian_loss(y_hat, y, log_scale_min=LOG_SCALE_MIN, reduce=False)
        yg = y_hat.clone().requires_grad_(True)
        total = ref_mix.mix_gaussian_loss(yg, y, log_scale_min=LOG_SCALE_MIN, reduce=True)
        total.backward()
        seed = 1234 + C
        torch.manual_seed(seed)
        samp = ref_mix.sample_from_mix_gaussian(y_hat, log_scale_min=LOG_SCALE_MIN)
        torch.manual_seed(seed)                      # the same draws, in the reference's order
        u_mix = torch.empty(B, T, M).uniform_(1e-5, 1.0 - 1e-5) if M > 1 else None
        z = torch.empty(B, T).normal_(0.0, 1.0)
        # the restatement reproduces the reference from these draws before anything is written
        assert float((mog_ref.mog_sample(y_hat, u_mix, z) - samp).abs().max()) < 1e-6, C
        assert float((mog_ref.mog_loss(y_hat, y, LOG_SCALE_MIN, reduce=False) - loss).abs().max()) <= 1e-6 * float(loss.abs().max()), C
        yr = y_hat.clone().requires_grad_(True)
        mog_ref.mog_loss(yr, y, LOG_SCALE_MIN, reduce=True).backward()
        assert float((yr.grad - yg.grad).abs().max()) <= 1e-6 * float(yg.grad.abs().max()), C
        out.update({f"y_hat_{C}": y_hat.numpy(), f"y_{C}": y.numpy(), f"loss_{C}": loss.detach().numpy(),
                    f"sum_{C}": np.float32(total.item()), f"grad_{C}": yg.grad.numpy(), f"samp_{C}": samp.numpy(),
                    f"z_{C}": z.numpy()})
        if u_mix is not None:
            out[f"u_mix_{C}"] = u_mix.numpy()
    out["log_scale_min"] = np.float32(LOG_SCALE_MIN)
    path = os.path.join(HERE, "mog.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
