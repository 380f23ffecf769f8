"""Gradient accumulation, host side: the window's loss weights (distributed.accum_weights), the two C entries' declarations against
their ctypes bindings, and the training script's --accum-steps option."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(metas, **kw):
    from wavenet_autoencoders_amd.distributed import accum_weights
    return accum_weights(metas, **kw)


def test_weights_sum_to_one_and_equal_shapes_give_one_over_m():
    for M in (1, 2, 3, 8):
        w, N = _weights([(4, 1280, None, 4 * 16 * 2)] * M)
        assert N == M * 4 * 1279
        assert all(abs(a - 1.0 / M) < 1e-15 and abs(b - 1.0 / M) < 1e-15 for a, b in w)
        assert abs(sum(a for a, _ in w) - 1.0) < 1e-12 and abs(sum(b for _, b in w) - 1.0) < 1e-12


def test_weights_of_ragged_lengths_follow_the_masked_count():
    # n_i = sum_b max(min(len_b, T_i) - 1, 0): lengths past T count as T, clips shorter than 2 contribute nothing
    metas = [(3, 100, torch.tensor([100, 250, 1]), 30), (2, 60, torch.tensor([0, 41]), 10), (1, 50, None, 0)]
    w, N = _weights(metas)
    n = [99 + 99 + 0, 0 + 40, 49]
    assert N == sum(n)
    for (a, b), ni, ei in zip(w, n, (30, 10, 0)):
        assert a == ni / N and b == ei / 40.0
    assert abs(sum(a for a, _ in w) - 1.0) < 1e-12 and abs(sum(b for _, b in w) - 1.0) < 1e-12
    # lengths as a list or an int64 tensor: the same numbers
    assert _weights([(3, 100, [100, 250, 1], 30)])[1] == 198.0


def test_a_window_without_loss_positions_or_latents_has_zero_weights():
    w, N = _weights([(2, 1, None, 0), (1, 5, torch.tensor([1]), 0)])
    assert N == 0.0 and w == [(0.0, 0.0), (0.0, 0.0)]


def test_world_two_uses_the_reduced_count():
    seen = []

    def total(n_local):
        seen.append(n_local)
        return n_local + 1000.0          # the other rank's window

    metas = [(2, 101, None, 8), (1, 51, torch.tensor([31]), 24)]
    w, N = _weights(metas, world=2, total=total)
    assert seen == [230.0] and N == 1230.0          # ONE collective for the whole window
    assert w[0] == (200 * 2 / 1230.0, 0.25) and w[1] == (30 * 2 / 1230.0, 0.75)
    # world 1 never calls it
    _weights(metas, world=1, total=lambda n: 1 / 0)


@pytest.mark.parametrize("name,nargs", [("wae_gproj_bwd_consume", 19), ("wae_accum_stats", 10)])
def test_entries_are_declared_and_bound_with_matching_arity(name, nargs):
    from wavenet_autoencoders_amd import _lib
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", header, re.S)
    assert m, f"{name} is not declared in include/wae.h"
    res, args = _lib.SIGNATURES[name]
    assert len(m.group(1).split(",")) == nargs == len(args) and res is _lib.c_i32
    assert os.path.exists(os.path.join(ROOT, "wavenet_autoencoders_amd", "csrc", "accum.hip"))
    # the consuming entry takes wae_gproj_bwd's arguments
    if name == "wae_gproj_bwd_consume":
        assert list(args) == list(_lib.SIGNATURES["wae_gproj_bwd"][1])
        plain = re.search(r"\bint wae_gproj_bwd\(([^;]*?)\);", header, re.S).group(1)
        strip = lambda s: [" ".join(p.replace("const float* c1", "float* c1").split()) for p in s.split(",")]  # noqa: E731
        assert strip(m.group(1)) == strip(plain)
    if os.path.exists(_lib.LIB_PATH):
        assert getattr(_lib.lib(), name).argtypes is not None


def test_accum_steps_option_parses_and_refuses_zero(capsys):
    sys.path.insert(0, ROOT)
    import vqwae_train
    assert vqwae_train.parse_args([]).accum_steps == 1
    assert vqwae_train.parse_args(["--accum-steps", "4"]).accum_steps == 4
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            vqwae_train.parse_args(["--accum-steps", bad])
        assert "--accum-steps" in capsys.readouterr().err


def test_engine_interface_is_there():
    import inspect
    from wavenet_autoencoders_amd.engine import WaeEngine
    sig = inspect.signature(WaeEngine.accumulate)
    assert list(sig.parameters)[:5] == ["self", "x", "c", "gid", "lengths"]
    for k in ("ce_weight", "vq_weight", "quantize_channels", "log_scale_min"):
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["ce_weight"].default == 1.0 and sig.parameters["vq_weight"].default == 1.0
    ap = inspect.signature(WaeEngine.apply_step).parameters
    assert [ap[k].default for k in ("lr", "clip_thresh", "ema_decay", "grad_hook", "grad_sync")] == [4e-4, 100.0, 0.9999, None, None]
    assert hasattr(WaeEngine, "discard_step") and "ce_scale" in inspect.signature(WaeEngine.train_step_accum).parameters
