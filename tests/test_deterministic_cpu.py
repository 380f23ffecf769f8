"""The reproducible train step without a GPU: the option (default off, the environment's flip, what it pins, its documentation), the
fixed-order entries of the small sums exported, declared in include/wae.h and bound in _lib.py, their refusals before any launch, and
vqwae_train.py's --deterministic reaching the options an engine is created with."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
PTR = ctypes.c_void_p(0x1000)


def _clean(monkeypatch):
    for k in list(os.environ):
        if k.startswith("WAE_"):
            monkeypatch.delenv(k, raising=False)


def test_the_option_is_off_by_default_and_follows_the_environment(monkeypatch):
    from wavenet_autoencoders_amd.options import EngineOptions
    _clean(monkeypatch)
    d = EngineOptions.from_env()
    assert d == EngineOptions() and d.deterministic is False and d.pinned() is d
    for val, want in (("1", True), ("0", False), ("yes", False)):
        monkeypatch.setenv("WAE_DETERMINISTIC", val)
        assert EngineOptions.from_env().deterministic is want, val


def test_the_mode_pins_the_switches_without_a_fixed_order_form(monkeypatch):
    from wavenet_autoencoders_amd.options import EngineOptions
    _clean(monkeypatch)
    monkeypatch.setenv("WAE_DETERMINISTIC", "1")
    for env in ({}, {"WAE_TN_STREAM": "1", "WAE_SIDE": "1", "WAE_CHAINS": "2"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        o = EngineOptions.from_env()
        p = o.pinned()
        assert p.deterministic and p.tn_stream is False and p.side is False and p.chains == "1"
        # ... and nothing else
        import dataclasses
        assert dataclasses.replace(p, tn_stream=o.tn_stream, side=o.side, chains=o.chains) == o


def test_the_option_is_documented_with_what_it_pins():
    import wavenet_autoencoders_amd.options as opts
    doc = opts.__doc__
    assert re.search(r"^  WAE_DETERMINISTIC +0 +1:", doc, re.M), "documented below the table, at two spaces"
    assert "WAE_DETERMINISTIC" not in set(re.findall(r"^    (WAE_[A-Z0-9_]+) ", doc, re.M))
    for word in ("tn_stream = False", "side = False", 'chains = "1"', "NotImplementedError", "same device model and build",
                 "Not the default mode's bits"):
        assert word in doc, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "WAE_DETERMINISTIC" in readme and "--deterministic" in readme
    for word in ("WAE_DETERMINISTIC", "wae_gemm_tn_tiles_det", "clip-major, split-minor", "does not promise"):
        assert word in design, word


def test_the_engine_reads_the_pinned_options():
    import inspect
    from wavenet_autoencoders_amd.engine import WaeEngine
    src = inspect.getsource(WaeEngine.__init__)
    assert "EngineOptions.from_env().pinned()" in src and "_det_bufs" in src


ENTRIES = {"wae_gproj_bwd_det_floats": 4, "wae_gproj_bwd_det": 22, "wae_upsample_stage_bwd_det_floats": 0, "wae_upsample_stage_bwd_det": 12,
           "wae_vq_slice_bwd_det": 15, "wae_vq_bwd_det": 13, "wae_vq_loss_det": 10, "wae_clip_adam_ema_det": 18}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_the_entries_are_declared_and_bound(name):
    from wavenet_autoencoders_amd import _lib
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    m = re.search(r"\b(?:int|int64_t) " + name + r"\(([^;]*?)\);", header, re.S)
    assert m, f"{name} is not declared in include/wae.h"
    nargs = 0 if m.group(1).strip() == "void" else len(m.group(1).split(","))
    assert nargs == ENTRIES[name] == len(_lib.SIGNATURES[name][1])
    assert getattr(_lib.lib(), name).argtypes is not None


def test_the_header_states_every_order():
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    for word in ("No floating-point atomics, no workgroup waits for another", "the clips of that speaker in index order",
                 "the blocks 0 .. nbw-1 in order", "one workgroup per code", "a code that no frame uses is not written",
                 "parts[1 ..", "at least 1025 doubles"):
        assert word in header, word


def test_the_size_queries():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert lib.wae_upsample_stage_bwd_det_floats() == 256 * 33
    assert lib.wae_gproj_bwd_det_floats(3, 2, 32, 8) == 2 * 2 * 3 * 8
    assert lib.wae_gproj_bwd_det_floats(8, 24, 136, 16) == 24 * 9 * 8 * 16        # 272 rows: eight blocks and a ragged ninth
    assert lib.wae_gproj_bwd_det_floats(8, 24, 128, 0) == 0


def test_the_entries_refuse_before_any_launch():
    """(the pointers are not device memory and there may be no device)"""
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    adam = (1, 4e-4, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.9999, None)
    calls = [
        lambda: lib.wae_upsample_stage_bwd_det(PTR, PTR, PTR, PTR, PTR, PTR, 256 * 33 - 1, 1, 3, 4, 4, None),
        lambda: lib.wae_upsample_stage_bwd_det(PTR, PTR, PTR, PTR, PTR, None, 256 * 33, 1, 3, 4, 4, None),
        lambda: lib.wae_upsample_stage_bwd_det(PTR, PTR, PTR, PTR, PTR, PTR, 256 * 33, 1, 3, 4, 17, None),
        lambda: lib.wae_gproj_bwd_det(PTR, PTR, 0, 400, 2000, PTR, 4000, None, PTR, 64 * 13, 13, 7, 3, 2, 40, 32, 8, 5, 0, PTR, 2 * 2 * 3 * 8 - 1, None),
        lambda: lib.wae_gproj_bwd_det(PTR, PTR, 0, 400, 2000, PTR, 4000, None, PTR, 64 * 13, 13, 7, 3, 2, 40, 32, 8, 5, 0, None, 1 << 20, None),
        lambda: lib.wae_gproj_bwd_det(PTR, PTR, 0, 400, 2000, PTR, 4000, None, PTR, 64 * 13, 9, 7, 3, 2, 40, 32, 8, 5, 0, PTR, 1 << 20, None),
        lambda: lib.wae_vq_slice_bwd_det(PTR, PTR, PTR, PTR, PTR, PTR, 2, 12, 3, 5, 37, 0, 0.5, 2.0, None),          # K = 0 with a codebook gradient
        lambda: lib.wae_vq_slice_bwd_det(PTR, PTR, PTR, PTR, PTR, PTR, 2, 12, 8, 5, 37, 9, 0.5, 2.0, None),          # the slice leaves the tensor
        lambda: lib.wae_vq_slice_bwd_det(PTR, PTR, PTR, PTR, PTR, PTR, 2, 2048, 0, 1025, 37, 9, 0.5, 2.0, None),     # D > 1024
        lambda: lib.wae_vq_bwd_det(PTR, PTR, PTR, PTR, PTR, None, 2, 16, 32, 8, 0.25, 1.0, None),
        lambda: lib.wae_vq_loss_det(PTR, PTR, None, 2, 12, 3, 5, 37, 1.25, None),
        lambda: lib.wae_vq_loss_det(PTR, PTR, PTR, 2, 12, 9, 5, 37, 1.25, None),
        lambda: lib.wae_clip_adam_ema_det(PTR, PTR, PTR, PTR, PTR, 100, PTR, 1024, PTR, *adam),
        lambda: lib.wae_clip_adam_ema_det(PTR, PTR, PTR, PTR, PTR, 100, None, 1025, PTR, *adam),
        lambda: lib.wae_clip_adam_ema_det(PTR, PTR, PTR, PTR, PTR, 100, PTR, 1025, PTR, 0, *adam[1:]),
    ]
    for i, call in enumerate(calls):
        assert call() == EINVAL, (i, lib.wae_last_error())


def test_the_training_script_carries_the_flag_to_the_options(monkeypatch):
    import vqwae_train
    _clean(monkeypatch)
    args = vqwae_train.parse_args([])
    assert args.deterministic is False and vqwae_train.engine_switches(args).deterministic is False
    assert "WAE_DETERMINISTIC" not in os.environ
    monkeypatch.setenv("WAE_DETERMINISTIC", "0")          # (monkeypatch restores what engine_switches sets below)
    args = vqwae_train.parse_args(["--deterministic"])
    assert args.deterministic is True
    opt = vqwae_train.engine_switches(args)
    assert opt.deterministic and not opt.tn_stream and not opt.side and opt.chains == "1"
    assert os.environ["WAE_DETERMINISTIC"] == "1"         # what WaeEngine.__init__ reads, before main() creates the engine
    import inspect
    src = inspect.getsource(vqwae_train.main)
    assert src.index("engine_switches(args)") < src.index("WaeEngine(geom")
