"""GPU: scalar-input decoders on the constant-size cooperative kernels (wae_ar_desc.scalar_input = 2, csrc/ar_coop.hip:
ar_coop_fast_body<.., SCALAR>), reached through WaeEngine.ar_path(scalar_coop=True, scalar_fast=True): single decodes, streamed decodes
and team lists at the reference's decoder sizes (20 layers, R = G = S = 256, C = 32) with a scalar head of O = 30 or 2 parameters.
REF20 has 2 stacks (dilations 1 .. 512: every residency tier of the 16-bit kernels holds layers); REF20x5 has 5 stacks (dilations 1, 2,
4, 8: at T = 48 every tap of every layer reads a row some step wrote, and every ring wraps).  Every decode checks that the cooperative
path ran and that no wait timed out; tolerances are those of tests/test_gpu_ar_scalar_coop.py."""
import ctypes
import functools
import math

import pytest
import torch

from oracle import wae_oracle as O
from helpers import rel_err
from test_gpu_ar_scalar_list import _alone, _equal, _items, _list

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-4, "bf16": 5e-2, "fp16": 1e-2}
REF20 = dict(layers=20, stacks=2, R=256, G=256, S=256, O=30, Cc=64, Cg=32, k=3, n_speakers=7, upsample_scales=None, cin_pad=0,
             scalar_input=True)
T48 = 48
LENS = [48, 17, 33, 5, 1]


def _cfg(stacks=2, O_ch=30, dist="Logistic", Cc=64):
    return dict(REF20, stacks=stacks, O=O_ch, Cc=Cc, output_distribution=dist)


@functools.lru_cache(maxsize=None)
def _state(stacks, O_ch, Cc):
    return O.make_state_dict(dict(_cfg(stacks, O_ch, "Logistic", Cc)), salt=5, with_encoder=False)


def _engine(cfg, dtype, monkeypatch, fast=True, scalar_coop=True, **split):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    monkeypatch.setenv("WAE_AR_COOP", "1")
    monkeypatch.setenv("WAE_AR_COOP_C", "32")
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype).ar_path(scalar_coop=scalar_coop, scalar_fast=fast, **split)
    assert eng.opt.ar_coop and eng.opt.ar_coop_c == 32
    eng.load_state_dict(_state(cfg["stacks"], cfg["O"], cfg["Cc"]))
    return eng


def _decode(eng, *args, cooperative=True, **kw):
    eng._ar_profile = None
    out = eng.incremental_forward(*args, **kw)
    torch.cuda.synchronize()
    if cooperative:
        assert eng._ar_profile is not None, "the decode fell back to the one-CU kernel"
        assert int(eng._ar_profile[0]) == 0, eng._ar_profile[:8].tolist()
    else:
        assert eng._ar_profile is None, "the decode took the cooperative path"
    return out


def _clip(cfg, B, T, salt=600):
    x = O.hash_fill((B, T), salt + 1) * 0.9
    c = O.hash_fill((B, cfg["Cc"], T), salt + 2) if cfg["Cc"] else None
    gid = (3 * torch.arange(B) + 1) % cfg["n_speakers"]
    return x, c, gid


def _draws(B, T, M, salt=500):
    u_mix = (O.hash_fill((B, T, M), salt + 1) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    u_log = (O.hash_fill((B, T), salt + 3) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    zn = O.hash_fill((B, T), salt + 2) * 1.7
    return u_mix, u_log, zn


def _draw_kw(cfg, B, T, salt=500):
    M = 1 if cfg["O"] == 2 else cfg["O"] // 3
    u_mix, u_log, zn = (t.cuda() for t in _draws(B, T, M, salt))
    if cfg["output_distribution"] == "Logistic":
        return dict(u_mix=u_mix, u_log=u_log, log_scale_min=-7.0)
    return dict(u_mix=u_mix if M > 1 else None, z=zn)


def _cu(t):
    return None if t is None else t.cuda()


@functools.lru_cache(maxsize=None)
def _oracle_parameters(stacks, O_ch, Cc, B, T=T48):
    """the CPU oracle's teacher-forced parameters: once per shape, shared by the storage types and the two distributions"""
    cfg = _cfg(stacks, O_ch, "Logistic", Cc)
    x, c, gid = _clip(cfg, B, T)
    with torch.no_grad():
        return O.incremental_forward(_state(stacks, O_ch, Cc), dict(layers=cfg["layers"], stacks=stacks, upsample_scales=None, cin_pad=0),
                                     c, gid, T, test_inputs=x.unsqueeze(1), mode="logits")


# ---- 1. the constant-size kernel really ran ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_the_flag_selects_the_kernel_with_one_shared_ring(dtype, monkeypatch):
    """wae_ar_generate_coop_scalar itself on a zeroed (1, 32, ring_total) ring: the constant-size kernels write member 0's region only
    (one ring shared by the 32 members), the any-shape kernel every member's own"""
    from wavenet_autoencoders_amd import _lib as L
    cfg = _cfg(5)
    eng = _engine(cfg, dtype, monkeypatch)
    eng.pack_ar_weights()
    g, T, dev = eng.g, 24, eng.device
    x, c, gid = _clip(cfg, 1, T)
    c_up = torch.zeros(1, T, g.Ccp, dtype=eng.tdtype, device=dev)
    eng._ar_cond_rows(c.cuda().contiguous().float(), c_up, True)
    zb = eng._ar_speaker_rows(1, gid.to(torch.int32).cuda())
    x = x.cuda().contiguous()
    rt = eng.ar_ring_total
    for flag in (1, 0):
        d = L.ArDesc(eng.dt, 1, T, g.layers, g.R, g.Rp, g.G, g.Hp, g.S, g.O, g.Cc, g.Ccp, g.k, 0, 0, 1, math.sqrt(1.0 / g.layers), T)
        d.scalar_sized = flag
        assert eng.lib.wae_ar_coop_ring_floats(ctypes.byref(d), 32, rt) == (rt if flag else 32 * rt)
        ring = torch.zeros(32 * rt, dtype=torch.float32, device=dev)
        msg, acc, err = eng._ar_exchange(d, 32, 1, torch.zeros)
        params = torch.zeros(1, g.O, T, dtype=torch.float32, device=dev)
        L.check(eng.lib.wae_ar_generate_coop_scalar(ctypes.byref(d), 32, 0, *eng._ar_net_args(ring, zb, c_up), L.ptr(x), None, None, -7.0, 0,
                                                    None, L.ptr(params), L.ptr(msg), L.ptr(acc), L.ptr(err), eng.stream()),
                "ar_generate_coop_scalar")
        torch.cuda.synchronize()
        assert int(err[0]) == 0, err[:8].tolist()
        regions = ring.view(32, rt)
        assert float(regions[0].abs().max()) > 0.0 and float(params.abs().max()) > 0.0
        if flag:
            assert int((regions[1:] != 0).sum()) == 0, "a member wrote a ring of its own: the any-shape kernel ran"
        else:
            assert float(regions[1].abs().max()) > 0.0, "member 1 wrote no ring of its own: the constant-size kernel ran"


# ---- 2. teacher-forced parameters against the oracle -------------------------------------------------------------------------------
def _teacher_forced(cfg, dtype, B, monkeypatch):
    eng = _engine(cfg, dtype, monkeypatch)
    x, c, gid = _clip(cfg, B, T48)
    out = _decode(eng, _cu(c), gid.cuda(), T48, mode="logits", test_inputs=x.cuda(), c_is_upsampled=True)
    want = _oracle_parameters(cfg["stacks"], cfg["O"], cfg["Cc"], B)
    assert out["logits"].shape == want.shape == (B, cfg["O"], T48)
    err = rel_err(out["logits"].cpu(), want)
    print(f"constant-size scalar kernel, teacher-forced {dtype} stacks={cfg['stacks']} O={cfg['O']} {cfg['output_distribution']} "
          f"Cc={cfg['Cc']} B={B}: rel err {err:.3e}")
    assert math.isfinite(err) and err < TOL[dtype]


@pytest.mark.parametrize("dist,O_ch", [("Logistic", 30), ("Normal", 30), ("Normal", 2)])
@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_teacher_forced_parameters_against_the_oracle(dtype, B, dist, O_ch, monkeypatch):
    _teacher_forced(_cfg(2, O_ch, dist), dtype, B, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_teacher_forced_parameters_with_wrapping_rings(dtype, monkeypatch):
    _teacher_forced(_cfg(5), dtype, 8, monkeypatch)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_teacher_forced_parameters_without_conditioning(dtype, monkeypatch):
    """Cc = 0: three W1 packets per thread in 16-bit storage, six in fp32"""
    _teacher_forced(_cfg(2, Cc=0), dtype, 2, monkeypatch)


# ---- 3. the draw is the parameters' draw -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,O_ch", [("Logistic", 30), ("Normal", 30), ("Normal", 2)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_draw_is_the_sampler_kernel_on_the_returned_parameters(dtype, dist, O_ch, monkeypatch):
    from wavenet_autoencoders_amd import _lib as L
    cfg = _cfg(5, O_ch, dist)
    eng = _engine(cfg, dtype, monkeypatch)
    B, T = 3, 40
    _, c, gid = _clip(cfg, B, T)
    M = 1 if O_ch == 2 else O_ch // 3
    kw = _draw_kw(cfg, B, T)
    out = _decode(eng, c.cuda(), gid.cuda(), T, mode="sample", c_is_upsampled=True, want_logits=True, **kw)
    params = out["logits"].contiguous()
    assert params.shape == (B, O_ch, T)
    again = torch.empty(B, T, device="cuda")
    if dist == "Logistic":
        L.check(L.lib().wae_dmol_sample(L.ptr(params), L.ptr(kw["u_mix"]), L.ptr(kw["u_log"]), L.ptr(again), B, M, T, -7.0, 0, None),
                "dmol_sample")
    else:
        L.check(L.lib().wae_mog_sample(L.ptr(params), L.ptr(kw["u_mix"]) if M > 1 else None, L.ptr(kw["z"]), L.ptr(again), B, O_ch, T, None),
                "mog_sample")
    torch.cuda.synchronize()
    assert float(out["x"].abs().max()) <= 1.0 and float(out["x"].std()) > 0.0
    assert torch.equal(again, out["x"]), float((again - out["x"]).abs().max())


# ---- 4. / 5. feedback wiring and partial forcing -----------------------------------------------------------------------------------
def _one_cu_parameters(cfg, dtype, monkeypatch, c, gid, inputs):
    """the one-CU kernel (an engine without the opt-in), teacher-forced on `inputs` (B, T)"""
    ref = _engine(cfg, dtype, monkeypatch, fast=False, scalar_coop=False)
    out = _decode(ref, c, gid, inputs.shape[1], mode="logits", test_inputs=inputs.contiguous(), c_is_upsampled=True, cooperative=False)
    return out["logits"].cpu()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_feeds_back_the_sample_it_drew(dtype, monkeypatch):
    cfg = _cfg(5)
    eng = _engine(cfg, dtype, monkeypatch)
    B = 2
    _, c, gid = _clip(cfg, B, T48)
    c, gid = c.cuda(), gid.cuda()
    out = _decode(eng, c, gid, T48, mode="sample", c_is_upsampled=True, want_logits=True, **_draw_kw(cfg, B, T48, salt=520))
    xs = out["x"]
    assert float(xs.std()) > 0.0
    fed = torch.cat([torch.zeros_like(xs[:, :1]), xs[:, :-1]], dim=1)
    err = rel_err(out["logits"].cpu(), _one_cu_parameters(cfg, dtype, monkeypatch, c, gid, fed))
    print(f"constant-size scalar kernel, feedback wiring {dtype}: rel err {err:.3e}")
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_partial_teacher_forcing(dtype, monkeypatch):
    """n_forced = 5 of T = 48: steps 0..4 are the fully forced decode's bit for bit, later steps consume the drawn samples"""
    cfg = _cfg(5)
    eng = _engine(cfg, dtype, monkeypatch)
    B, nf = 2, 5
    x, c, gid = (t.cuda() for t in _clip(cfg, B, T48))
    full = _decode(eng, c, gid, T48, mode="logits", test_inputs=x, c_is_upsampled=True)["logits"]
    part = _decode(eng, c, gid, T48, mode="sample", test_inputs=x, n_forced=nf, c_is_upsampled=True, want_logits=True,
                   **_draw_kw(cfg, B, T48, salt=540))
    assert torch.equal(part["logits"][:, :, :nf], full[:, :, :nf])
    fed = torch.cat([x[:, :nf], part["x"][:, nf - 1:-1]], dim=1)
    assert float((fed[:, nf:] - x[:, nf:]).abs().max()) > 1e-3
    want = _one_cu_parameters(cfg, dtype, monkeypatch, c, gid, fed)
    err = rel_err(part["logits"].cpu()[:, :, nf:], want[:, :, nf:])
    print(f"constant-size scalar kernel, partial forcing {dtype}: rel err of the free steps {err:.3e}")
    assert err < TOL[dtype]


# ---- 6. where the packets wait is not arithmetic -----------------------------------------------------------------------------------
def test_residency_splits_are_bitwise_one_result(monkeypatch):
    cfg = _cfg(2)
    B, T = 3, 40
    _, c, gid = _clip(cfg, B, T)
    kw = _draw_kw(cfg, B, T, salt=560)
    runs = {}
    for name, split in (("default", {}), ("streaming", dict(lds_layers=0, reg_layers=0)), ("no_vgpr_bank", dict(reg_layers=11)),
                        ("lds2_regs5", dict(lds_layers=2, reg_layers=5))):
        eng = _engine(cfg, "bf16", monkeypatch, **split)
        runs[name] = _decode(eng, c.cuda(), gid.cuda(), T, mode="sample", c_is_upsampled=True, want_logits=True, **kw)
    assert float(runs["default"]["x"].std()) > 0.0
    for name, r in runs.items():
        assert torch.equal(r["x"], runs["default"]["x"]) and torch.equal(r["logits"], runs["default"]["logits"]), name


# ---- 7. streaming ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_streamed_decode_is_the_one_shot_decode(dtype, monkeypatch):
    cfg = _cfg(5)
    eng = _engine(cfg, dtype, monkeypatch)
    B = 2
    _, c, gid = _clip(cfg, B, T48)
    kw = dict(mode="sample", c_is_upsampled=True, want_logits=True, **_draw_kw(cfg, B, T48, salt=580))
    whole = _decode(eng, c.cuda(), gid.cuda(), T48, **kw)
    assert float(whole["x"].std()) > 0.0
    for chunk in (1, 7, 48):
        parts = []
        for item in eng.incremental_stream(c.cuda(), gid.cuda(), T48, chunk, **kw):
            assert eng._ar_profile is not None and int(eng._ar_profile[0]) == 0
            parts.append(item)
        assert [p["x"].shape[1] for p in parts] == [min(chunk, T48 - t) for t in range(0, T48, chunk)]
        assert torch.equal(torch.cat([p["x"] for p in parts], dim=1), whole["x"]), chunk
        assert torch.equal(torch.cat([p["logits"] for p in parts], dim=2), whole["logits"]), chunk


# ---- 8. team lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dist,O_ch", [("bf16", "Logistic", 30), ("fp32", "Normal", 2)])
def test_team_list_items_are_their_single_decodes(dtype, dist, O_ch, monkeypatch):
    cfg = _cfg(5, O_ch, dist)
    eng = _engine(cfg, dtype, monkeypatch)
    items = _items(cfg, LENS)
    want = [_alone(eng, it, coop=True) for it in items]
    assert float(torch.cat([x for x, _ in want]).std()) > 0.0
    for teams in (2, 1):      # one team: every clip behind the first is decoded by a team that has just finished a longer one
        _equal(_list(eng, items, coop=True, want_logits=True, teams=teams), want, (dtype, dist, "teams", teams))
    perm = [3, 0, 4, 2, 1]
    _equal(_list(eng, [items[i] for i in perm], coop=True, want_logits=True, teams=2), [want[i] for i in perm], "permuted")
    # a forced prefix per item: inside the clip, the whole clip, one step, none
    gen = torch.Generator().manual_seed(8)
    for it, F in zip(items, (20, 17, 1, 0, 1)):
        if F:
            it["test_inputs"] = (torch.rand(F, generator=gen) * 1.8 - 0.9).cuda()
    want = [_alone(eng, it, coop=True) for it in items]
    _equal(_list(eng, items, coop=True, want_logits=True, teams=2), want, "forced prefixes")


def test_team_list_without_the_flag_stays_on_the_any_shape_kernel(monkeypatch):
    """the same list at scalar_fast=False is bitwise ITS single decode, and differs from the constant-size kernels' by rounding only"""
    cfg = _cfg(5)
    items = _items(cfg, LENS)
    slow = _engine(cfg, "fp32", monkeypatch, fast=False)
    want = [_alone(slow, it, coop=True) for it in items]
    _equal(_list(slow, items, coop=True, want_logits=True, teams=2), want, "any-shape")
    fast = _engine(cfg, "fp32", monkeypatch)
    for it, (_, wp) in zip(items, want):
        it = dict(it, test_inputs=O.hash_fill((it["T"],), 77).cuda() * 0.9)
        a = _alone(fast, it, "logits", coop=True)[1]
        b = _alone(slow, it, "logits", coop=True)[1]
        err = rel_err(a.cpu(), b.cpu())
        print(f"constant-size against any-shape, teacher-forced T={it['T']}: rel err {err:.3e}")
        assert err < TOL["fp32"]


# ---- 9. reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dist", [("fp32", "Logistic"), ("bf16", "Normal")])
def test_sampled_decode_is_reproducible(dtype, dist, monkeypatch):
    cfg = _cfg(2, 30, dist)
    eng = _engine(cfg, dtype, monkeypatch)
    B = 4
    _, c, gid = _clip(cfg, B, T48)
    kw = _draw_kw(cfg, B, T48, salt=590)
    runs = [_decode(eng, c.cuda(), gid.cuda(), T48, mode="sample", c_is_upsampled=True, want_logits=True, **kw) for _ in range(2)]
    assert torch.equal(runs[0]["x"], runs[1]["x"]) and torch.equal(runs[0]["logits"], runs[1]["logits"])
