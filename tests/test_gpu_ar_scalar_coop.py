"""GPU: scalar-input decoders on the cooperative decode kernel (wae_ar_generate_coop_scalar, csrc/ar_coop.hip: ar_coop_kernel<E, true>),
reached through WaeEngine.ar_path(scalar_coop=True).  Every case checks that the cooperative path really ran (a silent fall-back to
the one-CU kernel must not pass); a raised time-out flag is a failure."""
import numpy as np
import pytest
import torch

import mog_ref
from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
TOL = {"fp32": 1e-4, "bf16": 5e-2, "fp16": 1e-2}


def _engine(cfg, sd, dtype, monkeypatch, C=32, scalar_coop=True):
    """(WAE_AR_COOP / WAE_AR_COOP_C are read when the engine is built, cf. test_gpu_configs.py::_set_ar_path)"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    monkeypatch.setenv("WAE_AR_COOP", "1")
    monkeypatch.setenv("WAE_AR_COOP_C", str(C))
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype).ar_path(scalar_coop=scalar_coop)
    assert eng.opt.ar_coop and eng.opt.ar_coop_c == C
    eng.load_state_dict(sd)
    return eng


def _model_S(dtype, monkeypatch, O_ch=30, dist="Logistic", C=32, scalar_coop=True):
    """Golden model S (scalar input: R 32, G 64, S 32, O 30, B 2) or its O = 2 variant (closed-form weights of the same sizes)."""
    cfg, sd, ins, z, ocfg = golden_model("S")
    cfg = dict(cfg, output_distribution=dist)
    if O_ch != cfg["O"]:
        cfg["O"] = O_ch
        sd = O.make_state_dict(cfg, int(z["salt"]))
    return _engine(cfg, sd, dtype, monkeypatch, C, scalar_coop), cfg, sd, ins, ocfg


def _decode(eng, *args, cooperative=True, **kw):
    """incremental_forward + the proof of which path ran: the cooperative paths (and only they) leave their error / profile words in
    eng._ar_profile; word 0 is the time-out flag."""
    eng._ar_profile = None
    out = eng.incremental_forward(*args, **kw)
    torch.cuda.synchronize()
    if cooperative:
        assert eng._ar_profile is not None, "the decode fell back to the one-CU kernel"
        assert int(eng._ar_profile[0]) == 0, eng._ar_profile[:8].tolist()
    else:
        assert eng._ar_profile is None, "the decode took the cooperative path"
    return out


def _draws(B, T, M, salt=500):
    u_mix = (O.hash_fill((B, T, M), salt + 1) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    u_log = (O.hash_fill((B, T), salt + 3) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    zn = O.hash_fill((B, T), salt + 2) * 1.7
    return u_mix, u_log, zn


# ---- 1. the reference's own vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 8, 3])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scalar_coop_decode_against_reference_vectors(dtype, C, monkeypatch):
    """The inputs and tolerances of test_gpu_ar.py::test_scalar_input_decode_against_reference_vectors on 32 members (two of them own no
    parameter row), 8 (gate row slices fold inside a wave) and 3 (11-channel shares: the non-power-of-two split)."""
    eng, cfg, sd, ins, ocfg = _model_S(dtype, monkeypatch, C=C)
    z = load_npz("ar_S")
    c_up = torch.from_numpy(z["c_up"]).cuda()
    Tar = c_up.shape[-1]
    x = ins["x"][:, 0, :Tar].contiguous().cuda()
    g = ins["g"].cuda()
    out = _decode(eng, c_up, g, Tar, mode="logits", test_inputs=x, c_is_upsampled=True)
    err = rel_err(out["logits"].cpu(), z["params_tf"])
    print(f"teacher-forced parameters {dtype} C={C}: rel err {err:.3e}")
    assert err < TOL[dtype]
    if dtype == "fp32":
        roll = _decode(eng, c_up[:, :, :24].contiguous(), g, 24, mode="sample", c_is_upsampled=True,
                       u_mix=torch.from_numpy(z["u_mix"])[:, :24].contiguous().cuda(),
                       u_log=torch.from_numpy(z["u_log"])[:, :24].contiguous().cuda(), log_scale_min=-7.0)
        d = float((roll["x"].cpu() - torch.from_numpy(z["roll"])[:, 0]).abs().max())
        print(f"24-step roll-out C={C}: max abs diff {d:.3e}")
        assert d < 1e-3


# ---- 2. the Gaussian draw (the procedure and thresholds of test_gpu_mog.py::_decode_against_oracle) --------------------------------
def _gumbel_margin(params, u_mix):
    M, _, _ = mog_ref.layout(params.shape[1])
    if M == 1:
        return torch.full((params.shape[0], params.shape[2]), float("inf"))
    sc = (params.transpose(1, 2)[..., :M] - torch.log(-torch.log(u_mix))).double()
    top = sc.topk(2, dim=-1)[0]
    return top[..., 0] - top[..., 1]


def _gaussian_decode_against_oracle(O_ch, dtype, monkeypatch, T=40):
    eng, cfg, sd, ins, ocfg = _model_S(dtype, monkeypatch, O_ch=O_ch, dist="Normal")
    z = load_npz("ar_S")
    c_up = torch.from_numpy(z["c_up"])[:, :, :T].contiguous()
    g = ins["g"]
    B = c_up.shape[0]
    M = 1 if O_ch == 2 else O_ch // 3
    u_mix = (O.hash_fill((B, T, M), 501) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    zn = O.hash_fill((B, T), 502) * 1.7
    out = _decode(eng, c_up.cuda(), g.cuda(), T, mode="sample", c_is_upsampled=True, u_mix=u_mix.cuda() if M > 1 else None, z=zn.cuda())
    xs = out["x"].cpu()
    assert xs.shape == (B, T) and float(xs.abs().max()) <= 1.0
    ti = torch.cat([torch.zeros(B, 1), xs[:, :-1]], dim=1).unsqueeze(1)
    params = O.incremental_forward(sd, dict(ocfg, upsample_scales=None), c_up, g, T, test_inputs=ti, mode="logits")
    want = mog_ref.mog_sample(params, u_mix if M > 1 else None, zn)
    return xs, want, _gumbel_margin(params, u_mix)


@pytest.mark.parametrize("O_ch", [30, 2])
def test_scalar_coop_gaussian_draw_fp32(O_ch, monkeypatch):
    xs, want, margin = _gaussian_decode_against_oracle(O_ch, "fp32", monkeypatch)
    diff = (xs - want).abs()
    off = diff > 1e-4
    print(f"Gaussian draw fp32 O={O_ch}: max diff {float(diff.max()):.3e}, steps off {float(off.float().mean()):.3f}")
    assert bool((margin[off] < 1e-3).all()), (diff.max(), margin[off])
    assert float(off.float().mean()) <= 0.05


@pytest.mark.parametrize("O_ch", [30, 2])
def test_scalar_coop_gaussian_draw_bf16(O_ch, monkeypatch):
    xs, want, _ = _gaussian_decode_against_oracle(O_ch, "bf16", monkeypatch)
    within = float(((xs - want).abs() < 5e-2).float().mean())
    print(f"Gaussian draw bf16 O={O_ch}: steps within 5e-2 {within:.3f}")
    assert within >= 0.95


# ---- 3. the draw is the parameters' draw --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist,O_ch", [("Logistic", 30), ("Normal", 30), ("Normal", 2)])
def test_scalar_coop_draw_is_the_sampler_kernel_on_the_returned_parameters(dist, O_ch, monkeypatch):
    """wae_dmol_sample / wae_mog_sample on the returned parameters and the same draws give the returned samples bit for bit."""
    from wavenet_autoencoders_amd import _lib as L
    eng, cfg, sd, ins, ocfg = _model_S("fp32", monkeypatch, O_ch=O_ch, dist=dist)
    T = 40
    c_up = torch.from_numpy(load_npz("ar_S")["c_up"])[:, :, :T].contiguous().cuda()
    B = c_up.shape[0]
    M = 1 if O_ch == 2 else O_ch // 3
    u_mix, u_log, zn = (t.cuda() for t in _draws(B, T, M))
    kw = dict(u_mix=u_mix, u_log=u_log, log_scale_min=-7.0) if dist == "Logistic" else dict(u_mix=u_mix if M > 1 else None, z=zn)
    out = _decode(eng, c_up, ins["g"].cuda(), T, mode="sample", c_is_upsampled=True, want_logits=True, **kw)
    params = out["logits"].contiguous()
    assert params.shape == (B, O_ch, T)
    again = torch.empty(B, T, device="cuda")
    if dist == "Logistic":
        L.check(L.lib().wae_dmol_sample(L.ptr(params), L.ptr(u_mix), L.ptr(u_log), L.ptr(again), B, M, T, -7.0, 0, None), "dmol_sample")
    else:
        L.check(L.lib().wae_mog_sample(L.ptr(params), L.ptr(u_mix) if M > 1 else None, L.ptr(zn), L.ptr(again), B, O_ch, T, None),
                "mog_sample")
    torch.cuda.synchronize()
    assert float(out["x"].abs().max()) <= 1.0 and float(out["x"].abs().max()) > 0.0
    assert torch.equal(again, out["x"]), float((again - out["x"]).abs().max())


# ---- 4. / 5. feedback wiring and partial forcing ------------------------------------------------------------------------------------
def _one_cu_parameters(dtype, monkeypatch, c_up, g, inputs):
    """The one-CU kernel (an engine without the opt-in), teacher-forced on `inputs` (B, T)."""
    ref, *_ = _model_S(dtype, monkeypatch, scalar_coop=False)
    T = inputs.shape[1]
    out = _decode(ref, c_up, g, T, mode="logits", test_inputs=inputs.contiguous(), c_is_upsampled=True, cooperative=False)
    return out["logits"].cpu()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scalar_coop_feeds_back_the_sample_it_drew(dtype, monkeypatch):
    """A free-running cooperative decode; the one-CU kernel teacher-forced on [0, x[:-1]] computes the same parameters."""
    eng, cfg, sd, ins, ocfg = _model_S(dtype, monkeypatch)
    T = 40
    c_up = torch.from_numpy(load_npz("ar_S")["c_up"])[:, :, :T].contiguous().cuda()
    g = ins["g"].cuda()
    u_mix, u_log, _ = (t.cuda() for t in _draws(c_up.shape[0], T, 10, salt=520))
    out = _decode(eng, c_up, g, T, mode="sample", c_is_upsampled=True, want_logits=True, u_mix=u_mix, u_log=u_log, log_scale_min=-7.0)
    xs = out["x"]
    assert float(xs.std()) > 0.0
    fed = torch.cat([torch.zeros_like(xs[:, :1]), xs[:, :-1]], dim=1)
    want = _one_cu_parameters(dtype, monkeypatch, c_up, g, fed)
    err = rel_err(out["logits"].cpu(), want)
    print(f"feedback wiring {dtype}: rel err {err:.3e}")
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scalar_coop_partial_teacher_forcing(dtype, monkeypatch):
    """n_forced = 5 of T = 40: steps 0..4 are the fully forced decode's bit for bit, later steps consume the drawn samples."""
    eng, cfg, sd, ins, ocfg = _model_S(dtype, monkeypatch)
    T, nf = 40, 5
    c_up = torch.from_numpy(load_npz("ar_S")["c_up"])[:, :, :T].contiguous().cuda()
    g = ins["g"].cuda()
    x = ins["x"][:, 0, :T].contiguous().cuda()
    u_mix, u_log, _ = (t.cuda() for t in _draws(c_up.shape[0], T, 10, salt=540))
    full = _decode(eng, c_up, g, T, mode="logits", test_inputs=x, c_is_upsampled=True)["logits"]
    part = _decode(eng, c_up, g, T, mode="sample", test_inputs=x, n_forced=nf, c_is_upsampled=True, want_logits=True,
                   u_mix=u_mix, u_log=u_log, log_scale_min=-7.0)
    assert torch.equal(part["logits"][:, :, :nf], full[:, :, :nf])
    # from step nf on the input of step t is the sample drawn at t - 1, not test_inputs[t]
    fed = torch.cat([x[:, :nf], part["x"][:, nf - 1:-1]], dim=1)
    assert float((fed[:, nf:] - x[:, nf:]).abs().max()) > 1e-3
    want = _one_cu_parameters(dtype, monkeypatch, c_up, g, fed)
    err = rel_err(part["logits"].cpu()[:, :, nf:], want[:, :, nf:])
    print(f"partial forcing {dtype}: rel err of the free steps {err:.3e}")
    assert err < TOL[dtype]


# ---- 6. reproducibility -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", ["Logistic", "Normal"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_scalar_coop_sampled_decode_is_reproducible(dtype, dist, monkeypatch):
    eng, cfg, sd, ins, ocfg = _model_S(dtype, monkeypatch, dist=dist)
    T = 64
    c_up = torch.from_numpy(load_npz("ar_S")["c_up"])[:, :, :T].contiguous().cuda()
    u_mix, u_log, zn = (t.cuda() for t in _draws(c_up.shape[0], T, 10, salt=560))
    kw = dict(u_mix=u_mix, u_log=u_log, log_scale_min=-7.0) if dist == "Logistic" else dict(u_mix=u_mix, z=zn)
    runs = [_decode(eng, c_up, ins["g"].cuda(), T, mode="sample", c_is_upsampled=True, want_logits=True, **kw) for _ in range(2)]
    assert torch.equal(runs[0]["x"], runs[1]["x"]) and torch.equal(runs[0]["logits"], runs[1]["logits"])


# ---- 7. the reference's decoder geometry with a scalar head, through the oracle ------------------------------------------------------
REF_CFG = dict(layers=20, stacks=2, R=256, G=256, S=256, O=30, Cc=64, Cg=32, k=3, n_speakers=7, upsample_scales=None, cin_pad=0,
               scalar_input=True)


@pytest.mark.parametrize("dtype,B", [("fp32", 1), ("fp32", 8), ("bf16", 1), ("bf16", 8), ("fp16", 1)])
def test_scalar_coop_reference_sized_decoder_against_oracle(dtype, B, monkeypatch):
    sd = O.make_state_dict(dict(REF_CFG), salt=5, with_encoder=False)
    eng = _engine(REF_CFG, sd, dtype, monkeypatch)
    T = 64
    x = O.hash_fill((B, T), 601) * 0.9
    c = O.hash_fill((B, REF_CFG["Cc"], T), 602)
    gid = torch.arange(B) % REF_CFG["n_speakers"]
    out = _decode(eng, c.cuda(), gid.cuda(), T, mode="logits", test_inputs=x.cuda(), c_is_upsampled=True)
    with torch.no_grad():
        want = O.incremental_forward(sd, dict(layers=REF_CFG["layers"], stacks=REF_CFG["stacks"], upsample_scales=None, cin_pad=0), c, gid, T,
                                     test_inputs=x.unsqueeze(1), mode="logits")
    err = rel_err(out["logits"].cpu(), want)
    print(f"reference-sized decoder {dtype} B={B}: rel err {err:.3e}")
    assert np.isfinite(err) and err < TOL[dtype]


# ---- 8. fall-back -------------------------------------------------------------------------------------------------------------------
def test_scalar_coop_falls_back_to_one_cu_beyond_eight_utterances(monkeypatch):
    eng, cfg, sd, ins, ocfg = _model_S("fp32", monkeypatch)
    ref, *_ = _model_S("fp32", monkeypatch, scalar_coop=False)
    B, T = 9, 32
    c_up = O.hash_fill((B, cfg["Cc"], T), 701).cuda()
    gid = (torch.arange(B) % cfg["n_speakers"]).cuda()
    u_mix, u_log, _ = (t.cuda() for t in _draws(B, T, 10, salt=720))
    kw = dict(mode="sample", c_is_upsampled=True, want_logits=True, u_mix=u_mix, u_log=u_log, log_scale_min=-7.0, cooperative=False)
    a = _decode(eng, c_up, gid, T, **kw)
    b = _decode(ref, c_up, gid, T, **kw)
    assert torch.equal(a["x"], b["x"]) and torch.equal(a["logits"], b["logits"])
    # ... and eight utterances of the same call do take the cooperative path
    _decode(eng, c_up[:8].contiguous(), gid[:8], T, mode="sample", c_is_upsampled=True, u_mix=u_mix[:8].contiguous(),
            u_log=u_log[:8].contiguous(), log_scale_min=-7.0)
