"""GPU: the mixture-of-Gaussians output distribution (output_distribution "Normal", reference mixture.py:161-270) through every
layer -- the loss / sampler kernels against the reference's own outputs (tests/golden/mog.npz), teacher-forced decoder gradients
and the train step against autograd through the oracle and the restatement tests/mog_ref.py, the Gaussian draw of the persistent
autoregressive kernel, the module surface and the training script on a dump of float waves."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mog_ref
from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(O_ch, dtype, dist="Normal"):
    """Golden model S (scalar input, O = 30) or its O = 2 variant (same sizes, closed-form weights), as an engine."""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, ins, z, ocfg = golden_model("S")
    cfg = dict(cfg, output_distribution=dist)
    if O_ch != cfg["O"]:
        cfg["O"] = O_ch
        sd = O.make_state_dict(cfg, int(z["salt"]))
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd)
    return eng, cfg, sd, ins, z, ocfg


@pytest.mark.parametrize("C", [2, 3, 30])
def test_loss_gradient_and_sampler_kernels_against_reference(C):
    from wavenet_autoencoders_amd import _lib as L
    from wavenet_autoencoders_amd.losses import MixtureGaussianLoss
    from wavenet_autoencoders_amd.wavenet_vocoder.mixture import mix_gaussian_loss, sample_from_mix_gaussian
    z = load_npz("mog")
    lsm = float(z["log_scale_min"])
    y_hat = torch.from_numpy(z[f"y_hat_{C}"]).cuda()
    y = torch.from_numpy(z[f"y_{C}"]).cuda()
    per = mix_gaussian_loss(y_hat, y, log_scale_min=lsm, reduce=False)
    yg = y_hat.clone().requires_grad_(True)
    tot = mix_gaussian_loss(yg, y, log_scale_min=lsm, reduce=True)
    tot.backward()
    torch.cuda.synchronize()
    assert per.shape == (y_hat.shape[0], y_hat.shape[2], 1)
    assert rel_err(per.cpu(), z[f"loss_{C}"]) < 1e-5
    assert abs(float(tot.detach()) - float(z[f"sum_{C}"])) < 1e-5 * abs(float(z[f"sum_{C}"]))
    assert rel_err(yg.grad.cpu(), z[f"grad_{C}"]) < 1e-5
    # the sampler kernel on the reference's own draws
    B, _, T = y_hat.shape
    um = torch.from_numpy(z[f"u_mix_{C}"]).cuda() if f"u_mix_{C}" in z else None
    zn = torch.from_numpy(z[f"z_{C}"]).cuda()
    out = torch.empty(B, T, device="cuda")
    L.check(L.lib().wae_mog_sample(L.ptr(y_hat), L.ptr(um), L.ptr(zn), L.ptr(out), B, C, T, None), "mog_sample")
    torch.cuda.synchronize()
    assert rel_err(out.cpu(), z[f"samp_{C}"]) < 1e-5
    # the module API: a device draw in [-1, 1]; the masked criterion of vqwae_train.py:404-422
    s = sample_from_mix_gaussian(y_hat, log_scale_min=lsm)
    assert s.shape == (B, T) and float(s.abs().max()) <= 1.0 and bool(torch.isfinite(s).all())
    lengths = torch.tensor([T, T - 5])
    crit = MixtureGaussianLoss(log_scale_min=lsm)(y_hat, y, lengths=lengths.cuda())
    mask = (torch.arange(T).unsqueeze(0) < lengths.unsqueeze(1)).float().unsqueeze(-1)
    want = (torch.from_numpy(z[f"loss_{C}"]) * mask).sum() / mask.sum()
    assert abs(float(crit) - float(want)) < 1e-5 * abs(float(want))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("O_ch", [30, 2])
def test_teacher_forced_mog_gradients(O_ch, dtype):
    """eng.mog_loss_and_grad + decoder_backward with ragged lengths against autograd through the oracle's forward and the
    masked restatement (the tolerances of test_scalar_input_dmol_backward_fp32; bf16 those of test_decoder_backward_bf16_is_close)."""
    from wavenet_autoencoders_amd import backward as BW
    eng, cfg, sd, ins, z, ocfg = _model(O_ch, dtype)
    x, g = ins["x"][:, 0, :].contiguous(), ins["g"]
    B, T = x.shape
    c_up = torch.from_numpy(z["c_up"])
    lengths = torch.tensor([T, T - 97])
    psd = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("wavenet.") and "upsample_net" not in k}
    y = O.wavenet_forward(psd, dict(ocfg, upsample_scales=None), ins["xin"], c_up, g)
    assert y.shape[1] == O_ch
    loss = mog_ref.masked_mog_loss(y, x.unsqueeze(-1), lengths, -7.0)
    loss.backward()
    out = eng.decoder_forward(x.cuda(), c_up.cuda(), g.cuda(), train=True, c_is_upsampled=True, want_logits=True)
    got_loss, dyt = eng.mog_loss_and_grad(out["logits"], x.cuda(), lengths.cuda(), -7.0)
    BW.decoder_backward(eng, x.cuda(), None, lengths, g.cuda(), ext_dy=dyt)
    grads = BW.finish_grads(eng)
    torch.cuda.synchronize()
    fp32 = dtype == "fp32"
    assert abs(float(got_loss) - float(loss)) < (1e-4 if fp32 else 3e-2) * max(1.0, abs(float(loss))), (float(got_loss), float(loss))
    bad = {}
    for k, v in psd.items():
        gref = v.grad if v.grad is not None else torch.zeros_like(v)
        got = grads[eng.lay.off(k):eng.lay.off(k) + eng.lay.numel(k)].view(eng.lay.shapes[k]).cpu()
        err, ref = float((got - gref).abs().max()), float(gref.abs().max())
        if err > (1e-3 if fp32 else 8e-2) * max(ref, 1e-6) + (1e-7 if fp32 else 1e-6):
            bad[k] = (err, ref)
    assert not bad, bad


def test_train_step_reports_the_gaussian_loss():
    """With output_distribution "Normal" the train step's loss is the MoG loss of the oracle on the same weights (not the DMoL one)."""
    eng, cfg, sd, ins, z, ocfg = _model(30, "fp32")
    x, c, g = ins["x"][:, 0, :].contiguous(), ins["c"], ins["g"]
    B, T = x.shape
    with torch.no_grad():
        y, vq, _, _ = O.vqvae_forward(sd, ocfg, ins["xin"], c, g)
        full = torch.full((B,), T)
        want = float(mog_ref.masked_mog_loss(y, x.unsqueeze(-1), full, -7.0))
        dmol = float(O.masked_dmol_loss(y, x.unsqueeze(-1), full, 65536, -7.0))
    r = eng.train_step(x.cuda(), c.cuda(), g.cuda(), lengths=None, lr=2e-3, quantize_channels=65536, log_scale_min=-7.0)
    torch.cuda.synchronize()
    got = float(r["ce"])
    assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (got, want)
    assert abs(got - dmol) > 1e-2 * max(1.0, abs(dmol)), (got, dmol)
    assert abs(float(r["loss"]) - (want + float(vq))) < 1e-4 * max(1.0, abs(want + float(vq)))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("O_ch", [30, 2])
def test_train_step_learns(O_ch, dtype):
    eng, cfg, sd, ins, z, ocfg = _model(O_ch, dtype)
    x, c, g = ins["x"][:, 0, :].contiguous().cuda(), ins["c"].cuda(), ins["g"].cuda()
    losses = []
    for _ in range(6):
        r = eng.train_step(x, c, g, lengths=None, lr=2e-3, log_scale_min=-7.0)
        losses.append(float(r["ce"]))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in losses), losses
    assert bool(torch.isfinite(eng.params).all()) and np.isfinite(float(r["grad_norm"]))
    assert losses[-1] < losses[0], losses


def _gumbel_margin(params, u_mix):
    """Top-1 minus top-2 Gumbel score of every step (inf for one Gaussian)."""
    M, _, _ = mog_ref.layout(params.shape[1])
    if M == 1:
        return torch.full((params.shape[0], params.shape[2]), float("inf"))
    sc = (params.transpose(1, 2)[..., :M] - torch.log(-torch.log(u_mix))).double()
    top = sc.topk(2, dim=-1)[0]
    return top[..., 0] - top[..., 1]


def _decode_against_oracle(O_ch, dtype, T=40):
    eng, cfg, sd, ins, zm, ocfg = _model(O_ch, dtype)
    z = load_npz("ar_S")
    c_up = torch.from_numpy(z["c_up"])[:, :, :T].contiguous()
    g = ins["g"]
    B = c_up.shape[0]
    M = 1 if O_ch == 2 else O_ch // 3
    u_mix = (O.hash_fill((B, T, M), 501) * 0.5 + 0.5).clamp(1e-5, 1 - 1e-5)
    zn = O.hash_fill((B, T), 502) * 1.7
    out = eng.incremental_forward(c_up.cuda(), g.cuda(), T, mode="sample", c_is_upsampled=True,
                                  u_mix=u_mix.cuda() if M > 1 else None, z=zn.cuda())
    torch.cuda.synchronize()
    xs = out["x"].cpu()
    assert xs.shape == (B, T) and float(xs.abs().max()) <= 1.0
    # teacher-force the oracle on the start value 0 followed by the produced samples: the mixture parameters of every step
    ti = torch.cat([torch.zeros(B, 1), xs[:, :-1]], dim=1).unsqueeze(1)
    params = O.incremental_forward(sd, dict(ocfg, upsample_scales=None), c_up, g, T, test_inputs=ti, mode="logits")
    want = mog_ref.mog_sample(params, u_mix if M > 1 else None, zn)
    return xs, want, _gumbel_margin(params, u_mix)


@pytest.mark.parametrize("O_ch", [30, 2])
def test_autoregressive_gaussian_draw_fp32(O_ch):
    xs, want, margin = _decode_against_oracle(O_ch, "fp32")
    diff = (xs - want).abs()
    off = diff > 1e-4
    # a step may draw another mixture only where two Gumbel scores tie within rounding (cf. test_gpu_ar.py's categorical draws)
    assert bool((margin[off] < 1e-3).all()), (diff.max(), margin[off])
    assert float(off.float().mean()) <= 0.05


@pytest.mark.parametrize("O_ch", [30, 2])
def test_autoregressive_gaussian_draw_bf16(O_ch):
    xs, want, _ = _decode_against_oracle(O_ch, "bf16")
    assert float(((xs - want).abs() < 5e-2).float().mean()) >= 0.95


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_logistic_decode_is_bitwise_unchanged(dtype):
    """The Logistic draw of the same persistent kernel: bit for bit the roll-out and step parameters the build before the Gaussian
    branch returned (tests/golden/ar_S_logistic_roll.npz, recorded from it on the same inputs)."""
    eng, cfg, sd, ins, zm, ocfg = _model(30, dtype, dist="Logistic")
    z = load_npz("ar_S")
    rec = load_npz("ar_S_logistic_roll")
    c_up = torch.from_numpy(z["c_up"]).cuda()
    T = c_up.shape[-1]
    roll = eng.incremental_forward(c_up, ins["g"].cuda(), T, mode="sample", c_is_upsampled=True,
                                   u_mix=torch.from_numpy(z["u_mix"]).cuda(), u_log=torch.from_numpy(z["u_log"]).cuda(),
                                   log_scale_min=-7.0, want_logits=True)
    torch.cuda.synchronize()
    assert np.array_equal(roll["x"].cpu().numpy(), rec[f"x_{dtype}"])
    assert np.array_equal(roll["logits"].cpu().numpy(), rec[f"params_{dtype}"])


def test_module_incremental_forward_normal():
    """WaveNet(scalar_input=True, output_distribution="Normal") and VQVAE decode with the reference's shapes, samples in [-1, 1]."""
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    torch.manual_seed(3)
    w = WaveNet(out_channels=30, layers=4, stacks=2, residual_channels=32, gate_channels=64, skip_out_channels=32, cin_channels=16,
                gin_channels=-1, scalar_input=True, output_distribution="Normal").cuda().eval()
    c = torch.randn(2, 16, 50, device="cuda")
    y = w.incremental_forward(c=c, T=50)
    assert y.shape == (2, 1, 50) and float(y.abs().max()) <= 1.0 and bool(torch.isfinite(y).all())
    w2 = WaveNet(out_channels=2, layers=4, stacks=2, residual_channels=32, gate_channels=64, skip_out_channels=32, cin_channels=-1,
                 gin_channels=-1, scalar_input=True, output_distribution="Normal").cuda().eval()
    y2 = w2.incremental_forward(T=30)
    assert y2.shape == (1, 1, 30) and float(y2.abs().max()) <= 1.0
    wv = WaveNet(out_channels=30, layers=4, stacks=2, residual_channels=32, gate_channels=64, skip_out_channels=32, cin_channels=16,
                 gin_channels=-1, scalar_input=True, output_distribution="Normal", upsample_conditional_features=True,
                 upsample_params={"upsample_scales": [4, 4]})
    v = VQVAE(c_in=39, hid=16, K=32, wavenet=wv, encoder_hid=32).cuda().eval()
    feats = torch.randn(1, 39, 8, device="cuda")
    yv = v.incremental_forward(None, feats, None, 32, True, True, None, -7.0)
    assert yv.shape[0] == 1 and yv.shape[1] == 1 and float(yv.abs().max()) <= 1.0 and bool(torch.isfinite(yv).all())


HP = ("layers=4,residual_channels=32,gate_channels=64,skip_out_channels=32,encoder_hid=32,cin_channels=16,gin_channels=8,"
      "n_speakers=5,batch_size=2,max_time_steps=2560,checkpoint_interval=1000,input_type=raw,out_channels=30,"
      "output_distribution=Normal,log_scale_min=-7.0")


def test_train_script_on_float_waves_with_gaussian_output(tmp_path):
    rng = np.random.default_rng(6)
    dump = tmp_path / "dump"
    lines = []
    for u in range(3):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 40 + 4 * u
        np.save(d / "wave.npy", (0.3 * np.sin(np.arange(n * 160) * (0.05 + 0.01 * u)) + 0.05 * rng.standard_normal(n * 160))
                .astype(np.float32))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    ck = tmp_path / "ck"
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(ck),
                        "--preset", os.path.join(ROOT, "hps", "vqwae.json"), "--hparams", HP + ",train_eval_interval=2",
                        "--max-steps", "3", "--dtype", "fp32"], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = p.stdout
    assert "Finished" in out and "Eval at train step 2" in out
    line = [ln for ln in out.splitlines() if ln.startswith("step 1 loss")][0]
    assert np.isfinite(float(line.split()[3])), line
    for f in ("checkpoint_step000000003.pth", "checkpoint_latest.pth", "hparams.json"):
        assert (ck / f).exists(), f
    from scipy.io import wavfile
    sr, y = wavfile.read(ck / "intermediate" / "train_no_dev_eval" / "step000000002_predicted.wav")
    assert y.shape == (2560,) and float(np.abs(y.astype(np.float64)).max()) > 0
    # synthesis.py decodes the scalar model with its Gaussian draw (wavegen, synthesis.py:370-394)
    short = dump / "test" / "S0_0007"
    short.mkdir(parents=True)
    np.save(short / "mfcc.norm.npy", rng.standard_normal((7, 39)).astype(np.float32))
    (tmp_path / "syn.txt").write_text("test/S0_0007 V1\n")
    (tmp_path / "spk.json").write_text('{"V1": 2}')
    p = subprocess.run([sys.executable, os.path.join(ROOT, "synthesis.py"), str(dump), str(ck / "checkpoint_latest.pth"), "wav/",
                        str(tmp_path / "syn.txt"), str(tmp_path / "spk.json"), "english", "160", "25", "0", "--preset",
                        os.path.join(ROOT, "hps", "vqwae.json"), "--hparams", HP], cwd=str(tmp_path), env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    sr, y = wavfile.read(tmp_path / "wav" / "2019" / "english" / "test" / "V1_0007.wav")
    assert y.shape == (8 * 160,) and np.isfinite(y).all() and float(np.abs(y).max()) > 0
