"""Streaming decode on the GPU: a decode in resumable launches (wae_ar_desc.t0 > 0 continues from the caller's history ring;
WaeEngine / WaveNet / VQVAE.incremental_stream, synthesis.py --stream-chunk) is BITWISE the one-shot decode of the same arguments, on
every decode kernel: one CU (class ids, scalar logistic, scalar Gaussian), the any-shape cooperative kernel (class ids on 32 / 8 / 3
members, scalar dist 0 / 1) and the constant-size cooperative kernel at the reference's geometry (bf16, fp32; resident and streaming
weights).  The chunk list [1, 7, 1024, 1025, 503] has a single-step chunk, a chunk shorter than the largest dilation, and boundaries
on both sides of a wrap of the longest ring (2 * 512 + 1 rows)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2560
CHUNKS = [1, 7, 1024, 1025, 503]
# 20 layers in 2 stacks (dilations 1 .. 512), speaker and local conditioning; narrow, so that the any-shape kernels run it
SMALL = dict(layers=20, stacks=2, R=64, G=64, S=64, O=64, Cc=16, Cg=8, k=3, n_speakers=7, upsample_scales=None, cin_pad=0)
# the reference's decoder (hps/vqwae.json): the constant-size cooperative kernel
REF = dict(layers=20, stacks=2, R=256, G=256, S=256, O=256, Cc=64, Cg=32, k=3, n_speakers=153, upsample_scales=[4, 4, 8, 5], cin_pad=0)


def _engine(cfg, dtype, monkeypatch=None, coop="1", members=None, sd=None, salt=7, **path):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    if monkeypatch is not None:
        monkeypatch.setenv("WAE_AR_COOP", coop)
        if members is not None:
            monkeypatch.setenv("WAE_AR_COOP_C", str(members))
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    if path:
        eng.ar_path(**path)
    eng.load_state_dict(sd if sd is not None else O.make_state_dict(dict(cfg), salt=salt, with_encoder=False))
    return eng


def _cat(items):
    items = list(items)
    out = {}
    for k in items[0]:
        out[k] = None if items[0][k] is None else torch.cat([it[k] for it in items], dim=-1)
    return out, [next(v for v in it.values() if v is not None).shape[-1] for it in items]


def _same(eng, c, gid, chunks=CHUNKS, n=T, **kw):
    """stream == one-shot, bit for bit, in every returned array; returns the one-shot result"""
    if not eng.g.scalar_input and eng.g.O <= 127:
        kw.setdefault("init_idx", eng.g.O // 2 - 1)                    # (the default start class, 127, needs more classes)
    one = eng.incremental_forward(c, gid, n, **kw)
    one = {k: (None if v is None else v.clone()) for k, v in one.items()}
    got, lens = _cat(eng.incremental_stream(c, gid, n, chunks, **kw))
    torch.cuda.synchronize()
    assert lens == (list(chunks) if not isinstance(chunks, int) else [min(chunks, n - t) for t in range(0, n, chunks)])
    assert set(got) == set(one)
    for k, v in one.items():
        assert (v is None) == (got[k] is None), k
        if v is not None:
            assert got[k].shape == v.shape and got[k].dtype == v.dtype, k
            assert torch.equal(got[k], v), (k, kw.get("mode"), "first difference at", (got[k] != v).nonzero()[:1].tolist())
    return one


def _class_inputs(cfg, B, seed=5):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randn(B, cfg["Cc"], T, generator=gen).cuda()
    gid = torch.randint(0, cfg["n_speakers"], (B,), generator=gen).cuda()
    uni = torch.rand(B, T, generator=gen).cuda()
    forced = torch.randint(0, cfg["O"], (B, T), generator=gen).cuda()
    return c, gid, uni, forced


def _three_modes(eng, cfg, B, up=True):
    c, gid, uni, forced = _class_inputs(cfg, B)
    kw = dict(c_is_upsampled=True) if up else {}
    if not up:
        c = torch.randn(B, 64, T // 640, generator=torch.Generator().manual_seed(9)).cuda()
    s = _same(eng, c, gid, mode="sample", uniforms=uni, want_logits=True, **kw)
    assert int(torch.unique(s["idx"]).numel()) > cfg["O"] // 4          # a real roll-out, not a constant
    _same(eng, c, gid, mode="argmax", want_logits=True, init_idx=cfg["O"] // 2 - 1, **kw)
    _same(eng, c, gid, mode="logits", test_inputs=forced, **kw)


# ---- class ids ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_cu_class_ids(dtype, monkeypatch):
    _three_modes(_engine(SMALL, dtype, monkeypatch, coop="0"), SMALL, 2)


def test_one_cu_nine_utterances(monkeypatch):
    """more than 8 utterances decode one per CU whatever WAE_AR_COOP says"""
    eng = _engine(SMALL, "fp32", monkeypatch, coop="1")
    c, gid, uni, forced = _class_inputs(SMALL, 9)
    _same(eng, c, gid, mode="sample", uniforms=uni, want_logits=True, c_is_upsampled=True)
    assert getattr(eng, "_ar_profile", None) is None                    # (the cooperative paths leave their error / profile words)


@pytest.mark.parametrize("members", [32, 8, 3])
def test_any_shape_cooperative_kernel(members, monkeypatch):
    eng = _engine(SMALL, "fp32" if members != 8 else "bf16", monkeypatch, members=members)
    _three_modes(eng, SMALL, 2)
    assert eng._ar_profile is not None


@pytest.mark.parametrize("split", [{}, dict(lds_layers=0, reg_layers=0)], ids=["resident", "streaming"])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_constant_size_cooperative_kernel(dtype, split, monkeypatch):
    eng = _engine(REF, dtype, monkeypatch, **split)
    _three_modes(eng, REF, 2, up=False)
    assert eng._ar_profile is not None


def test_any_shape_kernel_on_the_reference_geometry(monkeypatch):
    eng = _engine(REF, "bf16", monkeypatch, generic=True)
    c, gid, uni, forced = _class_inputs(REF, 1)
    lat = torch.randn(1, 64, T // 640, generator=torch.Generator().manual_seed(9)).cuda()
    _same(eng, lat, gid, mode="sample", uniforms=uni, want_logits=True)


# ---- scalar-input decoders ----------------------------------------------------------------------------------------------------------
def _scalar_case(dist, O_ch, monkeypatch, coop, dtype="fp32"):
    cfg = dict(SMALL, O=O_ch, scalar_input=True, output_distribution=dist)
    eng = _engine(cfg, dtype, monkeypatch, coop="1" if coop else "0", scalar_coop=coop)
    B = 2
    gen = torch.Generator().manual_seed(11)
    c = torch.randn(B, cfg["Cc"], T, generator=gen).cuda()
    gid = torch.randint(0, cfg["n_speakers"], (B,), generator=gen).cuda()
    M = 1 if O_ch == 2 else O_ch // 3
    u_mix = (torch.rand(B, T, M, generator=gen) * (1 - 2e-5) + 1e-5).cuda()
    draws = (dict(u_mix=u_mix, u_log=(torch.rand(B, T, generator=gen) * (1 - 2e-5) + 1e-5).cuda()) if dist == "Logistic"
             else dict(z=torch.randn(B, T, generator=gen).cuda(), **(dict(u_mix=u_mix) if M > 1 else {})))
    forced = (torch.rand(B, T, generator=gen) * 2 - 1).cuda()
    s = _same(eng, c, gid, mode="sample", want_logits=True, c_is_upsampled=True, log_scale_min=-7.0, **draws)
    assert float(s["x"].std()) > 1e-3
    _same(eng, c, gid, mode="logits", test_inputs=forced, c_is_upsampled=True)
    assert (getattr(eng, "_ar_profile", None) is not None) == coop


@pytest.mark.parametrize("coop", [False, True], ids=["one_cu", "cooperative"])
def test_scalar_logistic(coop, monkeypatch):
    _scalar_case("Logistic", 30, monkeypatch, coop)


@pytest.mark.parametrize("coop", [False, True], ids=["one_cu", "cooperative"])
@pytest.mark.parametrize("O_ch", [2, 6])
def test_scalar_gaussian(O_ch, coop, monkeypatch):
    _scalar_case("Normal", O_ch, monkeypatch, coop, dtype="bf16" if O_ch == 6 else "fp32")


# ---- against the reference's own vectors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_golden_A_in_chunks(dtype, tol):
    """the tolerances of tests/test_gpu_ar.py::test_teacher_forced_equals_reference / test_greedy_rollout_bit_exact, decoded in chunks"""
    cfg, sd, ins, zm, ocfg = golden_model("A")
    z = load_npz("ar_A")
    eng = _engine(cfg, dtype, sd=sd)
    c_up = torch.from_numpy(z["c_up"]).cuda()
    Tar = c_up.shape[-1]
    got, _ = _cat(eng.incremental_stream(c_up, ins["g"].cuda(), Tar, 7, mode="logits", test_inputs=ins["x"][:, :Tar].cuda(),
                                         c_is_upsampled=True))
    torch.cuda.synchronize()
    assert rel_err(got["logits"].cpu(), z["tf_logits"]) < tol
    if dtype == "fp32":
        got, _ = _cat(eng.incremental_stream(c_up[:, :, :24].contiguous(), ins["g"].cuda(), 24, [1, 5, 11, 7], mode="argmax",
                                             init_idx=cfg["O"] // 2 - 1, c_is_upsampled=True))
        assert np.array_equal(got["idx"].cpu().numpy(), z["greedy"])


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 5e-2)])
def test_golden_S_in_chunks(dtype, tol):
    """tests/test_gpu_ar.py::test_scalar_input_decode_against_reference_vectors, decoded in chunks"""
    cfg, sd, ins, zm, ocfg = golden_model("S")
    z = load_npz("ar_S")
    eng = _engine(cfg, dtype, sd=sd)
    c_up = torch.from_numpy(z["c_up"]).cuda()
    Tar = c_up.shape[-1]
    x = ins["x"][:, 0, :Tar].contiguous().cuda()
    g = ins["g"].cuda()
    got, _ = _cat(eng.incremental_stream(c_up, g, Tar, 7, mode="logits", test_inputs=x, c_is_upsampled=True))
    torch.cuda.synchronize()
    assert rel_err(got["logits"].cpu(), z["params_tf"]) < tol
    if dtype == "fp32":
        roll, _ = _cat(eng.incremental_stream(c_up[:, :, :24].contiguous(), g, 24, [1, 5, 11, 7], mode="sample", c_is_upsampled=True,
                                              u_mix=torch.from_numpy(z["u_mix"])[:, :24].contiguous().cuda(),
                                              u_log=torch.from_numpy(z["u_log"])[:, :24].contiguous().cuda(), log_scale_min=-7.0))
        torch.cuda.synchronize()
        assert float((roll["x"].cpu() - torch.from_numpy(z["roll"])[:, 0]).abs().max()) < 1e-3


# ---- the engine's bookkeeping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["coop", "one_cu"])
@pytest.mark.parametrize("F", [1500, 1000, 2000], ids=["mid_chunk", "on_boundary", "end_of_chunk"])
def test_partial_teacher_forcing_across_chunks(F, kernel, monkeypatch):
    """test_inputs cover F steps: inside the second chunk, exactly on a boundary, and on the last step of a chunk"""
    eng = _engine(SMALL, "fp32", monkeypatch, coop="1" if kernel == "coop" else "0")
    c, gid, uni, forced = _class_inputs(SMALL, 2)
    one = _same(eng, c, gid, chunks=[1000, 1000, 560], mode="sample", uniforms=uni, test_inputs=forced[:, :F].contiguous(),
                c_is_upsampled=True)
    free = eng.incremental_forward(c, gid, T, mode="sample", uniforms=uni, init_idx=31, c_is_upsampled=True)["idx"]
    full = eng.incremental_forward(c, gid, T, mode="sample", uniforms=uni, test_inputs=forced, c_is_upsampled=True)["idx"]
    assert not torch.equal(one["idx"], free) and not torch.equal(one["idx"], full)      # forced, then free: neither of the two
    assert torch.equal(one["idx"][:, :F], full[:, :F])
    _same(eng, c, gid, chunks=[1000, 1000, 560], mode="sample", uniforms=uni, test_inputs=forced, n_forced=F, c_is_upsampled=True)


@pytest.mark.parametrize("kernel", ["coop", "one_cu"])
def test_start_class_per_utterance(kernel, monkeypatch):
    eng = _engine(SMALL, "fp32", monkeypatch, coop="1" if kernel == "coop" else "0")
    c, gid, uni, forced = _class_inputs(SMALL, 3)
    starts = torch.tensor([3, 40, 62])
    one = _same(eng, c, gid, mode="argmax", init_idx=starts, c_is_upsampled=True)
    other = eng.incremental_forward(c, gid, T, mode="argmax", init_idx=3, c_is_upsampled=True)["idx"]
    assert torch.equal(other[0], one["idx"][0]) and not torch.equal(other, one["idx"])


def test_seeded_draws_equal_the_seeded_one_shot_call(monkeypatch):
    eng = _engine(SMALL, "fp32", monkeypatch)
    c, gid, uni, forced = _class_inputs(SMALL, 2)
    torch.manual_seed(21)
    one = eng.incremental_forward(c, gid, T, mode="sample", init_idx=31, c_is_upsampled=True)["idx"].clone()
    torch.manual_seed(21)
    got, _ = _cat(eng.incremental_stream(c, gid, T, CHUNKS, mode="sample", init_idx=31, c_is_upsampled=True))
    assert torch.equal(got["idx"], one)
    for dist, O_ch in (("Logistic", 30), ("Normal", 6)):
        cfg = dict(SMALL, O=O_ch, scalar_input=True, output_distribution=dist)
        es = _engine(cfg, "fp32", monkeypatch, coop="0")
        torch.manual_seed(22)
        one = es.incremental_forward(c, gid, T, mode="sample", c_is_upsampled=True)["x"].clone()
        torch.manual_seed(22)
        got, _ = _cat(es.incremental_stream(c, gid, T, 640, mode="sample", c_is_upsampled=True))
        assert torch.equal(got["x"], one), dist


@pytest.mark.parametrize("path", ["class_one_cu", "class_coop", "scalar_logistic", "scalar_normal", "scalar_coop"])
def test_default_draws_are_made_in_the_same_order(path, monkeypatch):
    """No draws passed: after the same torch seed the one-shot call and the stream make the same draws, on every decode path"""
    coop = path in ("class_coop", "scalar_coop")
    cfg = dict(SMALL)
    if path.startswith("scalar"):
        cfg.update(O=6 if path == "scalar_normal" else 30, scalar_input=True,
                   output_distribution="Normal" if path == "scalar_normal" else "Logistic")
    eng = _engine(cfg, "fp32", monkeypatch, coop="1" if coop else "0", **(dict(scalar_coop=True) if path == "scalar_coop" else {}))
    c, gid, uni, forced = _class_inputs(SMALL, 2)
    kw = dict(mode="sample", c_is_upsampled=True, **({} if cfg.get("scalar_input") else dict(init_idx=31)))
    key = "x" if cfg.get("scalar_input") else "idx"
    eng._ar_profile = None
    torch.manual_seed(23)
    one = eng.incremental_forward(c, gid, T, **kw)[key].clone()
    torch.manual_seed(23)
    got, _ = _cat(eng.incremental_stream(c, gid, T, CHUNKS, **kw))
    assert torch.equal(got[key], one)
    assert (eng._ar_profile is not None) == coop                        # the path the case names ran
    torch.manual_seed(24)
    other = eng.incremental_forward(c, gid, T, **kw)[key]
    assert not torch.equal(other, one)                                  # (the draws matter: another seed, another roll-out)


def test_early_close_frees_the_stream_and_leaves_the_engine_usable(monkeypatch):
    eng = _engine(REF, "bf16", monkeypatch)
    c, gid, uni, forced = _class_inputs(REF, 1)
    lat = torch.randn(1, 64, T // 640, generator=torch.Generator().manual_seed(9)).cuda()
    one = eng.incremental_forward(lat, gid, T, mode="sample", uniforms=uni)["idx"].clone()
    it = eng.incremental_stream(lat, gid, T, 300, mode="sample", uniforms=uni)
    a, b = next(it), next(it)
    assert torch.equal(torch.cat([a["idx"], b["idx"]], 1), one[:, :600])
    it.close()
    with pytest.raises(StopIteration):
        next(it)
    assert eng._ar_keep is None
    again = eng.incremental_forward(lat, gid, T, mode="sample", uniforms=uni)["idx"]
    assert torch.equal(again, one)
    # ... and a second stream on the same engine starts from an empty ring
    got, _ = _cat(eng.incremental_stream(lat, gid, T, 1600, mode="sample", uniforms=uni))
    assert torch.equal(got["idx"], one)


def test_refusals_before_any_launch(monkeypatch):
    eng = _engine(REF, "bf16", monkeypatch)
    lat = torch.randn(1, 64, 1, device="cuda")
    gid = torch.zeros(1, dtype=torch.int64, device="cuda")
    for mode in ("probs", "raw"):
        with pytest.raises(ValueError):
            next(iter(eng.incremental_stream(lat, gid, 640, 160, mode=mode)))
    for chunk in (0, -3, [320, 0, 320], [320, 160]):
        with pytest.raises(ValueError):
            next(iter(eng.incremental_stream(lat, gid, 640, chunk, mode="argmax")))
    eng.ar_path(one_handover=True)
    with pytest.raises(ValueError):
        next(iter(eng.incremental_stream(lat, gid, 640, 160, mode="argmax")))
    eng.ar_path()
    assert sum(it["idx"].shape[1] for it in eng.incremental_stream(lat, gid, 640, 160, mode="argmax")) == 640


# ---- modules and the script ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scalar", [False, True], ids=["one_hot", "scalar"])
def test_vqvae_module_stream_equals_incremental_forward(scalar):
    from wavenet_autoencoders_amd.vqvae_model import VQVAE
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    torch.manual_seed(3)
    kw = dict(scalar_input=True, out_channels=30) if scalar else dict(out_channels=256)
    wn = WaveNet(layers=6, stacks=2, residual_channels=32, gate_channels=64, skip_out_channels=32, cin_channels=16, gin_channels=8,
                 n_speakers=5, use_speaker_embedding=True, upsample_conditional_features=True,
                 upsample_params={"upsample_scales": [4, 4, 5]}, **kw)
    v = VQVAE(c_in=39, hid=16, K=32, wavenet=wn, encoder_hid=32).cuda().eval()
    feats = torch.randn(2, 39, 32, device="cuda")
    g = torch.tensor([1, 4], device="cuda")
    Tn = 8 * 80                                                        # 32 frames -> 8 latent frames x 80
    torch.manual_seed(31)
    one = v.incremental_forward(None, feats, g, Tn, True, True, None, -7.0)
    torch.manual_seed(31)
    parts = list(v.incremental_stream(None, feats, g, Tn, True, True, None, -7.0, chunk=[1, 100, 300, 239]))
    assert [p.shape[-1] for p in parts] == [1, 100, 300, 239]
    assert all(p.shape[:2] == one.shape[:2] and p.dtype == one.dtype for p in parts)
    assert one.shape == ((2, 1, Tn) if scalar else (2, 256, Tn))
    assert torch.equal(torch.cat(parts, -1), one)


@pytest.mark.parametrize("scalar", [False, True], ids=["one_hot", "scalar"])
def test_wavenet_module_stream_equals_incremental_forward(scalar):
    from wavenet_autoencoders_amd.wavenet_vocoder import WaveNet
    torch.manual_seed(4)
    kw = dict(scalar_input=True, out_channels=30) if scalar else dict(out_channels=256)
    wn = WaveNet(layers=6, stacks=2, residual_channels=32, gate_channels=64, skip_out_channels=32, cin_channels=16, gin_channels=-1,
                 **kw).cuda().eval()
    Tn = 500
    c = torch.randn(2, 16, Tn, device="cuda")
    torch.manual_seed(32)
    one = wn.incremental_forward(c=c, T=Tn)
    torch.manual_seed(32)
    parts = list(wn.incremental_stream(c=c, T=Tn, chunk=77))
    assert [p.shape[-1] for p in parts] == [77] * 6 + [38]
    assert torch.equal(torch.cat(parts, -1), one)
    if not scalar:
        # fully teacher-forced, quantize=False: the softmax rows of every step
        one = wn.incremental_forward(c=c, T=Tn, test_inputs=one, quantize=False)
        got = torch.cat(list(wn.incremental_stream(c=c, T=Tn, test_inputs=torch.cat(parts, -1), quantize=False, chunk=[250, 250])), -1)
        assert torch.equal(got, one)
        with pytest.raises(ValueError):
            next(iter(wn.incremental_stream(c=c, T=Tn, quantize=False, chunk=77)))      # free-running dense feedback stays on chip


HP = ("layers=4,residual_channels=32,gate_channels=64,skip_out_channels=32,encoder_hid=32,cin_channels=16,gin_channels=8,"
      "n_speakers=5,batch_size=2,max_time_steps=2560,checkpoint_interval=1000")


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def _tiny_dump_and_checkpoint(tmp_path):
    """the dump of tests/test_gpu_scripts.py (the reference's on-disk format), one train step for a checkpoint, one test utterance"""
    rng = np.random.default_rng(5)
    dump = tmp_path / "dump"
    lines = []
    for u in range(3):
        d = dump / "train_no_dev" / f"utt{u}"
        d.mkdir(parents=True)
        n = 40 + 4 * u
        np.save(d / "wave.npy", rng.integers(0, 256, n * 160).astype(np.int16))
        np.save(d / "mfcc.norm.npy", rng.standard_normal((n, 39)).astype(np.float32))
        lines.append(f"utt{u}|{n}|{u}|dummy")
    (dump / "train_no_dev" / "train.txt").write_text("\n".join(lines) + "\n")
    preset = os.path.join(ROOT, "hps", "vqwae.json")
    ck = tmp_path / "ck"
    _run([os.path.join(ROOT, "vqwae_train.py"), "--dump-root", str(dump), "--checkpoint-dir", str(ck), "--preset", preset,
          "--hparams", HP, "--max-steps", "1", "--dtype", "fp32"], str(tmp_path))
    utt = dump / "test" / "S0_0007"
    utt.mkdir(parents=True)
    np.save(utt / "mfcc.norm.npy", rng.standard_normal((16, 39)).astype(np.float32))
    (tmp_path / "syn.txt").write_text("test/S0_0007 V1\n")
    (tmp_path / "spk.json").write_text(json.dumps({"V1": 2}))
    return dump, ck / "checkpoint_latest.pth", preset


def test_synthesis_script_writes_the_same_wav_with_stream_chunk(tmp_path):
    from scipy.io import wavfile
    dump, ckpt, preset = _tiny_dump_and_checkpoint(tmp_path)
    wavs, outs = [], []
    for dst, extra in (("one/", []), ("chunked/", ["--stream-chunk", "700"])):
        outs.append(_run([os.path.join(ROOT, "synthesis.py"), str(dump), str(ckpt), dst, str(tmp_path / "syn.txt"),
                          str(tmp_path / "spk.json"), "english", "160", "25", "0", "--preset", preset, "--hparams", HP, "--seed", "7"] + extra,
                         str(tmp_path)))
        sr, y = wavfile.read(tmp_path / dst.rstrip("/") / "2019" / "english" / "test" / "V1_0007.wav")
        assert sr == 16000 and y.shape == (16 * 160,) and float(np.abs(y).max()) > 0
        wavs.append(y)
    assert np.array_equal(wavs[0], wavs[1])
    assert "first audio: 700 samples after" in outs[1] and "first audio" not in outs[0]
