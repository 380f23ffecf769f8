"""List encoding on the GPU (fp32): wae_enc_conv_fwd_list bit for bit against wae_enc_conv_fwd per segment, WaeEngine.encode_list bit
for bit against the loop of encoder_forward + vq_forward, pinned to the reference's fixture and to the oracle, independent of grouping
and order, and the callers (inference_2019.encode_features_list, VQVAE.encode_list) against their one-utterance forms."""
import functools

import numpy as np
import pytest
import torch

from helpers import golden_model, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3                                  # tests/test_gpu_parity.py:40-41: latents norm-wise, indices equal
FS = [1, 2, 3, 4, 5, 37, 128, 129, 131]
TOUTS = [1, 7, 8, 9, 31, 32, 33, 65]
SLACK, SENTINEL = 16, -12345.5


# ---- 1. the raw entry ------------------------------------------------------------------------------------------------------------------
def _tin(tout, k, stride, pad):
    """the ODD input length under stride 2, else the only one, that gives tout outputs"""
    tin = (tout - 1) * stride + k - 2 * pad
    assert (tin + 2 * pad - k) // stride + 1 == tout and (stride == 1 or tin % 2 == 1)
    return tin


@pytest.mark.parametrize("et", [8, 16, 32])
@pytest.mark.parametrize("k,stride,pad,conv_in", [(1, 1, 0, False), (3, 1, 1, False), (5, 2, 2, False), (5, 1, 2, False), (3, 1, 0, True)])
def test_entry_is_bit_for_bit_the_single_call_per_segment(k, stride, pad, conv_in, et):
    from wavenet_autoencoders_amd import _lib as L
    from wavenet_autoencoders_amd import packing as PK
    lib, dev = L.lib(), "cuda"
    gen = torch.Generator().manual_seed(1000 * k + 100 * stride + 10 * pad + et)
    Tin = [_tin(t, k, stride, pad) for t in TOUTS]
    segs, tiles, _, Tout = PK.enc_list_tables(Tin, k, stride, pad, et)
    assert list(Tout) == TOUTS
    in_pitch, out_pitch = sum(Tin) + 5, sum(TOUTS) + SLACK
    segs_d, tiles_d = torch.from_numpy(segs).to(dev), torch.from_numpy(tiles).to(dev)
    same = stride == 1 and 2 * pad == k - 1
    shapes = [(ci, co, 0) for ci in (39, 256, 300) for co in (40, 64)]
    if same:                                     # residual is legal on a same-shape conv only: Cin == Cout
        shapes += [(40, 40, 1), (64, 64, 1), (300, 300, 1)]
    for Cin, Cout, residual in shapes:
        # neighbours differ by 1e3 in scale: a read across a segment boundary cannot hide; the pitch's slack holds 1e6
        x = torch.full((Cin, in_pitch), 1e6)
        o = 0
        for j, t in enumerate(Tin):
            x[:, o:o + t] = torch.randn(Cin, t, generator=gen) * (1e3 if j % 2 else 1.0)
            o += t
        w = torch.randn(Cout, Cin, k, generator=gen) / (Cin * k) ** 0.5
        b = None if conv_in else torch.randn(Cout, generator=gen)
        x_d, w_d, b_d = x.to(dev), w.to(dev), (None if b is None else b.to(dev))
        for relu in ((0,) if conv_in else (0, 1)):
            y = torch.full((Cout, out_pitch), SENTINEL, device=dev)
            L.check(lib.wae_enc_conv_fwd_list(L.ptr(x_d), L.ptr(w_d), L.ptr(b_d), L.ptr(y), L.ptr(segs_d), len(segs), L.ptr(tiles_d),
                                              len(tiles), et, in_pitch, out_pitch, Cin, Cout, k, stride, pad, relu, residual, None),
                    "enc_conv_fwd_list")
            for (io, ti, oo, to) in segs.tolist():
                xs = x_d[:, io:io + ti].contiguous()
                ref = torch.full((Cout, to), SENTINEL, device=dev)
                L.check(lib.wae_enc_conv_fwd(L.ptr(xs), L.ptr(w_d), L.ptr(b_d), L.ptr(ref), 1, Cin, ti, Cout, k, stride, pad, relu, residual,
                                             None), "enc_conv_fwd")
                assert torch.equal(y[:, oo:oo + to], ref), (Cin, Cout, relu, residual, to)
                assert not (ref == SENTINEL).any()
            torch.cuda.synchronize()
            assert (y[:, sum(TOUTS):] == SENTINEL).all(), (Cin, Cout, relu, residual)       # the slack columns come back untouched


# ---- 2.-4. encode_list ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _setup():
    """engine on the weights of golden_model("A"), the list's items, and the LOOP's answer per item, computed once"""
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    cfg, sd, ins, z, _ = golden_model("A")
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype="fp32")
    eng.load_state_dict(sd)
    eng.prepare_weights()
    c = ins["c"]
    items = [c[b, :, :min(F, c.shape[-1])].contiguous() for b in range(c.shape[0]) for F in FS]
    # the fixture is 8 frames long; utterances of the list's real lengths (more than one tile, odd lengths under the strided blocks)
    gen = torch.Generator().manual_seed(7)
    items += [torch.randn(cfg["c_in"], F, generator=gen) * 1.7 for F in FS]
    loop = [_loop(eng, it) for it in items]
    return eng, cfg, sd, ins, z, items, loop


def _loop(eng, item):
    lat = eng.encoder_forward(item[None].cuda())
    quant, idx, _ = eng.vq_forward(lat)
    return dict(latents=lat[0].clone(), quant=quant[0].clone(), idx=idx.clone())


def _same(got, want):
    for key in ("latents", "quant", "idx"):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        assert torch.equal(got[key], want[key]), key


def test_encode_list_is_bit_for_bit_the_loop():
    eng, cfg, _, _, _, items, loop = _setup()
    res = eng.encode_list(items, want_latents=True)
    assert len(res) == len(items)
    for it, got, want in zip(items, res, loop):
        assert got["quant"].shape == (cfg["Cc"], (it.shape[1] - 1) // 4 + 1) and got["idx"].dtype == torch.int64
        _same(got, want)
    # host arrays and device tensors, mixed, are the same list; what is not asked for is None
    mixed = [it.numpy() if i % 3 == 0 else it.cuda() if i % 3 == 1 else it for i, it in enumerate(items)]
    for got, want in zip(eng.encode_list(mixed), loop):
        assert got["latents"] is None and torch.equal(got["quant"], want["quant"]) and torch.equal(got["idx"], want["idx"])
    assert all(r["idx"] is None for r in eng.encode_list(items[:3], want_idx=False))


def test_encode_list_is_pinned_to_the_reference():
    eng, cfg, sd, ins, z, _, loop = _setup()
    c = ins["c"]
    res = eng.encode_list([c[b] for b in range(c.shape[0])], want_latents=True)
    lat = torch.stack([r["latents"] for r in res]).cpu()
    err = rel_err(lat, z["latents"])
    print(f"full-length items: latents rel err {err:.3e} against the fixture")
    assert err < FP32_TOL
    assert np.array_equal(torch.cat([r["idx"] for r in res]).cpu().numpy(), z["vq_idx"])
    # a truncated item against the oracle on the same slice; its indices against the loop only (the oracle may break a near-tie
    # the other way)
    cut = c[1, :, :5].contiguous()
    got = eng.encode_list([c[0], cut], want_latents=True)[1]
    with torch.no_grad():
        want_lat = O.encoder_forward(sd, cut[None])[0]
        want_q = O.vqvae_encode(sd, cut[None])[0]
    err = rel_err(got["latents"].cpu(), want_lat)
    print(f"truncated item: latents rel err {err:.3e} against the oracle")
    assert err < FP32_TOL and got["quant"].shape == want_q.shape
    _same(got, _loop(eng, cut))


def test_encode_list_does_not_depend_on_grouping_or_order():
    eng, _, _, _, _, items, loop = _setup()
    back = eng.encode_list(items[::-1], want_latents=True)[::-1]
    for got, want in zip(back, loop):
        _same(got, want)
    from wavenet_autoencoders_amd import packing as PK
    synth = items[-len(FS):]                                          # 1 + 2 + 3 + 4 + 5 + 37 + 128 + 129 + 131 = 440 frames
    groups = PK.encode_list_groups([it.shape[1] for it in synth], 180)
    assert len(groups) == 3, groups
    for got, want in zip(eng.encode_list(synth, want_latents=True, max_frames=180), loop[-len(FS):]):
        _same(got, want)


# ---- 5. the callers ---------------------------------------------------------------------------------------------------------------------
def test_inference_script_list_form_equals_its_loop():
    import inference_2019 as inf
    eng, _, _, _, _, items, _ = _setup()
    feats = [np.ascontiguousarray(it.numpy().T) for it in items[-len(FS):] + items[:4]]          # (N_i, c_in), as the .npy files
    got = inf.encode_features_list(eng, feats)
    assert len(got) == len(feats)
    for f, g in zip(feats, got):
        want = inf.encode_features(eng, f)
        assert g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want)


def test_inference_script_batches_write_the_loop_s_files(tmp_path, monkeypatch):
    """process_batch over batches of 3 (a short last one) against process_utterance per entry: the same paths, the same bytes"""
    import inference_2019 as inf
    eng, _, _, _, _, items, _ = _setup()
    monkeypatch.chdir(tmp_path)                                                                   # base_dir has six '/'-separated parts
    scp = []
    for i, it in enumerate(items[-len(FS):][2:9]):                                                # 7 utterances of 3 .. 131 frames
        base = f"db/x/english/test/utt{i}/"
        (tmp_path / base).mkdir(parents=True)
        np.save(base + "mfcc.norm.npy", np.ascontiguousarray(it.numpy().T))
        scp.append([f"utt{i}", base])
    want = [inf.process_utterance(base, "mfcc.norm", eng, "loop/") for _, base in scp]
    got = [p for entries in inf.batches(scp, 3) for p in inf.process_batch(entries, "mfcc.norm", eng, "list/")]
    assert [p[len("list/"):] for p in got] == [p[len("loop/"):] for p in want] and len(got) == 7
    for p, q in zip(got, want):
        assert open(p, "rb").read() == open(q, "rb").read()


def test_vqvae_module_encode_list_equals_encode():
    from test_gpu_modules import _build
    _, cfg, sd, _, _, items, _ = _setup()
    model, _ = _build(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    xs = items[-len(FS):] + items[:4]
    got = model.encode_list([x.cuda() for x in xs])
    assert len(got) == len(xs)
    for x, q in zip(xs, got):
        assert torch.equal(q, model.encode(x[None].cuda())[0])
