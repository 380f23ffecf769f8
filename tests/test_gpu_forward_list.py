"""The teacher-forced forward of a LIST of utterances of unequal lengths on the GPU (include/wae.h: wae_glu_layer_fwd_list,
wae_nll_segments; WaeEngine.decoder_forward_list / forward_list): every item bit for bit its own batch-1 forward, whatever the
order and the grouping; rows no item owns untouched; records that do not fit skipped; launches that do not grow with the list."""
import ctypes
import json
import types

import numpy as np
import pytest
import torch

from helpers import golden_model, load_npz, rel_err
from oracle import wae_oracle as O

pytestmark = pytest.mark.gpu

LENGTHS = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 700]
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DT = {"fp32": 0, "bf16": 1, "fp16": 2}
RP = 128
SENTINEL = 7.0


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _engine(cfg, sd, dtype):
    from wavenet_autoencoders_amd import Geometry
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = WaeEngine(Geometry.from_cfg(cfg), dtype=dtype)
    eng.load_state_dict(sd)
    return eng


# ---------------------------------------------------------------------------------------------------------------- one layer
class Layer:
    """One gated layer on random operands (the packed weights are an opaque fragment stream: any values serve a bitwise comparison
    of the two entries).  The arrays carry a margin of rows in front and behind, so that no table of these tests -- the out-of-contract
    ones included -- could take even a wrong kernel outside an allocation."""
    MARGIN = 1024

    def __init__(self, dtype, Hp, Ccp, rows, nzb, seed=0):
        from wavenet_autoencoders_amd import _lib as L
        self.L, self.lib = L, L.lib()
        self.dtype, self.dt, self.td = dtype, DT[dtype], TDT[dtype]
        self.Hp, self.Ccp, self.rows, self.nzb = Hp, Ccp, rows, nzb
        self.Ku, self.ucol = Hp + 64, 32
        gen = torch.Generator().manual_seed(1000 + seed)
        M = self.MARGIN
        desc = L.GluDesc(self.dt, 1, 1, RP, Ccp, Hp, 3, 1, 0)
        nbytes = self.lib.wae_glu_packed_bytes(ctypes.byref(desc))
        assert nbytes > 0
        es = 2 if self.dt else 4
        self.w = (torch.randn(nbytes // es, generator=gen) * 0.05).to(self.td).cuda()
        self.bias = (torch.randn(RP, generator=gen) * 0.1).cuda()
        self.zb_all = (torch.randn(nzb + 2, 2 * Hp, generator=gen) * 0.3).cuda()       # one spare row at either end
        self.x_all = torch.randn(rows + 2 * M, RP, generator=gen).to(self.td).cuda()
        self.c_all = torch.randn(rows + 2 * M, max(Ccp, 1), generator=gen).to(self.td).cuda() if Ccp else None
        self.x = self.x_all[M:M + rows]
        self.c = self.c_all[M:M + rows] if Ccp else None
        self.zb = self.zb_all[1:1 + nzb]

    def outputs(self):
        M = self.MARGIN
        xo = torch.full((self.rows + 2 * M, RP), SENTINEL, dtype=self.td, device="cuda")
        uo = torch.full((self.rows + 2 * M, self.Ku), SENTINEL, dtype=self.td, device="cuda")
        return xo, uo

    def _uptr(self, uo, row):
        return ctypes.c_void_p(uo.data_ptr() + ((self.MARGIN + row) * self.Ku + self.ucol) * uo.element_size())

    def run_list(self, table, nsegs, ntiles, dil, flags, x=None, c=None, rows=None, nzb=None):
        """-> (x_out, u_out) with their margins, prefilled with the sentinel"""
        L, M = self.L, self.MARGIN
        xo, uo = self.outputs()
        x = self.x if x is None else x
        c = self.c if c is None else c
        tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).cuda()
        d = L.GluDesc(self.dt, self.nzb if nzb is None else nzb, 0, RP, self.Ccp, self.Hp, 3, dil, flags)
        rc = self.lib.wae_glu_layer_fwd_list(ctypes.byref(d), L.ptr(tab), nsegs, ntiles, self.rows if rows is None else rows, L.ptr(x),
                                             ctypes.c_void_p(xo.data_ptr() + M * RP * xo.element_size()), L.ptr(c) if self.Ccp else None,
                                             self._uptr(uo, 0), self.Ku, L.ptr(self.zb), 2 * self.Hp, L.ptr(self.w), L.ptr(self.bias),
                                             None)
        L.check(rc, "glu_layer_fwd_list")
        torch.cuda.synchronize()
        return xo, uo

    def run_dense(self, off, T, zrow, dil, flags):
        """the dense entry with B = 1 on the rows [off, off + T) alone -> (x_out (T, Rp), u_out (T, Ku))"""
        L = self.L
        xo = torch.full((T, RP), SENTINEL, dtype=self.td, device="cuda")
        uo = torch.full((T, self.Ku), SENTINEL, dtype=self.td, device="cuda")
        xs = self.x[off:off + T].clone()
        cs = self.c[off:off + T].clone() if self.Ccp else None
        d = L.GluDesc(self.dt, 1, T, RP, self.Ccp, self.Hp, 3, dil, flags)
        L.check(self.lib.wae_glu_layer_fwd(ctypes.byref(d), L.ptr(xs), L.ptr(xo), L.ptr(cs) if self.Ccp else None,
                                           ctypes.c_void_p(uo.data_ptr() + self.ucol * uo.element_size()), self.Ku,
                                           L.ptr(self.zb[zrow]), 2 * self.Hp, None, L.ptr(self.w), L.ptr(self.bias), None), "glu_layer_fwd")
        torch.cuda.synchronize()
        return xo, uo


def _layout():
    """LENGTHS with gaps between some segments -> (offsets, rows)"""
    offs, at = [], 3
    for i, T in enumerate(LENGTHS):
        offs.append(at)
        at += T + (i % 3) * 5
    return offs, at + 4


@pytest.mark.parametrize("Hp", [32, 64, 96, 128, 192, 256])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_list_entry_is_the_dense_entry_per_segment(dtype, Hp):
    from wavenet_autoencoders_amd import packing as P
    offs, rows = _layout()
    n = len(LENGTHS)
    zrows = list(reversed(range(n)))                   # an item's zb row is the table's, not its index
    tile = P.GLU_LIST_TILES[DT[dtype]]
    plan = P.glu_list_plan(LENGTHS, tile, offsets=offs, zb_rows=zrows)
    owned = torch.zeros(rows, dtype=torch.bool)
    for o, T in zip(offs, LENGTHS):
        owned[o:o + T] = True
    for Ccp in (64, 0):
        ly = Layer(dtype, Hp, Ccp, rows, n, seed=Hp + Ccp)
        M = ly.MARGIN
        # rows of the inputs that no segment owns are NaN from the start: nothing may read them
        gaps = (~owned).cuda()
        ly.x[gaps] = float("nan")
        if Ccp:
            ly.c[gaps] = float("nan")
        for dil, flags in ((1, 0), (2, 0), (512, 0), (2, 4)):          # 4 = WAE_GLU_NO_OUT, the last layer
            xo, uo = ly.run_list(plan.table, n, plan.ntiles, dil, flags)
            # rows outside every segment, the margins and the columns of u beside the layer's: untouched
            keep = torch.ones(rows + 2 * M, dtype=torch.bool)
            keep[M:M + rows] = ~owned
            assert bool((xo[keep.cuda()] == SENTINEL).all()) and bool((uo[keep.cuda()] == SENTINEL).all())
            assert bool((uo[:, :ly.ucol] == SENTINEL).all()) and bool((uo[:, ly.ucol + Hp:] == SENTINEL).all())
            if flags & 4:
                assert bool((xo == SENTINEL).all())
            for i, (o, T) in enumerate(zip(offs, LENGTHS)):
                xd, ud = ly.run_dense(o, T, zrows[i], dil, flags)
                assert _same(xo[M + o:M + o + T], xd), (dtype, Hp, Ccp, dil, flags, T, "x_out")
                assert _same(uo[M + o:M + o + T], ud), (dtype, Hp, Ccp, dil, flags, T, "u_out")
        # every row outside the segment under test NaN: the segment's rows do not change (dilation 512 against items shorter than
        # 512: every earlier tap is the item's own zero pad, and the neighbour lies exactly there)
        xo, uo = ly.run_list(plan.table, n, plan.ntiles, 512, 0)
        for i in (1, 4, 7, 9, 10):
            o, T = offs[i], LENGTHS[i]
            x2 = torch.full_like(ly.x, float("nan"))
            x2[o:o + T] = ly.x[o:o + T]
            c2 = None
            if Ccp:
                c2 = torch.full_like(ly.c, float("nan"))
                c2[o:o + T] = ly.c[o:o + T]
            xo2, uo2 = ly.run_list(plan.table, n, plan.ntiles, 512, 0, x=x2, c=c2)
            assert _same(xo2[M + o:M + o + T], xo[M + o:M + o + T]) and _same(uo2[M + o:M + o + T], uo[M + o:M + o + T]), (dtype, Hp, T)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_records_that_do_not_fit_are_skipped(dtype):
    """Out-of-contract tables: the kernel ignores the record, writes nothing for it and reports no error.  Every table here keeps even
    a kernel that did NOT skip inside the allocations (Layer's margins; `rows` and the zb row count are passed smaller than what is
    allocated)."""
    from wavenet_autoencoders_amd import packing as P
    tile = P.GLU_LIST_TILES[DT[dtype]]
    rows, nzb = 1500, 2
    ly = Layer(dtype, 64, 64, rows, nzb, seed=3)
    M = ly.MARGIN
    good = [10, 300, 1, 0]                                    # {row_off, T, zb_row, tile0}
    gt = -(-300 // tile)
    ref_x, ref_u = ly.run_list([good, [0, 0, 0, gt]], 1, gt, 2, 0)
    assert not bool((ref_x[M + 10:M + 310] == SENTINEL).all())
    bad = {
        "T = 0": ([400, 0, 0, gt], 1),
        "T < 0": ([400, -5, 0, gt], 1),
        "row_off < 0": ([-3, 100, 0, gt], 1),
        "row_off + T > rows": ([1450, 100, 0, gt], 1),
        "zb_row < 0": ([400, 100, -1, gt], 1),
        "zb_row = B": ([400, 100, nzb, gt], 1),
        "too many tiles": ([400, 100, 0, gt], 2),
        "too few tiles": ([400, 2 * tile + 1, 0, gt], 2),
    }
    for what, (rec, ntile) in bad.items():
        table = [good, rec, [0, 0, 0, gt + ntile]]
        xo, uo = ly.run_list(table, 2, gt + ntile, 2, 0)
        assert _same(xo, ref_x) and _same(uo, ref_u), what                   # the good record as before, the sentinel everywhere else
        rec0 = list(rec)
        rec0[3] = 0
        for alone in (rec0, rec):             # the bad record alone; and with a tile0 above every tile of the grid
            xo, uo = ly.run_list([alone, [0, 0, 0, ntile]], 1, ntile, 2, 0)
            assert bool((xo == SENTINEL).all()) and bool((uo == SENTINEL).all()), what


# ---------------------------------------------------------------------------------------------------------------- the engine
DEC = dict(layers=10, stacks=1, R=32, G=32, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], cin_pad=0)
DEC_T = [1, 129, 300, 257, 1100]


def _dec_items(cfg, Ts, salt=0):
    items = []
    for i, T in enumerate(Ts):
        x = ((O.hash_fill((T,), 100 + salt + i) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
        items.append(dict(x=x, c=O.hash_fill((cfg["Cc"], T), 200 + salt + i, 1.0), gid=(2 * i + 1) % cfg["n_speakers"]))
    return items


def _alone(eng, it):
    """decoder_forward of the item as a batch of one -> (logits (O, T), nll (T,)) clones"""
    x = it["x"][None].cuda()
    out = eng.decoder_forward(x, it["c"][None].cuda(), torch.tensor([it["gid"]]).cuda(), targets=x, c_is_upsampled=True)
    torch.cuda.synchronize()
    return out["logits"][0].clone(), out["nll"][0].clone()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_decoder_forward_list_items_are_their_single_forwards(dtype):
    sd = O.make_state_dict(dict(DEC), salt=9, with_encoder=False)
    eng = _engine(DEC, sd, dtype)
    items = _dec_items(DEC, DEC_T)
    single = [_alone(eng, it) for it in items]
    runs = {}
    for name, order, kw in (("given", list(range(5)), {}), ("reversed", [4, 3, 2, 1, 0], {}), ("groups", list(range(5)), dict(max_rows=600))):
        if name == "groups":
            from wavenet_autoencoders_amd import packing as P
            assert len(P.forward_list_groups(DEC_T, 600)) == 3
        res, loss = eng.decoder_forward_list([items[i] for i in order], c_is_upsampled=True, **kw)
        torch.cuda.synchronize()
        eng.check_errors()
        sums = [None] * 5
        for r, i in zip(res, order):
            lg, nl = single[i]
            assert _same(r["logits"], lg), (dtype, name, i, "logits")
            assert _same(r["nll"], nl), (dtype, name, i, "nll")
            assert int(r["count"]) == DEC_T[i] - 1 and float(r["nll"][-1]) == 0.0
            sums[i] = r["nll_sum"].clone()
        runs[name] = torch.stack(sums)
        tot = sum(float(single[i][1].double().sum()) for i in range(5))
        ref = tot / sum(T - 1 for T in DEC_T)
        print(f"{dtype} {name}: loss {float(loss):.7f}, float64 of the returned nll {ref:.7f}")
        assert abs(float(loss) - ref) <= 1e-4 * abs(ref)
    assert _same(runs["given"], runs["reversed"]) and _same(runs["given"], runs["groups"])
    assert float(runs["given"][0]) == 0.0                       # T = 1: nothing to predict


def test_list_refusals_come_before_any_launch():
    sd = O.make_state_dict(dict(DEC), salt=9, with_encoder=False)
    eng = _engine(DEC, sd, "bf16")
    items = _dec_items(DEC, [5, 9])
    calls = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self._lib, name)

    eng.prepare_weights()
    eng.lib = Counting(eng.lib)
    with pytest.raises(ValueError):
        eng.decoder_forward_list([], c_is_upsampled=True)
    with pytest.raises(ValueError):
        eng.decoder_forward_list([items[0], dict(items[1], x=items[1]["x"][:0])], c_is_upsampled=True)
    with pytest.raises(ValueError):
        eng.decoder_forward_list([items[0], dict(items[1], c=items[1]["c"][:, :-1])], c_is_upsampled=True)
    with pytest.raises(ValueError):
        eng.decoder_forward_list(items)                          # (Cc, T) features do not upsample to T by 640
    with pytest.raises(ValueError):
        eng.decoder_forward_list([items[0], dict(items[1], gid=None)], c_is_upsampled=True)
    assert calls == []


def test_the_static_schedule_geometry():
    """hps/vqwae.json's decoder in bf16: the single forward runs the static-schedule layer kernel (csrc/glu_fwd_static.hip, bit-identical
    to the generic kernel by its own contract), the list the generic list kernel."""
    cfg = json.loads(str(load_npz("model_vqwae_probe")["cfg"]))
    sd = O.make_state_dict(cfg, 4)
    eng = _engine(cfg, sd, "bf16")
    items = []
    for i, T in enumerate((300, 1100)):
        x = ((O.hash_fill((T,), 300 + i) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
        items.append(dict(x=x, c=O.hash_fill((cfg["Cc"], T), 310 + i, 1.0), gid=7 + i))
    res, _ = eng.decoder_forward_list(items, c_is_upsampled=True)
    for r, it in zip(res, items):
        lg, nl = _alone(eng, it)
        assert _same(r["logits"], lg) and _same(r["nll"], nl)


SMALL = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
             c_in=39, K=32, cin_pad=0)
# 5, 8 and 20 feature frames (T = 1280, 1280, 3200 at scales [4, 4, 8, 5] behind the encoder's stride of 4).  The issue's 4 frames for
# the shortest item do not show the contrast below on the oracle: the padded batch moves that item's one latent by 0.49 and it still
# quantises to the same code of this 32-entry codebook; at 5 frames its second latent changes code (9 -> 21).
FRAMES = [5, 8, 20]


def _full_items(cfg, frames=FRAMES):
    items = []
    for i, F in enumerate(frames):
        T = -(-F // 4) * 640
        x = ((O.hash_fill((T,), 50 + i) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
        items.append(dict(x=x, feats=O.hash_fill((cfg["c_in"], F), 40 + i, 1.7), gid=(i + 1) % cfg["n_speakers"]))
    return items


def _padded(items, cfg):
    Fm, Tm = max(it["feats"].shape[1] for it in items), max(it["x"].numel() for it in items)
    c = torch.zeros(len(items), cfg["c_in"], Fm)
    x = torch.zeros(len(items), Tm, dtype=torch.long)
    for i, it in enumerate(items):
        c[i, :, :it["feats"].shape[1]] = it["feats"]
        x[i, :it["x"].numel()] = it["x"]
    return x, c


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_forward_list_items_are_their_single_forwards(dtype):
    sd = O.make_state_dict(SMALL, 1)
    eng = _engine(SMALL, sd, dtype)
    items = _full_items(SMALL)
    res, loss = eng.forward_list(items)
    torch.cuda.synchronize()
    emb = sd["vq.embedding.weight"]
    for r, it in zip(res, items):
        x = it["x"][None].cuda()
        out = eng.forward(x, it["feats"][None].cuda(), torch.tensor([it["gid"]]).cuda(), targets=x)
        torch.cuda.synchronize()
        assert torch.equal(r["idx"], out["idx"])
        assert _same(r["quant"], out["quant"][0]) and _same(r["latents"], out["latents"][0])
        assert _same(r["logits"], out["logits"][0]) and _same(r["nll"], out["nll"][0])
        with torch.no_grad():
            assert torch.equal(r["idx"].cpu(), O.vq_forward(emb, O.encoder_forward(sd, it["feats"][None]))[3])
    # why the list form exists: the zero-padded dense batch of the same items is another function at the utterance ends -- on the
    # oracle alone (the encoder's pad frames stop being zero behind the first block), and so on the GPU
    xp, cp = _padded(items, SMALL)
    with torch.no_grad():
        idx_pad = O.vq_forward(emb, O.encoder_forward(sd, cp))[3].view(len(items), -1)
    Tq0 = res[0]["idx"].numel()
    assert not torch.equal(idx_pad[0, :Tq0], res[0]["idx"].cpu())
    out = eng.forward(xp.cuda(), cp.cuda(), torch.tensor([it["gid"] for it in items]).cuda())
    torch.cuda.synchronize()
    assert not torch.equal(out["quant"][0][:, :Tq0], res[0]["quant"])


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-3), ("bf16", 5e-2), ("fp16", 1e-2)])
def test_forward_list_against_the_oracle(dtype, tol):
    cfg, sd, ins, z, ocfg = golden_model("A")
    eng = _engine(cfg, sd, dtype)
    items = []
    for i, F in enumerate((4, 12)):
        T = -(-F // 4) * int(np.prod(cfg["upsample_scales"]))
        x = ((O.hash_fill((T,), 60 + i) * 0.5 + 0.5) * cfg["O"]).long().clamp(0, cfg["O"] - 1)
        items.append(dict(x=x, feats=O.hash_fill((cfg["c_in"], F), 70 + i, 1.7), gid=i + 1))
    res, _ = eng.forward_list(items, want_nll=not cfg.get("scalar_input"))
    torch.cuda.synchronize()
    for r, it in zip(res, items):
        xin = torch.nn.functional.one_hot(it["x"][None], cfg["O"]).float().transpose(1, 2).contiguous()
        with torch.no_grad():
            y_ref, _, _, aux = O.vqvae_forward(sd, ocfg, xin, it["feats"][None], torch.tensor([it["gid"]]))
        assert torch.equal(r["idx"].cpu(), aux["idx"])
        err = rel_err(r["logits"].cpu(), y_ref[0])
        print(f"{dtype}: T {it['x'].numel()}: logits against the oracle, rel err {err:.3e}")
        assert err < tol


def test_launches_do_not_grow_with_the_list(monkeypatch):
    sd = O.make_state_dict(dict(DEC), salt=9, with_encoder=False)
    eng = _engine(DEC, sd, "bf16")
    eng.prepare_weights()
    counts = {}

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            counts[name] = counts.get(name, 0) + 1
            return getattr(self._lib, name)

    eng.lib = Counting(eng.lib)
    for name in ("empty", "zeros", "from_numpy"):                # the allocations and the table uploads
        def counted(*a, _f=getattr(torch, name), _n="torch." + name, **k):
            counts[_n] = counts.get(_n, 0) + 1
            return _f(*a, **k)
        monkeypatch.setattr(torch, name, counted)
    per_list = []
    for n in (3, 12):
        items = _dec_items(DEC, [40 + 13 * i for i in range(n)])
        counts.clear()
        eng.decoder_forward_list(items, c_is_upsampled=True)
        per_list.append(dict(counts))
    torch.cuda.synchronize()
    assert per_list[0] == per_list[1], per_list
    c = per_list[0]
    assert c["wae_glu_layer_fwd_list"] == DEC["layers"] and c["wae_first_conv_fwd"] == 1 and c["wae_gproj_fwd"] == 1
    assert c["wae_nll_segments"] == 1 and c.get("wae_glu_layer_fwd_drop", 0) == 0 and c.get("wae_glu_layer_fwd", 0) == 0
    assert c["torch.from_numpy"] == 2                            # the stack's table and upsample_list's


def test_dev_packed_scores_the_utterances_alone():
    """vqwae_train.evaluate(packed=True) on a padded batch of three utterances: sum nll_sum / sum count over their batch-1 forwards"""
    import vqwae_train
    sd = O.make_state_dict(SMALL, 1)
    eng = _engine(SMALL, sd, "bf16")
    items = _full_items(SMALL, [4, 8, 20])          # whole latent frames: T_i = 160 F_i, as the dumps' utterances
    xp, cp = _padded(items, SMALL)
    lengths = torch.tensor([it["x"].numel() for it in items])
    gid = torch.tensor([it["gid"] for it in items])
    hp = types.SimpleNamespace(max_time_steps=None, hop_size=160, cin_pad=0, quantize_channels=64, log_scale_min=-7.0)
    got = vqwae_train.evaluate(eng, [(xp, cp, gid, lengths)], "cuda:0", hp, packed=True)[0]
    tot = cnt = 0.0
    for it in items:
        x = it["x"][None].cuda()
        out = eng.forward(x, it["feats"][None].cuda(), torch.tensor([it["gid"]]).cuda(), targets=x, want_logits=False)
        tot += float(out["nll"][0].double().sum())
        cnt += it["x"].numel() - 1
    print(f"--dev-packed loss {got:.7f}, batch-1 forwards {tot / cnt:.7f}")
    assert abs(got - tot / cnt) <= 1e-4 * abs(tot / cnt)
