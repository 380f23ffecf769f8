"""The teacher-forced forward of a list, without a GPU: the host plan (packing.glu_list_plan, forward_list_groups), the numpy
restatement of wae_nll_segments against float64, the ABI of the new entries and their refusals before any launch, and the contracts of
the list kernels' ISA (csrc/obj/glu_fwd_list.s: no spills in the 16-bit instantiations, no instruction on a register with a load in
flight)."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_asm_contracts_cpu as contracts
from wavenet_autoencoders_amd import packing as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 127, 128, 129, 255, 256, 257, 700]
EINVAL, EUNSUPPORTED = -1, -2
PTR = ctypes.c_void_p(0x1000)


# ---------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("tile", [128, 256])
def test_the_tiles_of_an_item_cover_it_exactly_once(tile):
    plan = P.glu_list_plan(LENGTHS, tile)
    rec = plan.table
    assert rec.dtype == np.int32 and rec.shape == (len(LENGTHS) + 1, 4)
    per = [-(-T // tile) for T in LENGTHS]
    assert list(rec[:-1, 3]) == [sum(per[:i]) for i in range(len(per))]          # tile0: the running sum
    assert rec[-1, 3] == sum(per) == plan.ntiles                                   # the closing record holds the tile count
    assert list(rec[:-1, 1]) == LENGTHS and list(rec[:-1, 2]) == list(range(len(LENGTHS)))
    assert list(rec[:-1, 0]) == [sum(LENGTHS[:i]) for i in range(len(LENGTHS))] == list(plan.offsets)
    assert plan.rows == sum(LENGTHS)
    # tile by tile, as the kernel reads the table: the record of tile j, its columns, and what they cover
    cover = [np.zeros(T, dtype=np.int64) for T in LENGTHS]
    for j in range(plan.ntiles):
        i = int(np.searchsorted(rec[:, 3], j, side="right")) - 1
        k = j - rec[i, 3]
        assert 0 <= i < len(LENGTHS) and k * tile < LENGTHS[i]
        cover[i][k * tile:min((k + 1) * tile, LENGTHS[i])] += 1
    assert all((c == 1).all() for c in cover)


def test_the_callers_row_offsets_and_zb_rows():
    offs = [5000, 0, 300, 2000, 3000, 4000, 1000, 6000]
    zrows = [3, 1, 0, 2, 7, 6, 5, 4]
    plan = P.glu_list_plan(LENGTHS, 256, offsets=offs, zb_rows=zrows)
    assert list(plan.table[:-1, 0]) == offs and list(plan.table[:-1, 2]) == zrows
    assert plan.rows == 6000 + 700
    for bad in ([], [3, 0, 5], [3, -1]):
        with pytest.raises(ValueError):
            P.glu_list_plan(bad, 256)
    with pytest.raises(ValueError):
        P.glu_list_plan([3, 4], 256, offsets=[0])
    with pytest.raises(ValueError):
        P.glu_list_plan([3, 4], 0)


def test_the_tile_widths_are_the_librarys():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert {dt: lib.wae_glu_list_tile(dt) for dt in (0, 1, 2)} == P.GLU_LIST_TILES
    assert lib.wae_glu_list_tile(9) == EINVAL


def test_groups_never_split_an_item():
    Ts = [100, 200, 5000, 50, 50, 50, 900, 1000, 1]
    for cap in (1, 99, 300, 1000, 1001, 10 ** 9):
        groups = P.forward_list_groups(Ts, cap)
        assert [i for lo, hi in groups for i in range(lo, hi)] == list(range(len(Ts)))        # the list back, in order
        for lo, hi in groups:
            assert hi > lo
            assert sum(Ts[lo:hi]) <= cap or hi - lo == 1                                       # an oversize item is alone
    assert P.forward_list_groups(Ts, 300)[:2] == [(0, 2), (2, 3)]
    assert P.forward_list_groups(Ts) == [(0, len(Ts))] and P.FWD_LIST_MAX_ROWS == 1 << 20
    with pytest.raises(ValueError):
        P.forward_list_groups(Ts, 0)


# ---------------------------------------------------------------------------------------------------------------- the reduction
def _f64(nll, Ts, offs):
    sums = [float(np.sum(nll[o:o + T - 1].astype(np.float64))) for o, T in zip(offs, Ts)]
    cnt = sum(T - 1 for T in Ts)
    return sums, (sum(sums) / cnt if cnt else 0.0)


def test_nll_segments_restated_against_float64():
    rng = np.random.default_rng(5)
    Ts = [700, 1, 2, 255, 256, 257, 3000]
    offs = [0, 710, 720, 730, 1000, 1300, 1600]               # gaps between some items
    plan = P.glu_list_plan(Ts, 256, offsets=offs)
    nll = rng.gamma(2.0, 2.0, plan.rows + 7).astype(np.float32)
    out, sums, cnts, loss = P.nll_segments_restated(nll, plan.table)
    ref_sums, ref_loss = _f64(nll, Ts, offs)
    assert list(cnts) == [T - 1 for T in Ts] and cnts.dtype == np.int32 and sums.dtype == np.float32
    assert sums[1] == 0.0 and cnts[1] == 0                                        # T = 1: nothing to predict
    # fp64 partial sums rounded once to fp32: half an ulp of the sum, whatever the order
    np.testing.assert_allclose(sums, ref_sums, rtol=2.0 ** -23, atol=0)
    assert abs(float(loss) - ref_loss) <= 2.0 ** -22 * ref_loss                   # fp32 sums, fp64 walk, one rounding
    # the last row of every item is 0, every other row is untouched
    last = [o + T - 1 for o, T in zip(offs, Ts)]
    assert (out[last] == 0).all()
    keep = np.ones(nll.size, dtype=bool)
    keep[last] = False
    assert np.array_equal(out[keep], nll[keep]) and nll[last].min() > 0           # (and the input was not modified)


def test_a_list_without_a_target_has_loss_zero():
    plan = P.glu_list_plan([1, 1, 1], 128)
    _, sums, cnts, loss = P.nll_segments_restated(np.ones(3, dtype=np.float32), plan.table)
    assert not sums.any() and not cnts.any() and loss == 0.0 and np.isfinite(loss)


def test_records_outside_the_rows_are_skipped_by_the_restatement():
    table = np.array([[0, 4, 0, 0], [2, 9, 1, 1], [-1, 2, 2, 2], [4, 0, 3, 3], [0, 0, 0, 4]], dtype=np.int32)
    nll = np.arange(1, 7, dtype=np.float32)
    out, sums, cnts, _ = P.nll_segments_restated(nll, table)
    assert list(sums) == [6.0, 0, 0, 0] and list(cnts) == [3, 0, 0, 0]
    assert list(out) == [1, 2, 3, 0, 5, 6]


# ---------------------------------------------------------------------------------------------------------------- the ABI
def test_the_new_entries_are_declared_and_bound():
    from wavenet_autoencoders_amd import _lib
    header = open(os.path.join(ROOT, "include", "wae.h")).read()
    lib = _lib.lib()
    for name, nargs in (("wae_glu_layer_fwd_list", 15), ("wae_glu_list_tile", 1), ("wae_nll_segments", 9)):
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in include/wae.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1])
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"typedef struct wae_glu_seg \{ int32_t row_off, T, zb_row, tile0; \} wae_glu_seg;", header)
    assert [f[0] for f in _lib.GluSeg._fields_] == ["row_off", "T", "zb_row", "tile0"] and ctypes.sizeof(_lib.GluSeg) == 16


def _glu_list(lib, desc=None, **kw):
    from wavenet_autoencoders_amd import _lib
    fields = dict(dtype=1, B=2, T=0, Rp=128, Ccp=64, Hp=128, ktaps=3, dilation=1, flags=0)
    fields.update(desc or {})
    d = _lib.GluDesc(*[fields[n] for n, _ in _lib.GluDesc._fields_])
    a = dict(segs=PTR, nsegs=2, ntiles=3, rows=600, x_in=PTR, x_out=PTR, c_up=PTR, u_out=PTR, u_stride=128, zb=PTR, zb_stride=256,
             w=PTR, bias=PTR)
    a.update(kw)
    return lib.wae_glu_layer_fwd_list(ctypes.byref(d), a["segs"], a["nsegs"], a["ntiles"], a["rows"], a["x_in"], a["x_out"], a["c_up"],
                                      a["u_out"], a["u_stride"], a["zb"], a["zb_stride"], a["w"], a["bias"], None)


@pytest.mark.parametrize("case,code", [
    (dict(desc=dict(dtype=7)), EINVAL), (dict(desc=dict(B=0)), EINVAL), (dict(desc=dict(Rp=96)), EINVAL),
    (dict(desc=dict(Ccp=32)), EINVAL), (dict(desc=dict(Hp=288)), EINVAL), (dict(desc=dict(ktaps=0)), EINVAL),
    (dict(desc=dict(dilation=0)), EINVAL), (dict(x_in=None), EINVAL), (dict(u_out=None), EINVAL), (dict(zb=None), EINVAL),
    (dict(w=None), EINVAL), (dict(x_out=None), EINVAL), (dict(bias=None), EINVAL), (dict(c_up=None), EINVAL),
    (dict(u_stride=64), EINVAL), (dict(segs=None), EINVAL), (dict(nsegs=0), EINVAL), (dict(ntiles=0), EINVAL), (dict(rows=0), EINVAL),
    (dict(desc=dict(flags=2)), EUNSUPPORTED),            # WAE_GLU_SAVE_Z: the list form is inference only
    (dict(desc=dict(Hp=160), u_stride=160), EUNSUPPORTED),             # Hp / 32 = 5 has no tiling, as in the dense entry
])
def test_the_list_entry_refuses_before_any_launch(case, code):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert _glu_list(lib, **case) == code, lib.wae_last_error()
    assert lib.wae_last_error().startswith(b"glu")


def test_nll_segments_refuses_before_any_launch():
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    ok = [PTR, PTR, 2, 100, 0, PTR, PTR, PTR, None]
    for i, bad in ((0, None), (1, None), (5, None), (6, None), (7, None), (2, 0), (3, 0), (4, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.wae_nll_segments(*args) == EINVAL
        assert lib.wae_last_error().startswith(b"nll_segments: ")


# ---------------------------------------------------------------------------------------------------------------- the ISA
LIST_KERNEL = re.compile(r"glu_fwd_kernelI\w+?Lb1EEv")          # the kernel template's last argument: LIST = true


def _list_isa():
    path = os.path.join(contracts.OBJ, "glu_fwd_list.s")
    if not os.path.exists(path):
        pytest.skip("csrc/obj has not been built")
    return path


def _metadata(text):
    """kernel symbol -> its entry of the amdhsa.kernels metadata (the YAML at the end of the ISA file), as text"""
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for entry in re.split(r"\n  - \.", meta)[1:]:
        m = re.search(r"\.name:\s+(\S+)", entry)
        if m:
            out[m.group(1)] = entry
    return out


def test_the_16bit_list_kernels_do_not_spill():
    """Read from the kernels' metadata, not the instruction stream.  (The Hp = 256 tiling needed help to get here: csrc/glu_fwd_kernel.hpp,
    NARROW; the Hp = 192 tiling, C2's, is at 239 registers.)"""
    text = open(_list_isa()).read()
    meta = _metadata(text)
    k16 = [k for k in meta if re.search(r"glu_fwd_kernelIDF16[b_]", k)]
    k32 = [k for k in meta if re.search(r"glu_fwd_kernelIfL", k)]
    assert len(k16) == 12 and len(k32) == 6, sorted(meta)          # six gate tilings x (bf16, fp16); six in fp32
    assert len(meta) == 18 and all(LIST_KERNEL.search(k) for k in meta), sorted(meta)          # LIST = true, and nothing else in this file
    for k in k16:
        field = lambda name: int(re.search(r"\." + name + r":\s+(\d+)", meta[k]).group(1))      # noqa: E731
        assert field("vgpr_spill_count") == 0 and field("private_segment_fixed_size") == 0, (k, meta[k])
        assert field("vgpr_count") <= 256, (k, meta[k])             # two waves per SIMD


def test_no_instruction_touches_a_register_with_a_load_in_flight_in_the_list_kernels():
    path = _list_isa()
    kernels = contracts._kernels16(path)
    assert len(kernels) == 12, kernels
    bad, nloads = [], 0
    for k in kernels:
        rc, out = contracts._run("check_asm_regs.py", path, k, "3")           # glu_fwd's look-ahead: requests two chunks ahead
        last = out.strip().split("\n")[-1]
        m = re.search(r"(\d+) asm loads checked, (\d+) violation", last)
        assert m, (k, out[-400:])
        nloads += int(m.group(1))
        if int(m.group(2)):
            bad.append(last)
    assert not bad, bad
    assert nloads > 0, "the scanner found no inline-asm loads at all: its patterns no longer match the ISA"


def test_the_dense_file_holds_no_list_kernel():
    path = os.path.join(contracts.OBJ, "glu_fwd.s")
    if not os.path.exists(path):
        pytest.skip("csrc/obj has not been built")
    names = sorted(_metadata(open(path).read()))
    assert len(names) == 42 and not any(LIST_KERNEL.search(k) for k in names), names
