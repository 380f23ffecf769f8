"""The front end's and the training step's host paths (wavenet_autoencoders_amd/frontend.py, train.py) without a GPU: their structure,
read off the package sources with `ast` (one launch site per list kernel, one optimizer call, one packer; nothing of it left in
engine.py), with a self-test of the walkers; the packer (pack_time) on device="cpu"; the item intake of the list calls (list_items)."""
import ast
import glob
import os
import types

import numpy as np
import pytest
import torch

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavenet_autoencoders_amd")
# the entries of the front end and the optimizer that engine.py no longer reaches: prefixes, then whole names
MOVED_PREFIXES = ("wae_enc_conv_fwd", "wae_upsample_stage_fwd", "wae_vq_", "wae_clip_adam_ema")
MOVED_NAMES = ("wae_to_btc_list", "wae_accum_stats", "wae_masked_mean", "wae_dmol_loss_fwd", "wae_mog_loss_fwd")


def _trees():
    out = {}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            out[os.path.basename(path)] = ast.parse(f.read(), path)
    return out


def _functions(tree):
    """every function of the module, methods and nested ones included, as (name, node)"""
    return [(n.name, n) for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]


def _sites(trees, match):
    """{(file, innermost enclosing function | None)} of every attribute reference x.<name> with match(name)"""
    found = set()
    for rel, tree in trees.items():
        owner = {}
        for name, fn in _functions(tree):       # ast.walk is breadth-first: inner functions come later and overwrite
            for n in ast.walk(fn):
                owner[id(n)] = name
        for n in ast.walk(tree):
            if isinstance(n, ast.Attribute) and match(n.attr):
                found.add((rel, owner.get(id(n))))
    return found


def _moved(name):
    return name.startswith(MOVED_PREFIXES) or name in MOVED_NAMES


def _advances(trees, attr):
    return [(rel, n.lineno) for rel, tree in trees.items() for n in ast.walk(tree)
            if isinstance(n, ast.AugAssign) and isinstance(n.target, ast.Attribute) and n.target.attr == attr]


def _cuda_cat(trees):
    """{(file, function)} of the functions that both test is_cuda and call torch.cat"""
    hits = set()
    for rel, tree in trees.items():
        for name, fn in _functions(tree):
            nodes = list(ast.walk(fn))
            tests = any(isinstance(n, ast.Attribute) and n.attr == "is_cuda" for n in nodes)
            cats = any(isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "cat"
                       and getattr(n.func.value, "id", None) == "torch" for n in nodes)
            if tests and cats:
                hits.add((rel, name))
    return hits


def _imports(tree):
    names = []
    for n in ast.walk(tree):
        if isinstance(n, ast.ImportFrom):
            names += [n.module or ""] + [a.name for a in n.names]
        if isinstance(n, ast.Import):
            names += [a.name for a in n.names]
    return names


# ---- structure -----------------------------------------------------------------------------------------------------------------------------
def test_one_launch_site_per_list_kernel():
    trees = _trees()
    assert _sites(trees, lambda a: a == "wae_enc_conv_fwd_list") == {("frontend.py", "conv_list")}
    assert _sites(trees, lambda a: a == "wae_upsample_stage_fwd_list") == {("frontend.py", "ups_list_chain")}
    # the one call is what both chains use
    users = {name for name, fn in _functions(trees["frontend.py"])
             if any(isinstance(n, ast.Call) and getattr(n.func, "id", None) == "conv_list" for n in ast.walk(fn))}
    assert users == {"enc_list_chain", "ups_list_chain"}
    feed = {name for name, fn in _functions(trees["decode.py"])
            if any(isinstance(n, ast.Attribute) and n.attr == "conv_list" for n in ast.walk(fn))}
    assert feed == {"feed_list"}       # DecodeSession's conv_in takes the same call, on a record of its own


def test_engine_reaches_no_front_end_or_optimizer_entry():
    trees = _trees()
    assert _sites({"engine.py": trees["engine.py"]}, _moved) == set()


def test_one_optimizer_call_one_step_counter():
    trees = _trees()
    assert _sites(trees, lambda a: a.startswith("wae_clip_adam_ema")) == {("train.py", "clip_adam_ema")}
    callers = {name for name, fn in _functions(trees["train.py"])
               if any(isinstance(n, ast.Call) and getattr(n.func, "id", None) == "clip_adam_ema" for n in ast.walk(fn))}
    assert callers == {"step_apply"}
    adv = _advances(trees, "opt_step")
    assert len(adv) == 1 and adv[0][0] == "train.py"


def test_the_modules_do_not_import_the_engine():
    trees = _trees()
    for rel in ("frontend.py", "train.py"):
        assert all("engine" not in name.split(".") for name in _imports(trees[rel])), rel
    from wavenet_autoencoders_amd import engine, frontend, train
    assert engine.F is frontend and engine.TR is train


def test_one_packer():
    assert _cuda_cat(_trees()) == {("frontend.py", "pack_time")}


def test_the_walkers_see_what_they_look_for():
    src = ("import engine\nfrom . import engine as E\nfrom .engine import WaeEngine\n"
           "def a(eng):\n    eng.lib.wae_enc_conv_fwd_list(1)\n    def inner():\n        eng.lib.wae_clip_adam_ema_det(2)\n    eng.opt_step += 1\n"
           "class C:\n    def m(self, x):\n        f = self.lib.wae_vq_nearest\n        return torch.cat(x) if x[0].is_cuda else x\n"
           "def b(eng, x):\n    eng.opt_step = 0\n    return x.is_cuda\n"
           "def c(x):\n    return torch.cat(x)\n"
           "'wae_masked_mean in a string is no call'\n")
    trees = {"m.py": ast.parse(src)}
    assert _sites(trees, _moved) == {("m.py", "a"), ("m.py", "inner"), ("m.py", "m")}
    assert _sites(trees, lambda a: a == "wae_masked_mean") == set()
    assert _advances(trees, "opt_step") == [("m.py", 8)]
    assert _cuda_cat(trees) == {("m.py", "m")}
    assert [n for n in _imports(trees["m.py"]) if "engine" in n.split(".")] == ["engine", "engine", "engine"]
    assert _moved("wae_vq_stats_segments") and _moved("wae_to_btc_list") and not _moved("wae_to_btc") and not _moved("wae_gproj_fwd")


# ---- the packer ----------------------------------------------------------------------------------------------------------------------------
CPU = types.SimpleNamespace(device=torch.device("cpu"))


def test_pack_time_rows_1():
    from wavenet_autoencoders_amd.frontend import pack_time
    parts = [np.arange(0, 3), torch.arange(3, 8), np.arange(8, 9, dtype=np.int64), torch.arange(9, 11, dtype=torch.int16)]
    for items in (parts, [torch.as_tensor(p) for p in parts], [np.asarray(p) for p in parts]):
        got = pack_time(CPU, items, 1, torch.int32)
        assert got.shape == (1, 11) and got.dtype == torch.int32 and got.is_contiguous()
        assert got.view(-1).tolist() == list(range(11))                     # the caller's order
    one = pack_time(CPU, [np.linspace(0, 1, 5)], 1)
    assert one.dtype == torch.float32 and one.shape == (1, 5)


def test_pack_time_rows_3():
    from wavenet_autoencoders_amd.frontend import pack_time
    whole = torch.arange(3 * 12, dtype=torch.float64).reshape(3, 12)
    cuts = [(0, 2), (2, 7), (7, 8), (8, 12)]
    tensors = [whole[:, a:b] for a, b in cuts]                              # (views: not contiguous)
    mixed = [t.numpy() if i % 2 else t for i, t in enumerate(tensors)]
    lead = [t.reshape(1, 3, -1) if i in (1, 3) else t for i, t in enumerate(tensors)]      # (1, C, T) where _pack_cond_list took it
    for items in (tensors, mixed, [t.numpy() for t in tensors], lead):
        got = pack_time(CPU, items, 3)
        assert got.shape == (3, 12) and got.dtype == torch.float32 and got.is_contiguous()
        assert torch.equal(got, whole.float())
    assert torch.equal(pack_time(CPU, tensors[::-1], 3), torch.cat([t.float() for t in tensors[::-1]], dim=1))


def test_pack_cond_list_is_the_packer():
    from wavenet_autoencoders_amd.engine import WaeEngine
    eng = object.__new__(WaeEngine)
    eng.device, eng.g = torch.device("cpu"), types.SimpleNamespace(Cc=3)
    got = eng._pack_cond_list([np.ones((3, 2), np.float32), torch.zeros(1, 3, 4)])
    assert got.shape == (3, 6) and got[:, :2].eq(1).all() and got[:, 2:].eq(0).all()


# ---- the item intake -----------------------------------------------------------------------------------------------------------------------
CFG = dict(layers=4, stacks=2, R=32, G=48, S=32, O=64, Cc=16, Cg=8, k=3, n_speakers=5, upsample_scales=[4, 4, 8, 5], encoder_hid=32,
           c_in=39, K=32, cin_pad=0)


def _g(**kw):
    from wavenet_autoencoders_amd import Geometry
    return Geometry.from_cfg(dict(CFG, **kw))


def _item(T=8, rows=39, frames=2, gid=1, **kw):
    return dict(dict(x=torch.zeros(T, dtype=torch.int64), c=torch.zeros(rows, frames), gid=gid), **kw)


X2D, NOC = torch.zeros(2, 8), dict(c=None)
REFUSALS = [
    # (id, who, need, t_min, geometry, items, words)
    ("train_empty", "train_step_list", "train", 2, {}, [], "train_step_list: an empty list"),
    ("train_x_2d", "train_step_list", "train", 2, {}, [_item(), _item(x=X2D)], "item 1: x has shape (2, 8); every x is (T,) with T >= 2"),
    ("train_x_short", "train_step_list", "train", 2, {}, [_item(T=1)], "item 0: x has shape (1,); every x is (T,) with T >= 2"),
    ("train_no_x", "train_step_list", "train", 2, {}, [_item(), _item(), _item(x=None)], "item 2: x has shape (); every x is (T,)"),
    ("train_c_rows", "train_step_list", "train", 2, {}, [_item(), _item(rows=16)], "item 1: c has shape (16, 2); every c is (39, frames)"),
    ("train_c_missing", "train_step_list", "train", 2, {}, [_item(**NOC)], "item 0: c has shape (); every c is (39, frames)"),
    ("train_c_rows_no_encoder", "train_step_list", "train", 2, dict(c_in=None), [_item()], "item 0: c has shape (39, 2); every c is (16, frames)"),
    ("train_no_gid", "train_step_list", "train", 2, {}, [_item(), _item(gid=None)], "train_step_list: item 1 has no gid"),
    ("train_two_faults_in_item_order", "train_step_list", "train", 2, {}, [_item(rows=7), _item(x=X2D)], "item 0: c has shape (7, 2)"),
    ("train_two_faults_in_one_item", "train_step_list", "train", 2, {}, [_item(x=X2D, rows=7, gid=None)], "item 0: x has shape (2, 8)"),
    ("train_c_before_gid", "train_step_list", "train", 2, {}, [_item(rows=7, gid=None)], "item 0: c has shape (7, 2)"),
    ("fwd_empty", "decoder_forward_list", "c", 1, {}, [], "decoder_forward_list: an empty list"),
    ("fwd_x_empty", "decoder_forward_list", "c", 1, {}, [_item(), _item(T=0)], "item 1: x has shape (0,); every item is (T,) with T >= 1"),
    ("fwd_x_2d", "decoder_forward_list", "c", 1, {}, [_item(x=X2D)], "item 0: x has shape (2, 8); every item is (T,) with T >= 1"),
    ("fwd_gid_on_some", "decoder_forward_list", "c", 1, {}, [_item(), _item(gid=None)], "decoder_forward_list: gid on all items or on none"),
    ("fwd_no_c", "decoder_forward_list", "c", 1, {}, [_item(), _item(**NOC)], "model has local conditioning but an item has no c"),
    ("fwd_x_before_c", "decoder_forward_list", "c", 1, {}, [_item(**NOC), _item(T=0)], "item 1: x has shape (0,)"),
    ("fwd_gid_before_c", "decoder_forward_list", "c", 1, {}, [_item(**NOC), _item(gid=None)], "gid on all items or on none"),
    ("enc_empty", "encode_list", "feats", 1, {}, [], "encode_list: an empty list"),
    ("enc_rows", "encode_list", "feats", 1, {}, [torch.zeros(39, 4), np.zeros((16, 4))], "item 1 has shape (16, 4); every item is (c_in, F) = (39, F)"),
    ("enc_1d", "encode_list", "feats", 1, {}, [torch.zeros(39)], "item 0 has shape (39,); every item is (c_in, F) = (39, F)"),
    ("enc_no_array", "encode_list", "feats", 1, {}, [None], "item 0 has shape (); every item is (c_in, F)"),
    ("enc_no_frames", "encode_list", "feats", 1, {}, [torch.zeros(39, 4), torch.zeros(39, 0)], "encode_list: item 1 has no frames (F >= 1)"),
    ("enc_two_faults", "encode_list", "feats", 1, {}, [torch.zeros(39, 0), torch.zeros(3, 4)], "item 0 has no frames"),
]


@pytest.mark.parametrize("who,need,t_min,geom,items,words", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_list_items_refuses(who, need, t_min, geom, items, words):
    from wavenet_autoencoders_amd.train import list_items
    with pytest.raises(ValueError) as e:
        list_items(who, items, _g(**geom), need, t_min=t_min)
    assert words in str(e.value) and str(e.value).startswith(who + ": "), str(e.value)


def test_list_items_accepts():
    from wavenet_autoencoders_amd.train import list_items
    g = _g()
    a, b = _item(T=2, frames=3), dict(x=np.zeros(640), feats=np.zeros((39, 5)), gid=torch.tensor(4))      # (forward_list's name for the features)
    Ts, Fs, cs, gids = list_items("train_step_list", [a, b], g, "train", t_min=2)
    assert (Ts, Fs) == ([2, 640], [3, 5]) and cs[0] is a["c"] and cs[1] is b["feats"] and gids == [1, b["gid"]]
    a, b = _item(T=1, rows=16, frames=7, gid=None), _item(T=9, rows=16, frames=1, gid=None)
    Ts, Tcs, cs, gids = list_items("decoder_forward_list", [a, b], g, "c")
    assert (Ts, Tcs, gids) == ([1, 9], [7, 1], [None, None]) and cs[1] is b["c"]
    assert list_items("decoder_forward_list", [_item(T=3, **NOC)], _g(Cc=0, upsample_scales=None, c_in=None), "c")[:3] == ([3], None, None)
    feats = [np.zeros((39, 1)), torch.zeros(39, 6)]
    assert list_items("encode_list", feats, g, "feats") == (None, [1, 6], feats, None)
