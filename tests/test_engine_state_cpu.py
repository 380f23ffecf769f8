"""The engine's step state has owners: the package reads and writes it through declared attributes and the two records
(step_state.Saved, step_state.InFlight), never by probing an engine with getattr / hasattr / __dict__.  Checked on the sources with
`ast`: no GPU and no import of the package."""
import ast
import os

import pytest

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "wavenet_autoencoders_amd")
FILES = ["engine.py", "frontend.py", "train.py", "decode.py", "backward.py", "vqvae_model.py", "checkpoint.py", "wavenet_vocoder/wavenet.py", "wavenet_vocoder/modules.py"]
ENGINE_NAMES = {"self", "eng", "engine"}


def _tree(rel):
    with open(os.path.join(PKG, rel)) as f:
        return ast.parse(f.read(), rel)


def _is_engine(node):
    return isinstance(node, ast.Name) and node.id in ENGINE_NAMES


@pytest.mark.parametrize("rel", FILES)
def test_no_probing_of_an_engine(rel):
    bad = []
    for node in ast.walk(_tree(rel)):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id in ("getattr", "hasattr")
                and len(node.args) >= 2 and _is_engine(node.args[0])
                and isinstance(node.args[1], ast.Constant) and isinstance(node.args[1].value, str)):
            bad.append((node.lineno, f"{node.func.id}({node.args[0].id}, {node.args[1].value!r})"))
        if isinstance(node, ast.Attribute) and node.attr == "__dict__" and _is_engine(node.value):
            bad.append((node.lineno, f"{node.value.id}.__dict__"))
    assert not bad, bad


def _self_attrs(fn):
    """names assigned as self.<name> inside fn: plain, chained, tuple, augmented and annotated assignments, `with ... as` and `for`"""
    out = set()

    def targets(t):
        if isinstance(t, (ast.Tuple, ast.List)):
            for e in t.elts:
                targets(e)
        elif isinstance(t, ast.Starred):
            targets(t.value)
        elif isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self":
            out.add(t.attr)
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign):
            for t in node.targets:
                targets(t)
        elif isinstance(node, (ast.AugAssign, ast.AnnAssign, ast.For)):
            targets(node.target)
        elif isinstance(node, ast.With):
            for item in node.items:
                if item.optional_vars is not None:
                    targets(item.optional_vars)
    return out


def test_every_engine_attribute_is_declared_in_init():
    cls = next(n for n in _tree("engine.py").body if isinstance(n, ast.ClassDef) and n.name == "WaeEngine")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef)]
    declared = _self_attrs(next(f for f in fns if f.name == "__init__"))
    # a property with a setter is declared by the class
    declared |= {f.name for f in fns if any(isinstance(d, ast.Attribute) and d.attr == "setter" for d in f.decorator_list)}
    late = {(f.name, a) for f in fns if f.name != "__init__" for a in _self_attrs(f) if a not in declared}
    assert not late, sorted(late)


def test_the_checks_see_what_they_look_for():
    """the two walkers above on a source that breaks both rules"""
    src = ("class WaeEngine:\n    def __init__(self):\n        self.a = self.b = 0\n        self.c, self.d = 1, 2\n"
           "    def f(self, eng):\n        self.a += 1\n        with g() as self.e:\n            pass\n"
           "        return getattr(eng, 'x', None), hasattr(self, 'y'), eng.__dict__, getattr(self.hp, 'z', 0)\n")
    cls = ast.parse(src).body[0]
    init, f = cls.body
    assert _self_attrs(init) == {"a", "b", "c", "d"} and _self_attrs(f) == {"a", "e"}
    hits = [n for n in ast.walk(f) if isinstance(n, ast.Call) and getattr(n.func, "id", "") in ("getattr", "hasattr") and _is_engine(n.args[0])]
    assert len(hits) == 2 and sum(isinstance(n, ast.Attribute) and n.attr == "__dict__" and _is_engine(n.value) for n in ast.walk(f)) == 1
