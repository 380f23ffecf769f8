"""The eight decode entries share one set of refusals (csrc/ar_host.hpp), without a GPU: every entry refuses the same broken network
under its own name, and none accepts what it refused before the checks were shared -- the refusal tables of tests/test_ar_list_cpu.py,
test_ar_team_list_cpu.py, test_ar_stream_cpu.py and test_ar_scalar_coop_cpu.py, replayed from those modules (raw ctypes calls with dummy
pointers; every call returns before any launch)."""
import ctypes

import pytest

import test_ar_list_cpu as one_cu_list
import test_ar_scalar_coop_cpu as scalar_coop
import test_ar_stream_cpu as stream
import test_ar_team_list_cpu as team_list

P = ctypes.c_void_p(0x1000)
EINVAL = -1


def _net(w_layers=P, c_up=None):
    # dilations, ring_off, ring, ring_total, w_layers, layer_stride_bytes, w2_off_bytes, bias2, zb, first_tab, first_bias, w_head, head_bias,
    # c_up, c_dtype
    return [P, P, P, 1, w_layers, 1, 1, P, P, P, P, P, P, c_up, 0]


# entry -> (the name its messages begin with, scalar-input decoder?, arguments before the network, arguments behind it): a call that
# every check passes (and that these tests never make: each case breaks one thing)
ENTRIES = {
    "wae_ar_generate": ("ar_generate", 0, [], [P, P, P, P, None]),
    "wae_ar_generate_list": ("ar_generate_list", 0, [3, 2, P, P], [P, P, P, P, None]),
    "wae_ar_generate_scalar": ("ar_generate_scalar", 1, [], [P, P, P, -7.0, 0, P, P, None]),
    "wae_ar_generate_scalar_mog": ("ar_generate_scalar_mog", 1, [], [P, P, P, -7.0, P, P, None]),
    "wae_ar_generate_coop": ("ar_generate_coop", 0, [4], [P, P, P, P, P, P, P, None]),
    "wae_ar_generate_coop_fused": ("ar_generate_coop", 0, [4], [P, P, P, P, P, P, P, None, None]),      # (speaks as wae_ar_generate_coop)
    "wae_ar_generate_coop_list": ("ar_generate_coop_list", 0, [8, 3, 2, P, P, 24], [P, P, P, P, P, P, P, None]),
    "wae_ar_generate_coop_scalar": ("ar_generate_coop_scalar", 1, [4, 0], [P, P, P, -7.0, 0, P, P, P, P, P, None]),
}
FAULTS = {
    "null_w_layers": (dict(), dict(w_layers=None)),
    "dtype_7": (dict(dtype=7), dict()),
    "odd_G": (dict(G=47), dict()),
    "Cc_without_c_up": (dict(Cc=4, Ccp=4), dict(c_up=None)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_entry_refuses_a_broken_network_under_its_own_name(entry, fault):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    assert entry in _lib.SIGNATURES
    name, scalar, front, back = ENTRIES[entry]
    fields, net = FAULTS[fault]
    d = stream._desc(scalar=scalar, O=30 if scalar else 32, **fields)
    assert getattr(lib, entry)(ctypes.byref(d), *front, *_net(**net), *back) == EINVAL
    assert lib.wae_last_error().startswith(name.encode() + b": "), lib.wae_last_error()


def _table(mod):
    """the (case, code, text) rows a module's test_entry_refuses_before_any_launch is parametrised over"""
    mark, = [m for m in mod.test_entry_refuses_before_any_launch.pytestmark if m.name == "parametrize"]
    assert mark.args[0] == "case,code,text"
    return mark.args[1]


LISTS = [(mod, name, i) for mod, name in ((one_cu_list, b"ar_generate_list: "), (team_list, b"ar_generate_coop_list: "))
         for i in range(len(_table(mod)))]


@pytest.mark.parametrize("mod,name,i", LISTS, ids=[f"{name[:-2].decode()}-{i}" for _, name, i in LISTS])
def test_list_entries_still_refuse_their_tables(mod, name, i):
    from wavenet_autoencoders_amd import _lib
    lib = _lib.lib()
    case, code, text = _table(mod)[i]
    case = dict(case)
    d = mod._desc(**case.pop("d", {}))
    assert mod._call(lib, d, **case) == code
    err = lib.wae_last_error()
    assert err.startswith(name) and text in err, err


def test_team_list_checks_the_sequence_bound_before_the_ring():
    team_list.test_sequence_bound_is_thirty_one_bits()


@pytest.mark.parametrize("name,call,kw", stream.ENTRIES, ids=[e[1].__name__.lstrip("_") + str(i) for i, e in enumerate(stream.ENTRIES)])
def test_per_launch_entries_still_refuse_bad_continuations(name, call, kw):
    from wavenet_autoencoders_amd import _lib
    stream.test_every_entry_refuses_a_bad_continuation_before_any_launch(name, call, kw)
    assert _lib.lib().wae_last_error().startswith(name.encode() + b": ")


def test_dense_feedback_and_the_one_handover_form_are_still_not_continued():
    stream.test_modes_3_and_4_cannot_be_continued()
    stream.test_the_one_handover_form_cannot_be_continued()


def test_scalar_coop_entry_still_refuses_its_cases():
    scalar_coop.test_refusals_before_any_launch()
