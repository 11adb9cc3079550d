"""Wide decision transformers (256 < n_embd <= 1024) without a GPU: what jn_create admits and refuses, the state-dict
table of a wide zoo model, and which decision route a context takes (jn_debug_decision_route)."""
import ctypes as C

import pytest

import jolineedle_amd as ja
from jolineedle_amd import _lib
from jolineedle_amd.engine import GPT_ZOO, make_jn_config
from tests.helpers import model_config

SMALL = dict(patch_size=64, block_size=4, image_processor=None, with_detector=False, gpt_backbone="yolox-nano")
PER_AGENT, WIDE = 0, 1


def _create(max_batch=4, **kw):
    lib = _lib.load_library()
    cfg = make_jn_config(model_config(**{**SMALL, **kw}), 0, max_batch, 9)
    h = C.c_void_p()
    rc = lib.jn_create(C.byref(cfg), C.byref(h))
    return lib, rc, h


def _arch(n_layer, n_head, n_embd):
    return dict(model_type=None, n_layer=n_layer, n_head=n_head, n_embd=n_embd)


@pytest.mark.parametrize("kw", [dict(model_type="gopher-44m"), dict(model_type="gpt2"), dict(model_type="openai-gpt"),
                                dict(model_type="gpt2-medium"), _arch(2, 5, 320)],
                         ids=["gopher-44m", "gpt2", "openai-gpt", "gpt2-medium", "wide-320"])
def test_create_admits_wide_models_on_the_wide_route(kw):
    lib, rc, h = _create(**kw)
    assert rc == 0, lib.jn_last_error()
    try:
        assert lib.jn_debug_decision_route(h) == WIDE
    finally:
        lib.jn_destroy(h)


@pytest.mark.parametrize("kw", [_arch(2, 5, 260), dict(model_type="gpt2-large"), dict(model_type="gpt2-xl"), _arch(2, 4, 1088)],
                         ids=["260", "gpt2-large-1280", "gpt2-xl-1600", "1088"])
def test_create_refuses_what_neither_route_takes_and_names_both_bounds(kw):
    lib, rc, h = _create(**kw)
    assert rc == -1                                         # JN_EINVAL
    msg = lib.jn_last_error().decode()
    assert "n_embd" in msg and "256" in msg and "1024" in msg, msg


def test_state_dict_table_of_gopher_44m_matches_the_oracle():
    """Names, shapes and the reference's order (torch.optim.AdamW keys its state by position)."""
    from oracle.gpt_ref import build_gpt_ref
    kw = dict(SMALL, model_type="gopher-44m")
    oracle = build_gpt_ref(1, **kw)
    m = ja.GPT(model_config(**kw), max_batch=2)
    sd, osd = m.state_dict(), oracle.state_dict()
    assert list(sd) == list(osd)
    for k in sd:
        assert sd[k].shape == osd[k].shape and sd[k].dtype == osd[k].dtype, k
    assert [(n, tuple(p.shape)) for n, p in m.named_parameters()] == [(n, tuple(p.shape)) for n, p in oracle.named_parameters()]
    n_layer, n_head, n_embd = GPT_ZOO["gopher-44m"]
    assert sd["transformer.h.%d.mlp.c_fc.weight" % (n_layer - 1)].shape == (4 * n_embd, n_embd)


def test_decision_route_defaults_and_the_switch(monkeypatch):
    monkeypatch.delenv("JN_GPT_WIDE", raising=False)
    want = {"gpt-nano": PER_AGENT, "gpt-mini": PER_AGENT, "gpt-micro": PER_AGENT, "gopher-44m": WIDE}
    for name, route in want.items():
        lib, rc, h = _create(model_type=name)
        assert rc == 0, lib.jn_last_error()
        assert lib.jn_debug_decision_route(h) == route, name
        lib.jn_destroy(h)
    # the switch takes the wide route where that route admits the model (n_embd a multiple of 64) and nowhere else
    monkeypatch.setenv("JN_GPT_WIDE", "1")
    want = {"gpt-nano": PER_AGENT, "gpt-pico": PER_AGENT, "gpt-mini": WIDE, "gpt-micro": WIDE, "gopher-44m": WIDE}
    for name, route in want.items():
        lib, rc, h = _create(model_type=name)
        assert rc == 0, lib.jn_last_error()
        assert lib.jn_debug_decision_route(h) == route, name
        lib.jn_destroy(h)
    # a bare env context (n_embd 4) is not touched by it either
    from jolineedle_amd.engine import bare_env_config
    cfg = bare_env_config(64, 4, 0, 4)
    h = C.c_void_p()
    assert lib.jn_create(C.byref(cfg), C.byref(h)) == 0, lib.jn_last_error()
    assert lib.jn_debug_decision_route(h) == PER_AGENT
    lib.jn_destroy(h)
    # any other value of the variable is "off"
    monkeypatch.setenv("JN_GPT_WIDE", "0")
    lib, rc, h = _create(model_type="gpt-mini")
    assert rc == 0 and lib.jn_debug_decision_route(h) == PER_AGENT
    lib.jn_destroy(h)
