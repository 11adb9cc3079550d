"""jn_gpt_backward_route (host code, no device call): which backward differentiates the decision transformer.

The rule is restated here from its description in csrc/jn_kernels.h: the batched backward in its LDS form wherever a
head's q, k, v, dY and two score tiles fit 64 KB (4 (T + 1) hs + 2 (T + 1)^2 <= 16384 floats); nothing else on the wide
route; the one-workgroup-per-agent kernel up to T = 62, the length it has always been run at and is never launched above;
the tiled form from there on.  So every shape that trained before the tiled form existed takes the route it took then."""
from pathlib import Path

import pytest

from jolineedle_amd import _lib

NONE, LDS, PER_AGENT, TILED = 0, 1, 2, 3
ZOO = {48: 3, 32: 2, 128: 4, 192: 6, 256: 8}          # n_embd -> the head count the model zoo (or its nearest shape) gives it
SHAPES = [(C, nh) for C, n in ZOO.items() for nh in sorted({n, 1})]


def lds_fits(C, nh, T):
    hs, Lm = C // nh, T + 1
    return 4 * Lm * hs + 2 * Lm * Lm <= 16384


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


@pytest.fixture(autouse=True)
def _no_hook(monkeypatch):
    monkeypatch.delenv("JN_GPT_BWD_TILED", raising=False)


@pytest.mark.parametrize("C,nh", SHAPES)
def test_the_lengths_that_trained_before_keep_their_route(lib, C, nh):
    for T in range(1, 63):
        want = LDS if lds_fits(C, nh, T) else PER_AGENT
        assert lib.jn_gpt_backward_route(C, nh, T, 0) == want, (C, nh, T)


@pytest.mark.parametrize("C,nh", SHAPES)
def test_the_wide_route_has_the_lds_form_or_nothing(lib, C, nh):
    for T in range(1, 256):
        assert lib.jn_gpt_backward_route(C, nh, T, 1) == (LDS if lds_fits(C, nh, T) else NONE), (C, nh, T)


@pytest.mark.parametrize("C,nh", SHAPES)
def test_long_walks_take_the_lds_form_where_it_fits_and_the_tiled_form_elsewhere(lib, C, nh):
    got = {T: lib.jn_gpt_backward_route(C, nh, T, 0) for T in range(63, 256)}
    for T, r in got.items():
        assert r == (LDS if lds_fits(C, nh, T) else TILED), (C, nh, T)
    assert PER_AGENT not in got.values()


def test_named_thresholds_and_headline_shapes(lib):
    r = lib.jn_gpt_backward_route
    assert (r(48, 3, 74, 0), r(48, 3, 75, 0)) == (LDS, TILED)            # gpt-nano: LDS up to T = 74
    assert (r(192, 6, 63, 0), r(192, 6, 64, 0)) == (LDS, TILED)          # gpt-mini: up to T = 63
    assert (r(128, 4, 63, 0), r(128, 4, 64, 0)) == (LDS, TILED)          # gpt-micro, head size 32 as well
    assert r(48, 3, 20, 0) == LDS and r(192, 6, 32, 0) == LDS            # the headline shapes
    assert r(48, 3, 255, 0) == TILED and r(256, 1, 255, 0) == TILED and r(256, 1, 62, 0) == PER_AGENT
    # outside every form: no sequence, heads that do not divide, a sequence past 255 tokens + 1, a head wider than 256
    assert r(48, 3, 0, 0) == NONE and r(48, 5, 20, 0) == NONE and r(48, 3, 256, 0) == NONE and r(512, 1, 80, 0) == NONE
    assert r(48, 3, 20, 2) < 0                                           # decision_route is 0 or 1


def test_the_hook_sends_per_agent_route_shapes_to_the_tiled_form(lib, monkeypatch):
    monkeypatch.setenv("JN_GPT_BWD_TILED", "1")
    r = lib.jn_gpt_backward_route
    assert r(48, 3, 20, 0) == TILED and r(256, 1, 62, 0) == TILED and r(192, 6, 32, 0) == TILED
    assert r(128, 4, 20, 1) == LDS and r(320, 5, 46, 1) == NONE         # the wide route does not move
    monkeypatch.setenv("JN_GPT_BWD_TILED", "0")
    assert r(48, 3, 20, 0) == LDS


def test_the_entries_are_declared_exported_and_documented(lib):
    root = Path(__file__).resolve().parents[1]
    header = (root / "include" / "jnroll.h").read_text()
    for name in ("jn_gpt_backward_route", "jn_gpt_attention_backward"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "JN_GPT_BWD_TILED" in (root / "DESIGN.md").read_text()       # the hook is listed with the other switches
