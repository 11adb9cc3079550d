"""The cases of tests/train_cases.py without a GPU: they meet every edge the decision-side training kernels have, the plain fp32
restatements stay within the bars (which are 4 x their measured distance from fp64, printed here), every planted fault lands over a
bar, the fp64 references are what they claim to be on inputs small enough to check by hand, and the four entries are declared,
exported and refuse bad arguments before any device call."""
import ctypes as C
import math

import numpy as np
import pytest

from jolineedle_amd import _lib
from tests import train_cases as tc

NEW_ENTRIES = {"jn_reinforce_loss": 17, "jn_logits_grad": 10, "jn_ce_loss": 10, "jn_adamw": 11}


def _of(kind):
    return [c for c in tc.LOSS_CASES if c.kind == kind]


# ---- the cases meet the edges -----------------------------------------------------------------------------------------------------
def test_every_kernel_meets_every_edge_and_option():
    assert len(set(tc.LOSS_CASES)) == len(tc.LOSS_CASES) and len(set(tc.ADAM_CASES)) == len(tc.ADAM_CASES)
    for kind in ("rf", "lg", "ce"):
        cs = _of(kind)
        assert {c.B * c.T for c in cs} >= {1, 255, 256, 257, 1300} and {c.T for c in cs} == {1, 5, 20}
        assert {c.nA for c in cs} == {9, 5} and any(c.big for c in cs)
    for kind in ("rf", "ce"):
        assert {c.mask for c in _of(kind)} == {"full", "holes", "agent", "none"}
    for kind in ("rf", "lg"):
        assert {c.stop for c in _of(kind)} == {0, 1, 2, 3}
        for c in _of(kind):
            S = tc.steps_of(c, tc.inputs(c)["n_done"])
            assert S == {0: c.T, 1: 1, 2: c.T - 1, 3: c.T}[c.stop] and 1 <= S <= c.T
    rf = _of("rf")
    assert {c.norm for c in rf} == {0, 1} and {c.ew for c in rf} == {0.0, 0.01} and {c.scale for c in rf} == {1.0, 0.25}
    assert {c.up for c in _of("lg")} == {"both", "nolp", "noent"}
    assert {c.sw for c in _of("ce")} == {1.0, 2.5}
    for c in _of("ce"):
        d = tc.inputs(c)
        if c.nA > 8 and c.B * c.T >= 255 and c.mask != "none":      # targets that hit the weighted class and ones that do not
            y = d["target"][d["masks"] == 1]
            assert (y == 8).any() and (y != 8).any()
        lg = d["logits"][0, 0]
        assert lg[1] == lg[3] == lg.max() and int(d["target"][0, 0]) == 1
        others = d["logits"].reshape(-1, c.nA)[1:]
        if len(others):      # no other ties: the accuracy does not hang on an order
            top2 = others.topk(2, dim=1).values
            assert float((top2[:, 0] - top2[:, 1]).min()) > 0
    for c in tc.LOSS_CASES:
        d = tc.inputs(c)
        if c.mask in ("holes", "agent"):
            assert d["masks"].any() and not d["masks"].all()
        if c.mask == "agent":
            assert not d["masks"][c.B // 2].any()
    ad = tc.ADAM_CASES
    assert {c.n for c in ad if c.steps} == {1, 255, 256, 257, 65537} and {c.step for c in ad if not c.steps} == {1, 2, 10, 1000}
    assert {c.clip for c in ad} == {0.0, 1.0} and {c.gs for c in ad} == {1.0, 0.25} and {c.wd for c in ad} == {0.0, 0.01}
    g = tc.adam_inputs(next(c for c in ad if c.n == 257 and c.steps))["g"][0].tolist()
    for want in (0.0, 1e-12, 1e-3, 0.999, 1.0, 1.001, 50.0, 3.0):
        assert any(x == np.float32(want) for x in g) and any(x == -np.float32(want) for x in g), want
    one = tc.adam_inputs(next(c for c in ad if c.step == 1000))
    assert one["m"].abs().max() > 0 and one["v"].min() >= 0 and one["v"].max() > 0 and one["first"] == 1000


# ---- the references are the formulas, on inputs checked by hand ------------------------------------------------------------------
def test_references_on_inputs_small_enough_to_check_by_hand():
    # two classes with equal logits: p = 1/2, logp = -ln 2, H = ln 2; d logp[a] / d logits = (1/2, -1/2) for a = 0; d H = 0
    c = tc._case("rf", 1, 1, nA=2, ew=0.5, norm=0)
    d = tc.inputs(c)
    d["logits"].zero_(); d["actions"].zero_(); d["returns"].fill_(2.0); d["rewards"].fill_(3.0)
    r = tc.reference(c)
    ln2 = math.log(2.0)
    assert r["metrics"] == pytest.approx([2.0 * ln2, -ln2, 2.0 * ln2 - 0.5 * ln2, 3.0, 1.0, 1.0], abs=1e-14)
    assert r["dlogits"].flatten().tolist() == pytest.approx([-1.0, 1.0], abs=1e-14)      # -adv (onehot - p), the entropy term vanishes
    # AdamW, one element, first step: m = 0.1 g, v = 0.001 g^2, update = lr g / (|g| + eps), after decay
    a = tc.Adam(n=1, p="normal", wd=0.01, clip=1.0, gs=0.25, steps=5, step=0)
    d = tc.adam_inputs(a)
    st = tc.adam_reference(a)[0]
    gp = max(-1.0, min(1.0, float(d["g"][0][0]) * 0.25))
    assert gp == 0.75      # 3 scaled to 0.75, inside the clip
    assert float(st["m"][0]) == pytest.approx(0.1 * gp, rel=1e-14) and float(st["v"][0]) == pytest.approx(0.001 * gp * gp, rel=1e-12)
    p0 = float(d["p"][0])
    assert float(st["p"][0]) == pytest.approx(p0 * (1 - 1e-5) - 1e-3 * gp / (abs(gp) + 1e-8), rel=1e-12)


# ---- the bars mean something --------------------------------------------------------------------------------------------------------
def _check_bars(name, worst, at, measured, bar):
    print(f"fp32 restatement, {name}: " + ", ".join(f"{k} {worst[k]:.2e} ({at.get(k, '-')})" for k in measured))
    for k in measured:      # the figure written down covers what is measured here, tightly, and the bar is 4 x it, rounded up to one digit
        assert 0.8 * measured[k] <= worst[k] <= measured[k], (name, k, worst[k])
        assert bar[k] == pytest.approx(tc.bar_of(measured[k]), rel=1e-9), (name, k)


def test_fp32_restatements_stay_within_every_bar():
    worst, at = {}, {}
    for c in tc.LOSS_CASES:
        ref, got = tc.reference(c), tc.compute(c)
        assert not tc.over_bars(c, got, ref), (c, tc.over_bars(c, got, ref))
        w = worst.setdefault((c.kind, c.big), dict(l2=0.0, mx=0.0, met=0.0))
        for k, v in tc.distances(c, got, ref).items():
            if v > w[k]:
                w[k], at[c.kind, c.big, k] = v, tc.case_id(c)
    for kind, name, measured, bar in (("rf", "REINFORCE", tc.RF_FP32_MEASURED, tc.RF_BAR), ("lg", "logits_grad", tc.LG_FP32_MEASURED, tc.LG_BAR),
                                      ("ce", "cross-entropy", tc.CE_FP32_MEASURED, tc.CE_BAR)):
        for big, m, b in ((0, measured, bar), (1, tc.BIG_FP32_MEASURED[kind], tc.BIG_BAR[kind])):
            _check_bars(name + (", logits x 30" if big else ""), worst[kind, big], {k: at.get((kind, big, k)) for k in m}, m, b)


def test_fp32_adamw_restatement_stays_within_every_bar():
    worst, at = dict(p=0.0, m=0.0, v=0.0), {}
    for c in tc.ADAM_CASES:
        ref, got = tc.adam_reference(c), tc.adam_compute(c)
        assert not tc.adam_over_bars(got, ref), (c, tc.adam_over_bars(got, ref))
        for k, v in tc.adam_distances(got, ref).items():
            if v > worst[k]:
                worst[k], at[k] = v, tc.case_id(c)
    _check_bars("AdamW", worst, at, tc.AD_FP32_MEASURED, tc.AD_BAR)


def test_constants_formed_in_fp32_from_the_fp32_betas_miss_the_bars():
    """What the launcher and the kernel did before: 1 - beta1, 1 - beta2 and both bias corrections in fp32 from 0.9f and 0.999f.
    0.999f is 0.99900001287, so 1 - beta2 is 1.3e-5 below 0.001 and v is 1.3e-5 low at every step of every case.  From zero moments the
    fp32 bias correction 1 - powf(0.999f, 1) is the very same number and the first update is right; with the step count the
    correction loses the factor while v keeps it, and against pre-loaded moments it never had it: the update is then up to 6.4e-6
    (half of 1.3e-5) high, more where steps add up."""
    f = np.float32
    assert float(f(1.0) - f(0.999)) / 0.001 - 1.0 == pytest.approx(-1.29e-5, rel=1e-2)
    over_p = 0
    for c in tc.ADAM_CASES:
        ref, got = tc.adam_reference(c), tc.adam_compute(c, mutant="fp32_betas")
        d = tc.adam_distances(got, ref)
        print(f"{tc.case_id(c)}: p {d['p']:.1e} m {d['m']:.1e} v {d['v']:.1e}")
        assert 1.2e-5 <= d["v"] <= 1.4e-5 and d["v"] > 6 * tc.AD_BAR["v"]
        over_p += d["p"] > tc.AD_BAR["p"]
        first = tc.adam_distances(got[:1], ref[:1])["p"]
        if c.steps:      # from zero moments the two errors cancel in the first update
            assert first <= tc.AD_BAR["p"], (c, first)
        elif c.p == "zero":
            assert first > tc.AD_BAR["p"], (c, first)
    assert over_p >= len(tc.ADAM_CASES) // 2


# ---- the bars bite --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(tc.LOSS_MUTANTS))
def test_a_planted_fault_in_a_loss_kernel_exceeds_a_bar(mutant):
    cases = [c for c in tc.LOSS_CASES if tc.LOSS_MUTANTS[mutant](c)]
    assert cases
    caught = {c.kind: False for c in cases}
    for c in cases:
        if tc.over_bars(c, tc.compute(c, mutant=mutant), tc.reference(c)):
            caught[c.kind] = True
    assert all(caught.values()), (mutant, caught)      # on at least one case of every kernel the fault can be planted in


@pytest.mark.parametrize("mutant", sorted(tc.ADAM_MUTANTS))
def test_a_planted_fault_in_adamw_exceeds_a_bar(mutant):
    cases = [c for c in tc.ADAM_CASES if tc.ADAM_MUTANTS[mutant](c)]
    assert cases
    caught = [c for c in cases if tc.adam_over_bars(tc.adam_compute(c, mutant=mutant), tc.adam_reference(c))]
    assert caught, mutant
    if mutant in ("no_bc2", "fp32_betas"):      # nothing hides these: every case shows them
        assert len(caught) == len(cases), [tc.case_id(c) for c in cases if c not in caught]


# ---- the entries ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def lib():
    return _lib.load_library()


def test_library_declares_and_exports_the_entries(lib):
    header = (_lib.LIB_PATH.parents[2] / "include" / "jnroll.h").read_text()
    for name, n_args in NEW_ENTRIES.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == _lib.SIGNATURES[name][1]
        assert f"int {name}(" in header
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        text = (_lib.LIB_PATH.parents[2] / doc).read_text()
        for name in NEW_ENTRIES:
            assert f"`{name}`" in text, (doc, name)


P = 4096      # stands for a device pointer: every call below is refused before it is touched


def _g(o):
    return lambda k, d: o.get(k, d)


def _reinforce_loss(lib, **o):
    g = _g(o)
    return lib.jn_reinforce_loss(g("logits", P), g("actions", P), g("returns", P), g("rewards", P), g("masks", P), g("n_done", None), g("B", 2), g("T", 3),
                                 g("nA", 9), 1, 0.0, 1.0, 0.01, 1.0, g("dlogits", P), g("metrics", P), None)


def _logits_grad(lib, **o):
    g = _g(o)
    return lib.jn_logits_grad(g("logits", P), g("actions", P), g("dlogprobs", P), g("dentropies", P), g("n_done", None), g("B", 2), g("T", 3), g("nA", 9),
                              g("dlogits", P), None)


def _ce_loss(lib, **o):
    g = _g(o)
    return lib.jn_ce_loss(g("logits", P), g("target", P), g("masks", P), g("B", 2), g("T", 3), g("nA", 9), 2.5, g("dlogits", P), g("metrics", P), None)


def _adamw(lib, **o):
    g = _g(o)
    return lib.jn_adamw(g("p", P), g("g", P), g("m", P), g("v", P), g("n", 10), g("lr", 1e-3), g("wd", 0.01), g("step", 1), g("clip", 1.0), 1.0, None)


_SHAPES = (dict(B=0), dict(T=0), dict(nA=0), dict(nA=257), dict(B=-1), dict(B=1 << 13, T=(1 << 11) + 1))
REFUSALS = {
    _reinforce_loss: _SHAPES + tuple({k: None} for k in ("logits", "actions", "returns", "rewards", "masks", "dlogits", "metrics")),
    _logits_grad: _SHAPES + (dict(logits=None), dict(actions=None), dict(dlogits=None), dict(dlogprobs=None, dentropies=None)),
    _ce_loss: _SHAPES + tuple({k: None} for k in ("logits", "target", "masks", "dlogits", "metrics")),
    _adamw: (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(n=-5), dict(step=0), dict(step=-1), dict(lr=-1e-3), dict(wd=-0.01),
             dict(clip=-1.0), dict(lr=float("nan"))),
}


@pytest.mark.parametrize("entry", list(REFUSALS), ids=lambda f: f.__name__.strip("_"))
def test_entries_refuse_bad_arguments_before_any_device_call(lib, entry):
    for bad in REFUSALS[entry]:
        assert entry(lib, **bad) == -1, bad
        assert b"jn_" + entry.__name__.strip("_").encode() in lib.jn_last_error()
