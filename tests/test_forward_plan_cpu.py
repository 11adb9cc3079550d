"""The conv-stack forward plan (plan_forward, read through jn_debug_forward_plan) without a GPU: structural rules
restated here independently of the planner, the deferral boundary, the head-only range and known counts.

The known counts were NOT read off the planner: they come from a stand-alone host program that held the decisions of the
launch loop as it was before the plan was split off (the DWConv fusion match, the upsample scan, the deferral test and
the per-layer finalize) verbatim and counted them for these three nets at patch size 128."""
import ctypes as C

import pytest

from jolineedle_amd import _lib
from jolineedle_amd.engine import make_jn_config
from tests.helpers import model_config

STEM, CONV, DWPW, DWPW_ADD, ABSORBED, SPP, UPSAMPLE, ADDACT, PRED = range(1, 10)
P, MAX_BATCH = 128, 4097          # maps of 64, 32, 16, 8 and 4 pixels a side; 4097 > 65536 / (4 * 4)
DEFER_MAX_M = 65536               # JN_DEFER_MAX_M
ENC, DET = _lib.JN_NET_GPT_BACKBONE, _lib.JN_NET_DETECTOR


@pytest.fixture(scope="module")
def contexts():
    lib = _lib.load_library()
    kws = {"nano": dict(), "nano-bf16": dict(act_dtype="bf16"), "dense": dict(gpt_backbone="yolox-s"),
           "dense-bf16": dict(gpt_backbone="yolox-s", act_dtype="bf16"),
           "det": dict(gpt_backbone=None, image_processor="yolox-nano"),
           "det-bf16": dict(gpt_backbone=None, image_processor="yolox-nano", act_dtype="bf16")}
    handles = {}
    for name, kw in kws.items():
        cfg = make_jn_config(model_config(patch_size=P, **kw), 0, MAX_BATCH, 9)
        h = C.c_void_p()
        assert lib.jn_create(C.byref(cfg), C.byref(h)) == 0, lib.jn_last_error()     # plans every form, checks each
        handles[name] = h
    yield handles
    for h in handles.values():
        lib.jn_destroy(h)


def plan(h, net, N, train, with_head=0, first_op=0):
    lib = _lib.load_library()
    n = lib.jn_debug_forward_plan(h, net, N, train, with_head, first_op, None, 0)
    assert n > 0, lib.jn_last_error()
    buf = (C.c_int32 * (3 * n))()
    assert lib.jn_debug_forward_plan(h, net, N, train, with_head, first_op, buf, n) == n
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(n)]


def counts(steps):
    return {"dwpw": sum(r == DWPW for r, _, _ in steps), "dwpw_add": sum(r == DWPW_ADD for r, _, _ in steps),
            "conv": sum(r == CONV for r, _, _ in steps), "cand": sum(r == CONV and l >= 0 for r, l, _ in steps),
            "bn_now": sum(r in (STEM, CONV) and not d for r, _, d in steps)}


# (context, net, with_head, first_op): every form jn_create plans, the bf16 twins included
FORMS = [("nano", ENC, 0, 0), ("nano-bf16", ENC, 0, 0), ("dense", ENC, 0, 0), ("dense-bf16", ENC, 0, 0),
         ("det", DET, 0, 0), ("det", DET, 1, 0), ("det", DET, 1, 79), ("det-bf16", DET, 1, 0), ("det-bf16", DET, 1, 79)]


@pytest.mark.parametrize("name,net,head,first", FORMS)
def test_every_op_is_launched_or_absorbed_exactly_once(contexts, name, net, head, first):
    f32 = not name.endswith("bf16")
    for train in (0, 1):
        for N in (1, 16, 17, MAX_BATCH):
            steps = plan(contexts[name], net, N, train, head, first)
            covered = [0] * len(steps)
            for i, (route, link, deferred) in enumerate(steps):
                assert route in range(1, 10)
                if route == ABSORBED:
                    j = link - first
                    assert 0 <= j < i and steps[j][0] in (DWPW, DWPW_ADD)      # by a launched fusion inside the range
                    assert i - j == 1 or (i - j == 2 and steps[j][0] == DWPW_ADD)
                    assert not deferred
                    covered[i] += 1
                elif route in (DWPW, DWPW_ADD):
                    assert not train and f32 and link == first + i + 1 and not deferred
                    assert steps[i + 1][:2] == (ABSORBED, first + i)
                    assert (i + 2 < len(steps) and steps[i + 2][:2] == (ABSORBED, first + i)) == (route == DWPW_ADD)
                elif link >= 0:                                                  # an upsample candidate
                    assert route == CONV and f32 and steps[link - first][0] == UPSAMPLE and link - first > i
            fused = [i for i, s in enumerate(steps) if s[0] in (DWPW, DWPW_ADD)]
            assert sum(covered) == sum(1 if steps[i][0] == DWPW else 2 for i in fused)
            cands = [l for r, l, _ in steps if r == CONV and l >= 0]
            assert len(cands) == len(set(cands))                                 # an upsample belongs to one conv at most
            if head or not f32 or name.startswith("dense") or not train:
                assert not any(d for _, _, d in steps)                           # no deferral with the head, bf16, dense, eval


def test_deferral_boundary_per_map_size(contexts):
    """A layer is deferred while N * H * W <= 65536: for every map size of the 128 px nano encoder, at N = 65536 // (H * W)
    and not at that N + 1.  BatchNorm layers per map size (64, 32, 16, 8, 4 a side): 1, 7, 18, 26, 17 = 69."""
    h = contexts["nano"]
    not_deferred = {16: 0, 17: 1, 64: 1, 65: 8, 256: 8, 257: 26, 1024: 26, 1025: 52, 4096: 52, 4097: 69}
    before = None
    for side in (64, 32, 16, 8, 4):
        N = DEFER_MAX_M // (side * side)
        at, past = plan(h, ENC, N, 1), plan(h, ENC, N + 1, 1)
        assert counts(at)["bn_now"] == not_deferred[N] and counts(past)["bn_now"] == not_deferred[N + 1]
        assert not_deferred[N + 1] > not_deferred[N]
        for a, b in zip(at, past):
            assert a[:2] == b[:2] and a[2] >= b[2]            # only deferral moves with N, and only one way
        if before is not None:
            assert [s[2] for s in before] == [s[2] for s in at]     # nothing changes between two boundaries
        before = past
    assert plan(h, ENC, 16, 1)[0] == (STEM, -1, 1) and plan(h, ENC, 17, 1)[0] == (STEM, -1, 0)   # the 64 x 64 stem output
    assert not any(d for _, _, d in plan(h, ENC, 16, 0))       # eval never defers


def test_head_only_range_absorbs_nothing_from_outside(contexts):
    h = contexts["det"]
    whole, head = plan(h, DET, 4, 0, 1, 0), plan(h, DET, 4, 0, 1, 79)
    assert len(whole) == 109 and len(head) == 30
    assert head == whole[79:]                                   # the same routes, links as op indices of the whole net
    for route, link, _ in head:
        assert link == -1 or link >= 79
    assert head[0][0] == CONV                                   # a stem 1x1 conv, launched on its own
    # a range that starts on a pointwise conv whose depthwise conv lies outside runs that conv itself
    steps = plan(h, DET, 4, 0, 0, 0)
    i = next(i for i, s in enumerate(steps) if s[0] == DWPW)
    cut = plan(h, DET, 4, 0, 0, i + 1)
    assert cut[0][0] == CONV and cut[1:] == steps[i + 2:]


# (context, net, train, head, first) -> the old loop's counts; for train-mode passes also its bn_finalize launches (the
# BatchNorm layers that are not deferred) at N = 16 and N = 17
KNOWN = [
    ("nano", ENC, 0, 0, 0, dict(dwpw=7, dwpw_add=7, conv=40, cand=2), None),
    ("nano", ENC, 1, 0, 0, dict(dwpw=0, dwpw_add=0, conv=68, cand=2), {16: 0, 17: 1}),
    ("nano-bf16", ENC, 0, 0, 0, dict(dwpw=0, dwpw_add=0, conv=68, cand=0), None),
    ("nano-bf16", ENC, 1, 0, 0, dict(dwpw=0, dwpw_add=0, conv=68, cand=0), {16: 69, 17: 69}),
    ("dense", ENC, 0, 0, 0, dict(dwpw=0, dwpw_add=0, conv=50, cand=2), None),
    ("dense", ENC, 1, 0, 0, dict(dwpw=0, dwpw_add=0, conv=50, cand=2), {16: 51, 17: 51}),
    ("dense-bf16", ENC, 1, 0, 0, dict(dwpw=0, dwpw_add=0, conv=50, cand=0), {16: 51, 17: 51}),
    ("det", DET, 0, 0, 0, dict(dwpw=7, dwpw_add=7, conv=40, cand=2), None),
    ("det", DET, 1, 0, 0, dict(dwpw=0, dwpw_add=0, conv=68, cand=2), {16: 0, 17: 1}),
    ("det", DET, 0, 1, 0, dict(dwpw=19, dwpw_add=7, conv=43, cand=2), None),
    ("det", DET, 1, 1, 0, dict(dwpw=0, dwpw_add=0, conv=95, cand=2), {16: 96, 17: 96}),
    ("det", DET, 0, 1, 79, dict(dwpw=12, dwpw_add=0, conv=3, cand=0), None),
    ("det", DET, 1, 1, 79, dict(dwpw=0, dwpw_add=0, conv=27, cand=0), {16: 27, 17: 27}),
    ("det-bf16", DET, 0, 1, 0, dict(dwpw=0, dwpw_add=0, conv=95, cand=0), None),
]


@pytest.mark.parametrize("name,net,train,head,first,want,finalizes", KNOWN)
def test_known_counts_of_the_old_loop(contexts, name, net, train, head, first, want, finalizes):
    for N in (16, 17):
        got = counts(plan(contexts[name], net, N, train, head, first))
        bn_now = got.pop("bn_now")
        assert got == want, (N, got)
        if train:
            assert bn_now == finalizes[N], (N, bn_now)
