"""The YOLOX sizes of the reference's --gpt-backbone / --image-processor choices (engine.YOLOX_SIZES) without a GPU: jn_create plans
nano, s, m, l and x as patch encoder, as detector and in bf16 mode (yolox-tiny's refusal is pinned by tests/test_host_cpu.py and
listed in DESIGN.md section 6); the forward plans of m and x obey the
structural rules of tests/test_forward_plan_cpu.py; every Conv2d shape of the six oracle nets behind the stem is admitted by the
route entries at a small and a large pixel count."""
import ctypes as C

import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd.engine import YOLOX_SIZES, make_jn_config
from oracle import yolox_ref
from tests import test_forward_plan_cpu as fp
from tests.helpers import model_config

SIZES = ("yolox-nano", "yolox-s", "yolox-m", "yolox-l", "yolox-x")      # the sizes that run
ORACLE_SIZES = SIZES + ("yolox-tiny",)
FORMS = {"encoder": lambda s: dict(gpt_backbone=s, with_detector=False, image_processor=None),
         "detector": lambda s: dict(gpt_backbone=None, image_processor=s),
         "bf16": lambda s: dict(gpt_backbone=s, with_detector=False, image_processor=None, act_dtype="bf16"),
         "detector-bf16": lambda s: dict(gpt_backbone=None, image_processor=s, act_dtype="bf16")}


def _create(size, form, P=64, max_batch=4):
    lib = _lib.load_library()
    cfg = make_jn_config(model_config(patch_size=P, **FORMS[form](size)), 0, max_batch, 9)
    h = C.c_void_p()
    rc = lib.jn_create(C.byref(cfg), C.byref(h))
    return rc, h


def test_the_sizes_are_the_references():
    assert set(ORACLE_SIZES) | {"yolox"} == set(YOLOX_SIZES)


@pytest.mark.parametrize("form", ["encoder", "detector", "bf16"])
@pytest.mark.parametrize("size", SIZES)
def test_jn_create_plans_every_size(size, form):
    lib = _lib.load_library()
    rc, h = _create(size, form)
    assert rc == 0, lib.jn_last_error()
    lib.jn_destroy(h)


@pytest.fixture(scope="module")
def contexts():
    lib = _lib.load_library()
    handles = {}
    for size in ("yolox-m", "yolox-x"):
        for form in ("encoder", "bf16", "detector", "detector-bf16"):
            rc, h = _create(size, form, P=fp.P, max_batch=fp.MAX_BATCH)
            assert rc == 0, lib.jn_last_error()
            handles[(size, form)] = h
    yield handles
    for h in handles.values():
        lib.jn_destroy(h)


@pytest.mark.parametrize("form,net,head", [("encoder", fp.ENC, 0), ("bf16", fp.ENC, 0), ("detector", fp.DET, 0), ("detector", fp.DET, 1),
                                           ("detector-bf16", fp.DET, 1)])
@pytest.mark.parametrize("size", ["yolox-m", "yolox-x"])
def test_every_op_of_the_forward_plan_is_launched_once(contexts, size, form, net, head):
    """Dense nets: no depthwise-pointwise fusion, so nothing is absorbed; every op is one launch, no layer is deferred, and an
    upsample belongs to at most one fp32 conv."""
    f32 = not form.endswith("bf16")
    depth = {"yolox-m": 2, "yolox-x": 4}[size]
    for train in (0, 1):
        lengths = set()
        for N in (1, 16, 17, fp.MAX_BATCH):
            steps = fp.plan(contexts[(size, form)], net, N, train, head, 0)
            lengths.add(len(steps))
            for i, (route, link, deferred) in enumerate(steps):
                assert route in (fp.STEM, fp.CONV, fp.SPP, fp.UPSAMPLE, fp.ADDACT, fp.PRED), (i, route)      # nothing fused, nothing absorbed
                assert not deferred
                if link >= 0:
                    assert route == fp.CONV and f32 and steps[link][0] == fp.UPSAMPLE and link > i
            cands = [l for r, l, _ in steps if r == fp.CONV and l >= 0]
            assert len(cands) == len(set(cands))
            got = {r: sum(s[0] == r for s in steps) for r in (fp.STEM, fp.SPP, fp.UPSAMPLE, fp.ADDACT, fp.PRED)}
            # shortcut sums: the bottlenecks of dark2 .. dark4 (depth, 3 depth, 3 depth); dark5 and the PAFPN blocks have none
            assert got == {fp.STEM: 1, fp.SPP: 1, fp.UPSAMPLE: 2, fp.ADDACT: 7 * depth, fp.PRED: 3 if head else 0}, got
        assert len(lengths) == 1      # the plan of a dense net does not move with N


def _conv_shapes(size, P=64):
    """Every distinct Conv2d launch of the oracle's backbone, PAFPN and head over one P x P patch: (k, stride, groups, cin, cout, H, W,
    bias) with H x W the INPUT map, and the SPP's (hidden channels, H, W)."""
    net = yolox_ref.build_yolox(size, 2).eval()
    rec, spp = set(), []
    for m in net.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.register_forward_hook(lambda m, i, o: rec.add((m.kernel_size[0], m.stride[0], m.groups, m.in_channels, m.out_channels, i[0].shape[2],
                                                            i[0].shape[3], m.bias is not None)))
        if isinstance(m, yolox_ref.SPPBottleneck):
            m.register_forward_hook(lambda m, i, o: spp.append((m.conv1.conv.out_channels, i[0].shape[2], i[0].shape[3])))
    with torch.no_grad():
        net.head.raw_maps(net.backbone(torch.rand(1, 3, P, P)))
    return sorted(rec), spp


@pytest.mark.parametrize("size", ORACLE_SIZES)
def test_the_route_entries_admit_every_conv_of_the_oracle_net(size):
    """At (2 patches, 64 px) and (64 patches, 448 px): forward fp32 and bf16, the data gradient (plain and accumulating) and, for the dense
    3 x 3 convs, the weight gradient.  The head's predictors (1x1 convs with a bias and 4, 1 or nclasses outputs) are head_pred_kernel's,
    the stem conv (12 input channels after Focus) the stem kernels': neither has a route entry."""
    lib = _lib.load_library()
    convs, spp = _conv_shapes(size)
    seen = set()
    for k, stride, groups, cin, cout, H, W, bias in convs:
        if bias or cin == 12:
            continue
        seen.update((cin, cout))
        for N, mul in ((2, 1), (64, 7)):
            h, w = H * mul, W * mul
            if k == 1:
                for di, do, bf, tr, acc in ((0, 0, 0, 0, 0), (1, 1, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 1, 1)):
                    a, b = (cout, cin) if tr else (cin, cout)
                    assert lib.jn_pw_route(N, h, w, a, b, a, b, di, do, bf, tr, acc, 0, 0, 1, 0, 0, None) >= 1, (size, cin, cout, N, h, tr, lib.jn_last_error())
            elif groups == 1:
                for kind in (0, 1 if stride == 1 else 2, 3):
                    la, lb = (cin, cout) if kind <= 1 else (cout, cin)
                    assert lib.jn_conv3_route(kind, N, h, w, cin, cout, stride, 1, la, lb) >= 1, (size, kind, cin, cout, N, h, lib.jn_last_error())
            else:
                assert groups == cin == cout
                for dt in (0, 1):
                    assert lib.jn_dw3x3_route(N, cin, stride, dt) >= 1, (size, cin, stride, dt)
    for hid, H, W in spp:
        for N, mul in ((2, 1), (64, 7)):
            for dt, bwd in ((0, 0), (1, 0), (0, 1)):
                assert lib.jn_spp_route(dt, 4 * hid, hid, H * mul, W * mul, N, bwd) >= 1, (size, hid, H * mul, N, dt, bwd)
    want = {"yolox-tiny": {24, 48, 96, 192, 384, 768}, "yolox-m": {48, 96, 192, 384, 768, 1536}, "yolox-x": {80, 160, 320, 640, 1280, 2560}}
    assert want.get(size, set()) <= seen, (size, sorted(seen))
