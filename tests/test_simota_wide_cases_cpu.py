"""CPU only, oracle only: the committed wide SimOTA cases (tests/simota_wide_cases.py: 9 to 64 boxes in a patch) mean
something before the wide kernel sees them.  Every case is admissible under the margins of tests/simota_cases.py, an fp32
evaluation of the oracle assigns as the fp64 one does and stays inside the EXISTING bars, and the list reaches what a cut
to eight boxes would get wrong.  Plus the part of the opt-in's contract that needs no GPU."""
import re
from pathlib import Path

import pytest
import torch

from tests import simota_cases as sc
from tests import simota_wide_cases as wc

ROOT = Path(__file__).resolve().parents[1]


def test_every_wide_case_is_admissible():
    for case in wc.ALL:
        m = wc.margins(case)
        assert sc.admissible(m), (case, {k: m[k] for k in "abcde"})
    assert len(set(wc.ALL)) == len(wc.ALL) and not set(wc.ALL) & set(sc.CASES)
    assert all(c.P <= 448 and c.N <= 3 for c in wc.ALL)
    # the zero row in front is taken as a box, the last real row is not
    _, tg = wc.build(wc.ZERO_FIRST_WIDE)
    t = wc.margins(wc.ZERO_FIRST_WIDE)["patches"][0]
    real = (sc.to_cxcywh(tg)[0].sum(1) > 0)
    assert float(tg[0, 0].abs().sum()) == 0.0 and bool(real[1:].all()) and int(real.sum()) == tg.shape[1] - 1 >= 9
    assert t["ng"] == tg.shape[1] - 1 and wc.reference(wc.ZERO_FIRST_WIDE)["num_gt"] == t["ng"]


def test_margin_trace_agrees_with_the_oracle():
    for case in wc.ALL:
        ref, m = wc.reference(case), wc.margins(case)
        for n, t in enumerate(m["patches"]):
            assert torch.equal(t["fg"], ref["fg"][n]), (case, n)
        assert ref["num_fg"] == sum(t["nfg"] for t in m["patches"])
        assert ref["num_gt"] == sum(t["ng"] for t in m["patches"])


def test_the_wide_list_reaches_what_a_cut_to_eight_boxes_gets_wrong(capsys):
    count = dict.fromkeys(("patch with ng > 8", "patch with nc > 256", "contested anchor won by a box of index >= 8",
                           "foreground anchor matched to a box of index >= 8", "box with k >= 7", "box left without an anchor"), 0)
    ngmax = ncmax = kmax = 0
    for case in wc.ALL:
        ps, asg = wc.margins(case)["patches"], wc.assignment(case)
        for t, a in zip(ps, asg):
            wide = t["ng"] > 8
            count["patch with ng > 8"] += wide
            count["patch with nc > 256"] += t["nc"] > 256
            count["box with k >= 7"] += sum(k >= 7 for k in t["ks"])
            count["box left without an anchor"] += t["boxes_left_empty"]
            ngmax, ncmax, kmax = max(ngmax, t["ng"]), max(ncmax, t["nc"]), max([kmax] + t["ks"])
            if a is None:
                assert not wide
                continue
            late = a["matched"] >= 8
            count["foreground anchor matched to a box of index >= 8"] += int(late.sum())
            count["contested anchor won by a box of index >= 8"] += int((late & (a["claims"] > 1)).sum())
            if wide:                               # so a cut to the first eight rows changes num_fg of this patch
                assert bool(late.any()), case
            assert all(k <= 10 for k in t["ks"])
    with capsys.disabled():
        print("\nwide SimOTA case coverage (occurrences over the case list):")
        for k, v in count.items():
            print(f"  {v:5d}  {k}")
        print(f"  most boxes in a patch {ngmax}, most candidates {ncmax}, largest dynamic k {kmax}")
    assert count["patch with ng > 8"] >= 6 and count["patch with nc > 256"] >= 3, count
    assert all(v >= 1 for v in count.values()), count


def test_fp32_oracle_assigns_as_fp64_within_the_existing_bars(capsys):
    """The bars of simota_cases.py apply to the wide list unchanged: the fp32 CPU oracle itself is inside them here too."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # one summation order, whatever the machine
    try:
        worst = dict(metrics=[0.0] * 5, scale=0.0, grad_max=[0.0] * 6, grad_fg_l2=0.0)
        for case in wc.ALL:
            ref, got = wc.reference(case), wc.evaluate(case, torch.float32)
            assert torch.equal(got["fg"], ref["fg"]), case
            assert (got["num_fg"], got["num_gt"]) == (ref["num_fg"], ref["num_gt"]), case
            assert bool((got["grad"][~ref["fg"]][:, [0, 1, 2, 3, 5]] == 0).all()), case
            d = sc.distances(got, ref)
            sc.check_bars(d, case)
            worst["metrics"] = [max(a, b) for a, b in zip(worst["metrics"], d["metrics"])]
            worst["grad_max"] = [max(a, b) for a, b in zip(worst["grad_max"], d["grad_max"])]
            worst["scale"], worst["grad_fg_l2"] = max(worst["scale"], d["scale"]), max(worst["grad_fg_l2"], d["grad_fg_l2"])
    finally:
        torch.set_num_threads(threads)
    fmt = lambda vs: ", ".join(f"{v:.2e}" for v in vs)
    with capsys.disabled():
        print("\nfp32 CPU oracle, worst distance from fp64 over the wide cases (bars: those of simota_cases.py):")
        print(f"  metrics total / 5 iou / obj / cls / l1 (relative): {fmt(worst['metrics'])}   bars {fmt(sc.METRIC_RTOL)}")
        print(f"  scale (relative): {worst['scale']:.2e}   bar {sc.SCALE_RTOL:.2e}")
        print(f"  gradient columns 0-5 (max-norm / max|ref|): {fmt(worst['grad_max'])}   bars {fmt(sc.GRAD_MAX)}")
        print(f"  gradient, foreground rows, columns 0-3 and 5 (relative L2): {worst['grad_fg_l2']:.2e}   bar {sc.GRAD_FG_L2:.2e}")


# ---- the boundary of the feature (these fail without it) --------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_two_entry_points():
    from jolineedle_amd import _lib, yolox
    header = (ROOT / "include" / "jnroll.h").read_text()
    declared = set(re.findall(r"\b(jn_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load_library()
    for name in ("jn_yolox_loss_wide", "jn_set_det_loss_boxes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["jn_yolox_loss_wide"] == _lib.SIGNATURES["jn_yolox_loss"]
    assert lib.jn_abi_version() == 2                               # additive: the version and the structs did not move
    limit = int(re.search(r"#define JN_DETLOSS_MAX_BOXES (\d+)", header).group(1))
    assert yolox.MAX_BOXES_WIDE == limit >= 256
    assert yolox.DET_LOSS_BOXES == ("cap8", "all")


def test_an_unknown_policy_raises_before_any_library_call():
    from jolineedle_amd import yolox
    raw, tg = torch.zeros((1, 84, 6)), torch.zeros((1, 1, 5))      # CPU tensors: a library call would not get this far
    with pytest.raises(ValueError, match="nonsense"):
        yolox.yolox_loss(raw, tg, 64, boxes="nonsense")


def test_det_loss_boxes_survives_the_config_round_trip(tmp_path):
    import jolineedle_amd as ja
    from tests.helpers import model_config
    mc = model_config(patch_size=64, block_size=4, det_loss_boxes="all")
    tc = ja.CfgNode(patch_size=64, max_seq_len=4, work_dir=str(tmp_path), env_name="run")
    _, m2 = ja.config_from_file(ja.save_config(mc, tc))
    assert m2.det_loss_boxes == "all"
    _, m3 = ja.config_from_file(ja.save_config(model_config(patch_size=64, block_size=4), tc))
    assert getattr(m3, "det_loss_boxes", "cap8") == "cap8"


def test_the_switch_refuses_what_it_cannot_serve():
    """jn_set_det_loss_boxes on contexts planned without a GPU: JN_ESTATE (-5) without a detector, JN_EINVAL (-1) for "all"
    beyond 8400 anchors (a patch size above 640) and on a null context, JN_OK at 640 px and for the default anywhere."""
    from jolineedle_amd import _lib
    from jolineedle_amd.engine import Engine, make_jn_config
    from tests.helpers import model_config
    lib = _lib.load_library()
    mk = lambda **kw: Engine(make_jn_config(model_config(block_size=2, **kw), 0, 1, 9))
    bare = mk(patch_size=64, with_detector=False, image_processor=None)
    for flag in (0, 1):
        assert lib.jn_set_det_loss_boxes(bare.handle, flag) == -5 and b"detector" in lib.jn_last_error()
    big = mk(patch_size=672, image_processor="yolox-nano")
    assert lib.jn_set_det_loss_boxes(big.handle, 1) == -1 and b"A=9261" in lib.jn_last_error()
    assert lib.jn_set_det_loss_boxes(big.handle, 0) == 0
    edge = mk(patch_size=640, image_processor="yolox-nano")
    assert lib.jn_set_det_loss_boxes(edge.handle, 1) == 0 and lib.jn_set_det_loss_boxes(edge.handle, 0) == 0
    assert lib.jn_set_det_loss_boxes(None, 1) == -1
