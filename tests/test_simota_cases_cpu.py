"""CPU only, oracle only: the committed SimOTA cases (tests/simota_cases.py) mean something before any kernel sees them.
Every case is admissible, the list walks every branch of the assignment at least twice, an fp32 evaluation of the oracle
assigns as the fp64 one does, and the bars of tests/test_gpu_simota_loss.py are 8 x the fp32 oracle's distance from fp64."""
import torch

from tests import simota_cases as sc

ALL = sc.CASES + [sc.TIE_CASE]


def test_every_committed_case_is_admissible():
    for case in sc.CASES:
        m = sc.margins(case)
        assert sc.admissible(m), (case, {k: m[k] for k in "abcde"})
    m = sc.margins(sc.TIE_CASE)
    assert sc.admissible(m, tie=True) and m["e"] == 0.0, {k: m[k] for k in "abcde"}
    assert len(set(sc.CASES)) == len(sc.CASES)
    # the shapes: one partial chunk, three chunks with level 1 starting inside the second, the headline patch size
    assert {c.P for c in sc.CASES} == {64, 160, 448}
    assert [sc.n_anchors(P) for P in (64, 160, 448)] == [84, 525, 4116]
    assert {c.N for c in sc.CASES} >= {1, 2, 3, 4, 5, 8} and {c.nb for c in sc.CASES} >= {1, 2, 3, 4, 5, 6, 8}
    assert all(1 <= c.N <= 8 and 1 <= c.nb <= 8 for c in sc.CASES)


def test_margin_trace_agrees_with_the_oracle():
    """margins() restates the assignment to read the margins off; it must be the assignment the oracle makes."""
    for case in ALL:
        ref, m = sc.reference(case), sc.margins(case)
        for n, t in enumerate(m["patches"]):
            assert torch.equal(t["fg"], ref["fg"][n]), (case, n)
        assert ref["num_fg"] == sum(t["nfg"] for t in m["patches"])
        assert ref["num_gt"] == sum(t["ng"] for t in m["patches"])


def test_the_case_list_covers_every_branch_twice(capsys):
    count = dict.fromkeys(("box with k >= 2", "box with k >= 6", "box with k = 1 by the clamp (sum < 1)",
                           "contested anchor won by a box other than its first claimant", "box left without an anchor",
                           "patch with >= 150 candidates", "patch with candidates in >= 3 chunks",
                           "patch with candidates on all three levels", "empty patch beside a non-empty one",
                           "all-empty batch", "boxes but no candidate", "zero row first", "use_l1 on", "use_l1 off"), 0)
    kmax = ncmax = 0
    for case in sc.CASES:
        ps = sc.margins(case)["patches"]
        layouts = case.layout.split("+")
        count["use_l1 on" if case.use_l1 else "use_l1 off"] += 1
        count["all-empty batch"] += all(t["ng"] == 0 for t in ps)
        count["empty patch beside a non-empty one"] += any(t["ng"] == 0 for t in ps) and any(t["nfg"] > 0 for t in ps)
        for n, t in enumerate(ps):
            count["box with k >= 2"] += sum(k >= 2 for k in t["ks"])
            count["box with k >= 6"] += sum(k >= 6 for k in t["ks"])
            count["box with k = 1 by the clamp (sum < 1)"] += sum(s < 1.0 for s in t["sums"])
            count["contested anchor won by a box other than its first claimant"] += t["contested_not_first"]
            count["box left without an anchor"] += t["boxes_left_empty"]
            count["patch with >= 150 candidates"] += t["nc"] >= 150
            count["patch with candidates in >= 3 chunks"] += t["chunks"] >= 3
            count["patch with candidates on all three levels"] += t["levels"] == 3
            count["boxes but no candidate"] += t["ng"] > 0 and t["nc"] == 0
            if layouts[n % len(layouts)] == "zero-row-first":
                _, tg = sc.build(case)
                assert float(tg[n, 0].abs().sum()) == 0.0 and float(tg[n, 1].sum()) > 0.0 and t["ng"] == 1
                count["zero row first"] += 1
            kmax, ncmax = max([kmax] + t["ks"]), max(ncmax, t["nc"])
            assert t["nc"] <= 216 and all(k <= max(t["nc"] - 1, 1) for k in t["ks"])       # k never meets the nc clamp
    with capsys.disabled():
        print("\nSimOTA case coverage (occurrences over the case list):")
        for k, v in count.items():
            print(f"  {v:5d}  {k}")
        print(f"  largest dynamic k {kmax}, most candidates in a patch {ncmax}")
    short = {k: v for k, v in count.items() if v < 2}
    assert not short, short


def test_box_cap_case_holds_eleven_boxes():
    _, tg = sc.build(sc.BOX_CAP_CASE)
    rows = (sc.to_cxcywh(tg).sum(2) > 0).sum(1)
    assert tg.shape[1] == 12 and int(rows[0]) == 11 and int(rows.max()) == 11


def test_fp32_oracle_assigns_as_fp64_and_sets_the_bars(capsys):
    """The margins suffice for an fp32 evaluation: same foreground set, same counts, on every case.  Its distance from
    fp64 in every quantity the GPU test checks is what the fixed bars are 8 x of."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                      # one summation order, whatever the machine
    try:
        worst = dict(metrics=[0.0] * 5, scale=0.0, grad_max=[0.0] * 6, grad_fg_l2=0.0)
        for case in ALL:
            ref, got = sc.reference(case), sc.evaluate(case, torch.float32)
            assert torch.equal(got["fg"], ref["fg"]), case
            assert (got["num_fg"], got["num_gt"]) == (ref["num_fg"], ref["num_gt"]), case
            assert bool((got["grad"][~ref["fg"]][:, [0, 1, 2, 3, 5]] == 0).all()), case
            d = sc.distances(got, ref)
            sc.check_bars(d, case)                # the fp32 oracle itself stands 8 x inside the bars
            worst["metrics"] = [max(a, b) for a, b in zip(worst["metrics"], d["metrics"])]
            worst["grad_max"] = [max(a, b) for a, b in zip(worst["grad_max"], d["grad_max"])]
            worst["scale"], worst["grad_fg_l2"] = max(worst["scale"], d["scale"]), max(worst["grad_fg_l2"], d["grad_fg_l2"])
    finally:
        torch.set_num_threads(threads)
    fmt = lambda vs: ", ".join(f"{v:.2e}" for v in vs)
    with capsys.disabled():
        print("\nfp32 CPU oracle, worst distance from fp64 over the committed cases (bar = 8 x):")
        print(f"  metrics total / 5 iou / obj / cls / l1 (relative): {fmt(worst['metrics'])}   bars {fmt(sc.METRIC_RTOL)}")
        print(f"  scale (relative): {worst['scale']:.2e}   bar {sc.SCALE_RTOL:.2e}")
        print(f"  gradient columns 0-5 (max-norm / max|ref|): {fmt(worst['grad_max'])}   bars {fmt(sc.GRAD_MAX)}")
        print(f"  gradient, foreground rows, columns 0-3 and 5 (relative L2): {worst['grad_fg_l2']:.2e}   bar {sc.GRAD_FG_L2:.2e}")
    # the bars are the measured distances x 8 (written down to two digits), none of them wide, none above 1e-4
    pairs = list(zip(worst["metrics"], sc.METRIC_RTOL)) + list(zip(worst["grad_max"], sc.GRAD_MAX))
    pairs += [(worst["scale"], sc.SCALE_RTOL), (worst["grad_fg_l2"], sc.GRAD_FG_L2)]
    for measured, bar in pairs:
        assert bar <= 1e-4, bar
        assert 0.5 * bar <= 8.0 * measured <= 1.5 * bar, (measured, bar)
