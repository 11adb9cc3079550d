"""CPU only: the committed cases of the candidate policy "all" (tests/postprocess_all_cases.py) mean something before the
kernel sees them, and the boundary of the feature exists.  `run_all` equals the oracle (oracle/yolox_ref.py::postprocess,
which has no candidate cap, + clamp + the cut to max_out) bit for bit with no input doctored; it equals the first-2048
reference wherever at most 2048 anchors pass and differs from it on every case with more; every compared IoU is exactly
0, 1/2, 3/4 or 1; and each case reaches the branch it is named after."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import yolox_ref
from tests import postprocess_all_cases as pa
from tests import postprocess_cases as pc

F = np.float32
ROOT = Path(__file__).resolve().parent.parent


def _oracle(raw, case):
    if raw.shape[0] == 1:                          # the oracle's squeeze() needs two anchors; the second one does not pass
        raw = np.concatenate((raw, np.array([[5, 5, 4, 4, min(case.conf, 0.0) - 1.0, 1.0]], F)))
    out = yolox_ref.postprocess(torch.from_numpy(np.array(raw))[None], 1, case.conf, case.nms, class_agnostic=True)[0]
    if out is None:
        return torch.zeros((0, 7))
    out[:, :4].clamp_(0, case.P - 1)
    return out


def _same(x, y):
    return x[1] == y[1] and x[2] == y[2] and np.array_equal(x[0], y[0], equal_nan=False)


def _vs_oracle(case, raw, got):
    rows, count, (n_pass, n_keep) = got
    want = _oracle(raw, case)
    assert want.shape[0] == n_keep, case.name
    want = want[:case.max_out]
    assert count == want.shape[0] == min(n_keep, case.max_out), case.name
    assert torch.equal(torch.from_numpy(np.array(rows)).reshape(-1, 7), want), case.name
    assert rows.dtype == F and bool((rows[:, 6] == 0).all())


def test_every_case_is_admissible(capsys):
    """Run first: margins(case) is the reference run of every later test.  (b) = 0, (a) > pc.MARGIN_BAR, and the compared
    IoUs are a subset of {0, 1/2, 3/4, 1}."""
    lines = []
    for case in pa.CASES:
        m = pa.margins(case)
        lines.append(f"  {case.name:18s} pairs {m['pairs']:9d}  exactly on the threshold {m['exact']:5d}  (a) {m['a']:.3e}  "
                     f"(b) {m['b']:.3e}  IoUs {sorted(m['values'])}")
    with capsys.disabled():
        print("\npostprocess 'all' cases: (a) least |iou64 - thr| off the exact ties, (b) largest |iou32 - iou64|")
        print("\n".join(lines))
    for case in pa.CASES:
        m = pa.margins(case)
        assert m["b"] == 0.0 and m["nan"] == 0 and m["a"] > pc.MARGIN_BAR, (case.name, m)
        assert m["values"] <= {0.0, 0.5, 0.75, 1.0}, (case.name, m["values"])
        assert (m["exact"] > 0) == (case.nms == 0.5 and 0.5 in m["values"]), case.name
    assert len({c.name for c in pa.CASES}) == len(pa.CASES)
    assert sum(c.A == pa.POST_ALL_MAX_A and pa.reference(c)[2][0] > 8000 for c in pa.CASES) <= 8      # the slow ones


def test_run_all_equals_the_uncapped_oracle_on_every_new_case():
    for case in pa.CASES:
        _vs_oracle(case, pa.build(case), pa.reference(case))
    r = {c.name: pa.reference(c) for c in pa.CASES}
    assert r["count-8400"][1] == 5600 and r["count-8193"][2] == (8193, 6827) and r["all-disjoint-8400"][1] == 8400


def test_run_all_is_the_first_2048_reference_up_to_the_cap_and_the_oracle_beyond():
    beyond = []
    for case in pc.CASES:
        ref = pc.reference(case)
        got = pa.run_all(pc.build(case), case.conf, case.nms, case.P, case.max_out)
        if ref[2][0] <= pc.DET_CAP:
            assert _same(got, ref), case.name
        else:
            beyond.append(case.name)
            assert not _same(got, ref), case.name
            _vs_oracle(case, pc.build(case), got)                           # no input doctored: the oracle sees every passing anchor
            raw = pc.build(case)
            best = int(np.argmax(raw[:, 4] * raw[:, 5]))
            assert got[0][0, 4] == raw[best, 4] and got[0][0, 5] == raw[best, 5]      # the first row is the patch's best score
    assert beyond == ["cap-2049", "cap-3000"]
    got = {n: pa.run_all(pc.build(pc.BY_NAME[n]), 0.25, pc.BY_NAME[n].nms, 448, 2048)[2] for n in beyond}
    assert got == {"cap-2049": (2049, 1707), "cap-3000": (3000, 2000)}


def test_the_case_list_covers_the_counts_and_the_launches_mix_sizes():
    counts = sorted(c.args[0] for c in pa.CASES if c.kind == "lattice" and c.args[1] and c.max_out == pa.POST_ALL_MAX_A)
    assert counts == [300, 2049, 2100, 3000, 4095, 4096, 4097, 4116, 8191, 8192, 8193, 8400]
    assert {c.A for c in pa.CASES} == {2541, 4116, 8400} and max(c.A for c in pa.CASES) == pa.POST_ALL_MAX_A
    assert 2541 == sum((352 // s) ** 2 for s in (8, 16, 32)) and 8400 == sum((640 // s) ** 2 for s in (8, 16, 32))
    sizes = [len(cs) for *_, cs in pa.launches()]
    assert max(sizes) == 4 and sum(sizes) == len(pa.CASES)
    mixed = 0
    for conf, nms, P, max_out, cs in pa.launches():
        raw = pa.stack(cs)
        assert raw.shape == (len(cs), max(c.A for c in cs), 6)
        mixed += len({c.A for c in cs}) > 1 and len({pa.reference(c)[2][0] for c in cs}) > 1
        for n, c in enumerate(cs):
            if c.A < raw.shape[1]:                                 # the padding does not pass: same answer at the larger A
                assert _same(pa.run_all(raw[n], conf, nms, P, max_out), pa.reference(c)), c.name
    assert mixed >= 2


def test_every_case_reaches_its_branch():
    seen = set()
    for case in pa.CASES:
        raw = pa.build(case)
        ref = pa.reference(case)
        rows, count, (n_pass, n_keep) = ref
        score = raw[:, 4] * raw[:, 5]
        passing = np.nonzero(score >= F(case.conf))[0]
        kind = case.kind
        seen.add(kind)
        if n_pass > pc.DET_CAP:                                    # the first-2048 policy gives another answer
            assert not _same(pc.run(raw, case.conf, case.nms, case.P, case.max_out), ref), case.name
        if kind == "lattice":
            n, shadows, _ = case.args
            assert n_pass == n and len(np.unique(score[passing])) == n
            assert n_keep < n if shadows else n_keep == n == count == pa.POST_ALL_MAX_A
            if n > pc.DET_CAP:                                     # the best score sits on the last passing anchor and is row 0
                best = int(np.argmax(score))
                assert best == passing[-1] and rows[0, 4] == raw[best, 4] and rows[0, 5] == raw[best, 5]
            if case.name == "max-out-64":
                assert count == 64 < n_keep == 2000
            if case.P == 640 and not shadows:
                assert rows[:, 2].max() == 639 and pc.xyxy(raw)[passing, 2].max() == 640      # the clamp has work to do
        elif kind == "copies":
            assert n_pass == case.A == pa.POST_ALL_MAX_A and count == n_keep == 1 and rows[0, 4] * rows[0, 5] == score.max() == score[-1]
        elif kind == "ties-far":
            other = pa.run_all(raw, case.conf, case.nms, case.P, case.max_out, tie_high_index=True)
            assert other[1] == count and not _same(other, ref)     # as many survivors, other boxes
            e = pc.xyxy(raw)
            kept, kept_hi = {tuple(r[:4]) for r in rows}, {tuple(r[:4]) for r in other[0]}
            for a0, _, _ in pa.TIE_PAIRS:
                assert score[a0] == score[a0 + 1] and int((score == score[a0]).sum()) == 2
                assert tuple(e[a0]) in kept and tuple(e[a0 + 1]) not in kept
                assert tuple(e[a0]) not in kept_hi and tuple(e[a0 + 1]) in kept_hi
            assert [a0 + 1 for a0, _, _ in pa.TIE_PAIRS] == [2048, 4096, 8192]
        elif kind == "negative":
            assert n_pass == case.A == count and bool((score < 0).all()) and case.A & (case.A - 1) != 0
            # a pad of score 0 (for one that ranks last) would outrank every candidate
            pads = [(0.0, 0x7fffffff)] * ((1 << int(case.A).bit_length()) - case.A)
            order = sorted([(float(s), a) for a, s in enumerate(score)] + pads, key=lambda t: (-t[0], t[1]))
            assert all(a == 0x7fffffff for _, a in order[:len(pads)])
        elif kind == "empty":
            assert (count, n_pass, n_keep) == (0, 0, 0)
        elif kind == "last":
            assert n_pass == count == 1 and passing[0] == case.A - 1 == 8399
    assert seen == {c.kind for c in pa.CASES} and len(seen) == 6


# ---- the boundary of the feature (these fail without it) --------------------------------------------------------------
def test_the_header_declares_and_the_library_exports_the_two_entry_points():
    from jolineedle_amd import _lib
    header = (ROOT / "include" / "jnroll.h").read_text()
    declared = set(re.findall(r"\b(jn_[a-z_0-9]+)\s*\(", header))
    lib = _lib.load_library()
    for name in ("jn_postprocess_all", "jn_set_det_candidates"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.SIGNATURES["jn_postprocess_all"] == _lib.SIGNATURES["jn_postprocess"]
    assert lib.jn_abi_version() == 2                               # additive: the version and the structs did not move
    assert "jn_postprocess_all" in header[:header.index("int jn_postprocess(")]        # the capped entry points to the other
    assert "8400" in header[header.index("int jn_postprocess("):header.index("int jn_postprocess_all(")]


def test_an_unknown_policy_raises_before_any_library_call():
    from jolineedle_amd import yolox
    raw = torch.zeros((1, 4, 6))                                   # a CPU tensor: a library call would not get this far
    with pytest.raises(ValueError, match="nonsense"):
        yolox.postprocess(raw, 0.25, 0.45, 64, 4, candidates="nonsense")
    assert yolox.DET_CANDIDATES == ("first2048", "all")


def test_det_candidates_survives_the_config_round_trip(tmp_path):
    import jolineedle_amd as ja
    from tests.helpers import model_config
    mc = model_config(patch_size=64, block_size=4, det_candidates="all")
    tc = ja.CfgNode(patch_size=64, max_seq_len=4, work_dir=str(tmp_path), env_name="run")
    _, m2 = ja.config_from_file(ja.save_config(mc, tc))
    assert m2.det_candidates == "all"
    _, m3 = ja.config_from_file(ja.save_config(model_config(patch_size=64, block_size=4), tc))
    assert getattr(m3, "det_candidates", "first2048") == "first2048"


def test_the_switch_refuses_what_it_cannot_serve():
    """jn_set_det_candidates on contexts planned without a GPU: JN_ESTATE (-5) without a detector, JN_EINVAL (-1) for "all"
    beyond 8400 anchors (a patch size above 640) and on a null context, JN_OK at 640 px and for the default anywhere."""
    from jolineedle_amd import _lib
    from jolineedle_amd.engine import Engine, make_jn_config
    from tests.helpers import model_config
    lib = _lib.load_library()
    mk = lambda **kw: Engine(make_jn_config(model_config(block_size=2, **kw), 0, 1, 9))
    bare = mk(patch_size=64, with_detector=False, image_processor=None)
    for flag in (0, 1):
        assert lib.jn_set_det_candidates(bare.handle, flag) == -5 and b"detector" in lib.jn_last_error()
    big = mk(patch_size=672, image_processor="yolox-nano")
    assert lib.jn_set_det_candidates(big.handle, 1) == -1 and b"A=9261" in lib.jn_last_error()
    assert lib.jn_set_det_candidates(big.handle, 0) == 0
    edge = mk(patch_size=640, image_processor="yolox-nano")
    assert lib.jn_set_det_candidates(edge.handle, 1) == 0 and lib.jn_set_det_candidates(edge.handle, 0) == 0
    assert lib.jn_set_det_candidates(None, 1) == -1
