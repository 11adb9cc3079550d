"""The decision-side training kernels (csrc/kernels_train.hip), one launch each on caller tensors through jn_reinforce_loss,
jn_logits_grad, jn_ce_loss and jn_adamw, against the fp64 references of tests/train_cases.py: the losses as torch-fp64 statements
of their formulas differentiated by autograd, AdamW as torch.optim.AdamW on fp64 CPU tensors.  The bars are those of
train_cases.py: 4 x the distance of a plain fp32 restatement from the same reference (test_train_cases_cpu.py measures them and
shows that they bite).  Every output is a canary-filled tensor one row (AdamW: one element) longer than the kernel may write.

Beside the bars, exactly: rows that are not counted (masked, or t >= S) are zero, an empty mask gives dlogits of zeros and the
0 / 0 of the reference, metrics[5] is S, a token with both upstream gradients 0 gives a zero row, the constructed tie goes to the
first maximum and the accuracy is one fp32 division of the hit count.

AdamW.  Before this pin the launcher formed 1 - beta and both bias corrections in fp32 from 0.9f and 0.999f.  0.999f is
0.99900001287, so 1 - beta2 was 1.3e-5 below 0.001 and v came out 1.3e-5 low in every case (bar 2e-6).  From zero moments the fp32
bias correction of step 1 is that same number and the first update is right (the 6e-6 first-step error one derives from the bias
correction alone is not there); the update is off wherever the correction does not share v's factor: at later steps, and from
pre-loaded moments at any step.  Now 1 - beta, lr / bc1 and sqrt(bc2) are formed in double and rounded once.

Measured on one MI355X, worst of the cases (bar):
  before, AdamW   p 9.8e-06 (3e-6)   v 1.3e-05 (2e-6)   all 23 cases over a bar (p at the single steps 1 / 2 / 10 / 1000 from pre-loaded
                  moments: 6.8e-6 / 9.8e-6 / 4.5e-6 / 3.9e-6; five steps from zero: 1.7e-6 ... 7.6e-6)
  after,  AdamW   p 7.0e-07 (3e-6)   m 3.7e-07 (2e-6)   v 4.0e-07 (2e-6)    (the bits of the fp32 restatement: no contraction in the kernel)
  REINFORCE       l2 1.7e-07 (7e-7)  mx 4.1e-07 (2e-6)  met 4.3e-07 (3e-6);  logits x 30: 5.0e-07 (2e-6), 1.5e-06 (6e-6), 4.3e-07 (4e-6)
  logits_grad     l2 3.7e-07 (2e-6)  mx 1.0e-06 (3e-6);                      logits x 30: 6.2e-07 (3e-6), 1.9e-06 (8e-6)
  cross-entropy   l2 1.8e-07 (2e-6)  mx 5.2e-07 (3e-6)  met 3.4e-07 (3e-5);  logits x 30: 5.5e-07 (3e-6), 3.5e-06 (2e-5), 1.4e-06 (2e-4)
The 81 tests of this file take 4 s."""
import numpy as np
import pytest
import torch

from jolineedle_amd import _lib
from jolineedle_amd._lib import check, ptr
from tests import train_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _canary(rows, cols):
    return torch.full((rows + 1, cols), tc.CANARY, device=DEV)


def _stream():
    return _lib.current_stream(torch.device(DEV))


def _run(c):
    """The case's kernel: {"dlogits" [B, T, nA], "metrics"} on the CPU; the canary rows are checked here."""
    lib, d = _lib.load_library(), tc.inputs(c)
    B, T, nA = c.B, c.T, c.nA
    lg, act, nd = _dev(d["logits"]), _dev(d["actions"]), _dev(d["n_done"])
    dl = _canary(B * T, nA)
    out = {}
    if c.kind == "rf":
        met = _canary(1, 6)
        ret, rew, mk = _dev(d["returns"]), _dev(d["rewards"]), _dev(d["masks"])
        check(lib.jn_reinforce_loss(ptr(lg), ptr(act), ptr(ret), ptr(rew), ptr(mk), ptr(nd), B, T, nA, c.norm, d["ret_mean"], d["ret_std"], d["ew"],
                                    c.scale, ptr(dl), ptr(met), _stream()), "jn_reinforce_loss")
    elif c.kind == "lg":
        met = None
        glp, gh = _dev(d["dlogprobs"]), _dev(d["dentropies"])
        check(lib.jn_logits_grad(ptr(lg), ptr(act), ptr(glp), ptr(gh), ptr(nd), B, T, nA, ptr(dl), _stream()), "jn_logits_grad")
    else:
        met = _canary(1, 3)
        tg, mk = _dev(d["target"]), _dev(d["masks"])
        check(lib.jn_ce_loss(ptr(lg), ptr(tg), ptr(mk), B, T, nA, c.sw, ptr(dl), ptr(met), _stream()), "jn_ce_loss")
    assert bool((dl[-1] == tc.CANARY).all()), "the row past dlogits was written"
    out["dlogits"] = dl[:-1].view(B, T, nA).cpu()
    if met is not None:
        assert bool((met[-1] == tc.CANARY).all()), "the row past the metrics was written"
        out["metrics"] = met[0].cpu().tolist()
    return out


@pytest.mark.parametrize("c", tc.LOSS_CASES, ids=tc.case_id)
def test_loss_kernel_against_fp64(c):
    ref, got = tc.reference(c), _run(c)
    d = tc.distances(c, got, ref)
    print(f"{tc.case_id(c)}: " + ", ".join(f"{k} {v:.2e} (bar {tc.bars(c)[k]:.0e})" for k, v in d.items()))
    dl = got["dlogits"]
    assert not torch.isnan(dl).any()
    # exactly: the rows that are not counted
    sel = ref["sel"]
    assert not dl[~sel].any(), "a row that is not counted is not zero"
    if c.kind in ("rf", "lg"):
        assert not dl[:, ref["S"]:].any()
    if c.kind == "rf":
        assert got["metrics"][5] == float(ref["S"])
        assert got["metrics"][4] == float(np.float32(int(sel.sum())) / np.float32(c.B))      # the counted tokens only, S applied
    if c.kind == "lg":
        for i in tc.inputs(c)["zero_rows"]:
            assert not dl.view(-1, c.nA)[i].any()
    if c.kind == "ce":
        n, hits = ref["n"], ref["hits"]
        if n:
            assert got["metrics"][1] == float(np.float32(hits) / np.float32(n))      # the first maximum of the tie is the prediction
            assert got["metrics"][2] == float(np.float32(n) / np.float32(c.B))
    if c.mask == "none":
        assert not dl.any()
        assert all(np.isnan(a) == np.isnan(b) for a, b in zip(got["metrics"], ref["metrics"])) and np.isnan(got["metrics"][0])
    assert not tc.over_bars(c, got, ref), tc.over_bars(c, got, ref)


def test_a_second_launch_gives_the_same_bits():
    """No atomics in the two one-workgroup kernels: ordered sums."""
    for c in (tc._case("rf", 65, 20, mask="holes", stop=2), tc._case("ce", 65, 20, mask="holes")):
        a, b = _run(c), _run(c)
        assert torch.equal(a["dlogits"], b["dlogits"])
        assert np.array_equal(np.array(a["metrics"], dtype=np.float32).view(np.int32), np.array(b["metrics"], dtype=np.float32).view(np.int32))


def _adam_run(c):
    """The case's steps through jn_adamw, the state carried on the device: [{"p", "m", "v"}] on the CPU per step."""
    lib, d = _lib.load_library(), tc.adam_inputs(c)
    n = c.n
    state = {}
    for k in ("p", "m", "v"):
        state[k] = torch.full((n + 1,), tc.CANARY, device=DEV)
        state[k][:n] = d[k].to(DEV)
    out = []
    for i, g in enumerate(d["g"]):
        gd = torch.cat([g, torch.tensor([tc.CANARY])]).to(DEV)
        check(lib.jn_adamw(ptr(state["p"]), ptr(gd), ptr(state["m"]), ptr(state["v"]), n, tc.LR, c.wd, d["first"] + i, c.clip, c.gs, _stream()),
              "jn_adamw")
        for k in ("p", "m", "v"):
            assert float(state[k][n]) == tc.CANARY, f"the element past {k} was written"
        out.append({k: state[k][:n].cpu() for k in ("p", "m", "v")})
    return out


@pytest.mark.parametrize("c", tc.ADAM_CASES, ids=tc.case_id)
def test_adamw_kernel_against_torch_adamw_in_fp64(c):
    ref, got = tc.adam_reference(c), _adam_run(c)
    d = tc.adam_distances(got, ref)
    print(f"{tc.case_id(c)}: " + ", ".join(f"{k} {v:.2e} (bar {tc.AD_BAR[k]:.0e})" for k, v in d.items()))
    for st in got:
        assert not any(torch.isnan(st[k]).any() for k in st)
    assert not tc.adam_over_bars(got, ref), tc.adam_over_bars(got, ref)
