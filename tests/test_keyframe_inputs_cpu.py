"""CPU: the designed operands of the keyframe step (tests/keyframe_inputs.py) separate the contract from the wrong implementations a
kernel or a binding could be, and the restatement is the torch arithmetic of the reference's blend (modelscope/t2v_model.py:1555-1562)."""
import numpy as np
import pytest
import torch

import keyframe_inputs as KI


def _differs(a, b):
    """elements where two results differ (NaN against NaN counts as equal)"""
    return ~((a == b) | (a.isnan() & b.isnan()))


def test_special_weights_stand_where_they_decide():
    case = KI.kernel_case((2, 4, 200))
    v32 = torch.tensor(KI.V, dtype=torch.float32)
    assert float(v32) > KI.V                                        # the fp32 threshold lies above the float64 one
    for w, held in KI.special_weights():
        sel = case["mask"].isnan() if w != w else case["mask"] == w
        assert sel.sum() >= 8 and bool((case["held"][sel] == held).all()), w       # every channel of either video
    assert 0.3 < float(case["held"].float().mean()) < 0.8
    assert not torch.equal(case["mask"][0], case["mask"][1]) and not torch.equal(case["original"][0], case["original"][1])
    assert int(case["fence_orig"].sum()) == 3 and int(case["fence_x1"].sum()) == 3
    assert not (case["fence_orig"] & case["held"]).any() and (case["fence_x1"] & ~case["held"]).sum() == 0


@pytest.mark.parametrize("guided", [0, 2, 4])
def test_restatement_is_the_references_arithmetic(guided):
    case = KI.kernel_case((2, 4, 200))
    args = KI.step_args(case, guided)
    out = KI.keyframe_step(*args)
    x1 = KI.plain_step(*args[:5])
    # the reference's lines, written out with its own operators on one tensor
    binary = torch.where(case["mask"] <= KI.V, torch.zeros_like(case["mask"]), torch.ones_like(case["mask"]))
    to_inpaint = torch.tensor(KI.QCOEF[0], dtype=torch.float64) * case["original"] + case["qnoise"] * torch.tensor(KI.QCOEF[1], dtype=torch.float64)
    want = to_inpaint * (1 - binary) + x1 * binary
    assert want.dtype == torch.float32 and not _differs(out, want).any()
    clean = ~(case["fence_orig"] | case["fence_x1"])
    assert torch.equal(out[~case["held"] & clean], x1[~case["held"] & clean])                   # free: the step's own value
    assert torch.equal(out[case["held"] & clean], to_inpaint[case["held"] & clean])             # held: the re-noised original
    assert out[case["fence_orig"]].isnan().all() and out[case["fence_x1"]].isnan().all()        # arithmetic, not a select
    assert not out[clean].isnan().any()


@pytest.mark.parametrize("mutant", KI.MUTANTS)
def test_inputs_separate_the_mutants(mutant):
    case = KI.kernel_case((2, 4, 200))
    args = KI.step_args(case, 2)
    good, bad = KI.keyframe_step(*args), KI.keyframe_step(*args, mutant=mutant)
    d = _differs(good, bad)
    assert d.any(), mutant
    at = lambda w: case["mask"] == np.float32(w)
    if mutant in ("< instead of <=", "threshold compared in float64"):
        assert bool(d[at(KI.V)].all()) and int(d.sum()) == int(at(KI.V).sum())               # the weight fp32(v), and nothing else
    if mutant == "inverted polarity":
        assert bool(d[~(case["fence_orig"] | case["fence_x1"]) & ~case["mask"].isnan()].all())


def test_threshold_bits_round_trip():
    for S in (4, 5, 7, 50):
        for i in range(S - 1):
            v = (S - i - 1) / S
            assert np.array([KI.f32_bits(v)], dtype=np.int32).view(np.float32)[0] == np.float32(v)
