"""CPU: the float64 restatement of FreeU (tests/freeu_ref.py) in its two forms, and the proof that the designed operands of
tests/freeu_inputs.py expose every mutant of it — so that the GPU tests, which run the kernel on those operands, mean what they say."""
import pytest
import torch

import freeu_inputs as FI
import freeu_ref as FR

EXPOSED = 1e-2          # a mutant must move some output by at least this: five orders above the fp32 gates of the GPU tests


@pytest.mark.parametrize("hw", FR.SHAPES)
def test_closed_form_equals_the_fft_formulation(hw):
    H, W = hw
    v = torch.randn(3, 5, H, W, dtype=torch.float64, generator=torch.Generator().manual_seed(H * 100 + W))
    for scale in (0.9, 0.2, 1.0, 0.0, 1.7):
        d = (FR.fourier_filter_closed(v, scale) - FR.fourier_filter_fft(v, scale)).abs().max().item()
        assert d <= 1e-13, (hw, scale, d)


def test_fp32_fft_formulation_is_near_float64():
    """The gate of the GPU tests is taken from this error: it must be the rounding of fp32, not something else."""
    for H, W in FR.SHAPES:
        v = torch.randn(4, 6, H, W, generator=torch.Generator().manual_seed(H + 31 * W))
        e = (FR.fourier_filter_fft(v, 0.25).double() - FR.fourier_filter_fft(v.double(), 0.25)).abs().max().item()
        assert e <= 4e-6 and (e > 0 or H * W == 1), (H, W, e)          # (one pixel and a scale of 0.25: every step is exact)


@pytest.mark.parametrize("mutant", FR.MUTANTS)
def test_every_mutant_is_caught_by_its_named_input(mutant):
    name, geom = FI.CATCHES[mutant]
    assert geom in FI.GEOMS and name in FI.NAMES
    X = FI.operand(name, geom)
    c_total = geom[3] + geom[4]
    good, bad = FI.reference(X, geom), FI.reference(X, geom, variant=mutant)
    d = (good - bad)[:, :c_total].abs().max().item()
    assert d >= EXPOSED, (mutant, name, geom, d)


def test_stage_values_exchanged_is_caught():
    dim, f = 64, FR.MODELSCOPE
    assert FR.stage_gains(4 * dim, dim, f) == (f["b1"], f["s1"]) and FR.stage_gains(2 * dim, dim, f) == (f["b2"], f["s2"])
    assert FR.stage_gains(dim, dim, f) is None and FR.stage_gains(3 * dim, dim, f) is None
    assert FR.stage_gains(4 * dim, dim, f, exchanged=True) == (f["b2"], f["s2"]) != FR.stage_gains(4 * dim, dim, f)


@pytest.mark.parametrize("geom", FI.GEOMS)
@pytest.mark.parametrize("name", ["cos_y", "cos_x", "cos_minus", "cos_plus"])
def test_designed_planes_come_back_times_their_factor(name, geom):
    frames, h, w, c_h, c_s = geom
    k = FI.expected_factor(name, h, w, FI.S)
    if k is None:
        return                      # (an axis shorter than 3: the pattern is not a pair of bins there; the noise operand covers the size)
    X = FI.operand(name, geom)
    out = FI.reference(X, geom)
    sk = slice(c_h, c_h + c_s)
    s32 = float(torch.tensor(FI.S, dtype=torch.float32))
    k = 1.0 if name == "cos_minus" else (s32 + 1.0) / 2.0
    # The operand is the pattern rounded to fp32: X = pattern + e with |e| <= 2^-24 |pattern|, and e is in every bin.  The filter is
    # linear and moves no element by more than |e|max + 4 |s - 1| |e|max (four bins, each a mean of |e|), so out - k X is within
    # (1 + 4 |1 - s| + k) 2^-24 max|X| of zero.  A wrong factor would be off by 0.375 max|X|.
    bound = (1.0 + 4.0 * abs(1.0 - s32) + k) * 2.0 ** -24 * X[:, sk].abs().max().item()
    assert (out[:, sk] - k * X[:, sk].double()).abs().max().item() <= bound
    # and the buffer's other parts: half of the stream scaled, the other half and the guard columns as they were
    b32 = float(torch.tensor(FI.B, dtype=torch.float32))
    assert torch.equal(out[:, :c_h // 2], X[:, :c_h // 2].double() * b32) and torch.equal(out[:, c_h // 2:c_h], X[:, c_h // 2:c_h].double())
    assert torch.isnan(out[:, c_h + c_s:]).all()


def test_frames_and_channels_are_independent():
    """A NaN in one (frame, channel) plane stays there."""
    geom = (3, 3, 5, 64, 96)
    frames, h, w, c_h, c_s = geom
    X = FI.operand("noise", geom)
    clean = FI.reference(X, geom)
    X[1 * h * w + 7, c_h + 5] = float("nan")
    out = FI.reference(X, geom)
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[h * w:2 * h * w, c_h + 5] = True
    hit[:, c_h + c_s:] = True          # (the guard columns are NaN in both)
    assert torch.isnan(out[h * w:2 * h * w, c_h + 5]).all() and torch.equal(out[~hit], clean[~hit])
