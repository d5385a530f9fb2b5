"""GPU (-m gpu): every kernel of csrc/elementwise.hip but embed_rows / reshard_rows / resample, and softmax_rows_kernel, per segment on
adversarial inputs.

Both layout conversions (the sample wrap b % Bsrc, both places of the low-order image, padded and unpadded rows, fp16 and fp32), time_embed
(a ragged last workgroup, t = 0), copy2d (every dtype pair and activation, the low-order image, the concat window, in place), the row softmax
(fewer columns than threads, the maximum in the ragged tail, a constant row), the DDIM update through samplers._ddim_update /
_ddim_update_blend (both modes, guided / partly guided / unguided, several samples per batch, fp16 and fp32 eps and x, with and without
noise, the known-region blend with and without q-noise; coefficients of the first, a middle and the last step of a 50-step run on the SD
schedule, guidance scales 9 and 1), lincomb through samplers._lincomb (1 - 6 mixed terms, a cancelling pair), to_uint8 (all four kernels in
three addressings, bgr on / off, on a table that sits on every truncation boundary), depth_tokens (extremes at the seams of the reduction, a
constant frame, a NaN pixel) and avgpool2 (either and both outputs, odd H and W) — and for every kernel with a grid-stride loop one `*-wrap`
case of just over 8192 x 256 work units, which executes the loop's second pass.

Inputs, float64 references and checks are tests/elementwise_inputs.py (tests/test_elementwise_inputs_cpu.py proves on the CPU that a value
taken from the neighbouring sample, channel, frame, row or term, a wrong leading dimension, a dropped low-order image, the other mode's
formula, rounding instead of truncating ... each land far outside the bounds used here).  `harness.run_both` only executes; the sampler ops
run on views into larger NaN-filled device tensors.  Every expected value comes from `elementwise_inputs`, never from the interpreter;
every error is per segment and asserted on the worst one; every tensor is a window of a larger NaN (bytes: 0xA5) allocation, outputs start
as NaN and must come back finite with every fence element untouched.  The builder asserts from the op record which kernel variant a case
reaches.  Measured maxima: profiles/elementwise_adversarial.txt."""
import pytest
import torch

import elementwise_inputs as E
from harness import run_both
from interp import Interp
from interp_adapter import AdapterInterp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", E.CASES, ids=lambda c: c["id"])
def test_elementwise_kernels_per_segment_on_adversarial_inputs(c):
    b = E.build(c)
    if b.ops is None:
        _, got, _, _ = run_both(b.P, b.w, {}, b.init, interp=AdapterInterp if b.adapter else Interp)
    else:                                       # a sampler binding on fenced device tensors
        dev = torch.device("cuda:0")
        bigs = {k: e["big"].to(dev) for k, e in b.ext.items()}
        b.call(samplers, {k: b.xview(k, bigs[k]) for k in bigs})
        torch.cuda.synchronize()
        for k in bigs:
            b.ext[k]["big"] = bigs[k].cpu()
        got = None
    L.async_status()
    print(E.figures_line(b, E.verify(got, b)))
