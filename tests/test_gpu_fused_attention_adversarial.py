"""GPU (-m gpu): the three attention paths whose softmax lives inside a kernel that does something else as well, per segment on adversarial
inputs — T2V_EPI_TATTN (gemm2.hip tile 10: QKV projection + temporal self-attention), T2V_EPI_XATTN (t2v_epilogue_xattn on gemm2 tiles 8,
11, 5 and gemm.hip tile 0) and T2V_OP_ATTENTION with two roles on all three attn_kernel variants.

The inputs (tests/fused_attention_inputs.py; tests/test_fused_attention_inputs_cpu.py proves on the CPU what they do) place the logits
through the GEMMs with selection weights, so q, k, v are chosen fp16 values: every segment — TATTN (sample, pixel, head), XATTN (32-row
strip, head), two roles (outer sample, inner, head) — looks along its own orthonormal directions, peaks on its own key, carries its own
power-of-two scale, and has a logit 40 log2 units up where the kernel must not see it: in the next pixel's rows of the LDS image (the masked
key slots F .. 31 of TATTN), in the key row that follows a sample's last key (XATTN, two roles).  TATTN: 60 to 192 live rows of a tile,
ragged last tiles, sample seams, 0 / 1 / 8 / 30 masked slots, tpix 6 / 8 / 11 / 12, and two dense K = 320 cases with five column tiles.
XATTN: 1, 7, 32, 33, 64, 65, 77 and 96 keys, a sample seam inside a row tile, a_wrap, K as a column window of a wider buffer, V^T with
+- 32768 in the padding columns and NaN directly behind every sample's rows.  Two roles: key counts (154, 77), (77, 154), (24, 40),
(40, 24), (24, 20), (33, 32), (77, 40), one and two samples per role, running maxima that advance in the second role.

`harness.run_both` only executes; every expected value is adversarial.softmax_attention_ref (float64, explicit formula).  Every tensor is a
window of a larger NaN allocation; outputs start as NaN and must come back finite with every fence element still NaN.  Errors are one
rel-L2 per segment and the assert is on the worst segment at adversarial.TOL_HI = 2e-3, the suite's figure for these kernels' fp16 output
against an explicit reference.  Rows on which one visible key stands >= 30 log2 units above the rest (float64) equal that key's v bit for bit
(every row of the one-key case).  The pair launch of a two-role case equals the two single-role launches bit for bit.  Measured values:
profiles/fused_attention_adversarial.txt."""
import pytest

import fused_attention_inputs as FA
from harness import run_both
from interp import Interp
from interp_prompt import PromptInterp
from sd_webui_text2video_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", FA.CASES, ids=lambda c: c["id"])
def test_fused_attention_paths_per_segment_on_adversarial_inputs(c):
    b = FA.build(c)
    _, got, _, _ = run_both(b.P, b.w, {}, b.init, interp=PromptInterp if b.interp == "PromptInterp" else Interp)
    figs = FA.verify(got, b)
    L.async_status()
    print(FA.figures_line(b, figs))
    if c["family"] == "two_role":
        FA.verify_pair_equals_singles(got, b)
    if c["family"] == "xattn" and c["Lc"] == 1:
        assert figs["exact"] == c["B"] * c["rows"] * (c["N"] // 64)
    if c.get("variant") == "masked" or c.get("wrap"):
        assert figs["exact"] > 0
