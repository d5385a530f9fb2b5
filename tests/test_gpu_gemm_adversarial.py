"""GPU (-m gpu): every GEMM path per row segment on adversarial inputs.

Every instantiation — gemm.hip at both widths (128x64, 128x128) and gemm2.hip's tiles 1, 2, 3, 4, 5, 8, 9, 11, 12 — on M = BM + 37 (a whole
tile, a 32-row block, a 5-row block, dead blocks) x N = BN + 36 (a whole column tile, a block, one quad) with 6 k-tiles (the ring wraps) and
with one; gemm.hip's K tails (K = 200, K = 8) and N = 4; split-K with a shorter last split (25 k-tiles as 9 + 9 + 7, 17 as 9 + 8) through
the reduction kernel and through the ticket fold with every epilogue feature behind it; bias along M, ReLU, a_wrap and res_wrap with the wrap
inside a 32-row block; the residual wrap of the convolution gathers with and without split-K; the 3x3 gather (5 x 7 images, stride 1 / 2,
nearest x 2, padding (0, 1, 0, 1), Cin = 64 / 128), the C8 stem and the temporal gather (zero-padded and halo layouts) on every tile;
EPI_STATS with a ragged last strip; out_lo; the two-pass a_lo / weight_lo forms; and the fp32 accumulate on `offset` rows — on inputs whose
rows and column quads all differ in scale and whose seams weigh most (tests/gemm_inputs.py; tests/test_gemm_inputs_cpu.py proves on the CPU
that a leaking neighbour row, a lost K tail, a k-tile lost or doubled between splits, a residual, row-bias or bias index that is off, a
padding read from the neighbouring pixel or clip, a column quad that went through fp16, a missing low-order image and a strip that counts a
dead row each land far outside the tolerances used here, where one rel-L2 over the tensor would have passed most of them).

`harness.run_both` only executes.  Every expected value is float64 (A @ W.T, F.conv2d, F.conv3d on the unpacked weights + the epilogue
written out), every error is one rel-L2 per row segment (row m x the 32 columns of one accumulator block) and the asserts are on the worst
segment: max(2e-5, 4 x the same segment's error of torch's fp32 CPU result) for fp32 outputs, strips and hi + lo (hi + lo closer than hi
in every segment), 1e-3 for fp16 outputs, max(1e-3, 4 x torch's fp32 GEGLU rounded to fp16) for GEGLU.  Every tensor is a window of a larger
NaN allocation (ld = cols + 8); outputs start as NaN and must come back finite with every fence element still NaN.  The builder asserts
from the op records which path a case names.  Measured maxima: profiles/gemm_adversarial.txt."""
import pytest

import gemm_inputs as G
from harness import run_both
from sd_webui_text2video_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["id"])
def test_gemm_paths_per_row_segment_on_adversarial_inputs(c):
    b = G.build(c)
    _, got, _, _ = run_both(b.P, b.w, {}, b.init)
    L.async_status()
    print(G.figures_line(b, G.verify(got, b)))
