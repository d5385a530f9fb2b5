"""GPU (-m gpu): every normalisation path per statistics block on adversarial inputs.

The four stand-alone GroupNorm forms (three launches, cooperative with tagged records and with the grid barrier, single launch),
gn_coop_kernel at each rows-per-thread count, the two strip folds (phase 3), the sharded phases 1 / 2 (uneven slices, producer strips, halo
rows), T2V_EPI_GN on every tile with an instantiation (whole tiles, a tile across two instances, half-tile instances, dead results, hi + lo),
splitk_gn_kernel at two rows-per-thread counts per width, and LayerNorm stand-alone (every instantiation, the grid-stride walk), fused into
whole-row tiles and across column tiles — on inputs whose blocks all differ in mean and variance and whose seam rows weigh most
(tests/norm_inputs.py; tests/test_norm_inputs_cpu.py proves on the CPU that statistics from the neighbouring block, a lost or doubled
row, an n off by one row and unweighted parts each land far outside the tolerances used here).

`harness.run_both` only executes.  Every expected value is `norm_inputs.groupnorm_ref` (float64, explicit formula), every error is one
rel-L2 per (instance, group) block — per row for LayerNorm — and the asserts are on the worst block: 1e-3 for the fp16 output, 2e-5 for
hi + lo (on `offset` rows max(2e-5, 4 x the error of torch's fp32 group_norm on the CPU for that block)), hi + lo closer than hi; casts and
stored fp32 tensors bit-equal to the designed input.  Every tensor is a window of a larger NaN allocation with ld = C + 8; outputs start as
NaN and must come back finite with every fence element still NaN.  The builder asserts from the op records which path a case names.
Measured maxima: profiles/norm_adversarial.txt.

The rows-per-thread cases mirror the launcher's chunking from the device's CU count; whether such a launch really ran co-resident (and not
on the three-launch path the launcher falls back to when the occupancy query says no) cannot be observed from outside."""
import pytest

import norm_inputs as N
from harness import run_both
from sd_webui_text2video_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", N.CASES, ids=lambda c: c["id"])
def test_norm_paths_per_block_on_adversarial_inputs(c):
    b = N.build(c, ncu=L.device_info()[1])
    _, got, _, _ = run_both(b.P, b.w, {}, b.init)
    L.async_status()
    print(N.figures_line(b, N.verify(got, b)))
