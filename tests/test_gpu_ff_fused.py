"""GPU (-m gpu): the C = 320 GEGLU feed-forward pair as ONE launch (csrc/gemm2.hip ff_fused_kernel) against the same two records as two.

A plan whose records k, k + 1 are the GEGLU GEMM (N = 2560, K = 320) and the projection that reads exactly its result (N = 320, K = 1280)
runs them as one launch in which the [M, 1280] hidden tensor never leaves the chip (csrc/executor.hip ff_pair).  The recognition's row
cut-off (M >= 49152) sits in front of the kernel; the programs here set i[31] = 1 on the GEGLU record — a word no validation reads, which
waives the cut-off — so that the kernel is reached at M = 192 (one tile), 200 (a ragged second tile) and 576 (three tiles).

Every case (tests/ff_fused_inputs.py: chunk-distinct scales in W1 and W2, each bias present / absent, residual present / absent / wrapped at
M / 2, fp16 hi + lo and plain fp16 output, every buffer a window of a NaN allocation) runs in the same process from the same initial arena
  fused       records [geglu, projection] adjacent;      run_timed reports the projection at exactly 0.0 ms (the fused marker)
  two-launch  [geglu, MEMSET of a scratch buffer, projection];      the projection's time is > 0
and asserts
  (a) the stored output images (hi, and lo where present) are bit-identical;
  (b) both are within 1e-3 per row segment (the suite's fp16-output figure, tests/gemm_inputs.py) of the float64 reference that rounds the
      hidden tensor to fp16 — tests/test_ff_fused_inputs_cpu.py shows what that bound sees (a dropped / repeated chunk, swapped halves:
      90 .. 2500 x outside) and what only (a) sees (a hidden tensor that is not rounded);
  (c) every fence element is still NaN; the hidden window is finite after the two-launch run and UNTOUCHED after the fused run (the fused
      pair does not write it: include/t2v_hip.h);
  (d) the pair runs as two launches when a third record reads the hidden tensor, when the projection's output lies over the GEGLU GEMM's
      operand (the launch would store over rows it has yet to read), when the projection is split-K, when M is below the cut-off (no
      waiver), and — in a child process — for any pair under T2V_FF_FUSE=0.
Measured figures: profiles/ff_fused.txt."""
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":      # the child process of the last test: the paths tests/conftest.py sets up
    sys.path[:0] = [os.path.abspath(os.path.join(os.path.dirname(__file__), "..")), os.path.dirname(os.path.abspath(__file__))]

import ff_fused_inputs as FF
import gemm_inputs as G
from interp import Interp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import BoundProgram

pytestmark = pytest.mark.gpu


def run_plan(b, ops):
    """Run the records `ops` of b's program on the GPU from the case's initial arena -> (arena view on the CPU, per-record ms)."""
    it = Interp(b.P, b.w, poison=False)
    b.init(it)
    dev = torch.device("cuda:0")
    arena = it.arena.to(dev)
    w = {k: v.to(dev).contiguous() for k, v in b.w.items()}
    bp = BoundProgram(b.P, arena.data_ptr(), {k: v.data_ptr() for k, v in w.items()}, ops=ops)
    ms = bp.run_timed({}, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    L.async_status()
    it.arena = arena.cpu()
    return it, ms


def stored(it, b):
    return it.mat(b.full.ref, b.full.rows, b.full.cols, b.full.ld, torch.float16, {}).clone()


@pytest.mark.parametrize("c", FF.CASES, ids=lambda c: c["id"])
def test_fused_pair_is_bit_identical_to_two_launches_and_within_the_fp16_bound(c):
    _, _, ref = FF.inputs_of(c)
    b = FF.build(c)
    fused, ms_f = run_plan(b, b.ops("adjacent"))
    plain, ms_p = run_plan(b, b.ops("separated"))
    assert ms_f[1] == 0.0, f"the adjacent pair did not fuse (projection {ms_f[1]} ms)"
    assert ms_f[0] > 0.0 and ms_p[2] > 0.0, "the separated pair must run the projection as its own launch"
    FF.check_fences(fused, b, hidden_written=False)                                   # (c)
    FF.check_fences(plain, b, hidden_written=True)
    got_f, got_p = stored(fused, b), stored(plain, b)
    e_f, e_p = G.seg_err(got_f[:, :FF.C], ref), G.seg_err(got_p[:, :FF.C], ref)
    nbits = int((got_f.view(torch.int16) != got_p.view(torch.int16)).sum())
    print(f"FFFUSED {c['id']}: worst segment fused {float(e_f.max()):.3e}, two launches {float(e_p.max()):.3e} (bound {FF.TOL_F16:.0e}); "
          f"{nbits} of {got_f.numel()} stored values differ; fused {1e3 * ms_f[0]:.1f} us, two launches {1e3 * (ms_p[0] + ms_p[2]):.1f} us")
    assert nbits == 0, f"{nbits} stored values differ between the fused and the two-launch form"      # (a)
    assert float(e_f.max()) <= FF.TOL_F16 and float(e_p.max()) <= FF.TOL_F16                    # (b)


def test_pair_whose_hidden_tensor_has_a_third_reader_runs_unfused():
    b = FF.build(FF.CASES[0])
    it, ms = run_plan(b, b.ops("third-reader"))
    assert ms[1] > 0.0
    FF.check_fences(it, b, hidden_written=True)


def test_pair_whose_output_lies_over_its_own_operand_runs_unfused_and_is_right():
    """The lowerings give the projection the dead X buffer as its [M, 640] hi + lo output: as one launch a workgroup would store over X
    rows that another workgroup has yet to read (three tiles here)."""
    c = FF.CASES[4]
    b = FF.build(c, out_over_x=True)
    it, ms = run_plan(b, b.ops("adjacent"))
    assert ms[1] > 0.0
    FF.check_fences(it, b, hidden_written=True)
    e = G.seg_err(stored(it, b)[:, :FF.C], FF.inputs_of(c)[2])
    assert float(e.max()) <= FF.TOL_F16, float(e.max())


def test_pair_with_a_split_k_projection_runs_unfused():
    c = FF.CASES[1]
    b = FF.build(c, split_k=True)
    it, ms = run_plan(b, b.ops("adjacent"))
    assert ms[1] > 0.0
    FF.check_fences(it, b, hidden_written=True)
    assert float(G.seg_err(stored(it, b)[:, :FF.C], FF.inputs_of(c)[2]).max()) <= FF.TOL_F16


def test_pair_below_the_row_cutoff_runs_unfused():
    c = FF.CASES[4]
    b = FF.build(c, waive_cutoff=False)
    it, ms = run_plan(b, b.ops("adjacent"))
    assert ms[1] > 0.0
    FF.check_fences(it, b, hidden_written=True)


def test_switch_turns_the_fusion_off_in_a_child_process():
    env = dict(os.environ, T2V_FF_FUSE="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FFFUSED-CHILD projection ms > 0: True" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__":
    # the child of test_switch_turns_the_fusion_off_in_a_child_process: the adjacent pair, cut-off waived, under the caller's environment
    b = FF.build(FF.CASES[0])
    it, ms = run_plan(b, b.ops("adjacent"))
    FF.check_fences(it, b, hidden_written=ms[1] > 0.0)
    print(f"FFFUSED-CHILD projection ms > 0: {ms[1] > 0.0}")
