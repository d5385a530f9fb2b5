"""GPU (-m gpu): the footprint table (tests/plan_footprint.py) against the kernels, and the two plans of a program against recycled memory.

Per row — tiny ModelScope defaults, tiny LVDM defaults, tiny LVDM with T2V_GN_EPI=0, tiny VAE decode, tiny VAE encoder:
  (a) every op as a single-op plan under the confinement protocol (plan_hazards.Confinement): from the state of a clean chain, once with
      its pure outputs zero-filled and once with EVERY arena byte outside its declared read rectangles at 0xFF; the written rectangles
      must be bit-equal, and outside the written / scratch rectangles the poisoned arena must be untouched;
  (b) the whole program from a 0x00 arena and from a 0xFF arena: every ext output bit-equal; then the plan without the step-invariant
      ops, after 0xFF has been written over every byte that pass 2 does not need by plan_hazards' account: bit-equal again.
The synchronisation words and the exchange-record region are never poisoned: they are zero at bind time (the library's contract) and,
in (a), a copy of what the clean chain left.  Collective ops and T-sharded rows are checked statically only
(tests/test_plan_hazards_cpu.py).  Measured figures: profiles/plan_hazards.txt."""
import os
import time

import pytest
import torch

import plan_footprint as FP
import plan_hazards as H
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import BoundProgram, Program
from tools import program_digest as PD

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ROWS = ["tiny modelscope defaults", "tiny lvdm defaults", "tiny lvdm T2V_GN_EPI=0", "vae decode tiny n=2 8x8", "vae encoder tiny n=3 64x48"]


@pytest.fixture(scope="module")
def lowered(built_lib):
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for k in [k for k in os.environ if k.startswith("T2V_") and k not in PD.FIXED and k != "T2V_LIB_PATH"]:
            mp.delenv(k)
        for k, v in PD.FIXED.items():
            if k != "T2V_DEVICE_CUS":                    # the lowering plans for the device it will run on
                mp.setenv(k, v)
        rec = H.Recorder().install(mp)
        for r in PD.rows(ROOT):
            if r.label in ROWS:
                with PD.applied(r):
                    comp = r.thunk()
                out[r.label] = (comp, rec.events(comp.prog), r.net)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("label", ROWS)
def test_kernels_stay_inside_the_footprints(lowered, label):
    comp, events, net = lowered[label]
    prog, dev = comp.prog, torch.device("cuda:0")
    assert not any(op.kind in (L.OP_ALLGATHER, L.OP_HALO_EXCHANGE, L.OP_ALLTOALL, L.OP_STATS_HALO) for op in prog.ops)
    rep = H.analyse(prog, events)
    assert rep.hazards == []
    stream = torch.cuda.current_stream(dev).cuda_stream
    packed = comp.packer.materialise(net.state_dict(), dev)
    wptr = {k: v.data_ptr() for k, v in packed.items()}
    ext = H.ext_tensors(prog, dev)
    wext = sorted({int(x.name) for op in prog.ops for x in FP.footprint(op) if x.space == "ext" and x.mode != "r"})
    n, guard = prog.arena.high + 256, H.guarded_prefix(prog)
    ptrs = lambda e: {s: t.data_ptr() for s, t in e.items()}

    # ---- (a) op by op
    t0 = time.perf_counter()
    A = torch.zeros(n, dtype=torch.uint8, device=dev)
    plans = {}

    def run(k, arena, e):
        key = (k, arena.data_ptr())
        if key not in plans:
            plans[key] = BoundProgram(prog, arena.data_ptr(), wptr, ops=[prog.ops[k]])
        plans[key].run(ptrs(e), stream)

    conf = H.Confinement(prog, A, run)
    for k, op in enumerate(prog.ops):
        conf.step(k, op, ext)
    torch.cuda.synchronize()
    L.async_status()
    t_ops = time.perf_counter() - t0
    assert conf.checked == len(prog.ops)
    assert not conf.errors, "\n".join(conf.errors[:30])
    chain = {s: ext[s].clone() for s in wext}
    plans.clear()

    # ---- (b) the whole program from 0x00 and from 0xFF, then the plan without the step-invariant ops over recycled memory
    t0 = time.perf_counter()
    results, arena0, bound0 = [], None, None
    for fill in (0x00, 0xFF):
        arena = torch.full((n,), fill, dtype=torch.uint8, device=dev)
        arena[:guard] = 0
        for s in wext:
            ext[s].view(torch.uint8).fill_(0x7F) if ext[s].dtype != torch.uint8 else ext[s].fill_(0x7F)
        bound = BoundProgram(prog, arena.data_ptr(), wptr, stream=stream)
        bound.run(ptrs(ext), stream)
        torch.cuda.synchronize()
        results.append({s: ext[s].clone() for s in wext})
        if fill == 0x00:
            arena0, bound0 = arena, bound
    for s in wext:
        assert torch.equal(results[0][s], results[1][s]), f"ext slot {s}: the program's result depends on what the arena held before"
        assert torch.equal(results[0][s], chain[s]), f"ext slot {s}: the whole program and the op-by-op chain differ"
    keep = torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)
    keep[:guard] = arena0[:guard]
    carried = rep.carried if rep.carried is not None else ([], [])
    for a, b in zip(list(carried[0]), list(carried[1])):
        keep[int(a):int(b)] = arena0[int(a):int(b)]
    arena0.copy_(keep)
    for s in wext:
        ext[s].view(torch.uint8).fill_(0x7F) if ext[s].dtype != torch.uint8 else ext[s].fill_(0x7F)
    bound0.run(ptrs(ext), stream, skip_invariant=True)
    torch.cuda.synchronize()
    L.async_status()
    for s in wext:
        assert torch.equal(ext[s], results[0][s]), f"ext slot {s}: the plan without the step-invariant ops needs bytes the analysis calls dead"
    kept = int(sum(int(b) - int(a) for a, b in zip(list(carried[0]), list(carried[1]))))
    print(f"\n{label}: {len(prog.ops)} ops, arena {n / 1e6:.1f} MB, op-by-op protocol {t_ops:.2f} s, whole-program runs {time.perf_counter() - t0:.2f} s, "
          f"{kept} step-invariant bytes carried into pass 2")
