"""TEST INFRASTRUCTURE — one rank of tests/test_gpu_collectives_adversarial.py (2, 3 or 4 processes on ONE GPU, RCCL = tests/fake_rccl).

Builds two library communicators over the gloo group — one with a peer window of 256 KiB slots (T2V_PEER_WINDOW=1, T2V_PEER_SLOT_MB=0.25),
one without (T2V_PEER_WINDOW=0) — and runs every case of tests/collective_inputs.py of this world on both: the rank's records over its own
byte arena as one plan (kind DIRECT: one t2v_comm_all_gather call), one synchronize, then the whole arena against `expected` byte for
byte and t2v_comm_counters against the transports `shares` predicts.  One RESULT line per case and communicator, one SUMMARY line.
A case that ends in an error (T2V_ERR_ASYNC after T2V_PEER_TIMEOUT_MS included) is reported and ends the rank's run: nothing more is
launched after it."""
import ctypes
import datetime
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
import collective_inputs as C                                        # noqa: E402
from sd_webui_text2video_amd import _lib as L, parallel            # noqa: E402

lib = L.load()
t_start = time.time()
comms = {}
for window in (1, 0):
    os.environ["T2V_PEER_WINDOW"], os.environ["T2V_PEER_SLOT_MB"] = str(window), "0.25"
    comms[window] = parallel.Communicator(dist.group.WORLD, list(range(world)), rank, dev)
assert comms[1].window and comms[0].window is None, (comms[1].window, comms[0].window)
t_comm = time.time()
vp = ctypes.c_void_p
stream = vp(torch.cuda.current_stream(dev).cuda_stream)
totals = {1: [0, 0], 0: [0, 0]}
stopped = None
for case in (c for c in C.CASES if c["world"] == world):
    want = C.expected(case, rank)
    for window in (1, 0):
        comm = comms[window]
        arena = torch.from_numpy(C.initial(case, rank)).to(dev)
        b = C.build(case, rank, alloc=lambda n: arena.data_ptr())
        assert arena.numel() == b.plan.size and b.base % 256 == 0
        before = comm.counters()
        res = {"rank": rank, "case": case["id"], "window": window, "ok": False}
        t0 = time.time()
        try:
            if b.direct is not None:
                L.check(lib.t2v_comm_all_gather(comm.handle, vp(b.base + b.direct[0]), b.direct[1], stream))
            else:
                plan = vp()
                L.check(lib.t2v_plan_create(b.records, len(b.records), ctypes.byref(plan)))
                try:
                    L.check(lib.t2v_plan_set_comm(plan, comm.handle))
                    L.check(lib.t2v_plan_run(plan, None, 0, stream))
                finally:
                    torch.cuda.synchronize()
                    lib.t2v_plan_destroy(plan)
            torch.cuda.synchronize()
            L.async_status()
        except Exception as e:       # reported; this rank launches nothing more
            res["error"] = f"{type(e).__name__}: {e}"[:400]
            stopped = case["id"]
        else:
            got = arena.cpu().numpy()
            after = comm.counters()
            res["ms"] = round((time.time() - t0) * 1e3, 2)
            res["diff"] = C.first_difference(case, rank, got, want)
            res["counters"] = [after[0] - before[0], after[1] - before[1]]
            res["predicted"] = list(C.predicted_counters(case, rank, window=bool(window)))
            res["ok"] = res["diff"] is None and res["counters"] == res["predicted"]
            totals[window][0] += res["counters"][0]
            totals[window][1] += res["counters"][1]
        print("RESULT " + json.dumps(res), flush=True)
        if stopped:
            break
    if stopped:
        break
status = None
if not stopped:
    try:
        torch.cuda.synchronize()
        L.async_status()
        status = "clean"
    except Exception as e:
        status = f"{type(e).__name__}: {e}"[:400]
print("SUMMARY " + json.dumps({"rank": rank, "world": world, "stopped_at": stopped, "async_status": status, "setup_s": round(t_comm - t_start, 2),
                               "cases_s": round(time.time() - t_comm, 2), "window_comm": totals[1], "rccl_comm": totals[0],
                               "window": comms[1].window}), flush=True)
dist.barrier()          # nobody releases its window (or the stand-in's shared memory) while a peer may still be in an exchange
dist.destroy_process_group()
