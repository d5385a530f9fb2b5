"""GPU (-m gpu), ONE device: the four collective ops and t2v_comm_all_gather on the designed inputs of tests/collective_inputs.py.

2, 3 and 4 processes share cuda:0 (RCCL entry points: tests/fake_rccl, as in tests/test_gpu_fake_rccl.py).  Every process drives the library
with bare records over its own byte arena (tests/collective_worker.py) on two communicators — a peer window of 256 KiB slots, and none — and
compares every byte, fences and untouched gaps included, with collective_inputs.expected; t2v_comm_counters must advance by exactly the
transports collective_inputs.shares predicts (so eligibility came out the same on every rank), and t2v_async_status must be clean.
What the cases reach in csrc/comm.hip, and which wrong implementation each would catch, is proved on the CPU
(tests/test_collective_inputs_cpu.py).  All ranks sit on one device: this pins which bytes go where and through which transport, and
says nothing about behaviour across GPUs.

The misaligned base (DIRECT cases `off8`): t2v_comm_all_gather serves any base (include/t2v_hip.h) — a gather the window carries from a base
off 16 bytes runs on an aligned copy — so both communicators must produce the same bytes; before that the window communicator answered
T2V_ERR_BAD_ARG where the RCCL communicator succeeded."""
import json
import os
import subprocess
import sys
import time

import pytest

import collective_inputs as C
from test_gpu_fake_rccl import HERE, _free_port, fake_rccl      # noqa: F401  (fake_rccl: the fixture that builds the stand-in)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3, 4])
def test_collectives_on_designed_sizes(fake_rccl, world):      # noqa: F811
    port = _free_port()
    procs = []
    t0 = time.time()
    for r in range(world):
        env = {**os.environ, "RANK": str(r), "WORLD_SIZE": str(world), "LOCAL_RANK": str(r), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
               "T2V_RCCL_SONAME": fake_rccl, "T2V_PEER_TIMEOUT_MS": "5000"}
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "collective_worker.py")], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=240)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    wall = time.time() - t0
    cases = [c for c in C.CASES if c["world"] == world]
    summaries, failures = [], []
    for r, (p, out) in enumerate(zip(procs, outs)):
        lines = out.splitlines()
        results = [json.loads(ln[7:]) for ln in lines if ln.startswith("RESULT ")]
        failures += [f"rank {r} {x['case']} window={x['window']}: " + (x.get("error") or x.get("diff") or f"counters {x['counters']} != predicted {x['predicted']}")
                     for x in results if not x["ok"]]
        assert p.returncode == 0 and not failures, f"rank {r} (exit {p.returncode}):\n" + "\n".join(failures[:12]) + f"\n{out[-2000:]}"
        assert [(x["case"], x["window"]) for x in results] == [(c["id"], w) for c in cases for w in (1, 0)]
        summaries.append(json.loads(next(ln for ln in lines if ln.startswith("SUMMARY "))[8:]))
    s0 = summaries[0]
    print(f"collectives on designed sizes, {world} processes on one GPU: {len(cases)} cases x 2 communicators in {wall:.1f} s wall "
          f"(communicators {s0['setup_s']} s, cases {s0['cases_s']} s); exchanges (window, rccl) on the window communicator {s0['window_comm']}, "
          f"on the other {s0['rccl_comm']}; {s0['window']}")
    for r, s in enumerate(summaries):
        assert s["stopped_at"] is None and s["async_status"] == "clean", s
        want_w = [sum(v) for v in zip(*(C.predicted_counters(c, r, True) for c in cases))]
        want_r = [sum(v) for v in zip(*(C.predicted_counters(c, r, False) for c in cases))]
        assert s["window_comm"] == want_w and s["rccl_comm"] == want_r and want_r[0] == 0 and want_w[0] > 0 and want_w[1] > 0
