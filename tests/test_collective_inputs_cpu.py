"""CPU: what the designed collective inputs (tests/collective_inputs.py) expose, before a GPU runs them.

(1) two more writings of the contract agree with `expected`: harness.run_lockstep on CPU byte arenas (stand-in executors that carry `arena`
    and `steps`; the composite's pack / unpack through tests/interp.py) and the executed mirror of csrc/comm.hip (`simulate`);
(2) coverage: every share / trip / transport class has a case in every op kind that can reach it (collective_inputs.CANNOT names the kinds
    that cannot, and why); the classes of the slot logic — chosen in px_exchange from the pair's sequence number alone, whatever the op —
    are asked of the suite as a whole;
(3) the inputs bite: every wrong implementation of collective_inputs.VARIANTS is told apart from `expected` by a case, which is printed;
(4) the assertion bites: without the only case of a class, the coverage check names that class.
The printed report is committed as profiles/collectives_adversarial.txt."""
import numpy as np
import pytest
import torch

import collective_inputs as C
from harness import run_lockstep
from interp import Interp
from sd_webui_text2video_amd.program import COLLECTIVE_KINDS


class _Segment:
    """The compute ops between two collectives of the composite: RESHARD_ROWS through the CPU interpreter, on the executor's arena."""

    def __init__(self, ex, op):
        self.ex, self.op = ex, op

    def run(self, ext, stream):
        it = Interp.__new__(Interp)
        it.arena, it.weights = self.ex.arena, {}
        it.run(ext, ops=[self.op])


class _Executor:
    def __init__(self, built):
        self.arena = torch.from_numpy(built.arena.copy())
        self.steps = [("coll", op) if op.kind in COLLECTIVE_KINDS else ("seg", _Segment(self, op)) for op in built.ops]


@pytest.mark.parametrize("world", [2, 3, 4])
def test_expected_equals_lockstep_and_the_executed_mirror(world):
    for case in (c for c in C.CASES if c["world"] == world):
        exs = [_Executor(C.build(case, r)) for r in range(world)]
        run_lockstep(exs, [{} for _ in range(world)], None)
        sim = C.simulate(case)
        off = C.simulate(case, window=False)
        for r in range(world):
            want = C.expected(case, r)
            for name, got in (("run_lockstep", exs[r].arena.numpy()), ("simulate", sim[r]), ("simulate, no window", off[r])):
                assert C.first_difference(case, r, got, want) is None, f"{name}: {C.first_difference(case, r, got, want)}"


def test_tags_poison_and_fences():
    for case in C.CASES:
        for r in range(case["world"]):
            pl, a, e = C.plan(case, r), C.initial(case, r), C.expected(case, r)
            keep = np.ones(a.size, dtype=bool)
            for b in pl.bufs.values():
                keep[b["off"]: b["off"] + b["size"]] = False
                assert b["off"] >= C.FENCE and b["off"] + b["size"] + C.FENCE <= a.size
                for off, n in b["tagged"]:                       # no tagged unit can pass for poison
                    units = a[b["off"] + (off + 15 & ~15): b["off"] + (off + n & ~15)].reshape(-1, 16)
                    assert not (units == C.POISON).all(axis=1).any()
            assert (a[keep] == C.POISON).all() and (e[keep] == C.POISON).all()      # fences and gaps: poison before and after


def test_composite_is_the_clip():
    """The pixel-sharded intermediate is the clip's pixel split; the end result is input + residual (numpy on the global clip)."""
    for case in (c for c in C.CASES if c["kind"] == "COMPOSITE"):
        world, hw, c = case["world"], case["hw"], case["c"]
        n, y, x = C._clip(case)
        cnt = C.counts(case["frames"], world)
        outs, xps = [], []
        sim = C.simulate(case)
        for r in range(world):
            b = C.plan(case, r).bufs
            xps.append(sim[r][b["xp"]["off"]: b["xp"]["off"] + b["xp"]["size"]].view(np.float16).reshape(case["frames"], hw // world, c))
            outs.append(sim[r][b["out"]["off"]: b["out"]["off"] + b["out"]["size"]].view(np.float32).reshape(cnt[r], hw, c))
            assert np.array_equal(xps[r].view(np.uint16), C.pixel_split(case, r).view(np.uint16))
            # the receive slot of the short last slice is base_cnt chunks wide: xp has no gap (frames are consecutive), `back` of the
            # last rank is cnt(me) wide per peer — the all-to-all cases below carry the gap
        assert np.array_equal(np.concatenate(xps, axis=1).view(np.uint16), n.view(np.uint16))
        assert np.array_equal(np.concatenate(outs, axis=0), y + x)


def test_short_last_slice_keeps_its_gap():
    """Direction 0: the slot of the last slice is base_cnt * chunk wide, only last_cnt * chunk of it is written."""
    case = C.BY_ID["a2a-7f-4112-d0-w3"]
    for r in (0, 1):
        b = C.plan(case, r).bufs["s0.b1"]
        e = C.expected(case, r)[b["off"]: b["off"] + b["size"]]
        slot = e[2 * 3 * 4112: 3 * 3 * 4112]
        assert (slot[4112:] == C.POISON).all() and C.decode_unit(slot[:16]) == (case["serial"], 2, 0, r * 4112 // 16)


def test_shares_are_what_the_sizes_were_chosen_for():
    def one(cid, rank=0, peer=0):
        if cid not in C.BY_ID:          # a gather size runs at one world: whichever
            cid = next(c["id"] for c in C.CASES if c["id"].startswith(cid.rsplit("-", 1)[0] + "-w"))
        return C.shares(C.BY_ID[cid], rank)[0]["peers"][peer]

    p = one("gather-8208-w3")
    assert p["nb_recv"] == 2 and p["recv"][0] == [(0, 256), (256, 513)]
    assert one("gather-8176-w2")["nb_send"] == 1 and one("gather-8192-w2")["nb_send"] == 2
    assert one("gather-32752-w2")["nb_send"] == 7 and one("gather-32768-w3")["nb_send"] == 8
    p = one("gather-28688-w4")
    assert p["nb_recv"] == 7 and len({u1 - u0 for u0, u1 in p["recv"][0]}) == 2
    p = one("gather-131072-w4")
    assert p["trips"] == 1 and {u1 - u0 for u0, u1 in p["recv"][0]} == {1024}
    p = one("gather-131200-w2")
    assert p["trips"] == 2 and p["last_live"] == [1] and {u1 - u0 for u0, u1 in p["recv"][0]} == {1025}
    p = one("gather-200016-w4")
    assert {u1 - u0 for u0, u1 in p["recv"][0]} == {1562, 1563} and p["last_live"] == [3]
    assert [C.shares(C.BY_ID[c], 0)[0]["transport"] for c in ("gather-262144-w4", "gather-262160-w2", "gather-6002-w3")] == \
        ["window", "rccl:size", "rccl:unit"]
    p = one("stats-512+7680-F2-w2")
    assert p["nb_send"] == 2 and p["send"] == [[(0, 16), (16, 32)], [(0, 240), (240, 480)]]
    p = one("stats-16+131200-F2-w2")
    assert p["nb_recv"] == 8 and sum(u0 == u1 for u0, u1 in p["recv"][0]) == 7 and p["trips"] == 2
    s = C.shares(C.BY_ID["stats-512+7680-F1-w3"], 0)[0]                 # rank 0: rank 1 is a neighbour (two segments), rank 2 gets the part alone
    assert [(p["q"], p["nb_send"], p["sbytes"]) for p in s["peers"]] == [(1, 2, [512, 7680]), (2, 1, [512, 0])] and s["nbmax"] == 2
    p = one("a2a-7f-4112-d0-w3", rank=0, peer=1)                        # rank 0 (3 frames) and rank 2 (1 frame)
    assert (p["q"], p["nb_send"], p["nb_recv"]) == (2, 3, 1)
    p = one("a2a-7f-10928-d1-w3", rank=0, peer=1)
    assert (p["nb_send"], p["nb_recv"]) == (2, 8)
    p = one("a2a-5f-43744-d0-w2")
    assert p["sbytes"][0] == 131232 and p["trips"] == 1 and one("a2a-5f-43744-d0-w2", rank=1)["trips"] == 2
    for world in (2, 3, 4):
        case = C.BY_ID[f"sequence-w{world}"]
        assert C.predicted_counters(case, 0) == (14, 2) and C.predicted_counters(case, 0, window=False) == (0, 16)
        for r in range(world):          # every pair passes both slots, on every rank
            par = {}
            for s in C.shares(case, r):
                for p in s["peers"]:
                    if "parity" in p:
                        par.setdefault(p["q"], set()).add(p["parity"])
            assert set(par) == set(range(world)) - {r} and all(v == {0, 1} for v in par.values())
        if world > 2:       # halo exchanges touch neighbours only: rank 0's pair with rank 1 runs ahead of its pair with rank 2
            last = {p["q"]: p["seq"] for s in C.shares(case, 0) for p in s["peers"] if "seq" in p}
            assert last[1] == 14 and last[2] == 12


def _report_coverage(by, suite):
    print("\nclasses x cases (op kind: class: cases that reach it)")
    for k in C.KINDS:
        for cl in C.CLASSES:
            ids = by.get((k, cl), [])
            why = C.CANNOT.get((k, cl))
            print(f"  {k:14s} {cl:26s} " + (f"cannot: {why}" if why and not ids else f"{len(ids):3d}  {', '.join(ids[:3])}{' ...' if len(ids) > 3 else ''}"))
    for cl in C.SUITE_CLASSES:
        ids = suite.get(cl, [])
        print(f"  {'suite':14s} {cl:34s} {len(ids):3d}  {', '.join(ids[:3])}{' ...' if len(ids) > 3 else ''}")


def test_every_class_has_a_case_in_every_kind_that_can_reach_it():
    by, suite, missing = C.coverage()
    _report_coverage(by, suite)
    assert not missing, f"classes without a case: {missing}"
    for key, why in C.CANNOT.items():
        assert why and not by.get(key), f"{key} is listed as unreachable ({why}) but {by.get(key)} reach it"


def test_the_coverage_assertion_bites():
    by, _, _ = C.coverage()
    single = [(key, ids[0]) for key, ids in by.items() if len(ids) == 1 and key[1] in C.CLASSES and key not in C.CANNOT]
    assert single, "no class hangs on a single case: nothing to take away"
    for (kind, cl), cid in single[:4]:
        _, _, missing = C.coverage([c for c in C.CASES if c["id"] != cid])
        assert f"{kind}: {cl}" in missing, f"without {cid} the check should name {kind}: {cl}; it names {missing}"
    _, _, missing = C.coverage([c for c in C.CASES if c["kind"] != "SEQUENCE"])
    assert "suite: shrink after grow in one slot" in missing and "suite: window op after an RCCL op" in missing


def test_every_wrong_implementation_is_caught():
    want = {(c["id"], r): C.expected(c, r) for c in C.CASES for r in range(c["world"])}
    print("\nwrong implementation: the cases that tell it apart from `expected` (first three; where rank 0..n first differs)")
    uncaught = []
    for v, text in C.VARIANTS.items():
        caught = []
        for c in C.CASES:
            got = C.simulate(c, variant=v)
            diff = [C.first_difference(c, r, got[r], want[(c["id"], r)]) for r in range(c["world"])]
            if any(diff):
                caught.append((c["id"], next(d for d in diff if d)))
            if len(caught) == 3:
                break
        print(f"  {v}: {text}")
        for cid, d in caught:
            print(f"      {cid}: {d.split(': ', 1)[1]}")
        if not caught:
            uncaught.append(v)
    assert not uncaught, f"no case tells these apart from the contract: {uncaught}"
