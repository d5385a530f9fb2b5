"""CPU: every code path of every program a user can request has an adversarial case.

The requestable programs are the lattice of tests/geometry_lattice.py; tools/geometry_paths.py lowered all of them, wrote what it found to
profiles/geometry_paths.txt and a greedy cover of the keys the matrix of tests/test_record_paths_cpu.py lacks to tests/geometry_witnesses.py.
Lowering the whole lattice takes minutes, so this file checks
(1) the witnesses are live: every one lowers, and the keys profiles/geometry_paths.txt says it stands for are in its program (a policy change
    that moves keys makes the table stale: run the tool again);
(2) the witnesses are covered: every key of every witness program has an adversarial case;
(3) held-out closure: every key of a seeded sample of HELD_OUT lattice programs that are NOT witnesses has a case — no program is skipped,
    and one that does not lower fails the test;
(4) the check bites: without the only case of a witness key, that key is reported with its geometry and an op.
The adversarial side and the failure lines are those of tests/test_record_paths_cpu.py."""
import collections
import os
import time

import pytest

import geometry_lattice as GL
import geometry_witnesses as GW
import record_paths as RP
from test_plan_hazards_cpu import ROOT, _fixed_environment, _lower
from test_record_paths_cpu import adversarial_side, missing_of

SEED, HELD_OUT = 20251, 200
PROFILE = os.path.join(ROOT, "profiles", "geometry_paths.txt")


def _label(k):
    return f"{RP.kind_of(k)} [{RP.show(k)}]"


@pytest.fixture(scope="module")
def world():
    """(witness entry -> key -> [(label, op name)], held-out entry -> the same, adversarial: key -> [case id])."""
    mp = pytest.MonkeyPatch()
    t0 = time.time()
    try:
        _fixed_environment(mp)
        nets = GL.make_nets()

        def keys_of(e):
            low = collections.OrderedDict()
            for op in _lower(GL.row_of(e, nets)).prog.ops:          # (a program that does not lower raises here: the test fails)
                for k in RP.path_keys(op):
                    low.setdefault(k, []).append((e.label, op.name))
            return low

        witnesses = [GL.Entry(*w) for w in GW.WITNESSES]
        wit = collections.OrderedDict((e, keys_of(e)) for e in witnesses)
        held = collections.OrderedDict((e, keys_of(e)) for e in GL.held_out(witnesses, HELD_OUT, SEED))
        adv, _ = adversarial_side()
    finally:
        mp.undo()
    print(f"GEOMETRY-PATHS {len(wit)} witnesses + {len(held)} held-out programs lowered, adversarial side built: {time.time() - t0:.0f} s")
    return wit, held, adv


def _merged(programs):
    low = collections.OrderedDict()
    for per in programs.values():
        for k, where in per.items():
            low.setdefault(k, []).extend(where)
    return low


def test_witnesses_are_live(world):
    wit, _, _ = world
    assert len(set(wit)) == len(GW.WITNESSES) and set(wit) <= set(GL.entries()), "a witness is not a program of the lattice"
    by_label = {e.label: e for e in wit}
    stale, n = [], 0
    for ln in open(PROFILE).read().splitlines():
        if ln.startswith("witness: "):
            key, _case, _small, _op, stands = ln[len("witness: "):].split(" | ")
            n += 1
            if stands not in by_label:
                stale.append(f"{key}: '{stands}' is not in tests/geometry_witnesses.py")
            elif key not in {_label(k) for k in wit[by_label[stands]]}:
                stale.append(f"{key}: no longer in the program of '{stands}'")
    assert n >= len(wit), "profiles/geometry_paths.txt names fewer keys than there are witnesses"
    assert not stale, f"{len(stale)} stale witness lines (run tools/geometry_paths.py):\n" + "\n".join(stale)


def test_witnesses_are_covered(world):
    wit, _, adv = world
    miss = missing_of(_merged(wit), adv)
    assert not miss, f"{len(miss)} code paths of the witness programs without an adversarial case:\n" + "\n".join(miss)


def test_held_out_programs_are_covered(world):
    wit, held, adv = world
    assert len(held) == HELD_OUT and not set(held) & set(wit)
    miss = missing_of(_merged(held), adv)
    assert not miss, (f"{len(miss)} code paths of held-out lattice programs without an adversarial case (the enumeration of "
                      "tools/geometry_paths.py missed them):\n" + "\n".join(miss))


def test_the_check_bites(world):
    """Without the only case that covers some witness key, that key is reported — with its geometry and its op."""
    wit, _, adv = world
    low = _merged(wit)
    sole = [(k, adv[k][0]) for k in low if k in adv and len(set(adv[k])) == 1]
    assert sole, "no witness key with a single cover"
    for k, cid in (sole[0], sole[len(sole) // 2], sole[-1]):
        pruned = {kk: [c for c in cids if c != cid] for kk, cids in adv.items()}
        pruned = {kk: v for kk, v in pruned.items() if v}
        miss = missing_of(low, pruned)
        want = f"row '{low[k][0][0]}', op '{low[k][0][1]}'"
        assert any(RP.show(k) in m and want in m for m in miss), (cid, RP.show(k))
