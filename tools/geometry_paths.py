"""Every code path of every program a user can request: lowers the whole lattice of tests/geometry_lattice.py on the CPU (records only,
under program_digest.FIXED), keys every record (tests/record_paths.py) and compares the keys with the matrix of tests/test_record_paths_cpu.py
(tools/program_digest.py rows + extra_rows) and with the adversarial case lists.
Writes profiles/geometry_paths.txt — programs lowered, keys per kind, keys per kind the matrix lacks, the ones without an adversarial case,
a witness per key the matrix lacks (the smallest program of the lattice by F x H x W that has it, an op of it, and the program of the
greedy cover that stands for it), the growth of the count over a seeded shuffle, the wall time — and tests/geometry_witnesses.py: the
greedy cover as plain data, which tests/test_geometry_paths_cpu.py lowers again.
Usage: python tools/geometry_paths.py [--jobs N] [--limit N] [--no-write]      (--limit: a seeded sample of N programs, for a quick look)
Run it after every change of a selection policy (tile policy, split-K, GroupNorm launch form, attention kernel): such a change moves keys."""
import argparse
import collections
import multiprocessing
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "tests")]
SHUFFLE_SEED = 20250
CURVE = (30, 60, 120, 240, 500, 1000, 2000, 4000, 8000, 16000, 32000)

_NETS = None


def _setup():
    global _NETS
    from tools import program_digest as PD
    PD.fix_environment()
    import torch
    torch.set_num_threads(1)
    from sd_webui_text2video_amd.program import Program
    Program._DEVICE_CUS = None
    import geometry_lattice as GL
    _NETS = GL.make_nets()


def _lower_chunk(chunk):
    """[(entry index, entry)] -> (the chunk's keys, [(entry index, [(key index, op name)])], [(entry index, error)])."""
    import geometry_lattice as GL
    import record_paths as RP
    from tools import program_digest as PD
    if _NETS is None:
        _setup()
    keys, out, failed = {}, [], []
    for idx, e in chunk:
        try:
            r = GL.row_of(e, _NETS)
            with PD.applied(r):
                prog = r.thunk().prog
            seen = {}
            for op in prog.ops:
                for k in RP.path_keys(op):
                    seen.setdefault(keys.setdefault(k, len(keys)), op.name)
            out.append((idx, sorted(seen.items())))
        except Exception as ex:          # a geometry that does not lower is a finding: reported, never hidden
            failed.append((idx, f"{type(ex).__name__}: {ex}"))
    return list(keys), out, failed


def sweep(entries, jobs):
    """-> (key -> [(entry index, op name)] in entry order, [(entry index, error)])."""
    chunks = [list(enumerate(entries))[k:k + 64] for k in range(0, len(entries), 64)]
    per_entry, failed = {}, []
    if jobs > 1:
        with multiprocessing.get_context("fork").Pool(jobs, initializer=_setup) as pool:
            results = pool.imap_unordered(_lower_chunk, chunks)
            results = list(results)
    else:
        results = [_lower_chunk(c) for c in chunks]
    for keys, out, bad in results:
        failed += bad
        for idx, pairs in out:
            per_entry[idx] = [(keys[ki], name) for ki, name in pairs]
    return per_entry, sorted(failed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--limit", type=int, default=0)
    ap.add_argument("--no-write", action="store_true")
    args = ap.parse_args()
    t0 = time.time()
    _setup()
    import geometry_lattice as GL
    import record_paths as RP
    import test_record_paths_cpu as T
    from test_plan_hazards_cpu import ROOT, _lower, extra_rows
    from tools import program_digest as PD

    entries = GL.entries()
    if args.limit:
        entries = random.Random(SHUFFLE_SEED).sample(entries, args.limit)
    matrix = set()
    for source in (PD.rows(ROOT), extra_rows()):
        for r in source:
            for op in _lower(r).prog.ops:
                matrix.update(RP.path_keys(op))
    adv, _ = T.adversarial_side()
    t_sides = time.time() - t0
    t1 = time.time()
    per_entry, failed = sweep(entries, args.jobs)
    t_sweep = time.time() - t1

    where = collections.OrderedDict()          # key -> [entry index]
    opname = {}
    for idx in sorted(per_entry):
        for k, name in per_entry[idx]:
            where.setdefault(k, []).append(idx)
            opname[(k, idx)] = name
    fresh = [k for k in where if k not in matrix]
    kinds = sorted({RP.kind_of(k) for k in where})
    label = lambda k: f"{RP.kind_of(k)} [{RP.show(k)}]"

    # the greedy cover of the keys the matrix lacks: the program with the most keys not yet covered, the smaller one on a tie
    left, cover, stands = set(fresh), [], {}
    has = collections.defaultdict(set)
    for k in fresh:
        for idx in where[k]:
            has[idx].add(k)
    while left:
        best = max(has, key=lambda i: (len(has[i] & left), -entries[i].size, -i))
        got = has[best] & left
        cover.append(best)
        for k in got:
            stands[k] = best
        left -= got
        has = {i: s for i, s in has.items() if s & left}

    order = list(range(len(entries)))
    random.Random(SHUFFLE_SEED).shuffle(order)
    seen, curve = set(), []
    for n, idx in enumerate(order, 1):
        seen.update(k for k, _ in per_entry.get(idx, ()) if k not in matrix)
        if n in CURVE or n == len(order):
            curve.append((n, len(seen), sum(k not in adv for k in seen)))

    lines = [f"# tools/geometry_paths.py: the lattice of tests/geometry_lattice.py under program_digest.FIXED, records only",
             f"programs lowered: {len(per_entry)} of {len(entries)} ({len(failed)} failed to lower)",
             f"matrix keys (program_digest rows + extra_rows): {len(matrix)}; adversarial keys: {len(adv)}; lattice keys: {len(where)}",
             "# kind: lattice keys, of them not in the matrix, of them without an adversarial case"]
    for kind in kinds:
        lk = [k for k in where if RP.kind_of(k) == kind]
        lines.append(f"{kind}: {len(lk)} lattice keys, {sum(k not in matrix for k in lk)} not in the matrix, {sum(k not in adv for k in lk)} without a case")
    lines.append(f"total: {len(where)} lattice keys, {len(fresh)} not in the matrix, {sum(k not in adv for k in where)} without a case")
    lines.append("# excluded by a documented limit of the library (rule | the line that refuses it)")
    lines += [f"excluded: {rule} | {why}" for rule, why in GL.EXCLUDED] or ["excluded: none"]
    lines.append("# programs that failed to lower (findings, not exclusions)")
    lines += [f"failed: {entries[i].label} | {err}" for i, err in failed] or ["failed: none"]
    lines.append(f"# growth over a shuffle (seed {SHUFFLE_SEED}): programs, distinct keys the matrix lacks, of them without a case")
    lines += [f"curve: {n} {a} {b}" for n, a, b in curve]
    lines.append(f"# the greedy cover: {len(cover)} witness programs (tests/geometry_witnesses.py) for {len(fresh)} keys")
    lines.append("# witness: key | case | smallest program that has it | an op of it | the cover's program that stands for it")
    for k in fresh:
        small = min(where[k], key=lambda i: (entries[i].size, i))
        lines.append(f"witness: {label(k)} | {adv[k][0] if k in adv else 'NO CASE'} | {entries[small].label} | {opname[(k, small)]} | {entries[stands[k]].label}")
    lines.append(f"wall time: matrix + adversarial side {t_sides:.0f} s, lattice {t_sweep:.0f} s on {args.jobs} processes")
    text = "\n".join(lines) + "\n"
    sys.stdout.write("\n".join(ln for ln in lines if not ln.startswith("witness: ") or "NO CASE" in ln) + "\n")
    if args.no_write or args.limit:
        return
    keep = []
    path = os.path.join(HERE, "profiles", "geometry_paths.txt")
    if os.path.exists(path):          # lines other tools and tests add (measured on the GPU) stay
        keep = [ln for ln in open(path).read().splitlines() if ln.startswith(("gpu: ", "closure test: "))]
    with open(path, "w") as f:
        f.write(text + "".join(ln + "\n" for ln in keep))
    with open(os.path.join(HERE, "tests", "geometry_witnesses.py"), "w") as f:
        f.write('"""TEST DATA, written by tools/geometry_paths.py: the greedy cover of the code paths the lattice of tests/geometry_lattice.py has and the\n'
                'matrix of tests/test_record_paths_cpu.py lacks — (model, form, F, H, W, shard) per program, shard = (total frames, ranks, rank) or\n'
                'None.  profiles/geometry_paths.txt names the keys each one stands for."""\n')
        f.write("WITNESSES = [\n")
        for i in cover:
            f.write(f"    {tuple(entries[i])!r},\n")
        f.write("]\n")


if __name__ == "__main__":
    main()
