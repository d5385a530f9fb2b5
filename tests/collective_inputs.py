"""TEST INFRASTRUCTURE — designed inputs for the four collective ops (ALLGATHER, HALO_EXCHANGE, STATS_HALO, ALLTOALL) and t2v_comm_all_gather.

The forwards of the tiny UNet move a few tens of KB per message, all ranks alike.  Here every rank drives the library with bare records over
one byte arena, at the message sizes where csrc/comm.hip changes what it does: the workgroup count per message (1, 2..7, 8), uneven and
empty shares, a second trip of the receive loop and its partly live last trip, unequal send / receive sizes (all-to-all), the slot-size
boundary between the peer window and RCCL, slot reuse after a larger message, pair sequence numbers that diverge, window after RCCL.

  CASES                 dicts: id, kind, world, family (what the case is for) and the sizes
  plan(case, rank)      the rank's byte arena: buffers between poisoned fences, and its steps
  initial(case, rank)   the arena before the run.  Every SOURCE byte is tagged: the 16-byte unit u of buffer b of rank r holds the uint32
                        words (case serial, r, b, u) — a size that is no multiple of 16 takes the same bytes one by one — so a peer's data
                        is a function of its rank; everything else (destinations, fences in front and behind, gaps) is POISON, which no
                        tag equals (the first word of a tag is a small serial).
  expected(case, rank)  the arena after the run, receiver-centric, from the layout text of include/t2v_hip.h (ALLGATHER .. ALLTOALL) and the
                        comments above t2v_comm_allgather / _halo / _stats_halo / _alltoall.  Plain numpy; it shares no code with
                        csrc/comm.hip, parallel.ShardedExecutor or harness.run_lockstep.
  shares(case, rank)    MIRROR of px_exchange and peer_exchange_kernel (csrc/comm.hip, the line beside each formula): per step the
                        transport, per peer nb, the (u0, u1) of every segment and workgroup, trips of the receive loop, live loads of the
                        last trip, the slot parity from the pair's running sequence number.
  simulate(case, ...)   the same mirror executed on numpy windows, sender-centric, under the least friendly legal schedule (a rank pushes
                        message k + 1 as soon as it finished exchange k, before its peers read message k); VARIANTS are plausible wrong
                        implementations of it.  variant=None must equal expected (tests/test_collective_inputs_cpu.py).
  build(case, rank, alloc)  the records (program.Op with arena offsets; T2VOp with device addresses when `alloc` returns a base) and the arena.
"""
from __future__ import annotations

import collections
import functools

import numpy as np

from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd.program import NULL, Op, Ref

SLOT = 262144            # T2V_PEER_SLOT_MB=0.25: the slot the suite runs with
FENCE = 256
POISON = 0xA5
KINDS = ("ALLGATHER", "HALO_EXCHANGE", "STATS_HALO", "ALLTOALL")
_KIND_OF_OP = {"gather": "ALLGATHER", "direct": "ALLGATHER", "halo": "HALO_EXCHANGE", "stats_halo": "STATS_HALO", "alltoall": "ALLTOALL"}


def counts(frames: int, world: int):
    """Frames per slice of a clip split over `world` ranks: ceil(frames / world) each, a shorter last one."""
    base = -(-frames // world)
    return [base] * (world - 1) + [frames - base * (world - 1)]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
GATHER_SIZES = [(16, "one unit"), (512, "the deployed statistics part"), (8176, "top of nb = 1"), (8192, "nb = 2"),
                (8208, "513 units: shares 256 | 257"), (28688, "nb = 7, uneven shares"), (32752, "top of nb = 7"), (32768, "nb = 8"),
                (131072, "share of exactly 1024 units: one full trip"), (131200, "share 1025: second trip, one live lane"),
                (200016, "shares 1562 | 1563: mixed last trip"), (262144, "equal to the slot: window"), (262160, "above the slot: RCCL"),
                (6002, "not made of 16-byte units: RCCL")]
A2A_GEOMS = [(2, 5), (3, 7), (4, 10), (4, 8)]       # 3+2, 3+3+1, 3+3+3+1, 2+2+2+2
A2A_CHUNKS = [(16, "one unit per chunk"), (4112, "three chunks nb = 3 against one chunk nb = 1"), (10928, "32784 bytes nb = 8 against nb = 2"),
              (43744, "three chunks = 131232: a share above 1024 units"), (4100, "not 16-byte units: RCCL")]
SEQ_A2A = {2: 5, 3: 7, 4: 10}


def _sequence_steps(world):
    one = [dict(op="gather", bytes=131200), dict(op="halo", bytes=8208, F=2), dict(op="gather", bytes=6002), dict(op="gather", bytes=16),
           dict(op="stats_halo", part=512, frame=7680, F=2), dict(op="alltoall", frames=SEQ_A2A[world], chunk=4112, dir=0),
           dict(op="alltoall", frames=SEQ_A2A[world], chunk=4112, dir=1), dict(op="gather", bytes=512)]
    return [dict(s) for s in one] + [dict(s) for s in one]


def _make_cases():
    cases = []

    def add(cid, kind, world, family, steps, **kw):
        cases.append(dict(id=cid, kind=kind, world=world, family=family, steps=steps, serial=len(cases) + 1, **kw))

    for k, (n, why) in enumerate(GATHER_SIZES):
        for world in sorted({2 + k % 3} | ({2, 3, 4} if n in (512, 131200) else set())):
            add(f"gather-{n}-w{world}", "ALLGATHER", world, why, [dict(op="gather", bytes=n)], part_bytes=n)
    halos = [(2, 16, 1), (2, 8208, 3), (2, 131200, 1), (2, 262160, 3), (3, 16, 3), (3, 8208, 1), (3, 131200, 3), (3, 262160, 1),
             (4, 8208, 3), (4, 131200, 1)]
    for world, n, F in halos:
        add(f"halo-{n}-F{F}-w{world}", "HALO_EXCHANGE", world, "frame 1 is frame F" if F == 1 else "F = 3", [dict(op="halo", bytes=n, F=F)],
            frame_bytes=n, F=F)
    add("halo-200016-F2-w2", "HALO_EXCHANGE", 2, "shares 1562 | 1563: three live loads in the last trip", [dict(op="halo", bytes=200016, F=2)],
        frame_bytes=200016, F=2)
    add("halo-8208-Funeven-w3", "HALO_EXCHANGE", 3, "local frame counts differ per rank", [dict(op="halo", bytes=8208, F=[3, 2, 1])],
        frame_bytes=8208, F=[3, 2, 1])
    add("halo-6002-F1-w4", "HALO_EXCHANGE", 4, "not made of 16-byte units: RCCL", [dict(op="halo", bytes=6002, F=1)], frame_bytes=6002, F=1)
    add("halo-262144-F1-w2", "HALO_EXCHANGE", 2, "equal to the slot: window", [dict(op="halo", bytes=SLOT, F=1)], frame_bytes=SLOT, F=1)
    stats = [(512, 7680, "total 8192: nb = 2, segment split 16|16 and 240|240", (2, 3, 4)),
             (512, 40960, "second segment in shares of 320 units: two live loads in the only trip", (2,)),
             (16, 131200, "segment 0 has one unit: seven of eight workgroups have an empty share of it", (2, 3, 4)),
             (512, 200016, "second segment with a mixed last trip", (2, 3)), (500, 7680, "unit rule: RCCL", (2, 3)),
             (512, SLOT - 512, "part + frame equal to the slot: window", (2, 3)), (512, SLOT - 512 + 16, "part + frame = slot + 16: RCCL", (2, 3))]
    for part, frame, why, worlds in stats:
        for world in worlds:
            F = 1 if world == 3 else 2
            add(f"stats-{part}+{frame}-F{F}-w{world}", "STATS_HALO", world, why, [dict(op="stats_halo", part=part, frame=frame, F=F)],
                part_bytes=part, frame_bytes=frame, F=F)
    for world, frames in A2A_GEOMS:
        base = counts(frames, world)[0]
        above = -(-(SLOT + 16) // (16 * base)) * 16             # the smallest chunk of 16-byte units with base_cnt * chunk above the slot
        chunks = A2A_CHUNKS + [(above, f"base_cnt * chunk = {base * above}: just above the slot, RCCL")]
        if SLOT % base == 0 and (SLOT // base) % 16 == 0:
            chunks = chunks + [(SLOT // base, "base_cnt * chunk equal to the slot: window")]
        for chunk, why in chunks:
            for d in (0, 1):
                add(f"a2a-{frames}f-{chunk}-d{d}-w{world}", "ALLTOALL", world, why, [dict(op="alltoall", frames=frames, chunk=chunk, dir=d)],
                    frames=frames, chunk=chunk, dir=d)
    for world, frames in A2A_GEOMS:
        add(f"composite-{frames}f-w{world}", "COMPOSITE", world, "pack -> all-to-all 0 -> all-to-all 1 -> unpack + residual (hw = 48, c = 64)", None,
            frames=frames, hw=48, c=64)
    for world in (2, 3, 4):
        add(f"sequence-w{world}", "SEQUENCE", world, "both slots, shrink after grow, diverging pair sequence numbers, window after RCCL",
            _sequence_steps(world))
    for k, n in enumerate((16, 6002, 131200)):
        add(f"direct-{n}-w{2 + k}", "DIRECT", 2 + k, "t2v_comm_all_gather outside a plan", [dict(op="direct", bytes=n, base_off=0)], part_bytes=n)
    for world in (2, 3, 4):
        add(f"direct-8208-off8-w{world}", "DIRECT", world, "base 8 bytes off 16-byte alignment, the same on every rank",
            [dict(op="direct", bytes=8208, base_off=8)], part_bytes=8208, base_off=8)
    return cases


CASES = _make_cases()
BY_ID = {c["id"]: c for c in CASES}


# ---- tags ----------------------------------------------------------------------------------------------------------------------------
def tag_bytes(serial: int, rank: int, buf: int, off: int, n: int) -> np.ndarray:
    """Bytes [off, off + n) of buffer `buf` of rank `rank`: unit u = words (serial, rank, buf, u), little endian."""
    u0, u1 = off >> 4, (off + n + 15) >> 4
    w = np.empty((u1 - u0, 4), dtype="<u4")
    w[:, 0], w[:, 1], w[:, 2], w[:, 3] = serial, rank, buf, np.arange(u0, u1, dtype=np.uint32)
    return w.view(np.uint8).reshape(-1)[off - (u0 << 4): off - (u0 << 4) + n]


def decode_unit(b: np.ndarray):
    """16 bytes -> 'poison' or the tag (serial, sender, buffer, unit)."""
    if bytes(b) == bytes([POISON]) * 16:
        return "poison"
    return tuple(int(v) for v in np.frombuffer(bytes(b), dtype="<u4"))


# ---- the composite's clip (values, not tags: the check is arithmetic) -----------------------------------------------------------------
def _clip(case):
    """Global clip of the composite: N fp16 [F, hw, c] (the normalised tokens, frame split -> pixel split), Y fp32 (the block's result in the
    pixel split, on its way back) and X fp32 (the residual).  Every element distinct; Y + X is exact in fp32."""
    F, hw, c = case["frames"], case["hw"], case["c"]
    idx = np.arange(F * hw * c, dtype=np.int64).reshape(F, hw, c)
    n = (idx + 1 + case["serial"]).astype(np.uint16).view(np.float16)      # bit patterns below 0x7C00: finite, all distinct
    assert int(idx.max()) + 1 + case["serial"] < 0x7C00
    y = (idx + 0.5).astype(np.float32)
    x = (100000 + 2 * idx[::-1, ::-1, ::-1]).astype(np.float32)
    return n, y, x


# ---- plan: buffers and steps of one rank -----------------------------------------------------------------------------------------------
Plan = collections.namedtuple("Plan", "bufs steps size")        # bufs: name -> dict(off, size, id, tagged=[(off, n)], data=bytes or None)


def _layout(specs):
    bufs, cur = collections.OrderedDict(), 0
    for k, (name, size, tagged, data, mis) in enumerate(specs):
        off = -(-(cur + FENCE) // 256) * 256 + mis
        bufs[name] = dict(off=off, size=size, id=k, tagged=tagged, data=data)
        cur = off + size
    return bufs, -(-(cur + FENCE) // 256) * 256


@functools.lru_cache(maxsize=None)
def _plan(cid: str, rank: int) -> Plan:
    case = BY_ID[cid]
    world = case["world"]
    if case["kind"] == "COMPOSITE":
        return _plan_composite(case, rank)
    specs, steps = [], []
    for k, st in enumerate(case["steps"]):
        st = dict(st)
        b = [f"s{k}.b0", f"s{k}.b1"]
        if st["op"] in ("gather", "direct"):
            n = st["bytes"]
            specs.append((b[0], world * n, [(rank * n, n)], None, st.get("base_off", 0)))
            st["bufs"] = b[:1]
        elif st["op"] == "halo":
            n = st["bytes"]
            st["Fs"] = list(st["F"]) if isinstance(st["F"], (list, tuple)) else [st["F"]] * world
            F = st["Fs"][rank]
            specs.append((b[0], (F + 2) * n, [(n, F * n)], None, 0))
            st["bufs"] = b[:1]
        elif st["op"] == "stats_halo":
            p, n, F = st["part"], st["frame"], st["F"]
            st["Fs"] = [F] * world
            specs.append((b[0], world * p, [(rank * p, p)], None, 0))
            specs.append((b[1], (F + 2) * n, [(n, F * n)], None, 0))
            st["bufs"] = b
        else:
            cnt, ch = counts(st["frames"], world), st["chunk"]
            st["cnt"] = cnt
            ssize = world * (cnt[rank] if st["dir"] == 0 else cnt[0]) * ch
            rsize = world * (cnt[0] if st["dir"] == 0 else cnt[rank]) * ch
            specs.append((b[0], ssize, [(0, ssize)], None, 0))
            specs.append((b[1], rsize, [], None, 0))
            st["bufs"] = b
        steps.append(st)
    bufs, size = _layout(specs)
    return Plan(bufs, steps, size)


def _plan_composite(case, rank) -> Plan:
    """Buffers of unet.temporal_transformer_resharded around its two all-to-alls: n (frame split, fp16), stage, xp (pixel split), yp (the
    block's fp32 result, pixel split: an input here), back, x (residual) and out."""
    world, hw, c = case["world"], case["hw"], case["c"]
    cnt = counts(case["frames"], world)
    Ft, Fl, hwr, o = case["frames"], cnt[rank], hw // world, sum(cnt[:rank])
    n, y, x = _clip(case)
    px = slice(rank * hwr, (rank + 1) * hwr)
    specs = [("n", Fl * hw * c * 2, [], n[o:o + Fl].tobytes(), 0), ("stage", world * Fl * hwr * c * 2, [], None, 0),
             ("xp", Ft * hwr * c * 2, [], None, 0), ("yp", Ft * hwr * c * 4, [], np.ascontiguousarray(y[:, px]).tobytes(), 0),
             ("back", world * Fl * hwr * c * 4, [], None, 0), ("x", Fl * hw * c * 4, [], x[o:o + Fl].tobytes(), 0),
             ("out", Fl * hw * c * 4, [], None, 0)]
    bufs, size = _layout(specs)
    geo = dict(parts=world, rows=Fl * hwr, cols=c, chunk=hwr, own=rank, own_rows=o * hwr)
    steps = [dict(op="reshard", src="n", dst="stage", own_other="xp", own_is_src=False, dtype="f16", s_src=hw, s_dst=hwr, part_rows_src=hwr,
                  part_rows_dst=Fl * hwr, residual=None, **geo),
             dict(op="alltoall", frames=Ft, chunk=hwr * c * 2, dir=0, cnt=cnt, bufs=["stage", "xp"]),
             dict(op="alltoall", frames=Ft, chunk=hwr * c * 4, dir=1, cnt=cnt, bufs=["yp", "back"]),
             dict(op="reshard", src="back", dst="out", own_other="yp", own_is_src=True, dtype="f32", s_src=hwr, s_dst=hw, part_rows_src=Fl * hwr,
                  part_rows_dst=hwr, residual="x", **geo)]
    return Plan(bufs, steps, size)


def plan(case, rank) -> Plan:
    return _plan(case["id"], rank)


@functools.lru_cache(maxsize=64)
def _initial(cid: str, rank: int) -> np.ndarray:
    case = BY_ID[cid]
    pl = _plan(cid, rank)
    a = np.full(pl.size, POISON, dtype=np.uint8)
    for b in pl.bufs.values():
        if b["data"] is not None:
            a[b["off"]: b["off"] + b["size"]] = np.frombuffer(b["data"], dtype=np.uint8)
        for off, n in b["tagged"]:
            a[b["off"] + off: b["off"] + off + n] = tag_bytes(case["serial"], rank, b["id"], off, n)
    a.setflags(write=False)
    return a


def initial(case, rank) -> np.ndarray:
    return _initial(case["id"], rank).copy()


# ---- expected: what the header says lands where ------------------------------------------------------------------------------------------
def _peer_src(case, q, name, off, n):
    """Bytes [off, off + n) of buffer `name` of rank q before the run — a function of (case, q): no step writes a byte another step sends."""
    b = _plan(case["id"], q).bufs[name]
    assert off >= 0 and off + n <= b["size"]
    return _initial(case["id"], q)[b["off"] + off: b["off"] + off + n]


def expected(case, rank) -> np.ndarray:
    if case["kind"] == "COMPOSITE":
        return _expected_composite(case, rank)
    world, pl = case["world"], plan(case, rank)
    a = initial(case, rank)

    def put(name, off, data):
        b = pl.bufs[name]
        assert off >= 0 and off + len(data) <= b["size"]
        a[b["off"] + off: b["off"] + off + len(data)] = data

    for st in pl.steps:
        op, bufs = st["op"], st["bufs"]
        if op in ("gather", "direct", "stats_halo"):
            # "part q of `nparts` equal parts lives at base + q*bytes; this rank's part is already in place"
            n = st["part"] if op == "stats_halo" else st["bytes"]
            for q in range(world):
                if q != rank:
                    put(bufs[0], q * n, _peer_src(case, q, bufs[0], q * n, n))
        if op in ("halo", "stats_halo"):
            # "sends its first real frame to `prev` and its last to `next`, and receives their boundary frames into frame 0 / F+1"
            n, name, Fs = (st["frame"], bufs[1], st["Fs"]) if op == "stats_halo" else (st["bytes"], bufs[0], st["Fs"])
            if rank > 0:
                put(name, 0, _peer_src(case, rank - 1, name, Fs[rank - 1] * n, n))           # the previous rank's LAST real frame
            if rank + 1 < world:
                put(name, (Fs[rank] + 1) * n, _peer_src(case, rank + 1, name, n, n))        # the next rank's FIRST real frame
        if op == "alltoall":
            cnt, ch = st["cnt"], st["chunk"]
            for q in range(world):
                if q == rank:
                    continue
                if st["dir"] == 0:      # "receive cnt(q) chunks from q at p1 + q*i[4]*chunk"; q sent them "from p0 + me*cnt(q)*chunk" of ITS buffer
                    put(bufs[1], q * cnt[0] * ch, _peer_src(case, q, bufs[0], rank * cnt[q] * ch, cnt[q] * ch))
                else:                   # "receive cnt(me) chunks from q at p1 + q*cnt(me)*chunk"; q sent them "from p0 + me*i[4]*chunk"
                    put(bufs[1], q * cnt[rank] * ch, _peer_src(case, q, bufs[0], rank * cnt[0] * ch, cnt[rank] * ch))
    return a


def _expected_composite(case, rank) -> np.ndarray:
    """From the GLOBAL clip: xp is the clip's pixel split, out = Y + X on this rank's frames; stage / back hold the peers' parts (the rank's
    own part never goes through them: it keeps its poison)."""
    world, hw, c = case["world"], case["hw"], case["c"]
    cnt = counts(case["frames"], world)
    Fl, hwr, o = cnt[rank], hw // world, sum(cnt[:rank])
    n, y, x = _clip(case)
    pl, a = plan(case, rank), initial(case, rank)

    def put(name, off, arr):
        raw = np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8)
        b = pl.bufs[name]
        assert off + len(raw) <= b["size"]
        a[b["off"] + off: b["off"] + off + len(raw)] = raw

    for q in range(world):
        if q != rank:
            put("stage", q * Fl * hwr * c * 2, n[o:o + Fl, q * hwr:(q + 1) * hwr])
            put("back", q * Fl * hwr * c * 4, y[o:o + Fl, q * hwr:(q + 1) * hwr])
    put("xp", 0, n[:, rank * hwr:(rank + 1) * hwr])
    put("out", 0, y[o:o + Fl] + x[o:o + Fl])
    return a


def pixel_split(case, rank) -> np.ndarray:
    """The composite's pixel-sharded intermediate of `rank`, from the global clip."""
    hwr = case["hw"] // case["world"]
    return np.ascontiguousarray(_clip(case)[0][:, rank * hwr:(rank + 1) * hwr])


# ---- mirror of csrc/comm.hip -------------------------------------------------------------------------------------------------------------
PX_NB = 8                                                   # comm.hip:36


def px_nb_host(nbytes: int) -> int:                         # comm.hip:145-148: bytes >> 12 clamped to 1 .. PX_NB
    return min(max(nbytes >> 12, 1), PX_NB)


def share(units: int, j: int, nb: int):                     # comm.hip:159 / 195: u0 = units * j / nb, u1 = units * (j + 1) / nb
    return units * j // nb, units * (j + 1) // nb


def trips_of(n: int):
    """Receive loop of a share of n units (comm.hip:196-205: lane tid starts at u0 + tid, stride 1024, four loads 256 units apart):
    (trips, loads of the last trip that have a live lane)."""
    if n <= 0:
        return 0, 0
    trips = -(-n // 1024)
    return trips, -(-(n - (trips - 1) * 1024) // 256)


VARIANTS = collections.OrderedDict([
    ("nb-from-other-direction", "receive share bounds from nb_send instead of nb_recv"),
    ("offset-not-advanced", "the slot offset `off` stays 0 for the second segment"),
    ("k3-load-dropped", "the fourth load of a trip (units 768..1023 of every 1024) is never copied out"),
    ("second-trip-dropped", "the receive loop runs one trip only"),
    ("floor-share", "u1 = u0 + units / nb: the remainder of an uneven split is nobody's"),
    ("parity-fixed", "every message of a pair uses slot 0"),
    ("stale-tail", "the receiver copies the length of the previous message of the slot when that was longer"),
    ("cnt-swapped", "all-to-all: cnt(q) and cnt(me) swapped in the message sizes"),
    ("stride-swapped", "all-to-all: base_cnt and cnt(me) strides swapped"),
    ("prev-next-swapped", "halo: frame 1 goes to next, frame F to prev"),
    ("frame-F-for-F+1", "halo: the next rank's frame lands in frame F instead of F + 1"),
    ("gather-sends-part-0", "all-gather: every rank sends part 0 instead of its own"),
])


def messages(st, rank, world, variant=None):
    """One step as t2v_comm_* hands it to px_exchange: ([(q, [(buffer, off, n)] * 2 sent, the same received)], max_bytes, unit)."""
    op, bufs, v = st["op"], st["bufs"], variant
    msgs = []
    if op in ("gather", "direct"):                                                         # comm.hip:409-411
        n = st["bytes"]
        so = 0 if v == "gather-sends-part-0" else rank * n
        for q in range(world):
            if q != rank:
                msgs.append((q, [(bufs[0], so, n), None], [(bufs[0], q * n, n), None]))
        return msgs, n, n
    if op in ("halo", "stats_halo"):
        n, name, F = (st["frame"], bufs[1], st["Fs"][rank]) if op == "stats_halo" else (st["bytes"], bufs[0], st["Fs"][rank])
        prev, nxt = (rank - 1 if rank > 0 else -1), (rank + 1 if rank + 1 < world else -1)
        first, last = (F, 1) if v == "prev-next-swapped" else (1, F)
        to_prev = ((name, first * n, n), (name, 0, n))                                     # comm.hip:433 / 469
        to_next = ((name, last * n, n), (name, ((F if v == "frame-F-for-F+1" else F + 1)) * n, n))   # comm.hip:434 / 470
        if op == "halo":
            if prev >= 0:
                msgs.append((prev, [to_prev[0], None], [to_prev[1], None]))
            if nxt >= 0:
                msgs.append((nxt, [to_next[0], None], [to_next[1], None]))
            return msgs, n, n                                                              # comm.hip:436
        p = st["part"]
        for q in range(world):                                                             # comm.hip:466-472
            if q == rank:
                continue
            s, r = [(bufs[0], rank * p, p), None], [(bufs[0], q * p, p), None]
            if q == prev:
                s[1], r[1] = to_prev
            if q == nxt:
                s[1], r[1] = to_next
            msgs.append((q, s, r))
        return msgs, p + n, (1 if (p | n) & 15 else 16)                                    # comm.hip:474
    cnt, ch, base = st["cnt"], st["chunk"], st["cnt"][0]
    me = cnt[rank]
    for q in range(world):                                                                 # comm.hip:511-515
        if q == rank:
            continue
        a, b = (cnt[q], me) if v == "cnt-swapped" else (me, cnt[q])
        big, small = (me, base) if v == "stride-swapped" else (base, me)
        if st["dir"] == 0:
            msgs.append((q, [(bufs[0], q * small * ch, a * ch), None], [(bufs[1], q * big * ch, b * ch), None]))
        else:
            msgs.append((q, [(bufs[0], q * big * ch, b * ch), None], [(bufs[1], q * small * ch, a * ch), None]))
    return msgs, base * ch, ch                                                             # comm.hip:517


def transport(max_bytes, unit, window=True):
    """comm.hip:233: the window carries an op whose largest message fits a slot and whose segments are 16-byte units."""
    if not window:
        return "rccl:off"
    if unit & 15:
        return "rccl:unit"
    return "window" if max_bytes <= SLOT else "rccl:size"


def _seglen(seg):
    return 0 if seg is None else seg[2]


def shares(case, rank, window=True, seq0=None):
    """Per collective step of `rank`: dict(step, kind, transport, peers=[dict(q, seq, parity, nb_send, nb_recv, send=[[(u0, u1)] per
    workgroup] per segment, recv=..., trips, last_live, sbytes, rbytes)]).  seq0: the pairs' sequence numbers before the case."""
    world, pl = case["world"], plan(case, rank)
    seq = dict(seq0 or {})
    out = []
    for k, st in enumerate(pl.steps):
        if st["op"] == "reshard":
            continue
        msgs, max_bytes, unit = messages(st, rank, world)
        tr = transport(max_bytes, unit, window)
        peers = []
        for q, s, r in msgs:
            sb, rb = [_seglen(x) for x in s], [_seglen(x) for x in r]
            d = dict(q=q, sbytes=sb, rbytes=rb)
            if tr == "window":
                seq[q] = seq.get(q, 0) + 1                                                 # comm.hip:251
                nbs, nbr = px_nb_host(sum(sb)), px_nb_host(sum(rb))                        # comm.hip:264-265
                d.update(seq=seq[q], parity=seq[q] & 1, nb_send=nbs, nb_recv=nbr,          # comm.hip:252
                         send=[[share(n >> 4, j, nbs) for j in range(nbs)] for n in sb],
                         recv=[[share(n >> 4, j, nbr) for j in range(nbr)] for n in rb])
                tl = [trips_of(u1 - u0) for seg in d["recv"] for u0, u1 in seg]
                d.update(trips=max(t for t, _ in tl), last_live=sorted({l for t, l in tl if t}))
            peers.append(d)
        nbmax = max([max(p["nb_send"], p["nb_recv"]) for p in peers if "nb_send" in p] or [1])       # comm.hip:266-268
        out.append(dict(step=k, kind=_KIND_OF_OP[st["op"]], transport=tr, peers=peers, nbmax=nbmax))
    return out


def predicted_counters(case, rank, window=True):
    """(exchanges over the window, exchanges through RCCL) the case adds to t2v_comm_counters of `rank`."""
    trs = [s["transport"] for s in shares(case, rank, window) if s["peers"]]
    return sum(t == "window" for t in trs), sum(t != "window" for t in trs)


# ---- the mirror, executed -----------------------------------------------------------------------------------------------------------------
def _reshard(a, pl, st):
    """T2V_OP_RESHARD_ROWS, multi-part form, on the numpy arena (the composite's pack / unpack between the collectives)."""
    dt = np.float16 if st["dtype"] == "f16" else np.float32
    item, cols = np.dtype(dt).itemsize, st["cols"]
    view = lambda name, off_rows: a[pl.bufs[name]["off"] + off_rows * cols * item:].view(dt)
    r = np.arange(st["rows"])
    rs, rd = (r // st["chunk"]) * st["s_src"] + r % st["chunk"], (r // st["chunk"]) * st["s_dst"] + r % st["chunk"]
    for q in range(st["parts"]):
        own = q == st["own"]
        src = view(st["own_other"], st["own_rows"]) if own and st["own_is_src"] else view(st["src"], q * st["part_rows_src"])
        dst = view(st["own_other"], st["own_rows"]) if own and not st["own_is_src"] else view(st["dst"], q * st["part_rows_dst"])
        val = src[: (int(rs.max()) + 1) * cols].reshape(-1, cols)[rs]
        if st["residual"]:
            val = val + view(st["residual"], q * st["part_rows_dst"])[: (int(rd.max()) + 1) * cols].reshape(-1, cols)[rd]
        dst[: (int(rd.max()) + 1) * cols].reshape(-1, cols)[rd] = val


def simulate(case, variant=None, window=True):
    """All ranks of the case on numpy arenas and numpy windows -> [arena of rank 0, ...].  Schedule: every rank pushes message k; then, in
    rank order, a rank copies message k out of its window and at once pushes message k + 1 (it has finished exchange k: the protocol
    allows it) — so the peers behind it read message k with k + 1 already sitting in the other slot."""
    world = case["world"]
    pls = [plan(case, r) for r in range(world)]
    arenas = [initial(case, r) for r in range(world)]
    slots, prev_len = {}, {}
    seq = [collections.Counter() for _ in range(world)]
    pending = [dict() for _ in range(world)]
    v = variant

    def rng(r, seg):
        b = pls[r].bufs[seg[0]]
        return b["off"] + seg[1], seg[2]

    def window_step(k):
        if k >= len(pls[0].steps) or pls[0].steps[k]["op"] == "reshard":
            return False
        _, mb, unit = messages(pls[0].steps[k], 0, world, v)
        return transport(mb, unit, window) == "window"

    def bounds(units, j, nb):
        u0, u1 = share(units, j, nb)
        return (u0, u0 + units // nb) if v == "floor-share" else (u0, u1)

    def push(r, k):
        if k in pending[r]:
            return
        msgs, _, _ = messages(pls[r].steps[k], r, world, v)
        pending[r][k] = []
        for q, s, rv in msgs:
            seq[r][q] += 1
            sq = seq[r][q]
            par = 0 if v == "parity-fixed" else sq & 1
            slot = slots.setdefault((q, r, par), np.zeros(SLOT + 4096, dtype=np.uint8))
            sb, rb = [_seglen(x) for x in s], [_seglen(x) for x in rv]
            nbs = px_nb_host(sum(sb))
            off = 0
            for sg in range(2):
                if sb[sg]:
                    o, n = rng(r, s[sg])
                    for j in range(nbs):
                        u0, u1 = bounds(n >> 4, j, nbs)
                        slot[off + (u0 << 4): off + (u1 << 4)] = arenas[r][o + (u0 << 4): o + (u1 << 4)]
                if v != "offset-not-advanced":
                    off += sb[sg]
            pending[r][k].append((q, rv, sb, rb, par))

    def pull(r, k):
        for q, rv, sb, rb, par in pending[r][k]:
            slot = slots.setdefault((r, q, par), np.zeros(SLOT + 4096, dtype=np.uint8))
            nbr = px_nb_host(sum(rb))
            nb_bounds = px_nb_host(sum(sb)) if v == "nb-from-other-direction" else nbr
            off = 0
            last = max(sg for sg in range(2) if rb[sg]) if any(rb) else -1
            for sg in range(2):
                if rb[sg]:
                    o, n = rng(r, rv[sg])
                    units = n >> 4
                    if v == "stale-tail" and sg == last and prev_len.get((r, q, par), 0) > sum(rb):
                        units += (prev_len[(r, q, par)] - sum(rb)) >> 4
                    live = np.zeros(units, dtype=bool)
                    for j in range(nbr):
                        u0, u1 = bounds(units, j, nb_bounds)
                        u0, u1 = min(u0, units), min(u1, units)
                        rel = np.arange(u1 - u0)
                        keep = np.ones(u1 - u0, dtype=bool)
                        if v == "k3-load-dropped":
                            keep &= rel % 1024 < 768
                        if v == "second-trip-dropped":
                            keep &= rel < 1024
                        live[u0:u1] |= keep
                    idx = np.nonzero(np.repeat(live, 16))[0]
                    idx = idx[(o + idx < arenas[r].size) & (off + idx < slot.size)]
                    arenas[r][o + idx] = slot[off + idx]
                if v != "offset-not-advanced":
                    off += rb[sg]
            prev_len[(r, q, par)] = sum(rb)

    for k in range(len(pls[0].steps)):
        op = pls[0].steps[k]["op"]
        if op == "reshard":
            for r in range(world):
                _reshard(arenas[r], pls[r], pls[r].steps[k])
        elif window_step(k):
            for r in range(world):
                push(r, k)
            for r in range(world):
                pull(r, k)
                if window_step(k + 1):
                    push(r, k + 1)
        else:       # RCCL: the sends and receives of a pair match in order, each receive takes what its send carries
            sent = {}
            for r in range(world):
                for q, s, _ in messages(pls[r].steps[k], r, world, v)[0]:
                    sent[(r, q)] = [arenas[r][rng(r, x)[0]: rng(r, x)[0] + x[2]].copy() for x in s if x is not None]
            for r in range(world):
                for q, _, rv in messages(pls[r].steps[k], r, world, v)[0]:
                    for data, x in zip(sent.get((q, r), []), [x for x in rv if x is not None]):
                        o, n = rng(r, x)
                        m = min(n, len(data))
                        arenas[r][o: o + m] = data[:m]
    return arenas


# ---- records ------------------------------------------------------------------------------------------------------------------------------
Built = collections.namedtuple("Built", "arena ops records base plan direct")


def build(case, rank, alloc=None) -> Built:
    """The rank's records and buffers.  ops: program.Op with arena offsets (what the host executors read); records: the same as T2VOp over
    base = alloc(arena bytes) (a device address), None without `alloc`; direct: (byte offset, bytes) of a t2v_comm_all_gather call instead
    of a plan (kind DIRECT)."""
    world, pl = case["world"], plan(case, rank)
    ops, direct = [], None
    off = lambda name: pl.bufs[name]["off"]
    for k, st in enumerate(pl.steps):
        if st["op"] == "direct":
            direct = (off(st["bufs"][0]), st["bytes"])
        prev, nxt = (rank - 1 if rank > 0 else -1), (rank + 1 if rank + 1 < world else -1)
        if st["op"] in ("gather", "direct"):
            op = Op(L.OP_ALLGATHER, f"{case['id']}.{k}")
            op.i[0:4] = [st["bytes"] & 0xFFFFFFFF, st["bytes"] >> 32, world, rank]
            op.p[0] = Ref("arena", off(st["bufs"][0]))
        elif st["op"] == "halo":
            op = Op(L.OP_HALO_EXCHANGE, f"{case['id']}.{k}")
            op.i[0:5] = [st["bytes"] & 0xFFFFFFFF, st["bytes"] >> 32, st["Fs"][rank], prev, nxt]
            op.p[0] = Ref("arena", off(st["bufs"][0]))
        elif st["op"] == "stats_halo":
            op = Op(L.OP_STATS_HALO, f"{case['id']}.{k}")
            op.i[0:9] = [st["part"] & 0xFFFFFFFF, st["part"] >> 32, world, rank, st["frame"] & 0xFFFFFFFF, st["frame"] >> 32, st["Fs"][rank], prev, nxt]
            op.p[0], op.p[1] = Ref("arena", off(st["bufs"][0])), Ref("arena", off(st["bufs"][1]))
        elif st["op"] == "alltoall":
            op = Op(L.OP_ALLTOALL, f"{case['id']}.{k}")
            op.i[0:7] = [st["chunk"] & 0xFFFFFFFF, st["chunk"] >> 32, world, rank, st["cnt"][0], st["cnt"][-1], st["dir"]]
            op.p[0], op.p[1] = Ref("arena", off(st["bufs"][0])), Ref("arena", off(st["bufs"][1]))
        else:       # RESHARD_ROWS, multi-part form (include/t2v_hip.h; program.Program.reshard_parts)
            item, c = (2, st["cols"]) if st["dtype"] == "f16" else (4, st["cols"])
            op = Op(L.OP_RESHARD_ROWS, f"{case['id']}.{k}")
            op.i[0:8] = [st["rows"], c, st["chunk"], st["s_src"], st["s_dst"], c, c, L.F16 if st["dtype"] == "f16" else L.F32]
            op.i[9:15] = [st["parts"], st["part_rows_src"] * c, st["part_rows_dst"] * c, 0, st["own"], 1 if st["own_is_src"] else 0]
            op.p[0], op.p[1] = Ref("arena", off(st["src"])), Ref("arena", off(st["dst"]))
            op.p[3] = Ref("arena", off(st["own_other"]) + st["own_rows"] * c * item)
            if st["residual"]:
                op.i[8], op.i[12] = c, st["part_rows_dst"] * c
                op.p[2] = Ref("arena", off(st["residual"]))
        ops.append(op)
    base = records = None
    if alloc is not None:
        base = int(alloc(pl.size))
        records = (L.T2VOp * len(ops))()
        for rec, op in zip(records, ops):
            rec.kind, rec.tag = op.kind, 0
            for j, val in enumerate(op.i):
                rec.i[j] = val
            for j, ref in enumerate(op.p):
                rec.p[j] = 0 if ref is NULL or ref.space == "null" else base + ref.off
    return Built(initial(case, rank), ops, records, base, pl, direct)


# ---- reading a mismatch ----------------------------------------------------------------------------------------------------------------------
def where(case, rank, pos: int) -> str:
    """Arena byte `pos` of `rank` -> 'buffer name + offset' or the fence it lies in."""
    before = "front"
    for name, b in plan(case, rank).bufs.items():
        if b["off"] <= pos < b["off"] + b["size"]:
            return f"{name}+{pos - b['off']}"
        if b["off"] + b["size"] <= pos:
            before = name
    return f"fence behind {before}"


def first_difference(case, rank, got: np.ndarray, want: np.ndarray):
    """None, or a line naming the first differing 16-byte unit: where it lies, the tag found there and the tag expected."""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return f"arena of {got.size} bytes, expected {want.size}"
    pos = int(np.nonzero(got != want)[0][0])
    u = pos & ~15
    ids = {b["id"]: name for name, b in plan(case, rank).bufs.items()}

    def say(t):
        return t if t == "poison" else f"(serial {t[0]}, sender {t[1]}, buffer {ids.get(t[2], t[2])}, unit {t[3]})"

    return (f"case {case['id']} rank {rank}: first wrong byte {pos} = {where(case, rank, pos)}; unit there holds {say(decode_unit(got[u:u + 16]))}, "
            f"expected {say(decode_unit(want[u:u + 16]))}; {int((got != want).sum())} bytes differ")


# ---- coverage classes ---------------------------------------------------------------------------------------------------------------------
CLASSES = ["nb = 1", "nb in 2..7", "nb = 8", "units % nb != 0", "empty share", "trips > 1", "last trip: 1 live load", "last trip: 2 live loads",
           "last trip: 3 live loads", "nb_send != nb_recv", "idle workgroups", "transport window", "transport rccl:size", "transport rccl:unit",
           "slot boundary: equal", "slot boundary: above"]
SUITE_CLASSES = ["slot parity 0", "slot parity 1", "shrink after grow in one slot", "window op after an RCCL op", "pair sequence numbers diverge"]
# (kind, class) that no record of that kind can reach, and why
CANNOT = {}
for _k in ("ALLGATHER", "HALO_EXCHANGE"):
    CANNOT[(_k, "empty share")] = "one segment: nb >= 2 needs >= 8192 bytes = 512 units, so every workgroup has >= 64 units"
    CANNOT[(_k, "nb_send != nb_recv")] = "a rank sends and receives the same number of bytes"
    CANNOT[(_k, "idle workgroups")] = "every peer of the launch has the same message size, so nb == nbmax"
CANNOT[("STATS_HALO", "nb_send != nb_recv")] = "a rank sends a peer the part (+ frame) sizes it receives from it"
CANNOT[("ALLTOALL", "empty share")] = CANNOT[("ALLGATHER", "empty share")]


def classes_of(case):
    """{(kind, class)} and {suite class} the case reaches, over all of its ranks (from shares())."""
    hit, suite = set(), set()
    world = case["world"]
    allseq = []
    for rank in range(world):
        last_in_slot, seen_rccl = {}, False
        sh = shares(case, rank)
        for s in sh:
            k = s["kind"]
            if not s["peers"]:
                continue
            hit.add((k, "transport " + s["transport"]))
            _, mb, _ = messages(plan(case, rank).steps[s["step"]], rank, world)
            if mb == SLOT:
                hit.add((k, "slot boundary: equal"))
            if SLOT < mb <= SLOT + 64:
                hit.add((k, "slot boundary: above"))
            if s["transport"] != "window":
                seen_rccl = True
                continue
            if seen_rccl:
                suite.add("window op after an RCCL op")
            for p in s["peers"]:
                for nb in (p["nb_send"], p["nb_recv"]):
                    hit.add((k, "nb = 1" if nb == 1 else "nb = 8" if nb == 8 else "nb in 2..7"))
                    if nb < s["nbmax"]:
                        hit.add((k, "idle workgroups"))
                if p["nb_send"] != p["nb_recv"]:
                    hit.add((k, "nb_send != nb_recv"))
                for nbytes, nb, segs in ((p["sbytes"], p["nb_send"], p["send"]), (p["rbytes"], p["nb_recv"], p["recv"])):
                    for n, seg in zip(nbytes, segs):
                        if n and (n >> 4) % nb:
                            hit.add((k, "units % nb != 0"))
                        if n and any(u0 == u1 for u0, u1 in seg):
                            hit.add((k, "empty share"))
                if p["trips"] > 1:
                    hit.add((k, "trips > 1"))
                for l in p["last_live"]:
                    if l in (1, 2, 3):
                        hit.add((k, f"last trip: {l} live load" + ("s" if l > 1 else "")))
                suite.add(f"slot parity {p['parity']}")
                key = (p["q"], p["parity"])
                if last_in_slot.get(key, 0) > sum(p["rbytes"]):
                    suite.add("shrink after grow in one slot")
                last_in_slot[key] = sum(p["rbytes"])
        final = collections.Counter()
        for s in sh:
            for p in s["peers"]:
                if "seq" in p:
                    final[p["q"]] = p["seq"]
        allseq.append(final)
    if any(len(set(f.values())) > 1 for f in allseq if len(f) > 1):
        suite.add("pair sequence numbers diverge")
    return hit, suite


def coverage(cases=None):
    """-> (by class: {(kind, class): [case id]}, suite: {class: [case id]}, missing: [str])."""
    by, suite = collections.OrderedDict(), collections.OrderedDict()
    for c in (CASES if cases is None else cases):
        hit, su = classes_of(c)
        for key in hit:
            by.setdefault(key, []).append(c["id"])
        for key in su:
            suite.setdefault(key, []).append(c["id"])
    missing = [f"{k}: {cl}" for k in KINDS for cl in CLASSES if (k, cl) not in CANNOT and not by.get((k, cl))]
    missing += [f"suite: {cl}" for cl in SUITE_CLASSES if not suite.get(cl)]
    return by, suite, missing
