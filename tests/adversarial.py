"""TEST INFRASTRUCTURE — adversarial inputs for the streaming-softmax attention kernels (csrc/attention.hip), a float64 reference and a
float64 emulation of the kernels' stale-maximum schedule.  No test functions here: tests/test_adversarial_inputs_cpu.py checks that the
inputs do what they are meant to do, tests/test_gpu_attention_adversarial.py runs the kernels on them.  Both import the case lists below,
so they cannot drift apart.

Nothing in this module imports the product or tests/interp.py: the expected values of the GPU tests come from `softmax_attention_ref`.

Why these inputs.  attn_kernel, attn2_kernel and relpos_long_kernel stream the keys in tiles and advance the running maximum only when a
tile's maximum exceeds it by more than 2^8; O, l (and the long-clip kernel's edge masses w_lo / w_hi) are then multiplied by
alpha = exp2(m_run - m_tile).  On `randn` inputs the scaled logits spread over a few log2 units, so after the first tile (alpha = 0) that
multiplication never runs with a non-trivial alpha.  `late_max_qkv` plants, per (pixel, head) item, one key whose logit rises ~9.5 log2 units
above the rest for the even queries and another for the odd queries, in tiles that vary with the item; the other keys keep a visible
share of the mass, so a wrong alpha changes the output by far more than any tolerance.  `masked_spike` plants a logit 40 log2 units above
the rest where the kernel must not see it: a maximum taken before the mask underflows every probability of the row."""
from __future__ import annotations

import math

import torch

LOG2E = 1.4426950408889634
GROW = 8.0          # the kernels advance the running maximum only by more than this many log2 units
AMP = 4.0           # length of the query component along its direction
MASKED_RISE = 40.0  # log2 units of the spikes of masked_spike


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _f16(t: torch.Tensor) -> torch.Tensor:
    return t.half().double()


def _background(items, nq, nk, D, seed, noise):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(2, D, generator=g, dtype=torch.float64)
    u[0] /= u[0].norm()
    u[1] -= (u[1] @ u[0]) * u[0]
    u[1] /= u[1].norm()
    q = noise * torch.randn(items, nq, D, generator=g, dtype=torch.float64)
    k = noise * torch.randn(items, nk, D, generator=g, dtype=torch.float64)
    v = torch.randn(items, nk, D, generator=g, dtype=torch.float64)
    q = q + AMP * u[torch.arange(nq) % 2][None]          # even queries carry u0, odd queries u1
    return q, k, v, u


def spike_keys(item, nk, tile, placement="cycle", shift=0):
    """Keys of the u0 and the u1 spike of `item`.  'cycle': tile (item + shift) % ntiles resp. (3 item + 1 + shift) % ntiles, the place inside
    the tile varies with the item.  'second': both in the second tile, at its first keys (below most queries of a causal mask, inside a short
    ragged second tile)."""
    ntiles = -(-nk // tile)
    assert placement in ("cycle", "second")
    if placement == "second" and ntiles >= 2:
        return tile + item % 2, tile + 2 + item % 2
    s0 = min(((item + shift) % ntiles) * tile + (7 * item) % tile, nk - 1)
    s1 = min(((3 * item + 1 + shift) % ntiles) * tile + (7 * item + 4) % tile, nk - 1)
    if s1 == s0:
        s1 = s0 - 1 if s0 > 0 else min(1, nk - 1)
    return s0, s1


def _plant(k, u, items, nk, tile, scale, rise, low_rise, low_every, placement, shift):
    c = 1.0 / (scale * LOG2E * AMP)
    for it in range(items):
        s0, s1 = spike_keys(it, nk, tile, placement, shift)
        k[it, s0] += rise * c * u[0]
        k[it, s1] += (low_rise if low_every and it % low_every == 0 else rise) * c * u[1]


def late_max_qkv(items, nq, nk, D, tile, scale, seed, rise=9.5, low_rise=6.0, low_every=3, noise=0.35, placement="cycle", shift=0):
    """fp16-representable float64 q [items, nq, D], k, v [items, nk, D].  Background 0.35 randn (q, k) / randn (v); even queries + 4 u0, odd
    queries + 4 u1 (u0, u1 orthonormal); per item one key + rise / (scale log2(e) 4) u0 and another the same along u1 (every `low_every`-th
    item: `low_rise`, a rise below the threshold, whose probabilities of up to 2^8 go through the fp16 P operand)."""
    q, k, v, u = _background(items, nq, nk, D, seed, noise)
    _plant(k, u, items, nk, tile, scale, rise, low_rise, low_every, placement, shift)
    return _f16(q), _f16(k), _f16(v)


def masked_spike(items, nq, nk, D, tile, scale, seed, mode, spiked=(), noise=0.35, placement="cycle", shift=0, rise=9.5):
    """The late-maximum inputs plus a logit MASKED_RISE log2 units above the rest, seen alike by even and odd queries.
    mode 'causal': at one key s per item (the first two keys of the second tile, the last key of the first tile, the last key, by item);
      queries t < s must not see it, queries t >= s do.
    mode 'after': at key 0 of the items listed in `spiked`, which see it legitimately (their output is v[0]); the caller lays the items out
      so that this row follows another item's last key in memory, and fills the spare rows behind the last item with `spare_k`.
    Returns q, k, v, spare_k [D], keys (the spiked key per item, -1 = none)."""
    q, k, v, u = _background(items, nq, nk, D, seed, noise)
    _plant(k, u, items, nk, tile, scale, rise, 6.0, 3, placement, shift)
    big = MASKED_RISE / (scale * LOG2E * AMP) * (u[0] + u[1])
    keys = [-1] * items
    if mode == "causal":
        choice = [min(c, nk - 1) for c in (tile, tile + 1, tile - 1, tile, tile + 1, nk - 1)]
        for it in range(items):
            keys[it] = choice[it % len(choice)]
    else:
        assert mode == "after"
        for it in spiked:
            keys[it] = 0
    for it in range(items):
        if keys[it] >= 0:
            k[it, keys[it]] = noise * torch.randn(D, generator=torch.Generator().manual_seed(seed + 17 * it), dtype=torch.float64) + big
    return _f16(q), _f16(k), _f16(v), _f16(big), keys


def rel_tables(R, D, seed):
    """fp16-representable relative-position tables ek, ev [2R+1, D] (0.3 randn, as tests/test_gpu_relpos_long.py)."""
    g = torch.Generator().manual_seed(seed)
    ek = (0.3 * torch.randn(2 * R + 1, D, generator=g)).half().double()
    ev = (0.3 * torch.randn(2 * R + 1, D, generator=g)).half().double()
    return ek, ev


def rel_index(nq, nk, R, q_offset):
    return (torch.arange(nk)[None, :] - (torch.arange(nq)[:, None] + q_offset)).clamp(-R, R) + R          # [nq, nk]


def logits(q, k, scale, causal=False, rel=None):
    """Scaled logits [items, nq, nk] in float64, natural units; masked pairs are -inf."""
    q, k = q.double(), k.double()
    nq, nk = q.shape[1], k.shape[1]
    sim = torch.einsum("itd,isd->its", q, k)
    if rel is not None:
        ek, _, R, off = rel
        idx = rel_index(nq, nk, R, off)
        for t0 in range(0, nq, 64):                      # q_t . ek[idx[t, s]], a block of queries at a time (the table gather is [64, nk, D])
            sim[:, t0:t0 + 64] += torch.einsum("itd,tsd->its", q[:, t0:t0 + 64], ek.double()[idx[t0:t0 + 64]])
    sim = sim * scale
    if causal:
        sim = sim.masked_fill(torch.arange(nk)[None, :] > torch.arange(nq)[:, None], -math.inf)
    return sim


def softmax_attention_ref(q, k, v, scale, causal=False, rel=None):
    """softmax(q k^T scale) v in float64, written out.  causal: key s counts for query t only if s <= t.
    rel = (ek, ev, R, q_offset): the clamped relative-position terms, sim += q_t . ek[idx[t, s]] and out += sum_s p[t, s] ev[idx[t, s]] with
    idx[t, s] = clamp(s - (t + q_offset), -R, R) + R."""
    sim = logits(q, k, scale, causal, rel)
    p = torch.exp(sim - sim.max(dim=-1, keepdim=True).values)
    p = p / p.sum(dim=-1, keepdim=True)
    out = torch.einsum("its,isd->itd", p, v.double())
    if rel is not None:
        _, ev, R, off = rel
        idx = rel_index(q.shape[1], k.shape[1], R, off)
        for t0 in range(0, q.shape[1], 64):
            out[:, t0:t0 + 64] += torch.einsum("its,tsd->itd", p[:, t0:t0 + 64], ev.double()[idx[t0:t0 + 64]])
    return out


def stale_max_schedule(logits_log2, v, tile, qblock=32, rel=None, skip=None):
    """float64 emulation of the kernels' schedule on logits in log2 units [items, nq, nk] (-inf = masked): keys in tiles of `tile`, per query
    the running maximum advances only when the tile's maximum exceeds it by more than 8, then l, O (and w_lo / w_hi) are multiplied by
    alpha = exp2(m_run - m_tile); probabilities are rounded to fp16 before they meet V, as the MFMA operand is.
    rel = (ev, R, q_offset): the long-clip kernel (tile = qblock = 32) — a (query block, key tile) pair whose s - t' all clip to one table
      row adds its probability mass to w_hi (s - t' >= R) or w_lo (<= -R) instead of multiplying the table window; w_lo ev[0] + w_hi ev[2R]
      joins O at the end.
    skip = 'o' / 'w': the schedule WITHOUT the rescale of O / of w_lo and w_hi (the mutants the tests must catch).
    Returns dict(out, late, pairs_late, mixed, w_lo_hits, w_hi_hits, pairs): growth events on tiles after the first, (item, query) pairs with
    at least one, (item, block, tile) triples where some but not all of the block's queries grow, growth events that hit a non-zero w_lo /
    w_hi."""
    items, nq, nk = logits_log2.shape
    D = v.shape[-1]
    v = v.double()
    out = torch.zeros(items, nq, D, dtype=torch.float64)
    stats = dict(late=0, mixed=0, w_lo_hits=0, w_hi_hits=0, pairs=items * nq)
    grew = torch.zeros(items, nq, dtype=torch.bool)
    if rel is not None:
        ev, R, off = rel
        ev = ev.double()
        idx = rel_index(nq, nk, R, off)
    for t0 in range(0, nq, qblock):
        tt = slice(t0, min(t0 + qblock, nq))
        n = tt.stop - t0
        m = torch.full((items, n), -math.inf, dtype=torch.float64)
        l = torch.zeros(items, n, dtype=torch.float64)
        wl, wh = torch.zeros_like(l), torch.zeros_like(l)
        o = torch.zeros(items, n, D, dtype=torch.float64)
        for s0 in range(0, nk, tile):
            ss = slice(s0, min(s0 + tile, nk))
            edge = 0
            if rel is not None:
                dmin, dmax = s0 - (t0 + off + qblock - 1), s0 + tile - 1 - (t0 + off)
                edge = 1 if dmin >= R else (-1 if dmax <= -R else 0)
            sc = logits_log2[:, tt, ss]
            mt = sc.max(dim=-1).values
            grow = (mt - m) > GROW
            alpha = torch.where(grow, torch.exp2(m - mt), torch.ones_like(m))
            if s0 > 0:
                stats["late"] += int(grow.sum())
                grew[:, tt] |= grow
                stats["mixed"] += int((grow.any(dim=1) & ~grow.all(dim=1)).sum())
                stats["w_lo_hits"] += int((grow & (wl > 0)).sum())
                stats["w_hi_hits"] += int((grow & (wh > 0)).sum())
            l = l * alpha
            if skip != "w":
                wl, wh = wl * alpha, wh * alpha
            if skip != "o":
                o = o * alpha[..., None]
            m = torch.where(grow, mt, m)
            pr = torch.exp2(sc - m[..., None])
            ps = pr.sum(dim=-1)
            pr = pr.half().double()
            l = l + ps
            if edge > 0:
                wh = wh + ps
            if edge < 0:
                wl = wl + ps
            o = o + torch.einsum("its,isd->itd", pr, v[:, ss])
            if rel is not None and edge == 0:
                o = o + torch.einsum("its,tsd->itd", pr, ev[idx[tt, ss]])
        if rel is not None:
            o = o + wl[..., None] * ev[0] + wh[..., None] * ev[2 * R]
        out[:, tt] = o / l[..., None]
    stats["pairs_late"] = int(grew.sum())
    stats["out"] = out
    return stats


# ---- the case lists shared by the CPU and the GPU tests -------------------------------------------------------------------------------
# Tolerances are the ones the suite already applies to these kernels against an explicit reference on randn inputs.
TOL_HI, TOL_HILO = 2e-3, 1e-3


def _attn(id, layout, D, B, F, heads, nq, nk, tile, **kw):
    c = dict(id=id, layout=layout, D=D, B=B, F=F, heads=heads, nq=nq, nk=nk, tile=tile, causal=False, lo=False, variant="late",
             placement="cycle", shift=0, rise=9.5, low_every=3, attn2=False, waves=0, seed=1000 + 7 * D + nq + 3 * nk)
    c.update(kw)
    return c


# layouts (tests/test_gpu_attention_adversarial.py): 'self' = packed QKV rows [B, n, 3 inner], one item per (B, head) — the spatial and the
# causal form; 'temporal' = packed QKV rows [B, n, F pixels, 3 inner], one item per (B, pixel, head); 'cross' = Q rows [B, F, nq, inner]
# against K / V rows [B, nk, 8 + 2 inner] shared by the F frames (stride 0)
ATTN_CASES = []
for _D in (40, 64, 80, 160):                             # attn_kernel<4, D>: 5 and 16 tiles of 64 keys, the last one ragged
    for _hw in (300, 1000):
        _nt = -(-_hw // 64)
        ATTN_CASES.append(_attn(f"spatial-d{_D}-hw{_hw}", "self", _D, 2, 1, 2, _hw, _hw, 64, lo=(_D // 8 + _hw // 100) % 2 == 0,
                                shift=(_nt - 2) if _hw == 1000 else 0))
ATTN_CASES += [
    # attn_kernel<1, D> (nq <= 32, two 64-key tiles: 64 + 13 keys) and attn_kernel<1, D, 32> (nk <= 32: a single tile)
    _attn("small-d40-nq20-nk77", "cross", 40, 2, 3, 2, 20, 77, 64, placement="second"),
    _attn("small-d160-nq32-nk77", "cross", 160, 2, 2, 2, 32, 77, 64, placement="second", lo=True),
    _attn("small-d40-n20", "temporal", 40, 2, 5, 2, 20, 20, 32),
    _attn("small-d160-n32", "temporal", 160, 2, 3, 2, 32, 32, 32, lo=True),
    _attn("small-d40-nq20-nk24", "cross", 40, 2, 2, 2, 20, 24, 32),
    # text cross-attention: 77 keys = a 13-key second tile
    _attn("cross-d64-nq256", "cross", 64, 2, 2, 2, 256, 77, 64, placement="second"),
    _attn("cross-d80-nq256", "cross", 80, 2, 1, 2, 256, 77, 64, placement="second", lo=True),
    _attn("cross-d64-nq1024", "cross", 64, 2, 1, 2, 1024, 77, 64, placement="second", lo=True),
    _attn("cross-d80-nq1024", "cross", 80, 1, 2, 2, 1024, 77, 64, placement="second"),
]
for _L in (77, 129, 200):                                # causal (CLIP text towers): the spikes in the second tile, below most later queries
    # Lseq 77: only the 13 queries 64 .. 76 can see a key of the second tile at all (17 %), so every spike of that case is 10.5 log2 units
    ATTN_CASES.append(_attn(f"causal-L{_L}", "self", 64, 2, 1, 2, _L, _L, 64, causal=True, placement="second",
                            **(dict(rise=10.5, low_every=0) if _L == 77 else {})))
    ATTN_CASES.append(_attn(f"causal-L{_L}-masked", "self", 64, 3, 1, 2, _L, _L, 64, causal=True, placement="second", variant="masked",
                            **(dict(rise=10.5) if _L == 77 else {})))
ATTN_CASES += [
    # attn2_kernel (V transposed once, tiles by LDS-DMA): 8 waves, 4 waves, the default; also bitwise against attn_kernel
    _attn("attn2-w8-hw1024", "self", 64, 2, 1, 2, 1024, 1024, 64, attn2=True, waves=8, shift=14),
    _attn("attn2-w4-hw1000", "self", 64, 2, 1, 2, 1000, 1000, 64, attn2=True, waves=4, lo=True, shift=13),
    _attn("attn2-w0-hw2304", "self", 64, 2, 1, 2, 2304, 2304, 64, attn2=True, waves=0, shift=34),
    # a logit 40 log2 units up in the rows that follow an item's last key in memory
    _attn("spatial-d40-hw300-masked", "self", 40, 2, 1, 2, 300, 300, 64, variant="masked"),
    _attn("spatial-d160-hw1000-masked", "self", 160, 2, 1, 2, 1000, 1000, 64, variant="masked", lo=True, shift=14),
    _attn("small-d40-n20-masked", "temporal", 40, 2, 5, 2, 20, 20, 32, variant="masked"),
    _attn("cross-d64-nq256-masked", "cross", 64, 2, 2, 2, 256, 77, 64, placement="second", variant="masked"),
    _attn("attn2-w8-hw1000-masked", "self", 64, 2, 1, 2, 1000, 1000, 64, attn2=True, waves=8, variant="masked", shift=14),
]


def _rel(id, D, T, Tq, off, R, lo, **kw):
    c = dict(id=id, D=D, T=T, Tq=Tq, off=off, R=R, lo=lo, hw=5, b=2, heads=2, variant="late", seed=2000 + D + T + off, shift=0)
    c.update(kw)
    return c


# relpos_long_kernel (RELPOS_ATTN i[17] = 3): whole clips, T-sharded slices at the start / middle / end of the clip, the documented bound
# (T = 33: the second tile is one key; with the default seed the fp16 rounding of the sub-threshold probabilities alone leaves the float64
# emulation 1.02e-4 from the exact softmax, at the edge of the 1e-4 the CPU test asks of every case, so this case names its seed: 6.0e-5)
RELPOS_LONG_CASES = [_rel(f"long-d{D}-T{T}-R{R}", D, T, T, 0, R, n % 2 == 1, **(dict(seed=2077) if T == 33 else {}))
                     for n, (D, T, R) in enumerate([(40, 250, 16), (64, 100, 2), (80, 125, 16), (160, 48, 16), (40, 33, 2), (160, 64, 63)])]
RELPOS_LONG_CASES += [_rel(f"shard-d{D}-T{T}-q{off}+{Tq}-R{R}", D, T, Tq, off, R, n % 2 == 0)
                      for n, (D, T, Tq, off, R) in enumerate([(64, 250, 84, 166, 2), (40, 64, 20, 0, 16), (80, 100, 34, 33, 16)])]
RELPOS_LONG_CASES += [
    _rel("long-d40-T1024-R16", 40, 1024, 1024, 0, 16, False, hw=1, shift=29),
    _rel("long-d80-T125-R16-masked", 80, 125, 125, 0, 16, True, variant="masked"),
]

# relpos at <= 32 frames: every selector that applies, on the same inputs.  Selectors 0 (VALU kernel), 1 and 2 are single pass (range and masks
# only); forced 3 streams one 32-key tile.  Selector 1 needs R >= T - 1, selector 2 also T <= 16.
RELPOS_SHORT_CASES = [
    _rel("short-d40-T5", 40, 5, 5, 0, 16, False, sels=(0, 1, 2, 3)),
    _rel("short-d80-T16", 80, 16, 16, 0, 16, True, sels=(0, 1, 2, 3)),
    _rel("short-d160-T24", 160, 24, 24, 0, 24, False, sels=(0, 1, 3)),
    _rel("short-d64-T32", 64, 32, 32, 0, 31, True, sels=(0, 1, 3)),
    _rel("short-d40-T24-R4", 40, 24, 24, 0, 4, False, sels=(0, 3)),
    _rel("short-d80-T16-masked", 80, 16, 16, 0, 16, False, sels=(0, 1, 2, 3), variant="masked"),
]

# ---- the `lowered` family: one case per code path that a lowered program takes and no case above has (tests/record_paths.py is the key, ----
# ---- tests/test_record_paths_cpu.py the check; profiles/lowered_paths.txt names a deployed op for each).  Head dimension x kernel form x ----
# ---- one key tile / several x ragged keys x ragged queries x low-order output, at the smallest sizes of each class ----------------------
ATTN_CASES += [
    _attn("lowered-cross-d64-nq128-nk40", "cross", 64, 2, 1, 2, 128, 40, 64),                      # 4-wave kernel, whole query blocks, one ragged key tile
    _attn("lowered-self-d64-hw64", "self", 64, 2, 1, 2, 64, 64, 64),                               # ... half a query block, one whole key tile
    _attn("lowered-self-d40-hw64", "self", 40, 2, 1, 2, 64, 64, 64),
    _attn("lowered-self-d40-hw64-lo", "self", 40, 2, 1, 2, 64, 64, 64, lo=True),
    _attn("lowered-self-d160-hw64", "self", 160, 2, 1, 2, 64, 64, 64),
    _attn("lowered-cross-d40-nq64-nk9", "cross", 40, 2, 2, 2, 64, 9, 64),                          # VideoCrafter's 9-token context at the tiny size
    _attn("lowered-cross-d40-nq64-nk9-lo", "cross", 40, 2, 2, 2, 64, 9, 64, lo=True),
    _attn("lowered-self-d80-hw16", "self", 80, 2, 1, 2, 16, 16, 32),                               # one wave, the 32-key tile, both ragged
    _attn("lowered-self-d80-hw16-lo", "self", 80, 2, 1, 2, 16, 16, 32, lo=True),
    _attn("lowered-self-d160-hw16", "self", 160, 2, 1, 2, 16, 16, 32),
    _attn("lowered-cross-d64-nq20-nk77", "cross", 64, 2, 2, 2, 20, 77, 64, placement="second"),    # one wave, 64 + 13 keys
    _attn("lowered-cross-d160-nq16-nk77", "cross", 160, 2, 2, 2, 16, 77, 64, placement="second"),
    _attn("lowered-self-d64-hw192", "self", 64, 2, 1, 2, 192, 192, 64),                            # three whole key tiles, a ragged query block
    _attn("lowered-self-d40-hw256", "self", 40, 2, 1, 2, 256, 256, 64),                            # whole key tiles and whole query blocks
    _attn("lowered-self-d80-hw256", "self", 80, 2, 1, 2, 256, 256, 64),
]
RELPOS_LONG_CASES += [_rel("lowered-long-d160-T40-R16", 160, 40, 40, 0, 16, False)]               # a 40-frame clip: two key tiles, the clamp live
RELPOS_SHORT_CASES += [
    _rel("lowered-short-d40-T5-lo-relpos16", 40, 5, 5, 0, 16, True, sels=(2,)),
    _rel("lowered-short-d160-T16-relpos16", 160, 16, 16, 0, 16, False, sels=(2,)),
]
# T-sharded ranks: the VALU kernel (selector 0) on a slice of the queries at the start, in the middle and at the end of a clip of 5, 8 and
# 16 frames (TB = 1, 1, 2); the forced long-clip kernel on the same inputs as the second opinion
for _T, _Tq, _offs, _Ds in ((5, 2, (0, 2, 3), (40,)), (8, 3, (0, 3, 5), (80,)), (16, 4, (0, 6, 12), (40, 80, 160))):
    for _D in _Ds:
        RELPOS_SHORT_CASES += [_rel(f"lowered-shard-d{_D}-T{_T}-q{_o}+{_Tq}", _D, _T, _Tq, _o, 16, False, sels=(0, 3)) for _o in _offs]

# ---- the keys of the requestable lattice (tests/geometry_lattice.py; profiles/geometry_paths.txt names a witness program for each): other ----
# ---- latents and frame counts put every head dimension on every kernel form.  The size classes are the launcher's: attention.hip:1253-1255 ----
# ---- (launch_attn: nq <= 32 -> one wave, with the 32-key tile when the keys fit one; else 4 waves per 128 queries, 64-key tiles),      ----
# ---- attention.hip t2v_launch_attention (attn2_kernel<8>: 256 queries per workgroup) and, for nk_tiles, the key-tile loop that runs once or streams ----
ATTN_CASES += [
    # one wave, 64 + 13 keys (text cross-attention of a latent of at most 32 positions): ragged and whole query blocks
    _attn("lowered-cross-d80-nq16-nk77", "cross", 80, 2, 2, 2, 16, 77, 64, placement="second"),
    _attn("lowered-cross-d64-nq32-nk77", "cross", 64, 2, 2, 2, 32, 77, 64, placement="second"),
    _attn("lowered-cross-d80-nq32-nk77", "cross", 80, 2, 2, 2, 32, 77, 64, placement="second"),
    _attn("lowered-cross-d160-nq32-nk77", "cross", 160, 2, 2, 2, 32, 77, 64, placement="second"),
    # one wave, the 32-key tile, 32 queries and 32 keys: nothing ragged (a latent of 32 positions; 32 frames)
    _attn("lowered-temporal-d64-n32", "temporal", 64, 2, 3, 2, 32, 32, 32),
    _attn("lowered-temporal-d80-n32", "temporal", 80, 2, 3, 2, 32, 32, 32),
    _attn("lowered-temporal-d160-n32", "temporal", 160, 2, 3, 2, 32, 32, 32),
    # 4 waves: one key tile, ragged (48 keys) and whole (64), under a ragged query block; three whole key tiles under a ragged query block;
    # four whole key tiles under whole query blocks; 64 + 13 keys under a whole query block
    _attn("lowered-self-d80-hw48", "self", 80, 2, 1, 2, 48, 48, 64),
    _attn("lowered-self-d160-hw48", "self", 160, 2, 1, 2, 48, 48, 64),
    _attn("lowered-self-d80-hw64", "self", 80, 2, 1, 2, 64, 64, 64),
    _attn("lowered-self-d40-hw192", "self", 40, 2, 1, 2, 192, 192, 64),
    _attn("lowered-self-d80-hw192", "self", 80, 2, 1, 2, 192, 192, 64),
    _attn("lowered-self-d160-hw192", "self", 160, 2, 1, 2, 192, 192, 64),
    _attn("lowered-self-d160-hw256", "self", 160, 2, 1, 2, 256, 256, 64),
    _attn("lowered-cross-d160-nq128-nk77", "cross", 160, 2, 1, 2, 128, 77, 64, placement="second"),
    # attn2_kernel<8>: five whole key tiles, one whole 256-query block and a quarter of one (a 40 x 72 latent: 2880 = 11.25 blocks)
    _attn("lowered-attn2-w8-hw320", "self", 64, 2, 1, 2, 320, 320, 64, attn2=True, waves=8, shift=3),
]
# the VALU kernel's TB (attention.hip:1197, 1207-1211: seqattn_kernel<TB>, TB = ceil(T / 8) up to 4) at 17 .. 24 frames (TB = 3) and 25 .. 32
# (TB = 4), with the table index clamped (R < T - 1) and not; whole clips, then a T-sharded rank's queries at the start and inside the clip
RELPOS_SHORT_CASES += [
    _rel("lowered-short-d40-T17", 40, 17, 17, 0, 16, False, sels=(0, 3)),
    _rel("lowered-short-d80-T17", 80, 17, 17, 0, 16, False, sels=(0, 3)),
    _rel("lowered-short-d80-T18", 80, 18, 18, 0, 16, False, sels=(0, 3)),
    _rel("lowered-short-d160-T18", 160, 18, 18, 0, 16, False, sels=(0, 3)),
]
RELPOS_SHORT_CASES += [_rel(f"lowered-short-d{_D}-T25", _D, 25, 25, 0, 16, False, sels=(0, 3)) for _D in (40, 80, 160)]
RELPOS_SHORT_CASES += [_rel(f"lowered-shard-d{_D}-T24-q{_o}+3", _D, 24, 3, _o, 16, False, sels=(0, 3)) for _D in (40, 80, 160) for _o in (0, 3)]
# relpos_long_kernel on a T-sharded rank of a clip of two key tiles (40 frames): the queries at the start and at the end of the clip
RELPOS_LONG_CASES += [_rel(f"lowered-shard-d{_D}-T40-q{_o}+5", _D, 40, 5, _o, 16, False) for _D in (40, 80, 160) for _o in (0, 35)]


def attn_inputs(c):
    """Item tensors of an ATTN_CASES entry: q [B heads, F nq, D] for the 'cross' layout (the F frames of a sample share its keys) and
    [B F heads, nq, D] otherwise, k, v [.., nk, D]; items in (B, F, head) order.  Returns dict(q, k, v, spare_k, keys, scale)."""
    D, B, F, heads = c["D"], c["B"], c["F"], c["heads"]
    scale = D ** -0.5
    cross = c["layout"] == "cross"
    items = B * heads if cross else B * F * heads
    nq = c["nq"] * F if cross else c["nq"]
    per_b = items // B
    kw = dict(placement=c["placement"], shift=c["shift"], rise=c["rise"])
    if c["variant"] == "late":
        q, k, v = late_max_qkv(items, nq, c["nk"], D, c["tile"], scale, c["seed"], low_every=c["low_every"], **kw)
        return dict(q=q, k=k, v=v, spare_k=None, keys=[-1] * items, scale=scale)
    mode = "causal" if c["causal"] else "after"
    spiked = [it for it in range(items) if (it // per_b) % 2 == 1]      # the items of every second sample: key 0 follows the previous sample's last key
    q, k, v, spare, keys = masked_spike(items, nq, c["nk"], D, c["tile"], scale, c["seed"], mode, spiked, **kw)
    return dict(q=q, k=k, v=v, spare_k=spare, keys=keys, scale=scale)


def relpos_inputs(c):
    """Item tensors of a RELPOS_*_CASES entry, items in (b, pixel, head) order, and the tables: dict(q, k, v, ek, ev, spare_k, keys, scale)."""
    D, T, Tq, R = c["D"], c["T"], c["Tq"], c["R"]
    scale = D ** -0.5
    items = c["b"] * c["hw"] * c["heads"]
    per_b = items // c["b"]
    ek, ev = rel_tables(R, D, c["seed"] + 1)
    if c["variant"] == "late":
        q, k, v = late_max_qkv(items, Tq, T, D, 32, scale, c["seed"], shift=c["shift"])
        return dict(q=q, k=k, v=v, ek=ek, ev=ev, spare_k=None, keys=[-1] * items, scale=scale)
    spiked = [it for it in range(items) if (it // per_b) % 2 == 1]
    q, k, v, spare, keys = masked_spike(items, Tq, T, D, 32, scale, c["seed"], "after", spiked, shift=c["shift"])
    return dict(q=q, k=k, v=v, ek=ek, ev=ev, spare_k=spare, keys=keys, scale=scale)
