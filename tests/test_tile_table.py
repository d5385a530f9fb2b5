"""CPU: the two GEMM tile tables agree — GEMM_TILES (_lib.py) and T2V_TILES (csrc/t2v_kernels.h), the latter through the library's
validator, which reads it.  t2v_plan_create validates every record before any HIP call (tests/test_abi.py relies on the same): for each
fused epilogue the smallest record validation accepts, then ONLY i[22] varied over 0 .. 15 — accepted exactly on the ids for which
GEMM_TILES declares the feature, ids without an entry refused as unknown."""
import ctypes

import pytest

from sd_webui_text2video_amd import _lib as L

PTR = 0x1000                       # any non-null, non-slot value: nothing is dereferenced
IDS = range(16)


def _record(i, p, f=None):
    base_i = {3: i[2], 4: i[2], 5: i[1], 7: L.GATHER_PLAIN, 16: L.EPI_NONE, 17: L.F16, 19: 1}       # lda = ldw = K, ldc = N
    base_i.update(i)
    return dict(i=base_i, p={0: PTR, 1: PTR, 5: PTR, **p}, f=f or {})


GN_ROWS, GN_N, GN_GROUPS = 384, 640, 32
# feature -> [(record, the ids GEMM_TILES says accept it)]
RECORDS = {
    "plain": [(_record({0: 256, 1: 320, 2: 64}, {}), {t for t, g in L.GEMM_TILES.items() if not g.has(L.TILE_TATTN_ONLY)})],
    "gn": [(_record({0: GN_ROWS, 1: GN_N, 2: 64, 16: L.EPI_GN, 17: L.F32, 24: GN_ROWS, 25: GN_N, 28: GN_GROUPS},
                    {8: PTR, 9: PTR, 10: PTR, 11: PTR}, {2: 1e-5}),
            {t for t, g in L.GEMM_TILES.items() if g.fuses(L.TILE_GN, GN_N)})],
    "lnx": [(_record({0: 256, 1: 640, 2: 64, 8: 2, 9: 640, 17: L.F32}, {3: PTR, 7: PTR, 10: PTR, 11: PTR}, {0: 1e-5}),
             {t for t, g in L.GEMM_TILES.items() if g.fuses(L.TILE_LNX, 640)})],
    "ln": [(_record({0: 256, 1: 320, 2: 64, 8: 1, 9: 320, 17: L.F32}, {3: PTR, 7: PTR}, {0: 1e-5}),
            {t for t, g in L.GEMM_TILES.items() if g.fuses(L.TILE_LN, 320)})],
    # two base records: N = 320 for the whole-row tiles, N a multiple of 128 for the others
    "xattn": [(_record({0: 256, 1: n, 2: 64, 15: 256, 16: L.EPI_XATTN, 24: n, 25: 77, 26: 96}, {8: PTR, 9: PTR}, {1: 0.125}),
               {t for t, g in L.GEMM_TILES.items() if g.fuses(L.TILE_XATTN, n)}) for n in (320, 256)],
    "tattn": [(_record({0: 2 * 8 * 192, 1: 5 * 192, 2: 320, 5: 320, 8: 24, 9: 64, 10: 8, 16: L.EPI_TATTN}, {}, {1: 0.125}),
               {t for t, g in L.GEMM_TILES.items() if g.has(L.TILE_TATTN_ONLY)})],
}
DECLARED = {"plain": None, "gn": L.TILE_GN, "lnx": L.TILE_LNX, "ln": L.TILE_LN, "xattn": L.TILE_XATTN, "tattn": L.TILE_TATTN_ONLY}


def _validate(lib, rec, tile):
    op = (L.T2VOp * 1)()
    op[0].kind = L.OP_GEMM
    for k, v in rec["i"].items():
        op[0].i[k] = v
    for k, v in rec["f"].items():
        op[0].f[k] = v
    for k, v in rec["p"].items():
        op[0].p[k] = v
    op[0].i[22] = tile
    h = ctypes.c_void_p()
    rc = lib.t2v_plan_create(op, 1, ctypes.byref(h))
    msg = lib.t2v_last_error() if rc != 0 else b""
    if rc == 0:
        lib.t2v_plan_destroy(h)
    return rc, msg


def test_the_groupnorm_record_fits_every_declared_tile():
    """The base record must not be refused for its rows or groups on a tile that has the epilogue: then a missing table entry on either
    side would hide behind another refusal."""
    cpg = GN_N // GN_GROUPS
    tiles = [g for g in L.GEMM_TILES.values() if g.has(L.TILE_GN)]
    assert tiles
    for g in tiles:
        assert g.fuses(L.TILE_GN, GN_N)
        assert GN_ROWS % 32 == 0 and GN_ROWS >= g.bm
        assert cpg <= g.bn and (g.bn + cpg - 1) // cpg + 1 <= L.GN_PIECES


@pytest.mark.parametrize("feature", list(RECORDS))
def test_validator_accepts_a_feature_exactly_on_the_declared_tiles(built_lib, feature):
    accepted = set()
    for rec, expect in RECORDS[feature]:
        got = set()
        for tile in IDS:
            rc, msg = _validate(built_lib, rec, tile)
            if rc == 0:
                got.add(tile)
            else:
                assert rc == -1, (feature, tile, rc, msg)
                if tile not in L.GEMM_TILES:
                    assert b"unknown tile id" in msg, (feature, tile, msg)
        assert got, (feature, rec["i"][1], "the base record is accepted nowhere")
        assert got == expect, (feature, rec["i"][1], sorted(got), sorted(expect))
        accepted |= got
    # not vacuous: some id accepts, some id WITH an entry refuses, and together the records reach every tile that declares the feature
    assert accepted and set(L.GEMM_TILES) - accepted, (feature, sorted(accepted))
    if DECLARED[feature] is not None:
        assert accepted == {t for t, g in L.GEMM_TILES.items() if g.has(DECLARED[feature])}, (feature, sorted(accepted))


def test_table_ids_and_geometry():
    assert sorted(L.GEMM_TILES) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12]
    for t, g in L.GEMM_TILES.items():
        assert g.bm % 32 == 0 and g.bn % 32 == 0 and g.waves in (4, 8, 12) and g.per_cu in (1, 2), (t, g)
        assert g.has(L.TILE_GEMM2) == (t != 0)
