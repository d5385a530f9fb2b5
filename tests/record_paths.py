"""TEST INFRASTRUCTURE — the code path of an op record, as a key.  No test functions here: tests/test_record_paths_cpu.py keys every record
of every lowered program and every record of the adversarial case lists and demands that each lowered key has an adversarial case.

`path_keys(op)` -> the keys of a record, one per launch it makes (a split-K GEMM with a reduction launch makes two), each a tuple of
(field, value) pairs; `path_key(op)` -> their concatenation, or None for a kind that is out of scope.  A key holds every field of the record that
changes WHICH CODE RUNS: what selects a template instantiation or a kernel in a launcher, what a kernel branches on, and every size only
as the class the dispatch code distinguishes.  No pointers (only whether one is there), no plain sizes.  The authority is the dispatch
code; beside every field stands the place it was read from (file: function, line at the time of writing).  The device is the one
tools/program_digest.py FIXED pins: T2V_DEVICE_CUS = 256.

Out of scope (path_key returns None):
  MEMSET            hipMemsetAsync, no kernel of the project (executor.hip launch_op)
  ALLGATHER, HALO_EXCHANGE, STATS_HALO, ALLTOALL
                    collectives: they need peers and have no record fields that choose a kernel; their code paths depend on the
                    message size alone and have their own designed-input suite, tests/collective_inputs.py (share, trip and
                    transport classes; test_collective_inputs_cpu.py, test_gpu_collectives_adversarial.py)
  EMBED_ROWS, RESHARD_ROWS, RESAMPLE, TO_UINT8, EMPHASIS, FINGERPRINT, LORA_MERGE
                    their tests already demand bit equality at strided and ragged shapes, or they are never part of a plan
The plan-time feed-forward pair (executor.hip ff_pair -> t2v_launch_ff_fused) is a decision of the plan, not a field of a record: it keeps
its own suite (tests/ff_fused_inputs.py); its two records are keyed here as the two launches they are without the fusion."""
from __future__ import annotations

from sd_webui_text2video_amd import _lib as L

DEVICE_CUS = 256          # tools/program_digest.py FIXED["T2V_DEVICE_CUS"]
GNC_THREADS = 512         # norm.hip:410
_COLLECTIVE = "collective: tests/collective_inputs.py (designed sizes per message share, run by tests/test_gpu_collectives_adversarial.py)"
OUT_OF_SCOPE = {L.OP_MEMSET: "hipMemsetAsync", L.OP_ALLGATHER: _COLLECTIVE, L.OP_HALO_EXCHANGE: _COLLECTIVE, L.OP_STATS_HALO: _COLLECTIVE,
                L.OP_ALLTOALL: _COLLECTIVE, L.OP_EMBED_ROWS: "bit-exact tests", L.OP_RESHARD_ROWS: "bit-exact tests", L.OP_RESAMPLE: "bit-exact tests",
                L.OP_TO_UINT8: "bit-exact tests", L.OP_EMPHASIS: "bit-exact tests", L.OP_FINGERPRINT: "never part of a plan",
                L.OP_LORA_MERGE: "never part of a plan"}
KIND_NAMES = {L.OP_GEMM: "GEMM", L.OP_GROUPNORM: "GROUPNORM", L.OP_LAYERNORM: "LAYERNORM", L.OP_ATTENTION: "ATTENTION", L.OP_RELPOS_ATTN: "RELPOS_ATTN",
              L.OP_NCTHW_TO_CL: "NCTHW_TO_CL", L.OP_CL_TO_NCTHW: "CL_TO_NCTHW", L.OP_TIME_EMBED: "TIME_EMBED", L.OP_COPY2D: "COPY2D",
              L.OP_SOFTMAX: "SOFTMAX", L.OP_DDIM_STEP: "DDIM_STEP", L.OP_LINCOMB: "LINCOMB", L.OP_DEPTH_TOKENS: "DEPTH_TOKENS", L.OP_AVGPOOL2: "AVGPOOL2"}


def _has(ref) -> int:
    return int(ref.space != "null")


def coop_chunking(rows, n_inst, cv, ncu, max_chunk, kr_list):
    """norm.hip:629 coop_chunking -> (kr, nchunk): the first kr whose grid is at most one workgroup per CU; (0, 0): none."""
    for kr in kr_list:
        rc = (GNC_THREADS // cv) * kr
        nchunk = -(-rows // rc)
        if n_inst * nchunk <= ncu and nchunk <= max_chunk:
            return kr, nchunk
    return 0, 0


def _split_of(I, K):
    """t2v_kernels.h:233 t2v_normalize_splitk: clamped to the k-tiles, no empty splits."""
    kt = -(-K // L.GEMM_BK)
    s = max(1, min(I[19], kt))
    per = -(-kt // s)
    return -(-kt // per)


def gemm_keys(op):
    """The keys of a GEMM record, one per launch.  Without split-K, or with the fold in the GEMM's last-arriving workgroups (tickets), the
    record is one launch.  With a reduction launch it is two, and they share no code: the GEMM kernel stores its slab and skips every
    epilogue (t2v_kernels.h:462 `if (p.splitk > 1)` in t2v_epilogue_rows, gemm2.hip:491 t2v_store_splitk_slab for GEGLU), and the reduction
    — splitk_reduce_kernel (gemm.hip:309) or splitk_gn_kernel (norm.hip:538) — reads slabs whatever tile and gather wrote them.  So the
    first key holds the tile, the gather and the raggedness with the epilogue fields blank, the second the epilogue fields alone."""
    I, P = op.i, op.p
    M, N, K, gather, epi = I[0], I[1], I[2], I[7], I[16]
    plain = gather == L.GATHER_PLAIN
    tile = I[22]
    geo = L.GEMM_TILES.get(tile)
    # executor.hip launch_op: a gemm2 tile runs gemm2.hip only for K % 64 == 0 and not the C8 stem; everything else is gemm.hip's kernel
    gemm2 = geo is not None and geo.has(L.TILE_GEMM2) and (epi == L.EPI_TATTN or (gather != L.GATHER_CONV3X3_C8 and K % 64 == 0))
    kernel = tile if gemm2 else 0
    bm = L.GEMM_TILES[kernel].bm
    bn = L.GEMM_TILES[kernel].bn if gemm2 else L.tile0_bn(N)          # gemm.hip:422 t2v_launch_gemm: 128x64 when t2v_tile0_narrow(N)
    ln = I[8] if plain and epi != L.EPI_TATTN and I[8] in (1, 2) else 0          # executor.hip gemm_decode: the LayerNorm forms
    split = 1 if epi in (L.EPI_TATTN, L.EPI_XATTN, L.EPI_STATS) or ln else _split_of(I, K)
    gn = epi == L.EPI_GN
    fold = "-"
    if split > 1:
        # executor.hip gemm_decode / gemm_params: p[7] is the tickets of a split-K record; t2v_kernels.h:239: kept only for the plain epilogue, <= T2V_SYNC_INTS tiles, no GroupNorm behind it;
        # gemm.hip:431 / gemm2.hip:595: otherwise the reduction launch, with the GroupNorm in it when gn_out is set
        tiles = -(-M // bm) * -(-N // bn)
        fold = "tickets" if (_has(P[7]) and epi == L.EPI_NONE and tiles <= L.SYNC_INTS) else "reduce+gn" if gn else "reduce"
    slab = fold.startswith("reduce")
    wrap = "i30" if I[30] > 0 else "i12" if (plain and epi != L.EPI_TATTN and I[12] > 0) else "-"      # executor.hip gemm_decode res_wrap
    epilogue = [
        ("epi", epi if not gn else L.EPI_NONE),                         # executor.hip gemm_params p.epi; gemm.hip:418, gemm2.hip:538
        ("out", I[17]),                                                 # executor.hip gemm_params out_f32; gemm.hip:68, t2v_kernels.h:954, norm.hip:562
        ("act", I[18]),                                                 # gemm.hip:51-53; t2v_kernels.h:471-472
        ("bias", _has(P[2])),                                           # gemm.hip:38; t2v_kernels.h:455; norm.hip:548
        ("bias_m", int(I[20] != 0) if _has(P[2]) else 0),               # t2v_kernels.h:469
        ("rowbias", _has(P[3]) if not ln else 0),                       # gemm.hip:47; norm.hip:559; executor.hip gemm_decode (p[3] is gamma | beta under the LayerNorm forms)
        ("res", _has(P[4])),                                            # gemm.hip:56; t2v_kernels.h:556; norm.hip:560
        ("res_wrap", wrap if _has(P[4]) else "-"),                      # gemm.hip:57; t2v_kernels.h:429
        ("out_lo", int(plain and I[11] == 1)),                          # executor.hip gemm_decode out_lo; gemm.hip:68
    ]
    main = [
        ("kind", "GEMM"),
        ("tile", kernel),                                               # executor.hip launch_op; gemm2.hip:787 t2v_launch_gemm2 switch
        ("tile0_bn", bn if kernel == 0 else 0),                         # gemm.hip:422-428
        ("gather", gather),                                             # gemm.hip:397 launch_tile switch; gemm2.hip:549 launch_cfg switch
        ("stride", I[11] if gather in (L.GATHER_CONV3X3, L.GATHER_CONV3X3_C8) else 0),      # executor.hip gemm_decode stride; gemm.hip:182 / gemm2.hip:127 tap arithmetic
        ("up", int(I[12] != 0) if gather == L.GATHER_CONV3X3 else 0),   # gemm2.hip:582 G_CONV_UP instantiation
        ("i23", int(I[23] != 0)),                                       # executor.hip gemm_decode halo; gemm.hip:147 / 182, gemm2.hip:127 / 141
        ("i13", int(plain and epi != L.EPI_TATTN and I[13] > 0)),       # executor.hip gemm_decode a_wrap; gemm.hip:137, gemm2.hip:116
        ("ln", ln),                                                     # executor.hip gemm_params (GEMM_LN_ROW / GEMM_LN_CROSS); gemm2.hip:564-575 XE_LN / XE_LNX
        ("fold", "slab" if slab else fold),                             # gemm.hip:346 / gemm2.hip:525 grid.y; t2v_kernels.h:233, 462
        ("k_tail", int(K % 64 != 0)),                                   # executor.hip launch_op; gemm.hip K tail of the last k-tile
        ("m_ragged", int(M % bm != 0)),                                 # the m < p.M guards of every tail (t2v_kernels.h:461, 952)
        ("n_ragged", int(N % bn != 0)),                                 # the n < p.N guards (t2v_kernels.h:453, 948)
    ]
    if epi == L.EPI_XATTN:
        # executor.hip gemm_decode xa_lc / xa_lcp: keys per sample and their padded count — t2v_epilogue_xattn walks key blocks of 32 up to xa_lcp
        main += [("xa_ragged", int(I[25] % 32 != 0)), ("xa_blocks", min(-(-I[26] // 32), 4))]
    if ln == 2:
        cap = min(L.GEMM_TILES[kernel].per_cu * DEVICE_CUS, L.GN_PART_BYTES // (bm * 16))        # program.py:559
        main += [("lnx_chunked", int(-(-M // bm) * -(-N // bn) > cap))]
    norm = []
    if gn:
        rows = I[24]
        norm = [("gn_silu", int(I[26] != 0)),                          # executor.hip gemm_params gn_silu; norm.hip:794 dispatch_bool
                ("gn_lo", int(I[27] != 0)),                            # executor.hip gemm_params gn_lo
                ("i29", int(I[29] != 0))]                              # executor.hip gemm_params gn_store_out; t2v_kernels.h:941; norm.hip:561
    if slab:
        second = [("kind", "GEMM.reduce+gn" if gn else "GEMM.reduce")] + epilogue + norm
        if gn:
            # norm.hip:788 t2v_launch_splitk_reduce_gn: KR of splitk_gn_kernel<SILU, KR>
            second += [("kr", coop_chunking(I[24], M // I[24], N // 8, DEVICE_CUS, 1 << 30, (1, 2, 4, 8, 12, 16, 20))[0])]
        return [tuple(main), tuple(second)]
    if gn:
        # t2v_kernels.h:912-922, 966: a tile meets one instance (whole), two (straddle: slot 1 is live) or — half a tile — two whole ones
        norm += [("gn_seam", "half" if 2 * rows == bm else "whole" if rows % bm == 0 else "straddle")]
        # gemm.hip:361 / gemm2.hip:519 t2v_launch_coresident (t2v_kernels.h:214): more tiles than the device holds -> row chunks.  The capacity
        # is the occupancy API's on the device; the lowering's own bound (program.py:669 per_cu x CUs, the record region) stands in for it here
        cap = min(L.GEMM_TILES[kernel].per_cu * DEVICE_CUS, L.GN_PART_BYTES // (2 * L.GN_PIECES * 16))
        norm += [("gn_chunked", int(-(-M // bm) * -(-N // bn) > cap))]
        epilogue[0] = ("epi", L.EPI_GN)
    return [tuple(main + epilogue + norm)]


def groupnorm_key(op):
    I, P = op.i, op.p
    n_inst, rows, C, groups, phase = I[0], I[1], I[2], I[4], I[8]
    cv = C // 8
    rpb = I[11] if I[11] > 0 else L.GN_ROWS_PER_BLOCK                  # norm.hip:873
    nblk = -(-rows // rpb)
    fused = int(I[12] != 0)                                             # norm.hip:902, 925 gn_fused_kernel
    # norm.hip:912-913: the cooperative kernel runs when asked for (i[15], p[5]) and coop_chunking finds a grid of at most one workgroup per CU
    kr = 0
    if I[15] != 0 and _has(P[5]) and phase == 0 and not fused and groups <= 32 and cv <= GNC_THREADS:
        kr, nchunk = coop_chunking(rows, n_inst, cv, DEVICE_CUS, nblk, (4, 8, 12, 16, 20))
    records = int(kr != 0 and _has(P[7]) and n_inst * nchunk * groups * 16 <= I[18])          # norm.hip:920
    strips = int(_has(P[6]) and phase in (1, 3))                       # norm.hip:877-880
    launch = "coop" if kr else "fused" if fused else {0: "stats+finalize+apply", 1: "stats+fold", 2: "apply", 3: "strips+apply"}[phase]
    if strips and phase == 1:
        launch = "strips-fold"
    return (
        ("kind", "GROUPNORM"),
        ("in", I[5]),                                                   # norm.hip:965 run(float / f16)
        ("silu", int(I[6] != 0)),                                       # norm.hip:926 / 959 dispatch_bool
        ("phase", phase),                                               # norm.hip:939-947
        ("launch", launch),
        ("i12", fused),
        ("i15", int(I[15] != 0)),
        ("kr", kr),                                                     # norm.hip:642 dispatch_kr: gn_coop_kernel<T, SILU, KR>
        ("records", records),                                           # norm.hip:650 tagged records or the grid barrier
        ("lo", int(I[16] != 0)),                                        # norm.hip:903 lo_off
        ("cast", _has(P[8])),                                           # norm.hip:905 GnCast
        ("cast_lo", int(_has(P[8]) and I[20] != 0)),
        ("halo", (int(I[21] != 0), int(I[22] != 0)) if phase == 2 else (0, 0)),          # norm.hip:953
        ("nparts", int((I[9] if I[9] > 0 else 1) > 1)),                 # norm.hip:872, 946
        ("strips_wide", int(strips and (rows // 32) * (C // groups) > 1024)),            # norm.hip:933
        ("cols_loop", int(cv > 256)),                                   # norm.hip:895 R = 1: gn_stats_kernel's column loop
        ("one_block", int(nblk == 1) if launch.startswith("stats") else 0),              # norm.hip:893 g1
    )


def layernorm_key(op):
    M, C = op.i[0], op.i[1]
    maxv = 2 if C <= 512 else 3 if C <= 768 else 5 if C <= 1280 else 8          # norm.hip:983-986
    cap = op.i[4] if op.i[4] > 0 else 8 * 256                           # norm.hip:980
    return (("kind", "LAYERNORM"), ("maxv", maxv), ("grid_stride", int(maxv <= 3 and -(-M // 4) > cap)), ("m_ragged", int(M % 4 != 0)))


def attention_key(op):
    I, P = op.i, op.p
    nq, nk = I[0], I[1]
    alt = I[19] != 0                                                    # attention.hip t2v_attention_classify: T2V_ATTN_SECOND_ROLE
    nkmax = max(nk, I[20]) if alt else nk
    attn2 = _has(P[6])                                                  # attention.hip t2v_attention_classify: T2V_ATTN_VT
    if attn2:
        kernel = "attn2<4>" if I[18] == 4 else "attn2<8>"              # attention.hip t2v_launch_attention (vt_waves)
    else:
        kernel = "attn<1,32>" if nq <= 32 and nkmax <= 32 else "attn<1,64>" if nq <= 32 else "attn<4,64>"          # attention.hip launch_attn
    tile = 32 if kernel == "attn<1,32>" else 64
    return (
        ("kind", "ATTENTION"),
        ("head_dim", I[14] if I[14] > 0 else 64),                       # attention.hip t2v_attention_classify head_dim; t2v_launch_attention
        ("causal", int(I[15] != 0)),                                    # attention.hip t2v_launch_attention p.causal
        ("lo", int(I[16] != 0)),                                        # attention.hip t2v_launch_attention p.lo_off
        ("kernel", kernel),
        ("second_role", int(alt)),
        ("nk_tiles", min(-(-nkmax // tile), 2)),                       # one key tile, or the streaming loop
        ("nk_ragged", int(nk % tile != 0)),
        ("nk2_ragged", int(alt and I[20] % tile != 0)),
        ("nq_ragged", int(nq % (32 if kernel.startswith("attn<1") else 256 if kernel == "attn2<8>" else 128) != 0)),
    )


def relpos_key(op):
    I, P = op.i, op.p
    Tq, T, D, R, off, sel = I[0], I[1], (I[14] if I[14] > 0 else 64), I[15], I[16], I[17]
    # attention.hip:1132-1196 launch_seqattn: which kernel the selector really reaches
    if sel == 3:
        kernel = "long"
    elif sel == 2 and _has(P[6]) and _has(P[7]) and Tq == T and off == 0 and T <= 16 and R >= T - 1 and D in (40, 64, 80, 160):
        kernel = "relpos16"
    elif sel == 1 and Tq == T and off == 0 and R >= T - 1 and R <= 31 and D in (40, 64, 80, 160):
        kernel = "mfma"
    else:
        kernel = "valu"
    return (
        ("kind", "RELPOS_ATTN"),
        ("kernel", kernel),
        ("head_dim", D),                                                # attention.hip:1139 / 1154 / 1169 switch; the VALU kernel takes any D % 8 == 0
        ("offset", int(off > 0)),                                       # attention.hip:1125 q_off
        ("nq_lt_nk", int(Tq < T)),
        ("lo", int(I[18] != 0)),                                        # attention.hip:1131
        ("tb", min((T + 7) // 8, 4) if kernel == "valu" else 0),       # attention.hip:1181, 1191 seqattn_kernel<TB, REL>
        ("clipped", int(R < T - 1)),                                    # the clamp of the table index is live
        ("tiles", min(-(-T // 32), 2) if kernel == "long" else 0),     # relpos_long_kernel: one key tile or the streaming loop
    )


def elementwise_key(op):
    I, P, k = op.i, op.p, op.kind
    name = ("kind", KIND_NAMES[k])
    if k == L.OP_NCTHW_TO_CL:          # elementwise.hip:1164-1175
        return (name, ("in", I[5]), ("bsrc", int(0 < I[6] < I[0])), ("second", _has(P[2])), ("lo", int(I[7] != 0 and I[4] >= 2 * I[1])))
    if k == L.OP_CL_TO_NCTHW:          # elementwise.hip:1177-1186
        return (name, ("out", I[5]))
    if k == L.OP_TIME_EMBED:           # elementwise.hip:1298-1304: one kernel
        return (name,)
    if k == L.OP_COPY2D:               # elementwise.hip:1306-1321
        return (name, ("src", I[4]), ("dst", I[5]), ("act", I[6]), ("second", int(_has(P[2]) and I[4] == L.F32 and I[5] == L.F16)))
    if k == L.OP_SOFTMAX:              # attention.hip t2v_launch_softmax: one kernel; the column loop runs more than once past 256 columns
        return (name, ("cols_gt_256", int(I[1] > 256)))
    if k == L.OP_DDIM_STEP:            # elementwise.hip:1368-1485
        return (name, ("eps", I[3]), ("x", I[4]), ("mode", I[5]), ("guided", int(I[2] != 0)), ("cps", int(0 < I[6] < I[0])), ("blend", int(I[7] != 0)),
                ("i8", I[8]), ("i9", int(I[9] != 0)))
    if k == L.OP_LINCOMB:              # elementwise.hip:1487-1498
        return (name, ("terms", I[1]), ("out", I[2]), ("f32_terms", tuple(int(I[3 + t] == L.F32) for t in range(I[1]))))
    if k == L.OP_DEPTH_TOKENS:         # elementwise.hip:1254-1265
        return (name, ("in", I[3]), ("norm", int(I[4] != 0)))
    assert k == L.OP_AVGPOOL2          # elementwise.hip:1267-1273: one kernel, either output optional
    return (name, ("f32_out", _has(P[1])), ("f16_out", _has(P[2])))


_KEYERS = {L.OP_GROUPNORM: groupnorm_key, L.OP_LAYERNORM: layernorm_key, L.OP_ATTENTION: attention_key, L.OP_RELPOS_ATTN: relpos_key}
for _k in (L.OP_NCTHW_TO_CL, L.OP_CL_TO_NCTHW, L.OP_TIME_EMBED, L.OP_COPY2D, L.OP_SOFTMAX, L.OP_DDIM_STEP, L.OP_LINCOMB, L.OP_DEPTH_TOKENS, L.OP_AVGPOOL2):
    _KEYERS[_k] = elementwise_key


def path_keys(op):
    """The keys of a record, one per launch it makes (a split-K GEMM with a reduction launch: two); [] for a kind that is out of scope."""
    if op.kind in OUT_OF_SCOPE:
        return []
    return gemm_keys(op) if op.kind == L.OP_GEMM else [_KEYERS[op.kind](op)]


def path_key(op):
    """The key of a record: the tuple of its launch keys' fields (None for a kind that is out of scope; OUT_OF_SCOPE says why)."""
    ks = path_keys(op)
    return tuple(f for k in ks for f in k) if ks else None


def kind_of(key):
    return key[0][1]


def show(key):
    return " ".join(f"{n}={v}" for n, v in key[1:])
