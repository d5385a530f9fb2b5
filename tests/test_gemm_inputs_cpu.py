"""CPU: the adversarial GEMM inputs of tests/gemm_inputs.py do what tests/test_gpu_gemm_adversarial.py needs them to do, and every case's
program is right in layout, references and fencing before it meets a GPU.

1. Mutations.  Each is applied in float64 to a correct result on the designed inputs and judged by the GPU file's own rule
   (`gemm_inputs.bound_of`: per row segment).  The worst segment must land outside its tolerance by at least a factor of 4; the factor is
   printed, with the whole-tensor rel-L2 the rest of the suite would have seen (2e-5 for fp32, 1e-3 for fp16 outputs) and whether that
   would have passed:
     a 1 % leak of the neighbouring row into the smallest-scale row; the last 8 k-elements dropped in the last row; one k-tile dropped in
     one split and one counted twice; the residual wrap ignored; the row-bias batch index off by one at a seam row; a bias along M applied
     along N; convolution padding replaced by the wrapped neighbouring pixel; the temporal first-frame padding replaced by the previous
     clip's last frame; one column quad of an fp32 output rounded through fp16; out_lo missing; a strip that counts a dead row.
2. Every case's program runs through the interpreter ALONE (interp_adapter.AdapterInterp: fp32 accumulate) and `gemm_inputs.verify` applies
   the GPU file's own checks: windows finite, every fence element still NaN, per-segment errors within the GPU tolerances.
3. Every tile id, both gemm.hip widths, every gather, every epilogue feature and both split-K folds occur in CASES."""
import pytest
import torch
import torch.nn.functional as F

import gemm_inputs as G
from interp_adapter import AdapterInterp

_BY_ID = {c["id"]: c for c in G.CASES}
_built = {}


def _b(cid):
    if cid not in _built:
        _built[cid] = G.build(_BY_ID[cid])
    return _built[cid]


def _out(cid, name):
    return next(o for o in _b(cid).outs if o["name"] == name)


def _judge(what, cid, o, mutated, lo_missing=False):
    """The factor by which the worst segment of `mutated` misses the GPU file's tolerance (>= 4), and what one rel-L2 over the tensor says."""
    got = mutated if (o["rule"] == "f32" and not lo_missing) else mutated.half()       # fp16 outputs are stored rounded
    assert float((G.seg_err(o["ref"] if o["rule"] == "f32" else o["ref"].half(), o["ref"]) / G.bound_of(o)).max()) < 1.0, "the unmutated result must pass"
    factor = float((G.seg_err(got, o["ref"]) / G.bound_of(o)).max())
    whole, suite = G.rel_l2(got, o["ref"]), (G.TOL_F32 if o["run"].out_dt == "f32" else G.TOL_F16)
    print(f"MUTATION {what} [{cid} / {o['name']}]: worst segment / tolerance = {factor:.1f}; whole-tensor rel-L2 {whole:.2e} "
          f"{'PASSES' if whole < suite else 'fails'} the suite's {suite:g}")
    assert factor >= 4.0, (what, cid, o["name"], factor)
    return whole < suite


def _mutants():
    """(what, case id, output name, function of the expectation -> mutated float64 result[, lo_missing])."""
    def leak(o):
        r = G.row_scale(o["ref"].shape[0])
        s = int(torch.argmin(r[1:-1])) + 1
        y = o["ref"].clone()
        y[s] += 0.01 * o["ref"][s - 1]
        return y

    def drop_k_tail(o):
        run = o["run"]
        acc = o["acc"].clone()
        acc[-1] = run.X[run.M - 1, :run.K - 8] @ run.W[:, :run.K - 8].t()
        return G.epilogue(acc, run.e)

    def split_seam(o):
        run = o["run"]
        per = -(-(-(-run.K // 64)) // run.split)                                 # k-tiles per split: tile per - 1 ends split 0, tile per starts split 1
        part = lambda kt: run.X[:run.M, 64 * kt:64 * kt + 64] @ run.W[:, 64 * kt:64 * kt + 64].t()
        return G.epilogue(o["acc"] - part(per - 1) + part(per), run.e)

    def wrap_ignored(o):
        run, e = o["run"], dict(o["run"].e)
        rows = run.M - e["res_wrap"]
        beyond = G.row_scale(run.M)[e["res_wrap"]:, None] * G.col_scale(e["res"].shape[1]) * torch.randn(rows, e["res"].shape[1], generator=G._gen(5), dtype=torch.float64)
        e["res"], e["res_wrap"] = torch.cat([e["res"], beyond]), 0              # rows m >= wrap read whatever lies behind the residual
        return G.epilogue(o["acc"], e)

    def rowbias_seam(o):
        run, e = o["run"], dict(o["run"].e)
        e["rowbias"] = e["rowbias"].roll(1, 0)
        y = o["ref"].clone()
        y[e["rpb"]] = G.epilogue(o["acc"], e)[e["rpb"]]                          # the first row of batch 1 takes batch 0's row bias
        return y

    def bias_m_as_n(o):
        e = dict(o["run"].e)
        e["bias"], e["bias_m"] = e["bias"][torch.arange(o["run"].N) % o["run"].M], False
        return G.epilogue(o["acc"], e)

    def conv_wrapped_pixel(o):
        run = o["run"]
        B, H, Wd = run.geo["image"]
        x = run.X.view(B, H * Wd, -1)
        flat = torch.cat([x[:, -1:], x, x[:, :1]], dim=1)                        # pixel (y, -1) IS the linear neighbour (y - 1, W - 1), (y, W) is (y + 1, 0)
        xp = torch.zeros(B, H + 2, Wd + 2, x.shape[2], dtype=torch.float64)
        xp[:, 1:-1, 1:-1] = x.view(B, H, Wd, -1)
        y = torch.arange(H)
        xp[:, 1:-1, 0] = flat[:, y * Wd]                                          # flat index of (y, -1) is y W - 1, + 1 for the front pad
        xp[:, 1:-1, -1] = flat[:, (y + 1) * Wd + 1]
        acc = F.conv2d(xp.permute(0, 3, 1, 2), run.W).permute(0, 2, 3, 1).reshape(-1, run.N)
        return G.epilogue(acc, run.e)

    def tconv_previous_clip(o):
        run = o["run"]
        B, Fr, HW = run.geo["clip"]
        x = run.X.view(B, Fr, HW, -1)
        xp = F.pad(x, (0, 0, 0, 0, 1, 1))
        xp[1:, 0] = x[:-1, -1]                                                   # frame -1 of clip b is the last frame of clip b - 1
        acc = F.conv3d(xp.permute(0, 3, 1, 2)[..., None], run.W).permute(0, 2, 3, 1, 4).reshape(-1, run.N)
        return G.epilogue(acc, run.e)

    def quad_through_f16(o):
        y = o["ref"].clone()
        y[:, -4:] = y[:, -4:].half().double()
        return y

    inst = "inst-t0w64-N164-K384-"
    return [("1 % of the neighbouring row leaks into the smallest-scale row", inst + "scaled", "f32res", leak),
            ("1 % of the neighbouring row leaks into the smallest-scale row", "inst-t8-K384-scaled", "f16rowbias", leak),
            ("the last row drops the last 8 k-elements", inst + "marked", "f32res", drop_k_tail),
            ("the last row drops the last 8 k-elements", "inst-t2-K384-marked", "f16rowbias", drop_k_tail),
            ("the last row drops the last 8 k-elements", "tail-N164-K200-marked", "f16", drop_k_tail),
            ("a k-tile dropped in one split, the next counted twice", "splitk-t0-K1600-reduce", "f32-biasn-rowbias-silu-reswrap", split_seam),
            ("a k-tile dropped in one split, the next counted twice", "splitk-t9-K1088-tickets", "hilo-biasm", split_seam),
            ("the residual wrap ignored", "feat-t0-scaled", "wraps-biasm", wrap_ignored),
            ("the residual wrap ignored", "splitk-t5-K1600-tickets", "f32-biasn-rowbias-silu-reswrap", wrap_ignored),
            ("the residual wrap ignored", "reswrap-conv-t5-split2", "tickets", wrap_ignored),
            ("the residual wrap ignored", "reswrap-tconv-t0-split3", "reduce", wrap_ignored),
            ("the row-bias batch index off by one at a seam row", "inst-t1-K384-scaled", "f16rowbias", rowbias_seam),
            ("the row-bias batch index off by one at a seam row", "splitk-t0-K1088-reduce", "f32-biasn-rowbias-silu-reswrap", rowbias_seam),
            ("the bias along M applied along N", "feat-t3-marked", "biasm-f16", bias_m_as_n),
            ("the bias along M applied along N", "splitk-t5-K1088-reduce", "hilo-biasm", bias_m_as_n),
            ("convolution padding replaced by the wrapped neighbouring pixel", "conv-t0-Cin64", "s1", conv_wrapped_pixel),
            ("convolution padding replaced by the wrapped neighbouring pixel", "c8-stem", "stem-f16", conv_wrapped_pixel),
            ("the first frame's padding replaced by the previous clip's last frame", "tconv-t0", "padded", tconv_previous_clip),
            ("one column quad of an fp32 output rounded through fp16", inst + "scaled", "f32res", quad_through_f16),
            ("one column quad of an fp32 output rounded through fp16", "inst-t11-K64-marked", "f32res", quad_through_f16),
            ("out_lo missing", "stats-t0-marked", "hilo", lambda o: o["ref"].half().double(), True),
            ("out_lo missing", "splitk-t0-K1600-tickets", "hilo-biasm", lambda o: o["ref"].half().double(), True)]


_MUTANTS = _mutants()


@pytest.mark.parametrize("m", _MUTANTS, ids=[f"{i:02d}-{m[1]}-{m[2]}" for i, m in enumerate(_MUTANTS)])
def test_mutation_lands_outside_the_gpu_tolerance(m):
    what, cid, name, fn = m[:4]
    o = _out(cid, name)
    _judge(what, cid, o, fn(o), lo_missing=len(m) > 4)


def test_whole_tensor_rel_l2_misses_what_the_segments_catch():
    """The evidence behind the suite: at N = 356 the fp16-output tolerance of the existing tests passes the leak, and their fp32 tolerance
    passes the quad that went through fp16."""
    by = {(m[0], m[1]): m for m in _MUTANTS}
    for key in (("1 % of the neighbouring row leaks into the smallest-scale row", "inst-t8-K384-scaled"),
                ("one column quad of an fp32 output rounded through fp16", "inst-t11-K64-marked")):
        what, cid, name, fn = by[key][:4]
        o = _out(cid, name)
        assert _judge(what, cid, o, fn(o)), (key, "one rel-L2 over the tensor was expected to pass this mutation")


@pytest.mark.parametrize("cid,name", [("stats-t0-marked", "stats-f32"), ("stats-t3-scaled", "stats-f16")])
def test_a_strip_that_counts_a_dead_row_lands_outside_the_gpu_tolerance(cid, name):
    """A dead row of the last (ragged) strip holds what the epilogue makes of a zero accumulator: the bias."""
    o = _out(cid, name)
    stored = o["ref"] if o["run"].out_dt == "f32" else o["ref"].half().double()
    ref = G.strip_sums(stored)
    dead = o["run"].e["bias"] if o["run"].out_dt == "f32" else o["run"].e["bias"].half().double()
    assert stored.shape[0] % 32 != 0
    for j, what in enumerate(("sums", "sums of squares")):
        mutated = ref[:, j].clone()
        mutated[-1] += dead if j == 0 else dead * dead
        e_torch = G.seg_err(G.strip_sums(stored, torch.float32)[:, j], ref[:, j])
        factor = float((G.seg_err(mutated, ref[:, j]) / G.bound_of(dict(rule="f32", e_torch=e_torch))).max())
        print(f"MUTATION a strip counts a dead row [{cid} / {name} {what}]: worst (strip, 32 columns) / tolerance = {factor:.1f}")
        assert factor >= 4.0, (cid, name, what, factor)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["id"])
def test_the_program_passes_in_the_interpreter(c):
    b = _b(c["id"])
    assert b.outs and len(b.outs) == len([op for op in b.P.ops if not op.name.endswith((".a_lo", ".w_lo"))])
    for o in b.outs:
        if o["rule"] == "f16":        # the fp16 tolerance is not spent on the output format: 2^-11 per element
            assert float(G.seg_err(o["ref"].half(), o["ref"]).max()) <= 2.0 ** -11, (c["id"], o["name"])
    it = AdapterInterp(b.P, b.w, poison=False)
    b.init(it)
    it.run({})
    print(G.figures_line(b, G.verify(it, b)))


def test_the_inputs_are_what_the_docstring_says():
    r, c = G.row_scale(400), G.col_scale(400)
    assert set(r.log2().tolist()) == set(range(-4, 5)) and (r[1:] != r[:-1]).all() and (r[32:] != r[:-32]).all()
    assert set(c.log2().tolist()) == set(range(-2, 3)) and (c.view(-1, 4) == c.view(-1, 4)[:, :1]).all() and (c[4:] != c[:-4]).all()
    X, Xm = G.operand_rows("scaled", 70, 200, 3), G.operand_rows("marked", 70, 200, 3)
    ratio = (Xm / X)[0]
    marked = sorted(int(k) for k in torch.nonzero(ratio != 1).flatten())
    assert marked == [63, 64, 127, 128, 191] + list(range(192, 200)) and set(ratio[marked].tolist()) == {4.0}
    Xi = G.operand_rows("marked", 2 * 5 * 7, 64, 3, image=(2, 5, 7)) / G.operand_rows("marked", 70, 64, 3)
    assert (Xi.view(2, 5, 7, 64)[:, 1:-1, 1:-1] == 1).all() and (Xi.view(2, 5, 7, 64)[:, 0] == 4).all() and (Xi.view(2, 5, 7, 64)[:, :, -1] == 4).all()
    Xc = G.operand_rows("marked", 2 * 5 * 7, 64, 3, clip=(2, 5, 7)) / G.operand_rows("marked", 70, 64, 3)
    assert (Xc.view(2, 5, 7, 64)[:, 1:-1] == 1).all() and (Xc.view(2, 5, 7, 64)[:, 0] == 4).all() and (Xc.view(2, 5, 7, 64)[:, -1] == 4).all()
    Xo, Wo = G.operand_rows("offset", 64, 384, 3), G.weight_like("offset", (164, 384), 3)
    assert torch.allclose(Xo.mean(dim=1) / Xo.std(dim=1), torch.full((64,), 8.0, dtype=torch.float64), rtol=0.2)
    assert float((Wo.sum(dim=1).abs() / Wo.abs().sum(dim=1)).max()) < 1e-3
    xf, hi, lo = G.split_f32(torch.randn(8, 8, dtype=torch.float64))
    assert torch.equal(xf.float().double(), xf) and G.rel_l2(hi.double() + lo.double(), xf) < 2.0 ** -20


def test_the_packed_images_follow_the_abi():
    """k = (64-channel chunk, tap, channel) and the GEGLU interleave, element by element."""
    w4 = torch.arange(2 * 128 * 9, dtype=torch.float64).view(2, 128, 3, 3)
    p = G.pack_conv3x3(w4)
    for co, ci, ky, kx in ((0, 0, 0, 0), (1, 70, 2, 1), (0, 127, 1, 2), (1, 64, 0, 0)):
        assert p[co, (ci // 64) * 576 + (3 * ky + kx) * 64 + ci % 64] == w4[co, ci, ky, kx]
    w8 = torch.arange(2 * 8 * 9, dtype=torch.float64).view(2, 8, 3, 3)
    assert G.pack_conv3x3_c8(w8)[1, (3 * 2 + 1) * 8 + 5] == w8[1, 5, 2, 1]
    w5 = torch.arange(2 * 128 * 3, dtype=torch.float64).view(2, 128, 3, 1, 1)
    assert G.pack_tconv3(w5)[1, (100 // 64) * 192 + 2 * 64 + 100 % 64] == w5[1, 100, 2, 0, 0]
    rows = G.geglu_rows(144)
    assert sorted(rows.tolist()) == list(range(288)) and rows[16 * 3 + 5] == 8 * 3 + 5 and rows[16 * 3 + 8 + 5] == 144 + 8 * 3 + 5


def test_the_case_list_covers_every_path():
    have = set()
    for c in G.CASES:
        have |= _b(c["id"]).features
    want = {"tile0/64", "tile0/128"} | {f"tile{t}" for t in G.GEMM2_TILES}
    want |= {"gather:plain", "gather:conv", "gather:c8", "gather:tconv", "gather:tconv/halo", "stride2", "up", "pad_after_only"}
    want |= {"out:f32", "out:f16", "bias_n", "bias_m", "rowbias", "silu", "relu", "residual", "geglu", "stats:f32", "stats:f16", "out_lo", "a_lo", "weight_lo",
             "ldw", "a_wrap", "res_wrap:i12", "res_wrap:i30:conv", "res_wrap:i30:tconv", "splitk:uneven"}
    for fold in ("reduce", "tickets"):
        want |= {f"splitk:{fold}", f"splitk:{fold}:tile0", f"splitk:{fold}:tile5", f"splitk:{fold}:tile9"}
        want |= {f"splitk:{fold}:{f}" for f in ("bias_n", "bias_m", "rowbias", "silu", "out_lo", "res_wrap:i30:plain", "res_wrap:i30:conv", "res_wrap:i30:tconv")}
    want.add("splitk:reduce:geglu")                      # (GEGLU always folds in the reduction kernel)
    assert want <= have, sorted(want - have)
    # every instantiation at both reduction lengths and both variants; every gather on every tile
    ids = set(_BY_ID)
    for t in ("t0w64-N164", "t0w128-N228") + tuple(f"t{t}" for t in G.GEMM2_TILES):
        assert {f"inst-{t}-K{k}-{v}" for k in (384, 64) for v in ("scaled", "marked")} <= ids
    for t in (0,) + G.GEMM2_TILES:
        assert {f"conv-t{t}-Cin64", f"conv-t{t}-Cin128", f"tconv-t{t}"} <= ids
