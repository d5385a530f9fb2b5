"""CPU: a batch of different prompts in one pass (ragged text contexts).  (1) what the designed inputs of tests/prompt_batch_inputs.py
expose; (2) the lowering of a ragged batch — its records, its canonical forms, and through the interpreter against the oracle per
sample; (3) the packed context and its cache; (4) record validation with no GPU; (5) the samplers' handling of context lists."""
import ctypes

import pytest
import torch

import prompt_batch_inputs as PB
from harness import program_digest, rel_l2
from interp_prompt_batch import PromptBatchInterp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers as S
from sd_webui_text2video_amd import unet as U
from sd_webui_text2video_amd.program import Program, Ref, TShardSpec


# ---- 1. the designed inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", PB.LENGTH_LISTS, ids=[str(v) for v in PB.LENGTH_LISTS])
def test_attention_inputs_expose_a_table_read_wrongly(lens):
    ls, starts = PB.flat(lens)
    q, kv = PB.attention_inputs(lens)
    assert torch.isnan(kv[:PB.GUARD]).all() and torch.isnan(kv[-PB.GUARD:]).all() and torch.isfinite(kv[PB.GUARD:-PB.GUARD]).all()
    assert kv.shape[0] == 2 * PB.GUARD + sum(ls)               # packed without padding: a neighbour's rows directly before and behind
    table = list(zip(ls, starts))
    right = PB.attention_ref64(q, kv, table)
    assert torch.isfinite(right).all()
    per = PB.FRAMES * PB.NQ
    for s, (n, r) in enumerate(table):
        wrong = [(n + 1, r), (n, r + 1), (n, r - 1)] + ([(n - 1, r)] if n > 1 else [])        # one key too many, one row off, one too few
        for entry in wrong:
            moved = PB.attention_ref64(q, kv, table[:s] + [entry] + table[s + 1:])[s * per:(s + 1) * per]
            d = rel_l2(moved, right[s * per:(s + 1) * per])
            assert not d <= PB.EXPOSED, (s, entry, d)              # (a read of a guard row is a NaN: exposed as well)


def test_attention_inputs_samples_differ_from_their_neighbours():
    for lens in PB.LENGTH_LISTS:
        ls, starts = PB.flat(lens)
        _, kv = PB.attention_inputs(lens)
        v = kv[PB.GUARD:-PB.GUARD, PB.HEADS * PB.HEAD_DIM:].float()
        means = [float(v[r:r + n].mean()) for n, r in zip(ls, starts)]
        assert all(abs(a - b) > 2 * PB.SAMPLE_SHIFT - 1 for a, b in zip(means, means[1:])), means


# ---- 2. the lowering ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    m = U.UNetSD(**configs.TINY_UNET)
    sd = synth.load_synth(m, seed=0)
    return m, sd


def _attn(comp):
    return [op for op in comp.prog.ops if op.kind == L.OP_ATTENTION]


def test_canonical_context_lengths():
    from sd_webui_text2video_amd.lowering import canonical_context_lengths
    assert canonical_context_lengths(77, 6) == 77 and canonical_context_lengths([77] * 6, 6) == 77
    assert canonical_context_lengths((154, 77), 6) == (154, 77) and canonical_context_lengths((77, 77), 6) == 77
    assert canonical_context_lengths([154, 154, 154, 77, 77, 77], 6) == (154, 77)
    assert canonical_context_lengths([154, 77], 2) == (154, 77) and canonical_context_lengths([77, 77], 2) == 77
    assert canonical_context_lengths([154, 77, 154, 77], 4) == (154, 77, 154, 77)
    assert canonical_context_lengths([77, 154, 231], 3) == (77, 154, 231)
    with pytest.raises(AssertionError):
        canonical_context_lengths([77, 154, 231], 4)


@pytest.mark.parametrize("guided", [True, False])
def test_ragged_program_records(tiny, guided):
    m, sd = tiny
    lens = PB.LENGTH_LISTS[0]
    ls, starts = PB.flat(lens) if guided else (list(lens[0]), [0, 154, 231])
    B = len(ls)
    ragged = m._compile(B, 2, 8, 8, tuple(ls), "f32", "f32", "f32", x_batch=B // 2 if guided else 0)
    unfused = m._compile(B, 2, 8, 8, max(ls), "f32", "f32", "f32", x_batch=B // 2 if guided else 0)        # 231 > 96 keys: no fused to_q + attention
    assert [op.kind for op in ragged.prog.ops] == [op.kind for op in unfused.prog.ops]          # every text cross-attention stays ONE launch
    with_table = [op for op in _attn(ragged) if op.i[22]]
    assert len(with_table) == sum(1 for op in _attn(unfused) if op.i[1] == max(ls)) > 0
    packed = ragged.packer.materialise(m.state_dict(), "cpu")
    for op in with_table:
        assert op.i[22:25] == [B, max(ls), sum(ls)] and op.i[19:22] == [0, 0, 0] and op.i[3] == B and op.i[1] == max(ls) and op.i[9] == 0
        assert op.p[7].space == "weight" and op.p[4].space == "null" and op.p[6].space == "null"
        assert packed[op.p[7].name].dtype == torch.int32 and packed[op.p[7].name].tolist() == [[n, r] for n, r in zip(ls, starts)]
    assert not any(op.i[16] == L.EPI_XATTN for op in ragged.prog.ops if op.kind == L.OP_GEMM)
    kv = next(op for op in ragged.prog.ops if op.name == "attn2.kv.all")
    cast = next(op for op in ragged.prog.ops if op.name == "context.cast")
    assert kv.i[0] == sum(ls) == cast.i[0] and kv.meta.get("step_invariant") and cast.meta.get("step_invariant")
    assert ragged.prog.arena.high <= unfused.prog.arena.high        # the table is program data in the weight image, not an arena buffer


def test_short_ragged_batch_leaves_the_fused_path(tiny):
    m, _ = tiny
    ls, _ = PB.flat(PB.LENGTH_LISTS[2])                        # every sample <= 96 keys: the fused to_q + attention would apply to a uniform batch
    ragged = m._compile(6, 2, 8, 8, tuple(ls), "f32", "f32", "f32", x_batch=3)
    assert not any(op.i[16] == L.EPI_XATTN for op in ragged.prog.ops if op.kind == L.OP_GEMM)
    assert all(op.i[22:25] == [6, 40, sum(ls)] for op in _attn(ragged) if op.i[22]) and any(op.i[22] for op in _attn(ragged))
    uniform = m._compile(6, 2, 8, 8, 40, "f32", "f32", "f32", x_batch=3)
    assert any(op.i[16] == L.EPI_XATTN for op in uniform.prog.ops if op.kind == L.OP_GEMM) == bool(getattr(m, "fused_cross_attention", True))


def test_uniform_lengths_are_todays_programs(tiny):
    m, sd = tiny
    for lens, today in (([77] * 6, 77), ([154] * 3 + [77] * 3, (154, 77)), ([24, 24, 40, 40], (24, 40)), ([77, 77], 77), ([154, 77], (154, 77))):
        B = len(lens)
        assert program_digest(m._compile(B, 2, 8, 8, tuple(lens), "f32", "f32", "f32", x_batch=B // 2), sd) == \
            program_digest(m._compile(B, 2, 8, 8, today, "f32", "f32", "f32", x_batch=B // 2), sd), lens


def test_t_sharded_lowering_refuses_a_ragged_batch(tiny):
    m, _ = tiny
    with pytest.raises(L.T2VError, match=r"\[154, 77, 231\]"):
        m._compile(3, 2, 8, 8, (154, 77, 231), "f32", "f32", "f32", shard=TShardSpec.make(4, 2, 0))


@pytest.mark.parametrize("geom,lens", [((2, 8, 8), PB.LENGTH_LISTS[2]), ((2, 8, 8), PB.LENGTH_LISTS[1])])
def test_ragged_program_matches_the_oracle_per_sample(tiny, geom, lens):
    m, sd = tiny
    cfg = configs.TINY_UNET
    x, t, cs, us = PB.unet_inputs(cfg, geom, lens)
    V, (ls, _) = len(cs), PB.flat(lens)
    comp = m._compile(2 * V, *geom, tuple(ls), "f32", "f32", "f32", x_batch=V)
    packed_ctx = torch.cat([c[0] for c in cs + us])
    out = torch.empty(2 * V, cfg["out_dim"], *geom)
    PromptBatchInterp(comp.prog, comp.packer.materialise(m.state_dict(), "cpu")).run(
        {L.EXT_X: x, L.EXT_T: t.float().repeat(2 * V), L.EXT_CTX: packed_ctx, L.EXT_OUT: out})
    errs = [rel_l2(out[b:b + 1], tp.unet_forward(sd, cfg, x[b % V: b % V + 1], t, ctx)) for b, ctx in enumerate(cs + us)]
    print(f"ragged program {geom} {lens}: " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < 4e-3, errs          # (the interpreter against the oracle: the gate of the pair program's test)


def test_unet_inputs_expose_a_neighbours_row(tiny):
    """One row of the next sample's context read as an own key moves the oracle's eps by several gates."""
    import prompt_inputs as PI
    m, sd = tiny
    cfg = configs.TINY_UNET
    geom, lens = (2, 8, 8), PB.LENGTH_LISTS[2]
    x, t, cs, us = PB.unet_inputs(cfg, geom, lens)
    right = tp.unet_forward(sd, cfg, x[:1], t, cs[0])
    more = tp.unet_forward(sd, cfg, x[:1], t, torch.cat([cs[0], cs[1][:, :1]], dim=1))
    fewer = tp.unet_forward(sd, cfg, x[:1], t, cs[0][:, :-1])
    assert rel_l2(more, right) > 3 * PI.UNET_GATE and rel_l2(fewer, right) > 3 * PI.UNET_GATE, (rel_l2(more, right), rel_l2(fewer, right))


# ---- 3. the packed context and its cache ----------------------------------------------------------------------------------------------
def test_packed_context_layout_and_cache(tiny):
    m, _ = tiny
    cfg = configs.TINY_UNET
    _, _, cs, us = PB.unet_inputs(cfg, (2, 8, 8), PB.LENGTH_LISTS[0])
    seqs = cs + [u[0] for u in us]                              # [1, L, ctx] and [L, ctx] entries
    y, pair, lens = m._context_batch(seqs, "token a")
    assert pair is None and lens == (154, 77, 231, 77, 77, 154) and y.shape == (770, cfg["context_dim"])
    assert torch.equal(y, torch.cat([c[0] for c in cs + us]))            # every sample's rows in batch order, no padding
    again, _, _ = m._context_batch(seqs, "token a")
    assert again is y                                                    # built once per context token
    other, _, _ = m._context_batch(seqs, "token b")
    assert other is not y and torch.equal(other, y)
    fresh, _, _ = m._context_batch(seqs, None)
    assert fresh is not other                                            # no token: nothing is vouched for
    shorter, _, lens2 = m._context_batch(seqs[:5] + [seqs[5][:100]], "token b")
    assert lens2[-1] == 100 and shorter.shape[0] == 716                  # the same token with other lengths is another context
    # lengths that one tensor or the pair describes take those forms
    y1, p1, l1 = m._context_batch([cs[0], cs[0]], None)
    assert p1 is None and l1 is None and y1.shape == (2, 154, cfg["context_dim"])
    y2, p2, l2 = m._context_batch([cs[0], cs[0], us[0], us[0]], None)
    assert p2 == (154, 77) and l2 is None and torch.equal(y2, torch.cat([cs[0][0], cs[0][0], us[0][0], us[0][0]]))


# ---- 4. record validation with no GPU -------------------------------------------------------------------------------------------------
def test_table_records_are_validated_before_any_launch(built_lib):
    h, ptr = ctypes.c_void_p(), 0x1000

    def check(i, p, entry):
        op = (L.T2VOp * 1)()
        op[0].kind, op[0].f[0] = L.OP_ATTENTION, 0.125
        for k, v in i.items():
            op[0].i[k] = v
        for k, v in p.items():
            op[0].p[k] = v
        if entry == "plan":
            rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
            if rc == 0:
                built_lib.t2v_plan_destroy(h)
        else:
            rc = built_lib.t2v_run_ops(op, 1, None, 0, None)          # refused in validation: nothing is launched, no device is touched
        return rc, built_lib.t2v_last_error()

    base = {0: 64, 1: 231, 2: 2, 3: 6, 4: 2, 5: 128, 8: 256, 11: 128, 14: 64}
    tab = {22: 6, 23: 231, 24: 770}
    pp = {0: ptr, 1: ptr, 2: ptr, 3: ptr}
    assert check(base, pp, "plan")[0] == 0
    assert check({**base, **tab}, {**pp, 7: ptr}, "plan")[0] == 0
    refused = [(tab, {}, b"null table"),
               ({**tab, 19: 3, 20: 77, 21: 77 * 256}, {7: ptr, 4: ptr, 5: ptr}, b"second role"),
               ({**tab, 0: 231, 15: 1}, {7: ptr}, b"causal"),
               ({**tab, 17: 256}, {7: ptr, 6: ptr}, b"scratch"),
               ({**tab, 22: 5}, {7: ptr}, b"batch_outer"),
               ({**tab, 23: 0}, {7: ptr}, b"largest key count"),
               ({**tab, 24: 100}, {7: ptr}, b"rows spanned"),
               ({}, {7: ptr}, b"without its fields")]
    for entry in ("plan", "run"):
        for bad_i, bad_p, why in refused:
            rc, msg = check({**base, **bad_i}, {**pp, **bad_p}, entry)
            assert rc == -1 and b"table" in msg and why in msg, (entry, bad_i, msg)
    # the relative-position op takes no table
    op = (L.T2VOp * 1)()
    op[0].kind, op[0].f[0] = L.OP_RELPOS_ATTN, 0.125
    for k, v in {0: 4, 1: 4, 2: 1, 3: 1, 4: 1, 14: 64, 15: 4, 22: 1, 23: 4, 24: 4}.items():
        op[0].i[k] = v
    for k in range(6):
        op[0].p[k] = ptr
    assert built_lib.t2v_plan_create(op, 1, ctypes.byref(h)) == -1 and b"per-sample table" in built_lib.t2v_last_error()


def test_program_attention_table_fields():
    P = Program("t")
    q, kv, o = P.alloc(3 * 64, 128, "f16"), P.alloc(100, 256, "f16"), P.alloc(3 * 64, 128, "f16")
    kw = dict(nq=64, heads=2, b_outer=3, b_inner=1, q_strides=(128, 64 * 128, 0), kv_strides=(256, 0, 0), o_strides=(128, 64 * 128, 0), scale=0.125)
    op = P.attention("a", q.ref, kv.ref, kv.col_slice(128, 256).ref, o.ref, nk=50, table=(Ref("weight", 0, "tab"), [50, 1, 49], [0, 50, 51]), **kw)
    assert op.i[22:25] == [3, 50, 100] and op.p[7] == Ref("weight", 0, "tab")
    with pytest.raises(AssertionError):
        P.attention("b", q.ref, kv.ref, kv.ref, o.ref, nk=50, table=(Ref("weight", 0, "tab"), [50, 0, 49], [0, 50, 51]), **kw)
    with pytest.raises(AssertionError):
        P.attention("c", q.ref, kv.ref, kv.ref, o.ref, nk=50, table=(Ref("weight", 0, "tab"), [50, 1, 49], [0, 50, 51]), causal=True, **kw)


# ---- 5. the samplers' handling of context lists -----------------------------------------------------------------------------------------
def test_batch_contexts_forms():
    a, b, c = torch.randn(1, 77, 8), torch.randn(1, 154, 8), torch.randn(1, 77, 8)
    u = torch.randn(1, 77, 8)
    assert S.batch_contexts(a, u, 3) == (a, u)                                   # tensors: untouched
    one_c, one_u = S.batch_contexts([a], [u], 3)
    assert one_c is a and one_u is u                                              # lists of one entry: that tensor, today's path
    cc, uu = S.batch_contexts([a, c, a], u, 3)
    assert torch.is_tensor(cc) and torch.equal(cc, torch.cat([a, c, a])) and uu is u          # one length per role: the tensors
    cc, uu = S.batch_contexts([a, b[0], c], u, 3)                                 # lengths differ: lists, the single tensor repeated
    assert isinstance(cc, list) and [v.shape for v in cc] == [a.shape, b.shape, c.shape] and len(uu) == 3 and all(v is u for v in uu)
    cc, uu = S.batch_contexts(a, [u, b, u], 3)
    assert isinstance(cc, list) and all(v is a for v in cc) and [v.shape[1] for v in uu] == [77, 154, 77]
    with pytest.raises(ValueError, match="2 contexts for a batch of 3"):
        S.batch_contexts([a, b], u, 3)


class _ListModel:
    """Records what the evaluator hands to the model."""
    device = "cpu"

    def __init__(self):
        self.calls = []

    def forward_cfg_pair(self, x, t, pair, context_token=None, single_t=None):
        self.calls.append(("pair", pair, context_token))
        return torch.zeros(2 * x.shape[0], *x.shape[1:])

    def __call__(self, x, t, y):
        self.calls.append(("forward", y, getattr(self, "context_token", None)))
        return torch.zeros_like(x)


def test_eval_eps_pair_routes_context_lists():
    m = _ListModel()
    x = torch.zeros(3, 4, 2, 8, 8)
    cs, us = [torch.randn(1, n, 8) for n in (77, 154, 231)], [torch.randn(1, 77, 8)] * 3
    cache = {}
    eps, guided = S._eval_eps_pair(m, x, 601, cs, us, 9.0, cache=cache)
    assert guided and eps.shape[0] == 6 and m.calls[-1][0] == "pair" and m.calls[-1][1] == (cs, us)
    token = m.calls[-1][2]
    S._eval_eps_pair(m, x, 401, cs, us, 9.0, cache=cache)
    assert m.calls[-1][2] == token                                  # the same objects in the same run: the same context token
    S._eval_eps_pair(m, x, 401, cs, us, 9.0, cache={})
    assert m.calls[-1][2] != token                                  # another run: another token
    eps, guided = S._eval_eps_pair(m, x, 601, cs, None, 1.0, cache=cache)
    assert not guided and eps.shape[0] == 3 and m.calls[-1][0] == "forward" and m.calls[-1][1] == cs and m.calls[-1][2] is not None

    class _Pair:
        size, role = 2, 0
    with pytest.raises(L.T2VError, match="CFG-pair"):
        S._eval_eps_pair(m, x, 601, cs, us, 9.0, cfg_parallel=_Pair(), cache={})
    m.t_shard = object()
    with pytest.raises(L.T2VError, match=r"\[77, 154, 231\]"):
        S._eval_eps_pair(m, x, 601, cs, us, 9.0, cache={})
