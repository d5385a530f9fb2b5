"""CPU: the webui prompt syntax of the ModelScope path and a guided step whose cond / uncond contexts have different lengths.
(1) `parse_prompt_attention` on webui's acceptance table; (2) `tokenize_line` against the golden recorded from the reference
(tests/golden/make_golden_prompt.py) and, where the reference checkout is present, against the live reference; (3) the samplers'
routing of an unequal pair; (4) the lowering of the pair program; (5) the interpreter on it, and on T2V_OP_EMPHASIS; (6) proof, in
float64, that the designed inputs of the GPU tests expose the mistakes those tests exist to catch."""
import os

import numpy as np
import pytest
import torch

import prompt_inputs as PI
from harness import program_digest, rel_l2
from interp_prompt import PromptInterp
from oracle import configs, ref_bootstrap as rb, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers as S
from sd_webui_text2video_amd import text_encoder as TE
from sd_webui_text2video_amd import unet as U
from test_text_encoder_cpu import TINY, _seed_params

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "prompt_syntax.npz"))
needs_reference = pytest.mark.skipif(not rb.reference_available(), reason="the reference checkout is not on this machine")
CASES = [(i, e, b) for i in range(len(PI.PROMPTS)) for e, b in PI.SETTINGS]


# ---- 1. the parser ------------------------------------------------------------------------------------------------------------------
TABLE = [
    ("normal text", [["normal text", 1.0]]),
    ("an (important) word", [["an ", 1.0], ["important", 1.1], [" word", 1.0]]),
    ("(unbalanced", [["unbalanced", 1.1]]),
    (r"\(literal\]", [["(literal]", 1.0]]),
    ("(unnecessary)(parens)", [["unnecessaryparens", 1.1]]),
    (PI.TABLE_LAST, [["a ", 1.0], ["house", 1.573], [" ", 1.1], ["on", 1.0], [" a ", 1.1], ["hill", 0.55], [", sun, ", 1.1], ["sky", 1.4641],
                     [".", 1.1]]),
]


@pytest.mark.parametrize("text,expect", TABLE, ids=[t for t, _ in TABLE])
def test_parser_acceptance_table(text, expect):
    got = TE.parse_prompt_attention(text)
    assert [p for p, _ in got] == [p for p, _ in expect]
    for (_, w), (_, e) in zip(got, expect):
        assert abs(w - e) <= 1e-12 * abs(e), (w, e)


def test_parser_break_colon_and_empty():
    assert TE.parse_prompt_attention("") == [["", 1.0]]
    assert TE.parse_prompt_attention("a BREAK b") == [["a", 1.0], ["BREAK", -1], ["b", 1.0]]
    assert TE.parse_prompt_attention("BREAKFAST at 10:30") == [["BREAKFAST at 10:30", 1.0]]          # a word boundary; a colon without `)`
    assert TE.parse_prompt_attention("x] (y : .5 )") == [["x] ", 1.0], ["y ", 0.5]]                  # an unmatched closer is text; spaces round w
    assert TE.parse_prompt_attention("\\\\(a)") == [["\\", 1.0], ["a", 1.1]]


# ---- 2. tokenize_line ---------------------------------------------------------------------------------------------------------------
def _embedder(emphasis=False, backtrack=0, **kw):
    m = kw.pop("model", None) or TE.OpenClipTextModel(**TINY)
    return TE.FrozenOpenCLIPEmbedder(model=m, layer="penultimate", tokenizer=PI.ToyTokenizer(), device=kw.pop("device", "cpu"),
                                     enable_emphasis=emphasis, comma_padding_backtrack=backtrack)


def test_recorded_prompts_are_the_ones_the_tests_use():
    assert GOLD["prompts"].tolist() == PI.PROMPTS
    tok = PI.ToyTokenizer()
    assert [len(tok.encode(p)) for p in PI.PROMPTS[1:5]] == [75, 76, 83, 83]


@pytest.mark.parametrize("idx,emphasis,backtrack", CASES)
def test_tokenize_line_equals_the_golden(idx, emphasis, backtrack):
    emb = _embedder(emphasis, backtrack)
    assert (emb.id_start, emb.id_end, emb.comma_token) == (PI.START_ID, PI.END_ID, PI.COMMA_ID)
    chunks, count = emb.tokenize_line(PI.PROMPTS[idx])
    k = PI.key(idx, emphasis, backtrack)
    assert all(isinstance(c, tuple) and len(c[0]) == len(c[1]) == 77 for c in chunks)
    assert np.array_equal(np.array([t for t, _ in chunks]), GOLD[k + "_tokens"])
    assert np.array_equal(np.array([m for _, m in chunks], dtype=np.float64), GOLD[k + "_mult"])      # the same float operations: equal bits
    assert count == int(GOLD[k + "_count"])
    assert emb.get_target_prompt_token_count(count) == -(-max(count, 1) // 75) * 75


def test_golden_covers_what_it_was_recorded_for():
    """The recorded cases do what their names say (a fixture that never back-tracks or never breaks would prove nothing)."""
    n = lambda i, e, b: GOLD[PI.key(i, e, b) + "_tokens"].shape[0]
    body = lambda i, e, b: [int((r[1:] != PI.END_ID).sum()) for r in GOLD[PI.key(i, e, b) + "_tokens"]]
    assert n(0, True, 20) == 1 and n(1, True, 20) == 1 and n(2, True, 20) == 2
    assert body(3, True, 0) == [75, 8] and body(3, True, 20) == [71, 12]          # the text behind the comma moved to the next chunk
    assert body(4, True, 20) == body(4, True, 0) == [75, 8]                       # the comma is farther back than the window
    assert n(5, True, 0) == 2 and n(5, False, 0) == 1                             # BREAK is a word when emphasis is off
    assert n(6, True, 0) == 2 and body(6, True, 0)[0] == 0                        # BREAK first: an empty chunk in front
    assert int(GOLD[PI.key(5, True, 0) + "_count"]) == 75 + 3                      # a chunk closed by BREAK counts as full
    m = GOLD[PI.key(9, True, 20) + "_mult"]
    assert m.shape == (2, 77) and {1.4, 1.1}.issubset(set(np.round(m.ravel(), 12)))


@needs_reference
def test_tokenize_line_equals_the_live_reference():
    ref, ch = PI.reference_embedder()
    for idx, emphasis, backtrack in CASES:
        want, want_count = PI.reference_chunks(ref, ch, PI.PROMPTS[idx], emphasis, backtrack)
        got, count = _embedder(emphasis, backtrack).tokenize_line(PI.PROMPTS[idx])
        assert [(list(t), list(m)) for t, m in got] == want and count == want_count, (idx, emphasis, backtrack)
        assert ref.get_target_prompt_token_count(count) == _embedder().get_target_prompt_token_count(count)


def test_default_options_tokenise_as_before():
    """Emphasis off, back-track 0 (the constructor's defaults): plain 75-token chunks, every multiplier 1.0, brackets tokenised as text."""
    emb = _embedder()
    assert emb.enable_emphasis is False and emb.comma_padding_backtrack == 0
    for prompt in PI.PROMPTS + ["x " * 151]:
        tokens = PI.ToyTokenizer().encode(prompt)
        want, want_count = [], 0
        for c0 in range(0, max(len(tokens), 1), 75):
            body = tokens[c0:c0 + 75]
            want_count += len(body) if c0 + 75 >= len(tokens) else 75
            want.append(([PI.START_ID] + body + [PI.END_ID] * (76 - len(body)), [1.0] * 77))
        assert emb.tokenize_line(prompt) == (want, want_count)


def test_pipeline_hands_the_options_on():
    from sd_webui_text2video_amd import pipeline as PL
    emb = _embedder()
    pipe = PL.TextToVideoSynthesis.__new__(PL.TextToVideoSynthesis)
    pipe.clip_encoder = emb
    pipe.set_prompt_options(True, 20)
    assert emb.enable_emphasis is True and emb.comma_padding_backtrack == 20
    pipe.set_prompt_options(None, None)
    assert emb.enable_emphasis is True and emb.comma_padding_backtrack == 20
    pipe.clip_encoder = lambda texts: None           # an encoder without the options: nothing to set, no error
    pipe.set_prompt_options(True, 20)


# ---- 3. the samplers' routing -------------------------------------------------------------------------------------------------------
class _PairModel:
    def __init__(self):
        self.calls = []

    def forward_cfg_pair(self, x, t, ctx_pair, context_token=None, single_t=None):
        self.calls.append(("pair", ctx_pair, context_token))
        return torch.zeros(2 * x.shape[0], *x.shape[1:])

    def __call__(self, x, t, y):
        self.calls.append(("call", x.shape[0], tuple(y.shape)))
        return torch.zeros_like(x)


class _BatchModel:
    supports_cfg_batch = True

    def __init__(self):
        self.calls = []

    def __call__(self, x, t, y):
        self.calls.append((x.shape[0], tuple(y.shape)))
        return torch.zeros_like(x)


def test_eval_eps_pair_routes_unequal_lengths():
    x = torch.zeros(1, 4, 2, 4, 4)
    c, uc = torch.randn(1, 154, 8), torch.randn(1, 77, 8)
    m, cache = _PairModel(), {}
    eps, guided = S._eval_eps_pair(m, x, 601, c, uc, 9.0, cache=cache)
    S._eval_eps_pair(m, x, 581, c, uc, 9.0, cache=cache)
    assert guided and eps.shape[0] == 2 and [k for k, *_ in m.calls] == ["pair", "pair"]
    kind, pair, token = m.calls[0]
    assert isinstance(pair, tuple) and pair[0] is c and pair[1] is uc and token is not None
    assert m.calls[1][1] is pair and m.calls[1][2] == token                     # built once per run, the same token: the K / V are reused
    # a model that only batches gets two forwards (never the concatenation of 154 against 77 rows)
    b = _BatchModel()
    eps, guided = S._eval_eps_pair(b, x, 601, c, uc, 9.0, cache={})
    assert guided and eps.shape[0] == 2 and b.calls == [(1, (1, 154, 8)), (1, (1, 77, 8))]
    # equal lengths: as before — the concatenated batch
    c2 = torch.randn(1, 77, 8)
    m2 = _PairModel()
    S._eval_eps_pair(m2, x, 601, c2, uc, 9.0, cache={})
    assert torch.is_tensor(m2.calls[0][1]) and torch.equal(m2.calls[0][1], torch.cat([c2, uc]))
    b2 = _BatchModel()
    S._eval_eps_pair(b2, x, 601, c2, uc, 9.0, cache={})
    assert b2.calls == [(2, (2, 77, 8))]


# ---- 4. the lowering ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    m = U.UNetSD(**configs.TINY_UNET)
    sd = synth.load_synth(m, seed=0)
    return m, sd


def _ops(comp, kind):
    return [op for op in comp.prog.ops if op.kind == kind]


@pytest.mark.parametrize("share", [False, True])
def test_pair_program_records(tiny, share, monkeypatch):
    m, _ = tiny
    monkeypatch.setattr(m, "_share_now", share)
    V = 1
    ragged = m._compile(2 * V, 2, 8, 8, (154, 77), "f32", "f32", "f32", x_batch=V)
    unfused = m._compile(2 * V, 2, 8, 8, 154, "f32", "f32", "f32", x_batch=V)          # 154 > 96 keys: no fused to_q + attention
    assert len(_ops(ragged, L.OP_ATTENTION)) == len(_ops(unfused, L.OP_ATTENTION)) > 0
    assert [op.kind for op in ragged.prog.ops] == [op.kind for op in unfused.prog.ops]
    two_role = [op for op in _ops(ragged, L.OP_ATTENTION) if op.i[19]]
    assert len(two_role) == sum(1 for op in _ops(unfused, L.OP_ATTENTION) if op.i[1] == 154) > 0
    for op in two_role:
        assert (op.i[1], op.i[19], op.i[20], op.i[3]) == (154, V, 77, 2 * V) and op.i[21] == 77 * op.i[8] and op.i[9] == 154 * op.i[8]
        assert op.p[4].off - op.p[1].off == V * 154 * op.i[8] * 2 == op.p[5].off - op.p[2].off
    assert not any(op.i[16] == L.EPI_XATTN for op in _ops(ragged, L.OP_GEMM))
    kv = next(op for op in ragged.prog.ops if op.name == "attn2.kv.all")
    cast = next(op for op in ragged.prog.ops if op.name == "context.cast")
    assert kv.i[0] == V * 231 == cast.i[0] and kv.meta.get("step_invariant") and cast.meta.get("step_invariant")


def test_short_pair_leaves_the_fused_path_and_two_videos(tiny):
    m, _ = tiny
    V = 2
    ragged = m._compile(2 * V, 2, 8, 8, (24, 40), "f32", "f32", "f32", x_batch=V)
    assert not any(op.i[16] == L.EPI_XATTN for op in _ops(ragged, L.OP_GEMM))
    assert next(op for op in ragged.prog.ops if op.name == "attn2.kv.all").i[0] == V * 64
    assert all((op.i[19], op.i[20], op.i[1]) == (V, 40, 24) for op in _ops(ragged, L.OP_ATTENTION) if op.i[19])


def test_equal_pair_is_todays_program(tiny):
    m, sd = tiny
    for Lctx in (77, 7):
        assert program_digest(m._compile(2, 2, 8, 8, (Lctx, Lctx), "f32", "f32", "f32", x_batch=1), sd) == \
            program_digest(m._compile(2, 2, 8, 8, Lctx, "f32", "f32", "f32", x_batch=1), sd)


def test_t_sharded_lowering_refuses_an_unequal_pair(tiny):
    from sd_webui_text2video_amd.program import TShardSpec
    m, _ = tiny
    with pytest.raises(L.T2VError, match="154 and 77"):
        m._compile(1, 2, 8, 8, (154, 77), "f32", "f32", "f32", shard=TShardSpec.make(4, 2, 0))


def test_second_role_is_refused_where_no_kernel_takes_it(built_lib):
    import ctypes
    h, ptr = ctypes.c_void_p(), 0x1000

    def create(kind, i, p, f0=0.125):
        op = (L.T2VOp * 1)()
        op[0].kind, op[0].f[0] = kind, f0
        for k, v in i.items():
            op[0].i[k] = v
        for k, v in p.items():
            op[0].p[k] = v
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    base = {0: 64, 1: 154, 2: 2, 3: 2, 4: 2, 5: 128, 8: 256, 9: 154 * 256, 11: 128, 14: 64}
    pp = {0: ptr, 1: ptr, 2: ptr, 3: ptr}
    alt = {19: 1, 20: 77, 21: 77 * 256}
    assert create(L.OP_ATTENTION, base, pp)[0] == 0
    assert create(L.OP_ATTENTION, {**base, **alt}, {**pp, 4: ptr, 5: ptr})[0] == 0
    for bad_i, bad_p in (({**alt, 19: 2}, {4: ptr, 5: ptr}), ({**alt, 20: 0}, {4: ptr, 5: ptr}), (alt, {4: ptr}),
                         ({**alt, 0: 154, 15: 1}, {4: ptr, 5: ptr}), ({**alt, 17: 192}, {4: ptr, 5: ptr, 6: ptr})):
        rc, msg = create(L.OP_ATTENTION, {**base, **bad_i}, {**pp, **bad_p})
        assert rc == -1 and b"second role" in msg, (bad_i, msg)
    rel = {0: 4, 1: 4, 2: 1, 3: 1, 4: 1, 14: 64, 15: 4}
    rc, msg = create(L.OP_RELPOS_ATTN, {**rel, 19: 1}, {k: ptr for k in range(6)})
    assert rc == -1 and b"second role" in msg
    # the emphasis record
    assert create(L.OP_EMPHASIS, {0: 77, 1: 128, 2: 128, 3: 128, 4: L.F16}, {0: ptr, 1: ptr, 2: ptr})[0] == 0
    for bad in ({1: 126}, {2: 64}, {4: 7}, {0: 0}):
        rc, msg = create(L.OP_EMPHASIS, {0: 77, 1: 128, 2: 128, 3: 128, 4: L.F16, **bad}, {0: ptr, 1: ptr, 2: ptr})
        assert rc == -1 and b"emphasis" in msg
    assert create(L.OP_EMPHASIS, {0: 77, 1: 128, 2: 128, 3: 128}, {0: ptr, 1: ptr})[0] == -1


# ---- 5. the interpreter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,V,share", [((154, 77), 1, True), ((24, 40), 1, False), ((24, 40), 2, False)])
def test_pair_program_matches_the_oracle_per_role(tiny, lens, V, share, monkeypatch):
    m, sd = tiny
    cfg = configs.TINY_UNET
    monkeypatch.setattr(m, "_share_now", share)
    F, H, W = 2, 8, 8
    x, t, c, uc = PI.ragged_inputs(cfg, V, F, H, W, *lens)
    comp = m._compile(2 * V, F, H, W, lens, "f32", "f32", "f32", x_batch=V)
    packed_ctx = torch.cat([c.reshape(-1, c.shape[2]), uc.reshape(-1, uc.shape[2])])
    out = torch.empty(2 * V, cfg["out_dim"], F, H, W)
    PromptInterp(comp.prog, comp.packer.materialise(m.state_dict(), "cpu")).run(
        {L.EXT_X: x, L.EXT_T: t.float().repeat(2 * V), L.EXT_CTX: packed_ctx, L.EXT_OUT: out})
    tv = t.repeat(V)
    r_c, r_u = rel_l2(out[:V], tp.unet_forward(sd, cfg, x, tv, c)), rel_l2(out[V:], tp.unet_forward(sd, cfg, x, tv, uc))
    print(f"pair program {lens} V={V} share={share}: cond {r_c:.3e} uncond {r_u:.3e}")
    assert r_c < 4e-3 and r_u < 4e-3


def test_emphasis_op_in_the_interpreter():
    model = _seed_params(TE.OpenClipTextModel(**TINY), 4)
    tower = TE.ClipTextTower(model, heads=2, act="gelu", skip_last=1)
    plain, comp = tower._compile(2, 77), tower._compile(2, 77, emphasis=True)
    assert [op.kind for op in comp.prog.ops][:-1] == [op.kind for op in plain.prog.ops][:-1]
    assert comp.prog.ops[-1].kind == L.OP_EMPHASIS == 24 and plain.prog.ops[-1].kind == L.OP_COPY2D and comp.prog.ops[-1].p[1].space == "ext"
    g = torch.Generator().manual_seed(5)
    tok = torch.randint(1, 400, (2, 77), generator=g)
    _, mult = PI.emphasis_inputs(2, 77, 128)
    z = torch.empty(2, 77, 128)
    PromptInterp(comp.prog, comp.packer.materialise(model.state_dict(), "cpu")).run(
        {L.EXT_X: tok.to(torch.int32), TE.EXT_MULT: mult, L.EXT_OUT: z})
    ref = tp.clip_process_tokens(tp.clip_text_forward(model.state_dict(), tok, heads=2, layers=2), mult)
    assert rel_l2(z, ref) < 3e-3
    # the op alone, on the designed inputs, against the float64 formula
    from sd_webui_text2video_amd.program import Buf, Program, Ref
    for shape in PI.EMPHASIS_SHAPES:
        zin, mult = PI.emphasis_inputs(*shape)
        P = Program("emphasis")
        rows, W = shape[0] * shape[1], shape[2]
        P.emphasis("e", Buf(Ref("ext", 1), rows, W, W, "f32"), Ref("ext", 2), Buf(Ref("ext", 3), rows, W, W, "f32"))
        out = torch.empty(shape)
        PromptInterp(P, {}).run({1: zin, 2: mult, 3: out})
        assert PI.max_rel(out, PI.emphasis_ref64(zin, mult)) <= PI.EMPHASIS_GATE
        assert PI.max_rel(out, tp.clip_process_tokens(zin, mult)) <= 8 * PI.EMPHASIS_GATE      # (the reference's own fp32 means: a looser pin)


# ---- 6. what the designed inputs expose ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PI.EMPHASIS_SHAPES)
def test_emphasis_inputs_expose_the_mean_and_the_ratio(shape):
    z, m = PI.emphasis_inputs(*shape)
    ref = PI.emphasis_ref64(z, m)
    zm = z.double() * m.double()[..., None]
    assert float(zm.abs().sum() / zm.sum().abs()) <= 100                                   # the conditioning the gate's derivation assumes
    assert (m == 0).any() and (m < 0).any() and z.mean(dim=2).std() > 0.2
    assert PI.max_rel(PI.emphasis_ref64(z, m, "inverted"), ref) >= 100 * PI.EMPHASIS_GATE
    if shape[0] > 1:                                                                       # (one chunk: its mean IS the batch mean)
        assert bool((m[-1] == 1).all())
        assert PI.max_rel(PI.emphasis_ref64(z, m, "per_row"), ref) >= 100 * PI.EMPHASIS_GATE


@pytest.mark.parametrize("geom", [(2, 8, 8), (3, 16, 16)])
@pytest.mark.parametrize("lens", [(154, 77), (77, 154)])
def test_ragged_inputs_expose_the_key_count(tiny, geom, lens):
    """Both roles on the larger key count — the shorter side's extra keys being the other role's rows — moves the shorter role's eps
    by at least 10x the forward's gate."""
    _, sd = tiny
    cfg = configs.TINY_UNET
    x, t, c, uc = PI.ragged_inputs(cfg, 1, *geom, *lens)
    short, other = (uc, c) if lens[1] < lens[0] else (c, uc)
    right = tp.unet_forward(sd, cfg, x, t, short)
    wrong = tp.unet_forward(sd, cfg, x, t, torch.cat([short, other[:, :abs(lens[0] - lens[1])]], dim=1))
    assert rel_l2(wrong, right) >= 10 * PI.UNET_GATE
