"""GPU (-m gpu): the prompt syntax of the ModelScope path on the device.  (1) T2V_OP_ATTENTION with two roles against single-role launches
of the same kernel, bit for bit; (2) the tiny UNet on a cond / uncond pair of different context lengths against the oracle, per role;
(3) three sampling steps of every sampler (four of "DDIM", whose schedule admits no three) on such a pair against the same loop run as two forwards per step; (4) T2V_OP_EMPHASIS against
the float64 formula; (5) the embedder end to end on a prompt with emphasis and BREAK.  The inputs are those of tests/prompt_inputs.py;
tests/test_prompt_syntax_cpu.py proves what they expose."""
import os

import numpy as np
import pytest
import torch

import prompt_inputs as PI
from harness import rel_l2
from interp_prompt import PromptInterp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from sd_webui_text2video_amd import text_encoder as TE
from sd_webui_text2video_amd import unet as U
from sd_webui_text2video_amd.program import BoundProgram, Buf, Program, Ref
from test_text_encoder_cpu import TINY, _seed_params

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "prompt_syntax.npz"))


def _run(prog, host: PromptInterp, ext=None):
    """Run `prog` on the GPU from the arena contents of `host`; -> an interpreter object holding the arena after the run."""
    dev = torch.device(DEV)
    arena = host.arena.to(dev)
    ext_gpu = {k: v.to(dev).contiguous() for k, v in (ext or {}).items()}
    bound = BoundProgram(prog, arena.data_ptr(), {})
    bound.run({k: v.data_ptr() for k, v in ext_gpu.items()}, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    L.async_status()
    got = PromptInterp(prog, {}, poison=False)
    got.arena = arena.cpu()
    return got, {k: v.cpu() for k, v in ext_gpu.items()}


# ---- 1. the attention op with two roles -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1, 2])
@pytest.mark.parametrize("lens", [(154, 77), (77, 154), (40, 24), (24, 40), (33, 32)])
def test_attention_two_roles_equal_single_role_launches(lens, V):
    Lc, Lu = lens
    heads, nq, F, D, GUARD = 2, 64, 2, 64, 3
    inner, ld = heads * D, 2 * heads * D
    B = 2 * V
    P = Program("attention two roles")
    q = P.alloc(B * F * nq, inner, "f16")
    kv = P.alloc(GUARD + V * (Lc + Lu) + GUARD, ld, "f16")
    outs = [P.alloc(B * F * nq, inner, "f16") for _ in range(4)]
    rows = kv.row_slice(GUARD, GUARD + V * (Lc + Lu))
    k1, v1 = rows.col_slice(0, inner), rows.col_slice(inner, ld)
    k2, v2 = k1.row_slice(V * Lc, V * (Lc + Lu)), v1.row_slice(V * Lc, V * (Lc + Lu))
    common = dict(nq=nq, heads=heads, b_inner=F, q_strides=(inner, F * nq * inner, nq * inner), o_strides=(inner, F * nq * inner, nq * inner),
                  scale=D ** -0.5)
    # [0] both roles in one launch
    P.attention("pair", q.ref, k1.ref, v1.ref, outs[0].ref, nk=Lc, b_outer=B, kv_strides=(ld, Lc * ld, 0), alt=(V, Lu, k2.ref, v2.ref, Lu * ld), **common)
    # [1] each role as a launch of its own (all-zero second-role fields), on the same data
    q2, o2 = q.row_slice(V * F * nq, B * F * nq), outs[1].row_slice(V * F * nq, B * F * nq)
    P.attention("cond", q.ref, k1.ref, v1.ref, outs[1].ref, nk=Lc, b_outer=V, kv_strides=(ld, Lc * ld, 0), **common)
    P.attention("uncond", q2.ref, k2.ref, v2.ref, o2.ref, nk=Lu, b_outer=V, kv_strides=(ld, Lu * ld, 0), **common)
    # [2] / [3] a second role that describes the SAME layout as the first (Lc keys, the rows that follow) = the plain record over 2 V' samples
    Vh = min(V, (V * (Lc + Lu)) // (2 * Lc))           # samples of Lc keys that fit twice into the rows (and into q)
    if Vh:
        kh, vh = k1.row_slice(Vh * Lc, 2 * Vh * Lc), v1.row_slice(Vh * Lc, 2 * Vh * Lc)
        P.attention("same.alt", q.ref, k1.ref, v1.ref, outs[2].ref, nk=Lc, b_outer=2 * Vh, kv_strides=(ld, Lc * ld, 0),
                    alt=(Vh, Lc, kh.ref, vh.ref, Lc * ld), **common)
        P.attention("same.plain", q.ref, k1.ref, v1.ref, outs[3].ref, nk=Lc, b_outer=2 * Vh, kv_strides=(ld, Lc * ld, 0), **common)
    assert all(op.i[19:22] == [0, 0, 0] and op.p[4].space == "null" for op in P.ops if op.name in ("cond", "uncond", "same.plain"))

    host = PromptInterp(P, {}, poison=False)
    g = torch.Generator().manual_seed(Lc * 1000 + Lu + V)
    host.mat(q.ref, q.rows, inner, inner, torch.float16, {}).copy_(torch.randn(q.rows, inner, generator=g).half())
    kvv = host.mat(kv.ref, kv.rows, ld, ld, torch.float16, {})
    kvv.copy_((1.5 * torch.randn(kv.rows, ld, generator=g)).half())
    kvv[:GUARD] = float("nan")                         # in front of the first role's rows and behind the last role's: never read
    kvv[-GUARD:] = float("nan")
    for o in outs:
        host.mat(o.ref, o.rows, inner, inner, torch.float16, {}).fill_(float("nan"))
    got, _ = _run(P, host)
    rd = lambda b, n=None: got.mat(b.ref, b.rows if n is None else n, inner, inner, torch.float16, {})
    pair, single = rd(outs[0]), rd(outs[1])
    assert torch.isfinite(pair.float()).all()
    assert torch.equal(pair[: V * F * nq], single[: V * F * nq]), "cond role"
    assert torch.equal(pair[V * F * nq:], single[V * F * nq:]), "uncond role"
    if Vh:
        n = 2 * Vh * F * nq
        assert torch.isfinite(rd(outs[3], n).float()).all() and torch.equal(rd(outs[2], n), rd(outs[3], n))
    # and the interpreter's reading of the record agrees with the kernel (fp16 output rounding + fp16 probabilities)
    host.run({}, ops=P.ops[:1])
    want = host.mat(outs[0].ref, outs[0].rows, inner, inner, torch.float16, {})
    assert rel_l2(pair.float(), want.float()) < 2e-3


# ---- 2. the tiny UNet on a ragged pair ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    sd = synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, sd, betas


_REFS = {}


def _role_refs(sd, V, geom, lens):
    """The oracle's eps of each role, computed once per case and shared."""
    k = (V, geom, lens)
    if k not in _REFS:
        cfg = configs.TINY_UNET
        x, t, c, uc = PI.ragged_inputs(cfg, V, *geom, *lens)
        tv = t.repeat(V)
        _REFS[k] = (x, t, c, uc, tp.unet_forward(sd, cfg, x, tv, c), tp.unet_forward(sd, cfg, x, tv, uc))
    return _REFS[k]


@pytest.mark.parametrize("V,geom,lens,share", [(1, (2, 8, 8), (154, 77), True), (1, (2, 8, 8), (77, 154), False), (1, (3, 16, 16), (154, 77), False),
                                               (1, (3, 16, 16), (77, 154), True), (2, (2, 8, 8), (154, 77), True)])
def test_tiny_unet_ragged_pair(tiny, V, geom, lens, share, monkeypatch):
    net, sd, _ = tiny
    monkeypatch.setattr(net, "share_cfg_prefix", share, raising=False)
    x, t, c, uc, ref_c, ref_u = _role_refs(sd, V, geom, lens)
    xd, td, cd, ud = x.to(DEV), t.to(DEV), c.to(DEV), uc.to(DEV)
    token = ("ragged", V, geom, lens, share)
    eps = net.forward_cfg_pair(xd, td, (cd, ud), context_token=token, single_t=True)
    again = net.forward_cfg_pair(xd, td, (cd, ud), context_token=token, single_t=True)          # the step-invariant prologue is skipped
    assert eps.shape == (2 * V, 4) + geom and torch.equal(eps, again)
    r_c, r_u = rel_l2(eps[:V].float().cpu(), ref_c), rel_l2(eps[V:].float().cpu(), ref_u)
    print(f"ragged pair V={V} {geom} {lens} share={share}: cond {r_c:.3e} uncond {r_u:.3e}")
    assert r_c < PI.UNET_GATE and r_u < PI.UNET_GATE, (r_c, r_u)
    comp = next(cc for kk, cc in net._programs.items() if kk[:5] == (2 * V,) + geom + (lens,))      # (other batch sizes of the same lengths may still be cached)
    assert any(op.i[19] == V for op in comp.prog.ops if op.kind == L.OP_ATTENTION)


@pytest.mark.parametrize("share", [False, True])
def test_equal_pair_is_the_tensor_path(tiny, share, monkeypatch):
    net, sd, _ = tiny
    monkeypatch.setattr(net, "share_cfg_prefix", share, raising=False)
    x, t, c, uc = PI.ragged_inputs(configs.TINY_UNET, 1, 2, 8, 8, 77, 77)
    xd, td, cd, ud = x.to(DEV), t.to(DEV), c.to(DEV), uc.to(DEV)
    a = net.forward_cfg_pair(xd, td, torch.cat([cd, ud]), single_t=True)
    b = net.forward_cfg_pair(xd, td, (cd, ud), single_t=True)
    assert torch.equal(a, b)


# ---- 3. three sampling steps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DDIM_Gaussian", "DDIM", "UniPC"])
def test_three_steps_on_a_ragged_pair_match_the_two_forwards_loop(tiny, name, monkeypatch):
    net, sd, betas = tiny
    dev = torch.device(DEV)
    _, _, c, uc = PI.ragged_inputs(configs.TINY_UNET, 1, 2, 8, 8, 154, 77)
    c, uc = c.to(dev), uc.to(dev)
    # "DDIM" takes its timesteps as range(0, 1000, 1000 // S) + 1 (ddim/sampler.py make_schedule): S = 3 gives a fourth entry, 1000, past
    # the schedule's end, in the reference as here — no three-step DDIM run exists.  Its case runs the next count that does, 4 steps,
    # at the same gate (one more step of accumulated difference, not one fewer).
    steps = 4 if name == "DDIM" else 3

    def run():
        smp = samplers.Txt2VideoSampler(net, dev, betas=betas, sampler_name=name)
        smp.progress = False
        _, noise, shape = smp.get_noise(1, 4, 2, 64, 64, seed=1234)
        return smp.sample_loop(steps=steps, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=shape, noise=noise,
                               guidance_scale=9.0, eta=0.0, sampler_name=name).float().cpu()

    net._programs.clear()
    pair = run()
    assert [kk[:5] for kk in net._programs] == [(2, 2, 8, 8, (154, 77))]          # one program, both roles
    monkeypatch.delattr(U.UNetSD, "forward_cfg_pair")          # the same loop, two forwards per step (the path of a model without the pair entry)
    net._programs.clear()
    two = run()
    assert sorted(kk[:5] for kk in net._programs) == [(1, 2, 8, 8, 77), (1, 2, 8, 8, 154)]
    r = rel_l2(pair, two)
    print(f"{name}: pair program vs two forwards, {steps} steps: {r:.3e}")
    assert torch.isfinite(pair).all() and r < 3e-3, r


# ---- 4. the emphasis op ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("shape", PI.EMPHASIS_SHAPES)
def test_emphasis_op(shape, dt):
    z, m = PI.emphasis_inputs(*shape)
    rows, W = shape[0] * shape[1], shape[2]
    P = Program("emphasis")
    P.emphasis("e", Buf(Ref("ext", 1), rows, W, W, dt), Ref("ext", 2), Buf(Ref("ext", 3), rows, W, W, "f32"))
    host = PromptInterp(P, {}, poison=False)
    zin = z.half() if dt == "f16" else z

    def run(mult):
        return _run(P, host, {1: zin, 2: mult, 3: torch.full(shape, float("nan"))})[1][3]

    out, again = run(m), run(m)
    e = PI.max_rel(out, PI.emphasis_ref64(zin.float(), m))
    print(f"emphasis {shape} {dt}: max relative error {e / 2.0 ** -24:.2f} x 2^-24")
    assert e <= PI.EMPHASIS_GATE
    assert torch.equal(out, again)
    assert torch.equal(run(torch.ones_like(m)), zin.float())           # the ratio is exactly 1: the plain cast


# ---- 5. the embedder end to end -----------------------------------------------------------------------------------------------------------
def test_embedder_emphasis_and_break_end_to_end():
    model = _seed_params(TE.OpenClipTextModel(**TINY), 8)
    emb = TE.FrozenOpenCLIPEmbedder(model=model, layer="penultimate", tokenizer=PI.ToyTokenizer(), device=DEV, enable_emphasis=True,
                                    comma_padding_backtrack=20)
    k = PI.key(PI.PROMPTS.index(PI.EMBEDDER_PROMPT), True, 20)
    tokens, mult = torch.from_numpy(GOLD[k + "_tokens"]).long(), torch.from_numpy(GOLD[k + "_mult"]).float()
    z = emb([PI.EMBEDDER_PROMPT]).cpu()
    assert z.shape == (1, 2 * 77, 128) and tokens.shape == (2, 77)
    want = []
    for i in range(tokens.shape[0]):              # a chunk per call; what follows the first <end> is padding (clip_hardcode.py:408-411)
        tk = tokens[i:i + 1].clone()
        tk[0, tk[0].tolist().index(PI.END_ID) + 1:] = 0
        want.append(tp.clip_process_tokens(tp.clip_text_forward(model.state_dict(), tk, heads=2, layers=2), mult[i:i + 1]))
    r = rel_l2(z, torch.cat(want, dim=1))
    print(f"embedder end to end: {r:.3e}")
    assert r < 3e-3
    plain = TE.FrozenOpenCLIPEmbedder(model=model, layer="penultimate", tokenizer=PI.ToyTokenizer(), device=DEV)([PI.EMBEDDER_PROMPT]).cpu()
    assert plain.shape[1] == 77 and rel_l2(plain, z[:, :77]) > 3e-2          # without the options: brackets as text, one chunk
