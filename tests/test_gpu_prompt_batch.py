"""GPU (-m gpu): a batch of different prompts in one pass — ragged text contexts, one key count and one K / V location per sample.
(1) T2V_OP_ATTENTION with a per-sample table against single-role launches of the same kernel, bit for bit, and against the plain and
the two-role record where the table describes their layouts; (2) the tiny UNet on ragged batches of three videos against the oracle,
per sample; (3) three sampling steps of every sampler (four of "DDIM", see tests/test_gpu_prompt_syntax.py) on three different contexts
against each video's own run; (4) refused records launch nothing.  The inputs are those of tests/prompt_batch_inputs.py;
tests/test_prompt_batch_cpu.py proves what they expose."""
import ctypes

import pytest
import torch

import prompt_batch_inputs as PB
import prompt_inputs as PI
from harness import rel_l2
from interp_prompt_batch import PromptBatchInterp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from sd_webui_text2video_amd import unet as U
from sd_webui_text2video_amd.program import BoundProgram, Program, Ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _table(rows):
    return torch.tensor([[int(n), int(r)] for n, r in rows], dtype=torch.int32)


# ---- 1. the attention op with a per-sample table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", PB.LENGTH_LISTS, ids=[str(v) for v in PB.LENGTH_LISTS])
def test_attention_table_equals_single_role_launches(lens):
    heads, nq, F, D, GUARD = PB.HEADS, PB.NQ, PB.FRAMES, PB.HEAD_DIM, PB.GUARD
    inner, ld = heads * D, 2 * heads * D
    ls, starts = PB.flat(lens)
    B, total = len(ls), sum(ls)
    per = F * nq                                      # query / output rows of one outer sample
    P = Program("attention table")
    q = P.alloc(B * per, inner, "f16")
    kv = P.alloc(GUARD + total + GUARD, ld, "f16")
    outs = [P.alloc(B * per, inner, "f16") for _ in range(6)]
    rows = kv.row_slice(GUARD, GUARD + total)
    k1, v1 = rows.col_slice(0, inner), rows.col_slice(inner, ld)
    common = dict(nq=nq, heads=heads, b_inner=F, q_strides=(inner, per * inner, nq * inner), o_strides=(inner, per * inner, nq * inner),
                  scale=D ** -0.5)
    tables = {}

    def tab(name, lens_, starts_):
        tables[name] = _table(zip(lens_, starts_))
        return (Ref("weight", 0, name), list(lens_), list(starts_))

    # [0] every sample in one launch
    P.attention("table", q.ref, k1.ref, v1.ref, outs[0].ref, nk=max(ls), b_outer=B, kv_strides=(ld, 0, 0), table=tab("t.all", ls, starts), **common)
    # [1] each sample as a plain launch of its own (no table, no second role), on the same data
    for s, (n, r) in enumerate(zip(ls, starts)):
        ks, vs = k1.row_slice(r, r + n), v1.row_slice(r, r + n)
        P.attention(f"single.{s}", q.row_slice(s * per, (s + 1) * per).ref, ks.ref, vs.ref, outs[1].row_slice(s * per, (s + 1) * per).ref,
                    nk=n, b_outer=1, kv_strides=(ld, 0, 0), **common)
    # [2] / [3] a table that describes a uniform layout = the plain record
    L0 = ls[0]
    Vu = min(B, total // L0)
    P.attention("uniform.table", q.ref, k1.ref, v1.ref, outs[2].ref, nk=L0, b_outer=Vu, kv_strides=(ld, 0, 0),
                table=tab("t.uniform", [L0] * Vu, [s * L0 for s in range(Vu)]), **common)
    P.attention("uniform.plain", q.ref, k1.ref, v1.ref, outs[3].ref, nk=L0, b_outer=Vu, kv_strides=(ld, L0 * ld, 0), **common)
    # [4] / [5] a table that describes the two-role layout (Vp samples of Lc keys, then Vp samples of Lu keys) = the two-role record
    Lc = ls[0]
    Lu = next((n for n in ls if n != Lc), Lc)
    Vp = min(B // 2, total // (Lc + Lu))
    assert Vp >= 1 and Lu != Lc
    k2, v2 = k1.row_slice(Vp * Lc, Vp * (Lc + Lu)), v1.row_slice(Vp * Lc, Vp * (Lc + Lu))
    P.attention("pair.table", q.ref, k1.ref, v1.ref, outs[4].ref, nk=max(Lc, Lu), b_outer=2 * Vp, kv_strides=(ld, 0, 0),
                table=tab("t.pair", [Lc] * Vp + [Lu] * Vp, [s * Lc for s in range(Vp)] + [Vp * Lc + s * Lu for s in range(Vp)]), **common)
    P.attention("pair.roles", q.ref, k1.ref, v1.ref, outs[5].ref, nk=Lc, b_outer=2 * Vp, kv_strides=(ld, Lc * ld, 0),
                alt=(Vp, Lu, k2.ref, v2.ref, Lu * ld), **common)
    assert all(op.i[22:25] == [0, 0, 0] and op.p[7].space == "null" for op in P.ops if "table" not in op.name)
    assert all(op.i[19:22] == [0, 0, 0] and op.i[22] == op.i[3] for op in P.ops if "table" in op.name)

    host = PromptBatchInterp(P, tables, poison=False)
    qv, kvv = PB.attention_inputs(lens)
    host.mat(q.ref, q.rows, inner, inner, torch.float16, {}).copy_(qv)
    host.mat(kv.ref, kv.rows, ld, ld, torch.float16, {}).copy_(kvv)
    for o in outs:
        host.mat(o.ref, o.rows, inner, inner, torch.float16, {}).fill_(float("nan"))
    dev = torch.device(DEV)
    arena = host.arena.to(dev)
    tabs_gpu = {k: v.to(dev) for k, v in tables.items()}
    bound = BoundProgram(P, arena.data_ptr(), {k: v.data_ptr() for k, v in tabs_gpu.items()})
    bound.run({}, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    L.async_status()
    got = PromptBatchInterp(P, {}, poison=False)
    got.arena = arena.cpu()
    rd = lambda b, n=None: got.mat(b.ref, b.rows if n is None else n, inner, inner, torch.float16, {})
    table, single = rd(outs[0]), rd(outs[1])
    assert torch.isfinite(table.float()).all() and torch.isfinite(single.float()).all()
    for s in range(B):
        assert torch.equal(table[s * per:(s + 1) * per], single[s * per:(s + 1) * per]), f"sample {s} ({ls[s]} keys at row {starts[s]})"
    assert torch.isfinite(rd(outs[3], Vu * per).float()).all() and torch.equal(rd(outs[2], Vu * per), rd(outs[3], Vu * per)), "uniform layout"
    assert torch.isfinite(rd(outs[5], 2 * Vp * per).float()).all() and torch.equal(rd(outs[4], 2 * Vp * per), rd(outs[5], 2 * Vp * per)), "two-role layout"
    # the interpreter's reading of the record agrees with the kernel (fp16 output rounding + fp16 probabilities), and both with float64
    host.run({}, ops=P.ops[:1])
    want = host.mat(outs[0].ref, outs[0].rows, inner, inner, torch.float16, {})
    r_i, r_64 = rel_l2(table.float(), want.float()), rel_l2(table.float(), PB.attention_ref64(qv, kvv, list(zip(ls, starts))))
    print(f"attention table {lens}: vs interpreter {r_i:.3e}, vs float64 {r_64:.3e}")
    assert r_i < PB.INTERP_GATE and r_64 < PB.INTERP_GATE


# ---- 2. the tiny UNet on ragged batches -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    sd = synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, sd, betas


_REFS = {}


def _sample_refs(sd, geom, lens):
    """The oracle's eps of every sample alone, computed once per case and shared."""
    k = (geom, lens)
    if k not in _REFS:
        cfg = configs.TINY_UNET
        x, t, cs, us = PB.unet_inputs(cfg, geom, lens)
        V = len(cs)
        _REFS[k] = (x, t, cs, us, [tp.unet_forward(sd, cfg, x[b % V: b % V + 1], t, ctx) for b, ctx in enumerate(cs + us)])
    return _REFS[k]


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("geom,lens", PB.UNET_CASES)
def test_tiny_unet_ragged_batch(tiny, geom, lens, share, monkeypatch):
    net, sd, _ = tiny
    monkeypatch.setattr(net, "share_cfg_prefix", share, raising=False)
    x, t, cs, us, refs = _sample_refs(sd, geom, lens)
    V, (ls, _) = len(cs), PB.flat(lens)
    xd, td, cd, ud = x.to(DEV), t.to(DEV), [c.to(DEV) for c in cs], [u.to(DEV)[0] for u in us]       # ([1, L, ctx] and [L, ctx] entries)
    token = ("ragged batch", geom, lens, share)
    eps = net.forward_cfg_pair(xd, td, (cd, ud), context_token=token, single_t=True)
    again = net.forward_cfg_pair(xd, td, (cd, ud), context_token=token, single_t=True)          # the step-invariant prologue is skipped
    assert eps.shape == (2 * V, 4) + geom and torch.equal(eps, again)
    errs = [rel_l2(eps[b:b + 1].float().cpu(), ref) for b, ref in enumerate(refs)]
    print(f"ragged batch {geom} {lens} share={share}: " + " ".join(f"{e:.3e}" for e in errs))
    assert max(errs) < PI.UNET_GATE, errs
    comp = next(cc for kk, cc in net._programs.items() if kk[:5] == (2 * V,) + geom + (tuple(ls),))
    with_table = [op for op in comp.prog.ops if op.kind == L.OP_ATTENTION and op.i[22]]
    assert with_table and all(op.i[22] == 2 * V and op.i[23] == max(ls) and op.i[24] == sum(ls) for op in with_table)


def test_uniform_batch_is_todays_program(tiny):
    net, sd, _ = tiny
    geom = (2, 8, 8)
    x, t, cs, us = PB.unet_inputs(configs.TINY_UNET, geom, ((77, 77, 77), (154, 154, 154)))
    xd, td, cd, ud = x.to(DEV), t.to(DEV), [c.to(DEV) for c in cs], [u.to(DEV) for u in us]
    net._programs.clear()
    a = net.forward_cfg_pair(xd, td, (torch.cat(cd), torch.cat(ud)), single_t=True)
    keys = list(net._programs)
    assert [kk[:5] for kk in keys] == [(6,) + geom + ((77, 154),)]
    b = net.forward_cfg_pair(xd, td, (cd, ud), single_t=True)
    assert list(net._programs) == keys and torch.equal(a, b)                      # the same compiled program, the same bits
    assert not any(op.i[22] for op in net._programs[keys[0]].prog.ops if op.kind == L.OP_ATTENTION)
    same = net.forward_cfg_pair(xd, td, (cd, [u[:, :77] for u in ud]), single_t=True)          # one length everywhere: the plain batch
    assert torch.equal(same, net.forward_cfg_pair(xd, td, torch.cat(cd + [u[:, :77] for u in ud]), single_t=True))
    assert {kk[4] for kk in net._programs if kk[:4] == (6,) + geom} == {77, (77, 154)}


# ---- 3. three sampling steps on three different contexts ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DDIM_Gaussian", "DDIM", "UniPC"])
def test_three_steps_on_a_batch_of_prompts_match_single_video_runs(tiny, name):
    net, sd, betas = tiny
    dev = torch.device(DEV)
    geom, lens = PB.UNET_CASES[0]
    _, _, cs, us = PB.unet_inputs(configs.TINY_UNET, geom, lens)
    cs, us = [c.to(dev) for c in cs], [u.to(dev) for u in us]
    seeds = [1234, 77, 4321]
    steps = 4 if name == "DDIM" else 3           # no three-step "DDIM" schedule exists (tests/test_gpu_prompt_syntax.py)

    def run(c, uc, seed_list):
        smp = samplers.Txt2VideoSampler(net, dev, betas=betas, sampler_name=name)
        smp.progress = False
        noises = [smp.get_noise(1, 4, geom[0], 8 * geom[1], 8 * geom[2], seed=s)[1] for s in seed_list]
        noise = torch.cat(noises, dim=0)
        return smp.sample_loop(steps=steps, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=len(seed_list),
                               shape=tuple(noise.shape), noise=noise, guidance_scale=9.0, eta=0.0, sampler_name=name).float().cpu()

    net._programs.clear()
    batch = run(cs, us, seeds)
    ls, _ = PB.flat(lens)
    assert [kk[:5] for kk in net._programs] == [(6,) + geom + (tuple(ls),)]          # exactly one program for the whole batch
    assert batch.shape[0] == 3 and torch.isfinite(batch).all()
    for v in range(3):
        single = run(cs[v], us[v], [seeds[v]])
        r = rel_l2(batch[v:v + 1], single)
        print(f"{name}: video {v} of the batch vs its own run, {steps} steps: {r:.3e}")
        assert r < 3e-3, (v, r)


# ---- 4. refused records launch nothing --------------------------------------------------------------------------------------------------
def test_refused_table_records_launch_nothing():
    dev = torch.device(DEV)
    lib = L.load()
    heads, nq, D, B, n = 2, 64, 64, 2, 64
    inner = heads * D
    q = torch.randn(B * nq, inner, device=dev).half()
    kv = torch.randn(B * n, 2 * inner, device=dev).half()
    tab = _table([(n, 0), (n, n)]).to(dev)
    FILL = 7.0
    out = torch.full((B * nq, inner), FILL, device=dev, dtype=torch.float16)
    scratch = torch.zeros(B * heads * 64 * 64, device=dev, dtype=torch.float16)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch(i_over, p_over):
        op = L.T2VOp()
        op.kind, op.f[0] = L.OP_ATTENTION, D ** -0.5
        fields = {0: nq, 1: n, 2: heads, 3: B, 4: 1, 5: inner, 6: nq * inner, 8: 2 * inner, 11: inner, 12: nq * inner, 14: D,
                  22: B, 23: n, 24: B * n, **i_over}
        ptrs = {0: q.data_ptr(), 1: kv.data_ptr(), 2: kv.data_ptr() + 2 * inner, 3: out.data_ptr(), 7: tab.data_ptr(), **p_over}
        for k, v in fields.items():
            op.i[k] = v
        for k, v in ptrs.items():
            op.p[k] = v
        rc = lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, stream)
        msg = lib.t2v_last_error()
        torch.cuda.synchronize()
        return rc, msg

    refused = [({}, {7: 0}, b"null table"),
               ({19: 1, 20: n, 21: n * 2 * inner}, {4: kv.data_ptr(), 5: kv.data_ptr()}, b"second role"),
               ({15: 1}, {}, b"causal"),
               ({17: 64}, {6: scratch.data_ptr()}, b"scratch"),
               ({22: B + 1}, {}, b"batch_outer"),
               ({23: 0}, {}, b"largest key count"),
               ({22: 0, 23: 0, 24: 0}, {}, b"without its fields")]
    for i_over, p_over, why in refused:
        rc, msg = launch(i_over, p_over)
        assert rc == -1 and b"table" in msg and why in msg, (i_over, msg)
        assert bool((out == FILL).all()), (i_over, "a refused record wrote its output")
    rc, msg = launch({}, {})                     # the record itself is a good one
    assert rc == 0, msg
    assert torch.isfinite(out.float()).all() and not bool((out == FILL).any())
