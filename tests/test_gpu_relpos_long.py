"""GPU (-m gpu): VideoCrafter clips longer than 32 frames — the relative-position attention kernel of clips of any length
(RELPOS_ATTN i[17] = 3, csrc/attention.hip relpos_long_kernel) against the explicit formula, against the VALU kernel at
<= 32 frames, and the UNet / sampler / entry point at 40 and 48 frames against fixtures of the reference
(tests/golden/make_golden_long.py)."""
import os

import numpy as np
import pytest
import torch

from harness import fill, read, rel_l2, run_both
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import packing as pk
from sd_webui_text2video_amd import videocrafter as VC
from sd_webui_text2video_amd.program import Program, Ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def _relpos_case(D, T, Tq, off, R, lo, sel, seed, hw=5, b=2, heads=2):
    """One RELPOS_ATTN op over b x hw pixels of a T-frame clip (queries = frames [off, off + Tq)), output poisoned with NaN first.
    Returns (gpu output [b, Tq, hw, heads, D] fp32, low-order image or None, explicit-formula reference, op)."""
    inner = heads * D
    g = torch.Generator().manual_seed(seed)
    # fp16-representable tables: the kernel stages them as fp16, the formula reads them as fp32
    w = {"ek": (0.3 * torch.randn(2 * R + 1, D, generator=g)).half().float(), "ev": (0.3 * torch.randn(2 * R + 1, D, generator=g)).half().float()}
    w["ekL"], w["evL"] = pk.relpos_table_long(w["ek"], False), pk.relpos_table_long(w["ev"], True)
    P = Program()
    q, kv = P.alloc(b * Tq * hw, inner, "f16"), P.alloc(b * T * hw, 2 * inner, "f16")
    o = P.alloc(b * Tq * hw, 2 * inner if lo else inner, "f16")
    op = P.attention("a", q.ref, kv.col_slice(0, inner).ref, kv.col_slice(inner, 2 * inner).ref, o.ref, nq=Tq, nk=T, heads=heads,
                     b_outer=b, b_inner=hw, q_strides=(hw * inner, Tq * hw * inner, inner), kv_strides=(hw * kv.ld, T * hw * kv.ld, kv.ld),
                     o_strides=(hw * o.ld, Tq * hw * o.ld, o.ld), scale=D ** -0.5, head_dim=D, rel_k=Ref("weight", 0, "ek"),
                     rel_v=Ref("weight", 0, "ev"), max_rel=R, q_offset=off, relpos_mfma=sel, lo_off=inner if lo else 0,
                     rel_k_long=Ref("weight", 0, "ekL"), rel_vT_long=Ref("weight", 0, "evL"))

    def init(it):
        fill(it, q, g)
        fill(it, kv, g)
        it.mat(o.ref, o.rows, o.cols, o.ld, torch.float16, {}).fill_(float("nan"))
    it, got, _, _ = run_both(P, w, {}, init)
    qf = read(it, q).float().view(b, Tq, hw, heads, D)
    kvf = read(it, kv).float().view(b, T, hw, 2, heads, D)
    kf, vf = kvf[:, :, :, 0], kvf[:, :, :, 1]
    idx = (torch.arange(T)[None, :] - (torch.arange(Tq)[:, None] + off)).clamp(-R, R) + R              # [Tq, T]
    sim = (torch.einsum("btphd,bsphd->bphts", qf, kf) + torch.einsum("btphd,tsd->bphts", qf, w["ek"][idx])) * D ** -0.5
    p = sim.softmax(dim=-1)
    ref = torch.einsum("bphts,bsphd->btphd", p, vf) + torch.einsum("bphts,tsd->btphd", p, w["ev"][idx])
    out = read(got, o).float().view(b, Tq, hw, -1)
    hi = out[..., :inner].reshape(b, Tq, hw, heads, D)
    low = out[..., inner:].reshape(b, Tq, hw, heads, D) if lo else None
    return hi, low, ref, op


LONG_CASES = [(40, 33, 2), (40, 250, 16), (40, 125, 249), (64, 48, 16), (64, 100, 2), (64, 64, 63),
              (80, 64, 2), (80, 125, 16), (80, 33, 40), (160, 250, 2), (160, 100, 99), (160, 48, 16)]


@pytest.mark.parametrize("D,T,R", LONG_CASES)
def test_long_clip_relpos_attention_against_explicit_formula(D, T, R):
    """Every head_dim, T in {33, 48, 64, 100, 125, 250}, R clipped hard (2), the released model's 16, and unclipped (>= T - 1);
    ragged hw = 5, b = 2; the low-order output on every other case."""
    lo = (D + T) % 2 == 0
    hi, low, ref, op = _relpos_case(D, T, T, 0, R, lo, None, seed=T + D)
    assert op.i[17] == 3
    assert torch.isfinite(hi).all()
    r = rel_l2(hi, ref)
    assert r < 2e-3, r
    if lo:
        assert torch.isfinite(low).all()
        r2 = rel_l2(hi + low, ref)
        assert r2 < r and r2 < 1e-3, (r, r2)


@pytest.mark.parametrize("D,T,Tq,off,R", [(40, 64, 20, 0, 16), (80, 100, 34, 33, 16), (160, 48, 12, 36, 47), (64, 250, 84, 166, 2),
                                          (40, 40, 14, 14, 16)])
def test_long_clip_relpos_attention_sharded_queries(D, T, Tq, off, R):
    """The T-sharded form (videocrafter.py temporal_attn_sharded): Tq local queries = frames [off, off + Tq) at the start, middle
    and end of the clip, keys = all T frames."""
    hi, _, ref, op = _relpos_case(D, T, Tq, off, R, False, None, seed=7 * T + off)
    assert op.i[17] == 3 and op.i[16] == off
    assert torch.isfinite(hi).all()
    r = rel_l2(hi, ref)
    assert r < 2e-3, r


@pytest.mark.parametrize("T", [17, 24, 32])
def test_long_kernel_and_valu_kernel_agree_up_to_32_frames(T):
    """Forced i[17] = 3 and the VALU kernel (i[17] = 0) on identical inputs, both against the formula (R = 16 and R = 4)."""
    for D, R in ((40, 16), (80, 4)):
        hi3, _, ref, op3 = _relpos_case(D, T, T, 0, R, False, 3, seed=300 + T)
        hi0, _, ref0, op0 = _relpos_case(D, T, T, 0, R, False, 0, seed=300 + T)
        assert op3.i[17] == 3 and op0.i[17] == 0
        assert torch.equal(ref, ref0)
        assert rel_l2(hi3, ref) < 2e-3 and rel_l2(hi0, ref) < 2e-3
        assert rel_l2(hi3, hi0) < 2e-3


def test_released_config_48_frames_matches_reference_golden():
    """configs.LVDM_UNET (head_dim 40 / 80 / 160), 48 frames on a 16x16 latent, t = 500, 77 tokens: fp32 weights against the
    reference's own UNetModel; a .half() run returns fp16 and is finite."""
    gold = torch.from_numpy(np.load(os.path.join(GOLD, "lvdm_48f_16x16.npz"))["unet_eps"])
    net = VC.UNetModel(**configs.LVDM_UNET, init_weights=False)
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    net = net.to(DEV)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, 4, 48, 16, 16, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g)
    out = net(x.to(DEV), torch.tensor([500], device=DEV), context=ctx.to(DEV))
    assert out.shape == (1, 4, 48, 16, 16)
    r = rel_l2(out.float().cpu(), gold)
    assert r < 4e-3, r
    net = net.half()
    out16 = net(x.half().to(DEV), torch.tensor([500], device=DEV), context=ctx.half().to(DEV))
    assert out16.dtype == torch.float16 and torch.isfinite(out16).all()


def _inputs_tiny40():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 40, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 40, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def test_tiny_latent_diffusion_40_frames():
    """Tiny LatentDiffusion at 40 frames: UNet eps and a 4-step DDIM run (CFG 7.5, eta 0.3) against the reference fixtures, and
    sample_text2video end to end."""
    ld = VC.LatentDiffusion(configs.TINY_LVDM_UNET, dict(ddconfig=configs.TINY_VAE_DDCONFIG, embed_dim=4), image_size=[8, 8],
                            video_length=40, init_weights=False, **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    ld.first_stage_model.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.first_stage_model), seed=3), strict=True)
    ld = ld.to(DEV)
    gold = np.load(os.path.join(GOLD, "lvdm_tiny_40f.npz"))
    x, t, ctx, x_T = _inputs_tiny40()
    eps = ld.model.diffusion_model(x.to(DEV), t.to(DEV), context=ctx.to(DEV))
    r = rel_l2(eps.float().cpu(), torch.from_numpy(gold["unet_eps"]))
    assert r < 4e-3, r
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(123)
    x0, _ = smp.sample(S=4, conditioning={"c_crossattn": [ctx[0:1].to(DEV)]}, batch_size=1, shape=list(x_T.shape[1:]),
                       verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning={"c_crossattn": [ctx[1:2].to(DEV)]}, eta=0.3, x_T=x_T.to(DEV))
    r = rel_l2(x0.float().cpu(), torch.from_numpy(gold["ddim_x0"]))
    assert r < 2e-2, r

    class Enc:            # stands in for FrozenCLIPEmbedder (outside the hot path)
        def encode(self, prompts):
            return (ctx[0:1] if prompts[0] == "a cat" else ctx[1:2]).to(DEV).repeat(len(prompts), 1, 1)
    ld.cond_stage_model = Enc()
    smp.noise_gen.manual_seed(5)
    torch.manual_seed(0)
    vids = VC.sample_text2video(ld, "a cat", "", 1, 1, sampler=smp, ddim_steps=4, eta=0.0, cfg_scale=7.5, decode_frame_bs=8,
                                num_frames=40)
    assert vids.shape == (1, 40, 64, 64, 3) and vids.dtype == np.uint8
    assert vids.std() > 0
