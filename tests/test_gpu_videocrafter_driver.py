"""GPU (-m gpu): the VideoCrafter driver seam.  Form 1 of T2V_OP_TO_UINT8 bit for bit against bytes of the REAL reference's torch_to_np
(tests/golden/make_golden_frames.py), its refusals, `decode_first_stage_uint8` against the float route, the one-pass route of
`process_videocrafter` against its loop route (exactly, on an elementwise model) and against goldens of the reference's own sampler run
video by video (tests/golden/make_golden_driver.py), and the entry points.  Measured figures: profiles/videocrafter_driver.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frames_inputs as FI
from harness import rel_l2
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import videocrafter as VC

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
GUARD = 256

# One pass (batch of 3) against the reference's per-video goldens, rel-L2 per video.  The gate is the LARGEST error the single-video path
# (DDIMSampler.sample per video with noise_gen, untouched here) has against the same goldens, x 1.5: the batch changes only the GEMM
# tiling, so its error is another draw of the same rounding noise, and the three single-video errors show that spread.
# Measured on the MI355X (profiles/videocrafter_driver.txt): single-video 1.860e-3, 1.933e-3, 1.405e-3 -> gate 2.900e-3
# (the one pass measured 1.842e-3, 1.884e-3, 1.412e-3).
SINGLE_VIDEO_MAX = 1.933e-3
ONE_PASS_GATE = 1.5 * SINGLE_VIDEO_MAX


@pytest.fixture(scope="module")
def designed():
    z = np.load(os.path.join(GOLD, "torch_to_np_designed.npz"))
    d = {k: torch.from_numpy(z[k].copy()) for k in ("f32_in", "f32_out", "f32_half_out", "f16_out")}
    d["f16_in"] = torch.from_numpy(z["f16_in"].copy().view(np.float16))
    return d


def _record(src, out, shape, strides, half, form=1, bgr=0):
    NI, C, Fr, H, W = shape
    si, sc, sf, sy, sx = strides
    op = L.T2VOp()
    op.kind = L.OP_TO_UINT8
    vals = [NI, C, Fr, H, W, L.F16 if src.dtype == torch.float16 else L.F32, int(half), bgr, si & 0xFFFFFFFF, si >> 32, sc,
            sf & 0xFFFFFFFF, sf >> 32, sy, sx, form]
    for k, v in enumerate(vals):
        op.i[k] = v - (1 << 32) if v >= (1 << 31) else v
    op.p[0], op.p[1] = src.data_ptr(), out.data_ptr()
    return op


def _launch(op):
    return L.load().t2v_run_ops(ctypes.byref(op), 1, None, 0, ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream))


def _run_form1(video, half, tokens):
    """video [NI, C, F, H, W] (host) -> the kernel's bytes [NI, F, H, W, C] (host), the guard bytes around the output checked."""
    NI, C, Fr, H, W = video.shape
    if tokens:
        src = torch.full((NI * Fr * H * W, 4), float("nan"), dtype=video.dtype)
        src[:, :C] = video.permute(0, 2, 3, 4, 1).reshape(-1, C)
        strides = (Fr * H * W * 4, 1, H * W * 4, W * 4, 4)
    else:
        src, strides = video.contiguous(), (C * Fr * H * W, Fr * H * W, H * W, W, 1)
    n = video.numel()
    buf = torch.full((n + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    src = src.to(DEV)
    assert _launch(_record(src, buf[GUARD:], tuple(video.shape), strides, half)) == 0, L.load().t2v_last_error()
    torch.cuda.synchronize()
    host = buf.cpu()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + n:] == 0xA5).all(), "bytes outside the output were written"
    return host[GUARD:GUARD + n].view(NI, Fr, H, W, C)


KINDS = [("f32", "f32_in", "f32_out", False), ("f32-half", "f32_in", "f32_half_out", True), ("f16", "f16_in", "f16_out", False),
         ("f16-half", "f16_in", "f16_out", True)]


@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("tokens", [True, False], ids=["tokens-ld4", "ncfhw"])
def test_form1_op_matches_the_reference_bytes(designed, kind, tokens):
    """All four instantiations (TIN x HALF), both layouts, NI = 2, C = 3, H = 3, W = 5 and as many frames as hold the inputs: 706 frames =
    21 180 pixels for the fp16 table (83 workgroups, the last ragged), 16 frames = 480 pixels for the fp32 one (2, the second ragged)."""
    _, kin, kout, half = kind
    video, _ = FI.as_video(designed[kin], FI.FILL)
    want = FI.want_video(designed[kout], FI.FILL_BYTE, video.shape)
    got = _run_form1(video, half, tokens)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:5].tolist())
    if not tokens:                                                    # the stand-alone launch is the same record
        dev = VC.torch_to_np_device((video.half() if half else video).to(DEV))
        assert dev.dtype == torch.uint8 and torch.equal(dev.cpu(), want)


def test_form1_grid_stride_second_trip(designed):
    """2 097 452 pixels: grid_for caps the grid at 8192 x 256 threads, so the last 300 pixels are a second trip of the grid-stride loop.
    The designed fp32 inputs repeat with period 1305 (no multiple of 3), so those pixels carry boundary values of their own."""
    W = 2097152 + 300
    x, b = designed["f32_in"], designed["f32_out"]
    reps = -(-3 * W // x.numel())
    video = x.repeat(reps)[:3 * W].view(1, 3, 1, 1, W)
    want = b.repeat(reps)[:3 * W].view(1, 3, 1, 1, W).permute(0, 2, 3, 4, 1).contiguous()
    got = _run_form1(video, False, False)
    assert torch.equal(got, want)
    assert len(set(want[0, 0, 0, 2097152:].reshape(-1).tolist())) > 100          # the second trip is not one value


def test_form1_refusals_launch_nothing():
    shape = (1, 3, 2, 3, 5)
    src = torch.zeros(shape, device=DEV)
    out = torch.full((90,), 0xA5, dtype=torch.uint8, device=DEV)
    strides = (90, 30, 15, 5, 1)
    for kw in (dict(form=2), dict(form=-1), dict(form=1, bgr=1)):
        assert _launch(_record(src, out, shape, strides, False, **kw)) == -1, kw          # T2V_ERR_BAD_ARG
        assert b"uint8" in L.load().t2v_last_error(), kw
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    assert _launch(_record(src, out, shape, strides, False, form=0, bgr=1)) == 0           # form 0 keeps its bgr
    torch.cuda.synchronize()
    assert (out == 127).all()
    with pytest.raises(L.T2VError):
        VC.torch_to_np_device(torch.zeros(shape))


# ---- the decoder route ---------------------------------------------------------------------------------------------------------------------
def _tiny_ld():
    ld = VC.LatentDiffusion(configs.TINY_LVDM_UNET, dict(ddconfig=configs.TINY_VAE_DDCONFIG, embed_dim=4), image_size=[8, 8],
                            video_length=5, init_weights=False, **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    ld.first_stage_model.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.first_stage_model), seed=3), strict=True)
    return ld


@pytest.fixture(scope="module")
def tiny_ld():
    return _tiny_ld().to(DEV)


@pytest.fixture(scope="module")
def tiny_ld16():
    return _tiny_ld().half().to(DEV)


class _Enc:            # stands in for FrozenCLIPEmbedder (outside the hot path)
    def encode(self, prompts):
        ctx = FI.driver_inputs()[0].to(DEV)
        return torch.cat([ctx[0:1] if p == "a cat" else ctx[1:2] for p in prompts])


@pytest.mark.parametrize("which", ["fp32", "fp16"])
def test_decode_first_stage_uint8_equals_the_float_route(tiny_ld, tiny_ld16, which):
    ld = tiny_ld if which == "fp32" else tiny_ld16
    z = (torch.randn(1, 4, 5, 8, 8, generator=torch.Generator().manual_seed(21)) * 3.0 * ld.scale_factor).to(DEV)
    for bs in (None, 1, 2):
        vid = ld.decode_first_stage(z, decode_bs=bs, return_cpu=False)
        assert vid.dtype == (torch.float32 if which == "fp32" else torch.float16)
        want = VC.torch_to_np(vid).numpy()
        got = ld.decode_first_stage_uint8(z, decode_bs=bs)
        assert got.dtype == torch.uint8 and got.device.type == "cpu" and got.shape == (1, 5, 64, 64, 3)
        assert np.array_equal(got.numpy(), want), (which, bs, int((got.numpy() != want).sum()))
        dev = ld.decode_first_stage_uint8(z, decode_bs=bs, to_host=False)
        assert dev.is_cuda and torch.equal(dev.cpu(), got)
        assert torch.equal(VC.torch_to_np_device(vid).cpu(), got)          # the stand-alone launch on the float video
    assert len(set(want.reshape(-1).tolist())) > 100 and (want == 0).any() and (want == 255).any()
    # two videos: the frames of both in one output, video after video
    z2 = torch.cat([z, z.flip(2)])
    got2 = ld.decode_first_stage_uint8(z2, decode_bs=3)
    assert got2.shape == (2, 5, 64, 64, 3)
    assert np.array_equal(got2.numpy(), VC.torch_to_np(ld.decode_first_stage(z2, decode_bs=3, return_cpu=False)).numpy())


# ---- one pass against the loop ---------------------------------------------------------------------------------------------------------------
def _eps_standin(x, t, c, **kw):
    """Elementwise stand-in for apply_model: x may be the one x_t of a [cond | uncond] pair (t and c then hold both halves)."""
    if x.shape[0] != t.shape[0]:
        x = torch.cat([x, x])
    s = c.float().mean(dim=(1, 2)).view(-1, 1, 1, 1, 1)
    return 0.3 * x + 0.1 * torch.sin(x) + 0.05 * s + 1e-4 * t.float().view(-1, 1, 1, 1, 1)


def _args(model, **kw):
    return {**dict(model=model, prompt="a cat", n_prompt="", steps=FI.STEPS, frames=5, seed=FI.SEED, cfg_scale=FI.CFG, eta=FI.ETA), **kw}


def test_one_pass_equals_the_loop_on_an_elementwise_model(tiny_ld, monkeypatch):
    ld, V_ = tiny_ld, FI.VIDEOS
    monkeypatch.setattr(ld, "cond_stage_model", _Enc())
    monkeypatch.setattr(ld, "apply_model", _eps_standin)
    latents = []
    real = ld.decode_first_stage_uint8
    monkeypatch.setattr(ld, "decode_first_stage_uint8", lambda z, **k: (latents.append(z.clone()), real(z, **k))[1])
    torch.cuda.manual_seed(7)
    loop = VC.process_videocrafter(_args(ld, batch_count=V_, one_pass=False))
    torch.cuda.manual_seed(7)
    one = VC.process_videocrafter(_args(ld, batch_count=V_))
    assert [tuple(z.shape) for z in latents] == [(1, 4, 5, 8, 8)] * V_ + [(V_, 4, 5, 8, 8)]
    for v in range(V_):
        assert torch.equal(latents[V_][v:v + 1], latents[v]), v
        assert np.array_equal(one[v], loop[v])
    assert not torch.equal(latents[0], latents[1])
    # the streams are per video: equal start latents, video 1 differs from video 0 when the seeds differ and equals it when seed == -1
    ctx, x_T = FI.driver_inputs()
    kw = dict(S=FI.STEPS, conditioning={"c_crossattn": [ctx[0:1].repeat(2, 1, 1).to(DEV)]}, batch_size=2, shape=list(FI.SHAPE), verbose=False,
              eta=FI.ETA, x_T=x_T[0:1].repeat(2, 1, 1, 1, 1).to(DEV), unconditional_guidance_scale=FI.CFG,
              unconditional_conditioning={"c_crossattn": [ctx[1:2].repeat(2, 1, 1).to(DEV)]})
    smp = VC.DDIMSampler(ld)
    smp.noise_gens = [torch.Generator().manual_seed(FI.SEED), torch.Generator().manual_seed(FI.SEED + 1)]
    a, _ = smp.sample(**kw)
    assert not torch.equal(a[0], a[1])
    smp.noise_gens = [torch.Generator().manual_seed(-1), torch.Generator().manual_seed(-1)]
    b, _ = smp.sample(**kw)
    assert torch.equal(b[0], b[1])
    smp.noise_gens = smp.noise_gens[:1]
    with pytest.raises(ValueError, match="one per video"):
        smp.sample(**kw)


def test_one_pass_on_the_real_unet_matches_the_reference_per_video(tiny_ld):
    ld, V_ = tiny_ld, FI.VIDEOS
    gold = np.load(os.path.join(GOLD, "lvdm_driver_tiny.npz"))
    ctx, x_T = FI.driver_inputs()
    assert np.array_equal(gold["x_T"], x_T.numpy()) and int(gold["seed"]) == FI.SEED
    want = torch.from_numpy(gold["out"])

    def kw(n, xt):
        return dict(S=FI.STEPS, conditioning={"c_crossattn": [ctx[0:1].repeat(n, 1, 1).to(DEV)]}, batch_size=n, shape=list(FI.SHAPE),
                    verbose=False, eta=FI.ETA, x_T=xt.to(DEV), unconditional_guidance_scale=FI.CFG,
                    unconditional_conditioning={"c_crossattn": [ctx[1:2].repeat(n, 1, 1).to(DEV)]})
    smp = VC.DDIMSampler(ld)
    single = []
    for v in range(V_):               # the single-video path: what the loop route runs
        smp.noise_gen.manual_seed(FI.SEED + v)
        x, _ = smp.sample(**kw(1, x_T[v:v + 1]))
        single.append(rel_l2(x.cpu()[0], want[v]))
    smp.noise_gens = [torch.Generator().manual_seed(FI.SEED + v) for v in range(V_)]
    x, _ = smp.sample(**kw(V_, x_T))
    batch = [rel_l2(x.cpu()[v], want[v]) for v in range(V_)]
    print("single-video rel-L2 vs the reference goldens: " + ", ".join(f"{r:.3e}" for r in single))
    print("one pass (batch of 3) rel-L2 per video:       " + ", ".join(f"{r:.3e}" for r in batch) + f"   gate {ONE_PASS_GATE:.3e}")
    assert rel_l2(want[1], want[0]) > 0.5                             # the goldens are three different videos
    assert all(r < ONE_PASS_GATE for r in batch), (batch, single)


def test_entry_points(tiny_ld, monkeypatch):
    ld = tiny_ld
    monkeypatch.setattr(ld, "cond_stage_model", _Enc())
    smp = VC.DDIMSampler(ld)
    kw = dict(sampler=smp, ddim_steps=FI.STEPS, eta=FI.ETA, cfg_scale=FI.CFG, num_frames=5)
    for bs in (1, 2, None):
        outs = []
        for u8 in (False, True):
            smp.noise_gen.manual_seed(5)
            torch.cuda.manual_seed(3)
            outs.append(VC.sample_text2video(ld, "a cat", "", 1, 1, decode_frame_bs=bs, device_uint8=u8, **kw))
        assert outs[1].shape == (1, 5, 64, 64, 3) and outs[1].dtype == np.uint8 and np.array_equal(outs[0], outs[1]), bs
    torch.cuda.manual_seed(3)
    vids = VC.process_videocrafter(_args(ld, batch_count=2))
    assert len(vids) == 2 and all(v.shape == (5, 64, 64, 3) and v.dtype == np.uint8 for v in vids)
    assert not np.array_equal(vids[0], vids[1])
