"""GPU (-m gpu): the float bicubic mode of T2V_OP_RESAMPLE (i[9] = 1) — the kernel against tests/interp_bicubic.py bit for bit, its
memory discipline, and the opt-in depth path of T2VAdapterDepth (`depth_resize`) end to end on the tiny latent-diffusion fixture.

The constant frame of the end-to-end case.  The reference's formula (interpolate, estimator, interpolate, min-max normalise) divides by
max - min + 1e-7; on a constant frame that is the rounding noise of the interpolation itself.  torch's float32 interpolation of the
constant 5.75 is not constant (its float32 weights do not sum to 1 everywhere), so the float32 evaluation of the formula on the CPU gives
values up to +0.81 in that frame where the exact answer is -1 (measured on the CPU; float64 gives -1 + 2e-8).  The float32 comparison
therefore covers the four non-constant frames, and ALL frames are compared with the same formula in float64; the package's own result on
the constant frame must be exactly -1."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adapter_ref as AR
from interp_bicubic import bicubic_interp
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import videocrafter as VC
from test_bicubic_cpu import SHAPES, IDS, shape_input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP16_SHAPES = [((3, 5, 7), (13, 3)), ((3, 40, 56), (384, 384))]


def bits(t):
    return np.ascontiguousarray(t if isinstance(t, np.ndarray) else t.cpu().numpy()).view(np.int32)


def assert_bit_equal(got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {got.size} values differ, first at {tuple(bad[0])}"


# ---- bit equality with the interpreter ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", SHAPES, ids=IDS)
def test_fp32_input_equals_the_interpreter_bit_for_bit(src, dst):
    x = shape_input(src)
    out = VC.bicubic_resize(x[None].to(DEV), dst)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, src[0]) + dst
    assert_bit_equal(out[0], bicubic_interp(x.numpy(), *dst))


@pytest.mark.parametrize("src,dst", FP16_SHAPES, ids=[IDS[SHAPES.index(s)] for s in FP16_SHAPES])
def test_fp16_input_equals_the_interpreter_bit_for_bit(src, dst):
    x = shape_input(src).half()
    out = VC.bicubic_resize(x[:, None].to(DEV), dst)             # planes as the batch axis this time
    assert out.dtype == torch.float32 and tuple(out.shape) == (src[0], 1) + dst
    assert_bit_equal(out[:, 0], bicubic_interp(x.numpy(), *dst))


# ---- memory discipline --------------------------------------------------------------------------------------------------------------
def _run_record(src_view, dst_view, planes, src_hw, dst_hw, x_dt):
    comp = VC._bicubic_compile(planes, src_hw, dst_hw, x_dt)
    comp.ensure_bound(comp.packer.materialise({}, DEV), torch.device(DEV))
    comp.bound.run({L.EXT_X: src_view.data_ptr(), L.EXT_OUT: dst_view.data_ptr()}, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    torch.cuda.synchronize()


@pytest.mark.parametrize("src,dst,dt", [((3, 5, 7), (13, 3), "f32"), ((1, 4, 300), (3, 259), "f32"), ((3, 5, 7), (13, 3), "f16")])
def test_poison_fence(src, dst, dt):
    """The destination is a slice of a larger buffer filled with a byte pattern: no byte outside [P, Ho, Wo] changes.  The source sits
    between NaNs: a read outside the image would show in the output."""
    P, H, W = src
    n_in, n_out = P * H * W, P * dst[0] * dst[1]
    x = shape_input(src).to(torch.float16 if dt == "f16" else torch.float32)
    pad = 64
    src_buf = torch.full((n_in + 2 * pad,), float("nan"), dtype=x.dtype, device=DEV)
    src_buf[pad:pad + n_in] = x.reshape(-1).to(DEV)
    front, back = 1024, 4096
    dst_buf = torch.full((front + 4 * n_out + back,), 0xA5, dtype=torch.uint8, device=DEV)
    dst_view = dst_buf[front:front + 4 * n_out].view(torch.float32)
    _run_record(src_buf[pad:pad + n_in], dst_view, P, (H, W), dst, dt)
    host = dst_buf.cpu().numpy()
    assert (host[:front] == 0xA5).all() and (host[front + 4 * n_out:] == 0xA5).all()
    want = bicubic_interp(x.numpy(), *dst)
    assert np.isfinite(want).all()
    assert_bit_equal(host[front:front + 4 * n_out].view(np.float32).reshape(want.shape), want)


def test_nan_and_inf_reach_exactly_their_footprint():
    src, dst = (3, 5, 7), (13, 3)
    x = shape_input(src)
    x[1, 2, 3] = float("nan")
    x[2, 0, 6] = float("inf")
    out = VC.bicubic_resize(x[None].to(DEV), dst)[0].cpu().numpy()
    want = bicubic_interp(x.numpy(), *dst)
    assert np.array_equal(np.isfinite(out), np.isfinite(want)) and np.isfinite(out[0]).all() and not np.isfinite(out[1]).all()
    assert 0 < (~np.isfinite(want)).sum() < want.size / 2
    fin = np.isfinite(want)
    assert np.array_equal(out[fin].view(np.int32), want[fin].view(np.int32))        # NaN payloads are not compared


# ---- repeatability and the program cache ----------------------------------------------------------------------------------------------
def test_launches_repeat_and_the_program_cache_keeps_results_right():
    x = shape_input((3, 32, 32))
    xd = x[None].to(DEV)
    sizes = [(24, 24), (40, 24), (24, 40), (17, 51), (64, 8)]                 # five geometries, four programs kept
    first = [VC.bicubic_resize(xd, s) for s in sizes]
    assert len(VC._BICUBIC_PROGRAMS) <= 4
    for s, a in zip(sizes, first):
        b = VC.bicubic_resize(xd, s)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert_bit_equal(b[0], bicubic_interp(x.numpy(), *s))
    assert len(VC._BICUBIC_PROGRAMS) <= 4
    same = VC.bicubic_resize(xd.half(), (32, 32))                                # equal sizes: no launch, x.float()
    assert same.dtype == torch.float32 and torch.equal(same, xd.half().float())
    with pytest.raises(L.T2VError, match="no CPU fallback"):
        VC.bicubic_resize(x[None], (24, 24))
    with pytest.raises(ValueError):
        VC.bicubic_resize(xd[0], (24, 24))


# ---- the opt-in depth path end to end -----------------------------------------------------------------------------------------------------
def _stub(frames):                              # [n, 3, H, W] -> [n, 1, H, W]; stands in for MiDaS (outside the package)
    return frames.float().mean(1, keepdim=True) * 3 + 5


def _inputs_tiny():
    g = torch.Generator().manual_seed(7)
    torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    return ctx


@pytest.fixture(scope="module")
def tiny_ld():
    """The fixture pattern of tests/test_gpu_adapter.py: T2VAdapterDepth on the tiny UNet / VAE with a one-level adapter, here with the
    estimator working at 24 x 24 (`depth_resize`)."""
    seen = []

    def depth_model(frames):
        seen.append(tuple(frames.shape))
        return _stub(frames)
    ld = VC.T2VAdapterDepth(depth_model, dict(params=dict(channels=[320], nums_rb=2, cin=64, ksize=1, sk=True, use_conv=False), cond_name="depth"),
                            configs.TINY_LVDM_UNET, dict(ddconfig=configs.TINY_VAE_DDCONFIG, embed_dim=4), image_size=[8, 8],
                            video_length=5, init_weights=False, depth_resize=(24, 24), **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    ld.first_stage_model.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.first_stage_model), seed=3), strict=True)
    ld.adapter.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.adapter), seed=11), strict=True)
    assert ld.depth_resize == (24, 24)
    return ld.to(DEV), seen


def _videos():
    g = torch.Generator().manual_seed(61)
    videos = torch.rand(1, 3, 5, 32, 32, generator=g) * 2 - 1
    videos[:, :, 3] = 0.25                                   # a constant frame: depth normalises to -1
    return videos


def test_depth_resize_wraps_the_estimator_in_the_two_resizes(tiny_ld):
    ld, seen = tiny_ld
    videos = _videos()
    vd = videos.to(DEV)
    frames = vd.permute(0, 2, 1, 3, 4).reshape(5, 3, 32, 32)
    del seen[:]
    extra = ld.get_batch_depth(vd, (32, 32))
    assert seen == [(5, 3, 24, 24)]                          # one call, on all frames at the estimator's size
    assert extra.shape == (1, 1, 5, 32, 32) and extra.dtype == torch.float32 and extra.is_cuda
    kinds = [(o.kind, o.i[9]) for o in ld.adapter.last_program.ops]
    assert kinds == [(L.OP_RESAMPLE, 1), (L.OP_DEPTH_TOKENS, 0)]          # steps 4 and 5 are ONE program
    two_calls = ld.adapter.normalise_depth(VC.bicubic_resize(_stub(VC.bicubic_resize(frames, (24, 24))), (32, 32)))
    assert torch.equal(extra[0].permute(1, 0, 2, 3), two_calls)
    assert bool((extra[:, :, 3] == -1).all()) and float(extra.min()) == -1.0 and float(extra.max()) <= 1.0
    # the reference's formula with torch on the CPU (module docstring: float32 on the non-constant frames, float64 on all)
    kw = dict(mode="bicubic", align_corners=False)
    cpu = videos.permute(0, 2, 1, 3, 4).reshape(5, 3, 32, 32)
    want32 = AR.normalise_depth(F.interpolate(_stub(F.interpolate(cpu, size=(24, 24), **kw)), size=(32, 32), **kw))
    want64 = AR.normalise_depth(F.interpolate(F.interpolate(cpu.double(), size=(24, 24), **kw).mean(1, keepdim=True) * 3 + 5, size=(32, 32), **kw))
    got = extra[0].permute(1, 0, 2, 3).cpu()
    live = [0, 1, 2, 4]
    e32, e64 = float((got[live] - want32[live]).abs().max()), float((got.double() - want64).abs().max())
    print(f"depth_resize path vs the reference formula: {e32:.3e} (float32 torch, non-constant frames), {e64:.3e} (float64 torch, all frames); "
          f"float32 torch on the constant frame: {float(want32[3].min()):.3f} .. {float(want32[3].max()):.3f}")
    assert e32 < 1e-3 and e64 < 1e-3                          # (fp16 values of the reference's formula, as tests/test_gpu_adapter.py)
    # the estimator's answer already at target_size: no resize is emitted, and the result is the plain normalisation
    same = ld.get_batch_depth(vd[:, :, :, :24, :24], (24, 24))
    assert [o.kind for o in ld.adapter.last_program.ops] == [L.OP_DEPTH_TOKENS]
    assert torch.equal(same, ld.get_batch_depth(depth=_stub(vd[:, :, :, :24, :24].permute(0, 2, 1, 3, 4).reshape(5, 3, 24, 24)).reshape(1, 5, 1, 24, 24).permute(0, 2, 1, 3, 4)))
    # target_size must suit the adapter; depth= is unchanged
    with pytest.raises(ValueError, match="multiples of 8"):
        ld.get_batch_depth(vd, (30, 32))
    assert torch.equal(ld.get_batch_depth(depth=extra), ld.adapter.normalise_depth(extra[0].permute(1, 0, 2, 3)).permute(1, 0, 2, 3)[None])


def test_adapter_guided_synthesis_picks_the_resizes_up_from_the_model(tiny_ld):
    ld, seen = tiny_ld
    ctx = _inputs_tiny()

    class Enc:            # stands in for FrozenCLIPEmbedder (outside the hot path)
        def encode(self, prompts):
            return (ctx[0:1] if prompts[0] == "a cat" else ctx[1:2]).to(DEV).repeat(len(prompts), 1, 1)
    ld.cond_stage_model = Enc()
    vd = _videos().to(DEV)
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(5)
    torch.manual_seed(0)
    del seen[:]
    out, extra = VC.adapter_guided_synthesis(ld, "a cat", vd, [1, 4, 5, 8, 8], n_samples=1, ddim_steps=2, ddim_eta=0.0,
                                             unconditional_guidance_scale=7.5, sampler=smp)
    assert seen == [(5, 3, 24, 24)]
    assert extra.shape == (1, 1, 5, 32, 32) and torch.equal(extra, ld.get_batch_depth(vd, (32, 32)))
    assert out.shape == (1, 1, 3, 5, 64, 64) and out.is_cuda and bool(torch.isfinite(out).all())
    # depth_resize = None: today's behaviour, the estimator sees the frames as they are and must answer at target_size
    ld.depth_resize = None
    try:
        del seen[:]
        assert ld.get_batch_depth(vd, (32, 32)).shape == (1, 1, 5, 32, 32) and seen == [(5, 3, 32, 32)]
        with pytest.raises(ValueError, match="must arrive at target_size"):
            ld.get_batch_depth(vd, (64, 64))
    finally:
        ld.depth_resize = (24, 24)


def test_prepare_midas_input(tiny_ld):
    ld, _ = tiny_ld
    x = shape_input((6, 16, 24)).reshape(2, 3, 16, 24)
    out = ld.prepare_midas_input(x.to(DEV))
    assert tuple(out.shape) == (2, 3, 384, 384) and out.dtype == torch.float32
    assert_bit_equal(out.reshape(6, 384, 384), bicubic_interp(x.reshape(6, 16, 24).numpy(), 384, 384))
