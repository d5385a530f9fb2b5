"""GPU (-m gpu): keyframe inpainting — T2V_OP_DDIM_STEP mode 4 on the designed operands of tests/keyframe_inputs.py, and
`GaussianDiffusion.sample(inpaint="legacy")` on the tiny UNet against golden runs of the REAL reference's legacy loop
(tests/golden/make_golden_inpaint.py).

Op level, per case: the mode-4 record and the plain mode-0 record are launched on the same operands.  Free elements carry the plain
launch's values (the update part is the plain record's, bit for bit; equality of values: x1 + 0 turns a -0 into +0), held elements the
bits of the fp32 restatement of the blend, and the non-finite fences reach the output as the arithmetic blend passes them on — all
three are one comparison against the restatement evaluated on the plain launch's x1.  Every tensor is a window of a NaN-filled
allocation; the unguided cases carry NaN in the unconditional half of the eps pair, which must not be read.

End to end: the eta-0 goldens with injected noise.  The gate is 1.5 x the error (rel-L2) of the unmasked run on the GPU against ITS
golden — the precedent of profiles/videocrafter_driver.txt: what the run shows is the fp16-operand error of the UNet passed through
the same S guided steps.  Measured values: profiles/keyframe_inpaint.txt."""
import ctypes

import numpy as np
import pytest
import torch

import keyframe_inputs as KI
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L, samplers, unet as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64                     # elements: a window that starts there keeps the allocation's 16-byte alignment


def _window(n, dtype, offset, value=None):
    """-> (big, view): `n` elements inside a NaN-filled device allocation, `offset` elements behind the aligned start."""
    big = torch.full((n + 2 * PAD + 2,), float("nan"), dtype=dtype, device=DEV)
    view = big[PAD + offset: PAD + offset + n]
    if value is not None:
        view.copy_(value.reshape(-1).to(dtype))
    return big, view


def _fence_untouched(big, n, offset):
    return bool(torch.isnan(big[:PAD + offset]).all() and torch.isnan(big[PAD + offset + n:]).all())


def _differs(a, b):
    return ~((a == b) | (a.isnan() & b.isnan()))


def _device_operands(case, guided, edt, offset):
    """Every operand as a window; the 4-byte offset is one fp32 element and two fp16 elements."""
    shape = tuple(case["xt"].shape)
    n = case["xt"].numel()
    pair = case["eps_pair"].clone()
    if not guided:
        pair[shape[0]:] = float("nan")                    # the unconditional half is not read
    w = lambda t, dt=torch.float32, k=1: _window(t.numel(), dt, offset * (2 if dt == torch.float16 else 1), t)[1].view(t.shape)
    dev = dict(xt=w(case["xt"]), eps_pair=w(pair, edt), noise=None if case["noise"] is None else w(case["noise"]),
               original=w(case["original"]), mask=w(case["mask"]), qnoise=w(case["qnoise"]))
    out_big, out = _window(n, torch.float32, offset)
    plain_big, plain = _window(n, torch.float32, offset)
    return dev, pair, (out_big, out.view(shape)), (plain_big, plain.view(shape))


def _op_case(shape, edt, guided, eta, offset=0):
    case = KI.kernel_case(shape, edt, eta)
    dev, pair, (out_big, out), (plain_big, plain) = _device_operands(case, guided, edt, offset)
    n = out.numel()
    samplers._ddim_update_keyframe(out, dev["xt"], dev["eps_pair"], dev["noise"], case["coef"], guided, dev["original"], dev["mask"],
                                   dev["qnoise"], case["qcoef"], case["v"])
    samplers._ddim_update(plain, dev["xt"], dev["eps_pair"], dev["noise"], case["coef"], guided, 0)
    torch.cuda.synchronize()
    L.async_status()
    got, x1 = out.cpu(), plain.cpu()
    assert _fence_untouched(out_big, n, offset) and _fence_untouched(plain_big, n, offset)
    want = KI.keyframe_step(case["xt"], pair, case["noise"], case["coef"], guided, case["original"], case["mask"], case["qnoise"],
                            case["qcoef"], case["v"], x1=x1)
    clean = ~(case["fence_orig"] | case["fence_x1"])
    free, held = ~case["held"] & clean, case["held"] & clean
    assert free.sum() > n // 8 and held.sum() > n // 8
    assert torch.isfinite(x1[clean]).all()
    assert torch.equal(got[free], x1[free])                                                      # the plain record's update
    known = KI.keyframe_blend(torch.zeros_like(x1), case["original"], torch.zeros_like(x1), case["qnoise"], case["qcoef"], case["v"])
    assert torch.equal(got[held].view(torch.int32), known[held].view(torch.int32))               # the restatement's bits
    assert got[case["fence_orig"]].isnan().all() and got[case["fence_x1"]].isnan().all()          # arithmetic, not a select
    assert not _differs(got, want).any() and not got[clean].isnan().any()
    # the restatement of the whole step (every operation rounded by itself) agrees with the kernel's update to rounding
    whole = KI.keyframe_step(case["xt"], pair, case["noise"], case["coef"], guided, case["original"], case["mask"], case["qnoise"],
                             case["qcoef"], case["v"])
    assert float((got[free] - whole[free]).abs().max()) <= 1e-5 * float(whole[free].abs().max())
    for mutant in KI.MUTANTS:                                                                      # the launch is none of them
        if (mutant == "blend before the eta noise" and not eta) or (mutant == "the mask of the next sample in the batch" and shape[0] == 1):
            continue
        bad = KI.keyframe_step(case["xt"], pair, case["noise"], case["coef"], guided, case["original"], case["mask"], case["qnoise"],
                               case["qcoef"], case["v"], mutant=mutant, x1=None if mutant == "blend before the eta noise" else x1)
        assert _differs(got, bad).any(), mutant


@pytest.mark.parametrize("eta", [True, False])
@pytest.mark.parametrize("guided", [0, 2, 4])
@pytest.mark.parametrize("edt", [torch.float16, torch.float32])
@pytest.mark.parametrize("shape", KI.KERNEL_SHAPES)
def test_mode4_is_the_plain_step_and_the_blend(shape, edt, guided, eta):
    _op_case(shape, edt, guided, eta)


@pytest.mark.parametrize("eta", [True, False])
@pytest.mark.parametrize("guided", [0, 2, 4])
@pytest.mark.parametrize("edt", [torch.float16, torch.float32])
def test_mode4_unaligned_views_take_the_scalar_path(edt, guided, eta):
    _op_case(KI.KERNEL_SHAPES[-1], edt, guided, eta, offset=1)


def test_refused_records_launch_nothing():
    case = KI.kernel_case(KI.KERNEL_SHAPES[0])
    dev, _, (out_big, out), _ = _device_operands(case, 2, torch.float32, 0)
    lib = L.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def record():
        return samplers._ddim_record(out, dev["xt"], dev["eps_pair"], dev["noise"], case["coef"], 2, 4,
                                     keyframe=(dev["original"], dev["mask"], dev["qnoise"], case["qcoef"], case["v"]))

    def spoil(field, k, v):
        op = record()
        getattr(op, field)[k] = v
        return op
    for op, needle in ((spoil("i", 7, 1), b"mode 4"), (spoil("i", 8, 1), b"mode 4"), (spoil("i", 9, 1), b"mode 4"), (spoil("i", 4, L.F16), b"fp32 x"),
                       (spoil("p", 4, 0), b"original latent"), (spoil("p", 5, 0), b"original latent"), (spoil("p", 6, 0), b"blend noise"),
                       (spoil("i", 5, 5), b"mode")):
        assert lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, stream) == -1 and needle in lib.t2v_last_error(), needle
    torch.cuda.synchronize()
    assert torch.isnan(out_big).all()                                  # nothing was written
    assert lib.t2v_run_ops(ctypes.byref(record()), 1, None, 0, stream) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(out.cpu()[~case["fence_orig"] & ~case["fence_x1"]]).any()


# ---- the sampler on the tiny UNet ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, betas


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(KI.GOLD))


def _rel_l2(a, g):
    g = torch.as_tensor(g).double().reshape(-1)
    return float((a.detach().cpu().double().reshape(-1) - g).norm() / g.norm())


def _sample(tiny, gold, name, **kw):
    """The product's sampler with guidance over all channels ("fixed_small"), as the legacy class had to be built for the goldens."""
    net, betas = tiny
    samplers.available_samplers[0].register_buffers_to_model(net, betas, torch.device(DEV))
    d = samplers.GaussianDiffusion(net, betas, var_type="fixed_small")
    S, eta, kind = KI.CASES[name]
    latents, mask, c, uc = KI.case_inputs(name)
    if kind is not None:
        kw = dict(mask=mask.to(DEV), inpaint="legacy", inpaint_noise=torch.from_numpy(gold[f"{name}_noise"]).to(DEV), **kw)
    return d.sample(x_T=latents.to(DEV), S=S, shape=tuple(latents.shape), conditioning=c.to(DEV), unconditional_conditioning=uc.to(DEV),
                    unconditional_guidance_scale=KI.GUIDANCE, eta=eta, **kw)


def test_legacy_inpaint_matches_reference_golden(tiny, gold):
    plain = _rel_l2(_sample(tiny, gold, "plain"), gold["plain_out"])
    r = {name: _rel_l2(_sample(tiny, gold, name), gold[f"{name}_out"]) for name in ("frames_eta0", "spatial")}
    print(f"keyframe inpainting on the tiny UNet, rel-L2 vs the reference golden: plain {plain:.3e} (gate 1.5 x = {1.5 * plain:.3e}) "
          + " ".join(f"{k} {v:.3e}" for k, v in r.items()))
    x = _sample(tiny, gold, "frames_eta0").cpu()
    lat = torch.from_numpy(gold["frames_eta0_latents"])
    assert float((x[:, :, 0] - lat[:, :, 0]).abs().max()) < 0.5 < float((x[:, :, 4] - lat[:, :, 4]).abs().max())
    assert 0 < plain < 3e-2                                            # the tiny guided gate of tests/test_gpu_e2e.py
    assert max(r.values()) <= 1.5 * plain, (r, plain)


def test_public_route_equals_the_sampler_level_result(tiny):
    """`infer_conditioned(..., inpaint="legacy")` with the pipeline's own sampler (half-channel guidance, natural draws)."""
    from sd_webui_text2video_amd.pipeline import TextToVideoSynthesis
    net, betas = tiny
    latents, mask, c, uc = (t.to(DEV) for t in KI.case_inputs("frames_eta0"))
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM_Gaussian")
    smp.progress = False
    torch.manual_seed(11)
    want = smp.sample_loop(steps=4, strength=1, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=latents, shape=KI.SHAPE,
                           noise=torch.zeros(KI.SHAPE, device=DEV), guidance_scale=KI.GUIDANCE, eta=1.0, mask=mask,
                           sampler_name="DDIM_Gaussian", inpaint="legacy")
    pipe = TextToVideoSynthesis(sd_model=net, betas=betas, device=DEV)
    pipe.diffusion.progress = False
    kw = dict(latents=latents, strength=1, mask=mask, sampler="DDIM_Gaussian", decode=False)
    torch.manual_seed(11)
    _, x0 = pipe.infer_conditioned(c, uc, 4, 5, 1, KI.GUIDANCE, 64, 64, 1.0, inpaint="legacy", **kw)
    assert x0.dtype == torch.float32 and torch.equal(x0, want)
    torch.manual_seed(11)
    _, inert = pipe.infer_conditioned(c, uc, 4, 5, 1, KI.GUIDANCE, 64, 64, 1.0, **kw)
    assert not torch.equal(inert.float(), want)                       # without the keyword the mask does nothing
    assert float((x0[:, :, 0] - latents[:, :, 0]).abs().max()) < 0.5
