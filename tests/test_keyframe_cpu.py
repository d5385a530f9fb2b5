"""CPU: keyframe inpainting of the DDIM_Gaussian sampler, `GaussianDiffusion.sample(inpaint="legacy")` — the host logic against golden
runs of the REAL reference's legacy loop (GaussianDiffusion.ddim_sample_loop, modelscope/t2v_model.py:1460-1577;
tests/golden/make_golden_inpaint.py).

As in tests/test_ddim_inversion_cpu.py the device bindings are replaced by torch restatements (`_ddim_update_keyframe` and the plain
step by tests/keyframe_inputs.py, `_lincomb` by test_samplers_cpu's) and the UNet by the oracle port, so the product's own host logic
is under test: the start from the re-noised latents, the thresholds, the timesteps of the blend, the draw order, the refusals and the
keyword plumbing.  The record validation of T2V_OP_DDIM_STEP mode 4 needs no GPU (a refused record launches nothing).  The kernel
itself: tests/test_gpu_keyframe.py.

The gate.  The plain case (mask=None through the same legacy loop) is measured against its golden through the same machinery; what it
shows is the oracle port's rounding against the reference UNet's, passed through S guided steps.  The masked cases get twice that
error: the blend re-injects fresh noise after every step, so the roundings of the steps do not average out as in a plain run.
Measured (max-abs error over the golden's max-abs, the larger of the final latent's and the per-step x_t's): plain 9.43e-7, so the gate
is 1.89e-6; frames_eta0 8.78e-7, frames_eta1 1.15e-6, spatial 1.08e-6 (profiles/keyframe_inpaint.txt)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import keyframe_inputs as KI
from oracle import torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import pipeline, samplers
from test_samplers_cpu import _lincomb_cpu, _PortModel, _rel

MASKED = [n for n, (_, _, kind) in KI.CASES.items() if kind is not None]


def _at(ptr, n, dtype=torch.float32):
    ct = ctypes.c_float if dtype == torch.float32 else ctypes.c_uint16
    a = np.ctypeslib.as_array((ct * n).from_address(int(ptr)))
    return torch.from_numpy(a) if dtype == torch.float32 else torch.from_numpy(a.view(np.float16))


class _PlainStepLib:
    """Stands in for the library's `t2v_ddim_step` (the plain mode-0 step the sampler launches through a plan): the restatement, on the
    host tensors behind the pointers.  Everything else is the real library's."""

    def __init__(self):
        self.calls = 0

    def t2v_ddim_step(self, handle, xt, eps, noise, out, coef, stream):
        C, inner, guided, eps_dt, x_dt, samples = handle
        assert x_dt == "f32"
        n = samples * C * inner
        shape = (samples, C, inner)
        e = _at(eps, (2 if guided else 1) * n, torch.float32 if eps_dt == "f32" else torch.float16).view((-1,) + shape[1:])
        r = KI.plain_step(_at(xt, n).view(shape), e, None if noise is None else _at(noise, n).view(shape), list(coef), guided)
        _at(out, n).copy_(r.reshape(-1))
        self.calls += 1
        return 0


@pytest.fixture()
def cpu_kernels(monkeypatch):
    """-> the list of keyword-free argument tuples the keyframe binding was called with, and the plain-step stand-in"""
    calls, lib = [], _PlainStepLib()
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update_keyframe", lambda *a: (calls.append(a), KI.keyframe_update_cpu(*a))[1])
    monkeypatch.setattr(samplers.L, "load", lambda: lib)
    monkeypatch.setattr(samplers.GaussianDiffusion, "_step_plan",
                        lambda self, C, inner, guided, eps_dtype, x_dtype, samples=1: types.SimpleNamespace(handle=(C, inner, guided, eps_dtype, x_dtype, samples)))
    samplers.state.sampling_step = 0
    return types.SimpleNamespace(keyframe=calls, lib=lib)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(KI.GOLD))


@pytest.fixture(scope="module")
def port_model():
    return _PortModel()


def _diffusion(model):
    """The product's sampler as the goldens need it: "fixed_small" = guidance over all channels, as the legacy class had to be built."""
    samplers.available_samplers[0].register_buffers_to_model(model, tp.beta_schedule_linear_sd(), torch.device("cpu"))
    return samplers.GaussianDiffusion(model, tp.beta_schedule_linear_sd(), var_type="fixed_small")


def _run(name, gold, model, injected=True, **kw):
    S, eta, kind = KI.CASES[name]
    latents, mask, c, uc = KI.case_inputs(name)
    assert np.array_equal(latents.numpy(), gold[f"{name}_latents"]) and np.array_equal(c.half().numpy(), gold["c"])
    d = _diffusion(model)
    model.calls.clear()
    xts = []
    inner = model.__call__

    class _Seen:
        """the x_t of every (batched) model call"""
        supports_cfg_batch, num_timesteps, device = True, 1000, model.device

        def __call__(self, x, t, cc):
            xts.append(x[:1].clone())
            return inner(x, t, cc)
    if kind is not None:
        kw = dict(mask=mask, inpaint="legacy", **kw)
        if injected:
            kw["inpaint_noise"] = torch.from_numpy(gold[f"{name}_noise"])
    d.model = _Seen()
    torch.manual_seed(KI.SEED)
    before = latents.clone()
    real_step_noise = samplers._step_noise
    if injected and eta != 0.0:
        # injected blend noise leaves the generator where the golden's eta draws are not: they are replayed (the draw is still made)
        replay = iter(torch.from_numpy(gold[f"{name}_eta"]))
        samplers._step_noise = lambda *a: (real_step_noise(*a), next(replay))[1]
    try:
        x = d.sample(x_T=latents, S=S, shape=tuple(latents.shape), conditioning=c, unconditional_conditioning=uc,
                     unconditional_guidance_scale=KI.GUIDANCE, eta=eta, **kw)
    finally:
        samplers._step_noise = real_step_noise
    assert torch.equal(latents, before)                              # the caller's tensor is never written
    return x, torch.stack(xts)


@pytest.fixture(scope="module")
def plain_error(gold, port_model):
    """The measured error of the baseline: the plain run against its golden through the same machinery (module docstring)."""
    with pytest.MonkeyPatch.context() as mp:
        lib = _PlainStepLib()
        mp.setattr(samplers, "_lincomb", _lincomb_cpu)
        mp.setattr(samplers.L, "load", lambda: lib)
        mp.setattr(samplers.GaussianDiffusion, "_step_plan",
                   lambda self, C, inner, guided, eps_dtype, x_dtype, samples=1: types.SimpleNamespace(handle=(C, inner, guided, eps_dtype, x_dtype, samples)))
        x, xts = _run("plain", gold, port_model)
    e = max(_rel(x, gold["plain_out"]), _rel(xts, gold["plain_xt"]))
    print(f"plain run against its golden: {e:.3e}")
    assert 0 < e < 2e-5                                              # the CPU gate of tests/test_samplers_cpu.py
    return e


@pytest.mark.parametrize("name", MASKED)
def test_legacy_inpaint_matches_the_reference(cpu_kernels, gold, port_model, plain_error, name):
    S, eta, _ = KI.CASES[name]
    x, xts = _run(name, gold, port_model)
    e_out, e_xt = _rel(x, gold[f"{name}_out"]), _rel(xts, gold[f"{name}_xt"])
    print(f"{name}: final latent {e_out:.3e}, per-step x_t {e_xt:.3e}; gate 2 x {plain_error:.3e}")
    assert e_out <= 2 * plain_error and e_xt <= 2 * plain_error
    assert len(cpu_kernels.keyframe) == S - 1 and cpu_kernels.lib.calls == 1          # the last step is the plain step
    assert [a[-1] for a in cpu_kernels.keyframe] == [(S - i - 1) / S for i in range(S - 1)]
    assert not np.array_equal(x.numpy(), gold["plain_out"])


def test_natural_draws_follow_the_legacy_order(cpu_kernels, gold, port_model, plain_error):
    """Without inpaint_noise: n0, then per step the eta draw and (all steps but the last) the blend draw, on the global generator —
    with eta = 1 every one of them reaches the latent."""
    x, xts = _run("frames_eta1", gold, port_model, injected=False)
    assert max(_rel(x, gold["frames_eta1_out"]), _rel(xts, gold["frames_eta1_xt"])) <= 2 * plain_error
    for k, a in enumerate(cpu_kernels.keyframe):
        assert np.array_equal(a[8].numpy(), gold["frames_eta1_noise"][k + 1]) and np.array_equal(a[3].numpy(), gold["frames_eta1_eta"][k])
    after = torch.randn(3)
    torch.manual_seed(KI.SEED)
    for _ in range(2 * 4):                                            # 1 + S + (S - 1) draws and no inert-hook draw
        torch.randn(KI.SHAPE)
    assert torch.equal(after, torch.randn(3))


def test_held_frames_stay_at_the_picture(cpu_kernels, gold, port_model):
    x, _ = _run("frames_eta0", gold, port_model)
    lat = torch.from_numpy(gold["frames_eta0_latents"])
    assert float((x[:, :, 0] - lat[:, :, 0]).abs().max()) < 0.5 < float((x[:, :, 4] - lat[:, :, 4]).abs().max())


def test_default_is_what_it_was(cpu_kernels, gold, port_model):
    """inpaint=None: the mask does nothing, the latent is the plain run's bit for bit, and the draws are today's (the eta draw and the
    inert hook's, every step)."""
    latents, mask, c, uc = KI.case_inputs("frames_eta0")
    d = _diffusion(port_model)
    kw = dict(x_T=latents, S=4, shape=tuple(latents.shape), conditioning=c, unconditional_conditioning=uc,
              unconditional_guidance_scale=KI.GUIDANCE, eta=1.0)
    torch.manual_seed(3)
    a = d.sample(**kw)
    torch.manual_seed(3)
    b = d.sample(mask=mask, **kw)
    after = torch.randn(3)
    assert torch.equal(a, b) and not cpu_kernels.keyframe and cpu_kernels.lib.calls == 8
    torch.manual_seed(3)
    etas = []
    for _ in range(4):
        etas.append(torch.randn(KI.SHAPE))
        torch.randn(KI.SHAPE)
    assert torch.equal(after, torch.randn(3))
    # the same run written out with the restatement: the eta draws are the 1st, 3rd, ... of the generator
    x = latents.clone()
    ac, stride = d.alphas_cumprod, 250
    for k, t in enumerate((751, 501, 251, 1)):
        tt = torch.full((2,), float(t))
        eps = port_model(torch.cat([x, x]), tt, torch.cat([c, uc]))
        a_t, a_prev = ac[t].float(), ac[max(t - stride, 0)].float()
        sigma = 1.0 * torch.sqrt((1 - a_prev) / (1 - a_t) * (1 - a_t / a_prev))
        coef = [float(d.sqrt_recip_alphas_cumprod[t].float()), float(d.sqrt_recipm1_alphas_cumprod[t].float()), float(torch.sqrt(a_prev)),
                float(torch.sqrt(1 - a_prev - sigma ** 2)), float(sigma), KI.GUIDANCE]
        x = KI.plain_step(x, eps, etas[k], coef, 4)
    assert torch.equal(a, x)


# ---- keyword plumbing ---------------------------------------------------------------------------------------------------------------
def _loop_sampler(model, name="DDIM_Gaussian"):
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
    smp.progress = False
    return smp


def test_sample_loop_forwards_the_keyword(cpu_kernels, port_model):
    latents, mask, c, uc = KI.case_inputs("frames_eta0")
    smp = _loop_sampler(port_model)
    kw = dict(steps=2, strength=1, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=latents, shape=KI.SHAPE,
              noise=torch.zeros(KI.SHAPE), guidance_scale=KI.GUIDANCE, eta=0.0, mask=mask, sampler_name="DDIM_Gaussian")
    torch.manual_seed(1)
    plain = smp.sample_loop(**kw)
    assert not cpu_kernels.keyframe
    torch.manual_seed(1)
    held = smp.sample_loop(inpaint="legacy", **kw)
    assert len(cpu_kernels.keyframe) == 1 and cpu_kernels.keyframe[0][-1] == 0.5 and not torch.equal(plain, held)
    seen = {}
    smp.sampler.sample = lambda **k: seen.update(k) or torch.zeros(KI.SHAPE)
    smp.sample_loop(**kw)
    assert "inpaint" not in seen                                      # forwarded only when set
    smp.sample_loop(inpaint="legacy", **kw)
    assert seen["inpaint"] == "legacy" and seen["mask"] is mask
    for other in ("DDIM", "UniPC"):
        with pytest.raises(ValueError, match="DDIM_Gaussian sampler only"):
            _loop_sampler(port_model, other).sample_loop(inpaint="legacy", **dict(kw, sampler_name=other))


class _ToyPipe(pipeline.TextToVideoSynthesis):
    """A pipeline put together without __init__: the sampler loop is recorded, nothing is decoded."""

    def __init__(self, model):
        self.device = torch.device("cpu")
        self.sd_model = types.SimpleNamespace(to=lambda dev: None)
        self.diffusion = _loop_sampler(model)
        self.seen = []
        self.diffusion.sample_loop = lambda **k: self.seen.append(k) or torch.zeros(KI.SHAPE)
        self.autoencoder = self.clip_encoder = None

    def compute_latents(self, vd_out, cpu_vae=None, device=None, height=None, width=None):
        return torch.zeros(KI.SHAPE)

    def decode_frames(self, x0, bgr=False):
        return torch.zeros(x0.shape[2], 64, 64, 3, dtype=torch.uint8)


def test_infer_conditioned_and_process_modelscope_forward_the_keyword(port_model, monkeypatch):
    monkeypatch.setattr(pipeline.L, "async_status", lambda: None)
    pipe = _ToyPipe(port_model)
    latents, mask, c, uc = KI.case_inputs("frames_eta0")
    pipe.infer_conditioned(c, uc, 4, 5, 1, KI.GUIDANCE, 64, 64, latents=latents, strength=1, mask=mask, sampler="DDIM_Gaussian", decode=False)
    assert "inpaint" not in pipe.seen[-1]
    pipe.infer_conditioned(c, uc, 4, 5, 1, KI.GUIDANCE, 64, 64, latents=latents, strength=1, mask=mask, sampler="DDIM_Gaussian", decode=False,
                           inpaint="legacy")
    assert pipe.seen[-1]["inpaint"] == "legacy" and pipe.seen[-1]["mask"] is mask
    args = dict(pipe=pipe, cond=c, uncond=uc, steps=4, frames=5, seed=1, cfg_scale=KI.GUIDANCE, width=64, height=64, sampler="DDIM_Gaussian",
                inpainting_frames=5, inpainting_image=np.zeros((64, 64, 3), dtype=np.uint8), inpainting_weights=list(KI.FRAME_WEIGHTS))
    pipeline.process_modelscope(dict(args))
    assert "inpaint" not in pipe.seen[-1] and pipe.seen[-1]["mask"] is not None
    pipeline.process_modelscope(dict(args, inpaint="legacy"))
    k = pipe.seen[-1]
    assert k["inpaint"] == "legacy" and k["mask"].shape == KI.SHAPE and k["mask"][0, 0, :, 0, 0].tolist() == list(KI.FRAME_WEIGHTS)
    assert pipeline._restriction(None, None) == {} and pipeline._restriction(None, None, inpaint="legacy") == {"inpaint": "legacy"}
    # batches stay refused on the img2vid route
    with pytest.raises(NotImplementedError, match="img2vid"):
        pipe.infer_conditioned(c, uc, 4, 5, 1, KI.GUIDANCE, 64, 64, latents=latents, strength=1, mask=mask, sampler="DDIM_Gaussian",
                               decode=False, videos=2, inpaint="legacy")
    with pytest.raises(NotImplementedError, match="img2vid"):
        pipeline.process_modelscope(dict(args, inpaint="legacy", conds=[c, c]))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(cpu_kernels, port_model):
    latents, mask, c, uc = KI.case_inputs("frames_eta0")
    d = _diffusion(port_model)
    kw = dict(S=4, shape=KI.SHAPE, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=KI.GUIDANCE, eta=0.0)
    with pytest.raises(ValueError, match="needs the mask"):
        d.sample(x_T=latents, inpaint="legacy", **kw)
    with pytest.raises(ValueError, match="needs the mask"):
        d.sample(mask=mask, inpaint="legacy", **kw)                   # no x_T
    with pytest.raises(ValueError, match="None or 'legacy'"):
        d.sample(x_T=latents, mask=mask, inpaint="repaint", **kw)
    for extra in (dict(clamp=1.0), dict(percentile=0.995), dict(condition_fn=lambda x, t: x)):
        with pytest.raises(ValueError, match="clamp / percentile / condition_fn"):
            d.sample(x_T=latents, mask=mask, inpaint="legacy", **extra, **kw)
    with pytest.raises(L.T2VError, match="fp32 latent"):
        d.sample(x_T=latents.half(), mask=mask, inpaint="legacy", **kw)
    d.cfg_parallel = types.SimpleNamespace(size=2, role=0)
    with pytest.raises(L.T2VError, match="CFG-pair"):
        d.sample(x_T=latents, mask=mask, inpaint="legacy", **kw)
    d.cfg_parallel = None
    d.shared_noise = types.SimpleNamespace(total=10)
    with pytest.raises(L.T2VError, match="split over ranks"):
        d.sample(x_T=latents, mask=mask, inpaint="legacy", **kw)
    d.shared_noise = None
    d.model = types.SimpleNamespace(device=torch.device("cpu"), t_shard=object())
    with pytest.raises(L.T2VError, match="split over ranks"):
        d.sample(x_T=latents, mask=mask, inpaint="legacy", **kw)
    d.model = port_model
    with pytest.raises(L.T2VError, match="inpaint_noise"):
        d.sample(x_T=latents, mask=mask, inpaint="legacy", inpaint_noise=torch.zeros((3,) + KI.SHAPE), **kw)
    assert not cpu_kernels.keyframe and cpu_kernels.lib.calls == 0    # nothing ran


# ---- the record ---------------------------------------------------------------------------------------------------------------------
def _record(**kw):
    """A valid mode-4 DDIM_STEP record over made-up addresses, then the overrides."""
    op = L.T2VOp()
    op.kind = L.OP_DDIM_STEP
    ptr = 1 << 40
    op.i[0], op.i[1], op.i[2], op.i[6] = kw.get("C", 8), kw.get("inner", 768), kw.get("i2", 2), 4
    op.i[3], op.i[4], op.i[5] = kw.get("i3", L.F32), kw.get("i4", L.F32), kw.get("i5", 4)
    op.i[7], op.i[8], op.i[9], op.i[10] = kw.get("i7", 0), kw.get("i8", 0), kw.get("i9", 0), KI.f32_bits(0.75)
    for k, v in enumerate((1.7, 1.4, 0.9, 0.3, 0.2, 3.0, 0.8, kw.get("f7", 0.6))):
        op.f[k] = v
    op.p[0], op.p[1], op.p[2], op.p[3] = ptr, ptr + (1 << 30), ptr + (2 << 30), kw.get("p3", ptr + (3 << 30))
    op.p[4], op.p[5], op.p[6] = kw.get("p4", ptr + (4 << 30)), kw.get("p5", ptr + (5 << 30)), kw.get("p6", ptr + (6 << 30))
    return op


def test_record_validation_without_gpu(built_lib):
    lib = built_lib

    def refused(needle=b"mode 4", **kw):
        rc = lib.t2v_run_ops(ctypes.byref(_record(**kw)), 1, None, 0, None)
        return rc == -1 and b"DDIM" in lib.t2v_last_error() and needle in lib.t2v_last_error()

    def accepted(**kw):
        h = ctypes.c_void_p()
        rc = lib.t2v_plan_create(ctypes.byref(_record(**kw)), 1, ctypes.byref(h))
        if rc == 0:
            lib.t2v_plan_destroy(h)
        return rc == 0

    assert accepted() and accepted(i3=L.F16) and accepted(p6=0, f7=0.0)
    for part in (0, 1, 2, 3, 4):
        assert accepted(i2=part), part                                # the half-channel guidance of mode 0, and every other share
    assert refused(b"guided channels", i2=5)
    for field in ("i7", "i8", "i9"):
        assert refused(**{field: 1}), field
    assert refused(b"fp32 x", i4=L.F16)
    assert refused(b"original latent", p4=0) and refused(b"original latent", p5=0)
    assert refused(b"blend noise", p6=0) and refused(b"null DDIM step pointer", p3=0)
    assert refused(b"guided channels / mode", i5=5)
    assert accepted(i5=0) and refused(b"blend flag", i5=0, i7=2) and refused(b"mode 1", i5=0, i7=1)     # the earlier modes are what they were


def test_binding_builds_the_mode4_record(monkeypatch):
    seen = []

    class _Lib:
        def t2v_run_ops(self, op, n, ext, n_ext, stream):
            o = op._obj
            seen.append(([o.i[k] for k in range(12)], [o.f[k] for k in range(8)], [o.p[k] for k in range(9)], n))
            return 0
    monkeypatch.setattr(L, "load", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 0})())
    x = torch.zeros(2, 4, 3, 4, 4)
    eps, noise = torch.zeros(4, 4, 3, 4, 4, dtype=torch.float16), torch.zeros_like(x)
    out, orig, mask, qn = (torch.zeros_like(x) for _ in range(4))
    coef = (1.5, 0.25, 0.5, 0.125, 0.75, 3.0)
    samplers._ddim_update_keyframe(out, x, eps, noise, coef, 2, orig, mask, qn, (0.5, 0.25), 0.6)
    samplers._ddim_update_keyframe(out, x, eps, noise, coef[:4] + (0.0, 3.0), 4, orig, mask, None, (1.0, 0.0), 0.75)
    i, f, p, n = seen[0]
    assert i == [8, 48, 2, L.F16, L.F32, 4, 4, 0, 0, 0, KI.f32_bits(0.6), 0] and n == 1
    assert i[10] == int(np.array([0.6], dtype=np.float32).view(np.int32)[0])
    assert f == [1.5, 0.25, 0.5, 0.125, 0.75, 3.0, 0.5, 0.25]
    assert p == [x.data_ptr(), eps.data_ptr(), noise.data_ptr(), out.data_ptr(), orig.data_ptr(), mask.data_ptr(), qn.data_ptr(), 0, 0]
    i, f, p, n = seen[1]
    assert i[2] == 4 and i[10] == KI.f32_bits(0.75) and f[4] == 0.0 and f[6:] == [1.0, 0.0] and p[2] == 0 and p[6] == 0
    # every other record leaves the threshold word zero
    samplers._ddim_update(out, x, eps, noise, coef, 2, 0)
    assert seen[2][0][10] == 0 and seen[2][0][5] == 0
    for bad in (dict(orig=orig.half()), dict(mask=mask[:1]), dict(qn=qn.double())):
        a = dict(orig=orig, mask=mask, qn=qn)
        a.update(bad)
        with pytest.raises(L.T2VError, match="keyframe DDIM step"):
            samplers._ddim_update_keyframe(out, x, eps, noise, coef, 2, a["orig"], a["mask"], a["qn"], (0.5, 0.25), 0.6)
    assert len(seen) == 3
