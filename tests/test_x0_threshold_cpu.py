"""CPU: clamp / percentile x0 thresholding and classifier guidance of the DDIM_Gaussian sampler (gaussian_sampler.py:110-120, 199-211).

  * the torch restatement of the measure pass (tests/x0_threshold_ref.py) against what the REAL reference recorded
    (tests/golden/make_golden_threshold.py: the x0 that entered `restrict_range_x0` and the s it computed) and against `torch.quantile`,
    bit for bit;
  * the sampler loop's host logic with the device binding replaced by the restatement, against each golden run;
  * the record validation of T2V_OP_DDIM_STEP i[8] / i[9] (no GPU needed: a refused record launches nothing);
  * the keyword plumbing of `sample_loop` / `infer_conditioned`.
The kernels themselves: tests/test_gpu_x0_threshold.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import x0_threshold_ref as XR
from oracle import configs, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from test_samplers_cpu import _PortModel, _inputs, _rel

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_restatement_matches_the_reference_recorded_thresholds():
    gold = np.load(os.path.join(GOLD, "modelscope_threshold_tiny.npz"))
    for name in ("percentile", "percentile_cond"):
        x0s, ss = torch.from_numpy(gold[f"{name}_x0"]), torch.from_numpy(gold[f"{name}_s"])
        assert (ss > 1).sum() * 2 >= len(ss)                       # the thresholding is at work in the golden
        for k in range(XR.STEPS):
            tab = XR.measure(x0s[k], 0.995)
            assert torch.equal(_bits(tab[:, 0]), _bits(ss[k:k + 1])), (name, k, tab, ss[k])
            srt = torch.sort(x0s[k].flatten().abs())[0]
            lo, hi, _ = XR.ranks(srt.numel(), 0.995)
            assert torch.equal(_bits(tab[0, 2:4]), _bits(torch.stack([srt[lo], srt[hi]]))), (name, k)


@pytest.mark.parametrize("n", [1, 2, 3, 36, 201, 257, 2520, 131802])
def test_restatement_matches_torch_quantile_bit_for_bit(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2, n, generator=g) * 3
    for p in (0.995, 0.5, 1.0, 1e-3):
        want = torch.quantile(x.abs(), p, dim=1)
        tab = XR.measure(x, p)
        assert torch.equal(_bits(tab[:, 1]), _bits(want)), (n, p)
        assert torch.equal(_bits(tab[:, 0]), _bits(want.clamp(min=1.0))), (n, p)
    lo, hi, w = XR.ranks(201, 0.995)
    assert (lo, hi, float(w)) == (199, 199, 0.0)                    # an integer fp32 rank: weight 0
    assert XR.ranks(131802, 0.995)[0:2] == (131142, 131142)         # the exact rank is 131141.995: fp32 picks other neighbours
    xn = x.clone()
    xn[1, 0] = float("nan")
    tab = XR.measure(xn, 0.5)
    assert torch.isnan(tab[1, 0]) and torch.isnan(tab[1, 1]) and not torch.isnan(tab[0]).any()
    assert torch.isnan(torch.quantile(xn.abs(), 0.5, dim=1)[1])


def test_restrictions_and_guidance_term_restate_the_reference_methods():
    """restrict / step against the formulas of restrict_range_x0 and get_eps written out with torch ops on one tensor."""
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(1, 4, 3, 5, 5, generator=g) * 4
    s = torch.quantile(x0.flatten(1).abs(), 0.995, dim=1).clamp_(1.0)
    assert torch.equal(XR.restrict(x0, 2, s=XR.measure(x0, 0.995)[:, 0]), torch.min(s, torch.max(-s, x0)) / s)
    assert torch.equal(XR.restrict(x0, 1, 1.0), x0.clamp(-1, 1)) and XR.restrict(x0, 0) is x0
    xt, grad = torch.randn(1, 4, 3, 5, 5, generator=g), torch.randn(1, 4, 3, 5, 5, generator=g)
    eps = torch.randn(2, 4, 3, 5, 5, generator=g)
    coef = [1.7, 1.4, 0.9, 0.3, 0.0, 9.0]
    f = [torch.tensor(c) for c in coef]
    out, _ = XR.step(xt, eps, None, coef, 2, kind=1, bound=1.0, grad=grad, sqrt_1mat=0.8)
    e = torch.cat([eps[1:, :2] + f[5] * (eps[:1, :2] - eps[1:, :2]), eps[:1, 2:]], dim=1)
    x0r = (f[0] * xt - f[1] * e).clamp(-1, 1)
    e2 = (f[0] * xt - x0r) / f[1] - torch.tensor(0.8) * grad
    want = f[2] * (f[0] * xt - f[1] * e2) + f[3] * e2
    assert torch.equal(out, want)


@pytest.fixture()
def cpu_restricted_step(monkeypatch):
    calls = []
    monkeypatch.setattr(samplers, "_ddim_restricted_step", lambda *a, **k: (calls.append(k), XR.restricted_step_cpu(*a, **k))[1])
    samplers.state.sampling_step = 0
    return calls


class _ReplayModel:
    """Stands in for the UNet with the REFERENCE UNet's own answers, recorded by tests/golden/make_golden_threshold.py: per step the
    conditional and the unconditional prediction, and the x_t the reference's loop gave its UNet.  Two b = 1 calls per step, as the
    reference makes them.  What the loop under test hands over is kept, so that every step's x_t is compared with the reference's."""
    supports_cfg_batch = False
    num_timesteps = 1000

    def __init__(self, eps, c, uc):
        self.eps, self.c, self.uc = torch.from_numpy(eps), c, uc
        self.calls, self.xts = [], []

    def __call__(self, x, t, cond):
        k, role = divmod(len(self.calls), 2)
        assert cond is (self.c, self.uc)[role], "conditional first, then unconditional (gaussian_sampler.py:161-162)"
        self.calls.append((x.shape[0], t.tolist()))
        if role == 0:
            self.xts.append(x.clone())
        else:
            assert torch.equal(x, self.xts[-1])
        return self.eps[k, role:role + 1].clone()


def _run_case(name, model, c, uc, noise, calls):
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name="DDIM_Gaussian")
    smp.progress = False
    kw = XR.case_kwargs(name)
    seen_t = []
    if "condition_fn" in kw:
        fn = kw["condition_fn"]
        kw["condition_fn"] = lambda xt, t: (seen_t.append(t), fn(xt, t))[1]
    x0 = smp.sampler.sample(S=XR.STEPS, conditioning=c, unconditional_conditioning=uc, x_T=noise, shape=tuple(noise.shape),
                            unconditional_guidance_scale=XR.GUIDANCE, eta=0.0, **kw)
    assert len(calls) == XR.STEPS
    th = smp.sampler.last_thresholds
    if "percentile" in kw:
        assert tuple(th.shape) == (XR.STEPS, 1, 4)
        assert all(k["bound"] is None and k["percentile"] == 0.995 for k in calls)
    else:
        assert th is None
        assert all(k["bound"] == 1.0 and k["percentile"] is None for k in calls)     # clamp=True: [-1, 1] whatever the value
    if seen_t:
        assert [t.tolist() for t in seen_t] == [[751], [501], [251], [1]] and all(t.dtype == torch.long for t in seen_t)
    return x0, th


@pytest.mark.parametrize("name", ["percentile", "clamp03", "clamp50", "percentile_cond"])
def test_sampler_loop_host_logic_matches_reference(cpu_restricted_step, name):
    """The loop with the device binding replaced by the restatement reproduces each golden run of the reference to 2e-5 (max-abs error
    over the golden's max-abs, the CPU gate of tests/test_samplers_cpu.py): the final latent, the x_t of every step, and the s sequence.
    The UNet is stood in for by the reference UNet's recorded answers (`_ReplayModel`), so the comparison is between two LOOPS.  With
    the oracle port as the model (the test below) the port's own fp32 rounding, 2.9e-6 on the x0 of step 0, passes through three more
    guided steps: the percentile runs divide it by s and stay at 4e-6, the clamp runs grow it to 1.17e-4 — an error of the stand-in,
    not of the loop.  (The plain run goes through the cached plan's C entry point, which has no host stand-in:
    tests/test_gpu_x0_threshold.py.)"""
    gold = np.load(os.path.join(GOLD, "modelscope_threshold_tiny.npz"))
    noise, c, uc = _inputs()
    rec = "clamp03" if name == "clamp50" else name                  # clamp=0.3 and clamp=5.0 are one run in the reference (asserted by the generator)
    model = _ReplayModel(gold[f"{rec}_eps"], c, uc)
    x0, th = _run_case(name, model, c, uc, noise, cpu_restricted_step)
    assert [cl[1] for cl in model.calls] == [[t] for t in (751, 751, 501, 501, 251, 251, 1, 1)]
    xts = torch.cat(model.xts)
    errs = [_rel(xts[k], gold[f"{rec}_xt"][k, 0]) for k in range(XR.STEPS)]
    r = _rel(x0, gold[f"{name}_out"])
    print(f"restricted loop on the host ({name}): max-abs error / max-abs vs the reference golden = {r:.3e}; x_t per step {errs}")
    assert torch.equal(xts[0:1], noise) and max(errs) < 2e-5
    if th is not None:
        assert _rel(th[:, 0, 0], gold[f"{name}_s"]) < 2e-5
    assert r < 2e-5                                                 # the CPU gate of tests/test_samplers_cpu.py


@pytest.mark.parametrize("name", ["percentile", "percentile_cond"])
def test_sampler_loop_with_the_oracle_port_as_the_model(cpu_restricted_step, name):
    """The same loop around a real forward (the oracle port, batched cond | uncond as the product evaluates it), same gate.  Only the
    percentile runs: see above for what the port's rounding becomes in a clamp run."""
    gold = np.load(os.path.join(GOLD, "modelscope_threshold_tiny.npz"))
    noise, c, uc = _inputs()
    model = _PortModel()
    x0, th = _run_case(name, model, c, uc, noise, cpu_restricted_step)
    assert len(model.calls) == XR.STEPS
    assert _rel(th[:, 0, 0], gold[f"{name}_s"]) < 2e-5 and _rel(x0, gold[f"{name}_out"]) < 2e-5


def test_percentile_wins_over_clamp_and_bad_arguments_fail_before_any_launch(cpu_restricted_step):
    noise, c, uc = _inputs()
    model = _PortModel()
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name="DDIM_Gaussian")
    kw = dict(S=2, conditioning=c, unconditional_conditioning=uc, x_T=noise, shape=tuple(noise.shape), unconditional_guidance_scale=9.0)
    smp.sampler.sample(percentile=0.9, clamp=0.3, **kw)
    assert [(k["percentile"], k["bound"]) for k in cpu_restricted_step] == [(0.9, None)] * 2
    n_model = len(model.calls)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            smp.sampler.sample(percentile=bad, **kw)
    with pytest.raises(NotImplementedError, match="model_kwargs"):
        smp.sampler.sample(model_kwargs=[c, uc], **kw)
    with pytest.raises(L.T2VError, match="fp32"):
        smp.sampler.sample(percentile=0.9, **dict(kw, x_T=noise.half()))
    model.t_shard = object()
    with pytest.raises(L.T2VError, match="split over ranks"):
        smp.sampler.sample(clamp=1.0, **kw)
    model.t_shard = None
    smp.sampler.shared_noise = samplers.SharedNoise(1, noise.shape[2] + 2, 0, "cpu")
    with pytest.raises(L.T2VError, match="split over ranks"):
        smp.sampler.sample(clamp=1.0, **kw)
    assert len(model.calls) == n_model and len(cpu_restricted_step) == 2


@pytest.mark.parametrize("sampler", ["DDIM", "UniPC"])
def test_other_samplers_refuse_the_keywords(sampler):
    from sd_webui_text2video_amd import pipeline, unet as U
    noise, c, uc = _inputs()
    model = _PortModel()
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=sampler)
    kw = dict(steps=2, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape), noise=noise,
              guidance_scale=9.0, sampler_name=sampler)
    for extra in (dict(percentile=0.995), dict(clamp=1.0)):
        with pytest.raises(ValueError, match=sampler):
            smp.sample_loop(**kw, **extra)
    assert model.calls == []
    net = U.UNetSD(**configs.TINY_UNET, init_weights=False)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, device="cpu")
    for extra in (dict(percentile=0.995), dict(clamp=1.0)):
        with pytest.raises(ValueError, match=sampler):
            pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, sampler=sampler, device="cpu", **extra)
        with pytest.raises(ValueError, match=sampler):
            pipeline.process_modelscope(dict(pipe=pipe, cond=c, uncond=uc, steps=2, frames=3, seed=1, cfg_scale=9.0, width=128, height=128,
                                             sampler=sampler, **extra))


# ---- record validation (no GPU: a refused record launches nothing) -----------------------------------------------------------------
def _record(**kw):
    """A valid mode-0 DDIM_STEP record over made-up addresses, then the overrides: i8, i9, i5, i7, i4, f6, p3, p7, p8, inner, C."""
    op = L.T2VOp()
    op.kind = L.OP_DDIM_STEP
    ptr = 1 << 40
    op.i[0], op.i[1], op.i[2], op.i[6] = kw.get("C", 4), kw.get("inner", 768), 2, 4
    op.i[3], op.i[4], op.i[5], op.i[7] = L.F32, kw.get("i4", L.F32), kw.get("i5", 0), kw.get("i7", 0)
    op.i[8], op.i[9] = kw.get("i8", 0), kw.get("i9", 0)
    for k, v in enumerate([1.7, 1.4, 0.9, 0.3, 0.0, 9.0]):
        op.f[k] = v
    op.f[6], op.f[7] = kw.get("f6", 0.0), kw.get("f7", 0.0)
    op.p[0], op.p[1], op.p[3] = ptr, ptr + (1 << 30), kw.get("p3", ptr + (2 << 30))
    for k in (4, 5, 6, 7, 8):
        op.p[k] = kw.get(f"p{k}", 0)
    return op


def test_record_validation_without_gpu(built_lib):
    ptr = 3 << 40
    lib = built_lib

    def refused(needle=b"DDIM step", **kw):
        rc = lib.t2v_run_ops(ctypes.byref(_record(**kw)), 1, None, 0, None)
        return rc == -1 and b"DDIM step" in lib.t2v_last_error() and needle in lib.t2v_last_error()

    def accepted(**kw):
        h = ctypes.c_void_p()
        rc = lib.t2v_plan_create(ctypes.byref(_record(**kw)), 1, ctypes.byref(h))
        if rc == 0:
            lib.t2v_plan_destroy(h)
        return rc == 0

    nan = float("nan")
    ok1, ok2, ok3 = dict(i8=1, f6=1.0), dict(i8=2, p7=ptr), dict(i8=3, p7=ptr, f6=0.995)
    ok9 = dict(i9=1, p8=ptr, f7=0.5)
    for kw in (ok1, ok2, ok3, ok9, dict(ok1, **ok9), dict(ok2, **ok9), dict(ok3, p3=0), dict(ok3, f6=1.0)):
        assert accepted(**kw), kw
    # i[8] = 0: the new fields are not looked at
    assert accepted(f6=nan, f7=nan, p7=0xdeadbeef000, p8=0xdeadbeef000)
    assert accepted(i5=1, f6=nan, f7=3.0, p7=ptr, p8=ptr) and accepted(i4=L.F16, f6=nan, p7=ptr)
    assert refused(i8=4, p7=ptr) and refused(i8=-1, p7=ptr) and refused(i9=2, p8=ptr) and refused(i9=-1, p8=ptr)
    for ok in (ok1, ok2, ok3, ok9):
        assert refused(b"mode 0", i5=1, **ok), ok                                                     # mode 1 (LDM DDIM)
        assert refused(i5=1, i7=1, p4=ptr, p5=ptr, p6=ptr, **{k: v for k, v in ok.items() if k not in ("f6", "f7")}), ok     # with the mask blend
        assert refused(b"fp32 x", i4=L.F16, **ok), ok                                                 # fp16 x
    assert refused(b"mask blend", i7=1, p4=ptr, p5=ptr, **ok1)                                        # (i[7] = 1 in mode 0 is refused already)
    assert refused(b"p[7]", i8=2) and refused(b"p[7]", i8=3, f6=0.995) and refused(b"p[8]", i9=1)
    assert refused(b"null DDIM step pointer", p3=0, **ok1) and refused(b"null DDIM step pointer", p3=0, **ok2)
    assert refused(b"16 777 216", C=4, inner=4194305, **ok3) and accepted(C=4, inner=4194304, **ok3)
    assert accepted(C=8, inner=4194304, **ok3)                      # two samples of 2^24 elements: the limit is per sample
    for f6 in (0.0, -0.5, 1.0000001, nan):
        assert refused(b"percentile", **dict(ok3, f6=f6)), f6
    assert refused(b"bound", **dict(ok1, f6=-1.0)) and refused(b"bound", **dict(ok1, f6=nan))


def test_binding_builds_one_or_two_records():
    """`percentile`: measure then apply, over the same table row; otherwise one record; the guidance term rides on the apply record."""
    x = torch.zeros(2, 4, 3, 4, 4)
    eps, out, grad, table = torch.zeros(4, 4, 3, 4, 4), torch.zeros_like(x), torch.zeros_like(x), torch.zeros(2, 4)
    coef = [1.7, 1.4, 0.9, 0.3, 0.0, 9.0]
    ops = samplers._ddim_restricted_records(out, x, eps, None, coef, 2, percentile=0.995, table=table, grad=grad, sqrt_1mat=0.5)
    assert [(o.i[8], o.i[9]) for o in ops] == [(3, 0), (2, 1)] and ops[0].p[7] == ops[1].p[7] == table.data_ptr()
    assert ops[0].f[6] == np.float32(0.995) and ops[1].f[7] == 0.5 and ops[1].p[8] == grad.data_ptr()
    assert all((o.i[0], o.i[1], o.i[2], o.i[5], o.i[6], o.i[7]) == (8, 48, 2, 0, 4, 0) for o in ops)
    ops = samplers._ddim_restricted_records(out, x, eps, None, coef, 2, bound=1.0)
    assert [(o.i[8], o.i[9], o.f[6]) for o in ops] == [(1, 0, 1.0)]
    ops = samplers._ddim_restricted_records(out, x, eps, None, coef, 2, grad=grad, sqrt_1mat=0.5)
    assert [(o.i[8], o.i[9]) for o in ops] == [(0, 1)]
    with pytest.raises(L.T2VError):
        samplers._ddim_restricted_records(out, x, eps, None, coef, 2, percentile=0.995, table=table[:1])
    with pytest.raises(L.T2VError):
        samplers._ddim_restricted_records(out, x, eps, None, coef, 2, grad=grad[:, :, :1])
