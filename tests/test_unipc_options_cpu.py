"""CPU: the solver options of the UniPC sampler (uni_pc/uni_pc.py:314-343, 385-400, 551-743) and several videos per batch in the
"DDIM" and "UniPC" samplers.

  * the sampler loop's host arithmetic, with the device bindings replaced by torch restatements of the kernels (tests/test_samplers_cpu.py,
    tests/unipc_ref.py), against what the REAL reference's UniPC class computed per case (tests/golden/make_golden_unipc.py);
  * the launches of a default call, every refusal, the keyword plumbing, `inverse_lambda`;
  * the record validation of T2V_OP_DDIM_STEP mode 2 (no GPU needed: a refused record launches nothing);
  * a batch of two videos against the two single runs, exactly (the restatements are batch-independent).
The kernels themselves: tests/test_gpu_unipc_options.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import unipc_ref as UR
from oracle import configs, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from test_samplers_cpu import _PortModel, _ddim_update_cpu, _lincomb_cpu, _rel

GOLD = os.path.join(os.path.dirname(__file__), "golden", "unipc_options_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture()
def cpu_kernels(monkeypatch):
    """-> the list of launches: ("lincomb", n terms) | ("ddim", mode) | ("threshold", guided)."""
    calls = []
    monkeypatch.setattr(samplers, "_lincomb", lambda out, terms: (calls.append(("lincomb", len(terms))), _lincomb_cpu(out, terms))[1])
    monkeypatch.setattr(samplers, "_ddim_update", lambda *a, **k: (calls.append(("ddim", k.get("mode"))), _ddim_update_cpu(*a, **k))[1])
    monkeypatch.setattr(samplers, "_x0_threshold", lambda *a: (calls.append(("threshold", a[6])), UR.x0_threshold_cpu(*a))[1])
    samplers.state.sampling_step = 0
    return calls


class _ReplayModel:
    """Stands in for the UNet with the REFERENCE UNet's own answers at every evaluation (tests/golden/make_golden_unipc.py): one batched
    [cond | uncond] call per evaluation (one row at guidance 1), at the timestep the reference gave its UNet."""
    supports_cfg_batch = True
    num_timesteps = 1000

    def __init__(self, eps, ts):
        self.eps, self.ts, self.calls = torch.from_numpy(eps), ts, []

    def __call__(self, x, t, cond):
        k = len(self.calls)
        assert x.shape[0] == self.eps.shape[1] and abs(float(t[0]) - self.ts[k]) < 2e-2 and bool((t == t[0]).all()), (k, t, self.ts[k])
        self.calls.append((x.shape[0], t.tolist()))
        return self.eps[k].clone()


def _sampler(model, name="UniPC", **ctor):
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
    smp.progress = False
    if ctor:
        smp.sampler = samplers.UniPCSampler(model, **ctor)
    return smp


def _run(smp, gold, name, **over):
    steps, guidance, strength, kw = UR.CASES[name]
    c, uc, noise = (torch.from_numpy(gold[k]) for k in ("c", "uc", "noise"))
    samplers.state.sampling_step = 0
    return smp.sample_loop(steps=steps, strength=strength, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=None,
                           shape=tuple(noise.shape), noise=noise, guidance_scale=guidance, eta=0.0, sampler_name="UniPC",
                           **dict(dict(unipc=kw), **over))


@pytest.mark.parametrize("name", list(UR.CASES))
def test_each_option_matches_the_reference_class(cpu_kernels, gold, name):
    """Every case within 2e-5 (max-abs error over the golden's max-abs: the UniPC gate of tests/test_samplers_cpu.py) of the latent the
    reference's class computed; the host computes its scalars in float64 where the reference uses fp32 tensors.  The cases of
    unipc_ref.REPLAYED replay the reference UNet's recorded answers, the others (whose answers do not fit the golden file's size limit)
    evaluate the oracle port, as tests/test_samplers_cpu.py does for the default configuration.  Thresholded cases: q and s of every
    evaluation too."""
    steps = UR.CASES[name][0]
    model = _ReplayModel(gold[f"{name}_eps"], gold[f"{name}_t"]) if name in UR.REPLAYED else _PortModel()
    smp = _sampler(model)
    x0 = _run(smp, gold, name)
    evals = UR.evaluations(name)
    r = _rel(x0, gold[f"{name}_out"])
    print(f"UniPC {name} on the host: max-abs error / max-abs vs the reference golden = {r:.3e}")
    assert len(model.calls) == evals and samplers.state.sampling_step == steps         # one callback per step, none for denoise_to_zero
    th = smp.sampler.last_thresholds
    if name in UR.THRESHOLDED:
        assert tuple(th.shape) == (evals, 1, 4) and cpu_kernels.count(("threshold", UR.CASES[name][1] != 1.0)) == evals
        rq, rs = _rel(th[:, 0, 1], gold[f"{name}_q"]), _rel(th[:, 0, 0], gold[f"{name}_s"])
        print(f"    q per evaluation {th[:, 0, 1].tolist()}  (error {rq:.3e}; s {rs:.3e})")
        assert rq < 2e-5 and rs < 2e-5 and (gold[f"{name}_q"] > 1).any()
        assert float(x0.abs().max()) <= 1.0 + 1e-6 if UR.CASES[name][3].get("denoise_to_zero") else True
    else:
        assert th is None and all(k[0] == "lincomb" for k in cpu_kernels)
    assert r < 2e-5


def test_default_call_issues_the_launches_it_issued(cpu_kernels, gold):
    """No keyword: S data predictions of 3 terms and, per step, a predictor and (but for the last) a corrector — LINCOMB records only,
    the counts of the sampler as it was; the result is the golden of tests/golden/make_golden.py."""
    tiny = np.load(os.path.join(os.path.dirname(GOLD), "tiny.npz"))
    c, uc, noise = (torch.from_numpy(gold[k]) for k in ("c", "uc", "noise"))
    model = _PortModel()
    smp = _sampler(model)
    x0 = smp.sample_loop(steps=6, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=None,
                         shape=tuple(noise.shape), noise=noise, guidance_scale=9.0, eta=0.0, sampler_name="UniPC")
    assert _rel(x0, tiny["unipc_x0"]) < 2e-5
    # terms: prediction 3; predictor 2 / 3 / 4 at order 1 / 2 / 3; corrector one more
    want = [3] + [2, 3, 3] + [3, 3, 4] + [4, 3, 5] * 2 + [3, 3, 4] + [2]
    assert [k[0] for k in cpu_kernels] == ["lincomb"] * 17 and [k[1] for k in cpu_kernels] == want
    assert smp.sampler.last_thresholds is None
    # ... and explicit defaults are the same call
    first = list(cpu_kernels)
    del cpu_kernels[:]
    x1 = smp.sample_loop(steps=6, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=None,
                         shape=tuple(noise.shape), noise=noise, guidance_scale=9.0, eta=0.0, sampler_name="UniPC",
                         unipc=dict(variant="bh1", skip_type="time_uniform", order=3, lower_order_final=True, initial_corrector=True,
                                    denoise_to_zero=False, thresholding=False))
    assert torch.equal(x0, x1) and cpu_kernels == first


def test_sample_keyword_wins_over_the_constructor(cpu_kernels, gold):
    model = _ReplayModel(gold["order2_bh2_2steps_eps"], gold["order2_bh2_2steps_t"])
    smp = _sampler(model, variant="bh1", order=2)
    assert _rel(_run(smp, gold, "order2_bh2_2steps", unipc=dict(variant="bh2")), gold["order2_bh2_2steps_out"]) < 2e-5
    model.calls.clear()
    x_bh1 = _run(smp, gold, "order2_bh2_2steps", unipc=None)            # the constructor's bh1: another latent
    assert _rel(x_bh1, gold["order2_bh2_2steps_out"]) > 1e-3


def test_refusals(cpu_kernels, gold):
    c, uc, noise = (torch.from_numpy(gold[k]) for k in ("c", "uc", "noise"))
    model = _PortModel()
    smp = _sampler(model)
    kw = dict(S=3, batch_size=1, shape=tuple(noise.shape), conditioning=c, x_T=noise, unconditional_guidance_scale=9.0,
              unconditional_conditioning=uc)
    with pytest.raises(ValueError, match="vary_coeff.*cannot run on a video latent"):
        smp.sampler.sample(variant="vary_coeff", **kw)
    for key, bad in (("variant", "bh3"), ("skip_type", "uniform"), ("order", 4), ("order", 0), ("order", True), ("lower_order_final", 1),
                     ("initial_corrector", "no"), ("denoise_to_zero", 0), ("thresholding", 0.995)):
        with pytest.raises(ValueError, match=key):
            smp.sampler.sample(**{key: bad}, **kw)
        with pytest.raises(ValueError, match=key):
            samplers.UniPCSampler(model, **{key: bad})
        with pytest.raises(ValueError, match=key):
            smp.sample_loop(steps=3, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape),
                            noise=noise, guidance_scale=9.0, sampler_name="UniPC", unipc={key: bad})
    for extra in (dict(predict_x0=False), dict(method="singlestep"), dict(method="adaptive"), dict(max_val=2.0)):
        with pytest.raises(NotImplementedError, match=next(iter(extra))):
            smp.sampler.sample(**extra, **kw)
    with pytest.raises(ValueError, match="varient"):
        smp.sample_loop(steps=3, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape),
                        noise=noise, guidance_scale=9.0, sampler_name="UniPC", unipc=dict(varient="bh2"))
    with pytest.raises(AssertionError):                                  # steps >= order, as the reference (uni_pc.py:692)
        smp.sampler.sample(**dict(kw, S=2))
    smp.sampler.sample(order=2, **dict(kw, S=2))
    n_model, n_launch = len(model.calls), len(cpu_kernels)
    with pytest.raises(L.T2VError, match="fp32"):
        smp.sampler.sample(thresholding=True, **dict(kw, x_T=noise.half()))
    model.t_shard = object()
    with pytest.raises(L.T2VError, match="split over ranks"):
        smp.sampler.sample(thresholding=True, **kw)
    with pytest.raises(AssertionError, match="one video per batch"):
        smp.sampler.sample(**dict(kw, x_T=torch.cat([noise, noise])))
    model.t_shard = None
    smp.sampler.cfg_parallel = type("Pair", (), dict(size=2, role=0))()
    with pytest.raises(AssertionError, match="CFG-pair"):
        smp.sampler.sample(**dict(kw, x_T=torch.cat([noise, noise])))
    smp.sampler.cfg_parallel = None
    assert len(model.calls) == n_model and len(cpu_kernels) == n_launch
    # the binding: fp16 x, n > 2^24 per video and a wrong table are refused before any launch
    x = torch.zeros(2, 4, 3, 4, 4)
    eps, out, table = torch.zeros(4, 4, 3, 4, 4), torch.zeros_like(x), torch.zeros(2, 4)
    ops = samplers._x0_threshold_records(out, x, eps, 0.5, 0.8, 9.0, True, table)
    assert [(o.i[5], o.i[8]) for o in ops] == [(2, 3), (2, 2)] and ops[0].p[7] == ops[1].p[7] == table.data_ptr()
    assert all((o.i[0], o.i[1], o.i[2], o.i[6], o.i[7], o.i[9]) == (8, 48, 4, 4, 0, 0) for o in ops)
    assert ops[0].f[6] == np.float32(0.995) and ops[0].f[0] == 0.5 and ops[1].f[1] == np.float32(0.8) and ops[1].f[5] == 9.0
    assert [o.i[2] for o in samplers._x0_threshold_records(out, x, eps[:2], 0.5, 0.8, 1.0, False, table)] == [0, 0]
    with pytest.raises(L.T2VError, match="fp32"):
        samplers._x0_threshold_records(out, x.half(), eps, 0.5, 0.8, 9.0, True, table)
    with pytest.raises(L.T2VError, match="table"):
        samplers._x0_threshold_records(out, x, eps, 0.5, 0.8, 9.0, True, table[:1])
    big = torch.empty(1).expand(1, 4, 4194305)                           # (a view without storage: only its shape is looked at)
    with pytest.raises(L.T2VError, match="16 777 216"):
        samplers._x0_threshold_records(big, big, big, 0.5, 0.8, 9.0, False, table[:1].contiguous())


@pytest.mark.parametrize("sampler", ["DDIM", "DDIM_Gaussian"])
def test_other_samplers_refuse_the_keyword(sampler):
    from sd_webui_text2video_amd import pipeline, unet as U
    g = np.load(GOLD)
    c, uc, noise = (torch.from_numpy(g[k]) for k in ("c", "uc", "noise"))
    model = _PortModel()
    smp = _sampler(model, sampler)
    with pytest.raises(ValueError, match=f"unipc.*{sampler}"):
        smp.sample_loop(steps=2, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape),
                        noise=noise, guidance_scale=9.0, sampler_name=sampler, unipc=dict(variant="bh2"))
    assert model.calls == []
    pipe = pipeline.TextToVideoSynthesis(sd_model=U.UNetSD(**configs.TINY_UNET, init_weights=False), device="cpu")
    with pytest.raises(ValueError, match=f"unipc.*{sampler}"):
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, sampler=sampler, device="cpu", unipc=dict(variant="bh2"))
    with pytest.raises(ValueError, match=f"unipc.*{sampler}"):
        pipeline.process_modelscope(dict(pipe=pipe, cond=c, uncond=uc, steps=2, frames=3, seed=1, cfg_scale=9.0, width=128, height=128,
                                         sampler=sampler, unipc=dict(variant="bh2")))
    with pytest.raises(NotImplementedError, match="img2vid"):            # several videos per batch: not for the img2vid route
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, sampler=sampler, device="cpu", videos=2, latents=noise, mask=torch.ones_like(noise))


def test_inverse_lambda_round_trips_lam():
    ac = torch.cumprod(1 - tp.beta_schedule_linear_sd(), 0)
    ns = samplers._VPSchedule(ac)
    for t in (1.0, 0.9995, 0.7, 0.5005, 0.25, 0.0123, 0.0015, 0.001):
        assert abs(ns.inverse_lambda(ns.lam(t)) - t) < 1e-9, t
    lams = [ns.lam(t) for t in (1.0, 0.5, 0.001)]
    assert lams[0] < lams[1] < lams[2]                                   # the half-logSNR rises as t falls
    assert ns.inverse_lambda(0.5 * (lams[0] + lams[1])) > 0.5


# ---- record validation (no GPU: a refused record launches nothing) -----------------------------------------------------------------
def _record(**kw):
    """A valid mode-2 DDIM_STEP record over made-up addresses, then the overrides."""
    op = L.T2VOp()
    op.kind = L.OP_DDIM_STEP
    ptr = 1 << 40
    op.i[0], op.i[1], op.i[2], op.i[6] = kw.get("C", 4), kw.get("inner", 768), kw.get("i2", 4), kw.get("i6", 4)
    op.i[3], op.i[4], op.i[5], op.i[7] = L.F32, kw.get("i4", L.F32), kw.get("i5", 2), kw.get("i7", 0)
    op.i[8], op.i[9] = kw.get("i8", 2), kw.get("i9", 0)
    op.f[0], op.f[1], op.f[5], op.f[6] = 0.5, 0.8, 9.0, kw.get("f6", 0.995)
    op.p[0], op.p[1], op.p[3], op.p[7] = ptr, ptr + (1 << 30), kw.get("p3", ptr + (2 << 30)), kw.get("p7", 3 << 40)
    return op


def test_mode2_record_validation_without_gpu(built_lib):
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

    assert accepted(i8=2) and accepted(i8=3) and accepted(i8=3, p3=0) and accepted(i8=2, i2=0) and accepted(i8=3, f6=1.0)
    assert accepted(C=12, i8=3)                                          # three videos
    assert refused(b"mode 2", i8=1) and refused(b"mode 2", i8=0) and refused(i8=4)
    assert refused(b"fp32 x", i4=L.F16, i8=2) and refused(b"fp32 x", i4=L.F16, i8=3)
    assert refused(b"16 777 216", inner=4194305, i8=3) and refused(b"16 777 216", inner=4194305, i8=2)
    assert accepted(inner=4194304, i8=3) and accepted(C=8, inner=4194304, i8=2)      # the limit is per video
    assert refused(b"p[7]", p7=0, i8=2) and refused(b"p[7]", p7=0, i8=3) and refused(b"null DDIM step pointer", p3=0, i8=2)
    assert refused(b"mode 2", i7=1) and refused(b"mode 2", i9=1) and refused(b"all channels", i2=2)
    for f6 in (0.0, -0.5, 1.0000001, float("nan")):
        assert refused(b"quantile", i8=3, f6=f6), f6
    assert refused(i5=3) and refused(i5=-1)
    # records of mode 0 and mode 1 are validated as before
    assert accepted(i5=0, i8=0, i2=2) and accepted(i5=1, i8=0, i2=2) and refused(b"mode 0", i5=1, i8=2)


# ---- several videos per batch ------------------------------------------------------------------------------------------------------
class _ToyModel:
    """A UNet stand-in whose answer for a video depends on that video's rows only, through exactly rounded elementwise operations: a
    batch is bitwise its single runs (a real forward's GEMM blocking on the host is not batch-independent)."""
    supports_cfg_batch = True
    num_timesteps = 1000

    def __init__(self):
        self.calls = []

    def __call__(self, x, t, c):
        self.calls.append((x.shape[0], t.tolist()))
        k = (c[:, 0, 0].float() * 0.05 + t.float() * 1e-4).view(-1, 1, 1, 1, 1)
        return x.float() * 0.8 + x.float().roll(1, -1) * k


def _two(gold):
    c, uc = torch.from_numpy(gold["c"]), torch.from_numpy(gold["uc"])
    noises = [torch.randn(tuple(gold["noise"].shape), generator=torch.Generator().manual_seed(40 + v)) for v in range(2)]
    return c, uc, noises


@pytest.mark.parametrize("opts", [None, dict(thresholding=True, variant="bh2", denoise_to_zero=True)], ids=["default", "thresholded"])
def test_unipc_batch_of_two_equals_the_single_runs(cpu_kernels, gold, opts):
    c, uc, noises = _two(gold)
    model = _ToyModel()
    smp = _sampler(model)
    kw = dict(steps=3, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=None, guidance_scale=9.0,
              eta=0.0, sampler_name="UniPC", **({} if opts is None else dict(unipc=opts)))
    singles, tables = [], []
    for n in noises:
        singles.append(smp.sample_loop(shape=tuple(n.shape), noise=n, **kw))
        tables.append(smp.sampler.last_thresholds)
    launches = len(cpu_kernels) // 2
    del cpu_kernels[:]
    model.calls.clear()
    both = smp.sample_loop(shape=(2,) + tuple(noises[0].shape[1:]), noise=torch.cat(noises), **dict(kw, batch_size=2))
    assert len(cpu_kernels) == launches                                  # the launches of ONE run, over the whole batch
    assert [cl[0] for cl in model.calls] == [4] * (3 + (1 if opts else 0))          # one 2V-row forward per evaluation, one timestep
    assert all(len(set(cl[1])) == 1 for cl in model.calls)
    for v in range(2):
        assert torch.equal(both[v:v + 1], singles[v]), v
    assert not torch.equal(both[0], both[1])
    if opts:
        th = smp.sampler.last_thresholds
        assert tuple(th.shape) == (4, 2, 4)
        for v in range(2):
            assert torch.equal(th[:, v], tables[v][:, 0]), v
        assert not torch.equal(th[:, 0], th[:, 1])                       # each video has its own s
    # per-video conditioning is taken per video: the same rows, stacked, give the same batch
    again = smp.sample_loop(shape=(2,) + tuple(noises[0].shape[1:]), noise=torch.cat(noises),
                            **dict(kw, batch_size=2, conditioning=c.repeat(2, 1, 1), unconditional_conditioning=uc.repeat(2, 1, 1)))
    assert torch.equal(again, both)


def test_ddim_gaussian_noising_of_a_batch(cpu_kernels, gold):
    """vid2vid with DDIM_Gaussian: `encode_latent` repeats the one clip's latents, each video its own noise.  (Its plain step goes
    through the C entry point, which has no host stand-in: tests/test_gpu_unipc_options.py.)"""
    c, uc, noises = _two(gold)
    smp = _sampler(_ToyModel(), "DDIM_Gaussian")
    z0 = torch.randn(noises[0].shape, generator=torch.Generator().manual_seed(11))
    enc, dsteps = smp.encode_latent(z0, torch.cat(noises), 0.75, 4)
    assert dsteps == 3 and tuple(enc.shape) == (2,) + tuple(z0.shape[1:])
    for v in range(2):
        assert torch.equal(enc[v:v + 1], smp.encode_latent(z0, noises[v], 0.75, 4)[0])


@pytest.mark.parametrize("sampler", ["DDIM", "UniPC"])
@pytest.mark.parametrize("vid2vid", [False, True], ids=["txt2vid", "vid2vid"])
def test_batch_of_two_through_sample_loop(cpu_kernels, gold, sampler, vid2vid):
    """txt2vid and vid2vid (one clip's latents repeated, each video its own noise): each video equals its own single run, exactly."""
    c, uc, noises = _two(gold)
    z0 = torch.randn(noises[0].shape, generator=torch.Generator().manual_seed(11)) if vid2vid else None
    kw = dict(steps=4, strength=0.75 if vid2vid else None, conditioning=c, unconditional_conditioning=uc, latents=z0,
              is_vid2vid=vid2vid, guidance_scale=9.0, eta=0.0, sampler_name=sampler)
    singles = []
    for n in noises:
        smp = _sampler(_ToyModel(), sampler)                            # (vid2vid rebinds DDIM's `sample`: a sampler per run)
        singles.append(smp.sample_loop(batch_size=1, shape=tuple(n.shape), noise=n, **kw))
    model = _ToyModel()
    smp = _sampler(model, sampler)
    both = smp.sample_loop(batch_size=2, shape=(2,) + tuple(noises[0].shape[1:]), noise=torch.cat(noises), **kw)
    assert tuple(both.shape) == (2,) + tuple(noises[0].shape[1:]) and all(cl[0] == 4 for cl in model.calls)
    for v in range(2):
        assert torch.equal(both[v:v + 1], singles[v]), v
    assert _rel(both[0], both[1].numpy()) > 0.1


def test_process_modelscope_one_pass_route_takes_vid2vid_and_the_unipc_key():
    """`batch_count` videos of a vid2vid call with (cond, uncond) and no stitch stage are ONE `infer_conditioned(videos=batch_count)` call
    with the clip's latents, steps - skip_steps and the `unipc` dict; one video, a stitch stage or img2vid keep the loop."""
    from sd_webui_text2video_amd import pipeline
    from test_pipeline_cpu import _FakePipe, _args
    pipe = _FakePipe()
    lat = torch.randn(1, 4, 3, 1, 2)
    opts = dict(variant="bh2", thresholding=True)
    side = pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=lat, strength=0.5, cond="C", uncond="U", batch_count=3,
                                             sampler="UniPC", unipc=opts))
    assert pipe.calls == [("cond", 7 - 3, 3, 40, 9.0, 3)] and side[0].shape == (8, 48, 3)
    assert torch.equal(pipe.kw["latents"], lat) and pipe.kw["strength"] == 0.5 and pipe.kw["is_vid2vid"] is True and pipe.kw["unipc"] == opts
    pipe.calls.clear()
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=lat, strength=0.5, cond="C", uncond="U"))
    assert pipe.calls == [("cond", 7 - 3, 3, 40, 9.0, 1)] and "unipc" not in pipe.kw             # without the key nothing is forwarded
    pipe.calls.clear()
    pipeline.process_modelscope(_args(pipe, do_vid2vid=True, vid2vid_frames=lat, strength=0.5, cond="C", uncond="U", batch_count=2,
                                      stitch=lambda fr, info: b"x"))
    assert [cl[3] for cl in pipe.calls] == [40, 41] and all(cl[5] == 1 for cl in pipe.calls)    # the stitch stage keeps the loop
