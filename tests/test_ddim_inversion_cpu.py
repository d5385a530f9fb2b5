"""CPU: DDIM inversion (`DDIMSampler.encode`, ddim/sampler.py:222-267), the vid2vid route through it, and `temperature` / `ucg_schedule`
of `DDIMSampler.sample` — host logic against golden outputs of the REAL reference (tests/golden/make_golden_inversion.py).

As in tests/test_samplers_cpu.py the device bindings are replaced by torch restatements (`_ddim_invert` by tests/inversion_ref.py) and the
UNet by the oracle port, so only the product's own host arithmetic is under test; the record validation of T2V_OP_DDIM_STEP mode 3 needs
no GPU (a refused record launches nothing).  The kernel itself: tests/test_gpu_ddim_inversion.py."""
import ctypes

import numpy as np
import pytest
import torch

import inversion_ref as IR
from oracle import configs, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from test_samplers_cpu import _ddim_update_cpu, _lincomb_cpu, _PortModel, _rel


class _ListPortModel(_PortModel):
    """The oracle port with the product's batched entry: one `forward_cfg_pair` call per step, contexts as a [cond | uncond] tensor, a
    (cond, uncond) pair, or two lists of one context per video (any lengths)."""

    def _eval(self, x, t, ctx):
        if isinstance(ctx, (list, tuple)):
            return torch.cat([tp.unet_forward(self.sd, configs.TINY_UNET, x[v:v + 1].float(), t[v:v + 1], ctx[v]) for v in range(x.shape[0])])
        return tp.unet_forward(self.sd, configs.TINY_UNET, x.float(), t, ctx)

    def __call__(self, x, t, c):
        self.calls.append((x.shape[0], t.tolist()))
        return self._eval(x, t, c)

    def forward_cfg_pair(self, x, t, ctx, context_token=None, single_t=None):
        self.calls.append((2 * x.shape[0], t.tolist()))
        c, uc = ctx if isinstance(ctx, tuple) else ctx.chunk(2, dim=0)
        return torch.cat([self._eval(x, t, c), self._eval(x, t, uc)])


@pytest.fixture()
def cpu_kernels(monkeypatch):
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update", _ddim_update_cpu)
    monkeypatch.setattr(samplers, "_ddim_invert", IR.invert_cpu)
    samplers.state.sampling_step = 0


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(IR.GOLD))


def _sampler(model, name="DDIM"):
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
    smp.progress = False
    return smp


def test_encode_matches_the_reference(cpu_kernels, gold):
    z0, _, c, uc = IR.inputs()
    model = _PortModel()
    s = _sampler(model).sampler
    s.make_schedule(4)
    seen = []
    x, info = s.encode(z0, c, 3, callback=seen.append)
    r = {"enc_plain": _rel(x, gold["enc_plain"])}
    assert x.dtype == torch.float32 and info["x_encoded"] is x and info["intermediate_steps"] == [] and "intermediates" not in info
    assert seen == [0, 1, 2]
    assert [cl for cl in model.calls] == [(1, [0.0]), (1, [1.0]), (1, [2.0])]              # the quirk: t = i, one call per step
    model.calls.clear()
    xg, _ = s.encode(z0, c, 3, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)
    r["enc_guided"] = _rel(xg, gold["enc_guided"])
    assert [cl for cl in model.calls] == [(2, [0.0, 0.0]), (2, [1.0, 1.0]), (2, [2.0, 2.0])]   # one batched call per step
    xo, _ = s.encode(z0, c, 5, use_original_steps=True)
    r["enc_orig"] = _rel(xo, gold["enc_orig"])
    print("encode on the host vs the reference golden (max-abs / max-abs):", r)
    assert max(r.values()) < 2e-5
    assert torch.equal(z0, IR.inputs()[0])                          # the caller's latent is not written


def test_return_intermediates_bookkeeping(cpu_kernels, gold):
    z0, _, c, _ = IR.inputs()
    s = _sampler(_PortModel()).sampler
    s.make_schedule(6)
    assert s.ddim_timesteps.shape[0] == 7
    x, info = s.encode(z0, c, 5, return_intermediates=2)
    assert info["intermediate_steps"] == [0, 2, 3, 4] == gold["enc_inter_steps"].tolist()
    assert _rel(x, gold["enc_inter"]) < 2e-5
    assert len(info["intermediates"]) == 4
    for k, t in enumerate(info["intermediates"]):
        assert _rel(t, gold["enc_inter_intermediates"][k]) < 2e-5, k
    assert torch.equal(info["intermediates"][-1], x)
    s.encode(z0, c, 7)                                              # t_enc == the size of the timestep table passes ...
    with pytest.raises(AssertionError):
        s.encode(z0, c, 8)                                          # ... one more does not (sampler.py:227)
    with pytest.raises(ValueError, match=r"6.*5"):
        s.encode(z0, c, 5, return_intermediates=6)                  # (the reference divides by zero)
    with pytest.raises(ValueError, match="model_timesteps"):
        s.encode(z0, c, 5, model_timesteps="ddim")


def test_model_timestep_labels(cpu_kernels):
    z0, _, c, uc = IR.inputs()
    model = _PortModel()
    s = _sampler(model).sampler
    s.make_schedule(4)
    s.encode(z0, c, 3, model_timesteps="index")
    assert [cl[1] for cl in model.calls] == [[0.0], [1.0], [2.0]]
    model.calls.clear()
    s.encode(z0, c, 3, unconditional_guidance_scale=9.0, unconditional_conditioning=uc, model_timesteps="schedule")
    assert [cl for cl in model.calls] == [(2, [1.0, 1.0]), (2, [251.0, 251.0]), (2, [501.0, 501.0])]      # decode's (timestep, level) pairs
    model.calls.clear()
    a, _ = s.encode(z0, c, 3, use_original_steps=True, model_timesteps="schedule")       # original steps: the two labels coincide
    b, _ = s.encode(z0, c, 3, use_original_steps=True, model_timesteps="index")
    assert [cl[1] for cl in model.calls] == [[0.0], [1.0], [2.0]] * 2 and torch.equal(a, b)


def test_batches_equal_their_single_runs(cpu_kernels):
    z0, _, c, uc = IR.inputs()
    g = torch.Generator().manual_seed(21)
    z1 = torch.randn(IR.SHAPE, generator=g)
    c_long = torch.randn(1, 11, 1024, generator=g)
    model = _ListPortModel()
    s = _sampler(model).sampler
    s.make_schedule(4)
    kw = dict(unconditional_guidance_scale=9.0, model_timesteps="schedule")
    singles = [s.encode(z, cc, 3, unconditional_conditioning=uc, **kw)[0] for z, cc in ((z0, c), (z1, c), (z1, c_long))]
    model.calls.clear()
    two, _ = s.encode(torch.cat([z0, z1]), c, 3, unconditional_conditioning=uc, **kw)
    assert len(model.calls) == 3 and all(cl[0] == 4 for cl in model.calls)                # one 2 x videos forward per step
    assert _rel(two[0:1], singles[0].numpy()) < 2e-5 and _rel(two[1:2], singles[1].numpy()) < 2e-5
    model.calls.clear()
    ragged, _ = s.encode(torch.cat([z0, z1]), [c, c_long], 3, unconditional_conditioning=uc, **kw)       # 7 and 11 tokens
    assert len(model.calls) == 3
    assert _rel(ragged[0:1], singles[0].numpy()) < 2e-5 and _rel(ragged[1:2], singles[2].numpy()) < 2e-5
    plain, _ = s.encode(torch.cat([z0, z1]), [c, c_long], 3, model_timesteps="schedule")                 # unguided lists
    assert _rel(plain[1:2], s.encode(z1, c_long, 3, model_timesteps="schedule")[0].numpy()) < 2e-5


@pytest.mark.parametrize("k", range(len(IR.ROUNDTRIPS)))
def test_constant_eps_round_trip(cpu_kernels, gold, k):
    """With an eps that depends neither on x nor on t, decode(encode(x0, n), n) is the algebraic identity; what is left is the fp32
    arithmetic.  Gate: 4 x the error of the reference's own arithmetic on the same identity (roundtrip_ref_rel), floor 1e-6."""
    S, n = IR.ROUNDTRIPS[k]
    z0, _, c, _ = IR.inputs()
    rels = {}
    for labels in ("schedule", "index"):
        model = IR.ConstEpsModel(IR.const_eps())
        s = _sampler(model).sampler
        s.make_schedule(S)
        enc, _ = s.encode(z0, c, n, model_timesteps=labels)
        rels[labels] = IR.rel_l2(s.decode(enc, c, n), z0)
    ref = float(gold["roundtrip_ref_rel"][k])
    print(f"constant-eps round trip S={S} n={n}: {rels} (the reference's arithmetic: {ref:.3e})")
    assert rels["schedule"] <= max(1e-6, 4 * ref)
    assert rels["index"] == rels["schedule"]                        # the labels change what the UNet is asked, not the formulas


def test_temperature_and_ucg_schedule(cpu_kernels, gold):
    _, noise, c, uc = IR.inputs()
    model = _PortModel()
    s = _sampler(model).sampler
    kw = dict(S=4, batch_size=1, shape=tuple(noise.shape), conditioning=c, x_T=noise, unconditional_guidance_scale=9.0,
              unconditional_conditioning=uc)
    torch.manual_seed(IR.NOISE_SEED)
    x = s.sample(eta=1.0, temperature=IR.TEMPERATURE, **kw)
    assert _rel(x, gold["ddim_temp_x0"]) < 2e-5
    torch.manual_seed(IR.NOISE_SEED)
    assert _rel(s.sample(eta=1.0, **kw), gold["ddim_temp_x0"]) > 1e-2            # the keyword is what makes the difference
    x = s.sample(eta=0.0, ucg_schedule=list(IR.UCG_SCHEDULE), **kw)
    assert _rel(x, gold["ddim_ucg_x0"]) < 2e-5
    with pytest.raises(AssertionError):
        s.sample(eta=0.0, ucg_schedule=[9.0, 7.0, 5.0], **kw)                    # sampler.py:151
    base = np.load(IR.GOLD.replace("ddim_inversion_tiny", "tiny"))["ddim_x0"]
    assert _rel(s.sample(eta=0.0, **kw), base) < 2e-5                            # the defaults: the call it was


def _loop_kw(noise, c, uc, z0, **more):
    return dict(steps=4, strength=0.75, conditioning=c, unconditional_conditioning=uc, batch_size=1, latents=z0, shape=tuple(noise.shape),
                noise=noise, is_vid2vid=True, guidance_scale=9.0, eta=0.0, sampler_name="DDIM", **more)


def test_sample_loop_inversion_route(cpu_kernels, gold):
    z0, noise, c, uc = IR.inputs()
    model = _PortModel()
    smp = _sampler(model)
    x0 = smp.sample_loop(**_loop_kw(noise, c, uc, z0, inversion=True))
    assert _rel(x0, gold["vid2vid_inverted_x0"]) < 2e-5
    # three inversion steps under the prompt at the reference's labels, then decode's three guided steps
    assert [cl for cl in model.calls] == [(1, [0.0]), (1, [1.0]), (1, [2.0]), (2, [501.0] * 2), (2, [251.0] * 2), (2, [1.0] * 2)]
    model.calls.clear()
    smp = _sampler(model)
    smp.sample_loop(**_loop_kw(noise, c, uc, z0, inversion=dict(guidance_scale=3.0, model_timesteps="schedule")))
    assert [cl for cl in model.calls][:3] == [(2, [1.0] * 2), (2, [251.0] * 2), (2, [501.0] * 2)]
    # without the keyword: the noising route, as before
    tiny = np.load(IR.GOLD.replace("ddim_inversion_tiny", "tiny"))
    x0 = _sampler(_PortModel()).sample_loop(**_loop_kw(noise, c, uc, z0))
    assert _rel(x0, tiny["ddim_vid2vid_x0"]) < 2e-5
    x0 = _sampler(_PortModel()).sample_loop(**_loop_kw(noise, c, uc, z0, inversion=None))
    assert _rel(x0, tiny["ddim_vid2vid_x0"]) < 2e-5


def test_refusals(cpu_kernels):
    from sd_webui_text2video_amd import pipeline, unet as U
    z0, noise, c, uc = IR.inputs()
    model = _PortModel()
    for name in ("DDIM_Gaussian", "UniPC"):
        with pytest.raises(ValueError, match=name):
            _sampler(model, name).sample_loop(**dict(_loop_kw(noise, c, uc, z0, inversion=True), sampler_name=name))
    with pytest.raises(ValueError, match="vid2vid"):
        _sampler(model).sample_loop(**dict(_loop_kw(noise, c, uc, z0, inversion=True), is_vid2vid=False))
    with pytest.raises(ValueError, match="vid2vid"):
        _sampler(model).sample_loop(**dict(_loop_kw(noise, c, uc, z0, inversion=True), latents=None))
    with pytest.raises(ValueError, match=r"'scale'.*guidance_scale, model_timesteps"):
        _sampler(model).sample_loop(**_loop_kw(noise, c, uc, z0, inversion=dict(scale=2.0)))
    smp = _sampler(model)

    class _Pair:
        size, role = 2, 0
    smp.sampler.cfg_parallel = _Pair()
    with pytest.raises(L.T2VError, match="CFG-pair"):
        smp.sample_loop(**_loop_kw(noise, c, uc, z0, inversion=True))
    smp.sampler.cfg_parallel = None
    model.t_shard = object()
    with pytest.raises(L.T2VError, match="split over ranks"):
        smp.sample_loop(**_loop_kw(noise, c, uc, z0, inversion=True))
    model.t_shard = None
    assert model.calls == []
    # the public route carries the keyword down and the refusal up
    net = U.UNetSD(**configs.TINY_UNET, init_weights=False)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, device="cpu")
    with pytest.raises(ValueError, match="DDIM_Gaussian"):
        pipe.infer_conditioned(c, uc, 4, 3, 1, 9.0, 128, 128, sampler="DDIM_Gaussian", device="cpu", latents=z0, strength=0.75,
                               is_vid2vid=True, inversion=True)
    with pytest.raises(ValueError, match="vid2vid"):
        pipeline.process_modelscope(dict(pipe=pipe, cond=c, uncond=uc, steps=4, frames=3, seed=1, cfg_scale=9.0, width=128, height=128,
                                         sampler="DDIM", inversion=True))


# ---- record validation (no GPU: a refused record launches nothing) -----------------------------------------------------------------
def _record(**kw):
    """A valid mode-3 DDIM_STEP record over made-up addresses, then the overrides."""
    op = L.T2VOp()
    op.kind = L.OP_DDIM_STEP
    ptr = 1 << 40
    op.i[0], op.i[1], op.i[2], op.i[6] = kw.get("C", 8), kw.get("inner", 768), kw.get("i2", 4), 4
    op.i[3], op.i[4], op.i[5] = kw.get("i3", L.F32), kw.get("i4", L.F32), 3
    op.i[7], op.i[8], op.i[9] = kw.get("i7", 0), kw.get("i8", 0), kw.get("i9", 0)
    op.f[0], op.f[1], op.f[5] = 1.7, 0.4, 9.0
    op.p[0], op.p[1], op.p[3], op.p[4] = ptr, ptr + (1 << 30), kw.get("p3", ptr + (2 << 30)), kw.get("p4", 0)
    return op


def test_record_validation_without_gpu(built_lib):
    lib = built_lib

    def refused(needle=b"DDIM", **kw):
        rc = lib.t2v_run_ops(ctypes.byref(_record(**kw)), 1, None, 0, None)
        return rc == -1 and b"DDIM" in lib.t2v_last_error() and needle in lib.t2v_last_error()

    def accepted(**kw):
        h = ctypes.c_void_p()
        rc = lib.t2v_plan_create(ctypes.byref(_record(**kw)), 1, ctypes.byref(h))
        if rc == 0:
            lib.t2v_plan_destroy(h)
        return rc == 0

    assert accepted() and accepted(i2=0) and accepted(i3=L.F16) and accepted(p4=(1 << 40) + (3 << 30))
    assert refused(b"fp32 x", i4=L.F16)
    for part in (1, 2, 3):
        assert refused(b"all channels", i2=part), part                # guidance over some channels only
    assert refused(i2=5) and refused(i2=-1)
    for field in ("i7", "i8", "i9"):
        assert refused(b"mode 3", **{field: 1}), field
    assert refused(b"mode 3", i8=3, p3=0)
    assert refused(b"null DDIM step pointer", p3=0)


def test_binding_builds_the_mode3_record(monkeypatch):
    seen = []

    class _Lib:
        def t2v_run_ops(self, op, n, ext, n_ext, stream):
            o = op._obj
            seen.append(([o.i[k] for k in range(10)], [o.f[k] for k in (0, 1, 5)], [o.p[k] for k in range(5)], n))
            return 0
    monkeypatch.setattr(L, "load", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 0})())
    x = torch.zeros(2, 4, 3, 4, 4)
    eps, out, keep = torch.zeros(4, 4, 3, 4, 4, dtype=torch.float16), torch.zeros_like(x), torch.zeros_like(x)
    samplers._ddim_invert(out, x, eps, (1.5, 0.25, 9.0), True, keep=keep)
    samplers._ddim_invert(out, x, eps[:2], (1.5, 0.25, 1.0), False)
    i, f, p, n = seen[0]
    assert i == [8, 48, 4, L.F16, L.F32, 3, 4, 0, 0, 0] and f == [1.5, 0.25, 9.0] and n == 1
    assert p == [x.data_ptr(), eps.data_ptr(), 0, out.data_ptr(), keep.data_ptr()]
    i, f, p, n = seen[1]
    assert i[2] == 0 and p[4] == 0 and p[2] == 0
    with pytest.raises(L.T2VError, match="fp32"):
        samplers._ddim_invert(out, x.half(), eps, (1.5, 0.25, 9.0), True)
    with pytest.raises(L.T2VError, match="eps pair"):
        samplers._ddim_invert(out, x, eps[:2], (1.5, 0.25, 9.0), True)
    assert len(seen) == 2
