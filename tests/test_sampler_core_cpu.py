"""CPU: the three parts every sampling loop is built from (samplers.py): the T2V_OP_DDIM_STEP record builder with its launch tail,
the run guard, and the shared eps-pair evaluation as the DDIM_Gaussian loop uses it.

Records: every wrapper is called on CPU tensors with a capturing stand-in for the library, and EVERY element of i / f / p of every
record is compared with a table written out here from the field list of include/t2v_hip.h (fields not named are zero)."""
import types

import numpy as np
import pytest
import torch

from oracle import configs, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers, videocrafter as VC

SHAPE = (2, 4, 1, 1, 3)                 # B = 2 videos, C = 4 channels, inner = 3
COEF = [1.75, 1.5, 0.875, 0.25, 0.0, 9.0]
COEF_ETA = [1.75, 1.5, 0.875, 0.25, 0.125, 9.0]


# ---- 1. records ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def launches(monkeypatch):
    """-> the list of launches, each the list of its records as (kind, i[32], f[8], p[12])."""
    seen = []

    class _Lib:
        def t2v_run_ops(self, ops, n, ext, n_ext, stream):
            recs = [ops._obj] if hasattr(ops, "_obj") else [ops[k] for k in range(n)]
            assert ext is None and n_ext == 0 and stream.value in (0, None)
            seen.append([(o.kind, list(o.i), list(o.f), list(o.p)) for o in recs])
            return 0
    monkeypatch.setattr(L, "load", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    return seen


def _want(i, f, p, kind=L.OP_DDIM_STEP):
    """The whole record from the fields that are named: {index: value}, everything else zero."""
    full_i, full_f, full_p = [0] * L.OP_NI, [0.0] * L.OP_NF, [0] * L.OP_NP
    for k, v in i.items():
        full_i[k] = v
    for k, v in f.items():
        full_f[k] = float(np.float32(v))
    for k, v in p.items():
        full_p[k] = v
    return (kind, full_i, full_f, full_p)


def _operands(eps_dtype=torch.float32):
    x = torch.zeros(SHAPE)
    return x, torch.zeros((4,) + SHAPE[1:], dtype=eps_dtype), torch.zeros_like(x), torch.zeros_like(x)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("guided", [0, 2, 4])
@pytest.mark.parametrize("eps_dtype", [torch.float16, torch.float32])
def test_update_record(launches, eps_dtype, guided, mode):
    x, eps, out, noise = _operands(eps_dtype)
    tag = L.F16 if eps_dtype == torch.float16 else L.F32
    i = {0: 8, 1: 3, 2: guided, 3: tag, 4: L.F32, 5: mode, 6: 4}
    f = {0: 1.75, 1: 1.5, 2: 0.875, 3: 0.25, 4: 0.0, 5: 9.0}
    p = {0: x.data_ptr(), 1: eps.data_ptr(), 3: out.data_ptr()}
    assert samplers._ddim_update(out, x, eps, None, COEF, guided, mode=mode) is out          # no noise
    assert samplers._ddim_update(out, x, eps, noise, COEF, guided, mode=mode) is out         # noise given, sigma 0: p[2] stays 0
    assert samplers._ddim_update(out, x, eps, noise, COEF_ETA, guided, mode=mode) is out     # noise given, sigma != 0
    assert launches == [[_want(i, f, p)], [_want(i, f, p)], [_want(i, {**f, 4: 0.125}, {**p, 2: noise.data_ptr()})]]


def test_update_record_fp16_latent(launches):
    x, eps = torch.zeros(SHAPE, dtype=torch.float16), torch.zeros((4,) + SHAPE[1:], dtype=torch.float16)
    out = torch.zeros_like(x)
    samplers._ddim_update(out, x, eps, None, COEF, 2, mode=0)
    assert launches == [[_want({0: 8, 1: 3, 2: 2, 3: L.F16, 4: L.F16, 5: 0, 6: 4}, {0: 1.75, 1: 1.5, 2: 0.875, 3: 0.25, 5: 9.0},
                               {0: x.data_ptr(), 1: eps.data_ptr(), 3: out.data_ptr()})]]


def test_lincomb_record(launches):
    x, eps, out, _ = _operands(torch.float16)
    assert samplers._lincomb(out, [(0.5, x), (-2.0, eps[:2])]) is out
    assert launches == [[_want({0: 24, 1: 2, 2: L.F32, 3: L.F32, 4: L.F16}, {0: 0.5, 1: -2.0},
                               {0: x.data_ptr(), 1: eps.data_ptr(), 6: out.data_ptr()}, kind=L.OP_LINCOMB)]]


@pytest.mark.parametrize("with_qnoise", [False, True])
def test_blend_record(launches, with_qnoise):
    x, eps, out, noise = _operands(torch.float16)
    known, mask, qnoise = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    qcoef = (0.75, 0.5) if with_qnoise else (1.0, 0.0)
    assert samplers._ddim_update_blend(out, x, eps, noise, COEF_ETA, 4, known, mask, qnoise if with_qnoise else None, qcoef) is out
    want = _want({0: 8, 1: 3, 2: 4, 3: L.F16, 4: L.F32, 5: 1, 6: 4, 7: 1},
                 {0: 1.75, 1: 1.5, 2: 0.875, 3: 0.25, 4: 0.125, 5: 9.0, 6: qcoef[0], 7: qcoef[1]},
                 {0: x.data_ptr(), 1: eps.data_ptr(), 2: noise.data_ptr(), 3: out.data_ptr(), 4: known.data_ptr(), 5: mask.data_ptr(),
                  6: qnoise.data_ptr() if with_qnoise else 0})
    assert launches == [[want]]


def test_restricted_records(launches):
    x, eps, out, noise = _operands()
    grad, table = torch.zeros_like(x), torch.zeros(2, 4)
    i = {0: 8, 1: 3, 2: 2, 3: L.F32, 4: L.F32, 5: 0, 6: 4}
    f = {0: 1.75, 1: 1.5, 2: 0.875, 3: 0.25, 4: 0.125, 5: 9.0}
    p = {0: x.data_ptr(), 1: eps.data_ptr(), 2: noise.data_ptr(), 3: out.data_ptr()}
    # no restriction, the classifier-guidance term alone: one record
    samplers._ddim_restricted_step(out, x, eps, noise, COEF_ETA, 2, grad=grad, sqrt_1mat=0.625)
    assert launches.pop() == [_want({**i, 8: 0, 9: 1}, {**f, 7: 0.625}, {**p, 8: grad.data_ptr()})]
    # clamp: one record, with and without the term
    samplers._ddim_restricted_step(out, x, eps, noise, COEF_ETA, 2, bound=1.0)
    assert launches.pop() == [_want({**i, 8: 1}, {**f, 6: 1.0}, p)]
    samplers._ddim_restricted_step(out, x, eps, noise, COEF_ETA, 2, bound=1.0, grad=grad, sqrt_1mat=0.625)
    assert launches.pop() == [_want({**i, 8: 1, 9: 1}, {**f, 6: 1.0, 7: 0.625}, {**p, 8: grad.data_ptr()})]
    # percentile: the measure record (the percentile, no gradient fields), then the apply record (the gradient fields, no percentile)
    samplers._ddim_restricted_step(out, x, eps, noise, COEF_ETA, 2, percentile=0.995, table=table, grad=grad, sqrt_1mat=0.625)
    assert launches.pop() == [_want({**i, 8: 3}, {**f, 6: 0.995}, {**p, 7: table.data_ptr()}),
                              _want({**i, 8: 2, 9: 1}, {**f, 7: 0.625}, {**p, 7: table.data_ptr(), 8: grad.data_ptr()})]
    # ... and without noise and gradient; percentile wins over a bound given with it
    samplers._ddim_restricted_step(out, x, eps, None, COEF, 2, percentile=0.5, table=table, bound=1.0)
    p0 = {k: v for k, v in p.items() if k != 2}
    assert launches.pop() == [_want({**i, 8: 3}, {**f, 4: 0.0, 6: 0.5}, {**p0, 7: table.data_ptr()}),
                              _want({**i, 8: 2}, {**f, 4: 0.0}, {**p0, 7: table.data_ptr()})]
    assert launches == []
    ops = samplers._ddim_restricted_records(out, x, eps, None, COEF, 2, bound=1.0)
    assert len(ops) == 1 and launches == []          # the records alone launch nothing


@pytest.mark.parametrize("guided", [False, True])
def test_unipc_threshold_records(launches, guided):
    x, eps, out, _ = _operands(torch.float16)
    table = torch.zeros(2, 4)
    assert samplers._x0_threshold(out, x, eps, 0.625, 0.75, 7.5 if guided else 1.0, guided, table) is out
    i = {0: 8, 1: 3, 2: 4 if guided else 0, 3: L.F16, 4: L.F32, 5: 2, 6: 4}
    f = {0: 0.625, 1: 0.75, 5: 7.5 if guided else 1.0}
    p = {0: x.data_ptr(), 1: eps.data_ptr(), 3: out.data_ptr(), 7: table.data_ptr()}
    assert launches == [[_want({**i, 8: 3}, {**f, 6: samplers.UNIPC_QUANTILE}, p), _want({**i, 8: 2}, f, p)]]
    assert samplers.UNIPC_QUANTILE == 0.995


@pytest.mark.parametrize("with_keep", [False, True])
@pytest.mark.parametrize("guided", [False, True])
def test_inversion_record(launches, guided, with_keep):
    x, eps, out, keep = _operands(torch.float16)
    assert samplers._ddim_invert(out, x, eps if guided else eps[:2], (1.5, 0.25, 9.0), guided, keep=keep if with_keep else None) is out
    assert launches == [[_want({0: 8, 1: 3, 2: 4 if guided else 0, 3: L.F16, 4: L.F32, 5: 3, 6: 4}, {0: 1.5, 1: 0.25, 5: 9.0},
                               {0: x.data_ptr(), 1: eps.data_ptr(), 3: out.data_ptr(), 4: keep.data_ptr() if with_keep else 0})]]


def test_refused_operands_launch_nothing(launches):
    x, eps, out, noise = _operands()
    good = torch.zeros_like(x)
    bad = {"dtype": good.half(), "strides": torch.zeros(SHAPE[:-1] + (6,))[..., ::2], "shape": torch.zeros(SHAPE[:-1] + (2,))}
    assert not bad["strides"].is_contiguous() and bad["strides"].shape == x.shape
    for why, t in bad.items():
        with pytest.raises(L.T2VError, match="the gradient of a classifier-guided DDIM step must be fp32, contiguous"):
            samplers._ddim_restricted_step(out, x, eps, noise, COEF, 2, grad=t, sqrt_1mat=0.5)
        for blend in ((t, good, good), (good, t, good), (good, good, t)):
            with pytest.raises(L.T2VError, match="the blend operands of a masked DDIM step must be fp32, contiguous"):
                samplers._ddim_update_blend(out, x, eps, noise, COEF, 4, *blend, (0.75, 0.5))
        with pytest.raises(L.T2VError, match="a DDIM inversion step needs fp32, contiguous x / out / keep"):
            samplers._ddim_invert(out, x, eps, (1.5, 0.25, 9.0), True, keep=t)
        with pytest.raises(L.T2VError, match="a DDIM inversion step needs fp32, contiguous x / out / keep"):
            samplers._ddim_invert(t, x, eps, (1.5, 0.25, 9.0), True)
    tables = {"dtype": torch.zeros(2, 4, dtype=torch.float16), "strides": torch.zeros(2, 8)[:, ::2], "shape": torch.zeros(1, 4), "none": None}
    for why, t in tables.items():
        with pytest.raises(L.T2VError, match=r"the threshold table of a percentile DDIM step must be fp32 \[videos, 4\]"):
            samplers._ddim_restricted_step(out, x, eps, noise, COEF, 2, percentile=0.9, table=t)
        with pytest.raises(L.T2VError, match=r"the threshold table of a thresholded data prediction must be fp32 \[videos, 4\]"):
            samplers._x0_threshold(out, x, eps, 0.5, 0.75, 9.0, True, t)
    with pytest.raises(L.T2VError, match="needs an fp32 latent x"):
        samplers._x0_threshold(out, x.half(), eps, 0.5, 0.75, 9.0, True, torch.zeros(2, 4))
    with pytest.raises(L.T2VError, match="contiguous eps pair"):
        samplers._ddim_invert(out, x, eps[:2], (1.5, 0.25, 9.0), True)
    assert launches == []


# ---- 2. the run guard ------------------------------------------------------------------------------------------------------------------
class _Boom(RuntimeError):
    pass


class _BareModel:
    """A model without the optional attributes; records what it sees at every forward."""
    device = "cpu"
    num_timesteps = 1000

    def __init__(self, fail_at=None):
        self.events, self.fail_at, self.forwards = [], fail_at, 0
        self.alphas_cumprod = torch.cumprod(1 - tp.beta_schedule_linear_sd().double(), dim=0)

    def __call__(self, x, t, c):
        self.forwards += 1
        self.events.append(("forward", getattr(self, "auto_refresh", "absent"), getattr(self, "eps_out_dtype", "absent")))
        if self.forwards == self.fail_at:
            raise _Boom()
        return torch.zeros_like(x)


class _GuardedModel(_BareModel):
    def __init__(self, fail_at=None):
        super().__init__(fail_at)
        self.auto_refresh, self.eps_out_dtype = True, None

    def verify_weights(self, device):
        self.events.append(("verify", self.auto_refresh, self.eps_out_dtype))

    def refresh_weights(self, device):
        self.events.append(("refresh", self.auto_refresh, self.eps_out_dtype))


def _copy(out, x, *a, keep=None, **k):
    out.copy_(x)
    if keep is not None:
        keep.copy_(x)
    return out


def _loop_inputs():
    g = torch.Generator().manual_seed(3)
    return torch.randn(1, 4, 2, 4, 4, generator=g), torch.randn(1, 5, 8, generator=g), torch.randn(1, 5, 8, generator=g)


def _gaussian(model):
    x, c, uc = _loop_inputs()
    smp = samplers.GaussianDiffusion(model, tp.beta_schedule_linear_sd())
    return smp.sample(x_T=x, S=3, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=9.0, clamp=1.0)


def _ddim(model):
    x, c, uc = _loop_inputs()
    smp = samplers.DDIMSampler(model, device="cpu")
    return smp.sample(4, 1, tuple(x.shape), conditioning=c, x_T=x, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)


def _encode(model):
    x, c, uc = _loop_inputs()
    smp = samplers.DDIMSampler(model, device="cpu")
    smp.make_schedule(4)
    return smp.encode(x, c, 4, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)


def _unipc(model):
    x, c, uc = _loop_inputs()
    smp = samplers.UniPCSampler(model, device="cpu")
    return smp.sample(4, 1, tuple(x.shape), conditioning=c, x_T=x, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)


def _videocrafter(model):
    x, c, uc = _loop_inputs()
    m = VC.LatentDiffusion.__new__(VC.LatentDiffusion)
    torch.nn.Module.__init__(m)
    VC.LatentDiffusion.register_schedule(m, **configs.LVDM_SCHEDULE)
    m.apply_model = lambda xx, t, cc, **kw: model(xx, t, cc)
    m.model = types.SimpleNamespace(diffusion_model=model)
    return VC.DDIMSampler(m).sample(4, 1, tuple(x.shape[1:]), conditioning=c, x_T=x, unconditional_guidance_scale=9.0,
                                    unconditional_conditioning=uc, verbose=False)


LOOPS = {"DDIM_Gaussian": _gaussian, "DDIM": _ddim, "encode": _encode, "UniPC": _unipc, "VideoCrafter": _videocrafter}


@pytest.fixture()
def cpu_loops(monkeypatch):
    for name in ("_lincomb", "_ddim_update", "_ddim_restricted_step", "_ddim_invert"):
        monkeypatch.setattr(samplers, name, _copy)
    monkeypatch.setattr(samplers, "_lincomb", lambda out, terms: _copy(out, terms[0][1]))
    monkeypatch.setattr(samplers, "state", types.SimpleNamespace(interrupted=False, skipped=False, sampling_step=0, sampling_steps=0))


@pytest.mark.parametrize("loop", list(LOOPS))
def test_guard_around_every_loop(cpu_loops, loop):
    model = _GuardedModel()
    LOOPS[loop](model)
    kinds = [e[0] for e in model.events]
    assert kinds[:3] == ["verify", "refresh", "forward"] and kinds.count("verify") == kinds.count("refresh") == 1
    assert model.events[0][1:] == model.events[1][1:] == (True, None)            # both before the settings change
    forwards = [e for e in model.events if e[0] == "forward"]
    assert len(forwards) >= 3 and all(e[1:] == (False, torch.float32) for e in forwards)
    assert model.auto_refresh is True and model.eps_out_dtype is None


@pytest.mark.parametrize("loop", list(LOOPS))
def test_guard_restores_when_the_model_raises(cpu_loops, loop):
    model = _GuardedModel(fail_at=2)
    model.auto_refresh, model.eps_out_dtype = "kept", torch.float16              # whatever the values were, they come back
    with pytest.raises(_Boom):
        LOOPS[loop](model)
    assert model.forwards == 2 and model.events[-1] == ("forward", False, torch.float32)
    assert model.auto_refresh == "kept" and model.eps_out_dtype == torch.float16


@pytest.mark.parametrize("loop", list(LOOPS))
def test_model_without_the_optional_attributes_runs(cpu_loops, loop):
    model = _BareModel()
    LOOPS[loop](model)
    assert model.forwards >= 3 and set(model.events) == {("forward", "absent", "absent")}
    assert not hasattr(model, "auto_refresh") and not hasattr(model, "eps_out_dtype")


# ---- 3. DDIM_Gaussian through the shared evaluation -----------------------------------------------------------------------------------
class _PairModel:
    device = "cpu"

    def __init__(self):
        self.calls = []

    def forward_cfg_pair(self, x, t, ctx, context_token=None, single_t=None):
        self.calls.append(("pair", t.clone(), ctx, context_token, single_t))
        return torch.zeros(2 * x.shape[0], *x.shape[1:])

    def __call__(self, x, t, c):
        self.calls.append(("forward", t.clone(), c))
        return torch.zeros_like(x)


def _gaussian_run(model, x, c, uc, guide=9.0):
    smp = samplers.GaussianDiffusion(model, tp.beta_schedule_linear_sd())
    smp.sample(x_T=x, S=3, conditioning=c, unconditional_conditioning=uc, unconditional_guidance_scale=guide, clamp=1.0)
    return smp


def test_gaussian_loop_uses_the_shared_evaluation(cpu_loops, monkeypatch):
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 4, 2, 4, 4, generator=g)                                  # Bx = 2
    c, uc, c2, uc2 = (torch.randn(1, 5, 8, generator=g) for _ in range(4))
    model = _PairModel()
    smp = _gaussian_run(model, x, c, uc)
    want_t = smp.get_time_steps(1000 // 3, 1)[:3].tolist()
    assert [k for k, *_ in model.calls] == ["pair"] * 3
    for (_, t, ctx, token, single_t), t_step in zip(model.calls, want_t):
        assert t.dtype == torch.float32 and t.tolist() == [float(t_step)] * 4    # the 2 * Bx row, uploaded once: no repeat in the model
        assert single_t is True and torch.equal(ctx, torch.cat([c.expand(2, 5, 8), uc.expand(2, 5, 8)]))
    tokens = [call[3] for call in model.calls]
    assert tokens[0] is not None and tokens[0] == tokens[1] == tokens[2]         # the objects stay: one token, one [cond | uncond] batch
    assert model.calls[1][2] is model.calls[0][2] and model.calls[2][2] is model.calls[0][2]
    # another run: another token
    _gaussian_run(model, x, c, uc)
    assert model.calls[3][3] == model.calls[5][3] and model.calls[3][3] != tokens[0]
    # prompt scheduling swaps the conditioning objects from the third step on: the token follows
    del model.calls[:]
    plain = samplers.reconstruct_conds
    monkeypatch.setattr(samplers, "reconstruct_conds", lambda cond, uncond, step: (cond, uncond) if step < 2 else (c2, uc2))
    _gaussian_run(model, x, c, uc)
    tokens = [call[3] for call in model.calls]
    assert tokens[0] == tokens[1] and tokens[2] != tokens[1]
    assert torch.equal(model.calls[2][2], torch.cat([c2.expand(2, 5, 8), uc2.expand(2, 5, 8)]))
    monkeypatch.setattr(samplers, "reconstruct_conds", plain)
    # unguided (scale 1, or no unconditional conditioning): one b = Bx forward on the first half of the row
    for guide, u in ((1.0, uc), (None, uc), (9.0, None)):
        del model.calls[:]
        _gaussian_run(model, x, c, u, guide=guide)
        assert [k for k, *_ in model.calls] == ["forward"] * 3 and all(call[1].tolist() == [float(t)] * 2
                                                                       for call, t in zip(model.calls, want_t))


def test_gaussian_loop_without_a_pair_forward_calls_cond_then_uncond(cpu_loops):
    x, c, uc = _loop_inputs()

    class _Two:
        device = "cpu"
        supports_cfg_batch = False

        def __init__(self):
            self.calls = []

        def __call__(self, xx, t, cond):
            self.calls.append((cond, xx.shape[0], t.tolist()))
            return torch.zeros_like(xx)
    model = _Two()
    smp = _gaussian_run(model, x, c, uc)
    want_t = smp.get_time_steps(1000 // 3, 1)[:3].tolist()
    assert len(model.calls) == 6
    for k, (cond, b, t) in enumerate(model.calls):
        assert cond is (c, uc)[k % 2] and b == 1 and t == [float(want_t[k // 2])]

    class _Batch(_Two):
        supports_cfg_batch = True
    model = _Batch()
    _gaussian_run(model, x, c, uc)
    assert [(b, t) for _, b, t in model.calls] == [(2, [float(t)] * 2) for t in want_t]
    assert all(torch.equal(cond, torch.cat([c, uc])) for cond, _, _ in model.calls)
