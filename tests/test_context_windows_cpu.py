"""CPU: context windows (`context_windows=`, samplers.ContextWindows) — the schedule, what the designed operands of
tests/context_window_inputs.py expose, the host logic of the three samplers against the REAL reference run through windows
(tests/golden/make_golden_context_windows.py), the inert case and the keyword plumbing, and the validation of the two record forms.

As in tests/test_keyframe_cpu.py the kernels' bindings (`_window_gather`, `_window_blend`, the step bindings) are replaced by their
restatements and the UNet by the oracle port, so the product's own host logic is what runs; the kernels are checked on the GPU
(tests/test_gpu_context_windows.py).

One case of the issue's list cannot expose one mutation, by arithmetic: with F = 11, length 4 and overlap 3 the stride is 1, so the
flush-right last window (start 7) IS the next stride position and "stride position instead of flush right" changes nothing there.  The
test asserts that the two tables coincide for that shape and that the mutation is exposed for overlap 1 and 2.  Likewise the pyramid and
flat weights read the same from both ends, so "weights reversed" is checked on the designed table (DESIGNED_WEIGHTS), which is what the
GPU test hands the kernel."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import context_window_inputs as CW
from oracle import configs, torch_port as tp
from sd_webui_text2video_amd import _lib as L, samplers
from test_keyframe_cpu import _PlainStepLib
from test_samplers_cpu import _ddim_update_cpu, _inputs, _lincomb_cpu, _PortModel, _rel

GOLD = os.path.join(os.path.dirname(__file__), "golden", "context_windows.npz")
FRAMES, WINDOWS, STEPS, SCALE = 6, dict(length=4, overlap=2), 4, 9.0


# ---- 1. the schedule ---------------------------------------------------------------------------------------------------------------------
GRID = [(length, overlap) for length in (2, 3, 4, 5, 8, 16) for overlap in range(1, length)]


@pytest.mark.parametrize("length,overlap", GRID)
def test_schedule_properties(length, overlap):
    for kind in ("pyramid", "flat"):
        w = samplers.ContextWindows(length, overlap, kind)
        assert [w.weight(j) for j in range(length)] == CW.weights_ref(length, kind)
    w = samplers.ContextWindows(length, overlap)
    for frames in range(2, 41):
        starts = w.starts(frames)
        assert starts == CW.starts_ref(frames, length, overlap), (frames, starts)
        if frames <= length:
            assert not w.active(frames) and starts == [0]
            continue
        assert w.active(frames)
        assert all(0 <= s and s + length <= frames for s in starts)                       # full-length windows inside the clip
        assert all(b > a for a, b in zip(starts, starts[1:]))                             # strictly ascending: no duplicate
        assert starts[0] == 0 and starts[-1] == frames - length                           # the last one flush right
        assert all(s == k * (length - overlap) for k, s in enumerate(starts[:-1]))        # the others on the stride grid
        covered = {f for s in starts for f in range(s, s + length)}
        assert covered == set(range(frames))
        samplers._check_window_table(starts, frames, length)
    rows = 2 * len(w.starts(40))
    assert w.chunks(rows) == [(0, rows)]
    for batch in (1, 3, rows, rows + 5):
        ch = samplers.ContextWindows(length, overlap, batch=batch).chunks(rows)
        assert ch == CW.chunks_ref(rows, min(batch, rows)) and len({n for _, n in ch}) <= 2 and sum(n for _, n in ch) == rows


def test_schedule_refusals():
    for bad in (dict(length=1, overlap=1), dict(length=4, overlap=0), dict(length=4, overlap=4), dict(length=4, overlap=5),
                dict(length=4, overlap=1, weights="cosine"), dict(length=4, overlap=1, batch=0), dict(length=4.0, overlap=1),
                dict(length=4, overlap=True)):
        with pytest.raises(ValueError, match="context_windows"):
            samplers.ContextWindows(**bad)
    C = samplers.ContextWindows.coerce
    assert C(None) is None and C(C((4, 1))) is not None
    for form in (dict(length=4, overlap=1, weights="flat", batch=2), (4, 1, "flat", 2), [4, 1, "flat", 2]):
        w = C(form)
        assert (w.length, w.overlap, w.weights, w.batch) == (4, 1, "flat", 2)
    for bad in (dict(length=4), dict(length=4, overlap=1, shift=1), (4,), "16/4", 16):
        with pytest.raises(ValueError, match="context_windows"):
            C(bad)
    for starts in ([0, 5], [0, 3, 3, 7], [1, 4, 7], [0, 3, 6], [0, 3, 6, 8]):
        with pytest.raises(L.T2VError, match="context windows"):
            samplers._check_window_table(starts, 11, 4)


# ---- 2. what the designed operands expose ------------------------------------------------------------------------------------------------
def _differs(got, ref, bound):
    """-> (share of elements the mutation leaves unchanged, does any element differ beyond the GPU tolerance)."""
    same = (got - ref).abs() <= bound                  # (a NaN compares false: it differs)
    return float(same.double().mean()), bool((~same).any())


@pytest.mark.parametrize("shape", CW.BLEND_SHAPES, ids=CW.shape_id)
def test_designed_operands_expose_every_mutation(shape):
    starts = CW.starts_ref(CW.F, CW.LENGTH, shape["overlap"])
    nW, roles = len(starts), 2 if shape["guided"] else 1
    e = CW.eps_operand(roles, nW, shape["hw"], shape["dtype"])
    assert e.unique().numel() == e.numel()                                               # every coordinate has its own value
    ref, bound = CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F)
    assert bool(torch.isfinite(ref).all())
    # the forwards put together again give the same tensor, whatever the chunking
    for batch in CW.BATCHES:
        assert torch.equal(CW.assemble_ref(CW.split_chunks(e, batch), roles, CW.V * nW), e)
    stride_last = starts[:-1] + [(nW - 1) * (CW.LENGTH - shape["overlap"])]
    mutations = {
        "window start off by one": lambda: CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F, shift=1)[0],
        "weights reversed": lambda: CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F, reverse=True)[0],
        "normalised by the window count": lambda: CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F, normalise="count")[0],
        "w * V + v batch order": lambda: CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F, order="wv")[0],
    }
    if shape["overlap"] == 3:
        assert stride_last == starts          # stride 1: the flush-right window is the next stride position (module docstring)
    else:
        assert stride_last != starts
        mutations["last window at the stride position"] = lambda: CW.blend_ref(e, stride_last, CW.DESIGNED_WEIGHTS, CW.V, CW.F)[0]
    if shape["guided"]:
        mutations["cond / uncond halves swapped"] = lambda: CW.blend_ref(e, starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F, swap_roles=True)[0]
        for batch in (1, 3):
            mutations[f"uncond half at the full batch's offset (forwards of {batch})"] = lambda b=batch: CW.blend_ref(
                CW.assemble_ref(CW.split_chunks(e, b), roles, CW.V * nW, uncond_at="batch"), starts, CW.DESIGNED_WEIGHTS, CW.V, CW.F)[0]
    for name, run in mutations.items():
        same, exposed = _differs(run(), ref, bound)
        print(f"{CW.shape_id(shape)}: {name}: {100 * same:.1f} % of the elements unchanged")
        assert exposed, name
    # the gather: a wrong start, the other batch order and a wrong first row all land on other values
    x = CW.latent_operand(shape["hw"], shape["dtype"])
    assert x.unique().numel() == x.numel()
    good = CW.gather_ref(x, starts, CW.LENGTH, 0, CW.V * nW)
    assert not torch.equal(CW.gather_ref(x, [min(s + 1, CW.F - CW.LENGTH) for s in starts], CW.LENGTH, 0, CW.V * nW), good)
    assert not torch.equal(good.view(CW.V, nW, *good.shape[1:]).transpose(0, 1).reshape(good.shape), good)
    assert not torch.equal(CW.gather_ref(x, starts, CW.LENGTH, 1, CW.V * nW - 1), good[:-1])


# ---- 3. the samplers' host logic against the reference run through windows ----------------------------------------------------------------
@pytest.fixture()
def cpu_kernels(monkeypatch):
    """-> the calls of the two window bindings; every binding the samplers launch is its restatement."""
    calls, lib = types.SimpleNamespace(gather=[], blend=[]), _PlainStepLib()
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update", _ddim_update_cpu)
    monkeypatch.setattr(samplers, "_window_gather", lambda xw, x, s, row0: (calls.gather.append((tuple(xw.shape), row0)), CW.window_gather_cpu(xw, x, s, row0))[1])
    monkeypatch.setattr(samplers, "_window_blend",
                        lambda out, ch, s, w, roles: (calls.blend.append(([tuple(e.shape) for e in ch], roles)), CW.window_blend_cpu(out, ch, s, w, roles))[1])
    monkeypatch.setattr(samplers.L, "load", lambda: lib)
    monkeypatch.setattr(samplers.GaussianDiffusion, "_step_plan",
                        lambda self, C, inner, guided, eps_dtype, x_dtype, samples=1: types.SimpleNamespace(handle=(C, inner, guided, eps_dtype, x_dtype, samples)))
    samplers.state.sampling_step = 0
    calls.lib = lib
    return calls


@pytest.fixture(scope="module")
def port_model():
    return _PortModel()


def _noise(seed=1234, frames=FRAMES):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randn((1, 4, frames, 16, 16), generator=g)


def _sample(model, name, noise, **kw):
    _, c, uc = _inputs()
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
    smp.progress = False
    samplers.state.sampling_step = 0
    return smp.sample_loop(steps=STEPS, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=noise.shape[0], latents=None,
                           shape=tuple(noise.shape), noise=noise, guidance_scale=SCALE, eta=0.0, sampler_name=name, **kw)


@pytest.mark.parametrize("batch", [None, 1])
@pytest.mark.parametrize("name", ["DDIM_Gaussian", "DDIM", "UniPC"])
def test_windowed_samplers_match_the_reference_through_windows(cpu_kernels, port_model, name, batch):
    gold = np.load(GOLD)
    assert gold["starts"].tolist() == samplers.ContextWindows(**WINDOWS).starts(FRAMES) == [0, 2]
    port_model.calls.clear()
    x0 = _sample(port_model, name, _noise(), context_windows=dict(WINDOWS, batch=batch))
    e = _rel(x0, gold[f"{name}_x0_1234"])
    print(f"{name}, forwards of {batch or 'all'} windows: {e:.3e} against the reference through windows (gate 2e-5)")
    assert e < 2e-5                                            # the gate of tests/test_samplers_cpu.py for the same samplers
    # per evaluation: one gather and one forward per chunk, one blend; the forwards hold the windows as their batch ([cond | uncond])
    forwards = 1 if batch is None else 2
    assert len(cpu_kernels.blend) == STEPS and len(cpu_kernels.gather) == STEPS * forwards == len(port_model.calls)
    assert all(cl[0] == 2 * (2 // forwards) for cl in port_model.calls)
    assert all(roles == 2 and len(ch) == forwards for ch, roles in cpu_kernels.blend)
    assert not np.array_equal(x0.numpy(), gold[f"{name}_x0_1235"])


def test_windows_change_the_result(cpu_kernels, port_model):
    """The golden is not the full-clip run: windows of 4 out of 6 frames see other temporal context."""
    full = _sample(port_model, "DDIM", _noise())
    assert _rel(full, np.load(GOLD)["DDIM_x0_1234"]) > 1e-2


# ---- 4. inert, plumbing, refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["DDIM_Gaussian", "DDIM", "UniPC"])
def test_a_clip_no_longer_than_a_window_is_the_call_without_the_keyword(cpu_kernels, port_model, name):
    runs = []
    for kw in ({}, dict(context_windows=dict(length=4, overlap=2)), dict(context_windows=samplers.ContextWindows(3, 1, "flat", 1))):
        port_model.calls.clear()
        torch.manual_seed(7)
        x0 = _sample(port_model, name, _noise(frames=3), **kw)
        runs.append((x0, list(port_model.calls), torch.get_rng_state()))
    for x0, calls, rng in runs[1:]:
        assert torch.equal(x0, runs[0][0]) and calls == runs[0][1] and torch.equal(rng, runs[0][2])
    assert not cpu_kernels.gather and not cpu_kernels.blend


class _Stop(Exception):
    pass


def test_keyword_plumbing(monkeypatch, cpu_kernels, port_model):
    from sd_webui_text2video_amd import pipeline, unet as U
    seen = []

    def sample_loop(self, *a, **kw):
        seen.append(kw)
        raise _Stop
    noise, c, uc = _inputs()
    # sample_loop -> sampler.sample: forwarded (coerced) when set, absent otherwise
    for name in ("DDIM_Gaussian", "DDIM", "UniPC"):
        smp = samplers.Txt2VideoSampler(port_model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
        got = []
        smp.sampler.sample = lambda **kw: (got.append(kw), noise)[1]
        kw = dict(steps=2, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape), noise=noise,
                  guidance_scale=9.0, sampler_name=name)
        smp.sample_loop(**kw)
        smp.sample_loop(**kw, context_windows=(4, 2))
        assert "context_windows" not in got[0]
        w = got[1]["context_windows"]
        assert isinstance(w, samplers.ContextWindows) and (w.length, w.overlap, w.weights, w.batch) == (4, 2, "pyramid", None)
        with pytest.raises(ValueError, match="context_windows"):
            smp.sample_loop(**kw, context_windows=dict(length=4, overlap=4))
    # infer / infer_conditioned / process_modelscope -> sample_loop
    monkeypatch.setattr(samplers.Txt2VideoSampler, "sample_loop", sample_loop)
    net = U.UNetSD(**configs.TINY_UNET, init_weights=False)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, device="cpu")
    pipe.preprocess = lambda *a, **k: (c, uc)
    win = {"length": 16, "overlap": 4}
    with pytest.raises(_Stop):
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, device="cpu", context_windows=win)
    with pytest.raises(_Stop):
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, device="cpu")
    with pytest.raises(_Stop):
        pipe.infer("a", "b", 2, 3, 1, 9.0, 128, 128, cpu_vae="CPU (full precision)", device="cpu", context_windows=win)
    with pytest.raises(_Stop):
        pipeline.process_modelscope(dict(pipe=pipe, cond=c, uncond=uc, steps=2, frames=3, seed=1, cfg_scale=9.0, width=128, height=128,
                                         context_windows=win))
    assert [kw.get("context_windows") for kw in seen] == [win, None, win, win] and "context_windows" not in seen[1]


def test_refusals(cpu_kernels, port_model):
    from sd_webui_text2video_amd import videocrafter
    noise, win = _noise(), dict(length=4, overlap=2)
    split = types.SimpleNamespace(size=2, role=0)
    for name in ("DDIM_Gaussian", "DDIM", "UniPC"):
        _, c, uc = _inputs()
        smp = samplers.Txt2VideoSampler(port_model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
        kw = dict(S=2, batch_size=1, shape=tuple(noise.shape), conditioning=c, unconditional_conditioning=uc, x_T=noise,
                  unconditional_guidance_scale=9.0, context_windows=win)
        smp.sampler.cfg_parallel = split
        with pytest.raises(L.T2VError, match="CFG-pair"):
            smp.sampler.sample(**kw)
        smp.sampler.cfg_parallel = None
        port_model.t_shard = object()
        try:
            with pytest.raises(L.T2VError, match="split over ranks"):
                smp.sampler.sample(**kw)
        finally:
            del port_model.t_shard
        with pytest.raises(ValueError, match="context_windows"):
            smp.sampler.sample(**dict(kw, context_windows=dict(length=4, overlap=1, weights="hann")))
    ddim = samplers.Txt2VideoSampler(port_model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name="DDIM").sampler
    ddim.make_schedule(4)
    port_model.t_shard = object()
    try:
        with pytest.raises(L.T2VError, match="split over ranks"):
            ddim.decode(noise, torch.zeros(1, 7, 1024), 2, context_windows=win)
    finally:
        del port_model.t_shard
    assert not port_model.calls or port_model.calls.clear() is None
    vc = object.__new__(videocrafter.DDIMSampler)
    with pytest.raises(L.T2VError, match="VideoCrafter"):
        vc.sample(S=2, batch_size=1, shape=(4, 6, 8, 8), context_windows=win)


class _PairModel:
    """A UNetSD stand-in with `forward_cfg_pair`: records (rows, the context token, the context's batch) of every forward."""
    num_timesteps, device = 1000, torch.device("cpu")

    def __init__(self):
        self.seen = []

    def forward_cfg_pair(self, x, t, ctx, context_token=None, single_t=None):
        self.seen.append((x.shape[0], context_token, ctx.shape[0] if torch.is_tensor(ctx) else None))
        return torch.zeros((2 * x.shape[0],) + tuple(x.shape[1:]))

    def __call__(self, x, t, c):
        raise AssertionError("a guided step is one forward_cfg_pair call")


@pytest.mark.parametrize("per_video", [False, True])
def test_context_token_is_stable_over_the_steps(cpu_kernels, per_video):
    """The expanded conditioning of every forward is built once per run: from the second step on a forward carries the token (and so
    the cached context K/V) it carried at the step before.  Window (v, w) gets the context of video v."""
    model = _PairModel()
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name="DDIM")
    g = torch.Generator().manual_seed(3)
    V = 2
    c, uc = torch.randn(V if per_video else 1, 7, 1024, generator=g), torch.randn(V if per_video else 1, 7, 1024, generator=g)
    noise = torch.cat([_noise(1234), _noise(1235)])
    got = {}
    real = samplers._eval_eps_pair

    def spy(model_, x, t, cc, uu, guide, cfg=None, cache=None):
        got.setdefault(x.shape[0], []).append((cc, uu))
        return real(model_, x, t, cc, uu, guide, cfg, cache=cache)
    samplers._eval_eps_pair, before = spy, samplers._eval_eps_pair
    try:
        smp.sampler.sample(S=STEPS, batch_size=V, shape=tuple(noise.shape), conditioning=c, unconditional_conditioning=uc, x_T=noise,
                           unconditional_guidance_scale=SCALE, context_windows=dict(WINDOWS, batch=3))
    finally:
        samplers._eval_eps_pair = before
    # 2 videos x 2 windows in forwards of 3 and 1 rows
    assert [s[0] for s in model.seen] == [3, 1] * STEPS and all(s[2] == 2 * s[0] for s in model.seen)
    for k in (0, 1):
        tokens = [s[1] for s in model.seen[k::2]]
        assert all(t == tokens[0] for t in tokens[1:]), tokens
    assert model.seen[0][1] != model.seen[1][1] or not per_video
    if per_video:        # rows 0..2 are (v0, w0), (v0, w1), (v1, w0); row 3 is (v1, w1)
        cc, uu = got[3][0]
        assert torch.equal(cc, c[[0, 0, 1]]) and torch.equal(uu, uc[[0, 0, 1]])
        cc, uu = got[1][0]
        assert torch.equal(cc, c[[1]]) and torch.equal(uu, uc[[1]])
        assert all(a is got[3][0][0] for a, _ in got[3]) and all(a is got[1][0][0] for a, _ in got[1])      # the same objects at every step
    else:
        assert all(a is c and b is uc for calls in got.values() for a, b in calls)


# ---- 5. the records ----------------------------------------------------------------------------------------------------------------------
def _record(form, **kw):
    """A valid record of a context-window form of T2V_OP_LINCOMB over made-up addresses, then the overrides (i0..i9, p0, p1, p2, p6)."""
    op = L.T2VOp()
    op.kind = L.OP_LINCOMB
    ptr = 1 << 40
    base = {0: 2, 1: 4, 2: L.F32, 3: 11, 4: 16, 5: 4, 6: 4, 7: 2 if form == 1 else 3, 8: 0 if form == 1 else 5, 9: form}
    for k, v in base.items():
        op.i[k] = kw.get(f"i{k}", v)
    op.p[0], op.p[1], op.p[6] = kw.get("p0", ptr), kw.get("p1", ptr + (1 << 30)), kw.get("p6", ptr + (3 << 30))
    op.p[2] = kw.get("p2", ptr + (2 << 30) if form == 1 else 0)
    return op


def test_record_validation_without_gpu(built_lib):
    lib = built_lib

    def refused(op, needle):
        rc = lib.t2v_run_ops(ctypes.byref(op), 1, None, 0, None)
        return rc == -1 and needle in lib.t2v_last_error()

    def accepted(op):
        h = ctypes.c_void_p()
        rc = lib.t2v_plan_create(ctypes.byref(op), 1, ctypes.byref(h))
        if rc == 0:
            lib.t2v_plan_destroy(h)
        return rc == 0

    for form, name in ((1, b"window blend"), (2, b"window gather")):
        assert accepted(_record(form)) and accepted(_record(form, i2=L.F16))
        for field in ("i0", "i1", "i3", "i4", "i6"):
            assert refused(_record(form, **{field: 0}), name + b" (lincomb i[9] = " + str(form).encode()), field
        assert refused(_record(form, i5=1), b"window length") and refused(_record(form, i5=12), b"window length")
        assert accepted(_record(form, i5=11))
        assert refused(_record(form, i2=7), b"dtype")
        for slot in ("p0", "p1", "p6"):
            assert refused(_record(form, **{slot: 0}), b"null " + name + b" pointer"), slot
        assert refused(_record(form, i0=1 << 20, i3=1 << 10, i4=1 << 10), b"2^31 - 1 elements")
    assert refused(_record(1, i7=0), b"roles") and refused(_record(1, i7=3), b"roles") and accepted(_record(1, i7=1))
    assert refused(_record(1, i8=1), b"i[8] must be 0") and refused(_record(1, p2=0), b"null window blend pointer")
    assert refused(_record(2, i8=0), b"batch rows") and refused(_record(2, i7=-1), b"batch rows") and refused(_record(2, i7=4, i8=5), b"batch rows")
    assert accepted(_record(2, i7=0, i8=8)) and accepted(_record(2, i7=7, i8=1))
    assert refused(_record(3), b"form i[9]") and refused(_record(-1), b"form i[9]")
    # i[9] = 0: the linear combination validates exactly as before
    plain = L.T2VOp()
    plain.kind = L.OP_LINCOMB
    plain.i[0], plain.i[1], plain.i[2], plain.i[3], plain.i[4] = 16, 2, L.F32, L.F32, L.F16
    plain.p[0], plain.p[1], plain.p[6] = 1 << 40, 1 << 41, 1 << 42
    assert accepted(plain)
    plain.p[1] = 0
    assert refused(plain, b"null lincomb term")
    plain.p[1], plain.i[1] = 1 << 41, 7
    assert refused(plain, b"lincomb needs n > 0, 1..6 terms, an output")
    plain.i[1], plain.p[6] = 6, 0
    assert refused(plain, b"lincomb needs n > 0, 1..6 terms, an output")


def test_bindings_build_the_records(monkeypatch):
    seen = []

    class _Lib:
        def t2v_run_ops(self, ops, n, ext, n_ext, stream):
            arr = [ops._obj] if n == 1 and hasattr(ops, "_obj") else [ops[k] for k in range(n)]
            seen.append([(o.kind, [o.i[k] for k in range(10)], [o.p[k] for k in range(7)]) for o in arr])
            return 0
    monkeypatch.setattr(L, "load", lambda: _Lib())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 0})())
    x = torch.zeros(2, 4, 11, 2, 3, dtype=torch.float16)
    starts, wg = torch.tensor([0, 3, 6, 7], dtype=torch.int32), torch.tensor(CW.DESIGNED_WEIGHTS)
    xw = torch.zeros(3, 4, 4, 2, 3, dtype=torch.float16)
    samplers._window_gather(xw, x, starts, 5)
    assert seen[0] == [(L.OP_LINCOMB, [2, 4, L.F16, 11, 6, 4, 4, 5, 3, 2], [x.data_ptr(), starts.data_ptr(), 0, 0, 0, 0, xw.data_ptr()])]
    out = torch.zeros(4, 4, 11, 2, 3)
    e = torch.zeros(16, 4, 4, 2, 3)
    samplers._window_blend(out, [e], starts, wg, 2)
    assert seen[1] == [(L.OP_LINCOMB, [2, 4, L.F32, 11, 6, 4, 4, 2, 0, 1], [e.data_ptr(), starts.data_ptr(), wg.data_ptr(), 0, 0, 0, out.data_ptr()])]
    # several forwards: one COPY2D per forward into the common layout [roles, V * nW, ...], then the blend, in one call
    parts = [torch.zeros(6, 4, 4, 2, 3), torch.zeros(6, 4, 4, 2, 3), torch.zeros(4, 4, 4, 2, 3)]
    samplers._window_blend(out, parts, starts, wg, 2)
    per_row = 4 * 4 * 6
    kinds = [r[0] for r in seen[2]]
    assert kinds == [L.OP_COPY2D] * 3 + [L.OP_LINCOMB]
    stage = seen[2][3][2][0]
    for k, (rows, row0) in enumerate(((3, 0), (3, 3), (2, 6))):
        _, i, p = seen[2][k]
        assert i[:6] == [2, rows * per_row, rows * per_row, 8 * per_row, L.F32, L.F32]
        assert p[0] == parts[k].data_ptr() and p[1] == stage + row0 * per_row * 4
    assert seen[2][3][1] == seen[1][0][1] and stage not in [t.data_ptr() for t in parts]
    for bad in (lambda: samplers._window_gather(xw.float(), x, starts, 0), lambda: samplers._window_gather(xw, x, starts, 6),
                lambda: samplers._window_gather(xw, x, starts.long(), 0), lambda: samplers._window_blend(out, [e[:15]], starts, wg, 2),
                lambda: samplers._window_blend(out.half(), [e], starts, wg, 2), lambda: samplers._window_blend(out, [e], starts, wg[:3], 2)):
        with pytest.raises(L.T2VError, match="window"):
            bad()
    assert len(seen) == 3
