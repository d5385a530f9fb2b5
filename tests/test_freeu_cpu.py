"""CPU: FreeU in the ModelScope lowering and through the public interface.

Programs: with FreeU on, the TINY_UNET program has one T2V_OP_FREEU at exactly the decoder blocks whose stream has 4 dim (b1, s1) and
2 dim (b2, s2) channels, after every write into its concat buffer and before every read of it by the block — also with the shared
cond | uncond prefix; with FreeU off (never on, or on and off again) the program is byte for byte what it was.  The arena-hazard rules
of tests/plan_hazards.py hold on the FreeU programs (footprint: tests/freeu_footprint.py).  The interpreter's forward of these programs
equals the REAL reference with FreeU hooks (tests/golden/freeu_tiny.npz) at the tolerance tests/test_lowering_cpu.py gives the plain
tiny forward.  The keyword reaches the UNet from every entry point, is restored afterwards, and is refused where it is not built."""
import os
import types

import numpy as np
import pytest
import torch

import freeu_footprint as FF
import freeu_ref as FR
import plan_footprint as FP
import plan_hazards as H
from harness import program_digest, rel_l2
from interp_freeu import FreeuInterp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import pipeline, samplers, unet as U, videocrafter
from test_context_windows_cpu import _Stop, cpu_kernels  # noqa: F401  (the fixture)
from test_samplers_cpu import _inputs, _PortModel

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "freeu_tiny.npz"))
VALUES = dict(zip(("b1", "b2", "s1", "s2"), (float(v) for v in GOLD["freeu"])))
ON = dict(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
FORWARD_GATE = 4e-3            # tests/test_lowering_cpu.py::test_unet_program_matches_oracle_in_interpreter


@pytest.fixture(scope="module")
def net():
    m = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(m, seed=0)
    return m


def _lower(net, share, freeu=True, geom=(2, 3, 8, 8)):
    """-> (compiled program, allocation events) of the tiny forward, batched or with the shared cond | uncond prefix."""
    mp = pytest.MonkeyPatch()
    try:
        rec = H.Recorder().install(mp)
        net._share_now = bool(share)
        if freeu:
            net.enable_freeu(**ON)
        B, F, h, w = geom
        comp = net._compile(B, F, h, w, 7, "f32", "f32", "f32", x_batch=1 if share else 0)
        return comp, rec.events(comp.prog)
    finally:
        net.disable_freeu()
        net._share_now = False
        mp.undo()


# ---- programs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [False, True], ids=["batched", "shared-prefix"])
def test_the_op_sits_at_the_4dim_and_2dim_blocks_between_writers_and_readers(net, share):
    comp, events = _lower(net, share)
    ops, dim = comp.prog.ops, net.dim
    if share:
        assert any(".to_skip." in op.name for op in ops), "the shared prefix spreads input_blocks.0 into its skip window with copies"
    _, middle, outputs, _ = net._layout
    stream, want = middle[-1][2], {}
    for prefix, parts, _ in outputs:
        g = FR.stage_gains(stream, dim, VALUES)
        if g is not None:
            want[prefix + ".freeu"] = (stream, parts[0][1], g)
        stream = parts[0][2]
    found = {op.name: k for k, op in enumerate(ops) if op.kind == L.OP_FREEU}
    assert set(found) == set(want) and len(want) == 10
    assert sum(v[0] == 4 * dim for v in want.values()) == 7 and sum(v[0] == 2 * dim for v in want.values()) == 3
    fps = [FF.footprint(op) for op in ops]
    for name, k in found.items():
        op, (c_h, c_total, (b, s)) = ops[k], want[name]
        rows, ct, ld, ch, frames, h, w = op.i[0:7]
        assert (ct, ch, frames, rows) == (c_total, c_h, 2 * 3, 2 * 3 * h * w) and ld >= ct
        assert (op.f[0], op.f[1]) == (b, s) and op.p[0].space == "arena"
        off = op.p[0].off
        life = [a for a in events if a.off <= off < a.end and a.born <= k and (a.died is None or a.died > k)]
        assert len(life) == 1
        born, died = life[0].born, life[0].died if life[0].died is not None else len(ops)
        whole = FP.Rect.mat(off, rows, ct, ld, 4)
        halves = {"stream": FP.Rect.mat(off, rows, c_h, ld, 4), "skip": FP.Rect.mat(off + 4 * c_h, rows, ct - c_h, ld, 4)}
        block = name[:-len("freeu")]
        touching = lambda j, mode: [x for x in fps[j] if x.space == "arena" and (x.mode == mode) and FP.overlap(x.rects, [whole]) is not None]
        # before the op: every byte of both halves has been written; nobody of the block has run; what is read is the encoder's own chain
        written = FP.union([r for j in range(born, k) for x in touching(j, "w") for r in x.rects])
        for half, rect in halves.items():
            left = FP.subtract(rect.intervals(), written)
            assert len(left[0]) == 0, (name, half, "not written before the op")
        assert not any(ops[j].name.startswith(block) for j in range(0, k))
        for j in range(born, k):
            for x in touching(j, "r"):
                assert FP.overlap(x.rects, [halves["stream"]]) is None, (name, ops[j].name, "reads the stream half before the op")
        # after the op: nothing writes the buffer, and every reader is the block's own
        readers = [j for j in range(k + 1, died) if touching(j, "r")]
        assert readers and readers[0] == k + 1 and all(ops[j].name.startswith(block) for j in readers), (name, [ops[j].name for j in readers])
        assert not any(touching(j, "w") for j in range(k + 1, died)), name
    # the mutant "b and s of the two stages exchanged" would give other records
    assert all((ops[k].f[0], ops[k].f[1]) != FR.stage_gains(want[n][0], dim, VALUES, exchanged=True) for n, k in found.items())


@pytest.mark.parametrize("share", [False, True], ids=["batched", "shared-prefix"])
def test_without_the_keyword_the_program_is_what_it_was(net, share):
    net._share_now = bool(share)
    try:
        kw = dict(x_batch=1 if share else 0)
        before = program_digest(net._compile(2, 3, 8, 8, 7, "f32", "f32", "f32", **kw), net.state_dict())
        key_before = net._program_key(2, 3, 8, 8, 7, torch.float32, torch.float32, torch.float32)
        net.enable_freeu(**ON)
        assert net.freeu == VALUES
        on = net._compile(2, 3, 8, 8, 7, "f32", "f32", "f32", **kw)
        key_on = net._program_key(2, 3, 8, 8, 7, torch.float32, torch.float32, torch.float32)
        net.disable_freeu()
        assert net.freeu is None
        after = program_digest(net._compile(2, 3, 8, 8, 7, "f32", "f32", "f32", **kw), net.state_dict())
        key_after = net._program_key(2, 3, 8, 8, 7, torch.float32, torch.float32, torch.float32)
    finally:
        net.disable_freeu()
        net._share_now = False
    assert after == before and program_digest(on, net.state_dict()) != before
    assert key_on != key_before == key_after
    assert ("freeu", VALUES["b1"], VALUES["b2"], VALUES["s1"], VALUES["s2"]) in key_on
    # every op of the program with FreeU but the FreeU records is an op of the plain program, in order (pointers may move: other arena)
    plain = [(op.kind, op.name) for op in net._compile(2, 3, 8, 8, 7, "f32", "f32", "f32").prog.ops]
    net.enable_freeu(**ON)
    try:
        with_f = [(op.kind, op.name) for op in net._compile(2, 3, 8, 8, 7, "f32", "f32", "f32").prog.ops if op.kind != L.OP_FREEU]
    finally:
        net.disable_freeu()
    assert with_f == plain


@pytest.mark.parametrize("share", [False, True], ids=["batched", "shared-prefix"])
def test_arena_hazards_of_the_freeu_programs(net, share):
    comp, events = _lower(net, share)
    with FF.installed():
        rep = H.analyse(comp.prog, events)
        assert not rep.hazards, "\n".join(str(h) for h in rep.hazards[:8])
        assert rep.inplace[FF.INPLACE] == 2 * 10            # the scaled half and the skip of each of the ten records
    assert FF.INPLACE not in [name for name, _, _ in H.INPLACE_CLASSES] and H.footprint is FP.footprint
    # the rule bites: without the in-place class the same program is flagged at every FreeU record
    held = H.footprint
    H.footprint = FF.footprint
    try:
        rep = H.analyse(comp.prog, events)
    finally:
        H.footprint = held
    at = {h.op for h in rep.hazards if h.rule == "R3"}
    assert at == {k for k, op in enumerate(comp.prog.ops) if op.kind == L.OP_FREEU}


# ---- forward parity ------------------------------------------------------------------------------------------------------------------------
def _gold_inputs():
    cfg = configs.TINY_UNET
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 3, 16, 16, generator=g)
    y = torch.randn(2, 7, cfg["context_dim"], generator=g)
    g2 = torch.Generator().manual_seed(17)
    x_odd = torch.randn(1, 4, 2, 40, 72, generator=g2)
    c = torch.randn(1, 7, cfg["context_dim"], generator=g2)
    return x[:, :, :, :8, :8].contiguous(), y, torch.tensor([801.0, 401.0]), x_odd, c


@pytest.mark.parametrize("case", ["64", "odd", "64-shared"])
def test_interpreter_forward_matches_the_reference_with_hooks(net, case):
    x, y, t, x_odd, c = _gold_inputs()
    if case == "odd":
        comp, _ = _lower(net, False, geom=(1, 2, 40, 72))
        ext = {L.EXT_X: x_odd, L.EXT_T: torch.tensor([601.0]), L.EXT_CTX: c, L.EXT_OUT: torch.empty(1, 4, 2, 40, 72)}
        gold, plain = GOLD["eps_odd"], GOLD["plain_odd"]
    else:
        share = case.endswith("shared")
        comp, _ = _lower(net, share)
        xs, ts = (x[:1].contiguous(), t[:1].repeat(2)) if share else (x, t)
        ext = {L.EXT_X: xs, L.EXT_T: ts, L.EXT_CTX: y, L.EXT_OUT: torch.empty(2, 4, 3, 8, 8)}
        gold, plain = GOLD["eps_64"], GOLD["plain_64"]
    FreeuInterp(comp.prog, comp.packer.materialise(net.state_dict(), "cpu")).run(ext)
    out = ext[L.EXT_OUT]
    assert not torch.isnan(out).any()
    if case == "64-shared":
        # one x and one t for both samples: compared with the batched program on the same inputs (the golden has two x)
        comp2, _ = _lower(net, False)
        ext2 = {L.EXT_X: torch.cat([xs, xs]), L.EXT_T: ts, L.EXT_CTX: y, L.EXT_OUT: torch.empty(2, 4, 3, 8, 8)}
        FreeuInterp(comp2.prog, comp2.packer.materialise(net.state_dict(), "cpu")).run(ext2)
        assert rel_l2(out, ext2[L.EXT_OUT]) < FORWARD_GATE
        return
    assert rel_l2(out, torch.from_numpy(gold)) < FORWARD_GATE
    assert rel_l2(torch.from_numpy(gold), torch.from_numpy(plain)) >= 10 * FORWARD_GATE          # the golden's own condition


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------------
class _FreeuPortModel(_PortModel):
    """The oracle port with the FreeU switch of UNetSD: every forward notes the values in force."""

    def __init__(self):
        super().__init__()
        self._freeu, self.seen = None, []

    def enable_freeu(self, s1, s2, b1, b2):
        self._freeu = (b1, b2, s1, s2)

    def disable_freeu(self):
        self._freeu = None

    def __call__(self, x, t, c):
        self.seen.append(self._freeu)
        return super().__call__(x, t, c)


OTHER = {"b1": 1.1, "b2": 1.2, "s1": 0.6, "s2": 0.4}
AS_TUPLE = lambda v: (v["b1"], v["b2"], v["s1"], v["s2"])


@pytest.mark.parametrize("name", ["DDIM_Gaussian", "DDIM", "UniPC"])
def test_the_keyword_reaches_the_unet_and_is_restored(cpu_kernels, name):  # noqa: F811
    model = _FreeuPortModel()
    noise, c, uc = _inputs()
    smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
    smp.progress = False
    kw = dict(steps=4, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape), noise=noise,
              guidance_scale=9.0, eta=0.0, sampler_name=name)
    runs = []
    for freeu in (None, VALUES, OTHER, None):
        model.seen.clear()
        samplers.state.sampling_step = 0
        smp.sample_loop(**kw, **({"freeu": freeu} if freeu is not None else {}))
        runs.append(list(model.seen))
        assert model._freeu is None                                       # restored after the call
    assert runs[0] and set(runs[0]) == {None} == set(runs[3])
    assert set(runs[1]) == {AS_TUPLE(VALUES)} and set(runs[2]) == {AS_TUPLE(OTHER)} and len(runs[1]) == len(runs[0])
    # the sampler's own entry point, and a model that had FreeU on before the call keeps its values
    model.enable_freeu(s1=0.5, s2=0.5, b1=1.0, b2=1.0)
    model.seen.clear()
    smp.sampler.sample(S=4, batch_size=1, shape=tuple(noise.shape), conditioning=c, unconditional_conditioning=uc, x_T=noise,
                       unconditional_guidance_scale=9.0, freeu=VALUES)
    assert set(model.seen) == {AS_TUPLE(VALUES)} and model._freeu == (1.0, 1.0, 0.5, 0.5)
    # restored when the call raises
    model.disable_freeu()
    boom = lambda *a, **k: (_ for _ in ()).throw(_Stop())
    held, model.__class__.__call__ = model.__class__.__call__, boom
    try:
        with pytest.raises(_Stop):
            smp.sampler.sample(S=4, batch_size=1, shape=tuple(noise.shape), conditioning=c, unconditional_conditioning=uc, x_T=noise,
                               unconditional_guidance_scale=9.0, freeu=VALUES)
    finally:
        model.__class__.__call__ = held
    assert model._freeu is None


def test_the_keyword_is_forwarded_only_when_set(monkeypatch):
    seen = []

    def sample_loop(self, *a, **kw):
        seen.append(kw)
        raise _Stop
    noise, c, uc = _inputs()
    for name in ("DDIM_Gaussian", "DDIM", "UniPC"):
        smp = samplers.Txt2VideoSampler(_FreeuPortModel(), torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
        got = []
        smp.sampler.sample = lambda **kw: (got.append(kw), noise)[1]
        kw = dict(steps=4, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape), noise=noise,
                  guidance_scale=9.0, sampler_name=name)
        smp.sample_loop(**kw)
        smp.sample_loop(**kw, freeu=VALUES)
        assert "freeu" not in got[0] and got[1]["freeu"] == VALUES
    monkeypatch.setattr(samplers.Txt2VideoSampler, "sample_loop", sample_loop)
    net = U.UNetSD(**configs.TINY_UNET, init_weights=False)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, device="cpu")
    pipe.preprocess = lambda *a, **k: (c, uc)
    with pytest.raises(_Stop):
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, device="cpu", freeu=VALUES)
    with pytest.raises(_Stop):
        pipe.infer_conditioned(c, uc, 2, 3, 1, 9.0, 128, 128, device="cpu")
    with pytest.raises(_Stop):
        pipe.infer("a", "b", 2, 3, 1, 9.0, 128, 128, cpu_vae="CPU (full precision)", device="cpu", freeu=VALUES)
    with pytest.raises(_Stop):
        pipeline.process_modelscope(dict(pipe=pipe, cond=c, uncond=uc, steps=2, frames=3, seed=1, cfg_scale=9.0, width=128, height=128, freeu=VALUES))
    assert [kw.get("freeu") for kw in seen] == [VALUES, None, VALUES, VALUES] and "freeu" not in seen[1]


def test_refusals(cpu_kernels):  # noqa: F811
    noise, c, uc = _inputs()
    model = _FreeuPortModel()
    for name in ("DDIM_Gaussian", "DDIM", "UniPC"):
        smp = samplers.Txt2VideoSampler(model, torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name)
        kw = dict(S=2, batch_size=1, shape=tuple(noise.shape), conditioning=c, unconditional_conditioning=uc, x_T=noise, unconditional_guidance_scale=9.0)
        for bad in ({"b1": 1.2, "b2": 1.4, "s1": 0.9}, dict(VALUES, s3=1.0), dict(VALUES, b1=float("nan")), dict(VALUES, s2=float("inf")),
                    dict(VALUES, b2="1.4"), (1.2, 1.4, 0.9, 0.2), {}):
            with pytest.raises(ValueError, match="freeu"):
                smp.sampler.sample(**kw, freeu=bad)
            with pytest.raises(ValueError, match="freeu"):
                smp.sample_loop(steps=2, strength=None, conditioning=c, unconditional_conditioning=uc, batch_size=1, shape=tuple(noise.shape),
                                noise=noise, guidance_scale=9.0, sampler_name=name, freeu=bad)
        smp.sampler.cfg_parallel = types.SimpleNamespace(size=2, role=0)
        with pytest.raises(NotImplementedError, match="CFG-pair"):
            smp.sampler.sample(**kw, freeu=VALUES)
        smp.sampler.cfg_parallel = None
        model.t_shard = object()
        try:
            with pytest.raises(NotImplementedError, match="T-shard"):
                smp.sampler.sample(**kw, freeu=VALUES)
        finally:
            del model.t_shard
        with pytest.raises(NotImplementedError, match="enable_freeu"):
            samplers.Txt2VideoSampler(_PortModel(), torch.device("cpu"), betas=tp.beta_schedule_linear_sd(), sampler_name=name).sampler.sample(**kw, freeu=VALUES)
        assert not model.seen and model._freeu is None
    # the network's own switch
    net = U.UNetSD(**configs.TINY_UNET, init_weights=False)
    with pytest.raises(ValueError, match="freeu"):
        net.enable_freeu(s1=0.9, s2=0.2, b1=float("nan"), b2=1.4)
    with pytest.raises(AttributeError):
        net.freeu = VALUES                                                 # read-only
    net.enable_freeu(**ON)
    from sd_webui_text2video_amd.program import TShardSpec
    with pytest.raises(NotImplementedError, match="T-shard"):
        net._compile(1, 2, 8, 8, 5, "f32", "f32", "f32", shard=TShardSpec.make(4, 2, 0))
    # the VideoCrafter path
    vnet = videocrafter.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    with pytest.raises(NotImplementedError, match="VideoCrafter"):
        vnet.enable_freeu(**ON)
    assert vnet.freeu is None
    vc = object.__new__(videocrafter.DDIMSampler)
    with pytest.raises(NotImplementedError, match="VideoCrafter"):
        vc.sample(S=2, batch_size=1, shape=(4, 6, 8, 8), freeu=VALUES)
    with pytest.raises(NotImplementedError, match="VideoCrafter"):
        videocrafter.process_videocrafter(dict(model=None, prompt="a", steps=2, seed=1, freeu=VALUES))


def test_record_validation_without_gpu(built_lib):
    import ctypes
    h, ptr = ctypes.c_void_p(), 0x1000

    def create(i, f=(1.2, 0.9), p=ptr):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_FREEU
        for k, v in enumerate(i):
            op[0].i[k] = v
        op[0].f[0], op[0].f[1] = f
        op[0].p[0] = p
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    good = (24, 96, 104, 64, 2, 3, 4)
    assert create(good)[0] == 0 and create((24, 96, 96, 96, 2, 3, 4))[0] == 0            # (no skip at all: only the scaled half)
    for i, kw, needle in (((24, 96, 104, 63, 2, 3, 4), {}, b"even"), ((24, 96, 104, 0, 2, 3, 4), {}, b"even"), ((24, 96, 104, 98, 2, 3, 4), {}, b"exceeds C_total"),
                          ((25, 96, 104, 64, 2, 3, 4), {}, b"rows != frames * h * w"), (good, dict(p=0), b"null freeu pointer"),
                          ((24, 96, 90, 64, 2, 3, 4), {}, b"leading dimension"), (good, dict(f=(float("nan"), 1.0)), b"finite"),
                          (good, dict(f=(1.0, float("inf"))), b"finite"), ((0, 96, 104, 64, 0, 3, 4), {}, b"positive"), (good, dict(p=ptr + 2), b"aligned"),
                          ((2 * 2000 * 4, 96, 104, 64, 2, 2000, 4), {}, b"1024")):
        rc, msg = create(i, **kw)
        assert rc == -1 and needle in msg and b"freeu" in msg, (i, kw, rc, msg)
    assert L.OP_FREEU == 27 and L.ABI_VERSION == built_lib.t2v_abi_version()
