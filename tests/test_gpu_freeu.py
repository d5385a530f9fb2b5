"""GPU (-m gpu): FreeU on the device — T2V_OP_FREEU on the designed operands of tests/freeu_inputs.py against the float64 restatement
(tests/freeu_ref.py), and the tiny UNet with FreeU end to end.

Op level, every geometry with ld = C_total + 8 and NaN-filled guard columns: the scaled columns equal float32(x) * float32(b) bit for
bit; the untouched half of the stream and the guard columns keep their bits; the filtered columns lie within 4 x the maximum absolute
error of the fp32 torch.fft formulation (what FreeU itself computes) against float64 on the same operand — the margin is for a
different summation order of the same O(n eps) sums; b = s = 1 changes no value; two runs give the same bits; a NaN stays in its
(frame, channel) plane.  What the operands expose: tests/test_freeu_inputs_cpu.py.

Network level: the forward against the REAL reference with FreeU hooks (tests/golden/freeu_tiny.npz) at the gate of the plain tiny
forward (tests/test_gpu_e2e.py, 3.1e-3), the shared-prefix forward against the batched one, three DDIM_Gaussian steps against the
reference's latents at the few-step gate of the sampler tests (2e-2), context windows with FreeU against the windows evaluated one by
one (3e-3, tests/test_gpu_context_windows.py), and a call without the keyword after one with it, bit for bit."""
import os

import numpy as np
import pytest
import torch

import freeu_inputs as FI
from harness import rel_l2
from interp_freeu import FreeuInterp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers
from sd_webui_text2video_amd import unet as U
from sd_webui_text2video_amd.program import BoundProgram, Program

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "freeu_tiny.npz"))
VALUES = dict(zip(("b1", "b2", "s1", "s2"), (float(v) for v in GOLD["freeu"])))


# ---- 1. the op -----------------------------------------------------------------------------------------------------------------------------
def run_op(X: torch.Tensor, geom, b=FI.B, s=FI.S) -> torch.Tensor:
    """T2V_OP_FREEU on the operand X [rows, C_total + GUARD] (a copy) -> the buffer after the launch, on the host."""
    frames, h, w, c_h, c_s = geom
    P = Program("freeu op")
    fence = P.alloc(1, 64, "f32")                       # NaN rows in front of and behind the buffer: nothing outside it may change
    buf = P.alloc(frames * h * w, c_h + c_s, "f32", ld=c_h + c_s + FI.GUARD)
    fence2 = P.alloc(1, 64, "f32")
    P.freeu("freeu", buf, c_h=c_h, frames=frames, h=h, w=w, b=b, s=s)
    host = FreeuInterp(P, {})                           # (NaN-poisoned arena)
    host.mat(buf.ref, buf.rows, buf.ld, buf.ld, torch.float32, {}).copy_(X)
    before = host.arena.clone()
    arena = host.arena.to(DEV)
    BoundProgram(P, arena.data_ptr(), {}).run({}, torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    torch.cuda.synchronize()
    L.async_status()
    host.arena = arena.cpu()
    for f in (fence, fence2):                           # bytes outside the buffer keep their bits
        lo, hi = f.ref.off, f.ref.off + f.rows * f.ld * 4
        assert torch.equal(host.arena[lo:hi], before[lo:hi])
    return host.mat(buf.ref, buf.rows, buf.ld, buf.ld, torch.float32, {}).clone()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check(out, X, geom, b=FI.B, s=FI.S, what=""):
    """The record's contract on one operand -> (kernel error, fp32 torch.fft error), both maximum absolute against float64."""
    frames, h, w, c_h, c_s = geom
    c_total = c_h + c_s
    b32 = torch.tensor(b, dtype=torch.float32)
    assert same_bits(out[:, :c_h // 2], X[:, :c_h // 2] * b32), (what, geom, "scaled columns")
    assert same_bits(out[:, c_h // 2:c_h], X[:, c_h // 2:c_h]), (what, geom, "untouched half of the stream")
    assert same_bits(out[:, c_total:], X[:, c_total:]) and torch.isnan(out[:, c_total:]).all(), (what, geom, "guard columns")
    ref = FI.reference(X, geom, b, s)[:, c_h:c_total]
    e_kernel = (out[:, c_h:c_total].double() - ref).abs().max().item()
    e_fft = (FI.fp32_fft(X, geom, s).double() - ref).abs().max().item()
    print(f"freeu {what} {geom}: kernel {e_kernel:.3e}, fp32 torch.fft {e_fft:.3e} (max abs against float64; gate 4 x the latter)")
    assert e_kernel <= 4 * e_fft, (what, geom, e_kernel, e_fft)
    return e_kernel, e_fft


@pytest.mark.parametrize("geom", FI.GEOMS)
def test_op_against_the_float64_restatement(geom):
    X = FI.operand("noise", geom)
    out = run_op(X, geom)
    check(out, X, geom, what="noise")
    assert same_bits(run_op(X, geom), out)                                  # two runs, the same bits
    same = run_op(X, geom, b=1.0, s=1.0)
    c_total = geom[3] + geom[4]
    assert torch.equal(same[:, :c_total], X[:, :c_total])                   # b = s = 1: every value equal


@pytest.mark.parametrize("geom", FI.GEOMS)
@pytest.mark.parametrize("name", ["cos_y", "cos_x", "cos_minus", "cos_plus"])
def test_op_on_the_designed_operands(name, geom):
    X = FI.operand(name, geom)
    check(run_op(X, geom), X, geom, what=name)


def test_a_nan_stays_in_its_frame_and_channel():
    geom = (3, 3, 5, 64, 96)
    frames, h, w, c_h, c_s = geom
    X = FI.operand("noise", geom)
    clean = run_op(X, geom)
    X[1 * h * w + 7, c_h + 5] = float("nan")
    X[2 * h * w + 1, 3] = float("inf")                 # and one in the scaled half: an ordinary product
    out = run_op(X, geom)
    hit = torch.zeros_like(out, dtype=torch.bool)
    hit[h * w:2 * h * w, c_h + 5] = True
    hit[2 * h * w + 1, 3] = True
    assert torch.isnan(out[h * w:2 * h * w, c_h + 5]).all() and out[2 * h * w + 1, 3] == float("inf")
    assert same_bits(out[~hit], clean[~hit])


def test_malformed_records_are_refused_before_launch():
    lib = L.load()
    x = torch.zeros(24, 104, device=DEV)

    def create(i, f=(1.2, 0.9), p=None):
        op = (L.T2VOp * 1)()
        op[0].kind = L.OP_FREEU
        for k, v in enumerate(i):
            op[0].i[k] = v
        op[0].f[0], op[0].f[1] = f
        op[0].p[0] = x.data_ptr() if p is None else p
        rc = lib.t2v_run_ops(op, 1, None, 0, None)
        return rc, lib.t2v_last_error()

    good = (24, 96, 104, 64, 2, 3, 4)
    for i, kw, needle in (((24, 96, 104, 63, 2, 3, 4), {}, b"even"), ((24, 96, 104, 98, 2, 3, 4), {}, b"exceeds C_total"),
                          ((25, 96, 104, 64, 2, 3, 4), {}, b"rows != frames * h * w"), (good, dict(p=0), b"null freeu pointer"),
                          ((24, 96, 90, 64, 2, 3, 4), {}, b"leading dimension"), (good, dict(f=(float("nan"), 1.0)), b"finite")):
        rc, msg = create(i, **kw)
        assert rc == -1 and needle in msg and b"freeu" in msg, (i, kw, rc, msg)
    torch.cuda.synchronize()
    assert not x.any()                                  # nothing ran
    assert create(good)[0] == 0


# ---- 2. the network ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    betas = tp.beta_schedule_linear_sd()
    net.register_schedule(given_betas=betas.numpy())
    return net, betas


def _inputs():
    """The draws of tests/golden/make_golden_freeu.py:inputs."""
    cfg = configs.TINY_UNET
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 3, 16, 16, generator=g)
    y = torch.randn(2, 7, cfg["context_dim"], generator=g)
    g2 = torch.Generator().manual_seed(17)
    x_odd = torch.randn(1, 4, 2, 40, 72, generator=g2)
    c = torch.randn(1, 7, cfg["context_dim"], generator=g2)
    uc = torch.randn(1, 7, cfg["context_dim"], generator=g2)
    return x[:, :, :, :8, :8].contiguous(), y, torch.tensor([801, 401]), x_odd, c, uc


FORWARD_GATE = 3.1e-3            # tests/test_gpu_e2e.py::test_tiny_unet_forward_matches_reference_golden


def test_forward_with_freeu_matches_the_reference_with_hooks(tiny):
    net, _ = tiny
    x, y, t, x_odd, c, _ = _inputs()
    plain = net(x.to(DEV), t.to(DEV), y.to(DEV)).float().cpu()
    net.enable_freeu(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
    try:
        e64 = net(x.to(DEV), t.to(DEV), y.to(DEV)).float().cpu()
        eodd = net(x_odd.to(DEV), torch.tensor([601]).to(DEV), c.to(DEV)).float().cpu()
    finally:
        net.disable_freeu()
    r64, rodd = rel_l2(e64, torch.from_numpy(GOLD["eps_64"])), rel_l2(eodd, torch.from_numpy(GOLD["eps_odd"]))
    print(f"tiny forward with FreeU: rel-L2 {r64:.3e} (8 x 8 latent), {rodd:.3e} (40 x 72 latent) against the reference with hooks (gate {FORWARD_GATE})")
    assert r64 < FORWARD_GATE and rodd < FORWARD_GATE
    assert rel_l2(e64, plain) > 10 * FORWARD_GATE                         # and FreeU is not a no-op
    again = net(x.to(DEV), t.to(DEV), y.to(DEV)).float().cpu()
    assert torch.equal(again, plain)                                       # off again: the program without it, bit for bit


def test_shared_prefix_forward_equals_the_batched_one(tiny):
    net, _ = tiny
    x, y, t, *_ = _inputs()
    x1, t1 = x[:1].to(DEV), t[:1].to(DEV)
    net.enable_freeu(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
    try:
        assert net.share_cfg_prefix
        shared = net.forward_cfg_pair(x1, t1, y.to(DEV)).float().cpu()
        key = [k for k in net._programs if ("share",) in k and any(isinstance(e, tuple) and e[:1] == ("freeu",) for e in k)]
        assert key, list(net._programs)
        batched = net(torch.cat([x1, x1]), t1.repeat(2), y.to(DEV)).float().cpu()
    finally:
        net.disable_freeu()
    r = rel_l2(shared, batched)
    print(f"shared-prefix forward with FreeU against the batched one: rel-L2 {r:.3e} (gate {FORWARD_GATE})")
    assert r < FORWARD_GATE


def test_three_ddim_gaussian_steps_match_the_reference(tiny):
    net, betas = tiny
    *_, c, uc = _inputs()
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM_Gaussian")
    smp.progress = False
    _, noise, shape = smp.get_noise(1, 4, 3, 128, 128, seed=1234)
    kw = dict(steps=3, strength=None, conditioning=c.to(DEV), unconditional_conditioning=uc.to(DEV), batch_size=1, shape=shape, noise=noise,
              guidance_scale=9.0, eta=0.0, sampler_name="DDIM_Gaussian")
    before = smp.sample_loop(**kw).float().cpu()
    got = smp.sample_loop(**kw, freeu=VALUES).float().cpu()
    assert net.freeu is None
    r = rel_l2(got, torch.from_numpy(GOLD["latents"]))
    print(f"3 DDIM_Gaussian steps with FreeU: rel-L2 {r:.3e} against the reference's latents (gate 2e-2)")
    assert r < 2e-2
    assert rel_l2(got, torch.from_numpy(GOLD["plain_latents"])) > 0.1
    after = smp.sample_loop(**kw).float().cpu()
    assert torch.equal(after, before)                                      # a call without the keyword after one with it: the same bits


def test_context_windows_with_freeu_equal_the_windows_one_by_one(tiny):
    import test_gpu_context_windows as TW
    net, betas = tiny
    c, uc = TW._cond()
    noise = TW._noise((1234,))
    kw = dict(S=TW.STEPS, conditioning=c, unconditional_conditioning=uc, shape=tuple(noise.shape), unconditional_guidance_scale=TW.SCALE, eta=0.0)
    smp = samplers.Txt2VideoSampler(net, torch.device(DEV), betas=betas, sampler_name="DDIM_Gaussian")
    got = smp.sampler.sample(x_T=noise, context_windows=TW.WINDOWS, freeu=VALUES, **kw).float().cpu()
    assert net.freeu is None
    net.enable_freeu(s1=VALUES["s1"], s2=VALUES["s2"], b1=VALUES["b1"], b2=VALUES["b2"])
    try:
        ref = samplers.GaussianDiffusion(TW._Composed(net), betas).sample(x_T=noise, **kw).float().cpu()
    finally:
        net.disable_freeu()
    r = rel_l2(got, ref)
    print(f"context windows with FreeU against single-window forwards: rel-L2 {r:.3e} (gate 3e-3)")
    assert r < 3e-3
    assert rel_l2(got, smp.sampler.sample(x_T=noise, context_windows=TW.WINDOWS, **kw).float().cpu()) > 1e-2
