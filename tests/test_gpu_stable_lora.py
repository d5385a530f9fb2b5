"""GPU (-m gpu): the Stable LoRA merge on the device.  (1) T2V_OP_LORA_MERGE alone: ONE launch over mixed segments — fp16 and fp32, both forms,
r in {1, 3, 64}, weights of exactly one tile, one element less and one more, a [1, 1] weight, weights and factors one element past a 16-byte
boundary — against the numpy statement of the contract (tests/stable_lora_ref.py): fp16 bytes equal, fp32 inside twice the first-order
rounding bound, NaN guard regions around every weight bit-identical afterwards; positive and negative alpha.  (2) The tiny UNet end to end:
the device merge reproduces the digests the reference's own process_lora left on its fp16 tiny UNet (merge, undo, two files); the fp32 model's
merged forward against the reference's merged eps, back inside the gate after the undo with a partial re-pack; an alpha change through
StableLoraScript.process against a fresh load; process_modelscope with and without the `stable_lora` entry."""
import types

import numpy as np
import pytest
import torch

import stable_lora_ref as R
from harness import rel_l2
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import stable_lora as SL
from sd_webui_text2video_amd import unet as U, vae as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 3.1e-3                      # the gate of test_tiny_unet_forward_matches_reference_golden
GUARD = 64                         # guard elements on either side of every weight (a multiple of a 16-byte vector)
TILE = L.LORA_TILE
NP = {"f16": np.float16, "f32": np.float32}
# (weight shape, r, form, dtype, offset of W in elements past its guard, offset of the factors)
CASES = [
    ((6, 10), 3, R.DIRECT, "f16", 1, 0),
    ((1, 1), 1, R.DIRECT, "f16", 0, 0),
    ((64, TILE // 64), 3, R.DIRECT, "f16", 1, 1),            # exactly one tile; W and A both one element past a boundary: vector loads of A
    ((63, 65), 1, R.DIRECT, "f16", 0, 0),                    # one tile - 1: rows end inside vectors
    ((17, 241), 64, R.DIRECT, "f16", 0, 1),                  # one tile + 1: the second tile is one element
    ((8, 128), 64, R.DIRECT, "f16", 0, 0),                   # everything aligned
    ((5, 7, 3, 1, 1), 3, R.TEMPORAL, "f16", 1, 0),
    ((64, 64, 3, 1, 1), 64, R.TEMPORAL, "f16", 0, 0),        # three tiles, aligned: vector loads of A
    ((6, 10), 3, R.DIRECT, "f32", 1, 0),
    ((63, 65), 64, R.DIRECT, "f32", 0, 1),
    ((64, TILE // 64), 1, R.DIRECT, "f32", 0, 0),
    ((5, 7, 3, 1, 1), 1, R.TEMPORAL, "f32", 1, 1),
    ((64, 64, 3, 1, 1), 3, R.TEMPORAL, "f32", 0, 0),
]


@pytest.fixture(scope="module")
def kernel_cases():
    """Host arrays of every case, made once: W, A (one large column, one zero row), B (one zero row)."""
    rng = np.random.default_rng(26)
    out = []
    for shape, r, form, dt, w_off, f_off in CASES:
        N, J = shape[0], int(np.prod(shape[1:]))
        Jf = 3 * J if form == R.TEMPORAL else J
        W = rng.standard_normal(shape).astype(NP[dt])
        A = (0.25 * rng.standard_normal((r, Jf))).astype(NP[dt])
        B = (0.25 * rng.standard_normal((N, r))).astype(NP[dt])
        A[:, Jf // 2] *= 37.0
        if r > 1:
            A[r // 2, :] = 0
        if N > 1:
            B[N // 2, :] = 0
        out.append((W, A, B))
    return out


def _place(arr, offset):
    """arr on the device between NaN guards, `offset` elements past a 16-byte boundary -> (whole buffer, view of the payload)."""
    t = torch.from_numpy(arr.reshape(-1).copy())
    buf = torch.full((GUARD + offset + t.numel() + GUARD + 8,), float("nan"), dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + offset: GUARD + offset + t.numel()]
    view.copy_(t.to(DEV))
    return buf, view


@pytest.mark.parametrize("alpha", [0.7, -0.35])
def test_one_launch_over_mixed_segments_matches_the_contract(kernel_cases, alpha):
    placed, segments = [], []
    for (shape, r, form, dt, w_off, f_off), (W, A, B) in zip(CASES, kernel_cases):
        wb, wv = _place(W, w_off)
        ab, av = _place(A, f_off)
        bb, bv = _place(B, f_off)
        assert wv.data_ptr() % 16 == w_off * W.itemsize
        snapshot = wb.clone()
        placed.append((wb, wv, snapshot, ab, bb))
        segments.append((wv.data_ptr(), av.data_ptr(), bv.data_ptr(), shape[0], W.size // shape[0], r, form, L.F16 if dt == "f16" else L.F32))
    tables = SL.merge_device(segments, alpha, torch.device(DEV))
    torch.cuda.synchronize()
    assert tables[1].shape[0] == sum(-(-W.size // TILE) for W, _, _ in kernel_cases)
    bad = []                                                   # every case is looked at; the figures of all failures are reported together
    for (shape, r, form, dt, w_off, f_off), (W, A, B), (wb, wv, snapshot, ab, bb) in zip(CASES, kernel_cases, placed):
        tag = (shape, r, form, dt, w_off, f_off)
        got = wv.cpu().numpy().reshape(shape)
        bits = torch.int16 if dt == "f16" else torch.int32
        lo, hi = GUARD + w_off, GUARD + w_off + W.size
        if not (torch.equal(wb[:lo].view(bits), snapshot[:lo].view(bits)) and torch.equal(wb[hi:].view(bits), snapshot[hi:].view(bits))):
            bad.append(("guard region changed", tag))
        if dt == "f16":
            want = R.merge_f16(W, A, B, alpha, form)
            if got.tobytes() != want.tobytes():
                idx = np.flatnonzero(got.reshape(-1).view(np.uint16) != want.reshape(-1).view(np.uint16))
                bad.append((tag, f"{idx.size} of {W.size} elements differ", [(int(i), float(W.reshape(-1)[i]), float(got.reshape(-1)[i]),
                                                                          float(want.reshape(-1)[i])) for i in idx[:6]]))
            if got.tobytes() == W.tobytes():
                bad.append((tag, "nothing was merged"))
        else:
            w_star, S = R.merge_f64(W, A, B, alpha, form)
            err = np.abs(got.astype(np.float64) - w_star)
            bound = R.f32_bound(w_star, S, alpha, r)
            print(f"fp32 {tag}: largest error / bound {float((err / bound).max()):.3f}")
            if not np.all(err <= bound):
                bad.append((tag, "error / bound", float((err / bound).max())))
            if not np.isfinite(got).all() or np.array_equal(got, W):
                bad.append((tag, "not finite, or nothing was merged"))
    assert not bad, bad


# ---- the tiny UNet -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    g = R.golden()
    g["f1"] = {k: torch.from_numpy(v.copy()) for k, v in g["file1"].items()}
    g["f2"] = {k: torch.from_numpy(v.copy()) for k, v in g["file2"].items()}
    g["eps0"] = torch.from_numpy(np.load(R.GOLDEN.replace("stable_lora_tiny.npz", "tiny.npz"))["unet_eps"])
    return g


def _inputs():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 3, 16, 16, generator=g)
    y = torch.randn(2, 7, configs.TINY_UNET["context_dim"], generator=g)
    z = torch.randn(2, 4, 8, 8, generator=g)
    c = torch.randn(1, 7, configs.TINY_UNET["context_dim"], generator=g)
    uc = torch.randn(1, 7, configs.TINY_UNET["context_dim"], generator=g)
    return x, torch.tensor([801, 401]), y, c, uc


def _net(half):
    net = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(net, seed=0)
    net.register_schedule(given_betas=tp.beta_schedule_linear_sd().numpy())
    return (net.half() if half else net).to(DEV)


def _forward(net):
    x, t, y, *_ = _inputs()
    return net(x.to(DEV), t.to(DEV), y.to(DEV)).float().cpu()


ON = (True, True, True, True, True)            # use_bias, use_time, use_conv, use_emb, use_linear


def test_device_merge_reproduces_the_references_bytes(gold):
    net = _net(half=True)
    mods = dict(net.named_modules())
    watched = gold["touched"] + gold["untouched"]

    def digests():
        return [R.digest(mods[n].weight.detach().cpu().numpy()) for n in watched]

    assert digests() == gold["sha_original"]
    proc = SL.StableLoraProcessor()
    touched = proc.process_lora(net, [gold["f1"]], *ON, gold["alpha"])
    assert touched == [n + ".weight" for n in gold["touched"]]
    assert digests() == gold["sha_merged"]
    proc.process_lora(net, [gold["f1"]], *ON, gold["alpha"], undo_merge=True)
    assert digests() == gold["sha_undone"]
    proc.process_lora(net, [gold["f1"], gold["f2"]], *ON, gold["alpha"])
    assert digests() == gold["sha_two_files"]


def test_fp32_model_merged_forward_and_undo(gold):
    net = _net(half=False)
    r0 = rel_l2(_forward(net), gold["eps0"])
    n_images = len(net._packed)
    proc = SL.StableLoraProcessor()
    proc.process_lora(net, [gold["f1"]], *ON, gold["alpha"])
    assert 0 < net.last_repack < n_images // 2
    eps = _forward(net)
    r_merged, r_apart = rel_l2(eps, torch.from_numpy(gold["eps_merged"])), rel_l2(eps, gold["eps0"])
    proc.process_lora(net, [gold["f1"]], *ON, gold["alpha"], undo_merge=True)
    repacked = net.last_repack
    r_back = rel_l2(_forward(net), gold["eps0"])
    print(f"tiny fp32: un-merged {r0:.3e}, merged vs the reference's merged eps {r_merged:.3e}, merged vs un-merged {r_apart:.3e} "
          f"({r_apart / GATE:.0f} gates), after the undo {r_back:.3e}; {repacked} of {n_images} images re-packed")
    assert r0 < GATE and r_merged < GATE, (r0, r_merged)
    assert r_apart > 50 * GATE, r_apart
    assert r_back < GATE and 0 < repacked < n_images // 2, (r_back, repacked, n_images)
    assert net.verify_weights(DEV) == []                       # the recorded fingerprints followed the new bytes


def test_alpha_change_through_the_script_equals_a_fresh_load(gold):
    flags = dict(use_bias=True, use_linear=True, use_conv=True, use_emb=True, use_multiplier=1, use_time=True)
    a = types.SimpleNamespace(sd_model=_net(half=False), clip_encoder=None)
    script = SL.StableLoraScript()
    script.log = lambda *x: None
    _forward(a.sd_model)                                       # a live pack before the first load
    script.process(a, [gold["f1"]], 1.0, **flags)
    eps_1 = _forward(a.sd_model)
    script.process(a, [gold["f1"]], 0.5, **flags)              # undo at 1.0, merge at 0.5
    eps_a = _forward(a.sd_model)
    b = types.SimpleNamespace(sd_model=_net(half=False), clip_encoder=None)
    fresh = SL.StableLoraScript()
    fresh.log = lambda *x: None
    fresh.process(b, [gold["f1"]], 0.5, **flags)
    eps_b = _forward(b.sd_model)
    r, moved = rel_l2(eps_a, eps_b), rel_l2(eps_1, eps_b)
    print(f"alpha 1.0 -> 0.5 through the script vs a fresh load at 0.5: {r:.3e}; alpha 1.0 vs 0.5: {moved:.3e}")
    assert r < GATE and moved > 10 * GATE, (r, moved)
    script.process(a, [], 0.5, **flags)                        # selection emptied: unloaded
    assert not script.is_lora_loaded(a.sd_model) and rel_l2(_forward(a.sd_model), gold["eps0"]) < GATE


def test_process_modelscope_applies_the_selection(gold):
    from sd_webui_text2video_amd import pipeline
    *_, c, uc = _inputs()
    net = _net(half=True)
    ae = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4, init_weights=False)
    ae.load_state_dict(synth.synth_state_dict(synth.param_spec(ae), seed=3), strict=True)
    pipe = pipeline.TextToVideoSynthesis(sd_model=net, autoencoder=ae, betas=tp.beta_schedule_linear_sd(), device=DEV)
    pipe.diffusion.progress = False
    args = dict(pipe=pipe, cond=c.half(), uncond=uc.half(), steps=2, frames=3, seed=1234, cfg_scale=9.0, width=128, height=128, eta=0.0,
                sampler="DDIM_Gaussian", cpu_vae="GPU")
    lora = dict(lora_files_selection=[gold["f1"]], lora_alpha=1.0)
    base = np.stack(pipeline.process_modelscope(dict(args)))
    again = np.stack(pipeline.process_modelscope(dict(args)))
    assert np.array_equal(base, again) and not hasattr(net, "lora_loaded")           # no entry: nothing changes, bit for bit
    merged = np.stack(pipeline.process_modelscope(dict(args, stable_lora=lora)))
    assert hasattr(net, "lora_loaded") and merged.shape == base.shape
    changed = float((merged.astype(np.int32) != base.astype(np.int32)).mean())
    print(f"process_modelscope with the LoRA: {100 * changed:.1f} % of the uint8 values differ")
    assert changed > 0.05
    same = np.stack(pipeline.process_modelscope(dict(args, stable_lora=lora)))       # nothing changed since: no undo, no merge
    assert np.array_equal(same, merged)
    by_extra_args = np.stack(pipeline.process_modelscope(dict(args), extra_args=[[gold["f1"]], 1.0, True, True, True, True, 1, True]))
    assert np.array_equal(by_extra_args, merged)
