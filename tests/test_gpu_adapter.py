"""GPU (-m gpu): VideoCrafter depth adapter through the C ABI against golden outputs of the REAL reference
(tests/golden/make_golden_adapter.py: Adapter, UNetModel.forward(features_adapter=), the DDIM loop with features) and the
end-to-end entry point `adapter_guided_synthesis`.

Gates.  UNet forwards / the DDIM loop with features: the gates of the same forwards without features (tests/test_gpu_videocrafter.py:
4e-3 fp32 weights, 8e-3 fp16, 2e-2 the tiny 4-step loop), and no more than 10 % above the error of the same forward without features,
measured in the same test.  Adapter features: measured on the MI355X + 10 % per line (profiles/adapter_parity.txt, DESIGN.md
section 3 convention), every line below 4e-3."""
import os
import types

import numpy as np
import pytest
import torch

import adapter_ref as AR
from harness import rel_l2
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import videocrafter as VC

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
SEED_ADAPTER = 11

# rel-L2 gate of every adapter feature against the reference golden: the MI355X figure of profiles/adapter_parity.txt x 1.1
_MEASURED = {
    ("t2i", 0): 4.249e-4, ("t2i", 1): 4.913e-4, ("t2i", 2): 4.662e-4,
    ("full", 0): 4.330e-4, ("full", 1): 6.495e-4, ("full", 2): 7.319e-4,
    ("conv", 0): 3.888e-4, ("conv", 1): 7.499e-4, ("conv", 2): 7.931e-4,
    ("released", 0): 4.367e-4, ("released", 1): 5.730e-4, ("released", 2): 6.176e-4, ("released", 3): 5.872e-4,
}
FEATURE_GATES = {k: 1.1 * v for k, v in _MEASURED.items()}
assert max(FEATURE_GATES.values()) <= 4e-3


def _gold(name):
    return np.load(os.path.join(GOLD, name))


def _inputs_tiny():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 5, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


@pytest.fixture(scope="module")
def tiny_ld():
    """T2VAdapterDepth on the tiny UNet / VAE with a one-level adapter whose feature fits the UNet's single site (320 channels at
    half the 8 x 8 latent = 1/8 of 32 x 32 depth frames) and a stand-in depth estimator (the MiDaS network is outside the package)."""
    def depth_model(frames):                  # [n, 3, H, W] -> [n, 1, H, W], on the device
        return frames.float().mean(dim=1, keepdim=True) * 3.0 + 5.0
    ld = VC.T2VAdapterDepth(depth_model, dict(params=dict(channels=[320], nums_rb=2, cin=64, ksize=1, sk=True, use_conv=False), cond_name="depth"),
                            configs.TINY_LVDM_UNET, dict(ddconfig=configs.TINY_VAE_DDCONFIG, embed_dim=4), image_size=[8, 8],
                            video_length=5, init_weights=False, **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    sd = synth.synth_state_dict(synth.param_spec(net), seed=0)
    net.load_state_dict(sd, strict=True)
    ld.first_stage_model.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.first_stage_model), seed=3), strict=True)
    ld.adapter.load_state_dict(synth.synth_state_dict(synth.param_spec(ld.adapter), seed=SEED_ADAPTER), strict=True)
    assert ld.condtype == "depth" and any(k.startswith("adapter.body.0.block1") for k in ld.state_dict())
    return ld.to(DEV), sd


# ---- case 1: the adapter alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AR.OPTION_SETS))
def test_adapter_features_match_reference_golden(name):
    gold = _gold("lvdm_adapter_small.npz")
    net = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS[name], init_weights=False)
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=SEED_ADAPTER), strict=True)
    net = net.to(DEV)
    depth = AR.small_depth().to(DEV)
    feats = net(depth, normalise=True)                     # raw depth in: the normalisation runs inside the front-end launch
    assert [tuple(f.shape) for f in feats] == [gold[f"{name}_feat{k}"].shape for k in range(3)]
    for k, f in enumerate(feats):
        r = rel_l2(f.float().cpu(), torch.from_numpy(gold[f"{name}_feat{k}"]))
        print(f"adapter[{name}] feature {k}: rel-L2 {r:.3e} (gate {FEATURE_GATES[(name, k)]:.2e})")
        assert f.dtype == torch.float32 and r < FEATURE_GATES[(name, k)], (name, k, r)
    # the two-call form of the reference (get_batch_depth, then the adapter) gives the same bits; a constant frame is exactly -1
    norm = net.normalise_depth(depth)
    assert norm.shape == depth.shape and bool((norm[2] == -1).all()) and float(norm.min()) == -1.0 and float(norm.max()) <= 1.0
    assert torch.equal(norm.cpu(), torch.from_numpy(gold["depth_norm"]).half().float())
    for a, b in zip(net(norm), feats):
        assert torch.equal(a, b)
    for a, b in zip(net(depth.half(), normalise=False), net(depth.half().float(), normalise=False)):     # fp16 depth in
        assert torch.equal(a, b)
    # a NaN pixel makes its own frame NaN (torch.amin / amax propagate it) and leaves the other frames alone
    bad = depth.clone()
    bad[1, 0, 5, 7] = float("nan")
    nb = net.normalise_depth(bad)
    assert bool(torch.isnan(nb[1]).all()) and torch.equal(nb[[0, 2, 3, 4]], norm[[0, 2, 3, 4]])


# ---- cases 2, 3: the tiny UNet and DDIM loop with a feature --------------------------------------------------------------------------
def test_tiny_unet_with_feature_matches_reference_golden(tiny_ld):
    ld, sd = tiny_ld
    net = ld.model.diffusion_model
    gold = _gold("lvdm_adapter_tiny.npz")
    base = torch.from_numpy(_gold("lvdm_tiny.npz")["unet_eps"])
    x, t, ctx, _ = _inputs_tiny()
    feat = AR.tiny_feature().to(DEV)
    out = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[feat])
    plain = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV))
    r, r0 = rel_l2(out.cpu(), torch.from_numpy(gold["unet_eps"])), rel_l2(plain.cpu(), base)
    print(f"tiny UNet forward: rel-L2 {r:.3e} with a feature, {r0:.3e} without")
    assert out.dtype == torch.float32 and r < 4e-3 and r <= 1.1 * r0, (r, r0)
    # zero features reproduce the run without features bit for bit; a non-zero feature changes the output
    zero = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[torch.zeros_like(feat)])
    assert torch.equal(zero, plain) and rel_l2(out.cpu(), plain.cpu()) > 0.05
    # fp16 features, and the caller's own scaling of them (a new list: converted once, then reused)
    half = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[feat.half()])
    assert rel_l2(half.cpu(), out.cpu()) < 1e-3
    scaled = [0.8 * feat]
    n0 = net.adapter_conversions
    s1 = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=scaled)
    s2 = net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=scaled)
    assert net.adapter_conversions == n0 + 1 and torch.equal(s1, s2) and not torch.equal(s1, out)
    # the [cond | uncond] batch of a guided step on ONE x_t: both roles receive the same feature (shared prefix on and off)
    t1 = torch.tensor([801, 801], device=DEV)
    for share in (True, False):
        net.share_cfg_prefix = share
        try:
            net.single_timestep = True
            pair = net(x[0:1].to(DEV), t1, context=ctx.to(DEV), features_adapter=[feat[0:1]])
        finally:
            net.share_cfg_prefix = True
        rp = rel_l2(pair.cpu(), torch.from_numpy(gold["unet_eps_pair"]))
        print(f"tiny UNet [cond | uncond] pair with a feature (shared prefix {share}): rel-L2 {rp:.3e}")
        assert rp < 4e-3
    with pytest.raises(AssertionError, match="Mismatch features adapter"):
        net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[feat, feat])
    with pytest.raises(ValueError, match="expected shape"):
        net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[feat[:, :, :, :2]])
    with pytest.raises(ValueError):
        net(x.to(DEV), t.to(DEV), context=ctx.to(DEV), features_adapter=[feat.cpu()])


def test_t_sharded_forward_with_features_is_refused(tiny_ld):
    ld, _ = tiny_ld
    net = ld.model.diffusion_model
    x, t, ctx, _ = _inputs_tiny()
    net.t_shard = types.SimpleNamespace(size=2)
    try:
        with pytest.raises(L.T2VError, match="T-sharded"):
            net(x[0:1].to(DEV), t[0:1].to(DEV), context=ctx[0:1].to(DEV), features_adapter=[AR.tiny_feature()[0:1].to(DEV)])
    finally:
        net.t_shard = None


def _sample(ld, ctx, x_T, feats, seed=123, eta=0.3, batch=1):
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(seed)
    x0, _ = smp.sample(S=4, conditioning={"c_crossattn": [ctx[0:1].to(DEV).repeat(batch, 1, 1)]}, batch_size=batch, shape=list(x_T.shape[1:]),
                       verbose=False, unconditional_guidance_scale=7.5,
                       unconditional_conditioning={"c_crossattn": [ctx[1:2].to(DEV).repeat(batch, 1, 1)]}, eta=eta, x_T=x_T.to(DEV),
                       features_adapter=feats, temporal_length=5, conditional_guidance_scale_temporal=None)
    return x0


def test_tiny_ddim_sampling_with_feature_matches_reference_golden(tiny_ld):
    ld, _ = tiny_ld
    net = ld.model.diffusion_model
    _, _, ctx, x_T = _inputs_tiny()
    gold = torch.from_numpy(_gold("lvdm_adapter_tiny.npz")["ddim_x0"])
    feats = [AR.tiny_feature()[0:1].to(DEV)]
    n0 = getattr(net, "adapter_conversions", 0)
    x0 = _sample(ld, ctx, x_T, feats)
    assert net.adapter_conversions == n0 + 1            # four steps, one layout conversion
    r = rel_l2(x0.cpu(), gold)
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(123)
    plain, _ = smp.sample(S=4, conditioning={"c_crossattn": [ctx[0:1].to(DEV)]}, batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                          unconditional_guidance_scale=7.5, unconditional_conditioning={"c_crossattn": [ctx[1:2].to(DEV)]}, eta=0.3,
                          x_T=x_T.to(DEV))
    r0 = rel_l2(plain.cpu(), torch.from_numpy(_gold("lvdm_tiny.npz")["ddim_x0"]))
    print(f"tiny 4-step DDIM loop: rel-L2 {r:.3e} with a feature, {r0:.3e} without")
    assert r < 2e-2 and r <= 1.1 * r0, (r, r0)
    with pytest.raises(NotImplementedError, match="conditional_guidance_scale_temporal"):
        VC.DDIMSampler(ld).sample(S=2, conditioning=ctx[0:1].to(DEV), batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
                                  features_adapter=feats, conditional_guidance_scale_temporal=2.0)
    # a guided batch of two videos == two single runs from the same x_T (eta = 0: no noise draw), each with its own feature
    g = torch.Generator().manual_seed(21)
    xT = torch.randn(2, 4, 5, 8, 8, generator=g)
    both = AR.tiny_feature().to(DEV)
    lat2 = _sample(ld, ctx, xT, [both], eta=0.0, batch=2)
    for v in range(2):
        lat1 = _sample(ld, ctx, xT[v:v + 1], [both[v:v + 1]], eta=0.0)
        assert rel_l2(lat2[v:v + 1].float().cpu(), lat1.float().cpu()) < 3e-3, v


def test_adapter_guided_synthesis_entry_point(tiny_ld):
    """sample_text2video_adapter.py:96-137: prompts + videos -> depth -> features -> DDIM -> decoded clips."""
    ld, _ = tiny_ld
    _, _, ctx, _ = _inputs_tiny()

    class Enc:            # stands in for FrozenCLIPEmbedder (outside the hot path)
        def encode(self, prompts):
            return (ctx[0:1] if prompts[0] == "a cat" else ctx[1:2]).to(DEV).repeat(len(prompts), 1, 1)
    ld.cond_stage_model = Enc()
    g = torch.Generator().manual_seed(61)
    videos = (torch.rand(1, 3, 5, 32, 32, generator=g) * 2 - 1).to(DEV)
    videos[:, :, 3] = 0.25                                   # a constant frame: depth normalises to -1
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(5)
    torch.manual_seed(0)
    out, extra = VC.adapter_guided_synthesis(ld, "a cat", videos, [1, 4, 5, 8, 8], n_samples=2, ddim_steps=4, ddim_eta=0.0,
                                             unconditional_guidance_scale=7.5, sampler=smp)
    assert out.shape == (1, 2, 3, 5, 64, 64) and out.dtype == torch.float32 and out.is_cuda and torch.isfinite(out).all()
    assert extra.shape == (1, 1, 5, 32, 32) and extra.dtype == torch.float32
    assert float(extra.min()) == -1.0 and float(extra.max()) <= 1.0 and bool((extra[:, :, 3] == -1).all())
    want = AR.normalise_depth((videos.float().mean(dim=1, keepdim=True) * 3.0 + 5.0)[0].permute(1, 0, 2, 3).cpu())
    assert (extra[0].permute(1, 0, 2, 3).cpu() - want).abs().max() < 1e-3            # (fp16 values of the reference's formula)
    # depth passed directly instead of videos + the estimator: same conditioning
    extra2 = ld.get_batch_depth(depth=videos.float().mean(dim=1, keepdim=True) * 3.0 + 5.0)
    assert torch.equal(extra2, extra)
    with pytest.raises(ValueError, match="must arrive at target_size"):
        ld.get_batch_depth(videos, (64, 64))
    # the latent is the one `sample` gives with the same features
    feats = ld.get_adapter_features(extra)
    assert [tuple(f.shape) for f in feats] == [(1, 320, 5, 4, 4)]
    torch.manual_seed(0)
    lat, _ = VC.DDIMSampler(ld).sample(S=4, conditioning=ld.get_learned_conditioning(["a cat"]), batch_size=1, shape=[4, 5, 8, 8], verbose=False,
                                       unconditional_guidance_scale=7.5, unconditional_conditioning=ld.get_learned_conditioning([""]), eta=0.0,
                                       features_adapter=feats)
    dec = ld.decode_first_stage(lat, decode_bs=1, return_cpu=False)
    assert torch.equal(dec, out[:, 0])
    # ... and differs from the clip without the features
    torch.manual_seed(0)
    lat0, _ = VC.DDIMSampler(ld).sample(S=4, conditioning=ld.get_learned_conditioning(["a cat"]), batch_size=1, shape=[4, 5, 8, 8], verbose=False,
                                        unconditional_guidance_scale=7.5, unconditional_conditioning=ld.get_learned_conditioning([""]), eta=0.0)
    assert rel_l2(lat0.cpu(), lat.cpu()) > 0.02


# ---- case 4: the released UNet with the features of the 77 M-parameter adapter ---------------------------------------------------------
@pytest.fixture(scope="module")
def released():
    net = VC.UNetModel(**configs.LVDM_UNET, init_weights=False)
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    ad = VC.Adapter(**AR.RELEASED, init_weights=False)
    ad.load_state_dict(synth.synth_state_dict(synth.param_spec(ad), seed=SEED_ADAPTER), strict=True)
    return net.to(DEV), ad.to(DEV)


def test_released_config_with_adapter_features_matches_reference_golden(released):
    net, ad = released
    gold = _gold("lvdm_adapter_16f.npz")
    ld = types.SimpleNamespace(adapter=ad)
    extra = VC.T2VAdapterDepth.get_batch_depth(ld, depth=AR.released_depth().to(DEV))
    feats = VC.T2VAdapterDepth.get_adapter_features(ld, extra)
    assert [tuple(f.shape) for f in feats] == [(1, 320, 16, 32, 32), (1, 640, 16, 16, 16), (1, 1280, 16, 8, 8), (1, 1280, 16, 4, 4)]
    for k, f in enumerate(feats):
        r = rel_l2(AR.subsample(f[0].permute(1, 0, 2, 3)).float().cpu(), torch.from_numpy(gold[f"feat{k}"]))
        print(f"adapter[released] feature {k}: rel-L2 {r:.3e} (gate {FEATURE_GATES[('released', k)]:.2e})")
        assert r < FEATURE_GATES[("released", k)], (k, r)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(1, 4, 16, 32, 32, generator=g)
    ctx = torch.randn(1, 77, 768, generator=g)
    t = torch.tensor([500], device=DEV)
    n0 = getattr(net, "adapter_conversions", 0)
    out = net(x.to(DEV), t, context=ctx.to(DEV), features_adapter=feats)
    assert net.adapter_conversions == n0 + 1 and net._adapter_cache[2][0].data_ptr() == feats[0].data_ptr()      # taken as stored: no copy
    plain = net(x.to(DEV), t, context=ctx.to(DEV))
    r, r0 = rel_l2(out.float().cpu(), torch.from_numpy(gold["unet_eps"])), rel_l2(plain.float().cpu(), torch.from_numpy(_gold("lvdm_16f.npz")["unet_eps"]))
    print(f"released UNet forward (fp32 weights): rel-L2 {r:.3e} with features, {r0:.3e} without")
    assert r < 4e-3 and r <= 1.1 * r0, (r, r0)
    net16 = net.half()
    out16 = net16(x.half().to(DEV), t, context=ctx.half().to(DEV), features_adapter=feats)
    plain16 = net16(x.half().to(DEV), t, context=ctx.half().to(DEV))
    r16, r160 = rel_l2(out16.float().cpu(), torch.from_numpy(gold["unet_eps"])), rel_l2(plain16.float().cpu(), torch.from_numpy(_gold("lvdm_16f.npz")["unet_eps"]))
    print(f"released UNet forward (fp16 weights): rel-L2 {r16:.3e} with features, {r160:.3e} without")
    assert out16.dtype == torch.float16 and r16 < 8e-3 and r16 <= 1.1 * r160, (r16, r160)
