"""CPU: VideoCrafter depth adapter ("VideoControl") — parameter tree, the independent torch restatement against the live reference
and the committed goldens (tests/golden/make_golden_adapter.py), the adapter program and the UNet program with injection sites in
the CPU interpreter, the conditions on the program's size, and the host logic of features_adapter."""
import ctypes
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import adapter_ref as AR
from harness import rel_l2
from interp_adapter import AdapterInterp
from oracle import configs, synth
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import samplers, videocrafter as VC
from test_samplers_cpu import _ddim_update_cpu, _lincomb_cpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SEED_ADAPTER = 11


def _gold(name):
    return np.load(os.path.join(GOLD, name))


from oracle import ref_bootstrap as rb  # noqa: E402

needs_reference = pytest.mark.skipif(not rb.reference_available(), reason="the reference checkout is not on this machine")


def _reference_adapter():
    """The reference's own adapter module (callers carry `needs_reference`; anything that goes wrong in here is a failure)."""
    rb.bootstrap()
    return importlib.import_module("videocrafter.lvdm.models.modules.adapter")


def _inputs_tiny():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    x_T = torch.randn(1, 4, 5, 8, 8, generator=g)
    return x, torch.tensor([801, 401]), ctx, x_T


def _small_adapter(name, **over):
    net = VC.Adapter(**AR.SMALL, **{**AR.OPTION_SETS[name], **over})
    sd = synth.synth_state_dict(synth.param_spec(net), seed=SEED_ADAPTER)
    net.load_state_dict(sd, strict=True)
    return net, sd


@pytest.fixture(scope="module")
def tiny():
    net = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    sd = synth.synth_state_dict(synth.param_spec(net), seed=0)
    net.load_state_dict(sd, strict=True)
    return net, sd


# ---- parameter tree ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AR.OPTION_SETS))
def test_state_dict_keys_match_reference(name):
    gold = _gold("lvdm_adapter_small.npz")
    sd = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS[name]).state_dict()
    assert list(sd.keys()) == gold[f"{name}_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == gold[f"{name}_shapes"].tolist()
    rel = VC.Adapter(channels=AR.RELEASED["channels"], cin=64, **AR.OPTION_SETS[name], init_weights=False)
    sd = rel.state_dict()
    assert list(sd.keys()) == gold[f"{name}_released_keys"].tolist()
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == gold[f"{name}_released_shapes"].tolist()
    assert sum(p.numel() for p in rel.parameters()) == int(gold[f"{name}_released_params"])


def test_released_shapes_have_the_documented_sizes():
    gold = _gold("lvdm_adapter_small.npz")
    assert [(len(gold[f"{n}_released_keys"]), int(gold[f"{n}_released_params"]) // 10 ** 6) for n in ("t2i", "full", "conv")] == \
        [(38, 77), (60, 233), (44, 96)]


@needs_reference
def test_reference_state_dict_loads_strict():
    ad = _reference_adapter()
    for name, opts in AR.OPTION_SETS.items():
        ref = ad.Adapter(**AR.SMALL, **opts)
        VC.Adapter(**AR.SMALL, **opts, init_weights=False).load_state_dict(ref.state_dict(), strict=True)


def test_configuration_the_reference_cannot_run_raises():
    with pytest.raises(NotImplementedError, match="the reference fails too"):
        VC.Adapter(channels=[32, 64], nums_rb=2, cin=64, ksize=1, sk=False, use_conv=True)
    with pytest.raises(NotImplementedError, match="the reference fails too"):
        VC.Adapter()                                         # the constructor defaults: sk=False on [320, 640, 1280, 1280]
    VC.Adapter(channels=[32, 32], nums_rb=1, cin=64, ksize=1, sk=False, use_conv=True)      # every in_c == out_c: runs in the reference
    with pytest.raises(NotImplementedError):
        VC.Adapter(channels=[32], cin=192, sk=True)
    with pytest.raises(L.T2VError):                          # no CPU fallback
        VC.Adapter(**AR.SMALL, **AR.OPTION_SETS["t2i"])(torch.zeros(1, 1, 64, 48))


# ---- the independent restatement ----------------------------------------------------------------------------------------------------
@needs_reference
def test_adapter_ref_matches_live_reference():
    ad = _reference_adapter()
    depth = AR.normalise_depth(AR.small_depth())
    cases = [dict(AR.SMALL, **o) for o in AR.OPTION_SETS.values()] + [dict(channels=[32, 32], cin=64, nums_rb=2, ksize=3, sk=False, use_conv=False)]
    for kw in cases:
        ref = ad.Adapter(**kw).eval()
        sd = synth.load_synth(ref, seed=SEED_ADAPTER)
        with torch.no_grad():
            want = ref(depth)
        got = AR.adapter_forward(sd, depth, **{k: v for k, v in kw.items() if k != "cin"})
        assert len(want) == len(got)
        for a, b in zip(got, want):
            assert a.shape == b.shape and (a - b).abs().max() < 2e-5, kw


@pytest.mark.parametrize("name", list(AR.OPTION_SETS))
def test_adapter_ref_matches_golden(name):
    gold = _gold("lvdm_adapter_small.npz")
    depth = AR.small_depth()
    assert np.array_equal(depth.numpy(), gold["depth"])
    norm = AR.normalise_depth(depth)
    assert np.array_equal(norm.numpy(), gold["depth_norm"]) and bool((norm[2] == -1).all())
    _, sd = _small_adapter(name)
    feats = AR.adapter_forward(sd, norm, channels=AR.SMALL["channels"], **AR.OPTION_SETS[name])
    for k, f in enumerate(feats):
        assert np.abs(f.numpy() - gold[f"{name}_feat{k}"]).max() < 2e-5


def test_unet_ref_with_features_matches_golden(tiny):
    net, sd = tiny
    gold = _gold("lvdm_adapter_tiny.npz")
    x, t, ctx, _ = _inputs_tiny()
    feat = AR.tiny_feature()
    assert np.array_equal(feat.numpy(), gold["feature"])
    eps = AR.lvdm_unet_forward_features(sd, configs.TINY_LVDM_UNET, x, t, ctx, [feat])
    assert np.abs(eps.numpy() - gold["unet_eps"]).max() < 2e-5
    pair = AR.lvdm_unet_forward_features(sd, configs.TINY_LVDM_UNET, torch.cat([x[0:1]] * 2), torch.tensor([801, 801]), ctx, [feat[0:1]])
    assert np.abs(pair.numpy() - gold["unet_eps_pair"]).max() < 2e-5
    # and the feature matters: the golden without it is a different tensor
    assert rel_l2(eps, torch.from_numpy(_gold("lvdm_tiny.npz")["unet_eps"])) > 0.05


@needs_reference
def test_small_goldens_regenerate_exactly(tmp_path, monkeypatch):
    ad = _reference_adapter()
    sys.path.insert(0, GOLD)
    try:
        mg = importlib.import_module("make_golden_adapter")
    finally:
        sys.path.remove(GOLD)
    monkeypatch.setattr(mg, "OUT", str(tmp_path))
    _, om, vu, dd = mg.modules()
    mg.small(ad)
    mg.tiny(om, vu, dd)
    for name in ("lvdm_adapter_small.npz", "lvdm_adapter_tiny.npz"):
        new, old = np.load(os.path.join(str(tmp_path), name)), _gold(name)
        assert sorted(new.files) == sorted(old.files)
        for k in old.files:
            assert np.array_equal(new[k], old[k]), (name, k)


# ---- the adapter program in the interpreter -------------------------------------------------------------------------------------------
def _run_adapter(net, x, normalise, front_only=False):
    n, _, H, W = x.shape
    comp = net._compile(n, H, W, "f32", normalise, front_only)
    packed = comp.packer.materialise(net.state_dict(), "cpu")
    if front_only:
        outs = [torch.full((n * (H // 8) * (W // 8), 64), float("nan"), dtype=torch.float16)]
    else:
        outs = [torch.full((n * h * w, VC._pad64(c)), float("nan")) for c, h, w in net.feature_shapes(H, W)]
    ext = {L.EXT_X: x, **{L.EXT_ADAPTER + k: o for k, o in enumerate(outs)}}
    AdapterInterp(comp.prog, packed).run(ext)
    return comp, outs


@pytest.mark.parametrize("name", list(AR.OPTION_SETS))
def test_adapter_program_matches_golden_in_interpreter(name):
    gold = _gold("lvdm_adapter_small.npz")
    net, _ = _small_adapter(name)
    comp, outs = _run_adapter(net, AR.small_depth(), True)          # raw depth in, normalisation inside the front-end op
    shapes = net.feature_shapes(64, 48)
    assert [s[1:] for s in shapes] == [gold[f"{name}_feat{k}"].shape[2:] for k in range(3)]
    for k, (o, (c, h, w)) in enumerate(zip(outs, shapes)):
        assert torch.isfinite(o).all()
        assert bool((o[:, c:] == 0).all())                           # padding channels stay zero
        f = o.view(5, h, w, -1)[..., :c].permute(0, 3, 1, 2)
        r = rel_l2(f, torch.from_numpy(gold[f"{name}_feat{k}"]))
        print(f"adapter[{name}] feature {k}: rel-L2 {r:.3e} (interpreter)")
        assert r < 4e-3, (name, k, r)
    kinds = [op.kind for op in comp.prog.ops]
    assert kinds[0] == L.OP_DEPTH_TOKENS and kinds.count(L.OP_DEPTH_TOKENS) == 1
    assert kinds.count(L.OP_AVGPOOL2) == (0 if AR.OPTION_SETS[name]["use_conv"] else 2)
    relu = [op for op in comp.prog.ops if op.kind == L.OP_GEMM and op.i[18] == L.ACT_RELU]
    assert len(relu) == 3 * AR.OPTION_SETS[name]["nums_rb"] and all(op.name.endswith(".block1") for op in relu)


def test_sk_false_program_matches_restatement_in_interpreter():
    net = VC.Adapter(channels=[64, 64], nums_rb=1, cin=64, ksize=3, sk=False, use_conv=False)
    sd = synth.synth_state_dict(synth.param_spec(net), seed=3)
    net.load_state_dict(sd, strict=True)
    x = AR.normalise_depth(AR.small_depth())
    _, outs = _run_adapter(net, x, False)
    want = AR.adapter_forward(sd, x, channels=[64, 64], nums_rb=1, ksize=3, sk=False, use_conv=False)
    for o, f, (c, h, w) in zip(outs, want, net.feature_shapes(64, 48)):
        assert rel_l2(o.view(5, h, w, c).permute(0, 3, 1, 2), f) < 4e-3


def test_front_end_normalises_a_constant_frame_to_minus_one():
    net, _ = _small_adapter("t2i")
    depth = AR.small_depth()
    _, (tok,) = _run_adapter(net, depth, True, front_only=True)
    back = tok.view(5, 8, 6, 8, 8).permute(0, 1, 3, 2, 4).reshape(5, 1, 64, 48).float()
    assert bool((back[2] == -1).all())
    want = AR.normalise_depth(depth)
    assert torch.equal(back, want.half().float()) and float(back.min()) == -1.0 and float(back.max()) <= 1.0
    bad = depth.clone()
    bad[1, 0, 5, 7] = float("nan")                                   # torch.amin / amax propagate a NaN: the whole frame becomes NaN, no other
    _, (tok_nan,) = _run_adapter(net, bad, True, front_only=True)
    per_frame = tok_nan.view(5, -1)
    assert bool(torch.isnan(per_frame[1]).all()) and torch.equal(per_frame[[0, 2, 3, 4]], tok.view(5, -1)[[0, 2, 3, 4]])
    _, (raw,) = _run_adapter(net, depth, False, front_only=True)     # flag off: the values pass through
    assert torch.equal(raw.view(5, 8, 6, 8, 8).permute(0, 1, 3, 2, 4).reshape(5, 1, 64, 48), depth.half())


# ---- the UNet program with injection sites ---------------------------------------------------------------------------------------------
def _run_unet(net, comp, x, t, ctx, toks, B):
    packed = comp.packer.materialise(net.state_dict(), "cpu")
    out = torch.empty(B, 4, *x.shape[2:])
    ext = {L.EXT_X: x, L.EXT_T: t.float(), L.EXT_CTX: ctx, L.EXT_OUT: out, **{L.EXT_ADAPTER + k: v for k, v in enumerate(toks)}}
    AdapterInterp(comp.prog, packed).run(ext)
    return out


def test_unet_program_with_features_matches_golden_in_interpreter(tiny):
    net, _ = tiny
    gold = _gold("lvdm_adapter_tiny.npz")
    x, t, ctx, _ = _inputs_tiny()
    feat = AR.tiny_feature()
    toks = net._adapter_tokens([feat], x)
    assert toks[0].shape == (2 * 5 * 16, 320)
    comp = net._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", adapter=2)
    out = _run_unet(net, comp, x, t, ctx, toks, 2)
    r = rel_l2(out, torch.from_numpy(gold["unet_eps"]))
    print(f"tiny UNet with a feature: rel-L2 {r:.3e} (interpreter)")
    assert r < 4e-3
    # the [cond | uncond] batch on one x_t: both roles read the same feature rows — with and without the shared prefix
    t1 = torch.tensor([801, 801])
    for share in (False, True):
        net._share_now = share
        try:
            comp = net._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", x_batch=1, adapter=1)
        finally:
            net._share_now = False
        wrap = [op for op in comp.prog.ops if op.kind == L.OP_GEMM and op.i[30]]
        assert len(wrap) == 1 and wrap[0].i[30] == 5 * 16 and wrap[0].i[0] == 2 * 5 * 16
        pair = _run_unet(net, comp, x[0:1].contiguous(), t1, ctx, net._adapter_tokens([feat[0:1]], x[0:1]), 2)
        assert rel_l2(pair, torch.from_numpy(gold["unet_eps_pair"])) < 4e-3, share


def test_sites_that_end_in_a_transformer_add_the_feature_before_the_last_gemm():
    """Two ResBlocks per level (the released topology at two levels): the sites are blocks 2 and 5, ResBlock + transformer."""
    cfg = dict(configs.TINY_LVDM_UNET, num_res_blocks=2)
    net = VC.UNetModel(**cfg, init_weights=False)
    sd = synth.synth_state_dict(synth.param_spec(net), seed=0)
    net.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 4, 3, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    assert net.adapter_sites(8, 8) == [(320, 8, 8), (640, 4, 4)]
    feats = [torch.randn(1, 320, 3, 8, 8, generator=g) * 0.5, torch.randn(1, 640, 3, 4, 4, generator=g) * 0.5]
    t = torch.tensor([500, 500])
    want = AR.lvdm_unet_forward_features(sd, cfg, torch.cat([x, x]), t, ctx, feats)
    comp = net._compile(2, 3, 8, 8, 9, "f32", "f32", "f32", x_batch=1, adapter=1)
    base = net._compile(2, 3, 8, 8, 9, "f32", "f32", "f32", x_batch=1, adapter=0)
    assert len(comp.prog.ops) == len(base.prog.ops) + 2
    got = _run_unet(net, comp, x, t, ctx, net._adapter_tokens(feats, x), 2)
    assert rel_l2(got, want) < 4e-3
    assert rel_l2(got, AR.lvdm_unet_forward_features(sd, cfg, torch.cat([x, x]), t, ctx, None)) > 0.02


def test_program_without_features_is_unchanged_and_released_program_grows_by_at_most_one_launch_per_site(tiny):
    net, _ = tiny
    default = net._compile(2, 5, 8, 8, 9, "f32", "f32", "f32")                       # what forward(features_adapter=None) compiles
    low = VC._LvdmLowering(net, 2, 5, 8, 8, 9, "f32", "f32", "f32", adapter=0)      # the sites disabled
    disabled = low.build()
    sig = lambda prog: [(op.kind, op.name, tuple(op.i), tuple(op.f)) for op in prog.ops]
    assert sig(default.prog) == sig(disabled) and len(default.prog.ops) == len(disabled.ops)
    with_feat = net._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", adapter=2)
    assert [op.kind for op in with_feat.prog.ops] == [op.kind for op in disabled.ops]   # a convolution's residual: no launch at all
    # the released UNet: 4 sites, each at most one launch more
    rel = VC.UNetModel(**configs.LVDM_UNET, init_weights=False)
    assert rel.adapter_sites(32, 32) == [(320, 32, 32), (640, 16, 16), (1280, 8, 8), (1280, 4, 4)]
    for kw in (dict(B=2, x_batch=1), dict(B=1, x_batch=0)):
        a = rel._compile(kw["B"], 16, 32, 32, 77, "f16", "f32", "f16", x_batch=kw["x_batch"], adapter=0).prog
        b = rel._compile(kw["B"], 16, 32, 32, 77, "f16", "f32", "f16", x_batch=kw["x_batch"], adapter=1).prog
        extra = len(b.ops) - len(a.ops)
        print(f"released UNet B={kw['B']}: {len(a.ops)} launches without features, {len(b.ops)} with")
        assert 0 <= extra <= 4
        added = [op for op in b.ops if op.name.endswith(".adapter")]
        assert len(added) == extra and all(op.kind == L.OP_RESHARD_ROWS for op in added)
        rest = [op.kind for op in b.ops if not op.name.endswith(".adapter")]
        assert rest == [op.kind for op in a.ops]


# ---- host logic ----------------------------------------------------------------------------------------------------------------------
def test_feature_list_errors_and_single_conversion(tiny):
    net, _ = tiny
    x = torch.zeros(1, 4, 5, 8, 8)
    f = torch.randn(1, 320, 5, 4, 4)
    with pytest.raises(AssertionError, match="Mismatch features adapter"):
        net._adapter_tokens([f, f], x)
    with pytest.raises(AssertionError, match="Mismatch features adapter"):
        net._adapter_tokens([], x)
    for bad in (torch.randn(1, 320, 5, 8, 8), torch.randn(2, 320, 5, 4, 4), torch.randn(1, 640, 5, 4, 4), torch.randn(1, 320, 4, 4, 4)):
        with pytest.raises(ValueError, match="expected shape"):
            net._adapter_tokens([bad], x)
    with pytest.raises(ValueError):
        net._adapter_tokens([f.double()], x)
    net.adapter_conversions = 0
    feats = [f]
    a = net._adapter_tokens(feats, x)
    for _ in range(5):                                   # the steps of a sampling loop: the same list object
        assert net._adapter_tokens(feats, x) is a
    assert net.adapter_conversions == 1
    assert torch.equal(a[0].view(1, 5, 4, 4, 320).permute(0, 4, 1, 2, 3), f)
    f.mul_(0.5)                                          # an in-place change is a new version: converted again
    net._adapter_tokens(feats, x)
    scaled = [0.8 * v for v in feats]                    # ... and so is the caller's own scaling
    net._adapter_tokens(scaled, x)
    assert net.adapter_conversions == 3
    # channels-last storage (what Adapter / get_adapter_features return) is taken as it is: no copy
    store = torch.randn(1, 5, 4, 4, 320)
    view = store.permute(0, 4, 1, 2, 3)
    assert net._adapter_tokens([view], x)[0].data_ptr() == store.data_ptr()
    # the same list against an x of another geometry is checked again, cached or not
    net._adapter_tokens(feats, x)
    for other in (torch.zeros(2, 4, 5, 8, 8), torch.zeros(1, 4, 6, 8, 8), torch.zeros(1, 4, 5, 16, 16)):
        with pytest.raises(ValueError, match="expected shape"):
            net._adapter_tokens(feats, other)
    with pytest.raises(NotImplementedError):
        net(x, torch.tensor([1]), context=torch.zeros(1, 9, 768), features_adapter=[f], y=torch.zeros(1))
    with pytest.raises(NotImplementedError):
        net(x, torch.tensor([1]), context=torch.zeros(1, 9, 768), time_emb_replace=torch.zeros(1, 1280))


def test_t_sharded_forward_with_features_is_refused(tiny):
    net, _ = tiny
    net.t_shard = types.SimpleNamespace(size=2)
    try:
        with pytest.raises(L.T2VError, match="T-sharded"):
            net(torch.zeros(1, 4, 5, 8, 8), torch.tensor([1]), context=torch.zeros(1, 9, 768), features_adapter=[torch.zeros(1, 320, 5, 4, 4)])
    finally:
        net.t_shard = None


def test_ddim_sampler_passes_the_features_through(tiny, monkeypatch):
    net, sd = tiny
    monkeypatch.setattr(samplers, "_lincomb", _lincomb_cpu)
    monkeypatch.setattr(samplers, "_ddim_update", _ddim_update_cpu)
    gold = _gold("lvdm_adapter_tiny.npz")
    _, _, ctx, x_T = _inputs_tiny()
    feats = [AR.tiny_feature()[0:1]]
    ld = VC.LatentDiffusion.__new__(VC.LatentDiffusion)
    torch.nn.Module.__init__(ld)
    VC.LatentDiffusion.register_schedule(ld, **configs.LVDM_SCHEDULE)
    seen = []

    def apply_model(x, t, c, **kw):
        seen.append(kw.get("features_adapter"))
        return AR.lvdm_unet_forward_features(sd, configs.TINY_LVDM_UNET, x, t, c, kw.get("features_adapter"))
    ld.apply_model = apply_model
    ld.model = types.SimpleNamespace(diffusion_model=types.SimpleNamespace(refresh_weights=lambda d: None, auto_refresh=True))
    smp = VC.DDIMSampler(ld)
    smp.noise_gen.manual_seed(123)
    kw = dict(S=4, conditioning={"c_crossattn": [ctx[0:1]]}, batch_size=1, shape=list(x_T.shape[1:]), verbose=False,
              unconditional_guidance_scale=7.5, unconditional_conditioning={"c_crossattn": [ctx[1:2]]}, eta=0.3, x_T=x_T)
    x0, _ = smp.sample(**kw, features_adapter=feats, temporal_length=5, conditional_guidance_scale_temporal=None)
    assert len(seen) == 4 and all(s is feats for s in seen)            # the same list object at every step
    assert np.abs(x0.numpy() - gold["ddim_x0"]).max() < 2e-4 * np.abs(gold["ddim_x0"]).max()
    with pytest.raises(NotImplementedError, match="conditional_guidance_scale_temporal"):
        smp.sample(**kw, features_adapter=feats, conditional_guidance_scale_temporal=1.5)
    seen.clear()
    smp.sample(**kw)                                                   # without the keyword apply_model sees no such argument
    assert seen == [None] * 4


def test_depth_must_arrive_at_target_size():
    ld = VC.T2VAdapterDepth.__new__(VC.T2VAdapterDepth)
    torch.nn.Module.__init__(ld)
    ld.adapter = VC.Adapter(**AR.SMALL, **AR.OPTION_SETS["t2i"])
    ld.depth_stage_model = lambda frames: torch.zeros(frames.shape[0], 1, 48, 48)
    videos = torch.zeros(1, 3, 2, 64, 48)
    with pytest.raises(ValueError, match="must arrive at target_size"):
        ld.get_batch_depth(videos, (64, 48))
    ld.depth_stage_model = None
    with pytest.raises(RuntimeError, match="depth_stage_model"):
        ld.get_batch_depth(videos, (64, 48))
    with pytest.raises(ValueError):
        ld.get_batch_depth(depth=torch.zeros(1, 2, 64, 48))


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_validation_of_abi11_records_without_gpu(built_lib):
    h = ctypes.c_void_p()
    ptr = 0x1000

    def create(kind, i=(), p=()):
        op = (L.T2VOp * 1)()
        op[0].kind = kind
        for k, v in (i.items() if isinstance(i, dict) else enumerate(i)):
            op[0].i[k] = v
        for k, v in enumerate(p):
            op[0].p[k] = v
        rc = built_lib.t2v_plan_create(op, 1, ctypes.byref(h))
        if rc == 0:
            built_lib.t2v_plan_destroy(h)
        return rc, built_lib.t2v_last_error()

    assert L.ABI_VERSION == 11 and built_lib.t2v_abi_version() == 11
    assert create(L.OP_DEPTH_TOKENS, (5, 64, 48, L.F32, 1, 64), (ptr, ptr))[0] == 0
    for bad in ((5, 60, 48, L.F32, 1, 64), (5, 64, 48, L.F32, 2, 64), (5, 64, 48, L.F32, 1, 32), (0, 64, 48, L.F32, 1, 64)):
        rc, msg = create(L.OP_DEPTH_TOKENS, bad, (ptr, ptr))
        assert rc == -1 and b"depth tokens" in msg, bad
    assert create(L.OP_AVGPOOL2, (5, 8, 6, 64, 64, 64, 64), (ptr, ptr, ptr))[0] == 0
    assert create(L.OP_AVGPOOL2, (5, 8, 6, 64, 64, 0, 64), (ptr, 0, ptr))[0] == 0
    for bad, pp in (((5, 8, 6, 66, 68, 68, 68), (ptr, ptr, ptr)), ((5, 8, 6, 64, 64, 64, 64), (ptr, 0, 0)), ((5, 1, 6, 64, 64, 64, 64), (ptr, ptr, 0)),
                    ((5, 8, 6, 64, 32, 64, 64), (ptr, ptr, 0))):
        rc, msg = create(L.OP_AVGPOOL2, bad, pp)
        assert rc == -1 and b"average pooling" in msg, bad
    gemm = {0: 256, 1: 64, 2: 64, 3: 64, 4: 64, 5: 64, 17: L.F16}
    assert create(L.OP_GEMM, {**gemm, 18: L.ACT_RELU}, (ptr, ptr, 0, 0, 0, ptr))[0] == 0
    rc, msg = create(L.OP_GEMM, {**gemm, 18: 3}, (ptr, ptr, 0, 0, 0, ptr))
    assert rc == -1 and b"activation" in msg
    conv = {0: 256, 1: 64, 2: 576, 3: 64, 4: 576, 5: 64, 6: 64, 7: L.GATHER_CONV3X3, 8: 16, 9: 16, 10: 64, 11: 1, 13: 16, 14: 16, 17: L.F32}
    assert create(L.OP_GEMM, {**conv, 30: 128}, (ptr, ptr, 0, 0, ptr, ptr))[0] == 0
    for bad, pp in (({**conv, 30: 64}, (ptr, ptr, 0, 0, ptr, ptr)), ({**conv, 30: 128}, (ptr, ptr, 0, 0, 0, ptr))):
        rc, msg = create(L.OP_GEMM, bad, pp)
        assert rc == -1 and b"residual row wrap" in msg


def test_every_record_of_the_new_programs_passes_the_library_validation(built_lib, tiny):
    """t2v_plan_create validates every record before any HIP call: the adapter programs (small and released shapes, front end alone) and
    the UNet programs with injection sites are well-formed for the executor — checked here without a GPU, on made-up addresses."""
    from sd_webui_text2video_amd.program import BoundProgram
    progs = []
    for name in AR.OPTION_SETS:
        net, _ = _small_adapter(name)
        progs += [net._compile(5, 64, 48, "f32", True), net._compile(5, 64, 48, "f16", False, front_only=True)]
        rel = VC.Adapter(channels=AR.RELEASED["channels"], cin=64, **AR.OPTION_SETS[name], init_weights=False)
        progs.append(rel._compile(16, 256, 256, "f32", True))
    unet, _ = tiny
    progs += [unet._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", adapter=2), unet._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", x_batch=1, adapter=1)]
    progs.append(VC.UNetModel(**configs.LVDM_UNET, init_weights=False)._compile(2, 16, 32, 32, 77, "f16", "f32", "f16", x_batch=1, adapter=1))
    for comp in progs:
        fake = {n: 0x40000000 + 0x1000000 * k for k, (n, _, _) in enumerate(comp.packer.recipes)}
        bound = BoundProgram(comp.prog, 0x10000000, fake, reset_sync=False)
        assert built_lib.t2v_plan_num_ops(bound.handle) == len(comp.prog.ops)


def test_released_adapter_program_matches_golden_samples_in_interpreter():
    """Case 4's adapter half on the CPU: the 77 M-parameter shape on the seeded 16-frame 256 x 256 depth clip, one program of 33 launches."""
    gold = _gold("lvdm_adapter_16f.npz")
    ad = VC.Adapter(**AR.RELEASED, init_weights=False)
    ad.load_state_dict(synth.synth_state_dict(synth.param_spec(ad), seed=SEED_ADAPTER), strict=True)
    comp, outs = _run_adapter(ad, AR.released_depth()[0].permute(1, 0, 2, 3).contiguous(), True)
    shapes = ad.feature_shapes(256, 256)
    assert shapes == [(320, 32, 32), (640, 16, 16), (1280, 8, 8), (1280, 4, 4)] and len(comp.prog.ops) == 33
    for k, (o, (c, h, w)) in enumerate(zip(outs, shapes)):
        r = rel_l2(AR.subsample(o.view(16, h, w, c).permute(0, 3, 1, 2)), torch.from_numpy(gold[f"feat{k}"]))
        print(f"adapter[released] feature {k}: rel-L2 {r:.3e} (interpreter)")
        assert r < 4e-3, (k, r)
