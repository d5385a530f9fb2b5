"""CPU: the VideoCrafter LoRA loaders (videocrafter.net_load_lora / change_lora / net_load_lora_v2 / change_lora_v2) against the golden
of the REAL reference's loaders (tests/golden/make_golden_lora.py -> lvdm_lora_tiny.npz: the LoRA file's keys and factors, SHA-256 of
every touched weight after each step, the reference UNet's eps on the merged weights).  On CPU parameters the expression and the torch
op are the reference's, so the bytes must be equal."""
import hashlib
import os

import numpy as np
import pytest
import torch
from torch import nn

from harness import rel_l2
from interp import Interp
from oracle import configs, synth, torch_port as tp
from sd_webui_text2video_amd import _lib as L
from sd_webui_text2video_amd import videocrafter as VC

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "lvdm_lora_tiny.npz"))
ALPHA = float(GOLD["alpha"])
TOUCHED = [str(n) for n in GOLD["touched"]]
PREFIX = "model.diffusion_model."


def lora_state_dict():
    return {str(k): torch.from_numpy(GOLD[f"f{i}"].copy()) for i, k in enumerate(GOLD["keys"])}


def inputs_tiny():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    return x, torch.tensor([801, 401]), ctx


def make_ld():
    ld = VC.LatentDiffusion(configs.TINY_LVDM_UNET, image_size=[8, 8], video_length=5, init_weights=False, **configs.LVDM_SCHEDULE)
    net = ld.model.diffusion_model
    net.load_state_dict(synth.synth_state_dict(synth.param_spec(net), seed=0), strict=True)
    return ld, net


def digests(net):
    mods = dict(net.named_modules())
    return [hashlib.sha256(mods[n].weight.detach().contiguous().numpy().tobytes()).hexdigest() for n in TOUCHED]


@pytest.fixture(scope="module")
def lora_path(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lora") / "style.ckpt")
    torch.save(lora_state_dict(), path)
    return path


def test_golden_is_strong_enough_to_matter():
    assert float(GOLD["separation_over_gate"]) >= 100 and len(TOUCHED) == 40
    kinds = ("attn1.", "attn2.", "attn1_tmp.", "attn2_tmp.", "ff.net", "emb_layers.1", "time_embed")
    assert all(any(k in n for n in TOUCHED) for k in kinds)


def test_load_remove_and_v2_round_trip_are_bit_equal_to_the_reference(lora_path, capsys):
    ld, net = make_ld()
    versions = {n: dict(net.named_modules())[n].weight._version for n in TOUCHED}
    assert digests(net) == GOLD["sha_original"].tolist()
    assert VC.net_load_lora(ld, lora_path, alpha=ALPHA) is None
    out = capsys.readouterr().out.splitlines()
    conv3d = PREFIX + str(GOLD["conv3d"])
    assert out == [f"missing param at: {conv3d}.lora_down.weight", f"missing param at: {conv3d}.lora_up.weight", "load_weight_num: 80"]
    assert digests(net) == GOLD["sha_merged"].tolist()
    assert all(dict(net.named_modules())[n].weight._version > v for n, v in versions.items())       # in-place ops, not `.data`
    untouched = {k: v for k, v in synth.synth_state_dict(synth.param_spec(net), seed=0).items() if k[:-len(".weight")] not in TOUCHED}
    assert all(torch.equal(net.state_dict()[k], v) for k, v in untouched.items())                     # the Conv3d target included
    VC.net_load_lora(ld, lora_path, alpha=ALPHA, remove=True)
    assert digests(net) == GOLD["sha_removed"].tolist() != GOLD["sha_original"].tolist()            # v1 leaves its rounding residue

    ld, net = make_ld()
    origin = VC.net_load_lora_v2(ld, lora_path, alpha=ALPHA)
    assert digests(net) == GOLD["sha_v2_loaded"].tolist()
    assert sorted(origin) == sorted(PREFIX + n + ".lora.weight" for n in TOUCHED)                    # the reference's storage_key
    back = VC.net_load_lora_v2(ld, lora_path, alpha=ALPHA, remove=True, origin_weight=origin)
    assert back is origin and digests(net) == GOLD["sha_v2_removed"].tolist() == GOLD["sha_original"].tolist()
    assert "load_weight_num: 80" in capsys.readouterr().out


def test_change_lora_and_change_lora_v2(lora_path):
    ld, net = make_ld()
    assert VC.change_lora(ld, inject_lora=True, lora_scale=ALPHA, lora_path=lora_path) is None
    assert digests(net) == GOLD["sha_merged"].tolist()
    VC.change_lora(ld, inject_lora=False, last_time_lora=lora_path, last_time_lora_scale=ALPHA)
    assert digests(net) == GOLD["sha_removed"].tolist()
    ld, net = make_ld()
    origin = VC.change_lora_v2(ld, inject_lora=True, lora_scale=ALPHA, lora_path=lora_path)
    assert digests(net) == GOLD["sha_v2_loaded"].tolist()
    # a new scale: the previous one is restored from the snapshot first, then the file is merged at the new scale
    origin = VC.change_lora_v2(ld, inject_lora=True, lora_scale=0.3, lora_path=lora_path, last_time_lora=lora_path, last_time_lora_scale=ALPHA,
                               origin_weight=origin)
    other, net2 = make_ld()
    VC.net_load_lora(other, lora_path, alpha=0.3)
    assert digests(net) == digests(net2)
    origin = VC.change_lora_v2(ld, inject_lora=False, last_time_lora=lora_path, last_time_lora_scale=0.3, origin_weight=origin)
    assert digests(net) == GOLD["sha_original"].tolist()
    assert VC.change_lora_v2(ld) is None                                                             # nothing to do: the dict is handed through


def test_alpha_entries_are_never_read_and_the_key_order_does_not_matter(tmp_path):
    sd = lora_state_dict()
    swapped = {}
    for k, v in reversed(list(sd.items())):                      # every pair now meets its OTHER key first
        swapped[k] = torch.full_like(v, 123.0) if ".alpha" in k else v
    path = str(tmp_path / "swapped.ckpt")
    torch.save(swapped, path)
    ld, net = make_ld()
    VC.net_load_lora(ld, path, alpha=ALPHA)
    assert digests(net) == GOLD["sha_merged"].tolist()


def test_an_unresolvable_key_raises_and_leaves_every_parameter_unchanged(tmp_path):
    sd = lora_state_dict()
    bad = "cond_stage_model.transformer.text_model.encoder.layers.0.self_attn.q_proj"
    sd[bad + ".lora_down.weight"], sd[bad + ".lora_up.weight"] = torch.zeros(4, 8), torch.zeros(8, 4)      # LAST: the reference would die half-merged
    path = str(tmp_path / "bad.ckpt")
    torch.save(sd, path)
    for attach in (None, object()):
        ld, net = make_ld()
        ld.cond_stage_model = attach
        before = {k: v.clone() for k, v in ld.state_dict().items()}
        for fn in (VC.net_load_lora, VC.net_load_lora_v2):
            with pytest.raises(L.T2VError, match="cond_stage_model"):
                fn(ld, path, alpha=ALPHA)
        assert all(torch.equal(v, before[k]) for k, v in ld.state_dict().items())
    # a pair without its partner, and factors that do not fit the weight
    for mutate in (lambda d: d.pop(PREFIX + TOUCHED[-1] + ".lora_up.weight"),
                   lambda d: d.__setitem__(PREFIX + TOUCHED[-1] + ".lora_up.weight", torch.zeros(7, 4))):
        sd = lora_state_dict()
        mutate(sd)
        torch.save(sd, path)
        ld, net = make_ld()
        with pytest.raises(L.T2VError, match=TOUCHED[-1].replace(".", r"\.")):
            VC.net_load_lora(ld, path)
        assert digests(net) == GOLD["sha_original"].tolist()


def test_only_exact_linear_and_conv2d_classes_are_touched(tmp_path, capsys):
    class MyLinear(nn.Linear):
        pass

    class H(nn.Module):
        device = torch.device("cpu")

    h = H()
    h.seq = nn.Sequential(nn.Linear(8, 6), MyLinear(8, 6))
    before = [m.weight.detach().clone() for m in h.seq]
    sd = {}
    for k in (0, 1):
        sd[f"seq.{k}.lora_up.weight"], sd[f"seq.{k}.lora_down.weight"] = torch.ones(6, 2), torch.ones(2, 8)
    path = str(tmp_path / "cls.ckpt")
    torch.save(sd, path)
    VC.net_load_lora(h, path, alpha=0.5)
    assert torch.equal(h.seq[0].weight, before[0] + 0.5 * 2.0) and torch.equal(h.seq[1].weight, before[1])
    assert capsys.readouterr().out.count("missing param at: seq.1.") == 2


def test_an_fp16_model_rounds_like_the_reference_in_place_add(lora_path):
    ld, net = make_ld()
    ld = ld.half()
    sd = lora_state_dict()
    mods = dict(net.named_modules())
    want = {}
    for n in TOUCHED:
        w = mods[n].weight.detach().clone()
        assert w.dtype == torch.float16
        w.data += ALPHA * torch.mm(sd[PREFIX + n + ".lora_up.weight"].to(torch.float32), sd[PREFIX + n + ".lora_down.weight"].to(torch.float32))
        want[n] = w
    VC.net_load_lora(ld, lora_path, alpha=ALPHA)
    assert all(mods[n].weight.dtype == torch.float16 and torch.equal(mods[n].weight, want[n]) for n in TOUCHED)


def test_two_loras_stacked_and_removed_in_the_other_order(lora_path, tmp_path):
    g = torch.Generator().manual_seed(21)
    second = {}
    for n in TOUCHED[::3] + ["output_blocks.0.0.emb_layers.1"]:
        w = synth.synth_state_dict(synth.param_spec(make_ld()[1]), seed=0)[n + ".weight"]
        second[PREFIX + n + ".lora_up.weight"] = torch.randn(w.shape[0], 2, generator=g) * 0.1
        second[PREFIX + n + ".lora_down.weight"] = torch.randn(2, w.shape[1], generator=g) * 0.1
    path2 = str(tmp_path / "second.ckpt")
    torch.save(second, path2)
    ld, net = make_ld()
    orig = {k: v.clone() for k, v in net.state_dict().items()}
    VC.net_load_lora(ld, lora_path, alpha=ALPHA)
    VC.net_load_lora(ld, path2, alpha=1.3)
    VC.net_load_lora(ld, lora_path, alpha=ALPHA, remove=True)
    only_second, net2 = make_ld()
    VC.net_load_lora(only_second, path2, alpha=1.3)
    for k, v in net.state_dict().items():                      # = the second alone, up to four roundings of the largest intermediate
        assert (v - net2.state_dict()[k]).abs().max() <= 4 * 2.0 ** -24 * max(1.0, float(v.abs().max())), k
    VC.net_load_lora(ld, path2, alpha=1.3, remove=True)
    for k, v in net.state_dict().items():
        assert (v - orig[k]).abs().max() <= 4 * 2.0 ** -24 * max(1.0, float(v.abs().max())), k


def test_conv2d_targets_receive_the_delta_on_every_tap(tmp_path):
    class H(nn.Module):
        device = torch.device("cpu")

    h = H()
    h.c1, h.c3 = nn.Conv2d(8, 6, 1), nn.Conv2d(8, 6, 3, padding=1)
    sd = {}
    with torch.no_grad():
        for name in ("c1", "c3"):
            getattr(h, name).weight.copy_(torch.from_numpy(GOLD[f"conv_{name}_before"]))
            sd[f"{name}.lora_down.weight"] = torch.from_numpy(GOLD[f"conv_{name}_down"].copy())
            sd[f"{name}.lora_up.weight"] = torch.from_numpy(GOLD[f"conv_{name}_up"].copy())
    path = str(tmp_path / "conv.ckpt")
    torch.save(sd, path)
    VC.net_load_lora(h, path, alpha=ALPHA)
    for name in ("c1", "c3"):
        assert np.array_equal(getattr(h, name).weight.detach().numpy(), GOLD[f"conv_{name}_after"]), name
    d = h.c3.weight.detach() - torch.from_numpy(GOLD["conv_c3_before"])
    assert (d - d[:, :, :1, :1]).abs().max() <= 2.0 ** -22 and d.abs().max() > 1e-3      # the same delta on all nine taps


def test_merge_repacks_only_the_touched_images_and_the_program_computes_the_merged_model(lora_path):
    ld, net = make_ld()
    net.refresh_weights("cpu")
    assert net.last_repack == -1
    n_images = len(net._packed)
    ptrs = {k: v.data_ptr() for k, v in net._packed.items()}
    VC.net_load_lora(ld, lora_path, alpha=ALPHA)
    net.refresh_weights("cpu")                                  # the signature check alone: the versions moved
    assert 0 < net.last_repack < n_images // 2, (net.last_repack, n_images)
    assert {k: v.data_ptr() for k, v in net._packed.items()} == ptrs
    assert net.verify_weights("cpu") == []
    x, t, ctx = inputs_tiny()
    comp = net._compile(2, 5, 8, 8, 9, "f32", "f32", "f32")
    net._pack_missing(comp, torch.device("cpu"))
    full = comp.packer.materialise(net.state_dict(), "cpu")
    assert all(torch.equal(full[k], net._packed[k]) for k in full)
    out = torch.empty(2, 4, 5, 8, 8)
    Interp(comp.prog, net._packed).run({L.EXT_X: x, L.EXT_T: t.float(), L.EXT_CTX: ctx, L.EXT_OUT: out})
    want = tp.lvdm_unet_forward({k: v.clone() for k, v in net.state_dict().items()}, configs.TINY_LVDM_UNET, x, t, ctx)
    gold = torch.from_numpy(GOLD["eps_merged"])
    assert np.abs(want.numpy() - GOLD["eps_merged"]).max() < 2e-5 * max(1.0, float(gold.abs().max()))      # the port on merged weights = the reference
    assert rel_l2(out, want) < 4e-3 and rel_l2(out, gold) < 4e-3
