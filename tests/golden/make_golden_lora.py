"""Generate the VideoCrafter LoRA golden FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_lora.py          # lvdm_lora_tiny.npz, seconds on a CPU

The reference's own loaders (lvdm/models/modules/lora.py:620-755: net_load_lora, net_load_lora_v2), unmodified, merge a seeded LoRA
file into the reference's own UNetModel(**TINY_LVDM_UNET) with the synthetic weights of seed 0, held as `.model.diffusion_model` of a
stand-in module with `.device` (what the loaders read of LatentDiffusion).  The file: rank 4, factors ~ N(0, scale^2), an `.alpha`
entry per layer (which the loaders never read), 40 Linears covering attn1 / attn2 / attn1_tmp / attn2_tmp / ff / emb_layers.1 /
time_embed, every second pair with its lora_up key first, and one key whose target is a Conv3d (the 'missing param' branch).

Stored: the key order and the factors; the reference UNet's eps on the inputs of lvdm_tiny.npz with the merged weights (alpha 0.7);
for every touched weight the SHA-256 of its bytes after the v1 load, after the v1 removal, after a v2 load on fresh weights and after
the v2 removal.  (Digests, not the tensors: the tiny config is 320 channels wide, one touched weight is 0.4 - 3.3 MB and a committed
file is limited to 1 MiB.  The tests compare on the CPU, where the bytes must be EQUAL, so a digest says all there is to say.)
The factor scale is raised until the merged and the un-merged eps differ by at least 100 x the rel-L2 gate of
test_tiny_unet_matches_reference_golden (4e-3), and the ratio is recorded: a LoRA too weak to matter would let every parity test pass.
A Conv2d 1x1 and a 3x3 target (the reference adds the [o, i, 1, 1] delta to every tap) on a bare holder: weights before and after."""
import hashlib
import importlib
import os
import sys
import tempfile

import numpy as np
import torch
from torch import nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ALPHA, RANK, N_LINEARS, GATE = 0.7, 4, 40, 4e-3
KINDS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0",
         "attn1_tmp.to_q", "attn1_tmp.to_k", "attn1_tmp.to_v", "attn1_tmp.to_out.0", "attn2_tmp.to_q", "attn2_tmp.to_k", "attn2_tmp.to_v",
         "attn2_tmp.to_out.0", "ff.net.0.proj", "ff.net.2", "emb_layers.1", "time_embed.0", "time_embed.2")
PREFIX = "model.diffusion_model."


def inputs_tiny():
    """The inputs of lvdm_tiny.npz (tests/test_gpu_videocrafter.py:_inputs_tiny)."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 4, 5, 8, 8, generator=g)
    ctx = torch.randn(2, 9, 768, generator=g)
    return x, torch.tensor([801, 401]), ctx


class Holder(nn.Module):
    device = torch.device("cpu")


def pick_targets(net):
    """40 Linears, every kind of KINDS at least once: round-robin over the kinds in module order."""
    by_kind = {k: [n for n, m in net.named_modules() if m.__class__ is nn.Linear and n.endswith(k)] for k in KINDS}
    assert all(by_kind.values()), [k for k, v in by_kind.items() if not v]
    names, depth = [], 0
    while len(names) < N_LINEARS:
        for k in KINDS:
            if depth < len(by_kind[k]) and len(names) < N_LINEARS:
                names.append(by_kind[k][depth])
        depth += 1
    return names


def make_lora(net, names, conv3d_name, scale, seed=4):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, name in enumerate(names + [conv3d_name]):
        w = dict(net.named_modules())[name].weight
        down = torch.randn(RANK, w.shape[1], generator=g) * scale
        up = torch.randn(w.shape[0], RANK, generator=g) * scale
        base = PREFIX + name
        pair = [(base + ".lora_down.weight", down), (base + ".lora_up.weight", up)]
        for key, v in (pair[::-1] if k % 2 else pair):              # every second pair is met lora_up first
            sd[key] = v
        sd[base + ".alpha"] = torch.tensor(float(RANK) * 2)           # never read by the loaders
    return sd


def digest(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def main():
    rb.bootstrap()
    om = importlib.import_module("videocrafter.lvdm.models.modules.openaimodel3d")
    lora = importlib.import_module("videocrafter.lvdm.models.modules.lora")
    x, t, ctx = inputs_tiny()

    def fresh():
        net = om.UNetModel(**configs.TINY_LVDM_UNET).eval()
        synth.load_synth(net, seed=0)
        h = Holder()
        h.model = nn.Module()
        h.model.diffusion_model = net
        return h, net

    h, net = fresh()
    names = pick_targets(net)
    conv3d_name = next(n for n, m in net.named_modules() if m.__class__ is nn.Conv3d and n.endswith("proj_in"))
    mods = dict(net.named_modules())
    with torch.no_grad():
        eps0 = net(x, t, context=ctx)
    gold0 = np.load(os.path.join(OUT, "lvdm_tiny.npz"))["unet_eps"]
    assert np.array_equal(eps0.numpy(), gold0), "the un-merged reference forward is not lvdm_tiny.npz's"
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "lora.ckpt")
    scale = 0.05
    while True:
        h, net = fresh()
        mods = dict(net.named_modules())
        sd = make_lora(net, names, conv3d_name, scale)
        torch.save(sd, path)
        versions = [mods[n].weight._version for n in names]
        lora.net_load_lora(h, path, alpha=ALPHA)
        assert versions == [mods[n].weight._version for n in names]      # the reference's `.data +=` moves no version counter
        with torch.no_grad():
            eps = net(x, t, context=ctx)
        sep = rel_l2(eps, eps0)
        print(f"factor scale {scale:g}: merged vs un-merged eps rel-L2 {sep:.3e} = {sep / GATE:.1f} x the gate")
        if sep >= 100 * GATE:
            break
        scale *= 1.5
    out = {"keys": np.asarray(list(sd.keys())), "touched": np.asarray(names), "conv3d": np.asarray(conv3d_name),
           "alpha": np.float64(ALPHA), "scale": np.float64(scale), "separation": np.float64(sep), "separation_over_gate": np.float64(sep / GATE),
           "eps_merged": eps.numpy()}
    for k, (key, v) in enumerate(sd.items()):
        out[f"f{k}"] = v.numpy()
    out["sha_merged"] = np.asarray([digest(mods[n].weight) for n in names])
    lora.net_load_lora(h, path, alpha=ALPHA, remove=True)
    out["sha_removed"] = np.asarray([digest(mods[n].weight) for n in names])
    orig = synth.synth_state_dict(synth.param_spec(net), seed=0)
    resid = max(float((mods[n].weight - orig[n + ".weight"]).abs().max()) for n in names)
    print(f"v1 removal: largest residue {resid:.2e}")
    out["v1_residue"] = np.float64(resid)

    h, net = fresh()
    mods = dict(net.named_modules())
    origin = lora.net_load_lora_v2(h, path, alpha=ALPHA)
    out["sha_v2_loaded"] = np.asarray([digest(mods[n].weight) for n in names])
    assert len(origin) == len(names)
    origin = lora.net_load_lora_v2(h, path, alpha=ALPHA, remove=True, origin_weight=origin)
    out["sha_v2_removed"] = np.asarray([digest(mods[n].weight) for n in names])
    assert all(torch.equal(mods[n].weight, orig[n + ".weight"]) for n in names)     # v2 restores exactly what it snapshotted
    out["sha_original"] = np.asarray([digest(orig[n + ".weight"]) for n in names])

    # Conv2d targets on a bare holder: 1x1 and 3x3 (4-D factors [r, i, 1, 1] / [o, r, 1, 1])
    g = torch.Generator().manual_seed(9)
    ch = Holder()
    ch.c1, ch.c3 = nn.Conv2d(8, 6, 1), nn.Conv2d(8, 6, 3, padding=1)
    csd = {}
    with torch.no_grad():
        for name in ("c1", "c3"):
            w = getattr(ch, name).weight
            w.copy_(torch.randn(w.shape, generator=g) * 0.1)
            out[f"conv_{name}_before"] = w.detach().clone().numpy()
            csd[f"{name}.lora_down.weight"] = torch.randn(RANK, 8, 1, 1, generator=g) * 0.3
            csd[f"{name}.lora_up.weight"] = torch.randn(6, RANK, 1, 1, generator=g) * 0.3
            out[f"conv_{name}_down"], out[f"conv_{name}_up"] = csd[f"{name}.lora_down.weight"].numpy(), csd[f"{name}.lora_up.weight"].numpy()
    cpath = os.path.join(tmp, "conv.ckpt")
    torch.save(csd, cpath)
    lora.net_load_lora(ch, cpath, alpha=ALPHA)
    for name in ("c1", "c3"):
        out[f"conv_{name}_after"] = getattr(ch, name).weight.detach().numpy()
    np.savez_compressed(os.path.join(OUT, "lvdm_lora_tiny.npz"), **out)
    print("wrote lvdm_lora_tiny.npz:", os.path.getsize(os.path.join(OUT, "lvdm_lora_tiny.npz")), "bytes;", len(names), "Linears")


if __name__ == "__main__":
    main()
