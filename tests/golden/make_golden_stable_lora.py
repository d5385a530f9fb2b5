"""Generate the Stable LoRA golden FROM THE REAL REFERENCE (run where oracle/ref_bootstrap.py finds the reference checkout).

    python tests/golden/make_golden_stable_lora.py          # stable_lora_tiny.npz, seconds on a CPU

The reference's own `StableLoraProcessor.process_lora` (stable_lora/stable_utils/lora_processor.py:202-246), unmodified, with
`.device = "cpu"` and `.dtype` = the weights' dtype, merges seeded LoRA files into the reference's own UNetSD(**TINY_UNET) with the synthetic
weights of seed 0 — once fp32, once `.half()`.  The first file: rank 4, factors ~ N(0, scale^2), two modules of each of attn1.to_q,
attn2.to_k (context width), attn1.to_out.0, attn2.to_out.0, ff.net.0.proj and a SpatialTransformer's proj_in (both with 3-D factors: the
'proj' squeeze), ff.net.2, a ResBlock's 3x3 Conv2d, a 1x1 skip Conv2d, a temporal Conv3d (factors [r, 9 i] / [o, r]), plus a Conv1d proj_in
of a TemporalTransformer (the reference matches no class for it: untouched) and a `.bias` key for a module that has a bias (the reference sets
an attribute on the Parameter: nothing changes).  The second file (another seed) names every second target of the first.

Stored: the keys in order and the factors of both files; alpha; the touched and the untouched module names; for the fp16 model the
SHA-256 of every touched weight after the merge, after the undo, and after both files merged in one call on top of that (two files on one
module); the fp32 model's eps on tiny.npz's inputs after the merge.  (Digests, not tensors: a committed file is limited to 1 MiB, and the
tests compare bytes.)  The factor scale is raised until the merged and the un-merged eps differ by at least 100 x the 3.1e-3 gate of
test_tiny_unet_forward_matches_reference_golden; the ratio is recorded — a LoRA too weak to matter would let every test pass.

The call sequence of the state machine: the reference's own `StableLoraScript.process` (stable_lora/scripts/lora_webui.py:127-214) IS
imported and run — with a stub `gradio` module and stub `modules.images` / `modules.script_callbacks` that this script injects (they are
only used by `ui()`), `process_lora` replaced by a recorder, on stand-in modules and two real `.safetensors` files in a temporary
`cmd_opts.lora_dir` — through: first load, alpha change, second file added, option toggled, selection emptied.  The recording is the
reference's, not a reading of its code."""
import hashlib
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
ALPHA, RANK, GATE, PER_KIND = 0.7, 4, 3.1e-3, 2
FLAGS = dict(use_bias=True, use_time=True, use_conv=True, use_emb=True, use_linear=True)
# (class, name suffix, kernel size or None)
KINDS = ((nn.Linear, "attn1.to_q", None), (nn.Linear, "attn2.to_k", None), (nn.Linear, "attn1.to_out.0", None), (nn.Linear, "attn2.to_out.0", None),
         (nn.Linear, "ff.net.0.proj", None), (nn.Linear, "proj_in", None), (nn.Linear, "ff.net.2", None), (nn.Conv2d, "in_layers.2", (3, 3)),
         (nn.Conv2d, "skip_connection", (1, 1)), (nn.Conv3d, "", (3, 1, 1)))


def inputs_tiny():
    """The inputs of tiny.npz (tests/golden/make_golden.py:tiny)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 4, 3, 16, 16, generator=g)
    y = torch.randn(2, 7, configs.TINY_UNET["context_dim"], generator=g)
    return x, torch.tensor([801, 401]), y


def pick_targets(net):
    names = []
    for cls, suffix, ks in KINDS:
        found = [n for n, m in net.named_modules() if m.__class__ is cls and n.endswith(suffix) and (ks is None or tuple(m.kernel_size) == ks)]
        assert len(found) >= PER_KIND, (cls, suffix, found)
        names.extend(found[:PER_KIND])
    return names


def make_lora(net, names, extra, scale, seed):
    """names: merged targets; extra: (conv1d name, biased module name)."""
    g = torch.Generator().manual_seed(seed)
    mods = dict(net.named_modules())
    sd = {}
    for name in names + [extra[0]]:
        m = mods[name]
        w = m.weight
        o = w.shape[0]
        cols = w[0].numel() * (3 if isinstance(m, nn.Conv3d) else 1)
        A = torch.randn(RANK, cols, generator=g) * scale
        B = torch.randn(o, RANK, generator=g) * scale
        if isinstance(m, nn.Linear) and "proj" in name:
            A, B = A.unsqueeze(-1), B.unsqueeze(-1)
        sd[name + ".lora_A"], sd[name + ".lora_B"] = A, B
    sd[extra[1] + ".bias"] = torch.randn(mods[extra[1]].bias.shape, generator=g)
    return sd


def digest(t):
    return hashlib.sha256(t.detach().contiguous().numpy().tobytes()).hexdigest()


def rel_l2(a, b):
    return float((a - b).norm() / b.norm())


def record_call_sequence(tmp):
    """The reference's StableLoraScript.process on stand-ins, process_lora replaced by a recorder."""
    from safetensors.torch import save_file
    sys.modules.setdefault("gradio", types.ModuleType("gradio"))
    mods = sys.modules["modules"]
    for name in ("images", "script_callbacks"):
        if not hasattr(mods, name):
            m = types.ModuleType("modules." + name)
            sys.modules["modules." + name] = m
            setattr(mods, name, m)
    shared = sys.modules["modules.shared"]
    shared.cmd_opts.lora_dir = tmp
    web = importlib.import_module("stable_lora.scripts.lora_webui")
    for tag in ("f1", "f2"):
        save_file({"tag." + tag: torch.zeros(1)}, os.path.join(tmp, tag + ".safetensors"), metadata={"stable_lora_text_to_video": "1"})
    script = web.StableLoraScript()
    script.lora_files = [{"lora_name": t, "path": os.path.join(tmp, t + ".safetensors")} for t in ("f1", "f2")]
    script.log = lambda *a, **k: None
    p = types.SimpleNamespace(sd_model=nn.Linear(2, 2), clip_encoder=types.SimpleNamespace(model=types.SimpleNamespace(transformer=nn.Linear(3, 3))))
    calls = []

    def recorder(model, lora_files_list, use_bias, use_time, use_conv, use_emb, use_linear, lora_alpha, undo_merge=False):
        calls.append(dict(step=step, model="sd_model" if model is p.sd_model else "transformer",
                          files=[k.split(".")[1] for f in lora_files_list for k in f if k.startswith("tag.")],
                          flags=[bool(use_bias), bool(use_time), bool(use_conv), bool(use_emb), bool(use_linear)],
                          alpha=float(lora_alpha), undo=bool(undo_merge)))
    script.process_lora = recorder
    scenario = [  # selection, alpha, use_bias, use_linear, use_conv, use_emb, use_multiplier, use_time
        (["f1"], 1.0, True, True, True, True, 1, True),          # first load
        (["f1"], 0.5, True, True, True, True, 1, True),          # alpha change
        (["f1", "f2"], 0.5, True, True, True, True, 1, True),    # second file added
        (["f1", "f2"], 0.5, True, True, True, True, 1, False),   # option toggled
        ([], 0.5, True, True, True, True, 1, False),             # selection emptied
    ]
    loaded = []
    for step, args in enumerate(scenario):
        script.process(p, *args)
        loaded.append(bool(script.is_lora_loaded(p.sd_model)))
    return dict(scenario=scenario, calls=calls, loaded_after=loaded)


def main():
    rb.bootstrap()
    lp = importlib.import_module("stable_lora.stable_utils.lora_processor")
    x, t, y = inputs_tiny()

    def fresh(dtype):
        net, _ = rb.build_reference_unet(configs.TINY_UNET)
        synth.load_synth(net, seed=0)
        if dtype == torch.float16:
            net = net.half()
        proc = lp.StableLoraProcessor()
        proc.device, proc.dtype = "cpu", dtype
        return net, proc

    def merge(proc, net, files, alpha, undo=False):
        proc.process_lora(net, files, FLAGS["use_bias"], FLAGS["use_time"], FLAGS["use_conv"], FLAGS["use_emb"], FLAGS["use_linear"], alpha,
                          undo_merge=undo)

    net, proc = fresh(torch.float32)
    names = pick_targets(net)
    conv1d = next(n for n, m in net.named_modules() if m.__class__ is nn.Conv1d and n.endswith("proj_in"))
    biased = next(n for n, m in net.named_modules() if m.__class__ is nn.Linear and n.endswith("attn1.to_out.0") and n not in names)
    with torch.no_grad():
        eps0 = net(x, t, y)
    gold0 = np.load(os.path.join(OUT, "tiny.npz"))["unet_eps"]
    assert np.array_equal(eps0.numpy(), gold0), "the un-merged reference forward is not tiny.npz's"
    scale = 0.05
    while True:
        net, proc = fresh(torch.float32)
        sd1 = make_lora(net, names, (conv1d, biased), scale, seed=4)
        merge(proc, net, [sd1], ALPHA)
        with torch.no_grad():
            eps = net(x, t, y)
        sep = rel_l2(eps, eps0)
        print(f"factor scale {scale:g}: merged vs un-merged eps rel-L2 {sep:.3e} = {sep / GATE:.1f} x the gate")
        if sep >= 100 * GATE:
            break
        scale *= 1.5
    sd2 = make_lora(net, names[::2], (conv1d, biased), scale, seed=11)
    out = {"keys1": np.asarray(list(sd1.keys())), "keys2": np.asarray(list(sd2.keys())), "touched": np.asarray(names),
           "untouched": np.asarray([conv1d, biased]), "alpha": np.float64(ALPHA), "rank": np.int64(RANK), "scale": np.float64(scale),
           "separation": np.float64(sep), "separation_over_gate": np.float64(sep / GATE), "eps_merged": eps.numpy()}
    for tag, sd in (("a", sd1), ("b", sd2)):
        for k, v in enumerate(sd.values()):
            out[f"{tag}{k}"] = v.numpy()
    merge(proc, net, [sd1], ALPHA, undo=True)
    with torch.no_grad():
        out["fp32_undo_residue"] = np.float64(rel_l2(net(x, t, y), eps0))
    print(f"fp32 undo: eps back within {float(out['fp32_undo_residue']):.2e} of the un-merged one")

    # the deployed form: fp16 weights, fp16 factors, every step rounded to fp16
    net, proc = fresh(torch.float16)
    mods = dict(net.named_modules())
    watched = names + [conv1d, biased]
    out["sha_original"] = np.asarray([digest(mods[n].weight) for n in watched])
    bias0 = digest(mods[biased].bias)
    merge(proc, net, [sd1], ALPHA)
    out["sha_merged"] = np.asarray([digest(mods[n].weight) for n in watched])
    assert digest(mods[biased].bias) == bias0 and list(out["sha_merged"][-2:]) == list(out["sha_original"][-2:])
    assert all(a != b for a, b in zip(out["sha_merged"][:-2], out["sha_original"][:-2]))
    merge(proc, net, [sd1], ALPHA, undo=True)
    out["sha_undone"] = np.asarray([digest(mods[n].weight) for n in watched])
    merge(proc, net, [sd1, sd2], ALPHA)
    out["sha_two_files"] = np.asarray([digest(mods[n].weight) for n in watched])
    same = sum(a == b for a, b in zip(out["sha_undone"], out["sha_original"]))
    print(f"fp16: {len(names)} touched weights; after the undo {same - 2} of them are the original bytes again")

    with tempfile.TemporaryDirectory() as tmp:
        out["call_sequence"] = np.asarray(json.dumps(record_call_sequence(tmp)))
    print(json.loads(str(out["call_sequence"]))["calls"])
    path = os.path.join(OUT, "stable_lora_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote stable_lora_tiny.npz:", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
