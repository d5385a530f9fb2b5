"""Digest of every lowered program of a fixed matrix of networks, geometries and options: one line per row — op count, arena bytes,
SHA-256 (tests/harness.py program_digest).  A refactor of the lowerings is proven on the CPU by running this on both commits and
diffing the outputs: equal lines = the library is handed the same bytes.
Usage: python tools/program_digest.py [--root PATH]      PATH: the checkout whose package is lowered (default: this one)."""
import argparse
import importlib.util
import os
import sys
import traceback

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE)
ROOT = os.path.abspath(ap.parse_args().root)
# the output must not depend on the box or on the caller's environment
FIXED = {"T2V_EXPERIMENTAL": "1", "T2V_FUSED_TATTN": "force", "T2V_DEVICE_CUS": "256"}
os.environ.update(FIXED)
for k in [k for k in os.environ if k.startswith("T2V_") and k not in FIXED]:
    del os.environ[k]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401
from oracle import configs, synth  # noqa: E402
from sd_webui_text2video_amd import unet as U, vae as V, videocrafter as VC  # noqa: E402
from sd_webui_text2video_amd.program import TShardSpec  # noqa: E402

# the digest itself always comes from THIS checkout (the parent commit's harness does not have it)
_spec = importlib.util.spec_from_file_location("_digest_harness", os.path.join(HERE, "tests", "harness.py"))
_harness = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_harness)


def row(label, net, compile_fn, attrs=None, env=None, weights=True):
    """Lower one program with `attrs` set on the net and `env` in the environment; both are restored afterwards."""
    attrs, env = attrs or {}, env or {}
    missing = object()
    old_attrs = {k: getattr(net, k, missing) for k in attrs}
    old_env = {k: os.environ.get(k) for k in env}
    try:
        for k, v in attrs.items():
            setattr(net, k, v)
        os.environ.update(env)
        comp = compile_fn()
        digest = _harness.program_digest(comp, net.state_dict() if weights else None)
        print(f"{label:<58} {len(comp.prog.ops):5d} {comp.prog.arena.high:12d} {digest}", flush=True)
    except Exception as e:            # a row that does not lower is reported, never hidden
        tb = traceback.extract_tb(e.__traceback__)[-1]
        print(f"{label:<58} FAILED {type(e).__name__}: {e} ({os.path.basename(tb.filename)}:{tb.lineno})", flush=True)
    finally:
        for k, v in old_attrs.items():
            delattr(net, k) if v is missing else setattr(net, k, v)
        for k, v in old_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


OPTIONS = [("precise_operands", dict(precise_operands=True)), ("precise_operands=r3", dict(precise_operands="r3")),
           ("precise_operands=all", dict(precise_operands="all")),
           ("precise_attn_out", dict(precise_operands=True, precise_attn_out=True)),
           ("precise_resample", dict(precise_operands=True, precise_resample=True)),
           ("gn_producer_stats", dict(gn_producer_stats=True)),
           ("split_weight_prefixes", dict(split_weight_prefixes=("input_blocks.1.",))),
           ("fused_cross_attention=True", dict(fused_cross_attention=True)), ("fused_cross_attention=False", dict(fused_cross_attention=False)),
           ("fused_temporal_attention=False", dict(fused_temporal_attention=False)),
           ("fused_temporal_attention=True", dict(fused_temporal_attention=True)),
           ("fused_temporal_attention=force", dict(fused_temporal_attention="force")),
           ("norm_input_dtype=f32", dict(norm_input_dtype="f32"))]
KNOBS_OFF = ["T2V_GN_CAST", "T2V_ATTN2", "T2V_TSHARD_STRIPS", "T2V_GN_STRIPS_AUTO", "T2V_GN_EPI", "T2V_GN_COOP"]


def tiny_rows(tag, net, F, H, W, Lc):
    plain = lambda **kw: net._compile(2, F, H, W, Lc, "f32", "f32", "f32", **kw)
    row(f"{tag} defaults", net, plain)
    for name, attrs in OPTIONS:
        row(f"{tag} {name}", net, plain, attrs)
    row(f"{tag} precise_operands=False", net, plain, dict(precise_operands=False))
    row(f"{tag} _share_now x_batch=1", net, lambda: plain(x_batch=1), dict(_share_now=True))
    for name, attrs in (("fused_cross_attention", dict(fused_cross_attention=True)), ("precise_operands=False", dict(precise_operands=False)),
                        ("precise_attn_out all levels", dict(precise_operands="all", precise_attn_out=True))):
        row(f"{tag} _share_now x_batch=1 {name}", net, lambda: plain(x_batch=1), dict(attrs, _share_now=True))
    row(f"{tag} debug_taps", net, plain, dict(debug_taps=True))
    row(f"{tag} b=1 fp16 io", net, lambda: net._compile(1, F, H, W, Lc, "f16", "f16", "f16"))
    for total, R, env in ((5, 3, {}), (8, 4, {}), (8, 4, {"T2V_STATS_HALO": "0"})):
        for r in range(R):
            spec = TShardSpec.make(total, R, r)
            row(f"{tag} rank {r}/{R} of {total} f{''.join(f' {k}={v}' for k, v in env.items())}", net,
                lambda s=spec: net._compile(1, s.frames, H, W, Lc, "f32", "f32", "f32", shard=s), env=env)
    for k in KNOBS_OFF:
        row(f"{tag} {k}=0", net, plain, env={k: "0"})


def main():
    print("# row, ops, arena bytes, sha256")
    # ---- synthetic weights, tiny configurations: records AND packed images
    ms = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(ms, seed=0)
    tiny_rows("tiny modelscope", ms, 3, 16, 16, 7)
    lv = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    lv.load_state_dict(synth.synth_state_dict(synth.param_spec(lv), seed=0), strict=True)
    tiny_rows("tiny lvdm", lv, 5, 8, 8, 9)
    for F in (16, 40):
        row(f"tiny lvdm {F} frames", lv, lambda F=F: lv._compile(2, F, 8, 8, 9, "f32", "f32", "f32"))
    row("tiny lvdm T2V_RELPOS_MFMA=3", lv, lambda: lv._compile(2, 5, 8, 8, 9, "f32", "f32", "f32"), env={"T2V_RELPOS_MFMA": "3"})
    for n, xb in ((1, 1), (2, 0)):
        for share in (False, True):
            row(f"tiny lvdm adapter={n} share={int(share)}", lv,
                lambda n=n, xb=xb: lv._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", x_batch=xb, adapter=n), dict(_share_now=share))

    # ---- full size, records only
    full = U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False)
    for F, H, W in ((8, 32, 32), (24, 32, 32), (125, 32, 32), (24, 72, 128)):
        row(f"modelscope b=2 x_batch=1 {F} f {H}x{W}", full,
            lambda F=F, H=H, W=W: full._compile(2, F, H, W, 77, "f16", "f32", "f16", x_batch=1), weights=False)
    for total, R, ranks in ((125, 4, range(4)), (24, 3, (0,))):
        for r in ranks:
            spec = TShardSpec.make(total, R, r)
            row(f"modelscope rank {r}/{R} of {total} f 32x32", full,
                lambda s=spec: full._compile(1, s.frames, 32, 32, 77, "f16", "f32", "f16", shard=s), weights=False)
    fv = VC.UNetModel(**configs.LVDM_UNET, init_weights=False)
    for F in (16, 40):
        row(f"lvdm b=2 x_batch=1 {F} f 32x32", fv, lambda F=F: fv._compile(2, F, 32, 32, 77, "f16", "f32", "f16", x_batch=1), weights=False)
    row("lvdm 16 f adapter=1", fv, lambda: fv._compile(2, 16, 32, 32, 77, "f16", "f32", "f16", x_batch=1, adapter=1), weights=False)
    spec = TShardSpec.make(16, 4, 1)
    row("lvdm rank 1/4 of 16 f", fv, lambda: fv._compile(1, spec.frames, 32, 32, 77, "f16", "f32", "f16", shard=spec), weights=False)

    # ---- VAE (the declarations' base class changes under it)
    def vae_row(label, ae, n, h, w, build, weights):
        low = V._VaeLowering(ae, n, h, w, "f32", "f32")
        row(label, ae, lambda: U._Compiled(build(low), low.packer), weights=weights)

    tv = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4)
    synth.load_synth(tv, seed=3)
    fa = V.AutoencoderKL(configs.VAE_DDCONFIG, 4, init_weights=False)
    vae_row("vae decode tiny n=2 8x8", tv, 2, 8, 8, lambda low: low.build(), True)
    vae_row("vae decode n=2 32x32", fa, 2, 32, 32, lambda low: low.build(), False)
    vae_row("vae decode u8 tiny n=2 8x8", tv, 2, 8, 8, lambda low: low.build((1, False)), True)
    vae_row("vae encoder tiny n=3 64x48", tv, 3, 64, 48, lambda low: low.build_encoder(), True)
    vae_row("vae encoder u8_src tiny n=3 64x48 from 100x80", tv, 3, 64, 48, lambda low: low.build_encoder(u8_src=(100, 80)), True)


if __name__ == "__main__":
    main()
