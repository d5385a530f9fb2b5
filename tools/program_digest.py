"""Digest of every lowered program of a fixed matrix of networks, geometries and options: one line per row — op count, arena bytes,
SHA-256 (tests/harness.py program_digest).  A refactor of the lowerings is proven on the CPU by running this on both commits and
diffing the outputs: equal lines = the library is handed the same bytes.
Usage: python tools/program_digest.py [--root PATH]      PATH: the checkout whose package is lowered (default: this one).
The matrix itself is `rows()`: an iterator of (label, lowering thunk, attrs, env) that tests/test_plan_hazards_cpu.py walks too."""
import argparse
import contextlib
import importlib.util
import os
import sys
import traceback
from typing import NamedTuple

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the output must not depend on the box or on the caller's environment
FIXED = {"T2V_EXPERIMENTAL": "1", "T2V_FUSED_TATTN": "force", "T2V_DEVICE_CUS": "256"}


class Row(NamedTuple):
    label: str
    thunk: object          # () -> the compiled program (.prog, .packer), called inside `applied(row)`
    attrs: dict            # attributes set on `net` while the thunk runs
    env: dict              # environment variables set while the thunk runs (on top of FIXED)
    net: object
    weights: bool          # digest the packed images too (synthetic weights) or the records only
    shard: object = None   # the TShardSpec of a T-sharded row (this rank's slice of the clip)


def fix_environment():
    os.environ.update(FIXED)
    for k in [k for k in os.environ if k.startswith("T2V_") and k not in FIXED]:
        del os.environ[k]


@contextlib.contextmanager
def applied(r: Row):
    """`r.attrs` set on the net and `r.env` in the environment; both are restored afterwards."""
    missing = object()
    old_attrs = {k: getattr(r.net, k, missing) for k in r.attrs}
    old_env = {k: os.environ.get(k) for k in r.env}
    try:
        for k, v in r.attrs.items():
            setattr(r.net, k, v)
        os.environ.update(r.env)
        yield
    finally:
        for k, v in old_attrs.items():
            delattr(r.net, k) if v is missing else setattr(r.net, k, v)
        for k, v in old_env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def row(label, net, compile_fn, attrs=None, env=None, weights=True, shard=None) -> Row:
    return Row(label, compile_fn, attrs or {}, env or {}, net, weights, shard)


def print_row(r: Row, digest_fn):
    """Lower one program with `attrs` set on the net and `env` in the environment and print its line."""
    try:
        with applied(r):
            comp = r.thunk()
            digest = digest_fn(comp, r.net.state_dict() if r.weights else None)
        print(f"{r.label:<58} {len(comp.prog.ops):5d} {comp.prog.arena.high:12d} {digest}", flush=True)
    except Exception as e:            # a row that does not lower is reported, never hidden
        tb = traceback.extract_tb(e.__traceback__)[-1]
        print(f"{r.label:<58} FAILED {type(e).__name__}: {e} ({os.path.basename(tb.filename)}:{tb.lineno})", flush=True)


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


def tiny_rows(tag, net, F, H, W, Lc, TShardSpec):
    plain = lambda **kw: net._compile(2, F, H, W, Lc, "f32", "f32", "f32", **kw)
    yield row(f"{tag} defaults", net, plain)
    for name, attrs in OPTIONS:
        yield row(f"{tag} {name}", net, plain, attrs)
    yield row(f"{tag} precise_operands=False", net, plain, dict(precise_operands=False))
    yield row(f"{tag} _share_now x_batch=1", net, lambda: plain(x_batch=1), dict(_share_now=True))
    for name, attrs in (("fused_cross_attention", dict(fused_cross_attention=True)), ("precise_operands=False", dict(precise_operands=False)),
                        ("precise_attn_out all levels", dict(precise_operands="all", precise_attn_out=True))):
        yield row(f"{tag} _share_now x_batch=1 {name}", net, lambda: plain(x_batch=1), dict(attrs, _share_now=True))
    yield row(f"{tag} debug_taps", net, plain, dict(debug_taps=True))
    yield row(f"{tag} b=1 fp16 io", net, lambda: net._compile(1, F, H, W, Lc, "f16", "f16", "f16"))
    for total, R, env in ((5, 3, {}), (8, 4, {}), (8, 4, {"T2V_STATS_HALO": "0"})):
        for r in range(R):
            spec = TShardSpec.make(total, R, r)
            yield row(f"{tag} rank {r}/{R} of {total} f{''.join(f' {k}={v}' for k, v in env.items())}", net,
                      lambda s=spec: net._compile(1, s.frames, H, W, Lc, "f32", "f32", "f32", shard=s), env=env, shard=spec)
    for k in KNOBS_OFF:
        yield row(f"{tag} {k}=0", net, plain, env={k: "0"})


def rows(root=HERE):
    """Every row of the matrix, in the order the tool prints them.  `root`: the checkout whose package is lowered.  The caller provides
    the FIXED environment (fix_environment(), or a test's monkeypatch) before it iterates."""
    root = os.path.abspath(root)
    for p in (os.path.join(root, "tests"), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch  # noqa: F401
    from oracle import configs, synth
    from sd_webui_text2video_amd import unet as U, vae as V, videocrafter as VC
    from sd_webui_text2video_amd.program import TShardSpec

    # ---- synthetic weights, tiny configurations: records AND packed images
    ms = U.UNetSD(**configs.TINY_UNET)
    synth.load_synth(ms, seed=0)
    yield from tiny_rows("tiny modelscope", ms, 3, 16, 16, 7, TShardSpec)
    lv = VC.UNetModel(**configs.TINY_LVDM_UNET, init_weights=False)
    lv.load_state_dict(synth.synth_state_dict(synth.param_spec(lv), seed=0), strict=True)
    yield from tiny_rows("tiny lvdm", lv, 5, 8, 8, 9, TShardSpec)
    for F in (16, 40):
        yield row(f"tiny lvdm {F} frames", lv, lambda F=F: lv._compile(2, F, 8, 8, 9, "f32", "f32", "f32"))
    yield row("tiny lvdm T2V_RELPOS_MFMA=3", lv, lambda: lv._compile(2, 5, 8, 8, 9, "f32", "f32", "f32"), env={"T2V_RELPOS_MFMA": "3"})
    for n, xb in ((1, 1), (2, 0)):
        for share in (False, True):
            yield row(f"tiny lvdm adapter={n} share={int(share)}", lv,
                      lambda n=n, xb=xb: lv._compile(2, 5, 8, 8, 9, "f32", "f32", "f32", x_batch=xb, adapter=n), dict(_share_now=share))

    # ---- full size, records only
    full = U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False)
    for F, H, W in ((8, 32, 32), (24, 32, 32), (125, 32, 32), (24, 72, 128)):
        yield row(f"modelscope b=2 x_batch=1 {F} f {H}x{W}", full,
                  lambda F=F, H=H, W=W: full._compile(2, F, H, W, 77, "f16", "f32", "f16", x_batch=1), weights=False)
    for total, R, ranks in ((125, 4, range(4)), (24, 3, (0,))):
        for r in ranks:
            spec = TShardSpec.make(total, R, r)
            yield row(f"modelscope rank {r}/{R} of {total} f 32x32", full,
                      lambda s=spec: full._compile(1, s.frames, 32, 32, 77, "f16", "f32", "f16", shard=s), weights=False, shard=spec)
    fv = VC.UNetModel(**configs.LVDM_UNET, init_weights=False)
    for F in (16, 40):
        yield row(f"lvdm b=2 x_batch=1 {F} f 32x32", fv, lambda F=F: fv._compile(2, F, 32, 32, 77, "f16", "f32", "f16", x_batch=1), weights=False)
    yield row("lvdm 16 f adapter=1", fv, lambda: fv._compile(2, 16, 32, 32, 77, "f16", "f32", "f16", x_batch=1, adapter=1), weights=False)
    spec = TShardSpec.make(16, 4, 1)
    yield row("lvdm rank 1/4 of 16 f", fv, lambda: fv._compile(1, spec.frames, 32, 32, 77, "f16", "f32", "f16", shard=spec), weights=False, shard=spec)

    # ---- VAE (the declarations' base class changes under it)
    def vae_row(label, ae, n, h, w, build, weights):
        low = V._VaeLowering(ae, n, h, w, "f32", "f32")
        return row(label, ae, lambda: U._Compiled(build(low), low.packer), weights=weights)

    tv = V.AutoencoderKL(configs.TINY_VAE_DDCONFIG, 4)
    synth.load_synth(tv, seed=3)
    fa = V.AutoencoderKL(configs.VAE_DDCONFIG, 4, init_weights=False)
    yield vae_row("vae decode tiny n=2 8x8", tv, 2, 8, 8, lambda low: low.build(), True)
    yield vae_row("vae decode n=2 32x32", fa, 2, 32, 32, lambda low: low.build(), False)
    yield vae_row("vae decode u8 tiny n=2 8x8", tv, 2, 8, 8, lambda low: low.build((1, False)), True)
    yield vae_row("vae encoder tiny n=3 64x48", tv, 3, 64, 48, lambda low: low.build_encoder(), True)
    yield vae_row("vae encoder u8_src tiny n=3 64x48 from 100x80", tv, 3, 64, 48, lambda low: low.build_encoder(u8_src=(100, 80)), True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    root = ap.parse_args().root
    fix_environment()
    # the digest itself always comes from THIS checkout (the parent commit's harness does not have it)
    sys.path[:0] = [os.path.abspath(root), os.path.join(os.path.abspath(root), "tests")]
    import torch  # noqa: F401
    spec = importlib.util.spec_from_file_location("_digest_harness", os.path.join(HERE, "tests", "harness.py"))
    harness = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(harness)
    print("# row, ops, arena bytes, sha256")
    for r in rows(root):
        print_row(r, harness.program_digest)


if __name__ == "__main__":
    main()
