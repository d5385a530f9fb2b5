"""TEST INFRASTRUCTURE — the programs a user can obtain through the public interface, one entry per lowered program.  No test functions
here: tools/geometry_paths.py lowers every entry and keys every record (tests/record_paths.py), tests/test_geometry_paths_cpu.py demands an
adversarial case for every key of its witnesses and of a held-out sample.

An entry is plain data: Entry(model, form, F, H, W, shard) with the latent extents H x W and shard = (total frames, ranks, rank) or None;
`row_of(entry, nets)` makes the tools/program_digest.py row of it, so test_plan_hazards_cpu._lower and record_paths.path_keys work on it
unchanged.  The lowerings read no weights (init_weights=False: records only).

Where the limits come from:
  width, height  the webui sliders: 64 .. 1024 pixels in steps of 64 (reference scripts/t2v_helpers/args.py:52-53) = a latent of 8 .. 128 in
                 steps of 8, both orientations
  frames         the slider goes from 2 to 250 in steps of 1 (args.py:60); the library itself takes one frame too.  Every count from 1 to 40
                 (all residues of the tiles at every level of the UNet), then 48, 64, 100, 125 and the slider's end, 250
  the cap        F x H x W <= 1.2 x 125 x 32 x 32 latent positions: a fifth above the largest clip the project measures (125 frames at 256 x 256)
  LVDM frames    program.py:991 refuses clips of more than _lib.RELPOS_MAX_FRAMES (1024) frames: no frame count of the lattice reaches it
  adapter        videocrafter.py:241-242 refuses adapter features in a T-sharded forward: no sharded adapter entries (EXCLUDED says so)
  VAE frames     pipeline.py:301-302 decodes all frames of a clip in one program, videocrafter.py:941 / 963-965 in chunks of decode_bs = 16 and
                 a ragged last chunk (1 .. 15 frames) — all of them frame counts of the lattice; pipeline.py:289-292 and
                 videocrafter.py:919-920 encode all frames in one program.  vae.py:176 / 204 want image extents that are multiples of 8:
                 every latent of the lattice x 8 is one
  T shards       program.TShardSpec.make(total, ranks, rank): every rank of 2, 4 and 8 ranks over 24 and 125 frames at 32 x 32 and 40 x 72
The text tower is not here: its shapes do not depend on the video geometry."""
from __future__ import annotations

import random
from typing import NamedTuple, Optional

FRAMES = tuple(range(1, 41)) + (48, 64, 100, 125, 250)
EXTENTS = tuple(range(8, 129, 8))
CAP = int(1.2 * 125 * 32 * 32)
SHARD_TOTALS, SHARD_RANKS, SHARD_LATENTS = (24, 125), (2, 4, 8), ((32, 32), (40, 72))
MODELSCOPE_FORMS = ("guided", "pair", "b1")          # b = 2, x_batch = 1 | b = 4, x_batch = 2 (two videos) | b = 1, fp16 in and out
LVDM_FORMS = MODELSCOPE_FORMS + ("adapter",)          # the guided step with adapter = 1
VAE_FORMS = ("decode", "decode-u8", "encode")
# (rule, the line that refuses it): geometries of the lattice's ranges that are left out because the library refuses them
EXCLUDED = [("lvdm adapter=1 on any T shard", "videocrafter.py:241-242 T2VError: sharding the adapter features along T is not built")]


class Entry(NamedTuple):
    model: str                                # "modelscope" | "lvdm" | "vae"
    form: str
    F: int
    H: int
    W: int
    shard: Optional[tuple] = None             # (total, ranks, rank)

    @property
    def size(self):
        return self.F * self.H * self.W

    @property
    def label(self):
        s = f" rank {self.shard[2]}/{self.shard[1]} of {self.shard[0]} f" if self.shard else ""
        return f"{self.model} {self.form}{s} {self.F} f {self.H}x{self.W}"


def geometries():
    return [(F, H, W) for F in FRAMES for H in EXTENTS for W in EXTENTS if F * H * W <= CAP]


def entries():
    """Every program of the lattice, in a fixed order."""
    out = []
    for F, H, W in geometries():
        out += [Entry("modelscope", f, F, H, W) for f in MODELSCOPE_FORMS]
        out += [Entry("lvdm", f, F, H, W) for f in LVDM_FORMS]
        out += [Entry("vae", f, F, H, W) for f in VAE_FORMS]
    for model in ("modelscope", "lvdm"):
        for total in SHARD_TOTALS:
            for R in SHARD_RANKS:
                for r in range(R):
                    for H, W in SHARD_LATENTS:
                        out.append(Entry(model, "rank", _shard_frames(total, R, r), H, W, (total, R, r)))
    return out


def _shard_frames(total, R, r):
    from sd_webui_text2video_amd.program import TShardSpec
    return TShardSpec.make(total, R, r).frames


def make_nets():
    """The three networks at full size, without weights."""
    from oracle import configs
    from sd_webui_text2video_amd import unet as U, vae as V, videocrafter as VC
    return {"modelscope": U.UNetSD(**configs.MODELSCOPE_UNET, init_weights=False),
            "lvdm": VC.UNetModel(**configs.LVDM_UNET, init_weights=False),
            "vae": V.AutoencoderKL(configs.VAE_DDCONFIG, 4, init_weights=False)}


def row_of(e: Entry, nets):
    """The tools/program_digest.py row of an entry (records only)."""
    from sd_webui_text2video_amd import unet as U, vae as V
    from sd_webui_text2video_amd.program import TShardSpec
    from tools import program_digest as PD
    net, F, H, W = nets[e.model], e.F, e.H, e.W
    if e.model == "vae":
        def thunk():
            if e.form == "encode":          # image extents; fp16 frames (pipeline.py:290-291)
                low = V._VaeLowering(net, F, 8 * H, 8 * W, "f16", "f32")
                return U._Compiled(low.build_encoder(), low.packer)
            low = V._VaeLowering(net, F, H, W, "f32", "f16")
            return U._Compiled(low.build((1, False)) if e.form == "decode-u8" else low.build(), low.packer)
        return PD.row(e.label, net, thunk, weights=False)
    if e.shard is not None:
        spec = TShardSpec.make(*e.shard)
        return PD.row(e.label, net, lambda: net._compile(1, spec.frames, H, W, 77, "f16", "f32", "f16", shard=spec), weights=False, shard=spec)
    if e.form == "b1":
        return PD.row(e.label, net, lambda: net._compile(1, F, H, W, 77, "f16", "f16", "f16"), weights=False)
    b, xb = (4, 2) if e.form == "pair" else (2, 1)
    kw = dict(adapter=1) if e.form == "adapter" else {}
    return PD.row(e.label, net, lambda: net._compile(b, F, H, W, 77, "f16", "f32", "f16", x_batch=xb, **kw), weights=False)


def held_out(witnesses, n, seed):
    """A seeded sample of n entries that are not witnesses."""
    w = set(witnesses)
    rest = [e for e in entries() if e not in w]
    return random.Random(seed).sample(rest, n)
