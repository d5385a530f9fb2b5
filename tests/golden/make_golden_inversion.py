"""Generate tests/golden/ddim_inversion_tiny.npz FROM THE REAL REFERENCE (run where the reference is mounted):

    python tests/golden/make_golden_inversion.py

The reference's own `DDIMSampler` (scripts/samplers/ddim/sampler.py, through oracle/ref_bootstrap.py) on the tiny UNet, on the CPU, with
the seeds and inputs of make_golden.py:other_samplers (tests/inversion_ref.py:inputs).  As there, the only change is that the class's
cuda-pinned device points at the CPU; nothing of the reference is changed or copied.  Stored (each latent [1, 4, 3, 16, 16] fp32):

  enc_plain            encode, S = 4, t_enc = 3, scale 1
  enc_guided           encode, S = 4, t_enc = 3, scale 9 with uc
  enc_orig             encode, use_original_steps=True, t_enc = 5
  enc_inter            encode, S = 6, t_enc = 5, return_intermediates=2; enc_inter_intermediates / enc_inter_steps: what it kept
  vid2vid_inverted_x0  decode (scale 9 with uc, as ddim_vid2vid_x0 of tiny.npz) run on enc_plain
  roundtrip_ref_rel    rel-L2 of decode(encode(z0, n), n) against z0 with a constant eps (seed 3), (S, n) = (4, 3), (4, 4), (20, 20):
                       the error of the reference's own fp32 arithmetic on the algebraic identity
  ddim_temp_x0         sample, 4 steps, scale 9, eta = 1, temperature = 0.5, torch.manual_seed(0) before the run (the per-step draws)
  ddim_ucg_x0          sample, 4 steps, eta = 0, ucg_schedule = [9, 7, 5, 3]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import configs, ref_bootstrap as rb, synth  # noqa: E402
import inversion_ref as IR  # noqa: E402


def main():
    cfg = configs.TINY_UNET
    unet, betas = rb.build_reference_unet(cfg)
    synth.load_synth(unet, seed=0)
    ref = rb.bootstrap()
    cpu = torch.device("cpu")
    z0, noise, c, uc = IR.inputs(cfg["context_dim"])
    shape = tuple(noise.shape)
    out = {}

    def ddim(model):
        s = ref.samplers.Txt2VideoSampler(model, cpu, betas=betas, sampler_name="DDIM")
        s.sampler.device = cpu
        return s.sampler

    with torch.no_grad():
        smp = ddim(unet)
        smp.make_schedule(4)
        out["enc_plain"] = smp.encode(z0, c, 3)[0].numpy()
        out["enc_guided"] = smp.encode(z0, c, 3, unconditional_guidance_scale=9.0, unconditional_conditioning=uc)[0].numpy()
        out["vid2vid_inverted_x0"] = smp.decode(torch.from_numpy(out["enc_plain"]), c, 3, unconditional_guidance_scale=9.0,
                                                unconditional_conditioning=uc).numpy()
        out["enc_orig"] = smp.encode(z0, c, 5, use_original_steps=True)[0].numpy()
        smp.make_schedule(6)
        x, info = smp.encode(z0, c, 5, return_intermediates=2)
        out["enc_inter"] = x.numpy()
        out["enc_inter_intermediates"] = torch.stack(info["intermediates"]).numpy()
        out["enc_inter_steps"] = np.asarray(info["intermediate_steps"], dtype=np.int64)
        assert out["enc_inter_steps"].tolist() == [0, 2, 3, 4]

        # the constant-eps round trip: the alpha_cumprod_prev buffer the class reads is the one UNetSD.register_schedule made
        const = IR.ConstEpsModel(IR.const_eps())
        const.alphas_cumprod_prev = unet.alphas_cumprod_prev
        rels = []
        for S, n in IR.ROUNDTRIPS:
            smp = ddim(const)
            smp.make_schedule(S)
            enc, _ = smp.encode(z0, c, n)
            rels.append(IR.rel_l2(smp.decode(enc, c, n), z0))
        out["roundtrip_ref_rel"] = np.asarray(rels, dtype=np.float64)

        smp = ddim(unet)
        torch.manual_seed(IR.NOISE_SEED)
        out["ddim_temp_x0"] = smp.sample(S=4, batch_size=1, shape=shape, conditioning=c, x_T=noise.clone(), eta=1.0,
                                         temperature=IR.TEMPERATURE, unconditional_guidance_scale=9.0,
                                         unconditional_conditioning=uc).numpy()
        out["ddim_ucg_x0"] = smp.sample(S=4, batch_size=1, shape=shape, conditioning=c, x_T=noise.clone(), eta=0.0,
                                        ucg_schedule=list(IR.UCG_SCHEDULE), unconditional_guidance_scale=9.0,
                                        unconditional_conditioning=uc).numpy()
    np.savez_compressed(IR.GOLD, **out)
    print({k: (v.shape, float(np.asarray(v, dtype=np.float64).std())) for k, v in out.items()}, out["roundtrip_ref_rel"])


if __name__ == "__main__":
    main()
