"""Fixture generator (builder container only: imports the REAL reference through ref_loader): the reference's own
``generate_image`` with the scheduler settings beyond the SD defaults -- v-prediction, trailing / linspace timestep spacing,
zero-terminal-SNR betas -- injected as ``tests/ddim_variants.py::DDIMVariants`` (the reference takes whatever its
``DDIMScheduler.from_pretrained`` returns, elastic_diffusion.py:153).  Six cases (``ddim_variants.VARIANT_CASES``), fake
UNet / VAE, under a second of CPU each.  For every case the reference's final latent and the ``torch.rand(4)`` drawn right
after are stored, after asserting that ``ElasticOracle`` with the same scheduler is bit-identical on both.

    python tests/golden/make_scheduler_variants.py        # writes tests/golden/g13_scheduler_variants.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from tests import ddim_variants as V
    out = {}
    for name, c in V.VARIANT_CASES.items():
        z, tail, ts = V.run_reference_case(name)
        assert ts == c["timesteps"], (name, ts)
        assert bool(torch.isfinite(z).all()), name
        want, otail = V.run_oracle_case(name)
        assert torch.equal(z, want), f"{name}: oracle != reference"
        assert torch.equal(tail, otail), f"{name}: RNG end state differs"
        out[f"{name}/latent"] = z.numpy()
        out[f"{name}/rng_tail"] = tail.numpy()
        print(f"{name}: timesteps {ts}, max |latent| {float(z.abs().max()):.3g}, reference == oracle")
    path = os.path.join(ROOT, "tests", "golden", "g13_scheduler_variants.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
