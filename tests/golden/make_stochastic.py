"""Fixture generator (builder container only: imports the REAL reference through ref_loader): the reference's own
``generate_image`` with each STATELESS stochastic step injected as ``tests/stochastic_cpu.py::StochasticCPU`` -- DDIM at eta = 1
("eta1"; "euler_a" is the same step), first-order SDE-DPM-Solver++ ("sde1") and LCM ("lcm", whose last step is keyed by the
timestep and needs no counter).  The injected ``step`` draws ``torch.randn(sample.shape)`` where the reference calls it -- both
phases, and the reduced-resolution step inside RRG -- so the fixture pins the ORDER of the draws, not only the arithmetic.  The
second-order SDE step needs the history rule of DESIGN.md section 25 and exists only in ``StochasticOracle`` ("sde2").

Four cases (``dpm_solver_cpu.SOLVER_CASES``: epsilon / leading on a padded RePaint geometry, no RePaint, v-prediction / trailing,
ControlNet), fake UNet / VAE, about a second of CPU each.  Per case and sampler: the reference's final latent and the
``torch.rand(4)`` drawn right after (``<name>/<sampler>/...``), stored after asserting that ``StochasticOracle`` is bit-identical on
both; and ``StochasticOracle``'s second-order SDE latent and tail (``<name>/sde2/...``).  Latents are stored as fp32.

    python tests/golden/make_stochastic.py        # writes tests/golden/g18_stochastic.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from tests import dpm_solver_cpu as D
    from tests import stochastic_cpu as S
    out = {}
    for name in D.SOLVER_CASES:
        plain, plain_tail = D.run_oracle_case(name, 1)
        for key, kw in S.STATELESS.items():
            z, tail = S.run_reference_case(name, kw)
            assert bool(torch.isfinite(z).all()), (name, key)
            want, otail = S.run_oracle_case(name, kw)
            assert torch.equal(z, want), f"{name}/{key}: oracle != reference"
            assert torch.equal(tail, otail), f"{name}/{key}: RNG end state differs"
            # LCM's last step draws nothing, and on a padded geometry the strip reseeds of the last phase erase what came before
            assert key == "lcm" or not torch.equal(tail, plain_tail), f"{name}/{key}: the stochastic steps drew nothing"
            out[f"{name}/{key}/latent"], out[f"{name}/{key}/rng_tail"] = z.numpy(), tail.numpy()
            print(f"{name}/{key}: max |latent| {float(z.abs().max()):.3g}, reference == oracle (latent and RNG tail)")
        z2, tail2 = S.run_oracle_case(name, dict(sampler="dpmsolver++sde", solver_order=2))
        assert bool(torch.isfinite(z2).all()) and not torch.equal(z2, torch.from_numpy(out[f"{name}/sde1/latent"])), name
        assert torch.equal(tail2, torch.from_numpy(out[f"{name}/sde1/rng_tail"])), f"{name}: the order changes no draw"
        out[f"{name}/sde2/latent"], out[f"{name}/sde2/rng_tail"] = z2.numpy(), tail2.numpy()
    path = os.path.join(ROOT, "tests", "golden", "g18_stochastic.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
