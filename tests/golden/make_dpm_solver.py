"""Fixture generator (builder container only: imports the REAL reference through ref_loader): the reference's own
``generate_image`` with the FIRST-ORDER DPM-Solver++ step injected as ``tests/dpm_solver_cpu.py::DPMSolverCPU(solver_order=1)``.
The first-order step is stateless, so the reference -- which calls ``scheduler.step`` up to three times per timestep -- can run it;
the second-order step needs the history rule of DESIGN.md section 25 and exists only in ``SolverOracle``.

Four cases (``dpm_solver_cpu.SOLVER_CASES``: epsilon / leading on a padded RePaint geometry, no RePaint, v-prediction / trailing,
ControlNet), fake UNet / VAE, about a second of CPU each.  Per case: the reference's final latent and the ``torch.rand(4)`` drawn
right after (``<name>/order1/...``), stored after asserting that ``SolverOracle`` at order 1 is bit-identical on both, and
``SolverOracle``'s second-order latent and tail (``<name>/order2/...``).

    python tests/golden/make_dpm_solver.py        # writes tests/golden/g16_dpm_solver.npz
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
    out = {}
    for name in D.SOLVER_CASES:
        z, tail = D.run_reference_case(name)
        assert bool(torch.isfinite(z).all()), name
        want, otail = D.run_oracle_case(name, 1)
        assert torch.equal(z, want), f"{name}: order-1 oracle != reference"
        assert torch.equal(tail, otail), f"{name}: RNG end state differs"
        z2, tail2 = D.run_oracle_case(name, 2)
        assert bool(torch.isfinite(z2).all()) and not torch.equal(z2, z), name
        assert torch.equal(tail2, tail), f"{name}: the order changes no draw"
        out[f"{name}/order1/latent"], out[f"{name}/order1/rng_tail"] = z.numpy(), tail.numpy()
        out[f"{name}/order2/latent"], out[f"{name}/order2/rng_tail"] = z2.numpy(), tail2.numpy()
        print(f"{name}: max |latent| order 1 {float(z.abs().max()):.3g}, order 2 {float(z2.abs().max()):.3g}, "
              f"reference == oracle at order 1")
    path = os.path.join(ROOT, "tests", "golden", "g16_dpm_solver.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
