"""Fixture generator (builder container only: imports the REAL reference through ref_loader): the reference's own
``ElasticDiffusion.rescale_noise_cfg`` (the method does not use ``self``) on seeded inputs -- 4 shapes x 2 means x 2
rescale factors (tests/guidance_rescale_cpu.py: G15_*).  The inputs are NOT stored: they are regenerated from the
``torch.Generator`` seeds kept in the file (``local = randn + mean``, ``direction = 0.1 * randn``, g = 10).  Stored per case:
the reference's output (in full, or a strided sample of the largest shape) and, per (shape, mean), the per-sample
std ratio evaluated in fp64 on the same fp32 inputs -- the bar the device reduction is held to.

    python tests/golden/make_guidance_rescale.py        # writes tests/golden/g15_guidance_rescale.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from tests import guidance_rescale_cpu as G
    from tests.golden.ref_loader import load_reference
    ref = load_reference()
    out = {}
    for key, shape, mean, seed in G.g15_cases():
        _, _, m_cfg, m_text = G.g15_inputs(seed, shape, mean)
        out[f"{key}/seed"] = np.array(seed)
        r64 = G.ratio_fp64(m_cfg, m_text)
        out[f"{key}/ratio_fp64"] = r64.numpy()
        r32 = (G.sample_std(m_text) / G.sample_std(m_cfg)).flatten().double()
        worst = float(((r32 - r64).abs() / r64).max())
        for gr in G.G15_RESCALES:
            got = ref.ElasticDiffusion.rescale_noise_cfg(None, m_cfg, m_text, gr)
            assert got.dtype == torch.float32 and bool(torch.isfinite(got).all()), key
            assert torch.equal(got, G.rescale_guided(m_cfg, m_text, gr)), f"{key}: restatement != reference"
            out[f"{key}/gr{gr}/out"] = G.g15_probe(got).numpy()
        print(f"{key}: seed {seed}, fp64 ratio {r64.tolist()}, torch fp32 ratio off by {worst:.1e}")
    path = os.path.join(ROOT, "tests", "golden", "g15_guidance_rescale.npz")
    np.savez_compressed(path, torch_version=np.array(torch.__version__), **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
