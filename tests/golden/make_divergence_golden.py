#!/usr/bin/env python3
"""Generator of g23_divergence.npz: the reference's own MultiverseSim (reality_glitch_tests.py:148-256) on the CPU, 48 stars,
40 ticks.  Run by hand where the reference is available (like make_crash_golden.py), never by the suite:

    python tests/golden/make_divergence_golden.py <directory of the reference>      (or REFERENCE_DIR in the environment)

The file holds the initial state (create_disk_galaxy under torch.manual_seed(SEED)), the reference's two per-tick lists
divergence_ab_history / divergence_ac_history (largest |position difference| of universe A, FLOAT32, against B, the
reversed summation order, and against C, r^2 rounded through half()), and the fields of the DivergenceMetrics that every
step() returned: max_position_diff, mean_position_diff, max_velocity_diff, entropy_bits, divergence_rate.  Recorded
results only.  The reference imports matplotlib.pyplot at module level; without a display it picks its headless backend
and nothing is drawn.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_DIR")
if not REFERENCE:
    sys.exit(__doc__)
sys.path.insert(0, REFERENCE)
from galaxy import create_disk_galaxy                      # noqa: E402
from reality_glitch_tests import MultiverseSim             # noqa: E402

STARS, TICKS, SEED = 48, 40, 23


def main():
    torch.manual_seed(SEED)
    pos, vel, mass = create_disk_galaxy(num_stars=STARS, device="cpu")
    multi = MultiverseSim(pos, vel, mass, torch.device("cpu"))
    steps = [multi.step() for _ in range(TICKS)]
    out = dict(pos=pos.numpy(), vel=vel.numpy(), mass=mass.numpy(), seed=np.int64(SEED),
               divergence_ab_history=np.array(multi.divergence_ab_history, np.float64),
               divergence_ac_history=np.array(multi.divergence_ac_history, np.float64))
    for field in ("max_position_diff", "mean_position_diff", "max_velocity_diff", "entropy_bits", "divergence_rate"):
        out[field] = np.array([float(getattr(m, field)) for m in steps], np.float64)
    assert all(len(out[k]) == TICKS for k in out if k not in ("pos", "vel", "mass", "seed"))
    assert (out["max_position_diff"] > 1e-10).any() and (out["divergence_rate"] != 0).any(), "the run shows no divergence"
    np.savez_compressed(os.path.join(HERE, "g23_divergence.npz"), **out)
    for t in range(TICKS):
        print(f"{t + 1:3d} ab {out['divergence_ab_history'][t]:.3e} ac {out['divergence_ac_history'][t]:.3e} "
              f"bits {out['entropy_bits'][t]:.4f} rate {out['divergence_rate'][t]:+.5f}")
    print(f"{TICKS} ticks written")


if __name__ == "__main__":
    main()
