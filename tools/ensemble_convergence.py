"""The reference's convergence sweep (falsification_tests.py:44-104) as ONE FineGridEnsemble run.

The sweep steps one N = 2000 disk galaxy for 500 ticks under CUSTOM grids of 4, 8, ..., 4096 levels (the reference's list
goes on to 65 536 and beyond: those grids are the solo engine's generic kernel's) and prints the energy drift of each.
Here the eleven grids are the members of one FineGridEnsemble -- fp32, G = 0.001, dt = 0.01, softening 0.1, the package's
own create_disk_galaxy -- advanced by one run_recorded(500, every=500), against the loop of eleven solo GalaxySimulations.
Printed: the drift of every member from both, in the reference's format.  The two columns need not agree digit for digit: a
solo constructor evaluates the initial forces on the tiled path, whose sums differ from the one-launch body's in the last
bit, the members above 256 levels keep summing in another order than their solo runs, the ensemble's energies are the
batched ones (2e-6 relative), and 500 ticks under a coarse grid amplify a last-bit difference (measured on an MI355X:
168 % against 173 % at 4 levels, two to three equal digits from 8 levels on).  Then the two wall times (host clock, each ending
in a device synchronise, second of two runs), and the per-tick time (median of REPEATS run(200) calls, min .. max beside
it) of
  wide      the sweep's ensemble: "ens_grid_step_wide_kernel", tables in LDS sized for 4096 levels
  narrow    an ensemble of the same size whose members all have <= 256 levels: "ens_grid_step_kernel"
  wide257   the narrow ensemble with its last member at 257 levels: the smallest wide launch (tables padded to 512)
Usage: python tools/ensemble_convergence.py [--out FILE] [--stars N] [--ticks T]
"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbody_cosmological_simulation_amd as nb  # noqa: E402
from nbody_cosmological_simulation_amd.galaxy import create_disk_galaxy  # noqa: E402

LEVELS = [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]
NARROW = [4, 8, 16, 32, 64, 128, 256, 4, 8, 16, 32]
PARAMS = dict(G=0.001, softening=0.1, dt=0.01)
REPEATS = 7
TIMED_TICKS = 200


def drift(e0, e1):
    return (e1 - e0) / abs(e0) * 100


def sweep_ensemble(pos, vel, mass, ticks):
    t = time.perf_counter()
    ens = nb.FineGridEnsemble(pos, vel, mass, custom_levels=LEVELS, **PARAMS)
    hist = ens.run_recorded(ticks, every=ticks)
    ens.synchronize()
    wall = time.perf_counter() - t
    total = hist.total
    name = ens.force_kernel_name()
    ens.close()
    return [drift(float(total[0, b]), float(total[-1, b])) for b in range(len(LEVELS))], wall, name


def sweep_solos(pos, vel, mass, ticks):
    t = time.perf_counter()
    out, names = [], set()
    for levels in LEVELS:
        sim = nb.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=nb.PrecisionMode.CUSTOM,
                                  custom_levels=levels, **PARAMS)
        e0 = sim.get_total_energy()
        sim.run(ticks)
        out.append(drift(e0, sim.get_total_energy()))
        names.add(sim.force_kernel_name())
        sim.close()
    return out, time.perf_counter() - t, sorted(names)


def per_tick(pos, vel, mass, levels):
    ens = nb.FineGridEnsemble(pos, vel, mass, custom_levels=levels, **PARAMS)

    def run():
        t = time.perf_counter()
        ens.run(TIMED_TICKS)
        ens.synchronize()
        return (time.perf_counter() - t) / TIMED_TICKS * 1e6

    t = time.perf_counter()
    while time.perf_counter() - t < 0.2:
        run()
    us = [run() for _ in range(REPEATS)]
    name = ens.force_kernel_name()
    ens.close()
    return statistics.median(us), min(us), max(us), name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--stars", type=int, default=2000)
    ap.add_argument("--ticks", type=int, default=500)
    a = ap.parse_args()
    pos, vel, mass = (t.float().cuda() for t in create_disk_galaxy(num_stars=a.stars, galaxy_radius=10.0, seed=42))
    lines = [f"# convergence sweep: N = {a.stars}, {a.ticks} ticks, fp32, G = 0.001, dt = 0.01, softening 0.1, levels {LEVELS}"]
    for _ in range(2):                   # the second pass is the one reported: handles, clocks and caches are warm
        ens_drift, ens_wall, ens_name = sweep_ensemble(pos, vel, mass, a.ticks)
        solo_drift, solo_wall, solo_names = sweep_solos(pos, vel, mass, a.ticks)
    lines.append(f"# ensemble: {ens_name}; solo runs: {', '.join(solo_names)}")
    for levels, de, ds in zip(LEVELS, ens_drift, solo_drift):
        lines.append(f"  {levels:>7} levels ({math.log2(levels):>5.1f} bits): {de:+.6f}% drift (ensemble)  {ds:+.6f}% drift (solo)")
    lines.append(f"wall time of the sweep: one FineGridEnsemble.run_recorded {ens_wall * 1e3:.1f} ms, loop of {len(LEVELS)} solo "
                 f"runs {solo_wall * 1e3:.1f} ms ({solo_wall / ens_wall:.2f} x)")
    lines.append(f"# per tick of all {len(LEVELS)} members, us: median (min .. max) of {REPEATS} run({TIMED_TICKS}) calls")
    for tag, levels in (("wide", LEVELS), ("narrow", NARROW), ("wide257", NARROW[:-1] + [257])):
        med, lo, hi, name = per_tick(pos, vel, mass, levels)
        lines.append(f"  {tag:<8} {name:<26} levels {levels}: {med:.1f} ({lo:.1f} .. {hi:.1f})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
