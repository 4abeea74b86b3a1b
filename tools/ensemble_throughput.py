"""Throughput of GalaxyEnsemble against the loop of solo simulations it replaces.

For N in {256, 1024, 2048}, FLOAT64 and FLOAT32, and B in {1, 2, 4, 8, 16, 32} members, microseconds per tick of
  ens    one GalaxyEnsemble of B members doing run(200)
  solos  B GalaxySimulations doing run(200) one after another, each waited for before the next starts (the sweep loop)
Each figure is the median of REPEATS timed run(200) calls (host clock around work that ends in a device synchronise)
with the min .. max beside it; the two variants alternate inside one repeat, after ~0.2 s of the same work as warm-up so
the clocks are at their sustained level.  Usage: python tools/ensemble_throughput.py [--out FILE] [--modes M,M,...]
[--sizes N,N,...] [--members B,B,...]

--modes takes float64, float32 (the default pair) and the grid modes int8_sim, int4_sim and custom (64 levels), which run
a QuantizedEnsemble against solo simulations of the same mode.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbody_cosmological_simulation_amd as nb  # noqa: E402

TICKS = 200
REPEATS = 9
SIZES = (256, 1024, 2048)
MEMBERS = (1, 2, 4, 8, 16, 32)
MODES = (nb.PrecisionMode.FLOAT64, nb.PrecisionMode.FLOAT32)
GRID_MODES = (nb.PrecisionMode.INT8_SIM, nb.PrecisionMode.INT4_SIM, nb.PrecisionMode.CUSTOM)


def state(b, n, dtype):
    g = torch.Generator().manual_seed(7 + n)
    pos = torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 5
    vel = torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 0.05
    mass = 0.5 + torch.rand(b, n, generator=g, dtype=torch.float64)
    return pos.to(dtype), vel.to(dtype), mass.to(dtype)


def timed(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) / TICKS * 1e6


def measure(n, mode, b):
    dtype = torch.float64 if mode == nb.PrecisionMode.FLOAT64 else torch.float32
    pos, vel, mass = state(b, n, dtype)
    dts = [0.01 + 0.0007 * k for k in range(b)]
    cls = nb.QuantizedEnsemble if mode in GRID_MODES else nb.GalaxyEnsemble
    ens = cls(pos.cuda(), vel.cuda(), mass.cuda(), precision_mode=mode, dt=dts)
    solos = [nb.GalaxySimulation(pos[k].cuda(), vel[k].cuda(), mass[k].cuda(), precision_mode=mode, dt=dts[k]) for k in range(b)]

    def run_ens():
        ens.run(TICKS)
        ens.synchronize()

    def run_solos():
        for s in solos:
            s.run(TICKS)
            s.synchronize()

    t = time.perf_counter()
    while time.perf_counter() - t < 0.2:
        run_ens()
        run_solos()
    te, ts = [], []
    for _ in range(REPEATS):
        te.append(timed(run_ens))
        ts.append(timed(run_solos))
    assert ens.force_kernel_name() == ("ens_grid_step_kernel" if mode in GRID_MODES else "ens_step_kernel")
    assert solos[0].force_kernel_name() == "small_step_kernel"
    ens.close()
    for s in solos:
        s.close()
    return te, ts


def fmt(v):
    return f"{statistics.median(v):8.2f} ({min(v):7.2f} .. {max(v):7.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--modes", help="comma-separated precision modes (default: float64,float32)")
    ap.add_argument("--sizes", help="comma-separated N (default: 256,1024,2048)")
    ap.add_argument("--members", help="comma-separated B (default: 1,2,4,8,16,32)")
    args = ap.parse_args()
    modes = tuple(nb.PrecisionMode(m) for m in args.modes.split(",")) if args.modes else MODES
    for m in modes:
        if m not in MODES + GRID_MODES:
            ap.error(f"--modes takes float64, float32, int8_sim, int4_sim and custom (got {m.value})")
    sizes = tuple(int(v) for v in args.sizes.split(",")) if args.sizes else SIZES
    members = tuple(int(v) for v in args.members.split(",")) if args.members else MEMBERS
    lines = [f"# us per tick of all B members together, run({TICKS}), median (min .. max) of {REPEATS} repeats; "
             f"{torch.cuda.get_device_name(0)}" + ("; custom: 64 levels" if nb.PrecisionMode.CUSTOM in modes else ""),
             f"{'mode':8s} {'N':>5s} {'B':>3s}  {'ensemble':>28s}  {'B solo runs, one after another':>30s}  {'solos/ens':>9s}"]
    for mode in modes:
        for n in sizes:
            for b in members:
                te, ts = measure(n, mode, b)
                lines.append(f"{mode.value:8s} {n:5d} {b:3d}  {fmt(te):>28s}  {fmt(ts):>30s}  "
                             f"{statistics.median(ts) / statistics.median(te):9.2f}")
                print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
