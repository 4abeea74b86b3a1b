"""Cost of an energy curve of a GalaxyEnsemble: run_recorded() against the loop it replaces.

For FLOAT64 and FLOAT32, N in {256, 1024, 2048} and B in {1, 8, 32, 256} members, microseconds per tick of 200 ticks of
  rec k    (a) run_recorded(200, every=k): the energies sampled on the device, one native call
  loop k   (b) the same curve without it: 200 / k times run(k), get_kinetic_energy(), get_potential_energy() (the
           solo-equal read-out, one member at a time)
  run      (c) plain run(200), waited for
for k = 1 and k = 10.  Each figure is the median of REPEATS timed repeats (host clock around work that ends in a device
synchronise) with the min .. max beside it; the variants alternate inside one repeat, after every variant has run once
and ~0.2 s of run(200) as warm-up.  `sample` is what one sample costs on top of the ticks: ((a) - (c)) * k of the
medians.  The last column says whether (a) lies below (b) with ranges that do not overlap (max of a < min of b) for
both k; that is expected of every row with B >= 8.
Usage: python tools/ensemble_energy_history.py [--out FILE] [--modes float64,float32] [--members 1,8,32,256]
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
MEMBERS = (1, 8, 32, 256)
EVERY = (1, 10)
MODES = ("float64", "float32")


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
    """{variant: [us per tick of every repeat]} for variants ("rec", k), ("loop", k) and ("run", 0)."""
    dtype = torch.float64 if mode == nb.PrecisionMode.FLOAT64 else torch.float32
    pos, vel, mass = state(b, n, dtype)
    ens = nb.GalaxyEnsemble(pos.cuda(), vel.cuda(), mass.cuda(), precision_mode=mode,
                            dt=[0.01 + 0.0007 * (k % 32) for k in range(b)])

    def plain():
        ens.run(TICKS)
        ens.synchronize()

    def recorded(k):
        h = ens.run_recorded(TICKS, every=k)         # returns after the history has been copied out
        assert h.kinetic.shape == (1 + TICKS // k, b)

    def loop(k):
        curve = [(ens.get_kinetic_energy(), ens.get_potential_energy())]
        for _ in range(TICKS // k):
            ens.run(k)
            curve.append((ens.get_kinetic_energy(), ens.get_potential_energy()))
        assert len(curve) == 1 + TICKS // k

    variants = {("run", 0): plain}
    for k in EVERY:
        variants[("rec", k)] = lambda k=k: recorded(k)
        variants[("loop", k)] = lambda k=k: loop(k)
    for fn in variants.values():
        fn()
    t = time.perf_counter()
    while time.perf_counter() - t < 0.2:
        plain()
    out = {v: [] for v in variants}
    for _ in range(REPEATS):
        for v, fn in variants.items():
            out[v].append(timed(fn))
    ens.close()
    return out


def fmt(v):
    return f"{statistics.median(v):9.2f} ({min(v):8.2f} .. {max(v):8.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--members", default=",".join(str(b) for b in MEMBERS))
    args = ap.parse_args()
    modes = [nb.PrecisionMode(m) for m in args.modes.split(",")]
    members = [int(b) for b in args.members.split(",")]
    col = 32
    head = f"{'mode':8s} {'N':>5s} {'B':>4s}  {'(c) run':>{col}s}"
    for k in EVERY:
        head += f"  {f'(a) rec k={k}':>{col}s}  {f'(b) loop k={k}':>{col}s}  {f'sample k={k}':>11s}  {'b/a':>6s}"
    head += "  a below b"
    lines = [f"# us per tick of all B members together over {TICKS} ticks, median (min .. max) of {REPEATS} repeats; "
             f"{torch.cuda.get_device_name(0)}",
             "# (a) run_recorded(200, every=k); (b) 200 / k times run(k) + get_kinetic_energy() + get_potential_energy(); "
             "(c) run(200); sample = ((a) - (c)) * k, us per sample of all B members",
             head]
    failed = []

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for mode in modes:
        for n in SIZES:
            for b in members:
                r = measure(n, mode, b)
                run = r[("run", 0)]
                line = f"{mode.value:8s} {n:5d} {b:4d}  {fmt(run):>{col}s}"
                below = True
                for k in EVERY:
                    a, bb = r[("rec", k)], r[("loop", k)]
                    sample = (statistics.median(a) - statistics.median(run)) * k
                    line += (f"  {fmt(a):>{col}s}  {fmt(bb):>{col}s}  {sample:11.2f}  "
                             f"{statistics.median(bb) / statistics.median(a):6.2f}")
                    below = below and max(a) < min(bb)
                line += "  yes" if below else "  NO"
                if b >= 8 and not below:
                    failed.append(f"{mode.value} N={n} B={b}")
                lines.append(line)
                print(line, flush=True)
                flush()
    lines.append("# condition ((a) below (b), ranges not overlapping, for every row with B >= 8): "
                 + ("met by every row" if not failed else "NOT met by " + "; ".join(failed)))
    print(lines[-1], flush=True)
    flush()
    if not args.out:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
