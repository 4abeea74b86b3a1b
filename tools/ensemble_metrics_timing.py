"""Cost of the galaxy diagnostics of a GalaxyEnsemble: metrics() against the loop it replaces.

For float64 and float32 state, N in {256, 1024, 4096} (float32: 3072, the ensemble's limit for that dtype, in place of
4096) and B in {1, 8, 64, 512} members, microseconds per evaluation of ALL B members of
  batched  (a) ens.metrics(): one launch, one copy-out (20 bins, every member's own maximum radius, 90th percentile)
  loop     (b) the only route without it: the state downloaded once (device tensors), then
               metrics.native_metrics(pos[b], vel[b], mass[b], G=G[b]) member by member -- per member two native calls
               (the maximum radius first, then seven kernels and two radix sorts), each ending in a blocking read-back
Each figure is the median of REPEATS timed regions with the min .. max beside it.  A region is a host clock around K
back-to-back evaluations that end in a device synchronise (metrics() and native_metrics() return only after their results
have been copied out); K is chosen per variant from a pilot run so that a region lasts about 20 ms.  The variants alternate
inside one repeat, after every variant has run three times as warm-up.  The last column says whether (a) lies below (b)
with ranges that do not overlap (max of a < min of b); that is expected of every row with B >= 8.
Usage: python tools/ensemble_metrics_timing.py [--out FILE] [--dtypes float64,float32] [--members 1,8,64,512]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nbody_cosmological_simulation_amd as nb  # noqa: E402
from nbody_cosmological_simulation_amd import metrics as M  # noqa: E402

REPEATS = 9
REGION_S = 0.02
SIZES = {"float64": (256, 1024, 4096), "float32": (256, 1024, 3072)}
MEMBERS = (1, 8, 64, 512)
DTYPES = ("float64", "float32")
NUM_BINS = 20


def state(b, n, dtype):
    g = torch.Generator().manual_seed(7 + n)
    pos = torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 5
    vel = torch.randn(b, n, 2, generator=g, dtype=torch.float64) * 0.05
    mass = 0.5 + torch.rand(b, n, generator=g, dtype=torch.float64)
    return pos.to(dtype), vel.to(dtype), mass.to(dtype)


def measure(n, dtype_name, b):
    """{variant: [us per evaluation of all members, one figure per repeat]} for "batched" and "loop"."""
    dtype = getattr(torch, dtype_name)
    mode = nb.PrecisionMode.FLOAT64 if dtype == torch.float64 else nb.PrecisionMode.FLOAT32
    pos, vel, mass = state(b, n, dtype)
    G = [0.001 + 0.0001 * (k % 16) for k in range(b)]
    ens = nb.GalaxyEnsemble(pos.cuda(), vel.cuda(), mass.cuda(), precision_mode=mode, G=G)
    check = {}

    def batched():
        m = ens.metrics(num_bins=NUM_BINS)
        check["batched"] = (m.num_stars_per_bin[b - 1].tolist(), float(m.galaxy_radius[b - 1]))

    def loop():
        p, v, ms = ens.positions, ens.velocities, ens.masses
        out = [M.native_metrics(p[k], v[k], ms[k], G=G[k], num_bins=NUM_BINS) for k in range(b)]
        check["loop"] = (out[-1]["count"], out[-1]["r_percentile"])

    variants = {"batched": batched, "loop": loop}
    reps = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, min(200, int(REGION_S / max(time.perf_counter() - t, 1e-6))))
    assert check["batched"] == check["loop"], (check, "the two routes disagree on the last member's counts or radius")
    out = {name: [] for name in variants}
    for _ in range(REPEATS):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t) / reps[name] * 1e6)
    ens.close()
    return out


def fmt(v):
    return f"{statistics.median(v):11.1f} ({min(v):10.1f} .. {max(v):10.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--dtypes", default=",".join(DTYPES))
    ap.add_argument("--members", default=",".join(str(b) for b in MEMBERS))
    args = ap.parse_args()
    members = [int(b) for b in args.members.split(",")]
    col = 38
    lines = [f"# us per evaluation of the diagnostics of all B members ({NUM_BINS} bins, own maximum radius), median (min .. max) of "
             f"{REPEATS} timed regions of about {REGION_S * 1e3:.0f} ms; {torch.cuda.get_device_name(0)}",
             "# (a) ens.metrics(); (b) state download + metrics.native_metrics() member by member; float32 runs N = 3072 (its "
             "limit) where float64 runs 4096",
             f"{'dtype':8s} {'N':>5s} {'B':>4s}  {'(a) batched':>{col}s}  {'(b) loop':>{col}s}  {'b/a':>7s}  a below b"]
    failed = []

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    for dtype_name in args.dtypes.split(","):
        for n in SIZES[dtype_name]:
            for b in members:
                r = measure(n, dtype_name, b)
                a, bb = r["batched"], r["loop"]
                below = max(a) < min(bb)
                if b >= 8 and not below:
                    failed.append(f"{dtype_name} N={n} B={b}")
                lines.append(f"{dtype_name:8s} {n:5d} {b:4d}  {fmt(a):>{col}s}  {fmt(bb):>{col}s}  "
                             f"{statistics.median(bb) / statistics.median(a):7.1f}  {'yes' if below else 'NO'}")
                print(lines[-1], flush=True)
                flush()
    lines.append("# condition ((a) below (b), ranges not overlapping, for every row with B >= 8): "
                 + ("met by every row" if not failed else "NOT met by " + "; ".join(failed)))
    print(lines[-1], flush=True)
    flush()
    if not args.out:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
