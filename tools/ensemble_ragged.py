"""Members of different sizes in one launch per tick: what a RaggedEnsemble costs against what it replaces.

Disk galaxies (create_disk_galaxy(N, 10.0), seed 100 + N), G = 0.001, softening 0.1, dt 0.01, FLOAT32.  Two workloads:
  (a) the density sweep of density_limit_test.py: sizes 100 / 250 / 500 / 1000 / 2000, TICKS_A ticks per timing
        ragged        one RaggedEnsemble of the five sizes: run(TICKS_A), one launch per tick
        per-size      one GalaxyEnsemble of B = 1 per size: run(TICKS_A) of each issued in turn (five launch trains on five
                      streams, nothing waits in between), then one wait for each
        per-size/tick the same five ensembles, step() of each in turn, tick by tick, one wait at the end
        solo          five GalaxySimulations: run(TICKS_A) of each in turn, then one wait for each
  (b) the fp32 plane of the phase-space scan of omega_point_test.py: 50 members, 10 each of 100 / 575 / 1050 / 1525 / 2000 stars,
      as 25 pairs whose second member has positions[0, 0] one ulp up; CALLS_B calls of run_diverged(200, 1, energies=True),
      every odd member against its twin
        ragged        one RaggedEnsemble of the 50
        per-size      five GalaxyEnsembles of B = 10, the call of each in turn
A row (c), the ragged run at 256 threads per workgroup, is not here: that variant was not built.
Milliseconds per timing, median (min .. max) of REPEATS alternating repeats in one process after each contender has run
once; every repeat starts from the same state; the host clock around work that ends in a wait on the device.
Condition written down: in (a) and (b) the ragged median is not above the per-size median (the faster of its two forms in
(a)) by more than that contender's spread, max - min.
Usage: python tools/ensemble_ragged.py [--out FILE]
A step that fails ends the tool: nothing more is started on the device.
"""
import argparse
import os
import statistics
import sys
import time

REPEATS = 5
SIZES_A = [100, 250, 500, 1000, 2000]
TICKS_A = 2000
SIZES_B = [100, 575, 1050, 1525, 2000]
PER_SIZE_B = 10
TICKS_B, CALLS_B = 200, 10


def fmt(v, width=8):
    return f"{statistics.median(v):{width}.2f} ({min(v):{width}.2f} .. {max(v):{width}.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import nbody_cosmological_simulation_amd as nb
    from nbody_cosmological_simulation_amd.galaxy import create_disk_galaxy
    lines = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    F32 = nb.PrecisionMode.FLOAT32
    kw = dict(precision_mode=F32, G=0.001, softening=0.1, dt=0.01)
    galaxy = {n: tuple(t.float().cuda() for t in create_disk_galaxy(n, 10.0, device="cpu", seed=100 + n))
              for n in sorted(set(SIZES_A + SIZES_B))}

    def timed(variants, resets):
        times = {v: [] for v in variants}
        for rep in range(REPEATS + 1):
            for v, fn in variants.items():
                for r in resets[v]:
                    r()
                t = time.perf_counter()
                fn()
                if rep:
                    times[v].append((time.perf_counter() - t) * 1e3)
        return times

    def resetter(e):
        """Puts an ensemble back to the state it has now."""
        p, v, a = e.positions, e.velocities, e.accelerations

        def reset():
            e.set_state(positions=p, velocities=v)
            e.set_accelerations(a)
            e.synchronize()
        return reset

    def verdict(row, ragged, contender, name):
        spread = max(contender) - min(contender)
        r, c = statistics.median(ragged), statistics.median(contender)
        ok = r <= c + spread
        emit(f"({row}) ragged {r:.2f} ms against {name} {c:.2f} ms (spread {spread:.2f} ms): {c / r:.2f}x -- condition "
             f"(ragged <= contender + its spread): {'met' if ok else 'NOT MET'}")

    # ---- (a) the density sweep -------------------------------------------------------------------------------------------
    ragged = nb.RaggedEnsemble(*([galaxy[n][k] for n in SIZES_A] for k in range(3)), **kw)
    assert ragged.force_kernel_name() == "ens_step_ragged_kernel"
    per_size = [nb.GalaxyEnsemble(*(t.unsqueeze(0) for t in galaxy[n]), **kw) for n in SIZES_A]
    assert all(e.force_kernel_name() == "ens_step_kernel" for e in per_size)

    def run_ragged():
        ragged.run(TICKS_A)
        ragged.synchronize()

    def run_per_size():
        for e in per_size:
            e.run(TICKS_A)
        for e in per_size:
            e.synchronize()

    def step_per_size():
        for _ in range(TICKS_A):
            for e in per_size:
                e.step()
        for e in per_size:
            e.synchronize()

    def run_solo():
        sims = [nb.GalaxySimulation(*(t.clone() for t in galaxy[n]), **kw) for n in SIZES_A]
        for s in sims:
            s.step()                                     # (the first step leaves the constructor's tiled evaluation behind)
            s.synchronize()
        t = time.perf_counter()
        for s in sims:
            s.run(TICKS_A)
        for s in sims:
            s.synchronize()
        solo_ms.append((time.perf_counter() - t) * 1e3)
        assert all(s.force_kernel_name() == "small_step_kernel" for s in sims)
        for s in sims:
            s.close()

    solo_ms = []
    variants = {"ragged": run_ragged, "per-size": run_per_size, "per-size/tick": step_per_size, "solo": run_solo}
    resets = {"ragged": [resetter(ragged)], "per-size": [resetter(e) for e in per_size], "solo": []}
    resets["per-size/tick"] = resets["per-size"]
    ta = timed(variants, resets)
    ta["solo"] = solo_ms[1:]                             # its own clock: the constructors are not the workload
    emit(f"# RaggedEnsemble against what it replaces, FLOAT32: ms per timing, median (min .. max) of {REPEATS} alternating "
         f"repeats; {torch.cuda.get_device_name(0)}")
    emit(f"# (a) density sweep, sizes {SIZES_A}, {TICKS_A} ticks per timing; ragged work list: "
         f"{sum(-(-n // 8) for n in SIZES_A)} workgroups per tick")
    names = {"ragged": "ragged: one RaggedEnsemble, run()", "per-size": "per-size: five GalaxyEnsembles of B = 1, run() in turn",
             "per-size/tick": "per-size/tick: the same, step() in turn", "solo": "solo: five GalaxySimulations, run() in turn"}
    for v in variants:
        emit(f"{names[v]:58s} {fmt(ta[v]):>34s}   {statistics.median(ta[v]) / TICKS_A * 1e3:7.2f} us per tick")
    best = min(("per-size", "per-size/tick"), key=lambda v: statistics.median(ta[v]))
    verdict("a", ta["ragged"], ta[best], best)
    ragged.close()
    for e in per_size:
        e.close()

    # ---- (b) the phase-space scan's fp32 plane -----------------------------------------------------------------------------
    def twins(n):
        """PER_SIZE_B members of n stars: pairs, the second with positions[0, 0] one ulp up."""
        p, v, m = galaxy[n]
        q = p.clone()
        q[0, 0] = torch.nextafter(q[0, 0], torch.tensor(float("inf"), device=q.device))
        return [(q if b % 2 else p, v, m) for b in range(PER_SIZE_B)]

    members = [mem for n in SIZES_B for mem in twins(n)]
    B = len(members)
    base_all = [b - b % 2 for b in range(B)]
    base_one = [b - b % 2 for b in range(PER_SIZE_B)]
    ragged = nb.RaggedEnsemble(*([mem[k] for mem in members] for k in range(3)), **kw)
    per_size = [nb.GalaxyEnsemble(*(torch.stack([mem[k] for mem in twins(n)]) for k in range(3)), **kw) for n in SIZES_B]
    seen = {}

    def diverged_ragged():
        for _ in range(CALLS_B):
            h = ragged.run_diverged(TICKS_B, 1, base_all, energies=True)
        seen["ragged"] = np.asarray(h.max_position[-1].tolist())

    def diverged_per_size():
        last = []
        for _ in range(CALLS_B):
            last = [e.run_diverged(TICKS_B, 1, base_one, energies=True) for e in per_size]
        seen["per-size"] = np.concatenate([np.asarray(h.max_position[-1].tolist()) for h in last])

    variants = {"ragged": diverged_ragged, "per-size": diverged_per_size}
    resets = {"ragged": [resetter(ragged)], "per-size": [resetter(e) for e in per_size]}
    tb = timed(variants, resets)
    emit(f"# (b) phase-space plane: {B} members, {PER_SIZE_B} each of {SIZES_B}, {CALLS_B} calls of run_diverged({TICKS_B}, 1, "
         f"energies=True) per timing; ragged work list: {PER_SIZE_B * sum(-(-n // 8) for n in SIZES_B)} workgroups per tick")
    names = {"ragged": "ragged: one RaggedEnsemble of 50", "per-size": "per-size: five GalaxyEnsembles of B = 10, in turn"}
    for v in variants:
        emit(f"{names[v]:58s} {fmt(tb[v]):>34s}   {statistics.median(tb[v]) / (TICKS_B * CALLS_B) * 1e3:7.2f} us per tick")
    verdict("b", tb["ragged"], tb["per-size"], "per-size")
    emit(f"# last sample of the last call, max |d position|: the two agree bit for bit: "
         f"{bool(np.array_equal(seen['ragged'], seen['per-size'], equal_nan=True))}; largest {np.nanmax(seen['ragged']):.3g}")
    emit("# (c) the ragged run at 256 threads per workgroup: not built, not measured")
    ragged.close()
    for e in per_size:
        e.close()


if __name__ == "__main__":
    main()
