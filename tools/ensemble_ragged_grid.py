"""Grid-mode members of different sizes in one launch per tick: what a RaggedQuantizedEnsemble costs against what it
replaces.

Workload: the grid plane of the phase-space scan of omega_point_test.py:595-766 -- 50 members made of the sizes 100 / 575 /
1050 / 1525 / 2000 x five velocity multipliers x the a / b pair (the second member of a pair has positions[0, 0] one ulp
up), disk galaxies (create_disk_galaxy(N, 10.0), seed 100 + N), G = 0.001, softening 0.1, dt 0.01, CUSTOM at 256 levels
and again at 16 (the scan's "int8" / "int4" points: a grid on r^2, forces not snapped).  The call is
run_diverged(200, 1, energies=True), every odd member against its twin.
    ragged        one RaggedQuantizedEnsemble of the 50
    per-size      five QuantizedEnsembles of B = 10, the call of each in turn
    solo          fifty GalaxySimulations stepped tick by tick, the divergence of every pair read back after every tick with
                  (a.positions - b.positions).abs().max().item(), as the reference's loop does
Milliseconds per timing, median (min .. max) of REPEATS alternating repeats in one process after each contender has run
once; every repeat starts from the same state; the host clock around work that ends in a wait on the device.  No ratio is
set as a condition: the file records what was measured.
Usage: python tools/ensemble_ragged_grid.py [--out FILE]
A step that fails ends the tool: nothing more is started on the device.
"""
import argparse
import os
import statistics
import sys
import time

REPEATS = 5
SIZES = [100, 575, 1050, 1525, 2000]
MULTIPLIERS = [0.5, 0.75, 1.0, 1.25, 1.5]
TICKS = 200
LEVELS = [256, 16]


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

    galaxy = {n: tuple(t.float().cuda() for t in create_disk_galaxy(n, 10.0, device="cpu", seed=100 + n)) for n in SIZES}

    def plane(n):
        """The ten members of n stars: per multiplier the pair a / b."""
        p, v, m = galaxy[n]
        q = p.clone()
        q[0, 0] = torch.nextafter(q[0, 0], torch.tensor(float("inf"), device=q.device))
        return [(q if twin else p, v * mult, m) for mult in MULTIPLIERS for twin in (0, 1)]

    members = [mem for n in SIZES for mem in plane(n)]
    B, per = len(members), 2 * len(MULTIPLIERS)
    base_all = [b - b % 2 for b in range(B)]
    base_one = [b - b % 2 for b in range(per)]

    def resetter(e):
        """Puts an ensemble back to the state it has now."""
        p, v, a = e.positions, e.velocities, e.accelerations

        def reset():
            e.set_state(positions=p, velocities=v)
            e.set_accelerations(a)
            e.synchronize()
        return reset

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

    emit(f"# RaggedQuantizedEnsemble against what it replaces, CUSTOM grids: ms per call of run_diverged({TICKS}, 1, "
         f"energies=True), median (min .. max) of {REPEATS} alternating repeats; {torch.cuda.get_device_name(0)}")
    emit(f"# {B} members: {per} each of {SIZES} (multipliers {MULTIPLIERS} x the a / b pair); ragged work list: "
         f"{per * sum(-(-n // 8) for n in SIZES)} workgroups per tick")
    for levels in LEVELS:
        kw = dict(precision_mode=nb.PrecisionMode.CUSTOM, custom_levels=levels, G=0.001, softening=0.1, dt=0.01)
        ragged = nb.RaggedQuantizedEnsemble(*([mem[k] for mem in members] for k in range(3)), **kw)
        assert ragged.force_kernel_name() == "ens_grid_step_ragged_kernel"
        per_size = [nb.QuantizedEnsemble(*(torch.stack([mem[k] for mem in plane(n)]) for k in range(3)), **kw) for n in SIZES]
        assert all(e.force_kernel_name() == "ens_grid_step_kernel" for e in per_size)
        seen, solo_ms = {}, []

        def diverged_ragged():
            h = ragged.run_diverged(TICKS, 1, base_all, energies=True)
            seen["ragged"] = np.asarray(h.max_position[-1].tolist())

        def diverged_per_size():
            last = [e.run_diverged(TICKS, 1, base_one, energies=True) for e in per_size]
            seen["per-size"] = np.concatenate([np.asarray(h.max_position[-1].tolist()) for h in last])

        def diverged_solo():
            sims = [nb.GalaxySimulation(*(t.clone() for t in mem), **kw) for mem in members]
            for s in sims:
                s.step()                                 # (the first step leaves the constructor's tiled evaluation behind)
                s.synchronize()
            t = time.perf_counter()
            last = [0.0] * B
            for _ in range(TICKS):
                for s in sims:
                    s.step()
                for b in range(1, B, 2):
                    last[b] = (sims[b].positions - sims[b - 1].positions).abs().max().item()
            solo_ms.append((time.perf_counter() - t) * 1e3)
            assert all(s.force_kernel_name() == "small_step_kernel" for s in sims)
            for s in sims:
                s.close()

        variants = {"ragged": diverged_ragged, "per-size": diverged_per_size, "solo": diverged_solo}
        resets = {"ragged": [resetter(ragged)], "per-size": [resetter(e) for e in per_size], "solo": []}
        tb = timed(variants, resets)
        tb["solo"] = solo_ms[1:]                         # its own clock: the constructors are not the workload
        emit(f"# CUSTOM, {levels} levels")
        names = {"ragged": "ragged: one RaggedQuantizedEnsemble of 50", "per-size": "per-size: five QuantizedEnsembles of B = 10, in turn",
                 "solo": "solo: fifty GalaxySimulations, step() and .item() per tick"}
        for v in variants:
            emit(f"{names[v]:60s} {fmt(tb[v]):>34s}   {statistics.median(tb[v]) / TICKS * 1e3:8.2f} us per tick")
        r = statistics.median(tb["ragged"])
        emit(f"ragged against per-size: {statistics.median(tb['per-size']) / r:.2f}x; against solo: "
             f"{statistics.median(tb['solo']) / r:.2f}x")
        emit(f"# last sample, max |d position|: ragged and per-size agree bit for bit: "
             f"{bool(np.array_equal(seen['ragged'], seen['per-size'], equal_nan=True))}; largest {np.nanmax(seen['ragged']):.3g}")
        ragged.close()
        for e in per_size:
            e.close()


if __name__ == "__main__":
    main()
