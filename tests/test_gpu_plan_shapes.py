"""Every force-kernel variant and work-plan shape against the oracle (cases: plan_shapes.CASES).

Each case first asserts the shape it claims to cover -- the planner's keys for the device's CU count and, after the
evaluation, force_kernel_name() -- so a retune that moves a size off its shape fails here instead of quietly
dropping the shape from the suite.  Then, on the GPU:
  probes   all masses 0 but one (mass 1) at a few places: lanes 0 / 63 of a tile, the first tile, a middle super-row,
           the tiles on either side of it, the ragged last tile.  Every row i != k then holds exactly the one pair
           (i, k) and row k holds 0, so every row is compared with the oracle relative to ITS OWN value: a dropped,
           doubled or mis-rotated pair shows at any N (the array-max bar of the dense checks does not see one far
           pair at N >~ 32k).  fp64 also runs a three-probe set with masses 1, 2^-24, 2^-48.
  dense    a clustered core with a distant halo, mixed masses and its equal-mass twin (the UNIFORM kernels) at the
           suite's bars (fp64 1e-13, fp32 family 2e-6; grid modes: distance bins bit-identical, forces within one
           force-grid step); fp64 single-rank cases also the potential energy and three leapfrog steps vs OracleSim.
Multi-rank plans run as comm-less shards (NB_SYM=2) whose partial forces are summed and compared with the oracle.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import plan_shapes as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

MODE_CODES = {"float64": 0, "float32": 1, "bfloat16": 2, "float16": 3, "int8_sim": 4, "int4_sim": 5, "custom": 6}
# one pair, row by row: fp64 a few ulp (measured on MI355X: <= 1.1e-15); fp32 family a few fp32 ulp, 2^-23 = 1.19e-7
# (measured: <= 6.6e-7 -- the kernels' rsqrt-based 1 / r^3 against the reference's 1 / (r2 sqrt(r2)), both rounded)
PROBE_TOL_F64 = 1e-14
PROBE_TOL_F32 = 1e-6
FULL_ORACLE_MAX = 60000     # above: the dense check compares row samples


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def inputs(n, dim, seed, f64, uniform=False):
    """Clustered core (80 %) and a distant halo, shuffled through the tiles; mixed masses or all 0.7."""
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((n, dim)) * 0.5
    halo = rng.random(n) < 0.2
    pos[halo] *= 40.0
    vel = rng.standard_normal((n, dim)) * 0.05
    mass = np.full(n, 0.7) if uniform else 0.5 + rng.random(n)
    dt = np.float64 if f64 else np.float32
    return pos.astype(dt), vel.astype(dt), mass.astype(dt)


def probe_places(n, tile):
    """Lane 0 and 63 of the first tile, lane 0 / 63 of the last 64-slot of a middle super-row's tile, the tiles on
    either side of it, the first particle of the ragged last tile and the last particle."""
    T = -(-n // tile)
    mid = min(T - 1, 4 * ((T // 4) // 2) + 1)
    ks = [0, 63, mid * tile + tile - 64, mid * tile + tile - 1, (mid - 1) * tile + 17, (mid + 1) * tile + 40,
          (T - 1) * tile, n - 1]
    return sorted({k for k in ks if 0 <= k < n})


def rowwise(acc, ref, tol, what):
    """Every row relative to its own reference value; rows without a pair must be exactly 0."""
    a = np.asarray(acc, np.float64)
    r = np.asarray(ref, np.float64)
    scale = np.abs(r).max(axis=1)
    err = np.abs(a - r).max(axis=1)
    zero = scale == 0
    assert np.all(err[zero] == 0), f"{what}: rows {np.flatnonzero(zero & (err > 0))[:8]} should be 0"
    rel = np.where(zero, 0.0, err / np.where(zero, 1.0, scale))
    worst = int(rel.argmax())
    assert rel[worst] <= tol, f"{what}: row {worst} relative error {rel[worst]:.3e} > {tol:.1e}"
    return float(rel[worst])


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


class Runner:
    """Evaluates one case's inputs on the GPU (one handle, or the sum of its comm-less shards)."""

    def __init__(self, nb, case):
        self.nb = nb
        self.cid, self.n, self.dim, self.state, self.mode, self.world, self.env, self.keys, self.kernel = case

    def sims(self, pos, vel, mass):
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        mode = self.nb.PrecisionMode(self.mode)
        if self.world == 1:
            return [self.nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=mode)]
        return [self.nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=mode, shard=(r, self.world))
                for r in range(self.world)]

    def forces(self, pos, vel, mass, pe=False):
        sims = self.sims(pos, vel, mass)
        acc = 0
        pes = 0.0
        for s in sims:
            assert s.force_kernel_name() == self.kernel, (self.cid, s.force_kernel_name())
            acc = acc + s.accelerations.numpy().astype(np.float64)
            if pe:
                pes += s.get_potential_energy()
            s.close()
        return acc, pes


def oracle_probe(pos, mass, mode, k):
    """The oracle's forces of source k alone on every target (its own operation order, sources [k, k + 1))."""
    from oracle import oracle as O
    if mode == "float64":
        return O.accelerations_f64_fast(pos, mass, j_range=(k, k + 1))
    if mode == "float32" and pos.dtype == np.float32:
        return O.accelerations_f32_fast(pos, mass, j_range=(k, k + 1))
    return O.accelerations(pos, mass, mode, j_range=(k, k + 1), force_quant=False)


def check_probes(run, pos, vel, tile):
    f64 = run.mode == "float64"
    tol = PROBE_TOL_F64 if f64 else PROBE_TOL_F32
    worst = 0.0
    for k in probe_places(run.n, tile):
        mass = np.zeros(run.n, pos.dtype)
        mass[k] = 1
        acc, _ = run.forces(pos, vel, mass)
        worst = max(worst, rowwise(acc, oracle_probe(pos, mass, run.mode, k), tol, f"{run.cid} probe k={k}"))
    if f64:
        # three pairs per row told apart by their masses
        ks = probe_places(run.n, tile)
        trio = [ks[1], ks[len(ks) // 2], ks[-1]]
        if len(set(trio)) == 3:
            mass = np.zeros(run.n, pos.dtype)
            ref = 0
            for k, m in zip(trio, (1.0, 2.0 ** -24, 2.0 ** -48)):
                mass[k] = m
                single = np.zeros(run.n, pos.dtype)
                single[k] = m
                ref = ref + oracle_probe(pos, single, run.mode, k)
            worst = max(worst, rowwise(run.forces(pos, vel, mass)[0], ref, tol, f"{run.cid} probe trio {trio}"))
    print(f"{run.cid}: probes worst row relative error {worst:.2e}")


def check_dense(run, uniform):
    from oracle import oracle as O
    f64 = run.state == "float64"
    pos, vel, mass = inputs(run.n, run.dim, run.n + run.dim + uniform, f64, uniform)
    grid = run.mode in ("int8_sim", "int4_sim", "custom")
    single_fp64 = f64 and run.mode == "float64" and run.world == 1
    acc, pe = run.forces(pos, vel, mass, pe=run.mode == "float64" and run.n <= FULL_ORACLE_MAX)
    tag = f"{run.cid} dense{' uniform' if uniform else ''}"
    if grid:
        sims = run.sims(pos, vel, mass)
        assert run.world == 1 and run.n <= 12000, "grid cases: one rank, sizes the row oracle scans quickly"
        s = sims[0]
        dbg = s.quant_debug()
        levels = {"int8_sim": 256, "int4_sim": 16}.get(run.mode)
        for i0 in (0, run.n // 2 - 300, run.n - 600):
            ref, rdbg = O.accelerations_rows(pos, mass, run.mode, i0, i0 + 600, bins=True)
            assert np.float32(dbg["lmin"]) == np.float32(rdbg["lmin"]) and np.float32(dbg["lmax"]) == np.float32(rdbg["lmax"])
            assert np.array_equal(s.quant_bins_rows(i0, i0 + 600), rdbg["d2bins"].astype(np.int16)), f"{tag}: bins"
            if levels:
                fmin, fmax = np.float32(dbg["fmin"]), np.float32(dbg["fmax"])
                r32 = ref.astype(np.float32)
                k = np.rint((r32 - fmin) / (fmax - fmin) * np.float32(levels - 1))
                snapped = (k / np.float32(levels - 1) * (fmax - fmin) + fmin).astype(np.float64)
                step = float(fmax - fmin) / (levels - 1)
                assert np.abs(acc[i0:i0 + 600] - snapped).max() <= 1.01 * step, f"{tag}: more than one force-grid step"
            else:
                assert np.abs(acc[i0:i0 + 600] - ref).max() / np.abs(acc).max() < 2e-6, tag
        s.close()
        return
    tol = 1e-13 if run.mode == "float64" else 2e-6
    if run.n <= FULL_ORACLE_MAX:
        if run.mode == "float64":
            ref = O.accelerations_f64_fast(pos, mass)
        elif run.mode == "float32" and not f64:
            ref = O.accelerations_f32_fast(pos, mass)
        else:
            ref = O.accelerations(pos, mass, run.mode)
        assert relerr(acc, ref) < tol, (tag, relerr(acc, ref))
    else:
        rows = 512 if run.n > 300000 else 2048
        for i0 in (0, run.n // 2 - rows // 2, run.n - rows):
            ref, _ = O.accelerations_rows(pos, mass, run.mode, i0, i0 + rows)
            assert relerr(acc[i0:i0 + rows], ref) < tol, (tag, i0, relerr(acc[i0:i0 + rows], ref))
    if run.mode == "float64" and run.n <= FULL_ORACLE_MAX:
        pe_ref = O.potential_energy_f64_fast(pos, mass)
        assert abs(pe - pe_ref) <= 1e-12 * abs(pe_ref), (tag, pe, pe_ref)
    if single_fp64 and run.n <= 16384:
        sim = run.sims(pos, vel, mass)[0]
        ref = O.OracleSim(pos, vel, mass, "float64")
        sim.run(3)
        ref.run(3)
        assert relerr(sim.positions.numpy(), ref.positions) < 1e-13, tag
        assert relerr(sim.velocities.numpy(), ref.velocities) < 1e-12, tag
        sim.close()


@pytest.mark.parametrize("case", S.CASES, ids=[c[0] for c in S.CASES])
def test_plan_shape_vs_oracle(nb, cus, monkeypatch, case):
    run = Runner(nb, case)
    for k, v in run.env.items():
        monkeypatch.setenv(k, v)
    if run.world > 1:
        monkeypatch.setenv("NB_SYM", "2")
    f64 = run.state == "float64"
    # the shape this case claims, for this device
    got = S.rank_keys(run.n, run.dim, run.world, f64, MODE_CODES[run.mode], cus=cus, no_comm=run.world > 1)
    assert got == run.keys, f"{run.cid}: the planner moved this case off its shape: {sorted(got, key=str)}"
    p = S.plan(run.n, run.dim, 0, run.world, f64, MODE_CODES[run.mode], cus=cus, no_comm=run.world > 1, work=False)
    tile = p["tile_b"] if p["enabled"] else 256
    if run.mode not in ("int8_sim", "int4_sim", "custom"):
        pos, vel, _ = inputs(run.n, run.dim, run.n + 7, f64)
        check_probes(run, pos, vel, tile)
    for uniform in (False, True):
        check_dense(run, uniform)


@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16"])
def test_fp64_state_under_cast_modes_onesided(nb, cus, mode):
    """fp64 tensors under a cast mode take the one-sided fp64 kernel with two targets per thread (the QHOOK variants
    are compiled for R = 2 only): probes and the dense case against the oracle at N = 12 011."""
    from oracle import oracle as O
    n, dim = 12011, 2
    case = (f"cast-{mode}", n, dim, "float64", mode, 1, {}, {("onesided", 2, dim, True)}, "force_f64_kernel")
    run = Runner(nb, case)
    pos, vel, mass = inputs(n, dim, 5, True)
    worst = 0.0
    for k in probe_places(n, 512):
        m = np.zeros(n)
        m[k] = 1
        worst = max(worst, rowwise(run.forces(pos, vel, m)[0], oracle_probe(pos, m, mode, k), PROBE_TOL_F32, f"{mode} k={k}"))
    print(f"fp64 state, {mode}: probes worst row relative error {worst:.2e}")
    for uniform in (False, True):
        pos, vel, mass = inputs(n, dim, 6 + uniform, True, uniform)
        assert relerr(run.forces(pos, vel, mass)[0], O.accelerations(pos, mass, mode)) < 2e-6


@pytest.mark.parametrize("lanes", [16, 32, 64])
@pytest.mark.parametrize("state", ["float64", "float32"])
def test_small_kernel_lanes_vs_oracle(nb, monkeypatch, lanes, state):
    """The one-launch small-system step with 16 / 32 / 64 lanes per target (NB_SMALL_LANES): probes through the
    velocities of one step from rest (v1 = dt / 2 (a0 + a1), one pair per row) and a dense three-step run."""
    monkeypatch.setenv("NB_SMALL_LANES", str(lanes))
    _small_step_checks(nb, state, 1500, 2)
    _small_step_checks(nb, state, 1001, 3)


def _small_step_checks(nb, state, n, dim, expect_small=True):
    from oracle import oracle as O
    f64 = state == "float64"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    pos, vel, mass = inputs(n, dim, n + dim, f64)
    zero = np.zeros_like(vel)
    tol = PROBE_TOL_F64 if f64 else 4 * PROBE_TOL_F32
    for k in probe_places(n, 64):
        m = np.zeros(n, pos.dtype)
        m[k] = 1
        sim = nb.GalaxySimulation(T(pos), T(zero), T(m), precision_mode=nb.PrecisionMode(state))
        sim.step()
        assert (sim.force_kernel_name() == "small_step_kernel") == expect_small, sim.force_kernel_name()
        ref = O.OracleSim(pos, zero, m, state)
        ref.step()
        rowwise(sim.velocities.numpy(), ref.velocities, tol, f"small step {state} n={n} k={k}")
        sim.close()
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(state))
    ref = O.OracleSim(pos, vel, mass, state)
    sim.run(3)
    ref.run(3)
    assert (sim.force_kernel_name() == "small_step_kernel") == expect_small
    assert relerr(sim.positions.numpy(), ref.positions) < (1e-13 if f64 else 5e-6)
    sim.close()


def test_no_smalln_keeps_the_tiled_step(nb, monkeypatch):
    monkeypatch.setenv("NB_NO_SMALLN", "1")
    _small_step_checks(nb, "float64", 1500, 2, expect_small=False)
    _small_step_checks(nb, "float32", 1001, 3, expect_small=False)


_SMALL_BLOCK_CHILD = r"""
import os, sys
sys.path.insert(0, os.environ["NB_ROOT"]); sys.path.insert(0, os.path.join(os.environ["NB_ROOT"], "tests"))
import nbody_cosmological_simulation_amd as nb
import test_gpu_plan_shapes as M
for state in ("float64", "float32"):
    for n, dim in ((1500, 2), (2500, 3), (3001, 2)):
        M._small_step_checks(nb, state, n, dim)
print("SMALL-BLOCK-OK")
"""


@pytest.mark.parametrize("block", [256, 512])
def test_small_kernel_block_sizes_in_a_child(nb, block):
    """NB_SMALL_BLOCK is read once per process: each workgroup size in a fresh child, at sizes where the default
    picks the other one (256 threads for 2048 < N <= 3072, 512 elsewhere)."""
    env = dict(os.environ, NB_ROOT=ROOT, NB_SMALL_BLOCK=str(block))
    res = subprocess.run([sys.executable, "-c", _SMALL_BLOCK_CHILD], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "SMALL-BLOCK-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
