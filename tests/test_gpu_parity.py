"""GPU parity tests: the HIP path (through the C-ABI / ctypes shim) against
  (a) golden vectors produced by running the reference (tests/golden), and
  (b) the CPU oracle (oracle/) on the same seeded inputs.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q

Tolerances
  FLOAT64 mode : north_star bar -- 1e-10 relative (to the array's max magnitude) on
                 positions / velocities / energies; single evaluations are asserted at 1e-13.
  fp32 family  : 2e-6 relative on a single evaluation (fp32 rounding of ~15 operations per
                 pair; the reference's own torch kernels differ from a correctly rounded
                 evaluation by up to 3e-7, tests/test_oracle_golden.py).
  grid modes   : distance-bin indices and lmin/lmax bit-identical; force bins: flip count
                 reported and bounded (they depend on fp32 summation order).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

MODES = ["float64", "float32", "bfloat16", "float16", "int8_sim", "int4_sim", "custom"]
GRID = ["int8_sim", "int4_sim", "custom"]
G1 = ["g1_n64_d2_e0.1.npz", "g1_n257_d2_e0.05.npz", "g1_n64_d3_e0.01.npz", "g1_n257_d3_e0.1.npz"]


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def mk(nb, g, mode, **kw):
    return nb.GalaxySimulation(T(g["pos"]), T(g["vel"]), T(g["mass"]),
                               precision_mode=nb.PrecisionMode(mode), G=float(g["G"]),
                               softening=float(g["eps"]), dt=float(g["dt"]), **kw)


# --------------------------------------------------------------------------- single evaluation
@pytest.mark.parametrize("fname", G1)
@pytest.mark.parametrize("mode", MODES)
def test_single_evaluation_vs_reference(nb, fname, mode):
    g = load_golden(fname)
    sim = mk(nb, g, mode)
    acc = sim.accelerations.numpy()
    ref = g[f"{mode}/acc0"]
    assert acc.dtype == ref.dtype
    if mode in GRID:
        dbg = sim.quant_debug(bins=True)
        assert np.float32(dbg["lmin"]) == np.float32(g[f"{mode}/lmin"])
        assert np.float32(dbg["lmax"]) == np.float32(g[f"{mode}/lmax"])
        assert np.array_equal(dbg["d2bins"], g[f"{mode}/d2bins"]), "distance bins must be bit-identical"
    if mode in ("int8_sim", "int4_sim"):
        flips = int((dbg["fbins"] != g[f"{mode}/fbins"]).sum())
        print(f"{fname} {mode}: force-bin flips {flips}/{ref.size}")
        assert flips <= 2
        assert abs(dbg["fmin"] - float(g[f"{mode}/fmin"])) <= 2e-6 * abs(float(g[f"{mode}/fmin"]))
        assert abs(dbg["fmax"] - float(g[f"{mode}/fmax"])) <= 2e-6 * abs(float(g[f"{mode}/fmax"]))
        if flips == 0:
            assert relerr(acc, ref) < 2e-6
    else:
        assert relerr(acc, ref) < (1e-13 if mode == "float64" else 2e-6)


@pytest.mark.parametrize("fname", G1)
@pytest.mark.parametrize("mode", MODES)
def test_steps_and_energies_vs_reference(nb, fname, mode):
    g = load_golden(fname)
    sim = mk(nb, g, mode)
    assert abs(sim.get_potential_energy() - float(g[f"{mode}/pe0"])) <= 2e-6 * abs(float(g[f"{mode}/pe0"]))
    assert abs(sim.get_kinetic_energy() - float(g[f"{mode}/ke0"])) <= 2e-6 * abs(float(g[f"{mode}/ke0"]))
    sim.step()
    tol = 1e-13 if mode == "float64" else 2e-6
    assert sim.positions.numpy().dtype == g[f"{mode}/pos1"].dtype
    assert sim.velocities.numpy().dtype == g[f"{mode}/vel1"].dtype
    assert relerr(sim.positions.numpy(), g[f"{mode}/pos1"]) < tol
    assert relerr(sim.velocities.numpy(), g[f"{mode}/vel1"]) < tol
    for _ in range(9):
        sim.step()
    t10 = 1e-12 if mode == "float64" else (1e-5 if mode not in ("int8_sim", "int4_sim") else 2e-3)
    assert relerr(sim.positions.numpy(), g[f"{mode}/pos10"]) < t10
    assert relerr(sim.velocities.numpy(), g[f"{mode}/vel10"]) < t10 * 50
    if mode == "float64":
        ke, pe = g["float64/e10"]
        assert abs(sim.get_kinetic_energy() - ke) <= 1e-12 * abs(ke)
        assert abs(sim.get_potential_energy() - pe) <= 1e-12 * abs(pe)


@pytest.mark.parametrize("L", [4, 64, 1000])
def test_custom_levels_native(nb, L):
    """CUSTOM levels natively == the subclass-override sweep idiom of the reference (no force quant)."""
    g = load_golden("g1c_custom_levels.npz")
    sim = mk(nb, g, "custom", custom_levels=L)
    assert relerr(sim.accelerations.numpy(), g[f"L{L}/acc0"]) < 2e-6
    sim.run(5)
    assert relerr(sim.positions.numpy(), g[f"L{L}/pos5"]) < 1e-5


# --------------------------------------------------------------------------- config 1 trajectory
def test_config1_fp64_trajectory_and_energy_drift(nb):
    g = load_golden("g2_config1_n1024.npz")
    sim = mk(nb, g, "float64")
    scale = np.abs(g["float64/pos200"]).max()
    t = 0
    energies = {}
    for snap in (0, 1, 10, 100, 200):
        sim.run(snap - t)
        t = snap
        err = np.abs(sim.positions.numpy().astype(np.float64) - g[f"float64/pos{snap}"]).max() / scale
        verr = relerr(sim.velocities.numpy(), g[f"float64/vel{snap}"])
        print(f"tick {snap}: pos err {err:.2e} vel err {verr:.2e}")
        assert err < 1e-10 and verr < 1e-10          # north_star bar
        if snap in (100, 200):
            energies[snap] = sim.get_total_energy()
            ref_e = float(g[f"float64/diag{snap}/e"])
            assert abs(energies[snap] - ref_e) <= 1e-10 * abs(ref_e)
    drift = (energies[200] - energies[100]) / abs(energies[100])
    e100, e200 = float(g["float64/diag100/e"]), float(g["float64/diag200/e"])
    assert abs(drift - (e200 - e100) / abs(e100)) < 1e-10


@pytest.mark.parametrize("mode", MODES[1:])
def test_config1_other_modes_short_horizon(nb, mode):
    g = load_golden("g2_config1_n1024.npz")
    sim = mk(nb, g, mode)
    sim.run(10)
    tol = 5e-6 if mode not in ("int8_sim", "int4_sim") else 5e-3
    assert relerr(sim.positions.numpy(), g[f"{mode}/pos10"]) < tol


# --------------------------------------------------------------------------- tile coverage
@pytest.mark.parametrize("n,ticks", [(4096, 50), (8192, 5)])
def test_tile_coverage_fp64(nb, n, ticks):
    g = load_golden(f"g3_fp64_n{n}.npz")
    sim = mk(nb, g, "float64")
    assert relerr(sim.accelerations.numpy(), g["acc0"]) < 1e-13
    ke, pe = sim.get_kinetic_energy(), sim.get_potential_energy()
    assert abs(pe - g["e0"][1]) <= 2e-6 * abs(g["e0"][1])
    sim.run(ticks)
    assert relerr(sim.positions.numpy(), g["pos_final"]) < 1e-11
    assert relerr(sim.velocities.numpy(), g["vel_final"]) < 1e-11
    assert relerr(sim.accelerations.numpy(), g["acc_final"]) < 1e-11
    assert abs(sim.get_kinetic_energy() - g["e1"][0]) <= 1e-11 * abs(g["e1"][0])
    assert abs(sim.get_potential_energy() - g["e1"][1]) <= 1e-11 * abs(g["e1"][1])


# --------------------------------------------------------------------------- vs the oracle, sizes the reference cannot reach
@pytest.mark.parametrize("n,d", [(1, 2), (2, 3), (63, 2), (255, 2), (256, 3), (513, 2), (3001, 3), (20000, 2)])
def test_ragged_sizes_vs_oracle(nb, n, d):
    from oracle import oracle as O
    rng = np.random.default_rng(n * 10 + d)
    pos = (rng.standard_normal((n, d)) * 5).astype(np.float64)
    vel = (rng.standard_normal((n, d)) * 0.05).astype(np.float64)
    mass = (0.5 + rng.random(n)).astype(np.float64)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    ref = O.accelerations_f64_fast(pos, mass)
    if n > 1:
        assert relerr(sim.accelerations.numpy(), ref) < 1e-13
    else:
        assert np.all(sim.accelerations.numpy() == 0)
    # fp32 state, FLOAT32 mode
    p32, v32, m32 = pos.astype(np.float32), vel.astype(np.float32), mass.astype(np.float32)
    sim32 = nb.GalaxySimulation(T(p32), T(v32), T(m32), precision_mode=nb.PrecisionMode.FLOAT32)
    ref32 = O.accelerations_f32_fast(p32, m32)
    if n > 1:
        assert relerr(sim32.accelerations.numpy(), ref32) < 2e-6


def test_n65536_fp64_forces_and_invariants(nb):
    """BASELINE config 2 size: forces vs the oracle's fp64 fast path + size-independent properties."""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    n = 65536
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=42, device="cpu")
    pos, vel, mass = pos.double(), vel.double(), mass.double()
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64)
    acc = sim.accelerations.numpy()
    ref = O.accelerations_f64_fast(pos.numpy(), mass.numpy())
    assert relerr(acc, ref) < 1e-13
    # Newton's third law: total momentum change vanishes
    f = (acc * mass.numpy()[:, None]).sum(0)
    assert np.abs(f).max() < 1e-9 * np.abs(acc * mass.numpy()[:, None]).sum()
    # source-block partial sums (what each of P GPUs computes) add up to the full force
    parts = []
    for r in range(4):
        s = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64, shard=(r, 4))
        parts.append(s.accelerations.numpy())
        del s
    assert relerr(sum(parts), acc) < 1e-13
    # potential energy vs oracle
    pe = sim.get_potential_energy()
    pe_ref = O.potential_energy_f64_fast(pos.numpy(), mass.numpy())
    assert abs(pe - pe_ref) <= 1e-12 * abs(pe_ref)
    # 10 leapfrog steps against the oracle's fp64 step (BASELINE config 2 size; ~15 s of host time)
    o = O.lib()
    p64, v64, m64 = pos.numpy().copy(), vel.numpy().copy(), mass.numpy().copy()   # the oracle steps in place
    a64 = O.accelerations_f64_fast(p64, m64)
    o.nbo_step_f64_fast(n, 2, O._dp(p64), O._dp(v64), O._dp(m64), O._dp(a64), 0.001, 0.1 ** 2, 0.01, 10)
    sim10 = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64)
    e_start = sim10.get_total_energy()
    sim10.run(10)
    assert relerr(sim10.positions.numpy(), p64) < 1e-12
    assert relerr(sim10.velocities.numpy(), v64) < 1e-11
    ke_ref = 0.5 * float((m64 * (v64 ** 2).sum(1)).sum())
    pe_ref10 = O.potential_energy_f64_fast(p64, m64)
    drift_ref = (ke_ref + pe_ref10 - e_start) / abs(e_start)
    drift = (sim10.get_total_energy() - e_start) / abs(e_start)
    assert abs(drift - drift_ref) < 1e-10                      # north_star: energy drift matches to 1e-10
    # time reversal: run 5 steps, flip velocities, run 5 steps -> back to the start (leapfrog is reversible)
    e0 = sim.get_total_energy()
    sim.run(5)
    sim.velocities = -sim.velocities
    sim.run(5)
    assert relerr(sim.positions.numpy(), pos.numpy()) < 1e-12
    assert abs(sim.get_total_energy() - e0) <= 1e-12 * abs(e0)


def test_shard_partials_all_modes(nb):
    g = load_golden("g1_n257_d2_e0.05.npz")
    for mode in ("float64", "float32", "float16", "custom"):
        full = mk(nb, g, mode).accelerations.numpy().astype(np.float64)
        parts = [mk(nb, g, mode, shard=(r, 3)).accelerations.numpy().astype(np.float64) for r in range(3)]
        assert relerr(sum(parts), full) < (1e-13 if mode == "float64" else 1e-6), mode


# --------------------------------------------------------------------------- API semantics
def test_dtype_state_machine(nb):
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    for mode in MODES:
        sim = mk(nb, g, mode)
        rows = [[str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]]
        for _ in range(2):
            sim.step()
            rows.append([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)])
        assert rows == api["dtype_timeline_fp32_inputs"][mode], mode


def test_fp64_inputs_float64_mode(nb):
    g = load_golden("g4_api.npz")
    sim = nb.GalaxySimulation(T(g["pos"]).double(), T(g["vel"]).double(), T(g["mass"]).double(),
                              precision_mode=nb.PrecisionMode.FLOAT64, G=0.001, dt=0.01, softening=0.1)
    assert relerr(sim.accelerations.numpy(), g["in64/float64/acc0"]) < 1e-13
    sim.run(3)
    assert relerr(sim.positions.numpy(), g["in64/float64/pos3"]) < 1e-13
    ke, pe = g["in64/float64/e3"]
    assert abs(sim.get_kinetic_energy() - ke) <= 1e-13 * abs(ke)
    assert abs(sim.get_potential_energy() - pe) <= 1e-13 * abs(pe)


def test_inplace_mutation_and_attribute_writes(nb):
    g = load_golden("g4_api.npz")
    sim = mk(nb, g, "float32")
    sim.positions[0, 0] += 1e-3                       # omega_point_test.py:738 idiom
    sim.step()
    sim.positions[5, 1] -= 2e-3
    sim.velocities[7, 0] += 1e-2
    sim.step()
    assert relerr(sim.positions.numpy(), g["mutate/pos2"]) < 2e-6
    assert relerr(sim.velocities.numpy(), g["mutate/vel2"]) < 2e-5
    sim = mk(nb, g, "float64")
    sim.step()
    sim.dt = 0.02
    sim.step()
    sim.G = 0.002
    sim.step()
    assert relerr(sim.positions.numpy(), g["attrs/pos3"]) < 1e-13
    assert relerr(sim.velocities.numpy(), g["attrs/vel3"]) < 1e-12


def test_run_callback_get_state_run_comparison(nb):
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    calls = []
    sim = nb.GalaxySimulation(T(g["pos"]), T(g["vel"]), T(g["mass"]))
    sim.run(25, callback=lambda s, t: calls.append(int(t)), callback_interval=10)
    assert calls == api["run_callback_ticks_25_by_10"]
    assert sim.tick == api["tick_after_run"]
    st = sim.get_state()
    assert sorted(st.keys()) == api["get_state_keys"]
    assert st["precision_mode"] == api["get_state_precision_mode"]
    res = nb.run_comparison(T(g["pos"]), T(g["vel"]), T(g["mass"]),
                            [nb.PrecisionMode.FLOAT64, nb.PrecisionMode.INT4_SIM], num_ticks=20,
                            callback_interval=10)
    assert sorted(res.keys()) == api["run_comparison_keys"]
    assert sorted(res["float64"].keys()) == api["run_comparison_entry_keys"]
    assert res["float64"]["history"]["ticks"] == api["run_comparison_history_ticks"]
    # energies[0] is taken on fp32-typed state upstream (fp32 sums): 1e-6; later entries fp64
    e = np.array(res["float64"]["history"]["energies"])
    ref = g["runcmp/float64/energies"]
    assert abs(e[0] - ref[0]) <= 2e-6 * abs(ref[0])
    assert np.all(np.abs(e[1:] - ref[1:]) <= 1e-12 * np.abs(ref[1:]))
    assert relerr(res["float64"]["final_state"]["positions"].numpy(), g["runcmp/float64/pos_final"]) < 1e-13


def test_subclass_override_is_honoured(nb):
    """sensitivity_test.py:55-76 pattern: the override's tensor drives the leapfrog."""
    g = load_golden("g1c_custom_levels.npz")

    class CustomQuantSim(nb.GalaxySimulation):
        def __init__(self, *args, quant_levels, **kwargs):
            self.quant_levels = quant_levels
            self.calls = 0
            super().__init__(*args, **kwargs)

        def _compute_accelerations(self):
            self.calls += 1
            pos = self.positions
            diff = pos.unsqueeze(0) - pos.unsqueeze(1)
            dist_sq = (diff ** 2).sum(dim=-1) + self.softening_sq
            dist_sq = nb._grid_quantize_safe(dist_sq, self.quant_levels, min_val=0.01)
            ff = self.G / dist_sq ** 1.5
            ff = ff * self.masses.unsqueeze(0)
            ff = ff * (1 - torch.eye(self.num_stars, device=self.device))
            return (ff.unsqueeze(-1) * diff).sum(dim=1)

    for L in (4, 1000):
        sim = CustomQuantSim(T(g["pos"]), T(g["vel"]), T(g["mass"]), quant_levels=L,
                             precision_mode=nb.PrecisionMode.FLOAT32, G=0.001, dt=0.01, softening=0.1)
        assert sim.calls == 1
        assert relerr(sim.accelerations.numpy(), g[f"L{L}/acc0"]) < 2e-6
        for _ in range(5):
            sim.step()
        assert sim.calls == 6
        assert relerr(sim.positions.numpy(), g[f"L{L}/pos5"]) < 1e-5
        assert relerr(sim.velocities.numpy(), g[f"L{L}/vel5"]) < 1e-4


def test_tensor_hooks_vs_reference(nb):
    g = load_golden("g5_hooks.npz")
    d2, force = T(g["d2"]), T(g["force"])
    for mode in MODES:
        pm = nb.PrecisionMode(mode)
        out = nb.quantize_distance_squared(d2, pm).numpy()
        ref = g[f"qd2/{mode}"]
        assert out.dtype == ref.dtype
        if mode in GRID:
            assert relerr(out, ref) < 1e-6
        else:
            assert np.array_equal(out, ref)
        outf = nb.quantize_force(force, pm).numpy()
        reff = g[f"qf/{mode}"]
        if mode in GRID:
            assert relerr(outf, reff) < 1e-6
        else:
            assert np.array_equal(outf, reff)
    for L in (4, 16, 100, 1000):
        assert relerr(nb.quantize_distance_squared(d2, nb.PrecisionMode.CUSTOM, custom_levels=L).numpy(),
                      g[f"qd2/custom{L}"]) < 1e-6
        assert relerr(nb._grid_quantize_safe(d2, L, min_val=0.5).numpy(), g[f"safe/L{L}_min0.5"]) < 1e-6
        assert relerr(nb._grid_quantize(force, L).numpy(), g[f"lin/L{L}"]) < 1e-6
    const = torch.full((7, 7), 3.0)
    assert np.array_equal(nb._grid_quantize_safe(const, 16).numpy(), g["safe/const"])
    assert np.array_equal(nb._grid_quantize(const, 16).numpy(), g["lin/const"])
    assert relerr(nb.quantize_distance_squared(d2.double(), nb.PrecisionMode.INT8_SIM).numpy(),
                  g["qd2_64/int8_sim"]) < 1e-13
    assert np.array_equal(nb.quantize_distance_squared(d2.double(), nb.PrecisionMode.FLOAT16).numpy(),
                          g["qd2_64/float16"])


def test_large_tensor_hook_through_tables_vs_oracle(nb):
    """Tensors of 2 M elements and more take _grid_quantize_safe through threshold / value tables built for the
    tensor's own bounds (plain min / max, one lookup pass) instead of a library log + exp per element: the OUTPUT must
    be bit-identical to the elementwise formula (the oracle's), for every level count the tables serve, with values
    below the clamp, and NaN / inf / constant tensors must behave as torch's formula does."""
    from oracle import oracle as O
    rng = np.random.default_rng(77)
    n = 1 << 21
    base = np.exp(rng.uniform(np.log(1e-3), np.log(5e4), n)).astype(np.float32)       # seven decades, some below 0.01
    dev = torch.device("cuda:0")
    for L in (2, 16, 64, 256, 1000, 4096):
        got = nb._grid_quantize_safe(T(base).to(dev), L).cpu().numpy()
        ref = O.grid_quantize_safe(base, L)
        assert np.array_equal(got, ref), (L, int((got != ref).sum()))
    got = nb.quantize_distance_squared(T(base).to(dev), nb.PrecisionMode.INT8_SIM).cpu().numpy()
    assert np.array_equal(got, O.grid_quantize_safe(base, 256))
    got = nb._grid_quantize_safe(T(base).to(dev), 64, min_val=2.0).cpu().numpy()
    assert np.array_equal(got, O.grid_quantize_safe(base, 64, min_val=2.0))
    narrow = (1.0 + 1e-4 * rng.random(n)).astype(np.float32)                          # narrow grid: no estimate, binary search
    assert np.array_equal(nb._grid_quantize_safe(T(narrow).to(dev), 256).cpu().numpy(), O.grid_quantize_safe(narrow, 256))
    const = np.full(n, 3.0, np.float32)
    assert np.array_equal(nb._grid_quantize_safe(T(const).to(dev), 16).cpu().numpy(), const)
    low = np.full(n, 1e-4, np.float32)                                                # everything below the clamp
    assert np.array_equal(nb._grid_quantize_safe(T(low).to(dev), 16).cpu().numpy(), np.full(n, 0.01, np.float32))
    for bad in (np.nan, np.inf):
        t = base.copy()
        t[12345] = bad
        got = nb._grid_quantize_safe(T(t).to(dev), 64).cpu().numpy()
        with np.errstate(all="ignore"):
            ref = torch_formula_safe(t, 64)
        assert np.array_equal(got, ref, equal_nan=True), bad


def torch_formula_safe(t, levels, min_val=0.01):
    """quantization.py:91-127 with torch's own CPU ops (the non-finite cases, where only torch defines the answer)."""
    x = torch.from_numpy(t).clamp(min=min_val)
    lt = torch.log(x)
    lmin, lmax = lt.min(), lt.max()
    if (lmax - lmin) < 1e-10:
        return x.numpy()
    k = torch.round((lt - lmin) / (lmax - lmin) * (levels - 1))
    return torch.exp(k / (levels - 1) * (lmax - lmin) + lmin).clamp(min=min_val).numpy()


def torch_formula_linear(t, levels):
    """quantization.py:74-88 with torch's own CPU ops: only IEEE add, sub, mul, div, round, min and max, so the kernels
    must reproduce it bit for bit (tests/test_gpu_hooks_elements.py)."""
    x = torch.from_numpy(t)
    mn, mx = x.min(), x.max()
    if mx - mn < 1e-10:
        return x.numpy()
    k = torch.round((x - mn) / (mx - mn) * (levels - 1))
    return (k / (levels - 1) * (mx - mn) + mn).numpy()


def test_cuda_tensors_zero_copy_path(nb):
    """State handed over and read back as device tensors (torch is only the allocator here)."""
    g = load_golden("g1_n257_d2_e0.05.npz")
    dev = torch.device("cuda:0")
    sim = nb.GalaxySimulation(T(g["pos"]).to(dev), T(g["vel"]).to(dev), T(g["mass"]).to(dev),
                              precision_mode=nb.PrecisionMode.FLOAT64, softening=0.05)
    assert sim.accelerations.device.type == "cuda"
    assert relerr(sim.accelerations.cpu().numpy(), g["float64/acc0"]) < 1e-13
    sim.step()
    assert sim.positions.device.type == "cuda"
    assert relerr(sim.positions.cpu().numpy(), g["float64/pos1"]) < 1e-13


def test_nan_inf_propagate_silently(nb):
    pos = torch.randn(100, 2)
    pos[3, 0] = float("nan")
    sim = nb.GalaxySimulation(pos, torch.zeros(100, 2), torch.ones(100), precision_mode=nb.PrecisionMode.FLOAT32)
    assert torch.isnan(sim.accelerations).all()      # the reference's sum over j is NaN for every i
    sim.step()                                        # must not raise
    assert torch.isnan(sim.positions).any()


def test_errors_are_exceptions(nb):
    with pytest.raises(ValueError):
        nb.GalaxySimulation(torch.zeros(4, 4), torch.zeros(4, 4), torch.ones(4))
    with pytest.raises(ValueError):
        nb.GalaxySimulation(torch.zeros(4, 2), torch.zeros(5, 2), torch.ones(4))


def test_rccl_path_with_one_rank_communicator():
    """The multi-GPU step (nb_comm_init + RCCL all-reduce of forces / r2max / PE) exercised on one
    GPU with a 1-rank communicator: results must be bit-identical to the comm-less path, on the RCCL carrier and on
    the (opt-in) direct all-reduce; all simulations of the process share ONE communicator; a handle that outlives
    nb_comm_shutdown fails with NB_ERR_COMM instead of touching the destroyed communicator."""
    import subprocess
    import sys
    script = r'''
import ctypes, os, sys
sys.path.insert(0, os.environ["NB_ROOT"])
import numpy as np, torch
import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import runtime, galaxy, _native
pos, vel, mass = galaxy.create_disk_galaxy(9000, seed=5, device="cpu")   # pair-symmetric path (tiles of 128) + deferred kick
modes = (nb.PrecisionMode.FLOAT64, nb.PrecisionMode.FLOAT32, nb.PrecisionMode.FLOAT16, nb.PrecisionMode.INT4_SIM)
def run(mode, steps=(3, 2)):
    s = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode)
    for k in steps:                      # two native calls: the second starts from settled dtypes
        s.run(k)
    out = s.positions.numpy().copy(), s.velocities.numpy().copy(), s.get_total_energy()
    s.close()
    return out
base = {m: run(m) for m in modes}
os.environ["NBODY_FORCE_COMM"] = "1"
os.environ["NB_P2P"] = "force"          # with one rank RCCL's all-reduce is a no-op and would win the timing comparison
runtime.init_distributed(device=0)
assert _native.lib().nb_comm_ready() == 0
for carrier in ("direct", "rccl"):
    if carrier == "rccl":
        os.environ["NB_NO_P2P"] = "1"                  # read when a simulation is created: force vectors through RCCL
    for m, (p0, v0, e0) in base.items():
        p1, v1, e1 = run(m)
        assert np.array_equal(p0, p1), (m, carrier)
        assert np.array_equal(v0, v1), (m, carrier)
        assert e0 == e1, (m, carrier)
    os.environ.pop("NB_NO_P2P", None)
    assert _native.lib().nb_comm_ready() == 1          # one communicator for all of them
    # ... and beside it the direct all-reduce (1 rank: its kernel just moves the vector), opted into with NB_P2P
    assert _native.lib().nb_comm_p2p_state() == 2, runtime._p2p_log
    assert runtime.allreduce_label().startswith("direct")
info = (ctypes.c_int32 * 8)()
assert _native.lib().nb_comm_info(info) == 0
assert (info[0], info[1], info[3], info[4], info[5]) == (1, 0, 0, 1, 2), list(info)     # 1 rank, RCCL count 1, direct enabled
# two simulations alive at once share the ONE input buffer of the direct path: interleaved steps stay bit-identical
a = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64)
b = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT32)
for k in (3, 2):
    a.run(k); b.run(k)
for sim, m in ((a, nb.PrecisionMode.FLOAT64), (b, nb.PrecisionMode.FLOAT32)):
    assert np.array_equal(sim.positions.numpy(), base[m][0]), m
    assert np.array_equal(sim.velocities.numpy(), base[m][1]), m
a.close()
runtime.shutdown()
assert _native.lib().nb_comm_ready() == 0 and _native.lib().nb_comm_p2p_state() == 0
# b outlived the communicator it borrowed: every further collective use must fail cleanly (ADVICE r2)
try:
    b.run(1)
    raise SystemExit("a step on a handle whose communicator was shut down did not fail")
except _native.NativeError as e:
    assert e.code == -6 and "shut down" in str(e), e
try:
    b.get_potential_energy()
    raise SystemExit("an energy evaluation on a handle whose communicator was shut down did not fail")
except _native.NativeError as e:
    assert e.code == -6, e
b.close()
print("RCCL-1RANK-OK")
'''
    env = dict(os.environ, NB_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert "RCCL-1RANK-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("n,d", [(65, 2), (257, 3), (1000, 2), (4099, 2), (6000, 3)])
def test_pair_symmetric_kernel_vs_oracle(nb, monkeypatch, n, d, r, uniform):
    """The pair-symmetric fp64 kernel (nb_force_sym.hip) forced on for ragged / small sizes."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")
    monkeypatch.setenv("NB_SYM_R", str(r))
    rng = np.random.default_rng(n + d + r)
    pos = rng.standard_normal((n, d)) * 5
    vel = rng.standard_normal((n, d)) * 0.05
    mass = np.full(n, 0.7) if uniform else 0.5 + rng.random(n)    # uniform masses take the 14-op kernel
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    assert sim.force_kernel_name() == "force_sym_kernel<double"
    assert relerr(sim.accelerations.numpy(), O.accelerations_f64_fast(pos, mass)) < 1e-13
    pe_ref = O.potential_energy_f64_fast(pos, mass)
    assert abs(sim.get_potential_energy() - pe_ref) <= 1e-13 * abs(pe_ref)      # pair-symmetric PE kernel
    ref = O.OracleSim(pos, vel, mass, "float64")
    sim.run(3)
    ref.run(3)
    assert relerr(sim.positions.numpy(), ref.positions) < 1e-13
    assert relerr(sim.velocities.numpy(), ref.velocities) < 1e-12
    # bit-reproducible: same inputs, same bits
    sim2 = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    sim2.run(3)
    assert np.array_equal(sim.positions.numpy(), sim2.positions.numpy())


@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16", "int8_sim", "int4_sim", "custom"])
@pytest.mark.parametrize("n,d,r", [(300, 2, 2), (1000, 2, 4), (777, 3, 2), (4099, 2, 4)])
def test_pair_symmetric_fp32_kernels_vs_oracle(nb, monkeypatch, n, d, r, mode, uniform):
    """fp32-state pair-symmetric kernels (all hooks) forced on for ragged / small sizes."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")
    monkeypatch.setenv("NB_SYM_R", str(r))
    rng = np.random.default_rng(n + d)
    pos = (rng.standard_normal((n, d)) * 5).astype(np.float32)
    vel = (rng.standard_normal((n, d)) * 0.05).astype(np.float32)
    mass = (np.full(n, 0.7) if uniform else 0.5 + rng.random(n)).astype(np.float32)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode))
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    ref, dbg = O.accelerations(pos, mass, mode, debug=True)
    acc = sim.accelerations.numpy()
    assert acc.dtype == np.float32
    if mode in GRID:
        got = sim.quant_debug(bins=True)
        assert np.array_equal(got["d2bins"], dbg["d2bins"])
    if mode in ("int8_sim", "int4_sim"):
        flips = int((got["fbins"] != dbg["fbins"]).sum())
        assert flips <= 2
        assert relerr(acc, ref) < (2e-6 if flips == 0 else 2e-2)
    else:
        assert relerr(acc, ref) < 2e-6
    o0 = O.OracleSim(pos, vel, mass, mode)
    assert abs(sim.get_potential_energy() - o0.get_potential_energy()) <= 2e-6 * abs(o0.get_potential_energy())
    sim.run(2)          # fused kick+drift+pack path
    o = O.OracleSim(pos, vel, mass, mode)
    o.run(2)
    tol = 5e-6 if mode not in ("int8_sim", "int4_sim") else 5e-3
    assert relerr(sim.positions.numpy(), o.positions) < tol


def test_fp16_hook_overflow_gives_zero_force(nb):
    """quantization.py:56: r2 beyond the fp16 range becomes inf -> pow(inf,1.5)=inf -> G/inf = 0."""
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    pos = (rng.standard_normal((600, 2)) * 300).astype(np.float32)      # most r2 > 65504
    mass = np.ones(600, np.float32)
    for sym in ("0", "1"):
        os.environ["NB_SYM"] = sym
        try:
            sim = nb.GalaxySimulation(T(pos), torch.zeros(600, 2), T(mass), precision_mode=nb.PrecisionMode.FLOAT16)
        finally:
            del os.environ["NB_SYM"]
        acc = sim.accelerations.numpy()
        assert np.isfinite(acc).all()
        assert relerr(acc, O.accelerations(pos, mass, "float16")) < 2e-6


@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16"])
def test_fp64_state_under_cast_modes(nb, mode):
    """fp64 tensors with a non-FLOAT64 mode (omega_point_test.py:722-733 'native precision' sims)."""
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    sim = nb.GalaxySimulation(T(g["pos"]).double(), T(g["vel"]).double(), T(g["mass"]).double(),
                              precision_mode=nb.PrecisionMode(mode), G=0.001, dt=0.01, softening=0.1)
    r0 = [str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]
    assert relerr(sim.accelerations.numpy(), g[f"in64/{mode}/acc0"]) < 2e-6
    sim.run(3)
    r1 = [str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]
    assert [r0, r1] == api["dtype_timeline_fp64_inputs"][mode]
    assert relerr(sim.positions.numpy(), g[f"in64/{mode}/pos3"]) < 1e-6
    ke, pe = g[f"in64/{mode}/e3"]
    assert abs(sim.get_kinetic_energy() - ke) <= 1e-5 * abs(ke)
    assert abs(sim.get_potential_energy() - pe) <= 1e-6 * abs(pe)


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_half_precision_state_tensors(nb, name):
    """f16 / bf16 state in FLOAT32 mode (omega_point_test.py PRECISION_LEVELS)."""
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    tdt = getattr(torch, name)
    sim = nb.GalaxySimulation(T(g["pos"]).to(tdt), T(g["vel"]).to(tdt), T(g["mass"]).to(tdt),
                              precision_mode=nb.PrecisionMode.FLOAT32, G=0.001, dt=0.01, softening=0.1)
    r0 = [str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]
    assert relerr(sim.accelerations.numpy(), g[f"in_{name}/acc0"]) < 2e-6
    pe0 = float(g[f"in_{name}/pe0"])
    assert abs(sim.get_potential_energy() - pe0) <= 4e-3 * abs(pe0)       # a half-typed scalar upstream
    assert np.isfinite(sim.get_kinetic_energy())
    sim.run(3)
    r1 = [str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]
    assert [r0, r1] == api["dtype_timeline_half_inputs_float32_mode"][name]
    assert relerr(sim.positions.numpy(), g[f"in_{name}/pos3"]) < 1e-5
    assert relerr(sim.velocities.numpy(), g[f"in_{name}/vel3"]) < 1e-4


def test_snapshot_restart_is_bit_exact(nb, tmp_path):
    """snapshot -> restore -> continue gives the same bits as an uninterrupted run."""
    from nbody_cosmological_simulation_amd import checkpoint, galaxy
    pos, vel, mass = galaxy.create_disk_galaxy(9000, seed=9, device="cpu")     # pair-symmetric path (tiles of 128)
    for mode in (nb.PrecisionMode.FLOAT64, nb.PrecisionMode.FLOAT32, nb.PrecisionMode.INT4_SIM):
        a = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode)
        a.run(4)
        h = checkpoint.save_snapshot(a, str(tmp_path / f"snap_{mode.value}.npz"))
        assert h == checkpoint.state_hash(a)
        a.run(6)
        b = checkpoint.load_snapshot(str(tmp_path / f"snap_{mode.value}.npz"))
        assert b.tick == 4 and checkpoint.state_hash(b) == h
        assert [str(b.positions.dtype), str(b.accelerations.dtype)] == \
            ([ "torch.float64", "torch.float64"] if mode == nb.PrecisionMode.FLOAT64 else ["torch.float32", "torch.float32"])
        b.run(6)
        assert checkpoint.state_hash(a) == checkpoint.state_hash(b), mode
        assert a.get_total_energy() == b.get_total_energy()


def test_config3_diagnostics_vs_reference(nb):
    """BASELINE config 3 acceptance at the reference-runnable size: rotation curve, r90, bound fraction
    and dispersion after 200 ticks, per precision mode, against the reference's own numbers.
    float64: tight (same trajectory); other modes: inside the reference's self-noise bands
    (fp32 0.4 %, fp16 3.5 %, int8 10 %, int4 15 % on curve bins)."""
    from nbody_cosmological_simulation_amd import metrics
    g = load_golden("g2_config1_n1024.npz")
    bands = {"float64": 1e-9, "float32": 0.01, "bfloat16": 0.05, "float16": 0.05, "int8_sim": 0.15,
             "int4_sim": 0.25, "custom": 0.25}
    for mode, band in bands.items():
        sim = mk(nb, g, mode)
        sim.run(200)
        pos, vel, masses = sim.positions, sim.velocities, sim.masses
        rc = metrics.compute_rotation_curve(pos, vel)
        ref_v = g[f"{mode}/diag200/rc_v"]
        ref_n = g[f"{mode}/diag200/rc_n"]
        good = (ref_n >= 20) & np.isfinite(ref_v) & np.isfinite(rc["velocities"])
        assert good.sum() >= 5
        err = np.abs(rc["velocities"][good] - ref_v[good]) / np.abs(ref_v[good])
        assert np.median(err) < band, (mode, float(np.median(err)))
        r90 = metrics.compute_galaxy_radius(pos, 90)
        assert abs(r90 - float(g[f"{mode}/diag200/r90"])) <= max(band, 1e-9) * float(g[f"{mode}/diag200/r90"])
        bf = metrics.compute_bound_fraction(pos, vel, masses, sim.G)
        assert abs(bf - float(g[f"{mode}/diag200/bound"])) <= max(band, 2e-3)
        e = sim.get_total_energy()
        e_ref = float(g[f"{mode}/diag200/e"])
        assert abs(e - e_ref) <= max(band, 1e-10) * abs(e_ref)


@pytest.mark.parametrize("n", [262144, 1048576])
def test_baseline_config_4_5_sizes_fp32(nb, n):
    """BASELINE configs 4/5 sizes (N = 262 144 / 1 048 576, fp32): forces on a sample of targets vs the
    oracle, Newton's third law, and the 4-way source-block partials a 4-GPU run would all-reduce."""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=1, device="cpu")
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT32)
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    acc = sim.accelerations.numpy()
    assert np.isfinite(acc).all()
    for i0 in (0, n // 2 - 1000, n - 2048):
        ref = O.accelerations_f32_fast_subset(pos.numpy(), mass.numpy(), i0, i0 + 2048)
        assert relerr(acc[i0:i0 + 2048], ref) < 2e-6
    tot = np.abs(acc.astype(np.float64)).sum(0)
    assert np.abs(acc.astype(np.float64).sum(0)).max() < 1e-5 * tot.max()       # fp32 outputs: rounding only
    sim.step()
    assert np.isfinite(sim.positions.numpy()).all()
    if n == 262144:
        parts = [nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT32, shard=(r, 4)).accelerations.numpy().astype(np.float64)
                 for r in range(4)]
        s = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT32)
        assert relerr(sum(parts), s.accelerations.numpy()) < 1e-6


@pytest.mark.parametrize("n", [262144, 1048576])
def test_baseline_config_4_5_sizes_vs_reference_ops(nb, n):
    """g19: BASELINE configs 4 / 5 at their real sizes against the reference's arithmetic: FLOAT32 accelerations of 64
    sampled rows from the reference's torch expressions on row blocks (tests/golden/make_golden.py g19).  The initial
    conditions are regenerated here bit for bit (numpy PCG64 stream and one multiply-add: host-independent)."""
    g = load_golden("g19_big_n_rows.npz")
    pos = ((np.random.default_rng(1900 + n).random((n, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(40.0)).astype(np.float32)
    sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), torch.ones(n), precision_mode=nb.PrecisionMode.FLOAT32)
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    acc = sim.accelerations
    assert str(acc.dtype) == str(g[f"n{n}/acc_dtype"])
    got = acc.numpy()[g[f"n{n}/rows"]].astype(np.float64)
    ref = g[f"n{n}/acc_rows"]
    assert np.abs(got - ref).max() <= 2e-6 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim"])
def test_grid_modes_pruned_max_r2_edge_cases(nb, mode):
    """The pruned max-r2 search (exact by construction) on awkward clouds: a far outlier, collinear
    points, all particles coincident (degenerate grid), and a NaN coordinate (everything NaN upstream)."""
    from oracle import oracle as O
    rng = np.random.default_rng(11)
    clouds = {
        "outlier": np.vstack([rng.standard_normal((500, 2)) * 2, [[400.0, -300.0]]]).astype(np.float32),
        "collinear": np.stack([np.linspace(-30, 30, 300), np.zeros(300)], 1).astype(np.float32),
        "ring": np.stack([10 * np.cos(np.linspace(0, 6.28, 400)), 10 * np.sin(np.linspace(0, 6.28, 400))], 1).astype(np.float32),
        "coincident": np.zeros((64, 2), np.float32),
    }
    for name, pos in clouds.items():
        n = pos.shape[0]
        mass = np.ones(n, np.float32)
        sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), T(mass), precision_mode=nb.PrecisionMode(mode))
        ref, dbg = O.accelerations(pos, mass, mode, debug=True)
        got = sim.quant_debug(bins=True)
        assert np.float32(got["lmax"]) == np.float32(dbg["lmax"]), name
        assert np.array_equal(got["d2bins"], dbg["d2bins"]), name
    pos = clouds["ring"].copy()
    pos[7, 1] = np.nan
    sim = nb.GalaxySimulation(T(pos), torch.zeros(400, 2), torch.ones(400), precision_mode=nb.PrecisionMode(mode))
    assert torch.isnan(sim.accelerations).all()


@pytest.mark.parametrize("split", [2, 4])
def test_split_sweeps_match_whole_sweeps(nb, monkeypatch, split):
    """Work items cut into 64/split rotation steps (used when a rank owns few tile pairs) give the same
    physics as whole sweeps: forces and potential energy vs the oracle, fp64 and fp32/int8."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")
    monkeypatch.setenv("NB_SYM_SPLIT", str(split))
    rng = np.random.default_rng(split)
    n = 2500
    pos = rng.standard_normal((n, 2)) * 5
    vel = rng.standard_normal((n, 2)) * 0.05
    mass = 0.5 + rng.random(n)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    assert relerr(sim.accelerations.numpy(), O.accelerations_f64_fast(pos, mass)) < 1e-13
    pe_ref = O.potential_energy_f64_fast(pos, mass)
    assert abs(sim.get_potential_energy() - pe_ref) <= 1e-13 * abs(pe_ref)
    ref = O.OracleSim(pos, vel, mass, "float64")
    sim.run(3)
    ref.run(3)
    assert relerr(sim.positions.numpy(), ref.positions) < 1e-13
    p32, v32, m32 = pos.astype(np.float32), vel.astype(np.float32), np.ones(n, np.float32)
    for mode in ("float32", "int8_sim"):
        s32 = nb.GalaxySimulation(T(p32), T(v32), T(m32), precision_mode=nb.PrecisionMode(mode))
        r32, dbg = O.accelerations(p32, m32, mode, debug=True)
        if mode == "int8_sim":
            flips = int((s32.quant_debug(bins=True)["fbins"] != dbg["fbins"]).sum())
            assert flips <= 2
            if flips:
                continue
        assert relerr(s32.accelerations.numpy(), r32) < 2e-6, mode


def test_bench_plain_line_and_dumped_outputs(nb, tmp_path):
    """`bench.py` without --full prints the headline line only; --dump-outputs writes the state its timed steps left,
    which equals the same seeded galaxy stepped warm-up + timed steps by the engine directly."""
    import subprocess
    import sys
    from nbody_cosmological_simulation_amd import galaxy
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = tmp_path / "outputs"
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--n", "4096", "--steps", "7",
                          "--warmup", "3", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 7 and line["dtype"] == "f64" and line["ms_per_step"] > 0
    assert not {"cpu_baseline", "gpu_rows", "modes", "energy_drift_rel_timed_region"} & set(line)
    pos, vel, mass = galaxy.create_disk_galaxy(4096, seed=42, device="cpu")
    dev = torch.device("cuda", 0)
    sim = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=nb.PrecisionMode.FLOAT64, G=0.001,
                              softening=0.1, dt=0.01, device=dev)
    sim.run(3)
    sim.run(7)
    for name in ("positions", "velocities", "accelerations"):
        got = np.load(out_dir / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == (4096, 2), (name, got.dtype, got.shape)
        assert relerr(got, getattr(sim, name).cpu().numpy()) < 1e-13, name
    sim.close()


def test_c_client_of_the_cabi(nb, tmp_path):
    """A plain-C program (no Python, no torch) drives the engine through include/nbody_amd.h; its
    numbers must equal the Python mirror's on the same inputs and agree with the oracle."""
    import subprocess
    from oracle import oracle as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "nbody_cosmological_simulation_amd")
    exe = str(tmp_path / "cabi_smoke")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cabi", "cabi_smoke.c"),
                           "-o", exe, "-L", pkg, "-lnbody_amd", f"-Wl,-rpath,{pkg}", "-lm"])
    n, steps = 3000, 5
    out = subprocess.run([exe, str(n), str(steps)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [float(v) for v in out.stdout.split()]
    # same LCG in numpy
    s = np.uint64(12345)
    vals = []
    with np.errstate(over="ignore"):
        for _ in range(5 * n):
            s = s * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
            vals.append(float((int(s) >> 11) & ((1 << 53) - 1)) / float(1 << 53))
    v = np.array(vals).reshape(n, 5)
    pos = np.stack([20 * v[:, 0] - 10, 20 * v[:, 1] - 10], 1)
    vel = np.stack([0.2 * v[:, 2] - 0.1, 0.2 * v[:, 3] - 0.1], 1)
    mass = 0.5 + v[:, 4]
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    sim.run(steps)
    mine = [n, sim.get_kinetic_energy(), sim.get_potential_energy(), float(sim.positions.numpy().sum()),
            float(sim.velocities.numpy().sum())]
    assert got[0] == n
    for a, b in zip(got[1:3], mine[1:3]):
        assert a == b                       # same library, same inputs: identical bits
    ref = O.OracleSim(pos, vel, mass, "float64")
    ref.run(steps)
    assert abs(got[1] - ref.get_kinetic_energy()) <= 1e-12 * abs(got[1])
    assert abs(got[2] - ref.get_potential_energy()) <= 1e-12 * abs(got[2])


def test_integration_md_ctypes_stub_runs(nb):
    """The minimal ctypes stub printed in INTEGRATION.md section 3 is executable as written."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", text, flags=re.S)
    stub = [b for b in blocks if "class GalaxySimulation" in b][0]
    stub = stub.replace('C.CDLL("libnbody_amd.so")', f'C.CDLL("{nb._native.LIB_PATH}")')
    ns = {}
    exec(stub, ns)
    g = load_golden("g1_n257_d2_e0.05.npz")
    s = ns["GalaxySimulation"](T(g["pos"]), T(g["vel"]), T(g["mass"]), nb.PrecisionMode.FLOAT64, softening=0.05)
    s.step()
    pos = torch.empty(257, 2, dtype=torch.float64)
    vel = torch.empty(257, 2, dtype=torch.float64)
    s.read(pos, vel)
    assert relerr(pos.numpy(), g["float64/pos1"]) < 1e-13
    assert np.isfinite(s.get_total_energy())


def test_2000_tick_horizon_fp64_vs_oracle(nb):
    """BASELINE config 2 horizon (2 000 ticks) at the reference-runnable size N = 1024: trajectory and
    energy drift against the oracle (pinned to the reference up to 200 ticks by the golden vectors;
    the reference's own self-noise at 2 000 ticks is 3.7e-12 of the system scale)."""
    from oracle import oracle as O
    g = load_golden("g2_config1_n1024.npz")
    sim = mk(nb, g, "float64")
    ref = O.OracleSim(g["pos"], g["vel"], g["mass"], "float64")
    e0 = sim.get_total_energy()
    ref.step()                                   # fp32-typed first step: generic oracle
    p, v, m, a = (np.ascontiguousarray(x, np.float64).copy() for x in
                  (ref.positions, ref.velocities, ref.masses, ref.accelerations))
    O.lib().nbo_step_f64_fast(1024, 2, O._dp(p), O._dp(v), O._dp(m), O._dp(a), 0.001, 0.1 ** 2, 0.01, 999)
    sim.run(1000)
    err = np.abs(sim.positions.numpy() - p).max() / np.abs(p).max()
    verr = np.abs(sim.velocities.numpy() - v).max() / np.abs(v).max()
    print(f"1000 ticks: pos err {err:.2e} vel err {verr:.2e}")
    assert err < 1e-10 and verr < 1e-10          # north_star's bar, positions AND velocities (noise floor here ~1e-12)
    O.lib().nbo_step_f64_fast(1024, 2, O._dp(p), O._dp(v), O._dp(m), O._dp(a), 0.001, 0.1 ** 2, 0.01, 1000)
    sim.run(1000)
    scale = np.abs(p).max()
    err = np.abs(sim.positions.numpy() - p).max() / scale
    verr = np.abs(sim.velocities.numpy() - v).max() / np.abs(v).max()
    e_ref = 0.5 * float((m * (v ** 2).sum(1)).sum()) + O.potential_energy_f64_fast(p, m)
    drift, drift_ref = (sim.get_total_energy() - e0) / abs(e0), (e_ref - e0) / abs(e0)
    print(f"2000 ticks: pos err {err:.2e} vel err {verr:.2e} drift {drift:.6e} (oracle {drift_ref:.6e})")
    # Velocities at 2 000 ticks sit AT the chaos floor of this system: the reference against itself (sources summed
    # in reverse) differs by 9.7e-11 of max|v| and by 3.7e-12 of the system size in positions; the reference against
    # the oracle by 4.7e-10 / 1.1e-11 (tests/golden/measure_self_noise.py, profiles/r02_self_noise_n1024.txt).  No two
    # summation orders agree to 1e-10 in velocity there, so the velocity bound at this horizon is 1e-9 (measured
    # here: 3.3e-10); positions and the energy drift hold north_star's 1e-10.
    assert err < 1e-10 and verr < 1e-9
    assert abs(drift - drift_ref) < 1e-10


@pytest.mark.parametrize("n,d", [(5000, 2), (4500, 3)])
def test_float64_mode_first_evaluation_on_fp32_state_ragged(nb, monkeypatch, n, d):
    """main.py's flow at a ragged N on the pair-symmetric path: fp32 tensors in FLOAT64 mode -> first force
    with fp32 diff/r2, fp32-typed energies at tick 0, promotion to fp64 by the first step."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")         # force the symmetric path at any size
    rng = np.random.default_rng(n)
    pos = (rng.standard_normal((n, d)) * 5).astype(np.float32)
    vel = (rng.standard_normal((n, d)) * 0.05).astype(np.float32)
    mass = (0.5 + rng.random(n)).astype(np.float32)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.FLOAT64)
    assert sim.force_kernel_name() == "force_sym_kernel<double"
    ref = O.OracleSim(pos, vel, mass, "float64")
    assert sim.accelerations.dtype == torch.float64 and sim.positions.dtype == torch.float32
    assert relerr(sim.accelerations.numpy(), ref.accelerations) < 1e-13
    assert abs(sim.get_potential_energy() - ref.get_potential_energy()) <= 2e-6 * abs(ref.get_potential_energy())
    assert abs(sim.get_kinetic_energy() - ref.get_kinetic_energy()) <= 2e-6 * abs(ref.get_kinetic_energy())
    sim.run(2)
    ref.run(2)
    assert sim.positions.dtype == torch.float64
    assert relerr(sim.positions.numpy(), ref.positions) < 1e-13
    assert abs(sim.get_potential_energy() - ref.get_potential_energy()) <= 1e-12 * abs(ref.get_potential_energy())


def test_energy_memo_tracks_state_changes(nb):
    """Energies are memoised per device state: repeated calls are free, any step / edit invalidates."""
    g = load_golden("g1_n257_d2_e0.05.npz")
    sim = mk(nb, g, "float64")
    e0 = sim.get_total_energy()
    assert sim.get_total_energy() == e0
    sim.velocities[3, 0] += 0.5                      # in-place edit must be seen
    e1 = sim.get_total_energy()
    assert e1 != e0
    sim.step()
    assert sim.get_total_energy() != e1
    pe = sim.get_potential_energy()
    sim.G = 0.002                                    # attribute write changes the potential energy scale
    assert abs(sim.get_potential_energy() - 2 * pe) <= 1e-12 * abs(pe)


def test_randomised_configurations_vs_oracle(nb, monkeypatch):
    """Seeded sweep over (N, D, mode, softening, G, dt, masses, kernel family, steps): the engine must
    track the oracle everywhere, not only on the hand-picked cases above."""
    from oracle import oracle as O
    rng = np.random.default_rng(20261004)
    modes = ["float64", "float64", "float32", "bfloat16", "float16", "int8_sim", "int4_sim", "custom"]
    worst = {}
    for case in range(48):
        n = int(rng.integers(2, 700))
        d = int(rng.choice([2, 3]))
        mode = modes[case % len(modes)]
        eps = float(rng.choice([0.01, 0.05, 0.1, 0.3]))
        G = float(rng.choice([1e-3, 5e-3, 1e-2]))
        dt = float(rng.choice([0.005, 0.01, 0.02]))
        steps = int(rng.integers(1, 4))
        sym = int(rng.integers(0, 2))
        uniform = bool(rng.integers(0, 2))
        f64_in = mode == "float64" and bool(rng.integers(0, 2))
        dtype = np.float64 if f64_in else np.float32
        pos = (rng.standard_normal((n, d)) * rng.choice([1.0, 5.0, 20.0])).astype(dtype)
        vel = (rng.standard_normal((n, d)) * 0.05).astype(dtype)
        mass = (np.full(n, 1.3) if uniform else 0.2 + 2 * rng.random(n)).astype(dtype)
        monkeypatch.setenv("NB_SYM", str(sym))
        if sym:
            monkeypatch.setenv("NB_SYM_R", str(int(rng.choice([2, 4]))))      # D = 3, R = 4: two-half source sweeps
        sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode), G=G,
                                  softening=eps, dt=dt)
        ref = O.OracleSim(pos, vel, mass, mode, G=G, softening=eps, dt=dt)
        tag = f"case {case}: n={n} d={d} {mode} eps={eps} sym={sym} uniform={uniform} f64_in={f64_in}"
        quant = mode in ("int8_sim", "int4_sim")
        if mode in GRID:
            dbg = O.accelerations(pos, mass, mode, G=G, softening=eps, debug=True)[1]
            got = sim.quant_debug(bins=True)
            assert np.array_equal(got["d2bins"], dbg["d2bins"]), tag
            if quant and int((got["fbins"] != dbg["fbins"]).sum()) > 0:
                continue                                  # a flipped force bin: trajectories legitimately differ
        tol = 1e-12 if mode == "float64" else 3e-6
        e = relerr(sim.accelerations.numpy(), ref.accelerations)
        assert e < tol, (tag, e)
        sim.run(steps)
        ref.run(steps)
        if not quant:
            e2 = relerr(sim.positions.numpy(), ref.positions)
            assert e2 < (1e-12 if mode == "float64" else 1e-5), (tag, e2)
            assert str(sim.positions.dtype).replace("torch.", "") == str(ref.positions.dtype), tag
        worst[mode] = max(worst.get(mode, 0.0), e)
    print("worst single-evaluation errors:", {k: f"{v:.1e}" for k, v in worst.items()})


@pytest.mark.parametrize("name,code", [("float16", 0), ("bfloat16", 1)])
def test_half_precision_state_in_float64_mode(nb, name, code):
    """Default precision mode with f16 / bf16 tensors: half arithmetic for diff/r2 and the tick-0 energies,
    fp64 from the hook on, fp64 state after the first step (torch promotion)."""
    from oracle import oracle as O
    g = load_golden("g4_api.npz")
    tdt = getattr(torch, name)
    pos, vel, mass = (T(g[k]).to(tdt) for k in ("pos", "vel", "mass"))
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64, G=0.001, dt=0.01, softening=0.1)
    ref = O.OracleSim(pos.float().numpy(), vel.float().numpy(), mass.float().numpy(), "float64", codes=(code, code, code))
    assert sim.accelerations.dtype == torch.float64 and sim.positions.dtype == tdt
    assert relerr(sim.accelerations.numpy(), ref.accelerations) < 1e-13
    assert abs(sim.get_potential_energy() - ref.get_potential_energy()) <= 1e-2 * abs(ref.get_potential_energy())
    sim.run(3)
    ref.run(3)
    assert sim.positions.dtype == torch.float64 and sim.velocities.dtype == torch.float64
    assert relerr(sim.positions.numpy(), ref.positions) < 1e-13
    assert relerr(sim.velocities.numpy(), ref.velocities) < 1e-12


@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim", "custom"])
@pytest.mark.parametrize("masses", ["uniform", "mixed"])
def test_symmetric_grid_kernel_pair_selection(nb, monkeypatch, mode, masses):
    """Grid modes on the pair-symmetric path launch the uniform-mass kernel and the general kernel as a pair
    and let the device tables pick one (GridTables::uniform_ok).  Clouds that flip the choice -- ordinary,
    a narrow grid (no usable estimate), all particles coincident (degenerate grid), a NaN coordinate -- must
    match the oracle either way: accelerations before force quantisation, lmax and every distance bin."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")
    rng = np.random.default_rng(23)
    n = 700                                   # three tiles of 256: diagonal, off-diagonal and padded work
    clouds = {
        "ordinary": (rng.standard_normal((n, 2)) * 3).astype(np.float32),
        "narrow": (rng.standard_normal((n, 2)) * 0.0002).astype(np.float32),   # a = ln2 (L-1)/range > 1e4
        "coincident": np.full((n, 2), 0.25, np.float32),
    }
    mass = np.full(n, 0.75, np.float32) if masses == "uniform" else rng.uniform(0.5, 2.0, n).astype(np.float32)
    for name, pos in clouds.items():
        sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), T(mass), precision_mode=nb.PrecisionMode(mode))
        assert sim.force_kernel_name().startswith("force_sym_kernel<float"), name
        ref, dbg = O.accelerations(pos, mass, mode, debug=True)
        got = sim.quant_debug(bins=True)
        assert np.float32(got["lmax"]) == np.float32(dbg["lmax"]), name
        assert np.array_equal(got["d2bins"], dbg["d2bins"]), name
        acc = sim.accelerations.numpy()
        scale = np.abs(ref).max() + 1e-30
        # force quantisation (int8/int4) snaps to a grid of the summed forces: compare in grid steps
        tol = 2e-6 if mode == "custom" else 1.01 * (dbg["fmax"] - dbg["fmin"]) / ((256 if mode == "int8_sim" else 16) - 1) / scale
        assert np.abs(acc - ref).max() / scale <= max(tol, 2e-6), (name, np.abs(acc - ref).max() / scale)
    pos = clouds["ordinary"].copy()
    pos[5, 0] = np.nan
    sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), T(mass), precision_mode=nb.PrecisionMode(mode))
    assert torch.isnan(sim.accelerations).all()


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("levels", [256, 16, 64, 1000])
def test_grid_force_kernel_decides_pairs_at_the_bin_edges(nb, monkeypatch, levels, r):
    """Adversarial input for the table-free pair path of the FORCE kernel (its own bin decisions are not what
    nb_quant_bins_rows reports): a star at the origin and stars on a line whose r2 to it sits one fp32 step below /
    exactly on / one step above a bin threshold, for every threshold between r2 = 1 and 1.7 -- the zone where the
    estimate (v_log_f32, r2 from fused multiply-adds) must hand over to the exact thresholds with the reference's r2.
    All these pairs weigh about the same in the origin star's force, so ONE pair in a wrong bin moves it by
    (bin step) / (number of stars): 1e-4 ... 1e-2, far above the 2e-6 asserted.  The grids of INT8 (256 levels) and INT4
    (16) are run as CUSTOM grids of the same level counts -- the same kernel and tables without the force
    quantisation that would blur a wrong bin.  (Negative control, run once by hand: with the safety margin of the
    estimate removed -- sure_lim = 0.5 -- this test fails with errors of 1e-4.)"""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", "1")
    monkeypatch.setenv("NB_SYM_R", str(r))
    mode = "custom"
    eps2 = np.float32(0.1 * 0.1)
    xmax = np.float32(1.3)

    def r2_of(x):                       # the reference's fp32 r2 of the pair (origin, (x, 0)), op by op
        x = np.asarray(x, np.float32)
        return (x * x + np.float32(0.0)) + eps2

    r2max = r2_of(xmax)

    def bins(t):                        # bins of candidate r2 values under the system's own bounds (diagonal, farthest pair)
        arr = np.concatenate([[eps2, r2max], np.asarray(t, np.float32)]).astype(np.float32)
        _, b, _, _ = O.grid_quantize_safe(arr, levels, bins=True)
        return b[2:]

    k_lo, k_hi = int(bins([1.0])[0]) + 1, int(bins([1.68])[0])
    xs = []
    for k in range(k_lo, k_hi + 1):
        lo, hi = np.float32(1.0).view(np.uint32).astype(np.int64), np.float32(1.7).view(np.uint32).astype(np.int64)
        while hi - lo > 1:              # smallest fp32 r2 whose bin is >= k
            mid = (lo + hi) // 2
            if bins([np.array(mid, np.uint32).view(np.float32)])[0] >= k:
                hi = mid
            else:
                lo = mid
        thr = np.array(hi, np.uint32).view(np.float32)
        # positions whose r2 lands just below / on / just above the threshold
        x0 = np.float32(np.sqrt(np.float64(thr) - np.float64(eps2)))
        cand = (x0.view(np.uint32).astype(np.int64) + np.arange(-6, 7)).astype(np.uint32).view(np.float32)
        rr = r2_of(cand)
        below, above = cand[rr < thr], cand[rr >= thr]
        xs += [below.max(), above.min()]
        if (rr == thr).any():
            xs.append(cand[rr == thr][0])
    xs = np.unique(np.array(xs, np.float32))
    rng = np.random.default_rng(5)
    n = max(300 if r == 4 else 200, int(xs.size) + 50)
    fill = rng.uniform(1.0, 1.29, n - 2 - xs.size).astype(np.float32)
    pos = np.zeros((n, 2), np.float32)
    pos[1:1 + xs.size, 0] = xs
    pos[1 + xs.size:n - 1, 0] = fill
    pos[n - 1, 0] = xmax
    mass = np.full(n, 0.01, np.float32)
    ref, dbg = O.accelerations(pos, mass, mode, levels=levels, debug=True)
    edge_bins = dbg["d2bins"][0, 1:1 + xs.size]
    assert len(set(edge_bins.tolist())) >= max(1, (k_hi - k_lo) // 2)   # the constructed stars do straddle the thresholds
    sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), T(mass), precision_mode=nb.PrecisionMode(mode),
                              custom_levels=levels)
    assert sim.force_kernel_name().startswith("force_sym_kernel<float")
    got = sim.quant_debug(bins=True)
    assert np.float32(got["lmax"]) == np.float32(dbg["lmax"])
    assert np.array_equal(got["d2bins"], dbg["d2bins"])
    # ... and the force kernel's OWN decisions, read out of its pair loop (round 3): every star's bin checksums
    bs = sim.quant_bin_sums("tiled")
    k64 = dbg["d2bins"].astype(np.int64)
    wgt = (np.arange(n, dtype=np.int64) % 65521) + 1
    assert bs["path"] == "sym" and bs["shape"] == r
    assert np.array_equal(bs["sum_k"], k64.sum(axis=1)), "the pair loop put a pair into a bin the reference formula does not"
    assert np.array_equal(bs["sum_kw"], (k64 * wgt[None, :]).sum(axis=1))
    if levels <= 256:
        assert bs["fast_path"] and bs["pairs_table"] > 0 and bs["pairs_table_free"] > 0     # both routes were taken
    acc = sim.accelerations.numpy().astype(np.float64)
    assert abs(acc[0, 0] - ref[0, 0]) <= 2e-6 * abs(ref[0, 0]), (acc[0], ref[0])
    assert np.abs(acc - ref).max() <= 2e-6 * np.abs(ref).max()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_symmetric_plan_of_every_rank_adds_up(nb, monkeypatch, world):
    """Multi-GPU by construction: the pair-symmetric work lists the P ranks would run (snake-dealt super-rows,
    tail smoothing, per-rank slab prefixes) are executed one after the other on this GPU as comm-less shards
    (NB_SYM=2); what RCCL would all-reduce -- the partial forces and the partial potential energies -- must
    add up to the single-GPU result.  fp64 (fp64- and fp32-typed positions), fp32 and a grid mode; D = 2 and 3."""
    from nbody_cosmological_simulation_amd import galaxy
    monkeypatch.setenv("NB_SYM", "2")
    rng = np.random.default_rng(world)
    cases = []
    p2, v2, m2 = galaxy.create_disk_galaxy(9000, seed=world, device="cpu")
    cases.append(("f64 D2", p2.double(), v2.double(), m2.double(), nb.PrecisionMode.FLOAT64, 1e-13))
    cases.append(("f64-mode fp32-typed D2", p2, v2, m2, nb.PrecisionMode.FLOAT64, 1e-13))
    cases.append(("f32 D2", p2, v2, m2 * torch.from_numpy(rng.uniform(0.5, 1.5, 9000).astype(np.float32)),
                  nb.PrecisionMode.FLOAT32, 2e-6))
    cases.append(("custom D2", p2, v2, m2, nb.PrecisionMode.CUSTOM, 2e-6))
    # 9000 particles = 9 super-rows of 1024: at least one per rank (with fewer super-rows than ranks every
    # rank falls back to the one-sided source blocks -- the choice is rank-independent by construction)
    p3 = torch.from_numpy((rng.standard_normal((9000, 3)) * 4).astype(np.float32))
    cases.append(("f64 D3", p3.double(), torch.zeros(9000, 3, dtype=torch.float64), torch.ones(9000, dtype=torch.float64),
                  nb.PrecisionMode.FLOAT64, 1e-13))
    cases.append(("f32 D3", p3, torch.zeros(9000, 3), torch.ones(9000), nb.PrecisionMode.FLOAT32, 2e-6))
    if world == 8:      # the driver's scaling run: BASELINE config 2 on 8 ranks (tail-smoothed plans)
        pb, vb, mb = galaxy.create_disk_galaxy(65536, seed=42, device="cpu")
        cases.append(("f64 N=65536", pb.double(), vb.double(), mb.double(), nb.PrecisionMode.FLOAT64, 1e-13))
    for name, pos, vel, mass, mode, tol in cases:
        full = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode)
        assert full.force_kernel_name().startswith("force_sym_kernel"), name
        acc = full.accelerations.numpy().astype(np.float64)
        pe = full.get_potential_energy()
        parts, pes = [], []
        for r in range(world):
            s = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode, shard=(r, world))
            assert s.force_kernel_name().startswith("force_sym_kernel"), (name, r)
            parts.append(s.accelerations.numpy().astype(np.float64))
            pes.append(s.get_potential_energy())
            s.close()
        assert relerr(sum(parts), acc) < tol, (name, relerr(sum(parts), acc))
        # energies of fp32-typed state are fp32 numbers (each shard's partial is rounded on the way out here;
        # the real multi-GPU path all-reduces the fp64 partials before that rounding)
        pe_tol = 1e-12 if pos.dtype == torch.float64 else 2e-6
        assert abs(sum(pes) - pe) <= pe_tol * abs(pe), (name, sum(pes), pe)


@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim"])
def test_grid_modes_default_path_above_symmetric_threshold(nb, mode):
    """No tuning knobs: N = 9000 takes the production path of the large configs (pruned max-r2 search, uniform-mass
    packed symmetric kernel, fused force quantisation).  Every one of the 81 M distance bins, lmax, the force grid
    bounds and the quantised accelerations against the oracle's restatement of the reference."""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    pos, vel, mass = galaxy.create_disk_galaxy(9000, seed=77, device="cpu")
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode))
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    ref, dbg = O.accelerations(pos.numpy(), mass.numpy(), mode, debug=True)
    got = sim.quant_debug(bins=True)
    assert np.float32(got["lmin"]) == np.float32(dbg["lmin"]) and np.float32(got["lmax"]) == np.float32(dbg["lmax"])
    assert np.array_equal(got["d2bins"], dbg["d2bins"])
    levels = 256 if mode == "int8_sim" else 16
    step = (dbg["fmax"] - dbg["fmin"]) / (levels - 1)
    assert abs(got["fmin"] - dbg["fmin"]) <= 2e-6 * abs(dbg["fmin"]) and abs(got["fmax"] - dbg["fmax"]) <= 2e-6 * abs(dbg["fmax"])
    # forces are snapped to the force grid: identical up to bin flips of values that sit on a rounding boundary
    diff = np.abs(sim.accelerations.numpy().astype(np.float64) - ref.astype(np.float64))
    assert diff.max() <= 1.01 * step
    assert (diff > 0.5 * step).mean() < 1e-3


@pytest.mark.parametrize("mode", ["int8_sim", "custom"])
def test_grid_modes_trajectory_on_symmetric_path(nb, mode):
    """Three leapfrog steps at N = 9000 on the production grid path (fused quantisation + kicks + next opening
    kick inside nb_step) against the oracle stepping with the reference's operation order."""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    pos, vel, mass = galaxy.create_disk_galaxy(9000, seed=78, device="cpu")
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode))
    ref = O.OracleSim(pos.numpy(), vel.numpy(), mass.numpy(), mode)
    assert relerr(sim.accelerations.numpy(), ref.accelerations) < 2e-6     # same positions: same bins, same forces
    sim.run(3)
    ref.run(3)
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    v, v_ref = sim.velocities.numpy().astype(np.float64), ref.velocities.astype(np.float64)
    noise = load_golden("g21_reference_self_noise.npz")
    if mode == "custom":
        # The table-free pair path reproduces the accelerations to ~2e-7 (bins are identical for identical
        # positions); once a position differs in its last bit, a pair sitting on a bin edge can land in the
        # neighbouring bin of this 64-level grid (a 33 % jump of that pair's factor) -- on either side of the
        # comparison.  The REFERENCE does exactly that against itself when its initial positions move by one fp32 ulp
        # (golden g21, N = 4096: 0.098 % of the particles beyond 2e-6, max 4.1e-6): the share of such particles is held
        # to twice the reference's own; one flipped pair cannot move a velocity by more than 0.33 x the largest
        # softened pair acceleration (0.385 G m / eps^2) x dt / 2 per half kick.
        err = np.abs(v - v_ref).max(axis=1) / np.abs(v_ref).max()
        ref_frac = max(float(noise[f"traj/{c}/custom/ulp100/vel_frac_gt_2e-6"]) for c in ("n4096", "n1024"))
        print(f"custom 3 steps: max {err.max():.2e}, particles above 2e-6: {(err > 2e-6).sum()} of {err.size} "
              f"(reference against itself: {ref_frac:.2e})")
        assert (err > 2e-6).mean() <= 2 * ref_frac
        one_flip = 0.33 * 0.385 * 0.001 * 1.0 / 0.1 ** 2 * 0.005 / np.abs(v_ref).max()
        assert err.max() <= 2 * one_flip
    else:
        # int8 snaps the summed forces to a 256-level grid: a value on a rounding boundary may land in the
        # neighbouring bin (fp32 summation order), which moves that velocity component by step*dt/2 per half kick.
        # Such flips must stay isolated (share of particles: twice the reference's own under a one-ulp perturbation of
        # its initial positions, golden g21) and bounded by the six half kicks of three steps.
        _, dbg = O.accelerations(pos.numpy(), mass.numpy(), mode, debug=True)
        step = (dbg["fmax"] - dbg["fmin"]) / 255
        dv = np.abs(v - v_ref)
        ref_frac = max(float(noise[f"traj/{c}/int8_sim/ulp100/vel_frac_gt_2e-6"]) for c in ("n4096", "n1024"))
        frac = (dv.max(axis=1) > 2e-6 * np.abs(v_ref).max()).mean()
        print(f"int8 3 steps: particles above 2e-6: {frac:.2e} (reference against itself: {ref_frac:.2e})")
        assert dv.max() <= 6 * step * 0.01 / 2 * 1.5
        assert frac <= max(2 * ref_frac, 2.0 / dv.shape[0])
    assert relerr(sim.positions.numpy(), ref.positions) < 2e-6
    e, e_ref = sim.get_total_energy(), ref.get_total_energy()
    assert abs(e - e_ref) <= 2e-5 * abs(e_ref)


@pytest.mark.parametrize("mode", ["custom", "int8_sim", "int4_sim"])
@pytest.mark.parametrize("case", ["n4096", "n1024"])
def test_grid_mode_trajectories_vs_reference_within_its_own_noise(nb, case, mode):
    """Three leapfrog steps of the grid modes against the REFERENCE's own final state (golden g21: N = 4096 disk galaxy
    of g13, N = 1024 of config 1), with bars taken from what the reference does against ITSELF (same fixture): under a
    reversed summation order it reproduces itself to 1.2e-7 (its fp32 sums are nearly order-independent); with every
    initial coordinate moved by one fp32 ulp -- the state any implementation whose fp32 sums are not bit-identical to
    torch's is in after its first drift -- isolated particles jump (pairs crossing a distance-bin edge, force values
    crossing a force-bin edge).  Asserted: the share of particles beyond 2e-6 of max|v| and the largest deviation stay
    within TWICE the reference's own figures (floors: two particles -- one flipped pair touches two -- and the fp32
    single-evaluation bar 2e-6); positions and energy alike."""
    noise = load_golden("g21_reference_self_noise.npz")
    g = load_golden("g13_bins_n4096_d2.npz" if case == "n4096" else "g2_config1_n1024.npz")
    sim = nb.GalaxySimulation(T(g["pos"]), T(g["vel"]), T(g["mass"]), precision_mode=nb.PrecisionMode(mode),
                              G=0.001, softening=0.1, dt=0.01)
    sim.run(3)
    tag = f"traj/{case}/{mode}"
    v_ref = noise[f"{tag}/vel3"].astype(np.float64)
    v = sim.velocities.numpy().astype(np.float64)
    err = np.abs(v - v_ref).max(axis=1) / np.abs(v_ref).max()
    frac, worst = float((err > 2e-6).mean()), float(err.max())
    ref_frac = float(noise[f"{tag}/ulp100/vel_frac_gt_2e-6"])
    ref_max = float(noise[f"{tag}/ulp100/vel_max"])
    print(f"{tag}: particles beyond 2e-6: {frac:.2e} (reference vs itself {ref_frac:.2e}), max {worst:.2e} "
          f"(reference vs itself {ref_max:.2e}), kernel {sim.force_kernel_name()}")
    assert frac <= max(2 * ref_frac, 2.0 / err.size)
    assert worst <= max(2 * ref_max, 2e-6)
    assert relerr(sim.positions.numpy(), noise[f"{tag}/pos3"]) <= max(2 * float(noise[f"{tag}/ulp100/pos_relerr"]), 2e-6)
    e_ref = float(noise[f"{tag}/energy3"])
    assert abs(sim.get_total_energy() - e_ref) <= max(2 * float(noise[f"{tag}/ulp100/energy_relerr"]), 2e-6) * abs(e_ref)


def _exact_r2max_f32(pos, eps2):
    """max over all pairs of the reference's fp32 r2 = ((dx*dx + dy*dy) [+ dz*dz]) + eps2, one rounding per op (torch fp32
    on the CPU: separate multiply and add kernels, the reference's own arithmetic)."""
    p = torch.from_numpy(np.ascontiguousarray(pos, np.float32))
    e = torch.tensor(float(eps2), dtype=torch.float32)
    cols = [p[:, k].contiguous() for k in range(p.shape[1])]
    best = torch.tensor(0.0)
    for i0 in range(0, p.shape[0], 1024):
        r2 = None
        for c in cols:
            d = c[None, :] - c[i0:i0 + 1024, None]
            sq = d * d
            r2 = sq if r2 is None else r2 + sq
        best = torch.maximum(best, (r2 + e).max())
    return np.float32(best.item())


@pytest.mark.parametrize("mode", ["int4_sim", "custom", "custom1000"])
@pytest.mark.parametrize("n,d", [(3000, 2), (2500, 3), (5000, 3), (9000, 2), (30000, 2)])
def test_tracked_max_r2_search_is_exact_over_steps(nb, monkeypatch, n, d, mode):
    """Round 3: after its first evaluation a grid-mode simulation TRACKS the farthest pair (filter + scan, two launches,
    tables built by the scan's last workgroup) instead of searching it from scratch.  The maximum must stay the exact
    fp32 maximum over all pairs at every step -- also when a star outruns the margin of the candidate test (the scan
    then falls back to all pairs), on the one-launch small-system path (N = 3000, 2500: all-pairs pass) and on the tiled
    paths -- and the trajectory must be bit-identical to a run that searches from scratch every time (NB_NO_TRACK)."""
    rng = np.random.default_rng(n + d)
    pos = (rng.standard_normal((n, d)) * 4).astype(np.float32)
    vel = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    pos[7] = 0.0
    pos[7, 0] = 25.0                           # an escaper at the rim: 0.6 per step outwards, far beyond the 0.5 % margin
    vel[7] = 0.0                               # on rho_max -- every step's filter sees its bound violated
    vel[7, 0] = 60.0
    mass = np.ones(n, np.float32)
    eps2 = np.float32(0.1 * 0.1)

    def run(track):
        if track:
            monkeypatch.delenv("NB_NO_TRACK", raising=False)
        else:
            monkeypatch.setenv("NB_NO_TRACK", "1")
        if mode == "custom1000":               # more levels than one workgroup builds: the tables keep a launch of their own
            sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.CUSTOM, custom_levels=1000)
        else:
            sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode))
        got = []
        for _ in range(6):
            sim.run(1)
            dbg = sim.quant_debug()
            got.append((np.float32(dbg["r2max"]), np.float32(dbg["lmax"]), sim.positions.numpy().copy()))
        return got

    tracked, scratch = run(True), run(False)
    for step, ((r_t, l_t, x_t), (r_s, l_s, x_s)) in enumerate(zip(tracked, scratch)):
        assert r_t == r_s and l_t == l_s, (step, r_t, r_s)
        if n < 20000 or step % 2 == 1:          # the host-side exact maximum of 9e8 pairs takes seconds: every other step there
            want = _exact_r2max_f32(x_t, eps2)
            assert r_t == want, (step, r_t, want)
        assert np.array_equal(x_t, x_s), f"step {step}: the tracked search changed the trajectory"
    # the escaper did become a member of the farthest pair
    assert tracked[-1][0] > tracked[0][0]


def test_tracked_max_r2_search_survives_nan_and_new_positions(nb):
    """A NaN coordinate poisons the grid exactly like the from-scratch search (torch's max() is NaN); writing new
    positions re-seeds the search."""
    rng = np.random.default_rng(0)
    n = 5000
    pos = (rng.standard_normal((n, 2)) * 4).astype(np.float32)
    sim = nb.GalaxySimulation(T(pos), torch.zeros(n, 2), torch.ones(n), precision_mode=nb.PrecisionMode.CUSTOM)
    sim.run(2)
    x = sim.positions.numpy().copy()
    assert np.float32(sim.quant_debug()["r2max"]) == _exact_r2max_f32(x, np.float32(0.01))
    far = x * np.float32(3.0)                   # a different, three times larger system: the old far pair / bound are stale
    sim.positions = T(far)
    sim.run(1)
    assert np.float32(sim.quant_debug()["r2max"]) == _exact_r2max_f32(sim.positions.numpy(), np.float32(0.01))
    bad = sim.positions.numpy().copy()
    sim.run(1)                                  # tracked again ...
    bad = sim.positions.numpy().copy()
    bad[11, 1] = np.nan
    sim.positions = T(bad)
    sim.run(2)                                  # ... seeded with a NaN, then tracked with a NaN
    assert np.isnan(sim.quant_debug()["r2max"]) and torch.isnan(sim.accelerations).all()


@pytest.mark.parametrize("L,sym", [(512, 0), (1000, 1), (4096, 0), (4096, 1)])
def test_custom_levels_above_256_bins(nb, monkeypatch, L, sym):
    """sensitivity_test.py sweeps 512 / 1024 / 4096 levels: the fused path serves up to 4096 (tables sized per
    launch).  Every distance bin and lmax against the oracle, one-sided and symmetric kernels, then a short
    trajectory; more levels than that fail loudly."""
    from oracle import oracle as O
    monkeypatch.setenv("NB_SYM", str(sym))
    rng = np.random.default_rng(L + sym)
    n = 900
    pos = (rng.standard_normal((n, 2)) * 6).astype(np.float32)
    vel = (rng.standard_normal((n, 2)) * 0.05).astype(np.float32)
    mass = (np.ones(n) if sym else 0.5 + rng.random(n)).astype(np.float32)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.CUSTOM, custom_levels=L)
    ref, dbg = O.accelerations(pos, mass, "custom", levels=L, debug=True)
    got = sim.quant_debug(bins=True)
    assert np.float32(got["lmax"]) == np.float32(dbg["lmax"])
    assert np.array_equal(got["d2bins"], dbg["d2bins"])
    assert relerr(sim.accelerations.numpy(), ref) < 3e-6
    o = O.OracleSim(pos, vel, mass, "custom", levels=L)
    sim.run(3)
    o.run(3)
    assert relerr(sim.positions.numpy(), o.positions) < 1e-5
    # beyond the table capacity the per-pair generic path takes over (test_custom_levels_beyond_the_tables)
    big = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode.CUSTOM, custom_levels=5000)
    assert big.force_kernel_name() == "generic_force_kernel"


@pytest.mark.parametrize("n", [300, 1500])
@pytest.mark.parametrize("mode", ["float32", "float16", "float64"])
def test_half_typed_state_energies_follow_the_masses_dtype(nb, n, mode):
    """omega_point_test.py:722-733 builds simulations from float16 tensors: positions and velocities are promoted
    by the first step, the masses stay float16 for good, so `mass_prod` (simulation.py:185) is a float16 product
    even later on.  Energies before and after the promotion against the oracle's dtype model."""
    from oracle import oracle as O
    rng = np.random.default_rng(n)
    pos = (rng.standard_normal((n, 2)) * 5).astype(np.float16)
    vel = (rng.standard_normal((n, 2)) * 0.05).astype(np.float16)
    mass = (0.5 + rng.random(n)).astype(np.float16)
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode))
    ref = O.OracleSim(pos, vel, mass, mode)
    for steps in (0, 3):
        sim.run(steps)
        ref.run(steps)
        assert str(sim.masses.dtype) == "torch.float16"
        for got, want in ((sim.get_kinetic_energy(), ref.get_kinetic_energy()),
                          (sim.get_potential_energy(), ref.get_potential_energy())):
            # (float16-typed sums overflow to -inf at N = 1500 before the promotion, on both sides)
            assert got == want or abs(got - want) <= 2e-7 * abs(want), (steps, got, want)


@pytest.mark.parametrize("n", [96, 700])
@pytest.mark.parametrize("hname", ["float16", "bfloat16"])
@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16", "float64"])
def test_half_typed_state_vs_reference_golden(nb, n, hname, mode):
    """g7: the reference run from float16 / bfloat16 tensors (omega_point_test.py:722-733) in every cast mode and
    FLOAT64 -- energies before and after the promotion, state and dtypes after three steps."""
    g = load_golden("g7_half_state.npz")
    key = f"n{n}/{hname}/{mode}"
    tdt = getattr(torch, hname)
    sim = nb.GalaxySimulation(T(g[f"n{n}/{hname}/pos"]).to(tdt), T(g[f"n{n}/{hname}/vel"]).to(tdt),
                              T(g[f"n{n}/{hname}/mass"]).to(tdt), precision_mode=nb.PrecisionMode(mode))

    def close(got, want, tol):
        return got == want or abs(got - want) <= tol * abs(want)

    ke0, pe0 = g[key + "/e0"]
    assert close(sim.get_kinetic_energy(), ke0, 4e-3) and close(sim.get_potential_energy(), pe0, 8e-3)
    sim.run(3)
    ke3, pe3 = g[key + "/e3"]
    tol = 1e-9 if mode == "float64" else 2e-6
    assert close(sim.get_kinetic_energy(), ke3, tol) and close(sim.get_potential_energy(), pe3, tol)
    assert relerr(sim.positions.double().numpy(), g[key + "/pos3"]) < (1e-12 if mode == "float64" else 1e-5)
    assert relerr(sim.velocities.double().numpy(), g[key + "/vel3"]) < (1e-10 if mode == "float64" else 1e-4)
    assert [str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype), str(sim.masses.dtype)] == \
        list(g[key + "/dtypes3"])


@pytest.mark.parametrize("idx", range(12))
def test_parameter_extremes_vs_reference_golden(nb, idx):
    """g8: softening 0 / 1e-4 / 1.0, dt up to 2.0 through the stock class (crash_point_test.py, falsification_tests.py)
    -- NaN patterns (FLOAT16 at softening 1e-4, FLOAT64 at softening 0 incl. the NaN potential), grid clamps, and
    the violent dt = 2 runs against the reference's own numbers."""
    from test_oracle_golden import _g8_check
    g = load_golden("g8_extremes.npz")
    key = str(g["cases"][idx])
    _g8_check(lambda mode, eps, dt: nb.GalaxySimulation(T(g["pos"]), T(g["vel"]), T(g["mass"]),
                                                        precision_mode=nb.PrecisionMode(mode), G=0.001, softening=eps,
                                                        dt=dt),
              key, g, key.startswith("float64"))


@pytest.mark.parametrize("idx", range(35))
def test_degenerate_systems_vs_reference_golden(nb, idx):
    """g9: N = 1, 2, 3, coincident particles, a massless particle (3-D), all seven modes against the reference."""
    from test_oracle_golden import _g9_check
    g = load_golden("g9_degenerate.npz")
    _g9_check(lambda p, v, m, mode: nb.GalaxySimulation(T(p), T(v), T(m), precision_mode=nb.PrecisionMode(mode)),
              str(g["cases"][idx]), g)


@pytest.mark.parametrize("name", ["zero_neg_huge", "inf", "nan", "vec1d", "cube3d", "single"])
def test_tensor_hook_edge_values_vs_reference_golden(nb, name):
    """g10: the tensor-level hooks on zeros, negatives, 1e30, inf, NaN, 2-3 levels and odd shapes."""
    from test_oracle_golden import _g10_check
    g = load_golden("g10_hook_edges.npz")
    _g10_check((lambda t, mode: nb.quantize_distance_squared(T(t), nb.PrecisionMode(mode)).numpy(),
                lambda t, mode: nb.quantize_force(T(t), nb.PrecisionMode(mode)).numpy(),
                lambda t, L, mv: nb._grid_quantize_safe(T(t), L, min_val=mv).numpy(),
                lambda t, L: nb._grid_quantize(T(t), L).numpy()), g, name)


def test_metric_flow_vs_reference_golden(nb):
    """g12: main.py's flow -- collect_metrics at tick 0 and in a run() callback every 10 ticks (float64 and int4),
    compare_rotation_curves of the final states -- against the reference's time series."""
    from nbody_cosmological_simulation_amd import metrics
    g = load_golden("g12_metric_flow.npz")
    finals = {}
    for mode, tol in (("float64", 1e-9), ("int4_sim", 2e-5)):
        sim = nb.GalaxySimulation(T(g["pos"]), T(g["vel"]), T(g["mass"]), precision_mode=nb.PrecisionMode(mode))
        m = metrics.SimulationMetrics()
        metrics.collect_metrics(sim, 0, m)
        sim.run(30, callback=lambda s, t: metrics.collect_metrics(s, t, m), callback_interval=10)
        assert m.ticks == list(g[f"{mode}/ticks"])
        for f in ("total_energy", "kinetic_energy", "potential_energy", "galaxy_radius_90", "velocity_dispersion"):
            got, want = np.array(getattr(m, f)), g[f"{mode}/{f}"]
            assert np.abs(got - want).max() <= max(tol, 2e-6) * np.abs(want).max(), (mode, f, got, want)
        assert np.abs(np.array(m.bound_fraction) - g[f"{mode}/bound_fraction"]).max() <= 1.0 / 300 + 1e-9
        rc_v = np.array([rc["velocities"] for rc in m.rotation_curves])
        rc_n = np.array([rc["num_stars_per_bin"] for rc in m.rotation_curves])
        assert np.array_equal(rc_n, g[f"{mode}/rc_n"])
        assert np.allclose(rc_v, g[f"{mode}/rc_v"], rtol=max(tol, 5e-6), equal_nan=True)
        finals[mode] = m.rotation_curves[-1]
    cmp_ = metrics.compare_rotation_curves(finals["float64"], finals["int4_sim"])
    assert int(cmp_["num_valid_bins"]) == int(g["compare/num_valid_bins"])
    for key in ("outer_slope_baseline", "outer_slope_quantized"):
        assert abs(cmp_[key] - float(g[f"compare/{key}"])) <= 1e-4 * abs(float(g[f"compare/{key}"])), key
    assert abs(cmp_["mean_velocity_diff"] - float(g["compare/mean_velocity_diff"])) <= 2e-6


def test_several_simulations_at_once_are_independent(nb):
    """realtime_visual.py:75-109 keeps several simulations alive and steps them in turn: handles share nothing, so
    interleaved stepping -- and one Python thread per simulation (ctypes releases the GIL) -- gives the same bits
    as running each simulation alone."""
    import threading
    from nbody_cosmological_simulation_amd import checkpoint, galaxy
    modes = ["float64", "float32", "int4", "float16", "int8", "custom"]
    pos, vel, mass = galaxy.create_disk_galaxy(3000, seed=1, device="cpu")

    def fresh(m):
        return nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.get_mode_from_string(m))

    alone = {}
    for m in modes:
        s = fresh(m)
        s.run(60)
        alone[m] = checkpoint.state_hash(s)
        s.close()
    sims = {m: fresh(m) for m in modes}
    for _ in range(20):
        for m in modes:
            sims[m].run(3)
    assert {m: checkpoint.state_hash(s) for m, s in sims.items()} == alone
    sims = {m: fresh(m) for m in modes}
    threads = [threading.Thread(target=lambda s=s: [s.run(5) for _ in range(12)]) for s in sims.values()]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert {m: checkpoint.state_hash(s) for m, s in sims.items()} == alone


# --------------------------------------------------------------------------- round 2: bins pinned to the reference at scale
G13 = ["g13_bins_n4096_d2.npz", "g13_bins_n2048_d3.npz"]


def _row_crcs(bins):
    import zlib
    b = np.ascontiguousarray(np.asarray(bins).astype("<i2"))
    return np.array([zlib.crc32(b[i].tobytes()) for i in range(b.shape[0])], np.uint32)


@pytest.mark.parametrize("fname", G13)
@pytest.mark.parametrize("mode", GRID)
def test_g13_bins_at_scale_vs_reference(nb, fname, mode):
    """The HIP path against quant-bin assignments produced by the REFERENCE at N = 4096 (D = 2, pruned max-r2
    search is off, tiles of 128) and N = 2048 (D = 3, unequal masses, softening^2 below the grid floor so the clamp
    variant of the table-free path runs): CRC-32 of every row of the bin matrix, histogram, lmin / lmax, force grid."""
    g = load_golden(fname)
    sim = mk(nb, g, mode)
    dbg = sim.quant_debug(bins=True)
    assert np.float32(dbg["lmin"]) == np.float32(g[f"{mode}/lmin"])
    assert np.float32(dbg["lmax"]) == np.float32(g[f"{mode}/lmax"])
    levels = {"int8_sim": 256, "int4_sim": 16, "custom": 64}[mode]
    assert np.array_equal(np.bincount(dbg["d2bins"].ravel(), minlength=levels), g[f"{mode}/hist"])
    assert np.array_equal(_row_crcs(dbg["d2bins"]), g[f"{mode}/row_crc"]), "a row of bins differs from the reference"
    assert dbg["fast_path"], "the table-free pair path should be active here"
    assert dbg["fast_maxrel"] <= 2e-6 and dbg["fast_maxdev"] < 1e-3
    acc = sim.accelerations.numpy()
    ref = g[f"{mode}/acc0"]
    if mode == "custom":
        assert relerr(acc, ref) < 2e-6
    else:
        flips = int((dbg["fbins"] != g[f"{mode}/fbins"]).sum())
        print(f"{fname} {mode}: force-bin flips {flips} of {ref.size}")
        assert flips <= 6
        assert abs(dbg["fmin"] - float(g[f"{mode}/fmin"])) <= 2e-6 * abs(float(g[f"{mode}/fmin"]))
        assert abs(dbg["fmax"] - float(g[f"{mode}/fmax"])) <= 2e-6 * abs(float(g[f"{mode}/fmax"]))
        step = (float(g[f"{mode}/fmax"]) - float(g[f"{mode}/fmin"])) / (levels - 1)
        assert np.abs(acc.astype(np.float64) - ref).max() <= 1.01 * step


def test_config2_full_size_step_and_energies_vs_reference_ops(nb):
    """g17: BASELINE config 2 at its real size against the reference's own arithmetic -- N = 65 536, FLOAT64 mode, fp32
    initial conditions: the first force evaluation, one full leapfrog step (positions, velocities, second force
    evaluation) on 2048 sampled rows, and the kinetic / potential energies before and after, all from the reference's
    torch expressions evaluated on row blocks (tests/golden/make_golden.py g17; the reference itself cannot hold the
    N x N tensors).  north_star asks for 1e-10; 1e-12 is asserted."""
    g = load_golden("g17_step_n65536.npz")
    pos = torch.from_numpy(load_golden("g16_bins_n65536_rows.npz")["pos"])
    n = pos.shape[0]
    sim = nb.GalaxySimulation(pos, torch.zeros_like(pos), torch.ones(n), precision_mode=nb.PrecisionMode.FLOAT64)
    rows = g["rows"]
    assert str(sim.accelerations.dtype) == str(g["dtypes"][0]) and sim.positions.dtype == torch.float32
    a_scale, x_scale = np.abs(g["acc0"]).max(), np.abs(g["pos1"]).max()
    assert np.abs(sim.accelerations.numpy()[rows] - g["acc0"]).max() <= 1e-13 * a_scale
    assert sim.get_kinetic_energy() == g["e0"][0]
    # before the first step the state is fp32-typed: the reference's own PE is an fp32 sum of fp32 terms there (the
    # golden adds the same fp32 terms in fp64), so fp32 accuracy is the meaningful bar; after the step everything is fp64
    assert abs(sim.get_potential_energy() - g["e0"][1]) <= 2e-6 * abs(g["e0"][1])
    sim.step()
    assert [str(t.dtype) for t in (sim.positions, sim.velocities, sim.accelerations)] == [str(d) for d in g["dtypes"][1:]]
    assert np.abs(sim.positions.numpy()[rows] - g["pos1"]).max() <= 1e-13 * x_scale
    assert np.abs(sim.accelerations.numpy()[rows] - g["acc1"]).max() <= 1e-12 * a_scale
    assert np.abs(sim.velocities.numpy()[rows] - g["vel1"]).max() <= 1e-12 * np.abs(g["vel1"]).max()
    assert abs(sim.get_kinetic_energy() - g["e1"][0]) <= 1e-12 * abs(g["e1"][0])
    assert abs(sim.get_potential_energy() - g["e1"][1]) <= 1e-12 * abs(g["e1"][1])


@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim"])
def test_config3_full_size_force_quantisation_vs_reference_ops(nb, mode):
    """g18: INT8 / INT4 end to end at BASELINE config 3's real size -- the forces of every row at N = 65 536 from the
    reference's torch expressions on row blocks, then the reference's own quantize_force on the full (N, 2) tensor
    (tests/golden/make_golden.py g18).  The engine's force grid (fmin / fmax) to fp32 accuracy, and on 4096 sampled
    rows the force bins: a summed force that sits on a rounding boundary of the grid may land in the neighbouring bin
    (SURVEY.md section 7 hard part 2) -- at most a handful of the 8192 values, never further than one bin."""
    g = load_golden("g18_force_quant_n65536.npz")
    pos = torch.from_numpy(load_golden("g16_bins_n65536_rows.npz")["pos"])
    n = pos.shape[0]
    levels = 256 if mode == "int8_sim" else 16
    sim = nb.GalaxySimulation(pos, torch.zeros_like(pos), torch.ones(n), precision_mode=nb.PrecisionMode(mode))
    dbg = sim.quant_debug()
    fmin, fmax = float(g[f"{mode}/fmin"]), float(g[f"{mode}/fmax"])
    assert abs(dbg["fmin"] - fmin) <= 2e-6 * abs(fmin) and abs(dbg["fmax"] - fmax) <= 2e-6 * abs(fmax)
    rows = g["rows"]
    acc = sim.accelerations.numpy()[rows].astype(np.float64)
    step = (fmax - fmin) / (levels - 1)
    bins = np.rint((acc - dbg["fmin"]) / (dbg["fmax"] - dbg["fmin"]) * (levels - 1)).astype(np.int64)
    ref_bins = g[f"{mode}/fbins_rows"].astype(np.int64)
    flips = int((bins != ref_bins).sum())
    assert np.abs(bins - ref_bins).max() <= 1
    assert flips <= 8, flips
    assert np.abs(acc - g[f"{mode}/acc_rows"]).max() <= 1.01 * step
    same = bins == ref_bins
    assert np.abs(acc[same] - g[f"{mode}/acc_rows"][same]).max() <= 2e-6 * max(abs(fmin), abs(fmax))


def test_config3_full_size_bins_vs_reference_rows(nb):
    """g16: BASELINE config 3 at its real size, distance bins pinned to the REFERENCE itself -- six target rows at
    N = 65 536 (among them a row of the farthest pair, so the row block carries the global lmin / lmax) binned by the
    reference's own quantize_distance_squared (tests/golden/make_golden.py g16).  INT8 / INT4 / CUSTOM: lmin, lmax
    and every bin of every sampled row bit-identical (row CRCs); all seven modes: the accelerations of those rows
    against the reference's torch expressions evaluated on the row block."""
    import hashlib
    import zlib
    g = load_golden("g16_bins_n65536_rows.npz")
    pos = torch.from_numpy(g["pos"])              # the golden carries its positions (host-dependent last bits otherwise)
    assert hashlib.sha256(pos.numpy().tobytes()).hexdigest() == str(g["pos_sha256"])
    vel, mass = torch.zeros_like(pos), torch.ones(pos.shape[0])
    rows = [int(r) for r in g["rows"]]
    for mode in ("int8_sim", "int4_sim", "custom"):
        sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode))
        assert sim.force_kernel_name() == "force_sym_kernel<float"
        dbg = sim.quant_debug()
        assert np.float32(dbg["lmin"]) == np.float32(g[f"{mode}/lmin"]), mode
        assert np.float32(dbg["lmax"]) == np.float32(g[f"{mode}/lmax"]), mode
        assert np.float32(dbg["r2max"]) == np.float32(g["r2max"])
        for idx, r in enumerate(rows):
            k16 = np.ascontiguousarray(sim.quant_bins_rows(r, r + 1)[0].astype("<i2"))
            if r == 0:
                assert np.array_equal(k16[:4096], g[f"{mode}/row0_head"]), mode
            levels = {"int8_sim": 256, "int4_sim": 16, "custom": 64}[mode]
            assert np.array_equal(np.bincount(k16, minlength=levels), g[f"{mode}/row_hist"][idx]), (mode, r)
            assert zlib.crc32(k16.tobytes()) == int(g[f"{mode}/row_crc"][idx]), (mode, r)
        sim.close()
    # accelerations of the same rows against the reference's torch expressions on the row block (simulation.py:83-112);
    # INT8 / INT4: the golden stops before quantize_force, so the engine's snapped forces sit within half a grid step
    for mode in MODES:
        sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode))
        acc = sim.accelerations.numpy().astype(np.float64)[rows]
        ref = g[f"{mode}/acc_rows"]
        scale = np.abs(ref).max()
        if mode in ("int8_sim", "int4_sim"):
            dbg = sim.quant_debug()
            step = (float(dbg["fmax"]) - float(dbg["fmin"])) / ((256 if mode == "int8_sim" else 16) - 1)
            assert np.abs(acc - ref).max() <= 0.505 * step + 2e-6 * scale, (mode, np.abs(acc - ref).max(), step)
        else:
            tol = 1e-13 if mode == "float64" else 2e-6
            assert np.abs(acc - ref).max() <= tol * scale, (mode, np.abs(acc - ref).max() / scale)
        sim.close()


@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16", "int8_sim", "int4_sim", "custom"])
def test_config3_full_size_vs_oracle_on_row_samples(nb, mode):
    """BASELINE config 3 at its real size (N = 65 536 disk galaxy, every non-fp64 mode) against the ORACLE on
    three 2048-row target samples: accelerations, and for the grid modes the distance bins of those rows
    (bit-identical) with the global lmin / lmax.  INT8 / INT4 snap the summed forces to a grid whose bounds need
    every row; their rows are compared after snapping the oracle's rows to the engine's reported bounds."""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    n = 65536
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=42, device="cpu")
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode))
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    acc = sim.accelerations.numpy().astype(np.float64)
    grid = mode in GRID
    dbg = sim.quant_debug() if grid else None
    scale = np.abs(acc).max()
    for i0 in (0, n // 2 - 1000, n - 2048):
        ref, rdbg = O.accelerations_rows(pos.numpy(), mass.numpy(), mode, i0, i0 + 2048, bins=grid)
        ref = ref.astype(np.float64)
        if grid:
            assert np.float32(dbg["lmin"]) == np.float32(rdbg["lmin"]) and np.float32(dbg["lmax"]) == np.float32(rdbg["lmax"])
            assert np.array_equal(sim.quant_bins_rows(i0, i0 + 2048), rdbg["d2bins"].astype(np.int16)), \
                f"{mode}: distance bins of rows {i0}.. differ from the oracle"
        if mode in ("int8_sim", "int4_sim"):
            levels = 256 if mode == "int8_sim" else 16
            fmin, fmax = np.float32(dbg["fmin"]), np.float32(dbg["fmax"])
            r32 = ref.astype(np.float32)
            k = np.rint((r32 - fmin) / (fmax - fmin) * np.float32(levels - 1))
            snapped = (k / np.float32(levels - 1) * (fmax - fmin) + fmin).astype(np.float64)
            step = float(fmax - fmin) / (levels - 1)
            diff = np.abs(acc[i0:i0 + 2048] - snapped)
            assert diff.max() <= 1.01 * step                      # at most the neighbouring force bin
            assert (diff > 0.5 * step).mean() < 2e-3              # and only for values on a rounding boundary
            assert fmin <= r32.min() and fmax >= r32.max()        # the global bounds contain these rows
        else:
            assert np.abs(acc[i0:i0 + 2048] - ref).max() / scale < 2e-6


@pytest.mark.parametrize("mode", ["float64", "float32", "int8_sim"])
def test_three_dimensional_production_tiling_vs_oracle(nb, mode):
    """D = 3 at N >= 20 480: four targets per lane with the source tile swept in two halves (sym_rj) -- the
    production path of large 3-D systems.  Accelerations on row samples (all rows for the fp64 fast oracle), grid
    bins on row samples, three leapfrog steps in FLOAT64 mode."""
    from oracle import oracle as O
    n = 24576 + 77
    rng = np.random.default_rng(33)
    pos = (rng.standard_normal((n, 3)) * np.array([5.0, 5.0, 0.5])).astype(np.float32)
    vel = (rng.standard_normal((n, 3)) * 0.05).astype(np.float32)
    mass = np.ones(n, np.float32)
    if mode == "float64":
        p64, v64, m64 = pos.astype(np.float64), vel.astype(np.float64), mass.astype(np.float64)
        sim = nb.GalaxySimulation(T(p64), T(v64), T(m64), precision_mode=nb.PrecisionMode.FLOAT64)
        assert sim.force_kernel_name() == "force_sym_kernel<double"
        assert relerr(sim.accelerations.numpy(), O.accelerations_f64_fast(p64, m64)) < 1e-13
        ref = O.OracleSim(p64, v64, m64, "float64")
        sim.run(3)
        for _ in range(3):       # OracleSim's generic path is slow at this size: step with the fast fp64 force
            ref._vel = ref._vel + ref._acc * (ref.dt / 2)
            ref._pos = ref._pos + ref._vel * ref.dt
            ref._acc = O.accelerations_f64_fast(ref._pos, m64)
            ref._vel = ref._vel + ref._acc * (ref.dt / 2)
        assert relerr(sim.positions.numpy(), ref._pos) < 1e-13
        assert relerr(sim.velocities.numpy(), ref._vel) < 1e-12
        return
    sim = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode))
    assert sim.force_kernel_name() == "force_sym_kernel<float"
    acc = sim.accelerations.numpy().astype(np.float64)
    scale = np.abs(acc).max()
    for i0 in (0, n // 2, n - 1024):
        omode = "custom" if mode == "int8_sim" else mode
        ref, rdbg = O.accelerations_rows(pos, mass, omode, i0, i0 + 1024, levels=256 if mode == "int8_sim" else 0,
                                         bins=mode == "int8_sim")
        if mode == "int8_sim":
            assert np.array_equal(sim.quant_bins_rows(i0, i0 + 1024), rdbg["d2bins"].astype(np.int16))
            dbg = sim.quant_debug()
            step = (dbg["fmax"] - dbg["fmin"]) / 255
            assert np.abs(acc[i0:i0 + 1024] - ref.astype(np.float64)).max() <= 1.01 * step   # snapped to the force grid
        else:
            assert np.abs(acc[i0:i0 + 1024] - ref.astype(np.float64)).max() / scale < 2e-6


def test_config2_energy_drift_vs_oracle_200_ticks(nb):
    """BASELINE config 2 at a bounded horizon: N = 65 536 disk galaxy, FLOAT64 mode, 200 ticks against the oracle's
    OpenMP fp64 path from the same initial conditions -- |drift difference| < 1e-10 (north_star's bar; measured
    ~1e-14) and positions within 1e-10 of the system size.  (Beyond ~900 ticks at this N any two summation orders
    decorrelate; this is the horizon where the bar is meaningful.)"""
    from oracle import oracle as O
    from nbody_cosmological_simulation_amd import galaxy
    n, ticks = 65536, 200
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=42, device="cpu")
    p, v, m = (np.ascontiguousarray(t.double().numpy()) for t in (pos, vel, mass))
    lib = O.lib()
    acc = np.empty_like(p)
    lib.nbo_accelerations_f64_fast(n, 2, O._dp(p), O._dp(m), 0.001, 0.1 ** 2, 0, n, O._dp(acc))

    def energy():
        return lib.nbo_kinetic_energy(n, 2, O.F64, O._dp(v), O.F64, O._dp(m)) + O.potential_energy_f64_fast(p, m)

    e0 = energy()
    lib.nbo_step_f64_fast(n, 2, O._dp(p), O._dp(v), O._dp(m), O._dp(acc), 0.001, 0.1 ** 2, 0.01, ticks)
    drift_ref = (energy() - e0) / abs(e0)
    sim = nb.GalaxySimulation(pos.double(), vel.double(), mass.double(), precision_mode=nb.PrecisionMode.FLOAT64)
    g0 = sim.get_total_energy()
    assert abs(g0 - e0) <= 1e-13 * abs(e0)
    sim.run(ticks)
    drift = (sim.get_total_energy() - g0) / abs(g0)
    print(f"config 2, {ticks} ticks: drift {drift:.12e} oracle {drift_ref:.12e} diff {abs(drift - drift_ref):.2e}")
    assert abs(drift - drift_ref) < 1e-10
    size = np.abs(p).max()
    assert np.abs(sim.positions.numpy() - p).max() / size < 1e-10
    assert np.abs(sim.velocities.numpy() - v).max() / np.abs(v).max() < 1e-9


# --------------------------------------------------------------------------- native diagnostics (nb_metrics)
def test_native_metrics_vs_reference_goldens(nb):
    """The HIP diagnostics (nb_metrics_tensors through metrics.py) on the reference's own galaxies (g6): rotation
    curve (20 bins / 7 bins with a fixed max radius), r90 / r50, bound fraction, velocity dispersion."""
    from nbody_cosmological_simulation_amd import metrics
    g = load_golden("g6_galaxy_metrics.npz")
    for name in ("disk", "test", "halo"):
        for dev in ("cpu", "cuda"):
            p, v, m = (torch.from_numpy(g[f"{name}/{k}"]).to(dev) for k in ("pos", "vel", "mass"))
            rc = metrics.compute_rotation_curve(p, v)
            assert np.allclose(rc["radii"], g[f"{name}/rc_r"], rtol=1e-6)
            assert list(rc["num_stars_per_bin"]) == list(g[f"{name}/rc_n"])
            assert np.allclose(rc["velocities"], g[f"{name}/rc_v"], rtol=2e-6, equal_nan=True)
            rc7 = metrics.compute_rotation_curve(p, v, num_bins=7, max_radius=12.5)
            assert np.allclose(rc7["velocities"], g[f"{name}/rc7_v"], rtol=2e-6, equal_nan=True)
            assert abs(metrics.compute_galaxy_radius(p, 90) - float(g[f"{name}/r90"])) <= 1e-6 * float(g[f"{name}/r90"])
            assert abs(metrics.compute_galaxy_radius(p, 50) - float(g[f"{name}/r50"])) <= 1e-6 * float(g[f"{name}/r50"])
            assert abs(metrics.compute_bound_fraction(p, v, m, 0.001) - float(g[f"{name}/bound"])) <= 1e-6
            assert abs(metrics.compute_velocity_dispersion(v) - float(g[f"{name}/disp"])) <= 2e-6 * float(g[f"{name}/disp"])


@pytest.mark.parametrize("n,dtype", [(65536, "float32"), (65536, "float64"), (3001, "float32")])
def test_native_metrics_vs_oracle_at_scale(nb, n, dtype):
    """nb_metrics on an engine's device-resident state (collect_metrics' path) and nb_metrics_tensors against the
    numpy restatement at config 3's size: bin counts identical, means / r90 / dispersion to rounding, bound
    fraction exact for unit masses; unequal masses and non-finite stars (NaN position: no bin; infinite speed:
    its own bin only)."""
    from oracle import metrics_oracle as MO
    from nbody_cosmological_simulation_amd import galaxy, metrics
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=9, device="cpu")
    npdt = np.float64 if dtype == "float64" else np.float32
    if dtype == "float64":
        pos, vel, mass = pos.double(), vel.double(), mass.double()
    mode = nb.PrecisionMode.FLOAT64 if dtype == "float64" else nb.PrecisionMode.FLOAT32
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode)
    sim.run(2)
    m = metrics.SimulationMetrics()
    metrics.collect_metrics(sim, sim.tick, m)
    p, v, ms = sim.positions.numpy().astype(npdt), sim.velocities.numpy().astype(npdt), sim.masses.numpy().astype(npdt)
    edges = torch.linspace(0, float(MO.radii(p).max()), 21).numpy()
    ref = MO.rotation_curve(p, v, edges=edges)
    got = m.rotation_curves[0]
    assert got["num_stars_per_bin"] == ref["num_stars_per_bin"]
    assert np.allclose(got["velocities"], ref["velocities"], rtol=2e-6, equal_nan=True)
    assert m.galaxy_radius_90[0] == MO.galaxy_radius(p, 90)                 # an order statistic: exact
    assert m.bound_fraction[0] == MO.bound_fraction(p, v, ms, sim.G)        # unit masses: exact enclosed masses
    assert abs(m.velocity_dispersion[0] - MO.velocity_dispersion(v)) <= 2e-6 * MO.velocity_dispersion(v)
    # tensor-level entry, unequal masses, awkward stars
    rng = np.random.default_rng(n)
    ms2 = (0.5 + rng.random(n)).astype(npdt)
    bf = metrics.compute_bound_fraction(torch.from_numpy(p), torch.from_numpy(v), torch.from_numpy(ms2), 0.001)
    assert abs(bf - MO.bound_fraction(p, v, ms2, 0.001)) <= 3.0 / n       # fp32 cumsum order: a borderline star or two
    v2, p2 = v.copy(), p.copy()
    v2[5, 1] = np.inf
    p2[17, 0] = np.nan
    rc = metrics.compute_rotation_curve(torch.from_numpy(p2).cuda(), torch.from_numpy(v2).cuda(), num_bins=5, max_radius=10.0)
    ref2 = MO.rotation_curve(p2, v2, num_bins=5, max_radius=10.0, edges=torch.linspace(0, 10.0, 6).numpy())
    assert rc["num_stars_per_bin"] == ref2["num_stars_per_bin"]
    assert np.allclose(rc["velocities"], ref2["velocities"], rtol=2e-6, equal_nan=True)
    assert np.isinf(rc["velocities"]).sum() == 1


def test_shape_checks_before_native_calls(nb):
    """A rebound state tensor of another shape must raise before the native copy (which trusts N x D)."""
    g = load_golden("g1_n64_d2_e0.1.npz")
    sim = mk(nb, g, "float64")
    sim.positions = sim.positions[:10]
    with pytest.raises(ValueError):
        sim.step()
    sim = mk(nb, g, "float32")
    sim.masses = torch.ones(65)
    with pytest.raises(ValueError):
        sim.get_potential_energy()


def test_tensor_hooks_follow_the_callers_stream(nb):
    """The handle-less hooks queue on torch's current stream and do not synchronise for device tensors: a hook
    called under a side stream right after the producer kernel on that stream must see the producer's data."""
    if not torch.cuda.is_available():
        pytest.skip("needs torch's HIP device")
    from nbody_cosmological_simulation_amd import quantization as Q
    side = torch.cuda.Stream()
    x = torch.rand(1 << 20, device="cuda") * 50 + 0.02
    with torch.cuda.stream(side):
        y = x * 2.0                               # producer on the side stream
        q = Q._grid_quantize_safe(y, 64)
        z = q + 0.0                               # consumer on the side stream
    side.synchronize()
    ref = Q._grid_quantize_safe((x * 2.0).cpu(), 64)
    assert torch.equal(z.cpu(), ref)
    for _ in range(3):                            # repeated calls reuse the cached scratch
        assert torch.equal(Q._grid_quantize_safe(x, 256).cpu(), Q._grid_quantize_safe(x.cpu(), 256))


# --------------------------------------------------------------------------- dtype combinations beyond the scripts (g15)
_G15_TAGS = [f"{grp}/{m}" for grp in ("m64", "v64") for m in MODES] + \
            [f"{grp}/{m}" for grp in ("all64", "half", "bf16") for m in GRID]


@pytest.mark.parametrize("tag", _G15_TAGS)
def test_g15_dtype_combinations_vs_reference(nb, tag):
    """Every dtype combination the stock class accepts beyond what the scripts build, against the REFERENCE (g15):
    fp64 masses / fp64 velocities beside fp32 positions under all seven modes, the grid modes on fp64 state and on
    float16 / bfloat16 state.  dtype timeline identical; accelerations, energies and the state after three steps
    to fp32 rounding (1e-12 for the all-fp64 chains); INT8 / INT4 forces within one force-grid step."""
    g = load_golden("g15_dtype_combos.npz")
    assert int(g[f"{tag}/ok"]) == 1
    grp, mode = tag.split("/")
    pos, vel, mass = T(g["pos"]), T(g["vel"]), T(g["mass"])
    if grp == "m64":
        mass = mass.double()
    elif grp == "v64":
        vel = vel.double()
    elif grp == "all64":
        pos, vel, mass = pos.double(), vel.double(), mass.double()
    elif grp == "half":
        pos, vel, mass = pos.half(), vel.half(), mass.half()
    else:
        pos, vel, mass = pos.bfloat16(), vel.bfloat16(), mass.bfloat16()
    sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode(mode), G=0.001, softening=0.1, dt=0.01)
    names = lambda: [str(t.dtype) for t in (sim.positions, sim.velocities, sim.masses, sim.accelerations)]
    assert names() == list(g[f"{tag}/dtypes0"])
    # (round 2 allowed 4e-3 / 2e-2 on half-typed state: the generic kernel rounded the scalars G and levels - 1 to the
    # half type, which torch does not do for scalars that multiply or divide -- root-caused in round 3; the half-typed
    # chains now meet the same fp32 bar as everything else)
    tol = 1e-12 if grp == "all64" else 2e-6
    acc = sim.accelerations.double().numpy()
    ref = g[f"{tag}/acc0"]
    if mode in ("int8_sim", "int4_sim") and f"{tag}/fmin" in g.files:
        levels = 256 if mode == "int8_sim" else 16
        step = (float(g[f"{tag}/fmax"]) - float(g[f"{tag}/fmin"])) / (levels - 1)
        diff = np.abs(acc - ref)
        assert diff.max() <= 1.01 * step + tol * np.abs(ref).max()
        frac = float((diff > 0.5 * step).mean())
        print(f"{tag}: force values in a neighbouring force bin: {frac:.4f}")
        if grp in ("half", "bf16"):
            # the bar is the REFERENCE's own figure under a reversed summation order (golden g21: 0 ... 0.26 % over
            # eight systems of this recipe), doubled, and never below two values
            noise = load_golden("g21_reference_self_noise.npz")
            ref_frac = max(float(noise[f"half/{grp}/{mode}/{si}/frac_gt_half_step"]) for si in range(8))
            assert frac <= max(2 * ref_frac, 2.0 / diff.size), (frac, ref_frac)
        else:
            assert frac < 0.02
    else:
        assert relerr(acc, ref) < tol, relerr(acc, ref)
    ke, pe = sim.get_kinetic_energy(), sim.get_potential_energy()
    etol = max(tol, 2e-6) if grp != "all64" else 1e-12
    assert abs(ke - float(g[f"{tag}/e0"][0])) <= etol * abs(float(g[f"{tag}/e0"][0]))
    assert abs(pe - float(g[f"{tag}/e0"][1])) <= etol * abs(float(g[f"{tag}/e0"][1]))
    sim.run(3)
    assert names() == list(g[f"{tag}/dtypes3"])
    ptol = tol if mode not in ("int8_sim", "int4_sim") else max(tol, 1e-4)      # force-bin flips: dt^2 * one grid step
    assert relerr(sim.positions.double().numpy(), g[f"{tag}/pos3"]) < ptol
    assert relerr(sim.velocities.double().numpy(), g[f"{tag}/vel3"]) < ptol


def test_custom_levels_beyond_the_tables(nb):
    """CUSTOM grids with more levels than the fused tables hold (sensitivity_test.py:149-162 sweeps to 65 536 and
    beyond) run on the per-pair generic path -- O(N) memory, no N x N tensor -- and agree with the oracle's
    restatement of the same evaluation."""
    from oracle import oracle as O
    g = load_golden("g1_n257_d2_e0.05.npz")
    for L in (5000, 65536):
        sim = mk(nb, g, "custom", custom_levels=L)
        assert sim.force_kernel_name() == "generic_force_kernel"
        ref = O.accelerations(g["pos"], g["mass"], "custom", softening=float(g["eps"]), levels=L)
        assert relerr(sim.accelerations.numpy(), ref) < 2e-6
        sim.run(2)
        assert np.isfinite(sim.positions.numpy()).all()


def test_two_rank_rccl_step_matches_single_gpu(nb):
    """A REAL multi-GPU step: two fresh ranks (one per GPU) through `python -m torch.distributed.run`, the snake-dealt
    pair-symmetric plan, the RCCL all-reduce of the force vectors, the deferred closing kick, the r2max / PE
    collectives.  Skipped on a one-GPU box (the per-rank plans are then covered by the virtual-shard and the 1-rank
    communicator tests).  FLOAT64 <= 1e-12 of the single-GPU trajectory, INT4 distance bins identical, every rank
    bit-identical to the other."""
    import subprocess
    import sys
    import tempfile
    nproc = int(os.environ.get("NB_TWO_RANK_NPROC", "2"))      # 1: plumbing check of this test's script on a one-GPU box
    if nb._native.device_count() < nproc:
        pytest.skip("needs two GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = r'''
import os, sys, json, hashlib
sys.path.insert(0, os.environ["NB_ROOT"])
import numpy as np, torch, torch.distributed as dist
rank, lr = int(os.environ["RANK"]), int(os.environ["LOCAL_RANK"])
torch.cuda.set_device(lr)
dist.init_process_group("nccl", device_id=torch.device("cuda", lr))
import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import runtime, galaxy
out = {}
trace = {}
for name, n, mode in (("f64", 9000, nb.PrecisionMode.FLOAT64), ("f32", 9000, nb.PrecisionMode.FLOAT32),
                      ("int4", 3000, nb.PrecisionMode.INT4_SIM), ("int4_big", 9000, nb.PrecisionMode.INT4_SIM)):
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=5, device="cpu")
    runtime.reset_distributed()
    single = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode, device=torch.device("cuda", lr))
    single.run(3)
    runtime.init_distributed(device=lr)
    multi = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode, device=torch.device("cuda", lr))
    multi.run(3)
    p1, p2 = single.positions.cpu().numpy().astype(np.float64), multi.positions.cpu().numpy().astype(np.float64)
    out[name] = {"relerr": float(np.abs(p1 - p2).max() / np.abs(p1).max()),
                 "energy": [single.get_total_energy(), multi.get_total_energy()],
                 "hash": hashlib.sha256(multi.positions.cpu().numpy().tobytes()).hexdigest()}
    single.close(); multi.close()
    if name in ("f64", "int4_big"):
        # a step() loop and run(3) of the RCCL step, state read after every step (tests/test_gpu_kick_paths.py): the
        # deferred closing kick; INT4: the exchange of fp64 sums, nb_launch_finish_sums64, then the finish launch
        code = {torch.float32: 2, torch.float64: 3}
        def grab(sim, key):
            cs = []
            for part, t in (("x", sim.positions), ("v", sim.velocities), ("a", sim.accelerations)):
                trace[f"{key}/{part}"] = t.detach().cpu().double().numpy()
                cs.append(code[t.dtype])
            return cs
        mk = lambda: nb.GalaxySimulation(pos, vel * 1e-3, mass, precision_mode=mode, device=torch.device("cuda", lr))
        sim = mk()
        codes, paths = [grab(sim, f"{name}/0")], []
        for i in range(3):
            sim.step(); paths.append(sim.step_path_name()); codes.append(grab(sim, f"{name}/{i + 1}"))
        sim.close()
        sim = mk(); sim.run(3); paths.append(sim.step_path_name()); codes.append(grab(sim, f"{name}/run")); sim.close()
        out[name]["trace"] = {"codes": codes, "paths": paths, "dt": sim.dt}
gathered = [None] * dist.get_world_size()
dist.all_gather_object(gathered, out)
runtime.shutdown()
dist.barrier()
dist.destroy_process_group()
if rank == 0:
    json.dump(gathered, open(os.environ["NB_OUT"], "w"))
    np.savez(os.environ["NB_OUT"] + ".trace.npz", **trace)
'''
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "two_rank.py")
        open(path, "w").write(script)
        outp = os.path.join(tmp, "out.json")
        env = dict(os.environ, NB_ROOT=root, NB_OUT=outp, HSA_ENABLE_IPC_MODE_LEGACY="0")
        if nproc == 1:
            env["NBODY_FORCE_COMM"] = "1"      # our 1-rank RCCL communicator beside torch's NCCL process group
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            env.pop(k, None)
        res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
                              "--master-addr", "127.0.0.1", "--master-port", "29731", path], env=env,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
        ranks = json.load(open(outp))
        arrays = dict(np.load(outp + ".trace.npz"))
    assert len(ranks) == nproc
    for name in ("f64", "f32", "int4", "int4_big"):
        a, b = ranks[0][name], ranks[-1][name]
        assert a["hash"] == b["hash"], f"{name}: the two ranks hold different states"
        tol = 1e-12 if name == "f64" else (2e-6 if name == "f32" else 1e-4)
        assert a["relerr"] < tol, (name, a["relerr"])
        assert abs(a["energy"][0] - a["energy"][1]) <= max(tol, 1e-12) * abs(a["energy"][0]) * (1 if name != "int4" and name != "int4_big" else 100)
    # the kick sites of the RCCL step bit for bit, the launch after the exchange of fp64 sums included
    import test_gpu_kick_paths as K
    K.check_multirank_trace(ranks[0], arrays, "rccl", K.RCCL_PATHS)


def test_direct_allreduce_virtual_ranks():
    """The direct all-reduce kernel with the geometry of a full node on ONE GPU: 1..8 virtual ranks inside one process
    (own shared regions and streams).  Sequential mode checks the slice / portion arithmetic for every rank count
    and ragged lengths; the whole-node mode runs the real epoch barriers between 2..8 ranks in one dispatch (co-resident
    by construction), 1 MiB to 4 MiB, ten rounds each; two ranks also as two dispatches on two streams.  (This test
    is what exposed that hipDeviceMallocUncached regions return stale data on this stack -- nb_p2p.hip.)"""
    import subprocess
    import sys
    script = r'''
import os, sys, ctypes as C
sys.path.insert(0, os.environ["NB_ROOT"])
from nbody_cosmological_simulation_amd import _native as N
L = N.lib()
bad, us = C.c_int32(0), C.c_double(0.0)
for P in (1, 2, 3, 5, 7, 8):
    for dt, counts in ((N.NB_F64, (1, 63, 64 * P + 1, 4099, 131072)), (N.NB_F32, (2, 130, 8198, 262144))):
        for count in counts:
            N.check(L.nb_comm_p2p_virtual_test(0, P, count, dt, 0, 2, 0.5, C.byref(bad), C.byref(us)))
            assert bad.value == 0, ("sequential", P, dt, count, bad.value)
print("sequential ok", flush=True)
lat = {}
for P in (2, 3, 4, 5, 8):
    # the whole virtual node in ONE dispatch (blockIdx.y = rank): co-resident by construction, real barriers.  A short
    # probe first: a barrier that cannot complete shows up as bad >= 1e6 within a second, before anything long is queued
    N.check(L.nb_comm_p2p_virtual_test(0, P, 4099, N.NB_F64, 2, 1, 0.5, C.byref(bad), None))
    assert bad.value == 0, ("node probe", P, bad.value)
    for dt, count in ((N.NB_F64, 131072), (N.NB_F64, 4099), (N.NB_F32, 262144), (N.NB_F64, 524288)):
        N.check(L.nb_comm_p2p_virtual_test(0, P, count, dt, 2, 10, 0.5, C.byref(bad), C.byref(us)))
        assert bad.value == 0, ("node", P, dt, count, bad.value)
        if count == 131072:
            lat[P] = round(us.value, 1)
    print("node ok", P, lat, flush=True)
# one stream (and one dispatch) per rank: two ranks always get distinct hardware queues
N.check(L.nb_comm_p2p_virtual_test(0, 2, 131072, N.NB_F64, 1, 6, 0.5, C.byref(bad), C.byref(us)))
assert bad.value == 0, ("streams", bad.value)
print("P2P-VIRTUAL-OK", lat)
'''
    env = dict(os.environ, NB_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600)
    assert "P2P-VIRTUAL-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    print(res.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("world", [2, 4])
def test_direct_allreduce_between_processes(nb, world):
    """The direct all-reduce of the force vectors (csrc/nb_p2p.hip) between `world` PROCESSES sharing this GPU:
    HIP IPC export / import, the collective self-test, then random vectors of several lengths and both element types,
    each compared bit for bit with the rank-ordered host sum (tests/tools/p2p_worker.py).  A one-GPU box cannot put
    xGMI between the ranks; the protocol, the memory ordering across processes and the setup code are the same."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NB_ROOT=root, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NBODY_FORCE_COMM", "NB_NO_P2P"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                          "--master-addr", "127.0.0.1", "--master-port", str(29741 + world),
                          os.path.join(root, "tests", "tools", "p2p_worker.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and f"P2P-OK {world}" in res.stdout, res.stdout[-2000:] + res.stderr[-6000:]


@pytest.mark.parametrize("world,variant", [(2, ""), (4, ""), (2, "deferred-kick"), (3, "rccl-shaped")])
def test_multi_rank_product_path_on_one_gpu(nb, world, variant, tmp_path):
    """The REAL multi-rank step on a one-GPU box: `world` processes share the GPU, each is one rank of the engine
    (nb_create with nranks = world: its own snake-dealt work plan, deferred kicks, force quantisation after the sum,
    potential-energy sum) and the direct all-reduce carries every sum (NB_COMM=direct -- RCCL refuses several ranks
    on one GPU).  FLOAT64 <= 1e-12 of the single-GPU trajectory after five steps, the fp32 family 2e-6, grid modes
    within their bin-flip bands; every rank ends with bit-identical state."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outp = str(tmp_path / "multirank.json")
    env = dict(os.environ, NB_ROOT=root, NB_OUT=outp, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NBODY_FORCE_COMM", "NB_NO_P2P", "NB_P2P", "NB_COMM", "NB_P2P_NO_KICK"):
        env.pop(k, None)
    if variant == "deferred-kick":
        env["NB_P2P_NO_KICK"] = "1"     # the sum without fused leapfrog work: closing kicks deferred into the next pack launch
    if variant == "rccl-shaped":
        env["NB_NO_P2P"] = "1"          # the step as it runs on RCCL (reduce -> in-place all-reduce of acc -> pack), with the
                                        # direct-only communicator's copy + all-reduce standing in for ncclAllReduce
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                          "--master-addr", "127.0.0.1", "--master-port", str(29761 + world + (10 if variant else 0)),
                          os.path.join(root, "tests", "tools", "multirank_worker.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0 and f"MULTIRANK-OK {world}" in res.stdout, res.stdout[-2000:] + res.stderr[-6000:]
    got = json.load(open(outp))
    assert got["label"].startswith("direct loads only")
    ranks = got["ranks"]
    assert len(ranks) == world
    for name, tol_x, tol_v in (("f64", 1e-12, 1e-11), ("f64_onesided", 1e-12, 1e-11), ("f64_n65536", 1e-12, 1e-11),
                               ("f64_d3_unequal", 1e-12, 1e-11), ("f32_unequal", 2e-6, 2e-5), ("f32", 2e-6, 2e-5),
                               ("f16", 2e-6, 2e-5), ("int4", 1e-4, 5e-2), ("int8_big", 1e-4, 5e-2)):
        a = ranks[0][name]
        for r in ranks[1:]:
            assert r[name]["hash"] == a["hash"], f"{name}: ranks hold different states"
        assert a["relerr_x"] < tol_x and a["relerr_v"] < tol_v, (name, a)
        etol = 1e-12 if name.startswith("f64") else (2e-6 if name in ("f32", "f16", "f32_unequal") else 1e-3)
        assert abs(a["energy"][0] - a["energy"][1]) <= etol * abs(a["energy"][0]), (name, a["energy"])
    # INT8 on the pair-symmetric path: the ranks exchange unrounded fp64 sums, so the all-reduce adds no fp32 rounding
    # before the forces are snapped to their grid (with fp32 partials a force bin flips here: 1.2e-6 / 3.9e-4)
    assert ranks[0]["int8_big"]["relerr_x"] < 1e-7 and ranks[0]["int8_big"]["relerr_v"] < 1e-6, ranks[0]["int8_big"]
    assert ranks[0]["f64"]["kernel"].startswith("force_sym_kernel<double")
    assert ranks[0]["f64_onesided"]["kernel"].startswith("force_f64")
    # the kick sites of the multi-rank step, bit for bit (tests/test_gpu_kick_paths.py): the leapfrog recurrence of a
    # step() loop given the engine's own accelerations, run(k) against that loop, and the site each call reports
    import test_gpu_kick_paths as K
    K.check_multirank_trace(ranks[0], np.load(outp + ".trace.npz"), variant, K.MULTIRANK_PATHS[variant])


def test_direct_allreduce_dead_peer_drains_within_its_timeout(nb):
    """The bounded wait of the direct all-reduce kernel, exercised once: two virtual ranks, the second
    one never launches.  The first must give up after timeout_s, raise its status word and drain -- the call returns
    (no hang), reports the timed-out rank, and the kernel works normally afterwards."""
    import ctypes
    import time
    from nbody_cosmological_simulation_amd import _native as N
    L = N.lib()
    bad, us = ctypes.c_int32(0), ctypes.c_double(0.0)
    t0 = time.perf_counter()
    N.check(L.nb_comm_p2p_virtual_test(0, 2, 131072, N.NB_F64, 3, 1, 0.5, ctypes.byref(bad), ctypes.byref(us)))
    took = time.perf_counter() - t0
    assert bad.value >= 1000000, bad.value                  # a barrier timed out and said so
    assert 0.4 < took < 10.0, took                          # ... after the timeout, not never
    N.check(L.nb_comm_p2p_virtual_test(0, 2, 131072, N.NB_F64, 2, 3, 2.0, ctypes.byref(bad), ctypes.byref(us)))
    assert bad.value == 0


@pytest.mark.parametrize("scenario", ["dead-peer", "vote-no"])
def test_direct_allreduce_failure_paths(nb, scenario, tmp_path):
    """Error paths of the opt-in direct all-reduce with two PROCESSES on the one GPU (tests/tools/p2p_failure_worker.py):
    a peer that never joins a step -> the kernels drain after NB_P2P_TIMEOUT_S and positions / energy / synchronize raise
    NB_ERR_COMM (never garbage); a self-test that fails on one rank -> every rank votes the path down, nobody hangs.
    Either way the single-GPU engine afterwards is bit-identical to before."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outp = str(tmp_path / "p2p_failure.json")
    env = dict(os.environ, NB_ROOT=root, NB_OUT=outp, HSA_ENABLE_IPC_MODE_LEGACY="0", NB_SCENARIO=scenario, NB_P2P_TIMEOUT_S="1.5")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "NBODY_FORCE_COMM", "NB_NO_P2P", "NB_P2P", "NB_COMM", "NB_P2P_NO_KICK",
              "NB_TEST_P2P_FAIL_RANK"):
        env.pop(k, None)
    if scenario == "vote-no":
        env["NB_TEST_P2P_FAIL_RANK"] = "1"
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", str(29791 + (1 if scenario == "vote-no" else 0)),
                          os.path.join(root, "tests", "tools", "p2p_failure_worker.py")], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0 and f"P2P-FAILURE-OK {scenario}" in res.stdout, res.stdout[-2000:] + res.stderr[-6000:]
    ranks = json.load(open(outp))
    assert len(ranks) == 2 and all(r["single_gpu_unaffected"] for r in ranks)
    if scenario == "dead-peer":
        errs = ranks[0]["errors"]
        for name in ("positions", "energy", "synchronize"):
            assert errs[name] != "no error" and errs[name][0] == -6 and "did not arrive" in errs[name][1], (name, errs[name])
        assert ranks[0]["seconds"] < 30.0                   # bounded: a few timeouts, not the 60 s default
    else:
        for r in ranks:
            assert r["p2p_state"] != 2 and "could not be set up" in r["setup"], r
            assert "injected" in r["log"], r


def test_failed_selftest_leaves_the_step_on_rccl():
    """NB_P2P=auto with a self-test that fails (injected): the vote turns the direct path down and RCCL carries the step --
    here with a 1-rank RCCL communicator, bit-identical to the communicator-less engine."""
    import subprocess
    import sys
    script = r'''
import os, sys
sys.path.insert(0, os.environ["NB_ROOT"])
import numpy as np
import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import runtime, galaxy, _native
pos, vel, mass = galaxy.create_disk_galaxy(9000, seed=5, device="cpu")
def run():
    s = nb.GalaxySimulation(pos, vel, mass, precision_mode=nb.PrecisionMode.FLOAT64)
    s.run(3)
    out = s.positions.numpy().copy(), s.get_total_energy()
    s.close()
    return out
x0, e0 = run()
os.environ.update(NBODY_FORCE_COMM="1", NB_P2P="auto", NB_TEST_P2P_FAIL_RANK="0")
runtime.init_distributed(device=0)
x1, e1 = run()
assert _native.lib().nb_comm_ready() == 1 and _native.lib().nb_comm_p2p_state() != 2, runtime._p2p_log
assert runtime.allreduce_label().startswith("RCCL") and "injected" in runtime.allreduce_label(), runtime.allreduce_label()
assert np.array_equal(x0, x1) and e0 == e1
runtime.shutdown()
print("VOTE-NO-RCCL-OK")
'''
    env = dict(os.environ, NB_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert "VOTE-NO-RCCL-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,d,unequal", [(1, 2, False), (65, 2, True), (1000, 3, False), (3000, 2, True), (4096, 2, False)])
def test_small_system_single_launch_step_vs_oracle(nb, monkeypatch, n, d, unequal, mode):
    """Systems up to N = 4096 step with ONE launch per step (nb_small.hip: the lanes of a wave share a target, no
    reduction kernel, positions ping-pong between two buffers; grid modes: max-r2 + tables + force + finish).
    Five steps in two native calls against the oracle stepping with the reference's operation order, and against the
    two-launch path of the same engine (NB_NO_SMALLN)."""
    from oracle import oracle as O
    rng = np.random.default_rng(1000 * n + d)
    pos = (rng.standard_normal((n, d)) * 4).astype(np.float32)
    vel = (rng.standard_normal((n, d)) * 0.05).astype(np.float32)
    mass = (0.5 + rng.random(n)).astype(np.float32) if unequal else np.ones(n, np.float32)
    if mode == "float64":
        pos, vel, mass = pos.astype(np.float64), vel.astype(np.float64), mass.astype(np.float64)

    def run():
        s = nb.GalaxySimulation(T(pos), T(vel), T(mass), precision_mode=nb.PrecisionMode(mode))
        s.run(3)
        s.run(2)
        return s
    sim = run()
    # one launch per step up to N = 3072 with fp32 state, 4096 with fp64 state (above, the tiled path is ahead)
    expect_small = n <= 3072 or mode == "float64"
    assert (sim.force_kernel_name() == "small_step_kernel") == expect_small
    ref = O.OracleSim(pos, vel, mass, mode)
    ref.run(5)
    monkeypatch.setenv("NB_NO_SMALLN", "1")
    old = run()
    assert old.force_kernel_name() != "small_step_kernel"
    p, v = sim.positions.numpy().astype(np.float64), sim.velocities.numpy().astype(np.float64)
    if mode == "float64":
        assert relerr(p, ref.positions) < 1e-13 and relerr(v, ref.velocities) < 1e-12
        assert relerr(p, old.positions.numpy()) < 1e-13
        assert abs(sim.get_total_energy() - ref.get_total_energy()) <= 1e-12 * abs(ref.get_total_energy())
    elif mode in ("int8_sim", "int4_sim", "custom"):
        # bins are identical for identical positions; a last-bit difference can move a pair (or a force component)
        # across a bin edge: isolated outliers, bounded (see test_grid_modes_trajectory_on_symmetric_path)
        err = np.abs(v - ref.velocities.astype(np.float64)).max(axis=1) / max(np.abs(ref.velocities).max(), 1e-30)
        assert np.quantile(err, 0.99) < (2e-6 if mode == "custom" else 2e-3)
        assert err.max() < (1e-3 if mode == "custom" else 5e-2)
        if n > 1:
            dbg = sim.quant_debug(bins=n <= 1000)
            sim_pos = sim.positions.numpy()
            _, rdbg = O.accelerations(sim_pos, mass, mode, debug=True)
            assert np.float32(dbg["lmax"]) == np.float32(rdbg["lmax"])
            if n <= 1000:
                assert np.array_equal(dbg["d2bins"], rdbg["d2bins"])      # bins of the CURRENT positions: bit-identical
    else:
        assert relerr(p, ref.positions) < 2e-6 and relerr(v, ref.velocities) < 2e-5
    # reproducible: same inputs, same bits
    monkeypatch.delenv("NB_NO_SMALLN")
    again = run()
    assert np.array_equal(again.positions.numpy(), sim.positions.numpy())
    # an in-place edit between two native calls is picked up (omega_point_test.py:738)
    sim.positions[0] += 0.25
    sim.run(1)
    assert np.isfinite(sim.positions.numpy()).all()


def test_native_metrics_edge_cases(nb):
    """nb_metrics on awkward inputs against the numpy restatement: D = 3 (the plane is columns 0, 1; radii use all
    three), a single star, two stars, coincident stars (ties in both rankings), percentile 0 / 100."""
    from oracle import metrics_oracle as MO
    from nbody_cosmological_simulation_amd import metrics
    rng = np.random.default_rng(5)
    cases = {
        "d3": ((rng.standard_normal((700, 3)) * 3).astype(np.float32), (rng.standard_normal((700, 3)) * 0.2).astype(np.float32)),
        "one": (np.array([[1.5, -2.0]], np.float32), np.array([[0.1, 0.2]], np.float32)),
        "two": (np.array([[1.0, 0.0], [-3.0, 0.5]], np.float32), np.array([[0.0, 0.3], [0.1, -0.1]], np.float32)),
        "ties": (np.repeat(np.array([[2.0, 1.0], [0.5, -0.5], [4.0, 0.0]], np.float32), 5, axis=0),
                 np.tile(np.array([[0.05, 0.1]], np.float32), (15, 1))),
    }
    for name, (p, v) in cases.items():
        n = p.shape[0]
        m = np.ones(n, np.float32)
        for pct in (0, 50, 90, 100):
            assert metrics.compute_galaxy_radius(T(p), pct) == MO.galaxy_radius(p, pct), (name, pct)
        assert metrics.compute_bound_fraction(T(p), T(v), T(m), 0.001) == MO.bound_fraction(p, v, m, 0.001), name
        if n > 1:
            d = MO.velocity_dispersion(v)
            assert abs(metrics.compute_velocity_dispersion(T(v)) - d) <= 2e-6 * max(d, 1e-30) + 1e-12, name
            rmax = float(MO.radii(p).max())
            rc = metrics.compute_rotation_curve(T(p), T(v), num_bins=6)
            ref = MO.rotation_curve(p, v, num_bins=6, edges=torch.linspace(0, rmax, 7).numpy())
            assert rc["num_stars_per_bin"] == ref["num_stars_per_bin"], name
            assert np.allclose(rc["velocities"], ref["velocities"], rtol=2e-6, equal_nan=True), name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_snapshot_round_trip_of_half_typed_state_at_tick_zero(nb, tmp_path, dtype):
    """A snapshot taken before the first step of a half-typed simulation (the state is still bfloat16 / float16) can
    be hashed, stored and restored: identical dtypes, hash and continuation (state_hash used to raise on
    bfloat16)."""
    from nbody_cosmological_simulation_amd import checkpoint
    g = load_golden("g1_n64_d2_e0.1.npz")
    kw = dict(precision_mode=nb.PrecisionMode.FLOAT32, G=0.001, softening=0.1, dt=0.01)
    sim = nb.GalaxySimulation(T(g["pos"]).to(dtype), T(g["vel"]).to(dtype), T(g["mass"]).to(dtype), **kw)
    assert sim.positions.dtype == dtype
    path = str(tmp_path / "snap.npz")
    h = checkpoint.save_snapshot(sim, path)
    assert h == checkpoint.state_hash(sim) and len(h) == 16
    back = checkpoint.load_snapshot(path)
    assert back.positions.dtype == dtype and back.masses.dtype == dtype
    assert checkpoint.state_hash(back) == h
    sim.run(3)
    back.run(3)
    assert torch.equal(sim.positions, back.positions) and torch.equal(sim.velocities, back.velocities)


@pytest.mark.gpu
def test_handle_cache_reuse_is_invisible(nb):
    """Closed handles leave their stream and device allocation in the library's bounded cache (nb_cache_trim): a
    simulation built on a reused allocation -- stale contents of a DIFFERENT mode and size -- must give bit-identical
    results to one built on fresh memory, and the trim must hand the memory back."""
    from nbody_cosmological_simulation_amd import galaxy, runtime
    runtime.trim_cache()
    pos, vel, mass = galaxy.create_disk_galaxy(1500, seed=5, device="cpu")

    def run(mode):
        sim = nb.GalaxySimulation(pos, vel, mass, precision_mode=mode)
        sim.run(20)
        out = (sim.positions.clone(), sim.velocities.clone(), sim.get_total_energy())
        sim.close()
        return out

    fresh = {m: run(m) for m in (nb.PrecisionMode.FLOAT64, nb.PrecisionMode.INT8_SIM, nb.PrecisionMode.FLOAT32)}
    assert runtime.trim_cache() > 0 and runtime.trim_cache() == 0
    # fill the cache with an allocation full of other data, then rerun every mode on reused memory
    p2, v2, m2 = galaxy.create_disk_galaxy(2500, seed=9, device="cpu")
    other = nb.GalaxySimulation(p2 * 3, v2, m2, precision_mode=nb.PrecisionMode.INT4_SIM)
    other.run(5)
    other.close()
    for m, (x0, v0, e0) in fresh.items():
        x1, v1, e1 = run(m)
        assert torch.equal(x0, x1) and torch.equal(v0, v1) and e0 == e1, m
    assert runtime.trim_cache() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [700, 6000])
@pytest.mark.parametrize("mode", ["float64", "float32", "bfloat16"])
def test_step_loop_speculation_is_dropped_by_every_write(nb, monkeypatch, mode, n):
    """A Python loop of step() takes the next step's drifted positions from the previous native call (nb_step.cpp:
    step_small for small systems, reduce_sym_kernel's mode 3 on the tiled path).  Every write in between -- dt, G,
    softening, positions, velocities, masses, accelerations, an explicit force evaluation, a potential-energy evaluation
    (it rewrites the packed positions) -- must void them: the same sequence with speculation switched off (NB_NO_SPEC)
    gives bit-identical results, and a step() loop equals one run() call bit for bit."""
    from nbody_cosmological_simulation_amd import galaxy
    pos, vel, mass = galaxy.create_disk_galaxy(n, seed=11, device="cpu")
    pm = nb.PrecisionMode(mode)

    def script(sim):
        out = []
        sim.step(); sim.step()
        sim.dt = 0.02
        sim.step(); out.append(sim.positions.clone())
        sim.G = 0.002
        sim.step()
        sim.velocities = sim.velocities * 0.5          # rebinding: uploaded before the next step
        sim.step(); out.append(sim.velocities.clone())
        sim.positions[:10] += 0.25                       # in-place edit of the downloaded tensor
        sim.step()
        out.append(torch.tensor([sim.get_total_energy()], dtype=torch.float64))
        sim.step()
        sim.softening_sq = 0.02
        sim.masses = sim.masses * 2.0
        sim.step(); out.append(sim.positions.clone())
        sim.accelerations = sim._compute_accelerations()
        sim.step(); sim.step()
        sim.dt = 0.01
        sim.run(3)
        sim.step()
        sim.step()
        out += [sim.positions.clone(), sim.velocities.clone(), sim.accelerations.clone()]
        return out

    spec = nb.GalaxySimulation(pos, vel, mass, precision_mode=pm)
    a = script(spec)
    monkeypatch.setenv("NB_NO_SPEC", "1")
    plain = nb.GalaxySimulation(pos, vel, mass, precision_mode=pm)
    monkeypatch.delenv("NB_NO_SPEC")
    b = script(plain)
    assert spec.force_kernel_name() == plain.force_kernel_name()
    assert (spec.force_kernel_name() == "small_step_kernel") == (n == 700)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # step() loop == run(): bit for bit, including across reads of the state
    s1 = nb.GalaxySimulation(pos, vel, mass, precision_mode=pm)
    s2 = nb.GalaxySimulation(pos, vel, mass, precision_mode=pm)
    for k in range(7):
        s1.step()
        if k == 3:
            _ = s1.get_kinetic_energy(), s1.positions
    s2.run(7)
    assert torch.equal(s1.positions, s2.positions) and torch.equal(s1.velocities, s2.velocities)
    assert torch.equal(s1.accelerations, s2.accelerations)
