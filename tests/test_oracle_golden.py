"""Pins the CPU oracle (oracle/) to golden vectors produced by RUNNING the reference
(tests/golden/make_golden.py).  CPU only.

Tolerances (relative to max|reference| of the compared array unless noted):
  * FLOAT64 mode: 1e-13 single evaluation / short runs (observed <= 1e-15), trajectory
    bounds follow the reference's own self-noise floor.
  * fp32-family modes: 1e-6 single evaluation (observed <= 3e-7: torch SLEEF pow/exp vs
    correctly rounded, and torch's fp32 cascade sum vs double accumulation).
  * distance-bin indices, lmin/lmax: bit-exact.  Force bins: mismatch count reported, and
    bounded (they depend on the fp32 summation order of the reference).
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from oracle import oracle as O

MODES = ["float64", "float32", "bfloat16", "float16", "int8_sim", "int4_sim", "custom"]
GRID = ["int8_sim", "int4_sim", "custom"]
G1 = ["g1_n64_d2_e0.1.npz", "g1_n257_d2_e0.05.npz", "g1_n64_d3_e0.01.npz", "g1_n257_d3_e0.1.npz"]


def relerr(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def tol_single(mode):
    return 1e-13 if mode == "float64" else 1e-6


@pytest.mark.parametrize("fname", G1)
@pytest.mark.parametrize("mode", MODES)
def test_g1_single_evaluation(fname, mode):
    g = load_golden(fname)
    eps = float(g["eps"])
    acc, dbg = O.accelerations(g["pos"], g["mass"], mode, softening=eps, debug=True)
    ref = g[f"{mode}/acc0"]
    assert acc.dtype == ref.dtype
    if mode in GRID:
        assert dbg["lmin"] == float(g[f"{mode}/lmin"])
        assert dbg["lmax"] == float(g[f"{mode}/lmax"])
        assert np.array_equal(dbg["d2bins"], g[f"{mode}/d2bins"])          # bit-identical bins
    if mode in ("int8_sim", "int4_sim"):
        assert relerr(dbg["acc_prequant"], g[f"{mode}/acc0_prequant"]) < 1e-6
        assert abs(dbg["fmin"] - float(g[f"{mode}/fmin"])) <= 1e-6 * abs(float(g[f"{mode}/fmin"]))
        assert abs(dbg["fmax"] - float(g[f"{mode}/fmax"])) <= 1e-6 * abs(float(g[f"{mode}/fmax"]))
        flips = int((dbg["fbins"] != g[f"{mode}/fbins"]).sum())
        assert flips <= 2, f"{flips} force-bin flips"
        if flips == 0:
            assert relerr(acc, ref) < 1e-6
    else:
        assert relerr(acc, ref) < tol_single(mode)


@pytest.mark.parametrize("fname", G1)
def test_g1_r2_bit_exact(fname):
    """fp32 distance-squared matrix (no FMA, reference op order) is bit-identical."""
    g = load_golden(fname)
    pos = g["pos"].astype(np.float32)
    diff = pos[None, :, :] - pos[:, None, :]
    sq = diff * diff
    s = sq[..., 0]
    for k in range(1, pos.shape[1]):
        s = s + sq[..., k]
    r2 = s + np.float32(float(g["eps"]) ** 2)
    assert np.array_equal(r2, g["r2_f32"])
    # and the oracle's own rounding model agrees with native float arithmetic
    out, bins, lmin, lmax = O.grid_quantize_safe(g["r2_f32"], 256, bins=True)
    assert np.array_equal(bins, g["int8_sim/d2bins"])


@pytest.mark.parametrize("fname", G1)
@pytest.mark.parametrize("mode", MODES)
def test_g1_step_and_energy(fname, mode):
    g = load_golden(fname)
    sim = O.OracleSim(g["pos"], g["vel"], g["mass"], mode, G=float(g["G"]), softening=float(g["eps"]),
                      dt=float(g["dt"]))
    tol = 1e-13 if mode == "float64" else 2e-6
    assert abs(sim.get_potential_energy() - float(g[f"{mode}/pe0"])) <= 2e-6 * abs(float(g[f"{mode}/pe0"]))
    assert abs(sim.get_kinetic_energy() - float(g[f"{mode}/ke0"])) <= 2e-6 * abs(float(g[f"{mode}/ke0"]))
    sim.step()
    assert sim.positions.dtype == g[f"{mode}/pos1"].dtype
    assert sim.velocities.dtype == g[f"{mode}/vel1"].dtype
    assert relerr(sim.positions, g[f"{mode}/pos1"]) < tol
    assert relerr(sim.velocities, g[f"{mode}/vel1"]) < tol
    if mode not in ("int8_sim", "int4_sim"):
        assert relerr(sim.accelerations, g[f"{mode}/acc1"]) < max(tol, 1e-6 if mode != "float64" else 0)
    sim.run(9)
    t10 = 1e-12 if mode == "float64" else (1e-5 if mode not in ("int8_sim", "int4_sim") else 2e-3)
    assert relerr(sim.positions, g[f"{mode}/pos10"]) < t10
    assert relerr(sim.velocities, g[f"{mode}/vel10"]) < t10 * 50


def test_g1_fp64_energy_exact():
    g = load_golden(G1[1])
    sim = O.OracleSim(g["pos"], g["vel"], g["mass"], "float64", softening=float(g["eps"]))
    # fp32 state at tick 0: energies are fp32-typed in the reference
    assert abs(sim.get_potential_energy() - float(g["float64/pe0"])) <= 1e-6 * abs(float(g["float64/pe0"]))
    sim.run(10)
    ke, pe = g["float64/e10"]
    assert abs(sim.get_kinetic_energy() - ke) <= 1e-13 * abs(ke)
    assert abs(sim.get_potential_energy() - pe) <= 1e-13 * abs(pe)


@pytest.mark.parametrize("L", [4, 64, 1000])
def test_g1c_custom_levels_override_semantics(L):
    """sensitivity_test.py:55-76 pattern == CUSTOM mode with `levels`, no force quantisation."""
    g = load_golden("g1c_custom_levels.npz")
    sim = O.OracleSim(g["pos"], g["vel"], g["mass"], "custom", levels=L)
    assert relerr(sim.accelerations, g[f"L{L}/acc0"]) < 1e-6
    sim.run(5)
    assert relerr(sim.positions, g[f"L{L}/pos5"]) < 1e-5


def test_g2_config1_fp64_trajectory():
    """Config 1 (N=1024, 200 ticks, float64): particle-level parity at every snapshot."""
    g = load_golden("g2_config1_n1024.npz")
    sim = O.OracleSim(g["pos"], g["vel"], g["mass"], "float64")
    scale = np.abs(g["float64/pos200"]).max()
    bounds = {0: 1e-15, 1: 1e-14, 10: 1e-13, 100: 1e-12, 200: 1e-11}   # reference self-noise: 1.2e-15 @200
    t = 0
    for snap in (0, 1, 10, 100, 200):
        sim.run(snap - t)
        t = snap
        assert np.abs(sim.positions.astype(np.float64) - g[f"float64/pos{snap}"]).max() / scale < bounds[snap]
        assert relerr(sim.velocities, g[f"float64/vel{snap}"]) < bounds[snap] * 100
        if snap in (0, 100, 200):
            for key, fn in (("ke", sim.get_kinetic_energy), ("pe", sim.get_potential_energy)):
                ref = float(g[f"float64/diag{snap}/{key}"])
                tol = 1e-6 if snap == 0 else 1e-12     # tick 0 energies are fp32-typed upstream
                assert abs(fn() - ref) <= tol * abs(ref)
    e0 = float(g["float64/diag100/e"])
    e1 = float(g["float64/diag200/e"])
    drift_ref = (e1 - e0) / abs(e0)
    # energy-drift parity (north_star: 1e-10)
    sim2 = O.OracleSim(g["pos"], g["vel"], g["mass"], "float64")
    sim2.run(100)
    a = sim2.get_total_energy()
    sim2.run(100)
    b = sim2.get_total_energy()
    assert abs((b - a) / abs(a) - drift_ref) < 1e-10


@pytest.mark.parametrize("mode", MODES[1:])
def test_g2_config1_other_modes_short_horizon(mode):
    g = load_golden("g2_config1_n1024.npz")
    sim = O.OracleSim(g["pos"], g["vel"], g["mass"], mode)
    sim.run(10)
    tol = 5e-6 if mode not in ("int8_sim", "int4_sim") else 5e-3
    assert relerr(sim.positions, g[f"{mode}/pos10"]) < tol


@pytest.mark.parametrize("n", [4096])
def test_g3_fast_path_matches_reference(n):
    g = load_golden(f"g3_fp64_n{n}.npz")
    pos, mass = g["pos"], g["mass"]
    # first evaluation in FLOAT64 mode uses fp32 d/r2: generic oracle
    acc0 = O.accelerations(pos[:512] if False else pos, mass, "float64")
    assert relerr(acc0, g["acc0"]) < 1e-13
    # all-fp64 fast path vs the generic restatement on the final (fp64) state
    pf = g["pos_final"]
    fast = O.accelerations_f64_fast(pf, mass.astype(np.float64))
    assert relerr(fast, g["acc_final"]) < 1e-13
    pe = O.potential_energy_f64_fast(pf, mass.astype(np.float64))
    assert abs(pe - g["e1"][1]) <= 1e-13 * abs(g["e1"][1])


def test_g3_n8192_final_forces():
    g = load_golden("g3_fp64_n8192.npz")
    fast = O.accelerations_f64_fast(g["pos_final"], g["mass"].astype(np.float64))
    assert relerr(fast, g["acc_final"]) < 1e-13


def test_g4_dtype_state_machine_and_mixed_inputs():
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    names = {O.F16: "torch.float16", O.BF16: "torch.bfloat16", O.F32: "torch.float32", O.F64: "torch.float64"}
    for mode in MODES:
        sim = O.OracleSim(g["pos"], g["vel"], g["mass"], mode)
        rows = [[names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3])]]
        for _ in range(2):
            sim.step()
            rows.append([names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3])])
        assert rows == api["dtype_timeline_fp32_inputs"][mode], mode
        # fp64 inputs
        sim = O.OracleSim(g["pos"].astype(np.float64), g["vel"].astype(np.float64),
                          g["mass"].astype(np.float64), mode)
        tol = 1e-13 if mode == "float64" else 1e-6
        if mode not in ("int8_sim", "int4_sim"):
            assert relerr(sim.accelerations, g[f"in64/{mode}/acc0"]) < tol, mode
        r0 = [names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3])]
        sim.run(3)
        r1 = [names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3])]
        assert [r0, r1] == api["dtype_timeline_fp64_inputs"][mode], mode
        if mode not in ("int8_sim", "int4_sim"):
            assert relerr(sim.positions, g[f"in64/{mode}/pos3"]) < 1e-6
            ke, pe = g[f"in64/{mode}/e3"]
            assert abs(sim.get_potential_energy() - pe) <= 1e-6 * abs(pe)
            assert abs(sim.get_kinetic_energy() - ke) <= 1e-5 * abs(ke)


@pytest.mark.parametrize("name,code", [("float16", O.F16), ("bfloat16", O.BF16)])
def test_g4_half_precision_state(name, code):
    """omega_point_test.py:722-733: f16/bf16 state tensors in FLOAT32 mode."""
    api = json.load(open(os.path.join(GOLDEN, "api.json")))
    g = load_golden("g4_api.npz")
    import torch
    tdt = getattr(torch, name)
    rd = lambda a: torch.from_numpy(a).to(tdt).float().numpy()   # values representable in the half type
    sim = O.OracleSim(rd(g["pos"]), rd(g["vel"]), rd(g["mass"]), "float32", codes=(code, code, code))
    ref = g[f"in_{name}/acc0"]
    assert relerr(sim.accelerations, ref) < 2e-6
    assert abs(sim.get_potential_energy() - float(g[f"in_{name}/pe0"])) <= 4e-3 * abs(float(g[f"in_{name}/pe0"]))
    sim.run(3)
    names = {O.F16: "torch.float16", O.BF16: "torch.bfloat16", O.F32: "torch.float32", O.F64: "torch.float64"}
    assert [names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3])] == \
        api["dtype_timeline_half_inputs_float32_mode"][name][1]
    assert relerr(sim.positions, g[f"in_{name}/pos3"]) < 1e-5


def test_g5_tensor_hooks():
    g = load_golden("g5_hooks.npz")
    d2, force = g["d2"], g["force"]
    for mode in MODES:
        out = O.quantize_distance_squared(d2, mode)
        ref = g[f"qd2/{mode}"]
        assert out.dtype == ref.dtype
        if mode in GRID:
            assert relerr(out, ref) < 1e-6
        else:
            assert np.array_equal(out, ref)          # casts are exact (inf on fp16 overflow too)
        outf = O.quantize_force(force, mode)
        reff = g[f"qf/{mode}"]
        if mode in GRID:
            assert relerr(outf, reff) < 1e-6
        else:
            assert np.array_equal(outf, reff)
    for L in (4, 16, 100, 1000):
        assert relerr(O.quantize_distance_squared(d2, "custom", custom_levels=L), g[f"qd2/custom{L}"]) < 1e-6
        assert relerr(O.grid_quantize_safe(d2, L, min_val=0.5), g[f"safe/L{L}_min0.5"]) < 1e-6
        assert relerr(O.grid_quantize(force, L), g[f"lin/L{L}"]) < 1e-6
    const = np.full((7, 7), 3.0, np.float32)
    assert np.array_equal(O.grid_quantize_safe(const, 16), g["safe/const"])
    assert np.array_equal(O.grid_quantize(const, 16), g["lin/const"])
    assert relerr(O.quantize_distance_squared(d2.astype(np.float64), "int8_sim"), g["qd2_64/int8_sim"]) < 1e-13
    assert np.array_equal(O.quantize_distance_squared(d2.astype(np.float64), "float16"), g["qd2_64/float16"])


def test_j_range_partials_sum_to_full():
    g = load_golden(G1[1])
    pos, mass = g["pos"], g["mass"]
    full = O.accelerations(pos, mass, "float64", softening=0.05)
    n = pos.shape[0]
    parts = [O.accelerations(pos, mass, "float64", softening=0.05, j_range=(a, b), force_quant=False)
             for a, b in ((0, 100), (100, 200), (200, n))]
    assert relerr(sum(parts), full) < 1e-14
    f64 = O.accelerations_f64_fast(pos.astype(np.float64), mass.astype(np.float64), softening=0.05)
    p64 = sum(O.accelerations_f64_fast(pos.astype(np.float64), mass.astype(np.float64), softening=0.05, j_range=r)
              for r in ((0, 128), (128, n)))
    assert relerr(p64, f64) < 1e-14


@pytest.mark.parametrize("mode", ["float64", "float32", "bfloat16", "float16"])
def test_torch_materialised_restatement_agrees(mode):
    """oracle/torch_materialised.py (used by bench.py as 'the reference's PyTorch-CPU path') reproduces the
    golden trajectory bit for bit in FLOAT64 mode and agrees with the C oracle in the cast modes."""
    import torch
    from oracle import torch_materialised as TM
    g = load_golden("g2_config1_n1024.npz")
    pos, vel, m = (torch.from_numpy(g[k]) for k in ("pos", "vel", "mass"))
    st = dict(pos=pos, vel=vel, masses=m)
    st["acc"] = TM.accelerations(pos, m, mode=mode)
    for _ in range(10):
        TM.step(st, mode=mode)
    ref = g[f"{mode}/pos10"]
    assert st["pos"].numpy().dtype == ref.dtype
    if mode == "float64":
        assert np.array_equal(st["pos"].numpy(), ref)
    else:
        assert relerr(st["pos"].numpy(), ref) < 1e-6


@pytest.mark.parametrize("n", [96, 700])
@pytest.mark.parametrize("hname,code", [("float16", O.F16), ("bfloat16", O.BF16)])
@pytest.mark.parametrize("mode", ["float32", "bfloat16", "float16", "float64"])
def test_g7_half_typed_state(n, hname, code, mode):
    """Half-typed state through every cast mode and FLOAT64 (reference run, g7): energies before the promotion
    (half arithmetic, incl. the float16 overflow of the N = 700 potential sum), after it (masses still half:
    mass products rounded to half, simulation.py:185), and the state after three steps."""
    g = load_golden("g7_half_state.npz")
    key = f"n{n}/{hname}/{mode}"
    sim = O.OracleSim(g[f"n{n}/{hname}/pos"], g[f"n{n}/{hname}/vel"], g[f"n{n}/{hname}/mass"], mode,
                      codes=(code, code, code))

    def close(got, want, tol):
        return got == want or abs(got - want) <= tol * abs(want)

    ke0, pe0 = g[key + "/e0"]
    assert close(sim.get_kinetic_energy(), ke0, 4e-3) and close(sim.get_potential_energy(), pe0, 8e-3)
    sim.run(3)
    ke3, pe3 = g[key + "/e3"]
    tol = 1e-12 if mode == "float64" else 2e-6
    assert close(sim.get_kinetic_energy(), ke3, max(tol, 1e-9)) and close(sim.get_potential_energy(), pe3, max(tol, 1e-9))
    assert relerr(sim.positions, g[key + "/pos3"]) < (1e-12 if mode == "float64" else 1e-5)
    assert relerr(sim.velocities, g[key + "/vel3"]) < (1e-10 if mode == "float64" else 1e-4)
    names = {O.F16: "torch.float16", O.BF16: "torch.bfloat16", O.F32: "torch.float32", O.F64: "torch.float64"}
    assert [names[c] for c in (sim.codes[0], sim.codes[1], sim.codes[3], sim.codes[2])] == list(g[key + "/dtypes3"])


def _g8_check(get_sim, key, g, f64):
    """Shared by the oracle (here) and the engine (tests/test_gpu_parity.py): one g8 case against the reference."""
    mode, eps, dt = key.split("/")
    eps, dt = float(eps[3:]), float(dt[2:])
    sim = get_sim(mode, eps, dt)
    wild = dt >= 1.0 and eps <= 1e-3          # 2-unit steps through 1e-4-softened encounters: rounding is amplified

    def same(got, want, tol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        if not np.array_equal(np.isnan(got), np.isnan(want)):
            return False
        ok = ~np.isnan(want)
        return ok.sum() == 0 or np.abs(got[ok] - want[ok]).max() <= tol * max(np.abs(want[ok]).max(), 1e-300)

    acc = sim.accelerations
    acc = acc.double().numpy() if hasattr(acc, "double") else acc
    assert same(acc, g[key + "/acc0"], 1e-13 if f64 else 2e-6), key
    # tick 0: the state is still fp32-typed in every mode (fp32 inputs), so the energies are fp32 sums
    assert same([sim.get_kinetic_energy(), sim.get_potential_energy()], g[key + "/e0"], 2e-6), key
    sim.run(5)
    pos, vel = sim.positions, sim.velocities
    pos = pos.double().numpy() if hasattr(pos, "double") else pos
    vel = vel.double().numpy() if hasattr(vel, "double") else vel
    tol = 5e-2 if (wild and not f64) else (1e-9 if f64 else 1e-5)
    assert same(pos, g[key + "/pos5"], tol), key
    assert same(vel, g[key + "/vel5"], tol * (1 if f64 or wild else 10)), key
    # (the bf16 / softening 1e-3 run gains 45x its kinetic energy in five steps: a half-precision rounding flip of
    # one close pair's r2 moves it by 1e-5)
    e_tol = 5e-2 if wild and not f64 else (1e-9 if f64 else 1e-4)
    assert same([sim.get_kinetic_energy()], [g[key + "/e5"][0]], e_tol), key
    assert same([sim.get_potential_energy()], [g[key + "/e5"][1]], e_tol), key


@pytest.mark.parametrize("idx", range(12))
def test_g8_parameter_extremes(idx):
    """crash_point_test.py / falsification_tests.py parameter ranges through the stock class: softening 0 (NaN
    forces and NaN potential, like the reference's masked 0/0), 1e-4 (NaN in FLOAT16 mode, where it underflows),
    1.0; dt up to 2.0; grid modes below their 0.01 clamp."""
    g = load_golden("g8_extremes.npz")
    key = str(g["cases"][idx])
    _g8_check(lambda mode, eps, dt: O.OracleSim(g["pos"], g["vel"], g["mass"], mode, G=0.001, softening=eps, dt=dt),
              key, g, key.startswith("float64"))


def _g9_check(get_sim, key, g):
    sname, mode = key.split("/")
    sim = get_sim(g[sname + "/pos"], g[sname + "/vel"], g[sname + "/mass"], mode)
    f64 = mode == "float64"

    def same(got, want, tol):
        got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
        if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
            return False
        ok = ~np.isnan(want)
        return ok.sum() == 0 or np.abs(got[ok] - want[ok]).max() <= tol * max(np.abs(want[ok]).max(), 1e-300)

    tonp = lambda t: t.double().numpy() if hasattr(t, "double") else t
    assert same(tonp(sim.accelerations), g[key + "/acc0"], 1e-13 if f64 else 2e-6), key
    assert same([sim.get_kinetic_energy(), sim.get_potential_energy()], g[key + "/e0"], 2e-6), key
    sim.run(2)
    assert same(tonp(sim.positions), g[key + "/pos2"], 1e-13 if f64 else 1e-6), key
    assert same(tonp(sim.velocities), g[key + "/vel2"], 1e-12 if f64 else 1e-6), key
    assert same([sim.get_kinetic_energy(), sim.get_potential_energy()], g[key + "/e2"], 1e-12 if f64 else 2e-6), key


@pytest.mark.parametrize("idx", range(35))
def test_g9_degenerate_systems(idx):
    """N = 1, 2, 3, five coincident particles, a massless particle in 3-D, every mode (reference run, g9)."""
    g = load_golden("g9_degenerate.npz")
    _g9_check(lambda p, v, m, mode: O.OracleSim(p, v, m, mode), str(g["cases"][idx]), g)


G23_GROUPS = [(dim, f64) for dim in (2, 3) for f64 in (False, True)]


@pytest.mark.parametrize("kind_idx", range(10))
@pytest.mark.parametrize("dim,f64", G23_GROUPS, ids=[f"d{d}-{'f64' if f else 'f32'}" for d, f in G23_GROUPS])
def test_g23_edge_values(dim, f64, kind_idx):
    """NaN / infinite / runaway coordinates, massless stars and a NaN mass (tests/edge_cases.py) through the stock class
    at N = 48, every mode (reference run, g23): the oracle puts NaN, +inf and -inf where the reference does and agrees on
    the finite values at g9's bars.  The inputs are the stored ones; edge_cases.make must still produce them."""
    import edge_cases as E
    g = load_golden("g23_edge_values.npz")
    kind = E.KINDS[kind_idx]
    assert list(g["kinds"]) == list(E.KINDS) and list(g["modes"]) == MODES
    grp = f"d{dim}/{'f64' if f64 else 'f32'}"
    pos, vel, mass = (g[f"{grp}/{name}"][kind_idx] for name in ("pos", "vel", "mass"))
    again = E.make(kind, 48, dim, 23 + dim, f64, idx=E.variants(kind, 48, every_index=False)[0])
    for a, b in zip((pos, vel, mass), again[:3]):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), (kind, grp)
    for m, mode in enumerate(MODES):
        row = kind_idx * len(MODES) + m
        sim = O.OracleSim(pos, vel, mass, mode)
        m64 = mode == "float64"
        what = f"{grp} {mode}"
        E.compare(sim.accelerations, g[f"{grp}/acc0"][row], 1e-13 if m64 else 2e-6, kind, what + " acc0")
        E.compare([sim.get_kinetic_energy(), sim.get_potential_energy()], g[f"{grp}/e0"][row], 2e-6, kind, what + " e0")
        sim.run(2)
        E.compare(sim.positions, g[f"{grp}/pos2"][row], 1e-13 if m64 else 1e-6, kind, what + " pos2")
        if kind in E.FAR_KINDS:      # the far coordinate is the array maximum: the other stars on their own
            rest = np.delete(np.arange(48), list(again[3]))
            E.compare(np.asarray(sim.positions)[rest], g[f"{grp}/pos2"][row][rest], 1e-13 if m64 else 1e-6, kind, what + " pos2 rest")
        E.compare(sim.velocities, g[f"{grp}/vel2"][row], 1e-12 if m64 else 1e-6, kind, what + " vel2")
        E.compare([sim.get_kinetic_energy(), sim.get_potential_energy()], g[f"{grp}/e2"][row], 1e-12 if m64 else 2e-6, kind,
                  what + " e2")


def test_edge_compare_counts_what_it_leaves_out():
    """compare() fails when the engine misses a NaN the oracle has (an edge value written where nothing reads it), when
    an infinity has the wrong sign, and when a finite value is off; the inf-coord allowance covers forces only."""
    import edge_cases as E
    ref = np.array([[1.0, np.nan], [np.inf, -2.0], [-np.inf, 0.5]])
    assert E.compare(ref.copy(), ref, 1e-13, "nan-coord") == 0.0
    for at, value in (((0, 1), 3.0), ((1, 0), -np.inf), ((2, 0), np.nan), ((0, 0), np.nan), ((2, 1), 0.5 + 1e-12)):
        got = ref.copy()
        got[at] = value
        with pytest.raises(AssertionError):
            E.compare(got, ref, 1e-13, "nan-coord")
    got = ref.copy()
    got[0, 0] = np.nan                                  # NaN where the oracle is finite: forces of inf-coord only
    assert E.compare(got, ref, 1e-13, "inf-coord", from_forces=True) == 0.0
    with pytest.raises(AssertionError):
        E.compare(got, ref, 1e-13, "inf-coord")
    got[0, 1] = 1.0                                     # ... and never finite where the oracle is NaN
    with pytest.raises(AssertionError):
        E.compare(got, ref, 1e-13, "inf-coord", from_forces=True)


def _g10_check(fns, g, name):
    """fns: (quantize_distance_squared, quantize_force, grid_quantize_safe, grid_quantize) taking numpy arrays."""
    qd2, qf, safe, lin = fns
    t = g["in/" + name]

    def same(got, want, tol=1e-6):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        a, b = got.astype(np.float64), want.astype(np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        inf = np.isinf(b)
        assert np.array_equal(a[inf], b[inf]), name
        ok = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), ok), name
        if ok.any():
            assert np.abs(a[ok] - b[ok]).max() <= tol * max(np.abs(b[ok]).max(), 1e-300), name

    for mode in MODES:
        same(qd2(t, mode), g[f"{name}/qd2/{mode}"])
        same(qf(t - np.float32(15.0), mode), g[f"{name}/qf/{mode}"])
    for L in (2, 3, 7):
        same(safe(t, L, 0.01), g[f"{name}/safe/L{L}"])
        same(lin(t - np.float32(15.0), L), g[f"{name}/lin/L{L}"])


@pytest.mark.parametrize("name", ["zero_neg_huge", "inf", "nan", "vec1d", "cube3d", "single"])
def test_g10_hook_edge_values(name):
    """Tensor-level hooks on zeros, negatives, 1e30, inf, NaN, 2-3 levels, 1-D / 3-D / one-element tensors (g10)."""
    g = load_golden("g10_hook_edges.npz")
    _g10_check((O.quantize_distance_squared, O.quantize_force, O.grid_quantize_safe, O.grid_quantize), g, name)


# --------------------------------------------------------------------------- G13: bins at scale, from the reference
G13 = ["g13_bins_n4096_d2.npz", "g13_bins_n2048_d3.npz"]


def row_crcs(bins):
    import zlib
    b = np.ascontiguousarray(np.asarray(bins).astype("<i2"))
    return np.array([zlib.crc32(b[i].tobytes()) for i in range(b.shape[0])], np.uint32)


@pytest.mark.parametrize("fname", G13)
@pytest.mark.parametrize("mode", GRID)
def test_g13_bins_at_scale_vs_reference(fname, mode):
    """Quant-bin assignments of the REFERENCE at N = 4096 (D = 2) / N = 2048 (D = 3, softening below the grid
    floor): every row of the N x N int16 bin matrix by CRC-32, the bin histogram, lmin / lmax, the force grid."""
    g = load_golden(fname)
    acc, dbg = O.accelerations(g["pos"], g["mass"], mode, softening=float(g["eps"]), debug=True)
    assert np.float32(dbg["lmin"]) == np.float32(g[f"{mode}/lmin"])
    assert np.float32(dbg["lmax"]) == np.float32(g[f"{mode}/lmax"])
    levels = {"int8_sim": 256, "int4_sim": 16, "custom": 64}[mode]
    assert np.array_equal(np.bincount(dbg["d2bins"].ravel(), minlength=levels), g[f"{mode}/hist"])
    assert np.array_equal(row_crcs(dbg["d2bins"]), g[f"{mode}/row_crc"]), "a row of bins differs from the reference"
    n = g["pos"].shape[0]
    for r in (0, n // 2, n - 1):
        assert np.array_equal(dbg["d2bins"][r].astype(np.int16), g[f"{mode}/row{r}"])
    if mode != "custom":
        flips = int((dbg["fbins"] != g[f"{mode}/fbins"]).sum())
        print(f"{fname} {mode}: force-bin flips {flips} of {dbg['fbins'].size}")
        assert flips <= 4
        assert abs(dbg["fmin"] - float(g[f"{mode}/fmin"])) <= 2e-6 * abs(float(g[f"{mode}/fmin"]))
        assert abs(dbg["fmax"] - float(g[f"{mode}/fmax"])) <= 2e-6 * abs(float(g[f"{mode}/fmax"]))
    else:
        assert relerr(acc, g[f"{mode}/acc0"]) < 2e-6


@pytest.mark.parametrize("fname", G13)
@pytest.mark.parametrize("mode", ["int8_sim", "int4_sim", "custom"])
def test_g20_bin_checksums_vs_reference(fname, mode):
    """The per-row integer checksums the HIP path's production pair loops report (nb_quant_bin_sums: sum_j k and
    sum_j k * ((j mod 65521) + 1)) computed from the ORACLE's bin matrix equal the ones make_golden.py g20 computed
    from the reference's bin matrix -- so the fixture and the checksum definition are pinned on the CPU too."""
    g = load_golden(fname)
    ref = load_golden("g20_bin_checksums.npz")
    case = fname[len("g13_bins_"):-len(".npz")]
    _, dbg = O.accelerations(g["pos"], g["mass"], mode, softening=float(g["eps"]), debug=True)
    k = dbg["d2bins"].astype(np.int64)
    assert np.all(np.diag(k) == 0)
    w = (np.arange(k.shape[1], dtype=np.int64) % 65521) + 1
    assert np.array_equal(k.sum(axis=1), ref[f"g13_{case}/{mode}/s1"])
    assert np.array_equal((k * w[None, :]).sum(axis=1), ref[f"g13_{case}/{mode}/s2"])


def test_torch_scalar_semantics_on_half_tensors():
    """What the oracle's scalar_as / scalar_mul (nbody_oracle.c) encode, measured on torch itself (no reference code
    involved): a Python scalar ADDED to a half tensor is rounded to the tensor's dtype first; a Python scalar that
    MULTIPLIES / DIVIDES one stays in float; G / t is t.reciprocal() times float(G)."""
    import torch
    torch.manual_seed(0)
    for dt in (torch.float16, torch.bfloat16):
        x = (torch.rand(50000) * 10 + 0.1).to(dt)
        f = x.float()
        assert torch.equal(x * 0.001, (f * np.float32(0.001)).to(dt))
        assert not torch.equal(x * 0.001, (f * torch.tensor(0.001).to(dt).float()).to(dt))
        assert torch.equal(x / 3.3, (f / np.float32(3.3)).to(dt))
        assert torch.equal(0.001 / x, (x.reciprocal().float() * np.float32(0.001)).to(dt))
        y = (torch.rand(50000) * 0.05).to(dt)
        assert torch.equal(y + 0.0123, (y.float() + torch.tensor(0.0123).to(dt).float()).to(dt))
        assert not torch.equal(y + 0.0123, (y.float() + np.float32(0.0123)).to(dt))


_G15_HALF = [(grp, mode) for grp in ("half", "bf16") for mode in ("int8_sim", "int4_sim", "custom")]


@pytest.mark.parametrize("grp,mode", _G15_HALF)
def test_g15_grid_modes_on_half_typed_state_vs_reference(grp, mode):
    """The grid modes on float16 / bfloat16 state tensors (g15: the stock class accepts them): every op of
    quantization.py:106-127 rounds to the half type.  With the scalar semantics above the oracle reproduces the
    reference's forces to fp32 summation level -- before round 3 both the oracle and the HIP path rounded G and
    (levels - 1) to the half type first and sat 4e-4 away, which the 4e-3 bar of round 2 hid."""
    g = load_golden("g15_dtype_combos.npz")
    tag = f"{grp}/{mode}"
    assert int(g[f"{tag}/ok"]) == 1
    code = O.F16 if grp == "half" else O.BF16
    import torch
    cast = (lambda a: torch.from_numpy(a).half().float().numpy()) if grp == "half" else \
           (lambda a: torch.from_numpy(a).bfloat16().float().numpy())
    pos, mass = cast(g["pos"]), cast(g["mass"])
    acc, dbg = O.accelerations(pos, mass, mode, softening=0.1, debug=True, pos_code=code, mass_code=code)
    ref = g[f"{tag}/acc0"]
    if mode == "custom":
        assert relerr(acc, ref) < 2e-6, relerr(acc, ref)
    else:
        levels = 256 if mode == "int8_sim" else 16
        step = (float(g[f"{tag}/fmax"]) - float(g[f"{tag}/fmin"])) / (levels - 1)
        diff = np.abs(np.asarray(acc, np.float64) - ref)
        frac = float((diff > 0.5 * step).mean())
        print(f"{tag}: force values off by more than half a grid step: {frac:.4f}, max {diff.max() / step:.3f} steps")
        assert abs(dbg["fmin"] - float(g[f"{tag}/fmin"])) <= 2e-6 * abs(float(g[f"{tag}/fmin"]))
        assert abs(dbg["fmax"] - float(g[f"{tag}/fmax"])) <= 2e-6 * abs(float(g[f"{tag}/fmax"]))
        noise = load_golden("g21_reference_self_noise.npz")
        ref_frac = max(float(noise[f"half/{grp}/{mode}/{si}/frac_gt_half_step"]) for si in range(8))
        assert frac <= max(2 * ref_frac, 2.0 / diff.size), (frac, ref_frac)
        assert diff.max() <= 1.01 * step


def test_g14_state_hash_matches_reference():
    """checkpoint.state_hash against hashes produced by the reference's reproducibility.hash_tensor_state."""
    import json
    import torch
    from nbody_cosmological_simulation_amd import checkpoint
    want = json.load(open(os.path.join(GOLDEN, "g14_state_hash.json")))
    g = load_golden("g2_config1_n1024.npz")
    pos, vel = torch.from_numpy(g["pos"]), torch.from_numpy(g["vel"])
    assert checkpoint.state_hash(pos, vel) == want["float32"]
    assert checkpoint.state_hash(pos.double(), vel.double()) == want["float64"]
    assert checkpoint.state_hash(pos.half(), vel.half()) == want["float16"]
    assert checkpoint.state_hash(torch.from_numpy(g["float64/pos200"]), torch.from_numpy(g["float64/vel200"])) == \
        want["float64_tick200"]
    # bfloat16 (numpy has no such dtype; upstream's .numpy() raises there): hashed over the raw 16-bit patterns
    hb = checkpoint.state_hash(pos.bfloat16(), vel.bfloat16())
    assert len(hb) == 16 and hb != want["float16"]


def test_metrics_oracle_vs_reference():
    """oracle/metrics_oracle.py (the checker of the native nb_metrics kernels) on the reference's own galaxies (g6):
    rotation curve (20 bins, and 7 bins with a fixed max radius), r90 / r50, bound fraction, velocity dispersion."""
    from oracle import metrics_oracle as MO
    g = load_golden("g6_galaxy_metrics.npz")
    for name in ("disk", "test", "halo"):
        p, v, m = (g[f"{name}/{k}"] for k in ("pos", "vel", "mass"))
        rc = MO.rotation_curve(p, v)
        assert np.allclose(rc["radii"], g[f"{name}/rc_r"], rtol=1e-6)
        assert list(rc["num_stars_per_bin"]) == list(g[f"{name}/rc_n"])
        assert np.allclose(rc["velocities"], g[f"{name}/rc_v"], rtol=2e-6, equal_nan=True)
        rc7 = MO.rotation_curve(p, v, num_bins=7, max_radius=12.5)
        assert np.allclose(rc7["velocities"], g[f"{name}/rc7_v"], rtol=2e-6, equal_nan=True)
        assert abs(MO.galaxy_radius(p, 90) - float(g[f"{name}/r90"])) <= 1e-6 * float(g[f"{name}/r90"])
        assert abs(MO.galaxy_radius(p, 50) - float(g[f"{name}/r50"])) <= 1e-6 * float(g[f"{name}/r50"])
        assert abs(MO.bound_fraction(p, v, m, 0.001) - float(g[f"{name}/bound"])) <= 1e-6
        assert abs(MO.velocity_dispersion(v) - float(g[f"{name}/disp"])) <= 2e-6 * float(g[f"{name}/disp"])


def test_metrics_oracle_non_finite_stars():
    """One star with a NaN position belongs to no bin and one with an infinite speed only spoils its own bin
    (the reference's per-bin masked means, metrics.py:62-68) -- what blown-up INT4 runs produce."""
    from oracle import metrics_oracle as MO
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((500, 2)) * 3).astype(np.float32)
    v = (rng.standard_normal((500, 2)) * 0.2).astype(np.float32)
    v[7, 1] = np.inf
    rc = MO.rotation_curve(p, v, num_bins=5, max_radius=10.0)
    assert np.isinf(rc["velocities"]).sum() == 1 and np.isfinite(rc["velocities"]).sum() == 4
    p[11, 0] = np.nan
    rc2 = MO.rotation_curve(p, v, num_bins=5, max_radius=10.0)
    assert sum(rc2["num_stars_per_bin"]) == sum(rc["num_stars_per_bin"]) - 1
    assert np.isfinite(rc2["velocities"]).sum() == 4

def test_oracle_bins_at_config3_size_vs_reference_rows():
    """g16: distance bins of six target rows at N = 65 536 (BASELINE config 3's real size) as the REFERENCE's own
    quantize_distance_squared assigns them (row block containing the farthest pair: global lmin / lmax; generator:
    tests/golden/make_golden.py g16).  The oracle's rows must match bit for bit -- INT8 here (the all-pairs scan for
    lmax is the cost: once), all three grid modes on the GPU."""
    import hashlib
    import zlib
    g = load_golden("g16_bins_n65536_rows.npz")
    import torch
    pos = torch.from_numpy(g["pos"])              # the golden carries its positions (host-dependent last bits otherwise)
    assert hashlib.sha256(pos.numpy().tobytes()).hexdigest() == str(g["pos_sha256"])
    mass = torch.ones(pos.shape[0])
    rows = [int(r) for r in g["rows"]]
    for mode in ("int8_sim",):
        for idx, r in enumerate(rows[:3] + rows[3:4]):
            ridx = rows.index(r)
            _, dbg = O.accelerations_rows(pos.numpy(), mass.numpy(), mode, r, r + 1, bins=True)
            assert np.float32(dbg["lmin"]) == np.float32(g[f"{mode}/lmin"]) and np.float32(dbg["lmax"]) == np.float32(g[f"{mode}/lmax"])
            k16 = np.ascontiguousarray(dbg["d2bins"][0].astype("<i2"))
            assert zlib.crc32(k16.tobytes()) == int(g[f"{mode}/row_crc"][ridx]), (mode, r)
            if idx == 0:
                break          # one all-pairs scan on the CPU is enough here; the GPU test checks every row and mode
    # accelerations of the sampled rows as the reference's torch expressions give them (simulation.py:83-112 on the row
    # block); the cast modes need no global scan
    p_np, m_np = pos.numpy(), mass.numpy()
    for mode, tol in (("float64", 1e-13), ("float32", 2e-6), ("bfloat16", 2e-6), ("float16", 2e-6)):
        ref = g[f"{mode}/acc_rows"]
        scale = np.abs(ref).max()
        for idx, r in enumerate(rows):
            got, _ = O.accelerations_rows(p_np, m_np, mode, r, r + 1)
            assert np.abs(got[0].astype(np.float64) - ref[idx]).max() <= tol * scale, (mode, r)


def test_oracle_first_evaluation_and_drift_at_config2_size_vs_reference_ops():
    """g17 (N = 65 536, FLOAT64 mode, fp32 initial conditions, zero velocities): the first force evaluation of 2048
    sampled rows and the positions after the opening kick + drift, against the reference's own torch expressions
    evaluated on row blocks (make_golden.py g17).  The full step and the energies need every row's force: GPU test."""
    import torch
    g = load_golden("g17_step_n65536.npz")
    pos = load_golden("g16_bins_n65536_rows.npz")["pos"]
    mass = np.ones(pos.shape[0], np.float32)
    rows = g["rows"]
    scale = np.abs(g["acc0"]).max()
    for i0 in range(0, len(rows), 256):                      # the oracle evaluates contiguous row ranges
        for r in rows[i0:i0 + 8]:                            # a few rows per block keep this a seconds-long test
            got, _ = O.accelerations_rows(pos, mass, "float64", int(r), int(r) + 1)
            idx = int(np.where(rows == r)[0][0])
            assert got.dtype == np.float64
            assert np.abs(got[0] - g["acc0"][idx]).max() <= 1e-13 * scale
            v_half = 0.0 + got[0] * (0.01 / 2)
            x1 = pos[r].astype(np.float64) + v_half * 0.01
            assert np.abs(x1 - g["pos1"][idx]).max() <= 1e-15 * np.abs(g["pos1"]).max()


def test_oracle_prequant_forces_at_config3_size_vs_reference_ops():
    """g18: the forces BEFORE quantize_force of two sampled rows at N = 65 536 in INT8 mode (reference's torch
    expressions on row blocks with the global grid bounds) against the oracle; the full force grid is a GPU test."""
    g = load_golden("g18_force_quant_n65536.npz")
    pos = load_golden("g16_bins_n65536_rows.npz")["pos"]
    mass = np.ones(pos.shape[0], np.float32)
    scale = np.abs(g["int8_sim/pre_rows"]).max()
    for idx in (0, 2047):
        r = int(g["rows"][idx])
        got, _ = O.accelerations_rows(pos, mass, "int8_sim", r, r + 1)
        assert np.abs(got[0].astype(np.float64) - g["int8_sim/pre_rows"][idx]).max() <= 2e-6 * scale



def _pin_dtypes():
    import torch
    return [(O.F16, torch.float16), (O.BF16, torch.bfloat16), (O.F32, torch.float32), (O.F64, torch.float64)]


def test_axpy_and_one_term_kinetic_energy_match_torch_for_all_dtype_pairs():
    """The exact references of tests/test_gpu_kick_paths.py and tests/test_gpu_kinetic_dtypes.py, pinned against torch
    itself: nbo_axpy == `a + b * s` (result dtype and every value, 4096 elements, three scalars that are not fp32
    numbers) and nbo_kinetic_energy == `(0.5 * masses * (velocities ** 2).sum(dim=-1)).sum()` on inputs with a single
    nonzero mass (one term: no summation order), for all 16 dtype pairs of {f16, bf16, f32, f64}, 2-D and 3-D."""
    import torch
    dts = _pin_dtypes()
    code_of = {t: c for c, t in dts}
    rng = np.random.default_rng(11)
    n = 4096
    for ca, ta in dts:
        for cb, tb in dts:
            a = torch.from_numpy(rng.standard_normal(n) * 0.05).to(ta)
            b = torch.from_numpy(rng.standard_normal(n) * 3.0).to(tb)
            a64, b64 = O.as_f64(a.double().numpy()), O.as_f64(b.double().numpy())
            for s in (0.005, 0.0123, 0.01 / 3):
                want = a + b * s
                out = np.empty(n)
                code = O.lib().nbo_axpy(n, ca, O._dp(a64), cb, O._dp(b64), s, O._dp(out))
                assert code == code_of[want.dtype], (ta, tb, code, want.dtype)
                assert np.array_equal(out, want.double().numpy()), (ta, tb, s, int((out != want.double().numpy()).sum()))
            # kinetic energy: velocities typed `ta`, masses typed `tb`
            for d in (2, 3):
                nk = 300
                vel = torch.from_numpy(rng.standard_normal((nk, d)) * 0.3).to(ta)
                v64 = O.as_f64(vel.double().numpy())
                for k in (0, 17, nk - 1):
                    m = np.zeros(nk)
                    m[k] = 0.5 + rng.random()
                    mass = torch.from_numpy(m).to(tb)
                    want = (0.5 * mass * (vel ** 2).sum(dim=-1)).sum().item()
                    got = O.lib().nbo_kinetic_energy(nk, d, ca, O._dp(v64), cb, O._dp(O.as_f64(mass.double().numpy())))
                    assert got == want, (ta, tb, d, k, got, want)


# --------------------------------------------------------------------------- the per-star diagnostics oracle
def _torch_per_star(p, v, m, G, edges):
    """The reference's formulas (metrics.py:48-143) with torch's CPU ops, every intermediate kept."""
    import torch
    positions, velocities, masses = torch.from_numpy(p), torch.from_numpy(v), torch.from_numpy(m)
    radii = torch.sqrt((positions ** 2).sum(dim=-1))
    vt = torch.abs(positions[:, 0] * velocities[:, 1] - positions[:, 1] * velocities[:, 0]) / radii.clamp(min=0.1)
    com = (positions * masses.unsqueeze(-1)).sum(dim=0) / masses.sum()
    r_com = torch.sqrt(((positions - com) ** 2).sum(dim=-1))
    order = torch.argsort(r_com, stable=True)
    enclosed = torch.cumsum(masses[order], dim=0)[torch.argsort(order)]
    vesc = torch.sqrt(2 * G * enclosed / r_com.clamp(min=0.1))
    vm = torch.sqrt((velocities ** 2).sum(dim=-1))
    e = torch.from_numpy(edges)
    bins = torch.full((len(m),), -1, dtype=torch.int64)
    for b in range(len(edges) - 1):
        bins[(radii >= e[b]) & (radii < e[b + 1])] = b
    return {k: t.numpy() for k, t in dict(r=radii, vt=vt, vm=vm, com=com, r_com=r_com, order=order, enclosed=enclosed,
                                          vesc=vesc, bound=vm < vesc, bins=bins).items()}


def _oracle_per_star(p, v, m, G, edges):
    from oracle import metrics_oracle as MO
    rc = MO.com_radii(p, m)
    return dict(r=MO.radii(p), vt=MO.tangential_speeds(p, v), vm=MO.speeds(v), com=MO.centre_of_mass(p, m), r_com=rc,
                order=MO.stable_order(rc), enclosed=MO.enclosed_masses(p, m), vesc=MO.escape_speeds(p, m, G),
                bound=MO.bound_flags(p, v, m, G), bins=MO.bin_indices(MO.radii(p), edges))


def _per_star_agree(got, want, keys, tag):
    """Exact, except through a square root: torch's vectorised CPU sqrt is not correctly rounded (measured in float32:
    sqrt(115.328125f) comes out 0.5014 ulp from the true root, on the wrong side of a near-tie; float64 likewise),
    numpy's is -- see test_metrics_oracle_square_root_is_correctly_rounded.  So the roots themselves (r, |v|, r_com)
    are held to one float of torch's value and what is computed from a root by one more rounded divide (vt) or a
    divide and a second root (vesc) to two; everything else to equality."""
    floats = {"r": 1, "vm": 1, "r_com": 1, "vt": 2, "vesc": 2}
    for k in keys:
        a, b = got[k], want[k]
        if k in ("order", "bins", "bound"):
            assert np.array_equal(a, b), (k,) + tag
            continue
        assert a.dtype == b.dtype, (k,) + tag
        if k in floats:
            with np.errstate(invalid="ignore"):
                ok = (a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= floats[k] * np.spacing(np.abs(b)))
            assert ok.all(), (k,) + tag
        else:
            assert np.array_equal(a, b, equal_nan=True), (k,) + tag


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n,dim", [(1, 2), (2, 3), (257, 2), (1025, 3), (2049, 2)])
def test_metrics_oracle_per_star_functions_vs_torch_ops(n, dim, dtype):
    """Every per-star function of oracle/metrics_oracle.py against torch's CPU result of the reference formula, element
    by element: all of them on lattice inputs (whose sums are exact in any order, so torch's summation order cannot
    matter), the element-wise ones (r, vt, |v|, bins) on random inputs with awkward stars as well."""
    import torch
    import metrics_cases as MC
    rng = np.random.default_rng(n + dim)
    edges = torch.linspace(0, 12.5, 8).numpy()
    p, m = MC.lattice(n, dim, np.dtype(dtype))
    v = (rng.standard_normal((n, dim)) * 0.05).astype(dtype)
    want, got = _torch_per_star(p, v, m, 0.001, edges), _oracle_per_star(p, v, m, 0.001, edges)
    _per_star_agree(got, want, list(want), (n, dim, dtype))
    p = (rng.standard_normal((n, dim)) * 4).astype(dtype)
    p[0] = 0.05
    if n > 2:
        p[1, 0], v[2, 1] = np.nan, np.inf
    want, got = _torch_per_star(p, v, m, 0.001, edges), _oracle_per_star(p, v, m, 0.001, edges)
    _per_star_agree(got, want, ("r", "vt", "vm", "bins"), (n, dim, dtype))


def test_metrics_oracle_square_root_is_correctly_rounded():
    """The oracle's float32 roots are the correctly rounded ones: equal to the float64 root rounded once (53 >= 2 * 24 + 2
    bits: the double rounding is harmless for a square root).  The device tests hold the kernels to these."""
    import metrics_cases as MC
    from oracle import metrics_oracle as MO
    p, m = MC.lattice(2049, 3, np.dtype(np.float32))
    s = (p.astype(np.float64) ** 2).sum(axis=1)                       # exact on the lattice
    assert np.array_equal(MO.radii(p), np.sqrt(s).astype(np.float32))
    x = np.float32(115.328125)
    assert np.sqrt(x) == np.float32(np.sqrt(np.float64(x))) == np.float32(10.739093780517578)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_metrics_lattice_inputs_have_order_independent_sums(dtype):
    """The precondition of the exact star-by-star device tests, for each lattice case: the sums behind the centre of mass
    are float32 numbers, and the oracle's enclosed masses and centre of mass do not change under sequential,
    reversed-within-1024-blocks and pairwise float64 accumulation."""
    import metrics_cases as MC
    for n, dim in MC.LATTICE_CASES:
        p, m = MC.lattice(n, dim, np.dtype(dtype))
        assert len(np.unique(m)) > 1 or n == 1
        assert np.abs(p).max() <= 16 and m.min() >= 0.25 and m.max() <= 2
        assert MC.sums_round_trip_through_float32(p, m), (n, dim)
        assert MC.order_independent(p, m), (n, dim)


def test_metrics_random_mass_case_has_an_order_independent_seed():
    import metrics_cases as MC
    seed, p, m = MC.random_mass_case()
    assert seed is not None and seed <= 20
    assert MC.order_independent(p, m) and not MC.sums_round_trip_through_float32(p, m)      # it really rounds


def test_metrics_oracle_linspace_and_ranks():
    """MO.linspace_f32 is torch.linspace; the percentile rank where n * p / 100 is within an ulp of an integer."""
    import torch
    from oracle import metrics_oracle as MO
    for B in (1, 2, 7, 20, 255):
        for R in (1.0, 12.5, float(np.float32(12.3456789)), float(np.float32(0.7071067811865476))):
            assert np.array_equal(MO.linspace_f32(R, B), torch.linspace(0, R, B + 1).numpy()), (B, R)
    assert [MO.percentile_rank(300, p) for p in (29, 57, 58, 0, 100, 99.9)] == [87, 171, 174, 0, 299, 299]
    assert [MO.percentile_rank(1, p) for p in (0, 50, 100)] == [0, 0, 0]


def test_metrics_oracle_vs_reference_metric_flow_tick0():
    """g12: the reference's collect_metrics at tick 0 (float32 state) from the refactored aggregates."""
    from oracle import metrics_oracle as MO
    g = load_golden("g12_metric_flow.npz")
    p, v, m = g["pos"], g["vel"], g["mass"]
    for mode in ("float64", "int4_sim"):
        rc = MO.rotation_curve(p, v)
        assert list(rc["num_stars_per_bin"]) == list(g[f"{mode}/rc_n"][0])
        assert np.allclose(rc["velocities"], g[f"{mode}/rc_v"][0], rtol=2e-6, equal_nan=True)
        assert abs(MO.galaxy_radius(p, 90) - g[f"{mode}/galaxy_radius_90"][0]) <= 1e-6 * g[f"{mode}/galaxy_radius_90"][0]
        assert abs(MO.bound_fraction(p, v, m, 0.001) - g[f"{mode}/bound_fraction"][0]) <= 1e-6
        assert abs(MO.velocity_dispersion(v) - g[f"{mode}/velocity_dispersion"][0]) <= 2e-6 * g[f"{mode}/velocity_dispersion"][0]


# ---------------------------------------------------------------------------------------------------------------
# tests/hook_cases.py: the inputs of tests/test_gpu_hooks_elements.py meet their stated preconditions, and the oracle
# agrees with torch's CPU ops on them
def _csrc(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "nbody_cosmological_simulation_amd", "csrc", name)) as f:
        return f.read()


def test_hook_cases_launch_arithmetic_mirrors_the_sources():
    """hook_cases.placements restates the launch shapes of the min/max, the element-wise and the table kernel: the
    statements it restates must still be there (compared without white space)."""
    import hook_cases as HC

    def squeeze(text):
        return "".join(text.split())

    def has(fname, statement, times=1):
        n = squeeze(_csrc(fname)).count(squeeze(statement))
        assert n == times, (f"{fname} no longer holds `{statement}` ({n} of {times}): the launch shape changed -- update the "
                            "constants and mm_owner / placements at the top of tests/hook_cases.py with it")
    has("nb_internal.h", f"constexpr int NB_MINMAX_BLOCKS = {HC.MM_BLOCKS};")
    has("nb_internal.h", f"constexpr int NB_MAX_LUT = {HC.MAX_LUT};")
    has("nb_misc.hip", f"constexpr int EW_BLOCK = {HC.EW_THREADS};")
    has("nb_misc.hip", f"if (b > 2048 * 8) b = 2048 * 8;")
    has("nb_misc.hip", f"int blocks = (int)((count + {HC.MM_PER_BLOCK - 1}) / {HC.MM_PER_BLOCK});", 2)
    has("nb_misc.hip", "blocks = blocks < 1 ? 1 : (blocks > MM_BLOCKS ? MM_BLOCKS : blocks);", 2)
    has("nb_misc.hip", f"for (; i + 3 * stride < end; i += {HC.MM_UNROLL} * stride) {{")
    has("nb_misc.hip", f"(int64_t)blockIdx.x * {HC.MM_THREADS} + threadIdx.x, count, (int64_t)gridDim.x * {HC.MM_THREADS}, min_val, mn, mx);")
    has("nb_misc.hip", f"for (int i = threadIdx.x; i < nblocks; i += {HC.MM_THREADS}) {{", 2)
    has("nb_hooks.cpp", "count >= (int64_t)1 << 21")
    has("nb_grid.hip", "grid = grid < 1 ? 1 : (grid > 4096 ? 4096 : grid);")
    assert (HC.EW_BLOCKS, HC.TABLE_FROM, HC.TAB_PASS) == (2048 * 8, 1 << 21, 4096 * 256)


def test_hook_cases_placement_indices_fall_where_claimed():
    import hook_cases as HC
    # mm_owner against the loop of minmax_block written out, at sizes small enough to walk
    for count in (1, 5, 1025, 4097, 5000, 9001):
        blocks, stride = HC.mm_shape(count)
        unrolled, slot = np.zeros(count, bool), np.full(count, -1)
        seen = np.zeros(count, int)
        for g in range(stride):
            i = g
            while i + 3 * stride < count:
                for s in range(4):
                    unrolled[i + s * stride], slot[i + s * stride] = True, s
                    seen[i + s * stride] += 1
                i += 4 * stride
            while i < count:
                seen[i] += 1
                i += stride
        assert (seen == 1).all()
        own = HC.mm_owner(count, np.arange(count))
        assert np.array_equal(own["unrolled"], unrolled) and np.array_equal(own["slot"], slot), count
        assert own["block"].max() == min(blocks, (count + 255) // 256) - 1
    assert set(HC.placements(1025)) == {"first", "i255", "i256", "last", "last_but_one"}
    for count in (HC.BIG, HC.HUGE):
        pl = HC.placements(count)
        assert {"first", "i255", "i256", "last", "last_but_one", "unrolled_last", "tail_first", "block257"} <= set(pl)
        assert ("second_pass" in pl) == (count == HC.HUGE)
        assert len(set(pl.values())) == len(pl) and all(0 <= p < count for p in pl.values())
        assert HC.mm_shape(count) == (HC.MM_BLOCKS, HC.MM_BLOCKS * HC.MM_THREADS)
        own = {k: {f: int(v) for f, v in HC.mm_owner(count, p).items()} for k, p in pl.items()}
        assert own["unrolled_last"]["unrolled"] and own["unrolled_last"]["slot"] == 3
        assert pl["tail_first"] == pl["unrolled_last"] + 1 and not own["tail_first"]["unrolled"]
        assert own["last"]["last_of_thread"] and not own["last"]["unrolled"]
        assert own["block257"]["block"] == 257 and own["block257"]["block"] % 256 != own["block257"]["block"]
        assert own["i255"]["block"] == 0 and own["i256"]["block"] == 1
        if count == HC.HUGE:
            assert pl["second_pass"] >= HC.EW_PASS and pl["last"] >= HC.EW_PASS and pl["last"] >= 4 * HC.TAB_PASS
            assert own["unrolled_last"]["trip"] == 7                     # the second unrolled trip of stage 1
        assert count > HC.TABLE_FROM


def _torch_bins_safe(t, levels, min_val):
    """Bins of quantization.py:91-127 in torch CPU ops.  fp32: the logarithm is taken in double and rounded, as the
    kernels and the oracle do (torch's float log is a 1-ulp vector routine: its bins differ near every edge)."""
    import torch
    x = torch.from_numpy(t).clamp(min=min_val)
    lt = torch.log(x.double()).to(x.dtype)
    lmin, lmax = lt.min(), lt.max()
    if lmax - lmin < 1e-10:
        return None
    return torch.round((lt - lmin) / (lmax - lmin) * (levels - 1)).numpy().astype(np.int32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hook_cases_log_values_meet_their_preconditions(dtype):
    import hook_cases as HC
    dtype = np.dtype(dtype)
    names = set()
    for L in (16, 256):
        for name, x, m in HC.log_value_cases(dtype, levels=L):
            names.add(name)
            mt = dtype.type(m)
            out, bins, lmin, lmax = O.grid_quantize_safe(x, L, m, bins=True)
            if dtype == np.float32:
                skip, ok = HC.log32_mask(x, L, m)
                assert ok and skip.sum() == 0, name                      # the cap of 1e-6 is zero elements at this count
            else:
                skip = HC.log64_expect(x, L, m)["skip"]                  # asserts its cap of 1e-4
                assert skip.sum() == 0, name
            tb = _torch_bins_safe(x, L, m)
            if name in ("all_below_clamp", "constant", "same_log_pair", "log_below_switch"):
                assert tb is None and (bins == -1).all() and np.array_equal(out, np.maximum(x, mt)), name
            else:
                assert np.array_equal(bins[~skip], tb[~skip]), (name, L, int((bins != tb).sum()))
                assert bins.min() == 0 and bins.max() == L - 1
            if name.startswith("decades"):
                assert 0.01 <= (x < mt).mean() <= 0.05, (name, (x < mt).mean())
            if name == "bin0_clamped":
                lv0 = dtype.type(O.exp_f64(np.array([dtype.type(O.log_f64(np.array([mt]))[0])]))[0])
                assert lv0 < mt and (x < mt).any() and (out[x < mt] == mt).all() and (bins[x < mt] == 0).all()
            if name == "same_log_pair":
                assert len(np.unique(x)) == 2
                assert len(np.unique(O.log_f64(x).astype(dtype))) == 1
            if name.startswith("max_"):
                assert x.max() >= 1e30
            if name.startswith("log_") and name.endswith("_switch"):
                assert (1e-10 < lmax - lmin < 1e-9) == (name == "log_above_switch") and abs((lmax - lmin) / 1e-10 - 1) > 0.3
            if name == "every_float_narrow":
                # every float of the range is there, so the first float of each bin and the float before it are: the
                # table path's thresholds are hit exactly, from both sides
                u = np.unique(x)
                assert np.array_equal(u.view(np.uint32), np.arange(u[0].view(np.uint32), u[-1].view(np.uint32) + 1))
                ub = O.grid_quantize_safe(u, L, m, bins=True)[1]
                assert (np.diff(ub) >= 0).all() and len(np.unique(ub)) == L and 0.6931471805599453 * (L - 1) / (lmax - lmin) >= 1e4
    assert {"decades_min0.01", "decades_min0.5", "decades_min2", "decades_min1e-30", "bin0_clamped", "all_below_clamp",
            "constant", "same_log_pair", "narrow"} <= names
    assert ("every_float_narrow" in names) == (dtype == np.float32) and ("log_above_switch" in names) == (dtype == np.float64)


def test_hook_cases_fp64_bounds_are_the_derived_ones():
    import hook_cases as HC
    lmin, lmax = np.log(1e-30), np.log(1e-23)
    E = 1.5 * np.spacing(abs(lmin))
    assert HC.log64_rel_bound(lmin, lmax) == 5 * E + 1.5 * 2.0 ** -52
    assert HC.log64_delta(lmin, lmax, 4097) == 3 * E * 4096 / (lmax - lmin)
    assert HC.log64_rel_bound(lmin, lmax) < 1.1e-13 and HC.log64_delta(lmin, lmax, 4097) < 1e-10
    assert HC.log64_rel_bound(0.0, 1e-4) < 3.4e-16                 # no floor under max|l|
    t = np.resize(np.array([0.5, 0.6, 1.9, 2.0]), 40000)
    t[7] = 2.0 ** -0.5                                             # on the edge between bins 0 and 1 of three levels
    ref = HC.log64_expect(t, 3, 0.01)
    assert ref["skip"][7] and ref["skip"].sum() == 1
    t[8:13] = 2.0 ** -0.5                                          # six of 40 000: over the cap of 1e-4
    with pytest.raises(AssertionError):
        HC.log64_expect(t, 3, 0.01)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hook_cases_linear_oracle_is_bit_identical_to_torch_cpu_ops(dtype):
    import hook_cases as HC
    from test_gpu_parity import torch_formula_linear
    dtype = np.dtype(dtype)

    def same(a, b):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    cases = HC.linear_value_cases(dtype) + [(f"mixed{n}", HC.mixed_signs(n, dtype, seed=n)) for n in HC.SMALL_COUNTS]
    for name, x in cases:
        for L in HC.LEVELS + (HC.ROUNDING_LEVELS,):
            out, bins, mn, mx = O.grid_quantize(x, L, bins=True)
            assert same(out, torch_formula_linear(x, L)), (name, L)
            if name.startswith("below_switch") or name == "constant" or x.size == 1:
                assert (bins == -1).all() and same(out, x), name
            elif name.startswith("above_switch") and L <= 4097:
                assert bins.min() == 0 and bins.max() == L - 1 and not same(out, x)
        if name.endswith("_switch"):
            assert (dtype.type(x.max() - x.min()) < 1e-10) == name.startswith("below") and abs((x.max() - x.min()) / 1e-10 - 1) > 0.05
    assert (HC.mixed_signs(HC.VALUE_COUNT, dtype) < 0).any() and np.abs(HC.mixed_signs(HC.VALUE_COUNT, dtype)).max() > 1e4
    for L in (17, 257):
        x, want_bins = HC.ties(L, dtype)
        assert np.array_equal(x.astype(np.float64), np.concatenate([[-8.0, 8.0], -8.0 + (np.arange(L - 1) + 0.5) / (L - 1) * 16.0]))
        norm = (x.astype(np.float64) + 8.0) / 16.0 * (L - 1)
        assert np.array_equal(norm[2:], np.arange(L - 1) + 0.5)          # exact half-integers
        out, bins, _, _ = O.grid_quantize(x, L, bins=True)
        assert np.array_equal(bins, want_bins) and (bins[2:] % 2 == 0).all()
        assert same(out, torch_formula_linear(x, L))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hook_cases_moving_the_extremum_swaps_the_expected_output(dtype):
    import hook_cases as HC
    from test_gpu_parity import torch_formula_linear
    dtype, count = np.dtype(dtype), 1025
    for kind in ("lin", "log"):
        for which in ("min", "max"):
            x0 = HC.placed(count, dtype, kind, which)
            ext = x0.min() if which == "min" else x0.max()
            assert x0[0] == ext and (x0 == ext).sum() == 1               # unique
            for L in (256, 4097):
                f = (lambda a: O.grid_quantize(a, L)) if kind == "lin" else (lambda a: O.grid_quantize_safe(a, L))
                e0 = f(x0)
                if kind == "lin":
                    assert e0.tobytes() == torch_formula_linear(x0, L).tobytes()
                elif dtype == np.float32:
                    skip, ok = HC.log32_mask(x0, L)
                    assert ok and not skip.any()
                for p in HC.placements(count).values():
                    xp, ep = x0.copy(), e0.copy()
                    xp[[0, p]], ep[[0, p]] = xp[[p, 0]], ep[[p, 0]]
                    assert f(xp).tobytes() == ep.tobytes(), (kind, which, L, p)


def test_hook_cases_cast_values_hit_every_tie():
    import torch
    import hook_cases as HC
    x32, x64 = HC.cast_values(np.float32), HC.cast_values(np.float64)
    assert x32.dtype == np.float32 and x64.dtype == np.float64
    for pats, cast, mant in ((HC.f16_patterns(), lambda t: t.half(), 10), (HC.bf16_patterns(), lambda t: t.bfloat16(), 7)):
        assert len(np.unique(pats.view(np.uint32))) == 65536
        fam, mid = HC._half_family(pats)
        fin = np.unique(pats[np.isfinite(pats)])
        assert mid.size == fin.size - 1 and np.isin(fam[~np.isnan(fam)], x32).all()
        t = torch.from_numpy(mid.astype(np.float32))
        r = cast(t).float().numpy().astype(np.float64)
        lo, hi = fin[:-1].astype(np.float64), fin[1:].astype(np.float64)
        assert ((r == lo) | (r == hi)).all() and (r == lo).any() and (r == hi).any()      # a tie goes to a neighbour ...
        bits = cast(t).view(torch.int16).numpy()
        assert (bits & 1 == 0).all()                                                     # ... the even one
        # the doubles next to a tie round to the tie as floats: the double-rounding trap
        up = np.nextafter(mid, np.inf)
        assert np.isin(up, x64).all() and np.array_equal(up.astype(np.float32).astype(np.float64), mid) and (up != mid).all()
    for v in (65504.0, 65520.0, 65536.0, np.float32(65519.99)):
        assert v in x32
    assert np.isnan(x32).any() and np.isinf(x32).any() and (x32 == 0).any() and np.signbit(x32[x32 == 0]).any()
    assert ((np.abs(x32) > 0) & (np.abs(x32) < 1.1754944e-38)).any() and 1e300 in x64
