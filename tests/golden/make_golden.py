#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by RUNNING the reference.

Run only in the build container (the reference is mounted read-only at
/root/reference and never travels to the GPU box):

    python tests/golden/make_golden.py            # writes tests/golden/*.npz, api.json

What is captured:
  G1  single-evaluation known-answer tests: accelerations after __init__ and the full
      state after one step(), all 7 precision modes, N in {64,257}, D in {2,3}, three
      softenings, equal/unequal masses.  For the grid modes the input/output of the
      reference's own `_grid_quantize_safe` / `_grid_quantize` calls are intercepted
      (spy wrappers around the reference functions, nothing re-implemented) and reduced
      to lmin/lmax/bin-index matrix/fmin/fmax.
  G1c CUSTOM levels through the sensitivity_test.py-style subclass override.
  G2  config-1 trajectory: N=1024, seed 42, create_disk_galaxy ICs -> fp32,
      G=1e-3, dt=0.01, eps=0.1; float64 snapshots + energies; other modes final state
      + diagnostics from the reference's metrics.py.
  G3  tile coverage: N=4096 fp64 50 ticks, N=8192 fp64 5 ticks (final state + energy).
  G4  API semantics: dtype timeline, fp64-input run, in-place perturbation, subclass
      override, get_state keys, mode-string alias table.
  G5  tensor-level hooks: quantize_distance_squared / quantize_force / _grid_quantize*
      on random tensors.
  G6  initial-condition generators and diagnostics (galaxy.py / metrics.py), seeded.
  G8  parameter extremes (softening 0 / 1e-4 ... 1.0, dt up to 2.0) through the stock class, incl. the NaN cases.
  G9  degenerate systems: N = 1, 2, 3, coincident particles, a massless particle (all seven modes).
  G10 tensor-level hooks on awkward inputs (0, negative, 1e30, inf, NaN, 2-3 levels, 1-D / 3-D / single element).
  G11 galaxy generators with non-default parameters.
  G12 main.py's metric flow (collect_metrics in a run() callback, compare_rotation_curves).
  G13 quant-bin assignments AT SCALE from the reference itself: N = 4096 (D = 2, disk galaxy) and N = 2048 (D = 3),
      INT8 / INT4 / CUSTOM(64): lmin, lmax, CRC-32 of every row of the int16 bin matrix, bin histogram, three full
      rows, force-grid bounds and force bins, accelerations.
  G14 state hash: reproducibility.hash_tensor_state of the reference on golden states (fp32 / fp64 / fp16).
  G15 dtype combinations the stock class accepts beyond G1-G7: fp64 masses beside fp32 positions under every mode,
      grid modes (INT8 / INT4 / CUSTOM) on fp64 state, grid modes on float16 / bfloat16 state.
  G20 quant-bin CHECKSUMS per target row (sum k, sum k * ((j mod 65521) + 1)) from the reference's bin matrices on the
      stored g13 / g16 positions: what nb_quant_bin_sums reads out of the production pair loops.
  G21 the reference against ITSELF under a reversed summation order (its own code on the flipped particle order): noise
      floor of the grid-mode trajectories (N = 1024 / 4096, three steps) and of INT8 / INT4 on half-typed state.
  G23 edge values (tests/edge_cases.py: NaN / infinite / runaway coordinates, massless stars, a NaN mass) at N = 48.
  G7  half-typed state (float16 / bfloat16 tensors) through the cast modes and FLOAT64: energies before
      and after the promotion, state after three steps.

Only DATA (inputs + outputs) is stored; no reference source text.
"""
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)

import galaxy as ref_galaxy            # noqa: E402
import metrics as ref_metrics          # noqa: E402
import quantization as ref_quant       # noqa: E402
import simulation as ref_sim           # noqa: E402
from quantization import PrecisionMode  # noqa: E402

torch.set_num_threads(8)

MODES = [PrecisionMode.FLOAT64, PrecisionMode.FLOAT32, PrecisionMode.BFLOAT16,
         PrecisionMode.FLOAT16, PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM,
         PrecisionMode.CUSTOM]
GRID_LEVELS = {PrecisionMode.INT8_SIM: 256, PrecisionMode.INT4_SIM: 16, PrecisionMode.CUSTOM: 64}


def npy(t):
    if t.dtype == torch.bfloat16:
        t = t.float()
    return t.detach().cpu().numpy()


class Spy:
    """Intercepts the reference's grid-quantisation calls to record their tensors."""

    def __init__(self):
        self.safe = []   # (input, levels, min_val, output)
        self.lin = []    # (input, levels, output)

    def __enter__(self):
        self._safe = ref_quant._grid_quantize_safe
        self._lin = ref_quant._grid_quantize

        def spy_safe(tensor, levels, min_val=0.01):
            out = self._safe(tensor, levels, min_val)
            self.safe.append((tensor.clone(), levels, min_val, out.clone()))
            return out

        def spy_lin(tensor, levels):
            out = self._lin(tensor, levels)
            self.lin.append((tensor.clone(), levels, out.clone()))
            return out

        ref_quant._grid_quantize_safe = spy_safe
        ref_quant._grid_quantize = spy_lin
        return self

    def __exit__(self, *a):
        ref_quant._grid_quantize_safe = self._safe
        ref_quant._grid_quantize = self._lin


def safe_bins(tin, levels, min_val, tout):
    """Bin indices as the reference computed them (same torch ops on the captured input)."""
    ts = tin.clamp(min=min_val)
    lt = torch.log(ts)
    lmin, lmax = lt.min(), lt.max()
    if (lmax - lmin) < 1e-10:
        return None, float(lmin), float(lmax)
    k = torch.round((lt - lmin) / (lmax - lmin) * (levels - 1))
    # cross-check against the reference's own output values
    chk = torch.exp(k / (levels - 1) * (lmax - lmin) + lmin).clamp(min=min_val)
    assert torch.equal(chk, tout), "bin reconstruction does not reproduce reference output"
    return npy(k).astype(np.int32), float(lmin), float(lmax)


def lin_bins(tin, levels, tout):
    mn, mx = tin.min(), tin.max()
    if (mx - mn) < 1e-10:
        return None, float(mn), float(mx)
    k = torch.round((tin - mn) / (mx - mn) * (levels - 1))
    chk = k / (levels - 1) * (mx - mn) + mn
    assert torch.equal(chk, tout)
    return npy(k).astype(np.int32), float(mn), float(mx)


def make_ics(n, d, seed, unequal):
    g = torch.Generator().manual_seed(seed)
    pos = (torch.randn(n, d, generator=g) * 4.0).float()
    vel = (torch.randn(n, d, generator=g) * 0.05).float()
    if unequal:
        mass = (0.2 + 2.0 * torch.rand(n, generator=g)).float()
    else:
        mass = torch.ones(n)
    return pos, vel, mass


def g1():
    cases = [
        dict(name="n64_d2_e0.1", n=64, d=2, eps=0.1, unequal=False, seed=1),
        dict(name="n257_d2_e0.05", n=257, d=2, eps=0.05, unequal=True, seed=2),
        dict(name="n64_d3_e0.01", n=64, d=3, eps=0.01, unequal=False, seed=3),
        dict(name="n257_d3_e0.1", n=257, d=3, eps=0.1, unequal=True, seed=4),
    ]
    for c in cases:
        pos, vel, mass = make_ics(c["n"], c["d"], c["seed"], c["unequal"])
        out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=c["eps"], G=0.001, dt=0.01)
        for mode in MODES:
            with Spy() as spy:
                sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(),
                                               precision_mode=mode, G=0.001,
                                               softening=c["eps"], dt=0.01)
            tag = mode.value
            out[f"{tag}/acc0"] = npy(sim.accelerations)
            out[f"{tag}/pe0"] = sim.get_potential_energy()
            out[f"{tag}/ke0"] = sim.get_kinetic_energy()
            if mode in GRID_LEVELS:
                tin, lv, mv, tout = spy.safe[0]
                assert lv == GRID_LEVELS[mode]
                k, lmin, lmax = safe_bins(tin, lv, mv, tout)
                out[f"{tag}/d2bins"] = k.astype(np.int16)
                out[f"{tag}/lmin"] = lmin
                out[f"{tag}/lmax"] = lmax
                out["r2_f32"] = npy(tin)   # identical for the three grid modes (same fp32 inputs)
                if spy.lin:
                    fin, flv, fout = spy.lin[0]
                    fk, fmin, fmax = lin_bins(fin, flv, fout)
                    out[f"{tag}/fbins"] = fk.astype(np.int16)
                    out[f"{tag}/fmin"] = fmin
                    out[f"{tag}/fmax"] = fmax
                    out[f"{tag}/acc0_prequant"] = npy(fin)
            sim.step()
            out[f"{tag}/pos1"] = npy(sim.positions)
            out[f"{tag}/vel1"] = npy(sim.velocities)
            out[f"{tag}/acc1"] = npy(sim.accelerations)
            for _ in range(9):
                sim.step()
            out[f"{tag}/pos10"] = npy(sim.positions)
            out[f"{tag}/vel10"] = npy(sim.velocities)
            out[f"{tag}/e10"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
        np.savez_compressed(os.path.join(OUT, f"g1_{c['name']}.npz"), **out)
        print("G1", c["name"])


def g1c():
    """CUSTOM levels via the subclass-override idiom of the reference's sweep scripts."""
    from quantization import _grid_quantize_safe

    class CustomQuantSim(ref_sim.GalaxySimulation):
        def __init__(self, *args, quant_levels, **kwargs):
            self.quant_levels = quant_levels
            super().__init__(*args, **kwargs)

        def _compute_accelerations(self):
            pos = self.positions
            diff = pos.unsqueeze(0) - pos.unsqueeze(1)
            dist_sq = (diff ** 2).sum(dim=-1) + self.softening_sq
            if self.quant_levels < 10000:
                dist_sq = _grid_quantize_safe(dist_sq, self.quant_levels, min_val=0.01)
            ff = self.G / dist_sq ** 1.5
            ff = ff * self.masses.unsqueeze(0)
            ff = ff * (1 - torch.eye(self.num_stars, device=self.device))
            return (ff.unsqueeze(-1) * diff).sum(dim=1)

    pos, vel, mass = make_ics(257, 2, 11, True)
    out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=0.1, G=0.001, dt=0.01)
    for L in (4, 64, 1000):
        sim = CustomQuantSim(pos.clone(), vel.clone(), mass.clone(), quant_levels=L,
                             precision_mode=PrecisionMode.FLOAT32, G=0.001, dt=0.01, softening=0.1)
        out[f"L{L}/acc0"] = npy(sim.accelerations)
        for _ in range(5):
            sim.step()
        out[f"L{L}/pos5"] = npy(sim.positions)
        out[f"L{L}/vel5"] = npy(sim.velocities)
    np.savez_compressed(os.path.join(OUT, "g1c_custom_levels.npz"), **out)
    print("G1c")


def diagnostics(sim):
    rc = ref_metrics.compute_rotation_curve(sim.positions, sim.velocities)
    return dict(
        ke=sim.get_kinetic_energy(), pe=sim.get_potential_energy(), e=sim.get_total_energy(),
        r90=ref_metrics.compute_galaxy_radius(sim.positions, 90),
        bound=ref_metrics.compute_bound_fraction(sim.positions, sim.velocities, sim.masses, sim.G),
        disp=ref_metrics.compute_velocity_dispersion(sim.velocities),
        rc_r=np.asarray(rc["radii"], dtype=np.float64),
        rc_v=np.asarray(rc["velocities"], dtype=np.float64),
        rc_n=np.asarray(rc["num_stars_per_bin"], dtype=np.int64),
    )


def disk_ics(n, seed):
    torch.manual_seed(seed)
    p, v, m = ref_galaxy.create_disk_galaxy(num_stars=n, galaxy_radius=10.0, device=torch.device("cpu"))
    return p.float(), v.float(), m.float()


def g2():
    pos, vel, mass = disk_ics(1024, 42)
    out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=0.1, G=0.001, dt=0.01)
    snaps = (0, 1, 10, 100, 200)
    for mode in MODES:
        tag = mode.value
        sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode,
                                       G=0.001, dt=0.01, softening=0.1)
        for t in range(0, 201):
            if t > 0:
                sim.step()
            if t in snaps and (mode == PrecisionMode.FLOAT64 or t in (0, 10, 200)):
                out[f"{tag}/pos{t}"] = npy(sim.positions)
                out[f"{tag}/vel{t}"] = npy(sim.velocities)
                if mode == PrecisionMode.FLOAT64:
                    out[f"{tag}/acc{t}"] = npy(sim.accelerations)
            if t in (0, 100, 200):
                for k, v in diagnostics(sim).items():
                    out[f"{tag}/diag{t}/{k}"] = v
        print("G2", tag)
    np.savez_compressed(os.path.join(OUT, "g2_config1_n1024.npz"), **out)


def g3():
    for n, ticks in ((4096, 50), (8192, 5)):
        pos, vel, mass = disk_ics(n, 42)
        sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(),
                                       precision_mode=PrecisionMode.FLOAT64, G=0.001, dt=0.01, softening=0.1)
        e0 = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
        acc0 = npy(sim.accelerations)
        for _ in range(ticks):
            sim.step()
        e1 = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
        np.savez_compressed(os.path.join(OUT, f"g3_fp64_n{n}.npz"), pos=npy(pos), vel=npy(vel), mass=npy(mass),
                            eps=0.1, G=0.001, dt=0.01, ticks=ticks, acc0=acc0, e0=e0, e1=e1,
                            pos_final=npy(sim.positions), vel_final=npy(sim.velocities),
                            acc_final=npy(sim.accelerations))
        print("G3", n)


def g4():
    api = {}
    pos, vel, mass = make_ics(96, 2, 21, True)
    out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=0.1, G=0.001, dt=0.01)

    # dtype timeline, fp32 inputs, every mode
    tl = {}
    for mode in MODES:
        sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode)
        row = [[str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]]
        for _ in range(2):
            sim.step()
            row.append([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)])
        tl[mode.value] = row
    api["dtype_timeline_fp32_inputs"] = tl

    # fp64 inputs (hardware_leak_test.py-style), FLOAT64 and FLOAT32 modes
    tl64 = {}
    for mode in MODES:
        sim = ref_sim.GalaxySimulation(pos.double(), vel.double(), mass.double(), precision_mode=mode,
                                       G=0.001, dt=0.01, softening=0.1)
        row = [[str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]]
        out[f"in64/{mode.value}/acc0"] = npy(sim.accelerations)
        for _ in range(3):
            sim.step()
        row.append([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)])
        tl64[mode.value] = row
        out[f"in64/{mode.value}/pos3"] = npy(sim.positions)
        out[f"in64/{mode.value}/vel3"] = npy(sim.velocities)
        out[f"in64/{mode.value}/e3"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
    api["dtype_timeline_fp64_inputs"] = tl64

    # half-precision state (omega_point_test.py-style): FLOAT32 mode, f16 / bf16 inputs
    tlh = {}
    for name, dt_ in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
        sim = ref_sim.GalaxySimulation(pos.to(dt_), vel.to(dt_), mass.to(dt_),
                                       precision_mode=PrecisionMode.FLOAT32, G=0.001, dt=0.01, softening=0.1)
        row = [[str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)]]
        out[f"in_{name}/acc0"] = npy(sim.accelerations)
        out[f"in_{name}/pe0"] = sim.get_potential_energy()
        for _ in range(3):
            sim.step()
        row.append([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.accelerations.dtype)])
        tlh[name] = row
        out[f"in_{name}/pos3"] = npy(sim.positions)
        out[f"in_{name}/vel3"] = npy(sim.velocities)
    api["dtype_timeline_half_inputs_float32_mode"] = tlh

    # in-place perturbation between steps (omega_point_test.py butterfly idiom)
    sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=PrecisionMode.FLOAT32,
                                   G=0.001, dt=0.01, softening=0.1)
    sim.positions[0, 0] += 1e-3
    sim.step()
    sim.positions[5, 1] -= 2e-3
    sim.velocities[7, 0] += 1e-2
    sim.step()
    out["mutate/pos2"] = npy(sim.positions)
    out["mutate/vel2"] = npy(sim.velocities)

    # attribute changes between steps (dt / G / softening_sq are read every step)
    sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=PrecisionMode.FLOAT64,
                                   G=0.001, dt=0.01, softening=0.1)
    sim.step()
    sim.dt = 0.02
    sim.step()
    sim.G = 0.002
    sim.step()
    out["attrs/pos3"] = npy(sim.positions)
    out["attrs/vel3"] = npy(sim.velocities)

    # run() callback contract
    calls = []
    sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone())
    sim.run(25, callback=lambda s, t: calls.append(int(t)), callback_interval=10)
    api["run_callback_ticks_25_by_10"] = calls
    api["tick_after_run"] = sim.tick
    st = sim.get_state()
    api["get_state_keys"] = sorted(st.keys())
    api["get_state_precision_mode"] = st["precision_mode"]

    # run_comparison structure
    res = ref_sim.run_comparison(pos.clone(), vel.clone(), mass.clone(),
                                 [PrecisionMode.FLOAT64, PrecisionMode.INT4_SIM], num_ticks=20,
                                 callback_interval=10)
    api["run_comparison_keys"] = sorted(res.keys())
    api["run_comparison_entry_keys"] = sorted(res["float64"].keys())
    api["run_comparison_history_ticks"] = res["float64"]["history"]["ticks"]
    out["runcmp/float64/energies"] = np.array(res["float64"]["history"]["energies"])
    out["runcmp/int4_sim/energies"] = np.array(res["int4_sim"]["history"]["energies"])
    out["runcmp/float64/pos_final"] = npy(res["float64"]["final_state"]["positions"])

    # string helpers
    names = ["float64", "float32", "bfloat16", "bf16", "float16", "fp16", "int8", "int8_sim", "int4",
             "int4_sim", "custom", "FLOAT32", "Int4", "nonsense", ""]
    api["mode_from_string"] = {s: ref_quant.get_mode_from_string(s).value for s in names}
    api["describe_mode"] = {m.value: ref_quant.describe_mode(m) for m in MODES}
    api["precision_mode_members"] = {m.name: m.value for m in PrecisionMode}

    np.savez_compressed(os.path.join(OUT, "g4_api.npz"), **out)
    with open(os.path.join(OUT, "api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
    print("G4")


def g5():
    g = torch.Generator().manual_seed(5)
    out = {}
    d2 = (torch.rand(128, 128, generator=g) * 50.0 + 0.001).float()
    d2[3, 4] = 1e-5
    d2[10, 10] = 70000.0   # overflows fp16
    force = (torch.randn(300, 2, generator=g) * 0.01).float()
    out["d2"] = npy(d2)
    out["force"] = npy(force)
    for mode in MODES:
        out[f"qd2/{mode.value}"] = npy(ref_quant.quantize_distance_squared(d2, mode))
        out[f"qf/{mode.value}"] = npy(ref_quant.quantize_force(force, mode))
    for L in (4, 16, 100, 1000):
        out[f"qd2/custom{L}"] = npy(ref_quant.quantize_distance_squared(d2, PrecisionMode.CUSTOM, custom_levels=L))
        out[f"safe/L{L}_min0.5"] = npy(ref_quant._grid_quantize_safe(d2, L, min_val=0.5))
        out[f"lin/L{L}"] = npy(ref_quant._grid_quantize(force, L))
    const = torch.full((7, 7), 3.0)
    out["safe/const"] = npy(ref_quant._grid_quantize_safe(const, 16))
    out["lin/const"] = npy(ref_quant._grid_quantize(const, 16))
    # fp64 tensors through the same hooks
    out["qd2_64/int8_sim"] = npy(ref_quant.quantize_distance_squared(d2.double(), PrecisionMode.INT8_SIM))
    out["qd2_64/float16"] = npy(ref_quant.quantize_distance_squared(d2.double(), PrecisionMode.FLOAT16))
    np.savez_compressed(os.path.join(OUT, "g5_hooks.npz"), **out)
    print("G5")


def g6():
    """Initial-condition generators and diagnostics (galaxy.py / metrics.py), seeded."""
    out = {}
    for name, fn, kw in (("disk", ref_galaxy.create_disk_galaxy, dict(num_stars=2000)),
                         ("test", ref_galaxy.create_test_galaxy, dict(num_stars=1000)),
                         ("halo", ref_galaxy.create_galaxy_with_halo, dict(num_stars=1500))):
        torch.manual_seed(7)
        p, v, m = fn(device=torch.device("cpu"), **kw)
        out[f"{name}/pos"], out[f"{name}/vel"], out[f"{name}/mass"] = npy(p), npy(v), npy(m)
        rc = ref_metrics.compute_rotation_curve(p, v)
        out[f"{name}/rc_r"], out[f"{name}/rc_v"] = rc["radii"], rc["velocities"]
        out[f"{name}/rc_n"] = np.asarray(rc["num_stars_per_bin"])
        rc2 = ref_metrics.compute_rotation_curve(p, v, num_bins=7, max_radius=12.5)
        out[f"{name}/rc7_v"] = rc2["velocities"]
        out[f"{name}/r90"] = ref_metrics.compute_galaxy_radius(p, 90)
        out[f"{name}/r50"] = ref_metrics.compute_galaxy_radius(p, 50)
        out[f"{name}/bound"] = ref_metrics.compute_bound_fraction(p, v, m, 0.001)
        out[f"{name}/disp"] = ref_metrics.compute_velocity_dispersion(v)
    r = torch.linspace(0.1, 100, 50)
    out["nfw"] = npy(ref_galaxy.nfw_enclosed_mass(r, 5000.0, 30.0))
    out["nfw_r"] = npy(r)
    np.savez_compressed(os.path.join(OUT, "g6_galaxy_metrics.npz"), **out)
    print("G6")


def g7():
    """Half-typed state (omega_point_test.py:722-733 idiom) through every cast mode: energies before and after the
    promotion of positions / velocities (the masses stay half for good), state after three steps, dtype timeline."""
    out = {}
    for n in (96, 700):
        pos, vel, mass = make_ics(n, 2, 70 + n, True)
        for hname, dt_ in (("float16", torch.float16), ("bfloat16", torch.bfloat16)):
            p, v, m = pos.to(dt_), vel.to(dt_), mass.to(dt_)
            out[f"n{n}/{hname}/pos"], out[f"n{n}/{hname}/vel"], out[f"n{n}/{hname}/mass"] = npy(p), npy(v), npy(m)
            for mode in (PrecisionMode.FLOAT32, PrecisionMode.BFLOAT16, PrecisionMode.FLOAT16, PrecisionMode.FLOAT64):
                sim = ref_sim.GalaxySimulation(p.clone(), v.clone(), m.clone(), precision_mode=mode, G=0.001, dt=0.01,
                                               softening=0.1)
                key = f"n{n}/{hname}/{mode.value}"
                out[key + "/e0"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
                for _ in range(3):
                    sim.step()
                out[key + "/e3"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
                out[key + "/pos3"] = npy(sim.positions).astype(np.float64)
                out[key + "/vel3"] = npy(sim.velocities).astype(np.float64)
                out[key + "/dtypes3"] = np.array([str(sim.positions.dtype), str(sim.velocities.dtype),
                                                  str(sim.accelerations.dtype), str(sim.masses.dtype)])
    np.savez_compressed(os.path.join(OUT, "g7_half_state.npz"), **out)


def g8():
    """Parameter extremes of crash_point_test.py:243,412 and falsification_tests.py:284-285 through the stock class:
    softening 1e-4 ... 1.0 (below the grid clamp, below float16's smallest subnormal squared -> NaN upstream),
    dt up to 2.0, softening 0 in FLOAT64 mode (0/0 on the diagonal)."""
    out = {}
    pos, vel, mass = disk_ics(150, 8)
    out["pos"], out["vel"], out["mass"] = npy(pos), npy(vel), npy(mass)
    cases = [("float32", 1e-4, 0.01), ("float32", 1e-4, 2.0), ("float32", 1.0, 0.01), ("float32", 1.0, 2.0),
             ("float16", 1e-4, 0.01), ("float16", 0.05, 0.05), ("bfloat16", 1e-3, 0.02),
             ("int4_sim", 1e-4, 0.05), ("int8_sim", 1.0, 0.5), ("custom", 1e-3, 0.01),
             ("float64", 0.0, 0.01), ("float64", 1e-4, 2.0)]
    names = []
    for mode_name, eps, dt in cases:
        mode = PrecisionMode(mode_name)
        sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode, G=0.001, dt=dt,
                                       softening=eps)
        key = f"{mode_name}/eps{eps}/dt{dt}"
        names.append(key)
        out[key + "/acc0"] = npy(sim.accelerations).astype(np.float64)
        out[key + "/e0"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
        for _ in range(5):
            sim.step()
        out[key + "/pos5"] = npy(sim.positions).astype(np.float64)
        out[key + "/vel5"] = npy(sim.velocities).astype(np.float64)
        out[key + "/e5"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "g8_extremes.npz"), **out)


def g9():
    """Degenerate systems through the stock class, all seven modes: N = 1, 2, 3, five coincident particles,
    a massless particle.  Accelerations, energies, state after two steps."""
    out = {}
    gen = torch.Generator().manual_seed(9)
    systems = {}
    for n in (1, 2, 3):
        systems[f"n{n}"] = ((torch.randn(n, 2, generator=gen) * 3).float(), (torch.randn(n, 2, generator=gen) * 0.1).float(),
                            (0.5 + torch.rand(n, generator=gen)).float())
    systems["coincident5"] = (torch.full((5, 2), 1.25), (torch.randn(5, 2, generator=gen) * 0.1).float(), torch.ones(5))
    p = (torch.randn(6, 3, generator=gen) * 3).float()
    m = torch.ones(6)
    m[2] = 0.0
    systems["massless_d3"] = (p, (torch.randn(6, 3, generator=gen) * 0.1).float(), m)
    names = []
    for sname, (pos, vel, mass) in systems.items():
        out[f"{sname}/pos"], out[f"{sname}/vel"], out[f"{sname}/mass"] = npy(pos), npy(vel), npy(mass)
        for mode in MODES:
            sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode, G=0.001, dt=0.01,
                                           softening=0.1)
            key = f"{sname}/{mode.value}"
            names.append(key)
            out[key + "/acc0"] = npy(sim.accelerations).astype(np.float64)
            out[key + "/e0"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
            sim.step()
            sim.step()
            out[key + "/pos2"] = npy(sim.positions).astype(np.float64)
            out[key + "/vel2"] = npy(sim.velocities).astype(np.float64)
            out[key + "/e2"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "g9_degenerate.npz"), **out)


def g10():
    """Tensor-level hooks on awkward inputs: zeros, negatives, huge values, inf, NaN, two or three levels, odd
    shapes (1-D, 3-D, a single element), every mode."""
    g = torch.Generator().manual_seed(10)
    out = {}
    base = (torch.rand(40, 40, generator=g) * 30.0 + 0.02).float()
    tens = {}
    t = base.clone(); t[0, 0] = 0.0; t[1, 1] = -4.0; t[2, 2] = 1e30; t[3, 3] = 1e-30
    tens["zero_neg_huge"] = t
    t = base.clone(); t[5, 6] = float("inf")
    tens["inf"] = t
    t = base.clone(); t[7, 8] = float("nan")
    tens["nan"] = t
    tens["vec1d"] = base[0].clone()
    tens["cube3d"] = base[:27, :8].reshape(3, 9, 8).clone()
    tens["single"] = torch.tensor([[2.5]])
    names = []
    for name, t in tens.items():
        out[f"in/{name}"] = npy(t)
        for mode in MODES:
            out[f"{name}/qd2/{mode.value}"] = npy(ref_quant.quantize_distance_squared(t, mode))
            out[f"{name}/qf/{mode.value}"] = npy(ref_quant.quantize_force(t - 15.0, mode))
        for L in (2, 3, 7):
            out[f"{name}/safe/L{L}"] = npy(ref_quant._grid_quantize_safe(t, L, min_val=0.01))
            out[f"{name}/lin/L{L}"] = npy(ref_quant._grid_quantize(t - 15.0, L))
        names.append(name)
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(OUT, "g10_hook_edges.npz"), **out)


def g11():
    """Galaxy generators with non-default parameters (radius, core fraction, halo radius, dark-matter ratio,
    tiny and odd star counts)."""
    out = {}
    cases = [("disk_r5_c0.6", ref_galaxy.create_disk_galaxy, dict(num_stars=777, galaxy_radius=5.0, core_mass_fraction=0.6)),
             ("disk_r40_c0", ref_galaxy.create_disk_galaxy, dict(num_stars=1234, galaxy_radius=40.0, core_mass_fraction=0.0)),
             ("disk_n3", ref_galaxy.create_disk_galaxy, dict(num_stars=3)),
             ("test_n17", ref_galaxy.create_test_galaxy, dict(num_stars=17)),
             ("halo_r8_h50_dm20", ref_galaxy.create_galaxy_with_halo,
              dict(num_stars=900, galaxy_radius=8.0, halo_radius=50.0, dm_mass_ratio=20.0)),
             ("halo_dm0", ref_galaxy.create_galaxy_with_halo, dict(num_stars=500, dm_mass_ratio=0.0))]
    for name, fn, kw in cases:
        torch.manual_seed(11)
        p, v, m = fn(device=torch.device("cpu"), **kw)
        out[f"{name}/pos"], out[f"{name}/vel"], out[f"{name}/mass"] = npy(p), npy(v), npy(m)
        out[f"{name}/dtypes"] = np.array([str(p.dtype), str(v.dtype), str(m.dtype)])
    np.savez_compressed(os.path.join(OUT, "g11_generators.npz"), **out)


def g12():
    """main.py's metric flow: collect_metrics every 10 ticks over 30 ticks (float64 and int4), the rotation-curve
    comparison of the two final states, and the numbers behind the text summary."""
    out = {}
    pos, vel, mass = disk_ics(300, 12)
    out["pos"], out["vel"], out["mass"] = npy(pos), npy(vel), npy(mass)
    finals = {}
    for mode in (PrecisionMode.FLOAT64, PrecisionMode.INT4_SIM):
        sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode, G=0.001, dt=0.01,
                                       softening=0.1)
        m = ref_metrics.SimulationMetrics()
        ref_metrics.collect_metrics(sim, 0, m)
        sim.run(30, callback=lambda s, t: ref_metrics.collect_metrics(s, t, m), callback_interval=10)
        k = mode.value
        out[f"{k}/ticks"] = np.array(m.ticks)
        for f in ("total_energy", "kinetic_energy", "potential_energy", "galaxy_radius_90", "bound_fraction",
                  "velocity_dispersion"):
            out[f"{k}/{f}"] = np.array(getattr(m, f), dtype=np.float64)
        out[f"{k}/rc_v"] = np.array([rc["velocities"] for rc in m.rotation_curves], dtype=np.float64)
        out[f"{k}/rc_n"] = np.array([rc["num_stars_per_bin"] for rc in m.rotation_curves])
        finals[k] = m.rotation_curves[-1]
    cmp_ = ref_metrics.compare_rotation_curves(finals["float64"], finals["int4_sim"])
    for key, val in cmp_.items():
        out[f"compare/{key}"] = np.float64(val)
    np.savez_compressed(os.path.join(OUT, "g12_metric_flow.npz"), **out)


def g13():
    """Bin assignments at sizes where tiles, pruning and the table-free pair path are all in play."""
    import zlib
    cases = []
    torch.manual_seed(1313)
    p2, v2, m2 = ref_galaxy.create_disk_galaxy(num_stars=4096, device=torch.device("cpu"))
    cases.append(("n4096_d2", p2.float(), v2.float(), m2.float(), 0.1))
    g = torch.Generator().manual_seed(1314)
    p3 = torch.cat([p2[:2048], 0.4 * torch.randn(2048, 1, generator=g)], 1).float()
    v3 = torch.cat([v2[:2048], torch.zeros(2048, 1)], 1).float()
    m3 = (0.5 + torch.rand(2048, generator=g)).float()
    cases.append(("n2048_d3", p3, v3, m3, 0.05))            # softening^2 below the grid floor 0.01: clamp active
    for name, pos, vel, mass, eps in cases:
        n = pos.shape[0]
        out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=eps, G=0.001, dt=0.01)
        for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM):
            with Spy() as spy:
                sim = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode, G=0.001,
                                               softening=eps, dt=0.01)
            tag = mode.value
            tin, lv, mv, tout = spy.safe[0]
            k, lmin, lmax = safe_bins(tin, lv, mv, tout)
            k16 = np.ascontiguousarray(k.astype("<i2"))
            out[f"{tag}/lmin"], out[f"{tag}/lmax"] = lmin, lmax
            out[f"{tag}/row_crc"] = np.array([zlib.crc32(k16[i].tobytes()) for i in range(n)], np.uint32)
            out[f"{tag}/hist"] = np.bincount(k16.ravel(), minlength=lv).astype(np.int64)
            for r in (0, n // 2, n - 1):
                out[f"{tag}/row{r}"] = k16[r]
            out[f"{tag}/acc0"] = npy(sim.accelerations)
            if spy.lin:
                fin, flv, fout = spy.lin[0]
                fk, fmin, fmax = lin_bins(fin, flv, fout)
                out[f"{tag}/fbins"] = fk.astype(np.int16)
                out[f"{tag}/fmin"], out[f"{tag}/fmax"] = fmin, fmax
        np.savez_compressed(os.path.join(OUT, f"g13_bins_{name}.npz"), **out)
        print("G13", name)


def g16():
    """Config 3's REAL size pinned to the reference itself: distance bins of sampled target rows at N = 65 536.
    The reference cannot hold the N x N tensor, but its log grid is elementwise once lmin / lmax are known, and those
    are the logs of the clamped minimum (the diagonal, present in every row) and maximum of r2.  So: r2 rows with the
    reference's own expression (simulation.py:83-86) on a row subset, the global maximum located by a chunked scan
    with the same ops, and quantize_distance_squared of the reference applied to a row block that contains a row
    of the farthest pair -- its bounds are then the global ones, and every element of the block gets the bin the
    full evaluation would give it."""
    import hashlib
    import zlib
    n = 65536
    torch.manual_seed(42)
    pos, vel, mass = ref_galaxy.create_disk_galaxy(n, device="cpu")
    pos = pos.float()
    eps2 = 0.1 ** 2                                   # simulation.py:59: Python double
    best, istar = -1.0, -1
    for i0 in range(0, n, 512):                       # simulation.py:83-86 on row blocks
        diff = pos.unsqueeze(0) - pos[i0:i0 + 512].unsqueeze(1)
        d2 = (diff ** 2).sum(dim=-1) + eps2
        m = float(d2.max())
        if m > best:
            best, istar = m, i0 + int(d2.max(dim=1).values.argmax())
    rows = sorted({istar, 0, 1, 12345, n // 2, n - 1})
    diff = pos.unsqueeze(0) - pos[rows].unsqueeze(1)
    d2 = (diff ** 2).sum(dim=-1) + eps2
    assert float(d2.max()) == best
    # the positions themselves travel: torch's CPU transcendentals differ in the last bit between hosts (AVX2 /
    # AVX-512 code paths), so regenerating the galaxy elsewhere does not reproduce these bits
    out = dict(rows=np.array(rows, np.int64), istar=istar, r2max=np.float32(best), pos=npy(pos).astype(np.float32),
               pos_sha256=np.array(hashlib.sha256(npy(pos).tobytes()).hexdigest()))
    for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM):
        levels = {PrecisionMode.INT8_SIM: 256, PrecisionMode.INT4_SIM: 16, PrecisionMode.CUSTOM: 64}[mode]
        q = ref_quant.quantize_distance_squared(d2.clone(), mode)
        k, lmin, lmax = safe_bins(d2, levels, 0.01, q)
        k16 = np.ascontiguousarray(k.astype("<i2"))
        tag = mode.value
        out[f"{tag}/lmin"], out[f"{tag}/lmax"] = lmin, lmax
        out[f"{tag}/row_crc"] = np.array([zlib.crc32(k16[r].tobytes()) for r in range(len(rows))], np.uint32)
        out[f"{tag}/row_hist"] = np.stack([np.bincount(k16[r], minlength=levels) for r in range(len(rows))]).astype(np.int64)
        out[f"{tag}/row0_head"] = k16[rows.index(0)][:4096]       # the first 4096 bins of target row 0, for a readable failure
    # accelerations of the same rows, every stage with the reference's own torch expressions on the row block
    # (simulation.py:83-112; the hook sees a block with the global bounds, the eye mask is the block's slice of it).
    # INT8 / INT4 stop before quantize_force (its grid needs the forces of every row).
    ones = torch.ones(n)
    eye_rows = torch.zeros(len(rows), n)
    eye_rows[torch.arange(len(rows)), torch.tensor(rows)] = 1.0
    for mode in PrecisionMode:
        diff_m = pos.unsqueeze(0) - pos[rows].unsqueeze(1)
        dist_sq = (diff_m ** 2).sum(dim=-1) + eps2
        qd = ref_quant.quantize_distance_squared(dist_sq, mode)
        cubed = qd ** 1.5
        ff = 0.001 / cubed
        ff = ff * ones.unsqueeze(0)
        ff = ff * (1 - eye_rows)
        acc = (ff.unsqueeze(-1) * diff_m).sum(dim=1)
        out[f"{mode.value}/acc_rows"] = npy(acc.double())
        out[f"{mode.value}/acc_dtype"] = np.array(str(acc.dtype))
    np.savez_compressed(os.path.join(OUT, "g16_bins_n65536_rows.npz"), **out)
    print("G16 rows", rows, "r2max", best)


def g17():
    """BASELINE config 2's real size, one full leapfrog step and the energies from the reference's own torch
    expressions evaluated on row blocks (simulation.py:83-112 for the forces, :132-141 for the step, :172-190 for the
    energies): N = 65 536, FLOAT64 mode, the fp32 initial positions of g16 with zero velocities (fp32-typed first
    evaluation, fp64 afterwards -- the dtype promotion of the stock class happens by itself in these expressions).
    Every row's force is needed for the step, so the two evaluations cost ~2 x 128 row blocks; stored: 2048 sampled
    rows of the state after the step, the energies before and after.  The block sums of the potential energy are
    added in fp64 (the reference would add the whole N x N tensor at once: same terms, rounding-level difference)."""
    n = 65536
    g16_ = np.load(os.path.join(OUT, "g16_bins_n65536_rows.npz"))
    pos = torch.from_numpy(g16_["pos"]).clone()
    vel = torch.zeros_like(pos)
    masses = torch.ones(n)
    G, dt, eps2 = 0.001, 0.01, 0.1 ** 2
    mode = PrecisionMode.FLOAT64

    def forces(p):
        out = []
        for i0 in range(0, n, 256):
            rows = torch.arange(i0, min(i0 + 256, n))
            diff = p.unsqueeze(0) - p[rows].unsqueeze(1)
            dist_sq = (diff ** 2).sum(dim=-1) + eps2
            qd = ref_quant.quantize_distance_squared(dist_sq, mode)
            ff = G / (qd ** 1.5)
            ff = ff * masses.unsqueeze(0)
            eye_rows = torch.zeros(len(rows), n)
            eye_rows[torch.arange(len(rows)), rows] = 1.0
            ff = ff * (1 - eye_rows)
            out.append((ff.unsqueeze(-1) * diff).sum(dim=1))
        return torch.cat(out)

    def potential(p, m):
        total = 0.0
        for i0 in range(0, n, 256):
            rows = torch.arange(i0, min(i0 + 256, n))
            diff = p.unsqueeze(0) - p[rows].unsqueeze(1)
            dist = torch.sqrt((diff ** 2).sum(dim=-1) + eps2)
            mass_prod = m.unsqueeze(0) * m[rows].unsqueeze(1)
            mask = (torch.arange(n).unsqueeze(0) > rows.unsqueeze(1)).to(dist.dtype)        # triu(diagonal=1), these rows
            total += float((mass_prod * mask / dist).double().sum())
        return -G * total

    def kinetic(v, m):
        return float(0.5 * (m * (v ** 2).sum(dim=-1)).sum())

    acc = forces(pos)                                   # __init__ (simulation.py:69)
    e0 = (kinetic(vel, masses), potential(pos, masses))
    vel = vel + acc * (dt / 2)                          # step (simulation.py:132-141)
    pos1 = pos + vel * dt
    acc1 = forces(pos1)
    vel1 = vel + acc1 * (dt / 2)
    e1 = (kinetic(vel1, masses), potential(pos1, masses))
    rows = np.sort(np.random.default_rng(17).choice(n, 2048, replace=False))
    np.savez_compressed(os.path.join(OUT, "g17_step_n65536.npz"), rows=rows, acc0=npy(acc.double())[rows],
                        pos1=npy(pos1.double())[rows], vel1=npy(vel1.double())[rows], acc1=npy(acc1.double())[rows],
                        e0=np.array(e0), e1=np.array(e1),
                        dtypes=np.array([str(acc.dtype), str(pos1.dtype), str(vel1.dtype), str(acc1.dtype)]))
    print("G17", e0, e1, acc.dtype, pos1.dtype)


def g18():
    """Config 3's real size, INT8 / INT4 end to end: the forces of EVERY row at N = 65 536 through the reference's
    expressions on row blocks (the hook sees blocks carrying the global bounds: every block is given the diagonal
    value and the farthest pair's r2 as two extra entries of an extra row -- elementwise functions do not care), then
    the reference's own quantize_force on the full (N, 2) tensor: fmin / fmax and the force bins.  Stored: the force
    grid's bounds, the histogram of the force bins, and bins + values of 4096 sampled rows."""
    n = 65536
    g16_ = np.load(os.path.join(OUT, "g16_bins_n65536_rows.npz"))
    pos = torch.from_numpy(g16_["pos"]).clone()
    masses = torch.ones(n)
    G, eps2 = 0.001, 0.1 ** 2
    r2max = float(g16_["r2max"])
    out = dict(rows=np.sort(np.random.default_rng(18).choice(n, 4096, replace=False)))
    for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM):
        levels = 256 if mode == PrecisionMode.INT8_SIM else 16
        acc = []
        for i0 in range(0, n, 256):
            rows = torch.arange(i0, min(i0 + 256, n))
            diff = pos.unsqueeze(0) - pos[rows].unsqueeze(1)
            dist_sq = (diff ** 2).sum(dim=-1) + eps2
            # one extra row holding the global extremes, so that the hook's min / max are the full tensor's
            extra = torch.full((1, n), float(dist_sq[0, rows[0]]))                 # the diagonal value (r2 = eps2)
            extra[0, 0] = r2max
            qd = ref_quant.quantize_distance_squared(torch.cat([dist_sq, extra.to(dist_sq.dtype)]), mode)[:-1]
            ff = G / (qd ** 1.5)
            ff = ff * masses.unsqueeze(0)
            eye_rows = torch.zeros(len(rows), n)
            eye_rows[torch.arange(len(rows)), rows] = 1.0
            ff = ff * (1 - eye_rows)
            acc.append((ff.unsqueeze(-1) * diff).sum(dim=1))
        acc = torch.cat(acc)
        q = ref_quant.quantize_force(acc.clone(), mode)
        fk, fmin, fmax = lin_bins(acc, levels, q)
        tag = mode.value
        out[f"{tag}/fmin"], out[f"{tag}/fmax"] = fmin, fmax
        out[f"{tag}/fhist"] = np.bincount(fk.ravel(), minlength=levels).astype(np.int64)
        out[f"{tag}/fbins_rows"] = fk.astype(np.int16)[out["rows"]]
        out[f"{tag}/acc_rows"] = npy(q.double())[out["rows"]]
        out[f"{tag}/pre_rows"] = npy(acc.double())[out["rows"]]
        print("G18", tag, fmin, fmax)
    np.savez_compressed(os.path.join(OUT, "g18_force_quant_n65536.npz"), **out)


def g19_positions(n):
    """Host-independent initial conditions for the big configurations: numpy's PCG64 stream and one multiply-add (no
    transcendental, whose last bit depends on the host's vector ISA) -- tests regenerate them instead of loading them."""
    return ((np.random.default_rng(1900 + n).random((n, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(40.0)).astype(np.float32)


def g19():
    """BASELINE configs 4 / 5 at their real sizes (N = 262 144 and 1 048 576, FLOAT32 mode): the accelerations of 64
    sampled rows from the reference's torch expressions on row blocks (simulation.py:83-112; FLOAT32 needs no global
    pass).  Uniform square of stars, unit masses."""
    out = {}
    for n in (262144, 1048576):
        pos = torch.from_numpy(g19_positions(n))
        rows_all = np.sort(np.random.default_rng(19).choice(n, 64, replace=False))
        masses = torch.ones(n)
        acc = []
        for b in range(0, 64, 16):
            rows = torch.from_numpy(rows_all[b:b + 16])
            diff = pos.unsqueeze(0) - pos[rows].unsqueeze(1)
            dist_sq = (diff ** 2).sum(dim=-1) + 0.1 ** 2
            qd = ref_quant.quantize_distance_squared(dist_sq, PrecisionMode.FLOAT32)
            ff = 0.001 / (qd ** 1.5)
            ff = ff * masses.unsqueeze(0)
            eye_rows = torch.zeros(len(rows), n)
            eye_rows[torch.arange(len(rows)), rows] = 1.0
            ff = ff * (1 - eye_rows)
            acc.append((ff.unsqueeze(-1) * diff).sum(dim=1))
        acc = torch.cat(acc)
        out[f"n{n}/rows"] = rows_all
        out[f"n{n}/acc_rows"] = npy(acc.double())
        out[f"n{n}/acc_dtype"] = np.array(str(acc.dtype))
        print("G19", n, acc.dtype, float(acc.abs().max()))
    np.savez_compressed(os.path.join(OUT, "g19_big_n_rows.npz"), **out)


def g15():
    """Mixed / unusual dtype combinations through the stock class (quantization.py:58-69 is dtype-polymorphic,
    simulation.py:105 promotes through the mass product)."""
    pos, vel, mass = make_ics(193, 2, 15, True)
    out = dict(pos=npy(pos), vel=npy(vel), mass=npy(mass), eps=0.1, G=0.001, dt=0.01)

    def run(tag, p, v, m, mode):
        try:
            with Spy() as spy:
                sim = ref_sim.GalaxySimulation(p.clone(), v.clone(), m.clone(), precision_mode=mode, G=0.001,
                                               softening=0.1, dt=0.01, device=torch.device("cpu"))
            out[f"{tag}/dtypes0"] = np.array([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.masses.dtype),
                                              str(sim.accelerations.dtype)])
            out[f"{tag}/acc0"] = npy(sim.accelerations.double() if sim.accelerations.dtype != torch.float64 else sim.accelerations)
            out[f"{tag}/e0"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
            if spy.safe:
                tin, lv, mv, tout = spy.safe[0]
                out[f"{tag}/r2_dtype"] = np.array(str(tin.dtype))
                if tin.dtype in (torch.float32, torch.float64):
                    k, lmin, lmax = safe_bins(tin, lv, mv, tout)
                    if k is not None:
                        out[f"{tag}/d2bins"] = k.astype(np.int16)
                    out[f"{tag}/lmin"], out[f"{tag}/lmax"] = lmin, lmax
                else:
                    out[f"{tag}/q_out"] = npy(tout.double())
            if spy.lin:
                fin, flv, fout = spy.lin[0]
                if fin.dtype in (torch.float32, torch.float64):
                    fk, fmin, fmax = lin_bins(fin, flv, fout)
                    if fk is not None:
                        out[f"{tag}/fbins"] = fk.astype(np.int16)
                    out[f"{tag}/fmin"], out[f"{tag}/fmax"] = fmin, fmax
            for _ in range(3):
                sim.step()
            out[f"{tag}/dtypes3"] = np.array([str(sim.positions.dtype), str(sim.velocities.dtype), str(sim.masses.dtype),
                                              str(sim.accelerations.dtype)])
            out[f"{tag}/pos3"] = npy(sim.positions.double())
            out[f"{tag}/vel3"] = npy(sim.velocities.double())
            out[f"{tag}/e3"] = np.array([sim.get_kinetic_energy(), sim.get_potential_energy()])
            out[f"{tag}/ok"] = np.array(1)
        except Exception as exc:            # record what upstream does, including failing
            out[f"{tag}/ok"] = np.array(0)
            out[f"{tag}/error"] = np.array(type(exc).__name__ + ": " + str(exc)[:200])

    for mode in MODES:
        run(f"m64/{mode.value}", pos, vel, mass.double(), mode)                       # fp64 masses, fp32 positions
        run(f"v64/{mode.value}", pos, vel.double(), mass, mode)                       # fp64 velocities only
    for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM):
        run(f"all64/{mode.value}", pos.double(), vel.double(), mass.double(), mode)   # grid modes on fp64 state
        run(f"half/{mode.value}", pos.half(), vel.half(), mass.half(), mode)          # grid modes on float16 state
        run(f"bf16/{mode.value}", pos.bfloat16(), vel.bfloat16(), mass.bfloat16(), mode)
    np.savez_compressed(os.path.join(OUT, "g15_dtype_combos.npz"), **out)
    for k in sorted(out):
        if k.endswith("/ok") or k.endswith("/error") or k.endswith("dtypes0") or k.endswith("dtypes3"):
            print(k, out[k])
    print("G15")


def bin_checksums(k):
    """Per-row integer checksums of a bin matrix k (rows = targets, columns = ALL N sources incl. the diagonal):
    s1[i] = sum_j k[i, j],  s2[i] = sum_j k[i, j] * ((j mod 65521) + 1) -- what nb_quant_bin_sums reads out of the
    production pair loops (include/nbody_amd.h)."""
    k64 = np.asarray(k, np.int64)
    w = (np.arange(k64.shape[1], dtype=np.int64) % 65521) + 1
    return k64.sum(axis=1), (k64 * w[None, :]).sum(axis=1)


def g20():
    """Quant-bin checksums of the reference's own bin matrices, for the read-out of the production pair loops.
    Inputs are the STORED positions of g13 (N = 4096 D = 2; N = 2048 D = 3 with the grid floor active) and g16
    (N = 65 536, six target rows), so nothing depends on regenerating a galaxy on this host; the recomputed row CRCs
    must equal the ones those fixtures hold.  g13 cases: every row, from the reference class's own
    _grid_quantize_safe call (Spy); g16: the six rows through the reference's quantize_distance_squared on a row
    block that contains the farthest pair (global bounds), as g16 itself does."""
    import zlib
    out = {}
    for name in ("n4096_d2", "n2048_d3"):
        g = np.load(os.path.join(OUT, f"g13_bins_{name}.npz"))
        pos, vel, mass = (torch.from_numpy(g[k]).clone() for k in ("pos", "vel", "mass"))
        n = pos.shape[0]
        for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM):
            with Spy() as spy:
                ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), precision_mode=mode, G=0.001,
                                         softening=float(g["eps"]), dt=0.01)
            tin, lv, mv, tout = spy.safe[0]
            k, lmin, lmax = safe_bins(tin, lv, mv, tout)
            tag = mode.value
            k16 = np.ascontiguousarray(k.astype("<i2"))
            crc = np.array([zlib.crc32(k16[i].tobytes()) for i in range(n)], np.uint32)
            assert np.array_equal(crc, g[f"{tag}/row_crc"]), (name, tag, "bin matrix differs from the g13 fixture")
            assert np.all(np.diag(k) == 0)
            s1, s2 = bin_checksums(k)
            out[f"g13_{name}/{tag}/s1"], out[f"g13_{name}/{tag}/s2"] = s1, s2
            print("G20", name, tag, "sum k", int(s1.sum()))
    g16_ = np.load(os.path.join(OUT, "g16_bins_n65536_rows.npz"))
    pos = torch.from_numpy(g16_["pos"]).clone()
    rows = [int(r) for r in g16_["rows"]]
    eps2 = 0.1 ** 2
    diff = pos.unsqueeze(0) - pos[rows].unsqueeze(1)
    d2 = (diff ** 2).sum(dim=-1) + eps2
    assert float(d2.max()) == float(g16_["r2max"])
    for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM, PrecisionMode.CUSTOM):
        levels = GRID_LEVELS[mode]
        q = ref_quant.quantize_distance_squared(d2.clone(), mode)
        k, lmin, lmax = safe_bins(d2, levels, 0.01, q)
        tag = mode.value
        k16 = np.ascontiguousarray(k.astype("<i2"))
        crc = np.array([zlib.crc32(k16[r].tobytes()) for r in range(len(rows))], np.uint32)
        assert np.array_equal(crc, g16_[f"{tag}/row_crc"]), (tag, "bin rows differ from the g16 fixture")
        s1, s2 = bin_checksums(k)
        out[f"g16/{tag}/s1"], out[f"g16/{tag}/s2"] = s1, s2
    out["g16/rows"] = np.array(rows, np.int64)
    np.savez_compressed(os.path.join(OUT, "g20_bin_checksums.npz"), **out)
    print("G20 done")


class FlippedOrder(ref_sim.GalaxySimulation):
    """The reference against ITSELF under another summation order: the stock _compute_accelerations (its own code,
    nothing restated) is handed the particles in reversed order and the result is flipped back.  Every pair's
    arithmetic is unchanged (r2, hooks and the global grid bounds are symmetric in the particle order); only the order
    in which torch's sum(dim=1) meets the sources differs -- the rounding-level freedom any other correct
    implementation has too ("reduction order unspecified")."""

    def _compute_accelerations(self):
        p, m = self.positions, self.masses
        self.positions, self.masses = p.flip(0), m.flip(0)
        try:
            a = super()._compute_accelerations()
        finally:
            self.positions, self.masses = p, m
        return a.flip(0)


def g21():
    """Noise floor of the REFERENCE against itself for the two parity bars that round 2 widened after red runs
    (VERDICT r2 weak #2): what the reference does when only its summation order changes.
      traj/*  three leapfrog steps of the grid modes at N = 4096 (g13's disk galaxy) and N = 1024 (g2's): fraction of
              particles whose velocity differs by more than 2e-6 of max|v|, the maximum and the 99.9 % quantile; the
              stock run's final state is stored too, so the HIP path is compared with the reference itself.
      half/*  INT8 / INT4 on float16 / bfloat16 state (g15's system + 7 more seeds of the same recipe): fraction of
              force values that differ by more than half a force-grid step between the two summation orders."""
    out = {}
    cases = []
    g = np.load(os.path.join(OUT, "g13_bins_n4096_d2.npz"))
    cases.append(("n4096", *(torch.from_numpy(g[k]).clone() for k in ("pos", "vel", "mass"))))
    g = np.load(os.path.join(OUT, "g2_config1_n1024.npz"))
    cases.append(("n1024", *(torch.from_numpy(g[k]).clone() for k in ("pos", "vel", "mass"))))
    for name, pos, vel, mass in cases:
        for mode in (PrecisionMode.CUSTOM, PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM):
            kw = dict(precision_mode=mode, G=0.001, softening=0.1, dt=0.01, device=torch.device("cpu"))
            a = ref_sim.GalaxySimulation(pos.clone(), vel.clone(), mass.clone(), **kw)
            b = FlippedOrder(pos.clone(), vel.clone(), mass.clone(), **kw)
            tag = f"traj/{name}/{mode.value}"
            out[f"{tag}/acc0_relerr"] = np.float64((a.accelerations - b.accelerations).abs().max() / a.accelerations.abs().max())
            for _ in range(3):
                a.step()
                b.step()
            va, vb = a.velocities.double(), b.velocities.double()
            err = ((va - vb).abs().max(dim=1).values / va.abs().max()).numpy()
            out[f"{tag}/vel_frac_gt_2e-6"] = np.float64((err > 2e-6).mean())
            out[f"{tag}/vel_max"] = np.float64(err.max())
            out[f"{tag}/vel_q999"] = np.float64(np.quantile(err, 0.999))
            out[f"{tag}/pos_relerr"] = np.float64((a.positions.double() - b.positions.double()).abs().max() / a.positions.abs().max())
            ea, eb = a.get_total_energy(), b.get_total_energy()
            out[f"{tag}/energy_relerr"] = np.float64(abs(ea - eb) / abs(ea))
            out[f"{tag}/pos3"], out[f"{tag}/vel3"] = npy(a.positions), npy(a.velocities)
            out[f"{tag}/energy3"] = np.float64(ea)
            # ... and against itself on LAST-BIT-PERTURBED initial positions: a share `f` of the coordinates moved by one
            # fp32 ulp (seeded).  That is what any implementation whose fp32 force sums are not bit-identical to torch's
            # looks like after its first kick + drift: a rounding-level difference in a few coordinates, after which a
            # pair sitting on a bin edge lands in the neighbouring bin on one side of the comparison.
            for f in (0.02, 1.0):
                gen = torch.Generator().manual_seed(2100 + int(f * 100))
                sel = torch.rand(pos.shape, generator=gen) < f
                sign = torch.where(torch.rand(pos.shape, generator=gen) < 0.5, -1, 1).to(torch.int32)
                bits = pos.clone().view(torch.int32)
                # one ulp up or down in magnitude (sign-magnitude integers: +-1 on the bit pattern)
                pert = torch.where(sel, bits + sign, bits).view(torch.float32)
                c = ref_sim.GalaxySimulation(pert, vel.clone(), mass.clone(), **kw)
                for _ in range(3):
                    c.step()
                vc = c.velocities.double()
                errc = ((va - vc).abs().max(dim=1).values / va.abs().max()).numpy()
                ft = f"{tag}/ulp{int(f * 100)}"
                out[f"{ft}/vel_frac_gt_2e-6"] = np.float64((errc > 2e-6).mean())
                out[f"{ft}/vel_max"] = np.float64(errc.max())
                out[f"{ft}/vel_q999"] = np.float64(np.quantile(errc, 0.999))
                out[f"{ft}/pos_relerr"] = np.float64((a.positions.double() - c.positions.double()).abs().max() / a.positions.abs().max())
                out[f"{ft}/energy_relerr"] = np.float64(abs(ea - c.get_total_energy()) / abs(ea))
                print("G21", ft, "frac", out[f"{ft}/vel_frac_gt_2e-6"], "max", out[f"{ft}/vel_max"], "q999", out[f"{ft}/vel_q999"],
                      "E", out[f"{ft}/energy_relerr"])
            print("G21", tag, "frac", out[f"{tag}/vel_frac_gt_2e-6"], "max", out[f"{tag}/vel_max"], "q999", out[f"{tag}/vel_q999"],
                  "pos", out[f"{tag}/pos_relerr"], "E", out[f"{tag}/energy_relerr"])
    seeds = [15, 101, 102, 103, 104, 105, 106, 107]           # 15 = g15's system
    out["half/seeds"] = np.array(seeds)
    for si, seed in enumerate(seeds):
        pos, vel, mass = make_ics(193, 2, seed, True)
        out[f"half/ics{si}/pos"], out[f"half/ics{si}/vel"], out[f"half/ics{si}/mass"] = npy(pos), npy(vel), npy(mass)
        for grp, cast in (("half", lambda t: t.half()), ("bf16", lambda t: t.bfloat16())):
            for mode in (PrecisionMode.INT8_SIM, PrecisionMode.INT4_SIM):
                kw = dict(precision_mode=mode, G=0.001, softening=0.1, dt=0.01, device=torch.device("cpu"))
                with Spy() as spy:
                    a = ref_sim.GalaxySimulation(cast(pos), cast(vel), cast(mass), **kw)
                b = FlippedOrder(cast(pos), cast(vel), cast(mass), **kw)
                fin, flv, fout = spy.lin[0]
                step = (float(fin.max()) - float(fin.min())) / (flv - 1)
                diff = (a.accelerations.double() - b.accelerations.double()).abs().numpy()
                tag = f"half/{grp}/{mode.value}/{si}"
                out[f"{tag}/acc0"] = npy(a.accelerations.double())
                out[f"{tag}/step"] = np.float64(step)
                out[f"{tag}/frac_gt_half_step"] = np.float64((diff > 0.5 * step).mean())
                out[f"{tag}/max_in_steps"] = np.float64(diff.max() / step)
        print("G21 half seed", seed, {k.split("/", 1)[1]: float(v) for k, v in out.items()
                                      if k.endswith(f"/{si}/frac_gt_half_step")})
    np.savez_compressed(os.path.join(OUT, "g21_reference_self_noise.npz"), **out)
    print("G21 done")


def g14():
    """The reference's own state hash (reproducibility.py:227-232) on golden states."""
    import reproducibility as ref_repro
    g2_ = np.load(os.path.join(OUT, "g2_config1_n1024.npz"))
    pos, vel = torch.from_numpy(g2_["pos"]), torch.from_numpy(g2_["vel"])
    out = {
        "float32": ref_repro.hash_tensor_state(pos, vel),
        "float64": ref_repro.hash_tensor_state(pos.double(), vel.double()),
        "float16": ref_repro.hash_tensor_state(pos.half(), vel.half()),
        "float64_tick200": ref_repro.hash_tensor_state(torch.from_numpy(g2_["float64/pos200"]),
                                                       torch.from_numpy(g2_["float64/vel200"])),
    }
    json.dump(out, open(os.path.join(OUT, "g14_state_hash.json"), "w"), indent=1)
    print("G14", out)


def g23_edge_values():
    """Edge values through the stock class: every kind of tests/edge_cases.py (NaN / infinite / runaway coordinates,
    two runaways on one side, massless stars, a NaN mass) at N = 48, edge star n - 1, in 2-D and 3-D, fp32 and fp64 inputs, all seven modes.
    Per (dim, input dtype) group: the inputs of every kind, and per (kind, mode) the accelerations, both energies and
    the state after two steps, stacked along the first axis in the order of `cases`."""
    sys.path.insert(0, os.path.dirname(OUT))
    import edge_cases as E
    n = 48
    out = {"kinds": np.array(E.KINDS), "modes": np.array([m.value for m in MODES])}
    for dim in (2, 3):
        for f64 in (False, True):
            grp = f"d{dim}/{'f64' if f64 else 'f32'}"
            ins = [E.make(kind, n, dim, 23 + dim, f64, idx=E.variants(kind, n, every_index=False)[0]) for kind in E.KINDS]
            for k, name in enumerate(("pos", "vel", "mass")):
                out[f"{grp}/{name}"] = np.stack([c[k] for c in ins])
            rec = {key: [] for key in ("acc0", "e0", "pos2", "vel2", "e2")}
            for pos, vel, mass, _ in ins:
                for mode in MODES:
                    sim = ref_sim.GalaxySimulation(torch.from_numpy(pos.copy()), torch.from_numpy(vel.copy()),
                                                   torch.from_numpy(mass.copy()), precision_mode=mode, G=0.001, dt=0.01,
                                                   softening=0.1)
                    rec["acc0"].append(npy(sim.accelerations).astype(np.float64))
                    rec["e0"].append([sim.get_kinetic_energy(), sim.get_potential_energy()])
                    sim.step()
                    sim.step()
                    rec["pos2"].append(npy(sim.positions).astype(np.float64))
                    rec["vel2"].append(npy(sim.velocities).astype(np.float64))
                    rec["e2"].append([sim.get_kinetic_energy(), sim.get_potential_energy()])
            for key, rows in rec.items():
                out[f"{grp}/{key}"] = np.array(rows, np.float64)
    np.savez_compressed(os.path.join(OUT, "g23_edge_values.npz"), **out)
    print("G23 done")


if __name__ == "__main__":
    which = sys.argv[1:] or ["g1", "g1c", "g2", "g3", "g4", "g5", "g6", "g7", "g8", "g9", "g10", "g11", "g12", "g13", "g14", "g15", "g16", "g17", "g18", "g19", "g20", "g21", "g23_edge_values"]
    for w in which:
        globals()[w]()
