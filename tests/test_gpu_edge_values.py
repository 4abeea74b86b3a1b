"""Every pair kernel on edge values (tests/edge_cases.py) against the oracle, which test_oracle_golden.py's
test_g23_edge_values ties to the reference on the same kinds of input: NaN, infinite and runaway coordinates (r2
overflows), a star whose r^3 overflows but whose r2 does not, massless stars beside distinct and beside equal masses, all
masses 0, a NaN mass.

ROWS lists one shape per kernel family and variant, the smallest at which the kernel can still go wrong (knobs from
tests/plan_shapes.py): the one-launch small-system kernel on both sides of its 1024-source LDS tile, the ensemble kernel,
the pair-symmetric kernels with 1 / 2 / 4 targets per lane, every hand-off (NB_SYM_ROT) and row-split items, the one-sided
kernels with 1 / 2 / 4 targets per thread, the generic per-pair kernel, fp32-typed state in FLOAT64 mode (fp32 pair
arithmetic on fp64 storage, then narrow masses).  A test is one (row, kind); it runs the kind once per edge index
(10, n // 2 + 3, n - 1) where the kind edits one star, and the coordinate kinds with equal masses as well (the UNIFORM
kernels, where only the distance silences the padding).  Each run
  * asserts force_kernel_name() and, for every energy, pe_kernel_name() against plan_shapes.pe_variant;
  * compares the constructor's accelerations and both energies with the oracle through edge_cases.compare (classes must
    match; finite values at the bars of test_gpu_plan_shapes.py / test_gpu_energy_shapes.py for that kernel and mode);
  * runs three ticks and compares positions, velocities and the energies of the final state (another PE variant once
    fp32-typed positions have been promoted) the same way;
  * runaway kinds: the runaway star's acceleration is exactly 0, its position after three ticks is bit-equal to the
    oracle's (it flies on ballistically), and the OTHER stars are compared on their own (the array maximum is the runaway
    coordinate, against which any error of theirs would vanish).
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import edge_cases as E
import plan_shapes as S

pytestmark = pytest.mark.gpu

MODE_CODES = {"float64": 0, "float32": 1, "bfloat16": 2, "float16": 3, "int8_sim": 4, "int4_sim": 5, "custom": 6}
CODE = {torch.float16: S.DT_F16, torch.bfloat16: S.DT_BF16, torch.float32: S.DT_F32, torch.float64: S.DT_F64}
F64, F32 = torch.float64, torch.float32
SMALL, ENS, GENERIC = "small_step_kernel", "ens_step_kernel", "generic_force_kernel"
SYM = {"NB_SYM": "1", "NB_NO_SMALLN": "1"}
ONE = {"NB_SYM": "0", "NB_NO_SMALLN": "1"}
CLASSIC4 = {**SYM, "NB_SYM_R": "4", "NB_SYM_ROWSPLIT": "0"}
INT8_KINDS = ("nan-coord", "massless", "nan-mass")


def row(rid, kernel, n, dim, dtypes, mode, env=None, kinds=E.KINDS, every_index=False):
    """dtypes: torch dtypes of (positions, velocities, masses) as handed to the constructor."""
    return dict(id=rid, kernel=kernel, n=n, dim=dim, dtypes=dtypes, mode=mode, env=dict(env or {}), kinds=kinds,
                every_index=every_index)


A64, A32, M64 = (F64, F64, F64), (F32, F32, F32), (F32, F32, F64)
ROWS = [
    # ---- the one-launch small-system kernel: inside one 1024-source LDS tile, and one star past it
    row("small-f64-d2-65", SMALL, 65, 2, A64, "float64", every_index=True),
    row("small-f64-d3-65", SMALL, 65, 3, A64, "float64"),
    row("small-f64-d2-1025", SMALL, 1025, 2, A64, "float64"),
    row("small-f64-d3-1025", SMALL, 1025, 3, A64, "float64", every_index=True),
    row("small-f32-d2-65", SMALL, 65, 2, A32, "float32"),
    row("small-f32-d3-65", SMALL, 65, 3, A32, "float32", every_index=True),
    row("small-f32-d2-1025", SMALL, 1025, 2, A32, "float32", every_index=True),
    row("small-f32-d3-1025", SMALL, 1025, 3, A32, "float32"),
    row("small-bf16-d2-1025", SMALL, 1025, 2, A32, "bfloat16"),
    row("small-f16-d3-65", SMALL, 65, 3, A32, "float16"),
    # ---- pair-symmetric, fp64
    # (N = 1000 with four targets per lane is a row-split plan unless NB_SYM_ROWSPLIT=0 asks for classic work items)
    row("sym64-d2-r4-dpp", S.SYM64, 1000, 2, A64, "float64", {**CLASSIC4, "NB_SYM_ROT": "2"}, every_index=True),
    row("sym64-d2-r4-lanes", S.SYM64, 1000, 2, A64, "float64", {**CLASSIC4, "NB_SYM_ROT": "0"}, every_index=True),
    row("sym64-d2-r4-lds", S.SYM64, 1000, 2, A64, "float64", {**CLASSIC4, "NB_SYM_ROT": "1"}),
    row("sym64-d2-r2", S.SYM64, 1000, 2, A64, "float64", {**SYM, "NB_SYM_R": "2"}),
    row("sym64-d2-r1", S.SYM64, 1000, 2, A64, "float64", {**SYM, "NB_SYM_R": "1"}),
    row("sym64-d3-r4", S.SYM64, 1000, 3, A64, "float64", {**SYM, "NB_SYM_R": "4"}, every_index=True),
    row("sym64-d2-rowsplit2", S.SYM64, 2100, 2, A64, "float64", {**SYM, "NB_SYM_R": "4", "NB_SYM_ROWSPLIT": "2"}),
    row("sym64-d2-rowsplit2-lanes", S.SYM64, 2100, 2, A64, "float64",
        {**SYM, "NB_SYM_R": "4", "NB_SYM_ROWSPLIT": "2", "NB_SYM_ROT": "0"}),
    # ---- pair-symmetric, fp32 family
    *[row(f"sym32-{mode}-d{dim}-r2", S.SYM32, 1100, dim, A32, mode, SYM, every_index=(mode == "float32" and dim == 2))
      for mode in ("float32", "bfloat16", "float16") for dim in (2, 3)],
    *[row(f"sym32-{mode}-d{dim}-r4", S.SYM32, 3000, dim, A32, mode, {**SYM, "NB_SYM_R": "4"})
      for mode in ("float32", "bfloat16", "float16") for dim in (2, 3)],
    row("sym32-int8-d2-r2", S.SYM32, 1100, 2, A32, "int8_sim", SYM, kinds=INT8_KINDS),
    row("sym32-int8-d3-r4", S.SYM32, 3000, 3, A32, "int8_sim", {**SYM, "NB_SYM_R": "4"}, kinds=INT8_KINDS),
    # ---- one-sided
    row("one64-d2-r1", S.ONE64, 1000, 2, A64, "float64", {**ONE, "NB_R": "1"}),
    row("one64-d3-r2", S.ONE64, 1000, 3, A64, "float64", {**ONE, "NB_R": "2"}),
    row("one64-d2-r4", S.ONE64, 1000, 2, A64, "float64", {**ONE, "NB_R": "4"}, every_index=True),
    row("one32-d2", S.ONE32, 1000, 2, A32, "float32", ONE, every_index=True),
    row("one32-d3", S.ONE32, 1000, 3, A32, "float32", ONE),
    # ---- fp32-typed state in FLOAT64 mode: fp32 pair arithmetic on fp64 storage at tick 0, fp64 positions beside fp32
    #      masses (the narrow-mass PE variants) after the ticks
    row("f32in64-sym-d2-r4", S.SYM64, 1000, 2, A32, "float64", {**SYM, "NB_SYM_R": "4"}),
    row("f32in64-sym-d3-r2", S.SYM64, 1000, 3, A32, "float64", {**SYM, "NB_SYM_R": "2"}),
    row("f32in64-one-d2", S.ONE64, 1000, 2, A32, "float64", ONE),
    # ---- the generic per-pair kernel: fp64 masses beside fp32 positions under a cast mode (test_gpu_generic_shapes.py)
    row("generic-m64-float32-d2", GENERIC, 257, 2, M64, "float32"),
    row("generic-m64-float16-d3", GENERIC, 257, 3, M64, "float16"),
]
CASES = [(r, kind) for r in ROWS for kind in r["kinds"]]


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def held(a, dtype):
    """The values of `a` as a tensor of `dtype` holds them, as fp64."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).double().numpy()


@functools.lru_cache(maxsize=None)
def reference(kind, n, dim, dtypes, mode, idx, uniform):
    """One run of the oracle, shared by every row of the same shape, dtypes and mode."""
    from oracle import oracle as O
    pos, vel, mass, stars = E.make(kind, n, dim, n + dim, dtypes[0] == F64, idx=idx, uniform=uniform)
    ins = tuple(held(a, t) for a, t in zip((pos, vel, mass), dtypes))
    sim = O.OracleSim(*ins, mode, codes=tuple(CODE[t] for t in dtypes))
    out = dict(ins=ins, stars=stars, acc0=np.asarray(sim.accelerations, np.float64), ke0=sim.get_kinetic_energy(),
               pe0=sim.get_potential_energy(), step=None)
    if mode in ("int8_sim", "int4_sim"):       # one force-grid step, as test_gpu_plan_shapes.check_dense measures it
        _, dbg = O.accelerations(ins[0], ins[2], mode, debug=True, pos_code=CODE[dtypes[0]], mass_code=CODE[dtypes[2]])
        out["step"] = (dbg["fmax"] - dbg["fmin"]) / ({"int8_sim": 256, "int4_sim": 16}[mode] - 1)
    sim.run(3)
    out.update(pos3=np.asarray(sim.positions, np.float64), vel3=np.asarray(sim.velocities, np.float64),
               acc3=np.asarray(sim.accelerations, np.float64), codes3=tuple(sim.codes))
    return out


def oracle_energies(sim):
    """The oracle's (kinetic, potential) energy of the state the engine holds, in the engine's dtypes: the state after
    the ticks differs from the oracle's own by the force bars, which the energy kernels are not to be measured against."""
    from oracle import oracle as O
    pos, vel, mass = (O.as_f64(t.double().numpy()) for t in (sim.positions, sim.velocities, sim.masses))
    pc, vc, mc = (CODE[t.dtype] for t in (sim.positions, sim.velocities, sim.masses))
    n, d = pos.shape
    ke = O.lib().nbo_kinetic_energy(n, d, vc, O._dp(vel), mc, O._dp(mass))
    pe = O.lib().nbo_potential_energy(n, d, pc, O._dp(pos), mc, O._dp(mass), float(sim.G), float(sim.softening) ** 2, 0, n)
    return ke, pe


def bars(r, sim):
    """(acc, pos, vel) bars of the row: test_gpu_plan_shapes.py's for its kernel and mode."""
    if r["mode"] == "float64" and r["dtypes"] == A64:
        return 1e-13, 1e-13, 1e-12                      # check_dense: forces, three steps
    if r["mode"] in ("int8_sim", "int4_sim"):
        return None, 1e-4, 1e-4                         # one force-grid step; test_gpu_generic_shapes.py's ptol
    return 2e-6, 5e-6, 5e-6                             # fp32 family: check_dense, _small_step_checks


def energy_bar(sim):
    """test_gpu_energy_shapes.py: fp64 terms on fp64 positions 1e-12, everything else 2e-6."""
    return 1e-12 if (sim.positions.dtype == F64 and sim.masses.dtype == F64) else 2e-6


def check_energies(r, kind, sim, p, uniform, ke_ref, pe_ref, tag, log):
    storage_f64 = r["mode"] == "float64" or F64 in r["dtypes"]
    bar = energy_bar(sim)
    log.append(("ke", E.compare([sim.get_kinetic_energy()], [ke_ref], bar, kind, tag + " kinetic")))
    pe = sim.get_potential_energy()
    want = S.pe_variant(p, r["dim"], storage_f64, CODE[sim.positions.dtype], CODE[sim.masses.dtype], uniform,
                        no_pe_sym="NB_NO_PE_SYM" in r["env"])
    assert sim.pe_kernel_name() == want, (tag, sim.pe_kernel_name(), want)
    print(f"{tag}: PE {pe!r} oracle {pe_ref!r} [{want}]")
    log.append(("pe", E.compare([pe], [pe_ref], bar, kind, tag + " potential")))


def check_plan(r, p):
    """The shape the row's knobs ask for is the one the planner hands out (the knobs must be in the environment)."""
    env = r["env"]
    if r["kernel"] in (S.SYM64, S.SYM32):
        assert p["enabled"], (r["id"], p)
        assert p["r"] == int(env.get("NB_SYM_R", p["r"])), (r["id"], p)
        assert p["rowsplit"] == int(env.get("NB_SYM_ROWSPLIT", p["rowsplit"])), (r["id"], p)
    elif r["kernel"] in (S.ONE64, S.ONE32):
        assert not p["enabled"], (r["id"], p)
        assert p["onesided_r"] == int(env.get("NB_R", p["onesided_r"])), (r["id"], p)


def run_one(nb, cus, r, kind, idx, uniform):
    ref = reference(kind, r["n"], r["dim"], r["dtypes"], r["mode"], idx, uniform)
    stars = list(ref["stars"])
    tag = f"{r['id']} {kind} idx={idx}{' equal-masses' if uniform else ''}"
    P, V, M = (torch.from_numpy(a).to(t) for a, t in zip(ref["ins"], r["dtypes"]))
    mass_equal = bool(np.isfinite(ref["ins"][2]).all() and ref["ins"][2].min() == ref["ins"][2].max())
    storage_f64 = r["mode"] == "float64" or F64 in r["dtypes"]
    p = S.plan(r["n"], r["dim"], 0, 1, storage_f64, MODE_CODES[r["mode"]], cus=cus, work=False)
    check_plan(r, p)
    sim = nb.GalaxySimulation(P, V, M, precision_mode=nb.PrecisionMode(r["mode"]))
    log = []
    try:
        # a small system's first evaluation runs on the tiled kernel of its plan; the one-launch kernel takes the steps
        first = r["kernel"]
        if first == SMALL:
            first = (S.SYM64 if storage_f64 else S.SYM32) if p["enabled"] else (S.ONE64 if storage_f64 else S.ONE32)
        assert sim.force_kernel_name() == first, (tag, sim.force_kernel_name(), first)
        acc_bar, pos_bar, vel_bar = bars(r, sim)
        acc = sim.accelerations.double().numpy()
        if acc_bar is None:
            finite = np.isfinite(ref["acc0"])
            acc_bar = 1.01 * ref["step"] / np.abs(ref["acc0"][finite]).max() if finite.any() else 2e-6
        log.append(("acc", E.compare(acc, ref["acc0"], acc_bar, kind, tag + " accelerations", from_forces=True)))
        if kind in E.FAR_KINDS:
            # (runaways exactly 0: test_runaway_star_feels_exactly_nothing, which knows the one family that misses it)
            rest = np.delete(np.arange(r["n"]), stars)
            log.append(("acc-rest", E.compare(acc[rest], ref["acc0"][rest], acc_bar, kind, tag + " forces of the rest")))
        if kind == "all-massless":
            assert np.all(acc == 0), f"{tag}: forces of massless stars"
        check_energies(r, kind, sim, p, mass_equal, ref["ke0"], ref["pe0"], tag + " tick 0", log)
        sim.run(3)
        names = {S.DT_F16: torch.float16, S.DT_BF16: torch.bfloat16, S.DT_F32: F32, S.DT_F64: F64}
        assert [sim.positions.dtype, sim.velocities.dtype, sim.masses.dtype] == [names[c] for c in ref["codes3"][:3]], tag
        pos, vel = sim.positions.double().numpy(), sim.velocities.double().numpy()
        log.append(("pos", E.compare(pos, ref["pos3"], pos_bar, kind, tag + " positions", from_forces=True)))
        log.append(("vel", E.compare(vel, ref["vel3"], vel_bar, kind, tag + " velocities", from_forces=True)))
        if kind in E.RUNAWAY_KINDS:
            assert np.array_equal(pos[stars], ref["pos3"][stars]), \
                f"{tag}: the runaway star is at {pos[stars]!r}, the oracle's at {ref['pos3'][stars]!r}"
        if kind in E.FAR_KINDS:
            log.append(("pos-rest", E.compare(pos[rest], ref["pos3"][rest], pos_bar, kind, tag + " positions of the rest")))
            log.append(("vel-rest", E.compare(vel[rest], ref["vel3"][rest], vel_bar, kind, tag + " velocities of the rest")))
        if r["kernel"] == SMALL:
            assert sim.force_kernel_name() == SMALL, (tag, sim.force_kernel_name())
        if r["mode"] in ("float64", "float32"):
            # the last tick's forces (the half-precision hooks are left out: one ulp of state can move a pair's r2 across
            # a rounding boundary of the hook, a step of 2^-8 or 2^-11 in that pair's force)
            acc3 = sim.accelerations.double().numpy()
            log.append(("acc3", E.compare(acc3, ref["acc3"], acc_bar, kind, tag + " forces, tick 3", from_forces=True)))
            if kind in E.RUNAWAY_KINDS:
                # (fp32-typed positions promoted to fp64 by the first drift are no runaway any more: 3e19 squared is finite)
                still = ref["acc3"][stars] == 0
                assert still.all() or (r["mode"] == "float64" and r["dtypes"] == A32), tag
                assert np.all(acc3[stars][still] == 0), f"{tag}: the runaway star's force at tick 3 is {acc3[stars]!r}"
            if kind in E.FAR_KINDS:
                log.append(("acc3-rest", E.compare(acc3[rest], ref["acc3"][rest], acc_bar, kind, tag + " tick 3, the rest")))
        ke3, pe3 = oracle_energies(sim)
        check_energies(r, kind, sim, p, mass_equal, ke3, pe3, tag + " tick 3", log)
    finally:
        print(f"{tag} [{r['kernel']}]: " + " ".join(f"{k}={v:.2e}" for k, v in log))
        sim.close()


@pytest.mark.parametrize("case", CASES, ids=[f"{r['id']}-{kind}" for r, kind in CASES])
def test_edge_values_vs_oracle(nb, cus, monkeypatch, case):
    r, kind = case
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    for idx in E.variants(kind, r["n"], r["every_index"]):
        for uniform in ((False, True) if kind in E.COORD_KINDS else (False,)):
            run_one(nb, cus, r, kind, idx, uniform)


F32PAIR_REASON = ("fp32 pair arithmetic on fp64 storage (fp32-typed positions in FLOAT64 mode, first evaluation only): r2 "
                  "is formed in fp32, where the staging keeps it below 3.4e38, but q^(-3/2) is taken in fp64, where "
                  "(1e37)^(-3/2) = 3e-56 does not underflow -- the runaway star's row is ~1e-37 instead of exactly 0 (the "
                  "size of a padding particle's contribution there); exact would need an instruction in the pair loop "
                  "(DESIGN.md 4.10)")


def _zero_marks(r):
    f32pair = r["mode"] == "float64" and r["dtypes"] == A32
    return [pytest.mark.xfail(strict=True, reason=F32PAIR_REASON)] if f32pair else []


ZERO_CASES = [pytest.param(r, kind, id=f"{r['id']}-{kind}", marks=_zero_marks(r))
              for r in ROWS for kind in E.RUNAWAY_KINDS if kind in r["kinds"]]


@pytest.mark.parametrize("r,kind", ZERO_CASES)
def test_runaway_star_feels_exactly_nothing(nb, monkeypatch, r, kind):
    """The constructor's acceleration of a runaway star is exactly +-0 in every row, as upstream's G / inf ** 1.5."""
    for k, v in r["env"].items():
        monkeypatch.setenv(k, v)
    for idx in E.variants(kind, r["n"], r["every_index"]):
        for uniform in (False, True):
            ref = reference(kind, r["n"], r["dim"], r["dtypes"], r["mode"], idx, uniform)
            P, V, M = (torch.from_numpy(a).to(t) for a, t in zip(ref["ins"], r["dtypes"]))
            sim = nb.GalaxySimulation(P, V, M, precision_mode=nb.PrecisionMode(r["mode"]))
            try:
                got = sim.accelerations.double().numpy()[list(ref["stars"])]
            finally:
                sim.close()
            print(f"{r['id']} {kind} idx={idx} equal={uniform}: runaway rows {got.tolist()}")
            assert np.all(ref["acc0"][list(ref["stars"])] == 0)
            assert np.all(got == 0), f"{r['id']} {kind} idx={idx}: the runaway star's acceleration is {got!r}, not 0"


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("mode", ["float64", "float32"])
def test_ensemble_edge_member_stays_alone(nb, mode, dim, kind):
    """ens_step_kernel and the ensemble's energy kernel, B = 3, N = 257, the edge member in the middle, every kind: it
    follows the oracle like a solo system, and the two clean members are bit-identical to an ensemble that never held it."""
    n, t = 257, (F64 if mode == "float64" else F32)
    dtypes = (t, t, t)
    idx = E.variants(kind, n, every_index=False)[0]
    ref = reference(kind, n, dim, dtypes, mode, idx, False)
    clean = [tuple(held(a, t) for a in E.inputs(n, dim, 100 + b, t == F64)) for b in (0, 2)]
    members = [clean[0], ref["ins"], clean[1]]
    stack = lambda ms, k: torch.from_numpy(np.stack([m[k] for m in ms])).to(t)
    ens = nb.GalaxyEnsemble(stack(members, 0), stack(members, 1), stack(members, 2), precision_mode=nb.PrecisionMode(mode))
    alone = nb.GalaxyEnsemble(stack(clean, 0), stack(clean, 1), stack(clean, 2), precision_mode=nb.PrecisionMode(mode))
    try:
        assert ens.force_kernel_name() == ENS and alone.force_kernel_name() == ENS
        f64 = mode == "float64"
        acc_bar, pos_bar, vel_bar, e_bar = (1e-13, 1e-13, 1e-12, 1e-12) if f64 else (2e-6, 5e-6, 5e-6, 2e-6)
        tag = f"ensemble {mode} d{dim} {kind}"
        log = []

        def same_clean(what):
            for name in ("positions", "velocities", "accelerations"):
                a, b = getattr(ens, name).cpu(), getattr(alone, name).cpu()
                assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[1]), f"{tag}: clean members' {name} differ {what}"

        acc = ens.accelerations[1].double().cpu().numpy()
        log.append(("acc", E.compare(acc, ref["acc0"], acc_bar, kind, tag + " accelerations", from_forces=True)))
        if kind in E.RUNAWAY_KINDS:
            assert np.all(acc[list(ref["stars"])] == 0), tag
        log.append(("ke", E.compare([ens.get_kinetic_energy()[1]], [ref["ke0"]], e_bar, kind, tag + " kinetic")))
        log.append(("pe", E.compare([ens.get_potential_energy()[1]], [ref["pe0"]], e_bar, kind, tag + " potential")))
        same_clean("at tick 0")
        ens.run(3)
        alone.run(3)
        same_clean("after three ticks")
        pos = ens.positions[1].double().cpu().numpy()
        log.append(("pos", E.compare(pos, ref["pos3"], pos_bar, kind, tag + " positions", from_forces=True)))
        log.append(("vel", E.compare(ens.velocities[1].double().cpu().numpy(), ref["vel3"], vel_bar, kind, tag + " velocities",
                                     from_forces=True)))
        if kind in E.RUNAWAY_KINDS:
            s = list(ref["stars"])
            assert np.array_equal(pos[s], ref["pos3"][s]), tag
        if kind in E.FAR_KINDS:
            rest = np.delete(np.arange(n), list(ref["stars"]))
            log.append(("acc-rest", E.compare(acc[rest], ref["acc0"][rest], acc_bar, kind, tag + " forces of the rest")))
            log.append(("pos-rest", E.compare(pos[rest], ref["pos3"][rest], pos_bar, kind, tag + " positions of the rest")))
        from oracle import oracle as O           # the oracle's energy of the state the member holds now
        m64 = O.as_f64(ens.masses[1].double().cpu().numpy())
        pe3 = O.lib().nbo_potential_energy(n, dim, CODE[t], O._dp(O.as_f64(pos)), CODE[t], O._dp(m64), 0.001, 0.01, 0, n)
        log.append(("pe3", E.compare([ens.get_potential_energy()[1]], [pe3], e_bar, kind, tag + " potential, tick 3")))
        print(f"{tag}: " + " ".join(f"{k}={v:.2e}" for k, v in log))
    finally:
        ens.close()
        alone.close()
