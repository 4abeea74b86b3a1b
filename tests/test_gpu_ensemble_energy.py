"""The ensemble's batched energies on the GPU: energies() and run_recorded() against the CPU oracle and the ensemble's own
solo-equal read-out, member indexing at B = 1024, determinism, independence of the members, the recorded run against
twins driven by run() and step(), a NaN member, and the zero-softening rule.

Inputs and per-member G / softening / dt are test_gpu_ensemble's (B = 5, member 3 with uniform masses).  Bars are those
of test_gpu_energy_shapes: relative error 1e-12 under FLOAT64, 2e-6 for the fp32 family, kinetic and potential compared
separately (never their cancelling sum).  The energy kernel cuts a member into tiles of 256 stars and takes one
workgroup per tile pair, so the shapes sit around the tile: no pair at all, one pair, less than a wave, exactly one
tile, one star into a second tile (the first off-diagonal tile pair), three tiles, and the largest tile counts.
"""
import functools

import numpy as np
import pytest
import torch

from test_gpu_ensemble import B, G_, SOFT, DT, UNIFORM_MEMBER, T, members, make_ens, snapshot, same
from test_gpu_plan_shapes import inputs

pytestmark = pytest.mark.gpu

TOL = {"float64": 1e-12, "float32": 2e-6, "bfloat16": 2e-6, "float16": 2e-6}

CASES = [
    (1, 2, "float64"), (2, 3, "float32"), (37, 3, "float64"), (256, 2, "float32"), (257, 3, "float64"),
    (513, 2, "float32"), (1300, 2, "bfloat16"), (3073, 3, "float64"),
]
IDS = [f"n{n}-d{d}-{m}" for n, d, m in CASES]


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def close_to(got, ref, tol, what):
    """Relative to the reference's own value; a reference of exactly 0 (no pair) must be met exactly."""
    got, ref = float(got), float(ref)
    if ref == 0.0:
        assert got == 0.0, f"{what}: {got!r} where the reference is 0"
        return 0.0
    err = abs(got - ref) / abs(ref)
    print(f"{what}: got {got!r} reference {ref!r} relerr {err:.3e}")
    assert err <= tol, f"{what}: relative error {err:.3e} > {tol:.1e} (got {got!r}, reference {ref!r})"
    return err


def oracle_energies(pos, vel, mass, mode, G, softening, dt):
    from oracle import oracle as O
    sim = O.OracleSim(pos, vel, mass, mode, G=G, softening=softening, dt=dt)
    return sim.get_kinetic_energy(), sim.get_potential_energy()


def bits(t):
    """float64 tensor -> int64 numpy view: equality of these is bit equality, NaN payloads included."""
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def check_shapes(ke, pe, members_):
    for t in (ke, pe):
        assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == (members_,)


# ---- 1. against the CPU oracle and the solo-equal read-out -------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_energies_match_the_oracle_and_the_solo_equal_values(nb, case):
    n, d, mode = case
    e = make_ens(nb, case)
    e.run(2)
    ke, pe = e.energies()
    check_shapes(ke, pe, B)
    assert ke.device == e.device and pe.device == e.device
    pos, vel, mass = e.positions.numpy(), e.velocities.numpy(), e.masses.numpy()
    ke_solo, pe_solo = e.get_kinetic_energy(), e.get_potential_energy()
    for b in range(B):
        ke_ref, pe_ref = oracle_energies(pos[b], vel[b], mass[b], mode, G_[b], SOFT[b], DT[b])
        what = f"{IDS[CASES.index(case)]} member {b}"
        close_to(ke[b], ke_ref, TOL[mode], what + " kinetic vs oracle")
        close_to(pe[b], pe_ref, TOL[mode], what + " potential vs oracle")
        close_to(ke[b], ke_solo[b], TOL[mode], what + " kinetic vs get_kinetic_energy()")
        close_to(pe[b], pe_solo[b], TOL[mode], what + " potential vs get_potential_energy()")
        if n == 1:
            assert float(pe[b]) == 0.0 and float(ke[b]) > 0.0
    # the evaluation leaves the state alone
    same(snapshot(e), (pos, vel, e.accelerations.numpy()), "state after energies()")
    assert np.array_equal(e.positions.numpy(), pos) and np.array_equal(e.velocities.numpy(), vel)
    e.close()


# ---- 2. member indexing at the cap ----------------------------------------------------------------------------------------
def test_every_member_of_1024_is_its_own(nb):
    members_, n, d = 1024, 8, 2
    ms = [inputs(n, d, 7000 + b, False, uniform=(b % 97 == 5)) for b in range(members_)]
    p, v, m = (np.stack([x[k] for x in ms]) for k in range(3))
    G = [0.001 * (1 + 0.37 * ((b * 7) % 101) / 101) for b in range(members_)]
    soft = [0.05 + 0.1 * ((b * 13) % 89) / 89 for b in range(members_)]
    e = nb.GalaxyEnsemble(T(p), T(v), T(m), precision_mode=nb.PrecisionMode.FLOAT32, G=G, softening=soft, dt=0.01)
    e.run(1)
    ke, pe = e.energies()
    check_shapes(ke, pe, members_)
    pos, vel, mass = e.positions.numpy(), e.velocities.numpy(), e.masses.numpy()
    worst = 0.0
    for b in range(members_):
        ke_ref, pe_ref = oracle_energies(pos[b], vel[b], mass[b], "float32", G[b], soft[b], 0.01)
        for got, ref, name in ((ke[b], ke_ref, "kinetic"), (pe[b], pe_ref, "potential")):
            err = abs(float(got) - ref) / abs(ref)
            worst = max(worst, err)
            assert err <= 2e-6, f"member {b} {name}: relative error {err:.3e} (got {float(got)!r}, reference {ref!r})"
    print(f"B = 1024: worst relative error {worst:.3e}")
    e.close()


# ---- 3. determinism and independence --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(257, 3, "float64"), (513, 2, "float32"), (1300, 2, "bfloat16")],
                         ids=["n257-d3-float64", "n513-d2-float32", "n1300-d2-bfloat16"])
def test_energies_are_deterministic_and_independent_of_the_neighbours(nb, case):
    e = make_ens(nb, case)
    e.run(2)
    k1, p1 = e.energies()
    k2, p2 = e.energies()
    assert np.array_equal(bits(k1), bits(k2)) and np.array_equal(bits(p1), bits(p2))
    e.close()
    rev = list(reversed(range(B)))
    r = make_ens(nb, case, rev)
    r.run(2)
    kr, pr = r.energies()
    assert np.array_equal(bits(kr), bits(k1)[rev]) and np.array_equal(bits(pr), bits(p1)[rev])
    r.close()
    alone = make_ens(nb, case, [UNIFORM_MEMBER])
    alone.run(2)
    ka, pa = alone.energies()
    assert bits(ka)[0] == bits(k1)[UNIFORM_MEMBER] and bits(pa)[0] == bits(p1)[UNIFORM_MEMBER]
    alone.close()


# ---- 4. the recorded run against twins ------------------------------------------------------------------------------------
T0 = 3


@pytest.mark.parametrize("case", [(700, 2, "float64"), (1025, 2, "float32")], ids=["n700-d2-float64", "n1025-d2-float32"])
def test_run_recorded_against_twins(nb, case):
    # a twin driven by step(): its energies() after every tick are what the samples must equal bit for bit
    c = make_ens(nb, case)
    c.run(T0)
    want = {T0: c.energies()}
    for t in range(T0 + 1, T0 + 10):
        c.step()
        want[t] = c.energies()
    c.close()
    # a twin driven by run()
    twin = make_ens(nb, case)
    twin.run(T0)
    twin.run(5)
    state5 = snapshot(twin)
    twin.run(4)
    state9 = snapshot(twin)
    twin.close()

    e = make_ens(nb, case)
    e.run(T0)
    before = e.launches()
    h = e.run_recorded(5, every=2)
    assert isinstance(h, nb.EnergyHistory) and h.ticks == [T0, T0 + 2, T0 + 4]
    assert e.tick == T0 + 5 and e.launches() - before == 5
    same(snapshot(e), state5, "run_recorded(5, every=2) vs run(5)")
    for t in (h.kinetic, h.potential, h.total):
        assert t.dtype == torch.float64 and tuple(t.shape) == (3, B) and t.device == e.device
    for s, tick in enumerate(h.ticks):
        assert np.array_equal(bits(h.kinetic[s]), bits(want[tick][0])), f"kinetic of sample {s} (tick {tick})"
        assert np.array_equal(bits(h.potential[s]), bits(want[tick][1])), f"potential of sample {s} (tick {tick})"
    assert torch.equal(h.total, h.kinetic + h.potential)

    h2 = e.run_recorded(4, every=2)
    assert h2.ticks == [T0 + 5, T0 + 7, T0 + 9] and e.tick == T0 + 9 and e.launches() - before == 9
    same(snapshot(e), state9, "second run_recorded vs run(5) + run(4)")
    for s, tick in enumerate(h2.ticks):
        assert np.array_equal(bits(h2.kinetic[s]), bits(want[tick][0])), f"second call, kinetic of sample {s}"
        assert np.array_equal(bits(h2.potential[s]), bits(want[tick][1])), f"second call, potential of sample {s}"
    ke, pe = e.energies()
    assert np.array_equal(bits(h2.kinetic[-1]), bits(ke)) and np.array_equal(bits(h2.potential[-1]), bits(pe))
    e.close()

    e = make_ens(nb, case)
    e.run(T0)
    h1 = e.run_recorded(5, every=1)
    assert h1.ticks == [T0 + t for t in range(6)] and tuple(h1.kinetic.shape) == (6, B) and e.tick == T0 + 5
    same(snapshot(e), state5, "run_recorded(5, every=1) vs run(5)")
    for s, tick in enumerate(h1.ticks):
        assert np.array_equal(bits(h1.kinetic[s]), bits(want[tick][0])), f"every=1, kinetic of sample {s}"
        assert np.array_equal(bits(h1.potential[s]), bits(want[tick][1])), f"every=1, potential of sample {s}"
    # a sampled and an unsampled tick leave the same state behind: the energies against the oracle once more
    pos, vel, mass = e.positions.numpy(), e.velocities.numpy(), e.masses.numpy()
    for b in range(B):
        ke_ref, pe_ref = oracle_energies(pos[b], vel[b], mass[b], case[2], G_[b], SOFT[b], DT[b])
        close_to(h1.kinetic[-1, b], ke_ref, TOL[case[2]], f"member {b} last sample kinetic vs oracle")
        close_to(h1.potential[-1, b], pe_ref, TOL[case[2]], f"member {b} last sample potential vs oracle")
    e.close()


# ---- 5. a NaN member ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(257, 3, "float64"), (513, 2, "float32")], ids=["n257-d3-float64", "n513-d2-float32"])
def test_a_nan_member_leaves_the_other_histories_alone(nb, case):
    bad = 2
    others = [b for b in range(B) if b != bad]
    good = make_ens(nb, case)
    good.run(1)
    hg = good.run_recorded(4, every=2)
    good.close()
    p = members(case)[0].copy()
    p[bad, 0, 0] = np.nan
    e = make_ens(nb, case, pos=p)
    e.run(1)                       # every star of the member has met the NaN: its velocities are NaN from here on
    h = e.run_recorded(4, every=2)
    assert h.ticks == hg.ticks == [1, 3, 5]
    assert torch.isnan(h.kinetic[:, bad]).all() and torch.isnan(h.potential[:, bad]).all() and torch.isnan(h.total[:, bad]).all()
    assert np.array_equal(bits(h.kinetic[:, others]), bits(hg.kinetic[:, others]))
    assert np.array_equal(bits(h.potential[:, others]), bits(hg.potential[:, others]))
    assert not torch.isnan(hg.kinetic).any() and not torch.isnan(hg.potential).any()
    e.close()


# ---- 6. zero softening --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(257, 3, "float64"), (513, 2, "float32")], ids=["n257-d3-float64", "n513-d2-float32"])
def test_zero_softening_gives_a_nan_potential_like_the_solo_read_out(nb, case):
    zero = 1
    others = [b for b in range(B) if b != zero]
    soft = list(SOFT)
    soft[zero] = 0.0
    p, v, m = members(case)
    mk = lambda s: nb.GalaxyEnsemble(T(p), T(v), T(m), precision_mode=nb.PrecisionMode(case[2]), G=G_, softening=s, dt=DT)
    ref = mk(SOFT)
    kr, pr = ref.energies()
    ref.close()
    e = mk(soft)
    ke, pe = e.energies()
    pe_solo = e.get_potential_energy()
    assert np.isnan(pe_solo[zero]) and not any(np.isnan(pe_solo[b]) for b in others)
    assert np.array_equal(np.isnan(pe.cpu().numpy()), np.isnan(np.array(pe_solo)))
    assert torch.isfinite(ke).all()
    assert np.array_equal(bits(ke), bits(kr))                      # the kinetic energy does not see the softening
    assert np.array_equal(bits(pe[others]), bits(pr[others]))
    h = e.run_recorded(0, every=3)                                 # no tick: only the sample at entry
    assert h.ticks == [0] and e.tick == 0 and tuple(h.potential.shape) == (1, B)
    assert torch.isnan(h.potential[0, zero]) and np.array_equal(bits(h.potential[0, others]), bits(pr[others]))
    assert np.array_equal(bits(h.kinetic[0]), bits(kr))
    e.close()
