"""Divergence between the members of an ensemble, measured on the device: `divergence()` (the kernel alone) against torch's
own expressions on the downloaded state, planted extremes, and `run_diverged()` sample by sample against a twin ensemble.

Bars.  The maxima are exact (`==`): one subtraction in the state dtype and a maximum have no rounding freedom.  The mean is
a fixed-order fp64 sum of n * D <= 3075 non-negative terms, within n * D * 2^-53 < 4e-13 relative of any other fp64 order:
1e-12 against numpy's float64 mean of the |differences| formed in the state dtype; for fp32 state also 2e-6 against torch's
own fp32 .mean(), the suite's bar for fp32 sums added in another order.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 4
BASELINES = ([0, 0, 3, 1],          # itself, an earlier member, a later member, an earlier member
             [2, 3, 3, 0])          # later members, itself, an earlier member
SIZES = [1, 37, 255, 256, 257, 1025]          # the 256-thread stride and its neighbours, a multi-pass size
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def state(n, d, dtype, seed, members=B):
    g = torch.Generator().manual_seed(seed)
    p = (torch.randn(members, n, d, generator=g, dtype=torch.float64) * 3).to(dtype)
    v = (torch.randn(members, n, d, generator=g, dtype=torch.float64) * 0.1).to(dtype)
    m = (0.5 + torch.rand(members, n, generator=g, dtype=torch.float64)).to(dtype)
    return p, v, m


def make(nb, kind, p, v, m):
    M = nb.PrecisionMode
    if kind == "float64":
        return nb.GalaxyEnsemble(p, v, m, precision_mode=M.FLOAT64)
    if kind == "float32":
        return nb.GalaxyEnsemble(p, v, m, precision_mode=M.FLOAT32)
    if kind == "mixed":
        return nb.GalaxyEnsemble(p, v, m, precision_mode=[M.FLOAT32, M.FLOAT16, M.BFLOAT16, M.FLOAT16][:p.shape[0]])
    assert kind == "int8"
    return nb.QuantizedEnsemble(p, v, m, precision_mode=M.INT8_SIM)


def expected(pos, vel, baseline):
    """torch's expressions on the downloaded state, member by member: (max |dp|, fp64 mean of the T-typed |dp|, max |dv|,
    torch's own mean in the state dtype)."""
    out = []
    for b, base in enumerate(baseline):
        dp, dv = (pos[b] - pos[base]).abs(), (vel[b] - vel[base]).abs()
        with np.errstate(all="ignore"):
            mean64 = float(dp.numpy().astype(np.float64).mean())
        out.append((float(dp.max().double()), mean64, float(dv.max().double()), float(dp.mean().double())))
    return out


def eq(got, want):
    """`==`, with NaN equal to NaN."""
    return (got != got and want != want) or got == want


def check(e, baseline, what):
    got = e.divergence(baseline)
    pos, vel = e.positions, e.velocities
    assert all(t.dtype == torch.float64 and tuple(t.shape) == (e.num_members,) for t in got), what
    fp32 = pos.dtype == torch.float32
    for b, (mp, mean64, mv, mean_t) in enumerate(expected(pos, vel, baseline)):
        g_mp, g_mean, g_mv = (float(t[b]) for t in got)
        print(f"{what} member {b} vs {baseline[b]}: max_pos {g_mp:.9g} mean {g_mean:.17g} (numpy {mean64:.17g}) max_vel {g_mv:.9g}")
        assert eq(g_mp, mp), (what, b, g_mp, mp)
        assert eq(g_mv, mv), (what, b, g_mv, mv)
        if mean64 != mean64 or mean64 in (0.0, INF):
            assert eq(g_mean, mean64), (what, b, g_mean, mean64)
        else:
            assert abs(g_mean - mean64) <= 1e-12 * mean64, (what, b, g_mean, mean64)
            if fp32:
                assert abs(g_mean - mean_t) <= 2e-6 * mean64, (what, b, g_mean, mean_t)
    return got


# ---- the kernel alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["float64", "float32"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_divergence_equals_torch_on_the_downloaded_state(nb, n, d, kind):
    p, v, m = state(n, d, torch.float64 if kind == "float64" else torch.float32, 100 * n + d)
    e = make(nb, kind, p, v, m)
    launches = e.launches()
    for baseline in BASELINES:
        check(e, baseline, f"{kind} n{n} d{d} {baseline}")
    for member in (0, B - 1):                           # an int: one member for all
        check(e, [member] * B, f"{kind} n{n} d{d} all against {member}")
        assert all(torch.equal(a, b) for a, b in zip(e.divergence(member), e.divergence([member] * B)))
    assert e.launches() == launches and torch.equal(e.positions, p) and torch.equal(e.velocities, v)
    e.close()


@pytest.mark.parametrize("kind,n,d", [("mixed", 257, 3), ("int8", 255, 2)])
def test_divergence_on_a_mixed_and_on_a_quantized_ensemble(nb, kind, n, d):
    e = make(nb, kind, *state(n, d, torch.float32, 7 + n))
    e.run(2)                                             # a state the ensemble made itself
    for baseline in BASELINES:
        check(e, baseline, f"{kind} {baseline}")
    e.close()


@pytest.mark.parametrize("kind", ["float64", "float32"])
@pytest.mark.parametrize("d", [2, 3])
def test_planted_extremes(nb, kind, d):
    n = 257
    dtype = torch.float64 if kind == "float64" else torch.float32
    p, v, m = state(n, d, dtype, 40 + d)
    e = make(nb, kind, p, v, m)
    baseline = BASELINES[0]

    def put(edit):
        q, w = p.clone(), v.clone()
        edit(q, w)
        e.set_state(positions=q, velocities=w)
        return check(e, baseline, f"{kind} d{d}")

    clean = put(lambda q, w: None)
    assert [float(t[0]) for t in clean] == [0.0, 0.0, 0.0]          # against itself: exact zeros

    def first(q, w):                                    # the largest |d| in the very first element
        q[1, 0, 0] = q[0, 0, 0] + 1000.0
        w[1, 0, 0] = w[0, 0, 0] - 500.0
    got = put(first)
    assert float(got.max_position[1]) == float((p[0, 0, 0] + 1000.0 - p[0, 0, 0]).abs()) and float(got.max_velocity[1]) >= 499.0

    def last(q, w):                                     # ... and in the very last
        q[3, n - 1, d - 1] = q[1, n - 1, d - 1] - 2000.0
        w[3, n - 1, d - 1] = w[1, n - 1, d - 1] + 700.0
    got = put(last)
    assert float(got.max_position[3]) >= 1999.0 and float(got.max_velocity[3]) >= 699.0

    def zeros(q, w):                                    # -0.0 against +0.0 is 0: member 3 is member 1 up to the sign of a zero
        q[3], w[3] = q[1], w[1]
        q[1, 5, 0], q[3, 5, 0], w[1, 9, 1], w[3, 9, 1] = 0.0, -0.0, -0.0, 0.0
    got = put(zeros)
    assert [float(t[3]) for t in got] == [0.0, 0.0, 0.0]

    def nan(q, w):                                      # a NaN in one star of member 0: members 0 (itself) and 1 (against 0)
        q[0, n // 2, d - 1] = NAN
    got = put(nan)
    for b in (0, 1):
        assert np.isnan(float(got.max_position[b])) and np.isnan(float(got.mean_position[b]))
        assert float(got.max_velocity[b]) == float(clean.max_velocity[b])          # the velocities hold no NaN
    for b in (2, 3):
        assert all(float(g[b]) == float(c[b]) for g, c in zip(got, clean))

    def nan_vel(q, w):
        w[1, 0, 0] = NAN
    got = put(nan_vel)
    assert np.isnan(float(got.max_velocity[1])) and np.isnan(float(got.max_velocity[3]))
    assert float(got.max_position[1]) == float(clean.max_position[1]) and float(got.mean_position[3]) == float(clean.mean_position[3])

    def inf_inf(q, w):                                  # +inf against +inf: NaN
        q[0, 3, 0] = q[1, 3, 0] = INF
    got = put(inf_inf)
    assert np.isnan(float(got.max_position[1])) and np.isnan(float(got.mean_position[1])) and np.isnan(float(got.max_position[0]))

    def inf_finite(q, w):                               # +inf against a finite value: +inf, an ordinary value
        q[1, n - 1, 0] = INF
        w[3, 0, d - 1] = -INF
    got = put(inf_finite)
    assert float(got.max_position[1]) == INF and float(got.mean_position[1]) == INF
    assert float(got.max_position[3]) == INF and float(got.mean_position[3]) == INF and float(got.max_velocity[3]) == INF
    assert float(got.max_position[0]) == 0.0 and float(got.max_velocity[1]) == float(clean.max_velocity[1])
    e.close()


def test_divergence_refuses_what_names_no_member(nb):
    import ctypes as C
    from nbody_cosmological_simulation_amd import _native as N
    e = make(nb, "float32", *state(37, 2, torch.float32, 5))
    with pytest.raises(ValueError, match="baseline must name a member"):
        e.divergence(B)
    out = (C.c_double * B)()
    rc = N.lib().nb_ens_divergence(e._handle, (C.c_int32 * B)(0, 1, B, 0), out, out, out, 0)
    assert rc != 0 and "baseline[2]" in N.last_error()
    rc = N.lib().nb_ens_run_diverged(e._handle, 2, 1, (C.c_int32 * B)(0, -1, 0, 0), 0, out, out, out, None, None, 3, 0, None)
    assert rc != 0 and "baseline[1]" in N.last_error()
    assert e.launches() == 1
    e.close()


# ---- run_diverged ----------------------------------------------------------------------------------------------------------
MODES = ["float32", "bfloat16", "float16", "float32", "float16"]
TICKS = 6
TWIN = 3                               # the FLOAT32 member that starts 2^-10 away from member 0 in one coordinate


def galaxy(nb, n, d):
    """One galaxy under five modes: every member starts from the same state (member TWIN nudged), same G, softening, dt."""
    p, v, m = state(n, d, torch.float32, 900 + n, members=1)
    p, v, m = p.repeat(5, 1, 1), v.repeat(5, 1, 1), m.repeat(5, 1)
    p[TWIN, n // 3, 1] += 2.0 ** -10       # (1e-10, the reference's nudge, is below an fp32 ulp here: a no-op)
    assert p[TWIN, n // 3, 1] != p[0, n // 3, 1]
    return p, v, m


def ensemble(nb, n, d):
    return nb.GalaxyEnsemble(*galaxy(nb, n, d), precision_mode=[nb.PrecisionMode(x) for x in MODES], G=0.001, softening=0.1,
                             dt=0.01)


@pytest.mark.parametrize("every", [1, 2, 4])
@pytest.mark.parametrize("n,d", [(257, 3), (1025, 2)])
def test_run_diverged_sample_by_sample(nb, n, d, every):
    baseline = 0 if every != 4 else [3, 0, 0, 3, 0]
    bl = [baseline] * 5 if isinstance(baseline, int) else baseline
    S = 1 + TICKS // every
    e = ensemble(nb, n, d)
    e.run(1)
    launches = e.launches()
    h = e.run_diverged(TICKS, every=every, baseline=baseline, energies=True)
    assert e.launches() - launches == TICKS and e.tick == 1 + TICKS
    assert h.ticks == [1 + s * every for s in range(S)] and h.baseline == bl
    assert all(tuple(t.shape) == (S, 5) and t.dtype == torch.float64 for t in (h.max_position, h.mean_position, h.max_velocity))

    # sample s is divergence() of a twin after run(s * every); sample 0 is the state at entry
    twin = ensemble(nb, n, d)
    twin.run(1)
    for s in range(S):
        if s:
            twin.run(every)
        want = twin.divergence(baseline)
        for name, got_t, want_t in zip(("max_position", "mean_position", "max_velocity"), h[2:5], want):
            assert torch.equal(got_t[s], want_t), (name, s, got_t[s], want_t)
    twin.run(TICKS - (S - 1) * every)
    for name in ("positions", "velocities", "accelerations"):       # the final state is run(6)'s
        assert torch.equal(getattr(e, name), getattr(twin, name)), name
    twin.close()

    # the hooks show from the first tick on; the nudged twin from the entry sample on
    mp = h.max_position.numpy()
    print(f"n{n} d{d} every {every}: max_position\n{mp}")
    for b in range(5):
        if MODES[b] != MODES[bl[b]]:
            assert (mp[1:, b] > 0).all(), (b, mp[:, b])
    if baseline == 0:
        assert (mp[:, 0] == 0).all() and (mp[:, TWIN] >= 2.0 ** -11).all()
        assert h.butterfly(2.0 ** -12)[TWIN] and not h.butterfly(2.0 ** -12)[0]
        assert (h.peak()[-1] >= mp[-1]).all() and (h.entropy_bits()[1:, [1, 2, 4]] > 0).all()

    # energies=True is run_recorded's history, bit for bit; energies=False records none; two calls give the same history
    r = ensemble(nb, n, d)
    r.run(1)
    hr = r.run_recorded(TICKS, every)
    assert h.energy.ticks == hr.ticks and torch.equal(h.energy.kinetic, hr.kinetic) and torch.equal(h.energy.potential, hr.potential)
    r.close()
    again = ensemble(nb, n, d)
    again.run(1)
    h2 = again.run_diverged(TICKS, every=every, baseline=baseline, energies=False)
    assert h2.energy is None
    for a, b in zip(h[2:5], h2[2:5]):
        assert torch.equal(a, b)
    for name in ("positions", "velocities", "accelerations"):
        assert torch.equal(getattr(e, name), getattr(again, name)), name
    again.close()
    e.close()


def test_run_diverged_edges(nb):
    import ctypes as C
    from nbody_cosmological_simulation_amd import _native as N
    e = ensemble(nb, 257, 3)
    launches = e.launches()
    h = e.run_diverged(0)                                # no ticks: the entry sample alone
    assert h.ticks == [0] and tuple(h.max_position.shape) == (1, 5) and e.launches() == launches and e.tick == 0
    assert all(torch.equal(a[0], b) for a, b in zip(h[2:5], e.divergence(0)))
    h = e.run_diverged(3, every=5)                       # fewer ticks than the interval: still three ticks taken
    assert h.ticks == [0] and e.tick == 3 and e.launches() == launches + 3
    # a history over the 256 MiB cap is an error before any launch, and so is too small a capacity on the native side
    with pytest.raises(ValueError, match="above the limit"):
        e.run_diverged(3_000_000, every=1)
    out = (C.c_double * 10)()
    got = C.c_int32(-1)
    rc = N.lib().nb_ens_run_diverged(e._handle, 4, 1, (C.c_int32 * 5)(), 0, out, out, out, None, None, 2, 0, C.byref(got))
    assert rc != 0 and "capacity" in N.last_error() and got.value == 0
    for bad in (dict(every=0), dict(baseline=5), dict(baseline=[0, 0, 0])):
        with pytest.raises(ValueError):
            e.run_diverged(2, **bad)
    assert e.tick == 3 and e.launches() == launches + 3
    e.close()


def test_run_diverged_on_float64_and_quantized_ensembles(nb):
    for kind, dtype in (("float64", torch.float64), ("int8", torch.float32)):
        p, v, m = state(255, 2, dtype, 77)
        e, twin = make(nb, kind, p, v, m), make(nb, kind, p, v, m)
        h = e.run_diverged(4, every=2, baseline=BASELINES[1], energies=False)
        for s in range(3):
            if s:
                twin.run(2)
            for got_t, want_t in zip(h[2:5], twin.divergence(BASELINES[1])):
                assert torch.equal(got_t[s], want_t), (kind, s)
        assert torch.equal(e.positions, twin.positions) and torch.equal(e.velocities, twin.velocities)
        e.close()
        twin.close()
