"""The pruned and the tracked max-r2 search (nb_grid.hip) on clouds that are tight against the softening, and on
non-finite input.

The grid modes need the fp32 maximum of r2 = (dx*dx + dy*dy [+ dz*dz]) + eps2 over all pairs.  Above N = 3072 (fp32
state) it comes from two pruning searches: the pruned one on the first evaluation, the tracked one on every later
evaluation.  Both must return the very fp32 number an all-pairs scan returns.

Oracle: the fp32 all-pairs maximum in torch on the CPU, separate multiply and add, the reference's operation order
(`_exact_r2max_f32`, as in test_gpu_parity.py).  Both sides evaluate the same fp32 expression, so the bar is equality
(NaN equals NaN: torch's max() propagates it, and so must the searches).  eps2 is the fp32 rounding of the Python
float `softening ** 2`: that is what the reference adds to its fp32 tensor (simulation.py: softening_sq is a Python
float) and what the engine is handed.  (Squaring np.float32(0.1) in fp32 gives a different number, one ulp away.)

Every case is also run on a second handle created under NB_NO_PRUNE (all-pairs scan at every evaluation): r2max, lmax
and the positions must agree bit for bit at every step.

N = 3100: the smallest convenient size above the 3072 threshold.  G = 1e-5 keeps a cloud of 3100 unit masses near
static over the five steps (it shrinks by 4 % at softening 0.1, by 4e-5 at softening 1), so the bound on rho the tracked
search assumes settles at its steady 1e-4 margin by the fourth evaluation instead of being overrun by a collapse.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3100
G = 1e-5
STEPS = 5


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


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


def _eps2(soft):
    return np.float32(float(soft) ** 2)


def _same(a, b):
    """Equality of two floats where NaN equals NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(a, b, equal_nan=True))


# ----------------------------------------------------------------------------------------------- clouds
@functools.lru_cache(maxsize=None)
def _unit_cloud(name, d):
    """(N, d) float64 cloud of radius ~1 about the origin, fixed seed."""
    rng = np.random.default_rng(1000 * d + sorted(CLOUDS).index(name))
    x = np.zeros((N, d))
    if name == "ring":
        a = 2.0 * np.pi * np.arange(N) / N
        x[:, 0], x[:, 1] = np.cos(a), np.sin(a)
    elif name == "line":
        x[:, 0] = np.linspace(-1.0, 1.0, N)
    elif name == "ball":
        v = rng.standard_normal((N, d))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        x = v * rng.random((N, 1)) ** (1.0 / d)
    elif name == "gauss":
        x = rng.standard_normal((N, d))
    elif name == "two":
        x = rng.standard_normal((N, d)) * 0.05
        x[: N // 2] += 1.0
        x[N // 2:] -= 1.0
    elif name == "lattice":
        # 56 x 56 integer grid, 36 interior points taken out so that all four corners stay: both diagonals tie
        ij = np.array([(i, j) for i in range(56) for j in range(56) if not (i == 28 and 10 <= j < 46)], np.float64)
        assert ij.shape[0] == N
        x[:, :2] = (ij - 27.5) / (27.5 * np.sqrt(2.0))
    elif name == "dup":
        x = _unit_cloud("gauss", d).copy()
        p = torch.from_numpy(x)
        flat = int(torch.cdist(p, p).argmax())
        a, b = divmod(flat, N)
        others = [i for i in range(N) if i not in (a, b)]
        x[others[:10]] = x[a]
        x[others[10:20]] = x[b]
    else:
        raise KeyError(name)
    x.setflags(write=False)
    return x


CLOUDS = ("ring", "line", "ball", "gauss", "two", "lattice", "dup")


def _positions(name, d, radius, offset):
    return (_unit_cloud(name, d) * radius + offset).astype(np.float32)


def _cases():
    """(cloud, ratio, soft, d, offset).  Ratio 1e-3 -- where the softening dwarfs the cloud -- in full: every cloud at
    both softenings in both dimensions, plus the offset clouds; the two larger ratios with every cloud at two
    (softening, dimension) combinations that alternate from cloud to cloud."""
    out = []
    for name in CLOUDS:
        for soft in (0.1, 1.0):
            for d in (2, 3):
                out.append((name, 1e-3, soft, d, 0.0))
    for d in (2, 3):
        out.append(("two", 1e-3, 1.0, d, 1000.0))
    out.append(("gauss", 1e-3, 1.0, 2, 1000.0))
    out.append(("gauss", 1e-3, 0.1, 3, 1000.0))
    for ratio in (1e-2, 1.0):
        for i, name in enumerate(CLOUDS):
            out.append((name, ratio, 0.1, 2 + i % 2, 0.0))
            out.append((name, ratio, 1.0, 3 - i % 2, 0.0))
    out.append(("two", 1.0, 1.0, 2, 1000.0))
    return out


CASES = _cases()
# the first evaluation of these is also held against the CPU oracle's lmax
ORACLE_CASES = {("ring", 1e-3, 0.1, 2, 0.0), ("ball", 1e-3, 1.0, 3, 0.0), ("two", 1e-3, 1.0, 2, 1000.0)}


def _make(nb, monkeypatch, pos, mode, soft, no_prune, levels=None):
    if no_prune:
        monkeypatch.setenv("NB_NO_PRUNE", "1")          # read when the handle is created
    else:
        monkeypatch.delenv("NB_NO_PRUNE", raising=False)
    n, d = pos.shape
    sim = nb.GalaxySimulation(T(pos), torch.zeros(n, d), torch.ones(n), precision_mode=nb.PrecisionMode(mode), G=G,
                              softening=soft, custom_levels=levels)
    monkeypatch.delenv("NB_NO_PRUNE", raising=False)
    assert sim.force_kernel_name() != "small_step_kernel"
    return sim


def _read(sim):
    dbg = sim.quant_debug()
    return np.float32(dbg["r2max"]), np.float64(dbg["lmax"]), sim.positions.numpy().copy()


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: "{}-r{:g}-s{:g}-d{}-o{:g}".format(*CASES[i]))
def test_max_r2_searches_on_tight_clouds(nb, monkeypatch, case):
    """First evaluation (pruned search) and five steps (tracked search): r2max equals the host's fp32 all-pairs
    maximum at every read, and r2max, lmax and the trajectory are those of the all-pairs handle bit for bit."""
    name, ratio, soft, d, offset = CASES[case]
    mode = "int4_sim" if case % 3 == 2 else "custom"
    pos = _positions(name, d, ratio * soft, offset)
    eps2 = _eps2(soft)
    sim = _make(nb, monkeypatch, pos, mode, soft, no_prune=False)
    ref = _make(nb, monkeypatch, pos, mode, soft, no_prune=True)
    for read in range(STEPS + 1):
        if read:
            sim.run(1)
            ref.run(1)
        r_s, l_s, x_s = _read(sim)
        r_r, l_r, x_r = _read(ref)
        want = _exact_r2max_f32(x_r, eps2)
        print(f"read {read}: searched {r_s!r} all-pairs {r_r!r} host {want!r} lmax {l_s!r} / {l_r!r}")
        assert _same(r_r, want), (read, r_r, want)              # the all-pairs scan itself
        assert _same(r_s, want), (read, r_s, want)
        assert _same(l_s, l_r), (read, l_s, l_r)
        assert np.array_equal(x_s.view(np.uint32), x_r.view(np.uint32)), f"read {read}: the search changed the trajectory"
        if read == 0 and CASES[case] in ORACLE_CASES:
            from oracle import oracle as O
            _, dbg = O.accelerations(pos, np.ones(N, np.float32), mode, G=G, softening=soft, debug=True)
            assert np.float32(l_s) == np.float32(dbg["lmax"]), (l_s, dbg["lmax"])


@pytest.mark.parametrize("d", [2, 3])
def test_tracked_search_hands_its_maximum_to_multi_block_tables(nb, monkeypatch, d):
    """A grid of 1000 levels is more than one workgroup of tables: the tracked scan's last workgroup stores the maximum
    and the tables kernel follows with its arrival count, instead of the scan building the tables itself.  First
    evaluation and three steps of the gauss cloud at radius 4: r2max equals the host's fp32 all-pairs maximum at every
    read, and r2max, lmax and the trajectory are those of the all-pairs handle bit for bit."""
    soft = 0.1
    pos = _positions("gauss", d, 4.0, 0.0)
    eps2 = _eps2(soft)
    sim = _make(nb, monkeypatch, pos, nb.PrecisionMode.CUSTOM, soft, no_prune=False, levels=1000)
    ref = _make(nb, monkeypatch, pos, nb.PrecisionMode.CUSTOM, soft, no_prune=True, levels=1000)
    for read in range(4):
        if read:
            sim.run(1)
            ref.run(1)
        r_s, l_s, x_s = _read(sim)
        r_r, l_r, x_r = _read(ref)
        want = _exact_r2max_f32(x_r, eps2)
        print(f"read {read}: searched {r_s!r} all-pairs {r_r!r} host {want!r} lmax {l_s!r} / {l_r!r}")
        assert _same(r_s, want), (read, r_s, want)
        assert _same(r_s, r_r), (read, r_s, r_r)
        assert _same(l_s, l_r), (read, l_s, l_r)
        assert np.array_equal(x_s.view(np.uint32), x_r.view(np.uint32)), f"read {read}: the search changed the trajectory"


# ----------------------------------------------------------------------------------------------- non-finite bounds
def _bad_positions(kind, d):
    pos = (_unit_cloud("gauss", d) * 4.0).astype(np.float32)
    if kind == "posinf":
        pos[5, 0] = np.inf
    elif kind == "neginf":
        pos[5, d - 1] = -np.inf
    elif kind == "overflow":
        pos = (pos * np.float32(1e20)).astype(np.float32)     # finite coordinates, r2 overflows
        assert np.isfinite(pos).all()
    return pos


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", ["posinf", "neginf", "overflow"])
def test_max_r2_searches_on_non_finite_bounds(nb, monkeypatch, kind, d):
    """An infinite coordinate puts inf - inf = NaN on the diagonal of the reference's r2 matrix: r2max is NaN and every
    acceleration NaN.  A finite cloud scaled by 1e20 overflows r2: the maximum is +inf.  Pruned search (bad positions at
    construction), tracked search on the same bad positions (assigned after a clean start, forces evaluated twice:
    the first evaluation seeds, the second tracks), then one step; each against the host maximum and the all-pairs
    handle."""
    soft = 0.1
    eps2 = _eps2(soft)
    bad = _bad_positions(kind, d)
    want = _exact_r2max_f32(bad, eps2)
    assert np.isnan(want) if kind != "overflow" else want == np.float32(np.inf)

    # pruned search
    sim = _make(nb, monkeypatch, bad, "custom", soft, no_prune=False)
    ref = _make(nb, monkeypatch, bad, "custom", soft, no_prune=True)
    r_s, l_s, _ = _read(sim)
    r_r, l_r, _ = _read(ref)
    print(f"{kind} pruned: searched {r_s!r} all-pairs {r_r!r} host {want!r}")
    assert _same(r_r, want) and _same(r_s, want), (r_s, r_r, want)
    assert _same(l_s, l_r)
    a_s, a_r = sim.accelerations.numpy(), ref.accelerations.numpy()
    assert np.array_equal(a_s, a_r, equal_nan=True)
    if kind != "overflow":
        assert np.isnan(a_s).all()

    # tracked search
    clean = (_unit_cloud("gauss", d) * 4.0).astype(np.float32)
    sim = _make(nb, monkeypatch, clean, "custom", soft, no_prune=False)
    ref = _make(nb, monkeypatch, clean, "custom", soft, no_prune=True)
    sim.run(1)
    ref.run(1)
    assert _same(_read(sim)[0], _exact_r2max_f32(sim.positions.numpy(), eps2))
    for s in (sim, ref):
        s.positions = T(bad.copy())
    for what in ("seed", "track", "step"):
        for s in (sim, ref):
            if what == "step":
                s.run(1)
            else:
                s.accelerations = s.compute_forces()
        r_s, l_s, x_s = _read(sim)
        r_r, l_r, x_r = _read(ref)
        want = _exact_r2max_f32(x_r, eps2)
        print(f"{kind} {what}: searched {r_s!r} all-pairs {r_r!r} host {want!r}")
        assert _same(r_r, want) and _same(r_s, want), (what, r_s, r_r, want)
        assert _same(l_s, l_r), what
        assert np.array_equal(x_s, x_r, equal_nan=True), what
        a_s, a_r = sim.accelerations.numpy(), ref.accelerations.numpy()
        assert np.array_equal(a_s, a_r, equal_nan=True), what
        if kind != "overflow":
            assert np.isnan(a_s).all(), what
