"""The DPP hand-off of the fp64 pair-symmetric sweep (NB_SYM_ROT=2: source positions from the ring staged in LDS, source
accumulators moved one lane along by v_mov_b32_dpp wave_rol:1 in the VALU) against the lane rotation (NB_SYM_ROT=0:
ds_bpermute_b32).

Only data movement differs -- the same values meet in the same order -- so every output must be bit for bit the same:
accelerations of the first evaluation, and positions, velocities and accelerations after three steps.  Two handles per
case, built in one process from the same seeded state; the knob is read when a handle is created.

Shapes (2-D, R = 4: tiles of 256 particles, super-rows of four tiles) -- the smallest at which the exchange can go wrong:
  N = 256            one tile: the diagonal sweep only, nothing travels
  N = 1000           four tiles, one super-row, padding particles (at 1e150, real lanes of the rotate) in the last tile
  N = 2100           nine tiles: a partial last super-row, waves that skip source tiles below their own
  NB_SYM_SPLIT=3     pieces start 21 and 42 steps into the ring; step counts that are no power of two, so the
                     accumulators are not home when a piece ends
  NB_SYM_CL=1 / 4    one / several source tiles per workgroup: the ring is restaged between the two barriers
  NB_SYM_ROWSPLIT=2  the row-split twins: four waves at different steps of one tile
each with equal masses (mass factor applied to the finished sums) and with distinct masses (mass factors read from a
second ring), plus one case with softening 0 and coincident particles, where the NaNs must match by bit pattern (a DPP
move copies 32-bit words and must not quieten or canonicalise them), and one 3-D case, for which the mode has no
instantiation: NB_SYM_ROT=2 must then run the lane rotation and equal NB_SYM_ROT=0 as well.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

KERNEL = "force_sym_kernel<double"
BASE_ENV = {"NB_SYM": "1", "NB_SYM_R": "4", "NB_NO_SMALLN": "1"}

SHAPES = [
    ("n256", 256, {}),
    ("n1000", 1000, {}),
    ("n2100", 2100, {}),
    ("n2100-split3", 2100, {"NB_SYM_SPLIT": "3"}),
    ("n2100-cl1", 2100, {"NB_SYM_CL": "1"}),
    ("n2100-cl4", 2100, {"NB_SYM_CL": "4"}),
    ("n2100-rowsplit2", 2100, {"NB_SYM_ROWSPLIT": "2"}),
]
# (id, N, dim, knobs, masses, softening)
CASES = [(f"{cid}-{mk}", n, 2, env, mk, 0.1) for cid, n, env in SHAPES for mk in ("equal", "distinct")]
CASES.append(("n1000-eps0-coincident", 1000, 2, {}, "equal", 0.0))
CASES.append(("n1000-3d-no-instantiation", 1000, 3, {}, "distinct", 0.1))


def state(n, dim, masses, coincident):
    g = torch.Generator().manual_seed(2000 + n + dim)
    pos = torch.randn(n, dim, dtype=torch.float64, generator=g) * 3.0
    vel = torch.randn(n, dim, dtype=torch.float64, generator=g) * 0.1
    if masses == "equal":
        mass = torch.full((n,), 1.0 / n, dtype=torch.float64)
    else:
        mass = (0.5 + torch.rand(n, dtype=torch.float64, generator=g)) / n
    if coincident:
        pos[700] = pos[10]      # two tiles apart: the pair is met in an off-diagonal sweep
        pos[30] = pos[20]       # same tile: met in the diagonal sweep
    return pos, vel, mass


def same_bits(a, b, what):
    """torch.equal, and NaNs with the same bits in the same places."""
    assert a.dtype == torch.float64 and a.shape == b.shape, what
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)), what
    if not bool(torch.isnan(a).any()):
        assert torch.equal(a, b), what


@pytest.mark.parametrize("cid,n,dim,env,masses,softening", CASES, ids=[c[0] for c in CASES])
def test_dpp_handoff_equals_lane_rotation(cid, n, dim, env, masses, softening, monkeypatch):
    import nbody_cosmological_simulation_amd as nb

    for k, v in {**BASE_ENV, **env}.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda:0")
    pos, vel, mass = state(n, dim, masses, coincident=(softening == 0.0))
    out = {}
    for rot in ("0", "2"):
        monkeypatch.setenv("NB_SYM_ROT", rot)
        sim = nb.GalaxySimulation(pos.to(dev), vel.to(dev), mass.to(dev), precision_mode=nb.PrecisionMode.FLOAT64,
                                  softening=softening, device=dev)
        acc0 = sim._compute_accelerations().clone()
        assert sim.force_kernel_name() == KERNEL, (cid, rot, sim.force_kernel_name())
        sim.run(3)
        assert sim.force_kernel_name() == KERNEL, (cid, rot, sim.force_kernel_name())
        out[rot] = (acc0.cpu(), sim.positions.cpu().clone(), sim.velocities.cpu().clone(), sim.accelerations.cpu().clone())
        sim.close()
    nan = bool(torch.isnan(out["0"][0]).any())
    assert nan == (softening == 0.0), cid        # softening 0: the self pairs' 0 * inf; otherwise every sum is finite
    for name, a, b in zip(("first accelerations", "positions", "velocities", "accelerations"), out["0"], out["2"]):
        same_bits(a, b, f"{cid}: {name} after {'run(3)' if name != 'first accelerations' else 'compute_accelerations'}")
