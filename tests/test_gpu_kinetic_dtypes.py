"""Kinetic energy term by term: all 16 (velocities, masses) dtype pairs x 2-D / 3-D x fp32 / fp64 storage.

kinetic_kernel (nb_misc.hip) types the product m * |v|^2 like torch does, promote(velocities, masses): an fp64 product of
the unrounded mass beside fp64 masses, a half-rounded product only when the masses are typed like the half velocities,
an fp32 product otherwise.  The dense sums of the parity tests sit at 2e-6 and cannot see a product rounded in the wrong
type (6e-8 for an fp32-rounded mass), so every pair gets
  probes   all masses 0 but one -- at index 0, on both sides of a 256 boundary, at the last particle of a ragged N and
           (BIG_CASES) on both sides of the 1024-block cap of nb_launch_kinetic at N > 262 144.  One term, and the zeros
           add exactly: get_kinetic_energy() must EQUAL the oracle's value (nbo_kinetic_energy, which
           tests/test_oracle_golden.py pins against torch term by term);
  dense    random masses against the oracle at the project's bars: 1e-12 where the result type is fp64, 2e-6 where it is
           fp32, one ulp of the half type (2^-10 / 2^-7) where it is a half type; got == want also passes (a float16
           sum that overflows on both sides);
and both again after one step(), when the velocities' logical dtype has been promoted.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = 0, 1, 2, 3
TORCH_DT = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32, torch.float64: F64}
DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64]
NAME = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64"}
DENSE_TOL = {F64: 1e-12, F32: 2e-6, F16: 2.0 ** -10, BF16: 2.0 ** -7}

# (velocities, masses, dim, mode): FLOAT64 mode puts a pair without an fp64 tensor on fp64 storage as well
CASES = [(v, m, d, mode) for v in DTYPES for m in DTYPES for d in (2, 3)
         for mode in (("float64",) if torch.float64 in (v, m) else ("float32", "float64"))]
# past the 1024-block cap of the launch (1024 x 256 = 262 144 particles): the loop of every block wraps
# one case per kinetic_kernel instantiation (<float | double, fp32-typed | fp64 velocities, none | f16 | bf16>)
BIG_CASES = [(torch.float32, torch.float32, 3, "float32"), (torch.float64, torch.float64, 2, "float64"),
             (torch.float16, torch.float16, 2, "float32"), (torch.float32, torch.float64, 3, "float64"),
             (torch.bfloat16, torch.bfloat16, 3, "float32"), (torch.float16, torch.float64, 3, "float64"),
             (torch.bfloat16, torch.float32, 2, "float64")]
BIG_N = 262144 + 777


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


def promote(a, b):
    return a if a == b else (F64 if F64 in (a, b) else F32)


def oracle_ke(vel, mass):
    from oracle import oracle as O
    v = np.ascontiguousarray(vel.detach().cpu().double().numpy())
    m = np.ascontiguousarray(mass.detach().cpu().double().numpy())
    return O.lib().nbo_kinetic_energy(v.shape[0], v.shape[1], TORCH_DT[vel.dtype], O._dp(v), TORCH_DT[mass.dtype], O._dp(m))


def check(nb, v_t, m_t, dim, mode, n, places):
    rng = np.random.default_rng(n + dim + 7 * TORCH_DT[v_t] + 29 * TORCH_DT[m_t])
    pos = torch.from_numpy(rng.standard_normal((n, dim)) * 2.0).to(v_t)
    vel = torch.from_numpy(rng.standard_normal((n, dim)) * 0.3).to(v_t)
    dense = torch.from_numpy(0.5 + rng.random(n)).to(m_t)
    sim = nb.GalaxySimulation(pos, vel, dense, precision_mode=nb.PrecisionMode(mode))
    tag = f"v={NAME[v_t]} m={NAME[m_t]} d={dim} {mode} N={n}"
    try:
        for phase in ("tick0", "after step"):
            if phase == "after step":
                sim.masses = dense
                sim.step()
            V = sim.velocities
            T = promote(TORCH_DT[V.dtype], TORCH_DT[m_t])
            for k in places:
                m = np.zeros(n)
                m[k] = 0.5 + rng.random()
                mt = torch.from_numpy(m).to(m_t)
                sim.masses = mt
                got, want = sim.get_kinetic_energy(), oracle_ke(V, mt)
                assert want != 0.0 and np.isfinite(want), (tag, phase, k, want)
                assert got == want, f"{tag} {phase}: one-term kinetic energy at particle {k}: {got!r} != oracle {want!r} (relative {abs(got - want) / abs(want):.2e})"
            sim.masses = dense
            got, want = sim.get_kinetic_energy(), oracle_ke(V, dense)
            assert got == want or abs(got - want) <= DENSE_TOL[T] * abs(want), (tag, phase, "dense", got, want)
    finally:
        sim.close()


@pytest.mark.parametrize("v_t,m_t,dim,mode", CASES, ids=[f"v{NAME[c[0]]}-m{NAME[c[1]]}-d{c[2]}-{c[3]}" for c in CASES])
def test_kinetic_energy_dtype_pair(nb, v_t, m_t, dim, mode):
    n = 1000 + 37 * TORCH_DT[v_t] + 5 * TORCH_DT[m_t] + dim          # ragged: N % 256 != 0
    check(nb, v_t, m_t, dim, mode, n, (0, 255, 256, 511, 512, n - 1))


@pytest.mark.parametrize("v_t,m_t,dim,mode", BIG_CASES, ids=[f"v{NAME[c[0]]}-m{NAME[c[1]]}-d{c[2]}-{c[3]}" for c in BIG_CASES])
def test_kinetic_energy_past_the_block_cap(nb, v_t, m_t, dim, mode):
    check(nb, v_t, m_t, dim, mode, BIG_N, (0, 262143, 262144, 262144 + 255, 262144 + 256, BIG_N - 1))
