"""The leapfrog recurrence of every single-GPU kick site, bit for bit (cases: CASES and OVERRIDE_CASES below).

The update v += a dt/2; x += v dt (simulation.py:132-141) is fused into about ten launches (include/nbody_amd.h,
nb_step_path_name).  It is elementwise with two rounded operations per line, so given the accelerations the engine
itself reports, the state after a step is determined bit for bit:

    v_half = axpy(v_prev, a_prev, dt/2)      x_new = axpy(x_prev, v_half, dt)      v_new = axpy(v_half, a_new, dt/2)

with axpy the oracle's nbo_axpy in the logical dtype codes (pinned against torch by tests/test_oracle_golden.py).  No
tolerance and no force oracle: a kick with the wrong rounding, a stale scalar, a skipped tail element or a transposed
repack fails np.array_equal.  Every case
  * asserts step_path_name() against plan_shapes.step_path() after every call, so a retune that moves the case to
    another site fails (tests/test_distributed_cpu.py checks that every site the mirror can emit has a case here);
  * runs a step() loop of five steps with the state read after every step, with speculation on and with NB_NO_SPEC;
  * writes dt, then the velocities, between steps: the next step must use the new values, not a speculative drift;
  * asserts that two run(k) calls agree bit for bit, and that run(k) equals the verified step loop (k = 2, 5): the
    interior sites (kick mode 2) fall under the same contract;
  * on the pair-symmetric path rebuilds a simulation from a downloaded state and compares its accelerations with the
    ones the step computed from the repacked positions;
  * checks its own inputs: v_half != v_prev for > 99 % of the elements and an FMA evaluation of the kick differs from
    the two-rounding one in >= 1 % of them (otherwise the case could not tell the two apart).
The multi-rank sites -- the kicks inside the direct all-reduce (p2p:1, p2p:2), the INT8 exchange of fp64 sums with its
finish launch, and the closing kick deferred into the next pack launch (pack:2) -- need a communicator:
tests/tools/multirank_worker.py records a step() loop and run(k) on rank 0 and check_multirank_trace() below asserts the
same recurrence on them inside test_gpu_parity.test_multi_rank_product_path_on_one_gpu.  The kick modes of
nb_launch_finish_sums64 and of the fp64-exchange all-reduce are never selected (they need a force-quantising mode, whose
kicks always ride in the finish launch), so there is no "sums64:*" or "p2p:*,x64" site to test.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

import plan_shapes as S

pytestmark = pytest.mark.gpu

MODE_CODES = {"float64": 0, "float32": 1, "bfloat16": 2, "float16": 3, "int8_sim": 4, "int4_sim": 5, "custom": 6}
F16, BF16, F32, F64 = S.DT_F16, S.DT_BF16, S.DT_F32, S.DT_F64
TORCH_DT = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32, torch.float64: F64}
H, B, S32, D64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
# dtype chains (positions, velocities, masses), as tests/test_gpu_energy_shapes.CHAINS names them
CHAINS = {"f64": (D64, D64, D64), "f32": (S32, S32, S32), "h16": (H, H, H), "b16": (B, B, B), "m64": (S32, S32, D64),
          "v64": (S32, D64, S32), "h16-v64": (H, D64, H), "b16-v64": (B, D64, B), "h16-m32": (H, H, S32)}
G, DT0, DT1 = 0.02, 0.01, 0.0123          # dt values that are not fp32 numbers: a scalar cast at the wrong width shows
NSTEPS = 5

NS = {"NB_NO_SMALLN": "1"}
# (id, N, dim, chain, mode, custom levels, knobs, check the repack against a rebuilt simulation)
CASES = [
    # ---- small-system kernel: fp64 / fp32, 2-D / 3-D, each lane count; grid modes; INT8 / INT4 through fq_finish
    ("small-f64-d2", 700, 2, "f64", "float64", 0, {}, False),
    ("small-f64-d3", 1500, 3, "f64", "float64", 0, {}, False),
    ("small-f32-d2", 1000, 2, "f32", "float32", 0, {}, False),
    ("small-f32-d3", 2999, 3, "f32", "float32", 0, {}, False),
    ("small-f16-d2", 1300, 2, "f32", "float16", 0, {}, False),
    ("small-f64-lanes16", 900, 3, "f64", "float64", 0, {"NB_SMALL_LANES": "16"}, False),
    ("small-f32-lanes32", 900, 2, "f32", "float32", 0, {"NB_SMALL_LANES": "32"}, False),
    ("small-f64-lanes64", 1100, 2, "f64", "float64", 0, {"NB_SMALL_LANES": "64"}, False),
    ("small-int8-d2", 1000, 2, "f32", "int8_sim", 0, {}, False),
    ("small-int4-d3", 2500, 3, "f32", "int4_sim", 0, {}, False),
    ("small-custom-d2", 1000, 2, "f32", "custom", 0, {}, False),
    # ---- pair-symmetric path: R = 1 / 2 / 4, row-split, tail plan; grid modes with and without red_mm
    ("sym-f64-r1", 2000, 2, "f64", "float64", 0, NS, True),
    ("sym-f64-r2", 3000, 2, "f64", "float64", 0, {"NB_SYM": "1", "NB_SYM_R": "2", **NS}, True),
    ("sym-f64-rowsplit", 5200, 2, "f64", "float64", 0, {}, True),
    ("sym-f64-classic-d3", 8200, 3, "f64", "float64", 0, {}, True),
    ("sym-f64-tail8", 23800, 2, "f64", "float64", 0, {}, True),
    ("sym-f32-r2-d3", 4100, 3, "f32", "float32", 0, {}, True),
    ("sym-f32-r2-tail2", 11500, 2, "f32", "float32", 0, {}, True),
    ("sym-f32-r4", 21100, 2, "f32", "float32", 0, {}, True),
    ("sym-bf16-r2", 7100, 3, "f32", "bfloat16", 0, {}, True),
    ("sym-int8-redmm", 4000, 2, "f32", "int8_sim", 0, {}, True),
    ("sym-int4-redmm-d3", 7100, 3, "f32", "int4_sim", 0, {}, True),
    ("sym-int8-no-redmm", 4000, 2, "f32", "int8_sim", 0, {"NB_NO_RED_MM": "1"}, True),
    ("sym-int8-above-redmm", 65600, 2, "f32", "int8_sim", 0, {}, True),
    ("sym-custom", 4100, 3, "f32", "custom", 0, {}, True),
    # ---- one-sided path: reduce_kernel modes 1 and 2
    ("onesided-f64", 4000, 2, "f64", "float64", 0, NS, False),
    ("onesided-f32", 1000, 2, "f32", "float32", 0, {"NB_SYM": "0", **NS}, False),
    # ---- generic path: the closing kick in a launch of its own (axpy).  No call defers it: step_run defers only with
    # uniform dtypes outside the grid modes, which never take the generic path, so that branch of force_eval_generic is
    # not reachable
    ("generic-int8-f64", 600, 2, "f64", "int8_sim", 0, {}, False),
    ("generic-custom5000", 4100, 2, "f32", "custom", 5000, {}, False),
    ("generic-custom5000-small", 500, 3, "f32", "custom", 5000, {}, False),
    # ---- dtype chains under a cast mode and under a grid mode
    ("chain-f32-in-float64", 1000, 2, "f32", "float64", 0, {}, False),
    ("chain-f32-in-float64-sym", 5200, 2, "f32", "float64", 0, {}, False),
    ("chain-h16-in-float64", 700, 3, "h16", "float64", 0, {}, False),
    ("chain-h16-int8-sym", 1100, 2, "h16", "int8_sim", 0, {}, False),     # non-uniform first step on the symmetric path
] + [(f"chain-{c}-{m}", 600 + 37 * i, 2 + i % 2, c, m, 0, {}, False)
     for i, c in enumerate(("h16", "b16", "m64", "v64", "h16-v64", "b16-v64", "h16-m32"))
     for m in ("float32", "int8_sim")]

# caller-made accelerations through a subclass: (id, N, dim, chain, mode, dtype of the returned accelerations)
OVERRIDE_CASES = [
    ("override-f32", 1234, 3, "f32", "float32", S32),
    ("override-f64", 1234, 2, "f64", "float64", D64),
    ("override-a32-v64", 1234, 3, "v64", "float32", S32),          # fp32 accelerations, fp64 velocities
    ("override-a32-p64", 1234, 2, (D64, S32, S32), "float32", S32),  # fp32-typed velocities beside fp64 positions
    # the grid-stride loop of the elementwise kernels wraps above 4 194 304 elements (16 384 blocks of 256)
    ("override-wrap-1.5m", 1500007, 3, "f32", "float32", S32),
]


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def to64(t):
    """A tensor's values as float64 (exact for every dtype) and its dtype code."""
    return t.detach().cpu().double().numpy().copy(), TORCH_DT[t.dtype]


class State:
    def __init__(self, sim):
        (self.x, self.cx), (self.v, self.cv), (self.a, self.ca) = to64(sim.positions), to64(sim.velocities), to64(sim.accelerations)
        dts = (C.c_int32 * 4)()
        from nbody_cosmological_simulation_amd import _native as N
        N.check(N.lib().nb_state_dtypes(sim._handle, dts))
        # (the accelerations a subclass returned are typed by their tensor until the next native call takes them)
        assert [self.cx, self.cv] == [dts[0], dts[1]] and (sim._overridden() or self.ca == dts[3])
        self.cm = dts[2]

    def dts(self):
        return [self.cx, self.cv, self.cm, self.ca]


def axpy(a, ca, b, cb, s):
    from oracle import oracle as O
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = np.empty_like(a)
    code = O.lib().nbo_axpy(a.size, ca, O._dp(a), cb, O._dp(b), float(s), O._dp(out))
    return out, code


def same(a, b):
    return np.array_equal(a, b)


def check_step(tag, prev, cur, dt, mode=None):
    """The recurrence from `prev` to `cur` with the engine's own accelerations; dtypes as the oracle promotes them."""
    from oracle import oracle as O
    vh, cvh = axpy(prev.v, prev.cv, prev.a, prev.ca, dt / 2)
    x, cx = axpy(prev.x, prev.cx, vh, cvh, dt)
    v, cv = axpy(vh, cvh, cur.a, cur.ca, dt / 2)
    assert (cur.cx, cur.cv) == (cx, cv), (tag, "dtypes", (cur.cx, cur.cv), (cx, cv))
    if mode is not None:
        assert cur.ca == O.lib().nbo_acc_dtype(cx, cur.cm, MODE_CODES[mode]), (tag, "acceleration dtype", cur.ca)
    bad_x, bad_v = int((cur.x != x).sum()), int((cur.v != v).sum())
    assert same(cur.x, x), f"{tag}: {bad_x} of {x.size} positions differ from the recurrence (first at {np.argwhere(cur.x != x)[:3].tolist()})"
    assert same(cur.v, v), f"{tag}: {bad_v} of {v.size} velocities differ from the recurrence (first at {np.argwhere(cur.v != v)[:3].tolist()})"


_TORCH = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32, F64: torch.float64}


def check_inputs(tag, st, dt):
    """The kick must be visible in v, and an FMA must be distinguishable from two roundings (sample of 4096 elements)."""
    vh, cvh = axpy(st.v, st.cv, st.a, st.ca, dt / 2)
    assert (vh != st.v).mean() > 0.99, (tag, "a dt/2 is lost in v", float((vh != st.v).mean()))
    idx = np.random.default_rng(5).choice(vh.size, min(4096, vh.size), replace=False)
    s = float(np.float32(dt / 2)) if st.ca != F64 else dt / 2
    fma = np.array([float(Fraction(float(st.a.flat[i])) * Fraction(s) + Fraction(float(st.v.flat[i]))) for i in idx])
    fma = torch.from_numpy(fma).to(_TORCH[cvh]).double().numpy()
    share = float((fma != vh.flat[idx]).mean())
    assert share >= 0.01, (tag, "an FMA kick would not show", share)


def make_inputs(n, dim, chain, seed=0):
    p_t, v_t, m_t = CHAINS[chain] if isinstance(chain, str) else chain
    rng = np.random.default_rng(n + 31 * dim + seed)
    pos = rng.standard_normal((n, dim)) * 0.5
    pos[rng.random(n) < 0.2] *= 8.0
    vel = rng.standard_normal((n, dim)) * 0.01
    mass = 0.5 + rng.random(n)
    return torch.from_numpy(pos).to(p_t), torch.from_numpy(vel).to(v_t), torch.from_numpy(mass).to(m_t)


def storage_f64(chain, mode):
    ch = CHAINS[chain] if isinstance(chain, str) else chain
    return mode == "float64" or D64 in ch


def build(nb, case, dt=DT0):
    cid, n, dim, chain, mode, levels, env, _ = case
    P, V, M = make_inputs(n, dim, chain)
    return nb.GalaxySimulation(P, V, M, precision_mode=nb.PrecisionMode(mode), G=G, dt=dt,
                               custom_levels=levels or None)


def step_loop(nb, case, plan, env):
    """Five verified steps; then a dt write and a velocity write, each followed by a verified step.  Returns the
    states after 0 ... NSTEPS steps."""
    cid, n, dim, chain, mode, levels, _, _ = case
    f64 = storage_f64(chain, mode)
    sim = build(nb, case)
    try:
        states = [State(sim)]
        check_inputs(cid, states[0], DT0)
        spec = 0
        assert sim.step_path_name() == "none"
        for t in range(NSTEPS):
            want, spec, _ = S.step_path(plan, n, MODE_CODES[mode], f64, states[-1].dts(), 1, spec, env, levels)
            sim.step()
            assert sim.step_path_name() == want, (cid, "step", t, sim.step_path_name(), want)
            states.append(State(sim))
            check_step(f"{cid} step {t} [{want}]", states[-2], states[-1], DT0, mode)
        # a parameter write voids the speculative drift: the next step opens with the new dt
        sim.dt = DT1
        prev = states[-1]
        want, spec, _ = S.step_path(plan, n, MODE_CODES[mode], f64, prev.dts(), 1, 0, env, levels)
        sim.step()
        assert sim.step_path_name() == want, (cid, "after dt write", sim.step_path_name(), want)
        cur = State(sim)
        check_step(f"{cid} after dt write [{want}]", prev, cur, DT1, mode)
        # the step after that opens from the positions the last launch left at the NEW dt (kick applied on read)
        prev = cur
        want, spec2, _ = S.step_path(plan, n, MODE_CODES[mode], f64, prev.dts(), 1, spec, env, levels)
        assert ("spec_read" in want) == (spec != 0), (cid, want, spec)
        sim.step()
        assert sim.step_path_name() == want, (cid, "second step after dt write", sim.step_path_name(), want)
        cur = State(sim)
        check_step(f"{cid} second step after dt write [{want}]", prev, cur, DT1, mode)
        # ... and so does a state write
        newv = sim.velocities * 0.75
        sim.velocities = newv
        prev = cur
        prev.v, prev.cv = to64(newv)
        want, spec, _ = S.step_path(plan, n, MODE_CODES[mode], f64, prev.dts(), 1, 0, env, levels)
        sim.step()
        assert sim.step_path_name() == want, (cid, "after velocity write", sim.step_path_name(), want)
        check_step(f"{cid} after velocity write [{want}]", prev, State(sim), DT1, mode)
        return states
    finally:
        sim.close()


def sites_of(case, plan, spec_on=True):
    """Every path string the case's calls report (the coverage sweep reads this on a CPU machine)."""
    cid, n, dim, chain, mode, levels, env, _ = case
    ch = CHAINS[chain] if isinstance(chain, str) else chain
    f64 = storage_f64(chain, mode)
    out = set()
    for e in ((env, {**env, "NB_NO_SPEC": "1"}) if spec_on else (env,)):
        dts = [TORCH_DT[ch[0]], TORCH_DT[ch[1]], TORCH_DT[ch[2]], None]
        dts[3] = S.acc_dtype(MODE_CODES[mode], dts[0], dts[2])
        spec, d = 0, list(dts)
        for t in range(NSTEPS):
            name, spec, d = S.step_path(plan, n, MODE_CODES[mode], f64, d, 1, spec, e, levels)
            out.add(name)
        out.add(S.step_path(plan, n, MODE_CODES[mode], f64, d, 1, 0, e, levels)[0])
        for k in (2, 5):
            out.add(S.step_path(plan, n, MODE_CODES[mode], f64, list(dts), k, 0, e, levels)[0])
    return out


def case_plan(case, cus=256):
    cid, n, dim, chain, mode, levels, env, _ = case
    return S.plan(n, dim, 0, 1, storage_f64(chain, mode), MODE_CODES[mode], cus=cus, work=False)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kick_recurrence_bit_for_bit(nb, cus, monkeypatch, case):
    cid, n, dim, chain, mode, levels, env, repack = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plan = case_plan(case, cus)
    f64 = storage_f64(chain, mode)
    states = step_loop(nb, case, plan, env)
    # the same loop without speculation: same recurrence, and (deterministic paths) the same bits
    monkeypatch.setenv("NB_NO_SPEC", "1")
    nospec = step_loop(nb, case, plan, {**env, "NB_NO_SPEC": "1"})
    monkeypatch.delenv("NB_NO_SPEC")
    for a, b in zip(states, nospec):
        assert same(a.x, b.x) and same(a.v, b.v) and same(a.a, b.a), (cid, "speculation changes the bits")
    # run(k): deterministic, and equal to the verified step loop
    for k in (2, NSTEPS):
        runs = []
        for _ in range(2):
            sim = build(nb, case)
            want = S.step_path(plan, n, MODE_CODES[mode], f64, states[0].dts(), k, 0, env, levels)[0]
            sim.run(k)
            assert sim.step_path_name() == want, (cid, f"run({k})", sim.step_path_name(), want)
            runs.append(State(sim))
            sim.close()
        r0, r1 = runs
        assert same(r0.x, r1.x) and same(r0.v, r1.v) and same(r0.a, r1.a), (cid, f"run({k}) is not run-to-run deterministic")
        ref = states[k]
        assert r0.dts() == ref.dts(), (cid, f"run({k}) dtypes", r0.dts(), ref.dts())
        for name, got, want_ in (("accelerations", r0.a, ref.a), ("positions", r0.x, ref.x), ("velocities", r0.v, ref.v)):
            assert same(got, want_), f"{cid}: run({k}) {name} differ from the step loop in {int((got != want_).sum())} of {got.size} elements"
    if repack:
        # the accelerations of steps 1 and 2 were computed from repacked positions (pack launch; speculative repack of
        # the previous reduction): a simulation rebuilt from the downloaded state must find the same ones
        assert all(s.dts()[:2] == states[0].dts()[:2] for s in states), "repack check needs settled dtypes"
        _, _, M = make_inputs(n, dim, chain)
        p_t, v_t, _ = CHAINS[chain]
        for t in (1, 2):
            sim = nb.GalaxySimulation(torch.from_numpy(states[t].x).to(p_t), torch.from_numpy(states[t].v).to(v_t), M,
                                      precision_mode=nb.PrecisionMode(mode), G=G, dt=DT0, custom_levels=levels or None)
            a, _ = to64(sim.accelerations)
            sim.close()
            assert same(a, states[t].a), f"{cid}: accelerations of step {t} differ from a rebuilt simulation in {int((a != states[t].a).sum())} elements"


@pytest.mark.parametrize("case", OVERRIDE_CASES, ids=[c[0] for c in OVERRIDE_CASES])
def test_override_kicks_bit_for_bit(nb, case):
    """nb_kick_drift / nb_kick around caller-made accelerations (the subclass rule): distinct values per element, so a
    skipped or doubled element of the grid-stride loop cannot cancel."""
    cid, n, dim, chain, mode, a_t = case
    P, V, M = make_inputs(n, dim, chain)
    rng = np.random.default_rng(n)
    accs = [torch.from_numpy(rng.standard_normal((n, dim)) * 3.0 + 0.001 * np.arange(n * dim).reshape(n, dim) / (n * dim)).to(a_t)
            for _ in range(3)]

    class Fixed(nb.GalaxySimulation):
        calls = 0

        def _compute_accelerations(self):
            self.calls += 1
            return accs[(self.calls - 1) % len(accs)]

    sim = Fixed(P, V, M, precision_mode=nb.PrecisionMode(mode), G=G, dt=DT0)
    try:
        prev = State(sim)
        check_inputs(cid, prev, DT0)
        for t, dt in enumerate((DT0, DT0, DT1)):
            sim.dt = dt
            sim.step()
            mixed = storage_f64(chain, mode) and TORCH_DT[a_t] == F32
            want = "open=kick_a32 close=kick_a32" if mixed else "open=kick_drift close=axpy"
            assert sim.step_path_name() == want, (cid, sim.step_path_name(), want)
            cur = State(sim)
            check_step(f"{cid} step {t}", prev, cur, dt)
            prev = cur
        assert sim.calls == 4
    finally:
        sim.close()


# ---- multi-rank sites (tests/tools/multirank_worker.py under test_gpu_parity.test_multi_rank_product_path_on_one_gpu) ----
# step_path_name() of (a step() call, run(3)) per worker case and variant of that test: "" the kicks inside the direct
# all-reduce (p2p:1 / p2p:2; INT8 exchanges fp64 sums and kicks in the finish launch), "deferred-kick" / "rccl-shaped"
# the closing kick in a launch of its own, deferred into the next step's pack launch (pack:2) inside a call
def _paths(first_open, later_open, close, run):
    """Names of three step() calls and of run(3)."""
    return [f"open={first_open} close={close}"] + [f"open={later_open} close={close}"] * 2 + [run]


# f64 / f64_onesided start from fp32 state in FLOAT64 mode: their first step opens with a launch of its own (non-uniform
# dtypes), and inside run(3) its closing kick cannot be fused with the next opening kick
_P2P = {"f64": _paths("kick_drift", "pack:1", "p2p:1", "open=kick_drift mid=p2p:1+pack:1+p2p:2 close=p2p:1"),
        "f32": _paths("pack:1", "pack:1", "p2p:1", "open=pack:1 mid=p2p:2 close=p2p:1"),
        "int8_big": _paths("kick_drift", "kick_drift", "fq_finish:1", "open=kick_drift mid=fq_finish:2,packed close=fq_finish:1"),
        "f64_onesided": _paths("kick_drift", "kick_drift", "p2p:1", "open=kick_drift mid=p2p:1+kick_drift+p2p:2 close=p2p:1")}
_DEFER = {"f64": _paths("kick_drift", "pack:1", "axpy", "open=kick_drift mid=axpy+pack:1+pack:2 close=axpy"),
          "f32": _paths("pack:1", "pack:1", "axpy", "open=pack:1 mid=pack:2 close=axpy"),
          "int8_big": _P2P["int8_big"],
          "f64_onesided": _paths("kick_drift", "kick_drift", "axpy", "open=kick_drift mid=axpy+kick_drift close=axpy")}
MULTIRANK_PATHS = {"": _P2P, "deferred-kick": _DEFER, "rccl-shaped": _DEFER}
# test_gpu_parity.test_two_rank_rccl_step_matches_single_gpu (two GPUs): INT4 exchanges fp64 sums over RCCL, and
# nb_launch_finish_sums64 rounds them before the finish launch applies the kicks
RCCL_PATHS = {"f64": _DEFER["f64"], "int4_big": _P2P["int8_big"]}


class Snap:
    """One state of a worker's trace, shaped like State."""

    def __init__(self, arrays, key, codes):
        self.x, self.v, self.a = (np.ascontiguousarray(arrays[f"{key}/{p}"]) for p in "xva")
        self.cx, self.cv, self.ca = codes


def check_multirank_trace(rank0, arrays, variant, expected):
    seen = {}
    for name in expected:
        tr = rank0[name]["trace"]
        k = len(tr["codes"]) - 2
        states = [Snap(arrays, f"{name}/{i}", tr["codes"][i]) for i in range(k + 1)]
        check_inputs(f"multirank {name}", states[0], tr["dt"])
        for i in range(k):
            check_step(f"multirank {variant or 'direct'} {name} step {i} [{tr['paths'][i]}]", states[i], states[i + 1], tr["dt"])
        run = Snap(arrays, f"{name}/run", tr["codes"][-1])
        for part in "avx":
            got, want = getattr(run, part), getattr(states[k], part)
            assert same(got, want), f"multirank {variant} {name}: run({k}) [{tr['paths'][-1]}] differs from the step loop in {int((got != want).sum())} elements of {part}"
        seen[name] = tr["paths"]
    print("multirank step paths", variant or "direct", seen)
    for name, want in expected.items():
        assert seen[name] == want, (variant, name, seen[name], want)


def multirank_sites():
    """(part, site) tokens the multi-rank cases assert (for the coverage sweep)."""
    return {(part.split("=")[0], site) for v in MULTIRANK_PATHS.values() for names in v.values() for n in names
            for part in n.split() for site in part.split("=")[1].split("+")}


def test_step_path_name_before_any_step(nb):
    pos = torch.rand(300, 2, dtype=torch.float64)
    sim = nb.GalaxySimulation(pos, torch.zeros_like(pos), torch.ones(300, dtype=torch.float64))
    assert sim.step_path_name() == "none"
    sim.step()
    assert sim.step_path_name() == "open=kick_drift close=small:3"
    sim.close()
