"""Work-plan shapes of the force path, read through the device-free C-ABI entry nb_plan_debug.

One place for three things:
  plan() / shape_key()  what the planner (nb_plan.cpp) hands a rank: targets per lane R, source tiles per item cl,
                        row-split items, the step pieces its sweeps are cut into, the one-sided kernels' source chunks;
  COVERED               the shape keys tests/test_gpu_plan_shapes.py runs against the oracle on the GPU;
  pe_variant()          the potential-energy kernel variant energy_eval (nb_step.cpp) picks for a plan and a dtype
                        chain -- tests/test_gpu_energy_shapes.py asserts it against nb_pe_kernel_name on the GPU.
  step_path()           the sites of the leapfrog kicks step_run (nb_step.cpp) picks for a call -- tests/test_gpu_kick_paths.py
                        asserts it against nb_step_path_name on the GPU before it checks the recurrence bit for bit.
tests/test_distributed_cpu.py sweeps the planner over sizes, modes and rank counts and fails on a CPU machine when
it emits a key (or a PE variant) that no GPU case covers: a retune that creates a new shape needs a GPU case for it.
"""
import ctypes as C

import numpy as np

# mode codes of nb_config.mode and dtype codes of nb_dtype (include/nbody_amd.h)
FLOAT64, FLOAT32, BFLOAT16, FLOAT16, INT8 = 0, 1, 2, 3, 4
DT_F16, DT_BF16, DT_F32, DT_F64 = 0, 1, 2, 3
_DT_NAME = {DT_F16: "f16", DT_BF16: "bf16", DT_F32: "f32", DT_F64: "f64"}

_INFO = ["enabled", "r", "tile_b", "tiles", "np", "nwork", "nslots", "ncol", "cl", "nchunks", "col_mib", "row_mib",
         "rowsplit", "onesided_r", "os_nchunks", "os_chunk_len"]


def plan(n, dim, rank=0, world=1, is_f64=True, mode=FLOAT64, cus=256, work=True, no_comm=False):
    """The plan of one rank (the knobs NB_SYM* are read from the environment, as nb_create does)."""
    from nbody_cosmological_simulation_amd import _native as N
    L = N.lib()
    cfg = N.NbConfig(n=n, dim=dim, mode=mode, levels=0, G=1e-3, softening_sq=0.01, dt=0.01, device=0, rank=rank,
                     nranks=world, flags=N.NB_FLAG_NO_COMM if no_comm else 0)
    info = (C.c_int32 * 16)()
    N.check(L.nb_plan_debug(C.byref(cfg), int(is_f64), 0, cus, info, None, 0, None, None, None, None, None))
    out = dict(zip(_INFO, list(info)))
    if out["enabled"] and work:
        w = np.zeros((out["nwork"], 8), np.int32)
        N.check(L.nb_plan_debug(C.byref(cfg), int(is_f64), 0, cus, info, w.ctypes.data_as(C.POINTER(C.c_int32)),
                                out["nwork"], None, None, None, None, None))
        out["work"] = w
    return out


def pe_variant(p, dim, storage_f64, pos_dt, mass_dt, uniform, no_pe_sym=False):
    """The potential-energy kernel energy_eval launches, as nb_pe_kernel_name reports it, for a rank's plan `p` (from
    plan(); only enabled / r / rowsplit are read), the state's storage type, the logical dtypes of positions and
    masses (DT_*) and whether all masses are equal.  The pair-symmetric kernel walks the force plan's work list when
    the plan has two or four targets per lane and the positions are not half-typed; everything else (R = 1 plans,
    one-sided force plans, half-typed positions, NB_NO_PE_SYM) takes the one-sided kernel."""
    hp = pos_dt in (DT_F16, DT_BF16)
    T = "double" if storage_f64 else "float"
    if p["enabled"] and not hp and p["r"] in (2, 4) and not no_pe_sym:
        f32t = not storage_f64 or pos_dt != DT_F64
        narrow = storage_f64 and not f32t and not uniform and mass_dt != DT_F64
        return (f"potential_sym_kernel<{T},{dim},{p['r']},f32t={int(f32t)},uniform={int(bool(uniform))}"
                f"{',mass=' + _DT_NAME[mass_dt] if narrow else ''}{',rowsplit' if p['rowsplit'] > 0 else ''}>")
    pa_f32 = not storage_f64 or pos_dt != DT_F64
    narrow = not pa_f32 and mass_dt != DT_F64
    return (f"potential_kernel<{T},{dim},pa_f32={int(pa_f32)},hp={_DT_NAME[pos_dt] if hp else 'none'}"
            f"{',mass=' + _DT_NAME[mass_dt] if narrow else ''}>")


INT4, CUSTOM = 5, 6
SMALL_MAX_F64, SMALL_MAX_F32, LUT_MIN, MAX_LUT, RED_MM_MAX_BLOCKS = 4096, 3072, 256, 4096, 1024


def _promote(a, b):
    return a if a == b else (DT_F64 if DT_F64 in (a, b) else DT_F32)


def mode_levels(mode, levels=0):
    return {INT8: 256, INT4: 16}.get(mode, levels if levels > 0 else 64)


def acc_dtype(mode, pos_dt, mass_dt):
    """promote(promote(promote(Q, M), fp32), P), Q the hook's output dtype (nb_step.cpp acc_logical_dtype)."""
    q = DT_F64 if mode == FLOAT64 else (DT_F32 if mode <= FLOAT16 else pos_dt)
    return _promote(_promote(_promote(q, mass_dt), DT_F32), pos_dt)


def step_path(p, n, mode, storage_f64, dts, nsteps, spec=0, env=(), levels=0):
    """The string nb_step_path_name reports after nb_step(nsteps) on ONE GPU, the speculation state the call leaves
    (0 none, 1 small-system kernel, 2 reduce_sym_kernel) and the logical dtypes after it.  `p`: the rank's plan (only
    enabled is read); dts: logical dtypes [positions, velocities, masses, accelerations] before the call; spec: the
    state the previous call left (0 after any write of state or dt); env: the knobs of the case.  A line-by-line
    mirror of step_run / step_small / force_eval's choice of the launch that applies each kick."""
    P, V, M, A = dts
    sdt = DT_F64 if storage_f64 else DT_F32
    grid, fq = mode >= INT8, mode in (INT8, INT4)
    L = mode_levels(mode, levels)
    no_spec, no_smalln = "NB_NO_SPEC" in env, "NB_NO_SMALLN" in env
    parts = [[], [], []]

    def note(where, site):
        if site and site not in parts[where]:
            parts[where].append(site)

    def finish(spec_out):
        name = " ".join(k + "+".join(v) for k, v in zip(("open=", "mid=", "close="), parts) if v)
        return name or "none", spec_out, [P, V, M, A]

    def uniform():
        return P == sdt and V == sdt and A == sdt

    def small_ok():
        if no_smalln or n > (SMALL_MAX_F64 if storage_f64 else SMALL_MAX_F32):
            return False
        if grid and (storage_f64 or L > LUT_MIN or L < 2):
            return False
        if storage_f64 != (mode == FLOAT64):
            return False
        return uniform() and (M == sdt or (storage_f64 and M == DT_F32))

    def generic():
        if grid and L > MAX_LUT:
            return True
        if storage_f64:
            return False if mode == FLOAT64 else (True if grid else P != DT_F64)
        return grid and P in (DT_F16, DT_BF16)

    def plain(drift):
        return "kick_a32" if storage_f64 and A == DT_F32 else ("kick_drift" if drift else "axpy")

    pending = opened = open_on_read = False
    for t in range(nsteps):
        if not pending and small_ok():
            rest = nsteps - t
            speculate = not grid and not fq and not no_spec
            on_read = False
            if not opened:
                on_read = speculate and spec == 1
                note(0 if t == 0 else 1, "spec_read" if on_read else "kick_drift")
            for u in range(rest):
                last = u + 1 == rest
                if fq:
                    site = "fq_finish:%d,small" % (1 if last else 2)
                else:
                    site = "small:%d%s" % ((3 if speculate else 1) if last else 2, "|4" if (u == 0 and on_read) else "")
                note(2 if last else 1, site)
            return finish(1 if speculate else 0)
        if t == 0 and spec == 2 and p["enabled"] and not fq and not grid and uniform():
            opened = open_on_read = True
            note(0, "spec_read")
        fuse_pack = p["enabled"] and uniform() and not grid
        uni = uniform()
        if opened:
            pass
        elif fuse_pack:
            note(0 if t == 0 else 1, "pack:2" if pending else "pack:1")
        else:
            if pending:
                note(1, plain(False))
            note(0 if t == 0 else 1, plain(True))
        pending = False
        V = _promote(V, A)
        P = _promote(P, V)
        inner = t + 1 < nsteps
        may_defer = inner and fuse_pack
        want_open = inner and uni
        spec_next = (not inner) and uni and p["enabled"] and not no_spec
        site, opened = "", False
        if generic():
            site = "axpy"
        else:
            if storage_f64:
                used_sym = p["enabled"] and mode == FLOAT64 and (P == DT_F64 or (P == DT_F32 and p["r"] in (2, 4)))
            else:
                used_sym = p["enabled"] and P == DT_F32
            if fq:
                red_mm = used_sym and not storage_f64 and (n + 63) // 64 <= RED_MM_MAX_BLOCKS and "NB_NO_RED_MM" not in env
                k = 2 if want_open else 1
                tags = (",packed" if (k == 2 and used_sym) else "") + (",red_mm" if red_mm else "")
                site, opened = "fq_finish:%d%s" % (k, tags), want_open
            elif used_sym:
                spec_now = (not want_open) and spec_next and not grid
                k = 2 if want_open else (3 if spec_now else 1)
                site = "reduce_sym:%d%s" % (k, "|4" if (t == 0 and open_on_read) else "")
                opened = want_open
            else:
                site, opened = "reduce:%d" % (2 if want_open else 1), want_open
        note(1 if inner else 2, site)
        A = acc_dtype(mode, P, M)
        V = _promote(V, A)
    return finish(2 if parts[2] and parts[2][-1].startswith("reduce_sym:3") else 0)


def pieces(p):
    """Sorted distinct numbers of step pieces the sweeps of a plan are cut into (work items that share target tile
    and source range are the pieces of one sweep)."""
    _, counts = np.unique(p["work"][:, :3], axis=0, return_counts=True)
    return tuple(int(c) for c in np.unique(counts))


def shape_key(p, dim, is_f64):
    """(R, dim, fp64, row-split, piece counts, cl == 1) of an enabled plan."""
    return (p["r"], dim, bool(is_f64), p["rowsplit"] > 0, pieces(p), p["cl"] == 1)


def onesided_key(p, dim, is_f64):
    """Key of a plan that leaves the force to the one-sided kernels (fp32 state: always two targets per thread)."""
    return ("onesided", p["onesided_r"] if is_f64 else 2, dim, bool(is_f64))


def rank_keys(n, dim, world=1, is_f64=True, mode=FLOAT64, cus=256, no_comm=False):
    """Shape keys of every rank of a plan (no_comm: comm-less shards, as the GPU cases run them with NB_SYM=2)."""
    keys = set()
    for r in range(world):
        p = plan(n, dim, r, world, is_f64=is_f64, mode=mode, cus=cus, no_comm=no_comm)
        keys.add(shape_key(p, dim, is_f64) if p["enabled"] else onesided_key(p, dim, is_f64))
    return keys


def K(r, dim, f64, rowsplit, pieces_, cl1=True):
    return (r, dim, f64, rowsplit, tuple(pieces_), cl1)


# The GPU cases of tests/test_gpu_plan_shapes.py: (id, N, dim, state dtype, mode, ranks, knobs, shape keys of the
# ranks' plans, force kernel).  Ranks > 1 run as comm-less shards (NB_SYM=2) whose partial forces are summed.
# Sizes are ragged (N % tile != 0, tiles % 4 != 0) where the shape allows it.
F64, F32 = "float64", "float32"
SYM64, SYM32, ONE64, ONE32 = "force_sym_kernel<double", "force_sym_kernel<float", "force_f64_kernel", "force_f32_kernel"
CASES = [
    # ---- default plans, fp64, 2-D
    ("f64-d2-tiny-p8", 700, 2, F64, "float64", 1, {}, {K(1, 2, True, False, (8,))}, SYM64),
    ("f64-d2-tiny-p4", 1000, 2, F64, "float64", 1, {}, {K(1, 2, True, False, (4,))}, SYM64),
    ("f64-d2-tiny-p2", 1400, 2, F64, "float64", 1, {}, {K(1, 2, True, False, (2,))}, SYM64),
    ("f64-d2-tiny-p1", 2000, 2, F64, "float64", 1, {}, {K(1, 2, True, False, (1,))}, SYM64),
    ("f64-d2-onesided-r1", 4000, 2, F64, "float64", 1, {"NB_NO_SMALLN": "1"}, {("onesided", 1, 2, True)}, ONE64),
    ("f64-d2-rowsplit2", 5200, 2, F64, "float64", 1, {}, {K(4, 2, True, True, (2,))}, SYM64),
    ("f64-d2-rowsplit3", 6300, 2, F64, "float64", 1, {}, {K(4, 2, True, True, (3,))}, SYM64),
    ("f64-d2-rowsplit1", 12000, 2, F64, "float64", 1, {}, {K(4, 2, True, True, (1,))}, SYM64),
    ("f64-d2-classic6", 5800, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (6,))}, SYM64),
    ("f64-d2-classic6-b", 9900, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (6,))}, SYM64),
    ("f64-d2-classic2", 15400, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (2,))}, SYM64),
    ("f64-d2-whole", 22400, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (1,))}, SYM64),
    ("f64-d2-tail8", 23800, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (1, 8))}, SYM64),
    ("f64-d2-tail4", 32300, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (1, 4))}, SYM64),
    ("f64-d2-cl3-tail4", 56700, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (1, 4), False)}, SYM64),
    ("f64-d2-cl2", 52700, 2, F64, "float64", 1, {}, {K(4, 2, True, False, (1,), False)}, SYM64),
    ("f64-d2-onesided-r2-1m", 1 << 20, 2, F64, "float64", 1, {}, {("onesided", 2, 2, True)}, ONE64),
    # ---- default plans, fp64, 3-D
    ("f64-d3-onesided-r1", 5000, 3, F64, "float64", 1, {"NB_NO_SMALLN": "1"}, {("onesided", 1, 3, True)}, ONE64),
    ("f64-d3-classic3", 8200, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (3,))}, SYM64),
    ("f64-d3-classic4", 8900, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (4,))}, SYM64),
    ("f64-d3-classic5", 9700, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (5,))}, SYM64),
    ("f64-d3-classic5-b", 13000, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (5,))}, SYM64),
    ("f64-d3-classic2", 10100, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (2,))}, SYM64),
    ("f64-d3-whole", 22400, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (1,))}, SYM64),
    ("f64-d3-tail8", 23800, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (1, 8))}, SYM64),
    ("f64-d3-tail4", 32300, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (1, 4))}, SYM64),
    ("f64-d3-cl2-tail4", 46600, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (1, 4), False)}, SYM64),
    ("f64-d3-cl2", 52700, 3, F64, "float64", 1, {}, {K(4, 3, True, False, (1,), False)}, SYM64),
    ("f64-d3-onesided-r2", 535841, 3, F64, "float64", 1, {}, {("onesided", 2, 3, True)}, ONE64),
    # ---- default plans, fp32 family
    ("f32-d2-onesided", 1000, 2, F32, "float32", 1, {"NB_SYM": "0", "NB_NO_SMALLN": "1"}, {("onesided", 2, 2, False)}, ONE32),
    ("f32-d3-onesided", 2000, 3, F32, "float16", 1, {"NB_NO_SMALLN": "1"}, {("onesided", 2, 3, False)}, ONE32),
    ("f32-d2-p8", 1100, 2, F32, "float32", 1, {"NB_NO_SMALLN": "1"}, {K(2, 2, False, False, (8,))}, SYM32),
    ("f32-d2-p4", 1500, 2, F32, "float16", 1, {"NB_NO_SMALLN": "1"}, {K(2, 2, False, False, (4,))}, SYM32),
    ("f32-d2-p2", 4000, 2, F32, "int8_sim", 1, {}, {K(2, 2, False, False, (2,))}, SYM32),
    ("f32-d2-whole", 7100, 2, F32, "float32", 1, {}, {K(2, 2, False, False, (1,))}, SYM32),
    ("f32-d2-tail2", 11500, 2, F32, "float32", 1, {}, {K(2, 2, False, False, (1, 2))}, SYM32),
    ("f32-d3-p2", 4100, 3, F32, "float32", 1, {}, {K(2, 3, False, False, (2,))}, SYM32),
    ("f32-d3-whole", 7100, 3, F32, "float16", 1, {}, {K(2, 3, False, False, (1,))}, SYM32),
    ("f32-d3-tail2", 11500, 3, F32, "float32", 1, {}, {K(2, 3, False, False, (1, 2))}, SYM32),
    ("f32-d2-r4-p4", 21100, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (4,))}, SYM32),
    ("f32-d2-r4-whole", 22400, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (1,))}, SYM32),
    ("f32-d2-r4-tail8", 23800, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (1, 8))}, SYM32),
    ("f32-d2-r4-tail4", 32300, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (1, 4))}, SYM32),
    ("f32-d2-r4-cl2-tail4", 65600, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (1, 4), False)}, SYM32),
    ("f32-d2-r4-cl2", 71500, 2, F32, "float32", 1, {}, {K(4, 2, False, False, (1,), False)}, SYM32),
    ("f32-d3-r4-p4", 21100, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (4,))}, SYM32),
    ("f32-d3-r4-whole", 22400, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (1,))}, SYM32),
    ("f32-d3-r4-tail8", 23800, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (1, 8))}, SYM32),
    ("f32-d3-r4-tail4", 32300, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (1, 4))}, SYM32),
    ("f32-d3-r4-cl2-tail4", 65600, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (1, 4), False)}, SYM32),
    ("f32-d3-r4-cl2", 71500, 3, F32, "float32", 1, {}, {K(4, 3, False, False, (1,), False)}, SYM32),
    ("f32-d3-onesided-1m", 1 << 20, 3, F32, "float32", 1, {}, {("onesided", 2, 3, False)}, ONE32),
    # ---- multi-rank plans (comm-less shards, NB_SYM=2)
    ("f64-d2-9000-p2", 9000, 2, F64, "float64", 2, {}, {K(4, 2, True, True, (3,))}, SYM64),
    ("f64-d2-9000-p3", 9000, 2, F64, "float64", 3, {}, {K(4, 2, True, True, (2,))}, SYM64),
    ("f64-d2-9000-p4", 9000, 2, F64, "float64", 4, {}, {K(4, 2, True, False, (5,)), K(4, 2, True, True, (3,))}, SYM64),
    ("f64-d2-9000-p8", 9000, 2, F64, "float64", 8,
     {}, {K(4, 2, True, False, (6,)), K(4, 2, True, True, (2,)), K(4, 2, True, True, (3,)), K(4, 2, True, True, (4,))}, SYM64),
    ("f64-d2-16384-p4", 16384, 2, F64, "float64", 4, {}, {K(4, 2, True, True, (2,))}, SYM64),
    ("f64-d2-16384-p8", 16384, 2, F64, "float64", 8, {}, {K(4, 2, True, False, (6,))}, SYM64),
    ("f64-d2-19800-p2", 19800, 2, F64, "float64", 2, {}, {K(4, 2, True, False, (3,))}, SYM64),
    ("f64-d3-8192-p8", 8192, 3, F64, "float64", 8, {}, {K(4, 3, True, False, (8,))}, SYM64),
    ("f64-d3-8192-p2", 8192, 3, F64, "float64", 2, {}, {K(4, 3, True, False, (6,))}, SYM64),
    ("f32-d3-4096-p3", 4096, 3, F32, "float32", 3, {}, {K(2, 3, False, False, (4,))}, SYM32),
    ("f32-d3-4096-p8", 4096, 3, F32, "float32", 8, {}, {K(2, 3, False, False, (4,)), K(2, 3, False, False, (8,))}, SYM32),
    ("f32-d2-21100-p2", 21100, 2, F32, "float32", 2, {}, {K(4, 2, False, False, (2,))}, SYM32),
    ("f32-d2-22400-p3", 22400, 2, F32, "float32", 3, {}, {K(4, 2, False, False, (3,))}, SYM32),
    ("f32-d2-28625-p8", 28625, 2, F32, "float32", 8, {}, {K(4, 2, False, False, (5,)), K(4, 2, False, False, (6,))}, SYM32),
    ("f32-d3-21100-p2", 21100, 3, F32, "float32", 2, {}, {K(4, 3, False, False, (2,))}, SYM32),
    ("f32-d3-22400-p3", 22400, 3, F32, "float32", 3, {}, {K(4, 3, False, False, (3,))}, SYM32),
    ("f32-d3-28625-p8", 28625, 3, F32, "float32", 8, {}, {K(4, 3, False, False, (5,)), K(4, 3, False, False, (6,))}, SYM32),
    # ---- shapes forced through the per-handle knobs
    ("knob-r2-f64", 3000, 2, F64, "float64", 1, {"NB_SYM": "1", "NB_SYM_R": "2"}, {K(2, 2, True, False, (2,))}, SYM64),
    ("knob-r1-f64", 3100, 2, F64, "float64", 1, {"NB_SYM": "1", "NB_SYM_R": "1"}, {K(1, 2, True, False, (1,))}, SYM64),
    ("knob-r4-f32", 3000, 2, F32, "float32", 1, {"NB_SYM": "1", "NB_SYM_R": "4"}, {K(4, 2, False, False, (8,))}, SYM32),
    ("knob-cl3", 20000, 2, F64, "float64", 1, {"NB_SYM_CL": "3"}, {K(4, 2, True, False, (4,), False)}, SYM64),
    ("knob-cl8", 30000, 3, F64, "float64", 1, {"NB_SYM_CL": "8"}, {K(4, 3, True, False, (2,), False)}, SYM64),
    ("knob-cl5-f32", 30000, 2, F32, "float32", 1, {"NB_SYM_CL": "5"}, {K(4, 2, False, False, (4,), False)}, SYM32),
    ("knob-split3", 8000, 2, F64, "float64", 1, {"NB_SYM_SPLIT": "3"}, {K(4, 2, True, False, (3,))}, SYM64),
    ("knob-split5", 9000, 3, F64, "float64", 1, {"NB_SYM_SPLIT": "5"}, {K(4, 3, True, False, (5,))}, SYM64),
    ("knob-split7", 8000, 2, F32, "float32", 1, {"NB_SYM_SPLIT": "7"}, {K(2, 2, False, False, (7,))}, SYM32),
    ("knob-split16", 8000, 2, F64, "float64", 1, {"NB_SYM_SPLIT": "16"}, {K(4, 2, True, False, (16,))}, SYM64),
    ("knob-rowsplit1", 8000, 2, F64, "float64", 1, {"NB_SYM_ROWSPLIT": "1"}, {K(4, 2, True, True, (1,))}, SYM64),
    ("knob-rowsplit2", 8000, 2, F64, "float64", 1, {"NB_SYM_ROWSPLIT": "2"}, {K(4, 2, True, True, (2,))}, SYM64),
    ("knob-rowsplit3", 8000, 2, F64, "float64", 1, {"NB_SYM_ROWSPLIT": "3"}, {K(4, 2, True, True, (3,))}, SYM64),
    ("knob-rowsplit4", 8000, 2, F64, "float64", 1, {"NB_SYM_ROWSPLIT": "4"}, {K(4, 2, True, True, (4,))}, SYM64),
    ("knob-rowsplit8", 8000, 2, F64, "float64", 1, {"NB_SYM_ROWSPLIT": "8"}, {K(4, 2, True, True, (8,))}, SYM64),
    ("knob-tail2", 23800, 2, F64, "float64", 1, {"NB_SYM_TAIL": "2"}, {K(4, 2, True, False, (1, 2))}, SYM64),
    ("knob-tail4", 23800, 3, F64, "float64", 1, {"NB_SYM_TAIL": "4"}, {K(4, 3, True, False, (1, 4))}, SYM64),
    ("knob-tail16", 23800, 2, F32, "float32", 1, {"NB_SYM_TAIL": "16"}, {K(4, 2, False, False, (1, 16))}, SYM32),
    ("knob-onesided-r1", 12000, 2, F64, "float64", 1, {"NB_SYM": "0", "NB_R": "1"}, {("onesided", 1, 2, True)}, ONE64),
    ("knob-onesided-r2", 5000, 3, F64, "float64", 1, {"NB_SYM": "0", "NB_R": "2", "NB_NO_SMALLN": "1"},
     {("onesided", 2, 3, True)}, ONE64),
    ("knob-onesided-r4", 12000, 2, F64, "float64", 1, {"NB_SYM": "0", "NB_R": "4"}, {("onesided", 4, 2, True)}, ONE64),
]

# the shape keys the GPU module compares with the oracle: one entry per key, from the case table above
COVERED = sorted({k for case in CASES for k in case[7]}, key=str)
