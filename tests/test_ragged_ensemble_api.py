"""RaggedEnsemble without a GPU: the exports and what is inherited, every refusal of check_ragged_arguments (all made in
Python, before any native call), the refusals that need no device (a baseline of another size, the three follow-ups), the
C-ABI constructor's refusals before a device is looked for, the loud failure when there is no device, and the work-list
planner, which needs no device at all."""
import ctypes as C

import pytest
import torch

import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import _native
from nbody_cosmological_simulation_amd import ensemble as E

PM = nb.PrecisionMode


def state(sizes, d=2, dtype=torch.float32):
    g = torch.Generator().manual_seed(11)
    return ([torch.randn(n, d, generator=g).to(dtype) for n in sizes], [torch.randn(n, d, generator=g).to(dtype) for n in sizes],
            [(0.5 + torch.rand(n, generator=g)).to(dtype) for n in sizes])


@pytest.fixture
def no_native(monkeypatch):
    """Any native call fails the test: argument errors must be raised before the library is reached."""
    def boom():
        raise AssertionError("the native library was reached before the arguments were checked")
    monkeypatch.setattr(_native, "lib", boom)


def bare(sizes):
    """A RaggedEnsemble that never met the library: what the device-free refusals read."""
    e = object.__new__(E.RaggedEnsemble)
    e._sizes, e.num_members = list(sizes), len(sizes)
    return e


def test_package_exports_ragged_ensemble():
    assert "RaggedEnsemble" in nb.__all__ and "check_ragged_arguments" in nb.__all__
    assert nb.RaggedEnsemble is E.RaggedEnsemble and nb.check_ragged_arguments is E.check_ragged_arguments
    assert issubclass(E.RaggedEnsemble, E.GalaxyEnsemble) and not issubclass(E.RaggedEnsemble, E.QuantizedEnsemble)
    # inherited, not re-implemented
    for name in ("step", "run", "run_recorded", "run_members", "run_watched", "energies", "set_params", "member_ticks",
                 "launches", "force_kernel_name", "synchronize", "close", "get_state", "get_total_energy"):
        assert getattr(E.RaggedEnsemble, name) is getattr(E.GalaxyEnsemble, name), name
    # the list-speaking entries and the refusals are its own
    for name in ("positions", "velocities", "masses", "accelerations", "set_state", "set_accelerations", "divergence",
                 "run_diverged", "metrics", "run_crash_watched", "crash_measures"):
        assert getattr(E.RaggedEnsemble, name) is not getattr(E.GalaxyEnsemble, name), name


def test_new_symbols_are_exported():
    for name in ("nb_ens_create_ragged", "nb_ens_ragged_plan"):
        assert name in _native.EXPORTS, name


def test_good_arguments(no_native):
    sizes = [37, 700, 2, 64]
    p, v, m = state(sizes, 3)
    P, V, M, S, modes, G, soft, dt = E.check_ragged_arguments(p, v, m, PM.FLOAT32, G=[0.1, 0.2, 0.3, 0.4], dt=0.02)
    assert S == sizes and modes is None and G == [0.1, 0.2, 0.3, 0.4] and soft == [0.1] * 4 and dt == [0.02] * 4
    assert all(a is b for a, b in zip(P, p)) and isinstance(P, list)
    lst = [PM.FLOAT32, PM.BFLOAT16, PM.FLOAT16, PM.FLOAT32]
    assert E.check_ragged_arguments(tuple(p), tuple(v), tuple(m), lst)[4] == lst
    p64, v64, m64 = state([4096, 1], 2, torch.float64)
    assert E.check_ragged_arguments(p64, v64, m64)[3] == [4096, 1]                       # the fp64 limit itself
    assert E.check_ragged_arguments(*state([3072, 5]), PM.FLOAT16)[3] == [3072, 5]         # the fp32 limit itself


def test_mismatched_list_lengths(no_native):
    p, v, m = state([8, 9, 10])
    with pytest.raises(ValueError, match="positions has 3 members, velocities 2 and masses 3"):
        nb.RaggedEnsemble(p, v[:2], m, PM.FLOAT32)
    with pytest.raises(ValueError, match="positions has 3 members, velocities 3 and masses 4"):
        nb.RaggedEnsemble(p, v, m + m[:1], PM.FLOAT32)
    with pytest.raises(ValueError, match=r"B must be in \[1, 1024\], got 0"):
        nb.RaggedEnsemble([], [], [], PM.FLOAT32)
    with pytest.raises(ValueError, match="precision_mode has 2 entries for 3 members"):
        nb.RaggedEnsemble(p, v, m, [PM.FLOAT32, PM.FLOAT16])
    for kw in (dict(G=[0.001, 0.002]), dict(softening=[0.1] * 4), dict(dt=(0.01,))):
        with pytest.raises(ValueError, match="for 3 members"):
            nb.RaggedEnsemble(p, v, m, PM.FLOAT32, **kw)
    with pytest.raises(TypeError, match="positions must be a sequence of per-member tensors, got Tensor"):
        nb.RaggedEnsemble(torch.zeros(3, 8, 2), v, m, PM.FLOAT32)


def test_mixed_d_and_bad_shapes(no_native):
    p, v, m = state([8, 9, 10])
    p3, v3, _ = state([9], 3)
    with pytest.raises(ValueError, match="member 1 has D = 3 and member 0 has D = 2"):
        nb.RaggedEnsemble([p[0], p3[0], p[2]], [v[0], v3[0], v[2]], m, PM.FLOAT32)
    with pytest.raises(ValueError, match="member 2: D must be 2 or 3, got 4"):
        nb.RaggedEnsemble(p[:2] + [torch.zeros(10, 4)], v[:2] + [torch.zeros(10, 4)], m, PM.FLOAT32)
    with pytest.raises(ValueError, match=r"member 1: positions \(9, 2\), velocities \(8, 2\) and masses \(9,\) disagree"):
        nb.RaggedEnsemble(p, [v[0], v[0], v[2]], m, PM.FLOAT32)
    with pytest.raises(ValueError, match=r"member 0: positions must be \(N, D\) with \(N,\) masses"):
        nb.RaggedEnsemble([p[0][None]] + p[1:], v, m, PM.FLOAT32)
    with pytest.raises(TypeError, match=r"masses\[2\] must be a torch.Tensor, got list"):
        nb.RaggedEnsemble(p, v, m[:2] + [[1.0] * 10], PM.FLOAT32)


def test_an_empty_member(no_native):
    p, v, m = state([8, 9])
    with pytest.raises(ValueError, match="member 1 is empty"):
        nb.RaggedEnsemble([p[0], torch.zeros(0, 2), p[1]], [v[0], torch.zeros(0, 2), v[1]], [m[0], torch.zeros(0), m[1]],
                          PM.FLOAT32)


def test_a_member_above_the_modes_limit(no_native):
    with pytest.raises(ValueError, match=r"member 1 has N = 3073, above the limit of 3072 for torch.float32 state"):
        nb.RaggedEnsemble(*state([16, 3073]), PM.FLOAT32)
    with pytest.raises(ValueError, match=r"member 0 has N = 3073, above the limit of 3072"):
        nb.RaggedEnsemble(*state([3073, 16]), [PM.FLOAT32, PM.BFLOAT16])
    with pytest.raises(ValueError, match=r"member 2 has N = 4097, above the limit of 4096 for torch.float64 state"):
        nb.RaggedEnsemble(*state([16, 3073, 4097], 2, torch.float64), PM.FLOAT64)


def test_wrong_dtype(no_native):
    p, v, m = state([8, 9])
    with pytest.raises(TypeError, match=r"positions\[0\] must be torch.float64 under FLOAT64 \(got torch.float32\)"):
        nb.RaggedEnsemble(p, v, m)
    with pytest.raises(TypeError, match=r"velocities\[1\] must be torch.float32 under BFLOAT16 \(got torch.float64\)"):
        nb.RaggedEnsemble(p, [v[0], v[1].double()], m, PM.BFLOAT16)
    with pytest.raises(TypeError, match=r"masses\[0\] must be torch.float32 under FLOAT32 \(got torch.float16\)"):
        nb.RaggedEnsemble(p, v, [m[0].half(), m[1]], [PM.FLOAT32, PM.FLOAT16])
    with pytest.raises(TypeError, match="precision_mode must be a PrecisionMode or a list of them, got str"):
        nb.RaggedEnsemble(p, v, m, "float32")


def test_grid_modes_and_float64_in_a_list(no_native):
    p, v, m = state([8, 9])
    for mode in (PM.INT8_SIM, PM.INT4_SIM, PM.CUSTOM):
        with pytest.raises(ValueError, match=f"{mode.name} needs per-member quantisation tables .the ragged grid modes are a follow-up"):
            nb.RaggedEnsemble(p, v, m, mode)
    with pytest.raises(ValueError, match=r"precision_mode\[1\] = INT8_SIM: a grid mode"):
        nb.RaggedEnsemble(p, v, m, [PM.FLOAT32, PM.INT8_SIM])
    with pytest.raises(ValueError, match=r"precision_mode\[0\] = FLOAT64 beside other modes"):
        nb.RaggedEnsemble(p, v, m, [PM.FLOAT64, PM.FLOAT32])


def test_a_baseline_of_another_size_and_the_follow_ups_need_no_library(no_native):
    e = bare([700, 700, 37, 37])
    e._same_size_baselines([0, 0, 2, 2])
    e._same_size_baselines([1, 0, 3, 2])
    with pytest.raises(ValueError, match="baseline of member 2 is member 0: 37 stars against 700"):
        e.divergence(0)
    with pytest.raises(ValueError, match="baseline of member 1 is member 3: 700 stars against 37"):
        e.run_diverged(5, 1, [0, 3, 2, 2])
    with pytest.raises(ValueError, match="baseline must name a member"):
        e.divergence(4)
    for call, what in ((lambda: e.metrics(num_bins=8), "ragged metrics"), (lambda: e.run_crash_watched(5), "ragged crash watch"),
                       (lambda: e.crash_measures(), "ragged crash watch")):
        with pytest.raises(NotImplementedError, match=f"{what} .* follow-up"):
            call()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_gpu_means_loud_failure_not_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nb.RaggedEnsemble(*state([16, 300, 5]), PM.FLOAT32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nb.RaggedEnsemble(*state([16, 300, 5]), [PM.FLOAT32, PM.FLOAT16, PM.BFLOAT16])


def test_the_c_abi_refuses_bad_arguments_before_it_looks_for_a_device():
    """nb_ens_create_ragged: null arguments, members = 0, a size of 0 or above cfg->n are invalid (-1, the member named); a
    grid mode, a mode list beside any cfg->mode but FLOAT32, a bad list entry and a capacity above the mode's limit are
    unsupported (-5)."""
    lib = _native.lib()
    F64, F32, F16, INT8, INT4, CUSTOM = 0, 1, 3, 4, 5, 6

    def create(mode, sizes, n=64, members=None, modes=None, null=None):
        members = len(sizes) if members is None else members
        h = C.c_void_p()
        cfg = _native.NbEnsConfig(members=members, n=n, dim=2, mode=mode, device=0, flags=0)
        par = [(C.c_double * max(members, 1))(*([0.01] * max(members, 1))) for _ in range(3)]
        args = [C.byref(h), C.byref(cfg), (C.c_int32 * len(sizes))(*sizes), (C.c_int32 * len(modes))(*modes) if modes else None,
                *par]
        if null is not None:
            args[null] = None
        rc = lib.nb_ens_create_ragged(*args)
        assert rc != 0 and not h.value
        return rc, lib.nb_last_error().decode()

    for null in (0, 1, 2, 4, 5, 6):
        rc, msg = create(F32, [8, 9], null=null)
        assert rc == -1 and "null argument" in msg, (null, rc, msg)
    rc, msg = create(F32, [8], members=0)
    assert rc == -1 and "members" in msg, (rc, msg)
    rc, msg = create(F32, [8, 0, 9])
    assert rc == -1 and "sizes[1] = 0" in msg and "member 1" in msg, (rc, msg)
    rc, msg = create(F64, [8, 9, 65])
    assert rc == -1 and "sizes[2] = 65" in msg and "[1, 64]" in msg and "member 2" in msg, (rc, msg)
    for mode in (INT8, INT4, CUSTOM):
        rc, msg = create(mode, [8, 9])
        assert rc == -5 and "ragged grid modes" in msg, (mode, rc, msg)
    rc, msg = create(F16, [8, 9], modes=[F32, F16])
    assert rc == -5 and "NB_FLOAT32" in msg, (rc, msg)
    rc, msg = create(F32, [8, 9], modes=[F32, F64])
    assert rc == -5 and "modes[1]" in msg, (rc, msg)
    rc, msg = create(F32, [8, 3073], n=3073)
    assert rc == -5 and "3072" in msg, (rc, msg)
    rc, msg = create(F64, [8, 4097], n=4097)
    assert rc == -5 and "4096" in msg, (rc, msg)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_the_c_abi_fails_loudly_without_a_device():
    lib = _native.lib()
    h = C.c_void_p()
    cfg = _native.NbEnsConfig(members=2, n=9, dim=2, mode=1, device=0, flags=0)
    par = [(C.c_double * 2)(0.01, 0.01) for _ in range(3)]
    rc = lib.nb_ens_create_ragged(C.byref(h), C.byref(cfg), (C.c_int32 * 2)(8, 9), None, *par)
    assert rc == -2 and not h.value and "no CPU fallback" in lib.nb_last_error().decode()


# ---- the planner: no device ------------------------------------------------------------------------------------------------
def plan(sizes, lanes, capacity=None, ask=False):
    lib = _native.lib()
    items = C.c_int64(-1)
    arr = (C.c_int32 * len(sizes))(*sizes)
    if ask:
        rc = lib.nb_ens_ragged_plan(arr, len(sizes), lanes, None, 0, C.byref(items))
        return rc, items.value, None
    capacity = 4096 if capacity is None else capacity
    work = (C.c_int32 * (2 * max(capacity, 1)))(*([-7] * (2 * max(capacity, 1))))
    rc = lib.nb_ens_ragged_plan(arr, len(sizes), lanes, work, capacity, C.byref(items))
    return rc, items.value, list(work)


@pytest.mark.parametrize("sizes,lanes", [([37, 700, 1025, 2049, 2, 64, 8, 9], 64), ([257, 5, 2049], 16), ([257, 5, 2049], 32)],
                         ids=["eight-lanes64", "three-lanes16", "three-lanes32"])
def test_the_work_list(sizes, lanes):
    targets = 512 // lanes
    want_items = sum(-(-n // targets) for n in sizes)
    rc, items, _ = plan(sizes, lanes, ask=True)                    # a NULL list asks for the count
    assert rc == 0 and items == want_items
    rc, items, work = plan(sizes, lanes)
    assert rc == 0 and items == want_items
    got = [(work[2 * w], work[2 * w + 1]) for w in range(items)]
    assert all(x == -7 for x in work[2 * items:]), "wrote past the list"
    # every (member, blk) with blk * targets < n_b exactly once, and nothing else
    want = {(b, blk) for b, n in enumerate(sizes) for blk in range(-(-n // targets))}
    assert len(got) == len(set(got)) and set(got) == want
    assert all(blk * targets < sizes[b] for b, blk in got)
    # members by size descending, ties by index; blk ascending within a member
    order = sorted(range(len(sizes)), key=lambda b: (-sizes[b], b))
    assert got == [(b, blk) for b in order for blk in range(-(-sizes[b] // targets))]
    # exactly enough room is enough; one item less is refused and nothing is written
    rc, items, work = plan(sizes, lanes, capacity=want_items)
    assert rc == 0 and items == want_items
    rc, items, work = plan(sizes, lanes, capacity=want_items - 1)
    assert rc == -1 and items == want_items and "capacity" in _native.last_error() and all(x == -7 for x in work)


def test_the_work_list_keeps_ties_in_member_order():
    rc, items, work = plan([9, 700, 9, 700, 8], 64)
    assert rc == 0 and items == 2 + 88 + 2 + 88 + 1
    members = [work[2 * w] for w in range(items)]
    assert members == [1] * 88 + [3] * 88 + [0] * 2 + [2] * 2 + [4]


def test_the_planner_refuses_bad_arguments():
    lib = _native.lib()
    items = C.c_int64()
    one = (C.c_int32 * 1)(8)
    assert lib.nb_ens_ragged_plan(None, 1, 64, None, 0, C.byref(items)) == -1
    assert lib.nb_ens_ragged_plan(one, 1, 64, None, 0, None) == -1
    for lanes in (0, 8, 48, 128):
        assert lib.nb_ens_ragged_plan(one, 1, lanes, None, 0, C.byref(items)) == -1 and "lanes" in _native.last_error()
    assert lib.nb_ens_ragged_plan(one, 0, 64, None, 0, C.byref(items)) == -1
    assert lib.nb_ens_ragged_plan(one, 1025, 64, None, 0, C.byref(items)) == -1
    rc, _, _ = plan([8, 0, 9], 64, ask=True)
    assert rc == -1 and "sizes[1] = 0" in _native.last_error()
