"""Per-member tick budgets and the explosion watch without a GPU: the exports, check_member_ticks_arguments (broadcasting,
length / type / range errors, sample offsets of uneven budgets, the history cap), explosion_reason on a hand-written
table, the argument errors of run_members / run_watched (all raised in Python, before any native call), the lazily derived
member_ticks of a bare object, and the header's declaration of the new entry point."""
import math
import os
import re

import numpy as np
import pytest
import torch

import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import _native, ensemble

from conftest import ROOT

NAN, INF = float("nan"), float("inf")


@pytest.fixture
def no_native(monkeypatch):
    """Any native call fails the test: argument errors must be raised before the library is reached."""
    def boom():
        raise AssertionError("the native library was reached before the arguments were checked")
    monkeypatch.setattr(_native, "lib", boom)


def bare(members, tick=0):
    """A GalaxyEnsemble without a native handle, as the older API tests build it: only these three attributes."""
    e = object.__new__(nb.GalaxyEnsemble)
    e._handle = None
    e.num_members, e.tick, e.device = members, tick, torch.device("cpu")
    return e


def test_exports():
    for name in ("StabilityReport", "check_member_ticks_arguments", "explosion_reason"):
        assert name in nb.__all__ and getattr(nb, name) is getattr(ensemble, name), name
    for name in ("run_members", "run_watched"):
        assert callable(getattr(nb.GalaxyEnsemble, name)), name
        assert getattr(nb.QuantizedEnsemble, name) is getattr(nb.GalaxyEnsemble, name), name
    assert isinstance(nb.GalaxyEnsemble.member_ticks, property)
    assert (ensemble.REASON_NONE, ensemble.REASON_NONFINITE, ensemble.REASON_ENERGY, ensemble.REASON_UNBOUND) == (0, 1, 2, 3)
    assert nb.StabilityReport._fields == ("stable_ticks", "exploded", "reason", "initial_energy", "final_energy", "history")
    assert "nb_ens_run_members" in _native.EXPORTS
    assert "run_members" in ensemble.__doc__ and "run_watched" in ensemble.__doc__
    not_covered = ensemble.__doc__.split("Not covered:")[-1]
    assert "per-member tick counts" not in not_covered


def test_the_header_declares_the_entry_point_with_the_reason_codes():
    text = open(os.path.join(ROOT, "include", "nbody_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+nb_ens_run_members\s*\(([^)]*)\)\s*;", code)
    assert m, "nb_ens_run_members is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["nb_ens *e", "const int32_t *nsteps", "int32_t every", "int32_t watch", "double *kinetic",
                    "double *potential", "int64_t capacity", "int on_device", "int32_t *samples", "int32_t *stop_tick",
                    "int32_t *reason"]
    for name, value in (("NONE", 0), ("NONFINITE", 1), ("ENERGY", 2), ("UNBOUND", 3)):
        assert re.search(rf"#define\s+NB_ENS_REASON_{name}\s+{value}\b", code), name
        assert getattr(ensemble, f"REASON_{name}") == value
    assert re.search(r"#define\s+NB_ABI_VERSION\s+3\b", code)


# ---- check_member_ticks_arguments ---------------------------------------------------------------------------------------------
def test_budgets_are_broadcast_and_converted(no_native):
    f = nb.check_member_ticks_arguments
    assert f(7, None, 3) == ([7, 7, 7], None)
    assert f(0, None, 2) == ([0, 0], None)
    assert f([0, 1, 4, 7, 6], None, 5) == ([0, 1, 4, 7, 6], None)
    assert f((3, 0, 2), None, 3) == ([3, 0, 2], None)
    assert f(range(4), None, 4) == ([0, 1, 2, 3], None)
    assert f(torch.tensor([5, 0, 2]), None, 3) == ([5, 0, 2], None)
    assert f(torch.tensor([5, 0, 2], dtype=torch.int32), None, 3) == ([5, 0, 2], None)
    assert f(torch.tensor(4), None, 2) == ([4, 4], None)
    assert f(np.array([5, 0, 2], np.int16), None, 3) == ([5, 0, 2], None)
    assert f(np.int64(9), None, 2) == ([9, 9], None)
    assert f([np.int32(1), 2], None, 2) == ([1, 2], None)
    budgets, _ = f(np.array([5, 0, 2]), None, 3)
    assert all(type(v) is int for v in budgets)


def test_sample_offsets_follow_the_largest_budget(no_native):
    f = nb.check_member_ticks_arguments
    assert f([0, 1, 4, 7, 6], 1, 5)[1] == list(range(8))
    assert f([0, 1, 4, 7, 6], 2, 5)[1] == [0, 2, 4, 6]
    assert f([0, 1, 4, 7, 6], 3, 5)[1] == [0, 3, 6]
    assert f([3, 0, 2, 5, 5], 5, 5)[1] == [0, 5]
    assert f([3, 0, 2, 5, 5], 6, 5)[1] == [0]
    assert f(0, 1, 4)[1] == [0] and f([0, 0], 4, 2)[1] == [0]
    assert f(5, 2, 5) == ([5] * 5, nb.check_record_arguments(5, 2, 5))       # equal budgets: run_recorded's samples
    assert f(6, np.int64(3), 2)[1] == [0, 3, 6]


@pytest.mark.parametrize("call", ["function", "run_members", "run_watched"])
def test_argument_errors_are_raised_before_the_native_call(no_native, call):
    if call == "function":
        f = lambda num_ticks, every=None: nb.check_member_ticks_arguments(num_ticks, every, 4)
    elif call == "run_members":
        f = lambda num_ticks, every=None: bare(4).run_members(num_ticks, every)
    else:
        f = lambda num_ticks, every=None: bare(4).run_watched(num_ticks, 50 if every is None else every)
    for bad in (2.0, "3", None, True, [1, 2, 3, 4.0], [1, True, 2, 3], torch.tensor([1.0, 2.0, 3.0, 4.0]),
                np.array([1.5, 2, 3, 4]), [1, 2, 3, None], np.float64(3), torch.tensor([True] * 4)):
        with pytest.raises(TypeError, match="num_ticks must be an int or a sequence of ints"):
            f(bad)
    for bad in ([1, 2, 3], [1, 2, 3, 4, 5], [], torch.tensor([1, 2]), np.arange(7)):
        with pytest.raises(ValueError, match="entries for 4 members"):
            f(bad)
    for bad in (-1, [0, 1, -2, 3], torch.tensor([-1, 0, 0, 0])):
        with pytest.raises(ValueError, match="num_ticks must be >= 0"):
            f(bad)
    with pytest.raises(ValueError, match="int32"):
        f([0, 0, 0, 2 ** 31])
    what = "check_interval" if call == "run_watched" else "every"
    for bad in (2.0, "3", True, [2]):
        with pytest.raises(TypeError, match=f"{what} must be"):
            f(4, bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match=f"{what} must be >= 1"):
            f(4, bad)
    if call == "function":
        for bad in (2.0, False, None):
            with pytest.raises(TypeError, match="members must be an int"):
                nb.check_member_ticks_arguments(4, None, bad)
        with pytest.raises(ValueError, match="members must be >= 1"):
            nb.check_member_ticks_arguments(4, None, 0)
    if call == "run_watched":
        with pytest.raises(TypeError, match="check_interval must be an int"):
            bare(4).run_watched(4, None)


def test_history_byte_cap(no_native):
    # 16 bytes per member and sample, counted to the LARGEST budget: B = 1024 members fill 256 MiB with 16384 samples
    uneven = [0] * 1023 + [16383]
    assert len(nb.check_member_ticks_arguments(uneven, 1, 1024)[1]) == 16384
    uneven[-1] = 16384
    with pytest.raises(ValueError, match="raise `every`"):
        nb.check_member_ticks_arguments(uneven, 1, 1024)
    assert nb.check_member_ticks_arguments(uneven, None, 1024) == (uneven, None)      # no samples, no history
    assert len(nb.check_member_ticks_arguments(uneven, 2, 1024)[1]) == 8193
    e = bare(1024, tick=7)
    with pytest.raises(ValueError, match="raise `every`"):
        e.run_members(uneven, every=1)
    # run_watched's budgets are rounded up to whole batches before the cap is applied: 16383 ticks in ones fit, 16384 do not
    with pytest.raises(ValueError, match="raise `every`"):
        e.run_watched(16384, check_interval=1)
    with pytest.raises(ValueError, match="raise `every`"):
        e.run_watched(2 * 16383 + 1, check_interval=2)                       # 16384 batches of 2: 16385 samples
    assert e.tick == 7 and e.member_ticks == [7] * 1024                      # a refused call advances nothing


# ---- member_ticks ---------------------------------------------------------------------------------------------------------------
def test_member_ticks_of_a_bare_object_are_derived_from_the_tick(no_native):
    e = bare(3, tick=11)
    assert e.member_ticks == [11, 11, 11]
    assert "_member_ticks" not in e.__dict__                                   # nothing is stored until an uneven call
    e._advance(4)                                                              # what run / step / run_recorded do
    assert e.tick == 15 and e.member_ticks == [15, 15, 15] and "_member_ticks" not in e.__dict__
    e._advance(7, own=np.array([0, 7, 3], np.int32))                          # what run_members does with the stop ticks
    assert e.tick == 22 and e.member_ticks == [15, 22, 18]
    assert all(type(v) is int for v in e.member_ticks)
    e._advance(2)
    assert e.tick == 24 and e.member_ticks == [17, 24, 20]
    got = e.member_ticks
    got[0] = -1                                                                # a copy: edits are not tracked
    assert e.member_ticks == [17, 24, 20]


# ---- explosion_reason -------------------------------------------------------------------------------------------------------------
NONE, NONFINITE, ENERGY, UNBOUND = 0, 1, 2, 3
TABLE = [
    # (E0, E, finite, reason)                       what the row is about
    (-1.0, -1.0, True, NONE),                     # nothing moved
    (-1.0, -0.5, True, NONE),                     # drift 0.5, still bound
    (-1.0, 1.0, True, NONE),                      # E == |E0| exactly: not above it
    (-1.0, 1.0000001, True, UNBOUND),             # just above: drift 2, far from 10
    (-1.0, 9.0, True, UNBOUND),                   # drift exactly 10: "> 10.0" is false, the third criterion fires
    (-1.0, 9.0000001, True, ENERGY),              # a bound member with drift > 10: ENERGY, not UNBOUND (the order)
    (-2.0, 50.0, True, ENERGY),
    (-1.0, -11.5, True, ENERGY),                  # the energy criterion alone: more bound, never unbound
    (-1.0, -11.0, True, NONE),                    # drift exactly 10 downwards
    (2.0, 2.5, True, NONE),                       # E0 > 0: the third criterion never applies
    (2.0, 21.0, True, NONE),                      # drift 9.5
    (2.0, 23.0, True, ENERGY),                    # E0 > 0, drift 10.5: only the energy criterion can fire
    (2.0, -21.0, True, ENERGY),
    (1e-10, 5.0, True, NONE),                     # |E0| <= 1e-10: no drift test; E0 > 0: no unbound test
    (-1e-10, 5.0, True, UNBOUND),                 # |E0| <= 1e-10: no drift test, but a bound start turned unbound
    (-1e-11, -5.0, True, NONE),
    (0.0, 1e30, True, NONE),
    (1.0000001e-10, 5.0, True, ENERGY),           # just above the threshold: the drift test is back
    (-1.0, NAN, True, NONE),                      # NaN and Inf energies trip nothing by themselves
    (NAN, -1.0, True, NONE),
    (NAN, NAN, True, NONE),
    (INF, 1.0, True, NONE),                       # drift = inf / inf = NaN
    (-INF, 1.0, True, NONE),                      # drift NaN; 1 > inf false
    (-INF, INF, True, NONE),
    (-1.0, INF, True, ENERGY),                    # ... but an infinite drift is a drift
    (-1.0, -INF, True, ENERGY),
    (2.0, INF, True, ENERGY),
    (-1.0, -1.0, False, NONFINITE),               # finite = False wins over everything
    (-1.0, 50.0, False, NONFINITE),
    (-1.0, 5.0, False, NONFINITE),
    (NAN, NAN, False, NONFINITE),
    (0.0, 0.0, False, NONFINITE),
]


@pytest.mark.parametrize("row", TABLE, ids=[f"{i}-E0={r[0]}-E={r[1]}-{'finite' if r[2] else 'nonfinite'}" for i, r in enumerate(TABLE)])
def test_explosion_reason_table(no_native, row):
    e0, e, finite, want = row
    got = nb.explosion_reason(e0, e, finite)
    assert type(got) is int and got == want
    # the reference's detect_explosion (stability_test.py:34-61), written out: any criterion <=> a reason
    ref = (not finite) or (abs(e0) > 1e-10 and abs(e - e0) / abs(e0) > 10.0) or (e0 < 0 and e > abs(e0))
    assert (got != NONE) == ref
    # the same decision for what the device hands back: float64 scalars and 0-d tensors
    assert nb.explosion_reason(np.float64(e0), np.float64(e), np.bool_(finite)) == want
    assert nb.explosion_reason(torch.tensor(e0, dtype=torch.float64), torch.tensor(e, dtype=torch.float64), finite) == want


def test_explosion_reason_covers_every_code():
    assert {r[3] for r in TABLE} == {NONE, NONFINITE, ENERGY, UNBOUND}
    assert not math.isnan(TABLE[0][0])
