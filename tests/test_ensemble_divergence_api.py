"""Per-member mode lists and divergence histories, the parts that need no GPU: the pure argument checks
(`check_mode_list`, `check_divergence_arguments`), the reference's derived quantities (`entropy_bits`, `divergence_rate`)
against the reference's own recorded run (tests/golden/g23_divergence.npz, made by make_divergence_golden.py), and the
methods of a hand-made `DivergenceHistory`."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import ensemble
from nbody_cosmological_simulation_amd.ensemble import (DivergenceHistory, check_divergence_arguments, check_mode_list,
                                                        divergence_rate, entropy_bits)

M = nb.PrecisionMode
CAST = [M.FLOAT32, M.BFLOAT16, M.FLOAT16]
GRID = [M.INT8_SIM, M.INT4_SIM, M.CUSTOM]


def test_the_names_are_exported():
    for name in ("Divergence", "DivergenceHistory", "check_mode_list", "check_divergence_arguments", "entropy_bits",
                 "divergence_rate"):
        assert name in nb.__all__ and getattr(nb, name) is getattr(ensemble, name), name
    from nbody_cosmological_simulation_amd import _native
    for name in ("nb_ens_create_mixed", "nb_ens_divergence", "nb_ens_run_diverged"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    for name in ("divergence", "run_diverged"):
        assert callable(getattr(nb.GalaxyEnsemble, name)) and callable(getattr(nb.QuantizedEnsemble, name))


# ---- check_mode_list ---------------------------------------------------------------------------------------------------
def test_mode_list_accepts_the_cast_modes_in_any_order():
    import itertools
    for order in itertools.permutations(CAST):
        assert check_mode_list(list(order), 3) == list(order)
    modes = [M.FLOAT32, M.BFLOAT16, M.FLOAT16, M.FLOAT32, M.FLOAT16]
    assert check_mode_list(modes, 5) == modes and check_mode_list(tuple(modes)) == modes


def test_an_all_equal_list_is_the_uniform_mode():
    for m in CAST + [M.FLOAT64]:
        assert check_mode_list([m] * 4, 4) == [m] * 4
        assert check_mode_list([m], 1) == [m]


def test_mode_list_rejects_float64_beside_other_modes():
    for other in CAST:
        for modes in ([M.FLOAT64, other], [other, other, M.FLOAT64]):
            with pytest.raises(ValueError, match="storage type"):
                check_mode_list(modes, len(modes))


def test_mode_list_rejects_the_grid_modes():
    for g in GRID:
        for modes in ([M.FLOAT32, g], [g, M.FLOAT16, M.FLOAT32], [g, g]):
            with pytest.raises(ValueError, match="per-member quantisation tables.*QuantizedEnsemble"):
                check_mode_list(modes, len(modes))


def test_mode_list_rejects_a_wrong_length_and_wrong_types():
    with pytest.raises(ValueError, match="2 entries for 3 members"):
        check_mode_list([M.FLOAT32, M.FLOAT16], 3)
    with pytest.raises(ValueError, match="4 entries for 3 members"):
        check_mode_list([M.FLOAT32] * 4, 3)
    with pytest.raises(ValueError):
        check_mode_list([], None)
    with pytest.raises(TypeError):
        check_mode_list([M.FLOAT32, "float16"], 2)
    with pytest.raises(TypeError):
        check_mode_list(M.FLOAT32, 1)


def test_the_constructor_checks_the_list_before_it_touches_a_device():
    p, v, m = torch.zeros(3, 8, 2), torch.zeros(3, 8, 2), torch.ones(3, 8)
    with pytest.raises(ValueError, match="storage type"):
        nb.GalaxyEnsemble(p, v, m, precision_mode=[M.FLOAT32, M.FLOAT64, M.FLOAT16])
    with pytest.raises(ValueError, match="QuantizedEnsemble"):
        nb.GalaxyEnsemble(p, v, m, precision_mode=[M.FLOAT32, M.INT8_SIM, M.FLOAT16])
    with pytest.raises(ValueError, match="2 entries for 3 members"):
        nb.GalaxyEnsemble(p, v, m, precision_mode=[M.FLOAT32, M.FLOAT16])
    with pytest.raises(TypeError, match="float32"):        # an all-FLOAT64 list asks for fp64 state, like the scalar mode
        nb.GalaxyEnsemble(p, v, m, precision_mode=[M.FLOAT64] * 3)
    with pytest.raises(TypeError, match="float32"):        # a mixed list asks for fp32 state
        nb.GalaxyEnsemble(p.double(), v.double(), m.double(), precision_mode=[M.FLOAT32, M.FLOAT16, M.FLOAT16])


# ---- check_divergence_arguments ----------------------------------------------------------------------------------------
def test_divergence_arguments_accept_an_int_or_a_list():
    assert check_divergence_arguments(6, 2, 0, 4) == ([0, 0, 0, 0], [0, 2, 4, 6])
    assert check_divergence_arguments(6, 4, 3, 4) == ([3, 3, 3, 3], [0, 4])
    assert check_divergence_arguments(0, 1, [0, 0, 3, 1], 4) == ([0, 0, 3, 1], [0])
    assert check_divergence_arguments(5, 1, (2, 3, 3, 0), 4)[0] == [2, 3, 3, 0]
    assert check_divergence_arguments(5, 1, np.array([2, 3, 3, 0]), 4)[0] == [2, 3, 3, 0]
    assert check_divergence_arguments(5, 1, torch.tensor([1, 1]), 2)[0] == [1, 1]
    assert check_divergence_arguments(5, 7, np.int64(1), 2) == ([1, 1], [0])


def test_divergence_arguments_reject_what_names_no_member():
    for bad in (4, -1, [0, 0, 4, 1], [0, -1, 0, 0]):
        with pytest.raises(ValueError, match="baseline must name a member"):
            check_divergence_arguments(6, 1, bad, 4)
    for bad in ([0, 0, 0], [0] * 5, []):
        with pytest.raises(ValueError, match="entries for 4 members"):
            check_divergence_arguments(6, 1, bad, 4)
    for bad in (0.0, [0, 1.0, 0, 0], True, [0, False, 0, 0], "0", None):
        with pytest.raises(TypeError):
            check_divergence_arguments(6, 1, bad, 4)


def test_divergence_arguments_reject_bad_tick_counts():
    with pytest.raises(ValueError, match="every must be >= 1"):
        check_divergence_arguments(6, 0, 0, 4)
    with pytest.raises(ValueError, match="every must be >= 1"):
        check_divergence_arguments(6, -2, 0, 4)
    with pytest.raises(ValueError, match="num_ticks must be >= 0"):
        check_divergence_arguments(-1, 1, 0, 4)
    with pytest.raises(TypeError):
        check_divergence_arguments(6.0, 1, 0, 4)
    with pytest.raises(TypeError):
        check_divergence_arguments(6, 1.0, 0, 4)


def test_divergence_history_size_is_capped():
    """24 bytes per member and sample under MAX_HISTORY_BYTES: the first sample count over the limit is refused."""
    members = 1024
    fit = ensemble.MAX_HISTORY_BYTES // (ensemble.DIVERGENCE_SAMPLE_BYTES * members)
    assert len(check_divergence_arguments(fit - 1, 1, 0, members)[1]) == fit
    with pytest.raises(ValueError, match="above the limit"):
        check_divergence_arguments(fit, 1, 0, members)
    assert len(check_divergence_arguments(2 * fit - 1, 2, 0, members)[1]) == fit


# ---- the derived quantities against the reference's recorded run -------------------------------------------------------
def test_entropy_bits_and_divergence_rate_equal_the_reference():
    g = load_golden("g23_divergence.npz")
    ab, ac = g["divergence_ab_history"], g["divergence_ac_history"]
    assert ab.shape == ac.shape == (40,)
    series = np.maximum(ab, ac)                         # max(ab, ac) per tick: MultiverseSim.step's max_position_diff
    assert np.array_equal(series, g["max_position_diff"])
    assert (series > 1e-10).any()
    bits, rate = entropy_bits(series), divergence_rate(series)
    assert bits.dtype == rate.dtype == np.float64
    for t in range(40):
        assert bits[t] == g["entropy_bits"][t], t
        assert rate[t] == g["divergence_rate"][t], t
    assert (rate[:11] == 0).all() and (g["divergence_rate"][:11] == 0).all()
    assert (rate[11:] != 0).any()
    # scalars and columns
    assert entropy_bits(float(series[-1])) == g["entropy_bits"][-1] and entropy_bits(1e-10) == 0.0
    assert entropy_bits(float("nan")) == 0.0
    two = divergence_rate(np.stack([series, series[::-1]], axis=1))
    assert two.shape == (40, 2) and np.array_equal(two[:, 0], rate)
    assert np.array_equal(two[:, 1], divergence_rate(series[::-1].copy()))


def test_divergence_rate_edges():
    x = np.full(30, 1e-3)
    x[5] = 0.0                                           # series[i - 10] = 0 at i = 15: not above 1e-15 -> 0
    x[20] = 0.0                                          # series[i - 1] = 0 at i = 21: clamped to 1e-15
    r = divergence_rate(x)
    assert r[15] == 0.0 and r[21] == np.log(1e-15 / 1e-3) / 10
    assert r[11] == 0.0 and r[12] == 0.0                 # log(1) / 10
    assert divergence_rate(np.zeros(0)).shape == (0,) and not divergence_rate(np.ones(11)).any()


# ---- DivergenceHistory -------------------------------------------------------------------------------------------------
def hand_made():
    nan = float("nan")
    mp = torch.tensor([[0.0, 0.0, 0.0],
                       [0.0, 0.02, 0.5],
                       [0.0, nan, 0.25],
                       [0.0, 0.01, nan],
                       [0.0, 0.1, 0.75]], dtype=torch.float64)
    return DivergenceHistory([10, 12, 14, 16, 18], [0, 0, 1], mp, mp / 2, mp * 3, None)


def test_peak_and_butterfly():
    h = hand_made()
    want = np.array([[0.0, 0.0, 0.0], [0.0, 0.02, 0.5], [0.0, 0.02, 0.5], [0.0, 0.02, 0.5], [0.0, 0.1, 0.75]])
    assert np.array_equal(h.peak(), want)                # a NaN sample never replaces the maximum so far (Python's max)
    assert h.butterfly().tolist() == [False, False, True]          # 0.1 is not above 0.1
    assert h.butterfly(0.05).tolist() == [False, True, True]
    assert h.butterfly(threshold=1.0).tolist() == [False, False, False]
    assert h.energy is None and h.ticks == [10, 12, 14, 16, 18] and h.baseline == [0, 0, 1]


def test_history_entropy_and_rate():
    h = hand_made()
    bits = h.entropy_bits()
    assert bits.shape == (5, 3) and bits[0].tolist() == [0.0, 0.0, 0.0]
    assert bits[1, 2] == np.log2(0.5 / 1e-10 + 1) and bits[2, 1] == 0.0
    g = load_golden("g23_divergence.npz")
    series = torch.from_numpy(np.concatenate([[0.0], g["max_position_diff"]]))[:, None]       # the entry sample in front
    long = DivergenceHistory(list(range(41)), [0], series, series, series, None)
    rate = long.divergence_rate()
    assert rate.shape == (41, 1) and rate[0, 0] == 0.0
    assert np.array_equal(rate[1:, 0], g["divergence_rate"])
    assert np.array_equal(long.entropy_bits()[1:, 0], g["entropy_bits"])
