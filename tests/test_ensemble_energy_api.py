"""The ensemble's batched energies without a GPU: the exports, the sample offsets of run_recorded, its argument errors
(all raised in Python, before any native call), the byte cap of a history, and EnergyHistory.total."""
import pytest
import torch

import nbody_cosmological_simulation_amd as nb
from nbody_cosmological_simulation_amd import _native, ensemble


@pytest.fixture
def no_native(monkeypatch):
    """Any native call fails the test: argument errors must be raised before the library is reached."""
    def boom():
        raise AssertionError("the native library was reached before the arguments were checked")
    monkeypatch.setattr(_native, "lib", boom)


def bare(members, tick=0):
    """A GalaxyEnsemble without a native handle: enough for the checks run_recorded makes before its native call."""
    e = object.__new__(nb.GalaxyEnsemble)
    e._handle = None
    e.num_members, e.tick, e.device = members, tick, torch.device("cpu")
    return e


def test_exports():
    for name in ("EnergyHistory", "check_record_arguments"):
        assert name in nb.__all__ and getattr(nb, name) is getattr(ensemble, name), name
    for name in ("run_recorded", "energies"):
        assert callable(getattr(nb.GalaxyEnsemble, name)), name
    assert ensemble.MAX_HISTORY_BYTES == 256 << 20
    for name in ("nb_ens_energies", "nb_ens_run_recorded"):
        assert name in _native.EXPORTS, name
    assert "run_recorded" in ensemble.__doc__ and "energies()" in ensemble.__doc__


def test_sample_offsets(no_native):
    assert nb.check_record_arguments(5, 2, 5) == [0, 2, 4]
    assert nb.check_record_arguments(0, 3, 5) == [0]
    assert nb.check_record_arguments(3, 7, 5) == [0]
    assert nb.check_record_arguments(6, 1, 1) == [0, 1, 2, 3, 4, 5, 6]
    assert nb.check_record_arguments(6, 3, 1024) == [0, 3, 6]


@pytest.mark.parametrize("call", ["function", "method"])
def test_argument_errors_are_raised_before_the_native_call(no_native, call):
    if call == "function":
        f = lambda num_ticks, every=1: nb.check_record_arguments(num_ticks, every, 4)
    else:
        f = lambda num_ticks, every=1: bare(4).run_recorded(num_ticks, every)
    for bad in (2.0, "3", None, True):
        with pytest.raises(TypeError, match="num_ticks must be an int"):
            f(bad)
        with pytest.raises(TypeError, match="every must be an int"):
            f(4, bad)
    with pytest.raises(ValueError, match="num_ticks must be >= 0"):
        f(-1)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="every must be >= 1"):
            f(4, bad)
    with pytest.raises(TypeError, match="members must be an int"):
        nb.check_record_arguments(4, 1, 2.0)
    with pytest.raises(TypeError, match="members must be an int"):
        nb.check_record_arguments(4, 1, False)


def test_history_byte_cap(no_native):
    # 16 bytes per member and sample: B = 1024 members fill 256 MiB with 16384 samples = 16383 ticks at every = 1
    assert len(nb.check_record_arguments(16383, 1, 1024)) == 16384
    with pytest.raises(ValueError, match="raise `every`"):
        nb.check_record_arguments(16384, 1, 1024)
    with pytest.raises(ValueError, match="raise `every`"):
        bare(1024).run_recorded(16384)
    assert len(nb.check_record_arguments(16384, 2, 1024)) == 8193
    e = bare(1024, tick=7)
    with pytest.raises(ValueError):
        e.run_recorded(16384, every=1)
    assert e.tick == 7                                   # a refused call advances nothing


def test_energy_history_total():
    ke = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=torch.float64)
    pe = torch.tensor([[-4.0, -3.0], [-2.0, -1.0], [0.5, float("nan")]], dtype=torch.float64)
    h = nb.EnergyHistory([3, 5, 7], ke, pe)
    assert h.ticks == [3, 5, 7] and h.kinetic is ke and h.potential is pe
    tot = h.total
    assert tot.dtype == torch.float64 and tot.shape == (3, 2)
    assert torch.equal(tot[:2], torch.tensor([[-3.0, -1.0], [1.0, 3.0]], dtype=torch.float64))
    assert tot[2, 0].item() == 5.5 and torch.isnan(tot[2, 1])
    ticks, kinetic, potential = h                        # still a plain tuple of its three fields
    assert ticks == [3, 5, 7] and kinetic is ke and potential is pe
