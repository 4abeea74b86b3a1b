"""The tensor-level precision hooks (quantize_distance_squared, quantize_force, _grid_quantize, _grid_quantize_safe:
csrc/nb_hooks.cpp, the min/max, cast and quantise kernels of csrc/nb_misc.hip, grid_quantize_safe_tab_kernel of
csrc/nb_grid.hip) element by element.

The max-norm bars of test_gpu_parity.py cannot see a small element that lands in the wrong bin next to a maximum of
5e4.  Here every element is compared:

  fp32, all hooks     bit-identical to the oracle (uint32 views, NaN == NaN, the sign of zero counts).  The log grid
                      may skip the near-tie elements of hook_cases.log32_mask; none is expected.
  linear grid         fp32 and fp64 also bit-identical to the reference formula in torch CPU ops; nothing skipped.
  log grid, fp64      bin equality with the oracle (bin = nearest oracle level) outside DELTA of a half-integer
                      coordinate, and each value within REL of the oracle's; both bounds are derived in hook_cases.py
                      from the 1 ulp the device library documents for double log and exp.
                      REL = 5 * 1.5 ulp(max|l|) + 1.5 * 2^-52: 3.3e-16 for the narrow cases, 7.0e-15 for max|l| in
                      [4, 8), 1.4e-14 for seven decades above 0.01, 1.1e-13 above 1e-30, 8.5e-13 with a maximum of 1e300.
  casts               torch CPU's own .double() / .float() / .bfloat16().float() / .half().float(), bit for bit.

Counts walk over every ceiling in the launch code: the block sizes, 2^21 (library-call path below, table path from
there on; stage 1 of the min/max stops adding blocks), 2^22 (second grid-stride pass of the element-wise kernels,
second unrolled trip of stage 1, fifth pass of the table kernel).  The unique extremum, a NaN and the infinities are
put at every place a reduction could drop (hook_cases.placements).  Every value case runs from host and from device
memory and must give the same bits; inputs must come back unchanged.
"""
import numpy as np
import pytest
import torch

import hook_cases as HC
from hook_cases import F32, F64
from oracle import oracle as O
from test_gpu_parity import torch_formula_linear, torch_formula_safe

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEN = {"rel": 0.0, "bound": 0.0, "ratio": 0.0, "skipped32": 0, "skipped64": 0}


@pytest.fixture(scope="module", autouse=True)
def figures():
    """After the module's tests: the figures they saw, and the skip counts asserted.  Every case also asserts its own cap
    (1e-6 of the elements in fp32, 1e-4 in fp64); the inputs are fixed, the expected number of near-tie elements is
    zero, and zero is what must be seen -- a case that loses an element to the mask gets another seed in hook_cases."""
    yield
    print(f"\nhook elements: worst fp64 log-grid relative error {SEEN['rel']:.3e} (bound of that case {SEEN['bound']:.3e}), "
          f"worst error / bound {SEEN['ratio']:.3f}; skipped near-tie elements fp32 {SEEN['skipped32']}, fp64 {SEEN['skipped64']}")
    assert SEEN["skipped32"] == 0 and SEEN["skipped64"] == 0, SEEN
    assert SEEN["ratio"] <= 1.0, SEEN


@pytest.fixture(scope="module")
def nb():
    import nbody_cosmological_simulation_amd as pkg
    assert pkg._native.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return pkg


# ------------------------------------------------------------------------------------------------- comparisons
def _uint(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_bits(got, want, what, bins=None, skip=None):
    """Bit-identical element by element (NaN == NaN); on failure: how many differ, the first index, its oracle bin."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = (_uint(got) != _uint(want)) & ~(np.isnan(got) & np.isnan(want))
    if skip is not None:
        bad &= ~np.asarray(skip).reshape(bad.shape)
    if bad.any():
        idx = np.flatnonzero(bad.ravel())
        i = int(idx[0])
        msg = (f"{what}: {idx.size} of {got.size} elements differ; first at flat index {i}: "
               f"got {got.ravel()[i]!r} ({_uint(got).ravel()[i]:#x}), want {want.ravel()[i]!r} ({_uint(want).ravel()[i]:#x})")
        if callable(bins):
            bins = bins()
        if bins is not None:
            msg += f"; oracle bins of the first differing elements: {np.asarray(bins).ravel()[idx[:10]].tolist()}"
        raise AssertionError(msg)


def same_bits_t(got, want):
    """The same comparison on torch tensors of one device (the large placement loops stay on the GPU)."""
    iv = torch.int32 if got.dtype == torch.float32 else torch.int64
    return bool(((got.view(iv) == want.view(iv)) | (got.isnan() & want.isnan())).all())


def check_log64(got, ref, what):
    """fp64 log grid against hook_cases.log64_expect: got is a flat torch tensor on either device."""
    if ref["passthrough"]:
        assert_bits(got.cpu().numpy(), ref["out"], what + " (pass-through)")
        return
    d = got.device
    key = ("t", str(d))
    if key not in ref:
        lv = torch.from_numpy(ref["level_values"]).to(d)
        ref[key] = {"mids": (lv[1:] + lv[:-1]) / 2, "bins": torch.from_numpy(ref["bins"]).to(d),
                    "out": torch.from_numpy(ref["out"]).to(d), "skip": torch.from_numpy(ref["skip"]).to(d)}
    r = ref[key]
    gbin = torch.bucketize(got, r["mids"])
    bad = (gbin != r["bins"]) & ~r["skip"]
    rel = (got - r["out"]).abs() / r["out"]
    badv = ~(rel <= ref["rel_bound"])
    worst = float(rel[~badv].max()) if bool((~badv).any()) else 0.0
    if worst > SEEN["rel"]:
        SEEN["rel"], SEEN["bound"] = worst, ref["rel_bound"]
    SEEN["ratio"] = max(SEEN["ratio"], worst / ref["rel_bound"])
    SEEN["skipped64"] += int(r["skip"].sum())
    if bool(bad.any()) or bool(badv.any()):
        ib, iv = torch.nonzero(bad).ravel(), torch.nonzero(badv).ravel()
        i = int(ib[0]) if ib.numel() else int(iv[0])
        raise AssertionError(
            f"{what}: {ib.numel()} of {got.numel()} elements in another bin than the oracle's, {iv.numel()} beyond "
            f"{ref['rel_bound']:.3e} of its value; first at flat index {i}: got {float(got[i])!r} (bin {int(gbin[i])}), "
            f"want {float(r['out'][i])!r} (bin {int(r['bins'][i])}), rel {float(rel[i]):.3e}; oracle bins of the first: "
            f"{r['bins'][ib[:10]].tolist()}")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def both(fn, x, what):
    """fn on the tensor in host memory and in device memory: the same bits, the inputs bitwise unchanged."""
    th, keep = T(x), np.array(x, copy=True)
    td = th.to(DEV)
    out_h = fn(th)
    out_d = fn(td)
    assert out_h.device.type == "cpu" and out_d.device.type == "cuda", what
    assert_bits(out_d.cpu().numpy(), out_h.numpy(), what + ": device against host staging")
    assert_bits(th.numpy(), keep, what + ": host input modified")
    assert_bits(td.cpu().numpy(), keep, what + ": device input modified")
    return out_h.numpy()


def check_safe(nb, x, levels, min_val, what, fn=None):
    """_grid_quantize_safe (or fn) on x from both memories against the oracle, by the rule of x's dtype."""
    fn = fn or (lambda t: nb._grid_quantize_safe(t, levels, min_val=min_val))
    what = f"{what} L={levels} min_val={min_val:g} {x.dtype} n={x.size}"
    got = both(fn, x, what)
    if x.dtype == F32:
        ref, bins, _, _ = O.grid_quantize_safe(x, levels, min_val, bins=True)
        mask, ok = HC.log32_mask(x, levels, min_val)
        assert ok and mask.sum() <= 1e-6 * x.size, what
        SEEN["skipped32"] += int(mask.sum())
        assert_bits(got, ref, what, bins, mask)
    else:
        check_log64(T(got).ravel(), HC.log64_expect(x, levels, min_val), what)
    return got


def check_linear(nb, x, levels, what, fn=None):
    fn = fn or (lambda t: nb._grid_quantize(t, levels))
    what = f"{what} L={levels} {x.dtype} n={x.size}"
    got = both(fn, x, what)
    ref, bins, _, _ = O.grid_quantize(x, levels, bins=True)
    assert_bits(got, ref, what + " against the oracle", bins)
    with np.errstate(all="ignore"):
        assert_bits(got, torch_formula_linear(x, levels), what + " against torch's CPU ops", bins)
    return got


# ------------------------------------------------------------------------------------------------- counts and levels
@pytest.mark.parametrize("count,dtype", [(n, F32) for n in HC.SMALL_COUNTS] + [(n, F64) for n in HC.F64_COUNTS if n <= 1025],
                         ids=lambda v: str(v))
def test_small_counts(nb, count, dtype):
    for L in (16, 256):
        check_safe(nb, HC.decades(count, dtype, 0.01, L, seed=count), L, 0.01, "decades")
        check_linear(nb, HC.mixed_signs(count, dtype, seed=count), L, "mixed signs")


@pytest.mark.parametrize("levels,dtype", [(L, F32) for L in HC.LEVELS + (HC.ROUNDING_LEVELS,)] + [(L, F64) for L in HC.LEVELS],
                         ids=lambda v: str(v))
def test_levels(nb, levels, dtype):
    """ROUNDING_LEVELS: (float)(levels - 1) rounds, in fp32 only; at a small count."""
    n = 257 if levels == HC.ROUNDING_LEVELS else HC.VALUE_COUNT
    check_safe(nb, HC.decades(n, dtype, 0.01, levels, seed=3), levels, 0.01, "decades")
    check_linear(nb, HC.mixed_signs(n, dtype, seed=3), levels, "mixed signs")


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_log_grid_values(nb, dtype):
    for L in (16, 256):
        for name, x, m in HC.log_value_cases(dtype, levels=L):
            got = check_safe(nb, x, L, m, name)
            mt = dtype.type(m)
            if name in ("all_below_clamp", "constant", "same_log_pair", "log_below_switch"):      # degenerate grid: the clamped input
                assert_bits(got, np.maximum(x, mt), name + ": pass-through")
            if name == "log_above_switch":                               # a log range of 5e-10 is quantised
                assert len(np.unique(got)) <= L < len(np.unique(x))
            if name == "bin0_clamped":
                assert (got[x < mt] == mt).all(), "clamped elements come back as min_val exactly"


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_linear_grid_values(nb, dtype):
    for L in (16, 256):
        for name, x in HC.linear_value_cases(dtype):
            got = check_linear(nb, x, L, name)
            if name.startswith("below_switch") or name == "constant":
                assert_bits(got, x, name + ": pass-through")
            if name.startswith("above_switch"):
                assert not np.array_equal(got, x), name + ": must be quantised"
    # the elements near zero of the wide case, one by one, against the oracle
    x = HC.mixed_signs(HC.VALUE_COUNT, dtype)
    near0 = np.abs(x) < 1.0
    assert near0.sum() > 1000
    got = nb._grid_quantize(T(x), 4096).numpy()
    ref, bins, _, _ = O.grid_quantize(x, 4096, bins=True)
    assert_bits(got[near0], ref[near0], "elements near zero", bins[near0])


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("levels", [17, 257])
def test_linear_half_integer_ties_round_to_even(nb, levels, dtype):
    x, want_bins = HC.ties(levels, dtype)
    got = check_linear(nb, x, levels, "ties")
    want = (want_bins.astype(np.float64) / (levels - 1) * 16.0 - 8.0).astype(dtype)          # exact: powers of two
    assert_bits(got, want, "round half to even", want_bins)


def test_path_switch_at_2_21(nb):
    """2^21 - 1 elements take the library-call path, the same data with one non-extreme element appended the table
    path: the common outputs must be bit-identical to each other and to the oracle."""
    for L in (256, 4096):
        x = HC.decades(HC.SWITCH, F32, 0.01, L, seed=21)
        x[-1] = 1.0
        assert x[:-1].min() < 1.0 < x[:-1].max()
        below = check_safe(nb, x[:-1], L, 0.01, "below the switch")
        at = check_safe(nb, x, L, 0.01, "at the switch")
        assert_bits(at[:-1], below, f"the two paths at the switch, L={L}")
    x = HC.decades(HC.SWITCH, F32, 0.01, 4097, seed=22)
    check_safe(nb, x, 4097, 0.01, "4097 levels: element-wise at 2^21")


def test_values_on_the_table_path(nb):
    n = HC.SWITCH
    for name, x, m in HC.log_value_cases(F32, count=n, levels=64):
        if name.startswith("decades") and m not in (2.0, 1e-30):
            continue
        got = check_safe(nb, x, 64, m, name + " (tables)")
        if name == "every_float_narrow":            # both sides of every threshold, searched (no estimate on so narrow a grid)
            for L in (16, 256, 4096):
                check_safe(nb, x, L, m, name + " (tables)")
        if name in ("all_below_clamp", "constant", "same_log_pair"):
            assert_bits(got, np.maximum(x, np.float32(m)), name + ": pass-through on the table path")
            below = nb._grid_quantize_safe(T(x[:-1]), 64, min_val=m).numpy()
            assert_bits(below, got[:-1], name + ": pass-through on both paths")


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("count", [HC.BIG, HC.HUGE])
def test_large_counts(nb, count, dtype):
    check_safe(nb, HC.decades(count, dtype, 0.01, 256, seed=5), 256, 0.01, "decades")
    check_linear(nb, HC.mixed_signs(count, dtype, seed=5), 256, "mixed signs")


# ------------------------------------------------------------------------------------------------- extremum placement
def _oracle_bins(x0, kind, levels):
    """The oracle's bins of the tensor with the placed element at index 0 (the compared outputs are swapped back)."""
    return (O.grid_quantize if kind == "lin" else O.grid_quantize_safe)(x0, levels, bins=True)[1]


def _swap(t, p):
    if p:
        a, b = t[0].clone(), t[p].clone()
        t[0], t[p] = b, a


@pytest.mark.parametrize("which", ["min", "max"])
@pytest.mark.parametrize("kind", ["lin", "log"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("count", HC.PLACEMENT_COUNTS)
def test_extremum_at_every_place_a_reduction_could_drop(nb, count, dtype, kind, which):
    """The unique extremum at index 0 gives the expected output once (oracle); moving it to p swaps inputs 0 and p and
    therefore outputs 0 and p.  A reduction that loses the element at p changes the bounds and with them most bins.
    fp32 log grid: 256 levels go through the tables (plain min/max) from 2^21 on, 4097 keep the log-clamped min/max."""
    x0 = HC.placed(count, dtype, kind, which)
    xd = T(x0).to(DEV)
    for L in ((256,) if kind == "lin" or dtype == F64 else (256, 4097)):
        if kind == "lin":
            fn = lambda t: nb._grid_quantize(t, L)
            want = T(O.grid_quantize(x0, L)).to(DEV)
            with np.errstate(all="ignore"):
                assert_bits(want.cpu().numpy(), torch_formula_linear(x0, L), "oracle against torch's CPU ops")
            skip = None
        else:
            fn = lambda t: nb._grid_quantize_safe(t, L)
            if dtype == F32:
                want = T(O.grid_quantize_safe(x0, L)).to(DEV)
                mask, ok = HC.log32_mask(x0, L)
                assert ok and mask.sum() <= 1e-6 * count
                SEEN["skipped32"] += int(mask.sum())
                skip = mask
            else:
                ref64 = HC.log64_expect(x0, L)
        for name, p in HC.placements(count).items():
            what = f"{kind} {which} at {name} = {p}, n={count} {dtype} L={L}"
            _swap(xd, p)
            got = fn(xd).clone()
            _swap(xd, p)
            _swap(got, p)
            if kind == "log" and dtype == F64:
                check_log64(got, ref64, what)
            elif not same_bits_t(got, want) or skip is not None and skip.any():
                assert_bits(got.cpu().numpy(), want.cpu().numpy(), what, lambda: _oracle_bins(x0, kind, L), skip)
    assert_bits(xd.cpu().numpy(), x0, "input restored and unmodified")


@pytest.mark.parametrize("special", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("kind", ["lin", "log"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("count", HC.PLACEMENT_COUNTS)
def test_non_finite_at_every_place(nb, count, dtype, kind, special):
    """One NaN, +inf or -inf at the same places; torch's CPU formula says what comes out (NaN everywhere, except that
    the log grid clamps -inf to min_val like any small element)."""
    x0 = HC.placed(count, dtype, kind, "min")
    x0[0] = special
    levels = (256,) if kind == "lin" or dtype == F64 else (256, 4097)
    xd = T(x0).to(DEV)
    for L in levels:
        skip = None
        with np.errstate(all="ignore"):
            want_np = torch_formula_linear(x0, L) if kind == "lin" else torch_formula_safe(x0, L)
        finite_expected = bool(np.isfinite(want_np).all())
        assert finite_expected == (kind == "log" and special == -np.inf)
        if finite_expected and dtype == F64:
            ref64 = HC.log64_expect(x0, L)
        elif finite_expected:
            want_np = O.grid_quantize_safe(x0, L)              # libm against torch's log: the oracle is the fp32 contract
            skip, ok = HC.log32_mask(x0, L)
            assert ok and skip.sum() <= 1e-6 * count
            SEEN["skipped32"] += int(skip.sum())
        want = T(want_np).to(DEV)
        fn = (lambda t: nb._grid_quantize(t, L)) if kind == "lin" else (lambda t: nb._grid_quantize_safe(t, L))
        for name, p in HC.placements(count).items():
            what = f"{kind} {special} at {name} = {p}, n={count} {dtype} L={L}"
            _swap(xd, p)
            got = fn(xd).clone()
            _swap(xd, p)
            _swap(got, p)
            if finite_expected and dtype == F64:
                check_log64(got, ref64, what)
            elif not same_bits_t(got, want):
                assert_bits(got.cpu().numpy(), want_np, what, lambda: _oracle_bins(x0, kind, L), skip)


# ------------------------------------------------------------------------------------------------- casts
CASTS = {"FLOAT64": lambda t: t.double(), "FLOAT32": lambda t: t.float(), "BFLOAT16": lambda t: t.bfloat16().float(),
         "FLOAT16": lambda t: t.half().float()}


@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
@pytest.mark.parametrize("mode", list(CASTS))
def test_cast_modes_bit_for_bit(nb, mode, dtype):
    x = HC.cast_values(dtype)
    pm = nb.PrecisionMode[mode]
    want = CASTS[mode](T(x)).numpy()
    got = both(lambda t: nb.quantize_distance_squared(t, pm), x, f"quantize_distance_squared {mode} from {dtype}")
    assert_bits(got, want, f"quantize_distance_squared {mode} from {dtype}")
    if mode in ("BFLOAT16", "FLOAT16"):
        got = both(lambda t: nb.quantize_force(t, pm), x, f"quantize_force {mode} from {dtype}")
        assert_bits(got, want, f"quantize_force {mode} from {dtype}")
    else:
        for t in (T(x), T(x).to(DEV)):
            assert nb.quantize_force(t, pm) is t, "identity modes return the same tensor object"
    if dtype == F64 and mode == "FLOAT32":
        assert np.isinf(got[x == 1e300]).all()


def test_cast_second_pass(nb):
    """The cast kernel beyond 2^22 elements: every fp16 pattern, tiled."""
    x = np.resize(HC.cast_values(F32), HC.HUGE)
    for mode in ("FLOAT16", "BFLOAT16", "FLOAT64"):
        got = nb.quantize_distance_squared(T(x).to(DEV), nb.PrecisionMode[mode]).cpu().numpy()
        assert_bits(got, CASTS[mode](T(x)).numpy(), f"{mode} at n={x.size}")


# ------------------------------------------------------------------------------------------------- entry points
def test_mode_entry_points_and_custom_default(nb):
    PM = nb.PrecisionMode
    for dtype in (F32, F64):
        d2 = HC.decades(HC.VALUE_COUNT, dtype, 0.01, 64, seed=9)
        f = HC.mixed_signs(HC.VALUE_COUNT, dtype, seed=9)
        for pm, L, kw in ((PM.INT8_SIM, 256, {}), (PM.INT4_SIM, 16, {}), (PM.CUSTOM, 64, {}), (PM.CUSTOM, 64, {"custom_levels": None}),
                          (PM.CUSTOM, 1000, {"custom_levels": 1000})):
            got = check_safe(nb, d2, L, 0.01, f"quantize_distance_squared {pm.value} {kw}", lambda t: nb.quantize_distance_squared(t, pm, **kw))
            if dtype == F32:
                assert_bits(got, O.quantize_distance_squared(d2, pm.value, kw.get("custom_levels")), "the oracle's own entry point")
            got = check_linear(nb, f, L, f"quantize_force {pm.value} {kw}", lambda t: nb.quantize_force(t, pm, **kw))
            assert_bits(got, O.quantize_force(f, pm.value, kw.get("custom_levels")), "the oracle's own entry point")
        check_safe(nb, d2, 256, 0.5, "min_dist_sq", lambda t: nb.quantize_distance_squared(t, PM.INT8_SIM, min_dist_sq=0.5))


# ------------------------------------------------------------------------------------------------- calling conventions
def _views(ndim, size):
    """(name, view) pairs; each view works on a torch tensor and on a numpy array alike."""
    out = [("contiguous", lambda v: v)]
    if ndim == 2:
        out += [("transposed", lambda v: v.T), ("every second row", lambda v: v[::2]), ("every second column", lambda v: v[:, ::2])]
    if ndim == 1 and size > 1:
        out += [("every second", lambda v: v[::2])]
    if ndim == 3:
        out += [("last axis first", lambda v: v.swapaxes(0, 2))]
    return out


@pytest.mark.parametrize("kind", ["lin", "log"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=str)
def test_shapes_and_strides(nb, dtype, kind):
    """1-D, N x N, 3-D, a single element; transposed and strided inputs give the contiguous result in the input's shape,
    from host and from device memory."""
    n_all = 64 * 64
    x = HC.mixed_signs(n_all, dtype, seed=12) if kind == "lin" else HC.decades(n_all, dtype, 0.01, 64, seed=12)
    fn = (lambda t: nb._grid_quantize(t, 64)) if kind == "lin" else (lambda t: nb._grid_quantize_safe(t, 64))
    for shape in ((n_all - 1,), (45, 91), (64, 64), (5, 9, 91), (1,), (1, 1, 1)):
        a = x[:int(np.prod(shape))].reshape(shape)
        for name, view in _views(a.ndim, a.size):
            what = f"{kind} {name} {shape} {dtype}"
            dense = np.ascontiguousarray(view(a))
            for tt in (view(T(a)), view(T(a).to(DEV))):
                keep = tt.clone()
                got = fn(tt)
                assert got.shape == tt.shape and got.dtype == tt.dtype and got.device == tt.device, what
                if kind == "lin":
                    assert_bits(got.cpu().numpy(), O.grid_quantize(dense, 64), what)
                elif dtype == F32:
                    mask, ok = HC.log32_mask(dense, 64)
                    assert ok and not mask.any()
                    assert_bits(got.cpu().numpy(), O.grid_quantize_safe(dense, 64), what)
                else:
                    check_log64(got.contiguous().ravel(), HC.log64_expect(dense, 64), what)
                assert same_bits_t(tt.contiguous(), keep.contiguous()), what + ": input modified"


def test_empty_tensors_make_no_native_call(nb, monkeypatch):
    from nbody_cosmological_simulation_amd import quantization as Q

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"native call {name} for an empty tensor")
    monkeypatch.setattr(Q.N, "lib", lambda: NoCalls())
    PM = nb.PrecisionMode
    for device in ("cpu", DEV):
        for dt in (torch.float32, torch.float64):
            for shape in ((0,), (0, 3), (4, 0, 2)):
                e = torch.empty(shape, dtype=dt, device=device)
                for out, odt in ((nb._grid_quantize(e, 16), dt), (nb._grid_quantize_safe(e, 16), dt),
                                 (nb.quantize_distance_squared(e, PM.FLOAT64), torch.float64),
                                 (nb.quantize_distance_squared(e, PM.FLOAT16), torch.float32),
                                 (nb.quantize_distance_squared(e, PM.INT8_SIM), dt), (nb.quantize_force(e, PM.BFLOAT16), torch.float32),
                                 (nb.quantize_force(e, PM.CUSTOM), dt)):
                    assert out.shape == e.shape and out.dtype == odt and out.device == e.device


def test_scratch_grows_and_is_reused(nb):
    """small host -> 2^22 host -> small host -> device tensor on a side stream: the library's staging buffer grows, is
    kept, and a use on another stream waits for the previous one."""
    small = HC.decades(1025, F32, 0.01, 64, seed=30)
    large = HC.decades(1 << 22, F32, 0.01, 64, seed=31)
    ref_small, ref_large = O.grid_quantize_safe(small, 64), O.grid_quantize_safe(large, 64)
    mask, ok = HC.log32_mask(large, 64)
    assert ok and mask.sum() <= 4
    assert_bits(nb._grid_quantize_safe(T(small), 64).numpy(), ref_small, "small, first")
    assert_bits(nb._grid_quantize_safe(T(large), 64).numpy(), ref_large, "2^22 from the host", skip=mask)
    assert_bits(nb._grid_quantize_safe(T(small), 64).numpy(), ref_small, "small, after the large one")
    lin = HC.mixed_signs(1 << 22, F32, seed=31)
    assert_bits(nb._grid_quantize(T(lin), 64).numpy(), O.grid_quantize(lin, 64), "linear 2^22 from the host")
    side = torch.cuda.Stream(device=DEV)
    xd = T(large).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        got = nb._grid_quantize_safe(xd, 64)
        got_small = nb._grid_quantize_safe(T(small).to(DEV, non_blocking=False), 64)
    side.synchronize()
    assert_bits(got.cpu().numpy(), ref_large, "device tensor on a side stream", skip=mask)
    assert_bits(got_small.cpu().numpy(), ref_small, "small device tensor on a side stream")
    assert_bits(nb._grid_quantize_safe(T(small), 64).numpy(), ref_small, "small from the host, after the side stream")
