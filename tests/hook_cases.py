"""Inputs of the element-by-element tests of the tensor-level precision hooks (tests/test_gpu_hooks_elements.py) and the
CPU checks of their preconditions (tests/test_oracle_golden.py).  Pure numpy, deterministic, seeded.

What may be skipped, and why (every mask is computed from the reference alone):

  fp32 log grid   The kernels and the oracle evaluate (float)log((double)v) and (float)exp((double)x) with different
                  double libraries.  Both are good to about one double ulp, so the two float results can differ only
                  where the double value lies within 2 double ulps of the midpoint between two adjacent floats.  Such
                  elements (about 1.5e-8 of random data) are masked; a case whose clamped minimum or maximum is such a
                  value is rejected and the next seed taken.  Cap: 1e-6 of a case.
  fp64 log grid   The outputs are compared by bin, and the bin is rint() of the normalised coordinate
                  n = (l - lmin) / (lmax - lmin) * (L - 1).  An element is skipped if n is within DELTA of k + 1/2
                  (log64_delta below).  Cap: 1e-4 of a case.
  linear grid     nothing: only IEEE add, sub, mul, div, round, min and max are involved.

The placement indices MIRROR nb_launch_minmax_generic and ew_grid (csrc/nb_misc.hip) and
nb_launch_grid_quantize_safe_tab (csrc/nb_grid.hip); test_oracle_golden.py reads the constants out of those sources,
so a change of the launch shape shows up as a failing precondition test and not as a placement that silently tests
nothing.
"""
import numpy as np

from oracle import oracle as O

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)

# ---------------------------------------------------------------------------------------------- launch arithmetic
MM_BLOCKS = 2048                    # NB_MINMAX_BLOCKS: stage 1 stops adding blocks here
MM_THREADS = 256
MM_PER_BLOCK = 1024                 # blocks = ceil(count / 1024): at least four elements per thread
MM_UNROLL = 4
EW_BLOCKS, EW_THREADS = 2048 * 8, 256
EW_PASS = EW_BLOCKS * EW_THREADS    # 2^22 elements per grid-stride pass of the element-wise kernels
TAB_PASS = 4096 * 256               # 2^20 elements per pass of grid_quantize_safe_tab_kernel
TABLE_FROM = 1 << 21                # fp32 _grid_quantize_safe goes through tables from this count on ...
MAX_LUT = 4096                      # ... for up to this many levels
PASSTHROUGH = 1e-10

SMALL_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
SWITCH = TABLE_FROM
BIG = (1 << 21) + 3
HUGE = (1 << 22) + 257
F64_COUNTS = (1, 257, 1025, BIG, HUGE)
PLACEMENT_COUNTS = (1025, BIG, HUGE)
LEVELS = (2, 3, 16, 255, 256, 257, 4096, 4097)
ROUNDING_LEVELS = 16777218          # (float)(levels - 1) rounds to 2^24
VALUE_COUNT = 4097                  # the value cases: more than one block, no multiple of anything
MIN_VALS = (0.01, 0.5, 2.0, 1e-30)


def mm_shape(count):
    """(blocks, stride) of minmax_stage1_kernel."""
    blocks = min(max((count + MM_PER_BLOCK - 1) // MM_PER_BLOCK, 1), MM_BLOCKS)
    return blocks, blocks * MM_THREADS


def mm_owner(count, idx):
    """Who reads element idx in stage 1 of the plain min/max: thread g of the grid reads g, g + stride, ...; its first
    4 * (n_g // 4) elements go through the unrolled body (slot = position among the four loads), the rest through the
    tail loop.  (The log-clamped variant has no unrolled body: everything is tail.)"""
    blocks, stride = mm_shape(count)
    idx = np.asarray(idx, np.int64)
    g, q = idx % stride, idx // stride
    n_g = (count - g + stride - 1) // stride
    unrolled = q < MM_UNROLL * (n_g // MM_UNROLL)
    return {"block": g // MM_THREADS, "trip": q, "unrolled": unrolled, "slot": np.where(unrolled, q % MM_UNROLL, -1),
            "last_of_thread": q == n_g - 1}


def placements(count):
    """name -> index at which the extremum is put.  Names whose place does not exist at this count are left out
    (1025 elements: two blocks, no unrolled trip, one pass), and so are names that fall on an index already listed."""
    blocks, _ = mm_shape(count)
    own = mm_owner(count, np.arange(count))
    want = [("first", 0), ("i255", 255), ("i256", 256), ("last", count - 1), ("last_but_one", count - 2)]
    un = np.flatnonzero(own["unrolled"])
    if un.size:
        want.append(("unrolled_last", int(un[-1])))           # its slot is the fourth load, v3
    want.append(("tail_first", int(np.flatnonzero(~own["unrolled"])[0])))
    if blocks > 257:
        want.append(("block257", 257 * MM_THREADS + 17))      # stage 2 reads partial 257 on thread 1's second trip
    if count > EW_PASS + 100:
        want.append(("second_pass", EW_PASS + 100))
    out, seen = {}, set()
    for name, i in want:
        if 0 <= i < count and i not in seen:
            out[name] = i
            seen.add(i)
    return out


# ---------------------------------------------------------------------------------------------- fp32 log-grid mask
def near_f32_midpoint(y):
    """y (float64) lies within 2 double ulps of the midpoint between two adjacent float32 values."""
    y = np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        f = y.astype(np.float32)
        up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
        dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
        f = f.astype(np.float64)
        d = np.minimum(np.abs(y - (f + up) / 2), np.abs(y - (f + dn) / 2))
        return np.isfinite(y) & (d <= 2 * np.spacing(np.abs(y)))


def log32_mask(t, levels, min_val=0.01):
    """(mask of elements whose fp32 result may depend on the double library, bounds_ok).  bounds_ok is False when the
    log of the clamped minimum or maximum is itself such a value: every element would depend on it."""
    flat = np.ascontiguousarray(t, np.float32).ravel()
    with np.errstate(all="ignore"):
        x = np.maximum(flat, np.float32(min_val))
        l64 = O.log_f64(x)
        near = near_f32_midpoint(l64)
        lt = l64.astype(np.float32)
        if not np.all(np.isfinite(lt)):
            return np.zeros(t.shape, bool), True          # non-finite cases: torch's formula is the expectation
        lmin, lmax = lt.min(), lt.max()
        bounds_ok = not (near[lt == lmin].any() or near[lt == lmax].any())
        rng = np.float32(lmax - lmin)
        if rng < np.float32(PASSTHROUGH):
            return np.zeros(t.shape, bool), bounds_ok     # pass-through: no log or exp reaches the output
        lm1 = np.float32(levels - 1)
        k = np.rint((lt - lmin) / rng * lm1)
        lv = k / lm1 * rng + lmin
        near |= near_f32_midpoint(O.exp_f64(lv))
    return near.reshape(t.shape), bounds_ok


# ---------------------------------------------------------------------------------------------- fp64 log-grid bounds
# The device library documents 1 ulp for double log and for double exp; glibc's are good to 0.5 ulp (and a little:
# 0.52).  A device logarithm therefore differs from the oracle's by at most E = 1.5 ulp(M), M = max(|lmin|, |lmax|).
#   n = (l - lmin) / r * (L - 1), r = lmax - lmin.  With s = (l - lmin) / r in [0, 1]:
#   dn = [dl - (1 - s) dlmin - s dlmax] (L - 1) / r, |dn| <= 2 E (L - 1) / r.  Three logarithms are involved, and each is
#   allowed its full E:
#       DELTA = 3 E (L - 1) / r
#   (the third E also covers the roundings of the subtraction, the division and the product wherever M >= r, which
#   holds for every case here but is not needed: no element of any case comes within DELTA of an edge).
# The value: x = fl(fl(fl(k / (L - 1)) * r) + lmin) = (1 - s) lmin + s lmax up to three roundings of numbers <= M on
# either side (3 ulp(M) = 2 E together); the same three logarithms at E each give 3 E.  exp turns an absolute error of
# its argument into a relative one of its value and adds its own 1.5 ulp (1 device + 0.5 glibc), 1.5 * 2^-52 relative:
#       REL = 5 E + 1.5 * 2^-52            (the final clamp moves both sides to the same number or by less than that)
# REL by case: 3.3e-16 for the narrow cases (M <= 1e-4), 7.0e-15 for M in [4, 8), 1.4e-14 for the seven decades above
# 0.01 or 0.5 (M in [8, 16)), 2.7e-14 above 2.0, 1.1e-13 above 1e-30 (M = 69.5), 8.5e-13 with a maximum of 1e300.
def _E(lmin, lmax):
    return 1.5 * float(np.spacing(max(abs(lmin), abs(lmax))))


def log64_delta(lmin, lmax, levels):
    return 3 * _E(lmin, lmax) * (levels - 1) / (lmax - lmin)


def log64_rel_bound(lmin, lmax):
    return 5 * _E(lmin, lmax) + 1.5 * 2.0 ** -52


def log64_expect(t, levels, min_val=0.01):
    """The oracle's answer for an fp64 tensor and what is needed to compare with it: out, bins (-1: pass-through),
    level values, skip mask, relative bound.  Asserts the skip cap."""
    t = np.ascontiguousarray(t, np.float64)
    out, bins, lmin, lmax = O.grid_quantize_safe(t, levels, min_val, bins=True)
    ref = {"out": out.ravel(), "bins": bins.ravel(), "lmin": lmin, "lmax": lmax, "levels": levels,
           "passthrough": bool((bins == -1).all())}
    if ref["passthrough"]:
        ref["skip"] = np.zeros(t.size, bool)
        return ref
    assert not 0.7e-10 < lmax - lmin < 1.5e-10, "an fp64 log case must stay clear of the pass-through switch"
    n = (O.log_f64(np.maximum(t.ravel(), min_val)) - lmin) / (lmax - lmin) * (levels - 1)
    ref["skip"] = np.abs(n - np.floor(n) - 0.5) < log64_delta(lmin, lmax, levels)
    assert ref["skip"].sum() <= 1e-4 * t.size, (int(ref["skip"].sum()), t.size)
    ref["level_values"] = O.exp_f64(np.arange(levels, dtype=np.float64) / (levels - 1) * (lmax - lmin) + lmin)
    ref["rel_bound"] = log64_rel_bound(lmin, lmax)
    return ref


# ---------------------------------------------------------------------------------------------- log-grid values
def _seeded(build, dtype, levels, min_val, first_seed):
    """The first of 20 seeds whose case keeps its bounds off a near-tie and its masked share under the cap (fp32; the
    expected count of masked elements is zero).  fp64 cases assert their cap in log64_expect."""
    for seed in range(first_seed, first_seed + 20):
        x = build(np.random.default_rng(seed)).astype(dtype)
        if dtype == F64:
            return x
        mask, ok = log32_mask(x, levels, min_val)
        if ok and mask.sum() <= 1e-6 * x.size:
            return x
    raise AssertionError("no seed gives a case without near-tie elements")


def decades(count, dtype, min_val=0.01, levels=256, seed=0, top=None):
    """Seven decades, log-uniform, about 3 % of them below min_val; `top`: one element replaced by this maximum."""
    lo = np.log(min_val) - 0.2 * np.log(10.0)

    def build(rng):
        x = np.exp(rng.uniform(lo, lo + 7 * np.log(10.0), count))
        if top is not None and count > 1:
            x[count // 3] = top
        return x
    return _seeded(build, dtype, levels, min_val, 100 * seed + 1)


def clamp_matters_min_val(dtype):
    """A min_val m whose own grid level falls below it: T(exp(T(log(T(m))))) < T(m), so bin 0 -- the clamped elements --
    is lifted back by the clamp after exp."""
    T = dtype.type
    for m in np.linspace(0.011, 3.0, 400):
        mt = T(m)
        lg = T(O.log_f64(np.array([mt]))[0])
        if T(O.exp_f64(np.array([lg]))[0]) < mt and not near_f32_midpoint(O.exp_f64(np.array([lg])))[0]:
            return float(mt)
    raise AssertionError("no such min_val")


def every_float(count, lo=1.0, hi=1.0 + 1e-4):
    """Every float32 in [lo, hi], in order, repeated up to count (from the bottom again).  On the table path this grid
    is too narrow for the bin estimate, so the binary search over the thresholds runs; each threshold is a float of
    this range and so is its predecessor: both sides of every bin edge are present, exactly.  In fp32 the logarithms
    of neighbouring floats differ by 6e-8 or more or not at all, so no fp32 tensor has a log range between 1e-10 and
    1e-9: the switch itself is probed in fp64 (log_below_switch, log_above_switch)."""
    a, b = np.float32(lo).view(np.uint32), np.float32(hi).view(np.uint32)
    return np.resize(np.arange(a, b + 1, dtype=np.uint32).view(np.float32), count)


def log_value_cases(dtype, count=VALUE_COUNT, levels=256):
    """[(name, tensor, min_val)] -- the values of the issue's list, at one count and level count."""
    dtype = np.dtype(dtype)
    cases = [(f"decades_min{m:g}", decades(count, dtype, m, levels, seed=i), m) for i, m in enumerate(MIN_VALS)]
    m = clamp_matters_min_val(dtype)
    x = decades(count, dtype, m, levels, seed=7)
    assert (x < m).sum() >= 1 or count < 64
    cases.append(("bin0_clamped", x, m))
    rng = np.random.default_rng(11)
    cases.append(("all_below_clamp", rng.uniform(1e-5, 1e-3, count).astype(dtype), 0.01))
    cases.append(("constant", np.full(count, 3.0, dtype), 0.01))
    pair = np.where(np.arange(count) % 3 == 1, np.nextafter(dtype.type(1000), dtype.type(2000)), dtype.type(1000)).astype(dtype)
    cases.append(("same_log_pair", pair, 0.01))
    cases.append(("narrow", _seeded(lambda r: 1.0 + 1e-4 * r.random(count), dtype, levels, 0.01, 1300), 0.01))
    if dtype == F32:
        cases.append(("every_float_narrow", every_float(count), 0.01))
        cases.append(("max_1e30", decades(count, dtype, 0.01, levels, seed=14, top=1e30), 0.01))
        cases.append(("max_3e35", decades(count, dtype, 0.01, levels, seed=15, top=3e35), 0.01))
    else:
        cases.append(("max_1e300", decades(count, dtype, 0.01, levels, seed=14, top=1e300), 0.01))
        rng = np.random.default_rng(17)
        for name, width in (("log_below_switch", 0.5e-10), ("log_above_switch", 5e-10)):
            x = 1.0 + width * rng.random(count)
            x[count // 5], x[count // 2] = 1.0, 1.0 + width
            cases.append((name, x, 0.01))
    return cases


# ---------------------------------------------------------------------------------------------- linear-grid values
def mixed_signs(count, dtype, seed=0):
    """Both signs, magnitudes log-uniform over 1e-3 .. 5e4: a negative minimum, a huge maximum, many elements near 0."""
    rng = np.random.default_rng(2000 + seed)
    x = np.exp(rng.uniform(np.log(1e-3), np.log(5e4), count)) * rng.choice([-1.0, 1.0], count)
    return x.astype(dtype)


def ties(levels, dtype, mn=-8.0, rng_=16.0):
    """mn, mn + range and mn + (k + 1/2) / (L - 1) * range for every k: with range and L - 1 powers of two every value
    is exact and every normalised coordinate is exactly k + 1/2."""
    k = np.arange(levels - 1, dtype=np.float64)
    x = np.concatenate([[mn, mn + rng_], mn + (k + 0.5) / (levels - 1) * rng_])
    return x.astype(dtype), np.concatenate([[0, levels - 1], 2 * np.rint((k + 0.5) / 2)]).astype(np.int32)


def tiny_range(dtype, width, base=0.0, count=300):
    """Values spread over [base, base + width]: width just below / above the 1e-10 pass-through switch."""
    rng = np.random.default_rng(31)
    x = base + width * rng.random(count)
    x[5], x[77] = base, base + width
    return x.astype(dtype)


def linear_value_cases(dtype, count=VALUE_COUNT):
    dtype = np.dtype(dtype)
    cases = [("mixed_signs", mixed_signs(count, dtype)), ("constant", np.full(count, -2.5, dtype)),
             ("below_switch", tiny_range(dtype, 0.9e-10)), ("above_switch", tiny_range(dtype, 1.1e-10))]
    if dtype == F64:
        cases += [("below_switch_at_1", tiny_range(dtype, 0.9e-10, 1.0)), ("above_switch_at_1", tiny_range(dtype, 1.1e-10, 1.0))]
    return cases


# ---------------------------------------------------------------------------------------------- extremum placement
def placed(count, dtype, kind, which):
    """A tensor whose unique minimum (which = "min") or maximum ("max") sits at index 0; the tests move it by swapping
    elements 0 and p.  The quantisers are element-wise once the bounds are known and the bounds do not depend on the
    order, so the expected output of the swapped tensor is the swapped expected output (checked on the CPU at the
    smallest count).  kind: "lin" (both signs) or "log" (0.02 .. 1e3, min_val = 0.01 below all of it)."""
    dtype = np.dtype(dtype)

    def build(rng):
        if kind == "lin":
            x = rng.uniform(-1.0, 1.0, count)
            x[0] = -3.0 if which == "min" else 3.0
        else:
            x = np.exp(rng.uniform(np.log(0.02), np.log(1e3), count))
            x[0] = 0.011 if which == "min" else 2e3
        return x
    if kind == "lin":
        x = build(np.random.default_rng(4000 + count % 1000)).astype(dtype)
    else:
        x = _seeded(build, dtype, 4097, 0.01, 4100 + count % 1000)
    assert (x[1:] > x[0]).all() if which == "min" else (x[1:] < x[0]).all()
    return x


# ---------------------------------------------------------------------------------------------- cast values
def _half_family(values32):
    """All given half-type values (as float32), the midpoint of every adjacent finite pair and that midpoint +- one
    float32 ulp."""
    fin = np.unique(values32[np.isfinite(values32)])            # sorted; -0 and +0 fold into one
    mid = ((fin[1:].astype(np.float64) + fin[:-1].astype(np.float64)) / 2)
    mid32 = mid.astype(np.float32)
    assert np.array_equal(mid32.astype(np.float64), mid), "every tie must be a float32"
    with np.errstate(all="ignore"):
        around = [mid32, np.nextafter(mid32, np.float32(np.inf)), np.nextafter(mid32, np.float32(-np.inf))]
    return np.concatenate([values32] + around), mid


EDGE_VALUES = [0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 5.9604645e-8, 2.9802322e-8, 2.9802326e-8,
               6.097555e-5, 6.1035156e-5, 65504.0, 65519.99, 65520.0, 65536.0, -65504.0, -65519.99, -65520.0, 3.3895314e38,
               3.3961775e38, 3.4028235e38, np.inf, -np.inf, np.nan]


def f16_patterns():
    return np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)


def bf16_patterns():
    return (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)


def cast_values(dtype):
    """fp32: every fp16 and bf16 bit pattern, every tie between adjacent finite ones and its float neighbours, and the
    edge values.  fp64: the same, plus the doubles next to every tie -- they round to the tie as floats, and then to
    even, while a direct conversion to the half type would round them away from it -- and 1e300."""
    h, hmid = _half_family(f16_patterns())
    b, bmid = _half_family(bf16_patterns())
    with np.errstate(all="ignore"):
        x32 = np.concatenate([h, b, np.array(EDGE_VALUES, np.float64).astype(np.float32)])
    if np.dtype(dtype) == F32:
        return x32
    ties64 = np.concatenate([hmid, bmid])
    traps = np.concatenate([np.nextafter(ties64, np.inf), np.nextafter(ties64, -np.inf)])
    with np.errstate(invalid="ignore"):                     # signalling NaN patterns
        wide = x32.astype(np.float64)
    return np.concatenate([wide, traps, [1e300, -1e300, 65519.99, 65520.0 - 1e-9, 1e-320, 0.1]])
