"""csrc/pmath.h (the bit-reproducible math shared by host and device) against glibc and against float64.

Round 4: the transcendentals restate the algorithms of glibc's float functions -- what scalar_rgb calls
through enoki's scalar fallbacks -- so that a build of the restatement ON glibc (oracle/liboracle_libm.so) and the build on pmath.h
agree bit for bit.  Checked here:
 (a) pm_log / pm_exp / pm_sincos / pm_cbrt / pm_pow return glibc's bits on 10^6 arguments per function (tools/pmath_vs_glibc.cpp
     runs every fp32 argument: profiles/r04_pmath_vs_glibc.log, all zero);
 (b) the correctly rounded alternatives pm_*_cr (-DPM_CORRECTLY_ROUNDED; also the |x| >= 120 tail of pm_sincos) equal
     float32(f(float64(x))), and how far that is from glibc: its logf / sinf / cosf are 0.8 / 0.56-ulp routines, its cbrtf
     (<= 2.40) a ~1-ulp one.
The glibc identities are properties of glibc 2.28 .. 2.40 (cbrtf: glibc 2.41 ships a correctly rounded one); on another libm
they are skipped, not failed."""
import platform

import numpy as np
import pytest

import tests.oracle_binding as ob

LOG, EXP, SIN, COS, CBRT, POW = range(6)
CR = 6                                         # pm_*_cr = fn + 6
N = 100000


def glibc_version():
    name, ver = platform.libc_ver()
    if name != "glibc":
        return None
    return tuple(int(p) for p in ver.split(".")[:2])


GLIBC = glibc_version()
needs_glibc = pytest.mark.skipif(GLIBC is None or not ((2, 28) <= GLIBC), reason="the float functions restated by pmath.h are glibc >= 2.28's")


def evalf(fn, xs, ys=None, L=None):
    L = L or ob.lib()
    xs = np.ascontiguousarray(xs, np.float32)
    ys = np.zeros_like(xs) if ys is None else np.ascontiguousarray(ys, np.float32)
    out = np.empty_like(xs)
    L.oracle_math_n(fn, xs.size, ob._p(xs), ob._p(ys), ob._p(out))
    return out


def any_normal(rng, n):
    """Positive normal floats, uniform over the bit patterns (every exponent)."""
    return rng.integers(0x00800000, 0x7f800000, n, dtype=np.uint32).view(np.float32)


def arguments(fn, rng, n=N):
    if fn == LOG:      # half in (0, 1) (log(1 - u), medium.cpp:65), half anywhere
        x = np.concatenate([rng.random(n // 2).astype(np.float32), any_normal(rng, n // 2)])
        return x[x > 0], None
    if fn == EXP:      # transmittances exp(-tau), and the whole finite range
        return np.concatenate([-(20 * rng.random(n // 2)), (rng.random(n // 2) * 2 - 1) * 88.7]).astype(np.float32), None
    if fn in (SIN, COS):   # 2 pi u (warp.h), small arguments, the reduce_fast range
        return np.concatenate([2 * np.pi * rng.random(n // 2), (rng.random(n // 4) * 2 - 1) * 119.9,
                               any_normal(rng, n // 4) % np.float32(1.0)]).astype(np.float32), None
    if fn == CBRT:
        x = np.concatenate([rng.random(n // 2).astype(np.float32) * 2 - 1, any_normal(rng, n // 2) * rng.choice(np.float32([-1, 1]), n // 2)])
        return x, None
    x = np.concatenate([(rng.random(n // 2) * 2).astype(np.float32) + np.float32(1e-3), any_normal(rng, n // 2)])
    return x, (rng.random(x.size) * 12 - 6).astype(np.float32)


def ftz(a):
    a = a.copy()
    a[np.abs(a) < np.float32(1.17549435e-38)] = 0
    return a


@needs_glibc
@pytest.mark.parametrize("fn", [LOG, EXP, SIN, COS, CBRT, POW])
def test_same_bits_as_glibc(fn):
    if fn == CBRT and GLIBC > (2, 40):
        pytest.skip("glibc >= 2.41 ships another cbrtf")
    x, y = arguments(fn, np.random.default_rng(100 + fn), 1000000)
    a = evalf(fn, x, y)
    b = ftz(evalf(fn, x, y, ob.lib_libm()))
    differ = a.view(np.uint32) != b.view(np.uint32)
    assert not differ.any(), (int(differ.sum()), x[differ][:5], a[differ][:5], b[differ][:5])


F64 = {LOG: np.log, EXP: np.exp, SIN: np.sin, COS: np.cos, CBRT: np.cbrt}


def cr_arguments(fn, rng):
    x, y = arguments(fn, rng)
    if fn in (SIN, COS):
        x = np.concatenate([x, ((rng.random(N // 4) * 2 - 1) * 1e4).astype(np.float32)])   # the |x| >= 120 tail of pm_sincos
    return x, y


@pytest.mark.parametrize("fn", [LOG, EXP, SIN, COS, CBRT, POW])
def test_cr_routines_are_correctly_rounded(fn):
    """numpy's float64 functions are accurate to < 1 ulp of fp64, so their rounding to fp32 is the correctly rounded value except
    within ~2^-28 ulp of a rounding boundary."""
    x, y = cr_arguments(fn, np.random.default_rng(fn))
    got = evalf(CR + fn, x, y)
    with np.errstate(all="ignore"):
        ref64 = np.power(x.astype(np.float64), y.astype(np.float64)) if fn == POW else F64[fn](x.astype(np.float64))
        ref = ftz(ref64.astype(np.float32))
    bad = got != ref
    assert bad.sum() <= 1, (x[bad][:5], got[bad][:5], ref[bad][:5])
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    ok = np.isfinite(ref64) & (ref != 0) & np.isfinite(ref)
    assert (np.abs(got.astype(np.float64) - ref64)[ok] <= 0.5000001 * ulp[ok]).all()


def test_sincos_beyond_the_fast_reduction_is_the_correctly_rounded_routine():
    x = ((np.random.default_rng(7).random(20000) * 2 - 1) * 1e4).astype(np.float32)
    x = x[np.abs(x) >= 120]
    assert (evalf(SIN, x) == evalf(CR + SIN, x)).all() and (evalf(COS, x) == evalf(CR + COS, x)).all()
    assert np.abs(evalf(SIN, x) - np.sin(x.astype(np.float64))).max() < 6e-8


# share of calls in which correct rounding differs from glibc 2.35 (= glibc's own share of not correctly rounded results), measured
# with this file: log 0.37 %, exp 0.06 %, sin 1.3 %, cos 1.3 %, cbrt 11.5 %, pow 0.07 %.  (The ~1.5-ulp routines of rounds 1-3
# differed from glibc in 7.6 / 9.4 / 21.6 / 26.7 / 14.6 / 0.07 % of the calls.)  One-sided bounds.
CR_GLIBC_BOUND = {LOG: 0.01, EXP: 0.005, SIN: 0.02, COS: 0.02, CBRT: 0.15, POW: 0.005}


@needs_glibc
@pytest.mark.parametrize("fn", [LOG, EXP, SIN, COS, CBRT, POW])
def test_distance_of_correct_rounding_from_glibc(fn):
    x, y = arguments(fn, np.random.default_rng(200 + fn))
    a = evalf(CR + fn, x, y)
    b = ftz(evalf(fn, x, y, ob.lib_libm()))
    share = float((a.view(np.uint32) != b.view(np.uint32)).mean())
    print("fn %d: correct rounding differs from glibc in %.3f %% of the calls" % (fn, 100 * share))
    assert share < CR_GLIBC_BOUND[fn]
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    assert d[np.isfinite(a) & np.isfinite(b)].max() <= 1                    # never by more than one unit in the last place


@pytest.mark.parametrize("base", [0, CR])
def test_special_values(base):
    L = ob.lib()
    LOGf, EXPf, SINf, COSf, CBRTf, POWf = (base + k for k in range(6))
    assert L.oracle_math(LOGf, 1.0, 0) == 0.0
    assert L.oracle_math(LOGf, 0.0, 0) == -np.inf
    assert L.oracle_math(LOGf, 1e-40, 0) == -np.inf       # denormals count as zero
    assert np.isnan(L.oracle_math(LOGf, -1.0, 0))
    assert L.oracle_math(LOGf, np.inf, 0) == np.inf
    assert L.oracle_math(EXPf, 0.0, 0) == 1.0
    assert L.oracle_math(EXPf, -100.0, 0) == 0.0          # flush-to-zero below FLT_MIN
    assert L.oracle_math(EXPf, -87.4, 0) == 0.0
    assert L.oracle_math(EXPf, 100.0, 0) == np.inf and L.oracle_math(EXPf, -np.inf, 0) == 0.0
    assert np.isnan(L.oracle_math(EXPf, np.nan, 0))
    assert L.oracle_math(SINf, 0.0, 0) == 0.0 and L.oracle_math(COSf, 0.0, 0) == 1.0
    assert L.oracle_math(CBRTf, 8.0, 0) == 2.0 and L.oracle_math(CBRTf, -27.0, 0) == -3.0
    assert L.oracle_math(CBRTf, 0.0, 0) == 0.0 and L.oracle_math(CBRTf, np.inf, 0) == np.inf
    assert L.oracle_math(POWf, 2.0, 10.0) == 1024.0 and L.oracle_math(POWf, 0.0, 2.0) == 0.0 and L.oracle_math(POWf, 3.0, 0.0) == 1.0
    assert L.oracle_math(POWf, 0.0, -1.0) == np.inf and L.oracle_math(POWf, np.inf, -1.0) == 0.0 and L.oracle_math(POWf, 1.0, 5.5) == 1.0
    assert L.oracle_math(POWf, 0.5, 200.0) == 0.0 and L.oracle_math(POWf, 2.0, 200.0) == np.inf
    assert np.isnan(L.oracle_math(POWf, -1.0, 0.5))


# ---- pm_div_by_invariant (pmath.h): x / d through rd = pm_invariant_rcp(d), the division by the majorant in every tracking step of
# volpath / volpathmis.  The oracle divides; the kernels must give the same bits for every dividend a render can produce.
SQRT, RCP, RSQRT, DIVINV = 12, 13, 14, 15
OP_MUL, OP_ADD, OP_FMA, OP_DIV, OP_SQRT, OP_F64 = range(6)
FLT_MIN_BITS = 0x00800000


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def fp32_op(op, a, b=None, c=None):
    """IEEE fp32 operation under FTZ | DAZ (the render workers' MXCSR), through oracle_fp32_op_n."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.float32)
    c = np.zeros_like(a) if c is None else np.ascontiguousarray(c, np.float32)
    out = np.empty_like(a)
    ob.lib().oracle_fp32_op_n(op, a.size, ob._p(a), ob._p(b), ob._p(c), ob._p(out))
    return out


def admitted_divisors(rng, n_random=8):
    """Every biased exponent the predicate can admit (67..187) x significands 0, 1, 0x400000, 0x7ffffe and n_random seeded ones;
    the ones pm_invariant_rcp admits."""
    e = np.arange(67, 188, dtype=np.uint32)
    m = np.concatenate([np.array([0, 1, 0x400000, 0x7ffffe], np.uint32)[None, :].repeat(e.size, 0),
                        rng.integers(0, 0x7fffff, (e.size, n_random), dtype=np.uint32)], 1)
    d = f32((e[:, None] << 23) | m).ravel()
    L = ob.lib()
    return np.array([x for x in d if L.oracle_invariant_rcp(float(x)) != 0], np.float32)


def dividends(rng, d, per_binade=48):
    """For one divisor: every binade of x (denormals included), both signs, +-0 / inf / NaN, and a dense set whose quotient lands in
    [2^-128, 2^-123] -- around FLT_MIN, where a flushed remainder or a quotient that rounds up to FLT_MIN breaks the corrections --
    with the neighbours of RN(FLT_MIN d)."""
    e = np.arange(0, 255, dtype=np.uint32).repeat(per_binade)
    m = rng.integers(0, 0x800000, e.size, dtype=np.uint32)
    m[::per_binade] = 0
    m[1::per_binade] = 0x7fffff
    x = f32((e << 23) | m)
    q = f32(rng.integers(0x00400000, 0x02000000, 4096, dtype=np.uint32))          # [2^-128, 2^-123)
    band = fp32_op(OP_MUL, q, np.full(q.size, d, np.float32))
    near = (fp32_op(OP_MUL, f32([FLT_MIN_BITS]), np.float32([d])).view(np.uint32) + np.arange(-64, 65, dtype=np.int64)).astype(np.uint32)
    special = f32([0, 1, 0x7fffff, 0x7f800000, 0x7fc00000, 0x7f7fffff])
    x = np.concatenate([x, band, f32(near), special])
    return np.concatenate([x, -x])


def div_mismatches(x, d):
    got = evalf(DIVINV, x, np.full(x.size, d, np.float32))
    want = fp32_op(OP_DIV, x, np.full(x.size, d, np.float32))
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    nan = ((gb & 0x7fffffff) > 0x7f800000) & ((wb & 0x7fffffff) > 0x7f800000)
    return x[(gb != wb) & ~nan], got[(gb != wb) & ~nan], want[(gb != wb) & ~nan]


def test_div_by_invariant_is_the_division_over_the_admitted_range():
    """Every admitted divisor exponent x every dividend binade, the band of quotients around FLT_MIN, denormal / zero / non-finite
    dividends: bit for bit x / d under FTZ | DAZ (the oracle's division)."""
    rng = np.random.default_rng(1234)
    ds = admitted_divisors(rng)
    assert ds.size > 121 * 8
    for d in ds:
        x, got, want = div_mismatches(dividends(rng, d), d)
        assert x.size == 0, ("d = %a: %d mismatches" % (float(d), x.size),
                             ["x %08x got %08x want %08x" % t for t in zip(x.view(np.uint32)[:8], got.view(np.uint32)[:8], want.view(np.uint32)[:8])])


@pytest.mark.parametrize("d_bits", [0x3f800000, 0x3f800001, 0x3fc00000, 0x3fffff7e, 0x21800000, 0x5d7ffffe])   # 1, 1+ulp, 1.5, ~2, 2^-60, ~2^60
def test_div_by_invariant_on_a_full_binade_of_dividends(d_bits):
    d = f32([d_bits])[0]
    assert ob.lib().oracle_invariant_rcp(float(d)) != 0
    x = f32((np.uint32(127) << 23) | np.arange(0x800000, dtype=np.uint32))
    x = np.concatenate([x, x * np.float32(2.0 ** -100), x * np.float32(2.0 ** 61)])    # [1, 2), the low end, the high end of the window
    x, got, want = div_mismatches(x, d)
    assert x.size == 0, ["x %08x got %08x want %08x" % t for t in zip(x.view(np.uint32)[:8], got.view(np.uint32)[:8], want.view(np.uint32)[:8])]


def test_invariant_rcp_admits_exactly_its_range():
    """The predicate (pm_invariant_rcp, shared by scene_host.cpp and the tests) at its edges: biased exponents 66 / 67 and 187 / 188,
    the all-ones significand, non-positive and non-finite divisors."""
    L = ob.lib()
    rcp = lambda bits: L.oracle_invariant_rcp(float(f32([bits])[0]))
    assert rcp(66 << 23) == 0 and rcp((66 << 23) | 0x400000) == 0
    assert rcp(67 << 23) == 2.0 ** 60 and rcp((67 << 23) | 0x400000) != 0
    assert rcp(187 << 23) == 2.0 ** -60                    # d = 2^60: rd = 2^-60 is biased 67
    assert rcp((187 << 23) | 1) == 0                       # rd below 2^-60: biased 66
    assert rcp(188 << 23) == 0
    for e in (67, 127, 150, 186):
        assert rcp((e << 23) | 0x7fffff) == 0 and rcp((e << 23) | 0x7ffffe) != 0
    for bits in (0, 0x80000000, 0xbf800000, 0x7f800000, 0x7fc00000, 0x00000001, 0x007fffff):
        assert rcp(bits) == 0
    assert rcp(0x3fc00000) == np.float32(1 / np.float32(1.5))
    assert L.oracle_math(SQRT, 2.0, 0) == np.float32(np.sqrt(np.float32(2))) and L.oracle_math(RCP, 4.0, 0) == 0.25
    assert L.oracle_math(RSQRT, 4.0, 0) == 0.5 and L.oracle_math(DIVINV, 3.0, 1.5) == 2.0


def test_fp32_ops_flush_like_the_render_workers():
    """oracle_fp32_op_n runs under FTZ | DAZ: denormal operands count as zero, tiny results flush; a result that rounds UP to FLT_MIN
    is FLT_MIN (x86 detects tininess after rounding)."""
    tiny = f32([0x00000001, 0x007fffff])
    assert (fp32_op(OP_ADD, tiny, np.float32([0, 0])) == 0).all()
    assert (fp32_op(OP_MUL, f32([FLT_MIN_BITS]), np.float32([0.5])) == 0).all()
    assert fp32_op(OP_MUL, f32([0x3f7ffffe]), f32([0x00800001])).view(np.uint32)[0] == FLT_MIN_BITS
    assert fp32_op(OP_DIV, f32([0x00800001]), f32([0x3f800001])).view(np.uint32)[0] == FLT_MIN_BITS
    assert fp32_op(OP_F64, f32([FLT_MIN_BITS]), np.float32([0.75])).view(np.uint32)[0] == 0
