"""The device build of csrc/pmath.h against the host build (the oracle), bit for bit (run with -m gpu on an MI355X).

The film parity of the whole suite rests on one claim of pmath.h: the same source gives the same bits from gcc on x86-64 (the oracle,
under the render workers' MXCSR FTZ | DAZ) and from hipcc for gfx950 (-fgpu-flush-denormals-to-zero).  The device has paths the host
never runs -- the __constant__ tables, their LDS copies (PM_TABLES_IN_LDS), v_rcp-based pm_rcp inside pm_rsqrt, gfx950 fp64 inside
every transcendental, the GPU's flush mode -- so they are pinned here directly:
 * every fp32 bit pattern (2^32) of log, exp, sin, cos, cbrt, sqrt, rsqrt and the _cr routines: the constant-table build against
   the host (oracle_math_sweep, 16 threads), the LDS build against the constant-table build on the device;
 * pow on 1.6 * 10^9 structured pairs (every significand of [0.5, 2) x a list of exponents) and on threshold / negative / random pairs;
 * pm_div_by_invariant against the device's own x / d for all 2^32 dividends of 64 admitted divisors, and against the host's x / d on
   the band of quotients around FLT_MIN;
 * mul, add, fma, div, sqrt and the f64 -> f32 conversion at the flush boundary, against the host under FTZ | DAZ (equal, results
   that round up to FLT_MIN included), and comparisons with denormal operands.
tests/micro/pmath_device.hip is built twice with the product's flags and driven through ctypes in a child interpreter (a time limit
of its own; the suite's process never loads it).  Every assertion reports the first 8 mismatching bit patterns."""
import ctypes as C
import importlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import tests.oracle_binding as ob  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.slow]

UNARY = {"log": 0, "exp": 1, "sin": 2, "cos": 3, "cbrt": 4, "sqrt": 12, "rsqrt": 14,
         "log_cr": 6, "exp_cr": 7, "sin_cr": 8, "cos_cr": 9, "cbrt_cr": 10}
POW, POW_CR, RCP, DIVINV = 5, 11, 13, 15
OPS = {"mul": 0, "add": 1, "fma": 2, "div": 3, "sqrt": 4, "f64_to_f32": 5}
CHUNK = 1 << 26                         # 256 MiB of fp32 per device buffer and per pinned host buffer
THREADS = 16                            # host threads of the comparator


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def hexes(bits):
    return ["%08x" % b for b in np.asarray(bits, np.uint32)[:8]]


# ------------------------------------------------------------------------------------------------------------------ child side
class Device:
    """The two builds of tests/micro/pmath_device.hip in one process: `c` (constant-address-space tables) and `l` (LDS copies)."""

    def __init__(self, libdir):
        self.c = C.CDLL(os.path.join(libdir, "libpmd_const.so"))
        self.l = C.CDLL(os.path.join(libdir, "libpmd_lds.so"))
        for L in (self.c, self.l):
            L.pmd_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            L.pmd_host_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            L.pmd_free.argtypes = L.pmd_host_free.argtypes = [C.c_void_p]
            L.pmd_to_device.argtypes = L.pmd_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
            L.pmd_sweep.argtypes = [C.c_int, C.c_uint32, C.c_int64, C.c_float, C.c_void_p]
            L.pmd_pairs.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pmd_fp32_op.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pmd_compare.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
            L.pmd_div_sweep.argtypes = [C.c_uint32, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_uint64)]
        self.a, self.b, self.x, self.y = (self.alloc(CHUNK * 4) for _ in range(4))
        self.word = self.alloc(8)
        p = C.c_void_p()
        self.ok(self.c.pmd_host_malloc(C.byref(p), CHUNK * 4))
        self.pinned = p.value
        self.host = np.ctypeslib.as_array(C.cast(self.pinned, C.POINTER(C.c_float)), (CHUNK,))

    @staticmethod
    def ok(status):
        if status != 0:
            raise RuntimeError("HIP call failed")

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.c.pmd_malloc(C.byref(p), nbytes))
        return p.value

    def compare(self, n, a, b):
        cnt = C.c_uint64()
        self.ok(self.c.pmd_compare(n, a, b, self.word, C.byref(cnt)))
        return cnt.value

    def fetch(self, n, dptr):
        out = np.empty(n, np.float32)
        self.ok(self.c.pmd_to_host(out.ctypes.data, dptr, n * 4))
        return out

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        assert arr.size <= CHUNK
        self.ok(self.c.pmd_to_device(dptr, arr.ctypes.data, arr.nbytes))

    def pairs(self, lib, fn, x, y):
        """Device values of fn on the pairs (x, y), in chunks."""
        out = np.empty(x.size, np.float32)
        for k in range(0, x.size, CHUNK):
            n = min(CHUNK, x.size - k)
            self.upload(self.x, x[k:k + n]); self.upload(self.y, y[k:k + n])
            self.ok(lib.pmd_pairs(fn, n, self.x, self.y, self.a))
            self.ok(self.c.pmd_to_host(out[k:].ctypes.data, self.a, n * 4))
        return out


def nan_equal_mismatch(a, b):
    u, v = a.view(np.uint32), b.view(np.uint32)
    nan = ((u & 0x7fffffff) > 0x7f800000) & ((v & 0x7fffffff) > 0x7f800000)
    return (u != v) & ~nan


def sweep(dev, L, fn, first, n, y=0.0):
    """fn on the bit patterns first .. first + n - 1 (second argument y): the constant-table build against the host, the LDS build
    against the constant-table build.  Returns (host mismatches, first 8 of them, LDS mismatches, first 8 of them)."""
    host_bad, host_first, lds_bad, lds_first = 0, [], 0, []
    bad = (C.c_uint32 * 8)()
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        start = (first + k) & 0xffffffff
        dev.ok(dev.c.pmd_sweep(fn, start, m, y, dev.a))
        dev.ok(dev.l.pmd_sweep(fn, start, m, y, dev.b))
        d = dev.compare(m, dev.a, dev.b)
        if d:
            mis = np.nonzero(nan_equal_mismatch(dev.fetch(m, dev.a), dev.fetch(m, dev.b)))[0][:8]
            lds_first += [(start + int(i)) & 0xffffffff for i in mis][:8 - len(lds_first)]
            lds_bad += d
        dev.ok(dev.c.pmd_to_host(dev.pinned, dev.a, m * 4))
        h = L.oracle_math_sweep(fn, start, m, y, dev.pinned, bad, 8, THREADS)
        if h:
            host_first += list(bad[:min(h, 8)])[:8 - len(host_first)]
            host_bad += h
    return host_bad, host_first, lds_bad, lds_first


def host_pairs(L, fn, x, y):
    out = np.empty(x.size, np.float32)
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    L.oracle_math_n(fn, x.size, ob._p(x), ob._p(y), ob._p(out))
    return out


def pairs_report(dev, L, fn, x, y):
    c = dev.pairs(dev.c, fn, x, y)
    lds = dev.pairs(dev.l, fn, x, y)
    h = host_pairs(L, fn, x, y)
    bh, bl = nan_equal_mismatch(c, h), nan_equal_mismatch(c, lds)
    fmt = lambda m: ["x %08x y %08x" % (a, b) for a, b in zip(x.view(np.uint32)[m][:8], y.view(np.uint32)[m][:8])]
    return {"n": int(x.size), "host_bad": int(bh.sum()), "host_first": fmt(bh), "lds_bad": int(bl.sum()), "lds_first": fmt(bl)}


def pow_structured():
    """(first_bits, n, y) sweeps: every significand of [0.5, 2) x the exponents; every negative base of [-2, -0.5) x integers."""
    ys = [float(k) for k in range(-40, 41)] + [0.5, -0.5, 1 / 3, -1 / 3, 2.2, 1 / 2.2, 1e10, -1e10, 0.0, -0.0, np.inf, -np.inf, np.nan]
    out = [(0x3f000000, 1 << 24, y) for y in ys]
    out += [(0xbf000000, 1 << 24, y) for y in (-3.0, -2.0, -1.0, 1.0, 2.0, 3.0)]
    return out


def pow_pairs(rng):
    """Pairs that straddle the overflow (y log2 x = 128) and FLT_MIN (-126) / underflow (-150) thresholds, negative bases with integer
    exponents, and seeded random pairs over the whole range (every bit pattern of both)."""
    x = f32(rng.integers(0x00800000, 0x7f800000, 1 << 22, dtype=np.uint32))
    lg = np.log2(x.astype(np.float64))
    lg[lg == 0] = 1.0
    t = rng.choice([128.0, -126.0, -150.0], x.size) * (1 + rng.uniform(-2e-6, 2e-6, x.size))
    y = (t / lg).astype(np.float32)
    neg = -f32(rng.integers(0x00800000, 0x7f800000, 1 << 20, dtype=np.uint32))
    ny = rng.integers(-60, 61, neg.size).astype(np.float32)
    rx = f32(rng.integers(0, 1 << 32, 1 << 24, dtype=np.uint64).astype(np.uint32))
    ry = f32(rng.integers(0, 1 << 32, 1 << 24, dtype=np.uint64).astype(np.uint32))
    return np.concatenate([x, neg, rx]), np.concatenate([y, ny, ry])


def divisors(L, rng):
    """64 admitted divisors: the edges of the predicate's range (biased exponents 67 and 187, significands 0, 1, 0x400000, 0x7ffffe)
    and seeded random ones; each with its host reciprocal pm_invariant_rcp."""
    edge = [(e << 23) | m for e in (67, 68, 126, 127, 186, 187) for m in (0, 1, 0x400000, 0x7ffffe)]
    ds = []
    for b in edge + [int(v) for v in rng.integers(67 << 23, 188 << 23, 400, dtype=np.uint32)]:
        d = float(f32([b])[0])
        rd = L.oracle_invariant_rcp(d)
        if rd != 0 and b not in [x for x, _ in ds]:
            ds.append((b, rd))
        if len(ds) == 64:
            break
    assert len(ds) == 64
    return ds


def flush_operands(rng, n=1 << 20):
    """Operands whose exact result lies within two binades of FLT_MIN (both sides), with the targets that round UP to FLT_MIN, plus
    denormal operands."""
    tgt = f32(rng.integers(0x00200000, 0x01800000, n, dtype=np.uint32)).astype(np.float64)       # [2^-128, 2^-124)
    up = f32(np.uint32(0x00800000)).astype(np.float64) * (1 - rng.uniform(0, 2.0 ** -24, n // 8))  # rounds up to FLT_MIN
    tgt = np.concatenate([tgt, up])
    sgn = rng.choice([-1.0, 1.0], tgt.size)
    a = f32(rng.integers(0x3f800000, 0x40000000, tgt.size, dtype=np.uint32)).astype(np.float64) * 2.0 ** rng.integers(-20, 21, tgt.size)
    den = f32(rng.integers(1, 0x00800000, n // 4, dtype=np.uint32))
    ops = {}
    b = (tgt / a).astype(np.float32)                                     # a * b ~ tgt
    ops["mul"] = (np.concatenate([a.astype(np.float32), den, f32([0x3f7ffffe])]),
                  np.concatenate([b * sgn.astype(np.float32), np.float32(1.5) + den * 0, f32([0x00800001])]), None)
    b = (a * (1 + rng.uniform(-1e-7, 1e-7, a.size))).astype(np.float32)   # a - b ~ tiny: differences near FLT_MIN, scaled down
    sa = (tgt * 2.0 ** 20).astype(np.float32)
    sb = (sa.astype(np.float64) - tgt * sgn).astype(np.float32)
    ops["add"] = (np.concatenate([sa, den, den]), np.concatenate([-sb, np.float32(0) * den, den]), None)
    fa = a.astype(np.float32)
    fb = (tgt / a * 2.0 ** 10).astype(np.float32)
    fc = (-(fa.astype(np.float64) * fb.astype(np.float64)) + tgt * sgn).astype(np.float32)
    ops["fma"] = (np.concatenate([fa, den]), np.concatenate([fb, den]), np.concatenate([fc, np.float32(1e-38) + den * 0]))
    dd = (1.0 / a).astype(np.float32)
    dx = (tgt * sgn * dd.astype(np.float64)).astype(np.float32)          # dx / dd ~ tgt
    ops["div"] = (np.concatenate([dx, den, f32([0x00800001])]), np.concatenate([dd, np.float32(0.75) + den * 0, f32([0x3f800001])]), None)
    ops["sqrt"] = (np.concatenate([f32(np.arange(0, 0x01800000, 7, dtype=np.uint32)), -den]), None, None)   # denormal and smallest normal operands
    ops["f64_to_f32"] = (a.astype(np.float32), (tgt * sgn / a.astype(np.float32).astype(np.float64) * (1 + 2.0 ** -30)).astype(np.float32), None)
    ops["f64_to_f32"] = (np.concatenate([ops["f64_to_f32"][0], den]), np.concatenate([ops["f64_to_f32"][1], np.float32(1.0) + den * 0]), None)
    return ops


def child(case, libdir, only=None):
    L = ob.lib()
    dev = Device(libdir)
    rng = np.random.default_rng(20261016)
    out = {}
    if case == "unary":
        for name, fn in UNARY.items():
            if only and name not in only:
                continue
            hb, hf, lb, lf = sweep(dev, L, fn, 0, 1 << 32)
            out[name] = {"host_bad": hb, "host_first": hexes(hf), "lds_bad": lb, "lds_first": hexes(lf)}
    elif case == "pow":
        for fn, tag in ((POW, "pow"), (POW_CR, "pow_cr")):
            tot = {"n": 0, "host_bad": 0, "host_first": [], "lds_bad": 0, "lds_first": []}
            for first, n, y in pow_structured():
                hb, hf, lb, lf = sweep(dev, L, fn, first, n, y)
                tot["n"] += n; tot["host_bad"] += hb; tot["lds_bad"] += lb
                tot["host_first"] += ["x %08x y %r" % (b, y) for b in hf]; tot["lds_first"] += ["x %08x y %r" % (b, y) for b in lf]
            x, y = pow_pairs(rng)
            r = pairs_report(dev, L, fn, x, y)
            tot["n"] += r["n"]; tot["host_bad"] += r["host_bad"]; tot["lds_bad"] += r["lds_bad"]
            tot["host_first"] = (tot["host_first"] + r["host_first"])[:8]; tot["lds_first"] = (tot["lds_first"] + r["lds_first"])[:8]
            out[tag] = tot
    elif case == "div":
        ds = divisors(L, rng)
        cnt = C.c_uint64()
        res = {"divisors": len(ds), "device_bad": 0, "device_first": [], "band_n": 0, "band_bad": 0, "band_first": []}
        for b, rd in ds:
            d = float(f32([b])[0])
            for half in (0, 1 << 31):
                dev.ok(dev.c.pmd_div_sweep(half, 1 << 31, d, rd, dev.word, C.byref(cnt)))
                if cnt.value:
                    res["device_bad"] += cnt.value
                    res["device_first"].append("d %08x (dividends from %08x): %d" % (b, half, cnt.value))
            # the host's x / d on the band of quotients [2^-128, 2^-123] and around RN(FLT_MIN d)
            q = f32(rng.integers(0x00400000, 0x02000000, 1 << 16, dtype=np.uint32)).astype(np.float64)
            x = (q * d).astype(np.float32)
            near = ((np.float64(2.0 ** -126) * d) * (1 + np.arange(-4096, 4097) * 2.0 ** -30)).astype(np.float32)
            x = np.concatenate([x, near, -x, -near])
            dv = np.full(x.size, d, np.float32)
            got = dev.pairs(dev.c, DIVINV, x, dv)
            want = np.empty_like(x)
            L.oracle_fp32_op_n(3, x.size, ob._p(x), ob._p(dv), ob._p(dv), ob._p(want))
            m = nan_equal_mismatch(got, want)
            res["band_n"] += int(x.size); res["band_bad"] += int(m.sum())
            res["band_first"] += ["x %08x d %08x" % (u, b) for u in x.view(np.uint32)[m][:8]]
        res["device_first"] = res["device_first"][:8]; res["band_first"] = res["band_first"][:8]
        out["div"] = res
    elif case == "flush":
        for name, (a, b, c) in flush_operands(rng).items():
            b = np.zeros_like(a) if b is None else b
            c = np.zeros_like(a) if c is None else c
            dev.upload(dev.x, a); dev.upload(dev.y, b); dev.upload(dev.b, c)
            dev.ok(dev.c.pmd_fp32_op(OPS[name], a.size, dev.x, dev.y, dev.b, dev.a))
            got = dev.fetch(a.size, dev.a)
            want = np.empty_like(a)
            L.oracle_fp32_op_n(OPS[name], a.size, ob._p(a), ob._p(b), ob._p(c), ob._p(want))
            m = nan_equal_mismatch(got, want)
            near = np.abs(want.astype(np.float64)) < 2.0 ** -123
            out[name] = {"n": int(a.size), "near_flt_min": int(near.sum()), "bad": int(m.sum()),
                         "first": ["a %08x b %08x c %08x: device %08x host %08x" % t for t in
                                   zip(a.view(np.uint32)[m][:8], b.view(np.uint32)[m][:8], c.view(np.uint32)[m][:8],
                                       got.view(np.uint32)[m][:8], want.view(np.uint32)[m][:8])]}
    if case == "flush":                      # comparisons with denormal operands
        den = f32(rng.integers(1, 0x00800000, 1 << 18, dtype=np.uint32)) * rng.choice(np.float32([-1, 1]), 1 << 18)
        q = den.size // 4
        other = np.concatenate([den[::-1][:2 * q], np.zeros(q, np.float32), -np.zeros(q, np.float32)])
        norm = f32(rng.integers(0x00800000, 0x01000000, den.size, dtype=np.uint32)) * rng.choice(np.float32([-1, 1]), den.size)
        a = np.concatenate([den, den, norm, den])
        b = np.concatenate([other, norm, norm[::-1], np.float32(0) * den])
        for name, op, exact in (("lt", 6, np.less), ("eq", 7, np.equal)):
            dev.upload(dev.x, a); dev.upload(dev.y, b); dev.upload(dev.b, b)
            dev.ok(dev.c.pmd_fp32_op(op, a.size, dev.x, dev.y, dev.b, dev.a))
            got = dev.fetch(a.size, dev.a)
            want = np.empty_like(a)
            L.oracle_fp32_op_n(op, a.size, ob._p(a), ob._p(b), ob._p(b), ob._p(want))
            fa = np.where(np.abs(a) < np.float32(2.0 ** -126), np.float32(0), a)
            fb = np.where(np.abs(b) < np.float32(2.0 ** -126), np.float32(0), b)
            m = got != want
            out["cmp_" + name] = {"n": int(a.size), "bad": int(m.sum()),
                                  "device_is_exact": bool((got == exact(a, b)).all()), "host_is_flushed": bool((want == exact(fa, fb)).all()),
                                  "outside_class": int((m & (exact(a, b) == exact(fa, fb))).sum()),
                                  "first": ["a %08x b %08x: device %g host %g" % t for t in
                                            zip(a.view(np.uint32)[m][:8], b.view(np.uint32)[m][:8], got[m][:8], want[m][:8])]}
    print("PMD_RESULT " + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------------------------ test side
@pytest.fixture(scope="module")
def device_libs(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in importlib.import_module("eradiate-kernel_amd._buildid").FLAGS if f != "-Wall"]
    assert "-fgpu-flush-denormals-to-zero" in flags and "-shared" in flags and "-fPIC" in flags
    src = os.path.join(ROOT, "tests", "micro", "pmath_device.hip")
    out = tmp_path_factory.mktemp("pmath_device")
    for name, extra in (("libpmd_const.so", []), ("libpmd_lds.so", ["-DPM_TABLES_IN_LDS"])):
        subprocess.run([hipcc] + flags + extra + ["-w", src, "-o", str(out / name)], check=True, timeout=600)
    ob.lib()                                       # liboracle.so exists before the child loads it
    return str(out)


def run_child(case, libdir, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case, libdir], capture_output=True, text=True, timeout=timeout,
                       cwd=ROOT)
    line = [s for s in r.stdout.splitlines() if s.startswith("PMD_RESULT ")]
    assert r.returncode == 0 and line, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    res = json.loads(line[-1][len("PMD_RESULT "):])
    print(case, json.dumps(res))
    return res


def test_every_fp32_argument_of_the_unary_functions(device_libs):
    """log, exp, sin, cos, cbrt, sqrt, rsqrt and the _cr routines on all 2^32 bit patterns: device == host, LDS tables == constant tables."""
    res = run_child("unary", device_libs, timeout=1500)
    assert set(res) == set(UNARY)
    for name, r in res.items():
        assert r["host_bad"] == 0, ("%s: device (constant tables) against the host" % name, r)
        assert r["lds_bad"] == 0, ("%s: LDS tables against constant tables" % name, r)


def test_pow_on_structured_and_random_pairs(device_libs):
    res = run_child("pow", device_libs, timeout=900)
    for name in ("pow", "pow_cr"):
        r = res[name]
        assert r["n"] >= 10 ** 8
        assert r["host_bad"] == 0, (name, r)
        assert r["lds_bad"] == 0, (name, r)


def test_div_by_invariant_on_the_device(device_libs):
    """pm_div_by_invariant against the device's own x / d for all 2^32 dividends of 64 admitted divisors (the predicate's edges and
    random ones), and against the host's x / d where the quotient lies around FLT_MIN."""
    r = run_child("div", device_libs, timeout=900)["div"]
    assert r["divisors"] == 64
    assert r["device_bad"] == 0, r
    assert r["band_bad"] == 0 and r["band_n"] > 64 * 100000, r


def test_basic_ops_at_the_flush_boundary(device_libs):
    """mul, add, fma, div, sqrt and f64 -> f32 with results within two binades of FLT_MIN (including those that round up to FLT_MIN)
    and denormal operands: the device under -fgpu-flush-denormals-to-zero against the host under FTZ | DAZ."""
    res = run_child("flush", device_libs, timeout=600)
    assert set(res) == set(OPS) | {"cmp_lt", "cmp_eq"}
    # Comparisons with denormal operands, computed at run time: both sides compare the flushed values (pm_pow's
    # tests of y == 0 and x < 0 had differed on such operands -- compiled as bit tests against the constant -- and now read the bits).
    for name in ("cmp_lt", "cmp_eq"):
        r = res.pop(name)
        assert r["host_is_flushed"] and r["bad"] == 0, (name, r)
    for name, r in res.items():
        assert name == "sqrt" or r["near_flt_min"] > r["n"] // 4, (name, r)    # sqrt: no result comes near FLT_MIN
        assert r["bad"] == 0, (name, r)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2], sys.argv[3].split(",") if len(sys.argv) > 3 else None)
