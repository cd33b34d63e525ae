"""csrc/unit_config.h on the CPU: the one table that says what each device unit is.  The host preprocessor reads the header for every
unit, with and without -DMTSAMD_BLOCKSTATS, and the values are held against the literal table below -- the values the units had when
each switch was still decided by an expression of its own over MTS_TRAITS / MTS_SPEC_N / MTS_LEAN, read off those expressions.  A
switch that none of a unit's kernels reads is not pinned (units p and ps have no ring kernel).  Which promises a unit is COMPILED with
is held against what the host plan ASKS of a scene for it (render_plan.cpp: KERNEL_UNITS)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eradiate-kernel_amd", "csrc")
CXX = os.environ.get("CXX", "g++")
FIELDS = ("MTS_UNIT", "MTS_SPEC_N", "MTS_TRAITS", "MTS_STEP_FAST", "MTS_CROSS_CLASS", "MTS_HOT_DRCP", "MTS_OPAQUE_INIT", "MTS_GEOM_LDS", "MTS_MIS_THREADS",
          "MTS_PATH_ONLY", "MTS_VARIANT_NS", "MTS_LAUNCHER(launch_render)")
PROBE = '#include "unit_config.h"\n' + "".join("PROBE %d = %s ;\n" % (k, f) for k, f in enumerate(FIELDS)) + \
        "#ifdef MTS_LEAN\nPROBE lean = 1 ;\n#else\nPROBE lean = 0 ;\n#endif\n#ifdef MTS_LEAN_PATH\nPROBE lean_path = 1 ;\n#else\nPROBE lean_path = 0 ;\n#endif\n"
TRAITS = ("MT_UNIT_A", "MT_UNIT_B", "MT_UNIT_C", "MT_UNIT_H", "MT_UNIT_P", "MT_UNIT_P_NEEDS")

# unit: (KernelUnit, translation unit, MTS_SPEC_N, MTS_TRAITS, namespace, launcher,
#        (STEP_FAST, CROSS_CLASS, HOT_DRCP, GEOM_LDS, volpathmis threads) or None: path kernels only)
TABLE = {
    "general rgb":      (0, "kernels.hip",          3, 0,           "v_rgb",             "launch_render",          (0, 0, 0, 0, 512)),
    "general spectral": (0, "kernels_spectral.hip", 4, 0,           "v_spectral",        "launch_render_spectral", (0, 0, 1, 0, 256)),
    "a":                (1, "kernels_lean_a.hip",   3, "MT_UNIT_A", "v_rgb_lean_a",      "launch_render_lean_a",   (1, 1, 0, 1, 768)),
    "b":                (2, "kernels_lean_b.hip",   3, "MT_UNIT_B", "v_rgb_lean_b",      "launch_render_lean_b",   (1, 1, 0, 0, 512)),
    "c":                (7, "kernels_lean_c.hip",   3, "MT_UNIT_C", "v_rgb_lean_c",      "launch_render_lean_c",   (1, 0, 1, 0, 512)),
    "h":                (6, "kernels_lean_h.hip",   3, "MT_UNIT_H", "v_rgb_lean_h",      "launch_render_lean_h",   (0, 0, 0, 1, 512)),
    "s":                (3, "kernels_lean_s.hip",   4, "MT_UNIT_B", "v_spectral_lean",   "launch_render_lean_s",   (0, 0, 1, 0, 256)),
    "p":                (4, "kernels_lean_p.hip",   3, "MT_UNIT_P", "v_rgb_lean_p",      "launch_render_lean_p",   None),
    "ps":               (5, "kernels_lean_ps.hip",  4, "MT_UNIT_P", "v_spectral_lean_p", "launch_render_lean_ps",  None),
}
# -DMTSAMD_BLOCKSTATS: the lean units build no kernels; the general rgb unit stands in for a and b, the spectral one is as it is
BLOCKSTATS = {"general rgb": (0, 1, 0, 1, 512), "general spectral": (0, 0, 1, 0, 256)}


def preprocess(text, defines, check=True):
    r = subprocess.run([CXX, "-E", "-P", "-x", "c++", "-I", CSRC] + ["-D" + d for d in defines] + ["-"], input=text, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, r.stderr
    return r


def value(text):
    """a preprocessed constant expression over integers, | and parentheses -> int; anything else -> the text without blanks"""
    return eval(text, {"__builtins__": {}}) if re.fullmatch(r"[\d\s|()]+", text) else re.sub(r"\s+", "", text)


def probe(defines):
    got = dict(re.findall(r"PROBE (\w+) = (.*?) ;", preprocess(PROBE, defines).stdout))
    r = {f: value(got[str(k)]) for k, f in enumerate(FIELDS)}
    r["lean"], r["lean_path"] = int(got["lean"]), int(got["lean_path"])
    return r


@pytest.fixture(scope="module")
def traits():
    out = preprocess('#include "dscene.h"\n' + "".join("PROBE %d = %s ;\n" % (k, t) for k, t in enumerate(TRAITS)), []).stdout
    return {TRAITS[int(k)]: value(v) for k, v in re.findall(r"PROBE (\d+) = (.*?) ;", out)}


def unit_defines(name):
    """What the translation unit of `name` defines ahead of its `#include "kernels.hip"`: the #define lines of the file itself."""
    if TABLE[name][1] == "kernels.hip":
        return []
    src = open(os.path.join(CSRC, TABLE[name][1])).read()
    return ["%s=%s" % (m.group(1), m.group(2).split("//")[0].strip()) for m in re.finditer(r"^\s*#\s*define\s+(\w+)[ \t]*(.*)$", src, re.M)]


def ring_switches(got):
    return tuple(got[f] for f in ("MTS_STEP_FAST", "MTS_CROSS_CLASS", "MTS_HOT_DRCP", "MTS_GEOM_LDS", "MTS_MIS_THREADS"))


@pytest.mark.parametrize("name", list(TABLE))
def test_unit_is_what_the_table_says(name, traits):
    unit, _, spec_n, unit_traits, ns, launcher, ring = TABLE[name]
    for defines in (unit_defines(name), ["MTS_UNIT=%d" % unit] + (["MTS_SPEC_N=4"] if name == "general spectral" else [])):
        got = probe(defines)
        assert got["MTS_UNIT"] == unit and got["MTS_SPEC_N"] == spec_n
        assert got["MTS_TRAITS"] == (traits[unit_traits] if unit_traits else 0)
        assert got["MTS_VARIANT_NS"] == ns and got["MTS_LAUNCHER(launch_render)"] == launcher
        assert got["lean"] == (unit != 0) and got["lean_path"] == got["MTS_PATH_ONLY"] == (ring is None)
        if ring is not None:
            assert ring_switches(got) == ring
            assert got["MTS_OPAQUE_INIT"] == "(!%d)" % ring[2]                 # derived from MTS_HOT_DRCP, in one place


@pytest.mark.parametrize("name", list(TABLE))
def test_unit_of_the_diagnostic_build(name):
    unit, source, spec_n, _, ns, launcher, _ = TABLE[name]
    if unit == 0:
        got = probe(unit_defines(name) + ["MTSAMD_BLOCKSTATS"])
        assert (got["MTS_SPEC_N"], got["MTS_TRAITS"], got["MTS_VARIANT_NS"], got["MTS_LAUNCHER(launch_render)"], got["lean"]) == (spec_n, 0, ns, launcher, 0)
        assert ring_switches(got) == BLOCKSTATS[name] and got["MTS_PATH_ONLY"] == 0
        return
    # a lean unit builds no kernels: its file is empty to the compiler, and the table has no block for it
    assert preprocess(open(os.path.join(CSRC, source)).read(), ["MTSAMD_BLOCKSTATS"]).stdout.strip() == ""
    r = preprocess(PROBE, ["MTS_UNIT=%d" % unit, "MTSAMD_BLOCKSTATS"], check=False)
    assert r.returncode != 0 and "no lean units" in r.stderr


def test_a_unit_outside_the_table_does_not_compile():
    r = preprocess(PROBE, ["MTS_UNIT=8"], check=False)
    assert r.returncode != 0 and "names no unit" in r.stderr


def test_lean_files_define_nothing_but_their_unit():
    files = sorted(f for f in os.listdir(CSRC) if re.fullmatch(r"kernels_lean_\w+\.hip", f))
    assert files == sorted(t[1] for t in TABLE.values() if t[0] != 0)
    for f in files:
        src = open(os.path.join(CSRC, f)).read()
        assert re.findall(r"^\s*#\s*define\s+(\w+)", src, re.M) == ["MTS_UNIT"], f
        assert re.findall(r"^\s*#\s*include\s+(\S+)", src, re.M) == ['"kernels.hip"'], f
    assert unit_defines("general spectral") == ["MTS_SPEC_N=4"]


def test_compiled_traits_are_what_the_plan_asks(tmp_path, traits):
    """render_plan.cpp sends a scene to a unit when it keeps KERNEL_UNITS' promises for it; the unit's kernels are compiled with MTS_TRAITS.
    The two are the same MT_UNIT_* -- except `path`'s units, compiled with MT_UNIT_P, of which `path` can reach MT_UNIT_P_NEEDS."""
    out = str(tmp_path / "librender_plan.so")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "micro", "render_plan_shim.cpp"), os.path.join(CSRC, "render_plan.cpp"), "-o", out])
    lib = C.CDLL(out)
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    lib.rp_kernel_rows.argtypes = [i32p, i32p, i32p]
    rows, units, n_units = np.zeros((256, 6), np.int32), np.zeros((16, 2), np.int32), np.zeros(1, np.int32)
    n_rows = lib.rp_kernel_rows(rows, units, n_units)
    promises = {int(u): int(p) for u, p in units[:n_units[0]]}
    assert sorted(promises) == list(range(8))
    assert traits["MT_UNIT_P"] & traits["MT_UNIT_P_NEEDS"] == traits["MT_UNIT_P_NEEDS"]
    for name, (unit, _, spec_n, unit_traits, _, _, ring) in TABLE.items():
        compiled = probe(unit_defines(name))["MTS_TRAITS"]
        assert compiled == (traits[unit_traits] if unit_traits else 0)
        assert promises[unit] == (traits["MT_UNIT_P_NEEDS"] if ring is None else compiled), name
        # the rows of the unit are of the unit's build (rgb / mono or spectral), and a unit with the path kernels only has only `path` rows
        mine = [r for r in rows[:n_rows] if int(r[0]) == unit and bool(r[5]) == (spec_n == 4)]
        assert mine and (ring is not None or all(int(r[2]) == 0 for r in mine)), name
