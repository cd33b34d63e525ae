"""Does this tree compile to the same device code as another revision?  The proof a refactor of the kernels gives of itself.

    python tools/asm_identity.py OTHER_CSRC_DIR [--extra "-DMTSAMD_BLOCKSTATS"] [--keep DIR]

Compiles every device unit of _buildid.SOURCES from this tree's csrc/ and from OTHER_CSRC_DIR -- the csrc/ of another checkout, its
directory layout kept (csrc includes ../../include/mtsamd.h), for instance

    mkdir /tmp/parent && git archive HEAD~1 | tar -x -C /tmp/parent        # -> /tmp/parent/eradiate-kernel_amd/csrc

for the device only, to assembly, with the product flags of _buildid.py and no line tables (as step_loop_stats.compile_asm), at most 16
compilations side by side.  The two texts of a unit are compared line by line after dropping the lines that name the unit's
`__hip_cuid_` symbol (a hash of the source file's path and content).  Prints the number of differing lines per unit; the exit status
is 1 if any line differs.  --extra gives both sides more flags; --keep keeps the assembly files.  It compares text, nothing else.
"""
import argparse
import concurrent.futures
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "eradiate-kernel_amd"))
import _buildid  # noqa: E402

UNITS = [s for s in _buildid.SOURCES if s.endswith(".hip")]
DROP = "__hip_cuid_"


def compile_asm(csrc, unit, out, extra):
    flags = [f for f in _buildid.FLAGS if f not in ("-shared", "-fPIC")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + flags + extra + ["--cuda-device-only", "-S", "-x", "hip", os.path.join(csrc, unit), "-o", out]
    subprocess.run(cmd, check=True)
    kept = out + ".kept"
    with open(out, errors="replace") as src, open(kept, "w") as dst:
        dst.writelines(line for line in src if DROP not in line)
    return kept


def differing_lines(a, b):
    """lines that `diff` reports as only in a or only in b"""
    r = subprocess.run(["diff", a, b], capture_output=True, text=True, errors="replace")
    if r.returncode > 1:
        raise SystemExit("diff failed: " + r.stderr)
    return sum(1 for line in r.stdout.split("\n") if line[:1] in ("<", ">"))


def main():
    argv = sys.argv[1:]
    def opt(name):                                           # by hand: the value of --extra begins with a dash
        if name in argv:
            k = argv.index(name); v = argv[k + 1]; del argv[k:k + 2]
            return v
        return None
    args = argparse.Namespace(extra=opt("--extra") or "", keep=opt("--keep"))
    if len(argv) != 1 or argv[0].startswith("-"):
        raise SystemExit(__doc__)
    args.other_csrc = argv[0]
    other, extra = os.path.abspath(args.other_csrc), args.extra.split()
    with tempfile.TemporaryDirectory(prefix="asm_identity_") as tmp:
        out = args.keep or tmp
        os.makedirs(out, exist_ok=True)
        jobs = [(side, csrc, unit) for unit in UNITS for side, csrc in (("this", _buildid.CSRC), ("other", other))]
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            futures = {(side, unit): pool.submit(compile_asm, csrc, unit, os.path.join(out, "%s.%s.s" % (unit, side)), extra) for side, csrc, unit in jobs}
            kept = {k: f.result() for k, f in futures.items()}
        print("device assembly of %s against %s%s" % (os.path.relpath(_buildid.CSRC, ROOT), args.other_csrc, ", extra flags: " + args.extra if extra else ""))
        print("%-24s %10s %10s" % ("unit", "lines", "differing"))
        total = 0
        for unit in UNITS:
            with open(kept["this", unit], errors="replace") as f:
                lines = sum(1 for _ in f)
            d = differing_lines(kept["this", unit], kept["other", unit])
            total += d
            print("%-24s %10d %10d" % (unit, lines, d))
        print("IDENTICAL" if total == 0 else "DIFFERENT: %d lines" % total)
        return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
