"""Which function bodies of two device assembly files differ.

    python tools/asm_function_identity.py OTHER.s THIS.s [--allow SUBSTRING ...]

For a change that is meant to touch some kernels of a unit and no others: `tools/asm_identity.py --keep DIR` leaves the gfx950 assembly of
every unit of both trees in DIR (`<unit>.other.s.kept`, `<unit>.this.s.kept`); this compares them function by function -- a body is
the text between a function's label and its `.Lfunc_end`, with the per-file function number in local labels (`.LBB16_3`, `.LJTI16_0`,
`.Ltmp41`) normalised, since one more function ahead of it renumbers them all.  Prints the functions that are missing, new or different;
exit status 1 if a function differs, or is missing or new, whose mangled name contains none of the --allow substrings."""
import hashlib
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        if name is None:
            m = re.match(r"^(_Z[\w$.]*):", line)
            if m:
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = (hashlib.sha1("".join(body).encode()).hexdigest(), len(body))
            name = None
        else:
            body.append(re.sub(r"\.L([A-Za-z_]+?)\d+", r".L\1N", line.split(";")[0].rstrip()) + "\n")      # (comments name basic blocks by the same number)
    return out


def main():
    args = sys.argv[1:]
    allow = []
    while "--allow" in args:
        i = args.index("--allow")
        allow.append(args[i + 1])
        del args[i:i + 2]
    a, b = functions(args[0]), functions(args[1])
    changed = sorted(set(a) ^ set(b)) + sorted(k for k in a if k in b and a[k] != b[k])
    print("functions: other %d, this %d; identical bodies %d" % (len(a), len(b), sum(1 for k in a if k in b and a[k] == b[k])))
    bad = 0
    for k in changed:
        what = "missing" if k not in b else "new" if k not in a else "differs (%d -> %d lines)" % (a[k][1], b[k][1])
        allowed = any(s in k for s in allow)
        bad += not allowed
        print("%s %s: %s" % ("  allowed" if allowed else "UNEXPECTED", k, what))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
