"""Static figures of the tracking step: the two in-place repeat loops of wg_block (volpath_flat.h) in one device unit's assembly.

    python tools/step_loop_stats.py [unit.hip] [--kernel SUBSTRING] [--source DIR] [--asm FILE] [--keep FILE] [--histogram] [--trips] [--chain]

Compiles the unit (default kernels_lean_a.hip) for the device only, to assembly, with the product flags of _buildid.py plus line
tables (about 30 s; the added flags do not change the code), and finds the loops of the chosen kernel (default: the flagship,
render_kernel_wga<false, 1024, 1024, 4, false>) through the line table -- no marker in the kernel source, which would change the
code it measures:

  * a loop is the natural loop (control-flow graph of the kernel's basic blocks) of a branch that goes backward in the layout;
  * the repeat loops are the smallest loops that hold an instruction of the line of wg_block's `MTS_REPEAT_MIN` test;
  * the one with an instruction of a line that forms the roulette probability (main path's loop head) is B_MED, the one with a line
    that forms an NEE walk's remaining distance is B_MEDW;
  * the common path of a loop leaves out the blocks that only the branch on `__ballot(rare)` reaches (step_fast's rare path).

Instructions are COUNTED by mnemonic prefix / substring only (s_, v_, ds_, global_, scratch_, *_f64, *_f32, *mov*, *saveexec*,
*cbranch*, s_*_b64); a *saveexec* opens a divergent region.  --histogram adds the count of every mnemonic.  The control-flow graph
needs more than a class: a mnemonic with `branch` in it ends a block and names a successor, and two are known by name -- `s_branch`
(no fall-through) and `s_endpgm` (no successor).

--trips adds, for the common path of each loop, the memory instructions (global_load*, s_load*, ds_read*) and the s_waitcnt between them
in control-flow order from the loop head, and says whether (a) the grid gathers, (b) the medium record's scalar loads go out in one
round trip each, and (c) the logarithm's table read is issued ahead of the record (trips(), tests/test_step_round_trips.py).

--chain adds what of the step's table reads (ds_read*) and fp64 arithmetic (*_f64) stands behind the wait for the grid gathers, on the
voxels' chain (chain(), tests/test_step_chain.py).

The anchors are literal texts of source lines of volpath_flat.h (comments at those lines say so) and, for --trips, of cload's copy
loop in integrator_dev.h: a reworded line makes the tool stop with a message that names the anchor.
"""
import contextlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "eradiate-kernel_amd")
sys.path.insert(0, PKG)
import _buildid  # noqa: E402

HEADER = "volpath_flat.h"
REPEAT_ANCHOR = "MTS_REPEAT_MIN_W : MTS_REPEAT_MIN"     # the lane-count test at the foot of wg_block's repeat loop
MAIN_ANCHOR = "(p.eta * p.eta), .95f)"                  # Russian roulette at the main path's loop head: B_MED only
RARE_ANCHOR = "__ballot(rare)"                          # the one wave-uniform branch to the general step (VolpathMachine::step_fast)
WALK_ANCHOR = "(1.f - MTS_SHADOW_EPSILON) - "           # the distance an NEE walk has left, at its loop head: B_MEDW only
DEFAULT_KERNEL = "render_kernel_wga<false, 1024, 1024, 4, false>"
COLUMNS = ["instructions", "basic blocks", "no source line", "s_", "v_", "ds_", "global_", "scratch_", "exec-mask logic (s_*_b64, *saveexec*)",
           "divergent regions (*saveexec*)", "*cbranch*", "*cbranch* on exec", "s_ *mov*", "v_ *mov*", "*_f32", "*_f64"]


def compile_asm(unit, out):
    flags = [f for f in _buildid.FLAGS if f not in ("-shared", "-fPIC")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-gline-tables-only", "-x", "hip", os.path.join(SOURCE_DIR, unit), "-o", out]
    subprocess.run(cmd, check=True)


SOURCE_DIR = _buildid.CSRC                               # --source DIR: the csrc/ the assembly was compiled from (another revision)


def anchor_lines(text):
    """numbers of the code lines (not comment lines) of volpath_flat.h that hold `text`"""
    with open(os.path.join(SOURCE_DIR, HEADER)) as f:
        return {n for n, line in enumerate(f, 1) if text in line and not line.lstrip().startswith("//")}


def parse_kernel(asm_path, kernel):
    """-> (instructions of the kernel [(mnemonic, operands, (file name, line) or None)], {label: index of its first instruction})"""
    files, lines = {}, open(asm_path, errors="replace").read().split("\n")
    names = [m.group(1) for m in (re.match(r"^(_Z\w+):", l) for l in lines) if m]
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    want = [n for n, d in zip(names, dem) if kernel in d]
    if len(want) != 1:
        raise SystemExit("kernel %r matches %d functions of %s" % (kernel, len(want), asm_path))
    insts, labels, inside, loc = [], {}, False, None
    for l in lines:
        m = re.match(r'^\s+\.file\s+(\d+)\s+(?:"([^"]*)"\s+)?"([^"]*)"', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3))
            continue
        if not inside:
            inside = l.startswith(want[0] + ":")
            continue
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"^(\.LBB\w+):", l)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        m = re.match(r"^\s+\.loc\s+(\d+)\s+(\d+)", l)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        m = re.match(r"^\s+([a-z]\w*)\s*(.*?)\s*(?:;.*)?$", l)
        if m:
            insts.append((m.group(1), m.group(2), loc if loc and loc[1] else None))
    return insts, labels


def blocks_of(insts, labels):
    """basic blocks [(first, last)] in layout order and their successors (indices of blocks)"""
    starts = {0} | set(labels.values()) | {k + 1 for k, (mn, _, _) in enumerate(insts) if "branch" in mn or mn.startswith("s_endpgm")}
    starts = sorted(s for s in starts if s < len(insts))
    blocks = [(s, (starts[k + 1] if k + 1 < len(starts) else len(insts)) - 1) for k, s in enumerate(starts)]
    at = {s: k for k, s in enumerate(starts)}
    succ = []
    for k, (first, last) in enumerate(blocks):
        mn, ops, _ = insts[last]
        out = []
        if "branch" in mn:
            tgt = labels.get(ops.split(",")[-1].strip())
            if tgt is not None and tgt in at:
                out.append(at[tgt])
        if not (mn == "s_branch" or mn.startswith("s_endpgm")) and k + 1 < len(blocks):
            out.append(k + 1)
        succ.append(out)
    return blocks, succ


def dominators(succ):
    """immediate dominators of the blocks reachable from block 0 (Cooper, Harvey, Kennedy)"""
    order, seen, stack = [], {0}, [(0, iter(succ[0]))]
    while stack:
        node, it = stack[-1]
        nxt = next((o for o in it if o not in seen), None)
        if nxt is None:
            order.append(node); stack.pop()
        else:
            seen.add(nxt); stack.append((nxt, iter(succ[nxt])))
    rank = {b: k for k, b in enumerate(order)}              # postorder number
    pred = {b: [] for b in order}
    for b in order:
        for o in succ[b]:
            pred[o].append(b)
    idom = {0: 0}
    changed = True
    while changed:
        changed = False
        for b in reversed(order):
            if b == 0:
                continue
            new = None
            for q in pred[b]:
                if q not in idom:
                    continue
                if new is None:
                    new = q
                    continue
                x, y = q, new
                while x != y:
                    while rank[x] < rank[y]:
                        x = idom[x]
                    while rank[y] < rank[x]:
                        y = idom[y]
                new = x
            if idom.get(b) != new:
                idom[b] = new; changed = True
    return idom, pred


def loops(insts, labels):
    """natural loops of the kernel: sets of block indices (one per loop header), with the block list"""
    blocks, succ = blocks_of(insts, labels)
    idom, pred = dominators(succ)
    def dominates(a, b):
        while b != a and b != 0:
            b = idom[b]
        return b == a
    merged = {}                                              # several latches of one header: one loop
    for latch in idom:
        for header in succ[latch]:
            if not dominates(header, latch):
                continue
            body, todo = {header, latch}, [latch] if latch != header else []
            while todo:
                for q in pred[todo.pop()]:
                    if q not in body:
                        body.add(q); todo.append(q)
            merged.setdefault(header, set()).update(body)
    return blocks, list(merged.values()), (succ, dominates)


def stats(insts, blocks, body_blocks):
    body = [insts[k] for b in sorted(body_blocks) for k in range(blocks[b][0], blocks[b][1] + 1)]
    mns = [mn for mn, _, _ in body]
    s = dict.fromkeys(COLUMNS, 0)
    s["instructions"] = len(body)
    s["basic blocks"] = len(body_blocks)
    s["no source line"] = sum(1 for _, _, loc in body if loc is None)
    for mn, ops, _ in body:
        for p in ("s_", "v_", "ds_", "global_", "scratch_"):
            if mn.startswith(p):
                s[p] += 1
        if "saveexec" in mn or (mn.startswith("s_") and mn.endswith("_b64")):
            s["exec-mask logic (s_*_b64, *saveexec*)"] += 1
        if "saveexec" in mn:
            s["divergent regions (*saveexec*)"] += 1
        if "cbranch" in mn:
            s["*cbranch*"] += 1
            if "exec" in mn:
                s["*cbranch* on exec"] += 1
        if "mov" in mn and mn[:2] in ("s_", "v_"):
            s[mn[:2] + " *mov*"] += 1
        if "_f32" in mn:
            s["*_f32"] += 1
        if "_f64" in mn:
            s["*_f64"] += 1
    hist = {}
    for mn in mns:
        hist[mn] = hist.get(mn, 0) + 1
    return s, hist


def find_loops(asm_path, kernel=DEFAULT_KERNEL):
    """-> (insts, blocks, succ, dominates, {"B_MED": (blocks of the loop, blocks of its common path), "B_MEDW": (...)})"""
    insts, labels = parse_kernel(asm_path, kernel)
    repeat, main, walk = anchor_lines(REPEAT_ANCHOR), anchor_lines(MAIN_ANCHOR), anchor_lines(WALK_ANCHOR)
    for name, text, lines in (("REPEAT_ANCHOR", REPEAT_ANCHOR, repeat), ("MAIN_ANCHOR", MAIN_ANCHOR, main), ("WALK_ANCHOR", WALK_ANCHOR, walk)):
        if not lines:
            raise SystemExit("no code line of %s holds %s = %r any more: the line was reworded -- give tools/step_loop_stats.py its new text"
                             % (os.path.join(SOURCE_DIR, HEADER), name, text))
    blocks, found, (succ, dominates) = loops(insts, labels)
    rare = anchor_lines(RARE_ANCHOR)
    def has(body, lines):
        return any(loc is not None and loc[0] == HEADER and loc[1] in lines for b in body for _, _, loc in insts[blocks[b][0]:blocks[b][1] + 1])
    cand = sorted((body for body in found if has(body, repeat)), key=lambda body: sum(blocks[b][1] - blocks[b][0] + 1 for b in body))
    out = {}
    for body in cand:                                       # smallest first: a repeat loop lies inside the driver's loops
        if any(prev <= body for prev in out.values()):
            continue
        is_main, is_walk = has(body, main), has(body, walk)
        if is_main != is_walk:
            out.setdefault("B_MED" if is_main else "B_MEDW", body)
    if sorted(out) != ["B_MED", "B_MEDW"]:
        raise SystemExit("found the repeat loops %s, not one each of B_MED and B_MEDW: %d loops of %r hold an instruction of the REPEAT_ANCHOR line; "
                         "one must hold a MAIN_ANCHOR line and no WALK_ANCHOR line, one the reverse (see the anchors' comments)" % (sorted(out), len(cand), kernel))
    res = {}
    for name, body in out.items():
        # the common path: the loop without the blocks that only the wave-uniform branch to the rare path reaches (the side of that
        # branch which does not lead on to the repeat test by itself); a source without such a branch has none
        common = set(body)
        for b in body:
            mn, _, loc = insts[blocks[b][1]]
            if "cbranch" in mn and loc is not None and loc[0] == HEADER and loc[1] in rare:
                for s_ in succ[b]:
                    side = {x for x in body if dominates(s_, x)}
                    if not has(side, repeat):
                        common -= side
        res[name] = (body, common)
    return insts, blocks, succ, dominates, res


def step_loops(asm_path, kernel=DEFAULT_KERNEL):
    """-> {"B_MED": (stats, histogram, stats of the common path, its histogram), "B_MEDW": (...)} of the kernel in an assembly file"""
    insts, blocks, _, _, found = find_loops(asm_path, kernel)
    return {name: stats(insts, blocks, body) + stats(insts, blocks, common) for name, (body, common) in found.items()}


# --trips: the memory round trips of the common path.  A round trip is a load and the s_waitcnt that waits for it; two loads of one kind
# with such a wait between them on some path are two DEPENDENT trips -- the second is issued only when the first has come back.
RECORD_FILE, RECORD_ANCHOR = "integrator_dev.h", "tmp[k] = src[k];"     # cload: the scalar loads of a scene record (the step's: its medium)
MEMORY = ("global_load", "s_load", "ds_read")


def trips(asm_path, kernel=DEFAULT_KERNEL):
    """-> {"B_MED": {"listing": [text lines], "a": [...], "b": [...], "c": [...]}, "B_MEDW": {...}}: the memory instructions and waits
    of each repeat loop's common path in control-flow order from the loop head, and the instructions that break each rule (empty: kept)

      a  no path leads from one global_load_dwordx4 to another through an s_waitcnt that names vmcnt
      b  no path leads from one s_load of the medium record to another through an s_waitcnt that names lgkmcnt
      c  every path from the loop head meets a ds_read_b128 (the logarithm's table) before the first s_load of the medium record

    Paths run inside the common path and stop at a back edge -- the repeat loop's own and the waterfall's, whose second trip is another
    medium's lookup."""
    insts, blocks, succ, dominates, found = find_loops(asm_path, kernel)
    with open(os.path.join(SOURCE_DIR, RECORD_FILE)) as f:
        record_lines = {n for n, line in enumerate(f, 1) if RECORD_ANCHOR in line and not line.lstrip().startswith("//")}
    if not record_lines:
        raise SystemExit("no code line of %s holds RECORD_ANCHOR = %r any more: give tools/step_loop_stats.py its new text" % (RECORD_FILE, RECORD_ANCHOR))
    def is_record(k):
        mn, _, loc = insts[k]
        return mn.startswith("s_load") and loc is not None and loc[0] == RECORD_FILE and loc[1] in record_lines
    def is_gather(k):
        return insts[k][0] == "global_load_dwordx4"
    def waits(k, counter):
        return insts[k][0] == "s_waitcnt" and counter in insts[k][1]
    res = {}
    for name, (body, common) in found.items():
        head = next(b for b in common if all(dominates(b, x) for x in common))
        fwd = {b: [s for s in succ[b] if s in common and not dominates(s, b)] for b in common}      # no back edges: acyclic
        order, seen = [], set()
        def visit(b):
            seen.add(b)
            for s in sorted(fwd[b], reverse=True):
                if s not in seen:
                    visit(s)
            order.append(b)
        visit(head)
        order.reverse()                                      # reverse postorder: every block after all its predecessors
        listing = []
        for b in order:
            for k in range(blocks[b][0], blocks[b][1] + 1):
                mn, ops, loc = insts[k]
                if mn.startswith(MEMORY) or mn.startswith("s_waitcnt"):
                    listing.append("  block %-4d %-22s %-26s %s%s" % (b, "%s:%d" % loc if loc else "-", mn, ops, "   <- medium record" if is_record(k) else ""))
        # one forward pass of a small state machine per rule; a block's entry states are the union of its predecessors' exit states
        def run(start, step):
            state, broken = {b: set() for b in order}, []
            state[head] = {start}
            for b in order:
                cur = set(state[b])
                for k in range(blocks[b][0], blocks[b][1] + 1):
                    cur = step(k, cur, broken)
                for s in fwd[b]:
                    state[s] |= cur
            return ["%s:%d %s %s" % ((insts[k][2] or ("-", 0)) + insts[k][:2]) for k in broken]
        def two_trips(is_load, counter):                     # states: 0 no load yet, 1 a load in flight, 2 a load, then a wait for it
            def step(k, cur, broken):
                if is_load(k):
                    if 2 in cur:
                        broken.append(k)
                    return {1}
                if waits(k, counter):
                    return {2 if s == 1 else s for s in cur}
                return cur
            return step
        def log_first(k, cur, broken):                       # states: 0 no ds_read_b128 yet, 1 seen
            if insts[k][0] == "ds_read_b128":
                return {1}
            if is_record(k) and 0 in cur:
                broken.append(k)
                return {1}                                   # named once: the record's first load
            return cur
        res[name] = {"listing": listing, "a": run(0, two_trips(is_gather, "vmcnt")), "b": run(0, two_trips(is_record, "lgkmcnt")),
                     "c": run(0, log_first)}
    return res


def render_trips(res):
    rows = []
    for name in ("B_MED", "B_MEDW"):
        r = res[name]
        rows.append("%s, common path: memory instructions and waits in control-flow order from the loop head" % name)
        rows += r["listing"]
        for rule, text in (("a", "the gathers (global_load_dwordx4) go out in one round trip: no vmcnt wait between two of them"),
                           ("b", "the medium record's s_load go out in one round trip: no lgkmcnt wait between two of them"),
                           ("c", "the logarithm's table read (ds_read_b128) is issued before the medium record's first s_load")):
            rows.append("  (%s) %s: %s" % (rule, text, "yes" if not r[rule] else "NO -- " + "; ".join(r[rule])))
    return "\n".join(rows)


def chain(asm_path, kernel=DEFAULT_KERNEL):
    """-> {"B_MED": {"behind": [...], "reads": {"ds_read_b128": n, "ds_read_b64": n}}, "B_MEDW": {...}}: what of the step's table reads
    and fp64 arithmetic (the logarithm, the exponential) stands on the voxels' chain.

      behind  the instructions of the common path that are a ds_read* or carry _f64 in the mnemonic and lie on some path from the
              gathers' wait -- the first s_waitcnt that names vmcnt behind a global_load_dwordx4 -- to the loop's back edge
      reads   how many ds_read_b128 (the logarithm's table) and ds_read_b64 (the exponential's) the common path holds

    Paths run inside the common path and stop at a back edge, as in trips()."""
    insts, blocks, succ, dominates, found = find_loops(asm_path, kernel)
    res = {}
    for name, (body, common) in found.items():
        head = next(b for b in common if all(dominates(b, x) for x in common))
        fwd = {b: [s for s in succ[b] if s in common and not dominates(s, b)] for b in common}
        order, seen, stack = [], {head}, [(head, iter(sorted(fwd[head], reverse=True)))]
        while stack:                                         # reverse postorder: every block after all its predecessors
            b, it = stack[-1]
            nxt = next((s for s in it if s not in seen), None)
            if nxt is None:
                order.append(b); stack.pop()
            else:
                seen.add(nxt); stack.append((nxt, iter(sorted(fwd[nxt], reverse=True))))
        order.reverse()
        state, behind = {b: set() for b in order}, []        # states: 0 no gather yet, 1 a gather in flight, 2 behind the gathers' wait
        state[head] = {0}
        for b in order:
            cur = set(state[b])
            for k in range(blocks[b][0], blocks[b][1] + 1):
                mn, ops, loc = insts[k]
                if mn == "global_load_dwordx4":
                    cur = {1 if s == 0 else s for s in cur}
                elif mn == "s_waitcnt" and "vmcnt" in ops:
                    cur = {2 if s == 1 else s for s in cur}
                elif 2 in cur and (mn.startswith("ds_read") or "_f64" in mn):
                    behind.append("%s:%d %s %s" % ((loc or ("-", 0)) + (mn, ops)))
            for s in fwd[b]:
                state[s] |= cur
        mns = [insts[k][0] for b in common for k in range(blocks[b][0], blocks[b][1] + 1)]
        res[name] = {"behind": behind, "reads": {m: mns.count(m) for m in ("ds_read_b128", "ds_read_b64")}}
    return res


def render_chain(res):
    rows = []
    for name in ("B_MED", "B_MEDW"):
        r = res[name]
        rows.append("%s, common path: %d ds_read_b128, %d ds_read_b64; table reads and fp64 arithmetic behind the gathers' wait: %s"
                    % (name, r["reads"]["ds_read_b128"], r["reads"]["ds_read_b64"], "none" if not r["behind"] else len(r["behind"])))
        rows += ["  " + l for l in r["behind"]]
    return "\n".join(rows)


@contextlib.contextmanager
def compiled(unit="kernels_lean_a.hip", keep=None):
    """the unit's assembly, compiled now: at `keep`, or in a temporary directory that lives as long as the block"""
    with tempfile.TemporaryDirectory(prefix="step_loop_") as tmp:
        asm = keep or os.path.join(tmp, "unit.s")
        compile_asm(unit, asm)
        yield asm


def measure(unit="kernels_lean_a.hip", kernel=DEFAULT_KERNEL, keep=None):
    with compiled(unit, keep) as asm:
        return step_loops(asm, kernel)


def render(res, unit, kernel, histogram=False):
    rows = ["repeat loops of wg_block in %s, kernel %s" % (unit, kernel),
            "common path: the loop without the blocks behind its branch to the rare path (the general step); the same as the loop where there is none",
            "%-46s %8s %8s %14s %14s" % ("", "B_MED", "B_MEDW", "B_MED common", "B_MEDW common")]
    for c in COLUMNS:
        rows.append("%-46s %8d %8d %14d %14d" % (c, res["B_MED"][0][c], res["B_MEDW"][0][c], res["B_MED"][2][c], res["B_MEDW"][2][c]))
    if histogram:
        rows.append("mnemonics:")
        cols = [res["B_MED"][1], res["B_MEDW"][1], res["B_MED"][3], res["B_MEDW"][3]]
        for n in sorted(set().union(*cols), key=lambda n: (-sum(c.get(n, 0) for c in cols), n)):
            rows.append("  %-44s %8d %8d %14d %14d" % ((n,) + tuple(c.get(n, 0) for c in cols)))
    return "\n".join(rows)


if __name__ == "__main__":
    argv = sys.argv[1:]
    def opt(name):
        if name in argv:
            k = argv.index(name); v = argv[k + 1]; del argv[k:k + 2]
            return v
        return None
    kernel, asm, keep = opt("--kernel") or DEFAULT_KERNEL, opt("--asm"), opt("--keep")
    SOURCE_DIR = opt("--source") or SOURCE_DIR
    histogram, want_trips, want_chain = "--histogram" in argv, "--trips" in argv, "--chain" in argv
    argv = [a for a in argv if a not in ("--histogram", "--trips", "--chain")]
    unit = argv[0] if argv else "kernels_lean_a.hip"
    with (contextlib.nullcontext(asm) if asm else compiled(unit, keep)) as asm:
        print(render(step_loops(asm, kernel), unit, kernel, histogram))
        if want_trips:
            print(render_trips(trips(asm, kernel)))
        if want_chain:
            print(render_chain(chain(asm, kernel)))
