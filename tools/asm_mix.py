"""Static instruction mix of the device functions in a gfx950 assembly listing
(the compiler's own -S output for the device side), per function and per
innermost loop.  Classes only, by mnemonic prefix: float64 VALU (v_*_f64),
other VALU (v_*), SALU (s_*), waits (s_waitcnt*), no-ops (s_nop), LDS (ds_*),
vector memory (global_* / flat_* / buffer_* / scratch_*).  Static counts, not a
profile: a loop body is an address range, dead alternatives included.

    hipcc --offload-arch=gfx950 <the build's flags> --offload-device-only -S \
        beta-sgp_amd/csrc/bsgp_persist.hip -o persist.s
    python3 tools/asm_mix.py persist.s [--match persist_ls] [--loops 6]

prints one line per function whose (mangled) name contains --match (default:
every function), then its --loops largest innermost loops.  A loop is a
backward branch to a label of the same function; it is innermost when no other
loop lies inside its range.  --enclosing lists the largest loops of any depth
instead (dN = enclosed by N loops): the row-pair loop of a row pass is the
depth-0 loop around its chunk, transform-stage and gather loops.
"""
import argparse
import re
import sys

CLASSES = ("f64", "valu", "salu", "wait", "nop", "lds", "vmem", "other")
_LABEL = re.compile(r"^([.\w$]+):")
_BRANCH = re.compile(r"^s_c?branch\w*\s+([.\w$]+)")


def classify(op):
    if op.startswith("v_"):
        return "f64" if op.endswith("_f64") or "_f64_" in op else "valu"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.split("_")[0] in ("global", "flat", "buffer", "scratch"):
        return "vmem"
    return "other"


def functions(path):
    """[(name, [(kind, text)], code bytes or None)]: kind 'L' label / 'I' instruction."""
    out, cur, name = [], None, None
    for raw in open(path, errors="replace"):
        line = raw.split(";")[0].strip() if not raw.lstrip().startswith(";") else ""
        m = re.match(r"^\s*;\s*codeLenInByte\s*=\s*(\d+)", raw)
        if m and out:
            out[-1][2] = int(m.group(1))
            continue
        if not line:
            continue
        if line.startswith(".type") and "@function" in line:
            name = line.split()[1].split(",")[0]
            continue
        lab = _LABEL.match(line)
        if lab:
            if name is not None and lab.group(1) == name:
                cur = [name, [], None]
                out.append(cur)
                name = None
            elif cur is not None:
                cur[1].append(("L", lab.group(1)))
            continue
        if line.startswith("."):
            if line.startswith(".size") or line.startswith(".section") or line.startswith(".text"):
                cur = None if line.startswith(".size") else cur
            continue
        if cur is not None:
            cur[1].append(("I", line))
    return out


def mix(items):
    c = dict.fromkeys(CLASSES, 0)
    for kind, text in items:
        if kind == "I":
            c[classify(text.split()[0])] += 1
    return c


def all_loops(items):
    """[(first index, last index)] of every loop of one function: a backward
    branch to a label; branches to one label make one loop, up to the last."""
    where = {t: i for i, (k, t) in enumerate(items) if k == "L"}
    last = {}
    for i, (k, t) in enumerate(items):
        m = _BRANCH.match(t) if k == "I" else None
        if m and m.group(1) in where and where[m.group(1)] < i:
            last[where[m.group(1)]] = i
    return sorted(last.items())


def innermost_loops(items):
    """The loops that enclose no other loop."""
    loops = all_loops(items)
    return [(a, b) for a, b in loops
            if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in loops)]


def depth(loop, loops):
    """How many other loops enclose `loop`."""
    a, b = loop
    return sum(1 for a2, b2 in loops if (a2, b2) != (a, b) and a2 <= a and b <= b2)


def fmt(c):
    n = sum(c.values())
    return (f"{n:7d} instr  f64 {c['f64']:6d} ({100 * c['f64'] // max(n, 1):2d} %)  valu {c['valu']:6d}  "
            f"salu {c['salu']:6d}  wait {c['wait']:5d}  nop {c['nop']:5d}  lds {c['lds']:5d}  "
            f"vmem {c['vmem']:5d}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("asm")
    ap.add_argument("--match", action="append", default=[])
    ap.add_argument("--loops", type=int, default=6)
    ap.add_argument("--enclosing", action="store_true",
                    help="list the largest loops of any nesting depth (the row-pair loops of a "
                         "pass enclose its chunk and gather loops), not only the innermost ones")
    a = ap.parse_args(argv)
    for name, items, nbytes in functions(a.asm):
        if a.match and not any(m in name for m in a.match):
            continue
        print(f"{name}\n  code {nbytes if nbytes is not None else '?'} B {fmt(mix(items))}")
        every = all_loops(items)
        cand = every if a.enclosing else innermost_loops(items)
        loops = sorted(cand, key=lambda ab: ab[0] - ab[1])[:a.loops]
        for lo, hi in sorted(loops):
            tag = f"d{depth((lo, hi), every)} " if a.enclosing else ""
            print(f"    loop {tag}@{items[lo][1]:<12s} {fmt(mix(items[lo:hi + 1]))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
