"""Register table of the kernels from two compile logs taken with
``-Rpass-analysis=kernel-resource-usage`` (one "=== <source>[+<define>]" line per translation unit
of build.py's UNITS, then the compiler's remarks): per kernel VGPRs, SGPRs, scratch bytes per lane, occupancy and spill counts,
before -> after, as a markdown table.

usage: python scripts/resource_table.py BEFORE.log AFTER.log
"""
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch B"),
          ("Occupancy [waves/SIMD]", "occ"), ("SGPRs Spill", "SGPR spill"), ("VGPRs Spill", "VGPR spill")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    short = []
    for n in out[:len(names)]:
        n = n.replace("(anonymous namespace)::", "").replace("cmpc::", "")
        n = re.sub(r"^void ", "", n)
        n = re.sub(r"\(.*$", "", n)   # the name without its argument list
        # the wide kernels' fourth argument (the literal-model build) is not part of the comparison:
        # a literal build (row NV,P,R,1) is compared with the parent's build of the same class
        short.append(re.sub(r"(cmpc_solve_w_kernel<\d+, \w+, \w+), \w+>", r"\1>", n))
    return short


def unit(tu):
    """A log's unit label as the row of kWideBuild it builds: a log from before the build table names
    the wide units cmpc_wide_w<NV>[p][r][d].hip (128 and up were built refining without the r)."""
    m = re.fullmatch(r"cmpc_wide_w(\d+)(p?)(r?)(d?)\.hip", tu)
    if not m:
        return tu
    nv = int(m.group(1))
    return "cmpc_wide_unit.hip+CMPC_UNIT_WIDE=%d,%d,%d,%d" % (nv, bool(m.group(2)) or nv > 128,
                                                             bool(m.group(3)) or nv > 120, bool(m.group(4)))


def parse(path):
    table, tu, cur = {}, "?", None
    for line in open(path, errors="replace"):
        if line.startswith("=== "):
            tu = unit(line[4:].strip())
            continue
        m = re.search(r"remark:\s+(.*?): (.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2).strip()
        if key == "Function Name":   # (a unit compiled again later in the log replaces its earlier entry)
            cur = table[(tu, val)] = {}
        elif cur is not None:
            cur[key] = val
    return table


def main():
    # kernels are matched by unit and name: an added or moved argument type changes the mangled name
    def by_name(t):
        keys = list(t)   # in log order: a later compile of a unit replaces the earlier one
        return {(k[0], n): t[k] for k, n in zip(keys, demangle([k[1] for k in keys]))}
    before, after = by_name(parse(sys.argv[1])), by_name(parse(sys.argv[2]))
    print("| unit | kernel | " + " | ".join(h for _, h in FIELDS) + " |")
    print("|---|---|" + "---|" * len(FIELDS))
    changed = 0
    for tu, name in sorted(after):
        a = after[(tu, name)]
        b = before.get((tu, name)) or before.get((re.sub(r"(WIDE=\d+,\d,\d),1$", r"\1,0", tu), name), {})
        cells = []
        for f, _ in FIELDS:
            x, y = b.get(f, "-"), a.get(f, "-")
            cells.append(y if x == y else f"{x} -> {y}")
            changed += x != y
        print(f"| {tu} | `{name}` | " + " | ".join(cells) + " |")
    print(f"\n{len(after)} kernels, {changed} changed cells", file=sys.stderr)


if __name__ == "__main__":
    main()
