"""Developer: the per-kernel table of a built library, and the difference between two builds.
    python scripts/dev/kernel_table.py bear_amd/libbear_hip.so                 # the table
    python scripts/dev/kernel_table.py before/libbear_hip.so bear_amd/libbear_hip.so    # what differs; exit status 1 if anything does
One line per kernel of every gfx950 code object in the library: code object (in link order), mangled name, vector and scalar
registers, scratch and LDS bytes (the code object's metadata note) and the size of the kernel's code (its symbol).  A library
links one code object per unit, and a kernel belongs to exactly one of them: a change that only moves host code or regroups the
units leaves every line but the first column as it was.  The comparison therefore ignores that column and reports kernels that
are missing, new, emitted more than once, or whose numbers moved (kernel_resources.py does the same from two assembly dumps and
marks a changed occupancy)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_objects(lib):
    """The gfx950 code objects bundled in `lib`, extracted into a temporary directory, in bundle order."""
    tmp = tempfile.mkdtemp(prefix="kernel_table_")
    local = os.path.join(tmp, "lib.so")
    os.symlink(os.path.abspath(lib), local)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], check=True, cwd=tmp, stdout=subprocess.DEVNULL)
    names = [n for n in os.listdir(tmp) if "gfx950" in n]
    return [os.path.join(tmp, n) for n in sorted(names, key=lambda n: [int(x) for x in re.findall(r"\.(\d+)\.", n)])]


def kernels_of(obj):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True, text=True).stdout
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-s", "-W", obj], check=True, capture_output=True, text=True).stdout
    size = {}
    for line in syms.splitlines():
        p = line.split()
        if len(p) >= 8 and p[3] == "FUNC":
            size[p[7]] = int(p[2], 0)
    out, cur, inside = [], None, False
    for line in notes.splitlines():     # amdhsa.kernels: a list of maps, "  - .key: v" opens one, "    .key: v" goes on (deeper: its arguments)
        if not line.startswith(" "):
            inside, cur = line.startswith("amdhsa.kernels:"), None
            continue
        m = re.match(r"^  (- |  )\.(\w+):\s*(\S*)\s*$", line)
        if not inside or not m:
            continue
        if m.group(1) == "- ":
            cur = {}
            out.append(cur)
        cur[m.group(2)] = m.group(3)
    return [(k["name"],) + tuple(int(k[f]) for f in FIELDS) + (size[k["name"]],) for k in out]


def table(lib):
    rows = []
    for i, obj in enumerate(code_objects(lib)):
        rows += [(i,) + r for r in kernels_of(obj)]
    return rows


def fmt(r):
    return "%d %s vgpr=%d sgpr=%d scratch=%d lds=%d code=%d" % r


def by_name(rows):
    d = {}
    for r in rows:
        d.setdefault(r[1], []).append(r[2:])
    return d


if __name__ == "__main__":
    if len(sys.argv) == 2:
        for r in table(sys.argv[1]):
            print(fmt(r))
        sys.exit(0)
    a, b = by_name(table(sys.argv[1])), by_name(table(sys.argv[2]))
    bad = 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        if ra is None or rb is None:
            print("only in", sys.argv[2 if ra is None else 1], name)
        elif len(ra) != 1 or len(rb) != 1:
            print("emitted %d / %d times" % (len(ra), len(rb)), name)
        elif ra != rb:
            print("differs", name, dict(zip(FIELDS + ("code",), ra[0])), "->", dict(zip(FIELDS + ("code",), rb[0])))
        else:
            continue
        bad += 1
    print("%d kernels / %d kernels, %d differences" % (sum(map(len, a.values())), sum(map(len, b.values())), bad))
    sys.exit(1 if bad else 0)
