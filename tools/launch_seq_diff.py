"""Compare the ordered kernel launches of two rocprofv3 --kernel-trace directories (two builds of the library, the same command):
python tools/launch_seq_diff.py <dir A> <dir B> [label]
A launch is (kernel name, grid, workgroup, LDS bytes), ordered by start time.  Prints one verdict line; on a difference also the first differing
position and, if the two multisets of launches are equal, that only the order differs."""
import collections
import csv
import glob
import sys


def launches(d):
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[-1]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    lds = next(c for c in rows[0] if "LDS" in c.upper())
    key = lambda r: (r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"), int(r[lds]))
    return [key(r) for r in rows]


a, b = launches(sys.argv[1]), launches(sys.argv[2])
label = sys.argv[3] if len(sys.argv) > 3 else sys.argv[1]
ours = lambda s: sum(1 for k in s if "hulc_" in k[0])
if a == b:
    print(f"{label}: IDENTICAL — {len(a)} launches ({ours(a)} of the library), {len(set(a))} distinct (name, grid, workgroup, LDS)")
    sys.exit(0)
i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
same_set = collections.Counter(a) == collections.Counter(b)
print(f"{label}: DIFFERENT — {len(a)} vs {len(b)} launches, first difference at position {i}; " + ("the same launches in another order" if same_set else "the sets of launches differ"))
for s, n in ((a, "A"), (b, "B")):
    for k in s[max(0, i - 1): i + 3]:
        print(f"    {n}: {k[0][:110]} grid={k[1]} wg={k[2]} lds={k[3]}")
sys.exit(1)
