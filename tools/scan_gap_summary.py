#!/usr/bin/env python
"""Between consecutive single-query scans: idle time and overlap, from a rocprofv3 kernel trace of bench.py.
Usage: scan_gap_summary.py results.db [first] [count] [kernel-substring]
Takes the scan dispatches (default: names containing "scan_i8_kernel") in start order, skips `first` of them (default 50:
the warm-up steps) and looks at the next `count` (default 200: the timed steps).  Prints the gap from each scan's end
to the next scan's start (negative: they overlap), how many scans start before their predecessor ended, the scans' own
durations, and the share of the window -- first start to last end -- during which at least one scan ran."""
import glob
import sqlite3
import statistics
import sys


def main():
    path = sys.argv[1]
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    what = sys.argv[4] if len(sys.argv) > 4 else "scan_i8_kernel"
    if not path.endswith(".db"):
        path = sorted(glob.glob(path + "/**/*.db", recursive=True))[0]
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    name = "name" if "name" in cols else "kernel_name"
    qcol = next((q for q in ("queue_id", "stream_id") if q in cols), "0")
    rows = c.execute(f"select start, end, {qcol} from kernels where {name} like ? order by start", ("%" + what + "%",)).fetchall()
    print("== %s: %d dispatches of *%s*, looking at [%d, %d)" % (path, len(rows), what, first, first + count))
    rows = rows[first:first + count]
    if len(rows) < 2:
        print("(too few dispatches)")
        return
    gaps = [(rows[i + 1][0] - rows[i][1]) / 1e3 for i in range(len(rows) - 1)]
    durs = [(en - st) / 1e3 for st, en, _ in rows]
    overlapping = sum(g < 0 for g in gaps)
    # union of the scans' intervals
    covered, cur_s, cur_e = 0, rows[0][0], rows[0][1]
    for st, en, _ in rows[1:]:
        if st > cur_e:
            covered += cur_e - cur_s
            cur_s, cur_e = st, en
        else:
            cur_e = max(cur_e, en)
    covered += cur_e - cur_s
    window = max(en for _, en, _ in rows) - rows[0][0]
    q = sorted(gaps)
    print("queues used: %s" % sorted({r[2] for r in rows}))
    print("scan duration us: median %.1f  min %.1f  max %.1f" % (statistics.median(durs), min(durs), max(durs)))
    print("gap end -> next start us: median %.2f  p10 %.2f  p90 %.2f  min %.2f  max %.2f" % (
        statistics.median(gaps), q[len(q) // 10], q[len(q) * 9 // 10], q[0], q[-1]))
    print("scans that start before their predecessor ended: %d of %d" % (overlapping, len(gaps)))
    print("window %.1f us, at least one scan running for %.1f us: share %.4f" % (window / 1e3, covered / 1e3, covered / window))
    print("window per scan: %.2f us" % (window / 1e3 / len(rows)))


if __name__ == "__main__":
    main()
