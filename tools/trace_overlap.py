#!/usr/bin/env python3
"""How the jump and the inner launches of a split jump-sampler run lie on the queues.

    python tools/trace_overlap.py <dir of a `rocprofv3 --kernel-trace --output-format csv` run> [lines]

Reads the kernel trace (*_kernel_trace.csv), keeps the flow-MH launches (`flow_mh_b*`: the jump) and the inner launches
(`mala_kernel`, `hmc_kernel`) and prints: the queues, how many jumps lie wholly inside an inner launch of ANOTHER queue
and how many overlap one partly, the median durations -- of all launches, and of the jumps and inner launches that have a
launch of the other kind on another queue beside them for their whole length or part of it -- and a stretch of the
timeline from the middle of the trace (the format of profiles/r06_*_trace_overlap.txt).
"""
import bisect
import csv
import glob
import os
import statistics
import sys


def load(d):
    rows = []
    for f in glob.glob(os.path.join(d, '**', '*kernel_trace.csv'), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r['Kernel_Name']
            kind = 'jump' if 'flow_mh_b' in name else ('inner' if ('mala_kernel' in name or 'hmc_kernel' in name) else None)
            if kind:
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), str(r['Queue_Id']), kind, name))
    return sorted(rows)


def beside(rows, kind):
    """Per launch of `kind`: 2 = wholly inside a launch of the other kind on another queue, 1 = overlaps one partly, 0."""
    other = [r for r in rows if r[3] != kind]
    starts = [r[0] for r in other]
    out = []
    for s, e, q, k, _ in rows:
        if k != kind:
            continue
        best = 0
        i = bisect.bisect_right(starts, e)
        for o in other[max(0, i - 16):i]:
            if o[2] == q or o[1] <= s or o[0] >= e:
                continue
            best = max(best, 2 if (o[0] <= s and o[1] >= e) else 1)
        out.append(best)
    return out


def main(d, lines=16):
    rows = load(d)
    jumps = [r for r in rows if r[3] == 'jump']
    inner = [r for r in rows if r[3] == 'inner']
    jb, ib = beside(rows, 'jump'), beside(rows, 'inner')
    med = lambda v: statistics.median(v) / 1e3 if v else float('nan')   # noqa: E731
    print('kernel trace: queues %s inner launches %d jumps %d inside an inner launch on another queue %d overlapping one partly %d'
          % (sorted({r[2] for r in rows}), len(inner), len(jumps), jb.count(2), jb.count(1)))
    print('  inner median us %.1f' % med([r[1] - r[0] for r in inner]))
    print('  jump median us %.1f' % med([r[1] - r[0] for r in jumps]))
    print('  inner median us beside a jump of another queue (partly or wholly) %.1f, not beside one %.1f'
          % (med([r[1] - r[0] for r, b in zip(inner, ib) if b]), med([r[1] - r[0] for r, b in zip(inner, ib) if not b])))
    print('  jump median us wholly inside an inner launch of another queue %.1f, partly %.1f, beside none %.1f'
          % (med([r[1] - r[0] for r, b in zip(jumps, jb) if b == 2]), med([r[1] - r[0] for r, b in zip(jumps, jb) if b == 1]),
             med([r[1] - r[0] for r, b in zip(jumps, jb) if b == 0])))
    mid = rows[len(rows) // 2:len(rows) // 2 + lines]
    for s, e, q, _, name in mid:
        print('q%-3s %-28s start %9.1f end %9.1f dur %7.1f us' % (q, name[:28], (s - mid[0][0]) / 1e3, (e - mid[0][0]) / 1e3, (e - s) / 1e3))


if __name__ == '__main__':
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 16)
