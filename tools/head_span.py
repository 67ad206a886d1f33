#!/usr/bin/env python
"""DPT head wall span against its kernel time, per clip, from a rocprofv3 kernel trace of bench.py (what enc_span.py does for the
encoder): head_span.py <kernel_trace.csv> [more traces ...]

The head of one forward runs from the end of the encoder's last tap LayerNorm (ln_split_kernel MODE 1: the join of the frame
halves) to the end of depth_tail_up_kernel. Printed per trace: the median over forwards of the wall span, the sum of the head
kernels' durations, the time at least one of them runs (union) and span - union. With option head_lanes the head's kernels run on
two streams: idle time that was filled shows as a shorter span under a kernel sum that is no smaller."""
import csv
import statistics
import sys

from enc_span import ln_split_mode, union


def heads(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if ln_split_mode(r[2]) == 2]
    for j, i0 in enumerate(starts):
        body = rows[i0:starts[j + 1] if j + 1 < len(starts) else len(rows)]
        taps = [r[1] for r in body if ln_split_mode(r[2]) == 1]
        tails = [r[1] for r in body if "depth_tail_up_kernel" in r[2]]
        if not taps or not tails:
            continue
        t0, t1 = max(taps), max(tails)
        yield t0, t1, [r for r in body if t0 <= r[0] < t1]


if __name__ == "__main__":
    for path in sys.argv[1:]:
        spans, sums, unions, counts = [], [], [], []
        for t0, t1, ks in heads(path):
            spans.append((t1 - t0) / 1e6)
            sums.append(sum(e - s for s, e, _ in ks) / 1e6)
            unions.append(union([(s, e) for s, e, _ in ks]) / 1e6)
            counts.append(len(ks))
        if not spans:
            print(f"{path}: no head found")
            continue
        med = statistics.median
        print(f"{path}: {len(spans)} forwards, {med(counts):.0f} head kernels each; median ms per clip: span {med(spans):.3f}, "
              f"kernel sum {med(sums):.3f}, busy (union) {med(unions):.3f}, idle (span - union) {med(spans) - med(unions):.3f}; "
              f"spans {[round(v, 3) for v in spans]}")
