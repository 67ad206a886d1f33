#!/usr/bin/env python
"""Encoder wall span against its kernel time, per clip, from a rocprofv3 kernel trace of bench.py:
enc_span.py <kernel_trace.csv> [more traces ...]

The encoder of one forward runs from the split-stream centring pass (ln_split_kernel MODE 2, right behind the patch embedding) to
the end of its last tap LayerNorm (ln_split_kernel MODE 1; ViT-L: 4 per forward, 8 with the frame halves). Printed per trace: the
median over forwards of the wall span, the sum of the encoder kernels' durations, the time at least one of them runs (union), and
span - union = time with no encoder kernel on the chip (launch boundaries, empty queues)."""
import csv
import re
import statistics
import sys


def ln_split_mode(name):
    """MODE of an ln_split_kernel<LPR, NCH, MODE> (mangled or demangled name), else None."""
    m = re.search(r"ln_split_kernelILi\d+ELi\d+ELi(\d)EEEv", name) or re.search(r"ln_split_kernel<\d+, \d+, (\d)>", name)
    return int(m.group(1)) if m else None


def forwards(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if ln_split_mode(r[2]) == 2]
    for j, i0 in enumerate(starts):
        i1 = starts[j + 1] if j + 1 < len(starts) else len(rows)
        body = rows[i0:i1]
        taps = [k for k, r in enumerate(body) if ln_split_mode(r[2]) == 1]
        if not taps:
            continue
        t_end = max(body[k][1] for k in taps)
        enc = [r for r in body if r[0] < t_end]
        yield body[0][0], t_end, enc


def union(iv):
    tot, cur_s, cur_e = 0, None, None
    for s, e in sorted(iv):
        if cur_e is None or s > cur_e:
            if cur_e is not None:
                tot += cur_e - cur_s
            cur_s, cur_e = s, e
        else:
            cur_e = max(cur_e, e)
    return tot + (cur_e - cur_s if cur_e is not None else 0)


if __name__ == "__main__":
    for path in sys.argv[1:]:
        spans, sums, unions, counts = [], [], [], []
        for t0, t1, enc in forwards(path):
            spans.append((t1 - t0) / 1e6)
            sums.append(sum(e - s for s, e, _ in enc) / 1e6)
            unions.append(union([(s, e) for s, e, _ in enc]) / 1e6)
            counts.append(len(enc))
        if not spans:
            print(f"{path}: no encoder found")
            continue
        med = statistics.median
        print(f"{path}: {len(spans)} forwards, {med(counts):.0f} encoder kernels each; median ms per clip: span {med(spans):.3f}, "
              f"kernel sum {med(sums):.3f}, busy (union) {med(unions):.3f}, idle (span - union) {med(spans) - med(unions):.3f}; "
              f"spans {[round(v, 3) for v in spans]}")
