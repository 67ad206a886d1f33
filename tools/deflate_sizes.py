#!/usr/bin/env python
"""Sizes of the deflate encoder's streams (video_depth_anything_amd/deflate.py: the host twin, so no GPU is needed) beside zlib's raw
deflate at level 6, Z_RLE and Z_HUFFMAN_ONLY, and what the dynamic block header costs per coded chunk in three forms - the record
behind DESIGN.md 6k's header choice (profiles/deflate/sizes.txt):

  fixed     a fixed complete code-length code (lengths 0, 3..14 in 4 bits; 1, 2, 15..18 in 5), all 19 of its lengths listed, no repeat symbols
  built     a Huffman code of at most 7 bits built for the header's lengths, no repeat symbols: WHAT THE ENCODER WRITES
  repeats   the same with zlib's use of the repeat symbols 16, 17, 18

Inputs: the two fixture depth arrays of tests/golden and the synthetic inputs of tests/_deflate_inputs.py."""
import os
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _deflate_inputs as dinp  # noqa: E402
from video_depth_anything_amd import deflate  # noqa: E402


def zlib_raw(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, strategy)
    return len(c.compress(data)) + len(c.flush())


def built_bits(seq):
    """Header bits when the (symbol, repeat) tokens `seq` are written in a code built for them."""
    count = [0] * 19
    for s, _ in seq:
        count[s] += 1
    ln = deflate.code_lengths(count, deflate.CL_MAX_BITS)
    hclen = max(4, max(k + 1 for k, s in enumerate(deflate._CL_ORDER) if ln[s]))
    return 17 + 3 * hclen + sum(ln[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in seq)


def with_repeats(lens):
    """zlib's scan of a length sequence into tokens that use 16 (repeat the last 3..6 times), 17 and 18 (3..10, 11..138 zeros)."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k))
                run -= k
            if run >= 3:
                out.append((17, run))
                run = 0
            out += [(0, 1)] * run
        else:
            out.append((v, 1))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k))
                run -= k
            out += [(v, 1)] * run
        i = j
    return out


def main():
    print(f"{'input':28s} {'bytes':>8s} {'stream':>8s} {'level 6':>8s} {'Z_RLE':>8s} {'HUFFMAN':>8s} {'stored':>7s}   header bytes per coded chunk: fixed / built / repeats")
    for name, x in dinp.cases():
        data = x.tobytes()
        info = []
        s = deflate.deflate_numpy(x, info=info)
        assert zlib.decompress(s, -15) == data
        coded = [d for d in info if not d.get("stored", True)]
        fixed = built = rep = 0
        for d in coded:
            lens = d["lengths"]
            hlit = max(257, max(i for i, b in enumerate(lens) if b) + 1)
            seq = lens[:hlit] + [1 if d["matches"] else 0]
            fixed += 17 + 57 + sum(5 if v in (1, 2, 15) else 4 for v in seq)
            built += built_bits([(v, 1) for v in seq])
            rep += built_bits(with_repeats(seq))
            assert built_bits([(v, 1) for v in seq]) == d["header_bits"]
        k = max(1, len(coded))
        print(f"{name:28s} {len(data):8d} {len(s):8d} {zlib_raw(data, zlib.Z_DEFAULT_STRATEGY):8d} {zlib_raw(data, zlib.Z_RLE):8d} "
              f"{zlib_raw(data, zlib.Z_HUFFMAN_ONLY):8d} {len(info) - len(coded):3d}/{len(info):<3d}   {fixed / 8 / k:6.1f} / {built / 8 / k:6.1f} / {rep / 8 / k:6.1f}")


if __name__ == "__main__":
    main()
