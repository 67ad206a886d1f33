#!/usr/bin/env python
"""Sizes of the EXR writer's files (video_depth_anything_amd/exr.py: the host twin, so no GPU is needed) beside the same container
filled by zlib.compress at level 6 on the same filtered blocks - what an OpenEXR build's ZIP writer stores - and beside the
uncompressed pixels: the record behind DESIGN.md 6l (profiles/exr/sizes.txt). Per input: frames, pixel bytes, the twin's files,
zlib's files, how many blocks each writes raw, and the twin's chunks that fell back to a stored deflate block.

Inputs: the two fixture depth arrays of tests/golden and the cases of tests/_exr_inputs.py."""
import os
import sys
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import _exr_inputs as xinp  # noqa: E402
from video_depth_anything_amd import deflate, exr  # noqa: E402


def stored_chunks(frame):
    """(stored, all) chunks of the twin over a frame's blocks."""
    stored = total = 0
    for y in range(0, frame.shape[0], exr.ZIP_LINES):
        f = exr.filter_bytes(np.ascontiguousarray(frame[y:y + exr.ZIP_LINES]).reshape(-1).view(np.uint8))
        k, q = exr.block_chunks(f.size)
        for c in range(k):
            info = {}
            deflate.encode_chunk(f[c * q:(c + 1) * q], c == k - 1, info)
            stored += bool(info["stored"])
            total += 1
    return stored, total


def main():
    inputs = [(name, xinp.fixture_depths(name)) for name in ("tiny_video", "tiny_metric_video")] + [(name, xinp.case(name)) for name in xinp.names()]
    print(f"{'input':28s} {'shape':>14s} {'pixels':>9s} {'twin':>9s} {'ratio':>6s} {'zlib 6':>9s} {'ratio':>6s}   raw blocks twin / zlib / all   stored chunks")
    for name, d in inputs:
        twin = zl = raw_t = raw_z = blocks = stored = chunks = 0
        for frame in d:
            ft, fz = [], []
            a = exr.encode_exr_numpy(frame, info=ft)
            b = exr.encode_exr_numpy(frame, compress=lambda x: zlib.compress(x, 6), info=fz)
            assert exr.read_exr(a)["Z"].tobytes() == exr.read_exr(b)["Z"].tobytes() == np.ascontiguousarray(frame).tobytes()
            twin, zl, blocks = twin + len(a), zl + len(b), blocks + len(ft)
            raw_t, raw_z = raw_t + ft.count(False), raw_z + fz.count(False)
            s, c = stored_chunks(frame)
            stored, chunks = stored + s, chunks + c
        print(f"{name:28s} {'x'.join(map(str, d.shape)):>14s} {d.nbytes:9d} {twin:9d} {twin / d.nbytes:6.3f} {zl:9d} {zl / d.nbytes:6.3f}   "
              f"{raw_t:4d} / {raw_z:4d} / {blocks:<4d}             {stored:4d} / {chunks:<4d}")


if __name__ == "__main__":
    main()
