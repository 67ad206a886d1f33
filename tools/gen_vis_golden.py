#!/usr/bin/env python
"""Write tests/golden/vis_frames.npz: the frames the REFERENCE's utils/dc_utils.py save_video hands to its video writer for the
three depth cases of tests/_visualize_inputs.py, in colour and in gray, and the colour table it indexed.

    python tools/gen_vis_golden.py --reference <reference checkout> [--check]

The reference's module is imported at run time from that checkout; nothing of it is copied. Two things stand between its
save_video and a result on a machine without an H.264 encoder, both arranged from outside the module: a stand-in `imageio` in
sys.modules whose get_writer returns an object that records every append_data, and a stand-in `cv2` when neither decord nor cv2
is importable (the module imports one of them at the top; save_video calls neither). matplotlib must be importable (where it no
longer has `cm.get_cmap`, that name is bound to `matplotlib.colormaps.get_cmap`): the table is
the reference's own `cm.get_cmap("inferno").colors`, recorded as the bytes save_video makes of it, (colors * 255).astype(uint8).

Per case the fixture holds the depth, the colour frames [N,H,W,3] and the gray frames [N,H,W]. Checked here before anything is
written: every colour frame is table[gray frame] (so the reference's float lookup followed by a multiply is one uint8 gather),
case B uses every one of the 256 rows with row 255 at the maximum only, and no case holds a non-finite value or leaves its own
[min, max] - the region where numpy's astype(uint8) is defined. --check regenerates everything and compares it with the committed
file bit for bit. No test imports this tool or the reference.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
from _visualize_inputs import CASES, GOLDEN, case  # noqa: E402


class _Recorder:
    """What imageio.get_writer returns here: keeps the frames save_video appends."""
    last = None

    def __init__(self, path, **kwargs):
        self.path, self.kwargs, self.frames, self.closed = path, kwargs, [], False
        _Recorder.last = self

    def append_data(self, frame):
        self.frames.append(np.array(frame))

    def close(self):
        self.closed = True


def import_reference(root):
    imageio = types.ModuleType("imageio")
    imageio.get_writer = _Recorder
    sys.modules["imageio"] = imageio
    try:
        importlib.import_module("decord")
    except ImportError:
        try:
            importlib.import_module("cv2")
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    import matplotlib
    import matplotlib.cm as cm
    if not hasattr(cm, "get_cmap"):                      # matplotlib >= 3.11 drops the spelling the reference uses
        cm.get_cmap = matplotlib.colormaps.get_cmap
    sys.path.insert(0, os.path.abspath(root))
    return importlib.import_module("utils.dc_utils")


def run_reference(ref, depth, grayscale):
    ref.save_video(depth, "unused.mp4", fps=24, is_depths=True, grayscale=grayscale)
    rec = _Recorder.last
    assert rec.closed and len(rec.frames) == depth.shape[0]
    out = np.stack(rec.frames)
    assert out.dtype == np.uint8 and out.shape == depth.shape + (() if grayscale else (3,))
    return out


def generate(ref):
    table = (np.array(ref.cm.get_cmap("inferno").colors) * 255).astype(np.uint8)      # dc_utils.py:75,80 on every row
    assert table.shape == (256, 3)
    out = {"table": table}
    for name in CASES:
        depth = np.array(case(name))
        assert depth.dtype == np.float32 and np.isfinite(depth).all()
        colour, gray = run_reference(ref, depth, False), run_reference(ref, depth, True)
        assert np.array_equal(colour, table[gray]), f"case {name}: the colour frames are not table[gray]"
        assert gray[depth == depth.min()].max() == 0 and (gray[depth == depth.max()] == 255).all()
        if name == "B":
            assert depth.min() == 0 and depth.max() == 255
            assert np.array_equal(np.unique(gray), np.arange(256)), "case B: not every table row is used"
            assert (depth[gray == 255] == 255).all(), "case B: row 255 away from the maximum"
        out[f"{name}_depth"], out[f"{name}_colour"], out[f"{name}_gray"] = depth, colour, gray
        print(f"case {name}: depth {depth.shape} in [{depth.min()!r}, {depth.max()!r}], {np.unique(gray).size} levels used")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference project (its utils/dc_utils.py is imported)")
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture bit for bit instead of writing it")
    args = ap.parse_args()
    new = generate(import_reference(args.reference))
    if args.check:
        old = np.load(GOLDEN)
        assert sorted(old.files) == sorted(new), f"keys differ: {sorted(set(old.files) ^ set(new))}"
        bad = [k for k in new if np.asarray(new[k]).dtype != old[k].dtype or np.asarray(new[k]).tobytes() != old[k].tobytes()]
        if bad:
            sys.exit(f"fixture differs in {bad}")
        print(f"{GOLDEN}: reproduced bit for bit")
    else:
        np.savez(GOLDEN, **new)
        print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
