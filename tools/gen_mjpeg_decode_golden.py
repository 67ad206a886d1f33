#!/usr/bin/env python
"""Writes tests/golden/mjpeg_decode_streams.npz: baseline JPEG streams coded by PIL (libjpeg-turbo) and PIL's own decoded pixels
for them, so that the decoder's tests need no PIL (tests/_mjpeg_decode_inputs.py reads it).

Every shape (8x8, 9x5, 17x23, 33x50, 40x136 as H x W) meets every sampling (4:4:4, 4:2:2, 4:2:0, gray) twice; quality (50, 90,
100), restart interval (none, one MCU, one MCU row) and content (noise, ramp, checker) rotate over those 40 streams so that each
value meets each sampling and each shape. 40x136 is coded with one MCU per interval in 4:4:4 (85 intervals) and 4:2:0 (27): the
RSTm number wraps. No frame is narrower than 5 pixels: with subsampled chroma libjpeg-turbo's upsampler treats those otherwise.

The file holds `meta` (a JSON string: the PIL and libjpeg versions, and per stream h, w, sampling, quality, restart, content) and
per stream i `stream_i` (the JPEG's bytes) and `pixels_i` (uint8 [h,w,3] or [h,w])."""
import io
import json
import os

import numpy as np

SHAPES = [(8, 8), (9, 5), (17, 23), (33, 50), (40, 136)]
SAMPLINGS = ["444", "422", "420", "gray"]
QUALITIES = [50, 90, 100]
RESTARTS = ["none", "mcu", "row"]
CONTENTS = ["noise", "ramp", "checker"]
PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "mjpeg_decode_streams.npz")


def image(h, w, content, gray, seed):
    yy, xx = np.mgrid[:h, :w]
    if content == "noise":
        x = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif content == "ramp":
        x = np.stack([(yy * 5 + xx * 3) % 256, (xx * 7 + 40) % 256, (yy * 11 + xx) % 256], -1).astype(np.uint8)
    else:
        c = ((yy + xx) & 1) * 255
        x = np.stack([c, 255 - c, c], -1).astype(np.uint8)
    return np.ascontiguousarray(x[..., 0] if gray else x)


def cases():
    out = []
    for si, (h, w) in enumerate(SHAPES):
        for mi, samp in enumerate(SAMPLINGS):
            for rep in range(2):
                k = si + mi + rep
                restart = RESTARTS[(si + 2 * mi + 2 * rep) % 3]
                if (h, w) == (40, 136) and samp in ("444", "420") and rep == 0:
                    restart = "mcu"
                out.append(dict(h=h, w=w, sampling=samp, quality=QUALITIES[k % 3], restart=restart, content=CONTENTS[(2 * si + mi + 2 * rep) % 3]))
    return out


def build():
    """{name: array} of the fixture, made with the PIL that is importable."""
    import PIL
    from PIL import Image, features
    meta = dict(pil=PIL.__version__, jpg=features.version("jpg"), turbo=features.version("libjpeg_turbo") if features.check_feature("libjpeg_turbo") else None,
                streams=cases())
    out = {}
    for i, c in enumerate(meta["streams"]):
        gray = c["sampling"] == "gray"
        hs = 1 if c["sampling"] in ("444", "gray") else 2
        mcus_across = -(-c["w"] // (8 * hs))
        kw = dict(quality=c["quality"], restart_marker_blocks={"none": 0, "mcu": 1, "row": mcus_across}[c["restart"]])
        if not gray:
            kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[c["sampling"]]
        f = io.BytesIO()
        Image.fromarray(image(c["h"], c["w"], c["content"], gray, i)).save(f, "JPEG", **kw)
        out[f"stream_{i}"] = np.frombuffer(f.getvalue(), np.uint8)
        out[f"pixels_{i}"] = np.asarray(Image.open(io.BytesIO(f.getvalue())))
    out["meta"] = np.array(json.dumps(meta))
    return out


if __name__ == "__main__":
    arrays = build()
    np.savez_compressed(PATH, **arrays)
    print(f"{PATH}: {len(cases())} streams, {os.path.getsize(PATH)} bytes")
