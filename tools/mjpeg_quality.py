#!/usr/bin/env python
"""The quality table of DESIGN.md 6h: PSNR to the source of the integer encoder (mjpeg.encode_jpeg_numpy, whose bytes the device
reproduces) beside PIL's libjpeg encoder at the same tables and 4:4:4, both streams decoded by PIL, with the two stream sizes. A
diagonal depth ramp through the inferno table, uniform colour noise and the same ramp in gray, at the sizes of the tests (136 x 200)
and of a model-sized frame (518 x 518). No GPU. Output in profiles/mjpeg/quality.txt."""
import io
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from video_depth_anything_amd import mjpeg  # noqa: E402
from video_depth_anything_amd.visualize import colorize_numpy  # noqa: E402


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))


def main():
    print("image, size | quality | twin dB | PIL dB | twin - PIL | twin bytes | PIL bytes")
    for h, w in ((136, 200), (518, 518)):
        d = (np.add.outer(np.arange(h), np.arange(w)) / (h + w)).astype(np.float32)[None]
        images = {"ramp": colorize_numpy(d)[0], "noise": np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8),
                  "gray ramp": colorize_numpy(d, grayscale=True)[0]}
        for name, img in images.items():
            for q in (50, 75, 90, 95, 100):
                ours = mjpeg.encode_jpeg_numpy(img[None], q)[0]
                tabs = [t.tolist() for t in mjpeg.quant_tables(q)][:2 if img.ndim == 3 else 1]
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, "JPEG", qtables=tabs, subsampling=0)
                a, b = psnr(Image.open(io.BytesIO(ours)), img), psnr(Image.open(io.BytesIO(buf.getvalue())), img)
                print(f"{name}, {h} x {w} | {q} | {a:.3f} | {b:.3f} | {a - b:+.3f} | {len(ours)} | {len(buf.getvalue())}")


if __name__ == "__main__":
    main()
