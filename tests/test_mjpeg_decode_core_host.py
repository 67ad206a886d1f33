"""csrc/mjpeg_decode_core.h - the entropy decoder's per-interval loop, the text the device kernel runs - compiled for the host with
the address and undefined-behaviour sanitizers into a plain executable (tests/mjpeg_decode_core_main.cpp, its own main) and run
over good streams and the whole corrupt corpus: exit 0, no sanitizer report, coefficients and statuses equal to the Python twin's.
The evidence that the bounds logic holds before a corrupt stream is ever given to a GPU. Nothing is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import _mjpeg_decode_inputs as dinp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "mjpeg_decode_core_main.cpp")
INCLUDE = os.path.join(REPO, "video_depth_anything_amd", "csrc")
COMPILERS = ["g++", "/opt/rocm/llvm/bin/clang++", "clang++"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The sanitized executable, from the first compiler that builds one that runs."""
    out = str(tmp_path_factory.mktemp("mjd_core") / "mjpeg_decode_core_main")
    tried = []
    for cxx in COMPILERS:
        if shutil.which(cxx) is None:
            tried.append(f"{cxx}: not found")
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INCLUDE, SRC,
                            "-o", out], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([out], capture_output=True).returncode == 0:
            return out
        tried.append(f"{cxx}: {r.stderr[-300:]}")
    pytest.skip("no host compiler links and runs a program with -fsanitize=address,undefined: " + "; ".join(tried))


def case_file(path, jpeg):
    """One frame as the program reads it; returns the twin's (coefficients, status) for it."""
    from video_depth_anything_amd import mjpeg
    info = mjpeg.parse_jpeg(jpeg)
    iv, host_status = mjpeg.scan_intervals(jpeg, info)
    off, bw, blocks = info.geometry
    mw, mh = info.mcus
    so = info.scan_offset
    iv = iv.copy()
    iv[:, 0] -= so
    scan = jpeg[so:]
    head = struct.pack("<16i", 0x43444a4d, info.components, info.hs, info.vs, mw, mh, *off, *bw, blocks, iv.shape[0], len(scan), 0)
    with open(path, "wb") as f:
        f.write(head + mjpeg.decode_tables(info).tobytes() + iv.astype("<i4").tobytes() + scan)
    coef, status = mjpeg.decode_coefficients(jpeg, info)
    # the program sees what a lane sees: the statuses the host side finds (interval count, EOI) are not its business
    lane_status = 0
    tabs = mjpeg._python_tables(mjpeg.decode_tables(info))
    again = np.zeros_like(coef)
    for lo, ln, first, count in (iv + [so, 0, 0, 0]).tolist():
        lane_status = max(lane_status, mjpeg._decode_interval(jpeg, lo, ln, first, count, info, tabs, again))
    assert np.array_equal(again, coef) and max(lane_status, host_status) == status
    return coef, lane_status


def run(program, tmp_path, jpegs):
    want = [case_file(str(tmp_path / f"case{i}.bin"), j) for i, j in enumerate(jpegs)]
    files = [str(tmp_path / f"case{i}.bin") for i in range(len(jpegs))]
    r = subprocess.run([program] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(jpegs)
    for line, path, (coef, status) in zip(lines, files, want):
        assert line == f"{path} {status}"
        assert np.array_equal(np.fromfile(path + ".coef", "<i2").reshape(coef.shape), coef), path


def test_good_streams(program, tmp_path):
    jpegs = [j for _, j, _ in dinp.golden()[0]] + [j for case in dinp.OWN for j in dinp.own(case)]
    jpegs += [dinp.strip_dht(j) for j in dinp.own(dinp.OWN[3])]
    run(program, tmp_path, jpegs)


def test_the_corrupt_corpus(program, tmp_path):
    corpus = dinp.corrupt()
    assert len(corpus) >= 7
    run(program, tmp_path, [j for _, j, _ in corpus])


def test_a_sweep_of_truncations_and_flips(program, tmp_path):
    """The good 17x23 stream cut after every seventh byte of its scan (EOI kept), and with every fifth byte of the scan inverted in
    turn: whatever the decoder makes of them, it reads and writes inside its buffers and agrees with the twin."""
    from video_depth_anything_amd import mjpeg
    good = dinp.good_17x23()
    so = mjpeg.parse_jpeg(good).scan_offset
    cuts = [good[:at] + b"\xff\xd9" for at in range(so, len(good) - 2, 7)]
    flips = [good[:at] + bytes([good[at] ^ 0xFF]) + good[at + 1:] for at in range(so, len(good) - 2, 5)]
    run(program, tmp_path, cuts + flips)
