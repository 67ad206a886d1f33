"""csrc/deflate_core.h - the code builder one lane of the deflate kernel runs per chunk - compiled for the host with the address and
undefined-behaviour sanitizers into a plain executable (tests/deflate_core_main.cpp, its own main) and run over the histograms of
the deflate inputs and over histograms no byte string gives: exit 0, no sanitizer report, lengths and codes equal to the Python
twin's. Nothing is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _deflate_inputs as dinp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "deflate_core_main.cpp")
INCLUDE = os.path.join(REPO, "video_depth_anything_amd", "csrc")
COMPILERS = ["g++", "/opt/rocm/llvm/bin/clang++", "clang++"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The sanitized executable, from the first compiler that builds one that runs."""
    out = str(tmp_path_factory.mktemp("dfl_core") / "deflate_core_main")
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


def run(program, *files):
    r = subprocess.run([program] + list(files), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r.stdout


def test_lengths_and_codes_equal_the_twins(program, tmp_path):
    from video_depth_anything_amd import deflate
    hists = dinp.histograms()
    assert {"single_symbol", "all_equal", "fibonacci", "fibonacci_40", "two_symbols", "flat_histogram"} <= {n for n, _ in hists}
    path = str(tmp_path / "hist.bin")
    np.stack([h for _, h in hists]).astype("<u4").tofile(path)
    run(program, path)
    raw = np.fromfile(path + ".out", np.uint8).reshape(len(hists), 286 * 3)
    limited = 0
    for (name, h), row in zip(hists, raw):
        lens = deflate.code_lengths(h)
        assert row[:286].tolist() == lens, name
        assert row[286:].copy().view("<u2").tolist() == deflate.canonical_codes(lens), name
        used = [b for b in lens if b]
        assert max(used, default=0) <= 15 and (len(used) < 2 or sum(2 ** (15 - b) for b in used) == 2 ** 15), name       # a complete code
        limited += max(deflate.code_lengths(h, max_bits=64)) > 15
    assert limited >= 2                    # the length limit was exercised (the Fibonacci counts)


def test_the_length_symbols_are_the_rfc_table(program):
    from video_depth_anything_amd import deflate
    lines = run(program).split("\n")
    for ln in range(3, 259):
        assert tuple(int(v) for v in lines[ln - 3].split()) == (ln,) + deflate.length_symbol(ln)
    for k in range(19):
        assert lines[256 + k] == f"cl {k} {deflate._CL_ORDER[k]}"


def test_the_code_length_code_equals_the_twins(program, tmp_path):
    """The 19-symbol code of at most 7 bits that the header's lengths are written in: the histograms of the lengths the cases' first
    chunks give, and histograms that need the limit."""
    from video_depth_anything_amd import deflate
    hists = []
    for name, h in dinp.histograms():
        lens = deflate.code_lengths(h)
        if sum(1 for b in lens if b) >= 2:
            hists.append((name, np.bincount(lens + [1], minlength=19)))
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 0, 0, 0]
    hists += [("fibonacci_16", np.array(fib)), ("all_19_equal", np.full(19, 3)), ("one", np.eye(19, dtype=np.int64)[5]), ("none", np.zeros(19, np.int64))]
    path = str(tmp_path / "hist.cl")
    np.stack([h for _, h in hists]).astype("<u4").tofile(path)
    run(program, path)
    raw = np.fromfile(path + ".out", np.uint8).reshape(len(hists), 19 * 3)
    for (name, h), row in zip(hists, raw):
        lens = deflate.code_lengths(h, deflate.CL_MAX_BITS)
        assert row[:19].tolist() == lens and max(lens) <= 7, name
        assert row[19:].copy().view("<u2").tolist() == deflate.canonical_codes(lens), name
    assert max(deflate.code_lengths(fib, 64)) == 15
