"""The inputs of the deflate tests (test_deflate_numpy.py, test_deflate_core_host.py, test_deflate_gpu.py): the smallest byte strings
at which the encoder of csrc/deflate.hip can still go wrong. Every input is a (name, uint8 array) pair, built once and never changed."""
import functools
import os

import numpy as np

CHUNK = 16384
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUN_TOTALS = (1, 2, 3, 4, 5, 258, 259, 260, 261, 262, 517, 518)      # run lengths: tails of 0, 1 and 2 behind none, one and two full matches


def no_equal_neighbours(counts):
    """Byte values with the given {value: count}, arranged so that no two neighbours are equal: the most frequent value is spread
    over the even positions first, the rest fill what is left in order (works while no count exceeds half the total, rounded up)."""
    vals = sorted(counts, key=lambda v: (-counts[v], v))
    seq = np.concatenate([np.full(counts[v], v, np.uint8) for v in vals])
    n = seq.size
    out = np.zeros(n, np.uint8)
    slots = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    out[slots] = seq
    assert not (out[1:] == out[:-1]).any()
    return out


def fibonacci():
    """Value k occurs F(k) times, k = 1..20 (F(1) = F(2) = 1): 17 710 bytes, no equal neighbours. An unlimited Huffman code for the
    first chunk's counts is deeper than 15 bits."""
    f = [1, 1]
    while len(f) < 20:
        f.append(f[-1] + f[-2])
    x = no_equal_neighbours({k + 1: f[k] for k in range(20)})[::-1].copy()       # reversed: the rare values lie in the first chunk
    assert x.size == 17710 and np.unique(x[:CHUNK]).size == 20
    return x


def fibonacci_with_eob():
    """Value k occurs F(k + 1) times, k = 1..18: 10 944 bytes in one chunk, no equal neighbours. The end-of-block symbol's count of 1
    takes the place of F(1), so the 19 counts are the Fibonacci numbers exactly and the unlimited Huffman code is a chain 18 bits
    deep: the length limit works on a real chunk. (In `fibonacci` the extra 1 of end-of-block lets two chains grow side by side
    and the code stays 11 bits deep.)"""
    f = [1, 1]
    while len(f) < 19:
        f.append(f[-1] + f[-2])
    x = no_equal_neighbours({k: f[k] for k in range(1, 19)})
    assert x.size == 10944
    return x


def run_sweep():
    """Runs of every length 1..262 (every length code's first and last length and all its extra bits), a changing separator byte
    between them: 34 715 bytes, so some runs meet a chunk boundary too."""
    parts = []
    for n in range(1, 263):
        parts += [np.full(n, 10 + n % 3, np.uint8), np.array([200 + n % 50], np.uint8)]
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(1951)
    noise = rng.integers(0, 256, 3 * CHUNK, dtype=np.uint8)
    out = []
    # lengths: a smooth-ish signal, so both the coded and the stored path appear
    base = (np.cumsum(rng.integers(-1, 2, 2 * CHUNK + 3)) & 255).astype(np.uint8)
    for n in (0, 1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3):
        out.append((f"len_{n}", base[:n].copy()))
    # runs
    for n in RUN_TOTALS:
        out.append((f"run_{n}", np.concatenate([[9], np.full(n, 200, np.uint8), [9, 8]]).astype(np.uint8)))
    out.append(("run_sweep", run_sweep()))
    straddle = (np.arange(2 * CHUNK) % 251).astype(np.uint8)
    straddle[CHUNK - 300:CHUNK + 300] = 77
    out.append(("run_straddles_chunks", straddle))
    out.append(("one_byte_chunk", np.full(CHUNK, 42, np.uint8)))
    out.append(("zeros_two_chunks_and_a_bit", np.zeros(2 * CHUNK + 700, np.uint8)))
    # alphabet
    out.append(("two_symbols", rng.integers(0, 2, CHUNK, dtype=np.uint8) * 131 + 3))
    out.append(("all_256_no_neighbours", ((np.arange(CHUNK) * 37) & 255).astype(np.uint8)))
    out.append(("fibonacci", fibonacci()))
    out.append(("fibonacci_with_eob", fibonacci_with_eob()))
    out.append(("flat_histogram", np.tile(np.arange(256, dtype=np.uint8), CHUNK // 256)))
    skew = rng.choice(256, 2 * CHUNK, p=np.r_[0.5, np.full(255, 0.5 / 255)]).astype(np.uint8)
    out.append(("skewed_with_runs", skew))
    # incompressible: three chunks that take the stored fallback
    out.append(("noise_3_chunks", noise))
    # real data
    for name in ("tiny_video", "tiny_metric_video"):
        d = np.load(os.path.join(GOLDEN, name + ".npz"))["depths"]
        assert d.dtype == np.float32 and d.nbytes == 470400
        out.append((name, np.ascontiguousarray(d).reshape(-1).view(np.uint8).copy()))
    for _, x in out:
        x.setflags(write=False)
    return tuple(out)


def names():
    return [n for n, _ in cases()]


def case(name):
    return dict(cases())[name]


@functools.lru_cache(maxsize=None)
def twin_stream(name, final=True):
    """deflate_numpy of a case, computed once for all tests that compare against it."""
    from video_depth_anything_amd import deflate
    return deflate.deflate_numpy(case(name), final=final)


def histograms():
    """(name, counts [286]) for the code-length builder: the cases' first chunks plus what no byte string gives."""
    from video_depth_anything_amd import deflate
    out = []
    for name, x in cases():
        if x.size == 0:
            continue
        sym = deflate.chunk_tokens(np.asarray(x[:CHUNK]))[1]
        c = np.bincount(sym, minlength=286)
        c[256] = 1
        out.append((name, c.astype(np.int64)))
    one = np.zeros(286, np.int64)
    one[256] = 1
    out.append(("single_symbol", one))
    out.append(("nothing", np.zeros(286, np.int64)))
    out.append(("all_equal", np.full(286, 57, np.int64)))
    out.append(("all_ones", np.ones(286, np.int64)))
    fib = np.zeros(286, np.int64)
    a, b = 1, 1
    for k in range(40):                                               # 40 Fibonacci weights: an unlimited code would be 39 bits deep
        fib[7 * k] = a
        a, b = b, a + b
    out.append(("fibonacci_40", fib))
    two = np.zeros(286, np.int64)
    two[0], two[285] = 5, 5
    out.append(("two_symbols_equal", two))
    return out
