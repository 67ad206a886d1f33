"""The inputs of the EXR tests (test_exr_numpy.py, test_exr_gpu.py): the smallest float32 [frames, h, w] arrays at which the writer of
csrc/exr.hip can still go wrong. A block is 16 scanlines, L = 4 w rows bytes, cut into ceil(L / 16384) balanced chunks. Every case
is built once, never changed, and marked with the number of its blocks that the twin writes RAW (its zlib stream is not strictly
shorter than the rows): test_exr_numpy.py holds the twin to these numbers on the CPU, so that the GPU tests are known to reach the
compressed path, the raw path, or both."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LINES = 16


def steps(shape, seed):
    """Smooth in the way an RLE matcher and a Huffman code can use: a ramp quantised to multiples of 1/4 (the low mantissa bytes are
    zero, neighbouring pixels are often equal), different in every frame."""
    n, h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(np.floor((x + 2 * y + 5 * f + seed) / 8.0) / 4.0 + 1.0).astype(np.float32) for f in range(n)])


def noise(shape, seed):
    """Random bits: nothing to code, every chunk stored, every block raw. (NaNs of every payload among them.)"""
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint32).view(np.float32)


def special_bits():
    """NaNs with payloads (quiet and signalling), +-inf, -0.0, denormals, the largest and smallest normals: bits, not numbers."""
    bits = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000,
                     0x00000001, 0x807FFFFF, 0x00400000, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000], np.uint32)
    return np.tile(np.repeat(bits, 4), 16).reshape(1, 16, 64).view(np.float32)


def mixed():
    """Upper half noise, lower half smooth: 40 rows are a block of noise, one of 4 noise rows above 12 of steps, and 8 rows of steps."""
    x = steps((1, 40, 130), 3)
    x[0, :20] = noise((20, 130), 7)
    return x


# name: (array, blocks the twin writes raw)
@functools.lru_cache(maxsize=None)
def cases():
    out = {
        "one_pixel": (np.full((1, 1, 1), 1.5, np.float32), 1),                    # L = 4: no zlib stream is shorter
        "one_chunk": (steps((1, 16, 64), 0), 0),                                  # L = 4096
        "exactly_16384": (steps((1, 16, 256), 1), 0),                             # L = 16384: one full chunk
        "two_chunks_one_row_tail": (steps((2, 17, 257), 2), 0),                   # L = 16448 = 2 x 8256 (8192 used of the second), then L = 1028
        "three_chunks_five_row_tail": (steps((3, 37, 518), 4), 0),                # L = 33152 = 3 x 11072 (less 64), last block 5 rows
        # constant frames, 2 x 9600 bytes a block: of 0.0 f is one run of zeros through both chunks (matches of 258 cut by the chunk's
        # end); of 1.0 its first half is that run and its second half alternates between two bytes (a code of two one-bit symbols)
        "constant": (np.stack([np.zeros((33, 300), np.float32), np.ones((33, 300), np.float32)]), 0),
        "noise": (noise((1, 20, 100), 5), 2),
        "mixed": (mixed(), 1),                                                    # the block of 4 noise rows and 12 of steps still gains
        "special_bits": (special_bits(), 0),
    }
    for x, _ in out.values():
        assert x.dtype == np.float32 and x.ndim == 3
        x.setflags(write=False)
    return out


def names():
    return list(cases())


def case(name):
    return cases()[name][0]


def raw_blocks(name):
    return cases()[name][1]


def n_blocks(name):
    n, h, _ = case(name).shape
    return n * -(-h // LINES)


@functools.lru_cache(maxsize=None)
def twin(name):
    """(files, compressed flags per block over all frames) of a case by encode_exr_numpy, computed once for all tests."""
    from video_depth_anything_amd import exr
    files, flags = [], []
    for frame in case(name):
        files.append(exr.encode_exr_numpy(frame, info=flags))
    return tuple(files), tuple(flags)


def fixture_depths(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))["depths"]
