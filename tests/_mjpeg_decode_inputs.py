"""Streams shared by the CPU and GPU tests of the Motion-JPEG decoder, and the host twin's results for them (computed once per
process, never changed):

  golden   tests/golden/mjpeg_decode_streams.npz (tools/gen_mjpeg_decode_golden.py): PIL-coded streams of 8x8 to 40x136 in 4:4:4,
           4:2:2, 4:2:0 and gray, qualities 50 / 90 / 100, no restart markers / one MCU / one MCU row per interval, with PIL's pixels;
  own      the project's encoder's streams (encode_jpeg_numpy) of _mjpeg_inputs.SHAPES: 4:4:4 and gray, an interval per MCU row;
  no DHT   the same streams with every DHT segment cut out (the AVI MJPG convention: the Annex K tables are implied);
  corrupt  one good 17x23 stream (3 x 3 MCUs, DRI = 3) broken in the ways a file breaks, each with the status it must end in.
"""
import functools
import json
import os
import struct

import numpy as np

import _mjpeg_inputs as enc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mjpeg_decode_streams.npz")
OWN = [(shape, content, q) for shape in enc.SHAPES for content, q in (("noise", 100), ("ramp", 90), ("checker", 50))]


@functools.lru_cache(maxsize=None)
def golden():
    """[(meta dict, JPEG bytes, PIL's pixels)], and the fixture's record of the PIL that made it."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z["meta"]))
    out = []
    for i, c in enumerate(meta["streams"]):
        px = z[f"pixels_{i}"]
        px.setflags(write=False)
        out.append((c, z[f"stream_{i}"].tobytes(), px))
    return out, {k: meta[k] for k in ("pil", "jpg", "turbo")}


def golden_id(item):
    c = item[0]
    return f"{c['h']}x{c['w']}-{c['sampling']}-q{c['quality']}-{c['restart']}-{c['content']}"


def own_id(case):
    return enc.case_id(case)


def own(case):
    """The encoder twin's JPEGs of one case of OWN (a list, one per frame)."""
    return enc.reference(*case)[0]


def strip_dht(jpeg):
    """The stream without its DHT segments."""
    out, p = bytearray(jpeg[:2]), 2
    while True:
        m, ln = jpeg[p + 1], struct.unpack_from(">H", jpeg, p + 2)[0]
        if m != 0xC4:
            out += jpeg[p:p + 2 + ln]
        p += 2 + ln
        if m == 0xDA:
            return bytes(out) + jpeg[p:]


@functools.lru_cache(maxsize=None)
def twin_pixels(jpegs):
    """decode_jpeg_numpy of a tuple of JPEGs; read-only."""
    from video_depth_anything_amd import mjpeg
    px = mjpeg.decode_jpeg_numpy(list(jpegs))
    px.setflags(write=False)
    return px


# ----------------------------------------------------------------------------------------------------------------------- corrupt
def good_17x23():
    return own(((2, 17, 23, 3), "noise", 90))[0]


def _scan_parts(jpeg):
    """(header, the three intervals' bytes without their markers) of the good stream."""
    from video_depth_anything_amd import mjpeg
    info = mjpeg.parse_jpeg(jpeg)
    iv, status = mjpeg.scan_intervals(jpeg, info)
    assert status == 0 and iv.shape[0] == 3 and info.dri == 3
    return jpeg[:info.scan_offset], [jpeg[lo:lo + ln] for lo, ln, _, _ in iv.tolist()]


def _join(head, parts):
    out = head + parts[0]
    for i, p in enumerate(parts[1:]):
        out += bytes([0xFF, 0xD0 + (i & 7)]) + p
    return out + b"\xff\xd9"


# (byte of the scan, bits flipped in it): one flip that turns a code into a run that passes coefficient 63, one that leaves 16 bits
# that are no code (found by trying every bit of this stream once; the tests assert the statuses they end in)
RUN_FLIP, CODE_FLIP = (1, 0x40), (730, 0x10)


@functools.lru_cache(maxsize=None)
def corrupt():
    """[(name, JPEG bytes, the name of the status it must end in)]."""
    from video_depth_anything_amd import mjpeg
    S = mjpeg.DECODE_STATUS
    good = good_17x23()
    head, parts = _scan_parts(good)
    dri_at = head.index(b"\xff\xdd") + 4
    assert head[dri_at:dri_at + 2] == b"\x00\x03"

    def halves(p):                                                 # cut in the middle, but not between an FF and its stuffed 00
        at = len(p) // 2
        while p[at - 1] == 0xFF:
            at -= 1
        return p[:at], p[at:]
    out = [
        # cut in the middle of an interval, EOI kept so that the cut itself is what is found: in the second interval the third is
        # missing as well, in the last one only its own MCUs are
        ("truncated_in_second_interval", _join(head, [parts[0], halves(parts[1])[0]]), S[5]),
        ("truncated_in_last_interval", _join(head, parts[:2] + [halves(parts[2])[0]]), S[4]),
        ("rst_deleted", head + parts[0] + parts[1] + b"\xff\xd1" + parts[2] + b"\xff\xd9", S[5]),
        ("rst_inserted", _join(head, [parts[0], *halves(parts[1]), parts[2]]), S[5]),
        ("all_ff", head + b"\xff" * (len(good) - len(head) - 2) + b"\xff\xd9", S[7]),
        ("eoi_removed", good[:-2], S[7]),
        ("dri_raised", head[:dri_at] + b"\x00\x04" + head[dri_at + 2:] + good[len(head):], S[4]),
    ]
    for name, (at, mask), status in (("run_past_63", RUN_FLIP, 3), ("code_not_in_table", CODE_FLIP, 1)):
        flipped = bytearray(good)
        flipped[len(head) + at] ^= mask
        out.append((name, bytes(flipped), S[status]))
    # the two statuses no flip of that stream reaches, written by hand as gray frames with divisors of 1:
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    gray = lambda h, w: b"\xff\xd8" + seg(0xDB, b"\x00" + b"\x01" * 64) + seg(0xC0, struct.pack(">BHHB", 8, h, w, 1) + b"\x01\x11\x00")
    sos = seg(0xDA, b"\x01\x01\x00\x00\x3f\x00")
    # 20 blocks in one interval, each a DC difference of +2047 (Annex K: category 11 is 111111110, then 11 one-bits) and EOB
    # (1010): FF 7F FA, the FF stuffed. The predictor passes 32767 at the 17th block.
    out.append(("dc_predictor_overflow", gray(8, 160) + sos + b"\xff\x00\x7f\xfa" * 20 + b"\xff\xd9", S[6]))
    # tables of one 1-bit code each: DC category 0, AC symbol 0x0B = run 0, size 11, which baseline does not have
    one = lambda tc, sym: seg(0xC4, bytes([tc, 1] + [0] * 15 + [sym]))
    out.append(("ac_size_11", gray(8, 8) + one(0x00, 0) + one(0x10, 0x0B) + sos + b"\x3f\xff\xd9", S[2]))
    return out


def unsupported():
    """[(name, JPEG bytes, a word of the message)]: a good stream with header bytes patched into what the decoder does not read."""
    good = bytearray(good_17x23())
    sof = bytes(good).index(b"\xff\xc0")
    sos = bytes(good).index(b"\xff\xda")

    def patched(at, value):
        b = bytearray(good)
        b[at] = value
        return bytes(b)
    return [("sof2", patched(sof + 1, 0xC2), "SOF2"), ("12bit", patched(sof + 4, 12), "12-bit"), ("4_components", patched(sof + 9, 4), "4 components"),
            ("1x2_sampling", patched(sof + 11, 0x12), "sampling"), ("two_scans", patched(sos + 4, 1), "scans")]
