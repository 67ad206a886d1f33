"""Frames as baseline JPEG, and JPEG frames as a Motion-JPEG AVI: the video file of run.py without imageio, ffmpeg or any codec
library, with the bytes made on the device (csrc/mjpeg.hip).

The contract is `encode_jpeg_numpy`: every step is integer arithmetic, so the device reproduces the stream byte for byte.

  input     uint8 [N,H,W,3] RGB or [N,H,W] gray (a 1-component JPEG); the right and bottom edges are padded to a multiple of 8 by
            replicating the last column / row.
  colour    JFIF BT.601 full range in 16-bit fixed point, 4:4:4 (false-colour depth carries its signal in chroma):
              Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
              Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
              Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
            (32767, not 32768, in the chroma rounding: with 32768 a pure blue or red pixel gives 256. libjpeg does the same.)
  DCT       s = sample - 128;  Ci[k][n] = rint(8192 c_k cos((2n+1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2:
              t[k][x] = (sum_n Ci[k][n] s[n][x] + 128) >> 8           columns (|sum| < 2^22; t keeps 5 fractional bits)
              F[k][l] = (sum_m Ci[l][m] t[k][m] + 16384) >> 15        rows    (|sum| < 2^28); >> is the arithmetic shift
            F is EIGHT TIMES the coefficient: its 3 fractional bits go into the quantiser's rounding, as libjpeg's do. Rounding
            to an integer first costs up to 0.7 dB at quality 95 and 2.5 dB at 100 (DESIGN.md 6h has the measurements).
  quantise  Annex K tables scaled by libjpeg's rule (`quant_tables`); q = sign(F) ((2 |F| + 8 Q) // (16 Q)); AC clamped to +-1023.
  entropy   baseline sequential, the four Annex K Huffman tables, zig-zag order, one MCU = the Y, Cb, Cr blocks of one 8x8 tile;
            ONE RESTART INTERVAL PER MCU ROW (DRI = ceil(W / 8), RSTm cycling 0..7 between intervals, DC predictors reset, the
            last byte of an interval padded with 1-bits, FF -> FF 00) - the rows of a frame are coded independently.
  header    SOI, JFIF APP0, two DQT (one for gray), SOF0, four DHT (two for gray), DRI, SOS: `jpeg_header`, the same for every
            frame of a video. A frame is header + scan + EOI.

`write_avi` / `read_avi` are the container: RIFF AVI 1.0 with one MJPG video stream and an idx1 index, written in one pass.
"""
import struct

import numpy as np

from . import staging

# ------------------------------------------------------------------------------------------------------------ ITU T.81 Annex K
_QL = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_QC = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_DC_L_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
_DC_C_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
_DC_VALS = bytes(range(12))
_AC_L_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)
_AC_L_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_C_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)
_AC_C_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9ba"
    "c2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")

# ZIGZAG[i] = the natural (row * 8 + column) position of the i-th coefficient of the scan
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

_k, _n = np.arange(8)[:, None], np.arange(8)[None, :]
DCT_MATRIX = np.rint(8192 * np.where(_k == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * _n + 1) * _k * np.pi / 16)).astype(np.int64)

MAX_BLOCK_BITS = 64 * 26          # a block's bits before stuffing: DC at most 9 + 11, each of 63 AC at most 16 + 10


def _huffman(bits, vals):
    """(code, length) per symbol value 0..255 (length 0 = not in the table), built as T.81 Annex C builds them."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    c, i = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[i]], length[vals[i]] = c, ln
            c, i = c + 1, i + 1
        c <<= 1
    return code, length


_DC = (_huffman(_DC_L_BITS, _DC_VALS), _huffman(_DC_C_BITS, _DC_VALS))
_AC = (_huffman(_AC_L_BITS, _AC_L_VALS), _huffman(_AC_C_BITS, _AC_C_VALS))


def huffman_words():
    """uint32 [2, 256 + 16]: per table class (0 luminance, 1 chrominance) the AC table then the DC table, each entry
    code | length << 16 - what csrc/mjpeg.hip holds as constants (tests compare the two through the bytes they produce)."""
    out = np.zeros((2, 272), np.uint32)
    for t in range(2):
        out[t, :256] = _AC[t][0] | (_AC[t][1] << 16)
        out[t, 256:268] = (_DC[t][0] | (_DC[t][1] << 16))[:12]
    return out


def _check_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= quality <= 100:
        raise ValueError(f"mjpeg: quality must be an integer in 1..100, got {quality!r}")
    return int(quality)


def quant_tables(quality=90):
    """int [2, 64] in natural order: the Annex K luminance and chrominance tables scaled by libjpeg's quality rule."""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    t = np.array([_QL, _QC], dtype=np.int64)
    return np.clip((t * s + 50) // 100, 1, 255)


def _check_frames(frames):
    if str(frames.dtype).replace("torch.", "") != "uint8":
        raise TypeError(f"mjpeg: frames must be uint8, got {frames.dtype}")
    shape = tuple(frames.shape)
    if len(shape) not in (3, 4) or (len(shape) == 4 and shape[3] != 3) or 0 in shape:
        raise ValueError(f"mjpeg: frames must be [N,H,W,3] (RGB) or [N,H,W] (gray) and not empty, got {shape}")
    if shape[1] > 65535 or shape[2] > 65535:
        raise ValueError(f"mjpeg: a JPEG frame is at most 65535 x 65535, got {shape[1]} x {shape[2]}")
    return shape[0], shape[1], shape[2], (3 if len(shape) == 4 else 1)


def jpeg_header(h, w, channels=3, quality=90):
    """The bytes in front of every frame's scan: SOI, APP0, DQT, SOF0, DHT, DRI, SOS."""
    if channels not in (1, 3) or not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"mjpeg: bad frame {h} x {w} x {channels}")
    qt = quant_tables(quality)
    seg = lambda marker, body: bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if channels == 3 else 1):
        out += seg(0xDB, bytes([t]) + bytes(qt[t][ZIGZAG].tolist()))
    out += seg(0xC0, struct.pack(">BHHB", 8, h, w, channels) + b"".join(bytes([c + 1, 0x11, min(c, 1)]) for c in range(channels)))
    tables = [(0x00, _DC_L_BITS, _DC_VALS), (0x10, _AC_L_BITS, _AC_L_VALS)]
    if channels == 3:
        tables += [(0x01, _DC_C_BITS, _DC_VALS), (0x11, _AC_C_BITS, _AC_C_VALS)]
    for tc, bits, vals in tables:
        out += seg(0xC4, bytes([tc]) + bytes(bits) + vals)
    out += seg(0xDD, struct.pack(">H", (w + 7) // 8))
    out += seg(0xDA, bytes([channels]) + b"".join(bytes([c + 1, 0x11 * min(c, 1)]) for c in range(channels)) + b"\x00\x3f\x00")
    return out


# ---------------------------------------------------------------------------------------------------------------- the host twin
def quantized_blocks(frames, quality=90):
    """int64 [N, ceil(H/8), ceil(W/8), C, 64]: every block's quantised coefficients in zig-zag order (the transform kernel's output)."""
    frames = frames if isinstance(frames, np.ndarray) else np.asarray(frames)
    n, h, w, ch = _check_frames(frames)
    qt = quant_tables(quality)
    bh, bw = (h + 7) // 8, (w + 7) // 8
    x = frames.reshape(n, h, w, ch)
    x = np.pad(x, ((0, 0), (0, bh * 8 - h), (0, bw * 8 - w), (0, 0)), mode="edge").astype(np.int64)
    if ch == 3:
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        x = np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
                      (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
                      (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16], axis=-1)
    s = (x - 128).reshape(n, bh, 8, bw, 8, ch).transpose(0, 1, 3, 5, 2, 4)           # [n, bh, bw, c, row, column]
    t = (np.einsum("kn,...nx->...kx", DCT_MATRIX, s) + 128) >> 8
    f = (np.einsum("lm,...km->...kl", DCT_MATRIX, t) + 16384) >> 15                      # 8 x the coefficient
    q = 8 * qt[[0, 1, 1][:ch]].reshape(ch, 8, 8)
    v = np.sign(f) * ((2 * np.abs(f) + q) // (2 * q))
    v = v.reshape(n, bh, bw, ch, 64)[..., ZIGZAG]
    v[..., 1:] = np.clip(v[..., 1:], -1023, 1023)
    return v


def _category(v):
    """Number of bits of |v| (0 for 0), elementwise."""
    a = np.abs(v)
    c = np.zeros(a.shape, np.int64)
    for k in range(12):
        c += a >= (1 << k)
    return c


def _encode_frame(zz, ch, cover):
    """zz int64 [bh, bw, ch, 64] -> the frame's scan bytes (every interval stuffed, RSTm between them) + EOI."""
    bh, bw = zz.shape[:2]
    nb = bw * ch
    zz = zz.reshape(bh, nb, 64)
    tab = np.tile(np.array([0, 1, 1][:ch]), bw)                                        # table class of each block of an interval
    # one token per slot: DC, the 63 AC positions (ZRLs folded into the coefficient that ends the run), EOB
    val, nbits = np.zeros((bh, nb, 65), np.uint64), np.zeros((bh, nb, 65), np.int64)
    dc = zz[..., 0]
    diff = dc.copy()
    diff[:, ch:] -= dc[:, :-ch]                                                        # the left neighbour of the same component
    cat = _category(diff)
    amp = np.where(diff >= 0, diff, diff - 1) & ((1 << cat) - 1)
    code, ln = np.stack([_DC[t][0] for t in tab])[np.arange(nb), cat], np.stack([_DC[t][1] for t in tab])[np.arange(nb), cat]
    val[..., 0], nbits[..., 0] = ((code << cat) | amp).astype(np.uint64), ln + cat
    ac = zz[..., 1:]
    nz = ac != 0
    pos = np.arange(1, 64)
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=-1)                        # position of the latest non-zero up to here
    prev = np.concatenate([np.zeros(last.shape[:-1] + (1,), np.int64), last[..., :-1]], axis=-1)
    run = np.where(nz, pos - prev - 1, 0)
    zrl, run = run >> 4, run & 15
    cat = _category(ac)
    sym = (run << 4) | cat
    tb = np.broadcast_to(tab[None, :, None], sym.shape)
    accode, aclen = np.stack([_AC[0][0], _AC[1][0]]), np.stack([_AC[0][1], _AC[1][1]])
    amp = np.where(ac >= 0, ac, ac - 1) & ((1 << cat) - 1)
    v = np.zeros(sym.shape, np.uint64)
    b = np.zeros(sym.shape, np.int64)
    zcode, zlen = accode[tb, 0xF0], aclen[tb, 0xF0]
    for _ in range(3):                                                                 # a run of up to 62 zeros: at most three ZRL
        take = nz & (zrl > 0)
        v = np.where(take, (v << zlen.astype(np.uint64)) | zcode.astype(np.uint64), v)
        b = np.where(take, b + zlen, b)
        zrl = zrl - take
    sl = aclen[tb, sym]
    v = (((v << sl.astype(np.uint64)) | accode[tb, sym].astype(np.uint64)) << cat.astype(np.uint64)) | amp.astype(np.uint64)
    val[..., 1:64], nbits[..., 1:64] = np.where(nz, v, 0), np.where(nz, b + sl + cat, 0)
    eob = ~nz[..., -1]
    val[..., 64], nbits[..., 64] = np.where(eob, accode[tab, 0][None], 0), np.where(eob, aclen[tab, 0][None], 0)
    assert nbits.reshape(bh, nb, 65).sum(-1).max() <= MAX_BLOCK_BITS
    if cover is not None:
        cover["zrl"] += int(((np.where(nz, pos - prev - 1, 0)) >> 4).sum())
        cover["no_eob_blocks"] += int(nz[..., -1].sum())
        cover["max_dc_category"] = max(cover["max_dc_category"], int(_category(diff).max()))
        cover["max_ac_category"] = max(cover["max_ac_category"], int(cat.max()))
        cover["intervals"] += bh
    # bits: every interval starts on a byte, its last byte padded with ones
    ibits = nbits.reshape(bh, -1).sum(-1)
    ibytes = (ibits + 7) // 8
    start = np.concatenate([[0], np.cumsum(ibytes)])
    flat_n, flat_v = nbits.reshape(bh, -1), val.reshape(bh, -1)
    off = np.cumsum(flat_n, axis=-1) - flat_n + (start[:-1] * 8)[:, None]              # bit offset of every token in the frame
    keep = flat_n > 0
    tn, tv, to = flat_n[keep], flat_v[keep], off[keep]
    bits = np.ones(int(start[-1]) * 8, np.uint8)
    idx = np.repeat(np.arange(tn.size), tn)
    within = np.arange(idx.size) - np.repeat(np.cumsum(tn) - tn, tn)
    bits[to[idx] + within] = ((tv[idx] >> (tn[idx] - 1 - within).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    raw = np.packbits(bits)
    ff = np.flatnonzero(raw == 0xFF)
    if cover is not None:
        cover["stuffed_ff"] += int(ff.size)
    # insert: 00 behind every FF, FF Dm in front of every interval but the first
    at = np.concatenate([ff + 1, np.repeat(start[1:-1], 2)])
    what = np.concatenate([np.zeros(ff.size, np.uint8), np.stack([np.full(bh - 1, 0xFF), 0xD0 + (np.arange(bh - 1) & 7)], -1).reshape(-1).astype(np.uint8)])
    order = np.argsort(at, kind="stable")                                              # a stuffed 00 at an interval's end sorts before the marker
    return np.insert(raw, at[order], what[order]).tobytes() + b"\xff\xd9"


def new_coverage():
    return dict(zrl=0, stuffed_ff=0, no_eob_blocks=0, max_dc_category=0, max_ac_category=0, intervals=0)


def encode_jpeg_numpy(frames, quality=90, device=None, coverage=None):
    """list of N `bytes`, each a complete baseline JPEG of one frame: the contract. `device` is ignored. coverage: a dict from
    `new_coverage()` that this call adds to - ZRL symbols, stuffed FF bytes, blocks with a non-zero coefficient 63 (no EOB),
    the largest DC and AC category and the number of restart intervals coded."""
    frames = frames if isinstance(frames, np.ndarray) else np.asarray(frames)
    n, h, w, ch = _check_frames(frames)
    head = jpeg_header(h, w, ch, quality)
    out = []
    for i in range(n):                                                                 # a frame at a time: the bit array is 8 x the stream
        zz = quantized_blocks(frames[i:i + 1], quality)[0]
        out.append(head + _encode_frame(zz, ch, coverage))
    return out


# ------------------------------------------------------------------------------------------------------------------ the device
_BLOCK_BYTES = 1 << 25                        # frame bytes staged at a time by encode_jpeg's numpy path


def _device_tables(quality, ch):
    qt = quant_tables(quality)[:2 if ch == 3 else 1]
    return np.ascontiguousarray(qt, dtype=np.uint16)


def encode_jpeg(frames, quality=90, device=None):
    """The same bytes as encode_jpeg_numpy, made by vda_mjpeg_encode_u8. A CUDA uint8 tensor ([N,H,W,3] or [N,H,W]) gives
    (payload, lengths) on its device and stream: payload uint8 holds the frames' scans (entropy-coded data + EOI) back to back,
    lengths int64 [N] their sizes; frame i is jpeg_header(h, w, channels, quality) + payload[sum(lengths[:i]) :][: lengths[i]].
    A numpy array or memory map gives the list of complete JPEGs, the frames staged a block at a time (`device`, default "cuda")."""
    import torch
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = np.asarray(frames)
    n, h, w, ch = _check_frames(frames)
    _check_quality(quality)
    is_tensor, dev = staging.placement(frames, device, "mjpeg", "encode_jpeg_numpy", "encode_jpeg")
    from . import ops
    qt = _device_tables(quality, ch)
    with torch.cuda.device(dev):
        b = n if is_tensor else staging.frames_per_block(n, h * w * ch, _BLOCK_BYTES)          # frames per call
        work = torch.empty(ops.mjpeg_workspace_bytes(b, h, w, ch), dtype=torch.uint8, device=dev)
        payload = torch.empty(ops.mjpeg_out_bytes(b, h, w, ch), dtype=torch.uint8, device=dev)
        lengths = torch.empty(b, dtype=torch.int64, device=dev)
        if is_tensor:
            ops.mjpeg_encode(frames.contiguous(), qt, work, payload, lengths)
            return payload, lengths
        head = jpeg_header(h, w, ch, quality)
        out = []
        for _, m, x in staging.Staged(b, frames.shape[1:], torch.uint8, dev).blocks(frames):
            ops.mjpeg_encode(x, qt, work, payload, lengths)
            out += split_payload(head, payload, lengths[:m])
        return out


def split_payload(head, payload, lengths):
    """The complete JPEGs of a device (payload, lengths) pair: only the compressed bytes cross to the host."""
    ln = lengths.cpu().numpy()
    data = payload[:int(ln.sum())].cpu().numpy().tobytes()
    ends = np.cumsum(ln)
    return [head + data[int(e - l):int(e)] for e, l in zip(ends, ln)]


# --------------------------------------------------------------------------------------------------------------- the container
AVI_MAX_BYTES = (1 << 32) - 1                 # AVI 1.0: RIFF sizes are 32 bits (OpenDML is not written)


def _avi_headers(nframes, fps, width, height, movi_bytes, max_chunk):
    rate, scale = int(round(fps * 1000)), 1000
    avih = struct.pack("<14I", int(round(1e6 / fps)) if fps > 0 else 0, 0, 0, 0x10, nframes, 0, 1, max_chunk, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, nframes, max_chunk, 0xFFFFFFFF, 0, 0, 0, min(width, 32767), min(height, 32767))
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    chunk = lambda tag, body: tag + struct.pack("<I", len(body)) + body
    strl = b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf)
    hdrl = b"hdrl" + chunk(b"avih", avih) + chunk(b"LIST", strl)
    return chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"


def _file_size(f):
    return f.tell()


def write_avi(path, jpegs, fps, width, height):
    """RIFF AVI 1.0 with one MJPG stream: hdrl (avih, strl: strh + strf), movi of 00dc chunks padded to even length, idx1. `jpegs` is
    any iterable of complete JPEG frames (a generator of unknown length works): one streaming pass, then the sizes and the frame
    count are patched in. fps is stored as rate / scale with scale = 1000. Returns the number of frames written.
    ValueError (naming the frame reached) before the file would pass 4 GiB - 1."""
    if not fps > 0:
        raise ValueError(f"write_avi: fps must be positive, got {fps}")
    head_len = 12 + len(_avi_headers(0, fps, width, height, 0, 0))
    index, max_chunk = [], 0
    with open(path, "wb") as f:
        f.write(b"\0" * head_len)
        for i, jpg in enumerate(jpegs):
            jpg = bytes(jpg)
            pad = len(jpg) & 1
            # what the file would be once this chunk and the index that covers it are written
            if _file_size(f) + 8 + len(jpg) + pad + 8 + 16 * (len(index) + 1) > AVI_MAX_BYTES:
                raise ValueError(f"write_avi: {path} would pass 4 GiB - 1 at frame {i}; AVI 1.0 cannot hold it (OpenDML is not written)")
            index.append((f.tell() - head_len + 4, len(jpg)))                          # offset of the chunk from the 'movi' fourcc
            f.write(b"00dc" + struct.pack("<I", len(jpg)) + jpg + b"\0" * pad)
            max_chunk = max(max_chunk, len(jpg))
        movi_bytes = f.tell() - head_len
        f.write(b"idx1" + struct.pack("<I", 16 * len(index)))
        f.write(b"".join(b"00dc" + struct.pack("<III", 0x10, off, ln) for off, ln in index))
        total = f.tell()
        f.seek(0)
        f.write(b"RIFF" + struct.pack("<I", total - 8) + b"AVI " + _avi_headers(len(index), fps, width, height, movi_bytes, max_chunk))
        assert f.tell() == head_len
    return len(index)


def read_avi(path):
    """(jpegs, fps, width, height) of an AVI as write_avi writes it: the frames by idx1, cross-checked against a walk of movi."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"RIFF" or data[8:12] != b"AVI " or struct.unpack_from("<I", data, 4)[0] + 8 != len(data):
        raise ValueError(f"read_avi: {path} is not a complete RIFF AVI file")
    info, movi, idx = {}, None, None

    def walk(lo, hi):
        nonlocal movi, idx
        while lo + 8 <= hi:
            tag, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
            body = lo + 8
            if body + size > hi:
                raise ValueError(f"read_avi: chunk {tag!r} at {lo} runs past its list")
            if tag == b"LIST":
                kind = data[body:body + 4]
                if kind == b"movi":
                    movi = (body, body + size)
                else:
                    walk(body + 4, body + size)
            elif tag == b"idx1":
                idx = (body, size)
            else:
                info[tag] = data[body:body + size]
            lo = body + size + (size & 1)
    walk(12, len(data))
    if movi is None or idx is None or b"strh" not in info or b"strf" not in info:
        raise ValueError(f"read_avi: {path} lacks hdrl, movi or idx1")
    strh = struct.unpack_from("<4s4sIHHIIII", info[b"strh"])
    width, height = struct.unpack_from("<ii", info[b"strf"], 4)
    if strh[0] != b"vids" or strh[1] != b"MJPG" or info[b"strf"][16:20] != b"MJPG":
        raise ValueError(f"read_avi: the stream of {path} is {strh[0]!r} / {strh[1]!r}, not vids / MJPG")
    fps = strh[7] / strh[6]
    walked, lo = [], movi[0] + 4
    while lo + 8 <= movi[1]:
        tag, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
        if tag == b"00dc":
            walked.append((lo - movi[0], size))
        lo += 8 + size + (size & 1)
    indexed = [struct.unpack_from("<4sIII", data, idx[0] + 16 * i) for i in range(idx[1] // 16)]
    if [(off, ln) for _, _, off, ln in indexed] != walked or any(t != b"00dc" for t, _, _, _ in indexed):
        raise ValueError(f"read_avi: idx1 of {path} does not match its movi list")
    return [data[movi[0] + off + 8:movi[0] + off + 8 + ln] for off, ln in walked], fps, width, height


def is_mjpeg_avi(path):
    """True when `path` starts like a RIFF AVI whose first stream header is vids / MJPG (reads the first 4 KiB only)."""
    with open(path, "rb") as f:
        head = f.read(4096)
    at = head.find(b"strh")
    return head[:4] == b"RIFF" and head[8:12] == b"AVI " and at > 0 and head[at + 8:at + 16] == b"vidsMJPG"


def decode_jpegs(jpegs):
    """uint8 [N,H,W,3] RGB of JPEG frames, decoded by PIL."""
    import io

    from PIL import Image
    return np.stack([np.asarray(Image.open(io.BytesIO(j)).convert("RGB")) for j in jpegs])


# ------------------------------------------------------------------------------------------------------------------ the decoder
# Baseline JPEG back to pixels. `decode_jpeg_numpy` is the contract: the entropy decoder is the loop of
# csrc/mjpeg_decode_core.h restated in Python, and every later step is int32 arithmetic that wraps, so the device
# (csrc/mjpeg_decode.hip) reproduces it bit for bit - for corrupt streams too, whose frames end in a status instead of pixels.
#
#   parse      SOI, APPn / COM (skipped), DQT (8-bit), SOF0 (8-bit, 1 or 3 components; luma 1x1, 2x1 or 2x2 over 1x1 chroma), DHT,
#              DRI, one interleaved SOS (Ss = 0, Se = 63, Ah = Al = 0). A frame without DHT gets the Annex K tables (the AVI MJPG
#              convention). Anything else raises UnsupportedJpeg naming what was found.
#   entropy    the scan is cut at FF D0..D7 (the RSTm numbers are not trusted); interval i holds MCUs [i DRI, (i + 1) DRI); FF xx
#              inside an interval is the byte FF; canonical codes, EXTEND of T.81 F.2.2.1; DC predictors start at 0 per interval;
#              coefficients are int16 at natural positions; an error ends the interval and gives the frame a status (the largest
#              code of its intervals; DECODE_STATUS has the names).
#   pixels     d = coef * Q; libjpeg's `islow` IDCT (CONST_BITS 13, PASS1_BITS 2; columns descaled by 11, rows by 18, + 128,
#              clamped); chroma cropped to ceil(W / 2) (x ceil(H / 2)) and upsampled by libjpeg's "fancy" triangle filters with
#              replicated edges; R = Y + ((91881 cr + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
#              B = Y + ((116130 cb + 32768) >> 16), clamped.
# These are the pixels of PIL (libjpeg-turbo) byte for byte when the frame is at least 5 pixels wide; with subsampled chroma and
# W <= 4, H >= 2 libjpeg-turbo's upsampler takes another edge path (tests/golden/mjpeg_decode_streams.npz has no such frame).
class UnsupportedJpeg(ValueError):
    """A JPEG this decoder does not read (progressive, 12-bit, CMYK, other sampling, ...): callers fall back to PIL."""


DECODE_STATUS = {0: "ok", 1: "code not in the Huffman table", 2: "DC category above 11 or AC size above 10", 3: "run past coefficient 63",
                 4: "interval ends before its MCUs are decoded", 5: "wrong number of restart intervals", 6: "DC predictor outside int16",
                 7: "scan is not ended by EOI"}
_ST_CODE, _ST_SIZE, _ST_RUN, _ST_SHORT, _ST_COUNT, _ST_DC, _ST_EOI = 1, 2, 3, 4, 5, 6, 7
_ANNEX_K_DC = ((_DC_L_BITS, _DC_VALS), (_DC_C_BITS, _DC_VALS))
_ANNEX_K_AC = ((_AC_L_BITS, _AC_L_VALS), (_AC_C_BITS, _AC_C_VALS))
HUFF_DTYPE = np.dtype([("look", "<u2", 256), ("maxcode", "<i4", 18), ("valoff", "<i4", 18), ("vals", "u1", 256)])     # MjdHuff, 912 bytes
TABLES_DTYPE = np.dtype([("dc", HUFF_DTYPE, 3), ("ac", HUFF_DTYPE, 3), ("zigzag", "u1", 64)])                         # MjdTables


class JpegInfo:
    """What parse_jpeg found: height, width, components, hs / vs (luma sampling), qtables uint16 [components, 64] in natural
    order, dc / ac: per component its (bits, vals), dri, scan_offset (the first byte behind SOS), header (the bytes before it)."""
    __slots__ = ("height", "width", "components", "hs", "vs", "qtables", "dc", "ac", "dri", "scan_offset", "header")

    @property
    def mcus(self):
        return -(-self.width // (8 * self.hs)), -(-self.height // (8 * self.vs))       # across, down

    @property
    def geometry(self):
        """(comp_off, comp_bw, frame_blocks): each component's block grid within a frame's coefficients (MjdGeom)."""
        mw, mh = self.mcus
        off, bw, at = [0, 0, 0], [0, 0, 0], 0
        for c in range(self.components):
            hc, vc = (self.hs, self.vs) if c == 0 else (1, 1)
            off[c], bw[c] = at, mw * hc
            at += mw * hc * mh * vc
        return off, bw, at


def _huff_decode_table(bits, vals):
    """One MjdHuff record from a DHT's 16 counts and its values."""
    bits, vals = [int(b) for b in bits], bytes(vals)
    if sum(bits) > 256 or len(vals) < sum(bits):
        raise UnsupportedJpeg(f"mjpeg: a DHT table counts {sum(bits)} codes for {len(vals)} values")
    t = np.zeros((), HUFF_DTYPE)
    t["maxcode"][:] = -1
    t["vals"][:len(vals[:256])] = np.frombuffer(vals[:256], np.uint8)
    code, k = 0, 0
    for ln in range(1, 17):
        nb = bits[ln - 1]
        if code + nb > (1 << ln):
            raise UnsupportedJpeg(f"mjpeg: a DHT table has more codes of length {ln} than the code space holds")
        if nb:
            t["valoff"][ln], t["maxcode"][ln] = k - code, code + nb - 1
            if ln <= 8:
                for i in range(nb):
                    t["look"][(code + i) << (8 - ln):(code + i + 1) << (8 - ln)] = (ln << 8) | vals[k + i]
        code, k = (code + nb) << 1, k + nb
    return t


def parse_jpeg(data):
    """JpegInfo of one baseline JPEG; UnsupportedJpeg (a ValueError) names what this decoder does not read."""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise UnsupportedJpeg("mjpeg: no SOI at the start")
    info = JpegInfo()
    info.dri = 0
    qt, dht, sof, p = {}, {}, None, 2
    while True:
        if p + 4 > len(data):
            raise UnsupportedJpeg("mjpeg: the header ends before SOS")
        if data[p] != 0xFF:
            raise UnsupportedJpeg(f"mjpeg: byte {data[p]:#04x} at {p} where a marker should be")
        m = data[p + 1]
        if m == 0xFF:                                                                      # a fill byte
            p += 1
            continue
        ln = struct.unpack_from(">H", data, p + 2)[0]
        seg = data[p + 4:p + 2 + ln]
        if ln < 2 or p + 2 + ln > len(data):
            raise UnsupportedJpeg(f"mjpeg: segment {m:#04x} at {p} runs past the end")
        p += 2 + ln
        if 0xE0 <= m <= 0xEF or m == 0xFE:
            continue
        if m == 0xDB:
            s = 0
            while s < len(seg):
                if seg[s] >> 4:
                    raise UnsupportedJpeg("mjpeg: 16-bit DQT table")
                if (seg[s] & 15) > 3 or s + 65 > len(seg):
                    raise UnsupportedJpeg("mjpeg: bad DQT segment")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[s + 1:s + 65], np.uint8)
                qt[seg[s] & 15] = t
                s += 65
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                if s + 17 > len(seg) or (seg[s] >> 4) > 1 or (seg[s] & 15) > 3:
                    raise UnsupportedJpeg("mjpeg: bad DHT segment")
                bits = tuple(seg[s + 1:s + 17])
                if s + 17 + sum(bits) > len(seg):
                    raise UnsupportedJpeg("mjpeg: bad DHT segment")
                dht[seg[s]] = (bits, seg[s + 17:s + 17 + sum(bits)])
                s += 17 + sum(bits)
        elif m == 0xC0:
            if sof is not None or len(seg) < 6:
                raise UnsupportedJpeg("mjpeg: bad or second SOF0")
            prec, h, w, nc = struct.unpack_from(">BHHB", seg)
            if prec != 8:
                raise UnsupportedJpeg(f"mjpeg: {prec}-bit samples")
            if nc not in (1, 3):
                raise UnsupportedJpeg(f"mjpeg: {nc} components")
            if h < 1 or w < 1 or len(seg) < 6 + 3 * nc:
                raise UnsupportedJpeg(f"mjpeg: bad SOF0 ({h} x {w})")
            sof = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
            samp = [(c[1], c[2]) for c in sof]
            if nc == 3 and (samp[0] not in ((1, 1), (2, 1), (2, 2)) or samp[1:] != [(1, 1), (1, 1)]):
                raise UnsupportedJpeg(f"mjpeg: sampling factors {samp}")
            info.height, info.width, info.components = h, w, nc
            info.hs, info.vs = samp[0] if nc == 3 else (1, 1)                              # one component: a block per MCU, whatever its factors
        elif 0xC1 <= m <= 0xCF and m not in (0xC8, 0xCC):
            raise UnsupportedJpeg(f"mjpeg: SOF{m - 0xC0} (only baseline SOF0 is read)")
        elif m == 0xDD:
            if len(seg) != 2:
                raise UnsupportedJpeg("mjpeg: bad DRI segment")
            info.dri = struct.unpack(">H", seg)[0]
        elif m == 0xDA:
            if sof is None:
                raise UnsupportedJpeg("mjpeg: SOS before SOF0")
            ns = seg[0] if seg else 0
            if ns != info.components or len(seg) != 4 + 2 * ns:
                raise UnsupportedJpeg(f"mjpeg: a scan of {ns} of {info.components} components (several scans)")
            if [seg[1 + 2 * i] for i in range(ns)] != [c[0] for c in sof]:
                raise UnsupportedJpeg("mjpeg: the scan's components are not the frame's, in order")
            if tuple(seg[1 + 2 * ns:]) != (0, 63, 0):
                raise UnsupportedJpeg(f"mjpeg: scan parameters Ss, Se, AhAl = {tuple(seg[1 + 2 * ns:])}")
            info.dc, info.ac, q = [], [], []
            for i in range(ns):
                td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if not dht:                                                                # no DHT at all: the Annex K tables (AVI MJPG)
                    if td > 1 or ta > 1:
                        raise UnsupportedJpeg(f"mjpeg: no DHT and table selectors {td}, {ta}")
                    info.dc.append(_ANNEX_K_DC[td])
                    info.ac.append(_ANNEX_K_AC[ta])
                else:
                    if td not in dht or (0x10 | ta) not in dht:
                        raise UnsupportedJpeg(f"mjpeg: the scan names Huffman tables {td}, {ta} that no DHT defines")
                    info.dc.append(dht[td])
                    info.ac.append(dht[0x10 | ta])
                if sof[i][3] not in qt:
                    raise UnsupportedJpeg(f"mjpeg: the frame names quantisation table {sof[i][3]} that no DQT defines")
                q.append(qt[sof[i][3]])
            info.qtables = np.stack(q)
            info.scan_offset, info.header = p, data[:p]
            return info
        elif m in (0xD9, 0xD8) or 0xD0 <= m <= 0xD7 or m == 0x01:
            raise UnsupportedJpeg(f"mjpeg: marker {m:#04x} before SOS")
        else:
            raise UnsupportedJpeg(f"mjpeg: segment {m:#04x} is not read")


def decode_tables(info):
    """The MjdTables record (TABLES_DTYPE) of a parsed frame: what both the twin and the device decode with."""
    t = np.zeros((), TABLES_DTYPE)
    for c in range(info.components):
        t["dc"][c] = _huff_decode_table(*info.dc[c])
        t["ac"][c] = _huff_decode_table(*info.ac[c])
    t["zigzag"][:] = ZIGZAG
    return t


def scan_intervals(data, info):
    """The restart intervals of one frame's scan, found with a vectorised search (FF D0..D7 cannot occur inside stuffed data):
    (int64 [k, 4] of byte offset into `data`, byte length, first MCU, MCU count; host status). The scan ends at the first FF xx
    with xx neither 00 nor D0..D7: status 7 unless that is EOI. Another number of intervals than the frame has: status 5, and the
    intervals both counts have are decoded."""
    a = np.frombuffer(data, np.uint8)[info.scan_offset:]
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    mark = nxt != 0
    ff, nxt = ff[mark], nxt[mark]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    stop = np.flatnonzero(~rst)
    status = 0
    if stop.size:
        end = int(ff[stop[0]])
        if nxt[stop[0]] != 0xD9:
            status = _ST_EOI
        ff = ff[:stop[0]]
    else:
        end, status = a.size, _ST_EOI
    starts = np.concatenate([[0], ff + 2])
    ends = np.concatenate([ff, [end]])
    mw, mh = info.mcus
    total = mw * mh
    per = info.dri or total
    want = -(-total // per)
    if starts.size != want:
        status = max(status, _ST_COUNT)
    k = min(starts.size, want)
    first = np.arange(k, dtype=np.int64) * per
    iv = np.stack([starts[:k] + info.scan_offset, ends[:k] - starts[:k], first, np.minimum(per, total - first)], axis=-1).astype(np.int64)
    return iv, status


def _decode_interval(data, lo, length, first_mcu, mcu_count, info, tabs, coef):
    """mjd_decode_interval of csrc/mjpeg_decode_core.h, line by line: `coef` int16 [frame_blocks, 64] is written in place and the
    status returned."""
    mw, mh = info.mcus
    comp_off, comp_bw, _ = info.geometry
    zz = [int(z) for z in ZIGZAG]
    p, end, acc, cnt = lo, lo + length, 0, 0
    pred = [0, 0, 0]

    def symbol(t):
        nonlocal p, acc, cnt
        while cnt <= 24 and p < end:
            v = data[p]
            p += 2 if v == 0xFF else 1
            acc, cnt = ((acc << 8) | v) & 0xFFFFFFFF, cnt + 8
        code = (acc >> (cnt - 16)) & 0xFFFF if cnt >= 16 else ((acc << (16 - cnt)) | ((1 << (16 - cnt)) - 1)) & 0xFFFF
        e = t[0][code >> 8]
        ln, sym = e >> 8, e & 255
        if e == 0:
            for ln in range(9, 17):
                c = code >> (16 - ln)
                if c <= t[1][ln]:
                    sym = t[3][(t[2][ln] + c) & 255]
                    break
            else:
                return -_ST_SHORT if cnt < 16 else -_ST_CODE
        if ln > cnt:
            return -_ST_SHORT
        cnt -= ln
        return sym

    def receive_extend(size):
        nonlocal p, acc, cnt
        while cnt <= 24 and p < end:
            v = data[p]
            p += 2 if v == 0xFF else 1
            acc, cnt = ((acc << 8) | v) & 0xFFFFFFFF, cnt + 8
        if size > cnt:
            return None
        v = (acc >> (cnt - size)) & ((1 << size) - 1)
        cnt -= size
        return v - (1 << size) + 1 if v < (1 << (size - 1)) else v

    for mcu in range(first_mcu, min(first_mcu + mcu_count, mw * mh)):
        my, mx = divmod(mcu, mw)
        for c in range(info.components):
            hc, vc = (info.hs, info.vs) if c == 0 else (1, 1)
            dc_t, ac_t = tabs[0][c], tabs[1][c]
            for by in range(vc):
                for bx in range(hc):
                    out = coef[comp_off[c] + (my * vc + by) * comp_bw[c] + mx * hc + bx]
                    s = symbol(dc_t)
                    if s < 0:
                        return -s
                    if s > 11:
                        return _ST_SIZE
                    if s:
                        d = receive_extend(s)
                        if d is None:
                            return _ST_SHORT
                        pred[c] += d
                    if not -32768 <= pred[c] <= 32767:
                        return _ST_DC
                    out[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = symbol(ac_t)
                        if rs < 0:
                            return -rs
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        if s > 10:
                            return _ST_SIZE
                        k += r
                        if k > 63:
                            return _ST_RUN
                        v = receive_extend(s)
                        if v is None:
                            return _ST_SHORT
                        out[zz[k]] = v
                        k += 1
    return 0


def _python_tables(tabs):
    as_lists = lambda t: (t["look"].tolist(), t["maxcode"].tolist(), t["valoff"].tolist(), t["vals"].tolist())
    return [as_lists(tabs["dc"][c]) for c in range(3)], [as_lists(tabs["ac"][c]) for c in range(3)]


def decode_coefficients(data, info=None):
    """(int16 [frame_blocks, 64] at natural positions, status) of one frame: the entropy stage of the twin alone."""
    info = info or parse_jpeg(data)
    data = bytes(data)
    iv, status = scan_intervals(data, info)
    tabs = _python_tables(decode_tables(info))
    coef = np.zeros((info.geometry[2], 64), np.int16)
    for lo, ln, first, count in iv.tolist():
        status = max(status, _decode_interval(data, lo, ln, first, count, info, tabs, coef))
    return coef, status


_I32 = np.int32


def _idct_pass(v, shift):
    """The 8-point islow butterfly along the last axis of an int32 array (wrapping), descaled by `shift`."""
    i0, i1, i2, i3, i4, i5, i6, i7 = (v[..., k] for k in range(8))
    z1 = (i2 + i6) * _I32(4433)
    t2 = z1 - i6 * _I32(15137)
    t3 = z1 + i2 * _I32(6270)
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * _I32(9633)
    a0, a1, a2, a3 = a0 * _I32(2446), a1 * _I32(16819), a2 * _I32(25172), a3 * _I32(12299)
    z1, z2 = z1 * _I32(-7373), z2 * _I32(-20995)
    z3, z4 = z3 * _I32(-16069) + z5, z4 * _I32(-3196) + z5
    a0, a1, a2, a3 = a0 + (z1 + z3), a1 + (z2 + z4), a2 + (z2 + z3), a3 + (z1 + z4)
    out = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    return np.stack([(o + _I32(1 << (shift - 1))) >> shift for o in out], axis=-1)


def _planes(coef, info):
    """int16 [n, frame_blocks, 64] -> per component its int32 sample plane [n, 8 block rows, 8 block columns]."""
    mw, mh = info.mcus
    comp_off, comp_bw, _ = info.geometry
    out = []
    with np.errstate(over="ignore"):
        for c in range(info.components):
            hc, vc = (info.hs, info.vs) if c == 0 else (1, 1)
            bh, bw = mh * vc, mw * hc
            d = coef[:, comp_off[c]:comp_off[c] + bh * bw].astype(np.int32) * info.qtables[c].astype(np.int32)
            d = d.reshape(-1, bh, bw, 8, 8)
            ws = _idct_pass(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)                       # columns
            px = np.clip(_idct_pass(ws, 18) + _I32(128), 0, 255)                          # rows
            out.append(px.transpose(0, 1, 3, 2, 4).reshape(-1, bh * 8, bw * 8))
    return out


def _upsample(a, vertical):
    """libjpeg's fancy upsampling of an int32 chroma plane [n, h, w]: h2v1, or h2v2 with `vertical`; edges replicate."""
    if vertical:
        up, dn = np.concatenate([a[:, :1], a[:, :-1]], 1), np.concatenate([a[:, 1:], a[:, -1:]], 1)
        r = np.empty((a.shape[0], 2 * a.shape[1], a.shape[2]), np.int32)
        r[:, 0::2], r[:, 1::2] = 3 * a + up, 3 * a + dn
        bias, shift = (8, 7), 4
    else:
        r, bias, shift = a, (1, 2), 2
    lf, rt = np.concatenate([r[..., :1], r[..., :-1]], -1), np.concatenate([r[..., 1:], r[..., -1:]], -1)
    out = np.empty(r.shape[:2] + (2 * r.shape[2],), np.int32)
    out[..., 0::2], out[..., 1::2] = (3 * r + lf + bias[0]) >> shift, (3 * r + rt + bias[1]) >> shift
    return out


def pixels_from_coefficients(coef, info):
    """uint8 [n,H,W,3] (or [n,H,W]) from int16 [n, frame_blocks, 64]: dequantisation, IDCT, upsampling, colour - the twin's arithmetic."""
    h, w = info.height, info.width
    planes = _planes(coef, info)
    if info.components == 1:
        return planes[0][:, :h, :w].astype(np.uint8)
    y = planes[0][:, :h, :w]
    ch = []
    for pl in planes[1:]:
        if info.hs == 2:
            pl = _upsample(pl[:, :-(-h // info.vs), :-(-w // 2)], info.vs == 2)
        ch.append(pl[:, :h, :w] - _I32(128))
    cb, cr = ch
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def _same_geometry(a, b):
    return (a.height, a.width, a.components) == (b.height, b.width, b.components)


def _status_error(i, status):
    return ValueError(f"mjpeg: frame {i} does not decode: {DECODE_STATUS[int(status)]} (status {int(status)})")


def decode_jpeg_numpy(jpegs):
    """uint8 [N,H,W,3] RGB (or [N,H,W] for 1-component frames) of N baseline JPEGs of one geometry: the contract of the decoder.
    Pure numpy and Python (the entropy decoder is a Python loop: small frames). ValueError names the first frame whose stream is
    corrupt and its status; UnsupportedJpeg what is not read."""
    jpegs = [bytes(j) for j in jpegs]
    if not jpegs:
        raise ValueError("mjpeg: no frames")
    out, first = [], None
    for i, j in enumerate(jpegs):
        info = parse_jpeg(j)
        first = first or info
        if not _same_geometry(first, info):
            raise ValueError(f"mjpeg: frame {i} is {info.height} x {info.width} x {info.components}, frame 0 {first.height} x {first.width} x {first.components}")
        coef, status = decode_coefficients(j, info)
        if status:
            raise _status_error(i, status)
        out.append(pixels_from_coefficients(coef[None], info)[0])
    return np.stack(out)


def _device_groups(jpegs):
    """Consecutive frames whose bytes up to the end of SOS are equal: [(info, first frame, frame count)]."""
    groups = []
    for i, j in enumerate(jpegs):
        if groups and j.startswith(groups[-1][0].header):
            groups[-1][2] += 1
        else:
            groups.append([parse_jpeg(j), i, 1])
    return groups


def device_call_inputs(jpegs, info):
    """What one vda_mjpeg_decode_u8 call uploads for frames that share `info`'s header: (scan uint8 [bytes], intervals int32 [k, 5]
    of frame, byte offset, byte length, first MCU, MCU count; host status int32 [n])."""
    ivs, status, at, so = [], np.zeros(len(jpegs), np.int32), 0, info.scan_offset
    for f, j in enumerate(jpegs):
        iv, status[f] = scan_intervals(j, info)
        iv[:, 0] += at - so
        ivs.append(np.concatenate([np.full((iv.shape[0], 1), f, np.int64), iv], axis=1))
        at += len(j) - so
    if at > 0x7ffffff0:
        raise ValueError(f"mjpeg: {at} bytes of scans in one call (at most 2^31 - 16): decode fewer frames at a time")
    scan = np.frombuffer(b"".join(j[so:] for j in jpegs) or b"\0", np.uint8)            # (never an empty upload)
    return scan, np.ascontiguousarray(np.concatenate(ivs), dtype=np.int32), status


def decode_jpeg(jpegs, device="cuda", to_host=True):
    """decode_jpeg_numpy's pixels from the device (vda_mjpeg_decode_u8, csrc/mjpeg_decode.hip): a numpy array, or with
    to_host=False a cuda uint8 tensor. The headers are parsed and the restart markers found on the host; consecutive frames with the
    same header (all frames of a video) go in one call: three launches - entropy decoding with one lane per restart interval,
    IDCT, upsampling and colour. A stream WITHOUT restart markers is one interval per frame, so one lane decodes the whole frame:
    correct, and slow by nature (tools/mjpeg_decode_bench.py puts a number on it). Raises as the twin does."""
    import torch
    jpegs = [bytes(j) for j in jpegs]
    if not jpegs:
        raise ValueError("mjpeg: no frames")
    dev = staging.cuda_device(device, "mjpeg", "decode_jpeg_numpy")
    from . import ops
    groups = _device_groups(jpegs)
    first = groups[0][0]
    for info, i, _ in groups:
        if not _same_geometry(first, info):
            raise ValueError(f"mjpeg: frame {i} is {info.height} x {info.width} x {info.components}, frame 0 {first.height} x {first.width} x {first.components}")
    n, h, w, ch = len(jpegs), first.height, first.width, first.components
    with torch.cuda.device(dev):
        out = torch.empty((n, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device=dev)
        status = np.zeros(n, np.int32)
        for info, i, m in groups:
            scan, iv, host_status = device_call_inputs(jpegs[i:i + m], info)
            scan_d = torch.from_numpy(scan.copy()).to(dev, non_blocking=True)
            work = torch.empty(ops.mjpeg_decode_workspace_bytes(m, h, w, ch, info.hs, info.vs, iv.shape[0]), dtype=torch.uint8, device=dev)
            st = torch.empty(m, dtype=torch.int32, device=dev)
            ops.mjpeg_decode(scan_d, iv, decode_tables(info), info.qtables, info.hs, info.vs, work, out[i:i + m], st)
            status[i:i + m] = np.maximum(st.cpu().numpy(), host_status)
        bad = np.flatnonzero(status)
        if bad.size:
            raise _status_error(bad[0], status[bad[0]])
        return out.cpu().numpy() if to_host else out


def iter_avi(path, stride=1, limit=None):
    """A RIFF AVI with one MJPG stream, read incrementally: first (fps, width, height), then the body of every 00dc chunk of movi
    in file order. Only the chunk in hand is in memory (read_avi holds the file and checks idx1 against it; this does neither).
    stride / limit: only frames 0, stride, 2 * stride, ... below `limit` (None: all) are yielded; the others are skipped in the
    container, their bytes never read, and the walk ends at `limit`."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"iter_avi: {path} is not a RIFF AVI file")
        info, told = {}, False
        while True:
            hd = f.read(8)
            if len(hd) < 8:
                break
            tag, size = hd[:4], struct.unpack("<I", hd[4:])[0]
            if tag == b"LIST":
                kind = f.read(4)
                if kind != b"movi":
                    continue                                                               # hdrl, strl, ...: their chunks are read as they come
                if b"strh" not in info or b"strf" not in info:
                    raise ValueError(f"iter_avi: {path} has no stream header before movi")
                strh = struct.unpack_from("<4s4sIHHIIII", info[b"strh"])
                width, height = struct.unpack_from("<ii", info[b"strf"], 4)
                if strh[0] != b"vids" or strh[1] != b"MJPG":
                    raise ValueError(f"iter_avi: the stream of {path} is {strh[0]!r} / {strh[1]!r}, not vids / MJPG")
                yield strh[7] / strh[6], width, height
                told, left, frame = True, size - 4, 0
                while left >= 8 and (limit is None or frame < limit):
                    hd = f.read(8)
                    if len(hd) < 8:
                        raise ValueError(f"iter_avi: {path} ends inside its movi list")
                    tag, n = struct.unpack("<4sI", hd)
                    left -= 8
                    if tag == b"LIST":                                                     # a 'rec ' list: its chunks follow
                        f.read(4)
                        left -= 4
                        continue
                    take = n + (n & 1)
                    if n > left:
                        raise ValueError(f"iter_avi: chunk {tag!r} of {path} runs past movi")
                    if tag == b"00dc":
                        frame += 1
                    if tag == b"00dc" and (frame - 1) % stride == 0:
                        body = f.read(n)
                        if len(body) != n:
                            raise ValueError(f"iter_avi: {path} ends inside a frame")
                        f.seek(n & 1, 1)
                        yield body
                    else:
                        f.seek(take, 1)
                    left -= take
                return
            body = f.read(size)
            f.seek(size & 1, 1)
            info[tag] = body
        if not told:
            raise ValueError(f"iter_avi: {path} has no movi list")


def _decode_block(jpegs, device):
    """uint8 [m,H,W,3] of a block of frames: on the device, or on the host by PIL when it is there and by the twin otherwise; what
    this decoder does not read goes to PIL."""
    try:
        if device is not None:
            x = decode_jpeg(jpegs, device)
        else:
            try:
                return decode_jpegs(jpegs)
            except ImportError:
                x = decode_jpeg_numpy(jpegs)
    except UnsupportedJpeg:
        return decode_jpegs(jpegs)
    return x if x.ndim == 4 else np.repeat(x[..., None], 3, axis=-1)


def avi_frame_blocks(path, device=None, block=None):
    """uint8 [m,H,W,3] blocks of `block` frames (default scheduler.STEP, a window's new frames) of a Motion-JPEG AVI, decoded as
    the file is read: what infer_video_depth_stream takes, so a long .avi runs in bounded memory."""
    if block is None:
        from .scheduler import STEP
        block = STEP
    frames = iter_avi(path)
    next(frames)
    held = []
    for j in frames:
        held.append(j)
        if len(held) == block:
            yield _decode_block(held, device)
            held = []
    if held:
        yield _decode_block(held, device)
