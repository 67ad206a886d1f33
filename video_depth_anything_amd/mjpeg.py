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
    is_tensor = isinstance(frames, torch.Tensor)
    if not is_tensor and not isinstance(frames, np.ndarray):
        frames = np.asarray(frames)
    n, h, w, ch = _check_frames(frames)
    _check_quality(quality)
    if is_tensor and not frames.is_cuda:
        raise ValueError("mjpeg: encode_jpeg takes a cuda tensor or a numpy array; encode_jpeg_numpy is the host twin")
    dev = frames.device if is_tensor else torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise ValueError(f"mjpeg: needs a cuda device, got {device!r}; encode_jpeg_numpy is the host twin")
    from . import ops
    qt = _device_tables(quality, ch)
    with torch.cuda.device(dev):
        if is_tensor:
            x = frames.contiguous()
            work = torch.empty(ops.mjpeg_workspace_bytes(n, h, w, ch), dtype=torch.uint8, device=dev)
            payload = torch.empty(ops.mjpeg_out_bytes(n, h, w, ch), dtype=torch.uint8, device=dev)
            lengths = torch.empty(n, dtype=torch.int64, device=dev)
            ops.mjpeg_encode(x, qt, work, payload, lengths)
            return payload, lengths
        head = jpeg_header(h, w, ch, quality)
        b = max(1, min(n, _BLOCK_BYTES // (h * w * ch)))
        host_in = torch.empty((b, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8).pin_memory()
        dev_in = torch.empty_like(host_in, device=dev)
        work = torch.empty(ops.mjpeg_workspace_bytes(b, h, w, ch), dtype=torch.uint8, device=dev)
        payload = torch.empty(ops.mjpeg_out_bytes(b, h, w, ch), dtype=torch.uint8, device=dev)
        lengths = torch.empty(b, dtype=torch.int64, device=dev)
        out = []
        for i in range(0, n, b):
            m = min(b, n - i)
            np.copyto(host_in.numpy()[:m], frames[i:i + m])
            dev_in[:m].copy_(host_in[:m], non_blocking=True)
            ops.mjpeg_encode(dev_in[:m], qt, work, payload, lengths)
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
