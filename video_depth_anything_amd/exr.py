"""OpenEXR depth frames with ZIP compression made on the device: `run.py --save_exr` without the OpenEXR library
(csrc/exr.hip, csrc/deflate_chunk.h), and a reader for such files that needs numpy and zlib only.

The file is a single-part scanline file, every number little-endian:

  magic     76 2F 31 01, version 02 00 00 00
  header    attributes `name\\0 type\\0 int32 size, value`, in the order exr_header writes them, then one 00
  table     nb = ceil(h / lines) uint64: the position in the file of every block (lines = 16 for ZIP, 1 for ZIPS and none)
  blocks    int32 y, int32 dataSize, dataSize bytes. A block's raw bytes are its scanlines back to back (within a scanline the
            channels in alphabetical order, each its w values), L bytes. dataSize == L: the raw bytes themselves. Otherwise a zlib
            stream of the FILTERED bytes: the even bytes, then the odd ones (`t`), then f[0] = t[0], f[i] = (t[i] - t[i-1] + 128) & 255
            straight across the middle. A block is compressed only when that is strictly shorter than L.

The contract of the device is `encode_exr_numpy(depth)` with compress=None, the integer host twin: a block's f is cut into
k = ceil(L / 16384) BALANCED chunks of q = 64 ceil(L / (64 k)) bytes (the last shorter; a 518-wide block is 3 x 11 072 bytes, not
16 384 + 16 384 + 384 with a whole Huffman header for 384 bytes), each chunk is deflate.encode_chunk (BFINAL on the block's last,
a sync flush behind the others), and the stream is 78 01, the chunks, the Adler-32 of f big-endian.
"""
import os
import struct
import zlib

import numpy as np

from . import deflate, staging

MAGIC = b"\x76\x2f\x31\x01"
VERSION = 2
TILED, LONG_NAMES, DEEP, MULTIPART = 0x200, 0x400, 0x800, 0x1000           # flag bits of the version word
COMPRESSION = {"none": 0, "zips": 2, "zip": 3}
LINES = {0: 1, 2: 1, 3: 16}                                               # scanlines per block
PIXEL = {0: np.dtype("<u4"), 1: np.dtype("<f2"), 2: np.dtype("<f4")}      # UINT, HALF, FLOAT
ZIP_LINES = 16
ADLER = 65521
_STAGE_BYTES = 1 << 25                                                    # depth bytes staged at a time by the numpy path


def _attr(name, kind, value):
    return name.encode() + b"\0" + kind.encode() + b"\0" + struct.pack("<i", len(value)) + value


def exr_header(w, h, channel="Z", compression="zip"):
    """Magic, version and header of a w x h file with one FLOAT channel: what OpenEXR.Header(w, h) with that channel gives the
    reference's writer. 277 bytes for a one-letter channel name."""
    w, h = int(w), int(h)
    if w < 1 or h < 1:
        raise ValueError(f"exr_header: bad size {w} x {h}")
    if compression not in COMPRESSION:
        raise ValueError(f"exr_header: compression must be one of {sorted(COMPRESSION)}, got {compression!r}")
    chlist = channel.encode() + b"\0" + struct.pack("<iB3xii", 2, 0, 1, 1) + b"\0"
    window = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (MAGIC + struct.pack("<I", VERSION)
            + _attr("channels", "chlist", chlist)
            + _attr("compression", "compression", bytes([COMPRESSION[compression]]))
            + _attr("dataWindow", "box2i", window)
            + _attr("displayWindow", "box2i", window)
            + _attr("lineOrder", "lineOrder", b"\0")
            + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
            + b"\0")


def filter_bytes(raw):
    """f of a block's raw bytes (uint8 [L])."""
    raw = np.asarray(raw, np.uint8).reshape(-1)
    t = np.concatenate([raw[0::2], raw[1::2]])
    f = t.copy()
    f[1:] = t[1:] - t[:-1] + np.uint8(128)                                # uint8 arithmetic wraps: & 255
    return f


def unfilter_bytes(f):
    """filter_bytes undone."""
    f = np.asarray(f, np.uint8).reshape(-1)
    d = f.astype(np.int64)
    d[1:] -= 128
    t = (np.cumsum(d) & 255).astype(np.uint8)
    half = (f.size + 1) // 2
    raw = np.empty(f.size, np.uint8)
    raw[0::2], raw[1::2] = t[:half], t[half:]
    return raw


def block_chunks(L):
    """(k, q): the chunks of a block of L filtered bytes and the bytes of each but the last."""
    k = -(-L // deflate.CHUNK)
    return k, 64 * -(-L // (64 * k))


def adler32(f):
    """zlib.adler32 in the closed form the device sums in pieces: s1 = 1 + sum f, s2 = L + sum (L - i) f[i], both mod 65521."""
    f = np.asarray(f, np.uint8).reshape(-1).astype(np.uint64)
    L = f.size
    s1 = (1 + int(f.sum())) % ADLER
    s2 = (L + int((f * (np.uint64(L) - np.arange(L, dtype=np.uint64))).sum())) % ADLER
    return s2 << 16 | s1


def zip_stream_twin(f):
    """The zlib stream the device makes of a block's filtered bytes."""
    k, q = block_chunks(f.size)
    return b"\x78\x01" + b"".join(deflate.encode_chunk(f[c * q:(c + 1) * q], c == k - 1) for c in range(k)) + struct.pack(">I", adler32(f))


def _frame(depth):
    d = np.asarray(depth)
    if d.ndim != 2 or d.size == 0:
        raise ValueError(f"exr: a frame is a non-empty [h, w] array, got {d.shape}")
    return np.ascontiguousarray(d, dtype=np.float32)                      # float32 in: the bits as they are, NaN payloads too


def encode_exr_numpy(depth, compress=None, info=None):
    """The bytes of the EXR file of one float32 [h, w] frame, channel Z, ZIP. compress=None: the integer host twin, the device's
    bytes; compress=zlib.compress (any bytes -> zlib stream): a fast host writer. info: a list that receives per block True when
    it was written compressed."""
    d = _frame(depth)
    h, w = d.shape
    head = exr_header(w, h)
    nb = -(-h // ZIP_LINES)
    blocks = []
    for b in range(nb):
        raw = d[ZIP_LINES * b:ZIP_LINES * (b + 1)].reshape(-1).view(np.uint8)
        f = filter_bytes(raw)
        z = zip_stream_twin(f) if compress is None else compress(f.tobytes())
        data = z if len(z) < raw.size else raw.tobytes()
        if info is not None:
            info.append(len(z) < raw.size)
        blocks.append(struct.pack("<ii", ZIP_LINES * b, len(data)) + data)
    at, table = len(head) + 8 * nb, []
    for blk in blocks:
        table.append(at)
        at += len(blk)
    return head + struct.pack(f"<{nb}Q", *table) + b"".join(blocks)


# ------------------------------------------------------------------------------------------------------------------ the device
def _frames3(depths):
    if depths.ndim == 2:
        depths = depths[None]
    if depths.ndim != 3 or min(depths.shape) < 1:
        raise ValueError(f"exr: depths must be non-empty [frames, h, w] or [h, w], got {tuple(depths.shape)}")
    return depths


class _Encoder:
    """vda_exr_zip_f32's workspace and outputs for up to `cap` frames of h x w on `dev`, allocated once, and the call."""

    def __init__(self, dev, cap, h, w):
        import torch
        from . import ops
        self.ops = ops
        self.work = torch.empty(ops.exr_workspace_bytes(cap, h, w), dtype=torch.uint8, device=dev)
        self.payload = torch.empty(ops.exr_payload_bytes(cap, h, w), dtype=torch.uint8, device=dev)
        self.offsets = torch.empty(cap + 1, dtype=torch.int64, device=dev)

    def __call__(self, x, header_bytes):
        """(payload uint8, offsets int64 [frames + 1]) of a cuda fp32 [n, h, w] tensor with dense frames, n <= cap."""
        self.ops.exr_zip(x, header_bytes, self.work, self.payload, self.offsets)
        return self.payload, self.offsets[:x.shape[0] + 1]


def _dense(x):
    h, w = x.shape[1:]
    ok = x.stride(2) == 1 and x.stride(1) == w and (x.shape[0] == 1 or x.stride(0) >= h * w)
    return x if ok else x.contiguous()


def _files_of(payload, offsets, head):
    """The files of a device payload: one copy of the bytes in use to the host, cut at the offsets."""
    off = offsets.cpu().numpy()
    data = payload[:int(off[-1])].cpu().numpy()
    return [head + data[int(off[i]):int(off[i + 1])].tobytes() for i in range(off.size - 1)]


def _iter_files(depths, device, frames_per_block):
    """The files of the frames, a block of frames at a time: a cuda tensor is read in place, a host array goes through
    staging.Staged. device None: the host writer with zlib.compress."""
    import torch
    on_device = isinstance(depths, torch.Tensor) and depths.is_cuda
    if on_device:
        d = _frames3(depths)
        d = _dense(d if d.dtype == torch.float32 else d.float())
        dev = d.device
    else:
        if isinstance(depths, torch.Tensor):
            depths = depths.numpy()
        d = _frames3(depths if isinstance(depths, np.ndarray) else np.asarray(depths))
        if device is None:
            for frame in d:
                yield encode_exr_numpy(frame, compress=zlib.compress)
            return
        dev = staging.cuda_device(device, "exr", "encode_exr_numpy")
    n, h, w = d.shape
    head = exr_header(w, h)
    step = staging.frames_per_block(n, 4 * h * w, _STAGE_BYTES) if frames_per_block is None else min(int(frames_per_block), n)
    if step < 1:
        raise ValueError(f"exr: frames_per_block must be at least 1, got {frames_per_block!r}")
    with torch.cuda.device(dev):
        encode = _Encoder(dev, step, h, w)
        if on_device:
            views = (d[lo:lo + step] for lo in range(0, n, step))
        else:                                                                 # a memory map is read here, a block of it at a time
            views = (x for _, _, x in staging.Staged(step, (h, w), torch.float32, dev).blocks(d, casting="same_kind"))
        for x in views:
            yield from _files_of(*encode(x, len(head)), head)


def encode_exr(depths, device="cuda", frames_per_block=None):
    """encode_exr_numpy's files made by vda_exr_zip_f32. A CUDA tensor [frames, h, w] (or [h, w]; float32, frames dense - a strided
    view between frames is read in place): returns (payload uint8 tensor, offsets int64 tensor [frames + 1]) on its device and
    stream; frame f's file is exr_header(w, h) followed by payload[offsets[f]:offsets[f + 1]]. A numpy array or memory map: staged
    `frames_per_block` frames at a time (default: 32 MiB of them), returns the list of the files' bytes."""
    import torch
    if isinstance(depths, torch.Tensor) and depths.is_cuda:
        x = _frames3(depths)
        if x.dtype != torch.float32:
            raise ValueError(f"encode_exr: a cuda tensor must be float32, got {x.dtype}")
        x = _dense(x)
        with torch.cuda.device(x.device):
            return _Encoder(x.device, *x.shape)(x, len(exr_header(x.shape[2], x.shape[1])))
    if isinstance(depths, torch.Tensor):
        raise ValueError("encode_exr: takes a cuda tensor or a numpy array; encode_exr_numpy is the host twin")
    staging.cuda_device(device, "exr", "encode_exr_numpy")
    return list(_iter_files(depths, device, frames_per_block))


def write_exr_sequence(depths, directory, device="cuda", pattern="frame_{:05d}.exr", frames_per_block=None):
    """One file per frame of depths [frames, h, w] (a cuda tensor, a numpy array or a memory map, which is read a block of frames at
    a time) into `directory`, named pattern.format(index): the reference's <name>_depths_exr/frame_00000.exr ... Returns the paths.
    device=None: the host writer (zlib.compress), for a machine without a GPU."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for i, data in enumerate(_iter_files(depths, device, frames_per_block)):
        path = os.path.join(directory, pattern.format(i))
        with open(path, "wb") as f:
            f.write(data)
        paths.append(path)
    return paths


# ------------------------------------------------------------------------------------------------------------------ the reader
def _cstr(buf, at):
    end = buf.index(b"\0", at)
    return buf[at:end].decode("latin-1"), end + 1


def read_exr(path):
    """{channel: [h, w] array} of a single-part scanline file (a path, or the file's bytes): compression none, ZIPS or ZIP; FLOAT
    (float32), HALF (float16) or UINT (uint32) channels, any number of them. ValueError for what it does not read: tiled,
    multi-part and deep files, other compressions, subsampled channels."""
    if isinstance(path, (bytes, bytearray, memoryview)):
        buf = bytes(path)
    else:
        with open(path, "rb") as f:
            buf = f.read()
    if len(buf) < 9 or buf[:4] != MAGIC:
        raise ValueError("read_exr: not an OpenEXR file (magic)")
    version, = struct.unpack_from("<I", buf, 4)
    if version & 0xFF != VERSION:
        raise ValueError(f"read_exr: file format version {version & 0xFF}, reads 2")
    for bit, what in ((TILED, "tiled"), (DEEP, "deep"), (MULTIPART, "multi-part")):
        if version & bit:
            raise ValueError(f"read_exr: {what} files are not read (version word {version:#x})")
    at, attrs = 8, {}
    while True:
        name, at = _cstr(buf, at)
        if not name:
            break
        kind, at = _cstr(buf, at)
        size, = struct.unpack_from("<i", buf, at)
        attrs[name] = (kind, buf[at + 4:at + 4 + size])
        at += 4 + size
    for need in ("channels", "compression", "dataWindow"):
        if need not in attrs:
            raise ValueError(f"read_exr: the header lacks {need}")
    comp = attrs["compression"][1][0]
    if comp not in LINES:
        raise ValueError(f"read_exr: compression {comp} is not read (0 none, 2 ZIPS, 3 ZIP)")
    lines = LINES[comp]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if w < 1 or h < 1:
        raise ValueError(f"read_exr: bad dataWindow {x0, y0, x1, y1}")
    channels, ch, c_at = [], attrs["channels"][1], 0
    while ch[c_at]:
        cname, c_at = _cstr(ch, c_at)
        ptype, _, xs, ys = struct.unpack_from("<iB3xii", ch, c_at)
        c_at += 16
        if ptype not in PIXEL:
            raise ValueError(f"read_exr: channel {cname} has pixel type {ptype}")
        if xs != 1 or ys != 1:
            raise ValueError(f"read_exr: channel {cname} is subsampled ({xs}, {ys})")
        channels.append((cname, PIXEL[ptype]))
    line_bytes = sum(dt.itemsize for _, dt in channels) * w
    out = {cname: np.empty((h, w), dt.newbyteorder("=")) for cname, dt in channels}
    nb = -(-h // lines)
    for pos in struct.unpack_from(f"<{nb}Q", buf, at):
        y, size = struct.unpack_from("<ii", buf, pos)
        row = y - y0
        rows = min(lines, h - row)
        if row < 0 or rows < 1:
            raise ValueError(f"read_exr: a block at y = {y} outside the dataWindow")
        data = buf[pos + 8:pos + 8 + size]
        L = rows * line_bytes
        if len(data) != size or size > L:
            raise ValueError(f"read_exr: a block of {size} bytes at y = {y} (its rows hold {L})")
        if size < L:
            if comp == 0:
                raise ValueError(f"read_exr: an uncompressed block of {size} bytes at y = {y} (its rows hold {L})")
            f = np.frombuffer(zlib.decompress(data), np.uint8)
            if f.size != L:
                raise ValueError(f"read_exr: the block at y = {y} inflates to {f.size} bytes, its rows hold {L}")
            raw = unfilter_bytes(f)
        else:
            raw = np.frombuffer(data, np.uint8)
        raw = raw.reshape(rows, line_bytes)
        o = 0
        for cname, dt in channels:
            n = dt.itemsize * w
            out[cname][row:row + rows] = np.ascontiguousarray(raw[:, o:o + n]).view(dt).reshape(rows, w)
            o += n
    return out
