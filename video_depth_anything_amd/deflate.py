"""Raw deflate (RFC 1951) made on the device, and the .npz container around it: `run.py --save_npz` without zlib on one core
(csrc/deflate.hip, csrc/deflate_core.h).

The contract is `deflate_numpy`: every step is integer arithmetic with fixed tie-breaks, so the device reproduces the stream byte
for byte.

  chunks    the input is cut into independent chunks of CHUNK = 16384 bytes, a workgroup each; nothing refers across a chunk boundary.
            With `final` an empty input is one chunk of no bytes; without it, no chunk and an empty stream.
  tokens    a byte equal to its predecessor inside the chunk continues a run. A run's first byte is a literal; the other R bytes are
            cut from the front into distance-1 matches of 258 bytes and a rest: a rest of 3..257 bytes is one more match, a rest of 1
            or 2 is written as literals. (zlib's Z_RLE strategy: float32 depth gives a general LZ77 search nothing to find.)
            Byte k of those R bytes starts a token exactly when k % 258 == 0 or the rest is shorter than 3: no serial pass.
  lengths   the 286 literal/length counts (end-of-block counted once) sorted by (count, symbol); the two-queue Huffman merge, a
            leaf before an internal node of the same weight; depths above 15 are cut to 15 and the Kraft sum repaired by moving one
            code from the longest populated length below 15 down a level and one 15-bit code with it, until it is exact; then the
            lengths are dealt out in sorted order, the rarest symbols the longest (`code_lengths`; deflate_core.h is this, line by line).
  header    dynamic block; HLIT = through the last used symbol; one distance code (distance 1) of one bit when the chunk has a match,
            of zero bits when it has none; the HLIT + 1 code lengths are written one by one in a code-length code BUILT for them by
            the same `code_lengths`, limited to 7 bits, without the repeat symbols 16..18 (measured on depth data: a built code halves
            the header against a fixed 4/5-bit one, the repeat symbols then add nothing). At least two different
            lengths always occur (257..286 equal lengths cannot satisfy Kraft's equality), so that code is complete.
  bits      least significant bit first, Huffman codes bit-reversed; end-of-block; a chunk that is not the stream's last ends byte
            aligned with an empty stored block (zlib's sync flush, 00 00 FF FF behind the padding), so a stream is the concatenation
            of its chunks; the last chunk of a `final` call carries BFINAL on its block instead.
  stored    a chunk whose coded form would not be smaller than 5 + its bytes is one stored block (and so is a chunk of no bytes).

`savez_compressed` writes the ZIP container by hand (zipfile cannot take data that is already compressed): what np.load reads.
"""
import struct
import zlib

import numpy as np

from .staging import Staged, cuda_device, frames_per_block

CHUNK = 16384
NLIT = 286                      # literal/length symbols: 0..255 literals, 256 end of block, 257..285 lengths
MAX_BITS = 15
EOB = 256
STORED_OVERHEAD = 5             # a stored block: one byte of header bits, LEN, NLEN
_SYNC = b"\x00\x00\xff\xff"

# RFC 1951 3.2.5: (symbol, extra bits, first length) of the 29 length codes
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
# the order in which a dynamic header lists the code-length code's own lengths
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
CL_MAX_BITS = 7                 # the code-length code's own limit (its lengths are written in 3 bits)


def _length_tables():
    sym, nextra, extra = np.zeros(259, np.int64), np.zeros(259, np.int64), np.zeros(259, np.int64)
    for c in range(29):
        for ln in range(_LEN_BASE[c], _LEN_BASE[c + 1] if c < 28 else 259):     # code 284 ends at 257: 258 has its own code, 285
            sym[ln], nextra[ln], extra[ln] = 257 + c, _LEN_EXTRA[c], ln - _LEN_BASE[c]
    return sym, nextra, extra


_LEN_SYM, _LEN_NEXTRA, _LEN_EXTRAVAL = _length_tables()


def length_symbol(ln):
    """(symbol, number of extra bits, extra value) of a match length 3..258: the table of RFC 1951 3.2.5."""
    return int(_LEN_SYM[ln]), int(_LEN_NEXTRA[ln]), int(_LEN_EXTRAVAL[ln])


def _reverse(code, n):
    r = 0
    for _ in range(n):
        r, code = (r << 1) | (code & 1), code >> 1
    return r


def code_lengths(count, max_bits=MAX_BITS):
    """Huffman code lengths, at most `max_bits`, of the symbols with a non-zero count (the others get 0): the contract that
    csrc/deflate_core.h (dfl_build_lengths) restates. Integers only; ties go by (count, symbol)."""
    count = [int(c) for c in count]
    order = sorted((s for s in range(len(count)) if count[s] > 0), key=lambda s: (count[s], s))
    n = len(order)
    out = [0] * len(count)
    if n == 0:
        return out
    if n == 1:
        out[order[0]] = 1
        return out
    w = [count[s] for s in order]
    iw, pl, pi = [0] * (n - 1), [0] * n, [0] * (n - 1)
    li = ii = 0
    for j in range(n - 1):
        tot = 0
        for _ in range(2):
            if li < n and (ii >= j or w[li] <= iw[ii]):         # a leaf before an internal node of the same weight
                pl[li] = j
                tot += w[li]
                li += 1
            else:
                pi[ii] = j
                tot += iw[ii]
                ii += 1
        iw[j] = tot
    depth = [0] * (n - 1)
    for j in range(n - 3, -1, -1):
        depth[j] = depth[pi[j]] + 1
    blc = [0] * (max_bits + 1)
    for i in range(n):
        blc[min(depth[pl[i]] + 1, max_bits)] += 1
    total = sum(blc[b] << (max_bits - b) for b in range(1, max_bits + 1))
    while total > (1 << max_bits):                               # the Kraft sum in units of 2^-max_bits: each round takes one off
        blc[max_bits] -= 1
        for b in range(max_bits - 1, 0, -1):
            if blc[b]:
                blc[b] -= 1
                blc[b + 1] += 2
                break
        total -= 1
    i = 0
    for b in range(max_bits, 0, -1):                             # the rarest symbols get the longest codes
        for _ in range(blc[b]):
            out[order[i]] = b
            i += 1
    return out


def canonical_codes(lengths):
    """The canonical codes of RFC 1951 3.2.2 for `lengths`, each BIT-REVERSED (deflate writes Huffman codes most significant bit
    first into a stream that fills bytes from the least significant bit)."""
    lengths = [int(b) for b in lengths]
    blc = [0] * (MAX_BITS + 2)
    for b in lengths:
        blc[b] += 1
    blc[0] = 0
    nxt, code = [0] * (MAX_BITS + 2), 0
    for b in range(1, MAX_BITS + 1):
        code = (code + blc[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, b in enumerate(lengths):
        if b:
            out[s] = _reverse(nxt[b], b)
            nxt[b] += 1
    return out


def chunk_tokens(b):
    """The tokens of one chunk (uint8 [m], m >= 1) in stream order: (position, symbol, extra bits, extra value, is match)."""
    m = b.size
    i = np.arange(m)
    brk = np.ones(m, bool)
    brk[1:] = b[1:] != b[:-1]
    start = np.maximum.accumulate(np.where(brk, i, 0))
    nxt = np.minimum.accumulate(np.where(brk, i, m)[::-1])[::-1]                # the first break at or behind i
    end = np.concatenate([nxt[1:], [m]])                                       # the first break behind i: where i's run ends
    o, rest = i - start, end - start - 1
    k = o - 1
    seg = k // 258
    seglen = np.minimum(258, rest - seg * 258)
    lit = (o == 0) | (seglen < 3)
    mat = ~lit & (k - seg * 258 == 0)
    pos = np.flatnonzero(lit | mat)
    is_m = mat[pos]
    ln = np.where(is_m, seglen[pos], 3)
    sym = np.where(is_m, _LEN_SYM[ln], b[pos])
    return pos, sym, np.where(is_m, _LEN_NEXTRA[ln], 0), np.where(is_m, _LEN_EXTRAVAL[ln], 0), is_m


def _pack_bits(values, nbits):
    """Tokens (value, bit count <= 32) back to back, least significant bit first -> (uint8 bytes, bit count)."""
    values, nbits = np.asarray(values, np.uint64), np.asarray(nbits, np.int64)
    total = int(nbits.sum())
    bits = np.zeros((total + 7) // 8 * 8, np.uint8)
    idx = np.repeat(np.arange(nbits.size), nbits)
    within = np.arange(idx.size) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    bits[:total] = ((values[idx] >> within.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little"), total


def _stored(b, last):
    return bytes([1 if last else 0]) + struct.pack("<HH", b.size, b.size ^ 0xFFFF) + b.tobytes()


def encode_chunk(b, last, info=None):
    """One chunk's bytes. `last`: the final chunk of a final call (BFINAL, no sync flush). info: a dict that receives what the
    chunk did (stored, header bits, data bits, the lengths)."""
    b = np.ascontiguousarray(b, np.uint8).reshape(-1)
    m = b.size
    assert m <= CHUNK
    if m == 0:
        return _stored(b, last)
    pos, sym, nextra, extra, is_m = chunk_tokens(b)
    count = np.bincount(sym, minlength=NLIT)
    count[EOB] = 1
    lens = code_lengths(count)
    codes = canonical_codes(lens)
    hlit = max(257, int(np.flatnonzero(count)[-1]) + 1)
    has_match = bool(is_m.any())
    lens_a, codes_a = np.array(lens, np.int64), np.array(codes, np.int64)
    # header: BFINAL, BTYPE = 2, HLIT - 257, HDIST - 1 = 0, HCLEN - 4, the code-length code's own lengths, then the lengths in that code
    cl = list(lens[:hlit]) + [1 if has_match else 0]
    cl_lens = code_lengths(np.bincount(cl, minlength=19), CL_MAX_BITS)
    cl_codes = canonical_codes(cl_lens)
    assert sum(1 for b in cl_lens if b) >= 2                                   # (see the module's text: the code is complete)
    hclen = max(4, max(k + 1 for k, s in enumerate(_CL_ORDER) if cl_lens[s]))
    hv = [int(last), 2, hlit - 257, 0, hclen - 4] + [cl_lens[s] for s in _CL_ORDER[:hclen]] + [cl_codes[c] for c in cl]
    hn = [1, 2, 5, 5, 4] + [3] * hclen + [cl_lens[c] for c in cl]
    # a match: the length code, its extra bits, then the distance code '0' (one bit)
    tv = codes_a[sym] | (extra << lens_a[sym])
    tn = lens_a[sym] + nextra + is_m
    values = np.concatenate([np.array(hv, np.int64), tv, [codes[EOB]]])
    nbits = np.concatenate([np.array(hn, np.int64), tn, [lens[EOB]]])
    total = int(nbits.sum())
    coded_bytes = (total + 7) // 8 if last else (total + 3 + 7) // 8 + 4
    if info is not None:
        info.update(stored=coded_bytes >= m + STORED_OVERHEAD, header_bits=int(sum(hn)), data_bits=int(tn.sum()) + lens[EOB], lengths=lens,
                    matches=int(is_m.sum()), tokens=int(pos.size))
    if coded_bytes >= m + STORED_OVERHEAD:
        return _stored(b, last)
    if not last:
        values, nbits = np.concatenate([values, [0]]), np.concatenate([nbits, [3]])       # BFINAL = 0, BTYPE = 0; the padding is zeros
    body = _pack_bits(values, nbits)[0].tobytes()
    return body if last else body + _SYNC


def n_chunks(n, final=True):
    return max(1, -(-n // CHUNK)) if final else -(-n // CHUNK)


def out_bytes(n):
    """vda_deflate_out_bytes: no stream of n input bytes is longer (every chunk stored)."""
    return n + STORED_OVERHEAD * max(1, -(-n // CHUNK))


def _as_bytes(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, np.uint8)
    a = np.asarray(data)
    if not a.flags.c_contiguous:
        a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint8)


def deflate_numpy(data, final=True, info=None):
    """The raw deflate stream of `data` (bytes, or an array's C-order bytes): the integer host twin and the contract.
    final=False: a piece that ends byte aligned and open, to be followed by more. info: a list that receives a dict per chunk."""
    b = _as_bytes(data)
    out = []
    nch = n_chunks(b.size, final)
    for c in range(nch):
        d = {} if info is not None else None
        out.append(encode_chunk(b[c * CHUNK:(c + 1) * CHUNK], final and c == nch - 1, d))
        if info is not None:
            info.append(d)
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------------- CRC-32
_POLY = 0xEDB88320                    # zlib's polynomial, reflected: bit 31 is x^0


def _mulmod(a, b):
    """a(x) b(x) mod P(x) over GF(2) in the reflected representation."""
    p = 0
    for bit in range(31, -1, -1):
        if (a >> bit) & 1:
            p ^= b
        b = (b >> 1) ^ _POLY if b & 1 else b >> 1
    return p


def _x8n(n):
    """x^(8 n) mod P."""
    p, q = 0x80000000, 0x00800000     # x^0, x^8
    while n:
        if n & 1:
            p = _mulmod(q, p)
        q = _mulmod(q, q)
        n >>= 1
    return p


def crc32_combine(crc_a, crc_b, len_b):
    """zlib.crc32(a + b) from zlib.crc32(a), zlib.crc32(b) and len(b)."""
    return _mulmod(_x8n(int(len_b)), int(crc_a)) ^ int(crc_b)


class _CrcFold:
    """crc32_combine with a fixed len_b as four table look-ups: the per-chunk CRCs of a long stream are folded a chunk at a time."""

    def __init__(self, len_b):
        op = _x8n(len_b)
        basis = [_mulmod(op, 1 << k) for k in range(32)]
        self.t = []
        for byte in range(4):
            row = [0] * 256
            for v in range(1, 256):
                low = v & -v
                row[v] = row[v ^ low] ^ basis[8 * byte + low.bit_length() - 1]
            self.t.append(row)

    def __call__(self, crc_a, crc_b):
        t = self.t
        return t[0][crc_a & 255] ^ t[1][(crc_a >> 8) & 255] ^ t[2][(crc_a >> 16) & 255] ^ t[3][crc_a >> 24] ^ crc_b


_FOLD_CHUNK = None


def combine_chunk_crcs(crcs, n, crc=0):
    """The CRC-32 of `crc`'s bytes followed by n more, from those bytes' per-chunk CRCs (every chunk CHUNK long but the last)."""
    global _FOLD_CHUNK
    if n == 0:
        return crc
    if _FOLD_CHUNK is None:
        _FOLD_CHUNK = _CrcFold(CHUNK)
    crcs = [int(c) for c in crcs]
    full, tail = divmod(n, CHUNK)
    assert len(crcs) == full + (1 if tail else 0)
    for c in crcs[:full]:
        crc = _FOLD_CHUNK(crc, c)
    return crc32_combine(crc, crcs[-1], tail) if tail else crc


# ------------------------------------------------------------------------------------------------------------------ the device
_BLOCK_BYTES = 1 << 25                # input bytes staged at a time by deflate's numpy path: a multiple of CHUNK


class _Encoder:
    """vda_deflate_u8's workspace and outputs for inputs of up to `cap` bytes on `dev`, allocated once, and the call."""

    def __init__(self, dev, cap):
        import torch
        from . import ops
        self.ops = ops
        self.work = torch.empty(ops.deflate_workspace_bytes(cap), dtype=torch.uint8, device=dev)
        self.payload = torch.empty(ops.deflate_out_bytes(cap), dtype=torch.uint8, device=dev)
        self.length = torch.empty(1, dtype=torch.int64, device=dev)
        self.crcs = torch.empty(n_chunks(cap), dtype=torch.int32, device=dev)

    def __call__(self, x, final):
        """(the stream: a view of the payload, its length, the CRC-32 of x's bytes) of a device uint8 [n]."""
        self.ops.deflate(x, final, self.work, self.payload, self.length, self.crcs)
        ln, n = int(self.length.item()), x.numel()
        per_chunk = (self.crcs[:-(-n // CHUNK)].cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
        return self.payload[:ln], ln, combine_chunk_crcs(per_chunk, n)


class _Stager:
    """The numpy path for inputs of up to n bytes, at most `block` bytes at a time (staging.Staged): its buffers are allocated once
    per stream or file."""

    def __init__(self, dev, block, n):
        import torch
        assert block % CHUNK == 0 and block > 0
        block = CHUNK * frames_per_block(-(-n // CHUNK), CHUNK, block)     # no more than the chunks n fills
        self.staged, self.encode = Staged(block, (), torch.uint8, dev), _Encoder(dev, block)

    def pieces(self, b, final):
        """(stream bytes, CRC-32 of the input, input bytes) of every block of the uint8 array (or memory map) `b`."""
        if final and b.size == 0:                                           # one chunk of no bytes
            yield self.encode(self.staged.dev[:0], True)[0].cpu().numpy().tobytes(), 0, 0
        for lo, m, x in self.staged.blocks(b):
            stream, _, crc = self.encode(x, final and lo + m >= b.size)
            yield stream.cpu().numpy().tobytes(), crc, m


def deflate(data, device="cuda", final=True, block_bytes=None):
    """deflate_numpy's stream made by vda_deflate_u8. Bytes or a numpy array (a memory map is read block by block): staged
    `block_bytes` (a multiple of CHUNK, default 32 MiB) at a time, returns (bytes, crc32). A CUDA tensor (its contiguous bytes):
    returns (payload uint8 tensor, length, crc32) on its device and stream; only the length and the per-chunk CRCs (4 bytes per
    16 KiB) cross to the host."""
    import torch
    if isinstance(data, torch.Tensor):
        if not data.is_cuda:
            raise ValueError("deflate: takes a cuda tensor, bytes or a numpy array; deflate_numpy is the host twin")
        x = data.contiguous().reshape(-1).view(torch.uint8)
        with torch.cuda.device(x.device):
            return _Encoder(x.device, x.numel())(x, final)
    dev = cuda_device(device, "deflate", "deflate_numpy")
    b = _as_bytes(data)
    block = _BLOCK_BYTES if block_bytes is None else int(block_bytes)
    if block < CHUNK or block % CHUNK:
        raise ValueError(f"deflate: block_bytes must be a positive multiple of {CHUNK}, got {block_bytes!r}")
    with torch.cuda.device(dev):
        out, crc = [], 0
        for piece, piece_crc, m in _Stager(dev, block, b.size).pieces(b, final):
            out.append(piece)
            crc = crc32_combine(crc, piece_crc, m)
        return b"".join(out), crc


# --------------------------------------------------------------------------------------------------------------- the container
ZIP64_LIMIT = 0xFFFFFFFF
_DOS_TIME, _DOS_DATE = 0, (1980 - 1980) << 9 | 1 << 5 | 1          # 1980-01-01 00:00: what zipfile writes for "no date"


def npy_header(arr):
    """The .npy header np.save would put in front of `arr`'s C-order bytes."""
    import io
    if arr.dtype.hasobject:
        raise TypeError("deflate.savez_compressed: object arrays are not written (they need pickle)")
    f = io.BytesIO()
    np.lib.format.write_array_header_1_0(f, dict(descr=np.lib.format.dtype_to_descr(arr.dtype), fortran_order=False, shape=tuple(arr.shape)))
    return f.getvalue()


def _member_bytes(arr):
    """uint8 view of the array's C-order bytes; a memory map stays a memory map (read as it is sliced)."""
    if not arr.flags.c_contiguous:
        arr = np.ascontiguousarray(arr)
    return arr.reshape(-1).view(np.uint8)


def _twin_pieces(b, block):
    for lo in range(0, max(b.size, 1), block):
        piece = np.asarray(b[lo:lo + block])
        yield deflate_numpy(piece, final=lo + block >= b.size), zlib.crc32(piece), piece.size


def write_npz(path, arrays, pieces, zip64_limit=ZIP64_LIMIT):
    """The ZIP file of np.savez_compressed, written by hand: per array a member <key>.npy, method 8, whose stream is the .npy header
    as one stored block followed by the streams `pieces(uint8 bytes)` yields as (stream, crc32 of the piece's input, input bytes).
    ZIP64 extra fields and end records where a size or an offset reaches `zip64_limit`."""
    central = []
    with open(path, "wb") as f:
        for key, arr in arrays.items():
            arr = arr if isinstance(arr, np.ndarray) else np.asarray(arr)
            name = (key + ".npy").encode("utf-8")
            head = npy_header(arr)
            b = _member_bytes(arr)
            usize = len(head) + b.size
            big = STORED_OVERHEAD + len(head) + out_bytes(b.size) >= zip64_limit         # decided before the stream exists: by its bound
            offset = f.tell()
            extra = struct.pack("<HHQQ", 1, 16, 0, 0) if big else b""
            local = lambda crc, csize: struct.pack("<IHHHHHIIIHH", 0x04034B50, 45 if big else 20, 0x0800, 8, _DOS_TIME, _DOS_DATE, crc,
                                                   0xFFFFFFFF if big else csize, 0xFFFFFFFF if big else usize, len(name), len(extra)) + name
            f.write(local(0, 0) + extra)
            data_at = f.tell()
            f.write(b"\x00" + struct.pack("<HH", len(head), len(head) ^ 0xFFFF) + head)
            crc = zlib.crc32(head)
            for stream, piece_crc, m in pieces(b):
                f.write(stream)
                crc = crc32_combine(crc, piece_crc, m)
            end = f.tell()
            csize = end - data_at
            f.seek(offset)
            f.write(local(crc, csize) + (struct.pack("<HHQQ", 1, 16, usize, csize) if big else b""))
            f.seek(end)
            central.append((name, crc, csize, usize, offset, big))
        cd_at = f.tell()
        for name, crc, csize, usize, offset, big in central:
            fields = ([usize, csize] if big else []) + ([offset] if offset >= zip64_limit else [])
            extra = struct.pack("<HH" + "Q" * len(fields), 1, 8 * len(fields), *fields) if fields else b""
            f.write(struct.pack("<IHHHHHHIIIHHHHHII", 0x02014B50, 45 if fields else 20, 45 if fields else 20, 0x0800, 8, _DOS_TIME, _DOS_DATE, crc,
                                0xFFFFFFFF if big else csize, 0xFFFFFFFF if big else usize, len(name), len(extra), 0, 0, 0, 0o600 << 16,
                                0xFFFFFFFF if offset >= zip64_limit else offset) + name + extra)
        cd_size = f.tell() - cd_at
        n = len(central)
        if n >= 0xFFFF or cd_size >= zip64_limit or cd_at >= zip64_limit:
            at = f.tell()
            f.write(struct.pack("<IQHHIIQQQQ", 0x06064B50, 44, 45, 45, 0, 0, n, n, cd_size, cd_at))
            f.write(struct.pack("<IIQI", 0x07064B50, 0, at, 1))
            f.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, min(n, 0xFFFF), min(n, 0xFFFF), 0xFFFFFFFF if cd_size >= zip64_limit else cd_size,
                                0xFFFFFFFF if cd_at >= zip64_limit else cd_at, 0))
        else:
            f.write(struct.pack("<IHHHHIIH", 0x06054B50, 0, 0, n, n, cd_size, cd_at, 0))


def savez_compressed(path, device="cuda", _zip64_limit=ZIP64_LIMIT, _twin=False, _block_bytes=None, **arrays):
    """np.savez_compressed(path, **arrays) with the deflate streams made on `device`: one member <key>.npy per array, each the .npy
    header as a host-made stored block followed by the device stream of the array's C-order bytes; np.load reads it back bit for
    bit. A np.memmap is read block by block (32 MiB), so an array larger than memory can be written. device=None: np.savez_compressed
    itself. As numpy does, '.npz' is appended to a path that lacks it. (_twin: the same container fed by deflate_numpy, for tests;
    _zip64_limit: write ZIP64 records from that size on.)"""
    path = str(path)
    if not path.endswith(".npz"):
        path += ".npz"
    if device is None and not _twin:
        np.savez_compressed(path, **arrays)
        return path
    block = _BLOCK_BYTES if _block_bytes is None else int(_block_bytes)
    if block < CHUNK or block % CHUNK:
        raise ValueError(f"deflate: _block_bytes must be a positive multiple of {CHUNK}, got {_block_bytes!r}")
    if _twin:
        write_npz(path, arrays, lambda b: _twin_pieces(b, block), _zip64_limit)
        return path
    import torch
    dev = cuda_device(device, "deflate", "deflate_numpy")
    largest = max([np.asarray(a).nbytes if not isinstance(a, np.ndarray) else a.nbytes for a in arrays.values()] + [0])
    with torch.cuda.device(dev):
        stager = _Stager(dev, block, largest)
        write_npz(path, arrays, lambda b: stager.pieces(b, True), _zip64_limit)
    return path
