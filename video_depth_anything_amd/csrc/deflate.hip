// Raw deflate (RFC 1951) of a device byte buffer, for run.py --save_npz (video_depth_anything_amd/deflate.py). The
// contract is deflate.deflate_numpy and every step is integer arithmetic with fixed tie-breaks, so this file needs no special
// compile flag and reproduces the twin's stream byte for byte:
//
//   chunks    independent chunks of DFL_CHUNK = 16384 input bytes, one workgroup each
//   tokens    a run's first byte is a literal; its other R bytes are distance-1 matches of 258 from the front and a rest, which
//             is one more match when it is 3..257 long and literals when it is 1 or 2 (zlib's Z_RLE strategy)
//   code      dynamic Huffman, at most 15 bits (deflate_core.h); one distance code; the code lengths written one by one in a
//             code-length code built for them the same way (at most 7 bits, no repeat symbols)
//   end       end-of-block, then an empty stored block (sync flush) unless the chunk is the last of a final call, whose block
//             carries BFINAL; a chunk whose coded form is not smaller than 5 + its bytes is one stored block
//
// Launches. (a) encode (the steps behind the staging are deflate_chunk.h, which exr.hip shares): a workgroup stages its chunk in LDS, 64 bytes per thread (rows padded to 17 words: a wave's threads read
// their own rows without bank conflicts); each thread finds its bytes' run starts and ends from a 64-bit mask of run breaks and
// two workgroup scans (the latest break before it, the first behind it), counts its tokens' symbols into an LDS histogram, the
// symbols are ranked in parallel, ONE lane builds the code and then the code-length code (deflate_core.h), then bit lengths, a
// workgroup scan, and the bits go into zeroed LDS words - plain stores for the words a thread owns alone, OR-atomics for its first
// and last word, which neighbours share (OR is order-independent: the bytes never depend on scheduling) - and from there to the
// chunk's slot of the workspace.
// (b) crc: per chunk, the CRC-32 of its input bytes: each thread's 64 bytes by table, shifted to the chunk's end by a GF(2)
// multiplication and XOR-ed together. (c) offsets + pack: an exclusive prefix of the chunk lengths by one workgroup, then a
// workgroup per chunk copies its slot to its place in the payload; the total goes to `length`.
#include "deflate_chunk.h"

namespace {

// Bytes [0, m) of the chunk at `src` (any byte address) into the threads' rows: byte i lies in word (i >> 6) * DF_ROW + ((i & 63) >> 2).
// Whole aligned words are loaded and shifted together; a word is read only when at least one of its bytes is the chunk's (an aligned
// word never crosses a page, so the bytes of it outside the buffer are readable; their values go nowhere).
__device__ __forceinline__ void df_stage(const uint8_t* __restrict__ src, int m, uint32_t* rows) {
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3);
    const uint32_t* base = reinterpret_cast<const uint32_t*>(src - mis);
    for (int d = threadIdx.x; 4 * d < m; d += DF_T) {
        uint32_t v = base[d];                                                  // chunk bytes 4 d - mis ..: 4 d - mis < m holds
        if (mis) {
            const uint32_t hi = 4 * (d + 1) - (int)mis < m ? base[d + 1] : 0u;
            v = (v >> (8 * mis)) | (hi << (32 - 8 * mis));
        }
        rows[(d >> 4) * DF_ROW + (d & 15)] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------- (a) encode
// grid = chunks workgroups. `last_chunk`: the index of the chunk that carries BFINAL, or -1.
__global__ void __launch_bounds__(DF_T) deflate_encode_kernel(const uint8_t* __restrict__ in, long long n, long long last_chunk,
                                                              uint8_t* __restrict__ slots, int* __restrict__ chunk_len) {
    __shared__ DfShared S;
    const int t = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long at = chunk * DFL_CHUNK;
    const int m = (int)min((long long)DFL_CHUNK, n - at);                     // 0 only for the one chunk of an empty final stream
    const bool last = chunk == last_chunk;
    uint8_t* slot = slots + chunk * DF_SLOT;
    if (m <= 0) {                                                              // an empty stored block
        if (t == 0) {
            slot[0] = last ? 1 : 0, slot[1] = 0, slot[2] = 0, slot[3] = 0xff, slot[4] = 0xff;
            chunk_len[chunk] = DFL_STORED_OVERHEAD;
        }
        return;
    }
    df_clear(S);
    df_stage(in + at, m, S.rows);
    __syncthreads();
    df_encode_staged(S, m, last, slot, chunk_len + chunk);
}

// ---------------------------------------------------------------------------------------------------------------------- (b) crc
// a(x) b(x) mod P(x) over GF(2), zlib's CRC-32 polynomial in the reflected representation (bit 31 is x^0)
__device__ __forceinline__ uint32_t df_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 4
    for (int bit = 31; bit >= 0; --bit) {
        p ^= (a >> bit) & 1u ? b : 0u;
        b = (b >> 1) ^ (b & 1u ? 0xedb88320u : 0u);
    }
    return p;
}
// x^(8 n) mod P
__device__ __forceinline__ uint32_t df_x8n(uint32_t n) {
    uint32_t p = 0x80000000u, q = 0x00800000u;
    for (; n; n >>= 1) {
        if (n & 1u) p = df_mulmod(q, p);
        q = df_mulmod(q, q);
    }
    return p;
}

// grid = chunks workgroups: crc[chunk] = zlib's crc32 of the chunk's input bytes. With the register started at 0 and no final
// inversion the CRC is linear: a piece's value times x^(8 * bytes behind it), XOR-ed over the pieces, is the whole chunk's; the
// start value 0xffffffff adds itself times x^(8 m), and the result is inverted.
__global__ void __launch_bounds__(DF_T) deflate_crc_kernel(const uint8_t* __restrict__ in, long long n, uint32_t* __restrict__ crc) {
    __shared__ uint32_t rows[DF_T * DF_ROW];
    __shared__ uint32_t table[256];
    __shared__ uint32_t acc;
    const int t = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long at = chunk * DFL_CHUNK;
    const int m = (int)max(0ll, min((long long)DFL_CHUNK, n - at));
    {
        uint32_t c = (uint32_t)t;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1u ? 0xedb88320u : 0u);
        table[t] = c;
    }
    if (t == 0) acc = 0;
    if (m > 0) df_stage(in + at, m, rows);
    __syncthreads();
    const int valid = min(DF_SEG, max(0, m - t * DF_SEG));
    if (valid > 0) {
        uint32_t c = 0;
        for (int j = 0; j < valid; ++j) c = table[(c ^ df_byte(rows, t * DF_SEG + j)) & 0xffu] ^ (c >> 8);
        const uint32_t behind = (uint32_t)(m - (t * DF_SEG + valid));
        if (c) atomicXor(&acc, behind ? df_mulmod(c, df_x8n(behind)) : c);  // XOR: the order does not matter
    }
    __syncthreads();
    if (t == 0) crc[chunk] = m > 0 ? acc ^ df_mulmod(0xffffffffu, df_x8n((uint32_t)m)) ^ 0xffffffffu : 0u;
}

// --------------------------------------------------------------------------------------------------------- (c) offsets and pack
// one workgroup: offset[c] = the sum of chunk_len[0 .. c), *length = the sum of all
__global__ void __launch_bounds__(DF_T) deflate_offsets_kernel(const int* __restrict__ chunk_len, long long chunks, long long* __restrict__ offset,
                                                               long long* __restrict__ length) {
    __shared__ uint32_t sh[DF_T / 64];
    long long carry = 0;
    for (long long base = 0; base < chunks; base += DF_T) {
        const long long c = base + threadIdx.x;
        const uint32_t v = c < chunks ? (uint32_t)chunk_len[c] : 0u;
        uint32_t total;
        const uint32_t before = df_scan(v, total, sh);                         // 256 lengths of at most 16389: far below 2^32
        if (c < chunks) offset[c] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *length = carry;
}

// grid = chunks workgroups: the chunk's slot to its place in the payload. The destination may start at any byte: a head of at most
// 3 bytes, whole words put together from two of the slot's, a tail of at most 3 bytes.
__global__ void __launch_bounds__(DF_T) deflate_pack_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ chunk_len,
                                                            const long long* __restrict__ offset, uint8_t* __restrict__ out) {
    const long long chunk = blockIdx.x;
    const uint8_t* src = slots + chunk * DF_SLOT;
    const uint32_t* srcw = reinterpret_cast<const uint32_t*>(src);
    uint8_t* dst = out + offset[chunk];
    const int len = chunk_len[chunk];
    const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    const int words = (len - head) >> 2;
    if ((int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    uint32_t* dstw = reinterpret_cast<uint32_t*>(dst + head);
    const int sh = 8 * head;                                                   // the slot is word aligned: source byte head + 4 i is byte `head` of word i
    for (int i = threadIdx.x; i < words; i += DF_T) {
        const uint32_t lo = srcw[i];
        dstw[i] = sh ? (lo >> sh) | (srcw[i + 1] << (32 - sh)) : lo;           // word i + 1 < DF_SLOT / 4: head + 4 i + 4 <= len <= DF_SLOT - 11
    }
    const int done = head + 4 * words;
    if ((int)threadIdx.x < len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

struct DfLayout {
    size_t chunks, slots, chunk_len, offset, total, out;
};

DfLayout df_layout(size_t n) {
    DfLayout L;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    L.chunks = n ? (n + DFL_CHUNK - 1) / DFL_CHUNK : 1;
    L.slots = 0;
    L.chunk_len = L.slots + L.chunks * DF_SLOT;
    L.offset = L.chunk_len + up16(L.chunks * 4);
    L.total = L.offset + up16(L.chunks * 8);
    L.out = n + DFL_STORED_OVERHEAD * L.chunks;
    return L;
}

constexpr size_t DF_MAX_BYTES = (size_t)1 << 44;                               // 2^30 chunks: grid sizes and byte offsets stay far inside their types

}  // namespace

extern "C" size_t vda_deflate_workspace_bytes(size_t n) { return n <= DF_MAX_BYTES ? df_layout(n).total : 0; }

extern "C" size_t vda_deflate_out_bytes(size_t n) { return n <= DF_MAX_BYTES ? df_layout(n).out : 0; }

extern "C" int vda_deflate_u8(const uint8_t* in, size_t n, int final, void* workspace, size_t workspace_bytes, uint8_t* out, size_t out_capacity,
                              long long* length, uint32_t* crcs, vda_stream_t stream) {
    VDA_REQUIRE(in || n == 0, "vda_deflate_u8: in is null");
    VDA_REQUIRE(workspace, "vda_deflate_u8: workspace is null");
    VDA_REQUIRE(out, "vda_deflate_u8: out is null");
    VDA_REQUIRE(length, "vda_deflate_u8: length is null");
    VDA_REQUIRE(crcs, "vda_deflate_u8: crcs is null");
    VDA_REQUIRE(n <= DF_MAX_BYTES, "vda_deflate_u8: bad size n=%zu (at most 2^44 bytes a call)", n);
    VDA_REQUIRE(final == 0 || final == 1, "vda_deflate_u8: bad final=%d (0 or 1)", final);
    VDA_REQUIRE(((uintptr_t)workspace & 15) == 0, "vda_deflate_u8: workspace is not 16-byte aligned");
    VDA_REQUIRE(((uintptr_t)length & 7) == 0, "vda_deflate_u8: length is not 8-byte aligned");
    VDA_REQUIRE(((uintptr_t)crcs & 3) == 0, "vda_deflate_u8: crcs is not 4-byte aligned");
    const DfLayout L = df_layout(n);
    VDA_REQUIRE(workspace_bytes >= L.total, "vda_deflate_u8: workspace capacity %zu is below the %zu bytes of vda_deflate_workspace_bytes", workspace_bytes,
                L.total);
    VDA_REQUIRE(out_capacity >= L.out, "vda_deflate_u8: out capacity %zu is below the %zu bytes of vda_deflate_out_bytes", out_capacity, L.out);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    uint8_t* slots = ws + L.slots;
    int* chunk_len = reinterpret_cast<int*>(ws + L.chunk_len);
    long long* offset = reinterpret_cast<long long*>(ws + L.offset);
    // an empty input is one chunk of no bytes when the stream ends here, and no chunk (an empty piece) when it goes on
    const long long chunks = n ? (long long)L.chunks : (final ? 1 : 0);
    const long long last_chunk = final ? chunks - 1 : -1;
    const dim3 block(DF_T);
    if (chunks > 0) {
        hipLaunchKernelGGL(deflate_encode_kernel, dim3((unsigned)chunks), block, 0, (hipStream_t)stream, in, (long long)n, last_chunk, slots, chunk_len);
        VDA_LAUNCH_CHECK();
        hipLaunchKernelGGL(deflate_crc_kernel, dim3((unsigned)chunks), block, 0, (hipStream_t)stream, in, (long long)n, crcs);
        VDA_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(deflate_offsets_kernel, dim3(1), block, 0, (hipStream_t)stream, chunk_len, chunks, offset, length);
    VDA_LAUNCH_CHECK();
    if (chunks > 0) {
        hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)chunks), block, 0, (hipStream_t)stream, slots, chunk_len, offset, out);
        VDA_LAUNCH_CHECK();
    }
    return 0;
}
