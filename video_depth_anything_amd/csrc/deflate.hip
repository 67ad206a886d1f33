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
// Launches. (a) encode: a workgroup stages its chunk in LDS, 64 bytes per thread (rows padded to 17 words: a wave's threads read
// their own rows without bank conflicts); each thread finds its bytes' run starts and ends from a 64-bit mask of run breaks and
// two workgroup scans (the latest break before it, the first behind it), counts its tokens' symbols into an LDS histogram, the
// symbols are ranked in parallel, ONE lane builds the code and then the code-length code (deflate_core.h), then bit lengths, a
// workgroup scan, and the bits go into zeroed LDS words - plain stores for the words a thread owns alone, OR-atomics for its first
// and last word, which neighbours share (OR is order-independent: the bytes never depend on scheduling) - and from there to the
// chunk's slot of the workspace.
// (b) crc: per chunk, the CRC-32 of its input bytes: each thread's 64 bytes by table, shifted to the chunk's end by a GF(2)
// multiplication and XOR-ed together. (c) offsets + pack: an exclusive prefix of the chunk lengths by one workgroup, then a
// workgroup per chunk copies its slot to its place in the payload; the total goes to `length`.
#include "deflate_core.h"
#include "vda_common.h"

namespace {

constexpr int DF_T = 256;                        // threads of a workgroup
constexpr int DF_SEG = DFL_CHUNK / DF_T;         // input bytes of a thread: 64, the width of its break mask
constexpr int DF_ROW = DF_SEG / 4 + 1;           // words of a thread's row in LDS: 16 of data, one of padding
constexpr int DF_SLOT = 16400;                   // bytes of a chunk's slot in the workspace: 5 + 16384 rounded up to 16
constexpr int DF_OUT_WORDS = DF_SLOT / 4;
static_assert(DF_SEG == 64 && sizeof(DflScratch) <= DF_SLOT, "a break mask is one 64-bit word; the builder's scratch lies in the output words");

// exclusive sum of v over the workgroup's threads in thread order; `total` = the sum. `sh`: DF_T / 64 words of LDS.
__device__ __forceinline__ uint32_t df_scan(uint32_t v, uint32_t& total, uint32_t* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < DF_T / 64; ++i) {
        const uint32_t s = sh[i];
        before += i < wave ? s : 0u;
        all += s;
    }
    total = all;
    __syncthreads();                             // sh may be written again
    return before + incl - v;
}

// the largest v of the threads BEFORE this one (-1 when there is none or all are -1)
__device__ __forceinline__ int df_max_before(int v, int* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl = max(incl, up);
    }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    int before = -1;
#pragma unroll
    for (int i = 0; i < DF_T / 64; ++i) before = i < wave ? max(before, sh[i]) : before;
    const int prev = __shfl_up(incl, 1, 64);
    __syncthreads();
    return lane ? max(before, prev) : before;
}

// the smallest v of the threads BEHIND this one (`none` when there is none)
__device__ __forceinline__ int df_min_behind(int v, int none, int* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int dn = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl = min(incl, dn);
    }
    if (lane == 0) sh[wave] = incl;
    __syncthreads();
    int behind = none;
#pragma unroll
    for (int i = 0; i < DF_T / 64; ++i) behind = i > wave ? min(behind, sh[i]) : behind;
    const int next = __shfl_down(incl, 1, 64);
    __syncthreads();
    return lane < 63 ? min(behind, next) : behind;
}

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

__device__ __forceinline__ uint32_t df_byte(const uint32_t* rows, int i) {
    return (rows[(i >> 6) * DF_ROW + ((i & 63) >> 2)] >> (8 * (i & 3))) & 0xffu;
}

// `n` bits (at most 32) of `bits` at bit `pos` of zeroed words, least significant bit first, by OR-atomics: for the few tokens that
// no thread's run of tokens holds (the header, end-of-block, the flush)
__device__ __forceinline__ void df_put_shared(uint32_t* words, uint32_t pos, uint32_t bits, int n) {
    const unsigned long long v = (unsigned long long)bits << (pos & 31);
    atomicOr(words + (pos >> 5), (uint32_t)v);
    if ((pos & 31) + n > 32) atomicOr(words + (pos >> 5) + 1, (uint32_t)(v >> 32));
}

struct DfRuns {
    unsigned long long brk;      // bit j: byte j of this thread's 64 starts a run (or lies behind the chunk's end)
    int valid;                   // bytes of the chunk in this thread's row: 0..64
    int start_before;            // the latest run start before this thread's bytes
    int end_behind;              // the first run start (or the chunk's end) behind them
};

// This thread's tokens in stream order: fn(symbol, extra bit count, extra value, is match).
template <typename F>
__device__ __forceinline__ void df_tokens(const uint32_t* rows, const DfRuns& r, F&& fn) {
    const int t0 = threadIdx.x * DF_SEG;
    for (int j = 0; j < r.valid; ++j) {
        const unsigned long long low = r.brk & ((2ull << j) - 1ull), high = j < 63 ? r.brk >> (j + 1) : 0ull;
        const int start = low ? t0 + 63 - __clzll((long long)low) : r.start_before;
        const int end = high ? t0 + j + 1 + (__ffsll((long long)high) - 1) : r.end_behind;
        const int o = t0 + j - start;
        if (o == 0) {
            fn(df_byte(rows, t0 + j), 0, 0u, false);
            continue;
        }
        const int k = o - 1, seg = k / 258, seglen = min(258, end - start - 1 - seg * 258);
        if (seglen < 3) {
            fn(df_byte(rows, t0 + j), 0, 0u, false);
        } else if (k - seg * 258 == 0) {
            uint32_t extra;
            const uint32_t s = dfl_length_symbol(seglen, &extra);
            fn(s & 0xffffu, (int)(s >> 16), extra, true);
        }
    }
}

struct DfShared {
    uint32_t rows[DF_T * DF_ROW];
    uint32_t out[DF_OUT_WORDS];                  // the builder's scratch first, then the chunk's bits
    uint32_t count[DFL_NSYM + 2];
    uint16_t code[DFL_NSYM + 2];
    uint8_t len[DFL_NSYM + 2];
    uint32_t cl_count[DFL_NCL + 1];               // how often each code length 0..15 occurs in the header
    uint16_t cl_code[DFL_NCL + 1];
    uint8_t cl_len[DFL_NCL + 1];
    uint32_t sh[DF_T / 64];
    int n_used, hlit, has_match, hclen;
};

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
    for (int i = t; i < DFL_NSYM + 2; i += DF_T) S.count[i] = 0;
    if (t < DFL_NCL + 1) S.cl_count[t] = 0;
    df_stage(in + at, m, S.rows);
    __syncthreads();

    // runs: the break mask of this thread's bytes, then the latest break before and the first break behind them
    DfRuns r;
    r.valid = min(DF_SEG, max(0, m - t * DF_SEG));
    r.brk = 0;
    {
        uint32_t prev = t > 0 && r.valid > 0 ? df_byte(S.rows, t * DF_SEG - 1) : 0x100u;      // byte 0 of the chunk always starts a run
        for (int j = 0; j < DF_SEG; ++j) {
            const uint32_t b = j < r.valid ? df_byte(S.rows, t * DF_SEG + j) : 0x100u;
            if (b != prev || j >= r.valid) r.brk |= 1ull << j;
            prev = b;
        }
    }
    const unsigned long long in_chunk = r.valid >= 64 ? ~0ull : (1ull << r.valid) - 1ull;
    const unsigned long long own = r.brk & in_chunk;
    r.start_before = df_max_before(own ? t * DF_SEG + 63 - __clzll((long long)own) : -1, reinterpret_cast<int*>(S.sh));
    // (a thread whose 64 bytes all continue one run has no break to offer; a break behind the chunk's end stands for the end itself)
    r.end_behind = df_min_behind(r.brk ? min(m, t * DF_SEG + __ffsll((long long)r.brk) - 1) : m, m, reinterpret_cast<int*>(S.sh));
    // pass 1: the histogram
    df_tokens(S.rows, r, [&](uint32_t sym, int, uint32_t, bool) { atomicAdd(&S.count[sym], 1u); });
    if (t == 0) S.count[DFL_EOB] = 1;
    __syncthreads();

    // the used symbols ascending by (count, symbol): every symbol finds its rank
    DflScratch* sc = reinterpret_cast<DflScratch*>(S.out);
    for (int s = t; s < DFL_NSYM; s += DF_T) {
        const uint32_t c = S.count[s];
        int rank = 0, used = 0;
        for (int q = 0; q < DFL_NSYM; ++q) {
            const uint32_t cq = S.count[q];
            used += cq != 0;
            rank += cq != 0 && (cq < c || (cq == c && q < s));
        }
        if (c) sc->order[rank] = (uint16_t)s;
        if (s == 0) S.n_used = used;
    }
    __syncthreads();
    if (t == 0) {
        dfl_lengths_sorted(S.count, DFL_NSYM, S.n_used, DFL_MAX_BITS, S.len, sc);
        dfl_codes(S.len, DFL_NSYM, S.code, sc);
        int hlit = 257, has_match = 0;
        for (int s = 257; s < DFL_NSYM; ++s)
            if (S.count[s]) hlit = s + 1, has_match = 1;
        S.hlit = hlit, S.has_match = has_match;
    }
    __syncthreads();
    const int hlit = S.hlit, has_match = S.has_match;
    // the code-length code: a Huffman code of at most 7 bits for the hlit + 1 lengths the header lists (the distance code's last)
    atomicAdd(&S.cl_count[S.len[t]], 1u);
    if (256 + t < hlit) atomicAdd(&S.cl_count[S.len[256 + t]], 1u);
    if (t == 0) atomicAdd(&S.cl_count[has_match], 1u);
    __syncthreads();
    if (t == 0) {
        dfl_build_lengths(S.cl_count, DFL_NCL, DFL_CL_MAX_BITS, S.cl_len, sc);
        dfl_codes(S.cl_len, DFL_NCL, S.cl_code, sc);
        int hclen = 4;
        for (int k = 4; k < DFL_NCL; ++k)
            if (S.cl_len[dfl_cl_order(k)]) hclen = k + 1;
        S.hclen = hclen;
    }
    __syncthreads();
    for (int i = t; i < DF_OUT_WORDS; i += DF_T) S.out[i] = 0;                // the scratch is done with
    const int hclen = S.hclen;

    // bit offsets: the header's code lengths, then this thread's tokens
    uint32_t low_bits, high_bits, data_bits;
    const uint32_t cl0 = df_scan(S.cl_len[S.len[t]], low_bits, S.sh);
    const uint32_t cl1 = df_scan(256 + t < hlit ? S.cl_len[S.len[256 + t]] : 0, high_bits, S.sh);
    uint32_t mine = 0;
    df_tokens(S.rows, r, [&](uint32_t sym, int nextra, uint32_t, bool match) { mine += S.len[sym] + nextra + (match ? 1 : 0); });
    const uint32_t lengths_at = DFL_HEADER_BITS + 3 * hclen;
    const uint32_t first_data = lengths_at + low_bits + high_bits + S.cl_len[has_match];
    const uint32_t pos = first_data + df_scan(mine, data_bits, S.sh);
    const uint32_t eob_at = first_data + data_bits, total = eob_at + S.len[DFL_EOB];
    const uint32_t coded = last ? (total + 7) >> 3 : ((total + 3 + 7) >> 3) + 4;

    if (coded >= (uint32_t)m + DFL_STORED_OVERHEAD) {                          // one stored block
        if (t == 0) {
            slot[0] = last ? 1 : 0, slot[1] = (uint8_t)(m & 0xff), slot[2] = (uint8_t)(m >> 8);
            slot[3] = (uint8_t)(~m & 0xff), slot[4] = (uint8_t)((~m >> 8) & 0xff);
            chunk_len[chunk] = m + DFL_STORED_OVERHEAD;
        }
        for (int i = t; i < m; i += DF_T) slot[DFL_STORED_OVERHEAD + i] = (uint8_t)df_byte(S.rows, i);
        return;
    }
    // coded < m + 5 <= DF_SLOT - 11: every bit below lands inside S.out
    if (t == 0) {
        // BFINAL, BTYPE = 2, HLIT - 257, HDIST - 1 = 0, HCLEN - 4
        df_put_shared(S.out, 0, (last ? 1u : 0u) | (2u << 1) | ((uint32_t)(hlit - 257) << 3) | (0u << 8) | ((uint32_t)(hclen - 4) << 13), DFL_HEADER_BITS);
        for (int k = 0; k < hclen; ++k) df_put_shared(S.out, DFL_HEADER_BITS + 3 * k, S.cl_len[dfl_cl_order(k)], 3);
        df_put_shared(S.out, lengths_at + low_bits + high_bits, S.cl_code[has_match], S.cl_len[has_match]);
        df_put_shared(S.out, eob_at, S.code[DFL_EOB], S.len[DFL_EOB]);
        if (!last) df_put_shared(S.out, 8 * (coded - 2), 0xffffu, 16);         // 000, zeros to the byte's end, 00 00 FF FF
    }
    df_put_shared(S.out, lengths_at + cl0, S.cl_code[S.len[t]], S.cl_len[S.len[t]]);
    if (256 + t < hlit) df_put_shared(S.out, lengths_at + low_bits + cl1, S.cl_code[S.len[256 + t]], S.cl_len[S.len[256 + t]]);
    {
        // this thread's tokens from bit `pos` on: the first word it touches and the last may be shared, the words between are its own
        uint32_t widx = pos >> 5;
        unsigned long long acc = 0;
        int nacc = pos & 31;
        bool first = true;
        df_tokens(S.rows, r, [&](uint32_t sym, int nextra, uint32_t extra, bool match) {
            const int ln = S.len[sym];
            acc |= (unsigned long long)(S.code[sym] | (extra << ln)) << nacc;  // at most 15 + 5 (+ the distance code '0') bits: acc holds 31 + 21
            nacc += ln + nextra + (match ? 1 : 0);
            if (nacc >= 32) {
                if (first) atomicOr(S.out + widx, (uint32_t)acc);
                else S.out[widx] = (uint32_t)acc;
                first = false;
                acc >>= 32, nacc -= 32, ++widx;
            }
        });
        if (nacc > 0 && acc) atomicOr(S.out + widx, (uint32_t)acc);
    }
    __syncthreads();
    uint32_t* dst = reinterpret_cast<uint32_t*>(slot);
    for (uint32_t i = t; i < (coded + 3) >> 2; i += DF_T) dst[i] = S.out[i];
    if (t == 0) chunk_len[chunk] = (int)coded;
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
