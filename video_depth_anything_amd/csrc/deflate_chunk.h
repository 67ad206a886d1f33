// One chunk of the deflate encoder, from "the chunk's bytes lie in the workgroup's LDS rows" to "its bytes lie in its slot of the
// workspace and its length is known": the steps csrc/deflate.hip (a byte buffer, .npz) and csrc/exr.hip (the filtered bytes of an
// OpenEXR ZIP block, gathered from float32 depth) share. The contract is deflate.encode_chunk (video_depth_anything_amd/deflate.py),
// the code builder is deflate_core.h; what the steps are is told at the top of deflate.hip.
//
// A caller (a workgroup of DF_T threads) runs df_clear(S), stages its m bytes (1..DFL_CHUNK) into S.rows - byte i lies in word
// (i >> 6) * DF_ROW + ((i & 63) >> 2), so that a thread's 64 bytes are its own row and a wave's threads read theirs without bank
// conflicts -, __syncthreads(), then df_encode_staged. DfShared is all the LDS the encoder needs (about 34 KB: four workgroups a CU).
#pragma once
#include "deflate_core.h"
#include "vda_common.h"

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

// The histograms to zero: before the chunk is staged, so that the barrier behind the staging covers both.
__device__ __forceinline__ void df_clear(DfShared& S) {
    const int t = threadIdx.x;
    for (int i = t; i < DFL_NSYM + 2; i += DF_T) S.count[i] = 0;
    if (t < DFL_NCL + 1) S.cl_count[t] = 0;
}

// The chunk of m bytes (1..DFL_CHUNK) in S.rows -> `slot` (DF_SLOT bytes, word aligned) and *chunk_len. `last`: the chunk's block
// carries BFINAL and no sync flush follows it. Every thread of the workgroup calls it, behind a barrier after df_clear and the staging.
__device__ __forceinline__ void df_encode_staged(DfShared& S, int m, bool last, uint8_t* __restrict__ slot, int* __restrict__ chunk_len) {
    const int t = threadIdx.x;
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
            *chunk_len = m + DFL_STORED_OVERHEAD;
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
    if (t == 0) *chunk_len = (int)coded;
}
