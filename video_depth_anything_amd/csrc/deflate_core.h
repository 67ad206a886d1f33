// The code builder of the deflate encoder (video_depth_anything_amd/deflate.py: `code_lengths` and `canonical_codes` are the same
// steps in Python and the contract). One text for the device kernel (csrc/deflate.hip: one lane per chunk runs it
// over at most 286 symbols) and for the host program that runs it under the address and undefined-behaviour sanitizers
// (tests/deflate_core_main.cpp) - so this header includes nothing of HIP and allocates nothing.
//
// Integer arithmetic only, ties broken by (count, symbol): the lengths are a function of the counts alone.
//   sort      the symbols with a non-zero count, ascending by (count, symbol)
//   merge     the two-queue Huffman construction over the sorted leaves; of a leaf and an internal node of equal weight the
//             leaf goes first; the counts' sum must stay below 2^32
//   limit     depths above max_bits (15; 7 for the code-length code) are cut to it; while the Kraft sum (in units of 2^-max_bits)
//             exceeds 1: one code leaves the longest populated length below max_bits for the next length, and one code of max_bits
//             joins it there (each round lowers the sum by one unit)
//   deal      lengths go out in sorted order, the rarest symbols the longest
// Bounds: every array is indexed by a symbol < nsym <= DFL_NSYM or a leaf / node index < n <= nsym.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFL_HD __host__ __device__ inline
#else
#define DFL_HD inline
#endif

enum {
    DFL_CHUNK = 16384,       // input bytes of one independent chunk
    DFL_NSYM = 286,          // literal/length symbols
    DFL_EOB = 256,
    DFL_MAX_BITS = 15,
    DFL_STORED_OVERHEAD = 5, // a stored block: a byte of header bits, LEN, NLEN
    DFL_NCL = 19,            // symbols of the code-length code; this encoder writes 0..15 only, never the repeat symbols
    DFL_CL_MAX_BITS = 7,
    DFL_HEADER_BITS = 17,    // BFINAL, BTYPE, HLIT, HDIST, HCLEN; then 3 bits per listed length of the code-length code
};

struct DflScratch {
    uint32_t weight[DFL_NSYM];       // internal nodes' weights, in the order they are made
    uint16_t order[DFL_NSYM];        // used symbols, ascending by (count, symbol)
    uint16_t leaf_parent[DFL_NSYM];  // per sorted leaf: the internal node above it
    uint16_t node_parent[DFL_NSYM];  // per internal node: the one above it
    uint16_t node_depth[DFL_NSYM];
    // codes per length, next code per length: here and not on the stack, where the device would index them through scratch memory
    uint32_t blc[DFL_MAX_BITS + 2], next[DFL_MAX_BITS + 2];
};

// Used symbols ascending by (count, symbol) into order[]; returns how many. (The device sorts by ranks in parallel instead and
// gets the same order: the key is unique.)
DFL_HD int dfl_sort(const uint32_t* count, int nsym, uint16_t* order) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        if (count[s] == 0) continue;
        int i = n++;
        for (; i > 0 && count[order[i - 1]] > count[s]; --i) order[i] = order[i - 1];      // equal counts stay in symbol order
        order[i] = (uint16_t)s;
    }
    return n;
}

// len[0 .. nsym) from sc->order[0 .. n), the sorted used symbols.
DFL_HD void dfl_lengths_sorted(const uint32_t* count, int nsym, int n, int max_bits, uint8_t* len, DflScratch* sc) {
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    if (n <= 0) return;
    if (n == 1) {
        len[sc->order[0]] = 1;
        return;
    }
    int li = 0, ii = 0;              // next unmerged leaf, next unmerged internal node
    for (int j = 0; j < n - 1; ++j) {
        uint32_t tot = 0;
        for (int k = 0; k < 2; ++k) {
            if (li < n && (ii >= j || count[sc->order[li]] <= sc->weight[ii])) {
                sc->leaf_parent[li] = (uint16_t)j;
                tot += count[sc->order[li]];
                ++li;
            } else {
                sc->node_parent[ii] = (uint16_t)j;
                tot += sc->weight[ii];
                ++ii;
            }
        }
        sc->weight[j] = tot;
    }
    sc->node_depth[n - 2] = 0;
    for (int j = n - 3; j >= 0; --j) sc->node_depth[j] = (uint16_t)(sc->node_depth[sc->node_parent[j]] + 1);
    uint32_t* blc = sc->blc;
    if (max_bits > DFL_MAX_BITS) max_bits = DFL_MAX_BITS;
    for (int b = 0; b <= DFL_MAX_BITS; ++b) blc[b] = 0;
    for (int i = 0; i < n; ++i) {
        const int d = sc->node_depth[sc->leaf_parent[i]] + 1;
        ++blc[d < max_bits ? d : max_bits];
    }
    uint32_t total = 0;
    for (int b = 1; b <= max_bits; ++b) total += blc[b] << (max_bits - b);
    while (total > (1u << max_bits)) {
        --blc[max_bits];
        for (int b = max_bits - 1; b > 0; --b) {
            if (blc[b]) {
                --blc[b];
                blc[b + 1] += 2;
                break;
            }
        }
        --total;
    }
    int i = 0;
    for (int b = max_bits; b > 0; --b)
        for (uint32_t k = 0; k < blc[b] && i < n; ++k) len[sc->order[i++]] = (uint8_t)b;
}

DFL_HD void dfl_build_lengths(const uint32_t* count, int nsym, int max_bits, uint8_t* len, DflScratch* sc) {
    dfl_lengths_sorted(count, nsym, dfl_sort(count, nsym, sc->order), max_bits, len, sc);
}

DFL_HD uint32_t dfl_reverse(uint32_t code, int n) {
#if defined(__clang__)
    return n > 0 ? __builtin_bitreverse32(code) >> (32 - n) : 0u;       // one instruction on the device
#endif
    uint32_t r = 0;
    for (int i = 0; i < n; ++i, code >>= 1) r = (r << 1) | (code & 1u);
    return r;
}

// The canonical codes of RFC 1951 3.2.2, each bit-reversed: the stream fills bytes from the least significant bit, Huffman codes
// go in most significant bit first.
DFL_HD void dfl_codes(const uint8_t* len, int nsym, uint16_t* code, DflScratch* sc) {
    uint32_t *blc = sc->blc, *next = sc->next;
    for (int b = 0; b < DFL_MAX_BITS + 2; ++b) blc[b] = 0;
    for (int s = 0; s < nsym; ++s) ++blc[len[s] <= DFL_MAX_BITS ? len[s] : 0];
    blc[0] = 0;
    uint32_t c = 0;
    next[0] = 0;
    for (int b = 1; b <= DFL_MAX_BITS; ++b) {
        c = (c + blc[b - 1]) << 1;
        next[b] = c;
    }
    for (int s = 0; s < nsym; ++s) {
        const int b = len[s] <= DFL_MAX_BITS ? len[s] : 0;
        code[s] = b ? (uint16_t)dfl_reverse(next[b]++, b) : (uint16_t)0;
    }
}

// A match length 3..258 as RFC 1951 3.2.5 codes it, in closed form: symbol | extra bit count << 16, and the extra bits' value.
// Lengths 3..10 have a code each; from 11 on four codes share each power of two of (length - 3); 258 has code 285 to itself.
DFL_HD uint32_t dfl_length_symbol(int length, uint32_t* extra) {
    const uint32_t x = (uint32_t)(length - 3);
    *extra = 0;
    if (length == 258) return 285;
    if (x < 8) return 257 + x;
    int e = 1;
    while ((x >> (e + 2)) > 1) ++e;  // e = floor(log2 x) - 2, 1..5
    *extra = x & ((1u << e) - 1u);
    return (257 + 4 * e + (x >> e)) | ((uint32_t)e << 16);
}

// Where the header lists the length of code-length symbol s: position k of the order 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13,
// 2, 14, 1, 15 (RFC 1951 3.2.7).
DFL_HD int dfl_cl_order(int k) {
    const uint8_t order[DFL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[k < DFL_NCL ? (k < 0 ? 0 : k) : DFL_NCL - 1];
}
