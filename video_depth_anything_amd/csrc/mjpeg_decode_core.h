// The entropy decoder of one restart interval of a baseline JPEG scan (video_depth_anything_amd/mjpeg.py: `_decode_interval` is
// the same loop in Python and the contract). One text for the device kernel (csrc/mjpeg_decode.hip, a lane per
// interval) and for the host program that runs it under the address and undefined-behaviour sanitizers over a corpus of corrupt
// streams (tests/mjpeg_decode_core_main.cpp) - so this header includes nothing of HIP and allocates nothing.
//
// Bounds, none of which trusts the stream or the tables:
//   reads    `data[p]` only for 0 <= p < len; the byte behind an FF is skipped (it is the stuffed 00) whatever it is;
//   tables   every index into a table is masked to the table's size (a symbol is 8 bits, a lookahead index 8 bits, a code length
//            1..16, a value offset & 255, a zig-zag position & 63);
//   writes   a block's 64 coefficients at `coef + block * 64`, block < g.frame_blocks by construction of the MCU walk, which stops
//            at g.mw * g.mh whatever `first_mcu` and `mcu_count` say.
// A lane that meets an error returns its code at once; what it wrote until then stays (the twin leaves the same).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MJD_HD __host__ __device__ __forceinline__
#else
#define MJD_HD inline
#endif

enum {
    MJD_OK = 0,
    MJD_BAD_CODE = 1,        // a code that is not in the Huffman table
    MJD_BAD_SIZE = 2,        // DC category > 11 or AC size > 10
    MJD_RUN_PAST_63 = 3,     // a run that puts a coefficient behind position 63
    MJD_INTERVAL_SHORT = 4,  // the interval's bits end before its MCUs are decoded
    MJD_INTERVAL_COUNT = 5,  // (host) the scan has another number of intervals than DRI and the frame size give
    MJD_DC_RANGE = 6,        // a DC predictor outside int16
    MJD_NO_EOI = 7,          // (host) the scan is not ended by EOI
};

// One Huffman table: `look[b]` = length << 8 | symbol of the code that starts the 8 bits b (0: no code of up to 8 bits does);
// for lengths 9..16 the canonical search of T.81 F.2.2.3: maxcode[l] = the largest code of length l (-1: none),
// valoff[l] = index of the first value of length l - the smallest code of length l.
struct MjdHuff {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t vals[256];
};

// What a call uploads once: per component its DC table and its AC table, then the zig-zag order (natural position of scan
// position k) and the interval table's geometry.
struct MjdTables {
    MjdHuff dc[3], ac[3];
    uint8_t zigzag[64];
};

struct MjdGeom {
    int components;          // 1 or 3
    int hs, vs;              // blocks of component 0 per MCU, across and down (1x1, 2x1, 2x2); the others have one
    int mw, mh;              // MCUs across and down
    int comp_off[3];         // first block of each component's grid within a frame's coefficients
    int comp_bw[3];          // blocks across in each component's grid
    int frame_blocks;        // blocks of one frame, all components
};

// The bit reader: a 32-bit window refilled a byte at a time; unstuffing happens as the bytes enter it. (Measured on the MI355X: a
// 64-bit window refilled four bytes at a time, with the next four already in flight, was no faster with an interval per MCU row and
// slower without restart markers: profiles/mjpeg/decode_entropy_variants.txt.)
struct MjdBits {
    const uint8_t* data;
    int len, p;
    uint32_t acc;            // the low `cnt` bits are the stream's next bits
    int cnt;
};

MJD_HD void mjd_refill(MjdBits& b) {
    while (b.cnt <= 24 && b.p < b.len) {
        const uint32_t v = b.data[b.p];
        b.p += v == 0xffu ? 2 : 1;                 // FF 00 is the byte FF; the host cut the scan at every other FF xx
        b.acc = (b.acc << 8) | v;
        b.cnt += 8;
    }
}

// the next n <= 16 bits, 1-bits where the interval has ended (an encoder pads its last byte with them)
MJD_HD uint32_t mjd_peek(const MjdBits& b, int n) {
    const uint32_t mask = (1u << n) - 1u;
    if (b.cnt >= n) return (b.acc >> (b.cnt - n)) & mask;
    return ((b.acc << (n - b.cnt)) | ((1u << (n - b.cnt)) - 1u)) & mask;
}

// One symbol; < 0 = -(error code).
MJD_HD int mjd_symbol(MjdBits& b, const MjdHuff& t) {
    mjd_refill(b);
    const uint32_t code = mjd_peek(b, 16);
    const uint32_t e = t.look[code >> 8];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (e == 0) {
        len = 9;
        for (; len <= 16; ++len) {
            const int c = (int)(code >> (16 - len));
            if (c <= t.maxcode[len]) {
                sym = t.vals[(t.valoff[len] + c) & 255];
                break;
            }
        }
        if (len > 16) return b.cnt < 16 ? -MJD_INTERVAL_SHORT : -MJD_BAD_CODE;     // the padding's 1-bits are no code: the interval has ended
    }
    if (len > b.cnt) return -MJD_INTERVAL_SHORT;   // also what a table with a length outside 1..16 ends in
    b.cnt -= len;
    return sym;
}

// `size` <= 16 amplitude bits, sign-extended as EXTEND of T.81 F.2.2.1; ok = false when the interval ends inside them.
MJD_HD int mjd_receive_extend(MjdBits& b, int size, bool& ok) {
    if (size == 0) return 0;
    mjd_refill(b);
    if (size > b.cnt) {
        ok = false;
        return 0;
    }
    const int v = (int)mjd_peek(b, size);
    b.cnt -= size;
    return v < (1 << (size - 1)) ? v - (1 << size) + 1 : v;
}

// MCUs [first_mcu, first_mcu + mcu_count) of one frame from the `len` bytes at `data` (len <= 2^31 - 16: the offset is an int and runs
// up to 1 past it); `coef` is the frame's zeroed workspace.
MJD_HD int mjd_decode_interval(const uint8_t* data, int len, int first_mcu, int mcu_count, const MjdGeom& g, const MjdTables& t,
                               int16_t* coef) {
    MjdBits b = {data, len, 0, 0u, 0};
    int pred[3] = {0, 0, 0};
    const int total = g.mw * g.mh;
    if (first_mcu < 0 || mcu_count < 0) return MJD_OK;
    for (int m = 0; m < mcu_count; ++m) {
        const int mcu = first_mcu + m;
        if (mcu >= total) break;
        const int my = mcu / g.mw, mx = mcu - my * g.mw;
        for (int c = 0; c < g.components; ++c) {
            const int hc = c == 0 ? g.hs : 1, vc = c == 0 ? g.vs : 1;
            for (int by = 0; by < vc; ++by) {
                for (int bx = 0; bx < hc; ++bx) {
                    const int block = g.comp_off[c] + (my * vc + by) * g.comp_bw[c] + mx * hc + bx;
                    if (block < 0 || block >= g.frame_blocks) return MJD_OK;       // a geometry that contradicts itself: nothing is written
                    int16_t* out = coef + (long long)block * 64;
                    int s = mjd_symbol(b, t.dc[c]);
                    if (s < 0) return -s;
                    if (s > 11) return MJD_BAD_SIZE;
                    bool ok = true;
                    pred[c] += mjd_receive_extend(b, s, ok);
                    if (!ok) return MJD_INTERVAL_SHORT;
                    if (pred[c] < -32768 || pred[c] > 32767) return MJD_DC_RANGE;
                    out[0] = (int16_t)pred[c];
                    int k = 1;
                    while (k < 64) {
                        const int rs = mjd_symbol(b, t.ac[c]);
                        if (rs < 0) return -rs;
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;                                    // EOB
                            k += 16;                                               // ZRL
                            continue;
                        }
                        if (s > 10) return MJD_BAD_SIZE;
                        k += r;
                        if (k > 63) return MJD_RUN_PAST_63;
                        const int v = mjd_receive_extend(b, s, ok);
                        if (!ok) return MJD_INTERVAL_SHORT;
                        out[t.zigzag[k] & 63] = (int16_t)v;
                        ++k;
                    }
                }
            }
        }
    }
    return MJD_OK;
}
