// OpenEXR scanline files with ZIP compression, made on the device from float32 depth, for run.py --save_exr
// (video_depth_anything_amd/exr.py: encode_exr_numpy is the contract, byte for byte). One channel Z of FLOAT pixels.
//
//   blocks    a frame is cut into nb = ceil(h / 16) blocks of 16 scanlines (the last of h - 16 (nb - 1)); a block's raw bytes are
//             its rows of w float32 back to back, L = 4 w rows bytes
//   filter    OpenEXR's: the even bytes, then the odd ones (t), then the difference to the predecessor plus 128 (f), f[0] = t[0]
//   chunks    f is cut into k = ceil(L / 16384) balanced chunks of q = 64 ceil(L / (64 k)) bytes (the last shorter), a workgroup
//             each, coded by deflate_chunk.h: BFINAL on the block's last chunk, a sync flush behind the others
//   stream    78 01, the chunks, the Adler-32 of f big-endian; a block whose stream is not strictly shorter than L is written raw
//
// Launches. (a) encode: grid over (frame, block, chunk); a workgroup gathers its chunk of f straight from the depth tensor into the
// encoder's LDS rows (words loaded, bytes picked at stride 2, one byte looked back for the difference: no filtered copy in memory),
// leaves its Adler partial sums (sum f, sum (L - i) f) as 64-bit integers and the coded chunk in its slot. (b) blocks: a thread per
// block sums its chunks' lengths and partials and decides compressed or raw. (c) offsets: one workgroup's exclusive prefix of the
// block sizes; the frames' payload offsets fall out of it. (d) pack: grid as in (a); a workgroup copies its chunk (or, of a raw
// block, its share of the rows) to its place, the first of a block also writes the offset table's entry, y, dataSize and 78 01,
// the last the Adler-32. Integer arithmetic and order-independent OR-atomics in LDS only: the bytes never depend on scheduling.
#include "deflate_chunk.h"

namespace {

constexpr int EXR_LINES = 16;                    // scanlines of a ZIP block
constexpr int EXR_MAX_SIDE = 65535;              // L <= 64 * 65535 < 2^22: at most 256 chunks a block, every byte count an int
constexpr uint32_t EXR_ADLER = 65521;

struct ExrGeo {
    int frames, h, w, nb;
    int kfull;                                   // chunks of a block of 16 rows (of the only block when nb = 1)
    int cpf;                                     // chunks of a frame
};

struct ExrChunk {
    int frame, b, c;                             // frame, block of the frame, chunk of the block
    int L, k, q;                                 // the block's bytes, its chunks, bytes of a chunk but the last
    int at, m;                                   // this chunk: filtered bytes [at, at + m)
};

__host__ __device__ inline int exr_block_bytes(const ExrGeo& g, int b) {
    const int rows = g.h - EXR_LINES * b;
    return 4 * g.w * (rows < EXR_LINES ? rows : EXR_LINES);
}
__host__ __device__ inline int exr_chunks_of(int L) { return (L + DFL_CHUNK - 1) / DFL_CHUNK; }

__device__ __forceinline__ ExrChunk exr_chunk(const ExrGeo& g, long long id) {
    ExrChunk x;
    x.frame = (int)(id / g.cpf);
    const int in_frame = (int)(id - (long long)x.frame * g.cpf);
    x.b = min(in_frame / g.kfull, g.nb - 1);
    x.c = in_frame - x.b * g.kfull;
    x.L = exr_block_bytes(g, x.b);
    x.k = exr_chunks_of(x.L);
    x.q = 64 * ((x.L + 64 * x.k - 1) / (64 * x.k));
    x.at = x.c * x.q;
    x.m = min(x.q, x.L - x.at);                  // > 0: (k - 1) q < L for k <= 256
    return x;
}

// byte i of t: the block's even bytes, then its odd ones. `raw`: the block's rows as words.
__device__ __forceinline__ uint32_t exr_t(const uint32_t* __restrict__ raw, int half, int i) {
    const int j = i < half ? 2 * i : 2 * (i - half) + 1;
    return (raw[j >> 2] >> (8 * (j & 3))) & 0xffu;
}

__device__ __forceinline__ unsigned long long exr_sum(unsigned long long v, unsigned long long* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    unsigned long long all = 0;
#pragma unroll
    for (int i = 0; i < DF_T / 64; ++i) all += sh[i];
    return all;
}

// --------------------------------------------------------------------------------------------------------------------- (a) encode
__global__ void __launch_bounds__(DF_T) exr_encode_kernel(const float* __restrict__ depth, long long frame_stride, ExrGeo g, uint8_t* __restrict__ slots,
                                                          int* __restrict__ chunk_len, unsigned long long* __restrict__ partial) {
    __shared__ DfShared S;
    __shared__ unsigned long long red[2][DF_T / 64];
    const int t = threadIdx.x;
    const long long id = blockIdx.x;
    const ExrChunk x = exr_chunk(g, id);
    const int half = x.L >> 1;                   // L is a multiple of 4
    const uint32_t* raw = reinterpret_cast<const uint32_t*>(depth + (long long)x.frame * frame_stride + (long long)EXR_LINES * x.b * g.w);
    df_clear(S);
    // at, m and L are multiples of 4: a word of the rows is four bytes of f, all inside the block
    for (int d = t; 4 * d < x.m; d += DF_T) {
        const int i0 = x.at + 4 * d;
        uint32_t prev = i0 > 0 ? exr_t(raw, half, i0 - 1) : 128u;             // f[0] = t[0] = (t[0] - 128 + 128) & 255
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t cur = exr_t(raw, half, i0 + j);
            v |= ((cur - prev + 128u) & 0xffu) << (8 * j);
            prev = cur;
        }
        S.rows[(d >> 4) * DF_ROW + (d & 15)] = v;
    }
    __syncthreads();
    {
        // Adler-32's two sums over this chunk: s1 = sum f, s2 = sum (L - i) f, i the byte's place in the block
        const int valid = min(DF_SEG, max(0, x.m - t * DF_SEG));
        unsigned long long s1 = 0, s2 = 0;
        for (int j = 0; j < valid; ++j) {
            const unsigned long long f = df_byte(S.rows, t * DF_SEG + j);
            s1 += f;
            s2 += (unsigned long long)(x.L - (x.at + t * DF_SEG + j)) * f;
        }
        s1 = exr_sum(s1, red[0]);
        s2 = exr_sum(s2, red[1]);
        if (t == 0) partial[2 * id] = s1, partial[2 * id + 1] = s2;
    }
    df_encode_staged(S, x.m, x.c == x.k - 1, slots + id * DF_SLOT, chunk_len + id);
}

// --------------------------------------------------------------------------------------------------------------------- (b) blocks
// a thread per (frame, block): chunk_off = where each chunk starts in the block's deflate stream, data_size = the block's dataSize
// (its zlib stream's length when that is strictly below L, else L), adler = the Adler-32 of f
__global__ void __launch_bounds__(DF_T) exr_blocks_kernel(ExrGeo g, const int* __restrict__ chunk_len, const unsigned long long* __restrict__ partial,
                                                          int* __restrict__ chunk_off, int* __restrict__ data_size, uint32_t* __restrict__ adler) {
    const long long fb = (long long)blockIdx.x * DF_T + threadIdx.x;
    if (fb >= (long long)g.frames * g.nb) return;
    const int frame = (int)(fb / g.nb), b = (int)(fb - (long long)frame * g.nb);
    const int L = exr_block_bytes(g, b), k = exr_chunks_of(L);
    const long long first = (long long)frame * g.cpf + (long long)b * g.kfull;
    int sum = 0;
    unsigned long long s1 = 0, s2 = 0;
    for (int c = 0; c < k; ++c) {
        chunk_off[first + c] = sum;
        sum += chunk_len[first + c];             // at most 256 * 16389
        s1 += partial[2 * (first + c)], s2 += partial[2 * (first + c) + 1];
    }
    const int z = 2 + sum + 4;
    data_size[fb] = z < L ? z : L;
    adler[fb] = (uint32_t)((s2 + (unsigned long long)L) % EXR_ADLER) << 16 | (uint32_t)((s1 + 1ull) % EXR_ADLER);
}

// -------------------------------------------------------------------------------------------------------------------- (c) offsets
// one workgroup: block_pos[fb] = the sum of (8 + data_size) over the blocks before fb, of all frames; offsets[f] = where frame f's
// payload starts: its blocks' place plus the 8 nb bytes of every offset table before it
__global__ void __launch_bounds__(DF_T) exr_offsets_kernel(ExrGeo g, const int* __restrict__ data_size, long long* __restrict__ block_pos,
                                                           long long* __restrict__ offsets) {
    __shared__ uint32_t sh[DF_T / 64];
    const long long blocks = (long long)g.frames * g.nb;
    long long carry = 0;
    for (long long base = 0; base < blocks; base += DF_T) {
        const long long fb = base + threadIdx.x;
        const uint32_t v = fb < blocks ? 8u + (uint32_t)data_size[fb] : 0u;
        uint32_t total;
        const uint32_t before = df_scan(v, total, sh);                         // 256 sizes below 2^22 + 8
        if (fb < blocks) {
            block_pos[fb] = carry + before;
            if (fb % g.nb == 0) offsets[fb / g.nb] = 8ll * g.nb * (fb / g.nb) + carry + before;
        }
        carry += total;
    }
    if (threadIdx.x == 0) offsets[g.frames] = 8ll * g.nb * g.frames + carry;
}

// ----------------------------------------------------------------------------------------------------------------------- (d) pack
// `len` bytes from the word-aligned `srcw` to `dst` (any byte address): a head of at most 3 bytes, whole words put together from two
// of the source's, a tail of at most 3 bytes. Source word i + 1 is read only when it begins before byte `len`.
__device__ __forceinline__ void exr_copy(const uint32_t* __restrict__ srcw, int len, uint8_t* __restrict__ dst) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(srcw);
    const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    const int words = (len - head) >> 2;
    if ((int)threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    uint32_t* dstw = reinterpret_cast<uint32_t*>(dst + head);
    const int sh = 8 * head;
    for (int i = threadIdx.x; i < words; i += DF_T) {
        const uint32_t lo = srcw[i];
        dstw[i] = sh ? (lo >> sh) | (srcw[i + 1] << (32 - sh)) : lo;           // head >= 1: 4 i + 4 <= head + 4 i + 3 < len
    }
    const int done = head + 4 * words;
    if ((int)threadIdx.x < len - done) dst[done + threadIdx.x] = src[done + threadIdx.x];
}

__global__ void __launch_bounds__(DF_T) exr_pack_kernel(const float* __restrict__ depth, long long frame_stride, ExrGeo g, long long header_bytes,
                                                        const uint8_t* __restrict__ slots, const int* __restrict__ chunk_len,
                                                        const int* __restrict__ chunk_off, const int* __restrict__ data_size,
                                                        const uint32_t* __restrict__ adler, const long long* __restrict__ block_pos,
                                                        uint8_t* __restrict__ payload) {
    const int t = threadIdx.x;
    const long long id = blockIdx.x;
    const ExrChunk x = exr_chunk(g, id);
    const long long fb = (long long)x.frame * g.nb + x.b;
    const long long frame_pos = block_pos[(long long)x.frame * g.nb];          // of the frame's first block, among all blocks
    const long long table = 8ll * g.nb * x.frame + frame_pos;                  // the frame's payload: its offset table first
    uint8_t* block = payload + 8ll * g.nb * (x.frame + 1) + block_pos[fb];
    const int ds = data_size[fb];
    const bool compressed = ds < x.L;
    if (x.c == 0) {
        if (t < 8) {
            const unsigned long long where = (unsigned long long)(header_bytes + 8ll * g.nb + (block_pos[fb] - frame_pos));
            payload[table + 8 * x.b + t] = (uint8_t)(where >> (8 * t));
        } else if (t < 12) {
            block[t - 8] = (uint8_t)((uint32_t)(EXR_LINES * x.b) >> (8 * (t - 8)));
        } else if (t < 16) {
            block[t - 8] = (uint8_t)((uint32_t)ds >> (8 * (t - 12)));
        } else if (t < 18 && compressed) {
            block[t - 8] = t == 16 ? 0x78 : 0x01;
        }
    }
    if (compressed) {
        exr_copy(reinterpret_cast<const uint32_t*>(slots + id * DF_SLOT), chunk_len[id], block + 10 + chunk_off[id]);
        if (x.c == x.k - 1 && t >= 64 && t < 68) block[8 + ds - 4 + (t - 64)] = (uint8_t)(adler[fb] >> (8 * (67 - t)));     // big-endian
    } else {
        const uint32_t* raw = reinterpret_cast<const uint32_t*>(depth + (long long)x.frame * frame_stride + (long long)EXR_LINES * x.b * g.w);
        exr_copy(raw + (x.at >> 2), x.m, block + 8 + x.at);
    }
}

struct ExrLayout {
    ExrGeo g;
    size_t chunks, blocks;
    size_t slots, chunk_len, chunk_off, partial, data_size, adler, block_pos, total, payload;
};

// false: a size outside what the kernels' 32-bit arithmetic and one grid hold
bool exr_layout(long long frames, long long h, long long w, ExrLayout& L) {
    if (frames < 1 || h < 1 || w < 1 || h > EXR_MAX_SIDE || w > EXR_MAX_SIDE || frames > 0x7fffffffll) return false;
    ExrGeo& g = L.g;
    g.frames = (int)frames, g.h = (int)h, g.w = (int)w;
    g.nb = (g.h + EXR_LINES - 1) / EXR_LINES;
    const int klast = exr_chunks_of(exr_block_bytes(g, g.nb - 1));
    g.kfull = g.nb > 1 ? exr_chunks_of(exr_block_bytes(g, 0)) : klast;
    const long long cpf = (long long)(g.nb - 1) * g.kfull + klast;
    if (cpf * frames > 0x7fffffffll) return false;
    g.cpf = (int)cpf;
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    L.chunks = (size_t)cpf * (size_t)frames;
    L.blocks = (size_t)g.nb * (size_t)frames;
    L.slots = 0;
    L.chunk_len = L.slots + L.chunks * DF_SLOT;
    L.chunk_off = L.chunk_len + up16(L.chunks * 4);
    L.partial = L.chunk_off + up16(L.chunks * 4);
    L.data_size = L.partial + L.chunks * 16;
    L.adler = L.data_size + up16(L.blocks * 4);
    L.block_pos = L.adler + up16(L.blocks * 4);
    L.total = L.block_pos + up16(L.blocks * 8);
    L.payload = (size_t)frames * (16 * (size_t)g.nb + 4 * (size_t)w * (size_t)h);
    return true;
}

}  // namespace

extern "C" size_t vda_exr_workspace_bytes(int frames, int h, int w) {
    ExrLayout L;
    return exr_layout(frames, h, w, L) ? L.total : 0;
}

extern "C" size_t vda_exr_payload_bytes(int frames, int h, int w) {
    ExrLayout L;
    return exr_layout(frames, h, w, L) ? L.payload : 0;
}

extern "C" int vda_exr_zip_f32(const float* depth, int frames, int h, int w, long long frame_stride, long long header_bytes, void* workspace,
                               size_t workspace_bytes, uint8_t* payload, size_t payload_capacity, long long* offsets, vda_stream_t stream) {
    VDA_REQUIRE(depth, "vda_exr_zip_f32: depth is null");
    VDA_REQUIRE(workspace, "vda_exr_zip_f32: workspace is null");
    VDA_REQUIRE(payload, "vda_exr_zip_f32: payload is null");
    VDA_REQUIRE(offsets, "vda_exr_zip_f32: offsets is null");
    VDA_REQUIRE(frames > 0 && h > 0 && w > 0, "vda_exr_zip_f32: bad size frames=%d h=%d w=%d", frames, h, w);
    ExrLayout L;
    VDA_REQUIRE(exr_layout(frames, h, w, L), "vda_exr_zip_f32: too large frames=%d h=%d w=%d (h and w at most 65535, at most 2^31 - 1 chunks a call)",
                frames, h, w);
    VDA_REQUIRE(frame_stride >= (long long)h * w, "vda_exr_zip_f32: bad frame_stride=%lld (at least h * w = %lld)", frame_stride, (long long)h * w);
    VDA_REQUIRE(header_bytes >= 0, "vda_exr_zip_f32: bad header_bytes=%lld", header_bytes);
    VDA_REQUIRE(((uintptr_t)depth & 3) == 0, "vda_exr_zip_f32: depth is not 4-byte aligned");
    VDA_REQUIRE(((uintptr_t)workspace & 15) == 0, "vda_exr_zip_f32: workspace is not 16-byte aligned");
    VDA_REQUIRE(((uintptr_t)offsets & 7) == 0, "vda_exr_zip_f32: offsets is not 8-byte aligned");
    VDA_REQUIRE(workspace_bytes >= L.total, "vda_exr_zip_f32: workspace capacity %zu is below the %zu bytes of vda_exr_workspace_bytes", workspace_bytes,
                L.total);
    VDA_REQUIRE(payload_capacity >= L.payload, "vda_exr_zip_f32: payload capacity %zu is below the %zu bytes of vda_exr_payload_bytes", payload_capacity,
                L.payload);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    uint8_t* slots = ws + L.slots;
    int* chunk_len = reinterpret_cast<int*>(ws + L.chunk_len);
    int* chunk_off = reinterpret_cast<int*>(ws + L.chunk_off);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws + L.partial);
    int* data_size = reinterpret_cast<int*>(ws + L.data_size);
    uint32_t* adler = reinterpret_cast<uint32_t*>(ws + L.adler);
    long long* block_pos = reinterpret_cast<long long*>(ws + L.block_pos);
    const dim3 block(DF_T);
    hipLaunchKernelGGL(exr_encode_kernel, dim3((unsigned)L.chunks), block, 0, (hipStream_t)stream, depth, frame_stride, L.g, slots, chunk_len, partial);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(exr_blocks_kernel, dim3((unsigned)((L.blocks + DF_T - 1) / DF_T)), block, 0, (hipStream_t)stream, L.g, chunk_len, partial, chunk_off,
                       data_size, adler);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(exr_offsets_kernel, dim3(1), block, 0, (hipStream_t)stream, L.g, data_size, block_pos, offsets);
    VDA_LAUNCH_CHECK();
    hipLaunchKernelGGL(exr_pack_kernel, dim3((unsigned)L.chunks), block, 0, (hipStream_t)stream, depth, frame_stride, L.g, header_bytes, slots, chunk_len,
                       chunk_off, data_size, adler, block_pos, payload);
    VDA_LAUNCH_CHECK();
    return 0;
}
