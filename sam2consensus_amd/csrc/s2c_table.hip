// s2c_table.hip — per-position count tables as text, formatted on the device (--counts).
//
// One line per reference position, "P\tCOV\tn-\tnA\tnC\tnG\tnN\tnT\n": the position, the
// coverage (the sum of the six counts, :237) and the six counts of sequences[ref][pos]
// (:210-218) in S2C_NSYM order, plain decimal.  The kernels read any counts[6][padded_len]
// array (s2c_dev.counts after s2c_accumulate / s2c_pileup_counts, or a test's own) and know
// nothing else of a batch: the caller cuts the positions into blocks {a, b, p0}.
//
// Lines have no fixed width, so the text takes two passes like the FASTA bodies' lengths and
// gather: k_table_len sums each block's line lengths, the caller takes the exclusive prefix
// sum, k_table_write formats block i into dst[offs[i], offs[i+1]).  Both are one workgroup per
// block, grid-strided.  k_table_write walks its block in sub-blocks of TSUB positions, one per
// lane: coalesced loads of the six rows, the line length per lane, a workgroup scan of the
// lengths (DPP inside a row, the row and wave totals above it), every lane writes its line
// into LDS at its scanned offset, and the sub-block's contiguous bytes leave with 16-byte
// stores.  The LDS image is shifted by the destination's misalignment, so LDS reads and
// global stores are both 16-byte aligned; head and tail bytes go out singly.
#include "s2c_common.h"

namespace s2c {
namespace {

constexpr int TWG = 256;
constexpr int TSUB = TWG;            // positions per sub-block: one line per lane
constexpr int TLINE = 89;            // 10 digits of position, 11 of coverage, 6 x 10 of counts, 8 separators
constexpr int TBUF = TSUB * TLINE + 16;   // + the destination's misalignment (< 16)
constexpr int64_t TPOS_END = 10000000000ll;   // printed positions stay below 10^10 (10 digits)

// Inclusive prefix sum inside each 16-lane row (DPP row_shr, zeros shifted in).
__device__ __forceinline__ uint32_t row_scan16(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);
    return x;
}

__device__ __forceinline__ uint32_t ndig32(uint32_t x) {
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) +
           (x >= 10000000u) + (x >= 100000000u) + (x >= 1000000000u);
}
// values below 2^41 (positions < 10^10, coverage ≤ 6·(2^32 − 1)) split at 10^9 = 2^9 · 1953125
// with a 32-bit division by a constant: ⌊v / 10^9⌋ = ⌊⌊v / 2^9⌋ / 1953125⌋
__device__ __forceinline__ void split9(uint64_t v, uint32_t &hi, uint32_t &lo) {
    hi = (uint32_t)(v >> 9) / 1953125u;
    lo = (uint32_t)(v - (uint64_t)hi * 1000000000ull);
}
__device__ __forceinline__ uint32_t ndig64(uint64_t v) {
    if (v < 1000000000ull) return ndig32((uint32_t)v);
    uint32_t hi, lo;
    split9(v, hi, lo);
    return 9u + ndig32(hi);
}

struct Row {
    uint32_t c[NSYM];
    uint64_t cov, pos;
};
__device__ __forceinline__ Row load_row(const uint32_t *__restrict__ counts, uint64_t padded_len, uint64_t g, uint64_t pos) {
    Row r;
    r.cov = 0;
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) {
        r.c[s] = counts[s * padded_len + g];
        r.cov += r.c[s];
    }
    r.pos = pos;
    return r;
}
__device__ __forceinline__ uint32_t line_len(const Row &r) {
    uint32_t n = ndig64(r.pos) + ndig64(r.cov) + 8u;
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) n += ndig32(r.c[s]);
    return n;
}

// decimal digits of x written backwards, ending before byte `e` of buf; returns the first byte
__device__ __forceinline__ uint32_t put32(uint8_t *buf, uint32_t e, uint32_t x) {
    do {
        const uint32_t q = x / 10u;
        buf[--e] = (uint8_t)('0' + (x - q * 10u));
        x = q;
    } while (x);
    return e;
}
__device__ __forceinline__ uint32_t put64(uint8_t *buf, uint32_t e, uint64_t v) {
    if (v < 1000000000ull) return put32(buf, e, (uint32_t)v);
    uint32_t hi, lo;
    split9(v, hi, lo);
    for (int k = 0; k < 9; k++) {   // the low nine digits, zeros included
        const uint32_t q = lo / 10u;
        buf[--e] = (uint8_t)('0' + (lo - q * 10u));
        lo = q;
    }
    return put32(buf, e, hi);
}

struct Blk {
    int64_t a, b, p0;
    __device__ __forceinline__ bool ok(int64_t padded_len) const {
        return a >= 0 && a <= b && b <= padded_len && p0 >= 0 && p0 <= TPOS_END - (b - a);
    }
};
__device__ __forceinline__ Blk load_blk(const int64_t *__restrict__ blocks, uint64_t i) {
    return Blk{blocks[3 * i], blocks[3 * i + 1], blocks[3 * i + 2]};
}

// lens[i] = bytes of block i's text (0 for a block the guards refuse)
__global__ __launch_bounds__(TWG) void k_table_len(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                    const int64_t *__restrict__ blocks, uint64_t n,
                                                    int64_t *__restrict__ lens) {
    __shared__ uint64_t wsum[TWG / 64];
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Blk B = load_blk(blocks, i);
        uint64_t sum = 0;
        if (B.ok(padded_len))
            for (int64_t g = B.a + threadIdx.x; g < B.b; g += TWG)
                sum += line_len(load_row(counts, (uint64_t)padded_len, (uint64_t)g, (uint64_t)(B.p0 + (g - B.a))));
        sum = wave_sum(sum);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = sum;
        lds_sync();
        if (threadIdx.x == 0) {
            uint64_t t = 0;
            for (int w = 0; w < TWG / 64; w++) t += wsum[w];
            lens[i] = (int64_t)t;
        }
        lds_sync();   // (wsum is written again for the next block)
    }
}

// block i's text → dst[offs[i], offs[i+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_table_write(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                      const int64_t *__restrict__ blocks, const int64_t *__restrict__ offs,
                                                      uint64_t n, uint8_t *__restrict__ dst, int64_t dst_len) {
    __shared__ alignas(16) uint8_t buf[TBUF];
    __shared__ uint32_t wtot[2][TWG / 64];   // wave totals of the line lengths, by sub-block parity
    S2C_POISON(buf, TBUF);
    S2C_POISON(wtot, sizeof(wtot));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t par = 0;   // wtot's half: the next sub-block's totals never land on ones still being read
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Blk B = load_blk(blocks, i);
        const int64_t d0 = offs[i], d1 = offs[i + 1];
        if (!B.ok(padded_len) || d0 < 0 || d1 < d0 || d1 > dst_len) continue;
        const uint64_t cap = (uint64_t)(d1 - d0);
        uint64_t run = 0;   // bytes of the block written so far
        for (int64_t s0 = B.a; s0 < B.b; s0 += TSUB, par ^= 1u) {
            const int64_t g = s0 + tid;
            const bool in = g < B.b;
            Row r{};
            uint32_t len = 0;
            if (in) {
                r = load_row(counts, (uint64_t)padded_len, (uint64_t)g, (uint64_t)(B.p0 + (g - B.a)));
                len = line_len(r);
            }
            // inclusive scan of the lengths: the 16-lane row by DPP, then the rows and waves below
            uint32_t inc = row_scan16(len);
            const uint32_t r0 = __shfl(inc, 15), r1 = __shfl(inc, 31), r2 = __shfl(inc, 47);
            inc += (lane >= 16u ? r0 : 0u) + (lane >= 32u ? r1 : 0u) + (lane >= 48u ? r2 : 0u);
            if (lane == 63u) wtot[par][wv] = inc;
            lds_sync();
            uint32_t below = 0, tot = 0;
#pragma unroll
            for (uint32_t w = 0; w < TWG / 64; w++) {
                const uint32_t t = wtot[par][w];
                below += w < wv ? t : 0u;
                tot += t;
            }
            // the LDS image starts at the destination's offset inside its 16-byte word
            uint8_t *d = dst + d0 + run;
            const uint32_t sh = (uint32_t)((uintptr_t)d & 15u);
            if (in) {
                uint32_t e = sh + below + inc;   // the line's end; ≤ 15 + TSUB·TLINE < TBUF
                buf[--e] = '\n';
#pragma unroll
                for (int s = NSYM - 1; s >= 0; s--) {
                    e = put32(buf, e, r.c[s]);
                    buf[--e] = '\t';
                }
                e = put64(buf, e, r.cov);
                buf[--e] = '\t';
                put64(buf, e, r.pos);
            }
            lds_sync();
            // (offs that do not match the lengths: the text is cut at the block's range)
            const uint64_t left = cap - run;
            if ((uint64_t)tot > left) tot = (uint32_t)left;
            const uint32_t lo = sh, hi = sh + tot;
            const uint32_t vlo = (lo + 15u) & ~15u, vhi = hi & ~15u;
            uint8_t *d16 = d - sh;   // 16-byte aligned; byte k of buf goes to d16[k]
            for (uint32_t k = lo + tid; k < min(vlo, hi); k += TWG) d16[k] = buf[k];
            for (uint32_t k = vlo + 16u * tid; k < vhi; k += 16u * TWG) *(uint4 *)(d16 + k) = *(const uint4 *)(buf + k);
            for (uint32_t k = max(vhi, vlo) + tid; k < hi; k += TWG) d16[k] = buf[k];
            run += tot;   // (buf is written again only past the next sub-block's first barrier)
        }
    }
}

// (7 workgroups of k_table_write fit a CU's LDS: a grid of 8 per CU keeps them all busy)
unsigned table_grid(int64_t n) { return (unsigned)std::min<int64_t>(n, 8 * 256 * 4); }

}  // namespace
}  // namespace s2c

extern "C" int s2c_table_len(const uint32_t *counts, int64_t padded_len, const int64_t *blocks, int64_t n,
                             int64_t *lens, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad count table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !blocks || !lens) return s2c_set_error(S2C_ERR_ARG, "NULL count table buffer");
    k_table_len<<<table_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, blocks, (uint64_t)n, lens);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? S2C_OK : s2c_set_error(S2C_ERR_HIP, std::string("k_table_len: ") + hipGetErrorString(e));
}

extern "C" int s2c_table_write(const uint32_t *counts, int64_t padded_len, const int64_t *blocks, const int64_t *offs,
                               int64_t n, uint8_t *dst, int64_t dst_len, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0 || dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad count table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !blocks || !offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL count table buffer");
    k_table_write<<<table_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, blocks, offs, (uint64_t)n, dst,
                                                                  dst_len);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? S2C_OK : s2c_set_error(S2C_ERR_HIP, std::string("k_table_write: ") + hipGetErrorString(e));
}
