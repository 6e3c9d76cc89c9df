// s2c_text.h — what the kernels that format counts as text share (s2c_table.hip, s2c_sites.hip,
// s2c_runs.hip):
// the decimal digit code, one position's row and its counts line, the workgroup's scan of line
// lengths to offsets, the blocks {a, b, p0} with their guards, and the aligned store of a
// sub-block's text out of its LDS image.
#pragma once
#include "s2c_common.h"

namespace s2c {

constexpr int TWG = 256;
constexpr int TLINE = 89;            // 10 digits of position, 11 of coverage, 6 x 10 of counts, 8 separators
constexpr int64_t TPOS_END = 10000000000ll;   // printed positions stay below 10^10 (10 digits)

// Inclusive prefix sum inside each 16-lane row (DPP row_shr, zeros shifted in).
__device__ __forceinline__ uint32_t row_scan16(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);
    return x;
}
// Inclusive prefix sum over the wave: the 16-lane row by DPP, then the rows below
__device__ __forceinline__ uint32_t wave_scan(uint32_t x, uint32_t lane) {
    uint32_t inc = row_scan16(x);
    const uint32_t r0 = __shfl(inc, 15), r1 = __shfl(inc, 31), r2 = __shfl(inc, 47);
    inc += (lane >= 16u ? r0 : 0u) + (lane >= 32u ? r1 : 0u) + (lane >= 48u ? r2 : 0u);
    return inc;
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
// "P\tCOV\tn-\tnA\tnC\tnG\tnN\tnT" written backwards, ending before byte `e` of buf
__device__ __forceinline__ void put_row(uint8_t *buf, uint32_t e, const Row &r) {
#pragma unroll
    for (int s = NSYM - 1; s >= 0; s--) {
        e = put32(buf, e, r.c[s]);
        buf[--e] = '\t';
    }
    e = put64(buf, e, r.cov);
    buf[--e] = '\t';
    put64(buf, e, r.pos);
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

// buf[sh, sh + tot) → d[0, tot), sh = d's offset inside its 16-byte word: 16-byte stores (LDS
// reads and global stores both aligned), head and tail bytes singly
__device__ __forceinline__ void store_text(const uint8_t *buf, uint8_t *d, uint32_t sh, uint32_t tot, uint32_t tid) {
    const uint32_t lo = sh, hi = sh + tot;
    const uint32_t vlo = (lo + 15u) & ~15u, vhi = hi & ~15u;
    uint8_t *d16 = d - sh;   // 16-byte aligned; byte k of buf goes to d16[k]
    for (uint32_t k = lo + tid; k < min(vlo, hi); k += TWG) d16[k] = buf[k];
    for (uint32_t k = vlo + 16u * tid; k < vhi; k += 16u * TWG) *(uint4 *)(d16 + k) = *(const uint4 *)(buf + k);
    for (uint32_t k = max(vhi, vlo) + tid; k < hi; k += TWG) d16[k] = buf[k];
}

}  // namespace s2c
