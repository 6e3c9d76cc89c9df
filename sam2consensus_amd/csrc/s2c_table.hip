// s2c_table.hip — per-position count tables as text, formatted on the device (--counts).
//
// One line per reference position, "P\tCOV\tn-\tnA\tnC\tnG\tnN\tnT\n": the position, the
// coverage (the sum of the six counts, :237) and the six counts of sequences[ref][pos]
// (:210-218) in S2C_NSYM order, plain decimal.  The kernels read any counts[6][padded_len]
// array (s2c_dev.counts after s2c_accumulate / s2c_pileup_counts, or a test's own) and know
// nothing else of a batch: the caller cuts the positions into blocks {a, b, p0}.
//
// The dense table of the scheme in s2c_text.h: k_table_len sums each block's line lengths,
// k_table_write walks its block in sub-blocks of TSUB positions, one per lane: coalesced loads
// of the six rows, the line length per lane, and the write side of one line per lane, written
// out here (emit_lines is the same lines for the walks' emits).
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr int TSUB = TWG;            // positions per sub-block: one line per lane
constexpr int TBUF = text_buf(TLINE);
static_assert(15 + TSUB * TLINE < TBUF, "the LDS image holds a sub-block's lines behind the destination's misalignment");

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
        block_total(sum, wsum, threadIdx.x, &lens[i]);
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
            // inclusive scan of the lengths: the wave's (s2c_text.h), then the waves below
            const uint32_t inc = wave_scan(len, lane);
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
                put_row(buf, e, r);
            }
            lds_sync();
            // (offs that do not match the lengths: the text is cut at the block's range)
            const uint64_t left = cap - run;
            if ((uint64_t)tot > left) tot = (uint32_t)left;
            store_text(buf, d, sh, tot, tid);
            run += tot;   // (buf is written again only past the next sub-block's first barrier)
        }
    }
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_table_len(const uint32_t *counts, int64_t padded_len, const int64_t *blocks, int64_t n,
                             int64_t *lens, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad count table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !blocks || !lens) return s2c_set_error(S2C_ERR_ARG, "NULL count table buffer");
    k_table_len<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, blocks, (uint64_t)n, lens);
    return launched("k_table_len");
}

extern "C" int s2c_table_write(const uint32_t *counts, int64_t padded_len, const int64_t *blocks, const int64_t *offs,
                               int64_t n, uint8_t *dst, int64_t dst_len, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0 || dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad count table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !blocks || !offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL count table buffer");
    // (7 workgroups of k_table_write fit a CU's LDS: a grid of 8 per CU keeps them all busy)
    k_table_write<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, blocks, offs, (uint64_t)n, dst, dst_len);
    return launched("k_table_write");
}
