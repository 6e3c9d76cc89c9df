// s2c_sites.hip — sparse tables of mixed sites as text, selected on the device (--variants).
//
// The rule, at one position with counts c[0..5] in S2C_NSYM order: cov = Σc (64-bit);
// rank(s) = #{s' : c[s'] > c[s] or (c[s'] == c[s] and s' < s)}; major the symbol of rank 0
// (ties: the earlier symbol); alt = cov − c[major].  The position is a site iff
// cov >= min_cov, alt >= min_alt and (double)alt >= min_frac · (double)cov (one fp64 product,
// -ffp-contract=off).  A site's line is the count table's plus three fields,
// "P\tCOV\tn-\tnA\tnC\tnG\tnN\tnT\tM\tALT\t0.dddd\n": M the major symbol, ALT the other symbols
// with a non-zero count in rank order (1 to 5 of them), dddd = ⌊alt · 10000 / cov⌋.
//
// Three launches.  k_sites_mark reads the six rows once (24 B per position) and leaves one bit
// per position: a wave covers 64 aligned positions and its ballot is the mask word.
// k_sites_len and k_sites_write are k_table_len / k_table_write over that mask: one workgroup
// per block {a, b, p0}, only the mask words over [a, b) read (1/8 B per position), the six
// rows loaded for set bits alone: walk_mask (s2c_text.h) queues the selected positions, and
// whenever the queue holds TWG of them, and at the block's end, every lane takes one: dense row
// loads, and in k_sites_write one line per lane through emit_lines.
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr int SLINE = TLINE + 15;          // + "\tM", "\tALT" (≤ 5 symbols), "\t0.dddd"
constexpr int SBUF = text_buf(SLINE);
constexpr uint64_t SYMS = 0x544E4743412Dull;   // "-ACGNT", symbol s in byte s

struct Rule {
    uint64_t min_cov, min_alt;
    double min_frac;
};

// cov − the largest count
__device__ __forceinline__ uint64_t alt_of(const Row &r) {
    uint32_t mx = r.c[0];
#pragma unroll
    for (uint32_t s = 1; s < NSYM; s++) mx = max(mx, r.c[s]);
    return r.cov - mx;
}
__device__ __forceinline__ bool is_site(const Row &r, const Rule &R) {
    const uint64_t alt = alt_of(r);
    return r.cov >= R.min_cov && alt >= R.min_alt && (double)alt >= R.min_frac * (double)r.cov;
}
// symbols with a non-zero count (≥ 1 at a site: cov ≥ 1); ALT has one fewer
__device__ __forceinline__ uint32_t nonzero(const Row &r) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) n += r.c[s] != 0u;
    return n;
}
__device__ __forceinline__ uint32_t site_len(const Row &r) { return line_len(r) + 10u + (nonzero(r) - 1u); }

// the site's line written to buf, ending before byte `e`
__device__ __forceinline__ void put_site(uint8_t *buf, uint32_t e, const Row &r) {
    const uint32_t nalt = nonzero(r) - 1u;
    uint32_t f = (uint32_t)(alt_of(r) * 10000ull / r.cov);   // < 10000: alt/cov ≤ 5/6
    buf[--e] = '\n';
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t q = f / 10u;
        buf[--e] = (uint8_t)('0' + (f - q * 10u));
        f = q;
    }
    buf[--e] = '.';
    buf[--e] = '0';
    buf[--e] = '\t';
    e -= nalt;   // ALT at [e, e + nalt), M at e − 2: the non-zero symbols hold the ranks 0..nalt
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) {
        uint32_t rank = 0;
#pragma unroll
        for (uint32_t t = 0; t < NSYM; t++) rank += (r.c[t] > r.c[s]) || (r.c[t] == r.c[s] && t < s);
        if (r.c[s] != 0u) buf[rank ? e + rank - 1u : e - 2u] = (uint8_t)(SYMS >> (8u * s));
    }
    buf[e - 1u] = '\t';
    buf[e - 3u] = '\t';
    put_row(buf, e - 3u, r);
}

// mask[w] = the ballot of is_site over positions [64 w, 64 w + 64); bits at or past padded_len zero
__global__ __launch_bounds__(TWG) void k_sites_mark(const uint32_t *__restrict__ counts, int64_t padded_len, Rule R,
                                                     uint64_t *__restrict__ mask, uint64_t n_words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * MWORDS + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * MWORDS;
    for (uint64_t w = wave; w < n_words; w += n_waves) {
        const uint64_t g = w * 64u + lane;
        bool site = false;
        if (g < (uint64_t)padded_len) site = is_site(load_row(counts, (uint64_t)padded_len, g, 0), R);
        const uint64_t word = __ballot(site);
        if (lane == 0) mask[w] = word;
    }
}

// bits of mask word w inside [a, b) (w one of the words [a, b) overlaps)
__device__ __forceinline__ uint64_t blk_word(const uint64_t *__restrict__ mask, int64_t w, const Blk &B) {
    uint64_t m = mask[w];
    const int64_t lo = w << 6;
    if (B.a > lo) m &= ~0ull << (B.a - lo);
    if (B.b < lo + 64) m &= ~0ull >> (lo + 64 - B.b);
    return m;
}

// walk_mask over block B's sites: emit(head, cnt) on every TWG queued positions and on the rest
template <typename Emit>
__device__ __forceinline__ void walk_block(const uint64_t *__restrict__ mask, const Blk &B, uint64_t *queue, uint32_t lane,
                                           uint32_t wv, Emit emit) {
    const auto word = [](const uint64_t *__restrict__ mk, int64_t w, const Blk &K) { return blk_word(mk, w, K); };
    walk_mask<false>(mask, B, word, queue, lane, wv, emit, emit);
}

// lens[i] = bytes of block i's site lines (0 for a block the guards refuse)
__global__ __launch_bounds__(TWG) void k_sites_len(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                    const uint64_t *__restrict__ mask, const int64_t *__restrict__ blocks,
                                                    uint64_t n, int64_t *__restrict__ lens) {
    __shared__ uint64_t queue[QCAP];
    __shared__ uint64_t wsum[TWG / 64];
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Blk B = load_blk(blocks, i);
        uint64_t sum = 0;
        if (B.ok(padded_len) && B.a < B.b)
            walk_block(mask, B, queue, lane, wv, [&](uint32_t qh, uint32_t cnt) {
                lds_sync();
                const uint64_t g = tid < cnt ? queue[(qh + tid) & (QCAP - 1u)] : 0;
                lds_sync();
                if (tid < cnt)
                    sum += site_len(load_row(counts, (uint64_t)padded_len, g, (uint64_t)B.p0 + (g - (uint64_t)B.a)));
            });
        block_total(sum, wsum, tid, &lens[i]);
    }
}

// block i's site lines → dst[offs[i], offs[i+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_sites_write(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                      const uint64_t *__restrict__ mask, const int64_t *__restrict__ blocks,
                                                      const int64_t *__restrict__ offs, uint64_t n,
                                                      uint8_t *__restrict__ dst, int64_t dst_len) {
    __shared__ alignas(16) uint8_t buf[SBUF];
    __shared__ uint64_t queue[QCAP];
    __shared__ uint32_t wtot[TWG / 64];   // wave totals of the line lengths
    S2C_POISON(buf, SBUF);
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wtot, sizeof(wtot));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const Blk B = load_blk(blocks, i);
        const int64_t d0 = offs[i], d1 = offs[i + 1];
        if (!B.ok(padded_len) || d0 < 0 || d1 < d0 || d1 > dst_len || B.a == B.b) continue;
        const uint64_t cap = (uint64_t)(d1 - d0);
        uint64_t run = 0;   // bytes of the block written so far
        // cnt ≤ TWG queued positions, one line per lane
        walk_block(mask, B, queue, lane, wv, [&](uint32_t qh, uint32_t cnt) {
            lds_sync();   // (buf and wtot are no longer read either)
            const bool in = tid < cnt;
            Row r{};
            uint32_t len = 0;
            if (in) {
                const uint64_t g = queue[(qh + tid) & (QCAP - 1u)];
                r = load_row(counts, (uint64_t)padded_len, g, (uint64_t)B.p0 + (g - (uint64_t)B.a));
                len = site_len(r);
            }
            run += emit_lines<SLINE>(buf, wtot, dst + d0, cap, run, in, len, tid, lane, wv,
                                     [&](uint8_t *img, uint32_t e) { put_site(img, e, r); });
        });
    }
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_sites_mark(const uint32_t *counts, int64_t padded_len, int64_t min_cov, int64_t min_alt,
                              double min_frac, uint64_t *mask, void *stream) {
    using namespace s2c;
    if (padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad site table sizes");
    if (min_cov < 1 || min_alt < 1 || !(min_frac >= 0.0 && min_frac <= 1.0))
        return s2c_set_error(S2C_ERR_ARG, "site rule: min_cov >= 1, min_alt >= 1, 0 <= min_frac <= 1");
    if (padded_len == 0) return S2C_OK;
    if (!counts || !mask) return s2c_set_error(S2C_ERR_ARG, "NULL site table buffer");
    const int64_t n_words = (padded_len + 63) / 64;
    const unsigned grid = (unsigned)std::min<int64_t>((n_words + MWORDS - 1) / MWORDS, 8 * 256 * 8);
    k_sites_mark<<<grid, TWG, 0, (hipStream_t)stream>>>(counts, padded_len, Rule{(uint64_t)min_cov, (uint64_t)min_alt, min_frac},
                                                         mask, (uint64_t)n_words);
    return launched("k_sites_mark");
}

extern "C" int s2c_sites_len(const uint32_t *counts, int64_t padded_len, const uint64_t *mask, const int64_t *blocks,
                             int64_t n, int64_t *lens, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad site table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !mask || !blocks || !lens) return s2c_set_error(S2C_ERR_ARG, "NULL site table buffer");
    k_sites_len<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, mask, blocks, (uint64_t)n, lens);
    return launched("k_sites_len");
}

extern "C" int s2c_sites_write(const uint32_t *counts, int64_t padded_len, const uint64_t *mask, const int64_t *blocks,
                               const int64_t *offs, int64_t n, uint8_t *dst, int64_t dst_len, void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0 || dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad site table sizes");
    if (n == 0) return S2C_OK;
    if (!counts || !mask || !blocks || !offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL site table buffer");
    // (5 workgroups of k_sites_write fit a CU's LDS)
    k_sites_write<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, mask, blocks, offs, (uint64_t)n, dst, dst_len);
    return launched("k_sites_write");
}
