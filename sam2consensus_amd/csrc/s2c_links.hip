// s2c_links.hip — allele pairs that fragments carry across neighbouring mixed sites, counted and
// formatted on the device (--links).
//
// The sites are the set bits of the mask s2c_sites_mark left; site k (its rank: the set bits
// below it) pairs with site k + 1.  A fragment is a piece of the batch; it observes symbol s at
// position p iff it adds one to counts[s][p] (:210-218).  pairs[k][s1][s2] = the fragments that
// observe s1 at site k and s2 at site k + 1, u32 [n_sites][6][6].  A pair's line is
// "POS1\tPOS2\tREADS\tHAPS\tXY:n,XY:n,...\n": READS = Σ n, HAPS the non-zero entries, those
// entries by n falling, then (s1, s2) in -ACGNT order; listed iff READS >= min_reads (>= 1) and
// site k + 1 lies in the same reference.
//
// Four launches.
//   k_links_pop    pop[w] = popcount(mask[w]); the caller's exclusive prefix sum is rank[w].
//   k_links_count  one lane per piece, the token walk of k_reads (walk_piece): for every run it
//                  asks rank and the run's two end words how many sites lie under it — none,
//                  almost always — and visits those in position order, taking the symbol as the
//                  count does; (rank, symbol) of the observation before stays in registers, and
//                  an observation of the next rank adds one to a pair.  A site whose '-' the
//                  maxdel rule drops is no observation, so the ranks around it are not
//                  consecutive and nothing links across it.  Adds to one destination are summed
//                  in a workgroup's LDS table first (amplicons send every read to the same few
//                  rows); a workgroup takes a contiguous stretch of pieces — bucketed by start
//                  word, so its destinations are neighbours — and flushes the table every 1,024
//                  pieces, before the sites under them outgrow it.
//   k_links_len / k_links_write   the two passes of s2c_text.h over the blocks {a, b, p0} with
//                  their references' ranges {s, e}: walk_mask queues a block's sites, a lane per
//                  site reads its row of 36 counts; a listed pair looks its second site up in
//                  the mask (a fragment spans the two, so it is near).  Lines run to 542 bytes:
//                  an LDS image of TWG of them would leave one workgroup a CU.  The write pass
//                  hands a step's lines to s2c_text.h's emit_var_lines: when they sum to at most
//                  LIMG bytes (44 bytes a line on C5: nearly always) they go through an image of
//                  that size and store_text; a longer step stores its bytes singly through the
//                  block's guarded range (Out).  put_line writes to either.
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr uint32_t NPAIR = NSYM * NSYM;
constexpr uint32_t HCAP = 1024;            // slots of a workgroup's table of pending adds
constexpr uint32_t HPROBE = 4;             // slots tried before an add goes to HBM directly
constexpr uint32_t HSTEPS = 4;             // steps of TWG pieces between two flushes of the table
constexpr uint32_t HEMPTY = 0xFFFFFFFFu;
constexpr uint32_t NO_RANK = 0xFFFFFFFEu;  // (+ 1 is no rank either: ranks stay below n_sites < 2^32)
constexpr uint64_t SYMS = 0x544E4743412Dull;   // "-ACGNT", symbol s in byte s

__global__ __launch_bounds__(TWG) void k_links_pop(const uint64_t *__restrict__ mask, uint64_t n_words, uint32_t *__restrict__ pop) {
    for (uint64_t w = (uint64_t)blockIdx.x * TWG + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * TWG)
        pop[w] = (uint32_t)__popcll(mask[w]);
}

struct CountArgs {
    const uint32_t *pc, *ops, *bq, *bx, *rank;
    const uint64_t *mask;
    uint32_t *pairs;
    uint64_t n_qwords, padded_len, n_sites;
    uint32_t n, per, maxdel_active, maxdel;   // per: pieces per workgroup
};

// pairs[idx] += 1, through the workgroup's table when a slot is free for idx
__device__ __forceinline__ void add_pair(const CountArgs &d, uint32_t *hkey, uint32_t *hcnt, uint64_t idx) {
    if (idx < HEMPTY) {
        const uint32_t key = (uint32_t)idx;
        uint32_t s = (key * 2654435761u) >> 22;   // (HCAP = 2^10)
        for (uint32_t probe = 0; probe < HPROBE; probe++) {
            const uint32_t prev = atomicCAS(&hkey[s], HEMPTY, key);
            if (prev == HEMPTY || prev == key) {
                atomicAdd(&hcnt[s], 1u);
                return;
            }
            s = (s + 1u) & (HCAP - 1u);
        }
    }
    atomicAdd(d.pairs + idx, 1u);
}

// piece i walked against the sites: its observations in rising position, each one that follows
// an observation of the rank below adds its pair
__device__ __forceinline__ void piece_links(const CountArgs &d, uint32_t *hkey, uint32_t *hcnt, uint64_t i) {
    const uint4 P = ((const uint4 *)d.pc)[i];
    const uint32_t oend = d.pc[4 * i + 6];   // next piece's opoff (sentinel at the end)
    uint32_t prev_rank = NO_RANK, prev_sym = 0;
    walk_piece(GlobalMem{d.ops, d.bq, d.bx}, P, oend, d.maxdel_active != 0, d.maxdel,
               [&](uint32_t, uint32_t g, uint32_t l, uint32_t kind, uint64_t q) {
                   if (!l || (uint64_t)g >= d.padded_len) return;
                   const uint64_t hi = min((uint64_t)g + l, d.padded_len) - 1u;   // the run's last position
                   const uint64_t w0 = g >> 6, w1 = hi >> 6;
                   const uint64_t from_g = ~0ull << (g & 63u), upto_hi = ~0ull >> (63u - (hi & 63u));
                   // r: the sites below g (the rank of the first one under the run); left: those in [g, hi]
                   uint32_t r = d.rank[w0] + (uint32_t)__popcll(d.mask[w0] & ~from_g);
                   uint32_t left = d.rank[w1] + (uint32_t)__popcll(d.mask[w1] & upto_hi) - r;
                   for (uint64_t w = w0; w <= w1 && left; w++) {
                       uint64_t m = d.mask[w];
                       if (w == w0) m &= from_g;
                       if (w == w1) m &= upto_hi;
                       for (; m && left; m &= m - 1u, left--, r++) {
                           const uint64_t p = (w << 6) + (uint32_t)__builtin_ctzll(m);
                           uint32_t sym = 0;
                           if ((kind & 3u) == S2C_RUN_BASES) {
                               const uint64_t qq = q + (p - g), qw = qq >> 5;
                               const uint32_t sh = (uint32_t)(qq & 31u);
                               if (qw >= d.n_qwords) continue;
                               const uint32_t p0 = (d.bq[2 * qw] >> sh) & 1u, p1 = (d.bq[2 * qw + 1] >> sh) & 1u;
                               const uint32_t x = (kind & S2C_RUN_XBIT) ? (d.bx[qw] >> sh) & 1u : 0u;
                               sym = sym_code(p0, p1, x);
                               if (sym == 0u && (kind & S2C_RUN_DROP)) continue;   // (:210: this '-' is not counted)
                           }
                           if ((uint64_t)r >= d.n_sites) continue;
                           if (r == prev_rank + 1u) add_pair(d, hkey, hcnt, (uint64_t)prev_rank * NPAIR + prev_sym * NSYM + sym);
                           prev_rank = r;
                           prev_sym = sym;
                       }
                   }
               },
               [](uint64_t, uint64_t, uint32_t) {});
}

__global__ __launch_bounds__(TWG) void k_links_count(const CountArgs d) {
    __shared__ uint32_t hkey[HCAP];
    __shared__ uint32_t hcnt[HCAP];
    S2C_POISON(hkey, sizeof(hkey));
    S2C_POISON(hcnt, sizeof(hcnt));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x;
    for (uint32_t s = tid; s < HCAP; s += TWG) {
        hkey[s] = HEMPTY;
        hcnt[s] = 0u;
    }
    lds_sync();
    const uint64_t first = (uint64_t)blockIdx.x * d.per, last = min(first + d.per, (uint64_t)d.n);
    uint32_t step = 0;
    for (uint64_t base = first; base < last; base += TWG) {
        if (base + tid < last) piece_links(d, hkey, hcnt, base + tid);
        // the table to HBM every HSTEPS steps (while its keys, the sites under a few hundred
        // neighbouring pieces, still fit it) and at the end; base and last are the workgroup's
        if (++step == HSTEPS || base + TWG >= last) {
            step = 0;
            lds_sync();
            for (uint32_t s = tid; s < HCAP; s += TWG) {
                const uint32_t key = hkey[s];
                if (key != HEMPTY) {
                    atomicAdd(d.pairs + key, hcnt[s]);
                    hkey[s] = HEMPTY;
                    hcnt[s] = 0u;
                }
            }
            lds_sync();
        }
    }
}

struct LinkArgs {
    const uint64_t *mask;
    const uint32_t *rank, *pairs;
    const int64_t *blocks, *refs;
    uint64_t n, n_sites, min_reads;
    int64_t padded_len;
};

// the sites of mask word w inside [a, b) (w one of the words [a, b) overlaps)
__device__ __forceinline__ uint64_t site_word(const uint64_t *__restrict__ mask, int64_t w, const RBlk &B) {
    uint64_t m = mask[w];
    const int64_t lo = w << 6;
    if (B.a > lo) m &= ~0ull << (B.a - lo);
    if (B.b < lo + 64) m &= ~0ull >> (lo + 64 - B.b);
    return m;
}
template <typename Emit>
__device__ __forceinline__ void walk_block(const uint64_t *__restrict__ mask, const RBlk &B, uint64_t *queue, uint32_t lane,
                                           uint32_t wv, Emit emit) {
    const auto word = [](const uint64_t *__restrict__ mk, int64_t w, const RBlk &K) { return site_word(mk, w, K); };
    walk_mask<false>(mask, B, word, queue, lane, wv, emit, emit);
}

// the first site in [from, e), or e
__device__ __forceinline__ uint64_t next_site(const uint64_t *__restrict__ mask, uint64_t from, uint64_t e) {
    if (from >= e) return e;
    const uint64_t wl = (e - 1u) >> 6;
    uint64_t w = from >> 6, m = mask[w] & (~0ull << (from & 63u));
    while (!m && w < wl) m = mask[++w];
    const uint64_t p = (w << 6) + (m ? (uint32_t)__builtin_ctzll(m) : 64u);
    return p < e ? p : e;
}

struct Line {
    uint64_t pos1, pos2, reads;   // printed positions
    uint64_t nz;                  // bit k: entry k of the row is not zero
    uint32_t haps, len;           // len == 0: no line
    const uint4 *row;
};
// the row's 36 counts, the nine loads in flight together
__device__ __forceinline__ void load_pairs(const uint4 *row, uint32_t (&c)[NPAIR]) {
#pragma unroll
    for (uint32_t k = 0; k < NPAIR / 4; k++) {
        const uint4 v = row[k];
        c[4 * k] = v.x; c[4 * k + 1] = v.y; c[4 * k + 2] = v.z; c[4 * k + 3] = v.w;
    }
}
// The line of block B's site g; len = 0 when the pair is not listed — a rank at or past n_sites,
// READS < min_reads, no later site before e.
__device__ __forceinline__ Line line_of(const LinkArgs &d, const RBlk &B, uint64_t g) {
    Line L{};
    const uint64_t w = g >> 6;
    const uint64_t r = (uint64_t)d.rank[w] + (uint32_t)__popcll(d.mask[w] & ~(~0ull << (g & 63u)));
    if (r >= d.n_sites) return L;
    L.row = (const uint4 *)(d.pairs + r * NPAIR);
    uint32_t text = 0;
    for (uint32_t k4 = 0; k4 < NPAIR; k4 += 4u) {
        const uint4 v = L.row[k4 / 4u];
        const uint32_t c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            L.reads += c[j];
            L.nz |= (uint64_t)(c[j] != 0u) << (k4 + j);
            text += c[j] ? 4u + ndig32(c[j]) : 0u;   // "XY:n" and a ',' or the line's '\n'
        }
    }
    L.haps = (uint32_t)__popcll(L.nz);
    if (L.reads < d.min_reads) return L;
    const uint64_t g2 = next_site(d.mask, g + 1u, (uint64_t)B.e);
    if (g2 >= (uint64_t)B.e) return L;
    L.pos1 = (uint64_t)B.p0 + (g - (uint64_t)B.a);
    L.pos2 = (uint64_t)B.p0 + (g2 - (uint64_t)B.a);
    L.len = ndig64(L.pos1) + ndig64(L.pos2) + ndig64(L.reads) + ndig32(L.haps) + 4u + text;
    return L;
}

// the line at o[at, at + L.len): the head's numbers backwards from its end, then every non-zero
// entry behind the bytes of the entries that come before it.  An entry reads the row again — 144
// bytes the caches hold, nine loads in flight together, one round trip for each of the line's
// few entries — so that the kernel does not hold 36 counts and their widths in registers across
// the loop (the barrier keeps the compiler from hoisting the loads: 256 VGPRs, one wave a SIMD).
template <typename Dst>
__device__ __forceinline__ void put_line(const Dst &o, uint64_t at, const Line &L) {
    const uint64_t head = at + ndig64(L.pos1) + ndig64(L.pos2) + ndig64(L.reads) + ndig32(L.haps) + 4u;
    uint64_t e = head;
    o.put(--e, '\t');
    e = put32(o, e, L.haps);
    o.put(--e, '\t');
    e = put64(o, e, L.reads);
    o.put(--e, '\t');
    e = put64(o, e, L.pos2);
    o.put(--e, '\t');
    put64(o, e, L.pos1);
    for (uint64_t nz = L.nz; nz; nz &= nz - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctzll(nz);
        uint32_t ck = 0, off = 0;
        uint32_t c[NPAIR];
        asm volatile("" ::: "memory");
        load_pairs(L.row, c);
#pragma unroll
        for (uint32_t j = 0; j < NPAIR; j++) ck = j == k ? c[j] : ck;
#pragma unroll
        for (uint32_t j = 0; j < NPAIR; j++) off += (c[j] > ck || (c[j] == ck && j < k)) ? 4u + ndig32(c[j]) : 0u;
        const uint64_t s = head + off, end = s + 3u + ndig32(ck);
        o.put(s, (uint32_t)(SYMS >> (8u * (k / NSYM))) & 0xFFu);
        o.put(s + 1u, (uint32_t)(SYMS >> (8u * (k % NSYM))) & 0xFFu);
        o.put(s + 2u, ':');
        put32(o, end, ck);
        o.put(end, end + 1u == at + L.len ? '\n' : ',');
    }
}

// lens[i] = bytes of block i's lines (0 for a block the guards refuse)
__global__ __launch_bounds__(TWG) void k_links_len(const LinkArgs d, int64_t *__restrict__ lens) {
    __shared__ uint64_t queue[QCAP];
    __shared__ uint64_t wsum[TWG / 64];
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < d.n; i += gridDim.x) {
        const RBlk B = load_rblk(d.blocks, d.refs, i);
        uint64_t sum = 0;
        if (B.ok(d.padded_len) && B.a < B.b)
            walk_block(d.mask, B, queue, lane, wv, [&](uint32_t qh, uint32_t cnt) {
                lds_sync();
                const uint64_t g = tid < cnt ? queue[(qh + tid) & (QCAP - 1u)] : 0;
                lds_sync();
                if (tid < cnt) sum += line_of(d, B, g).len;
            });
        block_total(sum, wsum, tid, &lens[i]);
    }
}

// block i's lines → dst[offs[i], offs[i+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_links_write(const LinkArgs d, const int64_t *__restrict__ offs,
                                                      uint8_t *__restrict__ dst, int64_t dst_len) {
    __shared__ alignas(16) uint8_t buf[LIMG + 16];
    __shared__ uint64_t queue[QCAP];
    __shared__ uint32_t wtot[TWG / 64];   // wave totals of the line lengths
    S2C_POISON(buf, sizeof(buf));
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wtot, sizeof(wtot));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < d.n; i += gridDim.x) {
        const RBlk B = load_rblk(d.blocks, d.refs, i);
        const int64_t d0 = offs[i], d1 = offs[i + 1];
        if (!B.ok(d.padded_len) || d0 < 0 || d1 < d0 || d1 > dst_len || B.a == B.b) continue;
        const Out o{dst + d0, (uint64_t)(d1 - d0)};
        uint64_t run = 0;   // bytes of the block's lines so far
        walk_block(d.mask, B, queue, lane, wv, [&](uint32_t qh, uint32_t cnt) {
            lds_sync();   // (the entries are in; wtot and buf are no longer read)
            Line L{};
            if (tid < cnt) L = line_of(d, B, queue[(qh + tid) & (QCAP - 1u)]);
            run += emit_var_lines<LIMG>(buf, wtot, o, run, L.len, tid, lane, wv, [&](const auto &to, uint64_t at) { put_line(to, at, L); });
        });
    }
}

int check_sizes(int64_t padded_len, int64_t n_sites) {
    if (padded_len < 0 || n_sites < 0 || n_sites > 0xFFFFFFFFll) return s2c_set_error(S2C_ERR_ARG, "bad link table sizes");
    return S2C_OK;
}

int link_args(LinkArgs &a, const uint64_t *mask, const uint32_t *rank, int64_t padded_len, const uint32_t *pairs, int64_t n_sites,
              const int64_t *blocks, const int64_t *refs, int64_t n, int64_t min_reads) {
    if (n < 0 || check_sizes(padded_len, n_sites)) return s2c_set_error(S2C_ERR_ARG, "bad link table sizes");
    if (min_reads < 1 || min_reads > 0xFFFFFFFFll) return s2c_set_error(S2C_ERR_ARG, "link tables: 1 <= min_reads < 2^32");
    if (n == 0) return S2C_OK;
    if (!mask || !rank || !blocks || !refs || (n_sites > 0 && !pairs)) return s2c_set_error(S2C_ERR_ARG, "NULL link table buffer");
    if ((uintptr_t)pairs & 15u) return s2c_set_error(S2C_ERR_ARG, "link table pairs must be 16-byte aligned");
    a.mask = mask; a.rank = rank; a.pairs = pairs; a.blocks = blocks; a.refs = refs;
    a.n = (uint64_t)n; a.n_sites = (uint64_t)n_sites; a.min_reads = (uint64_t)min_reads;
    a.padded_len = padded_len;
    return S2C_OK;
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_links_pop(const uint64_t *mask, int64_t padded_len, uint32_t *pop, void *stream) {
    using namespace s2c;
    if (padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad link table sizes");
    if (padded_len == 0) return S2C_OK;
    if (!mask || !pop) return s2c_set_error(S2C_ERR_ARG, "NULL link table buffer");
    const int64_t n_words = (padded_len + 63) / 64;
    k_links_pop<<<walk_grid(n_words), TWG, 0, (hipStream_t)stream>>>(mask, (uint64_t)n_words, pop);
    return launched("k_links_pop");
}

extern "C" int s2c_links_count(const uint32_t *pc, const uint32_t *ops, const uint32_t *bq, const uint32_t *bx, int64_t n_pieces,
                               int64_t n_qwords, int maxdel_active, int maxdel, const uint64_t *mask, const uint32_t *rank,
                               int64_t padded_len, int64_t n_sites, uint32_t *pairs, void *stream) {
    using namespace s2c;
    if (n_pieces < 0 || n_pieces > 0xFFFFFFFFll || n_qwords < 0 || check_sizes(padded_len, n_sites))
        return s2c_set_error(S2C_ERR_ARG, "bad link table sizes");
    if (n_pieces == 0 || n_sites == 0 || padded_len == 0) return S2C_OK;
    if (!pc || !ops || !bq || !bx || !mask || !rank || !pairs) return s2c_set_error(S2C_ERR_ARG, "NULL link table buffer");
    CountArgs a;
    a.pc = pc; a.ops = ops; a.bq = bq; a.bx = bx; a.rank = rank; a.mask = mask; a.pairs = pairs;
    a.n_qwords = (uint64_t)n_qwords; a.padded_len = (uint64_t)padded_len; a.n_sites = (uint64_t)n_sites;
    a.n = (uint32_t)n_pieces;
    a.maxdel_active = maxdel_active ? 1u : 0u;
    a.maxdel = maxdel < 0 ? 0u : (uint32_t)maxdel;
    // piece_grid's workgroups, each a contiguous stretch of whole TWG-piece steps
    const int64_t steps = (n_pieces + TWG - 1) / TWG, grid0 = piece_grid(n_pieces);
    const int64_t per = (steps + grid0 - 1) / grid0 * TWG;
    a.per = (uint32_t)per;
    k_links_count<<<(unsigned)((n_pieces + per - 1) / per), TWG, 0, (hipStream_t)stream>>>(a);
    return launched("k_links_count");
}

extern "C" int s2c_links_len(const uint64_t *mask, const uint32_t *rank, int64_t padded_len, const uint32_t *pairs, int64_t n_sites,
                             const int64_t *blocks, const int64_t *refs, int64_t n, int64_t min_reads, int64_t *lens, void *stream) {
    using namespace s2c;
    LinkArgs a;
    const int rc = link_args(a, mask, rank, padded_len, pairs, n_sites, blocks, refs, n, min_reads);
    if (rc || n == 0) return rc;
    if (!lens) return s2c_set_error(S2C_ERR_ARG, "NULL link table buffer");
    k_links_len<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(a, lens);
    return launched("k_links_len");
}

extern "C" int s2c_links_write(const uint64_t *mask, const uint32_t *rank, int64_t padded_len, const uint32_t *pairs, int64_t n_sites,
                               const int64_t *blocks, const int64_t *refs, const int64_t *offs, int64_t n, int64_t min_reads,
                               uint8_t *dst, int64_t dst_len, void *stream) {
    using namespace s2c;
    LinkArgs a;
    if (dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad link table sizes");
    const int rc = link_args(a, mask, rank, padded_len, pairs, n_sites, blocks, refs, n, min_reads);
    if (rc || n == 0) return rc;
    if (!offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL link table buffer");
    k_links_write<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(a, offs, dst, dst_len);
    return launched("k_links_write");
}
