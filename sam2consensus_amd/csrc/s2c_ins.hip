// s2c_ins.hip — insertion motif tables as text, ordered and formatted on the device (--insertions).
//
// One line per distinct (position, motif) among the insertion events a batch keeps (:73-75,
// :221, :262-271), "P\tCOV\tREADS\tLEN\tMOTIF\n": the 1-based position the inserted columns
// follow (:371-372), the coverage there (the sum of the six counts, :294), the reads carrying
// exactly this motif, its length and its characters.  The kernels read what k_reads left
// (s2c_accumulate with keep_tables): per tile the hash table of the short motifs {key, count}
// and the list of long-motif events {pos, len, q}, the base planes and any counts[6][padded_len];
// they write none of them.  Tile i goes with block i of the count tables' blocks {a, b, p0}.
//
// Hash slot order and the arrival order of the atomics must not show in the bytes, so every
// tile's entries are ordered by (position; reads, falling; length; motif in -ACGNT order) — a
// total order.  One workgroup per tile, grid-strided; k_ins_len, for its tile:
//   bucket   the valid entries of both sources into their position's bucket of ent[] (HBM
//            scratch), by s2c_text.h's bucket_by_pos: an LDS histogram (2,048 bins), scanned to
//            bucket starts, a scatter (the order inside a bucket is the atomics', and nothing
//            below depends on it);
//   group    every long event counts the events of its bucket with its length and content
//            (compared through the planes, 32 bases a step): the one at the lowest slot keeps
//            the count as its reads, the others get 0 and are dead from here on;
//   rank     every live entry (reads >= min_reads) counts the live entries of its bucket that
//            come before it: its place in ord[] is the bucket's start plus that rank (the
//            dead entries' places stay holes behind the live ones);
//   scan     line lengths over ord[] in order, their exclusive 64-bit prefix sum (wg_scan) kept
//            per place, the total to lens[tile].
// No step holds entries in LDS, so no count of entries per tile is special: the work is
// Σ over positions of (entries at the position)², a handful per position in real data.
// k_ins_write walks ord[]: a lane per place writes its line's numbers and, for a short motif,
// its characters; long motifs are written by a wave each, a lane per character.  Every byte
// store is checked against the tile's range of dst.
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr uint32_t IPOS = S2C_TILE_MAX;        // positions of a tile: the histogram's bins
constexpr uint32_t HOLE = 0xFFFFFFFFu;
constexpr uint32_t ILEN_END = 1u << 24;        // motif lengths stay below 2^24 (len(SEQ))

struct InsArgs {
    const uint32_t *tiles, *ibkt, *ilong, *ilong_n, *bq, *bx, *counts;
    const int64_t *blocks;
    uint4 *ent, *ord;          // scratch: [n_bkt + n_lng] each, tile t's at boff + loff
    uint64_t n_tiles, n_bkt, n_lng, n_qwords;
    int64_t padded_len;
    uint32_t min_reads;
};

// An entry of ent[]: a short motif {key lo, key hi, reads, len} (key = pos | len << 11 | 3-bit
// codes << 16, add_event of s2c_reads.hip) or a long one {q lo, q hi | pos << 16, reads,
// len | 1 << 31} (q < 2^48: its first base in the planes).
__device__ __forceinline__ bool e_long(const uint4 &e) { return (e.w >> 31) != 0u; }
__device__ __forceinline__ uint32_t e_len(const uint4 &e) { return e.w & (ILEN_END - 1u); }
__device__ __forceinline__ uint32_t e_pos(const uint4 &e) { return e_long(e) ? (e.y >> 16) & 0x7FFu : e.x & 0x7FFu; }
__device__ __forceinline__ uint64_t e_q(const uint4 &e) { return (uint64_t)e.x | ((uint64_t)(e.y & 0xFFFFu) << 32); }
__device__ __forceinline__ uint64_t e_key(const uint4 &e) { return (uint64_t)e.x | ((uint64_t)e.y << 32); }

// the tile's part of the tables and of the scratch, or ok = false for a record outside them
struct Region {
    uint32_t boff, bcap, loff, lcap;
    uint64_t base, cap;
    bool ok;
};
__device__ __forceinline__ Region region_of(const InsArgs &d, uint64_t t) {
    const uint4 v = ((const uint4 *)d.tiles)[t * (S2C_TILE_WORDS / 4) + 1];
    Region R;
    R.boff = uni(v.x); R.bcap = uni(v.y); R.loff = uni(v.z); R.lcap = uni(v.w);
    R.base = (uint64_t)R.boff + R.loff;
    R.cap = (uint64_t)R.bcap + R.lcap;
    R.ok = (uint64_t)R.boff + R.bcap <= d.n_bkt && (uint64_t)R.loff + R.lcap <= d.n_lng;
    return R;
}

// a hash slot that holds a listable motif of a position below npos
__device__ __forceinline__ bool short_ok(const uint4 &v, uint32_t npos) {
    const uint32_t len = (v.x >> 11) & 31u;
    return (v.x | v.y) != 0u && v.z != 0u && len >= 1u && len <= S2C_SHORT_MOTIF && (v.x & 0x7FFu) < npos;
}
// a long event whose position is below npos and whose bases lie inside the planes
__device__ __forceinline__ bool long_ok(const uint4 &v, uint32_t npos, uint64_t n_qwords) {
    const uint64_t q = (uint64_t)v.z | ((uint64_t)v.w << 32);
    return v.x < npos && v.y >= 1u && v.y < ILEN_END && q < (1ull << 48) && q + v.y <= 32ull * n_qwords;
}

// "-ACGNT" index of query base q (add_event's mapping: sym_code)
__device__ __forceinline__ uint32_t plane_code(const InsArgs &d, uint64_t q) {
    const uint64_t w = q >> 5;
    const uint32_t sh = (uint32_t)(q & 31);
    return sym_code((d.bq[2 * w] >> sh) & 1u, (d.bq[2 * w + 1] >> sh) & 1u, (d.bx[w] >> sh) & 1u);
}
// symbol c of an entry's motif
__device__ __forceinline__ uint32_t e_sym(const InsArgs &d, const uint4 &e, uint32_t c) {
    return e_long(e) ? plane_code(d, e_q(e) + c) : (uint32_t)(e_key(e) >> (16u + 3u * c)) & 7u;
}

// plane bits {p0, p1, x} of the n <= 32 bases from q (inside the planes), bit k = base q + k
struct W3 {
    uint32_t p0, p1, x;
};
__device__ __forceinline__ W3 bases32(const InsArgs &d, uint64_t q, uint32_t n) {
    const uint64_t w = q >> 5;
    const uint32_t sh = (uint32_t)(q & 31);
    const bool two = sh + n > 32u;   // (then word w + 1 holds bases of the motif: inside the planes)
    const uint32_t m = n >= 32u ? 0xFFFFFFFFu : (1u << n) - 1u;
    W3 r;
    r.p0 = funnel(two ? d.bq[2 * (w + 1)] : 0u, d.bq[2 * w], sh) & m;
    r.p1 = funnel(two ? d.bq[2 * (w + 1) + 1] : 0u, d.bq[2 * w + 1], sh) & m;
    r.x = funnel(two ? d.bx[w + 1] : 0u, d.bx[w], sh) & m;
    return r;
}

// Motifs of one length compared symbol by symbol in -ACGNT order: < 0, 0, > 0
__device__ __forceinline__ int cmp_motif(const InsArgs &d, const uint4 &A, const uint4 &B, uint32_t len) {
    if (e_long(A) && e_long(B)) {
        const uint64_t qa = e_q(A), qb = e_q(B);
        for (uint32_t c = 0; c < len; c += 32u) {
            const uint32_t n = min(32u, len - c);
            const W3 a = bases32(d, qa + c, n), b = bases32(d, qb + c, n);
            const uint32_t df = (a.p0 ^ b.p0) | (a.p1 ^ b.p1) | (a.x ^ b.x);
            if (df) {
                const uint32_t k = (uint32_t)__builtin_ctz(df);
                const uint32_t ca = sym_code((a.p0 >> k) & 1u, (a.p1 >> k) & 1u, (a.x >> k) & 1u);
                const uint32_t cb = sym_code((b.p0 >> k) & 1u, (b.p1 >> k) & 1u, (b.x >> k) & 1u);
                return ca < cb ? -1 : 1;
            }
        }
        return 0;
    }
    if (!e_long(A) && !e_long(B)) {
        const uint64_t df = (e_key(A) ^ e_key(B)) >> 16;
        if (!df) return 0;
        const uint32_t c = (uint32_t)__builtin_ctzll(df) / 3u;
        return e_sym(d, A, c) < e_sym(d, B, c) ? -1 : 1;
    }
    for (uint32_t c = 0; c < len; c++) {   // (a long event of a short motif's length: hand-built tables only)
        const uint32_t ca = e_sym(d, A, c), cb = e_sym(d, B, c);
        if (ca != cb) return ca < cb ? -1 : 1;
    }
    return 0;
}

// entry J (bucket slot j) comes before entry I (slot i) of the same position
__device__ __forceinline__ bool before(const InsArgs &d, const uint4 &J, uint32_t j, const uint4 &I, uint32_t i) {
    if (J.z != I.z) return J.z > I.z;
    const uint32_t lj = e_len(J), li = e_len(I);
    if (lj != li) return lj < li;
    const int c = cmp_motif(d, J, I, li);
    if (c) return c < 0;
    return j < i;   // (equal lines: duplicate keys of a hand-built table)
}

// lens[t] = bytes of tile t's lines; ent[] and ord[] of the tile for k_ins_write
__global__ __launch_bounds__(TWG) void k_ins_len(const InsArgs d, int64_t *__restrict__ lens) {
    __shared__ uint32_t start[IPOS + 1];   // entries per position, then the buckets' starts
    __shared__ uint32_t cursor[IPOS];
    __shared__ uint64_t wsum[TWG / 64];
    __shared__ uint32_t total;
    S2C_POISON(start, sizeof(start));
    S2C_POISON(cursor, sizeof(cursor));
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t t = blockIdx.x; t < d.n_tiles; t += gridDim.x) {
        const Region R = region_of(d, t);
        if (!R.ok) {   // (a tile record outside the tables: nothing of it is touched)
            if (tid == 0) lens[t] = 0;
            continue;
        }
        const Blk B = load_blk(d.blocks, t);
        // positions of the tile that are listed: none for a block the guards refuse
        const uint32_t npos = B.ok(d.padded_len) ? (uint32_t)min((int64_t)IPOS, B.b - B.a) : 0u;
        const uint32_t nl = min(uni(d.ilong_n[t]), R.lcap);
        const uint4 *bk = (const uint4 *)d.ibkt + R.boff;
        const uint4 *lg = (const uint4 *)d.ilong + R.loff;
        uint4 *ent = d.ent + R.base, *ord = d.ord + R.base;
        const uint32_t cap = (uint32_t)min(R.cap, (uint64_t)0xFFFFFFFEu);
        // (1)-(3) the valid entries (n ≤ cap) of both sources into their position's bucket of
        // ent[]; every place of ord[] a hole
        const uint32_t n = bucket_by_pos<IPOS>(start, cursor, wsum, total, ent, tid, lane, wv, [&](auto f) {
            for (uint32_t e = tid; e < R.bcap; e += TWG) {
                const uint4 v = bk[e];
                if (short_ok(v, npos)) f(v.x & 0x7FFu, make_uint4(v.x, v.y, v.z, (v.x >> 11) & 31u));
            }
            for (uint32_t e = tid; e < nl; e += TWG) {
                const uint4 v = lg[e];
                if (long_ok(v, npos, d.n_qwords)) f(v.x, make_uint4(v.z, (v.w & 0xFFFFu) | (v.x << 16), 1u, v.y | (1u << 31)));
            }
        });
        for (uint32_t s = tid; s < cap; s += TWG) ord[s] = make_uint4(HOLE, 0u, 0u, 0u);
        wg_sync();
        // (4) equal long events of a bucket → one entry with their number as its reads
        for (uint32_t i = tid; i < n; i += TWG) {
            const uint4 I = ent[i];
            if (!e_long(I)) continue;
            const uint32_t pos = e_pos(I), len = e_len(I), s0 = start[pos], s1 = start[pos + 1];
            uint32_t same = 0, first = i;
            for (uint32_t j = s0; j < s1; j++) {
                const uint4 J = ent[j];
                if (e_long(J) && e_len(J) == len && (j == i || cmp_motif(d, J, I, len) == 0)) {
                    same++;
                    first = min(first, j);
                }
            }
            ent[i].z = first == i ? same : 0u;   // (.z is not read in this step)
        }
        wg_sync();
        // (5) the live entries' places
        for (uint32_t i = tid; i < n; i += TWG) {
            const uint4 I = ent[i];
            if (I.z < d.min_reads) continue;
            const uint32_t pos = e_pos(I), s0 = start[pos], s1 = start[pos + 1];
            uint32_t r = 0;
            for (uint32_t j = s0; j < s1; j++) {
                if (j == i) continue;
                const uint4 J = ent[j];
                r += (J.z >= d.min_reads && before(d, J, j, I, i)) ? 1u : 0u;
            }
            ord[s0 + r].x = i;
        }
        wg_sync();
        // (6) line lengths in order, their exclusive prefix sum
        uint64_t run = 0;
        for (uint32_t s0 = 0; s0 < n; s0 += TWG) {
            const uint32_t s = s0 + tid;
            const uint32_t i = s < n ? ord[s].x : HOLE;
            uint32_t len = 0;
            if (i != HOLE) {
                const uint4 E = ent[i];
                const uint32_t pos = e_pos(E);
                len = ndig64((uint64_t)B.p0 + pos) + ndig64(cov_at(d.counts, (uint64_t)d.padded_len, (uint64_t)B.a + pos)) + ndig32(E.z) +
                      ndig32(e_len(E)) + e_len(E) + 5u;   // (< 2^24 + 64: a wave's sum fits 32 bits)
            }
            uint64_t tot;
            const uint64_t end = wg_scan(len, wsum, lane, wv, tot);
            if (i != HOLE) {
                const uint64_t off = run + end - len;
                ord[s] = make_uint4(i, (uint32_t)off, (uint32_t)(off >> 32), len);
            }
            run += tot;
            lds_sync();   // (wsum is written again)
        }
        if (tid == 0) lens[t] = (int64_t)run;
        wg_sync();   // (start, cursor and total are written again for the next tile)
    }
}

// tile i's lines → dst[offs[i], offs[i+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_ins_write(const InsArgs d, const int64_t *__restrict__ offs,
                                                    uint8_t *__restrict__ dst, int64_t dst_len) {
    __shared__ uint32_t nlist;
    __shared__ uint32_t list[TWG];      // the sub-block's long motifs: their places in ord[]
    S2C_POISON(list, sizeof(list));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t t = blockIdx.x; t < d.n_tiles; t += gridDim.x) {
        const Region R = region_of(d, t);
        const Blk B = load_blk(d.blocks, t);
        const int64_t d0 = offs[t], d1 = offs[t + 1];
        if (!R.ok || !B.ok(d.padded_len) || d0 < 0 || d1 < d0 || d1 > dst_len) continue;
        const Out o{dst + d0, (uint64_t)(d1 - d0)};
        const uint4 *ent = d.ent + R.base, *ord = d.ord + R.base;
        const uint32_t cap = (uint32_t)min(R.cap, (uint64_t)0xFFFFFFFEu);
        for (uint32_t s0 = 0; s0 < cap; s0 += TWG) {
            if (tid == 0) nlist = 0u;
            lds_sync();
            const uint32_t s = s0 + tid;
            const uint4 O = s < cap ? ord[s] : make_uint4(HOLE, 0u, 0u, 0u);
            if (O.x != HOLE && O.x < cap) {
                const uint4 E = ent[O.x];
                const uint32_t pos = e_pos(E), len = e_len(E);
                const uint64_t off = (uint64_t)O.y | ((uint64_t)O.z << 32);
                uint64_t e = off + O.w - 1u - len;   // the byte after the tab before the motif
                o.put(--e, '\t');
                e = put32(o, e, len);
                o.put(--e, '\t');
                e = put32(o, e, E.z);
                o.put(--e, '\t');
                e = put64(o, e, pos < (uint32_t)(B.b - B.a) ? cov_at(d.counts, (uint64_t)d.padded_len, (uint64_t)B.a + pos) : 0ull);
                o.put(--e, '\t');
                put64(o, e, (uint64_t)B.p0 + pos);
                if (e_long(E)) {
                    list[atomicAdd(&nlist, 1u)] = s;
                } else {
                    const uint64_t m = off + O.w - 1u - len, key = e_key(E) >> 16;
                    for (uint32_t c = 0; c < len; c++) o.put(m + c, sym_char((uint32_t)(key >> (3u * c)) & 7u));
                    o.put(m + len, '\n');
                }
            }
            lds_sync();
            // the long motifs: a wave each, a lane per character
            const uint32_t nlg = nlist;
            for (uint32_t k = wv; k < nlg; k += TWG / 64) {
                const uint4 O2 = ord[list[k]];
                const uint4 E = ent[O2.x];
                const uint32_t len = e_len(E);
                const uint64_t q = e_q(E), m = ((uint64_t)O2.y | ((uint64_t)O2.z << 32)) + O2.w - 1u - len;
                if (q + len <= 32ull * d.n_qwords)
                    for (uint32_t c = lane; c < len; c += 64u) o.put(m + c, sym_char(plane_code(d, q + c)));
                if (lane == 0) o.put(m + len, '\n');
            }
            lds_sync();   // (nlist and list are written again)
        }
    }
}

int check_args(const uint32_t *tiles, int64_t n_tiles, int64_t n_bkt, int64_t n_lng, int64_t n_qwords, int64_t padded_len) {
    if (n_tiles < 0 || n_bkt < 0 || n_lng < 0 || n_qwords < 0 || padded_len < 0 || n_bkt >= (1ll << 32) || n_lng >= (1ll << 32))
        return s2c_set_error(S2C_ERR_ARG, "bad insertion table sizes");
    if (n_tiles > 0 && !tiles) return s2c_set_error(S2C_ERR_ARG, "NULL insertion table buffer");
    return S2C_OK;
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_ins_len(const uint32_t *tiles, int64_t n_tiles, const uint32_t *ibkt, int64_t n_bkt,
                           const uint32_t *ilong, int64_t n_lng, const uint32_t *ilong_n, const uint32_t *bq,
                           const uint32_t *bx, int64_t n_qwords, const uint32_t *counts, int64_t padded_len,
                           const int64_t *blocks, int64_t min_reads, uint32_t *scratch, int64_t *lens, void *stream) {
    using namespace s2c;
    int rc = check_args(tiles, n_tiles, n_bkt, n_lng, n_qwords, padded_len);
    if (rc) return rc;
    if (min_reads < 1 || min_reads > 0xFFFFFFFFll) return s2c_set_error(S2C_ERR_ARG, "insertion tables: 1 <= min_reads < 2^32");
    if (n_tiles == 0) return S2C_OK;
    if (!ibkt || !ilong || !ilong_n || !bq || !bx || !counts || !blocks || !scratch || !lens)
        return s2c_set_error(S2C_ERR_ARG, "NULL insertion table buffer");
    if ((uintptr_t)scratch & 15u) return s2c_set_error(S2C_ERR_ARG, "insertion table scratch must be 16-byte aligned");
    InsArgs a;
    a.tiles = tiles; a.ibkt = ibkt; a.ilong = ilong; a.ilong_n = ilong_n; a.bq = bq; a.bx = bx; a.counts = counts;
    a.blocks = blocks;
    a.ent = (uint4 *)scratch;
    a.ord = a.ent + (n_bkt + n_lng);
    a.n_tiles = (uint64_t)n_tiles; a.n_bkt = (uint64_t)n_bkt; a.n_lng = (uint64_t)n_lng; a.n_qwords = (uint64_t)n_qwords;
    a.padded_len = padded_len;
    a.min_reads = (uint32_t)min_reads;
    k_ins_len<<<text_grid(n_tiles), TWG, 0, (hipStream_t)stream>>>(a, lens);
    return launched("k_ins_len");
}

extern "C" int s2c_ins_write(const uint32_t *tiles, int64_t n_tiles, int64_t n_bkt, int64_t n_lng, const uint32_t *bq,
                             const uint32_t *bx, int64_t n_qwords, const uint32_t *counts, int64_t padded_len,
                             const int64_t *blocks, const uint32_t *scratch, const int64_t *offs, uint8_t *dst,
                             int64_t dst_len, void *stream) {
    using namespace s2c;
    int rc = check_args(tiles, n_tiles, n_bkt, n_lng, n_qwords, padded_len);
    if (rc) return rc;
    if (dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad insertion table sizes");
    if (n_tiles == 0) return S2C_OK;
    if (!bq || !bx || !counts || !blocks || !scratch || !offs || !dst)
        return s2c_set_error(S2C_ERR_ARG, "NULL insertion table buffer");
    if ((uintptr_t)scratch & 15u) return s2c_set_error(S2C_ERR_ARG, "insertion table scratch must be 16-byte aligned");
    InsArgs a;
    a.tiles = tiles; a.ibkt = nullptr; a.ilong = nullptr; a.ilong_n = nullptr; a.bq = bq; a.bx = bx; a.counts = counts;
    a.blocks = blocks;
    a.ent = (uint4 *)scratch;
    a.ord = a.ent + (n_bkt + n_lng);
    a.n_tiles = (uint64_t)n_tiles; a.n_bkt = (uint64_t)n_bkt; a.n_lng = (uint64_t)n_lng; a.n_qwords = (uint64_t)n_qwords;
    a.padded_len = padded_len;
    a.min_reads = 1u;
    k_ins_write<<<text_grid(n_tiles), TWG, 0, (hipStream_t)stream>>>(a, offs, dst, dst_len);
    return launched("k_ins_write");
}
