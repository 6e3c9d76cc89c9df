// s2c_dels.hip — the gap events that fragments carry, merged and formatted on the device (--deletions).
//
// A fragment is a piece of the batch, seqout[ka, kb) of its read (for a read over maxdel the host
// cut [ka, kb) to its first and last counted character, :210).  A gap character is a character
// of seqout that a D, N or P token produced (:70-72); an event is a maximal run of consecutive
// gap characters inside one fragment: tokens that add nothing to seqout (I, S, H, an M after SEQ
// ran out) do not split it, a base does, a '-' of SEQ does too.  One line per distinct (start,
// length), "REF\tSTART\tEND\tLEN\tREADS\tDROPPED\tCOV\n": the fragments that carry exactly this
// event, those among them whose '-' the maxdel rule kept out of the counts, and the sum of the
// six counts at START.
//
// Six launches.
//   k_dels_count    one lane per piece walks its tokens and counts its events; the total E (one
//                   8-byte read of the host) sizes what follows.
//   k_dels_collect  the same walk adds every event to an open-addressing table of 16-byte slots
//                   {g, len, reads, dropped} in HBM: the 64-bit key (g, len) is claimed with a
//                   compare-and-swap (len >= 1: zero is the empty slot), the counts are integer
//                   adds, so nothing depends on the order of arrival.  Probing is bounded by the
//                   slot count; a table that fills sets the overflow word.
//   k_dels_tiles / k_dels_scatter   the slots to their tile (wtile[g >> 5]): per-tile counts, the
//                   caller's exclusive prefix sum, a scatter into ent[].
//   k_dels_len      one workgroup per tile: the listed entries (reads >= min_reads, g inside the
//                   tile's block) into their position's bucket of tmp[] (s2c_text.h's
//                   bucket_by_pos), each one's rank in its bucket the entries of a smaller length (they
//                   are distinct by now: the quadratic term is over the lengths at one start),
//                   the ordered entries written back over the tile's part of ent[], their line
//                   lengths summed to lens[tile].
//   k_dels_write    TWG ordered entries a step, a lane a line, through s2c_text.h's
//                   emit_var_lines: the lines leave through an LDS image when the step's bytes
//                   fit it, and byte by byte through the tile's guarded range of dst when they do
//                   not (a reference name can be of any length).
// The maxdel rule behind the DROPPED column is s2c_common.h's piece_dashes, the count walk's own.
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr uint32_t DPOS = S2C_TILE_MAX;    // positions of a tile: the histogram's bins

struct WalkArgs {
    const uint32_t *pc, *ops, *bq, *bx;
    uint64_t n_ops, n_qwords, padded_len;
    uint32_t n, maxdel_active, maxdel;
    unsigned long long *total;   // k_dels_count
    uint4 *slots;                // k_dels_collect
    uint64_t n_slots;
    uint32_t hbits;              // n_slots = 1 << hbits
    uint32_t *overflow;
};

// where piece P's CIGAR tokens start (behind its prefix words) and its range of seqout;
// false for a piece without events (one M token) or whose prefix words lie outside the op words
__device__ __forceinline__ bool piece_tokens(const WalkArgs &d, const uint4 &P, uint64_t oend, uint64_t &o, int64_t &ka, int64_t &kb) {
    const uint32_t fl = P.w >> 24;
    if (fl & S2C_PF_SIMPLE) return false;
    o = P.z;
    ka = 0;
    kb = INT64_MAX;
    const uint64_t pre = ((fl & S2C_PF_RANGE) ? 2u : 0u) + ((fl & S2C_PF_INS) ? 3u : 0u);
    if (o + pre > oend) return false;
    if (fl & S2C_PF_RANGE) {
        ka = d.ops[o];
        kb = d.ops[o + 1];
    }
    o += pre;
    return true;
}

// The gap events of piece i in rising position, ev(g, len) for each: the D / N / P parts inside
// [ka, kb) merged by contiguity in g — a part whose first position continues the pending run
// extends it, anything else flushes it (a base between two gaps moves k on, so the next part
// is not contiguous; I, S, H and an M that takes nothing do not).  Returns the events.
template <class EvFn>
__device__ __forceinline__ uint32_t piece_events(const WalkArgs &d, uint64_t i, EvFn &&ev) {
    const uint4 P = ((const uint4 *)d.pc)[i];
    const uint64_t oend = min((uint64_t)d.pc[4 * i + 6], d.n_ops);   // next piece's opoff (sentinel at the end)
    const uint32_t slen = P.w & 0xFFFFFFu;
    uint64_t o;
    int64_t ka, kb;
    if (!piece_tokens(d, P, oend, o, ka, kb)) return 0u;
    int64_t k = 0;
    uint64_t start = 0, pg = 0, pl = 0;   // the pending run [pg, pg + pl)
    uint32_t n = 0;
    for (uint64_t j = o; j < oend; j++) {
        const uint32_t w = d.ops[j], op = w & 15u;
        const uint64_t l = w >> 4;
        if (op_bases(op)) {
            k += (int64_t)(start < slen ? (l < slen - start ? l : slen - start) : 0);
            start += l;
        } else if (op_dash(op)) {
            const int64_t s = k > ka ? k : ka, e = (k + (int64_t)l) < kb ? k + (int64_t)l : kb;
            if (e > s) {
                const uint64_t g = (uint64_t)P.x + (uint64_t)(s - ka);
                if (pl && g == pg + pl) {
                    pl += (uint64_t)(e - s);
                } else {
                    if (pl) { ev(pg, pl); n++; }
                    pg = g;
                    pl = (uint64_t)(e - s);
                }
            }
            k += (int64_t)l;
        } else if (op == S2C_OP_I || op == S2C_OP_S) {
            start += l;
        }
    }
    if (pl) { ev(pg, pl); n++; }
    return n;
}

// piece_dashes' view of a batch whose planes this file does not trust: a plane word at or past
// n_qwords reads as zero (no '-' there)
struct GuardedMem {
    const uint32_t *ops, *bq, *bx;
    uint64_t n_qwords;
    __device__ __forceinline__ uint32_t op(uint32_t j) const { return ops[j]; }
    __device__ __forceinline__ uint32_t p0(uint64_t w) const { return w < n_qwords ? bq[2 * w] : 0u; }
    __device__ __forceinline__ uint32_t p1(uint64_t w) const { return w < n_qwords ? bq[2 * w + 1] : 0u; }
    __device__ __forceinline__ uint32_t x(uint64_t w) const { return w < n_qwords ? bx[w] : 0u; }
};

// the maxdel rule (:210) for piece i's read, by the count walk's own piece_dashes: more than
// maxdel '-' in its seqout (the tokens end at n_ops at the latest, so their indices fit 32 bits)
__device__ __forceinline__ bool piece_dropped(const WalkArgs &d, uint64_t i) {
    const uint4 P = ((const uint4 *)d.pc)[i];
    const uint64_t oend = min((uint64_t)d.pc[4 * i + 6], d.n_ops);
    uint64_t o;
    int64_t ka, kb;
    if (!piece_tokens(d, P, oend, o, ka, kb)) return false;
    return piece_dashes(GuardedMem{d.ops, d.bq, d.bx, d.n_qwords}, (uint32_t)o, (uint32_t)oend, P.w & 0xFFFFFFu, P.w >> 24,
                        (uint64_t)P.y * 16) > (uint64_t)d.maxdel;
}

// an event clamped to padded_len: false when nothing of it is left
__device__ __forceinline__ bool clamp_event(const WalkArgs &d, uint64_t g, uint64_t &len) {
    if (g >= d.padded_len) return false;
    len = min(len, d.padded_len - g);   // (padded_len < 2^32: both fit 32 bits)
    return len != 0;
}

// (one add to *total per workgroup, and 8 workgroups a CU: adds to one address from all over the
// device serialise — with an add per wave, 32,768 waves, they were most of the kernel's time)
__global__ __launch_bounds__(TWG) void k_dels_count(const WalkArgs d) {
    __shared__ uint64_t wsum[TWG / 64];
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    uint64_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * TWG + threadIdx.x; i < d.n; i += (uint64_t)gridDim.x * TWG)
        piece_events(d, i, [&](uint64_t g, uint64_t len) { mine += clamp_event(d, g, len) ? 1u : 0u; });
    mine = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = mine;
    lds_sync();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < TWG / 64; w++) t += wsum[w];
        if (t) atomicAdd(d.total, (unsigned long long)t);
    }
}

// slots[(g, len)] += {1, drop}: the key claimed with a 64-bit compare-and-swap, at most n_slots probes
__device__ __forceinline__ void add_event(const WalkArgs &d, uint64_t g, uint64_t len, uint32_t drop) {
    if (!clamp_event(d, g, len)) return;
    const unsigned long long key = g | (len << 32);
    uint64_t s = d.hbits ? (key * 0x9E3779B97F4A7C15ull) >> (64u - d.hbits) : 0ull;
    for (uint64_t probe = 0; probe < d.n_slots; probe++) {
        uint4 *slot = d.slots + s;
        unsigned long long prev = __hip_atomic_load((unsigned long long *)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0ull) prev = atomicCAS((unsigned long long *)slot, 0ull, key);
        if (prev == 0ull || prev == key) {
            atomicAdd(&slot->z, 1u);
            if (drop) atomicAdd(&slot->w, 1u);
            return;
        }
        s = (s + 1u) & (d.n_slots - 1u);
    }
    atomicOr(d.overflow, 1u);   // (too few slots: the caller raises)
}

__global__ __launch_bounds__(TWG) void k_dels_collect(const WalkArgs d) {
    for (uint64_t i = (uint64_t)blockIdx.x * TWG + threadIdx.x; i < d.n; i += (uint64_t)gridDim.x * TWG) {
        // (the rule is asked only for a piece with events: most pieces have none)
        const uint32_t n = piece_events(d, i, [](uint64_t, uint64_t) {});
        if (!n) continue;
        const uint32_t drop = (d.maxdel_active && piece_dropped(d, i)) ? 1u : 0u;
        piece_events(d, i, [&](uint64_t g, uint64_t len) { add_event(d, g, len, drop); });
    }
}

// the tile of a slot that holds an entry: len >= 1, its word inside wtile, a tile below n_tiles
__device__ __forceinline__ bool slot_tile(const uint4 &v, const uint32_t *__restrict__ wtile, uint64_t n_words, uint64_t n_tiles,
                                          uint32_t &t) {
    if (v.y == 0u) return false;
    const uint64_t w = v.x >> 5;
    if (w >= n_words) return false;
    t = wtile[w];
    return (uint64_t)t < n_tiles;
}

__global__ __launch_bounds__(TWG) void k_dels_tiles(const uint4 *__restrict__ slots, uint64_t n_slots, const uint32_t *__restrict__ wtile,
                                                    uint64_t n_words, uint64_t n_tiles, uint32_t *__restrict__ tcount) {
    for (uint64_t s = (uint64_t)blockIdx.x * TWG + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * TWG) {
        const uint4 v = slots[s];
        uint32_t t;
        if (slot_tile(v, wtile, n_words, n_tiles, t)) atomicAdd(&tcount[t], 1u);
    }
}

__global__ __launch_bounds__(TWG) void k_dels_scatter(const uint4 *__restrict__ slots, uint64_t n_slots, const uint32_t *__restrict__ wtile,
                                                      uint64_t n_words, uint64_t n_tiles, const int64_t *__restrict__ tstart,
                                                      uint32_t *__restrict__ cursor, uint4 *__restrict__ ent, int64_t n_ent) {
    for (uint64_t s = (uint64_t)blockIdx.x * TWG + threadIdx.x; s < n_slots; s += (uint64_t)gridDim.x * TWG) {
        const uint4 v = slots[s];
        uint32_t t;
        if (!slot_tile(v, wtile, n_words, n_tiles, t)) continue;
        const int64_t t0 = tstart[t], t1 = tstart[t + 1];
        if (t0 < 0 || t1 < t0 || t1 > n_ent) continue;
        const int64_t at = t0 + (int64_t)atomicAdd(&cursor[t], 1u);
        if (at < t1) ent[at] = v;
    }
}

struct DelArgs {
    uint4 *ent, *tmp;          // [n_ent] each: tile t's entries at [tstart[t], tstart[t+1])
    const int64_t *tstart;
    uint32_t *tn;              // [n_tiles] the listed entries of a tile, in order at the front of its part of ent[]
    const uint32_t *tiles, *counts;
    const int64_t *blocks, *nametab;
    const uint8_t *names;
    uint64_t n_tiles, n_refs;
    int64_t n_ent, names_len, padded_len;
    uint32_t min_reads;
};

// what the two passes know of a tile: its entries [t0, t0 + cap), its block, its reference's
// name; npos = 0 (nothing listed) for a tile whose record, block or name the guards refuse
struct Tile {
    int64_t t0;
    uint32_t cap, npos, nlen;
    Blk B;
    const uint8_t *name;
};
__device__ __forceinline__ Tile tile_of(const DelArgs &d, uint64_t t) {
    Tile T{};
    const int64_t t0 = d.tstart[t], t1 = d.tstart[t + 1];
    T.B = load_blk(d.blocks, t);
    if (t0 < 0 || t1 < t0 || t1 > d.n_ent || t1 - t0 > 0xFFFFFFFEll) return T;
    T.t0 = t0;
    T.cap = (uint32_t)(t1 - t0);
    const uint64_t ref = d.tiles[t * S2C_TILE_WORDS + 2];
    if (ref >= d.n_refs || !T.B.ok(d.padded_len)) return T;
    const int64_t noff = d.nametab[2 * ref], nlen = d.nametab[2 * ref + 1];
    if (noff < 0 || nlen < 0 || nlen > 0x7FFFFFFFll || noff > d.names_len - nlen) return T;
    T.name = d.names + noff;
    T.nlen = (uint32_t)nlen;
    T.npos = (uint32_t)min((int64_t)DPOS, T.B.b - T.B.a);
    return T;
}
// an entry of tile T that is listed: an event of reads >= min_reads that starts inside the block
__device__ __forceinline__ bool listed(const DelArgs &d, const Tile &T, const uint4 &v) {
    return v.y >= 1u && v.z >= d.min_reads && (int64_t)v.x >= T.B.a && (int64_t)v.x - T.B.a < (int64_t)T.npos;
}

struct Line {
    uint64_t start, end, cov;
    uint32_t glen, reads, dropped, len;   // len == 0: no line
};
__device__ __forceinline__ Line line_of(const DelArgs &d, const Tile &T, const uint4 &v) {
    Line L{};
    L.start = (uint64_t)T.B.p0 + ((uint64_t)v.x - (uint64_t)T.B.a);
    L.end = L.start + v.y - 1u;
    L.cov = cov_at(d.counts, (uint64_t)d.padded_len, v.x);
    L.glen = v.y; L.reads = v.z; L.dropped = v.w;
    L.len = T.nlen + ndig64(L.start) + ndig64(L.end) + ndig32(L.glen) + ndig32(L.reads) + ndig32(L.dropped) + ndig64(L.cov) + 7u;
    return L;
}

// the line at o[at, at + L.len): the name forwards, the numbers backwards from the line's end
template <typename Dst>
__device__ __forceinline__ void put_line(const Dst &o, uint64_t at, const Tile &T, const Line &L) {
    for (uint32_t c = 0; c < T.nlen; c++) o.put(at + c, T.name[c]);
    uint64_t e = at + L.len;
    o.put(--e, '\n');
    e = put64(o, e, L.cov);
    o.put(--e, '\t');
    e = put32(o, e, L.dropped);
    o.put(--e, '\t');
    e = put32(o, e, L.reads);
    o.put(--e, '\t');
    e = put32(o, e, L.glen);
    o.put(--e, '\t');
    e = put64(o, e, L.end);
    o.put(--e, '\t');
    e = put64(o, e, L.start);
    o.put(--e, '\t');
}

// lens[t] = bytes of tile t's lines; its listed entries in order at the front of its part of ent[], tn[t] of them
__global__ __launch_bounds__(TWG) void k_dels_len(const DelArgs d, int64_t *__restrict__ lens) {
    __shared__ uint32_t start[DPOS + 1];   // entries per position, then the buckets' starts
    __shared__ uint32_t cursor[DPOS];
    __shared__ uint64_t wsum[TWG / 64];
    __shared__ uint32_t total;
    S2C_POISON(start, sizeof(start));
    S2C_POISON(cursor, sizeof(cursor));
    S2C_POISON(wsum, sizeof(wsum));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t t = blockIdx.x; t < d.n_tiles; t += gridDim.x) {
        const Tile T = tile_of(d, t);
        if (!T.cap || !T.npos) {   // (no entry, or a tile the guards refuse: nothing of it is touched)
            if (tid == 0) {
                lens[t] = 0;
                d.tn[t] = 0u;
            }
            continue;
        }
        uint4 *ent = d.ent + T.t0, *tmp = d.tmp + T.t0;
        // (1)-(3) the listed entries (n ≤ cap) into their position's bucket of tmp[]
        const uint32_t n = bucket_by_pos<DPOS>(start, cursor, wsum, total, tmp, tid, lane, wv, [&](auto f) {
            for (uint32_t e = tid; e < T.cap; e += TWG) {
                const uint4 v = ent[e];
                if (listed(d, T, v)) f((uint32_t)((int64_t)v.x - T.B.a), v);
            }
        });
        wg_sync();   // (ent[] is read no more: the ordered entries go back over it)
        // (4) every entry's place: its bucket's start plus the entries of a smaller length
        for (uint32_t i = tid; i < n; i += TWG) {
            const uint4 I = tmp[i];
            const uint32_t pos = (uint32_t)((int64_t)I.x - T.B.a), s0 = start[pos], s1 = start[pos + 1];
            uint32_t r = 0;
            for (uint32_t j = s0; j < s1; j++) {
                const uint32_t lj = tmp[j].y;
                r += (lj < I.y || (lj == I.y && j < i)) ? 1u : 0u;   // (equal keys: a hand-built table only)
            }
            ent[s0 + r] = I;
        }
        wg_sync();
        // (5) line lengths
        uint64_t sum = 0;
        for (uint32_t i = tid; i < n; i += TWG) sum += line_of(d, T, ent[i]).len;
        if (tid == 0) d.tn[t] = n;
        block_total(sum, wsum, tid, &lens[t]);
        wg_sync();   // (start, cursor and total are written again for the next tile)
    }
}

// tile t's lines → dst[offs[t], offs[t+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_dels_write(const DelArgs d, const int64_t *__restrict__ offs, uint8_t *__restrict__ dst,
                                                     int64_t dst_len) {
    __shared__ alignas(16) uint8_t buf[LIMG + 16];
    __shared__ uint32_t wtot[TWG / 64];   // wave totals of the line lengths
    S2C_POISON(buf, sizeof(buf));
    S2C_POISON(wtot, sizeof(wtot));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t t = blockIdx.x; t < d.n_tiles; t += gridDim.x) {
        const Tile T = tile_of(d, t);
        const int64_t d0 = offs[t], d1 = offs[t + 1];
        if (!T.cap || !T.npos || d0 < 0 || d1 < d0 || d1 > dst_len) continue;
        const uint32_t n = min(d.tn[t], T.cap);
        const Out o{dst + d0, (uint64_t)(d1 - d0)};
        const uint4 *ent = d.ent + T.t0;
        uint64_t run = 0;   // bytes of the tile's lines so far
        for (uint32_t s0 = 0; s0 < n; s0 += TWG) {
            lds_sync();   // (wtot and buf are no longer read)
            Line L{};
            if (s0 + tid < n) {
                const uint4 v = ent[s0 + tid];
                if (listed(d, T, v)) L = line_of(d, T, v);
            }
            run += emit_var_lines<LIMG>(buf, wtot, o, run, L.len, tid, lane, wv, [&](const auto &to, uint64_t at) { put_line(to, at, T, L); });
        }
    }
}

int walk_args(WalkArgs &a, const uint32_t *pc, const uint32_t *ops, int64_t n_pieces, int64_t n_ops, int64_t padded_len) {
    if (n_pieces < 0 || n_pieces > 0xFFFFFFFFll || n_ops < 0 || padded_len < 0 || padded_len > 0xFFFFFFFFll)
        return s2c_set_error(S2C_ERR_ARG, "bad deletion table sizes");
    a = WalkArgs{};
    a.pc = pc; a.ops = ops;
    a.n = (uint32_t)n_pieces; a.n_ops = (uint64_t)n_ops; a.padded_len = (uint64_t)padded_len;
    return S2C_OK;
}

int bucket_sizes(int64_t n_slots, int64_t n_words, int64_t n_tiles) {
    if (n_slots < 0 || n_slots > (1ll << 40) || n_words < 0 || n_tiles < 0 || n_tiles > 0xFFFFFFFFll)
        return s2c_set_error(S2C_ERR_ARG, "bad deletion table sizes");
    return S2C_OK;
}

int del_args(DelArgs &a, const uint32_t *ent, int64_t n_ent, const int64_t *tstart, const uint32_t *tn, const uint32_t *tiles,
             int64_t n_tiles, const int64_t *blocks, const uint8_t *names, int64_t names_len, const int64_t *nametab, int64_t n_refs,
             const uint32_t *counts, int64_t padded_len) {
    if (n_ent < 0 || n_ent > 0xFFFFFFFFll || n_tiles < 0 || names_len < 0 || n_refs < 0 || padded_len < 0)
        return s2c_set_error(S2C_ERR_ARG, "bad deletion table sizes");
    if (n_tiles == 0) return S2C_OK;
    if (!ent || !tstart || !tn || !tiles || !blocks || !names || !nametab || !counts)
        return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    if ((uintptr_t)ent & 15u) return s2c_set_error(S2C_ERR_ARG, "deletion table entries must be 16-byte aligned");
    a = DelArgs{};
    a.ent = (uint4 *)ent; a.tstart = tstart; a.tn = (uint32_t *)tn; a.tiles = tiles; a.counts = counts;
    a.blocks = blocks; a.nametab = nametab; a.names = names;
    a.n_tiles = (uint64_t)n_tiles; a.n_refs = (uint64_t)n_refs;
    a.n_ent = n_ent; a.names_len = names_len; a.padded_len = padded_len;
    a.min_reads = 1u;
    return S2C_OK;
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_dels_count(const uint32_t *pc, const uint32_t *ops, int64_t n_pieces, int64_t n_ops, int64_t padded_len,
                              uint64_t *n_events, void *stream) {
    using namespace s2c;
    WalkArgs a;
    const int rc = walk_args(a, pc, ops, n_pieces, n_ops, padded_len);
    if (rc) return rc;
    if (n_pieces == 0 || padded_len == 0) return S2C_OK;
    if (!pc || !ops || !n_events) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    a.total = (unsigned long long *)n_events;
    k_dels_count<<<piece_grid(n_pieces), TWG, 0, (hipStream_t)stream>>>(a);
    return launched("k_dels_count");
}

extern "C" int s2c_dels_collect(const uint32_t *pc, const uint32_t *ops, const uint32_t *bq, const uint32_t *bx, int64_t n_pieces,
                                int64_t n_ops, int64_t n_qwords, int maxdel_active, int maxdel, int64_t padded_len, uint32_t *slots,
                                int64_t n_slots, uint32_t *overflow, void *stream) {
    using namespace s2c;
    WalkArgs a;
    const int rc = walk_args(a, pc, ops, n_pieces, n_ops, padded_len);
    if (rc) return rc;
    if (n_qwords < 0 || n_slots < 1 || n_slots > (1ll << 40) || (n_slots & (n_slots - 1)))
        return s2c_set_error(S2C_ERR_ARG, "deletion tables: the slots are a power of two");
    if (n_pieces == 0 || padded_len == 0) return S2C_OK;
    if (!pc || !ops || !bq || !bx || !slots || !overflow) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    if ((uintptr_t)slots & 15u) return s2c_set_error(S2C_ERR_ARG, "deletion table slots must be 16-byte aligned");
    a.bq = bq; a.bx = bx; a.n_qwords = (uint64_t)n_qwords;
    a.maxdel_active = maxdel_active ? 1u : 0u;
    a.maxdel = maxdel < 0 ? 0u : (uint32_t)maxdel;
    a.slots = (uint4 *)slots; a.n_slots = (uint64_t)n_slots; a.overflow = overflow;
    a.hbits = 0;
    while ((1ll << a.hbits) < n_slots) a.hbits++;
    k_dels_collect<<<piece_grid(n_pieces), TWG, 0, (hipStream_t)stream>>>(a);
    return launched("k_dels_collect");
}

extern "C" int s2c_dels_tiles(const uint32_t *slots, int64_t n_slots, const uint32_t *wtile, int64_t n_words, int64_t n_tiles,
                              uint32_t *tcount, void *stream) {
    using namespace s2c;
    const int rc = bucket_sizes(n_slots, n_words, n_tiles);
    if (rc) return rc;
    if (n_slots == 0 || n_words == 0 || n_tiles == 0) return S2C_OK;
    if (!slots || !wtile || !tcount) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    if ((uintptr_t)slots & 15u) return s2c_set_error(S2C_ERR_ARG, "deletion table slots must be 16-byte aligned");
    k_dels_tiles<<<walk_grid(n_slots), TWG, 0, (hipStream_t)stream>>>((const uint4 *)slots, (uint64_t)n_slots, wtile, (uint64_t)n_words,
                                                                    (uint64_t)n_tiles, tcount);
    return launched("k_dels_tiles");
}

extern "C" int s2c_dels_scatter(const uint32_t *slots, int64_t n_slots, const uint32_t *wtile, int64_t n_words, int64_t n_tiles,
                                const int64_t *tstart, uint32_t *cursor, uint32_t *ent, int64_t n_ent, void *stream) {
    using namespace s2c;
    const int rc = bucket_sizes(n_slots, n_words, n_tiles);
    if (rc) return rc;
    if (n_ent < 0 || n_ent > 0xFFFFFFFFll) return s2c_set_error(S2C_ERR_ARG, "bad deletion table sizes");
    if (n_slots == 0 || n_words == 0 || n_tiles == 0 || n_ent == 0) return S2C_OK;
    if (!slots || !wtile || !tstart || !cursor || !ent) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    if (((uintptr_t)slots | (uintptr_t)ent) & 15u) return s2c_set_error(S2C_ERR_ARG, "deletion table slots and entries must be 16-byte aligned");
    k_dels_scatter<<<walk_grid(n_slots), TWG, 0, (hipStream_t)stream>>>((const uint4 *)slots, (uint64_t)n_slots, wtile, (uint64_t)n_words,
                                                                      (uint64_t)n_tiles, tstart, cursor, (uint4 *)ent, n_ent);
    return launched("k_dels_scatter");
}

extern "C" int s2c_dels_len(uint32_t *ent, uint32_t *tmp, int64_t n_ent, const int64_t *tstart, const uint32_t *tiles, int64_t n_tiles,
                            const int64_t *blocks, const uint8_t *names, int64_t names_len, const int64_t *nametab, int64_t n_refs,
                            const uint32_t *counts, int64_t padded_len, int64_t min_reads, uint32_t *tn, int64_t *lens, void *stream) {
    using namespace s2c;
    DelArgs a;
    const int rc = del_args(a, ent, n_ent, tstart, tn, tiles, n_tiles, blocks, names, names_len, nametab, n_refs, counts, padded_len);
    if (rc) return rc;
    if (min_reads < 1 || min_reads > 0xFFFFFFFFll) return s2c_set_error(S2C_ERR_ARG, "deletion tables: 1 <= min_reads < 2^32");
    if (n_tiles == 0) return S2C_OK;
    if (!tmp || !lens) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    if ((uintptr_t)tmp & 15u) return s2c_set_error(S2C_ERR_ARG, "deletion table entries must be 16-byte aligned");
    a.tmp = (uint4 *)tmp;
    a.min_reads = (uint32_t)min_reads;
    k_dels_len<<<text_grid(n_tiles), TWG, 0, (hipStream_t)stream>>>(a, lens);
    return launched("k_dels_len");
}

extern "C" int s2c_dels_write(const uint32_t *ent, int64_t n_ent, const int64_t *tstart, const uint32_t *tn, const uint32_t *tiles,
                              int64_t n_tiles, const int64_t *blocks, const uint8_t *names, int64_t names_len, const int64_t *nametab,
                              int64_t n_refs, const uint32_t *counts, int64_t padded_len, const int64_t *offs, uint8_t *dst,
                              int64_t dst_len, void *stream) {
    using namespace s2c;
    DelArgs a;
    if (dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad deletion table sizes");
    const int rc = del_args(a, ent, n_ent, tstart, tn, tiles, n_tiles, blocks, names, names_len, nametab, n_refs, counts, padded_len);
    if (rc || n_tiles == 0) return rc;
    if (!offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL deletion table buffer");
    k_dels_write<<<text_grid(n_tiles), TWG, 0, (hipStream_t)stream>>>(a, offs, dst, dst_len);
    return launched("k_dels_write");
}
