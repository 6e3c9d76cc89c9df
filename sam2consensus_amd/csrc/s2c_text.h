// s2c_text.h — the scheme of the kernels that write tables as text (s2c_table.hip, s2c_sites.hip,
// s2c_runs.hip, s2c_ins.hip, s2c_links.hip, s2c_dels.hip); each of those files keeps its line's
// format and what it selects.
//
// Lines have no fixed width, so a table takes two launches over its blocks {a, b, p0}, one
// workgroup per block, grid-strided: a length pass (block_total: lens[i] = bytes of block i's
// lines), the caller's exclusive prefix sum, and a write pass of block i into
// dst[offs[i], offs[i+1]).  The write pass goes TWG lines at a time, one per lane (emit_lines):
// a workgroup scan of the line lengths (DPP inside a row, the row and wave totals above it),
// every lane writes its line backwards into an LDS image at its scanned offset, and the image's
// contiguous bytes leave with 16-byte stores (store_text).  The image is shifted by the
// destination's misalignment, so LDS reads and global stores are both 16-byte aligned; head and
// tail bytes go out singly.  A sparse table picks its lines by a mask of one bit per position
// that a mark kernel left, and walk_mask queues a block's set bits for the two passes.
// The event tables (insertions, links, deletions) have lines without a useful width bound and
// entries that arrive in no order.  Their write step is emit_var_lines: the same scan, then the
// LDS image (Img) and store_text when the step's bytes fit it, and the guarded byte writer (Out)
// when they do not.  Their entries are ordered by bucket_by_pos, a counting sort over a tile's
// positions in LDS.  Both scan with wg_scan, the workgroup's prefix sum.
// Also here: the decimal digit code, one position's row and its counts line, the blocks with
// their guards (with their reference's range: RBlk), the barrier that orders a workgroup's
// scratch in HBM (wg_sync), and the launch grids.
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
// Inclusive prefix sum over the workgroup, in S (a wave's own sum fits 32 bits), and the
// workgroup's total: the wave's scan, lane 63 stores the wave's total, a barrier, the totals of
// the waves below.  wtot: TWG / 64 words of LDS that no lane still reads when the call starts; a
// barrier of the caller's stands between this call's reads and the next write of them.
// (emit_lines and k_table_write keep their own lines: DESIGN §4.4a)
template <typename S, typename W>
__device__ __forceinline__ S wg_scan(uint32_t x, W *wtot, uint32_t lane, uint32_t wv, S &tot) {
    const uint32_t inc = wave_scan(x, lane);
    if (lane == 63u) wtot[wv] = inc;
    lds_sync();
    S below = 0;
    tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < TWG / 64; w++) {
        const S t = (S)wtot[w];
        below += w < wv ? t : (S)0;
        tot += t;
    }
    return below + inc;
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
// the coverage alone
__device__ __forceinline__ uint64_t cov_at(const uint32_t *__restrict__ counts, uint64_t padded_len, uint64_t g) {
    uint64_t cov = 0;
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) cov += counts[s * padded_len + g];
    return cov;
}
__device__ __forceinline__ uint32_t line_len(const Row &r) {
    uint32_t n = ndig64(r.pos) + ndig64(r.cov) + 8u;
#pragma unroll
    for (uint32_t s = 0; s < NSYM; s++) n += ndig32(r.c[s]);
    return n;
}

// decimal digits of x written backwards, ending before byte `e` of buf; returns the first byte.
// buf: anything that stores a byte by buf[o] = ch — an LDS image's pointer (emit_lines' bound
// holds the lines inside it), or a guarded range of the destination (s2c_ins.hip's Out).
template <typename Buf, typename I>
__device__ __forceinline__ I put32(Buf buf, I e, uint32_t x) {
    do {
        const uint32_t q = x / 10u;
        buf[--e] = (uint8_t)('0' + (x - q * 10u));
        x = q;
    } while (x);
    return e;
}
// (v < 2^41)
template <typename Buf, typename I>
__device__ __forceinline__ I put64(Buf buf, I e, uint64_t v) {
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

// a block with the range [s, e) of its reference (the run tables, the link tables)
struct RBlk {
    int64_t a, b, p0, s, e;
    __device__ __forceinline__ bool ok(int64_t padded_len) const {
        return s >= 0 && s <= a && a <= b && b <= e && e <= padded_len && p0 >= 0 && p0 <= TPOS_END - (e - a);
    }
};
__device__ __forceinline__ RBlk load_rblk(const int64_t *__restrict__ blocks, const int64_t *__restrict__ refs, uint64_t i) {
    return RBlk{blocks[3 * i], blocks[3 * i + 1], blocks[3 * i + 2], refs[2 * i], refs[2 * i + 1]};
}

// A block's range of dst for a writer that stores byte by byte (k_ins_write; emit_var_lines'
// long steps): no byte is stored outside [0, cap).  o[k] = ch is put(k, ch), so put32 / put64
// write their digits through it.
struct Out {
    uint8_t *d;
    uint64_t cap;
    __device__ __forceinline__ void put(uint64_t o, uint32_t ch) const {
        if (o < cap) d[o] = (uint8_t)ch;
    }
    struct Byte {
        const Out &out;
        uint64_t o;
        __device__ __forceinline__ void operator=(uint8_t ch) const { out.put(o, ch); }
    };
    __device__ __forceinline__ Byte operator[](uint64_t o) const { return Byte{*this, o}; }
};
// the LDS image behind the same two calls: every line of a step lies inside it (emit_var_lines)
struct Img {
    uint8_t *b;
    __device__ __forceinline__ void put(uint64_t o, uint32_t ch) const { b[o] = (uint8_t)ch; }
    __device__ __forceinline__ uint8_t &operator[](uint64_t o) const { return b[o]; }
};

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

// The write side of one line per lane (k_sites_write, k_runs_write; k_table_write keeps its own
// copy of these lines: through this function its sub-block loop compiled to other instructions).
// Lane tid (lane of wave wv) has a line iff `has`, of len bytes (0 without one); put(buf, end)
// writes it backwards, ending before byte `end` of the LDS image buf.  The lines go, in lane
// order, to d0[run, ...), cut at d0[cap); returns the bytes stored (the same in every lane).
// wtot: TWG / 64 words of LDS for the waves' totals, which no lane still reads when the call
// starts (the walks' emits start with a barrier).  buf is written only past the first barrier
// inside, which every lane's reads of the call before (store_text) precede.
template <int LINE, int BUF, typename Put>
__device__ __forceinline__ uint32_t emit_lines(uint8_t (&buf)[BUF], uint32_t *wtot, uint8_t *d0, uint64_t cap, uint64_t run,
                                               bool has, uint32_t len, uint32_t tid, uint32_t lane, uint32_t wv, Put put) {
    static_assert(15 + TWG * LINE < BUF, "the LDS image holds TWG lines behind the destination's misalignment");
    // inclusive scan of the lengths: the wave's, then the waves below
    const uint32_t inc = wave_scan(len, lane);
    if (lane == 63u) wtot[wv] = inc;
    lds_sync();
    uint32_t below = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < TWG / 64; w++) {
        const uint32_t t = wtot[w];
        below += w < wv ? t : 0u;
        tot += t;
    }
    // the LDS image starts at the destination's offset inside its 16-byte word
    uint8_t *d = d0 + run;
    const uint32_t sh = (uint32_t)((uintptr_t)d & 15u);
    if (has) put(buf, sh + below + inc);   // the line's end ≤ 15 + TWG·LINE
    lds_sync();
    // (offs that do not match the lengths: the text is cut at the block's range)
    const uint64_t left = cap - run;
    if ((uint64_t)tot > left) tot = (uint32_t)left;
    store_text(buf, d, sh, tot, tid);
    return tot;
}
constexpr int text_buf(int line) { return TWG * line + 16; }   // + the destination's misalignment (< 16)

// The write side of a table whose lines have no useful width bound (k_links_write,
// k_dels_write: a reference name can have any length, so the sums are 64-bit).  Lane tid has a
// line of len bytes (0: none); put(o, at) writes it at o[at, at + len), o an Img or an Out.  The
// step's lines go, in lane order, to out.d[run, ...): through the LDS image buf and store_text
// when they sum to at most IMG bytes, byte by byte through out's guard when they do not; cut at
// out.cap either way.  Returns the step's bytes (the same in every lane).  wtot and buf: nobody
// still reads them when the call starts (the caller's step starts with a barrier).
constexpr uint32_t LIMG = 24 * 1024 - 16;   // the event tables' image: five workgroups a CU with the links' queue
template <uint32_t IMG, typename Put>
__device__ __forceinline__ uint64_t emit_var_lines(uint8_t (&buf)[IMG + 16], uint32_t *wtot, const Out &out, uint64_t run, uint32_t len,
                                                   uint32_t tid, uint32_t lane, uint32_t wv, Put put) {
    uint64_t tot;
    const uint64_t at = wg_scan(len, wtot, lane, wv, tot) - len;
    if (tot <= IMG) {   // (the same in every lane)
        uint8_t *d = out.d + run;
        const uint32_t sh = (uint32_t)((uintptr_t)d & 15u);
        if (len) put(Img{buf}, sh + at);
        lds_sync();
        // (offs that do not match the lengths: the text is cut at the block's range)
        const uint64_t left = run < out.cap ? out.cap - run : 0ull;
        if (left) store_text(buf, d, sh, (uint32_t)min(tot, left), tid);
    } else if (len) {
        put(out, run + at);
    }
    return tot;
}

// The length side: out[0] = Σ of sum over the workgroup (wsum: a word of LDS per wave).
__device__ __forceinline__ void block_total(uint64_t sum, uint64_t *wsum, uint32_t tid, int64_t *out) {
    sum = wave_sum(sum);
    if ((tid & 63u) == 0) wsum[tid >> 6] = sum;
    lds_sync();
    if (tid == 0) {
        uint64_t t = 0;
        for (int w = 0; w < TWG / 64; w++) t += wsum[w];
        *out = (int64_t)t;
    }
    lds_sync();   // (wsum is written again for the next block)
}

// Workgroup barrier that also orders the workgroup's global (scratch) stores before its loads
__device__ __forceinline__ void wg_sync() {
    __threadfence_block();
    __syncthreads();
}

// A tile's entries ordered by position (k_ins_len, k_dels_len): a counting sort over the tile's
// NPOS positions in LDS.  each(f) is the caller's loop over its sources, grid-strided over the
// workgroup; it calls f(pos, entry) for every valid entry, pos < NPOS, and is run twice: a
// histogram of the entries per position, then — the histogram scanned to the buckets' starts,
// each lane its NPOS / TWG bins — a scatter of every entry into its position's bucket of out[].
// Leaves start[p] the first place of position p's bucket (start[NPOS] = the entries, which is
// returned; total is the word of LDS they go through) and the order inside a bucket the
// atomics', on which nothing may depend.  The caller's wg_sync stands between the scatter and
// its reads of out[], and another before the next call (start, cursor and total are written again).
template <uint32_t NPOS, typename Each>
__device__ __forceinline__ uint32_t bucket_by_pos(uint32_t (&start)[NPOS + 1], uint32_t (&cursor)[NPOS], uint64_t *wsum, uint32_t &total,
                                                  uint4 *out, uint32_t tid, uint32_t lane, uint32_t wv, Each each) {
    constexpr uint32_t PER = NPOS / TWG;
    static_assert(PER * TWG == NPOS, "every lane scans the same number of bins");
    for (uint32_t p = tid; p <= NPOS; p += TWG) start[p] = 0u;
    for (uint32_t p = tid; p < NPOS; p += TWG) cursor[p] = 0u;
    lds_sync();
    each([&](uint32_t pos, const uint4 &) { atomicAdd(&start[pos], 1u); });
    lds_sync();
    uint32_t c[PER], sum = 0, all;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        c[k] = start[PER * tid + k];
        sum += c[k];
    }
    uint32_t at = wg_scan(sum, wsum, lane, wv, all) - sum;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        start[PER * tid + k] = at;
        at += c[k];
    }
    if (tid == TWG - 1) start[NPOS] = total = at;
    lds_sync();
    const uint32_t n = total;
    each([&](uint32_t pos, const uint4 &e) { out[start[pos] + atomicAdd(&cursor[pos], 1u)] = e; });
    return n;
}

constexpr uint32_t MWORDS = TWG / 64;      // mask words per step of the walk: one per wave
constexpr uint32_t QCAP = 2 * TWG;         // the queue: ≤ TWG positions left over + ≤ TWG new ones

// The walk both passes of a sparse table make over a block B = [a, b), a < b: its mask words,
// word(mask, w, B) each one's bits inside the block, MWORDS at a time (one per wave); the set
// bits' positions queued in LDS — a ring of QCAP; each lane's slot its bit's rank (mbcnt inside
// the word, popcounts of the words below) — and emit(head, TWG, mid...) called on the queue's
// first TWG positions whenever it holds TWG of them (HOLD: more than TWG, so the last one stays
// queued until its successor is — a line that needs the next position finds it at the next
// slot), and finish(head, cnt) on the rest, 1 ≤ cnt ≤ TWG, at the block's end.  A stretch
// without a set bit is skipped: no LDS, no barrier.  Every lane of the workgroup sees the same
// words, so the skips and the calls of emit and finish are the whole workgroup's.  Both start
// with a barrier (the entries are in, and what the call before read is no longer read) and have
// another between their reads of the queue and their end (the next entries land on the slots
// they read).  (word is the file's own function, and emit is called with the caller's own
// arguments, not through a wrapper: either changed the order of the step's instructions.)
template <bool HOLD, typename Blk, typename Word, typename Emit, typename Finish, typename... Mid>
__device__ __forceinline__ void walk_mask(const uint64_t *__restrict__ mask, const Blk &B, Word word, uint64_t *queue,
                                          uint32_t lane, uint32_t wv, Emit emit, Finish finish, Mid... mid) {
    uint32_t qh = 0, qn = 0;   // the queue's head and fill
    const int64_t wl = (B.b - 1) >> 6;   // the block's last mask word
    for (int64_t wb = B.a >> 6; wb <= wl; wb += MWORDS) {
        uint64_t m[MWORDS], any = 0;
#pragma unroll
        for (uint32_t w = 0; w < MWORDS; w++) {
            m[w] = wb + w <= wl ? word(mask, wb + w, B) : 0ull;
            any |= m[w];
        }
        if (!any) continue;
        uint64_t mine = 0;
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (uint32_t w = 0; w < MWORDS; w++) {
            const uint32_t c = (uint32_t)__popcll(m[w]);
            mine = w == wv ? m[w] : mine;
            pre += w < wv ? c : 0u;
            tot += c;
        }
        if ((mine >> lane) & 1u) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
            queue[(qh + qn + pre + rank) & (QCAP - 1u)] = (uint64_t)(((wb + wv) << 6) + lane);
        }
        qn += tot;   // ≤ 2·TWG = QCAP (< without HOLD)
        if (HOLD ? qn > (uint32_t)TWG : qn >= (uint32_t)TWG) {
            emit(qh, (uint32_t)TWG, mid...);
            qh = (qh + TWG) & (QCAP - 1u);
            qn -= TWG;
        }
    }
    if (qn) finish(qh, qn);
}

// the grid of a table's len and write kernels over n blocks: 8 workgroups per CU
inline unsigned text_grid(int64_t n) { return (unsigned)std::min<int64_t>(n, 8 * 256 * 4); }
// the grids of the grid-strided kernels with a lane per item over n items (mask words, hash
// slots: walk_grid) and of those whose lane walks a piece's tokens (piece_grid: 8 workgroups per CU)
inline unsigned walk_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + TWG - 1) / TWG, 8 * 256 * 4); }
inline unsigned piece_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + TWG - 1) / TWG, 8 * 256); }

// a launcher's last line: S2C_OK, or the launch's error as "<kernel>: <what HIP says>"
inline int launched(const char *kernel) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? S2C_OK : s2c_set_error(S2C_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(e));
}

}  // namespace s2c
