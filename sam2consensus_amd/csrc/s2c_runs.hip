// s2c_runs.hip — runs of equal coverage as text, found on the device (--depth, --lowcov).
//
// The class of a position with cov = Σc (64-bit): cov itself when cut == 0 (--depth), the
// predicate cov < cut when cut ≥ 1 (--lowcov).  A run is a maximal stretch of one class inside
// its reference [s, e); its line is "S\tE\tCOV\n" (cut == 0, at most 34 bytes) or "S\tE\n"
// (cut ≥ 1, only the runs whose predicate holds, at most 22 bytes), S and E the printed
// positions of its first and last position.
//
// Three launches, shaped as s2c_sites.hip's.  k_runs_mark reads the six rows once (24 B per
// position) and leaves one bit per position, set where the class differs from the position
// before: a wave covers 64 aligned positions, a lane's left neighbour comes from the lane
// below (lane 0's from the word before, or from a load of position g − 1), the ballot is the
// mask word.  k_runs_len and k_runs_write queue a block's set bits — the run starts — with
// walk_mask (s2c_text.h) as the sites' kernels do.  Two things a run needs that a site does not:
//   - its end is the next start.  The walk holds the queue's last entry back until the next one
//     arrives (HOLD), and lane k of an emit reads entries k and k + 1;
//   - the end of the block's last start lies past the block, possibly far (an uncovered
//     stretch of 30 Mb is half a million mask words).  The whole workgroup looks it up: each
//     lane reads RLOOK mask words per step, a ballot finds each wave's first non-zero word, the
//     lowest position of the waves wins; the lookup stops at e.
// A run belongs to the block that holds its start, so the text does not depend on how the
// blocks cut a reference; a block without a start gives no byte.  The bit at g == s is forced
// on (references start at multiples of 64 behind zero-count padding: a reference whose first
// coverage equals the class before it would lose its first run).
#include "s2c_text.h"

namespace s2c {
namespace {

constexpr int RLINE = 34;                  // 10 + 10 digits of positions, 11 of coverage, 3 separators
constexpr int RBUF = text_buf(RLINE);
constexpr uint32_t MCHUNK = 8;             // consecutive mask words per wave of k_runs_mark
constexpr uint32_t RLOOK = 2;              // mask words per lane and step of the end lookup
constexpr int64_t NO_START = INT64_MAX;

__device__ __forceinline__ uint64_t class_of(uint64_t cov, uint64_t cut) { return cut ? (uint64_t)(cov < cut) : cov; }

// mask[w] bit l = class(64 w + l) != class(64 w + l − 1); bit 0 of word 0 set; bits at or past
// padded_len zero.  A wave takes MCHUNK consecutive words, their 6 · MCHUNK row loads in flight
// together; lane 0's left neighbour is lane 63 of the word before, and for the chunk's first
// word a load of position g − 1 (one address for the wave).
__global__ __launch_bounds__(TWG) void k_runs_mark(const uint32_t *__restrict__ counts, int64_t padded_len, uint64_t cut,
                                                    uint64_t *__restrict__ mask, uint64_t n_words) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * MWORDS + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * MWORDS;
    for (uint64_t c = wave * MCHUNK; c < n_words; c += n_waves * MCHUNK) {
        uint64_t cls[MCHUNK];
#pragma unroll
        for (uint32_t k = 0; k < MCHUNK; k++) {
            const uint64_t g = (c + k) * 64u + lane;
            cls[k] = g < (uint64_t)padded_len ? class_of(cov_at(counts, (uint64_t)padded_len, g), cut) : 0ull;
        }
        // (position 0 has no left neighbour: no class equals ~0; c · 64 ≤ padded_len − 1 otherwise)
        unsigned long long prev = c ? class_of(cov_at(counts, (uint64_t)padded_len, c * 64u - 1u), cut) : ~0ull;
#pragma unroll
        for (uint32_t k = 0; k < MCHUNK; k++) {
            const bool in = (c + k) * 64u + lane < (uint64_t)padded_len;
            unsigned long long left = __shfl_up((unsigned long long)cls[k], 1);   // lane 0 gets its own value back
            left = lane == 0 ? prev : left;
            const uint64_t word = __ballot(in && cls[k] != left);
            if (lane == 0 && c + k < n_words) mask[c + k] = word;
            prev = __shfl((unsigned long long)cls[k], 63);
        }
    }
}

// The first set bit of mask in [b, e), or e: the end of the run that holds position b − 1
// (b < e).  The whole workgroup steps over the words, RLOOK per lane and step (their loads in
// flight together): a ballot per word finds each wave's first non-zero one, the lowest
// position of the waves wins; every lane returns the same.  One barrier per step: wfirst
// [2][MWORDS] is used by the step's parity (a wave a step ahead writes the other half).
__device__ __forceinline__ int64_t next_start(const uint64_t *__restrict__ mask, int64_t b, int64_t e, int64_t *wfirst,
                                              uint32_t tid, uint32_t lane, uint32_t wv) {
    const int64_t w0 = b >> 6, wl = (e - 1) >> 6;
    uint32_t par = 0;
    for (int64_t base = w0; base <= wl; base += RLOOK * TWG, par ^= MWORDS) {
        uint64_t m[RLOOK];
#pragma unroll
        for (uint32_t j = 0; j < RLOOK; j++) {
            const int64_t w = base + (int64_t)(j * TWG + tid);
            m[j] = w <= wl ? mask[w] : 0ull;
            if (w == w0) m[j] &= ~0ull << (b & 63);
        }
        int64_t pos = NO_START;
#pragma unroll
        for (int j = (int)RLOOK - 1; j >= 0; j--) {   // (downwards: the lowest word stays)
            const uint64_t bal = __ballot(m[j] != 0ull);
            if (bal) {
                const uint32_t src = (uint32_t)__builtin_ctzll(bal);
                const uint64_t mm = (uint64_t)__shfl((unsigned long long)m[j], (int)src);
                pos = ((base + (int64_t)((uint32_t)j * TWG + wv * 64u + src)) << 6) + __builtin_ctzll(mm);
            }
        }
        if (lane == 0) wfirst[par + wv] = pos;
        lds_sync();
        int64_t best = NO_START;
#pragma unroll
        for (uint32_t k = 0; k < MWORDS; k++) best = wfirst[par + k] < best ? wfirst[par + k] : best;
        if (best != NO_START) return best < e ? best : e;
    }
    return e;
}

// walk_mask over block B's run starts: emit(head, cnt, tail) on the queue's first cnt starts.
// While the walk goes on tail < 0: the end of start k is entry k + 1, which the queue holds.  At
// the block's end the last start's end = tail, the next start past the block — not looked up
// when cut ≥ 1 and the last run's predicate is false: it has no line, and its end is not used.
// the run starts of mask word w inside [a, b) (w one of the words [a, b) overlaps)
__device__ __forceinline__ uint64_t start_word(const uint64_t *__restrict__ mask, int64_t w, const RBlk &B) {
    uint64_t m = mask[w];
    const int64_t lo = w << 6;
    if (B.a == B.s && (B.s >> 6) == w) m |= 1ull << (B.s & 63);   // (the bit at g == s forced on)
    if (B.a > lo) m &= ~0ull << (B.a - lo);
    if (B.b < lo + 64) m &= ~0ull >> (lo + 64 - B.b);
    return m;
}

template <typename Emit>
__device__ __forceinline__ void walk_block(const uint32_t *__restrict__ counts, int64_t padded_len, uint64_t cut,
                                           const uint64_t *__restrict__ mask, const RBlk &B, uint64_t *queue, int64_t *wfirst,
                                           uint32_t tid, uint32_t lane, uint32_t wv, Emit emit) {
    const auto word = [](const uint64_t *__restrict__ mk, int64_t w, const RBlk &K) { return start_word(mk, w, K); };
    const auto last = [&](uint32_t qh, uint32_t qn) {
        bool need = true;
        if (cut) {
            lds_sync();   // (the entries are in)
            need = cov_at(counts, (uint64_t)padded_len, queue[(qh + qn - 1u) & (QCAP - 1u)]) < cut;
        }
        const int64_t tail = need && B.b < B.e ? next_start(mask, B.b, B.e, wfirst, tid, lane, wv) : B.e;
        emit(qh, qn, tail);
    };
    walk_mask<true>(mask, B, word, queue, lane, wv, emit, last, (int64_t)-1);
}

// lane tid's run of an emit: its start g and end (exclusive)
__device__ __forceinline__ void take_run(const uint64_t *queue, uint32_t qh, uint32_t cnt, int64_t tail, uint32_t tid,
                                         uint64_t &g, uint64_t &end) {
    g = queue[(qh + tid) & (QCAP - 1u)];
    end = (tail < 0 || tid + 1u < cnt) ? queue[(qh + tid + 1u) & (QCAP - 1u)] : (uint64_t)tail;
}

// bytes of the run's line: S and E the printed first and last position
__device__ __forceinline__ uint32_t run_len(uint64_t S, uint64_t E, uint64_t cov, uint64_t cut) {
    if (cut) return cov < cut ? ndig64(S) + ndig64(E) + 2u : 0u;
    return ndig64(S) + ndig64(E) + ndig64(cov) + 3u;
}
// the run's line (run_len > 0) written to buf, ending before byte `e`
__device__ __forceinline__ void put_run(uint8_t *buf, uint32_t e, uint64_t S, uint64_t E, uint64_t cov, uint64_t cut) {
    buf[--e] = '\n';
    if (!cut) {
        e = put64(buf, e, cov);
        buf[--e] = '\t';
    }
    e = put64(buf, e, E);
    buf[--e] = '\t';
    put64(buf, e, S);
}

template <typename F>
__device__ __forceinline__ int64_t wave_fold(int64_t v, F f) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = f(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}

// lens[i] = bytes of block i's lines; stats[i] = {runs, covered, passed, sumcov, mincov, maxcov}
// of the runs that start in block i (cut == 0; not written when cut ≥ 1)
__global__ __launch_bounds__(TWG) void k_runs_len(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                   const uint64_t *__restrict__ mask, const int64_t *__restrict__ blocks,
                                                   const int64_t *__restrict__ refs, uint64_t n, uint64_t cut, uint64_t min_cov,
                                                   int64_t *__restrict__ lens, int64_t *__restrict__ stats) {
    __shared__ uint64_t queue[QCAP];
    __shared__ int64_t wfirst[2 * MWORDS];
    __shared__ int64_t wacc[MWORDS][7];
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wfirst, sizeof(wfirst));
    S2C_POISON(wacc, sizeof(wacc));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const RBlk B = load_rblk(blocks, refs, i);
        uint64_t sum = 0, runs = 0, covered = 0, passed = 0, sumcov = 0;
        int64_t mn = INT64_MAX, mx = -1;
        if (B.ok(padded_len) && B.a < B.b)
            walk_block(counts, padded_len, cut, mask, B, queue, wfirst, tid, lane, wv, [&](uint32_t qh, uint32_t cnt, int64_t tail) {
                lds_sync();
                uint64_t g = 0, end = 0;
                if (tid < cnt) take_run(queue, qh, cnt, tail, tid, g, end);
                lds_sync();
                if (tid < cnt) {
                    const uint64_t cov = cov_at(counts, (uint64_t)padded_len, g), len = end - g;
                    const uint64_t S = (uint64_t)B.p0 + (g - (uint64_t)B.a);
                    sum += run_len(S, S + len - 1u, cov, cut);
                    runs += 1u;
                    covered += cov >= 1u ? len : 0u;
                    passed += cov >= min_cov ? len : 0u;
                    sumcov += len * cov;
                    mn = (int64_t)cov < mn ? (int64_t)cov : mn;
                    mx = (int64_t)cov > mx ? (int64_t)cov : mx;
                }
            });
        sum = wave_sum(sum);
        runs = wave_sum(runs);
        covered = wave_sum(covered);
        passed = wave_sum(passed);
        sumcov = wave_sum(sumcov);
        mn = wave_fold(mn, [](int64_t x, int64_t y) { return y < x ? y : x; });
        mx = wave_fold(mx, [](int64_t x, int64_t y) { return y > x ? y : x; });
        if (lane == 0) {
            wacc[wv][0] = (int64_t)sum;
            wacc[wv][1] = (int64_t)runs;
            wacc[wv][2] = (int64_t)covered;
            wacc[wv][3] = (int64_t)passed;
            wacc[wv][4] = (int64_t)sumcov;
            wacc[wv][5] = mn;
            wacc[wv][6] = mx;
        }
        lds_sync();
        if (tid == 0) {
            int64_t t[7] = {0, 0, 0, 0, 0, INT64_MAX, -1};
            for (uint32_t w = 0; w < MWORDS; w++) {
                for (int k = 0; k < 5; k++) t[k] += wacc[w][k];
                t[5] = wacc[w][5] < t[5] ? wacc[w][5] : t[5];
                t[6] = wacc[w][6] > t[6] ? wacc[w][6] : t[6];
            }
            lens[i] = t[0];
            if (!cut)
                for (int k = 0; k < 6; k++) stats[6 * i + k] = t[k + 1];
        }
        lds_sync();   // (wacc is written again for the next block)
    }
}

// block i's lines → dst[offs[i], offs[i+1]); never a byte outside that range
__global__ __launch_bounds__(TWG) void k_runs_write(const uint32_t *__restrict__ counts, int64_t padded_len,
                                                     const uint64_t *__restrict__ mask, const int64_t *__restrict__ blocks,
                                                     const int64_t *__restrict__ refs, const int64_t *__restrict__ offs,
                                                     uint64_t n, uint64_t cut, uint8_t *__restrict__ dst, int64_t dst_len) {
    __shared__ alignas(16) uint8_t buf[RBUF];
    __shared__ uint64_t queue[QCAP];
    __shared__ int64_t wfirst[2 * MWORDS];
    __shared__ uint32_t wtot[MWORDS];   // wave totals of the line lengths
    S2C_POISON(buf, RBUF);
    S2C_POISON(queue, sizeof(queue));
    S2C_POISON(wfirst, sizeof(wfirst));
    S2C_POISON(wtot, sizeof(wtot));
    S2C_POISON_DONE();
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    for (uint64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const RBlk B = load_rblk(blocks, refs, i);
        const int64_t d0 = offs[i], d1 = offs[i + 1];
        if (!B.ok(padded_len) || d0 < 0 || d1 < d0 || d1 > dst_len || B.a == B.b) continue;
        const uint64_t cap = (uint64_t)(d1 - d0);
        uint64_t done = 0;   // bytes of the block written so far
        // cnt ≤ TWG queued starts, one line (or none) per lane
        walk_block(counts, padded_len, cut, mask, B, queue, wfirst, tid, lane, wv, [&](uint32_t qh, uint32_t cnt, int64_t tail) {
            lds_sync();   // (buf and wtot are no longer read either)
            const bool in = tid < cnt;
            uint64_t S = 0, E = 0, cov = 0;
            uint32_t len = 0;
            if (in) {
                uint64_t g, end;
                take_run(queue, qh, cnt, tail, tid, g, end);
                cov = cov_at(counts, (uint64_t)padded_len, g);
                S = (uint64_t)B.p0 + (g - (uint64_t)B.a);
                E = S + (end - g) - 1u;
                len = run_len(S, E, cov, cut);
            }
            done += emit_lines<RLINE>(buf, wtot, dst + d0, cap, done, len != 0u, len, tid, lane, wv,
                                      [&](uint8_t *img, uint32_t e) { put_run(img, e, S, E, cov, cut); });
        });
    }
}

}  // namespace
}  // namespace s2c

extern "C" int s2c_runs_mark(const uint32_t *counts, int64_t padded_len, int64_t cut, uint64_t *mask, void *stream) {
    using namespace s2c;
    if (padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad run table sizes");
    if (cut < 0) return s2c_set_error(S2C_ERR_ARG, "run class: cut >= 0");
    if (padded_len == 0) return S2C_OK;
    if (!counts || !mask) return s2c_set_error(S2C_ERR_ARG, "NULL run table buffer");
    const int64_t n_words = (padded_len + 63) / 64;
    const int64_t per_wg = MWORDS * MCHUNK;
    const unsigned grid = (unsigned)std::min<int64_t>((n_words + per_wg - 1) / per_wg, 8 * 256 * 8);
    k_runs_mark<<<grid, TWG, 0, (hipStream_t)stream>>>(counts, padded_len, (uint64_t)cut, mask, (uint64_t)n_words);
    return launched("k_runs_mark");
}

extern "C" int s2c_runs_len(const uint32_t *counts, int64_t padded_len, const uint64_t *mask, const int64_t *blocks,
                            const int64_t *refs, int64_t n, int64_t cut, int64_t min_cov, int64_t *lens, int64_t *stats,
                            void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad run table sizes");
    if (cut < 0 || min_cov < 0) return s2c_set_error(S2C_ERR_ARG, "run class: cut >= 0, min_cov >= 0");
    if (n == 0) return S2C_OK;
    if (!counts || !mask || !blocks || !refs || !lens || (cut == 0 && !stats))
        return s2c_set_error(S2C_ERR_ARG, "NULL run table buffer");
    k_runs_len<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, mask, blocks, refs, (uint64_t)n, (uint64_t)cut,
                                                              (uint64_t)min_cov, lens, stats);
    return launched("k_runs_len");
}

extern "C" int s2c_runs_write(const uint32_t *counts, int64_t padded_len, const uint64_t *mask, const int64_t *blocks,
                              const int64_t *refs, const int64_t *offs, int64_t n, int64_t cut, uint8_t *dst, int64_t dst_len,
                              void *stream) {
    using namespace s2c;
    if (n < 0 || padded_len < 0 || dst_len < 0) return s2c_set_error(S2C_ERR_ARG, "bad run table sizes");
    if (cut < 0) return s2c_set_error(S2C_ERR_ARG, "run class: cut >= 0");
    if (n == 0) return S2C_OK;
    if (!counts || !mask || !blocks || !refs || !offs || !dst) return s2c_set_error(S2C_ERR_ARG, "NULL run table buffer");
    k_runs_write<<<text_grid(n), TWG, 0, (hipStream_t)stream>>>(counts, padded_len, mask, blocks, refs, offs, (uint64_t)n,
                                                                (uint64_t)cut, dst, dst_len);
    return launched("k_runs_write");
}
