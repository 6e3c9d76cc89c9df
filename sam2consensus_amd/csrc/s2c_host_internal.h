// s2c_host_internal.h — what more than one host unit of libs2c.so needs (not installed):
//   s2c_host.cpp    error state, plan knobs, worker-pool registry, gather / copy, parsecigar, layout
//   s2c_parse.cpp   the SAM line parser and the parser-side C-ABI (streamed batches, pack / unpack)
//   s2c_reader.cpp  plain / gzip / block-parallel BGZF byte source, s2c_parser_feed_file
//   s2c_plan.cpp    build_batch: pieces → sorted batch → tile plan; the layer planner; dwin / dpc
//   s2c_shard.cpp   s2c_batch_shard and the s2c_batch_* accessors
//   s2c_synth.cpp   the synthetic workloads
#pragma once
#include "../../include/s2c.h"

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

// ------------------------------------------------------------------ errors
int s2c_set_error(int code, const std::string &msg);   // (thread-local text of s2c_last_error)
// No C++ exception crosses the C-ABI: an allocation failure (e.g. a corrupt input's sizes)
// or any other exception becomes an error code.
template <class F>
int s2c_guarded(F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return s2c_set_error(S2C_ERR_LIMIT, "out of host memory");
    } catch (const std::length_error &e) {
        return s2c_set_error(S2C_ERR_LIMIT, std::string("size beyond this build's limits: ") + e.what());
    } catch (const std::exception &e) {
        return s2c_set_error(S2C_ERR_IO, std::string("host exception: ") + e.what());
    }
}

// ------------------------------------------------------------------ plan knobs (s2c_host.cpp)
const char *plan_env(const char *name);   // a plan override's value, read only under S2C_DEBUG_PLAN
int64_t plan_cus();                       // the device's compute units (s2c_plan_set_cus)

// ------------------------------------------------------------------ host worker pools
// Persistent host threads for the parse windows and the plan's parallel loops.  A thread
// made per window (16 per 64 MB block of a streamed file) maps its stack while the other
// threads first-touch their chunks' buffers; those page faults and the mapping serialise on
// the process's memory map, and the last thread of a window started 25-35 ms after the
// first (S2C_HOST_TIMING).  A pool's threads wait on a condition variable between runs.
// One run at a time per pool: a run asked for while the pool is busy (another thread's run,
// or a run nested in one) gets threads of its own, as before.  A forked child makes new pools.
class WorkerPool {
  public:
    // f(t) for t in [0, nt): t = 0 on the calling thread, the others on the pool's
    // (an exception of any f(t) is rethrown here once every thread is done with the run)
    template <class F>
    void run(int nt, F &&f) {
        if (nt <= 1) { f(0); return; }
        std::exception_ptr err;
        std::mutex em;
        auto safe = [&](int t) {
            try {
                f(t);
            } catch (...) {
                std::lock_guard<std::mutex> lk(em);
                if (!err) err = std::current_exception();
            }
        };
        // a run nested in this thread's own run of the pool must not try_lock the mutex it
        // holds (undefined behaviour): it is told apart by the owner's thread id
        std::unique_lock<std::mutex> rl;
        if (owner_.load(std::memory_order_relaxed) != std::this_thread::get_id()) rl = std::unique_lock<std::mutex>(run_m_, std::try_to_lock);
        if (!rl.owns_lock()) {   // busy: threads of its own
            std::vector<std::thread> th;
            for (int t = 1; t < nt; t++) th.emplace_back([&safe, t] { safe(t); });
            safe(0);
            for (auto &x : th) x.join();
            if (err) std::rethrow_exception(err);
            return;
        }
        const std::function<void(int)> job = [&safe](int t) { safe(t); };
        owner_.store(std::this_thread::get_id(), std::memory_order_relaxed);
        struct Release {
            std::atomic<std::thread::id> &o;
            ~Release() { o.store(std::thread::id(), std::memory_order_relaxed); }
        } release{owner_};
        {
            std::lock_guard<std::mutex> lk(m_);
            while ((int)n_threads_ < nt - 1) {
                const int t = n_threads_ + 1;
                std::thread([this, t] { loop(t); }).detach();
                n_threads_++;
            }
            job_ = &job;
            want_ = nt;
            left_ = nt - 1;
            gen_++;
        }
        go_.notify_all();
        safe(0);
        {
            std::unique_lock<std::mutex> lk(m_);
            done_.wait(lk, [&] { return left_ == 0; });
            job_ = nullptr;
        }
        if (err) std::rethrow_exception(err);
    }
    static WorkerPool &get(int which);   // the pool `which` of this process (registry: s2c_host.cpp)

  private:
    static std::mutex &reg_m();
    static WorkerPool *(&reg())[3];
    void loop(int t);
    std::mutex run_m_, m_;
    std::atomic<std::thread::id> owner_{};   // the thread running the pool's current run
    std::condition_variable go_, done_;
    const std::function<void(int)> *job_ = nullptr;
    uint64_t gen_ = 0;
    int want_ = 0, left_ = 0, n_threads_ = 0;
};
enum { POOL_PARSE = 0, POOL_PLAN = 1, POOL_IO = 2 };

// Host threads of the plan: the parse's (≤ 16, S2C_PARSE_THREADS), at most n / grain.
int plan_threads(int64_t n, int64_t grain);
// f(t, i0, i1) on nt contiguous ranges of [0, n), thread t on range t
template <class F>
void par_ranges(int nt, int64_t n, F &&f) {
    if (nt <= 1) { f(0, (int64_t)0, n); return; }
    WorkerPool::get(POOL_PLAN).run(nt, [&f, nt, n](int t) { f(t, n * t / nt, n * (t + 1) / nt); });
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t align_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

// ------------------------------------------------------------------ CIGAR tokens
inline int opcode_of(char c) {
    switch (c) {
        case 'M': return S2C_OP_M;
        case 'I': return S2C_OP_I;
        case 'D': return S2C_OP_D;
        case 'N': return S2C_OP_N;
        case 'S': return S2C_OP_S;
        case 'H': return S2C_OP_H;
        case 'P': return S2C_OP_P;
        case '=': return S2C_OP_EQ;
        case 'X': return S2C_OP_X;
        default: return -1;
    }
}
inline bool op_bases(uint32_t op) { return op == S2C_OP_M || op == S2C_OP_EQ || op == S2C_OP_X; }
inline bool op_dash(uint32_t op) { return op == S2C_OP_D || op == S2C_OP_N || op == S2C_OP_P; }

// re.findall(r"(\d+)([MIDNSHPX=]{1})", cigar) (:58): a match is a maximal digit run
// immediately followed by an op letter; everything else is skipped.  Appends token words
// (len << 4 | opcode).
template <class V>
int tokenize_cigar(const char *s, size_t n, V &out, uint32_t *ntok) {
    size_t i = 0;
    uint32_t k = 0;
    while (i < n) {
        if (s[i] < '0' || s[i] > '9') { i++; continue; }
        size_t j = i;
        uint64_t v = 0;
        bool big = false;
        while (j < n && s[j] >= '0' && s[j] <= '9') {
            v = v * 10 + (uint64_t)(s[j] - '0');
            if (v > S2C_OP_LEN_MAX) { big = true; v = S2C_OP_LEN_MAX; }
            j++;
        }
        if (j < n) {
            const int oc = opcode_of(s[j]);
            if (oc >= 0) {
                if (big) return s2c_set_error(S2C_ERR_LIMIT, "CIGAR op length >= 2^28 not supported");
                out.push_back((uint32_t)(v << 4) | (uint32_t)oc);
                k++;
                i = j + 1;
                continue;
            }
        }
        i = j;
    }
    *ntok = k;
    return S2C_OK;
}

// Allocator of the parser's and the batch's big arrays: default-initialising (resize() leaves
// the elements unwritten, so they are first touched by the threads that fill them, not by a
// serial zero-fill) and, from 4 MB on, backed by 2 MB-aligned anonymous mappings advised
// as transparent huge pages (512x fewer page faults for the GB-sized arrays of a batch).
constexpr size_t HUGE_PAGE = (size_t)2 << 20;
inline size_t huge_min() {   // S2C_HUGE_MIN_KB: the smallest array so mapped (default 4 MB)
    static const size_t m = [] { const char *e = getenv("S2C_HUGE_MIN_KB"); return e ? (size_t)atoll(e) << 10 : (size_t)4 << 20; }();
    return m;
}
inline bool huge_pages() {   // S2C_HUGEPAGES=0 turns the advice off
    static const bool on = [] { const char *e = getenv("S2C_HUGEPAGES"); return !e || atoi(e) != 0; }();
    return on;
}
template <class T>
struct uninit_alloc {
    using value_type = T;
    template <class U> struct rebind { using other = uninit_alloc<U>; };
    uninit_alloc() = default;
    template <class U> uninit_alloc(const uninit_alloc<U> &) {}
    static size_t map_len(size_t bytes) { return (bytes + HUGE_PAGE - 1) & ~(HUGE_PAGE - 1); }
    static bool poison() {   // S2C_MAP_POISON=1 (tests): every array starts as 0xA5 bytes, not zero pages
        static const bool on = getenv("S2C_MAP_POISON") != nullptr;
        return on;
    }
    T *allocate(size_t n) {
        T *p = allocate_raw(n);
        if (poison()) memset((void *)p, 0xA5, n * sizeof(T));
        return p;
    }
    T *allocate_raw(size_t n) {
        const size_t bytes = n * sizeof(T);
        if (bytes < huge_min()) {
            void *q = ::operator new(bytes);
            return (T *)q;
        }
        const size_t len = map_len(bytes);
        void *raw = mmap(nullptr, len + HUGE_PAGE, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw == MAP_FAILED) throw std::bad_alloc();
        const uintptr_t r = (uintptr_t)raw, a = (r + HUGE_PAGE - 1) & ~(uintptr_t)(HUGE_PAGE - 1);
        if (a > r) munmap(raw, a - r);                                      // the unaligned head
        if (r + len + HUGE_PAGE > a + len) munmap((void *)(a + len), r + len + HUGE_PAGE - (a + len));   // and tail
        if (huge_pages()) madvise((void *)a, len, MADV_HUGEPAGE);
        return (T *)a;
    }
    void deallocate(T *q, size_t n) {
        const size_t bytes = n * sizeof(T);
        if (bytes < huge_min()) ::operator delete((void *)q);
        else munmap((void *)q, map_len(bytes));
    }
    template <class U> void construct(U *q) noexcept { ::new ((void *)q) U; }
    template <class U, class... A> void construct(U *q, A &&...a) { ::new ((void *)q) U(std::forward<A>(a)...); }
    template <class U> bool operator==(const uninit_alloc<U> &) const { return true; }
    template <class U> bool operator!=(const uninit_alloc<U> &) const { return false; }
};
using u32buf = std::vector<uint32_t, uninit_alloc<uint32_t>>;

// ------------------------------------------------------------------ parser state
// One mapped read as the parser keeps it (file order).  Its tokens, base planes and
// insertion events live in the parse chunk that read it.
struct ReadRec {
    int64_t pos0;           // POS - 1 (:201)
    int64_t klen;           // len(seqout)
    int64_t kc0, kc1;       // counted seqout range [kc0, kc1); kc0 < 0: nothing counted
    uint64_t tok;           // first token (chunk toks)
    uint64_t q;             // first SEQ base (chunk planes, multiple of 16)
    uint32_t ref, ntok, slen, ev0, nev;
    uint8_t has_x, drop;
};
struct Event {              // insertion with a non-empty motif (:73-75), file order
    int64_t key;            // start_ref (:74), reference-relative
    uint64_t q;             // motif's first base (chunk planes)
    uint32_t ref, len, read;
};
struct Chunk {
    std::vector<ReadRec, uninit_alloc<ReadRec>> reads;
    u32buf toks;
    u32buf bq, bx;   // planes [k][2] and [k]; bases [0, nq)
    uint64_t nq = 0;
    uint64_t nz = 0;   // plane words [0, nz) initialised (pack_seq zeroes the words it reaches)
    std::vector<Event> ev;
    int64_t lines_total = 0, reads_mapped = 0, aligned = 0, qbases = 0, ntokens = 0;
    std::vector<uint32_t> sp;       // the current read's SEQ planes (seq_planes: 4 words per 32 chars)
    // an upper bound of its reads' extents (read_extent's hi): reference hb_ref, position
    // hb_pos in it (a read of an earlier reference ends below that reference's offset);
    // hb_pos < 0: no bound (no read yet, or a chunk made by s2c_parser_unpack)
    uint32_t hb_ref = 0;
    int64_t hb_pos = -1;
    void bound(uint32_t ref, int64_t pos0, int64_t klen, int64_t L) {
        const int64_t b = pos0 < 0 ? L : pos0 + klen;   // (a POS <= 0 wrap reaches the reference's end)
        if (hb_pos < 0 || ref > hb_ref) {
            hb_ref = ref;
            hb_pos = b;
        } else if (ref == hb_ref) {
            hb_pos = std::max(hb_pos, b);
        }
    }
};

struct s2c_parser {
    bool maxdel_active = true;
    int64_t maxdel = 150;
    bool in_header = true;
    int64_t header_lines = 0;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_len;
    std::unordered_map<std::string, uint32_t> ref_idx;
    std::vector<std::unique_ptr<Chunk>> chunks;   // file order
    std::string carry;              // partial line of the streaming feed
    int err = S2C_OK;
    std::string errmsg;
    std::string last_name;
    int64_t last_ref = -1;
    // streamed batches (s2c_parser_retain): tile width of every reference, the first global
    // position not yet emitted, chunks [0, n_kept) hold the reads kept from earlier batches,
    // and whether a later read reached below the frontier (input not coordinate-sorted)
    int64_t tile_width = 0;
    int64_t frontier = 0;
    int64_t plan_from = -1;   // s2c_parser_snapshot_from: plan the tiles from here only (-1: all)
    size_t n_kept = 0;
    bool late = false;
    bool detached = false;   // made by s2c_parser_detach: snapshot / retain / attach only, no input
    std::vector<uint8_t> blob;   // s2c_parser_pack's output
    // frees the chunks a retain dropped, off the caller's path; one at a time (the next retain
    // joins the previous one first) and joined when the parser is freed
    std::thread freer;
    void free_later(std::vector<std::unique_ptr<Chunk>> v) {
        if (freer.joinable()) freer.join();
        freer = std::thread([](std::vector<std::unique_ptr<Chunk>> w) { w.clear(); }, std::move(v));
    }
    s2c_parser() { chunks.emplace_back(new Chunk()); }
    ~s2c_parser() {
        if (freer.joinable()) freer.join();
    }
};

struct s2c_batch {
    s2c_batch_info info{};
    std::vector<std::string> names;
    std::vector<int64_t> ref_len, ref_off, ref_reads;
    u32buf pc, ops, bq, bx;   // filled entirely by the emitters (resize: no zero-fill)
    std::vector<uint32_t> rs, tiles, items, dense, deep, lp, wtile, rlist, ps;
    std::vector<uint32_t> lly, lpc, lops, lbq, lbx;   // layered windows of the non-dense tiles
    std::vector<uint32_t> lpx;                        // [n_lpieces] px of the layered pieces
    bool layers = false;                               // built (s2c_batch_layers)
    u32buf kmin, kmax;   // host only: global key range of each piece's insertion events
    std::vector<uint8_t> lmot;   // host only: the piece emits a motif > S2C_SHORT_MOTIF bases
    u32buf px;           // [pieces] the non-ACGT SEQ offsets of S2C_PF_XFEW pieces (s2c.h)
    std::vector<uint32_t> dwin;   // [dense][S2C_DWIN_WORDS] the dense items' windows (s2c.h)
    u32buf dpc;                   // [n_dpc][S2C_DPC_WORDS] compact piece records of the dense windows (s2c.h)
    // the dense windows' extension (s2c.h s2c_dense_ext; build_dwin): run records, 'N' events,
    // X-run slots, the rare pieces' records, and each window's {first, count} in the four
    u32buf drun, dnev, dxs, drare, dext;   // (each written whole by build_dwin)
    int64_t n_drun = 0, n_dnev = 0, n_dxs = 0, n_drare = 0;   // records / entries
    // ... and its lean part (s2c.h s2c_dense_lean; build_dwin): the rare pieces' op words, their
    // offsets, each window's {first, count}; the launch's window bytes, lane count and plane pairs
    u32buf rop, roff, drow;
    int64_t n_rop = 0, lean_lds = 0, lean_count = 0, lean_pairs = 1;
};

inline int perr(s2c_parser *p, int code, const std::string &msg) {
    p->err = code;
    p->errmsg = msg;
    return s2c_set_error(code, msg);
}

// n_bases of SEQ planes (bq [word][2], bx [word]), 16 bases at a time: from half-word
// src_half of the source arrays to half-word dst_half of the destination's (reads and pieces
// start at multiples of 16 bases on both sides)
inline void copy_planes(uint32_t *dst_bq, uint32_t *dst_bx, uint64_t dst_half, const uint32_t *src_bq,
                        const uint32_t *src_bx, uint64_t src_half, uint64_t n_bases) {
    const uint16_t *sq = (const uint16_t *)src_bq, *sx = (const uint16_t *)src_bx;
    uint16_t *dq = (uint16_t *)dst_bq, *dx = (uint16_t *)dst_bx;
    for (uint64_t h = 0; h < (n_bases + 15) / 16; h++) {
        const uint64_t s = src_half + h, d = dst_half + h;
        dq[(d >> 1) * 4 + (d & 1)] = sq[(s >> 1) * 4 + (s & 1)];           // p0
        dq[(d >> 1) * 4 + 2 + (d & 1)] = sq[(s >> 1) * 4 + 2 + (s & 1)];   // p1
        dx[d] = sx[s];
    }
}

// the first sorted piece with start word >= w
inline int64_t piece_at_word(const s2c_batch *b, int64_t w) {
    if ((int64_t)b->ps.size() == b->info.n_words + 1 && w <= b->info.n_words) return (int64_t)b->ps[w];
    int64_t lo = 0, hi = b->info.n_pieces;
    while (lo < hi) {
        const int64_t m = (lo + hi) / 2;
        if ((int64_t)(b->pc[4 * m] >> 5) < w) lo = m + 1; else hi = m;
    }
    return lo;
}
// the sorted piece whose op words hold op slot `slot`
inline int64_t piece_of_slot(const s2c_batch *b, uint32_t slot) {
    int64_t lo = 0, hi = b->info.n_pieces - 1;
    while (lo < hi) {
        const int64_t m = (lo + hi + 1) / 2;
        if (b->pc[4 * m + 2] <= slot) lo = m; else hi = m - 1;
    }
    return lo;
}

// ------------------------------------------------------------------ across the units
int parse_window(s2c_parser *p, const char *s, size_t n);   // s2c_parse.cpp: whole lines, in parallel pieces
void insertion_checks(const s2c_parser *p, std::vector<uint8_t> &bad_sym, std::vector<uint8_t> &bad_key);
// s2c_plan.cpp: the planner, and the parts of it a shard or the layer build runs again
int build_batch(s2c_parser *p, s2c_batch **out);
void tile_window(const s2c_batch *b, int64_t K, uint64_t a, uint64_t e, uint32_t *tw);
int64_t dense_bytes(const uint32_t *tw);
bool dense_fits(const uint32_t *tw);
int64_t nwp_of(int64_t tile_max);   // words per pass of the k_tile instantiation for tiles of <= tile_max positions
int64_t count_walked(const uint32_t *pc, int64_t n);
void mark_runs(s2c_batch *b);
void build_dwin(s2c_batch *b);
void build_layers(s2c_batch *b, int64_t G, bool with_dense);

// host phase times on stderr (S2C_HOST_TIMING=1)
struct PhaseClock {
    bool on = getenv("S2C_HOST_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void mark(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[s2c host] %-18s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};
