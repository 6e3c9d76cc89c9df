// s2c_host.cpp — what the host units of libs2c.so share (s2c_host_internal.h: the error
// state, the plan knobs, the worker pools) and the host calls that belong to none of them:
// FASTA body gather, threaded copy, the parsecigar mirror and the ABI layout self-check.
#include "s2c_host_internal.h"

#include <pthread.h>

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;
int s2c_set_error(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
extern "C" const char *s2c_last_error(void) { return g_err.c_str(); }
extern "C" int s2c_abi_version(void) { return S2C_ABI_VERSION; }

// ------------------------------------------------------------------ plan knobs
// Overrides of the batch plan's shape (tile widths, deep-tile items, dense / event routing)
// are measurement tools, not options: they are read only when S2C_DEBUG_PLAN is set, so the
// product plan is the same whatever else the environment holds.
const char *plan_env(const char *name) {
    static const bool debug = getenv("S2C_DEBUG_PLAN") != nullptr;
    return debug ? getenv(name) : nullptr;
}
// The device's compute units (grid shaping of k_tile's launches; s2c_plan_set_cus) — the
// MI355X's 256 until the caller names its device's.
static std::atomic<int64_t> g_plan_cus{256};
int64_t plan_cus() { return g_plan_cus.load(); }
extern "C" int s2c_plan_set_cus(int64_t cus) {
    if (cus <= 0 || cus > 4096) return s2c_set_error(S2C_ERR_ARG, "compute units outside (0, 4096]");
    g_plan_cus.store(cus);
    return S2C_OK;
}

// ------------------------------------------------------------------ host worker pools
// the pool of this process (pools are never destroyed: their threads may outlive main).
// fork: the registry's mutex is held across the fork (pthread_atfork) and a forked child
// forgets the parent's pools (their threads do not exist in it) and makes new ones
WorkerPool &WorkerPool::get(int which) {
    static std::once_flag once;
    std::call_once(once, [] {
        pthread_atfork([] { reg_m().lock(); }, [] { reg_m().unlock(); }, [] {
            for (auto &q : reg()) q = nullptr;
            reg_m().unlock();
        });
    });
    std::lock_guard<std::mutex> lk(reg_m());
    WorkerPool *&q = reg()[which];
    if (!q) q = new WorkerPool();
    return *q;
}
std::mutex &WorkerPool::reg_m() {
    static std::mutex m;
    return m;
}
WorkerPool *(&WorkerPool::reg())[3] {
    static WorkerPool *pools[3] = {nullptr, nullptr, nullptr};
    return pools;
}
void WorkerPool::loop(int t) {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
        go_.wait(lk, [&] { return gen_ != seen; });
        seen = gen_;
        if (t >= want_) continue;
        const std::function<void(int)> *j = job_;
        lk.unlock();
        (*j)(t);
        lk.lock();
        if (--left_ == 0) done_.notify_one();
    }
}
int plan_threads(int64_t n, int64_t grain) {
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<unsigned>(hw ? hw : 1, 16);
    if (const char *e = getenv("S2C_PARSE_THREADS")) nt = std::max(1, std::min(64, atoi(e)));
    if (const char *e = getenv("S2C_PLAN_THREADS")) nt = std::max(1, std::min(64, atoi(e)));   // (the plan's own)
    return (int)std::max<int64_t>(1, std::min<int64_t>(nt, n / std::max<int64_t>(grain, 1)));
}

// FASTA body assembly (:394-418): the tiles' body slots, concatenated in [threshold][tile]
// order (n blocks: raw[starts[i], starts[i] + lens[i]) → dst at the running offset), on the
// host threads for large outputs.  Every block must lie inside raw's raw_len bytes (the
// lengths come from the device: a block past the end is refused, never read).
static int s2c_gather_bodies_impl(const uint8_t *raw, int64_t raw_len, const int64_t *starts, const int64_t *lens,
                                  int64_t n, uint8_t *dst) {
    if (n < 0 || raw_len < 0 || (n > 0 && (!starts || !lens))) return s2c_set_error(S2C_ERR_ARG, "bad gather arguments");
    std::vector<int64_t> off(n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        if (lens[i] < 0 || starts[i] < 0) return s2c_set_error(S2C_ERR_ARG, "negative block");
        if (lens[i] > raw_len || starts[i] > raw_len - lens[i])
            return s2c_set_error(S2C_ERR_ARG, "body block past the end of the device output");
        off[i + 1] = off[i] + lens[i];
    }
    if (off[n] > 0 && (!raw || !dst)) return s2c_set_error(S2C_ERR_ARG, "bad gather arguments");
    par_ranges(plan_threads(off[n], (int64_t)1 << 22), n, [&](int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; i++) memcpy(dst + off[i], raw + starts[i], (size_t)lens[i]);
    });
    return S2C_OK;
}
extern "C" int s2c_gather_bodies(const uint8_t *raw, int64_t raw_len, const int64_t *starts, const int64_t *lens,
                                 int64_t n, uint8_t *dst) {
    return s2c_guarded([&] { return s2c_gather_bodies_impl(raw, raw_len, starts, lens, n, dst); });
}

// n bytes src → dst on the host threads (staging a batch into pinned buffers for its H2D:
// one thread's memcpy runs at a fraction of the memory bandwidth)
static int s2c_copy_bytes_impl(void *dst, const void *src, int64_t n) {
    if (n < 0 || (n > 0 && (!dst || !src))) return s2c_set_error(S2C_ERR_ARG, "bad copy arguments");
    const int64_t pieces = std::max<int64_t>(1, n >> 20);   // 1 MB pieces
    par_ranges(plan_threads(n, (int64_t)1 << 21), pieces, [&](int, int64_t i0, int64_t i1) {
        const int64_t a = n * i0 / pieces, b = n * i1 / pieces;
        memcpy((char *)dst + a, (const char *)src + a, (size_t)(b - a));
    });
    return S2C_OK;
}
extern "C" int s2c_copy_bytes(void *dst, const void *src, int64_t n) {
    return s2c_guarded([&] { return s2c_copy_bytes_impl(dst, src, n); });
}

// ------------------------------------------------------------------ parsecigar (:46-82)
static int s2c_parsecigar_impl(const char *cigar, size_t cigar_len, const char *seq, size_t seq_len,
                              int64_t pos_ref, char *seqout, size_t cap, size_t *seqout_len,
                              int64_t *ins, size_t max_ins, size_t *n_ins) {
    std::vector<uint32_t> toks;
    uint32_t nt = 0;
    int rc = tokenize_cigar(cigar, cigar_len, toks, &nt);
    if (rc) return rc;
    int64_t start = 0, start_ref = pos_ref;
    const int64_t slen = (int64_t)seq_len;
    size_t o = 0, ni = 0;
    auto put = [&](char c) -> bool {
        if (o + 1 >= cap) return false;
        seqout[o++] = c;
        return true;
    };
    for (uint32_t w : toks) {
        const uint32_t op = w & 15u;
        const int64_t l = (int64_t)(w >> 4);
        if (op_bases(op)) {
            int64_t take = start < slen ? std::min(l, slen - start) : 0;
            for (int64_t j = 0; j < take; j++)
                if (!put(seq[start + j])) return s2c_set_error(S2C_ERR_ARG, "seqout buffer too small");
            start += l;
            start_ref += l;
        } else if (op_dash(op)) {
            for (int64_t j = 0; j < l; j++)
                if (!put('-')) return s2c_set_error(S2C_ERR_ARG, "seqout buffer too small");
            start_ref += l;
        } else if (op == S2C_OP_I) {
            int64_t take = start < slen ? std::min(l, slen - start) : 0;
            if (ni < max_ins) {
                ins[3 * ni] = start_ref;
                ins[3 * ni + 1] = std::min(start, slen);
                ins[3 * ni + 2] = take;
            }
            ni++;
            start += l;
        } else if (op == S2C_OP_S) {
            start += l;
        }
    }
    if (cap) seqout[o] = 0;
    *seqout_len = o;
    *n_ins = ni;
    return ni > max_ins ? s2c_set_error(S2C_ERR_ARG, "insertion buffer too small") : S2C_OK;
}
extern "C" int s2c_parsecigar(const char *cigar, size_t cigar_len, const char *seq, size_t seq_len,
                              int64_t pos_ref, char *seqout, size_t cap, size_t *seqout_len,
                              int64_t *ins, size_t max_ins, size_t *n_ins) {
    return s2c_guarded([&] { return s2c_parsecigar_impl(cigar, cigar_len, seq, seq_len, pos_ref, seqout, cap, seqout_len, ins, max_ins, n_ins); });
}

// ------------------------------------------------------------------ ABI layout self-check
// Lets the ctypes mirror (sam2consensus_amd/_lib.py) verify struct sizes/offsets at load.
#include <cstddef>
extern "C" int s2c_layout(int64_t *out, int n) {
    const int64_t v[] = {
        (int64_t)sizeof(s2c_dev), (int64_t)offsetof(s2c_dev, kwin), (int64_t)offsetof(s2c_dev, thresholds),
        (int64_t)offsetof(s2c_dev, fill), (int64_t)offsetof(s2c_dev, runs), (int64_t)offsetof(s2c_dev, n_cols),
        (int64_t)offsetof(s2c_dev, tile_stats), (int64_t)offsetof(s2c_dev, out_cap),
        (int64_t)sizeof(s2c_synth_spec), (int64_t)offsetof(s2c_synth_spec, seed),
        (int64_t)sizeof(s2c_batch_info), (int64_t)sizeof(s2c_batch_arrays), (int64_t)sizeof(s2c_ws_sizes)};
    const int m = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < m; i++) out[i] = v[i];
    return m;
}
