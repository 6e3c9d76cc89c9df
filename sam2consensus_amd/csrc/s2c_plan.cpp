// s2c_plan.cpp — the packed batch and its tile plan from a parser's reads (build_batch, in
// named phases over one BatchPlan), k_tile's layer planner, and the parts of the plan a shard
// runs again (tile windows, rlist, dense windows).
#include "s2c_host_internal.h"

#include <cmath>

namespace {
constexpr int64_t TP_MIN = 256, TP_MAX = 2048;      // tile bounds (positions)
static int64_t deep_tile_min() {   // S2C_DEEP_TILE: the narrowest deep tile (positions)
    static const int64_t v = [] {
        const char *e = plan_env("S2C_DEEP_TILE");
        return e ? std::min<int64_t>(std::max<int64_t>(atoll(e), 64), 2048) : (int64_t)512;
    }();
    return v;
}
constexpr double E_TARGET = 262144.0;                // aligned bases per deep tile
// LDS a shallow tile's window is planned to (one wave per tile, ~10 resident per CU; C5's
// 30x gives 1024-position tiles — measured faster than 512, profiles/r02)
constexpr double DENSE_PLAN_BYTES = 16384.0;
inline uint32_t pow2_at_least(uint64_t v) {
    uint32_t c = 1;
    while (c < v) c <<= 1;
    return c;
}

struct Piece {
    uint64_t gpos;          // global coordinate of seqout char ka
    int64_t ka, kb;         // seqout range
    uint32_t chunk, read;
    uint8_t range, ins, lng;
    uint32_t nslots;        // prefix words + tokens
    uint32_t kmin, kmax;    // global keys of the insertion events it emits (ins)
    uint32_t qlen;          // plane bases: len(SEQ) rounded up to 16
    uint32_t ref;           // reference index
};
}  // namespace

// k_tile<nwp>: the words of a pass, for tiles of up to tile_max positions
int64_t nwp_of(int64_t tile_max) {
    int64_t nwp = 8;
    while (nwp * 32 < tile_max) nwp *= 2;
    return nwp;
}
// k_tile_dense's (its static LDS is 96·nwp + 128 bytes): never below 16
static int64_t dense_nwp_of(int64_t tile_max) { return tile_max <= 512 ? 16 : tile_max <= 1024 ? 32 : 64; }

// pieces walked op by op (neither one token nor long): k_tile's walk queue pays for them
int64_t count_walked(const uint32_t *pc, int64_t n) {
    std::atomic<int64_t> nw{0};
    par_ranges(plan_threads(n, 1 << 18), n, [&](int, int64_t k0, int64_t k1) {
        int64_t m = 0;
        for (int64_t k = k0; k < k1; k++) m += !((pc[4 * k + 3] >> 24) & (S2C_PF_SIMPLE | S2C_PF_LONG));
        nw += m;
    });
    return nw;
}

// px of a piece of read r (s2c.h S2C_PF_XFEW): the SEQ offsets of its first two non-ACGT
// chars when they are all 'N' (no '-': the maxdel rule never needs the plane scan), at most
// two and below 0xFFFF; sets S2C_PF_XFEW in fl.  0xFFFFFFFF otherwise.
static uint32_t xfew_offsets(const Chunk &c, const ReadRec &r, uint32_t &fl) {
    if (!(r.has_x & 1) || (r.has_x & 2)) return 0xFFFFFFFFu;
    const uint16_t *sx = (const uint16_t *)c.bx.data();
    uint32_t off[2] = {0xFFFFu, 0xFFFFu}, nf = 0;
    for (uint64_t h = 0; h < ((uint64_t)r.slen + 15) / 16; h++) {
        uint32_t m = sx[r.q / 16 + h];
        while (m) {
            const uint64_t o = 16 * h + (uint64_t)__builtin_ctz(m);
            m &= m - 1;
            if (o >= r.slen) break;
            if (nf == 2 || o >= 0xFFFFu) return 0xFFFFFFFFu;
            off[nf++] = (uint32_t)o;
        }
    }
    if (nf == 0) return 0xFFFFFFFFu;
    fl |= S2C_PF_XFEW;
    return off[0] | off[1] << 16;
}

// The dense items' windows (S2C_DWIN_WORDS) from the final tile records, and the compact
// piece records of every window (S2C_DPC_WORDS, in window order: a piece of two windows has
// two records, each relative to its own window).
void build_dwin(s2c_batch *b) {
    const size_t nd = b->dense.size() / S2C_ITEM_WORDS;
    b->dwin.assign(std::max<size_t>(nd, 1) * S2C_DWIN_WORDS, 0u);
    std::vector<uint64_t> base(nd + 1, 0);
    for (size_t i = 0; i < nd; i++) {
        const uint32_t t = b->dense[i * S2C_ITEM_WORDS];
        const uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
        uint32_t *o = &b->dwin[i * S2C_DWIN_WORDS];
        const uint32_t v[12] = {t, tw[0], tw[1], tw[8], tw[10], tw[11], tw[13], tw[14], tw[15], tw[16], tw[17], tw[18]};
        for (int k = 0; k < 12; k++) o[k] = v[k];
        o[12] = (uint32_t)base[i];
        base[i + 1] = base[i] + (tw[14] - tw[13]);
    }
    if (base[nd] >= ((uint64_t)1 << 32)) throw std::runtime_error("more than 2^32 dense window pieces");
    b->info.n_dpc = (int64_t)base[nd];
    b->dpc.resize(std::max<uint64_t>(base[nd], 1) * S2C_DPC_WORDS);
    if (!base[nd]) b->dpc[0] = b->dpc[1] = b->dpc[2] = 0;
    // The extension (s2c.h s2c_dense_ext) in two passes over the windows: each window's counts
    // {'N' events, X-run slots, rare pieces} into its dext row, a prefix sum, then the entries
    // with the compact records.  What a piece adds — one for both passes:
    //   ev(r)   an 'N' event of a SIMPLE | XFEW piece at tile-relative position r
    //   xs()    a SIMPLE piece whose non-ACGT chars are read from the planes
    //   rare()  a piece neither SIMPLE nor LONG
    auto classify = [](uint32_t fl, uint32_t rs, uint32_t slen, uint32_t px, uint32_t TL, auto &&ev, auto &&xs, auto &&rare) {
        if (fl & S2C_PF_SIMPLE) {
            if (fl & S2C_PF_XFEW) {
                for (int u = 0; u < 2; u++) {
                    const uint32_t off = (px >> (16 * u)) & 0xFFFFu, r = rs + off - 2048u;   // (r < 0 wraps past TL)
                    if (off < slen && r < TL) ev(r);
                }
            } else if (fl & S2C_PF_X) {
                xs();
            }
        } else if (!(fl & S2C_PF_LONG)) {
            rare();
        }
    };
    b->dext.resize(std::max<size_t>(nd, 1) * S2C_DEXT_WORDS);
    if (!nd) std::fill(b->dext.begin(), b->dext.end(), 0u);
    const int nth = plan_threads((int64_t)nd, 64);
    // (the lean part, s2c.h s2c_dense_lean: each window's rare op words counted here too, and the
    // launch's window bytes and largest lane count reduced over the windows)
    b->drow.resize(std::max<size_t>(nd, 1) * S2C_DLEAN_WORDS);
    std::fill(b->drow.begin(), b->drow.end(), 0u);
    const int64_t NWP = dense_nwp_of(b->info.tile_max), G = 128 / NWP, K = b->info.kwin;
    std::vector<int64_t> lds_t(nth, 0), cnt_t(nth, 0);
    par_ranges(nth, (int64_t)nd, [&](int t, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; i++) {
            const uint32_t *w = &b->dwin[(size_t)i * S2C_DWIN_WORDS];
            const uint32_t T0 = 32 * (w[1] >> 5), TL = 32 * ((w[2] - w[1] + 31) / 32);
            uint32_t nev = 0, nxs = 0, nrare = 0, nrop = 0;
            for (uint32_t k = w[6]; k < w[7]; k++) {
                const uint32_t *pc = &b->pc[4 * (size_t)k];
                classify(pc[3] >> 24, pc[0] - T0 + 2048u, pc[3] & 0xFFFFFFu, b->px[k], TL, [&](uint32_t) { nev++; },
                         [&] { nxs++; }, [&] { nrare++; nrop += pc[6] - pc[2]; });
            }
            uint32_t *x = &b->dext[(size_t)i * S2C_DEXT_WORDS];
            x[1] = w[9] - w[8];
            x[3] = nev;
            x[5] = nxs;
            x[7] = nrare;
            b->drow[(size_t)i * S2C_DLEAN_WORDS + 1] = nrop;
            lds_t[t] = std::max<int64_t>(lds_t[t], S2C_DENSE_LEAN_BYTES((int64_t)(w[9] - w[8]), (int64_t)(w[11] - w[10]),
                                                                         (int64_t)nrare, (int64_t)nrop, NWP));
            // the largest count of a lane (k_tile_dense's mxc): per wave, the record slots its
            // longest lane reads — lane 0 of the word with most candidates — plus the long rounds
            const int64_t W0 = w[1] >> 5, nwords = (w[2] - w[1] + 31) / 32, ntr = (w[5] - w[4] + G - 1) / G;
            for (int64_t wa = 0; wa < nwords; wa += NWP / 2) {
                int64_t nmx = 0;
                for (int64_t W = W0 + wa; W < W0 + std::min(wa + NWP / 2, nwords); W++)
                    nmx = std::max<int64_t>(nmx, ((int64_t)b->rs[W + 1] - (int64_t)b->rs[std::max<int64_t>(W - K, 0)] + G - 1) / G);
                cnt_t[t] = std::max(cnt_t[t], S2C_DENSE_SLOTS(nmx) + ntr);
            }
        }
    });
    b->lean_lds = *std::max_element(lds_t.begin(), lds_t.end());
    b->lean_count = *std::max_element(cnt_t.begin(), cnt_t.end());
    b->lean_pairs = S2C_DENSE_PAIRS(b->lean_count);
    uint64_t nrop_tot = 0;
    uint64_t tot[4] = {0, 0, 0, 0};   // records of drun (each block from an even record: 16 bytes), dnev, dxs, drare
    for (size_t i = 0; i < nd; i++) {
        uint32_t *x = &b->dext[i * S2C_DEXT_WORDS];
        for (int c = 0; c < 4; c++) {
            x[2 * c] = (uint32_t)tot[c];
            tot[c] += c == 0 ? (x[1] + 1u) & ~1u : x[2 * c + 1];
        }
        b->drow[i * S2C_DLEAN_WORDS] = (uint32_t)nrop_tot;
        nrop_tot += b->drow[i * S2C_DLEAN_WORDS + 1];
        if (tot[0] >= ((uint64_t)1 << 31)) throw std::runtime_error("more than 2^31 dense window run records");
    }
    b->n_drun = (int64_t)tot[0];
    b->n_dnev = (int64_t)tot[1];
    b->n_dxs = (int64_t)tot[2];
    b->n_drare = (int64_t)tot[3];
    b->drun.resize(std::max<uint64_t>(tot[0], 2) * 2);
    b->dnev.resize(std::max<uint64_t>(tot[1], 1));
    b->dxs.resize(std::max<uint64_t>(tot[2], 1));
    b->drare.resize(std::max<uint64_t>(tot[3], 1) * S2C_DPC_WORDS);
    if (!tot[0]) std::fill(b->drun.begin(), b->drun.end(), 0u);
    if (!tot[1]) b->dnev[0] = 0;
    if (!tot[2]) b->dxs[0] = 0;
    if (!tot[3]) b->drare[0] = b->drare[1] = b->drare[2] = 0;
    if (nrop_tot >= ((uint64_t)1 << 31)) throw std::runtime_error("more than 2^31 rare op words of dense windows");
    b->n_rop = (int64_t)nrop_tot;
    b->rop.resize(std::max<uint64_t>(nrop_tot, 1));
    b->roff.resize(std::max<uint64_t>(tot[3], 1));
    if (!nrop_tot) b->rop[0] = 0;
    if (!tot[3]) b->roff[0] = 0;
    par_ranges(nth, (int64_t)nd, [&](int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; i++) {
            const uint32_t *w = &b->dwin[(size_t)i * S2C_DWIN_WORDS];
            const uint32_t T0 = 32 * (w[1] >> 5), o0 = w[8], qw0 = w[10], TL = 32 * ((w[2] - w[1] + 31) / 32);
            const uint32_t *x = &b->dext[(size_t)i * S2C_DEXT_WORDS];
            uint32_t *o = &b->dpc[base[i] * S2C_DPC_WORDS];
            uint32_t *run = &b->drun[2 * (size_t)x[0]], *nev = &b->dnev[x[2]], *xs = &b->dxs[x[4]];
            uint32_t *rare = &b->drare[(size_t)x[6] * S2C_DPC_WORDS];
            uint32_t *rop = &b->rop[b->drow[(size_t)i * S2C_DLEAN_WORDS]], *roff = &b->roff[x[6]], ro = 0;
            std::fill(run, run + 2 * (size_t)((x[1] + 1u) & ~1u), 0u);   // (every slot but the SIMPLE pieces')
            for (uint32_t k = w[6]; k < w[7]; k++, o += S2C_DPC_WORDS) {
                const uint32_t *pc = &b->pc[4 * (size_t)k];
                const uint32_t rs = pc[0] - T0 + 2048u, qh = pc[1] - 2 * qw0, nops = pc[6] - pc[2], oj = pc[2] - o0;
                const uint32_t slen = pc[3] & 0xFFFFFFu, fl = pc[3] >> 24;
                if (rs >= 4096u || qh >= 8192u || nops > S2C_DPC_NOPS_MAX || oj >= 8192u || slen > S2C_DPC_SLEN_MAX)
                    throw std::runtime_error("dense window piece beyond the compact record's fields");
                o[0] = rs | qh << 12 | nops << 25;
                o[1] = oj | slen << 13 | fl << 24;
                o[2] = b->px[k];
                if (fl & S2C_PF_SIMPLE) {   // the run k_tile_dense's lean walk writes (rec_enc_b)
                    run[2 * oj] = rs | (rs + slen) << 16;
                    run[2 * oj + 1] = 16u * qh - rs;
                }
                classify(fl, rs, slen, o[2], TL, [&](uint32_t r) { *nev++ = r; }, [&] { *xs++ = oj; },
                         [&] {
                             for (int c = 0; c < S2C_DPC_WORDS; c++) *rare++ = o[c];
                             *roff++ = ro;
                             for (uint32_t j = 0; j < nops; j++) rop[ro++] = b->ops[pc[2] + j];
                         });
            }
        }
    });
}

// Pieces k_tile_dense's compact records cannot hold (len(SEQ) or op slots beyond their
// fields): prefix counts over the sorted pieces, so a tile window [pf0, pf1) holds one iff
// p[pf1] > p[pf0]; such a tile is not dense.
static std::vector<uint32_t> dpc_bad_prefix(const s2c_batch *b) {
    const int64_t NP = b->info.n_pieces;
    std::vector<uint32_t> p(NP + 1, 0);
    const int nt = plan_threads(NP, 1 << 16);
    std::vector<uint32_t> part(nt + 1, 0);
    auto bad = [&](int64_t k) {
        const uint32_t *pc = &b->pc[4 * (size_t)k];
        return (pc[3] & 0xFFFFFFu) > S2C_DPC_SLEN_MAX || pc[6] - pc[2] > S2C_DPC_NOPS_MAX;
    };
    par_ranges(nt, NP, [&](int t, int64_t k0, int64_t k1) {
        uint32_t c = 0;
        for (int64_t k = k0; k < k1; k++) c += bad(k);
        part[t + 1] = c;
    });
    for (int t = 0; t < nt; t++) part[t + 1] += part[t];
    par_ranges(nt, NP, [&](int t, int64_t k0, int64_t k1) {
        uint32_t c = part[t];
        for (int64_t k = k0; k < k1; k++) p[k + 1] = (c += bad(k));
    });
    return p;
}

// The window of tile [a, b): the short pieces starting in words [a/32 - K, ceil(b/32)) — a
// contiguous range of the bucketed pieces — their op slots and base plane words (+1 word for
// the funnel shift of the last one).  Tile words 13-18.
void tile_window(const s2c_batch *b, int64_t K, uint64_t a, uint64_t e, uint32_t *tw) {
    const int64_t pf0 = piece_at_word(b, std::max<int64_t>((int64_t)(a >> 5) - K, 0)), pf1 = piece_at_word(b, (int64_t)((e + 31) >> 5));
    tw[13] = (uint32_t)pf0;
    tw[14] = (uint32_t)pf1;
    tw[15] = b->pc[4 * pf0 + 2];
    tw[16] = b->pc[4 * pf1 + 2];
    tw[17] = pf1 > pf0 ? (uint32_t)(((uint64_t)b->pc[4 * pf0 + 1] * 16) >> 5) : 0u;
    tw[18] = pf1 > pf0 ? (uint32_t)(((uint64_t)b->pc[4 * (pf1 - 1) + 1] * 16 + (b->pc[4 * (pf1 - 1) + 3] & 0xFFFFFFu) + 31) / 32 + 1)
                       : tw[17];
}

// LDS bytes k_tile_dense keeps a tile's window in (s2c_dense.hip), and whether it fits (with
// query offsets of the window's base planes in 17 bits)
int64_t dense_bytes(const uint32_t *tw) {
    return S2C_DENSE_BYTES((int64_t)(tw[16] - tw[15]), (int64_t)(tw[18] - tw[17]));
}
bool dense_fits(const uint32_t *tw) {
    return dense_bytes(tw) <= S2C_DENSE_LDS && (int64_t)(tw[18] - tw[17]) <= S2C_DENSE_QW;
}

// PF_RUNS on the long pieces (the tile long lists read k_reads' run records of them; the
// tile kernels walk every short piece of their windows themselves), and the list of pieces
// k_reads walks (those, and the pieces emitting insertion events).
// k_tile's walk-queue variant (s2c_batch_info walk_queue): at least 1/32 of the pieces walked
// op by op, tiles of <= 1024 positions (the 2048-position instantiation has no LDS for it).
// It also records its finish tiles' short-motif insertion events (LDS event list, s2c_tile.hip).
static int64_t walk_queue_of(const s2c_batch_info &I) {
    return I.n_walked > 0 && 32 * I.n_walked >= I.n_pieces && I.tile_max <= 1024 ? 1 : 0;
}

// The pieces k_reads walks (rlist): first the ones s2c_run needs (n_rlist_run) — long pieces
// listed by non-dense tiles (k_reads writes their run records) and insertion pieces with an
// event k_tile does not record: a motif > S2C_SHORT_MOTIF bases, a long piece, or a key in a
// tile that is not a finish tile (deep / general: k_consensus votes it) or whose window does
// not hold the piece — then the other insertion pieces (the counts-only modes hash every event).
void mark_runs(s2c_batch *b) {
    const int64_t NP = b->info.n_pieces, K = b->info.kwin;
    std::vector<uint8_t> need(NP, 0);
    // long pieces listed by run slot (k_tile's tiles: k_reads writes their runs); a dense
    // tile lists its long pieces themselves (k_tile_dense walks them)
    for (int64_t t = 0; t < b->info.n_tiles && b->info.n_long > 0; t++) {
        const uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
        if (tw[3] & S2C_TILE_DENSE) continue;
        for (uint32_t e = tw[10]; e < tw[11]; e++) need[piece_of_slot(b, b->lp[e])] = 1;
    }
    // (the layers were cut for the instantiation planned, I.walk_queue: a shard whose parent
    // was planned for the non-queue one keeps it, whose chunk holds more plane bytes)
    b->info.walk_queue = walk_queue_of(b->info) && b->info.walk_queue ? 1 : 0;
    static const bool no_tile_events = plan_env("S2C_NO_TILE_EVENTS") != nullptr;   // (A/B: k_reads hashes every event)
    b->info.tile_events = b->info.walk_queue && !no_tile_events ? 1 : 0;
    const bool rec = b->info.tile_events != 0;
    auto tile_takes_events = [&](int64_t k) {   // every event of insertion piece k recorded by k_tile
        const uint32_t fl = b->pc[4 * k + 3] >> 24;
        if (!rec || (fl & S2C_PF_LONG) || ((size_t)k < b->lmot.size() && b->lmot[k]) || b->kmin[k] == 0xFFFFFFFFu) return false;
        const uint32_t t0 = b->wtile[b->kmin[k] >> 5], t1 = b->wtile[b->kmax[k] >> 5];
        if (t0 == 0xFFFFFFFFu || t1 == 0xFFFFFFFFu) return false;
        const int64_t ws = (int64_t)(b->pc[4 * k] >> 5);
        for (uint32_t t = t0; t <= t1; t++) {
            const uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
            const int64_t W0 = tw[0] >> 5, W1 = (tw[1] + 31) >> 5;
            if ((tw[3] & (S2C_TILE_DEEP | S2C_TILE_GENERAL | S2C_TILE_DENSE)) || ws < std::max<int64_t>(W0 - K, 0) || ws >= W1)
                return false;
        }
        return true;
    };
    b->rlist.clear();
    const int nt = plan_threads(NP, 1 << 18);
    std::vector<std::vector<uint32_t>> rl(nt), rx(nt);
    par_ranges(nt, NP, [&](int t, int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++) {
            uint32_t &w3 = b->pc[4 * k + 3];
            if (need[k]) w3 |= (uint32_t)S2C_PF_RUNS << 24;
            else w3 &= ~((uint32_t)S2C_PF_RUNS << 24);
            const bool ins = ((w3 >> 24) & S2C_PF_INS) != 0;
            if (need[k] || (ins && !tile_takes_events(k))) rl[t].push_back((uint32_t)k);
            else if (ins) rx[t].push_back((uint32_t)k);
        }
    });
    for (int t = 0; t < nt; t++) b->rlist.insert(b->rlist.end(), rl[t].begin(), rl[t].end());
    b->info.n_rlist_run = (int64_t)b->rlist.size();
    for (int t = 0; t < nt; t++) b->rlist.insert(b->rlist.end(), rx[t].begin(), rx[t].end());
    b->info.n_rlist = (int64_t)b->rlist.size();
    if (b->rlist.empty()) b->rlist.push_back(0);
}

// ------------------------------------------------------------------ k_tile's layer plan
// k_tile stages a tile's window in LDS one LAYER at a time: the window's start words
// [S0, S1) (S0 = max(W0 - K, 0)) are its segments, and layer l of nl takes from segment s
// its short pieces among [ps[s] + n_s*l/nl, ps[s] + n_s*(l+1)/nl) — every layer touches
// every word of the tile alike.  The layers are copied contiguously (build_layers), each
// one 16-byte aligned in every array, so a layer is one DMA per array.  A layer must fit
// the chunk (S2C_CHUNK_*): pieces, plane / non-ACGT / op bytes, run records, and per word
// <= S2C_CHUNK_LANE_RECS records per counting lane.
struct PieceBlocks {          // prefix sums over the sorted pieces (mod 2^32: differences exact)
    u32buf n, h, o;   // short pieces, their plane half-words, their op words (filled by the threads: no zero-fill)
};
static inline uint32_t piece_half_words(uint32_t w3) { return ((w3 & 0xFFFFFFu) + 15u) / 16u; }
static void piece_blocks(const s2c_batch *b, PieceBlocks &B) {
    const int64_t NP = b->info.n_pieces;
    B.n.resize(NP + 1);
    B.h.resize(NP + 1);
    B.o.resize(NP + 1);
    B.n[0] = B.h[0] = B.o[0] = 0;
    const int nt = plan_threads(NP, 1 << 18);
    std::vector<uint32_t> sn(nt + 1, 0), sh(nt + 1, 0), so(nt + 1, 0);
    par_ranges(nt, NP, [&](int t, int64_t k0, int64_t k1) {   // range sums (mod 2^32) ...
        uint32_t n = 0, h = 0, o = 0;
        for (int64_t k = k0; k < k1; k++) {
            const uint32_t w3 = b->pc[4 * k + 3];
            const bool s = !((w3 >> 24) & S2C_PF_LONG);
            n += s ? 1u : 0u;
            h += s ? piece_half_words(w3) : 0u;
            o += s ? b->pc[4 * k + 6] - b->pc[4 * k + 2] : 0u;
            B.n[k + 1] = n; B.h[k + 1] = h; B.o[k + 1] = o;
        }
        sn[t + 1] = n; sh[t + 1] = h; so[t + 1] = o;
    });
    for (int t = 0; t < nt; t++) { sn[t + 1] += sn[t]; sh[t + 1] += sh[t]; so[t + 1] += so[t]; }
    par_ranges(nt, NP, [&](int t, int64_t k0, int64_t k1) {   // ... then each range from its base
        for (int64_t k = k0; k < k1; k++) { B.n[k + 1] += sn[t]; B.h[k + 1] += sh[t]; B.o[k + 1] += so[t]; }
    });
}

// Segment s's pieces [p0, p0 + n) cut into nl slices at p0 + floor((n·l + r_s) / nl), the
// rotation r_s = (s · 2654435761) mod nl spreading the segments' rounding (a segment of fewer
// pieces than layers puts them in different layers for different segments, not all in the
// last one).
struct LayerSeg { uint64_t p0, n, s; };
static inline uint64_t layer_rot(uint64_t s, uint64_t nl) { return (s * 2654435761ull) % nl; }
static inline uint64_t layer_lo(const LayerSeg &g, uint64_t l, uint64_t nl) {
    return g.p0 + (g.n * l + layer_rot(g.s, nl)) / nl;
}
// c[l] = layer_lo(g, l, nl) for l = 0..nl with one division (floor((n·l + r) / nl) stepped:
// the remainder grows by n mod nl < nl per layer, so at most one carry per step)
static inline void layer_cuts(const LayerSeg &g, uint64_t nl, uint64_t *c) {
    const uint64_t qn = g.n / nl, rn = g.n % nl;
    uint64_t q = 0, rem = layer_rot(g.s, nl);
    for (uint64_t l = 0; l <= nl; l++) {
        c[l] = g.p0 + q;
        q += qn;
        rem += rn;
        if (rem >= nl) { rem -= nl; q++; }
    }
}
// the cut points of every segment of a tile (segment i's at cuts[i·(nl+1) ..])
static void tile_cuts(const std::vector<LayerSeg> &seg, uint64_t nl, std::vector<uint64_t> &cuts) {
    cuts.resize(seg.size() * (nl + 1));
    for (size_t i = 0; i < seg.size(); i++) layer_cuts(seg[i], nl, &cuts[i * (nl + 1)]);
}

// a layer's plane bytes in k_tile<nwp, wq>'s chunk, nwp = 64 / G (s2c.h S2C_CHUNK_QBYTES_OF)
static inline uint64_t chunk_qbytes(int64_t G, int64_t wq) { return S2C_CHUNK_QBYTES_OF(64 / std::max<int64_t>(G, 1), wq); }

static bool layer_fits(const PieceBlocks &B, size_t NS, const std::vector<uint64_t> &cuts, int64_t S0, int64_t W0,
                       int64_t W1, int64_t K, int64_t G, int64_t wq, uint64_t l, uint64_t nl, std::vector<int64_t> &recs) {
    uint64_t np = 0, nh = 0, rc = 0;
    for (size_t i = 0; i < NS; i++) {
        const uint64_t lo = cuts[i * (nl + 1) + l], hi = cuts[i * (nl + 1) + l + 1];
        recs[i] = (int64_t)(uint32_t)(B.o[hi] - B.o[lo]);
        np += (uint32_t)(B.n[hi] - B.n[lo]);
        nh += (uint32_t)(B.h[hi] - B.h[lo]);
        rc += (uint64_t)recs[i];
    }
    // (planes: 8 B per 2 half-words, + the funnel word, rounded to 16 B; non-ACGT: half)
    const uint64_t qb = chunk_qbytes(G, wq);
    if (np > S2C_CHUNK_PIECES || 4 * nh + 32 > qb || 2 * nh + 32 > qb / 2 ||
        4 * rc + 32 > S2C_CHUNK_OBYTES || rc > S2C_CHUNK_RECS)
        return false;
    for (int64_t W = W0; W < W1; W++) {
        int64_t r = 0;
        for (int64_t s = std::max(W - K, S0); s <= W; s++) r += recs[s - S0];
        if (r > (int64_t)S2C_CHUNK_LANE_RECS * G) return false;
    }
    return true;
}

// nl of tile [a, e) (0: a layer cannot fit, i.e. one piece alone exceeds the chunk)
static int64_t plan_layers(const s2c_batch *b, const PieceBlocks &B, int64_t K, uint64_t a, uint64_t e, int64_t G, int64_t wq) {
    const int64_t W0 = (int64_t)(a >> 5), W1 = (int64_t)((e + 31) >> 5), S0 = std::max<int64_t>(W0 - K, 0);
    std::vector<LayerSeg> seg;
    uint64_t tp = 0, th = 0, tr = 0, maxn = 0;
    for (int64_t s = S0; s < W1; s++) {
        const uint64_t p0 = b->ps[s], n = b->ps[s + 1] - p0;
        seg.push_back({p0, n, (uint64_t)s});
        tp += (uint32_t)(B.n[p0 + n] - B.n[p0]);
        th += (uint32_t)(B.h[p0 + n] - B.h[p0]);
        tr += (uint32_t)(B.o[p0 + n] - B.o[p0]);
        maxn = std::max(maxn, n);
    }
    if (maxn == 0) return 1;
    std::vector<int64_t> recs(seg.size());
    std::vector<uint64_t> cuts;
    // the fewest layers that fit (each layer costs its DMA round trips and barriers whatever
    // it holds: C3 −2.5 %, C4 −1.2 % against a start 10 % above the capacity bound): from the
    // capacity bound up in growing steps, then bisected back to the first fitting count
    uint64_t nl = std::max<uint64_t>({1, tp / S2C_CHUNK_PIECES + 1, (4 * th) / chunk_qbytes(G, wq) + 1,
                                      tr / S2C_CHUNK_RECS + 1});
    // (past maxn layers the rotation still spreads the segments' pieces: up to 4 per piece)
    const uint64_t nlmax = std::max<uint64_t>(maxn, 4 * tp);
    nl = std::min(nl, nlmax);
    auto fits = [&](uint64_t n) {
        tile_cuts(seg, n, cuts);
        bool ok = true;
        for (uint64_t l = 0; l < n && ok; l++) ok = layer_fits(B, seg.size(), cuts, S0, W0, W1, K, G, wq, l, n, recs);
        return ok;
    };
    uint64_t bad = nl - 1;   // (a count known not to fit, or the bound − 1)
    for (;; nl = nl + 1 + nl / 16) {
        if (nl > nlmax) nl = nlmax;
        if (fits(nl)) break;
        if (nl == nlmax) return 0;
        bad = nl;
    }
    while (nl - bad > 1) {   // (bisection: a count that fits is always the one kept, monotone or not)
        const uint64_t mid = bad + (nl - bad) / 2;
        if (fits(mid)) nl = mid;
        else bad = mid;
    }
    return (int64_t)nl;
}

// Whether tile tw's window, read in place from the sorted arrays (one layer: tile word 20 =
// S2C_LY_MAIN), fits k_tile's chunk: its pieces (long ones included: their op words and
// planes are in the range) [pf0, pf1), op words [o0, o1), plane words [qw0, qw1) at their
// arrays' own 16-byte phases.
static bool main_window_fits(const s2c_batch *b, const uint32_t *tw, int64_t K, int64_t G) {
    const uint64_t np = tw[14] - tw[13], no = tw[16] - tw[15], nq = tw[18] - tw[17];
    const uint64_t qb = chunk_qbytes(G, b->info.walk_queue);   // (the instantiation that runs it)
    if (np > S2C_CHUNK_PIECES || no > S2C_CHUNK_RECS || 4 * no + 32 > S2C_CHUNK_OBYTES || 8 * nq + 32 > qb ||
        4 * nq + 32 > qb / 2)
        return false;
    const int64_t W0 = tw[0] >> 5, W1 = (tw[1] + 31) >> 5;
    for (int64_t W = W0; W < W1; W++)
        if ((int64_t)b->rs[W + 1] - (int64_t)b->rs[std::max<int64_t>(W - K, 0)] > (int64_t)S2C_CHUNK_LANE_RECS * G)
            return false;
    return true;
}

// The layered windows (s2c.h, tile words 19-20): for every tile whose window is not read in
// place, its nl layers in order, each a copy of its short pieces (records with re-based qh /
// opoff, op words, base planes and non-ACGT words of SEQ[0:len], len the record's length
// field), contiguous (the kernel's DMA takes each array's 16-byte phase).
void build_layers(s2c_batch *b, int64_t G, bool with_dense) {
    s2c_batch_info &I = b->info;
    const int64_t NT = I.n_tiles, K = I.kwin;
    std::vector<uint64_t> lyp, lyo, lyh;   // layer starts: pieces, op words, plane half-words
    lyp.push_back(0); lyo.push_back(0); lyh.push_back(0);
    struct TL { int64_t t, ly0, nl; };
    std::vector<TL> tl;
    for (int64_t t = 0; t < NT; t++) {
        uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
        if ((!with_dense && (tw[3] & S2C_TILE_DENSE)) || tw[19] == 0) {   // (k_tile_dense reads its window in
            tw[20] = S2C_LY_NONE;                                          //  place; a ranged snapshot's unplanned tile)
            continue;
        }
        if (tw[19] == 1 && main_window_fits(b, tw, K, G)) {
            tw[20] = S2C_LY_MAIN;
            continue;
        }
        tl.push_back({t, 0, (int64_t)tw[19]});
    }
    PieceBlocks B;
    if (!tl.empty()) piece_blocks(b, B);
    for (TL &T : tl) {
        uint32_t *tw = &b->tiles[(size_t)T.t * S2C_TILE_WORDS];
        const int64_t nl = T.nl, W0 = tw[0] >> 5, W1 = (tw[1] + 31) >> 5, S0 = std::max<int64_t>(W0 - K, 0);
        T.ly0 = (int64_t)lyp.size() - 1;
        tw[20] = (uint32_t)T.ly0;
        std::vector<LayerSeg> seg;
        for (int64_t s = S0; s < W1; s++) seg.push_back({b->ps[s], (uint64_t)(b->ps[s + 1] - b->ps[s]), (uint64_t)s});
        std::vector<uint64_t> cuts;
        tile_cuts(seg, (uint64_t)nl, cuts);
        for (int64_t l = 0; l < nl; l++) {
            uint64_t np = 0, no = 0, nh = 0;
            for (size_t i = 0; i < seg.size(); i++) {
                const uint64_t lo = cuts[i * (nl + 1) + l], hi = cuts[i * (nl + 1) + l + 1];
                np += (uint32_t)(B.n[hi] - B.n[lo]);
                no += (uint32_t)(B.o[hi] - B.o[lo]);
                nh += (uint32_t)(B.h[hi] - B.h[lo]);
            }
            lyp.push_back(lyp.back() + np);
            lyo.push_back(lyo.back() + no);
            lyh.push_back(lyh.back() + nh);
        }
    }
    const int64_t NL = (int64_t)lyp.size() - 1;
    I.n_layers = NL;
    I.layers_dense = with_dense ? 1 : 0;
    I.n_lpieces = (int64_t)lyp.back();
    I.n_lops = (int64_t)lyo.back();
    I.n_lqwords = (int64_t)(lyh.back() / 2) + 2;   // (+ the funnel word after the last)
    b->lly.assign(4 * (size_t)(NL + 1), 0u);
    for (int64_t L = 0; L <= NL; L++) {
        b->lly[4 * L] = (uint32_t)lyp[L];
        b->lly[4 * L + 1] = (uint32_t)lyo[L];
        b->lly[4 * L + 2] = (uint32_t)lyh[L];
    }
    b->lpc.assign(4 * (size_t)(I.n_lpieces + 1), 0u);
    b->lops.assign(std::max<int64_t>(I.n_lops, 4), 0u);
    b->lbq.assign(2 * (size_t)I.n_lqwords, 0u);
    b->lbx.assign((size_t)I.n_lqwords, 0u);
    b->lpx.assign(std::max<int64_t>(I.n_lpieces, 1), 0xFFFFFFFFu);
    {
        uint32_t *sp = &b->lpc[4 * (size_t)I.n_lpieces];   // sentinel
        sp[1] = (uint32_t)lyh.back();
        sp[2] = (uint32_t)lyo.back();
    }
    auto copy_tiles = [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const TL &T = tl[i];
            const uint32_t *tw = &b->tiles[(size_t)T.t * S2C_TILE_WORDS];
            const int64_t W0 = tw[0] >> 5, W1 = (tw[1] + 31) >> 5, S0 = std::max<int64_t>(W0 - K, 0);
            std::vector<LayerSeg> seg;
            for (int64_t s = S0; s < W1; s++) seg.push_back({b->ps[s], (uint64_t)(b->ps[s + 1] - b->ps[s]), (uint64_t)s});
            std::vector<uint64_t> cuts;
            tile_cuts(seg, (uint64_t)T.nl, cuts);
            for (int64_t l = 0; l < T.nl; l++) {
                const int64_t L = T.ly0 + l;
                uint64_t kp = lyp[L], ko = lyo[L], kh = lyh[L];
                for (size_t i = 0; i < seg.size(); i++) {
                    const uint64_t lo = cuts[i * (T.nl + 1) + l], hi = cuts[i * (T.nl + 1) + l + 1];
                    for (uint64_t k = lo; k < hi; k++) {
                        const uint32_t *pr = &b->pc[4 * k];
                        if ((pr[3] >> 24) & S2C_PF_LONG) continue;
                        const uint32_t no = pr[6] - pr[2], nh = piece_half_words(pr[3]);
                        uint32_t *dp = &b->lpc[4 * kp];
                        dp[0] = pr[0];
                        dp[1] = (uint32_t)kh;
                        dp[2] = (uint32_t)ko;
                        dp[3] = pr[3];
                        b->lpx[kp] = b->px[k];
                        memcpy(&b->lops[ko], &b->ops[pr[2]], 4 * (size_t)no);
                        copy_planes(b->lbq.data(), b->lbx.data(), kh, b->bq.data(), b->bx.data(), pr[1], 16 * (uint64_t)nh);
                        kp++;
                        ko += no;
                        kh += nh;
                    }
                }
            }
        }
    };
    const size_t NTL = tl.size();
    unsigned hw = std::thread::hardware_concurrency();
    const int nt = (int)std::max<size_t>(1, std::min<size_t>(std::min<unsigned>(hw ? hw : 1, 16), NTL / 64));
    par_ranges(nt, (int64_t)NTL, [&](int, int64_t k0, int64_t k1) { copy_tiles((size_t)k0, (size_t)k1); });
}

// Layers per work item of a deep tile: IL = 64 per-wave layers (16 per wave), S2C_ITEM_LAYERS overrides.
static int64_t item_layers() {
    static const int64_t il = [] {
        const char *e = plan_env("S2C_ITEM_LAYERS");
        return e ? std::max<int64_t>(4, atoll(e)) : (int64_t)64;
    }();
    return il;
}
// Work items of a tile of nl layers: {tile, c, l0, l1}, enough that each one's run records
// per word stay <= S2C_ITEM_RECS (its u16 histogram) and, past 2·IL layers, an item takes
// <= IL (parallelism for the deep tiles: C4's 16.5 kb at 100,000x).
// The bound covers everything an item adds to a position's u16 halves: per word W, the run
// records of its layers' short pieces starting in words W - K .. W, and its share of the tile's
// long list (item c of nch counts entries [nlg·c/nch, nlg·(c+1)/nch)) — at most its entries, and
// at most the long pieces over W (lw[W]), since a piece's runs cover a position once.  A tile
// whose long runs alone pass the bound gets more items than layers (the later ones' layer
// ranges are empty) and so becomes deep.  0: no count of items keeps the bound (an error, not
// reached: an item of one layer and one long-list entry holds <= S2C_CHUNK_RECS + 1).
static int64_t plan_items(const s2c_batch *b, const PieceBlocks &B, int64_t K, uint64_t a, uint64_t e, int64_t nl, int64_t IL,
                          int64_t nlg, const uint32_t *lw) {
    if (nl <= 1 && nlg == 0) return 1;   // (one layer and no long run: its records fit the chunk)
    const int64_t W0 = (int64_t)(a >> 5), W1 = (int64_t)((e + 31) >> 5), S0 = std::max<int64_t>(W0 - K, 0);
    std::vector<LayerSeg> seg;
    for (int64_t s = S0; s < W1; s++) seg.push_back({b->ps[s], (uint64_t)(b->ps[s + 1] - b->ps[s]), (uint64_t)s});
    std::vector<uint64_t> cuts;
    tile_cuts(seg, (uint64_t)nl, cuts);
    // the short pieces' op slots before each cut (the records between two cuts: their difference)
    for (uint64_t &c : cuts) c = B.o[c];
    const uint64_t stride = (uint64_t)nl + 1;
    const int64_t nmax = std::max(nl, nlg);
    int64_t nch = nl > 2 * IL ? (nl + IL - 1) / IL : 1;
    if (nlg > S2C_ITEM_RECS && *std::max_element(lw + W0, lw + W1) > S2C_ITEM_RECS)   // (the share alone must fit)
        nch = std::max<int64_t>(nch, (nlg + S2C_ITEM_RECS - 1) / S2C_ITEM_RECS);
    for (;; nch++) {
        const int64_t lshare = (nlg + nch - 1) / nch;
        bool ok = true;
        for (int64_t c = 0; c < nch && ok; c++) {
            const uint64_t l0 = (uint64_t)(c * nl / nch), l1 = (uint64_t)((c + 1) * nl / nch);
            for (int64_t W = W0; W < W1 && ok; W++) {
                int64_t r = std::min<int64_t>(lshare, lw[W]);
                for (int64_t s = std::max(W - K, S0); s <= W; s++) {
                    const uint64_t *cs = &cuts[(uint64_t)(s - S0) * stride];
                    r += (uint32_t)(cs[l1] - cs[l0]);
                }
                ok = r <= S2C_ITEM_RECS;
            }
        }
        if (ok) return nch;
        if (nch >= nmax) return 0;
    }
}

// ------------------------------------------------------------------ build_batch
namespace {
struct Tile { int64_t a, b, ref; };

// What the phases of one build_batch hand to each other; each phase runs once, in
// build_batch's order (the members are listed in the order the phases fill them).
struct BatchPlan {
    explicit BatchPlan(s2c_parser *parser) : p(parser) {}
    s2c_parser *p;
    std::unique_ptr<s2c_batch> guard{new s2c_batch()};
    s2c_batch *b = guard.get();
    s2c_batch_info &I = b->info;
    const int64_t R = (int64_t)p->ref_names.size();
    std::vector<std::unique_ptr<Chunk>> &CH = p->chunks;
    int64_t NW = 0;                                  // 32-position words of the padded references
    std::vector<Piece, uninit_alloc<Piece>> pcs;     // the pieces, file order
    std::vector<int64_t> ref_span;                   // counted positions per reference
    int64_t NP = 0;
    int ntw = 1;                                     // host threads of the per-piece loops
    int64_t S = 64, K = 0;                           // short pieces' span limit; window lookback (words)
    std::vector<uint32_t, uninit_alloc<uint32_t>> order;        // sorted (by start word) → file order
    std::vector<uint64_t, uninit_alloc<uint64_t>> ooff, qoff;   // op-word / plane-base offsets, sorted order
    uint64_t NOPS = 0, NQ = 0;
    std::vector<Tile> tiles;
    int64_t tile_max = S2C_POS_ALIGN;
    int64_t tile_force = 0;   // diagnostic override (S2C_TILE_POS, a multiple of 64 in [64, 2048])
    const bool no_dense = plan_env("S2C_NO_DENSE") != nullptr;   // diagnostic: every tile through k_tile
    std::vector<int64_t> longs;                      // sorted indices of the long pieces
    int64_t P0 = 0, P1 = INT64_MAX;                  // the planned tiles (a whole batch: every tile)
    int64_t dense_cap = S2C_DENSE_LDS;
    int64_t NT = 0;
    std::vector<uint32_t> lcnt;                      // long-list CSR by tile
    std::vector<uint32_t> lwords;                    // long pieces over each word (plan_items' bound)
    std::vector<uint32_t> nshort, nlong, nev;        // per tile: insertion events by motif class, and all
    std::vector<uint64_t> ccap;                      // per tile: Σ motif lengths
    int64_t nwp = 8, G = 8, lcols = 0;               // k_tile<nwp>; counting lanes per word; its LDS columns
    PieceBlocks PB;
    // per tile (0: an unplanned tile): layers, items, the most candidate runs of a word, window run slots
    std::vector<int64_t> t_nl, t_nch, t_maxc, t_wruns;
    std::vector<uint32_t> dbad;                      // dpc_bad_prefix: pieces the compact records cannot hold

    bool planned(int64_t t) const { return t >= P0 && t < P1; }
    template <class Fn> void for_long(Fn fn) const;
    int read_pieces(uint32_t ci, uint32_t ri, Piece *dst, int64_t *span, int64_t *nrd) const;
    void emit_pieces(int64_t k0, int64_t k1);
    bool is_dense_tile(int64_t t) const;

    int layout();
    int pieces();
    void window();
    void bucket();
    void offsets();
    int alloc();
    void run_slots();
    void tile_widths();
    void plan_range();
    void split_dense_outliers();
    void tile_words();
    void long_lists();
    void insertion_plan();
    int tile_plans();
    void shape_item_grid();
    int tile_records();
    void long_lists_by_kind();
};

// the reformat-phase checks (:284-294), refs in header order: motif symbols (KeyError, :287)
// are checked for every key before any key's coverage lookup (IndexError, :294)
int check_insertions(const s2c_parser *p) {
    std::vector<uint8_t> bad_sym, bad_key;
    insertion_checks(p, bad_sym, bad_key);
    for (size_t r = 0; r < p->ref_names.size(); r++) {
        if (bad_sym[r]) return s2c_set_error(S2C_ERR_KEY, "KeyError: insertion base not in -ACGNT (:287)");
        if (bad_key[r]) return s2c_set_error(S2C_ERR_INDEX, "IndexError: insertion key out of range (:294)");
    }
    return S2C_OK;
}

// ---- the reference layout and the parse's totals
int BatchPlan::layout() {
    b->names = p->ref_names;
    b->ref_len = p->ref_len;
    b->ref_off.resize(R);
    b->ref_reads.assign(R, 0);
    int64_t g = 0;
    for (int64_t r = 0; r < R; r++) {
        b->ref_off[r] = g;
        g = align_up(g + p->ref_len[r], S2C_POS_ALIGN);
    }
    const int64_t Lpad = std::max<int64_t>(g, S2C_POS_ALIGN);
    if (Lpad >= ((int64_t)1 << 32) - 4096) return s2c_set_error(S2C_ERR_LIMIT, "more than 2^32 reference positions");
    NW = Lpad / 32;
    I.n_refs = R;
    I.padded_len = Lpad;
    I.n_words = NW;
    I.word_lo = 0;
    I.word_hi = NW;
    for (int64_t r = 0; r < R; r++) I.total_len += p->ref_len[r];
    I.header_lines = p->header_lines;
    for (auto &cp : CH) {
        I.lines_total += cp->lines_total;
        I.reads_mapped += cp->reads_mapped;
        I.aligned_bases += cp->aligned;
        I.query_bases += cp->qbases;
        I.n_tokens += cp->ntokens;
    }
    return S2C_OK;
}

// the pieces of read ri of chunk ci into dst (nullptr: count only); returns how many
int BatchPlan::read_pieces(uint32_t ci, uint32_t ri, Piece *dst, int64_t *span, int64_t *nrd) const {
    const Chunk &c = *CH[ci];
    const ReadRec &r = c.reads[ri];
    const int64_t L = p->ref_len[r.ref], off = b->ref_off[r.ref];
    bool any_key = false;   // an event the consensus can emit (key >= 0)
    uint64_t kmin = ~0ull, kmax = 0;
    for (uint32_t e = r.ev0; e < r.ev0 + r.nev; e++)
        if (c.ev[e].key >= 0) {
            any_key = true;
            kmin = std::min<uint64_t>(kmin, (uint64_t)(off + c.ev[e].key));
            kmax = std::max<uint64_t>(kmax, (uint64_t)(off + c.ev[e].key));
        }
    Piece tmp[2];
    int n = 0;
    if (r.kc0 >= 0) {
        const int64_t pa = r.pos0 + r.kc0;
        if (pa < 0) {
            const int64_t kb = std::min(r.kc1, -r.pos0);
            tmp[n++] = {(uint64_t)(off + L + pa), r.kc0, kb, ci, ri, 1, 0, 0, 0, 0, 0, 0, 0};
            if (r.kc1 > -r.pos0) tmp[n++] = {(uint64_t)off, -r.pos0, r.kc1, ci, ri, 1, 0, 0, 0, 0, 0, 0, 0};
        } else {
            const bool whole = r.kc0 == 0 && r.kc1 == r.klen;
            tmp[n++] = {(uint64_t)(off + pa), r.kc0, r.kc1, ci, ri, (uint8_t)!whole, 0, 0, 0, 0, 0, 0, 0};
        }
        nrd[r.ref] += n;
    }
    if (any_key) {   // (a read with events but nothing counted: a zero-span piece at its first key)
        if (n == 0) tmp[n++] = {kmin, 0, 0, ci, ri, 1, 0, 0, 0, 0, 0, 0, 0};
        tmp[0].ins = 1;
        tmp[0].kmin = (uint32_t)kmin;
        tmp[0].kmax = (uint32_t)kmax;
    }
    for (int k = 0; k < n; k++) {
        span[r.ref] += tmp[k].kb - tmp[k].ka;
        tmp[k].nslots = r.ntok + (tmp[k].range ? 2u : 0u) + (tmp[k].ins ? 3u : 0u);
        tmp[k].qlen = (uint32_t)align_up(r.slen, 16);
        tmp[k].ref = r.ref;
        if (dst) dst[k] = tmp[k];
    }
    return n;
}

// ---- pieces: the counted range of each read, split at the POS<=0 wrap (:212), plus a
//      zero-span piece for a read whose insertion events have nothing counted; in file
//      order (chunk by chunk), counted and then written by the host threads ----
int BatchPlan::pieces() {
    const int64_t NC = (int64_t)CH.size();
    std::vector<int64_t> chof(NC + 1, 0);
    const int ntp = plan_threads(NC, 1);
    std::vector<std::vector<int64_t>> tspan(ntp, std::vector<int64_t>(R, 0)), treads(ntp, std::vector<int64_t>(R, 0));
    {
        std::atomic<int64_t> nextc{0};
        par_ranges(ntp, ntp, [&](int t, int64_t, int64_t) {   // pass 1: pieces per chunk
            std::vector<int64_t> sp(R, 0), rd(R, 0);
            for (int64_t ci; (ci = nextc++) < NC;) {
                int64_t n = 0;
                for (uint32_t ri = 0; ri < (uint32_t)CH[ci]->reads.size(); ri++) n += read_pieces((uint32_t)ci, ri, nullptr, sp.data(), rd.data());
                chof[ci + 1] = n;
            }
            (void)t;
        });
    }
    for (int64_t ci = 0; ci < NC; ci++) chof[ci + 1] += chof[ci];
    pcs.resize((size_t)chof[NC]);
    {
        std::atomic<int64_t> nextc{0};
        par_ranges(ntp, ntp, [&](int t, int64_t, int64_t) {   // pass 2: written in place
            for (int64_t ci; (ci = nextc++) < NC;) {
                Piece *dst = pcs.data() + chof[ci];
                for (uint32_t ri = 0; ri < (uint32_t)CH[ci]->reads.size(); ri++)
                    dst += read_pieces((uint32_t)ci, ri, dst, tspan[t].data(), treads[t].data());
            }
        });
    }
    ref_span.assign(R, 0);
    for (int t = 0; t < ntp; t++)
        for (int64_t r = 0; r < R; r++) {
            ref_span[r] += tspan[t][r];
            b->ref_reads[r] += treads[t][r];
        }
    NP = (int64_t)pcs.size();
    if (NP >= ((int64_t)1 << 32) - 2) return s2c_set_error(S2C_ERR_LIMIT, "more than 2^32 pieces (split the input)");
    I.n_pieces = NP;
    ntw = plan_threads(NP, 1 << 18);
    return S2C_OK;
}

// ---- window: pieces up to S positions are short (reached from the run-slot CSR of the
//      kwin + 1 words before a word); the rare longer ones go to the tile long lists ----
void BatchPlan::window() {
    {
        std::vector<std::vector<int64_t>> th(ntw, std::vector<int64_t>(4097, 0));
        par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; k++) th[t][std::min<int64_t>(pcs[k].kb - pcs[k].ka, 4096)]++;
        });
        std::vector<int64_t> hist(4097, 0);
        for (int t = 0; t < ntw; t++)
            for (int s = 0; s <= 4096; s++) hist[s] += th[t][s];
        int64_t above = NP, lim = NP / 1000;
        for (int64_t s = 0; s <= 4096; s++) {
            above -= hist[s];
            if (s >= 64 && above <= lim) { S = s; break; }
        }
        S = std::min<int64_t>(S, 1024);
    }
    {
        std::vector<int64_t> tk(ntw, 0);
        par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
            int64_t kk = 0;
            for (int64_t k = k0; k < k1; k++) {
                Piece &q = pcs[k];
                const int64_t span = q.kb - q.ka;
                // long: a span past the window, or a piece too big for a quarter of k_tile's
                // per-wave chunk (its runs then come from k_reads through the long lists)
                q.lng = span > S || q.nslots > S2C_CHUNK_RECS / 4 || 4 * (uint64_t)(q.qlen / 16) + 32 > S2C_CHUNK_QBYTES / 4;
                if (!q.lng && span > 0) kk = std::max<int64_t>(kk, (int64_t)(((q.gpos + span - 1) >> 5) - (q.gpos >> 5)));
            }
            tk[t] = kk;
        });
        for (int t = 0; t < ntw; t++) K = std::max(K, tk[t]);
    }
    I.kwin = K;
}

// ---- bucket the pieces by start word (counting sort, stable in file order), and the piece CSR
void BatchPlan::bucket() {
    order.resize(NP);
    {
        std::atomic<bool> sorted{true};   // (coordinate-sorted input: already in word order)
        par_ranges(ntw, NP, [&](int, int64_t k0, int64_t k1) {
            for (int64_t k = std::max<int64_t>(k0, 1); k < k1 && sorted; k++)
                if ((pcs[k].gpos >> 5) < (pcs[k - 1].gpos >> 5)) sorted = false;
        });
        if (sorted) {
            par_ranges(ntw, NP, [&](int, int64_t k0, int64_t k1) {
                for (int64_t k = k0; k < k1; k++) order[k] = (uint32_t)k;
            });
        } else if ((uint64_t)(NW + 1) * (uint64_t)ntw <= ((uint64_t)1 << 27)) {
            // per-range histograms, word-major offsets, stable scatter (ranges in file order)
            std::vector<std::vector<uint32_t>> cnt(ntw);
            par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
                cnt[t].assign(NW + 1, 0u);
                for (int64_t k = k0; k < k1; k++) cnt[t][pcs[k].gpos >> 5]++;
            });
            uint64_t run = 0;
            for (int64_t w = 0; w <= NW; w++)
                for (int t = 0; t < ntw; t++) {
                    const uint32_t c = cnt[t][w];
                    cnt[t][w] = (uint32_t)run;
                    run += c;
                }
            par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
                for (int64_t k = k0; k < k1; k++) order[cnt[t][pcs[k].gpos >> 5]++] = (uint32_t)k;
            });
        } else {
            std::vector<uint64_t> cnt(NW + 1, 0);
            for (int64_t i = 0; i < NP; i++) cnt[(pcs[i].gpos >> 5) + 1]++;
            for (int64_t w = 0; w < NW; w++) cnt[w + 1] += cnt[w];
            for (int64_t i = 0; i < NP; i++) order[cnt[pcs[i].gpos >> 5]++] = (uint32_t)i;
        }
    }
    // piece CSR by start word: ps[w] = the first sorted piece starting in word ≥ w
    b->ps.resize(NW + 1);
    par_ranges(ntw, NP, [&](int, int64_t k0, int64_t k1) {
        for (int64_t k = k0; k < k1; k++) {
            const int64_t wk = (int64_t)(pcs[order[k]].gpos >> 5), wp = k ? (int64_t)(pcs[order[k - 1]].gpos >> 5) : -1;
            for (int64_t w = wp + 1; w <= wk; w++) b->ps[w] = (uint32_t)k;
        }
    });
    for (int64_t w = NP ? (int64_t)(pcs[order[NP - 1]].gpos >> 5) + 1 : 0; w <= NW; w++) b->ps[w] = (uint32_t)NP;
}

// ---- output offsets (ops, bases) in sorted order
void BatchPlan::offsets() {
    ooff.resize(NP + 1);
    qoff.resize(NP + 1);
    ooff[0] = qoff[0] = 0;
    {   // (range sums, then each range's prefix from its base)
        std::vector<uint64_t> so(ntw + 1, 0), sq(ntw + 1, 0);
        par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
            uint64_t a = 0, q = 0;
            for (int64_t k = k0; k < k1; k++) {
                const Piece &pc = pcs[order[k]];
                a += pc.nslots;
                q += pc.qlen;
                ooff[k + 1] = a;
                qoff[k + 1] = q;
            }
            so[t + 1] = a;
            sq[t + 1] = q;
        });
        for (int t = 0; t < ntw; t++) { so[t + 1] += so[t]; sq[t + 1] += sq[t]; }
        par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; k++) { ooff[k + 1] += so[t]; qoff[k + 1] += sq[t]; }
        });
    }
    NOPS = ooff[NP];
    NQ = qoff[NP];
}

// ---- the batch's arrays, sized (filled by emit: no zero-fill) and their uncovered tails
int BatchPlan::alloc() {
    // the kernels address run records and base planes with 32-bit buffer offsets (< 3.5 GB)
    if (16 * NOPS >= 0xE0000000ull) return s2c_set_error(S2C_ERR_LIMIT, "more than 2^28 op words (split the input)");
    if (NQ / 4 >= 0xE0000000ull) return s2c_set_error(S2C_ERR_LIMIT, "more than 14 G query bases (split the input)");
    I.n_ops = (int64_t)NOPS;
    I.n_qwords = (int64_t)((NQ + 31) / 32) + 2;
    b->pc.resize(4 * (size_t)(NP + 1));
    b->kmin.resize(NP);
    b->kmax.resize(NP);
    b->lmot.resize(NP);
    b->px.resize(std::max<int64_t>(NP, 1));
    b->ops.resize(std::max<uint64_t>(NOPS, 1));
    b->bq.resize(2 * (size_t)I.n_qwords);
    b->bx.resize((size_t)I.n_qwords);
    {   // the words the pieces do not cover: from the half-word after the last piece's bases on
        const uint64_t h0 = NQ / 16, nh = 2 * (uint64_t)I.n_qwords;
        uint16_t *dq = (uint16_t *)b->bq.data(), *dx = (uint16_t *)b->bx.data();
        for (uint64_t d = h0; d < nh; d++) {
            dq[(d >> 1) * 4 + (d & 1)] = 0;
            dq[(d >> 1) * 4 + 2 + (d & 1)] = 0;
            dx[d] = 0;
        }
        b->ops[0] = 0;
        for (int j = 0; j < 4; j++) b->pc[4 * (size_t)NP + j] = 0;
    }
    return S2C_OK;
}

// ---- emit: sorted pieces [k0, k1) — op words, piece records, px, base planes
void BatchPlan::emit_pieces(int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; k++) {
        const Piece &q = pcs[order[k]];
        const Chunk &c = *CH[q.chunk];
        const ReadRec &r = c.reads[q.read];
        uint32_t *o = &b->ops[ooff[k]];
        uint32_t fl = (r.has_x ? S2C_PF_X : 0u) | ((r.has_x & 2) ? S2C_PF_DASH : 0u);
        if (q.range) { fl |= S2C_PF_RANGE; *o++ = (uint32_t)q.ka; *o++ = (uint32_t)q.kb; }
        b->kmin[k] = 0xFFFFFFFFu;
        b->kmax[k] = 0u;
        b->lmot[k] = 0;
        if (q.ins) {
            fl |= S2C_PF_INS;
            b->kmin[k] = q.kmin;
            b->kmax[k] = q.kmax;
            for (uint32_t e = r.ev0; e < r.ev0 + r.nev; e++)
                if (c.ev[e].key >= 0 && c.ev[e].len > S2C_SHORT_MOTIF) b->lmot[k] = 1;
            const int64_t off = b->ref_off[r.ref], key0 = off + r.pos0;
            *o++ = (uint32_t)(uint64_t)key0;
            *o++ = (uint32_t)((uint64_t)key0 >> 32);
            *o++ = (uint32_t)off;
        }
        if (q.lng) fl |= S2C_PF_LONG;
        memcpy(o, &c.toks[r.tok], 4 * (size_t)r.ntok);
        b->px[k] = xfew_offsets(c, r, fl);
        uint32_t slen = r.slen;
        if (!q.range && !q.ins && !q.lng && r.ntok == 1 && op_bases(c.toks[r.tok] & 15u) && !(fl & S2C_PF_DASH)) {
            fl |= S2C_PF_SIMPLE;   // seqout = SEQ[0:take]: the field holds take (s2c.h)
            slen = std::min<uint32_t>(c.toks[r.tok] >> 4, r.slen);
        }
        uint32_t *pr = &b->pc[4 * (size_t)k];
        pr[0] = (uint32_t)q.gpos;
        pr[1] = (uint32_t)(qoff[k] / 16);
        pr[2] = (uint32_t)ooff[k];
        pr[3] = slen | (fl << 24);
        copy_planes(b->bq.data(), b->bx.data(), qoff[k] / 16, c.bq.data(), c.bx.data(), r.q / 16, r.slen);
    }
}

// ---- the sentinel piece, the run-slot CSR and the walked pieces' count
void BatchPlan::run_slots() {
    uint32_t *pr = &b->pc[4 * (size_t)NP];   // sentinel
    pr[1] = (uint32_t)(NQ / 16);
    pr[2] = (uint32_t)NOPS;
    // run-slot CSR by start word: the op slots before the first piece of word w
    b->rs.resize(NW + 1);
    par_ranges(plan_threads(NW + 1, 1 << 16), NW + 1, [&](int, int64_t w0, int64_t w1) {
        for (int64_t w = w0; w < w1; w++) b->rs[w] = (uint32_t)ooff[b->ps[w]];
    });
    I.n_walked = count_walked(b->pc.data(), NP);
}

// ---- tiles: width from depth; a shallow tile keeps its window's runs in LDS ----
void BatchPlan::tile_widths() {
    if (const char *e = plan_env("S2C_TILE_POS"))
        tile_force = align_up(std::min<int64_t>(std::max<int64_t>(atoll(e), 64), TP_MAX), S2C_POS_ALIGN);
    if (p->tile_width > 0) tile_force = p->tile_width;   // streamed batches: the same tiles every time
    std::vector<int64_t> ref_slots(R, 0), ref_np(R, 0), ref_qw(R, 0);
    {
        std::vector<std::vector<int64_t>> ts(ntw, std::vector<int64_t>(3 * R, 0)), tl(ntw);
        par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
            int64_t *a = ts[t].data();
            for (int64_t k = k0; k < k1; k++) {   // (a piece's reference from its start position)
                const Piece &q = pcs[order[k]];
                const uint32_t ref = q.ref;
                a[3 * ref] += q.nslots;
                a[3 * ref + 1]++;
                a[3 * ref + 2] += q.qlen;
                if (q.lng) tl[t].push_back(k);
            }
        });
        for (int t = 0; t < ntw; t++) {
            for (int64_t r = 0; r < R; r++) {
                ref_slots[r] += ts[t][3 * r];
                ref_np[r] += ts[t][3 * r + 1];
                ref_qw[r] += ts[t][3 * r + 2];
            }
            longs.insert(longs.end(), tl[t].begin(), tl[t].end());
        }
    }
    for (int64_t r = 0; r < R; r++) {
        const int64_t L = p->ref_len[r], off = b->ref_off[r];
        if (L == 0) continue;
        const double depth = (double)ref_span[r] / (double)L, spp = (double)ref_slots[r] / (double)L;
        // deep: ≈ E_TARGET aligned bases per tile, a power of two of words (every counting lane
        // of k_tile's waves busy) and at least S2C_DEEP_TILE positions (default 512: measured
        // against 256 / 320 on C3 and 256 on C4, profiles/r03/)
        int64_t tp = TP_MAX;
        if (depth > 0) {
            const double want = std::max(64.0, std::ceil(E_TARGET / depth));
            tp = (int64_t)1 << (int64_t)std::llround(std::log2(want));
            tp = std::max<int64_t>(tp, deep_tile_min());
        }
        const double win = 32.0 * (double)(K + 1) * spp;    // run slots per word's window
        if (win <= 200.0 && spp > 0) {
            // shallow: the widest tile whose window (12 B per op slot and 12 B per base plane word
            // in LDS, plane words below S2C_DENSE_QW; with a margin for the depth's spread) fits
            // the dense kernel
            const double qpp = ((double)ref_qw[r] / 32.0 + 0.25 * (double)ref_np[r]) / (double)L;
            const double bpp = (16.0 * (double)ref_slots[r] / (double)L) + 8.0 * qpp;   // S2C_DENSE_BYTES per position
            tp = TP_MAX;
            while (tp > TP_MIN && (((double)tp + 32.0 * (double)(K + 1)) * bpp + 1024.0 > DENSE_PLAN_BYTES ||
                                   ((double)tp + 32.0 * (double)(K + 1)) * qpp > 0.8 * S2C_DENSE_QW))
                tp /= 2;
        }
        tp = std::min(std::max(tp, TP_MIN), TP_MAX);
        if (tile_force > 0) tp = tile_force;
        const int64_t nt = ceil_div(L, tp);
        const int64_t step = align_up(ceil_div(L, nt), S2C_POS_ALIGN);
        for (int64_t a = off; a < off + L; a += step) {
            tiles.push_back({a, std::min(a + step, off + L), r});
            tile_max = std::max(tile_max, tiles.back().b - a);
        }
    }
}

// A ranged snapshot (s2c_parser_snapshot_from) plans tiles [P0, P1) only: from the first
// tile its streamed batch runs through the tile of the held reads' last position (the
// pieces' ends, the last read's POS: the stream driver's bound); the other tiles keep
// their bounds and insertion capacities but get no window, layers or work items
void BatchPlan::plan_range() {
    if (p->plan_from < 0) return;   // (a whole batch: every tile, after any split; a fixed tile width: no split)
    const int64_t NT0 = (int64_t)tiles.size();
    std::vector<int64_t> tmax(ntw, -1);
    par_ranges(ntw, NP, [&](int t, int64_t k0, int64_t k1) {
        int64_t m = -1;
        for (int64_t k = k0; k < k1; k++)
            if (pcs[k].kb > pcs[k].ka) m = std::max<int64_t>(m, (int64_t)pcs[k].gpos + (pcs[k].kb - pcs[k].ka) - 1);
        tmax[t] = m;
    });
    int64_t gmax = *std::max_element(tmax.begin(), tmax.end());
    for (auto it = p->chunks.rbegin(); it != p->chunks.rend(); ++it)
        if (!(*it)->reads.empty()) {
            const ReadRec &r = (*it)->reads.back();
            const int64_t L = p->ref_len[r.ref];
            if (L > 0) gmax = std::max<int64_t>(gmax, b->ref_off[r.ref] + std::min<int64_t>(std::max<int64_t>(r.pos0, 0), L - 1));
            break;
        }
    P0 = std::min<int64_t>(p->plan_from, NT0);
    int64_t tl = P0;   // first tile past gmax
    if (gmax >= 0) {
        int64_t lo = 0, hi = NT0;   // first tile with a > gmax
        while (lo < hi) {
            const int64_t m = (lo + hi) / 2;
            if (tiles[m].a > gmax) hi = m; else lo = m + 1;
        }
        tl = lo;
    }
    P1 = std::min<int64_t>(std::max<int64_t>(tl, P0), NT0);
}

// Launch LDS of k_tile_dense = the largest dense window, so one outlier window sets every
// tile's occupancy: when all but ≤ 0.2 % of the windows fit the share of a CU's 160 KB
// that lets 8 two-wave tiles reside (4 waves per SIMD, the kernel's register budget), the
// launch is sized to that share and the few tiles over it are split in two (each half's
// window fits; C5: 55 of 62,934 tiles), unless the tile width is fixed (streamed batches)
void BatchPlan::split_dense_outliers() {
    // (the kernel's static LDS; its dynamic LDS is never below S2C_DENSE_MIN_LDS, so for
    // 2048-position tiles (cap8 14,208 B) 8 tiles per CU cannot reside whatever the windows:
    // no tile is split for it)
    const int64_t cap8 = 163840 / 8 - (96 * dense_nwp_of(tile_max) + 128);
    const int64_t n0 = (int64_t)tiles.size();
    std::vector<int64_t> db(n0, -1);
    const int64_t q0 = std::min(P0, n0), q1 = std::min(P1, n0);   // (the planned tiles only: balanced ranges)
    par_ranges(plan_threads(q1 - q0, 64), q1 - q0, [&](int, int64_t i0, int64_t i1) {
        uint32_t tw[S2C_TILE_WORDS];
        for (int64_t t = q0 + i0; t < q0 + i1; t++) {
            tile_window(b, K, (uint64_t)tiles[t].a, (uint64_t)tiles[t].b, tw);
            if (dense_fits(tw)) db[t] = dense_bytes(tw);
        }
    });
    int64_t nfit = 0, over = 0;
    for (const int64_t x : db)
        if (x >= 0) { nfit++; over += x > cap8; }
    if (over > 0 && over * 500 <= nfit && cap8 >= S2C_DENSE_MIN_LDS) {
        dense_cap = cap8;
        if (tile_force == 0) {
            std::vector<Tile> split;
            split.reserve(n0 + over);
            for (int64_t t = 0; t < n0; t++) {
                const Tile &T = tiles[t];
                const int64_t mid = T.a + align_up((T.b - T.a) / 2, S2C_POS_ALIGN);
                if (db[t] > cap8 && mid < T.b) {
                    split.push_back({T.a, mid, T.ref});
                    split.push_back({mid, T.b, T.ref});
                } else {
                    split.push_back(T);
                }
            }
            tiles.swap(split);
        }
    }
}

// ---- the final tile list: its counts, and the tile of every word
void BatchPlan::tile_words() {
    NT = (int64_t)tiles.size();
    I.n_tiles = NT;
    I.tile_max = tile_max;
    I.plan_t0 = P0;
    I.plan_t1 = std::min<int64_t>(P1, NT);
    b->wtile.resize(NW);
    par_ranges(plan_threads(NW, 1 << 16), NW, [&](int, int64_t w0, int64_t w1) {
        std::fill(b->wtile.begin() + w0, b->wtile.begin() + w1, 0xFFFFFFFFu);
    });
    par_ranges(plan_threads(NT, 1 << 10), NT, [&](int, int64_t t0, int64_t t1) {   // (tiles hold disjoint words)
        for (int64_t t = t0; t < t1; t++)
            for (int64_t W = tiles[t].a >> 5; W < (tiles[t].b + 31) >> 5; W++) b->wtile[W] = (uint32_t)t;
    });
}

// fn(t, k) for every long piece k (sorted index) and every tile t it overlaps
template <class Fn>
void BatchPlan::for_long(Fn fn) const {
    for (const int64_t k : longs) {
        const Piece &q = pcs[order[k]];
        const uint32_t t0 = b->wtile[q.gpos >> 5], t1 = b->wtile[(q.gpos + (q.kb - q.ka) - 1) >> 5];
        for (uint32_t t = t0; t <= t1; t++) fn(t, k);
    }
}

// ---- long lists: run slots of long pieces per tile they overlap ----
void BatchPlan::long_lists() {
    lcnt.assign(NT + 1, 0);
    for_long([&](uint32_t t, int64_t k) { lcnt[t + 1] += pcs[order[k]].nslots; });
    for (int64_t t = 0; t < NT; t++) lcnt[t + 1] += lcnt[t];
    b->lp.resize(std::max<uint32_t>(lcnt[NT], 1));
    {
        std::vector<uint32_t> at(lcnt.begin(), lcnt.end() - 1);
        for_long([&](uint32_t t, int64_t k) {
            for (uint64_t s = ooff[k]; s < ooff[k + 1]; s++) b->lp[at[t]++] = (uint32_t)s;
        });
    }
    I.n_long = lcnt[NT];
    lwords.assign(NW + 1, 0);
    for (const int64_t k : longs) {   // (a difference array over the words, then its prefix sums)
        const Piece &q = pcs[order[k]];
        lwords[q.gpos >> 5]++;
        lwords[((q.gpos + (q.kb - q.ka) - 1) >> 5) + 1]--;
    }
    for (int64_t W = 0; W < NW; W++) lwords[W + 1] += lwords[W];
}

// ---- insertion plan: per tile its events' hash-table capacity, long-motif slots and an
//      upper bound of its columns (Σ motif lengths ≥ Σ over keys of the longest, :278-281)
void BatchPlan::insertion_plan() {
    nshort.assign(NT, 0);
    nlong.assign(NT, 0);
    nev.assign(NT, 0);
    ccap.assign(NT, 0);
    for (auto &cp : CH)
        for (const Event &e : cp->ev) {
            if (e.key < 0) continue;   // never emitted (:355 walks 0..LN-1)
            const uint64_t gk = (uint64_t)(b->ref_off[e.ref] + e.key);
            const uint32_t t = b->wtile[gk >> 5];
            nev[t]++;
            (e.len <= S2C_SHORT_MOTIF ? nshort : nlong)[t]++;
            ccap[t] += e.len;
            I.n_ins++;
            I.n_ins_bases += e.len;
        }
}

// ---- work items: per tile its layers (k_tile's per-wave LDS chunks; lane groups of G = 64 / nwp
//      lanes per word) split into items ----
int BatchPlan::tile_plans() {
    lcols = S2C_LDS_COLS(nwp);
    b->tiles.assign((size_t)NT * S2C_TILE_WORDS, 0u);
    // the k_tile instantiation the layers are cut for (its chunk's plane bytes): a shard of this
    // batch keeps the non-queue one when this is planned for it (mark_runs)
    I.walk_queue = walk_queue_of(I);
    const int64_t wq = I.walk_queue;
    // per tile (host threads): its window, the most candidate runs of a word, layers, items
    t_nl.assign(NT, 0);
    t_nch.assign(NT, 0);
    t_maxc.assign(NT, 0);
    t_wruns.assign(NT, 0);
    std::atomic<bool> too_big{false}, over_u16{false};
    const int64_t q0 = std::min(P0, NT), q1 = std::min(P1, NT);   // the planned tiles, in balanced ranges
    par_ranges(plan_threads(q1 - q0, 64), q1 - q0, [&](int, int64_t i0, int64_t i1) {
        for (int64_t t = q0 + i0; t < q0 + i1; t++) {
            const Tile &T = tiles[t];
            const int64_t w0 = T.a >> 5, w1 = (T.b + 31) >> 5;
            const int64_t nlg = lcnt[t + 1] - lcnt[t];
            int64_t maxc = 0;
            for (int64_t W = w0; W < w1; W++)
                maxc = std::max<int64_t>(maxc, (int64_t)b->rs[W + 1] - (int64_t)b->rs[std::max<int64_t>(W - K, 0)] + nlg);
            t_maxc[t] = maxc;
            const int64_t nl = plan_layers(b, PB, K, (uint64_t)T.a, (uint64_t)T.b, G, wq);
            t_nl[t] = nl;
            if (nl <= 0) { too_big = true; continue; }
            t_nch[t] = plan_items(b, PB, K, (uint64_t)T.a, (uint64_t)T.b, nl, item_layers(), nlg, lwords.data());
            if (t_nch[t] <= 0) { over_u16 = true; continue; }
            t_wruns[t] = (int64_t)b->rs[w1] - (int64_t)b->rs[std::max<int64_t>(w0 - K, 0)];
            tile_window(b, K, T.a, T.b, &b->tiles[(size_t)t * S2C_TILE_WORDS]);
        }
    });
    if (over_u16) return s2c_set_error(S2C_ERR_LIMIT, "a tile's run records exceed its work items' u16 histograms");
    return too_big ? s2c_set_error(S2C_ERR_LIMIT, "a read whose SEQ or CIGAR exceeds k_tile's LDS chunk") : S2C_OK;
}

// The dense class of a planned tile: one item, no insertion event, at most 255 candidate runs
// per word, a window that fits the launch's LDS and the compact piece records (S2C_DPC_*)
bool BatchPlan::is_dense_tile(int64_t t) const {
    const uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
    return t_nch[t] == 1 && nev[t] == 0 && (int64_t)ccap[t] <= lcols && t_maxc[t] <= 255 && !no_dense &&
           dense_fits(tw) && dense_bytes(tw) <= dense_cap && K <= 64 && dbad[tw[14]] == dbad[tw[13]];
}

// Grid shaping for k_tile: work items run in rounds of `slots` workgroups (the device's CUs
// × k_tile's workgroups per CU); the last round of a launch whose items all take about as
// long keeps the rest of the device idle.  The multi-item (deep) tiles' items are made
// smaller (down to half of IL layers) until the launch fills its last round: C4's 2,487
// items of ≤ 64 layers (3.24 rounds of 768) become 3,0xx of ≤ 52.
void BatchPlan::shape_item_grid() {
    const int64_t q0 = std::min(P0, NT), q1 = std::min(P1, NT);   // the planned tiles, in balanced ranges
    int64_t n_single = 0, n_multi = 0;
    for (int64_t t = P0; t < std::min<int64_t>(P1, NT); t++) {
        if (t_nch[t] > 1) n_multi += t_nch[t];
        else if (!is_dense_tile(t)) n_single++;
    }
    int64_t slots = plan_cus() * (nwp <= 16 ? 3 : 2);   // the device's CUs × k_tile<16>'s 3 workgroups per CU by LDS
    if (const char *e = plan_env("S2C_ITEM_SLOTS")) slots = std::max<int64_t>(0, atoll(e));
    const int64_t IL = item_layers();
    if (n_multi > 0 && slots > 0) {
        const int64_t rounds = (n_single + n_multi + slots - 1) / slots;
        int64_t best = IL;
        for (int64_t il = IL - 1; il >= std::max<int64_t>(4, IL / 2); il--) {
            int64_t n = n_single;
            for (int64_t t = 0; t < NT; t++)
                if (t_nch[t] > 1) n += std::max<int64_t>(t_nch[t], (t_nl[t] + il - 1) / il);
            if (n > rounds * slots) break;
            best = il;
        }
        if (best < IL)
            par_ranges(plan_threads(q1 - q0, 64), q1 - q0, [&](int, int64_t i0, int64_t i1) {
                for (int64_t t = q0 + i0; t < q0 + i1; t++)
                    if (t_nch[t] > 1)
                        t_nch[t] = std::max<int64_t>(t_nch[t], plan_items(b, PB, K, (uint64_t)tiles[t].a, (uint64_t)tiles[t].b, t_nl[t], best,
                                                                          (int64_t)lcnt[t + 1] - lcnt[t], lwords.data()));
            });
    }
}

// ---- the tile records (words 0-12 and 19; 13-18 are tile_plans' windows), the work items of
//      the planned tiles by class, and the insertion tables' slot bases
int BatchPlan::tile_records() {
    uint64_t boff = 0, loff = 0, coff = 0;
    int64_t runs_max = 0;
    I.chunk = 0;   // (the most layers of any tile)
    for (int64_t t = 0; t < NT; t++) {
        const Tile &T = tiles[t];
        const int64_t nl = t_nl[t], nch = t_nch[t];
        I.chunk = std::max<int64_t>(I.chunk, nl);
        runs_max = std::max(runs_max, t_wruns[t]);
        uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
        uint32_t fl = nch > 1 ? S2C_TILE_DEEP : 0u;
        if (nev[t] > S2C_EPI_KEYS || (int64_t)ccap[t] > lcols) fl |= S2C_TILE_GENERAL;
        if (!planned(t)) fl = 0;   // (a ranged snapshot's unplanned tile: no items)
        else if (is_dense_tile(t)) fl = S2C_TILE_DENSE;   // (one item, no event: neither deep nor general)
        const uint32_t bcap = nshort[t] ? pow2_at_least(2 * (uint64_t)nshort[t]) : 0u;
        tw[0] = (uint32_t)T.a; tw[1] = (uint32_t)T.b; tw[2] = (uint32_t)T.ref; tw[3] = fl;
        tw[4] = (uint32_t)boff; tw[5] = bcap; tw[6] = (uint32_t)loff; tw[7] = nlong[t];
        tw[8] = (uint32_t)coff; tw[9] = (uint32_t)ccap[t]; tw[10] = lcnt[t]; tw[11] = lcnt[t + 1];
        tw[12] = nev[t];
        tw[19] = (uint32_t)nl;
        tw[21] = planned(t) ? (uint32_t)nch : 0u;
        boff += bcap;
        loff += nlong[t];
        coff += ccap[t];
        if (!planned(t)) {
        } else if (fl == S2C_TILE_DENSE) {
            I.dense_lds = std::max<int64_t>(I.dense_lds, dense_bytes(tw));
            const uint32_t it[S2C_ITEM_WORDS] = {(uint32_t)t, 0u, 0u, (uint32_t)nl};
            b->dense.insert(b->dense.end(), it, it + S2C_ITEM_WORDS);
        } else {
            for (int64_t c = 0; c < nch; c++) {
                const uint32_t it[S2C_ITEM_WORDS] = {(uint32_t)t, (uint32_t)c, (uint32_t)(c * nl / nch),
                                                     (uint32_t)((c + 1) * nl / nch)};
                b->items.insert(b->items.end(), it, it + S2C_ITEM_WORDS);
            }
        }
        if (fl & (S2C_TILE_DEEP | S2C_TILE_GENERAL)) b->deep.push_back((uint32_t)t);
    }
    if (boff >= (1ull << 32) || loff >= (1ull << 32) || coff >= (1ull << 31))
        return s2c_set_error(S2C_ERR_LIMIT, "insertion tables exceed 2^32 slots (split the input)");
    I.n_items = (int64_t)(b->items.size() / S2C_ITEM_WORDS);
    I.n_dense = (int64_t)(b->dense.size() / S2C_ITEM_WORDS);
    I.n_deep = (int64_t)b->deep.size();
    I.n_bkt = (int64_t)boff;
    I.n_lng = (int64_t)loff;
    I.n_cols = (int64_t)coff;
    I.runs_max = runs_max;
    return S2C_OK;
}

// ---- the long lists once the tiles' kinds are known: a dense tile lists its long pieces
//      (k_tile_dense walks them itself), the others their run slots (k_reads' records)
void BatchPlan::long_lists_by_kind() {
    if (I.n_long == 0) return;
    std::vector<uint32_t> cnt2(NT + 1, 0);
    auto is_dense = [&](uint32_t t) { return (b->tiles[(size_t)t * S2C_TILE_WORDS + 3] & S2C_TILE_DENSE) != 0; };
    for_long([&](uint32_t t, int64_t k) { cnt2[t + 1] += is_dense(t) ? 1u : pcs[order[k]].nslots; });
    for (int64_t t = 0; t < NT; t++) cnt2[t + 1] += cnt2[t];
    std::vector<uint32_t> lp2(std::max<uint32_t>(cnt2[NT], 1), 0u), at(cnt2.begin(), cnt2.end() - 1);
    for_long([&](uint32_t t, int64_t k) {
        if (is_dense(t)) lp2[at[t]++] = (uint32_t)k;
        else
            for (uint64_t sl = ooff[k]; sl < ooff[k + 1]; sl++) lp2[at[t]++] = (uint32_t)sl;
    });
    for (int64_t t = 0; t < NT; t++) {
        b->tiles[(size_t)t * S2C_TILE_WORDS + 10] = cnt2[t];
        b->tiles[(size_t)t * S2C_TILE_WORDS + 11] = cnt2[t + 1];
    }
    b->lp.swap(lp2);
    I.n_long = cnt2[NT];
}
}  // namespace

// The batch of the reads p holds: the phases in order, S2C_HOST_TIMING=1 timing each.
int build_batch(s2c_parser *p, s2c_batch **out) {
    PhaseClock clk;
    if (const int rc = check_insertions(p)) return rc;
    clk.mark("checks");
    BatchPlan P(p);
    if (const int rc = P.layout()) return rc;
    if (const int rc = P.pieces()) return rc;
    clk.mark("pieces");
    P.window();
    clk.mark("window");
    P.bucket();
    clk.mark("bucket");
    P.offsets();
    clk.mark("offsets");
    if (const int rc = P.alloc()) return rc;
    clk.mark("alloc");
    // (in parallel over ranges of sorted pieces: each thread first-touches its range)
    par_ranges(plan_threads(P.NP, 65536), P.NP, [&](int, int64_t k0, int64_t k1) { P.emit_pieces(k0, k1); });
    clk.mark("emit threads");
    P.run_slots();
    clk.mark("emit");
    P.tile_widths();
    P.plan_range();
    P.split_dense_outliers();
    P.tile_words();
    clk.mark("tiles");
    P.long_lists();
    clk.mark("long lists");
    P.insertion_plan();
    clk.mark("ins plan");
    P.nwp = nwp_of(P.tile_max);
    P.G = 64 / P.nwp;   // (counting lanes per word of one wave: each wave runs its own layers)
    piece_blocks(P.b, P.PB);
    clk.mark("piece blocks");
    if (const int rc = P.tile_plans()) return rc;
    clk.mark("tile plans");
    P.dbad = dpc_bad_prefix(P.b);   // (windows k_tile_dense's compact piece records can hold)
    P.shape_item_grid();
    if (const int rc = P.tile_records()) return rc;
    clk.mark("items");
    P.long_lists_by_kind();
    mark_runs(P.b);
    clk.mark("mark_runs");
    build_dwin(P.b);
    clk.mark("dwin");
    *out = P.guard.release();
    return S2C_OK;
}
