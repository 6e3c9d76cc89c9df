// s2c_shard.cpp — sub-batches of a planned batch for the multi-GPU runs, the layered windows'
// entry points and the s2c_batch_* accessors.
#include "s2c_host_internal.h"

// ------------------------------------------------------------------ shards (multi-GPU)
// The sub-batch of tiles [t0, t1): the pieces whose runs can cover those tiles (short ones
// starting up to kwin + 1 words before, the long ones listed for them) or whose insertion
// events are keyed inside them, with their op words and base planes; run slots, long
// lists, hash-table / column slot bases and tile indices re-based.  Positions keep their
// global coordinates; words outside the shard map to no tile (k_reads drops events keyed
// there).  Counts of a position depend only on the runs covering it, so every shard's
// tiles get exactly the unsharded counts — no exchange of counts is needed.
static int s2c_batch_shard_impl(const s2c_batch *b, int64_t t0, int64_t t1, s2c_batch **out) {
    if (!b || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    const s2c_batch_info &I = b->info;
    if (t0 < 0 || t1 > I.n_tiles || t0 > t1) return s2c_set_error(S2C_ERR_ARG, "bad tile range");
    std::unique_ptr<s2c_batch> s(new s2c_batch());
    s2c_batch_info &J = s->info;
    J = I;
    s->names = b->names;
    s->ref_len = b->ref_len;
    s->ref_off = b->ref_off;
    s->ref_reads = b->ref_reads;
    const int64_t NP = I.n_pieces, NW = I.n_words, K = I.kwin;
    const uint32_t *T0 = &b->tiles[(size_t)t0 * S2C_TILE_WORDS];
    const uint64_t A = t1 > t0 ? T0[0] : 0, B = t1 > t0 ? b->tiles[(size_t)(t1 - 1) * S2C_TILE_WORDS + 1] : 0;
    const int64_t W0 = (int64_t)(A >> 5), W1 = (int64_t)((B + 31) >> 5);
    // ---- pieces: the window range, long pieces listed by the tiles, event pieces keyed inside
    std::vector<uint8_t> take(NP, 0);
    if (t1 > t0) {
        const int64_t pa = piece_at_word(b, std::max<int64_t>(W0 - K - 1, 0)), pb = piece_at_word(b, W1);
        for (int64_t k = pa; k < pb; k++) take[k] = 1;
        for (int64_t t = t0; t < t1; t++) {
            const uint32_t *tw = &b->tiles[(size_t)t * S2C_TILE_WORDS];
            const bool dl = (tw[3] & S2C_TILE_DENSE) != 0;   // (a dense tile lists pieces, others run slots)
            for (uint32_t e = tw[10]; e < tw[11]; e++) take[dl ? (int64_t)b->lp[e] : piece_of_slot(b, b->lp[e])] = 1;
        }
        for (int64_t k = 0; k < NP; k++)
            if (b->kmin[k] != 0xFFFFFFFFu && b->kmax[k] >= A && b->kmin[k] < B) take[k] = 1;
    }
    std::vector<int64_t> sel;
    for (int64_t k = 0; k < NP; k++)
        if (take[k]) sel.push_back(k);
    const int64_t NS = (int64_t)sel.size();
    std::vector<uint64_t> ooff(NS + 1, 0), qoff(NS + 1, 0);
    for (int64_t i = 0; i < NS; i++) {
        const int64_t k = sel[i];
        ooff[i + 1] = ooff[i] + (b->pc[4 * (k + 1) + 2] - b->pc[4 * k + 2]);
        qoff[i + 1] = qoff[i] + ((b->pc[4 * k + 3] & 0xFFFFFFu) + 15) / 16 * 16;
    }
    J.n_pieces = NS;
    J.n_ops = (int64_t)ooff[NS];
    J.n_qwords = (int64_t)((qoff[NS] + 31) / 32) + 2;
    s->pc.assign(4 * (size_t)(NS + 1), 0u);
    s->ops.assign(std::max<uint64_t>(ooff[NS], 1), 0u);
    s->bq.assign(2 * (size_t)J.n_qwords, 0u);
    s->bx.assign((size_t)J.n_qwords, 0u);
    s->kmin.assign(NS, 0xFFFFFFFFu);
    s->kmax.assign(NS, 0u);
    s->lmot.assign(NS, 0);
    s->px.assign(std::max<int64_t>(NS, 1), 0xFFFFFFFFu);
    std::unordered_map<uint32_t, uint32_t> slot_new, piece_new;   // old op slot / long piece → new
    for (int64_t i = 0; i < NS; i++) {
        const int64_t k = sel[i];
        const uint32_t o0 = b->pc[4 * k + 2], o1 = b->pc[4 * (k + 1) + 2];
        memcpy(&s->ops[ooff[i]], &b->ops[o0], 4 * (size_t)(o1 - o0));
        uint32_t *pr = &s->pc[4 * (size_t)i];
        pr[0] = b->pc[4 * k];
        pr[1] = (uint32_t)(qoff[i] / 16);
        pr[2] = (uint32_t)ooff[i];
        pr[3] = b->pc[4 * k + 3];
        if (pr[3] >> 24 & S2C_PF_LONG) {
            for (uint32_t o = o0; o < o1; o++) slot_new[o] = (uint32_t)(ooff[i] + (o - o0));
            piece_new[(uint32_t)k] = (uint32_t)i;
        }
        s->kmin[i] = b->kmin[k];
        s->kmax[i] = b->kmax[k];
        s->lmot[i] = b->lmot[k];
        s->px[i] = b->px[k];
        copy_planes(s->bq.data(), s->bx.data(), qoff[i] / 16, b->bq.data(), b->bx.data(), b->pc[4 * k + 1],
                    b->pc[4 * k + 3] & 0xFFFFFFu);
    }
    s->pc[4 * (size_t)NS + 1] = (uint32_t)(qoff[NS] / 16);
    s->pc[4 * (size_t)NS + 2] = (uint32_t)ooff[NS];
    s->rs.assign(NW + 1, 0u);
    s->ps.assign(NW + 1, 0u);
    for (int64_t i = 0; i < NS; i++) {
        s->rs[(s->pc[4 * i] >> 5) + 1] += (uint32_t)(ooff[i + 1] - ooff[i]);
        s->ps[(s->pc[4 * i] >> 5) + 1]++;
    }
    for (int64_t w = 0; w < NW; w++) {
        s->rs[w + 1] += s->rs[w];
        s->ps[w + 1] += s->ps[w];
    }
    // ---- tiles [t0, t1): slot bases re-based, long lists remapped, plan lists re-indexed
    const int64_t NT = t1 - t0;
    J.n_tiles = NT;
    s->tiles.assign(b->tiles.begin() + t0 * S2C_TILE_WORDS, b->tiles.begin() + t1 * S2C_TILE_WORDS);
    const uint32_t boff0 = NT ? T0[4] : 0, loff0 = NT ? T0[6] : 0, coff0 = NT ? T0[8] : 0;
    int64_t nbkt = 0, nlng = 0, ncol = 0;
    for (int64_t t = 0; t < NT; t++) {
        uint32_t *tw = &s->tiles[(size_t)t * S2C_TILE_WORDS];
        tw[4] -= boff0;
        tw[6] -= loff0;
        tw[8] -= coff0;
        nbkt = std::max<int64_t>(nbkt, (int64_t)tw[4] + tw[5]);
        nlng = std::max<int64_t>(nlng, (int64_t)tw[6] + tw[7]);
        ncol = std::max<int64_t>(ncol, (int64_t)tw[8] + tw[9]);
        const uint32_t l0 = (uint32_t)s->lp.size();
        const bool dl = (tw[3] & S2C_TILE_DENSE) != 0;
        for (uint32_t e = tw[10]; e < tw[11]; e++) s->lp.push_back(dl ? piece_new.at(b->lp[e]) : slot_new.at(b->lp[e]));
        tw[10] = l0;
        tw[11] = (uint32_t)s->lp.size();
    }
    J.n_long = (int64_t)s->lp.size();
    if (s->lp.empty()) s->lp.push_back(0);
    J.n_bkt = nbkt;
    J.n_lng = nlng;
    J.n_cols = ncol;
    s->wtile.assign(NW, 0xFFFFFFFFu);
    for (int64_t w = W0; w < W1; w++)
        if (b->wtile[w] != 0xFFFFFFFFu) s->wtile[w] = b->wtile[w] - (uint32_t)t0;
    auto sub_items = [&](const std::vector<uint32_t> &src, std::vector<uint32_t> &dst) {
        for (size_t i = 0; i < src.size(); i += S2C_ITEM_WORDS)
            if (src[i] >= (uint64_t)t0 && src[i] < (uint64_t)t1) {
                dst.insert(dst.end(), &src[i], &src[i] + S2C_ITEM_WORDS);
                dst[dst.size() - S2C_ITEM_WORDS] -= (uint32_t)t0;
            }
    };
    sub_items(b->items, s->items);
    sub_items(b->dense, s->dense);
    for (uint32_t t : b->deep)
        if (t >= (uint64_t)t0 && t < (uint64_t)t1) s->deep.push_back(t - (uint32_t)t0);
    J.n_items = (int64_t)(s->items.size() / S2C_ITEM_WORDS);
    J.n_dense = (int64_t)(s->dense.size() / S2C_ITEM_WORDS);
    J.n_deep = (int64_t)s->deep.size();
    int64_t runs_max = 0, aligned = 0;
    for (int64_t t = 0; t < NT; t++) {
        const uint32_t *tw = &s->tiles[(size_t)t * S2C_TILE_WORDS];
        const int64_t w0 = tw[0] >> 5, w1 = (tw[1] + 31) >> 5;
        runs_max = std::max<int64_t>(runs_max, (int64_t)s->rs[w1] - (int64_t)s->rs[std::max<int64_t>(w0 - K, 0)]);
        aligned += tw[1] - tw[0];
    }
    J.runs_max = runs_max;
    J.dense_lds = 0;
    for (int64_t t = 0; t < NT; t++) {
        uint32_t *tw = &s->tiles[(size_t)t * S2C_TILE_WORDS];
        tile_window(s.get(), K, tw[0], tw[1], tw);
        if (!(tw[3] & S2C_TILE_DENSE)) continue;
        if (!dense_fits(tw)) return s2c_set_error(S2C_ERR_LIMIT, "shard window beyond the dense kernel's LDS");
        J.dense_lds = std::max<int64_t>(J.dense_lds, dense_bytes(tw));
    }
    // (the shard's own layered windows are built on first use: s2c_batch_layers; until then
    // no tile word 20 names a layer of the parent's and launches with work items refuse it)
    J.n_layers = J.n_lpieces = J.n_lops = J.n_lqwords = 0;
    J.layers_dense = J.layers_built = 0;
    for (int64_t t = 0; t < NT; t++) s->tiles[(size_t)t * S2C_TILE_WORDS + 20] = S2C_LY_NONE;
    J.n_walked = count_walked(s->pc.data(), NS);   // the shard's own (its k_tile variant: mark_runs)
    mark_runs(s.get());
    build_dwin(s.get());
    // the shard's share of the workload's aligned bases (by its positions; for reporting)
    // the per-word entries the shard's launches read (s2c_batch_info word_lo / word_hi): its
    // tiles' words, the window lookback of k_tile_dense's run-slot ranges (rs[W - kwin]) and
    // the piece range above; k_reads drops events keyed outside
    J.plan_t0 = 0;   // (every tile of a shard has its plan: tile_window above, items copied)
    J.plan_t1 = NT;
    J.word_lo = t1 > t0 ? std::max<int64_t>(W0 - K - 1, 0) : 0;
    J.word_hi = t1 > t0 ? std::min<int64_t>(W1, NW) : 0;
    J.aligned_bases = I.total_len ? (int64_t)((double)I.aligned_bases * (double)aligned / (double)I.total_len) : 0;
    *out = s.release();
    return S2C_OK;
}
extern "C" int s2c_batch_shard(const s2c_batch *b, int64_t t0, int64_t t1, s2c_batch **out) {
    return s2c_guarded([&] { return s2c_batch_shard_impl(b, t0, t1, out); });
}

static int s2c_batch_layers_impl(s2c_batch *b, bool with_dense) {
    if (!b) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (b->layers && (b->info.layers_dense || !with_dense)) return S2C_OK;
    build_layers(b, 64 / nwp_of(b->info.tile_max), with_dense);
    b->layers = true;
    b->info.layers_built = 1;
    return S2C_OK;
}
extern "C" int s2c_batch_layers(s2c_batch *b) {
    return s2c_guarded([&] { return s2c_batch_layers_impl(b, true); });
}
extern "C" int s2c_batch_layers_mode(s2c_batch *b, int with_dense) {
    return s2c_guarded([&] { return s2c_batch_layers_impl(b, with_dense != 0); });
}

extern "C" int s2c_batch_info_get(const s2c_batch *b, s2c_batch_info *out) {
    if (!b || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    *out = b->info;
    return S2C_OK;
}

extern "C" int s2c_batch_arrays_get(const s2c_batch *b, s2c_batch_arrays *o) {
    if (!b || !o) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    o->ref_len = b->ref_len.data();
    o->ref_off = b->ref_off.data();
    o->ref_cov_reads = b->ref_reads.data();
    o->pc = b->pc.data();
    o->ops = b->ops.data();
    o->bq = b->bq.data();
    o->bx = b->bx.data();
    o->rs = b->rs.data();
    o->tiles = b->tiles.data();
    o->items = b->items.data();
    o->dense = b->dense.data();
    o->deep = b->deep.data();
    o->lp = b->lp.data();
    o->wtile = b->wtile.data();
    o->rlist = b->rlist.data();
    o->px = b->px.data();
    o->dwin = b->dwin.data();
    o->ps = b->ps.data();
    o->lly = b->lly.data();
    o->lpc = b->lpc.data();
    o->lops = b->lops.data();
    o->lbq = b->lbq.data();
    o->lbx = b->lbx.data();
    o->lpx = b->lpx.empty() ? nullptr : b->lpx.data();
    o->dpc = b->dpc.data();
    return S2C_OK;
}

extern "C" int s2c_batch_dense_ext_get(const s2c_batch *b, s2c_dense_ext *o) {
    if (!b || !o) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    o->drun = b->drun.data();
    o->dnev = b->dnev.data();
    o->dxs = b->dxs.data();
    o->drare = b->drare.data();
    o->dext = b->dext.data();
    o->n_drun = b->n_drun;
    o->n_dnev = b->n_dnev;
    o->n_dxs = b->n_dxs;
    o->n_drare = b->n_drare;
    o->n_dext = b->info.n_dense;
    return S2C_OK;
}

extern "C" int s2c_batch_dense_lean_get(const s2c_batch *b, s2c_dense_lean *o) {
    if (!b || !o) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    o->rop = b->rop.data();
    o->roff = b->roff.data();
    o->row = b->drow.data();
    o->n_rop = b->n_rop;
    o->n_roff = b->n_drare;
    o->n_row = b->info.n_dense;
    o->lds = b->lean_lds;
    o->count_max = b->lean_count;
    o->pairs = b->lean_pairs;
    return S2C_OK;
}

extern "C" const char *s2c_batch_ref_name(const s2c_batch *b, int64_t i) {
    if (!b || i < 0 || i >= (int64_t)b->names.size()) return nullptr;
    return b->names[i].c_str();
}

extern "C" void s2c_batch_free(s2c_batch *b) { delete b; }
