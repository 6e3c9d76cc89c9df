// s2c_parse.cpp — host side of libs2c.so: the SAM line parser and the parser-side C-ABI
// (the byte source is s2c_reader.cpp; the packed read batch and its tile plan s2c_plan.cpp).
//
// Reproduces the reference's record handling (zoujiayun/sam2consensus v2.1,
// sam2consensus.py) exactly, including its Python-2 quirks:
//   header pass            :149-172   (leading '@' lines, @SQ SN:/LN: parse)
//   record filter          :195       (line[0] != '@' and field[5] != "*"; FLAG ignored)
//   RNAME / POS            :200-201   (str.split()[0], int() - 1)
//   CIGAR tokens           :58-59     (regex matches; junk skipped)
//   the read pass's errors :195,:200,:201,:206,:212,:217,:221 in file order, and the
//                          reformat phase's :287 / :294 per reference
// and emits north_star subsystem (1), the packed batch: per read its CIGAR tokens and
// its SEQ as 2-bit base planes plus a non-ACGT plane, in QUERY order; pieces (a read,
// or its two parts around the POS<=0 wrap) bucketed by their start word; the tile plan.
// The CIGAR is NOT expanded here: seqout, the maxdel drop (:210) applied to the counts,
// and the insertion motif aggregation (:262-294) are computed on the device (k_reads).
// The host walks the tokens only to raise the reference's errors in file order (which
// needs the seqout length, the '-' count and the counted range) and to size the plan.
#include "s2c_host_internal.h"

// ------------------------------------------------------------------ tables
namespace {
// SEQ char → 3-bit plane code x·4 + p1·2 + p0: A 0, C 1, G 2, T 3, N 4, '-' 5, other 7
constexpr uint8_t Q_N = 4, Q_DASH = 5, Q_BAD = 7;
struct QLut {
    uint8_t v[256];
    QLut() {
        memset(v, Q_BAD, sizeof(v));
        v[(uint8_t)'A'] = 0; v[(uint8_t)'C'] = 1; v[(uint8_t)'G'] = 2; v[(uint8_t)'T'] = 3;
        v[(uint8_t)'N'] = Q_N; v[(uint8_t)'-'] = Q_DASH;
    }
};
const QLut QL;

inline bool py2_ws(char c) {  // Python 2 str.split()/int() whitespace (C locale isspace)
    return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\x0b' || c == '\x0c';
}

// Python 2 int(str): whitespace, sign, decimal digits, whitespace.  Saturates at ±2^62
// (positions that large are out of range anyway and raise IndexError downstream).
bool py2_int(const char *s, size_t n, int64_t *out) {
    size_t i = 0;
    while (i < n && py2_ws(s[i])) i++;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    size_t d0 = i;
    int64_t v = 0;
    const int64_t CAP = (int64_t)1 << 62;
    while (i < n && s[i] >= '0' && s[i] <= '9') {
        if (v < CAP) v = v * 10 + (s[i] - '0');
        if (v > CAP) v = CAP;
        i++;
    }
    if (i == d0) return false;
    while (i < n && py2_ws(s[i])) i++;
    if (i != n) return false;
    *out = neg ? -v : v;
    return true;
}

// first whitespace-delimited token (Python 2 str.split()[0])
bool py2_first_token(const char *s, size_t n, const char **tb, size_t *tl) {
    size_t i = 0;
    while (i < n && py2_ws(s[i])) i++;
    if (i == n) return false;
    size_t j = i;
    while (j < n && !py2_ws(s[j])) j++;
    *tb = s + i;
    *tl = j - i;
    return true;
}

// str.replace(pat, "") — Python's single left-to-right non-overlapping pass.
std::string py_remove(const char *s, size_t n, const char *pat) {
    size_t m = strlen(pat);
    std::string out;
    out.reserve(n);
    size_t i = 0;
    while (i < n) {
        if (i + m <= n && memcmp(s + i, pat, m) == 0) { i += m; continue; }
        out.push_back(s[i++]);
    }
    return out;
}
}  // namespace

// @SQ line (:160-169): refname = f[1].replace("SN:","").split()[0]; LN = int(f[2].replace("LN:",""))
static int parse_sq(s2c_parser *p, const char *s, size_t n) {
    const char *f[3];
    size_t fl[3];
    int nf = 0;
    const char *cur = s, *end = s + n;
    while (nf < 3) {
        const char *t = (const char *)memchr(cur, '\t', end - cur);
        f[nf] = cur;
        if (!t) { fl[nf++] = end - cur; break; }
        fl[nf++] = t - cur;
        cur = t + 1;
    }
    if (nf < 2) return perr(p, S2C_ERR_INDEX, "IndexError: @SQ line has no field 1 (:163)");
    std::string f1 = py_remove(f[1], fl[1], "SN:");
    const char *tb;
    size_t tl;
    if (!py2_first_token(f1.data(), f1.size(), &tb, &tl))
        return perr(p, S2C_ERR_INDEX, "IndexError: empty @SQ SN (:163)");
    std::string name(tb, tl);
    if (nf < 3) return perr(p, S2C_ERR_INDEX, "IndexError: @SQ line has no field 2 (:164)");
    std::string f2 = py_remove(f[2], fl[2], "LN:");
    int64_t ln;
    if (!py2_int(f2.data(), f2.size(), &ln))
        return perr(p, S2C_ERR_VALUE, "ValueError: invalid @SQ LN '" + f2 + "' (:164)");
    if (ln < 0) ln = 0;  // range(negative) → empty list (:167)
    auto it = p->ref_idx.find(name);
    if (it == p->ref_idx.end()) {
        p->ref_idx.emplace(name, (uint32_t)p->ref_names.size());
        p->ref_names.push_back(name);
        p->ref_len.push_back(ln);
    } else {
        p->ref_len[it->second] = ln;  // duplicate @SQ re-initialises (:167-169)
    }
    return S2C_OK;
}

// Context shared by the record parsers of one parse (read-only reference table).
struct RefView {
    const std::unordered_map<std::string, uint32_t> *idx;
    const std::vector<int64_t> *len;
    bool maxdel_active;
    int64_t maxdel;
};

// SEQ → bit planes, 32 chars per word group {p0, p1, x, bad} (bit j = char 32·w + j; the QL
// code's bits x·4 + p1·2 + p0, and bad = a char outside "-ACGNT"); bits past slen are zero.
static void seq_planes_scalar(const char *seq, size_t slen, uint32_t *o) {
    for (size_t w = 0; w * 32 < slen; w++) {
        const size_t m = std::min<size_t>(slen - 32 * w, 32);
        uint32_t p0 = 0, p1 = 0, x = 0, bad = 0;
        for (size_t j = 0; j < m; j++) {
            const uint32_t v = QL.v[(uint8_t)seq[32 * w + j]];
            p0 |= (v & 1u) << j;
            p1 |= ((v >> 1) & 1u) << j;
            x |= ((v >> 2) & 1u) << j;
            bad |= (v == Q_BAD ? 1u : 0u) << j;
        }
        o[4 * w] = p0; o[4 * w + 1] = p1; o[4 * w + 2] = x; o[4 * w + 3] = bad;
    }
}
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) static void seq_planes_avx2(const char *seq, size_t slen, uint32_t *o) {
    const __m256i A = _mm256_set1_epi8('A'), Cc = _mm256_set1_epi8('C'), Gg = _mm256_set1_epi8('G');
    const __m256i Tt = _mm256_set1_epi8('T'), Nn = _mm256_set1_epi8('N'), Dd = _mm256_set1_epi8('-');
    size_t w = 0;
    for (; 32 * w + 32 <= slen; w++) {
        const __m256i v = _mm256_loadu_si256((const __m256i *)(seq + 32 * w));
        const uint32_t a = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, A));
        const uint32_t c = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Cc));
        const uint32_t g = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Gg));
        const uint32_t t = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Tt));
        const uint32_t n = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Nn));
        const uint32_t d = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Dd));
        const uint32_t bad = ~(a | c | g | t | n | d);
        o[4 * w] = c | t | d | bad;
        o[4 * w + 1] = g | t | bad;
        o[4 * w + 2] = n | d | bad;
        o[4 * w + 3] = bad;
    }
    if (32 * w < slen) {   // the tail through a 32-byte copy padded with 'A' (all planes 0)
        alignas(32) char t[32];
        memset(t, 'A', sizeof(t));
        memcpy(t, seq + 32 * w, slen - 32 * w);
        const __m256i v = _mm256_load_si256((const __m256i *)t);
        const uint32_t a = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, A));
        const uint32_t c = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Cc));
        const uint32_t g = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Gg));
        const uint32_t tt = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Tt));
        const uint32_t n = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Nn));
        const uint32_t d = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, Dd));
        const uint32_t bad = ~(a | c | g | tt | n | d);
        o[4 * w] = c | tt | d | bad;
        o[4 * w + 1] = g | tt | bad;
        o[4 * w + 2] = n | d | bad;
        o[4 * w + 3] = bad;
    }
}
static const bool HAVE_AVX2 = __builtin_cpu_supports("avx2");
#endif
static void seq_planes(const char *seq, size_t slen, uint32_t *o) {
#if defined(__x86_64__)
    if (HAVE_AVX2) return seq_planes_avx2(seq, slen, o);
#endif
    seq_planes_scalar(seq, slen, o);
}
// the set bits of plane word group k (0 p0, 1 p1, 2 x, 3 bad) in chars [a, b)
static inline uint32_t plane_bits(const uint32_t *sp, int k, size_t a, size_t b, bool any) {
    uint32_t tot = 0;
    for (size_t w = a >> 5; w < ((b + 31) >> 5); w++) {
        uint32_t m = k == 4 ? sp[4 * w + 2] & sp[4 * w] & ~sp[4 * w + 1] : sp[4 * w + k];   // 4: '-' chars
        if (w == (a >> 5)) m &= ~0u << (a & 31);
        if (w == ((b - 1) >> 5) && (b & 31)) m &= ~0u >> (32 - (b & 31));
        if (any && m) return 1;
        tot += (uint32_t)__builtin_popcount(m);
    }
    return tot;
}
// QL code of char i from the planes
static inline uint8_t plane_code(const uint32_t *sp, size_t i) {
    const size_t w = i >> 5, j = i & 31;
    if ((sp[4 * w + 3] >> j) & 1u) return Q_BAD;
    return (uint8_t)(((sp[4 * w] >> j) & 1u) | (((sp[4 * w + 1] >> j) & 1u) << 1) | (((sp[4 * w + 2] >> j) & 1u) << 2));
}

// The read's planes (seq_planes) → the chunk's planes at a 16-base boundary; returns the
// first base index.  *has_x: bit 0 = a non-ACGT char, bit 1 = a '-' char (x = 1, p1 = 0, p0 = 1)
static uint64_t pack_seq(Chunk &c, const uint32_t *sp, size_t slen, uint8_t *has_x) {
    const uint64_t q0 = (c.nq + 15) & ~(uint64_t)15;
    const uint64_t q1 = q0 + slen;
    const size_t need = (size_t)((q1 + 31) >> 5) + 1;
    if (c.bx.size() < need) {   // (grown without a fill: the words are zeroed as reached, below)
        size_t cap = std::max(need, c.bx.size() * 2);
        c.bq.resize(2 * cap);
        c.bx.resize(cap);
    }
    if (c.nz < need) {   // the words first reached by this read (and the funnel word after it)
        memset(&c.bq[2 * c.nz], 0, 8 * (need - c.nz));
        memset(&c.bx[c.nz], 0, 4 * (need - c.nz));
        c.nz = need;
    }
    uint8_t anyx = 0;
    const uint32_t sh = (uint32_t)(q0 & 31);   // 0 or 16
    const uint64_t w0 = q0 >> 5;
    const size_t nw = (slen + 31) / 32;
    for (size_t w = 0; w < nw; w++) {
        const uint32_t p0 = sp[4 * w], p1 = sp[4 * w + 1], x = sp[4 * w + 2];
        anyx |= (x != 0 ? 1 : 0) | ((x & p0 & ~p1) != 0 ? 2 : 0);
        c.bq[2 * (w0 + w)] |= p0 << sh;
        c.bq[2 * (w0 + w) + 1] |= p1 << sh;
        c.bx[w0 + w] |= x << sh;
        if (sh) {
            c.bq[2 * (w0 + w + 1)] |= p0 >> (32 - sh);
            c.bq[2 * (w0 + w + 1) + 1] |= p1 >> (32 - sh);
            c.bx[w0 + w + 1] |= x >> (32 - sh);
        }
    }
    c.nq = q1;
    *has_x = anyx;
    return q0;
}

// The first ten tab-separated fields of line [s, end) (end after its '\n' when present: the
// last field split keeps it, as line.split('\t') does, :191); returns how many.
static int split_fields(const char *s, const char *end, const char **f, size_t *fl, int maxf = 10) {
    int nf = 0;
    const char *cur = s;
    while (nf < maxf) {
        const char *t = (const char *)memchr(cur, '\t', end - cur);
        f[nf] = cur;
        if (!t) { fl[nf++] = end - cur; break; }
        fl[nf++] = t - cur;
        cur = t + 1;
    }
    return nf;
}

// One line of a parse piece [s, lim): its end (after its '\n', else lim) and split_fields of
// it, in one pass — 32 bytes per step compared against '\t' and '\n' at once.
#if defined(__x86_64__)
__attribute__((target("avx2,bmi"))) static const char *scan_line_avx2(const char *s, const char *lim, const char **f,
                                                                     size_t *fl, int *nfo) {
    const __m256i T = _mm256_set1_epi8('\t'), N = _mm256_set1_epi8('\n');
    int nf = 0;
    const char *cur = s, *p = s;
    for (; p + 32 <= lim; p += 32) {
        const __m256i v = _mm256_loadu_si256((const __m256i *)p);
        const uint32_t mn = (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, N));
        uint32_t mt = nf < 10 ? (uint32_t)_mm256_movemask_epi8(_mm256_cmpeq_epi8(v, T)) : 0u;
        if (mn) mt &= (mn & (0u - mn)) - 1u;   // (the tabs before the line's '\n')
        while (mt && nf < 10) {
            const uint32_t i = (uint32_t)__builtin_ctz(mt);
            mt &= mt - 1;
            f[nf] = cur;
            fl[nf++] = (size_t)(p + i - cur);
            cur = p + i + 1;
        }
        if (mn) {
            const char *e = p + __builtin_ctz(mn) + 1;
            if (nf < 10) {
                f[nf] = cur;
                fl[nf++] = (size_t)(e - cur);
            }
            *nfo = nf;
            return e;
        }
    }
    const char *nl = (const char *)memchr(p, '\n', lim - p);   // (the piece's last < 32 bytes)
    const char *e = nl ? nl + 1 : lim;
    if (nf < 10) nf += split_fields(cur, e, f + nf, fl + nf, 10 - nf);
    *nfo = nf;
    return e;
}
#endif
static const char *scan_line(const char *s, const char *lim, const char **f, size_t *fl, int *nfo) {
#if defined(__x86_64__)
    if (HAVE_AVX2) return scan_line_avx2(s, lim, f, fl, nfo);
#endif
    const char *nl = (const char *)memchr(s, '\n', lim - s);
    const char *e = nl ? nl + 1 : lim;
    *nfo = split_fields(s, e, f, fl);
    return e;
}

static int process_fields(Chunk &c, const RefView &rv, std::string &last_name, int64_t &last_ref, const char **f,
                          const size_t *fl, int nf, std::string &emsg);
// One SAM record line (not a header line), n includes the trailing '\n' when present.
static int process_record(Chunk &c, const RefView &rv, std::string &last_name, int64_t &last_ref,
                          const char *s, size_t n, std::string &emsg) {
    const char *f[10];
    size_t fl[10];
    const int nf = s[0] == '@' ? 0 : split_fields(s, s + n, f, fl);
    return process_fields(c, rv, last_name, last_ref, s[0] == '@' ? nullptr : f, fl, nf, emsg);
}
// The record of fields f (nullptr: a line starting with '@' inside the records, :195).
static int process_fields(Chunk &c, const RefView &rv, std::string &last_name, int64_t &last_ref, const char **f,
                          const size_t *fl, int nf, std::string &emsg) {
    c.lines_total++;
    if (!f) return S2C_OK;                                             // :195
    auto fail = [&](int code, const std::string &m) { emsg = m; return code; };
    if (nf < 6) return fail(S2C_ERR_INDEX, "IndexError: record with < 6 fields (:195)");
    if (fl[5] == 1 && f[5][0] == '*') return S2C_OK;                  // unmapped (:195)
    c.reads_mapped++;
    const char *nb;
    size_t nl;
    if (!py2_first_token(f[2], fl[2], &nb, &nl)) return fail(S2C_ERR_INDEX, "IndexError: empty RNAME (:200)");
    int64_t pos1;
    if (!py2_int(f[3], fl[3], &pos1))
        return fail(S2C_ERR_VALUE, "ValueError: invalid POS '" + std::string(f[3], fl[3]) + "' (:201)");
    const int64_t pos0 = pos1 - 1;
    if (nf < 10) return fail(S2C_ERR_INDEX, "IndexError: record with < 10 fields (:206)");

    // ---- CIGAR tokens (:58-59) ----
    const uint64_t tok0 = c.toks.size();
    uint32_t ntok = 0;
    int rc = tokenize_cigar(f[5], fl[5], c.toks, &ntok);
    if (rc) return fail(rc, s2c_last_error());
    const char *seq = f[9];
    const int64_t slen = (int64_t)fl[9];
    if (slen >= ((int64_t)1 << 24)) return fail(S2C_ERR_LIMIT, "SEQ of 2^24 or more chars not supported");

    // ---- reference lookup: sequences[refname] / insertions[refname] (:212,:217,:221) ----
    int64_t ref;
    if (last_ref >= 0 && last_name.size() == nl && memcmp(last_name.data(), nb, nl) == 0) {
        ref = last_ref;
    } else {
        std::string name(nb, nl);
        auto it = rv.idx->find(name);
        ref = it == rv.idx->end() ? -1 : (int64_t)it->second;
        if (ref >= 0) { last_ref = ref; last_name = name; }
    }

    // ---- the token walk of parsecigar (:64-81): seqout length, its '-' count, the codes of
    //      the bases it takes (validated below), insertion events with non-empty motifs ----
    std::vector<uint32_t> &sp = c.sp;   // SEQ planes (query order)
    if (sp.size() < 4 * (size_t)((slen + 31) / 32)) sp.resize(4 * (size_t)((slen + 31) / 32) + 64);
    seq_planes(seq, (size_t)slen, sp.data());
    int64_t start = 0, start_ref = pos0, klen = 0, dashes = 0, mb = 0;
    bool any_bad = false;
    const uint32_t ev0 = (uint32_t)c.ev.size();
    uint32_t nev = 0;
    for (uint32_t t = 0; t < ntok; t++) {
        const uint32_t w = c.toks[tok0 + t], op = w & 15u;
        const int64_t l = (int64_t)(w >> 4);
        if (op_bases(op)) {
            const int64_t take = start < slen ? std::min(l, slen - start) : 0;
            if (take > 0) {
                dashes += plane_bits(sp.data(), 4, (size_t)start, (size_t)(start + take), false);
                any_bad |= plane_bits(sp.data(), 3, (size_t)start, (size_t)(start + take), true) != 0;
            }
            klen += take;
            mb += take;
            start += l;
            start_ref += l;
        } else if (op_dash(op)) {
            klen += l;
            dashes += l;
            start_ref += l;
        } else if (op == S2C_OP_I) {
            const int64_t take = start < slen ? std::min(l, slen - start) : 0;
            if (take > 0) {   // an empty motif never reaches a column (:280-287)
                c.ev.push_back({start_ref, (uint64_t)start, (uint32_t)std::max<int64_t>(ref, 0), (uint32_t)take,
                                (uint32_t)c.reads.size()});
                nev++;
                c.qbases += take;
            }
            start += l;
        } else if (op == S2C_OP_S) {
            start += l;
        }
        if (op != S2C_OP_S && op != S2C_OP_H) c.ntokens++;
    }
    if (klen >= ((int64_t)1 << S2C_RUN_KSHIFT)) return fail(S2C_ERR_LIMIT, "seqout of 2^27 or more positions not supported");
    c.aligned += klen;
    c.qbases += mb;
    if (ref < 0) return fail(S2C_ERR_KEY, "KeyError: '" + std::string(nb, nl) + "' (:212/:221)");
    const int64_t L = (*rv.len)[ref];

    // ---- maxdel rule (:210) and the checks of :211-218 in seqout order: index, then symbol ----
    const bool drop = rv.maxdel_active && dashes > rv.maxdel;
    const bool in_range = pos0 >= 0 && pos0 + klen <= L;
    int64_t kc0 = -1, kc1 = -1;
    if (!in_range || any_bad || drop) {
        int64_t k = 0, st = 0;
        for (uint32_t t = 0; t < ntok; t++) {
            const uint32_t w = c.toks[tok0 + t], op = w & 15u;
            const int64_t l = (int64_t)(w >> 4);
            int64_t take = 0;
            bool bases = false;
            if (op_bases(op)) { take = st < slen ? std::min(l, slen - st) : 0; bases = true; }
            else if (op_dash(op)) take = l;
            for (int64_t j = 0; j < take; j++, k++) {
                const uint8_t cd = bases ? plane_code(sp.data(), (size_t)(st + j)) : Q_DASH;
                if (drop && cd == Q_DASH) continue;            // '-' skipped (:216)
                const int64_t pp = pos0 + k;
                if (pp < -L || pp >= L) return fail(S2C_ERR_INDEX, "IndexError: list index out of range (:212)");
                if (cd == Q_BAD) return fail(S2C_ERR_KEY, "KeyError: base not in -ACGNT (:212)");
                if (kc0 < 0) kc0 = k;
                kc1 = k + 1;
            }
            if (bases || op == S2C_OP_I || op == S2C_OP_S) st += l;
        }
    } else if (klen > 0) {
        kc0 = 0;
        kc1 = klen;
    }
    for (uint32_t e = ev0; e < ev0 + nev; e++) c.ev[e].ref = (uint32_t)ref;
    ReadRec r;
    r.pos0 = pos0;
    r.klen = klen;
    r.kc0 = kc0;
    r.kc1 = kc1;
    r.tok = tok0;
    r.ref = (uint32_t)ref;
    r.ntok = ntok;
    r.slen = (uint32_t)slen;
    r.ev0 = ev0;
    r.nev = nev;
    r.drop = drop;
    if (kc0 >= 0 || nev > 0) {
        r.q = pack_seq(c, sp.data(), (size_t)slen, &r.has_x);
        for (uint32_t e = ev0; e < ev0 + nev; e++) c.ev[e].q += r.q;
    } else {
        r.q = 0;
        r.has_x = 0;
        c.toks.resize(tok0);   // nothing reaches the device from this read
        r.ntok = 0;
    }
    c.reads.push_back(r);
    c.bound((uint32_t)ref, pos0, klen, L);
    return S2C_OK;
}

// One line of the sequential feed (header lines included).
static int process_line(s2c_parser *p, const char *s, size_t n) {
    if (p->in_header) {
        if (s[0] == '@') {
            p->header_lines++;
            p->chunks.back()->lines_total++;
            if (n >= 3 && s[1] == 'S' && s[2] == 'Q') return parse_sq(p, s, n);
            return S2C_OK;
        }
        p->in_header = false;
    }
    RefView rv{&p->ref_idx, &p->ref_len, p->maxdel_active, p->maxdel};
    std::string emsg;
    int rc = process_record(*p->chunks.back(), rv, p->last_name, p->last_ref, s, n, emsg);
    if (rc) return perr(p, rc, emsg);
    return S2C_OK;
}

static int s2c_parser_new_impl(int maxdel_active, int64_t maxdel, s2c_parser **out) {
    if (!out) return s2c_set_error(S2C_ERR_ARG, "out is NULL");
    s2c_parser *p = new s2c_parser();
    p->maxdel_active = maxdel_active != 0;
    p->maxdel = maxdel;
    *out = p;
    return S2C_OK;
}
extern "C" int s2c_parser_new(int maxdel_active, int64_t maxdel, s2c_parser **out) {
    return s2c_guarded([&] { return s2c_parser_new_impl(maxdel_active, maxdel, out); });
}

extern "C" void s2c_parser_free(s2c_parser *p) { delete p; }

static int s2c_parser_feed_impl(s2c_parser *p, const char *buf, size_t len) {
    if (!p) return s2c_set_error(S2C_ERR_ARG, "parser is NULL");
    if (p->detached) return s2c_set_error(S2C_ERR_ARG, "a detached parser takes no input");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    const char *s = buf, *end = buf + len;
    if (!p->carry.empty()) {
        const char *nl = (const char *)memchr(s, '\n', end - s);
        if (!nl) { p->carry.append(s, len); return S2C_OK; }
        p->carry.append(s, nl + 1 - s);
        int rc = process_line(p, p->carry.data(), p->carry.size());
        p->carry.clear();
        if (rc) return rc;
        s = nl + 1;
    }
    if (end - s >= (ptrdiff_t)(4 << 20)) {   // a large block: its whole lines in parallel pieces
        const char *cut = end;
        while (cut > s && cut[-1] != '\n') cut--;
        if (cut > s) {
            int rc = parse_window(p, s, (size_t)(cut - s));
            if (rc) return rc;
            s = cut;
        }
        if (s < end) p->carry.assign(s, end - s);
        return S2C_OK;
    }
    while (s < end) {
        const char *nl = (const char *)memchr(s, '\n', end - s);
        if (!nl) { p->carry.assign(s, end - s); break; }
        int rc = process_line(p, s, nl + 1 - s);
        if (rc) return rc;
        s = nl + 1;
    }
    return S2C_OK;
}
extern "C" int s2c_parser_feed(s2c_parser *p, const char *buf, size_t len) {
    return s2c_guarded([&] { return s2c_parser_feed_impl(p, buf, len); });
}

extern "C" int s2c_parser_end_header(s2c_parser *p) {
    if (!p) return s2c_set_error(S2C_ERR_ARG, "parser is NULL");
    if (p->detached) return s2c_set_error(S2C_ERR_ARG, "a detached parser takes no input");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    if (!p->carry.empty()) return s2c_set_error(S2C_ERR_ARG, "header does not end with a newline");
    p->in_header = false;
    return S2C_OK;
}

static int feed_flush(s2c_parser *p) {
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    if (!p->carry.empty()) {   // last line without '\n'
        std::string last;
        last.swap(p->carry);
        int rc = process_line(p, last.data(), last.size());
        if (rc) return rc;
    }
    return S2C_OK;
}

// ------------------------------------------------------------------ parallel file parse
// A file is read in bounded windows (s2c_reader.cpp: WIN bytes, cut after the last '\n'; the
// partial last line carries into the next window), as the reference reads 50 KB chunks
// (:185-189).  In each window the header lines (:149-172) go first, in order; the record lines are cut
// into pieces at line ends, each parsed by its own thread into its own Chunk (the same
// process_record); chunks are kept in file order.  The first failing record in file order
// decides the error: a chunk stops at its first error, and no later chunk is kept.
int parse_window(s2c_parser *p, const char *s, size_t n) {
    size_t i = 0;
    while (i < n && p->in_header) {
        if (s[i] != '@') { p->in_header = false; break; }
        const char *nl = (const char *)memchr(s + i, '\n', n - i);
        const size_t e = nl ? (size_t)(nl - s) + 1 : n;
        int rc = process_line(p, s + i, e - i);
        if (rc) return rc;
        i = e;
    }
    if (i == n) return S2C_OK;
    const size_t body = n - i;
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)std::min<size_t>(std::min<unsigned>(hw ? hw : 1, 16), std::max<size_t>(1, body >> 22));   // ≥ 4 MB each
    if (const char *e = getenv("S2C_PARSE_THREADS")) nt = std::max(1, std::min(64, atoi(e)));
    // 4 pieces per thread (≥ 1 MB each), taken in turn by the threads: a thread slowed by
    // the others' work (a streamed snapshot planning beside the feed) holds up the window by
    // one piece, not by its fixed share
    const int np = nt == 1 ? 1 : (int)std::min<size_t>((size_t)nt * 4, std::max<size_t>((size_t)nt, body >> 20));
    std::vector<size_t> cut(np + 1, n);
    cut[0] = i;
    for (int k = 1; k < np; k++) {   // piece k starts after the line end nearest to its share
        size_t c = std::max(cut[k - 1], i + body * k / np);
        const char *nl = c < n ? (const char *)memchr(s + c, '\n', n - c) : nullptr;
        cut[k] = nl ? (size_t)(nl - s) + 1 : n;
    }
    std::vector<std::unique_ptr<Chunk>> cs(np);
    std::vector<int> rcs(np, S2C_OK);
    std::vector<std::string> msgs(np);
    RefView rv{&p->ref_idx, &p->ref_len, p->maxdel_active, p->maxdel};
    auto work = [&](int k) {
        cs[k].reset(new Chunk());
        Chunk &c = *cs[k];
        std::string last_name;
        int64_t last_ref = -1;
        const char *b = s + cut[k];
        const size_t m = cut[k + 1] - cut[k];
        c.reads.reserve(m / 150 + 16);   // (SAM lines of ≥ 150 bytes: no regrowth for typical reads)
        c.toks.reserve(m / 100 + 16);
        c.bx.resize(m / 32 + 64);     // SEQ bytes ≤ m: planes of ≤ m bases, 16-base aligned reads
        c.bq.resize(2 * c.bx.size());  // (no fill: pack_seq zeroes the words it reaches)
        size_t j = 0;
        while (j < m) {   // (a last line without '\n' counts, Py2)
            const char *f[10];
            size_t fl[10];
            int nf;
            const size_t e = (size_t)(scan_line(b + j, b + m, f, fl, &nf) - b);
            rcs[k] = process_fields(c, rv, last_name, last_ref, b[j] == '@' ? nullptr : f, fl, nf, msgs[k]);
            if (rcs[k]) return;
            j = e;
        }
    };
    static const bool timing = getenv("S2C_HOST_TIMING") != nullptr;
    std::vector<double> tw(nt, 0.0);
    const auto t0 = std::chrono::steady_clock::now();
    std::atomic<int> next{0};
    std::vector<double> ts(nt, 0.0);
    auto worker = [&](int t) {
        const auto a = std::chrono::steady_clock::now();
        for (int k; (k = next++) < np;) work(k);
        tw[t] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
        ts[t] = std::chrono::duration<double, std::milli>(a - t0).count();
    };
    WorkerPool::get(POOL_PARSE).run(nt, worker);
    if (timing) {   // (S2C_HOST_TIMING: the window's wall time, its threads' longest and mean)
        double mx = 0, sm = 0;
        for (double x : tw) { mx = std::max(mx, x); sm += x; }
        double smax = 0;
        for (double x : ts) smax = std::max(smax, x);
        fprintf(stderr, "[s2c feed] %zu B %d thr %d pieces wall %.2f ms max %.2f mean %.2f last start %.2f\n", n - i, nt, np,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), mx, sm / nt, smax);
    }
    for (int k = 0; k < np; k++) {
        if (!cs[k]->reads.empty() || cs[k]->lines_total) p->chunks.push_back(std::move(cs[k]));
        if (rcs[k]) return perr(p, rcs[k], msgs[k]);
    }
    return S2C_OK;
}

// Global coordinate of each reference's position 0 (header order, S2C_POS_ALIGN-aligned).
static std::vector<int64_t> ref_offsets(const s2c_parser *p, int64_t *padded) {
    std::vector<int64_t> off(p->ref_len.size());
    int64_t g = 0;
    for (size_t r = 0; r < off.size(); r++) {
        off[r] = g;
        g = (g + p->ref_len[r] + S2C_POS_ALIGN - 1) / S2C_POS_ALIGN * S2C_POS_ALIGN;
    }
    if (padded) *padded = g;
    return off;
}

// Global positions a read can change: its counted chars (the POS<=0 wrap puts the leading
// part at the reference's end, :212) and its emitted insertion keys.  false: none.
static bool read_extent(const Chunk &c, const ReadRec &r, int64_t off, int64_t L, int64_t *lo, int64_t *hi) {
    int64_t a = INT64_MAX, b = INT64_MIN;
    if (r.kc0 >= 0) {
        const int64_t pa = r.pos0 + r.kc0, pb = r.pos0 + r.kc1;   // [pa, pb) reference-relative
        if (pa < 0) {
            a = std::min(a, off + L + pa);
            b = std::max(b, off + L + std::min<int64_t>(pb, 0) - 1);
            if (pb > 0) { a = off; b = std::max(b, off + pb - 1); }
        } else {
            a = off + pa;
            b = off + pb - 1;
        }
    }
    for (uint32_t e = r.ev0; e < r.ev0 + r.nev; e++)
        if (c.ev[e].key >= 0) {
            a = std::min(a, off + c.ev[e].key);
            b = std::max(b, off + c.ev[e].key);
        }
    *lo = a;
    *hi = b;
    return a <= b;
}

// pred(chunk, read, ref_off) of every read held in chunks [c0, end), on the host threads (the
// streamed batches' per-read tests: a few ms per million reads instead of tens): flags in
// chunk-then-read order
template <class Pred, class ChunkPred>
static std::vector<uint8_t> read_flags(const s2c_parser *p, size_t c0, const std::vector<int64_t> &off, Pred &&pred,
                                       ChunkPred &&chunk_may) {
    const size_t nc = p->chunks.size() > c0 ? p->chunks.size() - c0 : 0;
    std::vector<int64_t> base(nc + 1, 0);
    std::vector<uint8_t> may(nc, 1);   // (chunk_may false: every flag of the chunk is 0, no read looked at)
    for (size_t i = 0; i < nc; i++) {
        may[i] = chunk_may(*p->chunks[c0 + i]) ? 1 : 0;
        base[i + 1] = base[i] + (may[i] ? (int64_t)p->chunks[c0 + i]->reads.size() : 0);
    }
    const int64_t n = base[nc];
    std::vector<uint8_t> g((size_t)n, 0);
    par_ranges(plan_threads(n, 1 << 15), n, [&](int, int64_t i0, int64_t i1) {
        if (i0 >= i1) return;
        size_t ci = (size_t)(std::upper_bound(base.begin(), base.end(), i0) - base.begin()) - 1;
        for (int64_t i = i0; i < i1; i++) {
            while (i >= base[ci + 1]) ci++;
            const Chunk &c = *p->chunks[c0 + ci];
            const ReadRec &r = c.reads[(size_t)(i - base[ci])];
            g[(size_t)i] = pred(c, r, off[r.ref]) ? 1 : 0;
        }
    });
    // the flags of every read, chunk by chunk (0 for the chunks skipped)
    std::vector<uint8_t> f;
    f.reserve(n);
    for (size_t i = 0; i < nc; i++) {
        if (may[i]) f.insert(f.end(), g.begin() + base[i], g.begin() + base[i + 1]);
        else f.insert(f.end(), p->chunks[c0 + i]->reads.size(), (uint8_t)0);
    }
    return f;
}

// Whether a read parsed since the last retain reaches below its frontier.
static void check_late(s2c_parser *p) {
    if (p->frontier <= 0 || p->late) return;
    const std::vector<int64_t> off = ref_offsets(p, nullptr);
    const std::vector<uint8_t> f = read_flags(p, p->n_kept, off, [&](const Chunk &c, const ReadRec &r, int64_t o) {
        int64_t lo, hi;
        return read_extent(c, r, o, p->ref_len[r.ref], &lo, &hi) && lo < p->frontier;
    }, [](const Chunk &) { return true; });
    p->late = std::find(f.begin(), f.end(), (uint8_t)1) != f.end();
}

static int s2c_parser_finish_impl(s2c_parser *p, s2c_batch **out) {
    if (!p || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    int rc = feed_flush(p);
    if (rc) return rc;
    check_late(p);
    return build_batch(p, out);
}
extern "C" int s2c_parser_finish(s2c_parser *p, s2c_batch **out) {
    return s2c_guarded([&] { return s2c_parser_finish_impl(p, out); });
}

static int s2c_parser_set_tile_width_impl(s2c_parser *p, int64_t width) {
    if (!p) return s2c_set_error(S2C_ERR_ARG, "parser is NULL");
    if (width != 0 && (width < S2C_POS_ALIGN || width > 2048 || width % S2C_POS_ALIGN))
        return s2c_set_error(S2C_ERR_ARG, "tile width must be 0 or a multiple of 64 in [64, 2048]");
    p->tile_width = width;
    return S2C_OK;
}
extern "C" int s2c_parser_set_tile_width(s2c_parser *p, int64_t width) {
    return s2c_guarded([&] { return s2c_parser_set_tile_width_impl(p, width); });
}

// The batch of everything parsed so far (the partial last line stays unparsed); the
// parser keeps going.  With t_from >= 0 (s2c_parser_snapshot_from) only the tiles a streamed
// batch can run are planned: from t_from through the tile of the reads' last position.
static int s2c_parser_snapshot_impl(s2c_parser *p, int64_t t_from, s2c_batch **out) {
    if (!p || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    if (t_from >= 0 && p->tile_width <= 0) return s2c_set_error(S2C_ERR_ARG, "a ranged snapshot needs a tile width");
    check_late(p);
    p->plan_from = t_from;
    const int rc = build_batch(p, out);
    p->plan_from = -1;
    return rc;
}
extern "C" int s2c_parser_snapshot(s2c_parser *p, s2c_batch **out) {
    return s2c_guarded([&] { return s2c_parser_snapshot_impl(p, -1, out); });
}
extern "C" int s2c_parser_snapshot_from(s2c_parser *p, int64_t t_from, s2c_batch **out) {
    if (t_from < 0) return s2c_set_error(S2C_ERR_ARG, "t_from < 0");
    return s2c_guarded([&] { return s2c_parser_snapshot_impl(p, t_from, out); });
}

// Append read r of chunk c to chunk d (its tokens, planes and events; no line counted
// again); with events_only it keeps only its insertion events (counted range cleared).
static void append_read(Chunk &d, const Chunk &c, const ReadRec &r, bool events_only) {
    ReadRec n = r;
    if (events_only) n.kc0 = n.kc1 = -1;
    n.tok = d.toks.size();
    d.toks.insert(d.toks.end(), c.toks.begin() + r.tok, c.toks.begin() + r.tok + r.ntok);
    n.ev0 = (uint32_t)d.ev.size();
    if (r.kc0 >= 0 || r.nev > 0) {   // its planes
        const uint64_t q0 = (d.nq + 15) & ~(uint64_t)15, q1 = q0 + r.slen;
        const size_t need = (size_t)((q1 + 31) >> 5) + 1;
        if (d.bx.size() < need) {
            const size_t cap = std::max(need, d.bx.size() * 2);
            d.bq.resize(2 * cap, 0u);
            d.bx.resize(cap, 0u);
            d.nz = cap;   // (zero-filled)
        }
        copy_planes(d.bq.data(), d.bx.data(), q0 / 16, c.bq.data(), c.bx.data(), r.q / 16, r.slen);
        d.nq = q1;
        n.q = q0;
    }
    for (uint32_t e = r.ev0; e < r.ev0 + r.nev; e++) {
        Event ev = c.ev[e];
        ev.q = ev.q - r.q + n.q;
        ev.read = (uint32_t)d.reads.size();
        d.ev.push_back(ev);
    }
    d.reads.push_back(n);
}

// Move the reads `keep` selects into one chunk; with events_only they keep only their
// insertion events (their counts are already in the running totals).
template <class Keep, class ChunkMay>
static void compact_reads(s2c_parser *p, Keep keep, ChunkMay chunk_may, bool events_only) {
    PhaseClock clk;
    const std::vector<int64_t> off = ref_offsets(p, nullptr);
    // (the tests in parallel — skipping the chunks chunk_may rules out — the copies in order)
    const std::vector<uint8_t> f = read_flags(p, 0, off, keep, [&](const Chunk &c) { return chunk_may(c, off); });
    clk.mark("retain tests");
    std::unique_ptr<Chunk> k(new Chunk());
    size_t i = 0;
    for (auto &cp : p->chunks)
        for (const ReadRec &r : cp->reads)
            if (f[i++]) {
                append_read(*k, *cp, r, events_only);
                k->bound(r.ref, r.pos0, r.klen, p->ref_len[r.ref]);
            }
    clk.mark("retain copies");
    // the dropped chunks' memory goes back on a thread of its own (hundreds of MB of reads:
    // tens of ms of page unmapping off the producer's path)
    p->free_later(std::move(p->chunks));
    p->chunks = std::vector<std::unique_ptr<Chunk>>();
    clk.mark("retain free");
    p->chunks.push_back(std::move(k));
    p->chunks.emplace_back(new Chunk());   // the sequential feed appends here
    p->n_kept = 1;
}

// Drop the reads that cannot change a global position >= gmin (their positions below it
// are emitted).
static int s2c_parser_retain_impl(s2c_parser *p, int64_t gmin) {
    if (!p) return s2c_set_error(S2C_ERR_ARG, "parser is NULL");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    if (gmin < p->frontier) return s2c_set_error(S2C_ERR_ARG, "retain: frontier moves backwards");
    compact_reads(p, [&](const Chunk &c, const ReadRec &r, int64_t off) {
        int64_t lo, hi;
        return read_extent(c, r, off, p->ref_len[r.ref], &lo, &hi) && hi >= gmin;
    }, [&](const Chunk &c, const std::vector<int64_t> &off) {   // (no read of c can reach gmin)
        // (a chunk without bounds — s2c_parser_unpack's — may hold any read: test its reads)
        if (c.hb_pos < 0) return !c.reads.empty();
        return off[c.hb_ref] + c.hb_pos >= gmin;
    }, false);
    p->frontier = gmin;
    return S2C_OK;
}
extern "C" int s2c_parser_retain(s2c_parser *p, int64_t gmin) {
    return s2c_guarded([&] { return s2c_parser_retain_impl(p, gmin); });
}

// Unsorted input: the counts of every read held are in the running totals; keep only the
// reads with insertion events, as event-only reads (their motifs are counted once, by the
// last batch, which holds every event — and the insertion checks of :284-294 see them all).
static int s2c_parser_retain_events_impl(s2c_parser *p) {
    if (!p) return s2c_set_error(S2C_ERR_ARG, "parser is NULL");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    compact_reads(p, [](const Chunk &, const ReadRec &r, int64_t) { return r.nev > 0; },
                  [](const Chunk &c, const std::vector<int64_t> &) { return !c.ev.empty(); }, true);
    return S2C_OK;
}
extern "C" int s2c_parser_retain_events(s2c_parser *p) {
    return s2c_guarded([&] { return s2c_parser_retain_events_impl(p); });
}

// Pipelined snapshots (s2c.h): the reads held move to a new parser with the same reference
// table and stream state; the feeding parser keeps its partial line and starts a new chunk.
static int s2c_parser_detach_impl(s2c_parser *p, s2c_parser **out) {
    if (!p || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    std::unique_ptr<s2c_parser> d(new s2c_parser());
    d->maxdel_active = p->maxdel_active;
    d->maxdel = p->maxdel;
    d->in_header = p->in_header;
    d->header_lines = p->header_lines;
    d->ref_names = p->ref_names;   // (the name index stays behind: d parses nothing)
    d->ref_len = p->ref_len;
    d->detached = true;
    d->last_name = p->last_name;
    d->last_ref = p->last_ref;
    d->tile_width = p->tile_width;
    d->frontier = p->frontier;
    d->n_kept = p->n_kept;
    d->late = p->late;
    d->chunks = std::move(p->chunks);
    p->chunks.clear();
    p->chunks.emplace_back(new Chunk());   // the sequential feed appends here
    p->n_kept = 0;
    *out = d.release();
    return S2C_OK;
}
extern "C" int s2c_parser_detach(s2c_parser *p, s2c_parser **out) {
    return s2c_guarded([&] { return s2c_parser_detach_impl(p, out); });
}
static int s2c_parser_attach_impl(s2c_parser *p, s2c_parser *det) {
    if (!p || !det) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    std::unique_ptr<s2c_parser> d(det);
    if (d->err && !p->err) {   // (an error of the detached reads comes first in file order)
        p->err = d->err;
        p->errmsg = d->errmsg;
    }
    std::vector<std::unique_ptr<Chunk>> cs = std::move(d->chunks);
    const size_t kept = cs.size();
    for (auto &c : p->chunks) cs.push_back(std::move(c));
    p->chunks = std::move(cs);
    // the detached parser's retained chunks are the kept ones; the reads fed since follow
    p->n_kept = kept;
    p->frontier = std::max(p->frontier, d->frontier);
    p->late = p->late || d->late;
    return S2C_OK;
}
extern "C" int s2c_parser_attach(s2c_parser *p, s2c_parser *det) {
    return s2c_guarded([&] { return s2c_parser_attach_impl(p, det); });
}

// state[0] = 1 if a read parsed after a retain reached below its frontier; state[1..2] =
// (reference index, POS - 1) of the last mapped read in file order (-1, 0: none yet);
// state[3] = reads held.
extern "C" int s2c_parser_stream_state(const s2c_parser *p, int64_t *state) {
    if (!p || !state) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    state[0] = p->late ? 1 : 0;
    state[1] = -1;
    state[2] = 0;
    state[3] = 0;
    for (auto it = p->chunks.rbegin(); it != p->chunks.rend(); ++it)
        if (!(*it)->reads.empty() && state[1] < 0) {
            state[1] = (*it)->reads.back().ref;
            state[2] = (*it)->reads.back().pos0;
        }
    for (auto &cp : p->chunks) state[3] += (int64_t)cp->reads.size();
    return S2C_OK;
}

// The insertion checks of the reformat phase (:284-294) over the reads held, per reference:
// a motif base outside -ACGNT (:287), a key outside the coverage list (:294).
void insertion_checks(const s2c_parser *p, std::vector<uint8_t> &bad_sym, std::vector<uint8_t> &bad_key) {
    const size_t R = p->ref_names.size();
    bad_sym.assign(R, 0);
    bad_key.assign(R, 0);
    for (auto &cp : p->chunks) {
        const Chunk &c = *cp;
        for (const Event &e : c.ev) {
            const int64_t L = p->ref_len[e.ref];
            for (uint32_t j = 0; j < e.len; j++) {
                const uint64_t b = e.q + j;
                const uint32_t x = (c.bx[b >> 5] >> (b & 31)) & 1u, p1 = (c.bq[2 * (b >> 5) + 1] >> (b & 31)) & 1u;
                if (x && p1) { bad_sym[e.ref] = 1; break; }   // code 7: not in -ACGNT
            }
            if (e.key < -L || e.key >= L) bad_key[e.ref] = 1;
        }
    }
}

// ------------------------------------------------------------------ distributed parse
// Multi-GPU CLI (sam2consensus_amd/dparse.py): every rank parses its blocks of the file;
// each read goes to the ranks whose position range it can change (read_extent, as the
// streamed retain); a rank plans its sub-batch from the reads it receives.

static int s2c_parser_pos_weights_impl(s2c_parser *p, int64_t shift, int64_t *w, int64_t n) {
    if (!p || (!w && n > 0) || shift < 0 || shift > 40) return s2c_set_error(S2C_ERR_ARG, "bad argument");
    int rc = feed_flush(p);
    if (rc) return rc;
    const std::vector<int64_t> off = ref_offsets(p, nullptr);
    for (auto &cp : p->chunks)
        for (const ReadRec &r : cp->reads) {
            int64_t lo, hi;
            if (!read_extent(*cp, r, off[r.ref], p->ref_len[r.ref], &lo, &hi)) continue;
            const int64_t k = lo >> shift;
            if (k >= 0 && k < n) w[k] += r.kc0 >= 0 ? r.kc1 - r.kc0 : 1;
        }
    return S2C_OK;
}
extern "C" int s2c_parser_pos_weights(s2c_parser *p, int64_t shift, int64_t *w, int64_t n) {
    return s2c_guarded([&] { return s2c_parser_pos_weights_impl(p, shift, w, n); });
}

static int s2c_parser_checks_impl(s2c_parser *p, uint8_t *bad, int64_t n_refs) {
    if (!p || (!bad && n_refs > 0)) return s2c_set_error(S2C_ERR_ARG, "bad argument");
    if (n_refs != (int64_t)p->ref_names.size()) return s2c_set_error(S2C_ERR_ARG, "n_refs differs from the header's");
    int rc = feed_flush(p);
    if (rc) return rc;
    std::vector<uint8_t> bs, bk;
    insertion_checks(p, bs, bk);
    for (int64_t r = 0; r < n_refs; r++) {
        bad[2 * r] = bs[r];
        bad[2 * r + 1] = bk[r];
    }
    return S2C_OK;
}
extern "C" int s2c_parser_checks(s2c_parser *p, uint8_t *bad, int64_t n_refs) {
    return s2c_guarded([&] { return s2c_parser_checks_impl(p, bad, n_refs); });
}

extern "C" int s2c_parser_progress(const s2c_parser *p, int64_t *out) {
    if (!p || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    out[0] = p->in_header ? 0 : 1;
    out[1] = (int64_t)p->ref_names.size();
    out[2] = p->header_lines;
    out[3] = 0;
    for (auto &cp : p->chunks) out[3] += cp->lines_total;
    out[4] = p->err;
    return S2C_OK;
}

extern "C" int s2c_parser_counters(s2c_parser *p, int64_t *out) {
    if (!p || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    int rc = feed_flush(p);
    if (rc) return rc;
    out[0] = p->header_lines;
    out[1] = out[2] = out[3] = 0;
    for (auto &cp : p->chunks) {
        out[1] += cp->lines_total;
        out[2] += cp->reads_mapped;
        out[3] += cp->aligned;
    }
    return S2C_OK;
}

namespace {
struct BlobHdr {
    uint32_t magic, version;
    uint64_t n_reads, n_toks, nq, n_qw, n_ev;
};
constexpr uint32_t BLOB_MAGIC = 0x42433253u;   // "S2CB"
}  // namespace

static int s2c_parser_pack_impl(s2c_parser *p, int64_t g0, int64_t g1, size_t *len) {
    if (!p || !len) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    int rc = feed_flush(p);
    if (rc) return rc;
    const std::vector<int64_t> off = ref_offsets(p, nullptr);
    Chunk d;
    for (auto &cp : p->chunks)
        for (const ReadRec &r : cp->reads) {
            int64_t lo, hi;
            if (read_extent(*cp, r, off[r.ref], p->ref_len[r.ref], &lo, &hi) && lo < g1 && hi >= g0)
                append_read(d, *cp, r, false);
        }
    BlobHdr h{BLOB_MAGIC, (uint32_t)S2C_ABI_VERSION, d.reads.size(), d.toks.size(), d.nq, d.bx.size(), d.ev.size()};
    const size_t bytes = sizeof(h) + h.n_reads * sizeof(ReadRec) + 4 * h.n_toks + 12 * h.n_qw + h.n_ev * sizeof(Event);
    p->blob.resize(bytes);
    uint8_t *o = p->blob.data();
    auto put = [&](const void *src, size_t n) {
        if (n) memcpy(o, src, n);
        o += n;
    };
    put(&h, sizeof(h));
    put(d.reads.data(), h.n_reads * sizeof(ReadRec));
    put(d.toks.data(), 4 * h.n_toks);
    put(d.bq.data(), 8 * h.n_qw);
    put(d.bx.data(), 4 * h.n_qw);
    put(d.ev.data(), h.n_ev * sizeof(Event));
    *len = bytes;
    return S2C_OK;
}
extern "C" int s2c_parser_pack(s2c_parser *p, int64_t g0, int64_t g1, size_t *len) {
    return s2c_guarded([&] { return s2c_parser_pack_impl(p, g0, g1, len); });
}

extern "C" int s2c_parser_blob_copy(const s2c_parser *p, void *dst, size_t cap) {
    if (!p || (!dst && !p->blob.empty())) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (cap < p->blob.size()) return s2c_set_error(S2C_ERR_ARG, "blob larger than the buffer");
    if (!p->blob.empty()) memcpy(dst, p->blob.data(), p->blob.size());
    return S2C_OK;
}

static int s2c_parser_unpack_impl(s2c_parser *p, const void *blob, size_t len) {
    if (!p || (!blob && len)) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    int rc = feed_flush(p);
    if (rc) return rc;
    BlobHdr h;
    if (len < sizeof(h)) return s2c_set_error(S2C_ERR_ARG, "blob too short");
    memcpy(&h, blob, sizeof(h));
    if (h.magic != BLOB_MAGIC || h.version != (uint32_t)S2C_ABI_VERSION)
        return s2c_set_error(S2C_ERR_ARG, "not a blob of this library version");
    const uint64_t lim = (uint64_t)len;
    if (h.n_reads > lim || h.n_toks > lim || h.n_qw > lim || h.n_ev > lim ||
        sizeof(h) + h.n_reads * sizeof(ReadRec) + 4 * h.n_toks + 12 * h.n_qw + h.n_ev * sizeof(Event) != len ||
        (h.nq + 31) / 32 + 1 > h.n_qw + (h.n_qw == 0 ? 1 : 0))
        return s2c_set_error(S2C_ERR_ARG, "blob size does not match its header");
    std::unique_ptr<Chunk> c(new Chunk());
    const uint8_t *in = (const uint8_t *)blob + sizeof(h);
    auto get = [&](auto &vec, size_t n) {
        vec.resize(n);
        const size_t nb = n * sizeof(vec[0]);
        if (nb) memcpy(vec.data(), in, nb);
        in += nb;
    };
    get(c->reads, h.n_reads);
    get(c->toks, h.n_toks);
    get(c->bq, 2 * h.n_qw);
    get(c->bx, h.n_qw);
    get(c->ev, h.n_ev);
    c->nq = h.nq;
    c->nz = h.n_qw;
    const size_t R = p->ref_names.size();
    for (const ReadRec &r : c->reads)   // indices into this chunk and the header's references
        if (r.ref >= R || r.tok + r.ntok > h.n_toks || (uint64_t)r.ev0 + r.nev > h.n_ev ||
            ((r.kc0 >= 0 || r.nev > 0) && r.q + r.slen > 32 * h.n_qw))
            return s2c_set_error(S2C_ERR_ARG, "blob read out of range");
    for (const Event &e : c->ev)
        if (e.ref >= R || e.read >= h.n_reads || e.q + e.len > 32 * h.n_qw)
            return s2c_set_error(S2C_ERR_ARG, "blob event out of range");
    p->chunks.push_back(std::move(c));
    p->chunks.emplace_back(new Chunk());   // the sequential feed appends here
    return S2C_OK;
}
extern "C" int s2c_parser_unpack(s2c_parser *p, const void *blob, size_t len) {
    return s2c_guarded([&] { return s2c_parser_unpack_impl(p, blob, len); });
}
