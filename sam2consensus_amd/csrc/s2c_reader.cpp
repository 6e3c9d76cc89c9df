// s2c_reader.cpp — the byte source of the file parse (plain, gzip, block-parallel BGZF),
// s2c_parser_feed_file's double-buffered windows over it, and the s2c_reader_* stream.
#include "s2c_host_internal.h"

#include <fcntl.h>
#include <unistd.h>
#include <zlib.h>

namespace {
constexpr size_t WIN = (size_t)64 << 20;   // bytes of a parse window (parse_window's input)

// BGZF (the blocked gzip of samtools / bgzip: members of <= 64 KB, each with a 'BC' extra
// field holding its compressed size) inflated block-parallel: the compressed stream is read
// in 32 MB pieces, the complete blocks of a piece are located by their sizes and inflated on
// all host threads straight into their output offsets (ISIZE from each trailer), CRC-checked.
// A member that is not BGZF-shaped switches the rest of the stream to sequential inflate.
struct Bgzf {
    FILE *f = nullptr;
    std::vector<unsigned char> cb;   // compressed bytes not yet inflated
    std::vector<char> out;           // inflated bytes of the last piece
    size_t opos = 0;
    bool eof = false, seq = false, seq_end = false;
    z_stream z{};
    unsigned nt = 1;
    ~Bgzf() {
        if (seq) inflateEnd(&z);
        if (f) fclose(f);
    }
    static bool block_at(const unsigned char *p, size_t n, size_t *bsize) {   // a BGZF header at p
        if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
        const size_t xlen = p[10] | (p[11] << 8);
        for (size_t k = 12; k + 4 <= 12 + xlen && k + 4 <= n; ) {   // the 'BC' subfield
            const size_t sl = p[k + 2] | (p[k + 3] << 8);
            if (p[k] == 'B' && p[k + 1] == 'C' && sl == 2 && k + 6 <= n) {
                *bsize = (size_t)(p[k + 4] | (p[k + 5] << 8)) + 1;
                return *bsize >= 12 + xlen + 8;
            }
            k += 4 + sl;
        }
        return false;
    }
    bool fill_cb() {   // append up to 32 MB; false at end of file
        const size_t h = cb.size(), want = (size_t)32 << 20;
        cb.resize(h + want);
        const size_t r = fread(cb.data() + h, 1, want, f);
        cb.resize(h + r);
        return r > 0;
    }
    // next piece of output into out; false: no more data (err set on a corrupt stream)
    bool next(bool &err) {
        out.clear();
        opos = 0;
        if (!seq) {
            if (!eof && cb.size() < ((size_t)32 << 20)) eof = !fill_cb();
            std::vector<size_t> off, len, isz;
            size_t k = 0, total = 0;
            while (true) {
                size_t bs;
                if (!block_at(cb.data() + k, cb.size() - k, &bs)) {
                    if (cb.size() - k >= 18 || (eof && cb.size() > k)) seq = true;   // not BGZF from here on
                    break;
                }
                if (k + bs > cb.size()) break;   // partial block: the next piece
                const unsigned char *t = cb.data() + k + bs - 4;
                const size_t is = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
                if (is > 65536) {   // not a BGZF block (≤ 64 KiB inflated): zlib checks the rest sequentially
                    seq = true;
                    break;
                }
                off.push_back(k);
                len.push_back(bs);
                isz.push_back(total);
                total += is;
                k += bs;
            }
            if (!off.empty()) {
                out.resize(total);
                std::atomic<size_t> nextb{0};
                std::atomic<bool> bad{false};
                auto work = [&] {
                    z_stream zz{};
                    if (inflateInit2(&zz, -15) != Z_OK) { bad = true; return; }
                    for (size_t b; (b = nextb++) < off.size();) {
                        const unsigned char *p = cb.data() + off[b];
                        const size_t hl = 12 + (size_t)(p[10] | (p[11] << 8));
                        const size_t dl = len[b] - hl - 8;
                        const size_t ol = (b + 1 < off.size() ? isz[b + 1] : total) - isz[b];
                        inflateReset(&zz);
                        zz.next_in = (Bytef *)(p + hl);
                        zz.avail_in = (uInt)dl;
                        zz.next_out = (Bytef *)out.data() + isz[b];
                        zz.avail_out = (uInt)ol;
                        const int r = inflate(&zz, Z_FINISH);
                        const unsigned char *t = p + len[b] - 8;
                        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
                        if (r != Z_STREAM_END || zz.total_out != ol ||
                            (uint32_t)crc32(0L, (const Bytef *)out.data() + isz[b], (uInt)ol) != crc)
                            bad = true;
                    }
                    inflateEnd(&zz);
                };
                WorkerPool::get(POOL_IO).run((int)std::min<size_t>(nt, off.size()), [&](int) { work(); });
                if (bad) { err = true; return false; }
            }
            cb.erase(cb.begin(), cb.begin() + k);
            if (seq) {
                if (inflateInit2(&z, 31) != Z_OK) { err = true; return false; }
                z.avail_in = 0;
            }
            if (!out.empty()) return true;
            if (!seq) {
                if (eof) {
                    if (!cb.empty()) { err = true; return false; }   // a truncated block
                    return false;
                }
                return next(err);
            }
        }
        // sequential inflate of the rest (gzip members one after the other)
        if (seq_end) return false;
        out.resize((size_t)8 << 20);
        size_t have = 0;
        while (have < out.size()) {
            if (z.avail_in == 0) {
                if (cb.empty()) {
                    if (eof || !fill_cb()) { eof = true; if (cb.empty()) { seq_end = true; break; } }
                }
                z.next_in = cb.data();
                z.avail_in = (uInt)cb.size();
            }
            z.next_out = (Bytef *)out.data() + have;
            z.avail_out = (uInt)(out.size() - have);
            const uInt before = z.avail_in;
            const int r = inflate(&z, Z_NO_FLUSH);
            have = out.size() - z.avail_out;
            const size_t used = before - z.avail_in;
            cb.erase(cb.begin(), cb.begin() + used);
            z.next_in = cb.data();
            z.avail_in = (uInt)cb.size();
            if (r == Z_STREAM_END) {
                if (cb.empty() && eof) { seq_end = true; break; }
                inflateReset(&z);   // the next member
                if (cb.empty() && !fill_cb()) { eof = true; seq_end = true; break; }
                z.next_in = cb.data();
                z.avail_in = (uInt)cb.size();
            } else if (r == Z_BUF_ERROR && cb.empty() && eof) {
                err = true; return false;   // truncated
            } else if (r != Z_OK && r != Z_BUF_ERROR) {
                err = true; return false;
            }
        }
        out.resize(have);
        return have > 0;
    }
    long read(char *dst, size_t n) {
        size_t tot = 0;
        while (tot < n) {
            if (opos == out.size()) {
                bool err = false;
                if (!next(err)) {
                    if (err) return -1;
                    break;
                }
            }
            const size_t k = std::min(n - tot, out.size() - opos);
            memcpy(dst + tot, out.data() + opos, k);
            opos += k;
            tot += k;
        }
        return (long)tot;
    }
};

struct Reader {   // plain, gzip or BGZF (:111-114) byte source
    FILE *f = nullptr;
    gzFile g = nullptr;
    std::unique_ptr<Bgzf> bz;
    int fd = -1;        // plain file: read by positioned reads on the host threads
    uint64_t off = 0;   // its next byte
    ~Reader() {
        if (f) fclose(f);
        if (g) gzclose(g);
        if (fd >= 0) close(fd);
    }
    // n bytes (fewer at end of file) of the plain file in parallel pieces of >= 4 MB: one
    // thread's copy out of the page cache was the file parse's bound past 4 parse threads
    long pread_par(char *dst, size_t n) {
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)std::min(hw ? hw : 1u, 16u), n >> 22}));
        std::vector<size_t> got(nt, 0);
        std::atomic<bool> bad{false};
        auto piece = [&](size_t k) {
            const size_t a = n * k / nt, b = n * (k + 1) / nt;
            size_t h = 0;
            while (a + h < b) {
                const ssize_t r = pread(fd, dst + a + h, b - a - h, (off_t)(off + a + h));
                if (r < 0) { bad = true; break; }
                if (r == 0) break;   // end of file
                h += (size_t)r;
            }
            got[k] = h;
        };
        WorkerPool::get(POOL_IO).run((int)nt, [&](int k) { piece((size_t)k); });
        if (bad) return -1;
        size_t tot = 0;   // (pieces after a short one are empty: the file ends there)
        for (size_t k = 0; k < nt; k++) {
            tot += got[k];
            if (got[k] < n * (k + 1) / nt - n * k / nt) break;
        }
        off += tot;
        return (long)tot;
    }
    long read(char *dst, size_t n) {
        if (bz) return bz->read(dst, n);
        if (fd >= 0) return pread_par(dst, n);
        if (g) {
            size_t tot = 0;
            while (tot < n) {
                const int r = gzread(g, dst + tot, (unsigned)std::min<size_t>(n - tot, 1u << 30));
                if (r < 0) return -1;
                if (r == 0) break;
                tot += (size_t)r;
            }
            return (long)tot;
        }
        return (long)fread(dst, 1, n, f);
    }
};
}  // namespace

// Open path as the reference reads it (:111-114): ".gz" → gzip (BGZF block-parallel), else plain.
static int reader_open(Reader &rd, const char *path) {
    const size_t n = strlen(path);
    if (n >= 3 && strcmp(path + n - 3, ".gz") == 0) {   // :111
        unsigned char h[18];
        size_t bs = 0, hn = 0;
        if (FILE *t = fopen(path, "rb")) {
            hn = fread(h, 1, sizeof(h), t);
            fclose(t);
        }
        if (Bgzf::block_at(h, hn, &bs)) {   // BGZF: block-parallel inflate
            rd.bz.reset(new Bgzf());
            rd.bz->f = fopen(path, "rb");
            if (!rd.bz->f) return s2c_set_error(S2C_ERR_IO, std::string("cannot open ") + path);
            const unsigned hw = std::thread::hardware_concurrency();
            rd.bz->nt = std::max(1u, std::min(hw ? hw : 1u, 16u));
        } else {
            rd.g = gzopen(path, "rb");
            if (!rd.g) return s2c_set_error(S2C_ERR_IO, std::string("cannot open ") + path);
            gzbuffer(rd.g, 1 << 20);
        }
    } else {
        rd.fd = open(path, O_RDONLY);
        if (rd.fd < 0) return s2c_set_error(S2C_ERR_IO, std::string("cannot open ") + path);
    }
    return S2C_OK;
}

static int s2c_parser_feed_file_impl(s2c_parser *p, const char *path) {
    if (!p || !path) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
    if (p->detached) return s2c_set_error(S2C_ERR_ARG, "a detached parser takes no input");
    if (p->err) return s2c_set_error(p->err, p->errmsg);
    Reader rd;
    if (const int rc = reader_open(rd, path)) return rc;
    // A reader thread inflates / reads window k + 1 while the workers parse window k (two
    // buffers).  The reader cuts each window after its last '\n' and carries the partial
    // line into the next one.
    struct Slot {
        std::vector<char> buf;
        size_t len = 0;
        bool full = false, eof = false, err = false;
    };
    Slot slots[2];
    std::mutex m;
    std::condition_variable cv;
    bool stop = false;
    std::vector<char> tail(p->carry.begin(), p->carry.end());   // a partial line from s2c_parser_feed
    p->carry.clear();
    std::thread reader([&] {
        for (int k = 0;; k ^= 1) {
            Slot &sl = slots[k];
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return !sl.full || stop; });
                if (stop) return;
            }
            std::vector<char> &buf = sl.buf;
            if (buf.size() < tail.size() + WIN) buf.resize(tail.size() + WIN + (1 << 20));
            if (!tail.empty()) memcpy(buf.data(), tail.data(), tail.size());
            size_t have = tail.size(), cut = 0;
            bool eof = false, err = false;
            for (;;) {
                if (buf.size() - have < WIN / 2) buf.resize(buf.size() + WIN);   // a line longer than a window
                const long r = rd.read(buf.data() + have, buf.size() - have);
                if (r < 0) { err = true; break; }
                have += (size_t)r;
                if (r == 0) { eof = true; cut = have; break; }
                size_t k2 = have;
                while (k2 > 0 && buf[k2 - 1] != '\n') k2--;
                if (k2) { cut = k2; break; }   // else: no complete line yet, read more
            }
            tail.assign(buf.data() + cut, buf.data() + have);
            {
                std::lock_guard<std::mutex> lk(m);
                sl.len = cut;
                sl.eof = eof;
                sl.err = err;
                sl.full = true;
            }
            cv.notify_all();
            if (eof || err) return;
        }
    });
    int rc = S2C_OK;
    for (int k = 0;; k ^= 1) {
        Slot &sl = slots[k];
        {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return sl.full; });
        }
        if (sl.err) {
            rc = perr(p, S2C_ERR_IO, "gzip read error");
            break;
        }
        if (sl.len) rc = parse_window(p, sl.buf.data(), sl.len);
        const bool eof = sl.eof;
        {
            std::lock_guard<std::mutex> lk(m);
            sl.full = false;
            if (rc) stop = true;
        }
        cv.notify_all();
        if (rc || eof) break;
    }
    {
        std::lock_guard<std::mutex> lk(m);
        stop = true;
    }
    cv.notify_all();
    reader.join();
    return rc;
}
extern "C" int s2c_parser_feed_file(s2c_parser *p, const char *path) {
    return s2c_guarded([&] { return s2c_parser_feed_file_impl(p, path); });
}

// The byte source of s2c_parser_feed_file as a stream (streamed batches, stream.py): the
// same plain / gzip / block-parallel BGZF reader, read in caller-sized pieces.
struct s2c_reader {
    Reader rd;
};
extern "C" int s2c_reader_open(const char *path, s2c_reader **out) {
    return s2c_guarded([&] {
        if (!path || !out) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
        std::unique_ptr<s2c_reader> r(new s2c_reader());
        if (const int rc = reader_open(r->rd, path)) return rc;
        *out = r.release();
        return S2C_OK;
    });
}
extern "C" int s2c_reader_read(s2c_reader *r, void *dst, size_t cap, size_t *n) {
    return s2c_guarded([&] {
        if (!r || !n || (cap && !dst)) return s2c_set_error(S2C_ERR_ARG, "NULL argument");
        size_t tot = 0;
        while (tot < cap) {   // (a full buffer unless the stream ends)
            const long k = r->rd.read((char *)dst + tot, cap - tot);
            if (k < 0) return s2c_set_error(S2C_ERR_IO, "gzip read error");
            if (k == 0) break;
            tot += (size_t)k;
        }
        *n = tot;
        return S2C_OK;
    });
}
extern "C" void s2c_reader_free(s2c_reader *r) { delete r; }
