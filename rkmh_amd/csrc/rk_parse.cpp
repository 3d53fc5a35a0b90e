// rk_parse.cpp -- FASTA/FASTQ(.gz) front end of the hot path (host side): the reader.
//
// Replaces parse_fastas (src/rkmh.cpp:238-292), which drives Heng Li's kseq macros through gzFile.  The record grammar below
// follows kseq_read (src/kseq.hpp:170-208) decision for decision -- records start at the next '>' or '@' wherever it is, the
// name ends at the first whitespace, sequence bytes are every isgraph() byte up to the next '>', '+' or '@', a FASTQ quality
// string is read by COUNT (so '@' inside it is data) and a short one ends the file (-2 ends the caller's loop, rkmh.cpp:251) --
// but it is a block scanner over a large zlib buffer that appends straight into one concatenated batch (bases + offsets) ready
// for hipMemcpyAsync, not a per-record kstring.  Bases are NOT upper-cased here: the device does that while staging
// (rkmh.cpp:252 / :856).
//
// Here: the gzip source, the sequential scanner, and the rk_reader_* / rk_parse_files entry points.  Well-formed plain input goes
// through the block-parallel front end instead (rk_parse_blocks.cpp), which hands anything irregular back to the scanner here.
#include "rk_parse_internal.hpp"

#include <fcntl.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>

using namespace rkparse;

// ---- the gzip source ----

// after a gzread that returned r for `want` bytes: r < 0 is a failure, and so is a short read that zlib explains with an error
// (Z_BUF_ERROR: the compressed stream ends before its end-of-stream mark; Z_DATA_ERROR: damaged)
void GzSource::check_read(int r, size_t want) {
    if (r >= 0 && (size_t)r >= want) return;
    int errnum = 0;
    const char* msg = gzerror(fp, &errnum);
    if (r >= 0 && (errnum == Z_OK || errnum == Z_STREAM_END)) return;
    std::lock_guard<std::mutex> l(io_mu);
    if (io_failed.load()) return;
    io_msg = msg && *msg ? msg : "read error";
    io_failed.store(true);
}

void GzSource::inflate_ahead() {
    size_t want_n = (size_t)256 << 10; // the first chunks are small (a reference panel of a megabyte is one of them), later ones 8 MB
    for (;;) {
        Chunk chunk;
        chunk.p.reset(new unsigned char[want_n]);
        const int r = gzread(fp, chunk.p.get(), (unsigned)want_n);
        check_read(r, want_n); // (before `done` is published under the lock: the consumer sees it)
        chunk.n = r > 0 ? (size_t)r : 0;
        const bool last = chunk.n < want_n;
        if (want_n < ((size_t)8 << 20)) want_n *= 4;
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return q.size() < 6 || stop; });
        if (stop) return;
        if (chunk.n) q.push_back(std::move(chunk));
        if (last) done = true;
        cv.notify_all();
        if (last) return;
    }
}

size_t GzSource::pull(unsigned char* dst, size_t want) {
    if (!threaded) { const int r = gzread(fp, dst, (unsigned)want); check_read(r, want); return r > 0 ? (size_t)r : 0; }
    if (!th.joinable()) th = std::thread(&GzSource::inflate_ahead, this);
    size_t got = 0;
    while (got < want) {
        if (cur_pos == cur.n) {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return !q.empty() || done; });
            if (q.empty()) break; // end of input
            cur = std::move(q.front());
            q.pop_front();
            cur_pos = 0;
            cv.notify_all();
        }
        const size_t n = std::min(want - got, cur.n - cur_pos);
        memcpy(dst + got, cur.p.get() + cur_pos, n);
        cur_pos += n; got += n;
    }
    return got;
}

GzSource::~GzSource() {
    if (th.joinable()) {
        { std::lock_guard<std::mutex> l(m); stop = true; }
        cv.notify_all();
        th.join();
    }
    if (fp) gzclose(fp);
}

// ---- the sequential scanner ----

// from here on the sequential scanner reads the input, beginning with what the block front end has not consumed
void rk_reader::to_sequential() {
    if (par_ok) was_irregular = true;
    par_ok = false;
    seq.pending = true;
    seq.pend_pos = 0;
    if (par.map) { seq.pend_ptr = par.map + par.map_pos; seq.pend_len = par.map_size - par.map_pos; seq.pend_then_eof = true; }
    else { seq.pend_ptr = par.blk.data(); seq.pend_len = par.blk.size(); seq.pend_then_eof = par.blk_eof; }
}

bool rk_reader::fill() {
    SeqState& s = seq;
    if (s.pending) {
        size_t n = s.pend_len - s.pend_pos;
        if (n > s.buf.size()) n = s.buf.size();
        if (n) {
            memcpy(s.buf.data(), s.pend_ptr + s.pend_pos, n);
            s.pend_pos += n;
            s.beg = 0; s.end = n;
            return true;
        }
        s.pending = false;
        std::vector<unsigned char>().swap(par.blk);
        if (s.pend_then_eof) s.eof = true;
    }
    if (s.eof || !src.fp) return false;
    s.beg = 0;
    s.end = src.pull(s.buf.data(), s.buf.size());
    if (s.end < s.buf.size()) s.eof = true;
    return s.end > 0;
}

int rk_reader::next(Batch& b) {
    SeqState& s = seq;
    int c;
    if (s.last_char == 0) {
        for (;;) { // jump to the next header char
            if (s.beg >= s.end && !fill()) return 0;
            const unsigned char* p = s.buf.data() + s.beg;
            const unsigned char* e = s.buf.data() + s.end;
            while (p < e && *p != '>' && *p != '@') ++p;
            s.beg = (size_t)(p - s.buf.data());
            if (p < e) { s.last_char = *p; ++s.beg; break; }
        }
    }
    const Batch::Mark rec0 = b.mark(); // a record that turns out truncated leaves the batch as it was here
    // name = up to the first whitespace
    bool any = false;
    c = -1;
    for (;;) {
        if (s.beg >= s.end && !fill()) { c = -1; break; }
        any = true;
        const unsigned char* p = s.buf.data() + s.beg;
        const unsigned char* e = s.buf.data() + s.end;
        const unsigned char* q = p;
        while (q < e && !T.space[*q]) ++q;
        if (!b.names.append((const char*)p, (size_t)(q - p))) return -3;
        s.beg = (size_t)(q - s.buf.data());
        if (q < e) { c = *q; ++s.beg; break; }
    }
    if (!any) { b.rewind(rec0); return 0; } // EOF right after a header char (ks_getuntil < 0)
    if (c != '\n' && c != -1) {             // comment: rest of the header line
        for (;;) {
            if (s.beg >= s.end && !fill()) break;
            const unsigned char* p = s.buf.data() + s.beg;
            const void* nl = memchr(p, '\n', s.end - s.beg);
            if (nl) { s.beg = (size_t)((const unsigned char*)nl - s.buf.data()) + 1; break; }
            s.beg = s.end;
        }
    }
    // sequence
    c = -1;
    for (;;) {
        if (s.beg >= s.end && !fill()) { c = -1; break; }
        const unsigned char* p = s.buf.data() + s.beg;
        const unsigned char* e = s.buf.data() + s.end;
        if (!b.bases.reserve(b.bases.n + (size_t)(e - p))) return -3;
        uint8_t* w = b.bases.p + b.bases.n;
        unsigned char cls = 0;
        while (p < e) {
            // fast path: copy a line's worth of keepers
            cls = T.seqcls[*p];
            if (cls == 1) { *w++ = *p++; continue; }
            if (cls == 2) break;
            ++p;
        }
        b.bases.n = (size_t)(w - b.bases.p);
        s.beg = (size_t)(p - s.buf.data());
        if (p < e) { c = *p; ++s.beg; break; }
    }
    const size_t slen = b.bases.n - rec0.bases;
    if (c == '>' || c == '@') s.last_char = c;
    bool fastq = (c == '+');
    if (fastq) {
        for (;;) { // rest of the '+' line
            c = getc();
            if (c == -1 || c == '\n') break;
        }
        if (c == -1) { b.rewind(rec0); return -2; }
        const size_t q0 = b.quals.n;
        size_t ql = 0;
        const bool keep_q = b.quals_ok && !skip_quals;
        if (keep_q && !b.quals.reserve(q0 + slen + 1)) return -3;
        for (;;) {
            c = getc();
            if (c == -1 || !(ql < slen)) break;
            if (c >= 33 && c <= 127) { if (keep_q) b.quals.p[q0 + ql] = (char)c; ++ql; }
        }
        s.last_char = 0;
        if (ql != slen) { b.rewind(rec0); return -2; }
        if (keep_q) b.quals.n = q0 + slen;
        else b.quals_ok = false;
    } else {
        b.quals_ok = false;
    }
    if (!b.names.push('\0')) return -3;
    if (!b.offsets.push((uint64_t)b.bases.n) || !b.name_offsets.push((uint64_t)b.names.n)) return -3;
    ++b.nseq;
    return 1;
}

// ---- opening ----

namespace {

int hand_over(Batch& b, rk_seqset* out) {
    if (!b.bases.reserve(b.bases.n + 64)) return perr(RK_ERR_NOMEM, "out of memory");
    memset(b.bases.p + b.bases.n, 0, 64); // dword-read slack for the device staging loads
    out->nseq = b.nseq;
    bool have_q = b.quals_ok && b.nseq > 0;
    out->bases = b.bases.release();
    out->offsets = b.offsets.release();
    out->names = b.names.release();
    out->name_offsets = b.name_offsets.release();
    out->quals = have_q ? b.quals.release() : nullptr;
    return RK_OK;
}

// CPUs this process may actually use: the affinity mask and the cgroup quota (a 256-thread host that grants a container 16 CPUs
// reports 256 from hardware_concurrency)
int granted_cpus() {
    static const int n = [] {
        long v = (long)std::thread::hardware_concurrency();
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) { const long a = CPU_COUNT(&set); if (a > 0 && (v <= 0 || a < v)) v = a; }
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) { // cgroup v2: "<quota|max> <period>"
            char q[32] = {0};
            long period = 0;
            if (fscanf(f, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
                const long c = (atol(q) + period - 1) / period;
                if (c > 0 && (v <= 0 || c < v)) v = c;
            }
            fclose(f);
        } else if (FILE* g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { // cgroup v1
            long quota = -1, period = 0;
            if (fscanf(g, "%ld", &quota) != 1) quota = -1;
            fclose(g);
            if (FILE* h = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(h, "%ld", &period) != 1) period = 0; fclose(h); }
            if (quota > 0 && period > 0) { const long c = (quota + period - 1) / period; if (v <= 0 || c < v) v = c; }
        }
        return (int)(v > 0 ? v : 8);
    }();
    return n;
}

// the environment's knobs, read once per open
struct Knobs {
    int threads;     // RKMH_PARSE_THREADS, at most 64
    size_t block_kb; // RKMH_PARSE_BLOCK_KB (testing knob: small blocks exercise cut/carry/merge); 0 = not set
    int gz_blocks;   // RKMH_GZ_BLOCKS, compressed input: 0 = the sequential scanner on the calling thread, 2 = inflater thread and
                     // block scanner whatever the file's size, anything else = those two for files of 8 MB and more
    Knobs() {
        const char* e = getenv("RKMH_PARSE_THREADS");
        const long v = e ? atol(e) : 0;
        // default: three quarters of the CPUs granted, 4 .. 16 (the classify and formatting threads of a stream run need the
        // rest; measured on 16 CPUs: 16 M reads' main loop 0.38 s with 8 parser threads, 0.32 s with 12, 0.34 s with 16)
        const long dflt = std::min<long>(16, std::max<long>(4, (long)granted_cpus() * 3 / 4));
        threads = (int)(v > 0 ? (v > 64 ? 64 : v) : dflt);
        e = getenv("RKMH_PARSE_BLOCK_KB");
        const long kb = e ? atol(e) : 0;
        block_kb = kb > 0 ? (size_t)kb : 0;
        e = getenv("RKMH_GZ_BLOCKS");
        gz_blocks = e ? atoi(e) : 1;
    }
};

// a regular uncompressed file is mapped: no read() copies at all.  Anything else is left unmapped, for gzFile
int map_plain_file(const char* path, uint64_t offset, BlockState& s) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return perr(RK_ERR_IO, std::string("cannot open ") + path);
    struct stat st;
    unsigned char magic[2] = {0, 0};
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && pread(fd, magic, 2, 0) >= 1 &&
        !(magic[0] == 0x1f && magic[1] == 0x8b)) {
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m != MAP_FAILED) {
            madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
            s.map = (const unsigned char*)m;
            s.map_size = s.map_total = (size_t)st.st_size;
            s.map_start = s.map_pos = (size_t)std::min<uint64_t>(offset, (uint64_t)st.st_size);
        }
    }
    close(fd);
    return RK_OK;
}

// STDIN, pipes and gzip through gzFile.  *blocks: the block front end can read it (plain text, or gzip behind the inflater thread)
int open_gz(const char* path, uint64_t offset, const Knobs& k, GzSource& src, bool* blocks) {
    const bool is_stdin = strcmp(path, "-") == 0;
    src.fp = is_stdin ? gzdopen(0, "r") : gzopen(path, "r");
    if (!src.fp) return perr(RK_ERR_IO, std::string("cannot open ") + path);
    gzbuffer(src.fp, 1 << 20);
    const bool plain = gzdirect(src.fp) != 0;
    // compressed: the inflater gets its own thread, and the block-parallel scanner parses what it delivers
    src.threaded = !plain && k.gz_blocks != 0;
    if (src.threaded && !is_stdin && k.gz_blocks != 2) { // a small file (a reference panel) is done before a thread and a block would be set up
        struct stat zst;
        if (stat(path, &zst) == 0 && zst.st_size < ((off_t)8 << 20)) src.threaded = false;
    }
    *blocks = plain || src.threaded;
    if (offset && gzseek(src.fp, (z_off_t)offset, SEEK_SET) < 0) return perr(RK_ERR_IO, std::string("cannot seek in ") + path);
    return RK_OK;
}

int reader_open_at(const char* path, uint64_t offset, rk_reader** out) {
    if (!path || !out) return perr(RK_ERR_ARG, "bad arguments");
    const Knobs k;
    std::unique_ptr<rk_reader> r(new rk_reader());
    r->seq.buf.resize(4u << 20);
    r->nthreads = k.threads;
    if (k.block_kb) { r->par.max_block = k.block_kb << 10; r->par.min_par = r->par.max_block / 8; }
    if (strcmp(path, "-") != 0) {
        const int rc = map_plain_file(path, offset, r->par);
        if (rc != RK_OK) return rc;
    }
    bool blocks = r->par.map != nullptr;
    if (!r->par.map) {
        const int rc = open_gz(path, offset, k, r->src, &blocks);
        if (rc != RK_OK) return rc;
    }
    r->par_ok = blocks && r->nthreads > 1;
    if (!r->par_ok && r->par.map) r->to_sequential();
    *out = r.release();
    return RK_OK;
}

} // namespace

// ---- the entry points ----

extern "C" {

int rk_reader_open(const char* path, rk_reader** out) { return reader_open_at(path, 0, out); }
// A reader that starts `offset` bytes into a regular uncompressed file, at a record start (the device-side FASTQ front end hands
// a file over to this scanner at the first block it refuses).
int rk_reader_open_at(const char* path, uint64_t offset, rk_reader** out) {
    if (path && strcmp(path, "-") == 0 && offset) return perr(RK_ERR_ARG, "rk_reader_open_at: STDIN has no offsets");
    return reader_open_at(path, offset, out);
}
// The records that START in bytes [lo, hi) of a regular uncompressed FASTQ file: from the first record start at or after lo (the
// four-line rule of find_record_start; lo = 0: the file's first byte) up to the first record start at or after hi.  Ranks of a
// multi-process run each read their own range this way.  The rule is only right for text that IS four lines per record, so the
// caller must check rk_reader_strict() after the last batch: 0 there (or here: RK_ERR_ARG for input that cannot be split at all)
// means "parse the whole file instead".
int rk_reader_open_range(const char* path, uint64_t lo, uint64_t hi, rk_reader** out) {
    if (!path || !out || hi < lo || strcmp(path, "-") == 0) return perr(RK_ERR_ARG, "bad arguments");
    rk_reader* opened = nullptr;
    const int rc = reader_open_at(path, 0, &opened);
    if (rc != RK_OK) return rc;
    std::unique_ptr<rk_reader> r(opened);
    BlockState& s = r->par;
    if (!s.map || !r->par_ok || s.map_size == 0 || s.map[0] != '@') return perr(RK_ERR_ARG, "byte ranges need an uncompressed regular FASTQ file");
    const unsigned char* base = s.map;
    const unsigned char* end = base + s.map_size;
    auto start_at = [&](uint64_t off) -> size_t {
        if (off == 0) return 0;
        if (off >= s.map_size) return s.map_size;
        const unsigned char* p = find_record_start(base, base + off, end, true);
        return p ? (size_t)(p - base) : s.map_size;
    };
    const size_t from = start_at(lo), to = start_at(hi);
    s.map_start = s.map_pos = from;
    s.map_size = to < from ? from : to;
    *out = r.release();
    return RK_OK;
}
// 1 while everything this reader has returned was read by the strict block-parallel front end (text that is four lines per
// record, on which its cuts and rk_reader_open_range's boundaries are exact); 0 once the sequential kseq scanner took over
int rk_reader_strict(const rk_reader* r) { return r && r->par_ok && !r->was_irregular ? 1 : 0; }

void rk_reader_set_options(rk_reader* r, int flags) {
    if (r) r->skip_quals = (flags & RK_READER_NO_QUALS) != 0;
}

void rk_reader_close(rk_reader* r) { delete r; }

// Reads up to max_records records / max_bases bases (0 = unlimited) into *out (malloc'd arrays; release with
// rk_seqset_free).  out->nseq == 0 means end of input.
int rk_reader_next(rk_reader* r, int64_t max_records, uint64_t max_bases, rk_seqset* out) {
    if (!r || !out) return perr(RK_ERR_ARG, "bad arguments");
    memset(out, 0, sizeof *out);
    Batch b;
    if (!b.init()) return perr(RK_ERR_NOMEM, "out of memory");
    while (!r->finished) {
        if (max_records > 0 && b.nseq >= max_records) break;
        if (max_bases > 0 && b.bases.n >= max_bases) break;
        if (r->par_ok && max_records > 0 && max_records < 65536) r->to_sequential(); // small exact batches
        if (r->par_ok) { // block-parallel: limits are soft (a whole block is appended at a time)
            int rb = r->next_block(b, max_records);
            if (rb == -3) return perr(RK_ERR_NOMEM, "out of memory");
            if (rb == 0) { r->finished = true; break; }
            if (rb == 1) break;
            continue; // -1: fell back to the sequential scanner
        }
        int rc = r->next(b);
        if (rc == -3) return perr(RK_ERR_NOMEM, "out of memory");
        if (rc <= 0) { r->finished = true; break; } // EOF, or truncated record: ends the file (rkmh.cpp:251)
    }
    if (r->src.io_failed.load()) return perr(RK_ERR_IO, "read failed (corrupt or truncated input?): " + r->src.read_error());
    return hand_over(b, out);
}

int rk_parse_files(const char* const* paths, int npaths, rk_seqset* out) {
    if (!paths || npaths < 0 || !out) return perr(RK_ERR_ARG, "bad arguments");
    memset(out, 0, sizeof *out);
    Batch b;
    if (!b.init()) return perr(RK_ERR_NOMEM, "out of memory");
    for (int i = 0; i < npaths; ++i) {
        rk_reader* opened = nullptr;
        const int rc = rk_reader_open(paths[i], &opened);
        if (rc != RK_OK) return rc;
        const std::unique_ptr<rk_reader> r(opened);
        for (;;) {
            int k = r->par_ok ? r->next_block(b, 0, /*open_cuts=*/true) : r->next(b);
            if (k == -3) return perr(RK_ERR_NOMEM, "out of memory");
            if (k == -1) continue;
            if (k <= 0) break;
        }
        if (r->src.io_failed.load())
            return perr(RK_ERR_IO, std::string(paths[i]) + ": read failed (corrupt or truncated input?): " + r->src.read_error());
    }
    return hand_over(b, out);
}

} // extern "C"
