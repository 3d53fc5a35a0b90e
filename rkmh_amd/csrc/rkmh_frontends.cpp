// rkmh_frontends.cpp -- how stream / filter get reads and references onto the devices: the device FASTQ front end (plain, BGZF and
// gzip files), packed reads, references through the device, the host scanner pipeline, the -M two-pass protocol over all of them,
// and the registry of input files.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <climits>

#include "rkmh_cli.hpp"

// Result rows of the streaming path live in a few recycled page-locked buffers (rk_host_alloc): a fresh 16 MB vector per batch is
// zero-filled and page-faulted by the host each time, and the library would have to page-lock or stage it (8 of the 14 ms a
// 1 M-read batch spent in its classify stage)
struct OutPool {
    std::mutex m;
    std::vector<std::pair<int32_t*, size_t>> free_; // (buffer, rows it holds)
    int32_t* get(size_t rows, size_t* cap) {
        {
            std::lock_guard<std::mutex> l(m);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].second >= rows) { int32_t* p = free_[i].first; *cap = free_[i].second; free_.erase(free_.begin() + (long)i); return p; }
        }
        size_t want = rows + rows / 4 + 4096;
        void* p = nullptr;
        if (rk_host_alloc(want * 16, &p) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); exit(1); }
        *cap = want;
        return (int32_t*)p;
    }
    void put(int32_t* p, size_t cap) { if (p) { std::lock_guard<std::mutex> l(m); free_.emplace_back(p, cap); } }
    ~OutPool() { for (auto& f : free_) rk_host_free(f.first); }
};
struct Classified { rk_seqset reads; int32_t* out4 = nullptr; size_t out_cap = 0; int64_t seq = 0; };

static inline char* put_int(char* w, int v) {
    char tmp[12];
    int n = 0;
    unsigned u = v < 0 ? 0u - (unsigned)v : (unsigned)v;
    do { tmp[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) *w++ = '-';
    while (n) *w++ = tmp[--n];
    return w;
}

// Lines of reads [lo, hi) in the format of rk_format_stream_line (rkmh.cpp:887-892), written straight into one buffer:
// name lengths come from the offset arrays, no per-line strlen / temporary / append.
static void format_range(const rk_seqset& refs, const rk_seqset& reads, const int32_t* out4, const Opts& o,
                         int64_t lo, int64_t hi, std::string& buf) {
    size_t maxref = 0;
    for (int64_t r = 0; r < refs.nseq; ++r) maxref = std::max<size_t>(maxref, (size_t)(refs.name_offsets[r + 1] - refs.name_offsets[r]));
    const size_t need = (size_t)(reads.name_offsets[hi] - reads.name_offsets[lo]) + (size_t)(hi - lo) * (maxref + 64);
    if (buf.size() < need) buf.resize(need);
    char* const w0 = &buf[0];
    char* w = w0;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t* r = out4 + i * 4;
        const size_t ln = (size_t)(refs.name_offsets[r[0] + 1] - refs.name_offsets[r[0]]) - 1; // offsets include the NUL
        const size_t lq = (size_t)(reads.name_offsets[i + 1] - reads.name_offsets[i]) - 1;
        memcpy(w, refs.names + refs.name_offsets[r[0]], ln); w += ln; *w++ = '\t';
        memcpy(w, reads.names + reads.name_offsets[i], lq); w += lq; *w++ = '\t';
        w = put_int(w, r[1]); *w++ = '\t';
        w = put_int(w, o.sketch);
        if (r[3] <= o.min_matches) { memcpy(w, "FAIL:DEPTH", 10); w += 10; }
        *w++ = '\t';
        if (r[1] < o.min_matches) { memcpy(w, "FAIL:MATCHES", 12); w += 12; }
        *w++ = '\t';
        if (!(r[2] > o.min_diff)) { memcpy(w, "FAIL:DIFF", 9); w += 9; }
        *w++ = '\n';
    }
    buf.resize((size_t)(w - w0));
}

// TSV lines in read order (rkmh.cpp:889-897); big batches are formatted by a few threads, written in order
void emit_lines(const rk_seqset& refs, const rk_seqset& reads, const int32_t* out4, const Opts& o, std::string& buf) {
    const int nt = reads.nseq >= 65536 ? 6 : 1;
    if (nt == 1) {
        format_range(refs, reads, out4, o, 0, reads.nseq, buf);
        fwrite(buf.data(), 1, buf.size(), stdout);
        return;
    }
    static std::vector<std::string> parts;
    parts.resize((size_t)nt);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            format_range(refs, reads, out4, o, reads.nseq * t / nt, reads.nseq * (t + 1) / nt, parts[(size_t)t]);
        });
    for (int t = 0; t < nt; ++t) {
        th[(size_t)t].join();
        fwrite(parts[(size_t)t].data(), 1, parts[(size_t)t].size(), stdout);
    }
}

// filter's records of a parsed batch (rkmh.cpp:1292-1300)
void emit_passing(const rk_seqset& reads, const int32_t* rows, const Opts& o, std::string& buf) {
    for (int64_t i = 0; i < reads.nseq; ++i) {
        const int32_t* r = rows + (size_t)i * 4;
        const FilterDecision d = filter_decide(r, o.min_diff);
        // rkmh.cpp:1292-1293.  read_min_lens <= 0 implies shared == 0 (a shared hash is a min), so the conjunction is the same
        // predicate on exact rows -- and it stays right on rows whose min_num was clamped to 0 (bound 0, only with -D >= 0)
        const bool depth_filter = r[3] <= 0 && d.shared <= 0, match_filter = d.shared < o.min_matches;
        if (depth_filter || match_filter || !d.diff_ok) continue;
        buf += '>';
        buf += reads.names + reads.name_offsets[i];
        buf += '\n';
        for (uint64_t j = reads.offsets[i]; j < reads.offsets[i + 1]; ++j) {
            signed char ch = (signed char)reads.bases[j];
            buf += (char)(((int)ch - 91) > 0 ? ch - 32 : ch); // to_upper as parse_fastas applies it (rkmh.cpp:280)
        }
        buf += "\n+\n";
        if (reads.quals) buf.append(reads.quals + reads.offsets[i], (size_t)(reads.offsets[i + 1] - reads.offsets[i]));
        buf += '\n';
        if (buf.size() > (1u << 22)) { fwrite(buf.data(), 1, buf.size(), stdout); buf.clear(); }
    }
    fwrite(buf.data(), 1, buf.size(), stdout);
    buf.clear();
}

// -M: how much of min_num the output needs (rk_set_min_num_bound).  stream / classify print FAIL:DEPTH iff num_mins <= -N
// (rkmh.cpp:938), filter keeps a read iff read_min_lens > 0 (:1292): min(num_mins, bound) answers both, and with it the masked pass
// looks up index keys (and at most `bound` surviving windows per read) in the depth map instead of every window.
// RKMH_EXACT_MIN_NUM=1 keeps the exact form (A/B runs, tests).
int min_num_bound_for(int compare_with) {
    if (env_flag("RKMH_EXACT_MIN_NUM", false)) return -1;
    return compare_with < 0 ? 0 : (compare_with >= 0x3fffffff ? -1 : compare_with + 1);
}
// One k-mer size of 17 .. 20 and no --kmer-cache: the enumeration behind the wide k-mer kernel (0.1 s at k = 17 ... 6.7 s at k = 20)
// is kept beside the first reference file, <ref>.k<k>.s<s>.rkkc, so that it is paid once -- the first run at k = 19 / 20 spends it
// (and classifies with the k-mer kernel itself), every later run with these references, k, sketch size and hashing policy loads
// the file in milliseconds (a file for other references is recognised by its tag and rewritten; with --devices the first
// context writes it while it builds its index, the others -- whose indexes are built afterwards -- load it).  RKMH_KMER_CACHE_AUTO=0 / --no-kmer-cache: off (k = 19 / 20 then stay with the hash-space kernel).  Nothing happens
// when the directory cannot be written.
bool g_no_kmer_cache = false;
static std::string auto_kmer_cache(const Opts& o) {
    if (g_no_kmer_cache || !env_flag("RKMH_KMER_CACHE_AUTO", true)) return "";
    if (o.ks.size() != 1 || o.ks[0] < 17 || o.ks[0] > 20 || o.refs.empty() || !strcmp(o.refs[0], "-")) return "";
    const std::string path = std::string(o.refs[0]) + ".k" + std::to_string(o.ks[0]) + ".s" + std::to_string(o.sketch) + ".rkkc";
    FILE* f = fopen(path.c_str(), "ab"); // (creates it empty when new: an empty file is "no list yet")
    if (!f) return "";
    fclose(f);
    return path;
}
void DeviceGroup::create(const Opts& o) {
        std::vector<int> ids = o.devices.empty() ? std::vector<int>{o.device} : o.devices;
        ctx.assign(ids.size(), nullptr);
        std::vector<std::thread> th;
        std::vector<std::string> err(ids.size());
        for (size_t i = 0; i < ids.size(); ++i)
            th.emplace_back([&, i] { if (rk_ctx_create(ids[i], &g_policy, &ctx[i]) != RK_OK) err[i] = rk_last_error(); });
        for (auto& t : th) t.join();
        for (auto& e : err) if (!e.empty()) { fprintf(stderr, "rkmh: %s\n", e.c_str()); exit(1); }
        if (o.kmer_cache && *o.kmer_cache) for (rk_ctx* cx : ctx) CK(rk_set_kmer_cache(cx, o.kmer_cache));
        else { const std::string ac = auto_kmer_cache(o); if (!ac.empty()) for (rk_ctx* cx : ctx) CK(rk_set_kmer_cache(cx, ac.c_str())); }
}
void DeviceGroup::share_references(const Opts& o) {
        if (ctx.size() < 2) return;
        const int R = rk_num_references(ctx[0]);
        std::vector<uint64_t> sk((size_t)R * (size_t)o.sketch);
        std::vector<int32_t> lens((size_t)R);
        CK(rk_get_reference_sketches(ctx[0], sk.data(), lens.data()));
        std::vector<std::thread> th;
        std::vector<std::string> err(ctx.size());
        for (size_t i = 1; i < ctx.size(); ++i)
            th.emplace_back([&, i] {
                if (rk_set_reference_sketches(ctx[i], sk.data(), lens.data(), R, o.ks.data(), (int)o.ks.size(), o.sketch) != RK_OK) err[i] = rk_last_error();
            });
        for (auto& t : th) t.join();
        for (auto& e : err) if (!e.empty()) { fprintf(stderr, "rkmh: %s\n", e.c_str()); exit(1); }
}
// reads [lo, hi) of a parsed set as a batch of their own (offsets stay absolute: the entry points only use differences and offsets[0])
static inline int64_t share_lo(int64_t n, size_t d, size_t nd) { return n * (int64_t)d / (int64_t)nd; }

// f(d) on every device at once, a thread each; an error of any ends the run
void group_run(DeviceGroup& g, const std::function<int(size_t)>& f) {
    const size_t D = g.size();
    std::vector<std::string> err(D);
    std::vector<std::thread> th;
    for (size_t d = 0; d < D; ++d) th.emplace_back([&, d] { if (f(d) != RK_OK) err[d] = rk_last_error(); });
    for (auto& t : th) t.join();
    for (auto& e : err) if (!e.empty()) { fprintf(stderr, "rkmh: %s\n", e.c_str()); exit(1); }
}
// all-reduce of the per-device depth tables inside one process: a binary tree onto device 0 (log2 D rounds, the adds of one round
// on different devices run concurrently) ...
static void sum_counters_on_group(DeviceGroup& g, std::vector<rk_counter*>& cnt) {
    const size_t D = g.size();
    for (size_t step = 1; step < D; step <<= 1)
        group_run(g, [&](size_t d) { return (d % (2 * step) == 0 && d + step < D) ? rk_counter_add(cnt[d], cnt[d + step]) : RK_OK; });
}
// ... and the full table handed back down the same tree
static void share_counters_on_group(DeviceGroup& g, std::vector<rk_counter*>& cnt) {
    const size_t D = g.size();
    size_t top = 1;
    while (top < D) top <<= 1;
    for (size_t step = top >> 1; step >= 1; step >>= 1)
        group_run(g, [&](size_t d) { return (d % (2 * step) == 0 && d + step < D) ? rk_counter_copy(cnt[d + step], cnt[d]) : RK_OK; });
}
// The depth maps of a -M run, one per device: compact (rk_counter_create_compact: only the slots of index keys, a few hundred KB)
// when the output needs min_num only up to bound 0 and every read's hashes fit the sketch, else the reference's full table.
void make_depth_maps(DeviceGroup& g, uint64_t slots, bool compact, std::vector<rk_counter*>& cnts) {
    for (rk_counter* k : cnts) rk_counter_destroy(k);
    cnts.assign(g.size(), nullptr);
    group_run(g, [&](size_t d) { return compact ? rk_counter_create_compact(g.ctx[d], slots, nullptr, &cnts[d]) : rk_counter_create(g.ctx[d], slots, &cnts[d]); });
}
// RKMH_FULL_DEPTH_MAP=1 keeps the full table (A/B runs, tests)
bool compact_maps_wanted(int bound, const char* read_map) {
    return bound == 0 && !read_map && !env_flag("RKMH_FULL_DEPTH_MAP", false);
}
// every read short enough that bottom-s selection cannot matter (conservative: len - k + 1 windows per size) and for the fused kernel
bool reads_fit_sketch(const rk_seqset& reads, const Opts& o) {
    for (int64_t i = 0; i < reads.nseq; ++i) {
        const int64_t len = (int64_t)(reads.offsets[i + 1] - reads.offsets[i]);
        int64_t nh = 0;
        for (int k : o.ks) nh += len - k + 1 > 0 ? len - k + 1 : 0;
        if (nh > o.sketch || len > 1500) return false;
    }
    return true;
}
static std::atomic<bool> g_need_full{false}; // a count pass met RK_ERR_NEED_FULL: repeat it with full tables

// The -M protocol of every front end (rkmh.cpp:904-948): count() is pass 1 -- every read counted into its device's table; the tables
// are summed onto device 0 and handed back down, so every device masks with the counts of the WHOLE read set, exactly as the
// reference's threads do with their shared counter -- then classify() is pass 2.  A compact map met by a read with more hashes than
// the sketch keeps (g_need_full) is replaced by full tables and pass 1 runs again.  false: count() was refused (a device front end met
// text it does not take) -- the tables are clear again and the caller takes another path.  A count pass that needs full tables
// when it has them already fails the run.  cnts[0] holds the summed table on return.
bool two_pass(DeviceGroup& g, std::vector<rk_counter*>& cnts, uint64_t slots, int min_occ, const std::function<bool()>& count,
              const std::function<void()>& classify, double& t0, const char* tick_count, const char* tick_classify) {
    for (int attempt = 0;; ++attempt) {
        g_need_full.store(false);
        const bool counted = count();
        const bool need_full = g_need_full.exchange(false);
        if (need_full && attempt == 0 && rk_counter_is_compact(cnts[0])) {
            make_depth_maps(g, slots, false, cnts); // a compact depth map cannot serve these reads: the same pass again into full tables
            continue;
        }
        if (counted && !need_full) break;
        if (!counted) {
            group_run(g, [&](size_t d) { return rk_counter_clear(cnts[d]); });
            return false;
        }
        fprintf(stderr, "rkmh: the count pass failed\n");
        fail_exit();
    }
    if (tick_count) tick(tick_count, t0);
    sum_counters_on_group(g, cnts);
    share_counters_on_group(g, cnts);
    group_run(g, [&](size_t d) { return rk_set_depth_filter(g.ctx[d], cnts[d], min_occ); });
    if (tick_count) tick("depth tables summed, mask built", t0);
    classify();
    if (tick_classify) tick(tick_classify, t0);
    return true;
}
// a parsed read set over the devices: device d takes reads [n d / D, n (d+1) / D)
void count_parsed(DeviceGroup& g, const rk_seqset& reads, std::vector<rk_counter*>& cnts) {
    group_run(g, [&](size_t d) {
        const int64_t lo = share_lo(reads.nseq, d, g.size()), hi = share_lo(reads.nseq, d + 1, g.size());
        return rk_count_batch(g.ctx[d], reads.bases, reads.offsets + lo, hi - lo, cnts[d]);
    });
}
void classify_parsed(DeviceGroup& g, const rk_seqset& reads, int32_t* out4) {
    group_run(g, [&](size_t d) {
        const int64_t lo = share_lo(reads.nseq, d, g.size()), hi = share_lo(reads.nseq, d + 1, g.size());
        return rk_classify_batch(g.ctx[d], reads.bases, reads.offsets + lo, hi - lo, out4 + lo * 4);
    });
}

// ------------------------------------------------------------------------------------------------------------------------
// stream / classify with the FASTQ front end ON THE DEVICE (rk_fastq_slot_*, rkmh_amd/csrc/rk_fastq.hip).  The host no longer
// parses the reads (parse_fastas -> kseq_read, rkmh.cpp:238-263): a coordinator cuts the file into byte ranges of whole records,
// N identical workers each read their range straight into a page-locked buffer, have the GPU split it into records, check it,
// pack it and classify it, and format the lines from the record names where they lie in the raw text; one writer puts the
// blocks back in input order.  Text the device refuses (anything but strictly four lines per record) hands the file over to the
// kseq-grammar scanner from that block on, so the output never depends on which front end ran.
// BGZF (bgzip) read files found by raw_eligible: their members are inflated ON THE DEVICE (rk_inflate.hip), thousands per launch,
// by a few workers with device-text slots -- or, RKMH_BGZF_DEVICE=0, by all but two of the CPUs (libdeflate / zlib), job by job
bool bgzf_on_device() {
    static const bool on = env_flag("RKMH_BGZF_DEVICE", true);
    return on;
}
// ordinary gzip read files (one deflate stream): inflated on the device as well (rk_gunzip.hip), stretch after stretch, one worker per
// file; RKMH_GZIP_DEVICE=0 (or RKMH_BGZF_DEVICE=0) leaves them to zlib and the host scanner
static bool gzip_on_device() {
    static const bool on = env_flag("RKMH_GZIP_DEVICE", true);
    return on && bgzf_on_device();
}

// The input files of the run, keyed by path: each is opened as an archive once -- BGZF unless RKMH_BGZF=0, else ordinary gzip when
// those are inflated on the device -- and the handle serves every later look at the path, as a read file or as a reference.
static std::map<std::string, Input> g_inputs;
static Input& input_of(const char* path) {
    auto it = g_inputs.find(path);
    if (it != g_inputs.end()) return it->second;
    Input in;
    if (env_flag("RKMH_BGZF", true) && rk_bgzf_open(path, &in.bz) == RK_OK) in.kind = IN_BGZF;
    else if (gzip_on_device() && rk_gzip_open(path, &in.gz) == RK_OK) in.kind = IN_GZIP;
    else in = Input();
    return g_inputs[path] = in;
}
static const Input* known_input(const char* path) { auto it = g_inputs.find(path); return it == g_inputs.end() ? nullptr : &it->second; }
static const Input* read_archive(const char* path) { const Input* in = known_input(path); return in && in->reads ? in : nullptr; }
bool any_read_archive() { for (auto& kv : g_inputs) if (kv.second.reads) return true; return false; }
static int first_byte(const Input& in) { return in.kind == IN_BGZF ? rk_bgzf_first_byte(in.bz) : rk_gzip_first_byte(in.gz); }
static int64_t text_bytes(const Input& in) { return in.kind == IN_BGZF ? (int64_t)rk_bgzf_text_bytes(in.bz) : (int64_t)rk_gzip_text_bytes_hint(in.gz); }

// a regular, uncompressed file that begins with '@' (FASTQ reads) / '>' (FASTA references) -- or, for reads, a BGZF file whose text
// does (*size is then the length of the text); RKMH_BGZF=0 leaves compressed files to the sequential zlib scanner
bool raw_eligible(const char* path, int64_t* size, char first) {
    if (!path || strcmp(path, "-") == 0) return false;
    if (first == '@' && env_flag("RKMH_BGZF", true)) {
        Input& in = input_of(path);
        if (in.kind != IN_PLAIN) {
            if (first_byte(in) != '@') return false;
            in.reads = true;
            *size = text_bytes(in);
            return true;
        }
    }
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    unsigned char magic[2] = {0, 0};
    const bool ok = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 && pread(fd, magic, 2, 0) >= 1 && magic[0] == (unsigned char)first;
    close(fd);
    if (ok) *size = (int64_t)st.st_size;
    return ok;
}

// Formatted blocks leave in the order of their numbers.  A worker parks its finished block and goes straight on to its next one (it
// only ever waits for memory: at most `window` blocks may be parked ahead of the one due); whoever parks the block that is DUE gives
// the run of consecutive ready blocks their places in the output, in order, and hands them to the writer threads: several of them,
// each with pwrite at the block's final offset, when standard output is a regular file (a file takes ~12 GB/s of buffered writes on the
// test boxes, tools/ubench/file_write.cpp: the output is not what limits the pipeline), one with fwrite otherwise.
struct OrderedOut {
    struct Parked { std::vector<char> buf; size_t len = 0; off_t at = 0; bool keep = false; };
    std::mutex m;
    std::condition_variable cv, cv_task;
    std::map<int64_t, Parked> parked;
    std::deque<Parked> tasks;             // blocks with their place assigned, waiting for a writer
    std::vector<std::vector<char>> spare; // buffers to format the next blocks into
    std::vector<std::thread> writers;
    int64_t next = 0;
    size_t in_flight = 0;                 // tasks queued or being written
    bool assigning = false, closing = false;
    std::atomic<bool> failed{false};      // set by any writer thread
    std::atomic<int64_t> limit{INT64_MAX}; // blocks from this number on are dropped, not written (another front end redoes them)
    bool direct = false;                   // standard output is a regular file not opened for appending
    off_t base = 0, total = 0;
    void lower_limit(int64_t seq) { int64_t cur = limit.load(); while (seq < cur && !limit.compare_exchange_weak(cur, seq)) {} }
    void start(size_t ndev = 1) {
        fflush(stdout);
        struct stat st;
        const int fl = fcntl(1, F_GETFL);
        const bool off_env = !env_flag("RKMH_OUT_DIRECT", true);
        if (!off_env && fstat(1, &st) == 0 && S_ISREG(st.st_mode) && fl >= 0 && !(fl & O_APPEND)) {
            // ("> out 2>&1": both descriptors are ONE open file; a diagnostic written to stderr during the pass would land at the
            // shared offset, inside the region the blocks are pwritten to -- such a run takes the ordered single-writer path)
            struct stat se;
            const bool same_as_stderr = fstat(2, &se) == 0 && se.st_dev == st.st_dev && se.st_ino == st.st_ino;
            const off_t cur = lseek(1, 0, SEEK_CUR);
            if (cur >= 0 && !same_as_stderr) { direct = true; base = cur; }
        }
        long nw = direct ? 3 : 1; // a pipe or a terminal takes the blocks from ONE thread, in order
        if (direct && ndev > 1) nw = std::min<long>(12, 2 + (long)ndev); // several devices produce lines several times as fast
        if (direct) nw = env_long("RKMH_OUT_WRITERS", nw, 1, 16);
        for (long i = 0; i < nw; ++i)
            writers.emplace_back([this] {
                std::unique_lock<std::mutex> l(m);
                for (;;) {
                    cv_task.wait(l, [&] { return !tasks.empty() || closing; });
                    if (tasks.empty()) return;
                    Parked e = std::move(tasks.front());
                    tasks.pop_front();
                    l.unlock();
                    if (e.keep && e.len) {
                        if (direct) {
                            size_t done_ = 0;
                            while (done_ < e.len) {
                                const ssize_t n = pwrite(1, e.buf.data() + done_, e.len - done_, e.at + (off_t)done_);
                                if (n <= 0) { failed = true; break; }
                                done_ += (size_t)n;
                            }
                        } else if (fwrite(e.buf.data(), 1, e.len, stdout) != e.len) failed = true;
                    }
                    l.lock();
                    if (spare.size() < 32) spare.push_back(std::move(e.buf));
                    --in_flight;
                    cv.notify_all();
                }
            });
    }
    std::vector<char> take_buffer() {
        std::lock_guard<std::mutex> l(m);
        if (spare.empty()) return std::vector<char>();
        std::vector<char> b = std::move(spare.back());
        spare.pop_back();
        return b;
    }
    // buf[0 .. len) are the lines of block seq; the buffer becomes the sink's (a spare one comes back from take_buffer)
    void put(int64_t seq, std::vector<char>&& buf, size_t len, int64_t window) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return seq < next + window && in_flight < (size_t)window; });
        Parked& pk = parked[seq];
        pk.buf = std::move(buf); pk.len = len;
        if (assigning) return; // the thread that is handing blocks out will find this one when its turn comes
        assigning = true;
        for (auto it = parked.find(next); it != parked.end(); it = parked.find(next)) {
            Parked e = std::move(it->second);
            parked.erase(it);
            e.keep = next < limit.load();
            e.at = base + total;
            if (e.keep) total += (off_t)e.len;
            ++next;
            ++in_flight;
            tasks.push_back(std::move(e));
        }
        assigning = false;
        cv_task.notify_all();
        cv.notify_all();
    }
    void finish() {
        {
            std::unique_lock<std::mutex> l(m);
            cv.wait(l, [&] { return in_flight == 0; });
            closing = true;
        }
        cv_task.notify_all();
        for (auto& t : writers) t.join();
        if (direct && lseek(1, base + total, SEEK_SET) < 0) failed = true; // later output continues behind the blocks
    }
};

void FormatPool::start(int n) {
    for (int i = (int)th.size(); i < n; ++i)
        th.emplace_back([this] {
            std::unique_lock<std::mutex> l(m);
            for (;;) {
                cv.wait(l, [&] { return !q.empty() || closing; });
                if (q.empty()) return;
                std::function<void()> f = std::move(q.front());
                q.pop_front();
                l.unlock();
                f();
                l.lock();
            }
        });
}
void FormatPool::stop() {
    { std::lock_guard<std::mutex> l(m); closing = true; }
    cv.notify_all();
    for (auto& t : th) t.join();
    th.clear();
    closing = false;
}
struct Latch {
    std::mutex m;
    std::condition_variable cv;
    int left = 0;
    void done() { std::lock_guard<std::mutex> l(m); if (--left == 0) cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return left == 0; }); }
};

const std::vector<const char*>* g_read_paths = nullptr;
bool RawEngine::create(DeviceGroup& g) {
    if (!w.empty()) return true;
    long mb = 16; // measured (tools/e2e_sweep.py, 16 CPUs): 8-16 MB blocks and 8 workers 82 M reads/s, 32 MB and 14 workers 56-73
    if (const long kb = env_long("RKMH_RAW_BLOCK_KB", 0, 4, LONG_MAX)) { block = (uint64_t)kb << 10; mb = 0; }
    if (mb) block = (uint64_t)mb << 20;
    long nw = std::max(2, granted_cpus_main() * 3 / 8); // 6 of 16 CPUs: 4 / 6 / 8 / 10 workers 77 / 97 / 83 / 95 M reads/s to /dev/null, 53-63 to a file
    // one link is saturated by about six workers (the sweep above: one GPU); with several devices in the process every device
    // gets that many as long as the CPUs last -- not measured (one-GPU boxes), the same reasoning per link
    const long cap = g.size() > 1 ? std::min<long>(64, 6 * (long)g.size()) : 12;
    if (nw > cap) nw = cap;
    bool any_bgzf = false;
    for (auto& kv : g_inputs) if (kv.second.reads && kv.second.bz) any_bgzf = true;
    const bool dev_inflate = any_read_archive() && bgzf_on_device();
    // BGZF inflated on the host: a worker inflates its job's members before the upload (~1 GB/s of text per core with libdeflate,
    // a third of that with zlib) -- the CPUs, not the link, set the rate, so all but two of them work
    if (any_bgzf && !dev_inflate) nw = std::max<long>(nw, std::min<long>(32, granted_cpus_main() - 2));
    nw = env_long("RKMH_RAW_WORKERS", nw, 1, 64);
    if ((size_t)nw < g.size()) nw = (long)g.size();
    // BGZF inflated on the device: the decode kernel takes the same time for 64 members as for 16 384 (a lane per member, one
    // wave per 64, two waves per CU: up to 32 768 members per launch in one round), so a job is as large as the file allows --
    // a third of the largest file, at most 1 GiB of text -- and three workers per device keep upload, decode, parsing and
    // formatting of consecutive jobs overlapped.  Their slots hold the text on the device only.
    bool all_bgzf = dev_inflate;
    if (dev_inflate) {
        uint64_t largest = 0;
        for (auto& kv : g_inputs) if (kv.second.reads && kv.second.bz) largest = std::max<uint64_t>(largest, rk_bgzf_text_bytes(kv.second.bz));
        mega = std::min<uint64_t>((uint64_t)1 << 30, std::max<uint64_t>((uint64_t)4 << 20, largest / 3 + ((uint64_t)1 << 20)));
        // (an ordinary gzip file is ONE stream: its stretches follow each other on one worker, so a slot takes a whole file when it can)
        for (auto& kv : g_inputs) if (kv.second.reads && kv.second.gz) mega = std::max<uint64_t>(mega, std::min<uint64_t>((uint64_t)1 << 30, rk_gzip_text_bytes_hint(kv.second.gz) * 5 / 4 + ((uint64_t)8 << 20)));
        if (const long kb = env_long("RKMH_BGZF_JOB_KB", 0, 64, 1536 << 10)) mega = (uint64_t)kb << 10; // (tests: small jobs)
        pieces = (int)std::min<uint64_t>(32, std::max<uint64_t>(1, mega >> 25)); // ~32 MB of text per output piece
        pieces = (int)env_long("RKMH_BGZF_PIECES", pieces, 1, 32);
    }
    const long ndev = dev_inflate ? env_long("RKMH_BGZF_DEVICE_WORKERS", 3, 1, 16) * (long)g.size() : 0;
    // (a run whose read files are ALL BGZF needs no plain-text workers -- their page-locked buffers are the start-up cost of this path)
    if (need_plain_workers || !g_read_paths) all_bgzf = false;
    else for (const char* p : *g_read_paths) if (!read_archive(p)) all_bgzf = false;
    if (all_bgzf) nw = 0;
    w.resize((size_t)(nw + ndev));
    for (size_t i = 0; i < w.size(); ++i) {
        w[i].dev = i % g.size();
        w[i].device_text = i >= (size_t)nw;
        w[i].bytes = (w[i].device_text ? mega : block) + 64; // (+ 64: a last block of exactly `block` bytes may get its missing newline)
    }
    // each worker creates its own slot when it starts (page-locking ~50 MB takes ~10 ms): the first blocks are on their way
    // while the later workers are still setting up.  Only the first slot is made here, to find out whether the front end works at all.
    if (rk_fastq_slot_create2(g.ctx[0], w[0].bytes, w[0].device_text ? RK_SLOT_DEVICE_TEXT : 0, &w[0].slot) != RK_OK) {
        fprintf(stderr, "rkmh: device FASTQ front end unavailable (%s): using the host scanner\n", rk_last_error());
        w.clear();
        return false;
    }
    if (pieces > 1) pool.start((int)std::min<long>(16, std::max<long>(2, granted_cpus_main() - 2)));
    if (dev_inflate)
        for (auto& kv : g_inputs)
            if (kv.second.reads && kv.second.gz && rk_gzip_plan(kv.second.gz, mega) > 0) gz_stretch = std::max<uint64_t>(gz_stretch, rk_gzip_stretch_bytes(kv.second.gz));
    return true;
}
// BGZF files that go to the device: the mapping is page-locked once (14 ms per GB), the DMA engine then reads the compressed
// members out of the page cache itself.  (Refused -- a platform limit -- the uploads go through the runtime's staging.)
void register_bgzf_mappings() {
    static std::mutex rm;
    static std::map<const rk_bgzf*, bool> registered;
    if (!bgzf_on_device() || !env_flag("RKMH_BGZF_REGISTER", true)) return;
    std::lock_guard<std::mutex> l(rm);
    for (auto& kv : g_inputs)
        if (kv.second.reads && kv.second.bz && !registered.count(kv.second.bz))
            registered[kv.second.bz] = rk_host_register_readonly(rk_bgzf_image(kv.second.bz), (size_t)rk_bgzf_file_bytes(kv.second.bz)) == RK_OK;
    static std::map<const rk_gzip*, bool> registered_gz;
    for (auto& kv : g_inputs)
        if (kv.second.reads && kv.second.gz && !registered_gz.count(kv.second.gz))
            registered_gz[kv.second.gz] = rk_host_register_readonly(rk_gzip_image(kv.second.gz), (size_t)rk_gzip_file_bytes(kv.second.gz)) == RK_OK;
}

// records [lo, hi) of a classified block as a result of their own (the spans index the same text)
static rk_fastq_result sub_result(const rk_fastq_result& r, int64_t lo, int64_t hi) {
    rk_fastq_result p = r;
    p.nrec = hi - lo;
    p.out4 = r.out4 + lo * 4;
    p.name_off = r.name_off + lo; p.name_len = r.name_len + lo;
    p.seq_off = r.seq_off + lo; p.seq_len = r.seq_len + lo; p.qual_off = r.qual_off + lo;
    return p;
}

// the lines of one block (rk_fastq_stream_lines: rk_format.cpp), names taken from where the slot says they lie
static size_t format_raw(const rk_line_parts* lp, const rk_fastq_result& r, const uint8_t* text, std::vector<char>& buf) {
    const size_t need = (size_t)rk_fastq_stream_lines_bound(lp, &r);
    if (buf.size() < need) buf.resize(need + need / 8); // (grows a few times, then stays: no per-block allocation or zero-fill)
    const int64_t n = rk_fastq_stream_lines(lp, &r, text, buf.data(), buf.size());
    if (n < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
    return (size_t)n;
}

// filter's decision: classify_and_count_diff_filter (src/equiv.hpp:324-353): scan from max_shared = prev_best = 0, empty sample name
FilterDecision filter_decide(const int32_t* r, int min_diff) {
    FilterDecision d;
    if (r[1] <= 0) { d.ref = -1; d.shared = 0; d.diff_ok = 0 > min_diff; return d; }
    d.ref = r[0]; d.shared = r[1];
    const int diff = r[2] - (r[0] == 0 ? 1 : 0); // the stream scan starts at -1, this one at 0
    d.diff_ok = diff > min_diff;
    return d;
}

// filter's output for one block (rk_fastq_filter_records: rk_format.cpp)
static size_t format_filter_raw(const rk_fastq_result& r, const uint8_t* text, const Opts& o, std::vector<char>& buf) {
    const size_t need = (size_t)rk_fastq_filter_records_bound(&r);
    if (buf.size() < need) buf.resize(need + need / 8);
    const int64_t n = rk_fastq_filter_records(&r, text, o.min_matches, o.min_diff, buf.data(), buf.size());
    if (n < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
    return (size_t)n;
}

// A run of read files through the device front end, as ONE pipeline: the workers go from the last blocks of a file straight to the
// first ones of the next (nothing drains between files), the output keeps the order of the command line.  Returns -1 when every
// file was taken whole; else *fail_file (an index into paths) and the byte offset in that file's text (a record start) from which
// the kseq-grammar scanner must continue -- nothing of that file from there on, and nothing of the files behind it, was printed.
// RAW_STREAM prints stream's lines, RAW_FILTER filter's records; RAW_COUNT prints nothing: it is pass 1 of -M (rkmh.cpp:904-910),
// every worker counts its blocks into its device's table cnts[dev] (summed by the caller), and the first refused block ends the pass.
int64_t stream_files_raw(RawEngine& eng, DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<const char*>& paths,
                                const std::vector<int64_t>& fsizes, RawKind kind, std::vector<rk_counter*>* cnts, size_t* fail_file) {
    rk_line_parts* lp = nullptr;
    if (kind == RAW_STREAM) CK(rk_line_parts_create(refs.names, refs.name_offsets, refs.nseq, o.sketch, o.min_matches, o.min_diff, &lp));
    const bool counting = kind == RAW_COUNT;
    // bz: compressed (BGZF) -- a job is a run of members [lo, hi); mega: ... inflated on the device: large jobs, device-text slots,
    // eng.pieces block numbers each (else by the worker that takes the job)
    struct File { const char* path = nullptr; int fd = -1; int64_t fsize = 0; rk_bgzf* bz = nullptr; rk_gzip* gz = nullptr; bool gz_own = false, gz_locked = false; bool mega = false; const uint8_t* fmap = nullptr; };
    std::vector<File> files(paths.size());
    const bool want_mmap = env_flag("RKMH_RAW_MMAP", false);
    for (size_t i = 0; i < paths.size(); ++i) {
        File& F = files[i];
        F.path = paths[i]; F.fsize = fsizes[i];
        F.fd = open(F.path, O_RDONLY);
        if (F.fd < 0) { fprintf(stderr, "rkmh: cannot open %s\n", F.path); fail_exit(); }
        if (const Input* in = read_archive(F.path)) { F.bz = in->bz; F.gz = in->gz; }
        // (a gzip stream has a position: a file named twice in one run is opened once more for its second turn)
        for (size_t j = 0; F.gz && !F.gz_own && j < i; ++j)
            if (files[j].gz == F.gz) {
                if (rk_gzip_open(F.path, &F.gz) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                F.gz_own = true;
                F.gz_locked = rk_host_register_readonly(rk_gzip_image(F.gz), (size_t)rk_gzip_file_bytes(F.gz)) == RK_OK;
            }
        if (F.gz && eng.mega == 0) { fprintf(stderr, "rkmh: %s: no device-text slots for a gzip stream\n", F.path); fail_exit(); }
        F.mega = (F.bz || F.gz) && eng.mega != 0;
        // RKMH_RAW_MMAP=1: the file is mapped and the mapping page-locked (hipHostRegister): the link reads the page cache itself, the
        // workers copy nothing (tools/ubench/mmap_register.hip)
        if (!F.bz && !F.gz && F.fsize > 0 && want_mmap) {
            void* mp = mmap(nullptr, (size_t)F.fsize, PROT_READ, MAP_SHARED, F.fd, 0);
            if (mp != MAP_FAILED) {
                if (rk_host_register_readonly(mp, (size_t)F.fsize) == RK_OK) F.fmap = (const uint8_t*)mp;
                else munmap(mp, (size_t)F.fsize);
            }
        }
        if (F.mega) register_bgzf_mappings(); // (normally done already, beside the references)
    }
    // file: index into files; at: where the job's first record starts in the (uncompressed) text; ext: its text in the mapped file; nseq: block numbers it owns
    struct Job { size_t file = 0; int64_t seq = 0, lo = 0, hi = 0, at = 0; const uint8_t* ext = nullptr; int64_t nseq = 1; };
    QueueT<Job> jobs_plain, jobs_mega; // (a worker takes the jobs its slot is made for)
    jobs_plain.cap = jobs_mega.cap = eng.w.size();
    bool any_mega = false, any_plain = false, any_gz = false;
    for (const File& F : files) { (F.mega ? any_mega : any_plain) = true; if (F.gz) any_gz = true; }
    OrderedOut out;
    if (!counting) out.start(g.size());
    std::atomic<int64_t> fail_seq{INT64_MAX};
    std::mutex fm;
    std::map<int64_t, std::pair<size_t, int64_t>> fail_at; // block number -> (file, its first byte)
    std::mutex tm;
    std::atomic<int> live_plain{0}, live_mega{0}, needed_mega{INT32_MAX};
    for (auto& x : eng.w) ++(x.device_text ? live_mega : live_plain);
    const int64_t window = (int64_t)eng.w.size() * 4 * (any_mega ? eng.pieces : 1) + 2;
    auto work = [&](size_t wi) {
        RawEngine::Worker& W = eng.w[wi];
        if (!(W.device_text ? any_mega : any_plain)) return; // (no file of this run is for this worker's kind of slot)
        if (W.device_text) { // (... or fewer jobs than workers of it: see needed_mega)
            size_t rank = 0;
            for (size_t j = 0; j < wi; ++j) if (eng.w[j].device_text) ++rank;
            if ((int)rank >= needed_mega.load()) { live_mega.fetch_sub(1); return; }
        }
        QueueT<Job>& jobs = W.device_text ? jobs_mega : jobs_plain;
        std::atomic<int>& live = W.device_text ? live_mega : live_plain;
        const double t_slot = now_s();
        bool slot_ok = true;
        if (!W.slot) {
            std::lock_guard<std::mutex> sl(eng.slot_mu);
            slot_ok = rk_fastq_slot_create2(g.ctx[W.dev], W.bytes, W.device_text ? RK_SLOT_DEVICE_TEXT : 0, &W.slot) == RK_OK;
        }
        // the gunzip work buffers (gigabytes): one worker at a time, and not beside the reference stage (allocations of that size slow
        // every other call of the runtime down while they last: the first slot's, made in create(), cost the references 0.45 s)
        if (slot_ok && W.device_text && eng.gz_stretch && any_gz) {
            std::lock_guard<std::mutex> sl(eng.slot_mu);
            slot_ok = rk_fastq_slot_reserve_gzip(W.slot, eng.gz_stretch) == RK_OK;
        }
        if (!slot_ok) {
            // (memory for another slot ran out: the other workers carry on -- unless this was the last one)
            fprintf(stderr, "rkmh: worker %zu: %s\n", wi, rk_last_error());
            if (live.fetch_sub(1) == 1) { fprintf(stderr, "rkmh: no worker of the device front end could start\n"); fail_exit(); }
            return;
        }
        rk_fastq_slot* const slot = W.slot;
        if (g_timing && W.device_text && now_s() - t_slot > 0.002) fprintf(stderr, "[rkmh timing] worker %zu: device-text slot of %.0f MB made in %.3f s\n", wi, (double)W.bytes / 1e6, now_s() - t_slot);
        if (W.device_text && kind == RAW_FILTER) CK(rk_fastq_slot_set_filter_output(slot, o.min_matches, o.min_diff));
        Job cur;
        double t_rd = 0, t_dv = 0, t_fm = 0;
        int64_t nblk = 0, nrec_ = 0;
        // (block numbers of a job that carry no output of their own)
        auto put_empty = [&](const Job& jb, int64_t from) { if (!counting) for (int64_t e = from; e < jb.nseq; ++e) out.put(jb.seq + e, std::vector<char>(), 0, window); };
        auto declare_failed = [&](const Job& jb) { // the scanner takes the file over from this job's first record
            { std::lock_guard<std::mutex> l(fm); fail_at[jb.seq] = std::make_pair(jb.file, jb.at); }
            if (!counting) out.lower_limit(jb.seq); // (before this block is parked: the sink cannot pass it)
            int64_t curf = fail_seq.load();
            while (jb.seq < curf && !fail_seq.compare_exchange_weak(curf, jb.seq)) {}
        };
        auto finish_block = [&](const Job& jb) {
            const double b = now_s();
            rk_fastq_result res;
            if (rk_fastq_slot_finish(slot, &res) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
            const double c = now_s();
            t_dv += c - b; ++nblk; nrec_ += res.status == 0 ? res.nrec : 0;
            if (res.status != 0) { declare_failed(jb); put_empty(jb, 0); return; }
            const uint8_t* const text = rk_fastq_slot_spans_base(slot);
            auto format_piece = [&](const rk_fastq_result& part, int64_t seq) {
                std::vector<char> buf = out.take_buffer();
                const size_t n = part.nrec == 0 ? 0 : (kind == RAW_FILTER ? format_filter_raw(part, text, o, buf) : format_raw(lp, part, text, buf));
                out.put(seq, std::move(buf), n, window);
            };
            if (jb.nseq == 1) format_piece(res, jb.seq);
            else { // the helpers format the pieces; the slot's arrays stay untouched until all of them are parked
                Latch latch;
                latch.left = (int)jb.nseq;
                for (int64_t e = 0; e < jb.nseq; ++e)
                    eng.pool.run([&, e] {
                        format_piece(sub_result(res, res.nrec * e / jb.nseq, res.nrec * (e + 1) / jb.nseq), jb.seq + e);
                        latch.done();
                    });
                latch.wait();
            }
            t_fm += now_s() - c;
            if (getenv("RKMH_TRACE_JOBS")) fprintf(stderr, "[job] worker %zu parked blocks %lld..%lld (%lld records)\n", wi, (long long)jb.seq, (long long)(jb.seq + jb.nseq - 1), (long long)res.nrec);
        };
        // an ordinary gzip file: ONE job of this worker -- its stretches in order, eng.pieces block numbers each
        auto gzip_file = [&](const Job& fj) {
            const File& F = files[fj.file];
            const int64_t per = eng.pieces, ncalls = fj.nseq / per;
            bool handed_over = false;
            for (int64_t r = 0; r < ncalls; ++r) {
                Job sub; sub.file = fj.file; sub.seq = fj.seq + r * per; sub.nseq = per;
                if (handed_over || sub.seq > fail_seq.load()) { put_empty(sub, 0); continue; }
                const double a = now_s();
                uint64_t nbytes = 0, off = 0;
                const int rc = rk_fastq_slot_load_gzip(slot, F.gz, r, &nbytes, &off);
                if (rc < 0) { fprintf(stderr, "rkmh: %s: %s\n", F.path, rk_last_error()); fail_exit(); }
                sub.at = (int64_t)off;
                if (rc != RK_OK) { // the sequential reader takes the file over from this stretch's first record
                    if (g_timing) fprintf(stderr, "[rkmh timing] %s: the device inflater stops at byte %lld of the text\n", F.path, (long long)off);
                    declare_failed(sub); put_empty(sub, 0); handed_over = true;
                    t_rd += now_s() - a;
                    continue;
                }
                if (nbytes == 0) { put_empty(sub, 0); t_rd += now_s() - a; continue; }
                if (counting) {
                    t_rd += now_s() - a;
                    const double b = now_s();
                    int32_t status = 0; int64_t nrec = 0;
                    const int crc = rk_fastq_slot_count(slot, nbytes, (*cnts)[W.dev], &status, &nrec);
                    if (crc == RK_ERR_NEED_FULL) { g_need_full.store(true); status = 1; }
                    else if (crc != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                    if (status != 0) { declare_failed(sub); handed_over = true; }
                    t_dv += now_s() - b; ++nblk; nrec_ += nrec;
                    continue;
                }
                if (rk_fastq_slot_submit(slot, nbytes) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                t_rd += now_s() - a;
                finish_block(sub);
                if (fail_seq.load() <= sub.seq) handed_over = true; // (text that is not four lines per record)
            }
            // (the file's 4 MB on the device stay until the run ends: hipFree waits for every stream of the device to drain -- seconds, while
            // the other workers' kernels run, tools/ubench/malloc_vs_kernels.hip -- and holds the runtime's lock meanwhile)
        };
        for (;;) {
            if (!jobs.pop(&cur)) break;
            // (a failure is declared at the first block number of the failing worker's own job: never inside another job's run)
            if (cur.seq > fail_seq.load()) { put_empty(cur, 0); continue; } // the scanner will redo this range
            if (files[cur.file].gz) { gzip_file(cur); continue; }
            const File& F = files[cur.file];
            rk_bgzf* const bz = F.bz;
            const char* const path = F.path;
            const int fd = F.fd;
            const int64_t fsize = F.fsize;
            const uint8_t* const fmap = F.fmap;
            const double a = now_s();
            uint64_t nbytes = 0;
            bool refused = false; // (BGZF: text that does not begin with '@', or a job whose records outgrow the slot)
            if (bz) {
                uint64_t off = 0;
                // the members inflated on the device (which may hand a job back: a member it cannot decode, a failed CRC-32 -- the host
                // inflater then reports the damage) or by this thread
                int rc = W.device_text ? rk_fastq_slot_load_bgzf(slot, bz, cur.lo, cur.hi, &nbytes, &off) : 1;
                if (rc < 0) { fprintf(stderr, "rkmh: %s: %s\n", path, rk_last_error()); fail_exit(); }
                if (rc != RK_OK) {
                    uint8_t* text = rk_fastq_slot_text(slot);
                    if (W.device_text) { if (W.host_text.size() < W.bytes) W.host_text.resize(W.bytes); text = W.host_text.data(); }
                    rc = rk_bgzf_fastq_records(bz, cur.lo, cur.hi, text, W.bytes - 1, &nbytes, &off);
                    if (rc == 1 || rc == RK_ERR_LIMIT) { refused = true; nbytes = 0; }
                    else if (rc != RK_OK) { fprintf(stderr, "rkmh: %s: %s\n", path, rk_last_error()); fail_exit(); }
                    if (!refused && cur.hi == rk_bgzf_members(bz) && nbytes && text[nbytes - 1] != '\n') text[nbytes++] = '\n';
                    if (!refused && W.device_text && rk_fastq_slot_set_source(slot, text) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                }
                cur.at = (int64_t)off;
            } else if (fmap && !(cur.hi == fsize && fmap[fsize - 1] != '\n')) { // (a last block without its newline is copied, to get one)
                cur.at = cur.lo;
                cur.ext = fmap + cur.lo;
                nbytes = (uint64_t)(cur.hi - cur.lo);
                if (rk_fastq_slot_set_source(slot, cur.ext) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
            } else {
                uint8_t* text = rk_fastq_slot_text(slot);
                cur.at = cur.lo;
                int64_t have = 0;
                while (have < cur.hi - cur.lo) {
                    const ssize_t n = pread(fd, text + have, (size_t)(cur.hi - cur.lo - have), (off_t)(cur.lo + have));
                    if (n <= 0) { fprintf(stderr, "rkmh: read error on %s\n", path); fail_exit(); } // (the other workers may be waiting for this block)
                    have += n;
                }
                nbytes = (uint64_t)(cur.hi - cur.lo);
                if (cur.hi == fsize && nbytes && text[nbytes - 1] != '\n') text[nbytes++] = '\n'; // a last line without its newline (the slot holds 64 spare bytes)
            }
            if (refused) {
                declare_failed(cur);
                put_empty(cur, 0);
                t_rd += now_s() - a;
                continue;
            }
            if (counting) {
                t_rd += now_s() - a;
                const double b = now_s();
                int32_t status = 0; int64_t nrec = 0;
                const int crc = rk_fastq_slot_count(slot, nbytes, (*cnts)[W.dev], &status, &nrec);
                if (crc == RK_ERR_NEED_FULL) { g_need_full.store(true); status = 1; } // a read with more hashes than the sketch keeps: the pass ends, the caller repeats it with full tables
                else if (crc != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                if (status != 0) declare_failed(cur);
                t_dv += now_s() - b; ++nblk; nrec_ += nrec;
                continue;
            }
            if (rk_fastq_slot_submit(slot, nbytes) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
            t_rd += now_s() - a;
            finish_block(cur);
        }
        std::lock_guard<std::mutex> l(tm);
        eng.t_read += t_rd; eng.t_dev += t_dv; eng.t_fmt += t_fm; eng.blocks += nblk; eng.records += nrec_;
    };
    // how many jobs the device-text workers will share (an ordinary gzip file is one job, a BGZF file a few): a worker without a job
    // to expect does not start -- its slot and work buffers are gigabytes of allocations that slow the others down while they are made
    // (one gzip file: 0.36 s as a command with one such worker setting up, 0.6 - 0.77 s with four or five)
    size_t mega_jobs = 0;
    for (const File& F : files) {
        if (F.gz) ++mega_jobs;
        else if (F.bz && F.mega) {
            const uint64_t target = eng.mega > ((uint64_t)1 << 20) ? eng.mega - ((uint64_t)1 << 18) : eng.mega * 3 / 4;
            std::vector<int64_t> first((size_t)rk_bgzf_members(F.bz) + 4);
            const int64_t nj = rk_bgzf_plan_members(F.bz, target, 16381, first.data(), (int64_t)first.size());
            mega_jobs += nj > 0 ? (size_t)nj : 1;
        }
    }
    needed_mega.store((int)std::min<size_t>(mega_jobs, (size_t)INT32_MAX));
    std::vector<std::thread> workers;
    for (size_t i = 0; i < eng.w.size(); ++i) workers.emplace_back(work, i);
    // coordinator: ranges of whole records, file after file.  The end of a range is the last record start (four-line rule,
    // rk_fastq_cut) inside a window in front of its nominal end; a range that is cut wrongly (possible only in text that is not
    // four lines per record) is refused by the device and the scanner takes over from its first byte.
    int64_t seq = 0;
    for (size_t fi = 0; fi < files.size() && fail_seq.load() == INT64_MAX; ++fi) {
        const File& F = files[fi];
        if (F.gz) { // one job: the file's stretches, in order, on one worker
            const int64_t ncalls = rk_gzip_plan(F.gz, eng.mega);
            if (ncalls < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
            Job jb; jb.file = fi; jb.seq = seq; jb.nseq = ncalls * eng.pieces;
            seq += jb.nseq;
            jobs_mega.push(jb);
            continue;
        }
        if (F.bz) { // jobs = runs of members holding about a block of text (the records are cut after inflating)
            const uint64_t per_job = F.mega ? eng.mega : eng.block;
            const uint64_t target = per_job > ((uint64_t)1 << 20) ? per_job - ((uint64_t)1 << 18) : per_job * 3 / 4;
            std::vector<int64_t> first((size_t)rk_bgzf_members(F.bz) + 4);
            // (device jobs: at most 16 381 members + the three around them = 256 waves of 64 members: two launches fill the chip exactly)
            const int64_t nj = rk_bgzf_plan_members(F.bz, target, F.mega ? 16381 : INT64_MAX, first.data(), (int64_t)first.size());
            if (nj < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
            const int64_t per = F.mega ? eng.pieces : 1;
            for (int64_t j = 0; j < nj && fail_seq.load() == INT64_MAX; ++j) {
                Job jb; jb.file = fi; jb.seq = seq; jb.nseq = per; jb.lo = first[(size_t)j]; jb.hi = first[(size_t)j + 1];
                seq += per;
                (F.mega ? jobs_mega : jobs_plain).push(jb);
            }
            continue;
        }
        std::vector<uint8_t> win;
        int64_t pos = 0;
        const int64_t B = (int64_t)eng.block, fsize = F.fsize;
        while (pos < fsize && fail_seq.load() == INT64_MAX) {
            int64_t hi = fsize;
            if (fsize - pos > B) {
                int64_t wlen = 1 << 16;
                hi = -1;
                while (hi < 0) {
                    if (wlen > B - 1) wlen = B - 1;
                    const int64_t wlo = pos + B - wlen; // the window ends at the nominal end of the range
                    win.resize((size_t)wlen);
                    int64_t got = 0;
                    while (got < wlen) {
                        const ssize_t n = pread(F.fd, win.data() + got, (size_t)(wlen - got), (off_t)(wlo + got));
                        if (n <= 0) break;
                        got += n;
                    }
                    const int64_t cut = got == wlen ? rk_fastq_cut(win.data(), (uint64_t)wlen) : -1;
                    if (cut > 0) hi = wlo + cut;
                    else if (wlen >= B - 1) break; // no record start anywhere in the range: not for the device
                    else wlen *= 8;
                }
                if (hi < 0) { // hand the file over from here
                    std::lock_guard<std::mutex> l(fm);
                    fail_at[seq] = std::make_pair(fi, pos);
                    if (!counting) out.lower_limit(seq);
                    int64_t cur = fail_seq.load();
                    while (seq < cur && !fail_seq.compare_exchange_weak(cur, seq)) {}
                    break;
                }
            }
            Job j; j.file = fi; j.seq = seq++; j.lo = pos; j.hi = hi;
            jobs_plain.push(j);
            pos = hi;
        }
    }
    jobs_plain.finish();
    jobs_mega.finish();
    for (auto& t : workers) t.join();
    if (!counting) out.finish();
    rk_line_parts_destroy(lp);
    for (File& F : files) {
        if (F.fmap) { rk_host_unregister(F.fmap); munmap((void*)F.fmap, (size_t)F.fsize); }
        if (F.gz_own) { if (F.gz_locked) rk_host_unregister(rk_gzip_image(F.gz)); rk_gzip_close(F.gz); }
        close(F.fd);
    }
    if (out.failed) { fprintf(stderr, "rkmh: write error on standard output\n"); fail_exit(); }
    const int64_t fs = fail_seq.load();
    if (fs == INT64_MAX) return -1;
    if (fail_file) *fail_file = fail_at[fs].first;
    return fail_at[fs].second;
}


// -M with the device front end (rkmh.cpp:904-948 without holding the reads in RAM): pass 1 counts every file's blocks, the depth
// tables are summed over the devices and become every context's mask, pass 2 reads the files again and prints.  false: some block
// is not four lines per record -- nothing was printed, the tables are clear again and the caller takes the parse-everything path.
bool two_pass_raw(RawEngine& eng, DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<int64_t>& sizes,
                  std::vector<rk_counter*>& cnts, RawKind kind, double& t0, uint64_t slots) {
    size_t ff = 0;
    auto count = [&] {
        if (stream_files_raw(eng, g, refs, o, o.reads, sizes, RAW_COUNT, &cnts, &ff) < 0) return true;
        if (g_timing && g_need_full.load() && rk_counter_is_compact(cnts[0]))
            fprintf(stderr, "[rkmh timing] %s: reads with more hashes than the sketch keeps: pass 1 restarts with full depth tables\n", o.reads[ff]);
        return false;
    };
    auto classify = [&] {
        if (stream_files_raw(eng, g, refs, o, o.reads, sizes, kind, nullptr, &ff) >= 0) {
            fprintf(stderr, "rkmh: %s changed between the two passes\n", o.reads[ff]);
            fail_exit();
        }
        fflush(stdout);
    };
    if (two_pass(g, cnts, slots, o.min_occ, count, classify, t0, "pass 1 (device front end + count)", "pass 2 (device front end + classify)")) return true;
    if (g_timing) fprintf(stderr, "[rkmh timing] %s: not four lines per record: the host scanner reads the run\n", o.reads[ff]);
    return false;
}

struct PackedFile {
    const char* path = nullptr;
    const uint8_t* map = nullptr;
    size_t size = 0;
    const rk_packed_header* hdr = nullptr;
    const rk_packed_block* dir = nullptr;
};
// maps and checks a packed file (every section inside the file, counts consistent); exits with a message otherwise
static PackedFile packed_open(const char* path) {
    PackedFile pf;
    pf.path = path;
    const int fd = open(path, O_RDONLY);
    struct stat st;
    if (fd < 0 || fstat(fd, &st) != 0 || st.st_size < (off_t)sizeof(rk_packed_header)) { fprintf(stderr, "rkmh: cannot read packed reads from %s\n", path); exit(1); }
    void* mp = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_SHARED, fd, 0);
    close(fd);
    if (mp == MAP_FAILED) { fprintf(stderr, "rkmh: cannot map %s\n", path); exit(1); }
    pf.map = (const uint8_t*)mp; pf.size = (size_t)st.st_size;
    pf.hdr = reinterpret_cast<const rk_packed_header*>(pf.map);
    auto bad = [&](const char* why) { fprintf(stderr, "rkmh: %s is not a packed read file of this build (%s): write it with `rkmh pack`\n", path, why); exit(1); };
    if (memcmp(pf.hdr->magic, RK_PACKED_MAGIC, 8) != 0 || pf.hdr->version != 1) bad("magic / version");
    const uint64_t nb = pf.hdr->nblocks, doff = pf.hdr->directory_off;
    if ((doff & 15) || doff > pf.size || nb > (pf.size - doff) / sizeof(rk_packed_block)) bad("directory");
    pf.dir = reinterpret_cast<const rk_packed_block*>(pf.map + doff);
    uint64_t nreads = 0;
    for (uint64_t i = 0; i < nb; ++i) {
        const rk_packed_block& b = pf.dir[i];
        auto inside = [&](uint64_t off, uint64_t n) { return (off & 15) == 0 && off <= doff && n <= doff - off; };
        if (!inside(b.offsets_off, ((uint64_t)b.nrec + 1) * 4) || !inside(b.bases_off, (b.nbases + 3) / 4 + 16) || !inside(b.exc_off, (uint64_t)b.nexc * 8) ||
            !inside(b.name_offsets_off, ((uint64_t)b.nrec + 1) * 4) || !inside(b.names_off, b.name_bytes + 32) || (b.quals_off && !inside(b.quals_off, b.nbases)))
            bad("a block's sections");
        const uint32_t* so = reinterpret_cast<const uint32_t*>(pf.map + b.offsets_off);
        const uint32_t* no = reinterpret_cast<const uint32_t*>(pf.map + b.name_offsets_off);
        if (so[0] != 0 || so[b.nrec] != b.nbases || no[0] != 0 || no[b.nrec] != b.name_bytes) bad("a block's offsets");
        nreads += b.nrec;
    }
    if (nreads != pf.hdr->nreads) bad("read count");
    return pf;
}

// The blocks of the packed files through the devices: per device a few workers, each with a packed slot (rk_packed_slot_*): upload the
// block's offsets, 2-bit bases and exceptions from the mapping, classify (or count: pass 1 of -M), format the lines from the names in
// the mapping -- large blocks in pieces, by the helper threads -- and park them in input order.
static void stream_packed(DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<PackedFile>& files, RawKind kind, std::vector<rk_counter*>* cnts) {
    const bool counting = kind == RAW_COUNT;
    rk_line_parts* lp = nullptr;
    if (kind == RAW_STREAM) CK(rk_line_parts_create(refs.names, refs.name_offsets, refs.nseq, o.sketch, o.min_matches, o.min_diff, &lp));
    struct Job { size_t file; uint64_t block; int64_t seq, nseq; };
    std::vector<Job> jobs;
    uint64_t max_reads = 1, max_bases = 16;
    const int64_t PIECE = 1 << 18; // reads per output piece
    int64_t seq = 0;
    for (size_t f = 0; f < files.size(); ++f)
        for (uint64_t b = 0; b < files[f].hdr->nblocks; ++b) {
            const rk_packed_block& blk = files[f].dir[b];
            max_reads = std::max<uint64_t>(max_reads, blk.nrec); max_bases = std::max<uint64_t>(max_bases, blk.nbases);
            const int64_t pieces = std::max<int64_t>(1, ((int64_t)blk.nrec + PIECE - 1) / PIECE);
            jobs.push_back(Job{f, b, seq, pieces});
            seq += pieces;
        }
    static std::map<const uint8_t*, bool> registered; // (a mapping is page-locked once; both passes of -M use it)
    for (const PackedFile& pf : files)
        if (!registered.count(pf.map) && env_flag("RKMH_PACKED_REGISTER", true)) {
            const double a = now_s();
            registered[pf.map] = rk_host_register_readonly(pf.map, pf.size) == RK_OK;
            if (g_timing) fprintf(stderr, "[rkmh timing] %s: mapping of %.0f MB %s in %.3f s\n", pf.path, (double)pf.size / 1e6, registered[pf.map] ? "page-locked" : "NOT page-locked (uploads are staged by the runtime)", now_s() - a);
        }
    const size_t nw = (size_t)env_long("RKMH_PACKED_WORKERS", 3, 1, 16) * g.size();
    OrderedOut out;
    if (!counting) out.start(g.size());
    FormatPool pool;
    if (!counting) pool.start((int)std::min<long>(16, std::max<long>(2, granted_cpus_main() - 2)));
    int64_t most_pieces = 1;
    for (const Job& jb : jobs) most_pieces = std::max(most_pieces, jb.nseq);
    // every worker has two slots: while the pool formats the lines of one block (from the rows in that slot's page-locked buffer) the
    // worker's next block is on the device in the other.  At most 2 nw consecutive blocks are open at a time, so a piece never waits
    // in put() for a piece that is queued behind it
    const int64_t window = (int64_t)nw * 2 * most_pieces + 2;
    std::atomic<size_t> next{0};
    std::mutex tm;
    double t_dev = 0, t_fmt = 0;
    auto work = [&](size_t wi) {
        rk_packed_slot* slot[2] = {nullptr, nullptr};
        rk_fastq_result res[2];
        Latch latch[2];
        const size_t dev = wi % g.size();
        const int nslot = counting ? 1 : 2;
        for (int i = 0; i < nslot; ++i)
            if (rk_packed_slot_create(g.ctx[dev], max_reads, max_bases, &slot[i]) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
        double dv = 0, fm = 0;
        int cur = 0;
        for (size_t j = next.fetch_add(1); j < jobs.size(); j = next.fetch_add(1)) {
            const Job& jb = jobs[j];
            const PackedFile& pf = files[jb.file];
            const rk_packed_block& blk = pf.dir[jb.block];
            const double a = now_s();
            if (counting) {
                const int rc = rk_packed_slot_count(slot[0], &blk, pf.map, (*cnts)[dev]);
                if (rc == RK_ERR_NEED_FULL) g_need_full.store(true);
                else if (rc != RK_OK) { fprintf(stderr, "rkmh: %s: %s\n", pf.path, rk_last_error()); fail_exit(); }
                dv += now_s() - a;
                continue;
            }
            latch[cur].wait(); // the lines of the block this slot held before are with the sink
            const double a2 = now_s();
            if (rk_packed_slot_classify(slot[cur], &blk, pf.map, &res[cur]) != RK_OK) { fprintf(stderr, "rkmh: %s: %s\n", pf.path, rk_last_error()); fail_exit(); }
            const double b = now_s();
            const rk_fastq_result* const rs = &res[cur];
            Latch* const lt = &latch[cur];
            { std::lock_guard<std::mutex> l(lt->m); lt->left = (int)jb.nseq; }
            for (int64_t e = 0; e < jb.nseq; ++e)
                pool.run([&out, &o, &pf, &blk, &jb, rs, lt, lp, kind, window, e] {
                    const int64_t lo = rs->nrec * e / jb.nseq, hi = rs->nrec * (e + 1) / jb.nseq;
                    std::vector<char> buf = out.take_buffer();
                    size_t n = 0;
                    if (hi > lo) {
                        const rk_fastq_result part = sub_result(*rs, lo, hi);
                        if (kind == RAW_FILTER) {
                            const size_t need = (size_t)rk_packed_filter_records_bound(&part);
                            if (buf.size() < need) buf.resize(need + need / 8);
                            const int64_t w = rk_packed_filter_records(&part, &blk, pf.map, o.min_matches, o.min_diff, buf.data(), buf.size());
                            if (w < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
                            n = (size_t)w;
                        } else n = format_raw(lp, part, pf.map + blk.names_off, buf);
                    }
                    out.put(jb.seq + e, std::move(buf), n, window);
                    lt->done();
                });
            dv += b - a2; fm += a2 - a;
            cur ^= 1;
        }
        for (int i = 0; i < nslot; ++i) { latch[i].wait(); rk_packed_slot_destroy(slot[i]); }
        std::lock_guard<std::mutex> l(tm);
        t_dev += dv; t_fmt += fm;
    };
    std::vector<std::thread> th;
    for (size_t i = 0; i < nw; ++i) th.emplace_back(work, i);
    for (auto& t : th) t.join();
    pool.stop();
    if (!counting) out.finish();
    rk_line_parts_destroy(lp);
    if (out.failed) { fprintf(stderr, "rkmh: write error on standard output\n"); fail_exit(); }
    if (g_timing) fprintf(stderr, "[rkmh timing] packed reads: %zu blocks; upload + classify %.3f s, waiting for the lines of an earlier block %.3f s (summed over %zu workers)\n", jobs.size(), t_dev, t_fmt, nw);
}

// stream / filter over packed files, with or without -M (two passes: count, sum over the devices, mask, classify)
void run_packed(DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<const char*>& paths, RawKind kind, uint64_t slots, int bound, double& t0) {
    std::vector<PackedFile> files;
    for (const char* p : paths) files.push_back(packed_open(p));
    if (kind == RAW_FILTER && !files.empty() && !(files[0].hdr->flags & RK_PACKED_QUALS) && g_timing) fprintf(stderr, "[rkmh timing] %s keeps no qualities: filter prints empty quality lines\n", files[0].path);
    if (o.read_depth) {
        std::vector<rk_counter*> cnts;
        make_depth_maps(g, slots, compact_maps_wanted(bound, nullptr), cnts);
        two_pass(g, cnts, slots, o.min_occ, [&] { stream_packed(g, refs, o, files, RAW_COUNT, &cnts); return true; },
                 [&] { stream_packed(g, refs, o, files, kind, nullptr); }, t0, "pass 1 (packed reads, count)", "pass 2 (packed reads, classify)");
        return;
    }
    stream_packed(g, refs, o, files, kind, nullptr);
    tick("packed reads: classify + format", t0);
}

// The -r files through the device (rk_fasta_load_*, rkmh_amd/csrc/rk_fasta.hip) instead of parse_fastas (rkmh.cpp:238-263): the
// workers of the read pipeline pread the raw text into their page-locked buffers and upload it, the GPU strips header lines and
// line ends, and the references are sketched from the packed bases where they lie -- the host never sees a base.  Worth its set-up
// for genome-sized references (BASELINE config 4: 3.1 GB of FASTA, where the host parser was the longest stage of the run);
// RKMH_RAW_REFS=1 forces it for any size, =0 turns it off.  false: not taken (small, compressed, not regular FASTA, no memory):
// the caller parses on the host.  On success refs carries the names only (all that stream / filter print).
// will refs_through_device take the -r files?  (sizes, total: the files' lengths and their sum with a newline after each)
bool refs_for_device(const Opts& o, std::vector<int64_t>* sizes, uint64_t* total_out) {
    const long env = env_long("RKMH_RAW_REFS", -1, 0, 1); // 0: never, 1: any size, else: genome-sized references only
    if (env == 0) return false;
    const bool forced = env == 1;
    std::vector<int64_t> size(o.refs.size(), 0);
    uint64_t total = 0;
    for (size_t i = 0; i < o.refs.size(); ++i) {
        if (!raw_eligible(o.refs[i], &size[i], '>')) {
            // an ordinary gzip file (genome.fa.gz as it is distributed): inflated on the device (rk_fasta_load_put_gzip); its text's
            // length is the trailer's word for it (a file of 4 GB of text or more ends up with the host parser)
            // ... and a bgzip'd genome: independent members (rk_fasta_load_put_bgzf)
            const Input* in = bgzf_on_device() ? &input_of(o.refs[i]) : nullptr;
            if (!in || in->kind == IN_PLAIN || first_byte(*in) != '>') return false;
            size[i] = text_bytes(*in);
        }
        total += (uint64_t)size[i] + 1; // a '\n' after every file
    }
    if (o.refs.empty() || (!forced && total < ((uint64_t)64 << 20))) return false;
    if (sizes) *sizes = size;
    if (total_out) *total_out = total;
    return true;
}
bool refs_through_device(RawEngine& eng, DeviceGroup& g, const Opts& o, int max_samples, uint64_t counter_slots, rk_seqset& refs,
                                DeviceRefs& keep) {
    std::vector<int64_t> size;
    uint64_t total = 0;
    if (!refs_for_device(o, &size, &total)) return false;
    eng.need_plain_workers = true;
    if (!eng.create(g)) return false;
    rk_fasta_load* load = nullptr;
    if (rk_fasta_load_create(g.ctx[0], total, &load) != RK_OK) {
        fprintf(stderr, "rkmh: references through the device: %s; parsing on the host\n", rk_last_error());
        return false;
    }
    struct Job { size_t file; int64_t lo, hi; uint64_t at; bool last; };
    std::vector<Job> jobs;
    struct GzRef { rk_gzip* gz; uint64_t at, size; };
    std::vector<GzRef> gz_refs;
    struct BzRef { rk_bgzf* bz; uint64_t at, size; };
    std::vector<BzRef> bz_refs;
    std::vector<int> fds(o.refs.size(), -1);
    {
        uint64_t at = 0;
        const int64_t B = (int64_t)eng.block;
        for (size_t i = 0; i < o.refs.size(); ++i) {
            const Input* in = known_input(o.refs[i]); // (refs_for_device found it to be BGZF or gzip -- or plain text)
            if (in && in->kind != IN_PLAIN) {
                if (in->bz) bz_refs.push_back(BzRef{in->bz, at, (uint64_t)size[i]});
                else gz_refs.push_back(GzRef{in->gz, at, (uint64_t)size[i]});
                at += (uint64_t)size[i] + 1;
                continue;
            }
            fds[i] = open(o.refs[i], O_RDONLY);
            if (fds[i] < 0) { fprintf(stderr, "rkmh: cannot open %s\n", o.refs[i]); fail_exit(); }
            for (int64_t lo = 0; lo < size[i]; lo += B) {
                const int64_t hi = std::min(size[i], lo + B);
                jobs.push_back(Job{i, lo, hi, at + (uint64_t)lo, hi == size[i]});
            }
            at += (uint64_t)size[i] + 1;
        }
    }
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&](size_t wi) {
        if (eng.w[wi].dev != 0 || eng.w[wi].device_text) return; // the text goes to the device that sketches, through a page-locked text buffer
        if (!eng.w[wi].slot && rk_fastq_slot_create(g.ctx[0], eng.w[wi].bytes, &eng.w[wi].slot) != RK_OK) return;
        rk_fastq_slot* slot = eng.w[wi].slot;
        uint8_t* text = rk_fastq_slot_text(slot);
        for (size_t j = next.fetch_add(1); j < jobs.size() && !failed.load(); j = next.fetch_add(1)) {
            const Job& jb = jobs[j];
            int64_t have = 0;
            while (have < jb.hi - jb.lo) {
                const ssize_t n = pread(fds[jb.file], text + have, (size_t)(jb.hi - jb.lo - have), (off_t)(jb.lo + have));
                if (n <= 0) { fprintf(stderr, "rkmh: read error on %s\n", o.refs[jb.file]); fail_exit(); }
                have += n;
            }
            uint64_t nbytes = (uint64_t)have;
            if (jb.last) text[nbytes++] = '\n'; // (the slot holds 64 spare bytes)
            if (rk_fasta_load_put(load, slot, jb.at, nbytes) != RK_OK) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); failed = true; }
        }
    };
    double tr = now_s();
    std::vector<std::thread> th;
    for (size_t i = 0; i < eng.w.size(); ++i) th.emplace_back(work, i);
    for (const GzRef& gr : gz_refs) { // (this thread: a gzip stream is inflated stretch after stretch)
        uint64_t nb = 0;
        const int rc = failed.load() ? 1 : rk_fasta_load_put_gzip(load, gr.gz, gr.at, &nb);
        if (rc < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); fail_exit(); }
        if (rc != RK_OK || nb != gr.size || rk_fasta_load_put_newline(load, gr.at + nb) != RK_OK) failed = true; // (the host parser reads the references)
    }
    if (!bz_refs.empty() && !failed.load()) { // bgzip'd references: runs of members inflated in the buffers of one device-text slot made for the purpose
        const uint64_t job_text = (uint64_t)512 << 20;
        rk_fastq_slot* via = nullptr;
        if (rk_fastq_slot_create2(g.ctx[0], job_text + ((uint64_t)1 << 20), RK_SLOT_DEVICE_TEXT, &via) != RK_OK) failed = true;
        for (const BzRef& br : bz_refs) {
            if (failed.load()) break;
            std::vector<int64_t> first((size_t)rk_bgzf_members(br.bz) + 4);
            const int64_t nj = rk_bgzf_plan_members(br.bz, job_text - ((uint64_t)1 << 18), 16381, first.data(), (int64_t)first.size());
            if (nj < 0) { failed = true; break; }
            rk_host_register_readonly(rk_bgzf_image(br.bz), (size_t)rk_bgzf_file_bytes(br.bz)); // (the DMA engine reads the mapping itself; refused: staged uploads)
            for (int64_t j = 0; j < nj && !failed.load(); ++j) {
                const int rc = rk_fasta_load_put_bgzf(load, via, br.bz, first[(size_t)j], first[(size_t)j + 1], br.at + rk_bgzf_text_offset(br.bz, first[(size_t)j]));
                if (rc != RK_OK) failed = true; // (a damaged member as well: the host parser reports it)
            }
            if (!failed.load() && rk_fasta_load_put_newline(load, br.at + br.size) != RK_OK) failed = true;
        }
        if (via) rk_fastq_slot_destroy(via);
    }
    for (auto& t : th) t.join();
    for (int fd : fds) if (fd >= 0) close(fd);
    tick("references: text read and uploaded", tr);
    bool ok = !failed.load() && next.load() >= jobs.size();
    rk_fasta_index ix;
    memset(&ix, 0, sizeof ix);
    if (ok && rk_fasta_load_finish(load, total, &ix) != RK_OK) { fprintf(stderr, "rkmh: references through the device: %s; parsing on the host\n", rk_last_error()); ok = false; }
    if (ok && ix.status != 0) {
        if (g_timing) fprintf(stderr, "[rkmh timing] references: not plain line-structured FASTA (status %d): the host parser reads them\n", ix.status);
        ok = false;
    }
    tick("references: headers and line ends stripped on the device", tr);
    if (ok) {
        keep.name_offsets.assign(ix.name_offsets, ix.name_offsets + ix.nseq + 1);
        keep.names.assign(ix.names, ix.names + keep.name_offsets.back());
        keep.names.push_back('\0');
        CK(rk_set_references_fasta(g.ctx[0], load, o.ks.data(), (int)o.ks.size(), o.sketch, max_samples, counter_slots));
        memset(&refs, 0, sizeof refs);
        refs.nseq = ix.nseq;
        refs.names = keep.names.data();
        refs.name_offsets = keep.name_offsets.data();
        tick("references: sketched", tr);
        if (g_timing) fprintf(stderr, "[rkmh timing] references through the device: %lld sequences, %.0f MB of text\n", (long long)ix.nseq, (double)total / 1e6);
    }
    rk_fasta_load_destroy(load);
    return ok;
}

// the kseq-grammar scanner as a producer thread: batches of the given files (each from a byte offset, 0 = its start), numbered
std::thread start_scanner(QueueT<Numbered>& q, std::vector<std::pair<const char*, uint64_t>> files, RawKind kind) {
    return std::thread([&q, files, kind] {
        int64_t seq = 0;
        for (auto& f : files) {
            rk_reader* rd = nullptr;
            if ((f.second ? rk_reader_open_at(f.first, f.second, &rd) : rk_reader_open(f.first, &rd)) != RK_OK) { q.err = rk_last_error(); break; }
            if (kind == RAW_STREAM) rk_reader_set_options(rd, RK_READER_NO_QUALS); // stream never looks at qualities (filter prints them)
            for (;;) {
                Numbered nb;
                if (rk_reader_next(rd, 1 << 20, 1ull << 28, &nb.reads) != RK_OK) { q.err = rk_last_error(); break; }
                if (nb.reads.nseq == 0) { rk_seqset_free(&nb.reads); break; }
                nb.seq = seq++;
                q.push(nb);
            }
            rk_reader_close(rd);
            if (!q.err.empty()) break;
        }
        q.finish();
    });
}

// kind: stream's lines (emit_lines) or filter's records (emit_passing)
void run_scanner_pipeline(DeviceGroup& group, const rk_seqset& refs, const Opts& o, RawKind kind, QueueT<Numbered>& q, std::thread& producer) {
    double t_cls = 0, t_emit = 0, t_wait = 0;
    // parser -> (one classify thread per device) -> writer.  Batches are numbered by the parser; the writer puts them back in
    // input order, so the output does not depend on how many devices took part or on which one was faster.
    if (q.cap < 2 * group.size()) { std::lock_guard<std::mutex> l(q.m); q.cap = 2 * group.size(); q.cv.notify_all(); }
    QueueT<Classified> done_q;
    done_q.cap = 2 * group.size() + 2;
    OutPool out_pool;
    std::thread writer([&] { // lines leave in read order: one writer, batches by number
        Classified c;
        std::string wbuf;
        std::map<int64_t, Classified> waiting;
        int64_t next = 0;
        while (done_q.pop(&c)) {
            waiting.emplace(c.seq, std::move(c));
            for (auto it = waiting.find(next); it != waiting.end(); it = waiting.find(next)) {
                double a = now_s();
                if (kind == RAW_FILTER) emit_passing(it->second.reads, it->second.out4, o, wbuf);
                else emit_lines(refs, it->second.reads, it->second.out4, o, wbuf);
                out_pool.put(it->second.out4, it->second.out_cap);
                rk_seqset_free(&it->second.reads);
                t_emit += now_s() - a;
                waiting.erase(it);
                ++next;
            }
        }
    });
    std::mutex tm;
    std::vector<std::string> werr(group.size());
    auto work = [&](size_t d) {
        for (;;) {
            double a = now_s();
            Numbered nb;
            if (!q.pop(&nb)) break;
            double b = now_s();
            Classified c;
            c.reads = nb.reads; c.seq = nb.seq;
            c.out4 = out_pool.get((size_t)c.reads.nseq, &c.out_cap);
            if (rk_classify_batch(group.ctx[d], c.reads.bases, c.reads.offsets, c.reads.nseq, c.out4) != RK_OK) { werr[d] = rk_last_error(); break; }
            double c2 = now_s();
            done_q.push(std::move(c));
            std::lock_guard<std::mutex> l(tm);
            t_wait += b - a; t_cls += c2 - b;
        }
    };
    std::vector<std::thread> workers;
    for (size_t d = 1; d < group.size(); ++d) workers.emplace_back(work, d);
    work(0);
    for (auto& t : workers) t.join();
    for (auto& e : werr) if (!e.empty()) { fprintf(stderr, "rkmh: %s\n", e.c_str()); fail_exit(); }
    done_q.finish();
    writer.join();
    if (g_timing) fprintf(stderr, "[rkmh timing] wait-for-parser %.3f s, classify %.3f s, format+write %.3f s (overlapped; summed over %zu device(s))\n", t_wait, t_cls, t_emit, group.size());
    producer.join();
    if (!q.err.empty()) { fprintf(stderr, "rkmh: %s\n", q.err.c_str()); fail_exit(); }
}
