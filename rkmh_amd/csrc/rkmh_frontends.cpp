// rkmh_frontends.cpp -- what the front ends of stream / filter share: the output (lines and records, blocks written in input order, the
// helper threads that format them), the devices of a run, the depth maps and the -M two-pass protocol, and the host scanner pipeline.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

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
std::atomic<bool> g_need_full{false}; // a count pass met RK_ERR_NEED_FULL: repeat it with full tables

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

// ---- OrderedOut (rkmh_cli.hpp): the blocks of a run written in the order of their numbers
void OrderedOut::start(size_t ndev) {
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
std::vector<char> OrderedOut::take_buffer() {
    std::lock_guard<std::mutex> l(m);
    if (spare.empty()) return std::vector<char>();
    std::vector<char> b = std::move(spare.back());
    spare.pop_back();
    return b;
}
void OrderedOut::put(int64_t seq, std::vector<char>&& buf, size_t len, int64_t window) {
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
void OrderedOut::finish() {
    {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return in_flight == 0; });
        closing = true;
    }
    cv_task.notify_all();
    for (auto& t : writers) t.join();
    if (direct && lseek(1, base + total, SEEK_SET) < 0) failed = true; // later output continues behind the blocks
}

// all n bytes at off, or false (the end of the file, or an error)
bool pread_full(int fd, void* dst, int64_t n, int64_t off) {
    for (int64_t have = 0; have < n;) {
        const ssize_t got = pread(fd, (char*)dst + have, (size_t)(n - have), (off_t)(off + have));
        if (got <= 0) return false;
        have += got;
    }
    return true;
}

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


// records [lo, hi) of a classified block as a result of their own (the spans index the same text)
rk_fastq_result sub_result(const rk_fastq_result& r, int64_t lo, int64_t hi) {
    rk_fastq_result p = r;
    p.nrec = hi - lo;
    p.out4 = r.out4 + lo * 4;
    p.name_off = r.name_off + lo; p.name_len = r.name_len + lo;
    p.seq_off = r.seq_off + lo; p.seq_len = r.seq_len + lo; p.qual_off = r.qual_off + lo;
    return p;
}

// the lines of one block (rk_fastq_stream_lines: rk_format.cpp), names taken from where the slot says they lie
size_t format_raw(const rk_line_parts* lp, const rk_fastq_result& r, const uint8_t* text, std::vector<char>& buf) {
    const size_t need = (size_t)rk_fastq_stream_lines_bound(lp, &r);
    if (buf.size() < need) buf.resize(need + need / 8); // (grows a few times, then stays: no per-block allocation or zero-fill)
    const int64_t n = rk_fastq_stream_lines(lp, &r, text, buf.data(), buf.size());
    if (n < 0) die();
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
size_t format_filter_raw(const rk_fastq_result& r, const uint8_t* text, const Opts& o, std::vector<char>& buf) {
    const size_t need = (size_t)rk_fastq_filter_records_bound(&r);
    if (buf.size() < need) buf.resize(need + need / 8);
    const int64_t n = rk_fastq_filter_records(&r, text, o.min_matches, o.min_diff, buf.data(), buf.size());
    if (n < 0) die();
    return (size_t)n;
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
