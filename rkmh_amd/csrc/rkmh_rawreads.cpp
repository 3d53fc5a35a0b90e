// rkmh_rawreads.cpp -- FASTQ read files through the device front end (plain, BGZF and gzip): the registry of input files, the engine and
// its workers (RawEngine), one pass over a run of files (stream_files_raw) and the -M protocol over two of them (two_pass_raw).
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <climits>

#include "rkmh_cli.hpp"

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
Input& input_of(const char* path) {
    auto it = g_inputs.find(path);
    if (it != g_inputs.end()) return it->second;
    Input in;
    if (env_flag("RKMH_BGZF", true) && rk_bgzf_open(path, &in.bz) == RK_OK) in.kind = IN_BGZF;
    else if (gzip_on_device() && rk_gzip_open(path, &in.gz) == RK_OK) in.kind = IN_GZIP;
    else in = Input();
    return g_inputs[path] = in;
}
const Input* known_input(const char* path) { auto it = g_inputs.find(path); return it == g_inputs.end() ? nullptr : &it->second; }
static const Input* read_archive(const char* path) { const Input* in = known_input(path); return in && in->reads ? in : nullptr; }
bool any_read_archive() { for (auto& kv : g_inputs) if (kv.second.reads) return true; return false; }

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

// ------------------------------------------------------------------------------------------------------------------------
// A run of read files through the device front end (stream_files_raw, at the end of this part): RawRun is the run -- its files, the
// two job queues, the ordered output, where it failed -- and the coordinator that plans the jobs; RawWorker is one worker thread.
namespace {
// bz: compressed (BGZF) -- a job is a run of members [first[j], first[j + 1]); mega: ... inflated on the device: large jobs, device-text
// slots, eng.pieces block numbers each (else by the worker that takes the job).  njobs < 0: the plan failed (said when its turn comes)
struct File {
    const char* path = nullptr; int fd = -1; int64_t fsize = 0; rk_bgzf* bz = nullptr; rk_gzip* gz = nullptr;
    bool gz_own = false, gz_locked = false, mega = false; const uint8_t* fmap = nullptr;
    std::vector<int64_t> first; int64_t njobs = 0;
};
// file: index into files; at: where the job's first record starts in the (uncompressed) text; nseq: block numbers it owns
struct Job { size_t file = 0; int64_t seq = 0, lo = 0, hi = 0, at = 0, nseq = 1; };
// what a loader found: nbytes of whole records in the slot, the first of them at byte `at` of the file's text -- or nothing (EMPTY), or
// text that is not for the device (REFUSED: the scanner takes the file over from `at`)
enum LoadState { LOADED, EMPTY, REFUSED };
struct Loaded { uint64_t nbytes = 0; int64_t at = 0; LoadState state = LOADED; };

struct RawRun {
    RawEngine& eng; DeviceGroup& g; const Opts& o; const RawKind kind; std::vector<rk_counter*>* const cnts;
    const bool counting;
    const bool trace_jobs = getenv("RKMH_TRACE_JOBS") != nullptr;
    rk_line_parts* lp = nullptr;
    std::vector<File> files;
    QueueT<Job> jobs_plain, jobs_mega; // (a worker takes the jobs its slot is made for)
    bool any_mega = false, any_plain = false, any_gz = false;
    OrderedOut out;
    std::atomic<int64_t> fail_seq{INT64_MAX};
    std::mutex fm;
    std::map<int64_t, std::pair<size_t, int64_t>> fail_at; // block number -> (file, its first byte)
    std::mutex tm;
    std::atomic<int> live_plain{0}, live_mega{0};
    int needed_mega = INT32_MAX;
    int64_t window = 0; // blocks that may be parked ahead of the one due: workers x 4 x (pieces if any device-text file else 1) + 2, for every put
    int64_t seq = 0;    // the coordinator's next block number
    std::vector<uint8_t> win;
    std::vector<std::thread> workers;

    RawRun(RawEngine& e, DeviceGroup& g_, const Opts& o_, RawKind k, std::vector<rk_counter*>* c) : eng(e), g(g_), o(o_), kind(k), cnts(c), counting(k == RAW_COUNT) {}
    void open_files(const std::vector<const char*>& paths, const std::vector<int64_t>& fsizes) {
        files.resize(paths.size());
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
                    CKE(rk_gzip_open(F.path, &F.gz));
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
            if (F.bz) { // jobs = runs of members holding about a block of text (the records are cut after inflating), planned ONCE
                const uint64_t per_job = F.mega ? eng.mega : eng.block;
                const uint64_t target = per_job > ((uint64_t)1 << 20) ? per_job - ((uint64_t)1 << 18) : per_job * 3 / 4;
                F.first.resize((size_t)rk_bgzf_members(F.bz) + 4);
                // (device jobs: at most 16 381 members + the three around them = 256 waves of 64 members: two launches fill the chip exactly)
                F.njobs = rk_bgzf_plan_members(F.bz, target, F.mega ? 16381 : INT64_MAX, F.first.data(), (int64_t)F.first.size());
            }
            (F.mega ? any_mega : any_plain) = true;
            if (F.gz) any_gz = true;
        }
        // how many jobs the device-text workers will share (an ordinary gzip file is one job, a BGZF file a few): a worker without a job
        // to expect does not start -- its slot and work buffers are gigabytes of allocations that slow the others down while they are made
        // (one gzip file: 0.36 s as a command with one such worker setting up, 0.6 - 0.77 s with four or five)
        size_t mega_jobs = 0;
        for (const File& F : files) {
            if (F.gz) ++mega_jobs;
            else if (F.bz && F.mega) mega_jobs += F.njobs > 0 ? (size_t)F.njobs : 1;
        }
        needed_mega = (int)std::min<size_t>(mega_jobs, (size_t)INT32_MAX);
    }
    void close_files() {
        for (File& F : files) {
            if (F.fmap) { rk_host_unregister(F.fmap); munmap((void*)F.fmap, (size_t)F.fsize); }
            if (F.gz_own) { if (F.gz_locked) rk_host_unregister(rk_gzip_image(F.gz)); rk_gzip_close(F.gz); }
            close(F.fd);
        }
    }
    void start_workers();
    // The coordinator: jobs file after file, numbered in the order of the output, until a hand-over is declared
    void plan() {
        for (size_t fi = 0; fi < files.size() && fail_seq.load() == INT64_MAX; ++fi) {
            if (files[fi].gz) plan_gzip(fi);
            else if (files[fi].bz) plan_bgzf(fi);
            else plan_plain(fi);
        }
        jobs_plain.finish();
        jobs_mega.finish();
    }
    // an ordinary gzip file is one job: its stretches, in order, on one worker
    void plan_gzip(size_t fi) {
        const int64_t ncalls = rk_gzip_plan(files[fi].gz, eng.mega);
        if (ncalls < 0) die();
        Job jb; jb.file = fi; jb.seq = seq; jb.nseq = ncalls * eng.pieces;
        seq += jb.nseq;
        jobs_mega.push(jb);
    }
    void plan_bgzf(size_t fi) {
        const File& F = files[fi];
        if (F.njobs < 0) die();
        const int64_t per = F.mega ? eng.pieces : 1;
        for (int64_t j = 0; j < F.njobs && fail_seq.load() == INT64_MAX; ++j) {
            Job jb; jb.file = fi; jb.seq = seq; jb.nseq = per; jb.lo = F.first[(size_t)j]; jb.hi = F.first[(size_t)j + 1];
            seq += per;
            (F.mega ? jobs_mega : jobs_plain).push(jb);
        }
    }
    // Plain text: ranges of whole records.  A range that is cut wrongly (possible only in text that is not four lines per record) is
    // refused by the device and the scanner takes over from its first byte.
    void plan_plain(size_t fi) {
        const File& F = files[fi];
        const int64_t B = (int64_t)eng.block;
        for (int64_t pos = 0; pos < F.fsize && fail_seq.load() == INT64_MAX;) {
            const int64_t hi = F.fsize - pos > B ? find_cut(F.fd, pos, B) : F.fsize;
            if (hi < 0) { declare_failed(seq, fi, pos); break; } // no record start anywhere in the range: hand the file over from here
            Job j; j.file = fi; j.seq = seq++; j.lo = pos; j.hi = hi;
            jobs_plain.push(j);
            pos = hi;
        }
    }
    // The end of the range that begins at pos: the last record start (four-line rule, rk_fastq_cut) inside a window in front of the
    // nominal end pos + B; the window widens until it holds one.  -1: none in the whole range -- not for the device.
    int64_t find_cut(int fd, int64_t pos, int64_t B) {
        for (int64_t wlen = 1 << 16;; wlen *= 8) {
            if (wlen > B - 1) wlen = B - 1;
            const int64_t wlo = pos + B - wlen; // the window ends at the nominal end of the range
            win.resize((size_t)wlen);
            const int64_t cut = pread_full(fd, win.data(), wlen, wlo) ? rk_fastq_cut(win.data(), (uint64_t)wlen) : -1;
            if (cut > 0) return wlo + cut;
            if (wlen >= B - 1) return -1;
        }
    }
    // the scanner takes the file over at byte `at`: block s and every later one is dropped.  (lower_limit comes before block s is
    // parked: the sink cannot pass it.)
    void declare_failed(int64_t s, size_t file, int64_t at) {
        { std::lock_guard<std::mutex> l(fm); fail_at[s] = std::make_pair(file, at); }
        if (!counting) out.lower_limit(s);
        int64_t cur = fail_seq.load();
        while (s < cur && !fail_seq.compare_exchange_weak(cur, s)) {}
    }
    // (block numbers of a job that carry no output of their own)
    void put_empty(const Job& jb) { if (!counting) for (int64_t e = 0; e < jb.nseq; ++e) out.put(jb.seq + e, std::vector<char>(), 0, window); }
};

struct RawWorker {
    RawRun& R; const size_t wi; RawEngine::Worker& W;
    rk_fastq_slot* slot = nullptr;
    double t_rd = 0, t_dv = 0, t_fm = 0;
    int64_t nblk = 0, nrec = 0;
    RawWorker(RawRun& r, size_t i) : R(r), wi(i), W(r.eng.w[i]) {}
    // Who starts: a worker with no file of its kind leaves at once, a device-text worker of rank >= needed_mega leaves without
    // allocating.  The slot is made under slot_mu, ONE worker at a time (RawEngine::slot_mu), the gzip work buffers only in a run
    // with a gzip file; a worker that cannot get a slot leaves, unless it is the last of its kind.
    bool start() {
        if (!(W.device_text ? R.any_mega : R.any_plain)) return false;
        std::atomic<int>& live = W.device_text ? R.live_mega : R.live_plain;
        if (W.device_text) {
            size_t rank = 0;
            for (size_t j = 0; j < wi; ++j) if (R.eng.w[j].device_text) ++rank;
            if ((int)rank >= R.needed_mega) { live.fetch_sub(1); return false; }
        }
        const double t_slot = now_s();
        bool slot_ok = true;
        if (!W.slot) {
            std::lock_guard<std::mutex> sl(R.eng.slot_mu);
            slot_ok = rk_fastq_slot_create2(R.g.ctx[W.dev], W.bytes, W.device_text ? RK_SLOT_DEVICE_TEXT : 0, &W.slot) == RK_OK;
        }
        // the gunzip work buffers (gigabytes): one worker at a time, and not beside the reference stage (allocations of that size slow
        // every other call of the runtime down while they last: the first slot's, made in create(), cost the references 0.45 s)
        if (slot_ok && W.device_text && R.eng.gz_stretch && R.any_gz) {
            std::lock_guard<std::mutex> sl(R.eng.slot_mu);
            slot_ok = rk_fastq_slot_reserve_gzip(W.slot, R.eng.gz_stretch) == RK_OK;
        }
        if (!slot_ok) {
            // (memory for another slot ran out: the other workers carry on -- unless this was the last one)
            fprintf(stderr, "rkmh: worker %zu: %s\n", wi, rk_last_error());
            if (live.fetch_sub(1) == 1) { fprintf(stderr, "rkmh: no worker of the device front end could start\n"); fail_exit(); }
            return false;
        }
        slot = W.slot;
        if (g_timing && W.device_text && now_s() - t_slot > 0.002) fprintf(stderr, "[rkmh timing] worker %zu: device-text slot of %.0f MB made in %.3f s\n", wi, (double)W.bytes / 1e6, now_s() - t_slot);
        if (W.device_text && R.kind == RAW_FILTER) CK(rk_fastq_slot_set_filter_output(slot, R.o.min_matches, R.o.min_diff));
        return true;
    }
    void run() {
        if (!start()) return;
        QueueT<Job>& jobs = W.device_text ? R.jobs_mega : R.jobs_plain;
        Job cur;
        while (jobs.pop(&cur)) {
            // (a failure is declared at the first block number of the failing worker's own job: never inside another job's run)
            if (cur.seq > R.fail_seq.load()) { R.put_empty(cur); continue; } // parked empty, not processed: the scanner will redo this range
            const File& F = R.files[cur.file];
            if (F.gz) { gzip_file(F, cur); continue; }
            const double a = now_s();
            const Loaded ld = F.bz ? load_bgzf(F, cur) : load_plain(F, cur);
            cur.at = ld.at;
            if (ld.state == REFUSED) { R.declare_failed(cur.seq, cur.file, cur.at); R.put_empty(cur); }
            t_rd += now_s() - a;
            if (ld.state == LOADED) process(cur, ld.nbytes);
        }
        std::lock_guard<std::mutex> l(R.tm);
        R.eng.t_read += t_rd; R.eng.t_dev += t_dv; R.eng.t_fmt += t_fm; R.eng.blocks += nblk; R.eng.records += nrec;
    }
    // an ordinary gzip file: ONE job of this worker -- its stretches in order, eng.pieces block numbers each
    void gzip_file(const File& F, const Job& fj) {
        const int64_t per = R.eng.pieces, ncalls = fj.nseq / per;
        bool handed_over = false;
        for (int64_t r = 0; r < ncalls; ++r) {
            Job sub; sub.file = fj.file; sub.seq = fj.seq + r * per; sub.nseq = per;
            if (handed_over || sub.seq > R.fail_seq.load()) { R.put_empty(sub); continue; }
            const double a = now_s();
            const Loaded ld = load_gzip_stretch(F, r);
            sub.at = ld.at;
            if (ld.state == REFUSED) { R.declare_failed(sub.seq, sub.file, sub.at); handed_over = true; }
            if (ld.state != LOADED) R.put_empty(sub);
            t_rd += now_s() - a;
            if (ld.state != LOADED) continue;
            process(sub, ld.nbytes);
            if (R.fail_seq.load() <= sub.seq) handed_over = true; // (text that is not four lines per record)
        }
        // (the file's 4 MB on the device stay until the run ends: hipFree waits for every stream of the device to drain -- seconds, while
        // the other workers' kernels run, tools/ubench/malloc_vs_kernels.hip -- and holds the runtime's lock meanwhile)
    }
    // the next stretch of the stream inflated on the device; REFUSED: the sequential reader takes the file over from this stretch's first record
    Loaded load_gzip_stretch(const File& F, int64_t r) {
        Loaded ld;
        uint64_t off = 0;
        const int rc = rk_fastq_slot_load_gzip(slot, F.gz, r, &ld.nbytes, &off);
        if (rc < 0) die(F.path);
        ld.at = (int64_t)off;
        if (rc != RK_OK) {
            if (g_timing) fprintf(stderr, "[rkmh timing] %s: the device inflater stops at byte %lld of the text\n", F.path, (long long)off);
            ld.state = REFUSED;
        } else if (ld.nbytes == 0) ld.state = EMPTY;
        return ld;
    }
    // The members of a BGZF job inflated on the device (which may hand a job back: a member it cannot decode, a failed CRC-32 -- the host
    // inflater then reports the damage) or by this thread; the host-inflated LAST job of a file gets the newline its text may lack.
    // REFUSED: text that does not begin with '@', or a job whose records outgrow the slot
    Loaded load_bgzf(const File& F, const Job& jb) {
        Loaded ld;
        uint64_t off = 0;
        int rc = W.device_text ? rk_fastq_slot_load_bgzf(slot, F.bz, jb.lo, jb.hi, &ld.nbytes, &off) : 1;
        if (rc < 0) die(F.path);
        if (rc != RK_OK) {
            uint8_t* text = rk_fastq_slot_text(slot);
            if (W.device_text) { if (W.host_text.size() < W.bytes) W.host_text.resize(W.bytes); text = W.host_text.data(); }
            rc = rk_bgzf_fastq_records(F.bz, jb.lo, jb.hi, text, W.bytes - 1, &ld.nbytes, &off);
            if (rc == 1 || rc == RK_ERR_LIMIT) { ld.state = REFUSED; ld.nbytes = 0; }
            else if (rc != RK_OK) die(F.path);
            else {
                if (jb.hi == rk_bgzf_members(F.bz) && ld.nbytes && text[ld.nbytes - 1] != '\n') text[ld.nbytes++] = '\n';
                if (W.device_text) CKE(rk_fastq_slot_set_source(slot, text));
            }
        }
        ld.at = (int64_t)off;
        return ld;
    }
    // Bytes [lo, hi) of a plain file: uploaded from the page-locked mapping where they lie, or read into the slot's text buffer.  The
    // LAST block of a file gets the newline it may lack -- a mapped one without it is therefore copied, not mapped.
    Loaded load_plain(const File& F, const Job& jb) {
        Loaded ld;
        ld.at = jb.lo;
        ld.nbytes = (uint64_t)(jb.hi - jb.lo);
        if (F.fmap && !(jb.hi == F.fsize && F.fmap[F.fsize - 1] != '\n')) {
            CKE(rk_fastq_slot_set_source(slot, F.fmap + jb.lo));
            return ld;
        }
        uint8_t* text = rk_fastq_slot_text(slot);
        if (!pread_full(F.fd, text, jb.hi - jb.lo, jb.lo)) { fprintf(stderr, "rkmh: read error on %s\n", F.path); fail_exit(); } // (the other workers may be waiting for this block)
        if (jb.hi == F.fsize && ld.nbytes && text[ld.nbytes - 1] != '\n') text[ld.nbytes++] = '\n'; // (the slot holds 64 spare bytes)
        return ld;
    }
    // One loaded block: counted into this device's depth table (pass 1 of -M: a block that is refused ends the pass), or classified
    // and its lines parked
    void process(const Job& jb, uint64_t nbytes) {
        const double a = now_s();
        if (!R.counting) {
            CKE(rk_fastq_slot_submit(slot, nbytes));
            t_rd += now_s() - a;
            finish_block(jb);
            return;
        }
        int32_t status = 0; int64_t n = 0;
        const int rc = rk_fastq_slot_count(slot, nbytes, (*R.cnts)[W.dev], &status, &n);
        if (rc == RK_ERR_NEED_FULL) { g_need_full.store(true); status = 1; } // a read with more hashes than the sketch keeps: the pass ends, the caller repeats it with full tables
        else if (rc != RK_OK) die();
        if (status != 0) R.declare_failed(jb.seq, jb.file, jb.at);
        t_dv += now_s() - a; ++nblk; nrec += n;
    }
    // the rows of a submitted block, its lines formatted (a job of several block numbers: in as many pieces, by the helper threads) and parked
    void finish_block(const Job& jb) {
        const double b = now_s();
        rk_fastq_result res;
        CKE(rk_fastq_slot_finish(slot, &res));
        const double c = now_s();
        t_dv += c - b; ++nblk; nrec += res.status == 0 ? res.nrec : 0;
        if (res.status != 0) { R.declare_failed(jb.seq, jb.file, jb.at); R.put_empty(jb); return; }
        const uint8_t* const text = rk_fastq_slot_spans_base(slot);
        if (jb.nseq == 1) format_piece(res, text, jb.seq);
        else { // the helpers format the pieces; the slot's arrays stay untouched until all of them are parked
            Latch latch;
            latch.left = (int)jb.nseq;
            for (int64_t e = 0; e < jb.nseq; ++e)
                R.eng.pool.run([&, e] {
                    format_piece(sub_result(res, res.nrec * e / jb.nseq, res.nrec * (e + 1) / jb.nseq), text, jb.seq + e);
                    latch.done();
                });
            latch.wait();
        }
        t_fm += now_s() - c;
        if (R.trace_jobs) fprintf(stderr, "[job] worker %zu parked blocks %lld..%lld (%lld records)\n", wi, (long long)jb.seq, (long long)(jb.seq + jb.nseq - 1), (long long)res.nrec);
    }
    void format_piece(const rk_fastq_result& part, const uint8_t* text, int64_t seq) {
        std::vector<char> buf = R.out.take_buffer();
        const size_t n = part.nrec == 0 ? 0 : (R.kind == RAW_FILTER ? format_filter_raw(part, text, R.o, buf) : format_raw(R.lp, part, text, buf));
        R.out.put(seq, std::move(buf), n, R.window);
    }
};

void RawRun::start_workers() {
    jobs_plain.cap = jobs_mega.cap = eng.w.size();
    for (auto& x : eng.w) ++(x.device_text ? live_mega : live_plain);
    window = (int64_t)eng.w.size() * 4 * (any_mega ? eng.pieces : 1) + 2;
    for (size_t i = 0; i < eng.w.size(); ++i) workers.emplace_back([this, i] { RawWorker(*this, i).run(); });
}
} // namespace

// A run of read files through the device front end, as ONE pipeline: the workers go from the last blocks of a file straight to the
// first ones of the next (nothing drains between files), the output keeps the order of the command line.  Returns -1 when every
// file was taken whole; else *fail_file (an index into paths) and the byte offset in that file's text (a record start) from which
// the kseq-grammar scanner must continue -- nothing of that file from there on, and nothing of the files behind it, was printed.
// RAW_STREAM prints stream's lines, RAW_FILTER filter's records; RAW_COUNT prints nothing: it is pass 1 of -M (rkmh.cpp:904-910),
// every worker counts its blocks into its device's table cnts[dev] (summed by the caller), and the first refused block ends the pass.
int64_t stream_files_raw(RawEngine& eng, DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<const char*>& paths,
                         const std::vector<int64_t>& fsizes, RawKind kind, std::vector<rk_counter*>* cnts, size_t* fail_file) {
    RawRun R(eng, g, o, kind, cnts);
    if (kind == RAW_STREAM) CK(rk_line_parts_create(refs.names, refs.name_offsets, refs.nseq, o.sketch, o.min_matches, o.min_diff, &R.lp));
    R.open_files(paths, fsizes);
    if (!R.counting) R.out.start(g.size());
    R.start_workers();
    R.plan();
    for (auto& t : R.workers) t.join();
    if (!R.counting) R.out.finish();
    rk_line_parts_destroy(R.lp);
    R.close_files();
    if (R.out.failed) { fprintf(stderr, "rkmh: write error on standard output\n"); fail_exit(); }
    const int64_t fs = R.fail_seq.load();
    if (fs == INT64_MAX) return -1;
    if (fail_file) *fail_file = R.fail_at[fs].first;
    return R.fail_at[fs].second;
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
