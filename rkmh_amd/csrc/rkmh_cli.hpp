// rkmh_cli.hpp -- what the files of the `rkmh` command line share (the program on top of librkmh_amd.so, include/rkmh_amd.h).
//   rkmh_main.cpp       main() and the dispatch to the sub-commands
//   rkmh_exit.cpp       the fork for a fast exit, done_exit / fail_exit, stage timings, the CPUs this process may use, RKMH_* knobs
//   rkmh_frontends.cpp  what the front ends share: formatting and ordered output, the devices of a run, depth maps and the -M two-pass
//                       protocol, the host scanner pipeline
//   rkmh_rawreads.cpp   FASTQ read files through the device front end (plain / BGZF / gzip): the registry of input files, RawEngine,
//                       stream_files_raw and two_pass_raw
//   rkmh_packed.cpp     reads written by `rkmh pack` (-F), and `pack` itself
//   rkmh_refs.cpp       the -r files through the device
//   rkmh_classify.cpp   stream / classify and filter: one driver, two thin commands
//   rkmh_commands.cpp   the hashing policy and the help text; call and hash
//   rkmh_sketch_json.cpp  the reader of the JSON sketches `sketch` writes (stream -R, dist, gather); stands alone
//   rkmh_sketches.cpp   sketch sets: made from sequence files, written as JSON, loaded from -R / -Q files, cut to one scaled
//   rkmh_sample.cpp     a sequence file into a device-side accumulator, never held whole (file_feed); one sketch per sequence file built so:
//                       the -g / one-query-per-file route of the sketch sets
//   rkmh_compare.cpp    sketch, dist, gather, multigather and manysearch
//   rkmh_cluster.cpp    cluster
//   rkmh_screen.cpp     screen: bottom-s reference sketches counted in whole read files
//   rkmh_hpv16.cpp      hpv16
#pragma once
#include <getopt.h>
#include <sys/types.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rkmh_amd.h"

// ---- the process (rkmh_exit.cpp)
double now_s();
extern const bool g_timing; // RKMH_TIMING: stage timings on stderr
void tick(const char* what, double& t0);
[[noreturn]] void done_exit();
[[noreturn]] void fail_exit();
[[noreturn]] void die(const char* what = nullptr); // "rkmh: [<what>: ]<rk_last_error()>" on stderr, then fail_exit
#define CK(call) do { if ((call) != RK_OK) die(#call); } while (0)
#define CKE(call, ...) do { if ((call) != RK_OK) die(__VA_ARGS__); } while (0) // the error alone, or behind a path: CKE(call, path)
bool pread_full(int fd, void* dst, int64_t n, int64_t off); // all n bytes at off, or false
void fork_for_fast_exit();
int granted_cpus_main();
// the RKMH_* knobs: env_flag -- unset: dflt, else atoi != 0; env_long -- unset or outside [lo, hi]: dflt
bool env_flag(const char* name, bool dflt);
long env_long(const char* name, long dflt, long lo, long hi);

// ---- the hashing policy and the help text (rkmh_commands.cpp)
extern rk_policy g_policy;
void policy_apply(const char* spec, const char* from);
std::string policy_text(const rk_policy& p);
#define HASH_POLICY_OPTION {"hash-policy", required_argument, 0, 1004}
#define HASH_POLICY_HELP \
    "  --hash-policy <spec>    the mkmh choices the reference's tree does not fix, as presets (default, mash, sourmash) and/or key=value:\n" \
    "                          fold=swap32|h1|w2w1, windows=len-k|len-k+1, zero=count|skip, mask=lt|le, freqmax=incl|excl,\n" \
    "                          canon=minhash|lexmin, dedup=multiset|distinct, seed=<n>;  `mash` = fold=h1,windows=len-k+1,seed=42 (the\n" \
    "                          smaller of both strand hashes is kept, repeated values stay);  canon=lexmin hashes only the strand that\n" \
    "                          is the smaller string, dedup=distinct sketches distinct values: the rules of Mash and sourmash;\n" \
    "                          `sourmash` = mash,canon=lexmin,dedup=distinct.  RKMH_POLICY: the same, read first\n"
void print_help();
int default_k(); // "No kmer size(s) provided..." on stderr, and the 16 it announces

// ---- the JSON sketches of `rkmh sketch`, read back (rkmh_sketch_json.cpp)
struct LoadedSketches {
    std::vector<std::string> names; std::vector<uint64_t> sk; std::vector<int32_t> lens; std::vector<int> ks; int S = 0; std::string policy;
    // a file of scaled sketches (`rkmh sketch --scaled`): scaled > 0, S = 0, sk holds the values of all sketches one after the other and
    // sketch i is sk[off[i], off[i + 1]).  Only `dist` compares such sketches: every other reader refuses them (refuse_scaled).
    uint64_t scaled = 0;
    std::vector<uint64_t> off;
    // "abundances" (`rkmh sketch --scaled <n> --abund`): every sketch of the file carries them or none does; parallel to sk, each 1 .. 2^32 - 1
    bool has_abund = false;
    std::vector<uint32_t> abund;
    std::string err; // why load_sketch_json returned false, where it knows more than "cannot load"
};
bool load_sketch_json(const char* path, LoadedSketches& L, int max_S = 0); // max_S > 0: a larger "length" is refused before anything of that size is allocated

// ---- sketch sets (rkmh_sketches.cpp): what sketch, dist and gather make from sequence files, write, load and compare
void refuse_scaled(const LoadedSketches& L, const char* path, const char* command); // exits when L holds scaled sketches
struct OutBuf { // lines on their way to a file: written whenever a row ends with more than 4 MB waiting, and at flush()
    FILE* to;
    std::string s;
    explicit OutBuf(FILE* f) : to(f) {}
    void append(const std::string& t) { s += t; }
    template <class... A> void appendf(const char* fmt, A... a) { char b[200]; s.append(b, (size_t)snprintf(b, sizeof b, fmt, a...)); } // up to 200 characters
    void end_row() { if (s.size() > (1u << 22)) flush(); }
    void flush() { fwrite(s.data(), 1, s.size(), to); s.clear(); }
};
// Bottom-s sketches, S values a row, and scaled ones as CSR (sketch i = values[off[i], off[i + 1])).  From sequence files: one per
// record -- or, whole_files (-g), one per FILE: its records are sketched one by one (no window spans two contigs) and united
// (rk_merge_sketches: the bottom S under the policy's dedup rule; rk_merge_scaled), named by the path as given, seqLen their sum.
struct SketchSet { std::vector<std::string> names; std::vector<uint64_t> seq_len; std::vector<uint64_t> sk; std::vector<int32_t> lens; };
// with_abund: abund lies parallel to values (the windows behind every value; -g and the one query of a -f file sum them: rk_merge_scaled_abund)
struct ScaledSet {
    std::vector<std::string> names; std::vector<uint64_t> seq_len; std::vector<uint64_t> values; std::vector<uint64_t> off = std::vector<uint64_t>(1, 0);
    bool with_abund = false; std::vector<uint32_t> abund;
};
// min_copies (--min-copies; above 1 only with whole_files on the device): only values seen that often over the whole file count
void sketch_files(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, int S, bool whole_files, SketchSet& out, uint64_t min_copies = 1);
void sketch_files_scaled(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, uint64_t max_hash, bool whole_files, ScaledSet& out);
// whole_files on the device (rkmh_sample.cpp; RKMH_SAMPLE_DEVICE=0 keeps the route that parses each file whole): sample_file_feed
// sends one file into an empty sample; the caller takes its sketch (rk_sample_finish, rk_sample_finish_bottom); sample_file_done
// gives the bases of its records, prints the timing line and leaves the sample empty again
bool sample_on_device();
struct SampleFed { const char* route = ""; int64_t blocks = 0; double t0 = 0, t1 = 0; }; // the route taken, its blocks, when the feed began and ended
// what the records of a file go into: a block of raw FASTQ text in a slot (as rk_fastq_slot_sample takes it; *status != 0: nothing of it
// was added), or a batch of the reader; both return the library's code.  file_feed is the driver, sample_file_feed its form for a sample
struct FileSink {
    std::function<int(rk_fastq_slot*, uint64_t, int32_t*, int64_t*)> slot_block;
    std::function<int(const rk_seqset&)> host_batch;
};
SampleFed file_feed(rk_ctx* ctx, const FileSink& sink, const char* path);
SampleFed sample_file_feed(rk_ctx* ctx, rk_sample* sample, const char* path);
void sample_file_done(rk_sample* sample, const char* path, const SampleFed& fed, uint64_t* nbases);
// --min-copies: a number of 1 .. 2^32 - 1; and its three refusals, which sketch and dist word alike (`command`: "sketch" / "dist")
bool parse_min_copies(const char* text, uint64_t& m);
void refuse_min_copies(const char* command, uint64_t m, bool whole_files, bool scaled);
struct SketchRow { const uint64_t* hashes; uint64_t n, length; const uint32_t* abund = nullptr; }; // a sketch to write; "length": the S of a bottom-s sketch, a scaled one's own size; abund: its "abundances", or none
void write_sketch_json(FILE* fo, const std::vector<std::string>& names, const std::vector<uint64_t>& seq_len, const std::string& kstr,
                       const std::vector<SketchRow>& rows, uint64_t scaled, uint64_t max_hash, uint64_t min_copies = 1); // scaled = 0: a bottom-s file; min_copies > 1: "minCopies"
bool parse_scaled(const char* text, uint64_t& scaled); // --scaled: a number of at least 1, nothing else
bool parse_at_least_1(const char* text, int& v);
// What dist and gather are told alike (-r -f -R -Q -k -s -g --scaled --device --hash-policy): the rows of their long_options, and
// shared_option, which takes such an option (false: the command's own)
struct CompareInputs {
    std::vector<const char*> ref_files, query_files, ref_json, query_json;
    std::vector<int> ks;
    int S = 0, device = 0; // S: 0 without -s, -1 for a -s below 1
    bool whole_files = false, scaled_given = false, scaled_ok = true;
    bool abund = false; // gather --abund: the queries carry abundances; dist --abund: both sides do
    uint64_t scaled = 0;
    uint64_t min_copies = 1; // dist --min-copies (0: not a number of 1 .. 2^32 - 1)
    bool self() const { return query_files.empty() && query_json.empty(); }
};
#define COMPARE_OPTIONS \
    {"help", no_argument, 0, 'h'}, {"kmer", required_argument, 0, 'k'}, {"fasta", required_argument, 0, 'f'}, {"reference", required_argument, 0, 'r'}, \
    {"pre-references", required_argument, 0, 'R'}, {"pre-queries", required_argument, 0, 'Q'}, {"sketch-size", required_argument, 0, 's'}, \
    {"whole-files", no_argument, 0, 'g'}, {"device", required_argument, 0, 1000}, {"scaled", required_argument, 0, 1005}, HASH_POLICY_OPTION
bool shared_option(int c, CompareInputs& in);
struct CompareRules { // where the two differ in what they accept and in their words
    const char* command;         // "dist" / "gather": every refusal begins "rkmh <command>: "
    const char* noun;            // "<noun> needs one k-mer size"
    const char* no_bottom;       // what a bottom-s file is told after "<path> holds bottom-s sketches; "; nullptr: such files are welcome
    bool file_is_one_query;      // every -f file is ONE query, whatever -g says of the -r files
    const char* too_many_loaded; // refusal of more than 2^31-1 loaded sketches on a side before a context exists; nullptr: none
    bool abund_both_sides = false; // --abund: the references carry abundances as the queries do (dist); false: the queries alone (gather)
};
[[noreturn]] void refuse(const CompareRules& rules, const std::string& why);
int one_k(const CompareInputs& in, const CompareRules& rules); // -k, 0 without one; several are refused
int run_k(const CompareRules& rules, int k); // -k, or what the sketch files said, or the default; inside the library's range (rkmh_compare.cpp)
// The -R and -Q files: each agrees in itself (load_sketch_json), with the others, with -k / -s / --scaled where given, and with the
// run's policy.  Bottom-s files join refs / queries; scaled files are kept as loaded, each at its own "scaled", until the run's value
// is known.  k: one_k()'s answer, then what the files said; S likewise (0: nobody said).
struct LoadedSides {
    SketchSet refs, queries;
    std::vector<LoadedSketches> sc_refs, sc_queries;
    int k = 0, S = 0;
    uint64_t largest_scaled = 0; // 0: no scaled file
};
void load_sketch_files(const CompareInputs& in, const CompareRules& rules, LoadedSides& ld);
// From the loaded scaled files and the -r / -f paths to the two sets of a scaled run, all at one scaled (--scaled, or the largest of
// the files: a cut is a prefix of every row), and its context.  Sides known from files alone are refused before the context exists.
struct ScaledRun { rk_ctx* ctx = nullptr; ScaledSet refs, own_queries; const ScaledSet* queries = nullptr; }; // queries: refs when there is no -f / -Q
void start_scaled_run(const CompareInputs& in, const CompareRules& rules, const LoadedSides& ld, int k, ScaledRun& run);

// ---- the sub-commands
int main_stream(int argc, char** argv);
int main_filter(int argc, char** argv);
int main_call(int argc, char** argv);
int main_sketch(int argc, char** argv);
int main_dist(int argc, char** argv);
int main_gather(int argc, char** argv);
int main_multigather(int argc, char** argv);
int main_manysearch(int argc, char** argv);
int main_cluster(int argc, char** argv);
int main_screen(int argc, char** argv);
int main_hash(int argc, char** argv);
int main_hpv16(int argc, char** argv);
int main_pack(int argc, char** argv);

// ---- stream / filter (rkmh_classify.cpp, rkmh_frontends.cpp, rkmh_rawreads.cpp, rkmh_packed.cpp, rkmh_refs.cpp)
struct Opts {
    std::vector<const char*> refs, reads;
    std::vector<const char*> packed; // -F <file>: reads written by `rkmh pack`
    std::vector<int> ks;
    int sketch = 1000, threads = 1, min_occ = -1, min_matches = -1, min_diff = 0, max_samples = 100000;
    const char* kmer_cache = getenv("RKMH_KMER_CACHE"); // --kmer-cache FILE: the k-mer enumeration of these references, kept between runs (rk_set_kmer_cache)
    bool read_depth = false, ref_depth = false;
    int device = 0;
    std::vector<int> devices; // --devices a,b,...: reads are spread over these GPUs (one host thread + rk_ctx each); empty = --device
};
std::vector<int> parse_devices(const char* arg);
extern bool g_no_kmer_cache;

// bounded queue between pipeline stages (parser -> classify -> format/write)
template <typename V> struct QueueT {
    std::mutex m;
    std::condition_variable cv;
    std::deque<V> q;
    bool done = false;
    size_t cap = 2;
    std::string err;
    void push(V s) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return q.size() < cap; });
        q.push_back(std::move(s));
        cv.notify_all();
    }
    bool pop(V* s) {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !q.empty() || done; });
        if (q.empty()) return false;
        *s = std::move(q.front());
        q.pop_front();
        cv.notify_all();
        return true;
    }
    void finish() { std::lock_guard<std::mutex> l(m); done = true; cv.notify_all(); }
};
struct Numbered { rk_seqset reads; int64_t seq = 0; };

// The devices of one run (--devices): context 0 builds the reference sketches (rk_set_references on its GPU), the others import
// them (rk_set_reference_sketches: a few MB through the host), all in parallel threads -- the in-process form of the one-rank-per-
// GPU layout of rkmh_amd/cli.py, and the GPU analogue of the reference's -t OpenMP threads (rkmh.cpp:734, :813-898).
struct DeviceGroup {
    std::vector<rk_ctx*> ctx;
    void create(const Opts& o);
    void share_references(const Opts& o); // after the references were set on ctx[0]: the same sketches on every other context
    void destroy() { for (rk_ctx* c : ctx) rk_ctx_destroy(c); ctx.clear(); }
    size_t size() const { return ctx.size(); }
};
void group_run(DeviceGroup& g, const std::function<int(size_t)>& f);
int min_num_bound_for(int compare_with);
bool compact_maps_wanted(int bound, const char* read_map);
bool reads_fit_sketch(const rk_seqset& reads, const Opts& o);
void make_depth_maps(DeviceGroup& g, uint64_t slots, bool compact, std::vector<rk_counter*>& cnts);
bool two_pass(DeviceGroup& g, std::vector<rk_counter*>& cnts, uint64_t slots, int min_occ, const std::function<bool()>& count,
              const std::function<void()>& classify, double& t0, const char* tick_count = nullptr, const char* tick_classify = nullptr);
extern std::atomic<bool> g_need_full; // a count pass met RK_ERR_NEED_FULL: two_pass repeats it with full tables
void count_parsed(DeviceGroup& g, const rk_seqset& reads, std::vector<rk_counter*>& cnts);
void classify_parsed(DeviceGroup& g, const rk_seqset& reads, int32_t* out4);

// what a pass over the reads does with each block: stream's lines, filter's records, or pass 1 of -M (count, print nothing)
enum RawKind { RAW_STREAM, RAW_FILTER, RAW_COUNT };
void emit_lines(const rk_seqset& refs, const rk_seqset& reads, const int32_t* out4, const Opts& o, std::string& buf);
void emit_passing(const rk_seqset& reads, const int32_t* rows, const Opts& o, std::string& buf);
struct FilterDecision { int ref; int shared; bool diff_ok; };
FilterDecision filter_decide(const int32_t* r, int min_diff);

// The input files of a run, each looked at once (rkmh_rawreads.cpp): what a path was found to be, and its open archive.  Read files
// and references share the table; `reads` marks the compressed files raw_eligible took as read files (the device front end's jobs).
enum InputKind { IN_PLAIN, IN_BGZF, IN_GZIP }; // IN_PLAIN: not opened as an archive (uncompressed text, or anything else)
struct Input { InputKind kind = IN_PLAIN; rk_bgzf* bz = nullptr; rk_gzip* gz = nullptr; bool reads = false; };
Input& input_of(const char* path);             // opens the path as an archive when it is looked at for the first time
const Input* known_input(const char* path);    // nullptr: not looked at yet
inline int first_byte(const Input& in) { return in.kind == IN_BGZF ? rk_bgzf_first_byte(in.bz) : rk_gzip_first_byte(in.gz); }
inline int64_t text_bytes(const Input& in) { return in.kind == IN_BGZF ? (int64_t)rk_bgzf_text_bytes(in.bz) : (int64_t)rk_gzip_text_bytes_hint(in.gz); }
bool bgzf_on_device();
bool raw_eligible(const char* path, int64_t* size, char first = '@');
bool any_read_archive();
void register_bgzf_mappings();

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
    void start(size_t ndev = 1);
    std::vector<char> take_buffer();
    // buf[0 .. len) are the lines of block seq; the buffer becomes the sink's (a spare one comes back from take_buffer)
    void put(int64_t seq, std::vector<char>&& buf, size_t len, int64_t window);
    void finish();
};
struct Latch {
    std::mutex m;
    std::condition_variable cv;
    int left = 0;
    void done() { std::lock_guard<std::mutex> l(m); if (--left == 0) cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return left == 0; }); }
};
// one block's rows as lines / records (rk_format.cpp), and records [lo, hi) of a block as a result of their own
rk_fastq_result sub_result(const rk_fastq_result& r, int64_t lo, int64_t hi);
size_t format_raw(const rk_line_parts* lp, const rk_fastq_result& r, const uint8_t* text, std::vector<char>& buf);
size_t format_filter_raw(const rk_fastq_result& r, const uint8_t* text, const Opts& o, std::vector<char>& buf);

// Work handed to a few helper threads: the lines of a device-inflated BGZF job (hundreds of megabytes of text, millions of records)
// are formatted piece by piece by all of them while its worker waits, each piece parked under its own block number
struct FormatPool {
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    std::vector<std::thread> th;
    bool closing = false;
    void start(int n);
    void run(std::function<void()> f) { { std::lock_guard<std::mutex> l(m); q.push_back(std::move(f)); } cv.notify_one(); }
    void stop();
};
extern const std::vector<const char*>* g_read_paths; // the -f files of this run (RawEngine::create: are they all BGZF?)
struct RawEngine {
    // one slot per worker: one block on the device at a time.  (Two slots per worker -- the next block read while the previous one is on
    // the device -- were measured no faster on 64 M reads and 0.2 s slower on 16 M, profiles/r04_e2e_ab.txt, and are gone.)
    struct Worker { rk_fastq_slot* slot = nullptr; size_t dev = 0; bool device_text = false; uint64_t bytes = 0; std::vector<uint8_t> host_text; };
    std::vector<Worker> w;
    uint64_t block = 0;  // text per job: plain files, and BGZF files inflated on the host
    uint64_t mega = 0;   // text per job of BGZF files inflated on the device (0: no such file in this run)
    int pieces = 1;      // block numbers (= output pieces, formatted in parallel) per device-inflated job
    uint64_t gz_stretch = 0; // ordinary gzip files in this run: the most compressed bytes one call takes (0: none)
    bool need_plain_workers = false; // the references go through the workers' page-locked text buffers (refs_through_device)
    FormatPool pool;
    double t_read = 0, t_dev = 0, t_fmt = 0;
    int64_t blocks = 0, records = 0;
    bool create(DeviceGroup& g);
    // A worker makes its slot when it starts, ONE worker at a time: allocations of several threads queue up inside the runtime anyway,
    // and they slow every other call down while they do (measured: a device-text slot of 841 MB takes 24 ms on its own -- 23 of
    // them page-locking its host arrays --, 60 to 230 ms when three are made at once beside the reference stage, which then takes
    // 0.45 s instead of 0.15).  The first worker's slot exists already (create); the others follow 24 ms apart.
    std::mutex slot_mu;
    void destroy() { pool.stop(); for (auto& x : w) if (x.slot) rk_fastq_slot_destroy(x.slot); w.clear(); }
};
int64_t stream_files_raw(RawEngine& eng, DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<const char*>& paths,
                         const std::vector<int64_t>& fsizes, RawKind kind, std::vector<rk_counter*>* cnts, size_t* fail_file);
bool two_pass_raw(RawEngine& eng, DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<int64_t>& sizes,
                  std::vector<rk_counter*>& cnts, RawKind kind, double& t0, uint64_t slots);
void run_packed(DeviceGroup& g, const rk_seqset& refs, const Opts& o, const std::vector<const char*>& paths, RawKind kind, uint64_t slots, int bound, double& t0);
struct DeviceRefs { std::vector<char> names; std::vector<uint64_t> name_offsets; };
bool refs_for_device(const Opts& o, std::vector<int64_t>* sizes = nullptr, uint64_t* total_out = nullptr);
bool refs_through_device(RawEngine& eng, DeviceGroup& g, const Opts& o, int max_samples, uint64_t counter_slots, rk_seqset& refs, DeviceRefs& keep);
std::thread start_scanner(QueueT<Numbered>& q, std::vector<std::pair<const char*, uint64_t>> files, RawKind kind);
void run_scanner_pipeline(DeviceGroup& group, const rk_seqset& refs, const Opts& o, RawKind kind, QueueT<Numbered>& q, std::thread& producer);
