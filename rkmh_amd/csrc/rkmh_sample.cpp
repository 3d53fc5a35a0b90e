// rkmh_sample.cpp -- the records of ONE sequence file into a device-side accumulator (file_feed over a FileSink: a sample here, the
// screen of rkmh_screen.cpp), and on top of it ONE sketch per sequence file, built on the device (rk_sample_*, include/rkmh_amd.h "SAMPLE SKETCHES"): the
// route of sketch_files_scaled for `sketch --scaled -g`, the query side of gather and multigather, and dist / manysearch with -g; and,
// into a bottom sample ("BOTTOM SAMPLES"), the route of sketch_files for `sketch -g -s` and `dist -g -s`.
// A file is never held whole: plain FASTQ text goes block by block through two alternating FASTQ slots (the next block is read while
// the device works on this one), a BGZF file job by job through two device-text slots, everything else (FASTA, ordinary gzip,
// standard input) through the sequential reader in bounded batches.  A block the device refuses -- text that is not four lines per
// record -- has added nothing: the kseq-grammar scanner takes the file over from its first byte, as it does for stream.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <future>

#include "rkmh_cli.hpp"

// RKMH_SAMPLE_DEVICE=0 keeps the route that parses each file whole (the measured comparison of the two: DESIGN.md section 20)
bool sample_on_device() {
    static const bool on = env_flag("RKMH_SAMPLE_DEVICE", true);
    return on;
}

namespace {

enum LoadState { LOADED, EMPTY, REFUSED, END };
struct Loaded { uint64_t nbytes = 0; int64_t at = 0, next = 0; LoadState state = END; };

struct SampleFile {
    rk_ctx* ctx; const FileSink& sink; const char* path;
    const char* route = "reader";
    int64_t blocks = 0, records = 0, handed_at = -1;
    rk_fastq_slot* slot[2] = {nullptr, nullptr};
    ~SampleFile() { for (rk_fastq_slot* s : slot) if (s) rk_fastq_slot_destroy(s); }

    // the sequential reader, from byte `at` of the file's text on: bounded batches into the sink
    void through_reader(uint64_t at) {
        rk_reader* rd = nullptr;
        CKE(at ? rk_reader_open_at(path, at, &rd) : rk_reader_open(path, &rd), path);
        rk_reader_set_options(rd, RK_READER_NO_QUALS);
        for (;;) {
            rk_seqset s;
            CKE(rk_reader_next(rd, 1 << 18, 1ull << 26, &s), path);
            if (s.nseq == 0) { rk_seqset_free(&s); break; }
            CKE(sink.host_batch(s), path);
            records += s.nseq;
            rk_seqset_free(&s);
        }
        rk_reader_close(rd);
    }

    // Blocks loaded by `load(which slot, where)` on a helper thread while the device works on the block before; where = Loaded::next.
    // Returns -1 when the file was taken whole, else the byte of its text from which the scanner continues.
    template <class Load>
    int64_t alternate(Load load, int64_t begin) {
        int which = 0;
        std::future<Loaded> next = std::async(std::launch::async, load, which, begin);
        for (;;) {
            const Loaded ld = next.get();
            if (ld.state == END) return -1;
            if (ld.state == REFUSED) return ld.at;
            const int cur = which;
            which ^= 1;
            next = std::async(std::launch::async, load, which, ld.next);
            if (ld.state == LOADED) {
                int32_t status = 0;
                int64_t n = 0;
                if (sink.slot_block(slot[cur], ld.nbytes, &status, &n) != RK_OK) { const std::string e = rk_last_error(); next.wait(); fprintf(stderr, "rkmh: %s: %s\n", path, e.c_str()); fail_exit(); }
                if (status != 0) { next.wait(); return ld.at; } // nothing of the block was added
                ++blocks; records += n;
            }
        }
    }

    void plain(int64_t fsize) {
        route = "plain";
        const uint64_t block = (uint64_t)env_long("RKMH_RAW_BLOCK_KB", 16 << 10, 4, LONG_MAX) << 10;
        const int fd = open(path, O_RDONLY);
        if (fd < 0) { fprintf(stderr, "rkmh: cannot open %s\n", path); fail_exit(); }
        for (auto& s : slot) CKE(rk_fastq_slot_create(ctx, block + 64, &s), path);
        std::vector<uint8_t> win[2];
        // the end of the range that begins at pos: the last record start (rk_fastq_cut) inside a window in front of pos + block, the
        // window widening until it holds one; -1: none in the whole range
        auto find_cut = [&](std::vector<uint8_t>& w, int64_t pos) -> int64_t {
            const int64_t B = (int64_t)block;
            for (int64_t wlen = 1 << 16;; wlen *= 8) {
                if (wlen > B - 1) wlen = B - 1;
                const int64_t wlo = pos + B - wlen;
                w.resize((size_t)wlen);
                const int64_t cut = pread_full(fd, w.data(), wlen, wlo) ? rk_fastq_cut(w.data(), (uint64_t)wlen) : -1;
                if (cut > 0) return wlo + cut;
                if (wlen >= B - 1) return -1;
            }
        };
        auto load = [&](int which, int64_t pos) {
            Loaded ld;
            ld.at = pos;
            if (pos >= fsize) return ld;
            const int64_t hi = fsize - pos > (int64_t)block ? find_cut(win[which], pos) : fsize;
            if (hi < 0) { ld.state = REFUSED; return ld; }
            uint8_t* text = rk_fastq_slot_text(slot[which]);
            if (!pread_full(fd, text, hi - pos, pos)) { fprintf(stderr, "rkmh: read error on %s\n", path); fail_exit(); }
            ld.nbytes = (uint64_t)(hi - pos);
            if (hi == fsize && ld.nbytes && text[ld.nbytes - 1] != '\n') text[ld.nbytes++] = '\n'; // (the slot holds 64 spare bytes)
            ld.next = hi;
            ld.state = LOADED;
            return ld;
        };
        handed_at = alternate(load, 0);
        close(fd);
    }

    void bgzf(rk_bgzf* bz) {
        route = "bgzf";
        register_bgzf_mappings(); // the compressed members leave from the page-locked mapping, as for stream
        const uint64_t job = (uint64_t)env_long("RKMH_BGZF_JOB_KB", 64 << 10, 64, 1536 << 10) << 10;
        const uint64_t target = job > ((uint64_t)1 << 20) ? job - ((uint64_t)1 << 18) : job * 3 / 4;
        std::vector<int64_t> first((size_t)rk_bgzf_members(bz) + 4);
        const int64_t njobs = rk_bgzf_plan_members(bz, target, 16381, first.data(), (int64_t)first.size());
        if (njobs < 0) die(path);
        for (auto& s : slot) CKE(rk_fastq_slot_create2(ctx, job + 64, RK_SLOT_DEVICE_TEXT, &s), path);
        std::vector<uint8_t> host_text[2];
        const int64_t members = rk_bgzf_members(bz);
        auto load = [&](int which, int64_t j) {
            Loaded ld;
            if (j >= njobs) return ld;
            const int64_t lo = first[(size_t)j], hi = first[(size_t)j + 1];
            uint64_t off = 0;
            int rc = rk_fastq_slot_load_bgzf(slot[which], bz, lo, hi, &ld.nbytes, &off);
            if (rc < 0) die(path);
            ld.state = LOADED;
            if (rc != RK_OK) { // a job the device hands back: inflated here, uploaded from this buffer
                std::vector<uint8_t>& text = host_text[which];
                if (text.size() < job + 64) text.resize(job + 64);
                rc = rk_bgzf_fastq_records(bz, lo, hi, text.data(), job + 63, &ld.nbytes, &off);
                if (rc == 1 || rc == RK_ERR_LIMIT) { ld.state = REFUSED; ld.nbytes = 0; }
                else if (rc != RK_OK) die(path);
                else {
                    if (hi == members && ld.nbytes && text[ld.nbytes - 1] != '\n') text[ld.nbytes++] = '\n';
                    CKE(rk_fastq_slot_set_source(slot[which], text.data()), path);
                }
            }
            if (ld.state == LOADED && ld.nbytes == 0) ld.state = EMPTY;
            ld.at = (int64_t)off;
            ld.next = j + 1;
            return ld;
        };
        handed_at = alternate(load, 0);
    }

    void run() {
        int64_t size = 0;
        if (raw_eligible(path, &size, '@')) {
            const Input* in = known_input(path);
            if (in && in->kind == IN_BGZF && bgzf_on_device()) bgzf(in->bz);
            else if (!in || in->kind == IN_PLAIN) plain(size);
            else { through_reader(0); return; } // (an ordinary gzip file: its device inflater is not part of this route)
            if (handed_at >= 0) {
                for (auto& s : slot) if (s) { rk_fastq_slot_destroy(s); s = nullptr; }
                if (g_timing) fprintf(stderr, "[rkmh timing] sample %s: the device front end stops at byte %lld of the text: the scanner takes over\n", path, (long long)handed_at);
                // (byte 0: the reader's own start, so that a file that is no FASTQ at all is read as whatever it is)
                through_reader((uint64_t)handed_at);
            }
            return;
        }
        through_reader(0);
    }
};

} // namespace

// All records of `path` into `sink`, by whichever route the file takes: raw FASTQ blocks through sink.slot_block, the reader's batches
// through sink.host_batch.
SampleFed file_feed(rk_ctx* ctx, const FileSink& sink, const char* path) {
    SampleFed fed;
    fed.t0 = now_s();
    SampleFile F{ctx, sink, path};
    F.run();
    fed.route = F.route;
    fed.blocks = F.blocks;
    fed.t1 = now_s();
    return fed;
}
// All records of `path` into the empty `sample`.  The caller then takes what it wants from the sample (rk_sample_finish,
// rk_sample_finish_bottom) and ends with sample_file_done.
SampleFed sample_file_feed(rk_ctx* ctx, rk_sample* sample, const char* path) {
    const FileSink sink{[sample](rk_fastq_slot* slot, uint64_t nbytes, int32_t* status, int64_t* nrec) { return rk_fastq_slot_sample(slot, nbytes, sample, status, nrec); },
                        [sample](const rk_seqset& s) { return rk_sample_add_batch(sample, s.bases, s.offsets, s.nseq); }};
    return file_feed(ctx, sink, path);
}
// *nbases = the bases of the file's records; the timing line; `sample` is empty again
void sample_file_done(rk_sample* sample, const char* path, const SampleFed& fed, uint64_t* nbases) {
    rk_sample_stats_t st;
    st.struct_size = sizeof st;
    CKE(rk_sample_stats(sample, &st), path);
    *nbases = st.nbases;
    if (g_timing)
        fprintf(stderr, "[rkmh timing] sample %s: %s route, %lld blocks, %llu sequences, %llu bases, %llu windows kept, %llu distinct, %u folds, %u batches run again: feed %.3f s, finish %.3f s\n",
                path, fed.route, (long long)fed.blocks, (unsigned long long)st.nseq, (unsigned long long)st.nbases, (unsigned long long)st.kept, (unsigned long long)st.distinct,
                st.folds, st.retries, fed.t1 - fed.t0, now_s() - fed.t1);
    CKE(rk_sample_reset(sample), path);
}
