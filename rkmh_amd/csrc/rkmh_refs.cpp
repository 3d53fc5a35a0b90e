// rkmh_refs.cpp -- the -r files through the device (plain, gzip and BGZF FASTA) instead of the host parser.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>

#include "rkmh_cli.hpp"

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
            if (!pread_full(fds[jb.file], text, jb.hi - jb.lo, jb.lo)) { fprintf(stderr, "rkmh: read error on %s\n", o.refs[jb.file]); fail_exit(); }
            uint64_t nbytes = (uint64_t)(jb.hi - jb.lo);
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
        if (rc < 0) die();
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
