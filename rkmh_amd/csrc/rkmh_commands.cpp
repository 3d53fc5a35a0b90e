// rkmh_commands.cpp -- the sub-commands of `rkmh` beside stream / filter: pack, call, sketch (and the JSON sketches stream -R reads),
// dist, gather, hash and hpv16; the hashing policy of the run and the help text they share.
#include <unistd.h>

#include <algorithm>
#include <set>

#include "rkmh_cli.hpp"
#include <cerrno>

// The hashing policy of this run: the build's defaults, then RKMH_POLICY, then --hash-policy (rk_policy_parse: presets `default`
// `mash` and `sourmash`, or fold= / windows= / zero= / mask= / freqmax= / canon= / dedup= / seed=).  The arithmetic behind these switches is mkmh's, which the
// reference's tree does not hold (src/rkmh.cpp:17); every context of the process is created with g_policy.
rk_policy g_policy;
void policy_apply(const char* spec, const char* from) {
    if (rk_policy_parse(spec, &g_policy) != RK_OK) { fprintf(stderr, "rkmh: %s: %s\n", from, rk_last_error()); exit(1); }
}
std::string policy_text(const rk_policy& p) {
    char b[160];
    if (rk_policy_describe(&p, b, sizeof b) < 0) { fprintf(stderr, "rkmh: %s\n", rk_last_error()); exit(1); }
    return b;
}

void print_help() {
    fprintf(stderr,
            "rkmh (MI355X build): MinHash read classification on AMD Instinct GPUs\n"
            "Usage: rkmh <command> [options]\n"
            "  classify / stream   classify reads against a set of references\n"
            "  filter              print the reads that match a reference (or classify reads arriving on STDIN)\n"
            "  call                call SNPs / 1-bp deletions from k-mer depth along a reference\n"
            "  hash                print the k-mer hashes of every sequence\n"
            "  hpv16               HPV type and HPV16 lineage / sublineage k-mer matches of every read\n"
            "  sketch              write MinHash sketches as JSON (load them with stream -R); --scaled: scaled (FracMinHash) sketches for dist\n"
            "  dist                Mash distance between every query sketch and every reference sketch; --scaled: Jaccard and containment of scaled sketches\n"
            "  gather              decompose a sample's scaled sketch into references, greedily: what each explains once the better matches are taken out\n"
            "  pack                write reads as a packed file (2 bits per base + names): stream|filter -F <file> classifies it without parsing\n"
            "Run a command without options for its help text.\n");
}
static void help_hash() {
    fprintf(stderr,
            "rkmh hash -f <seqs.fa|fq> [-k <k>]... [--hash-policy <spec>]\n"
            "  prints one line per sequence: name, then every k-mer hash, tab separated\n" HASH_POLICY_HELP);
}

// ------------------------------------------------------------------------------------------------------------------------
// Packed reads: `rkmh pack` writes them, `stream|filter -F` reads them (include/rkmh_amd.h, "PACKED READS").  The reference parses
// -F/--pre-reads and does nothing with it (src/rkmh.cpp:659-664); here it names reads that were parsed ONCE: 2 bits per base, the
// names and (optionally) the quality strings kept for the host -- a run then moves ~42 bytes per 150-base read over the link
// instead of 315 of FASTQ text, parses nothing, and formats its lines from the names where they lie in the mapped file.
static void help_pack() {
    fprintf(stderr,
            "rkmh pack -f <reads.fq|fa[.gz]> [-f ...] -o <out.rkp> [--no-quals] [--block-reads <n>]\n"
            "  writes the reads as a packed file (2 bits per base, names, quality strings unless --no-quals) that\n"
            "  `rkmh stream|filter -F <out.rkp>` classifies without parsing; independent of k, sketch size and hashing policy\n");
}
int main_pack(int argc, char** argv) {
    std::vector<const char*> files;
    const char* outp = nullptr;
    bool keep_quals = true;
    long block_reads = 1 << 20;
    if (argc <= 2) { help_pack(); exit(1); }
    static struct option long_options[] = {{"help", no_argument, 0, 'h'}, {"fasta", required_argument, 0, 'f'}, {"output", required_argument, 0, 'o'},
                                           {"no-quals", no_argument, 0, 1010}, {"block-reads", required_argument, 0, 1011}, {"threads", required_argument, 0, 't'}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hf:o:t:", long_options, nullptr)) != -1) {
        switch (c) {
            case 'f': files.push_back(optarg); break;
            case 'o': outp = optarg; break;
            case 't': break;
            case 1010: keep_quals = false; break;
            case 1011: block_reads = atol(optarg); break;
            default: help_pack(); exit(1);
        }
    }
    if (files.empty() || !outp) { help_pack(); exit(1); }
    if (block_reads < 1024 || block_reads > (16 << 20)) { fprintf(stderr, "rkmh pack: --block-reads must lie between 1024 and 16777216\n"); exit(1); }
    FILE* fo = fopen(outp, "wb");
    if (!fo) { fprintf(stderr, "rkmh pack: cannot write %s\n", outp); exit(1); }
    rk_packed_header hdr;
    memset(&hdr, 0, sizeof hdr);
    memcpy(hdr.magic, RK_PACKED_MAGIC, 8);
    hdr.version = 1;
    std::vector<rk_packed_block> dir;
    uint64_t at = 0;
    bool quals_everywhere = keep_quals;
    auto put = [&](const void* p, size_t n) { if (n && fwrite(p, 1, n, fo) != n) { fprintf(stderr, "rkmh pack: write error on %s\n", outp); exit(1); } at += n; };
    auto align16 = [&]() { static const char z[16] = {0}; const size_t pad = (size_t)((16 - (at & 15)) & 15); put(z, pad); };
    put(&hdr, sizeof hdr); // (rewritten at the end)
    const int nt = std::max(1, std::min(granted_cpus_main(), 16));
    std::vector<uint8_t> b2;
    std::vector<std::vector<rk_packed_exception>> exc_t((size_t)nt);
    std::vector<uint32_t> offs, noffs;
    std::vector<char> names;
    for (const char* path : files) {
        rk_reader* rd = nullptr;
        CK(rk_reader_open(path, &rd));
        if (!keep_quals) rk_reader_set_options(rd, RK_READER_NO_QUALS);
        for (;;) {
            rk_seqset s;
            CK(rk_reader_next(rd, block_reads, (uint64_t)3 << 30, &s));
            if (s.nseq == 0) { rk_seqset_free(&s); break; }
            const uint64_t b0 = s.offsets[0], nb = s.offsets[s.nseq] - b0;
            if (nb >= ((uint64_t)1 << 32) - 64 || s.nseq > 0x7ffffff0ll) { fprintf(stderr, "rkmh pack: a block of more than 4 G bases\n"); exit(1); }
            rk_packed_block blk;
            memset(&blk, 0, sizeof blk);
            blk.nrec = (uint32_t)s.nseq; blk.nbases = nb;
            offs.resize((size_t)s.nseq + 1);
            uint32_t maxlen = 0;
            for (int64_t i = 0; i <= s.nseq; ++i) offs[(size_t)i] = (uint32_t)(s.offsets[i] - b0);
            for (int64_t i = 0; i < s.nseq; ++i) maxlen = std::max(maxlen, offs[(size_t)i + 1] - offs[(size_t)i]);
            blk.max_len = maxlen;
            // 2-bit bases and exceptions: pieces of whole bytes (4 bases), a thread each
            b2.assign((size_t)((nb + 3) / 4), 0);
            {
                std::vector<std::thread> th;
                const uint64_t per = (((nb + (uint64_t)nt - 1) / (uint64_t)nt) + 3) & ~(uint64_t)3;
                for (int t = 0; t < nt; ++t)
                    th.emplace_back([&, t] {
                        const uint64_t lo = std::min(nb, per * (uint64_t)t), hi = std::min(nb, lo + per);
                        auto& ex = exc_t[(size_t)t];
                        ex.resize((size_t)(hi - lo) + 1);
                        const int64_t ne = rk_packed_encode(s.bases + b0 + lo, hi - lo, lo, b2.data() + lo / 4, ex.data(), ex.size());
                        if (ne < 0) { fprintf(stderr, "rkmh pack: %s\n", rk_last_error()); fail_exit(); }
                        ex.resize((size_t)ne);
                    });
                for (auto& t : th) t.join();
            }
            noffs.resize((size_t)s.nseq + 1);
            names.clear();
            for (int64_t i = 0; i < s.nseq; ++i) {
                noffs[(size_t)i] = (uint32_t)names.size();
                const char* nm = s.names + s.name_offsets[i];
                names.insert(names.end(), nm, nm + (s.name_offsets[i + 1] - s.name_offsets[i] - 1)); // (the offsets include the NUL)
            }
            noffs[(size_t)s.nseq] = (uint32_t)names.size();
            if (names.size() >= ((uint64_t)1 << 32)) { fprintf(stderr, "rkmh pack: more than 4 GB of names in one block\n"); exit(1); }
            blk.name_bytes = names.size();
            align16(); blk.offsets_off = at; put(offs.data(), offs.size() * 4);
            align16(); blk.bases_off = at; put(b2.data(), b2.size());
            { static const char z[16] = {0}; put(z, 16); } // (the bases are uploaded in whole dwords; the unpacked tail is never read)
            align16(); blk.exc_off = at;
            uint64_t nexc = 0;
            for (auto& ex : exc_t) { put(ex.data(), ex.size() * sizeof(rk_packed_exception)); nexc += ex.size(); }
            if (nexc > 0xffffffffull) { fprintf(stderr, "rkmh pack: too many non-ACGT bases in one block\n"); exit(1); }
            blk.nexc = (uint32_t)nexc;
            align16(); blk.name_offsets_off = at; put(noffs.data(), noffs.size() * 4);
            align16(); blk.names_off = at; put(names.data(), names.size());
            { static const char z[32] = {0}; put(z, 32); } // (the formatters copy names in 16-byte steps)
            if (keep_quals && s.quals) { align16(); blk.quals_off = at; put(s.quals + b0, (size_t)nb); }
            else quals_everywhere = false;
            dir.push_back(blk);
            hdr.nreads += (uint64_t)s.nseq; hdr.nbases += nb;
            rk_seqset_free(&s);
        }
        rk_reader_close(rd);
    }
    if (!quals_everywhere) for (auto& b : dir) b.quals_off = 0; // (all or nothing: a file that keeps qualities keeps them for every read)
    align16();
    hdr.directory_off = at; hdr.nblocks = dir.size(); hdr.flags = quals_everywhere && !dir.empty() ? RK_PACKED_QUALS : 0u;
    put(dir.data(), dir.size() * sizeof(rk_packed_block));
    { static const char z[64] = {0}; put(z, 64); }
    if (fseek(fo, 0, SEEK_SET) != 0 || fwrite(&hdr, sizeof hdr, 1, fo) != 1 || fclose(fo) != 0) { fprintf(stderr, "rkmh pack: write error on %s\n", outp); exit(1); }
    fprintf(stderr, "rkmh pack: %llu reads, %llu bases in %zu blocks%s -> %s (%.1f bytes per read)\n", (unsigned long long)hdr.nreads, (unsigned long long)hdr.nbases, dir.size(),
            hdr.flags & RK_PACKED_QUALS ? ", with qualities" : "", outp, hdr.nreads ? (double)(at + dir.size() * sizeof(rk_packed_block)) / (double)hdr.nreads : 0.0);
    return 0;
}

// call: main_call, src/rkmh.cpp:1455-1904.  The GPU returns one record per candidate k-mer that passed the depth
// tests; the VCF rows are the records aggregated by (ref, pos, orig, alt) exactly as rkmh.cpp:1821-1829 / :1856-1863.
static void help_call() {
    fprintf(stderr,
            "rkmh call -r <ref.fa> -f <reads.fq> [-k <k>] [-w <window>]\n"
            "  calls SNPs and 1-bp deletions from the k-mer depth of the reads along the reference (VCF-like rows)\n" HASH_POLICY_HELP);
}
int main_call(int argc, char** argv) {
    std::vector<const char*> refs, reads;
    std::vector<int> ks;
    int window_len = 100, device = 0;
    bool show_depth = false;
    if (argc <= 2) { help_call(); exit(1); }
    static struct option long_options[] = {
        {"help", no_argument, 0, 'h'},        {"kmer", required_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'}, {"reference", required_argument, 0, 'r'},
        {"sketch", required_argument, 0, 's'}, {"threads", required_argument, 0, 't'},
        {"window-len", required_argument, 0, 'w'}, {"show-depth", no_argument, 0, 'd'},
        {"device", required_argument, 0, 1000}, HASH_POLICY_OPTION, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hdk:f:r:s:t:w:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 'r': refs.push_back(optarg); break;
            case 'f': reads.push_back(optarg); break;
            case 'k': ks.push_back(atoi(optarg)); break;
            case 'w': window_len = atoi(optarg); break;
            case 'd': show_depth = true; break;             // sets show_depth, clears output_vcf: prints nothing (Appendix A.3)
            case 's': case 't': break;                        // parsed, unused
            case 1000: device = atoi(optarg); break;
            case '?': case 'h': default: print_help(); exit(1);
        }
    }
    if (ks.empty()) {
        fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n");
        ks.push_back(16);
    } else if (ks.size() > 1) {                               // rkmh.cpp:1543-1552
        fprintf(stderr, "Only a single kmer size may be used for calling.\nSizes provided: ");
        for (int k : ks) fprintf(stderr, "%d ", k);
        fprintf(stderr, "\nPlease choose a single kmer size.\n");
        exit(1);
    }
    fprintf(stderr, "Parsing sequences...\n");
    if (refs.empty()) {
        fprintf(stderr, "No references were provided. Please provide at least one reference file in fasta/fastq format.\n");
        help_call(); exit(1);
    }
    if (reads.empty()) {
        fprintf(stderr, "No reads were provided. Please provide at least one read file in fasta/fastq format.\n");
        help_call(); exit(1);
    }
    rk_seqset R, Q;
    CK(rk_parse_files(refs.data(), (int)refs.size(), &R));
    CK(rk_parse_files(reads.data(), (int)reads.size(), &Q));
    if (R.nseq < 1) { fprintf(stderr, "rkmh: no reference sequences found\n"); exit(1); }
    if (R.nseq > 1) fprintf(stderr, "WARNING: more than one ref provided. VCF will not be correct\n");
    if (show_depth) return 0;
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    rk_call_record* rec = nullptr;
    int64_t nrec = 0;
    CK(rk_call(ctx, R.bases, R.offsets, (int)R.nseq, Q.bases, Q.offsets, Q.nseq, ks[0], window_len, &rec, &nrec));
    printf("##fileformat=VCF4.2\n##source=rkmh\n##reference=%s\n"
           "##INFO=<ID=KD,Number=1,Type=Integer,Description=\"Number of times call for specific kmer appears\">\n"
           "##INFO=<ID=MD,Number=1,Type=Integer,Description=\"Maximum depth found for the rescue kmer.\">\n"
           "##INFO=<ID=RD,Number=1,Type=Integer,Description=\"Average depth in region\">"
           "##INFO=<ID=OD,Number=1,Type=Integer,Description=\"Depth of original kmer at site before modification.\">\n", refs[0]);
    struct Agg { int kc = 0, md = 0, rd = 0, od = 0; };
    std::map<std::string, Agg> rows; // lexicographic key order, as the reference's std::map (rkmh.cpp:1885)
    char key[4096];
    for (int64_t i = 0; i < nrec; ++i) {
        const rk_call_record& r = rec[i];
        snprintf(key, sizeof key, "%s\t%d\t.\t%c\t%c", R.names + R.name_offsets[r.ref], r.pos, (char)r.orig, (char)r.alt);
        Agg& a = rows[key];
        a.kc += 1;
        if (r.alt_depth > a.md) a.md = r.alt_depth;
        if (r.avg_d > a.rd) a.rd = r.avg_d;
        if (r.depth > a.od) a.od = r.depth;
    }
    for (auto& kv : rows) printf("%s\t99\tPASS\tKC=%d;MD=%d;RD=%d;OD=%d\n", kv.first.c_str(), kv.second.kc, kv.second.md, kv.second.rd, kv.second.od);
    fflush(stdout);
    rk_free(rec);
    rk_seqset_free(&R); rk_seqset_free(&Q);
    rk_ctx_destroy(ctx);
    return 0;
}

// ---- JSON sketches (the schema of dump_hash_json, src/rkmh.cpp:489-525; dead code in the reference, kept here as the
// interchange format SURVEY.md section 8f ranks next).  Keys are emitted in the alphabetical order nlohmann::json uses.
static void json_escape(std::string& out, const char* s) {
    for (; *s; ++s) {
        unsigned char ch = (unsigned char)*s;
        if (ch == '"' || ch == '\\') { out += '\\'; out += (char)ch; }
        else if (ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); out += b; }
        else out += (char)ch;
    }
}
static void help_sketch() {
    fprintf(stderr,
            "rkmh sketch -f <seqs.fa|fq> [-k <k>]... [-s <sketch> | --scaled <n>] [-g] [-o <out.json>] [--kmer-cache <file>]\n"
            "  writes a JSON array with one MinHash sketch per sequence (schema of the reference's dump_hash_json);\n"
            "  -g: one sketch per input FILE (named by its path; no k-mer spans two of its records), as Mash sketches an assembly;\n"
            "  --scaled <n>: scaled (FracMinHash) sketches instead of bottom-s ones: every distinct hash up to (2^64 - 1) / n, so the size\n"
            "  grows with the sequence; objects gain \"scaled\" and \"maxHash\"; such files serve `rkmh dist` only\n"
            "  `rkmh stream -R <out.json>` loads it instead of sketching references again;\n"
            "  --kmer-cache <file>: also enumerates the k-mers behind these sketches (k 8 .. 18) into <file>, which\n"
            "  `rkmh stream -R <out.json> --kmer-cache <file>` then loads instead of enumerating them at every start\n"
            "  the file records the hashing policy (\"hashPolicy\"); stream -R refuses sketches hashed under another one\n" HASH_POLICY_HELP);
}
// The sketches `sketch` writes and `dist` compares, one per sequence of the files -- or, whole_files (-g), one per FILE: the records
// of a file are sketched one by one (no window spans two contigs) and reduced to the bottom S of their union under the policy's dedup
// rule (rk_merge_sketches); such a sketch is named by the path as given and its seqLen is the sum of the record lengths.
struct SketchSet { std::vector<std::string> names; std::vector<uint64_t> seq_len; std::vector<uint64_t> sk; std::vector<int32_t> lens; };
static void sketch_files(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, int S, bool whole_files, SketchSet& out) {
    auto sketch_records = [&](const rk_seqset& s, std::vector<uint64_t>& sk, std::vector<int32_t>& lens) {
        sk.assign((size_t)s.nseq * (size_t)S, 0);
        lens.assign((size_t)s.nseq, 0);
        CK(rk_sketch_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), S, sk.data(), lens.data()));
    };
    if (!whole_files) {
        rk_seqset s;
        CK(rk_parse_files(files.data(), (int)files.size(), &s));
        sketch_records(s, out.sk, out.lens);
        for (int64_t i = 0; i < s.nseq; ++i) {
            out.names.push_back(s.names + s.name_offsets[i]);
            out.seq_len.push_back(s.offsets[i + 1] - s.offsets[i]);
        }
        rk_seqset_free(&s);
        return;
    }
    out.sk.assign(files.size() * (size_t)S, 0);
    out.lens.assign(files.size(), 0);
    std::vector<uint64_t> sk;
    std::vector<int32_t> lens;
    for (size_t f = 0; f < files.size(); ++f) {
        rk_seqset s;
        CK(rk_parse_files(&files[f], 1, &s));
        if (s.nseq > 0x7fffffffll) { fprintf(stderr, "rkmh: %s holds more than 2^31-1 records\n", files[f]); exit(1); }
        sketch_records(s, sk, lens);
        CK(rk_merge_sketches(sk.data(), lens.data(), (int)s.nseq, S, rk_policy_dedup(&g_policy), &out.sk[f * (size_t)S], &out.lens[f]));
        out.names.push_back(files[f]);
        out.seq_len.push_back(s.nseq ? s.offsets[s.nseq] - s.offsets[0] : 0);
        rk_seqset_free(&s);
    }
}
// --scaled: a number of at least 1, nothing else
static bool parse_scaled(const char* text, uint64_t& scaled) {
    if (!text || !isdigit((unsigned char)*text)) return false;
    char* e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(text, &e, 10);
    if (errno != 0 || *e != 0 || v == 0) return false;
    scaled = (uint64_t)v;
    return true;
}
// Scaled sketches as `sketch --scaled` writes and `dist --scaled` compares them: CSR, sketch i = values[off[i], off[i + 1]).  One per
// sequence of the files -- or, whole_files (-g), one per FILE: its records are sketched one by one and united (rk_merge_scaled).
struct ScaledSet { std::vector<std::string> names; std::vector<uint64_t> seq_len; std::vector<uint64_t> values; std::vector<uint64_t> off = std::vector<uint64_t>(1, 0); };
static void sketch_files_scaled(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, uint64_t max_hash, bool whole_files, ScaledSet& out) {
    auto sketch_records = [&](const rk_seqset& s, uint64_t** v, std::vector<uint64_t>& off) {
        off.assign((size_t)s.nseq + 1, 0);
        CK(rk_sketch_scaled_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), max_hash, v, off.data()));
    };
    std::vector<uint64_t> off;
    if (!whole_files) {
        rk_seqset s;
        CK(rk_parse_files(files.data(), (int)files.size(), &s));
        uint64_t* v = nullptr;
        sketch_records(s, &v, off);
        for (int64_t i = 0; i < s.nseq; ++i) {
            out.names.push_back(s.names + s.name_offsets[i]);
            out.seq_len.push_back(s.offsets[i + 1] - s.offsets[i]);
            out.values.insert(out.values.end(), v + off[(size_t)i], v + off[(size_t)i + 1]);
            out.off.push_back(out.values.size());
        }
        rk_free(v);
        rk_seqset_free(&s);
        return;
    }
    for (size_t f = 0; f < files.size(); ++f) {
        rk_seqset s;
        CK(rk_parse_files(&files[f], 1, &s));
        if (s.nseq > 0x7fffffffll) { fprintf(stderr, "rkmh: %s holds more than 2^31-1 records\n", files[f]); exit(1); }
        uint64_t* v = nullptr;
        sketch_records(s, &v, off);
        uint64_t* u = nullptr;
        uint64_t nu = 0;
        CK(rk_merge_scaled(v, off.data(), (int)s.nseq, max_hash, &u, &nu));
        out.names.push_back(files[f]);
        out.seq_len.push_back(s.nseq ? s.offsets[s.nseq] - s.offsets[0] : 0);
        out.values.insert(out.values.end(), u, u + nu);
        out.off.push_back(out.values.size());
        rk_free(u);
        rk_free(v);
        rk_seqset_free(&s);
    }
}
int main_sketch(int argc, char** argv) {
    std::vector<const char*> files;
    std::vector<int> ks;
    int S = 1000, device = 0;
    const char* outp = nullptr;
    const char* kmer_cache = nullptr;
    bool whole_files = false, s_given = false, scaled_given = false, scaled_ok = true;
    uint64_t scaled = 0;
    if (argc <= 2) { help_sketch(); exit(1); }
    optind = 2;
    int c;
    static struct option long_options[] = {{"help", no_argument, 0, 'h'}, {"kmer", required_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'}, {"reference", required_argument, 0, 'r'}, {"sketch-size", required_argument, 0, 's'},
        {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1000}, {"kmer-cache", required_argument, 0, 1003},
        {"whole-files", no_argument, 0, 'g'}, {"scaled", required_argument, 0, 1005}, HASH_POLICY_OPTION, {0, 0, 0, 0}};
    while ((c = getopt_long(argc, argv, "hgk:f:r:s:o:t:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 1005: scaled_given = true; scaled_ok = parse_scaled(optarg, scaled); break;
            case 1003: kmer_cache = optarg; break;
            case 'g': whole_files = true; break;
            case 'f': case 'r': files.push_back(optarg); break;
            case 'k': ks.push_back(atoi(optarg)); break;
            case 's': S = atoi(optarg); s_given = true; break;
            case 'o': outp = optarg; break;
            case 't': break;
            case 1000: device = atoi(optarg); break;
            default: help_sketch(); exit(1);
        }
    }
    if (ks.empty()) { fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n"); ks.push_back(16); }
    if (files.empty()) { fprintf(stderr, "rkmh: -f <file> is required\n"); exit(1); }
    if (scaled_given) {
        if (!scaled_ok) { fprintf(stderr, "rkmh sketch: --scaled takes a number of at least 1\n"); exit(1); }
        if (s_given) { fprintf(stderr, "rkmh sketch: --scaled and -s are two kinds of sketch; give one of them\n"); exit(1); }
        if (kmer_cache) { fprintf(stderr, "rkmh sketch: --kmer-cache serves `stream -R`; scaled sketches serve `rkmh dist` only\n"); exit(1); }
    }
    if (!scaled_given && whole_files && (S < 1 || S > RK_MAX_SKETCH)) { fprintf(stderr, "rkmh sketch: -g needs a sketch size of 1 .. %d\n", RK_MAX_SKETCH); exit(1); }
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    if (scaled_given) {
        uint64_t max_hash = 0;
        CK(rk_scaled_max_hash(scaled, &max_hash));
        ScaledSet set;
        sketch_files_scaled(ctx, files, ks, max_hash, whole_files, set);
        FILE* fo = outp ? fopen(outp, "w") : stdout;
        if (!fo) { fprintf(stderr, "rkmh: cannot write %s\n", outp); exit(1); }
        std::string kstr;
        for (size_t i = 0; i < ks.size(); ++i) { kstr += std::to_string(ks[i]); if (i + 1 < ks.size()) kstr += ' '; }
        const std::string pol_text = policy_text(g_policy);
        std::string o = "[";
        char num[32];
        // today's keys in their alphabetical places, plus "maxHash" and "scaled"; "length" is the sketch's own number of hashes
        for (size_t i = 0; i < set.names.size(); ++i) {
            std::string name;
            json_escape(name, set.names[i].c_str());
            if (i) o += ',';
            o += "{\"alphabet\":\"ATGC\",\"canonical\":\"true\",\"hashBits\":64,\"hashPolicy\":\"" + pol_text + "\",\"hashSeed\":" + std::to_string(g_policy.seed) +
                 ",\"hashType\":\"MurmurHash3_x64_128\",\"kmer\":\"" + kstr + "\",\"maxHash\":" + std::to_string(max_hash) +
                 ",\"name\":\"" + name + "\",\"preserveCase\":\"false\",\"scaled\":" + std::to_string(scaled) + ",\"seqLen\":" + std::to_string(set.seq_len[i]) +
                 ",\"sketches\":{\"comment\":\"\",\"hashes\":[";
            for (uint64_t j = set.off[i]; j < set.off[i + 1]; ++j) {
                int n = snprintf(num, sizeof num, j > set.off[i] ? ",%llu" : "%llu", (unsigned long long)set.values[(size_t)j]);
                o.append(num, (size_t)n);
            }
            o += "],\"length\":" + std::to_string(set.off[i + 1] - set.off[i]) + ",\"name\":\"" + name + "\"}}";
            if (o.size() > (1u << 22)) { fwrite(o.data(), 1, o.size(), fo); o.clear(); }
        }
        o += "]\n";
        fwrite(o.data(), 1, o.size(), fo);
        if (fo != stdout) fclose(fo);
        rk_ctx_destroy(ctx);
        return 0;
    }
    SketchSet set;
    sketch_files(ctx, files, ks, S, whole_files, set);
    const std::vector<uint64_t>& sk = set.sk;
    const std::vector<int32_t>& lens = set.lens;
    const int64_t nsk = (int64_t)set.names.size();
    if (kmer_cache && *kmer_cache) {
        // the index of these sketches is built once here, for its k-mer enumeration: the file's tag hashes the index keys, k and the
        // hashing policy, so a later `stream -R <these sketches> --kmer-cache <file>` finds it -- and anything else does not use it
        CK(rk_set_kmer_cache(ctx, kmer_cache));
        CK(rk_set_reference_sketches(ctx, sk.data(), lens.data(), (int)nsk, ks.data(), (int)ks.size(), S));
        if (rk_kmer_cache_state(ctx) == 0) fprintf(stderr, "rkmh: no k-mer enumeration for these sketches (k-mer sizes outside 8 .. 18, or a hash with two k-mers): %s not written\n", kmer_cache);
    }
    FILE* fo = outp ? fopen(outp, "w") : stdout;
    if (!fo) { fprintf(stderr, "rkmh: cannot write %s\n", outp); exit(1); }
    std::string kstr;
    for (size_t i = 0; i < ks.size(); ++i) { kstr += std::to_string(ks[i]); if (i + 1 < ks.size()) kstr += ' '; }
    std::string o = "[";
    char num[32];
    // "hashPolicy": this build's addition to dump_hash_json's keys (src/rkmh.cpp:489-525) -- what hashType / hashSeed leave open
    const std::string pol_text = policy_text(g_policy);
    for (int64_t i = 0; i < nsk; ++i) {
        std::string name;
        json_escape(name, set.names[(size_t)i].c_str());
        if (i) o += ',';
        o += "{\"alphabet\":\"ATGC\",\"canonical\":\"true\",\"hashBits\":64,\"hashPolicy\":\"" + pol_text + "\",\"hashSeed\":" + std::to_string(g_policy.seed) +
             ",\"hashType\":\"MurmurHash3_x64_128\",\"kmer\":\"" + kstr +
             "\",\"name\":\"" + name + "\",\"preserveCase\":\"false\",\"seqLen\":" + std::to_string(set.seq_len[(size_t)i]) +
             ",\"sketches\":{\"comment\":\"\",\"hashes\":[";
        for (int j = 0; j < lens[(size_t)i]; ++j) {
            int n = snprintf(num, sizeof num, j ? ",%llu" : "%llu", (unsigned long long)sk[(size_t)i * S + j]);
            o.append(num, (size_t)n);
        }
        o += "],\"length\":" + std::to_string(S) + ",\"name\":\"" + name + "\"}}";
        if (o.size() > (1u << 22)) { fwrite(o.data(), 1, o.size(), fo); o.clear(); }
    }
    o += "]\n";
    fwrite(o.data(), 1, o.size(), fo);
    if (fo != stdout) fclose(fo);
    rk_ctx_destroy(ctx);
    return 0;
}

// minimal reader for the files written above (tolerates whitespace; no general JSON support is claimed)
static bool json_find(const std::string& t, size_t from, size_t to, const char* key, size_t& vpos) {
    std::string pat = std::string("\"") + key + "\"";
    size_t p = t.find(pat, from);
    if (p == std::string::npos || p >= to) return false;
    p = t.find(':', p + pat.size());
    if (p == std::string::npos || p >= to) return false;
    ++p;
    while (p < to && isspace((unsigned char)t[p])) ++p;
    vpos = p;
    return true;
}
static std::string json_string_at(const std::string& t, size_t p) {
    std::string r;
    if (t[p] != '"') return r;
    for (++p; p < t.size() && t[p] != '"'; ++p) {
        if (t[p] == '\\' && p + 1 < t.size()) { ++p; r += t[p]; } else r += t[p];
    }
    return r;
}
bool load_sketch_json(const char* path, LoadedSketches& L, int max_S) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::string t;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) t.append(buf, n);
    fclose(f);
    // objects are delimited by their "sketches":{...}} tail; walk by the "alphabet" key that opens each object
    size_t pos = 0;
    std::vector<std::vector<uint64_t>> all;
    while ((pos = t.find("\"alphabet\"", pos)) != std::string::npos) {
        size_t next = t.find("\"alphabet\"", pos + 10);
        size_t end = next == std::string::npos ? t.size() : next;
        size_t v;
        if (!json_find(t, pos, end, "kmer", v)) return false;
        std::vector<int> ks;
        { std::string kk = json_string_at(t, v); char* e = &kk[0]; while (*e) { while (*e == ' ') ++e; if (!*e) break; ks.push_back((int)strtol(e, &e, 10)); } }
        if (L.ks.empty()) L.ks = ks; else if (ks != L.ks) return false;
        { // the policy the sketches were hashed under (absent: a file of an earlier build, which knew the defaults only)
            std::string pol = "default";
            if (json_find(t, pos, end, "hashPolicy", v)) pol = json_string_at(t, v);
            if (L.names.empty()) L.policy = pol; else if (pol != L.policy) return false;
        }
        size_t sp;
        if (!json_find(t, pos, end, "sketches", sp)) return false;
        // "scaled" / "maxHash" (`sketch --scaled`): all objects of a file or none, and all the same
        uint64_t scaled = 0, max_hash = 0;
        if (json_find(t, pos, sp, "scaled", v)) {
            scaled = strtoull(t.c_str() + v, nullptr, 10);
            uint64_t expect = 0;
            if (scaled == 0 || !json_find(t, pos, sp, "maxHash", v) || rk_scaled_max_hash(scaled, &expect) != RK_OK ||
                (max_hash = strtoull(t.c_str() + v, nullptr, 10)) != expect) {
                L.err = "sketch " + std::to_string(all.size()) + ": \"scaled\" must be at least 1 and \"maxHash\" = (2^64 - 1) / scaled";
                return false;
            }
        }
        if (!all.empty() && scaled != L.scaled) { L.err = "its sketches disagree in scaled"; return false; }
        L.scaled = scaled;
        if (!json_find(t, pos, end, "name", v)) return false;
        L.names.push_back(json_string_at(t, v));
        if (!json_find(t, sp, end, "length", v)) return false;
        int S = (int)strtol(t.c_str() + v, nullptr, 10);
        if (scaled) S = 0; // (a scaled sketch's "length" is its own number of hashes)
        else if (L.S == 0) L.S = S; else if (S != L.S) return false;
        if (!json_find(t, sp, end, "hashes", v)) return false;
        std::vector<uint64_t> h;
        const char* q = t.c_str() + v;
        if (*q != '[') return false;
        ++q;
        for (;;) {
            while (*q && (isspace((unsigned char)*q) || *q == ',')) ++q;
            if (*q == ']' || !*q) break;
            char* e;
            h.push_back(strtoull(q, &e, 10));
            if (e == q) return false;
            q = e;
        }
        if (scaled)
            for (size_t j = 0; j < h.size(); ++j)
                if (h[j] == 0 || h[j] > max_hash || (j && h[j] <= h[j - 1])) {
                    L.err = "sketch " + std::to_string(all.size()) + ": the hashes of a scaled sketch are ascending, distinct and at most its maxHash";
                    return false;
                }
        all.push_back(h);
        pos = end;
    }
    if (!all.empty() && L.scaled) {
        L.off.assign(1, 0);
        for (const auto& h : all) {
            if (h.size() > 0x7fffffffull) return false;
            L.lens.push_back((int32_t)h.size());
            L.sk.insert(L.sk.end(), h.begin(), h.end());
            L.off.push_back(L.sk.size());
        }
        return true;
    }
    if (all.empty() || L.S <= 0) return false;
    if (max_S > 0 && L.S > max_S) return false; // (before the rows are allocated: L.S tells the caller why)
    L.sk.assign(all.size() * (size_t)L.S, 0);
    for (size_t i = 0; i < all.size(); ++i) {
        if ((int)all[i].size() > L.S) return false;
        L.lens.push_back((int32_t)all[i].size());
        for (size_t j = 0; j < all[i].size(); ++j) L.sk[i * (size_t)L.S + j] = all[i][j];
    }
    return true;
}

void refuse_scaled(const LoadedSketches& L, const char* path, const char* command) {
    if (!L.scaled) return;
    fprintf(stderr, "rkmh: %s holds scaled sketches (scaled = %llu); scaled sketches serve `rkmh dist`, not %s, which needs bottom-s sketches\n", path,
            (unsigned long long)L.scaled, command);
    exit(1);
}

// ------------------------------------------------------------------------------------------------------------------------
// dist: the Mash distance of every (query, reference) pair of sketches -- `mash dist`, which the reference has no command for.  The
// four counts of a pair come from one launch over all pairs (rk_compare_sketches); the floating point is rk_mash_distance's.
// Everything that can be refused is refused before a context exists: nothing is printed by a run that fails.
// A loaded file of scaled sketches, kept at its own "scaled" until the run's value is known (dist, gather), and the cut down to it: a
// prefix of every row, because rows ascend and max_hash is monotone in scaled.
struct ScaledFile { std::string path; LoadedSketches L; };
static void cut_scaled_files(const std::vector<ScaledFile>& from, uint64_t max_hash, ScaledSet& into) {
    for (const ScaledFile& f : from)
        for (size_t i = 0; i < f.L.names.size(); ++i) {
            const uint64_t* b = f.L.sk.data() + f.L.off[i];
            const uint64_t* e = std::upper_bound(b, f.L.sk.data() + f.L.off[i + 1], max_hash);
            into.names.push_back(f.L.names[i]);
            into.values.insert(into.values.end(), b, e);
            into.off.push_back(into.values.size());
        }
}
static void help_dist() {
    fprintf(stderr,
            "rkmh dist (-r <refs.fa> ... | -R <refs.json>) [-f <queries.fa|fq> ... | -Q <queries.json>] [-k <k>] [-s <sketch> | --scaled <n>] [-g] [-d <maxdist>]\n"
            "  prints one line per (query, reference) pair, query by query: reference, query, Mash distance, common/denom of the merged\n"
            "  bottom-s sketch, shared hashes (the multiset intersection `stream` counts); without -f / -Q every reference is compared\n"
            "  with every reference\n"
            "  -R / -Q: sketches written by `rkmh sketch` (their k-mer size, sketch size and hashing policy must agree with each other and the run)\n"
            "  --scaled <n>: compare scaled (FracMinHash) sketches, every distinct hash up to (2^64 - 1) / n: -r / -f files are sketched at n,\n"
            "  -R / -Q files hold sketches of `rkmh sketch --scaled <m>`, m <= n, and are cut down to n (without --scaled: to the largest m\n"
            "  among them); a line is then: reference, query, distance from shared/union, shared/union, shared/|query|, shared/|reference|\n"
            "  (the last two: how much of the query is contained in the reference, and the reverse); not with -s\n"
            "  -g: one sketch per input FILE, as Mash sketches an assembly;  -d <x>: only pairs at distance <= x;  --device <id>: GPU to use\n" HASH_POLICY_HELP);
}
int main_dist(int argc, char** argv) {
    std::vector<const char*> ref_files, query_files, ref_json, query_json;
    std::vector<int> ks;
    int S = 0, device = 0;
    bool whole_files = false, scaled_given = false, scaled_ok = true;
    uint64_t scaled = 0; // --scaled, or the largest "scaled" of the files loaded
    double max_dist = 2.0;
    if (argc <= 2) { help_dist(); exit(1); }
    static struct option long_options[] = {{"help", no_argument, 0, 'h'}, {"kmer", required_argument, 0, 'k'}, {"fasta", required_argument, 0, 'f'},
        {"reference", required_argument, 0, 'r'}, {"pre-references", required_argument, 0, 'R'}, {"pre-queries", required_argument, 0, 'Q'},
        {"sketch-size", required_argument, 0, 's'}, {"whole-files", no_argument, 0, 'g'}, {"max-dist", required_argument, 0, 'd'},
        {"threads", required_argument, 0, 't'}, {"device", required_argument, 0, 1000}, {"scaled", required_argument, 0, 1005}, HASH_POLICY_OPTION, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:d:t:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 1005: scaled_given = true; scaled_ok = parse_scaled(optarg, scaled); break;
            case 'r': ref_files.push_back(optarg); break;
            case 'f': query_files.push_back(optarg); break;
            case 'R': ref_json.push_back(optarg); break;
            case 'Q': query_json.push_back(optarg); break;
            case 'k': ks.push_back(atoi(optarg)); break;
            case 's': S = atoi(optarg); if (S < 1) S = -1; break;
            case 'g': whole_files = true; break;
            case 'd': max_dist = atof(optarg); break;
            case 't': break;
            case 1000: device = atoi(optarg); break;
            default: help_dist(); exit(1);
        }
    }
    auto refuse = [](const std::string& why) { fprintf(stderr, "rkmh dist: %s\n", why.c_str()); exit(1); };
    if (ks.size() > 1) {
        std::string given;
        for (int k : ks) given += " " + std::to_string(k);
        refuse("a distance needs one k-mer size; sizes provided:" + given);
    }
    if (scaled_given && !scaled_ok) refuse("--scaled takes a number of at least 1");
    if (scaled_given && S != 0) refuse("--scaled and -s are two kinds of sketch; give one of them");
    if (S != 0 && (S < 1 || S > RK_MAX_SKETCH)) refuse("sketch size outside 1 .. " + std::to_string(RK_MAX_SKETCH));
    if (ref_files.empty() == ref_json.empty()) refuse("references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (!query_files.empty() && !query_json.empty()) refuse("queries come from -f <fasta|fastq> ... or from -Q <sketches.json> ..., not both");
    if (whole_files && ref_files.empty() && query_files.empty()) refuse("-g says how -r / -f files are sketched; sketches loaded with -R / -Q are what they are");
    const bool self = query_files.empty() && query_json.empty();
    // sketch files: each agrees in itself (load_sketch_json), with the others, with -k / -s where given, and with the run's policy
    int k = ks.empty() ? 0 : ks[0];
    // scaled files: kept as loaded (each at its own "scaled") until the run's value is known, then cut down to it
    std::vector<ScaledFile> sc_refs, sc_queries;
    bool any_bottom = false, any_scaled = false;
    uint64_t largest_scaled = 0;
    const int s_option = S;
    auto load = [&](const std::vector<const char*>& paths, SketchSet& into, std::vector<ScaledFile>& sc_into) {
        for (const char* path : paths) {
            LoadedSketches L;
            if (!load_sketch_json(path, L, RK_MAX_SKETCH)) {
                if (!L.err.empty()) refuse(std::string(path) + ": " + L.err);
                if (L.S > RK_MAX_SKETCH) refuse(std::string(path) + ": sketch size outside 1 .. " + std::to_string(RK_MAX_SKETCH));
                refuse(std::string("cannot load sketches from ") + path + " (unreadable, or its sketches disagree in kmer, hashPolicy or length)");
            }
            rk_policy theirs;
            rk_default_policy(&theirs);
            if (rk_policy_parse(L.policy.c_str(), &theirs) != RK_OK) refuse(std::string(path) + ": " + rk_last_error());
            if (!rk_policy_same_hashes(&theirs, &g_policy))
                refuse(std::string(path) + " holds sketches hashed with " + policy_text(theirs) + ", this run hashes with " + policy_text(g_policy) + ": pass --hash-policy " + policy_text(theirs));
            if (L.ks.size() != 1) refuse(std::string(path) + " holds sketches of " + std::to_string(L.ks.size()) + " k-mer sizes; a distance needs one");
            if (k != 0 && L.ks[0] != k) refuse(std::string(path) + " holds sketches of k = " + std::to_string(L.ks[0]) + ", the others (or -k) say " + std::to_string(k));
            (L.scaled ? any_scaled : any_bottom) = true;
            if (any_scaled && any_bottom) refuse(std::string(path) + ": scaled and bottom-s sketches cannot be compared with each other");
            if (L.scaled) {
                if (s_option != 0) refuse(std::string(path) + " holds scaled sketches (scaled = " + std::to_string(L.scaled) + "); -s is for bottom-s sketches");
                if (scaled_given && L.scaled > scaled)
                    refuse(std::string(path) + " holds sketches of scaled = " + std::to_string(L.scaled) + ": they cannot be made finer, --scaled must be at least that");
                largest_scaled = std::max(largest_scaled, L.scaled);
                k = L.ks[0];
                sc_into.push_back(ScaledFile{path, std::move(L)});
                continue;
            }
            if (scaled_given) refuse(std::string(path) + " holds bottom-s sketches; --scaled compares scaled ones (rkmh sketch --scaled)");
            if (S != 0 && L.S != S) refuse(std::string(path) + " holds sketches of size " + std::to_string(L.S) + ", the others (or -s) say " + std::to_string(S));
            k = L.ks[0]; S = L.S;
            into.names.insert(into.names.end(), L.names.begin(), L.names.end());
            into.sk.insert(into.sk.end(), L.sk.begin(), L.sk.end());
            into.lens.insert(into.lens.end(), L.lens.begin(), L.lens.end());
        }
    };
    SketchSet refs, queries;
    load(ref_json, refs, sc_refs);
    load(query_json, queries, sc_queries);
    if (k == 0) { fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n"); k = 16; }
    if (k < 1 || k > RK_MAX_K) refuse("k-mer size outside 1 .. " + std::to_string(RK_MAX_K));
    if (scaled_given || any_scaled) {
        if (!scaled_given) scaled = largest_scaled;
        uint64_t max_hash = 0;
        CK(rk_scaled_max_hash(scaled, &max_hash));
        ScaledSet sr, sq;
        cut_scaled_files(sc_refs, max_hash, sr);
        cut_scaled_files(sc_queries, max_hash, sq);
        // sides that come from sketch files alone are known now: refused before a context exists, like everything above
        if (ref_files.empty() && sr.names.empty()) refuse("no reference sketches");
        if (!self && query_files.empty() && sq.names.empty()) refuse("no query sketches");
        if (sr.names.size() > 0x7fffffffull || sq.names.size() > 0x7fffffffull) refuse("more than 2^31-1 sketches on one side");
        rk_ctx* sctx = nullptr;
        CK(rk_ctx_create(device, &g_policy, &sctx));
        const std::vector<int> kk(1, k);
        if (!ref_files.empty()) sketch_files_scaled(sctx, ref_files, kk, max_hash, whole_files, sr);
        if (!query_files.empty()) sketch_files_scaled(sctx, query_files, kk, max_hash, whole_files, sq);
        const ScaledSet& q = self ? sr : sq;
        const size_t nq = q.names.size(), nr = sr.names.size();
        if (nr == 0 || nq == 0) { fprintf(stderr, "rkmh dist: no %s sketches\n", nr == 0 ? "reference" : "query"); exit(1); }
        if (nq > 0x7fffffffull || nr > 0x7fffffffull) refuse("more than 2^31-1 sketches on one side");
        std::vector<int32_t> shared(nq * nr);
        CK(rk_compare_scaled(sctx, q.values.data(), q.off.data(), (int)nq, sr.values.data(), sr.off.data(), (int)nr, 0, shared.data()));
        std::string o;
        char num[160];
        for (size_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < nr; ++j) {
                const long long sh = shared[i * nr + j], lq = (long long)(q.off[i + 1] - q.off[i]), lr = (long long)(sr.off[j + 1] - sr.off[j]);
                double jac = 0, d = 1;
                CK(rk_scaled_distance(sh, lq, lr, k, &jac, &d));
                if (d > max_dist) continue;
                o += sr.names[j]; o += '\t'; o += q.names[i];
                const int n = snprintf(num, sizeof num, "\t%.6g\t%lld/%lld\t%lld/%lld\t%lld/%lld\n", d, sh, lq + lr - sh, sh, lq, sh, lr);
                o.append(num, (size_t)n);
                if (o.size() > (1u << 22)) { fwrite(o.data(), 1, o.size(), stdout); o.clear(); }
            }
        fwrite(o.data(), 1, o.size(), stdout);
        fflush(stdout);
        rk_ctx_destroy(sctx);
        return 0;
    }
    if (S == 0) S = 1000;
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    const std::vector<int> k1(1, k);
    if (!ref_files.empty()) sketch_files(ctx, ref_files, k1, S, whole_files, refs);
    if (!query_files.empty()) sketch_files(ctx, query_files, k1, S, whole_files, queries);
    const SketchSet& q = self ? refs : queries;
    const size_t nq = q.names.size(), nr = refs.names.size();
    if (nr == 0 || nq == 0) { fprintf(stderr, "rkmh dist: no %s sketches\n", nr == 0 ? "reference" : "query"); exit(1); }
    if (nq > 0x7fffffffull || nr > 0x7fffffffull) refuse("more than 2^31-1 sketches on one side");
    std::vector<int32_t> out4(nq * nr * 4);
    CK(rk_compare_sketches(ctx, q.sk.data(), q.lens.data(), (int)nq, refs.sk.data(), refs.lens.data(), (int)nr, S, out4.data()));
    std::string o;
    char num[96];
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nr; ++j) {
            const int32_t* r = &out4[(i * nr + j) * 4];
            double jac = 0, d = 1;
            CK(rk_mash_distance(r[2], r[3], k, &jac, &d));
            if (d > max_dist) continue;
            o += refs.names[j]; o += '\t'; o += q.names[i];
            const int n = snprintf(num, sizeof num, "\t%.6g\t%d/%d\t%d\n", d, r[2], r[3], r[0]);
            o.append(num, (size_t)n);
            if (o.size() > (1u << 22)) { fwrite(o.data(), 1, o.size(), stdout); o.clear(); }
        }
    fwrite(o.data(), 1, o.size(), stdout);
    fflush(stdout);
    rk_ctx_destroy(ctx);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// gather: which references make up a sample, and how much of it each explains once the better matches are taken out (include/
// rkmh_amd.h, "GATHER").  References and queries are scaled sketches, made or loaded as `dist --scaled` makes and loads them; the
// references go to the device once, the queries are gathered against them one after the other (rk_gather_scaled_device).
// Everything that can be refused is refused before a context exists.
static void help_gather() {
    fprintf(stderr,
            "rkmh gather (-r <refs.fa> ... | -R <refs.json> ...) (-f <sample.fa|fq[.gz]> ... | -Q <queries.json> ...) [-k <k>] [--scaled <n>] [-g]\n"
            "            [--min-shared <n>] [--max-rounds <n>] [--device <id>]\n"
            "  decomposes every query into references, greedily: the reference that holds most of what is left of the query is printed and\n"
            "  its hashes leave the query, until the best reference holds fewer than --min-shared (default 1) of them or --max-rounds lines\n"
            "  are printed; one line per pick, query by query: query, rank (from 1), reference, unique/|query| (hashes only this pick\n"
            "  explains at its turn), total/|query|, total/|reference| (total: all hashes the two share), remaining (hashes of the query\n"
            "  left unexplained); a query that no reference matches prints nothing\n"
            "  -f: every file is ONE query, the union of its records (a sample is a file of reads);  -Q: every sketch of the file is a query\n"
            "  -r: one reference per record, with -g one per FILE;  -R / -Q: scaled sketches written by `rkmh sketch --scaled <m>`\n"
            "  --scaled <n>: -r / -f files are sketched at n, -R / -Q files (m <= n) are cut down to n; without it: the largest m among the\n"
            "  files; not with -s (bottom-s sketches cannot be decomposed)\n" HASH_POLICY_HELP);
}
static bool parse_at_least_1(const char* text, int& v) {
    uint64_t u = 0;
    if (!parse_scaled(text, u) || u > 0x7fffffffull) return false;
    v = (int)u;
    return true;
}
int main_gather(int argc, char** argv) {
    std::vector<const char*> ref_files, query_files, ref_json, query_json;
    std::vector<int> ks;
    int device = 0, min_shared = 1, max_rounds = 0x7fffffff;
    bool whole_files = false, scaled_given = false, scaled_ok = true, s_given = false, min_ok = true, rounds_ok = true;
    uint64_t scaled = 0; // --scaled, or the largest "scaled" of the files loaded
    if (argc <= 2) { help_gather(); exit(1); }
    static struct option long_options[] = {{"help", no_argument, 0, 'h'}, {"kmer", required_argument, 0, 'k'}, {"fasta", required_argument, 0, 'f'},
        {"reference", required_argument, 0, 'r'}, {"pre-references", required_argument, 0, 'R'}, {"pre-queries", required_argument, 0, 'Q'},
        {"sketch-size", required_argument, 0, 's'}, {"whole-files", no_argument, 0, 'g'}, {"device", required_argument, 0, 1000},
        {"scaled", required_argument, 0, 1005}, {"min-shared", required_argument, 0, 1006}, {"max-rounds", required_argument, 0, 1007},
        HASH_POLICY_OPTION, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 1005: scaled_given = true; scaled_ok = parse_scaled(optarg, scaled); break;
            case 1006: min_ok = parse_at_least_1(optarg, min_shared); break;
            case 1007: rounds_ok = parse_at_least_1(optarg, max_rounds); break;
            case 'r': ref_files.push_back(optarg); break;
            case 'f': query_files.push_back(optarg); break;
            case 'R': ref_json.push_back(optarg); break;
            case 'Q': query_json.push_back(optarg); break;
            case 'k': ks.push_back(atoi(optarg)); break;
            case 's': s_given = true; break;
            case 'g': whole_files = true; break;
            case 1000: device = atoi(optarg); break;
            default: help_gather(); exit(1);
        }
    }
    auto refuse = [](const std::string& why) { fprintf(stderr, "rkmh gather: %s\n", why.c_str()); exit(1); };
    if (ks.size() > 1) {
        std::string given;
        for (int k : ks) given += " " + std::to_string(k);
        refuse("gather needs one k-mer size; sizes provided:" + given);
    }
    if (s_given) refuse("-s makes bottom-s sketches, which cannot be decomposed; gather works on scaled ones (--scaled)");
    if (scaled_given && !scaled_ok) refuse("--scaled takes a number of at least 1");
    if (!min_ok) refuse("--min-shared takes a number of at least 1");
    if (!rounds_ok) refuse("--max-rounds takes a number of at least 1");
    if (ref_files.empty() == ref_json.empty()) refuse("references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (query_files.empty() == query_json.empty()) refuse("queries come from -f <fasta|fastq> ... or from -Q <sketches.json> ..., one of the two");
    if (whole_files && ref_files.empty()) refuse("-g says how -r files are sketched; sketches loaded with -R are what they are");
    int k = ks.empty() ? 0 : ks[0];
    std::vector<ScaledFile> sc_refs, sc_queries;
    uint64_t largest_scaled = 0;
    auto load = [&](const std::vector<const char*>& paths, std::vector<ScaledFile>& into) { // the checks of `dist`, scaled files only
        for (const char* path : paths) {
            LoadedSketches L;
            if (!load_sketch_json(path, L, RK_MAX_SKETCH)) {
                if (!L.err.empty()) refuse(std::string(path) + ": " + L.err);
                refuse(std::string("cannot load sketches from ") + path + " (unreadable, or its sketches disagree in kmer, hashPolicy or length)");
            }
            rk_policy theirs;
            rk_default_policy(&theirs);
            if (rk_policy_parse(L.policy.c_str(), &theirs) != RK_OK) refuse(std::string(path) + ": " + rk_last_error());
            if (!rk_policy_same_hashes(&theirs, &g_policy))
                refuse(std::string(path) + " holds sketches hashed with " + policy_text(theirs) + ", this run hashes with " + policy_text(g_policy) + ": pass --hash-policy " + policy_text(theirs));
            if (L.ks.size() != 1) refuse(std::string(path) + " holds sketches of " + std::to_string(L.ks.size()) + " k-mer sizes; gather needs one");
            if (k != 0 && L.ks[0] != k) refuse(std::string(path) + " holds sketches of k = " + std::to_string(L.ks[0]) + ", the others (or -k) say " + std::to_string(k));
            if (!L.scaled) refuse(std::string(path) + " holds bottom-s sketches; gather decomposes scaled ones (rkmh sketch --scaled)");
            if (scaled_given && L.scaled > scaled)
                refuse(std::string(path) + " holds sketches of scaled = " + std::to_string(L.scaled) + ": they cannot be made finer, --scaled must be at least that");
            largest_scaled = std::max(largest_scaled, L.scaled);
            k = L.ks[0];
            into.push_back(ScaledFile{path, std::move(L)});
        }
    };
    load(ref_json, sc_refs);
    load(query_json, sc_queries);
    if (!scaled_given && largest_scaled == 0) refuse("no sketch file says at which scaled to sketch: give --scaled <n>");
    if (k == 0) { fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n"); k = 16; }
    if (k < 1 || k > RK_MAX_K) refuse("k-mer size outside 1 .. " + std::to_string(RK_MAX_K));
    if (!scaled_given) scaled = largest_scaled;
    uint64_t max_hash = 0;
    CK(rk_scaled_max_hash(scaled, &max_hash));
    ScaledSet sr, sq;
    cut_scaled_files(sc_refs, max_hash, sr);
    cut_scaled_files(sc_queries, max_hash, sq);
    if (ref_files.empty() && sr.names.empty()) refuse("no reference sketches");
    if (query_files.empty() && sq.names.empty()) refuse("no query sketches");
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    const std::vector<int> kk(1, k);
    if (!ref_files.empty()) sketch_files_scaled(ctx, ref_files, kk, max_hash, whole_files, sr);
    if (!query_files.empty()) sketch_files_scaled(ctx, query_files, kk, max_hash, true, sq); // a sample: one sketch per file
    const size_t nq = sq.names.size(), nr = sr.names.size();
    if (nr == 0 || nq == 0) { fprintf(stderr, "rkmh gather: no %s sketches\n", nr == 0 ? "reference" : "query"); exit(1); }
    if (nr > 0x7fffffffull) refuse("more than 2^31-1 reference sketches");
    // the references go to the device once; every query follows them into the same two arrays
    uint64_t longest = 0;
    for (size_t i = 0; i < nq; ++i) longest = std::max(longest, sq.off[i + 1] - sq.off[i]);
    if (longest > 0x7fffffffull) refuse("a query of more than 2^31-1 hashes");
    const int rows = (int)std::min<size_t>((size_t)max_rounds, nr);
    void *d_rv = nullptr, *d_ro = nullptr, *d_q = nullptr, *d_out = nullptr;
    CK(rk_device_alloc(ctx, sr.values.size() * 8, &d_rv));
    CK(rk_device_alloc(ctx, sr.off.size() * 8, &d_ro));
    CK(rk_device_alloc(ctx, (size_t)longest * 8, &d_q));
    CK(rk_device_alloc(ctx, (size_t)rows * 16, &d_out));
    CK(rk_device_upload(ctx, d_rv, sr.values.data(), sr.values.size() * 8));
    CK(rk_device_upload(ctx, d_ro, sr.off.data(), sr.off.size() * 8));
    std::vector<int32_t> out4((size_t)rows * 4);
    std::string o;
    char num[200];
    for (size_t i = 0; i < nq; ++i) {
        const uint64_t lq = sq.off[i + 1] - sq.off[i];
        int n = 0;
        CK(rk_device_upload(ctx, d_q, sq.values.data() + sq.off[i], (size_t)lq * 8));
        CK(rk_gather_scaled_device(ctx, d_q, lq, d_rv, d_ro, (int)nr, sr.values.size(), min_shared, rows, d_out, &n, rk_ctx_stream(ctx)));
        CK(rk_device_download(ctx, out4.data(), d_out, (size_t)n * 16));
        for (int t = 0; t < n; ++t) {
            const int32_t* r = &out4[(size_t)t * 4];
            const size_t ref = (size_t)r[0];
            if (ref >= nr) { fprintf(stderr, "rkmh gather: row %d names reference %d of %zu\n", t, r[0], nr); exit(1); }
            o += sq.names[i];
            const int m = snprintf(num, sizeof num, "\t%d\t", t + 1);
            o.append(num, (size_t)m);
            o += sr.names[ref];
            const int m2 = snprintf(num, sizeof num, "\t%d/%llu\t%d/%llu\t%d/%llu\t%d\n", r[1], (unsigned long long)lq, r[2], (unsigned long long)lq, r[2],
                                    (unsigned long long)(sr.off[ref + 1] - sr.off[ref]), r[3]);
            o.append(num, (size_t)m2);
        }
        if (o.size() > (1u << 22)) { fwrite(o.data(), 1, o.size(), stdout); o.clear(); }
    }
    fwrite(o.data(), 1, o.size(), stdout);
    fflush(stdout);
    for (void* p : {d_rv, d_ro, d_q, d_out}) rk_device_free(ctx, p);
    rk_ctx_destroy(ctx);
    return 0;
}

int main_hash(int argc, char** argv) {
    std::vector<const char*> files;
    std::vector<int> ks;
    int device = 0;
    bool print_kmers = false;
    if (argc <= 2) { help_hash(); exit(1); }
    static struct option long_options[] = {
        {"help", no_argument, 0, 'h'},        {"kmer", required_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'}, {"sketch-size", required_argument, 0, 's'},
        {"threads", required_argument, 0, 't'}, {"min-kmer-occurence", required_argument, 0, 'M'},
        {"max-samples", required_argument, 0, 'I'}, {"output", required_argument, 0, 'o'},
        {"device", required_argument, 0, 1000}, HASH_POLICY_OPTION, {0, 0, 0, 0}};
    optind = 2;
    int c;
    bool use_freqs = false;
    while ((c = getopt_long(argc, argv, "ThcwKk:f:s:t:mM:I:o:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 'f': files.push_back(optarg); break;
            case 'k': ks.push_back(atoi(optarg)); break;
            case 'K': print_kmers = true; break;
            case 'M': case 'I': use_freqs = true; break;       // accepted; nothing is printed (rkmh.cpp:2047,2109-2111)
            case 'T': case 'c': case 'w': case 'm': case 's': case 't': case 'o': break; // accepted and ignored
            case 1000: device = atoi(optarg); break;
            case '?': case 'h': default: print_help(); exit(1);
        }
    }
    if (ks.empty()) {
        fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n");
        ks.push_back(16);
    }
    if (files.empty()) { fprintf(stderr, "rkmh: -f <file> is required\n"); exit(1); }
    if (use_freqs) return 0;
    rk_ctx* ctx = nullptr;
    if (!print_kmers) CK(rk_ctx_create(device, &g_policy, &ctx));
    rk_reader* rd = nullptr;
    CK(rk_reader_open(files[0], &rd)); // only input_files[0] is used, rkmh.cpp:2064,2085
    std::string buf;
    for (;;) {
        rk_seqset s;
        CK(rk_reader_next(rd, 1000, 1ull << 28, &s)); // 1000-record buffers, rkmh.cpp:2085-2094
        if (s.nseq == 0) { rk_seqset_free(&s); break; }
        buf.clear();
        if (print_kmers) {
            for (int64_t i = 0; i < s.nseq; ++i) {
                buf += s.names + s.name_offsets[i];
                const uint8_t* seq = s.bases + s.offsets[i];
                int64_t len = (int64_t)(s.offsets[i + 1] - s.offsets[i]);
                for (int k : ks)
                    for (int64_t w = 0; w + k < len + (g_policy.drop_last_window ? 0 : 1); ++w) { // len-k windows, or len-k+1 (policy U3)
                        buf += '\t';
                        for (int j = 0; j < k; ++j) {
                            signed char ch = (signed char)seq[w + j];
                            buf += (char)(((int)ch - 91) > 0 ? ch - 32 : ch);
                        }
                    }
                buf += '\n';
            }
        } else {
            std::vector<uint64_t> ho((size_t)s.nseq + 1);
            uint64_t* h = nullptr;
            CK(rk_hash_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), &h, ho.data()));
            char num[32];
            for (int64_t i = 0; i < s.nseq; ++i) {
                buf += s.names + s.name_offsets[i];
                for (uint64_t j = ho[(size_t)i]; j < ho[(size_t)i + 1]; ++j) {
                    int n = snprintf(num, sizeof num, "\t%llu", (unsigned long long)h[j]);
                    buf.append(num, (size_t)n);
                }
                buf += '\n';
            }
            rk_free(h);
        }
        fwrite(buf.data(), 1, buf.size(), stdout);
        rk_seqset_free(&s);
    }
    rk_reader_close(rd);
    if (ctx) rk_ctx_destroy(ctx);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// hpv16 (main_hpv16, src/rkmh.cpp:2366-2723): HPV type of every read (set intersection of ALL its k-mer hashes with all hashes
// of each type reference), and its similarity to the k-mers specific to each HPV16 lineage / sublineage.
// Two mkmh functions on this path are absent from the reference snapshot (hash_set_intersection_size :2673, sort_by_similarity
// :2688/:2700); what they are taken to do is stated in DESIGN.md (policies U13/U14) and restated in oracle/oracle.py::hpv16.
static void help_hpv16() {
    fprintf(stderr,
            "rkmh hpv16 -f <reads.fq> [-R <dir>] [-k <k>]... [-t <n>] [-M <n>]\n"
            "  classifies every read to an HPV type (<dir>/all_pave_ref.fa) and reports its k-mer matches to the\n"
            "  HPV16 lineages / sublineages of <dir>/new_refs.fa; <dir> defaults to ./data (as the reference: run it from the\n"
            "  rkmh directory).  Also writes lineage_specific_hashes.<k>.tst into the working directory.\n"
            "  -s/-N/-D are accepted and unused, as in the reference.  --device <id>: GPU to use.\n"
            "  Reads of any length are accepted; those with more than 16384 k-mers (all -k together) are answered one at a time.\n" HASH_POLICY_HELP);
}
int main_hpv16(int argc, char** argv) {
    std::vector<const char*> read_files;
    std::string refpath = "data";                       // :2369
    std::vector<int> ks;
    int min_kmer_occ = 0, device = 0;
    bool do_read_depth = false;
    if (argc <= 2) { help_hpv16(); exit(1); }           // :2386-2389 (prints the classify help there)
    static struct option long_options[] = {             // :2393-2405
        {"help", no_argument, 0, 'h'},           {"kmer", no_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'},    {"reference", required_argument, 0, 'r'},
        {"sketch", required_argument, 0, 's'},   {"threads", required_argument, 0, 't'},
        {"min-kmer-occurence", required_argument, 0, 'M'}, {"min-matches", required_argument, 0, 'N'},
        {"min-diff", required_argument, 0, 'D'}, {"max-samples", required_argument, 0, 'I'},
        {"device", required_argument, 0, 1000},  HASH_POLICY_OPTION, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hk:f:R:s:t:M:N:D:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 't': case 's': case 'N': case 'D': break;          // parsed; nothing downstream reads them (:2411, :2428, :2435-2440)
            case 'f': read_files.push_back(optarg); break;
            case 'R': refpath = optarg; break;
            case 'k': if (optarg) ks.push_back(atoi(optarg)); break; // (--kmer is declared no_argument there too: unusable)
            case 'M': min_kmer_occ = atoi(optarg); do_read_depth = true; break;
            case 1000: device = atoi(optarg); break;
            case '?': case 'h': print_help(); exit(1);
            default: print_help(); abort();                          // --reference / --max-samples: declared, no case (:2441-2443)
        }
    }
    if (ks.empty()) {
        fprintf(stderr, "NO KMER SIZE PROVIDED. USING A DEFAULT KMER SIZE OF 16\n");   // :2449
        ks.push_back(16);
    }
    auto existing = [](const std::string& p) -> std::string {      // bundled test data is kept gzipped
        FILE* f = fopen(p.c_str(), "rb");
        if (f) { fclose(f); return p; }
        f = fopen((p + ".gz").c_str(), "rb");
        if (f) { fclose(f); return p + ".gz"; }
        fprintf(stderr, "rkmh hpv16: cannot open %s (pass the directory holding all_pave_ref.fa and new_refs.fa with -R)\n", p.c_str());
        exit(1);
    };
    const std::string type_file = existing(refpath + "/all_pave_ref.fa"), sub_file = existing(refpath + "/new_refs.fa");   // :2453-2456
    double t0 = now_s();
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    const rk_policy pol = g_policy;
    rk_seqset types, subs, reads;
    const char* p1[1] = {type_file.c_str()};
    const char* p2[1] = {sub_file.c_str()};
    CK(rk_parse_files(p1, 1, &types));
    CK(rk_parse_files(p2, 1, &subs));
    if (types.nseq < 1 || subs.nseq < 1) { fprintf(stderr, "rkmh hpv16: no sequences in the reference files\n"); exit(1); }
    memset(&reads, 0, sizeof reads);
    if (!read_files.empty()) CK(rk_parse_files(read_files.data(), (int)read_files.size(), &reads));
    tick("parse", t0);
    // all hashes (first -k only, :2546 and :2553) of the type and of the lineage/sublineage references, on the GPU
    const int k0 = ks[0];
    uint64_t *th = nullptr, *sh = nullptr;
    std::vector<uint64_t> tho((size_t)types.nseq + 1), sho((size_t)subs.nseq + 1);
    CK(rk_hash_batch(ctx, types.bases, types.offsets, types.nseq, &k0, 1, &th, tho.data()));
    CK(rk_hash_batch(ctx, subs.bases, subs.offsets, subs.nseq, &k0, 1, &sh, sho.data()));
    // lineage- and sublineage-specific k-mers: union per (sub)lineage, minus every other one (:2560-2650), in std::map order
    auto specific = [&](int key_len, std::vector<std::string>& names, std::vector<std::vector<uint64_t>>& lists) {
        std::map<std::string, std::set<uint64_t>> groups;
        for (int64_t i = 0; i < subs.nseq; ++i) {
            std::string key(subs.names + subs.name_offsets[i]);
            key = key.substr(0, (size_t)key_len);                    // subtype_keys[i][0] / substr(0, 2)
            groups[key].insert(sh + sho[(size_t)i], sh + sho[(size_t)i + 1]);
        }
        for (auto& x : groups) {
            std::vector<uint64_t> xdiff(x.second.begin(), x.second.end()), diff;
            for (auto& y : groups) {
                if (y.first == x.first) continue;
                diff.clear();
                std::set_difference(xdiff.begin(), xdiff.end(), y.second.begin(), y.second.end(), std::back_inserter(diff));
                xdiff.swap(diff);
            }
            names.push_back(x.first);
            lists.push_back(xdiff);                                  // ascending (mkmh::sort of a sorted range, :2592)
        }
    };
    std::vector<std::string> lin_names, sublin_names;
    std::vector<std::vector<uint64_t>> lin_lists, sublin_lists;
    specific(1, lin_names, lin_lists);
    {   // :2598-2611
        FILE* ofi = fopen(("lineage_specific_hashes." + std::to_string(k0) + ".tst").c_str(), "w");
        fprintf(stderr, "Lineage specific kmer table created:\n");
        for (size_t i = 0; i < lin_names.size(); ++i) {
            fprintf(stderr, "\t%s\t%zu\n", lin_names[i].c_str(), lin_lists[i].size());
            if (ofi) {
                fprintf(ofi, "%s\t", lin_names[i].c_str());
                for (uint64_t x : lin_lists[i]) fprintf(ofi, "%llu\t", (unsigned long long)x);
                fprintf(ofi, "\n");
            }
        }
        if (ofi) fclose(ofi);
    }
    specific(2, sublin_names, sublin_lists);
    fprintf(stderr, "Sublineage specific kmer table created:\n");   // :2647-2650
    for (size_t i = 0; i < sublin_names.size(); ++i) fprintf(stderr, "\t%s\t%zu\n", sublin_names[i].c_str(), sublin_lists[i].size());
    // reference lists for the device: distinct non-zero values, ascending (set semantics of hash_set_intersection_size, U13)
    const int ntype = (int)types.nseq, nlin = (int)lin_names.size(), nsub = (int)sublin_names.size(), nref = ntype + nlin + nsub;
    const int S = RK_MAX_SKETCH;   // list capacity = most hashes a read may have here (no bottom-s on this path)
    std::vector<uint64_t> lists((size_t)nref * (size_t)S, 0);
    std::vector<int32_t> lens((size_t)nref, 0);
    std::vector<size_t> full_len((size_t)nref, 0);                   // reflens as the reference passes them to sort_by_similarity
    auto put = [&](int r, std::vector<uint64_t> v) {
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        if (!v.empty() && v[0] == 0) v.erase(v.begin());
        if (v.size() > (size_t)S) { fprintf(stderr, "rkmh hpv16: reference %d has %zu distinct k-mers (limit %d)\n", r, v.size(), S); exit(1); }
        memcpy(&lists[(size_t)r * S], v.data(), v.size() * 8);
        lens[(size_t)r] = (int32_t)v.size();
    };
    for (int i = 0; i < ntype; ++i) put(i, std::vector<uint64_t>(th + tho[(size_t)i], th + tho[(size_t)i + 1]));
    for (int i = 0; i < nlin; ++i) { put(ntype + i, lin_lists[(size_t)i]); full_len[(size_t)(ntype + i)] = lin_lists[(size_t)i].size(); }
    for (int i = 0; i < nsub; ++i) { put(ntype + nlin + i, sublin_lists[(size_t)i]); full_len[(size_t)(ntype + nlin + i)] = sublin_lists[(size_t)i].size(); }
    rk_free(th); rk_free(sh);
    CK(rk_set_kmer_form(ctx, 0));   // these "references" are only used through the general kernels: no need to enumerate the k-mer universe
    CK(rk_set_reference_sketches(ctx, lists.data(), lens.data(), nref, ks.data(), (int)ks.size(), S));   // reads are hashed with EVERY -k (:2661)
    tick("tables", t0);
    rk_counter* cnt = nullptr;
    if (do_read_depth) {                                             // :2514-2530, then mask_by_frequency per read (:2663)
        CK(rk_counter_create(ctx, 800000000ull, &cnt));
        CK(rk_count_batch(ctx, reads.bases, reads.offsets, reads.nseq, cnt));
        CK(rk_set_depth_filter(ctx, cnt, min_kmer_occ));
    }
    std::vector<int32_t> out4((size_t)reads.nseq * 4), tail((size_t)reads.nseq * (size_t)(nlin + nsub));
    // The batched path keeps every hash of a read in the in-LDS sorter (RK_MAX_SKETCH values).  A longer read (a nanopore or
    // rolling-circle read of more than ~16 kb, or ~8 kb with two -k) is answered one at a time instead: hashed on the GPU
    // (rk_hash_batch, any length), masked (-M), then intersected with every list on the host exactly as :2666-2704 does -- the
    // reference handles reads of any length, so does this.
    auto hashes_of = [&](int64_t i) -> int64_t {
        const int64_t len = (int64_t)(reads.offsets[i + 1] - reads.offsets[i]);
        int64_t hn = 0;
        for (int k : ks) { const int64_t nw = pol.drop_last_window ? len - k : len - k + 1; if (nw > 0) hn += nw; }
        return hn;
    };
    std::vector<int64_t> longs, normal;
    for (int64_t i = 0; i < reads.nseq; ++i) (hashes_of(i) > (int64_t)S ? longs : normal).push_back(i);
    if (longs.empty()) {
        if (reads.nseq > 0) CK(rk_classify_groups_batch(ctx, reads.bases, reads.offsets, reads.nseq, ntype, out4.data(), tail.data()));
    } else {
        fprintf(stderr, "rkmh hpv16: %zu read(s) with more than %d k-mers are classified one at a time\n", longs.size(), S);
        if (!normal.empty()) { // the other reads as a batch of their own
            std::vector<uint64_t> off(normal.size() + 1, 0);
            for (size_t j = 0; j < normal.size(); ++j) off[j + 1] = off[j] + (reads.offsets[normal[j] + 1] - reads.offsets[normal[j]]);
            std::vector<uint8_t> sub((size_t)off.back() + 64);
            for (size_t j = 0; j < normal.size(); ++j) memcpy(sub.data() + off[j], reads.bases + reads.offsets[normal[j]], (size_t)(off[j + 1] - off[j]));
            std::vector<int32_t> o4(normal.size() * 4), tl(normal.size() * (size_t)(nlin + nsub));
            CK(rk_classify_groups_batch(ctx, sub.data(), off.data(), (int64_t)normal.size(), ntype, o4.data(), tl.data()));
            for (size_t j = 0; j < normal.size(); ++j) {
                memcpy(&out4[(size_t)normal[j] * 4], &o4[j * 4], 16);
                memcpy(&tail[(size_t)normal[j] * (size_t)(nlin + nsub)], &tl[j * (size_t)(nlin + nsub)], sizeof(int32_t) * (size_t)(nlin + nsub));
            }
        }
        for (int64_t i : longs) {
            uint64_t* h = nullptr;
            uint64_t ho[2] = {0, 0};
            const uint64_t one[2] = {0, reads.offsets[i + 1] - reads.offsets[i]};
            CK(rk_hash_batch(ctx, reads.bases + reads.offsets[i], one, 1, ks.data(), (int)ks.size(), &h, ho));
            if (cnt) CK(rk_mask_by_frequency(ctx, h, (int)ho[1], cnt, min_kmer_occ));
            std::vector<uint64_t> v(h, h + ho[1]);
            rk_free(h);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            if (!v.empty() && v[0] == 0) v.erase(v.begin());
            auto isect = [&](int r) { // distinct non-zero values in both ascending arrays (U13)
                const uint64_t* a = &lists[(size_t)r * S];
                const int na = lens[(size_t)r];
                int n = 0, x = 0; size_t y = 0;
                while (x < na && y < v.size()) { if (a[x] == v[y]) { ++n; ++x; ++y; } else if (a[x] < v[y]) ++x; else ++y; }
                return n;
            };
            int best = 0, best_id = 0, prev = -1;                                   // first maximum wins (:2669-2679)
            for (int r = 0; r < ntype; ++r) { const int c2 = isect(r); if (c2 > best) { prev = best; best = c2; best_id = r; } }
            int32_t* o = &out4[(size_t)i * 4];
            o[0] = best_id; o[1] = best; o[2] = best - prev; o[3] = (int32_t)v.size();
            for (int r = 0; r < nlin + nsub; ++r) tail[(size_t)i * (size_t)(nlin + nsub) + (size_t)r] = isect(ntype + r);
        }
    }
    tick("classify", t0);
    const bool den_read = getenv("RKMH_HPV16_SIM") && !strcmp(getenv("RKMH_HPV16_SIM"), "read");   // U14: similarity denominator
    // The lines (one stable sort and a dozen "%g" per read) are written by all granted CPUs, 16 k reads per piece, and leave in input order.
    auto emit_range = [&](int64_t lo, int64_t hi, std::string& buf) {
        char num[64];
        std::vector<int> order;
        std::vector<double> sims;
        auto ranked = [&](const int32_t* cnts, int first, int n, int hashnum, const std::vector<std::string>& names, std::string& a, std::string& b) {
            // sort_by_similarity (U14): intersection / list size, descending, ties in reference order
            order.resize((size_t)n); sims.resize((size_t)n);
            for (int i = 0; i < n; ++i) {
                order[(size_t)i] = i;
                const double den = den_read ? (double)hashnum : (double)full_len[(size_t)(first + i)];
                sims[(size_t)i] = den > 0 ? (double)cnts[i] / den : 0.0;
            }
            std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sims[(size_t)x] > sims[(size_t)y]; });
            for (int i : order) {
                a += names[(size_t)i]; a += ':';
                snprintf(num, sizeof num, "%g", sims[(size_t)i]);        // ostream << double
                a += num; a += ';';
                b += std::to_string(cnts[i]); b += ';';
            }
        };
        std::string la, lb, sa, sb;
        for (int64_t i = lo; i < hi; ++i) {
            const int64_t len = (int64_t)(reads.offsets[i + 1] - reads.offsets[i]);
            int64_t hashnum = 0;
            for (int k : ks) { const int64_t nw = pol.drop_last_window ? len - k : len - k + 1; if (nw > 0) hashnum += nw; }
            const int32_t* r = &out4[(size_t)i * 4];
            const int32_t* t = &tail[(size_t)i * (size_t)(nlin + nsub)];
            buf += reads.names + reads.name_offsets[i]; buf += '\t';
            buf += types.names + types.name_offsets[r[0]]; buf += '\t';
            buf += std::to_string(r[1]); buf += '/'; buf += std::to_string(hashnum); buf += '\t';
            la.clear(); lb.clear(); sa.clear(); sb.clear();
            ranked(t, ntype, nlin, (int)hashnum, lin_names, la, lb);
            ranked(t + nlin, ntype + nlin, nsub, (int)hashnum, sublin_names, sa, sb);
            buf += la; buf += '\t'; buf += sa; buf += '\t'; buf += lb; buf += '\t'; buf += sb; buf += '\n';
        }
    };
    {
        const int64_t PIECE = 1 << 14;
        const int nth = std::max(1, std::min(granted_cpus_main(), 32));
        const int64_t npieces = (reads.nseq + PIECE - 1) / PIECE;
        for (int64_t p0 = 0; p0 < npieces; p0 += nth) { // a wave of pieces at a time: memory stays bounded, the order is the input's
            const int64_t np = std::min<int64_t>(nth, npieces - p0);
            std::vector<std::string> bufs((size_t)np);
            std::vector<std::thread> th;
            for (int64_t q = 0; q < np; ++q)
                th.emplace_back([&, q] { emit_range((p0 + q) * PIECE, std::min(reads.nseq, (p0 + q + 1) * PIECE), bufs[(size_t)q]); });
            for (auto& t : th) t.join();
            for (auto& b : bufs) fwrite(b.data(), 1, b.size(), stdout);
        }
    }
    tick("emit", t0);
    if (cnt) rk_counter_destroy(cnt);
    rk_seqset_free(&types); rk_seqset_free(&subs);
    if (!read_files.empty()) rk_seqset_free(&reads);
    rk_ctx_destroy(ctx);
    return 0;
}
