// rkmh_commands.cpp -- the hashing policy of the run and the help text the sub-commands share; call and hash.
#include "rkmh_cli.hpp"

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
            "  multigather         gather for many queries at once, through an inverted index of the references: the lines of gather, byte for byte\n"
            "  manysearch          search many scaled sketches against a collection through an inverted index: only the pairs that match, in dist's columns\n"
            "  cluster             group a collection of scaled sketches into single-linkage clusters at a Jaccard or max-containment threshold\n"
            "  screen              which bottom-s reference sketches a read file contains: shared k-mers, identity and median multiplicity per reference\n"
            "  pack                write reads as a packed file (2 bits per base + names): stream|filter -F <file> classifies it without parsing\n"
            "Run a command without options for its help text.\n");
}
int default_k() { fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n"); return 16; }
static void help_hash() {
    fprintf(stderr,
            "rkmh hash -f <seqs.fa|fq> [-k <k>]... [--hash-policy <spec>]\n"
            "  prints one line per sequence: name, then every k-mer hash, tab separated\n" HASH_POLICY_HELP);
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
    if (ks.empty()) ks.push_back(default_k());
    else if (ks.size() > 1) {                               // rkmh.cpp:1543-1552
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
    if (ks.empty()) ks.push_back(default_k());
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
