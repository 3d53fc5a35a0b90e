// rkmh_screen.cpp -- `rkmh screen`: which bottom-s reference sketches a read file contains (include/rkmh_amd.h, "SCREEN"; what Mash
// calls screen).  The references are made or loaded as dist makes and loads its bottom-s side and become resident once
// (rk_screen_create); every -f file is ONE read set and goes through the file driver of rkmh_sample.cpp (file_feed) into the screen:
// no file is held whole, device memory is the reference values whatever the file holds.  Everything that can be refused is refused
// before a context exists.
#include <cerrno>
#include <cmath>

#include "rkmh_cli.hpp"

static void help_screen() {
    fprintf(stderr,
            "rkmh screen (-r <refs.fa> ... | -R <refs.json> ...) -f <reads.fq|fa[.gz]> ... [-k <k>] [-s <sketch>] [-g] [--min-copies <m>]\n"
            "            [-w | --winner-takes-all] [--min-shared <n>] [--min-identity <x>] [--device <id>]\n"
            "  counts, for every reference sketch, how many of its hashes occur among the k-mers of a read file -- a metagenome, a mixed\n"
            "  sample: the question is containment, not the similarity `dist -g` reports -- and how often; every -f file is ONE read set\n"
            "  prints one line per (file, reference) with at least --min-shared (default 1) shared hashes and an identity of at least\n"
            "  --min-identity (default 0), files in the order given, references in their order: identity, shared/|reference|, median\n"
            "  multiplicity of the shared hashes, reference, file;  identity = (shared/|reference|)^(1/k)\n"
            "  --min-copies <m>: a hash counts as present when at least m windows of the file hash to it (default 1)\n"
            "  -w: winner takes all: a hash shared by several references counts only for the one with the largest shared/|reference|\n"
            "  (the first of equals); shared, median and identity are then those of the hashes a reference owns\n"
            "  -r: one reference per record, with -g one per FILE;  -R: bottom-s sketches written by `rkmh sketch -s` (or Mash's, as JSON)\n"
            "  not with --scaled (scaled references are decomposed by `rkmh gather`), --abund or -Q; there is no p-value\n" HASH_POLICY_HELP);
}
static const CompareRules screen_rules = {"screen", "a screen", nullptr, false, "more than 2^31-1 reference sketches"};

// a decimal number of 0 .. 1, nothing else
static bool parse_unit(const char* text, double& x) {
    if (!text || !*text) return false;
    char* e = nullptr;
    errno = 0;
    const double v = strtod(text, &e);
    if (errno != 0 || *e != 0 || !(v >= 0.0 && v <= 1.0)) return false;
    x = v;
    return true;
}

int main_screen(int argc, char** argv) {
    CompareInputs in;
    int min_shared = 1;
    bool min_ok = true, id_ok = true, owned = false;
    double min_identity = 0.0;
    if (argc <= 2) { help_screen(); exit(1); }
    static struct option long_options[] = {COMPARE_OPTIONS, {"min-shared", required_argument, 0, 1006}, {"abund", no_argument, 0, 1008},
                                           {"min-copies", required_argument, 0, 1012}, {"min-identity", required_argument, 0, 1013},
                                           {"winner-takes-all", no_argument, 0, 'w'}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgwk:f:r:R:Q:s:", long_options, nullptr)) != -1) {
        if (shared_option(c, in)) continue;
        switch (c) {
            case 'w': owned = true; break;
            case 1006: min_ok = parse_at_least_1(optarg, min_shared); break;
            case 1008: in.abund = true; break;
            case 1012: if (!parse_min_copies(optarg, in.min_copies)) in.min_copies = 0; break;
            case 1013: id_ok = parse_unit(optarg, min_identity); break;
            default: help_screen(); exit(1);
        }
    }
    LoadedSides ld;
    ld.k = one_k(in, screen_rules);
    if (in.scaled_given) refuse(screen_rules, "--scaled makes scaled sketches; screen counts bottom-s ones (-s): scaled references are decomposed by `rkmh gather`");
    if (in.abund) refuse(screen_rules, "--abund has no meaning here: screen counts the copies of every reference hash itself (the median column)");
    if (!in.query_json.empty()) refuse(screen_rules, "-Q has no meaning here: screen reads the sequences themselves, -f <reads> ...");
    if (in.query_files.empty()) refuse(screen_rules, "no read files: give -f <reads.fq|fa[.gz]> ..., each file is one read set");
    if (in.min_copies == 0) refuse(screen_rules, "--min-copies takes a number of 1 .. 4294967295");
    if (!id_ok) refuse(screen_rules, "--min-identity takes a number from 0 to 1");
    if (!min_ok) refuse(screen_rules, "--min-shared takes a number of at least 1");
    if (in.S != 0 && (in.S < 1 || in.S > RK_MAX_SKETCH)) refuse(screen_rules, "sketch size outside 1 .. " + std::to_string(RK_MAX_SKETCH));
    if (in.ref_files.empty() == in.ref_json.empty()) refuse(screen_rules, "references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (in.whole_files && in.ref_files.empty()) refuse(screen_rules, "-g says how -r files are sketched; sketches loaded with -R are what they are");
    in.abund = false;
    load_sketch_files(in, screen_rules, ld);
    if (ld.largest_scaled != 0) refuse(screen_rules, "the -R files hold scaled sketches; screen counts bottom-s ones: scaled references are decomposed by `rkmh gather`");
    const int k = run_k(screen_rules, ld.k);
    const int S = ld.S ? ld.S : 1000;
    if (ld.refs.names.size() > 0x7fffffffull) refuse(screen_rules, screen_rules.too_many_loaded);
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(in.device, &g_policy, &ctx));
    const std::vector<int> k1(1, k);
    if (!in.ref_files.empty()) sketch_files(ctx, in.ref_files, k1, S, in.whole_files, ld.refs);
    const SketchSet& refs = ld.refs;
    const size_t nr = refs.names.size();
    if (nr == 0) refuse(screen_rules, "no reference sketches");
    if (nr > 0x7fffffffull) refuse(screen_rules, screen_rules.too_many_loaded);
    // the rows as CSR, and the number of distinct values of each
    std::vector<uint64_t> values, off(nr + 1, 0), len(nr, 0);
    for (size_t i = 0; i < nr; ++i) {
        const uint64_t* row = &refs.sk[i * (size_t)S];
        const size_t n = (size_t)std::max(refs.lens[i], 0);
        values.insert(values.end(), row, row + n);
        off[i + 1] = values.size();
        for (size_t t = 0; t < n; ++t) len[i] += t == 0 || row[t] != row[t - 1];
    }
    rk_screen* screen = nullptr;
    CK(rk_screen_create(ctx, k1.data(), 1, values.data(), off.data(), (int64_t)nr, &screen));
    const FileSink sink{[screen](rk_fastq_slot* slot, uint64_t nbytes, int32_t* status, int64_t* nrec) { return rk_fastq_slot_screen(slot, nbytes, screen, status, nrec); },
                        [screen](const rk_seqset& s) { return rk_screen_add_batch(screen, s.bases, s.offsets, s.nseq); }};
    std::vector<uint32_t> out4(nr * 4);
    OutBuf o(stdout);
    for (const char* f : in.query_files) {
        const SampleFed fed = file_feed(ctx, sink, f);
        CKE(rk_screen_rows(screen, in.min_copies, out4.data()), f);
        if (g_timing) {
            rk_screen_stats_t st;
            st.struct_size = sizeof st;
            CKE(rk_screen_stats(screen, &st), f);
            fprintf(stderr, "[rkmh timing] screen %s: %s route, %lld blocks, %llu sequences, %llu bases, %llu windows counted into %llu keys: feed %.3f s, rows %.3f s\n", f,
                    fed.route, (long long)fed.blocks, (unsigned long long)st.nseq, (unsigned long long)st.nbases, (unsigned long long)st.counted,
                    (unsigned long long)st.nkeys, fed.t1 - fed.t0, now_s() - fed.t1);
        }
        CKE(rk_screen_reset(screen), f);
        for (size_t i = 0; i < nr; ++i) {
            const uint32_t* r = &out4[i * 4 + (owned ? 2 : 0)];
            if (r[0] < (uint32_t)min_shared) continue;
            double identity = 0;
            CK(rk_screen_identity(r[0], len[i], k, &identity));
            if (identity < min_identity) continue;
            o.appendf("%.6g\t%u/%llu\t%u\t", identity, r[0], (unsigned long long)len[i], r[1]);
            o.append(refs.names[i]); o.append("\t"); o.append(f); o.append("\n");
            o.end_row();
        }
    }
    o.flush();
    fflush(stdout);
    rk_screen_destroy(screen);
    rk_ctx_destroy(ctx);
    return 0;
}
