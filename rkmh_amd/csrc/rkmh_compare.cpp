// rkmh_compare.cpp -- the commands on sketch sets (rkmh_sketches.cpp): sketch writes them, dist compares all pairs, gather decomposes
// one query after the other and multigather all at once, manysearch reports the pairs that match.
#include <algorithm>

#include "rkmh_cli.hpp"

static void help_sketch() {
    fprintf(stderr,
            "rkmh sketch -f <seqs.fa|fq> [-k <k>]... [-s <sketch> | --scaled <n> [--abund]] [-g [--min-copies <m>]] [-o <out.json>] [--kmer-cache <file>]\n"
            "  writes a JSON array with one MinHash sketch per sequence (schema of the reference's dump_hash_json);\n"
            "  -g: one sketch per input FILE (named by its path; no k-mer spans two of its records), as Mash sketches an assembly;\n"
            "  a bottom-s sketch with -g is built on the device as the file is read: no file is held whole (RKMH_SAMPLE_DEVICE=0: the old route)\n"
            "  --min-copies <m> (with -g and -s; default 1): only k-mers seen at least m times over the whole file count, as `mash sketch -r -m`\n"
            "  filters the errors out of a read set, but exactly; objects gain \"minCopies\".  While fewer than <sketch> k-mers have m copies every\n"
            "  distinct k-mer of the file is kept on the device with its count: a file of low coverage at m >= 2 needs memory for all of them\n"
            "  --scaled <n>: scaled (FracMinHash) sketches instead of bottom-s ones: every distinct hash up to (2^64 - 1) / n, so the size\n"
            "  grows with the sequence; objects gain \"scaled\" and \"maxHash\"; such files serve `rkmh dist` only\n"
            "  --abund (with --scaled): \"sketches\" gains \"abundances\", parallel to \"hashes\": how many windows of the sequence hash to each\n"
            "  value (with -g: summed over the file's records); `rkmh gather --abund -Q` and `rkmh dist --abund -R / -Q` need them, every other reader ignores them\n"
            "  `rkmh stream -R <out.json>` loads it instead of sketching references again;\n"
            "  --kmer-cache <file>: also enumerates the k-mers behind these sketches (k 8 .. 18) into <file>, which\n"
            "  `rkmh stream -R <out.json> --kmer-cache <file>` then loads instead of enumerating them at every start\n"
            "  the file records the hashing policy (\"hashPolicy\"); stream -R refuses sketches hashed under another one\n" HASH_POLICY_HELP);
}
int main_sketch(int argc, char** argv) {
    std::vector<const char*> files;
    std::vector<int> ks;
    int S = 1000, device = 0;
    const char* outp = nullptr;
    const char* kmer_cache = nullptr;
    bool whole_files = false, s_given = false, scaled_given = false, scaled_ok = true, abund = false;
    uint64_t scaled = 0, min_copies = 1;
    if (argc <= 2) { help_sketch(); exit(1); }
    optind = 2;
    int c;
    static struct option long_options[] = {{"help", no_argument, 0, 'h'}, {"kmer", required_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'}, {"reference", required_argument, 0, 'r'}, {"sketch-size", required_argument, 0, 's'},
        {"output", required_argument, 0, 'o'}, {"device", required_argument, 0, 1000}, {"kmer-cache", required_argument, 0, 1003},
        {"whole-files", no_argument, 0, 'g'}, {"scaled", required_argument, 0, 1005}, {"abund", no_argument, 0, 1008}, {"min-copies", required_argument, 0, 1012}, HASH_POLICY_OPTION, {0, 0, 0, 0}};
    while ((c = getopt_long(argc, argv, "hgk:f:r:s:o:t:", long_options, nullptr)) != -1) {
        switch (c) {
            case 1008: abund = true; break;
            case 1012: if (!parse_min_copies(optarg, min_copies)) min_copies = 0; break;
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
    if (ks.empty()) ks.push_back(default_k());
    if (files.empty()) { fprintf(stderr, "rkmh: -f <file> is required\n"); exit(1); }
    if (scaled_given) {
        if (!scaled_ok) { fprintf(stderr, "rkmh sketch: --scaled takes a number of at least 1\n"); exit(1); }
        if (s_given) { fprintf(stderr, "rkmh sketch: --scaled and -s are two kinds of sketch; give one of them\n"); exit(1); }
        if (kmer_cache) { fprintf(stderr, "rkmh sketch: --kmer-cache serves `stream -R`; scaled sketches serve `rkmh dist` only\n"); exit(1); }
    }
    if (abund && !scaled_given) { fprintf(stderr, "rkmh sketch: --abund goes with --scaled <n>; bottom-s sketches keep no abundances\n"); exit(1); }
    refuse_min_copies("sketch", min_copies, whole_files, scaled_given);
    if (!scaled_given && whole_files && (S < 1 || S > RK_MAX_SKETCH)) { fprintf(stderr, "rkmh sketch: -g needs a sketch size of 1 .. %d\n", RK_MAX_SKETCH); exit(1); }
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(device, &g_policy, &ctx));
    SketchSet set;
    ScaledSet sc;
    std::vector<SketchRow> rows;
    uint64_t max_hash = 0;
    if (scaled_given) {
        CK(rk_scaled_max_hash(scaled, &max_hash));
        sc.with_abund = abund;
        sketch_files_scaled(ctx, files, ks, max_hash, whole_files, sc);
        static const uint32_t no_values = 0; // (an empty sketch still says "abundances":[])
        const uint32_t* ab = !abund ? nullptr : sc.abund.empty() ? &no_values : sc.abund.data();
        for (size_t i = 0; i < sc.names.size(); ++i)
            rows.push_back({sc.values.data() + sc.off[i], sc.off[i + 1] - sc.off[i], sc.off[i + 1] - sc.off[i], ab ? ab + sc.off[i] : nullptr});
    } else {
        sketch_files(ctx, files, ks, S, whole_files, set, min_copies);
        if (kmer_cache && *kmer_cache) {
            // the index of these sketches is built once here, for its k-mer enumeration: the file's tag hashes the index keys, k and the
            // hashing policy, so a later `stream -R <these sketches> --kmer-cache <file>` finds it -- and anything else does not use it
            CK(rk_set_kmer_cache(ctx, kmer_cache));
            CK(rk_set_reference_sketches(ctx, set.sk.data(), set.lens.data(), (int)set.names.size(), ks.data(), (int)ks.size(), S));
            if (rk_kmer_cache_state(ctx) == 0) fprintf(stderr, "rkmh: no k-mer enumeration for these sketches (k-mer sizes outside 8 .. 18, or a hash with two k-mers): %s not written\n", kmer_cache);
        }
        for (size_t i = 0; i < set.names.size(); ++i) rows.push_back({set.sk.data() + i * (size_t)S, (uint64_t)set.lens[i], (uint64_t)S});
    }
    FILE* fo = outp ? fopen(outp, "w") : stdout;
    if (!fo) { fprintf(stderr, "rkmh: cannot write %s\n", outp); exit(1); }
    std::string kstr;
    for (size_t i = 0; i < ks.size(); ++i) { kstr += std::to_string(ks[i]); if (i + 1 < ks.size()) kstr += ' '; }
    write_sketch_json(fo, scaled_given ? sc.names : set.names, scaled_given ? sc.seq_len : set.seq_len, kstr, rows, scaled_given ? scaled : 0, max_hash, min_copies);
    if (fo != stdout) fclose(fo);
    rk_ctx_destroy(ctx);
    return 0;
}

// -k, or what the sketch files said, or the default; inside the library's range
int run_k(const CompareRules& rules, int k) {
    if (k == 0) k = default_k();
    if (k < 1 || k > RK_MAX_K) refuse(rules, "k-mer size outside 1 .. " + std::to_string(RK_MAX_K));
    return k;
}

// ------------------------------------------------------------------------------------------------------------------------
// dist: the Mash distance of every (query, reference) pair of sketches -- `mash dist`, which the reference has no command for.  The
// four counts of a pair come from one launch over all pairs (rk_compare_sketches); the floating point is rk_mash_distance's.  With
// scaled sketches: their shared values (rk_compare_scaled) and rk_scaled_distance; with --abund on top of that the four sums of
// rk_compare_scaled_abund, the row sums of both sides and rk_angular_similarity: three more columns.
// Everything that can be refused is refused before a context exists: nothing is printed by a run that fails.
static void help_dist() {
    fprintf(stderr,
            "rkmh dist (-r <refs.fa> ... | -R <refs.json>) [-f <queries.fa|fq> ... | -Q <queries.json>] [-k <k>] [-s <sketch> | --scaled <n> [--abund]] [-g [--min-copies <m>]] [-d <maxdist>]\n"
            "  prints one line per (query, reference) pair, query by query: reference, query, Mash distance, common/denom of the merged\n"
            "  bottom-s sketch, shared hashes (the multiset intersection `stream` counts); without -f / -Q every reference is compared\n"
            "  with every reference\n"
            "  -R / -Q: sketches written by `rkmh sketch` (their k-mer size, sketch size and hashing policy must agree with each other and the run)\n"
            "  --scaled <n>: compare scaled (FracMinHash) sketches, every distinct hash up to (2^64 - 1) / n: -r / -f files are sketched at n,\n"
            "  -R / -Q files hold sketches of `rkmh sketch --scaled <m>`, m <= n, and are cut down to n (without --scaled: to the largest m\n"
            "  among them); a line is then: reference, query, distance from shared/union, shared/union, shared/|query|, shared/|reference|\n"
            "  (the last two: how much of the query is contained in the reference, and the reverse); not with -s\n"
            "  --abund (scaled runs only): both sides keep how many of their windows hash to each value (-r / -f files are sketched so, with -g\n"
            "  summed over a file's records; -R / -Q files must come from `rkmh sketch --scaled <m> --abund`); a line keeps its six columns and\n"
            "  gains three: the angular similarity of the two abundance vectors, 1 - 2 acos(cosine) / pi (1: the same proportions, 0: nothing\n"
            "  shared), wq_in/wq_total (the query's windows whose hash the reference holds / all windows the query kept) and wr_in/wr_total\n"
            "  (the same for the reference); -d still filters on the distance column\n"
            "  --min-copies <m> (with -g, bottom-s sketches only): -f files -- without -f, the -r files -- are sketched from the k-mers seen at\n"
            "  least m times over the whole file (read sets: `mash sketch -r -m`; -r genomes beside -f read sets are sketched as they are);\n"
            "  until <sketch> k-mers have m copies, every distinct k-mer of a file stays on the device\n"
            "  -g: one sketch per input FILE, as Mash sketches an assembly;  -d <x>: only pairs at distance <= x;  --device <id>: GPU to use\n" HASH_POLICY_HELP);
}
// the six columns of a pair of scaled sketches, without the end of the line: dist --scaled and manysearch print a pair alike
static void append_scaled_pair(OutBuf& o, const std::string& ref, const std::string& query, double d, long long sh, long long lq, long long lr) {
    o.append(ref); o.append("\t"); o.append(query);
    o.appendf("\t%.6g\t%lld/%lld\t%lld/%lld\t%lld/%lld", d, sh, lq + lr - sh, sh, lq, sh, lr);
}
static const CompareRules dist_rules = {"dist", "a distance", nullptr, false, "more than 2^31-1 sketches on one side", true};
static int dist_scaled(const CompareInputs& in, const LoadedSides& ld, int k, double max_dist) {
    ScaledRun run;
    start_scaled_run(in, dist_rules, ld, k, run);
    const ScaledSet &q = *run.queries, &sr = run.refs;
    const size_t nq = q.names.size(), nr = sr.names.size();
    if (nq > 0x7fffffffull || nr > 0x7fffffffull) refuse(dist_rules, "more than 2^31-1 sketches on one side");
    std::vector<int32_t> shared(in.abund ? 0 : nq * nr);
    std::vector<uint64_t> out4(in.abund ? nq * nr * 4 : 0), qsums, rsums; // --abund: the four sums of every pair, (sum, sumsq) of every sketch
    if (in.abund) {
        CK(rk_compare_scaled_abund(run.ctx, q.values.data(), q.abund.data(), q.off.data(), (int)nq, sr.values.data(), sr.abund.data(), sr.off.data(), (int)nr, 0, out4.data()));
        rsums.resize(nr * 2);
        CK(rk_abund_row_sums(run.ctx, sr.abund.data(), sr.off.data(), (int)nr, rsums.data()));
        if (&q != &sr) {
            qsums.resize(nq * 2);
            CK(rk_abund_row_sums(run.ctx, q.abund.data(), q.off.data(), (int)nq, qsums.data()));
        }
    } else
        CK(rk_compare_scaled(run.ctx, q.values.data(), q.off.data(), (int)nq, sr.values.data(), sr.off.data(), (int)nr, 0, shared.data()));
    const std::vector<uint64_t>& qs = &q != &sr ? qsums : rsums;
    OutBuf o(stdout);
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nr; ++j) {
            const uint64_t* w = in.abund ? &out4[(i * nr + j) * 4] : nullptr;
            const long long sh = w ? (long long)w[0] : shared[i * nr + j], lq = (long long)(q.off[i + 1] - q.off[i]), lr = (long long)(sr.off[j + 1] - sr.off[j]);
            double jac = 0, d = 1;
            CK(rk_scaled_distance(sh, lq, lr, k, &jac, &d));
            if (d > max_dist) continue;
            append_scaled_pair(o, sr.names[j], q.names[i], d, sh, lq, lr);
            if (w) {
                double angular = 0;
                CK(rk_angular_similarity(w[1], qs[i * 2 + 1], rsums[j * 2 + 1], nullptr, &angular));
                o.appendf("\t%.6g\t%llu/%llu\t%llu/%llu", angular, (unsigned long long)w[2], (unsigned long long)qs[i * 2], (unsigned long long)w[3], (unsigned long long)rsums[j * 2]);
            }
            o.append("\n");
            o.end_row();
        }
    o.flush();
    fflush(stdout);
    rk_ctx_destroy(run.ctx);
    return 0;
}
static int dist_bottom(const CompareInputs& in, LoadedSides& ld, int k, double max_dist) {
    const int S = ld.S ? ld.S : 1000;
    rk_ctx* ctx = nullptr;
    CK(rk_ctx_create(in.device, &g_policy, &ctx));
    const std::vector<int> k1(1, k);
    if (!in.ref_files.empty()) sketch_files(ctx, in.ref_files, k1, S, in.whole_files, ld.refs, in.self() ? in.min_copies : 1); // (genomes hold most k-mers once: --min-copies is for the read sets)
    if (!in.query_files.empty()) sketch_files(ctx, in.query_files, k1, S, in.whole_files, ld.queries, in.min_copies);
    const SketchSet &refs = ld.refs, &q = in.self() ? ld.refs : ld.queries;
    const size_t nq = q.names.size(), nr = refs.names.size();
    if (nr == 0 || nq == 0) refuse(dist_rules, std::string("no ") + (nr == 0 ? "reference" : "query") + " sketches");
    if (nq > 0x7fffffffull || nr > 0x7fffffffull) refuse(dist_rules, "more than 2^31-1 sketches on one side");
    std::vector<int32_t> out4(nq * nr * 4);
    CK(rk_compare_sketches(ctx, q.sk.data(), q.lens.data(), (int)nq, refs.sk.data(), refs.lens.data(), (int)nr, S, out4.data()));
    OutBuf o(stdout);
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nr; ++j) {
            const int32_t* r = &out4[(i * nr + j) * 4];
            double jac = 0, d = 1;
            CK(rk_mash_distance(r[2], r[3], k, &jac, &d));
            if (d > max_dist) continue;
            o.append(refs.names[j]); o.append("\t"); o.append(q.names[i]);
            o.appendf("\t%.6g\t%d/%d\t%d\n", d, r[2], r[3], r[0]);
            o.end_row();
        }
    o.flush();
    fflush(stdout);
    rk_ctx_destroy(ctx);
    return 0;
}
int main_dist(int argc, char** argv) {
    CompareInputs in;
    double max_dist = 2.0;
    if (argc <= 2) { help_dist(); exit(1); }
    static struct option long_options[] = {COMPARE_OPTIONS, {"max-dist", required_argument, 0, 'd'}, {"threads", required_argument, 0, 't'}, {"abund", no_argument, 0, 1008}, {"min-copies", required_argument, 0, 1012}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:d:t:", long_options, nullptr)) != -1) {
        if (shared_option(c, in)) continue;
        switch (c) {
            case 'd': max_dist = atof(optarg); break;
            case 't': break;
            case 1008: in.abund = true; break;
            case 1012: if (!parse_min_copies(optarg, in.min_copies)) in.min_copies = 0; break;
            default: help_dist(); exit(1);
        }
    }
    LoadedSides ld;
    ld.k = one_k(in, dist_rules);
    if (in.scaled_given && !in.scaled_ok) refuse(dist_rules, "--scaled takes a number of at least 1");
    if (in.scaled_given && in.S != 0) refuse(dist_rules, "--scaled and -s are two kinds of sketch; give one of them");
    if (in.abund && in.S != 0) refuse(dist_rules, "--abund compares scaled sketches (--scaled <n>, or files of `rkmh sketch --scaled <n> --abund`); -s makes bottom-s ones, which keep no abundances");
    if (in.S != 0 && (in.S < 1 || in.S > RK_MAX_SKETCH)) refuse(dist_rules, "sketch size outside 1 .. " + std::to_string(RK_MAX_SKETCH));
    if (in.ref_files.empty() == in.ref_json.empty()) refuse(dist_rules, "references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (!in.query_files.empty() && !in.query_json.empty()) refuse(dist_rules, "queries come from -f <fasta|fastq> ... or from -Q <sketches.json> ..., not both");
    if (in.whole_files && in.ref_files.empty() && in.query_files.empty()) refuse(dist_rules, "-g says how -r / -f files are sketched; sketches loaded with -R / -Q are what they are");
    refuse_min_copies("dist", in.min_copies, in.whole_files, in.scaled_given);
    load_sketch_files(in, dist_rules, ld);
    refuse_min_copies("dist", in.min_copies, in.whole_files, ld.largest_scaled != 0);
    if (in.abund && !in.scaled_given && ld.largest_scaled == 0)
        refuse(dist_rules, "--abund compares scaled sketches: give --scaled <n>, or -R / -Q files of `rkmh sketch --scaled <n> --abund`");
    const int k = run_k(dist_rules, ld.k);
    return in.scaled_given || ld.largest_scaled ? dist_scaled(in, ld, k, max_dist) : dist_bottom(in, ld, k, max_dist);
}

// ------------------------------------------------------------------------------------------------------------------------
// gather: which references make up a sample, and how much of it each explains once the better matches are taken out (include/
// rkmh_amd.h, "GATHER").  References and queries are scaled sketches, made or loaded as `dist --scaled` makes and loads them; the
// references go to the device once, the queries are gathered against them one after the other (rk_gather_scaled_device).
// Everything that can be refused is refused before a context exists.
static void help_gather() {
    fprintf(stderr,
            "rkmh gather (-r <refs.fa> ... | -R <refs.json> ...) (-f <sample.fa|fq[.gz]> ... | -Q <queries.json> ...) [-k <k>] [--scaled <n>] [-g]\n"
            "            [--min-shared <n>] [--max-rounds <n>] [--abund] [--device <id>]\n"
            "  decomposes every query into references, greedily: the reference that holds most of what is left of the query is printed and\n"
            "  its hashes leave the query, until the best reference holds fewer than --min-shared (default 1) of them or --max-rounds lines\n"
            "  are printed; one line per pick, query by query: query, rank (from 1), reference, unique/|query| (hashes only this pick\n"
            "  explains at its turn), total/|query|, total/|reference| (total: all hashes the two share), remaining (hashes of the query\n"
            "  left unexplained); a query that no reference matches prints nothing\n"
            "  -f: every file is ONE query, the union of its records (a sample is a file of reads);  -Q: every sketch of the file is a query\n"
            "  -r: one reference per record, with -g one per FILE;  -R / -Q: scaled sketches written by `rkmh sketch --scaled <m>`\n"
            "  --scaled <n>: -r / -f files are sketched at n, -R / -Q files (m <= n) are cut down to n; without it: the largest m among the\n"
            "  files; not with -s (bottom-s sketches cannot be decomposed)\n"
            "  --abund: the query keeps how many of its windows hash to each value (-f files are sketched so, summed over a file's records;\n"
            "  -Q files must come from `rkmh sketch --scaled <m> --abund`); the picks are the same, every line gains two columns:\n"
            "  wunique/wtotal (the windows behind the hashes only this pick explains at its turn / all windows the query kept) and the mean\n"
            "  abundance of those hashes, wunique / unique; abundances in -R files are ignored\n" HASH_POLICY_HELP);
}
static const CompareRules gather_rules = {"gather", "gather", "gather decomposes scaled ones (rkmh sketch --scaled)", true, nullptr};
// what gather and multigather share: the switches, the refusals (all before a context exists), the run's two sides
struct GatherRun {
    CompareInputs in;
    int min_shared = 1, max_rounds = 0x7fffffff, k = 0;
    LoadedSides ld;
    ScaledRun run;
};
static void start_gather_run(int argc, char** argv, const CompareRules& rules, void (*help)(), GatherRun& g) {
    CompareInputs& in = g.in;
    int &min_shared = g.min_shared, &max_rounds = g.max_rounds;
    bool min_ok = true, rounds_ok = true;
    if (argc <= 2) { help(); exit(1); }
    static struct option long_options[] = {COMPARE_OPTIONS, {"min-shared", required_argument, 0, 1006}, {"max-rounds", required_argument, 0, 1007}, {"abund", no_argument, 0, 1008}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:", long_options, nullptr)) != -1) {
        if (shared_option(c, in)) continue;
        switch (c) {
            case 1006: min_ok = parse_at_least_1(optarg, min_shared); break;
            case 1007: rounds_ok = parse_at_least_1(optarg, max_rounds); break;
            case 1008: in.abund = true; break;
            default: help(); exit(1);
        }
    }
    LoadedSides& ld = g.ld;
    ld.k = one_k(in, rules);
    if (in.S != 0) refuse(rules, "-s makes bottom-s sketches, which cannot be decomposed; gather works on scaled ones (--scaled)");
    if (in.scaled_given && !in.scaled_ok) refuse(rules, "--scaled takes a number of at least 1");
    if (!min_ok) refuse(rules, "--min-shared takes a number of at least 1");
    if (!rounds_ok) refuse(rules, "--max-rounds takes a number of at least 1");
    if (in.ref_files.empty() == in.ref_json.empty()) refuse(rules, "references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (in.query_files.empty() == in.query_json.empty()) refuse(rules, "queries come from -f <fasta|fastq> ... or from -Q <sketches.json> ..., one of the two");
    if (in.whole_files && in.ref_files.empty()) refuse(rules, "-g says how -r files are sketched; sketches loaded with -R are what they are");
    load_sketch_files(in, rules, ld);
    if (!in.scaled_given && ld.largest_scaled == 0) refuse(rules, "no sketch file says at which scaled to sketch: give --scaled <n>");
    g.k = run_k(rules, ld.k);
    start_scaled_run(in, rules, ld, g.k, g.run);
    const ScaledSet &sr = g.run.refs, &sq = *g.run.queries;
    if (sr.names.size() > 0x7fffffffull) refuse(rules, "more than 2^31-1 reference sketches");
    for (size_t i = 0; i < sq.names.size(); ++i)
        if (sq.off[i + 1] - sq.off[i] > 0x7fffffffull) refuse(rules, "a query of more than 2^31-1 hashes");
}
// the lines of one query: its n rows (ref, unique, total, remaining), with wunique and the query's wtotal when the run carries abundances
static void append_gather_rows(OutBuf& o, const char* cmd, const ScaledSet& sq, size_t i, const ScaledSet& sr, const int32_t* out4, int n, const uint64_t* wunique,
                               uint64_t wtotal) {
    const size_t nr = sr.names.size();
    const uint64_t lq = sq.off[i + 1] - sq.off[i];
    for (int t = 0; t < n; ++t) {
        const int32_t* r = &out4[(size_t)t * 4];
        const size_t ref = (size_t)r[0];
        if (ref >= nr) { fprintf(stderr, "rkmh %s: row %d names reference %d of %zu\n", cmd, t, r[0], nr); exit(1); }
        o.append(sq.names[i]);
        o.appendf("\t%d\t", t + 1);
        o.append(sr.names[ref]);
        o.appendf("\t%d/%llu\t%d/%llu\t%d/%llu\t%d", r[1], (unsigned long long)lq, r[2], (unsigned long long)lq, r[2], (unsigned long long)(sr.off[ref + 1] - sr.off[ref]), r[3]);
        if (wunique) o.appendf("\t%llu/%llu\t%.6g", (unsigned long long)wunique[(size_t)t], (unsigned long long)wtotal, (double)wunique[(size_t)t] / (double)r[1]);
        o.append("\n");
    }
    o.end_row();
}
int main_gather(int argc, char** argv) {
    GatherRun g;
    start_gather_run(argc, argv, gather_rules, help_gather, g);
    const CompareInputs& in = g.in;
    const int min_shared = g.min_shared, max_rounds = g.max_rounds;
    rk_ctx* ctx = g.run.ctx;
    const ScaledSet &sr = g.run.refs, &sq = *g.run.queries;
    const size_t nq = sq.names.size(), nr = sr.names.size();
    // the references go to the device once; every query follows them into the same two arrays
    uint64_t longest = 0;
    for (size_t i = 0; i < nq; ++i) longest = std::max(longest, sq.off[i + 1] - sq.off[i]);
    const int rows = (int)std::min<size_t>((size_t)max_rounds, nr);
    void *d_rv = nullptr, *d_ro = nullptr, *d_q = nullptr, *d_out = nullptr, *d_qa = nullptr, *d_wu = nullptr;
    CK(rk_device_alloc(ctx, sr.values.size() * 8, &d_rv));
    CK(rk_device_alloc(ctx, sr.off.size() * 8, &d_ro));
    CK(rk_device_alloc(ctx, (size_t)longest * 8, &d_q));
    CK(rk_device_alloc(ctx, (size_t)rows * 16, &d_out));
    if (in.abund) {
        CK(rk_device_alloc(ctx, (size_t)longest * 4, &d_qa));
        CK(rk_device_alloc(ctx, (size_t)rows * 8, &d_wu));
    }
    std::vector<uint64_t> wunique((size_t)(in.abund ? rows : 0));
    CK(rk_device_upload(ctx, d_rv, sr.values.data(), sr.values.size() * 8));
    CK(rk_device_upload(ctx, d_ro, sr.off.data(), sr.off.size() * 8));
    std::vector<int32_t> out4((size_t)rows * 4);
    OutBuf o(stdout);
    for (size_t i = 0; i < nq; ++i) {
        const uint64_t lq = sq.off[i + 1] - sq.off[i];
        int n = 0;
        CK(rk_device_upload(ctx, d_q, sq.values.data() + sq.off[i], (size_t)lq * 8));
        uint64_t wtotal = 0;
        if (in.abund) {
            const uint32_t* qa = sq.abund.data() + sq.off[i];
            for (uint64_t j = 0; j < lq; ++j) wtotal += qa[j];
            CK(rk_device_upload(ctx, d_qa, qa, (size_t)lq * 4));
            CK(rk_gather_scaled_abund_device(ctx, d_q, d_qa, lq, d_rv, d_ro, (int)nr, sr.values.size(), min_shared, rows, d_out, d_wu, &n, rk_ctx_stream(ctx)));
            CK(rk_device_download(ctx, wunique.data(), d_wu, (size_t)n * 8));
        } else
            CK(rk_gather_scaled_device(ctx, d_q, lq, d_rv, d_ro, (int)nr, sr.values.size(), min_shared, rows, d_out, &n, rk_ctx_stream(ctx)));
        CK(rk_device_download(ctx, out4.data(), d_out, (size_t)n * 16));
        append_gather_rows(o, "gather", sq, i, sr, out4.data(), n, in.abund ? wunique.data() : nullptr, wtotal);
    }
    o.flush();
    fflush(stdout);
    for (void* p : {d_rv, d_ro, d_q, d_out, d_qa, d_wu}) if (p) rk_device_free(ctx, p);
    rk_ctx_destroy(ctx);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// multigather: gather for all queries at once (include/rkmh_amd.h, "MULTIGATHER").  The switches, the refusals and the lines are
// gather's; the references become one resident inverted index (rk_scaled_index_create) and the queries go through
// rk_multigather_scaled in as few calls as its limits allow -- queries do not influence each other, so the lines do not depend on
// where the batch is cut.
static void help_multigather() {
    fprintf(stderr,
            "rkmh multigather (-r <refs.fa> ... | -R <refs.json> ...) (-f <sample.fa|fq[.gz]> ... | -Q <queries.json> ...) [-k <k>] [--scaled <n>] [-g]\n"
            "                 [--min-shared <n>] [--max-rounds <n>] [--abund] [--device <id>]\n"
            "  `rkmh gather` for many queries at once: the same switches, the same lines, byte for byte; the references become one resident\n"
            "  inverted index (hash -> the references that hold it) and all queries are decomposed together, a round of picks for the whole\n"
            "  batch at a time, so the work follows the hashes the queries share with the references, not queries x references\n"
            "  -f: every file is ONE query, the union of its records;  -Q: every sketch of the file is a query;  -r / -R, -g, --scaled,\n"
            "  --min-shared, --max-rounds, --abund: as for `rkmh gather`\n" HASH_POLICY_HELP);
}
static const CompareRules multigather_rules = {"multigather", "multigather", "multigather decomposes scaled ones (rkmh sketch --scaled)", true, nullptr};
int main_multigather(int argc, char** argv) {
    GatherRun g;
    start_gather_run(argc, argv, multigather_rules, help_multigather, g);
    rk_ctx* ctx = g.run.ctx;
    const ScaledSet &sr = g.run.refs, &sq = *g.run.queries;
    const size_t nq = sq.names.size(), nr = sr.names.size();
    rk_scaled_index* idx = nullptr;
    CK(rk_scaled_index_create(ctx, sr.values.data(), sr.off.data(), (int64_t)nr, &idx));
    // queries per call: the search's workgroup limit (queries x reference blocks below 2^24), and at most 2^31 - 1 candidates, of
    // which a query has nr at most
    const uint64_t nblk = (nr + RK_SEARCH_REF_BLOCK - 1) / RK_SEARCH_REF_BLOCK;
    const size_t per_call = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(0xffffffull / nblk, 0x7fffffffull / nr));
    std::vector<uint64_t> row_off;
    OutBuf o(stdout);
    for (size_t q0 = 0; q0 < nq; q0 += per_call) {
        const size_t n = std::min(per_call, nq - q0);
        row_off.assign(n + 1, 0);
        int32_t* rows = nullptr;
        uint64_t* wunique = nullptr;
        uint64_t nrows = 0;
        CK(rk_multigather_scaled(ctx, idx, sq.values.data(), g.in.abund ? sq.abund.data() : nullptr, sq.off.data() + q0, (int64_t)n, g.min_shared, g.max_rounds,
                                 &rows, &wunique, row_off.data(), &nrows));
        for (size_t i = 0; i < n; ++i) {
            const uint64_t a = row_off[i], b = row_off[i + 1];
            if (a > b || b > nrows || b - a > nr) { fprintf(stderr, "rkmh multigather: query %zu has rows %llu .. %llu of %llu\n", q0 + i, (unsigned long long)a, (unsigned long long)b, (unsigned long long)nrows); exit(1); }
            uint64_t wtotal = 0;
            if (g.in.abund)
                for (uint64_t j = sq.off[q0 + i]; j < sq.off[q0 + i + 1]; ++j) wtotal += sq.abund[j];
            append_gather_rows(o, "multigather", sq, q0 + i, sr, rows + a * 4, (int)(b - a), g.in.abund ? wunique + a : nullptr, wtotal);
        }
        rk_free(rows);
        if (wunique) rk_free(wunique);
    }
    o.flush();
    fflush(stdout);
    rk_scaled_index_destroy(idx);
    rk_ctx_destroy(ctx);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------
// manysearch: many queries against a collection of references, only the pairs that match (include/rkmh_amd.h, "SEARCH").  Both sides
// are scaled sketches, made or loaded as `dist --scaled` makes and loads them; the references become a resident inverted index once
// (rk_scaled_index_create), the queries are searched against it in one call (rk_search_scaled).  Host memory is the two sides and
// the hits, never queries x references.  Everything that can be refused is refused before a context exists.
static void help_manysearch() {
    fprintf(stderr,
            "rkmh manysearch (-r <refs.fa> ... | -R <refs.json> ...) (-f <queries.fa|fq> ... | -Q <queries.json> ...) [-k <k>] [--scaled <n>] [-g]\n"
            "                [--min-shared <n>] [--min-containment <x>] [--device <id>]\n"
            "  searches every query sketch against every reference sketch through an inverted index of the references (hash -> the references\n"
            "  that hold it) and prints only the pairs that match: one line per pair that shares at least --min-shared hashes (default 1),\n"
            "  query by query, references in input order, in the six columns of `dist --scaled`: reference, query, distance from\n"
            "  shared/union, shared/union, shared/|query|, shared/|reference|; a line is the line `dist --scaled` prints for that pair\n"
            "  --min-containment <x> (0 .. 1, default 0): only pairs with shared/|query| >= x as well: the query's threshold is the larger of\n"
            "  --min-shared and the smallest count t with t / |query| >= x; an empty query matches nothing\n"
            "  -r: one reference per record, with -g one per FILE;  -f: one query per record, with -g one per FILE; without -f / -Q the\n"
            "  references are searched against themselves;  -R / -Q: scaled sketches written by `rkmh sketch --scaled <m>`\n"
            "  --scaled <n>: -r / -f files are sketched at n, -R / -Q files (m <= n) are cut down to n; without it: the largest m among the\n"
            "  files; not with -s (bottom-s sketches) and not with --abund (abundances play no part in a search)\n" HASH_POLICY_HELP);
}
static const CompareRules manysearch_rules = {"manysearch", "manysearch", "manysearch searches scaled ones (rkmh sketch --scaled)", false,
                                              "more than 2^31-1 sketches on one side"};
int main_manysearch(int argc, char** argv) {
    CompareInputs in;
    int min_shared = 1;
    bool min_ok = true, cont_ok = true, abund = false;
    double min_cont = 0.0;
    if (argc <= 2) { help_manysearch(); exit(1); }
    static struct option long_options[] = {COMPARE_OPTIONS, {"min-shared", required_argument, 0, 1006}, {"abund", no_argument, 0, 1008},
                                           {"min-containment", required_argument, 0, 1009}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:", long_options, nullptr)) != -1) {
        if (shared_option(c, in)) continue;
        switch (c) {
            case 1006: min_ok = parse_at_least_1(optarg, min_shared); break;
            case 1008: abund = true; break;
            case 1009: {
                char* e = nullptr;
                min_cont = strtod(optarg, &e);
                cont_ok = e != optarg && *e == 0 && min_cont >= 0.0 && min_cont <= 1.0; // (a NaN fails both comparisons)
                break;
            }
            default: help_manysearch(); exit(1);
        }
    }
    LoadedSides ld;
    ld.k = one_k(in, manysearch_rules);
    if (in.S != 0) refuse(manysearch_rules, "-s makes bottom-s sketches; manysearch works on scaled ones (--scaled)");
    if (abund) refuse(manysearch_rules, "--abund has no meaning here: a search counts shared hashes, abundances play no part");
    if (in.scaled_given && !in.scaled_ok) refuse(manysearch_rules, "--scaled takes a number of at least 1");
    if (!min_ok) refuse(manysearch_rules, "--min-shared takes a number of at least 1");
    if (!cont_ok) refuse(manysearch_rules, "--min-containment takes a number from 0 to 1");
    if (in.ref_files.empty() == in.ref_json.empty()) refuse(manysearch_rules, "references come from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (!in.query_files.empty() && !in.query_json.empty()) refuse(manysearch_rules, "queries come from -f <fasta|fastq> ... or from -Q <sketches.json> ..., not both");
    if (in.whole_files && in.ref_files.empty() && in.query_files.empty()) refuse(manysearch_rules, "-g says how -r / -f files are sketched; sketches loaded with -R / -Q are what they are");
    load_sketch_files(in, manysearch_rules, ld);
    if (!in.scaled_given && ld.largest_scaled == 0) refuse(manysearch_rules, "no sketch file says at which scaled to sketch: give --scaled <n>");
    const int k = run_k(manysearch_rules, ld.k);
    ScaledRun run;
    start_scaled_run(in, manysearch_rules, ld, k, run);
    const ScaledSet &q = *run.queries, &sr = run.refs;
    const size_t nq = q.names.size(), nr = sr.names.size();
    if (nq > 0x7fffffffull || nr > 0x7fffffffull) refuse(manysearch_rules, "more than 2^31-1 sketches on one side");
    std::vector<int32_t> q_min(nq, 1); // per query: the count that --min-containment asks of it
    for (size_t i = 0; i < nq; ++i) {
        const uint64_t lq = q.off[i + 1] - q.off[i];
        if (lq > 0x7fffffffull) refuse(manysearch_rules, "a query of more than 2^31-1 hashes");
        int32_t t = 0;
        CK(rk_search_min_count(min_cont, lq, &t));
        q_min[i] = std::max(t, 1);
    }
    rk_scaled_index* idx = nullptr;
    CK(rk_scaled_index_create(run.ctx, sr.values.data(), sr.off.data(), (int64_t)nr, &idx));
    rk_search_hit* hits = nullptr;
    uint64_t nhits = 0;
    CK(rk_search_scaled(run.ctx, idx, q.values.data(), q.off.data(), (int64_t)nq, min_shared, q_min.data(), &hits, &nhits));
    OutBuf o(stdout);
    for (uint64_t h = 0; h < nhits; ++h) {
        const size_t i = (size_t)hits[h].query, j = (size_t)hits[h].ref;
        if (i >= nq || j >= nr) { fprintf(stderr, "rkmh manysearch: hit %llu names query %d and reference %d of %zu x %zu\n", (unsigned long long)h, hits[h].query, hits[h].ref, nq, nr); exit(1); }
        const long long sh = hits[h].shared, lq = (long long)(q.off[i + 1] - q.off[i]), lr = (long long)(sr.off[j + 1] - sr.off[j]);
        double jac = 0, d = 1;
        CK(rk_scaled_distance(sh, lq, lr, k, &jac, &d));
        append_scaled_pair(o, sr.names[j], q.names[i], d, sh, lq, lr);
        o.append("\n");
        o.end_row();
    }
    o.flush();
    fflush(stdout);
    rk_free(hits);
    rk_scaled_index_destroy(idx);
    rk_ctx_destroy(run.ctx);
    return 0;
}
