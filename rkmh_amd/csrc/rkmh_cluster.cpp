// rkmh_cluster.cpp -- `rkmh cluster`: the single-linkage clusters of a collection of scaled sketches (include/rkmh_amd.h, "CLUSTER").
// The collection is made or loaded as manysearch makes and loads its reference side, becomes a resident inverted index once
// (rk_scaled_index_create) and is searched against itself and clustered in one call (rk_cluster_scaled): the hits stay on the device,
// host memory is the collection and one label per sketch.  Everything that can be refused is refused before a context exists.
#include <algorithm>

#include "rkmh_cli.hpp"

static void help_cluster() {
    fprintf(stderr,
            "rkmh cluster (-r <refs.fa> ... | -R <refs.json> ...) [-g] [-k <k>] [--scaled <n>] [--min-shared <n>]\n"
            "             [--min-jaccard <x> | --min-max-containment <x>] [--representatives] [--device <id>]\n"
            "  groups the sketches of a collection into single-linkage clusters: two sketches are linked when they share at least\n"
            "  --min-shared hashes (default 1) and their similarity is at least x; a cluster is everything reachable over links\n"
            "  --min-jaccard <x>: shared/union >= x (the default, with x = 0: any pair sharing --min-shared hashes links)\n"
            "  --min-max-containment <x>: shared/min(|a|, |b|) >= x;  x is a decimal from 0 to 1 with at most six digits after the point\n"
            "  prints one line per sketch: cluster, size, representative, member, |member|; clusters in the order of their first member,\n"
            "  numbered from 0, members in input order; the representative is the member with the most hashes (the first of equals)\n"
            "  --representatives: one line per cluster instead: cluster, size, representative, |representative|\n"
            "  -r: one sketch per record, with -g one per FILE;  -R: scaled sketches written by `rkmh sketch --scaled <m>`\n"
            "  --scaled <n>: -r files are sketched at n, -R files (m <= n) are cut down to n; without it: the largest m among the files;\n"
            "  not with -f / -Q (one collection is clustered), -s (bottom-s sketches) or --abund (abundances play no part)\n" HASH_POLICY_HELP);
}
static const CompareRules cluster_rules = {"cluster", "cluster", "cluster groups scaled ones (rkmh sketch --scaled)", false,
                                           "more than 2^31-1 sketches on one side"};

// a decimal from 0 to 1 with at most six digits after the point -> parts per million, exactly; anything else: false
static bool parse_ppm(const char* text, uint32_t& ppm) {
    const char* p = text;
    uint32_t whole = 0, frac = 0;
    int nwhole = 0, nfrac = 0;
    for (; *p >= '0' && *p <= '9'; ++p, ++nwhole) {
        if (nwhole >= 1) return false; // one digit before the point: 0 or 1
        whole = (uint32_t)(*p - '0');
    }
    if (*p == '.') {
        for (++p; *p >= '0' && *p <= '9'; ++p, ++nfrac) {
            if (nfrac >= 6) return false;
            frac = frac * 10 + (uint32_t)(*p - '0');
        }
    }
    if (*p != 0 || nwhole + nfrac == 0 || whole > 1) return false;
    for (; nfrac < 6; ++nfrac) frac *= 10;
    if (whole == 1 && frac != 0) return false;
    ppm = whole * 1000000u + frac;
    return true;
}

int main_cluster(int argc, char** argv) {
    CompareInputs in;
    int min_shared = 1;
    bool min_ok = true, x_ok = true, abund = false, reps_only = false, jaccard_given = false, cont_given = false;
    uint32_t min_ppm = 0;
    if (argc <= 2) { help_cluster(); exit(1); }
    static struct option long_options[] = {COMPARE_OPTIONS, {"min-shared", required_argument, 0, 1006}, {"abund", no_argument, 0, 1008},
                                           {"min-jaccard", required_argument, 0, 1010}, {"min-max-containment", required_argument, 0, 1011},
                                           {"representatives", no_argument, 0, 1012}, {0, 0, 0, 0}};
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, "hgk:f:r:R:Q:s:", long_options, nullptr)) != -1) {
        if (shared_option(c, in)) continue;
        switch (c) {
            case 1006: min_ok = parse_at_least_1(optarg, min_shared); break;
            case 1008: abund = true; break;
            case 1010: jaccard_given = true; x_ok = parse_ppm(optarg, min_ppm) && x_ok; break;
            case 1011: cont_given = true; x_ok = parse_ppm(optarg, min_ppm) && x_ok; break;
            case 1012: reps_only = true; break;
            default: help_cluster(); exit(1);
        }
    }
    LoadedSides ld;
    ld.k = one_k(in, cluster_rules);
    if (!in.query_files.empty() || !in.query_json.empty()) refuse(cluster_rules, "-f / -Q have no meaning here: one collection is clustered, given with -r or -R");
    if (in.S != 0) refuse(cluster_rules, "-s makes bottom-s sketches; cluster works on scaled ones (--scaled)");
    if (abund) refuse(cluster_rules, "--abund has no meaning here: a link counts shared hashes, abundances play no part");
    if (in.scaled_given && !in.scaled_ok) refuse(cluster_rules, "--scaled takes a number of at least 1");
    if (!min_ok) refuse(cluster_rules, "--min-shared takes a number of at least 1");
    if (jaccard_given && cont_given) refuse(cluster_rules, "--min-jaccard and --min-max-containment are two measures: give one of the two");
    if (!x_ok) refuse(cluster_rules, "--min-jaccard and --min-max-containment take a decimal from 0 to 1 with at most six digits after the point");
    if (in.ref_files.empty() == in.ref_json.empty()) refuse(cluster_rules, "the collection comes from -r <fasta> ... or from -R <sketches.json> ..., one of the two");
    if (in.whole_files && in.ref_files.empty()) refuse(cluster_rules, "-g says how -r files are sketched; sketches loaded with -R are what they are");
    load_sketch_files(in, cluster_rules, ld);
    if (!in.scaled_given && ld.largest_scaled == 0) refuse(cluster_rules, "no sketch file says at which scaled to sketch: give --scaled <n>");
    const int k = run_k(cluster_rules, ld.k);
    ScaledRun run;
    start_scaled_run(in, cluster_rules, ld, k, run);
    const ScaledSet& sr = run.refs;
    const size_t n = sr.names.size();
    if (n < 1) refuse(cluster_rules, "the collection holds no sketch");
    if (n > 0x7fffffffull) refuse(cluster_rules, "more than 2^31-1 sketches on one side");
    std::vector<uint64_t> lens(n);
    for (size_t i = 0; i < n; ++i) lens[i] = sr.off[i + 1] - sr.off[i];
    rk_scaled_index* idx = nullptr;
    CK(rk_scaled_index_create(run.ctx, sr.values.data(), sr.off.data(), (int64_t)n, &idx));
    std::vector<int32_t> labels(n), cl_off(n + 1), members(n), rep(n);
    CK(rk_cluster_scaled(run.ctx, idx, sr.values.data(), sr.off.data(), (int64_t)n, min_shared, cont_given ? RK_CLUSTER_MAX_CONTAINMENT : RK_CLUSTER_JACCARD,
                         min_ppm, 0, labels.data()));
    int64_t ncl = 0;
    CK(rk_cluster_members(labels.data(), lens.data(), (int64_t)n, &ncl, cl_off.data(), members.data(), rep.data()));
    OutBuf o(stdout);
    for (int64_t cl = 0; cl < ncl; ++cl) {
        const int32_t size = cl_off[cl + 1] - cl_off[cl];
        const std::string head = std::to_string(cl) + "\t" + std::to_string(size) + "\t" + sr.names[(size_t)rep[cl]] + "\t";
        if (reps_only) {
            o.append(head + std::to_string(lens[(size_t)rep[cl]]) + "\n");
            o.end_row();
            continue;
        }
        for (int32_t m = cl_off[cl]; m < cl_off[cl + 1]; ++m) {
            const size_t i = (size_t)members[m];
            o.append(head + sr.names[i] + "\t" + std::to_string(lens[i]) + "\n");
            o.end_row();
        }
    }
    o.flush();
    fflush(stdout);
    rk_scaled_index_destroy(idx);
    rk_ctx_destroy(run.ctx);
    return 0;
}
