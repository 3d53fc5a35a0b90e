// rkmh_sketches.cpp -- sketch sets, and everything sketch, dist and gather do to them that is not a command: made from sequence files,
// written as JSON (read back: rkmh_sketch_json.cpp), loaded from -R / -Q files under the checks of a comparison, cut down to one scaled.
#include <algorithm>
#include <cerrno>

#include "rkmh_cli.hpp"
#include "rkmh_min_copies.hpp"

// ---- from sequence files.  The walk both kinds share: all(s) makes a sketch of every record of s, one(s) ONE sketch of all of them.
template <class All, class One>
static void walk_files(const std::vector<const char*>& files, bool whole_files, std::vector<std::string>& names, std::vector<uint64_t>& seq_len, All all, One one) {
    if (!whole_files) {
        rk_seqset s;
        CK(rk_parse_files(files.data(), (int)files.size(), &s));
        all(s);
        for (int64_t i = 0; i < s.nseq; ++i) {
            names.push_back(s.names + s.name_offsets[i]);
            seq_len.push_back(s.offsets[i + 1] - s.offsets[i]);
        }
        rk_seqset_free(&s);
        return;
    }
    for (size_t f = 0; f < files.size(); ++f) {
        rk_seqset s;
        CK(rk_parse_files(&files[f], 1, &s));
        if (s.nseq > 0x7fffffffll) { fprintf(stderr, "rkmh: %s holds more than 2^31-1 records\n", files[f]); exit(1); }
        one(s);
        names.push_back(files[f]);
        seq_len.push_back(s.nseq ? s.offsets[s.nseq] - s.offsets[0] : 0);
        rk_seqset_free(&s);
    }
}
void sketch_files(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, int S, bool whole_files, SketchSet& out, uint64_t min_copies) {
    if (whole_files && sample_on_device()) { // one sketch per file: a bottom sample on the device, no file held whole (rkmh_sample.cpp)
        rk_sample* sample = nullptr;
        CK(rk_sample_create_bottom(ctx, ks.data(), (int)ks.size(), S, min_copies, 0, &sample));
        for (const char* f : files) {
            const SampleFed fed = sample_file_feed(ctx, sample, f);
            out.sk.resize(out.sk.size() + (size_t)S, 0);
            out.lens.push_back(0);
            CKE(rk_sample_finish_bottom(sample, &out.sk[out.sk.size() - (size_t)S], &out.lens.back()), f);
            uint64_t threshold = 0, candidates = 0, weight = 0, nbases = 0;
            uint32_t cuts = 0;
            CKE(rk_sample_bottom_state(sample, &threshold, &candidates, &weight, &cuts), f);
            sample_file_done(sample, f, fed, &nbases);
            if (g_timing)
                fprintf(stderr, "[rkmh timing] bottom sample %s: sketch size %d, min copies %llu: threshold %llu, %llu candidates of weight %llu, %u cuts\n", f, S,
                        (unsigned long long)min_copies, (unsigned long long)threshold, (unsigned long long)candidates, (unsigned long long)weight, cuts);
            out.names.push_back(f);
            out.seq_len.push_back(nbases);
        }
        rk_sample_destroy(sample);
        return;
    }
    auto batch = [&](const rk_seqset& s, std::vector<uint64_t>& sk, std::vector<int32_t>& lens) {
        sk.assign((size_t)s.nseq * (size_t)S, 0);
        lens.assign((size_t)s.nseq, 0);
        CK(rk_sketch_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), S, sk.data(), lens.data()));
    };
    std::vector<uint64_t> sk;
    std::vector<int32_t> lens;
    walk_files(files, whole_files, out.names, out.seq_len, [&](const rk_seqset& s) { batch(s, out.sk, out.lens); },
               [&](const rk_seqset& s) {
                   batch(s, sk, lens);
                   out.sk.resize(out.sk.size() + (size_t)S, 0);
                   out.lens.push_back(0);
                   CK(rk_merge_sketches(sk.data(), lens.data(), (int)s.nseq, S, rk_policy_dedup(&g_policy), &out.sk[out.sk.size() - (size_t)S], &out.lens.back()));
               });
}
void sketch_files_scaled(rk_ctx* ctx, const std::vector<const char*>& files, const std::vector<int>& ks, uint64_t max_hash, bool whole_files, ScaledSet& out) {
    if (whole_files && sample_on_device()) { // one sketch per file: accumulated on the device, no file held whole (rkmh_sample.cpp)
        rk_sample* sample = nullptr;
        CK(rk_sample_create(ctx, ks.data(), (int)ks.size(), max_hash, out.with_abund ? 1 : 0, 0, &sample));
        for (const char* f : files) {
            uint64_t *v = nullptr, n = 0, nbases = 0;
            uint32_t* a = nullptr;
            const SampleFed fed = sample_file_feed(ctx, sample, f);
            CKE(rk_sample_finish(sample, &v, &a, &n), f);
            sample_file_done(sample, f, fed, &nbases);
            out.values.insert(out.values.end(), v, v + n);
            if (out.with_abund) out.abund.insert(out.abund.end(), a, a + n);
            out.off.push_back(out.values.size());
            out.names.push_back(f);
            out.seq_len.push_back(nbases);
            rk_free(v);
            rk_free(a);
        }
        rk_sample_destroy(sample);
        return;
    }
    std::vector<uint64_t> off;
    auto batch = [&](const rk_seqset& s, uint64_t** v, uint32_t** a) {
        off.assign((size_t)s.nseq + 1, 0);
        if (out.with_abund) CK(rk_sketch_scaled_abund_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), max_hash, v, a, off.data()));
        else CK(rk_sketch_scaled_batch(ctx, s.bases, s.offsets, s.nseq, ks.data(), (int)ks.size(), max_hash, v, off.data()));
    };
    auto row = [&](const uint64_t* b, const uint64_t* e, const uint32_t* a) {
        out.values.insert(out.values.end(), b, e);
        if (out.with_abund) out.abund.insert(out.abund.end(), a, a + (e - b));
        out.off.push_back(out.values.size());
    };
    walk_files(files, whole_files, out.names, out.seq_len,
               [&](const rk_seqset& s) {
                   uint64_t* v = nullptr;
                   uint32_t* a = nullptr;
                   batch(s, &v, &a);
                   for (int64_t i = 0; i < s.nseq; ++i) row(v + off[(size_t)i], v + off[(size_t)i + 1], a ? a + off[(size_t)i] : nullptr);
                   rk_free(v);
                   rk_free(a);
               },
               [&](const rk_seqset& s) {
                   uint64_t *v = nullptr, *u = nullptr;
                   uint32_t *a = nullptr, *ua = nullptr;
                   uint64_t nu = 0;
                   batch(s, &v, &a);
                   if (out.with_abund) CK(rk_merge_scaled_abund(v, a, off.data(), (int)s.nseq, max_hash, &u, &ua, &nu));
                   else CK(rk_merge_scaled(v, off.data(), (int)s.nseq, max_hash, &u, &nu));
                   row(u, u + nu, ua);
                   for (void* p : {(void*)u, (void*)ua, (void*)v, (void*)a}) rk_free(p);
               });
}

// ---- as JSON (the schema of dump_hash_json, src/rkmh.cpp:489-525; dead code in the reference, kept here as the interchange format
// SURVEY.md section 8f ranks next).  Keys are emitted in the alphabetical order nlohmann::json uses.  "hashPolicy" is this build's
// addition to them -- what hashType / hashSeed leave open --, and so are the "maxHash" and "scaled" of a scaled sketch.
static void json_escape(std::string& out, const char* s) {
    for (; *s; ++s) {
        unsigned char ch = (unsigned char)*s;
        if (ch == '"' || ch == '\\') { out += '\\'; out += (char)ch; }
        else if (ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); out += b; }
        else out += (char)ch;
    }
}
void write_sketch_json(FILE* fo, const std::vector<std::string>& names, const std::vector<uint64_t>& seq_len, const std::string& kstr,
                       const std::vector<SketchRow>& rows, uint64_t scaled, uint64_t max_hash, uint64_t min_copies) {
    const std::string head = "{\"alphabet\":\"ATGC\",\"canonical\":\"true\",\"hashBits\":64,\"hashPolicy\":\"" + policy_text(g_policy) + "\",\"hashSeed\":" +
                             std::to_string(g_policy.seed) + ",\"hashType\":\"MurmurHash3_x64_128\",\"kmer\":\"" + kstr + "\"" +
                             (scaled ? ",\"maxHash\":" + std::to_string(max_hash) : std::string()) + min_copies_json(min_copies) + ",\"name\":\"";
    const std::string scaled_key = scaled ? "\"scaled\":" + std::to_string(scaled) + "," : std::string();
    OutBuf o(fo);
    o.append("[");
    for (size_t i = 0; i < rows.size(); ++i) {
        std::string name;
        json_escape(name, names[i].c_str());
        if (i) o.append(",");
        o.append(head + name + "\",\"preserveCase\":\"false\"," + scaled_key + "\"seqLen\":" + std::to_string(seq_len[i]) + ",\"sketches\":{");
        if (rows[i].abund) { // (in its alphabetical place)
            o.append("\"abundances\":[");
            for (uint64_t j = 0; j < rows[i].n; ++j) o.appendf(j ? ",%u" : "%u", (unsigned)rows[i].abund[j]);
            o.append("],");
        }
        o.append("\"comment\":\"\",\"hashes\":[");
        for (uint64_t j = 0; j < rows[i].n; ++j) o.appendf(j ? ",%llu" : "%llu", (unsigned long long)rows[i].hashes[j]);
        o.append("],\"length\":" + std::to_string(rows[i].length) + ",\"name\":\"" + name + "\"}}");
        o.end_row();
    }
    o.append("]\n");
    o.flush();
}

void refuse_scaled(const LoadedSketches& L, const char* path, const char* command) {
    if (!L.scaled) return;
    fprintf(stderr, "rkmh: %s holds scaled sketches (scaled = %llu); scaled sketches serve `rkmh dist`, not %s, which needs bottom-s sketches\n", path,
            (unsigned long long)L.scaled, command);
    exit(1);
}

// ---- the inputs of dist and gather
bool parse_scaled(const char* text, uint64_t& scaled) {
    if (!text || !isdigit((unsigned char)*text)) return false;
    char* e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(text, &e, 10);
    if (errno != 0 || *e != 0 || v == 0) return false;
    scaled = (uint64_t)v;
    return true;
}
bool parse_at_least_1(const char* text, int& v) {
    uint64_t u = 0;
    if (!parse_scaled(text, u) || u > 0x7fffffffull) return false;
    v = (int)u;
    return true;
}
bool parse_min_copies(const char* text, uint64_t& m) { return min_copies_from_text(text, m); }
void refuse_min_copies(const char* command, uint64_t m, bool whole_files, bool scaled) {
    const char* why = m == 0 ? "--min-copies takes a number of 1 .. 4294967295"
                    : m == 1 ? nullptr
                    : scaled ? "--min-copies filters bottom-s sketches (-s); scaled sketches keep every copy count with --abund"
                    : !whole_files ? "--min-copies counts the copies of a k-mer over a whole file: it needs -g"
                    : !sample_on_device() ? "--min-copies needs the sample built on the device: not with RKMH_SAMPLE_DEVICE=0"
                    : nullptr;
    if (!why) return;
    fprintf(stderr, "rkmh %s: %s\n", command, why);
    exit(1);
}
bool shared_option(int c, CompareInputs& in) {
    switch (c) {
        case 1004: policy_apply(optarg, "--hash-policy"); return true;
        case 1005: in.scaled_given = true; in.scaled_ok = parse_scaled(optarg, in.scaled); return true;
        case 'r': in.ref_files.push_back(optarg); return true;
        case 'f': in.query_files.push_back(optarg); return true;
        case 'R': in.ref_json.push_back(optarg); return true;
        case 'Q': in.query_json.push_back(optarg); return true;
        case 'k': in.ks.push_back(atoi(optarg)); return true;
        case 's': in.S = atoi(optarg); if (in.S < 1) in.S = -1; return true;
        case 'g': in.whole_files = true; return true;
        case 1000: in.device = atoi(optarg); return true;
        default: return false;
    }
}
void refuse(const CompareRules& rules, const std::string& why) { fprintf(stderr, "rkmh %s: %s\n", rules.command, why.c_str()); exit(1); }
int one_k(const CompareInputs& in, const CompareRules& rules) {
    if (in.ks.size() > 1) {
        std::string given;
        for (int k : in.ks) given += " " + std::to_string(k);
        refuse(rules, std::string(rules.noun) + " needs one k-mer size; sizes provided:" + given);
    }
    return in.ks.empty() ? 0 : in.ks[0];
}
void load_sketch_files(const CompareInputs& in, const CompareRules& rules, LoadedSides& ld) {
    bool any_bottom = false;
    auto load = [&](const std::vector<const char*>& paths, SketchSet& into, std::vector<LoadedSketches>& sc_into, bool need_abund) {
        for (const char* path : paths) {
            const std::string p(path);
            LoadedSketches L;
            if (!load_sketch_json(path, L, RK_MAX_SKETCH)) {
                if (!L.err.empty()) refuse(rules, p + ": " + L.err);
                if (!rules.no_bottom && L.S > RK_MAX_SKETCH) refuse(rules, p + ": sketch size outside 1 .. " + std::to_string(RK_MAX_SKETCH));
                refuse(rules, "cannot load sketches from " + p + " (unreadable, or its sketches disagree in kmer, hashPolicy or length)");
            }
            rk_policy theirs;
            rk_default_policy(&theirs);
            if (rk_policy_parse(L.policy.c_str(), &theirs) != RK_OK) refuse(rules, p + ": " + rk_last_error());
            if (!rk_policy_same_hashes(&theirs, &g_policy))
                refuse(rules, p + " holds sketches hashed with " + policy_text(theirs) + ", this run hashes with " + policy_text(g_policy) + ": pass --hash-policy " + policy_text(theirs));
            if (L.ks.size() != 1) refuse(rules, p + " holds sketches of " + std::to_string(L.ks.size()) + " k-mer sizes; " + rules.noun + " needs one");
            if (ld.k != 0 && L.ks[0] != ld.k) refuse(rules, p + " holds sketches of k = " + std::to_string(L.ks[0]) + ", the others (or -k) say " + std::to_string(ld.k));
            if (!L.scaled && rules.no_bottom) refuse(rules, p + " holds bottom-s sketches; " + rules.no_bottom);
            if (!L.scaled && in.abund) refuse(rules, p + " holds bottom-s sketches, which keep no abundances; --abund needs sketches of `rkmh sketch --scaled <n> --abund`");
            if (!L.scaled) any_bottom = true;
            if ((L.scaled || ld.largest_scaled) && any_bottom) refuse(rules, p + ": scaled and bottom-s sketches cannot be compared with each other");
            ld.k = L.ks[0];
            if (L.scaled) { // (no bottom-s file came before: S is still the -s option)
                if (ld.S != 0) refuse(rules, p + " holds scaled sketches (scaled = " + std::to_string(L.scaled) + "); -s is for bottom-s sketches");
                if (in.scaled_given && L.scaled > in.scaled)
                    refuse(rules, p + " holds sketches of scaled = " + std::to_string(L.scaled) + ": they cannot be made finer, --scaled must be at least that");
                if (need_abund && !L.has_abund) refuse(rules, p + " holds no abundances; --abund needs " + (rules.abund_both_sides ? "" : "query ") + "sketches of `rkmh sketch --scaled <n> --abund`");
                ld.largest_scaled = std::max(ld.largest_scaled, L.scaled);
                sc_into.push_back(std::move(L));
                continue;
            }
            if (in.scaled_given) refuse(rules, p + " holds bottom-s sketches; --scaled compares scaled ones (rkmh sketch --scaled)");
            if (ld.S != 0 && L.S != ld.S) refuse(rules, p + " holds sketches of size " + std::to_string(L.S) + ", the others (or -s) say " + std::to_string(ld.S));
            ld.S = L.S;
            into.names.insert(into.names.end(), L.names.begin(), L.names.end());
            into.sk.insert(into.sk.end(), L.sk.begin(), L.sk.end());
            into.lens.insert(into.lens.end(), L.lens.begin(), L.lens.end());
        }
    };
    ld.S = in.S;
    load(in.ref_json, ld.refs, ld.sc_refs, in.abund && rules.abund_both_sides);
    load(in.query_json, ld.queries, ld.sc_queries, in.abund);
}

static void cut_scaled_files(const std::vector<LoadedSketches>& from, uint64_t max_hash, ScaledSet& into) {
    for (const LoadedSketches& L : from)
        for (size_t i = 0; i < L.names.size(); ++i) {
            const uint64_t* b = L.sk.data() + L.off[i];
            const uint64_t* e = std::upper_bound(b, L.sk.data() + L.off[i + 1], max_hash);
            into.names.push_back(L.names[i]);
            into.values.insert(into.values.end(), b, e);
            if (into.with_abund) into.abund.insert(into.abund.end(), L.abund.begin() + (ptrdiff_t)L.off[i], L.abund.begin() + (ptrdiff_t)(L.off[i] + (uint64_t)(e - b)));
            into.off.push_back(into.values.size());
        }
}
void start_scaled_run(const CompareInputs& in, const CompareRules& rules, const LoadedSides& ld, int k, ScaledRun& run) {
    uint64_t max_hash = 0;
    CK(rk_scaled_max_hash(in.scaled_given ? in.scaled : ld.largest_scaled, &max_hash));
    ScaledSet &sr = run.refs, &sq = run.own_queries;
    sq.with_abund = in.abund;
    sr.with_abund = in.abund && rules.abund_both_sides; // (gather: the references' abundances play no part)
    cut_scaled_files(ld.sc_refs, max_hash, sr);
    cut_scaled_files(ld.sc_queries, max_hash, sq);
    if (in.ref_files.empty() && sr.names.empty()) refuse(rules, "no reference sketches");
    if (!in.self() && in.query_files.empty() && sq.names.empty()) refuse(rules, "no query sketches");
    if (rules.too_many_loaded && (sr.names.size() > 0x7fffffffull || sq.names.size() > 0x7fffffffull)) refuse(rules, rules.too_many_loaded);
    CK(rk_ctx_create(in.device, &g_policy, &run.ctx));
    const std::vector<int> kk(1, k);
    if (!in.ref_files.empty()) sketch_files_scaled(run.ctx, in.ref_files, kk, max_hash, in.whole_files, sr);
    if (!in.query_files.empty()) sketch_files_scaled(run.ctx, in.query_files, kk, max_hash, rules.file_is_one_query || in.whole_files, sq);
    run.queries = in.self() ? &sr : &sq;
    if (sr.names.empty() || run.queries->names.empty()) refuse(rules, std::string("no ") + (sr.names.empty() ? "reference" : "query") + " sketches");
}
