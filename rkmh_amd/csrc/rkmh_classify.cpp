// rkmh_classify.cpp -- stream / classify and filter (src/rkmh.cpp:584-989 and :996-1424): one driver, run_classify, with the stages
// both commands share; main_stream and main_filter parse their options and say what is theirs (Command).
#include "rkmh_cli.hpp"

static void help_stream() {
    fprintf(stderr,
            "rkmh stream|classify -r <refs.fa> -f <reads.fq> [-k <k>]... [-s <sketch>] [options]\n"
            "  -r/--reference <file>   reference FASTA/FASTQ(.gz); repeatable\n"
            "  -f/--fasta <file>       read FASTA/FASTQ(.gz); repeatable\n"
            "  -k/--kmer <k>           k-mer size; repeatable (default 16)\n"
            "  -s/--sketch-size <s>    sketch size (default 1000; at most 16384 in this build)\n"
            "  -t/--threads <n>        accepted for compatibility (the per-read loop runs on the GPU)\n"
            "  -M/--min-kmer-occurence <n>  drop read k-mers seen fewer than n times across all reads\n"
            "  -I/--max-samples <n>    drop reference k-mers counted more than n times across references\n"
            "  -N/--min-matches <n>    flag FAIL:DEPTH / FAIL:MATCHES\n"
            "  -D/--min-diff <n>       flag FAIL:DIFF\n"
            "  -p/-q <file>, -S <n>, -i, -z, -m   parsed and ignored, as in the reference\n"
            "  -F/--pre-reads <file.rkp>  reads packed by `rkmh pack` (2 bits per base + names) instead of -f text; repeatable\n"
            "  -R <sketches.json>      reference sketches written by `rkmh sketch` instead of -r\n"
            "  --depth-map-cache <file>  (with -M) save the read-depth map of this run, or reuse the file if it was saved\n"
            "                          from the same reads, k-mer sizes and hashing policy (anything else is refused)\n"
            "  --kmer-cache <file>       keep the k-mer enumeration of these references (k 8 .. 18; up to 20 once the file exists) in\n"
            "                          <file>; reused while references, k and hashing policy match.  Without it, ONE k of 17 .. 20 keeps\n"
            "                          its enumeration in <first -r file>.k<k>.s<s>.rkkc (--no-kmer-cache: not; k 19 / 20 then hash every window)\n"
            HASH_POLICY_HELP
            "  --device <id>           GPU to use (default 0)\n"
            "  --devices <a,b,..|all>  spread the reads over several GPUs of this node (stream, filter): one host thread and one\n"
            "                          context per device, reference sketches built on the first and imported by the others, -M depth\n"
            "                          tables summed after pass 1; output order and content are those of a single-device run\n");
}
// filter: main_filter, src/rkmh.cpp:996-1424.  Same sketches as stream; the decision is filter_decide (rkmh_frontends.cpp).
static void help_filter() {
    fprintf(stderr,
            "rkmh filter -r <refs.fa> -f <reads.fq> [-k <k>]... [-s <sketch>] [-M n] [-I n] [-N n] [-D n] [-i]\n"
            "  prints the reads (as >name / SEQ / + / QUAL) whose best reference passes the match and diff filters;\n"
            "  -i then classifies reads arriving on STDIN and prints one 'Sample: ... Result: ...' line each\n" HASH_POLICY_HELP);
}

std::vector<int> parse_devices(const char* arg) {
    std::vector<int> d;
    if (!strcmp(arg, "all")) { const int n = rk_device_count(); for (int i = 0; i < n; ++i) d.push_back(i); return d; }
    for (const char* p = arg; *p;) {
        char* e = nullptr;
        const long v = strtol(p, &e, 10);
        if (e == p || v < 0) { fprintf(stderr, "rkmh: bad --devices list '%s'\n", arg); exit(1); }
        d.push_back((int)v);
        p = *e == ',' ? e + 1 : e;
        if (*e && *e != ',') { fprintf(stderr, "rkmh: bad --devices list '%s'\n", arg); exit(1); }
    }
    return d;
}

// The options of stream (src/rkmh.cpp:626-650) and filter (:1963-1983): one table and one switch.  stream adds -z / -m / --output-reads
// / --merge-sketch (parsed and ignored) and --depth-map-cache, and reads -R; filter reads -i.  (The long options keep each command's
// order: getopt lists them in it when an abbreviation is ambiguous.)
static void parse_classify_options(int argc, char** argv, RawKind kind, Opts& o, const char** pre_refs, const char** read_map, bool* in_stream) {
    const bool stream = kind == RAW_STREAM;
    std::vector<struct option> long_options = {
        {"help", no_argument, 0, 'h'},           {"kmer", required_argument, 0, 'k'},
        {"fasta", required_argument, 0, 'f'},    {"reference", required_argument, 0, 'r'},
        {"sketch-size", required_argument, 0, 's'}, {"ref-sketch", required_argument, 0, 'S'},
        {"threads", required_argument, 0, 't'},  {"min-kmer-occurence", required_argument, 0, 'M'},
        {"min-matches", required_argument, 0, 'N'}, {"min-diff", required_argument, 0, 'D'},
        {"max-samples", required_argument, 0, 'I'}, {"pre-reads", required_argument, 0, 'F'},
        {"pre-references", required_argument, 0, 'R'}, {"read-kmer-map-file", required_argument, 0, 'p'},
        {"ref-kmer-map-file", required_argument, 0, 'q'}, {"in-stream", no_argument, 0, 'i'}};
    if (stream)
        long_options.insert(long_options.end(), {
            {"output-reads", no_argument, 0, 'z'},   {"merge-sketch", no_argument, 0, 'm'},
            {"device", required_argument, 0, 1000},  {"depth-map-cache", required_argument, 0, 1001}, {"kmer-cache", required_argument, 0, 1003},
            {"devices", required_argument, 0, 1002}, {"no-kmer-cache", no_argument, 0, 1005}});
    else
        long_options.insert(long_options.end(), {
            {"device", required_argument, 0, 1000}, {"devices", required_argument, 0, 1002}, {"kmer-cache", required_argument, 0, 1003}, {"no-kmer-cache", no_argument, 0, 1005}});
    long_options.insert(long_options.end(), {HASH_POLICY_OPTION, {0, 0, 0, 0}});
    optind = 2;
    int c;
    while ((c = getopt_long(argc, argv, stream ? "zmhdk:f:r:s:S:t:M:N:I:R:F:p:q:iD:" : "hdk:f:r:s:S:t:M:N:I:R:F:p:q:iD:", long_options.data(), nullptr)) != -1) {
        switch (c) {
            case 1004: policy_apply(optarg, "--hash-policy"); break;
            case 'm': case 'z': break;                        // (stream) parsed and ignored, rkmh.cpp:656-658,709-714
            case 'i': if (!stream) *in_stream = true; break; // stream: parsed and ignored; filter: classify reads from STDIN (rkmh.cpp:1329)
            case 'R': if (stream) *pre_refs = optarg; break;  // stream: sketches of `rkmh sketch` (pre-hashed references: parsed but
                                                              // unimplemented in the reference, :662-664); filter: parsed, body empty (:1142-1151)
            // -p/-q (k-mer map files): the reference parses them and does nothing (bodies commented out, :665-670, :744-769);
            // so do we -- no file is read or written.  The reusable depth map is this build's own, explicit option below.
            case 'F': o.packed.push_back(optarg); break;      // --pre-reads: parsed and unused in the reference (:659-664, :1139-1141); here: reads packed by `rkmh pack`
            case 'p': case 'q': case 'S': break; // parsed, bodies empty in the reference (:665-670,:697-700)
            case 1001: *read_map = optarg; break;             // (stream) --depth-map-cache FILE (not a reference flag): see the -M block
            case 1003: o.kmer_cache = optarg; break;          // --kmer-cache FILE (not a reference flag): rk_set_kmer_cache
            case 1005: g_no_kmer_cache = true; break;
            case 't': o.threads = atoi(optarg); break;
            case 'r': o.refs.push_back(optarg); break;
            case 'f': o.reads.push_back(optarg); break;
            case 'k': o.ks.push_back(atoi(optarg)); break;
            case 'N': o.min_matches = atoi(optarg); break;
            case 'D': o.min_diff = atoi(optarg); break;
            case 's': o.sketch = atoi(optarg); break;
            case 'M': o.min_occ = atoi(optarg); o.read_depth = true; break;
            case 'I': o.max_samples = atoi(optarg); o.ref_depth = true; break;
            case 1000: o.device = atoi(optarg); break;
            case 1002: o.devices = parse_devices(optarg); break;
            case '?': case 'h': default: print_help(); exit(1);
        }
    }
}

// What stream and filter do differently; everything else is run_classify's.
struct Command {
    RawKind kind;                   // RAW_STREAM: a TSV line per read; RAW_FILTER: the reads that pass, as FASTQ records
    uint64_t slots;                 // depth-table slots: HASHTCounter(200000000) (rkmh.cpp:739) / read_hash_counter (:1187)
    uint64_t ref_slots;             // slots of the reference-sample counter (rk_set_references: 0 = the library's; filter: 10 M, :1188)
    int max_samples;                // -I as the command applies it (-1: no sample filter)
    int bound;                      // rk_set_min_num_bound with -M (min_num_bound_for; -1: exact)
    const LoadedSketches* sketches; // stream -R: the reference sketches of `rkmh sketch` instead of -r
    const char* read_map;           // stream --depth-map-cache
    bool in_stream;                 // filter -i
};

// Which front end reads which -f file: raw_size[i] >= 0 -- the device front end (stream_files_raw), else the kseq-grammar scanner.
// Regular uncompressed FASTQ files and BGZF / gzip FASTQ go through the device: the host neither parses the reads nor holds them;
// gzip the device does not take, STDIN, FASTA and text that is not four lines per record through the scanner.  RKMH_RAW=0 forces the
// scanner.  stream decides file by file; filter takes all files or none (looking no further than the first that does not qualify);
// -M reads every file twice and takes the device only when ALL of them qualify (two_pass_raw).  Looked at before the engine is made:
// it is laid out for the kinds of read files there are.  Returns whether every file qualifies.
static bool route_reads(const Opts& o, bool file_by_file, std::vector<int64_t>& raw_size) {
    g_read_paths = &o.reads;
    raw_size.assign(o.reads.size(), -1);
    if (!env_flag("RKMH_RAW", true)) return false;
    bool all = !o.reads.empty();
    for (size_t i = 0; i < o.reads.size(); ++i) {
        if (raw_eligible(o.reads[i], &raw_size[i])) continue;
        raw_size[i] = -1;
        all = false;
        if (!file_by_file) break;
    }
    if (!file_by_file && !all) raw_size.assign(o.reads.size(), -1);
    return all;
}

static void front_end_timing(const RawEngine& eng, bool two_passes) {
    if (g_timing)
        fprintf(stderr, "[rkmh timing] device front end: %lld blocks, %lld records; read %.3f s, %s %.3f s, format %.3f s (summed over %zu workers%s)\n",
                (long long)eng.blocks, (long long)eng.records, eng.t_read, two_passes ? "device" : "upload + index + classify", eng.t_dev, eng.t_fmt,
                eng.w.size(), two_passes ? ", both passes" : "");
}

// filter -i (rkmh.cpp:1329-1408): reads from STDIN are classified, one line each
static void classify_stdin(DeviceGroup& group, const rk_seqset& refs, const Opts& o, std::vector<rk_counter*>& cnts, const std::vector<int32_t>& ref_lens) {
    rk_ctx* ctx = group.ctx[0];
    std::string buf;
    std::vector<int32_t> out4;
    // (-i keeps exact rows and full tables -- its lines print min(len) itself -- so the table, if any, is the one the files filled)
    if (cnts.empty()) make_depth_maps(group, 10000000ull, false, cnts);
    rk_counter* cnt = cnts[0];
    CK(rk_set_depth_filter(ctx, o.min_occ > 0 ? cnt : nullptr, o.min_occ)); // :1365
    rk_reader* rd = nullptr;
    CK(rk_reader_open("-", &rd));
    char line[8192];
    for (;;) {
        rk_seqset s;
        CK(rk_reader_next(rd, 1 << 18, 1ull << 27, &s));
        if (s.nseq == 0) { rk_seqset_free(&s); break; }
        out4.resize((size_t)s.nseq * 4);
        CK(rk_classify_batch(ctx, s.bases, s.offsets, s.nseq, out4.data()));
        for (int64_t i = 0; i < s.nseq; ++i) {
            const int32_t* r = &out4[(size_t)i * 4];
            const FilterDecision d = filter_decide(r, o.min_diff);
            const int uni = d.ref < 0 ? 0 : (r[3] < ref_lens[(size_t)d.ref] ? r[3] : ref_lens[(size_t)d.ref]);
            int n = snprintf(line, sizeof line, "Sample: %s\tResult: %s\t%d\t%d\t%s\t%s\t%s\n", s.names + s.name_offsets[i],
                             d.ref < 0 ? "" : refs.names + refs.name_offsets[d.ref], d.shared, uni, r[3] <= 0 ? "FAIL:DEPTH" : "",
                             d.shared < o.min_matches ? "FAIL:MATCHES" : "", d.diff_ok ? "" : "FAIL:DIFF");
            if (n > 0) buf.append(line, (size_t)(n < (int)sizeof line ? n : (int)sizeof line - 1));
        }
        fwrite(buf.data(), 1, buf.size(), stdout);
        buf.clear();
        rk_seqset_free(&s);
    }
    rk_reader_close(rd);
}

[[noreturn]] static void run_classify(const Opts& o, const Command& c) {
    std::vector<int64_t> raw_size;
    const bool all_raw = route_reads(o, c.kind == RAW_STREAM, raw_size);
    bool any_raw = false; // some file of a one-pass run goes through the device front end
    for (int64_t s : raw_size) if (s >= 0 && !o.read_depth) any_raw = true;
    const bool raw_two_pass = o.read_depth && all_raw && !c.read_map;
    // The scanner starts NOW when it has all the files: while the GPU contexts come up and the references are sketched -- a few
    // tenths of a second -- it is already filling its first batches.
    QueueT<Numbered> q;
    q.cap = 4;
    std::thread producer;
    if (!o.read_depth && !any_raw && o.packed.empty()) {
        std::vector<std::pair<const char*, uint64_t>> files;
        for (const char* path : o.reads) files.emplace_back(path, 0);
        producer = start_scanner(q, files, c.kind);
    }

    double t0 = now_s();
    DeviceGroup group;
    group.create(o);
    if (o.read_depth && !c.in_stream) for (rk_ctx* cx : group.ctx) CK(rk_set_min_num_bound(cx, c.bound));
    rk_ctx* ctx = group.ctx[0];
    tick("context", t0);
    // the front end's kernels (and the inflater's) are loaded while the references are sketched, not in front of the first block
    // ... and so are the front end's engine and its first slot made and the BGZF mappings page-locked (unless the references themselves
    // go through the engine: then it is made for them first -- and filter then loads no kernels ahead either)
    RawEngine eng; // the workers and page-locked buffers of the device front ends (created by whoever needs them first)
    std::thread warm;
    if ((any_raw || raw_two_pass) && env_flag("RKMH_WARM_UP", true)) {
        const bool prepare = c.sketches || !refs_for_device(o);
        const bool inflate = any_read_archive() && bgzf_on_device(); // (the table of inputs is complete: the thread only reads it)
        if (prepare || c.kind == RAW_STREAM)
            warm = std::thread([&o, &eng, &group, prepare, inflate] {
                const std::vector<int> ids = o.devices.empty() ? std::vector<int>{o.device} : o.devices;
                for (int id : ids) rk_warm_up(id, inflate);
                if (prepare && eng.create(group)) register_bgzf_mappings();
            });
    }
    // references: sketches from a file (stream -R), through the device, or parsed on the host.  filter: the sample-count filter
    // applies when max_samples < 100000 (rkmh.cpp:1211); its counter is filled once per distinct hash per reference and only when -I
    // was given (rkmh.cpp:1193, :348-355)
    if (c.kind == RAW_FILTER) CK(rk_set_reference_count_mode(ctx, 1));
    rk_seqset refs;
    memset(&refs, 0, sizeof refs);
    DeviceRefs dev_refs;
    bool refs_owned = false;
    std::string pre_names;
    std::vector<uint64_t> pre_noff;
    if (c.sketches) { // names come from the JSON file; emit_lines only needs names + name_offsets
        const LoadedSketches& pre = *c.sketches;
        pre_noff.push_back(0);
        for (auto& nm : pre.names) { pre_names += nm; pre_names += '\0'; pre_noff.push_back(pre_names.size()); }
        refs.nseq = (int64_t)pre.names.size();
        refs.names = &pre_names[0];
        refs.name_offsets = pre_noff.data();
        CK(rk_set_reference_sketches(ctx, pre.sk.data(), pre.lens.data(), (int)pre.lens.size(), o.ks.data(), (int)o.ks.size(), o.sketch));
    } else if (refs_through_device(eng, group, o, c.max_samples, c.ref_slots, refs, dev_refs)) {
        if (c.kind == RAW_FILTER) tick("references: upload + strip + sketch on the device", t0);
    } else {
        CK(rk_parse_files(o.refs.data(), (int)o.refs.size(), &refs));
        if (refs.nseq < 1) { fprintf(stderr, "rkmh: no reference sequences found\n"); exit(1); }
        refs_owned = true;
        if (c.kind == RAW_FILTER) tick("parse references", t0);
        CK(rk_set_references(ctx, refs.bases, refs.offsets, (int)refs.nseq, o.ks.data(), (int)o.ks.size(), o.sketch, c.max_samples, c.ref_slots));
    }
    std::vector<int32_t> ref_lens((size_t)refs.nseq); // (filter -i prints min(len) against them)
    if (c.in_stream) {
        std::vector<uint64_t> sk((size_t)refs.nseq * (size_t)o.sketch);
        CK(rk_get_reference_sketches(ctx, sk.data(), ref_lens.data()));
    }
    group.share_references(o);
    tick(c.kind == RAW_FILTER ? "sketch references" : "references", t0);
    if (warm.joinable()) { warm.join(); tick("kernels loaded (waited)", t0); }
    if (!o.packed.empty()) { // reads written by `rkmh pack`: nothing to parse
        run_packed(group, refs, o, o.packed, c.kind, c.slots, c.bound, t0);
        fflush(stdout);
        tick("main loop + flush", t0);
        done_exit();
    }
    std::vector<rk_counter*> cnts;
    const bool compact_ok = o.read_depth && compact_maps_wanted(c.bound, c.read_map);
    bool depth_done = false;
    if (raw_two_pass && eng.create(group)) {
        // regular FASTQ files: both passes through the device front end, the reads are never held in host memory
        make_depth_maps(group, c.slots, compact_ok, cnts);
        tick("depth tables", t0);
        depth_done = two_pass_raw(eng, group, refs, o, raw_size, cnts, c.kind, t0, c.slots);
        front_end_timing(eng, true);
    }
    if (o.read_depth && !depth_done) {
        // two passes over ALL reads (rkmh.cpp:904-948): the reference holds them in RAM, so do we
        rk_seqset reads;
        CK(rk_parse_files(o.reads.data(), (int)o.reads.size(), &reads));
        tick("parse reads", t0);
        const bool cmp = compact_ok && reads_fit_sketch(reads, o);
        if (cnts.empty() || cmp != (rk_counter_is_compact(cnts[0]) != 0)) make_depth_maps(group, c.slots, cmp, cnts);
        // --depth-map-cache FILE: reuse a saved depth map (pass 1 is skipped) or save this run's for the next one.  The file
        // records what it was counted from (k list, hashing policy, fingerprint of the read set); a file that does not match
        // THIS run is refused with a diagnostic rather than used (CK exits).
        uint8_t tag[RK_DEPTH_TAG_BYTES];
        if (c.read_map) CK(rk_depth_map_tag(ctx, o.ks.data(), (int)o.ks.size(), reads.bases, reads.offsets, reads.nseq, tag));
        FILE* probe = c.read_map ? fopen(c.read_map, "rb") : nullptr;
        const bool cached = probe != nullptr;
        if (probe) fclose(probe);
        std::vector<int32_t> out4((size_t)reads.nseq * 4);
        two_pass(group, cnts, c.slots, o.min_occ,
                 [&] { // count (rkmh.cpp:321-338) -- or the saved table
                     if (cached) CK(rk_counter_load_tagged(cnts[0], c.read_map, tag, sizeof tag));
                     else count_parsed(group, reads, cnts);
                     return true;
                 },
                 [&] { // keep get(h) >= min_kmer_occ (:1260); the summed table is saved before the masked pass
                     if (c.read_map && !cached) CK(rk_counter_save_tagged(cnts[0], c.read_map, tag, sizeof tag));
                     classify_parsed(group, reads, out4.data());
                 }, t0);
        tick("count + classify", t0);
        std::string buf;
        if (c.kind == RAW_FILTER) emit_passing(reads, out4.data(), o, buf);
        else emit_lines(refs, reads, out4.data(), o, buf);
        tick("emit", t0);
        rk_seqset_free(&reads);
    } else if (!o.read_depth && !any_raw) {
        run_scanner_pipeline(group, refs, o, c.kind, q, producer);
    } else if (!o.read_depth) {
        const bool eng_ok = eng.create(group);
        tick("device front end", t0);
        for (size_t i = 0; i < o.reads.size();) {
            int64_t resume = 0;
            if (eng_ok && raw_size[i] >= 0) { // the run of files from here on that the device front end reads, as one pipeline
                size_t j = i;
                while (j < o.reads.size() && raw_size[j] >= 0) ++j;
                const std::vector<const char*> run(o.reads.begin() + (long)i, o.reads.begin() + (long)j);
                const std::vector<int64_t> sizes(raw_size.begin() + (long)i, raw_size.begin() + (long)j);
                size_t ff = 0;
                resume = stream_files_raw(eng, group, refs, o, run, sizes, c.kind, nullptr, &ff);
                if (resume < 0) { i = j; continue; }
                i += ff; // (the files in front of the refused block are done)
                fflush(stdout);
                if (g_timing) fprintf(stderr, "[rkmh timing] %s: not four lines per record at byte %lld: the scanner reads on from there\n", o.reads[i], (long long)resume);
            }
            QueueT<Numbered> q1;
            q1.cap = 4;
            std::thread p1 = start_scanner(q1, {{o.reads[i], (uint64_t)resume}}, c.kind);
            run_scanner_pipeline(group, refs, o, c.kind, q1, p1);
            ++i;
        }
        front_end_timing(eng, false);
    }
    if (c.in_stream) classify_stdin(group, refs, o, cnts, ref_lens);
    fflush(stdout);
    tick("main loop + flush", t0);
    // everything is written and the process ends here: releasing page-locked buffers, streams and contexts one by one took 0.08 s of
    // a 0.55 s run, and freeing a genome-sized reference set, the contexts and the HIP runtime's exit handlers 0.7 s of a 2.5 s C4
    // filter run -- and produce nothing (the operating system takes it all back at once); a profiler's run keeps the orderly way out
    if (getenv("RKMH_SLOW_EXIT")) {
        for (rk_counter* k : cnts) rk_counter_destroy(k);
        eng.destroy();
        if (refs_owned) rk_seqset_free(&refs);
        group.destroy();
        tick("teardown", t0);
    }
    done_exit();
}

int main_stream(int argc, char** argv) {
    Opts o;
    const char* pre_refs = nullptr;
    const char* read_map = nullptr;
    bool in_stream = false;
    if (argc <= 2) { help_stream(); exit(1); }
    parse_classify_options(argc, argv, RAW_STREAM, o, &pre_refs, &read_map, &in_stream);
    LoadedSketches pre;
    if (pre_refs) {
        if (!load_sketch_json(pre_refs, pre)) { fprintf(stderr, "rkmh: cannot load sketches from %s\n", pre_refs); exit(1); }
        refuse_scaled(pre, pre_refs, "-R");
        // sketches hashed under another policy would meet read hashes they can never equal: refused, not classified against
        rk_policy theirs;
        rk_default_policy(&theirs);
        if (rk_policy_parse(pre.policy.c_str(), &theirs) != RK_OK) { fprintf(stderr, "rkmh: %s: %s\n", pre_refs, rk_last_error()); exit(1); }
        if (!rk_policy_same_hashes(&theirs, &g_policy)) {
            fprintf(stderr, "rkmh: %s holds sketches hashed with %s, this run hashes with %s: pass --hash-policy %s\n", pre_refs,
                    policy_text(theirs).c_str(), policy_text(g_policy).c_str(), policy_text(theirs).c_str());
            exit(1);
        }
        o.ks = pre.ks; o.sketch = pre.S;
    }
    if (o.ks.empty()) {
        fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n"); // rkmh.cpp:729
        o.ks.push_back(16);
    }
    if (o.refs.empty() && !pre_refs) { fprintf(stderr, "rkmh: at least one -r reference file (or -R sketches) is required\n"); exit(1); }
    if (!o.packed.empty() && !o.reads.empty()) { fprintf(stderr, "rkmh: give the reads either as text (-f) or as packed files (-F), not both\n"); exit(1); }
    run_classify(o, Command{RAW_STREAM, 200000000ull, 0, o.ref_depth ? o.max_samples : -1, min_num_bound_for(o.min_matches), pre_refs ? &pre : nullptr, read_map, false});
}

int main_filter(int argc, char** argv) {
    Opts o;
    const char* pre_refs = nullptr;
    const char* read_map = nullptr;
    bool in_stream = false;
    if (argc <= 2) { help_filter(); exit(1); }
    parse_classify_options(argc, argv, RAW_FILTER, o, &pre_refs, &read_map, &in_stream);
    if (o.ks.empty()) {
        fprintf(stderr, "No kmer size(s) provided. Will use a default kmer size of 16.\n");
        o.ks.push_back(16);
    }
    if (o.refs.empty()) { fprintf(stderr, "rkmh: at least one -r reference file is required\n"); exit(1); }
    if (!o.packed.empty() && (!o.reads.empty() || in_stream)) { fprintf(stderr, "rkmh: give the reads either as text (-f / -i) or as packed files (-F), not both\n"); exit(1); }
    // file mode compares read_min_lens with 0 (rkmh.cpp:1292); the STDIN lines print min(len) itself (:1397): exact there
    // (with -D >= 0 a read that shares nothing fails the diff test anyway, so not even min(read_min_lens, 1) is needed: bound 0)
    const int bound = (o.read_depth && !in_stream) ? min_num_bound_for(o.min_diff >= 0 ? -1 : 0) : -1;
    run_classify(o, Command{RAW_FILTER, 10000000ull, 10000000ull, o.max_samples < 100000 ? o.max_samples : -1, bound, nullptr, nullptr, in_stream});
}
