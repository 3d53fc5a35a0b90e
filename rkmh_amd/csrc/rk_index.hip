// rk_index.hip -- the reference side of main_stream (src/rkmh.cpp:783-785, :816-838) behind the C ABI: sketches -> the resident
// lookup index (fingerprint buckets, posting lists of genome families, the k-mer-space filter and maps with their enumeration
// cache), and the per-key masks of the -M depth filter.  The layout of every structure is host-only code in rk_index_plan.hpp;
// build_index here reads the knobs, calls the planning steps, uploads what they return and publishes the result.
#include "rk_api_internal.hpp"
#include "rk_index_plan.hpp"

// ---- the k-mer enumeration cache (rk_set_kmer_cache) ----
// File: "RKKM1\n", u64 tag, u32 entries, then per entry {u32 k, u32 found, found x (u32 k-mer, u32 key id)}.  The tag is a hash of
// everything the lists depend on: every index key in key-id order, the number of keys, fold, seed and the strand rule.  Any other file is ignored
// (and overwritten after the enumeration has run): a cache never changes results, it only skips the work that would reproduce it.
static uint64_t kmer_cache_tag(const rk_ctx* c, const std::vector<uint32_t>& dense, size_t nkeys) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](uint64_t v) { h ^= v; h *= 0x100000001b3ull; h ^= h >> 29; };
    mix(0x726b6b6d31ull); mix((uint64_t)nkeys); mix((uint64_t)(uint32_t)c->pol.fold); mix((uint64_t)c->pol.seed);
    if (c->pol.canon) mix(0x63616e6f6e00ull | (uint64_t)(uint32_t)c->pol.canon); // (canon=minhash: the tag files on disk already carry)
    for (size_t q = 0; q < nkeys; ++q) mix(((uint64_t)dense[q * 4 + 1] << 32) | dense[q * 4]);
    return h;
}
static bool kmer_cache_read(const std::string& path, uint64_t tag, std::map<int, std::vector<uint32_t>>& lists) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[6];
    uint64_t ftag = 0;
    uint32_t n = 0;
    bool ok = fread(magic, 1, 6, f) == 6 && memcmp(magic, "RKKM1\n", 6) == 0 && fread(&ftag, 8, 1, f) == 1 && fread(&n, 4, 1, f) == 1 && ftag == tag && n <= 64;
    for (uint32_t i = 0; ok && i < n; ++i) {
        uint32_t k = 0, found = 0;
        ok = fread(&k, 4, 1, f) == 1 && fread(&found, 4, 1, f) == 1 && k >= 1 && k <= (uint32_t)KW_MAX_K && found <= 0x3fffffffu;
        if (!ok) break;
        std::vector<uint32_t> l((size_t)found * (k > 16 ? 3 : 2)); // (k-mer, key id) -- a wide k-mer takes two words
        ok = l.empty() || fread(l.data(), 4, l.size(), f) == l.size();
        if (ok) lists[(int)k] = std::move(l);
    }
    fclose(f);
    if (!ok) lists.clear();
    return ok;
}
static bool kmer_cache_write(const std::string& path, uint64_t tag, const std::map<int, std::vector<uint32_t>>& lists) {
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return false;
    const uint32_t n = (uint32_t)lists.size();
    bool ok = fwrite("RKKM1\n", 1, 6, f) == 6 && fwrite(&tag, 8, 1, f) == 1 && fwrite(&n, 4, 1, f) == 1;
    for (auto& kv : lists) {
        const uint32_t k = (uint32_t)kv.first;
        const uint32_t found = (uint32_t)(kv.second.size() / (k > 16 ? 3 : 2));
        ok = ok && fwrite(&k, 4, 1, f) == 1 && fwrite(&found, 4, 1, f) == 1 && (kv.second.empty() || fwrite(kv.second.data(), 4, kv.second.size(), f) == kv.second.size());
    }
    ok = (fclose(f) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), path.c_str()) == 0; // (atomic: a concurrent reader sees the old file or the new one)
    if (!ok) remove(tmp.c_str());
    return ok;
}

static int build_key_mask(rk_ctx* c);
// RKMH_INDEX_TIMING=1: where the time of an index build goes (stderr)
struct IndexClock {
    bool on = getenv("RKMH_INDEX_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void tick(const char* what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "[rkmh index] %-28s %.2f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
        t = n;
    }
};

// ---- references --------------------------------------------------------------------------------
// The environment of an index build.  RKMH_KBASES, RKMH_KMER_PREFILTER and RKMH_KF4_ENTRIES are read once per process, the others
// at every build (tests change them between builds of one process).
struct IndexKnobs {
    int nbases;         // RKMH_KBASES: base lists of build_kpost (default KBASE_MAX)
    int pre_mode;       // RKMH_PREFILTER=0 turns the first-level filter off (A/B runs)
    long pre_maxkb;     // RKMH_PRE_MAXKB overrides the filter's cap (tests); 0: the rule
    int kmer_mode;      // RKMH_KMER_PREFILTER=0 turns the k-mer-space structures off (A/B runs, tests); default: as pre_mode
    int enum_maxk;      // RKMH_KMER_ENUM_MAXK: the longest wide k enumerated unasked (default 18)
    double kf4_entries; // RKMH_KF4_ENTRIES: forced density of the group filter (A/B runs); 0: the rule
    bool force_dup;     // RKMH_KMAP_FORCE_DUP (tests): behave as if two k-mers shared a key (nothing is built)
};
static IndexKnobs read_knobs() {
    static const int nbase_env = getenv("RKMH_KBASES") ? atoi(getenv("RKMH_KBASES")) : KBASE_MAX;
    static const int kmer_env = getenv("RKMH_KMER_PREFILTER") ? atoi(getenv("RKMH_KMER_PREFILTER")) : -1;
    static const double kf4_entries = getenv("RKMH_KF4_ENTRIES") ? atof(getenv("RKMH_KF4_ENTRIES")) : 0.0;
    IndexKnobs kn{};
    kn.nbases = nbase_env; kn.kf4_entries = kf4_entries;
    kn.pre_mode = getenv("RKMH_PREFILTER") ? atoi(getenv("RKMH_PREFILTER")) : 1;
    if (const char* e = getenv("RKMH_PRE_MAXKB")) { const long v = atol(e); if (v >= 16 && v <= (1 << 20)) kn.pre_maxkb = v; }
    kn.kmer_mode = kmer_env >= 0 ? kmer_env : (kn.pre_mode > 0 ? 1 : 0);
    kn.enum_maxk = getenv("RKMH_KMER_ENUM_MAXK") ? atoi(getenv("RKMH_KMER_ENUM_MAXK")) : 18;
    kn.force_dup = getenv("RKMH_KMAP_FORCE_DUP") != nullptr;
    return kn;
}

// one resident array: room for it and `slack_bytes` more (what a kernel may request past its end), then the copy
template <typename T>
static int upload(DevBuf& d, const std::vector<T>& v, size_t slack_bytes = 0) {
    RKCHK(d.reserve(v.size() * sizeof(T) + slack_bytes));
    if (!v.empty()) HIPCHK(hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return RK_OK;
}

// k-mer-space structures (every k-mer size of the run from 8 to 16): every k-mer of the 4^k universe whose canonical hash is a key
// (or 0), found by exhaustive enumeration on the device -- see k_enum_kmers -- goes into the group filter and the exact map of
// k_classify_kmer (rk_kmer.hip), one pair per size.  Are they built for this run?
static bool kmer_form_eligible(const rk_ctx* c, const IndexKnobs& kn, size_t distinct, bool wide_k) {
    const size_t kmer_max_keys = 6000000;
    // (dedup=distinct: row field 3 counts a read's distinct hashes, which only k_classify_tile has a form for -- no k-mer-space structures)
    bool all_k_ok = kn.kmer_mode > 0 && c->kmer_form_allowed && !c->dedup && c->ks.n >= 1 && c->ks.n <= KM_MAX_KS && distinct <= kmer_max_keys;
    for (int j = 0; j < c->ks.n; ++j) all_k_ok = all_k_ok && c->ks.k[j] >= KPRE_MIN_K && (c->ks.k[j] <= 16 || wide_k);
    if (wide_k && distinct >= (size_t)KW_EMPTY - 16) all_k_ok = false; // (key numbers of the wide map are 20 bits)
    for (int j = 0; j + 1 < c->ks.n; ++j) for (int i = j + 1; i < c->ks.n; ++i) all_k_ok = all_k_ok && c->ks.k[j] != c->ks.k[i]; // a size given twice hashes twice: hash-space path
    return all_k_ok;
}

// the k-mers of size k whose canonical hash is a key of ix (or 0), from the device.  They come back as a list (one per strand
// pair): normally exactly one per key, plus any k-mer that collides with a key or hashes to 0; found > list_cap: the list is cut
static int enumerate_kmers(rk_ctx* c, const RefIndex& ix, int k, uint32_t list_cap, uint32_t& found, KmerList& list) {
    DevBuf d_list, d_stats;
    struct Release { DevBuf& a; DevBuf& b; ~Release() { a.release(); b.release(); } } release_list{d_list, d_stats}; // freed on every path out
    RKCHK(d_list.reserve((size_t)list_cap * (k > 16 ? 16 : 8)));
    RKCHK(d_stats.reserve(16));
    HIPCHK(hipMemsetAsync(d_stats.p, 0, 16, c->st));
    hipError_t le = launch_enum_kmers(ix, c->pol, k, d_stats.as<uint32_t>(), d_list.as<uint2>(), list_cap, c->st);
    if (le == hipSuccess) le = hipMemcpyAsync(&found, d_stats.p, 4, hipMemcpyDeviceToHost, c->st);
    if (le == hipSuccess) le = hipStreamSynchronize(c->st);
    const size_t got = std::min<uint32_t>(found, list_cap);
    std::vector<uint32_t> raw(got * (k > 16 ? 4 : 2));
    if (le == hipSuccess && !raw.empty()) le = hipMemcpy(raw.data(), d_list.p, raw.size() * 4, hipMemcpyDeviceToHost);
    if (le != hipSuccess) return fail(RK_ERR_HIP, "k-mer enumeration: %s", hipGetErrorString(le));
    list = sort_kmer_list(raw, got, k);
    return RK_OK;
}

// filter, map and value table of k-mer size number kidx onto the device
static int upload_kmer_maps(rk_ctx* c, int kidx, const KmerMaps& m, const std::vector<uint32_t>& vals, bool wide) {
    RKCHK(upload(c->d_km1[(size_t)kidx], m.cells));
    RKCHK(upload(c->d_km1v[(size_t)kidx], vals, 16));
    RKCHK(upload(c->d_kf4[(size_t)kidx], m.f4));
    if (!wide) return upload(c->d_km1cells[(size_t)kidx], m.km1cells, 16);
    RKCHK(upload(c->d_kkeys, m.kkeys));
    return upload(c->d_kslots, m.kslots);
}

// a full bottom-S sketch of uniform hashes keeps the fraction (largest kept hash / 2^64) of the k-mers
static double sketch_density(const rk_ctx* c) {
    double density = 0.0;
    for (int r = 0; r < c->nref; ++r) {
        const int len = c->h_lens[(size_t)r];
        double d = 1.0;
        if (len == c->S && len > 0) d = (double)c->h_sk[(size_t)r * c->S + (size_t)len - 1] / 18446744073709551616.0;
        if (d > density) density = d;
    }
    return density;
}

// The context's sketches (h_sk, h_lens, ks, S, nref: set and checked by rk_set_reference_sketches, the one caller) -> the resident index.  From the first line to
// the publish block the context has no references: a failure on the way leaves it as a fresh context is.
static int build_index(rk_ctx* c) {
    IndexClock clk;
    const IndexKnobs kn = read_knobs();
    const int R = c->nref;
    // ---- reset
    c->have_refs = false;
    c->ix = RefIndex{}; memset(&c->ksets, 0, sizeof c->ksets);
    memset(&c->ksets_m, 0, sizeof c->ksets_m); // a depth filter set earlier refers to the old key ids
    c->kmer_cache_state = 0;
    rk_index_stats_t st{}; // rk_index_stats: filled where each form is chosen, published with have_refs
    RefIndex ix{};
    KmerSets ksets{};
    uint32_t ncells[KM_MAX_KS] = {0}, vmasks[KM_MAX_KS] = {0}, kpre = 0;
    // ---- the hash-space side: bucket table, dense entries, posting lists, first-level filter
    const std::vector<HashPair> pairs = sorted_pairs(c->h_sk.data(), c->h_lens.data(), R, c->S);
    clk.tick("pairs sorted");
    HashTable t;
    const PlanError pe = fill_hash_table(pairs, t, st);
    if (pe.code != RK_OK) return fail(pe.code, "%s", pe.msg);
    clk.tick("bucket table");
    compact_hash_table(t, st);
    RKCHK(upload(c->d_fpb, t.fpb));
    RKCHK(upload(c->d_base, t.base));
    RKCHK(upload(c->d_kv, t.dense));
    RKCHK(upload(c->d_post, t.post, 256)); // the k-mer-space kernel reads a hit's first sixteen postings before it knows the list's length
    ix.fpb = c->d_fpb.as<uint4>(); ix.base = c->d_base.as<uint32_t>(); ix.kv = c->d_kv.as<uint4>(); ix.post = c->d_post.as<uint32_t>();
    ix.bmask = t.nb - 1; ix.bshift = 32 - t.lg; ix.nref = R;
    if (kn.pre_mode > 0) {
        const uint32_t pwords = prefilter_words(t.distinct, kn.pre_maxkb ? (size_t)kn.pre_maxkb * 256 : prefilter_cap_words(t.distinct));
        RKCHK(upload(c->d_pre, plan_prefilter(pairs, pwords)));
        ix.pre = c->d_pre.as<uint32_t>(); ix.pmask = pwords - 1;
    }
    // ---- the k-mer-space side
    // one k of 17 .. 20 (wide k-mers, 64-bit): the 4^k enumeration takes 0.1 s (k = 17), 0.4 s (18), 1.7 s (19), 6.7 s (20) -- done unasked
    // up to RKMH_KMER_ENUM_MAXK (default 18); beyond that only with a cache file (rk_set_kmer_cache): from it, or -- once -- into it
    const bool wide_k = c->ks.n == 1 && c->ks.k[0] > 16 && c->ks.k[0] <= KW_MAX_K;
    bool all_k_ok = kmer_form_eligible(c, kn, t.distinct, wide_k);
    clk.tick("index + prefilter uploaded");
    std::vector<uint32_t> kpost, kbase;
    std::unordered_map<uint32_t, KList> kremap;
    if (all_k_ok) {
        build_kpost(t.post, R, kn.nbases, kpost, kbase, kremap, st);
        if (kpost.size() >= 0x3fffffffull) all_k_ok = false;
        else {
            RKCHK(upload(c->d_kpost, kpost));
            RKCHK(upload(c->d_kbase, kbase));
            ix.kpost = c->d_kpost.as<uint32_t>(); ix.kbase = c->d_kbase.as<uint32_t>();
            for (int b = 0; b < KBASE_MAX; ++b) ix.kbase_n += kbase[2 * (size_t)b + 1] != 0u ? 1u : 0u;
        }
    }
    clk.tick("posting lists (kpost)");
    std::map<int, std::vector<uint32_t>> kcache;
    bool kcache_dirty = false;
    uint64_t kcache_tag = 0;
    if (all_k_ok && !c->kmer_cache_path.empty()) {
        kcache_tag = kmer_cache_tag(c, t.dense, t.nkeys);
        if (kmer_cache_read(c->kmer_cache_path, kcache_tag, kcache)) c->kmer_cache_state = 1;
    }
    if (all_k_ok && wide_k && c->ks.k[0] > kn.enum_maxk && kcache.find(c->ks.k[0]) == kcache.end() && c->kmer_cache_path.empty()) all_k_ok = false; // too long to do for one run
    std::vector<uint8_t> seen(all_k_ok ? t.nkeys + 1 : 0, 0); // across the sizes: a key found by two k-mers of ANY sizes disables the form
    int built = 0;
    for (int kidx = 0; all_k_ok && kidx < c->ks.n; ++kidx) {
        const int k = c->ks.k[kidx];
        // a handful of k-mers beyond one per key at most, so twice the keys is ample room; more than that disables this form
        const uint32_t list_cap = (uint32_t)std::min<size_t>(2 * t.distinct + 4096, 0x3fffffffu);
        KmerList list;
        uint32_t found = 0;
        const auto cached = kcache.find(k);
        const bool from_cache = cached != kcache.end(); // the enumeration of an earlier run with these keys, this k and this hashing policy
        if (from_cache) { list.k = k; list.w = cached->second; found = list.found(); }
        else {
            RKCHK(enumerate_kmers(c, ix, k, list_cap, found, list));
            if (found <= list_cap && !c->kmer_cache_path.empty()) { kcache[k] = list.w; kcache_dirty = true; }
        }
        kpre += found;
        bool ok = found <= list_cap && !kn.force_dup;
        clk.tick(from_cache ? "k-mer lists from the cache" : "k-mer enumeration");
        if (!ok || !one_preimage(list, t.nkeys, seen)) break; // one size without its structures: the hash-space kernels serve the run
        ValueTable vt{R, t, kremap, st, {}, {}};
        KmerMaps m;
        ok = k > 16 ? plan_wide_maps(list, vt, m) : plan_narrow_maps(list, vt, kn.kf4_entries, m);
        if (ok) {
            RKCHK(upload_kmer_maps(c, kidx, m, vt.vals, k > 16));
            ksets.km1[kidx] = c->d_km1[(size_t)kidx].as<uint4>(); ksets.km1_b[kidx] = m.b; ksets.km1_vals[kidx] = c->d_km1v[(size_t)kidx].as<uint32_t>();
            ksets.kf4[kidx] = c->d_kf4[(size_t)kidx].as<uint4>(); ksets.kf4_n[kidx] = m.nsect; ksets.k[kidx] = k;
            if (k > 16) { ix.kkeys = c->d_kkeys.as<uint2>(); ix.kslots = c->d_kslots.as<uint32_t>(); }
            else { ncells[kidx] = found; vmasks[kidx] = m.vmask; }
            st.km1_bits[kidx] = m.b; st.km1_longest_hop[kidx] = m.longest_hop; st.kf4_sectors[kidx] = m.nsect; st.found[kidx] = found;
            ++built;
        }
        if (k > 16) clk.tick("wide filter + map");
        if (!ok) break;
    }
    clk.tick("filter + exact map");
    if (kcache_dirty) c->kmer_cache_state = kmer_cache_write(c->kmer_cache_path, kcache_tag, kcache) ? 2 : 3;
    if (built == c->ks.n && built > 0) { // every size has its filter and map
        ksets.n = built;
        ix.kf4 = ksets.kf4[0]; ix.kf4_n = ksets.kf4_n[0]; ix.km1 = ksets.km1[0]; ix.km1_b = ksets.km1_b[0];
        ix.km1_vals = ksets.km1_vals[0]; ix.kpk = (uint32_t)ksets.k[0];
        st.kmer_form = 1;
    } else {
        memset(&ksets, 0, sizeof ksets);
        memset(&st.kmer_form, 0, sizeof st - offsetof(rk_index_stats_t, kmer_form)); // not built: every k-mer-space counter reads 0
    }
    st.struct_size = (uint32_t)sizeof st;
    // ---- publish
    c->ix = ix; c->ksets = ksets;
    memcpy(c->km1_ncells, ncells, sizeof ncells); memcpy(c->km1_vmask, vmasks, sizeof vmasks);
    c->nkeys = (uint32_t)t.nkeys; c->h_keyhash = std::move(t.keyhash);
    c->kpre_inserted = kpre; c->istats = st; c->density = sketch_density(c);
    ++c->index_gen;
    c->have_refs = true;
    return build_key_mask(c); // a bounded depth filter set earlier follows the new key ids
}

extern "C" int rk_set_reference_sketches(rk_ctx* c, const uint64_t* sketches, const int32_t* lens, int nref,
                                         const int* ks, int nks, int S) {
    // every refusal that needs no device work comes before anything in the context changes: the previous reference set stays as it was
    if (!c || !sketches || !lens || nref < 1) return fail(RK_ERR_ARG, "bad arguments (need >= 1 reference)");
    if (S < 1 || S > RK_MAX_SKETCH) return fail(RK_ERR_LIMIT, "sketch size %d outside [1,%d]", S, RK_MAX_SKETCH);
    KsArr ksa{};
    RKCHK(check_ks(ks, nks, &ksa));
    for (int r = 0; r < nref; ++r)
        if (lens[r] < 0 || lens[r] > S) return fail(RK_ERR_ARG, "sketch length %d of reference %d outside [0,%d]", lens[r], r, S);
    if (nref > 0xFFFFF) return fail(RK_ERR_LIMIT, "more than 2^20-1 references");
    RKCHK(set_dev(c));
    c->have_refs = false; // from the first change until build_index publishes
    c->ks = ksa; c->nref = nref; c->S = S;
    c->h_sk.assign(sketches, sketches + (size_t)nref * S);
    c->h_lens.assign(lens, lens + nref);
    return build_index(c);
}

// bases on the host, or (d_bases != nullptr) already on this context's device
int set_references_impl(rk_ctx* c, const uint8_t* bases, const uint8_t* d_bases, const uint64_t* offsets, int nref,
                               const int* ks, int nks, int S, int max_samples, uint64_t counter_slots) {
    if (!c || !offsets || nref < 1) return fail(RK_ERR_ARG, "bad arguments (need >= 1 reference; rkmh.cpp:848 is undefined for 0)");
    if (S < 1 || S > RK_MAX_SKETCH) return fail(RK_ERR_LIMIT, "sketch size %d outside [1,%d]", S, RK_MAX_SKETCH);
    GeneralCfg cfg;
    RKCHK(check_ks(ks, nks, &cfg.ks));
    cfg.S = S;
    std::vector<uint64_t> sk((size_t)nref * S);
    std::vector<int32_t> lens((size_t)nref);
    GeneralOut go; go.sketches = sk.data(); go.lens = lens.data();
    rk_counter* cnt = nullptr;
    if (max_samples >= 0) {
        // -I path (rkmh.cpp:828-838): pass 1 counts every k-mer occurrence, pass 2 sketches with the range filter
        RKCHK(rk_counter_create(c, counter_slots ? counter_slots : 200000000ull, &cnt));
        GeneralCfg c1 = cfg;
        if (c->ref_count_mode == 1) c1.distinct_counter = cnt; else c1.inc_counter = cnt;
        GeneralOut none;
        int r = general_run(c, bases, d_bases, offsets, nref, c1, none);
        if (r != RK_OK) { rk_counter_destroy(cnt); return r; }
        cfg.filt_counter = cnt; cfg.filter_mode = FILTER_RANGE; cfg.fmin = 0; cfg.fmax = max_samples;
    }
    IndexClock clk;
    int r = general_run(c, bases, d_bases, offsets, nref, cfg, go);
    clk.tick("reference sketches (device)");
    if (cnt) rk_counter_destroy(cnt);
    if (r != RK_OK) return r;
    return rk_set_reference_sketches(c, sk.data(), lens.data(), nref, ks, nks, S);
}
extern "C" int rk_set_references(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int nref,
                                 const int* ks, int nks, int S, int max_samples, uint64_t counter_slots) {
    return set_references_impl(c, bases, nullptr, offsets, nref, ks, nks, S, max_samples, counter_slots);
}

extern "C" int rk_get_reference_sketches(rk_ctx* c, uint64_t* sketches, int32_t* lens) {
    if (!c || !sketches || !lens) return fail(RK_ERR_ARG, "bad arguments");
    if (!c->have_refs) return fail(RK_ERR_STATE, "no references set");
    memcpy(sketches, c->h_sk.data(), c->h_sk.size() * 8);
    memcpy(lens, c->h_lens.data(), c->h_lens.size() * 4);
    return RK_OK;
}
extern "C" int rk_num_references(const rk_ctx* c) { return c ? c->nref : 0; }

extern "C" int rk_set_reference_count_mode(rk_ctx* c, int mode) {
    if (!c || (mode != 0 && mode != 1)) return fail(RK_ERR_ARG, "mode must be 0 or 1");
    c->ref_count_mode = mode;
    return RK_OK;
}

extern "C" int rk_set_kmer_form(rk_ctx* c, int enable) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    c->kmer_form_allowed = enable != 0;
    return RK_OK;
}
extern "C" int rk_set_kmer_cache(rk_ctx* c, const char* path) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    c->kmer_cache_path = path ? path : "";
    return RK_OK;
}
extern "C" int rk_kmer_cache_state(const rk_ctx* c) { return c ? c->kmer_cache_state : 0; }
extern "C" int rk_index_stats(const rk_ctx* c, rk_index_stats_t* out) {
    if (!c || !out) return fail(RK_ERR_ARG, "bad arguments");
    if (!c->have_refs) return fail(RK_ERR_STATE, "no references set");
    if (out->struct_size < sizeof(uint32_t)) return fail(RK_ERR_ARG, "struct_size is not set");
    const uint32_t n = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof c->istats);
    memcpy(out, &c->istats, n);
    out->struct_size = n;
    return RK_OK;
}
extern "C" int rk_kmer_form(const rk_ctx* c, uint32_t* kmers_found) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    if (!c->have_refs) return fail(RK_ERR_STATE, "no references set");
    if (kmers_found) *kmers_found = c->kpre_inserted;
    return c->ksets.n >= 1 ? 1 : 0;
}

// the per-key form of the depth filter (bounded min_num): keep bit per key id, masked copies of the exact k-mer maps
static int build_key_mask(rk_ctx* c) {
    c->ix.keepkey = nullptr;
    memset(&c->ksets_m, 0, sizeof c->ksets_m);
    if (!c->depth || c->min_num_bound < 0 || !c->have_refs) return RK_OK;
    RKCHK(set_dev(c));
    RKCHK(c->d_keepkey.reserve(((size_t)c->nkeys + 31) / 32 * 4 + 16));
    if (c->depth->compact && c->depth->index_gen != c->index_gen)
        return fail(RK_ERR_STATE, "the compact depth map was laid out for another reference set");
    HIPCHK(launch_keep_keys(c->ix, c->nkeys, c->depth->d, c->depth->slots, c->depth->compact ? c->depth->c_keysid.as<uint32_t>() : nullptr,
                            c->min_occ, c->pol, c->d_keepkey.as<uint32_t>(), c->st));
    if (c->ksets.n >= 1) {
        c->ksets_m = c->ksets;
        for (int j = 0; j < c->ksets.n; ++j) {
            if (c->ksets.k[j] > 16) continue; // wide k-mers: the kernel tests the key's keep bit itself (kkeys carries the key id)
            const size_t bytes = (size_t)16 << c->ksets.km1_b[j];
            RKCHK(c->d_km1m[(size_t)j].reserve(bytes));
            HIPCHK(hipMemcpyAsync(c->d_km1m[(size_t)j].p, c->ksets.km1[j], bytes, hipMemcpyDeviceToDevice, c->st));
            HIPCHK(launch_km1_mask(c->d_km1cells[(size_t)j].as<uint2>(), c->km1_ncells[j], c->d_keepkey.as<uint32_t>(),
                                   c->d_km1m[(size_t)j].as<uint32_t>(), c->km1_vmask[j], c->st));
            c->ksets_m.km1[j] = c->d_km1m[(size_t)j].as<uint4>();
        }
    }
    // the hash-space kernels: a copy of the key array with the verdict in each entry's fourth dword
    RKCHK(c->d_kvm.reserve(((size_t)c->nkeys + 1) * 16));
    HIPCHK(launch_kv_mask(c->ix.kv, c->nkeys, c->d_keepkey.as<uint32_t>(), c->d_kvm.as<uint4>(), c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    c->ix.keepkey = c->d_keepkey.as<uint32_t>();
    return RK_OK;
}

extern "C" int rk_set_depth_filter(rk_ctx* c, rk_counter* counter, int min_kmer_occ) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    if (counter && counter->compact && c->min_num_bound != 0)
        return fail(RK_ERR_STATE, "a compact depth map only answers min_num bound 0 (rk_set_min_num_bound(ctx, 0) first)");
    c->depth = nullptr; c->min_occ = min_kmer_occ;
    c->ix.keepkey = nullptr;
    memset(&c->ksets_m, 0, sizeof c->ksets_m);
    if (counter) {
        if (counter->compact && (counter->index_gen != c->index_gen || counter->ctx != c))
            return fail(RK_ERR_STATE, "the compact depth map was laid out for another reference set or context");
        c->depth = counter; // (every failure below leaves the context without a filter)
        struct Undo { rk_ctx* c; bool armed = true; ~Undo() { if (armed) { c->depth = nullptr; c->ix.keepkey = nullptr; } } } undo{c};
        // the fused kernel's masked forms read one KEEP bit per slot instead of the 4-byte count (k_keep_bits): a snapshot of
        // the table as it is NOW -- the -M flow sets the filter after pass 1 (and after the all-reduce in multi-GPU runs)
        RKCHK(set_dev(c));
        // pass 1 (rk_count_batch_device) is asynchronous on the CALLER's stream, an all-reduce may run on yet another one: the
        // snapshot must see the finished table, so the whole device is drained first (once per -M run: not a hot path)
        HIPCHK(hipDeviceSynchronize());
        RKCHK(counter_settle(counter));
        if (c->min_num_bound != 0) { // bound 0: no window is ever looked up by slot (the mask acts through the keys alone)
            RKCHK(c->d_keepbits.reserve(((counter->slots + 31) / 32) * 4 + 16));
            HIPCHK(launch_keep_bits(counter->d, counter->slots, min_kmer_occ, c->pol, c->d_keepbits.as<uint32_t>(), c->st));
            HIPCHK(hipStreamSynchronize(c->st));
        }
        RKCHK(build_key_mask(c));
        undo.armed = false;
    }
    return RK_OK;
}

// How much of min_num (row field 3) the caller needs under a depth filter.  num_mins only ever meets `num_mins <= min_matches`
// (src/rkmh.cpp:938; filter: `read_min_lens <= 0`, :1292), so a caller that compares with n needs min(min_num, n + 1) and no more.
extern "C" int rk_set_min_num_bound(rk_ctx* c, int bound) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    const int nb = bound < 0 ? -1 : bound;
    if (nb == c->min_num_bound) return RK_OK;
    if (c->depth && c->depth->compact && nb != 0) return fail(RK_ERR_STATE, "the depth filter in use is a compact map: it only answers min_num bound 0");
    c->min_num_bound = nb;
    if (c->depth) return rk_set_depth_filter(c, c->depth, c->min_occ); // rebuild the snapshot in the other form
    return RK_OK;
}
extern "C" int rk_min_num_bound(const rk_ctx* c) { return c ? c->min_num_bound : -1; }

