// rk_general.hip -- the general path: hash tiles -> (optional) in-LDS sort / sketch / intersect, for sequences of any length, and the
// entry points that are nothing but one run of it (rk_calc_hashes*, rk_calc_hash, rk_hash_batch, rk_sketch_batch,
// rk_classify_groups_batch).  rk_minhashes* live here too: they sort hashes that are already on the host through the same launch.
#include "rk_api_internal.hpp"

static uint32_t next_pow2(uint32_t x) { uint32_t p = 64; while (p < x) p <<= 1; return p; }

// mask_by_frequency of the general path: by slot of the depth table, or -- compact depth map -- through the keep bits of the index keys
static void apply_depth_cfg(const rk_ctx* c, GeneralCfg& cfg) {
    if (!c->depth) return;
    if (c->depth->compact) { cfg.filter_mode = FILTER_KEYMASK; return; }
    cfg.filt_counter = c->depth; cfg.filter_mode = FILTER_MASK_MIN; cfg.fmin = c->min_occ;
}
GeneralCfg classify_cfg(const rk_ctx* c) {
    GeneralCfg cfg;
    cfg.ks = c->ks; cfg.S = c->S; cfg.classify = true;
    apply_depth_cfg(c, cfg);
    return cfg;
}

namespace {
// One chunk of a batch, as planned on the host: sequences [i0,i1).  Everything is relative to the chunk (sequence ids to i0, segment
// offsets to its first hash); the vectors are reused from chunk to chunk.
struct Chunk {
    int64_t i0 = 0, i1 = 0;
    uint64_t base0 = 0;              // offsets[i0]
    uint64_t nbases = 0, nhashes = 0;
    std::vector<TileDesc> tiles;
    std::vector<uint64_t> seg;       // [n()+1] first hash of every sequence
    std::vector<std::vector<uint32_t>> classes = std::vector<std::vector<uint32_t>>(32); // ids by next_pow2(hashes): class cls sorts 64 << cls values
    std::vector<uint32_t> long_seqs; // ids with more hashes than the in-LDS sorter holds
    std::vector<uint32_t> presel;    // ids whose block radix-selects the bottom S before it sorts (filled by the sort step)
    std::vector<uint32_t> sel_ids;   // dedup=distinct: presel + long_seqs, the sequences a selection runs on, and ...
    std::vector<DedupSeg> dsegs;     // ... the hash-set region of each of them (filled by the sort step)
    int64_t n() const { return i1 - i0; }
};
struct GTick { // RKMH_INDEX_TIMING (stderr: where a general-path batch spends its time)
    const bool on;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[rkmh general] %-24s %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t0).count());
        t0 = now;
    }
};
struct HostFree { void operator()(void* p) const { free(p); } };
} // namespace

static bool needs_sort(const GeneralOut& out) { return out.sketches || out.lens || out.out4 || out.write_back_sorted; }
// tiles of one sequence that starts `rel` bytes into the chunk's bases; its hashes follow those of the sequence before it
static void push_tiles(const rk_ctx* c, const GeneralCfg& cfg, uint64_t rel, uint64_t len, Chunk& ch) {
    uint64_t o = ch.seg.back();
    for (int j = 0; j < (cfg.single_kmer ? 1 : cfg.ks.n); ++j) { // (calc_hash(string): the whole sequence is the one window)
        const uint32_t k = cfg.single_kmer ? (uint32_t)len : (uint32_t)cfg.ks.k[j];
        const uint32_t nw = cfg.single_kmer ? 1u : (uint32_t)num_windows((int)len, (int)k, c->pol.drop_last_window);
        for (uint32_t w0 = 0; w0 < nw; w0 += HASH_TILE_WIN) {
            const uint32_t cnt = std::min<uint32_t>(HASH_TILE_WIN, nw - w0);
            ch.tiles.push_back(TileDesc{rel + w0, o + w0, cnt + k - 1u, cnt, k, 0u});
        }
        o += nw;
    }
    ch.seg.push_back(o);
}

// ---- plan: pick the chunk [ch.i0, i1), describe its tiles, bin its sequences by sort size.  Host code only.
static int plan_chunk(const rk_ctx* c, const uint64_t* offsets, int64_t n, const GeneralCfg& cfg, const GeneralOut& out, Chunk& ch) {
    const uint64_t MAX_CHUNK_BASES = 1ull << 28, MAX_CHUNK_HASHES = 1ull << 26;
    const bool need_sort = needs_sort(out);
    ch.tiles.clear(); ch.seg.assign(1, 0);
    for (auto& v : ch.classes) v.clear();
    ch.long_seqs.clear();
    ch.base0 = offsets[ch.i0]; ch.nbases = ch.nhashes = 0;
    for (ch.i1 = ch.i0; ch.i1 < n; ++ch.i1) {
        const int64_t i = ch.i1;
        const uint64_t len = offsets[i + 1] - offsets[i];
        const uint64_t nh = cfg.single_kmer ? 1 : hashes_of(c->pol, cfg.ks, len);
        if (len > 0x7fffffffull) return fail(RK_ERR_LIMIT, "sequence %lld longer than 2^31-1", (long long)i);
        if (cfg.filter_mode == FILTER_KEYMASK && (nh > (uint64_t)cfg.S || cfg.keep_all))
            return fail(RK_ERR_NEED_FULL, "sequence %lld has %llu hashes for a sketch of %d: bottom-s selection needs the depth of every hash, "
                        "which a compact depth map does not hold", (long long)i, (unsigned long long)nh, cfg.S);
        if (cfg.keep_all && nh > (uint64_t)cfg.S)
            return fail(RK_ERR_LIMIT, "sequence %lld has %llu hashes; without bottom-s selection at most %d take part", (long long)i,
                        (unsigned long long)nh, cfg.S);
        if (i > ch.i0 && (ch.nbases + len > MAX_CHUNK_BASES || ch.nhashes + nh > MAX_CHUNK_HASHES)) break;
        if (need_sort && nh > (uint64_t)SORT_MAX_P && out.write_back_sorted)
            return fail(RK_ERR_LIMIT, "sequence %lld has %llu hashes; in-place sorting handles <= %d",
                        (long long)i, (unsigned long long)nh, SORT_MAX_P);
        if (cfg.single_kmer && (len < 1 || len > RK_MAX_K))
            return fail(RK_ERR_LIMIT, "k-mer length %llu outside [1,%d]", (unsigned long long)len, RK_MAX_K);
        push_tiles(c, cfg, cfg.abs_starts ? cfg.abs_starts[i] : offsets[i] - ch.base0, len, ch);
        if (need_sort) {
            if (nh > (uint64_t)SORT_MAX_P) ch.long_seqs.push_back((uint32_t)(i - ch.i0)); // radix select, then sort <= S candidates
            else {
                int cls = 0; while ((64u << cls) < nh) ++cls; // 64 << cls = next_pow2(nh)
                ch.classes[cls].push_back((uint32_t)(i - ch.i0));
            }
        }
        ch.nbases += len; ch.nhashes += nh;
    }
    return RK_OK;
}

// ---- upload and hash: the chunk's bases (unless resident), tiles and segment offsets go up, every window is hashed into w_hashes
static int upload_and_hash(rk_ctx* c, const uint8_t* bases, const uint8_t* d_bases_in, const GeneralCfg& cfg, const GeneralOut& out,
                           Chunk& ch, uint64_t hash_cursor) {
    const uint8_t* d_bases;
    if (d_bases_in) d_bases = cfg.abs_starts ? d_bases_in : d_bases_in + ch.base0;
    else {
        RKCHK(c->w_bases.reserve(ch.nbases + 64));
        if (ch.nbases) RKCHK(upload_staged(c, c->w_bases.p, bases + ch.base0, ch.nbases, c->st));
        d_bases = c->w_bases.as<uint8_t>();
    }
    if (((uintptr_t)d_bases & 3) != 0) {
        // stage_piece reads aligned dwords; a misaligned base pointer is folded into the tile offsets
        uint64_t mis = (uintptr_t)d_bases & 3;
        d_bases -= mis;
        for (auto& t : ch.tiles) t.base_off += mis;
    }
    RKCHK(c->w_tiles.reserve(ch.tiles.size() * sizeof(TileDesc)));
    RKCHK(c->w_segoff.reserve(ch.seg.size() * 8));
    RKCHK(c->w_hashes.reserve((ch.nhashes + 1) * 8));
    if (!ch.tiles.empty()) HIPCHK(hipMemcpyAsync(c->w_tiles.p, ch.tiles.data(), ch.tiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->w_segoff.p, ch.seg.data(), ch.seg.size() * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_hash_tiles(d_bases, c->w_tiles.as<TileDesc>(), (uint32_t)ch.tiles.size(), c->w_hashes.as<uint64_t>(),
                             cfg.inc_counter ? cfg.inc_counter->d : nullptr, cfg.inc_counter ? cfg.inc_counter->slots : 1,
                             c->pol, c->st));
    if (out.hashes && !out.write_back_sorted && ch.nhashes)
        HIPCHK(hipMemcpyAsync(out.hashes + hash_cursor, c->w_hashes.p, ch.nhashes * 8, hipMemcpyDeviceToHost, c->st));
    return RK_OK;
}

// ---- counter side effects of the chunk's hashes: `call`'s exact depth map, filter's once-per-sequence counts
static int count_hashes(rk_ctx* c, const GeneralCfg& cfg, const Chunk& ch, uint64_t hash_cursor) {
    if (cfg.depth_insert) HIPCHK(launch_depth_insert(c->w_hashes.as<uint64_t>(), ch.nhashes, *cfg.depth_insert, c->st));
    if (cfg.depth_lookup) HIPCHK(launch_depth_lookup(c->w_hashes.as<uint64_t>(), ch.nhashes, *cfg.depth_lookup, cfg.depth_out + hash_cursor, c->st));
    if (!cfg.distinct_counter) return RK_OK;
    for (int64_t q = 0; q < ch.n(); ++q) {
        const uint64_t n_h = ch.seg[(size_t)q + 1] - ch.seg[(size_t)q];
        if (n_h == 0) continue;
        uint64_t tsize = 1024;
        while (tsize < 2 * n_h) tsize <<= 1;
        RKCHK(c->w_table.reserve((tsize + 1) * 8));
        HIPCHK(launch_count_distinct(c->w_hashes.as<uint64_t>() + ch.seg[(size_t)q], n_h, c->w_table.as<uint64_t>(), tsize,
                                     cfg.distinct_counter->d, cfg.distinct_counter->slots, c->st));
    }
    return RK_OK;
}

// The arguments of every launch_sort_intersect on the context's workspaces: `count` sequence ids at d_ids, sorted as P values each.
// The host pointers of `out` only say which results are wanted; gcount / ntail as the sort step laid them out.
static SortArgs sort_args(rk_ctx* c, const GeneralCfg& cfg, const GeneralOut& out, const uint32_t* d_ids, uint32_t count, uint32_t P,
                          int32_t* gcount = nullptr, uint32_t gcount_rows = 0, size_t ntail = 0) {
    SortArgs a{};
    a.hashes = c->w_hashes.as<uint64_t>(); a.seg_off = c->w_segoff.as<uint64_t>();
    a.seq_ids = d_ids; a.nlist = count; a.P = P; a.S = cfg.S;
    a.write_back = out.write_back_sorted ? 1 : 0;
    a.sketches = out.sketches ? c->w_sk.as<uint64_t>() : nullptr;
    a.lens = out.lens ? c->w_lens.as<int32_t>() : nullptr;
    a.out4 = out.out4 ? c->w_out.as<int32_t>() : nullptr;
    a.counter = cfg.filt_counter ? cfg.filt_counter->d : nullptr;
    a.slots = cfg.filt_counter ? cfg.filt_counter->slots : 1;
    a.filter_mode = cfg.filter_mode; a.fmin = cfg.fmin; a.fmax = cfg.fmax;
    if (cfg.classify && out.out4) { a.gcount = gcount; a.gcount_rows = gcount_rows; }
    if (cfg.classify) { a.argmax_n = cfg.argmax_n; a.tail_counts = ntail ? c->w_tail.as<int32_t>() : nullptr; }
    a.dedup = c->dedup ? 1 : 0;
    return a;
}

// dedup=distinct, the exact de-duplication pass in front of a selection: the sequences ids[] (u64 segment offsets at w_segoff, ids
// already at d_ids) keep one copy of every value in w_hashes, the others become 0.  dsegs outlives the upload.  The hash sets live
// in w_table, at most 2^25 slots (or one sequence's set) per launch.
static uint64_t dedup_slots(uint64_t n_h) { uint64_t t = 1024; while (t < 2 * n_h) t <<= 1; return t; }
static int dedup_sequences(rk_ctx* c, const std::vector<uint64_t>& seg, const std::vector<uint32_t>& ids, const uint32_t* d_ids, std::vector<DedupSeg>& dsegs) {
    const uint64_t BATCH_SLOTS = 1ull << 25;
    dsegs.resize(ids.size());
    std::vector<size_t> cut(1, 0); // batches [cut[b], cut[b+1])
    uint64_t used = 0, most = 0;
    for (size_t j = 0; j < ids.size(); ++j) {
        const uint64_t slots = dedup_slots(seg[ids[j] + 1] - seg[ids[j]]);
        if (j > cut.back() && (used + slots > BATCH_SLOTS || j - cut.back() == 65535)) { cut.push_back(j); used = 0; }
        dsegs[j] = DedupSeg{used, slots - 1};
        used += slots;
        most = std::max(most, used);
    }
    cut.push_back(ids.size());
    RKCHK(c->w_table.reserve(most * 8));
    RKCHK(c->w_dedup.reserve(ids.size() * sizeof(DedupSeg)));
    HIPCHK(hipMemcpyAsync(c->w_dedup.p, dsegs.data(), ids.size() * sizeof(DedupSeg), hipMemcpyHostToDevice, c->st));
    for (size_t b = 0; b + 1 < cut.size(); ++b) {
        const size_t j0 = cut[b], j1 = cut[b + 1];
        uint64_t max_n = 0;
        for (size_t j = j0; j < j1; ++j) max_n = std::max(max_n, seg[ids[j] + 1] - seg[ids[j]]);
        HIPCHK(hipMemsetAsync(c->w_table.p, 0, (dsegs[j1 - 1].tab_off + dsegs[j1 - 1].tmask + 1) * 8, c->st));
        HIPCHK(launch_dedup_segments(c->w_hashes.as<uint64_t>(), c->w_segoff.as<uint64_t>(), d_ids + j0, c->w_dedup.as<DedupSeg>() + j0,
                                     (uint32_t)(j1 - j0), max_n, c->w_table.as<uint64_t>(), c->st));
    }
    return RK_OK;
}

static int reserve_select(rk_ctx* c, int S) { // the scratch of select_then_sort
    RKCHK(c->w_sel.reserve((size_t)S * 8 + 64));
    return c->w_selstate.reserve(16 * 4 + 8192 * 4);
}
// One sequence with more hashes than a block selects from: the exact bottom S of its kept hashes by multi-block radix select into
// w_sel, then the launch `a` (one id, P = next_pow2(S)) sorts those instead of the sequence's segment.  The selection has applied
// the filter already and nothing is written back.
static int select_then_sort(rk_ctx* c, const GeneralCfg& cfg, SortArgs a, const uint64_t* d_hashes, uint64_t n_h) {
    uint32_t* st_ = c->w_selstate.as<uint32_t>();
    HIPCHK(launch_select_bottom(d_hashes, n_h, cfg.S, cfg.filt_counter ? cfg.filt_counter->d : nullptr, cfg.filt_counter ? cfg.filt_counter->slots : 1,
                                cfg.filter_mode, cfg.fmin, cfg.fmax, c->pol, st_, st_ + 16, c->w_sel.as<uint64_t>(), c->st));
    a.nlist = 1; a.write_back = 0;
    a.filter_mode = FILTER_NONE; a.counter = nullptr;
    a.sel_hashes = c->w_sel.as<uint64_t>(); a.sel_len = st_ + 8;
    HIPCHK(launch_sort_intersect(a, cfg.classify ? &c->ix : nullptr, c->pol, c->st));
    return RK_OK;
}

// ---- sort / sketch / intersect: every sequence of the chunk through launch_sort_intersect, by one of three routes
static int sort_chunk(rk_ctx* c, const GeneralCfg& cfg, const GeneralOut& out, Chunk& ch, size_t ntail) {
    const uint64_t PRESEL_MAX_HASHES = 1ull << 18; // one block streams its sequence a few times; beyond this the multi-block select is faster (measured: 3 M hashes 4 ms vs 0.7 ms)
    const size_t S = (size_t)cfg.S, cn = (size_t)ch.n();
    if (out.sketches) RKCHK(c->w_sk.reserve(cn * S * 8));
    if (out.lens) RKCHK(c->w_lens.reserve(cn * 4));
    if (out.out4) RKCHK(c->w_out.reserve(cn * 16));
    if (ntail) RKCHK(c->w_tail.reserve(cn * ntail * 4));
    RKCHK(c->w_ids.reserve(cn * 4 * (c->dedup ? 2 : 1)));
    // Sequences with far more hashes than the sketch keeps (long reads, genomes up to a few million k-mers) are not
    // sorted whole: their block radix-selects the bottom S first and sorts only those.
    const uint32_t Psel = next_pow2((uint32_t)S);
    const bool can_presel = !out.write_back_sorted && Psel <= (uint32_t)SORT_MAX_P;
    // panels whose per-reference counter row does not fit the LDS beside the largest sort buffer count in global rows
    int32_t* gcount = nullptr; uint32_t gcount_rows = 0;
    if (cfg.classify && out.out4) {
        // with classification every launch sorts at most next_pow2(S) values (longer sequences are pre-selected)
        gcount_rows = sort_intersect_global_rows(Psel, c->ix.nref);
        if (gcount_rows) {
            RKCHK(c->w_gcount.reserve((size_t)gcount_rows * (size_t)c->ix.nref * 4));
            gcount = c->w_gcount.as<int32_t>();
        }
    }
    uint32_t* d_ids = c->w_ids.as<uint32_t>(); // the next free id slot: every launch reads its ids from its own piece of w_ids
    auto launch = [&](const std::vector<uint32_t>& ids, uint32_t P, uint32_t preselect) -> int {
        HIPCHK(hipMemcpyAsync(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->st));
        SortArgs a = sort_args(c, cfg, out, d_ids, (uint32_t)ids.size(), P, gcount, gcount_rows, ntail);
        a.preselect = preselect; d_ids += ids.size();
        HIPCHK(launch_sort_intersect(a, cfg.classify ? &c->ix : nullptr, c->pol, c->st));
        return RK_OK;
    };
    // 1. by size class: one launch per power of two, each block sorts its whole sequence
    ch.presel.clear();
    for (int cls = 0; cls < 32; ++cls) {
        auto& ids = ch.classes[cls];
        if (ids.empty()) continue;
        if (can_presel && (64u << cls) > Psel) { ch.presel.insert(ch.presel.end(), ids.begin(), ids.end()); continue; }
        RKCHK(launch(ids, 64u << cls, 0));
    }
    // 2. block pre-select: long sequences of moderate size take the same route; only the huge ones need the multi-block select
    if (can_presel) {
        size_t keep = 0;
        for (uint32_t li : ch.long_seqs) {
            if (ch.seg[li + 1] - ch.seg[li] <= PRESEL_MAX_HASHES) ch.presel.push_back(li);
            else ch.long_seqs[keep++] = li;
        }
        ch.long_seqs.resize(keep);
    }
    if (c->dedup && ch.presel.size() + ch.long_seqs.size() > 0) { // (both lists' ids go up once more, behind the launches' own)
        std::vector<uint32_t>& sel_ids = ch.sel_ids;
        sel_ids = ch.presel;
        sel_ids.insert(sel_ids.end(), ch.long_seqs.begin(), ch.long_seqs.end());
        uint32_t* d_sel = c->w_ids.as<uint32_t>() + cn;
        HIPCHK(hipMemcpyAsync(d_sel, sel_ids.data(), sel_ids.size() * 4, hipMemcpyHostToDevice, c->st));
        RKCHK(dedup_sequences(c, ch.seg, sel_ids, d_sel, ch.dsegs));
    }
    if (!ch.presel.empty()) RKCHK(launch(ch.presel, Psel, 1));
    // 3. multi-block select: sequences longer than the LDS sorter, exact bottom-S by radix select first
    if (!ch.long_seqs.empty()) RKCHK(reserve_select(c, cfg.S));
    for (const uint32_t& li : ch.long_seqs) {
        HIPCHK(hipMemcpyAsync(d_ids, &li, 4, hipMemcpyHostToDevice, c->st));
        RKCHK(select_then_sort(c, cfg, sort_args(c, cfg, out, d_ids, 1, Psel, gcount, gcount_rows, ntail),
                               c->w_hashes.as<uint64_t>() + ch.seg[li], ch.seg[li + 1] - ch.seg[li]));
        d_ids += 1;
        HIPCHK(hipStreamSynchronize(c->st)); // w_sel / state are reused by the next long sequence
    }
    return RK_OK;
}

// ---- download: results of the chunk into the caller's arrays at its sequences' places; synchronises
static int download(rk_ctx* c, const GeneralCfg& cfg, const GeneralOut& out, const Chunk& ch, size_t ntail, uint64_t hash_cursor, GTick& tick) {
    if (needs_sort(out)) {
        const size_t i0 = (size_t)ch.i0, cn = (size_t)ch.n(), S = (size_t)cfg.S;
        // the ids vectors must outlive the async copies
        HIPCHK(hipStreamSynchronize(c->st));
        tick("kernels done");
        if (out.write_back_sorted && out.hashes && ch.nhashes)
            HIPCHK(hipMemcpyAsync(out.hashes + hash_cursor, c->w_hashes.p, ch.nhashes * 8, hipMemcpyDeviceToHost, c->st));
        if (out.sketches) HIPCHK(hipMemcpyAsync(out.sketches + i0 * S, c->w_sk.p, cn * S * 8, hipMemcpyDeviceToHost, c->st));
        if (out.lens) HIPCHK(hipMemcpyAsync(out.lens + i0, c->w_lens.p, cn * 4, hipMemcpyDeviceToHost, c->st));
        if (out.out4) HIPCHK(hipMemcpyAsync(out.out4 + i0 * 4, c->w_out.p, cn * 16, hipMemcpyDeviceToHost, c->st));
        if (ntail) HIPCHK(hipMemcpyAsync(out.tail_counts + i0 * ntail, c->w_tail.p, cn * ntail * 4, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(hipStreamSynchronize(c->st));
    tick("results downloaded");
    // -M with a bounded min_num: the general path computes min_num exactly; rows carry min(min_num, bound) on every path
    if (out.out4 && cfg.classify && !cfg.keep_all && (cfg.filter_mode == FILTER_MASK_MIN || cfg.filter_mode == FILTER_KEYMASK) && c->min_num_bound >= 0)
        for (int64_t q = ch.i0; q < ch.i1; ++q) if (out.out4[q * 4 + 3] > c->min_num_bound) out.out4[q * 4 + 3] = c->min_num_bound;
    return RK_OK;
}

int general_run(rk_ctx* c, const uint8_t* bases, const uint8_t* d_bases_in, const uint64_t* offsets, int64_t n,
                const GeneralCfg& cfg, const GeneralOut& out) {
    RKCHK(set_dev(c));
    if (n <= 0) return RK_OK;
    if ((cfg.inc_counter && cfg.inc_counter->compact) || (cfg.distinct_counter && cfg.distinct_counter->compact) || (cfg.filt_counter && cfg.filt_counter->compact))
        return fail(RK_ERR_STATE, "a compact depth map only serves rk_count_batch* of reads that fit the sketch and rk_set_depth_filter");
    if (cfg.classify && !c->have_refs) return fail(RK_ERR_STATE, "classify before rk_set_references");
    static const bool gtiming = getenv("RKMH_INDEX_TIMING") != nullptr; GTick tick{gtiming};
    const size_t ntail = (cfg.classify && cfg.argmax_n > 0 && out.tail_counts) ? (size_t)(c->ix.nref - cfg.argmax_n) : 0; // hpv16: raw counts of the references beside the argmax
    Chunk ch;
    uint64_t hash_cursor = 0; // position in out.hashes
    while (ch.i0 < n) {
        RKCHK(plan_chunk(c, offsets, n, cfg, out, ch));
        tick("chunk planned");
        RKCHK(upload_and_hash(c, bases, d_bases_in, cfg, out, ch, hash_cursor));
        tick("uploaded, hashing launched");
        RKCHK(count_hashes(c, cfg, ch, hash_cursor));
        if (out.scaled) {
            if (gtiming) { HIPCHK(hipStreamSynchronize(c->st)); tick("hashed"); }
            RKCHK(scaled_keep_chunk(c, ch.seg, ch.nhashes, ch.i0, *out.scaled));
            tick("scaled kept");
        }
        if (needs_sort(out)) {
            RKCHK(sort_chunk(c, cfg, out, ch, ntail));
            tick("sorts launched");
        }
        RKCHK(download(c, cfg, out, ch, ntail, hash_cursor, tick));
        hash_cursor += ch.nhashes;
        ch.i0 = ch.i1;
    }
    return RK_OK;
}

static void fill_hash_offsets(const rk_ctx* c, const uint64_t* offsets, int64_t n, const KsArr& ks, uint64_t* ho) {
    ho[0] = 0;
    for (int64_t i = 0; i < n; ++i) ho[i + 1] = ho[i] + hashes_of(c->pol, ks, offsets[i + 1] - offsets[i]);
}

// ------------------------------------------------------------------------------------------------
// inner boundary: the one-sequence mirrors of the mkmh calls
static int calc_hashes_impl(rk_ctx* c, const char* seq, int len, const int* ks, int nks, uint64_t** out, int* n, rk_counter* counter) {
    if (!c || !out || !n || (!seq && len > 0) || len < 0) return fail(RK_ERR_ARG, "bad arguments");
    GeneralCfg cfg;
    RKCHK(check_ks(ks, nks, &cfg.ks));
    cfg.inc_counter = counter;
    uint64_t offs[2] = {0, (uint64_t)len};
    uint64_t ho[2];
    fill_hash_offsets(c, offs, 1, cfg.ks, ho);
    uint64_t* h = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(ho[1] ? ho[1] : 1));
    if (!h) return fail(RK_ERR_NOMEM, "malloc");
    // upper-casing is the caller's job in the reference (to_upper precedes calc_hashes, rkmh.cpp:856-860);
    // the device upper-cases on the fly, which is idempotent for already upper-cased input.
    GeneralOut go; go.hashes = h;
    int r = general_run(c, (const uint8_t*)seq, nullptr, offs, 1, cfg, go);
    if (r != RK_OK) { free(h); return r; }
    *out = h; *n = (int)ho[1];
    return RK_OK;
}
extern "C" int rk_calc_hashes(rk_ctx* c, const char* seq, int len, const int* ks, int nks, uint64_t** out, int* n) {
    return calc_hashes_impl(c, seq, len, ks, nks, out, n, nullptr);
}
extern "C" int rk_calc_hashes_counted(rk_ctx* c, const char* seq, int len, const int* ks, int nks, uint64_t** out, int* n, rk_counter* counter) {
    if (!counter) return fail(RK_ERR_ARG, "counter is NULL");
    return calc_hashes_impl(c, seq, len, ks, nks, out, n, counter);
}
extern "C" int rk_calc_hash(rk_ctx* c, const char* kmer, int k, uint64_t* out) {
    if (!c || !kmer || !out) return fail(RK_ERR_ARG, "bad arguments");
    GeneralCfg cfg; cfg.single_kmer = true; cfg.ks.n = 1; cfg.ks.k[0] = k;
    uint64_t offs[2] = {0, (uint64_t)k};
    GeneralOut go; go.hashes = out;
    return general_run(c, (const uint8_t*)kmer, nullptr, offs, 1, cfg, go);
}

// sort-only pipeline over hashes that are already on the host (minhashes & friends): one segment, one sequence id
static int minhashes_impl(rk_ctx* c, uint64_t* h, int n, int S, uint64_t** mins, int* m, const rk_counter* counter,
                          int filter_mode, int fmin, int fmax, bool sort_input) {
    if (!c || (!h && n > 0) || n < 0 || !mins || !m) return fail(RK_ERR_ARG, "bad arguments");
    if (S < 1 || S > RK_MAX_SKETCH) return fail(RK_ERR_LIMIT, "sketch size %d outside [1,%d]", S, RK_MAX_SKETCH);
    RKCHK(set_dev(c));
    std::unique_ptr<uint64_t, HostFree> r((uint64_t*)malloc(sizeof(uint64_t) * (size_t)S));
    if (!r) return fail(RK_ERR_NOMEM, "malloc");
    // Longer than the in-LDS sorter holds (the reference calls minhashes on every whole reference, rkmh.cpp:822, :835-836):
    // the sketch is the exact bottom S of the kept hashes by radix select (the route rk_set_references takes for long
    // sequences) + a sort of those <= S values; the side effect of mkmh::minhashes -- the caller's array comes back sorted
    // ascending -- is a whole-array device sort (rk_sort.hip).
    const bool long_input = n > SORT_MAX_P;
    size_t tmp_bytes = 0;
    if (long_input && sort_input) HIPCHK(sort_u64_temp_bytes((uint64_t)n, &tmp_bytes));
    RKCHK(c->w_hashes.reserve((size_t)(n + 1) * 8));
    RKCHK(c->w_segoff.reserve(16));
    RKCHK(c->w_ids.reserve(4));
    RKCHK(c->w_sk.reserve((size_t)S * 8));
    RKCHK(c->w_lens.reserve(4));
    if (long_input) RKCHK(reserve_select(c, S));
    if (long_input && sort_input) RKCHK(c->w_misc.reserve(tmp_bytes));
    const uint64_t seg[2] = {0, (uint64_t)n};
    const uint32_t id0 = 0;
    int32_t len = 0;
    if (n) HIPCHK(hipMemcpyAsync(c->w_hashes.p, h, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->w_segoff.p, seg, 16, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->w_ids.p, &id0, 4, hipMemcpyHostToDevice, c->st));
    GeneralCfg cfg;
    cfg.S = S; cfg.filt_counter = counter; cfg.filter_mode = filter_mode; cfg.fmin = fmin; cfg.fmax = fmax;
    GeneralOut out; out.sketches = r.get(); out.lens = &len; out.write_back_sorted = sort_input;
    const SortArgs a = sort_args(c, cfg, out, c->w_ids.as<uint32_t>(), 1, next_pow2((uint32_t)(long_input ? S : n)));
    if (long_input && c->dedup) {
        // dedup=distinct: the caller's array comes back sorted with every copy, as always -- so it is sorted and sent back first;
        // then all but one copy of every value are zeroed and the selection runs on distinct values
        if (sort_input) {
            HIPCHK(launch_sort_u64(c->w_hashes.as<uint64_t>(), (uint64_t)n, c->w_misc.p, tmp_bytes, c->st));
            HIPCHK(hipMemcpyAsync(h, c->w_hashes.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st));
        }
        std::vector<DedupSeg> dsegs;
        RKCHK(dedup_sequences(c, {0, (uint64_t)n}, {0u}, c->w_ids.as<uint32_t>(), dsegs));
        RKCHK(select_then_sort(c, cfg, a, c->w_hashes.as<uint64_t>(), (uint64_t)n));
        HIPCHK(hipStreamSynchronize(c->st)); // dsegs
    } else if (long_input) {
        RKCHK(select_then_sort(c, cfg, a, c->w_hashes.as<uint64_t>(), (uint64_t)n));
        if (sort_input) HIPCHK(launch_sort_u64(c->w_hashes.as<uint64_t>(), (uint64_t)n, c->w_misc.p, tmp_bytes, c->st));
    } else HIPCHK(launch_sort_intersect(a, nullptr, c->pol, c->st));
    if (sort_input && n && !(long_input && c->dedup)) HIPCHK(hipMemcpyAsync(h, c->w_hashes.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(r.get(), c->w_sk.p, (size_t)S * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipMemcpyAsync(&len, c->w_lens.p, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    *m = len;
    *mins = r.release();
    return RK_OK;
}
extern "C" int rk_minhashes(rk_ctx* c, uint64_t* h, int n, int S, uint64_t** mins, int* m) {
    return minhashes_impl(c, h, n, S, mins, m, nullptr, FILTER_NONE, 0, 0, true);
}
extern "C" int rk_minhashes_frequency_filter(rk_ctx* c, uint64_t* h, int n, int S, uint64_t** out, int* m,
                                             const rk_counter* counter, int min_count, int max_count) {
    if (!counter) return fail(RK_ERR_ARG, "counter is NULL");
    return minhashes_impl(c, h, n, S, out, m, counter, FILTER_RANGE, min_count, max_count, true);
}

// ---- batched: hash / sketch --------------------------------------------------------------------
extern "C" int rk_hash_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nseq,
                             const int* ks, int nks, uint64_t** out, uint64_t* hash_offsets) {
    if (!c || !offsets || nseq < 0 || !out || !hash_offsets) return fail(RK_ERR_ARG, "bad arguments");
    GeneralCfg cfg;
    RKCHK(check_ks(ks, nks, &cfg.ks));
    fill_hash_offsets(c, offsets, nseq, cfg.ks, hash_offsets);
    uint64_t total = hash_offsets[nseq];
    uint64_t* h = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)(total ? total : 1));
    if (!h) return fail(RK_ERR_NOMEM, "malloc");
    GeneralOut go; go.hashes = h;
    int r = general_run(c, bases, nullptr, offsets, nseq, cfg, go);
    if (r != RK_OK) { free(h); return r; }
    *out = h;
    return RK_OK;
}

extern "C" int rk_sketch_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nseq,
                               const int* ks, int nks, int S, uint64_t* sketches, int32_t* lens) {
    if (!c || !offsets || nseq < 0 || !sketches || !lens) return fail(RK_ERR_ARG, "bad arguments");
    if (S < 1 || S > RK_MAX_SKETCH) return fail(RK_ERR_LIMIT, "sketch size %d outside [1,%d]", S, RK_MAX_SKETCH);
    GeneralCfg cfg;
    RKCHK(check_ks(ks, nks, &cfg.ks));
    cfg.S = S;
    GeneralOut go; go.sketches = sketches; go.lens = lens;
    return general_run(c, bases, nullptr, offsets, nseq, cfg, go);
}

// hpv16's per-read loop (src/rkmh.cpp:2656-2719): every hash of the read takes part (calc_hashes + mask + sort, no bottom-s);
// argmax over the first argmax_refs references (the HPV types, :2669-2679), raw intersection sizes against the others (the
// lineage- and sublineage-specific k-mer sets that sort_by_similarity ranks, :2688-2704).
extern "C" int rk_classify_groups_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int argmax_refs,
                                        int32_t* out4, int32_t* tail_counts) {
    if (!c || !offsets || nreads < 0 || (nreads > 0 && (!out4 || !bases))) return fail(RK_ERR_ARG, "bad arguments");
    if (!c->have_refs) return fail(RK_ERR_STATE, "classify before rk_set_references");
    if (argmax_refs < 1 || argmax_refs > c->ix.nref) return fail(RK_ERR_ARG, "argmax_refs %d outside [1,%d]", argmax_refs, c->ix.nref);
    if (argmax_refs < c->ix.nref && !tail_counts && nreads > 0) return fail(RK_ERR_ARG, "tail_counts is NULL");
    GeneralCfg cfg = classify_cfg(c);
    cfg.keep_all = true;
    cfg.argmax_n = argmax_refs < c->ix.nref ? argmax_refs : 0;
    GeneralOut go; go.out4 = out4; go.tail_counts = cfg.argmax_n ? tail_counts : nullptr;
    return general_run(c, bases, nullptr, offsets, nreads, cfg, go);
}
