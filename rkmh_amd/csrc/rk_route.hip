// rk_route.hip -- the hot loop: which kernel answers a batch of reads (the fused classify / count kernels, the k-mer-space kernel, the
// general path for what they hand back) and the double-buffered host pipeline around them.
#include "rk_api_internal.hpp"

// The -M count pass in its slot-partitioned form (rk_count.hip): worth its fixed cost (six launches, two passes over a slot
// array) for batches of millions of windows into tables that do not fit a few workgroups' LDS; RKMH_COUNT_BINS=1 / 0 forces it
// on (any size: the tests) / off (one device atomic per window, 2.6e10/s)
static int count_bins_env() {
    const char* e = getenv("RKMH_COUNT_BINS"); // read per pass (a few launches each): tests switch it inside one process
    return e && *e ? atoi(e) : -1;
}
// tl: the count pass into k as the atomic form launches it
static int count_partitioned(TileLaunch tl, rk_counter* k, uint64_t total_bases, bool* done) {
    *done = false;
    const hipStream_t st = tl.batch.st;
    const int env = count_bins_env();
    if (env == 0 || total_bases == 0 || !classify_tile_supported(0, tl.batch.maxlen)) return RK_OK;
    const uint64_t stride = (total_bases + 3) & ~3ull;
    CountPlan pl;
    if (stride >= (1ull << 31) || !count_plan(k->slots, stride * (uint64_t)tl.ks->n, &pl)) return RK_OK;
    if (env < 0 && (pl.n < ((uint64_t)4 << 20) || pl.nsub < 256)) return RK_OK;
    std::lock_guard<std::mutex> lock(k->mu);
    if (!k->last) HIPCHK(hipEventCreateWithFlags(&k->last, hipEventDisableTiming));
    if (k->last_set) HIPCHK(hipStreamWaitEvent(st, k->last, 0)); // the previous pass into this table: scratch and sub-ranges are its
    if (k->last_atomic_set) HIPCHK(hipStreamWaitEvent(st, k->last_atomic, 0)); // atomics still landing would race with the plain adds
    const size_t need = count_plan_scratch_bytes(pl);
    if (need > k->ws.cap) { HIPCHK(hipDeviceSynchronize()); RKCHK(k->ws.reserve(need)); } // nothing may still be reading the old arrays
    const CountScratch sc = count_plan_carve(pl, k->ws.p);
    HIPCHK(launch_count_prepare(pl, sc, st));
    tl.out4 = (int32_t*)sc.flat; // the kernel writes every window's slot here instead of counting it
    tl.slot_stride = (uint32_t)stride;
    HIPCHK(launch_classify_tile(tl));
    HIPCHK(launch_count_bins(pl, sc, k->d, st));
    HIPCHK(hipEventRecord(k->last, st));
    k->last_set = true;
    *done = true;
    return RK_OK;
}

int fused_device(rk_ctx* c, const void* d_bases, const void* d_offs, int64_t nreads, void* d_out4,
                 uint32_t max_read_len, int mode, rk_counter* count_into, hipStream_t st, uint64_t total_bases) {
    if (nreads > 0xfffffff0ll) return fail(RK_ERR_LIMIT, "more than 2^32-16 reads in one device batch");
    if (((uintptr_t)d_bases & 3) != 0) return fail(RK_ERR_ARG, "d_bases must be 4-byte aligned");
    int32_t* counter = nullptr; uint64_t slots = 1; int min_occ = 0;
    // the mask acts per key: no slot bitmap in the kernels.  (dedup=distinct with a bound above 0 takes the exact per-window form: the
    // probe that counts a read's first `bound` surviving windows would count repeated values)
    const bool bounded = mode != 1 && c->depth && c->min_num_bound >= 0 && !(c->dedup && c->min_num_bound > 0);
    if (bounded && !c->ix.keepkey) return fail(RK_ERR_STATE, "depth filter: the per-key mask was not built");
    if (mode == 1) { counter = count_into->d; slots = count_into->slots; }
    else if (c->depth && !bounded) { counter = c->d_keepbits.as<int32_t>(); slots = c->depth->slots; min_occ = c->min_occ; } // the keep bitmap, see rk_set_depth_filter
    uint32_t ml = max_read_len < 1 ? 1 : (max_read_len > (uint32_t)FUSED_MAXLEN ? (uint32_t)FUSED_MAXLEN : max_read_len);
    int expect = 0; // hits an error-free read is expected to score: sizes the kernel's per-read hit multiset
    for (int j = 0; j < c->ks.n; ++j) expect += (int)(c->density * (double)num_windows((int)ml, c->ks.k[j], c->pol.drop_last_window)) + 1;
    TileLaunch tl; // what every pass through k_classify_tile has in common
    ReadBatch& rb = tl.batch;
    rb.bases = (const uint8_t*)d_bases;
    rb.offs = (const uint32_t*)d_offs;
    rb.nreads = (uint32_t)nreads;
    rb.maxlen = (int)ml;
    rb.expect_hits = expect;
    rb.st = st;
    RefIndex ix0 = c->ix; ix0.keepkey = nullptr;
    tl.pass = mode == 1 ? TILE_COUNT : (counter ? TILE_CLASSIFY_MASKED : TILE_CLASSIFY);
    tl.ks = &c->ks;
    tl.S = c->S;
    tl.ix = &ix0;
    tl.pol = &c->pol;
    tl.counter = counter;
    tl.slots = slots;
    tl.min_occ = min_occ;
    if (mode == 1 && count_into->compact) {
        // pass 1 into a compact depth map: hash every window, count the few whose slot is tracked (k_classify_tile, MODE 1, cs.tab)
        if (count_into->index_gen != c->index_gen || count_into->ctx != c)
            return fail(RK_ERR_STATE, "the compact depth map was laid out for another reference set or context");
        const uint64_t nh = hashes_of(c->pol, c->ks, max_read_len);
        if (nh > (uint64_t)c->S || max_read_len > (uint32_t)FUSED_MAXLEN || !classify_tile_supported(0, (int)ml))
            return fail(RK_ERR_NEED_FULL, "reads of up to %u bases have more hashes (%llu) than the sketch keeps (%d): bottom-s selection needs the "
                        "depth of every hash, which a compact depth map does not hold", max_read_len, (unsigned long long)nh, c->S);
        tl.compact = &count_into->cs;
        HIPCHK(launch_classify_tile(tl));
        std::lock_guard<std::mutex> lock(count_into->mu);
        if (!count_into->last_atomic) HIPCHK(hipEventCreateWithFlags(&count_into->last_atomic, hipEventDisableTiming));
        HIPCHK(hipEventRecord(count_into->last_atomic, st)); // readers of the map wait for the latest pass (they all add with atomics: no order among them)
        count_into->last_atomic_set = true;
        return RK_OK;
    }
    if (mode == 1) {
        bool done = false;
        RKCHK(count_partitioned(tl, count_into, total_bases, &done));
        if (done) return RK_OK;
        // atomic form: other passes into this table may still be adding with plain stores
        std::lock_guard<std::mutex> lock(count_into->mu);
        if (count_into->last_set) HIPCHK(hipStreamWaitEvent(st, count_into->last, 0));
        // atomic passes are CHAINED too (each waits for the one before): last_atomic is a single event re-recorded by every pass, so
        // it only covers all of them if every pass already contains its predecessors -- otherwise a slot-partitioned pass that follows
        // two atomic passes on different streams would wait for the second one only and its plain adds could lose the first one's counts
        if (count_into->last_atomic_set) HIPCHK(hipStreamWaitEvent(st, count_into->last_atomic, 0));
        if (!classify_tile_supported(0, (int)ml)) return fail(RK_ERR_LIMIT, "count pass: batch not supported by the fused kernel");
        HIPCHK(launch_classify_tile(tl)); // (out4 stays null: given an array there, the pass would write slots to it)
        // a later pass of either form must not overlap this one
        if (!count_into->last_atomic) HIPCHK(hipEventCreateWithFlags(&count_into->last_atomic, hipEventDisableTiming));
        HIPCHK(hipEventRecord(count_into->last_atomic, st));
        count_into->last_atomic_set = true;
        return RK_OK;
    }
    RefIndex ix = c->ix;
    if (!bounded) ix.keepkey = nullptr;
    else {
        if (c->ksets_m.n >= 1) ix.km1 = c->ksets_m.km1[0]; // (the compile-time-k kernels read the first size's structures from ix)
        ix.kv = c->d_kvm.as<uint4>();                       // (hash-space kernels: the key array with the mask's verdict in it)
    }
    if (c->depth && c->min_num_bound >= 0) rb.nmin_cap = c->min_num_bound;
    // classification with k-mer sizes the exact k-mer maps were enumerated for: the k-mer-space kernel (rk_kmer.hip); under a
    // bounded depth filter it reads the masked copies of the maps (a dropped key is a zero-hash k-mer there)
    if (!counter && c->ksets.n == c->ks.n && c->ksets.n >= 1 && (!bounded || c->ksets_m.n == c->ksets.n) &&
        classify_kmer_supported(c->ix.nref, (int)ml, c->ks.k[0]))
        HIPCHK(launch_classify_kmer(rb, bounded ? c->ksets_m : c->ksets, c->S, ix, (int32_t*)d_out4, c->pol));
    else if (classify_tile_supported(c->ix.nref, (int)ml)) {
        tl.ix = &ix;
        tl.out4 = (int32_t*)d_out4;
        tl.dedup = c->dedup;
        HIPCHK(launch_classify_tile(tl));
    } else
        HIPCHK(launch_fill_reroute((int32_t*)d_out4, (uint32_t)nreads, st)); // e.g. more than 16384 references: general path
    // bound > 0: the first `bound` surviving windows of every answered read are counted by hashing them (k_min_num_probe)
    if (bounded && c->min_num_bound > 0)
        HIPCHK(launch_min_num_probe((const uint8_t*)d_bases, (const uint32_t*)d_offs, (uint32_t)nreads, c->ks, c->S, c->min_num_bound,
                                    c->d_keepbits.as<uint32_t>(), c->depth->slots, c->pol, (int32_t*)d_out4, st));
    return RK_OK;
}

static int device_max_len(rk_ctx* c, const void* d_offs, int64_t nreads, hipStream_t st, uint32_t* out, uint32_t* end_off = nullptr) {
    RKCHK(c->w_misc.reserve(16));
    HIPCHK(launch_max_len((const uint32_t*)d_offs, (uint32_t)nreads, c->w_misc.as<uint32_t>(), st));
    HIPCHK(hipMemcpyAsync(out, c->w_misc.p, 4, hipMemcpyDeviceToHost, st));
    if (end_off) HIPCHK(hipMemcpyAsync(end_off, (const uint32_t*)d_offs + nreads, 4, hipMemcpyDeviceToHost, st)); // one past the last base
    HIPCHK(hipStreamSynchronize(st));
    return RK_OK;
}

// the reads idx[] of a host batch gathered into a contiguous sub-batch (offsets from 0), with room for their rows
struct SubBatch { std::vector<uint64_t> offs; std::vector<uint8_t> bases; std::vector<int32_t> rows; };
static SubBatch gather_reads(const uint8_t* bases, const uint64_t* offsets, const std::vector<int64_t>& idx) {
    SubBatch sb{std::vector<uint64_t>(idx.size() + 1, 0), {}, std::vector<int32_t>(idx.size() * 4)};
    for (size_t j = 0; j < idx.size(); ++j) sb.offs[j + 1] = sb.offs[j] + (offsets[idx[j] + 1] - offsets[idx[j]]);
    sb.bases.resize((size_t)sb.offs.back() + 64);
    for (size_t j = 0; j < idx.size(); ++j) memcpy(sb.bases.data() + sb.offs[j], bases + offsets[idx[j]], (size_t)(sb.offs[j + 1] - sb.offs[j]));
    return sb;
}
static void scatter_rows(const SubBatch& sb, const std::vector<int64_t>& idx, int32_t* out4) {
    for (size_t j = 0; j < idx.size(); ++j) memcpy(out4 + idx[j] * 4, sb.rows.data() + j * 4, 16);
}

// reroute reads the fused kernel flagged (max_id == -2) through the general path; offsets = u64 host offsets
static int reroute_flagged(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int32_t* out4) {
    std::vector<int64_t> idx;
    for (int64_t i = 0; i < nreads; ++i) if (out4[i * 4] == -2) idx.push_back(i);
    if (idx.empty()) return RK_OK;
    SubBatch sb = gather_reads(bases, offsets, idx);
    GeneralOut go; go.out4 = sb.rows.data();
    RKCHK(general_run(c, sb.bases.data(), nullptr, sb.offs.data(), (int64_t)idx.size(), classify_cfg(c), go));
    scatter_rows(sb, idx, out4);
    return RK_OK;
}

extern "C" int rk_classify_batch_device(rk_ctx* c, const void* d_bases, const void* d_offs, int64_t nreads,
                                        void* d_out4, uint32_t max_read_len, void* hip_stream) {
    if (!c || nreads < 0 || (nreads > 0 && (!d_bases || !d_offs || !d_out4))) return fail(RK_ERR_ARG, "bad arguments");
    if (!c->have_refs) return fail(RK_ERR_STATE, "classify before rk_set_references");
    RKCHK(set_dev(c));
    if (nreads == 0) return RK_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    // the resident-input entry point serves reads the fused kernel can take (len <= FUSED_MAXLEN and all
    // hashes inside the sketch); anything else is flagged -2 in d_out4 for the caller (rk_classify_batch
    // reroutes those through the general path itself).
    if (max_read_len == 0) RKCHK(device_max_len(c, d_offs, nreads, st, &max_read_len));
    return fused_device(c, d_bases, d_offs, nreads, d_out4, max_read_len, 0, nullptr, st);
}

// Rows the fused kernel handed back (max_id == -2 in `rows`, the host copy of d_out4: long reads, reads with more windows than the
// sketch keeps, ...) answered by the general kernels on the RESIDENT bases -- only the 4-byte offsets and the flagged rows cross
// the link -- and written into rows and d_out4.  Synchronises st.
int reroute_flagged_device(rk_ctx* c, const void* d_bases, const void* d_offs, int64_t nreads, void* d_out4, int32_t* rows, hipStream_t st) {
    std::vector<uint32_t> idx;
    for (int64_t i = 0; i < nreads; ++i) if (rows[(size_t)i * 4] == -2) idx.push_back((uint32_t)i);
    if (idx.empty()) return RK_OK;
    std::vector<uint32_t> offs32((size_t)nreads + 1);
    HIPCHK(hipMemcpyAsync(offs32.data(), d_offs, ((size_t)nreads + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t m = idx.size();
    std::vector<uint64_t> lens_ps(m + 1, 0), starts(m);
    for (size_t j = 0; j < m; ++j) {
        starts[j] = offs32[idx[j]];
        lens_ps[j + 1] = lens_ps[j] + (uint64_t)(offs32[(size_t)idx[j] + 1] - offs32[idx[j]]);
    }
    std::vector<int32_t> res(m * 4);
    GeneralCfg cfg = classify_cfg(c);
    cfg.abs_starts = starts.data();
    GeneralOut go; go.out4 = res.data();
    std::lock_guard<std::mutex> lock(c->general_mu); // (the general path works in the context's own buffers)
    RKCHK(general_run(c, nullptr, (const uint8_t*)d_bases, lens_ps.data(), (int64_t)m, cfg, go));
    for (size_t j = 0; j < m; ++j) memcpy(rows + (size_t)idx[j] * 4, res.data() + j * 4, 16);
    // scatter the answers into the device rows too
    RKCHK(c->w_ids.reserve(m * 4));
    RKCHK(c->w_out.reserve(m * 16));
    HIPCHK(hipMemcpyAsync(c->w_ids.p, idx.data(), m * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->w_out.p, res.data(), m * 16, hipMemcpyHostToDevice, st));
    HIPCHK(launch_scatter_rows(c->w_out.as<int32_t>(), c->w_ids.as<uint32_t>(), (uint32_t)m, (int32_t*)d_out4, st));
    HIPCHK(hipStreamSynchronize(st));
    return RK_OK;
}

// Same contract as rk_classify_batch_device, but no row is left flagged: rows the fused kernel hands back (long reads,
// reads with more windows than the sketch keeps, ...) are answered by the general kernels on the resident bases -- only
// the 4-byte offsets and the flagged rows cross PCIe.  Synchronises `hip_stream` (it has to look at the flags).
extern "C" int rk_classify_batch_device_all(rk_ctx* c, const void* d_bases, const void* d_offs, int64_t nreads,
                                            void* d_out4, uint32_t max_read_len, void* hip_stream) {
    RKCHK(rk_classify_batch_device(c, d_bases, d_offs, nreads, d_out4, max_read_len, hip_stream));
    if (nreads == 0) return RK_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int32_t> rows((size_t)nreads * 4);
    HIPCHK(hipMemcpyAsync(rows.data(), d_out4, (size_t)nreads * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return reroute_flagged_device(c, d_bases, d_offs, nreads, d_out4, rows.data(), st);
}

extern "C" int rk_count_batch_device(rk_ctx* c, const void* d_bases, const void* d_offs, int64_t nreads,
                                     rk_counter* counter, void* hip_stream) {
    if (!c || !counter || nreads < 0 || (nreads > 0 && (!d_bases || !d_offs))) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    if (nreads == 0) return RK_OK;
    hipStream_t st = (hipStream_t)hip_stream;
    uint32_t ml = 0, end_off = 0;
    RKCHK(device_max_len(c, d_offs, nreads, st, &ml, &end_off));
    if (ml > (uint32_t)FUSED_MAXLEN) return fail(RK_ERR_LIMIT, "rk_count_batch_device: reads longer than %d need rk_count_batch", FUSED_MAXLEN);
    if (c->ks.n == 0) return fail(RK_ERR_STATE, "k-mer sizes unknown: call rk_set_references first");
    return fused_device(c, d_bases, d_offs, nreads, nullptr, ml, 1, counter, st, end_off);
}

// double-buffered host pipeline around the fused kernel. mode 0 classify, mode 1 count.
// Page-locked inputs (rk_host_alloc / hipHostMalloc: what the FASTQ front end fills) are read by the DMA engine where they lie;
// pageable ones go through the context's pinned staging buffers, copied by host_threads() threads while the previous chunk is on
// the link.  Results land directly in out4 when that is page-locked.  *flagged receives the number of rows the kernel handed back.
static int host_pipeline(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int32_t* out4,
                         int mode, rk_counter* count_into, int64_t* flagged = nullptr) {
    RKCHK(set_dev(c));
    // reads per chunk: the last chunk's kernel and D2H are not overlapped with anything, and a chunk's H2D cannot start before the
    // chunk two places earlier has left its slot, so shorter chunks finish sooner.  Measured (150 bp reads from page-locked buffers;
    // chunks of 2 M / 512 k / 128 k reads): 4 M reads 278 / 292 / 252 M reads/s, 16 M reads 300 / 313 M reads/s.  (Fixed: the override this was measured with is gone.)
    // (The count pass keeps chunks of 2 M reads: its slot-partitioned form streams the whole table once per launch, rk_count.hip.)
    const int64_t MAX_READS = mode == 1 ? (int64_t)1 << 21 : (int64_t)1 << 19;
    const uint64_t MAX_BASES = 1ull << 29;
    bool src_pinned = nreads > 0 && caller_pinned_host(bases + offsets[0], (size_t)(offsets[nreads] - offsets[0]) + 4);
    bool out_pinned = mode == 0 && nreads > 0 && caller_pinned_host(out4, (size_t)nreads * 16);
    // pageable buffers of some size are page-locked for this call instead of being copied through the staging buffers
    ScopedHostRegister reg_src(nreads > 0 && !src_pinned ? bases + offsets[0] : nullptr, nreads > 0 ? (size_t)(offsets[nreads] - offsets[0]) + 4 : 0, (size_t)8 << 20);
    ScopedHostRegister reg_out(mode == 0 && nreads > 0 && !out_pinned ? out4 : nullptr, (size_t)nreads * 16, (size_t)4 << 20);
    src_pinned = src_pinned || reg_src.ok;
    out_pinned = out_pinned || reg_out.ok;
    int64_t i0 = 0, nflag = 0;
    int which = 0;
    auto drain = [&](Slot& s) -> int {
        if (!s.busy) return RK_OK;
        HIPCHK(hipEventSynchronize(s.done));
        if (mode == 0) {
            int32_t* dst = out4 + s.first * 4;
            const int32_t* src = out_pinned ? dst : s.h_out.as<int32_t>();
            std::vector<int64_t> part((size_t)host_threads() + 1, 0);
            std::atomic<int> slot_no{0};
            par_for((size_t)s.n, (size_t)1 << 17, [&](size_t lo, size_t hi) { // copy out (unless the DMA wrote in place) and count the rows handed back
                if (!out_pinned) memcpy(dst + lo * 4, src + lo * 4, (hi - lo) * 16);
                int64_t k = 0;
                for (size_t i = lo; i < hi; ++i) k += src[i * 4] == -2;
                part[(size_t)slot_no.fetch_add(1) % part.size()] += k;
            });
            for (int64_t k : part) nflag += k;
        }
        s.busy = false;
        return RK_OK;
    };
    while (i0 < nreads) {
        // a chunk: at most MAX_READS reads / MAX_BASES bases (offsets are monotone: the end is found by bisection, the longest read
        // by a parallel scan)
        int64_t i1 = std::min(nreads, i0 + MAX_READS);
        const uint64_t b0 = offsets[i0];
        if (offsets[i1] - b0 > MAX_BASES) {
            int64_t lo = i0 + 1, hi = i1;
            while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (offsets[mid] - b0 <= MAX_BASES) lo = mid; else hi = mid - 1; }
            i1 = lo;
        }
        const int64_t cn = i1 - i0;
        const uint64_t cb = offsets[i1] - b0;
        if (cb > 0xfffffff0ull) return fail(RK_ERR_LIMIT, "read %lld too long for a 32-bit batch", (long long)i0);
        Slot& s = c->slot[which];
        RKCHK(drain(s));
        RKCHK(s.h_offs.reserve((size_t)(cn + 1) * 4));
        if (!src_pinned) RKCHK(s.h_bases.reserve(cb + 64));
        if (!out_pinned && mode == 0) RKCHK(s.h_out.reserve((size_t)cn * 16));
        RKCHK(s.d_bases.reserve(cb + 64)); RKCHK(s.d_offs.reserve((size_t)(cn + 1) * 4)); RKCHK(s.d_out.reserve((size_t)cn * 16));
        uint32_t* ho = s.h_offs.as<uint32_t>();
        std::atomic<uint32_t> maxlen_a{0};
        par_for((size_t)cn + 1, (size_t)1 << 17, [&](size_t lo, size_t hi) { // 32-bit offsets relative to the chunk + the longest read
            uint32_t ml = 0;
            for (size_t i = lo; i < hi; ++i) {
                ho[i] = (uint32_t)(offsets[(size_t)i0 + i] - b0);
                if (i < (size_t)cn) { const uint64_t len = offsets[(size_t)i0 + i + 1] - offsets[(size_t)i0 + i]; if (len > ml) ml = (uint32_t)std::min<uint64_t>(len, 0xffffffffull); }
            }
            uint32_t cur = maxlen_a.load();
            while (ml > cur && !maxlen_a.compare_exchange_weak(cur, ml)) {}
        });
        const uint32_t maxlen = maxlen_a.load();
        const void* hsrc = bases + b0;
        if (!src_pinned) { par_memcpy(s.h_bases.p, bases + b0, cb); hsrc = s.h_bases.p; }
        HIPCHK(hipMemcpyAsync(s.d_bases.p, hsrc, cb, hipMemcpyHostToDevice, s.st));
        HIPCHK(hipMemcpyAsync(s.d_offs.p, s.h_offs.p, (size_t)(cn + 1) * 4, hipMemcpyHostToDevice, s.st));
        RKCHK(fused_device(c, s.d_bases.p, s.d_offs.p, cn, s.d_out.p, maxlen, mode, count_into, s.st, cb));
        if (mode == 0) HIPCHK(hipMemcpyAsync(out_pinned ? (void*)(out4 + i0 * 4) : s.h_out.p, s.d_out.p, (size_t)cn * 16, hipMemcpyDeviceToHost, s.st));
        HIPCHK(hipEventRecord(s.done, s.st));
        s.first = i0; s.n = cn; s.busy = true;
        which ^= 1;
        i0 = i1;
    }
    RKCHK(drain(c->slot[0]));
    RKCHK(drain(c->slot[1]));
    if (flagged) *flagged = nflag;
    return RK_OK;
}

extern "C" int rk_classify_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int32_t* out4) {
    if (!c || !offsets || nreads < 0 || (nreads > 0 && !out4)) return fail(RK_ERR_ARG, "bad arguments");
    if (!c->have_refs) return fail(RK_ERR_STATE, "classify before rk_set_references");
    if (nreads == 0) return RK_OK;
    // Reads the fused kernel is certain to hand back (longer than it stages, or with more windows than the sketch keeps,
    // so that bottom-S selection matters) go to the general path directly instead of being uploaded and hashed twice.
    // This only routes: the fused kernel still flags whatever it cannot answer exactly.
    auto general_only = [&](int64_t i) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        if (len > (uint64_t)FUSED_MAXLEN) return true;
        return hashes_of(c->pol, c->ks, len) > (uint64_t)c->S;
    };
    std::atomic<int64_t> ngen_a{0};
    par_for((size_t)nreads, (size_t)1 << 17, [&](size_t lo, size_t hi) {
        int64_t k = 0;
        for (size_t i = lo; i < hi; ++i) k += general_only((int64_t)i) ? 1 : 0;
        ngen_a += k;
    });
    const int64_t ngen = ngen_a.load();
    if (ngen == nreads || !classify_tile_supported(c->ix.nref, 1)) { // e.g. a nanopore batch: one pass through the general path
        GeneralOut go; go.out4 = out4;
        return general_run(c, bases, nullptr, offsets, nreads, classify_cfg(c), go);
    }
    if (ngen * 8 > nreads) { // mixed batch: the short reads are gathered for the fused kernel, the rest marked for the general path
        std::vector<int64_t> idx;
        idx.reserve((size_t)(nreads - ngen));
        for (int64_t i = 0; i < nreads; ++i) {
            if (general_only(i)) out4[i * 4] = -2;
            else idx.push_back(i);
        }
        SubBatch sb = gather_reads(bases, offsets, idx);
        RKCHK(host_pipeline(c, sb.bases.data(), sb.offs.data(), (int64_t)idx.size(), sb.rows.data(), 0, nullptr));
        scatter_rows(sb, idx, out4);
        return reroute_flagged(c, bases, offsets, nreads, out4);
    }
    int64_t nflag = 0;
    RKCHK(host_pipeline(c, bases, offsets, nreads, out4, 0, nullptr, &nflag));
    return nflag ? reroute_flagged(c, bases, offsets, nreads, out4) : RK_OK; // the pipeline counted the rows the kernel handed back
}

extern "C" int rk_count_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, rk_counter* counter) {
    if (!c || !offsets || nreads < 0 || !counter) return fail(RK_ERR_ARG, "bad arguments");
    if (c->ks.n == 0) return fail(RK_ERR_STATE, "k-mer sizes unknown: call rk_set_references first");
    if (nreads == 0) return RK_OK;
    // reads longer than the fused kernel's limit go through the tile hasher
    bool any_long = false;
    for (int64_t i = 0; i < nreads; ++i) if (offsets[i + 1] - offsets[i] > (uint64_t)FUSED_MAXLEN) { any_long = true; break; }
    if (!any_long) return host_pipeline(c, bases, offsets, nreads, nullptr, 1, counter);
    if (counter->compact) return fail(RK_ERR_NEED_FULL, "reads longer than %d bases: a compact depth map only counts reads that fit the sketch", FUSED_MAXLEN);
    RKCHK(counter_settle(counter));
    GeneralCfg cfg; cfg.ks = c->ks; cfg.inc_counter = counter;
    GeneralOut none;
    return general_run(c, bases, nullptr, offsets, nreads, cfg, none);
}
