// rk_search.hip -- search (include/rkmh_amd.h, "SEARCH"): the resident inverted index of a collection of scaled sketches (value -> the
// references that hold it) and the thresholded many-against-many search on top of it.  The work grows with the values the two sides
// share, not with the number of pairs.  The host-only form is rk_search_scaled_host (rk_scaled_host.cpp); semantics, bounds and
// measurements: DESIGN.md section 15.
#include "rk_sets.hpp"

// (struct rk_scaled_index: rk_sets.hpp)
namespace {

constexpr int SEARCH_T = 256;                  // threads of a workgroup of every kernel here but the scan
constexpr int SEARCH_WAVES = SEARCH_T / 64;
constexpr uint32_t RB = RK_SEARCH_REF_BLOCK;   // references per workgroup: its counters are RB int32 in LDS
constexpr uint32_t WAVE_SPAN = RB / SEARCH_WAVES; // counters one wave reads out, a contiguous span

static_assert(RB * 4 <= 32768 && RB % (SEARCH_WAVES * 64) == 0, "the counters of a reference block fit 32 KB and split into whole rounds per wave");

// ---- the build ------------------------------------------------------------------------------------------------------------
// One wave per row, grid-stride: id[t] = r for every position t of the clamped row r.  (id[] was filled with 2^32 - 1 before: the id
// of a position that no row covers.)
__global__ __launch_bounds__(SEARCH_T) void k_index_ids(const uint64_t* __restrict__ off, uint32_t nref, uint64_t nvalues, uint32_t* __restrict__ id) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * SEARCH_WAVES;
    for (uint64_t r = (uint64_t)blockIdx.x * SEARCH_WAVES + (threadIdx.x >> 6); r < nref; r += nwaves) { // wave-uniform
        uint64_t r0, r1;
        clamped_row(off, r, nvalues, r0, r1);
        for (uint64_t t = r0 + lane; t < r1; t += 64) id[t] = (uint32_t)r;
    }
}

// KEEP_RUN's scatter over the sorted values: keys[j] = the j-th distinct value, post_off[j] = where it first stands, which is where its
// posting list begins; a write lands below nkeys, the scan's total, only.  post_off[nkeys] = n.
__global__ __launch_bounds__(KEEP_T) void k_index_keys(const uint64_t* __restrict__ v, uint64_t n, const uint64_t* __restrict__ pre,
                                                       uint64_t* __restrict__ keys, uint64_t* __restrict__ post_off, uint64_t nkeys) {
    keep_scatter_block<KEEP_RUN, true>(v, n, 0, nullptr, 0, pre, keys, post_off, nkeys);
    if (blockIdx.x == 0 && threadIdx.x == 0) post_off[nkeys] = n;
}

// block_max[b] = the longest posting list among the keys workgroup b strides over (the host takes the maximum of at most 1 024 numbers)
__global__ __launch_bounds__(SEARCH_T) void k_longest_list(const uint64_t* __restrict__ post_off, uint64_t nkeys, uint32_t* __restrict__ block_max) {
    __shared__ uint32_t wmax[SEARCH_WAVES];
    uint64_t best = 0;
    for (uint64_t j = (uint64_t)blockIdx.x * SEARCH_T + threadIdx.x; j < nkeys; j += (uint64_t)gridDim.x * SEARCH_T) {
        const uint64_t a = post_off[j], b = post_off[j + 1];
        best = max(best, b > a ? b - a : (uint64_t)0);
    }
    uint32_t m = (uint32_t)min(best, (uint64_t)0xffffffffu);
    for (int d = 32; d > 0; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) block_max[blockIdx.x] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// ---- the search -----------------------------------------------------------------------------------------------------------
// One workgroup per (query q, reference block b): workgroup w = q * nblk + b counts, for the references [b * RB, b * RB + nrb), how many
// of q's values each holds, in LDS.  The query row is clamped to [0, q_nvalues]; every posting offset is clamped to npost; every id read
// from post[] is checked against the block's range before it indexes the counters; w is checked before it indexes count[] / pre[];
// every write position is checked against cap_hits.  EMIT = false: count[w] = the counters at or above the query's threshold.
// EMIT = true: the counters again, then the hits (q, ref, shared) in ascending reference order from pre[w] on: wave v reads out the
// span [v * WAVE_SPAN, (v + 1) * WAVE_SPAN) of the counters, 64 at a time, positions from ballots.
template <bool EMIT>
__global__ __launch_bounds__(SEARCH_T) void k_search_block(const uint64_t* __restrict__ keys, uint32_t nkeys, const uint64_t* __restrict__ post_off,
                                                           const uint32_t* __restrict__ post, uint64_t npost, uint32_t nref,
                                                           const uint64_t* __restrict__ qv, const uint64_t* __restrict__ qoff, uint32_t nq, uint64_t q_nvalues,
                                                           int32_t min_shared, const int32_t* __restrict__ q_min, uint32_t nblk, uint32_t nwg,
                                                           uint32_t* __restrict__ count, const uint64_t* __restrict__ pre, int32_t* __restrict__ hits,
                                                           uint64_t cap_hits) {
    __shared__ int32_t cnt[RB];
    __shared__ uint32_t wsum[SEARCH_WAVES];
    const uint32_t w = blockIdx.x;
    if (w >= nwg) return; // (whole workgroups)
    const uint32_t q = w / nblk, b = w % nblk;
    if (q >= nq) return;
    const uint32_t base = b * RB;                        // b < nblk = ceil(nref / RB): base < nref
    const uint32_t nrb = min(RB, nref - base);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t r = threadIdx.x; r < RB; r += SEARCH_T) cnt[r] = 0;
    __syncthreads();
    uint64_t q0, q1;
    clamped_row(qoff, q, q_nvalues, q0, q1);
    for (uint64_t t0 = q0 + (uint64_t)wave * 64; t0 < q1; t0 += SEARCH_T) { // wave-uniform: every lane takes part in the ballots below
        const uint64_t t = t0 + lane;
        uint64_t p0 = 0, p1 = 0; // this lane's posting list, narrowed to the block
        if (t < q1) {
            const uint64_t x = qv[t];
            const uint32_t lo = first_not_below(keys, 0u, nkeys, x);
            if (lo < nkeys && keys[lo] == x) {
                const uint64_t a = min(post_off[lo], npost), e = max(min(post_off[lo + 1], npost), a);
                p0 = first_not_below(post, a, e, base);
                p1 = nrb == RB ? first_not_below(post, p0, e, base + nrb) : e; // (the last block: nothing valid lies beyond it)
            }
        }
        const bool wide = p1 - p0 >= 64;
        if (!wide)
            for (uint64_t i = p0; i < p1; ++i) {
                const uint32_t rel = post[i] - base;
                if (rel < nrb) atomicAdd(&cnt[rel], 1);
            }
        uint64_t todo = __ballot(wide); // lists of 64 entries or more: the whole wave walks each
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t s0 = shfl_u64(p0, src), s1 = shfl_u64(p1, src);
            for (uint64_t i = s0 + lane; i < s1; i += 64) {
                const uint32_t rel = post[i] - base;
                if (rel < nrb) atomicAdd(&cnt[rel], 1);
            }
        }
    }
    __syncthreads();
    int32_t thr = min_shared;
    if (q_min) thr = max(thr, q_min[q]);
    thr = max(thr, 1);
    // the counters of this wave's span at or above the threshold
    const uint32_t span0 = wave * WAVE_SPAN;
    uint32_t mine = 0; // wave-uniform
    for (uint32_t r0 = span0; r0 < span0 + WAVE_SPAN; r0 += 64) mine += (uint32_t)__popcll(__ballot(cnt[r0 + lane] >= thr));
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (!EMIT) {
        if (threadIdx.x == 0) count[w] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        return;
    }
    uint64_t at = pre[w];
    for (uint32_t v = 0; v < wave; ++v) at += wsum[v];
    for (uint32_t r0 = span0; r0 < span0 + WAVE_SPAN; r0 += 64) {
        const int32_t n = cnt[r0 + lane];
        const uint64_t bal = __ballot(n >= thr);
        const uint64_t pos = at + lanes_below(bal);
        if (n >= thr && pos < cap_hits) {
            int32_t* __restrict__ h = hits + pos * 3;
            h[0] = (int32_t)q; h[1] = (int32_t)(base + r0 + lane); h[2] = n;
        }
        at += (uint64_t)__popcll(bal);
    }
}

// The build on resident arrays, on stream st; synchronises it.  The scratch (ids, sorted values, the sort's own) is freed on return.
int index_build(rk_scaled_index* ix, const uint64_t* d_values, const uint64_t* d_off, uint32_t nref, uint64_t nvalues, hipStream_t st) {
    ix->nref = nref;
    ix->npost = nvalues;
    struct Scratch { DevBuf ids, sorted, tmp, cnt, pre; ~Scratch() { for (DevBuf* b : {&ids, &sorted, &tmp, &cnt, &pre}) b->release(); } } s;
    RKCHK(ix->post.reserve((size_t)nvalues * 4 + 4));
    uint64_t nkeys = 0;
    if (nvalues) {
        // 1. the reference id of every value position
        RKCHK(s.ids.reserve((size_t)nvalues * 4));
        HIPCHK(hipMemsetAsync(s.ids.p, 0xff, (size_t)nvalues * 4, st));
        hipLaunchKernelGGL(k_index_ids, dim3(wave_grid(nref, SEARCH_WAVES)), dim3(SEARCH_T), 0, st, d_off, nref, nvalues, s.ids.as<uint32_t>());
        HIPCHK(hipGetLastError());
        // 2. the pairs ordered by value; the sort is stable, so the ids of one value stay ascending
        size_t tmp_bytes = 0;
        HIPCHK(sort_pairs_u64_u32_temp_bytes(nvalues, &tmp_bytes));
        RKCHK(s.tmp.reserve(tmp_bytes));
        RKCHK(s.sorted.reserve((size_t)nvalues * 8));
        HIPCHK(launch_sort_pairs_u64_u32(d_values, s.sorted.as<uint64_t>(), s.ids.as<uint32_t>(), ix->post.as<uint32_t>(), nvalues, s.tmp.p, tmp_bytes, st));
        // 3. the first of every value is its key; where it stands is where its list begins
        const uint64_t nblocks = (nvalues + KEEP_BLK - 1) / KEEP_BLK; // < 2^23: nvalues < 2^32
        RKCHK(keep_counts<KEEP_RUN>(s.cnt, s.pre, s.sorted.as<uint64_t>(), nvalues, 0, nullptr, 0, nullptr, st));
        HIPCHK(hipMemcpyAsync(&nkeys, s.pre.as<uint64_t>() + nblocks, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (nkeys < 1 || nkeys > nvalues) return fail(RK_ERR_HIP, "scaled index: %llu keys of %llu values", (unsigned long long)nkeys, (unsigned long long)nvalues);
        RKCHK(ix->keys.reserve((size_t)nkeys * 8));
        RKCHK(ix->post_off.reserve((size_t)(nkeys + 1) * 8));
        hipLaunchKernelGGL(k_index_keys, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, s.sorted.as<uint64_t>(), nvalues, s.pre.as<uint64_t>(),
                           ix->keys.as<uint64_t>(), ix->post_off.as<uint64_t>(), nkeys);
        const uint32_t lblocks = (uint32_t)std::min<uint64_t>((nkeys + SEARCH_T - 1) / SEARCH_T, 1024);
        uint32_t* d_max = s.ids.as<uint32_t>(); // (the sort is done with the ids; lblocks <= nvalues entries are there)
        hipLaunchKernelGGL(k_longest_list, dim3(lblocks), dim3(SEARCH_T), 0, st, ix->post_off.as<uint64_t>(), nkeys, d_max);
        HIPCHK(hipGetLastError());
        std::vector<uint32_t> bm(lblocks);
        HIPCHK(hipMemcpyAsync(bm.data(), d_max, (size_t)lblocks * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ix->longest = *std::max_element(bm.begin(), bm.end());
    } else {
        RKCHK(ix->keys.reserve(8));
        RKCHK(ix->post_off.reserve(8));
        HIPCHK(hipMemsetAsync(ix->post_off.p, 0, 8, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    ix->nkeys = nkeys;
    return RK_OK;
}

int check_index_shape(const rk_ctx* c, int64_t nref, rk_scaled_index** idx) {
    if (!c || !idx) return fail(RK_ERR_ARG, "bad arguments");
    if (nref < 1) return fail(RK_ERR_ARG, "scaled index: need at least one reference sketch, got %lld", (long long)nref);
    if (nref > 0x7fffffffll) return fail(RK_ERR_LIMIT, "scaled index: %lld reference sketches are more than 2^31-1", (long long)nref);
    return RK_OK;
}
int check_values_limit(uint64_t nvalues) {
    if (nvalues > 0xffffffffull) return fail(RK_ERR_LIMIT, "scaled index: %llu reference values are more than 2^32-1", (unsigned long long)nvalues);
    return RK_OK;
}

int make_index(rk_ctx* c, const uint64_t* d_values, const uint64_t* d_off, int64_t nref, uint64_t nvalues, hipStream_t st, rk_scaled_index** idx) {
    std::unique_ptr<rk_scaled_index, void (*)(rk_scaled_index*)> ix(new rk_scaled_index, rk_scaled_index_destroy);
    ix->ctx = c;
    ix->device = c->device;
    RKCHK(index_build(ix.get(), d_values, d_off, (uint32_t)nref, nvalues, st));
    *idx = ix.release();
    return RK_OK;
}

} // namespace

// ---- the steps of a search, shared with rk_multigather.hip (declared in rk_sets.hpp) ----------------------------------------------
int rk::check_search_shape(const rk_ctx* c, const rk_scaled_index* ix, int64_t nq, int min_shared, uint64_t* nwg, uint32_t* nblk, const char* who) {
    if (ix->ctx != c) return fail(RK_ERR_ARG, "%s: the index was made on another context", who);
    if (nq < 1) return fail(RK_ERR_ARG, "%s: need at least one query sketch, got %lld", who, (long long)nq);
    if (min_shared < 1) return fail(RK_ERR_ARG, "%s: min_shared %d is below 1", who, min_shared);
    if (nq > 0x7fffffffll) return fail(RK_ERR_LIMIT, "%s: %lld query sketches are more than 2^31-1", who, (long long)nq);
    *nblk = (ix->nref + RB - 1) / RB;
    *nwg = (uint64_t)nq * *nblk;
    if (*nwg > 0xffffffull) return fail(RK_ERR_LIMIT, "%s: %lld queries x %u reference blocks are more workgroups than one launch takes", who, (long long)nq, *nblk);
    return RK_OK;
}

// pass 1 and the scan on stream st -> *total (synchronises st); the caller holds ix->mu
int rk::search_count(rk_scaled_index* ix, const uint64_t* d_qv, const uint64_t* d_qo, uint32_t nq, uint64_t q_nvalues, int min_shared, const int32_t* d_qmin,
                 uint32_t nblk, uint32_t nwg, hipStream_t st, uint64_t* total, const char* who) {
    RKCHK(ix->w_cnt.reserve((size_t)nwg * 4));
    RKCHK(ix->w_pre.reserve(((size_t)nwg + 1) * 8));
    hipLaunchKernelGGL(k_search_block<false>, dim3(nwg), dim3(SEARCH_T), 0, st, ix->keys.as<uint64_t>(), (uint32_t)ix->nkeys, ix->post_off.as<uint64_t>(),
                       ix->post.as<uint32_t>(), ix->npost, ix->nref, d_qv, d_qo, nq, q_nvalues, (int32_t)min_shared, d_qmin, nblk, nwg, ix->w_cnt.as<uint32_t>(),
                       (const uint64_t*)nullptr, (int32_t*)nullptr, (uint64_t)0);
    hipLaunchKernelGGL(k_scan_blocks<uint32_t>, dim3(1), dim3(1024), 0, st, ix->w_cnt.as<uint32_t>(), (uint64_t)nwg, ix->w_pre.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(total, ix->w_pre.as<uint64_t>() + nwg, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (*total > (uint64_t)nq * ix->nref) return fail(RK_ERR_HIP, "%s: %llu hits of %u x %u pairs", who, (unsigned long long)*total, nq, ix->nref);
    return RK_OK;
}
int rk::search_emit(rk_scaled_index* ix, const uint64_t* d_qv, const uint64_t* d_qo, uint32_t nq, uint64_t q_nvalues, int min_shared, const int32_t* d_qmin,
                uint32_t nblk, uint32_t nwg, hipStream_t st, int32_t* d_hits, uint64_t cap_hits) {
    hipLaunchKernelGGL(k_search_block<true>, dim3(nwg), dim3(SEARCH_T), 0, st, ix->keys.as<uint64_t>(), (uint32_t)ix->nkeys, ix->post_off.as<uint64_t>(),
                       ix->post.as<uint32_t>(), ix->npost, ix->nref, d_qv, d_qo, nq, q_nvalues, (int32_t)min_shared, d_qmin, nblk, nwg, ix->w_cnt.as<uint32_t>(),
                       ix->w_pre.as<uint64_t>(), d_hits, cap_hits);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

extern "C" void rk_scaled_index_destroy(rk_scaled_index* ix) {
    if (!ix) return;
    hipError_t e = hipSetDevice(ix->device); (void)e;
    for (DevBuf* b : {&ix->keys, &ix->post_off, &ix->post, &ix->w_cnt, &ix->w_pre, &ix->w_qv, &ix->w_qo, &ix->w_qmin, &ix->w_hits, &ix->w_cl, &ix->w_mg, &ix->w_mg_io, &ix->w_mg_out}) b->release();
    delete ix;
}

extern "C" int rk_scaled_index_stats(const rk_scaled_index* ix, rk_scaled_index_stats_t* out) {
    if (!ix || !out || out->struct_size < sizeof(uint32_t)) return fail(RK_ERR_ARG, "bad arguments");
    rk_scaled_index_stats_t s{};
    s.nref = ix->nref; s.npost = ix->npost; s.nkeys = ix->nkeys; s.longest_posting = ix->longest;
    const uint32_t n = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof s);
    s.struct_size = n;
    memcpy(out, &s, n);
    return RK_OK;
}

extern "C" int rk_scaled_index_create_device(rk_ctx* c, const void* d_values, const void* d_offsets, int64_t nref, uint64_t nvalues, void* hip_stream,
                                             rk_scaled_index** idx) {
    RKCHK(check_index_shape(c, nref, idx));
    if (!d_offsets || (!d_values && nvalues)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_values_limit(nvalues));
    RKCHK(set_dev(c));
    return make_index(c, (const uint64_t*)d_values, (const uint64_t*)d_offsets, nref, nvalues, (hipStream_t)hip_stream, idx);
}

extern "C" int rk_scaled_index_create(rk_ctx* c, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, rk_scaled_index** idx) {
    RKCHK(check_index_shape(c, nref, idx));
    if (!r_offsets) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_csr(r_offsets, nref, "scaled index: ", "the references", RK_ERR_ARG));
    const uint64_t rn = r_offsets[nref] - r_offsets[0]; // the values the rows cover
    if (rn && !r_values) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_values_limit(rn));
    RKCHK(set_dev(c));
    struct Up { DevBuf v, o; ~Up() { v.release(); o.release(); } } up;
    RKCHK(up.v.reserve((size_t)rn * 8 + 8));
    RKCHK(up.o.reserve(((size_t)nref + 1) * 8));
    std::vector<uint64_t> off;
    RKCHK(upload_csr(r_values, r_offsets, nref, up.v.as<uint64_t>(), up.o.as<uint64_t>(), off, c->st));
    return make_index(c, up.v.as<uint64_t>(), up.o.as<uint64_t>(), nref, rn, c->st, idx); // (synchronises: off lives until there)
}

extern "C" int rk_search_scaled_device(rk_ctx* c, rk_scaled_index* ix, const void* d_q_values, const void* d_q_offsets, int64_t nq, uint64_t q_nvalues,
                                       int min_shared, const void* d_q_min, void* d_hits, uint64_t cap_hits, uint64_t* nhits, void* hip_stream) {
    if (!c || !ix || !d_q_offsets || !nhits || (!d_q_values && q_nvalues) || (!d_hits && cap_hits)) return fail(RK_ERR_ARG, "bad arguments");
    uint64_t nwg = 0, total = 0;
    uint32_t nblk = 0;
    RKCHK(check_search_shape(c, ix, nq, min_shared, &nwg, &nblk, "search"));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    const uint64_t* qv = (const uint64_t*)d_q_values;
    const uint64_t* qo = (const uint64_t*)d_q_offsets;
    RKCHK(search_count(ix, qv, qo, (uint32_t)nq, q_nvalues, min_shared, (const int32_t*)d_q_min, nblk, (uint32_t)nwg, st, &total, "search"));
    if (total && cap_hits) {
        RKCHK(search_emit(ix, qv, qo, (uint32_t)nq, q_nvalues, min_shared, (const int32_t*)d_q_min, nblk, (uint32_t)nwg, st, (int32_t*)d_hits, cap_hits));
        HIPCHK(hipStreamSynchronize(st));
    }
    *nhits = total;
    return RK_OK;
}

extern "C" int rk_search_scaled(rk_ctx* c, rk_scaled_index* ix, const uint64_t* q_values, const uint64_t* q_offsets, int64_t nq, int min_shared,
                                const int32_t* q_min, rk_search_hit** hits, uint64_t* nhits) {
    if (!c || !ix || !q_offsets || !hits || !nhits) return fail(RK_ERR_ARG, "bad arguments");
    uint64_t nwg = 0, total = 0;
    uint32_t nblk = 0;
    RKCHK(check_search_shape(c, ix, nq, min_shared, &nwg, &nblk, "search"));
    RKCHK(check_csr(q_offsets, nq, "search: ", "the queries", RK_ERR_ARG));
    for (int64_t i = 0; q_min && i < nq; ++i)
        if (q_min[i] < 1) return fail(RK_ERR_ARG, "search: q_min %d of query %lld is below 1", q_min[i], (long long)i);
    const uint64_t qn = q_offsets[nq] - q_offsets[0];
    if (qn && !q_values) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    RKCHK(ix->w_qv.reserve((size_t)qn * 8 + 8));
    RKCHK(ix->w_qo.reserve(((size_t)nq + 1) * 8));
    if (q_min) RKCHK(ix->w_qmin.reserve((size_t)nq * 4));
    std::vector<uint64_t> off;
    const uint64_t* qv = ix->w_qv.as<uint64_t>();
    const uint64_t* qo = ix->w_qo.as<uint64_t>();
    const int32_t* qm = q_min ? ix->w_qmin.as<int32_t>() : nullptr;
    RKCHK(upload_csr(q_values, q_offsets, nq, ix->w_qv.as<uint64_t>(), ix->w_qo.as<uint64_t>(), off, c->st));
    if (q_min) HIPCHK(hipMemcpyAsync(ix->w_qmin.p, q_min, (size_t)nq * 4, hipMemcpyHostToDevice, c->st));
    RKCHK(search_count(ix, qv, qo, (uint32_t)nq, qn, min_shared, qm, nblk, (uint32_t)nwg, c->st, &total, "search")); // (synchronises: off lives until there)
    rk_search_hit* out = (rk_search_hit*)malloc(sizeof(rk_search_hit) * (size_t)std::max<uint64_t>(total, 1));
    if (!out) return fail(RK_ERR_NOMEM, "malloc of %llu hits", (unsigned long long)total);
    if (total) {
        int r = ix->w_hits.reserve((size_t)total * sizeof(rk_search_hit));
        if (r == RK_OK) r = search_emit(ix, qv, qo, (uint32_t)nq, qn, min_shared, qm, nblk, (uint32_t)nwg, c->st, ix->w_hits.as<int32_t>(), total);
        if (r == RK_OK) {
            hipError_t e = hipMemcpyAsync(out, ix->w_hits.p, (size_t)total * sizeof(rk_search_hit), hipMemcpyDeviceToHost, c->st);
            if (e == hipSuccess) e = hipStreamSynchronize(c->st);
            if (e != hipSuccess) r = fail(RK_ERR_HIP, "search: downloading %llu hits failed: %s", (unsigned long long)total, hipGetErrorString(e));
        }
        if (r != RK_OK) { free(out); return r; }
    }
    *hits = out;
    *nhits = total;
    return RK_OK;
}
