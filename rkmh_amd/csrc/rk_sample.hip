// rk_sample.hip -- the sample accumulator (include/rkmh_amd.h, "SAMPLE SKETCHES"): ONE scaled sketch, with or without abundances,
// that stays on the device while reads are fed to it batch by batch or straight from a FASTQ slot.  k_sample_keep hashes the windows
// of a resident batch and keeps only the values under the threshold (the per-window hash array of the general path never exists);
// the kept values wait in a pending array behind the resident distinct set until a fold -- sort, drop repeats, sum the run's counts
// -- unites them with it.  The union over all reads is therefore taken on the device; the host sees a cursor per feed and the
// finished arrays.  Semantics, sizes and measurements: DESIGN.md section 20.
#include "rk_sets.hpp"
#include "rk_tile_walk.hpp"

struct rk_sample {
    rk_ctx* ctx = nullptr; // compared and used while feeding; destroy does not follow it
    int device = 0;
    KsArr ks{};
    int kmax = 0;
    uint64_t max_hash = 0;
    bool with_abund = false;
    // keys[cur] holds the resident distinct values at [0, n_res) and the pending ones behind them, at [n_res, n_res + pend_cap);
    // cnts[cur] lies parallel (abundances only).  The other pair takes the sorted array of a fold.
    DevBuf keys[2], cnts[2];
    int cur = 0;
    uint64_t n_res = 0, pend_cap = 0, cap_total = 0;
    uint64_t pending = 0;   // the host's copy of the cursor: kept values waiting behind the resident set
    uint64_t last_need = 0; // what the latest batch kept: the room the next one is expected to want
    uint64_t seen_bases = 0, last_bases = 0; // the device's base total at the latest look; the bases of the latest batch (sizes the next grid)
    DevBuf state;           // uint64[4] on the device: the cursor, sequences fed, bases fed
    PinBuf h_state;
    DevBuf w_cnt, w_pre, w_src, w_tmp, w_bases, w_offs;
    uint32_t folds = 0, retries = 0;
    uint64_t kept = 0;
    // a bottom sample ("BOTTOM SAMPLES"): sketch_size > 0, counts always kept, and max_hash is its threshold T, which a cut lowers
    int sketch_size = 0;
    uint32_t min_copies = 1;
    uint32_t cuts = 0;
    uint64_t weight = 0;    // the weight of the resident set at the latest look of a cut
    DevBuf cut_state;       // uint64[3] on the device: what k_cut_find leaves (cut length, threshold, weight)
    std::mutex mu; // feeds, folds and reads of one sample take turns
};

namespace {

constexpr int SK_T = TW_T;                                              // the workgroup of the tile walk (rk_tile_walk.hpp)
constexpr int SK_STAGE = 1024;                                         // kept values a workgroup holds back in LDS
constexpr uint64_t SK_DEFAULT_PENDING = (uint64_t)1 << 22;             // values (32 MB): DESIGN.md section 20
constexpr uint64_t SK_PIECE_BASES = (uint64_t)64 << 20;                // rk_sample_add_batch uploads pieces of about this many bases
constexpr uint32_t SK_FIRST_READS = 4096;                              // a bottom sample before its first cut: reads of the first sub-batch, doubling

// the workgroup's staged values leave for the pending array: one 64-bit atomicAdd on the cursor says where; the store happens only
// when all of them fit below cap, the cursor advances either way.  Called by all threads with the same m (a register of each, never
// read from LDS: no thread can see another's later round), after a barrier behind the last store to stage[].
__device__ __forceinline__ void flush_stage(const uint64_t* stage, uint32_t m, uint64_t* flush_at, uint64_t* __restrict__ pend, uint64_t cap,
                                            unsigned long long* __restrict__ state) {
    if (m == 0) return;
    if (threadIdx.x == 0) *flush_at = atomicAdd(&state[0], (unsigned long long)m);
    __syncthreads();
    const uint64_t at = *flush_at;
    if (at + m <= cap)
        for (uint32_t i = threadIdx.x; i < m; i += SK_T) pend[at + i] = stage[i];
    __syncthreads(); // stage[] and flush_at may be written again
}

// The windows of a resident batch (walk_tiles, rk_tile_walk.hpp: the bases as one piece cut into tiles, read starts in a bitmap, every
// window hashed at the k this instantiation serves); the hashes 0 < h <= max_hash are compacted with wave ballots into stage[] and leave
// for the pending array whenever fewer than SK_T places are left there.
template <int KT>
__global__ __launch_bounds__(SK_T) void k_sample_keep(const uint8_t* __restrict__ bases, const uint32_t* __restrict__ offs, uint32_t n, KsArr ks, int kmax,
                                                      uint64_t max_hash, DevPolicy pol, uint64_t* __restrict__ pend, uint64_t cap,
                                                      unsigned long long* __restrict__ state, int add_totals) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[stage_lds_dwords(HASH_TILE_MAXB)];
    __shared__ uint32_t bnd[TW_BND_DW];
    __shared__ uint64_t stage[SK_STAGE];
    __shared__ uint64_t flush_at;
    __shared__ uint32_t wcnt[2][SK_T / 64]; // kept per wave in this round; two sets in turn, so that a wave a round ahead writes the other one
    const uint32_t first = offs[0], end = offs[n];
    if (add_totals && blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&state[1], (unsigned long long)n);
        atomicAdd(&state[2], (unsigned long long)(end > first ? end - first : 0u));
    }
    if (end <= first) return;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t nstage = 0, par = 0; // values waiting in stage[], the set of wcnt in turn: the same in every thread
    walk_tiles<KT>(bases, offs, n, first, end, ks, kmax, pol, lds, bnd, [&](uint64_t h) {
        const bool keep = h != 0 && h <= max_hash;
        const uint64_t bal = __ballot(keep);
        if ((threadIdx.x & 63) == 0) wcnt[par][wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < SK_T / 64; ++w) {
            const uint32_t cw = wcnt[par][w];
            before += w < wave ? cw : 0u;
            all += cw;
        }
        const uint32_t at = nstage + before + lanes_below(bal);
        if (keep && at < (uint32_t)SK_STAGE) stage[at] = h; // (always: at most SK_STAGE - SK_T values wait when a round begins)
        nstage += all;
        par ^= 1u;
        if (nstage > (uint32_t)(SK_STAGE - SK_T)) {
            __syncthreads();
            flush_stage(stage, nstage, &flush_at, pend, cap, state);
            nstage = 0;
        }
    });
    __syncthreads();
    flush_stage(stage, nstage, &flush_at, pend, cap, state);
}

// KEEP_RUN's scatter that also notes where each first stood (k_keep_first_src's form without segments)
__global__ __launch_bounds__(KEEP_T) void k_keep_run_src(const uint64_t* __restrict__ v, uint64_t n, const uint64_t* __restrict__ pre, uint64_t* __restrict__ out,
                                                         uint64_t* __restrict__ src, uint64_t out_cap) {
    keep_scatter_block<KEEP_RUN, true>(v, n, 0, nullptr, 0, pre, out, src, out_cap);
}

// out[j] = min(2^32 - 1, the sum of w[src[j] .. src[j + 1])) for run j < m (the last run ends at n): rk_merge_scaled_abund's rule.  A
// lane sums a run of up to 16 entries itself; longer runs are summed one after the other by the whole wave.  Sums are 64-bit: fewer
// than 2^32 entries below 2^32 each.
__global__ __launch_bounds__(KEEP_T) void k_run_sums(const uint64_t* __restrict__ src, uint64_t m, uint64_t n, const uint32_t* __restrict__ w,
                                                     uint32_t* __restrict__ out) {
    const uint64_t j = (uint64_t)blockIdx.x * KEEP_T + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    const bool have = j < m;
    uint64_t begin = 0, end = 0;
    if (have) {
        begin = min(src[j], n);
        end = max(min(j + 1 < m ? src[j + 1] : n, n), begin);
    }
    uint64_t sum = 0;
    const bool is_long = end - begin > 16;
    if (!is_long)
        for (uint64_t t = begin; t < end; ++t) sum += w[t];
    uint64_t todo = __ballot(is_long);
    while (todo) { // (wave-uniform)
        const int l = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint64_t b = shfl_u64(begin, l), e = shfl_u64(end, l);
        uint64_t part = 0;
        for (uint64_t t = b + (uint64_t)lane; t < e; t += 64) part += w[t];
        for (int d = 32; d > 0; d >>= 1) part += shfl_xor_u64(part, d);
        if (lane == l) sum = part;
    }
    if (have) out[j] = (uint32_t)min(sum, (uint64_t)0xffffffffu);
}

// `bytes` behind b, the first keep_bytes of what it holds carried over (DevBuf::reserve drops the contents)
int grow_preserve(DevBuf& b, size_t bytes, size_t keep_bytes, hipStream_t st) {
    if (bytes <= b.cap) return RK_OK;
    DevBuf nb;
    RKCHK(nb.reserve(bytes));
    if (keep_bytes && b.p) {
        hipError_t e = hipMemcpyAsync(nb.p, b.p, keep_bytes, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { nb.release(); return fail(RK_ERR_HIP, "copy into a grown sample array failed: %s", hipGetErrorString(e)); }
    }
    b.release();
    b = nb;
    return RK_OK;
}

// room for `total` values in both pairs of arrays; the resident set stays where it is
int ensure_capacity(rk_sample* s, uint64_t total, hipStream_t st) {
    if (total <= s->cap_total) return RK_OK;
    if (total > ((uint64_t)1 << 40)) return fail(RK_ERR_LIMIT, "a sample of %llu values", (unsigned long long)total);
    const uint64_t cap = total + total / 4 + 64;
    RKCHK(grow_preserve(s->keys[s->cur], (size_t)cap * 8, (size_t)s->n_res * 8, st));
    RKCHK(s->keys[s->cur ^ 1].reserve((size_t)cap * 8));
    if (s->with_abund) {
        RKCHK(grow_preserve(s->cnts[s->cur], (size_t)cap * 4, (size_t)s->n_res * 4, st));
        RKCHK(s->cnts[s->cur ^ 1].reserve((size_t)cap * 4));
    }
    s->cap_total = cap;
    return RK_OK;
}

// The m values behind the resident set (their counts too when !fill_ones) are united with it: sort, keep the first of every run,
// sum the runs' counts.  Ends with the cursor at 0, room for pend_cap values behind the new resident set, and st synchronised.
int fold_values(rk_sample* s, uint64_t m, bool fill_ones, hipStream_t st) {
    if (m == 0) return RK_OK;
    const uint64_t n = s->n_res + m;
    uint64_t* A = s->keys[s->cur].as<uint64_t>();
    uint64_t* B = s->keys[s->cur ^ 1].as<uint64_t>();
    uint32_t* VA = s->cnts[s->cur].as<uint32_t>();
    uint32_t* VB = s->cnts[s->cur ^ 1].as<uint32_t>();
    uint64_t *sorted, *out;
    size_t tmp_bytes = 0;
    if (s->with_abund) {
        if (fill_ones) HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(VA + s->n_res), 1, (size_t)m, st));
        HIPCHK(sort_pairs_u64_u32_temp_bytes(n, &tmp_bytes));
        RKCHK(s->w_tmp.reserve(tmp_bytes));
        HIPCHK(launch_sort_pairs_u64_u32(A, B, VA, VB, n, s->w_tmp.p, tmp_bytes, st));
        sorted = B; out = A;
    } else {
        HIPCHK(sort_u64_temp_bytes(n, &tmp_bytes));
        RKCHK(s->w_tmp.reserve(tmp_bytes));
        HIPCHK(launch_sort_u64(A, n, s->w_tmp.p, tmp_bytes, st));
        sorted = A; out = B;
    }
    RKCHK(keep_counts<KEEP_RUN>(s->w_cnt, s->w_pre, sorted, n, 0, nullptr, 0, nullptr, st));
    const uint64_t nblocks = (n + KEEP_BLK - 1) / KEEP_BLK;
    uint64_t* h = s->h_state.as<uint64_t>();
    HIPCHK(hipMemcpyAsync(h + 4, s->w_pre.as<uint64_t>() + nblocks, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint64_t nd = h[4];
    if (nd == 0 || nd > n) return fail(RK_ERR_HIP, "sample fold: %llu distinct values of %llu", (unsigned long long)nd, (unsigned long long)n);
    if (s->with_abund) {
        if ((nd + KEEP_T - 1) / KEEP_T > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%llu distinct values are more than one run-sum launch takes", (unsigned long long)nd);
        RKCHK(s->w_src.reserve((size_t)nd * 8));
        hipLaunchKernelGGL(k_keep_run_src, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, sorted, n, s->w_pre.as<uint64_t>(), out, s->w_src.as<uint64_t>(), nd);
        hipLaunchKernelGGL(k_run_sums, dim3((uint32_t)((nd + KEEP_T - 1) / KEEP_T)), dim3(KEEP_T), 0, st, s->w_src.as<uint64_t>(), nd, n, VB, VA);
        HIPCHK(hipGetLastError());
    } else {
        RKCHK(keep_scatter<KEEP_RUN>(s->w_pre, sorted, n, 0, nullptr, 0, out, nd, st));
        s->cur ^= 1; // the distinct values went to the other array
    }
    HIPCHK(hipMemsetAsync(s->state.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    s->n_res = nd;
    s->pending = 0;
    ++s->folds;
    return ensure_capacity(s, s->n_res + s->pend_cap, st);
}
int fold_pending(rk_sample* s, hipStream_t st) { return fold_values(s, s->pending, true, st); }

// A bottom sample behind a fold -- the resident set sorted and distinct, nothing pending --: where its bottom sketch_size ends
// (rk_bottom.hip); when it ends inside the set, T comes down to the value there and the set is cut off behind it.  One 24-byte look.
int cut_resident(rk_sample* s, hipStream_t st) {
    uint64_t* h = s->h_state.as<uint64_t>();
    RKCHK(bottom_cut_device(s->w_cnt, s->w_pre, s->keys[s->cur].as<uint64_t>(), s->cnts[s->cur].as<uint32_t>(), s->n_res, (uint32_t)s->sketch_size, s->min_copies,
                            s->ctx->dedup, s->cut_state.as<uint64_t>(), st));
    HIPCHK(hipMemcpyAsync(h + 5, s->cut_state.p, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (h[5] > s->n_res) return fail(RK_ERR_HIP, "sample cut at %llu of %llu values", (unsigned long long)h[5], (unsigned long long)s->n_res);
    s->weight = h[7];
    if (h[5]) {
        if (h[5] < s->n_res || h[6] < s->max_hash) ++s->cuts; // (a cut behind its own last entry changes nothing and is not counted)
        s->n_res = h[5];
        s->max_hash = h[6];
    }
    return RK_OK;
}
int fold_and_cut(rk_sample* s, hipStream_t st) {
    RKCHK(fold_pending(s, st));
    return s->sketch_size ? cut_resident(s, st) : RK_OK;
}

int launch_keep(rk_sample* s, const void* d_bases, const void* d_offs, uint32_t n, uint64_t bound_bases, int add_totals, hipStream_t st) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((bound_bases + HASH_TILE_WIN - 1) / HASH_TILE_WIN, 1), 4096);
    uint64_t* pend = s->keys[s->cur].as<uint64_t>() + s->n_res;
    unsigned long long* state = s->state.as<unsigned long long>();
    bool k16 = false, other = false;
    for (int j = 0; j < s->ks.n; ++j) (s->ks.k[j] == 16 ? k16 : other) = true;
    if (k16)
        hipLaunchKernelGGL(k_sample_keep<16>, dim3(grid), dim3(SK_T), 0, st, (const uint8_t*)d_bases, (const uint32_t*)d_offs, n, s->ks, s->kmax, s->max_hash,
                           s->ctx->pol, pend, s->pend_cap, state, add_totals);
    if (other)
        hipLaunchKernelGGL(k_sample_keep<0>, dim3(grid), dim3(SK_T), 0, st, (const uint8_t*)d_bases, (const uint32_t*)d_offs, n, s->ks, s->kmax, s->max_hash,
                           s->ctx->pol, pend, s->pend_cap, state, k16 ? 0 : add_totals);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

// one batch of resident reads into the sample; the caller holds s->mu and has set the device.  Synchronises st.
int feed_one(rk_sample* s, const void* d_bases, const void* d_offs, uint32_t n, uint64_t bound_bases, hipStream_t st) {
    uint64_t* h = s->h_state.as<uint64_t>();
    const uint64_t before = s->pending;
    // a batch whose size the caller cannot say (the device entry) gets the grid of twice the batch before it: the base total comes
    // back with the cursor, in the same look; the kernel strides, so any grid is right
    if (bound_bases == 0) bound_bases = s->last_bases ? 2 * s->last_bases : 0xffffffffull;
    RKCHK(launch_keep(s, d_bases, d_offs, n, bound_bases, 1, st));
    HIPCHK(hipMemcpyAsync(h, s->state.p, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->last_bases = h[2] - s->seen_bases;
    s->seen_bases = h[2];
    if (h[0] < before) return fail(RK_ERR_HIP, "sample cursor went back from %llu to %llu", (unsigned long long)before, (unsigned long long)h[0]);
    const uint64_t need = h[0] - before;
    if (h[0] > s->pend_cap) {
        // some workgroup found no room: the cursor goes back to where the batch began (what the batch did store lies behind it and is
        // forgotten), the values from before are folded, the pending array grows to what the batch asked for, and the batch runs again
        h[0] = before;
        HIPCHK(hipMemcpyAsync(s->state.p, h, 8, hipMemcpyHostToDevice, st)); // (h[0] is written next by the copy behind the second run, on this stream)
        RKCHK(fold_pending(s, st)); // (a bottom sample: no cut here -- T stays, so the second run keeps what the first kept)
        if (need > s->pend_cap) {
            s->pend_cap = need;
            RKCHK(ensure_capacity(s, s->n_res + s->pend_cap, st));
        }
        ++s->retries;
        RKCHK(launch_keep(s, d_bases, d_offs, n, bound_bases, 0, st));
        HIPCHK(hipMemcpyAsync(h, s->state.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (h[0] != need) return fail(RK_ERR_HIP, "sample batch kept %llu values at first and %llu when run again", (unsigned long long)need, (unsigned long long)h[0]);
    }
    s->pending = h[0];
    s->kept += need;
    s->last_need = need;
    // the look is paid for: when the next batch, if it keeps what this one kept, would not fit, fold now and spare it the second run
    // (a bottom sample also folds, and then cuts, whenever more waits than is resident: T follows the data at a cost that stays
    // proportional to what was kept; the first feed always does)
    if (s->pend_cap - s->pending < s->last_need || (s->sketch_size && s->pending > s->n_res)) RKCHK(fold_and_cut(s, st));
    return RK_OK;
}
// A bottom sample that has not cut yet keeps every window: a large batch goes in as sub-batches of 4 096, 8 192, ... reads (offs + i
// with a smaller n is a batch like any other) until the first cut has brought T down, and the rest then goes in as one.
int feed_locked(rk_sample* s, const void* d_bases, const void* d_offs, uint32_t n, uint64_t bound_bases, hipStream_t st) {
    if (!s->sketch_size || s->cuts || n <= SK_FIRST_READS) return feed_one(s, d_bases, d_offs, n, bound_bases, st);
    const uint32_t* offs = (const uint32_t*)d_offs;
    uint32_t i = 0;
    for (uint32_t step = SK_FIRST_READS; s->cuts == 0 && n - i > step; i += step, step *= 2) RKCHK(feed_one(s, d_bases, offs + i, step, 0, st));
    return feed_one(s, d_bases, offs + i, n - i, bound_bases, st);
}

int check_sample(const rk_sample* s) {
    if (!s || !s->ctx) return fail(RK_ERR_ARG, "sample is NULL");
    return RK_OK;
}

} // namespace

namespace rk {
rk_ctx* sample_ctx(const rk_sample* s) { return s ? s->ctx : nullptr; }
int sample_feed_device(rk_sample* s, const void* d_bases, const void* d_offs_u32, int64_t nseq, uint64_t bound_bases, hipStream_t st) {
    RKCHK(check_sample(s));
    if (nseq < 0 || (nseq > 0 && (!d_bases || !d_offs_u32))) return fail(RK_ERR_ARG, "bad arguments");
    if (nseq > 0x7fffffffll) return fail(RK_ERR_LIMIT, "more than 2^31-1 sequences in one batch");
    if (nseq == 0) return RK_OK;
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    return feed_locked(s, d_bases, d_offs_u32, (uint32_t)nseq, bound_bases, st);
}
}

extern "C" void rk_sample_destroy(rk_sample* s) {
    if (!s) return;
    hipError_t e = hipSetDevice(s->device); (void)e;
    // (every feed, fold and download of the sample ended with its stream synchronised: nothing of it is in flight)
    for (DevBuf* b : {&s->keys[0], &s->keys[1], &s->cnts[0], &s->cnts[1], &s->state, &s->w_cnt, &s->w_pre, &s->w_src, &s->w_tmp, &s->w_bases, &s->w_offs, &s->cut_state}) b->release();
    s->h_state.release();
    delete s;
}

extern "C" int rk_sample_create(rk_ctx* c, const int* ks, int nks, uint64_t max_hash, int with_abund, uint64_t pending_cap, rk_sample** out) {
    if (!c || !out) return fail(RK_ERR_ARG, "bad arguments");
    KsArr ka{};
    RKCHK(check_ks(ks, nks, &ka));
    if (max_hash == 0) return fail(RK_ERR_ARG, "max_hash is 0: no value could be kept");
    if (pending_cap > ((uint64_t)1 << 36)) return fail(RK_ERR_LIMIT, "a pending array of %llu values", (unsigned long long)pending_cap);
    RKCHK(set_dev(c));
    rk_sample* s = new rk_sample();
    struct Guard { rk_sample* s; ~Guard() { if (s) rk_sample_destroy(s); } } guard{s};
    s->ctx = c; s->device = c->device; s->ks = ka; s->max_hash = max_hash; s->with_abund = with_abund != 0;
    for (int j = 0; j < ka.n; ++j) s->kmax = std::max(s->kmax, (int)ka.k[j]);
    s->pend_cap = pending_cap ? pending_cap : SK_DEFAULT_PENDING;
    RKCHK(s->state.reserve(32));
    RKCHK(s->h_state.reserve(64));
    HIPCHK(hipMemsetAsync(s->state.p, 0, 32, c->st));
    RKCHK(ensure_capacity(s, s->pend_cap, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    guard.s = nullptr;
    *out = s;
    return RK_OK;
}

extern "C" int rk_sample_reset(rk_sample* s) {
    RKCHK(check_sample(s));
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipMemsetAsync(s->state.p, 0, 32, s->ctx->st));
    HIPCHK(hipStreamSynchronize(s->ctx->st));
    s->n_res = 0; s->pending = 0; s->last_need = 0; s->seen_bases = 0; s->last_bases = 0; s->kept = 0; s->folds = 0; s->retries = 0;
    if (s->sketch_size) { s->max_hash = ~0ull; s->cuts = 0; s->weight = 0; }
    return RK_OK;
}

extern "C" int rk_sample_add_batch_device(rk_sample* s, const void* d_bases, const void* d_offsets_u32, int64_t nseq, void* hip_stream) {
    return sample_feed_device(s, d_bases, d_offsets_u32, nseq, 0, (hipStream_t)hip_stream);
}

extern "C" int rk_sample_add_batch(rk_sample* s, const uint8_t* bases, const uint64_t* offsets, int64_t nseq) {
    RKCHK(check_sample(s));
    if (!offsets || nseq < 0) return fail(RK_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < nseq; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(RK_ERR_ARG, "offsets decrease at sequence %lld", (long long)i);
        if (offsets[i + 1] - offsets[i] > 0x7fffffffull) return fail(RK_ERR_LIMIT, "sequence %lld holds 2^31 bases or more", (long long)i);
    }
    if (nseq > 0 && offsets[nseq] > offsets[0] && !bases) return fail(RK_ERR_ARG, "bad arguments");
    if (nseq == 0) return RK_OK;
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    std::vector<uint32_t> off32;
    for (int64_t i0 = 0; i0 < nseq;) { // pieces of whole sequences; a sequence longer than a piece is alone in its own
        int64_t i1 = i0 + 1;
        while (i1 < nseq && offsets[i1 + 1] - offsets[i0] <= SK_PIECE_BASES && i1 - i0 < ((int64_t)1 << 22)) ++i1;
        const uint64_t nb = offsets[i1] - offsets[i0];
        off32.resize((size_t)(i1 - i0) + 1);
        for (int64_t i = i0; i <= i1; ++i) off32[(size_t)(i - i0)] = (uint32_t)(offsets[i] - offsets[i0]);
        RKCHK(s->w_bases.reserve((size_t)nb + 64));
        RKCHK(s->w_offs.reserve(off32.size() * 4));
        if (nb) HIPCHK(hipMemcpyAsync(s->w_bases.p, bases + offsets[i0], (size_t)nb, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(s->w_offs.p, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, c->st));
        RKCHK(feed_locked(s, s->w_bases.p, s->w_offs.p, (uint32_t)(i1 - i0), nb, c->st)); // (synchronises: off32 may be refilled)
        i0 = i1;
    }
    return RK_OK;
}

extern "C" int rk_sample_add_sketch(rk_sample* s, const uint64_t* values, const uint32_t* abund, uint64_t n) {
    RKCHK(check_sample(s));
    if (s->sketch_size) return fail(RK_ERR_ARG, "a bottom sample takes reads, not sketches: uniting two of them needs the smaller of two thresholds");
    if (n && !values) return fail(RK_ERR_ARG, "bad arguments");
    if (s->with_abund && n && !abund) return fail(RK_ERR_ARG, "a sample with abundances takes a sketch with abundances");
    if (n > 0x7fffffffull) return fail(RK_ERR_LIMIT, "a sketch of 2^31 values or more");
    for (uint64_t i = 0; i < n; ++i) {
        if (values[i] == 0) return fail(RK_ERR_ARG, "value %llu of the sketch is 0", (unsigned long long)i);
        if (i && values[i] <= values[i - 1]) return fail(RK_ERR_ARG, "the sketch does not ascend at value %llu", (unsigned long long)i);
        if (abund && abund[i] == 0) return fail(RK_ERR_ARG, "abundance 0 at value %llu of the sketch", (unsigned long long)i);
    }
    const uint64_t m = (uint64_t)(std::upper_bound(values, values + n, s->max_hash) - values); // values above max_hash are cut off
    if (m == 0) return RK_OK;
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(fold_pending(s, c->st));
    RKCHK(ensure_capacity(s, s->n_res + std::max(m, s->pend_cap), c->st));
    HIPCHK(hipMemcpyAsync(s->keys[s->cur].as<uint64_t>() + s->n_res, values, (size_t)m * 8, hipMemcpyHostToDevice, c->st));
    if (s->with_abund) HIPCHK(hipMemcpyAsync(s->cnts[s->cur].as<uint32_t>() + s->n_res, abund, (size_t)m * 4, hipMemcpyHostToDevice, c->st));
    RKCHK(fold_values(s, m, false, c->st));
    uint64_t sum = m; // a sample without abundances counts a value of a sketch once, whatever abundances came with it
    if (abund && s->with_abund) { sum = 0; for (uint64_t i = 0; i < m; ++i) sum += abund[i]; }
    s->kept += sum;
    return RK_OK;
}

extern "C" int rk_sample_device(rk_sample* s, const void** d_values, const void** d_abund, uint64_t* n) {
    RKCHK(check_sample(s));
    if (!d_values || !n) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(fold_pending(s, s->ctx->st));
    *d_values = s->keys[s->cur].p;
    if (d_abund) *d_abund = s->with_abund ? s->cnts[s->cur].p : nullptr;
    *n = s->n_res;
    return RK_OK;
}

extern "C" int rk_sample_finish(rk_sample* s, uint64_t** values, uint32_t** abund, uint64_t* n) {
    RKCHK(check_sample(s));
    if (!values || !n || (s->with_abund && !abund)) return fail(RK_ERR_ARG, "bad arguments");
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(fold_pending(s, c->st));
    const uint64_t nd = s->n_res;
    uint64_t* v = (uint64_t*)malloc((size_t)std::max<uint64_t>(nd, 1) * 8);
    uint32_t* a = s->with_abund ? (uint32_t*)malloc((size_t)std::max<uint64_t>(nd, 1) * 4) : nullptr;
    if (!v || (s->with_abund && !a)) { free(v); free(a); return fail(RK_ERR_NOMEM, "malloc of %llu sample values", (unsigned long long)nd); }
    hipError_t e = hipSuccess;
    if (nd) e = hipMemcpyAsync(v, s->keys[s->cur].p, (size_t)nd * 8, hipMemcpyDeviceToHost, c->st);
    if (nd && a && e == hipSuccess) e = hipMemcpyAsync(a, s->cnts[s->cur].p, (size_t)nd * 4, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) { free(v); free(a); return fail(RK_ERR_HIP, "download of the sample failed: %s", hipGetErrorString(e)); }
    *values = v;
    if (abund) *abund = a;
    *n = nd;
    return RK_OK;
}

extern "C" int rk_sample_stats(rk_sample* s, rk_sample_stats_t* out) {
    RKCHK(check_sample(s));
    if (!out || out->struct_size < sizeof(uint32_t)) return fail(RK_ERR_ARG, "bad arguments");
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    uint64_t* h = s->h_state.as<uint64_t>();
    HIPCHK(hipMemcpyAsync(h, s->state.p, 24, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    rk_sample_stats_t t{};
    t.folds = s->folds; t.retries = s->retries;
    t.nseq = h[1]; t.nbases = h[2];
    t.kept = s->kept; t.distinct = s->n_res;
    const uint32_t size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof t);
    t.struct_size = size;
    memcpy(out, &t, size);
    return RK_OK;
}

// ---- bottom samples
extern "C" int rk_sample_create_bottom(rk_ctx* c, const int* ks, int nks, int sketch_size, uint64_t min_copies, uint64_t pending_cap, rk_sample** out) {
    if (!c || !out) return fail(RK_ERR_ARG, "bad arguments");
    if (sketch_size < 1 || sketch_size > RK_MAX_SKETCH) return fail(RK_ERR_ARG, "sketch size %d outside [1,%d]", sketch_size, RK_MAX_SKETCH);
    if (min_copies < 1 || min_copies > 0xffffffffull) return fail(RK_ERR_ARG, "min_copies %llu outside [1,2^32-1]", (unsigned long long)min_copies);
    rk_sample* s = nullptr;
    RKCHK(rk_sample_create(c, ks, nks, ~0ull, 1, pending_cap, &s));
    s->sketch_size = sketch_size;
    s->min_copies = (uint32_t)min_copies;
    const int rc = s->cut_state.reserve(32);
    if (rc != RK_OK) { rk_sample_destroy(s); return rc; }
    *out = s;
    return RK_OK;
}

extern "C" int rk_sample_finish_bottom(rk_sample* s, uint64_t* row, int32_t* len) {
    RKCHK(check_sample(s));
    if (!row || !len) return fail(RK_ERR_ARG, "bad arguments");
    if (!s->sketch_size) return fail(RK_ERR_ARG, "a scaled sample has no bottom-s row: rk_sample_finish gives its values");
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(fold_and_cut(s, c->st));
    const uint64_t nd = s->n_res;
    std::vector<uint64_t> v((size_t)nd);
    std::vector<uint32_t> a((size_t)nd);
    if (nd) {
        HIPCHK(hipMemcpyAsync(v.data(), s->keys[s->cur].p, (size_t)nd * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipMemcpyAsync(a.data(), s->cnts[s->cur].p, (size_t)nd * 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return rk_bottom_emit(v.data(), a.data(), nd, s->sketch_size, s->min_copies, c->dedup ? 1 : 0, row, len);
}

extern "C" int rk_sample_bottom_state(rk_sample* s, uint64_t* threshold, uint64_t* candidates, uint64_t* qualifying_weight, uint32_t* cuts) {
    RKCHK(check_sample(s));
    if (!s->sketch_size) return fail(RK_ERR_ARG, "a scaled sample has no bottom state");
    std::lock_guard<std::mutex> lk(s->mu);
    if (threshold) *threshold = s->max_hash;
    if (candidates) *candidates = s->n_res;
    if (qualifying_weight) *qualifying_weight = s->weight;
    if (cuts) *cuts = s->cuts;
    return RK_OK;
}
