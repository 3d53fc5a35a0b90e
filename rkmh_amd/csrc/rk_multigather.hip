// rk_multigather.hip -- multigather (include/rkmh_amd.h, "MULTIGATHER"): the greedy decomposition of rk_gather.hip for a whole batch
// of queries at once, through the resident inverted index of rk_search.hip.  The candidates of every query come from one search at
// threshold min_shared; their counts are kept up to date incrementally -- a value that leaves a query takes 1 from the count of every
// candidate its posting list names -- so nothing is recounted, and a round is two launches for the whole batch (k_mg_pick,
// k_mg_remove) whatever the number of queries.  The host-only form is rk_multigather_scaled_host (rk_scaled_host.cpp); semantics,
// bounds and measurements: DESIGN.md section 18.
#include "rk_sets.hpp"

namespace {

constexpr int MG_T = 256;                 // threads of a workgroup of every kernel here but the scan
constexpr int MG_WAVES = MG_T / 64;
constexpr uint32_t MG_MISS = 0xffffffffu; // the key position of a query value that no reference holds
constexpr uint32_t MG_MAX_SLICES = 64;    // workgroups that share one query's values in k_mg_remove, at most
constexpr uint64_t MG_MAX_CAND = 0x7fffffffull; // candidates of one call: their positions are 32-bit

// per query, what the rounds hand to each other (16 bytes; the rows written so far are t[q], an array of its own that the last scan reads)
struct MgQuery {
    int32_t finished;   // the best count fell below min_shared, or every row there is room for is written: no launch touches the query again
    int32_t pick_ref;   // the reference picked in round pick_round
    int32_t pick_round; // the round whose k_mg_pick wrote pick_ref: k_mg_remove of another round leaves the query alone
    int32_t remaining;  // values of the query not yet explained
};
// per call (16 bytes, downloaded after the setup and after every group of rounds)
struct MgControl {
    uint32_t finished;  // queries with finished = 1
    uint32_t max_rcap;  // the largest row capacity of a query: no more rounds than that can write anything
    uint32_t longest;   // the most values of a query that has a candidate: sizes the grid of k_mg_remove
    uint32_t pad;
};

// the candidates of query q: positions [c0, c1) of the hit array, from the scan the search left behind (pre[q * nblk]: hits before
// query q's), clamped to the ncand hits there are
__device__ __forceinline__ void candidate_range(const uint64_t* __restrict__ pre, uint32_t q, uint32_t nblk, uint64_t ncand, uint32_t& c0, uint32_t& c1) {
    const uint64_t a = min(pre[(uint64_t)q * nblk], ncand);
    c0 = (uint32_t)a;
    c1 = (uint32_t)max(min(pre[((uint64_t)q + 1) * nblk], ncand), a);
}

// Setup, grid-stride.  Per candidate c: its reference and its count (= total, the hit's shared) out of the hit triples.  Per query:
// the row capacity min(max_rounds, its candidates), t = 0, its state; a query without a candidate is finished from the start.
__global__ __launch_bounds__(MG_T) void k_mg_init(const int32_t* __restrict__ hits, uint64_t ncand, const uint64_t* __restrict__ pre, uint32_t nblk,
                                                  const uint64_t* __restrict__ qoff, uint32_t nq, uint64_t q_nvalues, uint32_t max_rounds,
                                                  uint32_t* __restrict__ cand_ref, int32_t* __restrict__ count, uint32_t* __restrict__ t,
                                                  uint32_t* __restrict__ rcap, MgQuery* __restrict__ mq, MgControl* __restrict__ ctl) {
    const uint64_t step = (uint64_t)gridDim.x * MG_T, first = (uint64_t)blockIdx.x * MG_T + threadIdx.x;
    for (uint64_t c = first; c < ncand; c += step) {
        cand_ref[c] = (uint32_t)hits[c * 3 + 1];
        count[c] = hits[c * 3 + 2];
    }
    for (uint64_t q = first; q < nq; q += step) {
        uint32_t c0, c1;
        candidate_range(pre, (uint32_t)q, nblk, ncand, c0, c1);
        uint64_t q0, q1;
        clamped_row(qoff, q, q_nvalues, q0, q1);
        const uint32_t cap = min(max_rounds, c1 - c0);
        t[q] = 0;
        rcap[q] = cap;
        MgQuery s;
        s.finished = cap == 0; s.pick_ref = -1; s.pick_round = -1; s.remaining = (int32_t)(q1 - q0);
        mq[q] = s;
        if (cap == 0) atomicAdd(&ctl->finished, 1u);
        else { atomicMax(&ctl->max_rcap, cap); atomicMax(&ctl->longest, (uint32_t)(q1 - q0)); }
    }
}

// Once per value position of the query batch: where the value stands in keys, or MG_MISS; a value that no reference holds can never
// leave its query through a pick, so its alive byte starts at 0 and no round looks at it again (remaining is arithmetic, not a count
// of bytes).  No round repeats a key search.
__global__ __launch_bounds__(MG_T) void k_mg_keypos(const uint64_t* __restrict__ keys, uint32_t nkeys, const uint64_t* __restrict__ qv, uint64_t q_nvalues,
                                                    uint32_t* __restrict__ keypos, uint8_t* __restrict__ alive) {
    const uint64_t step = (uint64_t)gridDim.x * MG_T;
    for (uint64_t i = (uint64_t)blockIdx.x * MG_T + threadIdx.x; i < q_nvalues; i += step) {
        const uint64_t x = qv[i];
        const uint32_t lo = first_not_below(keys, 0u, nkeys, x);
        const bool found = lo < nkeys && keys[lo] == x;
        keypos[i] = found ? lo : MG_MISS;
        alive[i] = found ? 1 : 0;
    }
}

// One workgroup per query.  The pick is the maximum of (count << 32 | ~local candidate) over the query's candidates -- k_gather_pick's
// reduction: the largest count, and among equal counts the lowest candidate position, which is the lowest reference because a query's
// candidates ascend by reference.  A maximum does not depend on the order it is reduced in.  Writes row t[q] into the query's row
// range and the pick into its state, or finishes the query; a finished query returns at once and is never written again.
__global__ __launch_bounds__(MG_T) void k_mg_pick(int32_t round, uint32_t nq, int32_t min_shared, const uint64_t* __restrict__ pre, uint32_t nblk,
                                                  uint64_t ncand, const uint32_t* __restrict__ cand_ref, const int32_t* __restrict__ count,
                                                  const int32_t* __restrict__ hits, uint32_t nref, uint32_t* __restrict__ t, const uint32_t* __restrict__ rcap,
                                                  MgQuery* __restrict__ mq, const uint64_t* __restrict__ row_base, int32_t* __restrict__ rows,
                                                  uint64_t rows_cap, MgControl* __restrict__ ctl) {
    __shared__ uint64_t wbest[MG_WAVES];
    const uint32_t q = blockIdx.x;
    if (q >= nq) return;
    if (mq[q].finished) return; // (uniform: the state is written after the barrier below only)
    uint32_t c0, c1;
    candidate_range(pre, q, nblk, ncand, c0, c1);
    const uint32_t n_c = c1 - c0;
    uint64_t best = 0;
    for (uint32_t i = threadIdx.x; i < n_c; i += MG_T) {
        const int32_t n = count[c0 + i];
        best = max(best, ((uint64_t)(uint32_t)(n > 0 ? n : 0) << 32) | (uint64_t)(uint32_t)~i);
    }
    for (int d = 32; d > 0; d >>= 1) best = max(best, shfl_xor_u64(best, d));
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < MG_WAVES; ++w) best = max(best, wbest[w]);
    const int32_t n = (int32_t)(best >> 32);
    const uint32_t i = ~(uint32_t)best;
    const uint32_t row = t[q], cap = rcap[q];
    uint32_t r = nref;
    if (i < n_c) r = cand_ref[c0 + i];
    if (n < min_shared || n < 1 || i >= n_c || r >= nref || row >= cap) {
        mq[q].finished = 1;
        atomicAdd(&ctl->finished, 1u);
        return;
    }
    const int32_t left = mq[q].remaining - n;
    const uint64_t at = row_base[q] + row;
    if (at < rows_cap) {
        int32_t* o = rows + at * 4;
        o[0] = (int32_t)r; o[1] = n; o[2] = hits[(uint64_t)(c0 + i) * 3 + 2]; o[3] = left;
    }
    t[q] = row + 1;
    MgQuery s;
    s.finished = row + 1 >= cap; s.pick_ref = (int32_t)r; s.pick_round = round; s.remaining = left;
    mq[q] = s;
    if (s.finished) atomicAdd(&ctl->finished, 1u);
}

// one reference less holds an alive value of this query: 1 off its count, when it is a candidate (its place: a search in the query's
// candidate range, which ascends by reference).  The id 2^32 - 1 of a position no row covers, like every id at or beyond nref, falls out.
__device__ __forceinline__ void one_less(uint32_t r, uint32_t nref, const uint32_t* __restrict__ cand_ref, uint32_t c0, uint32_t c1, int32_t* count) {
    if (r >= nref) return;
    const uint32_t at = first_not_below(cand_ref, c0, c1, r);
    if (at < c1 && cand_ref[at] == r) atomicSub(&count[at], 1);
}

// The values of this round's picks leave their queries.  `slices` workgroups per query (workgroup w: query w / slices) stride the
// query's values, 64 per wave at a time.  A lane whose value is alive looks the pick up in the value's posting list -- the lists
// ascend: a search from the stored key position -- and on a match that same lane, the only one that owns the value, clears its byte,
// takes its abundance (W) and walks the list: 1 off the count of every candidate of this query it names.  A list of 64 entries or
// more is walked by the whole wave, as k_search_block walks it.  The count updates are integer atomics on global memory: integer adds
// commute, so the counts after the launch -- all the next k_mg_pick reads -- do not depend on the order of arrival.  W: the wave adds
// its lanes' abundances with shuffles and its first lane adds the sum to wunique of the row k_mg_pick has just written.
template <bool W>
__global__ __launch_bounds__(MG_T) void k_mg_remove(int32_t round, uint32_t nq, uint32_t slices, const uint64_t* __restrict__ qoff, uint64_t q_nvalues,
                                                    const uint32_t* __restrict__ q_abund, uint32_t nkeys, const uint64_t* __restrict__ post_off,
                                                    const uint32_t* __restrict__ post, uint64_t npost, uint32_t nref, const uint64_t* __restrict__ pre,
                                                    uint32_t nblk, uint64_t ncand, const uint32_t* __restrict__ cand_ref, int32_t* count,
                                                    const uint32_t* __restrict__ t, const MgQuery* __restrict__ mq, const uint32_t* __restrict__ keypos,
                                                    uint8_t* alive, const uint64_t* __restrict__ row_base, unsigned long long* wunique, uint64_t rows_cap) {
    const uint32_t q = blockIdx.x / slices, slice = blockIdx.x % slices;
    if (q >= nq) return;
    const MgQuery s = mq[q]; // (no launch of this kernel writes the state: uniform over the query's workgroups)
    if (s.pick_round != round || s.pick_ref < 0 || (uint32_t)s.pick_ref >= nref) return;
    const uint32_t pick = (uint32_t)s.pick_ref;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c0, c1;
    candidate_range(pre, q, nblk, ncand, c0, c1);
    uint64_t q0, q1;
    clamped_row(qoff, q, q_nvalues, q0, q1);
    unsigned long long sum = 0;
    for (uint64_t t0 = q0 + ((uint64_t)slice * MG_WAVES + wave) * 64; t0 < q1; t0 += (uint64_t)slices * MG_T) { // wave-uniform: every lane takes part in the ballot
        const uint64_t i = t0 + lane;
        uint64_t p0 = 0, p1 = 0; // the posting list of this lane's value, when the pick holds it
        if (i < q1 && alive[i]) {
            const uint32_t kp = keypos[i];
            if (kp < nkeys) {
                const uint64_t a = min(post_off[kp], npost), e = max(min(post_off[kp + 1], npost), a);
                const uint64_t at = first_not_below(post, a, e, pick);
                if (at < e && post[at] == pick) {
                    p0 = a; p1 = e;
                    alive[i] = 0;
                    if (W) sum += q_abund[i];
                }
            }
        }
        const bool wide = p1 - p0 >= 64;
        if (!wide)
            for (uint64_t j = p0; j < p1; ++j) one_less(post[j], nref, cand_ref, c0, c1, count);
        uint64_t todo = __ballot(wide);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t s0 = shfl_u64(p0, src), s1 = shfl_u64(p1, src);
            for (uint64_t j = s0 + lane; j < s1; j += 64) one_less(post[j], nref, cand_ref, c0, c1, count);
        }
    }
    if (W) {
        for (int d = 32; d > 0; d >>= 1) sum += shfl_xor_u64(sum, d);
        const uint32_t row = t[q] - 1; // the row of this round's pick (t >= 1: the pick wrote it)
        const uint64_t at = row_base[q] + row;
        if (lane == 0 && sum != 0 && t[q] >= 1 && at < rows_cap) atomicAdd(wunique + at, sum);
    }
}

// One wave per query, grid-stride: its t[q] rows (and their wunique) from its row range to where the compact answer has them,
// row_offsets[q] on, as far as cap_rows.
__global__ __launch_bounds__(MG_T) void k_mg_pack(uint32_t nq, const uint32_t* __restrict__ t, const uint32_t* __restrict__ rcap,
                                                  const uint64_t* __restrict__ row_base, const int32_t* __restrict__ rows,
                                                  const unsigned long long* __restrict__ wu, uint64_t rows_cap, const uint64_t* __restrict__ row_offsets,
                                                  int32_t* __restrict__ out4, unsigned long long* __restrict__ out_w, uint64_t cap_rows) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * MG_WAVES;
    for (uint64_t q = (uint64_t)blockIdx.x * MG_WAVES + (threadIdx.x >> 6); q < nq; q += nwaves) {
        const uint32_t n = min(t[q], rcap[q]);
        const uint64_t src = row_base[q], dst = row_offsets[q];
        for (uint32_t i = lane; i < n; i += 64) {
            const uint64_t a = src + i, b = dst + i;
            if (a >= rows_cap || b >= cap_rows) continue;
            for (int k = 0; k < 4; ++k) out4[b * 4 + k] = rows[a * 4 + k];
            if (out_w) out_w[b] = wu[a];
        }
    }
}

// the state of one call, carved out of ix->w_mg (every part 256-byte aligned)
struct MgWork {
    int32_t* hits = nullptr; uint32_t* cand_ref = nullptr; int32_t* count = nullptr; uint32_t* keypos = nullptr; uint8_t* alive = nullptr;
    uint32_t* t = nullptr; uint32_t* rcap = nullptr; uint64_t* row_base = nullptr; MgQuery* mq = nullptr; MgControl* ctl = nullptr;
    int32_t* rows = nullptr; unsigned long long* wu = nullptr;
    uint64_t ncand = 0, rows_cap = 0;
};
struct Carver {
    char* base = nullptr;
    size_t at = 0;
    template <typename T> T* take(size_t n) { T* p = base ? (T*)(base + at) : nullptr; at += (n * sizeof(T) + 255) & ~(size_t)255; return p; }
};
void carve(Carver& cv, MgWork& w, uint64_t ncand, uint64_t nq, uint64_t q_nvalues, uint64_t rows_cap) {
    w.hits = cv.take<int32_t>(ncand * 3); w.cand_ref = cv.take<uint32_t>(ncand); w.count = cv.take<int32_t>(ncand);
    w.keypos = cv.take<uint32_t>(q_nvalues); w.alive = cv.take<uint8_t>(q_nvalues);
    w.t = cv.take<uint32_t>(nq + 1); w.rcap = cv.take<uint32_t>(nq + 1); w.row_base = cv.take<uint64_t>(nq + 1);
    w.mq = cv.take<MgQuery>(nq); w.ctl = cv.take<MgControl>(1);
    w.rows = cv.take<int32_t>(rows_cap * 4); w.wu = cv.take<unsigned long long>(rows_cap);
}

inline uint32_t flat_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + MG_T - 1) / MG_T, 1), 1u << 16); }

// Everything up to the compact row offsets, on resident arrays, on stream st; the caller holds ix->mu.  d_row_offsets (nq + 1 uint64,
// all of them written) and *total, the number of rows, are the answer's shape; the rows themselves stay in w for mg_pack.
// Synchronises st.
int mg_rounds(rk_scaled_index* ix, const uint64_t* d_qv, const uint32_t* d_qa, const uint64_t* d_qo, uint32_t nq, uint64_t q_nvalues, int min_shared,
              int max_rounds, uint32_t nblk, uint32_t nwg, hipStream_t st, uint64_t* d_row_offsets, MgWork& w, uint64_t* total) {
    *total = 0;
    uint64_t ncand = 0;
    RKCHK(search_count(ix, d_qv, d_qo, nq, q_nvalues, min_shared, nullptr, nblk, nwg, st, &ncand, "multigather"));
    if (ncand > MG_MAX_CAND)
        return fail(RK_ERR_LIMIT, "multigather: %llu candidates (pairs that share at least min_shared values) are more than 2^31-1: send fewer queries per call",
                    (unsigned long long)ncand);
    if (ncand == 0) { // no query has a candidate: no row
        HIPCHK(hipMemsetAsync(d_row_offsets, 0, ((size_t)nq + 1) * 8, st));
        HIPCHK(hipStreamSynchronize(st));
        return RK_OK;
    }
    const uint64_t rows_cap = std::min<uint64_t>(ncand, (uint64_t)nq * (uint64_t)max_rounds); // a query writes min(max_rounds, its candidates) rows at most
    Carver size;
    MgWork none;
    carve(size, none, ncand, nq, q_nvalues, rows_cap);
    RKCHK(ix->w_mg.reserve(size.at));
    Carver cv;
    cv.base = ix->w_mg.as<char>();
    carve(cv, w, ncand, nq, q_nvalues, rows_cap);
    w.ncand = ncand; w.rows_cap = rows_cap;
    const uint64_t* pre = ix->w_pre.as<uint64_t>();
    // 1. the candidates: the hits of the search in (query, reference) order; their references and counts; the state of every query
    RKCHK(search_emit(ix, d_qv, d_qo, nq, q_nvalues, min_shared, nullptr, nblk, nwg, st, w.hits, ncand));
    HIPCHK(hipMemsetAsync(w.ctl, 0, sizeof(MgControl), st));
    if (d_qa) HIPCHK(hipMemsetAsync(w.wu, 0, (size_t)rows_cap * 8, st));
    hipLaunchKernelGGL(k_mg_init, dim3(flat_grid(std::max<uint64_t>(ncand, nq))), dim3(MG_T), 0, st, w.hits, ncand, pre, nblk, d_qo, nq, q_nvalues,
                       (uint32_t)max_rounds, w.cand_ref, w.count, w.t, w.rcap, w.mq, w.ctl);
    hipLaunchKernelGGL(k_scan_blocks<uint32_t>, dim3(1), dim3(1024), 0, st, w.rcap, (uint64_t)nq, w.row_base);
    // 2. where every query value stands in the index
    if (q_nvalues)
        hipLaunchKernelGGL(k_mg_keypos, dim3(flat_grid(q_nvalues)), dim3(MG_T), 0, st, ix->keys.as<uint64_t>(), (uint32_t)ix->nkeys, d_qv, q_nvalues, w.keypos, w.alive);
    HIPCHK(hipGetLastError());
    MgControl ctl{};
    HIPCHK(hipMemcpyAsync(&ctl, w.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (ctl.finished > nq || ctl.max_rcap > (uint32_t)max_rounds) return fail(RK_ERR_HIP, "multigather: %u of %u queries finished, row capacity %u of %d", ctl.finished, nq, ctl.max_rcap, max_rounds);
    // 3. rounds, in groups of RK_GATHER_BATCH: a query writes a row or finishes in every round, so max_rcap rounds are all there can be
    // workgroups per query in k_mg_remove: eight values per lane of the longest query, at most MG_MAX_SLICES, at most 2^22 workgroups in all
    const uint32_t slices = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(((uint64_t)ctl.longest + MG_T * 8 - 1) / (MG_T * 8), MG_MAX_SLICES), (1u << 22) / nq));
    const dim3 remove_grid(nq * slices); // nq < 2^24 (the search's workgroup limit), slices <= 2^22 / nq: below 2^31
    for (uint32_t launched = 0; launched < ctl.max_rcap && ctl.finished < nq;) {
        const uint32_t group = std::min<uint32_t>(RK_GATHER_BATCH, ctl.max_rcap - launched);
        for (uint32_t i = 0; i < group; ++i) {
            const int32_t round = (int32_t)(launched + i);
            hipLaunchKernelGGL(k_mg_pick, dim3(nq), dim3(MG_T), 0, st, round, nq, (int32_t)min_shared, pre, nblk, ncand, w.cand_ref, w.count, w.hits, ix->nref,
                               w.t, w.rcap, w.mq, w.row_base, w.rows, rows_cap, w.ctl);
            if (d_qa)
                hipLaunchKernelGGL(k_mg_remove<true>, remove_grid, dim3(MG_T), 0, st, round, nq, slices, d_qo, q_nvalues, d_qa, (uint32_t)ix->nkeys,
                                   ix->post_off.as<uint64_t>(), ix->post.as<uint32_t>(), ix->npost, ix->nref, pre, nblk, ncand, w.cand_ref, w.count, w.t, w.mq,
                                   w.keypos, w.alive, w.row_base, w.wu, rows_cap);
            else
                hipLaunchKernelGGL(k_mg_remove<false>, remove_grid, dim3(MG_T), 0, st, round, nq, slices, d_qo, q_nvalues, (const uint32_t*)nullptr,
                                   (uint32_t)ix->nkeys, ix->post_off.as<uint64_t>(), ix->post.as<uint32_t>(), ix->npost, ix->nref, pre, nblk, ncand, w.cand_ref,
                                   w.count, w.t, w.mq, w.keypos, w.alive, w.row_base, (unsigned long long*)nullptr, rows_cap);
        }
        HIPCHK(hipGetLastError());
        launched += group;
        HIPCHK(hipMemcpyAsync(&ctl, w.ctl, sizeof ctl, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (ctl.finished > nq) return fail(RK_ERR_HIP, "multigather: %u of %u queries finished", ctl.finished, nq);
    }
    // 4. the compact answer's shape: row_offsets = the scan of the rows written per query
    hipLaunchKernelGGL(k_scan_blocks<uint32_t>, dim3(1), dim3(1024), 0, st, w.t, (uint64_t)nq, d_row_offsets);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(total, d_row_offsets + nq, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (*total > rows_cap) return fail(RK_ERR_HIP, "multigather: %llu rows written of at most %llu", (unsigned long long)*total, (unsigned long long)rows_cap);
    return RK_OK;
}

// the rows (and wunique, when d_out_w is given) in query order into the caller's arrays, as far as cap_rows; asynchronous on st
int mg_pack(const MgWork& w, uint32_t nq, const uint64_t* d_row_offsets, int32_t* d_out4, uint64_t* d_out_w, uint64_t cap_rows, hipStream_t st) {
    hipLaunchKernelGGL(k_mg_pack, dim3(wave_grid(nq, MG_WAVES)), dim3(MG_T), 0, st, nq, w.t, w.rcap, w.row_base, w.rows, w.wu, w.rows_cap, d_row_offsets, d_out4,
                       (unsigned long long*)d_out_w, cap_rows);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

int check_multigather_shape(const rk_ctx* c, const rk_scaled_index* ix, int64_t nq, int min_shared, int max_rounds, uint64_t* nwg, uint32_t* nblk) {
    RKCHK(check_search_shape(c, ix, nq, min_shared, nwg, nblk, "multigather"));
    if (max_rounds < 1) return fail(RK_ERR_ARG, "multigather: max_rounds %d is below 1", max_rounds);
    return RK_OK;
}

} // namespace

extern "C" int rk_multigather_scaled_device(rk_ctx* c, rk_scaled_index* ix, const void* d_q_values, const void* d_q_abund, const void* d_q_offsets, int64_t nq,
                                            uint64_t q_nvalues, int min_shared, int max_rounds, void* d_out4, void* d_wunique, uint64_t cap_rows,
                                            void* d_row_offsets, uint64_t* nrows, void* hip_stream) {
    if (!c || !ix || !d_q_offsets || !d_row_offsets || !nrows || (!d_q_values && q_nvalues) || (!d_out4 && cap_rows) || (d_q_abund && !d_wunique && cap_rows))
        return fail(RK_ERR_ARG, "bad arguments");
    uint64_t nwg = 0, total = 0;
    uint32_t nblk = 0;
    RKCHK(check_multigather_shape(c, ix, nq, min_shared, max_rounds, &nwg, &nblk));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    hipStream_t st = (hipStream_t)hip_stream;
    MgWork w;
    RKCHK(mg_rounds(ix, (const uint64_t*)d_q_values, (const uint32_t*)d_q_abund, (const uint64_t*)d_q_offsets, (uint32_t)nq, q_nvalues, min_shared, max_rounds, nblk,
                    (uint32_t)nwg, st, (uint64_t*)d_row_offsets, w, &total));
    if (total && cap_rows) {
        RKCHK(mg_pack(w, (uint32_t)nq, (const uint64_t*)d_row_offsets, (int32_t*)d_out4, d_q_abund ? (uint64_t*)d_wunique : nullptr, cap_rows, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    *nrows = total;
    return RK_OK;
}

extern "C" int rk_multigather_scaled(rk_ctx* c, rk_scaled_index* ix, const uint64_t* q_values, const uint32_t* q_abund, const uint64_t* q_offsets, int64_t nq,
                                     int min_shared, int max_rounds, int32_t** rows4, uint64_t** wunique, uint64_t* row_offsets, uint64_t* nrows) {
    if (!c || !ix || !q_offsets || !rows4 || !row_offsets || !nrows || (q_abund && !wunique)) return fail(RK_ERR_ARG, "bad arguments");
    uint64_t nwg = 0, total = 0;
    uint32_t nblk = 0;
    RKCHK(check_multigather_shape(c, ix, nq, min_shared, max_rounds, &nwg, &nblk));
    RKCHK(check_csr(q_offsets, nq, "multigather: ", "the queries", RK_ERR_ARG));
    const uint64_t qn = q_offsets[nq] - q_offsets[0];
    if (qn && !q_values) return fail(RK_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < nq; ++i)
        for (uint64_t t = q_offsets[i]; t < q_offsets[i + 1]; ++t)
            if (q_values[t] == 0 || (t > q_offsets[i] && q_values[t] <= q_values[t - 1]))
                return fail(RK_ERR_ARG, "multigather: query %lld is not ascending, distinct and non-zero at value %llu", (long long)i, (unsigned long long)(t - q_offsets[i]));
    if (q_abund) RKCHK(check_abund(q_abund, q_offsets[0], q_offsets[nq], "multigather: ", "the queries"));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    RKCHK(ix->w_qv.reserve((size_t)qn * 8 + 8));
    RKCHK(ix->w_qo.reserve(((size_t)nq + 1) * 8));
    // the host entry's own: the row offsets, then the query's abundances; the packed answer follows once its size is known
    const size_t off_bytes = (((size_t)nq + 1) * 8 + 255) & ~(size_t)255, ab_bytes = q_abund ? ((size_t)qn * 4 + 255) & ~(size_t)255 : 0;
    RKCHK(ix->w_mg_io.reserve(off_bytes + ab_bytes + 256));
    uint64_t* d_ro = ix->w_mg_io.as<uint64_t>();
    uint32_t* d_qa = q_abund ? (uint32_t*)(ix->w_mg_io.as<char>() + off_bytes) : nullptr;
    std::vector<uint64_t> off;
    RKCHK(upload_csr(q_values, q_offsets, nq, ix->w_qv.as<uint64_t>(), ix->w_qo.as<uint64_t>(), off, c->st));
    if (q_abund && qn) HIPCHK(hipMemcpyAsync(d_qa, q_abund + q_offsets[0], (size_t)qn * 4, hipMemcpyHostToDevice, c->st));
    MgWork w;
    RKCHK(mg_rounds(ix, ix->w_qv.as<uint64_t>(), d_qa, ix->w_qo.as<uint64_t>(), (uint32_t)nq, qn, min_shared, max_rounds, nblk, (uint32_t)nwg, c->st, d_ro, w,
                    &total)); // (synchronises: off lives until there)
    int32_t* out = (int32_t*)malloc(16 * (size_t)std::max<uint64_t>(total, 1));
    uint64_t* out_w = q_abund ? (uint64_t*)malloc(8 * (size_t)std::max<uint64_t>(total, 1)) : nullptr;
    int r = !out || (q_abund && !out_w) ? fail(RK_ERR_NOMEM, "malloc of %llu rows", (unsigned long long)total) : RK_OK;
    if (r == RK_OK && total) {
        r = ix->w_mg_out.reserve((size_t)total * 24); // the packed rows, then their wunique
        int32_t* d_out = ix->w_mg_out.as<int32_t>();
        uint64_t* d_w = q_abund ? (uint64_t*)(ix->w_mg_out.as<char>() + (size_t)total * 16) : nullptr;
        if (r == RK_OK) r = mg_pack(w, (uint32_t)nq, d_ro, d_out, d_w, total, c->st);
        if (r == RK_OK) {
            hipError_t e = hipMemcpyAsync(out, d_out, (size_t)total * 16, hipMemcpyDeviceToHost, c->st);
            if (e == hipSuccess && d_w) e = hipMemcpyAsync(out_w, d_w, (size_t)total * 8, hipMemcpyDeviceToHost, c->st);
            if (e != hipSuccess) r = fail(RK_ERR_HIP, "multigather: downloading %llu rows failed: %s", (unsigned long long)total, hipGetErrorString(e));
        }
    }
    if (r == RK_OK) {
        hipError_t e = hipMemcpyAsync(row_offsets, d_ro, ((size_t)nq + 1) * 8, hipMemcpyDeviceToHost, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) r = fail(RK_ERR_HIP, "multigather: downloading the row offsets failed: %s", hipGetErrorString(e));
    } else {
        hipError_t e = hipStreamSynchronize(c->st); (void)e; // (nothing of this call is in flight when the next one takes the buffers)
    }
    if (r != RK_OK) { free(out); free(out_w); return r; }
    *rows4 = out;
    if (q_abund) *wunique = out_w;
    *nrows = total;
    return RK_OK;
}
