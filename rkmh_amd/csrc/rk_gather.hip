// rk_gather.hip -- gather (include/rkmh_amd.h, "GATHER"): the greedy decomposition of one scaled sketch Q into reference sketches.
// Round after round the reference that shares most with what is left of Q is written out and its values leave Q.  The state stays on
// the device across rounds: one byte per query value (alive), and per candidate reference the list of the query indices it holds.
// The host-only form of the same loop is rk_gather_scaled_host (rk_scaled_host.cpp); semantics, bounds and measurements: DESIGN.md
// section 12.  With the query's abundances every row also gets the weight it explains (k_gather_remove_w; section 13).
#include "rk_sets.hpp"

namespace {

constexpr int GATHER_T = 256;                 // threads of a workgroup of the probe, compact, count and remove kernels
constexpr int GATHER_WAVES = GATHER_T / 64;
constexpr int PICK_T = 1024;                  // the one workgroup of k_gather_pick
constexpr uint32_t MISS = 0xffffffffu;        // a reference value that Q does not hold

// what the rounds hand to each other (device memory, 32 bytes; downloaded after every group of rounds)
struct GatherState {
    int32_t t;          // rows written so far
    int32_t done;       // the best count fell below min_shared: no round does anything any more
    int32_t pick;       // the candidate picked by this round's k_gather_pick, -1: none
    int32_t remaining;  // |alive|
    int32_t pad[4];
};

// One wave per reference, grid-stride.  Lanes stride the row; each looks its value up in Q (first element not below it: at most 32
// halvings, nq < 2^31) and writes the query index, or MISS, into hit[], which lies parallel to the reference values.  The hits of a
// row are counted with ballots; the first lane stores total[r].
__global__ __launch_bounds__(GATHER_T) void k_gather_probe(const uint64_t* __restrict__ q, uint32_t nq, const uint64_t* __restrict__ rv,
                                                           const uint64_t* __restrict__ roff, uint32_t nref, uint64_t nvalues,
                                                           uint32_t* __restrict__ hit, int32_t* __restrict__ total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * GATHER_WAVES;
    for (uint64_t r = (uint64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6); r < nref; r += nwaves) { // wave-uniform
        uint64_t r0, r1;
        clamped_row(roff, (uint32_t)r, nvalues, r0, r1);
        uint32_t cnt = 0;
        for (uint64_t t0 = r0; t0 < r1; t0 += 64) {
            const uint64_t t = t0 + lane;
            bool found = false;
            if (t < r1) {
                const uint64_t x = rv[t];
                const uint32_t lo = first_not_below(q, 0u, nq, x);
                found = lo < nq && q[lo] == x;
                hit[t] = found ? lo : MISS;
            }
            cnt += (uint32_t)__popcll(__ballot(found));
        }
        if (lane == 0) total[r] = (int32_t)cnt;
    }
}

// One wave per candidate, grid-stride: the hits of its row, in row order, to list[coff[c] ...).  Positions come from ballots (as in
// k_keep_scatter); a write lands below coff[c + 1] and below nlist only.
__global__ __launch_bounds__(GATHER_T) void k_gather_compact(const uint64_t* __restrict__ roff, uint32_t nref, uint64_t nvalues,
                                                             const uint32_t* __restrict__ hit, const int32_t* __restrict__ cand,
                                                             const uint64_t* __restrict__ coff, uint32_t ncand, uint64_t nlist,
                                                             uint32_t* __restrict__ list) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * GATHER_WAVES;
    for (uint64_t c = (uint64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6); c < ncand; c += nwaves) {
        const uint32_t r = (uint32_t)cand[c];
        if (r >= nref) continue;
        uint64_t r0, r1;
        clamped_row(roff, r, nvalues, r0, r1);
        const uint64_t end = min(coff[c + 1], nlist);
        uint64_t at = min(coff[c], end);
        for (uint64_t t0 = r0; t0 < r1; t0 += 64) {
            const uint64_t t = t0 + lane;
            const uint32_t h = t < r1 ? hit[t] : MISS;
            const uint64_t bal = __ballot(h != MISS);
            const uint64_t mine = at + lanes_below(bal);
            if (h != MISS && mine < end) list[mine] = h;
            at += (uint64_t)__popcll(bal);
        }
    }
}

// One wave per candidate, grid-stride: count[c] = how many of its hits are still alive.
__global__ __launch_bounds__(GATHER_T) void k_gather_count(const GatherState* __restrict__ state, int32_t max_rounds, const uint8_t* __restrict__ alive,
                                                           uint32_t nq, const uint64_t* __restrict__ coff, uint32_t ncand, uint64_t nlist,
                                                           const uint32_t* __restrict__ list, int32_t* __restrict__ count) {
    if (state->done || state->t >= max_rounds) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * GATHER_WAVES;
    for (uint64_t c = (uint64_t)blockIdx.x * GATHER_WAVES + (threadIdx.x >> 6); c < ncand; c += nwaves) {
        const uint64_t end = min(coff[c + 1], nlist), begin = min(coff[c], end);
        int32_t cnt = 0;
        for (uint64_t i = begin + lane; i < end; i += 64) {
            const uint32_t h = list[i];
            if (h < nq) cnt += alive[h];
        }
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if (lane == 0) count[c] = cnt;
    }
}

// One workgroup.  The pick is the maximum of (count << 32 | ~c) over the candidates: the largest count, and among equal counts the
// lowest candidate index -- candidates are listed by ascending reference index, so that is the lowest reference.  A maximum does not
// depend on the order it is reduced in.  Writes row t and the pick into the state, or sets done.
__global__ __launch_bounds__(PICK_T) void k_gather_pick(GatherState* __restrict__ state, int32_t max_rounds, int32_t min_shared,
                                                        const int32_t* __restrict__ count, const int32_t* __restrict__ cand, uint32_t ncand,
                                                        const int32_t* __restrict__ total, uint32_t nref, int32_t* __restrict__ out4) {
    __shared__ uint64_t wbest[PICK_T / 64];
    if (state->done || state->t >= max_rounds) { // (uniform: nothing has been written to the state in this launch)
        if (threadIdx.x == 0) state->pick = -1;
        return;
    }
    uint64_t best = 0;
    for (uint32_t c = threadIdx.x; c < ncand; c += PICK_T) {
        const int32_t n = count[c];
        const uint64_t key = ((uint64_t)(uint32_t)(n > 0 ? n : 0) << 32) | (uint64_t)(uint32_t)~c;
        best = max(best, key);
    }
    for (int d = 32; d > 0; d >>= 1) best = max(best, (uint64_t)__shfl_xor((unsigned long long)best, d, 64));
    if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < PICK_T / 64; ++w) best = max(best, wbest[w]);
    const int32_t n = (int32_t)(best >> 32);
    const uint32_t c = ~(uint32_t)best;
    const int32_t t = state->t;
    if (n < min_shared || n < 1 || c >= ncand) { state->done = 1; state->pick = -1; return; }
    const uint32_t r = (uint32_t)cand[c];
    const int32_t left = state->remaining - n;
    if (t >= 0 && t < max_rounds) { // (always: checked on entry)
        int32_t* row = out4 + (size_t)t * 4;
        row[0] = (int32_t)r; row[1] = n; row[2] = r < nref ? total[r] : 0; row[3] = left;
    }
    state->pick = (int32_t)c;
    state->t = t + 1;
    state->remaining = left;
}

// A grid over the pick's hit list: its query values leave.  One byte per value: lanes that clear distinct indices need no atomic.
__global__ __launch_bounds__(GATHER_T) void k_gather_remove(const GatherState* __restrict__ state, uint8_t* __restrict__ alive, uint32_t nq,
                                                            const uint64_t* __restrict__ coff, uint32_t ncand, uint64_t nlist,
                                                            const uint32_t* __restrict__ list) {
    const int32_t c = state->pick;
    if (c < 0 || (uint32_t)c >= ncand) return;
    const uint64_t end = min(coff[c + 1], nlist), begin = min(coff[c], end);
    const uint64_t step = (uint64_t)gridDim.x * GATHER_T;
    for (uint64_t i = begin + (uint64_t)blockIdx.x * GATHER_T + threadIdx.x; i < end; i += step) {
        const uint32_t h = list[i];
        if (h < nq) alive[h] = 0;
    }
}

// k_gather_remove when the call carries abundances (include/rkmh_amd.h, "ABUNDANCE"): the same grid over the same list; a lane also
// reads the abundance of every value it takes out of the query, the wave adds its lanes' sums with shuffles, and its first lane adds
// the result to wunique[t - 1], the row k_gather_pick has just written.  Integer sums: the order of the additions cannot change them.
// Indices within one hit list are distinct (the rows ascend), so no two lanes see the same byte alive.
__global__ __launch_bounds__(GATHER_T) void k_gather_remove_w(const GatherState* __restrict__ state, int32_t max_rounds, uint8_t* __restrict__ alive,
                                                              const uint32_t* __restrict__ q_abund, uint32_t nq, const uint64_t* __restrict__ coff,
                                                              uint32_t ncand, uint64_t nlist, const uint32_t* __restrict__ list,
                                                              unsigned long long* __restrict__ wunique) {
    const int32_t c = state->pick; // (uniform over the grid: whole workgroups leave)
    if (c < 0 || (uint32_t)c >= ncand) return;
    const int32_t row = state->t - 1;
    const uint64_t end = min(coff[c + 1], nlist), begin = min(coff[c], end);
    const uint64_t step = (uint64_t)gridDim.x * GATHER_T;
    unsigned long long sum = 0;
    for (uint64_t i = begin + (uint64_t)blockIdx.x * GATHER_T + threadIdx.x; i < end; i += step) {
        const uint32_t h = list[i];
        if (h < nq) {
            if (alive[h]) sum += q_abund[h];
            alive[h] = 0;
        }
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum != 0 && row >= 0 && row < max_rounds) atomicAdd(wunique + row, sum);
}

// The loop on resident arrays, on stream st, with the context's work buffers (the caller holds general_mu).  d_out4 takes at most
// max_rounds rows.  d_wunique != nullptr: a weighted call (d_q_abund: one uint32 per query value), d_wunique takes one uint64 per row and is zeroed as far as rows can be
// written.  Synchronises st.
int gather_run(rk_ctx* c, const uint64_t* d_q, const uint32_t* d_q_abund, uint64_t nq, const uint64_t* d_rv, const uint64_t* d_ro, int nref,
               uint64_t r_nvalues, int min_shared, int max_rounds, int32_t* d_out4, uint64_t* d_wunique, int* nrounds, hipStream_t st) {
    *nrounds = 0;
    const uint32_t nq32 = (uint32_t)nq;
    if (d_wunique) HIPCHK(hipMemsetAsync(d_wunique, 0, (size_t)std::min(max_rounds, nref) * 8, st));
    // 1. probe: hit[] parallel to the reference values, total[r]
    RKCHK(c->w_g_hit.reserve((size_t)r_nvalues * 4 + 4));
    RKCHK(c->w_g_total.reserve((size_t)nref * 4));
    RKCHK(c->w_g_alive.reserve((size_t)nq + 1));
    RKCHK(c->w_g_state.reserve(sizeof(GatherState)));
    uint32_t* d_hit = c->w_g_hit.as<uint32_t>();
    int32_t* d_total = c->w_g_total.as<int32_t>();
    uint8_t* d_alive = c->w_g_alive.as<uint8_t>();
    GatherState* d_state = c->w_g_state.as<GatherState>();
    hipLaunchKernelGGL(k_gather_probe, dim3(wave_grid((uint64_t)nref, GATHER_WAVES)), dim3(GATHER_T), 0, st, d_q, nq32, d_rv, d_ro, (uint32_t)nref, r_nvalues, d_hit, d_total);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> total((size_t)nref);
    HIPCHK(hipMemcpyAsync(total.data(), d_total, (size_t)nref * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // 2. the candidates: references that share at least min_shared values with Q -- the others can never win -- and where each one's
    // hit list begins
    std::vector<int32_t> cand;
    std::vector<uint64_t> coff(1, 0);
    uint64_t longest = 0;
    for (int r = 0; r < nref; ++r) {
        const int32_t n = total[(size_t)r];
        if (n < 0 || (uint64_t)n > nq || (uint64_t)n > r_nvalues) return fail(RK_ERR_HIP, "gather: reference %d shares %d values with a query of %llu", r, n, (unsigned long long)nq);
        if (n < min_shared) continue;
        cand.push_back(r);
        coff.push_back(coff.back() + (uint64_t)n);
        longest = std::max(longest, (uint64_t)n);
    }
    const uint32_t ncand = (uint32_t)cand.size();
    if (ncand == 0) return RK_OK;
    const uint64_t nlist = coff.back();
    RKCHK(c->w_g_cand.reserve((size_t)ncand * 4));
    RKCHK(c->w_g_coff.reserve(((size_t)ncand + 1) * 8));
    RKCHK(c->w_g_count.reserve((size_t)ncand * 4));
    RKCHK(c->w_g_list.reserve((size_t)nlist * 4));
    int32_t* d_cand = c->w_g_cand.as<int32_t>();
    uint64_t* d_coff = c->w_g_coff.as<uint64_t>();
    int32_t* d_count = c->w_g_count.as<int32_t>();
    uint32_t* d_list = c->w_g_list.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(d_cand, cand.data(), (size_t)ncand * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_coff, coff.data(), ((size_t)ncand + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gather_compact, dim3(wave_grid(ncand, GATHER_WAVES)), dim3(GATHER_T), 0, st, d_ro, (uint32_t)nref, r_nvalues, d_hit, d_cand, d_coff, ncand, nlist, d_list);
    HIPCHK(hipGetLastError());
    // 3. the state of this call: every query value alive, no row written (nothing of an earlier call on this context survives)
    GatherState s0{};
    s0.pick = -1; s0.remaining = (int32_t)nq;
    HIPCHK(hipMemsetAsync(d_alive, 1, (size_t)nq, st));
    HIPCHK(hipMemcpyAsync(d_state, &s0, sizeof s0, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (cand, coff and s0 are pageable host memory: they live until here)
    // 4. rounds, in groups of RK_GATHER_BATCH: no reference is picked twice, so min(max_rounds, ncand) rounds are all there can be
    const int rounds = (int)std::min<uint64_t>((uint64_t)max_rounds, ncand);
    const dim3 count_grid(wave_grid(ncand, GATHER_WAVES)), remove_grid((uint32_t)std::min<uint64_t>((longest + GATHER_T - 1) / GATHER_T, 1024));
    GatherState s{};
    for (int launched = 0; launched < rounds;) {
        const int group = std::min(RK_GATHER_BATCH, rounds - launched);
        for (int i = 0; i < group; ++i) {
            hipLaunchKernelGGL(k_gather_count, count_grid, dim3(GATHER_T), 0, st, d_state, rounds, d_alive, nq32, d_coff, ncand, nlist, d_list, d_count);
            hipLaunchKernelGGL(k_gather_pick, dim3(1), dim3(PICK_T), 0, st, d_state, rounds, min_shared, d_count, d_cand, ncand, d_total, (uint32_t)nref, d_out4);
            if (d_wunique)
                hipLaunchKernelGGL(k_gather_remove_w, remove_grid, dim3(GATHER_T), 0, st, d_state, rounds, d_alive, d_q_abund, nq32, d_coff, ncand, nlist, d_list,
                                   (unsigned long long*)d_wunique);
            else
                hipLaunchKernelGGL(k_gather_remove, remove_grid, dim3(GATHER_T), 0, st, d_state, d_alive, nq32, d_coff, ncand, nlist, d_list);
        }
        HIPCHK(hipGetLastError());
        launched += group;
        HIPCHK(hipMemcpyAsync(&s, d_state, sizeof s, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (s.done) break;
    }
    if (s.t < 0 || s.t > rounds) return fail(RK_ERR_HIP, "gather: %d rows written of at most %d", s.t, rounds);
    *nrounds = s.t;
    return RK_OK;
}

int check_gather_shape(uint64_t nq, int nref, int min_shared, int max_rounds) {
    if (nref < 1) return fail(RK_ERR_ARG, "gather: need at least one reference sketch, got %d", nref);
    if (min_shared < 1) return fail(RK_ERR_ARG, "gather: min_shared %d is below 1", min_shared);
    if (max_rounds < 1) return fail(RK_ERR_ARG, "gather: max_rounds %d is below 1", max_rounds);
    if (nq > 0x7fffffffull) return fail(RK_ERR_LIMIT, "gather: a query of %llu values is more than 2^31-1", (unsigned long long)nq);
    return RK_OK;
}

// the entry on resident arrays; d_wunique: nullptr for the plain call
int gather_resident(rk_ctx* c, const void* d_q_values, const void* d_q_abund, uint64_t nq, const void* d_r_values, const void* d_r_offsets, int nref,
                    uint64_t r_nvalues, int min_shared, int max_rounds, void* d_out4, void* d_wunique, int* nrounds, void* hip_stream) {
    if (!c || !d_r_offsets || !d_out4 || !nrounds || (!d_q_values && nq) || (!d_r_values && r_nvalues)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_gather_shape(nq, nref, min_shared, max_rounds));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(c->general_mu);
    return gather_run(c, (const uint64_t*)d_q_values, (const uint32_t*)d_q_abund, nq, (const uint64_t*)d_r_values, (const uint64_t*)d_r_offsets, nref, r_nvalues,
                      min_shared, max_rounds, (int32_t*)d_out4, (uint64_t*)d_wunique, nrounds, (hipStream_t)hip_stream);
}

// the entry on host arrays; wunique: nullptr for the plain call
int gather_uploaded(rk_ctx* c, const uint64_t* q_values, const uint32_t* q_abund, uint64_t nq, const uint64_t* r_values, const uint64_t* r_offsets, int nref,
                    int min_shared, int max_rounds, int32_t* out4, uint64_t* wunique, int* nrounds) {
    if (!c || !r_offsets || !out4 || !nrounds || (!q_values && nq)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_gather_shape(nq, nref, min_shared, max_rounds));
    for (uint64_t i = 0; i < nq; ++i)
        if (q_values[i] == 0 || (i && q_values[i] <= q_values[i - 1])) return fail(RK_ERR_ARG, "gather: the query is not ascending, distinct and non-zero at value %llu", (unsigned long long)i);
    if (wunique) RKCHK(check_abund(q_abund, 0, nq, "gather: ", "the query"));
    RKCHK(check_csr(r_offsets, nref, "gather: ", "the references", RK_ERR_LIMIT));
    const uint64_t rn = r_offsets[nref] - r_offsets[0]; // the values the rows cover
    if (rn && !r_values) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(c->general_mu); // the general path's work buffers serve here too
    const int rows = std::min(max_rounds, nref);
    RKCHK(c->w_sk.reserve((size_t)(nq + rn) * 8 + 8));
    RKCHK(c->w_sc_off.reserve(((size_t)nref + 1) * 8));
    RKCHK(c->w_out.reserve((size_t)rows * 16));
    uint64_t* d_q = c->w_sk.as<uint64_t>();
    uint64_t* d_rv = d_q + nq;
    uint64_t* d_ro = c->w_sc_off.as<uint64_t>();
    uint64_t* d_wu = nullptr;  // the weighted call: wunique[rows], then the query's abundances
    uint32_t* d_qa = nullptr;
    if (wunique) {
        RKCHK(c->w_g_ab.reserve((size_t)rows * 8 + (size_t)nq * 4 + 4));
        d_wu = c->w_g_ab.as<uint64_t>();
        d_qa = (uint32_t*)(d_wu + rows);
        if (nq) HIPCHK(hipMemcpyAsync(d_qa, q_abund, (size_t)nq * 4, hipMemcpyHostToDevice, c->st));
    }
    std::vector<uint64_t> off;
    if (nq) HIPCHK(hipMemcpyAsync(d_q, q_values, (size_t)nq * 8, hipMemcpyHostToDevice, c->st));
    RKCHK(upload_csr(r_values, r_offsets, nref, d_rv, d_ro, off, c->st));
    RKCHK(gather_run(c, d_q, d_qa, nq, d_rv, d_ro, nref, rn, min_shared, rows, c->w_out.as<int32_t>(), d_wu, nrounds, c->st)); // (synchronises: off lives until there)
    if (*nrounds) HIPCHK(hipMemcpyAsync(out4, c->w_out.p, (size_t)*nrounds * 16, hipMemcpyDeviceToHost, c->st));
    if (wunique) HIPCHK(hipMemcpyAsync(wunique, d_wu, (size_t)rows * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

} // namespace

extern "C" int rk_gather_scaled_device(rk_ctx* c, const void* d_q_values, uint64_t nq, const void* d_r_values, const void* d_r_offsets, int nref,
                                       uint64_t r_nvalues, int min_shared, int max_rounds, void* d_out4, int* nrounds, void* hip_stream) {
    return gather_resident(c, d_q_values, nullptr, nq, d_r_values, d_r_offsets, nref, r_nvalues, min_shared, max_rounds, d_out4, nullptr, nrounds, hip_stream);
}
extern "C" int rk_gather_scaled_abund_device(rk_ctx* c, const void* d_q_values, const void* d_q_abund, uint64_t nq, const void* d_r_values,
                                             const void* d_r_offsets, int nref, uint64_t r_nvalues, int min_shared, int max_rounds, void* d_out4,
                                             void* d_wunique, int* nrounds, void* hip_stream) {
    if (!d_wunique || (!d_q_abund && nq)) return fail(RK_ERR_ARG, "bad arguments");
    return gather_resident(c, d_q_values, d_q_abund, nq, d_r_values, d_r_offsets, nref, r_nvalues, min_shared, max_rounds, d_out4, d_wunique,
                           nrounds, hip_stream);
}

extern "C" int rk_gather_scaled(rk_ctx* c, const uint64_t* q_values, uint64_t nq, const uint64_t* r_values, const uint64_t* r_offsets, int nref,
                                int min_shared, int max_rounds, int32_t* out4, int* nrounds) {
    return gather_uploaded(c, q_values, nullptr, nq, r_values, r_offsets, nref, min_shared, max_rounds, out4, nullptr, nrounds);
}
extern "C" int rk_gather_scaled_abund(rk_ctx* c, const uint64_t* q_values, const uint32_t* q_abund, uint64_t nq, const uint64_t* r_values,
                                      const uint64_t* r_offsets, int nref, int min_shared, int max_rounds, int32_t* out4, uint64_t* wunique, int* nrounds) {
    if (!wunique || (!q_abund && nq)) return fail(RK_ERR_ARG, "bad arguments");
    return gather_uploaded(c, q_values, q_abund, nq, r_values, r_offsets, nref, min_shared, max_rounds, out4, wunique, nrounds);
}
