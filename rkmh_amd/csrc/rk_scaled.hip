// rk_scaled.hip -- scaled (FracMinHash) sketches (include/rkmh_amd.h, "SCALED SKETCHES"): the step of the general path that turns a
// chunk's window hashes into one variable-length set per sequence (keep / sort / drop repeats), and k_scaled_pairs, which intersects
// every pair of such sets, plainly or weighted by abundance.  The compaction behind keep and drop repeats is rk_sets.hpp's.  The
// host-only half (threshold, union, distance) is rk_scaled_host.cpp; semantics, routes, the lane rule and measurements: DESIGN.md
// section 11; the abundances (the run lengths of the drop-repeats step): section 13; the weighted pairs and k_abund_row_sums: section 14.
#include "rk_sets.hpp"

namespace {

// ---- abundances (include/rkmh_amd.h, "ABUNDANCE"): the length of every run that KEEP_FIRST collapses.  Every element of the sorted
// array is the first of its value in its segment or a repeat of the element before it, so run j ends where run j + 1 begins, and the
// last one at n.  k_keep_first_src is KEEP_FIRST's scatter that also notes where each first stood; k_run_lengths subtracts neighbours.
__global__ __launch_bounds__(KEEP_T) void k_keep_first_src(const uint64_t* __restrict__ v, uint64_t n, const uint64_t* __restrict__ off, uint32_t nseg,
                                                           const uint64_t* __restrict__ pre, uint64_t* __restrict__ out, uint64_t* __restrict__ src,
                                                           uint64_t out_cap) {
    keep_scatter_block<KEEP_FIRST, true>(v, n, 0, off, nseg, pre, out, src, out_cap);
}
// abund[j] = (j + 1 < m ? src[j + 1] : n) - src[j] for j < m, m = *kept (the scan's total: the number of firsts) clamped to cap, the
// length of src[] and abund[]; a run longer than 2^32 - 1 is stored as 2^32 - 1.  One thread per run.
__global__ __launch_bounds__(KEEP_T) void k_run_lengths(const uint64_t* __restrict__ src, const uint64_t* __restrict__ kept, uint64_t n, uint64_t cap,
                                                        uint32_t* __restrict__ abund) {
    const uint64_t m = min(*kept, cap);
    const uint64_t j = (uint64_t)blockIdx.x * KEEP_T + threadIdx.x;
    if (j >= m) return;
    const uint64_t begin = src[j], end = j + 1 < m ? src[j + 1] : n;
    abund[j] = (uint32_t)min(end > begin ? end - begin : (uint64_t)0, (uint64_t)0xffffffffu);
}

// KEEP_FIRST's scatter with the abundances: d_src and d_abund hold n entries each, as out does; the number of firsts is read on the device
int keep_first_abund(rk_ctx* c, const uint64_t* v, uint64_t n, const uint64_t* d_off, uint32_t nseg, uint64_t* out, uint64_t* d_src, uint32_t* d_abund) {
    const uint64_t nblocks = (n + KEEP_BLK - 1) / KEEP_BLK;
    if (!nblocks) return RK_OK;
    if ((n + KEEP_T - 1) / KEEP_T > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%llu kept values are more than one run-length launch takes", (unsigned long long)n);
    const uint64_t* d_pre = c->w_sc_pre.as<uint64_t>();
    hipLaunchKernelGGL(k_keep_first_src, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, c->st, v, n, d_off, nseg, d_pre, out, d_src, n);
    hipLaunchKernelGGL(k_run_lengths, dim3((uint32_t)((n + KEEP_T - 1) / KEEP_T)), dim3(KEEP_T), 0, c->st, d_src, d_pre + nblocks, n, n, d_abund);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

int grow_sink(ScaledSink& sink, size_t more) {
    if (sink.len + more <= sink.cap) return RK_OK;
    size_t cap = std::max(sink.len + more, sink.cap + sink.cap / 2) + 16;
    uint64_t* p = (uint64_t*)realloc(sink.values, cap * 8);
    if (!p) return fail(RK_ERR_NOMEM, "realloc of %zu scaled values", cap);
    sink.values = p;
    if (sink.with_abund) {
        uint32_t* a = (uint32_t*)realloc(sink.abund, cap * 4);
        if (!a) return fail(RK_ERR_NOMEM, "realloc of %zu abundances", cap);
        sink.abund = a;
    }
    sink.cap = cap;
    return RK_OK;
}

} // namespace

// One chunk of general_run: its hashes are in w_hashes, its segment offsets (seg[n + 1], also at w_segoff) say which belong to which
// sequence.  Appends the scaled sketch of every sequence of the chunk to sink.values and sets sink.offsets[i0 + 1 ..].  Synchronises.
int scaled_keep_chunk(rk_ctx* c, const std::vector<uint64_t>& seg, uint64_t nhashes, int64_t i0, ScaledSink& sink) {
    const size_t cn = seg.size() - 1;
    if (cn > 0x7ffffffeull) return fail(RK_ERR_LIMIT, "more than 2^31-2 sequences in one chunk");
    const uint32_t nseg = (uint32_t)cn;
    if (nhashes == 0) {
        for (size_t q = 0; q < cn; ++q) sink.offsets[i0 + q + 1] = sink.len;
        return RK_OK;
    }
    // 1. keep: 0 < h <= max_hash, compacted; koff1 = where each sequence's kept values begin
    RKCHK(c->w_sc_off.reserve((cn + 1) * 8 * 2));
    uint64_t* d_koff1 = c->w_sc_off.as<uint64_t>();
    uint64_t* d_koff2 = d_koff1 + cn + 1;
    const uint64_t* d_hashes = c->w_hashes.as<uint64_t>();
    const uint64_t* d_seg = c->w_segoff.as<uint64_t>();
    RKCHK(keep_counts<KEEP_HASH>(c->w_sc_cnt, c->w_sc_pre, d_hashes, nhashes, sink.max_hash, d_seg, nseg, d_koff1, c->st));
    std::vector<uint64_t> koff(cn + 1);
    HIPCHK(hipMemcpyAsync(koff.data(), d_koff1, (cn + 1) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    const uint64_t total1 = koff[cn];
    if (total1 > nhashes) return fail(RK_ERR_HIP, "scaled keep: %llu values kept of %llu hashes", (unsigned long long)total1, (unsigned long long)nhashes);
    if (total1 == 0) {
        for (size_t q = 0; q < cn; ++q) sink.offsets[i0 + q + 1] = sink.len;
        return RK_OK;
    }
    RKCHK(c->w_sc_a.reserve((size_t)total1 * 8));
    RKCHK(c->w_sc_b.reserve((size_t)total1 * 8));
    uint64_t* d_a = c->w_sc_a.as<uint64_t>();
    uint64_t* d_b = c->w_sc_b.as<uint64_t>();
    RKCHK(keep_scatter<KEEP_HASH>(c->w_sc_pre, d_hashes, nhashes, sink.max_hash, d_seg, nseg, d_a, total1, c->st));
    // 2. sort every sequence's kept values in place: up to SORT_MAX_P by the in-LDS sorter, one launch per power of two (the general
    // path's size classes); longer ones by the whole-array radix sort, one call each.  0 or 1 values need no sort.
    std::vector<std::vector<uint32_t>> classes(32);
    std::vector<uint32_t> long_ids;
    uint64_t longest = 0;
    size_t nids = 0;
    for (size_t q = 0; q < cn; ++q) {
        const uint64_t m = koff[q + 1] - koff[q];
        if (m < 2) continue;
        if (m > (uint64_t)SORT_MAX_P) { long_ids.push_back((uint32_t)q); longest = std::max(longest, m); continue; }
        int cls = 0; while ((64u << cls) < m) ++cls;
        classes[cls].push_back((uint32_t)q); ++nids;
    }
    RKCHK(c->w_ids.reserve((nids + 1) * 4));
    uint32_t* d_ids = c->w_ids.as<uint32_t>();
    for (int cls = 0; cls < 32; ++cls) {
        const std::vector<uint32_t>& ids = classes[cls];
        if (ids.empty()) continue;
        HIPCHK(hipMemcpyAsync(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, c->st));
        SortArgs a{};
        a.hashes = d_a; a.seg_off = d_koff1; a.seq_ids = d_ids; a.nlist = (uint32_t)ids.size(); a.P = 64u << cls; a.S = 1;
        a.write_back = 1; a.slots = 1; a.filter_mode = FILTER_NONE;
        HIPCHK(launch_sort_intersect(a, nullptr, c->pol, c->st));
        d_ids += ids.size();
    }
    if (!long_ids.empty()) {
        size_t tmp_bytes = 0;
        HIPCHK(sort_u64_temp_bytes(longest, &tmp_bytes));
        RKCHK(c->w_misc.reserve(tmp_bytes));
        for (uint32_t q : long_ids) HIPCHK(launch_sort_u64(d_a + koff[q], koff[q + 1] - koff[q], c->w_misc.p, tmp_bytes, c->st));
    }
    // 3. drop repeats: the first of every value in its segment stays
    RKCHK(keep_counts<KEEP_FIRST>(c->w_sc_cnt, c->w_sc_pre, d_a, total1, 0, d_koff1, nseg, d_koff2, c->st));
    uint32_t* d_abund = nullptr;
    if (sink.with_abund) { // the run lengths leave with the values
        RKCHK(c->w_sc_src.reserve((size_t)total1 * 8));
        RKCHK(c->w_sc_ab.reserve((size_t)total1 * 4));
        d_abund = c->w_sc_ab.as<uint32_t>();
        RKCHK(keep_first_abund(c, d_a, total1, d_koff1, nseg, d_b, c->w_sc_src.as<uint64_t>(), d_abund));
    } else
        RKCHK(keep_scatter<KEEP_FIRST>(c->w_sc_pre, d_a, total1, 0, d_koff1, nseg, d_b, total1, c->st));
    std::vector<uint64_t> koff2(cn + 1);
    HIPCHK(hipMemcpyAsync(koff2.data(), d_koff2, (cn + 1) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st)); // (the id vectors of step 2 live until here)
    const uint64_t total2 = koff2[cn];
    if (total2 > total1) return fail(RK_ERR_HIP, "scaled keep: %llu distinct values of %llu", (unsigned long long)total2, (unsigned long long)total1);
    RKCHK(grow_sink(sink, (size_t)total2));
    if (total2) HIPCHK(hipMemcpyAsync(sink.values + sink.len, d_b, (size_t)total2 * 8, hipMemcpyDeviceToHost, c->st));
    if (total2 && d_abund) HIPCHK(hipMemcpyAsync(sink.abund + sink.len, d_abund, (size_t)total2 * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    for (size_t q = 0; q < cn; ++q) sink.offsets[i0 + q + 1] = sink.len + koff2[q + 1];
    sink.len += (size_t)total2;
    return RK_OK;
}

static int sketch_scaled(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nseq, const int* ks, int nks, uint64_t max_hash,
                         uint64_t** values, uint32_t** abunds, uint64_t* sk_offsets) {
    if (!c || !offsets || nseq < 0 || !values || !sk_offsets) return fail(RK_ERR_ARG, "bad arguments");
    GeneralCfg cfg;
    RKCHK(check_ks(ks, nks, &cfg.ks));
    ScaledSink sink;
    sink.max_hash = max_hash; sink.offsets = sk_offsets; sink.with_abund = abunds != nullptr;
    sink.values = (uint64_t*)malloc(8 * 16); sink.cap = 16;
    if (sink.with_abund) sink.abund = (uint32_t*)malloc(4 * 16);
    if (!sink.values || (sink.with_abund && !sink.abund)) { free(sink.values); free(sink.abund); return fail(RK_ERR_NOMEM, "malloc"); }
    sk_offsets[0] = 0;
    GeneralOut go; go.scaled = &sink;
    const int r = general_run(c, bases, nullptr, offsets, nseq, cfg, go);
    if (r != RK_OK) { free(sink.values); free(sink.abund); return r; }
    *values = sink.values;
    if (abunds) *abunds = sink.abund;
    return RK_OK;
}
extern "C" int rk_sketch_scaled_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nseq, const int* ks, int nks,
                                      uint64_t max_hash, uint64_t** values, uint64_t* sk_offsets) {
    return sketch_scaled(c, bases, offsets, nseq, ks, nks, max_hash, values, nullptr, sk_offsets);
}
extern "C" int rk_sketch_scaled_abund_batch(rk_ctx* c, const uint8_t* bases, const uint64_t* offsets, int64_t nseq, const int* ks, int nks,
                                            uint64_t max_hash, uint64_t** values, uint32_t** abunds, uint64_t* sk_offsets) {
    if (!abunds) return fail(RK_ERR_ARG, "bad arguments");
    return sketch_scaled(c, bases, offsets, nseq, ks, nks, max_hash, values, abunds, sk_offsets);
}

// ---- pairs ---------------------------------------------------------------------------------------------------------------
// ---- pairs, plain and weighted (include/rkmh_amd.h, "WEIGHTED COMPARISON") ------------------------------------
namespace {

constexpr int PAIRS_T = 256;

// What a lane of k_scaled_pairs keeps of its slice of the merge.  equal(eq, ...) sees every step of it: ii and jj are the indices at
// which x and y were read, inside the clamped rows, so the abundances XW, YW, which lie parallel to the values, may be read there.
// add_lane(d) adds the partial result of lane (self ^ d); store writes the pair's answer.
struct PairsPlain { // the number of equal values: one int32 per pair
    typedef int32_t Out;
    static constexpr int WIDTH = 1;
    static constexpr bool WEIGHTED = false;
    int cnt = 0;
    __device__ __forceinline__ void equal(bool eq, const uint32_t* __restrict__, const uint32_t* __restrict__, uint32_t, uint32_t) { cnt += eq ? 1 : 0; }
    __device__ __forceinline__ void add_lane(int d) { cnt += __shfl_xor(cnt, d, 64); }
    __device__ __forceinline__ void store(Out* out, uint64_t p, bool) const { out[p] = cnt; }
};
// shared, dot (saturating), wx, wy: four uint64 per pair.  X is the shorter row whichever side it is: the sums are kept per row of
// the merge (wx, wy) and given their sides at the end.  wx and wy cannot overflow: fewer than 2^31 values below 2^32 each.
struct PairsWeighted {
    typedef uint64_t Out;
    static constexpr int WIDTH = 4;
    static constexpr bool WEIGHTED = true;
    uint64_t cnt = 0, dot = 0, wx = 0, wy = 0;
    __device__ __forceinline__ void equal(bool eq, const uint32_t* __restrict__ XW, const uint32_t* __restrict__ YW, uint32_t ii, uint32_t jj) {
        if (eq) {
            const uint64_t u = XW[ii], w = YW[jj];
            cnt += 1;
            dot = sat_add(dot, u * w); // (2^32 - 1)^2 < 2^64
            wx += u;
            wy += w;
        }
    }
    __device__ __forceinline__ void add_lane(int d) {
        cnt += shfl_xor_u64(cnt, d);
        dot = sat_add(dot, shfl_xor_u64(dot, d));
        wx += shfl_xor_u64(wx, d);
        wy += shfl_xor_u64(wy, d);
    }
    __device__ __forceinline__ void store(Out* out, uint64_t p, bool a_short) const {
        uint64_t* o = out + p * 4;
        o[0] = cnt;
        o[1] = dot;
        o[2] = a_short ? wx : wy;
        o[3] = a_short ? wy : wx;
    }
};

// L lanes per pair, 64 / L pairs per wave.  The shorter row X is cut into L contiguous slices, lane `sub` owns X[s0, s1): it finds the
// first element of the other row Y that is not below X[s0] (at most 32 halvings) and walks a two-pointer merge from there until its
// slice or Y ends, handing every step to its Acc.  Every element of X belongs to exactly one lane, so a value at a slice boundary is
// counted once.  Every step advances an index below its length; every read is at an index of a row clamped to [0, nvalues]; compares
// are 64-bit unsigned.  Rows that are not ascending give meaningless results and nothing worse.  The L partial results are added
// with shuffles inside the aligned group of L lanes; no LDS, no atomics; the group's first lane stores.  aw, bw: PairsWeighted only.
template <int L, typename Acc>
__global__ __launch_bounds__(PAIRS_T) void k_scaled_pairs(const uint64_t* __restrict__ av, const uint32_t* __restrict__ aw, const uint64_t* __restrict__ aoff,
                                                          int na, uint64_t an, const uint64_t* __restrict__ bv, const uint32_t* __restrict__ bw,
                                                          const uint64_t* __restrict__ boff, int nb, uint64_t bn, typename Acc::Out* __restrict__ out) {
    const uint64_t npairs = (uint64_t)na * (uint64_t)nb;
    const uint64_t p = (uint64_t)blockIdx.x * (PAIRS_T / L) + threadIdx.x / L;
    const uint32_t sub = threadIdx.x % L;
    const bool live = p < npairs; // lanes without a pair still take part in the shuffles
    Acc acc;
    bool a_short = true;
    if (live) {
        uint64_t a0, a1, b0, b1;
        clamped_row(aoff, p / (uint64_t)nb, an, a0, a1);
        clamped_row(boff, p % (uint64_t)nb, bn, b0, b1);
        const uint32_t la = (uint32_t)(a1 - a0), lb = (uint32_t)(b1 - b0);
        a_short = la <= lb;
        const uint64_t* __restrict__ X = a_short ? av + a0 : bv + b0;
        const uint64_t* __restrict__ Y = a_short ? bv + b0 : av + a0;
        const uint32_t* __restrict__ XW = a_short ? aw + a0 : bw + b0;
        const uint32_t* __restrict__ YW = a_short ? bw + b0 : aw + a0;
        const uint32_t lx = a_short ? la : lb, ly = a_short ? lb : la;
        const uint32_t s0 = (uint32_t)((uint64_t)lx * sub / L), s1 = (uint32_t)((uint64_t)lx * (sub + 1) / L);
        if (s0 < s1 && ly > 0) {
            uint64_t x = X[s0];
            uint32_t ii = s0, jj = L > 1 && s0 > 0 ? first_not_below(Y, 0u, ly, x) : 0u;
            if (jj < ly) {
                uint64_t y = Y[jj];
                for (;;) {
                    const bool ax = x <= y, ay = y <= x;
                    acc.equal(ax && ay, XW, YW, ii, jj);
                    ii += ax ? 1u : 0u;
                    jj += ay ? 1u : 0u;
                    if (ii >= s1 || jj >= ly) break;
                    if (ax) x = X[ii];
                    if (ay) y = Y[jj];
                }
            }
        }
    }
    for (int d = L >> 1; d > 0; d >>= 1) acc.add_lane(d);
    if (live && sub == 0) acc.store(out, p, a_short); // a_short is the group's: every lane of it has the same pair
}

// out[i * 2] = sum of row i's abundances, out[i * 2 + 1] = sum of their squares, saturating.  One wave per row, grid-stride; the
// lanes stride the row.  Rows are clamped to [0, nvalues] and to 2^31 - 1 entries, so the sum is exact.
constexpr int SUMS_T = 256;
__global__ __launch_bounds__(SUMS_T) void k_abund_row_sums(const uint32_t* __restrict__ w, const uint64_t* __restrict__ off, int n, uint64_t nvalues,
                                                           uint64_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i = (uint64_t)blockIdx.x * (SUMS_T / 64) + (threadIdx.x >> 6); i < (uint64_t)n; i += (uint64_t)gridDim.x * (SUMS_T / 64)) { // whole waves
        uint64_t r0, r1;
        clamped_row(off, i, nvalues, r0, r1);
        uint64_t sum = 0, sq = 0;
        for (uint64_t t = lane; t < r1 - r0; t += 64) {
            const uint64_t u = w[r0 + t];
            sum += u;
            sq = sat_add(sq, u * u);
        }
        for (int d = 32; d > 0; d >>= 1) {
            sum += shfl_xor_u64(sum, d);
            sq = sat_add(sq, shfl_xor_u64(sq, d));
        }
        if (lane == 0) { out[i * 2] = sum; out[i * 2 + 1] = sq; }
    }
}

// The lane rule of lanes = 0: a function of the mean length of the shorter side alone (measured at 800 and 5 000 values: DESIGN.md section 11).
int auto_lanes(uint64_t an, int na, uint64_t bn, int nb) {
    const uint64_t mean = std::min(an / (uint64_t)na, bn / (uint64_t)nb);
    return mean < 16384 ? 1 : mean < 262144 ? 8 : 64;
}

template <typename Acc>
int launch_scaled_pairs(const uint64_t* av, const uint32_t* aw, const uint64_t* aoff, int na, uint64_t an, const uint64_t* bv, const uint32_t* bw,
                        const uint64_t* boff, int nb, uint64_t bn, int lanes, typename Acc::Out* out, hipStream_t st) {
    const int L = lanes ? lanes : auto_lanes(an, na, bn, nb);
    const uint64_t per = (uint64_t)(PAIRS_T / L), blocks = ((uint64_t)na * (uint64_t)nb + per - 1) / per;
    if (blocks > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%d x %d sketches are more pairs than one launch takes", na, nb);
    auto* kernel = L == 1 ? k_scaled_pairs<1, Acc> : L == 8 ? k_scaled_pairs<8, Acc> : k_scaled_pairs<64, Acc>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(PAIRS_T), 0, st, av, aw, aoff, na, an, bv, bw, boff, nb, bn, out);
    HIPCHK(hipGetLastError());
    return RK_OK;
}
int launch_row_sums(const uint32_t* w, const uint64_t* off, int n, uint64_t nvalues, uint64_t* out, hipStream_t st) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + SUMS_T / 64 - 1) / (SUMS_T / 64), 16384);
    hipLaunchKernelGGL(k_abund_row_sums, dim3(blocks), dim3(SUMS_T), 0, st, w, off, n, nvalues, out);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

int check_pairs_shape(int na, int nb, int lanes) {
    if (na < 1 || nb < 1) return fail(RK_ERR_ARG, "need at least one sketch on each side, got %d x %d", na, nb);
    if (lanes != 0 && lanes != 1 && lanes != 8 && lanes != 64) return fail(RK_ERR_ARG, "lanes %d is none of 0, 1, 8, 64", lanes);
    return RK_OK;
}

// The entry on host arrays behind rk_compare_scaled and rk_compare_scaled_abund (PairsWeighted: with the abundances of both sides).
// When b is a itself, it is uploaded once.  The rows of the answer leave in blocks of at most 64 MB.
template <typename Acc>
int compare_uploaded(rk_ctx* c, const uint64_t* a_values, const uint32_t* a_abund, const uint64_t* a_offsets, int na, const uint64_t* b_values,
                     const uint32_t* b_abund, const uint64_t* b_offsets, int nb, int lanes, typename Acc::Out* out) {
    if (!c || !a_offsets || !b_offsets || !out) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_pairs_shape(na, nb, lanes));
    RKCHK(check_csr(a_offsets, na, "", "a", RK_ERR_ARG));
    RKCHK(check_csr(b_offsets, nb, "", "b", RK_ERR_ARG));
    const uint64_t an = a_offsets[na], bn = b_offsets[nb];
    if ((an && (!a_values || (Acc::WEIGHTED && !a_abund))) || (bn && (!b_values || (Acc::WEIGHTED && !b_abund)))) return fail(RK_ERR_ARG, "bad arguments");
    const bool self = a_values == b_values && a_abund == b_abund && a_offsets == b_offsets && na == nb;
    if (Acc::WEIGHTED) {
        RKCHK(check_abund(a_abund, a_offsets[0], an, "", "a"));
        if (!self) RKCHK(check_abund(b_abund, b_offsets[0], bn, "", "b"));
    }
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(c->general_mu); // the general path's work buffers serve here too
    RKCHK(c->w_sk.reserve((size_t)(an + (self ? 0 : bn)) * 8 + 8));
    if (Acc::WEIGHTED) RKCHK(c->w_sc_ab.reserve((size_t)(an + (self ? 0 : bn)) * 4 + 4));
    RKCHK(c->w_sc_off.reserve(((size_t)na + 1 + (self ? 0 : (size_t)nb + 1)) * 8));
    uint64_t* d_av = c->w_sk.as<uint64_t>();
    uint64_t* d_bv = self ? d_av : d_av + an;
    uint32_t* d_aw = Acc::WEIGHTED ? c->w_sc_ab.as<uint32_t>() : nullptr;
    uint32_t* d_bw = self || !d_aw ? d_aw : d_aw + an;
    uint64_t* d_ao = c->w_sc_off.as<uint64_t>();
    uint64_t* d_bo = self ? d_ao : d_ao + na + 1;
    if (an) HIPCHK(hipMemcpyAsync(d_av, a_values, (size_t)an * 8, hipMemcpyHostToDevice, c->st));
    if (an && d_aw) HIPCHK(hipMemcpyAsync(d_aw, a_abund, (size_t)an * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(d_ao, a_offsets, ((size_t)na + 1) * 8, hipMemcpyHostToDevice, c->st));
    if (!self) {
        if (bn) HIPCHK(hipMemcpyAsync(d_bv, b_values, (size_t)bn * 8, hipMemcpyHostToDevice, c->st));
        if (bn && d_bw) HIPCHK(hipMemcpyAsync(d_bw, b_abund, (size_t)bn * 4, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(d_bo, b_offsets, ((size_t)nb + 1) * 8, hipMemcpyHostToDevice, c->st));
    }
    const int L = lanes ? lanes : auto_lanes(an, na, bn, nb); // one choice for all row blocks
    // the rows of the answer leave in blocks of at most 64 MB (one row when nb alone is wider than that)
    const size_t row_bytes = (size_t)nb * Acc::WIDTH * sizeof(typename Acc::Out);
    size_t rows = std::max<size_t>(1, ((size_t)64 << 20) / row_bytes);
    if (rows > (size_t)na) rows = (size_t)na;
    RKCHK(c->w_out.reserve(rows * row_bytes));
    for (size_t r0 = 0; r0 < (size_t)na; r0 += rows) {
        const int n = (int)std::min(rows, (size_t)na - r0);
        RKCHK(launch_scaled_pairs<Acc>(d_av, d_aw, d_ao + r0, n, an, d_bv, d_bw, d_bo, nb, bn, L, c->w_out.as<typename Acc::Out>(), c->st));
        HIPCHK(hipMemcpyAsync(out + r0 * (size_t)nb * Acc::WIDTH, c->w_out.p, (size_t)n * row_bytes, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return RK_OK;
}

} // namespace

extern "C" int rk_compare_scaled_device(rk_ctx* c, const void* d_a_values, const void* d_a_offsets, int na, uint64_t a_nvalues,
                                        const void* d_b_values, const void* d_b_offsets, int nb, uint64_t b_nvalues, int lanes,
                                        void* d_shared, void* hip_stream) {
    if (!c || !d_a_offsets || !d_b_offsets || !d_shared || (!d_a_values && a_nvalues) || (!d_b_values && b_nvalues)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_pairs_shape(na, nb, lanes));
    RKCHK(set_dev(c));
    return launch_scaled_pairs<PairsPlain>((const uint64_t*)d_a_values, nullptr, (const uint64_t*)d_a_offsets, na, a_nvalues, (const uint64_t*)d_b_values, nullptr,
                                           (const uint64_t*)d_b_offsets, nb, b_nvalues, lanes, (int32_t*)d_shared, (hipStream_t)hip_stream);
}
extern "C" int rk_compare_scaled_abund_device(rk_ctx* c, const void* d_a_values, const void* d_a_abund, const void* d_a_offsets, int na, uint64_t a_nvalues,
                                              const void* d_b_values, const void* d_b_abund, const void* d_b_offsets, int nb, uint64_t b_nvalues, int lanes,
                                              void* d_out4, void* hip_stream) {
    if (!c || !d_a_offsets || !d_b_offsets || !d_out4 || ((!d_a_values || !d_a_abund) && a_nvalues) || ((!d_b_values || !d_b_abund) && b_nvalues))
        return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_pairs_shape(na, nb, lanes));
    RKCHK(set_dev(c));
    return launch_scaled_pairs<PairsWeighted>((const uint64_t*)d_a_values, (const uint32_t*)d_a_abund, (const uint64_t*)d_a_offsets, na, a_nvalues,
                                              (const uint64_t*)d_b_values, (const uint32_t*)d_b_abund, (const uint64_t*)d_b_offsets, nb, b_nvalues, lanes,
                                              (uint64_t*)d_out4, (hipStream_t)hip_stream);
}

extern "C" int rk_compare_scaled(rk_ctx* c, const uint64_t* a_values, const uint64_t* a_offsets, int na, const uint64_t* b_values,
                                 const uint64_t* b_offsets, int nb, int lanes, int32_t* shared) {
    return compare_uploaded<PairsPlain>(c, a_values, nullptr, a_offsets, na, b_values, nullptr, b_offsets, nb, lanes, shared);
}
extern "C" int rk_compare_scaled_abund(rk_ctx* c, const uint64_t* a_values, const uint32_t* a_abund, const uint64_t* a_offsets, int na, const uint64_t* b_values,
                                       const uint32_t* b_abund, const uint64_t* b_offsets, int nb, int lanes, uint64_t* out4) {
    return compare_uploaded<PairsWeighted>(c, a_values, a_abund, a_offsets, na, b_values, b_abund, b_offsets, nb, lanes, out4);
}

extern "C" int rk_abund_row_sums_device(rk_ctx* c, const void* d_abund, const void* d_offsets, int n, uint64_t nvalues, void* d_out2, void* hip_stream) {
    if (!c || !d_offsets || !d_out2 || (!d_abund && nvalues)) return fail(RK_ERR_ARG, "bad arguments");
    if (n < 1) return fail(RK_ERR_ARG, "need at least one sketch, got %d", n);
    RKCHK(set_dev(c));
    return launch_row_sums((const uint32_t*)d_abund, (const uint64_t*)d_offsets, n, nvalues, (uint64_t*)d_out2, (hipStream_t)hip_stream);
}

extern "C" int rk_abund_row_sums(rk_ctx* c, const uint32_t* abund, const uint64_t* offsets, int n, uint64_t* out2) {
    if (!c || !offsets || !out2) return fail(RK_ERR_ARG, "bad arguments");
    if (n < 1) return fail(RK_ERR_ARG, "need at least one sketch, got %d", n);
    RKCHK(check_csr(offsets, n, "", "the sketches", RK_ERR_ARG));
    const uint64_t nv = offsets[n];
    if (nv && !abund) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_abund(abund, offsets[0], nv, "", "the sketches"));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(c->general_mu);
    RKCHK(c->w_sc_ab.reserve((size_t)nv * 4 + 4));
    RKCHK(c->w_sc_off.reserve(((size_t)n + 1) * 8));
    RKCHK(c->w_out.reserve((size_t)n * 16));
    if (nv) HIPCHK(hipMemcpyAsync(c->w_sc_ab.p, abund, (size_t)nv * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->w_sc_off.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->st));
    RKCHK(launch_row_sums(c->w_sc_ab.as<uint32_t>(), c->w_sc_off.as<uint64_t>(), n, nv, c->w_out.as<uint64_t>(), c->st));
    HIPCHK(hipMemcpyAsync(out2, c->w_out.p, (size_t)n * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}
