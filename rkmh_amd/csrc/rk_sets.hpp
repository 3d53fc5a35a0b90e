// rk_sets.hpp -- what the parts that work on sets of scaled sketches (rk_scaled.hip, rk_gather.hip, rk_search.hip, rk_multigather.hip,
// rk_cluster.hip) share: the resident inverted index and the steps of a search on it (defined in rk_search.hip, used by rk_multigather.hip
// and rk_cluster.hip too), rows
// of a CSR side clamped on the device, the lookup in an ascending array, 64-bit shuffles, the order-preserving compaction, and the host
// checks and upload of a CSR side.  Everything in the unnamed namespace has internal linkage: each part compiles its own copy of what it uses.
#pragma once
#include "rk_api_internal.hpp"

// ---- the resident inverted index (rk_search.hip builds and searches it; rk_multigather.hip gathers through it) -----------------
struct rk_scaled_index {
    rk_ctx* ctx = nullptr; // compared, never followed: the index may outlive its context
    int device = 0;
    uint32_t nref = 0, longest = 0;
    uint64_t npost = 0, nkeys = 0;
    DevBuf keys, post_off, post;
    DevBuf w_cnt, w_pre, w_qv, w_qo, w_qmin, w_hits; // searches: per-workgroup hit counts, their scan, an uploaded query batch, its hits
    DevBuf w_cl; // cluster (rk_cluster.hip): the flag word of the rounds, then the host entry's parent[]
    DevBuf w_mg, w_mg_io, w_mg_out; // multigather: the state of one call (candidates, counts, key positions, alive bytes, rows); the host entry's row offsets and abundances; its packed answer
    std::mutex mu;
};
namespace rk {
// The steps of a search (rk_search.hip), for the entries there and for multigather; `who` begins the messages; the caller holds ix->mu.
// search_count: pass 1 and the scan on stream st -> *total (synchronises st); ix->w_pre then holds, at entry q * nblk, how many hits
// lie before query q's.  search_emit: pass 2, the hits in (query, reference) order as far as cap_hits.
int check_search_shape(const rk_ctx* c, const rk_scaled_index* ix, int64_t nq, int min_shared, uint64_t* nwg, uint32_t* nblk, const char* who);
int search_count(rk_scaled_index* ix, const uint64_t* d_qv, const uint64_t* d_qo, uint32_t nq, uint64_t q_nvalues, int min_shared, const int32_t* d_qmin,
                 uint32_t nblk, uint32_t nwg, hipStream_t st, uint64_t* total, const char* who);
int search_emit(rk_scaled_index* ix, const uint64_t* d_qv, const uint64_t* d_qo, uint32_t nq, uint64_t q_nvalues, int min_shared, const int32_t* d_qmin,
                uint32_t nblk, uint32_t nwg, hipStream_t st, int32_t* d_hits, uint64_t cap_hits);
}

namespace {

// ---- device helpers -------------------------------------------------------------------------------------------------------
// row r of a CSR side, clamped to [0, nvalues] and to 2^31 - 1 values: whatever off[] holds, r0 <= r1 <= nvalues and r1 - r0 < 2^31
__device__ __forceinline__ void clamped_row(const uint64_t* __restrict__ off, uint64_t r, uint64_t nvalues, uint64_t& r0, uint64_t& r1) {
    r0 = min(off[r], nvalues);
    r1 = max(min(off[r + 1], nvalues), r0);
    r1 = r0 + min(r1 - r0, (uint64_t)0x7fffffffu);
}

// first index in [lo, hi) whose element is not below x (hi when there is none); a[] ascends there; one halving per bit of hi - lo
template <typename T, typename I>
__device__ __forceinline__ I first_not_below(const T* __restrict__ a, I lo, I hi, T x) {
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// min(a + b, 2^64 - 1).  Associative and commutative on non-negative numbers: the result is min(true sum, 2^64 - 1) in any order.
__device__ __forceinline__ uint64_t sat_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}
// a 64-bit value from lane src, or from lane (self ^ d), as two halves
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

// ---- the compaction: an order-preserving selection from a flat array ---------------------------------------------------------
//   KEEP_HASH      v = a chunk's window hashes:            element t stays when 0 < v[t] <= max_hash
//   KEEP_FIRST     v = the kept values, sorted by segment: element t stays when it is the first of its value in its segment
//   KEEP_RUN       v = sorted values, no segments:         element t stays when it is the first of its value
// Because the order is kept, a segment's values stay together; where a segment begins in the output is the number of elements kept
// before its first one (k_keep_bounds).  Count first (k_keep_count), scan the block counts (k_scan_blocks), size the output, scatter
// (keep_scatter_block): no atomics, positions come from wave ballots.
enum { KEEP_HASH = 0, KEEP_FIRST = 1, KEEP_RUN = 2 };
constexpr int KEEP_T = 256, KEEP_ROUNDS = 4, KEEP_BLK = KEEP_T * KEEP_ROUNDS; // elements of one workgroup: round r, thread t -> element r * 256 + t

// does a segment begin at element t?  off[0 .. nseg] ascending (equal entries: empty segments); at most 33 halvings
__device__ __forceinline__ bool segment_starts_at(const uint64_t* __restrict__ off, uint32_t nseg, uint64_t t) {
    const uint32_t s = first_not_below(off, 0u, nseg + 1, t);
    return s <= nseg && off[s] == t;
}
template <int MODE>
__device__ __forceinline__ bool keeps(const uint64_t* __restrict__ v, uint64_t t, uint64_t max_hash, const uint64_t* __restrict__ off, uint32_t nseg) {
    const uint64_t x = v[t];
    if (MODE == KEEP_HASH) return x != 0 && x <= max_hash;
    if (t == 0 || v[t - 1] != x) return true;
    return MODE == KEEP_FIRST && segment_starts_at(off, nseg, t); // equal to the element before it: stays only as the first of the next segment
}

template <int MODE>
__global__ __launch_bounds__(KEEP_T) void k_keep_count(const uint64_t* __restrict__ v, uint64_t n, uint64_t max_hash, const uint64_t* __restrict__ off,
                                                       uint32_t nseg, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t wsum[KEEP_T / 64];
    const uint64_t base = (uint64_t)blockIdx.x * KEEP_BLK;
    uint32_t cnt = 0; // wave-uniform
    for (int r = 0; r < KEEP_ROUNDS; ++r) {
        const uint64_t t = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
        cnt += (uint32_t)__popcll(__ballot(t < n && keeps<MODE>(v, t, max_hash, off, nseg)));
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pre[b] = block_count[0] + ... + block_count[b - 1] for b in [0, nblocks]; one workgroup of 1024, each thread a contiguous span.
// (A template so that a translation unit that scans nothing holds no copy of it; Count is uint32_t.)
template <typename Count>
__global__ __launch_bounds__(1024) void k_scan_blocks(const Count* __restrict__ block_count, uint64_t nblocks, uint64_t* __restrict__ pre) {
    __shared__ uint64_t part[1024];
    const uint64_t per = (nblocks + 1023) / 1024;
    const uint64_t b0 = min((uint64_t)threadIdx.x * per, nblocks), b1 = min(b0 + per, nblocks);
    uint64_t sum = 0;
    for (uint64_t b = b0; b < b1; ++b) sum += block_count[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (int i = 0; i < 1024; ++i) { const uint64_t s = part[i]; part[i] = acc; acc += s; }
        pre[nblocks] = acc;
    }
    __syncthreads();
    uint64_t acc = part[threadIdx.x];
    for (uint64_t b = b0; b < b1; ++b) { pre[b] = acc; acc += block_count[b]; }
}

// out_off[s] = elements kept before element off[s], for s in [0, nseg]: one wave per boundary counts the part of its block before it
template <int MODE>
__global__ __launch_bounds__(KEEP_T) void k_keep_bounds(const uint64_t* __restrict__ v, uint64_t n, uint64_t max_hash, const uint64_t* __restrict__ off,
                                                        uint32_t nseg, const uint64_t* __restrict__ pre, uint64_t* __restrict__ out_off) {
    const uint32_t s = blockIdx.x * (KEEP_T / 64) + (threadIdx.x >> 6);
    if (s > nseg) return; // whole waves leave
    const uint64_t p = min(off[s], n);
    const uint64_t blk = p / KEEP_BLK; // <= number of blocks; pre has an entry for it
    uint64_t cnt = 0;
    for (uint64_t t0 = blk * KEEP_BLK; t0 < p; t0 += 64) { // at most 16 rounds
        const uint64_t t = t0 + (threadIdx.x & 63);
        cnt += (uint64_t)__popcll(__ballot(t < p && keeps<MODE>(v, t, max_hash, off, nseg)));
    }
    if ((threadIdx.x & 63) == 0) out_off[s] = pre[blk] + cnt;
}

// the scatter of one workgroup; SRC: the index t of every kept element also goes to src[], parallel to out[]
template <int MODE, bool SRC>
__device__ __forceinline__ void keep_scatter_block(const uint64_t* __restrict__ v, uint64_t n, uint64_t max_hash, const uint64_t* __restrict__ off,
                                                   uint32_t nseg, const uint64_t* __restrict__ pre, uint64_t* __restrict__ out, uint64_t* __restrict__ src,
                                                   uint64_t out_cap) {
    __shared__ uint32_t wcnt[KEEP_ROUNDS * (KEEP_T / 64)]; // kept by (round, wave), in element order
    const uint64_t base = (uint64_t)blockIdx.x * KEEP_BLK;
    const uint32_t wave = threadIdx.x >> 6;
    uint64_t x[KEEP_ROUNDS];
    uint32_t rank[KEEP_ROUNDS];
    bool keep[KEEP_ROUNDS];
    for (int r = 0; r < KEEP_ROUNDS; ++r) {
        const uint64_t t = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
        keep[r] = t < n && keeps<MODE>(v, t, max_hash, off, nseg);
        x[r] = t < n ? v[t] : 0;
        const uint64_t bal = __ballot(keep[r]);
        rank[r] = lanes_below(bal);
        if ((threadIdx.x & 63) == 0) wcnt[r * (KEEP_T / 64) + wave] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    const uint64_t first = pre[blockIdx.x];
    uint32_t before = 0;
    for (int r = 0; r < KEEP_ROUNDS; ++r)
        for (uint32_t w = 0; w < KEEP_T / 64; ++w) {
            if (w == wave && keep[r]) {
                const uint64_t at = first + before + rank[r];
                if (at < out_cap) { // (always: out holds pre[nblocks] values)
                    out[at] = x[r];
                    if (SRC) src[at] = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
                }
            }
            before += wcnt[r * (KEEP_T / 64) + w];
        }
}
template <int MODE>
__global__ __launch_bounds__(KEEP_T) void k_keep_scatter(const uint64_t* __restrict__ v, uint64_t n, uint64_t max_hash, const uint64_t* __restrict__ off,
                                                         uint32_t nseg, const uint64_t* __restrict__ pre, uint64_t* __restrict__ out, uint64_t out_cap) {
    keep_scatter_block<MODE, false>(v, n, max_hash, off, nseg, pre, out, nullptr, out_cap);
}

// Count and scan on stream st, in the caller's scratch: cnt takes the block counts, pre their scan (pre[number of blocks]: how many
// elements stay).  With segments (every mode but KEEP_RUN) d_out_off takes where each of the nseg begins in the output, and the end.
template <int MODE>
int keep_counts(DevBuf& cnt, DevBuf& pre, const uint64_t* v, uint64_t n, uint64_t max_hash, const uint64_t* d_off, uint32_t nseg, uint64_t* d_out_off,
                hipStream_t st) {
    const uint64_t nblocks = (n + KEEP_BLK - 1) / KEEP_BLK;
    if (nblocks > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%llu hashes are more than one compaction takes", (unsigned long long)n);
    RKCHK(cnt.reserve((size_t)(nblocks + 1) * 4));
    RKCHK(pre.reserve((size_t)(nblocks + 1) * 8));
    if (nblocks) hipLaunchKernelGGL(k_keep_count<MODE>, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, v, n, max_hash, d_off, nseg, cnt.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_blocks<uint32_t>, dim3(1), dim3(1024), 0, st, cnt.as<uint32_t>(), nblocks, pre.as<uint64_t>());
    if constexpr (MODE != KEEP_RUN)
        hipLaunchKernelGGL(k_keep_bounds<MODE>, dim3((nseg + 1 + KEEP_T / 64 - 1) / (KEEP_T / 64)), dim3(KEEP_T), 0, st, v, n, max_hash, d_off, nseg,
                           pre.as<uint64_t>(), d_out_off);
    HIPCHK(hipGetLastError());
    return RK_OK;
}
template <int MODE>
int keep_scatter(DevBuf& pre, const uint64_t* v, uint64_t n, uint64_t max_hash, const uint64_t* d_off, uint32_t nseg, uint64_t* out, uint64_t out_cap,
                 hipStream_t st) {
    const uint64_t nblocks = (n + KEEP_BLK - 1) / KEEP_BLK;
    if (!nblocks) return RK_OK;
    hipLaunchKernelGGL(k_keep_scatter<MODE>, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, v, n, max_hash, d_off, nseg, pre.as<uint64_t>(), out, out_cap);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

// ---- host helpers ---------------------------------------------------------------------------------------------------------
// workgroups of `waves_per_workgroup` waves for that many waves; the kernels stride beyond 2^16 of them
inline uint32_t wave_grid(uint64_t nwaves, uint32_t waves_per_workgroup) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((nwaves + waves_per_workgroup - 1) / waves_per_workgroup, 1), 1u << 16);
}

// the offsets off[0 .. n] of a CSR side ascend (RK_ERR_ARG) and no row holds 2^31 values or more (long_row_code)
inline int check_csr(const uint64_t* off, int64_t n, const char* prefix, const char* side, int long_row_code) {
    for (int64_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return fail(RK_ERR_ARG, "%soffsets of %s decrease at sketch %lld", prefix, side, (long long)i);
        if (off[i + 1] - off[i] > 0x7fffffffull) return fail(long_row_code, "%ssketch %lld of %s holds 2^31 values or more", prefix, (long long)i, side);
    }
    return RK_OK;
}
// every abundance w[begin .. end) is at least 1
inline int check_abund(const uint32_t* w, uint64_t begin, uint64_t end, const char* prefix, const char* side) {
    for (uint64_t t = begin; t < end; ++t)
        if (w[t] == 0) return fail(RK_ERR_ARG, "%sabundance 0 at value %llu of %s", prefix, (unsigned long long)t, side);
    return RK_OK;
}
// Uploads the rows [0, n) of a checked CSR side on stream st: the off[n] - off[0] values they cover to d_values, the offsets less
// off[0] to d_off.  The offsets leave from `rebased`, pageable host memory: it lives until st is synchronised.
inline int upload_csr(const uint64_t* values, const uint64_t* off, int64_t n, uint64_t* d_values, uint64_t* d_off, std::vector<uint64_t>& rebased,
                      hipStream_t st) {
    rebased.resize((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) rebased[(size_t)i] = off[i] - off[0];
    if (rebased[(size_t)n]) HIPCHK(hipMemcpyAsync(d_values, values + off[0], (size_t)rebased[(size_t)n] * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, rebased.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
    return RK_OK;
}

} // namespace
