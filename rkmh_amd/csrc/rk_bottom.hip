// rk_bottom.hip -- the cut of a bottom sample (include/rkmh_amd.h, "BOTTOM SAMPLES"): given a sorted distinct set of (value, count)
// pairs, where do its sketch_size smallest sketch elements end?  Entry j weighs 0 when its count is below min_copies, else 1
// (dedup=distinct) or min(count, sketch_size) (dedup=multiset: a value stands in the sketch once per copy); j* is the first entry at
// which the running sum of the weights reaches sketch_size.  Three launches: k_cut_weights sums the weights of every block of KEEP_BLK
// entries, k_scan_blocks (rk_sets.hpp) scans the block sums, k_cut_find scans inside the one block the crossing falls into.  The
// sample accumulator (rk_sample.hip) calls this behind a fold; rk_bottom_cut is its public form on host arrays.  DESIGN.md section 22.
#include "rk_sets.hpp"

namespace {

__device__ __forceinline__ uint32_t cut_weight(uint32_t count, uint32_t sketch_size, uint32_t min_copies, int distinct) {
    if (count < min_copies) return 0;
    return distinct ? 1u : min(count, sketch_size);
}

// block_sum[b] = the weights of entries [b * KEEP_BLK, (b + 1) * KEEP_BLK) below n, summed: at most 1 024 * 16 384 = 2^24
__global__ __launch_bounds__(KEEP_T) void k_cut_weights(const uint32_t* __restrict__ counts, uint64_t n, uint32_t sketch_size, uint32_t min_copies, int distinct,
                                                        uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t wsum[KEEP_T / 64];
    const uint64_t base = (uint64_t)blockIdx.x * KEEP_BLK;
    uint32_t sum = 0;
    for (int r = 0; r < KEEP_ROUNDS; ++r) {
        const uint64_t t = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
        if (t < n) sum += cut_weight(counts[t], sketch_size, min_copies, distinct);
    }
    for (int d = 32; d > 0; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) block_sum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pre[b] = the weight in front of block b, pre[nblocks] = all of it.  The one block with pre[b] < sketch_size <= pre[b + 1] holds j*:
// every other workgroup leaves whole, before any barrier.  There, round by round in entry order, a wave scans its 64 weights with
// shuffles and the sums of (round, wave) meet in LDS; the one thread whose inclusive sum is the first to reach sketch_size stores
// (j* + 1, values[j*], that sum) to state[0 .. 3) with plain stores.  When no block crosses, state[0] and state[1] keep what the host
// wrote and thread 0 of workgroup 0 stores the whole weight to state[2]: exactly one thread of the grid writes each word.  An entry at
// or behind n weighs nothing, so values[] and counts[] are read below n only; counts that changed between the two kernels, or values
// that do not ascend, give a meaningless cut and nothing else.
__global__ __launch_bounds__(KEEP_T) void k_cut_find(const uint64_t* __restrict__ values, const uint32_t* __restrict__ counts, uint64_t n, uint32_t sketch_size,
                                                     uint32_t min_copies, int distinct, const uint64_t* __restrict__ pre, uint64_t nblocks,
                                                     uint64_t* __restrict__ state) {
    __shared__ uint32_t wsum[KEEP_ROUNDS * (KEEP_T / 64)]; // the weight of (round, wave), in entry order: at most 64 * 16 384 each
    const uint64_t all = pre[nblocks];
    if (blockIdx.x == 0 && threadIdx.x == 0 && all < (uint64_t)sketch_size) state[2] = all;
    const uint64_t before = pre[blockIdx.x];
    if (!(before < (uint64_t)sketch_size && (uint64_t)sketch_size <= pre[blockIdx.x + 1])) return; // (the same in every thread)
    const uint64_t base = (uint64_t)blockIdx.x * KEEP_BLK;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t w[KEEP_ROUNDS], incl[KEEP_ROUNDS];
    for (int r = 0; r < KEEP_ROUNDS; ++r) {
        const uint64_t t = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
        w[r] = t < n ? cut_weight(counts[t], sketch_size, min_copies, distinct) : 0u;
        uint32_t x = w[r];
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)x, d, 64);
            if (lane >= (uint32_t)d) x += y;
        }
        incl[r] = x;
        if (lane == 63) wsum[r * (KEEP_T / 64) + wave] = x;
    }
    __syncthreads();
    uint64_t front = before; // the weight in front of this thread's wave in round r
    for (int r = 0; r < KEEP_ROUNDS; ++r)
        for (uint32_t v = 0; v < KEEP_T / 64; ++v) {
            if (v == wave) {
                const uint64_t upto = front + incl[r];
                if (upto >= (uint64_t)sketch_size && upto - w[r] < (uint64_t)sketch_size) { // (w[r] > 0: an entry below n)
                    const uint64_t t = base + (uint64_t)(r * KEEP_T) + threadIdx.x;
                    state[0] = t + 1;
                    state[1] = values[t];
                    state[2] = upto;
                }
            }
            front += wsum[r * (KEEP_T / 64) + v];
        }
}

} // namespace

namespace rk {
int bottom_cut_device(DevBuf& cnt, DevBuf& pre, const uint64_t* d_values, const uint32_t* d_counts, uint64_t n, uint32_t sketch_size, uint32_t min_copies,
                      bool distinct, uint64_t* d_state, hipStream_t st) {
    HIPCHK(hipMemsetAsync(d_state, 0, 24, st)); // "no cut"
    if (n == 0) return RK_OK;
    const uint64_t nblocks = (n + KEEP_BLK - 1) / KEEP_BLK;
    if (nblocks > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%llu entries are more than one cut takes", (unsigned long long)n);
    RKCHK(cnt.reserve((size_t)(nblocks + 1) * 4));
    RKCHK(pre.reserve((size_t)(nblocks + 1) * 8));
    hipLaunchKernelGGL(k_cut_weights, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, d_counts, n, sketch_size, min_copies, distinct ? 1 : 0, cnt.as<uint32_t>());
    hipLaunchKernelGGL(k_scan_blocks<uint32_t>, dim3(1), dim3(1024), 0, st, cnt.as<uint32_t>(), nblocks, pre.as<uint64_t>());
    hipLaunchKernelGGL(k_cut_find, dim3((uint32_t)nblocks), dim3(KEEP_T), 0, st, d_values, d_counts, n, sketch_size, min_copies, distinct ? 1 : 0,
                       pre.as<uint64_t>(), nblocks, d_state);
    HIPCHK(hipGetLastError());
    return RK_OK;
}
}

extern "C" int rk_bottom_cut(rk_ctx* c, const uint64_t* values, const uint32_t* counts, uint64_t n, int sketch_size, uint64_t min_copies, int distinct,
                             uint64_t* cut_len, uint64_t* threshold) {
    if (!c || !cut_len || !threshold || (n && (!values || !counts))) return fail(RK_ERR_ARG, "rk_bottom_cut: bad arguments");
    if (sketch_size < 1 || sketch_size > RK_MAX_SKETCH) return fail(RK_ERR_ARG, "rk_bottom_cut: sketch size %d outside [1,%d]", sketch_size, RK_MAX_SKETCH);
    if (min_copies < 1 || min_copies > 0xffffffffull) return fail(RK_ERR_ARG, "rk_bottom_cut: min_copies %llu outside [1,2^32-1]", (unsigned long long)min_copies);
    if (n >= ((uint64_t)1 << 31) * KEEP_BLK) return fail(RK_ERR_LIMIT, "rk_bottom_cut: %llu entries are more than one cut takes", (unsigned long long)n);
    *cut_len = 0;
    *threshold = 0;
    if (n == 0) return RK_OK;
    RKCHK(set_dev(c));
    struct Work { DevBuf v, a, cnt, pre, state; ~Work() { for (DevBuf* b : {&v, &a, &cnt, &pre, &state}) b->release(); } } w;
    RKCHK(w.v.reserve((size_t)n * 8));
    RKCHK(w.a.reserve((size_t)n * 4));
    RKCHK(w.state.reserve(32));
    HIPCHK(hipMemcpyAsync(w.v.p, values, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(w.a.p, counts, (size_t)n * 4, hipMemcpyHostToDevice, c->st));
    RKCHK(bottom_cut_device(w.cnt, w.pre, w.v.as<uint64_t>(), w.a.as<uint32_t>(), n, (uint32_t)sketch_size, (uint32_t)min_copies, distinct != 0,
                            w.state.as<uint64_t>(), c->st));
    uint64_t h[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(h, w.state.p, 24, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    if (h[0] > n) return fail(RK_ERR_HIP, "rk_bottom_cut: a cut at %llu of %llu entries", (unsigned long long)h[0], (unsigned long long)n);
    *cut_len = h[0];
    *threshold = h[1];
    return RK_OK;
}
