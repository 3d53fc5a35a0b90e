// rk_pairs.hip -- all-pairs sketch comparison (include/rkmh_amd.h, "SKETCH COMPARISON"): k_sketch_pairs and the two entry points on
// top of it.  What Mash's `dist` and sourmash's `compare` answer; the reference has no analogue (its only sketch-to-sketch call is
// hash_intersection_size for one pair, src/rkmh.cpp:869).  The host-only half (rk_merge_sketches, rk_mash_distance) is
// rk_pairs_host.cpp; semantics, tile geometry and measurements: DESIGN.md section 10.
#include "rk_api_internal.hpp"

namespace {

constexpr size_t PAIRS_LDS = 158 * 1024; // for the rows; gfx950 gives one workgroup 160 KB, the lengths below take a little of it
constexpr int PAIRS_MAX_T = 16;          // most rows of one side in a tile (16 x 16 pairs = 256 lanes)

// The four counts of one pair: a two-pointer merge of A[0, la) and B[0, lb), both ascending, both sides advancing on equality.
//   shared           steps that take from both sides                  = sum over values of min(mult_a, mult_b)
//   shared_distinct  such steps whose value is new                    = |D(a) & D(b)|  (the first step at a value takes from every
//                                                                       side that holds it: all smaller values are consumed by then)
//   denom, common    new values seen / new values seen on both sides, both frozen once S new values were seen
// 0 is never a value (it is the padding of short sketches): a step at 0 advances and counts nothing.
// At most la + lb steps, each advances at least one index below its length, and every read is at an index of [0, max(len - 1, 0)] of a
// row of S >= 1 values: unsorted rows give meaningless counts and nothing worse.
template <typename PA, typename PB>
__device__ __forceinline__ int4 merge_counts(PA A, int la, PB B, int lb, int S) {
    int shared = 0, sdist = 0, common = 0, denom = 0;
    int i = 0, j = 0;
    const int ea = max(la - 1, 0), eb = max(lb - 1, 0); // the last index read: a finished (or empty) side re-reads it and the value is ignored
    uint64_t va = A[0], vb = B[0], prev = 0;
    const int steps = la + lb;
    for (int t = 0; t < steps; ++t) {
        const bool ha = i < la, hb = j < lb;
        if (!(ha && hb) && (denom >= S || !(ha || hb))) break; // one side is done: only denom can still move
        const bool ta = ha && (!hb || va <= vb), tb = hb && (!ha || vb <= va); // 64-bit unsigned compares
        const uint64_t v = ta ? va : vb;
        const bool fresh = v != prev && v != 0, both = ta && tb;
        prev = v;
        shared += (both && v != 0) ? 1 : 0;
        sdist += (both && fresh) ? 1 : 0;
        const bool counts = fresh && denom < S;
        denom += counts ? 1 : 0;
        common += (counts && both) ? 1 : 0;
        i += ta ? 1 : 0;
        j += tb ? 1 : 0;
        va = A[min(i, ea)]; // both reads issue together: one LDS latency per step, whichever side advanced
        vb = B[min(j, eb)];
    }
    return make_int4(shared, sdist, common, denom);
}

// One workgroup per TA x TB tile of pairs, one lane per pair.  The tile's TA rows of `a` are staged in LDS (the first len values of
// each, `stride` uint64 apart: odd, so that lanes at the same index of different rows meet different banks), its TB rows of `b`
// beside them -- or, B_GLOBAL, left in global memory where a sketch is too large for both sides to fit (pairs_geometry).
// lens are clamped to [0, S] here; rows past na / nb have no lane.  The only global writes: one int4 per pair.
template <bool B_GLOBAL>
__global__ __launch_bounds__(256) void k_sketch_pairs(const uint64_t* __restrict__ a, const int32_t* __restrict__ alens, int na,
                                                      const uint64_t* __restrict__ b, const int32_t* __restrict__ blens, int nb, int S,
                                                      int stride, int TA, int TB, uint32_t tiles_b, int4* __restrict__ out) {
    extern __shared__ uint64_t lds_rows[];
    __shared__ int lens[4 + 256]; // the tile's rows: TA + TB <= 32 staged, at most 4 + 64, 2 + 128 or 1 + 256 with b in global memory
    const int a0 = (int)(blockIdx.x / tiles_b) * TA, b0 = (int)(blockIdx.x % tiles_b) * TB;
    const int nta = min(TA, na - a0), ntb = min(TB, nb - b0); // rows of this tile: >= 1 by the grid's size
    for (int r = threadIdx.x; r < nta + ntb; r += blockDim.x) {
        const int l = r < nta ? alens[a0 + r] : blens[b0 + r - nta];
        lens[r] = min(max(l, 0), S);
    }
    __syncthreads();
    const int staged = B_GLOBAL ? nta : nta + ntb;
    for (int r = 0; r < staged; ++r) {
        const uint64_t* src = r < nta ? a + (size_t)(a0 + r) * (size_t)S : b + (size_t)(b0 + r - nta) * (size_t)S;
        uint64_t* dst = lds_rows + (size_t)r * (size_t)stride;
        const int l = lens[r];
        for (int x = threadIdx.x; x < l; x += blockDim.x) dst[x] = src[x];
    }
    __syncthreads();
    const int p = threadIdx.x, ia = p / TB, ib = p % TB;
    if (ia >= nta || ib >= ntb) return;
    const uint64_t* A = lds_rows + (size_t)ia * (size_t)stride;
    int4 r;
    if (B_GLOBAL) r = merge_counts(A, lens[ia], b + (size_t)(b0 + ib) * (size_t)S, lens[nta + ib], S);
    else r = merge_counts(A, lens[ia], lds_rows + (size_t)(nta + ib) * (size_t)stride, lens[nta + ib], S);
    out[(size_t)(a0 + ia) * (size_t)nb + (size_t)(b0 + ib)] = r;
}

// Tile geometry as a function of the sketch size alone (DESIGN.md section 10 has the table).  rows = sketches of `stride` uint64
// that fit the LDS.  From 8 rows up both sides are staged: TB = rows / 2, TA = the rest, 16 at most.  Below that a tile of
// all-LDS rows would hold 9 pairs or fewer, so only `a` is staged (1, 2 or 4 rows) and 256 lanes read their `b` row from global memory.
struct PairsGeometry { int stride, ta, tb, threads; bool b_global; size_t lds; };
PairsGeometry pairs_geometry(int S) {
    PairsGeometry g;
    g.stride = S | 1;
    const int rows = (int)(PAIRS_LDS / ((size_t)g.stride * 8));
    g.b_global = rows < 8;
    if (!g.b_global) {
        g.tb = std::min(PAIRS_MAX_T, rows / 2);
        g.ta = std::min(PAIRS_MAX_T, rows - g.tb);
        g.threads = (g.ta * g.tb + 63) / 64 * 64;
        g.lds = (size_t)(g.ta + g.tb) * (size_t)g.stride * 8;
    } else {
        g.ta = rows >= 4 ? 4 : rows >= 2 ? 2 : 1;
        g.tb = 256 / g.ta;
        g.threads = 256;
        g.lds = (size_t)g.ta * (size_t)g.stride * 8;
    }
    return g;
}

// Dynamic LDS above 64 KB has to be granted to a kernel: once per device and instantiation, for all of the CU's LDS.
int allow_large_lds(bool b_global) {
    static std::mutex mu;
    static std::vector<int> done[2]; // devices on which the instantiation has its grant
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    std::vector<int>& d = done[b_global ? 1 : 0];
    if (std::find(d.begin(), d.end(), dev) != d.end()) return RK_OK;
    const void* fn = b_global ? reinterpret_cast<const void*>(k_sketch_pairs<true>) : reinterpret_cast<const void*>(k_sketch_pairs<false>);
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(160 * 1024 - sizeof(int) * (4 + 256))));
    d.push_back(dev);
    return RK_OK;
}

// rows [0, na) of d_a against rows [0, nb) of d_b -> d_out4[na * nb * 4], on st; nothing is checked here but the grid's size
int launch_pairs(const uint64_t* d_a, const int32_t* d_alens, int na, const uint64_t* d_b, const int32_t* d_blens, int nb, int S,
                 int32_t* d_out4, hipStream_t st) {
    const PairsGeometry g = pairs_geometry(S);
    const uint64_t tiles_a = ((uint64_t)na + g.ta - 1) / g.ta, tiles_b = ((uint64_t)nb + g.tb - 1) / g.tb;
    if (tiles_a * tiles_b > 0x7fffffffull) return fail(RK_ERR_LIMIT, "%d x %d sketches are more tiles than one launch takes", na, nb);
    if (g.lds > 64 * 1024) RKCHK(allow_large_lds(g.b_global));
    const dim3 grid((uint32_t)(tiles_a * tiles_b)), block((uint32_t)g.threads);
    if (g.b_global)
        hipLaunchKernelGGL(k_sketch_pairs<true>, grid, block, g.lds, st, d_a, d_alens, na, d_b, d_blens, nb, S, g.stride, g.ta, g.tb, (uint32_t)tiles_b, (int4*)d_out4);
    else
        hipLaunchKernelGGL(k_sketch_pairs<false>, grid, block, g.lds, st, d_a, d_alens, na, d_b, d_blens, nb, S, g.stride, g.ta, g.tb, (uint32_t)tiles_b, (int4*)d_out4);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

int check_shape(int na, int nb, int S) {
    if (S < 1 || S > RK_MAX_SKETCH) return fail(RK_ERR_ARG, "sketch size %d outside [1,%d]", S, RK_MAX_SKETCH);
    if (na < 1 || nb < 1) return fail(RK_ERR_ARG, "need at least one sketch on each side, got %d x %d", na, nb);
    return RK_OK;
}

} // namespace

extern "C" int rk_compare_sketches_device(rk_ctx* c, const void* d_a, const void* d_alens, int na, const void* d_b, const void* d_blens, int nb,
                                          int S, void* d_out4, void* hip_stream) {
    if (!c || !d_a || !d_alens || !d_b || !d_blens || !d_out4) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_shape(na, nb, S));
    RKCHK(set_dev(c));
    return launch_pairs((const uint64_t*)d_a, (const int32_t*)d_alens, na, (const uint64_t*)d_b, (const int32_t*)d_blens, nb, S, (int32_t*)d_out4,
                        (hipStream_t)hip_stream);
}

extern "C" int rk_compare_sketches(rk_ctx* c, const uint64_t* a, const int32_t* alens, int na, const uint64_t* b, const int32_t* blens, int nb,
                                   int S, int32_t* out4) {
    if (!c || !a || !alens || !b || !blens || !out4) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_shape(na, nb, S));
    for (int i = 0; i < na; ++i) if (alens[i] < 0 || alens[i] > S) return fail(RK_ERR_ARG, "length %d of sketch %d (a) outside [0,%d]", alens[i], i, S);
    for (int i = 0; i < nb; ++i) if (blens[i] < 0 || blens[i] > S) return fail(RK_ERR_ARG, "length %d of sketch %d (b) outside [0,%d]", blens[i], i, S);
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(c->general_mu); // the general path's work buffers serve here too
    const bool self = a == b && alens == blens && na == nb;
    const size_t abytes = (size_t)na * (size_t)S * 8, bbytes = self ? 0 : (size_t)nb * (size_t)S * 8;
    RKCHK(c->w_sk.reserve(abytes + bbytes));
    RKCHK(c->w_lens.reserve(((size_t)na + (size_t)nb) * 4));
    uint64_t* d_a = c->w_sk.as<uint64_t>();
    uint64_t* d_b = self ? d_a : d_a + (size_t)na * (size_t)S;
    int32_t* d_al = c->w_lens.as<int32_t>();
    int32_t* d_bl = self ? d_al : d_al + na;
    HIPCHK(hipMemcpyAsync(d_a, a, abytes, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(d_al, alens, (size_t)na * 4, hipMemcpyHostToDevice, c->st));
    if (!self) {
        HIPCHK(hipMemcpyAsync(d_b, b, bbytes, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(d_bl, blens, (size_t)nb * 4, hipMemcpyHostToDevice, c->st));
    }
    // the rows of the answer leave in blocks of at most 64 MB (whole tiles of `a` rows; one tile row when nb alone is wider than that)
    const PairsGeometry g = pairs_geometry(S);
    const size_t row_bytes = (size_t)nb * 16;
    size_t rows = ((size_t)64 << 20) / row_bytes / (size_t)g.ta * (size_t)g.ta;
    if (rows < (size_t)g.ta) rows = (size_t)g.ta;
    if (rows > (size_t)na) rows = (size_t)na;
    RKCHK(c->w_out.reserve(rows * row_bytes));
    for (size_t r0 = 0; r0 < (size_t)na; r0 += rows) {
        const int n = (int)std::min(rows, (size_t)na - r0);
        RKCHK(launch_pairs(d_a + r0 * (size_t)S, d_al + r0, n, d_b, d_bl, nb, S, c->w_out.as<int32_t>(), c->st));
        HIPCHK(hipMemcpyAsync(out4 + r0 * (size_t)nb * 4, c->w_out.p, (size_t)n * row_bytes, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
    }
    return RK_OK;
}
