// rk_cluster.hip -- cluster (include/rkmh_amd.h, "CLUSTER"): the single-linkage clusters of a collection of scaled sketches from the
// hits of a search, by hook and compress on parent[n]; and the self-search of a collection against its own inverted index, block by
// block, whose hits never leave the device.  The host-only form is rk_cluster_hits_host (rk_cluster_host.cpp); the argument for the
// algorithm, the blocking and the measurements: DESIGN.md section 23.
#include "rk_sets.hpp"

namespace {

constexpr int CL_T = 256;               // threads of a workgroup of every kernel here
constexpr uint32_t CL_GRID_CAP = 2048;  // workgroups of one launch at the most: the kernels stride beyond CL_GRID_CAP * CL_T elements

inline uint32_t cl_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + CL_T - 1) / CL_T, 1), CL_GRID_CAP); }

__global__ __launch_bounds__(CL_T) void k_cluster_init(int32_t* __restrict__ parent, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * CL_T + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CL_T) parent[i] = (int32_t)i;
}

// Lanes stride the hits.  Hit h names u = query + qbase (the hits of a block of queries count from the block's first) and v = ref; both
// are checked against n before anything is indexed with them, the lengths are those of the clamped rows, the link test is the header's,
// in signed 64 bits.  pu and pv are checked against n as well (they are ours, and always are).  A wave in which some lane linked
// raises *flag to `round`; the host compares.
__global__ __launch_bounds__(CL_T) void k_cluster_hook(const int32_t* __restrict__ hits, uint64_t nhits, int64_t qbase, const uint64_t* __restrict__ off,
                                                       uint32_t n, uint64_t nvalues, int measure, uint32_t min_ppm, int32_t* parent, uint32_t* flag,
                                                       uint32_t round) {
    bool linked = false;
    for (uint64_t h = (uint64_t)blockIdx.x * CL_T + threadIdx.x; h < nhits; h += (uint64_t)gridDim.x * CL_T) {
        const int32_t* __restrict__ t = hits + h * 3;
        const int64_t u = (int64_t)t[0] + qbase, v = t[1], shared = t[2];
        if (u < 0 || v < 0 || u >= (int64_t)n || v >= (int64_t)n || u == v || shared < 1) continue;
        uint64_t a0, a1, b0, b1;
        clamped_row(off, (uint64_t)u, nvalues, a0, a1);
        clamped_row(off, (uint64_t)v, nvalues, b0, b1);
        const int64_t lu = (int64_t)(a1 - a0), lv = (int64_t)(b1 - b0); // each below 2^31
        const int64_t denom = measure == RK_CLUSTER_JACCARD ? lu + lv - shared : min(lu, lv);
        if (shared * 1000000 < (int64_t)min_ppm * denom) continue;
        const int32_t pu = parent[u], pv = parent[v];
        if (pu == pv || (uint32_t)pu >= n || (uint32_t)pv >= n) continue;
        atomicMin(&parent[max(pu, pv)], min(pu, pv));
        linked = true;
    }
    if (__any(linked) && (threadIdx.x & 63) == 0) atomicMax(flag, round);
}

// Every node repeats parent[i] = parent[parent[i]] until its parent is a root.  A value read is an ancestor, maybe an old one; it is
// followed only while it is a smaller index inside [0, n), so the walk ends whatever parent[] holds.  Roots are not written.
__global__ __launch_bounds__(CL_T) void k_cluster_compress(int32_t* parent, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * CL_T + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CL_T) {
        int32_t p = parent[i];
        if ((uint32_t)p >= n) continue;
        for (;;) {
            const int32_t g = parent[p];
            if (g >= p || g < 0) break; // p is a root
            p = g;
            parent[i] = p;
        }
    }
}

// pre[w] -= delta for the w < count entries of a search's scan, modulo 2^64: search_emit then writes the hits [delta, delta + cap_hits)
// of the block at [0, cap_hits) -- a hit before them lands at 2^64 - something, one after them at cap_hits or beyond, and both fail
// the kernel's own test against cap_hits.
__global__ __launch_bounds__(CL_T) void k_cluster_shift(uint64_t* __restrict__ pre, uint64_t count, uint64_t delta) {
    for (uint64_t w = (uint64_t)blockIdx.x * CL_T + threadIdx.x; w < count; w += (uint64_t)gridDim.x * CL_T) pre[w] -= delta;
}

// The state of one clustering on the device: parent[n], the flag word, the number of hook launches so far (what the flag is raised to).
struct Forest {
    int32_t* parent = nullptr;
    uint32_t* flag = nullptr;
    uint32_t n = 0, rounds = 0;
    const uint64_t* off = nullptr; // the collection's CSR offsets, n + 1, resident
    uint64_t nvalues = 0;
    int measure = 0;
    uint32_t min_ppm = 0;
};

int forest_init(Forest& f, hipStream_t st) {
    HIPCHK(hipMemsetAsync(f.flag, 0, 4, st));
    hipLaunchKernelGGL(k_cluster_init, dim3(cl_grid(f.n)), dim3(CL_T), 0, st, f.parent, f.n);
    HIPCHK(hipGetLastError());
    f.rounds = 0;
    return RK_OK;
}

// hook; while the hook changed something: compress, hook.  Synchronises st once per hook.  On return every tree is a star again.
int forest_hook(Forest& f, const int32_t* d_hits, uint64_t nhits, int64_t qbase, hipStream_t st) {
    if (!nhits) return RK_OK;
    for (;;) {
        ++f.rounds;
        hipLaunchKernelGGL(k_cluster_hook, dim3(cl_grid(nhits)), dim3(CL_T), 0, st, d_hits, nhits, qbase, f.off, f.n, f.nvalues, f.measure, f.min_ppm,
                           f.parent, f.flag, f.rounds);
        HIPCHK(hipGetLastError());
        uint32_t seen = 0;
        HIPCHK(hipMemcpyAsync(&seen, f.flag, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (seen != f.rounds) return RK_OK;
        hipLaunchKernelGGL(k_cluster_compress, dim3(cl_grid(f.n)), dim3(CL_T), 0, st, f.parent, f.n);
        HIPCHK(hipGetLastError());
    }
}

int check_cluster_shape(const char* who, int64_t n, int measure, uint32_t min_ppm) {
    if (n < 1) return fail(RK_ERR_ARG, "%s: need at least one sketch, got %lld", who, (long long)n);
    if (n > 0x7fffffffll) return fail(RK_ERR_LIMIT, "%s: %lld sketches are more than 2^31-1", who, (long long)n);
    if (measure != RK_CLUSTER_JACCARD && measure != RK_CLUSTER_MAX_CONTAINMENT) return fail(RK_ERR_ARG, "%s: measure %d is not defined", who, measure);
    if (min_ppm > 1000000u) return fail(RK_ERR_ARG, "%s: min_ppm %u is above 1000000", who, min_ppm);
    return RK_OK;
}
int check_self_shape(const rk_ctx* c, const rk_scaled_index* ix, int64_t nref, int min_shared, int measure, uint32_t min_ppm) {
    RKCHK(check_cluster_shape("cluster", nref, measure, min_ppm));
    if (ix->ctx != c) return fail(RK_ERR_ARG, "cluster: the index was made on another context");
    if (min_shared < 1) return fail(RK_ERR_ARG, "cluster: min_shared %d is below 1", min_shared);
    if ((uint64_t)nref != ix->nref) return fail(RK_ERR_ARG, "cluster: %lld sketches, but the index holds %u", (long long)nref, ix->nref);
    return RK_OK;
}

constexpr size_t CL_FLAG_BYTES = 256; // the flag word at the head of w_cl; the host entry's parent[] follows it

// The collection against its own index, block by block, on stream st; the caller holds ix->mu, f is laid out and f.flag lies in
// ix->w_cl.  Never more than cap hits are resident.  A block: search_count gives its total; above cap it is halved, down to one query,
// whose hits go through in pieces of cap (k_cluster_shift); what fits is emitted and hooked to its fixpoint before the next block's
// hits take its place.  After a block that fills at most half of cap the next one is twice as long.
int cluster_self(rk_scaled_index* ix, const uint64_t* d_v, const uint64_t* d_o, int min_shared, uint64_t cap, Forest& f, hipStream_t st) {
    const uint32_t n = f.n, nblk = (ix->nref + RK_SEARCH_REF_BLOCK - 1) / RK_SEARCH_REF_BLOCK;
    const uint32_t longest = std::max<uint32_t>(0xffffffu / nblk, 1); // queries of one search launch at the most (nblk <= 2^18)
    RKCHK(forest_init(f, st));
    uint32_t want = longest;
    for (uint32_t q0 = 0; q0 < n;) {
        const uint32_t nq = std::min(want, n - q0), nwg = nq * nblk;
        uint64_t total = 0;
        RKCHK(search_count(ix, d_v, d_o + q0, nq, f.nvalues, min_shared, nullptr, nblk, nwg, st, &total, "cluster"));
        if (total > cap && nq > 1) { want = nq / 2; continue; }
        for (uint64_t first = 0; first < total; first += cap) {
            const uint64_t piece = std::min(cap, total - first);
            RKCHK(ix->w_hits.reserve((size_t)piece * sizeof(rk_search_hit)));
            if (first) {
                hipLaunchKernelGGL(k_cluster_shift, dim3(cl_grid((uint64_t)nwg + 1)), dim3(CL_T), 0, st, ix->w_pre.as<uint64_t>(), (uint64_t)nwg + 1, cap);
                HIPCHK(hipGetLastError());
            }
            RKCHK(search_emit(ix, d_v, d_o + q0, nq, f.nvalues, min_shared, nullptr, nblk, nwg, st, ix->w_hits.as<int32_t>(), piece));
            RKCHK(forest_hook(f, ix->w_hits.as<int32_t>(), piece, (int64_t)q0, st));
        }
        q0 += nq;
        if (total <= cap / 2) want = (uint32_t)std::min<uint64_t>((uint64_t)nq * 2, longest);
    }
    HIPCHK(hipStreamSynchronize(st));
    return RK_OK;
}

} // namespace

extern "C" int rk_cluster_hits_device(rk_ctx* c, const void* d_hits, uint64_t nhits, const void* d_offsets, int64_t n, uint64_t nvalues, int measure,
                                      uint32_t min_ppm, void* d_labels, uint32_t* rounds, void* hip_stream) {
    if (!c || !d_offsets || !d_labels || (!d_hits && nhits)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_cluster_shape("cluster", n, measure, min_ppm));
    RKCHK(set_dev(c));
    hipStream_t st = (hipStream_t)hip_stream;
    struct Scratch { DevBuf flag; ~Scratch() { flag.release(); } } s;
    RKCHK(s.flag.reserve(CL_FLAG_BYTES));
    Forest f;
    f.parent = (int32_t*)d_labels; f.flag = s.flag.as<uint32_t>(); f.n = (uint32_t)n;
    f.off = (const uint64_t*)d_offsets; f.nvalues = nvalues; f.measure = measure; f.min_ppm = min_ppm;
    RKCHK(forest_init(f, st));
    RKCHK(forest_hook(f, (const int32_t*)d_hits, nhits, 0, st));
    HIPCHK(hipStreamSynchronize(st));
    if (rounds) *rounds = f.rounds;
    return RK_OK;
}

extern "C" int rk_cluster_hits(rk_ctx* c, const rk_search_hit* hits, uint64_t nhits, const uint64_t* lens, int64_t n, int measure, uint32_t min_ppm,
                               int32_t* labels) {
    if (!c || !lens || !labels || (!hits && nhits)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_cluster_shape("cluster", n, measure, min_ppm));
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (lens[i] > 0x7fffffffull) return fail(RK_ERR_LIMIT, "cluster: sketch %lld holds 2^31 values or more", (long long)i);
        off[(size_t)i + 1] = off[(size_t)i] + lens[i];
    }
    RKCHK(set_dev(c));
    struct Up { DevBuf h, o, l; ~Up() { h.release(); o.release(); l.release(); } } up;
    RKCHK(up.h.reserve((size_t)nhits * sizeof(rk_search_hit) + 16));
    RKCHK(up.o.reserve(((size_t)n + 1) * 8));
    RKCHK(up.l.reserve((size_t)n * 4));
    if (nhits) HIPCHK(hipMemcpyAsync(up.h.p, hits, (size_t)nhits * sizeof(rk_search_hit), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(up.o.p, off.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->st));
    RKCHK(rk_cluster_hits_device(c, up.h.p, nhits, up.o.p, n, off[(size_t)n], measure, min_ppm, up.l.p, nullptr, c->st));
    HIPCHK(hipMemcpyAsync(labels, up.l.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

extern "C" int rk_cluster_scaled_device(rk_ctx* c, rk_scaled_index* ix, const void* d_values, const void* d_offsets, int64_t nref, uint64_t nvalues,
                                        int min_shared, int measure, uint32_t min_ppm, uint64_t hit_cap, void* d_labels, void* hip_stream) {
    if (!c || !ix || !d_offsets || !d_labels || (!d_values && nvalues)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_self_shape(c, ix, nref, min_shared, measure, min_ppm));
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    RKCHK(ix->w_cl.reserve(CL_FLAG_BYTES));
    Forest f;
    f.parent = (int32_t*)d_labels; f.flag = ix->w_cl.as<uint32_t>(); f.n = (uint32_t)nref;
    f.off = (const uint64_t*)d_offsets; f.nvalues = nvalues; f.measure = measure; f.min_ppm = min_ppm;
    return cluster_self(ix, (const uint64_t*)d_values, f.off, min_shared, hit_cap ? hit_cap : RK_CLUSTER_HIT_CAP, f, (hipStream_t)hip_stream);
}

extern "C" int rk_cluster_scaled(rk_ctx* c, rk_scaled_index* ix, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, int min_shared,
                                 int measure, uint32_t min_ppm, uint64_t hit_cap, int32_t* labels) {
    if (!c || !ix || !r_offsets || !labels) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_self_shape(c, ix, nref, min_shared, measure, min_ppm));
    RKCHK(check_csr(r_offsets, nref, "cluster: ", "the collection", RK_ERR_LIMIT));
    const uint64_t rn = r_offsets[nref] - r_offsets[0];
    if (rn && !r_values) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(ix->mu);
    RKCHK(ix->w_qv.reserve((size_t)rn * 8 + 8));
    RKCHK(ix->w_qo.reserve(((size_t)nref + 1) * 8));
    RKCHK(ix->w_cl.reserve(CL_FLAG_BYTES + (size_t)nref * 4));
    std::vector<uint64_t> off;
    RKCHK(upload_csr(r_values, r_offsets, nref, ix->w_qv.as<uint64_t>(), ix->w_qo.as<uint64_t>(), off, c->st));
    Forest f;
    f.parent = (int32_t*)((char*)ix->w_cl.p + CL_FLAG_BYTES); f.flag = ix->w_cl.as<uint32_t>(); f.n = (uint32_t)nref;
    f.off = ix->w_qo.as<uint64_t>(); f.nvalues = rn; f.measure = measure; f.min_ppm = min_ppm;
    RKCHK(cluster_self(ix, ix->w_qv.as<uint64_t>(), f.off, min_shared, hit_cap ? hit_cap : RK_CLUSTER_HIT_CAP, f, c->st)); // (synchronises: off lives until there)
    HIPCHK(hipMemcpyAsync(labels, f.parent, (size_t)nref * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}
