// rk_cluster_host.cpp -- the host half of cluster (include/rkmh_amd.h, "CLUSTER"): the single-linkage clusters of a list of hits by
// union-find, and the clusters of a label array laid out with their representatives.  Host code only, usable without a GPU; the
// kernels are rk_cluster.hip.  The link test is the one expression both halves share in words: signed 64-bit integers, nothing wraps.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(int code, const std::string& msg) { rk__set_error(msg.c_str()); return code; }

int find_root(std::vector<int32_t>& parent, int32_t x) {
    int32_t r = x;
    while (parent[(size_t)r] != r) r = parent[(size_t)r];
    while (parent[(size_t)x] != r) { const int32_t next = parent[(size_t)x]; parent[(size_t)x] = r; x = next; } // path compression
    return r;
}
} // namespace

extern "C" int rk_cluster_hits_host(const rk_search_hit* hits, uint64_t nhits, const uint64_t* lens, int64_t n, int measure, uint32_t min_ppm,
                                    int32_t* labels) {
    const std::string who = "rk_cluster_hits_host: ";
    if (!lens || !labels || (!hits && nhits)) return bad(RK_ERR_ARG, who + "bad arguments");
    if (n < 1) return bad(RK_ERR_ARG, who + "need at least one sketch, got " + std::to_string(n));
    if (n > 0x7fffffffll) return bad(RK_ERR_LIMIT, who + std::to_string(n) + " sketches are more than 2^31-1");
    if (measure != RK_CLUSTER_JACCARD && measure != RK_CLUSTER_MAX_CONTAINMENT) return bad(RK_ERR_ARG, who + "measure " + std::to_string(measure) + " is not defined");
    if (min_ppm > 1000000u) return bad(RK_ERR_ARG, who + "min_ppm " + std::to_string(min_ppm) + " is above 1000000");
    for (int64_t i = 0; i < n; ++i)
        if (lens[i] > 0x7fffffffull) return bad(RK_ERR_LIMIT, who + "sketch " + std::to_string(i) + " holds 2^31 values or more");
    std::vector<int32_t> parent((size_t)n);
    for (int64_t i = 0; i < n; ++i) parent[(size_t)i] = (int32_t)i;
    for (uint64_t h = 0; h < nhits; ++h) {
        const int64_t i = hits[h].query, j = hits[h].ref, shared = hits[h].shared;
        if (i < 0 || j < 0 || i >= n || j >= n || i == j || shared < 1) continue;
        const int64_t li = (int64_t)lens[i], lj = (int64_t)lens[j];
        const int64_t denom = measure == RK_CLUSTER_JACCARD ? li + lj - shared : (li < lj ? li : lj);
        if (shared * 1000000 < (int64_t)min_ppm * denom) continue;
        const int32_t a = find_root(parent, (int32_t)i), b = find_root(parent, (int32_t)j);
        if (a != b) parent[(size_t)(a > b ? a : b)] = a > b ? b : a; // the smaller root stays a root: a root is the minimum of its tree
    }
    for (int64_t i = 0; i < n; ++i) labels[i] = find_root(parent, (int32_t)i);
    return RK_OK;
}

extern "C" int rk_cluster_members(const int32_t* labels, const uint64_t* lens, int64_t n, int64_t* ncl, int32_t* cl_off, int32_t* members, int32_t* rep) {
    const std::string who = "rk_cluster_members: ";
    if (!labels || !lens || !ncl || !cl_off || !members || !rep) return bad(RK_ERR_ARG, who + "bad arguments");
    if (n < 1) return bad(RK_ERR_ARG, who + "need at least one sketch, got " + std::to_string(n));
    if (n > 0x7fffffffll) return bad(RK_ERR_LIMIT, who + std::to_string(n) + " sketches are more than 2^31-1");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t l = labels[i];
        if (l < 0 || l > i || labels[l] != l) return bad(RK_ERR_ARG, who + "label " + std::to_string(l) + " of sketch " + std::to_string(i) + " is not the smallest index of a cluster");
    }
    // roots ascend with the clusters' smallest members: number them, count, lay out, fill in index order
    std::vector<int32_t> cluster_of((size_t)n, -1), fill;
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i)
        if (labels[i] == i) cluster_of[(size_t)i] = (int32_t)c++;
    for (int64_t k = 0; k <= c; ++k) cl_off[k] = 0;
    for (int64_t i = 0; i < n; ++i) ++cl_off[cluster_of[(size_t)labels[i]] + 1];
    for (int64_t k = 0; k < c; ++k) cl_off[k + 1] += cl_off[k];
    fill.assign(cl_off, cl_off + c);
    for (int64_t k = 0; k < c; ++k) rep[k] = -1;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t k = cluster_of[(size_t)labels[i]];
        members[fill[(size_t)k]++] = (int32_t)i;
        if (rep[k] < 0 || lens[i] > lens[rep[k]]) rep[k] = (int32_t)i; // (strictly larger: among equal lengths the lowest index stays)
    }
    *ncl = c;
    return RK_OK;
}
