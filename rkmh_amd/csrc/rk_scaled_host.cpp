// rk_scaled_host.cpp -- the host half of scaled (FracMinHash) sketches (include/rkmh_amd.h, "SCALED SKETCHES"): the threshold of a
// `scaled` value, the union of sketches (what `-g` reduces the records of a file with, and what cuts a sketch down to a larger
// `scaled`), and the one place where counts become floating point.  Host code only, usable without a GPU; the kernels are
// rk_scaled.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(const std::string& msg) { rk__set_error(msg.c_str()); return RK_ERR_ARG; }
} // namespace

// max_hash(scaled) = floor((2^64 - 1) / scaled): a hash h is kept when 0 < h <= max_hash.  scaled = 1 keeps everything.
extern "C" int rk_scaled_max_hash(uint64_t scaled, uint64_t* max_hash) {
    if (!max_hash) return bad("rk_scaled_max_hash: max_hash is NULL");
    if (scaled == 0) return bad("rk_scaled_max_hash: scaled must be at least 1");
    *max_hash = ~0ull / scaled;
    return RK_OK;
}

// *out (malloc'd, rk_free), *out_len: the ascending distinct values v of n sketches (CSR: sketch i is values[offsets[i], offsets[i+1]))
// with 0 < v <= max_hash.  n = 1 cuts one sketch down to a larger `scaled`: exact, because max_hash is monotone in scaled.
extern "C" int rk_merge_scaled(const uint64_t* values, const uint64_t* offsets, int n, uint64_t max_hash, uint64_t** out, uint64_t* out_len) {
    if (!out || !out_len || n < 0 || (n > 0 && !offsets)) return bad("rk_merge_scaled: bad arguments");
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return bad("rk_merge_scaled: offsets decrease at sketch " + std::to_string(i));
    const uint64_t lo = n ? offsets[0] : 0, hi = n ? offsets[n] : 0;
    if (hi > lo && !values) return bad("rk_merge_scaled: values is NULL");
    std::vector<uint64_t> v;
    v.reserve((size_t)(hi - lo));
    for (uint64_t t = lo; t < hi; ++t)
        if (values[t] != 0 && values[t] <= max_hash) v.push_back(values[t]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    uint64_t* r = (uint64_t*)malloc(sizeof(uint64_t) * (v.empty() ? 1 : v.size()));
    if (!r) { rk__set_error("rk_merge_scaled: malloc"); return RK_ERR_NOMEM; }
    if (!v.empty()) memcpy(r, v.data(), v.size() * 8);
    *out = r;
    *out_len = (uint64_t)v.size();
    return RK_OK;
}

// ---- gather on the host (include/rkmh_amd.h, "GATHER"): the loop of rk_gather.hip on host threads -- each reference value looked up in
// Q once, the hits of every candidate kept as a list of query indices, then per round a recount of every list against one byte per
// query value, the pick, and the removal.
namespace {
// f(begin, end) over [0, n) in contiguous pieces on at most nt threads (the caller's thread takes the first piece)
template <typename F>
void on_threads(size_t n, int nt, size_t min_piece, F f) {
    const size_t pieces = std::max<size_t>(1, std::min<size_t>((size_t)std::max(nt, 1), n / std::max<size_t>(min_piece, 1)));
    if (pieces == 1) { f((size_t)0, n); return; }
    const size_t per = (n + pieces - 1) / pieces;
    std::vector<std::thread> th;
    for (size_t i = 1; i < pieces; ++i) {
        const size_t lo = per * i, hi = std::min(n, lo + per);
        if (lo >= hi) break;
        th.emplace_back([=] { f(lo, hi); });
    }
    f((size_t)0, std::min(n, per));
    for (auto& t : th) t.join();
}
} // namespace

extern "C" int rk_gather_scaled_host(const uint64_t* q, uint64_t nq, const uint64_t* rv, const uint64_t* roff, int nref, int min_shared,
                                     int max_rounds, int threads, int32_t* out4, int* nrounds) {
    if (!roff || !out4 || !nrounds || (!q && nq)) return bad("rk_gather_scaled_host: bad arguments");
    if (nref < 1) return bad("rk_gather_scaled_host: need at least one reference sketch");
    if (min_shared < 1 || max_rounds < 1) return bad("rk_gather_scaled_host: min_shared and max_rounds must be at least 1");
    if (nq > 0x7fffffffull) { rk__set_error("rk_gather_scaled_host: a query of more than 2^31-1 values"); return RK_ERR_LIMIT; }
    for (uint64_t i = 0; i < nq; ++i)
        if (q[i] == 0 || (i && q[i] <= q[i - 1])) return bad("rk_gather_scaled_host: the query is not ascending, distinct and non-zero at value " + std::to_string(i));
    for (int i = 0; i < nref; ++i) {
        if (roff[i + 1] < roff[i]) return bad("rk_gather_scaled_host: offsets of the references decrease at sketch " + std::to_string(i));
        if (roff[i + 1] - roff[i] > 0x7fffffffull) { rk__set_error("rk_gather_scaled_host: a reference sketch of 2^31 values or more"); return RK_ERR_LIMIT; }
    }
    if (roff[nref] > roff[0] && !rv) return bad("rk_gather_scaled_host: r_values is NULL");
    *nrounds = 0;
    // the hits of every reference: a row ascends, so each lookup starts where the one before it ended
    std::vector<std::vector<uint32_t>> hits((size_t)nref);
    on_threads((size_t)nref, threads, 1, [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) {
            const uint64_t* at = q;
            for (uint64_t t = roff[r]; t < roff[r + 1] && at < q + nq; ++t) {
                at = std::lower_bound(at, q + nq, rv[t]);
                if (at < q + nq && *at == rv[t]) hits[r].push_back((uint32_t)(at - q));
            }
        }
    });
    std::vector<int> cand; // references with total >= min_shared, ascending: the others can never win
    for (int r = 0; r < nref; ++r)
        if (hits[(size_t)r].size() >= (size_t)min_shared) cand.push_back(r);
    std::vector<uint8_t> alive((size_t)nq, 1);
    std::vector<int32_t> count(cand.size());
    int64_t remaining = (int64_t)nq;
    const int rows = (int)std::min<size_t>((size_t)max_rounds, cand.size());
    for (int t = 0; t < rows; ++t) {
        on_threads(cand.size(), threads, 16, [&](size_t lo, size_t hi) {
            for (size_t c = lo; c < hi; ++c) {
                int32_t n = 0;
                for (uint32_t h : hits[(size_t)cand[c]]) n += alive[h];
                count[c] = n;
            }
        });
        size_t best = 0; // the largest count; among equals the first candidate = the lowest reference index
        for (size_t c = 1; c < cand.size(); ++c)
            if (count[c] > count[best]) best = c;
        if (count[best] < min_shared) break;
        const std::vector<uint32_t>& mine = hits[(size_t)cand[best]];
        for (uint32_t h : mine) alive[h] = 0;
        remaining -= count[best];
        int32_t* row = out4 + (size_t)t * 4;
        row[0] = cand[best]; row[1] = count[best]; row[2] = (int32_t)mine.size(); row[3] = (int32_t)remaining;
        *nrounds = t + 1;
    }
    return RK_OK;
}

// rk_mash_distance's formula and clamps on j = shared / (la + lb - shared): j = 0 and the distance 1 when the union is empty; the
// distance is 1 when shared = 0, else -ln(2j / (1 + j)) / k clamped to [0, 1] (never -0).  Either result pointer may be NULL.
extern "C" int rk_scaled_distance(int64_t shared, int64_t la, int64_t lb, int k, double* jaccard, double* distance) {
    if (shared < 0 || la < 0 || lb < 0 || shared > std::min(la, lb) || k < 1)
        return bad("rk_scaled_distance: need 0 <= shared <= min(la, lb) and k >= 1");
    const double uni = (double)la + (double)lb - (double)shared;
    const double j = uni > 0 ? (double)shared / uni : 0.0;
    double d = 1.0;
    if (shared > 0) {
        d = -std::log(2.0 * j / (1.0 + j)) / (double)k;
        if (!(d > 0.0)) d = 0.0;
        if (d > 1.0) d = 1.0;
    }
    if (jaccard) *jaccard = j;
    if (distance) *distance = d;
    return RK_OK;
}
