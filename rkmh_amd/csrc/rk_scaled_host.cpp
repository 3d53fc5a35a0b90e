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
