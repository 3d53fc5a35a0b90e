// rk_pairs_host.cpp -- the host half of sketch comparison (include/rkmh_amd.h, "SKETCH COMPARISON"): the bottom-S of a union of
// sketches (what `-g` reduces the records of a file with) and the one place where counts become floating point, Mash's distance.
// Host code only, usable without a GPU; the all-pairs kernel is rk_pairs.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(const std::string& msg) { rk__set_error(msg.c_str()); return RK_ERR_ARG; }
} // namespace

// out[sketch_size] (zero padded), *out_len: the sketch_size smallest values of the union of n sketches (rows of sketch_size uint64,
// the first lens[i] of row i are its values; zeros are padding, never values).  distinct = 0 keeps repeats (dedup=multiset: the
// sketch of the concatenated hashes), 1 keeps each value once (dedup=distinct).  Exact: a value among the sketch_size smallest of
// the union is among the sketch_size smallest of its part.
extern "C" int rk_merge_sketches(const uint64_t* sketches, const int32_t* lens, int n, int sketch_size, int distinct, uint64_t* out, int32_t* out_len) {
    if (!out || !out_len || n < 0 || (n > 0 && (!sketches || !lens))) return bad("rk_merge_sketches: bad arguments");
    if (sketch_size < 1 || sketch_size > RK_MAX_SKETCH) return bad("rk_merge_sketches: sketch size " + std::to_string(sketch_size) + " outside [1," + std::to_string(RK_MAX_SKETCH) + "]");
    const size_t S = (size_t)sketch_size;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (lens[i] < 0 || lens[i] > sketch_size) return bad("rk_merge_sketches: length " + std::to_string(lens[i]) + " of sketch " + std::to_string(i) + " outside [0," + std::to_string(sketch_size) + "]");
        total += (size_t)lens[i];
    }
    std::vector<uint64_t> v;
    v.reserve(total);
    for (int i = 0; i < n; ++i)
        for (int32_t j = 0; j < lens[i]; ++j) {
            const uint64_t h = sketches[(size_t)i * S + (size_t)j];
            if (h != 0) v.push_back(h);
        }
    std::sort(v.begin(), v.end());
    if (distinct) v.erase(std::unique(v.begin(), v.end()), v.end());
    const size_t m = std::min(v.size(), S);
    if (m) memcpy(out, v.data(), m * 8);
    if (m < S) memset(out + m, 0, (S - m) * 8);
    *out_len = (int32_t)m;
    return RK_OK;
}

// Mash's distance from the merged bottom-S counts of rk_compare_sketches (fields 2 and 3): j = common / denom (0 when denom = 0);
// the distance is 1 when common = 0, else -ln(2j / (1 + j)) / k clamped to [0, 1] (never -0).  Either result pointer may be NULL.
extern "C" int rk_mash_distance(int common, int denom, int k, double* jaccard, double* distance) {
    if (common < 0 || denom < 0 || common > denom || k < 1) return bad("rk_mash_distance: need 0 <= common <= denom and k >= 1");
    const double j = denom > 0 ? (double)common / (double)denom : 0.0;
    double d = 1.0;
    if (common > 0) {
        d = -std::log(2.0 * j / (1.0 + j)) / (double)k;
        if (!(d > 0.0)) d = 0.0;
        if (d > 1.0) d = 1.0;
    }
    if (jaccard) *jaccard = j;
    if (distance) *distance = d;
    return RK_OK;
}
