// rk_screen_host.cpp -- the host half of screen (include/rkmh_amd.h, "SCREEN"): the four numbers per reference computed from a counted
// set by the definition, and the identity.  Host code only, usable without a GPU; the kernels are rk_screen.hip.  The owner rule is the
// one expression both halves share in words: unsigned 64-bit products of numbers below 2^31, nothing wraps.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(int code, const std::string& msg) { rk__set_error(msg.c_str()); return code; }
constexpr uint64_t SAT = 0xffffffffull;
constexpr uint32_t NONE = 0xffffffffu;

uint32_t lower_median(std::vector<uint32_t>& c) {
    if (c.empty()) return 0;
    const size_t at = (c.size() - 1) / 2;
    std::nth_element(c.begin(), c.begin() + (std::ptrdiff_t)at, c.end());
    return c[at];
}
} // namespace

extern "C" int rk_screen_rows_host(const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, const uint64_t* c_values, const uint64_t* c_counts,
                                   uint64_t nc, uint64_t min_copies, uint32_t* out4) {
    const std::string who = "rk_screen_rows_host: ";
    if (!r_offsets || !out4 || (nc && (!c_values || !c_counts))) return bad(RK_ERR_ARG, who + "bad arguments");
    if (nref < 1) return bad(RK_ERR_ARG, who + "need at least one reference sketch, got " + std::to_string(nref));
    if (nref > 0x7fffffffll) return bad(RK_ERR_LIMIT, who + std::to_string(nref) + " reference sketches are more than 2^31-1");
    if (min_copies < 1 || min_copies > SAT) return bad(RK_ERR_ARG, who + "min_copies " + std::to_string(min_copies) + " outside [1,2^32-1]");
    for (int64_t r = 0; r < nref; ++r) {
        if (r_offsets[r + 1] < r_offsets[r]) return bad(RK_ERR_ARG, who + "offsets of the references decrease at sketch " + std::to_string(r));
        if (r_offsets[r + 1] - r_offsets[r] > 0x7fffffffull) return bad(RK_ERR_LIMIT, who + "sketch " + std::to_string(r) + " of the references holds 2^31 values or more");
    }
    if (r_offsets[nref] > r_offsets[0] && !r_values) return bad(RK_ERR_ARG, who + "bad arguments");
    for (uint64_t i = 0; i < nc; ++i) {
        if (c_values[i] == 0) return bad(RK_ERR_ARG, who + "value " + std::to_string(i) + " of the counted set is 0");
        if (i && c_values[i] <= c_values[i - 1]) return bad(RK_ERR_ARG, who + "the counted set does not ascend at value " + std::to_string(i));
    }
    // the rows collapsed; (value, reference) pairs of the present values, by value then reference
    struct Hit { uint64_t v; uint32_t r, c; };
    std::vector<Hit> hits;
    std::vector<uint64_t> len((size_t)nref, 0), shared((size_t)nref, 0);
    std::vector<uint32_t> cs;
    for (int64_t r = 0; r < nref; ++r) {
        cs.clear();
        for (uint64_t t = r_offsets[r]; t < r_offsets[r + 1]; ++t) {
            const uint64_t v = r_values[t];
            if (v == 0) return bad(RK_ERR_ARG, who + "value " + std::to_string(t - r_offsets[r]) + " of reference " + std::to_string(r) + " is 0");
            if (t > r_offsets[r] && v < r_values[t - 1]) return bad(RK_ERR_ARG, who + "reference " + std::to_string(r) + " descends at value " + std::to_string(t - r_offsets[r]));
            if (t > r_offsets[r] && v == r_values[t - 1]) continue;
            ++len[(size_t)r];
            const uint64_t* at = std::lower_bound(c_values, c_values + nc, v);
            if (at == c_values + nc || *at != v) continue;
            const uint64_t c = std::min(c_counts[at - c_values], SAT);
            if (c < min_copies) continue;
            hits.push_back(Hit{v, (uint32_t)r, (uint32_t)c});
            cs.push_back((uint32_t)c);
        }
        shared[(size_t)r] = cs.size();
        out4[r * 4 + 0] = (uint32_t)cs.size();
        out4[r * 4 + 1] = lower_median(cs);
    }
    std::stable_sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.v < b.v; }); // (references stay ascending inside a value)
    std::vector<std::vector<uint32_t>> owned((size_t)nref);
    for (size_t i = 0; i < hits.size();) {
        size_t j = i;
        uint32_t best = NONE;
        for (; j < hits.size() && hits[j].v == hits[i].v; ++j) {
            const uint32_t a = hits[j].r;
            if (best == NONE || shared[a] * len[best] > shared[best] * len[a]) best = a; // (equal ratios: the earlier, lower index stays)
        }
        owned[best].push_back(hits[i].c);
        i = j;
    }
    for (int64_t r = 0; r < nref; ++r) {
        out4[r * 4 + 2] = (uint32_t)owned[(size_t)r].size();
        out4[r * 4 + 3] = lower_median(owned[(size_t)r]);
    }
    return RK_OK;
}

extern "C" int rk_screen_identity(uint64_t shared, uint64_t len, int k, double* identity) {
    const std::string who = "rk_screen_identity: ";
    if (!identity) return bad(RK_ERR_ARG, who + "bad arguments");
    if (k < 1) return bad(RK_ERR_ARG, who + "k " + std::to_string(k) + " is below 1");
    if (shared > len) return bad(RK_ERR_ARG, who + std::to_string(shared) + " shared values of " + std::to_string(len));
    if (shared == 0) *identity = 0.0;
    else if (shared == len) *identity = 1.0;
    else *identity = std::pow((double)shared / (double)len, 1.0 / (double)k);
    return RK_OK;
}
