// rk_bottom_host.cpp -- the host half of bottom samples (include/rkmh_amd.h, "BOTTOM SAMPLES"): from a sorted distinct set of
// (value, count) pairs to the bottom-s sketch row.  Host code only, usable without a GPU; the cut that bounds the set is rk_bottom.hip.
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(const std::string& msg) { rk__set_error(msg.c_str()); return RK_ERR_ARG; }
} // namespace

// row[sketch_size] (zero padded), *len: ascending, every value whose count is at least min_copies -- once (distinct), or once per
// copy (multiset) --, cut off where sketch_size is reached.  values[0, n) ascend and are distinct (checked: RK_ERR_ARG), no value is 0.
extern "C" int rk_bottom_emit(const uint64_t* values, const uint32_t* counts, uint64_t n, int sketch_size, uint64_t min_copies, int distinct, uint64_t* row,
                              int32_t* len) {
    if (!row || !len || (n && (!values || !counts))) return bad("rk_bottom_emit: bad arguments");
    if (sketch_size < 1 || sketch_size > RK_MAX_SKETCH) return bad("rk_bottom_emit: sketch size " + std::to_string(sketch_size) + " outside [1," + std::to_string(RK_MAX_SKETCH) + "]");
    if (min_copies < 1 || min_copies > 0xffffffffull) return bad("rk_bottom_emit: min_copies " + std::to_string(min_copies) + " outside [1,2^32-1]");
    const size_t S = (size_t)sketch_size;
    size_t at = 0;
    for (uint64_t j = 0; j < n; ++j) {
        if (values[j] == 0 || (j && values[j] <= values[j - 1])) return bad("rk_bottom_emit: the values do not ascend at entry " + std::to_string(j));
        if (at == S || counts[j] < min_copies) continue; // (the walk goes on for the check alone)
        size_t copies = distinct ? 1 : (size_t)counts[j];
        if (copies > S - at) copies = S - at;
        for (size_t t = 0; t < copies; ++t) row[at++] = values[j];
    }
    if (at < S) memset(row + at, 0, (S - at) * 8);
    *len = (int32_t)at;
    return RK_OK;
}
