// AddressSanitizer + UBSan over the host half of bottom samples (rk_bottom_host.cpp: rk_bottom_emit, the row building of
// rk_sample_finish_bottom) and the text side of --min-copies (rkmh_min_copies.hpp: the option's value, the "minCopies" key); no GPU,
// nothing loaded into Python.  Random counted sets -- arrays of exactly n entries, rows of exactly sketch_size: a read or write past
// either is the sanitizer's to find -- against a plain expansion done here, under both dedup rules, at min_copies 1, 2, 3 and 2^32 - 1,
// with counts that saturate and counts that alone fill the row; then every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rkmh_amd.h"
#include "rkmh_min_copies.hpp"

static std::string g_err;
extern "C" void rk__set_error(const char* msg) { g_err = msg ? msg : ""; }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void check_emit(const std::vector<uint64_t>& v, const std::vector<uint32_t>& c, int S, uint64_t m, int distinct) {
    std::vector<uint64_t> want;
    for (size_t j = 0; j < v.size() && want.size() < (size_t)S; ++j) {
        if (c[j] < m) continue;
        const uint64_t copies = distinct ? 1 : c[j];
        for (uint64_t t = 0; t < copies && want.size() < (size_t)S; ++t) want.push_back(v[j]);
    }
    std::vector<uint64_t> row((size_t)S, 0xababababababababull);
    int32_t len = -1;
    EXPECT(rk_bottom_emit(v.empty() ? nullptr : v.data(), c.empty() ? nullptr : c.data(), v.size(), S, m, distinct, row.data(), &len) == RK_OK);
    EXPECT(len == (int32_t)want.size());
    for (size_t j = 0; j < row.size(); ++j) EXPECT(row[j] == (j < want.size() ? want[j] : 0));
}

int main() {
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    int nsets = 0;
    for (int n : {0, 1, 2, 63, 64, 65, 1000, 1024, 1025, 20000}) {
        std::vector<uint64_t> v((size_t)n);
        for (auto& t : v) t = next() | 1;
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        std::vector<uint32_t> c(v.size());
        for (size_t j = 0; j < c.size(); ++j) {
            const uint64_t r = next() % 100;
            c[j] = r < 50 ? 1u : r < 80 ? 2u : r < 95 ? 3u : r < 98 ? (uint32_t)(next() % 40000) + 1 : 0xffffffffu;
        }
        for (int S : {1, 2, 64, 1000, RK_MAX_SKETCH})
            for (uint64_t m : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)0xffffffffull})
                for (int distinct : {0, 1}) { check_emit(v, c, S, m, distinct); ++nsets; }
    }
    check_emit({5}, {0xffffffffu}, RK_MAX_SKETCH, 0xffffffffull, 0);   // one saturated count fills the largest row
    check_emit({5, 9}, {3, 1}, 2, 1, 0);                               // cut off inside a value's copies
    // refusals
    uint64_t v2[2] = {5, 9}, same[2] = {5, 5}, down[2] = {9, 5}, zero[2] = {0, 5}, row[4];
    uint32_t c2[2] = {1, 1};
    int32_t len = 0;
    EXPECT(rk_bottom_emit(v2, c2, 2, 4, 1, 0, row, &len) == RK_OK && len == 2 && row[2] == 0 && row[3] == 0);
    EXPECT(rk_bottom_emit(same, c2, 2, 4, 1, 0, row, &len) == RK_ERR_ARG && !g_err.empty());
    EXPECT(rk_bottom_emit(down, c2, 2, 4, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(zero, c2, 2, 4, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(nullptr, c2, 2, 4, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, nullptr, 2, 4, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, 4, 1, 0, nullptr, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, 4, 1, 0, row, nullptr) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, 0, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, RK_MAX_SKETCH + 1, 1, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, 4, 0, 0, row, &len) == RK_ERR_ARG);
    EXPECT(rk_bottom_emit(v2, c2, 2, 4, 1ull << 32, 0, row, &len) == RK_ERR_ARG);
    // --min-copies as text, and the key of the sketch file
    uint64_t m = 7;
    EXPECT(min_copies_from_text("1", m) && m == 1);
    EXPECT(min_copies_from_text("4294967295", m) && m == 0xffffffffull);
    for (const char* t : {"", "0", "-1", "+2", " 2", "2 ", "2x", "x", "4294967296", "18446744073709551616", "99999999999999999999999"}) {
        m = 7;
        EXPECT(!min_copies_from_text(t, m) && m == 7);
    }
    EXPECT(!min_copies_from_text(nullptr, m));
    EXPECT(min_copies_json(0).empty() && min_copies_json(1).empty());
    EXPECT(min_copies_json(2) == ",\"minCopies\":2");
    EXPECT(min_copies_json(0xffffffffull) == ",\"minCopies\":4294967295");
    printf("%d sets, %d mismatches\n", nsets, g_bad);
    return g_bad ? 1 : 0;
}
