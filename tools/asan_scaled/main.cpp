// AddressSanitizer + UBSan over the host half of scaled sketches (rk_scaled_host.cpp; no GPU, nothing loaded into Python).
// Input: the hand-checked vectors as text (run.sh writes them from tests/golden/scaled_kat.json), one per line:
//   want na a... nb b...
// For each: the union of {a, b} by rk_merge_scaled against a sort of the concatenation done here, with and without a cut, |a| + |b|
// - |union| against the recorded `shared`, and rk_scaled_distance on those counts.  Then 17-part merges (empty, short and long parts,
// values repeated inside and across parts, zeros), rk_scaled_max_hash and every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rkmh_amd.h"

static std::string g_err;
extern "C" void rk__set_error(const char* msg) { g_err = msg ? msg : ""; }
extern "C" void rk_free(void* p) { free(p); }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

// the union of the parts cut at max_hash, checked against a sort done here; returns its size
static size_t check_merge(const std::vector<std::vector<uint64_t>>& parts, uint64_t max_hash) {
    std::vector<uint64_t> values, want;
    std::vector<uint64_t> off(1, 0);
    for (const auto& p : parts) {
        values.insert(values.end(), p.begin(), p.end());
        off.push_back(values.size());
        for (uint64_t v : p) if (v != 0 && v <= max_hash) want.push_back(v);
    }
    std::sort(want.begin(), want.end());
    want.erase(std::unique(want.begin(), want.end()), want.end());
    std::vector<uint64_t> exact(values);   // exactly as many as the offsets say: a read past it is the sanitizer's to find
    uint64_t* out = nullptr;
    uint64_t n = ~0ull;
    EXPECT(rk_merge_scaled(exact.empty() ? nullptr : exact.data(), off.data(), (int)parts.size(), max_hash, &out, &n) == RK_OK);
    EXPECT(n == want.size());
    if (out && n == want.size())
        for (size_t j = 0; j < want.size(); ++j) EXPECT(out[j] == want[j]);
    rk_free(out);
    return want.size();
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    long long want_shared;
    int nvec = 0;
    while (fscanf(f, "%lld", &want_shared) == 1) {
        std::vector<std::vector<uint64_t>> ab(2);
        for (auto& x : ab) {
            int n = 0;
            if (fscanf(f, "%d", &n) != 1) return 2;
            x.resize((size_t)n);
            for (auto& v : x) { unsigned long long t; if (fscanf(f, "%llu", &t) != 1) return 2; v = t; }
        }
        const size_t uni = check_merge(ab, ~0ull);
        const long long la = (long long)ab[0].size(), lb = (long long)ab[1].size();
        EXPECT(la + lb - (long long)uni == want_shared);
        if (!ab[0].empty()) check_merge(ab, ab[0][ab[0].size() / 2]);      // a cut that sits on a value
        if (!ab[1].empty()) check_merge(ab, ab[1][0] - 1);                 // and one just below a value
        check_merge({ab[1], ab[0]}, ~0ull);
        double j = -1, d = -1;
        EXPECT(rk_scaled_distance(want_shared, la, lb, 21, &j, &d) == RK_OK);
        EXPECT(j == (uni ? (double)want_shared / (double)uni : 0.0) && d >= 0.0 && d <= 1.0 && !std::signbit(d));
        EXPECT((want_shared == 0) == (d == 1.0) || want_shared > 0);
        EXPECT(rk_scaled_distance(want_shared, la, lb, 21, nullptr, nullptr) == RK_OK);
        ++nvec;
    }
    fclose(f);
    EXPECT(nvec >= 20);
    // 17 parts
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    int nmerge = 0;
    for (int size : {1, 2, 5, 64, 1000, 20000}) {
        std::vector<uint64_t> pool((size_t)size + (size_t)size / 2 + 3);
        for (auto& v : pool) v = next() | 1;
        pool[0] = ~0ull;
        std::vector<std::vector<uint64_t>> parts(17);
        for (int i = 0; i < 17; ++i) {
            const int len = i % 4 == 0 ? 0 : i % 4 == 1 ? 1 : i % 4 == 2 ? size : size / 2;
            for (int j = 0; j < len; ++j) parts[(size_t)i].push_back(pool[next() % pool.size()]);
            if (i % 5 == 2) parts[(size_t)i].push_back(0);                  // zeros are never values
            if (i % 2) std::sort(parts[(size_t)i].begin(), parts[(size_t)i].end());
        }
        for (uint64_t mh : {(uint64_t)~0ull, (uint64_t)(~0ull / 2), (uint64_t)(~0ull / 1000), (uint64_t)1}) { check_merge(parts, mh); ++nmerge; }
        check_merge({parts[2]}, ~0ull / 3);
        check_merge({}, ~0ull);
        nmerge += 2;
    }
    // rk_scaled_max_hash
    uint64_t mh = 0;
    EXPECT(rk_scaled_max_hash(1, &mh) == RK_OK && mh == ~0ull);
    EXPECT(rk_scaled_max_hash(2, &mh) == RK_OK && mh == 0x7fffffffffffffffull);
    EXPECT(rk_scaled_max_hash(3, &mh) == RK_OK && mh == 0x5555555555555555ull);
    EXPECT(rk_scaled_max_hash(1000, &mh) == RK_OK && mh == 18446744073709551ull);
    EXPECT(rk_scaled_max_hash(1ull << 32, &mh) == RK_OK && mh == 0xffffffffull);
    EXPECT(rk_scaled_max_hash(~0ull, &mh) == RK_OK && mh == 1);
    // refusals
    EXPECT(rk_scaled_max_hash(0, &mh) == RK_ERR_ARG && !g_err.empty());
    EXPECT(rk_scaled_max_hash(5, nullptr) == RK_ERR_ARG);
    uint64_t row[4] = {1, 2, 3, 4}, up[2] = {0, 4}, down[3] = {0, 3, 2};
    uint64_t* out = nullptr;
    uint64_t n = 0;
    EXPECT(rk_merge_scaled(row, down, 2, ~0ull, &out, &n) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled(nullptr, up, 1, ~0ull, &out, &n) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled(row, nullptr, 1, ~0ull, &out, &n) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled(row, up, -1, ~0ull, &out, &n) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled(row, up, 1, ~0ull, nullptr, &n) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled(row, up, 1, ~0ull, &out, nullptr) == RK_ERR_ARG);
    EXPECT(rk_scaled_distance(-1, 5, 5, 21, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_scaled_distance(2, -1, 5, 21, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_scaled_distance(6, 5, 9, 21, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_scaled_distance(6, 9, 5, 21, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_scaled_distance(1, 5, 5, 0, nullptr, nullptr) == RK_ERR_ARG);
    double j = -1, d = -1;
    EXPECT(rk_scaled_distance(0, 0, 0, 21, &j, &d) == RK_OK && j == 0.0 && d == 1.0);
    EXPECT(rk_scaled_distance(INT64_MAX / 4, INT64_MAX / 2, INT64_MAX / 2, 21, &j, &d) == RK_OK && j > 0.33 && j < 0.34);
    printf("%d vectors, %d merges, %d mismatches\n", nvec, nmerge, g_bad);
    return g_bad ? 1 : 0;
}
