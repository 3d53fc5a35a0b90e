// AddressSanitizer + UBSan over the host half of sketch comparison (rk_pairs_host.cpp; no GPU, nothing loaded into Python).
// Input: the hand-checked vectors as text (run.sh writes them from tests/golden/pairs_kat.json), one per line:
//   S k common denom jaccard distance na a... nb b...
// For each: rk_mash_distance against the recorded values, rk_merge_sketches of {a, b} under both rules against a sort of the
// concatenation done here.  Then a 17-part merge (empty, short and full parts, values repeated inside and across parts) at several
// sketch sizes, and every refusal.  Prints a summary; exits non-zero on a mismatch.
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

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void check_merge(const std::vector<std::vector<uint64_t>>& parts, int S) {
    const int n = (int)parts.size();
    std::vector<uint64_t> rows((size_t)n * (size_t)S, 0), cat;
    std::vector<int32_t> lens((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        lens[(size_t)i] = (int32_t)parts[(size_t)i].size();
        std::copy(parts[(size_t)i].begin(), parts[(size_t)i].end(), rows.begin() + (size_t)i * (size_t)S);
        cat.insert(cat.end(), parts[(size_t)i].begin(), parts[(size_t)i].end());
    }
    std::sort(cat.begin(), cat.end());
    for (int distinct = 0; distinct < 2; ++distinct) {
        std::vector<uint64_t> want = cat;
        if (distinct) want.erase(std::unique(want.begin(), want.end()), want.end());
        if (want.size() > (size_t)S) want.resize((size_t)S);
        std::vector<uint64_t> out((size_t)S, 77);   // exactly S: a write past it is the sanitizer's to find
        int32_t m = -1;
        EXPECT(rk_merge_sketches(n ? rows.data() : nullptr, n ? lens.data() : nullptr, n, S, distinct, out.data(), &m) == RK_OK);
        EXPECT(m == (int32_t)want.size());
        for (size_t j = 0; j < (size_t)S; ++j) EXPECT(out[j] == (j < want.size() ? want[j] : 0));
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int S, k, common, denom, nvec = 0;
    double jac, dist;
    while (fscanf(f, "%d %d %d %d %lf %lf", &S, &k, &common, &denom, &jac, &dist) == 6) {
        std::vector<std::vector<uint64_t>> ab(2);
        for (auto& x : ab) {
            int n = 0;
            if (fscanf(f, "%d", &n) != 1) return 2;
            x.resize((size_t)n);
            for (auto& v : x) { unsigned long long t; if (fscanf(f, "%llu", &t) != 1) return 2; v = t; }
        }
        double j = -1, d = -1;
        EXPECT(rk_mash_distance(common, denom, k, &j, &d) == RK_OK);
        EXPECT(j == jac && std::fabs(d - dist) < 1e-15 && !std::signbit(d));
        EXPECT(rk_mash_distance(common, denom, k, nullptr, nullptr) == RK_OK);
        check_merge(ab, S);
        ++nvec;
    }
    fclose(f);
    EXPECT(nvec >= 20);
    // 17 parts
    uint64_t x = 88172645463325252ull;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    int nmerge = 0;
    for (int S2 : {1, 2, 5, 64, 1000, RK_MAX_SKETCH}) {
        std::vector<uint64_t> pool((size_t)S2 + (size_t)S2 / 2 + 3);
        for (auto& v : pool) v = next() | 1;
        std::vector<std::vector<uint64_t>> parts(17);
        for (int i = 0; i < 17; ++i) {
            const int len = i % 4 == 0 ? 0 : i % 4 == 1 ? 1 : i % 4 == 2 ? S2 : S2 / 2;
            for (int j = 0; j < len; ++j) parts[(size_t)i].push_back(pool[next() % pool.size()]);
            std::sort(parts[(size_t)i].begin(), parts[(size_t)i].end());
        }
        check_merge(parts, S2);
        check_merge({parts[2]}, S2);
        check_merge({}, S2);
        nmerge += 3;
    }
    // refusals
    uint64_t row[4] = {1, 2, 3, 4}, out[4];
    int32_t len = 4, m = 0, over = 5, neg = -1;
    EXPECT(rk_merge_sketches(row, &len, 1, 0, 0, out, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(row, &len, 1, RK_MAX_SKETCH + 1, 0, out, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(row, &over, 1, 4, 0, out, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(row, &neg, 1, 4, 0, out, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(nullptr, &len, 1, 4, 0, out, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(row, &len, 1, 4, 0, nullptr, &m) == RK_ERR_ARG);
    EXPECT(rk_merge_sketches(row, &len, -1, 4, 0, out, &m) == RK_ERR_ARG && !g_err.empty());
    EXPECT(rk_mash_distance(-1, 5, 16, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_mash_distance(6, 5, 16, nullptr, nullptr) == RK_ERR_ARG);
    EXPECT(rk_mash_distance(1, 5, 0, nullptr, nullptr) == RK_ERR_ARG);
    printf("%d vectors, %d merges, %d mismatches\n", nvec, nmerge, g_bad);
    return g_bad ? 1 : 0;
}
