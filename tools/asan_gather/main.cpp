// AddressSanitizer + UBSan over rk_gather_scaled_host (rk_scaled_host.cpp; no GPU, nothing loaded into Python).
// Input: the hand-checked vectors as text (run.sh writes them from tests/golden/gather_kat.json), one per line:
//   min_shared max_rounds nrows rows(4 each)... nq q... nref (len values...)...
// Each runs on 1 and 4 threads in arrays of exactly the sizes the call may touch.  Then seeded random sets against a plain loop
// written here, and every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "rkmh_amd.h"

static std::string g_err;
extern "C" void rk__set_error(const char* msg) { g_err = msg ? msg : ""; }
extern "C" void rk_free(void* p) { free(p); }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

typedef std::vector<uint64_t> Set;

static std::vector<int32_t> plain(const Set& q, const std::vector<Set>& refs, int min_shared, int max_rounds) {
    std::vector<int32_t> rows;
    Set alive(q);
    for (int t = 0; t < max_rounds; ++t) {
        int best = -1; size_t best_n = 0;
        for (size_t r = 0; r < refs.size(); ++r) {
            Set both;
            std::set_intersection(alive.begin(), alive.end(), refs[r].begin(), refs[r].end(), std::back_inserter(both));
            if (best < 0 || both.size() > best_n) { best = (int)r; best_n = both.size(); }
        }
        if (best < 0 || best_n < (size_t)min_shared) break;
        Set total, left;
        std::set_intersection(q.begin(), q.end(), refs[best].begin(), refs[best].end(), std::back_inserter(total));
        std::set_difference(alive.begin(), alive.end(), refs[best].begin(), refs[best].end(), std::back_inserter(left));
        alive.swap(left);
        rows.insert(rows.end(), {(int32_t)best, (int32_t)best_n, (int32_t)total.size(), (int32_t)alive.size()});
    }
    return rows;
}

static void check(const Set& q, const std::vector<Set>& refs, int min_shared, int max_rounds, const std::vector<int32_t>& want) {
    Set values;
    std::vector<uint64_t> off(1, 0);
    for (const Set& r : refs) { values.insert(values.end(), r.begin(), r.end()); off.push_back(values.size()); }
    Set qq(q); // exactly nq values: a read past them is the sanitizer's to find
    for (int threads : {1, 4}) {
        std::vector<int32_t> out((size_t)std::min<size_t>((size_t)max_rounds, refs.size()) * 4, -7);
        int n = -1;
        EXPECT(rk_gather_scaled_host(qq.empty() ? nullptr : qq.data(), qq.size(), values.empty() ? nullptr : values.data(), off.data(), (int)refs.size(),
                                     min_shared, max_rounds, threads, out.empty() ? (int32_t*)&n : out.data(), &n) == RK_OK);
        EXPECT(n >= 0 && (size_t)n * 4 == want.size());
        if (n >= 0 && (size_t)n * 4 == want.size()) EXPECT(std::equal(want.begin(), want.end(), out.begin()));
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int nvec = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        long long min_shared, max_rounds, nrows, n;
        s >> min_shared >> max_rounds >> nrows;
        std::vector<int32_t> want((size_t)nrows * 4);
        for (auto& x : want) s >> x;
        s >> n;
        Set q((size_t)n);
        for (auto& x : q) s >> x;
        s >> n;
        std::vector<Set> refs((size_t)n);
        for (auto& r : refs) { s >> n; r.resize((size_t)n); for (auto& x : r) s >> x; }
        EXPECT(!s.fail());
        check(q, refs, (int)min_shared, (int)max_rounds, want);
        EXPECT(plain(q, refs, (int)min_shared, (int)max_rounds) == want);
        ++nvec;
    }
    EXPECT(nvec >= 16);
    std::mt19937_64 rng(7);
    int nrand = 0;
    for (int nref : {1, 9, 65, 300}) {
        Set pool(3000);
        for (auto& x : pool) x = rng() | 1;
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        auto draw = [&](size_t m) { Set s; for (size_t i = 0; i < m; ++i) s.push_back(pool[rng() % pool.size()]); std::sort(s.begin(), s.end()); s.erase(std::unique(s.begin(), s.end()), s.end()); return s; };
        std::vector<Set> refs;
        for (int r = 0; r < nref; ++r) refs.push_back(draw((size_t[]){0, 1, 7, 64, 65, 129, 1000}[rng() % 7]));
        Set q = draw(1500);
        for (uint64_t x = 2; x < 400; x += 2) q.push_back(x); // foreign (even) values
        std::sort(q.begin(), q.end());
        for (int min_shared : {1, 20}) for (int max_rounds : {1, 5, 1000}) { check(q, refs, min_shared, max_rounds, plain(q, refs, min_shared, max_rounds)); ++nrand; }
    }
    // refusals
    Set q = {1, 2, 3}, v = {1, 2, 3, 4};
    std::vector<uint64_t> off = {0, 2, 4}, down = {0, 3, 1};
    Set unsorted = {2, 1, 3}, zero = {0, 1, 2};
    int32_t out[8]; int n = 0;
    EXPECT(rk_gather_scaled_host(q.data(), 3, v.data(), off.data(), 0, 1, 1, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(q.data(), 3, v.data(), off.data(), 2, 0, 1, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(q.data(), 3, v.data(), off.data(), 2, 1, 0, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(unsorted.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(zero.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(q.data(), 3, v.data(), down.data(), 2, 1, 2, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(q.data(), 1ull << 31, v.data(), off.data(), 2, 1, 2, 1, out, &n) == RK_ERR_LIMIT);
    EXPECT(rk_gather_scaled_host(nullptr, 3, v.data(), off.data(), 2, 1, 2, 1, out, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_host(q.data(), 3, v.data(), off.data(), 2, 1, 2, 1, nullptr, &n) == RK_ERR_ARG);
    printf("%d vectors, %d random cases, %d failures\n", nvec, nrand, g_bad);
    return g_bad ? 1 : 0;
}
