// AddressSanitizer + UBSan over rk_search_scaled_host and rk_search_min_count (rk_scaled_host.cpp; no GPU, nothing loaded into Python).
// Input: the hand-checked vectors as text (run.sh writes them from tests/golden/search_kat.json), one per line:
//   min_shared has_q_min nhits hits(3 each)... nq [q_min...] (len values...)... nref (len values...)...
// Each runs on 1 and 4 threads in arrays of exactly the sizes the call may touch.  Then seeded random sets against a plain loop
// written here, the threshold rule against its definition, and every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
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

static std::vector<int32_t> plain(const std::vector<Set>& refs, const std::vector<Set>& queries, int min_shared, const std::vector<int32_t>& q_min) {
    std::vector<int32_t> hits;
    for (size_t i = 0; i < queries.size(); ++i)
        for (size_t j = 0; j < refs.size(); ++j) {
            Set both;
            std::set_intersection(queries[i].begin(), queries[i].end(), refs[j].begin(), refs[j].end(), std::back_inserter(both));
            const int thr = q_min.empty() ? min_shared : std::max(min_shared, q_min[i]);
            if ((int)both.size() >= thr) hits.insert(hits.end(), {(int32_t)i, (int32_t)j, (int32_t)both.size()});
        }
    return hits;
}

static void csr(const std::vector<Set>& rows, Set& values, std::vector<uint64_t>& off) {
    off.assign(1, 0);
    for (const Set& r : rows) { values.insert(values.end(), r.begin(), r.end()); off.push_back(values.size()); }
}

static void check(const std::vector<Set>& refs, const std::vector<Set>& queries, int min_shared, const std::vector<int32_t>& q_min, const std::vector<int32_t>& want) {
    Set rv, qv; // exactly the values the offsets cover: a read past them is the sanitizer's to find
    std::vector<uint64_t> ro, qo;
    csr(refs, rv, ro);
    csr(queries, qv, qo);
    for (int threads : {1, 4}) {
        rk_search_hit* hits = nullptr;
        uint64_t n = ~0ull;
        EXPECT(rk_search_scaled_host(rv.empty() ? nullptr : rv.data(), ro.data(), (int64_t)refs.size(), qv.empty() ? nullptr : qv.data(), qo.data(),
                                     (int64_t)queries.size(), min_shared, q_min.empty() ? nullptr : q_min.data(), threads, &hits, &n) == RK_OK);
        EXPECT(hits != nullptr && n * 3 == want.size());
        if (hits && n * 3 == want.size()) EXPECT(std::equal(want.begin(), want.end(), &hits[0].query));
        rk_free(hits);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    static_assert(sizeof(rk_search_hit) == 12, "a hit is three int32");
    std::ifstream in(argv[1]);
    std::string line;
    int nvec = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        long long min_shared, has_q_min, nhits, n;
        s >> min_shared >> has_q_min >> nhits;
        std::vector<int32_t> want((size_t)nhits * 3);
        for (auto& x : want) s >> x;
        s >> n;
        std::vector<Set> queries((size_t)n);
        std::vector<int32_t> q_min(has_q_min ? (size_t)n : 0);
        for (auto& x : q_min) s >> x;
        for (auto& q : queries) { s >> n; q.resize((size_t)n); for (auto& x : q) s >> x; }
        s >> n;
        std::vector<Set> refs((size_t)n);
        for (auto& r : refs) { s >> n; r.resize((size_t)n); for (auto& x : r) s >> x; }
        EXPECT(!s.fail());
        check(refs, queries, (int)min_shared, q_min, want);
        EXPECT(plain(refs, queries, (int)min_shared, q_min) == want);
        ++nvec;
    }
    EXPECT(nvec >= 20);
    std::mt19937_64 rng(11);
    int nrand = 0;
    for (int nref : {1, 9, 65, 300}) {
        Set pool(3000);
        for (auto& x : pool) x = rng() | 1;
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        auto draw = [&](size_t m) { Set s; for (size_t i = 0; i < m; ++i) s.push_back(pool[rng() % pool.size()]); std::sort(s.begin(), s.end()); s.erase(std::unique(s.begin(), s.end()), s.end()); return s; };
        const size_t lens[] = {0, 1, 7, 64, 65, 129, 1000};
        std::vector<Set> refs, queries;
        for (int r = 0; r < nref; ++r) refs.push_back(draw(lens[rng() % 7]));
        for (int q = 0; q < 20; ++q) queries.push_back(draw(lens[rng() % 7]));
        std::vector<int32_t> q_min;
        for (int q = 0; q < 20; ++q) q_min.push_back(1 + (int32_t)(rng() % 40));
        for (int min_shared : {1, 20}) {
            check(refs, queries, min_shared, {}, plain(refs, queries, min_shared, {}));
            check(refs, queries, min_shared, q_min, plain(refs, queries, min_shared, q_min));
            nrand += 2;
        }
    }
    // the threshold rule against its definition
    for (double x : {0.0, 0.1, 0.5, 0.7, 1.0})
        for (uint64_t len = 0; len <= 20; ++len) {
            int32_t t = -1, want = 0;
            while (len && (double)want / (double)len < x) ++want;
            EXPECT(rk_search_min_count(x, len, &t) == RK_OK && t == want);
        }
    // refusals
    Set v = {1, 2, 3, 4}, q = {2, 3, 9};
    std::vector<uint64_t> off = {0, 2, 4}, qoff = {0, 3}, down = {0, 3, 1};
    int32_t zero[1] = {0}, t = 0;
    rk_search_hit* hits = nullptr;
    uint64_t n = 0;
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 0, q.data(), qoff.data(), 1, 1, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), qoff.data(), 0, 1, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), qoff.data(), 1, 0, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), qoff.data(), 1, 1, zero, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), down.data(), 2, q.data(), qoff.data(), 1, 1, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), down.data(), 2, 1, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(nullptr, off.data(), 2, q.data(), qoff.data(), 1, 1, nullptr, 1, &hits, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), qoff.data(), 1, 1, nullptr, 1, nullptr, &n) == RK_ERR_ARG);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 1ll << 31, q.data(), qoff.data(), 1, 1, nullptr, 1, &hits, &n) == RK_ERR_LIMIT);
    EXPECT(rk_search_scaled_host(v.data(), off.data(), 2, q.data(), qoff.data(), 1ll << 31, 1, nullptr, 1, &hits, &n) == RK_ERR_LIMIT);
    EXPECT(rk_search_min_count(-0.5, 3, &t) == RK_ERR_ARG && rk_search_min_count(1.5, 3, &t) == RK_ERR_ARG && rk_search_min_count(std::nan(""), 3, &t) == RK_ERR_ARG);
    EXPECT(rk_search_min_count(0.5, 3, nullptr) == RK_ERR_ARG && rk_search_min_count(0.5, 1ull << 31, &t) == RK_ERR_LIMIT);
    EXPECT(hits == nullptr);
    printf("%d vectors, %d random cases, %d failures\n", nvec, nrand, g_bad);
    return g_bad ? 1 : 0;
}
