// AddressSanitizer + UBSan over rk_multigather_scaled_host (rk_scaled_host.cpp; no GPU, nothing loaded into Python).
// Seeded random batches -- empty queries, repeated queries, queries without a candidate -- in arrays of exactly the sizes the call may
// touch, on 1 and 4 threads, plain and with abundances, against rk_gather_scaled_host / rk_gather_scaled_abund_host query by query;
// then every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "rkmh_amd.h"

static std::string g_err;
extern "C" void rk__set_error(const char* msg) { g_err = msg ? msg : ""; }
extern "C" void rk_free(void* p) { free(p); }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

typedef std::vector<uint64_t> Set;

static void check(const std::vector<Set>& refs, const std::vector<Set>& queries, bool weighted, int min_shared, int max_rounds, std::mt19937_64& rng) {
    Set rv, qv;
    std::vector<uint64_t> ro(1, 0), qo(1, 0);
    for (const Set& r : refs) { rv.insert(rv.end(), r.begin(), r.end()); ro.push_back(rv.size()); }
    for (const Set& q : queries) { qv.insert(qv.end(), q.begin(), q.end()); qo.push_back(qv.size()); }
    std::vector<uint32_t> qa(qv.size());
    for (auto& a : qa) a = rng() % 5 == 0 ? 0xffffffffu : 1 + (uint32_t)(rng() % 500);
    const int nref = (int)refs.size(), cap = std::min(max_rounds, nref);
    for (int threads : {1, 4}) {
        int32_t* rows = nullptr;
        uint64_t* wu = nullptr;
        uint64_t n = ~0ull;
        std::vector<uint64_t> off(queries.size() + 1, ~0ull);
        EXPECT(rk_multigather_scaled_host(rv.empty() ? nullptr : rv.data(), ro.data(), nref, qv.empty() ? nullptr : qv.data(), weighted ? qa.data() : nullptr, qo.data(),
                                          (int64_t)queries.size(), min_shared, max_rounds, threads, &rows, &wu, off.data(), &n) == RK_OK);
        EXPECT(rows && (!weighted || wu) && off[0] == 0 && off.back() == n);
        if (!rows) continue;
        for (size_t i = 0; i < queries.size(); ++i) {
            std::vector<int32_t> out((size_t)cap * 4 + 4, -7);
            std::vector<uint64_t> w((size_t)cap + 1, 7);
            int m = -1;
            const Set& q = queries[i];
            const uint32_t* a = qa.data() + qo[i];
            if (weighted) EXPECT(rk_gather_scaled_abund_host(q.empty() ? nullptr : q.data(), q.empty() ? nullptr : a, q.size(), rv.data(), ro.data(), nref, min_shared, max_rounds, 1, out.data(), w.data(), &m) == RK_OK);
            else EXPECT(rk_gather_scaled_host(q.empty() ? nullptr : q.data(), q.size(), rv.data(), ro.data(), nref, min_shared, max_rounds, 1, out.data(), &m) == RK_OK);
            EXPECT(m >= 0 && off[i + 1] - off[i] == (uint64_t)m);
            if (m < 0 || off[i + 1] - off[i] != (uint64_t)m) continue;
            EXPECT(std::equal(out.begin(), out.begin() + (size_t)m * 4, rows + off[i] * 4));
            if (weighted) EXPECT(std::equal(w.begin(), w.begin() + m, wu + off[i]));
        }
        rk_free(rows);
        if (weighted) rk_free(wu);
    }
}

int main() {
    std::mt19937_64 rng(11);
    int ncase = 0;
    for (int nref : {1, 9, 65, 300}) {
        Set pool(3000);
        for (auto& x : pool) x = rng() | 1;
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        auto draw = [&](size_t m) { Set s; for (size_t i = 0; i < m; ++i) s.push_back(pool[rng() % pool.size()]); std::sort(s.begin(), s.end()); s.erase(std::unique(s.begin(), s.end()), s.end()); return s; };
        std::vector<Set> refs, queries;
        for (int r = 0; r < nref; ++r) refs.push_back(draw((size_t[]){0, 1, 7, 64, 65, 129, 1000}[rng() % 7]));
        Set foreign;
        for (uint64_t x = 2; x < 400; x += 2) foreign.push_back(x); // (even: no reference holds them)
        queries.push_back(draw(1500));
        queries.push_back(Set());
        queries.push_back(foreign);
        queries.push_back(queries[0]);
        for (int i = 0; i < 5; ++i) queries.push_back(draw((size_t[]){1, 9, 64, 700}[rng() % 4]));
        queries.push_back(Set());
        for (bool weighted : {false, true})
            for (int min_shared : {1, 20})
                for (int max_rounds : {1, 5, 1000}) { check(refs, queries, weighted, min_shared, max_rounds, rng); ++ncase; }
    }
    // refusals
    Set v = {1, 2, 3, 4}, q = {1, 2, 3, 9}, unsorted = {2, 1, 3, 9}, zero = {0, 1, 3, 9}, twice = {1, 1, 3, 9};
    std::vector<uint64_t> off = {0, 2, 4}, down = {0, 3, 1};
    std::vector<uint32_t> ab = {1, 2, 3, 4}, ab0 = {1, 0, 3, 4};
    int32_t* rows = nullptr; uint64_t* wu = nullptr; uint64_t n = 0, ro[3];
#define MG(rv_, roff_, nref_, qv_, qa_, qoff_, nq_, ms_, mr_) rk_multigather_scaled_host(rv_, roff_, nref_, qv_, qa_, qoff_, nq_, ms_, mr_, 1, &rows, &wu, ro, &n)
    EXPECT(MG(v.data(), off.data(), 0, q.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), nullptr, off.data(), 0, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), nullptr, off.data(), 2, 0, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), nullptr, off.data(), 2, 1, 0) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, unsorted.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, zero.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, twice.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), ab0.data(), off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), down.data(), 2, q.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), nullptr, down.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 1ll << 31, q.data(), nullptr, off.data(), 2, 1, 1) == RK_ERR_LIMIT);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), nullptr, off.data(), 1ll << 31, 1, 1) == RK_ERR_LIMIT);
    EXPECT(MG(v.data(), off.data(), 2, nullptr, nullptr, off.data(), 2, 1, 1) == RK_ERR_ARG);
    EXPECT(rk_multigather_scaled_host(v.data(), off.data(), 2, q.data(), ab.data(), off.data(), 2, 1, 1, 1, &rows, nullptr, ro, &n) == RK_ERR_ARG);
    EXPECT(rk_multigather_scaled_host(v.data(), off.data(), 2, q.data(), nullptr, off.data(), 2, 1, 1, 1, &rows, &wu, nullptr, &n) == RK_ERR_ARG);
    EXPECT(MG(v.data(), off.data(), 2, q.data(), ab.data(), off.data(), 2, 1, 5) == RK_OK && n == 2 && ro[1] == 1 && ro[2] == 2 && wu[0] == 3 && wu[1] == 3); // {1, 2} from {1, 2}; {3} of {3, 9} from {3, 4}
    rk_free(rows); rk_free(wu);
    printf("%d random cases, %d failures\n", ncase, g_bad);
    return g_bad ? 1 : 0;
}
