// AddressSanitizer + UBSan over rk_merge_scaled_abund and rk_gather_scaled_abund_host (rk_scaled_host.cpp; no GPU, nothing loaded into
// Python).  Input: the hand-checked vectors as text (run.sh writes them from tests/golden/abund_kat.json), one per line:
//   G min_shared max_rounds nrows rows(4 each)... wunique(nrows)... nq q... abund... nref (len values...)...
//   M max_hash nparts (len values... abund...)... nwant values... abund...
// Each gather runs on 1 and 4 threads in arrays of exactly the sizes the call may touch.  Then seeded random sets against plain loops
// written here, and every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
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
typedef std::vector<uint32_t> Abund;
static const uint64_t SAT = 0xffffffffull;

// the rows and the weights by set algebra on (value -> abundance) maps
static void plain(const Set& q, const Abund& a, const std::vector<Set>& refs, int min_shared, int max_rounds, std::vector<int32_t>& rows, Set& wunique) {
    rows.clear(); wunique.clear();
    std::map<uint64_t, uint32_t> alive;
    for (size_t i = 0; i < q.size(); ++i) alive[q[i]] = a[i];
    for (int t = 0; t < max_rounds; ++t) {
        int best = -1; size_t best_n = 0;
        for (size_t r = 0; r < refs.size(); ++r) {
            size_t n = 0;
            for (uint64_t x : refs[r]) n += alive.count(x);
            if (best < 0 || n > best_n) { best = (int)r; best_n = n; }
        }
        if (best < 0 || best_n < (size_t)min_shared) break;
        Set total;
        std::set_intersection(q.begin(), q.end(), refs[best].begin(), refs[best].end(), std::back_inserter(total));
        uint64_t w = 0;
        for (uint64_t x : refs[best]) { auto it = alive.find(x); if (it != alive.end()) { w += it->second; alive.erase(it); } }
        rows.insert(rows.end(), {(int32_t)best, (int32_t)best_n, (int32_t)total.size(), (int32_t)alive.size()});
        wunique.push_back(w);
    }
}

static void check_gather(const Set& q, const Abund& a, const std::vector<Set>& refs, int min_shared, int max_rounds, const std::vector<int32_t>& want, const Set& want_w) {
    Set values;
    std::vector<uint64_t> off(1, 0);
    for (const Set& r : refs) { values.insert(values.end(), r.begin(), r.end()); off.push_back(values.size()); }
    Set qq(q); // exactly nq values and nq abundances: a read past them is the sanitizer's to find
    Abund aa(a);
    uint64_t wtotal = 0, got_w = 0;
    for (uint32_t x : a) wtotal += x;
    for (int threads : {1, 4}) {
        const size_t rows = std::min<size_t>((size_t)max_rounds, refs.size());
        std::vector<int32_t> out(rows * 4, -7), plain_out(rows * 4, -7);
        Set wu(rows, 77);
        int n = -1, pn = -1;
        int32_t none4 = 0; uint64_t none = 0;
        EXPECT(rk_gather_scaled_abund_host(qq.empty() ? nullptr : qq.data(), aa.empty() ? nullptr : aa.data(), qq.size(), values.empty() ? nullptr : values.data(),
                                           off.data(), (int)refs.size(), min_shared, max_rounds, threads, out.empty() ? &none4 : out.data(),
                                           wu.empty() ? &none : wu.data(), &n) == RK_OK);
        EXPECT(rk_gather_scaled_host(qq.empty() ? nullptr : qq.data(), qq.size(), values.empty() ? nullptr : values.data(), off.data(), (int)refs.size(), min_shared,
                                     max_rounds, threads, plain_out.empty() ? &none4 : plain_out.data(), &pn) == RK_OK);
        EXPECT(n >= 0 && (size_t)n * 4 == want.size() && pn == n);
        if (n < 0 || (size_t)n * 4 != want.size()) continue;
        EXPECT(std::equal(want.begin(), want.end(), out.begin()) && std::equal(want.begin(), want.end(), plain_out.begin()));
        EXPECT(std::equal(want_w.begin(), want_w.end(), wu.begin()));
        for (size_t t = (size_t)n; t < rows; ++t) EXPECT(wu[t] == 0); // zeroed as far as rows can be written
        got_w = 0;
        for (int t = 0; t < n; ++t) got_w += wu[(size_t)t];
        EXPECT(got_w <= wtotal);
    }
}

static void plain_merge(const std::vector<std::pair<Set, Abund>>& parts, uint64_t max_hash, Set& v, Abund& a) {
    std::map<uint64_t, uint64_t> tot;
    for (const auto& p : parts)
        for (size_t i = 0; i < p.first.size(); ++i)
            if (p.first[i] != 0 && p.first[i] <= max_hash) tot[p.first[i]] = std::min(tot[p.first[i]] + p.second[i], SAT);
    v.clear(); a.clear();
    for (const auto& kv : tot) { v.push_back(kv.first); a.push_back((uint32_t)kv.second); }
}

static void check_merge(const std::vector<std::pair<Set, Abund>>& parts, uint64_t max_hash, const Set& want_v, const Abund& want_a) {
    Set values; Abund abund;
    std::vector<uint64_t> off(1, 0);
    for (const auto& p : parts) { values.insert(values.end(), p.first.begin(), p.first.end()); abund.insert(abund.end(), p.second.begin(), p.second.end()); off.push_back(values.size()); }
    uint64_t* ov = nullptr; uint32_t* oa = nullptr; uint64_t n = ~0ull;
    EXPECT(rk_merge_scaled_abund(values.empty() ? nullptr : values.data(), abund.empty() ? nullptr : abund.data(), off.data(), (int)parts.size(), max_hash, &ov, &oa, &n) == RK_OK);
    EXPECT(n == want_v.size() && ov && oa);
    if (n == want_v.size() && ov && oa) EXPECT(std::equal(want_v.begin(), want_v.end(), ov) && std::equal(want_a.begin(), want_a.end(), oa));
    uint64_t* pv = nullptr; uint64_t pn = 0; // the values of the plain merge
    EXPECT(rk_merge_scaled(values.empty() ? nullptr : values.data(), off.data(), (int)parts.size(), max_hash, &pv, &pn) == RK_OK);
    EXPECT(pn == n && pv && ov && std::equal(pv, pv + pn, ov));
    rk_free(ov); rk_free(oa); rk_free(pv);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int ngather = 0, nmerge = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string kind;
        long long n;
        s >> kind;
        if (kind == "G") {
            long long min_shared, max_rounds, nrows;
            s >> min_shared >> max_rounds >> nrows;
            std::vector<int32_t> want((size_t)nrows * 4);
            for (auto& x : want) s >> x;
            Set want_w((size_t)nrows);
            for (auto& x : want_w) s >> x;
            s >> n;
            Set q((size_t)n);
            Abund a((size_t)n);
            for (auto& x : q) s >> x;
            for (auto& x : a) s >> x;
            s >> n;
            std::vector<Set> refs((size_t)n);
            for (auto& r : refs) { s >> n; r.resize((size_t)n); for (auto& x : r) s >> x; }
            EXPECT(!s.fail());
            check_gather(q, a, refs, (int)min_shared, (int)max_rounds, want, want_w);
            std::vector<int32_t> rows; Set w;
            plain(q, a, refs, (int)min_shared, (int)max_rounds, rows, w);
            EXPECT(rows == want && w == want_w);
            ++ngather;
        } else {
            uint64_t max_hash;
            s >> max_hash >> n;
            std::vector<std::pair<Set, Abund>> parts((size_t)n);
            for (auto& p : parts) { s >> n; p.first.resize((size_t)n); p.second.resize((size_t)n); for (auto& x : p.first) s >> x; for (auto& x : p.second) s >> x; }
            s >> n;
            Set want_v((size_t)n); Abund want_a((size_t)n);
            for (auto& x : want_v) s >> x;
            for (auto& x : want_a) s >> x;
            EXPECT(!s.fail());
            check_merge(parts, max_hash, want_v, want_a);
            Set v; Abund a;
            plain_merge(parts, max_hash, v, a);
            EXPECT(v == want_v && a == want_a);
            ++nmerge;
        }
    }
    EXPECT(ngather >= 14 && nmerge >= 10);
    std::mt19937_64 rng(11);
    int nrand = 0;
    for (int nref : {1, 9, 65, 300}) {
        Set pool(3000);
        for (auto& x : pool) x = rng() | 1;
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        auto draw = [&](size_t m) { Set s; for (size_t i = 0; i < m; ++i) s.push_back(pool[rng() % pool.size()]); std::sort(s.begin(), s.end()); s.erase(std::unique(s.begin(), s.end()), s.end()); return s; };
        auto weights = [&](size_t m) { Abund a(m); for (auto& x : a) { const uint64_t r = rng() % 100; x = r < 80 ? 1u : r < 98 ? (uint32_t)(2 + rng() % 500) : (uint32_t)SAT; } return a; };
        std::vector<Set> refs;
        for (int r = 0; r < nref; ++r) refs.push_back(draw((size_t[]){0, 1, 7, 64, 65, 129, 1000}[rng() % 7]));
        Set q = draw(1500);
        for (uint64_t x = 2; x < 400; x += 2) q.push_back(x); // foreign (even) values
        std::sort(q.begin(), q.end());
        const Abund a = weights(q.size());
        for (int min_shared : {1, 20}) for (int max_rounds : {1, 5, 1000}) {
            std::vector<int32_t> rows; Set w;
            plain(q, a, refs, min_shared, max_rounds, rows, w);
            check_gather(q, a, refs, min_shared, max_rounds, rows, w);
            ++nrand;
        }
        std::vector<std::pair<Set, Abund>> parts; // the references as the parts of a union
        for (const Set& r : refs) parts.emplace_back(r, weights(r.size()));
        for (uint64_t max_hash : {(uint64_t)~0ull, pool[pool.size() / 3], (uint64_t)0}) {
            Set v; Abund m;
            plain_merge(parts, max_hash, v, m);
            check_merge(parts, max_hash, v, m);
            ++nrand;
        }
    }
    // refusals
    Set q = {1, 2, 3}, v = {1, 2, 3, 4};
    Abund a = {1, 2, 3}, a0 = {1, 0, 3}, va = {1, 1, 1, 1}, va0 = {1, 1, 0, 1};
    std::vector<uint64_t> off = {0, 2, 4}, down = {0, 3, 1};
    Set unsorted = {2, 1, 3}, zero = {0, 1, 2};
    int32_t out[8]; uint64_t wu[2]; int n = 0;
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_OK && n == 2 && wu[0] == 3 && wu[1] == 3);
    EXPECT(rk_gather_scaled_abund_host(q.data(), nullptr, 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a0.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, nullptr, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 0, 1, 1, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 2, 0, 1, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 2, 1, 0, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(unsorted.data(), a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(zero.data(), a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), down.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 1ull << 31, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_LIMIT);
    EXPECT(rk_gather_scaled_abund_host(nullptr, a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, out, wu, &n) == RK_ERR_ARG);
    EXPECT(rk_gather_scaled_abund_host(q.data(), a.data(), 3, v.data(), off.data(), 2, 1, 2, 1, nullptr, wu, &n) == RK_ERR_ARG);
    uint64_t* ov = nullptr; uint32_t* oa = nullptr; uint64_t on = 0;
    EXPECT(rk_merge_scaled_abund(v.data(), nullptr, off.data(), 2, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(nullptr, va.data(), off.data(), 2, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va0.data(), off.data(), 2, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), down.data(), 2, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), nullptr, 2, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), off.data(), -1, ~0ull, &ov, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), off.data(), 2, ~0ull, nullptr, &oa, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), off.data(), 2, ~0ull, &ov, nullptr, &on) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(v.data(), va.data(), off.data(), 2, ~0ull, &ov, &oa, nullptr) == RK_ERR_ARG);
    EXPECT(rk_merge_scaled_abund(nullptr, nullptr, nullptr, 0, ~0ull, &ov, &oa, &on) == RK_OK && on == 0);
    rk_free(ov); rk_free(oa);
    printf("%d gather vectors, %d merge vectors, %d random cases, %d failures\n", ngather, nmerge, nrand, g_bad);
    return g_bad ? 1 : 0;
}
