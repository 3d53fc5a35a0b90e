// AddressSanitizer + UBSan over rk_compare_scaled_abund_host, rk_abund_row_sums_host and rk_angular_similarity (rk_scaled_host.cpp; no
// GPU, nothing loaded into Python).  Input: the hand-checked vectors as text (run.sh writes them from tests/golden/wdist_kat.json), one
// per line:
//   P want(4) sums_a(2) sums_b(2) na a... aw... nb b... bw...
//   S dot sumsq_a sumsq_b cosine angular
// Each pair runs on 1 and 4 threads, mirrored and against itself, in arrays of exactly the sizes the call may touch.  Then seeded random
// CSR sets against a set-algebra loop written here, and every refusal.  Prints a summary; exits non-zero on a mismatch.
#include <algorithm>
#include <cmath>
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

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

typedef std::vector<uint64_t> Set;
typedef std::vector<uint32_t> Abund;
struct Sketch { Set v; Abund w; };
typedef unsigned __int128 u128;
static const uint64_t SAT32 = 0xffffffffull, U64 = ~0ull;

// the four fields from a (value -> abundance) map, sums in 128 bits
static void plain_pair(const Sketch& a, const Sketch& b, uint64_t out[4]) {
    std::map<uint64_t, uint32_t> mb;
    for (size_t i = 0; i < b.v.size(); ++i) mb[b.v[i]] = b.w[i];
    u128 dot = 0;
    uint64_t cnt = 0, wa = 0, wb = 0;
    for (size_t i = 0; i < a.v.size(); ++i) {
        auto it = mb.find(a.v[i]);
        if (it == mb.end()) continue;
        ++cnt; dot += (u128)a.w[i] * it->second; wa += a.w[i]; wb += it->second;
    }
    out[0] = cnt; out[1] = dot > (u128)U64 ? U64 : (uint64_t)dot; out[2] = wa; out[3] = wb;
}
static void plain_sums(const Abund& w, uint64_t out[2]) {
    u128 sq = 0;
    uint64_t s = 0;
    for (uint32_t x : w) { s += x; sq += (u128)x * x; }
    out[0] = s; out[1] = sq > (u128)U64 ? U64 : (uint64_t)sq;
}

struct Csr { Set v; Abund w; std::vector<uint64_t> off; };
static Csr csr(const std::vector<Sketch>& rows) {
    Csr c;
    c.off.push_back(0);
    for (const Sketch& r : rows) { c.v.insert(c.v.end(), r.v.begin(), r.v.end()); c.w.insert(c.w.end(), r.w.begin(), r.w.end()); c.off.push_back(c.v.size()); }
    return c;
}
template <class T> static const T* ptr(const std::vector<T>& x) { return x.empty() ? nullptr : x.data(); } // exactly the values there are: a read past them is the sanitizer's to find

static void check_sets(const std::vector<Sketch>& A, const std::vector<Sketch>& B) {
    const Csr a = csr(A), b = csr(B);
    for (int threads : {1, 4}) {
        std::vector<uint64_t> out(A.size() * B.size() * 4, 77);
        EXPECT(rk_compare_scaled_abund_host(ptr(a.v), ptr(a.w), a.off.data(), (int)A.size(), ptr(b.v), ptr(b.w), b.off.data(), (int)B.size(), threads, out.data()) == RK_OK);
        for (size_t i = 0; i < A.size(); ++i)
            for (size_t j = 0; j < B.size(); ++j) {
                uint64_t want[4];
                plain_pair(A[i], B[j], want);
                EXPECT(std::equal(want, want + 4, &out[(i * B.size() + j) * 4]));
            }
    }
    for (const std::vector<Sketch>* S : {&A, &B}) {
        const Csr c = csr(*S);
        std::vector<uint64_t> out(S->size() * 2, 77);
        EXPECT(rk_abund_row_sums_host(ptr(c.w), c.off.data(), (int)S->size(), out.data()) == RK_OK);
        for (size_t i = 0; i < S->size(); ++i) {
            uint64_t want[2];
            plain_sums((*S)[i].w, want);
            EXPECT(want[0] == out[i * 2] && want[1] == out[i * 2 + 1]);
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <vectors.txt>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    int npair = 0, nsim = 0;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string kind;
        s >> kind;
        if (kind == "P") {
            uint64_t want[4], sa[2], sb[2];
            for (auto& x : want) s >> x;
            for (auto& x : sa) s >> x;
            for (auto& x : sb) s >> x;
            Sketch a, b;
            size_t n;
            s >> n; a.v.resize(n); a.w.resize(n);
            for (auto& x : a.v) s >> x;
            for (auto& x : a.w) s >> x;
            s >> n; b.v.resize(n); b.w.resize(n);
            for (auto& x : b.v) s >> x;
            for (auto& x : b.w) s >> x;
            EXPECT(!s.fail());
            uint64_t got[4], g2[2];
            plain_pair(a, b, got);
            EXPECT(std::equal(want, want + 4, got));
            plain_sums(a.w, g2); EXPECT(g2[0] == sa[0] && g2[1] == sa[1]);
            plain_sums(b.w, g2); EXPECT(g2[0] == sb[0] && g2[1] == sb[1]);
            check_sets({a}, {b});
            check_sets({b}, {a});
            check_sets({a, b}, {a, b});
            ++npair;
        } else if (kind == "S") {
            uint64_t dot, sa, sb;
            double cosine, angular, c = -1, a = -1;
            s >> dot >> sa >> sb >> cosine >> angular;
            EXPECT(!s.fail());
            EXPECT(rk_angular_similarity(dot, sa, sb, &c, &a) == RK_OK && c == cosine && std::fabs(a - angular) <= 1e-15);
            ++nsim;
        }
    }
    EXPECT(npair >= 20 && nsim >= 6);
    std::mt19937_64 rng(17);
    int nrand = 0;
    const uint32_t weights[5] = {1, 2, 255, 65535, (uint32_t)SAT32};
    for (int rep = 0; rep < 6; ++rep) {
        Set pool(4000);
        for (auto& x : pool) x = rng() | 1;
        std::sort(pool.begin(), pool.end());
        pool.erase(std::unique(pool.begin(), pool.end()), pool.end());
        auto draw = [&](size_t m) {
            Sketch s;
            for (size_t i = 0; i < m; ++i) s.v.push_back(pool[rng() % pool.size()]);
            std::sort(s.v.begin(), s.v.end());
            s.v.erase(std::unique(s.v.begin(), s.v.end()), s.v.end());
            for (size_t i = 0; i < s.v.size(); ++i) s.w.push_back(weights[rng() % 5]);
            return s;
        };
        const size_t lens[8] = {0, 1, 7, 64, 65, 129, 1000, 3000};
        std::vector<Sketch> A, B;
        for (int i = 0; i < 1 + rep * 3; ++i) A.push_back(draw(lens[rng() % 8]));
        for (int i = 0; i < 17 - rep * 3; ++i) B.push_back(draw(lens[rng() % 8]));
        check_sets(A, B);
        check_sets(A, A);
        ++nrand;
    }
    // a sketch against itself at sums above 2^53, and the edges of the floating point
    double c = -1, a = -1;
    for (uint64_t s : Set{(1ull << 53) + 1, (1ull << 60) + 12345, (1ull << 63) + 1, U64 - 1, U64, 3})
        EXPECT(rk_angular_similarity(s, s, s, &c, &a) == RK_OK && c == 1.0 && a == 1.0);
    EXPECT(rk_angular_similarity(0, 0, 0, &c, &a) == RK_OK && c == 0.0 && a == 0.0);
    EXPECT(rk_angular_similarity(0, 0, 5, &c, &a) == RK_OK && c == 0.0 && a == 0.0);
    EXPECT(rk_angular_similarity(1, 0, 5, &c, &a) == RK_ERR_ARG);
    EXPECT(rk_angular_similarity(1, 5, 0, &c, &a) == RK_ERR_ARG);
    EXPECT(rk_angular_similarity(1, 2, 2, nullptr, nullptr) == RK_OK);
    EXPECT(rk_angular_similarity(1, 2, 2, &c, nullptr) == RK_OK && c == 0.5);
    // refusals
    Set v = {1, 2, 3, 4};
    Abund w = {1, 2, 3, 4}, w0 = {1, 2, 0, 4};
    std::vector<uint64_t> off = {0, 2, 4}, down = {0, 3, 1}, wide = {0, 1ull << 31, 1ull << 31}, none = {0, 0, 0};
    uint64_t out[16], o2[4];
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_OK && out[0] == 2 && out[1] == 5 && out[2] == 3 && out[3] == 3);
    EXPECT(rk_compare_scaled_abund_host(nullptr, nullptr, none.data(), 2, v.data(), w.data(), off.data(), 2, 0, out) == RK_OK && out[0] == 0);
    EXPECT(rk_compare_scaled_abund_host(v.data(), nullptr, off.data(), 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), nullptr, off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(nullptr, w.data(), off.data(), 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), nullptr, 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), w.data(), off.data(), 2, 1, nullptr) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 0, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), w.data(), off.data(), -1, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), down.data(), 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), w.data(), wide.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w0.data(), off.data(), 2, v.data(), w.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_compare_scaled_abund_host(v.data(), w.data(), off.data(), 2, v.data(), w0.data(), off.data(), 2, 1, out) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), off.data(), 2, o2) == RK_OK && o2[0] == 3 && o2[1] == 5 && o2[2] == 7 && o2[3] == 25);
    EXPECT(rk_abund_row_sums_host(nullptr, none.data(), 2, o2) == RK_OK && o2[0] == 0 && o2[3] == 0);
    EXPECT(rk_abund_row_sums_host(nullptr, off.data(), 2, o2) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), nullptr, 2, o2) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), off.data(), 2, nullptr) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), off.data(), 0, o2) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), down.data(), 2, o2) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w.data(), wide.data(), 2, o2) == RK_ERR_ARG);
    EXPECT(rk_abund_row_sums_host(w0.data(), off.data(), 2, o2) == RK_ERR_ARG);
    printf("%d pair vectors, %d similarity vectors, %d random cases, %d failures\n", npair, nsim, nrand, g_bad);
    return g_bad ? 1 : 0;
}
