// The host baseline of tools/bench_pairs.py: the four counts of rk_compare_sketches for every pair, as a plain two-pointer loop on
// OpenMP threads.  Build: g++ -O3 -fopenmp -o tools/ubench/pairs_cpu tools/ubench/pairs_cpu.cpp
// Usage: pairs_cpu <in.bin> <out.bin> <threads> <runs>
//   in.bin   int32 na, nb, S, 0; uint64 a[na * S]; uint64 b[nb * S]; int32 alens[na]; int32 blens[nb]
//   out.bin  int32 out4[na * nb * 4] of the last run
// Prints "cpu_seconds <median> <min> <max>".
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static inline void pair_counts(const uint64_t* A, int la, const uint64_t* B, int lb, int S, int32_t* out) {
    int shared = 0, sdist = 0, common = 0, denom = 0, i = 0, j = 0;
    uint64_t prev = 0;
    while (i < la || j < lb) {
        const bool ha = i < la, hb = j < lb;
        if (!(ha && hb) && denom >= S) break;
        const uint64_t va = ha ? A[i] : 0, vb = hb ? B[j] : 0;
        const bool ta = ha && (!hb || va <= vb), tb = hb && (!ha || vb <= va), both = ta && tb;
        const uint64_t v = ta ? va : vb;
        const bool fresh = v != prev && v != 0;
        prev = v;
        shared += both && v != 0;
        sdist += both && fresh;
        if (fresh && denom < S) { ++denom; common += both; }
        i += ta; j += tb;
    }
    out[0] = shared; out[1] = sdist; out[2] = common; out[3] = denom;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s <in.bin> <out.bin> <threads> <runs>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4) return 2;
    const int na = hdr[0], nb = hdr[1], S = hdr[2];
    std::vector<uint64_t> a((size_t)na * S), b((size_t)nb * S);
    std::vector<int32_t> al((size_t)na), bl((size_t)nb), out((size_t)na * nb * 4);
    if (fread(a.data(), 8, a.size(), f) != a.size() || fread(b.data(), 8, b.size(), f) != b.size() || fread(al.data(), 4, al.size(), f) != al.size() ||
        fread(bl.data(), 4, bl.size(), f) != bl.size()) return 2;
    fclose(f);
    const int threads = atoi(argv[3]), runs = std::max(1, atoi(argv[4]));
    omp_set_num_threads(threads);
    std::vector<double> t;
    for (int r = 0; r < runs; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 4) collapse(2)
        for (int i = 0; i < na; ++i)
            for (int j0 = 0; j0 < nb; j0 += 64)   // a row of a stays in L1 / L2 across 64 rows of b
                for (int j = j0; j < std::min(nb, j0 + 64); ++j)
                    pair_counts(&a[(size_t)i * S], std::min(std::max(al[i], 0), S), &b[(size_t)j * S], std::min(std::max(bl[j], 0), S), S, &out[((size_t)i * nb + j) * 4]);
        t.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { perror(argv[2]); return 2; }
    fclose(f);
    printf("cpu_seconds %.6f %.6f %.6f\n", t[t.size() / 2], t.front(), t.back());
    return 0;
}
