// The host baseline of tools/bench_scaled.py: |a_i & b_j| for every pair of CSR sets, as a plain two-pointer loop on OpenMP threads.
// Build: g++ -O3 -fopenmp -o tools/ubench/scaled_cpu tools/ubench/scaled_cpu.cpp
// Usage: scaled_cpu <in.bin> <out.bin> <threads> <runs>
//   in.bin   int64 na, nb; uint64 a_off[na + 1]; uint64 b_off[nb + 1]; uint64 a[a_off[na]]; uint64 b[b_off[nb]]
//   out.bin  int32 shared[na * nb] of the last run
// Prints "cpu_seconds <median> <min> <max>".
#include <omp.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static inline int32_t shared_count(const uint64_t* A, uint64_t la, const uint64_t* B, uint64_t lb) {
    int32_t n = 0;
    uint64_t i = 0, j = 0;
    while (i < la && j < lb) {
        const uint64_t x = A[i], y = B[j];
        n += x == y;
        i += x <= y;
        j += y <= x;
    }
    return n;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s <in.bin> <out.bin> <threads> <runs>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int64_t hdr[2];
    if (fread(hdr, 8, 2, f) != 2 || hdr[0] < 1 || hdr[1] < 1) return 2;
    const int64_t na = hdr[0], nb = hdr[1];
    std::vector<uint64_t> ao((size_t)na + 1), bo((size_t)nb + 1);
    if (fread(ao.data(), 8, ao.size(), f) != ao.size() || fread(bo.data(), 8, bo.size(), f) != bo.size()) return 2;
    std::vector<uint64_t> a((size_t)ao[(size_t)na]), b((size_t)bo[(size_t)nb]);
    if (fread(a.data(), 8, a.size(), f) != a.size() || fread(b.data(), 8, b.size(), f) != b.size()) return 2;
    fclose(f);
    std::vector<int32_t> out((size_t)na * (size_t)nb);
    const int threads = atoi(argv[3]), runs = std::max(1, atoi(argv[4]));
    omp_set_num_threads(threads);
    std::vector<double> t;
    for (int r = 0; r < runs; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic, 4) collapse(2)
        for (int64_t i = 0; i < na; ++i)
            for (int64_t j0 = 0; j0 < nb; j0 += 64)   // a row of a stays in L1 / L2 across 64 rows of b
                for (int64_t j = j0; j < std::min(nb, j0 + 64); ++j)
                    out[(size_t)i * (size_t)nb + (size_t)j] = shared_count(&a[ao[(size_t)i]], ao[(size_t)i + 1] - ao[(size_t)i], &b[bo[(size_t)j]], bo[(size_t)j + 1] - bo[(size_t)j]);
        t.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(t.begin(), t.end());
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) { perror(argv[2]); return 2; }
    fclose(f);
    printf("cpu_seconds %.6f %.6f %.6f\n", t[t.size() / 2], t.front(), t.back());
    return 0;
}
