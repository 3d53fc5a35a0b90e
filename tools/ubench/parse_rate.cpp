// tools/ubench/parse_rate.cpp -- how fast the host read parser reads a FASTQ of fixed 150-base records: rk_reader_next to the end of
// the file (1 << 20 records per batch) and rk_parse_files, on the plain file (mapped, block front end) and on its gzip copy (inflater
// thread + block front end).  Median and spread (min .. max) of 7 runs after 2 warm-ups.  Stand-alone, host code only:
//   C=rkmh_amd/csrc; SRCS="$C/rk_pool.cpp $C/rk_parse.cpp $C/rk_parse_blocks.cpp $C/rk_bgzf.cpp"
//   g++ -O3 -std=c++17 -Iinclude -o /tmp/parse_rate tools/ubench/parse_rate.cpp $SRCS -lz -lpthread -ldl
//   RKMH_PARSE_THREADS=12 /tmp/parse_rate [reads = 4000000] [keep]
// The files go to $TMPDIR (/tmp) and are reused when they are there; they are removed at the end unless `keep` is given, which is
// what a comparison of two builds wants: alternate the two programs on the same files.
#include "../../include/rkmh_amd.h"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <sys/stat.h>
#include <unistd.h>

extern "C" void rk__set_error(const char* m) { fprintf(stderr, "parser error: %s\n", m); }

static const size_t READ_LEN = 150;

static void write_files(const std::string& plain, const std::string& gz, long reads) {
    FILE* f = fopen(plain.c_str(), "wb");
    gzFile g = gzopen(gz.c_str(), "wb1");
    if (!f || !g) { fprintf(stderr, "cannot write %s / %s\n", plain.c_str(), gz.c_str()); exit(2); }
    uint64_t x = 0x9e3779b97f4a7c15ull;
    std::string chunk;
    for (long i = 0; i < reads; ++i) {
        char name[32];
        chunk.append(name, (size_t)snprintf(name, sizeof name, "@r%ld\n", i));
        const size_t at = chunk.size();
        chunk.resize(at + 2 * READ_LEN + 4);
        char* s = &chunk[at];
        char* q = s + READ_LEN + 3;
        for (size_t j = 0; j < READ_LEN; ++j) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            s[j] = "ACGT"[x & 3];
            q[j] = (char)(35 + ((x >> 8) % 40));
        }
        s[READ_LEN] = '\n'; s[READ_LEN + 1] = '+'; s[READ_LEN + 2] = '\n'; q[READ_LEN] = '\n';
        if (chunk.size() >= ((size_t)8 << 20) || i + 1 == reads) {
            if (fwrite(chunk.data(), 1, chunk.size(), f) != chunk.size() || gzwrite(g, chunk.data(), (unsigned)chunk.size()) <= 0) { fprintf(stderr, "write failed\n"); exit(2); }
            chunk.clear();
        }
    }
    fclose(f);
    gzclose(g);
}

static long read_batches(const char* path) {
    rk_reader* r = nullptr;
    if (rk_reader_open(path, &r) != RK_OK) exit(3);
    long n = 0;
    for (;;) {
        rk_seqset b;
        if (rk_reader_next(r, 1 << 20, 0, &b) != RK_OK) exit(3);
        const long got = (long)b.nseq;
        rk_seqset_free(&b);
        if (got == 0) break;
        n += got;
    }
    rk_reader_close(r);
    return n;
}

static long parse_whole(const char* path) {
    const char* paths[1] = {path};
    rk_seqset s;
    if (rk_parse_files(paths, 1, &s) != RK_OK) exit(3);
    const long n = (long)s.nseq;
    rk_seqset_free(&s);
    return n;
}

static void measure(const char* what, long (*fn)(const char*), const char* path, long reads) {
    std::vector<double> t;
    for (int run = 0; run < 9; ++run) {
        const auto t0 = std::chrono::steady_clock::now();
        const long n = fn(path);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (n != reads) { fprintf(stderr, "%s: %ld records, expected %ld\n", what, n, reads); exit(4); }
        if (run >= 2) t.push_back(dt); // two warm-ups
    }
    std::sort(t.begin(), t.end());
    printf("%-28s median %.4f s  spread %.4f s (%.4f .. %.4f)  %.1f M reads/s\n", what, t[3], t[6] - t[0], t[0], t[6], (double)reads / t[3] / 1e6);
}

int main(int argc, char** argv) {
    const long reads = argc > 1 ? atol(argv[1]) : 4000000;
    const bool keep = argc > 2 && strcmp(argv[2], "keep") == 0;
    const char* tmp = getenv("TMPDIR");
    const std::string plain = std::string(tmp && *tmp ? tmp : "/tmp") + "/rk_parse_rate_" + std::to_string(reads) + ".fq", gz = plain + ".gz";
    struct stat st;
    if (stat(plain.c_str(), &st) != 0 || stat(gz.c_str(), &st) != 0) write_files(plain, gz, reads);
    setenv("RKMH_GZ_BLOCKS", "2", 1); // the gzip copy through the inflater thread and the block front end, whatever its size
    measure("plain  rk_reader_next", read_batches, plain.c_str(), reads);
    measure("plain  rk_parse_files", parse_whole, plain.c_str(), reads);
    measure("gzip   rk_reader_next", read_batches, gz.c_str(), reads);
    measure("gzip   rk_parse_files", parse_whole, gz.c_str(), reads);
    if (!keep) { unlink(plain.c_str()); unlink(gz.c_str()); }
    return 0;
}
