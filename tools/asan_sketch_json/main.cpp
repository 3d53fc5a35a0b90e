// AddressSanitizer + UBSan over the reader of sketch files (rkmh_sketch_json.cpp: load_sketch_json; no GPU, nothing loaded into
// Python).  Every argument is a file; each is loaded twice, without a size limit as `stream -R` does and with RK_MAX_SKETCH as dist and
// gather do, and answered by one line: the path, then `ok` with what was read, or the refusal.  What is read is checked for the shape
// the callers rely on (rows inside sk, offsets ascending).  Exits non-zero when that shape is wrong; the sanitizers speak for themselves.
#include "rkmh_cli.hpp"

extern "C" void rk__set_error(const char*) {} // what rk_scaled_host.cpp asks of the library around it
extern "C" void rk_free(void* p) { free(p); }

static int g_bad = 0;
#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

static void load(const char* path, int max_S) {
    LoadedSketches L;
    if (!load_sketch_json(path, L, max_S)) {
        printf("%s\t%s\n", path, L.err.empty() ? "cannot load" : L.err.c_str());
        return;
    }
    const size_t n = L.names.size();
    EXPECT(n > 0 && L.lens.size() == n && L.ks.size() >= 1);
    if (L.scaled) {
        EXPECT(L.S == 0 && L.off.size() == n + 1 && L.off[0] == 0 && L.off[n] == L.sk.size());
        for (size_t i = 0; i < n; ++i) EXPECT(L.off[i] <= L.off[i + 1] && L.off[i + 1] - L.off[i] == (uint64_t)L.lens[i]);
    } else {
        EXPECT(L.S > 0 && (max_S == 0 || L.S <= max_S) && L.sk.size() == n * (size_t)L.S);
        for (size_t i = 0; i < n; ++i) EXPECT(L.lens[i] >= 0 && L.lens[i] <= L.S);
    }
    uint64_t sum = 0; // every value and every name is read once
    for (uint64_t v : L.sk) sum += v;
    for (const std::string& s : L.names) sum += s.size();
    printf("%s\tok\t%zu sketches, k %d, S %d, scaled %llu, policy %s, sum %llu\n", path, n, L.ks[0], L.S, (unsigned long long)L.scaled, L.policy.c_str(), (unsigned long long)sum);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s <sketches.json> ...\n", argv[0]); return 2; }
    for (int i = 1; i < argc; ++i) { load(argv[i], 0); load(argv[i], RK_MAX_SKETCH); }
    return g_bad ? 1 : 0;
}
