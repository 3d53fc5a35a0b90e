// rkmh_sketch_json.cpp -- the reader of the JSON sketches `rkmh sketch` writes (rkmh_sketches.cpp: write_sketch_json).  Files that users
// hand in, parsed by hand: nothing here exits, consults the run's policy or calls the library beyond rk_scaled_max_hash, so the file
// links with rk_scaled_host.cpp alone (tools/asan_sketch_json).  A file it cannot make sense of is a plain `false`.
#include <cctype>

#include "rkmh_cli.hpp"

// minimal reader for the files written by write_sketch_json (tolerates whitespace; no general JSON support is claimed)
static bool json_find(const std::string& t, size_t from, size_t to, const char* key, size_t& vpos) {
    std::string pat = std::string("\"") + key + "\"";
    size_t p = t.find(pat, from);
    if (p == std::string::npos || p >= to) return false;
    p = t.find(':', p + pat.size());
    if (p == std::string::npos || p >= to) return false;
    ++p;
    while (p < to && isspace((unsigned char)t[p])) ++p;
    vpos = p;
    return true;
}
static std::string json_string_at(const std::string& t, size_t p) {
    std::string r;
    if (t[p] != '"') return r;
    for (++p; p < t.size() && t[p] != '"'; ++p) {
        if (t[p] == '\\' && p + 1 < t.size()) { ++p; r += t[p]; } else r += t[p];
    }
    return r;
}
bool load_sketch_json(const char* path, LoadedSketches& L, int max_S) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    std::string t;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) t.append(buf, n);
    fclose(f);
    // objects are delimited by their "sketches":{...}} tail; walk by the "alphabet" key that opens each object
    size_t pos = 0;
    std::vector<std::vector<uint64_t>> all;
    std::vector<std::vector<uint32_t>> all_abund;
    while ((pos = t.find("\"alphabet\"", pos)) != std::string::npos) {
        size_t next = t.find("\"alphabet\"", pos + 10);
        size_t end = next == std::string::npos ? t.size() : next;
        size_t v;
        if (!json_find(t, pos, end, "kmer", v)) return false;
        std::vector<int> ks;
        { std::string kk = json_string_at(t, v); char* e = &kk[0]; while (*e) { while (*e == ' ') ++e; if (!*e) break; ks.push_back((int)strtol(e, &e, 10)); } }
        if (L.ks.empty()) L.ks = ks; else if (ks != L.ks) return false;
        { // the policy the sketches were hashed under (absent: a file of an earlier build, which knew the defaults only)
            std::string pol = "default";
            if (json_find(t, pos, end, "hashPolicy", v)) pol = json_string_at(t, v);
            if (L.names.empty()) L.policy = pol; else if (pol != L.policy) return false;
        }
        size_t sp;
        if (!json_find(t, pos, end, "sketches", sp)) return false;
        // "scaled" / "maxHash" (`sketch --scaled`): all objects of a file or none, and all the same
        uint64_t scaled = 0, max_hash = 0;
        if (json_find(t, pos, sp, "scaled", v)) {
            scaled = strtoull(t.c_str() + v, nullptr, 10);
            uint64_t expect = 0;
            if (scaled == 0 || !json_find(t, pos, sp, "maxHash", v) || rk_scaled_max_hash(scaled, &expect) != RK_OK ||
                (max_hash = strtoull(t.c_str() + v, nullptr, 10)) != expect) {
                L.err = "sketch " + std::to_string(all.size()) + ": \"scaled\" must be at least 1 and \"maxHash\" = (2^64 - 1) / scaled";
                return false;
            }
        }
        if (!all.empty() && scaled != L.scaled) { L.err = "its sketches disagree in scaled"; return false; }
        L.scaled = scaled;
        if (!json_find(t, pos, end, "name", v)) return false;
        L.names.push_back(json_string_at(t, v));
        if (!json_find(t, sp, end, "length", v)) return false;
        int S = (int)strtol(t.c_str() + v, nullptr, 10);
        if (scaled) S = 0; // (a scaled sketch's "length" is its own number of hashes)
        else if (L.S == 0) L.S = S; else if (S != L.S) return false;
        if (!json_find(t, sp, end, "hashes", v)) return false;
        std::vector<uint64_t> h;
        const char* q = t.c_str() + v;
        if (*q != '[') return false;
        ++q;
        for (;;) {
            while (*q && (isspace((unsigned char)*q) || *q == ',')) ++q;
            if (*q == ']' || !*q) break;
            char* e;
            h.push_back(strtoull(q, &e, 10));
            if (e == q) return false;
            q = e;
        }
        if (scaled)
            for (size_t j = 0; j < h.size(); ++j)
                if (h[j] == 0 || h[j] > max_hash || (j && h[j] <= h[j - 1])) {
                    L.err = "sketch " + std::to_string(all.size()) + ": the hashes of a scaled sketch are ascending, distinct and at most its maxHash";
                    return false;
                }
        // "abundances" (`sketch --scaled <n> --abund`): parallel to "hashes", every entry 1 .. 2^32 - 1; all objects of a file or none
        std::vector<uint32_t> ab;
        const bool has_abund = scaled && json_find(t, sp, end, "abundances", v);
        if (has_abund) {
            const std::string bad = "sketch " + std::to_string(all.size()) + ": \"abundances\" holds one number of 1 .. 2^32 - 1 for every hash";
            q = t.c_str() + v;
            if (*q != '[') { L.err = bad; return false; }
            ++q;
            for (;;) {
                while (*q && (isspace((unsigned char)*q) || *q == ',')) ++q;
                if (*q == ']' || !*q) break;
                char* e;
                const unsigned long long a = isdigit((unsigned char)*q) ? strtoull(q, &e, 10) : 0;
                if (a < 1 || a > 0xffffffffull) { L.err = bad; return false; }
                ab.push_back((uint32_t)a);
                q = e;
            }
            if (ab.size() != h.size()) { L.err = bad; return false; }
        }
        if (!all.empty() && has_abund != L.has_abund) { L.err = "its sketches disagree in carrying abundances"; return false; }
        L.has_abund = has_abund;
        all_abund.push_back(ab);
        all.push_back(h);
        pos = end;
    }
    if (!all.empty() && L.scaled) {
        L.off.assign(1, 0);
        for (const auto& h : all) {
            if (h.size() > 0x7fffffffull) return false;
            L.lens.push_back((int32_t)h.size());
            L.sk.insert(L.sk.end(), h.begin(), h.end());
            L.off.push_back(L.sk.size());
        }
        for (const auto& a : all_abund) L.abund.insert(L.abund.end(), a.begin(), a.end());
        return true;
    }
    if (all.empty() || L.S <= 0) return false;
    if (max_S > 0 && L.S > max_S) return false; // (before the rows are allocated: L.S tells the caller why)
    L.sk.assign(all.size() * (size_t)L.S, 0);
    for (size_t i = 0; i < all.size(); ++i) {
        if ((int)all[i].size() > L.S) return false;
        L.lens.push_back((int32_t)all[i].size());
        for (size_t j = 0; j < all[i].size(); ++j) L.sk[i * (size_t)L.S + j] = all[i][j];
    }
    return true;
}
