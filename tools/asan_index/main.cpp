// AddressSanitizer + UBSan over the host-only planning layer of the index build (rkmh_amd/csrc/rk_index_plan.hpp; no GPU, nothing loaded
// into Python).  The layer does not check that a k-mer hashes to its key, so the inputs are synthetic: seeded 64-bit keys and lists that
// give distinct k-mers to key ids.  Every plan is read back with the documented probes, written out plainly here: the fingerprint
// buckets with their IDX_OVF chains, the value forms, the first-level filter, the (base, exceptions) lists of build_kpost, compound
// values, the group filter and the exact maps of narrow and wide k-mers.  Prints a one-line summary; exits non-zero on a mismatch.
#include <cstdio>
#include <random>
#include <set>

#include "rk_index_plan.hpp"

static int g_bad = 0, g_checks = 0;
#define EXPECT(c) do { ++g_checks; if (!(c)) { if (g_bad < 40) fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #c); ++g_bad; } } while (0)

typedef std::map<uint32_t, uint32_t> Post;  // reference -> multiplicity
typedef std::map<uint64_t, Post> Panel;     // key -> its postings

struct Built {
    int R = 0;
    HashTable t;
    rk_index_stats_t st{};
    std::vector<HashPair> pairs;
    std::vector<uint32_t> kpost, kbase;
    std::unordered_map<uint32_t, KList> kremap;
};

static void build(const Panel& p, int R, Built& b) {
    std::vector<std::vector<uint64_t>> rows((size_t)R);
    for (auto& kv : p) for (auto& rm : kv.second) rows[rm.first].insert(rows[rm.first].end(), rm.second, kv.first); // (std::map: ascending keys)
    size_t S = 1;
    for (auto& r : rows) S = std::max(S, r.size());
    std::vector<uint64_t> sk((size_t)R * S, 0);
    std::vector<int32_t> lens((size_t)R);
    for (int r = 0; r < R; ++r) { std::copy(rows[(size_t)r].begin(), rows[(size_t)r].end(), sk.begin() + (size_t)r * S); lens[(size_t)r] = (int32_t)rows[(size_t)r].size(); }
    b.R = R;
    b.pairs = sorted_pairs(sk.data(), lens.data(), R, (int)S);
    EXPECT(fill_hash_table(b.pairs, b.t, b.st).code == RK_OK);
    compact_hash_table(b.t, b.st);
}

// the documented probe: fingerprint, key compare through base[] and the dense entries, IDX_OVF followed to the next bucket
static uint32_t find_key(const HashTable& t, uint64_t h) {
    const uint32_t fp = index_fp(h), mask = t.nb - 1;
    for (uint32_t b = index_bucket(h, mask), steps = 0; steps <= t.nb; b = (b + 1) & mask, ++steps) {
        for (uint32_t q = 0; q < (uint32_t)IDX_SLOTS; ++q) {
            const uint32_t f = t.fpb[(size_t)IDX_SLOTS * b + q] & (q == 0 ? 0x7fffu : 0xffffu);
            if (f != fp) continue;
            const uint32_t id = t.base[b] + q;
            if (id < t.nkeys && ((((uint64_t)t.dense[4 * (size_t)id + 1]) << 32) | t.dense[4 * (size_t)id]) == h) return id;
        }
        if (!(t.fpb[(size_t)IDX_SLOTS * b] & IDX_OVF)) return IDX_NOT_FOUND;
    }
    return IDX_NOT_FOUND;
}
typedef std::vector<std::pair<uint32_t, uint32_t>> Entries;
static Entries list_at(const std::vector<uint32_t>& post, uint32_t off) {
    Entries e;
    for (uint32_t q = 0; q < post[off]; ++q) e.emplace_back(post[off + 1 + 2 * q], post[off + 2 + 2 * q]);
    return e;
}
static Entries hash_value_entries(const HashTable& t, uint32_t v) {
    if (v >> 31) return list_at(t.post, v & 0x7fffffffu);
    if (((v >> 29) & 3u) == 1u) return Entries{{v & 2047u, 1u}, {(v >> 11) & 2047u, 1u}};
    return Entries{{v & 0xFFFFFu, (v >> 20) & 0x1FFu}};
}
static Entries sorted(Entries e) { std::sort(e.begin(), e.end()); return e; }
static Entries entries_of(const Post& p) { return Entries(p.begin(), p.end()); }

static void check_table(const Panel& p, int R, std::mt19937_64& rng) {
    Built b;
    build(p, R, b);
    const HashTable& t = b.t;
    rk_index_stats_t want{};
    uint32_t nb = 256;
    while ((size_t)nb * 250 < p.size() * 100 + 100) nb <<= 1;
    EXPECT(t.nb == nb && t.nkeys == p.size() && t.distinct == p.size() && t.base.size() == (size_t)nb + 1 && t.dense.size() == (p.size() + 1) * 4);
    std::vector<uint32_t> used(nb, 0);
    std::set<uint32_t> over;
    want.keys = (uint32_t)p.size(); want.buckets = nb; want.post_words = 1;
    for (auto& kv : p) {
        const uint64_t h = kv.first;
        const Entries e = entries_of(kv.second);
        const uint32_t id = find_key(t, h);
        EXPECT(id != IDX_NOT_FOUND && t.keyhash[id] == h);
        if (id == IDX_NOT_FOUND) continue;
        const uint32_t v = t.dense[4 * (size_t)id + 2];
        EXPECT(sorted(hash_value_entries(t, v)) == e && t.dense[4 * (size_t)id + 3] == 0);
        const bool single = e.size() == 1 && e[0].second <= 511, pair = e.size() == 2 && e[0].second == 1 && e[1].second == 1 && e[1].first < 2048;
        if (single) { ++(e[0].second == 1 ? want.single_once : want.single_multi); EXPECT(!(v >> 29)); }
        else if (pair) { ++want.pair; EXPECT((v >> 29) == 1u); }
        else {
            ++want.list; want.list_longest = std::max(want.list_longest, (uint32_t)e.size()); want.post_words += 1 + 2 * (uint32_t)e.size();
            EXPECT(v >> 31);
            Entries order = e; // members in (ref & 3, input order) order
            std::stable_sort(order.begin(), order.end(), [](const std::pair<uint32_t, uint32_t>& x, const std::pair<uint32_t, uint32_t>& y) { return (x.first & 3u) < (y.first & 3u); });
            EXPECT(hash_value_entries(t, v) == order);
        }
        uint32_t home = (uint32_t)(h >> 32) & (nb - 1), at = home, chain = 1;
        while (used[at] == 8) { over.insert(at); at = (at + 1) & (nb - 1); ++chain; }
        ++used[at];
        want.longest_chain = std::max(want.longest_chain, chain);
        if (at < home) want.chain_wrapped = 1;
    }
    want.buckets_overflowed = (uint32_t)over.size();
    EXPECT(memcmp(&want, &b.st, sizeof want) == 0);
    for (int i = 0; i < 16; ++i) { uint64_t h = rng() | 1; if (!p.count(h)) EXPECT(find_key(t, h) == IDX_NOT_FOUND); }
    for (uint32_t bk : over) { uint64_t h = ((rng() & ~(uint64_t)(nb - 1)) | bk) << 32 | (uint32_t)rng(); if (!p.count(h)) EXPECT(find_key(t, h) == IDX_NOT_FOUND); } // misses that walk a chain
    // first-level filter: every key passes
    const uint32_t pw = prefilter_words(t.distinct, prefilter_cap_words(t.distinct));
    const std::vector<uint32_t> pre = plan_prefilter(b.pairs, pw);
    EXPECT(pre.size() == pw);
    for (auto& kv : p) EXPECT((pre[index_pre_word(kv.first, pw - 1)] & index_pre_bits(kv.first)) == index_pre_bits(kv.first));
}

static uint64_t fresh_key(std::mt19937_64& rng, const Panel& p) { for (;;) { const uint64_t h = rng(); if (h && !p.count(h)) return h; } }
static uint64_t key_in_bucket(std::mt19937_64& rng, const Panel& p, uint32_t bucket) { // brute force over the seeded stream
    for (;;) { const uint64_t h = rng(); if (h && (((uint32_t)(h >> 32)) & 255u) == bucket && !p.count(h)) return h; }
}
static Post once(std::initializer_list<uint32_t> refs) { Post p; for (uint32_t r : refs) p[r] = 1; return p; }
static Post range(uint32_t lo, uint32_t hi) { Post p; for (uint32_t r = lo; r < hi; ++r) p[r] = 1; return p; }

static Panel forms_panel(std::mt19937_64& rng, int R) {
    Panel p;
    const uint32_t top = (uint32_t)R - 1;
    p[fresh_key(rng, p)] = Post{{0, 1}};
    p[fresh_key(rng, p)] = Post{{top, 1}};
    p[fresh_key(rng, p)] = Post{{0, 2}};
    p[fresh_key(rng, p)] = Post{{top, 0x1FF}};   // the last multiplicity of the 9-bit field
    p[fresh_key(rng, p)] = Post{{0, 0x200}};     // one more: a one-entry list
    if (R >= 12) {
        p[fresh_key(rng, p)] = once({1, 10});
        p[fresh_key(rng, p)] = Post{{2, 1}, {8, 2}};
        p[fresh_key(rng, p)] = once({0, 3, 7});
        p[fresh_key(rng, p)] = once({1, 4, 6, 10});
        p[fresh_key(rng, p)] = once({0, 1, 2, 3, 4, 6, 7});
        p[fresh_key(rng, p)] = Post{{3, 1}, {6, 2}, {10, 1}};
        for (int i = 0; i < 3; ++i) p[fresh_key(rng, p)] = range(0, 12);
        for (int i = 0; i < 40; ++i) p[fresh_key(rng, p)] = Post{{(uint32_t)(rng() % 12), 1}};
    }
    if (R >= 2100) {
        p[fresh_key(rng, p)] = once({5, 2047});  // pair
        p[fresh_key(rng, p)] = once({5, 2048});  // list
        p[fresh_key(rng, p)] = once({2047, 2048});
        p[fresh_key(rng, p)] = once({1, 2, 511});
        p[fresh_key(rng, p)] = once({1, 2, 512});
        Post far; for (uint32_t r = 3; r < 2099; r += 61) far[r] = 1;
        p[fresh_key(rng, p)] = far;
        p[fresh_key(rng, p)] = Post{{2099, 1}};
    }
    return p;
}
static Panel chains_panel(std::mt19937_64& rng) { // 256 buckets: groups that overflow, one in the last bucket (the chain wraps to bucket 0)
    Panel p;
    const Post posts[5] = {Post{{0, 1}}, Post{{1, 1}}, once({0, 1}), Post{{0, 2}}, Post{{1, 3}}};
    int n = 0;
    for (auto g : {std::make_pair(255u, 19), std::make_pair(0u, 8), std::make_pair(100u, 17), std::make_pair(37u, 9)})
        for (int i = 0; i < g.second; ++i) p[key_in_bucket(rng, p, g.first)] = posts[n++ % 5];
    while (p.size() < 400) p[fresh_key(rng, p)] = posts[n++ % 5];
    return p;
}

// ---- build_kpost ---------------------------------------------------------------------------------------------------------------------
static void append(std::vector<uint32_t>& post, const Post& l) { post.push_back((uint32_t)l.size()); for (auto& rm : l) { post.push_back(rm.first); post.push_back(rm.second); } }
static Post variant(Post base, std::initializer_list<uint32_t> minus, std::initializer_list<uint32_t> plus) { for (uint32_t r : minus) base.erase(r); for (uint32_t r : plus) base[r] = 1; return base; }
// a kpost list back to its plain content: header (entries | (base + 1) << 24), the base's members, the exceptions
static Entries expand_kpost(const std::vector<uint32_t>& kpost, const std::vector<uint32_t>& kbase, uint32_t off) {
    const uint32_t head = kpost[off], n = head & 0xFFFFFFu, b = head >> 24;
    std::map<uint32_t, int64_t> m;
    if (b) for (uint32_t q = 0; q < kbase[2 * (b - 1) + 1]; ++q) m[kbase[kbase[2 * (b - 1)] + q]] += 1;
    for (uint32_t q = 0; q < n; ++q) { const uint32_t r = kpost[off + 1 + 2 * q], mu = kpost[off + 2 + 2 * q]; m[r] += (mu >> 31) ? -(int64_t)(mu & 0x7fffffffu) : (int64_t)mu; }
    Entries e;
    for (auto& x : m) { EXPECT(x.second >= 0); if (x.second > 0) e.emplace_back(x.first, (uint32_t)x.second); }
    return e;
}
// the inline form: tag 111, base, count, eight 10-bit fields of reference and sign
static Entries expand_inline(const std::vector<uint32_t>& kbase, uint32_t ix, uint32_t iy, uint32_t iw) {
    const uint32_t b = (ix >> 26) & 7u, nex = (ix >> 22) & 15u;
    const uint32_t f[8] = {ix & 1023u, (ix >> 10) & 1023u, iy & 1023u, (iy >> 10) & 1023u, (iy >> 20) & 1023u, iw & 1023u, (iw >> 10) & 1023u, (iw >> 20) & 1023u};
    std::map<uint32_t, int64_t> m;
    for (uint32_t q = 0; q < kbase[2 * b + 1]; ++q) m[kbase[kbase[2 * b] + q]] += 1;
    EXPECT((ix >> 29) == 7u && nex <= 8);
    for (uint32_t q = 0; q < nex && q < 8; ++q) m[f[q] & 511u] += (f[q] & 512u) ? -1 : 1;
    Entries e;
    for (auto& x : m) { EXPECT(x.second == 0 || x.second == 1); if (x.second > 0) e.emplace_back(x.first, 1u); }
    return e;
}
struct KpostOut { std::vector<uint32_t> kpost, kbase; std::unordered_map<uint32_t, KList> remap; rk_index_stats_t st{}; };
static void check_kpost(const std::vector<uint32_t>& post, int R, int nbases, KpostOut& o) {
    build_kpost(post, R, nbases, o.kpost, o.kbase, o.remap, o.st);
    size_t lists = 0;
    for (size_t off = 1; off < post.size(); off += 1 + 2 * (size_t)post[off], ++lists) {
        EXPECT(o.remap.count((uint32_t)off) == 1); // remap covers every list offset
        if (!o.remap.count((uint32_t)off)) continue;
        const KList kl = o.remap.at((uint32_t)off);
        const Entries e = sorted(list_at(post, (uint32_t)off));
        EXPECT(expand_kpost(o.kpost, o.kbase, kl.plain) == e && (o.kpost[kl.plain] >> 24) == 0);
        EXPECT(expand_kpost(o.kpost, o.kbase, kl.enc) == e);
        if (kl.ix) EXPECT(expand_inline(o.kbase, kl.ix, kl.iy, kl.iw) == e && (o.kpost[kl.enc] >> 24) != 0);
    }
    EXPECT(o.remap.size() == lists);
    uint32_t kept = 0;
    for (int b = 0; b < KBASE_MAX; ++b) kept += o.kbase[2 * (size_t)b + 1] != 0;
    EXPECT(kept == o.st.bases_kept);
}
static void kpost_cases() {
    const Post A = range(0, 24), B = range(24, 36);
    std::vector<uint32_t> post(1, 0u);
    std::vector<uint32_t> at; // offsets of the variants: distance 0, 1, 8, 9 from A
    for (int i = 0; i < 60; ++i) { if (i == 0) at.push_back((uint32_t)post.size()); append(post, A); }
    for (int i = 0; i < 40; ++i) append(post, B);
    at.push_back((uint32_t)post.size()); append(post, variant(A, {}, {36}));
    at.push_back((uint32_t)post.size()); append(post, variant(A, {1, 2, 3, 4}, {24, 25, 36, 37}));
    at.push_back((uint32_t)post.size()); append(post, variant(A, {5, 6, 8, 9}, {26, 27, 28, 36, 37}));
    Post twice = A; twice[3] = 2;
    const uint32_t at_twice = (uint32_t)post.size(); append(post, twice); // not simple: never against a base
    append(post, once({1, 2, 39}));
    // (with a slot free a list at distance > 6 from A is far from every base and becomes one itself: two slots, so A and B take them)
    KpostOut all;
    check_kpost(post, 40, KBASE_MAX, all);
    EXPECT(all.st.bases_kept == 4 && !((all.remap.at(at[2]).ix >> 22) & 15u));
    KpostOut o;
    check_kpost(post, 40, 2, o);
    EXPECT(o.st.bases_kept == 2 && o.st.bases_dropped_by_share_rule == 0);
    EXPECT(o.remap.at(at[0]).ix && o.remap.at(at[1]).ix && o.remap.at(at[2]).ix && ((o.remap.at(at[2]).ix >> 22) & 15u) == 8); // 0, 1, 8 exceptions: inside the value
    EXPECT(!o.remap.at(at[3]).ix && o.remap.at(at[3]).enc != o.remap.at(at[3]).plain && (o.kpost[o.remap.at(at[3]).enc] & 0xFFFFFFu) == 9); // 9: a (base, exceptions) list
    EXPECT(o.remap.at(at_twice).enc == o.remap.at(at_twice).plain && !o.remap.at(at_twice).ix);
    KpostOut none; // RKMH_KBASES=0, and more than 0xFFFF references: no bases
    check_kpost(post, 40, 0, none);
    EXPECT(none.st.bases_kept == 0 && none.st.bases_dropped_by_share_rule == 0);
    KpostOut many;
    check_kpost(post, 0x10000, KBASE_MAX, many);
    EXPECT(many.st.bases_kept == 0);
    // an exception reference >= 512 gets no inline form
    std::vector<uint32_t> big(1, 0u);
    for (int i = 0; i < 30; ++i) append(big, range(0, 16));
    const uint32_t at_big = (uint32_t)big.size(); append(big, variant(range(0, 16), {}, {550}));
    const uint32_t at_small = (uint32_t)big.size(); append(big, variant(range(0, 16), {}, {511}));
    KpostOut ob;
    check_kpost(big, 600, KBASE_MAX, ob);
    EXPECT(ob.st.bases_kept == 1 && !ob.remap.at(at_big).ix && ob.remap.at(at_big).enc != ob.remap.at(at_big).plain && ob.remap.at(at_small).ix);
    // the 5 % rule: one base of 8 references saves 7 of its 8 postings; ballast of x one-entry lists (not simple): kept while 140 >= 8 + x
    for (int x : {20, 132, 133, 4000}) {
        std::vector<uint32_t> pl(1, 0u);
        append(pl, range(0, 8));
        for (int i = 0; i < x; ++i) append(pl, Post{{9, 2}});
        KpostOut op;
        check_kpost(pl, 12, KBASE_MAX, op);
        EXPECT(op.st.bases_kept == (x <= 132 ? 1u : 0u) && op.st.bases_dropped_by_share_rule == (x <= 132 ? 0u : 1u));
    }
}

// ---- compound values, group filter, maps ---------------------------------------------------------------------------------------------
// a compound value back to the postings the kernels count from it
static Entries expand_value(const Built& b, const std::vector<uint32_t>& vals, uint32_t id, int& form) {
    if (id < (uint32_t)b.R) { form = 0; return Entries{{id, 1u}}; }
    const uint32_t* cv = &vals[4 * (size_t)(id - (uint32_t)b.R)];
    if (!(cv[0] >> 31)) { form = ((cv[0] >> 29) & 3u) == 1u ? 2 : 1; return sorted(hash_value_entries(b.t, cv[0])); }
    if ((cv[0] >> 29) == 7u) { form = 4; EXPECT(expand_kpost(b.kpost, b.kbase, cv[2]) == expand_inline(b.kbase, cv[0], cv[1], cv[3])); return expand_inline(b.kbase, cv[0], cv[1], cv[3]); }
    if ((cv[0] >> 30) == 3u) {
        form = 3;
        const uint32_t n = ((cv[0] >> 27) & 7u) + 3u, f[6] = {cv[0] & 511u, (cv[0] >> 9) & 511u, (cv[0] >> 18) & 511u, cv[1] & 511u, (cv[1] >> 9) & 511u, (cv[1] >> 18) & 511u};
        Entries e;
        for (uint32_t q = 0; q < n && q < 6; ++q) e.emplace_back(f[q], 1u);
        return sorted(e);
    }
    form = (cv[0] & 0x3fffffffu) != cv[2] ? 5 : 6;
    EXPECT(expand_kpost(b.kpost, b.kbase, cv[2]) == expand_kpost(b.kpost, b.kbase, cv[0] & 0x3fffffffu) && (b.kpost[cv[2]] >> 24) == 0);
    return expand_kpost(b.kpost, b.kbase, cv[0] & 0x3fffffffu);
}
static void check_filter(const KmerList& l, const KmerMaps& m) {
    const int k = l.k;
    const bool wide = k > 16;
    const uint64_t cm = (1ull << (2 * (k - 3))) - 1ull;
    EXPECT(m.f4.size() == (size_t)4 * m.nsect && m.nsect >= 256 && m.nsect % 8 == 0);
    for (uint32_t i = 0; i < l.found(); ++i)
        for (int o = 0; o < 2; ++o) {
            const uint64_t X = o ? (wide ? packed_revcomp64(l.kmer(i), k) : (uint64_t)packed_revcomp((uint32_t)l.kmer(i), k)) : l.kmer(i);
            const uint32_t bits = kf4_bits(wide ? kw_fold(X) : (uint32_t)X);
            for (uint32_t j = 0; j < 4; ++j) {
                const uint64_t core = (X >> (2 * (3 - j))) & cm;
                if (!wide) EXPECT((uint32_t)core == (((uint32_t)X >> (2 * (3 - j))) & kf4_core_mask(k)));
                EXPECT((m.f4[(size_t)kf4_sector(wide ? kw_fold(core) : (uint32_t)core, m.nsect) * 4 + j] & bits) == bits);
            }
        }
}
// the documented probe of km1: bucket from km1_y, remainder and hop tag, full flag followed.  -> cell index or ~0
static uint32_t find_narrow(const KmerMaps& m, int k, uint32_t kmer, uint32_t& id) {
    const uint32_t kbits = 2u * (uint32_t)k, r = kbits - m.b, vb = km1_vbits(k, m.b), vmask = (1u << vb) - 1u, y = km1_y(kmer, k);
    uint32_t bk = r ? y >> r : y;
    const uint32_t rem = r ? y & ((1u << r) - 1u) : 0u;
    for (uint32_t hop = 0; hop < (1u << KM1_HB); ++hop, bk = (bk + 1) & ((1u << m.b) - 1u)) {
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t cell = m.cells[(size_t)bk * 4 + q];
            if ((cell & vmask) != vmask && (cell >> (vb + 1)) == (rem | (hop << r))) { id = cell & vmask; return bk * 4 + q; }
        }
        if (!(m.cells[(size_t)bk * 4 + 3] & (1u << vb))) break;
    }
    return ~0u;
}
// the wide map: bucket and tag from kw_y, the key number leads to kkeys, the full k-mer settles it
static uint32_t find_wide(const KmerMaps& m, int k, uint64_t kmer, uint32_t& vid) {
    const uint32_t kbits = 2u * (uint32_t)k;
    const uint64_t y = kw_y(kmer, k);
    uint32_t bk = (uint32_t)(y >> (kbits - m.b));
    const uint32_t tag = (uint32_t)(y >> (kbits - m.b - KW_TAG)) & ((1u << KW_TAG) - 1u);
    for (uint32_t hop = 0; hop < (1u << KM1_HB); ++hop, bk = (bk + 1) & ((1u << m.b) - 1u)) {
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t cell = m.cells[(size_t)bk * 4 + q], num = cell & KW_EMPTY;
            if (num == KW_EMPTY || (cell >> (KW_IDBITS + 1)) != ((hop << KW_TAG) | tag)) continue;
            if (m.kkeys[2 * (size_t)num] == (uint32_t)kmer && (m.kkeys[2 * (size_t)num + 1] & 0xFFu) == (uint32_t)(kmer >> 32)) { vid = m.kkeys[2 * (size_t)num + 1] >> 8; return num; }
        }
        if (!(m.cells[(size_t)bk * 4 + 3] & (1u << KW_IDBITS))) break;
    }
    return ~0u;
}
static uint64_t revcomp_any(uint64_t v, int k) { return k > 16 ? packed_revcomp64(v, k) : (uint64_t)packed_revcomp((uint32_t)v, k); }
// `found` distinct k-mers, one per strand pair, the first a palindrome; key ids 0, 1, .. with a zero-hash entry now and then
static KmerList make_list(std::mt19937_64& rng, int k, uint32_t found, uint32_t nkeys, std::set<uint64_t>& used) {
    KmerList l; l.k = k;
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    uint64_t pal = 0; // A..AT..T reads the same on both strands (k even); odd k has no palindrome
    for (int i = 0; i < k; ++i) pal |= (uint64_t)(i < k / 2 ? 0 : 2) << (2 * i);
    uint32_t slot = 0;
    for (uint32_t i = 0; i < found; ++i) {
        uint64_t v = (i == 0 && k % 2 == 0) ? pal : rng() & mask;
        while (used.count(v) || used.count(revcomp_any(v, k))) v = rng() & mask;
        used.insert(v);
        if (i == 0 && k % 2 == 0) EXPECT(revcomp_any(v, k) == v);
        l.w.push_back((uint32_t)v);
        if (k > 16) l.w.push_back((uint32_t)(v >> 32));
        l.w.push_back((i % 97 == 3 || slot >= nkeys) ? IDX_NOT_FOUND : slot++);
    }
    return l;
}
static uint32_t want_start_bits(uint32_t found, uint32_t b, uint32_t bmax) { while (b < bmax && (double)found > 0.65 * 4.0 * (double)(1ull << b)) ++b; return b; }

static void check_maps(const Built& b, std::mt19937_64& rng, int k, uint32_t found) {
    std::set<uint64_t> used;
    const KmerList l = make_list(rng, k, found, (uint32_t)b.t.nkeys, used);
    std::vector<uint8_t> seen(b.t.nkeys + 1, 0);
    EXPECT(l.found() == found && one_preimage(l, b.t.nkeys, seen));
    rk_index_stats_t st{};
    ValueTable vt{b.R, b.t, b.kremap, st, {}, {}};
    KmerMaps m;
    const bool wide = k > 16;
    const bool ok = wide ? plan_wide_maps(l, vt, m) : plan_narrow_maps(l, vt, 0.0, m);
    EXPECT(ok);
    if (!ok) return;
    check_filter(l, m);
    const uint32_t kbits = 2u * (uint32_t)k;
    EXPECT(m.cells.size() == (size_t)4 << m.b && m.longest_hop < (1u << KM1_HB));
    uint32_t want_b = wide ? want_start_bits(found, 12, 26) : want_start_bits(found, std::min(kbits, 12u), std::min(kbits, 28u));
    if (!wide) while ((uint64_t)b.R + vt.vals.size() / 4 + 2 > (uint64_t)((1u << km1_vbits(k, want_b)) - 1u)) ++want_b; // ids need more bits
    // the smallest the rule allows: from there on, the first size at which every key finds one of four cells within eight buckets
    auto fits = [&](uint32_t bits) {
        std::vector<uint8_t> fill((size_t)1 << bits, 0);
        for (uint32_t i = 0; i < found; ++i) {
            uint32_t bk = wide ? (uint32_t)(kw_y(l.kmer(i), k) >> (kbits - bits)) : (kbits > bits ? km1_y((uint32_t)l.kmer(i), k) >> (kbits - bits) : km1_y((uint32_t)l.kmer(i), k)), hop = 0;
            while (hop < 8 && fill[bk] == 4) { bk = (bk + 1) & ((1u << bits) - 1u); ++hop; }
            if (hop == 8) return false;
            ++fill[bk];
        }
        return true;
    };
    while (!fits(want_b)) ++want_b;
    EXPECT(m.b == want_b);
    if (!wide && k == 16 && b.R > 255) EXPECT(m.b > want_start_bits(found, 12, 28)); // (this table's ids do not fit vbits at the rule's first size)
    uint32_t forms[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < found; ++i) {
        uint32_t id = 0, at;
        const uint32_t slot = l.slot(i);
        if (wide) {
            at = find_wide(m, k, l.kmer(i), id);
            EXPECT(at == i && m.kslots[i] == (slot == IDX_NOT_FOUND ? 0u : slot) && m.kkeys[2 * (size_t)i] == (uint32_t)l.kmer(i));
            if (slot == IDX_NOT_FOUND) { EXPECT(id == KW_VID_ZERO); continue; }
        } else {
            at = find_narrow(m, k, (uint32_t)l.kmer(i), id);
            EXPECT(at != ~0u && at == m.km1cells[2 * (size_t)i] && m.km1cells[2 * (size_t)i + 1] == slot); // cell_of names that cell
            if (slot == IDX_NOT_FOUND) { EXPECT(id == m.vmask - 1u); continue; }
        }
        int form = -1;
        EXPECT(id < (uint32_t)b.R + vt.vals.size() / 4);
        if (id >= (uint32_t)b.R + vt.vals.size() / 4) continue;
        EXPECT(expand_value(b, vt.vals, id, form) == sorted(hash_value_entries(b.t, b.t.dense[4 * (size_t)slot + 2])));
        ++forms[form];
    }
    EXPECT(forms[0] == st.kv_reference && forms[1] == st.kv_single_multi && forms[2] == st.kv_pair && forms[3] == st.kv_inline_list &&
           forms[4] == st.kv_base_inline && forms[5] == st.kv_base_list && forms[6] == st.kv_plain_list);
    const uint64_t mask = (1ull << (2 * k)) - 1ull;
    for (int i = 0; i < 64; ++i) {
        uint64_t v = rng() & mask;
        if (used.count(v)) continue;
        uint32_t id;
        EXPECT((wide ? find_wide(m, k, v, id) : find_narrow(m, k, (uint32_t)v, id)) == ~0u);
    }
}
// a table of nkeys keys whose postings take every form, the family lists among them
static void map_table(std::mt19937_64& rng, int R, size_t nkeys, Built& b) {
    Panel p = forms_panel(rng, R);
    if (R >= 40) {
        for (int i = 0; i < 60; ++i) p[fresh_key(rng, p)] = range(0, 24);
        p[fresh_key(rng, p)] = variant(range(0, 24), {}, {36});
        p[fresh_key(rng, p)] = variant(range(0, 24), {5, 6, 8, 9}, {26, 27, 28, 36, 37});
    }
    while (p.size() < nkeys) p[fresh_key(rng, p)] = Post{{(uint32_t)(rng() % (uint64_t)R), 1}};
    build(p, R, b);
    b.st = rk_index_stats_t{};
    build_kpost(b.t.post, R, KBASE_MAX, b.kpost, b.kbase, b.kremap, b.st);
}

int main() {
    std::mt19937_64 rng(20261);
    for (int R : {1, 12, 2100}) check_table(forms_panel(rng, R), R, rng);
    check_table(chains_panel(rng), 2, rng);
    { Panel big = forms_panel(rng, 12); while (big.size() < 3000) big[fresh_key(rng, big)] = Post{{(uint32_t)(rng() % 12), 1}}; check_table(big, 12, rng); } // more than 256 buckets
    // the word count of the first-level filter: 4096 words, doubling while a key has fewer than 32 bits, up to the cap
    EXPECT(prefilter_words(0, 262144) == 4096 && prefilter_words(4096, 262144) == 4096 && prefilter_words(4097, 262144) == 8192 && prefilter_words(8193, 262144) == 16384);
    EXPECT(prefilter_words(262144, 262144) == 262144 && prefilter_words(262145, 262144) == 262144 && prefilter_words(5000000, 524288) == 524288 && prefilter_words(100000, 4096) == 4096);
    EXPECT(prefilter_cap_words(2000000) == 262144 && prefilter_cap_words(2000001) == 524288);
    kpost_cases();
    Built b40, b2100;
    map_table(rng, 40, 40100, b40);
    map_table(rng, 2100, 12000, b2100);
    EXPECT(b40.st.bases_kept >= 1);
    const uint32_t step = 10649; // 0.65 * 4 * 2^12 = 10649.6: the last list a map of 2^12 buckets takes
    int nmaps = 0;
    for (int k : {8, 12, 13, 16, 17, 20})
        for (uint32_t found : {0u, 1u, 5u, step, step + 1, k == 8 ? 30000u : 40000u}) { check_maps(b40, rng, k, found); ++nmaps; } // (4^8 k-mers are 32 896 strand pairs)
    for (int k : {13, 16, 17}) { check_maps(b2100, rng, k, 9000); ++nmaps; } // narrow: R + values does not fit vbits at the first b
    // refusals
    {
        std::set<uint64_t> used;
        KmerList l = make_list(rng, 16, 50, 1000, used);
        std::vector<uint8_t> seen(b40.t.nkeys + 1, 0);
        KmerList twice = l; twice.w[2 * 7 + 1] = twice.w[2 * 2 + 1]; // one key id named twice
        EXPECT(!one_preimage(twice, b40.t.nkeys, seen));
        std::fill(seen.begin(), seen.end(), 0);
        KmerList beyond = l; beyond.w[2 * 9 + 1] = (uint32_t)b40.t.nkeys; // a key id >= nkeys
        EXPECT(!one_preimage(beyond, b40.t.nkeys, seen));
        std::fill(seen.begin(), seen.end(), 0);
        EXPECT(one_preimage(l, b40.t.nkeys, seen) && !one_preimage(l, b40.t.nkeys, seen)); // across the sizes of a run: seen[] is shared
        // wide: a value id >= KW_VID_ZERO does not fit kkeys
        uint32_t pair_slot = 0;
        while (pair_slot < b40.t.nkeys && ((b40.t.dense[4 * (size_t)pair_slot + 2] >> 29) != 1u)) ++pair_slot;
        EXPECT(pair_slot < b40.t.nkeys);
        KmerList w = make_list(rng, 17, 4, 0, used);
        w.w[3 * 1 + 2] = pair_slot;
        for (int R : {(int)KW_VID_ZERO - 1, (int)KW_VID_ZERO}) {
            rk_index_stats_t st{};
            ValueTable vt{R, b40.t, b40.kremap, st, {}, {}};
            KmerMaps m;
            EXPECT(plan_wide_maps(w, vt, m) == (R < (int)KW_VID_ZERO));
        }
    }
    // a Panel whose postings overflow is beyond a test's memory: the refusal's code and text are checked where they are made
    printf("%d checks, %d maps, %d failures\n", g_checks, nmaps, g_bad);
    return g_bad ? 1 : 0;
}
