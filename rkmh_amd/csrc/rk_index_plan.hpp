// rk_index_plan.hpp -- the host half of an index build (rk_index.hip, build_index): every resident structure the classify readers decode,
// laid out in plain vectors.  No HIP runtime call, no rk_ctx, no environment variable: sizes and knobs come in as arguments, a
// refusal goes back as a value (PlanError, or false where the hash-space kernels simply stay in charge), and only the driver uploads
// or fails.  tools/asan_index runs all of it under ASan + UBSan without a GPU.
//   sorted_pairs        the (hash, reference) pairs of the sketches, by hash
//   fill_hash_table, compact_hash_table   fingerprint buckets with their overflow chains and the value forms; base[] and the dense entries
//   plan_prefilter      the first-level filter in front of the bucket table
//   build_kpost         the posting lists of the k-mer-space kernel: identical lists once, (base, exceptions) forms
//   sort_kmer_list, one_preimage   the enumeration list in its reproducible order; every key found by exactly one k-mer
//   ValueTable          value ids and compound values of the k-mer-space kernels
//   plan_kf4, place_cells, plan_narrow_maps, plan_wide_maps   group filter and exact map of one k-mer size
#pragma once
#include "../../include/rkmh_amd.h"
#include "rk_device.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <unordered_map>
#include <utility>
#include <vector>

using namespace rk; // (rk_device.hpp; as rk_api_internal.hpp does)

struct PlanError { int code = RK_OK; const char* msg = ""; };

// ---- pairs ---------------------------------------------------------------------------------------------------------------------
struct HashPair { uint64_t h; uint32_t ref; };
// by (hash, reference): the pairs come in reference order, so a stable radix sort on the hash alone (four 16-bit digits) does it
inline std::vector<HashPair> sorted_pairs(const uint64_t* sk, const int32_t* lens, int R, int S) {
    std::vector<HashPair> pairs;
    for (int r = 0; r < R; ++r)
        for (int j = 0; j < lens[r]; ++j) {
            const uint64_t h = sk[(size_t)r * S + j];
            if (h != 0) pairs.push_back(HashPair{h, (uint32_t)r});
        }
    std::vector<HashPair> tmp(pairs.size());
    std::vector<uint32_t> cnt((size_t)1 << 16);
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 16 * pass;
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (const HashPair& p : pairs) ++cnt[(size_t)((p.h >> sh) & 0xFFFFu)];
        uint32_t run = 0;
        for (uint32_t& v : cnt) { const uint32_t here = v; v = run; run += here; }
        for (const HashPair& p : pairs) tmp[cnt[(size_t)((p.h >> sh) & 0xFFFFu)]++] = p;
        pairs.swap(tmp);
    }
    return pairs;
}

// ---- hash-space table ----------------------------------------------------------------------------------------------------------
struct HashTable {
    uint32_t nb = 256, lg = 8;       // buckets and their log2
    size_t distinct = 0, nkeys = 0;
    std::vector<uint16_t> fpb;       // [nb * IDX_SLOTS] fingerprints; bit 15 of a bucket's slot 0: IDX_OVF
    std::vector<uint32_t> kv;        // [nb * IDX_SLOTS * 4] {key lo, key hi, value, 0} per slot: what compact_hash_table reads
    std::vector<uint32_t> base;      // [nb + 1] keys stored in earlier buckets: key id = base[bucket] + position in the bucket
    std::vector<uint32_t> dense;     // [(nkeys + 1) * 4] {key lo, key hi, value, 0} per key id
    std::vector<uint32_t> post;      // posting lists: [off] = count, then count x (reference, multiplicity)
    std::vector<uint64_t> keyhash;   // [nkeys] the hash of each key id
};
typedef std::vector<std::pair<uint32_t, uint32_t>> RefGroup; // (reference, multiplicity) of one hash, by reference

// bucketed table: 8 slots per bucket, at most 2.5 keys per bucket on average (P(more than 8) ~ 0.1 %)
inline void bucket_count(size_t distinct, uint32_t& nb, uint32_t& lg) {
    nb = 256; lg = 8;
    const size_t load_pct = 250;
    while ((size_t)nb * load_pct < distinct * 100 + 100) { nb <<= 1; ++lg; }
}
// Every hash's references grouped into (reference, multiplicity), its value chosen -- a reference with its multiplicity, a pair of
// references, or a list appended to `post` -- and the key stored in the first free slot of its bucket or, down the IDX_OVF chain, of a
// later one.  One function on locals, moved into `t` at the end: the loop runs once per key of the index.
inline PlanError fill_hash_table(const std::vector<HashPair>& pairs, HashTable& t, rk_index_stats_t& stats) {
    rk_index_stats_t st = stats;
    size_t distinct = 0;
    for (size_t i = 0; i < pairs.size(); ++i) if (i == 0 || pairs[i].h != pairs[i - 1].h) ++distinct;
    uint32_t nb, lg;
    bucket_count(distinct, nb, lg);
    const uint32_t size = nb * IDX_SLOTS, bmask = nb - 1;
    std::vector<uint16_t> fpb(size, 0);
    std::vector<uint32_t> kv((size_t)size * 4, 0); // {key lo, key hi, value, 0} per slot
    std::vector<uint32_t> post;
    post.push_back(0);
    size_t i = 0;
    RefGroup grp;
    while (i < pairs.size()) {
        size_t j = i;
        grp.clear();
        while (j < pairs.size() && pairs[j].h == pairs[i].h) {
            size_t k = j; while (k < pairs.size() && pairs[k].h == pairs[i].h && pairs[k].ref == pairs[j].ref) ++k;
            grp.emplace_back(pairs[j].ref, (uint32_t)(k - j));
            j = k;
        }
        uint32_t v;
        if (grp.size() == 1 && grp[0].second <= 0x1FFu) {
            v = grp[0].first | (grp[0].second << 20);
            ++(grp[0].second == 1 ? st.single_once : st.single_multi);
        } else if (grp.size() == 2 && grp[0].second == 1 && grp[1].second == 1 && grp[0].first < 2048 && grp[1].first < 2048) {
            v = (1u << 29) | grp[0].first | (grp[1].first << 11);
            ++st.pair;
        } else {
            if (post.size() + 1 + 2 * grp.size() >= 0x3fffffffull) return PlanError{RK_ERR_LIMIT, "postings overflow"}; // (offsets stay below 2^30: the k-mer-space value table uses the two top bits)
            v = 0x80000000u | (uint32_t)post.size();
            ++st.list; st.list_longest = std::max(st.list_longest, (uint32_t)grp.size());
            post.push_back((uint32_t)grp.size());
            // Order inside a list is free.  The fused kernels walk a list 16 postings per step and add to packed per-reference
            // counters, four (or two) references per LDS word: in ascending order the 16 lanes of a step meet four by four in one word
            // (the genomes of one family have consecutive ids) and the LDS serves them one after the other.  Ordered by
            // (ref mod 4, ref) a step's postings fall into 16 different words instead.
            std::stable_sort(grp.begin(), grp.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return (a.first & 3u) < (b.first & 3u); });
            for (auto& g : grp) { post.push_back(g.first); post.push_back(g.second); }
        }
        uint32_t b = index_bucket(pairs[i].h, bmask);
        const uint32_t home = b;
        for (uint32_t chain = 1;; ++chain) {
            uint32_t q = 0;
            while (q < (uint32_t)IDX_SLOTS && fpb[(size_t)IDX_SLOTS * b + q] != 0) ++q;
            if (q < (uint32_t)IDX_SLOTS) {
                const size_t sl = (size_t)IDX_SLOTS * b + q;
                fpb[sl] |= (uint16_t)index_fp(pairs[i].h);
                kv[4 * sl] = (uint32_t)pairs[i].h; kv[4 * sl + 1] = (uint32_t)(pairs[i].h >> 32); kv[4 * sl + 2] = v;
                st.longest_chain = std::max(st.longest_chain, chain);
                if (b < home) st.chain_wrapped = 1;
                break;
            }
            if (!(fpb[(size_t)IDX_SLOTS * b] & IDX_OVF)) ++st.buckets_overflowed;
            fpb[(size_t)IDX_SLOTS * b] |= (uint16_t)IDX_OVF; // the key goes further down the chain: lookups must follow
            b = (b + 1) & bmask;
        }
        i = j;
    }
    t.nb = nb; t.lg = lg; t.distinct = distinct;
    t.fpb = std::move(fpb); t.kv = std::move(kv); t.post = std::move(post);
    stats = st;
    return PlanError{};
}
// compact the key/value entries: key id = (keys stored in earlier buckets) + position in the bucket
// (t.kv stays until the table goes: releasing its megabytes is no part of a build's timed steps)
inline void compact_hash_table(HashTable& t, rk_index_stats_t& st) {
    const uint32_t nb = t.nb;
    const std::vector<uint16_t>& fpb = t.fpb;
    const std::vector<uint32_t>& kv = t.kv;
    std::vector<uint32_t> base((size_t)nb + 1, 0);
    for (uint32_t b = 0; b < nb; ++b) {
        uint32_t q = 0;
        while (q < (uint32_t)IDX_SLOTS && fpb[(size_t)IDX_SLOTS * b + q] != 0) ++q;
        base[(size_t)b + 1] = base[b] + q;
    }
    const size_t nkeys = base[nb];
    st.keys = (uint32_t)nkeys; st.buckets = nb; st.post_words = (uint32_t)t.post.size();
    std::vector<uint32_t> dense((nkeys + 1) * 4, 0); // (one entry past the last key)
    for (uint32_t b = 0; b < nb; ++b)
        for (uint32_t q = 0; q < base[(size_t)b + 1] - base[b]; ++q)
            memcpy(&dense[((size_t)base[b] + q) * 4], &kv[((size_t)IDX_SLOTS * b + q) * 4], 16);
    t.keyhash.resize(nkeys);
    for (size_t q = 0; q < nkeys; ++q) t.keyhash[q] = ((uint64_t)dense[q * 4 + 1] << 32) | dense[q * 4];
    t.nkeys = nkeys; t.base = std::move(base); t.dense = std::move(dense);
}

// ---- first-level filter --------------------------------------------------------------------------------------------------------
// First-level filter in front of the bucket table (RKMH_PREFILTER=0 turns it off for A/B runs): two bits set per key,
// 32 bits per key where that fits in 1 MB -- measured at C2 (163 k keys): 256 KB 0.976 ms, 512 KB 0.959, 1 MB 0.953,
// 2 MB 0.997 (the filter then crowds the reads and the table out of the 4 MB L2); at 10^6 keys 1 MB beats 2 MB (1.07 vs
// 1.12 ms) although one window in twenty then passes by chance; only beyond 2 * 10^6 keys does 2 MB win (4 * 10^6
// keys: 1 MB 2.28 ms, 2 MB 1.77, 4 MB 1.99).  (RKMH_PRE_MAXKB overrides the cap: tests.)
inline size_t prefilter_cap_words(size_t distinct) { return (size_t)(distinct > 2000000 ? 2048 : 1024) * 256; }
inline uint32_t prefilter_words(size_t distinct, size_t max_words) {
    const size_t bits_per_key = 32;
    uint32_t pwords = 1u << 12;
    while ((size_t)pwords * 32 < distinct * bits_per_key && (size_t)pwords * 2 <= max_words) pwords <<= 1;
    return pwords;
}
inline std::vector<uint32_t> plan_prefilter(const std::vector<HashPair>& pairs, uint32_t pwords) {
    std::vector<uint32_t> pre(pwords, 0);
    for (const HashPair& p : pairs) pre[index_pre_word(p.h, pwords - 1)] |= index_pre_bits(p.h);
    return pre;
}

// ---- posting lists of the k-mer-space kernel -----------------------------------------------------------------------------------
// The posting lists of the k-mer-space kernel (RefIndex::kpost).  `post` holds one list per key; the genomes of one family share
// most of their sketch hashes, so many keys carry the same list and most of the others carry a list that differs from it in a
// few places (BASELINE config 3's panel: 61 near-identical Zika genomes, 21 HPV16 variants -- a read of theirs walked ~640
// postings).  Identical lists are stored once, and up to KBASE_MAX frequent long lists become BASES: a list close to a base is
// stored as (base, exceptions) -- the kernel adds one to the read's counter of that base, applies the few exceptions (+1 for a
// reference the base lacks, -1 for one it has in excess) and expands each touched base once per read before the arg-max
// (k_classify_kmer, phase 2).  Every such list is ALSO kept in plain form (the sparse-counter kernels cannot subtract).
// remap[offset in post] = (offset of the form the dense-counter kernels walk, offset of the plain form), both into kpost.
// kpost list = header (entries | (base + 1) << 24; base field 0: plain) then entries x (reference, multiplicity; bit 31: -1).
// A list within eight exceptions of its base (most of them) needs no list at all: base and exceptions go INTO the compound value
// (ix, iy, iw: tag 111, base, count, eight 10-bit fields of reference and sign) and the lane that finds the hit applies them.
// nbase_env: RKMH_KBASES (KBASE_MAX when unset).
constexpr int KBASE_MAX = 8;
struct KList { uint32_t enc = 0, plain = 0, ix = 0, iy = 0, iw = 0; };
inline void build_kpost(const std::vector<uint32_t>& post, int R, int nbase_env, std::vector<uint32_t>& kpost, std::vector<uint32_t>& kbase,
                        std::unordered_map<uint32_t, KList>& remap, rk_index_stats_t& st) {
    struct Dist { std::vector<std::pair<uint32_t, uint32_t>> e; uint32_t weight = 0, plain = 0, enc = 0, ix = 0, iy = 0, iw = 0; bool simple = true; };
    std::map<std::vector<std::pair<uint32_t, uint32_t>>, uint32_t> ids; // list content (sorted by reference) -> distinct id
    std::vector<Dist> dl;
    std::vector<std::pair<uint32_t, uint32_t>> owner; // (offset in post, distinct id)
    for (size_t off = 1; off < post.size();) {
        const uint32_t n = post[off];
        std::vector<std::pair<uint32_t, uint32_t>> e(n);
        for (uint32_t q = 0; q < n; ++q) e[q] = {post[off + 1 + 2 * q], post[off + 2 + 2 * q]};
        std::sort(e.begin(), e.end());
        auto it = ids.find(e);
        if (it == ids.end()) {
            it = ids.emplace(e, (uint32_t)dl.size()).first;
            Dist d; d.e = e;
            for (auto& x : e) d.simple = d.simple && x.second == 1u;
            dl.push_back(std::move(d));
        }
        dl[it->second].weight += 1;
        owner.emplace_back((uint32_t)off, it->second);
        off += 1 + 2 * (size_t)n;
    }
    const int nbase_max = R <= 0xFFFF ? std::min(std::max(nbase_env, 0), KBASE_MAX) : 0;
    // bases: the heaviest long lists (keys x references) that are not close to a base already chosen
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < dl.size(); ++i) if (dl[i].simple && dl[i].e.size() >= 8) order.push_back(i);
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint64_t wa = (uint64_t)dl[a].weight * dl[a].e.size(), wb = (uint64_t)dl[b].weight * dl[b].e.size();
        return wa != wb ? wa > wb : a < b;
    });
    auto sym_diff = [](const std::vector<std::pair<uint32_t, uint32_t>>& a, const std::vector<uint32_t>& b) {
        size_t i = 0, j = 0, d = 0;
        while (i < a.size() && j < b.size()) { if (a[i].first == b[j]) { ++i; ++j; } else if (a[i].first < b[j]) { ++i; ++d; } else { ++j; ++d; } }
        return d + (a.size() - i) + (b.size() - j);
    };
    std::vector<std::vector<uint32_t>> bases;
    for (uint32_t i : order) {
        if ((int)bases.size() >= nbase_max) break;
        bool far = true;
        for (auto& b : bases) far = far && sym_diff(dl[i].e, b) > std::max<size_t>(4, dl[i].e.size() / 4);
        if (!far) continue;
        std::vector<uint32_t> b;
        for (auto& x : dl[i].e) b.push_back(x.first);
        bases.push_back(std::move(b));
    }
    // Are the bases worth their price?  The kernel that knows (base, exceptions) lists carries per-read base counters, a test of every
    // compound value and an expansion step for EVERY read of every batch (k_classify_kmer<..., FAM>: 313.7 against 304.1 us per 1 M
    // reads on BASELINE config 2's panel, whose 182 HPV types share a handful of conserved k-mers and nothing else).  They stay only
    // where they take a real share of the posting walks away: at least 5 % of all postings of the index (config 3's panel: 70 %).
    if (!bases.empty()) {
        uint64_t total = 0, saved = 0;
        for (auto& d : dl) {
            total += (uint64_t)d.weight * d.e.size();
            if (!d.simple || d.e.size() < 8) continue;
            size_t bd = ~(size_t)0;
            for (auto& b : bases) bd = std::min(bd, sym_diff(d.e, b));
            if (2 * (1 + bd) <= d.e.size()) saved += (uint64_t)d.weight * (d.e.size() - bd - 1);
        }
        if (saved * 20 < total) { bases.clear(); st.bases_dropped_by_share_rule = 1; }
    }
    st.bases_kept = (uint32_t)bases.size();
    kbase.assign(2 * KBASE_MAX, 0u);
    for (size_t b = 0; b < bases.size(); ++b) {
        kbase[2 * b] = (uint32_t)kbase.size(); kbase[2 * b + 1] = (uint32_t)bases[b].size();
        kbase.insert(kbase.end(), bases[b].begin(), bases[b].end());
    }
    kbase.resize(kbase.size() + 64, 0u); // (the expansion reads 16 members at a time)
    kpost.assign(1, 0u);
    for (auto& d : dl) {
        d.plain = (uint32_t)kpost.size();
        kpost.push_back((uint32_t)d.e.size());
        for (auto& x : d.e) { kpost.push_back(x.first); kpost.push_back(x.second); }
        d.enc = d.plain;
        if (!d.simple || d.e.size() < 8 || bases.empty()) continue;
        size_t best = 0, bd = ~(size_t)0;
        for (size_t b = 0; b < bases.size(); ++b) { const size_t dd = sym_diff(d.e, bases[b]); if (dd < bd) { bd = dd; best = b; } }
        if (2 * (1 + bd) > d.e.size()) continue; // not worth it: at least half of the walk must go
        d.enc = (uint32_t)kpost.size();
        kpost.push_back((uint32_t)bd | ((uint32_t)(best + 1) << 24));
        const std::vector<uint32_t>& B = bases[best];
        size_t i = 0, j = 0;
        uint32_t ex[8] = {0, 0, 0, 0, 0, 0, 0, 0}, nex = 0;
        bool small_refs = true;
        auto exception = [&](uint32_t ref, bool neg) {
            kpost.push_back(ref); kpost.push_back(neg ? 0x80000001u : 1u);
            small_refs = small_refs && ref < 512u;
            if (nex < 8) ex[nex] = ref | (neg ? 512u : 0u);
            ++nex;
        };
        while (i < d.e.size() || j < B.size()) {
            if (j == B.size() || (i < d.e.size() && d.e[i].first < B[j])) { exception(d.e[i].first, false); ++i; }
            else if (i == d.e.size() || B[j] < d.e[i].first) { exception(B[j], true); ++j; }
            else { ++i; ++j; }
        }
        if (nex <= 8 && small_refs) {
            d.ix = 0xE0000000u | ((uint32_t)best << 26) | (nex << 22) | ex[0] | (ex[1] << 10);
            d.iy = ex[2] | (ex[3] << 10) | (ex[4] << 20);
            d.iw = ex[5] | (ex[6] << 10) | (ex[7] << 20);
        }
    }
    kpost.resize(kpost.size() + 64, 0u); // a hit's first sixteen postings are requested with the header
    for (auto& o : owner) { KList kl; kl.enc = dl[o.second].enc; kl.plain = dl[o.second].plain; kl.ix = dl[o.second].ix; kl.iy = dl[o.second].iy; kl.iw = dl[o.second].iw; remap[o.first] = kl; }
}

// ---- the enumeration list ------------------------------------------------------------------------------------------------------
// The k-mers of one size whose canonical hash is a key (or 0), one per strand pair, as the enumeration cache keeps them: per item
// (k-mer, key id) -- a wide k-mer (k > 16) takes two words.  Key id IDX_NOT_FOUND: the k-mer hashes to 0.
struct KmerList {
    int k = 0;
    std::vector<uint32_t> w;
    size_t lw() const { return k > 16 ? 3 : 2; }
    uint32_t found() const { return (uint32_t)(w.size() / lw()); }
    uint64_t kmer(size_t i) const { return k > 16 ? ((uint64_t)w[3 * i + 1] << 32) | w[3 * i] : (uint64_t)w[2 * i]; }
    uint32_t slot(size_t i) const { return w[lw() * i + lw() - 1]; }
};
// raw: what the device appended, 2 words per item (k-mer, key id) or, wide, 4 (k-mer low, high, key id, unused)
// (the device appends in a racy order: sorted by k-mer, the list -- and the cache file -- is reproducible)
inline KmerList sort_kmer_list(const std::vector<uint32_t>& raw, size_t got, int k) {
    std::vector<std::pair<uint64_t, uint32_t>> items(got);
    for (size_t i = 0; i < got; ++i)
        items[i] = k > 16 ? std::make_pair(((uint64_t)raw[4 * i + 1] << 32) | raw[4 * i], raw[4 * i + 2]) : std::make_pair((uint64_t)raw[2 * i], raw[2 * i + 1]);
    std::sort(items.begin(), items.end());
    KmerList l; l.k = k;
    const size_t lw = l.lw();
    l.w.resize(got * lw);
    for (size_t i = 0; i < got; ++i) {
        l.w[lw * i] = (uint32_t)items[i].first;
        if (k > 16) l.w[lw * i + 1] = (uint32_t)(items[i].first >> 32);
        l.w[lw * i + lw - 1] = items[i].second;
    }
    return l;
}
// Built only when every key has exactly one preimage (found == keys + zero-hash k-mers with no two entries sharing a key id):
// the k-mer then identifies the key in the per-read hit multiset.  Anything else leaves the hash-space kernels in charge.
// seen: [nkeys + 1], shared by the sizes of a run -- a key found by two k-mers of ANY sizes disables the form
inline bool one_preimage(const KmerList& l, size_t nkeys, std::vector<uint8_t>& seen) {
    for (uint32_t i = 0; i < l.found(); ++i) {
        const uint32_t slot = l.slot(i);
        if (slot == IDX_NOT_FOUND) continue;
        if (slot >= nkeys || seen[slot]) return false; // two different k-mers with the same 64-bit canonical hash
        seen[slot] = 1;
    }
    return true;
}

// ---- compound values -----------------------------------------------------------------------------------------------------------
// value id of an index key for the k-mer-space kernels: the reference itself (one posting, once) or nref + the number of a
// compound value of four dwords in `vals` (km1_vals) -- shared by the narrow and the wide form.  One table per k-mer size.
struct ValueTable {
    int R;
    const HashTable& t;
    const std::unordered_map<uint32_t, KList>& kremap;
    rk_index_stats_t& st;
    std::vector<uint32_t> vals;
    std::unordered_map<uint32_t, uint32_t> val_id;
    uint32_t value_id_of(uint32_t slot) {
        const uint32_t val = t.dense[(size_t)slot * 4 + 2];
        if (!(val >> 31) && ((val >> 29) & 3u) == 0u && ((val >> 20) & 0x1FFu) == 1u) { ++st.kv_reference; return val & 0xFFFFFu; } // one posting, once: the reference
        // lists: identical ones share one compound value (and one copy in kpost, see build_kpost)
        uint32_t vkey = val;
        KList kl;
        if (val >> 31) { kl = kremap.at(val & 0x7fffffffu); vkey = 0x80000000u | kl.plain; }
        auto it = val_id.find(vkey);
        if (it == val_id.end()) {
            it = val_id.emplace(vkey, (uint32_t)(R + vals.size() / 4)).first;
            // four dwords per entry: the index value and, for a list of three to six references that each hold the hash
            // once (what related types of one panel share), the list itself, nine bits per reference -- the kernel then
            // counts it in the lane that found the hit instead of fetching the posting list from global memory (KM1V_INLINE)
            uint32_t x = val, y = 0;
            if (RK_KMER_INLINE_N && (val >> 31)) {
                const uint32_t off = val & 0x7fffffffu, n = t.post[off];
                bool ok3 = n >= 3 && n <= 6;
                for (uint32_t q = 0; ok3 && q < n; ++q) ok3 = t.post[off + 1 + 2 * q] < 512u && t.post[off + 2 + 2 * q] == 1u;
                if (ok3) {
                    uint32_t r[6] = {0, 0, 0, 0, 0, 0};
                    for (uint32_t q = 0; q < n; ++q) r[q] = t.post[off + 1 + 2 * q];
                    x = 0xC0000000u | ((n - 3u) << 27) | r[0] | (r[1] << 9) | (r[2] << 18);
                    y = r[3] | (r[4] << 9) | (r[5] << 18);
                }
            }
            // a list that stays a list: x = the form the dense-counter kernels walk (plain, or base + exceptions) -- or, within eight
            // exceptions of its base, x, y and w hold base and exceptions themselves -- and z = the plain form (sparse counters)
            uint32_t z = 0, w = 0;
            if ((x >> 30) == 2u) {
                z = kl.plain;
                if (kl.ix) { x = kl.ix; y = kl.iy; w = kl.iw; } else x = 0x80000000u | kl.enc;
            }
            vals.push_back(x); vals.push_back(y); vals.push_back(z); vals.push_back(w);
        }
        // (rk_index_stats: the form this key's compound value took, read off the value the kernels will decode)
        const uint32_t* cv = &vals[4 * (size_t)(it->second - (uint32_t)R)];
        if (!(cv[0] >> 31)) ++(((cv[0] >> 29) & 3u) == 1u ? st.kv_pair : st.kv_single_multi);
        else if ((cv[0] >> 29) == 7u) ++st.kv_base_inline;
        else if ((cv[0] >> 30) == 3u) ++st.kv_inline_list;
        else ++((cv[0] & 0x3fffffffu) != cv[2] ? st.kv_base_list : st.kv_plain_list);
        return it->second;
    }
};

// ---- group filter and exact map of one k-mer size --------------------------------------------------------------------------------
struct KmerMaps {
    uint32_t nsect = 0, b = 0, longest_hop = 0, vmask = 0;
    std::vector<uint32_t> f4;       // [4 * nsect] the group filter
    std::vector<uint32_t> cells;    // [4 << b] the exact map
    std::vector<uint32_t> km1cells; // narrow: (cell, key id) per found k-mer (rk_set_depth_filter masks cells by key)
    std::vector<uint32_t> kkeys, kslots; // wide: parallel to the list, see KW_C in rk_device.hpp
};
// sectors of the filter for `found` k-mers at e entries per sector
inline uint32_t kf4_sector_count(uint32_t found, double e) {
    const double want = (double)found * 8.0 / e;
    return want < 256.0 ? 256u : (want > 16777216.0 ? 16777216u : ((uint32_t)want + 7u) & ~7u);
}
inline uint32_t kf4_sectors_wide(uint32_t found) { return kf4_sector_count(found, found > 300000u ? 18.0 : 13.0); }
// start size of a map of four-cell buckets at a load of 0.65
inline uint32_t map_start_bits(uint32_t found, uint32_t b, uint32_t bmax) {
    const double load = 0.65;
    while (b < bmax && (double)found > load * 4.0 * (double)((size_t)1 << b)) ++b;
    return b;
}
// group filter of k_classify_kmer (kf4_sector in rk_device.hpp): every found k-mer in both orientations under its four
// alignments, RK_KF4_NBITS (three) bits each in dword j of the 16-byte sector its alignment-j core selects (at 14 entries per
// sector about 9 of a dword's 32 bits are set: one window in ~45 of those that hit nothing passes by chance)
// Size (any sector count, kf4_sector scales the hashed core): a sparser filter sends fewer windows to the exact map, a
// smaller one leaves more of an XCD's 4 MB of L2 to the map and the streaming bases -- and the second matters more until
// the panel is far beyond any cache.  Measured optimum, entries per sector (tools/kf4_density.sh, 1 M reads; ms at the
// optimum / at the 5-10 a power-of-two size would give): 161 k keys (C2, 1 MB map) 12-13.5 (0.321 / 0.335); 239 k keys
// (266 references, C3; 2 MB map) 12.5-16 (0.343 / 0.425); 270 k 14 (0.353 / 0.433); 360 k (4 MB map) 20 (0.397 / 0.584);
// 540 k 20-24 (0.592 / 0.655); 900 k (8 MB map) 14 (0.747 / 0.787); 1.8 M <= 10 (0.894); 3.6 M <= 10 (0.947).
// kf4_entries: RKMH_KF4_ENTRIES, a forced density (A/B runs; 0: the rule)
inline uint32_t kf4_sectors_narrow(int k, uint32_t found, double kf4_entries) {
    const uint32_t kbits = 2u * (uint32_t)k;
    const uint32_t be = map_start_bits(found, kbits < 12u ? kbits : 12u, kbits < 28u ? kbits : 28u); // the map's size, as its builder will choose it
    const size_t map_bytes = (size_t)16 << be;
    // (k = 16 with s = 2000, 322 k keys: 20 entries 0.646, 13 entries 0.665; k = 12, whose 9-base cores crowd the sectors
    // unevenly: 6-8 entries 0.477, 10 entries 0.504, 13 entries 0.555; k = 13: 9-13 entries 0.40, 6 entries 0.435)
    // (all of the above with two bits per entry; with the three shipped -- kf4_bits -- the optima move little: C2 14 entries
    // 0.314, 12 0.317, 17 0.326; 266 references 13-14 0.332; s = 2000 16 0.626, 20 0.635; 400 references 20 0.407)
    // (k = 15 / 14 with three bits: 12.5 entries 0.348 / 0.366, 14 entries 0.360 / 0.369, 11 entries 0.353 / 0.375)
    double e = k <= 12 ? 7.0 : (k == 13 ? 10.0 : 13.0);
    if (found > 1500000u) e = 8.0;                                             // far beyond any cache: fewer false candidates win
    else if (found > 300000u && map_bytes <= ((size_t)4 << 20)) e = 18.0;      // map and filter fight for the L2: smallest useful filter
    if (kf4_entries > 0.0) e = kf4_entries;
    return kf4_sector_count(found, e);
}
// the fill, for 32-bit and 64-bit k-mers: a wide k-mer and its cores go through kw_fold, a narrow one as it is
inline std::vector<uint32_t> plan_kf4(const KmerList& l, uint32_t nsect) {
    const int k = l.k;
    const bool wide = k > 16;
    std::vector<uint32_t> f4((size_t)4 * nsect, 0u);
    const uint64_t cm = (1ull << (2 * (k - 3))) - 1ull; // (kf4_core_mask(k) for k <= 16)
    for (uint32_t i = 0; i < l.found(); ++i) {
        const uint64_t v = l.kmer(i), rv = wide ? packed_revcomp64(v, k) : (uint64_t)packed_revcomp((uint32_t)v, k);
        for (int o = 0; o < (rv == v ? 1 : 2); ++o) {
            const uint64_t X = o ? rv : v;
            const uint32_t bits = kf4_bits(wide ? kw_fold(X) : (uint32_t)X);
            for (uint32_t j = 0; j < 4; ++j) {
                const uint64_t core = (X >> (2 * (3 - j))) & cm;
                f4[(size_t)kf4_sector(wide ? kw_fold(core) : (uint32_t)core, nsect) * 4 + j] |= bits;
            }
        }
    }
    return f4;
}
// Map placement, for km1 and the wide map alike.  A bucket is four cells; a cell, from the top: hop, tag (tagbits), one flag bit (bit
// idbits: in a bucket's last cell, "a key that wanted this bucket, or passed through it, lies further on") and the id (idbits; all
// ones = empty).  A key whose bucket is full moves on by up to 2^KM1_HB - 1 buckets.  item(i, bucket, tag, id) names key i's
// home bucket, tag and id.  False: some key found no cell within its hops (the table must double).
struct MapShape { uint32_t b, idbits, tagbits, empty_cell; };
template <typename Item>
inline bool place_cells(const MapShape& s, uint32_t n, Item item, std::vector<uint32_t>& cells, uint32_t* cell_of, uint32_t& longest_hop) {
    const uint32_t nbk = 1u << s.b, idmask = (1u << s.idbits) - 1u, flag = 1u << s.idbits;
    cells.assign((size_t)nbk * 4, s.empty_cell);
    longest_hop = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t bk, tag, id;
        item(i, bk, tag, id);
        bool placed = false;
        for (uint32_t hop = 0; hop < (1u << KM1_HB) && !placed; ++hop) {
            uint32_t* e = &cells[(size_t)bk * 4];
            for (int q = 0; q < 4 && !placed; ++q)
                if ((e[q] & idmask) == idmask) { // empty (no key carries the all-ones id; the flag of a last cell stays)
                    e[q] = (e[q] & flag) | (((hop << s.tagbits) | tag) << (s.idbits + 1)) | id;
                    if (cell_of) cell_of[i] = bk * 4u + (uint32_t)q;
                    longest_hop = std::max(longest_hop, hop);
                    placed = true;
                }
            if (!placed) { e[3] |= flag; bk = (bk + 1) & (nbk - 1); } // full: later lookups that miss here try the next bucket
        }
        if (!placed) return false;
    }
    return true;
}
// narrow k-mers (k <= 16): filter, the exact map (KM1_C in rk_device.hpp) and the cells of each key.  If the hops are not enough, or
// the value ids do not fit the cell, the table doubles (shorter remainders leave more bits for the id).  False: no map -- a list
// that names a key id twice or beyond nkeys is the caller's to refuse (one_preimage).
inline bool plan_narrow_maps(const KmerList& l, ValueTable& vt, double kf4_entries, KmerMaps& m) {
    const int k = l.k;
    const uint32_t found = l.found(), kbits = 2u * (uint32_t)k;
    m.nsect = kf4_sectors_narrow(k, found, kf4_entries);
    m.f4 = plan_kf4(l, m.nsect);
    std::vector<uint32_t> vid(found), cell_of(found);
    const uint32_t VID_ZERO = 0xFFFFFFFEu; // placeholder, mapped to the layout's id below
    for (uint32_t i = 0; i < found; ++i) vid[i] = l.slot(i) == IDX_NOT_FOUND ? VID_ZERO : vt.value_id_of(l.slot(i));
    bool built = false;
    for (m.b = map_start_bits(found, kbits < 12u ? kbits : 12u, kbits < 28u ? kbits : 28u); m.b <= kbits && m.b <= 28 && !built; ++m.b) {
        const uint32_t r = kbits - m.b, vb = km1_vbits(k, m.b), vmask = (1u << vb) - 1u, rmask = r ? (1u << r) - 1u : 0u;
        if ((uint64_t)vt.R + vt.vals.size() / 4 + 2 > (uint64_t)vmask) continue; // ids need more bits: a longer bucket index frees them
        built = place_cells(MapShape{m.b, vb, r, ~(1u << vb)}, found, [&](uint32_t i, uint32_t& bk, uint32_t& tag, uint32_t& id) { // empty: tag and id all ones, flag clear
            const uint32_t y = km1_y((uint32_t)l.kmer(i), k);
            bk = r ? y >> r : y; tag = y & rmask; id = vid[i] == VID_ZERO ? vmask - 1u : vid[i];
        }, m.cells, cell_of.data(), m.longest_hop);
        if (built) { m.vmask = vmask; break; }
    }
    if (!built) return false; // the hash-space kernels serve the panel
    m.km1cells.resize(2 * (size_t)found);
    for (uint32_t i = 0; i < found; ++i) { m.km1cells[2 * (size_t)i] = cell_of[i]; m.km1cells[2 * (size_t)i + 1] = l.slot(i); }
    return true;
}
// wide k-mers (k = 17 .. KW_MAX_K): the same group filter (sector and bits from kw_fold of core and k-mer), the km2 map and kkeys.
// False: a value id beyond the 24 bits kkeys has for it, or no map of up to 2^26 buckets takes the keys.
inline bool plan_wide_maps(const KmerList& l, ValueTable& vt, KmerMaps& m) {
    const int k = l.k;
    const uint32_t found = l.found(), kbits = 2u * (uint32_t)k;
    m.nsect = kf4_sectors_wide(found);
    m.f4 = plan_kf4(l, m.nsect);
    m.kkeys.assign((size_t)found * 2 + 4, 0u); m.kslots.assign((size_t)found + 4, 0u);
    for (uint32_t i = 0; i < found; ++i) {
        const uint32_t slot = l.slot(i);
        const uint32_t vid = slot == IDX_NOT_FOUND ? KW_VID_ZERO : vt.value_id_of(slot);
        if (vid >= KW_VID_ZERO && slot != IDX_NOT_FOUND) return false; // (value ids are 24 bits here)
        m.kkeys[2 * (size_t)i] = (uint32_t)l.kmer(i); m.kkeys[2 * (size_t)i + 1] = (uint32_t)(l.kmer(i) >> 32) | (vid << 8);
        m.kslots[i] = slot == IDX_NOT_FOUND ? 0u : slot;
    }
    for (m.b = map_start_bits(found, 12, 26); m.b <= 26; ++m.b) {
        const uint32_t b = m.b;
        const bool placed = place_cells(MapShape{b, KW_IDBITS, KW_TAG, KW_EMPTY}, found, [&](uint32_t i, uint32_t& bk, uint32_t& tag, uint32_t& id) { // empty: key number all ones, hop / tag / flag clear
            const uint64_t y = kw_y(l.kmer(i), k);
            bk = (uint32_t)(y >> (kbits - b)); tag = (uint32_t)(y >> (kbits - b - KW_TAG)) & ((1u << KW_TAG) - 1u); id = i;
        }, m.cells, nullptr, m.longest_hop);
        if (placed) return true;
    }
    return false;
}
