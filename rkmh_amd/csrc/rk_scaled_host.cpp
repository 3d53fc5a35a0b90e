// rk_scaled_host.cpp -- the host half of scaled (FracMinHash) sketches (include/rkmh_amd.h, "SCALED SKETCHES"): the threshold of a
// `scaled` value, the union of sketches (what `-g` reduces the records of a file with, and what cuts a sketch down to a larger
// `scaled`), the host forms of gather, of search and of the weighted comparison, and the places where counts become floating point.  Host code
// only, usable without a GPU; the kernels are rk_scaled.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rkmh_amd.h"

extern "C" void rk__set_error(const char* msg);

namespace {
int bad(const std::string& msg) { rk__set_error(msg.c_str()); return RK_ERR_ARG; }
} // namespace

// max_hash(scaled) = floor((2^64 - 1) / scaled): a hash h is kept when 0 < h <= max_hash.  scaled = 1 keeps everything.
extern "C" int rk_scaled_max_hash(uint64_t scaled, uint64_t* max_hash) {
    if (!max_hash) return bad("rk_scaled_max_hash: max_hash is NULL");
    if (scaled == 0) return bad("rk_scaled_max_hash: scaled must be at least 1");
    *max_hash = ~0ull / scaled;
    return RK_OK;
}

// *out (malloc'd, rk_free), *out_len: the ascending distinct values v of n sketches (CSR: sketch i is values[offsets[i], offsets[i+1]))
// with 0 < v <= max_hash.  n = 1 cuts one sketch down to a larger `scaled`: exact, because max_hash is monotone in scaled.
extern "C" int rk_merge_scaled(const uint64_t* values, const uint64_t* offsets, int n, uint64_t max_hash, uint64_t** out, uint64_t* out_len) {
    if (!out || !out_len || n < 0 || (n > 0 && !offsets)) return bad("rk_merge_scaled: bad arguments");
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return bad("rk_merge_scaled: offsets decrease at sketch " + std::to_string(i));
    const uint64_t lo = n ? offsets[0] : 0, hi = n ? offsets[n] : 0;
    if (hi > lo && !values) return bad("rk_merge_scaled: values is NULL");
    std::vector<uint64_t> v;
    v.reserve((size_t)(hi - lo));
    for (uint64_t t = lo; t < hi; ++t)
        if (values[t] != 0 && values[t] <= max_hash) v.push_back(values[t]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    uint64_t* r = (uint64_t*)malloc(sizeof(uint64_t) * (v.empty() ? 1 : v.size()));
    if (!r) { rk__set_error("rk_merge_scaled: malloc"); return RK_ERR_NOMEM; }
    if (!v.empty()) memcpy(r, v.data(), v.size() * 8);
    *out = r;
    *out_len = (uint64_t)v.size();
    return RK_OK;
}

// rk_merge_scaled with abundances (include/rkmh_amd.h, "ABUNDANCE"): the values as rk_merge_scaled gives them, and per value the sum of
// its abundances over the parts, saturating at 2^32 - 1.  A cut to a smaller max_hash keeps the prefix of both arrays.
extern "C" int rk_merge_scaled_abund(const uint64_t* values, const uint32_t* abunds, const uint64_t* offsets, int n, uint64_t max_hash,
                                     uint64_t** out_values, uint32_t** out_abunds, uint64_t* out_len) {
    if (!out_values || !out_abunds || !out_len || n < 0 || (n > 0 && !offsets)) return bad("rk_merge_scaled_abund: bad arguments");
    for (int i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return bad("rk_merge_scaled_abund: offsets decrease at sketch " + std::to_string(i));
    const uint64_t lo = n ? offsets[0] : 0, hi = n ? offsets[n] : 0;
    if (hi > lo && (!values || !abunds)) return bad("rk_merge_scaled_abund: values or abunds is NULL");
    std::vector<std::pair<uint64_t, uint32_t>> v;
    v.reserve((size_t)(hi - lo));
    for (uint64_t t = lo; t < hi; ++t) {
        if (abunds[t] == 0) return bad("rk_merge_scaled_abund: abundance 0 at value " + std::to_string(t));
        if (values[t] != 0 && values[t] <= max_hash) v.emplace_back(values[t], abunds[t]);
    }
    std::sort(v.begin(), v.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
    size_t m = 0; // distinct values so far; sums saturate (an integer sum: the order of the parts cannot change it)
    for (size_t t = 0; t < v.size(); ++t) {
        if (m && v[m - 1].first == v[t].first) v[m - 1].second = (uint32_t)std::min<uint64_t>((uint64_t)v[m - 1].second + v[t].second, 0xffffffffull);
        else v[m++] = v[t];
    }
    uint64_t* rv = (uint64_t*)malloc(sizeof(uint64_t) * (m ? m : 1));
    uint32_t* ra = (uint32_t*)malloc(sizeof(uint32_t) * (m ? m : 1));
    if (!rv || !ra) { free(rv); free(ra); rk__set_error("rk_merge_scaled_abund: malloc"); return RK_ERR_NOMEM; }
    for (size_t t = 0; t < m; ++t) { rv[t] = v[t].first; ra[t] = v[t].second; }
    *out_values = rv;
    *out_abunds = ra;
    *out_len = (uint64_t)m;
    return RK_OK;
}

// ---- gather on the host (include/rkmh_amd.h, "GATHER"): the loop of rk_gather.hip on host threads -- each reference value looked up in
// Q once, the hits of every candidate kept as a list of query indices, then per round a recount of every list against one byte per
// query value, the pick, and the removal.
namespace {
// f(begin, end) over [0, n) in contiguous pieces on at most nt threads (the caller's thread takes the first piece)
template <typename F>
void on_threads(size_t n, int nt, size_t min_piece, F f) {
    const size_t pieces = std::max<size_t>(1, std::min<size_t>((size_t)std::max(nt, 1), n / std::max<size_t>(min_piece, 1)));
    if (pieces == 1) { f((size_t)0, n); return; }
    const size_t per = (n + pieces - 1) / pieces;
    std::vector<std::thread> th;
    for (size_t i = 1; i < pieces; ++i) {
        const size_t lo = per * i, hi = std::min(n, lo + per);
        if (lo >= hi) break;
        th.emplace_back([=] { f(lo, hi); });
    }
    f((size_t)0, std::min(n, per));
    for (auto& t : th) t.join();
}
} // namespace

// The loop of both host entries.  wunique != nullptr (rk_gather_scaled_abund_host): wunique[t] = the abundances of the query values
// that row t removes, summed; the rows themselves never depend on it.
static int gather_host(const std::string& who, const uint64_t* q, const uint32_t* q_abund, uint64_t nq, const uint64_t* rv, const uint64_t* roff, int nref,
                       int min_shared, int max_rounds, int threads, int32_t* out4, uint64_t* wunique, int* nrounds) {
    if (!roff || !out4 || !nrounds || (!q && nq)) return bad(who + ": bad arguments");
    if (nref < 1) return bad(who + ": need at least one reference sketch");
    if (min_shared < 1 || max_rounds < 1) return bad(who + ": min_shared and max_rounds must be at least 1");
    if (nq > 0x7fffffffull) { rk__set_error((who + ": a query of more than 2^31-1 values").c_str()); return RK_ERR_LIMIT; }
    for (uint64_t i = 0; i < nq; ++i)
        if (q[i] == 0 || (i && q[i] <= q[i - 1])) return bad(who + ": the query is not ascending, distinct and non-zero at value " + std::to_string(i));
    for (int i = 0; i < nref; ++i) {
        if (roff[i + 1] < roff[i]) return bad(who + ": offsets of the references decrease at sketch " + std::to_string(i));
        if (roff[i + 1] - roff[i] > 0x7fffffffull) { rk__set_error((who + ": a reference sketch of 2^31 values or more").c_str()); return RK_ERR_LIMIT; }
    }
    if (roff[nref] > roff[0] && !rv) return bad(who + ": r_values is NULL");
    *nrounds = 0;
    if (wunique) std::fill(wunique, wunique + std::min(max_rounds, nref), (uint64_t)0); // every row there can be
    // the hits of every reference: a row ascends, so each lookup starts where the one before it ended
    std::vector<std::vector<uint32_t>> hits((size_t)nref);
    on_threads((size_t)nref, threads, 1, [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r) {
            const uint64_t* at = q;
            for (uint64_t t = roff[r]; t < roff[r + 1] && at < q + nq; ++t) {
                at = std::lower_bound(at, q + nq, rv[t]);
                if (at < q + nq && *at == rv[t]) hits[r].push_back((uint32_t)(at - q));
            }
        }
    });
    std::vector<int> cand; // references with total >= min_shared, ascending: the others can never win
    for (int r = 0; r < nref; ++r)
        if (hits[(size_t)r].size() >= (size_t)min_shared) cand.push_back(r);
    std::vector<uint8_t> alive((size_t)nq, 1);
    std::vector<int32_t> count(cand.size());
    int64_t remaining = (int64_t)nq;
    const int rows = (int)std::min<size_t>((size_t)max_rounds, cand.size());
    for (int t = 0; t < rows; ++t) {
        on_threads(cand.size(), threads, 16, [&](size_t lo, size_t hi) {
            for (size_t c = lo; c < hi; ++c) {
                int32_t n = 0;
                for (uint32_t h : hits[(size_t)cand[c]]) n += alive[h];
                count[c] = n;
            }
        });
        size_t best = 0; // the largest count; among equals the first candidate = the lowest reference index
        for (size_t c = 1; c < cand.size(); ++c)
            if (count[c] > count[best]) best = c;
        if (count[best] < min_shared) break;
        const std::vector<uint32_t>& mine = hits[(size_t)cand[best]];
        if (wunique) {
            uint64_t w = 0; // at most 2^31 - 1 values of at most 2^32 - 1 each: below 2^63
            for (uint32_t h : mine) w += alive[h] ? (uint64_t)q_abund[h] : 0;
            wunique[t] = w;
        }
        for (uint32_t h : mine) alive[h] = 0;
        remaining -= count[best];
        int32_t* row = out4 + (size_t)t * 4;
        row[0] = cand[best]; row[1] = count[best]; row[2] = (int32_t)mine.size(); row[3] = (int32_t)remaining;
        *nrounds = t + 1;
    }
    return RK_OK;
}

extern "C" int rk_gather_scaled_host(const uint64_t* q, uint64_t nq, const uint64_t* rv, const uint64_t* roff, int nref, int min_shared,
                                     int max_rounds, int threads, int32_t* out4, int* nrounds) {
    return gather_host("rk_gather_scaled_host", q, nullptr, nq, rv, roff, nref, min_shared, max_rounds, threads, out4, nullptr, nrounds);
}

// q_abund and wunique are checked here; everything else as rk_gather_scaled_host checks it
extern "C" int rk_gather_scaled_abund_host(const uint64_t* q, const uint32_t* q_abund, uint64_t nq, const uint64_t* rv, const uint64_t* roff, int nref,
                                           int min_shared, int max_rounds, int threads, int32_t* out4, uint64_t* wunique, int* nrounds) {
    const std::string who = "rk_gather_scaled_abund_host";
    if (!wunique || (!q_abund && nq)) return bad(who + ": bad arguments");
    if (q && nq <= 0x7fffffffull)
        for (uint64_t i = 0; i < nq; ++i)
            if (q_abund[i] == 0) return bad(who + ": abundance 0 at query value " + std::to_string(i));
    return gather_host(who, q, q_abund, nq, rv, roff, nref, min_shared, max_rounds, threads, out4, wunique, nrounds);
}

// ---- multigather on the host (include/rkmh_amd.h, "MULTIGATHER"): gather_host query after query -- `threads` host threads share the
// queries, each runs the loop above on one thread -- and the rows of all queries laid end to end.
extern "C" int rk_multigather_scaled_host(const uint64_t* rv, const uint64_t* roff, int64_t nref, const uint64_t* qv, const uint32_t* q_abund,
                                          const uint64_t* qoff, int64_t nq, int min_shared, int max_rounds, int threads, int32_t** rows4,
                                          uint64_t** wunique, uint64_t* row_offsets, uint64_t* nrows) {
    const std::string who = "rk_multigather_scaled_host";
    if (!roff || !qoff || !rows4 || !row_offsets || !nrows || (q_abund && !wunique)) return bad(who + ": bad arguments");
    if (nref < 1 || nq < 1) return bad(who + ": need at least one sketch on each side");
    if (min_shared < 1 || max_rounds < 1) return bad(who + ": min_shared and max_rounds must be at least 1");
    if (nref > 0x7fffffffll || nq > 0x7fffffffll) { rk__set_error((who + ": more than 2^31-1 sketches on one side").c_str()); return RK_ERR_LIMIT; }
    for (int64_t i = 0; i < nq; ++i) {
        if (qoff[i + 1] < qoff[i]) return bad(who + ": offsets of the queries decrease at sketch " + std::to_string(i));
        if (qoff[i + 1] - qoff[i] > 0x7fffffffull) return bad(who + ": sketch " + std::to_string(i) + " of the queries holds 2^31 values or more");
    }
    if (qoff[nq] > qoff[0] && !qv) return bad(who + ": values are NULL");
    // every query is checked before any is gathered (the references: by the first gather_host below, before it computes anything)
    for (int64_t i = 0; i < nq; ++i)
        for (uint64_t t = qoff[i]; t < qoff[i + 1]; ++t) {
            if (qv[t] == 0 || (t > qoff[i] && qv[t] <= qv[t - 1]))
                return bad(who + ": query " + std::to_string(i) + " is not ascending, distinct and non-zero at value " + std::to_string(t - qoff[i]));
            if (q_abund && q_abund[t] == 0) return bad(who + ": abundance 0 at value " + std::to_string(t - qoff[i]) + " of query " + std::to_string(i));
        }
    for (int64_t i = 0; i < nref; ++i) {
        if (roff[i + 1] < roff[i]) return bad(who + ": offsets of the references decrease at sketch " + std::to_string(i));
        if (roff[i + 1] - roff[i] > 0x7fffffffull) { rk__set_error((who + ": a reference sketch of 2^31 values or more").c_str()); return RK_ERR_LIMIT; }
    }
    if (roff[nref] > roff[0] && !rv) return bad(who + ": r_values is NULL");
    const int cap = (int)std::min<int64_t>(max_rounds, nref); // rows of one query at most
    std::vector<std::vector<int32_t>> rows((size_t)nq);
    std::vector<std::vector<uint64_t>> wu((size_t)nq);
    std::vector<int> code((size_t)nq, RK_OK);
    on_threads((size_t)nq, threads, 1, [&](size_t lo, size_t hi) {
        std::vector<int32_t> out4((size_t)cap * 4);
        std::vector<uint64_t> w((size_t)cap);
        for (size_t i = lo; i < hi; ++i) {
            int n = 0;
            code[i] = gather_host(who, qv + qoff[i], q_abund ? q_abund + qoff[i] : nullptr, qoff[i + 1] - qoff[i], rv, roff, (int)nref, min_shared, max_rounds, 1,
                                  out4.data(), q_abund ? w.data() : nullptr, &n);
            if (code[i] != RK_OK) return;
            rows[i].assign(out4.begin(), out4.begin() + (size_t)n * 4);
            if (q_abund) wu[i].assign(w.begin(), w.begin() + n);
        }
    });
    for (int c : code)
        if (c != RK_OK) return c; // (the thread's message may be another thread's: the checks above leave nothing for gather_host to refuse)
    uint64_t total = 0;
    for (int64_t i = 0; i < nq; ++i) { row_offsets[i] = total; total += rows[(size_t)i].size() / 4; }
    row_offsets[nq] = total;
    int32_t* out = (int32_t*)malloc(16 * (size_t)(total ? total : 1));
    uint64_t* out_w = q_abund ? (uint64_t*)malloc(8 * (size_t)(total ? total : 1)) : nullptr;
    if (!out || (q_abund && !out_w)) { free(out); free(out_w); rk__set_error((who + ": malloc").c_str()); return RK_ERR_NOMEM; }
    for (int64_t i = 0; i < nq; ++i) {
        const std::vector<int32_t>& r = rows[(size_t)i];
        if (!r.empty()) memcpy(out + row_offsets[i] * 4, r.data(), r.size() * 4);
        if (q_abund && !wu[(size_t)i].empty()) memcpy(out_w + row_offsets[i], wu[(size_t)i].data(), wu[(size_t)i].size() * 8);
    }
    *rows4 = out;
    if (q_abund) *wunique = out_w;
    *nrows = total;
    return RK_OK;
}

// ---- search on the host (include/rkmh_amd.h, "SEARCH"): the inverted index of rk_search.hip from a stable sort of (value, reference)
// pairs, then per query one counter per reference, the touched ones read out in ascending order.  Host memory: the index, one counter
// array per thread and the hits -- never nq x nref.
extern "C" int rk_search_scaled_host(const uint64_t* rv, const uint64_t* roff, int64_t nref, const uint64_t* qv, const uint64_t* qoff, int64_t nq,
                                     int min_shared, const int32_t* q_min, int threads, rk_search_hit** hits, uint64_t* nhits) {
    const std::string who = "rk_search_scaled_host";
    if (!roff || !qoff || !hits || !nhits) return bad(who + ": bad arguments");
    if (nref < 1 || nq < 1) return bad(who + ": need at least one sketch on each side");
    if (min_shared < 1) return bad(who + ": min_shared must be at least 1");
    if (nref > 0x7fffffffll || nq > 0x7fffffffll) { rk__set_error((who + ": more than 2^31-1 sketches on one side").c_str()); return RK_ERR_LIMIT; }
    for (int side = 0; side < 2; ++side) {
        const uint64_t* off = side ? qoff : roff;
        const char* name = side ? "the queries" : "the references";
        for (int64_t i = 0; i < (side ? nq : nref); ++i) {
            if (off[i + 1] < off[i]) return bad(who + ": offsets of " + name + " decrease at sketch " + std::to_string(i));
            if (off[i + 1] - off[i] > 0x7fffffffull) return bad(who + ": sketch " + std::to_string(i) + " of " + name + " holds 2^31 values or more");
        }
    }
    if ((roff[nref] > roff[0] && !rv) || (qoff[nq] > qoff[0] && !qv)) return bad(who + ": values are NULL");
    if (q_min)
        for (int64_t i = 0; i < nq; ++i)
            if (q_min[i] < 1) return bad(who + ": q_min of query " + std::to_string(i) + " is below 1");
    // the index: pairs ordered by value, the references of one value ascending (they are pushed in reference order; the sort is stable)
    std::vector<std::pair<uint64_t, uint32_t>> pairs;
    pairs.reserve((size_t)(roff[nref] - roff[0]));
    for (int64_t r = 0; r < nref; ++r)
        for (uint64_t t = roff[r]; t < roff[r + 1]; ++t) pairs.emplace_back(rv[t], (uint32_t)r);
    std::stable_sort(pairs.begin(), pairs.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
    std::vector<uint64_t> keys, post_off;
    for (size_t t = 0; t < pairs.size(); ++t)
        if (t == 0 || pairs[t - 1].first != pairs[t].first) { keys.push_back(pairs[t].first); post_off.push_back(t); }
    post_off.push_back(pairs.size());
    std::vector<std::vector<rk_search_hit>> per_query((size_t)nq);
    on_threads((size_t)nq, threads, 1, [&](size_t lo, size_t hi) {
        std::vector<int32_t> count((size_t)nref, 0);
        std::vector<uint32_t> touched;
        for (size_t q = lo; q < hi; ++q) {
            const int32_t thr = q_min ? std::max(min_shared, q_min[q]) : min_shared;
            touched.clear();
            for (uint64_t t = qoff[q]; t < qoff[q + 1]; ++t) {
                const size_t j = (size_t)(std::lower_bound(keys.begin(), keys.end(), qv[t]) - keys.begin());
                if (j == keys.size() || keys[j] != qv[t]) continue;
                for (uint64_t p = post_off[j]; p < post_off[j + 1]; ++p) {
                    const uint32_t r = pairs[(size_t)p].second;
                    if (count[r]++ == 0) touched.push_back(r);
                }
            }
            std::sort(touched.begin(), touched.end());
            for (uint32_t r : touched) {
                if (count[r] >= thr) per_query[q].push_back({(int32_t)q, (int32_t)r, count[r]});
                count[r] = 0;
            }
        }
    });
    size_t total = 0;
    for (const auto& h : per_query) total += h.size();
    rk_search_hit* out = (rk_search_hit*)malloc(sizeof(rk_search_hit) * (total ? total : 1));
    if (!out) { rk__set_error((who + ": malloc").c_str()); return RK_ERR_NOMEM; }
    size_t at = 0;
    for (const auto& h : per_query) {
        if (!h.empty()) memcpy(out + at, h.data(), h.size() * sizeof(rk_search_hit));
        at += h.size();
    }
    *hits = out;
    *nhits = (uint64_t)total;
    return RK_OK;
}

// *t = the smallest integer t with (double)t / (double)len >= x: what a containment of at least x asks a query of len values to share.
// 0 for x = 0 or an empty query; never above len.
extern "C" int rk_search_min_count(double x, uint64_t len, int32_t* t) {
    if (!t) return bad("rk_search_min_count: t is NULL");
    if (!(x >= 0.0 && x <= 1.0)) return bad("rk_search_min_count: the containment must lie in [0, 1]");
    if (len > 0x7fffffffull) { rk__set_error("rk_search_min_count: a query of more than 2^31-1 values"); return RK_ERR_LIMIT; }
    int64_t n = 0;
    if (len) {
        n = (int64_t)((double)len * x); // near the answer; the two loops settle it by the definition
        while (n > 0 && (double)(n - 1) / (double)len >= x) --n;
        while ((double)n / (double)len < x) ++n;
    }
    *t = (int32_t)n;
    return RK_OK;
}

// ---- weighted comparison on the host (include/rkmh_amd.h, "WEIGHTED COMPARISON"): the sums of k_scaled_pairs<L, PairsWeighted> and k_abund_row_sums
// from plain loops, and the one place where they become floating point.
namespace {
inline uint64_t sat_add(uint64_t a, uint64_t b) { const uint64_t s = a + b; return s < a ? ~0ull : s; }
// the checks of one side: offsets that ascend, rows below 2^31 values, arrays where there are values, no abundance of 0
int check_abund_side(const std::string& who, const char* side, const uint64_t* values, bool need_values, const uint32_t* abund, const uint64_t* off, int n) {
    for (int i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return bad(who + ": offsets of " + side + " decrease at sketch " + std::to_string(i));
        if (off[i + 1] - off[i] > 0x7fffffffull) return bad(who + ": sketch " + std::to_string(i) + " of " + side + " holds 2^31 values or more");
    }
    if (off[n] > 0 && ((need_values && !values) || !abund)) return bad(who + ": values or abundances of " + side + " are NULL");
    for (uint64_t t = off[0]; t < off[n]; ++t)
        if (abund[t] == 0) return bad(who + ": abundance 0 at value " + std::to_string(t) + " of " + side);
    return RK_OK;
}
} // namespace

extern "C" int rk_compare_scaled_abund_host(const uint64_t* av, const uint32_t* aw, const uint64_t* aoff, int na, const uint64_t* bv, const uint32_t* bw,
                                            const uint64_t* boff, int nb, int threads, uint64_t* out4) {
    const std::string who = "rk_compare_scaled_abund_host";
    if (!aoff || !boff || !out4) return bad(who + ": bad arguments");
    if (na < 1 || nb < 1) return bad(who + ": need at least one sketch on each side");
    if (int r = check_abund_side(who, "a", av, true, aw, aoff, na)) return r;
    if (int r = check_abund_side(who, "b", bv, true, bw, boff, nb)) return r;
    on_threads((size_t)na, threads, 1, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            for (size_t j = 0; j < (size_t)nb; ++j) {
                uint64_t ii = aoff[i], jj = boff[j], cnt = 0, dot = 0, wa = 0, wb = 0;
                const uint64_t ie = aoff[i + 1], je = boff[j + 1];
                while (ii < ie && jj < je) {
                    const uint64_t x = av[ii], y = bv[jj];
                    if (x == y) {
                        cnt += 1;
                        dot = sat_add(dot, (uint64_t)aw[ii] * (uint64_t)bw[jj]);
                        wa += aw[ii];
                        wb += bw[jj];
                    }
                    ii += x <= y;
                    jj += y <= x;
                }
                uint64_t* o = out4 + (i * (size_t)nb + j) * 4;
                o[0] = cnt; o[1] = dot; o[2] = wa; o[3] = wb;
            }
    });
    return RK_OK;
}

extern "C" int rk_abund_row_sums_host(const uint32_t* abund, const uint64_t* offsets, int n, uint64_t* out2) {
    const std::string who = "rk_abund_row_sums_host";
    if (!offsets || !out2) return bad(who + ": bad arguments");
    if (n < 1) return bad(who + ": need at least one sketch");
    if (int r = check_abund_side(who, "the sketches", nullptr, false, abund, offsets, n)) return r;
    for (int i = 0; i < n; ++i) {
        uint64_t sum = 0, sq = 0;
        for (uint64_t t = offsets[i]; t < offsets[i + 1]; ++t) {
            const uint64_t u = abund[t];
            sum += u;
            sq = sat_add(sq, u * u);
        }
        out2[(size_t)i * 2] = sum;
        out2[(size_t)i * 2 + 1] = sq;
    }
    return RK_OK;
}

// cosine = dot / sqrt(sumsq_a * sumsq_b), at most 1; angular = 1 - 2 acos(cosine) / pi.  The root is taken of the product: sqrt(fl(s) *
// fl(s)) is fl(s) exactly, so a sketch against itself gives 1 and 1.  Either sumsq 0: both 0.  A saturated input is the number it is.
extern "C" int rk_angular_similarity(uint64_t dot, uint64_t sumsq_a, uint64_t sumsq_b, double* cosine, double* angular) {
    if (dot > 0 && (sumsq_a == 0 || sumsq_b == 0)) return bad("rk_angular_similarity: a positive dot product needs both sums of squares positive");
    double c = 0.0, a = 0.0;
    if (sumsq_a != 0 && sumsq_b != 0) {
        c = (double)dot / std::sqrt((double)sumsq_a * (double)sumsq_b);
        if (c > 1.0) c = 1.0;
        a = 1.0 - 2.0 * std::acos(c) / 3.141592653589793;
    }
    if (cosine) *cosine = c;
    if (angular) *angular = a;
    return RK_OK;
}

// rk_mash_distance's formula and clamps on j = shared / (la + lb - shared): j = 0 and the distance 1 when the union is empty; the
// distance is 1 when shared = 0, else -ln(2j / (1 + j)) / k clamped to [0, 1] (never -0).  Either result pointer may be NULL.
extern "C" int rk_scaled_distance(int64_t shared, int64_t la, int64_t lb, int k, double* jaccard, double* distance) {
    if (shared < 0 || la < 0 || lb < 0 || shared > std::min(la, lb) || k < 1)
        return bad("rk_scaled_distance: need 0 <= shared <= min(la, lb) and k >= 1");
    const double uni = (double)la + (double)lb - (double)shared;
    const double j = uni > 0 ? (double)shared / uni : 0.0;
    double d = 1.0;
    if (shared > 0) {
        d = -std::log(2.0 * j / (1.0 + j)) / (double)k;
        if (!(d > 0.0)) d = 0.0;
        if (d > 1.0) d = 1.0;
    }
    if (jaccard) *jaccard = j;
    if (distance) *distance = d;
    return RK_OK;
}
