// rk_screen.hip -- screen (include/rkmh_amd.h, "SCREEN"): which reference sketches are contained in a read set.  The references' values
// are the keys of a resident inverted index (rk_search.hip's); k_screen_count hashes the windows of a resident batch as k_sample_keep
// does (rk_tile_walk.hpp) and, instead of keeping a hash, looks it up among the keys and adds 1 to the key's counter.  Memory is
// O(reference values): no pending array, no sort, no fold, no look at a cursor.  k_screen_rows and k_screen_owner turn the counters into
// (shared, median, owned shared, owned median) per reference.  The host-only form is rk_screen_rows_host (rk_screen_host.cpp);
// semantics, registers and measurements: DESIGN.md section 24.
#include "rk_sets.hpp"
#include "rk_tile_walk.hpp"

struct rk_screen {
    rk_ctx* ctx = nullptr; // compared and used while feeding; destroy does not follow it
    int device = 0;
    KsArr ks{};
    int kmax = 0;
    rk_scaled_index* ix = nullptr; // keys, post_off, post of the collapsed rows (owned)
    uint32_t nref = 0;
    uint64_t nkeys = 0, nvalues = 0; // distinct values of all rows; values of the collapsed rows
    uint64_t max_key = 0;
    uint32_t dir_shift = 0, ndir = 0; // bucket of h = h >> dir_shift, below ndir for every h <= max_key
    DevBuf dir;      // uint32[ndir + 1]: the keys of bucket b are keys[dir[b] .. dir[b + 1])
    DevBuf roff;     // uint64[nref + 1]: the collapsed rows
    DevBuf pos;      // uint32[nvalues]: where every value of a collapsed row stands in keys
    DevBuf counts;   // uint64[nkeys]
    DevBuf state;    // uint64[4] on the device: sequences fed, bases fed, windows counted
    DevBuf owner;    // uint32[nkeys]: the work array of a row call
    DevBuf w_out, w_bases, w_offs, w_vals, w_cnts;
    PinBuf h_state;
    uint64_t injected = 0; // the sum of what rk_screen_add_counts added
    std::mutex mu; // feeds and reads of one screen take turns
};

namespace {

constexpr int SC_WAVES = TW_T / 64;
constexpr uint32_t SC_NONE = 0xffffffffu;
constexpr uint64_t SC_SAT = 0xffffffffull;
constexpr uint64_t SC_PIECE_BASES = (uint64_t)64 << 20; // rk_screen_add_batch uploads pieces of about this many bases
constexpr int SC_DIR_MIN_BITS = 4, SC_DIR_MAX_BITS = 24;

// what the lookup needs, by value
struct ScreenKeys {
    const uint64_t* keys;
    const uint32_t* dir;
    uint64_t max_key;
    uint32_t nkeys, ndir, shift;
};

// where h stands in keys, SC_NONE when it is no key: one directory read (two neighbouring entries), then a search among the few keys
// of that bucket.  The bucket is checked against the directory size, the bucket's range and the position against nkeys.
__device__ __forceinline__ uint32_t key_position(const ScreenKeys& K, uint64_t h) {
    if (h == 0 || h > K.max_key) return SC_NONE;
    const uint64_t b = h >> K.shift;
    if (b >= (uint64_t)K.ndir) return SC_NONE;
    const uint32_t hi = min(K.dir[b + 1], K.nkeys);
    const uint32_t lo = min(K.dir[b], hi);
    const uint32_t p = first_not_below(K.keys, lo, hi, h);
    return p < hi && K.keys[p] == h ? p : SC_NONE;
}

// The windows of a resident batch (walk_tiles: k_sample_keep's walk), each looked up among the keys; a match adds 1 to counts[position]:
// one 64-bit atomicAdd on global memory, its result unused.  INTEGER ADDS COMMUTE (the precedent: k_mg_remove, k_cluster_hook), so the
// counts never depend on the order of arrival, on the grid or on how a batch is cut; a 64-bit counter cannot overflow (2^32 windows per
// batch at most), so there is no saturation here: the clamp to 2^32 - 1 happens where counts are read.  Lanes of a wave that hit the
// same key are NOT combined first: every lane issues its own atomic.  No staging array, no cursor.
// state[0] += n, state[1] += the bases (workgroup 0, when add_totals); state[2] += the matches, one atomic per wave that had any.
template <int KT>
__global__ __launch_bounds__(TW_T) void k_screen_count(const uint8_t* __restrict__ bases, const uint32_t* __restrict__ offs, uint32_t n, KsArr ks, int kmax,
                                                      DevPolicy pol, ScreenKeys K, unsigned long long* __restrict__ counts,
                                                      unsigned long long* __restrict__ state, int add_totals) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[stage_lds_dwords(HASH_TILE_MAXB)];
    __shared__ uint32_t bnd[TW_BND_DW];
    const uint32_t first = offs[0], end = offs[n];
    if (add_totals && blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&state[0], (unsigned long long)n);
        atomicAdd(&state[1], (unsigned long long)(end > first ? end - first : 0u));
    }
    if (end <= first) return;
    uint32_t mine = 0;
    walk_tiles<KT>(bases, offs, n, first, end, ks, kmax, pol, lds, bnd, [&](uint64_t h) {
        const uint32_t p = key_position(K, h);
        if (p < K.nkeys) {
            atomicAdd(&counts[p], 1ull);
            ++mine;
        }
    });
    for (int d = 32; d > 0; d >>= 1) mine += (uint32_t)__shfl_xor((int)mine, d, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&state[2], (unsigned long long)mine);
}

// rk_screen_add_counts: counts[position of v[t]] += c[t] for every v[t] that is a key
__global__ __launch_bounds__(TW_T) void k_screen_inject(const uint64_t* __restrict__ v, const uint32_t* __restrict__ c, uint64_t n, ScreenKeys K,
                                                       unsigned long long* __restrict__ counts) {
    for (uint64_t t = (uint64_t)blockIdx.x * TW_T + threadIdx.x; t < n; t += (uint64_t)gridDim.x * TW_T) {
        const uint32_t p = key_position(K, v[t]);
        if (p < K.nkeys) atomicAdd(&counts[p], (unsigned long long)c[t]);
    }
}

// is reference a (shared sa, length la) a better owner than b?  The larger shared / length, cross-multiplied in unsigned 64-bit (both
// factors below 2^31); among equal ratios the lower index.
__device__ __forceinline__ bool better_owner(uint32_t a, uint64_t sa, uint64_t la, uint32_t b, uint64_t sb, uint64_t lb) {
    if (b == SC_NONE) return a != SC_NONE;
    if (a == SC_NONE) return false;
    const uint64_t x = sa * lb, y = sb * la;
    return x > y || (x == y && a < b);
}

// owner[key] = the reference of the key's posting list with the largest shared / length (out4[r * 4] of a first run of k_screen_rows), or
// 2^32 - 1 when the key is not present.  One lane per key; lists of 64 entries or more are walked by the whole wave, one after the
// other (k_search_block's form).  Posting offsets are clamped to npost, every id is checked against nref.
__global__ __launch_bounds__(TW_T) void k_screen_owner(const unsigned long long* __restrict__ counts, uint32_t nkeys, const uint64_t* __restrict__ post_off,
                                                      const uint32_t* __restrict__ post, uint64_t npost, const uint64_t* __restrict__ roff, uint32_t nref,
                                                      const uint32_t* __restrict__ out4, uint32_t min_copies, uint32_t* __restrict__ owner) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nthreads = (uint64_t)gridDim.x * TW_T;
    for (uint64_t k0 = (uint64_t)blockIdx.x * TW_T + (threadIdx.x & ~63u); k0 < nkeys; k0 += nthreads) { // wave-uniform
        const uint64_t key = k0 + lane;
        uint64_t p0 = 0, p1 = 0;
        if (key < nkeys && min((uint64_t)counts[key], SC_SAT) >= (uint64_t)min_copies) {
            p0 = min(post_off[key], npost);
            p1 = max(min(post_off[key + 1], npost), p0);
        }
        uint32_t best = SC_NONE;
        uint64_t bs = 0, bl = 1;
        const bool wide = p1 - p0 >= 64;
        if (!wide)
            for (uint64_t i = p0; i < p1; ++i) {
                const uint32_t r = post[i];
                if (r >= nref) continue;
                const uint64_t s = out4[(uint64_t)r * 4], l = roff[r + 1] - roff[r];
                if (better_owner(r, s, l, best, bs, bl)) { best = r; bs = s; bl = l; }
            }
        uint64_t todo = __ballot(wide);
        while (todo) {
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t s0 = shfl_u64(p0, src), s1 = shfl_u64(p1, src);
            uint32_t wb = SC_NONE;
            uint64_t ws = 0, wl = 1;
            for (uint64_t i = s0 + lane; i < s1; i += 64) {
                const uint32_t r = post[i];
                if (r >= nref) continue;
                const uint64_t s = out4[(uint64_t)r * 4], l = roff[r + 1] - roff[r];
                if (better_owner(r, s, l, wb, ws, wl)) { wb = r; ws = s; wl = l; }
            }
            for (int d = 32; d > 0; d >>= 1) {
                const uint32_t ob = (uint32_t)__shfl_xor((int)wb, d, 64);
                const uint64_t os = shfl_xor_u64(ws, d), ol = shfl_xor_u64(wl, d);
                if (better_owner(ob, os, ol, wb, ws, wl)) { wb = ob; ws = os; wl = ol; }
            }
            if ((int)lane == src) best = wb;
        }
        if (key < nkeys) owner[key] = best;
    }
}

// One wave per reference, grid-stride.  Lanes stride pos[] of the collapsed row, load and clamp the count, test presence (OWNED: and
// owner == r).  shared comes from ballot popcounts; the lower median -- the element at index (shared - 1) / 2 of the qualifying counts in
// ascending order -- from bisection on the VALUE between the smallest and the largest qualifying count: at most 32 passes of "how many
// qualifying counts are <= mid", no sort, no LDS.  OWNED = false writes out4[r * 4 + 0 .. 1], OWNED = true out4[r * 4 + 2 .. 3].
// Row offsets are clamped to nvalues, every position is checked against nkeys.
template <bool OWNED>
__global__ __launch_bounds__(TW_T) void k_screen_rows(const uint64_t* __restrict__ roff, uint32_t nref, uint64_t nvalues, const uint32_t* __restrict__ pos,
                                                     const unsigned long long* __restrict__ counts, uint32_t nkeys, const uint32_t* __restrict__ owner,
                                                     uint32_t min_copies, uint32_t* __restrict__ out4) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t nwaves = (uint64_t)gridDim.x * SC_WAVES;
    for (uint64_t r = (uint64_t)blockIdx.x * SC_WAVES + (threadIdx.x >> 6); r < nref; r += nwaves) { // wave-uniform
        uint64_t r0, r1;
        clamped_row(roff, r, nvalues, r0, r1);
        // the qualifying count behind position t of the row, 0 when it does not qualify (a qualifying count is at least min_copies >= 1)
        auto qual = [&](uint64_t t) -> uint32_t {
            if (t >= r1) return 0u;
            const uint32_t p = pos[t];
            if (p >= nkeys) return 0u;
            if (OWNED && owner[p] != (uint32_t)r) return 0u;
            const uint32_t c = (uint32_t)min((uint64_t)counts[p], SC_SAT);
            return c >= min_copies ? c : 0u;
        };
        uint32_t shared = 0, lo = SC_NONE, hi = 0; // wave-uniform after the reduction
        for (uint64_t t0 = r0; t0 < r1; t0 += 64) {
            const uint32_t c = qual(t0 + lane);
            shared += (uint32_t)__popcll(__ballot(c != 0));
            if (c) { lo = min(lo, c); hi = max(hi, c); }
        }
        for (int d = 32; d > 0; d >>= 1) {
            lo = min(lo, (uint32_t)__shfl_xor((int)lo, d, 64));
            hi = max(hi, (uint32_t)__shfl_xor((int)hi, d, 64));
        }
        uint32_t median = 0;
        if (shared) {
            const uint32_t need = (shared - 1) / 2 + 1; // the median is the smallest x with `need` qualifying counts <= x
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                uint32_t below = 0;
                for (uint64_t t0 = r0; t0 < r1; t0 += 64) {
                    const uint32_t c = qual(t0 + lane);
                    below += (uint32_t)__popcll(__ballot(c != 0 && c <= mid));
                }
                if (below >= need) hi = mid; else lo = mid + 1;
            }
            median = lo;
        }
        if (lane == 0) {
            out4[r * 4 + (OWNED ? 2 : 0)] = shared;
            out4[r * 4 + (OWNED ? 3 : 1)] = median;
        }
    }
}

int check_screen(const rk_screen* s) {
    if (!s || !s->ctx) return fail(RK_ERR_ARG, "screen is NULL");
    return RK_OK;
}
ScreenKeys screen_keys(rk_screen* s) {
    return ScreenKeys{s->ix->keys.as<uint64_t>(), s->dir.as<uint32_t>(), s->max_key, (uint32_t)s->nkeys, s->ndir, s->dir_shift};
}

// one resident batch, asynchronous on st; the caller holds s->mu and has set the device.  bound_bases sizes the grid (0: not known; the
// kernel strides, so any grid is right)
int launch_count(rk_screen* s, const void* d_bases, const void* d_offs, uint32_t n, uint64_t bound_bases, hipStream_t st) {
    const uint64_t tiles = bound_bases ? (bound_bases + HASH_TILE_WIN - 1) / HASH_TILE_WIN : 4096;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(tiles, 1), 4096);
    unsigned long long* counts = s->counts.as<unsigned long long>();
    unsigned long long* state = s->state.as<unsigned long long>();
    const ScreenKeys K = screen_keys(s);
    bool k16 = false, other = false;
    for (int j = 0; j < s->ks.n; ++j) (s->ks.k[j] == 16 ? k16 : other) = true;
    if (k16)
        hipLaunchKernelGGL(k_screen_count<16>, dim3(grid), dim3(TW_T), 0, st, (const uint8_t*)d_bases, (const uint32_t*)d_offs, n, s->ks, s->kmax, s->ctx->pol, K,
                           counts, state, 1);
    if (other)
        hipLaunchKernelGGL(k_screen_count<0>, dim3(grid), dim3(TW_T), 0, st, (const uint8_t*)d_bases, (const uint32_t*)d_offs, n, s->ks, s->kmax, s->ctx->pol, K,
                           counts, state, k16 ? 0 : 1);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

// rows(plain) -> owner -> rows(owned) on st; the caller holds s->mu and has set the device
int launch_rows(rk_screen* s, uint32_t min_copies, uint32_t* d_out4, hipStream_t st) {
    const uint64_t* roff = s->roff.as<uint64_t>();
    const uint32_t* pos = s->pos.as<uint32_t>();
    const unsigned long long* counts = s->counts.as<unsigned long long>();
    uint32_t* owner = s->owner.as<uint32_t>();
    const uint32_t nkeys = (uint32_t)s->nkeys;
    const uint32_t rgrid = wave_grid(s->nref, SC_WAVES);
    hipLaunchKernelGGL(k_screen_rows<false>, dim3(rgrid), dim3(TW_T), 0, st, roff, s->nref, s->nvalues, pos, counts, nkeys, (const uint32_t*)owner, min_copies, d_out4);
    if (nkeys)
        hipLaunchKernelGGL(k_screen_owner, dim3(wave_grid((nkeys + 63) / 64, SC_WAVES)), dim3(TW_T), 0, st, counts, nkeys, s->ix->post_off.as<uint64_t>(),
                           s->ix->post.as<uint32_t>(), s->ix->npost, roff, s->nref, (const uint32_t*)d_out4, min_copies, owner);
    hipLaunchKernelGGL(k_screen_rows<true>, dim3(rgrid), dim3(TW_T), 0, st, roff, s->nref, s->nvalues, pos, counts, nkeys, (const uint32_t*)owner, min_copies, d_out4);
    HIPCHK(hipGetLastError());
    return RK_OK;
}

int check_min_copies(uint64_t m) {
    if (m < 1 || m > SC_SAT) return fail(RK_ERR_ARG, "screen: min_copies %llu outside [1,2^32-1]", (unsigned long long)m);
    return RK_OK;
}

} // namespace

namespace rk {
rk_ctx* screen_ctx(const rk_screen* s) { return s ? s->ctx : nullptr; }
int screen_feed_device(rk_screen* s, const void* d_bases, const void* d_offs_u32, int64_t nseq, uint64_t bound_bases, hipStream_t st) {
    RKCHK(check_screen(s));
    if (nseq < 0 || (nseq > 0 && (!d_bases || !d_offs_u32))) return fail(RK_ERR_ARG, "bad arguments");
    if (nseq > 0x7fffffffll) return fail(RK_ERR_LIMIT, "more than 2^31-1 sequences in one batch");
    if (nseq == 0) return RK_OK;
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    return launch_count(s, d_bases, d_offs_u32, (uint32_t)nseq, bound_bases, st);
}
}

extern "C" void rk_screen_destroy(rk_screen* s) {
    if (!s) return;
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipDeviceSynchronize(); // (a feed on the caller's stream may still be in flight)
    (void)e;
    if (s->ix) rk_scaled_index_destroy(s->ix);
    for (DevBuf* b : {&s->dir, &s->roff, &s->pos, &s->counts, &s->state, &s->owner, &s->w_out, &s->w_bases, &s->w_offs, &s->w_vals, &s->w_cnts}) b->release();
    s->h_state.release();
    delete s;
}

extern "C" int rk_screen_create(rk_ctx* c, const int* ks, int nks, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, rk_screen** out) {
    if (!c || !out || !r_offsets) return fail(RK_ERR_ARG, "bad arguments");
    KsArr ka{};
    RKCHK(check_ks(ks, nks, &ka));
    if (nref < 1) return fail(RK_ERR_ARG, "screen: need at least one reference sketch, got %lld", (long long)nref);
    if (nref > 0x7fffffffll) return fail(RK_ERR_LIMIT, "screen: %lld reference sketches are more than 2^31-1", (long long)nref);
    RKCHK(check_csr(r_offsets, nref, "screen: ", "the references", RK_ERR_LIMIT));
    if (r_offsets[nref] > r_offsets[0] && !r_values) return fail(RK_ERR_ARG, "bad arguments");
    // the rows collapsed: ascending, repeats dropped
    std::vector<uint64_t> cv, co((size_t)nref + 1, 0);
    cv.reserve((size_t)(r_offsets[nref] - r_offsets[0]));
    for (int64_t r = 0; r < nref; ++r) {
        for (uint64_t t = r_offsets[r]; t < r_offsets[r + 1]; ++t) {
            const uint64_t v = r_values[t];
            if (v == 0) return fail(RK_ERR_ARG, "screen: value %llu of reference %lld is 0", (unsigned long long)(t - r_offsets[r]), (long long)r);
            if (t > r_offsets[r] && v < r_values[t - 1]) return fail(RK_ERR_ARG, "screen: reference %lld descends at value %llu", (long long)r, (unsigned long long)(t - r_offsets[r]));
            if (t == r_offsets[r] || v != r_values[t - 1]) cv.push_back(v);
        }
        co[(size_t)r + 1] = cv.size();
    }
    if (cv.size() > 0xffffffffull) return fail(RK_ERR_LIMIT, "screen: %llu reference values are more than 2^32-1", (unsigned long long)cv.size());
    RKCHK(set_dev(c));
    rk_screen* s = new rk_screen();
    struct Guard { rk_screen* s; ~Guard() { if (s) rk_screen_destroy(s); } } guard{s};
    s->ctx = c; s->device = c->device; s->ks = ka; s->nref = (uint32_t)nref; s->nvalues = cv.size();
    for (int j = 0; j < ka.n; ++j) s->kmax = std::max(s->kmax, (int)ka.k[j]);
    RKCHK(rk_scaled_index_create(c, cv.data(), co.data(), nref, &s->ix)); // (synchronises the context's stream)
    s->nkeys = s->ix->nkeys;
    std::vector<uint64_t> keys((size_t)s->nkeys);
    if (s->nkeys) {
        HIPCHK(hipMemcpyAsync(keys.data(), s->ix->keys.p, (size_t)s->nkeys * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(hipStreamSynchronize(c->st));
        for (size_t j = 1; j < keys.size(); ++j)
            if (keys[j] <= keys[j - 1]) return fail(RK_ERR_HIP, "screen: the keys of the index do not ascend at %zu", j);
    }
    // where every reference value stands among the keys
    std::vector<uint32_t> pos(cv.size());
    for (size_t t = 0; t < cv.size(); ++t) {
        const size_t p = (size_t)(std::lower_bound(keys.begin(), keys.end(), cv[t]) - keys.begin());
        if (p >= keys.size() || keys[p] != cv[t]) return fail(RK_ERR_HIP, "screen: reference value %zu is no key of the index", t);
        pos[t] = (uint32_t)p;
    }
    // the directory over the leading bits below the largest key: about two buckets per key
    s->max_key = keys.empty() ? 0 : keys.back();
    int bits_key = 0;
    while (bits_key < 64 && (s->max_key >> bits_key) != 0) ++bits_key;
    int dir_bits = SC_DIR_MIN_BITS;
    while (dir_bits < SC_DIR_MAX_BITS && ((uint64_t)1 << dir_bits) < 2 * s->nkeys) ++dir_bits;
    s->dir_shift = (uint32_t)std::max(bits_key - dir_bits, 0);
    s->ndir = (uint32_t)(s->max_key >> s->dir_shift) + 1; // at most 2^dir_bits
    std::vector<uint32_t> dir((size_t)s->ndir + 1);
    {
        size_t j = 0;
        for (uint32_t b = 0; b <= s->ndir; ++b) { // dir[b] = the first key whose bucket is not below b
            while (j < keys.size() && (keys[j] >> s->dir_shift) < (uint64_t)b) ++j;
            dir[b] = (uint32_t)j;
        }
    }
    RKCHK(s->dir.reserve(dir.size() * 4));
    RKCHK(s->roff.reserve(co.size() * 8));
    RKCHK(s->pos.reserve(pos.size() * 4 + 4));
    RKCHK(s->counts.reserve((size_t)s->nkeys * 8 + 8));
    RKCHK(s->owner.reserve((size_t)s->nkeys * 4 + 4));
    RKCHK(s->state.reserve(32));
    RKCHK(s->h_state.reserve(64));
    HIPCHK(hipMemcpyAsync(s->dir.p, dir.data(), dir.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(s->roff.p, co.data(), co.size() * 8, hipMemcpyHostToDevice, c->st));
    if (!pos.empty()) HIPCHK(hipMemcpyAsync(s->pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemsetAsync(s->counts.p, 0, (size_t)s->nkeys * 8 + 8, c->st));
    HIPCHK(hipMemsetAsync(s->state.p, 0, 32, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    guard.s = nullptr;
    *out = s;
    return RK_OK;
}

extern "C" int rk_screen_reset(rk_screen* s) {
    RKCHK(check_screen(s));
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipMemsetAsync(s->counts.p, 0, (size_t)s->nkeys * 8 + 8, s->ctx->st));
    HIPCHK(hipMemsetAsync(s->state.p, 0, 32, s->ctx->st));
    HIPCHK(hipStreamSynchronize(s->ctx->st));
    s->injected = 0;
    return RK_OK;
}

extern "C" int rk_screen_stats(rk_screen* s, rk_screen_stats_t* out) {
    RKCHK(check_screen(s));
    if (!out || out->struct_size < sizeof(uint32_t)) return fail(RK_ERR_ARG, "bad arguments");
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    uint64_t* h = s->h_state.as<uint64_t>();
    HIPCHK(hipMemcpyAsync(h, s->state.p, 24, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    rk_screen_stats_t t{};
    t.nref = s->nref; t.dir_shift = s->dir_shift; t.dir_buckets = s->ndir;
    t.nkeys = s->nkeys; t.nseq = h[0]; t.nbases = h[1]; t.counted = h[2]; t.injected = s->injected;
    const uint32_t size = std::min<uint32_t>(out->struct_size, (uint32_t)sizeof t);
    t.struct_size = size;
    memcpy(out, &t, size);
    return RK_OK;
}

extern "C" int rk_screen_add_batch_device(rk_screen* s, const void* d_bases, const void* d_offsets_u32, int64_t nseq, void* hip_stream) {
    return screen_feed_device(s, d_bases, d_offsets_u32, nseq, 0, (hipStream_t)hip_stream);
}

extern "C" int rk_screen_add_batch(rk_screen* s, const uint8_t* bases, const uint64_t* offsets, int64_t nseq) {
    RKCHK(check_screen(s));
    if (!offsets || nseq < 0) return fail(RK_ERR_ARG, "bad arguments");
    for (int64_t i = 0; i < nseq; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(RK_ERR_ARG, "offsets decrease at sequence %lld", (long long)i);
        if (offsets[i + 1] - offsets[i] > 0x7fffffffull) return fail(RK_ERR_LIMIT, "sequence %lld holds 2^31 bases or more", (long long)i);
    }
    if (nseq > 0 && offsets[nseq] > offsets[0] && !bases) return fail(RK_ERR_ARG, "bad arguments");
    if (nseq == 0) return RK_OK;
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    std::vector<uint32_t> off32;
    for (int64_t i0 = 0; i0 < nseq;) { // pieces of whole sequences; a sequence longer than a piece is alone in its own
        int64_t i1 = i0 + 1;
        while (i1 < nseq && offsets[i1 + 1] - offsets[i0] <= SC_PIECE_BASES && i1 - i0 < ((int64_t)1 << 22)) ++i1;
        const uint64_t nb = offsets[i1] - offsets[i0];
        off32.resize((size_t)(i1 - i0) + 1);
        for (int64_t i = i0; i <= i1; ++i) off32[(size_t)(i - i0)] = (uint32_t)(offsets[i] - offsets[i0]);
        RKCHK(s->w_bases.reserve((size_t)nb + 64));
        RKCHK(s->w_offs.reserve(off32.size() * 4));
        if (nb) HIPCHK(hipMemcpyAsync(s->w_bases.p, bases + offsets[i0], (size_t)nb, hipMemcpyHostToDevice, c->st));
        HIPCHK(hipMemcpyAsync(s->w_offs.p, off32.data(), off32.size() * 4, hipMemcpyHostToDevice, c->st));
        RKCHK(launch_count(s, s->w_bases.p, s->w_offs.p, (uint32_t)(i1 - i0), nb, c->st));
        HIPCHK(hipStreamSynchronize(c->st)); // off32 and the two buffers may be refilled
        i0 = i1;
    }
    return RK_OK;
}

extern "C" int rk_screen_add_counts(rk_screen* s, const uint64_t* values, const uint32_t* counts, uint64_t n) {
    RKCHK(check_screen(s));
    if (n && (!values || !counts)) return fail(RK_ERR_ARG, "bad arguments");
    if (n > 0x7fffffffull) return fail(RK_ERR_LIMIT, "screen: a counted set of 2^31 values or more");
    for (uint64_t i = 0; i < n; ++i) {
        if (values[i] == 0) return fail(RK_ERR_ARG, "screen: value %llu of the counted set is 0", (unsigned long long)i);
        if (i && values[i] <= values[i - 1]) return fail(RK_ERR_ARG, "screen: the counted set does not ascend at value %llu", (unsigned long long)i);
    }
    if (n == 0) return RK_OK;
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(s->w_vals.reserve((size_t)n * 8));
    RKCHK(s->w_cnts.reserve((size_t)n * 4));
    HIPCHK(hipMemcpyAsync(s->w_vals.p, values, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(s->w_cnts.p, counts, (size_t)n * 4, hipMemcpyHostToDevice, c->st));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + TW_T - 1) / TW_T, 4096);
    hipLaunchKernelGGL(k_screen_inject, dim3(grid), dim3(TW_T), 0, c->st, s->w_vals.as<uint64_t>(), s->w_cnts.as<uint32_t>(), n, screen_keys(s),
                       s->counts.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->st));
    for (uint64_t i = 0; i < n; ++i) s->injected += counts[i];
    return RK_OK;
}

extern "C" int rk_screen_rows_device(rk_screen* s, uint64_t min_copies, void* d_out4, void* hip_stream) {
    RKCHK(check_screen(s));
    if (!d_out4) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_min_copies(min_copies));
    RKCHK(set_dev(s->ctx));
    std::lock_guard<std::mutex> lk(s->mu);
    return launch_rows(s, (uint32_t)min_copies, (uint32_t*)d_out4, (hipStream_t)hip_stream);
}

extern "C" int rk_screen_rows(rk_screen* s, uint64_t min_copies, uint32_t* out4) {
    RKCHK(check_screen(s));
    if (!out4) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(check_min_copies(min_copies));
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    RKCHK(s->w_out.reserve((size_t)s->nref * 16));
    RKCHK(launch_rows(s, (uint32_t)min_copies, s->w_out.as<uint32_t>(), c->st));
    HIPCHK(hipMemcpyAsync(out4, s->w_out.p, (size_t)s->nref * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

extern "C" int rk_screen_counts(rk_screen* s, uint64_t** keys_out, uint64_t** counts_out, uint64_t* nkeys) {
    RKCHK(check_screen(s));
    if (!keys_out || !counts_out || !nkeys) return fail(RK_ERR_ARG, "bad arguments");
    rk_ctx* c = s->ctx;
    RKCHK(set_dev(c));
    std::lock_guard<std::mutex> lk(s->mu);
    const uint64_t n = s->nkeys;
    uint64_t* k = (uint64_t*)malloc((size_t)std::max<uint64_t>(n, 1) * 8);
    uint64_t* v = (uint64_t*)malloc((size_t)std::max<uint64_t>(n, 1) * 8);
    if (!k || !v) { free(k); free(v); return fail(RK_ERR_NOMEM, "malloc of %llu screen counts", (unsigned long long)n); }
    hipError_t e = hipSuccess;
    if (n) e = hipMemcpyAsync(k, s->ix->keys.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st);
    if (n && e == hipSuccess) e = hipMemcpyAsync(v, s->counts.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) { free(k); free(v); return fail(RK_ERR_HIP, "download of the screen counts failed: %s", hipGetErrorString(e)); }
    *keys_out = k;
    *counts_out = v;
    *nkeys = n;
    return RK_OK;
}
