// rk_api.hip -- the C ABI of include/rkmh_amd.h on top of the gfx950 kernels (rk_kernels.hip).
// Host-side orchestration only: device memory, tile descriptors, the reference index build, the
// pinned double-buffered H2D/D2H pipeline.  No CPU implementation of any hashing/sketching step lives
// here: every entry point fails with RK_ERR_HIP when no GPU is usable.
#include "rk_api_internal.hpp"

static thread_local std::string g_err;
int rk::fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* rk_last_error(void) { return g_err.c_str(); }
extern "C" void rk__set_error(const char* msg) { g_err = msg ? msg : ""; }
extern "C" const char* rk_version(void) { return "rkmh_amd 0.1 (gfx950)"; }
extern "C" void rk_default_policy(rk_policy* p) {
    p->fold = RK_FOLD_SWAP32; p->drop_last_window = 1; p->counter_counts_zero = 1;
    p->mask_strict_less = 1; p->freq_max_inclusive = 1; p->seed = 42;
    p->canon = RK_CANON_MINHASH;
}
extern "C" int rk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" void rk__pool_forget(void* p); // rk_pool.cpp: big parser buffers are tracked for recycling
extern "C" void rk_free(void* p) { rk__pool_forget(p); free(p); }

extern "C" int rk_device_props(int device, int32_t* compute_units, int32_t* clock_khz, int64_t* l2_bytes, int64_t* hbm_bytes) {
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, device);
    if (e != hipSuccess) return fail(RK_ERR_HIP, "hipGetDeviceProperties(%d): %s", device, hipGetErrorString(e));
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (clock_khz) *clock_khz = p.clockRate;
    if (l2_bytes) *l2_bytes = p.l2CacheSize;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return RK_OK;
}

extern "C" int rk_ctx_create(int device, const rk_policy* policy, rk_ctx** out) {
    if (!out) return fail(RK_ERR_ARG, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(RK_ERR_HIP, "no HIP device available (%s): rkmh_amd has no CPU fallback", hipGetErrorString(e));
    if (device < 0 || device >= n) return fail(RK_ERR_ARG, "device %d out of range [0,%d)", device, n);
    HIPCHK(hipSetDevice(device));
    rk_ctx* c = new rk_ctx();
    c->device = device;
    rk_policy p;
    if (policy) p = *policy; else rk_default_policy(&p);
    if ((rk_policy_strand(&p) != RK_CANON_MINHASH && rk_policy_strand(&p) != RK_CANON_LEXMIN) || (p.canon & ~(RK_CANON_STRAND_MASK | RK_DEDUP_DISTINCT)) != 0) {
        delete c; return fail(RK_ERR_ARG, "hash policy: field 'canon' holds an unknown value");
    }
    c->pol.fold = p.fold; c->pol.drop_last_window = p.drop_last_window;
    c->pol.counter_counts_zero = p.counter_counts_zero; c->pol.mask_strict_less = p.mask_strict_less;
    c->pol.freq_max_inclusive = p.freq_max_inclusive; c->pol.seed = p.seed;
    c->pol.canon = rk_policy_strand(&p); // the kernels' policy carries the strand rule alone; U6 acts through the launches (c->dedup)
    c->dedup = rk_policy_dedup(&p) != 0;
    HIPCHK(hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking));
    for (auto& s : c->slot) {
        HIPCHK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
    *out = c;
    return RK_OK;
}
extern "C" int rk_ctx_policy(const rk_ctx* c, rk_policy* out) {
    if (!c || !out) return fail(RK_ERR_ARG, "bad arguments");
    out->fold = c->pol.fold; out->drop_last_window = c->pol.drop_last_window; out->counter_counts_zero = c->pol.counter_counts_zero;
    out->mask_strict_less = c->pol.mask_strict_less; out->freq_max_inclusive = c->pol.freq_max_inclusive; out->seed = c->pol.seed;
    out->canon = c->pol.canon | (c->dedup ? RK_DEDUP_DISTINCT : 0);
    return RK_OK;
}
extern "C" void rk_ctx_destroy(rk_ctx* c) {
    if (!c) return;
    hipError_t e = hipSetDevice(c->device); (void)e;
    e = hipDeviceSynchronize(); (void)e;
    for (DevBuf* b : {&c->d_fpb, &c->d_base, &c->d_kv, &c->d_post, &c->d_pre, &c->d_keepbits, &c->d_kpost, &c->d_kbase, &c->d_kkeys, &c->d_kslots, &c->w_bases, &c->w_tiles, &c->w_hashes, &c->w_segoff,
                      &c->w_ids, &c->w_sk, &c->w_lens, &c->w_out, &c->w_misc, &c->w_sel, &c->w_selstate, &c->w_table, &c->w_gcount, &c->w_tail, &c->w_dedup,
                      &c->w_sc_cnt, &c->w_sc_pre, &c->w_sc_off, &c->w_sc_a, &c->w_sc_b, &c->w_sc_src, &c->w_sc_ab,
                      &c->w_g_hit, &c->w_g_total, &c->w_g_alive, &c->w_g_state, &c->w_g_cand, &c->w_g_coff, &c->w_g_count, &c->w_g_list, &c->w_g_ab}) b->release();
    for (int j = 0; j < KM_MAX_KS; ++j) { c->d_kf4[j].release(); c->d_km1[j].release(); c->d_km1v[j].release(); c->d_km1m[j].release(); c->d_km1cells[j].release(); }
    c->d_keepkey.release(); c->d_kvm.release();
    for (auto& s : c->slot) {
        s.h_bases.release(); s.h_offs.release(); s.h_out.release();
        s.d_bases.release(); s.d_offs.release(); s.d_out.release();
        if (s.done) { e = hipEventDestroy(s.done); (void)e; }
        if (s.st) { e = hipStreamDestroy(s.st); (void)e; }
    }
    if (c->st) { e = hipStreamDestroy(c->st); (void)e; }
    delete c;
}
extern "C" void* rk_ctx_stream(rk_ctx* c) { return c ? (void*)c->st : nullptr; }
extern "C" int rk_ctx_synchronize(rk_ctx* c) {
    if (!c) return fail(RK_ERR_ARG, "ctx is NULL");
    RKCHK(set_dev(c));
    HIPCHK(hipDeviceSynchronize());
    return RK_OK;
}

int check_ks(const int* ks, int nks, KsArr* out) {
    if (!ks || nks < 1 || nks > RK_MAX_KS) return fail(RK_ERR_ARG, "need 1..%d k-mer sizes, got %d", RK_MAX_KS, nks);
    out->n = nks;
    for (int i = 0; i < nks; ++i) {
        if (ks[i] < 1 || ks[i] > RK_MAX_K) return fail(RK_ERR_LIMIT, "k=%d outside [1,%d]", ks[i], RK_MAX_K);
        out->k[i] = ks[i];
    }
    return RK_OK;
}

// ---- host memory: page-locked buffers, temporary registrations, the staged upload ----------------
// is [p, p + bytes) page-locked host memory the DMA engines can read directly (rk_host_alloc, hipHostMalloc, hipHostRegister)?
bool is_pinned_host(const void* p, size_t bytes) {
    if (!p || bytes == 0) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeHost) return false;
    hipPointerAttribute_t b;
    if (hipPointerGetAttributes(&b, (const char*)p + bytes - 1) != hipSuccess) { (void)hipGetLastError(); return false; }
    return b.type == hipMemoryTypeHost;
}

// Page-locks a caller's pageable buffer for the duration of one call (hipHostRegister of memory that is already touched takes
// 2-3 ms per 256 MB on the MI355X host, measured: tools/ubench/host_register.hip -- a tenth of the staging copy it replaces), so the
// DMA engines read / write it in place.  Fails quietly (read-only mappings, a page shared with another registration, a platform
// limit): the caller then takes the staging path.  RKMH_HOST_REGISTER=0 disables.
// Several host threads may work on neighbouring pieces of ONE caller buffer (bin/rkmh --devices: a context per device, each with its
// range of the reads): their page-rounded registrations would overlap, and a piece whose first and last byte lie in a neighbour's
// registered pages would LOOK page-locked (is_pinned_host samples both ends) while its middle is not.  So temporary registrations
// are kept in a process-wide list: a range that touches another thread's registration is neither registered nor trusted.
static std::mutex g_temp_reg_mu;
static std::vector<std::pair<uintptr_t, uintptr_t>> g_temp_reg; // [lo, hi) page ranges registered by a ScopedHostRegister that is alive
static bool touches_temp_registration(const void* p, size_t bytes) { // caller holds g_temp_reg_mu
    const uintptr_t lo = (uintptr_t)p & ~(uintptr_t)4095, hi = ((uintptr_t)p + bytes + 4095) & ~(uintptr_t)4095;
    for (const auto& r : g_temp_reg) if (lo < r.second && r.first < hi) return true;
    return false;
}
// is_pinned_host for a caller's buffer: page-locked by the caller, not merely overlapping a temporary registration of ours
bool caller_pinned_host(const void* p, size_t bytes) {
    if (!p || bytes == 0) return false;
    std::lock_guard<std::mutex> l(g_temp_reg_mu);
    return !touches_temp_registration(p, bytes) && is_pinned_host(p, bytes);
}
static bool host_register_enabled() {
    static const bool on = [] { const char* e = getenv("RKMH_HOST_REGISTER"); return !(e && *e == '0'); }();
    return on;
}
ScopedHostRegister::ScopedHostRegister(const void* p, size_t bytes, size_t min_bytes) {
    if (!p || bytes < min_bytes || !host_register_enabled()) return;
    std::lock_guard<std::mutex> l(g_temp_reg_mu);
    if (touches_temp_registration(p, bytes)) return; // a neighbouring piece of the same buffer is registered: staging path
    lo = (uintptr_t)p & ~(uintptr_t)4095; hi = ((uintptr_t)p + bytes + 4095) & ~(uintptr_t)4095;
    if (hipHostRegister((void*)lo, hi - lo, hipHostRegisterPortable) == hipSuccess) { ok = true; g_temp_reg.emplace_back(lo, hi); }
    else (void)hipGetLastError();
}
ScopedHostRegister::~ScopedHostRegister() {
    if (!ok) return;
    std::lock_guard<std::mutex> l(g_temp_reg_mu);
    hipError_t e = hipHostUnregister((void*)lo); (void)e;
    for (size_t i = 0; i < g_temp_reg.size(); ++i) if (g_temp_reg[i].first == lo && g_temp_reg[i].second == hi) { g_temp_reg.erase(g_temp_reg.begin() + (long)i); break; }
}

// Host -> device copy of a pageable buffer through the context's two pinned staging buffers (the same ones the fused
// host pipeline uses): the CPU fills one while the DMA engine drains the other.  hipMemcpyAsync straight from pageable
// memory runs at a fraction of the link rate and blocks the caller for the whole transfer.
int upload_staged(rk_ctx* c, void* dst, const uint8_t* src, size_t bytes, hipStream_t st) {
    const size_t CH = 16u << 20;
    // (a few megabytes -- a reference panel -- are not worth two 16 MB page-locked buffers: creating those takes longer than the copy)
    if (bytes <= (4u << 20)) { HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); return RK_OK; }
    for (int i = 0; i < 2; ++i) {
        if (c->slot[i].busy) { HIPCHK(hipEventSynchronize(c->slot[i].done)); c->slot[i].busy = false; }
        RKCHK(c->slot[i].h_bases.reserve(CH));
    }
    int which = 0;
    bool used[2] = {false, false};
    for (size_t off = 0; off < bytes; off += CH) {
        const size_t nb = bytes - off < CH ? bytes - off : CH;
        Slot& sl = c->slot[which];
        if (used[which]) HIPCHK(hipEventSynchronize(sl.done)); // its previous chunk has left the pinned buffer
        par_memcpy(sl.h_bases.p, src + off, nb);
        HIPCHK(hipMemcpyAsync((uint8_t*)dst + off, sl.h_bases.p, nb, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(sl.done, st));
        used[which] = true;
        which ^= 1;
    }
    return RK_OK;
}

// page-locked host memory for callers that want rk_classify_batch / rk_count_batch to run at link speed (no staging copy)
extern "C" int rk_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(RK_ERR_ARG, "out is NULL");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { *out = nullptr; return fail(RK_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    return RK_OK;
}
// page-lock caller memory that is only read (a mapping of an input file): the DMA engines then read it in place
extern "C" int rk_host_register_readonly(const void* p, size_t bytes) {
    if (!p || !bytes) return fail(RK_ERR_ARG, "bad arguments");
    hipError_t e = hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterReadOnly);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostRegister(const_cast<void*>(p), bytes, hipHostRegisterDefault); }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(RK_ERR_HIP, "hipHostRegister(%zu bytes): %s", bytes, hipGetErrorString(e)); }
    return RK_OK;
}
extern "C" void rk_host_unregister(const void* p) { if (p) { hipError_t e = hipHostUnregister(const_cast<void*>(p)); (void)e; } }
extern "C" void rk_host_free(void* p) { if (p) { hipError_t e = hipHostFree(p); (void)e; } }

// device memory for callers that keep arrays resident between calls of the *_device entries without a HIP runtime of their own (the
// command line: `rkmh gather` uploads its references once); the copies run on the context's stream and return when they are done
extern "C" int rk_device_alloc(rk_ctx* c, size_t bytes, void** out) {
    if (!c || !out) return fail(RK_ERR_ARG, "bad arguments");
    *out = nullptr;
    RKCHK(set_dev(c));
    hipError_t e = hipMalloc(out, bytes ? bytes : 1);
    if (e != hipSuccess) { *out = nullptr; return fail(RK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)); }
    return RK_OK;
}
extern "C" void rk_device_free(rk_ctx* c, void* p) {
    if (!c || !p) return;
    hipError_t e = hipSetDevice(c->device); (void)e;
    e = hipFree(p); (void)e;
}
extern "C" int rk_device_upload(rk_ctx* c, void* d_dst, const void* src, size_t bytes) {
    if (!c || ((!d_dst || !src) && bytes)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    if (bytes) HIPCHK(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}
extern "C" int rk_device_download(rk_ctx* c, void* dst, const void* d_src, size_t bytes) {
    if (!c || ((!dst || !d_src) && bytes)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

// ---- inner boundary: the mirrors that are one copy-launch-copy ----------------------------------
extern "C" int rk_to_upper(rk_ctx* c, char* seq, int len) {
    if (!c || (!seq && len > 0) || len < 0) return fail(RK_ERR_ARG, "bad arguments");
    if (len == 0) return RK_OK;
    RKCHK(set_dev(c));
    RKCHK(c->w_bases.reserve((size_t)len));
    HIPCHK(hipMemcpyAsync(c->w_bases.p, seq, (size_t)len, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_to_upper(c->w_bases.as<uint8_t>(), (uint64_t)len, c->st));
    HIPCHK(hipMemcpyAsync(seq, c->w_bases.p, (size_t)len, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

extern "C" int rk_mask_by_frequency(rk_ctx* c, uint64_t* h, int n, const rk_counter* counter, int min_occ) {
    if (!c || !counter || (!h && n > 0) || n < 0) return fail(RK_ERR_ARG, "bad arguments");
    if (n == 0) return RK_OK;
    RKCHK(set_dev(c));
    RKCHK(c->w_hashes.reserve((size_t)n * 8));
    HIPCHK(hipMemcpyAsync(c->w_hashes.p, h, (size_t)n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_mask_by_frequency(c->w_hashes.as<uint64_t>(), (uint64_t)n, counter->d, counter->slots, min_occ, c->pol, c->st));
    HIPCHK(hipMemcpyAsync(h, c->w_hashes.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

extern "C" int rk_hash_intersection_size(rk_ctx* c, const uint64_t* a, int na, const uint64_t* b, int nb, int* out) {
    if (!c || !out || na < 0 || nb < 0 || (!a && na) || (!b && nb)) return fail(RK_ERR_ARG, "bad arguments");
    RKCHK(set_dev(c));
    RKCHK(c->w_hashes.reserve((size_t)(na + nb + 2) * 8));
    RKCHK(c->w_lens.reserve(4));
    uint64_t* da = c->w_hashes.as<uint64_t>();
    uint64_t* db = da + na;
    if (na) HIPCHK(hipMemcpyAsync(da, a, (size_t)na * 8, hipMemcpyHostToDevice, c->st));
    if (nb) HIPCHK(hipMemcpyAsync(db, b, (size_t)nb * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_intersect_pair(da, na, db, nb, c->w_lens.as<int>(), c->st));
    HIPCHK(hipMemcpyAsync(out, c->w_lens.p, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return RK_OK;
}

// mkmh::hash_intersection with 7 arguments, as filter's classify_* helpers call it (equiv.hpp:308, 340, 364): (array, start,
// length) twice, then the sketch size, which bounds the result.  Callee-allocated result, released with rk_free.
extern "C" int rk_hash_intersection(rk_ctx* c, const uint64_t* a, int a_start, int a_len, const uint64_t* b, int b_start, int b_len,
                                    int S, uint64_t** out, int* n) {
    if (!c || !out || !n || a_start < 0 || b_start < 0 || a_len < 0 || b_len < 0 || S < 0 || (!a && a_len) || (!b && b_len))
        return fail(RK_ERR_ARG, "bad arguments");
    *out = nullptr; *n = 0;
    RKCHK(set_dev(c));
    const int cap = S < a_len ? S : a_len;
    RKCHK(c->w_hashes.reserve((size_t)(a_len + b_len + cap + 2) * 8));
    RKCHK(c->w_lens.reserve(4));
    uint64_t* da = c->w_hashes.as<uint64_t>();
    uint64_t* db = da + a_len;
    uint64_t* dout = db + b_len;
    if (a_len) HIPCHK(hipMemcpyAsync(da, a + a_start, (size_t)a_len * 8, hipMemcpyHostToDevice, c->st));
    if (b_len) HIPCHK(hipMemcpyAsync(db, b + b_start, (size_t)b_len * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(launch_intersect_pair_emit(da, a_len, db, b_len, cap, dout, c->w_lens.as<int>(), c->st));
    int cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, c->w_lens.p, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    uint64_t* r = (uint64_t*)malloc((size_t)(cnt > 0 ? cnt : 1) * 8);
    if (!r) return fail(RK_ERR_NOMEM, "malloc");
    if (cnt) HIPCHK(hipMemcpy(r, dout, (size_t)cnt * 8, hipMemcpyDeviceToHost));
    *out = r; *n = cnt;
    return RK_OK;
}
