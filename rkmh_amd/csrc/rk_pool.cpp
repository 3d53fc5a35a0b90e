// rk_pool.cpp -- recycling of the big batch buffers that the read parser hands to its callers.
//
// A 256 MB batch handed to the caller comes back through rk_seqset_free a few milliseconds later; glibc serves and releases blocks of
// that size with mmap / munmap, so every batch paid ~65 000 page faults again (measured on bin/rkmh stream, 16 M reads: 2.4 s of
// system time against 2.0 s of user time).  Buffers of at least 1 MB that this library hands out are remembered with their capacity;
// rk_seqset_free parks up to POOL_SLOTS of them and the next batch's arrays start from a parked buffer instead of a fresh mapping.
// rk_free forgets a pointer before freeing it.
#include "rk_parse_internal.hpp"

#include <unordered_map>

namespace rkparse {
namespace pool {
constexpr size_t MIN_BYTES = (size_t)1 << 20, MAX_BYTES = (size_t)512 << 20, POOL_SLOTS = 24, POOL_BYTES = (size_t)3 << 29; // park at most 1.5 GB
struct State {
    std::mutex mu;
    std::unordered_map<void*, size_t> cap;           // every live buffer of >= MIN_BYTES this library handed out
    std::vector<std::pair<size_t, void*>> parked;    // (capacity, buffer) ready for reuse
    size_t parked_bytes = 0;
};
static State& st() { static State* s = new State(); return *s; } // leaked on purpose: buffers may be returned during exit
void remember(void* p, size_t bytes) {
    if (!p) return;
    std::lock_guard<std::mutex> g(st().mu);
    // an address this map still knows from an EARLIER buffer (one the caller released with plain free(), which the header allows
    // for malloc'd arrays) must not keep that buffer's capacity: a small buffer at the same address would later be parked and
    // reused with it.  The entry is overwritten, or dropped when the new buffer is too small to be worth parking.
    if (bytes < MIN_BYTES) st().cap.erase(p);
    else st().cap[p] = bytes;
}
void forget(void* p) {
    if (!p) return;
    std::lock_guard<std::mutex> g(st().mu);
    st().cap.erase(p);
}
void* take(size_t bytes, size_t* got) {
    if (bytes < MIN_BYTES) return nullptr;
    std::lock_guard<std::mutex> g(st().mu);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < st().parked.size(); ++i)
        if (st().parked[i].first >= bytes && st().parked[i].first <= 4 * bytes && (best == (size_t)-1 || st().parked[i].first < st().parked[best].first)) best = i;
    if (best == (size_t)-1) return nullptr;
    void* p = st().parked[best].second;
    *got = st().parked[best].first;
    st().parked_bytes -= *got;
    st().parked.erase(st().parked.begin() + (long)best);
    return p;
}
void give_back(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(st().mu);
        auto it = st().cap.find(p);
        if (it != st().cap.end()) {
            const size_t bytes = it->second;
            st().cap.erase(it);
            if (bytes <= MAX_BYTES && st().parked.size() < POOL_SLOTS && st().parked_bytes + bytes <= POOL_BYTES) {
                st().parked.emplace_back(bytes, p);
                st().parked_bytes += bytes;
                return;
            }
        }
    }
    free(p);
}
// frees every parked buffer (a long-lived caller that is done parsing gets its ~1.5 GB back)
static void trim() {
    std::vector<std::pair<size_t, void*>> old;
    {
        std::lock_guard<std::mutex> g(st().mu);
        old.swap(st().parked);
        st().parked_bytes = 0;
    }
    for (auto& e : old) free(e.second);
}
} // namespace pool
} // namespace rkparse

using namespace rkparse;

extern "C" {

void rk__pool_forget(void* p) { pool::forget(p); } // rk_free (rk_api.hip) calls this before free()
void rk_pool_trim(void) { pool::trim(); }

void rk_seqset_free(rk_seqset* s) {
    if (!s) return;
    pool::give_back(s->bases); pool::give_back(s->offsets); pool::give_back(s->names); pool::give_back(s->name_offsets); pool::give_back(s->quals);
    memset(s, 0, sizeof *s);
}

} // extern "C"
