// rk_tile_walk.hpp -- the walk over the windows of a resident read batch that the sample accumulator (rk_sample.hip, k_sample_keep) and
// the screen (rk_screen.hip, k_screen_count) share: the bases of a batch as ONE piece cut into tiles of HASH_TILE_WIN window positions,
// a tile staged in LDS, the read starts that fall into it marked in a bitmap, every position that is a window of its read hashed.  What
// becomes of a hash is the caller's: walk_tiles hands every round of TW_T positions to a callable.  Everything has internal linkage.
#pragma once
#include "rk_api_internal.hpp"

namespace {

constexpr int TW_T = 256;                                              // threads of a workgroup that walks
constexpr int TW_BND_DW = (HASH_TILE_WIN + MAX_K + 2 + 31) / 32 + 2;   // the read-start bitmap of a tile (+ the word no_boundary reads ahead)
constexpr uint32_t TW_BND_BITS = (uint32_t)(TW_BND_DW - 2) * 32u;

// bits [bit, bit + left) of the bitmap all zero?  (window_valid's walk, on the read-start bitmap)
__device__ __forceinline__ bool no_boundary(const uint32_t* bnd, uint32_t bit, int left) {
    uint32_t idx = bit >> 5;
    const uint32_t sh = bit & 31;
    uint32_t lo = bnd[idx], acc = 0;
    while (left > 0) {
        const uint32_t hi = bnd[idx + 1];
        const uint32_t x = __builtin_amdgcn_alignbit(hi, lo, sh);
        acc |= x & (left >= 32 ? 0xffffffffu : ((1u << left) - 1u));
        lo = hi; ++idx; left -= 32;
    }
    return acc == 0;
}

// The bases of a batch, offs[0] = first .. offs[n] = end (end > first), as ONE piece cut into tiles of HASH_TILE_WIN window positions
// (grid-stride).  A tile stages its positions and the kmax - 1 bases behind them in lds[stage_lds_dwords(HASH_TILE_MAXB)], marks the read
// starts that fall into it in bnd[TW_BND_DW], and hashes position p at every k of the list that this instantiation serves (KT = 16:
// k = 16; KT = 0: every other k).  p is a window of its read when no read start lies in (p, p + k - 1 + drop_last_window]: the read
// then holds k bases from p on, and one more where the policy drops the last window.  offs[n], the end of the last read, is a start
// like the others.  round(h) is called by WHOLE workgroups, once per TW_T positions and k: h is the thread's window hash, 0 where its
// position is no window (or hashes to 0: an invalid base); it may use barriers.
template <int KT, typename Round>
__device__ __forceinline__ void walk_tiles(const uint8_t* __restrict__ bases, const uint32_t* __restrict__ offs, uint32_t n, uint32_t first, uint32_t end,
                                           const KsArr& ks, int kmax, const DevPolicy& pol, uint32_t* lds, uint32_t* bnd, Round&& round) {
    const uint32_t total = end - first;
    const uint32_t ntiles = (uint32_t)(((uint64_t)total + HASH_TILE_WIN - 1) / HASH_TILE_WIN);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        __syncthreads(); // the readers of the tile before are done
        const uint32_t a = first + tile * (uint32_t)HASH_TILE_WIN; // below `end`
        const uint32_t left = end - a;
        const uint32_t nb = min(left, (uint32_t)(HASH_TILE_WIN + kmax - 1));
        const uint32_t nwin = min(left, (uint32_t)HASH_TILE_WIN);
        const Staged s = stage_piece(bases, (uint64_t)a, nb, lds, HASH_TILE_MAXB, threadIdx.x, TW_T, [] { __syncthreads(); });
        for (uint32_t i = threadIdx.x; i < (uint32_t)TW_BND_DW; i += TW_T) bnd[i] = 0;
        __syncthreads();
        // the first read start behind the tile's first position: one binary search; the ones after it are marked while they fall into the bitmap
        uint32_t lo = 0, hi = n + 1;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (offs[mid] <= a) lo = mid + 1; else hi = mid;
        }
        for (uint32_t r = lo + threadIdx.x; r <= n; r += TW_T) {
            const uint32_t rel = offs[r] - a; // (offsets that do not ascend: a wrapped difference ends the walk)
            if (rel >= TW_BND_BITS) break;
            atomicOr(&bnd[rel >> 5], 1u << (rel & 31u));
        }
        __syncthreads();
        for (int j = 0; j < ks.n; ++j) {
            const int k = ks.k[j];
            if (KT ? k != KT : k == 16) continue; // the other instantiation's
            const int span = k - 1 + (pol.drop_last_window ? 1 : 0);
            for (uint32_t i0 = 0; i0 < nwin; i0 += TW_T) { // whole workgroups
                const uint32_t i = i0 + threadIdx.x;
                uint64_t h = 0;
                if (i < nwin && i + (uint32_t)k <= nb && no_boundary(bnd, i + 1, span)) h = canonical_window<KT>(s, i, k, pol);
                round(h);
            }
        }
    }
}

} // namespace
