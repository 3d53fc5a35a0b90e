/*
 * rkmh_amd.h -- C ABI of the MI355X-native rkmh classify/stream hot path.
 *
 * Drop-in boundary.  The reference has no FFI layer; the hot path sits behind
 * two concentric interfaces, both mirrored here with plain pointers and sizes:
 *
 *   inner  = the mkmh free functions called from /root/reference/src/rkmh.cpp and src/equiv.hpp
 *            (to_upper, calc_hashes, calc_hash, minhashes, mask_by_frequency,
 *             minhashes_frequency_filter, hash_intersection_size, HASHTCounter), and
 *   outer  = the per-read loop of main_stream (src/rkmh.cpp:813-898 and :904-948), which this
 *            library replaces by batched entry points (rk_set_references + rk_classify_batch*).
 *
 * Every compute entry point runs hand-written HIP kernels on a gfx950 device; there is NO CPU
 * fallback: without a usable GPU rk_ctx_create fails with RK_ERR_HIP and nothing else can be called.
 *
 * Ownership: buffers returned through `uint64_t**` are malloc'd by the library and released with
 * rk_free (the reference's convention is callee-new[] / caller-delete[], e.g. src/rkmh.cpp:823,864;
 * new[] must not cross a C ABI).  Batched entry points only use caller-owned buffers.
 * Errors: every function returns RK_OK (0) or a negative RK_ERR_*; rk_last_error() gives the text
 * (thread-local).  Threading: one rk_ctx per host thread (the reference calls mkmh concurrently from
 * OpenMP workers on disjoint data, src/rkmh.cpp:845-870; here concurrency is the batch itself).
 */
#ifndef RKMH_AMD_H
#define RKMH_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RK_OK 0
#define RK_ERR_ARG (-1)   /* bad argument */
#define RK_ERR_HIP (-2)   /* HIP runtime / no device */
#define RK_ERR_NOMEM (-3)
#define RK_ERR_STATE (-4) /* e.g. classify before rk_set_references */
#define RK_ERR_LIMIT (-5) /* exceeds a documented limit */
#define RK_ERR_IO (-6)
#define RK_ERR_NEED_FULL (-7) /* a compact depth map cannot answer this input: repeat the pass with a full rk_counter */

#define RK_MAX_KS 8     /* number of -k values per run (src/rkmh.cpp:680-682 pushes onto a vector) */
#define RK_MAX_K 64     /* largest k-mer size */
#define RK_MAX_SKETCH 16384 /* largest -s handled by the in-LDS sorter */

/* Unpinned mkmh choices -- identical meaning to oracle/rk_oracle.h */
enum { RK_FOLD_SWAP32 = 0, RK_FOLD_H1 = 1, RK_FOLD_W2W1 = 2 };
enum { RK_CANON_MINHASH = 0, RK_CANON_LEXMIN = 1 };
/* U6 rides in the `canon` word (its layout is fixed): the low byte is the strand rule, bit 8 the sketch rule */
enum { RK_CANON_STRAND_MASK = 0xFF, RK_DEDUP_DISTINCT = 0x100 };
typedef struct rk_policy {
    int32_t fold;                /* U1 */
    int32_t drop_last_window;    /* U3: 1 => len-k windows */
    int32_t counter_counts_zero; /* U12 */
    int32_t mask_strict_less;    /* U9 */
    int32_t freq_max_inclusive;  /* U10 */
    uint32_t seed;               /* 42, src/rkmh.cpp:497 */
    int32_t canon;               /* U2: RK_CANON_MINHASH = both strands are hashed, the smaller hash is kept; RK_CANON_LEXMIN = only the
                                    strand that is the smaller upper-case string (A < C < G < T) is hashed; a palindrome is its own.
                                    U6, bit 8 (RK_DEDUP_DISTINCT): a sketch holds the S smallest DISTINCT non-zero hashes and
                                    intersections are set intersections (Mash, sourmash); clear = mkmh's multiset.  Read the word
                                    through rk_policy_strand / rk_policy_dedup. */
} rk_policy;
int rk_policy_strand(const rk_policy* p); /* the strand rule: RK_CANON_MINHASH / RK_CANON_LEXMIN */
int rk_policy_dedup(const rk_policy* p);  /* the sketch rule: 0 = multiset, 1 = distinct */
void rk_default_policy(rk_policy* p);
/* The policy as text -- what `--hash-policy` / RKMH_POLICY of bin/rkmh and rkmh_amd.cli take and what a sketch file records
 * ("hashPolicy", next to the hashType / hashSeed keys of src/rkmh.cpp:493-497).  spec = comma-separated items applied left to
 * right onto *p (initialise it first, e.g. rk_default_policy): a preset -- `default`, or `mash`: the first 64 bits of
 * MurmurHash3_x64_128 over all len-k+1 windows, seed 42 (the strand rule stays: the smaller of the two strand hashes), or
 * `sourmash` = mash,canon=lexmin,dedup=distinct -- or key=value:
 * fold=swap32|h1|w2w1 (U1), windows=len-k|len-k+1 (U3), zero=count|skip (U12), mask=lt|le (U9), freqmax=incl|excl (U10),
 * canon=minhash|lexmin (U2; lexmin = the strand rule of Mash and sourmash), dedup=multiset|distinct (U6; distinct = the sketch
 * rule of Mash and sourmash; `default` and `mash` leave it alone), seed=<n>.
 * rk_policy_describe writes the canonical text with every key spelled out, canon= only when it is not minhash and, behind it,
 * dedup= only when it is distinct (returns its length or a negative error).
 * rk_policy_same_hashes: 1 when two policies give the same hash values and sketches (fold, window rule, canon, dedup, seed). */
int rk_policy_parse(const char* spec, rk_policy* p);
int rk_policy_describe(const rk_policy* p, char* dst, size_t cap);
int rk_policy_same_hashes(const rk_policy* a, const rk_policy* b);

typedef struct rk_ctx rk_ctx;
typedef struct rk_counter rk_counter;

const char* rk_last_error(void);
const char* rk_version(void);
int rk_device_count(void);
/* Compute units, peak engine clock (kHz), L2 bytes (one XCD's) and HBM bytes of a device (hipGetDeviceProperties); any
 * out pointer may be NULL.  Used by bench.py to turn instruction counts into issue-slot fractions on the actual part. */
int rk_device_props(int device, int32_t* compute_units, int32_t* clock_khz, int64_t* l2_bytes, int64_t* hbm_bytes);

/* One context = one GPU (one process per GPU in multi-GPU runs). policy may be NULL (defaults). */
int rk_ctx_create(int device, const rk_policy* policy, rk_ctx** out);
int rk_ctx_policy(const rk_ctx* ctx, rk_policy* out); /* the policy the context was created with */
void rk_ctx_destroy(rk_ctx* ctx);
int rk_ctx_synchronize(rk_ctx* ctx);
/* The context's own non-blocking hipStream_t (what the host-buffer entry points enqueue on). */
void* rk_ctx_stream(rk_ctx* ctx);
void rk_free(void* p);
/* Page-locked host memory (hipHostMalloc).  rk_classify_batch / rk_count_batch read page-locked `bases` by DMA where they lie and
 * write page-locked `out4` in place -- no staging copy on either side (the reference has no analogue: its reads never leave the
 * host, src/rkmh.cpp:845-898); pageable buffers keep working through the library's own pinned staging buffers. */
int rk_host_alloc(size_t bytes, void** out);
void rk_host_free(void* p);
/* Device memory on the context's GPU, for callers that keep arrays resident between calls of the *_device entries and have no HIP
 * runtime of their own (`rkmh gather` uploads its references once).  The copies run on the context's stream and return when done. */
int rk_device_alloc(rk_ctx* ctx, size_t bytes, void** out);
void rk_device_free(rk_ctx* ctx, void* p);
int rk_device_upload(rk_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int rk_device_download(rk_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ------------------------------------------------------------------------------------------------
 * INNER boundary: one-sequence mirrors of the mkmh calls (replaces, file:line of the call site):
 * ---------------------------------------------------------------------------------------------- */
/* mkmh::to_upper(char*, int)                         src/rkmh.cpp:227,818,856,908 */
int rk_to_upper(rk_ctx* ctx, char* seq, int len);
/* mkmh::calc_hashes(const char*, int, vector<int>&, hash_t*&, int&)   src/rkmh.cpp:821,860,2101 */
int rk_calc_hashes(rk_ctx* ctx, const char* seq, int len, const int* ks, int nks, uint64_t** out, int* n);
/* 6-arg form with HASHTCounter*                      src/rkmh.cpp:831,909,1611,1616 */
int rk_calc_hashes_counted(rk_ctx* ctx, const char* seq, int len, const int* ks, int nks,
                           uint64_t** out, int* n, rk_counter* counter);
/* mkmh::calc_hash(string)                            src/rkmh.cpp:1811,1852,2198 */
int rk_calc_hash(rk_ctx* ctx, const char* kmer, int k, uint64_t* out);
/* mkmh::minhashes(hash_t*, int, int, hash_t*&, int&) src/rkmh.cpp:822,863,917 (sorts h in place) */
int rk_minhashes(rk_ctx* ctx, uint64_t* h, int n, int sketch_size, uint64_t** mins, int* m);
/* mkmh::mask_by_frequency(hash_t*, int, HASHTCounter*, int)  src/rkmh.cpp:916 */
int rk_mask_by_frequency(rk_ctx* ctx, uint64_t* h, int n, const rk_counter* counter, int min_occ);
/* mkmh::minhashes_frequency_filter(...)              src/rkmh.cpp:835-836 */
int rk_minhashes_frequency_filter(rk_ctx* ctx, uint64_t* h, int n, int sketch_size, uint64_t** out, int* m,
                                  const rk_counter* counter, int min_count, int max_count);
/* mkmh::hash_intersection_size(const hash_t*, int, const hash_t*, int, int&)  src/rkmh.cpp:869,922 */
int rk_hash_intersection_size(rk_ctx* ctx, const uint64_t* a, int na, const uint64_t* b, int nb, int* out);
/* mkmh::hash_intersection(hash_t*, int start, int len, hash_t*, int start, int len, int sketch_size) -> tuple<hash_t*, int>
 * as called from src/equiv.hpp:308,340,364 (the comment at equiv.hpp:303-305 names the arguments (ptr, len, start); the CALLS
 * pass (ptr, start, len) and that order is kept).  The matching hashes of a[a_start, a_start+a_len) and b[...], ascending,
 * both sides advancing on equality as in rk_hash_intersection_size, at most sketch_size of them.  *out is allocated by
 * the callee (the reference's callers delete[] it, equiv.hpp:317,349); release it with rk_free. */
int rk_hash_intersection(rk_ctx* ctx, const uint64_t* a, int a_start, int a_len, const uint64_t* b, int b_start, int b_len,
                         int sketch_size, uint64_t** out, int* n);

/* HASHTCounter (ctor src/rkmh.cpp:739,742,1187; increment :335; get :1218,1260): int32 slots in HBM,
 * slot = key % slots.  rk_counter_wrap adopts caller-owned DEVICE memory (e.g. a torch tensor, so
 * that the table can be all-reduced over RCCL between pass 1 and pass 2 of the -M path).  The library orders ITS passes into a
 * table among themselves; work the CALLER has in flight on the memory (a fill on torch's stream, a collective) must have
 * finished -- or be on the stream given to the pass -- before a pass is started: the passes run on the context's or the given
 * stream, not on the caller's. */
int rk_counter_create(rk_ctx* ctx, uint64_t slots, rk_counter** out);
int rk_counter_wrap(rk_ctx* ctx, void* d_counts_int32, uint64_t slots, rk_counter** out);
void rk_counter_destroy(rk_counter* c);   /* allowed after rk_ctx_destroy of its context; every other call is not */
int rk_counter_clear(rk_counter* c);
/* dst += src and dst = src, element-wise, for two tables of equal size that may belong to contexts on DIFFERENT devices: the
 * reduce / broadcast of a -M run that spreads its reads over several GPUs inside one process (bin/rkmh --devices).  The
 * reference's OpenMP threads share one HASHTCounter (src/rkmh.cpp:739, :909); one table per device summed after pass 1 gives the
 * same counts.  Both calls synchronise the two contexts' streams. */
int rk_counter_add(rk_counter* dst, const rk_counter* src);
int rk_counter_copy(rk_counter* dst, const rk_counter* src);
int rk_counter_increment(rk_counter* c, uint64_t key);
int rk_counter_get(const rk_counter* c, uint64_t key, int32_t* out);
/* Counter (de)serialisation (what the reference's commented-out read_hash_counter.write_to_binary / deserialize would do,
 * src/rkmh.cpp:744-769, :911-913; docs/todo.md:1).  File = "RKHT2\n", u64 slots, u64 nnz, u32 tag_len, tag, then
 * nnz x (u32 slot, i32 count), little endian ("RKHT1\n" files of round 1, without the tag field, load as untagged).
 * rk_counter_load* require a counter with the same number of slots and REPLACE its contents.  A file saved with a
 * provenance tag only loads through rk_counter_load_tagged with the identical tag (RK_ERR_ARG otherwise); an untagged
 * file only loads through rk_counter_load. */
int rk_counter_save(rk_counter* c, const char* path);
int rk_counter_load(rk_counter* c, const char* path);
int rk_counter_save_tagged(rk_counter* c, const char* path, const void* tag, uint32_t tag_len);
int rk_counter_load_tagged(rk_counter* c, const char* path, const void* tag, uint32_t tag_len);
/* Provenance tag of a READ depth map (pass 1 of -M, src/rkmh.cpp:904-910): k list, seed, fold, window and zero-counting
 * policy of the context, and a fingerprint of the read set (count, total bases, hashes of the lengths and of up to
 * 2 MiB of bases).  Host-side. */
#define RK_DEPTH_TAG_BYTES 128
int rk_depth_map_tag(const rk_ctx* ctx, const int* ks, int nks, const uint8_t* bases, const uint64_t* offsets,
                     int64_t nseq, uint8_t tag[RK_DEPTH_TAG_BYTES]);
void* rk_counter_device_ptr(rk_counter* c);
uint64_t rk_counter_slots(const rk_counter* c);
/* Compact depth map for -M runs that need min_num only up to bound 0 (rk_set_min_num_bound(ctx, 0): `stream` without -N,
 * `filter` with -D >= 0).  mask_by_frequency (src/rkmh.cpp:916) then changes a read's row only through windows whose hash is a
 * sketch hash, and whether such a hash survives depends on ONE slot of the HASHTCounter, hash % slots -- so only the slots that
 * some key of the reference index maps to are counted: rk_counter_entries() int32 instead of `slots` (a few hundred KB instead of
 * the 800 MB of rkmh.cpp:739), counted EXACTLY (every window of every read is still hashed; collisions into a tracked slot count,
 * as in the full table).  Laid out from the references of `ctx` at this call (create it after rk_set_references; it is refused
 * once the references change).  d_counts_int32: NULL (the library allocates and zeroes) or caller-owned, ZEROED device memory of
 * rk_counter_compact_entries() int32 (e.g. a torch tensor to all-reduce between the passes).
 * Serves rk_count_batch / rk_count_batch_device / rk_fastq_slot_count, rk_counter_clear / _add / _copy / _get (of index keys) and
 * rk_set_depth_filter.  Any batch holding a read with more hashes than the sketch keeps is refused with RK_ERR_NEED_FULL before
 * anything is counted (bottom-s selection depends on the depth of every hash): the caller repeats the pass with a full table. */
int rk_counter_create_compact(rk_ctx* ctx, uint64_t slots, void* d_counts_int32, rk_counter** out);
int rk_counter_compact_entries(const rk_ctx* ctx, uint64_t slots, uint64_t* entries);
uint64_t rk_counter_entries(const rk_counter* c); /* int32 entries behind rk_counter_device_ptr (= slots for a full table) */
int rk_counter_is_compact(const rk_counter* c);

/* ------------------------------------------------------------------------------------------------
 * OUTER boundary: batched replacements of main_stream's loops.
 * Sequences are concatenated ASCII bytes (any case; upper-casing happens on the device, as
 * src/rkmh.cpp:856 does per read) + offsets[n+1] (offsets[i]..offsets[i+1] = sequence i).
 * ---------------------------------------------------------------------------------------------- */

/* calc_hashes for a batch (hash sub-command, src/rkmh.cpp:2097-2104).  hash_offsets[n+1] (caller
 * array) receives the per-sequence segment bounds; *out is malloc'd [hash_offsets[n]] (rk_free). */
int rk_hash_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nseq,
                  const int* ks, int nks, uint64_t** out, uint64_t* hash_offsets);

/* calc_hashes + minhashes for a batch (src/rkmh.cpp:816-826 for refs, :860-863 for reads).
 * sketches: caller [nseq * sketch_size] (zero padded), lens: caller [nseq]. */
int rk_sketch_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nseq,
                    const int* ks, int nks, int sketch_size, uint64_t* sketches, int32_t* lens);

/* Reference side of main_stream (src/rkmh.cpp:783-785 + :816-826): sketch every reference on the
 * GPU and build the resident lookup index.  max_samples < 0 => plain path; >= 0 => the -I path
 * (src/rkmh.cpp:828-838) with a counter of counter_slots (0 => 200000000, src/rkmh.cpp:742). */
int rk_set_references(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int nref,
                      const int* ks, int nks, int sketch_size, int max_samples, uint64_t counter_slots);
/* How the -I counter is filled by the next rk_set_references: 0 = once per k-mer occurrence (main_stream,
 * src/rkmh.cpp:831), 1 = once per distinct hash per reference (main_filter's hash_sequences, src/rkmh.cpp:348-355). */
int rk_set_reference_count_mode(rk_ctx* ctx, int mode);
/* Import already-built sketches (after an RCCL broadcast from the rank that sketched them). */
int rk_set_reference_sketches(rk_ctx* ctx, const uint64_t* sketches, const int32_t* lens, int nref,
                              const int* ks, int nks, int sketch_size);
/* Export: sketches [nref*sketch_size], lens [nref] (caller arrays). */
int rk_get_reference_sketches(rk_ctx* ctx, uint64_t* sketches, int32_t* lens);
int rk_num_references(const rk_ctx* ctx);

/* Which form of the fused kernel plain classification (no -M) will use for the references now set: returns 1 when the
 * k-mer-space form is active (single k from 8 to 16: the 4^k k-mer universe was enumerated and every k-mer whose canonical hash
 * is a sketch hash -- or 0 -- is known, so windows are filtered and resolved by k-mer and never hashed), 0 for the hash-space
 * form, negative on error.  *kmers_found (may be NULL) = k-mers the enumeration found (one per strand pair). */
int rk_kmer_form(const rk_ctx* ctx, uint32_t* kmers_found);
/* Whether the NEXT rk_set_references / rk_set_reference_sketches may build the k-mer-space form (default 1).  A caller that only
 * uses the general kernels on these references (hpv16's rk_classify_groups_batch) saves the enumeration by passing 0. */
int rk_set_kmer_form(rk_ctx* ctx, int enable);
/* The k-mer-space form rests on an enumeration of the whole 4^k k-mer universe (every k-mer whose canonical hash is an index key:
 * 26 ms at k = 16 on MI355X, 4 x per further base) -- a function of the index keys, k, fold and seed alone.  With a cache file set,
 * the NEXT rk_set_references / rk_set_reference_sketches loads the lists from it when its tag (a hash of exactly those inputs)
 * matches and skips the enumeration; otherwise it enumerates -- k = 19 and 20 (1.7 s, 6.7 s) included, which without a cache file
 * are left to the hash-space kernel -- and (re)writes the file.  A stale or foreign file is never used.
 * path NULL or "": no cache.  rk_kmer_cache_state: of the last index build -- 0 none, 1 loaded, 2 enumerated and written, 3
 * enumerated (the file could not be written). */
int rk_set_kmer_cache(rk_ctx* ctx, const char* path);
int rk_kmer_cache_state(const rk_ctx* ctx);

/* What the index of this context was built as (host only, read only: counters that the last index build filled as it went).
 * Every key of the index (a distinct sketch hash) takes one of several value forms, chosen by thresholds that the kernels decode
 * again on their side ("Index value forms"); these counters say which form each key took, so a test can build a key
 * at a threshold and prove on which side it fell.
 *   hash-space index   keys, buckets; buckets_overflowed = buckets whose overflow flag is set; longest_chain = the largest number
 *                      of buckets a stored key lies past its home bucket, plus one (1: every key is at home); chain_wrapped = 1
 *                      when some key was stored in a lower-numbered bucket than its home (the chain ran past the last bucket)
 *   values, per key    single_once (one reference, multiplicity 1), single_multi (one reference, 2 .. 511), pair (two references
 *                      below 2048 once each, 11 + 11 bits), list (a posting list: everything else); list_longest = entries of the
 *                      longest list, post_words = 32-bit words of the posting array
 *   k-mer-space form   all zero when it is not built (rk_kmer_form returns 0).  kmer_form = 1; bases_kept = base lists in use;
 *                      bases_dropped_by_share_rule = 1 when bases were chosen and the 5 % rule cleared them; per key found by the
 *                      enumeration, as the value table classifies it: kv_reference (the value id is the reference), kv_single_multi,
 *                      kv_pair, kv_inline_list (3 .. 6 references below 512 once each, tag 11), kv_base_inline (base and up to eight
 *                      exceptions in the value, tag 111), kv_base_list (a (base, exceptions) list in the posting array),
 *                      kv_plain_list; per k-mer size of the run, in the order given: km1_bits (log2 of the exact map's buckets),
 *                      km1_longest_hop (buckets past its own of the farthest cell), kf4_sectors, found (k-mers enumerated)
 * The caller sets out->struct_size = sizeof(rk_index_stats_t) as it was compiled; at most that many bytes are written, and
 * struct_size comes back as the number written (the structure may grow at its end).  RK_ERR_STATE before any references are set. */
typedef struct rk_index_stats_t {
    uint32_t struct_size;
    uint32_t keys, buckets, buckets_overflowed, longest_chain, chain_wrapped;
    uint32_t single_once, single_multi, pair, list, list_longest, post_words;
    uint32_t kmer_form, bases_kept, bases_dropped_by_share_rule;
    uint32_t kv_reference, kv_single_multi, kv_pair, kv_inline_list, kv_base_inline, kv_base_list, kv_plain_list;
    uint32_t km1_bits[RK_MAX_KS], km1_longest_hop[RK_MAX_KS], kf4_sectors[RK_MAX_KS], found[RK_MAX_KS];
} rk_index_stats_t;
int rk_index_stats(const rk_ctx* ctx, rk_index_stats_t* out);

/* Read-depth filter (-M, src/rkmh.cpp:701-704): when set, classify masks hashes whose counter
 * value is below min_kmer_occ (mask_by_frequency, :916) before sketching.  NULL disables.
 * The table is read as it is AT THIS CALL (the fused kernel uses a one-bit-per-slot snapshot of the comparison): set the
 * filter after pass 1 (rk_count_batch*, and after any all-reduce of the table), and again if the table changes later. */
int rk_set_depth_filter(rk_ctx* ctx, rk_counter* counter, int min_kmer_occ);
/* How much of min_num (row field 3) the caller needs while a depth filter is set.  The reference uses num_mins in ONE predicate,
 * `depth_filter = num_mins <= min_matches` (src/rkmh.cpp:938; filter: `read_min_lens[i] <= 0`, :1292), so a caller that compares
 * with n needs min(num_mins, n + 1) and nothing more.  bound < 0 (default): row field 3 is num_mins exactly -- every window is
 * looked up in the depth map.  bound >= 0: row field 3 = min(num_mins, bound); max_id / max_shared / diff are unchanged (the mask
 * changes them only through windows whose hash is a sketch hash: one keep bit per index key, taken when the filter is set), and
 * only the first windows of a read -- until `bound` of them survive -- are looked up by slot.  bound 0 looks up none.
 * May be called before or after rk_set_depth_filter (the snapshot is rebuilt in the other form). */
int rk_set_min_num_bound(rk_ctx* ctx, int bound);
int rk_min_num_bound(const rk_ctx* ctx);

/* Pass 1 of the -M path (src/rkmh.cpp:904-910): hash every read and increment the counter.
 * Passes into ONE counter are ordered by the library (each waits on its stream for the previous one: large batches add their
 * counts with plain stores, not atomics), whatever streams they are given; rk_counter_get / _clear / _add / _copy / _save /
 * _increment and rk_set_depth_filter wait for the passes enqueued so far.  A caller that reads the table through
 * rk_counter_device_ptr() synchronises with the pass's stream itself, as before. */
int rk_count_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, rk_counter* counter);
int rk_count_batch_device(rk_ctx* ctx, const void* d_bases, const void* d_offsets_u32, int64_t nreads,
                          rk_counter* counter, void* hip_stream);

/* The per-read hot loop (src/rkmh.cpp:845-898 / :911-948) for a batch of reads in HOST memory:
 * to_upper -> calc_hashes -> minhashes -> hash_intersection_size vs every reference -> argmax/diff.
 * out4[i*4+0..3] = max_id, max_shared, diff, min_num  (exactly the variables of :874-888).
 * Staged through pinned buffers with hipMemcpyAsync overlapped with the kernels. */
int rk_classify_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int32_t* out4);

/* Same, inputs already resident in HBM (the measured configuration).  d_bases: 4-byte aligned, readable
 * up to the next multiple of 4 past the last base; d_offsets_u32: uint32 [nreads+1] byte offsets into
 * d_bases; d_out4: int32 [nreads*4].  max_read_len: upper bound of the read lengths in the batch (sizes the
 * per-wave LDS image; 0 => determined by a device reduction, which costs one stream sync).
 * hip_stream: the hipStream_t to enqueue on (NULL = HIP's null stream; rk_ctx_stream() = the context's own).
 * Asynchronous: returns after enqueueing.
 * Reads the fused kernel cannot take (longer than 1528 bases, more than 16384 references, or more non-zero hashes than the sketch
 * size) come back with max_id = -2; rk_classify_batch reroutes those itself. */
int rk_classify_batch_device(rk_ctx* ctx, const void* d_bases, const void* d_offsets_u32, int64_t nreads,
                             void* d_out4, uint32_t max_read_len, void* hip_stream);
/* As above, but rows the fused kernel cannot answer (long reads, reads with more windows than the sketch keeps) are
 * answered by the general kernels on the resident bases instead of being flagged; synchronises hip_stream. */
int rk_classify_batch_device_all(rk_ctx* ctx, const void* d_bases, const void* d_offsets_u32, int64_t nreads,
                                 void* d_out4, uint32_t max_read_len, void* hip_stream);

/* hpv16's per-read loop (main_hpv16, src/rkmh.cpp:2656-2719).  The references set with rk_set_reference_sketches are hash
 * LISTS here, not bottom-s sketches: first the argmax_refs HPV type references (all hashes of each, :2546-2547), then the
 * lineage- and sublineage-specific k-mer sets (:2568-2650); sketch_size = the longest list.  Per read: calc_hashes (all -k),
 * mask_by_frequency when a depth filter is set (:2663), sort (:2666); out4 = (max_id, max_shared, diff, non-zero hashes) over
 * the first argmax_refs references with the strict-> first-max rule of :2675-2678; tail_counts[i][nref - argmax_refs] = the
 * intersection size against each remaining reference (what sort_by_similarity ranks, :2688, :2700).  With reference lists
 * of DISTINCT values the intersection is the number of distinct non-zero read hashes present in the list
 * (hash_set_intersection_size; absent from /root/reference, policy U13 of DESIGN.md).  No bottom-s: a read with more hashes
 * than sketch_size is refused (RK_ERR_LIMIT).  Host buffers; runs the general kernels (k_hash_tiles + k_sort_intersect). */
int rk_classify_groups_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nreads, int argmax_refs,
                             int32_t* out4, int32_t* tail_counts);

/* ------------------------------------------------------------------------------------------------
 * `call` (main_call, src/rkmh.cpp:1455-1904): k-mer depth map of the reads, sliding-window mean depth along the
 * references (window NOT reset between references, as a single-threaded run of src/rkmh.cpp:1769-1791), and at
 * every position whose depth is below half that mean the 3k SNP and k one-base-deletion k-mers are hashed and
 * looked up; every candidate passing the tests of :1814 / :1853 comes back as one record (rk_free the array).
 * The caller aggregates records into VCF rows (KC/MD/RD/OD, :1821-1829) -- see rkmh_main.cpp. */
typedef struct rk_call_record {
    int32_t ref;        /* reference index */
    int32_t pos;        /* j + alt_pos + 1 (src/rkmh.cpp:1815, :1855) */
    int32_t alt_depth;  /* depth of the rescue k-mer */
    int32_t avg_d;      /* truncated window mean at the position */
    int32_t depth;      /* depth of the original k-mer */
    uint8_t orig, alt;  /* reference base, alternative base ('-' for a deletion) */
    uint8_t kind;       /* 0 SNP, 1 deletion */
    uint8_t pad;
} rk_call_record;
int rk_call(rk_ctx* ctx, const uint8_t* ref_bases, const uint64_t* ref_offsets, int nref,
            const uint8_t* read_bases, const uint64_t* read_offsets, int64_t nreads, int k, int window_len,
            rk_call_record** out, int64_t* nout);

/* Formats one stdout line of stream/classify exactly as src/rkmh.cpp:887-893. Returns bytes written
 * (excluding NUL) or a negative error if cap is too small. */
int rk_format_stream_line(char* dst, size_t cap, const char* ref_name, const char* read_name,
                          int max_shared, int diff, int min_num, int sketch_size, int min_matches, int min_diff);

/* ------------------------------------------------------------------------------------------------
 * FASTA/FASTQ(.gz) front end (parse_fastas, src/rkmh.cpp:238-292; grammar src/kseq.hpp:170-208).
 * Host-side; fills malloc'd concatenated buffers (rk_free each).  names/quals are NUL-separated.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rk_seqset {
    int64_t nseq;
    uint8_t* bases;      /* concatenated, NOT upper-cased here (device does it) */
    uint64_t* offsets;   /* [nseq+1] */
    char* names;         /* name_0 \0 name_1 \0 ... */
    uint64_t* name_offsets; /* [nseq+1] */
    char* quals;         /* concatenated (same offsets as bases) or NULL when any record lacks quals */
} rk_seqset;
int rk_parse_files(const char* const* paths, int npaths, rk_seqset* out);
void rk_seqset_free(rk_seqset* s);
/* rk_seqset_free parks large batch buffers (up to 1.5 GB in all) for the next batch instead of returning them to the system;
 * this releases whatever is parked (a long-lived process that has finished parsing) */
void rk_pool_trim(void);
/* Streaming form (the build's replacement of KSEQ_Reader::get_next_buffer, src/rkmh.cpp:951-959, 2085-2094):
 * up to max_records records / max_bases bases per call (0 = unlimited); out->nseq == 0 at end of input.
 * path "-" reads STDIN.  Uncompressed input read with max_records == 0 or >= 65536 goes through the
 * block-parallel scanner (RKMH_PARSE_THREADS, default 8): a batch is then a whole block of about
 * max_records records, so both limits are approximate there; any input that is not strictly
 * line-structured falls back to the sequential kseq-grammar scanner with identical results. */
typedef struct rk_reader rk_reader;
int rk_reader_open(const char* path, rk_reader** out);
/* the same reader, starting `offset` bytes into the file at a record start (how a file is handed from the device-side FASTQ front
 * end, rk_fastq_slot_*, to this scanner at the first block the device refuses) */
int rk_reader_open_at(const char* path, uint64_t offset, rk_reader** out);
/* the records that START in bytes [lo, hi) of a regular uncompressed FASTQ file (how the ranks of a multi-process run each read
 * their own part of the reads); valid only while rk_reader_strict() stays 1 -- see rk_parse.cpp */
int rk_reader_open_range(const char* path, uint64_t lo, uint64_t hi, rk_reader** out);
int rk_reader_strict(const rk_reader* r);
#define RK_READER_NO_QUALS 1 /* do not keep quality strings (stream/classify never read them) */
void rk_reader_set_options(rk_reader* r, int flags);
int rk_reader_next(rk_reader* r, int64_t max_records, uint64_t max_bases, rk_seqset* out);
void rk_reader_close(rk_reader* r);

/* Synthetic-workload generator of the measured configuration: reads [lo,hi) of the
 * global read set drawn from the reference panel with 1 % substitutions, strand flips and 1-in-1000 'N'.
 * Host-side utility for bench.py and the tests; out holds (hi-lo)*read_len bytes. */
int rk_synth_reads(const uint8_t* ref_bases, const uint64_t* ref_offsets, int nref, uint64_t lo, uint64_t hi,
                   int read_len, uint64_t seed, uint8_t* out, int threads);

/* ------------------------------------------------------------------------------------------------
 * FASTQ text parsed ON THE DEVICE: a block of raw FASTQ text (as it lies in the file, starting at a record start and ending after
 * a record's last newline) is uploaded, split into records, checked, packed and classified by the GPU (rk_fastq.hip) -- the
 * device-side replacement of the host loop  parse_fastas -> kseq_read  (src/rkmh.cpp:238-263; grammar src/kseq.hpp:170-208)
 * followed by the per-read loop (src/rkmh.cpp:845-898), for text that is strictly four lines per record.  For any other text
 * (multi-line sequences, blank lines, carriage returns, '>' / '+' / '@' inside a sequence, a quality string of another length,
 * ...) the call reports status != 0 and leaves the block to the kseq-grammar scanner (rk_reader_* / rk_parse_*): it never guesses.
 * One slot = one block in flight (own stream, page-locked text buffer); several slots of a context may be used from several threads.
 * ---------------------------------------------------------------------------------------------- */
typedef struct rk_fastq_slot rk_fastq_slot;
typedef struct rk_fastq_result {
    int32_t status;            /* 0: the fields below are valid; != 0 (RK_FASTQ_* bits): parse this block on the host instead */
    int64_t nrec;              /* records of the block */
    const int32_t* out4;       /* [nrec][4] rows (max_id, max_shared, diff, min_num) as rk_classify_batch writes them */
    const uint32_t* name_off;  /* name of record i = text[name_off[i] .. name_off[i] + name_len[i])  (header up to the first whitespace) */
    const uint32_t* name_len;
    const uint32_t* seq_off;   /* its sequence = text[seq_off[i] .. + seq_len[i]) */
    const uint32_t* seq_len;
    const uint32_t* qual_off;  /* its quality string = text[qual_off[i] .. + seq_len[i]) */
} rk_fastq_result;             /* the arrays live in the slot and are overwritten by its next call */
#define RK_FASTQ_CR 1          /* a carriage return somewhere in the block */
#define RK_FASTQ_LINES 2       /* lines do not come in fours / no final newline */
#define RK_FASTQ_RECORD 4      /* a record without '@' / '+' line starts, with an empty sequence or a quality string of another length */
#define RK_FASTQ_CHAR 8        /* a sequence byte kseq would not keep, or a quality byte outside 33..127 */
#define RK_FASTQ_CAP 16        /* more records than a block of this size is sized for (records of under 64 bytes on average) */
int rk_fastq_slot_create(rk_ctx* ctx, uint64_t max_bytes, rk_fastq_slot** out);
/* flags: RK_SLOT_DEVICE_TEXT = the block's text never visits the host.  Such a slot has no text buffer of its own (blocks come from
 * rk_fastq_slot_load_bgzf, or from caller memory named with rk_fastq_slot_set_source), may be hundreds of megabytes large at little
 * page-locked memory, and its finish() brings back -- besides the rows -- only the bytes the output needs, packed on the device:
 * the record NAMES (what stream / classify print, src/rkmh.cpp:887-892) or, after rk_fastq_slot_set_filter_output, name, sequence
 * and quality string of the records filter prints (src/rkmh.cpp:1292-1300).  The result's name_off / seq_off / qual_off then index
 * rk_fastq_slot_spans_base() -- which is what the formatters below are to be given as `text` for ANY slot. */
#define RK_SLOT_DEVICE_TEXT 1
int rk_fastq_slot_create2(rk_ctx* ctx, uint64_t max_bytes, int flags, rk_fastq_slot** out);
int rk_fastq_slot_set_filter_output(rk_fastq_slot* slot, int min_matches, int min_diff);
const uint8_t* rk_fastq_slot_spans_base(const rk_fastq_slot* slot);   /* of the last finished block; valid until the slot's next call */
uint8_t* rk_fastq_slot_text(rk_fastq_slot* slot);  /* page-locked buffer of max_bytes: the caller fills it with the block's text (NULL for a device-text slot) */
/* ... or names the text where it lies: the slot's NEXT block (submit / classify / count) is uploaded from `text` -- caller memory,
 * ideally page-locked (a mapping of the input file registered with hipHostRegister: the link reads the page cache, no copy), valid
 * and unchanged until that block's finish / count has returned.  The formatters are given the same pointer. */
int rk_fastq_slot_set_source(rk_fastq_slot* slot, const uint8_t* text);
int rk_host_register_readonly(const void* p, size_t bytes);   /* hipHostRegister of memory that is only read (a file mapping) */
void rk_host_unregister(const void* p);
int rk_fastq_slot_classify(rk_fastq_slot* slot, uint64_t nbytes, rk_fastq_result* res);
/* the same in two halves (classify = submit + finish): submit enqueues the upload and the splitting / checking / packing kernels and
 * returns at once, finish waits, classifies and collects -- a host thread with two slots reads its next block in between */
int rk_fastq_slot_submit(rk_fastq_slot* slot, uint64_t nbytes);
int rk_fastq_slot_finish(rk_fastq_slot* slot, rk_fastq_result* res);
/* pass 1 of -M (src/rkmh.cpp:904-910) on a block of raw text: every window's hash counted into `counter` (a table of the slot's
 * context); *status != 0: the block is not four lines per record and nothing of it was counted */
int rk_fastq_slot_count(rk_fastq_slot* slot, uint64_t nbytes, rk_counter* counter, int32_t* status, int64_t* nrec);

/* The output of stream / classify (line format src/rkmh.cpp:887-892) and of filter (records src/rkmh.cpp:1292-1300, decision
 * src/equiv.hpp:324-353) for one classified block, written from the names, sequences and quality strings where they lie in the
 * block's raw text (rk_fastq_slot_text).  rk_line_parts holds what does not depend on the read ("ref name \t" per reference, the
 * eight possible line tails).  dst must hold *_bound() bytes; the functions return the bytes written or a negative RK_ERR_*. */
typedef struct rk_line_parts rk_line_parts;
int rk_line_parts_create(const char* ref_names, const uint64_t* ref_name_offsets, int64_t nref, int sketch_size, int min_matches,
                         int min_diff, rk_line_parts** out);   /* names NUL-terminated, back to back, as in rk_seqset */
void rk_line_parts_destroy(rk_line_parts* parts);
uint64_t rk_fastq_stream_lines_bound(const rk_line_parts* parts, const rk_fastq_result* res);
int64_t rk_fastq_stream_lines(const rk_line_parts* parts, const rk_fastq_result* res, const uint8_t* text, char* dst, uint64_t cap);
uint64_t rk_fastq_filter_records_bound(const rk_fastq_result* res);
int64_t rk_fastq_filter_records(const rk_fastq_result* res, const uint8_t* text, int min_matches, int min_diff, char* dst, uint64_t cap);

/* ---- references from raw FASTA text (replaces parse_fastas over the -r files, src/rkmh.cpp:238-263 + :816-826, for regular text).
 * The text of the files, concatenated (a '\n' after each file), is uploaded block by block through a slot's page-locked buffer;
 * rk_fasta_load_finish strips header lines and line ends ON THE DEVICE and returns the record table; rk_set_references_fasta
 * sketches the packed bases where they lie.  status != 0 (RK_FASTA_* bits): the text is not plain line-structured FASTA (carriage
 * returns, '>', '+' or '@' inside sequence lines, bases before the first header, bytes outside 33..126) -- parse it on the host. */
typedef struct rk_fasta_load rk_fasta_load;
typedef struct rk_fasta_index {
    int32_t status;
    int64_t nseq;
    const uint64_t* offsets;       /* [nseq + 1] sequence i = packed bases [offsets[i], offsets[i+1]) (on the device) */
    const char* names;             /* NUL-terminated names (header line up to the first whitespace), back to back */
    const uint64_t* name_offsets;  /* [nseq + 1] */
} rk_fasta_index;                  /* the arrays belong to the rk_fasta_load */
#define RK_FASTA_BAD_CHAR 1
#define RK_FASTA_BAD_NAME 2
#define RK_FASTA_BAD_LEAD 4
#define RK_FASTA_EMPTY 8
int rk_fasta_load_create(rk_ctx* ctx, uint64_t text_bytes, rk_fasta_load** out);
int rk_fasta_load_put(rk_fasta_load* load, rk_fastq_slot* via, uint64_t text_offset, uint64_t nbytes);
int rk_fasta_load_finish(rk_fasta_load* load, uint64_t total_bytes, rk_fasta_index* out);
struct rk_gzip;
/* the text of an ordinary gzip file (rk_gzip_open) inflated on the device into the load's text at text_offset; 1: parse on the host instead */
int rk_fasta_load_put_gzip(rk_fasta_load* load, struct rk_gzip* gz, uint64_t text_offset, uint64_t* text_bytes);
/* ... and of members [b0, b1) of a BGZF file (a bgzip'd genome), inflated in the buffers of `via` (RK_SLOT_DEVICE_TEXT); 1: parse on the host */
struct rk_bgzf;
int rk_fasta_load_put_bgzf(rk_fasta_load* load, rk_fastq_slot* via, const struct rk_bgzf* z, int64_t b0, int64_t b1, uint64_t text_offset);
int rk_fasta_load_put_newline(rk_fasta_load* load, uint64_t text_offset);   /* the separator behind such a file */
int rk_fasta_load_get_bases(rk_fasta_load* load, uint8_t* dst);   /* the packed bases, offsets[nseq] bytes, to the host */
int rk_set_references_fasta(rk_ctx* ctx, rk_fasta_load* load, const int* ks, int nks, int sketch_size, int max_samples, uint64_t counter_slots);
void rk_fasta_load_destroy(rk_fasta_load* load);
void rk_fastq_slot_destroy(rk_fastq_slot* slot);
/* Where to cut: the offset of the LAST record start in text[1 .. n) under the four-line rule (a line that begins with '@' whose
 * second line below begins with '+'), or -1 when there is none: text[0 .. offset) then holds whole records only. */
int64_t rk_fastq_cut(const uint8_t* text, uint64_t n);

/* BGZF (bgzip) FASTQ files for the device front end.  The reference opens every input through gzFile (src/rkmh.cpp:238-263): one
 * sequential inflater.  A BGZF file is a chain of independent gzip members (<= 64 KB of text each) whose headers give their
 * lengths, so any number of threads can each inflate the members of their own block of the file.  rk_bgzf_open: RK_ERR_ARG = not a
 * BGZF file (plain gzip, plain text: take another path).  rk_bgzf_plan groups consecutive members into jobs of about target_bytes
 * of text (first[j] .. first[j + 1]); rk_bgzf_fastq_records inflates one job and copies the whole FASTQ records that START in it
 * (four-line rule at both ends, as rk_fastq_cut) to dst, ready for rk_fastq_slot_submit; it returns 1 when the text does not
 * begin with '@'.  Thread-safe on one rk_bgzf. */
typedef struct rk_bgzf rk_bgzf;
int rk_bgzf_open(const char* path, rk_bgzf** out);
void rk_bgzf_close(rk_bgzf* z);
int64_t rk_bgzf_members(const rk_bgzf* z);
uint64_t rk_bgzf_text_bytes(const rk_bgzf* z);
uint64_t rk_bgzf_text_offset(const rk_bgzf* z, int64_t member);
const char* rk_bgzf_inflater(void); /* "libdeflate" (where it can be loaded and RKMH_NO_LIBDEFLATE is unset) or "zlib": what rk_bgzf_fastq_records inflates with */
int rk_bgzf_first_byte(const rk_bgzf* z);
int64_t rk_bgzf_plan(const rk_bgzf* z, uint64_t target_bytes, int64_t* first, int64_t cap);
int64_t rk_bgzf_plan_members(const rk_bgzf* z, uint64_t target_bytes, int64_t max_members, int64_t* first, int64_t cap);   /* ... and of at most max_members members each */
int rk_bgzf_fastq_records(const rk_bgzf* z, int64_t b0, int64_t b1, uint8_t* dst, uint64_t cap, uint64_t* nbytes, uint64_t* text_off);
const uint8_t* rk_bgzf_image(const rk_bgzf* z);   /* the mapped file */
/* the member whose text ends with the byte in front of member b0's text (b0 - 1 unless that one is empty; b0 when no text precedes) */
int64_t rk_bgzf_lead_member(const rk_bgzf* z, int64_t b0);
int rk_bgzf_member(const rk_bgzf* z, int64_t member, uint64_t* file_off, uint32_t* total_bytes, uint32_t* header_bytes, uint32_t* text_bytes);
/* The same job inflated ON THE DEVICE (rk_inflate.hip: a lane per member decodes, a wave per member resolves the matches in LDS,
 * another checks the member's CRC-32 -- as gzread does for everything the reference reads, src/rkmh.cpp:238-263): the compressed
 * bytes cross the link instead of the text (by DMA straight from the mapped file when the caller page-locked it:
 * rk_host_register_readonly(rk_bgzf_image(z), rk_bgzf_file_bytes(z))), the records that start in members [b0, b1) land in the slot's
 * device text buffer -- and, for a slot without RK_SLOT_DEVICE_TEXT, a copy of them in rk_fastq_slot_text().  The NEXT
 * rk_fastq_slot_submit / _classify / _count of the slot is given *nbytes and skips its upload.  A job may hold tens of thousands
 * of members (one launch decodes them all: the decode kernel takes the same ~15 ms for 64 members as for 32 768).
 * Returns RK_OK, or 1: take the host route (rk_bgzf_fastq_records) for this job -- it reports damaged members. */
int rk_fastq_slot_load_bgzf(rk_fastq_slot* slot, const rk_bgzf* z, int64_t b0, int64_t b1, uint64_t* nbytes, uint64_t* text_off);

/* ---- ordinary gzip files (ONE deflate stream) inflated on the device: rk_gunzip.hip ------------------------------------------
 * The reference reads every input through gzopen / gzread (/root/reference/src/rkmh.cpp:238-263).  rk_gzip_open maps a gzip file
 * that is not BGZF (RFC 1952 header, deflate payload, trailer); rk_gzip_plan(slot_bytes) cuts its compressed bytes into stretches
 * that inflate to about a slot each (by the ratio the trailer's ISIZE implies), rewinds the stream, and returns how many calls of
 * rk_fastq_slot_load_gzip the file takes.  Each call inflates the next stretch on the device -- block headers found by a kernel, a
 * lane per chunk, the text in front of a chunk resolved in stream order, CRC-32 and ISIZE checked at the end of the stream -- and
 * leaves the whole FASTQ records of it in the slot's device text, for rk_fastq_slot_submit / _count; the bytes behind the last
 * record start wait on the device for the next call.  Calls come in order, all on slots (RK_SLOT_DEVICE_TEXT) of one device.
 * rk_fastq_slot_load_gzip returns RK_OK, or 1: the device route ends here (stored / fixed-code stretches longer than a chunk's
 * scratch, text that outgrows the slot, a second member behind the first, no FASTQ) -- nothing of the text from *text_off on has
 * been delivered, and the caller's sequential reader (rk_reader_open_at(path, *text_off)) continues from there; < 0: damaged data. */
typedef struct rk_gzip rk_gzip;
int rk_gzip_open(const char* path, rk_gzip** out);
void rk_gzip_close(rk_gzip* gz);
const uint8_t* rk_gzip_image(const rk_gzip* gz);        /* the mapped file (rk_host_register_readonly lets the DMA engine read it) */
uint64_t rk_gzip_file_bytes(const rk_gzip* gz);
int rk_gzip_first_byte(const rk_gzip* gz);              /* of the text; -1: not decodable */
uint64_t rk_gzip_text_bytes_hint(const rk_gzip* gz);    /* from ISIZE (modulo 2^32): for sizing only */
int64_t rk_gzip_plan(rk_gzip* gz, uint64_t slot_bytes); /* calls the file takes; rewinds */
int64_t rk_gzip_calls(const rk_gzip* gz);
void rk_gzip_release_device(rk_gzip* gz);              /* frees the device buffers of a file that has been read; rk_gzip_plan before the next pass */
int rk_fastq_slot_load_gzip(rk_fastq_slot* s, rk_gzip* gz, int64_t call, uint64_t* nbytes, uint64_t* text_off);
uint64_t rk_gzip_stretch_bytes(const rk_gzip* gz);      /* compressed bytes per call, after rk_gzip_plan */
int rk_fastq_slot_reserve_gzip(rk_fastq_slot* s, uint64_t comp_bytes); /* optional: the work buffers of the calls, made ahead of the first one */
uint64_t rk_bgzf_file_bytes(const rk_bgzf* z);   /* length of rk_bgzf_image */

/* ------------------------------------------------------------------------------------------------
 * PACKED READS (`rkmh pack`, `stream|filter -F`; the reference parses -F/--pre-reads and does nothing with it, src/rkmh.cpp:659-664).
 * FASTQ text costs ~315 bytes per 150-base read on every hop; a packed file keeps per read 2 bits per base, a 4-byte offset and --
 * for the host only -- its name (and, optionally, its quality string): ~42 bytes per read cross the link, 16 come back.
 * File (little endian; every section 16-byte aligned so a mapping of the file can be uploaded as it lies):
 *   header  rk_packed_header
 *   blocks  per block: offsets u32[nrec + 1] (in BASES, from the block's first base), bases2 u8[ceil(nbases / 4)] (base i in bits
 *           2 (i & 3) of byte i >> 2; A = 0, C = 1, T = 2, G = 3 -- (ASCII >> 1) & 3 --, anything else stored as 0 and listed in),
 *           exceptions {u32 base index, u32 original byte}[nexc] (every byte that is not one of ACGTacgt: N, IUPAC codes ...; lower case
 *           acgt is NOT kept -- mkmh's to_upper folds it before anything looks, src/rkmh.cpp:856), name_offsets u32[nrec + 1], names
 *           (back to back, no terminators), quals u8[nbases] when the file keeps them
 *   directory  rk_packed_block[nblocks] at header.directory_off
 * rk_packed_encode fills one block's device-bound sections from ASCII bases (host code); rk_classify_batch_device_packed /
 * rk_count_batch_device_packed take them from device memory: the bases are expanded to ASCII in HBM (exceptions restored) and go
 * through the same kernels as rk_classify_batch_device_all / rk_count_batch_device -- rows are bit-identical by construction. */
#define RK_PACKED_MAGIC "RKPK1\n\0"
#define RK_PACKED_QUALS 1u
typedef struct rk_packed_header {
    char magic[8];
    uint32_t version, flags;          /* flags: RK_PACKED_QUALS */
    uint64_t nreads, nbases, nblocks;
    uint64_t directory_off;           /* rk_packed_block[nblocks] */
    uint64_t reserved[2];
} rk_packed_header;                   /* 64 bytes */
typedef struct rk_packed_block {
    uint64_t offsets_off, bases_off, exc_off, name_offsets_off, names_off, quals_off;  /* from the start of the file; quals_off 0: none */
    uint32_t nrec, nexc;
    uint64_t nbases, name_bytes;
    uint32_t max_len, pad;
} rk_packed_block;                    /* 80 bytes */
typedef struct rk_packed_exception { uint32_t pos, byte; } rk_packed_exception;
/* bases[0 .. n) -> bases2 (ceil(n / 4) bytes, the last byte's unused bits 0) and the exceptions (at most cap; positions are
 * base_index0 + i); returns the number of exceptions, or a negative error (more than cap).  Host code, thread-safe. */
int64_t rk_packed_encode(const uint8_t* bases, uint64_t n, uint64_t base_index0, uint8_t* bases2, rk_packed_exception* exc, uint64_t cap);
/* the inverse on the host (what filter prints of a passing read): bases [first, first + n) of a block -> ASCII, exceptions restored
 * (exc sorted by pos, as rk_packed_encode leaves them) */
void rk_packed_decode(const uint8_t* bases2, uint64_t first, uint64_t n, const rk_packed_exception* exc, uint32_t nexc, uint8_t* out);
/* d_bases2: ceil(nbases / 4) bytes (4-byte aligned, readable to the next multiple of 4); d_offsets_u32[nreads + 1] in bases;
 * d_exc: nexc pairs (may be NULL when nexc == 0); d_ascii: the caller's scratch, 16 * ceil(nbases / 16) + 64 bytes of device memory,
 * 16-byte aligned -- it holds the batch's ASCII bases on return.  Rows as rk_classify_batch_device_all (no row left flagged);
 * synchronises the stream. */
int rk_classify_batch_device_packed(rk_ctx* ctx, const void* d_bases2, const void* d_offsets_u32, int64_t nreads, uint64_t nbases,
                                    const void* d_exc, uint32_t nexc, void* d_ascii, void* d_out4, uint32_t max_read_len, void* hip_stream);
/* pass 1 of -M on such a batch (src/rkmh.cpp:904-910).  max_read_len: the longest read (the file's directory has it; required).  Asynchronous. */
int rk_count_batch_device_packed(rk_ctx* ctx, const void* d_bases2, const void* d_offsets_u32, int64_t nreads, uint64_t nbases,
                                 const void* d_exc, uint32_t nexc, void* d_ascii, rk_counter* counter, uint32_t max_read_len, void* hip_stream);

/* One block of a packed file in flight (own stream and device arrays): what `stream|filter -F` is made of.  file = the packed file
 * in memory (a mapping; page-locked with rk_host_register_readonly the DMA engine reads the page cache itself).  classify: res->out4 =
 * the rows; name_off / name_len index file + block->names_off (the stream formatter rk_fastq_stream_lines takes that as `text`);
 * seq_off (= qual_off) / seq_len are in BASES from the block's first base -- rk_packed_filter_records decodes what filter prints.
 * The arrays live in the slot and in the mapping until the slot's next call.  count: pass 1 of -M. */
typedef struct rk_packed_slot rk_packed_slot;
int rk_packed_slot_create(rk_ctx* ctx, uint64_t max_reads, uint64_t max_bases, rk_packed_slot** out);
void rk_packed_slot_destroy(rk_packed_slot* slot);
int rk_packed_slot_classify(rk_packed_slot* slot, const rk_packed_block* block, const uint8_t* file, rk_fastq_result* res);
int rk_packed_slot_count(rk_packed_slot* slot, const rk_packed_block* block, const uint8_t* file, rk_counter* counter);
uint64_t rk_packed_filter_records_bound(const rk_fastq_result* res);
int64_t rk_packed_filter_records(const rk_fastq_result* res, const rk_packed_block* block, const uint8_t* file, int min_matches, int min_diff,
                                 char* dst, uint64_t cap);

/* Loads the code objects of the device front end's kernels (with_inflate != 0: and of the device inflater) on `device` ahead of
 * their first launch -- tens of milliseconds a caller can spend on a second thread while its references are sketched.  Optional. */
int rk_warm_up(int device, int with_inflate);

/* ------------------------------------------------------------------------------------------------
 * SKETCH COMPARISON (`rkmh dist`; what `mash dist` and `sourmash compare` answer -- the reference compares sketches one pair at a
 * time, src/rkmh.cpp:869).  A sketch is a row of rk_sketch_batch: sketch_size uint64, ascending, the first len of them non-zero,
 * zeros behind.  Values may repeat (dedup=multiset) or not (dedup=distinct); D(x) = the distinct values of x[0, len).  Zeros are
 * padding, never values.  Every pair (row i of a, row j of b) gives four int32 at out4[(i * nb + j) * 4]:
 *   0 shared           sum over values of min(multiplicity in a, multiplicity in b) = rk_hash_intersection_size of the two rows
 *   1 shared_distinct  |D(a) & D(b)|
 *   2 common           |U & D(a) & D(b)|, U = the min(sketch_size, |D(a) | D(b)|) smallest values of D(a) | D(b): Mash's numerator
 *   3 denom            |U|
 * One launch of k_sketch_pairs (rk_pairs.hip): a tile of pairs per workgroup, a lane per pair walking a two-pointer merge.  Rows
 * that are not ascending give meaningless counts and nothing worse.
 * rk_compare_sketches: host arrays; RK_ERR_ARG for a sketch_size outside [1, RK_MAX_SKETCH], na or nb below 1, a length outside
 * [0, sketch_size], NULL.  a and b (and their lengths) may be the same arrays: uploaded once.  The answer is computed in row blocks.
 * rk_compare_sketches_device: device arrays the caller sized (d_out4: na * nb * 16 bytes), asynchronous on hip_stream (NULL = HIP's
 * null stream; rk_ctx_stream() = the context's own, as for rk_classify_batch_device); lengths outside [0, sketch_size] are clamped
 * on the device. */
int rk_compare_sketches(rk_ctx* ctx, const uint64_t* a, const int32_t* alens, int na, const uint64_t* b, const int32_t* blens, int nb,
                        int sketch_size, int32_t* out4);
int rk_compare_sketches_device(rk_ctx* ctx, const void* d_a, const void* d_alens, int na, const void* d_b, const void* d_blens, int nb,
                               int sketch_size, void* d_out4, void* hip_stream);
/* Host code, usable without a GPU (rk_pairs_host.cpp).  rk_merge_sketches: the sketch_size smallest values of the union of n
 * sketches -> out[sketch_size] (zero padded), *out_len; distinct = 0 keeps repeats, 1 keeps each value once.  Exact: the bottom of
 * a union only ever needs the bottom of each part.  rk_mash_distance: j = common / denom (0 when denom = 0); the distance is 1 when
 * common = 0, else -ln(2j / (1 + j)) / k clamped to [0, 1]; RK_ERR_ARG for negative counts, common > denom or k < 1. */
int rk_merge_sketches(const uint64_t* sketches, const int32_t* lens, int n, int sketch_size, int distinct, uint64_t* out, int32_t* out_len);
int rk_mash_distance(int common, int denom, int k, double* jaccard, double* distance);

/* ------------------------------------------------------------------------------------------------
 * SCALED SKETCHES (`rkmh sketch --scaled`, `rkmh dist --scaled`; the FracMinHash sketches that sourmash makes by default).  These
 * are this library's own definitions; no compatibility with any other tool's files is claimed.
 *   max_hash(scaled) = floor((2^64 - 1) / scaled), scaled >= 1; scaled = 1 keeps everything.
 *   The scaled sketch of a sequence: the ascending array of the DISTINCT window hashes h with 0 < h <= max_hash, under the
 *   context's policy and the k-mer sizes given, pooled over the sizes as rk_sketch_batch pools them.  0 stays "no hash".  A scaled
 *   sketch is a set under every policy (the dedup key governs bottom-S sketches only); fold, windows, canon and seed apply unchanged.
 *   A batch of scaled sketches is CSR: sketch i is values[offsets[i], offsets[i + 1]), both arrays uint64, offsets[n + 1].
 *   For a pair: shared = |A & B|, union = |A| + |B| - shared, Jaccard = shared / union, containment of A in B = shared / |A|.
 *   A sketch made at scaled = n becomes one of scaled N >= n by cutting it at the first value above max_hash(N) (rk_merge_scaled).
 * rk_scaled_max_hash: host only; RK_ERR_ARG for scaled = 0.
 * rk_sketch_scaled_batch: input as for rk_hash_batch.  *values is malloc'd (rk_free), sk_offsets[nseq + 1] is the caller's.  It takes
 * max_hash rather than scaled, so a threshold can sit exactly on a hash.  Any batch the general path takes: empty sequences,
 * sequences shorter than k, up to 2^31 - 1 bases in one, any number of chunks.  Per chunk the window hashes are kept, compacted with
 * wave ballots, sorted by sequence and freed of repeats on the device (rk_scaled.hip).
 * rk_compare_scaled: host arrays; shared[i * nb + j] = |a_i & b_j|.  a and b may be the same arrays: uploaded once.  RK_ERR_ARG for
 * NULL, na or nb below 1, offsets that decrease, a sketch of 2^31 values or more, lanes outside {0, 1, 8, 64}.  The answer is
 * downloaded in row blocks.  lanes: how many lanes of k_scaled_pairs share one pair; 0 = chosen from the mean length of the shorter
 * side; the answer never depends on it.
 * rk_compare_scaled_device: resident arrays (x_nvalues = the number of uint64 behind d_x_values; d_shared: na * nb int32),
 * asynchronous on hip_stream (NULL = HIP's null stream; rk_ctx_stream() = the context's own).  Every row is clamped on the device to
 * lie inside [0, nvalues]; rows that are not ascending give meaningless counts and nothing worse.
 * rk_merge_scaled: host only; the ascending distinct union of n sketches cut at max_hash -> *out (malloc'd, rk_free), *out_len.
 * rk_scaled_distance: host only; rk_mash_distance's formula and clamps on j = shared / (la + lb - shared); j = 0 and distance 1 when
 * the union is empty; RK_ERR_ARG for negative counts, shared > min(la, lb) or k < 1.  Either result pointer may be NULL. */
int rk_scaled_max_hash(uint64_t scaled, uint64_t* max_hash);
int rk_sketch_scaled_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nseq, const int* ks, int nks,
                           uint64_t max_hash, uint64_t** values, uint64_t* sk_offsets);
int rk_compare_scaled(rk_ctx* ctx, const uint64_t* a_values, const uint64_t* a_offsets, int na, const uint64_t* b_values,
                      const uint64_t* b_offsets, int nb, int lanes, int32_t* shared);
int rk_compare_scaled_device(rk_ctx* ctx, const void* d_a_values, const void* d_a_offsets, int na, uint64_t a_nvalues,
                             const void* d_b_values, const void* d_b_offsets, int nb, uint64_t b_nvalues, int lanes,
                             void* d_shared, void* hip_stream);
int rk_merge_scaled(const uint64_t* values, const uint64_t* offsets, int n, uint64_t max_hash, uint64_t** out, uint64_t* out_len);
int rk_scaled_distance(int64_t shared, int64_t la, int64_t lb, int k, double* jaccard, double* distance);

/* ------------------------------------------------------------------------------------------------
 * GATHER (`rkmh gather`; the greedy minimum-set-cover that sourmash calls `gather`: which references make up a sample, and how much
 * of it each explains once the better matches are taken out).  These are this library's own definitions.
 *   Inputs: a query set Q of nq ascending, distinct, non-zero uint64; nref reference sets in CSR (values, offsets[nref + 1]), each
 *   ascending and distinct; min_shared >= 1; max_rounds >= 1.
 *   State: alive = Q; total[r] = |Q & R_r|.
 *   Round t = 0, 1, ...: count[r] = |alive & R_r| for every r; the pick is the r with the largest count, among equals the LOWEST
 *   reference index; if that count is below min_shared, stop; otherwise the row
 *     out4[t] = (ref, unique = count[ref], total[ref], remaining = |alive| after the removal), four int32,
 *   is written and alive -= R_ref; stop after max_rounds rows.  *nrounds = the number of rows written.
 *   It follows that unique never increases from row to row, that no reference is picked twice, that nq - sum(unique) = remaining of
 *   the last row, and that a reference whose total is below min_shared is never picked.  Base-pair estimates are not part of
 *   it; abundance and the weighted share of a pick: "ABUNDANCE" below.
 * All three entries refuse (RK_ERR_ARG, a size beyond the limit RK_ERR_LIMIT) before anything is launched: NULL, nref < 1,
 * min_shared < 1, max_rounds < 1, nq > 2^31 - 1.
 * rk_gather_scaled: host arrays; additionally refuses a query that is not strictly ascending or holds 0, offsets that decrease and a
 * row of 2^31 values or more.  out4 holds min(max_rounds, nref) rows.
 * rk_gather_scaled_device: resident arrays (r_nvalues = the number of uint64 behind d_r_values), so a database stays resident while
 * many queries are gathered against it; d_out4 takes at most max_rounds rows (min(max_rounds, nref) are all there can be).  It runs on
 * hip_stream (NULL = HIP's null stream; rk_ctx_stream() = the context's own) and SYNCHRONISES it: the setup needs the hit counts on
 * the host to lay out the candidates' hit lists, and every group of RK_GATHER_BATCH rounds ends with a look at the state.  Every row
 * is clamped on the device to lie inside [0, r_nvalues] and every index is checked before it is used; rows or a query that are not
 * ascending give meaningless rows and nothing worse.  The work buffers are the context's: calls on one context take turns.
 * The kernels (rk_gather.hip): k_gather_probe and k_gather_compact once per call (each reference value looked up in Q; the hits
 * of every candidate -- a reference with total >= min_shared -- as a list of query indices), then per round k_gather_count,
 * k_gather_pick, k_gather_remove on one byte per query value, without a host round trip inside a group of rounds.
 * rk_gather_scaled_host: host code, usable without a GPU (rk_scaled_host.cpp): the same rows from the same loop on `threads` host
 * threads (below 1: one); the checks of rk_gather_scaled. */
#define RK_GATHER_BATCH 16 /* rounds enqueued between two looks at the state; the rows never depend on it */
int rk_gather_scaled(rk_ctx* ctx, const uint64_t* q_values, uint64_t nq, const uint64_t* r_values, const uint64_t* r_offsets, int nref,
                     int min_shared, int max_rounds, int32_t* out4, int* nrounds);
int rk_gather_scaled_device(rk_ctx* ctx, const void* d_q_values, uint64_t nq, const void* d_r_values, const void* d_r_offsets, int nref,
                            uint64_t r_nvalues, int min_shared, int max_rounds, void* d_out4, int* nrounds, void* hip_stream);
int rk_gather_scaled_host(const uint64_t* q_values, uint64_t nq, const uint64_t* r_values, const uint64_t* r_offsets, int nref,
                          int min_shared, int max_rounds, int threads, int32_t* out4, int* nrounds);

/* ------------------------------------------------------------------------------------------------
 * ABUNDANCE (`rkmh sketch --scaled <n> --abund`, `rkmh gather --abund`; what sourmash calls track_abundance).  These are this
 * library's own definitions, chosen to coincide with sourmash's where that can be known.
 *   The abundance sketch of a sequence at max_hash: its scaled sketch values[] (unchanged: ascending, distinct, 0 < h <= max_hash)
 *   plus a parallel uint32 abund[]: abund[j] = the number of windows of that sequence whose hash equals values[j], pooled over the
 *   k-mer sizes as the values are.  Windows that hash to 0 are not counted.  Every abundance is >= 1 and sum(abund) = the number of
 *   kept windows (a count beyond 2^32 - 1 is stored as 2^32 - 1).  A batch is the CSR of scaled sketches plus one uint32 per value.
 *   Union (the -g reduction; one query per -f file): the ascending distinct union of the values; abundances are summed per value,
 *   saturating at 2^32 - 1.  Cutting to a larger `scaled` keeps the prefix of both arrays.
 *   Weighted gather: rows and pick rule are exactly rk_gather_scaled's -- the pick is by the UNWEIGHTED count, lowest reference index
 *   among equals.  Row t also gets uint64 wunique[t] = the sum of q_abund[i] over the query values i that the pick of row t removes
 *   (the ones still alive at its turn).  wtotal = sum(q_abund) is the caller's to compute.  Reference abundances play no part.  It
 *   follows that with all abundances 1 wunique = unique, and that sum_t wunique[t] + the abundances of the values alive at the end
 *   = wtotal.
 * rk_sketch_scaled_abund_batch: rk_sketch_scaled_batch plus *abunds (both malloc'd, rk_free); the values are bit-identical to
 * rk_sketch_scaled_batch's.  On the device the abundance of a value is the length of its run among the sorted kept values of its
 * sequence, taken where the repeats are dropped (rk_scaled.hip: k_keep_first_src, k_run_lengths); it leaves with the values.
 * rk_merge_scaled_abund: host only; rk_merge_scaled plus the summed abundances; RK_ERR_ARG also for a NULL abunds and an abundance of 0.
 * rk_gather_scaled_abund / _device / _host: rk_gather_scaled / _device / _host plus q_abund (uint32[nq]) and wunique; the checks of
 * their plain forms, and RK_ERR_ARG for a NULL q_abund when nq > 0 and for a NULL wunique.  wunique takes min(max_rounds, nref)
 * uint64 (d_wunique: max_rounds may be given) and is zeroed that far at the start of every call, then rows [0, *nrounds) are written.
 * The two entries that take host arrays also refuse an abundance of 0; the device entry cannot check that cheaply: there a 0 adds
 * nothing.  On the device k_gather_remove_w takes k_gather_remove's place, so a round stays three launches. */
int rk_sketch_scaled_abund_batch(rk_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, int64_t nseq, const int* ks, int nks,
                                 uint64_t max_hash, uint64_t** values, uint32_t** abunds, uint64_t* sk_offsets);
int rk_merge_scaled_abund(const uint64_t* values, const uint32_t* abunds, const uint64_t* offsets, int n, uint64_t max_hash,
                          uint64_t** out_values, uint32_t** out_abunds, uint64_t* out_len);
int rk_gather_scaled_abund(rk_ctx* ctx, const uint64_t* q_values, const uint32_t* q_abund, uint64_t nq, const uint64_t* r_values,
                           const uint64_t* r_offsets, int nref, int min_shared, int max_rounds, int32_t* out4, uint64_t* wunique, int* nrounds);
int rk_gather_scaled_abund_device(rk_ctx* ctx, const void* d_q_values, const void* d_q_abund, uint64_t nq, const void* d_r_values,
                                  const void* d_r_offsets, int nref, uint64_t r_nvalues, int min_shared, int max_rounds, void* d_out4,
                                  void* d_wunique, int* nrounds, void* hip_stream);
int rk_gather_scaled_abund_host(const uint64_t* q_values, const uint32_t* q_abund, uint64_t nq, const uint64_t* r_values,
                                const uint64_t* r_offsets, int nref, int min_shared, int max_rounds, int threads, int32_t* out4,
                                uint64_t* wunique, int* nrounds);

/* ------------------------------------------------------------------------------------------------
 * WEIGHTED COMPARISON (`rkmh dist --abund`: two abundance sketches compared by the angle between their abundance vectors, as the
 * sourmash family compares samples once abundances are tracked).  These are this library's own definitions; no compatibility with any
 * other tool's files is claimed.
 *   Inputs: an abundance sketch is values[] (ascending, distinct, non-zero uint64) and a parallel uint32 abund[], every entry >= 1; a
 *   batch is the CSR of scaled sketches plus one uint32 per value, as rk_sketch_scaled_abund_batch returns it.  wA(x) = the abundance
 *   of value x in sketch A.
 *   Per pair (row i of a, row j of b), four uint64 at out4[(i * nb + j) * 4]:
 *     0 shared   |A & B|: rk_compare_scaled's number for the pair
 *     1 dot      sum over x in A & B of wA(x) * wB(x); every product fits 64 bits, the SUM SATURATES at 2^64 - 1
 *     2 wa_in    sum over x in A & B of wA(x)
 *     3 wb_in    sum over x in A & B of wB(x)
 *   Saturating addition of non-negative numbers is associative and commutative: the result is min(true sum, 2^64 - 1) in whatever
 *   order the lanes add, so it is the same for every `lanes` value.  wa_in and wb_in cannot overflow (fewer than 2^31 values, each
 *   below 2^32).
 *   Per sketch (rk_abund_row_sums*), two uint64 at out2[i * 2]: sum = the sum of its abundances, exact; sumsq = the sum of their
 *   squares, saturating at 2^64 - 1.
 *   It follows that with all abundances 1 dot = wa_in = wb_in = shared; that swapping the sides swaps fields 2 and 3 and keeps 0 and
 *   1; and that a sketch against itself gives dot = sumsq, wa_in = wb_in = sum and shared = its length.
 *   Floating point, host only: rk_angular_similarity(dot, sumsq_a, sumsq_b): cosine = (double)dot / sqrt((double)sumsq_a *
 *   (double)sumsq_b), clamped to at most 1; angular = 1 - 2 acos(cosine) / pi.  When either sumsq is 0 both results are 0.  The root is
 *   taken of the product, not of each factor: sqrt(fl(s) * fl(s)) is fl(s) exactly in IEEE binary arithmetic, so a sketch compared
 *   with itself gives cosine 1 and angular similarity 1.  RK_ERR_ARG when dot is positive and one of the sumsq is 0; a saturated
 *   input is taken as the number it is.  Either result pointer may be NULL.
 * rk_compare_scaled_abund: host arrays; the checks of rk_compare_scaled, and RK_ERR_ARG for a NULL abundance array where there are
 * values and for an abundance of 0.  a and b may be the same arrays: uploaded once, abundances included.  The answer is downloaded in
 * row blocks of at most 64 MB (a row is nb * 32 bytes).  lanes as for rk_compare_scaled; the answer never depends on it.
 * rk_compare_scaled_abund_device: resident arrays (d_x_abund: x_nvalues uint32 parallel to d_x_values; d_out4: na * nb * 32 bytes),
 * asynchronous on hip_stream; every row is clamped on the device to lie inside [0, nvalues], and every abundance is read at an index
 * at which a value of that clamped row was just read; rows that are not ascending give meaningless numbers and nothing worse.  This
 * entry cannot check the abundances cheaply: a 0 adds nothing.
 * rk_abund_row_sums: host arrays, n >= 1; RK_ERR_ARG for NULL, offsets that decrease, a row of 2^31 values or more, an abundance of
 * 0.  rk_abund_row_sums_device: resident arrays (nvalues = the number of uint32 behind d_abund; d_out2: n * 16 bytes), asynchronous,
 * rows clamped as above.
 * The kernels (rk_scaled.hip): k_scaled_pairs<1 | 8 | 64, PairsWeighted> -- the layout, slices and merge of the plain comparison
 * (k_scaled_pairs<L, PairsPlain>) carrying four sums instead of one count -- and k_abund_row_sums, one wave per row.
 * rk_compare_scaled_abund_host, rk_abund_row_sums_host, rk_angular_similarity: host code, usable without a GPU (rk_scaled_host.cpp);
 * the checks of the entries on host arrays; `threads` host threads share the rows of a (below 1: one). */
int rk_compare_scaled_abund(rk_ctx* ctx, const uint64_t* a_values, const uint32_t* a_abund, const uint64_t* a_offsets, int na,
                            const uint64_t* b_values, const uint32_t* b_abund, const uint64_t* b_offsets, int nb, int lanes, uint64_t* out4);
int rk_compare_scaled_abund_device(rk_ctx* ctx, const void* d_a_values, const void* d_a_abund, const void* d_a_offsets, int na, uint64_t a_nvalues,
                                   const void* d_b_values, const void* d_b_abund, const void* d_b_offsets, int nb, uint64_t b_nvalues, int lanes,
                                   void* d_out4, void* hip_stream);
int rk_abund_row_sums(rk_ctx* ctx, const uint32_t* abund, const uint64_t* offsets, int n, uint64_t* out2);
int rk_abund_row_sums_device(rk_ctx* ctx, const void* d_abund, const void* d_offsets, int n, uint64_t nvalues, void* d_out2, void* hip_stream);
int rk_compare_scaled_abund_host(const uint64_t* a_values, const uint32_t* a_abund, const uint64_t* a_offsets, int na, const uint64_t* b_values,
                                 const uint32_t* b_abund, const uint64_t* b_offsets, int nb, int threads, uint64_t* out4);
int rk_abund_row_sums_host(const uint32_t* abund, const uint64_t* offsets, int n, uint64_t* out2);
int rk_angular_similarity(uint64_t dot, uint64_t sumsq_a, uint64_t sumsq_b, double* cosine, double* angular);

/* ------------------------------------------------------------------------------------------------
 * SEARCH (`rkmh manysearch`; what the sourmash family calls manysearch: many query sketches against a large collection of reference
 * sketches, reporting only the pairs that match).  These are this library's own definitions.
 *   Inputs: a reference batch of scaled sketches in CSR (uint64 values[], uint64 offsets[nref + 1]), every row ascending, distinct and
 *   non-zero; a query batch of the same form with nq rows; a scalar min_shared >= 1 and an optional int32 q_min[nq].  A NULL q_min:
 *   every query's threshold is min_shared; otherwise query i's threshold is max(min_shared, q_min[i]).
 *   Index: for each distinct value over all reference rows, the ascending list of the references that hold it (its posting list):
 *     keys[nkeys]          ascending distinct uint64
 *     post_off[nkeys + 1]  uint64; the list of keys[j] is post[post_off[j], post_off[j + 1])
 *     post[npost]          uint32 reference ids, ascending within a key; npost = the number of reference values
 *   Answer: an array of hits rk_search_hit = {int32 query, int32 ref, int32 shared}: one hit per pair with shared = |Q_query & R_ref|
 *   at or above that query's threshold, nothing for any other pair, sorted by (query, ref) ascending.  It follows that with every
 *   threshold at 1 the hits are exactly the non-zero entries of rk_compare_scaled on the same inputs, in row-major order, with the same
 *   counts; and that an empty query or an empty reference gives no hit.
 * rk_scaled_index_create: host arrays; RK_ERR_ARG for NULL, nref < 1, offsets that decrease, a row of 2^31 values or more; RK_ERR_LIMIT
 * for more than 2^31 - 1 rows or 2^32 - 1 values.  The values are uploaded, the index is built on the device once (a kernel writes the
 * reference id of every value position, a stable radix sort orders the (value, id) pairs by value, the first of every value is kept
 * as its key) and stays resident until rk_scaled_index_destroy.  It belongs to the context it was made on and is used with no other;
 * it may be destroyed before or after it.  Searches on one index take turns (its work buffers are its own).
 * rk_scaled_index_create_device: resident arrays (nvalues = the number of uint64 behind d_values; they are only read, and not needed
 * after the call); runs on hip_stream (NULL = HIP's null stream) and SYNCHRONISES it.  Every row is clamped on the device to lie
 * inside [0, nvalues], as k_scaled_pairs clamps its rows; npost = nvalues; a position no row covers gets the id 2^32 - 1, which no
 * search counts.  Rows that are not ascending give a meaningless index and nothing worse.
 * rk_scaled_index_stats: the caller sets out->struct_size as for rk_index_stats; longest_posting = the entries of the longest list.
 * rk_search_scaled: host arrays; *hits is malloc'd (rk_free; never NULL on success), *nhits the number of hits.
 * rk_search_scaled_device: resident arrays (q_nvalues = the number of uint64 behind d_q_values; d_q_min NULL or nq int32; d_hits takes
 * cap_hits hits of 12 bytes, and may be NULL when cap_hits = 0).  Writes the first min(total, cap_hits) hits in order and returns the
 * total in *nhits.  It runs on hip_stream and SYNCHRONISES it, as rk_gather_scaled_device does: the total is read on the host between
 * the counting pass and the writing pass.  Query rows are clamped to [0, q_nvalues]; a d_q_min entry below 1 counts as 1 (this entry
 * cannot check them cheaply); every index is checked before it is used; rows that are not ascending give meaningless hits and nothing
 * worse.
 * All entries refuse (RK_ERR_ARG, a size beyond its limit RK_ERR_LIMIT) before anything is launched: NULL, nq < 1, min_shared < 1, a
 * q_min entry below 1 (host arrays only), more than 2^31 - 1 rows on a side, more than 2^24 - 1 workgroups in one call (nq times the
 * number of reference blocks: search the queries in several calls), an index of another context.
 * The kernels (rk_search.hip): k_search_block<EMIT>, one workgroup per (query, block of RK_SEARCH_REF_BLOCK consecutive references)
 * with the block's int32 counters in LDS; lanes stride the query's values, look each up in keys (at most 32 halvings), narrow its
 * posting list to the block's ids (two more searches) and add 1 to the counter of every reference in that range (a list of 64
 * entries or more inside the block is walked by the whole wave).  Integer adds commute: the counts do not depend on the order of
 * arrival.  Pass 1 stores the number of counters at or above the threshold per workgroup, an exclusive 64-bit scan gives every
 * workgroup its place, pass 2 recomputes the counters and writes its hits in ascending reference order.  No atomics on global memory.
 * rk_search_scaled_host: host code, usable without a GPU (rk_scaled_host.cpp): the same array from an index built on the host, on
 * `threads` host threads (below 1: one); the checks of rk_search_scaled.
 * rk_search_min_count: host only; *t = the smallest integer t with (double)t / (double)len >= x, the count that a containment
 * shared / |query| >= x asks of a query of len values (0 for x = 0 or len = 0; never above len).  `rkmh manysearch --min-containment`
 * passes max(1, t) as q_min.  RK_ERR_ARG for x outside [0, 1] (a NaN included), RK_ERR_LIMIT for len > 2^31 - 1. */
#define RK_SEARCH_REF_BLOCK 8192 /* references per workgroup of the search kernel: 32 KB of int32 counters in LDS */
typedef struct rk_search_hit { int32_t query, ref, shared; } rk_search_hit;
typedef struct rk_scaled_index rk_scaled_index;
typedef struct rk_scaled_index_stats_t {
    uint32_t struct_size;
    uint32_t nref;
    uint64_t npost, nkeys;
    uint32_t longest_posting, reserved;
} rk_scaled_index_stats_t;
int rk_scaled_index_create(rk_ctx* ctx, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, rk_scaled_index** idx);
int rk_scaled_index_create_device(rk_ctx* ctx, const void* d_values, const void* d_offsets, int64_t nref, uint64_t nvalues, void* hip_stream,
                                  rk_scaled_index** idx);
void rk_scaled_index_destroy(rk_scaled_index* idx);
int rk_scaled_index_stats(const rk_scaled_index* idx, rk_scaled_index_stats_t* out);
int rk_search_scaled(rk_ctx* ctx, rk_scaled_index* idx, const uint64_t* q_values, const uint64_t* q_offsets, int64_t nq, int min_shared,
                     const int32_t* q_min, rk_search_hit** hits, uint64_t* nhits);
int rk_search_scaled_device(rk_ctx* ctx, rk_scaled_index* idx, const void* d_q_values, const void* d_q_offsets, int64_t nq, uint64_t q_nvalues,
                            int min_shared, const void* d_q_min, void* d_hits, uint64_t cap_hits, uint64_t* nhits, void* hip_stream);
int rk_search_scaled_host(const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, const uint64_t* q_values, const uint64_t* q_offsets,
                          int64_t nq, int min_shared, const int32_t* q_min, int threads, rk_search_hit** hits, uint64_t* nhits);
int rk_search_min_count(double min_containment, uint64_t len, int32_t* t);

/* ------------------------------------------------------------------------------------------------
 * MULTIGATHER (`rkmh multigather`; what the sourmash family calls fastmultigather: GATHER for a batch of queries at once, through the
 * inverted index of SEARCH).  These are this library's own definitions.
 *   Inputs: a rk_scaled_index of the references; a query batch of nq rows in CSR (uint64 q_values[], uint64 q_offsets[nq + 1]), every
 *   row ascending, distinct and non-zero -- rows may be empty, and rows may repeat one another; an optional uint32 q_abund[] parallel
 *   to q_values, every entry >= 1; min_shared >= 1; max_rounds >= 1.
 *   Answer: the rows of query i are EXACTLY the rows rk_gather_scaled gives for Q_i against the indexed references with the same
 *   min_shared and max_rounds: (ref, unique, total, remaining), four int32; the pick is by the largest count, among equal counts the
 *   lowest reference index; a query stops when its best count falls below min_shared, or after max_rounds rows.  With q_abund every
 *   row also has a uint64 wunique as rk_gather_scaled_abund defines it.  Queries do not influence each other.  The output is compact:
 *   uint64 row_offsets[nq + 1], the rows of query i at [row_offsets[i], row_offsets[i + 1]) in pick order, wunique parallel to the rows.
 *   It follows that permuting the queries permutes the row blocks; that a query given twice gets the same rows twice; and that an
 *   empty query, or a query with no candidate (no reference shares min_shared values with it), gets no row.
 * rk_multigather_scaled: host arrays.  *rows4 and, when q_abund is given, *wunique are malloc'd (rk_free; never NULL on success);
 * row_offsets (nq + 1 uint64) is the caller's; *nrows = row_offsets[nq].  The checks of rk_search_scaled, and those of rk_gather_scaled
 * on every row: RK_ERR_ARG for a row that is not strictly ascending or holds 0, and for an abundance of 0.
 * rk_multigather_scaled_device: resident arrays (q_nvalues = the number of uint64 behind d_q_values; d_q_abund NULL or q_nvalues
 * uint32; d_out4 takes cap_rows rows of 16 bytes and d_wunique cap_rows uint64 -- d_wunique is used only with d_q_abund, and both may
 * be NULL when cap_rows = 0; d_row_offsets nq + 1 uint64).  Writes the first min(total, cap_rows) rows in order, ALWAYS all of
 * d_row_offsets, and returns the total in *nrows: the convention of rk_search_scaled_device.  It runs on hip_stream and SYNCHRONISES
 * it, as rk_gather_scaled_device does: the number of candidates is read on the host before the state is laid out, and every group of
 * RK_GATHER_BATCH rounds ends with a look at a 16-byte control word.  Query rows are clamped to [0, q_nvalues]; every index is checked
 * before it is used; rows that are not ascending give meaningless rows and nothing worse.  The alive bytes lie parallel to d_q_values:
 * query rows that share storage (possible only with offsets that do not ascend) share them, and then get meaningless rows and nothing
 * worse.  This entry cannot check abundances cheaply: a 0 adds nothing.
 * rk_multigather_scaled_host: host code, usable without a GPU (rk_scaled_host.cpp): the reference CSR instead of an index; the loop
 * of rk_gather_scaled_host query after query, the queries shared among `threads` host threads (below 1: one); the same checks (and
 * those of rk_gather_scaled_host on the references), the same arrays.
 * All entries refuse (RK_ERR_ARG, a size beyond its limit RK_ERR_LIMIT) before anything is launched: NULL, nq < 1, min_shared < 1,
 * max_rounds < 1, more than 2^31 - 1 rows on a side, more than 2^24 - 1 workgroups of the search (nq times the number of reference
 * blocks), an index of another context.  More than 2^31 - 1 candidates -- (query, reference) pairs that share at least min_shared
 * values, known after the counting pass -- give RK_ERR_LIMIT: send fewer queries per call.  The work buffers are the index's own, under
 * its mutex, as the search's are: calls on one index take turns, and the context's structure is not touched.
 * The kernels (rk_multigather.hip).  Candidates: k_search_block<false / true> at threshold min_shared; the hits of a query, ascending
 * by reference, are its candidates, shared = total = the initial count.  k_mg_keypos stores once where every query value stands in
 * keys.  A round is two launches for the whole batch: k_mg_pick, one workgroup per query, takes the maximum of (count << 32 |
 * ~candidate position) and writes the row; k_mg_remove looks the pick up in the posting list of every alive value of its query, and
 * on a match clears the value's byte, adds its abundance to the row's wunique and takes 1 from the count of every candidate of that
 * query the posting list names.  THESE ARE INTEGER ATOMICS ON GLOBAL MEMORY (atomicSub, atomicAdd; the first in the sketch-set layer):
 * integer adds commute, so the counts a pick reads, and with them the rows, never depend on the order of arrival; pick and remove are
 * separate launches on one stream, so no pick reads counts a remove is still changing.  The last kernel, k_mg_pack, lays the rows out
 * in query order. */
int rk_multigather_scaled(rk_ctx* ctx, rk_scaled_index* idx, const uint64_t* q_values, const uint32_t* q_abund, const uint64_t* q_offsets,
                          int64_t nq, int min_shared, int max_rounds, int32_t** rows4, uint64_t** wunique, uint64_t* row_offsets, uint64_t* nrows);
int rk_multigather_scaled_device(rk_ctx* ctx, rk_scaled_index* idx, const void* d_q_values, const void* d_q_abund, const void* d_q_offsets,
                                 int64_t nq, uint64_t q_nvalues, int min_shared, int max_rounds, void* d_out4, void* d_wunique, uint64_t cap_rows,
                                 void* d_row_offsets, uint64_t* nrows, void* hip_stream);
int rk_multigather_scaled_host(const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, const uint64_t* q_values, const uint32_t* q_abund,
                               const uint64_t* q_offsets, int64_t nq, int min_shared, int max_rounds, int threads, int32_t** rows4,
                               uint64_t** wunique, uint64_t* row_offsets, uint64_t* nrows);

/* ------------------------------------------------------------------------------------------------
 * SAMPLE SKETCHES (the -g / one-sketch-per-file side of `rkmh sketch --scaled`, `gather`, `multigather`: the one scaled sketch of a
 * whole read set, built on the device).  These are this library's own definitions.
 *   A sample is one abundance sketch at (ks, the context's policy, max_hash) that reads are ADDED to.  After any sequence of adds it
 *   equals rk_merge_scaled_abund over the rk_sketch_scaled_abund_batch rows of every sequence fed, at the same ks, policy and
 *   max_hash, bit for bit: values ascending, distinct, 0 < h <= max_hash; abund[j] = the number of windows, over all sequences fed,
 *   that hash to values[j], saturating at 2^32 - 1.  A sample created without abundances holds the same values and no abund array.
 *   The result never depends on batch boundaries, the order of the feeds, pending_cap or the number of folds.
 *   On the device the sample is a resident distinct set (values, counts) and, behind it, a PENDING array of kept window hashes.  A
 *   feed (k_sample_keep, rk_sample.hip) treats the batch's bases as one piece cut into tiles of 2048 window positions, stages a tile
 *   in LDS, marks the read starts that fall into it, hashes every position that is a window of its read -- a window that crosses a
 *   read start is none, a read has len - k or len - k + 1 windows as the policy says, a window with an invalid base hashes to 0 and 0
 *   is never kept -- and appends the hashes 0 < h <= max_hash to the pending array: compacted with wave ballots in LDS, then one
 *   64-bit atomicAdd on a device cursor per flush of a workgroup (integer atomics on global memory, as in MULTIGATHER; the array is
 *   sorted afterwards, so the order of arrival never reaches the result).  The window hashes of the batch are never written out.
 *   Every store is guarded by position + count <= capacity and the cursor always advances: after a feed the host reads the cursor
 *   (the one look a feed needs).  Beyond the capacity, the cursor is set back to where the batch began, the values from before are
 *   folded, the pending array grows to what the cursor asked for and the batch runs again: nothing is lost, nothing counted twice.
 *   A FOLD unites pending and resident: (value, count) pairs, pending ones with count 1, are radix-sorted by value, the first of every
 *   run is kept (the order-preserving compaction of the sketch-set layer) and k_run_sums adds each run's counts, saturating at
 *   2^32 - 1.  Without abundances only the values are sorted.  A fold synchronises.
 * rk_sample_create: pending_cap = values the pending array holds; 0 = the library's default (2^22 values, 32 MB); any other value is
 *   taken as given, down to 1 (it grows when one batch needs more).  RK_ERR_ARG / RK_ERR_LIMIT for NULL, nks outside 1 .. RK_MAX_KS, a k
 *   outside 1 .. RK_MAX_K, max_hash = 0.  The sample uses the policy its context has at each feed and is used with that context only;
 *   destroy it before the context.
 * rk_sample_add_batch: host arrays as for rk_hash_batch; refuses offsets that decrease and a sequence of 2^31 bases or more.  The
 *   bases are uploaded in pieces of whole sequences (about 64 MB; a longer sequence alone in its piece) on the context's stream.
 * rk_sample_add_batch_device: resident bases and uint32 offsets[nseq + 1], the form rk_count_batch_device takes, any read lengths;
 *   runs on hip_stream (NULL = HIP's null stream) and SYNCHRONISES it for the look at the cursor.  Offsets that do not ascend give a
 *   meaningless sample and no store outside the sample's arrays; the bases from offsets[0] to offsets[nseq] (and up to three bytes
 *   beyond, to the next dword) must be readable.
 * rk_sample_add_sketch: unites an abundance sketch (ascending, distinct, non-zero values; abundances >= 1: the checks of
 *   rk_merge_scaled_abund) into the sample; values above max_hash are cut off.  abund may be NULL only for a sample without abundances;
 *   such a sample ignores abundances that are given and adds one per value to `kept`.
 * rk_fastq_slot_sample: rk_fastq_slot_count's steps on a block of raw FASTQ text, then a feed from the slot's packed bases.
 *   *status != 0: the block is not four lines per record and NOTHING of it was added.  The only slot entry that works on a context
 *   without references.  RK_ERR_ARG for a sample of another context.
 * rk_sample_finish: folds what is pending; *values and, for a sample with abundances, *abund are malloc'd (rk_free; never NULL on
 *   success), *n their length.  The sample stays usable.  abund may be NULL for a sample without abundances.
 * rk_sample_device: folds, then gives the resident arrays (uint64 values, uint32 abundances or NULL): valid until the next add, reset
 *   or destroy; what rk_gather_scaled_device and rk_multigather_scaled_device take as a query, without a round trip.
 * rk_sample_stats: the caller sets out->struct_size as for rk_index_stats.  nseq, nbases: sequences and bases fed (a refused FASTQ
 *   block adds none); kept: windows kept = the unsaturated sum of the abundances; distinct: the length after the last fold; folds,
 *   retries: folds done, batches run a second time.
 * rk_sample_reset: an empty sample again, its arrays kept.  Calls on one sample take turns. */
typedef struct rk_sample rk_sample;
typedef struct rk_sample_stats_t { uint32_t struct_size, folds, retries, reserved; uint64_t nseq, nbases, kept, distinct; } rk_sample_stats_t;
int rk_sample_create(rk_ctx* ctx, const int* ks, int nks, uint64_t max_hash, int with_abund, uint64_t pending_cap, rk_sample** out);
void rk_sample_destroy(rk_sample* sample);
int rk_sample_reset(rk_sample* sample);
int rk_sample_add_batch(rk_sample* sample, const uint8_t* bases, const uint64_t* offsets, int64_t nseq);
int rk_sample_add_batch_device(rk_sample* sample, const void* d_bases, const void* d_offsets_u32, int64_t nseq, void* hip_stream);
int rk_sample_add_sketch(rk_sample* sample, const uint64_t* values, const uint32_t* abund, uint64_t n);
int rk_fastq_slot_sample(rk_fastq_slot* slot, uint64_t nbytes, rk_sample* sample, int32_t* status, int64_t* nrec);
int rk_sample_finish(rk_sample* sample, uint64_t** values, uint32_t** abund, uint64_t* n);
int rk_sample_device(rk_sample* sample, const void** d_values, const void** d_abund, uint64_t* n);
int rk_sample_stats(rk_sample* sample, rk_sample_stats_t* out);

/* BOTTOM SAMPLES (the -g side of `rkmh sketch -s` and `rkmh dist -s`: the one bottom-s sketch of a whole read set, built on the
 * device, with --min-copies).  These are this library's own definitions.
 *   Let W be the multiset of the non-zero window hashes of every sequence fed -- the windows are the policy's and the k list is
 *   pooled, exactly as rk_sketch_batch and the samples above take them -- and c(v) the multiplicity of v in W.  At sketch_size S
 *   (1 .. RK_MAX_SKETCH) and min_copies m (1 .. 2^32 - 1), v QUALIFIES when c(v) >= m.  The sketch is, ascending:
 *     dedup=distinct: the S smallest qualifying values, each once;
 *     dedup=multiset: the S smallest elements of W restricted to qualifying values -- each qualifying value c(v) times, the last
 *       one cut off where S is reached.
 *   The dedup rule is the context's policy.  At m = 1 this is rk_merge_sketches over the rk_sketch_batch rows of every sequence fed,
 *   bit for bit.  Counts saturate at 2^32 - 1 as above; a saturated count qualifies for every m, and S <= 16 384 keeps saturation
 *   out of the row.  m > 1 is what `mash sketch -r -m` is for -- a sequencing error makes k new k-mers, each seen once, and the
 *   smallest hashes of a read set are mostly those -- but exact: the copies are counted, not estimated by a Bloom filter.
 *   On the device a bottom sample is a sample as above that always keeps counts, and a THRESHOLD T, the max_hash its feeds keep
 *   under: 2^64 - 1 at first, and it only comes down.  The resident set holds EVERY value <= T seen so far with its exact count,
 *   qualifying or not.  A CUT follows a fold (resident sorted and distinct, nothing pending): entry j weighs 0 when its count is
 *   below m, else 1 (distinct) or min(count, S) (multiset); j* is the first entry at which the running sum of the weights reaches S;
 *   when there is one, T becomes values[j*] and the resident set ends behind j* -- a truncation, nothing moves.  This is exact: S
 *   sketch elements lie at or below the new T already, counts only grow, so the final row ends at or below T, and every value <= T
 *   keeps its exact count because every later window <= T is still kept.  The kernels (rk_bottom.hip): k_cut_weights sums the
 *   weights of every 1 024 entries, k_scan_blocks scans the sums, k_cut_find scans inside the one block that crosses S and stores
 *   (j* + 1, values[j*], the weight up to j*); the host reads those 24 bytes.  A sample folds and cuts after its first feed and then
 *   whenever more values wait than are resident (and where a scaled sample would fold); the fold inside a batch that is run again does
 *   not cut.  The row never depends on any of this, nor on batch boundaries, feed order or pending_cap.
 *   MEMORY: while fewer than S values qualify, every value is a candidate and stays.  At m = 1 that ends with the first feed (a
 *   sample that has not cut yet takes a large batch as sub-batches of 4 096, 8 192, ... reads, so T is down before most of it is
 *   hashed).  At m >= 2 a file of low coverage, where few k-mers repeat, keeps EVERY distinct k-mer with its count: 12 bytes each,
 *   twice (two array pairs), until RK_ERR_LIMIT (2^40 values) or the allocation's RK_ERR_NOMEM.
 * rk_sample_create_bottom: an rk_sample; rk_sample_add_batch, rk_sample_add_batch_device, rk_fastq_slot_sample, rk_sample_stats,
 *   rk_sample_reset (T back to 2^64 - 1) and rk_sample_destroy work on it unchanged.  Refuses what rk_sample_create refuses, and a
 *   sketch_size or min_copies outside its range (RK_ERR_ARG), before anything is launched.
 * rk_sample_finish_bottom: folds, cuts, downloads the resident set and writes row[sketch_size] (zero padded) and *len with
 *   rk_bottom_emit; the sample stays usable.  RK_ERR_ARG on a scaled sample.
 * rk_sample_finish / rk_sample_device on a bottom sample give its STATE, the resident candidates: every value <= T fed so far, with
 *   its count (T: rk_sample_bottom_state after the call).  rk_sample_add_sketch on a bottom sample is RK_ERR_ARG: uniting two bottom
 *   samples needs the smaller of two thresholds.
 * rk_sample_bottom_state: T, the resident candidates after the latest fold, the weight of the resident set at the latest cut (below
 *   S: no cut yet; it is not kept up to date between cuts) and the number of cuts that lowered T.  Any pointer may be NULL.  RK_ERR_ARG
 *   on a scaled sample.  (rk_sample_stats_t is as it was.)
 * rk_bottom_cut: the cut on host arrays -- values ascending and distinct, counts parallel --: uploads them, runs the three kernels;
 *   *cut_len = j* + 1 and *threshold = values[j*], or *cut_len = 0 (and *threshold = 0): no cut.  Arrays that do not ascend give a
 *   meaningless cut and nothing worse.  RK_ERR_ARG for NULL, sketch_size outside 1 .. RK_MAX_SKETCH, min_copies outside 1 .. 2^32 - 1;
 *   RK_ERR_LIMIT for n >= 2^31 * 1 024; all before anything is launched.
 * rk_bottom_emit (host code, usable without a GPU; rk_bottom_host.cpp): the row of a sorted distinct (values, counts) set under the
 *   definition above; RK_ERR_ARG when the values do not ascend, or one is 0. */
int rk_sample_create_bottom(rk_ctx* ctx, const int* ks, int nks, int sketch_size, uint64_t min_copies, uint64_t pending_cap, rk_sample** out);
int rk_sample_finish_bottom(rk_sample* sample, uint64_t* row, int32_t* len);
int rk_sample_bottom_state(rk_sample* sample, uint64_t* threshold, uint64_t* candidates, uint64_t* qualifying_weight, uint32_t* cuts);
int rk_bottom_cut(rk_ctx* ctx, const uint64_t* values, const uint32_t* counts, uint64_t n, int sketch_size, uint64_t min_copies, int distinct,
                  uint64_t* cut_len, uint64_t* threshold);
int rk_bottom_emit(const uint64_t* values, const uint32_t* counts, uint64_t n, int sketch_size, uint64_t min_copies, int distinct, uint64_t* row,
                   int32_t* len);

/* ------------------------------------------------------------------------------------------------
 * CLUSTER (`rkmh cluster`; what the sourmash family does with pairwise + cluster: the single-linkage clusters of a collection of
 * scaled sketches at a similarity threshold).  These are this library's own definitions.
 *   Inputs: n sketches with lengths len[i] < 2^31; a list of hits rk_search_hit {query, ref, shared} over those n sketches (SEARCH); a
 *   measure and a threshold min_ppm in parts per million, 0 .. 1 000 000.
 *   A hit LINKS i = query and j = ref when 0 <= i, j < n, i != j, shared >= 1 and
 *       shared * 1000000 >= min_ppm * denom,   denom = len[i] + len[j] - shared  (RK_CLUSTER_JACCARD)
 *                                              denom = min(len[i], len[j])       (RK_CLUSTER_MAX_CONTAINMENT)
 *   evaluated exactly in signed 64-bit integers (shared * 10^6 < 2^51, |min_ppm * denom| < 2^53: nothing wraps), so host and device
 *   agree bit for bit -- floating point, host only.  A hit whose shared exceeds what the lengths allow is no error: it is judged by
 *   the formula as written (a denom of 0 or below links).
 *   The graph is undirected: one direction of a pair is enough; duplicate hits, self hits and hits naming an index outside [0, n) change
 *   nothing.  Answer: int32 labels[n], labels[i] = the smallest index in the connected component of i.  It follows that
 *   labels[labels[i]] == labels[i] <= i; that the answer depends neither on the order nor on the multiplicity of the hits; that with no
 *   linking hit labels[i] = i; that at min_ppm = 0 every hit with shared >= 1 links; and that at min_ppm = 1 000 000 under Jaccard only
 *   identical sets link.
 * rk_cluster_hits_host: host code, usable without a GPU (rk_cluster_host.cpp): union-find over the linking hits.  lens: n uint64.
 * rk_cluster_hits: the same host arrays; uploads them (the lengths as CSR offsets), runs the device path, downloads the labels.
 * rk_cluster_hits_device: resident hits (nhits of 12 bytes; may be NULL when nhits = 0) and the collection's CSR offsets (n + 1
 * uint64): the length of sketch i is that of row i clamped to [0, nvalues], as every kernel of the layer takes it.  d_labels takes n
 * int32.  It runs on hip_stream and SYNCHRONISES it, as rk_gather_scaled_device does: every round ends with a look at a 4-byte word.
 * *rounds = the number of hook launches (the pointer may be NULL).  Every index is checked before it is used.
 * rk_cluster_scaled: host CSR arrays of the collection the index was made from (nref = the index's); searches the collection against
 * its own index at min_shared and clusters it; the hits never leave the device.  Never more than hit_cap hits are held (0: the
 * library's default, RK_CLUSTER_HIT_CAP; any other value is taken as given, down to 1): the queries go through in blocks of at most
 * (2^24 - 1) / (reference blocks) queries, the search's workgroup limit; the counting pass gives a block's total, a block that does not
 * fit is halved, down to a single query, and a single query with more hits than hit_cap is emitted and clustered in pieces of hit_cap
 * hits.  Each block (each piece) is hooked to its fixpoint before its hits are dropped: sound because a tree never splits (below), so
 * two sketches once under one root stay under one root.  The work buffers are the index's own, under its mutex, as the search's are.
 * rk_cluster_scaled_device: the same on resident d_values / d_offsets (nvalues uint64 behind d_values); d_labels takes nref int32;
 * runs on hip_stream and SYNCHRONISES it.
 * All entries refuse (RK_ERR_ARG, a size beyond its limit RK_ERR_LIMIT) before anything is launched: NULL, n < 1, n > 2^31 - 1, a
 * measure outside the two defined, min_ppm > 1 000 000, min_shared < 1, an index of another context or of another number of sketches;
 * host arrays only: a length of 2^31 or more, offsets that decrease.
 * rk_cluster_members: host only.  *ncl = the number of clusters; cl_off[0 .. ncl] and members[n]: the clusters ordered by their
 * smallest member, members ascending inside a cluster (cluster c = members[cl_off[c], cl_off[c + 1])); rep[c] = its member with the
 * largest len, among equal lengths the lowest index.  cl_off takes n + 1, members and rep n int32.  RK_ERR_ARG for labels that do not
 * satisfy labels[labels[i]] == labels[i] <= i.
 * The kernels (rk_cluster.hip): hook and compress on parent[n].  k_cluster_init: parent[i] = i.  k_cluster_hook: lanes stride the hits
 * under a grid cap; each applies the link test, reads pu = parent[u], pv = parent[v] and, when they differ,
 * atomicMin(&parent[max(pu, pv)], min(pu, pv)) and marks the round as changed.  k_cluster_compress: every node follows parent[] to
 * its root and stores it.  The loop: hook; while the hook changed something: compress, hook.  Why this is right:
 *   - parent[i] <= i always, and a parent value only decreases: init, atomicMin with a smaller value, compress to an ancestor.
 *   - Before every hook every tree is a star (init; compress).  A hook therefore writes only to nodes that were roots when it began,
 *     and only roots of that moment as values; a changed round makes at least one of those roots a non-root: the loop ends.
 *   - A hook that changes nothing found pu == pv for every linking hit, exactly (the launch before it is complete): both ends of every
 *     linking hit are under one root.  Links are only made between the ends of linking hits, so a tree lies inside one component:
 *     at the fixpoint trees and components are the same sets.  A root is the minimum of its tree (parent[i] <= i), so the label is
 *     the component's smallest index.
 *   - An atomicMin that overrides an earlier link of the same round (a hung under c, then under b < c) loses that link for now; the
 *     hit that made it is looked at again in the next round, which the override has marked as changed.
 *   - Trees never split: the star under a root a stays under a, whatever a is hung under.  The trees after a round are unions of the
 *     trees before it; that is what lets rk_cluster_scaled drop a block's hits once they are at their fixpoint.
 *   Integer atomics on global memory are device scope and commute (the precedent: k_mg_remove); which of two links wins is not fixed,
 *   the fixpoint is.  Plain reads of parent[] inside a launch may be stale on a part with several L2s; harmless: in a hook the
 *   non-roots are not written and a root's stale value is the root itself, still in the tree and a root when the launch began; in a
 *   compress an older parent is still an ancestor and roots are not written; launch boundaries make the writes of the launch before
 *   visible. */
#define RK_CLUSTER_JACCARD 0
#define RK_CLUSTER_MAX_CONTAINMENT 1
#define RK_CLUSTER_HIT_CAP (1ull << 25) /* hits held at once by rk_cluster_scaled when hit_cap = 0: 384 MB */
int rk_cluster_hits_host(const rk_search_hit* hits, uint64_t nhits, const uint64_t* lens, int64_t n, int measure, uint32_t min_ppm, int32_t* labels);
int rk_cluster_hits(rk_ctx* ctx, const rk_search_hit* hits, uint64_t nhits, const uint64_t* lens, int64_t n, int measure, uint32_t min_ppm,
                    int32_t* labels);
int rk_cluster_hits_device(rk_ctx* ctx, const void* d_hits, uint64_t nhits, const void* d_offsets, int64_t n, uint64_t nvalues, int measure,
                           uint32_t min_ppm, void* d_labels, uint32_t* rounds, void* hip_stream);
int rk_cluster_scaled(rk_ctx* ctx, rk_scaled_index* idx, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, int min_shared,
                      int measure, uint32_t min_ppm, uint64_t hit_cap, int32_t* labels);
int rk_cluster_scaled_device(rk_ctx* ctx, rk_scaled_index* idx, const void* d_values, const void* d_offsets, int64_t nref, uint64_t nvalues,
                             int min_shared, int measure, uint32_t min_ppm, uint64_t hit_cap, void* d_labels, void* hip_stream);
int rk_cluster_members(const int32_t* labels, const uint64_t* lens, int64_t n, int64_t* ncl, int32_t* cl_off, int32_t* members, int32_t* rep);

/* ------------------------------------------------------------------------------------------------
 * SCREEN (`rkmh screen`; what Mash calls screen: which reference sketches are CONTAINED in a read set -- a metagenome, a mixed
 * sample -- rather than how similar the whole set is to each).  These are this library's own definitions.
 *   Inputs: nref reference rows in CSR (uint64 values[], uint64 offsets[nref + 1]); every row ascending and non-zero; REPEATS INSIDE A
 *   ROW ARE ALLOWED (multiset policies write them); rows may be empty.  R_r is the set of distinct values of row r, len_r = |R_r|: the
 *   collapsed row.  The bottom-s rows of rk_sketch_batch / `rkmh sketch -s` / Mash are the intended input; any such rows work.
 *   W is the multiset of the non-zero window hashes of every sequence fed: windows, the pooled k list, the policy and invalid bases
 *   exactly as SAMPLE SKETCHES define them.  c(v) is the multiplicity of v in W, REPORTED as min(c, 2^32 - 1); counts injected with
 *   rk_screen_add_counts add to it.  min_copies m is 1 .. 2^32 - 1; v is PRESENT when the reported c(v) >= m.
 *   Per reference r, four uint32 at out4[r * 4]:
 *     shared   #{v in R_r : v present}
 *     median   the lower median of the reported c(v) over the present v in R_r: the element at index (shared - 1) / 2 in ascending
 *              order; 0 when shared = 0
 *     wshared, wmedian   the same two numbers over the present v in R_r whose OWNER is r
 *   owner(v) is the reference in v's posting list (the references whose R holds v) with the largest shared_r / len_r, compared as
 *   shared_a * len_b > shared_b * len_a in unsigned 64-bit (both factors are below 2^31: nothing wraps); among equal ratios the lowest
 *   reference index.  This is Mash's one-pass winner-takes-all.
 *   It follows that wshared_r <= shared_r; that the wshared of all references sum to the number of present keys; that the reference
 *   with the best ratio (lowest index among equals) has wshared = shared; that for pairwise disjoint rows w* = *; that of a reference
 *   given twice the second copy has wshared = 0; that feeding a read set twice doubles every count; and that batch boundaries, feed
 *   order and grid size never reach the result.
 *   IDENTITY is host arithmetic, floating point only: (shared / len)^(1 / k); 0 when shared = 0 (or len = 0), 1 when shared = len.
 *   There is no p-value: Mash's needs genome-size and k-mer-space assumptions that this library has no pinned definition for.
 *   On the device a screen is the inverted index of SEARCH over the collapsed rows (keys, post_off, post), pos[] -- where every value
 *   of a collapsed row stands in keys --, uint64 counts[nkeys] and a DIRECTORY over the leading bits below the largest key (about two
 *   buckets per key, 16 .. 2^24 buckets, chosen from nkeys at create): memory is O(reference values), whatever is fed.
 *   The kernels (rk_screen.hip).  k_screen_count walks the windows of a resident batch exactly as k_sample_keep does (the walk is one
 *   piece of device code, rk_tile_walk.hpp); a hash above the largest key is rejected, any other is looked up -- one directory read,
 *   then a search among the few keys of that bucket -- and a match adds 1 to counts[position]: ONE 64-BIT atomicAdd ON GLOBAL MEMORY,
 *   its result unused.  Integer adds commute (the precedent: k_mg_remove, k_cluster_hook), so the counts never depend on the order of
 *   arrival; 64-bit counters cannot overflow, so there is no saturation logic: the clamp to 2^32 - 1 happens where counts are read.
 *   Lanes of a wave that hit the same key are not combined.  There is no staging array, no cursor and no look from the host: a feed of
 *   resident bases is asynchronous.  k_screen_rows<plain>: one wave per reference strides pos[] of the row, loads and clamps the
 *   counts; shared from ballot popcounts, the median by bisection on the VALUE (at most 32 passes of "how many qualifying counts are
 *   <= mid": no sort, no LDS array).  k_screen_owner: one lane per present key (one wave for posting lists of 64 entries or more)
 *   picks the owner by the rule above from the shared of the first run, 2^32 - 1 for a key that is not present.  k_screen_rows<owned>
 *   runs again with the test owner == r.  Every index is checked before it is used.
 * rk_screen_create: collapses the rows on the host, builds the index (rk_scaled_index_create), pos[] and the directory, zeroes the
 *   counts.  Refuses before anything is launched: NULL, nks outside 1 .. RK_MAX_KS, a k outside 1 .. RK_MAX_K, nref < 1 (RK_ERR_ARG);
 *   offsets that decrease, a row that descends or holds 0 (RK_ERR_ARG); nref > 2^31 - 1, a row of 2^31 values or more, more than
 *   2^32 - 1 collapsed values (RK_ERR_LIMIT).  The screen uses the policy its context has at each feed and is used with that context
 *   only; destroy it before the context.
 * rk_screen_add_batch: host arrays as for rk_sample_add_batch, the same refusals, uploaded in pieces of about 64 MB of whole
 *   sequences on the context's stream; synchronises it.
 * rk_screen_add_batch_device: resident bases and uint32 offsets[nseq + 1], the form rk_sample_add_batch_device takes; ASYNCHRONOUS
 *   on hip_stream (NULL = HIP's null stream): it needs no look at a cursor.  The other entries work on the context's stream: the
 *   caller orders them behind its own stream (synchronise it before rows, counts, stats or reset).  Offsets that do not ascend give
 *   meaningless counts and no store outside the screen's arrays.
 * rk_fastq_slot_screen: rk_fastq_slot_sample's steps on a block of raw FASTQ text, then the feed from the slot's packed bases, on
 *   the slot's stream, which it synchronises.  *status != 0: the block is not four lines per record and NOTHING of it was added.
 *   RK_ERR_ARG for a screen of another context.
 * rk_screen_add_counts: adds counts[i] to c(values[i]) for ascending, distinct, non-zero values (RK_ERR_ARG otherwise); values that
 *   are no key are ignored.  The route for abundance sketches made elsewhere (rk_sample_finish), and to counts of 2^32 and beyond.
 * rk_screen_rows: out4 takes nref * 4 uint32.  rk_screen_rows_device: d_out4 the same on the device; launches rows, owner, rows on
 *   hip_stream and does not synchronise it; calls on one screen share its owner array, so two of them must not be in flight at once.
 *   RK_ERR_ARG for min_copies outside 1 .. 2^32 - 1.  The screen stays usable.
 * rk_screen_counts: *keys_out (ascending) and *counts_out (the RAW 64-bit counts, not clamped), malloc'd (rk_free; never NULL on
 *   success), *nkeys their length.
 * rk_screen_stats: the caller sets out->struct_size as for rk_index_stats.  nkeys: distinct values of all rows; dir_buckets,
 *   dir_shift: the directory (bucket of h = h >> dir_shift); nseq, nbases: sequences and bases fed (a refused FASTQ block adds none);
 *   counted: windows that matched a key; injected: the sum of what rk_screen_add_counts was given, keys or not.
 * rk_screen_reset: every count and total back to 0, the arrays kept.  Calls on one screen take turns.
 * rk_screen_rows_host (host code, usable without a GPU; rk_screen_host.cpp): the definition on a counted set -- c_values ascending,
 *   distinct and non-zero, c_counts parallel (uint64, clamped as above; a count of 0 is allowed and is never present) -- with the
 *   checks of rk_screen_create on the rows and RK_ERR_ARG for a counted set that does not ascend.
 * rk_screen_identity (host code): RK_ERR_ARG for NULL, k < 1 or shared > len. */
typedef struct rk_screen rk_screen;
typedef struct rk_screen_stats_t { uint32_t struct_size, nref, dir_shift, dir_buckets; uint64_t nkeys, nseq, nbases, counted, injected; } rk_screen_stats_t;
int rk_screen_create(rk_ctx* ctx, const int* ks, int nks, const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, rk_screen** out);
void rk_screen_destroy(rk_screen* screen);
int rk_screen_reset(rk_screen* screen);
int rk_screen_stats(rk_screen* screen, rk_screen_stats_t* out);
int rk_screen_add_batch(rk_screen* screen, const uint8_t* bases, const uint64_t* offsets, int64_t nseq);
int rk_screen_add_batch_device(rk_screen* screen, const void* d_bases, const void* d_offsets_u32, int64_t nseq, void* hip_stream);
int rk_fastq_slot_screen(rk_fastq_slot* slot, uint64_t nbytes, rk_screen* screen, int32_t* status, int64_t* nrec);
int rk_screen_add_counts(rk_screen* screen, const uint64_t* values, const uint32_t* counts, uint64_t n);
int rk_screen_rows(rk_screen* screen, uint64_t min_copies, uint32_t* out4);
int rk_screen_rows_device(rk_screen* screen, uint64_t min_copies, void* d_out4, void* hip_stream);
int rk_screen_counts(rk_screen* screen, uint64_t** keys_out, uint64_t** counts_out, uint64_t* nkeys);
int rk_screen_rows_host(const uint64_t* r_values, const uint64_t* r_offsets, int64_t nref, const uint64_t* c_values, const uint64_t* c_counts,
                        uint64_t nc, uint64_t min_copies, uint32_t* out4);
int rk_screen_identity(uint64_t shared, uint64_t len, int k, double* identity);

#ifdef __cplusplus
}
#endif
#endif
