// rk_parse_internal.hpp -- what the sources of the host read parser share (nothing else includes this):
//   rk_pool.cpp          recycling of the big batch buffers
//   rk_parse.cpp         the reader: gzip source, sequential kseq scanner, the rk_reader_* entry points and rk_parse_files
//   rk_parse_blocks.cpp  the block-parallel front end: cut finders, piece scanners, rk_reader::next_block
//   rk_bgzf.cpp          BGZF input: member table, host inflater, record cutter
#pragma once
#include "../../include/rkmh_amd.h"

#include <sys/mman.h>
#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

extern "C" void rk__set_error(const char* msg); // rk_api.hip

namespace rkparse {

struct Tables {
    unsigned char seqcls[256] = {}; // 0 skip, 1 keep, 2 terminator
    unsigned char space[256] = {};
    constexpr Tables() {
        for (int c = 0; c < 256; ++c) {
            seqcls[c] = (c >= 33 && c <= 126) ? 1 : 0;
            space[c] = (c == ' ' || (c >= 9 && c <= 13)) ? 1 : 0;
        }
        seqcls['>'] = seqcls['+'] = seqcls['@'] = 2;
    }
};
inline constexpr Tables T{};

inline int perr(int code, const std::string& m) { rk__set_error(m.c_str()); return code; }

namespace pool { // rk_pool.cpp
void remember(void* p, size_t bytes);  // p is a buffer of `bytes` that is about to be handed to the caller
void forget(void* p);                  // p is about to be freed by someone else
void* take(size_t bytes, size_t* got); // a parked buffer of at least `bytes` (and at most 4x that), or nullptr
void give_back(void* p);               // parks p if it is one of ours and there is room; else frees it
} // namespace pool

template <typename V> struct Grow { // malloc-backed growable array handed over to C callers
    V* p = nullptr;
    size_t n = 0, cap = 0;
    // Owns p: movable, never copied.  (It used to have only the implicit, shallow copy: std::vector<Piece>::resize relocating live
    // pieces -- a later block using more workers than an earlier one -- left the new elements pointing at buffers the old ones had
    // freed, and the next reserve() was a double free.  Seen as a rare abort of the parser tests; found with AddressSanitizer.)
    Grow() = default;
    Grow(const Grow&) = delete;
    Grow& operator=(const Grow&) = delete;
    Grow(Grow&& o) noexcept : p(o.p), n(o.n), cap(o.cap) { o.p = nullptr; o.n = o.cap = 0; }
    Grow& operator=(Grow&& o) noexcept {
        if (this != &o) { free(p); p = o.p; n = o.n; cap = o.cap; o.p = nullptr; o.n = o.cap = 0; }
        return *this;
    }
    bool reserve(size_t want) {
        if (want <= cap) return true;
        if (!p) { // a parked batch buffer of the right size (rk_pool.cpp)
            size_t got = 0;
            if (void* q = pool::take(want * sizeof(V), &got)) { p = (V*)q; cap = got / sizeof(V); return true; }
        }
        size_t nc = cap ? cap : 1024;
        while (nc < want) nc += nc >> 1;
        V* q = (V*)realloc(p, nc * sizeof(V));
        if (!q) return false;
        p = q; cap = nc;
        return true;
    }
    bool push(V v) { if (n == cap && !reserve(n + 1)) return false; p[n++] = v; return true; }
    bool append(const V* s, size_t k) { if (k == 0) return true; if (!reserve(n + k)) return false; memcpy(p + n, s, k * sizeof(V)); n += k; return true; }
    V* release() { V* r = p; pool::remember(r, cap * sizeof(V)); p = nullptr; n = cap = 0; return r; }
    ~Grow() { free(p); }
};

struct Batch {
    Grow<uint8_t> bases;
    Grow<uint64_t> offsets;
    Grow<char> names;
    Grow<uint64_t> name_offsets;
    Grow<char> quals;
    bool quals_ok = true; // every record so far had a quality string
    int64_t nseq = 0;
    bool init() { return offsets.push(0) && name_offsets.push(0); }

    // Mark and rewind: what the batch held at some point, and dropping everything appended since (the buffers keep their capacity).
    // A record that was abandoned before it pushed its offsets is rewound the same way: only bases and names have moved then.
    struct Mark {
        int64_t nseq = 0;
        size_t bases = 0, offsets = 0, names = 0, quals = 0; // (name_offsets runs in step with offsets)
        bool quals_ok = true;
    };
    Mark mark() const { return Mark{nseq, bases.n, offsets.n, names.n, quals.n, quals_ok}; }
    void rewind(const Mark& m) {
        nseq = m.nseq; bases.n = m.bases; offsets.n = name_offsets.n = m.offsets; names.n = m.names; quals.n = m.quals;
        quals_ok = m.quals_ok;
    }
};

struct Piece { // what one worker of the block front end scanned
    Grow<uint8_t> bases;
    Grow<uint64_t> ends;      // cumulative base count after each record (piece-local)
    Grow<char> names;
    Grow<uint64_t> name_ends; // cumulative name bytes (with the NULs) after each record
    Grow<char> quals;
    size_t lead = 0;          // FASTA pieces that start inside a record: bases that continue the previous piece's last record
    bool bad = false, oom = false;
};

// rk_parse_blocks.cpp.  First record start at or after `from` (line-aligned); for FASTQ the line two below must begin with '+',
// which a quality line that happens to begin with '@' can never satisfy (its +2 line is a sequence line).
const unsigned char* find_record_start(const unsigned char* base, const unsigned char* from, const unsigned char* e, bool fastq);
// last record start in (base, e): records before it are complete inside the block
const unsigned char* find_last_record_start(const unsigned char* base, const unsigned char* e, bool fastq);

// Where the bytes come from when the file is not mapped: gzFile (plain text through a pipe or STDIN, or gzip).  Compressed input is one
// deflate stream that only a sequential reader can follow (src/rkmh.cpp:238-263), so with `threaded` set zlib inflates on its OWN
// thread, a few 8 MB chunks ahead, while the block scanner's threads parse what has arrived.
struct GzSource {
    gzFile fp = nullptr;
    bool threaded = false;
    size_t pull(unsigned char* dst, size_t want); // `want` bytes of the (inflated) input, fewer only at its end
    // a read that FAILED (gzread < 0: a corrupt or truncated gzip stream, an I/O error) -- not an end of input.  Set by whichever
    // thread reads (the inflater thread included), reported by rk_reader_next / rk_parse_files: the reference's kseq takes the
    // failed gzread for the end of the file and exits 0 with what it had (src/kseq.hpp:75-85); this build says so
    std::atomic<bool> io_failed{false};
    std::string read_error() { std::lock_guard<std::mutex> l(io_mu); return io_msg; }
    ~GzSource(); // stops and joins the inflater thread, closes the file

private:
    std::mutex io_mu;
    std::string io_msg;
    void check_read(int r, size_t want);
    struct Chunk { std::unique_ptr<unsigned char[]> p; size_t n = 0; }; // (not a vector: no zero fill of megabytes that gzread overwrites)
    std::thread th; // started by the first pull()
    std::mutex m;
    std::condition_variable cv;
    std::deque<Chunk> q;
    bool done = false, stop = false;
    Chunk cur;
    size_t cur_pos = 0;
    void inflate_ahead(); // the thread's body
};

// The sequential kseq scanner's position: its window of the input, and the bytes a fallback of the block front end left for it
struct SeqState {
    std::vector<unsigned char> buf;
    size_t beg = 0, end = 0;
    bool eof = false;
    int last_char = 0;
    const unsigned char* pend_ptr = nullptr; // after a fallback the scanner is fed from here first
    size_t pend_len = 0, pend_pos = 0;
    bool pending = false, pend_then_eof = false;
};

// The block front end's position (plain, well-formed files only; see rk_parse_blocks.cpp)
struct BlockState {
    const unsigned char* map = nullptr; // regular uncompressed file: the whole file, mmap'd
    size_t map_size = 0, map_pos = 0, map_start = 0; // map_start: where this reader began (rk_reader_open_at); map_size: where it ends
    size_t map_total = 0;                            // bytes really mapped (rk_reader_open_range reads a part of the file)
    std::vector<unsigned char> blk;     // pipes: current block; starts with the tail of the previous one
    bool blk_eof = false;
    double bytes_per_rec = 0;
    size_t max_block = 384u << 20; // RKMH_PARSE_BLOCK_KB
    size_t min_par = 1u << 20;     // blocks smaller than this are scanned by one thread
    std::vector<Piece> pieces;     // per-worker scratch, reused across blocks
    bool rec_open = false;         // a FASTA header has been seen: a block / piece may begin with sequence data of that record
    // open-cut parsing restarts the file from byte 0 with the sequential scanner on any irregularity (a block may have begun
    // inside a record, which the sequential scanner cannot resume): the batch as it was at the start of the file
    bool file_start_marked = false;
    Batch::Mark file_start;
    ~BlockState() { if (map) munmap((void*)map, map_total); }
};

} // namespace rkparse

struct rk_reader {
    rkparse::GzSource src;
    rkparse::SeqState seq;
    rkparse::BlockState par;
    bool par_ok = false;        // still in block-parallel mode
    bool was_irregular = false; // the block-parallel front end handed the input to the sequential scanner
    bool skip_quals = false;    // RK_READER_NO_QUALS
    bool finished = false;
    int nthreads = 1;

    // rk_parse.cpp
    void to_sequential();
    bool fill();
    int getc() { return seq.beg >= seq.end && !fill() ? -1 : seq.buf[seq.beg++]; }
    int next(rkparse::Batch& b); // one record appended to b: 1 record read, 0 clean EOF, -2 truncated, -3 out of memory

    // rk_parse_blocks.cpp.  Appends the records of the next block to b: 1 = block consumed (more may follow), 0 = end of input,
    // -1 = input is not strictly line-structured: the block was handed back to the sequential scanner, -3 = out of memory.
    // open_cuts (whole-file parsing of a mapped file into ONE batch): FASTA blocks and pieces may end inside a record
    int next_block(rkparse::Batch& b, int64_t max_records, bool open_cuts = false);
};
