// rk_parse_blocks.cpp -- the block-parallel front end of the host read parser.
//
// kseq's grammar is inherently sequential (a quality string is read by count, '@' may be data), so the parallel path only accepts
// input on which that grammar provably coincides with the line-oriented one: every FASTQ record is exactly four lines (header, one
// sequence line of keeper bytes, a '+' line, a quality line of exactly as many bytes 33..127), every FASTA sequence line holds only
// keeper bytes.  A block is cut at validated record starts, the pieces are scanned by worker threads under those strict rules, and
// ANY deviation anywhere in the block hands the untouched block back to the sequential scanner (rk_parse.cpp) and disables this
// path for the rest of the file, so the result is always the one kseq_read (src/kseq.hpp:170-208) would produce.
#include "rk_parse_internal.hpp"

#include <algorithm>

using namespace rkparse;

namespace rkparse {

inline const unsigned char* find_nl(const unsigned char* p, const unsigned char* e) {
    return p < e ? (const unsigned char*)memchr(p, '\n', (size_t)(e - p)) : nullptr;
}

const unsigned char* find_record_start(const unsigned char* base, const unsigned char* from,
                                       const unsigned char* e, bool fastq) {
    const unsigned char* p = from;
    if (p > base && p[-1] != '\n') {
        const unsigned char* nl = find_nl(p, e);
        if (!nl) return nullptr;
        p = nl + 1;
    }
    while (p < e) {
        if (fastq) {
            if (*p == '@') {
                const unsigned char* l1 = find_nl(p, e);
                if (!l1) return nullptr;
                const unsigned char* l2 = find_nl(l1 + 1, e);
                if (!l2 || l2 + 1 >= e) return nullptr;
                if (l2[1] == '+') return p;
            }
        } else if (*p == '>') {
            return p;
        }
        const unsigned char* nl = find_nl(p, e);
        if (!nl) return nullptr;
        p = nl + 1;
    }
    return nullptr;
}

const unsigned char* find_last_record_start(const unsigned char* base, const unsigned char* e, bool fastq) {
    size_t win = 1u << 16;
    const size_t total = (size_t)(e - base);
    for (;;) {
        const unsigned char* from = total > win ? e - win : base + 1;
        const unsigned char* best = nullptr;
        const unsigned char* p = from;
        for (;;) {
            const unsigned char* q = find_record_start(base, p, e, fastq);
            if (!q) break;
            best = q;
            p = q + 1;
        }
        if (best && best > base) return best;
        if (win >= total) return nullptr;
        win *= 16;
    }
}

} // namespace rkparse

namespace {

// true when [p, e) are all keeper bytes (class 1)
inline bool all_keepers(const unsigned char* p, const unsigned char* e) {
    unsigned acc = 0; // arithmetic form of seqcls == 1 so the loop vectorises
    for (; p < e; ++p) {
        const unsigned c = *p;
        acc |= (unsigned)((c - 33u) > 93u) | (unsigned)(c == '>') | (unsigned)(c == '+') | (unsigned)(c == '@');
    }
    return acc == 0;
}
inline bool all_quals(const unsigned char* p, const unsigned char* e) {
    unsigned acc = 0;
    for (; p < e; ++p) acc |= (unsigned)((unsigned)(*p - 33u) > 94u);
    return acc == 0;
}

inline bool push_name(Piece& o, const unsigned char* p, const unsigned char* nl) {
    const unsigned char* q = p;
    while (q < nl && !T.space[*q]) ++q;
    if (!o.names.append((const char*)p, (size_t)(q - p)) || !o.names.push('\0')) return false;
    return o.name_ends.push((uint64_t)o.names.n);
}

void parse_fastq_piece(const unsigned char* p, const unsigned char* e, bool want_quals, Piece& o) {
    while (p < e) {
        while (p < e && (*p == '\n' || *p == '\r')) ++p;
        if (p >= e) break;
        if (*p != '@') { o.bad = true; return; }
        ++p;
        const unsigned char* nl = find_nl(p, e);
        if (!nl) { o.bad = true; return; }
        if (!push_name(o, p, nl)) { o.oom = true; return; }
        p = nl + 1;
        nl = find_nl(p, e);
        if (!nl) { o.bad = true; return; }
        const unsigned char* se = nl;
        if (se > p && se[-1] == '\r') --se;
        const size_t slen = (size_t)(se - p);
        if (!all_keepers(p, se)) { o.bad = true; return; }
        if (!o.bases.append(p, slen) || !o.ends.push((uint64_t)o.bases.n)) { o.oom = true; return; }
        p = nl + 1;
        if (p >= e || *p != '+') { o.bad = true; return; }
        nl = find_nl(p, e);
        if (!nl) { o.bad = true; return; }
        p = nl + 1;
        nl = find_nl(p, e);
        const unsigned char* qe = nl ? nl : e;
        const unsigned char* qend = qe;
        if (qend > p && qend[-1] == '\r') --qend;
        if ((size_t)(qend - p) != slen || !all_quals(p, qend)) { o.bad = true; return; }
        if (want_quals && !o.quals.append((const char*)p, slen)) { o.oom = true; return; }
        p = nl ? nl + 1 : e;
    }
}

// FASTA piece [p, e).  A piece may begin INSIDE a record (cuts may fall anywhere outside a header line, so that a
// chromosome-sized record is shared by all workers): bases before the piece's first header line are its `lead`, the
// continuation of the record that was open when the piece began.  at_ls: p is the first byte of a line.  need_header:
// nothing is open yet (start of the file), so anything but blank lines before the first header is an irregularity.
void parse_fasta_piece(const unsigned char* p, const unsigned char* e, bool at_ls, bool need_header, Piece& o) {
    bool opened = false; // a header was seen in this piece
    o.lead = 0;
    while (p < e) {
        if (at_ls && *p == '>') {
            if (opened) { if (!o.ends.push((uint64_t)o.bases.n)) { o.oom = true; return; } }
            else o.lead = o.bases.n;
            ++p;
            const unsigned char* nl = find_nl(p, e);
            if (!nl) { o.bad = true; return; } // the file ends inside a header line: leave it to the sequential scanner
            if (!push_name(o, p, nl)) { o.oom = true; return; }
            p = nl + 1;
            opened = true;
            continue;
        }
        if (!opened && need_header) { // before the very first header only blank lines are regular
            if (*p == '\n' || *p == '\r') { at_ls = *p == '\n'; ++p; continue; }
            o.bad = true; return;
        }
        const unsigned char* nl = find_nl(p, e);
        const unsigned char* se = nl ? nl : e;
        if (nl && se > p && se[-1] == '\r') --se;
        if (!all_keepers(p, se)) { o.bad = true; return; }
        if (!o.bases.append(p, (size_t)(se - p))) { o.oom = true; return; }
        p = nl ? nl + 1 : e;
        at_ls = nl != nullptr;
    }
    if (opened) { if (!o.ends.push((uint64_t)o.bases.n)) { o.oom = true; return; } }
    else o.lead = o.bases.n;
}

// a legal FASTA cut at or before `pos`: anywhere except inside a header line (then the start of that line)
size_t fasta_cut(const unsigned char* base, size_t pos) {
    if (pos == 0) return 0;
    const unsigned char* nl = (const unsigned char*)memrchr(base, '\n', pos);
    const size_t ls = nl ? (size_t)(nl - base) + 1 : 0;
    return base[ls] == '>' ? ls : pos;
}

// f(0) on the caller, f(1) .. f(nt - 1) on threads of their own; returns when all are done
template <typename F> void run_on_workers(int nt, F f) {
    std::vector<std::thread> th;
    for (int i = 1; i < nt; ++i) th.emplace_back(f, i);
    f(0);
    for (auto& t : th) t.join();
}

// ---- the steps of next_block ----

// what step 1 decides
struct BlockCut {
    const unsigned char* base = nullptr; // the block's first byte
    size_t cut = 0;                      // how many of its bytes this call consumes: whole records, or with ...
    bool fastq = false;
    bool fasta_open = false;             // ... the open-record FASTA rules, anything that does not split a header line
};

// hands the input to the sequential scanner: -1.  Under open cuts from the first byte of the file, dropping what this file
// contributed so far
int irregular(rk_reader& r, Batch& b, bool open_cuts) {
    if (open_cuts) {
        b.rewind(r.par.file_start);
        r.par.map_pos = r.par.map_start;
        r.par.rec_open = false;
    }
    r.to_sequential();
    return -1;
}

// the next `target` bytes of the input (fewer at its end): of the mapping, or the pipe's block topped up to that size
struct BlockBytes { const unsigned char* base; size_t avail; bool at_eof; };
BlockBytes block_bytes(rk_reader& r, size_t target) {
    BlockState& s = r.par;
    if (s.map) {
        const size_t left = s.map_size - s.map_pos;
        return {s.map + s.map_pos, std::min(left, target), left <= target};
    }
    while (!s.blk_eof && s.blk.size() < target) {
        const size_t have = s.blk.size();
        size_t want = target - have;
        if (want > (1u << 30)) want = 1u << 30;
        s.blk.resize(have + want);
        const size_t got = r.src.pull(s.blk.data() + have, want);
        s.blk.resize(have + got);
        if (got < want) s.blk_eof = true;
    }
    return {s.blk.data(), s.blk.size(), s.blk_eof};
}

// Step 1: the block and its cut.  1 = chosen, 0 = end of input, -1 = irregular (handed over)
int choose_cut(rk_reader& r, Batch& b, int64_t max_records, bool open_cuts, BlockCut& c) {
    BlockState& s = r.par;
    size_t target = s.bytes_per_rec > 0 && max_records > 0 ? (size_t)(s.bytes_per_rec * (double)max_records) : (64u << 20);
    if (open_cuts) target = s.max_block;
    if (target < (4u << 20)) target = 4u << 20;
    if (target > s.max_block) target = s.max_block;
    for (;; target *= 2) { // (again with a larger block while no cut is found in it)
        const BlockBytes k = block_bytes(r, target);
        if (k.avail == 0) return 0;
        c.base = k.base;
        const unsigned char* e = k.base + k.avail;
        const unsigned char* p = k.base;
        while (p < e && (*p == '\n' || *p == '\r')) ++p;
        if (p >= e) { // blank lines only
            if (!k.at_eof) continue;
            if (s.map) s.map_pos = s.map_size; else s.blk.clear();
            return 0;
        }
        const bool resumed = open_cuts && s.rec_open; // continuing a FASTA file: the block may begin with sequence data
        if (!resumed && *p != '@' && *p != '>') return irregular(r, b, open_cuts);
        c.fastq = !resumed && *p == '@';
        c.fasta_open = resumed || (!c.fastq && open_cuts);
        if (k.at_eof) c.cut = k.avail;
        else if (c.fasta_open) c.cut = fasta_cut(k.base, k.avail); // 0: a header line longer than the block
        else {
            const unsigned char* last = find_last_record_start(k.base, e, c.fastq);
            c.cut = last ? (size_t)(last - k.base) : 0;           // 0: a single record longer than the block
        }
        if (c.cut > 0) return 1;
    }
}

// Step 2: piece i of nt is [starts[i], starts[i + 1]) of the cut, every boundary a legal cut itself
std::vector<size_t> split_cut(const BlockCut& c, int nt) {
    std::vector<size_t> starts((size_t)nt + 1);
    starts[0] = 0;
    starts[(size_t)nt] = c.cut;
    for (int i = 1; i < nt; ++i) {
        const size_t before = starts[(size_t)i - 1];
        const size_t from = std::max(c.cut / (size_t)nt * (size_t)i, before);
        if (c.fasta_open) { starts[(size_t)i] = std::max(fasta_cut(c.base, from), before); continue; }
        const unsigned char* q = find_record_start(c.base, c.base + from, c.base + c.cut, c.fastq);
        starts[(size_t)i] = q ? (size_t)(q - c.base) : c.cut;
    }
    return starts;
}

// Step 3: every worker scans its piece into r.par.pieces[i] under the strict rules
void scan_pieces(rk_reader& r, const BlockCut& c, const std::vector<size_t>& starts, bool want_quals) {
    BlockState& s = r.par;
    const int nt = (int)starts.size() - 1;
    if (s.pieces.size() < (size_t)nt) s.pieces.resize((size_t)nt);
    run_on_workers(nt, [&](int i) {
        Piece& pc = s.pieces[(size_t)i];
        pc.bases.n = pc.ends.n = pc.names.n = pc.name_ends.n = pc.quals.n = 0;
        pc.bad = pc.oom = false;
        const unsigned char* p = c.base + starts[(size_t)i];
        const unsigned char* e = c.base + starts[(size_t)i + 1];
        // upper bounds up front (untouched pages cost nothing): no geometric regrowth copies of 100 MB sequence lines
        const size_t span = (size_t)(e - p);
        if (!pc.bases.reserve(c.fastq ? span / 2 + 64 : span + 64) || (want_quals && !pc.quals.reserve(span / 2 + 64))) { pc.oom = true; return; }
        if (c.fastq) { parse_fastq_piece(p, e, want_quals, pc); return; }
        // (an open-record block lies in the mapping, so the byte in front of it can be read unless it begins the file)
        const bool at_ls = (p == c.base && (!c.fasta_open || s.map_pos == 0)) || p[-1] == '\n';
        parse_fasta_piece(p, e, at_ls, /*need_header=*/i == 0 && !(c.fasta_open && s.rec_open), pc);
        if (!c.fasta_open && pc.lead) pc.bad = true; // closed-cut blocks begin at a record start by construction
    });
}

// Step 4: the pieces' records appended to b -- prefix sums, then every worker copies its own piece into place.  1, -1 or -3 as
// next_block
int merge_pieces(rk_reader& r, Batch& b, const BlockCut& c, int nt, bool want_quals, bool open_cuts) {
    std::vector<Piece>& pieces = r.par.pieces;
    std::vector<size_t> rec0((size_t)nt + 1), base0((size_t)nt + 1), name0((size_t)nt + 1);
    rec0[0] = (size_t)b.nseq; base0[0] = b.bases.n; name0[0] = b.names.n;
    for (int i = 0; i < nt; ++i) {
        rec0[(size_t)i + 1] = rec0[(size_t)i] + pieces[(size_t)i].ends.n;
        base0[(size_t)i + 1] = base0[(size_t)i] + pieces[(size_t)i].bases.n;
        name0[(size_t)i + 1] = name0[(size_t)i] + pieces[(size_t)i].names.n;
    }
    const size_t nrec = rec0[(size_t)nt], nb = base0[(size_t)nt], nn = name0[(size_t)nt];
    const size_t q_before = b.quals.n;
    if (!b.bases.reserve(nb + 64) || !b.offsets.reserve(nrec + 1) || !b.names.reserve(nn + 1) ||
        !b.name_offsets.reserve(nrec + 1))
        return -3;
    if (want_quals && !b.quals.reserve(q_before + (nb - base0[0]) + 1)) return -3;
    run_on_workers(nt, [&](int i) {
        Piece& pc = pieces[(size_t)i];
        if (pc.bases.n) memcpy(b.bases.p + base0[(size_t)i], pc.bases.p, pc.bases.n);
        if (pc.names.n) memcpy(b.names.p + name0[(size_t)i], pc.names.p, pc.names.n);
        if (want_quals && pc.quals.n)
            memcpy(b.quals.p + q_before + (base0[(size_t)i] - base0[0]), pc.quals.p, pc.quals.n);
        uint64_t* off = b.offsets.p + rec0[(size_t)i] + 1;
        uint64_t* noff = b.name_offsets.p + rec0[(size_t)i] + 1;
        for (size_t j = 0; j < pc.ends.n; ++j) {
            off[j] = (uint64_t)base0[(size_t)i] + pc.ends.p[j];
            noff[j] = (uint64_t)name0[(size_t)i] + pc.name_ends.p[j];
        }
    });
    if (c.fasta_open) { // a piece's leading bases belong to the record that was open when the piece began
        for (int i = 0; i < nt; ++i) {
            const size_t lead = pieces[(size_t)i].lead;
            if (!lead) continue;
            if (rec0[(size_t)i] == 0) return irregular(r, b, open_cuts); // sequence data before any header (cannot happen: need_header)
            b.offsets.p[rec0[(size_t)i]] = (uint64_t)base0[(size_t)i] + lead;
        }
        if (nrec > 0) r.par.rec_open = true;
    }
    b.bases.n = nb; b.names.n = nn;
    b.offsets.n = nrec + 1; b.name_offsets.n = nrec + 1;
    if (want_quals) b.quals.n = q_before + (nb - base0[0]);
    const size_t got = nrec - (size_t)b.nseq;
    if (got && !want_quals) b.quals_ok = false;
    if (got) r.par.bytes_per_rec = (double)c.cut / (double)got;
    b.nseq = (int64_t)nrec;
    return 1;
}

// Step 5: the cut is done with; a pipe's block keeps its unfinished tail for the next call
void consume(BlockState& s, size_t cut) {
    if (s.map) { s.map_pos += cut; return; }
    const size_t tail = s.blk.size() - cut;
    if (tail) memmove(s.blk.data(), s.blk.data() + cut, tail);
    s.blk.resize(tail);
}

} // namespace

int rk_reader::next_block(Batch& b, int64_t max_records, bool open_cuts) {
    if (!par.map) open_cuts = false;
    if (open_cuts && !par.file_start_marked) { par.file_start_marked = true; par.file_start = b.mark(); }
    BlockCut c;
    const int chosen = choose_cut(*this, b, max_records, open_cuts, c);
    if (chosen != 1) return chosen;
    const int nt = c.cut < par.min_par ? 1 : nthreads;
    const std::vector<size_t> starts = split_cut(c, nt);
    const bool want_quals = c.fastq && b.quals_ok && !skip_quals;
    scan_pieces(*this, c, starts, want_quals);
    for (int i = 0; i < nt; ++i) {
        if (par.pieces[(size_t)i].oom) return -3;
        if (par.pieces[(size_t)i].bad) return irregular(*this, b, open_cuts);
    }
    const int merged = merge_pieces(*this, b, c, nt, want_quals, open_cuts);
    if (merged != 1) return merged;
    consume(par, c.cut);
    return 1;
}

extern "C" int64_t rk_fastq_cut(const uint8_t* text, uint64_t n) {
    if (!text || n < 2) return -1;
    const unsigned char* p = find_last_record_start(text, text + n, true);
    return p ? (int64_t)(p - text) : -1;
}
