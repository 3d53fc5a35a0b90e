// rk_bgzf.cpp -- BGZF (bgzip) input, host side: the member table, the host inflater and the FASTQ record cutter.
//
// The file is a chain of INDEPENDENT gzip members of at most 64 KB of text each, and every member's header says how long the member
// is ('BC' extra field) -- so, unlike plain gzip (one deflate stream that only a sequential reader can follow, src/rkmh.cpp:238-263
// through gzFile), the members can be found without inflating anything and inflated by as many threads as there are.  The device
// FASTQ front end's workers each inflate the members of their job straight in front of the upload (rkmh_rawreads.cpp,
// stream_files_raw); nothing in the process ever reads the file sequentially.
// Inflate = libdeflate when the system has it (dlopen: ~3 x zlib's rate per core), zlib otherwise; CRC-32 and ISIZE are checked.
#include "rk_parse_internal.hpp"

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

using namespace rkparse;

struct rk_bgzf {
    int fd = -1;
    const unsigned char* map = nullptr;
    size_t size = 0;
    std::vector<uint64_t> coff, uoff; // [members + 1] offset in the file / in the text
    std::vector<uint16_t> hlen;       // [members] header bytes (12 + XLEN)
};

namespace {
struct Deflate {
    void* h = nullptr;
    void* (*alloc)() = nullptr;
    int (*run)(void*, const void*, size_t, void*, size_t, size_t*) = nullptr;
    uint32_t (*crc)(uint32_t, const void*, size_t) = nullptr;
    Deflate() {
        if (getenv("RKMH_NO_LIBDEFLATE")) return;
        h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
        if (!h) return;
        alloc = (void* (*)())dlsym(h, "libdeflate_alloc_decompressor");
        run = (int (*)(void*, const void*, size_t, void*, size_t, size_t*))dlsym(h, "libdeflate_deflate_decompress");
        crc = (uint32_t (*)(uint32_t, const void*, size_t))dlsym(h, "libdeflate_crc32");
        if (!alloc || !run || !crc) { alloc = nullptr; run = nullptr; crc = nullptr; }
    }
};
const Deflate& deflate_lib() { static const Deflate d; return d; }

// one member's text into dst[0 .. usize); false: corrupt
bool inflate_member(const rk_bgzf* z, size_t b, unsigned char* dst) {
    const unsigned char* m = z->map + z->coff[b];
    const size_t total = (size_t)(z->coff[b + 1] - z->coff[b]), h = z->hlen[b], usize = (size_t)(z->uoff[b + 1] - z->uoff[b]);
    const unsigned char* payload = m + h;
    const size_t clen = total - h - 8;
    uint32_t want_crc;
    memcpy(&want_crc, m + total - 8, 4);
    const Deflate& L = deflate_lib();
    if (L.run) {
        static thread_local void* dec = L.alloc();
        size_t got = 0;
        if (!dec || L.run(dec, payload, clen, dst, usize, &got) != 0 || got != usize) return false;
        return L.crc(0, dst, usize) == want_crc;
    }
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<unsigned char*>(payload); zs.avail_in = (uInt)clen;
    zs.next_out = dst; zs.avail_out = (uInt)usize;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == usize;
    inflateEnd(&zs);
    return ok && (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, (uInt)usize) == want_crc;
}
} // namespace

extern "C" {

// RK_OK and *out = the opened file; RK_ERR_ARG: not a BGZF file (not an error to report: the caller takes another path)
int rk_bgzf_open(const char* path, rk_bgzf** out) {
    if (!path || !out) return perr(RK_ERR_ARG, "bad arguments");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return perr(RK_ERR_IO, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 28) { close(fd); return perr(RK_ERR_ARG, "not a BGZF file"); }
    void* mp = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_SHARED, fd, 0);
    if (mp == MAP_FAILED) { close(fd); return perr(RK_ERR_IO, std::string("cannot map ") + path); }
    rk_bgzf* z = new rk_bgzf();
    z->fd = fd; z->map = (const unsigned char*)mp; z->size = (size_t)st.st_size;
    size_t p = 0;
    uint64_t u = 0;
    bool ok = true;
    while (ok && p < z->size) {
        const unsigned char* m = z->map + p;
        if (z->size - p < 26 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || m[3] != 4) { ok = false; break; } // FLG = FEXTRA alone, as bgzip writes it
        const size_t xlen = (size_t)m[10] | ((size_t)m[11] << 8);
        if (12 + xlen + 8 > z->size - p) { ok = false; break; }
        size_t bsize = 0;
        for (size_t q = 12; q + 4 <= 12 + xlen;) {
            const size_t slen = (size_t)m[q + 2] | ((size_t)m[q + 3] << 8);
            if (m[q] == 'B' && m[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) bsize = ((size_t)m[q + 4] | ((size_t)m[q + 5] << 8)) + 1;
            q += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || bsize > z->size - p) { ok = false; break; }
        uint32_t isize;
        memcpy(&isize, m + bsize - 4, 4);
        if (isize > 65536) { ok = false; break; }
        z->coff.push_back(p); z->uoff.push_back(u); z->hlen.push_back((uint16_t)(12 + xlen));
        p += bsize; u += isize;
    }
    if (!ok || z->coff.empty()) { rk_bgzf_close(z); return perr(RK_ERR_ARG, "not a BGZF file"); }
    z->coff.push_back(p); z->uoff.push_back(u);
    madvise(mp, z->size, MADV_WILLNEED);
    *out = z;
    return RK_OK;
}
void rk_bgzf_close(rk_bgzf* z) {
    if (!z) return;
    if (z->map) munmap((void*)z->map, z->size);
    if (z->fd >= 0) close(z->fd);
    delete z;
}
int64_t rk_bgzf_members(const rk_bgzf* z) { return z ? (int64_t)z->hlen.size() : 0; }
// the file image and one member's place in it: bytes [*file_off, *file_off + *total) = header (*header bytes) + deflate stream + CRC-32 + ISIZE
const uint8_t* rk_bgzf_image(const rk_bgzf* z) { return z ? z->map : nullptr; }
uint64_t rk_bgzf_file_bytes(const rk_bgzf* z) { return z ? (uint64_t)z->size : 0; }
int rk_bgzf_member(const rk_bgzf* z, int64_t m, uint64_t* file_off, uint32_t* total, uint32_t* header, uint32_t* text_bytes) {
    if (!z || m < 0 || (size_t)m >= z->hlen.size()) return perr(RK_ERR_ARG, "bad arguments");
    if (file_off) *file_off = z->coff[(size_t)m];
    if (total) *total = (uint32_t)(z->coff[(size_t)m + 1] - z->coff[(size_t)m]);
    if (header) *header = z->hlen[(size_t)m];
    if (text_bytes) *text_bytes = (uint32_t)(z->uoff[(size_t)m + 1] - z->uoff[(size_t)m]);
    return RK_OK;
}
uint64_t rk_bgzf_text_bytes(const rk_bgzf* z) { return z ? z->uoff.back() : 0; }
uint64_t rk_bgzf_text_offset(const rk_bgzf* z, int64_t member) {
    if (!z || member < 0) return 0;
    return z->uoff[(size_t)std::min<int64_t>(member, (int64_t)z->hlen.size())];
}
// which inflater rk_bgzf_fastq_records runs in this process: "libdeflate" or "zlib".  libdeflate is the more lenient of the two: it
// accepts a code-length repeat that runs past HLIT + HDIST and bits that match no code of an incomplete one-code tree, and then
// delivers the text the member's CRC-32 and ISIZE vouch for, where zlib reports a corrupt member (tests/deflate_cases.py)
const char* rk_bgzf_inflater(void) { return deflate_lib().run ? "libdeflate" : "zlib"; }
// the text's first byte (0: empty or corrupt): '@' = FASTQ
int rk_bgzf_first_byte(const rk_bgzf* z) {
    if (!z) return 0;
    std::vector<unsigned char> t(65536);
    for (size_t b = 0; b < z->hlen.size(); ++b) {
        if (z->uoff[b + 1] == z->uoff[b]) continue;
        return inflate_member(z, b, t.data()) ? (int)t[0] : 0;
    }
    return 0;
}
// consecutive members grouped into jobs of about target_bytes of text: first[j] = first member of job j, first[jobs] = members
int64_t rk_bgzf_plan(const rk_bgzf* z, uint64_t target_bytes, int64_t* first, int64_t cap) { return rk_bgzf_plan_members(z, target_bytes, INT64_MAX, first, cap); }
// ... and of at most max_members members each (the device inflater decodes 64 members per wave: a job of 16 384 members is 256
// waves, two of which fill the chip -- one member more and a launch has a straggler that waits for the other launch's slots)
int64_t rk_bgzf_plan_members(const rk_bgzf* z, uint64_t target_bytes, int64_t max_members, int64_t* first, int64_t cap) {
    if (!z || !first || cap < 2 || max_members < 1) return perr(RK_ERR_ARG, "bad arguments");
    const size_t nb = z->hlen.size();
    int64_t nj = 0;
    size_t b = 0;
    while (b < nb) {
        if (nj + 1 >= cap) return perr(RK_ERR_LIMIT, "rk_bgzf_plan: more jobs than the caller's array holds");
        first[nj++] = (int64_t)b;
        const uint64_t start = z->uoff[b];
        const size_t b_first = b;
        while (b < nb && z->uoff[b + 1] - start <= target_bytes && (int64_t)(b - b_first) < max_members) ++b;
        if (b == b_first && b < nb) ++b; // (a member larger than the target: alone)
    }
    first[nj] = (int64_t)nb;
    return nj;
}
// The member that holds the byte in front of member b0's text: b0 - 1, unless that one is empty (the end-of-file marker `cat a.gz
// b.gz` leaves in the middle of a file) -- then the nearest one before it with text; b0 itself when no text precedes it.  Both
// record cutters (here and rk_inflate.hip's) begin their text there, so the cut at b0 sees the real previous byte and agrees with
// the cut the previous job made at its end.
int64_t rk_bgzf_lead_member(const rk_bgzf* z, int64_t b0) {
    if (!z || b0 <= 0) return 0;
    if ((size_t)b0 > z->hlen.size()) b0 = (int64_t)z->hlen.size();
    int64_t m = b0 - 1;
    while (m > 0 && z->uoff[(size_t)m + 1] == z->uoff[(size_t)m]) --m;
    return z->uoff[(size_t)m + 1] == z->uoff[(size_t)m] ? b0 : m;
}
// The whole FASTQ records that START in the text of members [b0, b1): the members are inflated (with the one in front, for its
// last byte, and as many behind as the last record reaches into), the first record start at or after the text of b0 and of b1
// is found by the four-line rule of find_record_start -- the same function at both ends, so neighbouring jobs agree -- and the
// bytes between them are copied to dst.  *text_off = where they begin in the uncompressed text.  Returns RK_OK, RK_ERR_IO
// (corrupt member), RK_ERR_LIMIT (more than cap bytes), or 1: the text does not begin with '@' (member 0 only).
int rk_bgzf_fastq_records(const rk_bgzf* z, int64_t b0, int64_t b1, uint8_t* dst, uint64_t cap, uint64_t* nbytes, uint64_t* text_off) {
    if (!z || !dst || !nbytes || b0 < 0 || b1 < b0 || (size_t)b1 > z->hlen.size()) return perr(RK_ERR_ARG, "bad arguments");
    *nbytes = 0;
    const size_t nb = z->hlen.size();
    const size_t lo = (size_t)rk_bgzf_lead_member(z, b0);
    static thread_local std::vector<unsigned char> buf;
    size_t have_b = lo; // members [lo, have_b) are in buf
    auto extend_to = [&](size_t upto) -> bool {
        if (upto > nb) upto = nb;
        const size_t need = (size_t)(z->uoff[upto] - z->uoff[lo]);
        if (buf.size() < need + 64) buf.resize(need + (need >> 2) + 65536);
        for (; have_b < upto; ++have_b)
            if (!inflate_member(z, have_b, buf.data() + (z->uoff[have_b] - z->uoff[lo]))) return false;
        return true;
    };
    if (!extend_to((size_t)b1)) return perr(RK_ERR_IO, "corrupt BGZF member");
    const uint64_t u_lo = z->uoff[lo];
    auto first_start = [&](size_t member, bool* need_more) -> size_t { // offset in buf; == text in buf when there is none
        *need_more = false;
        const unsigned char* base = buf.data();
        const unsigned char* e = base + (z->uoff[have_b] - u_lo);
        const unsigned char* from = base + (z->uoff[member] - u_lo);
        if (z->uoff[member] == 0) return 0; // (no text in front of it: the file's first record)
        if (from >= e) { *need_more = have_b < nb; return (size_t)(e - base); }
        const unsigned char* q = find_record_start(base, from, e, true);
        if (q) return (size_t)(q - base);
        *need_more = have_b < nb;
        return (size_t)(e - base);
    };
    bool more = false;
    size_t tail = first_start((size_t)b1, &more);
    for (size_t step = 2; more; step *= 2) { // the last record reaches into the members behind
        if (!extend_to(have_b + step)) return perr(RK_ERR_IO, "corrupt BGZF member");
        tail = first_start((size_t)b1, &more);
    }
    size_t head = first_start((size_t)b0, &more);
    if (head > tail) head = tail;
    if (z->uoff[(size_t)b0] == 0 && tail > 0 && buf[0] != '@') return 1; // (the job begins the file's text)
    const size_t n = tail - head;
    if (text_off) *text_off = u_lo + head;
    if (n > cap) return perr(RK_ERR_LIMIT, "rk_bgzf_fastq_records: the records of the job need more bytes than the buffer holds");
    memcpy(dst, buf.data() + head, n);
    *nbytes = n;
    return RK_OK;
}

} // extern "C"
