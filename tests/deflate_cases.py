"""A DEFLATE *writer* (RFC 1951) and a catalogue of streams that zlib's encoder never produces -- test infrastructure for the device
inflater (rk_inflate.hip, rk_gunzip.hip).  Every compressed byte the older inflate tests feed the decoder was written by zlib; the
cases here are written bit by bit instead, so that a case can force a repeat code across the literal/length | distance boundary, a
code 16 behind an 18, exactly 128 long-coded symbols, a literal run of exactly 255 between two matches, and so on.

What is adversarial is the ENCODING (and the bytes 128..255 inside names and comments); the text of every legal case is valid FASTQ
(or FASTA), because the device route is reached through the record loaders.  zlib's *decoder* is the arbiter of what is legal
(tests/test_deflate_cases_cpu.py): it is what the reference's gzopen runs.

A case is a Case(name, containers, text, expectation, facts):
  containers   {"bgzf": file image or None, "gzip": file image or None}; raws = the raw deflate streams with their texts
  expectation  "device"   the device route must take it (status 0);
               "handover" the job is the host's by a limit the source names (more than LONG_CAP literal/length symbols with codes
                          longer than the 8-bit root, rk_inflate.hip: LONG_CAP);
               "refused"  structurally invalid: zlib raises, the device returns 1 and the host route reports an error.
               It is decided from `facts` and the limits below, never from what the device did.
  facts        what the writer saw while it wrote: blocks by type, longest code, long-coded symbols, whether a repeat crossed the
               boundary, largest distance, literal runs, entries per member (as pass 1 counts them) ...
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

# limits of the device decoder, as rk_inflate.hip names them
LT, DT = 8, 6                 # root table bits (k_inflate_lanes<8, 6>)
LONG_CAP = 128                # literal/length symbols with codes longer than LT bits; more: the member is the host's
DLONG_CAP = 32                # distance symbols with codes longer than DT bits (an alphabet of 30 never exceeds it)
MEMBER_TEXT_MAX = 65536       # WIN_BYTES

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

Case = namedtuple("Case", "name containers text expectation facts raws kind")


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        """n bits of value, least significant first (header fields, extra bits)"""
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: most significant bit first"""
        self.bits(int(format(code & ((1 << n) - 1), "0%db" % n)[::-1], 2) if n else 0, n)   # (an over-subscribed code of a refused case: its low bits)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def pos(self):
        return 8 * len(self.out) + self.n

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """codes of a canonical Huffman code from its lengths (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        nxt[l] += 1 if l else 0
    return codes


def kraft(lens, unit=15):
    return sum(1 << (unit - l) for l in lens if l)


def complete_lengths(n, n_long, root, maxbits=15):
    """the multiset of lengths (ascending) of a COMPLETE code of n symbols of which exactly n_long are longer than `root` bits"""
    n_short = n - n_long
    if n_long == 0:
        long_part, k_long2 = [], 0
    else:
        # a symbols of root + 1 bits and, when n_long is odd, two of root + 2: the long part is a whole number of 2^-root
        if n_long % 2 == 0:
            long_part = [root + 1] * n_long
        else:
            assert n_long >= 3
            long_part = [root + 1] * (n_long - 2) + [root + 2] * 2
        k_long2 = kraft(long_part, root + 2)
        assert k_long2 % 4 == 0
    units = (1 << root) - k_long2 // 4           # what the short symbols have to fill, in 2^-root
    assert units >= 0
    short = [root - b for b in range(root + 1) if (units >> b) & 1]      # the binary representation: one symbol per set bit
    assert len(short) <= n_short <= units, (len(short), n_short, units)
    while len(short) < n_short:                  # split the shortest code that can still be split
        short.sort()
        i = next(i for i, l in enumerate(short) if l < root)
        l = short.pop(i)
        short += [l + 1, l + 1]
    out = sorted(short + long_part)
    assert kraft(out) == 1 << 15 and max(out) <= maxbits and sum(1 for l in out if l > root) == n_long
    return out


def assign_lengths(nsym, sorted_lens, order):
    """sorted_lens (ascending) handed to the symbols in `order` (most wanted first); the others get no code"""
    lens = [0] * nsym
    for s, l in zip(order, sorted_lens):
        lens[s] = l
    return lens


def huffman_lengths(freq, maxbits):
    """a complete length-limited code for the symbols with freq > 0 (at least two symbols get a code)"""
    import heapq
    n = len(freq)
    freq = list(freq)
    used = [s for s in range(n) if freq[s]]
    for s in range(n):
        if len(used) >= 2:
            break
        if not freq[s]:
            freq[s] = 1
            used.append(s)
    while True:
        heap = [(freq[s], s, (s,)) for s in used]
        heapq.heapify(heap)
        lens = [0] * n
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                lens[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        if max(lens) <= maxbits:
            return lens
        freq = [(f + 1) // 2 if f else 0 for f in freq]


def len_symbol(length):
    if length == 258:
        return 28
    return max(i for i in range(28) if LEN_BASE[i] <= length)


def dist_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def rle(seq, zero16=False):
    """code-length symbols for the sequence of lengths: greedy repeats over the WHOLE sequence (literal/length and distance lengths
    as one run of numbers -- so a run of equal lengths across the boundary becomes one repeat, as libdeflate and zopfli write it).
    zero16: the last three of a long run of zeros are sent as code 16 behind the 17/18 (a repeat of a zero)."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        r = j - i
        if v == 0:
            while r >= 3:
                if zero16 and r >= 6 and r - 3 <= 138:
                    out.append((18, r - 3) if r - 3 >= 11 else (17, r - 3))
                    out.append((16, 3))
                    r = 0
                    break
                k = min(r, 138)
                if r - k in (1, 2) and k > 13:
                    k -= 3 - (r - k) if k - (3 - (r - k)) >= 11 else 0
                out.append((18, k) if k >= 11 else (17, k))
                r -= k
            out += [0] * r
        else:
            out.append(v)
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, k))
                r -= k
            out += [v] * r
        i = j
    return out


def expand_cl(clseq):
    out = []
    for it in clseq:
        if isinstance(it, tuple):
            s, k = it
            assert (s == 16 and 3 <= k <= 6) or (s == 17 and 3 <= k <= 10) or (s == 18 and 11 <= k <= 138)
            out += [out[-1] if s == 16 else 0] * k
        else:
            out.append(it)
    return out


class Deflate:
    """one raw deflate stream under construction: blocks are queued and written by raw(), which marks the last one final.
    Tokens: an int is a literal byte, a tuple (length, distance) a match, ("len_sym", symbol, extra, distance) a match whose length
    is spelled with a given symbol (258 as 284 + 31), ("raw", bits, nbits) bits written as they are (refused cases)."""

    def __init__(self, check=True):
        self.blocks = []
        self.check = check

    def stored(self, data, nlen=None):
        self.blocks.append(("stored", bytes(data), nlen))

    def fixed(self, toks, eob=True):
        self.blocks.append(("fixed", list(toks), eob))

    def dynamic(self, toks, ll=None, dl=None, cl=None, hclen=None, zero16=False, eob=True, cl_lens=None, hlit=None, hdist=None):
        self.blocks.append(("dynamic", list(toks), ll, dl, cl, hclen, zero16, eob, cl_lens, hlit, hdist))

    def reserved(self):
        self.blocks.append(("reserved",))

    # -- writing
    def raw(self, final_last=True):
        w = BitWriter()
        f = dict(blocks={"stored": 0, "fixed": 0, "dynamic": 0}, empty_blocks={"stored": 0, "fixed": 0, "dynamic": 0}, longest_ll=0, longest_dl=0,
                 long_ll_max=0, long_dl_max=0, repeat_crossed=[], rep16_after_zero_run=0, rep16_after=[], dynamic_header_bits=[], max_dist=0, dist_syms=set(), lit_runs=[], entries=0, literals=0,
                 high_literals=0, len258=0, len258_as_284=0, stored_hdr_bit_offsets=set(), hlit=set(), hdist=set(), hclen=set(), first_block=None, final_block=None,
                 final_empty=False, incomplete_dist=0, no_dist_code=0, matches=[], out_len=0, final_dynamic_bits_from_end=None)
        self._f, self._run, self._op = f, 0, 0
        for i, b in enumerate(self.blocks):
            final = 1 if (final_last and i == len(self.blocks) - 1) else 0
            start = w.pos
            before = self._op
            w.bits(final, 1)
            kind = b[0]
            if kind == "reserved":
                w.bits(3, 2)
                continue
            f["blocks"][kind] += 1
            if i == 0:
                f["first_block"] = kind
            if kind == "stored":
                w.bits(0, 2)
                f["stored_hdr_bit_offsets"].add(w.pos & 7)
                w.align()
                data, nlen = b[1], b[2]
                w.bits(len(data), 16)
                w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
                for c in data:
                    w.bits(c, 8)
                    self._lit(c)
            elif kind == "fixed":
                w.bits(1, 2)
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                self._tokens(w, b[1], ll, canonical(ll), [5] * 32, canonical([5] * 32), b[2])
            else:
                w.bits(2, 2)
                f["dynamic_header_bits"].append(start)
                self._dynamic(w, *b[1:])
            if self._op == before:
                f["empty_blocks"][kind] += 1
            if final:
                f["final_block"], f["final_empty"] = kind, self._op == before
                self._final_start = start
        f["lit_runs"].append(self._run)       # the tail
        f["entries"] += 1
        f["out_len"] = self._op
        out = w.done()
        if f["final_block"] == "dynamic":
            f["final_dynamic_bits_from_end"] = 8 * len(out) - self._final_start
        self.facts = f
        return out

    def _lit(self, c):
        f = self._f
        f["literals"] += 1
        f["high_literals"] += c >= 128
        self._op += 1
        self._run += 1
        if self._run == 255:                      # pass 1: an entry of length 0 carries 255 literals of a longer run
            f["lit_runs"].append(255)
            f["entries"] += 1
            self._run = 0

    def _match(self, length, dist):
        f = self._f
        if self.check:
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= self._op, (length, dist, self._op)
        f["lit_runs"].append(self._run)
        f["entries"] += 1
        self._run = 0
        self._op += length
        f["max_dist"] = max(f["max_dist"], dist)
        f["len258"] += length == 258
        f["matches"].append((length, dist))

    def _tokens(self, w, toks, ll, lc, dl, dc, eob):
        f = self._f
        for t in toks:
            if isinstance(t, tuple) and t[0] == "raw":
                w.bits(t[1], t[2])
                continue
            if isinstance(t, tuple) and t[0] == "sym":          # a literal/length symbol as it is (286, 287 under the fixed code)
                w.code(lc[t[1]], ll[t[1]])
                continue
            if isinstance(t, tuple) and t[0] == "dist_sym":     # length 3, then a distance symbol as it is (30, 31)
                w.code(lc[257], ll[257])
                w.code(dc[t[1]], dl[t[1]])
                continue
            if not isinstance(t, tuple):
                assert ll[t], "literal %d has no code" % t
                w.code(lc[t], ll[t])
                self._lit(t)
                continue
            if t[0] == "len_sym":
                _, ls, extra, dist = t
                length = LEN_BASE[ls] + extra
                f["len258_as_284"] += (ls == 27 and extra == 31)
            else:
                length, dist = t
                ls = len_symbol(length)
                extra = length - LEN_BASE[ls]
            assert ll[257 + ls], "length symbol %d has no code" % (257 + ls)
            w.code(lc[257 + ls], ll[257 + ls])
            w.bits(extra, LEN_EXTRA[ls])
            ds = dist_symbol(min(dist, 32768))
            assert dl[ds], "distance symbol %d has no code" % ds
            w.code(dc[ds], dl[ds])
            w.bits(min(dist, 32768) - DIST_BASE[ds], DIST_EXTRA[ds])
            f["dist_syms"].add(ds)
            self._match(length, dist)
        if eob:
            w.code(lc[256], ll[256])

    def _dynamic(self, w, toks, ll, dl, cl, hclen, zero16, eob, cl_lens, hlit, hdist):
        f = self._f
        if ll is None or dl is None:
            fl, fd = [0] * 286, [0] * 30
            fl[256] = 1
            for t in toks:
                if not isinstance(t, tuple):
                    fl[t] += 1
                elif t[0] == "len_sym":
                    fl[257 + t[1]] += 1
                    fd[dist_symbol(t[3])] += 1
                elif isinstance(t[0], int):
                    fl[257 + len_symbol(t[0])] += 1
                    fd[dist_symbol(t[1])] += 1
            if ll is None:
                ll = huffman_lengths(fl, 15)
                while len(ll) > 257 and ll[-1] == 0:
                    ll.pop()
            if dl is None:
                dl = huffman_lengths(fd, 15)
                while len(dl) > 1 and dl[-1] == 0:
                    dl.pop()
        nlit, ndist = (len(ll), len(dl)) if hlit is None else (hlit, hdist)
        if cl is None:
            cl = rle(list(ll) + list(dl), zero16)
        seq = expand_cl(cl) if self.check else None
        if self.check:
            assert seq == list(ll) + list(dl), "the code-length symbols do not spell the lengths"
            assert 257 <= nlit <= 286 and 1 <= ndist <= 30
        # facts of the header
        at, prev_zero_rep = 0, False
        for it in cl:
            k = it[1] if isinstance(it, tuple) else 1
            if isinstance(it, tuple):
                if at < nlit < at + k:
                    f["repeat_crossed"].append(it[0])
                if it[0] == 16 and prev_zero_rep:
                    f["rep16_after_zero_run"] += 1
                    f["rep16_after"].append(prev_code)
            prev_zero_rep = isinstance(it, tuple) and (it[0] in (17, 18) or (it[0] == 16 and prev_zero_rep))
            prev_code = it[0] if isinstance(it, tuple) else it
            at += k
        f["hlit"].add(nlit); f["hdist"].add(ndist)
        f["longest_ll"] = max(f["longest_ll"], max(ll)); f["longest_dl"] = max(f["longest_dl"], max(dl))
        f["long_ll_max"] = max(f["long_ll_max"], sum(1 for l in ll if l > LT)); f["long_dl_max"] = max(f["long_dl_max"], sum(1 for l in dl if l > DT))
        if max(dl) == 0:
            f["no_dist_code"] += 1
        elif kraft(dl) < (1 << 15):
            f["incomplete_dist"] += 1
        # the code-length code
        if cl_lens is None:
            fc = [0] * 19
            for it in cl:
                fc[it[0] if isinstance(it, tuple) else it] += 1
            cl_lens = huffman_lengths(fc, 7)
        n = 19
        while n > 4 and cl_lens[CL_ORDER[n - 1]] == 0:
            n -= 1
        if hclen is not None:
            n = hclen
        f["hclen"].add(n)
        w.bits(nlit - 257, 5); w.bits(ndist - 1, 5); w.bits(n - 4, 4)
        for i in range(n):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canonical(cl_lens)
        for it in cl:
            s = it[0] if isinstance(it, tuple) else it
            w.code(cc[s], cl_lens[s])
            if isinstance(it, tuple):
                w.bits(it[1] - (3 if s < 18 else 11), 2 if s == 16 else (3 if s == 17 else 7))
        ll2, dl2 = list(ll) + [0] * (288 - len(ll)), list(dl) + [0] * (32 - len(dl))
        self._tokens(w, toks, ll2, canonical(ll2), dl2, canonical(dl2), eob)


# ---- texts ---------------------------------------------------------------------------------------------------------------------
def fastq(rng, n, lo=30, hi=200, high=False, tag=b"r"):
    """n records; high: bytes 128..255 in names and comments (kseq keeps them)"""
    recs = []
    for i in range(n):
        L = int(rng.integers(lo, hi))
        s = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=L, p=[0.3, 0.2, 0.2, 0.29, 0.01]))
        q = bytes(rng.integers(33, 75, size=L, dtype=np.uint8))
        name = tag + b"%d" % i
        if high:
            name += bytes(rng.integers(128, 256, size=int(rng.integers(1, 12)), dtype=np.uint8)) + b" c\xff\x80" + bytes(rng.integers(128, 256, size=6, dtype=np.uint8))
        recs.append(b"@" + name + b"\n" + s + b"\n+\n" + q + b"\n")
    return b"".join(recs)


def fastq_exact(rng, nbytes, high=False, tag=b"x"):
    """whole records, exactly nbytes of them"""
    out, i = [], 0
    left = nbytes
    while left > 700:
        r = fastq(rng, 1, 60, 200, high, tag + b"%d_" % i)
        out.append(r); left -= len(r); i += 1
    name = b"@" + tag + b"end" + (b"" if left % 2 == 0 else b"e")       # '@' name '\n' seq '\n+\n' qual '\n': 2 L + len(name) + 5
    L = (left - len(name) - 5) // 2
    assert L > 0 and 2 * L + len(name) + 5 == left
    s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L))
    out.append(name + b"\n" + s + b"\n+\n" + bytes(rng.integers(33, 75, size=L, dtype=np.uint8)) + b"\n")
    text = b"".join(out)
    assert len(text) == nbytes
    return text


def fasta(rng, n, width=60, lo=200, hi=3000):
    recs = []
    for i in range(n):
        sq = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(lo, hi))))
        recs.append(b">chr%d case\n" % i + b"\n".join(sq[j:j + width] for j in range(0, len(sq), width)) + b"\n")
    return b"".join(recs)


# ---- tokenisers ----------------------------------------------------------------------------------------------------------------
def all_literals(text):
    return list(text)


def greedy(text, dists, min_len=3, max_len=258, start=0, before=0):
    """greedy matches at the given distances only (the longest over the set), literals elsewhere.  `before`: bytes of text in front
    of text[start] that matches may reach (text[0:start] when the tokens continue a stream)"""
    toks, p, n = [], start, len(text)
    dists = sorted(dists)
    while p < n:
        best, bd = 0, 0
        for d in dists:
            if d > p:
                break
            if text[p] != text[p - d] or p + 2 >= n or text[p + 1] != text[p + 1 - d] or text[p + 2] != text[p + 2 - d]:
                continue
            l = 3
            lim = min(max_len, n - p)
            while l < lim and text[p + l] == text[p + l - d]:
                l += 1
            if l > best:
                best, bd = l, d
        if best >= min_len:
            toks.append((best, bd)); p += best
        else:
            toks.append(text[p]); p += 1
    return toks


class Tok:
    """text and tokens made together: lit() appends bytes as literals, copy() a match (the text grows by what the match copies)"""

    def __init__(self):
        self.text = bytearray()
        self.toks = []

    def lit(self, bs):
        self.text += bs
        self.toks += list(bs)
        return self

    def copy(self, length, dist, sym=None):
        assert dist <= len(self.text)
        for _ in range(length):
            self.text.append(self.text[-dist])
        self.toks.append((length, dist) if sym is None else ("len_sym",) + sym + (dist,))
        return self

    def name_copy(self, length, dist):
        """a match of exactly this distance inside a record's NAME: literal padding until the bytes it copies hold no line end, blank or '@'"""
        while any(c in b"\n\r\t @" for c in self.text[len(self.text) - dist:len(self.text) - dist + length][:min(length, dist)]):
            self.lit(b"x")
        return self.copy(length, dist)

    def run(self, byte, n):
        """n times `byte`: one literal, then distance-1 matches of length 258 and a rest"""
        self.lit(bytes([byte])); n -= 1
        while n >= 3:
            k = min(258, n)
            if n - k in (1, 2):      # (never leave a rest too short for a match in front of a longer run: 259, 260 -> 256, 257 + 3)
                k = n - 3
            self.copy(k, 1); n -= k
        self.lit(bytes([byte]) * n)
        return self


def member_tokens(text):
    """ordinary tokens for a text whose encoding is not the point (nearest-distance candidates from a 4-byte hash)"""
    toks, p, n, last = [], 0, len(text), {}
    while p < n:
        key = bytes(text[p:p + 4])
        q = last.get(key)
        l = 0
        if q is not None and p - q <= 32768 and len(key) == 4:
            l, lim = 4, min(258, n - p)
            while l < lim and text[p + l] == text[q + l]:
                l += 1
        if l >= 4:
            toks.append((l, p - q))
            for j in range(p, min(p + l, n - 3), 7):
                last[bytes(text[j:j + 4])] = j
            p += l
        else:
            last[key] = p
            toks.append(text[p]); p += 1
    return toks


# ---- containers ----------------------------------------------------------------------------------------------------------------
BGZF_EOF = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00"


def bgzf_member(raw, text, crc=None, isize=None):
    """the bytes synth.bgzf_compress writes around zlib's output, around `raw`"""
    assert len(raw) + 26 <= 65536, "a BGZF member is at most 64 KB"
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(raw) + 25) + raw +
            struct.pack("<II", (zlib.crc32(text) & 0xffffffff) if crc is None else crc, len(text) if isize is None else isize))


def bgzf_file(members, eof=True):
    return b"".join(members) + (BGZF_EOF if eof else b"")


def gzip_container(raw, text):
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff))


def zlib_member(text, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = co.compress(text) + co.flush()
    return bgzf_member(raw, text)


# ---- the catalogue -------------------------------------------------------------------------------------------------------------
def _merge_facts(fs):
    out = {}
    for f in fs:
        for k, v in f.items():
            if k not in out:
                out[k] = v.copy() if hasattr(v, "copy") else v
            elif isinstance(v, dict):
                for kk, vv in v.items():
                    out[k][kk] = out[k].get(kk, 0) + vv
            elif isinstance(v, set):
                out[k] |= v
            elif isinstance(v, list):
                out[k] = out[k] + v
            elif isinstance(v, bool) or v is None or isinstance(v, str):
                out[k] = v
            elif k in ("longest_ll", "longest_dl", "long_ll_max", "long_dl_max", "max_dist"):
                out[k] = max(out[k], v)
            else:
                out[k] = out[k] + v
    return out


def expectation_of(facts):
    """from the limits rk_inflate.hip names -- never from what the device did"""
    if facts["long_ll_max"] > LONG_CAP or facts["long_dl_max"] > DLONG_CAP:
        return "handover"
    return "device"


def _case(name, streams, kind="fastq", gzip_form=True, bgzf_form=True, extra_facts=None, members=None):
    """streams: Deflate objects, one per BGZF member, with their texts [(deflate, text)]; the single-stream form exists for one-stream cases"""
    raws, facts, per_member = [], [], []
    for d, text in streams:
        raw = d.raw()
        assert d.facts["out_len"] == len(text), "%s: the tokens spell %d bytes, the text has %d" % (name, d.facts["out_len"], len(text))
        assert not bgzf_form or len(text) <= MEMBER_TEXT_MAX, "%s: a BGZF member holds at most 64 KB of text" % name
        raws.append((raw, bytes(text)))
        facts.append(d.facts)
        per_member.append(d.facts["entries"])
    f = _merge_facts(facts)
    f["entries_per_member"] = per_member
    f["literals_per_member"] = [x["literals"] for x in facts]
    f.update(extra_facts or {})
    text = b"".join(t for _, t in raws)
    cont = {"bgzf": bgzf_file(members if members is not None else [bgzf_member(r, t) for r, t in raws]) if bgzf_form else None,
            "gzip": gzip_container(raws[0][0], raws[0][1]) if gzip_form and len(raws) == 1 else None}
    return Case(name, cont, text, expectation_of(f), f, raws, kind)


def _high_text(seed, n=12):
    return fastq(np.random.default_rng(seed), n, high=True)


def _lens_cases():
    out = []
    # -- a code-16 run that begins in the literal/length lengths and ends in the distance lengths
    out.append(_crossing_case("repeat16_crosses_hlit", 16))
    out.append(_crossing_case("repeat18_crosses_hlit", 18))
    out.append(_crossing_case("repeat17_crosses_hlit", 17))
    out.append(_crossing_case("repeat16_after_18", "16 after 18"))
    out.append(_crossing_case("repeat16_after_17", "16 after 17"))
    out.append(_crossing_case("repeat18_crosses_into_incomplete_distance_code", "incomplete"))
    # -- HLIT = 257: no length symbol at all, no distance code (one distance length, zero)
    text = fastq(np.random.default_rng(2), 8)
    d = Deflate()
    fl = [0] * 257
    for c in text:
        fl[c] += 1
    fl[256] = 1
    d.dynamic(all_literals(text), ll=huffman_lengths(fl, 15), dl=[0])
    out.append(_case("hlit257_no_length_symbols_no_distance_code", [(d, text)]))
    # -- only the end-of-block code (one code of one bit: incomplete, and accepted), in front of and behind the text
    d = Deflate()
    only_eob = [0] * 256 + [1]
    d.dynamic([], ll=only_eob, dl=[0])
    d.dynamic(all_literals(text))
    d.dynamic([], ll=only_eob, dl=[0])
    out.append(_case("dynamic_blocks_with_only_the_end_of_block_code", [(d, text)]))
    # -- HCLEN = 5, the least a legal block can have (HCLEN = 4 transmits lengths for 16, 17, 18 and 0 only: no symbol can have a code
    # and the end-of-block code is missing -- that header is in the refused list): every code has 8 bits, sent as 8 and repeats
    text = fastq(np.random.default_rng(3), 8)
    d = Deflate()
    ll = [8] * 257
    ll[0] = 0                                                    # 256 codes of 8 bits: complete
    d.dynamic(all_literals(text), ll=ll, dl=[0], cl_lens=[2, 0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0, 2])
    c = _case("hclen5_the_least_a_legal_header_has", [(d, text)])
    assert c.facts["hclen"] == {5}
    out.append(c)
    return out


def _crossing_params(which):
    """literal/length lengths that END with the value the distance lengths BEGIN with -> (ll, dl, distances in the code, zero16)"""
    if which == 16:
        # 251 symbols of 8 bits and 10 of 9 (symbols 251 .. 260); distance lengths 9 9 9 9 1 2 3 4 5 6 7: complete, five long codes
        return [8] * 251 + [9] * 10, [9, 9, 9, 9, 1, 2, 3, 4, 5, 6, 7], (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33), False
    if which == 17:      # 270 symbols used, three zero lengths behind them and three zero distance lengths in front: code 17, six zeros
        return [8] * 242 + [9] * 28 + [0] * 3, [0, 0, 0, 1, 2, 3, 3], (4, 5, 7, 9), False
    if which == "16 after 17":      # four + three zeros: a 17 of four and a 16 of three behind it
        return [8] * 242 + [9] * 28 + [0] * 4, [0, 0, 0, 1, 2, 3, 3], (4, 5, 7, 9), True
    if which == "incomplete":       # twenty zeros across the boundary into a distance code of ONE code of one bit (distance 4): incomplete
        return [8] * 242 + [9] * 28 + [0] * 16, [0, 0, 0, 1], (4,), False
    # 270 symbols used (242 of 8 bits, 28 of 9), sixteen zero lengths behind them and four zero distance lengths in front: one run
    # of twenty zeros across the boundary (code 18; "16 after 18": 18 for seventeen of them, 16 for the last three)
    return [8] * 242 + [9] * 28 + [0] * 16, [0, 0, 0, 0, 2, 2, 2, 2], (5, 7, 9, 13), which == "16 after 18"


def _crossing_case(name, which):
    rng = np.random.default_rng(10 + len(str(which)) + (which if isinstance(which, int) else 0))
    text = fastq(rng, 10, high=True)
    ll, dl, dists, zero16 = _crossing_params(which)
    d = Deflate()
    d.dynamic(greedy(text, dists, max_len=6), ll=ll, dl=dl, zero16=zero16)      # (length symbols 257 .. 260 have a code in every variant)
    return _case(name, [(d, text)])


def _crossing_stream_case(name, which, nblocks=40):
    """ONE stream of many small dynamic blocks (each below 1 KB of compressed bytes), EVERY one of which carries the crossing run in
    its header: with RKMH_GZIP_CHUNK_KB=1 every chunk boundary has such a header behind it, and the number of chunks the device
    route forms is gz_header_ok's verdict on them"""
    rng = np.random.default_rng(200 + len(str(which)))
    ll, dl, dists, zero16 = _crossing_params(which)
    d, text = Deflate(), b""
    for i in range(nblocks):
        at = len(text)
        text += fastq(rng, 2, lo=120, hi=150, high=True, tag=b"c%d_" % i)
        d.dynamic(greedy(text, dists, max_len=6, start=at), ll=ll, dl=dl, zero16=zero16)
    c = _case(name, [(d, text)], bgzf_form=len(text) <= MEMBER_TEXT_MAX)
    bits = c.facts["dynamic_header_bits"]
    assert len(c.facts["repeat_crossed"]) == nblocks and max(b - a for a, b in zip(bits, bits[1:])) < 8192
    return c


def _long_cap_case(n_long):
    """HLIT = 286, every symbol with a code, exactly n_long of them longer than the 8-bit root: the literals 128 .. 255 (and, for
    129, symbol 285), all of which the text uses"""
    rng = np.random.default_rng(20 + n_long)
    text = fastq(rng, 40, high=True)
    # every byte 128 .. 255 at least once, in one name
    text = b"@all" + bytes(range(128, 256)) + b"\nACGT\n+\nIIII\n" + text
    lens = complete_lengths(286, n_long, LT)
    long_syms = list(range(128, 256)) + ([285] if n_long > 128 else [])
    long_syms = long_syms[:n_long]
    cnt = np.bincount(np.frombuffer(text, np.uint8), minlength=256)
    short_syms = sorted((s for s in range(286) if s not in set(long_syms)), key=lambda s: -(int(cnt[s]) if s < 256 else (5 if s > 256 else 1)))
    order = short_syms + sorted(long_syms, key=lambda s: -(int(cnt[s]) if s < 256 else 0))
    ll = assign_lengths(286, lens, order)
    assert sum(1 for l in ll if l > LT) == n_long and all(ll[s] > LT for s in long_syms)
    toks = greedy(text, (1, 2, 3, 4, 35, 36, 70, 100, 200, 300), max_len=258)
    d = Deflate()
    d.dynamic(toks, ll=ll)
    return _case("long_codes_%d_of_cap_%d" % (n_long, LONG_CAP), [(d, text)])


def _all_distances_case():
    """HLIT = 286 and HDIST = 30, all thirty distance symbols in use (the last distance of each, 32 768 included), twenty of them
    with codes above the 6-bit root.  One long read, then thirty short records whose NAMES copy 12 bytes from an exact distance back"""
    rng = np.random.default_rng(30)
    L = 16500
    head = b"@long\xc3\xa9 one read\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L)) + b"\n+\n" + bytes(rng.integers(33, 75, size=L, dtype=np.uint8)) + b"\n"
    tk = Tok()
    tk.toks = greedy(head, (1, 2, 3, 4), max_len=258)
    tk.text = bytearray(head)
    reps = [DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1 for s in range(30)]
    for s in range(29, -1, -1):
        tk.lit(b"@d%02d_" % s)
        if reps[s] < 16:
            tk.lit(b"0123456789abcdef"[:reps[s]])
        tk.name_copy(12, reps[s])
        tk.lit(b"\nACGTNACGT\n+\nIIIIIIIII\n")
    text = bytes(tk.text)
    assert len(text) <= MEMBER_TEXT_MAX
    cnt = np.bincount(np.frombuffer(text, np.uint8), minlength=256)
    ll = assign_lengths(286, complete_lengths(286, 100, LT), sorted(range(286), key=lambda s: -(int(cnt[s]) if s < 256 else 3)))
    dl = assign_lengths(30, complete_lengths(30, 20, DT), list(range(30)))
    d = Deflate()
    d.dynamic(tk.toks, ll=ll, dl=dl)
    return _case("hlit286_hdist30_all_thirty_distances_twenty_long", [(d, text)])


def _fixed_high_case():
    text = _high_text(40, 30)
    d = Deflate()
    d.fixed(greedy(text, (1, 2, 3, 4, 5, 6, 35, 70), max_len=258))
    return _case("fixed_code_literals_128_to_255", [(d, text)])


def _empty_block_cases():
    out = []
    rng = np.random.default_rng(50)
    text = fastq(rng, 6, high=True)
    only_eob = [0] * 256 + [1]
    for name, first, last in (("empty_stored_block_first_and_final", "stored", "stored"), ("empty_fixed_block_first_and_final", "fixed", "fixed"),
                              ("empty_dynamic_block_first_and_final", "dynamic", "dynamic")):
        d = Deflate()

        def empty(kind):
            if kind == "stored":
                d.stored(b"")
            elif kind == "fixed":
                d.fixed([])
            else:
                d.dynamic([], ll=only_eob, dl=[0])
        empty(first)
        h = len(text) // 2
        d.fixed(all_literals(text[:h]))
        for k in ("stored", "fixed", "dynamic", "stored"):
            empty(k)
        d.dynamic(greedy(text, (1, 2, 3, 4), start=h))
        empty(last)
        out.append(_case(name, [(d, text)]))
    # hundreds of blocks of one symbol each: fixed, dynamic (two codes of one bit) and stored in turn
    text = fastq(rng, 5, lo=40, hi=60, high=True)
    d = Deflate()
    for i, c in enumerate(text):
        if i % 3 == 0:
            d.fixed([c])
        elif i % 3 == 1:
            ll = [0] * 257
            ll[c], ll[256] = 1, 1
            d.dynamic([c], ll=ll, dl=[0])
        else:
            d.stored(bytes([c]))
    c = _case("hundreds_of_one_symbol_blocks", [(d, text)])
    out.append(c)
    # a stored block behind a block that ends at each of the eight bit offsets: a fixed block of '@' and h nine-bit literals
    # (bytes >= 144) ends 3 + 8 + 9 h + 7 bits behind a byte boundary
    d, parts = Deflate(), []
    for h in range(8):
        name = b"@" + bytes([0xC0 + h]) * h
        rest = b"s%d\nACGTACGT\n+\nIIIIIIII\n" % h
        d.fixed(all_literals(name))
        d.stored(rest)
        parts.append(name + rest)
    out.append(_case("stored_block_behind_every_bit_offset", [(d, b"".join(parts))]))
    return out


def _literal_run_cases():
    out = []
    rng = np.random.default_rng(60)
    # between two matches: one long read whose bases are runs of fresh literals of exactly R bytes, a short match between them
    t = Tok()
    t.lit(b"@runs\n")
    start = len(t.text)
    t.lit(b"ACGTACGT").copy(4, 4)
    for R in (254, 255, 256, 509, 510, 511, 1, 2, 765):
        t.lit(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=R)))
        t.copy(5, 7)
    N = len(t.text) - start
    t.lit(b"\n+\n").run(ord("F"), N).lit(b"\n")
    d = Deflate()
    d.dynamic(t.toks)
    c = _case("literal_runs_254_to_511_between_matches", [(d, bytes(t.text))])
    out.append(c)
    # at the tail: a match, then exactly R literals to the end of the member
    for R in (254, 255, 256, 509, 510, 511):
        t = Tok()
        N = R + 40
        t.lit(b"@tail%d\n" % R).run(ord("A"), N).lit(b"\n+\n").run(ord("I"), N - (R - 1))
        assert isinstance(t.toks[-1], tuple)
        t.lit(bytes(rng.integers(33, 75, size=R - 1, dtype=np.uint8)) + b"\n")
        d = Deflate()
        d.fixed(t.toks)
        c = _case("literal_tail_of_%d" % R, [(d, bytes(t.text))])
        out.append(c)
    # totals of literals = 0, 1, 2, 3 mod 4 (the partial dword of the literal stream)
    for m in range(4):
        t = Tok()
        name = b"@m%d" % m
        t.lit(name + b"\n").run(ord("C"), 50).lit(b"\n+\n").run(ord("I"), 50).lit(b"\n")
        while sum(1 for x in t.toks if not isinstance(x, tuple)) % 4 != m:
            t = Tok()
            name += b"x"
            t.lit(name + b"\n").run(ord("C"), 50).lit(b"\n+\n").run(ord("I"), 50).lit(b"\n")
        d = Deflate()
        d.dynamic(t.toks)
        out.append(_case("literal_total_%d_mod_4" % m, [(d, bytes(t.text))]))
    return out


def _place_cases():
    out = []
    rng = np.random.default_rng(70)
    # one long read: 32 000 x 'A', 32 000 x 'I' -- two literals and two chains of distance-1 matches of length 258
    t = Tok()
    t.lit(b"@long\n").run(ord("A"), 32000).lit(b"\n+\n").run(ord("I"), 32000).lit(b"\n")
    d = Deflate()
    d.dynamic(t.toks)
    out.append(_case("long_read_of_distance_1_matches_of_258", [(d, bytes(t.text))]))
    # distance 32 768 and 32 767 with length 258 in a member of 65 536 bytes: the text repeats with that period
    for period in (32768, 32767):
        H = fastq_exact(rng, period, tag=b"p%d_" % period)
        R = fastq(rng, 3, tag=b"after")
        text = H + H + R
        m1 = text[:65536]
        t = Tok()
        t.toks = member_tokens(H)
        t.text = bytearray(H)
        left = period
        while left:
            k = 258 if left - 258 not in (1, 2) else 255
            k = min(k, left)
            t.copy(k, period, sym=(27, 31) if (k == 258 and left % 5 == 0) else None)
            left -= k
        t.lit(m1[2 * period:])
        assert bytes(t.text) == m1
        d1, d2 = Deflate(), Deflate()
        d1.dynamic(t.toks)
        d2.fixed(member_tokens(text[65536:]))
        c = _case("distance_%d_length_258_in_a_65536_byte_member" % period, [(d1, m1), (d2, text[65536:])])
        out.append(c)
    # matches of length 258 at distances 2 .. 17: the copy overlaps its own output with a period that does not divide 8 or 16
    t = Tok()
    t.lit(b"@overlap\n")
    s0 = len(t.text)
    for dd in range(2, 18):
        t.lit(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=dd))).copy(258, dd)
    N = len(t.text) - s0
    t.lit(b"\n+\n")
    q0 = len(t.text)
    for dd in range(2, 18):
        t.lit(bytes(rng.integers(33, 75, size=dd, dtype=np.uint8))).copy(258, dd)
    assert len(t.text) - q0 == N
    t.lit(b"\n")
    d = Deflate()
    d.dynamic(t.toks)
    out.append(_case("self_overlapping_matches_of_258_at_distances_2_to_17", [(d, bytes(t.text))]))
    # several hundred matches, each a copy of the match before it
    t = Tok()
    t.lit(b"@chain\n").lit(b"GATTA")
    for _ in range(400):
        t.copy(5, 5)
    t.lit(b"\n+\n").lit(b"5:I?F")
    for _ in range(400):
        t.copy(5, 5)
    t.lit(b"\n")
    d = Deflate()
    d.dynamic(t.toks)
    out.append(_case("chain_of_400_matches_each_copying_the_one_before", [(d, bytes(t.text))]))
    # 511, 512 and 513 entries in one member (matches + the tail's entry): the 512-entry stage of pass 2
    for E in (511, 512, 513):
        nm = E - 1
        a = (nm + 1) // 2
        t = Tok()
        t.lit(b"@e%d\n" % E).lit(b"A")
        for _ in range(a):
            t.copy(3, 1)
        t.lit(b"\n+\n").lit(b"I")
        if nm - a == a:
            for _ in range(a):
                t.copy(3, 1)
        else:
            for _ in range(a - 2):
                t.copy(3, 1)
            t.copy(6, 1)
        t.lit(b"\n")
        d = Deflate()
        d.dynamic(t.toks)
        c = _case("member_of_%d_entries" % E, [(d, bytes(t.text))])
        assert c.facts["entries_per_member"] == [E], c.facts["entries_per_member"]
        out.append(c)
    return out


def _container_cases():
    out = []
    rng = np.random.default_rng(80)
    # members of 1, 2, 65 535, 0 (in the MIDDLE of the file) and 65 536 bytes of text
    text = fastq(rng, 900, lo=60, hi=120)
    sizes = [1, 2, 65535, 0, 65536, 3000]    # (two empty members in a row would use up the loader's two members of lookahead: a documented hand-over)
    members, at, texts = [], 0, []
    for s in sizes:
        members.append(zlib_member(text[at:at + s]))
        texts.append(text[at:at + s]); at += s
    members.append(zlib_member(text[at:]))
    texts.append(text[at:])
    cont = {"bgzf": bgzf_file(members), "gzip": None}
    f = dict(member_text_sizes=sizes + [len(text) - at], empty_members_in_the_middle=1, long_ll_max=0, long_dl_max=0)
    out.append(Case("members_of_0_1_2_65535_65536_bytes", cont, text, "device", f, [], "fastq"))
    # cat a.fq.gz b.fq.gz: the first file's end-of-file member lies in the middle; the first text ends inside a quality line
    a_end = text.find(b"\n+\n", 40000) + 3 + 10
    a, b = text[:a_end], text[a_end:]

    def own(tx, block):
        ms = []
        for lo in range(0, len(tx), block):
            dd = Deflate()
            dd.dynamic(member_tokens(tx[lo:lo + block]))
            ms.append(bgzf_member(dd.raw(), tx[lo:lo + block]))
        return ms
    img = bgzf_file(own(a, 9000)) + bgzf_file(own(b, 11000))
    na = (len(a) + 8999) // 9000
    f = dict(empty_member_at=na, halves=(len(a), len(b)), long_ll_max=0, long_dl_max=0)
    out.append(Case("cat_of_two_bgzf_files_empty_member_mid_file", {"bgzf": img, "gzip": None}, text, "device", f, [], "fastq"))
    return out


def _stream_cases():
    """the single-stream route (rk_gunzip.hip): the catalogue's token shapes in ONE long stream, so that RKMH_GZIP_CHUNK_KB=1 puts
    chunk edges in front of and inside them"""
    out = []
    rng = np.random.default_rng(90)
    # (a) every block carries an incomplete one-code distance tree (one distance code of one bit: distance 1 only).  By
    # gz_header_ok such a header still qualifies as a chunk start (dist_max == 1), as zlib accepts it
    tk_all, d = Tok(), Deflate()
    for i in range(60):
        t = Tok()
        L = int(rng.integers(200, 900))
        t.lit(b"@inc%d\xe9\n" % i).lit(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L))).lit(b"\n+\n").run(ord("I") - i % 5, L).lit(b"\n")
        fl = [0] * 286
        fl[256] = 1
        for x in t.toks:
            fl[x if not isinstance(x, tuple) else 257 + len_symbol(x[0])] += 1
        d.dynamic(t.toks, ll=huffman_lengths(fl, 15), dl=[1])
        tk_all.text += t.text
    c = _case("stream_every_block_with_an_incomplete_one_code_distance_tree", [(d, bytes(tk_all.text))], bgzf_form=True)
    assert c.facts["incomplete_dist"] == 60
    out.append(c)
    # (b) the token shapes of the catalogue, one block each, many times over, between ordinary blocks
    d, text = Deflate(), bytearray()
    only_eob = [0] * 256 + [1]
    for rep in range(14):
        fresh = fastq(rng, 25, high=True, tag=b"s%d_" % rep)
        at = len(text)
        text += fresh
        d.dynamic(greedy(bytes(text), (1, 2, 3, 4, 35, 36, 70, 100, 200, 300), start=at))
        # far copies at exact distances, inside a record's name
        if len(text) > 33000:
            t = Tok(); t.text = text
            t.lit(b"@far%d_" % rep).name_copy(20, 32768).lit(b"_").name_copy(20, 32767).lit(b"\nACGT\n+\nIIII\n")
            d.fixed(t.toks)
            text = t.text
        # self-overlap, literal runs of 255 / 256 / 510, a chain, empty blocks, one-symbol blocks, a stored block
        t = Tok(); t.text = text
        n0 = len(text)
        t.lit(b"@mix%d\n" % rep)
        s0 = len(t.text)
        for dd in (2, 3, 5, 7, 11, 13, 17):
            t.lit(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=dd))).copy(258, dd)
        for R in (255, 256, 510):
            t.lit(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=R))).copy(5, 5)
        for _ in range(60):
            t.copy(5, 5)
        N = len(t.text) - s0
        t.lit(b"\n+\n").run(ord("J"), N).lit(b"\n")
        text = t.text
        d.dynamic(t.toks)
        d.dynamic([], ll=only_eob, dl=[0]); d.fixed([]); d.stored(b"")
        rec = b"@st%d\nACGTNACGT\n+\nIIIIIIIII\n" % rep
        for c_ in rec[:6]:
            d.fixed([c_])
        d.stored(rec[6:])
        text += rec
    # a dynamic final block inside the last 4 096 bits
    rec = b"@last\nACGT\n+\nFFFF\n"
    text += rec
    d.dynamic(all_literals(rec))
    out.append(_crossing_stream_case("stream_every_block_with_a_crossing_16", 16))
    out.append(_crossing_stream_case("stream_every_block_with_a_crossing_18", 18))
    out.append(_crossing_stream_case("stream_every_block_with_a_crossing_18_into_an_incomplete_distance_code", "incomplete"))
    # (c) no block qualifies as a chunk start: fixed and stored blocks only (k_gz_find_starts looks for dynamic headers).  The stretch is
    # then ONE chunk; it stays the device's as long as its entries and literals fit the scratch region of a stretch's last chunk
    # (rk_gunzip.hip, region_of: 5 bytes per compressed byte + 1.3 MB) -- always, for a file of this size
    fs, ftext = Deflate(), fastq(rng, 700, high=True, tag=b"f")
    for lo in range(0, len(ftext), 3000):
        if (lo // 3000) % 3 == 2:
            fs.stored(ftext[lo:lo + 3000])
        else:
            fs.fixed(greedy(ftext[:lo + 3000], (1, 2, 3, 4, 35, 70, 300), start=lo))
    out.append(_case("stream_of_fixed_and_stored_blocks_no_chunk_start", [(fs, ftext)], bgzf_form=False))
    c = _case("stream_of_the_catalogue_token_shapes", [(d, bytes(text))], bgzf_form=False)
    assert c.facts["final_dynamic_bits_from_end"] < 4096 and c.facts["max_dist"] == 32768
    out.append(c)
    return out


def _fasta_cases():
    out = []
    rng = np.random.default_rng(95)
    text = fasta(rng, 6)
    # members of ~6 KB: crossing repeats and distance-1 .. 61 matches (the line width + 1 is the commonest distance in a genome)
    ms, raws = [], []
    for lo in range(0, len(text), 6000):
        part = text[lo:lo + 6000]
        d = Deflate()
        d.dynamic(greedy(part, (1, 2, 3, 4, 61, 122), max_len=258), zero16=True)
        raws.append((d, part))
    out.append(_case("fasta_members_with_zero_run_repeats", raws, kind="fasta", gzip_form=False))
    d = Deflate()
    h = len(text) // 3
    d.fixed(greedy(text[:h], (1, 2, 3, 4, 61)))
    d.stored(text[h:h + 5000])
    d.dynamic(greedy(text, (1, 2, 3, 4, 61, 122, 183), start=h + 5000), zero16=True)
    out.append(_case("fasta_stream_fixed_stored_dynamic", [(d, text)], kind="fasta", bgzf_form=False))
    return out


_CACHE = {}


def legal_cases():
    if "legal" not in _CACHE:
        cs = []
        cs += _lens_cases()
        cs += [_long_cap_case(128), _long_cap_case(129), _all_distances_case(), _fixed_high_case()]
        cs += _empty_block_cases()
        cs += _literal_run_cases()
        cs += _place_cases()
        cs += _container_cases()
        cs += _stream_cases()
        cs += _fasta_cases()
        assert len({c.name for c in cs}) == len(cs)
        _CACHE["legal"] = cs
    return _CACHE["legal"]


# ---- refused streams -----------------------------------------------------------------------------------------------------------
# (name, the line of k_inflate_lanes that refuses it, builder).  Every one is a single small BGZF member; `text` is what the footer
# claims (CRC-32 and ISIZE of it), so that only the named fault stands between the member and its text.
Refused = namedtuple("Refused", "name why member raw text arbiter")


def refused_cases():
    if "refused" in _CACHE:
        return _CACHE["refused"]
    rec = b"@bad\nACGTACGTAC\n+\nIIIIIIIIII\n"
    only_eob = [0] * 256 + [1]
    out = []

    def add(name, why, build, text=rec, crc=None, isize=None, arbiter="zlib", cut=None):
        d = Deflate(check=False)
        build(d)
        raw = d.raw()
        if cut is not None:
            raw = raw[:cut]
        out.append(Refused(name, why, bgzf_member(raw, text, crc, isize), raw, text, arbiter))

    lits = all_literals(rec)
    fl = [0] * 257
    for c in rec:
        fl[c] += 1
    fl[256] = 1
    good_ll = huffman_lengths(fl, 15)
    add("block_type_3", "fail(4)", lambda d: (d.fixed(lits[:5]), d.reserved()))
    add("stored_len_nlen_mismatch", "fail(3)", lambda d: d.stored(rec, nlen=(len(rec) ^ 0xFFFF) ^ 0x0100))
    add("hlit_287", "fail(5)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], hlit=287, hdist=1))
    add("hdist_31", "fail(5)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], hlit=257, hdist=31))
    cl_used = rle(good_ll + [0])
    add("code_length_code_incomplete", "fail(11)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], cl_lens=_cl_lens_bad(cl_used, incomplete=True)))
    add("code_length_code_over_subscribed", "fail(11)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], cl_lens=_cl_lens_bad(cl_used, incomplete=False)))
    add("code_16_as_the_first_length", "fail(9)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], cl=[(16, 3)] + cl_used[3:], cl_lens=_cl_lens_for(cl_used + [(16, 3)])))
    add("repeat_past_hlit_plus_hdist", "fail(9)", lambda d: d.dynamic(lits, ll=good_ll, dl=[0], cl=rle(good_ll) + [(18, 11)], cl_lens=_cl_lens_for(cl_used + [(18, 11)])))
    no_eob = list(good_ll); no_eob[256] = 0
    add("no_end_of_block_code", "fail(10)", lambda d: d.dynamic(lits, ll=no_eob, dl=[0], eob=False))
    add("hclen_4_no_symbol_can_have_a_code", "fail(10)", lambda d: d.dynamic([], ll=[0] * 257, dl=[0], cl=[(18, 138), (18, 119), 0], cl_lens=[1] + [0] * 17 + [1], hclen=4, eob=False))
    over = list(good_ll); over[ord("A")] = 1; over[ord("C")] = 1
    add("literal_length_code_over_subscribed", "fail(11)", lambda d: d.dynamic(lits, ll=over, dl=[0]))
    inc = [l + 1 if l else 0 for l in good_ll]
    add("literal_length_code_incomplete", "fail(11)", lambda d: d.dynamic(lits, ll=inc, dl=[0]))
    add("bit_pattern_with_no_code", "fail(13)", lambda d: (d.fixed(lits), d.dynamic([("raw", 1, 1)], ll=only_eob, dl=[0], eob=False)))
    add("fixed_code_symbol_286", "fail(14)", lambda d: d.fixed(lits[:7] + [("sym", 286)] + lits[7:]))
    add("fixed_code_symbol_287", "fail(14)", lambda d: d.fixed(lits[:7] + [("sym", 287)] + lits[7:]))
    add("fixed_code_distance_symbol_30", "fail(13) / fail(14)", lambda d: d.fixed(lits[:12] + [("dist_sym", 30)] + lits[15:]))
    add("fixed_code_distance_symbol_31", "fail(13) / fail(14)", lambda d: d.fixed(lits[:12] + [("dist_sym", 31)] + lits[15:]))
    add("distance_before_the_start_of_the_member", "fail(20)", lambda d: d.fixed(lits[:6] + [(4, 7)] + lits[10:]))
    add("text_longer_than_isize", "fail(16)", lambda d: d.fixed(lits + lits), text=rec, arbiter="gzip")
    add("text_shorter_than_isize", "fail(21)", lambda d: d.fixed(lits), text=rec, isize=len(rec) + 5, arbiter="gzip")
    add("member_cut_short", "fail(2)", lambda d: d.fixed(lits), cut=12)
    add("wrong_crc32", "status 30 (k_crc32_members)", lambda d: d.fixed(lits), crc=(zlib.crc32(rec) ^ 0x00010000) & 0xffffffff, arbiter="gzip")
    _CACHE["refused"] = out
    return out


def _cl_lens_for(clseq):
    fc = [0] * 19
    for it in clseq:
        fc[it[0] if isinstance(it, tuple) else it] += 1
    return huffman_lengths(fc, 7)


def _cl_lens_bad(clseq, incomplete):
    lens = _cl_lens_for(clseq)
    used = [s for s in range(19) if lens[s]]
    if incomplete:
        s = max(used, key=lambda s: lens[s])
        lens[s] += 1                                   # one code a bit longer: the code no longer fills its space
        assert lens[s] <= 7
    else:
        s = max(used, key=lambda s: lens[s])
        lens[s] -= 1                                   # one code a bit shorter: more codes than the space holds
    return lens
