"""Reference panels built key by key, so that every value form of the resident index (rk_index_plan.hpp: fill_hash_table / build_kpost, driven by build_index in rk_index.hip) is
built on purpose and on both sides of the threshold that selects it, and read sets that show each such key to each of the three
readers that decode the forms independently: accumulate_posting (the general path, rk_kernels.hip), the drain of k_classify_tile
(rk_classify.hip) and the drain and phase 2 of k_classify_kmer (rk_kmer.hip).  tests/test_index_cases_cpu.py checks without a GPU
that the inputs mean what they claim; tests/test_gpu_index_forms.py hands them to the device and reads rk_index_stats.

Everything comes from seeds.  A panel is a dict  hash -> {reference: multiplicity}; reference r's sketch row is the ascending
expansion of its keys, handed over with Context.set_reference_sketches, so the test -- not a sketching pass -- decides which
reference holds which hash how often.  Keys are window hashes (k = 16, default policy) of real k-mers of a seeded source text
(random sequence, a tandem repeat of a 23-base unit, an A run and a C run of 540 bases): reads cut from the text hit them, and the
k-mer-space enumeration finds exactly one preimage each.  Every key carries the form it is MEANT to take -- in the hash-space value
(single_once, single_multi, pair, list) and in the k-mer-space value table (reference, single_multi, pair, inline, base_inline,
base_list, plain) -- next to Python restatements of the builder's rules (hash_form, bucket_fill, kmer_forms) that say what it WILL take.

  panels       forms (12 references, S = 2000), wide_ids (2100, S = 256: sparse counter rows), families (40, S = 2000: base lists),
               chains (2, 256 buckets: overflow chains that wrap from the last bucket to bucket 0)
  read sets    .one (a key's k-mer plus one base: one window), .cuts (150 bases of the text), .tandem (cuts of the repeat that hold a
               key 1, 2, 29, 30 and 31 times), .runs (510 .. 513 windows of a base run), .probes (a key n times and private keys of ONE
               of its references, the k-mers joined by N: that reference is the read's unique maximum, so its posting shows in the row),
               .long (1600 .. 2400 bases, beyond the fused kernels: cuts of the text, the runs, and every probe padded with N)
  mutations    mutations(panel): the neighbouring mistake at every labelled key -- see tests/test_index_cases_cpu.py
  limits       may_hand_back_kmer: what k_classify_kmer documents (tile_cases.may_hand_back holds k_classify_tile's)

One pair of references per panel is identical on purpose (Panel.dup: every key of the first is a key of the second), so the first-wins
tie is exercised; `chains` has none: with two references in all, identical rows would give every key the same value and a lookup that
returned the wrong key could not be told from the right one.
"""
import collections
import functools

import numpy as np

import tile_cases as tc

K = 16
KS = [K]
POL = tc.DEFAULT
UNIT_LEN, UNIT_COPIES, RUN = 23, 40, 540
SLOTS = 8                      # slots of a bucket (IDX_SLOTS)
KBASE_MAX = 8                  # base lists of an index (rk_index_plan.hpp)
COUNT_SLOTS = 3000017          # depth map of the -M passes
LONG_MIN, LONG_MAX = 1600, 2400
HS_FORMS = ("single_once", "single_multi", "pair", "list")
KV_FORMS = ("reference", "single_multi", "pair", "inline", "base_inline", "base_list", "plain")


# ---- the builder's rules, restated ---------------------------------------------------------------------------------------------------
def hash_form(post):
    """fill_hash_table (rk_index_plan.hpp): one reference with multiplicity <= 511 is stored inline; two references once each, both below 2048, as a pair of
    11-bit fields; anything else is a posting list"""
    refs = sorted(post)
    if len(refs) == 1 and post[refs[0]] <= 511:
        return "single_once" if post[refs[0]] == 1 else "single_multi"
    if len(refs) == 2 and all(post[r] == 1 for r in refs) and refs[1] < 2048:
        return "pair"
    return "list"


def n_buckets(nkeys):
    nb = 256
    while nb * 250 < nkeys * 100 + 100:
        nb *= 2
    return nb


Fill = collections.namedtuple("Fill", "nb stored overflowed longest_chain wrapped")


def bucket_fill(keys):
    """fill_hash_table (rk_index_plan.hpp): keys in ascending order, home bucket = (h >> 32) & (buckets - 1), eight slots, then the next bucket (the
    bucket left behind gets its overflow flag).  .stored: key -> (home, bucket it lies in)"""
    nb = n_buckets(len(keys))
    used = [0] * nb
    over = set()
    stored, longest, wrapped = {}, 0, 0
    for h in sorted(keys):
        home = b = (h >> 32) & (nb - 1)
        chain = 1
        while used[b] == SLOTS:
            over.add(b)
            b = (b + 1) & (nb - 1)
            chain += 1
        used[b] += 1
        stored[h] = (home, b)
        longest = max(longest, chain)
        wrapped |= int(b < home)
    return Fill(nb, stored, len(over), longest, wrapped)


def _sym_diff(a, b):
    return len(set(a) ^ set(b))


KmerForms = collections.namedtuple("KmerForms", "bases dropped form")


def kmer_forms(panel):
    """build_kpost and ValueTable::value_id_of (rk_index_plan.hpp): which lists become bases (the heaviest simple lists of >= 8 references, keys x references, none
    within max(4, size / 4) of a base already chosen, at most eight), whether the 5 % rule then clears them, and the form of every
    key's value: a list of 3 .. 6 references below 512 once each is inline; a simple list of >= 8 references whose nearest base lies
    at d with 2 (1 + d) <= size is (base, exceptions) -- inside the value up to eight exceptions (all below 512), else as a list"""
    lists = collections.OrderedDict()          # content -> [weight, first appearance] in ascending key order, as `post` is walked
    for h in sorted(panel.post):
        if hash_form(panel.post[h]) == "list":
            e = tuple(sorted(panel.post[h].items()))
            lists.setdefault(e, [0, len(lists)])[0] += 1
    simple = {e: all(m == 1 for _, m in e) for e in lists}
    cand = [e for e in lists if simple[e] and len(e) >= 8]
    cand.sort(key=lambda e: (-lists[e][0] * len(e), lists[e][1]))
    bases = []
    for e in cand:
        if len(bases) >= KBASE_MAX:
            break
        refs = [r for r, _ in e]
        if all(_sym_diff(refs, b) > max(4, len(e) // 4) for b in bases):
            bases.append(refs)
    dropped = 0
    if bases:
        total = sum(w * len(e) for e, (w, _) in lists.items())
        saved = 0
        for e, (w, _) in lists.items():
            if simple[e] and len(e) >= 8:
                bd = min(_sym_diff([r for r, _ in e], b) for b in bases)
                if 2 * (1 + bd) <= len(e):
                    saved += w * (len(e) - bd - 1)
        if saved * 20 < total:
            bases, dropped = [], 1
    form = {}
    for h, post in panel.post.items():
        hs = hash_form(post)
        if hs != "list":
            form[h] = "reference" if hs == "single_once" else hs
            continue
        e = tuple(sorted(post.items()))
        refs = [r for r, _ in e]
        if 3 <= len(e) <= 6 and simple[e] and max(refs) < 512:
            form[h] = "inline"
        elif simple[e] and len(e) >= 8 and bases:
            ds = [_sym_diff(refs, b) for b in bases]
            bd = min(ds)
            exc = set(refs) ^ set(bases[ds.index(bd)])
            if 2 * (1 + bd) > len(e):
                form[h] = "plain"
            else:
                form[h] = "base_inline" if bd <= 8 and all(r < 512 for r in exc) else "base_list"
        else:
            form[h] = "plain"
    return KmerForms(bases, dropped, form)


# ---- the limits k_classify_kmer documents (rk_kmer.hip), beside tile_cases.may_hand_back -------------------------------------------
def may_hand_back_kmer(sketches, h, length, sparse):
    """k_classify_kmer flags a read for the general path (phase 2, `reroute`) when it is longer than the kernel stages, when its
    non-zero hashes do not all fit the sketch (the callers here rule that out: windows <= S), when its hit multiset overflows --
    EVERY occurrence of a hit takes a slot ("more hits than the set holds"), the set has the power of two >= 3 x the expected hits of
    the batch's longest read and at most 1024 slots, and with whole rows handed over (density 1) a read never has more hits than a
    third of that unless the cap acts: more than 1024 hit occurrences -- or, under a sparse row, when it hits more references than the
    128-entry map holds.  There is no limit on how often one k-mer occurs (the rank is counted by probing, not kept in 5 bits)."""
    if length > tc.FUSED_MAXLEN:
        return True
    allv = np.unique(np.concatenate([np.asarray(s, dtype=np.uint64) for s in sketches])) if len(sketches) else np.zeros(0, np.uint64)
    hit = np.isin(h[h != 0], allv)
    if int(hit.sum()) > 1024:
        return True
    if sparse:
        multi, _ = tc.shared_counts(sketches, h)
        return int((multi > 0).sum()) > 128
    return False


# ---- the source text ---------------------------------------------------------------------------------------------------------------------
class Text:
    """random sequence, then UNIT x 40, an A run and a C run of 540 bases between random flanks; .h[p] = hash of the window at p"""

    def __init__(self, orc, seed, nrand):
        rng = np.random.default_rng(seed)

        def flank(n, avoid):
            while True:
                f = tc.rand(rng, n)
                if f[:1] not in avoid and f[-1:] not in avoid:
                    return f
        body = tc.rand(rng, nrand - 1) + b"G"
        while True:
            self.unit = tc.rand(rng, UNIT_LEN)
            self.tandem_at = len(body)
            self.a_at = self.tandem_at + UNIT_LEN * UNIT_COPIES + 120
            self.c_at = self.a_at + RUN + 120
            self.text = body + self.unit * UNIT_COPIES + flank(120, (b"A",)) + b"A" * RUN + flank(120, (b"A", b"C")) + b"C" * RUN + flank(120, (b"C",))
            self.h = orc.calc_hashes(self.text, KS, POL.oracle(orc))
            self.count = collections.Counter(self.h.tolist())
            th = self.h[self.tandem_at: self.tandem_at + UNIT_LEN].tolist()
            if len(set(th)) == UNIT_LEN and all(self.count[x] in (UNIT_COPIES - 1, UNIT_COPIES) for x in th):
                break
        assert 0 not in self.count
        assert len(self.h) == len(self.text) - K
        self.nrand = nrand
        assert self.count[int(self.h[self.a_at])] == RUN - K + 1 == self.count[int(self.h[self.c_at])] and RUN - K + 1 > 512
        free = [p for p in range(nrand - K) if self.count[int(self.h[p])] == 1]
        self.free = [free[i] for i in rng.permutation(len(free)).tolist()]      # positions of k-mers the text holds once
        self.rng = rng

    def take(self, want=None):
        """the position of an unused k-mer (want: a predicate on its hash)"""
        for i, p in enumerate(self.free):
            if want is None or want(int(self.h[p])):
                return self.free.pop(i)
        raise AssertionError("the text has no such k-mer left")

    def kmer(self, p):
        return self.text[p: p + K]


# ---- panels --------------------------------------------------------------------------------------------------------------------------------
class Panel:
    def __init__(self, name, orc, nref, S, seed, nrand, nfill, dup):
        self.name, self.nref, self.S, self.dup = name, nref, S, dup
        self.text = Text(orc, seed, nrand)
        self.post, self.hs, self.kv, self.label, self.pos = {}, {}, {}, {}, {}
        self.boundary = []          # the labelled keys, in the order they were made
        self.missing = {}           # key -> references of its base that it lacks (the -1 exceptions)
        self.misses = []            # (chains) (position, hash) of k-mers that are no keys but walk an overflow chain
        self.filler = {}
        for r in range(nref):
            if dup and r == dup[1]:
                continue
            twin = dup and r == dup[0]
            self.filler[r] = [self.add(self.text.take(), {r: 1}, "pair" if twin else "single_once", "pair" if twin else "reference")
                              for _ in range(nfill)]
        if dup:
            self.filler[dup[1]] = self.filler[dup[0]]

    def add(self, pos, post, hs, kv, label=None):
        """a key at the k-mer of text position `pos`; post without the second twin (it follows the first); hs, kv: the forms it is meant to take"""
        h = int(self.text.h[pos])
        assert h not in self.post and h != 0
        post = dict(post)
        if self.dup:
            assert self.dup[1] not in post
            if self.dup[0] in post:
                post[self.dup[1]] = post[self.dup[0]]
        assert all(0 <= r < self.nref and m >= 1 for r, m in post.items())
        self.post[h], self.hs[h], self.kv[h], self.pos[h] = post, hs, kv, pos
        if label:
            self.label[h] = label
            self.boundary.append(h)
        return h

    def finish(self):
        self.by_ref = [dict() for _ in range(self.nref)]
        for h, post in self.post.items():
            for r, m in post.items():
                self.by_ref[r][h] = m
        self.sk = np.zeros((self.nref, self.S), dtype=np.uint64)
        self.ln = np.zeros(self.nref, dtype=np.int32)
        for r in range(self.nref):
            self._write_row(r, self.by_ref[r])
        return self

    def _write_row(self, r, keys):
        hs = sorted(keys)
        row = np.repeat(np.array(hs, dtype=np.uint64), [keys[h] for h in hs])
        assert len(row) <= self.S, (self.name, r, len(row))
        self.sk[r] = 0
        self.sk[r, : len(row)] = row
        self.ln[r] = len(row)

    def rows(self, refs=None):
        """the references' sketches as ascending arrays (tile_cases' form)"""
        return [self.sk[r, : int(self.ln[r])] for r in (range(self.nref) if refs is None else refs)]

    def hit_rows(self, h):
        """the rows of the references that hold any hash of h: the only ones tile_cases.may_hand_back's answer depends on"""
        refs = sorted({r for x in set(h.tolist()) if x in self.post for r in self.post[x]})
        return self.rows(refs or [0])

    class _Mutated:
        def __init__(self, panel, h, post):
            self.p, self.h, self.new = panel, h, post

        def __enter__(self):
            p = self.p
            self.touched = sorted(set(p.post.get(self.h, {})) | set(self.new))
            for r in self.touched:
                keys = dict(p.by_ref[r])
                keys.pop(self.h, None)
                if r in self.new:
                    keys[self.h] = self.new[r]
                p._write_row(r, keys)
            return p

        def __exit__(self, *a):
            for r in self.touched:
                self.p._write_row(r, self.p.by_ref[r])

    def mutated(self, h, post):
        """with panel.mutated(h, post): the sketches as they would be if key h had the postings `post` (h may be a new key)"""
        return Panel._Mutated(self, h, post)

    def counts(self, which):
        c = collections.Counter((self.hs if which == "hs" else self.kv).values())
        return {f: c.get(f, 0) for f in (HS_FORMS if which == "hs" else KV_FORMS)}


def _spread(rng, n, lo, hi, avoid):
    """n references from [lo, hi) that cover all four residues mod 4, none of `avoid`"""
    while True:
        refs = sorted(set(rng.choice(np.arange(lo, hi), size=n, replace=False).tolist()))
        if len({r & 3 for r in refs}) == 4 and not set(refs) & set(avoid):
            return refs


def _once(refs):
    return {r: 1 for r in refs}


ALL12 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11)     # every reference of `forms` but the second twin, which follows the first


@functools.lru_cache(maxsize=None)
def _forms(orc):
    P = Panel("forms", orc, 12, 2000, 1601, 8000, 4, (5, 9))
    T = P.text
    P.add(T.take(), {0: 1}, "single_once", "reference", "once@0")
    P.add(T.take(), {11: 1}, "single_once", "reference", "once@11")
    for r, m in ((1, 2), (2, 3), (3, 30), (4, 31)):
        P.add(T.take(), {r: m}, "single_multi", "single_multi", "mult%d" % m)
    P.add(T.a_at, {6: 511}, "single_multi", "single_multi", "mult511")
    P.add(T.c_at, {7: 512}, "list", "plain", "mult512")                   # one entry too many for the 9-bit field: a one-entry list
    P.add(T.take(), _once((1, 10)), "pair", "pair", "pair")
    P.add(T.take(), {2: 1, 8: 2}, "list", "plain", "two(1,2)")
    for refs in ((0, 3, 7), (1, 4, 6, 10), (0, 2, 6, 8, 11), (1, 3, 4, 7, 8, 10)):
        P.add(T.take(), _once(refs), "list", "inline", "list%d" % len(refs))
    P.add(T.take(), _once((0, 1, 2, 3, 4, 6, 7)), "list", "plain", "list7")
    P.add(T.take(), {3: 1, 6: 2, 10: 1}, "list", "plain", "list3(2)")
    P.add(T.take(), _once(ALL12), "list", "plain", "list12")               # (with the twin: all 12)
    t = T.tandem_at                                                            # tandem keys: ranks above 0 meet entries of different multiplicity
    P.add(t + 0, {0: 1, 4: 3, 8: 40}, "list", "plain", "tandem(1,3,40)")
    P.add(t + 5, {2: 2, 7: 30}, "list", "plain", "tandem(2,30)")
    P.add(t + 9, {1: 31}, "single_multi", "single_multi", "tandem31")
    P.add(t + 13, {3: 40}, "single_multi", "single_multi", "tandem40")
    P.add(t + 17, _once((6, 10)), "pair", "pair", "tandem pair")
    P.add(t + 21, _once((1, 2, 11)), "list", "inline", "tandem list3")
    # ballast: the one simple list of >= 8 references (list12) would become a base unless the bases save under 5 % of all postings
    for j in range(20):
        post = _once(ALL12)
        post[(0, 1, 2, 3, 4, 6, 7, 8, 10, 11)[j % 10]] = 2
        P.add(T.take(), post, "list", "plain")
    return P.finish()


@functools.lru_cache(maxsize=None)
def _wide_ids(orc):
    P = Panel("wide_ids", orc, 2100, 256, 1602, 40000, 2, (700, 701))
    T = P.text
    rng = np.random.default_rng(2100)
    P.add(T.take(), _once((5, 2047)), "pair", "pair", "pair(5,2047)")
    P.add(T.take(), _once((5, 2048)), "list", "plain", "pair(5,2048)")
    P.add(T.take(), _once((2047, 2048)), "list", "plain", "pair(2047,2048)")
    P.add(T.take(), _once((1, 2, 511)), "list", "inline", "list(1,2,511)")
    P.add(T.take(), _once((1, 2, 512)), "list", "plain", "list(1,2,512)")
    # four long lists, far from one another: each becomes a base and is its own (base, no exceptions) value -- which the sparse rows
    # cannot use (they cannot subtract), so the k-mer-space kernel walks the plain form kept beside it
    for n in (15, 16, 17, 33):
        P.add(T.take(), _once(_spread(rng, n, 3, 2099, (700, 701))), "list", "base_inline", "list%d" % n)
    P.add(T.take(), {2099: 1}, "single_once", "reference", "once@2099")
    return P.finish()


FAM_A, FAM_B = tuple(range(24)), tuple(range(24, 36))


@functools.lru_cache(maxsize=None)
def _families(orc):
    """The (base, exceptions) forms.  A list becomes a base of its own whenever it is far from every base chosen and a slot is free,
    and a list of 24 at distance > 6 from FAM_A IS far: such a list is only ever stored against FAM_A when all eight slots are taken
    by heavier lists.  So the panel has eight: FAM_A (60 keys), FAM_B (40) and six decoys of 16 references carried by three keys each."""
    P = Panel("families", orc, 40, 2000, 1603, 8000, 4, (38, 39))
    T = P.text
    rng = np.random.default_rng(40)
    A, B = set(FAM_A), set(FAM_B)
    a_keys = [P.add(T.take(), _once(A), "list", "base_inline") for _ in range(60)]
    b_keys = [P.add(T.take(), _once(B), "list", "base_inline") for _ in range(40)]
    decoys = []
    while len(decoys) < 6:
        d = set(rng.choice(38, size=16, replace=False).tolist())
        if all(len(d ^ x) > 12 for x in [A, B] + decoys):
            decoys.append(d)
    for d in decoys:
        for _ in range(3):
            P.add(T.take(), _once(d), "list", "base_inline")

    def variant(base, minus, plus, kv, label):
        h = P.add(T.take(), _once((set(base) - set(minus)) | set(plus)), "list", kv, label)
        P.missing[h] = tuple(minus)
        return h
    for h, label in ((a_keys[0], "A"), (a_keys[1], "A'"), (b_keys[0], "B")):
        P.label[h] = label
        P.boundary.append(h)
    variant(A, (), (36,), "base_inline", "A+1")
    variant(A, (7,), (), "base_inline", "A-1")
    variant(A, (1, 2, 3, 4), (24, 25, 36, 37), "base_inline", "A+4-4")               # 8 exceptions: the last that fit the value
    variant(A, (5, 6, 8, 9), (26, 27, 28, 36, 37), "base_list", "A+5-4")             # 9: a (base, exceptions) list
    variant(A, (10, 11, 12, 13, 14), (29, 30, 31, 32, 36, 37), "base_list", "A+6-5")  # 11: 2 (1 + 11) <= 25
    variant(A, (15, 16, 17, 18, 19, 20), (24, 26, 28, 30, 32, 34), "plain", "A+6-6")  # 12: 2 (1 + 12) > 24
    post = _once(A)
    post[3] = 2
    P.add(T.take(), post, "list", "plain", "A(3 twice)")                                # not simple: never gets a base
    variant(B, (), (37,), "base_inline", "B+1")                                         # base number 1
    variant(B, (30,), (), "base_inline", "B-1")
    last = sorted(decoys[5])
    variant(last, (last[0],), (next(r for r in range(38) if r not in decoys[5]),), "base_inline", "decoy+1-1")   # a base beyond the first two
    P.decoys = [tuple(sorted(d)) for d in decoys]
    return P.finish()


CHAIN_LAST, CHAIN_MID = 255, 100
CHAIN_POSTS = ({0: 1}, {1: 1}, {0: 1, 1: 1}, {0: 2}, {1: 3})


@functools.lru_cache(maxsize=None)
def _chains(orc):
    P = Panel("chains", orc, 2, 2000, 1604, 40000, 60, None)
    T = P.text
    # (the fillers were taken first: they must stay out of the buckets the chains run through)
    near = set(range(CHAIN_LAST - 1, CHAIN_LAST + 1)) | set(range(0, 6)) | set(range(CHAIN_MID - 1, CHAIN_MID + 6))
    for h in [h for h in list(P.post) if ((h >> 32) & 255) in near]:
        for d in (P.post, P.hs, P.kv, P.pos):
            del d[h]
        for r in (0, 1):
            P.filler[r] = [x for x in P.filler[r] if x != h]
    n = 0
    for bucket, cnt in ((CHAIN_LAST, 19), (0, 8), (CHAIN_MID, 17)):
        for _ in range(cnt):
            post = CHAIN_POSTS[n % len(CHAIN_POSTS)]
            hs = hash_form(post)
            P.add(T.take(lambda h: ((h >> 32) & 255) == bucket), post, hs, "reference" if hs == "single_once" else hs, "bucket%d #%d" % (bucket, n))
            n += 1
    for bucket in (CHAIN_LAST, 0, 1, CHAIN_MID):
        for _ in range(6):
            p = T.take(lambda h: ((h >> 32) & 255) == bucket)
            P.misses.append((p, int(T.h[p])))
    assert len(P.post) < 640
    return P.finish()


PANELS = ("forms", "wide_ids", "families", "chains")


def panel(orc, name):
    return {"forms": _forms, "wide_ids": _wide_ids, "families": _families, "chains": _chains}[name](orc)


# ---- reads ---------------------------------------------------------------------------------------------------------------------------------
def _join(kmers):
    """k-mers joined by N and closed by one: under windows=len-k every k-mer is exactly one valid window"""
    return b"N".join(kmers) + b"N"


def _occurrences(P, h, n):
    """text that holds key h exactly n times and no other valid window: its k-mer n times, or -- a run's key -- a run of n windows"""
    T = P.text
    if P.pos[h] in (T.a_at, T.c_at):
        return [T.text[P.pos[h]: P.pos[h] + 1] * (K + n - 1)]
    return [T.kmer(P.pos[h])] * n


def _probe(P, h, m, n):
    """key h n times and enough private keys of reference m that m is the read's unique maximum (but for its twin)"""
    post = P.post[h]
    others = max([min(n, mu) for r, mu in post.items() if r != m and not (P.dup and {r, m} == set(P.dup))] + [0])
    f = max(1, others - min(n, post.get(m, 0)) + 1)
    assert f <= len(P.filler[m]), (P.name, P.label.get(h), m, f)
    return _join(_occurrences(P, h, n) + [P.text.kmer(P.pos[x]) for x in P.filler[m][:f]])


Reads = collections.namedtuple("Reads", "one cuts tandem runs probes long probe_of")


@functools.lru_cache(maxsize=None)
def reads(orc, name):
    """the read sets of a panel (tuples of bytes); .probe_of: (key, reference) -> the places of its probes in short() and in .long"""
    P = panel(orc, name)
    T = P.text
    rng = np.random.default_rng(9000 + len(name))
    one = [T.text[P.pos[h]: P.pos[h] + K + 1] for h in P.boundary] + [T.text[p: p + K + 1] for p, _ in P.misses]
    cuts = [T.text[p: p + 150] for p in rng.integers(0, len(T.text) - 150, 36).tolist()]
    cuts += [T.text[a - 40: a + 110] for a in (T.tandem_at, T.a_at, T.c_at)] + [T.text[a + RUN - 100: a + RUN + 50] for a in (T.a_at, T.c_at)]
    if P.S >= 400:                                                     # more than 255 windows: 16-bit counter fields
        cuts += [T.text[p: p + 400] for p in rng.integers(0, T.nrand - 400, 3).tolist()]
    tandem, runs, long_ = [], [], []
    if name == "forms":
        for n in (1, 2, 29, 30, 31):                                   # the key at the repeat's first base n times, the other phases n - 1 or n
            tandem.append(T.text[T.tandem_at: T.tandem_at + UNIT_LEN * (n - 1) + K + 1])
        for at in (T.a_at, T.c_at):
            for n in (510, 511, 512, 513):
                runs.append(T.text[at: at + 1] * (K + n))              # n windows of the run
                long_.append(T.text[at - 1100: at] + runs[-1][:-1] + T.text[at + RUN: at + RUN + 100])   # (no last window is dropped inside a read)
    for L in (1600, 1777, 2016, 2017, 2200, 2400):
        p = int(rng.integers(0, len(T.text) - L))
        long_.append(T.text[p: p + L])
    long_.append(T.text[T.tandem_at - 400: T.tandem_at + UNIT_LEN * UNIT_COPIES + 400])
    probes, probe_of = [], {}
    base = len(one) + len(cuts) + len(tandem) + len(runs)

    def add_probe(h, m, n):
        r = _probe(P, h, m, n)
        if len(r) <= tc.FUSED_MAXLEN and len(r) - K <= P.S:
            probe_of.setdefault((h, m), []).append(("short", base + len(probes)))
            probes.append(r)
        probe_of.setdefault((h, m), []).append(("long", len(long_)))
        long_.append(r + b"N" * (LONG_MIN + 17 * (len(long_) % 48) - len(r)))
    for h in P.boundary:
        for m, mu in sorted(P.post[h].items()):
            add_probe(h, m, mu + 1)
            if mu + 1 > 30:
                add_probe(h, m, 1)                                      # its presence, in a read the hash-space kernel answers itself
            if mu == 30:
                add_probe(h, m, 30)                                     # the most occurrences the hash-space kernel's hit set counts
        for m in P.missing.get(h, ()):
            add_probe(h, m, 1)
    for p, _ in P.misses:                                               # the misses, where the general path looks them up
        long_.append(_join([T.kmer(p)]) + b"N" * (LONG_MIN + 17 * (len(long_) % 48) - K - 1))
    assert all(LONG_MIN <= len(r) <= LONG_MAX for r in long_)
    return Reads(tuple(one), tuple(cuts), tuple(tandem), tuple(runs), tuple(probes), tuple(long_), probe_of)


def short(rd):
    return rd.one + rd.cuts + rd.tandem + rd.runs + rd.probes


def batches(rd):
    """the short reads as the batches the GPU test classifies: those of <= 255 windows (8-bit counter fields; dense rows only), then all"""
    s = short(rd)
    small = [i for i, r in enumerate(s) if tc.nwin(len(r), K) <= 255]
    return [small, list(range(len(s)))] if len(small) < len(s) else [small]


def hashes(orc, seqs):
    return [tc.window_hashes(orc, r, KS, POL) for r in seqs]


def want_rows(orc, P, seqs, min_occ=None, threads=8):
    """the oracle's plain merge on the panel's rows as they are now"""
    qb, qo = tc.pack(list(seqs))
    if min_occ is None:
        return orc.classify_stream(qb, qo, KS, P.S, P.sk, P.ln, POL.oracle(orc), threads=threads)
    return orc.classify_stream(qb, qo, KS, P.S, P.sk, P.ln, POL.oracle(orc), threads=threads, min_kmer_occ=min_occ, counter_slots=COUNT_SLOTS)


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------
def _with(post, m, mult):
    new = dict(post)
    new[m] = mult
    return new


Mutation = collections.namedtuple("Mutation", "what key ref post high")


def mutations(P):
    """The neighbouring mistake at every labelled key: (what, key, the reference it concerns, the key's postings after it, high).
    high: the old or the new multiplicity is above 30.  Changes that change nothing (an id masked to itself, an id pushed out of the
    panel) are no mutations and are left out."""
    out = []
    for h in P.boundary:
        post = P.post[h]
        for m, mu in sorted(post.items()):
            def put(what, new, high=False):
                new = {r: c for r, c in new.items() if c > 0}
                if new != post and all(0 <= r < P.nref for r in new):
                    out.append(Mutation(what, h, m, new, high))
            second_twin = bool(P.dup) and m == P.dup[1]     # its decrease shows in no row: see tests/test_index_cases_cpu.py
            if not second_twin:
                put("multiplicity-1", _with(post, m, mu - 1), mu > 30)
            put("multiplicity+1", _with(post, m, mu + 1), mu + 1 > 30)
            if len(post) > 1 and not second_twin:
                put("dropped", _with(post, m, 0))
            for what, m2 in (("id-1", m - 1), ("id+1", m + 1), ("id&511", m & 511), ("id&2047", m & 2047)):
                if m2 != m and 0 <= m2 < P.nref:
                    new = _with(post, m, 0)
                    new[m2] = new.get(m2, 0) + mu
                    put(what, new)
        # a sign flipped: a +1 exception counted as -1 shows no later than the member dropped (above); a -1 exception counted as +1
        # gives a reference the key lacks the base's posting and one more
        for m in P.missing.get(h, ()):
            out.append(Mutation("sign", h, m, _with(post, m, 2), False))
    if P.misses:
        fill = bucket_fill(P.post)
        for p, mh in P.misses:
            home = (mh >> 32) & (fill.nb - 1)
            chain = [h for h, (hm, b) in fill.stored.items() if hm == home] or [h for h, (hm, b) in fill.stored.items() if b == home]
            last = max(chain, key=lambda h: ((fill.stored[h][1] - home) & (fill.nb - 1), h))
            out.append(Mutation("miss->hit", mh, None, dict(P.post[last]), False))
    return out
