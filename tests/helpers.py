import ctypes as C
import json
import os

import numpy as np


def load_refs_reads(orc, data_dir, ref_file, reads_file):
    r = orc.kseq_parse_file(os.path.join(data_dir, ref_file))
    q = orc.kseq_parse_file(os.path.join(data_dir, reads_file))
    return r, q


def golden(golden_dir, tag):
    return json.load(open(os.path.join(golden_dir, "classify_%s.json" % tag)))


def rand_dna(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tolist())


def _call_fixture(orc, data_dir, tmp_path, cov=40, seed=5, ref=None):
    """C5-like input: reads drawn from HPV16 (or from `ref`, a (name, sequence) pair of at least 7.2 kb) carrying planted SNPs
    and 1-bp deletions, 0.5 % substitution noise.  tmp_path None: nothing is written, the two paths come back as None."""
    rec = ref if ref is not None else orc.kseq_parse_file(os.path.join(data_dir, "hpv_16.fa.gz"))[0]
    ref = bytearray(orc.to_upper(rec[1]))
    rng = np.random.default_rng(seed)
    mut = bytearray(ref)
    for pos, alt in ((500, b"A"), (1200, b"C"), (2503, b"G"), (4000, b"T"), (6100, b"A")):
        mut[pos] = alt[0] if mut[pos] != alt[0] else b"ACGT"[(b"ACGT".index(alt) + 1) % 4]
    for pos in (7000, 3100):
        del mut[pos]
    n = cov * len(ref) // 150
    reads = []
    for _ in range(n):
        st = int(rng.integers(0, len(mut) - 150))
        r = bytearray(mut[st:st + 150])
        for j in np.nonzero(rng.random(150) < 0.005)[0]:
            r[j] = b"ACGT"[int(rng.integers(0, 4))]
        if rng.random() < 0.5:
            r = bytearray(bytes(r).translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1])
        reads.append(bytes(r))
    if tmp_path is None:
        return rec, reads, None, None
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">" + rec[0] + b"\n" + rec[1] + b"\n")
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    return rec, reads, fa, fq


def _through_device(gctx, path, text, slot_bytes, env):
    """every stretch of the file through a device-text slot; the records filter prints for each must equal those of the same bytes
    as plain text; returns the statuses"""
    from rkmh_amd import api
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    gz = api.Gzip.open(str(path))
    assert gz is not None and gz.first_byte() == ord("@")
    dev = api.FastqSlot(gctx, max_bytes=slot_bytes, device_text=True)
    plain = api.FastqSlot(gctx, max_bytes=slot_bytes)
    dev.set_filter_output(-1, -100)      # every read passes: the whole text comes back, as filter prints it
    statuses, at = [], 0
    try:
        ncalls = gz.plan(slot_bytes)
        for call in range(ncalls):
            st, n, off = dev.load_gzip(gz, call)
            statuses.append(st)
            if st != 0:
                break
            assert off == at, (call, off, at)
            if n == 0:
                continue
            want_text = text[off:off + n] if off + n <= len(text) else text[off:] + b"\n"
            assert len(want_text) == n
            res = dev.classify_raw(n)
            assert res.status == 0, (call, res.status)
            got = dev.filter_records(res, -1, -100)
            buf = plain.text_buffer()
            C.memmove(buf, want_text, n)
            res2 = plain.classify_raw(n)
            assert res2.status == 0 and res2.nrec == res.nrec
            assert got == plain.filter_records(res2, -1, -100), (call, off, n)
            at = off + (n if off + n <= len(text) else n - 1)
        if all(s == 0 for s in statuses):
            assert at == len(text)
    finally:
        dev.destroy(); plain.destroy(); gz.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return statuses
