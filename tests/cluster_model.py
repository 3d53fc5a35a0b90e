"""Cluster (rk_cluster_hits*, rk_cluster_scaled, `rkmh cluster`) in pure Python and numpy, from the definitions in
include/rkmh_amd.h, "CLUSTER" -- it calls neither the library nor the oracle.  Two implementations that share only the link test's
wording:

  links           which hits link, by the definition, in Python integers (no width: nothing can wrap)
  union_find      labels from a plain-Python union-find over the linking hits
  links_np        the same test on whole arrays in int64
  propagate       labels from a numpy min-label propagation to its fixpoint (np.minimum.at over both directions of every link of links_np)
  members         the clusters of a label array: (cl_off, members, rep) as rk_cluster_members lays them out
  cluster_text    the lines of `rkmh cluster`
  ppm             a decimal string of at most six digits after the point -> parts per million, exactly
Pinned by tests/golden/cluster_kat.json."""
import numpy as np

JACCARD, MAX_CONTAINMENT = 0, 1


def links(hits, lens, measure, min_ppm):
    """-> list of (i, j) for every hit that links, in hit order (duplicates stay)"""
    assert measure in (JACCARD, MAX_CONTAINMENT) and 0 <= min_ppm <= 1000000
    n, out = len(lens), []
    for i, j, shared in np.asarray(hits, dtype=np.int64).reshape(-1, 3).tolist():
        if not (0 <= i < n and 0 <= j < n) or i == j or shared < 1:
            continue
        li, lj = int(lens[i]), int(lens[j])
        denom = li + lj - shared if measure == JACCARD else min(li, lj)
        if shared * 1000000 >= min_ppm * denom:
            out.append((i, j))
    return out


def union_find(hits, lens, measure=JACCARD, min_ppm=0):
    n = len(lens)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in links(hits, lens, measure, min_ppm):
        a, b = find(i), find(j)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def links_np(hits, lens, measure, min_ppm):
    """the link test once more, on whole arrays in int64 (every product stays below 2^53) -> int64 [m, 2]"""
    assert measure in (JACCARD, MAX_CONTAINMENT) and 0 <= min_ppm <= 1000000
    h = np.asarray(hits, dtype=np.int64).reshape(-1, 3)
    ln = np.asarray(lens).astype(np.int64)
    assert (ln < (1 << 31)).all()
    n = len(ln)
    h = h[(h[:, 0] >= 0) & (h[:, 0] < n) & (h[:, 1] >= 0) & (h[:, 1] < n) & (h[:, 0] != h[:, 1]) & (h[:, 2] >= 1)]
    li, lj, s = ln[h[:, 0]], ln[h[:, 1]], h[:, 2]
    denom = li + lj - s if measure == JACCARD else np.minimum(li, lj)
    return h[s * 1000000 >= min_ppm * denom][:, :2]


def propagate(hits, lens, measure=JACCARD, min_ppm=0):
    n = len(lens)
    lab = np.arange(n, dtype=np.int64)
    e = links_np(hits, lens, measure, min_ppm)
    if len(e):
        u, v = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
        while True:
            new = lab.copy()
            np.minimum.at(new, u, lab[v])
            new = new[new]                                      # (a jump: the label of my label, itself a member of my component)
            if (new == lab).all():
                break
            lab = new
    return lab.astype(np.int32)


def members(labels, lens):
    """-> (cl_off int32 [ncl + 1], members int32 [n], rep int32 [ncl])"""
    labels = [int(x) for x in labels]
    roots = sorted(set(labels))
    groups = [[i for i in range(len(labels)) if labels[i] == r] for r in roots]
    assert all(g[0] == r for g, r in zip(groups, roots))
    cl_off = np.cumsum([0] + [len(g) for g in groups]).astype(np.int32)
    rep = [min(g, key=lambda i: (-int(lens[i]), i)) for g in groups]
    return cl_off, np.array([i for g in groups for i in g], dtype=np.int32), np.array(rep, dtype=np.int32)


def cluster_text(names, lens, labels, representatives=False):
    cl_off, mem, rep = members(labels, lens)
    out = []
    for c in range(len(rep)):
        head = "%d\t%d\t%s\t" % (c, cl_off[c + 1] - cl_off[c], names[rep[c]])
        if representatives:
            out.append(head + "%d\n" % int(lens[rep[c]]))
        else:
            out.extend(head + "%s\t%d\n" % (names[i], int(lens[i])) for i in mem[cl_off[c]:cl_off[c + 1]])
    return "".join(out)


def ppm(text):
    whole, _, frac = text.partition(".")
    assert len(whole) <= 1 and len(frac) <= 6 and (whole + frac).isdigit()
    v = int(whole or "0") * 1000000 + int((frac + "000000")[:6])
    assert v <= 1000000
    return v
