"""Host model of ks_spectra_kmeans / ks_spectra_group_means: a numpy
transcription of the contract in include/kmer_spans.h, sentence by sentence.
The GPU tests compare every output against it bit for bit.

numpy rounds each elementwise FP64 operation once and np.cumsum adds strictly
left to right, so each piece below performs the header's operations in the
header's order (the plain Python loops of tests/test_kmeans.py pin that)."""
import numpy as np

CHUNK = 256  # KS_KM_CHUNK


def profiles(counts, rows=None) -> np.ndarray:
    """p[s][c] = (double)cnt / (double)T, T the row's integer sum."""
    c = np.asarray(counts)
    if rows is not None:
        c = c[np.asarray(rows, dtype=np.int64)]
    c = c.astype(np.uint64)
    tot = c.sum(axis=1, dtype=np.uint64)
    assert (tot > 0).all(), "a selected row has no counts"
    return c.astype(np.float64) / tot.astype(np.float64)[:, None]


def sum_in_order(x) -> np.ndarray:
    """Sums along the first axis of x [k, ...], left to right from +0.0."""
    x = np.asarray(x, dtype=np.float64)
    return np.cumsum(np.concatenate([np.zeros((1,) + x.shape[1:]), x], axis=0), axis=0)[-1]


def sqdist(p, cen) -> np.ndarray:
    """acc[s][j]: acc = +0.0; for c ascending: d = p[s][c] - cen[j][c]; acc = acc + d * d."""
    p, cen = np.asarray(p, dtype=np.float64), np.asarray(cen, dtype=np.float64)
    acc = np.zeros((p.shape[0], cen.shape[0]))
    for c in range(p.shape[1]):
        d = p[:, c][:, None] - cen[:, c][None, :]
        acc = acc + d * d
    return acc


def assign(acc) -> np.ndarray:
    """The j with the smallest acc, j ascending with a strict <: the first minimum.  Labels 1 .. g."""
    return (np.argmin(acc, axis=1) + 1).astype(np.int32)


def chunked_sum(v, chunk=CHUNK) -> np.ndarray:
    """The group sum of the members' values v [k, ...] (ascending position order):
    a partial per `chunk` consecutive members, the partials added in order.
    chunk=None: the plain left-to-right sum (the order the contract does NOT use)."""
    v = np.asarray(v, dtype=np.float64)
    if chunk is None:
        return sum_in_order(v)
    parts = [sum_in_order(v[t:t + chunk]) for t in range(0, v.shape[0], chunk)]
    return sum_in_order(np.stack(parts)) if parts else np.zeros(v.shape[1:])


def update(p, label, cen, empty="keep", chunk=CHUNK) -> np.ndarray:
    """cen[j][c] = S_j[c] / (double)n_j; a group without members keeps its row or gets NaN."""
    new = np.array(cen, dtype=np.float64, copy=True)
    for j in range(new.shape[0]):
        mem = np.flatnonzero(label == j + 1)
        if mem.size:
            new[j] = chunked_sum(p[mem], chunk) / np.float64(mem.size)
        elif empty == "nan":
            new[j] = np.nan
    return new


def withinss(p, label, cen) -> np.ndarray:
    """The group sum of acc(s, j) over the members of j against cen, +0.0 for an empty group."""
    g = cen.shape[0]
    out = np.zeros(g)
    for j in range(g):
        mem = np.flatnonzero(label == j + 1)
        if mem.size:
            out[j] = chunked_sum(sqdist(p[mem], cen[j:j + 1])[:, 0])
    return out


def totss(p) -> float:
    """The single group of all rows: its chunked centre, then its chunked sum."""
    cen = (chunked_sum(p) / np.float64(p.shape[0]))[None, :]
    return float(chunked_sum(sqdist(p, cen)[:, 0]))


def group_means(counts, group, ngroups=None, rows=None) -> dict:
    p = profiles(counts, rows)
    group = np.asarray(group, dtype=np.int64)
    g = int(group.max()) if ngroups is None else int(ngroups)
    assert group.shape == (p.shape[0],) and group.min() >= 1 and group.max() <= g
    cen = update(p, group, np.zeros((g, p.shape[1])), empty="nan")
    return {"centers": cen, "size": np.bincount(group, minlength=g + 1)[1:].astype(np.int32),
            "withinss": withinss(p, group, cen)}


def kmeans(counts, centers, rows=None, iter_max=10) -> dict:
    """R's kmeans_Lloyd: labels start at 0; per pass assign, stop if nothing
    changed, otherwise recompute every centre (also after the last pass)."""
    p = profiles(counts, rows)
    centers = np.asarray(centers)
    if centers.ndim == 1:  # positions of the selection: those rows' profiles
        cen = p[centers.astype(np.int64)].copy()
    else:
        cen = np.array(centers, dtype=np.float64, copy=True)
    assert np.isfinite(cen).all() and iter_max >= 1
    g = cen.shape[0]
    label = np.zeros(p.shape[0], dtype=np.int32)
    it, converged = 0, False
    for it in range(1, iter_max + 1):
        new = assign(sqdist(p, cen))
        changed = bool((new != label).any())
        label = new
        if not changed:
            converged = True
            break
        cen = update(p, label, cen)
    wss = withinss(p, label, cen)
    tot = float(sum_in_order(wss))
    tss = totss(p)
    return {"cluster": label, "centers": cen, "size": np.bincount(label, minlength=g + 1)[1:].astype(np.int32),
            "withinss": wss, "tot_withinss": tot, "totss": tss, "betweenss": tss - tot, "iter": it,
            "converged": converged}
