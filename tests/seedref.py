"""Host model of ks_spectra_kmeans_seed: a numpy transcription of the contract
in include/kmer_spans.h, sentence by sentence, built on kmeansref's profiles,
sqdist and chunked_sum.  The GPU tests compare every output against it bit for
bit; the plain Python loops of tests/test_kmeans_seed.py pin the model itself."""
import numpy as np

from tests import kmeansref as KR

CHUNK = KR.CHUNK  # KS_KM_CHUNK
U_MAX = 1.0 - 2.0 ** -53  # the largest double below 1


def chunk_prefix(mind, chunk=CHUNK):
    """(C, P): C[c] the chunk's left-to-right sum from +0.0, P[0] = +0.0,
    P[c + 1] = P[c] + C[c].  chunk=None: one chunk of all rows (the plain
    left-to-right order the contract does NOT use)."""
    mind = np.asarray(mind, dtype=np.float64)
    if chunk is None:
        chunk = max(mind.size, 1)
    C = np.array([KR.sum_in_order(mind[t:t + chunk]) for t in range(0, mind.size, chunk)], dtype=np.float64)
    P = np.cumsum(np.concatenate([[0.0], C]))
    return C, P


def dsq_pick(mind, uj, chunk=CHUNK):
    """(position, pot) of a D^2 pick from the uniform number uj."""
    mind = np.asarray(mind, dtype=np.float64)
    if chunk is None:
        chunk = max(mind.size, 1)
    C, P = chunk_prefix(mind, chunk)
    pot = P[-1]
    if pot == 0.0:
        return 0, pot
    t = np.float64(uj) * pot
    hit = np.flatnonzero(P[1:] > t)
    assert hit.size, "no chunk: u is not below 1"
    cs = int(hit[0])
    # acc = +0.0; acc = acc + mind[s], s ascending: the running sums of the chunk
    acc = np.cumsum(np.concatenate([[0.0], mind[cs * chunk:(cs + 1) * chunk]]))[1:]
    inside = np.flatnonzero(P[cs] + acc > t)
    assert inside.size, "no row inside the chunk"
    return cs * chunk + int(inside[0]), pot


def seed(counts, g, method="maximin", rows=None, first=0, u=None, chunk=CHUNK) -> dict:
    p = KR.profiles(counts, rows)
    m, g = p.shape[0], int(g)
    assert g >= 1 and method in ("maximin", "kmeans++")
    dsq = method == "kmeans++"
    if dsq:
        u = np.asarray(u, dtype=np.float64)
        assert u.shape == (g,) and ((u >= 0) & (u < 1)).all()
    else:
        assert u is None
    if first is None or first == -1:
        assert dsq
        first = int(u[0] * np.float64(m))
    assert 0 <= first < m
    mind = np.full(m, np.inf)
    near = np.zeros(m, dtype=np.int32)
    picked = np.zeros(g, dtype=np.int64)
    pick_dist = np.full(g, np.inf)
    potential = np.full(g, np.inf)
    for j in range(g):
        if j == 0:
            r = first
        elif dsq:
            r, pot = dsq_pick(mind, u[j], chunk)
            pick_dist[j], potential[j] = mind[r], pot
        else:
            r = int(np.argmax(mind))  # the first maximum: the lowest position on a tie
            pick_dist[j], potential[j] = mind[r], chunk_prefix(mind, chunk)[1][-1]
        picked[j] = r
        acc = KR.sqdist(p, p[r:r + 1])[:, 0]
        lower = acc < mind
        mind = np.where(lower, acc, mind)
        near = np.where(lower, np.int32(j + 1), near).astype(np.int32)
    pot = KR.chunked_sum(mind, chunk)
    assert chunk is None or pot.tobytes() == chunk_prefix(mind, chunk)[1][-1].tobytes()
    far = int(np.argmax(mind))
    return {"rows": picked, "nearest": near, "mindist": mind, "pick_dist": pick_dist, "potential": potential,
            "n_distinct": 1 + int((pick_dist[1:] > 0).sum()), "potential_final": float(pot),
            "radius": float(mind[far]), "far_row": far}

