"""Host model of ks_spectra_knn: a numpy transcription of the contract in
include/kmer_spans.h.  The GPU tests compare index bit for bit, and dist bit
for bit when squared.

The profiles and the squared distance are those of tests/kmeansref.py (the
inner loop of ks_spectra_dist, one rounding per operation); the selection is
np.lexsort on (acc, position), the total order of the contract."""
import numpy as np

from tests.kmeansref import profiles, sqdist

MAX_K = 64  # KS_KNN_MAX_K


def select(acc, k, exclude=None) -> tuple:
    """(index int64 [na, k], acc float64 [na, k]) of acc [na, nb]: per query the
    k candidates with the smallest (acc, position), ascending.  exclude: per
    query the one candidate position left out of its list (the self form:
    exclude[s] = s), or None."""
    acc = np.asarray(acc, dtype=np.float64)
    na, nb = acc.shape
    assert 1 <= k <= MAX_K and k <= (nb if exclude is None else nb - 1), "k exceeds the number of candidate rows"
    pos = np.arange(nb, dtype=np.int64)
    index = np.empty((na, k), dtype=np.int64)
    for s in range(na):
        order = np.lexsort((pos, acc[s]))  # by acc, ties by position
        if exclude is not None:
            order = order[order != exclude[s]]
        index[s] = order[:k]
    return index, np.take_along_axis(acc, index, axis=1)


def knn(counts, k, rows=None, rows_b=None, squared=False) -> tuple:
    """(index, dist) as ks_spectra_knn returns them."""
    pa = profiles(counts, rows)
    self_form = rows_b is None
    pb = pa if self_form else profiles(counts, rows_b)
    index, acc = select(sqdist(pa, pb), k, np.arange(pa.shape[0]) if self_form else None)
    return index, (acc if squared else np.sqrt(acc))
