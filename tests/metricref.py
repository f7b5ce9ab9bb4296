"""Host model of the metric field of the distance flags (KS_DIST_METRIC_MASK,
include/kmer_spans.h): one function per metric, each the header's loop over k
written out, vectorised over the pairs as ref_sq of tests/test_spectra_dist.py
is.  numpy rounds every operation on its own (no FMA), np.sqrt is correctly
rounded, and every pair has one accumulator, so the GPU tests compare bits.

Every function takes the profile matrix p [m, ncol] (profiles(): counts / row
sum, NaN rows where the sum is 0) and the pairs (i[x], j[x]) and returns the
VALUE of each pair: what ks_spectra_knn ranks by and the last step starts
from.  result() is that last step."""
import numpy as np

from tests.test_spectra_dist import condensed_pairs, profiles

METRICS = ("euclidean", "manhattan", "maximum", "canberra", "hellinger")
HAS_SQUARED = ("euclidean", "hellinger")


def _columns(p, i, j):
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    return np.ascontiguousarray(np.asarray(p, dtype=np.float64).T), i, j


def euclidean(p, i, j) -> np.ndarray:
    """acc = 0; for k ascending: d = p_i[k] - p_j[k]; acc = acc + d * d."""
    pt, i, j = _columns(p, i, j)
    acc = np.zeros(i.size, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(pt.shape[0]):
            d = pt[k][i] - pt[k][j]
            acc = acc + d * d
    return acc


def manhattan(p, i, j) -> np.ndarray:
    """acc = 0; for k ascending: acc = acc + |p_i[k] - p_j[k]|."""
    pt, i, j = _columns(p, i, j)
    acc = np.zeros(i.size, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        for k in range(pt.shape[0]):
            acc = acc + np.abs(pt[k][i] - pt[k][j])
    return acc


def maximum(p, i, j) -> np.ndarray:
    """acc = 0; for k ascending: t = |p_i[k] - p_j[k]|; acc = t > acc ? t : acc;
    a NaN t makes the result NaN."""
    pt, i, j = _columns(p, i, j)
    acc = np.zeros(i.size, dtype=np.float64)
    nan = np.zeros(i.size, dtype=bool)
    with np.errstate(invalid="ignore"):
        for k in range(pt.shape[0]):
            t = np.abs(pt[k][i] - pt[k][j])
            nan |= np.isnan(t)
            acc = np.where(t > acc, t, acc)
    return np.where(nan, np.nan, acc)


def canberra(p, i, j) -> np.ndarray:
    """for k ascending: s = p_i[k] + p_j[k]; s == 0: the column is omitted;
    otherwise acc = acc + |p_i[k] - p_j[k]| / s, cnt = cnt + 1.  The value is
    acc if cnt == ncol, otherwise acc / ((double)cnt / (double)ncol)."""
    pt, i, j = _columns(p, i, j)
    ncol = pt.shape[0]
    acc = np.zeros(i.size, dtype=np.float64)
    cnt = np.zeros(i.size, dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(ncol):
            s = pt[k][i] + pt[k][j]
            keep = s != 0.0  # a NaN s is kept: acc becomes NaN
            q = np.abs(pt[k][i] - pt[k][j]) / s
            acc = np.where(keep, acc + q, acc)
            cnt = cnt + keep
        scaled = acc / (cnt.astype(np.float64) / np.float64(ncol))
    return np.where(cnt == ncol, acc, scaled)


def canberra_count(p, i, j) -> np.ndarray:
    """cnt of canberra(): the columns of each pair that are not omitted."""
    pt, i, j = _columns(p, i, j)
    with np.errstate(invalid="ignore"):
        return sum(((pt[k][i] + pt[k][j]) != 0.0).astype(np.int64) for k in range(pt.shape[0]))


def hellinger(p, i, j) -> np.ndarray:
    """q[k] = sqrt(p[k]), one correctly rounded root per entry; the Euclidean
    loop over q."""
    with np.errstate(invalid="ignore"):
        return euclidean(np.sqrt(np.asarray(p, dtype=np.float64)), i, j)


VALUE = {"euclidean": euclidean, "manhattan": manhattan, "maximum": maximum, "canberra": canberra,
         "hellinger": hellinger}


def result(metric: str, value, squared: bool = False) -> np.ndarray:
    """The distance returned for a value: euclidean value or sqrt(value),
    hellinger 0.5 * value or sqrt(0.5 * value), the others the value."""
    value = np.asarray(value, dtype=np.float64)
    assert metric in METRICS and not (squared and metric not in HAS_SQUARED)
    if metric in HAS_SQUARED:
        v = value if metric == "euclidean" else 0.5 * value
        with np.errstate(invalid="ignore"):
            return v if squared else np.sqrt(v)
    return value


def before_root(metric: str, value) -> np.ndarray:
    """What a final root, if the plain form of the metric has one, is taken of."""
    value = np.asarray(value, dtype=np.float64)
    return 0.5 * value if metric == "hellinger" else value


def condensed_value(metric: str, counts, rows=None) -> np.ndarray:
    p = profiles(counts)
    if rows is not None:
        p = p[np.asarray(rows, dtype=np.int64)]
    return VALUE[metric](p, *condensed_pairs(p.shape[0]))


def cross_value(metric: str, counts, rows_a, rows_b) -> np.ndarray:
    p = profiles(counts)
    a = np.arange(p.shape[0]) if rows_a is None else np.asarray(rows_a, dtype=np.int64)
    b = np.arange(p.shape[0]) if rows_b is None else np.asarray(rows_b, dtype=np.int64)
    ii, jj = np.meshgrid(a, b, indexing="ij")
    return VALUE[metric](p, ii.ravel(), jj.ravel()).reshape(a.size, b.size)
