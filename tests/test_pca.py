"""Principal components of region spectra (ks_spectra_pca, include/
kmer_spans.h): the host model the GPU tests compare against (tests/pcaref.py)
checked against numpy's SVD and eigvalsh and a hand-worked case, the Jacobi
schedule the library exports, and the argument checks of the host entry, which
all happen before any device use -- this file runs without a GPU."""
import numpy as np
import pytest

from tests import pcaref as R
from kmer_spans_amd._lib import KS_PCA_MAX_NCOL, KS_PCA_MAX_SWEEPS, KS_PCA_NO_CENTER


def test_constants_agree():
    assert (KS_PCA_MAX_NCOL, KS_PCA_MAX_SWEEPS, KS_PCA_NO_CENTER) == (R.KS_PCA_MAX_NCOL, R.KS_PCA_MAX_SWEEPS, 1)


# ------------------------------------------------------------ the host model

def test_model_hand_worked():
    """counts [[1,0],[0,1]] centred: center (.5, .5), G [[.5,-.5],[-.5,.5]],
    sdev (1, 0), first loading (+1, -1) / sqrt(2)."""
    r = R.ref_pca(np.array([[1, 0], [0, 1]], dtype=np.uint32))
    assert r["center"].tolist() == [0.5, 0.5]
    assert r["G"].tolist() == [[0.5, -0.5], [-0.5, 0.5]]
    assert r["sdev"].tolist() == [1.0, 0.0]
    assert r["rotation"][0, 0] > 0 and r["rotation"][1, 0] < 0
    assert np.abs(r["rotation"][:, 0] - np.array([1.0, -1.0]) / np.sqrt(2.0)).max() <= 2.0 ** -52
    assert r["n_sweeps"] == 2 and r["n_rotations"] == 1


def test_model_zero_gram():
    # m and the row sum are powers of two: every partial sum of the mean's chain is exact
    r = R.ref_pca(np.tile(np.array([[3, 1, 0, 2, 2]], dtype=np.uint32), (4, 1)))
    assert not r["G"].any() and not r["sdev"].any() and not r["x"].any()
    assert np.array_equal(r["rotation"], np.eye(5)) and (r["n_sweeps"], r["n_rotations"]) == (1, 0)


@pytest.mark.parametrize("m,ncol,center", [(40, 16, True), (40, 16, False), (9, 17, True), (130, 64, True)])
def test_model_against_numpy(m, ncol, center):
    """Tie-free input: singular values, loadings (up to the sign the rule
    fixes) and scores against numpy's SVD; eigenvalues against eigvalsh."""
    rng = np.random.default_rng(m * 1000 + ncol)
    r = R.ref_pca(R.synth_counts(rng, m, ncol), center=center)
    p = R.profiles(R.synth_counts(np.random.default_rng(m * 1000 + ncol), m, ncol))
    xc = p - p.mean(axis=0) if center else p
    u, sv, vt = np.linalg.svd(xc, full_matrices=False)
    tol = 64 * ncol * R.EPS
    k = min(m, ncol)
    # in squares: a zero singular value (the centred rank is m - 1) is an eigenvalue of rounding size, sqrt(eps) as sdev
    assert np.abs(r["sdev"][:k] ** 2 * (m - 1.0) - sv ** 2).max() <= tol * sv[0] ** 2
    assert np.abs(r["lambda"] - np.linalg.eigvalsh(r["G"])[::-1]).max() <= tol * r["lambda"][0]
    assert (np.diff(r["lambda"]) <= 0).all()
    res, orth, ev = R.eigen_errors(r["G"], r["lambda"], r["rotation"])
    assert max(res, orth, ev) <= 64 * ncol
    # the leading components are well separated here: compare them up to sign
    for j in range(3):
        gap = min(sv[j] - sv[j + 1], sv[j - 1] - sv[j] if j else np.inf) / sv[0]
        w = vt[j] if vt[j][np.argmax(np.abs(vt[j]))] > 0 else -vt[j]
        assert np.abs(r["rotation"][:, j] - w).max() <= tol / gap
        assert np.abs(r["x"][:, j] - xc @ w).max() <= tol / gap
    # the sign rule
    top = np.argmax(np.abs(r["rotation"]), axis=0)
    assert (r["rotation"][top, np.arange(ncol)] > 0).all()


def test_model_centre_and_gram_are_the_plain_loops():
    rng = np.random.default_rng(5)
    p = R.profiles(R.synth_counts(rng, 7, 5))
    acc = [0.0] * 5
    for s in range(7):
        for c in range(5):
            acc[c] = acc[c] + p[s, c]
    cen = np.array([a / 7.0 for a in acc])
    assert np.array_equal(R.bits(R.ref_center(p)), R.bits(cen))
    xc = R.ref_xc(p, cen)
    g = np.zeros((5, 5))
    for a in range(5):
        for b in range(5):
            t = 0.0
            for s in range(7):
                t = t + xc[s, a] * xc[s, b]
            g[a, b] = t
    assert np.array_equal(R.bits(R.ref_gram(xc)), R.bits(g))
    rot = rng.standard_normal((5, 3))
    x = np.zeros((7, 3))
    for s in range(7):
        for j in range(3):
            t = 0.0
            for c in range(5):
                t = t + xc[s, c] * rot[c, j]
            x[s, j] = t
    assert np.array_equal(R.bits(R.ref_scores(xc, rot)), R.bits(x))


@pytest.mark.parametrize("case", ["both_strands", "zero_columns", "rank2"])
def test_model_terminates(case):
    rng = np.random.default_rng(11)
    if case == "both_strands":  # exact duplicate columns
        c = R.synth_counts(rng, 30, 8)
        c = np.concatenate([c, c[:, ::-1]], axis=1)
    elif case == "zero_columns":
        c = R.synth_counts(rng, 30, 16)
        c[:, [3, 4, 9]] = 0
    else:
        c = R.synth_counts(rng, 3, 16)
    r = R.ref_pca(c)
    assert r["n_sweeps"] < 20
    assert max(R.eigen_errors(r["G"], r["lambda"], r["rotation"])) <= 64 * 16


# ----------------------------------------------------- the exported schedule

def _round_pairs(ncol, rnd):
    from kmer_spans_amd import _lib
    L = _lib.load()
    half = (ncol + 1) // 2
    p, q = np.full(half, -1, dtype=np.int32), np.full(half, -1, dtype=np.int32)
    cnt = L.ks_pca_round_pairs(ncol, rnd, p.ctypes.data, q.ctypes.data)
    return cnt, p, q


@pytest.mark.parametrize("ncol", list(range(1, 71)) + [1024])
def test_round_pairs(ncol):
    """Every unordered pair exactly once per sweep, pairs disjoint within a
    round, p < q < ncol, and the model's schedule is the library's."""
    big = ncol + (ncol & 1)
    seen = np.zeros((ncol, ncol), dtype=np.int32)
    for rnd in range(big - 1):
        cnt, p, q = _round_pairs(ncol, rnd)
        assert cnt == ncol // 2
        p, q = p[:cnt], q[:cnt]
        assert (p < q).all() and (p >= 0).all() and (q < ncol).all()
        both = np.concatenate([p, q])
        assert np.unique(both).size == both.size
        seen[p, q] += 1
        mp, mq = R.round_pairs(ncol, rnd)
        assert np.array_equal(mp, p) and np.array_equal(mq, q)
    assert np.array_equal(seen, np.triu(np.ones((ncol, ncol), dtype=np.int32), 1))


def test_round_pairs_bad_arguments():
    assert _round_pairs(4, -1)[0] == -1 and _round_pairs(4, 3)[0] == -1 and _round_pairs(5, 5)[0] == -1
    from kmer_spans_amd import _lib
    one = np.zeros(1, dtype=np.int32)
    assert _lib.load().ks_pca_round_pairs(0, 0, one.ctypes.data, one.ctypes.data) == -1
    assert _lib.load().ks_pca_round_pairs(KS_PCA_MAX_NCOL + 1, 0, one.ctypes.data, one.ctypes.data) == -1
    assert _round_pairs(1, 0)[0] == 0  # one column: the only pair holds the dummy


# ------------------------------------------------- host entry: validation

C8 = np.arange(1, 33, dtype=np.uint32).reshape(8, 4)


def _pca(c, rows=None, m=None, ncol=None, n=None, flags=0, ncomp=None, null=()):
    from kmer_spans_amd import _lib
    L = _lib.load()
    c = np.ascontiguousarray(c, dtype=np.uint32)
    n = c.shape[0] if n is None else n
    ncol = c.shape[1] if ncol is None else ncol
    r = np.ascontiguousarray(rows, dtype=np.int64) if rows is not None else None
    m = (n if r is None else r.size) if m is None else m
    ncomp = ncol if ncomp is None else ncomp
    size = max(1, abs(ncol)) * max(1, abs(ncol), abs(m))
    out = {k: np.full(size, -7.0) for k in ("center", "sdev", "rotation", "x", "gram")}
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in out.items()}
    rc = L.ks_spectra_pca(None, None if "spectra" in null else c.ctypes.data, n, ncol,
                          r.ctypes.data if r is not None else None, m, flags, ncomp, ptr["center"], ptr["sdev"],
                          ptr["rotation"], ptr["x"], ptr["gram"])
    return rc, L.ks_last_error().decode(), out


EMPTY = C8.copy()
EMPTY[5] = 0


@pytest.mark.parametrize("kw,msg", [
    (dict(c=C8, m=1), "at least 2 rows"),
    (dict(c=C8, m=0), "at least 2 rows"),
    (dict(c=C8, rows=[3]), "at least 2 rows"),
    (dict(c=C8, ncol=0), "ncol must be between 1 and 1024"),
    (dict(c=C8, ncol=1025), "ncol must be between 1 and 1024"),
    (dict(c=C8, ncomp=0), "ncomp must be between 1 and ncol = 4"),
    (dict(c=C8, ncomp=5), "ncomp must be between 1 and ncol = 4"),
    (dict(c=C8, flags=2), "unknown pca flags"),
    (dict(c=C8, m=9), "exceeds n = 8"),
    (dict(c=C8, rows=[0, 1, 8]), "row index 2 out of range"),
    (dict(c=C8, rows=[0, -1, 9]), "row index 1 out of range"),
    (dict(c=EMPTY), "row 5 has no counts"),
    (dict(c=EMPTY, rows=[7, 5, 0, 5]), "row 1 has no counts"),
    (dict(c=EMPTY, rows=[9, 5]), "row index 0 out of range"),  # the index comes first
    (dict(c=C8, null=("spectra",)), "null spectra"),
    (dict(c=C8, null=("center",)), "null output"),
    (dict(c=C8, null=("sdev",)), "null output"),
    (dict(c=C8, null=("rotation",)), "null output"),
])
def test_host_entry_rejects_before_any_device_call(kw, msg):
    """No GPU is present when this file runs alone: a device call would fail
    with a device error, not with these messages; the outputs stay untouched."""
    rc, err, out = _pca(**kw)
    assert rc == 1 and msg in err, err
    assert all((v == -7.0).all() for v in out.values())


def test_api_rejects_before_any_device_call():
    import kmer_spans_amd as K
    with pytest.raises(K.KmerSpansError, match="row 5 has no counts"):
        K.region_pca(EMPTY)
    with pytest.raises(K.KmerSpansError, match="row index 1 out of range"):
        K.region_pca(C8, rows=[0, 8])
    with pytest.raises(K.KmerSpansError, match="ncomp must be between"):
        K.region_pca(C8, ncomp=0)
    with pytest.raises(K.KmerSpansError, match="ncomp must be between"):
        K.region_pca(C8, ncomp=5)
    with pytest.raises(K.KmerSpansError, match="at least 2 rows"):
        K.region_pca(C8[:1])
    with pytest.raises(K.KmerSpansError, match="ncol must be between"):
        K.region_pca(np.ones((3, 1025), dtype=np.uint32))
    with pytest.raises(K.KmerSpansError, match="integer counts"):
        K.region_pca(np.ones((3, 4)))
    with pytest.raises(K.KmerSpansError, match="1-d array of integer"):
        K.region_pca(C8, rows=[[0, 1]])
