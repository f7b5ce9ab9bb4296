"""Host model of ks_spectra_pca (include/kmer_spans.h): the profile, the
centre, the cross-product and the scores as plain loops in the contract's
order of operations (numpy rounds every product and every sum separately: no
FMA), the cyclic Jacobi with the contract's schedule, rotation formulas and
skip rule, vectorised per round, and the order and sign rule.  The centre, G
and the scores are what the device must reproduce bit for bit; the Jacobi is
the yardstick of the eigen stage's error (numpy's sqrt and division are
correctly rounded, the device's may differ in the last bit)."""
import numpy as np

KS_PCA_MAX_NCOL = 1024
KS_PCA_MAX_SWEEPS = 64
EPS = 2.0 ** -52


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def profiles(counts, rows=None) -> np.ndarray:
    """p[r][c] = (double)cnt / (double)T of the selected rows, in selection order."""
    c = np.asarray(counts).astype(np.uint64)
    if rows is not None:
        c = c[np.asarray(rows, dtype=np.int64)]
    t = c.sum(axis=1, dtype=np.uint64)
    assert int(t.min()) > 0 and int(t.max()) < 2 ** 44
    return c.astype(np.float64) / t.astype(np.float64)[:, None]


def ref_center(p: np.ndarray, center: bool = True) -> np.ndarray:
    """One accumulator per column over the rows in order, then one division."""
    m, ncol = p.shape
    if not center:
        return np.zeros(ncol)
    acc = np.zeros(ncol)
    for r in range(m):
        acc = acc + p[r]
    return acc / float(m)


def ref_xc(p: np.ndarray, cen: np.ndarray, center: bool = True) -> np.ndarray:
    return p - cen[None, :] if center else p.copy()


def ref_gram(xc: np.ndarray) -> np.ndarray:
    g = np.zeros((xc.shape[1], xc.shape[1]))
    for r in range(xc.shape[0]):
        g = g + np.outer(xc[r], xc[r])
    return g


def ref_scores(xc: np.ndarray, rotation: np.ndarray) -> np.ndarray:
    x = np.zeros((xc.shape[0], rotation.shape[1]))
    for c in range(xc.shape[1]):
        x = x + np.outer(xc[:, c], rotation[c])
    return x


def round_pairs(ncol: int, rnd: int):
    """The pairs of round rnd (0 .. P - 2) of the round-robin order, P = ncol
    rounded up to even: slot 0 is (P - 1, rnd), slot i = 1 .. P/2 - 1 is
    ((rnd + i) mod (P - 1), (rnd - i) mod (P - 1)); each as (low, high); the
    pair holding the dummy index (>= ncol) is left out."""
    big = ncol + (ncol & 1)
    n1 = big - 1
    i = np.arange(big // 2)
    a = np.where(i == 0, big - 1, (rnd + i) % n1)
    b = (rnd - i) % n1
    p, q = np.minimum(a, b), np.maximum(a, b)
    keep = q < ncol
    return p[keep].astype(np.int64), q[keep].astype(np.int64)


def ref_jacobi(g: np.ndarray):
    """Cyclic two-sided Jacobi of the symmetric g.  Returns (lam, v, n_sweeps,
    n_rotations): g ~ v diag(lam) v^T, columns in Jacobi order (unsorted)."""
    ncol = g.shape[0]
    a = np.array(g, dtype=np.float64)
    v = np.eye(ncol)
    floor = EPS * float(np.abs(np.diag(a)).max())
    eps2 = EPS * EPS
    big = ncol + (ncol & 1)
    n_rot = 0
    for sweep in range(KS_PCA_MAX_SWEEPS):
        rot_sweep = 0
        for rnd in range(big - 1):
            p, q = round_pairs(ncol, rnd)
            if p.size == 0:
                continue
            app, aqq, apq = a[p, p], a[q, q], a[p, q]
            rot = (np.abs(apq) > floor) & ~(apq * apq <= eps2 * np.abs(app * aqq))
            k = int(rot.sum())
            if k == 0:
                continue
            rot_sweep += k
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                t = np.where(theta < 0.0, -t, t)
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
            t = np.where(rot, t, 0.0)
            c = np.where(rot, c, 1.0)
            s = np.where(rot, s, 0.0)
            # columns, then rows: every entry (i, j) with i in pair k1 and j in pair k2
            # sees the column step of k2 first and the row step of k1 second
            ap, aq = a[:, p].copy(), a[:, q].copy()
            a[:, p] = c * ap - s * aq
            a[:, q] = s * ap + c * aq
            rp, rq = a[p, :].copy(), a[q, :].copy()
            a[p, :] = c[:, None] * rp - s[:, None] * rq
            a[q, :] = s[:, None] * rp + c[:, None] * rq
            # the pair's own 2 x 2 block in closed form
            a[p, p] = np.where(rot, app - t * apq, app)
            a[q, q] = np.where(rot, aqq + t * apq, aqq)
            a[p, q] = np.where(rot, 0.0, apq)
            a[q, p] = a[p, q]
            # the device computes the blocks with k1 < k2 (slot order) and mirrors them;
            # here the upper triangle stands in for that: same magnitude of rounding
            a = np.triu(a) + np.triu(a, 1).T
            vp, vq = v[:, p].copy(), v[:, q].copy()
            v[:, p] = c * vp - s * vq
            v[:, q] = s * vp + c * vq
        n_rot += rot_sweep
        if rot_sweep == 0:
            return np.diag(a).copy(), v, sweep + 1, n_rot
    raise RuntimeError("no convergence in %d sweeps" % KS_PCA_MAX_SWEEPS)


def order_and_sign(lam: np.ndarray, v: np.ndarray):
    """Descending by eigenvalue, equal values in Jacobi column order; each
    vector's entry of largest magnitude (the lowest index among equals) positive."""
    perm = np.argsort(-lam, kind="stable")
    lam, v = lam[perm], v[:, perm].copy()
    for j in range(v.shape[1]):
        i = int(np.argmax(np.abs(v[:, j])))  # first maximum
        if v[i, j] < 0:
            v[:, j] = -v[:, j]
    return lam, v


def ref_pca(counts, rows=None, center=True, ncomp=None):
    """The whole contract on the host."""
    p = profiles(counts, rows)
    m, ncol = p.shape
    ncomp = ncol if ncomp is None else ncomp
    cen = ref_center(p, center)
    xc = ref_xc(p, cen, center)
    g = ref_gram(xc)
    lam, v, n_sweeps, n_rot = ref_jacobi(g)
    lam, v = order_and_sign(lam, v)
    sdev = np.sqrt(np.maximum(lam, 0.0) / float(m - 1))
    rot = np.ascontiguousarray(v[:, :ncomp])
    return {"center": cen, "G": g, "lambda": lam, "sdev": sdev, "rotation": rot, "x": ref_scores(xc, rot),
            "n_sweeps": n_sweeps, "n_rotations": n_rot}


def eigen_errors(g, lam, v):
    """(residual, orthogonality, eigenvalue error) in units of 2^-52:
    max|G V - V diag(lam)| / ||G||_2, max|V^T V - I|, max|lam - eigvalsh(G)| / lam_max
    (lam descending).  An all-zero G gives zeros."""
    w = np.linalg.eigvalsh(g)[::-1]
    norm = float(np.abs(w).max())
    if norm == 0.0:
        return 0.0, float(np.abs(v.T @ v - np.eye(v.shape[1])).max()) / EPS, 0.0
    res = float(np.abs(g @ v - v * lam[None, :]).max()) / norm
    orth = float(np.abs(v.T @ v - np.eye(v.shape[1])).max())
    ev = float(np.abs(lam - w).max()) / norm
    return res / EPS, orth / EPS, ev / EPS


def synth_counts(rng, m: int, ncol: int, hi: int = 1000) -> np.ndarray:
    c = rng.integers(0, hi, size=(m, ncol)).astype(np.uint32)
    c[rng.random((m, ncol)) < 0.3] = 0
    c[:, 0] |= 1  # no empty row
    return c
