"""Principal components of region spectra on the device (ks_spectra_pca_dev
and the host form) against the host model of tests/pcaref.py: the centre, the
cross-product G and the scores bit for bit; the eigen stage by its residual,
orthogonality and eigenvalue error against the same figures of the model's
Jacobi on the same G.  Runs on an MI355X (pytest -m gpu).

Bounds of the eigen stage.  The three figures (pcaref.eigen_errors, units of
2^-52) of the device must each be within 4x the model's figure for the same
G.  Three allowances for the measuring itself are added, each derived from
the arithmetic, u = 2^-53 being the unit roundoff and one unit being 2 u:

* The device's eigenvalues are not an output: they are read as
  sdev^2 (m - 1).  sdev = sqrt(lambda / (m - 1)) carries the division's
  rounding halved by the root and the root's own; squaring doubles both and
  adds one, the product with m - 1 adds another: (1 + 2 + 1 + 1) u = 2.5 units
  of lambda_j at most, so 2.5 units of lambda_max on the eigenvalue figure
  (SDEV_ROUND_TRIP).
* Trace: sum(sdev^2) (m - 1) against trace(G), both sums taken with math.fsum
  (correctly rounded: u of the sum each, 1 unit of trace(G) together).  The
  model's own trace figure, |sum(max(lambda, 0)) - trace(G)| / lambda_max with
  its eigenvalues taken directly, times 4, plus the round trip of every term,
  2.5 units of lambda_j each and so 2.5 trace(G) / lambda_max in all, plus that
  1: 4 x model + 3.5 trace(G) / lambda_max.
* ncol < 16: the model's figures can be exactly 0 (ncol = 1 always is), where
  a factor allows nothing.  What the float64 measurement itself can add is
  allowed on top: a dot product of ncol terms in V^T V and in G V errs by at
  most ncol u = ncol / 2 units, and the residual also takes the round trip of
  lambda: residual + (2.5 + ncol / 2), orthogonality + ncol / 2, at most 4.5
  units.  From ncol = 16 on neither is added.

The angle check uses 4x the largest of the model's three figures, divided by
the relative gap (the error of a vector is governed by the 2-norm of its
residual and by the loss of orthogonality, of which the latter is the
largest figure).  Where the model is too slow to run (ncol = 1024) the bound
is the first-order worst case instead: an entry of V or A takes part in one
rotation per round, a rotation rounds it 3 times by at most 2^-53 relative,
there are ncol - 1 rounds per sweep and the bound doubles as a margin for the
entries' growth: 4 * n_sweeps * ncol units of 2^-52, for the trace too."""
import math

import numpy as np
import pytest

from tests import pcaref as R
from tests.pcaref import bits

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SDEV_ROUND_TRIP = 2.5  # units of 2^-52 lambda_max (the module docstring)


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


def to_dev(counts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(counts, dtype=np.uint32).view(np.int32)).cuda()


def run(ctx, counts, rows=None, center=True, ncomp=None, scores=True, gram=True, dev_counts=None):
    from kmer_spans_amd import device as D
    dc = to_dev(counts) if dev_counts is None else dev_counts
    res, st = D.region_pca(ctx, dc, rows=rows, center=center, ncomp=ncomp, scores=scores, gram=gram)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()}, st


def assert_bits(got, want, what):
    same = bits(got) == bits(want)
    assert got.shape == want.shape and same.all(), (what, np.argwhere(~same)[:6].tolist(), got[~same][:4],
                                                    want[~same][:4])


def check_exact_stages(got, counts, rows, center, what):
    """center, G and x against the model's loops."""
    p = R.profiles(counts, rows)
    cen = R.ref_center(p, center)
    assert_bits(got["center"], cen, what + ": center")
    xc = R.ref_xc(p, cen, center)
    g = got["G"]
    assert np.array_equal(bits(g), bits(g.T)), what + ": G is not symmetric in bits"
    assert_bits(g, R.ref_gram(xc), what + ": G")
    if got["x"] is not None:
        assert_bits(got["x"], R.ref_scores(xc, got["rotation"]), what + ": x from the returned rotation")


def check_order_and_sign(got, what):
    sdev, rot = got["sdev"], got["rotation"]
    assert (np.diff(sdev) <= 0).all() and (sdev >= 0).all(), what + ": sdev not descending"
    top = np.argmax(np.abs(rot), axis=0)  # the first maximum
    assert (rot[top, np.arange(rot.shape[1])] > 0).all(), what + ": sign rule"


def check_eigen_stage(got, st, m, what, bound=None):
    """The eigen stage on the downloaded G; prints every figure before it asserts."""
    g, v, sdev = got["G"], got["rotation"], got["sdev"]
    ncol = g.shape[0]
    assert v.shape == (ncol, ncol)
    lam = sdev ** 2 * float(m - 1)
    w = np.linalg.eigvalsh(g)[::-1]
    lmax = float(np.abs(w).max())
    # the device's eigenvalues as it returns them: sdev^2 (m - 1).  sdev clips rounding-size
    # negative eigenvalues at 0: the eigenvalue figure compares against the clipped truth
    dev = list(R.eigen_errors(g, lam, v))
    dev[2] = float(np.abs(lam - np.maximum(w, 0.0)).max()) / lmax / R.EPS if lmax else 0.0
    tr = math.fsum(np.diag(g).tolist())
    trace = abs(math.fsum(lam.tolist()) - tr) / lmax / R.EPS if lmax else 0.0
    if bound is None:
        ml, mv, msw, mrot = R.ref_jacobi(g)
        ml, mv = R.order_and_sign(ml, mv)
        mod = list(R.eigen_errors(g, ml, mv))
        mod[2] = float(np.abs(np.maximum(ml, 0.0) - np.maximum(w, 0.0)).max()) / lmax / R.EPS if lmax else 0.0
        mtrace = abs(math.fsum(np.maximum(ml, 0.0).tolist()) - tr) / lmax / R.EPS if lmax else 0.0
        lim = [FACTOR * x for x in mod]
        lim[2] += SDEV_ROUND_TRIP
        if ncol < 16:  # the measurement's own rounding, where the model's figure can be 0 (the module docstring)
            lim[0] += SDEV_ROUND_TRIP + ncol / 2.0
            lim[1] += ncol / 2.0
        trace_lim = FACTOR * mtrace + (SDEV_ROUND_TRIP + 1.0) * (abs(tr) / lmax if lmax else 0.0)
        print(f"{what}: ncol {ncol} m {m} sweeps device {st['n_sweeps']} model {msw}, rotations device "
              f"{st['n_rotations']} model {mrot}; residual/orthogonality/eigenvalue in 2^-52: device "
              f"{dev[0]:.1f} {dev[1]:.1f} {dev[2]:.1f}, model {mod[0]:.1f} {mod[1]:.1f} {mod[2]:.1f}; trace device "
              f"{trace:.1f} model {mtrace:.1f} limit {trace_lim:.1f}")
    else:
        lim = [bound] * 3
        trace_lim = bound
        print(f"{what}: ncol {ncol} m {m} sweeps {st['n_sweeps']} rotations {st['n_rotations']}; residual/"
              f"orthogonality/eigenvalue in 2^-52: device {dev[0]:.1f} {dev[1]:.1f} {dev[2]:.1f}, bound {bound:.0f}; "
              f"trace {trace:.1f}")
    assert 1 <= st["n_sweeps"] < R.KS_PCA_MAX_SWEEPS, (what, st)
    for name, d, b in zip(("residual", "orthogonality", "eigenvalue"), dev, lim):
        assert d <= b, (what, name, d, b)
    assert trace <= trace_lim, (what, "trace", trace, trace_lim)
    check_order_and_sign(got, what)
    # separated components against numpy's vectors
    if lmax:
        ww, vv = np.linalg.eigh(g)
        ww, vv = ww[::-1], vv[:, ::-1]
        up = np.concatenate([[np.inf], ww[:-1] - ww[1:]])
        down = np.concatenate([ww[:-1] - ww[1:], [np.inf]])
        gap = np.minimum(up, down) / lmax
        worst = 0.0
        for j in np.flatnonzero(gap > 1e-6):
            cosv = abs(float(v[:, j] @ vv[:, j])) / float(np.linalg.norm(v[:, j]))
            sine = float(np.sqrt(max(0.0, 1.0 - min(cosv, 1.0) ** 2)))
            # 1 - cos^2 cannot resolve a sine below sqrt(2^-52): measure the small ones directly
            d = v[:, j] / np.linalg.norm(v[:, j])
            d = d - vv[:, j] * np.sign(float(d @ vv[:, j]))
            sine = min(sine, float(np.linalg.norm(d)))
            worst = max(worst, sine * gap[j] / R.EPS) if np.isfinite(gap[j]) else worst
            assert sine <= max(lim) * R.EPS / gap[j], (what, "angle of component", int(j), sine, gap[j])
        print(f"{what}: {int((gap > 1e-6).sum())} separated components, worst sine * gap {worst:.1f} (2^-52)")


# --------------------------------------------------------------- known answers

def test_two_by_two(ctx):
    import kmer_spans_amd as K
    c = np.array([[1, 0], [0, 1]], dtype=np.uint32)
    got, st = run(ctx, c)
    assert got["center"].tolist() == [0.5, 0.5]
    assert got["G"].tolist() == [[0.5, -0.5], [-0.5, 0.5]]
    assert got["sdev"][1] == 0.0 and abs(got["sdev"][0] - 1.0) <= 2 * R.EPS
    want = np.array([1.0, -1.0]) / np.sqrt(2.0)
    assert np.abs(got["rotation"][:, 0] - want).max() <= 2 * R.EPS
    assert np.abs(got["x"][:, 0] - np.array([1.0, -1.0]) / np.sqrt(2.0)).max() <= 2 * R.EPS
    assert (st["n_sweeps"], st["n_rotations"]) == (2, 1)
    host = K.region_pca(c)  # api -> host entry
    for k in ("center", "sdev", "rotation", "x"):
        assert_bits(host[k], got[k], "2 x 2, host entry: " + k)


def test_identical_rows(ctx):
    # m and the row sum are powers of two: every partial sum of the mean's chain, 3 p included, is exact
    c = np.tile(np.array([[3, 1, 0, 2, 2]], dtype=np.uint32), (4, 1))
    got, st = run(ctx, c)
    assert not got["G"].any() and not got["sdev"].any() and not got["x"].any()
    assert np.array_equal(got["rotation"], np.eye(5))
    assert (st["n_sweeps"], st["n_rotations"]) == (1, 0)
    assert_bits(got["center"], R.profiles(c)[0], "identical rows: center")


# ---------------------------------- every stage at tile, chunk and block seams

CASES = [(2, 4, True), (2, 17, False), (3, 1, True), (3, 16, False), (63, 16, True), (63, 64, False),
         (64, 17, True), (64, 4, False), (65, 64, True), (65, 1, False), (257, 256, True), (257, 17, False),
         (1025, 16, True), (1025, 256, False), (1025, 4, False), (130, 64, True)]


@pytest.mark.parametrize("m,ncol,center", CASES)
def test_stages(ctx, m, ncol, center):
    rng = np.random.default_rng(1000 * m + ncol)
    c = R.synth_counts(rng, m, ncol)
    what = f"m {m} ncol {ncol} center {center}"
    got, st = run(ctx, c, center=center)
    check_exact_stages(got, c, None, center, what)
    if not center:
        assert not got["center"].any()
    check_eigen_stage(got, st, m, what)
    assert st["panel_bytes"] >= 8 * m * ncol and st["ms_total"] > 0


def test_fewer_components_are_the_full_call_s_bits(ctx):
    rng = np.random.default_rng(77)
    c = R.synth_counts(rng, 70, 80)
    dc = to_dev(c)
    full, _ = run(ctx, c, dev_counts=dc)
    for k in (1, 3, 64, 65):
        part, _ = run(ctx, c, ncomp=k, dev_counts=dc)
        assert part["rotation"].shape == (80, k) and part["x"].shape == (70, k)
        assert_bits(part["rotation"], np.ascontiguousarray(full["rotation"][:, :k]), f"ncomp {k}: rotation")
        assert_bits(part["x"], np.ascontiguousarray(full["x"][:, :k]), f"ncomp {k}: x")
        for key in ("center", "sdev", "G"):
            assert_bits(part[key], full[key], f"ncomp {k}: {key}")
    none, _ = run(ctx, c, ncomp=2, scores=False, gram=False, dev_counts=dc)
    assert none["x"] is None and "G" not in none
    assert_bits(none["rotation"], np.ascontiguousarray(full["rotation"][:, :2]), "no scores: rotation")


# ------------------------------------------------------------------ termination

def fold_both_strands(c, q):
    """row[w] = n[w] + n[rc(w)] as ks_region_spectra does: exact duplicate columns."""
    idx = np.arange(4 ** q)
    rc = np.zeros_like(idx)
    for i in range(q):
        rc = rc * 4 + (((idx >> (2 * i)) & 3) ^ 2)
    return (c + c[:, rc]).astype(np.uint32)


@pytest.mark.parametrize("case", ["both_strands_q2", "both_strands_q3", "zero_columns", "rank2"])
def test_termination(ctx, case):
    rng = np.random.default_rng(len(case))
    if case.startswith("both_strands"):
        q = int(case[-1])
        c, m = fold_both_strands(R.synth_counts(rng, 90, 4 ** q), q), 90
    elif case == "zero_columns":
        c, m = R.synth_counts(rng, 50, 32), 50
        c[:, [1, 2, 7, 30, 31]] = 0
    else:
        c, m = R.synth_counts(rng, 3, 16), 3
    got, st = run(ctx, c)
    check_exact_stages(got, c, None, True, case)
    check_eigen_stage(got, st, m, case)
    assert st["n_sweeps"] < 32, st
    if case == "rank2":
        assert (got["sdev"][2:] <= 1e-7 * got["sdev"][0]).all()


# ------------------------------------------------------------------- selections

@pytest.mark.parametrize("center", [True, False])
def test_selections(ctx, center):
    rng = np.random.default_rng(31)
    c = R.synth_counts(rng, 120, 16)
    dc = to_dev(c)
    sels = {"reversed": np.arange(119, -1, -1), "repeated": np.array([5, 5, 9, 5, 100, 9, 0]),
            "subset": np.sort(rng.choice(120, 67, replace=False)), "shuffled": rng.permutation(120)[:66]}
    for name, rows in sels.items():
        got, st = run(ctx, c, rows=rows.astype(np.int64), center=center, dev_counts=dc)
        check_exact_stages(got, c, rows, center, name)
        check_eigen_stage(got, st, rows.size, name)
    import torch
    got, _ = run(ctx, c, rows=torch.from_numpy(sels["subset"].astype(np.int64)).cuda(), center=center, dev_counts=dc)
    check_exact_stages(got, c, sels["subset"], center, "cuda selection")
    # selection order is part of the contract: the reversed centre is another chain of additions
    fwd, _ = run(ctx, c, center=center, dev_counts=dc)
    rev, _ = run(ctx, c, rows=sels["reversed"].astype(np.int64), center=center, dev_counts=dc)
    assert_bits(rev["G"], R.ref_gram(R.ref_xc(R.profiles(c)[::-1], rev["center"], center)), "reversed G")
    assert np.allclose(fwd["G"], rev["G"], rtol=0, atol=1e-12)


# ----------------------------------------------------------------------- errors

def test_errors_leave_outputs_and_context_alone(ctx):
    import ctypes as C
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(3)
    c = R.synth_counts(rng, 40, 16)
    c[[17, 30]] = 0
    dc = to_dev(c)
    L = _lib.load()

    def raw(rows, m):
        outs = [torch.full((n,), -7.0, dtype=torch.float64, device="cuda") for n in (16, 16, 256, 40 * 16, 256)]
        r = torch.from_numpy(np.asarray(rows, dtype=np.int64)).cuda() if rows is not None else None
        st = _lib.PcaStats()
        rc = L.ks_spectra_pca_dev(ctx.handle, C.c_void_p(dc.data_ptr()), 40, 16,
                                  C.c_void_p(r.data_ptr()) if r is not None else None, m, 0, 16,
                                  *[C.c_void_p(o.data_ptr()) for o in outs], C.byref(st))
        torch.cuda.synchronize()
        return rc, L.ks_last_error().decode(), [o.cpu().numpy() for o in outs]

    for rows, m, msg in [(None, 40, "row 17 has no counts"), ([3, 30, 4, 17], 4, "row 1 has no counts"),
                         ([3, 40, 17], 3, "row index 1 out of range"), ([-1, 2], 2, "row index 0 out of range")]:
        rc, err, outs = raw(rows, m)
        assert rc == 1 and msg in err, err
        assert all((o == -7.0).all() for o in outs), msg
    with pytest.raises(K.KmerSpansError, match="row 17 has no counts"):
        D.region_pca(ctx, dc)
    # a good call on the same context right after
    rows = np.array([r for r in range(40) if r not in (17, 30)], dtype=np.int64)
    got, st = run(ctx, c, rows=rows, dev_counts=dc)
    check_exact_stages(got, c, rows, True, "after the rejected calls")
    check_eigen_stage(got, st, rows.size, "after the rejected calls")
    with pytest.raises(K.KmerSpansError, match="contiguous int32"):
        D.region_pca(ctx, dc.double())
    with pytest.raises(K.KmerSpansError, match="at least 2 rows"):
        D.region_pca(ctx, dc, rows=np.array([1], dtype=np.int64))
    with pytest.raises(K.KmerSpansError, match="ncomp must be between"):
        D.region_pca(ctx, dc, rows=rows, ncomp=17)


# ---------------------------------------------------- repeatability, host entry

def test_repeatable_and_host_entry(ctx):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(8)
    c = R.synth_counts(rng, 300, 64)
    dc = to_dev(c)
    rows = rng.permutation(300)[:211].astype(np.int64)
    first, st1 = run(ctx, c, rows=rows, dev_counts=dc)
    second, st2 = run(ctx, c, rows=rows, dev_counts=dc)
    D.region_distances(ctx, dc, rows=rows[:50])  # an unrelated call on the same context
    third, st3 = run(ctx, c, rows=rows, dev_counts=dc)
    for other, st in ((second, st2), (third, st3)):
        for k in first:
            assert_bits(other[k], first[k], "repeat: " + k)
        assert (st["n_sweeps"], st["n_rotations"]) == (st1["n_sweeps"], st1["n_rotations"])
    for center in (True, False):
        dev, _ = run(ctx, c, rows=rows, center=center, ncomp=5, dev_counts=dc)
        host = K.region_pca(c, rows=rows, center=center, ncomp=5)
        for k in ("center", "sdev", "rotation", "x"):
            assert_bits(host[k], dev[k], f"host entry, center {center}: {k}")
    assert K.region_pca(c, ncomp=1, scores=False)["x"] is None


# --------------------------------------------------------------------- pipeline

def test_pipeline_scan_spectra_pca(ctx):
    """A planted-repeat scan, device.region_spectra and device.region_pca with
    nothing downloaded in between; region_distances runs from the same tensor."""
    import torch
    from kmer_spans_amd import device as D
    k = 7
    rng = np.random.default_rng(17)
    s = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=120_000)
    plants = {"a150": (20_000, b"A" * 150), "a420": (50_000, b"A" * 420), "ca": (80_000, b"CA" * 120),
              "ca2": (100_000, b"CA" * 60)}
    for name, (at, unit) in plants.items():
        flank = ord("N") if name.startswith("a") else ord("G")
        s[at - 30:at] = flank
        s[at:at + len(unit)] = np.frombuffer(unit, dtype=np.uint8)
        s[at + len(unit):at + len(unit) + 30] = flank
    ds = D.from_host([s.tobytes()], "cuda")
    counts = torch.zeros(4 ** k, dtype=torch.int32, device="cuda")
    words = D.count(ctx, ds, k, counts)
    tab = D.DeviceTable.from_counts(ctx, counts, k, "rank", total=words, thr=0.75, expand=True)
    pos, _, _ = D.scan(ctx, ds, k, tab, 20, 5.0)
    n = pos.shape[1]
    assert n >= 4
    sp, _, _ = D.region_spectra(ctx, ds, pos, q=2, both_strands=True, entropy=False)
    res, st = D.region_pca(ctx, sp, gram=True)
    dist, _ = D.region_distances(ctx, sp)
    assert dist.numel() == n * (n - 1) // 2
    got = {key: v.cpu().numpy() for key, v in res.items()}
    c = sp.cpu().numpy().view(np.uint32)
    check_exact_stages(got, c, None, True, "pipeline")
    check_eigen_stage(got, st, n, "pipeline")
    print(f"{n} regions, sdev {got['sdev'][:3]}")


# ----------------------------------------------------------------- larger sizes

def test_large_m(ctx):
    """m = 8192 at ncol = 256: many Gram chunks and projection tiles."""
    rng = np.random.default_rng(8192)
    m, ncol = 8192, 256
    c = R.synth_counts(rng, m, ncol)
    got, st = run(ctx, c)
    check_exact_stages(got, c, None, True, "m 8192")
    check_eigen_stage(got, st, m, "m 8192")
    print("m 8192 ncol 256:", st)


def test_max_ncol(ctx):
    """ncol = 1024, the documented cap, at m = 33 (rank 32); the model's Jacobi
    is too slow here: the first-order bound of the module docstring."""
    rng = np.random.default_rng(1024)
    m, ncol = 33, 1024
    c = R.synth_counts(rng, m, ncol)
    got, st = run(ctx, c)
    check_exact_stages(got, c, None, True, "ncol 1024")
    check_eigen_stage(got, st, m, "ncol 1024", bound=4.0 * st["n_sweeps"] * ncol)
    print("m 33 ncol 1024:", st)
