"""The argument scaffold of the device region_* wrappers (kmer_spans_amd/
device.py): every wrapper refuses a bad tensor with its text and before any
library call, a valid call on the same context afterwards returns the model's
answer, and region_pca takes the default context for ctx=None as its siblings
do.  5 x 4 counts and a 6-entry condensed vector; the models are the ones of
the analyses' own GPU tests.  Runs on an MI355X (pytest -m gpu)."""
import numpy as np
import pytest

from tests import test_gpu_hclust as TH
from tests import test_gpu_kmeans as TK
from tests import test_gpu_kmeans_seed as TS
from tests import test_gpu_knn as TN
from tests import test_gpu_nj as TJ
from tests import test_gpu_pca as TP
from tests import test_gpu_silhouette as TL
from tests import test_gpu_spectra as TR
from tests import test_gpu_spectra_dist as TD

pytestmark = pytest.mark.gpu

COUNTS = np.array([[9, 1, 0, 2], [1, 8, 3, 0], [0, 2, 7, 5], [4, 4, 4, 1], [2, 0, 1, 11]], dtype=np.uint32)
DIST = np.array([1.0, 2.5, 4.0, 3.0, 5.5, 0.75])  # n = 4: pairs 01 02 03 12 13 23
GROUP = np.array([1, 1, 2, 2], dtype=np.int32)
LABELS = np.array([1, 2, 2, 1, 2], dtype=np.int32)
SEQS = [b"ACGTTGCANNACGGTCATTAGGCA", b"TTTTACGCGCGAAT"]
IVS = [(0, 1, 24), (1, 2, 9), (0, 11, 13)]

E_COUNTS = "counts must be a contiguous int32 [n, ncol] cuda tensor"
E_ROWS = "rows must be a 1-d int64 array (numpy or cuda tensor)"
E_ROWS_B = "rows_b must be a 1-d int64 array (numpy or cuda tensor)"
E_DIST = "dist must be a contiguous 1-d float64 cuda tensor"


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


@pytest.fixture(scope="module")
def dev():
    """The inputs on the device: good ones and one bad one of every kind."""
    import torch
    good = TK.to_dev(COUNTS)
    dist = TH.dist_dev(DIST)
    return {
        "counts": good, "dist": dist,
        "float counts": good.to(torch.float32),
        "strided counts": TK.to_dev(np.ascontiguousarray(COUNTS.T)).t(),        # 5 x 4, column-major
        "int32 rows": torch.tensor([0, 2], dtype=torch.int32, device="cuda"),
        "2-d rows": np.zeros((2, 2), dtype=np.int64),
        "strided dist": TH.dist_dev(np.repeat(DIST, 2))[::2],                    # the same 6 values, stride 2
    }


def refused(monkeypatch, call, text):
    """call raises KmerSpansError(text) without asking for the library."""
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    with monkeypatch.context() as m:
        m.setattr(D, "load", no_library)
        with pytest.raises(_lib.KmerSpansError) as e:
            call()
    assert str(e.value) == text


def counts_and_rows_cases(dev, fn):
    """The refusals every wrapper with (ctx, counts, ..., rows=) shares: fn(counts, rows)."""
    return [(lambda: fn(dev["float counts"], None), E_COUNTS),
            (lambda: fn(dev["strided counts"], None), E_COUNTS),
            (lambda: fn(dev["counts"], dev["int32 rows"]), E_ROWS),
            (lambda: fn(dev["counts"], dev["2-d rows"]), E_ROWS)]


def test_the_bad_inputs_are_bad_in_one_way_only(dev):
    import torch
    assert dev["float counts"].shape == (5, 4) and dev["float counts"].is_contiguous()
    s = dev["strided counts"]
    assert s.shape == (5, 4) and s.dtype == torch.int32 and not s.is_contiguous()
    assert np.array_equal(s.cpu().numpy().view(np.uint32), COUNTS)
    d = dev["strided dist"]
    assert d.shape == (6,) and d.dtype == torch.float64 and not d.is_contiguous()
    assert np.array_equal(d.cpu().numpy(), DIST)


def test_region_spectra(ctx, dev, monkeypatch):
    import torch
    from kmer_spans_amd import device as D
    ds = D.from_host(SEQS, "cuda")
    pos = np.array(IVS, dtype=np.int32).T.copy()
    small = torch.empty(3 * 16 - 1, dtype=torch.int32, device="cuda")
    refused(monkeypatch, lambda: D.region_spectra(ctx, ds, pos, q=2, out=small),
            "out must be a contiguous int32 cuda tensor of R * 4^q elements")
    TR.check_device(ctx, SEQS, IVS, 2, True, ds=ds, what="after a refused out=")


def test_region_distances(ctx, dev, monkeypatch):
    import torch
    from kmer_spans_amd import device as D
    cases = counts_and_rows_cases(dev, lambda c, r: D.region_distances(ctx, c, rows=r))
    cases.append((lambda: D.region_distances(ctx, dev["counts"], rows_b=dev["int32 rows"]), E_ROWS_B))
    small = torch.empty(9, dtype=torch.float64, device="cuda")
    cases.append((lambda: D.region_distances(ctx, dev["counts"], out=small),
                  "out must be a contiguous float64 cuda tensor of 10 elements"))
    for call, text in cases:
        refused(monkeypatch, call, text)
        TD.check_device(ctx, COUNTS, dev_counts=dev["counts"], what="condensed")
        TD.check_device(ctx, COUNTS, rows=np.array([4, 0]), rows_b=np.array([1, 1, 3]), dev_counts=dev["counts"],
                        what="cross")


def test_region_pca(ctx, dev, monkeypatch):
    from kmer_spans_amd import device as D
    for call, text in counts_and_rows_cases(dev, lambda c, r: D.region_pca(ctx, c, rows=r)):
        refused(monkeypatch, call, text)
        got, _ = TP.run(ctx, COUNTS, dev_counts=dev["counts"])
        TP.check_exact_stages(got, COUNTS, None, True, "pca")
        TP.check_order_and_sign(got, "pca")


def test_region_pca_takes_the_default_context(ctx, dev):
    """ctx=None is the library's default context on device 0, as for every other wrapper."""
    from kmer_spans_amd import device as D
    want, _ = D.region_pca(ctx, dev["counts"], gram=True)
    got, _ = D.region_pca(None, dev["counts"], gram=True)
    assert sorted(got) == sorted(want)
    for key in want:
        assert np.array_equal(TP.bits(got[key].cpu().numpy()), TP.bits(want[key].cpu().numpy())), key


def test_region_kmeans_and_group_means(ctx, dev, monkeypatch):
    from kmer_spans_amd import device as D
    cases = counts_and_rows_cases(dev, lambda c, r: D.region_kmeans(ctx, c, [0, 3], rows=r))
    cases += counts_and_rows_cases(dev, lambda c, r: D.region_group_means(ctx, c, LABELS, rows=r))
    for call, text in cases:
        refused(monkeypatch, call, text)
        TK.check_kmeans(ctx, COUNTS, [0, 3], dev=dev["counts"], what="k-means")
        TK.check_means(ctx, COUNTS, LABELS, dev=dev["counts"], what="group means")


def test_region_kmeans_seed(ctx, dev, monkeypatch):
    from kmer_spans_amd import device as D
    for call, text in counts_and_rows_cases(dev, lambda c, r: D.region_kmeans_seed(ctx, c, 2, rows=r)):
        refused(monkeypatch, call, text)
        TS.check_seed(ctx, COUNTS, 3, "maximin", first=1, dev=dev["counts"], what="maximin")
        TS.check_seed(ctx, COUNTS, 3, "kmeans++", first=None, u=[0.3, 0.9, 0.5], dev=dev["counts"], what="dsq")


def test_region_knn(ctx, dev, monkeypatch):
    from kmer_spans_amd import device as D
    cases = counts_and_rows_cases(dev, lambda c, r: D.region_knn(ctx, c, 2, rows=r))
    cases.append((lambda: D.region_knn(ctx, dev["counts"], 2, rows_b=dev["2-d rows"]), E_ROWS_B))
    for call, text in cases:
        refused(monkeypatch, call, text)
        TN.check_knn(ctx, COUNTS, 3, dev=dev["counts"], what="self")
        TN.check_knn(ctx, COUNTS, 2, rows=np.array([4, 0]), rows_b=np.array([1, 3, 3]), dev=dev["counts"],
                     what="cross")


def test_trees_and_silhouette(ctx, dev, monkeypatch):
    from kmer_spans_amd import device as D
    bad = dev["strided dist"]
    for call in (lambda: D.region_hclust(ctx, bad), lambda: D.region_nj(ctx, bad),
                 lambda: D.region_silhouette(ctx, bad, GROUP)):
        refused(monkeypatch, call, E_DIST)
        for method in ("complete", "single", "average"):
            TH.check_device(ctx, dev["dist"], method, what=method)
        TJ.check_device(ctx, dev["dist"], "bindings n=4")
        TL.check_device(ctx, dev["dist"], GROUP, what="silhouette")
