"""The cases of tests/test_panel_checks.py through the device forms: the words
the normalise kernel leaves are reported as the host checks report the same
selection, by every entry point.  Then one valid call per entry point at
m = 5, ncol = 65 with a selection that names a row twice, against the host
models bit for bit."""
import numpy as np
import pytest

from tests.test_gpu_kmeans import check_kmeans, check_means
from tests.test_gpu_kmeans_seed import check_seed
from tests.test_gpu_knn import check_knn
from tests.test_gpu_pca import check_exact_stages, check_order_and_sign, run, to_dev
from tests.test_panel_checks import (SHAPES, assert_refused, clean, counts_of, cross_cases, group_of,
                                     single_cases)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    c = _lib.context(0)
    D.bind_torch_stream(c)
    return c


def device_entries(ctx):
    from kmer_spans_amd import device as D
    return {
        "pca": lambda dc, rows: D.region_pca(ctx, dc, rows=rows, ncomp=1),
        "kmeans": lambda dc, rows: D.region_kmeans(ctx, dc, [1, 2], rows=rows),
        "group_means": lambda dc, rows: D.region_group_means(ctx, dc, group_of(len(rows)), 2, rows=rows),
        "seed": lambda dc, rows: D.region_kmeans_seed(ctx, dc, 2, rows=rows),
        "knn self": lambda dc, rows: D.region_knn(ctx, dc, 1, rows=rows),
        "knn cross": lambda dc, rows: D.region_knn(ctx, dc, 1, rows=rows, rows_b=clean(len(rows))),
    }


@pytest.mark.parametrize("ncol,m", SHAPES)
def test_every_entry_point_reports_the_same_row(ctx, ncol, m):
    dc = to_dev(counts_of(ncol))
    for name, rows, text in single_cases(m):
        for entry, call in device_entries(ctx).items():
            assert_refused(lambda: call(dc, rows), text, (entry, name, ncol, m))


@pytest.mark.parametrize("ncol,m", SHAPES)
def test_cross_form_reports_the_second_selection(ctx, ncol, m):
    from kmer_spans_amd import device as D
    dc = to_dev(counts_of(ncol))
    for name, rows, rows_b, text in cross_cases(m):
        assert_refused(lambda: D.region_knn(ctx, dc, 1, rows=rows, rows_b=rows_b), text, (name, ncol, m))


def test_valid_calls_match_the_models(ctx):
    counts = counts_of(65)
    rows = np.array([1, 3, 5, 3, 0], dtype=np.int64)  # row 3 twice
    dc = to_dev(counts)
    for center in (True, False):
        got, _ = run(ctx, counts, rows=rows, center=center, ncomp=1, dev_counts=dc)
        check_exact_stages(got, counts, rows, center, f"pca, center {center}")
        check_order_and_sign(got, f"pca, center {center}")
    check_kmeans(ctx, counts, np.array([1, 2]), rows=rows, what="kmeans", dev=dc)
    check_means(ctx, counts, group_of(5), 2, rows=rows, what="group means", dev=dc)
    check_seed(ctx, counts, 2, "maximin", rows=rows, what="seed maximin", dev=dc)
    check_seed(ctx, counts, 2, "kmeans++", rows=rows, u=np.array([0.25, 0.75]), what="seed kmeans++", dev=dc)
    check_knn(ctx, counts, 1, rows=rows, what="knn self", dev=dc)
    check_knn(ctx, counts, 1, rows=rows, rows_b=clean(5), what="knn cross", dev=dc)
