"""The row checks of the profile panel agree across every entry point that
builds one: region_pca, region_kmeans, region_group_means, region_kmeans_seed
and region_knn (self and cross) refuse the same faulty selection with the same
message, a string built here from the position alone.  The host forms validate
before they touch a device, so this file runs without a GPU;
tests/test_gpu_panel_checks.py runs the same cases through the device forms.

n = 9 rows; ncol = 1 (one live lane of the wave that sums a row) and 65 (one
column past the 64-lane stride); selections of m = 5 (the last workgroup of the
normalise launch holds one wave of four) and m = 8 (full); k = 1, g = 2,
ncomp = 1.  The order pinned: every index of the first selection, then of the
second, before any row sum; in each, the lowest position."""
import numpy as np
import pytest

N = 9
SPARE = 8  # the row without counts; no clean selection names it
SHAPES = [(ncol, m) for ncol in (1, 65) for m in (5, 8)]


def counts_of(ncol: int) -> np.ndarray:
    c = np.random.default_rng(ncol).integers(1, 50, size=(N, ncol)).astype(np.uint32)
    c[SPARE] = 0
    return c


def clean(m: int) -> np.ndarray:
    """m rows with counts, out of order."""
    return (2 * np.arange(m, dtype=np.int64) + 1) % N


def message(kind: str, pos: int, second: bool = False) -> str:
    sel = " of the second selection" if second else ""
    return f"row index {pos}{sel} out of range" if kind == "index" else f"row {pos}{sel} has no counts"


def faulty(m: int):
    """(name, selection, kind, reported position) of every fault of one selection."""
    out = []

    def add(name, puts, kind, pos):
        rows = clean(m)
        for p, v in puts:
            rows[p] = v
        out.append((name, rows, kind, pos))

    for v in (-1, N):
        add(f"index {v} first", [(0, v)], "index", 0)
        add(f"index {v} last", [(m - 1, v)], "index", m - 1)
    add("two indices", [(m - 2, -1), (1, N)], "index", 1)
    add("empty first", [(0, SPARE)], "empty", 0)
    add("empty last", [(m - 1, SPARE)], "empty", m - 1)
    add("empty first, index last", [(0, SPARE), (m - 1, N)], "index", m - 1)
    return out


def single_cases(m: int):
    """(name, rows, message): for every entry point."""
    return [(name, rows, message(kind, pos)) for name, rows, kind, pos in faulty(m)]


def cross_cases(m: int):
    """(name, rows, rows_b, message): the cross form alone."""
    out = [("second: " + name, clean(m), rows, message(kind, pos, True)) for name, rows, kind, pos in faulty(m)]
    first_empty = clean(m)
    first_empty[0] = SPARE
    second_index = clean(m)
    second_index[m - 1] = N
    out.append(("empty in the first, index in the second", first_empty, second_index, message("index", m - 1, True)))
    return out


def group_of(m: int) -> np.ndarray:
    return (np.arange(m) % 2 + 1).astype(np.int32)


def host_entries():
    import kmer_spans_amd as K
    return {
        "pca": lambda c, rows: K.region_pca(c, rows=rows, ncomp=1),
        "kmeans": lambda c, rows: K.region_kmeans(c, [1, 2], rows=rows),
        "group_means": lambda c, rows: K.region_group_means(c, group_of(len(rows)), 2, rows=rows),
        "seed": lambda c, rows: K.region_kmeans_seed(c, 2, rows=rows),
        "knn self": lambda c, rows: K.region_knn(c, 1, rows=rows),
        "knn cross": lambda c, rows: K.region_knn(c, 1, rows=rows, rows_b=clean(len(rows))),
    }


def assert_refused(call, text, what):
    import kmer_spans_amd as K
    with pytest.raises(K.KmerSpansError) as e:
        call()
    assert str(e.value) == text, (what, str(e.value), text)


@pytest.mark.parametrize("ncol,m", SHAPES)
def test_every_entry_point_reports_the_same_row(ncol, m):
    c = counts_of(ncol)
    for name, rows, text in single_cases(m):
        for entry, call in host_entries().items():
            assert_refused(lambda: call(c, rows), text, (entry, name, ncol, m))


@pytest.mark.parametrize("ncol,m", SHAPES)
def test_cross_form_reports_the_second_selection(ncol, m):
    import kmer_spans_amd as K
    c = counts_of(ncol)
    for name, rows, rows_b, text in cross_cases(m):
        assert_refused(lambda: K.region_knn(c, 1, rows=rows, rows_b=rows_b), text, (name, ncol, m))
