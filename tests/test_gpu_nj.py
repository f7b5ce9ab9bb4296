"""Neighbour joining on the device (ks_nj_dev / ks_nj) against the host
reference of tests/test_nj.py: join, root and the bits of length and
root_length identical, with and without compaction; beyond the numpy
reference's reach, additive trees that must come back exactly, and at
n = 4,100 the torch transcription of tests/njref.py on the device.  Runs on an
MI355X (pytest -m gpu)."""
import numpy as np
import pytest

from tests.test_nj import (ALL_EQUAL6, FIVE, FIVE_TREE, assert_additive_exact, assert_same_nj, assert_tree_is, bits,
                           predicted_compactions, random_additive, ref_nj, sample_pairs, signed_zero_case)
from tests.test_spectra_dist import random_counts

pytestmark = pytest.mark.gpu


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


def dist_dev(d):
    import torch
    return torch.from_numpy(np.ascontiguousarray(d, dtype=np.float64)).cuda()


_refs = {}


def ref_cached(key, host, n):
    """ref_nj once per input (key names it); never modified afterwards."""
    if key not in _refs:
        _refs[key] = ref_nj(host, n)
    return _refs[key]


def check_device(ctx, dist, key, want=None):
    """device.region_nj on a CUDA tensor, compacting and not, against the
    reference on its download."""
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    host = dist.cpu().numpy()
    n = _lib.nj_n(host.size)
    want = ref_cached(key, host, n) if want is None else want
    tree, st = D.region_nj(ctx, dist)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(host)), (key, "keep_input=True changed the input")
    assert_same_nj(tree, want, key)
    # compaction was measured in: the count is the threshold's
    assert st["n"] == n and st["n_compactions"] == predicted_compactions(n), (key, st)
    flat, st_flat = D.region_nj(ctx, dist, compact=False)
    assert_same_nj(flat, want, f"{key} without compaction")
    assert st_flat["n_compactions"] == 0 and st_flat["work_bytes"] == 8 * host.size
    return tree, st, want


# ------------------------------------------------------------- known answers

def test_known_answers(ctx):
    import kmer_spans_amd as K
    tree, _, _ = check_device(ctx, dist_dev(FIVE), "five taxa")
    assert_tree_is(tree, FIVE_TREE)
    assert_tree_is(K.region_nj(np.array(FIVE, dtype=np.float64)), FIVE_TREE)  # api -> host entry
    tree, st, _ = check_device(ctx, dist_dev([3, 4, 5]), "three taxa")
    assert tree["join"].shape == (0, 2) and tree["root"].tolist() == [-1, -2, -3]
    assert tree["root_length"].tolist() == [1.0, 2.0, 3.0]
    tree, _, _ = check_device(ctx, dist_dev(np.full(15, 0.75)), "all equal 6")
    assert_tree_is(tree, ALL_EQUAL6)
    tree, _, _ = check_device(ctx, dist_dev(signed_zero_case()), "signed zeros 6")
    assert tree["join"].tolist() == ALL_EQUAL6["join"]


# ------------------------------------------------- sizes across the reduction edges

@pytest.fixture(scope="module")
def tie_free():
    """device.region_distances of random_counts at ncol = 16, per n, made once."""
    made = {}

    def get(ctx, n):
        from kmer_spans_amd import device as D
        if n not in made:
            d, _ = D.region_distances(ctx, to_dev(random_counts(np.random.default_rng(n), n, 16)))
            made[n] = d
        return made[n]
    return get


@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513])
def test_sizes(ctx, tie_free, n):
    """One wave, one block stride, and one entry either side of each; from 16
    rows on the matrix is compacted, at 513 six times."""
    _, st, _ = check_device(ctx, tie_free(ctx, n), f"tie free {n}")
    if n == 513:
        assert st["n_compactions"] == 6
    if n >= 16:
        half = n // 2
        assert st["work_bytes"] == 8 * (n * (n - 1) // 2) + 8 * (half * (half - 1) // 2)


# ------------------------------------------------------------------- ties

@pytest.mark.parametrize("n", [130, 400])
def test_tie_heavy(ctx, n):
    """Distances drawn from {1, 2, 3}: many equal q at every step."""
    rng = np.random.default_rng(n)
    d = rng.integers(1, 4, size=n * (n - 1) // 2).astype(np.float64)
    check_device(ctx, dist_dev(d), f"ties {n}")


def test_all_equal(ctx):
    n = 300
    tree, _, _ = check_device(ctx, dist_dev(np.full(n * (n - 1) // 2, 0.75)), "all equal 300")
    assert tree["join"].tolist() == [[-1, -2]] + [[s, -(s + 2)] for s in range(1, n - 3)]
    assert tree["root"].tolist() == [n - 3, -(n - 1), -n]


def test_signed_zeros(ctx):
    """-0.0 and +0.0 compare equal: the pair decides, on the device as on the host."""
    n = 150
    rng = np.random.default_rng(150)
    d = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, 2.0]), size=n * (n - 1) // 2)
    assert np.signbit(d).any() and (~np.signbit(d) & (d == 0)).any()
    check_device(ctx, dist_dev(d), "signed zeros 150")


def test_proportional_families(ctx):
    """Rows x2, x3, x1000 of one row are at distance exactly 0 of it and at
    equal distances of every other row: ties in q that the lowest pair wins."""
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(6)
    c = random_counts(rng, 70, 256, hi=4000)
    for fam in ((10, 11, 40, 69), (3, 50, 51)):
        base = c[fam[0]].astype(np.uint64)
        for row, f in zip(fam[1:], (2, 3, 1000)):
            c[row] = (base * f).astype(np.uint32)
    d, _ = D.region_distances(ctx, to_dev(c))
    host = d.cpu().numpy()
    assert (host == 0).sum() == 6 + 3
    check_device(ctx, d, "proportional")


def test_pipeline_scan_spectra_distances_nj(ctx):
    """A planted-repeat scan, device.region_spectra, device.region_distances
    and device.region_nj with nothing downloaded in between (the two poly-A
    regions have proportional counts: a distance of exactly 0 among the input)."""
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
    R = pos.shape[1]
    assert R >= 4
    sp, _, _ = D.region_spectra(ctx, ds, pos, q=4, both_strands=True, entropy=False)
    dist, _ = D.region_distances(ctx, sp)
    tree, st = D.region_nj(ctx, dist, keep_input=False)  # the distances are consumed
    del dist
    again, _ = D.region_distances(ctx, sp)
    host = again.cpu().numpy()
    assert_same_nj(tree, ref_nj(host, R), "pipeline")
    assert st["n"] == R and st["work_bytes"] == (8 * ((R // 2) * (R // 2 - 1) // 2) if R >= 16 else 0)
    print(f"{R} regions, {int((host == 0).sum())} pairs at distance 0")


# ---------------------------------------------------------------- keep_input

def test_keep_input(ctx, tie_free):
    from kmer_spans_amd import device as D
    n = 257
    d = tie_free(ctx, n).clone()
    before = d.cpu().numpy().copy()
    kept, st_kept = D.region_nj(ctx, d, keep_input=True)
    assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    used, st_used = D.region_nj(ctx, d, keep_input=False)  # allowed to overwrite d
    assert_same_nj(used, kept, "keep_input=False")
    assert st_kept["work_bytes"] - st_used["work_bytes"] == 8 * before.size


# --------------------------------------------------------- non-finite entries

def test_nan_from_an_empty_row(ctx):
    """An empty spectrum row is NaN against every row: hclust's error, the
    input left alone, and the context works on."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(11)
    c = random_counts(rng, 90, 16)
    c[37] = 0
    d, _ = D.region_distances(ctx, to_dev(c))
    before = d.cpu().numpy().copy()
    assert int(np.flatnonzero(np.isnan(before))[0]) == 36  # pair (0, 37)
    for keep in (True, False):
        with pytest.raises(K.KmerSpansError, match="^dissimilarity at offset 36 is not finite$"):
            D.region_nj(ctx, d, keep_input=keep)
        assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    c[37] = c[36]
    good, _ = D.region_distances(ctx, to_dev(c))
    check_device(ctx, good, "after a rejected call")


@pytest.mark.parametrize("at", [0, 1, 4094, 4095, 8001, 8384])
@pytest.mark.parametrize("bad", [np.inf, -np.inf])
def test_planted_infinity(ctx, tie_free, at, bad):
    """An infinity at an even or an odd offset, at the first and at the last
    one (n = 130: 8,385 entries, an odd count), with a NaN further on."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 130
    d = tie_free(ctx, 257)[:n * (n - 1) // 2].clone()  # any finite values serve
    d[at] = bad
    if at + 7 < d.numel():
        d[at + 7] = float("nan")
    before = d.cpu().numpy().copy()
    for keep in (False, True):
        with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {at} is not finite$"):
            D.region_nj(ctx, d, keep_input=keep)
        assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    check_device(ctx, tie_free(ctx, 63), "tie free 63")


def test_unaligned_input(ctx, tie_free):
    """A view that starts 8 bytes into an allocation: the check's 8-byte path,
    and row segments whose 16-byte boundaries fall on the other parity."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 65
    src = tie_free(ctx, n)
    buf = torch.empty(src.numel() + 1, dtype=torch.float64, device="cuda")
    view = buf[1:]
    view.copy_(src)
    assert view.data_ptr() % 16 == 8
    want = ref_cached(f"tie free {n}", src.cpu().numpy(), n)
    for keep in (True, False):  # in place: the kernels run on the view itself
        view.copy_(src)
        tree, _ = D.region_nj(ctx, view, keep_input=keep, compact=keep)
        assert_same_nj(tree, want, f"unaligned keep_input={keep}")
    view.copy_(src)
    view[src.numel() - 1] = float("inf")
    with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {src.numel() - 1} is not finite$"):
        D.region_nj(ctx, view)


def test_device_argument_checks(ctx, tie_free):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    d = tie_free(ctx, 65)
    for bad in (d[:7], d[:1], d.cpu(), d.float(), d[:6].view(3, 2), d[:12:2], d.cpu().numpy()):
        with pytest.raises(K.KmerSpansError):
            D.region_nj(ctx, bad)


# ------------------------------------------------------------- the host entry

def test_host_entry(ctx, tie_free):
    import kmer_spans_amd as K
    d = tie_free(ctx, 255)
    tree, _, _ = check_device(ctx, d, "tie free 255")
    assert_same_nj(K.region_nj(d.cpu().numpy()), tree, "host entry")


# ------------------------------------------- beyond the numpy loop's reach

@pytest.mark.parametrize("n", [1025, 2049, 2051, 8200])
def test_additive_trees_come_back_exactly(ctx, n):
    """Rows longer than one block pass.  Branch lengths are multiples of 1/64
    up to 4 and a path has at most n of them: every sum the algorithm forms
    (row sums: n paths) stays below 4 n^2 < 2^53 / 64, so all of it is exact and
    the tree's path lengths are the input.  n = 2,051: 1,025 block minima, the
    first second pass of k_nj_join's reduction over them.  n = 8,200: 4,100 row
    pairs for the 2,048 blocks of k_nj_min, so every block walks two or three
    and merges their minima; three k_nj_join blocks; compactions from 8,200
    and from 4,100 rows (the host builds the 538 MB square once, 3.6 s)."""
    assert 4 * n * n < 2 ** 53 // 64
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(n)
    d = random_additive(rng, n)
    i, j = sample_pairs(rng, n, 10_000)
    assert i.size >= 10_000 and set(i.tolist()) == set(range(n)) and (i != j).all()
    dev = dist_dev(d)
    tree, st = D.region_nj(ctx, dev)
    assert_additive_exact(tree, d, n, i, j, f"additive n={n}")
    assert st["n_compactions"] == predicted_compactions(n)
    flat, _ = D.region_nj(ctx, dev, compact=False)
    assert_same_nj(flat, tree, "without compaction")


# ------------------------------- exact, where k_nj_min's grid is capped

BIG_N = 4100
# The steps the torch reference runs: all n - 3 = 4,097.  Measured on the MI355X, ref_nj_torch on
# "cuda" takes 2.83 s on the tie-free input and 1.99 s on the tie-heavy one, the two tests 3.0 s
# and 2.2 s in all (pytest --durations=0).  Were a test to pass 10 s, this would be
# the largest multiple of 256 that stays within it, never fewer than 256 -- and a prefix is never
# shortened to make a failure go away.
BIG_STEPS = BIG_N - 3


def check_big(ctx, dist, key):
    """device.region_nj at n = 4,100 against ref_nj_torch (tests/njref.py) run
    on "cuda" on the downloaded bits: join equal and length bit-equal over the
    reference's steps, root and root_length when it runs to the end; then
    compact=False against compact=True over all steps."""
    import time
    from kmer_spans_amd import device as D
    from tests.njref import ref_nj_torch
    n = BIG_N
    host = dist.cpu().numpy()
    assert host.size == n * (n - 1) // 2
    t0 = time.perf_counter()
    want = ref_nj_torch(host, n, compact=True, steps=BIG_STEPS, device="cuda")
    print(f"{key}: ref_nj_torch on cuda, {want['steps']} of {n - 3} steps in {time.perf_counter() - t0:.2f} s")
    k = want["steps"]
    assert k == BIG_STEPS >= 256 and (k == n - 3 or k % 256 == 0)
    tree, st = D.region_nj(ctx, dist)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(host)), (key, "keep_input=True changed the input")
    differ = np.flatnonzero((tree["join"][:k] != want["join"]).any(axis=1))
    assert differ.size == 0, (key, "join from step", int(differ[0]), tree["join"][differ[0]], want["join"][differ[0]])
    assert np.array_equal(bits(tree["length"][:k]), bits(want["length"])), (key, "length")
    if k == n - 3:
        assert_same_nj(tree, want, key)
        assert want["n_compactions"] == predicted_compactions(n)
    assert st["n"] == n and st["n_compactions"] == predicted_compactions(n), (key, st)
    flat, st_flat = D.region_nj(ctx, dist, compact=False)
    assert_same_nj(flat, tree, f"{key} without compaction")
    assert st_flat["n_compactions"] == 0 and st_flat["work_bytes"] == 8 * host.size


def test_capped_grid_tie_free(ctx, tie_free):
    """n = 4,100: 2,050 row pairs for 2,048 k_nj_min blocks, so blocks 0 and 1
    walk two pairs and merge their minima; two k_nj_join blocks share the k of
    the update; 2,048 block minima take two passes of the join's reduction;
    the first compaction is from 4,100 rows, five to a thread in k_nj_rank."""
    check_big(ctx, tie_free(ctx, BIG_N), f"tie free {BIG_N}")


def test_capped_grid_tie_heavy(ctx):
    """The same with distances from {1, 2, 3}: across the pairs a block walks
    and across the blocks, equal q must fall to the lower (i, j)."""
    rng = np.random.default_rng(BIG_N)
    d = rng.integers(1, 4, size=BIG_N * (BIG_N - 1) // 2).astype(np.float64)
    check_big(ctx, dist_dev(d), f"ties {BIG_N}")
