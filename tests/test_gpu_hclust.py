"""Hierarchical clustering on the device (ks_hclust_dev / ks_hclust) against
the host reference of tests/test_hclust.py: merge, the bits of height and order
identical, and the count of rescanned rows.  Runs on an MI355X (pytest -m gpu)."""
import numpy as np
import pytest

from tests.test_hclust import METHODS, assert_same_tree, bits, ref_cut, ref_tree
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


def n_of(length: int) -> int:
    from kmer_spans_amd import _lib
    return _lib.hclust_n(length)


def check_device(ctx, dist, method, what="", want=None):
    """device.region_hclust on a CUDA tensor against the reference on its download."""
    from kmer_spans_amd import device as D
    host = dist.cpu().numpy()
    n = n_of(host.size)
    tree, st = D.region_hclust(ctx, dist, method=method)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(host)), (what, "keep_input=True changed the input")
    want = ref_tree(host, n, method) if want is None else want
    assert_same_tree(tree, want, what)
    assert tree["method"] == method and st["n"] == n
    assert st["n_rescans"] == want["n_rescans"], (what, st["n_rescans"], want["n_rescans"])
    return tree, st, want


# ------------------------------------------------------------- known answers

@pytest.mark.parametrize("method", METHODS)
def test_line_of_five(ctx, method):
    import kmer_spans_amd as K
    from tests.test_hclust import LINE5, LINE5_HEIGHT, LINE5_MERGE, LINE5_ORDER, line_dist
    d = line_dist(LINE5)
    tree, _, _ = check_device(ctx, dist_dev(d), method, "line of five")
    assert tree["merge"].tolist() == LINE5_MERGE and tree["order"].tolist() == LINE5_ORDER
    assert tree["height"].tolist() == LINE5_HEIGHT[method]
    host = K.region_hclust(d, method=method)  # api -> host entry
    assert_same_tree(host, tree, "host entry")


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


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1025])
def test_sizes(ctx, tie_free, n, method):
    """One wave, one block stride, and one entry either side of each."""
    check_device(ctx, tie_free(ctx, n), method, f"n={n} {method}")


# ------------------------------------------------------------------- ties

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [130, 600])
def test_tie_heavy(ctx, n, method):
    """Distances drawn from {0, 1, 2, 3}: many equal minima, many rescans per step."""
    rng = np.random.default_rng(n)
    d = rng.integers(0, 4, size=n * (n - 1) // 2).astype(np.float64)
    _, st, _ = check_device(ctx, dist_dev(d), method, f"ties n={n} {method}")
    print(f"n = {n} {method}: {st['n_rescans']} rescans in {n - 1} steps")
    assert st["n_rescans"] > n


@pytest.mark.parametrize("method", METHODS)
def test_all_equal(ctx, method):
    n = 300
    tree, _, _ = check_device(ctx, dist_dev(np.full(n * (n - 1) // 2, 0.75)), method, "all equal")
    assert tree["merge"].tolist() == [[-1, -2]] + [[-(s + 2), s] for s in range(1, n - 1)]
    assert tree["order"].tolist() == list(range(n, 2, -1)) + [1, 2]
    assert tree["height"].tolist() == [0.75] * (n - 1)


@pytest.mark.parametrize("method", METHODS)
def test_signed_zeros(ctx, method):
    """-0.0 and +0.0 compare equal: the index decides, on the device as on the host."""
    n = 150
    rng = np.random.default_rng(150)
    d = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, 2.0]), size=n * (n - 1) // 2)
    assert np.signbit(d).any() and (~np.signbit(d) & (d == 0)).any()
    check_device(ctx, dist_dev(d), method, "signed zeros")


# --------------------------------------------------- proportional families

def test_proportional_families_merge_first(ctx):
    """Rows x2, x3, x1000 of one row are at distance exactly 0: the families
    merge before anything else, at height 0, and a cut at h = 0 puts each
    family in one group and every other row in a group of its own."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(6)
    c = random_counts(rng, 70, 256, hi=4000)
    fams = [(10, 11, 40, 69), (3, 50, 51)]
    for fam in fams:
        base = c[fam[0]].astype(np.uint64)
        for row, f in zip(fam[1:], (2, 3, 1000)):
            c[row] = (base * f).astype(np.uint32)
    d, _ = D.region_distances(ctx, to_dev(c))
    tree, _, _ = check_device(ctx, d, "complete", "proportional")
    zero_merges = sum(len(f) - 1 for f in fams)
    assert not tree["height"][:zero_merges].any() and tree["height"][zero_merges] > 0
    g = K.cut_tree(tree, h=0.0)
    assert np.array_equal(g, ref_cut(tree["merge"], tree["height"], 70, h=0.0))
    assert len(set(g.tolist())) == 70 - zero_merges
    for fam in fams:
        assert len(set(g[list(fam)].tolist())) == 1
        assert (g == g[fam[0]]).sum() == len(fam)


# ------------------------------------------------------------------ pipeline

def test_pipeline_scan_spectra_distances_hclust(ctx):
    """The planted-repeat scan of test_pipeline_scan_spectra_distances, then
    device.region_spectra, device.region_distances and device.region_hclust
    with nothing downloaded in between: the tree is the reference's on the
    downloaded distances, and the two poly-A regions (nothing but AAAA / TTTT
    windows, so proportional counts) are joined at height 0."""
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
    tree, st = D.region_hclust(ctx, dist, keep_input=False)  # the distances are consumed: the scan's pos are host data
    del dist
    # only now anything comes back: the distances again, for the reference
    again, _ = D.region_distances(ctx, sp)
    want = ref_tree(again.cpu().numpy(), R, "complete")
    assert_same_tree(tree, want, "pipeline")
    assert st["n_rescans"] == want["n_rescans"] and st["work_bytes"] == 0

    def region_in(name):
        at, unit = plants[name]
        hit = [r for r in range(R) if min(pos[2, r], at + len(unit)) - max(pos[1, r], at + 1) + 1 > len(unit) // 2]
        assert len(hit) == 1, (name, pos.T.tolist())
        return hit[0]
    ra, rb = sorted((region_in("a150"), region_in("a420")))
    rows = tree["merge"].tolist()
    assert [-(ra + 1), -(rb + 1)] in rows
    at = rows.index([-(ra + 1), -(rb + 1)])
    assert tree["height"][at] == 0.0
    print(f"{R} regions; poly-A regions {ra} and {rb} joined at step {at}, height {tree['height'][at]}")


# ---------------------------------------------------------------- keep_input

@pytest.mark.parametrize("method", METHODS)
def test_keep_input(ctx, tie_free, method):
    from kmer_spans_amd import device as D
    n = 257
    d = tie_free(ctx, n).clone()
    before = d.cpu().numpy().copy()
    kept, st_kept = D.region_hclust(ctx, d, method=method, keep_input=True)
    assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    used, st_used = D.region_hclust(ctx, d, method=method, keep_input=False)
    assert_same_tree(used, kept, "keep_input=False")
    assert st_kept["work_bytes"] - st_used["work_bytes"] == 8 * before.size
    assert st_used["n_rescans"] == st_kept["n_rescans"]
    assert not np.array_equal(bits(d.cpu().numpy()), bits(before)), "in place: the matrix was updated"


# --------------------------------------------------------- non-finite entries

def test_nan_from_an_empty_row(ctx):
    """An empty spectrum row is NaN against every row: the call names the
    first such offset, leaves the input alone, and the context works on."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    rng = np.random.default_rng(11)
    c = random_counts(rng, 90, 16)
    c[37] = 0
    d, _ = D.region_distances(ctx, to_dev(c))
    before = d.cpu().numpy().copy()
    first = int(np.flatnonzero(np.isnan(before))[0])
    assert first == 36  # pair (0, 37)
    for keep in (True, False):
        with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {first} is not finite$"):
            D.region_hclust(ctx, d, keep_input=keep)
        after = d.cpu().numpy()
        assert np.array_equal(bits(after), bits(before))
    c[37] = c[36]
    good, _ = D.region_distances(ctx, to_dev(c))
    check_device(ctx, good, "complete", "after a rejected call")


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
            D.region_hclust(ctx, d, keep_input=keep)
        assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    check_device(ctx, tie_free(ctx, 63), "single", "after a rejected call")


def test_unaligned_input(ctx, tie_free):
    """A view that starts 8 bytes into an allocation: the check's 8-byte path."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 65
    src = tie_free(ctx, n)
    buf = torch.empty(src.numel() + 1, dtype=torch.float64, device="cuda")
    view = buf[1:]
    view.copy_(src)
    assert view.data_ptr() % 16 == 8
    tree, _, _ = check_device(ctx, view, "complete", "unaligned")
    view[src.numel() - 1] = float("inf")
    with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {src.numel() - 1} is not finite$"):
        D.region_hclust(ctx, view)


def test_device_argument_checks(ctx, tie_free):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    d = tie_free(ctx, 65)
    for bad in (d[:7], d.cpu(), d.float(), d[:6].view(3, 2), d[:12:2], d.cpu().numpy()):
        with pytest.raises(K.KmerSpansError):
            D.region_hclust(ctx, bad)
    with pytest.raises(K.KmerSpansError, match="method must be one of"):
        D.region_hclust(ctx, d, method="ward")


# ------------------------------------------------------------- the host entry

@pytest.mark.parametrize("method", METHODS)
def test_host_entry(ctx, tie_free, method):
    import kmer_spans_amd as K
    d = tie_free(ctx, 255)
    tree, _, want = check_device(ctx, d, method, "device entry")
    host = K.region_hclust(d.cpu().numpy(), method=method)
    assert_same_tree(host, tree, "host entry")
    assert host["method"] == method


# ------------------------------------- the finiteness pass past its first stride

def check_stride(max_bytes=1 << 30):
    """(E, n): the entries a full grid of check_all_finite (8 * num_cus blocks
    of 256 threads, 16 bytes a thread) reads in one stride, and the smallest n
    whose condensed vector holds an odd count of more than 2 E + 3 entries, so
    that some threads take a third item and thread 0 the odd tail."""
    import torch
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    E = 2 * 256 * 8 * num_cus
    n = int(np.sqrt(4.0 * E)) - 2
    while n * (n - 1) // 2 <= 2 * E + 3 or not (n * (n - 1) // 2) & 1:
        n += 1
    if 8 * (n * (n - 1) // 2) > max_bytes:
        pytest.skip(f"{num_cus} CUs: a vector of more than two strides of the check would pass 1 GB")
    return E, n


@pytest.fixture(scope="module")
def long_vector():
    """(E, n, finite values on the device); the tests work on clones."""
    import torch
    E, n = check_stride()
    gen = torch.Generator(device="cuda").manual_seed(n)
    return E, n, torch.rand(n * (n - 1) // 2, dtype=torch.float64, device="cuda", generator=gen)


def assert_names(call, d, at):
    """call(d, keep) is refused naming offset `at`, keep_input both ways, and no bit of d changes."""
    import torch
    import kmer_spans_amd as K
    before = d.clone()
    for keep in (False, True):
        with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {at} is not finite$"):
            call(d, keep)
        assert torch.equal(d.view(torch.int64), before.view(torch.int64)), (at, keep, "the input changed")


PLANTS = {"E-1": lambda E, total: E - 1, "E": lambda E, total: E, "E+1": lambda E, total: E + 1,
          "2E+1": lambda E, total: 2 * E + 1, "last": lambda E, total: total - 1}


@pytest.mark.parametrize("where", list(PLANTS))
@pytest.mark.parametrize("bad", [np.inf, np.nan])
def test_planted_past_the_first_stride(ctx, long_vector, where, bad):
    """One bad entry where only a later grid-stride item of k_hclust_check
    reads it: the last entry of the first stride, the first two of the second,
    one of the third, and the odd tail that thread 0 reads after its loop
    (n = 2,050 at 256 CUs: 2,100,225 entries, 0.1 s a case)."""
    from kmer_spans_amd import device as D
    E, n, src = long_vector
    total = src.numel()
    assert total > 2 * E + 3 and total & 1 and src.data_ptr() % 16 == 0
    at = PLANTS[where](E, total)
    d = src.clone()
    assert d.data_ptr() % 16 == 0
    d[at] = float(bad)
    assert_names(lambda x, keep: D.region_hclust(ctx, x, keep_input=keep), d, at)


def test_two_planted_the_lower_is_named(ctx, long_vector):
    """Two bad entries: the lower one at a later item of a higher thread than
    the higher one (the threads settle it by atomicMin), then both in one
    thread (its first hit stays)."""
    from kmer_spans_amd import device as D
    E, n, src = long_vector
    threads = E // 2  # a thread reads two entries per item
    for lo, hi in ((E + 2 * (threads - 1), 2 * E + 3), (E + 6, 2 * E + 6), (E - 3, E + 1)):
        assert lo < hi < src.numel()
        d = src.clone()
        d[lo], d[hi] = float("nan"), float("-inf")
        assert_names(lambda x, keep: D.region_hclust(ctx, x, keep_input=keep), d, lo)


@pytest.mark.parametrize("where", ["E/2-1", "E/2", "E+1", "last"])
def test_planted_past_the_first_stride_unaligned(ctx, long_vector, where):
    """The same on a view that starts 8 bytes into an allocation: k_hclust_check1
    reads one entry per item, so its stride is E / 2 entries."""
    import torch
    from kmer_spans_amd import device as D
    E, n, src = long_vector
    buf = torch.empty(src.numel() + 1, dtype=torch.float64, device="cuda")
    view = buf[1:]
    view.copy_(src)
    assert view.data_ptr() % 16 == 8
    at = {"E/2-1": E // 2 - 1, "E/2": E // 2, "E+1": E + 1, "last": src.numel() - 1}[where]
    view[at] = float("inf")
    if at + E // 2 < src.numel():
        view[at + E // 2] = float("nan")  # the same thread's next item
    assert_names(lambda x, keep: D.region_hclust(ctx, x, keep_input=keep), view, at)


def test_nj_and_silhouette_past_the_first_stride(ctx, long_vector):
    """region_nj and region_silhouette run the same pass, each with a result word of its own."""
    from kmer_spans_amd import device as D
    E, n, src = long_vector
    group = (np.arange(n) % 2 + 1).astype(np.int32)
    d = src.clone()
    d[E + 1] = float("nan")
    assert_names(lambda x, keep: D.region_nj(ctx, x, keep_input=keep), d, E + 1)
    d = src.clone()
    d[2 * E + 1] = float("inf")
    assert_names(lambda x, keep: D.region_silhouette(ctx, x, group), d, 2 * E + 1)
    d[E] = float("nan")
    assert_names(lambda x, keep: D.region_nj(ctx, x, keep_input=keep), d, E)
    good = src[:10].clone()  # the words are clear again: n = 5 goes through
    D.region_hclust(ctx, good)
    D.region_nj(ctx, good)


# ------------------------------------ exact, where the blocks of a step multiply

@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [4096, 4097])
def test_two_pair_blocks(ctx, tie_free, n, method):
    """The last grid of one k_hclust_pair block and the first of two: from
    4,097 on every block repeats the arg-min, the blocks share the k of the row
    update (k0 + u * 2048) and append to one list.  ref_tree takes 1.3 s at
    this size on a slow host (complete and average; single 0.8 s); a case,
    reference included, 0.4 to 0.7 s on the MI355X machine."""
    check_device(ctx, tie_free(ctx, n), method, f"n={n} {method}")


@pytest.mark.parametrize("method", ["complete", "average"])
def test_three_pair_blocks(ctx, tie_free, method):
    """n = 8,193: three blocks, k = k0 + u * 3072.  ref_tree is most of the
    test's time: about 5 s on a slow host, and the whole case 1.7 s on the
    MI355X machine."""
    check_device(ctx, tie_free(ctx, 8193), method, f"n=8193 {method}")


TIE_RICH_V = 128


@pytest.mark.parametrize("method", METHODS)
def test_two_pair_blocks_tie_rich(ctx, method):
    """n = 4,097, integers from {0 .. V-1}, V = 128, as star_ties of
    tests/test_hclust.py lays them out: up to 63 rows are listed in one step,
    by both blocks of k_hclust_pair, and rescanned in four rounds of the 16
    blocks of k_hclust_rescan.  The order of the list is whatever the atomic
    counter gives; the tree and the count must not depend on it.

    ref_tree alone, measured on the host: complete 1.0 s and 27,023 rescans,
    single 1.8 s and 135,068, average 1.0 s and 27,133, against 4 n = 16,388
    (a case on the MI355X machine, reference included: 0.6, 1.0 and 0.6 s).
    Every V from 1 up finishes in under 2 s, so the time does not choose V;
    V = 128 is the smallest power of two at which a step lists several times
    the 16 rows that k_hclust_rescan takes side by side (V = 16 is the
    smallest that reaches 4 n for every method, with at most 7 rows a step).
    Uniform integers never reach 4 n for single linkage (star_ties has the
    figures), which is why the input is laid out."""
    from tests.test_hclust import star_ties
    n = 4097
    d = star_ties(np.random.default_rng(n), n, TIE_RICH_V)
    assert d.min() == 0 and d.max() == TIE_RICH_V - 1 and (d == np.floor(d)).all()
    _, st, want = check_device(ctx, dist_dev(d), method, f"tie rich n={n} {method}")
    print(f"n = {n} {method} V = {TIE_RICH_V}: {want['n_rescans']} rescans in {n - 1} steps")
    assert want["n_rescans"] >= 4 * n


# -------------------------------------------------------- scale: invariants

@pytest.fixture(scope="module")
def big(ctx):
    from kmer_spans_amd import device as D
    n = 8192
    d, _ = D.region_distances(ctx, to_dev(random_counts(np.random.default_rng(8192), n, 16)))
    return n, d


@pytest.mark.parametrize("method", METHODS)
def test_scale_invariants(ctx, big, method):
    """n = 8,192 (268 MB): what must hold of any tree of this contract, for all
    three methods.  A tree built from a stale nearest neighbour can satisfy all
    of it; the host reference is not too slow at this size (about 5 s a
    method), and test_two_pair_blocks and test_three_pair_blocks compare
    against it exactly at n = 4,096, 4,097 and 8,193."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n, d = big
    tree, st = D.region_hclust(ctx, d, method=method)
    print(f"n = {n} {method}: ms_check {st['ms_check']:.3f} ms_init {st['ms_init']:.3f} ms_merge {st['ms_merge']:.3f} "
          f"n_rescans {st['n_rescans']}")
    merge, height, order = tree["merge"], tree["height"], tree["order"]
    assert (np.diff(height) >= 0).all()
    if method == "complete":
        assert bits(height[-1:])[0] == bits(d.max().cpu().numpy())
        assert bits(height[:1])[0] == bits(d.min().cpu().numpy())
    if method == "single":
        assert bits(height[:1])[0] == bits(d.min().cpu().numpy())
    flat = merge.ravel()
    step = np.repeat(np.arange(n - 1), 2)
    assert ((flat < 0) | (flat <= step)).all() and (flat != 0).all() and (flat >= -n).all()
    assert np.unique(flat).size == flat.size  # every observation and every step but the last, once each
    assert flat.size == 2 * (n - 1) and set(np.abs(flat[flat < 0]).tolist()) == set(range(1, n + 1))
    assert np.array_equal(np.sort(order), np.arange(1, n + 1))
    g = K.cut_tree(tree, k=10)
    assert set(g.tolist()) == set(range(1, 11)) and g[0] == 1
    assert st["n"] == n and st["n_rescans"] >= n - 1 and st["work_bytes"] == 8 * d.numel()
