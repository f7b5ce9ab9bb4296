"""Silhouette widths, medoids and diameters on the device (ks_silhouette_dev /
ks_silhouette) against the host reference of tests/test_silhouette.py: the
group sums, a, b, width, neighbor, size, medoid, diameter, avg_width and
avg_width_all identical in every bit.  Runs on an MI355X (pytest -m gpu)."""
import numpy as np
import pytest

from tests.test_nj import bits
from tests.test_silhouette import (CHUNK, assert_same_silhouette, order_pin_case, ref_silhouette, tie_heavy_case,
                                   ties_in)
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


def check_device(ctx, dist, group, ngroups=None, what="", want=None):
    """device.region_silhouette (with the sums) on a CUDA tensor against the
    reference on its download; the input's bits are unchanged."""
    from kmer_spans_amd import _lib
    from kmer_spans_amd import device as D
    host = dist.cpu().numpy()
    n = _lib.hclust_n(host.size)
    res, st = D.region_silhouette(ctx, dist, group, ngroups=ngroups, sums=True)
    assert np.array_equal(bits(dist.cpu().numpy()), bits(host)), (what, "the input changed")
    want = ref_silhouette(host, n, group, ngroups) if want is None else want
    got = dict(res, sums=res["sums"].cpu().numpy())
    assert_same_silhouette(got, want, what)
    g = want["size"].size
    chunks = int(((want["size"].astype(np.int64) + CHUNK - 1) // CHUNK).sum())
    assert (st["n"], st["ngroups"], st["n_chunks"]) == (n, g, chunks), (what, st)
    assert st["work_bytes"] >= 52 * n + 8 * chunks + 4 * g
    return res, st, want


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


# ------------------------------------------------------------- known answers

def test_lines(ctx):
    import kmer_spans_amd as K
    from tests.test_silhouette import line_dist
    d = line_dist([0, 1, 3, 10, 12])
    res, _, _ = check_device(ctx, dist_dev(d), [1, 1, 1, 2, 2], what="line, two groups")
    assert res["medoid"].tolist() == [1, 3] and res["diameter"].tolist() == [3.0, 2.0]
    assert res["b"].tolist() == [11.0, 10.0, 8.0, 26.0 / 3.0, 32.0 / 3.0]
    res, _, _ = check_device(ctx, dist_dev(line_dist([0, 1, 5, 6, 20])), [1, 1, 2, 2, 3], what="line, three groups")
    assert res["width"].tolist() == [4.5 / 5.5, 3.5 / 4.5, 3.5 / 4.5, 4.5 / 5.5, 0.0]
    assert res["neighbor"].tolist() == [2, 2, 1, 1, 2] and res["medoid"].tolist() == [0, 2, 4]
    host = K.region_silhouette(d, [1, 1, 1, 2, 2], sums=True)  # api -> host entry
    assert_same_silhouette(host, ref_silhouette(d, 5, [1, 1, 1, 2, 2]), "host entry")


# ----------------------------------------- sizes across strip and chunk edges

def labellings(n: int):
    """(name, labels, ngroups): interleaved and contiguous groups, g = 2 and g = n."""
    i = np.arange(n)
    out = [("two interleaved", i % 2 + 1, 2), ("two contiguous", (i >= (n + 1) // 2) + 1, 2), ("g = n", i + 1, n)]
    if n >= 8:
        out += [("five interleaved", i % 5 + 1, 5), ("three contiguous", i * 3 // n + 1, 3)]
    return out


@pytest.mark.parametrize("n", [2, 3, 4, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_sizes(ctx, tie_free, n):
    """One strip of 64 rows, one chunk of 256 members, and one either side of each."""
    d = tie_free(ctx, n)
    for name, group, g in labellings(n):
        check_device(ctx, d, group.astype(np.int32), g, f"n={n} {name}")


def test_groups_of_exactly_256_257_and_513(ctx, tie_free):
    n = 256 + 257 + 513
    rng = np.random.default_rng(1026)
    group = np.repeat([1, 2, 3], [256, 257, 513])[rng.permutation(n)].astype(np.int32)
    d = tie_free(ctx, 1025)
    import torch
    d = torch.cat([d, d[:n * (n - 1) // 2 - d.numel()] * 0.5])  # any finite values serve
    _, st, want = check_device(ctx, d, group, 3, "256 | 257 | 513")
    assert want["size"].tolist() == [256, 257, 513] and st["n_chunks"] == 1 + 2 + 3


def test_empty_groups_and_ngroups_above_the_largest_label(ctx, tie_free):
    n = 257
    rng = np.random.default_rng(257)
    group = np.array([1, 3, 6])[rng.integers(0, 3, size=n)].astype(np.int32)
    res, _, want = check_device(ctx, tie_free(ctx, n), group, 8, "labels 1 3 6 of 8")
    assert res["medoid"][[1, 3, 4, 6, 7]].tolist() == [-1] * 5 and res["size"][[1, 3, 4, 6, 7]].tolist() == [0] * 5
    assert set(res["neighbor"].tolist()) <= {1, 3, 6}
    dense, _ = check_device(ctx, tie_free(ctx, n), group, None, "labels 1 3 6 of 6")[:2]
    for k in ("width", "a", "b", "neighbor"):
        assert np.array_equal(dense[k], res[k])


# ------------------------------------------------------------------- ties

@pytest.mark.parametrize("n", [130, 600])
def test_tie_heavy(ctx, n):
    """Distances from {0, 1, 2, 3} in groups of five: equal means to several
    groups and equal medoid sums; the lowest label and the lowest index win."""
    d, group, g = tie_heavy_case(n)
    want = ref_silhouette(d, n, group, g)
    b_ties, med_ties = ties_in(want, group)
    print(f"n = {n}: {b_ties} rows with a tie in b, {med_ties} groups with a tie in the medoid")
    assert b_ties > 0 and med_ties > 0
    check_device(ctx, dist_dev(d), group, g, f"ties n={n}", want=want)


def test_all_equal(ctx):
    n = 300
    group = (np.arange(n) % 7 + 1).astype(np.int32)
    res, _, _ = check_device(ctx, dist_dev(np.full(n * (n - 1) // 2, 0.75)), group, 7, "all equal")
    assert not res["width"].any() and res["avg_width_all"] == 0.0 and not res["avg_width"].any()
    assert (res["a"] == 0.75).all() and (res["b"] == 0.75).all() and (res["diameter"] == 0.75).all()
    assert res["medoid"].tolist() == list(range(7))
    assert res["neighbor"].tolist() == [2 if c == 1 else 1 for c in group]


def test_signed_zeros(ctx):
    """-0.0 adds as zero and is no larger than the +0.0 far starts from."""
    n = 150
    rng = np.random.default_rng(150)
    d = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, 2.0]), size=n * (n - 1) // 2)
    assert np.signbit(d).any() and (~np.signbit(d) & (d == 0)).any()
    check_device(ctx, dist_dev(d), (np.arange(n) % 4 + 1).astype(np.int32), 4, "signed zeros")
    zeros = np.where(rng.random(n * (n - 1) // 2) < 0.5, -0.0, 0.0)
    res, _, _ = check_device(ctx, dist_dev(zeros), (np.arange(n) % 4 + 1).astype(np.int32), 4, "only zeros")
    assert not np.signbit(res["sums"].cpu().numpy()).any() and not np.signbit(res["diameter"]).any()


def test_order_pin(ctx):
    """Sixty binades and a group of 600: only the chunked order gives these bits."""
    d, n, group, g = order_pin_case()
    check_device(ctx, dist_dev(d), group, g, "order pin")


# ------------------------------------------------------------ call behaviour

def test_repeat_and_sums_flag(ctx, tie_free):
    """The same call twice gives the same bits; sums=False gives the same other outputs."""
    from kmer_spans_amd import device as D
    n = 513
    d = tie_free(ctx, n)
    group = (np.arange(n) * 7 % 11 + 1).astype(np.int32)
    first, _, want = check_device(ctx, d, group, 11, "first")
    again, _ = D.region_silhouette(ctx, d, group, sums=True)
    plain, _ = D.region_silhouette(ctx, d, group)
    assert "sums" not in plain
    assert np.array_equal(bits(again["sums"].cpu().numpy()), bits(first["sums"].cpu().numpy()))
    for other in (again, plain):
        assert_same_silhouette(other, want, "again", sums=False)
    import torch
    as_tensor, _ = D.region_silhouette(ctx, d, torch.from_numpy(group).cuda())  # a CUDA tensor is downloaded
    assert_same_silhouette(as_tensor, want, "labels from a tensor", sums=False)


def test_nan_from_an_empty_row(ctx, tie_free):
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
    group = (np.arange(90) % 3 + 1).astype(np.int32)
    with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {first} is not finite$"):
        D.region_silhouette(ctx, d, group, sums=True)
    assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    check_device(ctx, tie_free(ctx, 63), (np.arange(63) % 3 + 1).astype(np.int32), 3, "after a rejected call")


@pytest.mark.parametrize("at", [0, 1, 4095, 8384])
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
    group = (np.arange(n) % 2 + 1).astype(np.int32)
    with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {at} is not finite$"):
        D.region_silhouette(ctx, d, group)
    assert np.array_equal(bits(d.cpu().numpy()), bits(before))
    check_device(ctx, tie_free(ctx, 63), (np.arange(63) % 2 + 1).astype(np.int32), 2, "after a rejected call")


def test_unaligned_input(ctx, tie_free):
    """A view that starts 8 bytes into an allocation: the check's 8-byte path
    and the kernel's 8-byte loads."""
    import torch
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 65
    src = tie_free(ctx, n)
    buf = torch.empty(src.numel() + 1, dtype=torch.float64, device="cuda")
    view = buf[1:]
    view.copy_(src)
    assert view.data_ptr() % 16 == 8
    group = (np.arange(n) % 3 + 1).astype(np.int32)
    check_device(ctx, view, group, 3, "unaligned")
    view[src.numel() - 1] = float("inf")
    with pytest.raises(K.KmerSpansError, match=f"^dissimilarity at offset {src.numel() - 1} is not finite$"):
        D.region_silhouette(ctx, view, group)


def test_device_argument_checks(ctx, tie_free):
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    d = tie_free(ctx, 65)
    group = (np.arange(65) % 2 + 1).astype(np.int32)
    for bad in (d[:7], d.cpu(), d.float(), d[:6].view(3, 2), d[:12:2], d.cpu().numpy()):
        with pytest.raises(K.KmerSpansError):
            D.region_silhouette(ctx, bad, group)
    with pytest.raises(K.KmerSpansError, match="group must hold"):
        D.region_silhouette(ctx, d, group[:64])
    with pytest.raises(K.KmerSpansError, match="^group\\[3\\] = 2 is not in 1 .. 1$"):
        D.region_silhouette(ctx, d, np.where(np.arange(65) == 3, 2, 1), ngroups=1)
    with pytest.raises(K.KmerSpansError, match="at least 2 non-empty groups"):
        D.region_silhouette(ctx, d, np.full(65, 2, dtype=np.int32), ngroups=3)


def test_host_entry(ctx, tie_free):
    import kmer_spans_amd as K
    n = 257
    d = tie_free(ctx, n)
    group = np.array([1, 2, 5])[np.arange(n) % 3].astype(np.int32)
    _, _, want = check_device(ctx, d, group, 6, "device entry")
    host = K.region_silhouette(d.cpu().numpy(), group, ngroups=6, sums=True)
    assert_same_silhouette(host, want, "host entry")
    assert_same_silhouette(K.region_silhouette(d.cpu().numpy(), group, ngroups=6), want, "host entry", sums=False)


# ------------------------------------------------------------------ pipeline

def test_pipeline_scan_spectra_distances_hclust_cut_silhouette(ctx):
    """A planted-repeat scan, then device.region_spectra, region_distances,
    region_hclust, cut_tree(h=) and device.region_silhouette: nothing but the
    tree and the labels leaves the device before the result.  Every diameter
    is within the cut height; at h = 0 the two poly-A regions (nothing but
    AAAA / TTTT windows, so proportional counts) form a group of diameter 0."""
    import torch
    import kmer_spans_amd as K
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
    tree, _ = D.region_hclust(ctx, dist)  # complete linkage; keeps dist
    height = tree["height"]
    below = height[height < height[-1]]
    assert below.size, "the tree has one height only"
    h = float(below[below.size // 2])  # a cut that leaves at least two groups
    group = K.cut_tree(tree, h=h)
    res, st = D.region_silhouette(ctx, dist, group, sums=True)
    assert (res["diameter"] <= h).all() and res["size"].sum() == R and st["work_bytes"] > 0
    # only now the distances come back, for the reference
    assert_same_silhouette(dict(res, sums=res["sums"].cpu().numpy()),
                           ref_silhouette(dist.cpu().numpy(), R, group), "pipeline")

    def region_in(name):
        at, unit = plants[name]
        hit = [r for r in range(R) if min(pos[2, r], at + len(unit)) - max(pos[1, r], at + 1) + 1 > len(unit) // 2]
        assert len(hit) == 1, (name, pos.T.tolist())
        return hit[0]
    ra, rb = region_in("a150"), region_in("a420")
    assert group[ra] == group[rb]
    zero = K.cut_tree(tree, h=0.0)
    tight, _ = D.region_silhouette(ctx, dist, zero)
    c = zero[ra] - 1
    assert zero[rb] == zero[ra] and tight["size"][c] == 2 and tight["diameter"][c] == 0.0
    assert tight["a"][ra] == 0.0 and tight["a"][rb] == 0.0 and tight["medoid"][c] == min(ra, rb)
    assert tight["width"][ra] == 1.0 and tight["width"][rb] == 1.0
    print(f"{R} regions; h = {h}: {res['size'].size} groups, avg width {res['avg_width_all']:.4f}; "
          f"poly-A regions {ra} and {rb} in group {group[ra]}")


# -------------------------------------------------------- scale: invariants

def test_scale_invariants(ctx):
    """n = 8,192 (268 MB), k = 10 groups of the complete-linkage tree: the host
    reference is too slow here, so only what must hold of any result."""
    import kmer_spans_amd as K
    from kmer_spans_amd import device as D
    n = 8192
    d, _ = D.region_distances(ctx, to_dev(random_counts(np.random.default_rng(8192), n, 16)))
    tree, _ = D.region_hclust(ctx, d)
    group = K.cut_tree(tree, k=10)
    res, st = D.region_silhouette(ctx, d, group)
    print(f"n = {n}: ms_check {st['ms_check']:.3f} ms_sums {st['ms_sums']:.3f} ms_widths {st['ms_widths']:.3f} "
          f"chunks {st['n_chunks']} work_bytes {st['work_bytes']} sizes {res['size'].tolist()}")
    assert (res["width"] >= -1).all() and (res["width"] <= 1).all()
    assert res["size"].sum() == n and np.array_equal(res["size"], np.bincount(group, minlength=11)[1:])
    assert (group[res["medoid"]] == np.arange(1, 11)).all()
    assert (res["neighbor"] != group).all() and (res["neighbor"] >= 1).all() and (res["neighbor"] <= 10).all()
    assert (res["diameter"] <= tree["height"][-1]).all() and (res["diameter"] >= 0).all()
    assert (res["a"] >= 0).all() and (res["b"] > 0).all() and st["n"] == n and st["ngroups"] == 10
    single = res["size"][group - 1] == 1
    assert not res["width"][single].any()
