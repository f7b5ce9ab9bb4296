"""Neighbour joining of a condensed dissimilarity vector (ks_nj / ks_nj_dev /
ks_nj_edges, include/kmer_spans.h): the host reference the GPU tests compare
against bit for bit (a numpy transcription of the header's contract, masked
and compacting), additive trees that must come back exactly, known answers
worked by hand, the host-only edge table through ctypes, the Newick writer,
and the argument checks of the device entries, which all happen before any
device use -- this file runs without a GPU."""
import numpy as np
import pytest

MIN_DIM = 8  # no compaction to fewer rows (ks_nj_dev's description in the header)


# ------------------------------------------------------------ host reference

def square0(d, n: int) -> np.ndarray:
    """The condensed vector as a full symmetric matrix, +0.0 on the diagonal."""
    m = np.zeros((n, n))
    i, j = np.triu_indices(n, 1)
    m[i, j] = d
    m[j, i] = d
    return m


def predicted_compactions(n: int) -> int:
    """How often ks_nj_dev compacts: after a join that leaves r <= m / 2 live
    rows of the m stored ones, r >= MIN_DIM."""
    m, c = n, 0
    for s in range(n - 3):
        left = n - s - 1
        if 2 * left <= m and left >= MIN_DIM:
            m, c = left, c + 1
    return c


def ref_nj(d, n: int, compact: bool = False):
    """The header's algorithm, step for step.  compact=False masks dead rows,
    compact=True drops them from the stored matrix at the device's threshold;
    the two must agree in every bit.  np.cumsum sums in order (np.sum does
    not); the +0.0 of the diagonal changes no partial sum, which starts at
    +0.0 and so is never -0.0.  np.argmin of the row-major q returns the first
    minimum, which is the tie rule (and compares -0.0 equal to +0.0); a NaN q
    is no candidate, as on the device, where it fails every <."""
    d = np.asarray(d, dtype=np.float64)
    assert d.shape == (n * (n - 1) // 2,) and n >= 3 and np.isfinite(d).all()
    M = square0(d, n)
    S = np.cumsum(M, axis=1)[:, -1].copy()
    live = np.ones(n, dtype=bool)
    node = -(np.arange(n, dtype=np.int64) + 1)
    join = np.zeros((n - 3, 2), dtype=np.int32)
    length = np.zeros((n - 3, 2), dtype=np.float64)
    r, compactions = n, 0
    for s in range(n - 3):
        m = M.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            q = (float(r - 2) * M - S[:, None]) - S[None, :]
        ok = np.triu(live[:, None] & live[None, :], 1) & (q < np.inf)
        q = np.where(ok, q, np.inf)
        at = int(np.argmin(q))
        a, b = divmod(at, m)
        if not q[a, b] < np.inf:
            raise ArithmeticError("no pair has q < +inf")
        dab = M[a, b]
        delta = (S[a] - S[b]) / float(r - 2)
        join[s] = node[a], node[b]
        length[s] = 0.5 * (dab + delta), 0.5 * (dab - delta)
        k = live.copy()
        k[[a, b]] = False
        x, y = M[a, k], M[b, k]
        dn = 0.5 * ((x + y) - dab)
        S[k] = ((S[k] - x) - y) + dn
        M[a, k] = dn
        M[k, a] = dn
        S[a] = 0.5 * ((S[a] + S[b]) - float(r) * dab)
        live[b] = False
        node[a] = s + 1
        r -= 1
        if compact and 2 * r <= m and r >= MIN_DIM:
            keep = np.flatnonzero(live)
            M, S, node, live = M[np.ix_(keep, keep)], S[keep], node[keep], np.ones(r, dtype=bool)
            compactions += 1
    x, y, z = (int(v) for v in np.flatnonzero(live))
    root = np.array([node[x], node[y], node[z]], dtype=np.int32)
    root_length = np.array([0.5 * ((M[x, y] + M[x, z]) - M[y, z]), 0.5 * ((M[x, y] + M[y, z]) - M[x, z]),
                            0.5 * ((M[x, z] + M[y, z]) - M[x, y])])
    return {"join": join, "length": length, "root": root, "root_length": root_length, "n_compactions": compactions}


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same_nj(got, want, what=""):
    assert np.array_equal(got["join"], want["join"]), (what, "join", got["join"][:6], want["join"][:6])
    assert np.array_equal(bits(got["length"]), bits(want["length"])), (what, "length")
    assert np.array_equal(got["root"], want["root"]), (what, "root", got["root"], want["root"])
    assert np.array_equal(bits(got["root_length"]), bits(want["root_length"])), (what, "root_length")


# ----------------------------------------------------- path lengths of a tree

def tree_parents(tree, n: int):
    """(parent, length to the parent, edges to the root) per node: leaf i is i,
    the node of step t is n + t, the trifurcation 2n - 3 (its own parent)."""
    top = 2 * n - 3
    idx = lambda c: -c - 1 if c < 0 else n + c - 1  # noqa: E731
    parent = np.full(top + 1, -1, dtype=np.int64)
    plen = np.zeros(top + 1)
    for t in range(n - 3):
        for c in range(2):
            v = idx(int(tree["join"][t, c]))
            parent[v], plen[v] = n + t, tree["length"][t, c]
    for c in range(3):
        v = idx(int(tree["root"][c]))
        parent[v], plen[v] = top, tree["root_length"][c]
    parent[top] = top
    assert (parent >= 0).all()
    level = np.zeros(top + 1, dtype=np.int64)
    depth = np.zeros(top + 1)
    order = [top] + list(range(n + n - 4, n - 1, -1))  # a step's parent is a later step or the trifurcation
    kids = [[] for _ in range(top + 1)]
    for v in range(top):
        kids[parent[v]].append(v)
    for u in order:
        for v in kids[u]:
            level[v], depth[v] = level[u] + 1, depth[u] + plen[v]
    return parent, depth, level


def path_lengths(tree, n: int, i, j) -> np.ndarray:
    """Leaf-to-leaf path lengths for the pairs (i[x], j[x]), through node
    depths and lowest common ancestors, all pairs climbing at once."""
    parent, depth, level = tree_parents(tree, n)
    u, v = np.array(i, dtype=np.int64), np.array(j, dtype=np.int64)
    while True:
        up_u, up_v = level[u] > level[v], level[v] > level[u]
        same = ~up_u & ~up_v & (u != v)
        if not (up_u | up_v | same).any():
            break
        u = np.where(up_u | same, parent[u], u)
        v = np.where(up_v | same, parent[v], v)
    return (depth[np.asarray(i)] + depth[np.asarray(j)]) - 2.0 * depth[u]


def random_additive(rng, n: int):
    """The condensed distances of a random unrooted binary tree of n leaves
    with branch lengths in {1/64 .. 4}: clusters are joined at random, h is a
    leaf's distance to the root of its cluster.  Every sum is a small multiple
    of 1/64 and exact."""
    D = np.zeros((n, n))
    h = np.zeros(n)
    clusters = [np.array([i]) for i in range(n)]

    def link(A, B, la, lb):
        D[np.ix_(A, B)] = (h[A] + la)[:, None] + (h[B] + lb)[None, :]
        D[np.ix_(B, A)] = D[np.ix_(A, B)].T

    ln = lambda: float(rng.integers(1, 257)) / 64.0  # noqa: E731
    while len(clusters) > 3:
        x, y = sorted(rng.choice(len(clusters), size=2, replace=False))
        B, A = clusters.pop(y), clusters.pop(x)
        la, lb = ln(), ln()
        link(A, B, la, lb)
        h[A] += la
        h[B] += lb
        clusters.append(np.concatenate([A, B]))
    ls = [ln(), ln(), ln()]
    for p in range(3):
        for q in range(p + 1, 3):
            link(clusters[p], clusters[q], ls[p], ls[q])
    i, j = np.triu_indices(n, 1)
    return D[i, j].copy()


def sample_pairs(rng, n: int, count: int):
    """Pairs i != j that include every leaf."""
    i = np.concatenate([np.arange(n), rng.integers(0, n, size=max(count - n, 0))])
    j = (i + rng.integers(1, n, size=i.size)) % n
    return i, j


def assert_additive_exact(tree, d, n: int, i, j, what=""):
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    want = np.asarray(d)[lo * n - lo * (lo + 1) // 2 + (hi - lo - 1)]
    got = path_lengths(tree, n, i, j)
    assert np.array_equal(got, want), (what, float(np.abs(got - want).max()))
    assert (tree["length"] >= 0).all() and (tree["root_length"] >= 0).all(), (what, "a negative length")


# ------------------------------------------------- the reference's properties

@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("kind", ["uniform", "ties"])
def test_masked_and_compacting_reference_agree(n, kind):
    rng = np.random.default_rng(n)
    size = n * (n - 1) // 2
    d = rng.random(size) if kind == "uniform" else rng.integers(1, 4, size=size).astype(np.float64)
    masked, compacted = ref_nj(d, n), ref_nj(d, n, compact=True)
    assert_same_nj(compacted, masked, f"{kind} n={n}")
    assert masked["n_compactions"] == 0 and compacted["n_compactions"] == predicted_compactions(n) > 0


def test_predicted_compactions():
    assert [predicted_compactions(n) for n in (3, 15, 16, 17, 64, 513)] == [0, 0, 1, 1, 3, 6]


@pytest.mark.parametrize("n", [4, 5, 17, 60])
def test_additive_trees_come_back_exactly(n):
    rng = np.random.default_rng(1000 + n)
    d = random_additive(rng, n)
    i, j = np.triu_indices(n, 1)
    for compact in (False, True):
        assert_additive_exact(ref_nj(d, n, compact), d, n, i, j, f"n={n}")


# ------------------------------------- the torch reference (tests/njref.py)

def torch_ref_cases():
    """(name, n, d): the inputs that tie ref_nj_torch to ref_nj."""
    def size(n):
        return n * (n - 1) // 2
    out = [(f"uniform {n}", n, np.random.default_rng(n).random(size(n))) for n in (5, 65, 257)]
    out.append(("ties 130", 130, np.random.default_rng(130).integers(1, 4, size=size(130)).astype(np.float64)))
    out.append(("signed zeros 200", 200, np.random.default_rng(200).choice(np.array([-0.0, 0.0, 1.0, 2.0]), size=size(200))))
    out.append(("all equal 60", 60, np.full(size(60), 0.75)))
    return out


@pytest.mark.parametrize("case", torch_ref_cases(), ids=lambda c: c[0])
def test_torch_reference_equals_the_numpy_reference(case):
    """ref_nj_torch on the CPU against ref_nj, every bit, masked and compacting."""
    pytest.importorskip("torch")
    from tests.njref import ref_nj_torch
    name, n, d = case
    if name.startswith("signed"):
        assert np.signbit(d).any() and (~np.signbit(d) & (d == 0)).any()
    want = ref_nj(d, n)
    for compact in (False, True):
        got = ref_nj_torch(d, n, compact=compact, device="cpu")
        assert_same_nj(got, want, f"{name} compact={compact}")
        assert got["n_compactions"] == (predicted_compactions(n) if compact else 0) and got["steps"] == n - 3


@pytest.mark.parametrize("compact", [False, True])
def test_torch_reference_prefix(compact):
    """steps=k returns the first k rows of the full result and no root."""
    pytest.importorskip("torch")
    from tests.njref import ref_nj_torch
    n = 65
    d = np.random.default_rng(65).random(n * (n - 1) // 2)
    full = ref_nj_torch(d, n, compact=compact)
    for k in (0, 1, 31, 40, n - 3):  # 33 live rows after step 31: across the first compaction
        head = ref_nj_torch(d, n, compact=compact, steps=k)
        assert head["steps"] == k and head["join"].shape == (k, 2) and head["length"].shape == (k, 2)
        assert np.array_equal(head["join"], full["join"][:k])
        assert np.array_equal(bits(head["length"]), bits(full["length"][:k]))
        if k < n - 3:
            assert head["root"] is None and head["root_length"] is None
        else:
            assert_same_nj(head, full, "the whole loop")


# ------------------------------------------------------------- known answers

FIVE =[5, 9, 9, 8, 10, 10, 9, 8, 7, 3]  # the textbook five taxa a .. e
FIVE_TREE = {"join": [[-1, -2], [1, -3]], "length": [[2.0, 3.0], [3.0, 4.0]], "root": [2, -4, -5],
             "root_length": [2.0, 2.0, 1.0]}


def assert_tree_is(tree, want):
    for key in ("join", "length", "root", "root_length"):
        assert np.asarray(tree[key]).tolist() == want[key], (key, tree[key])


def test_textbook_five_taxa():
    """After (a, b) the pairs (u, c) and (d, e) tie at q = -28: the lower pair wins."""
    assert_tree_is(ref_nj(FIVE, 5), FIVE_TREE)


def test_three_taxa():
    t = ref_nj([3, 4, 5], 3)
    assert t["join"].shape == (0, 2) and t["length"].shape == (0, 2)
    assert t["root"].tolist() == [-1, -2, -3] and t["root_length"].tolist() == [1.0, 2.0, 3.0]


ALL_EQUAL6 = {"join": [[-1, -2], [1, -3], [2, -4]], "length": [[.375, .375], [0.0, .375], [0.0, .375]],
              "root": [3, -5, -6], "root_length": [0.0, .375, .375]}


def test_all_equal():
    assert_tree_is(ref_nj(np.full(15, 0.75), 6), ALL_EQUAL6)


def signed_zero_case():
    """n = 6, every distance a zero: q is -0.0 where D is -0.0 and +0.0 where D
    is +0.0.  D(0, 1) = +0.0 against -0.0 everywhere else: -0.0 < +0.0 is false,
    so the lowest pair wins all the same."""
    d = np.full(15, -0.0)
    d[0] = 0.0
    return d


def test_signed_zeros():
    d = signed_zero_case()
    assert np.signbit(d[1:]).all() and not np.signbit(d[0])
    t, plain = ref_nj(d, 6), ref_nj(np.zeros(15), 6)
    assert t["join"].tolist() == plain["join"].tolist() == ALL_EQUAL6["join"]
    assert t["root"].tolist() == plain["root"].tolist()
    assert not t["length"].any() and not t["root_length"].any()


# ------------------------------------------------------- the host edge table

def _edges(join, length, root, root_length, n, nulls=()):
    from kmer_spans_amd import _lib
    L = _lib.load()
    join = np.ascontiguousarray(join, dtype=np.int32).reshape(-1, 2)
    length = np.ascontiguousarray(length, dtype=np.float64).reshape(-1, 2)
    root = np.ascontiguousarray(root, dtype=np.int32)
    root_length = np.ascontiguousarray(root_length, dtype=np.float64)
    edge = np.full((max(2 * n - 3, 1), 2), -7, dtype=np.int32)
    el = np.full(max(2 * n - 3, 1), -7.0)
    arrs = {"join": join, "length": length, "root": root, "root_length": root_length, "edge": edge, "edge_length": el}
    ptr = {k: (None if k in nulls or v.size == 0 else v.ctypes.data) for k, v in arrs.items()}
    rc = L.ks_nj_edges(ptr["join"], ptr["length"], ptr["root"], ptr["root_length"], n, ptr["edge"], ptr["edge_length"])
    return rc, L.ks_last_error().decode(), edge, el


def walk_edges(tree, n: int):
    """Preorder from the trifurcation, children in stored order, with a stack."""
    ident = lambda c: -c if c < 0 else 2 * n - 2 - (c - 1)  # noqa: E731
    edge, el = [], []
    stack = [(int(tree["root"][c]), n + 1, float(tree["root_length"][c])) for c in (2, 1, 0)]
    while stack:
        code, par, ln = stack.pop()
        edge.append((par, ident(code)))
        el.append(ln)
        if code > 0:
            for c in (1, 0):
                stack.append((int(tree["join"][code - 1, c]), ident(code), float(tree["length"][code - 1, c])))
    return np.array(edge, dtype=np.int32), np.array(el)


def caterpillar(n: int):
    join = np.array([[-1, -2]] + [[t, -(t + 2)] for t in range(1, n - 3)], dtype=np.int32)
    length = np.arange(2 * (n - 3), dtype=np.float64).reshape(-1, 2) / 8.0
    return {"join": join, "length": length, "root": np.array([n - 3, -(n - 1), -n], dtype=np.int32),
            "root_length": np.array([0.5, 0.25, 0.125])}


@pytest.mark.parametrize("n", [3, 4, 5, 60, 5000])
def test_edges_against_a_python_walk(n):
    import kmer_spans_amd as K
    if n == 5000:
        tree = caterpillar(n)  # n - 3 nodes deep: no recursion survives it
    elif n == 3:
        tree = ref_nj([3, 4, 5], 3)
    else:
        tree = ref_nj(np.random.default_rng(n).random(n * (n - 1) // 2) + 0.5, n)
    got = K.nj_edges(tree)
    edge, el = walk_edges(tree, n)
    assert got["Nnode"] == n - 2 and got["n_tip"] == n and got["edge"].shape == (2 * n - 3, 2)
    assert np.array_equal(got["edge"], edge) and np.array_equal(bits(got["edge_length"]), bits(el))
    e = got["edge"]
    assert sorted(e[:, 1].tolist()) == [v for v in range(1, 2 * n - 1) if v != n + 1]  # every node but the root, once
    assert e[0, 0] == n + 1 and (e[:, 0] > n).all() and (e[:, 0] <= 2 * n - 2).all()
    seen = {n + 1}
    for p, c in e.tolist():  # preorder: a parent comes before its children
        assert p in seen
        seen.add(c)
    # the step numbering: the children of step t hang under 2n - 2 - t
    for t in range(min(n - 3, 50)):
        kids = e[e[:, 0] == 2 * n - 2 - t, 1].tolist()
        assert kids == [(-c if c < 0 else 2 * n - 2 - (c - 1)) for c in tree["join"][t].tolist()]


def test_five_taxa_edges():
    import kmer_spans_amd as K
    got = K.nj_edges(FIVE_TREE)
    assert got["edge"].tolist() == [[6, 7], [7, 8], [8, 1], [8, 2], [7, 3], [6, 4], [6, 5]]
    assert got["edge_length"].tolist() == [2.0, 3.0, 2.0, 3.0, 4.0, 2.0, 1.0]


def test_edges_reject_malformed_tables():
    import kmer_spans_amd as K
    t = ref_nj(np.random.default_rng(9).random(45) + 0.5, 10)
    j, ln, r, rl = t["join"], t["length"], t["root"], t["root_length"]
    assert _edges(j, ln, r, rl, 10)[0] == 0

    def bad_join(row, col, value, needle):
        b = j.copy()
        b[row, col] = value
        rc, msg, edge, el = _edges(b, ln, r, rl, 10)
        assert rc != 0 and needle in msg, (row, col, value, msg)
        return msg
    bad_join(3, 1, 0, "neither an observation nor an earlier step")
    bad_join(3, 1, -11, "neither an observation nor an earlier step")
    bad_join(3, 0, 4, "neither an observation nor an earlier step")  # its own step
    bad_join(3, 0, 7, "neither an observation nor an earlier step")  # a later one
    assert "join[3][1]" in bad_join(3, 1, 8, "neither")
    other = int(j[0, 0])
    assert other != int(j[5, 1])
    bad_join(5, 1, other, "used twice")  # ... which also leaves a node out
    b = r.copy()
    b[2] = 8  # n - 3 = 7 steps: no step 8
    rc, msg, _, _ = _edges(j, ln, b, rl, 10)
    assert rc != 0 and "root[0][2]" in msg
    b[2] = r[0]
    rc, msg, _, _ = _edges(j, ln, b, rl, 10)
    assert rc != 0 and "used twice" in msg
    for null in ("join", "length", "root", "root_length", "edge", "edge_length"):
        rc, msg, _, _ = _edges(j, ln, r, rl, 10, nulls=(null,))
        assert rc != 0 and "null" in msg
    for n in (2, 0, -1):
        rc, msg, _, _ = _edges(j, ln, r, rl, n)
        assert rc != 0 and "at least 3 observations" in msg
    with pytest.raises(K.KmerSpansError, match="used twice"):
        K.nj_edges({"join": [[-1, -2]], "length": [[1.0, 1.0]], "root": [1, -3, -3], "root_length": [1.0, 1.0, 1.0]})
    with pytest.raises(K.KmerSpansError, match="a tree holds"):
        K.nj_edges({"join": [[-1, -2]], "length": [[1.0, 1.0]], "root": [1, -3], "root_length": [1.0, 1.0]})


# --------------------------------------------------------------------- newick

def parse_newick(text: str):
    """{(leaf a, leaf b): path length} of a Newick string, a < b, without
    recursion: a parent and a length per node, then every leaf's way up."""
    assert text.endswith(";")
    parent, plen, label = [-1], [0.0], [None]  # node 0: the outermost group
    cur, stack, at, body = 0, [], 0, text[:-1]

    def child_of(u):
        parent.append(u), plen.append(0.0), label.append(None)
        return len(parent) - 1
    while at < len(body):
        ch = body[at]
        if ch == "(":  # cur becomes a group: its first member is next
            stack.append(cur)
            cur = child_of(cur)
            at += 1
        elif ch == ",":
            cur = child_of(stack[-1])
            at += 1
        elif ch == ")":  # what follows names the group itself
            cur = stack.pop()
            at += 1
        else:
            end = at
            while end < len(body) and body[end] not in "(),":
                end += 1
            name, _, ln = body[at:end].partition(":")
            if name:
                label[cur] = name
            if ln:
                plen[cur] = float(ln)
            at = end
    assert not stack and cur == 0
    up = {}
    for v, name in enumerate(label):
        if name is not None:
            way, total, u = {}, 0.0, v
            while u != -1:
                way[u] = total  # in order: the first shared node is the lowest common ancestor
                total, u = total + plen[u], parent[u]
            up[name] = way
    out = {}
    for a in up:
        for b in up:
            if a < b:
                meet = next(u for u in up[a] if u in up[b])
                out[a, b] = up[a][meet] + up[b][meet]
    return out


def test_newick_round_trip():
    import kmer_spans_amd as K
    assert K.nj_newick(FIVE_TREE) == "(((1:2.0,2:3.0):3.0,3:4.0):2.0,4:2.0,5:1.0);"
    assert K.nj_newick(ref_nj([3, 4, 5], 3), labels=["a", "b", "c"]) == "(a:1.0,b:2.0,c:3.0);"
    n = 24
    rng = np.random.default_rng(24)
    labels = [f"r{i}" for i in range(n)]
    # an additive tree with dyadic lengths: every path sum is exact in any order
    d = random_additive(rng, n)
    tree = ref_nj(d, n)
    back = parse_newick(K.nj_newick(tree, labels))
    i, j = np.triu_indices(n, 1)
    for x, y, w in zip(i.tolist(), j.tolist(), d.tolist()):
        assert back[tuple(sorted((labels[x], labels[y])))] == w, (x, y)
    # lengths with all 53 bits in use: each is written as the text that reads back as the same double
    tree = ref_nj(rng.random(n * (n - 1) // 2) + 0.1, n)
    text = K.nj_newick(tree, labels)
    written = sorted(float(tok.split(":")[1]) for tok in text.replace("(", ",").replace(")", ",").split(",")
                     if ":" in tok)
    have = sorted(tree["length"].ravel().tolist() + tree["root_length"].tolist())
    assert np.array_equal(bits(written), bits(have))
    assert len(K.nj_newick(caterpillar(5000))) > 5000 * 8  # deep: the walk is a loop
    with pytest.raises(K.KmerSpansError, match="labels are needed"):
        K.nj_newick(FIVE_TREE, labels=["a"])
    with pytest.raises(K.KmerSpansError, match="Newick punctuation"):
        K.nj_newick(FIVE_TREE, labels=["a", "b", "c(", "d", "e"])


# ------------------------------------------------------------ argument checks

def _nj(n, flags=0, dev=False, d=None, diss=True, outs=(True, True, True, True)):
    """A call that must be refused before any device use: this machine has no GPU."""
    from kmer_spans_amd import _lib
    L = _lib.load()
    d = np.ones(max(1, abs(n) * (abs(n) - 1) // 2)) if d is None else np.ascontiguousarray(d, dtype=np.float64)
    arrs = _lib.nj_outputs(max(abs(n), 4))
    ptr = [x.ctypes.data if keep else None for x, keep in zip(arrs, outs)]
    dp = d.ctypes.data if diss else None
    if dev:  # the pointer is never followed: the arguments fail first
        rc = L.ks_nj_dev(None, dp, n, flags, ptr[0], ptr[1], ptr[2], ptr[3], None)
    else:
        rc = L.ks_nj(None, dp, n, ptr[0], ptr[1], ptr[2], ptr[3])
    return rc, L.ks_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_entries_validate_before_any_device_call(dev):
    for n in (2, 1, 0, -3):
        rc, msg = _nj(n, dev=dev)
        assert rc != 0 and "at least 3 observations" in msg
    assert _nj(5, dev=dev, diss=False)[0] != 0
    for k in range(4):
        rc, msg = _nj(5, dev=dev, outs=tuple(x != k for x in range(4)))
        assert rc != 0 and "null output" in msg
    if dev:
        for flags in (4, 8, 5, -1):
            rc, msg = _nj(5, flags=flags, dev=True)
            assert rc != 0 and "unknown nj flags" in msg


@pytest.mark.parametrize("badval", [np.nan, np.inf, -np.inf])
def test_host_entry_rejects_non_finite(badval):
    """ks_nj checks every entry on the host before any device call."""
    import kmer_spans_amd as K
    d = np.ones(10)
    d[[4, 7]] = badval
    rc, msg = _nj(5, d=d)
    assert rc != 0 and msg == "dissimilarity at offset 4 is not finite"
    with pytest.raises(K.KmerSpansError, match="^dissimilarity at offset 4 is not finite$"):
        K.region_nj(d)


def test_python_argument_checks():
    import kmer_spans_amd as K
    from kmer_spans_amd import _lib
    for size in (0, 1, 2, 4, 5, 7):
        with pytest.raises(K.KmerSpansError, match="n\\(n-1\\)/2"):
            K.region_nj(np.ones(size))
    with pytest.raises(K.KmerSpansError, match="1-d"):
        K.region_nj(np.ones((3, 1)))
    assert [_lib.nj_n(m * (m - 1) // 2) for m in (3, 4, 1000, 24611, 66000)] == [3, 4, 1000, 24611, 66000]
    assert {"region_nj", "nj_edges", "nj_newick"} <= set(K.__all__)
