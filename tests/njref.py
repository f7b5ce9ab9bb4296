"""A second transcription of the neighbour-joining contract of
include/kmer_spans.h (ks_nj_dev), in torch, for sizes the numpy loop of
tests/test_nj.py (ref_nj, O(n^3) on the host) cannot reach.  It runs on any
torch device: on "cpu" the tests tie it to ref_nj bit for bit, on "cuda" it is
a chain of plain elementwise and reduction kernels of torch that share nothing
with ks_nj.hip.

Every FP64 operation of the contract is one torch call of its own, in the
contract's order: no alpha=, no addcmul / addcdiv, no torch.compile, nothing
that may fuse a multiplication into an addition.  torch.sub(x, y) is x + (-1) y
inside torch, which rounds as x - y whether or not it is fused.  A divisor is
always a tensor on the device: with a Python number torch multiplies by the
rounded reciprocal instead.  Multiplications by 0.5 and by an integer count take
a Python number, which is the same FP64 product.

With steps=k the loop ends after k joins and only join[:k] and length[:k] come
back: row s of the device's output depends on the steps before it alone, so a
prefix is a complete check of those steps."""
import numpy as np
import torch

MIN_DIM = 8  # no compaction to fewer rows (ks_nj_dev's description in the header)


def _upper(m: int, device) -> torch.Tensor:
    """True at (i, j), i < j."""
    idx = torch.arange(m, device=device)
    return idx[:, None] < idx[None, :]


def ref_nj_torch(d, n: int, compact: bool = False, steps=None, device="cpu"):
    """The header's algorithm, step for step (compare ref_nj of test_nj.py).

    d: the condensed vector, a numpy array or a tensor, every entry finite.
    compact=True drops dead rows at the device's threshold, compact=False masks
    them.  Returns a dict of numpy arrays join int32 [k, 2], length float64
    [k, 2] with k = n - 3 or steps, n_compactions, steps, and, when the loop ran
    to the end, root int32 [3] and root_length float64 [3] (None otherwise)."""
    dev = torch.device(device)
    d = torch.as_tensor(d, dtype=torch.float64).to(dev)
    assert d.shape == (n * (n - 1) // 2,) and n >= 3 and bool(torch.isfinite(d).all())
    total = n - 3
    k_steps = total if steps is None else int(steps)
    assert 0 <= k_steps <= total
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)

    # the full symmetric matrix, +0.0 on the diagonal
    M = torch.zeros((n, n), dtype=torch.float64, device=dev)
    iu = torch.triu_indices(n, n, 1, device=dev)
    M[iu[0], iu[1]] = d
    M[iu[1], iu[0]] = d
    del iu
    # row sums: n column additions into one accumulator from +0.0 (row j is column j)
    S = torch.zeros(n, dtype=torch.float64, device=dev)
    for j in range(n):
        S = torch.add(S, M[j])
    live = torch.ones(n, dtype=torch.bool, device=dev)
    pairs = _upper(n, dev)  # live pairs of the upper triangle
    node = [-(i + 1) for i in range(n)]
    join = np.zeros((k_steps, 2), dtype=np.int32)
    length = torch.zeros((k_steps, 2), dtype=torch.float64, device=dev)
    r, compactions = n, 0
    for s in range(k_steps):
        m = M.shape[0]
        rm2 = torch.full((), float(r - 2), dtype=torch.float64, device=dev)
        q = torch.mul(M, rm2)
        q = torch.sub(q, S[:, None])
        q = torch.sub(q, S[None, :])
        ok = torch.logical_and(pairs, torch.lt(q, inf))  # a NaN q is no candidate
        q = torch.where(ok, q, inf)
        qmin = q.min()
        if not bool(torch.lt(qmin, inf)):
            raise ArithmeticError("no pair has q < +inf")
        # the lowest flat index among the minima: -0.0 == +0.0, the pair decides
        at = int(torch.where(torch.eq(q, qmin).reshape(-1))[0].min())
        del q, ok
        a, b = divmod(at, m)
        dab = M[a, b].clone()
        sa, sb = S[a].clone(), S[b].clone()
        delta = torch.div(torch.sub(sa, sb), rm2)
        join[s] = node[a], node[b]
        length[s, 0] = torch.mul(torch.add(dab, delta), 0.5)
        length[s, 1] = torch.mul(torch.sub(dab, delta), 0.5)
        k = live.clone()
        k[a] = False
        k[b] = False
        x, y = M[a].clone(), M[b].clone()
        dn = torch.mul(torch.sub(torch.add(x, y), dab), 0.5)
        S_new = torch.add(torch.sub(torch.sub(S, x), y), dn)
        S = torch.where(k, S_new, S)
        row = torch.where(k, dn, x)
        M[a, :] = row
        M[:, a] = row
        S[a] = torch.mul(torch.sub(torch.add(sa, sb), torch.mul(dab, float(r))), 0.5)
        live[b] = False
        pairs[b, :] = False
        pairs[:, b] = False
        node[a] = s + 1
        r -= 1
        if compact and 2 * r <= m and r >= MIN_DIM:
            keep = torch.nonzero(live).reshape(-1)
            M = M.index_select(0, keep).index_select(1, keep).contiguous()
            S = S.index_select(0, keep)
            node = [node[i] for i in keep.tolist()]
            live = torch.ones(r, dtype=torch.bool, device=dev)
            pairs = _upper(r, dev)
            compactions += 1
    out = {"join": join, "length": length.cpu().numpy(), "root": None, "root_length": None,
           "n_compactions": compactions, "steps": k_steps}
    if k_steps == total:
        x, y, z = (int(v) for v in torch.nonzero(live).reshape(-1).tolist())
        dxy, dxz, dyz = M[x, y], M[x, z], M[y, z]
        out["root"] = np.array([node[x], node[y], node[z]], dtype=np.int32)
        out["root_length"] = torch.stack([torch.mul(torch.sub(torch.add(dxy, dxz), dyz), 0.5),
                                          torch.mul(torch.sub(torch.add(dxy, dyz), dxz), 0.5),
                                          torch.mul(torch.sub(torch.add(dxz, dyz), dxy), 0.5)]).cpu().numpy()
    return out
