"""Exact integer model of the frontier reindex and of the multi-hop chain
that feeds it, in numpy / int64 with no GPU, shared by
test_frontier_model_cpu.py, test_gpu_reindex_exact.py and
test_gpu_fused_hops_exact.py.

Everything here is deterministic given its inputs, so every comparison the
tests make against it is exact equality or set membership.  The graphs and
the reindex inputs the tests use are built here too, once, so the CPU file
validates the model on small versions of exactly what the GPU files run.
"""
from collections import namedtuple

import numpy as np
import torch

# One hop as the sampler lays it out: edge_index = [src_local, dst_local],
# dst_ptr has n_dst + 1 entries, e_id is aligned with the edge columns.
Hop = namedtuple("Hop", "frontier edge_index dst_ptr e_id")
# hops[0] is the seeds' hop (the sampler's adjs[-1]); sizes is laid out as
# sizes_dev: [m_0, u_0, m_1, u_1, ...].
Hops = namedtuple("Hops", "hops sizes")


def _np(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.int64))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int64))


def _dedup(items):
    """(frontier, uniq, rank): `frontier` is `items` deduplicated in
    first-occurrence order; uniq[i] sits at frontier[rank[i]]."""
    uniq, first = np.unique(items, return_index=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(uniq.size, dtype=np.int64)
    rank[order] = np.arange(uniq.size, dtype=np.int64)
    return uniq[order], uniq, rank


def _reindex_np(seeds, nbrs, counts):
    assert counts.size == seeds.size and int(counts.sum()) == nbrs.size
    frontier, uniq, rank = _dedup(np.concatenate([seeds, nbrs]))
    col = rank[np.searchsorted(uniq, nbrs)]
    row = np.repeat(np.arange(seeds.size, dtype=np.int64), counts)
    return frontier, row, col


def reindex_model(seeds, nbrs, counts):
    """(frontier, row, col) as int64 CPU tensors: frontier is
    concat(seeds, nbrs) deduplicated in first-occurrence order, col[j] the
    position of nbrs[j] in it, row the seed POSITION each neighbour belongs
    to (repeat_interleave(arange(len(seeds)), counts))."""
    return tuple(_t(x) for x in
                 _reindex_np(_np(seeds), _np(nbrs), _np(counts)))


def _row_slots(indptr, nodes, counts):
    """CSR slots of the first counts[i] entries of every nodes[i]'s row,
    concatenated, and the exclusive scan of counts (n + 1 entries)."""
    ptr = np.zeros(nodes.size + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    m = int(ptr[-1])
    slots = (np.repeat(indptr[nodes] - ptr[:-1], counts)
             + np.arange(m, dtype=np.int64))
    return slots, ptr


def hops_model(indptr, indices, seeds, fanouts, eid=None):
    """The whole batch for a graph on which every row a hop reads is no
    longer than that hop's fanout: the draw then copies the row in CSR
    order, so frontier, edges, pointer and edge ids are all determined.
    Raises ValueError where a longer row is reached."""
    indptr, indices, prev = _np(indptr), _np(indices), _np(seeds)
    eid = None if eid is None else _np(eid)
    hops, sizes = [], []
    for k in fanouts:
        deg = indptr[prev + 1] - indptr[prev]
        if deg.size and int(deg.max()) > k:
            raise ValueError(f"a row of degree {int(deg.max())} is read "
                             f"with fanout {k}: the draw is random")
        slots, ptr = _row_slots(indptr, prev, deg)
        frontier, row, col = _reindex_np(prev, indices[slots], deg)
        e_id = slots if eid is None else eid[slots]
        hops.append(Hop(_t(frontier), _t(np.stack([col, row])), _t(ptr),
                        _t(e_id)))
        sizes += [slots.size, frontier.size]
        prev = frontier
    return Hops(hops, torch.tensor(sizes, dtype=torch.int64))


def check_hop_structure(prev_frontier, frontier, edge_index, dst_ptr,
                        indptr, indices, k):
    """Everything about one hop that does not depend on which neighbours a
    row longer than k drew: the dst ids and the pointer exactly, every
    source a member of its dst's CSR row, short rows whole and in CSR
    order, and the frontier (hence every local id) exactly the
    first-occurrence dedup of concat(prev_frontier, drawn neighbours).
    dst_ptr may be None for an engine that emits none (the CPU one)."""
    prev, frontier = _np(prev_frontier), _np(frontier)
    ei = _np(edge_index)
    indptr, indices = _np(indptr), _np(indices)
    assert ei.ndim == 2 and ei.shape[0] == 2
    src, dst = ei[0], ei[1]
    m = src.size
    deg = indptr[prev + 1] - indptr[prev]
    cnt = np.minimum(deg, k)
    ptr = np.zeros(prev.size + 1, dtype=np.int64)
    np.cumsum(cnt, out=ptr[1:])
    assert m == int(ptr[-1])
    assert np.array_equal(
        dst, np.repeat(np.arange(prev.size, dtype=np.int64), cnt))
    if dst_ptr is not None:
        dst_ptr = _np(dst_ptr)
        assert np.array_equal(dst_ptr, ptr)
        assert int(dst_ptr[-1]) == m
    if m:
        assert int(src.min()) >= 0 and int(src.max()) < frontier.size
    out = frontier[src]
    # membership: (row node, neighbour) must be an edge of the CSR
    n_nodes = indptr.size - 1
    owner = np.repeat(np.arange(n_nodes, dtype=np.int64), np.diff(indptr))
    assert np.isin(prev[dst] * n_nodes + out, owner * n_nodes + indices).all()
    # rows no longer than k: whole, in CSR order
    whole = deg[dst] <= k
    slot = indptr[prev[dst]] + (np.arange(m, dtype=np.int64) - ptr[dst])
    assert np.array_equal(out[whole], indices[slot[whole]])
    want, _, _ = _dedup(np.concatenate([prev, out]))
    assert np.array_equal(frontier, want)


# ---- graphs ---------------------------------------------------------------

DET_PATTERN = np.array([0, 1, 2, 3, 0, 3, 2, 1], dtype=np.int64)
HUB_EVERY, HUB_DEGREE = 10, 60


def det_graph(n=6000, seed=11):
    """(indptr, indices) int64 tensors: degrees cycle through DET_PATTERN
    (at most 3), targets random, so many targets repeat.  With every fanout
    >= 3 a batch on it is fully determined."""
    rng = np.random.default_rng(seed)
    degs = DET_PATTERN[np.arange(n) % DET_PATTERN.size]
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(degs, out=indptr[1:])
    indices = rng.integers(0, n, int(indptr[-1]), dtype=np.int64)
    return _t(indptr), _t(indices)


def mixed_graph(n=6000, seed=11):
    """det_graph, except every 10th node has 60 random out-edges: rows far
    above any fanout next to the short ones.  For check_hop_structure."""
    d_indptr, d_indices = (_np(x) for x in det_graph(n, seed))
    rng = np.random.default_rng(seed + 1)
    degs = np.diff(d_indptr)
    hub = np.arange(n) % HUB_EVERY == 0
    new_degs = np.where(hub, HUB_DEGREE, degs)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(new_degs, out=indptr[1:])
    indices = np.empty(int(indptr[-1]), dtype=np.int64)
    hub_slot = np.repeat(hub, new_degs)
    indices[hub_slot] = rng.integers(0, n, int(hub_slot.sum()),
                                     dtype=np.int64)
    indices[~hub_slot] = d_indices[~np.repeat(hub, degs)]
    return _t(indptr), _t(indices)


def shuffled_coo(indptr, indices, seed=5):
    """The graph's edges as a [2, E] COO edge_index in shuffled order."""
    indptr, indices = _np(indptr), _np(indices)
    src = np.repeat(np.arange(indptr.size - 1, dtype=np.int64),
                    np.diff(indptr))
    perm = np.random.default_rng(seed).permutation(src.size)
    return _t(np.stack([src[perm], indices[perm]]))


def nodes_of_degree(indptr, degree):
    indptr = _np(indptr)
    return _t(np.flatnonzero(np.diff(indptr) == degree))


def mixed_seed_batches(indptr, seed=3):
    """The batch shapes of test_gpu_dst_ptr.py on a graph of n nodes:
    random seeds, then a zero-degree seed last, a hub seed last, and a
    single zero-degree seed."""
    n = _np(indptr).size - 1
    g = torch.Generator().manual_seed(seed)
    zero = int(nodes_of_degree(indptr, 0)[0])
    hub = int(nodes_of_degree(indptr, HUB_DEGREE)[1])
    return [
        torch.randint(0, n, (257,), generator=g),
        torch.cat([torch.randint(0, n, (63,), generator=g),
                   torch.tensor([zero])]),
        torch.cat([torch.randint(0, n, (100,), generator=g),
                   torch.tensor([hub])]),
        torch.tensor([zero]),
    ]


# ---- reindex inputs -------------------------------------------------------

def _counts_summing_to(rng, n, m, hi):
    """n counts, the first n - 1 random in 0..hi (cut off once they would
    pass m), the last one whatever brings the sum to m."""
    c = rng.integers(0, hi + 1, n - 1, dtype=np.int64)
    cum = np.minimum(np.concatenate([[0], np.cumsum(c)]), m)
    c = np.diff(cum)
    return np.concatenate([c, [m - int(c.sum())]]).astype(np.int64)


def case_strided(small=False, seed=21):
    """Unique seeds, neighbours drawn with repeats from an id range that
    holds the seeds.  Full size: 40 000 + 560 000 items, more than the 2048
    x 256 a capped grid covers at once, and more rows than the 2048 x 16 of
    expand_rows_kernel, so every kernel takes a second stride iteration."""
    n, m, ids = (400, 5600, 3000) if small else (40000, 560000, 300000)
    rng = np.random.default_rng(seed)
    seeds = rng.permutation(ids)[:n].astype(np.int64)
    nbrs = rng.integers(0, ids, m, dtype=np.int64)
    return _t(seeds), _t(nbrs), _t(_counts_summing_to(rng, n, m, 28))


def case_one_hot(small=False, key_is_seed=False):
    """One seed and m copies of one id: every insert but one contends for
    one slot."""
    m = 1000 if small else 100000
    seed_id = 7
    key = seed_id if key_is_seed else 12345
    return (torch.tensor([seed_id]), torch.full((m,), key, dtype=torch.int64),
            torch.tensor([m]))


def case_wide_keys(seed=22):
    """Keys i * N + v up to just below 2^62, as sample_temporal builds
    them.  Neighbours repeat, and some differ from a seed key only above
    bit 31 or only in bit 0, so a 32-bit hash, compare or store merges or
    splits keys."""
    b = 1000
    big_n = (1 << 62) // b
    rng = np.random.default_rng(seed)
    tree = np.arange(b, dtype=np.int64)
    seeds = tree * big_n + rng.integers(0, big_n - (1 << 35), b,
                                        dtype=np.int64)
    assert int(seeds.max()) < (1 << 62) and int(seeds.max()) >= (1 << 61)
    per = 8
    base = np.repeat(seeds, per)
    shift = np.tile(np.array([0, 1 << 32, 1 << 33, 3 << 32, 1, 1 << 31,
                              (1 << 32) + 1, 0], dtype=np.int64), b)
    nbrs = base + shift
    assert int(nbrs.max()) < (1 << 62)
    return _t(seeds), _t(nbrs), torch.full((b,), per, dtype=torch.int64)


def case_duplicate_seeds(seed=23):
    """64 seeds from 20 ids, 500 neighbours from 40 ids that hold them."""
    rng = np.random.default_rng(seed)
    seeds = rng.integers(100, 120, 64, dtype=np.int64)
    nbrs = rng.integers(100, 140, 500, dtype=np.int64)
    return _t(seeds), _t(nbrs), _t(_counts_summing_to(rng, 64, 500, 14))


def case_zero_rows(n):
    """n seeds without a single neighbour (n may be 0)."""
    return (torch.arange(n, dtype=torch.int64) * 3 + 5,
            torch.zeros(0, dtype=torch.int64),
            torch.zeros(n, dtype=torch.int64))


def cases_around_pow2(power=4096, seed=24):
    """All-unique items with 2 * (n + m) + 64 two below, equal to and two
    above a power of two (the sum is even): the table capacity is that
    power, at its fullest, then twice it."""
    rng = np.random.default_rng(seed)
    out = []
    for delta in (-1, 0, 1):
        total = (power - 64) // 2 + delta
        n = 100
        keys = rng.permutation(1 << 20)[:total].astype(np.int64)
        out.append((_t(keys[:n]), _t(keys[n:]),
                    _t(_counts_summing_to(rng, n, total - n, 40))))
    return out
