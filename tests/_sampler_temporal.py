"""Shared by test_cpu_sampler_temporal.py and test_gpu_sampler_temporal.py:
the graphs, a numpy model of "edges of v that exist by a bound", and the
checks of temporal sampling (sample_temporal, temporal sample_links), the
same in every mode.

Graph T has 3000 nodes and is built from a shuffled COO, so the topo has an
`eid` and no row is in time order.  Its hub row holds 5000 edges; with 2999
other nodes their targets cannot all be distinct, so every other node is a
target once or twice.  Nothing below needs distinct targets: edges are told
apart by their ids.
"""
import numpy as np
import torch

import quiver

I64_MIN = -2 ** 63
I64_MAX = 2 ** 63 - 1
SEED = 2025

N_T = 3000
# special rows of graph T, by node id
R_DEG0, R_DEG1, R_DEG5, R_DEG6, R_DEG10, R_DEG11, R_DEG40 = range(7)
R_SAME = 7          # 12 edges that share the time 500
R_TIES = 8          # times [1, 1, 1, 2, 2, 3]
R_HUB = 9           # 5000 edges, times a shuffle of 0..4999
HUB_DEG = 5000
STEP = 10           # rows 1..6: times are a shuffle of 0, 10, 20, ...
SPECIAL_DEG = {R_DEG0: 0, R_DEG1: 1, R_DEG5: 5, R_DEG6: 6, R_DEG10: 10,
               R_DEG11: 11, R_DEG40: 40}

CHI2_DF = 39
CHI2_BOUND = CHI2_DF + 5 * np.sqrt(2 * CHI2_DF)         # 83.2


class Model:
    """Edges by id: src, dst, time.  `eligible` lists the ids of a row's
    edges with time <= bound in the order a whole row is returned in:
    ascending time, ties in CSR order (= ascending id, for COO positions
    under a stable CSR build and for CSR slots alike)."""

    def __init__(self, src, dst, time, nodes):
        self.src, self.dst, self.time = src, dst, time
        self.nodes = nodes
        self.order = np.lexsort((np.arange(len(src)), time, src))
        self.indptr = np.zeros(nodes + 1, dtype=np.int64)
        self.indptr[1:] = np.cumsum(np.bincount(src, minlength=nodes))
        self._memo = {}

    def eligible(self, v, bound):
        got = self._memo.get((v, bound))
        if got is None:
            ids = self.order[self.indptr[v]:self.indptr[v + 1]]
            got = ids[self.time[ids] <= bound]
            self._memo[(v, bound)] = got
        return got


def _targets(rng, v, nodes, count):
    pick = rng.permutation(nodes - 1)[:count]
    return pick + (pick >= v)


def graph_t():
    """(coo [2, E], edge_time [E], topo, model)."""
    rng = np.random.default_rng(11)
    src, dst, time = [], [], []
    for v in range(N_T):
        if v in SPECIAL_DEG:
            d = SPECIAL_DEG[v]
            t = rng.permutation(d) * STEP
        elif v == R_SAME:
            d, t = 12, np.full(12, 500)
        elif v == R_TIES:
            d, t = 6, rng.permutation(np.array([1, 1, 1, 2, 2, 3]))
        elif v == R_HUB:
            d, t = HUB_DEG, rng.permutation(HUB_DEG)
        else:
            d = int(rng.integers(3, 9))
            t = rng.integers(0, 1000, d)
        if v == R_HUB:
            others = np.array([x for x in range(N_T) if x != v])
            to = np.concatenate([rng.permutation(others),
                                 rng.permutation(others)])[:d]
        else:
            to = _targets(rng, v, N_T, d)
        src.append(np.full(d, v))
        dst.append(to)
        time.append(t)
    src, dst, time = (np.concatenate(x).astype(np.int64)
                      for x in (src, dst, time))
    shuffle = rng.permutation(len(src))
    src, dst, time = src[shuffle], dst[shuffle], time[shuffle]
    coo = torch.from_numpy(np.stack([src, dst]))
    topo = quiver.CSRTopo(coo, node_count=N_T)
    return coo, torch.from_numpy(time), topo, Model(src, dst, time, N_T)


N_T0 = 50


def graph_t0():
    """(edge_time [E], topo, model): given as indptr / indices, no eid,
    every row already in time order (with ties)."""
    rng = np.random.default_rng(12)
    deg = rng.integers(0, 10, N_T0)
    deg[:3] = [0, 1, 9]
    indptr = np.zeros(N_T0 + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(deg)
    src = np.repeat(np.arange(N_T0), deg)
    dst = rng.integers(0, N_T0, len(src))
    time = np.concatenate([np.sort(rng.integers(0, 6, d)) for d in deg])
    time = time.astype(np.int64)
    topo = quiver.CSRTopo(indptr=torch.from_numpy(indptr),
                          indices=torch.from_numpy(dst))
    return torch.from_numpy(time), topo, Model(src, dst, time, N_T0)


def make_sampler(topo, mode, sizes, edge_time, seed=SEED, return_eid=True):
    s = quiver.GraphSageSampler(topo, list(sizes), device=0, mode=mode,
                                return_eid=return_eid, edge_time=edge_time)
    s.lazy_init_quiver()
    if mode != "CPU":               # the CPU engine has no seed to set
        s.quiver.set_seed(seed)
    return s


def sample(sampler, seeds, bounds):
    """sample_temporal with the result's types and devices checked."""
    tb = sampler.sample_temporal(torch.as_tensor(seeds, dtype=torch.long),
                                 torch.as_tensor(bounds, dtype=torch.long))
    assert isinstance(tb, quiver.TemporalBatch)
    want = "cpu" if sampler.mode == "CPU" else "cuda"
    assert tb.n_id.device.type == want and tb.batch.device.type == want
    assert tb.n_id.dtype == torch.int64 and tb.batch.dtype == torch.int64
    assert tb.batch.shape == tb.n_id.shape
    for adj in tb.adjs:
        assert adj.edge_index.device.type == want
        assert adj.e_id.device.type == want
    return tb


def hops(tb, sizes):
    """(edge_index, e_id, n_src, n_dst, fanout) as numpy, seeds' hop
    first."""
    out = []
    for adj, k in zip(tb.adjs[::-1], sizes):
        out.append((adj.edge_index.cpu().numpy(), adj.e_id.cpu().numpy(),
                    int(adj.size[0]), int(adj.size[1]), k))
    return out


def check_structure(model, seeds, bounds, tb, sizes):
    """Check 1 of the issue."""
    seeds = np.asarray(seeds, dtype=np.int64)
    bounds = np.asarray(bounds, dtype=np.int64)
    b = len(seeds)
    n_id, batch = tb.n_id.cpu().numpy(), tb.batch.cpu().numpy()
    assert tb.batch_size == b
    assert np.array_equal(n_id[:b], seeds)
    assert np.array_equal(batch[:b], np.arange(b))
    assert n_id.min(initial=0) >= 0 and n_id.max(initial=0) < model.nodes
    assert len(np.unique(batch * model.nodes + n_id)) == len(n_id)
    assert len(tb.adjs) == len(sizes)
    n_prev = b
    for ei, e_id, n_src, n_dst, _ in hops(tb, sizes):
        assert n_dst == n_prev and n_src >= n_dst
        assert ei.shape == (2, len(e_id)) and e_id.dtype == np.int64
        src, dst = ei
        if len(e_id):
            assert src.min() >= 0 and src.max() < n_src
            assert dst.min() >= 0 and dst.max() < n_dst
        # every entry this hop added is the source of one of its edges
        assert np.array_equal(np.unique(src[src >= n_dst]),
                              np.arange(n_dst, n_src))
        assert np.array_equal(batch[src], batch[dst])
        assert np.array_equal(model.src[e_id], n_id[dst])
        assert np.array_equal(model.dst[e_id], n_id[src])
        assert np.all(model.time[e_id] <= bounds[batch[dst]])
        n_prev = n_src
    assert n_prev == len(n_id)


def check_counts(model, bounds, tb, sizes):
    """Check 2 of the issue: every target of every hop has min(k,
    |eligible|) distinct eligible edges, and exactly the model's list, in
    its order, where all eligible edges fit."""
    bounds = np.asarray(bounds, dtype=np.int64)
    n_id, batch = tb.n_id.cpu().numpy(), tb.batch.cpu().numpy()
    for ei, e_id, _, n_dst, k in hops(tb, sizes):
        dst = ei[1]
        assert np.all(dst[1:] >= dst[:-1])
        ptr = np.zeros(n_dst + 1, dtype=np.int64)
        ptr[1:] = np.cumsum(np.bincount(dst, minlength=n_dst))
        for d in range(n_dst):
            got = e_id[ptr[d]:ptr[d + 1]]
            elig = model.eligible(int(n_id[d]), int(bounds[batch[d]]))
            if k == -1 or len(elig) <= k:
                assert np.array_equal(got, elig), (d, got, elig)
            else:
                assert len(got) == k, (d, len(got), k)
                assert len(np.unique(got)) == k
                assert np.all(np.isin(got, elig))


def run_case(model, sampler, seeds, bounds):
    """One batch through checks 1 and 2; returns the batch."""
    tb = sample(sampler, seeds, bounds)
    check_structure(model, seeds, bounds, tb, sampler.sizes)
    check_counts(model, bounds, tb, sampler.sizes)
    return tb


def structure_seeds():
    """64 seeds: every special row, duplicates, plain rows; mixed bounds."""
    rng = np.random.default_rng(21)
    seeds = list(range(10)) + [R_DEG10, R_DEG10, R_HUB, R_DEG40, R_TIES]
    bounds = [0, 0, 20, 100, 45, 1000, 170, 500, 2, 3000,
              I64_MAX, 10, 100, I64_MIN, 1]
    rest = 64 - len(seeds)
    seeds += rng.integers(10, N_T, rest).tolist()
    bounds += rng.integers(0, 1000, rest).tolist()
    return seeds, bounds


def search_cases():
    """Check 3: (seed, bound) pairs around every edge of the search."""
    cases = []
    for bound in (499, 500, 501, I64_MIN, I64_MAX):
        cases.append((R_SAME, bound))
    for bound in (0, 1, 2, 3, 4, I64_MIN, I64_MAX):
        cases.append((R_TIES, bound))
    # between two values: row R_DEG40 holds the multiples of 10 under 400
    for bound in (-1, 0, 15, 389, 390, 391):
        cases.append((R_DEG40, bound))
    for bound in (-1, 0, 2500, HUB_DEG - 1, HUB_DEG, I64_MIN, I64_MAX):
        cases.append((R_HUB, bound))
    for bound in (0, I64_MIN, I64_MAX):
        cases.append((R_DEG0, bound))
    return [c[0] for c in cases], [c[1] for c in cases]


def branch_cases():
    """Check 4 at k = 5: (seed, bound, eligible) for the copy (m = 5), the
    reservoir (m = 6, 10: k < m <= 2k) and Floyd (m = 11, 40), on whole rows
    and on prefixes of longer ones."""
    return [(R_DEG5, I64_MAX, 5), (R_DEG6, I64_MAX, 6),
            (R_DEG10, I64_MAX, 10), (R_DEG11, I64_MAX, 11),
            (R_DEG40, I64_MAX, 40),
            (R_DEG40, 4 * STEP, 5), (R_DEG40, 5 * STEP, 6),
            (R_DEG40, 9 * STEP, 10), (R_DEG40, 10 * STEP, 11),
            (R_DEG11, 9 * STEP + 5, 10)]


def drawn_ids(tb):
    return tb.adjs[0].e_id.cpu().numpy()


def share_past_2048(model, tb):
    """Share of the drawn hub edges whose position in time order is >= 2048
    (the hub's times are a shuffle of 0..4999: position == time)."""
    return float((model.time[drawn_ids(tb)] >= 2048).mean())


def share_window(p, draws, sds=12):
    """p -/+ `sds` binomial standard deviations of a share over `draws`
    draws.  Draws of one row are without replacement, which only narrows
    the true spread."""
    sd = np.sqrt(p * (1 - p) / draws)
    return p - sds * sd, p + sds * sd


def chi_square_inclusion(model, tb, v, rows, k):
    """Chi-square of how often each edge of row v was drawn in `rows`
    copies at fanout k, against rows * k / m each."""
    ids = model.eligible(v, I64_MAX)
    got = drawn_ids(tb)
    assert len(got) == rows * k and np.all(np.isin(got, ids))
    count = np.array([(got == i).sum() for i in ids])
    expect = rows * k / len(ids)
    return float(((count - expect) ** 2 / expect).sum())


def derive_batch(adjs, batch_size, n):
    """Tree index of every n_id entry from the edges alone: seeds are
    their own roots and every source joins its target's tree."""
    batch = np.full(n, -1, dtype=np.int64)
    batch[:batch_size] = np.arange(batch_size)
    for adj in adjs[::-1]:
        src, dst = adj.edge_index.cpu().numpy()
        batch[src] = batch[dst]
    assert batch.min() >= 0
    return torch.from_numpy(batch)


# ---- the cases, one function per check of the issue ----------------------

def case_structure(mode, g):
    _, time, topo, model = g
    seeds, bounds = structure_seeds()
    assert len(seeds) == 64
    run_case(model, make_sampler(topo, mode, [5, 3], time), seeds, bounds)


def case_search(mode, g):
    _, time, topo, model = g
    seeds, bounds = search_cases()
    tb = run_case(model, make_sampler(topo, mode, [-1], time), seeds, bounds)
    # spot values, independent of the model: all ties in, nothing below
    cnt = np.bincount(tb.adjs[0].edge_index[1].cpu().numpy(),
                      minlength=len(seeds))
    assert cnt[:5].tolist() == [0, 12, 12, 0, 12]
    assert cnt[5:12].tolist() == [0, 3, 5, 6, 6, 0, 6]
    assert cnt[12:18].tolist() == [0, 1, 2, 39, 40, 40]
    assert cnt[18:25].tolist() == [0, 1, 2501, 5000, 5000, 0, 5000]
    assert cnt[25:].tolist() == [0, 0, 0]


def case_branches(mode, g):
    _, time, topo, model = g
    cases = branch_cases()
    for v, bound, m in cases:
        assert len(model.eligible(v, bound)) == m
    seeds = [c[0] for c in cases] * 3
    bounds = [c[1] for c in cases] * 3
    run_case(model, make_sampler(topo, mode, [5], time), seeds, bounds)
    # reservoir at k > 128, over positions past 2048
    s = make_sampler(topo, mode, [130], time)
    for bound in (HUB_DEG - 1, 2999):
        tb = run_case(model, s, [R_HUB] * 8, [bound] * 8)
        assert len(drawn_ids(tb)) == 8 * 130
        assert int(model.time[drawn_ids(tb)].max()) >= 2048


def case_coverage(mode, g):
    _, time, topo, model = g
    s = make_sampler(topo, mode, [5], time)
    for v, bound, m in ((R_DEG40, I64_MAX, 40), (R_DEG10, 7 * STEP, 8)):
        elig = model.eligible(v, bound)
        assert len(elig) == m
        tb = sample(s, [v] * 2000, [bound] * 2000)
        check_structure(model, [v] * 2000, [bound] * 2000, tb, [5])
        got = drawn_ids(tb)
        assert len(got) == 2000 * 5
        # every eligible edge at least once (a miss: under 40 * (35/40) **
        # 2000), and no other edge
        assert set(got.tolist()) == set(elig.tolist())


def case_past_2048(mode, g):
    """Check 6.  4000 copies of the hub at k = 5 and bound 4999: 20 000
    draws, expected share 2952/5000 = 0.590, binomial sd 0.0035, window
    [0.55, 0.63].  At k = 130 and bound 2999: 520 000 draws, expected share
    952/3000 = 0.3173, binomial sd 0.00065; the window is that share -/+ 12
    sd (the first window is -/+ 11.4 of its sd), [0.3096, 0.3251]."""
    _, time, topo, model = g
    rows = 4000
    tb = sample(make_sampler(topo, mode, [5], time), [R_HUB] * rows,
                [HUB_DEG - 1] * rows)
    check_structure(model, [R_HUB] * rows, [HUB_DEG - 1] * rows, tb, [5])
    share = share_past_2048(model, tb)
    print("k=5 share past 2048", share)
    assert len(drawn_ids(tb)) == rows * 5
    assert 0.55 <= share <= 0.63
    tb = sample(make_sampler(topo, mode, [130], time), [R_HUB] * rows,
                [2999] * rows)
    check_structure(model, [R_HUB] * rows, [2999] * rows, tb, [130])
    share = share_past_2048(model, tb)
    lo, hi = share_window(952 / 3000, rows * 130)
    print("k=130 share past 2048", share, "window", lo, hi)
    assert len(drawn_ids(tb)) == rows * 130
    assert lo <= share <= hi


def uniformity_stat(mode, g, seed=SEED):
    """Check 7: 16 000 copies of the m = 40 row at k = 5; the chi-square of
    the 40 inclusion counts against 2000 each, df = 39, bound df + 5
    sqrt(2 df) = 83.2.  Draws without replacement correlate the counts
    negatively, so the bound is conservative.  Ten runs of the CPU engine,
    which has no seed to fix, gave 21.7 to 47.7."""
    _, time, topo, model = g
    rows = 16_000
    s = make_sampler(topo, mode, [5], time, seed=seed)
    tb = sample(s, [R_DEG40] * rows, [I64_MAX] * rows)
    stat = chi_square_inclusion(model, tb, R_DEG40, rows, 5)
    print("chi-square", stat, "bound", CHI2_BOUND)
    return stat


def case_disjoint(mode, g):
    _, time, topo, model = g
    seeds, bounds = [R_DEG10, R_DEG10], [1 * STEP, 8 * STEP]
    tb = run_case(model, make_sampler(topo, mode, [-1], time), seeds, bounds)
    ei = tb.adjs[0].edge_index.cpu().numpy()
    assert np.bincount(ei[1], minlength=2).tolist() == [2, 9]
    # the two neighbours of the first tree are in the second as well:
    # each appears once per tree
    n_id, batch = tb.n_id.cpu().numpy(), tb.batch.cpu().numpy()
    assert len(n_id) == 2 + 2 + 9
    assert set(n_id[batch == 0][1:]) <= set(n_id[batch == 1][1:])


def case_many_rows(mode, g):
    _, time, topo, model = g
    rng = np.random.default_rng(31)
    rows = 40_000
    seeds = rng.integers(0, N_T, rows)
    seeds[seeds == R_HUB] = R_DEG40
    bounds = rng.integers(0, 1000, rows)
    tb = run_case(model, make_sampler(topo, mode, [5], time), seeds, bounds)
    # the rows past the first grid of 32 768 are filled
    dst = tb.adjs[0].edge_index[1].cpu().numpy()
    assert (dst >= 32_768).sum() > 3 * (rows - 32_768) // 2


def case_links(mode, g):
    coo, time, topo, model = g
    p, k = 50, 3
    gen = torch.Generator().manual_seed(5)
    at = torch.randperm(coo.shape[1], generator=gen)[:p]
    pos, t = coo[:, at], time[at]
    s = make_sampler(topo, mode, [4, 3], time)
    b = s.sample_links(pos, num_neg=k, edge_label_time=t)
    assert isinstance(b, quiver.LinkBatch) and len(b) == 6
    want = "cpu" if mode == "CPU" else "cuda"
    for x in (b.n_id, b.edge_label_index, b.edge_label, b.neg_ok):
        assert x.device.type == want
    n_id, eli = b.n_id.cpu(), b.edge_label_index.cpu()
    assert torch.equal(n_id[eli[:, :p]], pos)
    assert tuple(eli.shape) == (2, p * (1 + k))
    assert tuple(b.edge_label.shape) == (p * (1 + k),)
    assert torch.equal(b.edge_label.cpu(),
                       torch.tensor([1.0] * p + [0.0] * (p * k)))
    assert tuple(b.neg_ok.shape) == (p * k,) and b.neg_ok.dtype == torch.bool
    assert b.batch_size == p * (2 + k)
    assert len(n_id[:b.batch_size]) == p * (2 + k)
    # seed positions: head i, tails P + i and 2P + i * K + j
    head = torch.cat([torch.arange(p), torch.arange(p).repeat_interleave(k)])
    tail = torch.cat([p + torch.arange(p), 2 * p + torch.arange(p * k)])
    assert torch.equal(eli, torch.stack([head, tail]))
    assert torch.equal(n_id[eli[0, p:]], pos[0].repeat_interleave(k))
    seeds = n_id[:b.batch_size]
    bounds = torch.cat([t, t, t.repeat_interleave(k)])
    tb = quiver.TemporalBatch(b.n_id, b.batch_size, b.adjs,
                              derive_batch(b.adjs, b.batch_size, len(n_id)))
    check_structure(model, seeds.numpy(), bounds.numpy(), tb, [4, 3])
    check_counts(model, bounds.numpy(), tb, [4, 3])
    return b


def case_t0(mode):
    time, topo, model = graph_t0()
    assert topo.eid is None
    s = make_sampler(topo, mode, [2, -1], time)
    # rows were in time order: the topo's own storage goes to the engine
    assert s.temporal_[0].data_ptr() == topo.indices.data_ptr()
    assert s.temporal_[2] is None
    rng = np.random.default_rng(41)
    seeds = list(range(N_T0)) + [2, 2]
    bounds = rng.integers(-1, 7, len(seeds)).tolist()
    tb = run_case(model, s, seeds, bounds)      # model ids are CSR slots
    for adj in tb.adjs:
        e = adj.e_id.cpu()
        v = tb.n_id.cpu()[adj.edge_index[1].cpu()]
        assert bool((topo.indptr[v] <= e).all())
        assert bool((e < topo.indptr[v + 1]).all())


def case_unsorted_without_eid(mode, g):
    """A topo without eid whose rows are not in time order: ids are CSR
    slots of the topo as given, not of the sampler's sorted copy."""
    _, time, topo, model = g
    plain = quiver.CSRTopo(indptr=topo.indptr, indices=topo.indices)
    t_csr = time[topo.eid]
    slots = Model(np.repeat(np.arange(N_T), topo.degree.numpy()),
                  topo.indices.numpy(), t_csr.numpy(), N_T)
    s = make_sampler(plain, mode, [5, 3], t_csr)
    assert s.temporal_[0].data_ptr() != plain.indices.data_ptr()
    seeds, bounds = structure_seeds()
    run_case(slots, s, seeds, bounds)
    assert torch.equal(plain.indices, topo.indices)     # left as it was


def case_plain_sample_same_graph(mode, g, check_coo_ids):
    """sample() of a sampler with edge_time draws from the same graph and
    reports the same ids."""
    coo, time, topo, _ = g
    s = make_sampler(topo, mode, [4, 3], time)
    seeds = torch.arange(64)
    n_id, bs, adjs = s.sample(seeds)
    assert bs == 64 and torch.equal(n_id[:64].cpu(), seeds)
    check_coo_ids(coo, topo, n_id, adjs, [4, 3])


def case_python_errors(mode, g):
    import pytest
    _, time, topo, _ = g
    mk = lambda **kw: quiver.GraphSageSampler(topo, [3], mode=mode, **kw)
    with pytest.raises(ValueError):
        mk(edge_time=time.float())
    with pytest.raises(ValueError):
        mk(edge_time=time.to(torch.int32))
    with pytest.raises(ValueError):
        mk(edge_time=time[:-1])
    with pytest.raises(ValueError):
        mk(edge_time=time.view(1, -1))
    with pytest.raises(ValueError):
        mk(edge_time=time, edge_weight=torch.ones(len(time)))
    with pytest.raises(ValueError):
        quiver.MixedGraphSageSampler(None, 1, topo, [3], edge_time=time)
    plain = mk()
    with pytest.raises(ValueError):
        plain.sample_temporal(torch.arange(4), torch.zeros(4, dtype=torch.long))
    pos = torch.tensor([[20, 21], [22, 23]])
    with pytest.raises(ValueError):
        plain.sample_links(pos, edge_label_time=torch.zeros(2, dtype=torch.long))
    s = mk(edge_time=time)
    seeds = torch.arange(4)
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(4),
                torch.zeros(4, dtype=torch.int32),
                torch.zeros(4, 1, dtype=torch.long)):
        with pytest.raises(ValueError):
            s.sample_temporal(seeds, bad)
    with pytest.raises(ValueError):
        s.sample_temporal(torch.tensor([0, N_T]), torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        s.sample_temporal(seeds.float(), torch.zeros(4, dtype=torch.long))
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(2)):
        with pytest.raises(ValueError):
            s.sample_links(pos, edge_label_time=bad)
