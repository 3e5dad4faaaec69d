"""Shared by test_cpu_sampler_walks.py and test_gpu_sampler_walks.py: the
graphs and the checks of GraphSageSampler.random_walk, the same in every
mode.  Rows are built by hand and left unsorted."""
import numpy as np
import pytest
import torch

import quiver

SEED = 2025
PQ = [(1.0, 1.0), (0.5, 2.0), (4.0, 0.25)]
PQ2 = PQ[1:]                                    # second-order only
# (D, pos): length of t's row, position of the adjacent node in it
W_EXACT = [(1, 0), (16, 15), (17, 16), (64, 63), (65, 64), (200, 199),
           (200, 0)]
W_REJECT = [(17, 16), (200, 199)]
CHI2_DF2_BOUND = 27.6                           # exp(-27.6 / 2) = 1e-6

N_S = 2000
S_DEGREES = [0, 1, 15, 16, 17, 64, 65, 5000]    # nodes 0..7, node 7 the hub


def topo_from_rows(rows, eid=False):
    deg = torch.tensor([len(r) for r in rows], dtype=torch.long)
    indptr = torch.zeros(len(rows) + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.from_numpy(np.concatenate(
        [np.asarray(r, dtype=np.int64) for r in rows]))
    perm = torch.randperm(indices.numel(),
                          generator=torch.Generator().manual_seed(4))
    return quiver.CSRTopo(indptr=indptr, indices=indices,
                          eid=perm if eid else None)


def make_sampler(topo, mode, seed=SEED, **kw):
    s = quiver.GraphSageSampler(topo, [2], device=0, mode=mode, **kw)
    s.lazy_init_quiver()
    s.quiver.set_seed(seed)
    return s


def walks(topo, mode, start, length, p=1.0, q=1.0, seed=SEED, **kw):
    """random_walk with shapes, dtypes and device checked; on the host."""
    s = make_sampler(topo, mode, seed, return_eid=kw.pop("return_eid", False))
    walk, e_id = s.random_walk(start, length, p, q, **kw)
    b = len(start)
    assert tuple(walk.shape) == (b, length + 1) and walk.dtype == torch.int64
    assert tuple(e_id.shape) == (b, length if s.return_eid else 0)
    assert e_id.dtype == torch.int64
    want = "cpu" if mode == "CPU" else "cuda"
    assert walk.device.type == want and e_id.device.type == want
    return s, walk.cpu(), e_id.cpu()


def structure_graph(eid):
    rng = np.random.default_rng(11)
    deg = S_DEGREES + list(rng.integers(0, 9, N_S - len(S_DEGREES)))
    return topo_from_rows([rng.integers(0, N_S, d) for d in deg], eid)


def check_structure(mode, p, q, return_eid, eid):
    topo = structure_graph(eid)
    n, length = N_S, 8
    start = torch.arange(4096) % n              # every node twice at least
    s, walk, e_id = walks(topo, mode, start, length, p, q,
                          return_eid=return_eid)
    assert torch.equal(walk[:, 0], start)
    src = torch.repeat_interleave(torch.arange(n), topo.degree)
    keys = src * n + topo.indices
    u, v = walk[:, :-1], walk[:, 1:]
    alive = v >= 0
    assert bool(torch.isin(u[alive] * n + v[alive], keys).all())
    # a walk ends only at an empty row, and stays ended
    ends = ~alive & (u >= 0)
    assert bool((topo.degree[u[ends]] == 0).all())
    assert not bool((alive & (u < 0)).any())
    assert bool(ends.any()) and bool(alive[:, -1].any())
    assert bool((walk[:n] != walk[n:2 * n]).any())
    if return_eid:
        assert torch.equal(e_id < 0, ~alive)
        slot_of = torch.arange(keys.numel()) if topo.eid is None \
            else torch.argsort(topo.eid)        # edge id -> CSR slot
        assert torch.equal(keys[slot_of[e_id[alive]]],
                           u[alive] * n + v[alive])
    s.quiver.set_seed(SEED)
    again = s.random_walk(start, length, p, q)
    assert torch.equal(again[0].cpu(), walk)
    assert torch.equal(again[1].cpu(), e_id)
    assert not torch.equal(s.random_walk(start, length, p, q)[0].cpu(), walk)


def check_determined(mode, p, q):
    cycle = topo_from_rows([[(v + 1) % 7] for v in range(7)])
    start = torch.arange(20) % 7
    _, walk, _ = walks(cycle, mode, start, 20, p, q)
    assert torch.equal(walk, (start[:, None] + torch.arange(21)) % 7)
    path = topo_from_rows([[1], [2], [3], []])
    _, walk, e_id = walks(path, mode, [0, 0], 6, p, q, return_eid=True)
    assert walk.tolist() == [[0, 1, 2, 3, -1, -1, -1]] * 2
    assert e_id.tolist() == [[0, 1, 2, -1, -1, -1]] * 2


def check_no_return(mode):
    rows = [[1]] + [[v + 1, v - 1] if v % 2 else [v - 1, v + 1]
                    for v in range(1, 49)] + [[48]]
    _, walk, _ = walks(topo_from_rows(rows), mode, [0] * 8, 40, 1e9, 1.0)
    assert torch.equal(walk, torch.arange(41).expand(8, 41))


def check_uniform_step(mode, degree, count):
    rng = np.random.default_rng(12)
    rows = [rng.permutation(degree) + 1] + [[]] * degree
    _, walk, _ = walks(topo_from_rows(rows), mode, [0] * count, 1)
    got = np.bincount(walk[:, 1].numpy(), minlength=degree + 1)[1:]
    expect = count / degree
    stat = float(((got - expect) ** 2 / expect).sum())
    df = degree - 1
    print("chi-square", stat, "bound", df + 5 * np.sqrt(2 * df))
    assert stat < df + 5 * np.sqrt(2 * df)


def check_second_order(mode, d, pos, p, q, extra=0, **kw):
    """W(D, pos): t = 0, c_i = 1 + i, b_i = 1 + D + i, and `extra` further
    far nodes in every c_i's row.  The second step of a walk from t
    returns, goes to c_pos or goes far with weights 1/p : 1 : (1 + extra)/q."""
    far = list(range(1 + 2 * d, 1 + 2 * d + extra))
    rows = [list(range(1, d + 1))] + \
        [[0, 1 + pos, 1 + d + i] + far for i in range(d)] + \
        [[]] * (d + extra)
    _, walk, _ = walks(topo_from_rows(rows), mode, [0] * 60_000, 2, p, q,
                       **kw)
    last = walk[:, 2]
    got = np.array([int((last == 0).sum()), int((last == 1 + pos).sum()), 0])
    got[2] = len(last) - got[:2].sum()
    assert int(last.min()) >= 0
    weight = np.array([1 / p, 1.0, (1 + extra) / q])
    expect = len(last) * weight / weight.sum()
    stat = float(((got - expect) ** 2 / expect).sum())
    print("classes", got, "expected", expect.round(1), "chi-square", stat)
    assert stat < CHI2_DF2_BOUND


def check_exhaustion(mode):
    topo = topo_from_rows([[1], [0] * 17])
    _, walk, _ = walks(topo, mode, [0] * 4, 6, 1e9, 1.0, max_tries=16)
    assert walk.tolist() == [[0, 1, 0, 1, 0, 1, 0]] * 4


BAD_ARGS = [dict(p=0.0), dict(p=float("inf")), dict(q=float("nan")),
            dict(q=-1.0), dict(walk_length=0), dict(max_tries=15),
            dict(edge_weight=True)]


def check_arguments(mode, bad):
    topo = topo_from_rows([[1], [0, 0]])
    bad = dict(bad)
    weight = torch.ones(3) if bad.pop("edge_weight", False) else None
    s = make_sampler(topo, mode, edge_weight=weight)
    args = dict(walk_length=3, p=1.0, q=1.0, max_tries=256)
    args.update(bad)
    with pytest.raises(ValueError):
        s.random_walk([0, 1], **args)


def check_empty_batch(mode, return_eid):
    topo = topo_from_rows([[1], [0, 0]])
    for p in (1.0, 2.0):
        walks(topo, mode, torch.zeros(0, dtype=torch.long), 5, p,
              return_eid=return_eid)


# (check, its arguments after the mode, repeated in UVA mode): every mode
# runs all of them; UVA repeats those whose row reads matter there
CASES = (
    [(check_structure, (p, q, r, e), True) for p, q in PQ
     for r, e in [(False, False), (True, False), (True, True)]]
    + [(check_determined, pq, False) for pq in PQ]
    + [(check_no_return, (), False), (check_exhaustion, (), False)]
    + [(check_uniform_step, a, False)
       for a in [(40, 40_000), (5000, 100_000)]]
    + [(check_second_order, (d, pos, p, q), True)
       for d, pos in W_EXACT for p, q in PQ2]
    + [(check_second_order, (d, pos, p, q, 30), True)
       for d, pos in W_REJECT for p, q in PQ2 + [(0.05, 1.0)]]
    + [(check_arguments, (bad,), False) for bad in BAD_ARGS]
    + [(check_empty_batch, (r,), False) for r in (False, True)])


def case_id(case):
    return "-".join([case[0].__name__[6:]] + [str(a) for a in case[1]])
