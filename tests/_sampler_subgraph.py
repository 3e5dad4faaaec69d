"""Shared by test_cpu_sampler_subgraph.py and test_gpu_sampler_subgraph.py:
the graphs, the node sets and the checks of GraphSageSampler.subgraph and
sample_saint_rw, the same in every mode.  Nothing is drawn by subgraph, so
every comparison with the model below is exact."""
import functools

import numpy as np
import pytest
import torch

import quiver
from quiver import _ext
from quiver.pyg.sage_sampler import DST_PTR_ATTR
from _sampler_walks import topo_from_rows

N_S = 6000
EID_MODES = [(False, False), (True, False), (True, True)]  # return_eid, eid


def model(topo, nodes, with_ids):
    """(n_id, edge_index, dst_ptr, e_id) of the induced subgraph: the set's
    rows in first-occurrence order, each row's slots in order."""
    indptr, indices = topo.indptr.tolist(), topo.indices.tolist()
    eid = None if topo.eid is None else topo.eid.tolist()
    local = {}
    for v in nodes:
        local.setdefault(v, len(local))
    src, dst, ids, ptr = [], [], [], [0]
    for i, u in enumerate(local):
        for s in range(indptr[u], indptr[u + 1]):
            if indices[s] in local:
                src.append(local[indices[s]])
                dst.append(i)
                ids.append(s if eid is None else eid[s])
        ptr.append(len(src))
    long = functools.partial(torch.tensor, dtype=torch.long)
    return (long(list(local)), long([src, dst]), long(ptr),
            long(ids if with_ids else []))


@functools.lru_cache(None)
def structure_graph(eid):
    """Nodes 0..12 have the degrees below (12 is the hub), 13 has all its
    neighbours in the set and 14 none.  Members sit at the first and last
    slot of every chunk, so on both sides of every chunk boundary, and at a
    few random slots; every other slot holds a node kept out of the sets
    (62 and 66, next to the members 63..65, among them)."""
    c = _ext.subgraph_chunk_slots()
    degrees = [0, 1, 15, 16, 17, 63, 64, 65, c - 1, c, c + 1, 2 * c + 1, 5000]
    rng = np.random.default_rng(21)
    members = list(range(15)) + [63, 64, 65, N_S - 1]
    rows = []
    for d in degrees:
        row = rng.choice([62, 66] + list(range(100, 3000)), d)
        at = {s for k in range(0, d, c) for s in (k, min(k + c, d) - 1)}
        at |= set(rng.integers(0, max(d, 1), d // 20).tolist())
        for s in sorted(at):
            row[s] = members[s % len(members)]
        rows.append(row)
    rows[4][[0, 16]] = 64               # an edge stored twice
    rows[5][0] = 5                      # self-loops, the hub's at a chunk's
    rows[12][c] = 12                    # first slot
    rows[12][[1, 2]] = [62, 66]
    rows += [rng.choice(members, 40), rng.integers(100, 3000, 40)]
    rows += [rng.integers(0, N_S, d)
             for d in rng.integers(0, 9, N_S - len(rows))]
    return topo_from_rows(rows, eid)


@functools.lru_cache(None)
def big_graph(eid):
    rng = np.random.default_rng(22)
    return topo_from_rows([rng.integers(0, 50_000, d)
                           for d in rng.integers(0, 9, 50_000)], eid)


def node_set(name):
    """(graph, nodes).  The structured sets are out of id order and hold
    duplicates; none holds 62 or 66."""
    g = torch.Generator().manual_seed(23)
    if name == "big":       # more chunks than the capped grid has subgroups
        return big_graph, torch.randperm(50_000, generator=g)[:40_000]
    core = torch.tensor([12, 65, 3, 14, 0, 64, N_S - 1, 12, 7, 13, 63, 1, 11,
                         5, 2, 3, 10, 4, 9, 6, 8, 65])
    if name == "one":
        return structure_graph, [12]
    if name == "seventeen":
        return structure_graph, core[:18]           # 12 is there twice
    if name == "three_hundred":
        rest = 3000 + torch.randperm(2999, generator=g)[:281]
        return structure_graph, torch.cat([core, rest, core[:5]])
    return structure_graph, core


def make_sampler(topo, mode, **kw):
    return quiver.GraphSageSampler(topo, [2], device=0, mode=mode, **kw)


def check_batch(sampler, topo, sub, nodes):
    want = model(topo, torch.as_tensor(nodes).tolist(), sampler.return_eid)
    dst_ptr = getattr(sub.edge_index, DST_PTR_ATTR)
    got = (sub.n_id, sub.edge_index, dst_ptr, sub.e_id)
    device = "cpu" if sampler.mode == "CPU" else "cuda"
    for g, w in zip(got, want):
        assert g.device.type == device and g.dtype == torch.int64
        assert torch.equal(g.cpu(), w)
    return want


def check_set(mode, name, return_eid, eid):
    graph, nodes = node_set(name)
    topo = graph(eid)
    s = make_sampler(topo, mode, return_eid=return_eid)
    n_id, edge_index, _, _ = check_batch(s, topo, s.subgraph(nodes), nodes)
    assert edge_index.size(1) > 0
    if name == "struct":    # a full row, an empty row, the doubled edge
        deg = torch.bincount(edge_index[1], minlength=len(n_id))
        assert deg[n_id == 13] == 40 and deg[n_id == 14] == 0
        pair = edge_index[:, n_id[edge_index[1]] == 4]
        assert int((n_id[pair[0]] == 64).sum()) >= 2
    s.quiver.set_seed(5)    # no effect: nothing is drawn
    check_batch(s, topo, s.subgraph(nodes), nodes)


def check_empty(mode, return_eid):
    topo = structure_graph(False)
    s = make_sampler(topo, mode, return_eid=return_eid)
    sub = s.subgraph(torch.zeros(0, dtype=torch.long))
    check_batch(s, topo, sub, [])
    assert tuple(sub.edge_index.shape) == (2, 0)


def check_bad_id(mode, bad, device="cpu"):
    """Ids -1 and N raise; the sampler works on afterwards."""
    topo = structure_graph(False)
    s = make_sampler(topo, mode)
    nodes = torch.tensor([3, N_S if bad else -1, 12], device=device)
    with pytest.raises(ValueError):
        s.subgraph(nodes)
    check_batch(s, topo, s.subgraph([3, 12]), [3, 12])


def check_saint_rw(mode, p, q):
    topo = structure_graph(True)
    s = make_sampler(topo, mode, return_eid=True)
    roots = torch.tensor([7, 0, 12, 7, 5000, 1] + list(range(100, 400)))
    s.lazy_init_quiver()
    s.quiver.set_seed(31)
    walk = s.random_walk(roots, 3, p, q)[0].cpu()
    assert bool((walk < 0).any())               # node 0 has no out-edge
    s.quiver.set_seed(31)
    sub = s.sample_saint_rw(roots, 3, p, q)
    n_id = sub.n_id.cpu()
    assert set(n_id.tolist()) == set(walk[walk >= 0].tolist())
    assert len(set(n_id.tolist())) == n_id.numel()
    lead = list(dict.fromkeys(roots.tolist()))
    assert n_id[:len(lead)].tolist() == lead
    check_batch(s, topo, sub, n_id)


def check_layer(mode):
    """A sorted_dst layer takes the batch as it is, and the attached
    dst_ptr changes nothing but the searchsorted it saves."""
    graph, nodes = node_set("three_hundred")
    sub = make_sampler(graph(False), mode).subgraph(nodes)
    n = sub.n_id.numel()
    assert getattr(sub.edge_index, DST_PTR_ATTR).numel() == n + 1
    torch.manual_seed(0)
    conv = quiver.nn.SAGEConv(8, 4, sorted_dst=True).to(sub.n_id.device)
    x = torch.randn(N_S, 8, device=sub.n_id.device)[sub.n_id]
    with torch.no_grad():
        out = conv((x, x), sub.edge_index, (n, n))
        plain = conv((x, x), sub.edge_index.clone(), (n, n))
    assert tuple(out.shape) == (n, 4) and torch.equal(out, plain)


# (check, its arguments after the mode, repeated in UVA mode): every mode
# runs all of them; UVA repeats those that read rows
CASES = (
    [(check_set, ("struct", r, e), True) for r, e in EID_MODES]
    + [(check_set, (name, True, True), True)
       for name in ("one", "seventeen", "three_hundred", "big")]
    + [(check_empty, (r,), False) for r in (False, True)]
    + [(check_bad_id, (bad,), True) for bad in (0, 1)]
    + [(check_saint_rw, pq, True) for pq in [(1.0, 1.0), (0.5, 2.0)]]
    + [(check_layer, (), False)])


def case_id(case):
    return "-".join([case[0].__name__[6:]] + [str(a) for a in case[1]])
