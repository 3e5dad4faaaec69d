"""Shared by test_cpu_sampler_links.py and test_gpu_sampler_links.py: the
graphs and the checks of the negative-tail draw (sample_negative) and of
link-prediction batches (sample_links), the same in every mode."""
import numpy as np
import torch

import quiver

NEG_TRIES = 16
NUM_NEGS = [1, 5, 16, 17, 40]
SEED = 2024

# ---- graph A: sparse, 5000 nodes, with the special rows first ----------
N_A = 5000
A_DEGREES = [0, 1, 15, 16, 17, 40]      # nodes 0..5
A_ONE_LEFT = 6                          # degree N-2: one valid tail
A_NONE_LEFT = 7                         # degree N-1: none
A_VALID_TAIL = 4321                     # the one node missing from row 6
A_SOURCES = 200                         # sources 0..199 in the small cases

# ---- graph B: 64 nodes, every row 48 distinct neighbours ----------------
N_B = 64
B_DEGREE = 48

# ---- uniformity: 200 nodes, node 0 of degree 40 -------------------------
N_U = 200
U_DEGREE = 40
U_REPEAT = 1000
U_NUM_NEG = 16
U_DF = N_U - 1 - U_DEGREE - 1           # 159 valid tails
CHI2_BOUND = U_DF + 5 * np.sqrt(2 * U_DF)       # 246.9


def _topo_from_rows(rows, nodes):
    deg = torch.tensor([len(r) for r in rows], dtype=torch.long)
    indptr = torch.zeros(nodes + 1, dtype=torch.long)
    indptr[1:] = torch.cumsum(deg, 0)
    indices = torch.from_numpy(
        np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]))
    return quiver.CSRTopo(indptr=indptr, indices=indices)


def _others(rng, v, nodes, count):
    """`count` distinct nodes other than v, in random (unsorted) order."""
    pick = rng.permutation(nodes - 1)[:count]
    return pick + (pick >= v)


def graph_a():
    rng = np.random.default_rng(1)
    rows = []
    for v in range(N_A):
        if v < len(A_DEGREES):
            rows.append(_others(rng, v, N_A, A_DEGREES[v]))
        elif v == A_ONE_LEFT:
            row = np.array([x for x in range(N_A)
                            if x != v and x != A_VALID_TAIL])
            rows.append(rng.permutation(row))
        elif v == A_NONE_LEFT:
            rows.append(rng.permutation(
                np.array([x for x in range(N_A) if x != v])))
        else:
            rows.append(_others(rng, v, N_A, int(rng.integers(0, 9))))
    return _topo_from_rows(rows, N_A)


def graph_b():
    rng = np.random.default_rng(2)
    return _topo_from_rows([_others(rng, v, N_B, B_DEGREE)
                            for v in range(N_B)], N_B)


def graph_u():
    rng = np.random.default_rng(3)
    rows = [_others(rng, 0, N_U, U_DEGREE)] + [np.zeros(0, np.int64)] * (
        N_U - 1)
    return _topo_from_rows(rows, N_U)


def edge_keys(topo):
    """The host set of the graph's edges, as sorted keys u * N + v."""
    n = topo.node_count
    u = torch.repeat_interleave(torch.arange(n), topo.degree)
    return np.unique((u * n + topo.indices).numpy())


def make_sampler(topo, mode, sizes=(4, 3), seed=SEED, **kw):
    s = quiver.GraphSageSampler(topo, list(sizes), device=0, mode=mode, **kw)
    s.lazy_init_quiver()
    if mode != "CPU":               # the CPU engine has no seed to set
        s.quiver.set_seed(seed)
    return s


def draw(sampler, src, num_neg, tries=NEG_TRIES):
    """sample_negative, with shape, dtype and device checked; on the host."""
    neg, ok = sampler.sample_negative(src, num_neg, tries)
    p = len(src)
    assert tuple(neg.shape) == (p, num_neg) and neg.dtype == torch.int64
    assert tuple(ok.shape) == (p, num_neg) and ok.dtype == torch.bool
    want = "cpu" if sampler.mode == "CPU" else "cuda"
    assert neg.device.type == want and ok.device.type == want
    return neg.cpu(), ok.cpu()


def check_valid(topo, keys, src, neg, ok):
    """Every value in range; every ok entry neither u nor in u's row."""
    n = topo.node_count
    src = torch.as_tensor(src)
    if neg.numel() == 0:
        return
    assert int(neg.min()) >= 0 and int(neg.max()) < n
    u = src[:, None].expand_as(neg)
    is_edge = torch.from_numpy(
        np.isin((u * n + neg).numpy(), keys, assume_unique=False))
    bad = ok & (is_edge | (neg == u))
    assert not bool(bad.any()), (u[bad][:8], neg[bad][:8])


def check_validity_case(mode, topo, keys, num_neg):
    n = topo.node_count
    src = torch.arange(min(n, A_SOURCES))
    s = make_sampler(topo, mode)
    neg, ok = draw(s, src, num_neg)
    check_valid(topo, keys, src, neg, ok)
    if n == N_A:
        # a truncated range never gets here; an exact draw misses it with
        # probability 0.9 ** 200 at num_neg = 1
        assert int(neg.max()) >= 0.9 * N_A
    return src, neg, ok


def check_ok_flags_a(mode, topo, keys):
    src, neg, ok = check_validity_case(mode, topo, keys, 40)
    plain = torch.ones(len(src), dtype=torch.bool)
    plain[[A_ONE_LEFT, A_NONE_LEFT]] = False
    # a draw in a plain row fails with probability under 0.01 ** 16
    assert bool(ok[plain].all())
    assert not bool(ok[A_NONE_LEFT].any())
    assert bool((neg[A_ONE_LEFT][ok[A_ONE_LEFT]] == A_VALID_TAIL).all())
    # with 256 tries a draw in that row succeeds with probability 5 %, so
    # 1024 of them leave the check above something to look at (none at
    # all: e ** -51)
    src = torch.full((64,), A_ONE_LEFT)
    neg, ok = draw(make_sampler(topo, mode), src, 16, tries=256)
    assert bool(ok.any())
    assert bool((neg[ok] == A_VALID_TAIL).all())
    assert int(neg.min()) >= 0 and int(neg.max()) < N_A


def not_ok_share_b(mode, topo, keys):
    src = torch.arange(N_B)
    s = make_sampler(topo, mode)
    neg, ok = draw(s, src, 16)
    check_valid(topo, keys, src, neg, ok)
    share = 1.0 - float(ok.float().mean())
    print("graph B not-ok share", share)
    return share


def chi_square(tails, valid):
    """Chi-square statistic of `tails` against the uniform draw over
    `valid` (every tail must be one of them)."""
    valid = np.asarray(valid)
    at = np.searchsorted(valid, tails)
    assert np.all(valid[np.minimum(at, len(valid) - 1)] == tails)
    count = np.bincount(at, minlength=len(valid))
    expect = len(tails) / len(valid)
    return float(((count - expect) ** 2 / expect).sum())


def uniformity_draw(mode, topo):
    """16 000 tails of node 0 of graph U and their chi-square statistic
    over the 159 valid tails, df = 158, bound df + 5 sqrt(2 df) = 246.9.

    Checked with numpy (default_rng(0), 16 000 draws) before any seed was
    chosen: an exact uniform draw over the 159 valid tails gives 184.1,
    well inside; a draw that reaches only the first 2048/5000 of the node
    range (the 67 valid tails under 82, as a 53-bit multiply that
    overflows would leave it) gives 22 153, far outside.  Ten runs of the
    CPU engine, which has no seed to fix, gave 129 to 177."""
    s = make_sampler(topo, mode, seed=77)
    src = torch.zeros(U_REPEAT, dtype=torch.long)
    neg, ok = draw(s, src, U_NUM_NEG)
    assert bool(ok.all())       # one draw fails with (41/200) ** 16
    row = set(topo.indices[:U_DEGREE].tolist())
    valid = [v for v in range(1, N_U) if v not in row]
    assert len(valid) == U_DF + 1
    stat = chi_square(neg.flatten().numpy(), valid)
    print("chi-square", stat, "bound", CHI2_BOUND)
    return neg, stat


def check_links(mode, coo, topo, num_neg, return_eid=False, sizes=(4, 3)):
    """The issue's checks of one sample_links batch."""
    p = 50
    g = torch.Generator().manual_seed(5)
    pos = coo[:, torch.randperm(coo.shape[1], generator=g)[:p]]
    s = make_sampler(topo, mode, sizes=sizes, return_eid=return_eid)
    b = s.sample_links(pos, num_neg=num_neg)
    assert isinstance(b, quiver.LinkBatch)
    want = "cpu" if mode == "CPU" else "cuda"
    for t in (b.n_id, b.edge_label_index, b.edge_label, b.neg_ok):
        assert t.device.type == want
    n_id, eli = b.n_id.cpu(), b.edge_label_index.cpu()
    total = p * (1 + num_neg)
    assert tuple(eli.shape) == (2, total) and eli.dtype == torch.int64
    assert tuple(b.neg_ok.shape) == (p * num_neg,)
    assert b.neg_ok.dtype == torch.bool
    assert b.edge_label.dtype == torch.float32
    assert torch.equal(b.edge_label.cpu(),
                       torch.tensor([1.0] * p + [0.0] * (p * num_neg)))
    assert int(eli.min()) >= 0 and int(eli.max()) < b.batch_size
    glob = n_id[eli]
    assert torch.equal(glob[:, :p], pos)
    assert torch.equal(glob[0, p:], pos[0].repeat_interleave(num_neg))
    seeds = n_id[:b.batch_size]
    assert torch.unique(seeds).numel() == b.batch_size
    assert set(seeds.tolist()) == set(glob.flatten().tolist())
    # accepted negatives are no edges of the graph
    n = topo.node_count
    is_edge = np.isin((glob[0, p:] * n + glob[1, p:]).numpy(),
                      edge_keys(topo))
    ok = b.neg_ok.cpu().numpy()
    assert not np.any(ok & (is_edge | (glob[0, p:] == glob[1, p:]).numpy()))
    assert len(b.adjs) == len(sizes)
    n_dst = b.batch_size
    for adj in b.adjs[::-1]:
        assert int(adj.size[1]) == n_dst
        n_dst = int(adj.size[0])
        if return_eid:
            m = adj.edge_index.shape[1]
            assert m > 0 and tuple(adj.e_id.shape) == (m,)
            e = adj.e_id.cpu()
            assert torch.equal(coo[0, e], n_id[adj.edge_index[1].cpu()])
            assert torch.equal(coo[1, e], n_id[adj.edge_index[0].cpu()])
    assert n_dst == n_id.numel()
    return b
