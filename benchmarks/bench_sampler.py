#!/usr/bin/env python3
"""Sampling throughput (SEPS = sampled edges / second).

Mirrors the reference's headline sampling benchmark
(torch-quiver benchmarks/sample/bench_sampler.py: SEPS counted as
sum(edge counts) / sample time) on synthetic graphs of the named shapes:
  - ogbn-products: 2.45M nodes / 123.7M edges, fanout [15,10,5]
  - reddit:        233k nodes / 114.6M edges, fanout [25,10]
Baselines to beat (other hardware): CPU 1.84M/2.0M, UVA 34.29M/33.15M SEPS.
"""
import argparse
import json
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import quiver

SHAPES = {
    "products": dict(nodes=2_449_029, edges=123_718_280, fanout=[15, 10, 5],
                     train=196_615),
    "reddit": dict(nodes=232_965, edges=114_615_892, fanout=[25, 10],
                   train=153_431),
}


def make_graph(nodes, edges, seed=0, max_deg=20_000):
    rng = np.random.default_rng(seed)
    raw = rng.pareto(1.3, nodes) + 0.1
    deg = np.maximum((raw * (edges / raw.sum())).astype(np.int64), 1)
    np.clip(deg, 1, max_deg, out=deg)
    deg = -np.sort(-deg)
    indptr = np.zeros(nodes + 1, dtype=np.int64)
    np.cumsum(deg, out=indptr[1:])
    u = rng.random(int(indptr[-1]), dtype=np.float32)
    indices = np.clip((u * u * nodes).astype(np.int64), 0, nodes - 1)
    return torch.from_numpy(indptr), torch.from_numpy(indices)


def make_weights(edges, seed=1):
    """fp32 edge weights, uniform in [0.5, 2)."""
    rng = np.random.default_rng(seed)
    w = rng.random(edges, dtype=np.float32)
    w *= 1.5
    w += 0.5
    return torch.from_numpy(w)


def bench(mode, shape, batch=1024, iters=50, warmup=5, device=0,
          return_eid=False, edge_weight=False):
    cfg = SHAPES[shape]
    indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    opts = {}
    if return_eid:
        opts["return_eid"] = True
    if edge_weight:
        opts["edge_weight"] = make_weights(indices.numel())
    sampler = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                      mode=mode, **opts)
    g = torch.Generator().manual_seed(7)
    batches = [torch.randint(0, cfg["train"], (batch,), generator=g)
               for _ in range(warmup + iters)]
    for i in range(warmup):
        sampler.sample(batches[i])
    if mode != "CPU":
        torch.cuda.synchronize()
    edges = 0
    t0 = time.perf_counter()
    for i in range(iters):
        _, _, adjs = sampler.sample(batches[warmup + i])
        edges += sum(adj.edge_index.shape[1] for adj in adjs)
    if mode != "CPU":
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(mode=mode, shape=shape, seps=edges / dt,
                ms_per_batch=dt / iters * 1000, batch=batch, iters=iters,
                return_eid=bool(return_eid), edge_weight=bool(edge_weight))


def _timed(fn, args_list, sync):
    """ms per call of fn over args_list, ending in a device synchronise."""
    t0 = time.perf_counter()
    for a in args_list:
        fn(a)
    sync()
    return (time.perf_counter() - t0) / len(args_list) * 1000


def _stats(xs):
    """median and spread of the repeats."""
    return dict(median=float(np.median(xs)), min=float(np.min(xs)),
                max=float(np.max(xs)))


def bench_links(mode, shape, topo, batch=1024, num_neg=1, iters=30,
                repeats=7, warmup=5, device=0):
    """Link-prediction batches: sample_negative alone, torch.unique on a
    batch's endpoints alone, sample_links end to end, and, as the
    baseline, plain sample() on the link batches' own seed nodes.  Each
    repeat times `iters` calls of each of the four in turn; reported are
    the median and the min..max over the repeats, in ms per call."""
    cfg = SHAPES[shape]
    sampler = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                      mode=mode)
    dev = "cpu" if mode == "CPU" else f"cuda:{device}"
    sync = (lambda: None) if mode == "CPU" else torch.cuda.synchronize
    g = torch.Generator().manual_seed(7)
    pos = []
    for _ in range(iters):
        src = torch.randint(0, cfg["train"], (batch,), generator=g)
        at = topo.indptr[src] + (torch.randint(0, 1 << 40, (batch,),
                                               generator=g)
                                 % topo.degree[src].clamp(min=1))
        pos.append(torch.stack([src, topo.indices[at]]).to(dev))
    srcs = [p[0].contiguous() for p in pos]
    # the seed sets and endpoint lists of these very batches
    seeds, ends, not_ok = [], [], 0
    for p, s in zip(pos, srcs):
        b = sampler.sample_links(p, num_neg=num_neg)
        seeds.append(b.n_id[:b.batch_size].clone())
        ends.append(torch.cat([p[0], p[1], sampler.sample_negative(
            s, num_neg)[0].reshape(-1)]))
        not_ok += int((~b.neg_ok).sum())
    parts = dict(
        sample_negative=(lambda s: sampler.sample_negative(s, num_neg), srcs),
        unique=(lambda e: torch.unique(e, return_inverse=True), ends),
        sample_links=(lambda p: sampler.sample_links(p, num_neg=num_neg),
                      pos),
        sample=(sampler.sample, seeds))
    for fn, args_list in parts.values():
        _timed(fn, args_list[:warmup], sync)
    ms = {k: [] for k in parts}
    for _ in range(repeats):
        for k, (fn, args_list) in parts.items():
            ms[k].append(_timed(fn, args_list, sync))
    res = dict(mode=mode, shape=shape, links=True, batch=batch,
               num_neg=num_neg, iters=iters, repeats=repeats,
               seed_nodes=float(np.mean([s.numel() for s in seeds])),
               not_ok=not_ok)
    for k, v in ms.items():
        res[k + "_ms"] = _stats(v)
    links = res["sample_links_ms"]["median"]
    res["share_negative"] = res["sample_negative_ms"]["median"] / links
    res["share_unique"] = res["unique_ms"]["median"] / links
    return res


TIME_RANGE = 1 << 20


def make_times(edges, seed=2):
    """int64 edge times, uniform in [0, 2**20)."""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, TIME_RANGE, edges,
                                         dtype=np.int64))


def bench_temporal(mode, shape, topo, edge_time, batch=1024, iters=30,
                   repeats=7, warmup=5, device=0, links=False, num_neg=1):
    """Temporal sampling: sample_temporal with every seed bounded at the
    median edge time, beside two reference points on the same seeds from a
    sampler without edge times: plain sample() (the fused chain, merged
    frontier) and sample() with sort_frontier=True (the per-hop path that
    sample_temporal is built like).  With `links` also temporal
    sample_links beside the merged sample_links.  Each repeat times `iters`
    calls of each in turn; reported are the median and the min..max over
    the repeats, in ms per call."""
    cfg = SHAPES[shape]
    t0 = time.perf_counter()
    temporal = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                       mode=mode, edge_time=edge_time)
    sort_s = time.perf_counter() - t0
    plain = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                    mode=mode)
    per_hop = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                      mode=mode)
    per_hop.sort_frontier = True
    dev = "cpu" if mode == "CPU" else f"cuda:{device}"
    sync = (lambda: None) if mode == "CPU" else torch.cuda.synchronize
    g = torch.Generator().manual_seed(7)
    seeds = [torch.randint(0, cfg["train"], (batch,), generator=g).to(dev)
             for _ in range(iters)]
    median = TIME_RANGE // 2
    bound = torch.full((batch,), median, dtype=torch.long, device=dev)
    parts = dict(
        sample_temporal=(lambda s: temporal.sample_temporal(s, bound), seeds),
        sample=(plain.sample, seeds),
        sample_per_hop=(per_hop.sample, seeds))
    if links:
        pos = []
        for _ in range(iters):
            src = torch.randint(0, cfg["train"], (batch,), generator=g)
            at = topo.indptr[src] + (torch.randint(0, 1 << 40, (batch,),
                                                   generator=g)
                                     % topo.degree[src].clamp(min=1))
            pos.append(torch.stack([src, topo.indices[at]]).to(dev))
        parts["sample_links_temporal"] = (
            lambda p: temporal.sample_links(p, num_neg=num_neg,
                                            edge_label_time=bound), pos)
        parts["sample_links"] = (
            lambda p: plain.sample_links(p, num_neg=num_neg), pos)
    sizes = {}
    for k, (fn, args_list) in parts.items():
        _timed(fn, args_list[:warmup], sync)
        out = fn(args_list[0])
        sizes[k] = dict(frontier=int(out[0].numel()),
                        edges=int(sum(a.edge_index.shape[1]
                                      for a in out[2])))
    ms = {k: [] for k in parts}
    for _ in range(repeats):
        for k, (fn, args_list) in parts.items():
            ms[k].append(_timed(fn, args_list, sync))
    res = dict(mode=mode, shape=shape, temporal=True, links=bool(links),
               batch=batch, num_neg=num_neg, iters=iters, repeats=repeats,
               bound=median, sort_seconds=sort_s, first_batch=sizes)
    for k, v in ms.items():
        res[k + "_ms"] = _stats(v)
    return res


def torch_uniform_walk(indptr, indices, start, length):
    """The only baseline there is: a uniform walk as `length` rounds of
    torch index arithmetic on device-resident indptr / indices."""
    last = indices.numel() - 1
    cur, out = start, [start]
    for _ in range(length):
        live = cur >= 0
        at = cur.clamp(min=0)
        beg = indptr[at]
        deg = indptr[at + 1] - beg
        r = (torch.rand(cur.numel(), device=cur.device,
                        dtype=torch.float64) * deg).long()
        nxt = indices[(beg + r).clamp(max=last)]
        cur = torch.where(live & (deg > 0), nxt, torch.full_like(nxt, -1))
        out.append(cur)
    return torch.stack(out, 1)


def bench_walk(mode, shape, topo, p, q, length=20, batches=(1024, 65536),
               iters=20, repeats=7, warmup=3, device=0):
    """random_walk: uniform walks and (p, q) walks of `length` steps for
    each batch size, and in GPU mode the plain-torch uniform walk on the
    same starts (it needs the CSR in HBM, so UVA mode has no baseline).
    Each repeat times `iters` calls of each in turn, over `iters` different
    start sets; reported are the median and the min..max over the repeats
    in ms per call, and walk steps per second at the median."""
    cfg = SHAPES[shape]
    sampler = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                      mode=mode)
    dev = f"cuda:{device}"
    sync = torch.cuda.synchronize
    res = dict(mode=mode, shape=shape, walk=True, walk_length=length, p=p,
               q=q, iters=iters, repeats=repeats, batches={})
    if mode == "GPU":
        d_indptr, d_indices = topo.indptr.to(dev), topo.indices.to(dev)
    g = torch.Generator().manual_seed(7)
    for batch in batches:
        starts = [torch.randint(0, cfg["train"], (batch,), generator=g)
                  .to(dev) for _ in range(iters)]
        parts = dict(
            uniform=lambda s: sampler.random_walk(s, length),
            node2vec=lambda s: sampler.random_walk(s, length, p, q))
        if mode == "GPU":
            parts["torch_uniform"] = lambda s: torch_uniform_walk(
                d_indptr, d_indices, s, length)
        for fn in parts.values():
            _timed(fn, starts[:warmup], sync)
        ms = {k: [] for k in parts}
        for _ in range(repeats):
            for k, fn in parts.items():
                ms[k].append(_timed(fn, starts, sync))
        cell = {}
        for k, v in ms.items():
            cell[k + "_ms"] = _stats(v)
            cell[k + "_steps_per_s"] = \
                batch * length / (float(np.median(v)) * 1e-3)
        res["batches"][str(batch)] = cell
    return res


class TorchSubgraph:
    """The comparison for GraphSageSampler.subgraph in GPU mode: the same
    (n_id, edge_index) from torch ops alone on device-resident indptr /
    indices.  Rows are expanded with repeat_interleave and membership and
    local ids come from one dense lookup tensor over all nodes, kept
    between calls and reset after each."""

    def __init__(self, indptr, indices):
        self.indptr, self.indices = indptr, indices
        self.lookup = torch.full((indptr.numel() - 1,), -1,
                                 dtype=torch.long, device=indptr.device)

    def __call__(self, nodes):
        dev = nodes.device
        uniq, inv = torch.unique(nodes, return_inverse=True)
        first = torch.full_like(uniq, nodes.numel()).scatter_reduce_(
            0, inv, torch.arange(nodes.numel(), device=dev), "amin")
        n_id = uniq[torch.argsort(first)]
        n = n_id.numel()
        self.lookup[n_id] = torch.arange(n, device=dev)
        beg = self.indptr[n_id]
        deg = self.indptr[n_id + 1] - beg
        row = torch.repeat_interleave(torch.arange(n, device=dev), deg)
        start = torch.cumsum(deg, 0) - deg
        slot = torch.arange(row.numel(), device=dev) + (beg - start)[row]
        src = self.lookup[self.indices[slot]]
        keep = src >= 0
        edge_index = torch.stack([src[keep], row[keep]])
        self.lookup[n_id] = -1
        return n_id, edge_index


def bench_subgraph(mode, shape, topo, iters=10, repeats=7, warmup=2,
                   device=0, chunks=(64, 256, 1024), passes=10):
    """subgraph on three kinds of node set: the nodes of a GraphSAINT
    random-walk batch (3000 roots, walks of 2 steps), 100 000 uniform
    random nodes, and, for the cost of a hub row, 1024 uniform nodes with
    and without node 0 (the graph's longest row).  Timed per set: the
    engine at every built chunk size, the public call, sample_saint_rw as
    a whole (walk + subgraph) and, in GPU mode, TorchSubgraph.  Each repeat
    times `passes` rounds over `iters` different sets for each in turn;
    reported are the median and the min..max over the repeats in ms per
    call, the mean slots of the sets' rows and edges found, and for UVA
    mode the host bytes the two passes read (16 B a slot)."""
    cfg = SHAPES[shape]
    sampler = quiver.GraphSageSampler(topo, cfg["fanout"], device=device,
                                      mode=mode)
    sampler.lazy_init_quiver()
    dev = f"cuda:{device}"
    sync = torch.cuda.synchronize
    g = torch.Generator().manual_seed(7)
    n_nodes = cfg["nodes"]
    roots = [torch.randint(0, cfg["train"], (3000,), generator=g).to(dev)
             for _ in range(iters)]

    def walk_nodes(r):
        walk = sampler.random_walk(r, 2)[0]
        return torch.where(walk < 0, walk[:, :1], walk).t().reshape(-1)

    no_hub = [1 + torch.randint(0, n_nodes - 1, (1024,), generator=g)
              .to(dev) for _ in range(iters)]
    sets = dict(
        saint_rw=[walk_nodes(r) for r in roots],
        uniform_100k=[torch.randint(0, n_nodes, (100_000,), generator=g)
                      .to(dev) for _ in range(iters)],
        no_hub_1k=no_hub,
        hub_1k=[torch.cat([s.new_zeros(1), s]) for s in no_hub])
    res = dict(mode=mode, shape=shape, subgraph=True, iters=iters,
               passes=passes, repeats=repeats, default_chunk=quiver._ext.subgraph_chunk_slots(),
               sets={})
    if mode == "GPU":
        torch_sub = TorchSubgraph(topo.indptr.to(dev), topo.indices.to(dev))
    degree = topo.degree.to(dev)
    for name, node_sets in sets.items():
        parts = {f"chunk_{c}": (lambda s, c=c: sampler.quiver.subgraph(s, c))
                 for c in chunks}
        parts["subgraph"] = sampler.subgraph
        if mode == "GPU":
            parts["torch"] = torch_sub
        lists = {k: node_sets for k in parts}
        if name == "saint_rw":
            parts["sample_saint_rw"] = lambda r: sampler.sample_saint_rw(r, 2)
            lists["sample_saint_rw"] = roots
        for k, fn in parts.items():
            _timed(fn, lists[k][:warmup], sync)
        ms = {k: [] for k in parts}
        for _ in range(repeats):
            for k, fn in parts.items():
                ms[k].append(_timed(fn, lists[k] * passes, sync))
        subs = [sampler.subgraph(s) for s in node_sets]
        slots = float(np.mean([int(degree[b.n_id].sum()) for b in subs]))
        cell = {k + "_ms": _stats(v) for k, v in ms.items()}
        cell.update(
            nodes=float(np.mean([b.n_id.numel() for b in subs])),
            row_slots=slots,
            edges=float(np.mean([b.edge_index.size(1) for b in subs])))
        if mode == "UVA":
            cell["host_bytes_read"] = 16 * slots
            cell["host_gbps"] = 16 * slots / (
                cell["subgraph_ms"]["median"] * 1e-3) / 1e9
        res["sets"][name] = cell
    return res


ROW_BYTES = 400     # a feature row of bench.py's products preset: 100 fp32


def bench_labor(mode, shape, topo, layer_dependency=False, batch=1024,
                iters=10, repeats=7, warmup=2, device=0, passes=3,
                chunks=(64, 256, 1024)):
    """sample_labor beside plain sample() on the same seed batches: the
    public call, the engine with either fill pass (hit mask, hashing again)
    and at every built chunk size, and, for the cost of a hub row, batches
    of 1024 seeds with and without node 0 (the graph's longest row).  Each
    repeat times `passes` rounds over `iters` batches for each in turn;
    reported are the median and the min..max over the repeats in ms per
    batch and, as means over the batches, the edges of every hop (hop 0
    first), n_id.numel(), the bytes a gather of n_id moves at ROW_BYTES a
    row, and the ratio of the two methods' n_id sizes."""
    cfg = SHAPES[shape]
    sizes = cfg["fanout"]
    sampler = quiver.GraphSageSampler(topo, sizes, device=device, mode=mode)
    sampler.lazy_init_quiver()
    eng, ld = sampler.quiver, bool(layer_dependency)
    dev = f"cuda:{device}"
    sync = torch.cuda.synchronize
    g = torch.Generator().manual_seed(7)
    seeds = [torch.randint(0, cfg["train"], (batch,), generator=g).to(dev)
             for _ in range(iters)]
    no_hub = [1 + torch.randint(0, cfg["nodes"] - 1, (1024,), generator=g)
              .to(dev) for _ in range(iters)]
    hub = [torch.cat([s.new_zeros(1), s[1:]]) for s in no_hub]

    def labor(s):
        return sampler.sample_labor(s, ld)

    parts = dict(sample=(sampler.sample, seeds), labor=(labor, seeds))
    for v, name in ((1, "labor_mask_fill"), (0, "labor_rehash_fill")):
        parts[name] = (lambda s, v=v: eng.sample_labor_hops(
            s, sizes, ld, 0, v), seeds)
    for c in chunks:
        parts[f"labor_chunk_{c}"] = (lambda s, c=c: eng.sample_labor_hops(
            s, sizes, ld, c), seeds)
    parts["labor_no_hub_1k"] = (labor, no_hub)
    parts["labor_hub_1k"] = (labor, hub)
    for fn, args_list in parts.values():
        _timed(fn, args_list[:warmup], sync)
    ms = {k: [] for k in parts}
    for _ in range(repeats):
        for k, (fn, args_list) in parts.items():
            ms[k].append(_timed(fn, args_list * passes, sync))
    res = dict(mode=mode, shape=shape, labor=True, layer_dependency=ld,
               batch=batch, iters=iters, passes=passes, repeats=repeats,
               default_chunk=quiver._ext.labor_chunk_slots(),
               default_mask_fill=quiver._ext.labor_mask_fill(mode == "GPU"))
    for k, v in ms.items():
        res[k + "_ms"] = _stats(v)
    for k in ("sample", "labor", "labor_no_hub_1k", "labor_hub_1k"):
        fn, args_list = parts[k]
        outs = [fn(s) for s in args_list]
        n_id = float(np.mean([o[0].numel() for o in outs]))
        res[k + "_sizes"] = dict(
            edges_per_hop=np.mean([[a.edge_index.size(1) for a in o[2][::-1]]
                                   for o in outs], axis=0).tolist(),
            n_id=n_id, gather_bytes=n_id * ROW_BYTES)
    res["n_id_ratio"] = (res["labor_sizes"]["n_id"]
                         / res["sample_sizes"]["n_id"])
    if mode == "UVA":
        # what the mask fill reads of the pinned rows: every long row once,
        # and 8 B for every edge of the batch (a whole row is read by the
        # fill pass alone)
        degree = topo.degree.to(dev)
        slots = []
        for s in seeds:
            n_id, _, adjs = labor(s)
            rows, total = s, 0
            for adj, k in zip(adjs[::-1], sizes):
                d = degree[rows]
                total += int(d[d > k].sum()) + adj.edge_index.size(1)
                rows = n_id[:int(adj.size[0])]
            slots.append(total)
        res["host_bytes_read"] = 8 * float(np.mean(slots))
        res["host_gbps"] = res["host_bytes_read"] / (
            res["labor_ms"]["median"] * 1e-3) / 1e9
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--modes", default="UVA,GPU,CPU")
    p.add_argument("--shapes", default="products,reddit")
    p.add_argument("--batch", type=int, default=1024)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--cpu-iters", type=int, default=5)
    p.add_argument("--return-eid", action="store_true",
                   help="sample with return_eid=True (Adj.e_id filled)")
    p.add_argument("--edge-weight", action="store_true",
                   help="edge-weighted draws, fp32 weights uniform in "
                        "[0.5, 2) from a fixed seed")
    p.add_argument("--links", action="store_true",
                   help="time link-prediction batches (sample_negative, "
                        "sample_links) beside plain sample()")
    p.add_argument("--num-neg", type=int, default=1,
                   help="negatives per positive edge with --links")
    p.add_argument("--repeats", type=int, default=7,
                   help="repeats of the timed window with --links and "
                        "--temporal")
    p.add_argument("--temporal", action="store_true",
                   help="time sample_temporal (synthetic edge times, seeds "
                        "bounded at the median) beside plain sample(); with "
                        "--links also temporal sample_links")
    p.add_argument("--walk", action="store_true",
                   help="time random_walk (uniform and --p/--q walks, B = "
                        "1024 and 65536) in GPU and UVA mode, beside a "
                        "plain-torch uniform walk in GPU mode")
    p.add_argument("--p", type=float, default=0.5)
    p.add_argument("--q", type=float, default=2.0)
    p.add_argument("--walk-length", type=int, default=20)
    p.add_argument("--subgraph", action="store_true",
                   help="time subgraph (GraphSAINT random-walk sets, 100 000 "
                        "uniform nodes, a set with and without the hub row; "
                        "chunks of 64, 256 and 1024 slots) in GPU and UVA "
                        "mode, beside a plain-torch version in GPU mode")
    p.add_argument("--labor", action="store_true",
                   help="time sample_labor (either fill pass, chunks of 64, "
                        "256 and 1024 slots, a batch with and without the "
                        "hub row) beside plain sample() on the same seeds in "
                        "GPU and UVA mode, with the sizes of both methods' "
                        "batches")
    p.add_argument("--layer-dependency", action="store_true",
                   help="with --labor: one variate per node for all hops")
    args = p.parse_args()
    if args.labor:
        assert torch.cuda.is_available(), "--labor needs a GPU"
        for shape in args.shapes.split(","):
            cfg = SHAPES[shape]
            indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
            topo = quiver.CSRTopo(indptr=indptr, indices=indices)
            for mode in args.modes.split(","):
                if mode == "CPU":       # timed on the GPU only
                    continue
                print(json.dumps(bench_labor(
                    mode, shape, topo, args.layer_dependency,
                    batch=args.batch, iters=min(args.iters, 10),
                    repeats=args.repeats)), flush=True)
        sys.exit(0)
    if args.subgraph:
        assert torch.cuda.is_available(), "--subgraph needs a GPU"
        for shape in args.shapes.split(","):
            cfg = SHAPES[shape]
            indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
            topo = quiver.CSRTopo(indptr=indptr, indices=indices)
            for mode in args.modes.split(","):
                if mode == "CPU":       # timed on the GPU only
                    continue
                print(json.dumps(bench_subgraph(
                    mode, shape, topo, iters=min(args.iters, 10),
                    repeats=args.repeats)), flush=True)
        sys.exit(0)
    if args.walk:
        assert torch.cuda.is_available(), "--walk needs a GPU"
        for shape in args.shapes.split(","):
            cfg = SHAPES[shape]
            indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
            topo = quiver.CSRTopo(indptr=indptr, indices=indices)
            for mode in args.modes.split(","):
                if mode == "CPU":       # the walks are timed on the GPU
                    continue
                print(json.dumps(bench_walk(
                    mode, shape, topo, args.p, args.q,
                    length=args.walk_length, iters=min(args.iters, 20),
                    repeats=args.repeats)), flush=True)
        sys.exit(0)
    if args.temporal:
        for shape in args.shapes.split(","):
            cfg = SHAPES[shape]
            indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
            topo = quiver.CSRTopo(indptr=indptr, indices=indices)
            edge_time = make_times(indices.numel())
            for mode in args.modes.split(","):
                if mode != "CPU" and not torch.cuda.is_available():
                    continue
                iters = args.cpu_iters if mode == "CPU" else args.iters
                print(json.dumps(bench_temporal(
                    mode, shape, topo, edge_time, batch=args.batch,
                    iters=iters, repeats=args.repeats, links=args.links,
                    num_neg=args.num_neg)), flush=True)
        sys.exit(0)
    if args.links:
        for shape in args.shapes.split(","):
            cfg = SHAPES[shape]
            indptr, indices = make_graph(cfg["nodes"], cfg["edges"])
            topo = quiver.CSRTopo(indptr=indptr, indices=indices)
            for mode in args.modes.split(","):
                if mode != "CPU" and not torch.cuda.is_available():
                    continue
                iters = args.cpu_iters if mode == "CPU" else args.iters
                print(json.dumps(bench_links(
                    mode, shape, topo, batch=args.batch,
                    num_neg=args.num_neg, iters=iters,
                    repeats=args.repeats)), flush=True)
        sys.exit(0)
    for shape in args.shapes.split(","):
        for mode in args.modes.split(","):
            if mode != "CPU" and not torch.cuda.is_available():
                continue
            iters = args.cpu_iters if mode == "CPU" else args.iters
            res = bench(mode, shape, batch=args.batch, iters=iters,
                        return_eid=args.return_eid,
                        edge_weight=args.edge_weight)
            print(json.dumps(res), flush=True)
