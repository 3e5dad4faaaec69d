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
    args = p.parse_args()
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
