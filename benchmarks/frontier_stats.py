#!/usr/bin/env python3
"""Rows gathered per step and their cold share on a bench.py preset.

Uses bench.py's own generators, constants and seed streams (graph, train
ids, batches), samples the first batches and counts how many frontier
rows fall past the hot cache, and how many of a batch's cold rows were
already cold rows of the previous batches (--window).  One JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import quiver  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--preset", default="products",
                   choices=sorted(bench.PRESETS))
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--batches", type=int, default=33)
    p.add_argument("--window", type=int, default=2,
                   help="previous batches whose cold rows count as repeats")
    args = p.parse_args()

    ps = bench.PRESETS[args.preset]
    indptr, indices, _ = bench.make_graph(seed=0, nodes=ps["nodes"],
                                          edges=ps["edges"])
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    sampler = quiver.GraphSageSampler(topo, bench.FANOUT, device=0,
                                      mode=ps["mode"])
    # same placement as bench.py; the row values do not matter here
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    feat = torch.zeros(ps["nodes"], ps["feat_dim"], dtype=dtype)
    feature = quiver.Feature(0, device_list=[0],
                             device_cache_size=ps["cache"],
                             cache_policy="device_replicate", csr_topo=topo)
    feature.from_cpu_tensor(feat)
    row_bytes = ps["feat_dim"] * feat.element_size()
    hot_rows = feature._shard_tensor().shard_tensor.shard_rows()[0]

    tg = torch.Generator().manual_seed(42)
    train_idx = torch.randint(0, ps["nodes"], (ps["train"],), generator=tg)
    sg = torch.Generator().manual_seed(1234)
    rows = cold = 0
    # repeat shares: of a batch's cold rows, how many were also cold rows
    # of batch B-1, of batch B-2, of any of the previous W batches.  Only
    # batches with a full window behind them are counted.
    W = args.window
    prev = []                      # sorted cold rows of the last W batches
    rep = {"b1": 0, "b2": 0, "win": 0}
    rep_cold = {"b1": 0, "b2": 0, "win": 0}

    def shared(a, b):
        return int(torch.isin(a, b, assume_unique=True).sum())

    for _ in range(args.batches):
        seeds = train_idx[torch.randint(0, ps["train"], (bench.BATCH,),
                                        generator=sg)]
        n_id, _, _ = sampler.sample(seeds)
        rows += n_id.numel()
        r = feature.feature_order[n_id]
        c = r[r >= hot_rows]
        cold += c.numel()
        if len(prev) >= 1:
            rep["b1"] += shared(c, prev[-1])
            rep_cold["b1"] += c.numel()
        if len(prev) >= 2:
            rep["b2"] += shared(c, prev[-2])
            rep_cold["b2"] += c.numel()
        if W >= 1 and len(prev) >= W:
            rep["win"] += shared(c, torch.cat(prev[-W:]).unique())
            rep_cold["win"] += c.numel()
        prev = (prev + [c])[-max(W, 2):]

    def share(k):
        return rep[k] / rep_cold[k] if rep_cold[k] else None

    print(json.dumps({
        "preset": args.preset, "dtype": args.dtype, "batches": args.batches,
        "rows_per_step": rows / args.batches, "cold_share": cold / rows,
        "row_bytes": row_bytes,
        "cold_MB_per_step": cold / args.batches * row_bytes / 1e6,
        "window": W,
        "repeat_share_b1": share("b1"), "repeat_share_b2": share("b2"),
        "repeat_share_window": share("win"),
    }), flush=True)


if __name__ == "__main__":
    main()
