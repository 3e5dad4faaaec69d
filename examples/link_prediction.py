#!/usr/bin/env python3
"""Link prediction with GraphSAGE: positives from the graph, negatives
drawn next to the CSR by the sampler (GraphSageSampler.sample_links), a
dot-product decoder and binary cross-entropy over edge_label.

Synthetic symmetrised graph with planted communities, so there is
something to learn; swap in real data by loading your own edge_index and
features.  The default size is small enough for --mode CPU.

--temporal gives every edge a synthetic time and trains on each positive
with only the edges that existed before it: its endpoints and negatives
root one tree each (sample_links(..., edge_label_time=t - 1)), so no
message crosses an edge from the positive's future, nor the positive
itself."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

import quiver
from quiver.nn import GraphSAGE


class Encoder(GraphSAGE):
    """GraphSAGE that returns the last layer's embeddings as they are (the
    classifier's log_softmax has no place in front of a dot product)."""

    def forward(self, x, adjs):
        for i, (edge_index, _, size) in enumerate(adjs):
            x = self.convs[i]((x, x[:size[1]]), edge_index, size)
            if i != self.num_layers - 1:
                x = F.relu(x)
        return x


def community_graph(nodes, degree, groups, gen):
    """Symmetrised COO graph: most edges stay inside a node's group."""
    src = torch.arange(nodes).repeat_interleave(degree)
    group = src % groups
    inside = torch.rand(src.numel(), generator=gen) < 0.9
    peer = torch.randint(0, nodes // groups, (src.numel(),), generator=gen)
    dst = torch.where(inside, peer * groups + group,
                      torch.randint(0, nodes, (src.numel(),), generator=gen))
    keep = src != dst
    src, dst = src[keep], dst[keep]
    return torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", default="CPU", choices=["CPU", "GPU", "UVA"])
    p.add_argument("--nodes", type=int, default=2000)
    p.add_argument("--degree", type=int, default=8)
    p.add_argument("--dim", type=int, default=32)
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--num-neg", type=int, default=2)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--temporal", action="store_true",
                   help="synthetic edge times; sample each positive's "
                        "message graph from the edges before it")
    args = p.parse_args()

    gen = torch.Generator().manual_seed(0)
    groups = 10
    edge_index = community_graph(args.nodes, args.degree, groups, gen)
    topo = quiver.CSRTopo(edge_index, node_count=args.nodes)
    x_cpu = torch.randn(args.nodes, args.dim, generator=gen)
    x_cpu[:, :groups] += 2 * F.one_hot(torch.arange(args.nodes) % groups,
                                       groups)

    dev = "cpu" if args.mode == "CPU" else "cuda:0"
    edge_time = None
    if args.temporal:
        # an edge and its reverse happen at the same moment
        half = edge_index.shape[1] // 2
        t = torch.randint(0, 1 << 20, (half,), generator=gen)
        edge_time = torch.cat([t, t])
    sampler = quiver.GraphSageSampler(topo, [10, 5], device=0, mode=args.mode,
                                      edge_time=edge_time)
    if args.mode == "CPU":
        feature = x_cpu
    else:
        feature = quiver.Feature(0, device_list=[0], device_cache_size="64M",
                                 cache_policy="device_replicate",
                                 csr_topo=topo)
        feature.from_cpu_tensor(x_cpu)

    model = Encoder(args.dim, 64, 32, num_layers=2).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)

    t0 = time.perf_counter()
    for step in range(args.steps):
        at = torch.randint(0, edge_index.shape[1], (args.batch,),
                           generator=gen)
        if args.temporal:
            # t - 1: the bound is inclusive, and the positive (and its
            # reverse) must stay out of its own message graph
            batch = sampler.sample_links(edge_index[:, at],
                                         num_neg=args.num_neg,
                                         edge_label_time=edge_time[at] - 1)
        else:
            batch = sampler.sample_links(edge_index[:, at],
                                         num_neg=args.num_neg)
        z = model(feature[batch.n_id], [adj.to(dev) for adj in batch.adjs])
        head, tail = batch.edge_label_index
        logit = (z[head] * z[tail]).sum(-1)
        # a negative whose draws were all rejected may be a real edge
        keep = torch.ones_like(batch.edge_label, dtype=torch.bool)
        keep[args.batch:] = batch.neg_ok
        loss = F.binary_cross_entropy_with_logits(logit[keep],
                                                  batch.edge_label[keep])
        opt.zero_grad()
        loss.backward()
        opt.step()
        print(f"step {step}: loss={float(loss):.4f} "
              f"seeds={batch.batch_size} frontier={batch.n_id.numel()}",
              flush=True)
    if args.mode != "CPU":
        torch.cuda.synchronize()
    print(f"{args.steps} steps in {time.perf_counter() - t0:.2f}s")


if __name__ == "__main__":
    main()
