#!/usr/bin/env python3
"""One GATv2Conv (or TransformerConv) layer, fused kernels against the
layer's torch chain.

Shapes: the hidden layers of `bench.py --model gat` on products (heads 4,
64 channels per head, 256 input channels) at synthetic frontier sizes for
batch 1024 and fanouts 15 / 10 / 5: every dst has exactly `fanout` edges
with uniformly random sources, dst-sorted, segment pointer attached as the
sampler does.  The layer follows GAT(v2=True): x_dst = x[:n_dst], separate
lin_l / lin_r.

Method: device events around `iters` back-to-back calls, iters sized so a
window lasts >= 0.5 s, after warming every (path, mode) pair; three rounds
alternating fused and chain, median reported.  Peak memory is the
allocator's peak over one fwd+bwd minus what was allocated before it.
Both paths get the same parameters and inputs; their outputs are compared.

--edge-dim D gives both layers edge_dim=D and a random [E, D] edge_attr in
the row dtype (one row per edge); --shapes picks rows of SHAPES by index.
--layer transformer measures TransformerConv (beta=False, root_weight=True,
PyG's defaults) the same way; it takes no edge features.

  python benchmarks/bench_gatv2.py [--layer gatv2|transformer] [--md FILE]
                                   [--edge-dim D] [--shapes I..]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quiver.nn import GATv2Conv, TransformerConv  # noqa: E402
from quiver.pyg.sage_sampler import DST_PTR_ATTR  # noqa: E402

H, C, IN = 4, 64, 256
# (n_dst, fanout, n_src): inner, middle and outer hop of a 1024-seed batch
SHAPES = [(1024, 15, 15000), (15000, 10, 140000), (140000, 5, 600000)]


def make_inputs(n_dst, fanout, n_src, dtype):
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, n_src, (n_dst * fanout,), generator=g)
    dst = torch.arange(n_dst).repeat_interleave(fanout)
    ei = torch.stack([src, dst]).cuda()
    setattr(ei, DST_PTR_ATTR, (torch.arange(n_dst + 1) * fanout).cuda())
    x = torch.randn(n_src, IN, generator=g).to("cuda", dtype)
    return x.requires_grad_(), ei


def make_step(conv, x, ei, n_dst, backward, fw):
    size = (x.size(0), n_dst)

    def step():
        out = conv((x, x[:n_dst]), ei, size, **fw)
        if backward:
            x.grad = None
            conv.zero_grad(set_to_none=True)
            out.backward(torch.ones_like(out))
        return out
    return step


def time_ms(step, iters):
    beg, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    beg.record()
    for _ in range(iters):
        step()
    end.record()
    torch.cuda.synchronize()
    return beg.elapsed_time(end) / iters


def peak_mib(step):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--md", help="also write the table to this file")
    ap.add_argument("--edge-dim", type=int, default=None,
                    help="edge feature width (default: no edge features)")
    ap.add_argument("--shapes", type=int, nargs="+",
                    default=list(range(len(SHAPES))),
                    help="indices into SHAPES (default: all)")
    ap.add_argument("--layer", choices=["gatv2", "transformer"],
                    default="gatv2", help="which layer to measure")
    args = ap.parse_args()
    kw = {} if args.edge_dim is None else dict(edge_dim=args.edge_dim)
    layer = GATv2Conv if args.layer == "gatv2" else TransformerConv
    assert layer is GATv2Conv or not kw, "TransformerConv has no edge_dim"
    assert torch.cuda.is_available(), "bench_gatv2 needs a GPU"
    lines = ["| dtype | n_dst | fanout | n_src | mode | fused ms | chain ms |"
             " speedup | fused peak MiB | chain peak MiB |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for dtype in (torch.float32, torch.bfloat16):
        for n_dst, fanout, n_src in (SHAPES[i] for i in args.shapes):
            x, ei = make_inputs(n_dst, fanout, n_src, dtype)
            ea = None
            if args.edge_dim is not None:
                ea = torch.randn(ei.size(1), args.edge_dim,
                                 generator=torch.Generator().manual_seed(1)
                                 ).to("cuda", dtype)
            torch.manual_seed(0)
            fw = {} if ea is None else dict(edge_attr=ea)
            convs = {"fused": layer(IN, C, heads=H, sorted_dst=True, **kw),
                     "chain": layer(IN, C, heads=H, sorted_dst=False, **kw)}
            convs["chain"].load_state_dict(convs["fused"].state_dict())
            for c in convs.values():
                c.to("cuda", dtype)
            with torch.no_grad():
                a, b = (convs[k]((x, x[:n_dst]), ei, (n_src, n_dst),
                                 **fw).float()
                        for k in ("fused", "chain"))
                diff = ((a - b).abs().max() / b.abs().max()).item()
            del a, b
            for backward in (False, True):
                steps = {k: make_step(c, x, ei, n_dst, backward, fw)
                         for k, c in convs.items()}
                iters = {}
                for k, s in steps.items():
                    for _ in range(3):
                        s()
                    iters[k] = int(min(500, max(5, 500.0 / time_ms(s, 3))))
                ms = {k: [] for k in steps}
                for _ in range(3):
                    for k, s in steps.items():
                        ms[k].append(time_ms(s, iters[k]))
                med = {k: statistics.median(v) for k, v in ms.items()}
                peak = {k: peak_mib(s) for k, s in steps.items()}
                rec = dict(dtype=str(dtype).split(".")[-1], n_dst=n_dst,
                           fanout=fanout, n_src=n_src,
                           mode="fwd+bwd" if backward else "fwd",
                           fused_ms=med["fused"], chain_ms=med["chain"],
                           fused_ms_rounds=ms["fused"],
                           chain_ms_rounds=ms["chain"],
                           fused_peak_mib=peak["fused"],
                           chain_peak_mib=peak["chain"],
                           out_rel_diff=diff)
                print(json.dumps(rec), flush=True)
                lines.append(
                    f"| {rec['dtype']} | {n_dst} | {fanout} | {n_src} | "
                    f"{rec['mode']} | {med['fused']:.3f} | {med['chain']:.3f}"
                    f" | {med['chain'] / med['fused']:.2f}x | "
                    f"{peak['fused']:.0f} | {peak['chain']:.0f} |")
            del x, ei, ea, convs, steps
            torch.cuda.empty_cache()
    table = "\n".join(lines)
    print(table)
    if args.md:
        with open(args.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
