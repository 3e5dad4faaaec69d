"""TransformerConv's torch chain in float64 on the CPU against a per-dst
loop written from the layer's definition."""
import pytest
import torch

from quiver.nn import TransformerConv

N, N_DST, IN, H, C = 30, 12, 10, 3, 4


def _loop(conv, x, edge_index):
    """out[d] from torch.softmax over the edges of d, one dst at a time."""
    src, dst = edge_index
    q = conv.lin_query(x[:N_DST]).view(-1, H, C)
    k = conv.lin_key(x).view(-1, H, C)
    v = conv.lin_value(x).view(-1, H, C)
    rows = []
    for d in range(N_DST):
        s = src[dst == d]
        alpha = torch.softmax(
            torch.einsum("hc,ehc->eh", q[d], k[s]) / C ** 0.5, dim=0)
        o = torch.einsum("eh,ehc->hc", alpha, v[s])
        o = o.reshape(-1) if conv.concat else o.mean(0)
        if conv.root_weight:
            r = conv.lin_skip(x[d])
            if conv.lin_beta is not None:
                b = torch.sigmoid(conv.lin_beta(torch.cat([o, r, o - r])))
                o = b * r + (1 - b) * o
            else:
                o = o + r
        rows.append(o)
    return torch.stack(rows)


@pytest.mark.parametrize("concat", [True, False])
@pytest.mark.parametrize("beta,root_weight",
                         [(False, False), (False, True), (True, True)])
def test_chain_matches_per_dst_loop(beta, root_weight, concat):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, IN, generator=g, dtype=torch.float64)
    # dst 0 has no edge, the others 1 to 6 in shuffled order
    dst = torch.cat([torch.arange(1, N_DST),
                     torch.randint(1, N_DST, (25,), generator=g)])
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    edge_index = torch.stack(
        [torch.randint(0, N, (dst.numel(),), generator=g), dst])
    torch.manual_seed(4)
    conv = TransformerConv(IN, C, heads=H, concat=concat, beta=beta,
                           root_weight=root_weight).double()
    out = conv((x, x[:N_DST]), edge_index, (N, N_DST))
    assert out.shape == (N_DST, H * C if concat else C)
    torch.testing.assert_close(out, _loop(conv, x, edge_index),
                               rtol=1e-12, atol=1e-12)
    assert sorted(n for n, _ in conv.named_children()) == sorted(
        ["lin_key", "lin_query", "lin_value", "lin_skip"]
        + (["lin_beta"] if beta else []))
