"""GATv2Conv's torch path against the GATv2 formula in float64 (CPU)."""
import pytest
import torch
import torch.nn.functional as F

from quiver.nn import GAT, GATv2Conv
from quiver.pyg.sage_sampler import Adj


def _formula64(conv, x_src, x_dst, src, dst):
    H, C = conv.heads, conv.out_channels
    lin = lambda m, x: F.linear(x.double(), m.weight.double(),
                                m.bias.double()).view(-1, H, C)
    xl, xr = lin(conv.lin_l, x_src), lin(conv.lin_r, x_dst)
    out = torch.zeros(x_dst.size(0), H, C, dtype=torch.float64)
    for d in range(x_dst.size(0)):
        e = (dst == d).nonzero().flatten()
        if e.numel() == 0:
            continue
        z = F.leaky_relu(xl[src[e]] + xr[d], conv.negative_slope)
        alpha = (z * conv.att.double()).sum(-1).softmax(0)     # [e, H]
        out[d] = (alpha.unsqueeze(-1) * xl[src[e]]).sum(0)
    out = out.reshape(-1, H * C) if conv.concat else out.mean(1)
    return out + conv.bias.double()


@pytest.mark.parametrize("kw", [dict(), dict(share_weights=True),
                                dict(concat=False), dict(sorted_dst=True)],
                         ids=["split", "shared", "mean", "sorted"])
def test_gatv2_conv_matches_float64_formula(kw):
    torch.manual_seed(0)
    conv = GATv2Conv(8, 64, heads=2, **kw)
    torch.nn.init.normal_(conv.bias)
    x = torch.randn(40, 8)
    n_dst = 6
    lens = torch.tensor([20, 0, 1, 7, 3, 12])
    dst = torch.repeat_interleave(torch.arange(n_dst), lens)
    src = torch.randint(0, 40, (dst.numel(),))
    out = conv((x, x[:n_dst]), torch.stack([src, dst]), (40, n_dst))
    expect = _formula64(conv, x, x[:n_dst], src, dst)
    assert out.dtype == torch.float32
    err = (out.double() - expect).abs().max() / expect.abs().max()
    assert err <= 1e-5


def test_gatv2_parameter_names():
    names = {n for n, _ in GATv2Conv(8, 4, heads=2).named_parameters()}
    assert names == {"lin_l.weight", "lin_l.bias", "lin_r.weight",
                     "lin_r.bias", "att", "bias"}
    shared = GATv2Conv(8, 4, heads=2, share_weights=True)
    assert shared.lin_r is shared.lin_l
    assert shared.att.shape == (1, 2, 4)


def test_gat_v2_model_forward_backward():
    torch.manual_seed(0)
    model = GAT(8, 8, 4, num_layers=2, heads=2, v2=True)
    assert all(isinstance(c, GATv2Conv) for c in model.convs)
    e2 = torch.stack([torch.arange(30), torch.arange(30) % 10])
    e1 = torch.stack([torch.arange(10), torch.arange(10) % 4])
    adjs = [Adj(e2, torch.tensor([]), (30, 10)),
            Adj(e1, torch.tensor([]), (10, 4))]
    out = model(torch.randn(30, 8), adjs)
    assert out.shape == (4, 4)
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
