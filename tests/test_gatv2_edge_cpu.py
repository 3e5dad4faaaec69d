"""GATv2Conv with edge_dim: the torch path against the formula in float64
(CPU), argument checks and the GAT model plumbing."""
import pytest
import torch
import torch.nn.functional as F

from quiver.nn import GAT, GATv2Conv
from quiver.pyg.sage_sampler import Adj

LENS = torch.tensor([20, 0, 1, 7, 3, 12])      # 43 edges over 6 targets
N_DST, N_SRC = LENS.numel(), 40


def _call(conv, edge_attr=None, edge_id=None):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N_SRC, 8, generator=g)
    dst = torch.repeat_interleave(torch.arange(N_DST), LENS)
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    out = conv((x, x[:N_DST]), torch.stack([src, dst]), (N_SRC, N_DST),
               edge_attr=edge_attr, edge_id=edge_id)
    return out, x, src, dst


@pytest.mark.parametrize("with_id", [False, True], ids=["rows", "edge_id"])
@pytest.mark.parametrize("kw", [dict(), dict(concat=False),
                                dict(sorted_dst=True)],
                         ids=["split", "mean", "sorted"])
def test_gatv2_conv_edge_matches_float64_formula(kw, with_id):
    torch.manual_seed(0)
    conv = GATv2Conv(8, 64, heads=2, edge_dim=3, **kw)
    torch.nn.init.normal_(conv.bias)
    H, C = conv.heads, conv.out_channels
    table = torch.randn(100 if with_id else 43, 3)
    eid = torch.randint(0, 100, (43,)) if with_id else None
    out, x, src, dst = _call(conv, table, eid)
    lin = lambda m, t: F.linear(
        t.double(), m.weight.double(),
        None if m.bias is None else m.bias.double()).view(-1, H, C)
    xl, xr = lin(conv.lin_l, x), lin(conv.lin_r, x[:N_DST])
    pe = lin(conv.lin_edge, table[eid] if with_id else table)
    expect = torch.zeros(N_DST, H, C, dtype=torch.float64)
    for d in range(N_DST):
        e = (dst == d).nonzero().flatten()
        if e.numel():
            z = F.leaky_relu(xl[src[e]] + xr[d] + pe[e], conv.negative_slope)
            alpha = (z * conv.att.double()).sum(-1).softmax(0)     # [e, H]
            expect[d] = (alpha.unsqueeze(-1) * xl[src[e]]).sum(0)
    expect = expect.reshape(-1, H * C) if conv.concat else expect.mean(1)
    expect = expect + conv.bias.double()
    assert out.dtype == torch.float32
    assert (out.double() - expect).abs().max() / expect.abs().max() <= 1e-5


@pytest.mark.parametrize("edge_dim,attr_shape,id_len", [
    (None, (43, 3), None),   # edge_attr without edge_dim
    (3, (43, 4), None),      # width other than edge_dim
    (3, (42, 3), None),      # not one row per edge, no edge_id
    (3, None, 43),           # edge_id without edge_attr
], ids=["no_edge_dim", "width", "rows", "id_alone"])
def test_gatv2_conv_edge_bad_arguments(edge_dim, attr_shape, id_len):
    conv = GATv2Conv(8, 4, heads=2, edge_dim=edge_dim)
    ea = None if attr_shape is None else torch.randn(attr_shape)
    eid = None if id_len is None else torch.zeros(id_len, dtype=torch.int64)
    with pytest.raises(ValueError):
        _call(conv, ea, eid)


def test_gat_v2_edge_model_forward_backward():
    params = dict(GATv2Conv(8, 4, heads=2, edge_dim=3).named_parameters())
    assert params["lin_edge.weight"].shape == (8, 3)
    assert "lin_edge.bias" not in params
    plain = dict(GATv2Conv(8, 4, heads=2).named_parameters())
    assert not any(n.startswith("lin_edge") for n in plain)
    torch.manual_seed(0)
    model = GAT(8, 8, 4, num_layers=2, heads=2, v2=True, edge_dim=3)
    e2 = torch.stack([torch.arange(30), torch.arange(30) % 10])
    e1 = torch.stack([torch.arange(10), torch.arange(10) % 4])
    table = torch.randn(50, 3)
    adjs = [Adj(e2, torch.randint(0, 50, (30,)), (30, 10)),
            Adj(e1, torch.randint(0, 50, (10,)), (10, 4))]
    x = torch.randn(30, 8)
    out = model(x, adjs, edge_attr=table)
    assert out.shape == (4, 4)
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in model.parameters())
    # e_id left empty (a sampler without return_eid) is an error that says so
    with pytest.raises(ValueError, match="return_eid"):
        model(x, [Adj(e2, torch.tensor([]), (30, 10)), adjs[1]],
              edge_attr=table)
    with pytest.raises(ValueError):
        GAT(8, 8, 4, v2=False, edge_dim=3)
