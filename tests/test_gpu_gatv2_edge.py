"""Edge features in the fused GATv2 kernels against the formula in float64,
by the rule of tests/test_gpu_gatv2.py: truth in float64 on inputs rounded
to the kernel dtype, yardstick the same function in that dtype, err =
max|got - truth| / max|truth|, err_kernel <= 4 * err_yardstick + 16 * eps.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import quiver
from quiver import _ext
from quiver.nn import GATv2Conv, _GatV2Attn, _GatV2AttnEdge

pytestmark = pytest.mark.gpu

SLOPE = 0.2
N_SRC, N_DST, XR_ROWS, TABLE_ROWS = 300, 40, 43, 500
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8}
NAMES = ("out", "g_xl", "g_xr", "g_att", "g_w")


def _formula_grads(dtype, xl, xr, att, ea, w, g_out, src, dst, H):
    xl, xr, att, w = (t.to(dtype, copy=True).requires_grad_()
                      for t in (xl, xr, att, w))
    C = xl.size(1) // H
    x = xl.view(-1, H, C).index_select(0, src)
    z = F.leaky_relu(x + xr.view(-1, H, C).index_select(0, dst)
                     + (ea.to(dtype) @ w.t()).view(-1, H, C), SLOPE)
    logit = (z * att.view(1, H, C)).sum(-1)
    idx = dst.unsqueeze(-1).expand_as(logit)
    amax = logit.new_full((N_DST, H), float("-inf")).scatter_reduce(
        0, idx, logit.detach(), reduce="amax")
    p = (logit - amax.index_select(0, dst)).exp()
    alpha = p / p.new_zeros(N_DST, H).index_add(0, dst, p).index_select(0, dst)
    out = x.new_zeros(N_DST, H, C).index_add(0, dst, x * alpha.unsqueeze(-1))
    out = out.reshape(N_DST, H * C)
    out.backward(g_out.to(dtype))
    return [t.detach().double() for t in (out, xl.grad, xr.grad, att.grad,
                                          w.grad)]


def _err(got, truth):
    return ((got.double().cpu() - truth).abs().max() / truth.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _case(H, C, D, dtype, with_id):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 21, (N_DST,), generator=g)
    lens[7] = 300  # longer than any lane group: ids are re-batched
    assert (lens == 0).any() and (lens == 1).any()
    dst = torch.repeat_interleave(torch.arange(N_DST), lens)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).float()
    xl, xr, att = rnd(N_SRC, H * C), rnd(XR_ROWS, H * C), rnd(H * C)
    g_out = rnd(N_DST, H * C)
    w = (rnd(H * C, D) / D ** 0.5).to(dtype).float()
    if with_id:
        # rows no id selects are NaN: reading one poisons the output
        eid = torch.randint(0, TABLE_ROWS, (dst.numel(),), generator=g)
        table = torch.full((TABLE_ROWS, D), float("nan"))
        table[eid] = rnd(dst.numel(), D)
        assert table.isnan().any()
        ea = table[eid]
    else:
        eid, table = None, rnd(dst.numel(), D)
        ea = table
    inputs = (xl, xr, att, ea, w, g_out, src, dst)
    truth = _formula_grads(torch.float64, *inputs, H)
    err_y = [_err(y, t)
             for y, t in zip(_formula_grads(dtype, *inputs, H), truth)]
    return inputs, (table, eid, ptr, lens), truth, err_y


def _run_kernel(case, H, dtype, w=None):
    (xl, xr, att, _, w0, g_out, src, _), (table, eid, ptr, _) = case[:2]
    xl, xr = (t.to("cuda", dtype).requires_grad_() for t in (xl, xr))
    att, w = (t.cuda().requires_grad_()
              for t in (att, w0 if w is None else w))
    out = _GatV2AttnEdge.apply(
        xl, xr, att, table.to("cuda", dtype),
        None if eid is None else eid.cuda(), w, src.cuda(), ptr.cuda(), H,
        SLOPE)
    out.backward(g_out.to("cuda", dtype))
    return out.detach(), xl.grad, xr.grad, att.grad, w.grad


@pytest.mark.parametrize("with_id", [False, True], ids=["rows", "edge_id"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,C,D", [(1, 4, 1), (3, 12, 5), (4, 64, 16),
                                   (8, 64, 16), (1, 256, 32)])
def test_gatv2_attn_edge_matches_fp64(H, C, D, dtype, with_id):
    case = _case(H, C, D, dtype, with_id)
    lens, truth, err_y = case[1][3], case[2], case[3]
    got = _run_kernel(case, H, dtype)
    for i, name in enumerate(NAMES):
        assert torch.isfinite(got[i]).all(), name
        err_k = _err(got[i], truth[i])
        print(f"{name}: err_kernel={err_k:.3e} err_yardstick={err_y[i]:.3e} "
              f"ratio={err_k / max(err_y[i], 1e-30):.2f}")
        assert err_k <= 4 * err_y[i] + 16 * EPS[dtype], name
    assert got[2].shape == (XR_ROWS, H * C) and got[4].shape == (H * C, D)
    assert (got[2][N_DST:] == 0).all()          # no gradient past n_dst
    assert (got[0][(lens == 0).cuda()] == 0).all()  # empty segments


def test_gatv2_attn_edge_term_is_there():
    dtype = torch.float32
    case = _case(4, 64, 16, dtype, False)
    (xl, xr, att, _, w, _, src, _), (_, _, ptr, _) = case[:2]
    plain = _GatV2Attn.apply(xl.cuda(), xr.cuda(), att.cuda(), src.cuda(),
                             ptr.cuda(), 4, SLOPE).double().cpu()
    with_edge = _run_kernel(case, 4, dtype)[0]
    zero_w = _run_kernel(case, 4, dtype, w=torch.zeros_like(w))[0]
    bound = 4 * case[3][0] + 16 * EPS[dtype]
    assert _err(with_edge, plain) > bound and _err(zero_w, plain) <= bound


@pytest.mark.parametrize("edge_dim", [8, 300], ids=["fused", "above_cap"])
def test_gatv2_conv_edge_routing(small_graph, edge_dim):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    sampler = quiver.GraphSageSampler(topo, [5], device=0, mode="GPU",
                                      return_eid=True)
    n_id, _, adjs = sampler.sample(torch.arange(64))
    edge_index, e_id, size = adjs[0]
    torch.manual_seed(0)
    x0 = torch.randn(n_id.numel(), 32)
    table = torch.randn(indices.numel(), edge_dim)

    def run(sorted_dst, device, dtype):
        torch.manual_seed(1)
        conv = GATv2Conv(32, 16, heads=2, sorted_dst=sorted_dst,
                         edge_dim=edge_dim).to(device, dtype)
        x = x0.to(device, dtype).requires_grad_()
        ei = edge_index if sorted_dst else edge_index.clone().to(device)
        out = conv((x, x[:size[1]]), ei, size,
                   edge_attr=table.to(device, dtype), edge_id=e_id.to(device))
        out.square().sum().backward()
        assert conv.lin_edge.weight.grad is not None
        return [out.detach(), x.grad] + [p.grad for p in conv.parameters()]

    fused = run(True, "cuda", torch.float32)
    if edge_dim * 2 * 16 > 8192:
        # above the LDS cap of the kernels: the torch chain serves it
        assert all(torch.isfinite(t).all() for t in fused)
        return
    truth = [t.double() for t in run(False, "cpu", torch.float64)]
    chain = run(False, "cuda", torch.float32)
    for f, c, t in zip(fused, chain, truth, strict=True):
        assert _err(f, t) <= 4 * _err(c, t) + 16 * EPS[torch.float32]


_CALLS = {
    "fwd": lambda a: _ext.gatv2_attn_edge(
        a["xl"], a["xr"], a["att"], a["ea"], a["eid"], a["w"], a["src"],
        a["ptr"], 2, SLOPE),
    "bwd": lambda a: _ext.gatv2_attn_edge_backward(
        a["go"], a["xl"], a["xr"], a["att"], a["ea"], a["eid"], a["w"],
        a["out"], a["lse"], a["src"], a["ptr"], 2, SLOPE, True, True, True,
        True),
}
_BREAK = {
    "edge_attr_1d": lambda a: dict(ea=a["ea"][:, 0]),
    "edge_attr_strided": lambda a: dict(ea=a["ea"].new_zeros(5, 6)[:, ::2]),
    "edge_attr_dtype": lambda a: dict(ea=a["ea"].bfloat16()),
    "edge_attr_on_cpu": lambda a: dict(ea=a["ea"].cpu()),
    # 4 edges, 3 rows, no edge_id
    "edge_attr_rows": lambda a: dict(ea=a["ea"][:3], src=a["src"].new_zeros(4)),
    "edge_id_dtype": lambda a: dict(eid=a["src"].int()),
    "edge_id_length": lambda a: dict(eid=a["src"].new_zeros(2)),
    "edge_id_on_cpu": lambda a: dict(eid=a["src"].cpu()),
    "w_edge_shape": lambda a: dict(w=a["w"].new_zeros(8, 3)),
    "w_edge_dtype": lambda a: dict(w=a["w"].bfloat16()),
    # 1025 * 8 > 8192
    "above_cap": lambda a: dict(ea=a["ea"].new_zeros(5, 1025),
                                w=a["w"].new_zeros(1025, 8)),
}


@pytest.mark.parametrize("fault", list(_BREAK))
@pytest.mark.parametrize("op", list(_CALLS))
def test_gatv2_edge_bad_arguments_raise(op, fault):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    args = dict(xl=z(3, 8), xr=z(0, 8), att=z(8), ea=z(5, 3), eid=None,
                w=z(3, 8), go=z(0, 8), out=z(0, 8), lse=z(0, 2),
                src=z(0, dtype=torch.int64), ptr=z(1, dtype=torch.int64))
    _CALLS[op](args)  # the well-formed zero-segment call goes through
    args.update(_BREAK[fault](args))
    with pytest.raises(RuntimeError):
        _CALLS[op](args)
