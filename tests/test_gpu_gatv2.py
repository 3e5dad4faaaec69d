"""Fused GATv2 attention (csrc/gatv2_kernels.hip) against the formula in
float64.

Truth: `_formula` on the CPU in float64, on the inputs the kernel gets
(rounded to the kernel dtype first).  Yardstick: the same function in the
kernel's dtype.  With err = max|got - truth| / max|truth| per tensor, the
kernel must satisfy err_kernel <= 4 * err_yardstick + 16 * eps(dtype).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import quiver
from quiver import _ext
from quiver.nn import GATv2Conv, _GatV2Attn

pytestmark = pytest.mark.gpu

SLOPE = 0.2
N_SRC, N_DST, XR_ROWS = 300, 40, 43
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8}


def _formula(xl, xr, att, src, dst, n_dst, H):
    C = xl.size(1) // H
    x = xl.view(-1, H, C).index_select(0, src)
    z = F.leaky_relu(x + xr.view(-1, H, C).index_select(0, dst), SLOPE)
    logit = (z * att.view(1, H, C)).sum(-1)
    idx = dst.unsqueeze(-1).expand_as(logit)
    amax = logit.new_full((n_dst, H), float("-inf")).scatter_reduce(
        0, idx, logit.detach(), reduce="amax")
    p = (logit - amax.index_select(0, dst)).exp()
    alpha = p / p.new_zeros(n_dst, H).index_add(0, dst, p).index_select(0, dst)
    out = x.new_zeros(n_dst, H, C).index_add(0, dst, x * alpha.unsqueeze(-1))
    return out.reshape(n_dst, H * C), logit


def _formula_grads(dtype, xl, xr, att, g_out, src, dst, H):
    """(out, g_xl, g_xr, g_att, logit) of the formula evaluated in dtype."""
    xl, xr, att = (t.to(dtype, copy=True).requires_grad_()
                   for t in (xl, xr, att))
    out, logit = _formula(xl, xr, att, src, dst, N_DST, H)
    out.backward(g_out.to(dtype))
    return [t.detach().double() for t in (out, xl.grad, xr.grad, att.grad,
                                          logit)]


def _err(got, truth):
    return ((got.double().cpu() - truth).abs().max() / truth.abs().max()).item()


@functools.lru_cache(maxsize=None)
def _case(H, C, dtype, scale=1.0):
    """Inputs (CPU, rounded to dtype), float64 truth and yardstick errors."""
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(0, 21, (N_DST,), generator=g)
    lens[7] = 300  # longer than any lane group: ids are re-batched
    assert (lens == 0).any() and (lens == 1).any()
    dst = torch.repeat_interleave(torch.arange(N_DST), lens)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dtype).float()
    xl, xr = scale * rnd(N_SRC, H * C), scale * rnd(XR_ROWS, H * C)
    xl, xr = xl.to(dtype).float(), xr.to(dtype).float()
    att, g_out = rnd(H * C), rnd(N_DST, H * C)
    inputs = (xl, xr, att, g_out, src, dst)
    truth = _formula_grads(torch.float64, *inputs, H)
    yard = _formula_grads(dtype, *inputs, H)
    err_y = [_err(y, t) for y, t in zip(yard[:4], truth[:4])]
    return inputs, ptr, lens, truth, err_y


def _run_kernel(case, H, dtype, xl_grad=True):
    (xl, xr, att, g_out, src, dst), ptr, _, _, _ = case
    xl = xl.to("cuda", dtype).requires_grad_(xl_grad)
    xr = xr.to("cuda", dtype).requires_grad_()
    att = att.cuda().requires_grad_()
    out = _GatV2Attn.apply(xl, xr, att, src.cuda(), ptr.cuda(), H, SLOPE)
    out.backward(g_out.to("cuda", dtype))
    return out.detach(), xl.grad, xr.grad, att.grad


def _check_bound(got, case, dtype, names=("out", "g_xl", "g_xr", "g_att")):
    truth, err_y = case[3], case[4]
    for i, name in enumerate(("out", "g_xl", "g_xr", "g_att")):
        if name not in names:
            continue
        assert torch.isfinite(got[i]).all(), name
        err_k = _err(got[i], truth[i])
        print(f"{name}: err_kernel={err_k:.3e} err_yardstick={err_y[i]:.3e} "
              f"ratio={err_k / max(err_y[i], 1e-30):.2f}")
        assert err_k <= 4 * err_y[i] + 16 * EPS[dtype], name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,C", [(1, 4), (3, 12), (4, 64), (8, 64), (1, 256)])
def test_gatv2_attn_matches_fp64(H, C, dtype):
    case = _case(H, C, dtype)
    lens = case[2]
    got = _run_kernel(case, H, dtype)
    _check_bound(got, case, dtype)
    assert got[2].shape == (XR_ROWS, H * C)
    assert (got[2][N_DST:] == 0).all()          # no gradient past n_dst
    assert (got[0][(lens == 0).cuda()] == 0).all()  # empty segments


def test_gatv2_attn_large_logits():
    case = _case(4, 64, torch.float32, 1.7)
    assert case[3][4].abs().max() >= 50  # the truth's logits
    _check_bound(_run_kernel(case, 4, torch.float32), case, torch.float32)


def test_gatv2_attn_need_flags():
    case = _case(4, 64, torch.float32)
    full = _run_kernel(case, 4, torch.float32)
    part = _run_kernel(case, 4, torch.float32, xl_grad=False)
    assert part[1] is None
    assert torch.equal(part[2], full[2])
    # g_att is summed by atomics: order-dependent, held to the bound
    _check_bound(part, case, torch.float32, names=("g_att",))


@pytest.mark.parametrize("kw", [dict(share_weights=False),
                                dict(share_weights=True),
                                dict(concat=False),
                                dict(dropout=0.5)],
                         ids=["split", "shared", "mean", "dropout"])
def test_gatv2_conv_routing(small_graph, kw):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    sampler = quiver.GraphSageSampler(topo, [5], device=0, mode="GPU")
    n_id, _, adjs = sampler.sample(torch.arange(64))
    edge_index, _, size = adjs[0]
    torch.manual_seed(0)
    x0 = torch.randn(n_id.numel(), 32)

    def run(sorted_dst, device, dtype):
        torch.manual_seed(1)
        conv = GATv2Conv(32, 16, heads=2, sorted_dst=sorted_dst, **kw)
        conv = conv.to(device, dtype)
        x = x0.to(device, dtype).requires_grad_()
        ei = edge_index if sorted_dst else edge_index.clone().to(device)
        out = conv((x, x[:size[1]]), ei, size)
        out.square().sum().backward()
        return [out.detach(), x.grad] + [p.grad for p in conv.parameters()]

    fused = run(True, "cuda", torch.float32)
    if kw.get("dropout"):
        # training-mode attention dropout takes the torch chain
        assert all(torch.isfinite(t).all() for t in fused)
        return
    truth = [t.double() for t in run(False, "cpu", torch.float64)]
    chain = run(False, "cuda", torch.float32)
    assert len(fused) == len(truth) == len(chain)
    for f, c, t in zip(fused, chain, truth):
        assert _err(f, t) <= 4 * _err(c, t) + 16 * EPS[torch.float32]


def _zero_segment_args():
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    return dict(xl=z(3, 8), xr=z(0, 8), att=z(8), go=z(0, 8), out=z(0, 8),
                lse=z(0, 2), src=z(0, dtype=torch.int64),
                ptr=z(1, dtype=torch.int64), heads=2)


_CALLS = {
    "fwd": lambda a: _ext.gatv2_attn(a["xl"], a["xr"], a["att"], a["src"],
                                     a["ptr"], a["heads"], SLOPE),
    "bwd": lambda a: _ext.gatv2_attn_backward(
        a["go"], a["xl"], a["xr"], a["att"], a["out"], a["lse"], a["src"],
        a["ptr"], a["heads"], SLOPE, True, True, True),
}
_BREAK = {
    "src_on_cpu": lambda a: a.update(src=a["src"].cpu()),
    "dst_ptr_on_cpu": lambda a: a.update(ptr=a["ptr"].cpu()),
    "dst_ptr_empty": lambda a: a.update(ptr=a["ptr"][:0]),
    "att_length": lambda a: a.update(att=a["att"][:4]),
    "lse_shape": lambda a: a.update(lse=a["lse"].new_zeros(0, 3)),
    "grad_out_dtype": lambda a: a.update(go=a["go"].bfloat16()),
    # 6 channels per head
    "chead_not_multiple_of_4": lambda a: a.update(
        xl=a["xl"].new_zeros(3, 12), xr=a["xr"].new_zeros(0, 12),
        att=a["att"].new_zeros(12), go=a["go"].new_zeros(0, 12),
        out=a["out"].new_zeros(0, 12)),
    "dim_above_1024": lambda a: a.update(
        xl=a["xl"].new_zeros(3, 1032), xr=a["xr"].new_zeros(0, 1032),
        att=a["att"].new_zeros(1032), go=a["go"].new_zeros(0, 1032),
        out=a["out"].new_zeros(0, 1032)),
}
_BAD_ARGS = [(op, fault) for fault in _BREAK for op in _CALLS
             if not (op == "fwd" and fault in ("lse_shape", "grad_out_dtype"))]


@pytest.mark.parametrize("op,fault", _BAD_ARGS,
                         ids=[f"{op}-{fault}" for op, fault in _BAD_ARGS])
def test_gatv2_bad_arguments_raise(op, fault):
    args = _zero_segment_args()
    _CALLS[op](args)  # the well-formed call goes through
    _BREAK[fault](args)
    with pytest.raises(RuntimeError):
        _CALLS[op](args)
