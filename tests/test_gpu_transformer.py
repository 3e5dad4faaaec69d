"""Fused dot-product attention (csrc/transformer_kernels.hip) against the
formula in float64.

Truth: `_formula` on the CPU in float64, on the inputs the kernel gets
(rounded to the kernel dtype first).  Yardstick: the same function in the
kernel's dtype.  With err = max|got - truth| / max|truth| per tensor, the
kernel must satisfy err_kernel <= 4 * err_yardstick + 16 * eps(dtype).
"""
import functools

import pytest
import torch

import quiver
from quiver import _ext
from quiver.nn import TransformerConv, _TConvAttn

pytestmark = pytest.mark.gpu

N_SRC, N_DST, Q_ROWS = 300, 40, 43
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -8}
NAMES = ("out", "g_q", "g_kv", "g_k", "g_v")


def _formula(q, kv, src, dst, n_dst, H):
    HC = q.size(1)
    C = HC // H
    k = kv[:, :HC].reshape(-1, H, C).index_select(0, src)
    v = kv[:, HC:].reshape(-1, H, C).index_select(0, src)
    logit = (q.view(-1, H, C).index_select(0, dst) * k).sum(-1) / C ** 0.5
    idx = dst.unsqueeze(-1).expand_as(logit)
    amax = logit.new_full((n_dst, H), float("-inf")).scatter_reduce(
        0, idx, logit.detach(), reduce="amax")
    p = (logit - amax.index_select(0, dst)).exp()
    alpha = p / p.new_zeros(n_dst, H).index_add(0, dst, p).index_select(0, dst)
    out = v.new_zeros(n_dst, H, C).index_add(0, dst, v * alpha.unsqueeze(-1))
    return out.reshape(n_dst, HC), logit


def _with_halves(out, g_q, g_kv):
    half = g_kv.size(1) // 2
    return [out, g_q, g_kv, g_kv[:, :half], g_kv[:, half:]]


def _formula_grads(dtype, q, kv, g_out, src, dst, H):
    """NAMES of the formula evaluated in dtype, then its logits."""
    q, kv = (t.to(dtype, copy=True).requires_grad_() for t in (q, kv))
    out, logit = _formula(q, kv, src, dst, N_DST, H)
    out.backward(g_out.to(dtype))
    return [t.detach().double()
            for t in _with_halves(out, q.grad, kv.grad) + [logit]]


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
    q, kv = scale * rnd(Q_ROWS, H * C), scale * rnd(N_SRC, 2 * H * C)
    q, kv = q.to(dtype).float(), kv.to(dtype).float()
    inputs = (q, kv, rnd(N_DST, H * C), src, dst)
    truth = _formula_grads(torch.float64, *inputs, H)
    yard = _formula_grads(dtype, *inputs, H)
    err_y = [_err(y, t) for y, t in zip(yard[:5], truth[:5])]
    return inputs, ptr, lens, truth, err_y


def _run_kernel(case, H, dtype, kv_grad=True):
    (q, kv, g_out, src, _), ptr = case[0], case[1]
    q = q.to("cuda", dtype).requires_grad_()
    kv = kv.to("cuda", dtype).requires_grad_(kv_grad)
    out = _TConvAttn.apply(q, kv, src.cuda(), ptr.cuda(), H)
    out.backward(g_out.to("cuda", dtype))
    return out.detach(), q.grad, kv.grad


def _check_bound(got, case, dtype):
    truth, err_y = case[3], case[4]
    for i, (name, g) in enumerate(zip(NAMES, _with_halves(*got))):
        assert torch.isfinite(g).all(), name
        err_k = _err(g, truth[i])
        print(f"{name}: err_kernel={err_k:.3e} err_yardstick={err_y[i]:.3e} "
              f"ratio={err_k / max(err_y[i], 1e-30):.2f}")
        assert err_k <= 4 * err_y[i] + 16 * EPS[dtype], name


# the kernels' cap is 512 channels, so there is no wider case to add
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,C", [(1, 4), (3, 12), (4, 64), (8, 64), (1, 256)])
def test_tconv_attn_matches_fp64(H, C, dtype):
    assert _ext.tconv_max_dim() == 512
    case = _case(H, C, dtype)
    lens = case[2]
    got = _run_kernel(case, H, dtype)
    _check_bound(got, case, dtype)
    assert got[1].shape == (Q_ROWS, H * C)
    assert (got[1][N_DST:] == 0).all()          # no gradient past n_dst
    assert (got[0][(lens == 0).cuda()] == 0).all()  # empty segments


def test_tconv_attn_large_logits():
    case = _case(4, 64, torch.float32, 4.0)
    assert case[3][5].abs().max() >= 50  # the truth's logits
    _check_bound(_run_kernel(case, 4, torch.float32), case, torch.float32)


def test_tconv_attn_need_flags():
    case = _case(4, 64, torch.float32)
    full = _run_kernel(case, 4, torch.float32)
    part = _run_kernel(case, 4, torch.float32, kv_grad=False)
    assert part[2] is None
    assert torch.equal(part[1], full[1])  # a plain store: bitwise


@pytest.mark.parametrize("kw", [dict(concat=False), dict(beta=True),
                                dict(root_weight=False), dict(dropout=0.5)],
                         ids=["mean", "beta", "no_root", "dropout"])
def test_transformer_conv_routing(small_graph, kw, monkeypatch):
    indptr, indices = small_graph
    topo = quiver.CSRTopo(indptr=indptr, indices=indices)
    sampler = quiver.GraphSageSampler(topo, [5], device=0, mode="GPU")
    n_id, _, adjs = sampler.sample(torch.arange(64))
    edge_index, _, size = adjs[0]
    torch.manual_seed(0)
    x0 = torch.randn(n_id.numel(), 32)
    calls, real = [], _TConvAttn.apply
    monkeypatch.setattr(_TConvAttn, "apply",
                        lambda *a: (calls.append(1), real(*a))[1])

    def run(sorted_dst, device, dtype):
        torch.manual_seed(1)
        conv = TransformerConv(32, 16, heads=2, sorted_dst=sorted_dst, **kw)
        conv = conv.to(device, dtype)
        x = x0.to(device, dtype).requires_grad_()
        ei = edge_index if sorted_dst else edge_index.clone().to(device)
        out = conv((x, x[:size[1]]), ei, size)
        out.square().sum().backward()
        return dict([("out", out.detach()), ("x", x.grad)]
                    + [(n, p.grad) for n, p in conv.named_parameters()])

    fused = run(True, "cuda", torch.float32)
    if kw.get("dropout"):
        # training-mode attention dropout takes the torch chain
        assert not calls
        assert all(torch.isfinite(t).all() for t in fused.values())
        return
    assert len(calls) == 1
    truth = run(False, "cpu", torch.float64)
    chain = run(False, "cuda", torch.float32)
    assert len(calls) == 1 and fused.keys() == truth.keys() == chain.keys()
    for name, t in truth.items():
        f, c = fused[name], chain[name]
        # an unused lin_skip / lin_beta has no gradient on any path
        assert (f is None) == (t is None) == (c is None), name
        if t is None:
            continue
        # a key bias shifts every logit of a segment alike, so its gradient
        # is zero but for rounding and has no scale of its own: it is
        # measured on the scale of the key weight's gradient
        ref = truth["lin_key.weight"] if name == "lin_key.bias" else t
        err_f, err_c = (((g.double().cpu() - t).abs().max()
                         / ref.abs().max()).item() for g in (f, c))
        print(f"{name}: err_fused={err_f:.3e} err_chain={err_c:.3e}")
        assert err_f <= 4 * err_c + 16 * EPS[torch.float32], name


def _zero_segment_args(dim=8):
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    return dict(q=z(0, dim), kv=z(3, 2 * dim), go=z(0, dim), out=z(0, dim),
                lse=z(0, 2), src=z(0, dtype=torch.int64),
                ptr=z(1, dtype=torch.int64), heads=2)


_CALLS = {
    "fwd": lambda a: _ext.tconv_attn(a["q"], a["kv"], a["src"], a["ptr"],
                                     a["heads"]),
    "bwd": lambda a: _ext.tconv_attn_backward(
        a["go"], a["q"], a["kv"], a["out"], a["lse"], a["src"], a["ptr"],
        a["heads"], True, True),
}
_BREAK = {
    "src_on_cpu": lambda a: a.update(src=a["src"].cpu()),
    "dst_ptr_empty": lambda a: a.update(ptr=a["ptr"][:0]),
    "kv_width": lambda a: a.update(kv=a["kv"][:, :12].contiguous()),
    "lse_shape": lambda a: a.update(lse=a["lse"].new_zeros(0, 3)),
    "grad_out_dtype": lambda a: a.update(go=a["go"].bfloat16()),
    # 6 channels per head
    "chead_not_multiple_of_4": lambda a: a.update(_zero_segment_args(12)),
    "dim_above_cap": lambda a: a.update(
        _zero_segment_args(_ext.tconv_max_dim() + 8)),
}
_BAD_ARGS = [(op, fault) for fault in _BREAK for op in _CALLS
             if not (op == "fwd" and fault in ("lse_shape", "grad_out_dtype"))]


@pytest.mark.parametrize("op,fault", _BAD_ARGS,
                         ids=[f"{op}-{fault}" for op, fault in _BAD_ARGS])
def test_tconv_bad_arguments_raise(op, fault):
    args = _zero_segment_args()
    _CALLS[op](args)  # the well-formed call goes through
    _BREAK[fault](args)
    with pytest.raises(RuntimeError):
        _CALLS[op](args)
