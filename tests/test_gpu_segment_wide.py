"""Segment-mean kernels with the lane group sized to the row: forward
(rows in flight), backward scatter and the fused input-gradient entry
point, against fp64 references with bounds derived from the data."""
import pytest
import torch

from quiver import _ext
import quiver.nn as qnn
from quiver.nn import GraphSAGE, SAGEConv

gpu = pytest.mark.gpu

U32 = 2.0 ** -24        # fp32 unit roundoff
N_SRC = 3000
BLOCK = 256             # threads per block of the segment kernels


def _bf16_ulp(v):
    """Spacing of bf16 (8 significant bits) at magnitude |v|."""
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    return torch.pow(2.0, e - 7)


def _segments(n_dst, lengths, seed):
    """dst-sorted edge list whose segment lengths cycle through `lengths`."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor([lengths[d % len(lengths)] for d in range(n_dst)])
    ptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(lens, 0)
    src = torch.randint(0, N_SRC, (int(ptr[-1]),), generator=g)
    return src, ptr, lens


def _lengths():
    u = _ext.segment_mean_rows_in_flight()
    return [0, 1, u - 1, u, u + 1, 3 * u + 2]


_X = {}


def _features(dim, dtype):
    """One shared feature table per (dim, dtype), never modified."""
    key = (dim, dtype)
    if key not in _X:
        g = torch.Generator().manual_seed(100 + dim)
        _X[key] = torch.randn(N_SRC, dim, generator=g).to(dtype).cuda()
    return _X[key]


def _n_dst_cases(dim, bf16):
    groups = BLOCK // _ext.segment_mean_lanes(dim, bf16)
    return [1, groups - 1, groups + 1, 4097]


@gpu
@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("dim,dtype", [
    (256, torch.float32), (100, torch.float32), (64, torch.float32),
    (7, torch.float32), (256, torch.bfloat16), (100, torch.bfloat16),
    (64, torch.bfloat16)])
def test_forward_vs_fp64(dim, dtype, case):
    bf16 = dtype == torch.bfloat16
    n_dst = _n_dst_cases(dim, bf16)[case]
    src, ptr, lens = _segments(n_dst, _lengths(), seed=case)
    x = _features(dim, dtype)
    out = _ext.segment_mean_gather(x, src.cuda(), ptr.cuda()).cpu()
    assert out.shape == (n_dst, dim) and out.dtype == dtype

    x64 = x.cpu().double()
    dst = torch.repeat_interleave(torch.arange(n_dst), lens)
    ssum = torch.zeros(n_dst, dim, dtype=torch.float64)
    ssum.index_add_(0, dst, x64[src])
    sabs = torch.zeros(n_dst, dim, dtype=torch.float64)
    sabs.index_add_(0, dst, x64[src].abs())
    cnt = lens.clamp(min=1).double().unsqueeze(1)
    ref = ssum / cnt
    # L-term sequential fp32 sum (L-1 roundings), 1/L rounded, one multiply:
    # |err| <= (L + 1) u * sum|x| / L to first order; (L + 2) covers the
    # higher-order terms.  bf16 adds the final rounding, under one ulp.
    tol = (lens.double().unsqueeze(1) + 2) * U32 * sabs / cnt
    if bf16:
        tol = tol + _bf16_ulp(ref)
    err = (out.double() - ref).abs()
    assert bool((err <= tol).all()), (err - tol).max()
    # empty segments give exact zeros
    assert bool((out[lens == 0] == 0).all())


@gpu
@pytest.mark.parametrize("dim", [256, 100, 64, 7])
def test_forward_fp32_bitwise_sequential(dim):
    """fp32 adds in ascending edge order, then one multiply by 1/count:
    bit for bit a loop over the edge position."""
    n_dst = 4097
    src, ptr, lens = _segments(n_dst, _lengths(), seed=11)
    x = _features(dim, torch.float32)
    src, ptr, lens = src.cuda(), ptr.cuda(), lens.cuda()
    out = _ext.segment_mean_gather(x, src, ptr)
    acc = torch.zeros(n_dst, dim, device="cuda")
    for p in range(int(lens.max())):
        live = (lens > p).nonzero().squeeze(1)
        acc[live] = acc[live] + x[src[ptr[live] + p]]
    # 1/count as a correctly rounded fp32 division (done on the host)
    lens_h = lens.cpu()
    inv = torch.where(lens_h > 0, 1.0 / lens_h.clamp(min=1).float(),
                      torch.zeros(())).cuda()
    ref = acc * inv.unsqueeze(1)
    assert torch.equal(out, ref), (out - ref).abs().max()


def _scatter_reference(go, gself, src, ptr, lens):
    """fp64 grad_x and the sum of |terms| per element."""
    n_dst, dim = go.shape
    dst = torch.repeat_interleave(torch.arange(n_dst), lens)
    term = go.double()[dst] / lens.double()[dst].unsqueeze(1)
    ref = torch.zeros(N_SRC, dim, dtype=torch.float64)
    ref.index_add_(0, src, term)
    mag = torch.zeros(N_SRC, dim, dtype=torch.float64)
    mag.index_add_(0, src, term.abs())
    terms = torch.zeros(N_SRC, dtype=torch.float64)
    terms.index_add_(0, src, torch.ones(src.numel(), dtype=torch.float64))
    if gself is not None:
        ref[:gself.size(0)] += gself.double()
        mag[:gself.size(0)] += gself.double().abs()
        terms[:gself.size(0)] += 1
    return ref, mag, terms.unsqueeze(1)


@gpu
@pytest.mark.parametrize("with_self", [False, True])
@pytest.mark.parametrize("dim,dtype", [
    (256, torch.float32), (100, torch.float32), (64, torch.float32),
    (7, torch.float32), (256, torch.bfloat16), (100, torch.bfloat16),
    (64, torch.bfloat16)])
def test_backward_entry_points_vs_fp64(dim, dtype, with_self):
    bf16 = dtype == torch.bfloat16
    groups = BLOCK // _ext.segment_mean_lanes(dim, bf16)
    n_dst = 2 * groups + 1
    src, ptr, lens = _segments(n_dst, _lengths(), seed=5)
    g = torch.Generator().manual_seed(dim)
    go = torch.randn(n_dst, dim, generator=g).to(dtype)
    gself = torch.randn(n_dst, dim, generator=g).to(dtype) \
        if with_self else None
    if with_self:
        gx = _ext.segment_mean_prefix_backward(
            go.cuda(), gself.cuda(), src.cuda(), ptr.cuda(), N_SRC)
    else:
        gx = _ext.segment_mean_gather_backward(
            go.cuda(), src.cuda(), ptr.cuda(), N_SRC)
        # the fused entry point without a self-path gradient is the same
        gx2 = _ext.segment_mean_prefix_backward(
            go.cuda(), None, src.cuda(), ptr.cuda(), N_SRC)
        assert gx2.shape == gx.shape
    assert gx.shape == (N_SRC, dim) and gx.dtype == dtype
    ref, mag, terms = _scatter_reference(go, gself, src, ptr, lens)
    if bf16:
        # every term is rounded to bf16 before it is added (half an ulp)
        # and the packed atomic keeps the running sum in bf16 (one more
        # rounding per add, counted as a full ulp since its rounding mode
        # is not documented), all at magnitudes the sum can reach
        # (<= sum|terms|, 2 % headroom for the roundings themselves)
        tol = (1.5 * terms + 1) * _bf16_ulp(1.02 * mag)
    else:
        # T terms added in arrival order (T-1 roundings), each term
        # carrying the roundings of 1/L and of the multiply
        tol = (terms + 2) * U32 * mag
    err = (gx.cpu().double() - ref).abs()
    assert bool((err <= tol).all()), (err - tol).max()
    # rows no edge points at, below the self-path rows: exact zeros
    untouched = (terms.squeeze(1) == 0)
    assert bool((gx.cpu()[untouched] == 0).all())


def _hand_adjs(hidden_src, seed):
    """Two dst-sorted hops: N_SRC -> 600 -> 100 with segments of 0..11."""
    g = torch.Generator().manual_seed(seed)
    adjs, n_src = [], N_SRC
    for n_dst in (600, 100):
        lens = torch.randint(0, 12, (n_dst,), generator=g)
        dst = torch.repeat_interleave(torch.arange(n_dst), lens)
        src = torch.randint(0, n_src, (dst.numel(),), generator=g)
        adjs.append((torch.stack([src, dst]).cuda(), None, (n_src, n_dst)))
        n_src = n_dst
    return adjs


def _model_grads(sorted_dst, hidden, dtype, x, adjs, target):
    torch.manual_seed(0)
    m = GraphSAGE(x.size(1), hidden, 8, num_layers=2, dropout=0.0,
                  sorted_dst=sorted_dst).cuda().to(dtype)
    out = m(x.to(dtype), adjs)
    torch.nn.functional.nll_loss(out, target).backward()
    return [out.detach().double().cpu()] + \
        [p.grad.double().cpu() for p in m.parameters()]


@gpu
@pytest.mark.parametrize("min_k", [64, 1 << 30])
@pytest.mark.parametrize("hidden", [256, 100])
def test_two_layer_sage_grads_vs_plain_path(hidden, min_k, monkeypatch):
    """Fused path (segment kernels + fused input gradient) against
    autograd through the plain torch path on the same weights.  The bound
    is the plain fp32 path's own distance from its fp64 run: both fp32
    paths add the same terms in different orders, so the fused one may
    sit as far from fp64 as the plain one does, within a factor of 2 in
    L2 norm per tensor, plus what storing the tensor in fp32 costs."""
    monkeypatch.setattr(qnn, "_WGRAD_MIN_K", min_k)
    adjs = _hand_adjs(N_SRC, seed=21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(N_SRC, 100, generator=g).cuda()
    target = torch.randint(0, 8, (100,), generator=g).cuda()
    fused = _model_grads(True, hidden, torch.float32, x, adjs, target)
    plain = _model_grads(False, hidden, torch.float32, x, adjs, target)
    ref64 = _model_grads(False, hidden, torch.float64, x, adjs, target)
    for i, (f, p, r) in enumerate(zip(fused, plain, ref64)):
        e_f = (f - r).norm().item()
        e_p = (p - r).norm().item()
        print(f"tensor {i}: fused-fp64 {e_f:.3e} plain-fp64 {e_p:.3e} "
              f"norm {r.norm().item():.3e}")
        assert e_f <= 2 * e_p + U32 * r.norm().item(), (i, e_f, e_p)


@gpu
def test_prefix_function_matches_plain_autograd():
    """_SegmentMeanPrefix (x as aggregation source and as x[:n_dst]) vs
    the index_add chain, gradient bound from term count and |grad|."""
    dim, n_dst = 256, 517
    src, ptr, lens = _segments(n_dst, _lengths(), seed=9)
    dst = torch.repeat_interleave(torch.arange(n_dst), lens)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(N_SRC, dim, generator=g)
    go = torch.randn(n_dst, dim, generator=g)
    gself = torch.randn(n_dst, dim, generator=g)
    x = x0.clone().cuda().requires_grad_(True)
    conv_in = x * 1.0
    agg, x_dst = qnn._SegmentMeanPrefix.apply(conv_in, src.cuda(),
                                              ptr.cuda(), n_dst)
    assert x_dst.data_ptr() == conv_in.data_ptr()
    ((agg * go.cuda()).sum() + (x_dst * gself.cuda()).sum()).backward()
    ref, mag, terms = _scatter_reference(go, gself, src, ptr, lens)
    err = (x.grad.cpu().double() - ref).abs()
    tol = (terms + 2) * U32 * mag
    assert bool((err <= tol).all()), (err - tol).max()
    # and the plain torch chain agrees with the same reference
    xp = x0.clone().cuda().requires_grad_(True)
    aggp = qnn._mean_aggregate(xp, src.cuda(), dst.cuda(), n_dst,
                               sorted_dst=False)
    ((aggp * go.cuda()).sum() + (xp[:n_dst] * gself.cuda()).sum()).backward()
    errp = (xp.grad.cpu().double() - ref).abs()
    assert bool((errp <= tol).all()), (errp - tol).max()


@gpu
def test_input_without_grad_runs_no_backward_kernel(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("segment-mean backward launched for an input "
                             "that carries no grad")
    monkeypatch.setattr(_ext, "segment_mean_gather_backward", boom,
                        raising=False)
    monkeypatch.setattr(_ext, "segment_mean_prefix_backward", boom,
                        raising=False)
    adjs = _hand_adjs(N_SRC, seed=2)
    ei, _, size = adjs[0]
    x = _features(100, torch.float32)
    assert not x.requires_grad
    conv = SAGEConv(100, 16, sorted_dst=True).cuda()
    out = conv((x, x[:size[1]]), ei, size)
    out.sum().backward()
    assert x.grad is None
    assert conv.lin_l.weight.grad is not None
    assert conv.lin_r.weight.grad is not None


def test_cpu_fallback_without_gpu_tensor_or_pointer():
    """sorted_dst layers on CPU tensors with a bare edge_index take the
    torch path: no native kernel, no attached pointer needed."""
    g = torch.Generator().manual_seed(4)
    n_src, n_dst = 50, 12
    lens = torch.randint(0, 5, (n_dst,), generator=g)
    dst = torch.repeat_interleave(torch.arange(n_dst), lens)
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    ei = torch.stack([src, dst])
    x = torch.randn(n_src, 8, generator=g, requires_grad=True)
    torch.manual_seed(0)
    a = SAGEConv(8, 4, sorted_dst=True)
    torch.manual_seed(0)
    b = SAGEConv(8, 4, sorted_dst=False)
    out_a = a((x, x[:n_dst]), ei, (n_src, n_dst))
    out_b = b((x, x[:n_dst]), ei, (n_src, n_dst))
    assert torch.equal(out_a, out_b)
    out_a.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape
