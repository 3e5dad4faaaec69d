"""Minimal PyG-compatible GNN layers/models in plain torch.

The reference relies on torch_geometric for its models; this environment
has no PyG, so the SAGE/GAT model families used by examples, serving and
bench.py live here.  The layers follow PyG's bipartite convention: forward
((x_src, x_dst), edge_index, size) with edge_index[0] indexing x_src and
edge_index[1] indexing x_dst — exactly what GraphSageSampler's adjs feed.
On GPU tensors with dst-sorted edges (the sampler's layout) aggregation and
attention run on the fused HIP segment kernels (csrc/segment_kernels.hip,
csrc/gatv2_kernels.hip, csrc/transformer_kernels.hip) through the autograd
functions below; other inputs take the plain torch index_add /
scatter_reduce chain.
"""
import functools
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _ext
# tensor attribute under which GraphSageSampler hangs a hop's segment
# pointer on its edge_index (survives `for edge_index, _, size in adjs`,
# not clone()/.to()/indexing)
from .pyg.sage_sampler import DST_PTR_ATTR

__all__ = ["SAGEConv", "GATConv", "GATv2Conv", "TransformerConv",
           "GraphSAGE", "GAT", "GraphTransformer", "QLinear"]


def _as_pair(x):
    if isinstance(x, (tuple, list)):
        return x[0], x[1]
    return x, x


class _SegmentMeanAgg(torch.autograd.Function):
    """Fused mean aggregation over dst-sorted edges (csrc/segment_kernels.hip).

    Replaces x[src] -> zeros -> index_add -> deg -> div with one kernel in
    each direction; the layer-1 input features carry no grad, so their
    backward is skipped entirely.
    """

    @staticmethod
    def forward(ctx, x, src, dst_ptr):
        ctx.save_for_backward(src, dst_ptr)
        ctx.n_src = x.size(0)
        return _ext.segment_mean_gather(x, src, dst_ptr)

    @staticmethod
    def backward(ctx, grad_out):
        src, dst_ptr = ctx.saved_tensors
        grad_x = _ext.segment_mean_gather_backward(
            grad_out.contiguous(), src, dst_ptr, ctx.n_src)
        return grad_x, None, None


class _SegmentMeanPrefix(torch.autograd.Function):
    """Mean aggregation plus the self-path slice for the bipartite prefix
    case (x_dst is x[:n_self]): returns (agg, x[:n_self]).

    Autograd would otherwise assemble grad_x from a zero-filled scatter
    target, a zero-padded slice gradient and a full-size add; here the
    backward makes one native call that stores the self-path rows (zeros
    below them) and scatters the aggregation's part on top.
    """

    @staticmethod
    def forward(ctx, x, src, dst_ptr, n_self):
        ctx.save_for_backward(src, dst_ptr)
        ctx.n_src = x.size(0)
        ctx.set_materialize_grads(False)
        return (_ext.segment_mean_gather(x, src, dst_ptr),
                x.narrow(0, 0, n_self))

    @staticmethod
    def backward(ctx, grad_agg, grad_self):
        src, dst_ptr = ctx.saved_tensors
        if grad_agg is None:
            if grad_self is None:
                return None, None, None, None
            grad_x = grad_self.new_zeros((ctx.n_src, grad_self.size(1)))
            grad_x[:grad_self.size(0)] = grad_self
            return grad_x, None, None, None
        grad_x = _ext.segment_mean_prefix_backward(
            grad_agg.contiguous(), grad_self, src, dst_ptr, ctx.n_src)
        return grad_x, None, None, None


class _SegmentWSum(torch.autograd.Function):
    """Weighted segment sum over dst-sorted edges (GAT attention
    aggregation, csrc/segment_kernels.hip).  Replaces the torch chain
    h_src[src] (materialize [E,H,C]) * alpha -> zeros -> index_add, which
    moves ~E*H*C*4 bytes twice per layer."""

    @staticmethod
    def forward(ctx, x, w, src, dst_ptr, heads):
        ctx.save_for_backward(x, w, src, dst_ptr)
        ctx.heads = heads
        return _ext.segment_wsum(x, w, src, dst_ptr, heads)

    @staticmethod
    def backward(ctx, grad_out):
        x, w, src, dst_ptr = ctx.saved_tensors
        gx, gw = _ext.segment_wsum_backward(
            grad_out.contiguous(), x, w, src, dst_ptr, ctx.heads,
            ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (gx if ctx.needs_input_grad[0] else None,
                gw if ctx.needs_input_grad[1] else None, None, None, None)


class _GatDots(torch.autograd.Function):
    """Fused per-head attention dots: (h*att_src).sum(-1) and the same
    for att_dst over the prefix rows, in ONE read of h (the torch chain
    materializes a broadcast product and reduces it, ~3x the traffic on
    a ~1 GB projected frontier)."""

    @staticmethod
    def forward(ctx, h, att_src, att_dst, n_dst, heads):
        asrc, adst = _ext.gat_dots(h, att_src, att_dst, n_dst, heads)
        ctx.save_for_backward(h, att_src, att_dst)
        ctx.heads = heads
        return asrc, adst

    @staticmethod
    def backward(ctx, g_asrc, g_adst):
        h, att_src, att_dst = ctx.saved_tensors
        g_h, g_as, g_ad = _ext.gat_dots_backward(
            h, att_src, att_dst, g_asrc.contiguous(), g_adst.contiguous(),
            ctx.heads)
        return g_h, g_as, g_ad, None, None


class _GatAlpha(torch.autograd.Function):
    """Fused GAT attention coefficients over dst-sorted edges: per-node
    logit gathers + add + leaky_relu + segment softmax in one kernel pair
    (no [E,H] torch intermediates)."""

    @staticmethod
    def forward(ctx, asrc, adst, src, dst_ptr, heads, slope, n_edges):
        alpha = _ext.gat_alpha(asrc, adst, src, dst_ptr, heads, slope,
                               n_edges)
        ctx.save_for_backward(alpha, asrc, adst, src, dst_ptr)
        ctx.heads, ctx.slope = heads, slope
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        alpha, asrc, adst, src, dst_ptr = ctx.saved_tensors
        g_asrc, g_adst = _ext.gat_alpha_backward(
            grad_alpha, alpha, asrc, adst, src, dst_ptr, ctx.heads,
            ctx.slope)
        return g_asrc, g_adst, None, None, None, None, None


class _GatV2Attn(torch.autograd.Function):
    """Fused GATv2 attention over dst-sorted edges (csrc/gatv2_kernels.hip):
    out[d,h,:] = sum_e softmax_seg(<att[h], leaky_relu(xl[src_e,h] +
    xr[d,h])>) * xl[src_e,h,:], one pass over each segment in either
    direction (online softmax forward, alpha recomputed from the saved
    log-sum-exp backward) and no [E,H,C] tensor at all."""

    @staticmethod
    def forward(ctx, xl, xr, att, src, dst_ptr, heads, slope):
        out, lse = _ext.gatv2_attn(xl, xr, att, src, dst_ptr, heads, slope)
        ctx.save_for_backward(xl, xr, att, out, lse, src, dst_ptr)
        ctx.heads, ctx.slope = heads, slope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        xl, xr, att, out, lse, src, dst_ptr = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        g_xl, g_xr, g_att = _ext.gatv2_attn_backward(
            grad_out.contiguous(), xl, xr, att, out, lse, src, dst_ptr,
            ctx.heads, ctx.slope, *need)
        return (g_xl if need[0] else None, g_xr if need[1] else None,
                g_att if need[2] else None, None, None, None, None)


class _GatV2AttnEdge(torch.autograd.Function):
    """_GatV2Attn with edge features inside the non-linearity:
    z = xl[src_e] + xr[d] + edge_attr[row_e] @ w_edge, row_e = edge_id[e]
    when edge_id is given, else e.  The kernels project the D raw values of
    an edge themselves, so no [E, H*C] tensor exists in either direction.
    w_edge is lin_edge.weight ([H*C, D]); its gradient comes back in its
    dtype.  edge_attr gets no gradient."""

    @staticmethod
    def forward(ctx, xl, xr, att, edge_attr, edge_id, w_edge, src, dst_ptr,
                heads, slope):
        w = w_edge.detach().t().contiguous().float()       # [D, H*C]
        out, lse = _ext.gatv2_attn_edge(xl, xr, att, edge_attr, edge_id, w,
                                        src, dst_ptr, heads, slope)
        ctx.save_for_backward(xl, xr, att, edge_attr, edge_id, w, out, lse,
                              src, dst_ptr)
        ctx.heads, ctx.slope, ctx.w_dtype = heads, slope, w_edge.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (xl, xr, att, edge_attr, edge_id, w, out, lse, src,
         dst_ptr) = ctx.saved_tensors
        need = ctx.needs_input_grad
        g_xl, g_xr, g_att, g_w = _ext.gatv2_attn_edge_backward(
            grad_out.contiguous(), xl, xr, att, edge_attr, edge_id, w, out,
            lse, src, dst_ptr, ctx.heads, ctx.slope, need[0], need[1],
            need[2], need[5])
        return (g_xl if need[0] else None, g_xr if need[1] else None,
                g_att if need[2] else None, None, None,
                g_w.t().to(ctx.w_dtype) if need[5] else None,
                None, None, None, None)


class _TConvAttn(torch.autograd.Function):
    """Fused scaled dot-product attention over dst-sorted edges
    (csrc/transformer_kernels.hip): q [>= n_dst, H*C] one query row per dst,
    kv [n_src, 2*H*C] the key row then the value row of each source,
    out[d,h,:] = sum_e softmax_seg(<q[d,h], k[src_e,h]> / sqrt(C)) *
    v[src_e,h,:].  One pass over each segment in either direction (online
    softmax forward, alpha recomputed from the saved log-sum-exp backward)
    and no [E,H,C] tensor at all."""

    @staticmethod
    def forward(ctx, q, kv, src, dst_ptr, heads):
        out, lse = _ext.tconv_attn(q, kv, src, dst_ptr, heads)
        ctx.save_for_backward(q, kv, out, lse, src, dst_ptr)
        ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q, kv, out, lse, src, dst_ptr = ctx.saved_tensors
        need = ctx.needs_input_grad[:2]
        g_q, g_kv = _ext.tconv_attn_backward(
            grad_out.contiguous(), q, kv, out, lse, src, dst_ptr, ctx.heads,
            *need)
        return (g_q if need[0] else None, g_kv if need[1] else None,
                None, None, None)


class _QLinearFn(torch.autograd.Function):
    """Linear layer whose weight gradient uses the split-K HIP kernel
    (csrc/wgrad_kernels.hip).

    Big-frontier linear GEMM routing (all measured, benchmarks/):
    - weight-grad: custom MFMA split-K (csrc/wgrad_kernels.hip,
      deterministic workspace reduce, 2.8-5.7x rocBLAS on these shapes)
      with the bias grad folded in;
    - narrow-output data-grads (in_features <= 128): custom tall-M MFMA
      kernel (csrc/gemm_kernels.hip, 1.1-1.25x);
    - forward and wide data-grads: rocBLAS (it wins there).
    Custom-kernel numerics are exact f32 fmaf chains
    (v_mfma_f32_32x32x2_f32).
    """

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        if ctx.needs_input_grad[0]:
            # narrow-output data-grads (in_features <= 128) beat rocBLAS
            # on the tall-M MFMA kernel (measured 1.1-1.25x; wide shapes
            # lose ~15% — rocBLAS keeps those; benchmarks/bench_gemm.py)
            if weight.size(1) <= 128 and grad_out.is_cuda \
                    and grad_out.dtype == torch.float32:
                grad_x = _ext.tall_gemm(grad_out, weight, None)
            else:
                grad_x = grad_out @ weight
        else:
            grad_x = None
        grad_w, grad_b = _ext.wgrad(grad_out, x, ctx.has_bias)
        return grad_x, grad_w, (grad_b if ctx.has_bias else None)


# frontier sizes below this use plain F.linear (rocBLAS wgrad is fine there)
_WGRAD_MIN_K = 16384


def _qlinear(x, weight, bias):
    """F.linear with QLinear's routing."""
    if (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and x.size(0) >= _WGRAD_MIN_K and torch.is_grad_enabled()):
        return _QLinearFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)


class QLinear(nn.Linear):
    """nn.Linear with the custom tall-skinny weight-grad path on GPU fp32
    inputs with a large leading (frontier) dimension."""

    def forward(self, x):
        return _qlinear(x, self.weight, self.bias)


_ARANGE_CACHE = {}


def _arange(n, device):
    """Cached 0..n view (avoids one alloc+launch per layer per step)."""
    key = device.index if device.type == "cuda" else -1
    cached = _ARANGE_CACHE.get(key)
    if cached is None or cached.numel() < n:
        cached = torch.arange(max(n, 1 << 20), device=device)
        _ARANGE_CACHE[key] = cached
    return cached[:n]


_QUIVER_DEBUG = bool(int(__import__("os").environ.get("QUIVER_DEBUG", "0")))


def _dst_ptr_from_sorted(dst, n_dst):
    """Segment pointer from a dst-sorted edge list.  searchsorted silently
    returns garbage on unsorted input, so sorted_dst=True layers fed edges
    from a non-quiver sampler would be silently wrong — QUIVER_DEBUG=1
    turns that into a loud error."""
    if _QUIVER_DEBUG and dst.numel() > 1:
        assert bool((dst[1:] >= dst[:-1]).all()), \
            "sorted_dst=True but edge_index[1] is not sorted ascending"
    return torch.searchsorted(dst, _arange(n_dst + 1, dst.device))


def _dst_ptr_for(edge_index, n_dst):
    """Segment pointer of a dst-sorted edge_index: the one the sampler
    attached (its own scan of the per-dst sampled counts) when present and
    of the right length, else rebuilt from the edge list."""
    dst = edge_index[1]
    ptr = getattr(edge_index, DST_PTR_ATTR, None)
    if (ptr is None or ptr.dim() != 1 or ptr.numel() != n_dst + 1
            or ptr.device != dst.device or ptr.dtype != torch.int64):
        return _dst_ptr_from_sorted(dst, n_dst)
    if _QUIVER_DEBUG:
        assert torch.equal(ptr, _dst_ptr_from_sorted(dst, n_dst)), \
            "sampler-attached dst_ptr disagrees with edge_index[1]"
    return ptr


def _is_prefix(x_src, x_dst):
    """x_dst is the leading rows of x_src, as a view (the bipartite prefix
    convention: the models pass (x, x[:n_dst]))."""
    return (x_dst.data_ptr() == x_src.data_ptr()
            and x_dst.size(0) <= x_src.size(0)
            and x_dst.stride() == x_src.stride()
            and x_dst.size(1) == x_src.size(1))


def _fused_mean_ok(x_src, dst, sorted_dst):
    return (sorted_dst and x_src.is_cuda and dst.numel() > 0
            and (x_src.dtype == torch.float32
                 or (x_src.dtype == torch.bfloat16
                     and x_src.size(1) % 2 == 0)))


def _mean_torch(x_src, src, dst, n_dst):
    agg = torch.zeros((n_dst, x_src.size(1)), dtype=x_src.dtype,
                      device=x_src.device)
    agg.index_add_(0, dst, x_src[src])
    deg = torch.zeros(n_dst, dtype=x_src.dtype, device=x_src.device)
    deg.index_add_(0, dst, torch.ones_like(dst, dtype=x_src.dtype))
    return agg / deg.clamp_(min=1).unsqueeze(-1)


def _mean_aggregate(x_src, src, dst, n_dst, sorted_dst=False, dst_ptr=None):
    """Mean of x_src[src] grouped by dst.  Uses the fused HIP kernel when
    the caller guarantees dst is sorted ascending (our sampler's layout)
    on fp32 or even-width bf16 GPU tensors."""
    if not _fused_mean_ok(x_src, dst, sorted_dst):
        return _mean_torch(x_src, src, dst, n_dst)
    if dst_ptr is None:
        dst_ptr = _dst_ptr_from_sorted(dst, n_dst)
    return _SegmentMeanAgg.apply(x_src, src, dst_ptr)


class SAGEConv(nn.Module):
    """GraphSAGE-mean convolution.

    Set sorted_dst=True when edge_index[1] is sorted ascending (always the
    case for GraphSageSampler's adjs) to enable the fused segment-mean HIP
    kernel."""

    def __init__(self, in_channels, out_channels, bias=True,
                 sorted_dst=False):
        super().__init__()
        self.sorted_dst = sorted_dst
        self.lin_l = QLinear(in_channels, out_channels, bias=bias)  # neigh
        self.lin_r = QLinear(in_channels, out_channels, bias=False)  # self
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin_l.weight)
        nn.init.xavier_uniform_(self.lin_r.weight)
        if self.lin_l.bias is not None:
            nn.init.zeros_(self.lin_l.bias)

    def forward(self, x, edge_index, size: Tuple[int, int] = None):
        x_src, x_dst = _as_pair(x)
        src, dst = edge_index[0], edge_index[1]
        n_dst = x_dst.size(0) if size is None else int(size[1])
        # aggregate-then-project: segment mean on in_channels, one GEMM after
        if not _fused_mean_ok(x_src, dst, self.sorted_dst):
            agg = _mean_torch(x_src, src, dst, n_dst)
        else:
            dst_ptr = _dst_ptr_for(edge_index, n_dst)
            if (x_src.requires_grad and torch.is_grad_enabled()
                    and x_src.is_contiguous() and _is_prefix(x_src, x_dst)):
                # x feeds both paths: one function owns the whole input
                # gradient (inputs without grad, e.g. layer 0, skip this
                # and never run a backward)
                agg, x_dst = _SegmentMeanPrefix.apply(x_src, src, dst_ptr,
                                                      x_dst.size(0))
            else:
                agg = _SegmentMeanAgg.apply(x_src, src, dst_ptr)
        out = self.lin_l(agg)
        if (x_dst.is_cuda and x_dst.dtype == torch.float32
                and x_dst.size(0) >= _WGRAD_MIN_K
                and torch.is_grad_enabled()):
            # large frontier: route the self path through QLinear so ITS
            # weight grad also takes the split-K kernel
            return out + self.lin_r(x_dst)
        # small/no-grad: self path fused into the neighbor GEMM via addmm
        return out.addmm_(x_dst, self.lin_r.weight.t()) if not out.requires_grad \
            else torch.addmm(out, x_dst, self.lin_r.weight.t())


class GATConv(nn.Module):
    """Graph attention convolution (multi-head, concat)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True,
                 negative_slope=0.2, dropout=0.0, bias=True,
                 sorted_dst=False):
        super().__init__()
        self.sorted_dst = sorted_dst
        self.heads = heads
        self.out_channels = out_channels
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.lin = QLinear(in_channels, heads * out_channels, bias=False)
        self.att_src = nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = nn.Parameter(torch.empty(1, heads, out_channels))
        out_dim = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(out_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)
        nn.init.xavier_uniform_(self.att_src)
        nn.init.xavier_uniform_(self.att_dst)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, size: Tuple[int, int] = None):
        x_src, x_dst = _as_pair(x)
        src, dst = edge_index[0], edge_index[1]
        H, C = self.heads, self.out_channels
        n_dst = x_dst.size(0) if size is None else int(size[1])

        h2 = self.lin(x_src)
        # bf16 models: the projected features stay bf16 end to end — the
        # dots/wsum kernels take bf16 h with fp32 accumulation, while the
        # LOGITS (alpha) and softmax stay fp32 (standard practice, and
        # they are [*, H]-small).  Odd head widths fall back to one
        # boundary cast; torch's bf16 softmax fallback chain
        # (scatter_reduce amax -> ~120 rocprim sort kernels) is far
        # slower than either.
        out_dtype = h2.dtype
        # decided once: `segments` = dst-sorted edges on the GPU (the alpha
        # kernel's layout), `native` = h additionally fits the dots/wsum
        # kernels; dst_ptr is set exactly when a segment kernel may run
        segments = self.sorted_dst and h2.is_cuda
        native = (segments and C % 4 == 0
                  and h2.dtype in (torch.float32, torch.bfloat16))
        if segments and not native and h2.dtype == torch.bfloat16:
            h2 = h2.float()
        dst_ptr = (_dst_ptr_for(edge_index, n_dst)
                   if segments and dst.numel() > 0 else None)
        h_src = h2.view(-1, H, C)
        prefix = _is_prefix(x_src, x_dst)
        if prefix and native:
            # bipartite prefix convention (x_dst is x_src[:n_dst]) with
            # the fused dots kernel: one read of h for both logit sets
            alpha_src, alpha_dst = _GatDots.apply(
                h2, self.att_src.reshape(-1).float(),
                self.att_dst.reshape(-1).float(), x_dst.size(0), H)
        else:
            if prefix:
                h_dst = h_src[:x_dst.size(0)]
            else:
                h_dst = self.lin(x_dst).view(-1, H, C)
            alpha_src = (h_src * self.att_src).sum(-1)  # [N_src, H]
            alpha_dst = (h_dst * self.att_dst).sum(-1)  # [N_dst, H]
        if dst_ptr is not None and alpha_src.dtype == torch.float32:
            alpha = _GatAlpha.apply(alpha_src, alpha_dst, src, dst_ptr, H,
                                    self.negative_slope, src.numel())
        else:
            alpha = alpha_src[src] + alpha_dst[dst]     # [E, H]
            alpha = F.leaky_relu(alpha, self.negative_slope)
            # segment softmax over incoming edges of each dst (torch path)
            alpha_max = torch.full((n_dst, H), float("-inf"),
                                   dtype=alpha.dtype, device=alpha.device)
            alpha_max = alpha_max.scatter_reduce(
                0, dst.unsqueeze(-1).expand_as(alpha), alpha, reduce="amax",
                include_self=True)
            alpha = (alpha - alpha_max[dst]).exp()
            denom = torch.zeros((n_dst, H), dtype=alpha.dtype,
                                device=alpha.device)
            denom.index_add_(0, dst, alpha)
            alpha = alpha / denom[dst].clamp(min=1e-16)
        if self.training and self.dropout > 0:
            alpha = F.dropout(alpha, p=self.dropout)

        if (native and dst_ptr is not None
                and alpha.dtype == torch.float32):
            # fused weighted segment sum over the dst-sorted edges
            out = _SegmentWSum.apply(h_src.reshape(-1, H * C), alpha, src,
                                     dst_ptr, H)
            out = out if self.concat else out.view(n_dst, H, C).mean(1)
        else:
            msg = h_src[src] * alpha.unsqueeze(-1)      # [E, H, C]
            out = torch.zeros((n_dst, H, C), dtype=msg.dtype,
                              device=msg.device)
            out.index_add_(0, dst, msg)
            out = (out.reshape(n_dst, H * C) if self.concat
                   else out.mean(1))
        if self.bias is not None:
            out = out + self.bias
        return out.to(out_dtype) if out.dtype != out_dtype else out


# widest heads * out_channels the fused GATv2 kernels keep in registers
_GATV2_MAX_DIM = 1024
# largest edge_dim * heads * out_channels of the fused edge-feature kernels:
# the fp32 lin_edge weight and its gradient accumulator share one block's
# LDS (2 * 4 * 8192 bytes = 64 KiB)
_GATV2_MAX_EDGE_WEIGHT = 8192
# When lin_edge's weight gradient is needed, the fused edge backward is bound
# by its fp32 LDS atomics (edge_dim * heads * out_channels per two edges) and
# was measured against the torch chain (profiles/SEGMENT_GATV2.md): faster
# up to this weight size for bf16 rows and, for fp32 rows, only at the
# smallest measured edge count; slower or level elsewhere, which goes to the
# chain.
_GATV2_EDGE_TRAIN_MAX_WEIGHT = 4096
_GATV2_EDGE_TRAIN_FP32_MAX_EDGES = 16384


class GATv2Conv(nn.Module):
    """GATv2 convolution (Brody et al., "How Attentive are Graph Attention
    Networks?"), PyG's parameter names and semantics: lin_l projects the
    source rows, lin_r the target rows (the same module when
    share_weights), and the logit of an edge is
    att[h] . leaky_relu(lin_l(x_src)[src] + lin_r(x_dst)[dst]).

    With sorted_dst=True (GraphSageSampler's adjs) on GPU tensors of fp32
    or bf16, out_channels % 4 == 0 and heads * out_channels <= 1024, the
    attention and aggregation run in the fused kernels of
    csrc/gatv2_kernels.hip.  Attention dropout in training mode, and any
    other input, takes the plain torch chain below.

    edge_dim=D adds lin_edge (no bias) and forward(..., edge_attr=,
    edge_id=): lin_edge(edge_attr) joins the sum inside the leaky_relu; the
    messages carry no edge term.  edge_attr is [E, D] with a row per column
    of edge_index, or with edge_id (int64 [E], e.g. Adj.e_id of a sampler
    built with return_eid=True) any table whose row edge_id[e] belongs to
    edge e.  The fused kernels project the raw rows themselves when also
    D * heads * out_channels <= 8192 and edge_attr needs no gradient; with
    a weight gradient for lin_edge to compute, only where that was measured
    faster than the torch chain (see _GATV2_EDGE_TRAIN_MAX_WEIGHT)."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True,
                 negative_slope=0.2, dropout=0.0, bias=True,
                 share_weights=False, sorted_dst=False, edge_dim=None):
        super().__init__()
        self.sorted_dst = sorted_dst
        self.edge_dim = edge_dim
        self.heads = heads
        self.out_channels = out_channels
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.share_weights = share_weights
        self.lin_l = QLinear(in_channels, heads * out_channels, bias=bias)
        self.lin_r = (self.lin_l if share_weights else
                      QLinear(in_channels, heads * out_channels, bias=bias))
        self.lin_edge = (None if edge_dim is None else
                         QLinear(edge_dim, heads * out_channels, bias=False))
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        out_dim = heads * out_channels if concat else out_channels
        self.bias = nn.Parameter(torch.zeros(out_dim)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in ((self.lin_l,) if self.share_weights
                    else (self.lin_l, self.lin_r)):
            nn.init.xavier_uniform_(lin.weight)
            if lin.bias is not None:
                nn.init.zeros_(lin.bias)
        if self.lin_edge is not None:
            nn.init.xavier_uniform_(self.lin_edge.weight)
        nn.init.xavier_uniform_(self.att)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _fused_ok(self, xl, dst):
        H, C = self.heads, self.out_channels
        return (self.sorted_dst and xl.is_cuda and dst.numel() > 0
                and xl.dtype in (torch.float32, torch.bfloat16)
                and C % 4 == 0 and H * C <= _GATV2_MAX_DIM
                and not (self.training and self.dropout > 0))

    def _checked_edge_attr(self, edge_attr, edge_id, n_edges):
        if edge_attr is None:
            if edge_id is not None:
                raise ValueError("GATv2Conv: edge_id given without edge_attr")
            return None
        if self.edge_dim is None:
            raise ValueError("GATv2Conv: edge_attr given to a layer built "
                             "without edge_dim")
        if edge_attr.dim() == 1:
            edge_attr = edge_attr.view(-1, 1)
        if edge_attr.dim() != 2 or edge_attr.size(1) != self.edge_dim:
            raise ValueError(f"GATv2Conv: edge_attr must be [*, "
                             f"{self.edge_dim}], got "
                             f"{tuple(edge_attr.shape)}")
        if edge_id is None and edge_attr.size(0) != n_edges:
            raise ValueError(f"GATv2Conv: edge_attr has {edge_attr.size(0)} "
                             f"rows for {n_edges} edges; pass edge_id to "
                             "select rows of a table")
        if edge_id is not None and edge_id.numel() != n_edges:
            raise ValueError(f"GATv2Conv: edge_id has {edge_id.numel()} "
                             f"entries for {n_edges} edges")
        return edge_attr

    def _fused_edge_ok(self, xl, edge_attr, edge_id, n_edges):
        weight = self.edge_dim * self.heads * self.out_channels
        if torch.is_grad_enabled() and self.lin_edge.weight.requires_grad \
                and not (weight <= _GATV2_EDGE_TRAIN_MAX_WEIGHT
                         and (xl.dtype == torch.bfloat16 or n_edges
                              <= _GATV2_EDGE_TRAIN_FP32_MAX_EDGES)):
            return False
        # the kernels pad a head to a power of two of 4-byte words and the
        # edge variant holds at most 1024 such slots
        words = self.out_channels * xl.element_size() // 4
        slots = self.heads * (1 << (words - 1).bit_length())
        return (slots <= 1024
                and edge_attr.is_cuda and not edge_attr.requires_grad
                and edge_attr.is_floating_point()
                and (edge_id is None or (edge_id.is_cuda
                                         and edge_id.dtype == torch.int64))
                and weight <= _GATV2_MAX_EDGE_WEIGHT)

    def forward(self, x, edge_index, size: Tuple[int, int] = None,
                edge_attr=None, edge_id=None):
        x_src, x_dst = _as_pair(x)
        src, dst = edge_index[0], edge_index[1]
        H, C = self.heads, self.out_channels
        n_dst = x_dst.size(0) if size is None else int(size[1])
        edge_attr = self._checked_edge_attr(edge_attr, edge_id, src.numel())

        xl = self.lin_l(x_src)
        if self.share_weights and _is_prefix(x_src, x_dst):
            # bipartite prefix convention: the target rows are already
            # projected, as the leading rows of xl
            xr = xl[:x_dst.size(0)]
        else:
            xr = self.lin_r(x_dst)

        fused = self._fused_ok(xl, dst)
        if fused and edge_attr is not None:
            fused = self._fused_edge_ok(xl, edge_attr, edge_id, src.numel())
        if fused and edge_attr is not None:
            # the table stays as it is (edge_id selects rows in the kernel);
            # a table of another float dtype is narrow: cast it whole
            out = _GatV2AttnEdge.apply(
                xl, xr, self.att.reshape(-1).float(),
                edge_attr.to(xl.dtype).contiguous(), edge_id,
                self.lin_edge.weight, src, _dst_ptr_for(edge_index, n_dst),
                H, self.negative_slope)
            out = out if self.concat else out.view(n_dst, H, C).mean(1)
        elif fused:
            out = _GatV2Attn.apply(
                xl, xr, self.att.reshape(-1).float(), src,
                _dst_ptr_for(edge_index, n_dst), H, self.negative_slope)
            out = out if self.concat else out.view(n_dst, H, C).mean(1)
        else:
            xl3 = xl.view(-1, H, C)
            z = xl3[src] + xr.view(-1, H, C)[dst]
            if edge_attr is not None:
                ea = edge_attr if edge_id is None else edge_attr[edge_id]
                z = z + self.lin_edge(ea.to(xl.dtype)).view(-1, H, C)
            z = F.leaky_relu(z, self.negative_slope)     # [E, H, C]
            alpha = (z * self.att).sum(-1)               # [E, H]
            # segment softmax over the incoming edges of each dst
            amax = torch.full((n_dst, H), float("-inf"), dtype=alpha.dtype,
                              device=alpha.device)
            amax = amax.scatter_reduce(
                0, dst.unsqueeze(-1).expand_as(alpha), alpha, reduce="amax",
                include_self=True)
            alpha = (alpha - amax[dst]).exp()
            denom = torch.zeros((n_dst, H), dtype=alpha.dtype,
                                device=alpha.device)
            denom.index_add_(0, dst, alpha)
            alpha = alpha / denom[dst].clamp(min=1e-16)
            if self.training and self.dropout > 0:
                alpha = F.dropout(alpha, p=self.dropout)
            out = torch.zeros((n_dst, H, C), dtype=xl.dtype,
                              device=xl.device)
            out.index_add_(0, dst, xl3[src] * alpha.unsqueeze(-1))
            out = (out.reshape(n_dst, H * C) if self.concat
                   else out.mean(1))
        if self.bias is not None:
            out = out + self.bias
        return out


class TransformerConv(nn.Module):
    """Graph transformer convolution (Shi et al., "Masked Label Prediction:
    Unified Message Passing Model for Semi-Supervised Classification"),
    PyG's parameter names and semantics without edge features: the logit of
    an edge is <lin_query(x_dst)[dst], lin_key(x_src)[src]> / sqrt(C) per
    head, softmax over the incoming edges of each dst, and the message is
    lin_value(x_src)[src].  root_weight adds lin_skip(x_dst); beta gates the
    two with sigmoid(lin_beta([out, x_r, out - x_r])).

    Keys and values come from one GEMM over x_src (the lin_key and lin_value
    weights concatenated), so a source node owns one [2 * heads * C] row.
    With sorted_dst=True (GraphSageSampler's adjs) on GPU tensors of fp32
    or bf16, out_channels % 4 == 0 and heads * out_channels within the
    kernels' cap (_ext.tconv_max_dim()), the attention and aggregation run
    in the fused kernels of csrc/transformer_kernels.hip.  Attention dropout
    in training mode, and any other input, takes the plain torch chain
    below."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True,
                 beta=False, dropout=0.0, bias=True, root_weight=True,
                 sorted_dst=False):
        super().__init__()
        in_src, in_dst = _as_pair(in_channels)
        self.sorted_dst = sorted_dst
        self.heads = heads
        self.out_channels = out_channels
        self.concat = concat
        self.beta = beta
        self.dropout = dropout
        self.root_weight = root_weight
        self.lin_key = QLinear(in_src, heads * out_channels)
        self.lin_query = QLinear(in_dst, heads * out_channels)
        self.lin_value = QLinear(in_src, heads * out_channels)
        out_dim = heads * out_channels if concat else out_channels
        self.lin_skip = QLinear(in_dst, out_dim, bias=bias)
        # as in PyG, lin_skip (and lin_beta with beta) exist whatever
        # root_weight says and are unused without it
        self.lin_beta = QLinear(3 * out_dim, 1, bias=False) if beta else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value,
                    self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def _fused_ok(self, q, dst):
        H, C = self.heads, self.out_channels
        return (self.sorted_dst and q.is_cuda and dst.numel() > 0
                and q.dtype in (torch.float32, torch.bfloat16)
                and C % 4 == 0 and H * C <= _ext.tconv_max_dim()
                and not (self.training and self.dropout > 0))

    def forward(self, x, edge_index, size: Tuple[int, int] = None):
        x_src, x_dst = _as_pair(x)
        src, dst = edge_index[0], edge_index[1]
        H, C = self.heads, self.out_channels
        n_dst = x_dst.size(0) if size is None else int(size[1])

        q = self.lin_query(x_dst)
        # keys and values in one pass over x_src, the largest matrix of a
        # step: row i is [lin_key(x_src)[i], lin_value(x_src)[i]]
        kv = _qlinear(
            x_src, torch.cat([self.lin_key.weight, self.lin_value.weight]),
            torch.cat([self.lin_key.bias, self.lin_value.bias]))

        if self._fused_ok(q, dst):
            out = _TConvAttn.apply(q, kv, src,
                                   _dst_ptr_for(edge_index, n_dst), H)
            out = out if self.concat else out.view(n_dst, H, C).mean(1)
        else:
            k3 = kv[:, :H * C].view(-1, H, C)
            v3 = kv[:, H * C:].view(-1, H, C)
            alpha = (q.view(-1, H, C)[dst] * k3[src]).sum(-1) / C ** 0.5
            # segment softmax over the incoming edges of each dst
            amax = torch.full((n_dst, H), float("-inf"), dtype=alpha.dtype,
                              device=alpha.device)
            amax = amax.scatter_reduce(
                0, dst.unsqueeze(-1).expand_as(alpha), alpha, reduce="amax",
                include_self=True)
            alpha = (alpha - amax[dst]).exp()
            denom = torch.zeros((n_dst, H), dtype=alpha.dtype,
                                device=alpha.device)
            denom.index_add_(0, dst, alpha)
            alpha = alpha / denom[dst].clamp(min=1e-16)
            if self.training and self.dropout > 0:
                alpha = F.dropout(alpha, p=self.dropout)
            out = torch.zeros((n_dst, H, C), dtype=kv.dtype,
                              device=kv.device)
            out.index_add_(0, dst, v3[src] * alpha.unsqueeze(-1))
            out = (out.reshape(n_dst, H * C) if self.concat
                   else out.mean(1))
        if self.root_weight:
            x_r = self.lin_skip(x_dst)
            if self.lin_beta is not None:
                b = torch.sigmoid(
                    self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return out


class GraphSAGE(nn.Module):
    """Multi-layer GraphSAGE matching the reference examples' training/
    inference loop (forward(x, adjs) over per-hop bipartite graphs)."""

    def __init__(self, in_channels, hidden_channels, out_channels,
                 num_layers=3, dropout=0.5, sorted_dst=True):
        super().__init__()
        self.num_layers = num_layers
        self.dropout = dropout
        self.convs = nn.ModuleList()
        # sorted_dst: GraphSageSampler emits dst-sorted adjs -> fused kernel
        if num_layers == 1:
            self.convs.append(SAGEConv(in_channels, out_channels,
                                       sorted_dst=sorted_dst))
        else:
            self.convs.append(SAGEConv(in_channels, hidden_channels,
                                       sorted_dst=sorted_dst))
            for _ in range(num_layers - 2):
                self.convs.append(SAGEConv(hidden_channels, hidden_channels,
                                           sorted_dst=sorted_dst))
            self.convs.append(SAGEConv(hidden_channels, out_channels,
                                       sorted_dst=sorted_dst))

    def forward(self, x, adjs):
        for i, (edge_index, _, size) in enumerate(adjs):
            x_target = x[:size[1]]
            x = self.convs[i]((x, x_target), edge_index, size)
            if i != self.num_layers - 1:
                x = F.relu(x, inplace=True)
                if self.dropout > 0:
                    x = F.dropout(x, p=self.dropout, training=self.training)
        return torch.log_softmax(x, dim=-1)

    def full_forward(self, x, edge_index):
        n = x.size(0)
        # fused segment path needs dst-sorted edges; sort once up front
        order = torch.argsort(edge_index[1], stable=True)
        edge_index = edge_index[:, order]
        for i, conv in enumerate(self.convs):
            x = conv((x, x), edge_index, (n, n))
            if i != self.num_layers - 1:
                x = F.relu(x)
        return torch.log_softmax(x, dim=-1)


class GAT(nn.Module):
    def __init__(self, in_channels, hidden_channels, out_channels,
                 num_layers=2, heads=4, dropout=0.5, sorted_dst=True,
                 v2=False, edge_dim=None):
        super().__init__()
        if edge_dim is not None and not v2:
            raise ValueError("GAT: edge_dim needs v2=True (GATConv takes no "
                             "edge features)")
        self.num_layers = num_layers
        self.dropout = dropout
        self.convs = nn.ModuleList()
        conv = GATv2Conv if v2 else GATConv
        if edge_dim is not None:
            conv = functools.partial(GATv2Conv, edge_dim=edge_dim)
        # sorted_dst: GraphSageSampler emits dst-sorted adjs -> fused kernel
        if num_layers == 1:
            self.convs.append(conv(in_channels, out_channels, heads=1,
                                   sorted_dst=sorted_dst))
        else:
            self.convs.append(conv(in_channels, hidden_channels,
                                   heads=heads, sorted_dst=sorted_dst))
            for _ in range(num_layers - 2):
                self.convs.append(conv(hidden_channels * heads,
                                       hidden_channels, heads=heads,
                                       sorted_dst=sorted_dst))
            self.convs.append(conv(hidden_channels * heads, out_channels,
                                   heads=1, sorted_dst=sorted_dst))

    def forward(self, x, adjs, edge_attr=None):
        """edge_attr: the graph's edge-feature table; each layer reads the
        rows named by its hop's Adj.e_id, so the sampler must be built with
        return_eid=True."""
        for i, (edge_index, e_id, size) in enumerate(adjs):
            x_target = x[:size[1]]
            if edge_attr is None:
                x = self.convs[i]((x, x_target), edge_index, size)
            else:
                if e_id.numel() == 0 and edge_index.size(1) > 0:
                    raise ValueError(
                        "GAT: edge_attr given but Adj.e_id is empty; build "
                        "the sampler with return_eid=True")
                x = self.convs[i]((x, x_target), edge_index, size,
                                  edge_attr=edge_attr, edge_id=e_id)
            if i != self.num_layers - 1:
                x = F.elu(x, inplace=True)
                if self.dropout > 0:
                    x = F.dropout(x, p=self.dropout, training=self.training)
        return torch.log_softmax(x, dim=-1)


class GraphTransformer(nn.Module):
    """Multi-layer TransformerConv model (the UniMP stack without label
    propagation), shaped like GAT: hidden layers concatenate `heads` heads,
    the output layer has one."""

    def __init__(self, in_channels, hidden_channels, out_channels,
                 num_layers=2, heads=4, dropout=0.5, beta=True,
                 sorted_dst=True):
        super().__init__()
        self.num_layers = num_layers
        self.dropout = dropout
        self.convs = nn.ModuleList()
        conv = functools.partial(TransformerConv, beta=beta,
                                 sorted_dst=sorted_dst)
        # sorted_dst: GraphSageSampler emits dst-sorted adjs -> fused kernel
        if num_layers == 1:
            self.convs.append(conv(in_channels, out_channels, heads=1))
        else:
            self.convs.append(conv(in_channels, hidden_channels, heads=heads))
            for _ in range(num_layers - 2):
                self.convs.append(conv(hidden_channels * heads,
                                       hidden_channels, heads=heads))
            self.convs.append(conv(hidden_channels * heads, out_channels,
                                   heads=1))

    def forward(self, x, adjs):
        for i, (edge_index, _, size) in enumerate(adjs):
            x_target = x[:size[1]]
            x = self.convs[i]((x, x_target), edge_index, size)
            if i != self.num_layers - 1:
                x = F.relu(x, inplace=True)
                if self.dropout > 0:
                    x = F.dropout(x, p=self.dropout, training=self.training)
        return torch.log_softmax(x, dim=-1)
