"""PyG-compatible k-hop neighbor samplers.

Capability parity with reference quiver/pyg/sage_sampler.py:
  - GraphSageSampler: GPU (DMA) / UVA (zero-copy host CSR) / CPU modes,
    returns (n_id, batch_size, adjs[::-1]) with PyG's Adj convention.
  - MixedGraphSageSampler + SampleJob: CPU/GPU work-stealing for one epoch.
The native engines are the wave64 HIP kernels (csrc/sample_kernels.hip,
csrc/reindex_kernels.hip) and the at::parallel_for CPU engine.
"""
import time
from dataclasses import dataclass
from typing import Generic, NamedTuple, Tuple, TypeVar

import torch
import torch.multiprocessing as mp

from .. import _ext
from ..trace import trace_scope
from ..utils import CSRTopo

T_co = TypeVar("T_co", covariant=True)
T = TypeVar("T")

__all__ = ["GraphSageSampler", "MixedGraphSageSampler", "SampleJob", "Adj",
           "LinkBatch", "TemporalBatch"]

# attribute name, shared with quiver.nn and quiver.loader
DST_PTR_ATTR = "_quiver_dst_ptr"


def _attach_dst_ptr(edge_index, dst_ptr):
    """Hang the hop's segment pointer (the sampler's own scan of the
    per-dst sampled counts, n_dst + 1 entries) on edge_index so the
    sorted_dst layers need no searchsorted.  A plain tensor attribute:
    Adj stays a 3-tuple and consumers that copy edge_index simply fall
    back to rebuilding the pointer."""
    setattr(edge_index, DST_PTR_ATTR, dst_ptr)
    return edge_index


class Adj(NamedTuple):
    edge_index: torch.Tensor
    e_id: torch.Tensor
    size: Tuple[int, int]

    def to(self, *args, **kwargs):
        return Adj(self.edge_index.to(*args, **kwargs),
                   self.e_id.to(*args, **kwargs), self.size)


class LinkBatch(NamedTuple):
    """What GraphSageSampler.sample_links returns."""
    n_id: torch.Tensor              # as sample(): global ids, seeds first
    batch_size: int                 # number of seed nodes
    adjs: list                      # as sample()
    edge_label_index: torch.Tensor  # int64 [2, P*(1+K)], LOCAL ids into n_id
    edge_label: torch.Tensor        # float32 [P*(1+K)]: 1 for the first P
    neg_ok: torch.Tensor            # bool [P*K]


class TemporalBatch(NamedTuple):
    """What GraphSageSampler.sample_temporal returns."""
    n_id: torch.Tensor      # int64 global ids, the seeds first and in order
    batch_size: int         # number of seeds (not deduplicated)
    adjs: list              # as sample()
    batch: torch.Tensor     # int64 [len(n_id)]: seed index of each entry's tree


@dataclass(frozen=True)
class _FakeDevice(object):
    pass


@dataclass(frozen=True)
class _StopWork(object):
    pass


class GraphSageSampler:
    """K-hop CSR neighbor sampler.

    Args:
        csr_topo: quiver.CSRTopo of the graph to sample from.
        sizes: fanout per hop, e.g. [15, 10, 5].
        device: GPU id (ignored in CPU mode).
        mode: "UVA" (graph pinned in host DRAM, zero-copy sampled from the
            GPU), "GPU" (graph resident in HBM), or "CPU".
        return_eid: fill every Adj.e_id with the int64 id of the graph
            edge each edge_index column was drawn from.  Ids are COO
            positions when the topo carries an `eid` (built from an
            edge_index, or given one), else CSR slots.
        edge_weight: float tensor [E] in that same id space.  A row longer
            than the fanout then yields distinct edges drawn without
            replacement by successive sampling, each draw in proportion to
            the weights of the edges still in the row.  Weights must be
            finite and strictly positive.
        edge_time: int64 tensor [E] in that same id space; any int64 value
            is allowed.  Enables :meth:`sample_temporal` and the
            `edge_label_time` of :meth:`sample_links`.  The sampler keeps
            its own time-sorted copy of the rows (8 B per edge for the
            times, plus permuted copies of `indices` and of the id map
            unless every row is already in time order); `csr_topo` is not
            modified.  Every other method samples the same graph as
            without it; a row returned whole comes in time order.  Not
            combinable with `edge_weight`.
    """

    def __init__(self, csr_topo: CSRTopo, sizes, device=0, mode="UVA",
                 return_eid=False, edge_weight=None, edge_time=None):
        assert mode in ["UVA", "GPU", "CPU"], f"invalid mode: {mode}"
        if edge_time is not None and edge_weight is not None:
            raise ValueError("edge_time cannot be combined with edge_weight: "
                             "there is no weighted temporal draw")
        self.csr_topo = csr_topo
        self.sizes = list(sizes)
        self.mode = mode
        self.quiver = None
        self.device = device
        self.ipc_handle_ = None
        self.return_eid = bool(return_eid)
        # weights in CSR order, fp32; None = uniform draws
        self.w_csr_ = None if edge_weight is None else \
            self._csr_weights(csr_topo, edge_weight)
        # optional: keep the frontier tail ascending (monotone gather/CSR
        # addresses).  Measured ~+8% on pure PCIe gathers but e2e-neutral
        # (the extra torch ops cost what the locality saves) — off by
        # default, flip on for cold-tier-dominated workloads.
        self.sort_frontier = False
        # (indices, times, id map or None), every row sorted by time; None =
        # no edge times
        self.temporal_ = None if edge_time is None else \
            self._time_sorted(csr_topo, edge_time)

    @staticmethod
    def _time_sorted(csr_topo, edge_time):
        """Validate per-edge times and sort every CSR row by them, stably.
        Returns (indices, time, eid) in the sorted slot order; eid maps a
        sorted slot to the id it reports (None: the slot itself).  Rows
        already in time order pass the topo's own tensors through."""
        t = torch.as_tensor(edge_time).detach().cpu()
        if t.dim() != 1 or t.numel() != csr_topo.edge_count:
            raise ValueError(
                f"edge_time must have shape [{csr_topo.edge_count}] (one "
                f"time per edge), got {tuple(t.shape)}")
        if t.dtype != torch.int64:
            raise ValueError(f"edge_time must be int64, got {t.dtype}")
        if csr_topo.eid is not None:
            t = t[csr_topo.eid]
        t = t.contiguous()
        row = torch.repeat_interleave(
            torch.arange(csr_topo.node_count), csr_topo.degree)
        if bool(((t[1:] >= t[:-1]) | (row[1:] != row[:-1])).all()):
            return csr_topo.indices, t, csr_topo.eid
        order = torch.argsort(t, stable=True)
        perm = order[torch.argsort(row[order], stable=True)]
        eid = perm if csr_topo.eid is None else csr_topo.eid[perm]
        return (csr_topo.indices[perm].contiguous(), t[perm].contiguous(),
                eid.contiguous())

    @staticmethod
    def _csr_weights(csr_topo, edge_weight):
        """Validate per-edge weights and permute them to CSR order once."""
        w = torch.as_tensor(edge_weight).detach().cpu()
        if w.dim() != 1 or w.numel() != csr_topo.edge_count:
            raise ValueError(
                f"edge_weight must have shape [{csr_topo.edge_count}] (one "
                f"weight per edge), got {tuple(w.shape)}")
        if not w.is_floating_point():
            raise ValueError("edge_weight must be a float tensor")
        w = w.to(torch.float32)
        if not bool(torch.isfinite(w).all()) or not bool((w > 0).all()):
            raise ValueError(
                "edge_weight must be finite and strictly positive (checked "
                "as float32); an edge that must never be drawn has to be "
                "removed from the graph instead of given weight 0")
        if csr_topo.eid is not None:
            w = w[csr_topo.eid]
        return w.contiguous()

    def lazy_init_quiver(self):
        if self.quiver is not None:
            return
        opts = self.return_eid or self.w_csr_ is not None
        none = torch.zeros(0, dtype=torch.long)
        # the id map travels to the engine only when ids are asked for, so
        # the default keeps its memory footprint
        indices, eid = self.csr_topo.indices, self.csr_topo.eid
        if self.temporal_ is not None:
            # the engine sees the time-sorted rows, and reports ids through
            # the map that undoes the sort
            indices, _, eid = self.temporal_
        if not self.return_eid:
            eid = None
        w = self.w_csr_ if self.w_csr_ is not None \
            else torch.zeros(0, dtype=torch.float32)
        if self.mode == "CPU":
            self.device = "cpu"
            self.quiver = _ext.cpu_quiver_from_csr_array(
                self.csr_topo.indptr, indices)
            if opts:
                self.quiver.set_edge_options(
                    none if eid is None else eid, w)
            if self.temporal_ is not None:
                self.quiver.set_edge_time(self.temporal_[1], self.return_eid)
        else:
            self.device = torch.cuda.current_device()
            self.quiver = _ext.device_quiver_from_csr_array(
                self.csr_topo.indptr, indices,
                none if eid is None else eid, self.device,
                self.mode != "UVA")
            if opts:
                self.quiver.set_edge_options(w, self.return_eid)
            if self.temporal_ is not None:
                self.quiver.set_edge_time(self.temporal_[1])

    def _sample_layer(self, batch, size, with_eid):
        self.lazy_init_quiver()
        if not isinstance(batch, torch.Tensor):
            batch = torch.tensor(batch, dtype=torch.long)
        n_id = batch.to(self.device, non_blocking=False)
        size = size if size != -1 else self.csr_topo.node_count
        fn = self.quiver.sample_neighbor_eid if with_eid \
            else self.quiver.sample_neighbor
        if self.mode in ("GPU", "UVA"):
            return fn(0, n_id, size)
        return fn(n_id, size)

    def sample_layer(self, batch, size):
        out, cnt = self._sample_layer(batch, size, False)
        return out, cnt

    def sample_layer_eid(self, batch, size):
        """sample_layer plus the id of every drawn edge, aligned with the
        neighbours: (out, cnt, e_id)."""
        return self._sample_layer(batch, size, True)

    def reindex(self, inputs, outputs, counts):
        return self.quiver.reindex_single(inputs, outputs, counts)

    def _split_edges(self, edges):
        """(edge_index, e_id) from one hop's native edge tensor: [2, m], or
        with ids on [3, m] = (src, dst, id).  Views, no copy."""
        if self.return_eid:
            return edges[:2], edges[2]
        return edges, torch.tensor([])

    def sample(self, input_nodes):
        """Sample a k-hop computational graph rooted at `input_nodes`.

        Returns (n_id, batch_size, adjs) exactly as PyG's NeighborSampler:
        edge_index[0] = source local id in n_id, edge_index[1] = target.
        """
        self.lazy_init_quiver()
        if not isinstance(input_nodes, torch.Tensor):
            input_nodes = torch.tensor(input_nodes, dtype=torch.long)
        nodes = input_nodes.to(self.device)
        adjs = []
        batch_size = len(nodes)
        if (self.mode in ("GPU", "UVA") and not self.sort_frontier
                and all(s > 0 for s in self.sizes)):
            # fused native loop: zero per-hop syncs, one call per batch
            # (the python per-hop loop cost ~12 stream syncs and ~40 torch
            # ops; the training step was launch-bound)
            with trace_scope("sampler.sample_hops"):
                hops = self.quiver.sample_hops_ptr(nodes, self.sizes)
            prev_n = nodes.size(0)
            for frontier, edges, dst_ptr in hops:
                # edges is emitted by the native chain as one [2, m]
                # tensor (edges[0]=src local, edges[1]=dst local): no
                # stack copy here
                edge_index, e_id = self._split_edges(edges)
                _attach_dst_ptr(edge_index, dst_ptr)
                adj_size = torch.LongTensor([frontier.size(0), prev_n])
                adjs.append(Adj(edge_index, e_id, adj_size))
                prev_n = frontier.size(0)
            return frontier, batch_size, adjs[::-1]
        for size in self.sizes:
            e_id = torch.tensor([])
            with trace_scope("sampler.sample_layer"):
                if self.return_eid:
                    out, cnt, e_id = self.sample_layer_eid(nodes, size)
                else:
                    out, cnt = self.sample_layer(nodes, size)
            with trace_scope("sampler.reindex"):
                frontier, row_idx, col_idx = self.reindex(nodes, out, cnt)
            if self.sort_frontier:
                bs0 = nodes.size(0)
                u = frontier.numel()
                if u > bs0:
                    tail, perm = torch.sort(frontier[bs0:])
                    frontier = torch.cat([frontier[:bs0], tail])
                    inv = torch.empty(u, dtype=torch.long,
                                      device=frontier.device)
                    inv[:bs0] = torch.arange(bs0, device=frontier.device)
                    inv[bs0 + perm] = torch.arange(bs0, u,
                                                   device=frontier.device)
                    col_idx = inv[col_idx]
            row_idx, col_idx = col_idx, row_idx
            edge_index = torch.stack([row_idx, col_idx], dim=0)
            adj_size = torch.LongTensor([frontier.size(0), nodes.size(0)])
            adjs.append(Adj(edge_index, e_id, adj_size))
            nodes = frontier
        return nodes, batch_size, adjs[::-1]

    def sample_temporal(self, seeds, seed_time):
        """Sample one k-hop tree per seed that holds only edges which
        existed by the seed's time bound.

        Args:
            seeds: int64 [B] node ids; not deduplicated, a node given twice
                roots two trees.
            seed_time: int64 [B], CPU or GPU.  An edge e is eligible under
                seed i iff edge_time[e] <= seed_time[i], at every hop of
                the seed's tree.  Pass t - 1 to exclude an event at t.

        A node with m eligible edges yields all of them, in ascending time
        order (ties in CSR order), when m is at most the fanout, else
        `fanout` distinct ones, every subset equally likely.  A fanout of
        -1 takes all eligible edges.

        Trees are disjoint: a node reached under two seeds appears twice in
        `n_id`, once per seed; within one tree it appears once.  Returns
        TemporalBatch(n_id, batch_size, adjs, batch): `n_id[:B] == seeds`,
        `batch[j]` is the index of the seed whose tree holds `n_id[j]`,
        `adjs` is laid out as :meth:`sample` returns it, both endpoints of
        every edge in one tree.  Needs a sampler built with `edge_time`.
        """
        if self.temporal_ is None:
            raise ValueError("sample_temporal needs a sampler built with "
                             "edge_time")
        self.lazy_init_quiver()
        if not isinstance(seeds, torch.Tensor):
            seeds = torch.tensor(seeds, dtype=torch.long)
        self._check_ids(seeds, "seeds", (None,))
        seed_time = torch.as_tensor(seed_time)
        b = seeds.numel()
        if seed_time.dtype != torch.int64 or tuple(seed_time.shape) != (b,):
            raise ValueError(
                f"seed_time must be int64 of shape [{b}] (one bound per "
                f"seed), got {seed_time.dtype} {tuple(seed_time.shape)}")
        n = self.csr_topo.node_count
        if b * n >= 2 ** 62:
            raise ValueError(f"{b} seeds on {n} nodes: the (seed, node) "
                             "keys do not fit 62 bits")
        seeds = seeds.to(self.device)
        seed_time = seed_time.to(self.device).contiguous()
        # node v in the tree of seed i is the key i * n + v: the frontier
        # is deduplicated per tree by the ordinary reindex
        keys = torch.arange(b, device=seeds.device) * n + seeds
        adjs = []
        for size in self.sizes:
            with trace_scope("sampler.sample_layer"):
                out, cnt, e_id = self.quiver.sample_neighbor_temporal(
                    keys, seed_time, int(size))
            with trace_scope("sampler.reindex"):
                frontier, row_idx, col_idx = self.reindex(keys, out, cnt)
            edge_index = torch.stack([col_idx, row_idx], dim=0)
            adj_size = torch.LongTensor([frontier.size(0), keys.size(0)])
            adjs.append(Adj(edge_index,
                            e_id if self.return_eid else torch.tensor([]),
                            adj_size))
            keys = frontier
        return TemporalBatch(keys % n, b, adjs[::-1],
                             torch.div(keys, n, rounding_mode="floor"))

    def _check_ids(self, ids, name, shape):
        """int64 node ids of the wanted rank; the id range is checked on a
        CPU input only (on a GPU one it would cost a sync)."""
        if ids.dtype != torch.int64:
            raise ValueError(f"{name} must be int64, got {ids.dtype}")
        if ids.dim() != len(shape) or any(
                want is not None and got != want
                for got, want in zip(ids.shape, shape)):
            raise ValueError(f"{name} must have shape {shape} (None = any), "
                             f"got {tuple(ids.shape)}")
        if ids.device.type == "cpu" and ids.numel() > 0:
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.csr_topo.node_count:
                raise ValueError(
                    f"{name} holds ids outside [0, "
                    f"{self.csr_topo.node_count}): min {lo}, max {hi}")

    def sample_negative(self, src, num_neg=1, neg_tries=16):
        """Draw `num_neg` negative tails for every source node in `src`.

        A tail is drawn uniformly from all nodes and redrawn, up to
        `neg_tries` candidates in all, while it is the source itself or
        one of the source's out-neighbours (on a symmetrised graph that
        covers both directions).  A source that occurs several times in
        `src` draws independently each time.

        Returns (neg int64 [P, num_neg], ok bool [P, num_neg]) on the
        sampler's device.  ok == False marks a tail whose `neg_tries`
        candidates were all rejected: the value is a valid node id but may
        be a real edge or the source.
        """
        self.lazy_init_quiver()
        if not isinstance(src, torch.Tensor):
            src = torch.tensor(src, dtype=torch.long)
        self._check_ids(src, "src", (None,))
        if num_neg < 1 or neg_tries < 1:
            raise ValueError("num_neg and neg_tries must be >= 1")
        src = src.to(self.device).contiguous()
        return self.quiver.sample_negative(src, int(num_neg), int(neg_tries))

    def sample_links(self, edge_label_index, num_neg=1, neg_tries=16,
                     edge_label_time=None):
        """One link-prediction batch: the positive edges given, `num_neg`
        sampled negatives for each, and the k-hop computational graph of
        all their endpoints.

        Args:
            edge_label_index: int64 [2, P] global ids (src row, dst row) of
                the positive edges, a tensor or a (src, dst) pair.
            num_neg: negative tails per positive edge, drawn with
                :meth:`sample_negative` from the positive's source.  0
                gives the positives only.
            neg_tries: candidates per negative before it is given up.
            edge_label_time: int64 [P], the time of every positive; needs a
                sampler built with `edge_time`.  See "Temporal" below.

        Returns a LinkBatch.  `n_id`, `batch_size` and `adjs` are what
        :meth:`sample` returns for the seed nodes, the distinct endpoints
        of all positives and negatives.  `edge_label_index` holds LOCAL
        ids into `n_id`: the P positives in input order, then the
        negatives of edge 0, of edge 1, ..., each with its positive's
        source as head.  `edge_label` is 1 for the positives and 0 after.

        Two things are left to the caller:
          (a) The positives' own edges may appear in `adjs`, the message
              graph.  Who must exclude them builds the sampler with
              return_eid=True and masks the hops by `Adj.e_id`.
          (b) `neg_ok[i] == False` marks a negative whose `neg_tries`
              candidates were all rejected; it may be a real edge, or the
              source itself.  Mask the loss with `neg_ok` where that
              matters (near-complete rows only).

        Temporal: with `edge_label_time` the endpoints are not merged.
        The seeds are cat[src, dst, negatives], P * (2 + num_neg) of them,
        each the root of its own tree through :meth:`sample_temporal` with
        the time of its positive as bound (a negative inherits its
        positive's), so `batch_size == P * (2 + num_neg)` and
        `edge_label_index` holds seed positions: head i for positive i and
        for its negatives, tails P + i and 2P + i * num_neg + j.  The
        bound is inclusive: pass t - 1 to keep an event at t out of its
        own message graph.  Negatives are still rejected against the
        source's whole row, whatever the times of its edges: a tail that
        becomes a neighbour only later is not drawn either.
        """
        self.lazy_init_quiver()
        if not isinstance(edge_label_index, torch.Tensor):
            if len(edge_label_index) != 2:
                raise ValueError("edge_label_index must be [2, P] or a "
                                 "(src, dst) pair")
            edge_label_index = torch.stack(
                [torch.as_tensor(e) for e in edge_label_index])
        self._check_ids(edge_label_index, "edge_label_index", (2, None))
        if num_neg < 0 or neg_tries < 1:
            raise ValueError("num_neg must be >= 0 and neg_tries >= 1")
        pos = edge_label_index.to(self.device)
        src, dst = pos[0].contiguous(), pos[1]
        p = src.numel()
        if p == 0:
            raise ValueError("edge_label_index holds no edge")
        if edge_label_time is not None:
            if self.temporal_ is None:
                raise ValueError("edge_label_time needs a sampler built "
                                 "with edge_time")
            t = torch.as_tensor(edge_label_time)
            if t.dtype != torch.int64 or tuple(t.shape) != (p,):
                raise ValueError(
                    f"edge_label_time must be int64 of shape [{p}], got "
                    f"{t.dtype} {tuple(t.shape)}")
            t = t.to(self.device)
        if num_neg > 0:
            with trace_scope("sampler.sample_negative"):
                neg, ok = self.quiver.sample_negative(src, int(num_neg),
                                                      int(neg_tries))
            ends = torch.cat([src, dst, neg.reshape(-1)])
            neg_ok = ok.reshape(-1)
        else:
            ends = torch.cat([src, dst])
            neg_ok = torch.zeros(0, dtype=torch.bool, device=ends.device)
        if edge_label_time is not None:
            # every endpoint roots its own tree: a seed's position is its
            # local id
            n_id, batch_size, adjs, _ = self.sample_temporal(
                ends, torch.cat([t, t, t.repeat_interleave(int(num_neg))]))
            local = torch.arange(ends.numel(), device=ends.device)
        else:
            # distinct endpoints as seeds: sample() keeps its seeds first
            # and in order, so a seed's position is its local id
            seeds, local = torch.unique(ends, return_inverse=True)
            n_id, batch_size, adjs = self.sample(seeds)
        head = torch.cat([local[:p],
                          local[:p].repeat_interleave(int(num_neg))])
        tail = local[p:]
        label = torch.zeros(head.numel(), dtype=torch.float32,
                            device=ends.device)
        label[:p] = 1
        return LinkBatch(n_id, batch_size, adjs, torch.stack([head, tail]),
                         label, neg_ok)

    def sample_async(self, input_nodes):
        """Enqueue one full multi-hop sample with ZERO host syncs.

        Returns a token for :meth:`sample_finalize`.  The per-hop tensors
        in the token are upper-bound sized; exact sizes land in a pinned
        host buffer via an async D2H, valid once the enqueueing stream's
        work for this batch completes (callers order with an event).
        GPU/UVA modes with positive fanouts only.
        """
        self.lazy_init_quiver()
        if self.mode not in ("GPU", "UVA") or not all(
                s > 0 for s in self.sizes):
            raise RuntimeError("sample_async requires GPU/UVA mode with "
                               "positive fanouts")
        if not isinstance(input_nodes, torch.Tensor):
            input_nodes = torch.tensor(input_nodes, dtype=torch.long)
        nodes = input_nodes.to(self.device)
        raw, sizes_dev, ptrs = self.quiver.sample_hops_raw(nodes, self.sizes)
        sizes_pin = torch.empty(sizes_dev.numel(), dtype=torch.int64,
                                pin_memory=True)
        sizes_pin.copy_(sizes_dev, non_blocking=True)
        return (nodes, raw, sizes_dev, sizes_pin, ptrs)

    def sample_finalize(self, token):
        """Build (n_id, batch_size, adjs) from a sample_async token.

        The caller must have synchronized with the producing stream (e.g.
        event.synchronize()) so the pinned sizes are valid.
        """
        nodes, raw, _sizes_dev, sizes_pin = token[:4]
        ptrs = token[4] if len(token) > 4 else None
        adjs = []
        prev = nodes.size(0)
        frontier = nodes
        for h, (f_ub, e_ub) in enumerate(raw):
            m = int(sizes_pin[2 * h])
            u = int(sizes_pin[2 * h + 1])
            frontier = f_ub[:u]
            # zero-copy: a narrowed view of the upper-bound edge buffer
            edge_index, e_id = self._split_edges(e_ub.narrow(1, 0, m))
            if ptrs is not None:
                # upper-bound-sized scan; its first prev + 1 entries are
                # this hop's segment pointer
                _attach_dst_ptr(edge_index, ptrs[h].narrow(0, 0, prev + 1))
            adjs.append(Adj(edge_index, e_id, torch.LongTensor([u, prev])))
            prev = u
        return frontier, nodes.size(0), adjs[::-1]

    def sample_prob(self, train_idx, total_node_count):
        """Multi-hop access probability of every node when seeding from
        train_idx — drives access-probability feature placement.

        The propagation formula (reference cal_next,
        cuda_random.cu.hpp:71-104) reads each node's CSR row as BOTH its
        out- and in-edges, i.e. it assumes a symmetrized graph — true for
        the OGB/Reddit datasets the reference targets.  On a directed
        graph the propagation runs against edge direction and the
        resulting placement can be badly mis-ranked."""
        self.lazy_init_quiver()
        if self.mode == "CPU":
            raise RuntimeError("sample_prob needs a GPU sampler")
        last_prob = torch.zeros(total_node_count, device=self.device)
        last_prob[train_idx] = 1
        for size in self.sizes:
            cur_prob = torch.zeros(total_node_count, device=self.device)
            self.quiver.cal_neighbor_prob(0, last_prob, cur_prob, size)
            last_prob = cur_prob
        return last_prob

    def share_ipc(self):
        if self.temporal_ is not None:
            # the time-sorted rows travel in shared memory: a worker does
            # not sort again
            for x in self.temporal_:
                if x is not None:
                    x.share_memory_()
            return (self.csr_topo, self.sizes, self.mode, self.return_eid,
                    None, self.temporal_)
        if not self.return_eid and self.w_csr_ is None:
            return self.csr_topo, self.sizes, self.mode
        if self.w_csr_ is not None:
            self.w_csr_.share_memory_()
        return (self.csr_topo, self.sizes, self.mode, self.return_eid,
                self.w_csr_)

    @classmethod
    def lazy_from_ipc_handle(cls, ipc_handle):
        csr_topo, sizes, mode = ipc_handle[:3]
        return_eid, w_csr = ipc_handle[3:5] if len(ipc_handle) > 3 \
            else (False, None)
        sampler = cls(csr_topo, sizes, _FakeDevice, mode,
                      return_eid=return_eid)
        # validated and permuted to CSR order by the sharing process
        sampler.w_csr_ = w_csr
        if len(ipc_handle) > 5:
            sampler.temporal_ = tuple(ipc_handle[5])
        return sampler


class SampleJob(Generic[T_co]):
    """Abstract job list for MixedGraphSageSampler."""

    def __getitem__(self, index) -> T_co:
        raise NotImplementedError

    def __len__(self) -> int:
        raise NotImplementedError

    def shuffle(self) -> None:
        raise NotImplementedError


def cpu_sampler_worker_loop(rank, quiver_sampler, task_queue, result_queue):
    import torch as _torch
    _torch.set_num_threads(1)  # pool parallelism comes from worker count
    while True:
        task = task_queue.get()
        if isinstance(task, _StopWork):
            result_queue.put(_StopWork())
            break
        t0 = time.time()
        res = quiver_sampler.sample(task)
        result_queue.put((res, time.time() - t0))


class MixedGraphSageSampler:
    """CPU+GPU work-stealing sampler over a SampleJob for one epoch.

    Modes: UVA_CPU_MIXED / GPU_CPU_MIXED (adaptive split between the device
    sampler and a pool of CPU sampler processes) and UVA_ONLY / GPU_ONLY.
    Mirrors reference sage_sampler.py:207-376.
    """

    def __init__(self, sample_job: SampleJob, num_workers, csr_topo: CSRTopo,
                 sizes, device=0, mode="UVA_CPU_MIXED", return_eid=False,
                 edge_weight=None, edge_time=None):
        assert mode in ["UVA_CPU_MIXED", "GPU_CPU_MIXED", "UVA_ONLY",
                        "GPU_ONLY"], f"invalid mode: {mode}"
        if edge_time is not None:
            raise ValueError("MixedGraphSageSampler has no temporal "
                             "sampling; use GraphSageSampler.sample_temporal")
        # return_eid / edge_weight: as GraphSageSampler, applied to the
        # device sampler and the CPU sampler alike
        self.return_eid = bool(return_eid)
        self.w_csr_ = None if edge_weight is None else \
            GraphSageSampler._csr_weights(csr_topo, edge_weight)
        self.sample_job = sample_job
        self.num_workers = num_workers
        self.csr_topo = csr_topo
        self.sizes = list(sizes)
        self.mode = mode
        self.device = device
        self.device_sampler = None
        self.cpu_sampler = None
        self.workers = []
        self.task_queues = []
        self.result_queue = None
        self.inited = False

    def lazy_init(self):
        if self.inited:
            return
        dev_mode = "UVA" if self.mode.startswith("UVA") else "GPU"
        self.device_sampler = GraphSageSampler(self.csr_topo, self.sizes,
                                               self.device, dev_mode,
                                               return_eid=self.return_eid)
        # already validated and in CSR order
        self.device_sampler.w_csr_ = self.w_csr_
        if self.mode.endswith("MIXED"):
            self.cpu_sampler = GraphSageSampler(self.csr_topo, self.sizes,
                                                mode="CPU",
                                                return_eid=self.return_eid)
            self.cpu_sampler.w_csr_ = self.w_csr_
            ctx = mp.get_context("spawn")
            self.result_queue = ctx.Queue()
            for w in range(self.num_workers):
                q = ctx.Queue()
                p = ctx.Process(target=cpu_sampler_worker_loop,
                                args=(w, self.cpu_sampler, q,
                                      self.result_queue),
                                daemon=True)
                p.start()
                self.task_queues.append(q)
                self.workers.append(p)
        self.inited = True

    def decide_task_num(self, dev_time, dev_tasks, cpu_service, cpu_tasks):
        """How many tasks to hand the CPU pool per GPU inline task.

        Measured-time split (reference sage_sampler.py:272-288): the pool
        can finish num_workers * t_dev / t_cpu tasks while the device
        samples one; half that keeps the tail from ending on a slow CPU
        task.  Until both sides have measurements, seed every worker one
        task so the first estimate exists.
        """
        if cpu_tasks == 0 or dev_tasks == 0:
            return max(1, self.num_workers)
        t_dev = dev_time / dev_tasks          # device seconds per task
        t_cpu = cpu_service / cpu_tasks       # ONE worker's seconds per task
        return max(0, int(self.num_workers * t_dev / max(t_cpu, 1e-9) / 2))

    def __iter__(self):
        self.lazy_init()
        self.sample_job.shuffle()
        return self.iter_sampler()

    def iter_sampler(self):
        n = len(self.sample_job)
        next_task = 0
        pending_cpu = 0
        dev_time, dev_done = 0.0, 0
        cpu_service, cpu_done = 0.0, 0   # summed per-task worker seconds
        rr = 0                           # round-robin worker cursor
        try:
            while next_task < n or pending_cpu > 0:
                # hand a slice to CPU workers (round-robin so the pool
                # load-balances instead of piling on worker 0)
                if self.task_queues and next_task < n:
                    want = self.decide_task_num(dev_time, dev_done,
                                                cpu_service, cpu_done)
                    # cap queue depth: a task handed out now is committed
                    # even if the measured rates later say otherwise
                    want = min(want, n - next_task,
                               2 * len(self.task_queues) - pending_cpu)
                    for _ in range(max(0, want)):
                        self.task_queues[rr % len(self.task_queues)].put(
                            self.sample_job[next_task])
                        rr += 1
                        next_task += 1
                        pending_cpu += 1
                # GPU samples inline
                if next_task < n:
                    t0 = time.time()
                    res = self.device_sampler.sample(
                        self.sample_job[next_task])
                    dev_time += time.time() - t0
                    dev_done += 1
                    next_task += 1
                    yield res
                # drain CPU results
                while pending_cpu > 0:
                    try:
                        res = self.result_queue.get(
                            block=(next_task >= n))
                    except Exception:
                        break
                    if isinstance(res, _StopWork):
                        continue
                    if isinstance(res, tuple) and len(res) == 2 \
                            and isinstance(res[1], float):
                        res, dt = res
                        cpu_service += dt
                    pending_cpu -= 1
                    cpu_done += 1
                    yield res
                    if next_task < n:
                        break
        finally:
            pass

    def shutdown(self):
        for q in self.task_queues:
            q.put(_StopWork())
        for p in self.workers:
            p.join(timeout=5)
            if p.is_alive():
                p.terminate()
        self.workers = []
        self.task_queues = []
        self.inited = False

    def share_ipc(self):
        handle = (self.sample_job, self.num_workers, self.csr_topo,
                  self.sizes, self.device, self.mode)
        if not self.return_eid and self.w_csr_ is None:
            return handle
        if self.w_csr_ is not None:
            self.w_csr_.share_memory_()
        return handle + (self.return_eid, self.w_csr_)

    @classmethod
    def lazy_from_ipc_handle(cls, ipc_handle):
        sampler = cls(*ipc_handle[:6])
        if len(ipc_handle) > 6:
            sampler.return_eid, sampler.w_csr_ = ipc_handle[6:]
        return sampler
