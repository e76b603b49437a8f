#!/usr/bin/env python3
"""Training / profiling harness - the host-side mirror of the reference's main_tcgnn.py.

Same flags (main_tcgnn.py:18-27), same flow (load -> preprocess -> move metadata -> model ->
9 warm-up + `--epochs` timed train steps, or `--single_kernel` SAG profile), same stdout lines
(`Prep. (ms):\\t%.3f`, `Train (ms):\\t%6.3f`, `=> SAG profiling avg (ms): %.3f`), so the reference's
1_bench_gcn.py / 2_tcgnn_single_kernel.py / 1_log2csv.py drive and scrape it unchanged.

Additions: `--synthetic <shape>` builds a seeded graph of a named shape (no dataset files exist on
the GPU box), `--graph_dir` relocates tcgnn-ae-graphs/, `--gpu_preprocess` uses the device SGT.
`run(args)` returns the measured numbers so bench.py and the tests can call it in-process.
"""
import argparse
import os
import os.path as osp
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

BLK_H, BLK_W = 16, 8  # config.py:1-2
# f3: a GCN layer that WIDENS (the classifier at the artifact's hidden = 16: 16 -> 22 .. 121 classes) is evaluated as (A H) W in
# one launch (tcgnn_spmm_gemm: aggregation at the narrow width, dense update in the kernel's epilogue) instead of A (H W) - the
# same matrix, fewer columns through the aggregation.  "auto": exactly those layers; "1" / "0": every eligible layer / none.
AGGREGATE_FIRST = os.environ.get("TCGNN_AGGREGATE_FIRST", "auto")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--dataset", type=str, default="amazon0601", help="dataset")
    p.add_argument("--dim", type=int, default=96, help="input embedding dimension")
    p.add_argument("--num_layers", type=int, default=2, help="num layers")
    p.add_argument("--hidden", type=int, default=16, help="hidden dimension")
    p.add_argument("--classes", type=int, default=22, help="number of output classes")
    p.add_argument("--epochs", type=int, default=200, help="number of epoches")
    p.add_argument("--model", type=str, default="gcn", help="GNN model", choices=["gcn", "gin", "agnn", "gat", "gatv2", "sage", "transformer", "pna", "gine"])
    p.add_argument("--single_kernel", action="store_true", help="whether to profile a single SAG kernel")
    p.add_argument("--synthetic", type=str, default=None, help="named synthetic shape instead of a dataset file")
    p.add_argument("--scale", type=float, default=1.0, help="shrink a synthetic shape (N*scale, nnz*scale^2)")
    p.add_argument("--graph_dir", type=str, default="tcgnn-ae-graphs/")
    p.add_argument("--gpu_preprocess", action="store_true", help="run the sparse-graph translation on the GPU")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--generator", type=str, default="uniform", help="generator of a --synthetic shape (tcgnn_graph.GENERATORS): uniform, rmat, sbm, sbm_hubs, sbm_shuffled (the communities of sbm under random node ids)")
    p.add_argument("--reorder", action="store_true", help="relabel the nodes so that communities are contiguous (tcgnn_graph.community_order) before the sparse-graph translation; features and labels follow (not in the reference)")
    p.add_argument("--hip_graph", action="store_true", help="capture one epoch in a HIP graph after the dry epochs and replay it (not in the reference)")
    p.add_argument("--norm", type=str, default="none", choices=["none", "both", "right", "left"],
                   help="GCN only: DGL GraphConv's degree normalisation of the aggregation (not in the reference: its GCN aggregates with the binary A)")
    p.add_argument("--bias", action="store_true", help="GCN only: a learned bias per layer, fused into the aggregation's stores (not in the reference)")
    p.add_argument("--directed", action="store_true", help="a --synthetic shape built without symmetrisation (a dataset is used as stored either way), "
                   "and every layer back-propagates through A^T (directed=True; not in the reference, whose backward uses A)")
    p.add_argument("--attention", type=str, default="reference", choices=["reference", "softmax"],
                   help="AGNN only: 'softmax' normalises the cosine scores over every node's incoming edges (DGL's AGNNConv; exact gradients) - "
                   "not in the reference, whose layer aggregates with the raw scores")
    p.add_argument("--heads", type=int, default=1, help="GAT, GATv2 and transformer only: attention heads of the hidden layers, which concatenate `heads` heads of "
                   "hidden / heads features (it must divide); the output layer has one head of `classes` (not in the reference)")
    p.add_argument("--aggregator", type=str, default="mean", choices=["mean", "max", "pool"],
                   help="SAGE only: GraphSAGE's neighbour aggregation - 'mean', or the element-wise maximum over a node's incoming edges of the "
                   "features ('max') or of a learned projection of them ('pool') (not in the reference)")
    p.add_argument("--edge-dim", dest="edge_dim", type=int, default=16,
                   help="GINE only: width of the edge features; the datasets here carry none, so they are drawn once on the device from --seed (not in the reference)")
    p.add_argument("--fanout", type=str, default=None,
                   help="K[,K...]: train every epoch on a freshly sampled graph that keeps at most K in-edges per node (TCGNN.sample_neighbors, seed + epoch); "
                   "several values give one fan-out per layer, input layer first; the final loss is evaluated on the full graph (not in the reference)")
    p.add_argument("--batch-size", dest="batch_size", type=int, default=None,
                   help="B: with --fanout, mini-batch training - every epoch cuts a seeded permutation of the nodes into batches of B seeds, samples each "
                   "batch's layer graphs, relabels them to the nodes they touch (tcgnn_layers.sample_batch) and takes one optimiser step per batch on the "
                   "seeds' loss; the final loss is evaluated on the full graph (not in the reference)")
    p.add_argument("--sampler", type=str, default="dense", choices=["dense", "rows", "saint", "cluster"],
                   help="with --batch-size: 'dense' samples every hop over all rows of the graph behind a frontier mask; 'rows' samples from the list of "
                   "frontier rows (tcgnn_layers.sample_batch_rows), so a step costs its batch - the same batches, bit for bit; 'saint' (GraphSAINT) trains "
                   "on the subgraph induced on the nodes that one random walk from each of B roots visits, 'cluster' (Cluster-GCN) on the one induced on B "
                   "consecutive node ids - both without --fanout, the loss over every node of the batch (not in the reference)")
    p.add_argument("--walk-length", dest="walk_length", type=int, default=2,
                   help="--sampler saint only: steps of every root's random walk (not in the reference)")
    p.add_argument("--saint-norm", dest="saint_norm", type=int, default=0,
                   help="S: --sampler saint / cluster only - weight every node's loss by GraphSAINT's node normalisation, estimated from S batches drawn "
                   "before training (0: off; not in the reference)")
    return p


def parse_fanout(text, num_layers):
    """--fanout's value as one fan-out per layer (None: no sampling)"""
    if text is None:
        return None
    ks = [int(t) for t in str(text).split(",")] if not isinstance(text, (list, tuple)) else [int(t) for t in text]
    if len(ks) == 1:
        ks = ks * num_layers
    if len(ks) != num_layers or min(ks) < 0:
        raise ValueError("--fanout takes one value >= 0, or one per layer (%d), got %r" % (num_layers, text))
    return ks


SUBGRAPH_SAMPLERS = ("saint", "cluster")


def parse_batch_size(batch_size, fanout, hip_graph=False, sampler="dense"):
    """--batch-size's value checked against the flags it depends on (None: no mini-batches)"""
    if sampler in SUBGRAPH_SAMPLERS:
        if batch_size is None:
            raise ValueError("--sampler %s trains on induced subgraphs of --batch-size roots or node ids and needs --batch-size" % sampler)
        if fanout is not None:
            raise ValueError("--sampler %s trains on the whole induced subgraph and takes no --fanout" % sampler)
    if batch_size is None:
        return None
    if fanout is None and sampler not in SUBGRAPH_SAMPLERS:
        raise ValueError("--batch-size trains on sampled mini-batches and needs --fanout")
    if hip_graph:
        raise ValueError("--batch-size samples a new graph every step and can not be combined with --hip_graph, which replays one captured epoch")
    if int(batch_size) < 1:
        raise ValueError("--batch-size takes a value >= 1, got %r" % (batch_size,))
    return int(batch_size)


def parse_sampler(sampler, batch_size):
    """--sampler's value checked against the flag it depends on"""
    if sampler not in ("dense", "rows") + SUBGRAPH_SAMPLERS:
        raise ValueError("--sampler takes 'dense', 'rows', 'saint' or 'cluster', got %r" % (sampler,))
    if sampler == "rows" and batch_size is None:
        raise ValueError("--sampler rows samples a mini-batch from its list of rows and needs --batch-size")
    if sampler in SUBGRAPH_SAMPLERS and batch_size is None:
        raise ValueError("--sampler %s trains on induced subgraphs of --batch-size roots or node ids and needs --batch-size" % sampler)
    return sampler


def parse_walk_length(walk_length):
    """--walk-length's value"""
    if int(walk_length) < 0:
        raise ValueError("--walk-length takes a value >= 0, got %r" % (walk_length,))
    return int(walk_length)


# the seed stride of --saint-norm's dry batches: batch_seed's epoch argument, which no dry step (epoch = epochs) or timed epoch reaches
SAINT_NORM_EPOCH = 1 << 40


def epoch_order(num_nodes, seed, epoch):
    """the permutation of the nodes that epoch `epoch` cuts into batches: a function of (num_nodes, seed + epoch) alone, drawn on the host"""
    return torch.randperm(num_nodes, generator=torch.Generator().manual_seed((int(seed) + int(epoch)) % (1 << 63)))


def batch_seed(seed, epoch, index):
    """the sampling seed of batch `index` of epoch `epoch` (sample_layers draws hop h with this + h: the stride keeps batches apart)"""
    return ((int(seed) * 1000003 + int(epoch)) * 1000003 + int(index)) * 64


class Net(nn.Module):
    """conv1 -> relu -> dropout -> [hidden convs + relu] -> conv2 -> log_softmax (main_tcgnn.py:75-139)."""

    def __init__(self, conv_cls, in_dim, hidden, classes, num_layers, out_cls=None, **conv_kwargs):
        """out_cls (a GAT model: one head of `classes` behind hidden layers of several heads): what builds the output layer; None: conv_cls."""
        super().__init__()
        self.conv1 = conv_cls(in_dim, hidden, **conv_kwargs)
        self.hidden_layers = nn.ModuleList(conv_cls(hidden, hidden, **conv_kwargs) for _ in range(num_layers - 2))
        self.conv2 = (out_cls or conv_cls)(hidden, classes, **conv_kwargs)
        self.relu = nn.ReLU()

    def _act(self, conv, x, meta):
        # GCNConv can run the ReLU inside its aggregation kernel (tcgnn_layers.TCGNNFunction fuse_relu); same values
        import tcgnn_layers as L
        if isinstance(conv, L.GCNConv):
            return conv(x, *meta, fuse_relu=True)
        return self.relu(conv(x, *meta))

    def forward(self, x, meta):
        """meta: the graph's five tensors, or a sequence of such groups with one graph per layer (fan-out sampling)"""
        per_layer = list(meta) if isinstance(meta[0], (list, tuple)) else [meta] * (len(self.hidden_layers) + 2)
        meta = per_layer[-1]
        x = self._act(self.conv1, x, per_layer[0])
        x = F.dropout(x, training=self.training)
        for conv, m in zip(self.hidden_layers, per_layer[1:-1]):
            x = self._act(conv, x, m)
        import tcgnn_layers as L
        din, dout = self.conv2.weights.shape if isinstance(self.conv2, L.GCNConv) else (0, 0)   # (only GCNConv has the aggregate-first form)
        want = AGGREGATE_FIRST in (True, "1") or (AGGREGATE_FIRST == "auto" and din < dout)
        if want and isinstance(self.conv2, L.GCNConv) and max(din, dout) <= 128:
            x = self.conv2(x, *meta, aggregate_first=True)
        else:
            x = self.conv2(x, *meta)
        return F.log_softmax(x, dim=1)


def load_graph(args):
    import tcgnn_graph as G
    if args.synthetic:
        rp, col, dim, classes = G.synthetic_shape(args.synthetic, seed=args.seed, scale=args.scale, generator=getattr(args, "generator", "uniform"),
                                                   device="cuda" if torch.cuda.is_available() else "cpu", directed=getattr(args, "directed", False))
        n = rp.numel() - 1
        gen = torch.Generator().manual_seed(args.seed)
        ds = argparse.Namespace(num_nodes=n, num_edges=col.numel(), column_index=col.cpu(), row_pointers=rp.cpu(),
                                num_features=args.dim, num_classes=args.classes,
                                x=torch.randn(n, args.dim, generator=gen), y=torch.ones(n).long())
        return ds
    path = osp.join(args.graph_dir, args.dataset + ".npz")
    return G.TCGNN_dataset(path, args.dim, args.classes, load_from_txt=False, seed=args.seed)


def node_nll_loss(log_probs, y):
    """F.nll_loss(log_probs, y) of main_tcgnn.py:149 (mean over all nodes, no class weights, no ignore_index hit)
    as a gather + mean: torch's 2-D nll_loss kernels reduce N = 233k rows in ONE workgroup (0.36 ms forward +
    0.23 ms backward per Reddit epoch, 8 % of the GCN epoch, measured with rocprofv3); this form is 30x faster
    and differs only in summation order."""
    return -log_probs.gather(1, y.view(-1, 1)).mean()


def make_adam(params, lr=0.01):
    """Adam(lr=0.01, capturable=True) of main_tcgnn.py:143.  On the GPU the FUSED implementation (one kernel per step over all
    parameters) instead of torch's default foreach form: the same update, but the foreach step is ~30 launches of ~5 us each -
    0.15 ms of a 2.7 ms Reddit epoch, most of a Citeseer-sized one (profiles/r03/epoch_gcn_timeline.txt).  TCGNN_FUSED_ADAM=0
    keeps the default form."""
    params = list(params)
    if params and params[0].is_cuda and os.environ.get("TCGNN_FUSED_ADAM", "1") != "0":
        try:
            return torch.optim.Adam(params, lr=lr, capturable=True, fused=True)
        except (RuntimeError, TypeError, ValueError):   # (a torch build without the fused kernels)
            pass
    return torch.optim.Adam(params, lr=lr, capturable=True)


def time_training(model_name, meta, x, y, in_dim, hidden, classes, num_layers, epochs, seed=0, warmup=9, hip_graph=False, tune=True,
                  norm="none", bias=False, directed=False, attention="reference", heads=1, aggregator="mean", edge_dim=16, fanout=None,
                  batch_size=None, batch_hook=None, sampler="dense", walk_length=2, saint_norm=0):
    """The timed part of main_tcgnn.py (:141-181) on tensors that already live on the GPU:
    Adam(lr=0.01), nll_loss over all nodes, `warmup` dry epochs then `epochs` timed ones.
    hip_graph: capture one whole epoch (forward, loss, backward, Adam step - the reference already asks for a capturable
    Adam, main_tcgnn.py:143) in a HIP graph after the dry epochs and replay it: on Citeseer-sized graphs an epoch is
    ~60 launches of a few microseconds each and the host, not the GPU, sets the time.
    norm / bias (GCN only, not in the reference): GCNConv(norm=..., bias=...), DGL GraphConv's normalised layer.
    directed (not in the reference): every layer with directed=True (backward through A^T), and A^T's plan prepared with A's.
    attention (AGNN only, not in the reference): AGNNConv(attention=...); 'softmax' prepares A^T's plan and the edge operators' buffers.
    heads (GAT, GATv2 and transformer only, not in the reference): the hidden layers are GATConv / GATv2Conv / TransformerConv(., hidden / heads, heads=heads) -
    concatenated back to `hidden` - and the output layer is one head of `classes`; A^T's plan and the edge operators' buffers are prepared at the per-head widths.
    aggregator (SAGE only, not in the reference): SAGEConv(aggregator=...); 'max' and 'pool' prepare the transposed CSR their backward walks.
    model 'pna' (not in the reference): PNAConv layers with their default aggregators and scalers; the transposed CSR is prepared as for SAGE's max.
    model 'gine' (not in the reference): GINEConv layers with edge_dim=edge_dim; no dataset here has edge features, so edge_attr [E, edge_dim] is drawn
    ONCE, standard normal, from a generator on the device seeded with `seed`, and every layer reads it; the transposed CSR is prepared as for SAGE's max.
    fanout (not in the reference; None: the path above, unchanged): a list of one fan-out per layer.  Every epoch, dry ones included, draws
    tcgnn_layers.sample_meta(meta, k, seed + epoch) per distinct k, builds what the model's operators need on it (the plan at every width and,
    for the layers with a `directed` switch, A^T's - a sampled graph is not symmetric, so those layers are built with directed=True - or, for
    the planless models, only the transposed CSR) and trains on it; GINE gathers edge_attr[eid].  The three parts are timed apart, each
    behind a device synchronisation: the result holds sample_ms, plan_ms and train_ms per epoch and their sum epoch_ms.  Plans are created
    every epoch: that cost is plan_ms, not hidden.  final_loss is the loss on the FULL graph after the last step (model.eval()).  Refused
    together with hip_graph: a captured epoch replays one graph.
    batch_size (not in the reference; None: the paths above, unchanged; needs fanout): mini-batch training.  Every timed epoch draws
    epoch_order(N, seed, epoch) and cuts it into batches of batch_size seeds - every node is a seed exactly once per epoch.  Per batch:
    tcgnn_layers.sample_layers with batch_seed(seed, epoch, index), compact_layers (the two halves of sample_batch, timed apart), x[nodes]
    (and, for GINE, edge_attr[eid]), what the model's operators need on the compact graphs, and ONE optimiser step on
    node_nll_loss(out[seed_pos], y[seeds]).  `warmup` counts dry STEPS here (batches of a permutation no timed epoch uses), not epochs.
    The result holds sample_ms, compact_ms, plan_ms and train_ms per epoch (each behind a device synchronisation), their sum epoch_ms,
    batches (per epoch), mean_block_nodes (the mean M) and final_loss on the FULL graph.  batch_hook(epoch, index, seeds), when given, is
    called before every timed step.  Refused together with hip_graph.
    sampler (not in the reference; needs batch_size for 'rows'): 'dense' is the step above; 'rows' draws the same batch through
    tcgnn_layers.sample_layers_rows and compact_layers_rows (the two halves of sample_batch_rows, timed apart as sample_ms and compact_ms):
    the sampler runs over the batch's rows, not over all N.  The batches, and with them every loss, are bit-equal.
    sampler 'saint' / 'cluster' (not in the reference; need batch_size, refuse fanout and hip_graph): subgraph sampling.  A batch is the
    subgraph the full graph induces on a node set (tcgnn_layers.subgraph_batch: ONE square block that every layer runs on, built and
    prepared once per batch), and the loss runs over ALL M rows of it, against y[batch.nodes].  'saint': every timed epoch cuts
    epoch_order(N, seed, epoch) into batches of batch_size ROOTS; the node set is what one walk of walk_length steps from every root
    visits (the backend's random_walk with batch_seed(seed, epoch, index)).  'cluster': the node ids are cut into ceil(N / batch_size)
    ranges of batch_size consecutive ids - communities under --reorder or the sbm generators - and batch i of an epoch is range number
    epoch_order(ceil(N / batch_size), seed, epoch)[i].  saint_norm = S > 0: S dry batches are drawn first, with batch_seed's epoch at
    SAINT_NORM_EPOCH (a stride no epoch uses; for 'cluster', the first S ranges of that epoch's order), the nodes' appearances counted
    with index_add_, and every node's NLL weighted by tcgnn_layers.saint_node_norm(counts, S) - summed, as PyG's example does, not
    averaged.  The result holds the keys of the mini-batch path - sample_ms covers the walk (or the range), compact_ms extend_nodes,
    induce_subgraph and the feature and label gathers - plus mean_block_edges.  batch_hook gets the epoch's order in place of the seeds."""
    import tcgnn_layers as L
    batch_size = parse_batch_size(batch_size, fanout, hip_graph, sampler=sampler)
    sampler = parse_sampler(sampler, batch_size)
    subgraph = sampler in SUBGRAPH_SAMPLERS
    walk_length = parse_walk_length(walk_length)
    if int(saint_norm) < 0 or (int(saint_norm) and not subgraph):
        raise ValueError("--saint-norm takes a value >= 0 and applies to --sampler saint / cluster only, got %r" % (saint_norm,))
    if fanout is not None and hip_graph:
        raise ValueError("--fanout samples a new graph every epoch and can not be combined with --hip_graph, which replays one captured epoch")
    fanout = parse_fanout(fanout, num_layers)
    directed = bool(directed) or fanout is not None or subgraph
    heads = int(heads)
    multi_head = model_name in ("gat", "gatv2", "transformer")
    if heads != 1 and not multi_head:
        raise ValueError("heads applies to the multi-head attention models - the transformer and the GAT model only")
    if multi_head and (heads < 1 or hidden % heads):
        raise ValueError("--hidden (%d) must be a multiple of --heads (%d)" % (hidden, heads))
    out_cls = None
    if model_name == "gat":
        def conv_cls(a, b):
            return L.GATConv(a, b // heads, heads=heads)
        out_cls = L.GATConv
    elif model_name == "gatv2":
        def conv_cls(a, b):
            return L.GATv2Conv(a, b // heads, heads=heads)
        out_cls = L.GATv2Conv
    elif model_name == "transformer":
        def conv_cls(a, b):
            return L.TransformerConv(a, b // heads, heads=heads)
        out_cls = L.TransformerConv
    elif model_name == "sage":
        def conv_cls(a, b, **kw):
            return L.SAGEConv(a, b, aggregator=aggregator, **kw)
    elif model_name == "gine":
        edge_attr = torch.randn(meta[1].numel(), int(edge_dim), device=x.device, generator=torch.Generator(device=x.device).manual_seed(seed))

        class conv_cls(L.GINEConv):
            def __init__(self, a, b, **kw):
                super().__init__(a, b, edge_dim=int(edge_dim), **kw)

            def forward(self, X, *graph):   # (a sampled graph's rows of edge_attr: sampled_attr, keyed by its column_index)
                return super().forward(X, *graph, edge_attr=sampled_attr.get(graph[1].data_ptr(), edge_attr))
    else:
        if aggregator != "mean":
            raise ValueError("aggregator applies to the SAGE model only")
        conv_cls = {"gcn": L.GCNConv, "gin": L.GINConv, "agnn": L.AGNNConv, "pna": L.PNAConv}[model_name]
    sampled_attr = {}
    torch.manual_seed(seed)
    if model_name != "gcn" and (norm != "none" or bias):
        raise ValueError("norm / bias apply to the GCN model only")
    conv_kwargs = {"norm": norm, "bias": True} if bias else ({"norm": norm} if norm != "none" else {})
    if directed:
        conv_kwargs["directed"] = True
    if attention != "reference":
        if model_name != "agnn":
            raise ValueError("attention applies to the AGNN model only")
        conv_kwargs["attention"] = attention
    if multi_head or model_name in ("pna", "gine"):
        conv_kwargs.pop("directed", None)   # (GATConv, GATv2Conv, TransformerConv, PNAConv and GINEConv back-propagate through A^T on every graph)
    model = Net(conv_cls, in_dim, hidden, classes, num_layers, out_cls=out_cls, **conv_kwargs).to(x.device)
    optimizer = make_adam(model.parameters())

    def train():
        model.train()
        optimizer.zero_grad()
        loss = node_nll_loss(model(x, meta), y)
        loss.backward()
        optimizer.step()
        return loss

    prep = getattr(L.backend(), "prepare", None)
    planless = model_name in ("pna", "gine") or (model_name == "sage" and aggregator != "mean")

    def prepare(meta):
        """what this model's operators need on the graph `meta`, built now: nothing is built (or synchronised) inside a step"""
        if planless and prep is not None and meta[2].numel() == 0:
            L.backend().transpose_graph(meta[0], meta[1])   # (a sampled graph without metadata: the transposed CSR is all the planless operators need)
        elif prep is not None and meta[0].is_cuda and model_name == "sage":
            # a mean layer aggregates at min(in, out), the max layers take no plan-based aggregation at all
            dims = [in_dim] + [hidden] * max(1, num_layers - 1) + [classes]
            prep([min(a, b) for a, b in zip(dims[:-1], dims[1:])] if aggregator == "mean" else [], *meta,
                 **({"max_aggregation": True} if aggregator != "mean" else ({"transpose": True} if directed else {})))
        elif prep is not None and meta[0].is_cuda and model_name in ("pna", "gine"):
            prep([], *meta, max_aggregation=True)   # (forward_stats / backward_stats, forward_ue / edge_sum are planless: the transposed CSR is all they need)
        elif prep is not None and meta[0].is_cuda:   # every width this model aggregates at
            prep(([in_dim] if model_name == "gin" else []) + [hidden // heads] * max(1, num_layers - 1) + [classes], *meta,
                 **({"transpose": True, "edge_valued": True, "attention": True, "heads": heads} if multi_head else
                    {"transpose": True, "edge_valued": True, "attention": True} if attention == "softmax" else
                    ({"transpose": True, "edge_valued": model_name == "agnn"} if directed else {})))

    if fanout is None and not subgraph:
        prepare(meta)
    if tune:   # the tall dense products of this model: library / layout / slab count measured once, here, not inside autograd
        L.tune(L.tune_layers(x.shape[0], [in_dim] + [hidden] * (num_layers - 1) + [classes]), device=x.device)
    if subgraph:
        full, n = meta, x.shape[0]
        spent = {"sample_ms": 0.0, "compact_ms": 0.0, "plan_ms": 0.0, "train_ms": 0.0}
        block_nodes, block_edges, loss = 0, 0, None
        per_epoch = (n + batch_size - 1) // batch_size

        def lap(key, since):
            torch.cuda.synchronize()
            now = time.perf_counter()
            spent[key] += (now - since) * 1e3
            return now

        def draw(epoch, index, order):
            """the node ids of batch `index` of an epoch whose order is `order` (roots for 'saint', range numbers for 'cluster')"""
            if sampler == "saint":
                roots = order[index * batch_size:(index + 1) * batch_size].to(torch.int32)
                return L.backend().random_walk(full[0], full[1], roots, walk_length, batch_seed(seed, epoch, index)).reshape(-1)
            lo = int(order[index]) * batch_size
            return torch.arange(lo, min(lo + batch_size, n), dtype=torch.int32, device=x.device)

        def orders(epoch):
            order = epoch_order(n if sampler == "saint" else per_epoch, seed, epoch)
            return order.to(x.device) if sampler == "saint" else order   # (range numbers are read on the host)

        node_norm = None
        if int(saint_norm):
            counts = torch.zeros(n, dtype=torch.float32, device=x.device)
            order = orders(SAINT_NORM_EPOCH)
            for index in range(int(saint_norm)):
                nodes = L.subgraph_batch(full, draw(SAINT_NORM_EPOCH, index % per_epoch, order), plan=False).nodes
                counts.index_add_(0, nodes.long(), torch.ones(nodes.numel(), dtype=torch.float32, device=x.device))
            node_norm = L.saint_node_norm(counts, int(saint_norm))

        def step(epoch, index, order):
            """one optimiser step on the induced subgraph of batch `index`; -> (loss, M, E_b)"""
            t = time.perf_counter()
            ids = draw(epoch, index, order)
            t = lap("sample_ms", t)
            batch = L.subgraph_batch(full, ids, plan=False, layers=num_layers)
            at = batch.nodes.long()
            xb, yb = x[at], y[at]
            t = lap("compact_ms", t)
            sampled_attr.clear()
            m = batch.metas[0]
            if not planless:
                m = L.csr_meta(m[0], m[1])
                batch.metas = [m] * num_layers   # (one tuple object: a layer's plan is looked up, not rebuilt)
            prepare(m)
            if model_name == "gine":
                sampled_attr[m[1].data_ptr()] = edge_attr[batch.eids[0].long()]
            t = lap("plan_ms", t)
            model.train()
            optimizer.zero_grad()
            out = model(xb, batch.metas)
            if node_norm is None:
                loss = node_nll_loss(out, yb)
            else:
                loss = -(out.gather(1, yb.view(-1, 1)).view(-1) * node_norm[at]).sum()
            loss.backward()
            optimizer.step()
            lap("train_ms", t)
            return loss, batch.nodes.numel(), m[1].numel()

        order = orders(epochs)   # the dry steps: an order no timed epoch uses
        for index in range(min(warmup, per_epoch)):
            loss, _, _ = step(epochs, index, order)
        spent = dict.fromkeys(spent, 0.0)
        for epoch in range(epochs):
            order = orders(epoch)
            for index in range(per_epoch):
                if batch_hook is not None:
                    batch_hook(epoch, index, order)
                loss, m, e = step(epoch, index, order)
                block_nodes += m
                block_edges += e
        model.eval()
        with torch.no_grad():
            final = float(node_nll_loss(model(x, full), y))
        r = {k: v / max(epochs, 1) for k, v in spent.items()}
        r.update(epoch_ms=sum(r.values()), final_loss=final, sampled_loss=float(loss.detach()) if loss is not None else float("nan"), fanout=None,
                 batch_size=batch_size, batches=per_epoch, mean_block_nodes=block_nodes / max(per_epoch * epochs, 1),
                 mean_block_edges=block_edges / max(per_epoch * epochs, 1), sampler=sampler, walk_length=walk_length, saint_norm=int(saint_norm))
        return r
    if batch_size is not None:
        full, n = meta, x.shape[0]
        spent = {"sample_ms": 0.0, "compact_ms": 0.0, "plan_ms": 0.0, "train_ms": 0.0}
        block_nodes, loss = 0, None

        def lap(key, since):
            torch.cuda.synchronize()
            now = time.perf_counter()
            spent[key] += (now - since) * 1e3
            return now

        def step(epoch, index, seeds):
            """one optimiser step on the compact batch of `seeds`; -> (loss, M)"""
            t = time.perf_counter()
            if sampler == "rows":   # tcgnn_layers.sample_batch_rows, timed in its two parts
                drawn = L.sample_layers_rows(full, seeds, fanout, batch_seed(seed, epoch, index))
                t = lap("sample_ms", t)
                batch = L.compact_layers_rows(*drawn, seeds, plan=False)
            else:
                graphs = L.sample_layers(full, seeds, fanout, batch_seed(seed, epoch, index))
                t = lap("sample_ms", t)
                batch = L.compact_layers(graphs, seeds, plan=False)   # (with the line above: tcgnn_layers.sample_batch, timed in its two parts)
            xb, yb = x[batch.nodes.long()], y[seeds]
            t = lap("compact_ms", t)
            sampled_attr.clear()
            for i, (m, eid) in enumerate(zip(batch.metas, batch.eids)):
                if not planless:
                    m = batch.metas[i] = L.csr_meta(m[0], m[1])
                prepare(m)
                if model_name == "gine":
                    sampled_attr[m[1].data_ptr()] = edge_attr[eid.long()]
            t = lap("plan_ms", t)
            model.train()
            optimizer.zero_grad()
            loss = node_nll_loss(model(xb, batch.metas)[batch.seed_pos], yb)
            loss.backward()
            optimizer.step()
            lap("train_ms", t)
            return loss, batch.nodes.numel()

        order = epoch_order(n, seed, epochs).to(x.device)   # the dry steps: a permutation no timed epoch uses
        for index in range(min(warmup, (n + batch_size - 1) // batch_size)):
            loss, _ = step(epochs, index, order[index * batch_size:(index + 1) * batch_size])
        spent = dict.fromkeys(spent, 0.0)
        batches = 0
        for epoch in range(epochs):
            order = epoch_order(n, seed, epoch).to(x.device)
            batches = 0
            for index, lo in enumerate(range(0, n, batch_size)):
                seeds = order[lo:lo + batch_size]
                if batch_hook is not None:
                    batch_hook(epoch, index, seeds)
                loss, m = step(epoch, index, seeds)
                block_nodes += m
                batches += 1
        model.eval()
        with torch.no_grad():
            final = float(node_nll_loss(model(x, full), y))
        r = {k: v / max(epochs, 1) for k, v in spent.items()}
        r.update(epoch_ms=sum(r.values()), final_loss=final, sampled_loss=float(loss.detach()) if loss is not None else float("nan"), fanout=fanout, batch_size=batch_size,
                 batches=batches, mean_block_nodes=block_nodes / max(batches * epochs, 1))
        return r
    if fanout is not None:
        full, spent = meta, {"sample_ms": 0.0, "plan_ms": 0.0, "train_ms": 0.0}

        def lap(key, since):
            torch.cuda.synchronize()
            now = time.perf_counter()
            spent[key] += (now - since) * 1e3
            return now

        for epoch in range(warmup + epochs):
            if epoch == warmup:
                spent = dict.fromkeys(spent, 0.0)
            t = time.perf_counter()
            drawn = {k: L.sample_meta(full, k, seed + epoch, plan=False) for k in set(fanout)}
            t = lap("sample_ms", t)
            sampled_attr.clear()
            for k, (m, eid) in drawn.items():
                if not planless:
                    m = L.csr_meta(m[0], m[1])
                    drawn[k] = (m, eid)
                prepare(m)
                if model_name == "gine":
                    sampled_attr[m[1].data_ptr()] = edge_attr[eid.long()]
            t = lap("plan_ms", t)
            meta = [drawn[k][0] for k in fanout]
            loss = train()
            lap("train_ms", t)
        model.eval()
        with torch.no_grad():
            final = float(node_nll_loss(model(x, full), y))
        r = {k: v / max(epochs, 1) for k, v in spent.items()}
        r.update(epoch_ms=sum(r.values()), final_loss=final, sampled_loss=float(loss.detach()), fanout=fanout)
        return r
    for _ in range(warmup):
        train()
    torch.cuda.synchronize()
    if hip_graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):   # allocator / workspace warm-up on a side stream, as graph capture requires
            for _ in range(3):
                train()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        model.train()
        with torch.cuda.graph(graph):
            static_loss = node_nll_loss(model(x, meta), y)
            static_loss.backward()
            optimizer.step()
        graph.replay()
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(epochs):
            graph.replay()
        torch.cuda.synchronize()
        return {"train_ms": (time.perf_counter() - start) * 1e3 / max(epochs, 1), "final_loss": float(static_loss.detach()), "hip_graph": True}
    start = time.perf_counter()
    for _ in range(epochs):
        loss = train()
    torch.cuda.synchronize()
    return {"train_ms": (time.perf_counter() - start) * 1e3 / max(epochs, 1), "final_loss": float(loss.detach())}


def run(args, quiet=False):
    import TCGNN
    import tcgnn_layers as L
    say = (lambda *a, **k: None) if quiet else print
    if args.synthetic and args.dataset == build_parser().get_default("dataset"):
        args.dataset = args.synthetic   # the scrapers take the graph's name from `dataset=` in this line (1_log2csv.py:13-16)
    say(args)
    if not torch.cuda.is_available():
        raise RuntimeError("tcgnn_harness needs the GPU: the TCGNN operators have no CPU path")
    device = torch.device("cuda:0")
    ds = load_graph(args)
    num_nodes, num_edges = ds.num_nodes, ds.num_edges
    column_index, row_pointers = ds.column_index, ds.row_pointers
    x_host, y_host = ds.x, ds.y
    if getattr(args, "reorder", False):
        import tcgnn_graph as G
        start = time.perf_counter()
        order = G.community_order(row_pointers.to(device), column_index.to(device), seed=args.seed)
        row_pointers, column_index = (t.cpu() for t in G.permute_csr(row_pointers.to(device), column_index.to(device), order))
        x_host, y_host = x_host[order.cpu()], y_host[order.cpu()]
        torch.cuda.synchronize()
        say("Reorder:\t{:.3f} ms".format((time.perf_counter() - start) * 1e3))   # (not "(ms):" - 1_log2csv.py:17 would scrape it as a result)

    # metadata allocated exactly as main_tcgnn.py:44-47 does (edge arrays sized by the RAW edge count)
    num_row_windows = (num_nodes + BLK_H - 1) // BLK_H
    edgeToColumn = torch.zeros(num_edges, dtype=torch.int)
    edgeToRow = torch.zeros(num_edges, dtype=torch.int)
    blockPartition = torch.zeros(num_row_windows, dtype=torch.int)

    start = time.perf_counter()
    if args.gpu_preprocess:
        column_index, row_pointers = column_index.to(device), row_pointers.to(device)
        blockPartition, edgeToColumn, edgeToRow = blockPartition.to(device), edgeToColumn.to(device), edgeToRow.to(device)
        TCGNN.preprocess_gpu(column_index, row_pointers, num_nodes, BLK_H, BLK_W, blockPartition, edgeToColumn, edgeToRow)
        torch.cuda.synchronize()
    else:
        TCGNN.preprocess(column_index, row_pointers, num_nodes, BLK_H, BLK_W, blockPartition, edgeToColumn, edgeToRow)
    prep_ms = (time.perf_counter() - start) * 1e3
    say("Prep. (ms):\t{:.3f}".format(prep_ms))

    meta = tuple(t.to(device) for t in (row_pointers, column_index, blockPartition, edgeToColumn, edgeToRow))
    x, y = x_host.to(device), y_host.to(device)
    result = {"prep_ms": prep_ms, "num_nodes": num_nodes, "nnz": int(column_index.numel()), "num_edges_raw": int(num_edges),
              "edge_arrays_len": int(edgeToColumn.numel()), "num_row_windows": int(blockPartition.numel())}

    if args.single_kernel:
        result["sag_ms"] = L.SAG(*meta).profile(x)
        return result

    if args.model == "gine":
        say("edge_attr:\t[%d, %d] standard normal, drawn once on the device from seed %d (the dataset carries no edge features)"
            % (meta[1].numel(), getattr(args, "edge_dim", 16), args.seed))
    r = time_training(args.model, meta, x, y, ds.num_features, args.hidden, ds.num_classes, args.num_layers, args.epochs,
                      seed=args.seed, warmup=9, hip_graph=getattr(args, "hip_graph", False),  # 9 dry epochs, main_tcgnn.py:166-167
                      norm=getattr(args, "norm", "none"), bias=getattr(args, "bias", False), directed=getattr(args, "directed", False),
                      attention=getattr(args, "attention", "reference"), heads=getattr(args, "heads", 1),
                      aggregator=getattr(args, "aggregator", "mean"), edge_dim=getattr(args, "edge_dim", 16), fanout=getattr(args, "fanout", None),
                      batch_size=getattr(args, "batch_size", None), batch_hook=getattr(args, "batch_hook", None),
                      sampler=getattr(args, "sampler", "dense"), walk_length=getattr(args, "walk_length", 2), saint_norm=getattr(args, "saint_norm", 0))
    if "sample_ms" in r:
        say("Sample (ms):\t{:6.3f}\nPlan (ms):\t{:6.3f}".format(r["sample_ms"], r["plan_ms"]))
    if "compact_ms" in r:
        say("Compact (ms):\t{:6.3f}\nBatches:\t{:d}\tmean block nodes {:.1f}".format(r["compact_ms"], r["batches"], r["mean_block_nodes"]))
    say("Train (ms):\t{:6.3f}".format(r["train_ms"]))
    result.update(r)
    return result


if __name__ == "__main__":
    run(build_parser().parse_args())
