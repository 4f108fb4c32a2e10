"""SR-GNN (Wu et al., AAAI 2019) restated the way the paper writes it: per session a dense adjacency matrix built in numpy
from the raw sequence, its column- and row-normalised forms stacked as ``A [B, n, 2n]``, ``torch.matmul`` and autograd.
It shares no code with the product's edge lists.  ``dtype=torch.float64`` is "exact", ``torch.float32`` gives the
reference's own rounding error.

``DEFECTS`` names wrong variants of it; tests/test_srgnn_host.py shows that the fixtures of srgnn_edges.py see every one.
``edge_lists`` is a second, independent restatement of the session graph as ragged lists (what csrc/srgnn.hip builds),
held against the dense matrices there."""
import numpy as np
import torch
import torch.nn.functional as F

DEFECTS = (
    "edge_multiplicity",            # a transition that occurs twice weighs twice
    "self_loops_dropped",           # s_t == s_{t+1} makes no edge
    "in_by_outdeg",                 # the in-mean divided by the node's out-degree
    "in_out_swapped",               # a_in from the out-neighbours and the reverse
    "b_iah_skipped_isolated",       # b_iah only where indeg > 0
    "b_oah_skipped_isolated",       # b_oah only where outdeg > 0
    "b_in_on_empty_mean",           # linear_edge_in.bias added to an empty mean
    "r_z_swapped",                  # the chunks taken as z, r, n
    "h_update_reversed",            # h' = z n + (1 - z) h
    "r_on_gi_n",                    # n = tanh(r gi_n + gh_n)
    "step_once",                    # the cell run once whatever `step`
    "h_T_at_T_minus_1",             # h_T read at the padded end instead of len - 1
    "padded_in_s_g",                # positions >= len left in the sum
    "softmax_over_positions",       # alpha normalised over the positions
    "nonhybrid_ignored",            # linear_transform applied although nonhybrid is set
    "item_0_in_softmax",            # the padding row scored as well
    "target_not_shifted",           # cross-entropy against target instead of target - 1
    "loss_summed",                  # sum over the batch instead of the mean
    "alias_first_appearance",       # nodes in order of first appearance (the numbers do not move: a builder defect)
)
GRAPH_DEFECTS = ("alias_first_appearance",)


def shapes(n_node, H):
    """``state_dict()`` names and shapes, in order."""
    return {"embedding.weight": (n_node, H), "gnn.w_ih": (3 * H, 2 * H), "gnn.w_hh": (3 * H, H), "gnn.b_ih": (3 * H,),
            "gnn.b_hh": (3 * H,), "gnn.b_iah": (H,), "gnn.b_oah": (H,), "gnn.linear_edge_in.weight": (H, H),
            "gnn.linear_edge_in.bias": (H,), "gnn.linear_edge_out.weight": (H, H), "gnn.linear_edge_out.bias": (H,),
            "linear_one.weight": (H, H), "linear_one.bias": (H,), "linear_two.weight": (H, H), "linear_two.bias": (H,),
            "linear_three.weight": (1, H), "linear_transform.weight": (H, 2 * H), "linear_transform.bias": (H,)}


def n_params(n_node, H):
    return sum(int(np.prod(s)) for s in shapes(n_node, H).values())


def session_graph(items, defect=None):
    """``(nodes, alias, A)`` of one session: ``A[u, v]`` is 1 where the transition u -> v occurs."""
    items = [int(i) for i in items]
    nodes = list(dict.fromkeys(items)) if defect == "alias_first_appearance" else sorted(set(items))
    alias = [nodes.index(i) for i in items]
    A = np.zeros((len(nodes), len(nodes)))
    for t in range(len(items) - 1):
        u, v = alias[t], alias[t + 1]
        if defect == "self_loops_dropped" and u == v:
            continue
        A[u, v] = A[u, v] + 1 if defect == "edge_multiplicity" else 1
    return nodes, alias, A


def dense_batch(seq, lens, defect=None):
    """The batch as the published code feeds it: ``items [B, n]`` (0-padded node ids), ``alias [B, T]`` (0 behind a
    length), ``A_in, A_out [B, n, n]`` (row v of A_in: the weights of v's in-neighbours), ``indeg, outdeg [B, n]``,
    ``mask [B, T]``."""
    seq, lens = np.asarray(seq), np.asarray(lens).reshape(-1)
    T, B = seq.shape
    graphs = [session_graph(seq[:lens[b], b], defect) for b in range(B)]
    n = max(len(g[0]) for g in graphs)
    items = np.zeros((B, n), dtype=np.int64)
    alias = np.zeros((B, T), dtype=np.int64)
    A_in, A_out = np.zeros((B, n, n)), np.zeros((B, n, n))
    indeg, outdeg = np.zeros((B, n)), np.zeros((B, n))
    for b, (nodes, al, A) in enumerate(graphs):
        k = len(nodes)
        items[b, :k] = nodes
        alias[b, :len(al)] = al
        s_in, s_out = A.sum(0), A.sum(1)
        indeg[b, :k], outdeg[b, :k] = s_in, s_out
        by = s_out if defect == "in_by_outdeg" else s_in
        A_in[b, :k, :k] = (A / np.where(by == 0, 1, by)[None, :]).T
        A_out[b, :k, :k] = A / np.where(s_out == 0, 1, s_out)[:, None]
    if defect == "in_out_swapped":
        A_in, A_out, indeg, outdeg = A_out, A_in, outdeg, indeg
    mask = np.arange(T)[None, :] < lens[:, None]
    return items, alias, A_in, A_out, indeg, outdeg, mask


def edge_lists(items):
    """The session graph of one session as ragged lists: ``(nodes, alias, in_lists, out_lists)`` with the neighbours of
    every node ascending."""
    items = [int(i) for i in items]
    nodes = sorted(set(items))
    alias = [nodes.index(i) for i in items]
    edges = sorted(set(zip(alias[:-1], alias[1:])))
    in_lists = [[u for u, v in edges if v == k] for k in range(len(nodes))]
    out_lists = [[v for u, v in edges if u == k] for k in range(len(nodes))]
    return nodes, alias, in_lists, out_lists


def forward(w, cfg, batch, dtype=torch.float64, defect=None):
    """``(loss, scores [B, n_node - 1], query [B, H])`` as tensors of ``dtype``; ``w`` may hold tensors that require a
    gradient.  ``cfg``: ``H step nonhybrid``; ``batch``: ``(seq [T, B], target [B], lens)``."""
    seq, target, lens = batch
    lens = np.asarray(lens).reshape(-1)
    items, alias, A_in, A_out, indeg, outdeg, mask = dense_batch(seq, lens, defect)
    t = lambda a: torch.as_tensor(a, dtype=dtype)      # noqa: E731
    A_in, A_out, mask_t = t(A_in), t(A_out), t(mask)
    has_in, has_out = t(indeg > 0)[:, :, None], t(outdeg > 0)[:, :, None]
    B, T = alias.shape
    h = w["embedding.weight"][torch.as_tensor(items)]
    for _ in range(1 if defect == "step_once" else cfg["step"]):
        p_in = h @ w["gnn.linear_edge_in.weight"].T + w["gnn.linear_edge_in.bias"]
        p_out = h @ w["gnn.linear_edge_out.weight"].T + w["gnn.linear_edge_out.bias"]
        a_in = torch.matmul(A_in, p_in) + (w["gnn.b_iah"] * has_in if defect == "b_iah_skipped_isolated" else w["gnn.b_iah"])
        a_out = torch.matmul(A_out, p_out) + (w["gnn.b_oah"] * has_out if defect == "b_oah_skipped_isolated"
                                              else w["gnn.b_oah"])
        if defect == "b_in_on_empty_mean":
            a_in = a_in + w["gnn.linear_edge_in.bias"] * (1 - has_in)
        gi = torch.cat([a_in, a_out], 2) @ w["gnn.w_ih"].T + w["gnn.b_ih"]
        gh = h @ w["gnn.w_hh"].T + w["gnn.b_hh"]
        i_r, i_z, i_n = gi.chunk(3, 2)
        h_r, h_z, h_n = gh.chunk(3, 2)
        if defect == "r_z_swapped":
            i_r, i_z, h_r, h_z = i_z, i_r, h_z, h_r
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(r * i_n + h_n) if defect == "r_on_gi_n" else torch.tanh(i_n + r * h_n)
        h = z * n + (1 - z) * h if defect == "h_update_reversed" else n + z * (h - n)
    rows = torch.arange(B)[:, None]
    x = h[rows, torch.as_tensor(alias)]                                         # [B, T, H]
    last = np.full(B, T - 1) if defect == "h_T_at_T_minus_1" else lens - 1
    ht = x[torch.arange(B), torch.as_tensor(last)]
    q1 = ht @ w["linear_one.weight"].T + w["linear_one.bias"]
    q2 = x @ w["linear_two.weight"].T + w["linear_two.bias"]
    alpha = torch.sigmoid(q1[:, None, :] + q2) @ w["linear_three.weight"].T   # [B, T, 1]
    if defect == "softmax_over_positions":
        alpha = torch.softmax(alpha.masked_fill(mask_t[:, :, None] == 0, float("-inf")), 1)
    keep = torch.ones_like(mask_t) if defect == "padded_in_s_g" else mask_t
    s_g = (alpha * x * keep[:, :, None]).sum(1)
    if cfg["nonhybrid"] and defect != "nonhybrid_ignored":
        a = s_g
    else:
        a = torch.cat([s_g, ht], 1) @ w["linear_transform.weight"].T + w["linear_transform.bias"]
    scores = a @ w["embedding.weight"][1:].T
    tgt = torch.as_tensor(np.asarray(target).reshape(-1), dtype=torch.int64)
    if defect == "item_0_in_softmax":
        logits, index = a @ w["embedding.weight"].T, tgt
    elif defect == "target_not_shifted":
        logits, index = scores, tgt
    else:
        logits, index = scores, tgt - 1
    loss = F.cross_entropy(logits, index, reduction="sum" if defect == "loss_summed" else "mean")
    return loss, scores, a


def grads(w, cfg, batch, dtype=torch.float64, defect=None):
    """``(loss, {name: gradient}, query [B, H], scores [B, n_node - 1])`` as python / numpy values; a parameter the loss
    does not reach (``linear_transform`` under ``nonhybrid``) has a zero gradient."""
    wt = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in w.items()}
    loss, scores, a = forward(wt, cfg, batch, dtype, defect)
    g = torch.autograd.grad(loss, list(wt.values()), allow_unused=True)
    out = {k: (np.zeros(v.shape) if gk is None else gk.detach().numpy().astype(np.float64)) for (k, v), gk in zip(wt.items(), g)}
    return float(loss.detach()), out, a.detach().numpy().astype(np.float64), scores.detach().numpy().astype(np.float64)


def adam_step(w, g, state, lr, l2, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam with ``weight_decay=l2`` on float32 numpy weights, in place (``g`` excludes the decay)."""
    state["t"] += 1
    t = state["t"]
    for k in w:
        gk = (np.asarray(g[k], dtype=np.float32) + np.float32(l2) * w[k]).astype(np.float32)
        state["m"][k] = (np.float32(beta1) * state["m"][k] + np.float32(1 - beta1) * gk).astype(np.float32)
        state["v"][k] = (np.float32(beta2) * state["v"][k] + np.float32(1 - beta2) * gk * gk).astype(np.float32)
        step = np.float32(lr / (1 - beta1 ** t))
        denom = (np.sqrt(state["v"][k]) / np.float32(np.sqrt(1 - beta2 ** t)) + np.float32(eps)).astype(np.float32)
        w[k] -= (step * state["m"][k] / denom).astype(np.float32)


def new_adam_state(w):
    return {"t": 0, "m": {k: np.zeros_like(v) for k, v in w.items()}, "v": {k: np.zeros_like(v) for k, v in w.items()}}
