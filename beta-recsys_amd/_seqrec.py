"""What the sequence models (``sasrec.py``, ``tisasrec.py``) share on the Python side: the limits of the HIP kernels
(``csrc/seqrec.hpp``), the common config parsing, the workspace and id plumbing of the model, and the dropout-mask /
step plumbing of the engine.  Each model keeps its own parameter layout, constructor, feature call and C entry point."""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_DIM, MAX_LEN, HEAD_WIDTHS = 128, 256, (16, 32, 64)


class _FeedForwardParams(nn.Module):
    """``PointWiseFeedForward``'s two ``Conv1d(kernel_size=1)``."""

    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        self.conv1 = _ParamView(w1, b1)
        self.conv2 = _ParamView(w2, b2)


class _SeqModel(_FlatModel):
    """Subclasses name their ``hiprec_*_workspace_bytes`` / ``hiprec_*_param_floats`` entry points and own ``shape``."""

    _WORKSPACE_BYTES = _PARAM_FLOATS = None

    def _configure(self, config, needs, also_bad=False):
        """The config keys both models read, validated; ``needs`` is the model's text for a count below 1."""
        self.config = config
        self.user_num = config["n_users"]
        self.item_num = int(config["n_items"])
        self.hidden_units = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.num_blocks = int(config["num_blocks"])
        self.num_heads = int(config["num_heads"])
        self.dropout_rate = float(config["dropout_rate"])
        self.batch_size = config["batch_size"]
        self.l2_emb = float(config["l2_emb"])
        D, H, T = self.hidden_units, self.num_heads, self.maxlen
        if self.num_blocks < 1 or H < 1 or self.item_num < 1 or T < 1 or also_bad:
            raise ValueError(needs)
        if D % H != 0 or D // H not in HEAD_WIDTHS:
            raise ValueError(f"the HIP attention supports head widths emb_dim / num_heads in {HEAD_WIDTHS}; "
                             f"got emb_dim {D}, num_heads {H}")
        if D > MAX_DIM:
            raise ValueError(f"emb_dim must be <= {MAX_DIM}, got {D}")
        if T > MAX_LEN:
            raise ValueError(f"maxlen must be <= {MAX_LEN}, got {T}")
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len):
        need = getattr(lib, self._WORKSPACE_BYTES)(ctypes.byref(self.shape), int(batch), int(seq_len))
        if need == 0:
            raise ValueError(f"unsupported batch {batch} x sequence length {seq_len}")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def sequences(self, seqs):
        """``[B, T]`` ids (numpy, list or tensor) as ``(flat int64 device tensor, B, T)``; T must be <= maxlen."""
        shape = tuple(seqs.shape) if torch.is_tensor(seqs) else np.asarray(seqs).shape
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("sequences must be [batch >= 1, length >= 1]")
        if shape[1] > self.maxlen:
            raise ValueError(f"sequence length {shape[1]} exceeds maxlen {self.maxlen}")
        return index_tensor(seqs, self._flat.device), int(shape[0]), int(shape[1])

    def _item_ids(self, ids):
        idx = index_tensor(ids, self._flat.device)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.item_num):
            raise IndexError(f"item id outside [0, {self.item_num}]")
        return idx

    def _logits(self, feats, pos_seqs, neg_seqs):
        """``(pos_logits, neg_logits)``, each ``[B, T]``: the features against the rows of the two id arrays."""
        return tuple((feats * self.item_emb.weight.data[self._item_ids(ids)].view(feats.shape)).sum(-1)
                     for ids in (pos_seqs, neg_seqs))

    def _predict_from_feats(self, feats, item_indices):
        """``[n_seqs, n_indices]`` logits of the last position's feature against the rows of ``item_indices`` (1-D),
        through the exact-fp32 MFMA GEMM."""
        lib, dev = _lib.load(), self._flat.device
        if np.ndim(item_indices) != 1:
            raise ValueError("item_indices must be 1-D: one list of candidate items for every sequence")
        idx = self._item_ids(item_indices)
        rows = self.item_emb.weight.data[idx].contiguous()
        B, T, D = feats.shape
        logits = torch.empty((B, idx.numel()), dtype=torch.float32, device=dev)
        if idx.numel():
            last = feats[:, T - 1, :]
            _lib.check(lib.hiprec_gemm_f32(0, B, idx.numel(), D, ctypes.c_void_p(last.data_ptr()), T * D, _lib.ptr(rows),
                                           D, _lib.ptr(logits), idx.numel(), None, 0, None, 0, _lib.stream_ptr(dev)))
        return logits


class _SeqEngine(FlatModelEngine):
    """Subclasses supply ``_mask_shapes(B, T)`` (the reference's shapes in its call order: ``_N_FIXED_MASKS`` masks
    drawn once per step, then per block attention, dropout1, dropout2), ``_MASK_NAMES`` for the error text, and
    ``_enqueue_grad(batch_data, keep_masks)``."""

    _N_FIXED_MASKS = _MASK_NAMES = None

    def _alloc_extra(self, lib, dev):
        m = self.model
        if getattr(lib, m._PARAM_FLOATS)(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError(f"the flat {type(m).__name__} buffer is not laid out as libhiprec.so expects; "
                               "rebuild the library")

    def _keep_masks(self, B, T, keep_masks):
        """The keep masks of one step as uint8 device tensors, or None (no dropout)."""
        m = self.model
        p = m.dropout_rate
        if p == 0.0 or not m.training:
            return None
        dev = m.flat.device
        shapes = self._mask_shapes(B, T)
        if keep_masks is not None:
            if len(keep_masks) != len(shapes):
                raise ValueError(f"{len(shapes)} keep masks expected ({self._MASK_NAMES}; per block attention, dropout1, "
                                 f"dropout2), got {len(keep_masks)}")
            out = []
            for k, s in zip(keep_masks, shapes):
                t = torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k)).to(torch.uint8)
                if t.numel() != int(np.prod(s)):
                    raise ValueError(f"keep mask of {t.numel()} elements where {s} is expected")
                out.append(t.reshape(-1).contiguous().to(dev))
            return out
        cfg = self.config["model"]
        rng = cfg["dropout_rng"] if "dropout_rng" in cfg else "torch_cpu"
        self._dropout_step += 1
        D = m.hidden_units
        out = []
        if rng == "torch_cpu":
            # nn.Dropout / F.dropout on the CPU draw torch.empty_like(input).bernoulli_(1 - p) on the reference's shape
            # of each input; the two FFN dropouts of a block see Conv1d's [B, D, T] layout
            for i, s in enumerate(shapes):
                if i >= self._N_FIXED_MASKS and (i - self._N_FIXED_MASKS) % 3 != 0:
                    k = torch.empty(B, D, T).bernoulli_(1 - p).transpose(1, 2)
                else:
                    k = torch.empty(s).bernoulli_(1 - p)
                out.append(k.to(torch.uint8).reshape(-1).contiguous().to(dev))
        elif rng == "device":
            seed = int(cfg["dropout_seed"]) if "dropout_seed" in cfg else 0
            lib = _lib.load()
            for i, s in enumerate(shapes):
                buf = torch.empty(int(np.prod(s)), dtype=torch.uint8, device=dev)
                _lib.check(lib.hiprec_edge_dropout_mask(_lib.ptr(buf), buf.numel(), 1.0 - p, seed * 64 + i,
                                                        self._dropout_step, _lib.stream_ptr(dev)))
                out.append(buf)
        else:
            raise ValueError(f"unknown dropout_rng {rng!r}: 'torch_cpu' or 'device'")
        return out

    def _keep_array(self, B, T, keep_masks):
        """``_keep_masks`` as the host array of device pointers the C entry points take (None: no dropout)."""
        keep = self.last_keep_masks = self._keep_masks(B, T, keep_masks)
        return None if keep is None else (ctypes.c_void_p * len(keep))(*[k.data_ptr() for k in keep])

    # ---- the step ----------------------------------------------------------------------------------------------
    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """The reference's ``train_single_batch``: one step on the model's batch tuple, returns ``loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _recommend_from_feats(self, feats, k, seen):
        """The ``k`` best next items by the last position's feature against ``item_emb.weight[1:]``."""
        from .recommend import topk_factors

        n, T, _ = feats.shape
        table = self.model.item_emb.weight.data[1:]
        if seen is not None:
            rows, items = (index_tensor(x, feats.device) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(feats[:, T - 1, :], table, 1.0, None, torch.arange(n, device=feats.device), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
