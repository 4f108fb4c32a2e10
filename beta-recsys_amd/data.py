"""Device-side training-set construction: the data step in front of the hot path.

Mirrors the three loader builders of ``beta_rec/data/base_data.py`` that feed the engines of this
package — same inputs (the split's ``train`` frame, ``n_users``, ``n_items``), same row order and
tensor layout of the resulting dataset, batches of the same tuple shape:

* ``instance_bpr_loader``      (base_data.py:218-253)  (user, pos, neg) triples, one negative per row
* ``instance_bce_loader``      (base_data.py:182-216)  (user, item, rating): each row followed by its
                                                        ``num_negative`` negatives with rating 0
* ``instance_mul_neg_loader``  (base_data.py:254-288)  (user, pos, neg[num_negative])

The reference samples with ``random.sample`` inside a pandas ``iterrows`` loop on the host and then
lets a ``DataLoader`` index the tensors element by element; here the negatives come from
``hiprec_sample_negatives`` (csrc/sampler.hip: k distinct items, uniform over the items the user
never touched — the same distribution, a different random stream) and the batches from device-side
batchers.  No CPU fallback: the sampler runs in libhiprec.so or not at all.
"""
import numpy as np
import torch

from . import _lib
from ._stats import _new_stats, raise_on_status, read_stats
from .eval import DEFAULT_ITEM_COL, DEFAULT_RATING_COL, DEFAULT_USER_COL, _column, _resolve_device
from .mf import DeviceTripleBatcher


def _draw_seed():
    """A 62-bit seed from torch's global CPU generator, so ``torch.manual_seed`` controls the draw."""
    return int(torch.randint(0, 2**62, (1,)).item())


def build_positive_csr(users, items, n_users, n_items):
    """(user_ptr[n_users+1], pos_sorted): each user's positive items, ascending and unique
    (``groupby(user)[item].apply(set)``, base_data.py:227-231) — torch ops on the tensors' device."""
    users = users.to(torch.int64)
    items = items.to(torch.int64)
    if users.numel() and (int(users.min()) < 0 or int(users.max()) >= n_users
                          or int(items.min()) < 0 or int(items.max()) >= n_items):
        raise IndexError("training frame holds a user / item id outside [0, n_users) x [0, n_items)")
    key = torch.unique(users * n_items + items)          # sorted
    owner = torch.div(key, n_items, rounding_mode="floor")
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(torch.bincount(owner, minlength=n_users), 0, out=ptr[1:])
    return ptr, (key - owner * n_items).contiguous()


def sample_negatives(users, items, n_users, n_items, k=1, seed=None, device=None):
    """int64 tensor [n_rows, k]: for every (user, item) row, k distinct items the user never interacted
    with anywhere in the frame, uniformly at random (a pure function of ``seed``)."""
    if k < 1:
        raise ValueError(f"k must be >= 1, got {k}")
    if torch.is_tensor(users) and users.device.type == "cuda" and device is None:
        device = users.device
    dev = _resolve_device(device)
    lib = _lib.load()
    users_t = torch.as_tensor(np.asarray(users) if not torch.is_tensor(users) else users).to(dev, torch.int64).reshape(-1).contiguous()
    items_t = torch.as_tensor(np.asarray(items) if not torch.is_tensor(items) else items).to(dev, torch.int64).reshape(-1).contiguous()
    if users_t.numel() != items_t.numel():
        raise ValueError("users and items differ in length")
    ptr, cols = build_positive_csr(users_t, items_t, int(n_users), int(n_items))
    out = torch.empty((users_t.numel(), int(k)), dtype=torch.int64, device=dev)
    stats = _new_stats(dev)
    seed = _draw_seed() if seed is None else int(seed)
    with torch.cuda.device(dev):
        _lib.check(lib.hiprec_sample_negatives(
            _lib.ptr(ptr), _lib.ptr(cols), int(n_users), int(n_items), _lib.ptr(users_t), users_t.numel(),
            int(k), seed, _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr(dev)))
    raise_on_status(read_stats(stats).status)
    return out


class DeviceTensorBatcher:
    """``DataLoader(TensorDataset-like, batch_size, shuffle=True)`` over device-resident tensors:
    iterating yields tuples of batch slices, a fresh device-side permutation per epoch."""

    def __init__(self, tensors, batch_size, shuffle=True):
        self.tensors = tuple(tensors)
        if len({t.shape[0] for t in self.tensors}) != 1:
            raise ValueError("tensors differ in length")
        self.batch_size = int(batch_size)
        self.shuffle = shuffle

    def __len__(self):
        n = self.tensors[0].shape[0]
        return (n + self.batch_size - 1) // self.batch_size

    def permutation(self):
        """One epoch's visiting order (int64, on the tensors' device); None = sequential."""
        n = self.tensors[0].shape[0]
        if not (self.shuffle and n):
            return None
        dev = self.tensors[0].device
        perm = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(_lib.load().hiprec_random_permutation(_lib.ptr(perm), n, _draw_seed(), _lib.stream_ptr(dev)))
        return perm

    def __iter__(self):
        n = self.tensors[0].shape[0]
        perm = self.permutation()
        for off in range(0, n, self.batch_size):
            if perm is None:
                yield tuple(t[off:off + self.batch_size] for t in self.tensors)
            else:
                idx = perm[off:off + self.batch_size]
                yield tuple(t[idx] for t in self.tensors)


def _train_columns(data, device):
    dev = _resolve_device(device)
    train = data.train
    users = torch.as_tensor(np.asarray(_column(train, DEFAULT_USER_COL))).to(dev, torch.int64)
    items = torch.as_tensor(np.asarray(_column(train, DEFAULT_ITEM_COL))).to(dev, torch.int64)
    return dev, users, items


def instance_bpr_loader(data, batch_size, device, seed=None):
    """base_data.py:218-253: one negative per training row; batches of (user, pos_item, neg_item).
    Returns a :class:`DeviceTripleBatcher` (``user_tensor / pos_item_tensor / neg_item_tensor`` like
    the reference's ``PairwiseNegativeDataset``), which ``MFEngine.train_an_epoch`` runs resident."""
    dev, users, items = _train_columns(data, device)
    neg = sample_negatives(users, items, data.n_users, data.n_items, 1, seed, dev)[:, 0].contiguous()
    print(f"Making PairwiseNegativeDataset of length {users.numel()}")
    return DeviceTripleBatcher(users, items, neg, batch_size, shuffle=True)


def instance_bce_loader(data, batch_size, device, num_negative, seed=None):
    """base_data.py:182-216: every training row (rating kept) followed by ``num_negative`` sampled
    negatives of its user with rating 0; batches of (user, item, rating)."""
    dev, users, items = _train_columns(data, device)
    ratings = torch.as_tensor(np.asarray(_column(data.train, DEFAULT_RATING_COL))).to(dev, torch.float32)
    k = int(num_negative)
    neg = sample_negatives(users, items, data.n_users, data.n_items, k, seed, dev)
    all_users = users.repeat_interleave(k + 1)
    all_items = torch.cat([items[:, None], neg], dim=1).reshape(-1)
    all_ratings = torch.cat([ratings[:, None], torch.zeros_like(neg, dtype=torch.float32)], dim=1).reshape(-1)
    print(f"Making RatingDataset of length {all_users.numel()}")
    return DeviceTensorBatcher((all_users, all_items, all_ratings), batch_size, shuffle=True)


def instance_mul_neg_loader(data, batch_size, device, num_negative, seed=None):
    """base_data.py:254-288: batches of (user, pos_item, neg_items[num_negative])."""
    dev, users, items = _train_columns(data, device)
    neg = sample_negatives(users, items, data.n_users, data.n_items, int(num_negative), seed, dev)
    print(f"Making PairwiseNegativeDataset of length {users.numel()}")
    return DeviceTensorBatcher((users, items, neg), batch_size, shuffle=True)


class SequenceSampler:
    """Host-side batches for SASRec, by the rule of the reference's ``sample_function``
    (beta_rec/recommenders/sasrec.py:31-77), vectorised in numpy: a uniformly random user with at least two items;
    ``seq`` the last ``maxlen`` items before the final one, ``pos`` the item that follows each of them, ``neg`` one item
    per real position drawn uniformly from 1 .. n_items outside the user's set; all three left-padded with 0.

    ``user_train``: dict user id -> list of item ids (1-based, in time order).  ``next_batch()`` returns
    ``(users [B], seq [B, maxlen], pos [B, maxlen], neg [B, maxlen])`` int64 arrays -- what ``SASRecEngine.
    train_an_epoch`` asks for.  Same distribution as the reference's sampler, not its RNG stream; the same ``seed`` gives
    the same batches.  ``n_users`` is kept for the reference's signature."""

    def __init__(self, user_train, n_users, n_items, batch_size, maxlen, seed=0):
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.batch_size, self.maxlen = int(batch_size), int(maxlen)
        self.users = np.array(sorted(u for u, items in user_train.items() if len(items) >= 2), dtype=np.int64)
        if self.users.size == 0:
            raise ValueError("no user has two or more items")
        self.items = {int(u): np.asarray(user_train[u], dtype=np.int64) for u in self.users}
        for u, items in self.items.items():
            if items.min() < 1 or items.max() > self.n_items:
                raise IndexError(f"user {u} holds an item outside [1, {self.n_items}]")
            if np.unique(items).size >= self.n_items:
                raise ValueError(f"user {u} has interacted with every item: no negative exists")
        self.rng = np.random.default_rng(seed)

    def _negatives(self, n, taken):
        """``n`` ids uniform over 1 .. n_items outside the sorted array ``taken`` (rejection, all at once)."""
        out = self.rng.integers(1, self.n_items + 1, n)
        while True:
            at = np.searchsorted(taken, out)
            bad = (at < taken.size) & (taken[np.minimum(at, taken.size - 1)] == out)
            if not bad.any():
                return out
            out[bad] = self.rng.integers(1, self.n_items + 1, int(bad.sum()))

    def next_batch(self):
        B, T = self.batch_size, self.maxlen
        users = self.users[self.rng.integers(0, self.users.size, B)]
        seq, pos, neg = (np.zeros((B, T), dtype=np.int64) for _ in range(3))
        for b, u in enumerate(users):
            items = self.items[int(u)]
            n = min(T, items.size - 1)
            seq[b, T - n:] = items[-n - 1:-1]
            pos[b, T - n:] = items[-n:]
            neg[b, T - n:] = self._negatives(n, np.unique(items))
        return users, seq, pos, neg

    def close(self):
        """The reference's sampler owns worker processes; this one owns nothing."""


class ClozeSampler:
    """Host-side batches for BERT4Rec's cloze task: a uniformly random user with at least one item; the last ``maxlen``
    items, left-padded with 0; every real position replaced by ``[MASK]`` (``n_items + 1``) independently with
    probability ``mask_prob``; a sequence in which none was drawn gets its LAST position masked, so every sequence
    trains and the last-item case the model is queried with is seen.  ``labels`` hold the original item at the masked
    positions and 0 elsewhere.

    ``user_train``: dict user id -> list of item ids (1-based, in time order).  ``next_batch()`` returns
    ``(users [B], seq [B, maxlen], labels [B, maxlen])`` int64 arrays -- what ``BERT4RecEngine.train_an_epoch`` asks
    for.  The same ``seed`` gives the same batches.  ``last_forced [B]`` tells which sequences of the last batch had
    their mask forced.  ``n_users`` is kept for the signature of the other samplers."""

    def __init__(self, user_train, n_users, n_items, batch_size, maxlen, mask_prob=0.2, seed=0):
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.batch_size, self.maxlen = int(batch_size), int(maxlen)
        self.mask_prob = float(mask_prob)
        self.mask_id = self.n_items + 1
        if not 0.0 < self.mask_prob < 1.0:
            raise ValueError("mask_prob must be in (0, 1)")
        if self.batch_size < 1 or self.maxlen < 1:
            raise ValueError("batch_size and maxlen must be >= 1")
        self.users = np.array(sorted(u for u, items in user_train.items() if len(items) >= 1), dtype=np.int64)
        if self.users.size == 0:
            raise ValueError("no user has an item")
        # every user's last maxlen items as one left-padded table: a batch is a row gather
        self.table = np.zeros((self.users.size, self.maxlen), dtype=np.int64)
        for r, u in enumerate(self.users):
            items = np.asarray(user_train[u], dtype=np.int64)
            if items.min() < 1 or items.max() > self.n_items:
                raise IndexError(f"user {u} holds an item outside [1, {self.n_items}]")
            n = min(self.maxlen, items.size)
            self.table[r, self.maxlen - n:] = items[-n:]
        self.rng = np.random.default_rng(seed)
        self.last_forced = None

    def next_batch(self):
        rows = self.rng.integers(0, self.users.size, self.batch_size)
        hist = self.table[rows]
        real = hist != 0
        masked = real & (self.rng.random(hist.shape) < self.mask_prob)
        self.last_forced = ~masked.any(1)
        masked[self.last_forced, -1] = True        # left-padded: the last position is always real
        seq = np.where(masked, self.mask_id, hist)
        labels = np.where(masked, hist, 0)
        return self.users[rows], seq, labels

    def close(self):
        """Owns nothing."""


class WindowSampler:
    """Host-side batches for Caser: every stride-1 window of ``L + T`` consecutive items of every user, the first ``L``
    as the input sequence and the last ``T`` as the targets.  A history shorter than ``L + T`` becomes ONE window,
    left-padded with 0 (its targets are all real); a user with ``len <= T`` has no input and is left out.

    ``user_train``: dict user id -> list of item ids (1-based, in time order).  An epoch is one pass: ``len(sampler)``
    batches of ``(users [B], seq [B, L], pos [B, T], neg [B, neg_samples])`` int64 arrays in a fresh random order, the
    last batch ragged.  The negatives are uniform over ``1 .. n_items`` outside the user's own set and are redrawn every
    epoch.  The same ``seed`` gives the same epochs."""

    def __init__(self, user_train, n_users, n_items, batch_size, L, T, neg_samples, seed=0):
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.batch_size, self.L, self.T, self.neg_samples = int(batch_size), int(L), int(T), int(neg_samples)
        if min(self.batch_size, self.L, self.T, self.neg_samples) < 1:
            raise ValueError("batch_size, L, T and neg_samples must be >= 1")
        users, windows, keys = [], [], []
        width = self.L + self.T
        for u in sorted(user_train):
            items = np.asarray(user_train[u], dtype=np.int64).reshape(-1)
            if not 0 <= int(u) < self.n_users:
                raise IndexError(f"user {u} outside [0, {self.n_users})")
            if items.size and (items.min() < 1 or items.max() > self.n_items):
                raise IndexError(f"user {u} holds an item outside [1, {self.n_items}]")
            if items.size <= self.T:
                continue
            own = np.unique(items)
            if own.size >= self.n_items:
                raise ValueError(f"user {u} has interacted with every item: no negative can be drawn")
            keys.append(int(u) * (self.n_items + 1) + own)
            if items.size < width:
                w = np.zeros((1, width), dtype=np.int64)
                w[0, width - items.size:] = items
            else:
                w = np.lib.stride_tricks.sliding_window_view(items, width)
            users.append(np.full(w.shape[0], int(u), dtype=np.int64))
            windows.append(w)
        if not windows:
            raise ValueError(f"no user has more than T = {self.T} items")
        self.users = np.concatenate(users)
        self.windows = np.ascontiguousarray(np.concatenate(windows))
        self._keys = np.concatenate(keys)       # sorted: users ascending, each user's items ascending
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return (self.users.size + self.batch_size - 1) // self.batch_size

    def _draw_negatives(self):
        n = self.users.size
        neg = self.rng.integers(1, self.n_items + 1, (n, self.neg_samples))
        base = self.users[:, None] * (self.n_items + 1)
        while True:
            key = base + neg
            at = np.minimum(np.searchsorted(self._keys, key), self._keys.size - 1)
            hit = self._keys[at] == key
            if not hit.any():
                return neg
            neg[hit] = self.rng.integers(1, self.n_items + 1, int(hit.sum()))

    def __iter__(self):
        order = self.rng.permutation(self.users.size)
        neg = self._draw_negatives()
        for s in range(0, order.size, self.batch_size):
            idx = order[s:s + self.batch_size]
            w = self.windows[idx]
            yield self.users[idx], w[:, :self.L], w[:, self.L:], neg[idx]

    def close(self):
        """Owns nothing."""


def last_window(user_train, L):
    """The query sequences of Caser: the last ``L`` items of every history, left-padded with 0.  ``user_train``: a dict
    user id -> item list, which gives ``(users [n], seq [n, L])`` with the users ascending, or a list of item lists,
    which gives ``seq [n, L]`` in the list's order.  int64 arrays."""
    L = int(L)
    if L < 1:
        raise ValueError("L must be >= 1")
    by_user = isinstance(user_train, dict)
    users = sorted(user_train) if by_user else None
    hists = [user_train[u] for u in users] if by_user else list(user_train)
    seq = np.zeros((len(hists), L), dtype=np.int64)
    for r, h in enumerate(hists):
        items = np.asarray(h, dtype=np.int64).reshape(-1)[-L:]
        seq[r, L - items.size:] = items
    return (np.asarray(users, dtype=np.int64), seq) if by_user else seq


def instance_vae_loader(users, items, n_users, n_items):
    """``(user_indices, matrix)`` as base_data.py:513-532 hands them to ``VAECFEngine.train_an_epoch``: the ids of the
    users that occur, ascending, and the ``[n_users, n_items]`` scipy CSR matrix of the interactions (one per distinct
    pair; the epoch loop binarises it anyway)."""
    from scipy.sparse import csr_matrix

    u = np.asarray(users.cpu() if torch.is_tensor(users) else users, dtype=np.int64).reshape(-1)
    i = np.asarray(items.cpu() if torch.is_tensor(items) else items, dtype=np.int64).reshape(-1)
    if u.shape != i.shape:
        raise ValueError("users and items differ in length")
    if u.size and (u.min() < 0 or u.max() >= n_users or i.min() < 0 or i.max() >= n_items):
        raise IndexError("training frame holds a user / item id outside [0, n_users) x [0, n_items)")
    matrix = csr_matrix((np.ones(len(u), dtype=np.float32), (u, i)), shape=(n_users, n_items))
    matrix.data[:] = 1.0
    return np.unique(u), matrix


def time_relation(time_seq, time_span):
    """The reference's ``computeRePos`` (beta_rec/recommenders/tisasrec.py:108-127) for one ``[T]`` sequence or a batch
    ``[B, T]`` of them: ``min(|t_i - t_j|, time_span)`` as int32 ``[..., T, T]``."""
    ts = np.asarray(time_seq, dtype=np.int64)
    return np.minimum(np.abs(ts[..., :, None] - ts[..., None, :]), int(time_span)).astype(np.int32)


class TimeSequenceSampler(SequenceSampler):
    """Host-side batches for TiSASRec, by the rule of the reference's ``sample_function``
    (beta_rec/recommenders/tisasrec.py:220-279), vectorised like :class:`SequenceSampler`: what that class draws, plus
    ``time_seq`` (the time stamps of ``seq``, 0 at padded positions) and ``time_matrix = time_relation(time_seq,
    time_span)`` (the reference looks the latter up in a per-user table it builds beforehand by the same rule).

    ``user_train``: dict user id -> list of ``[item, time]`` pairs (items 1-based, integer times, in time order).
    ``next_batch()`` returns ``(users [B], seq [B, maxlen], time_seq [B, maxlen], time_matrix [B, maxlen, maxlen] int32,
    pos [B, maxlen], neg [B, maxlen])`` -- what ``TiSASRecEngine.train_an_epoch`` asks for."""

    def __init__(self, user_train, n_users, n_items, batch_size, maxlen, time_span, seed=0):
        for u, pairs in user_train.items():
            if any(len(p) != 2 for p in pairs):
                raise ValueError(f"user {u}: every entry must be an [item, time] pair")
        super().__init__({u: [p[0] for p in pairs] for u, pairs in user_train.items()}, n_users, n_items, batch_size,
                         maxlen, seed)
        self.time_span = int(time_span)
        if self.time_span < 1:
            raise ValueError("time_span must be >= 1")
        self.times = {int(u): np.asarray([p[1] for p in user_train[u]], dtype=np.int64) for u in self.users}

    def next_batch(self):
        users, seq, pos, neg = super().next_batch()
        B, T = seq.shape
        time_seq = np.zeros((B, T), dtype=np.int64)
        for b, u in enumerate(users):
            times = self.times[int(u)]
            n = min(T, times.size - 1)
            time_seq[b, T - n:] = times[-n - 1:-1]
        return users, seq, time_seq, time_relation(time_seq, self.time_span), pos, neg


# ---- session batches for NARM (beta_rec/datasets/seq_data_utils.py) -------------------------------------------------------
def session_prefixes(sequences):
    """``dataset_to_seq_target_format`` (seq_data_utils.py:107-128) on a list of item sequences: for each sequence and
    ``i = 1 .. len - 1`` the pair ``(seq[:-i], seq[-i])``, in that order.  Returns ``(out_seqs, labels)``."""
    out_seqs, labs = [], []
    for seq in sequences:
        seq = list(seq)
        for i in range(1, len(seq)):
            labs.append(seq[-i])
            out_seqs.append(seq[:-i])
    return out_seqs, labs


class SessionLoader:
    """What ``DataLoader(SeqDataset((out_seqs, labels)), batch_size, shuffle=False, collate_fn=collate_fn)`` yields
    (seq_data_utils.py:131-179): the batches in order; within a batch the sessions sorted by length, descending and
    stable; the ids zero-padded to the batch's longest and time-major ``[T, B]`` int64, the labels ``[B]`` in the sorted
    order, the lengths as a list.  Re-iterable: one loader serves every epoch.  The ragged arrays are built once; a batch
    is cut from them with array operations only.

    ``shuffle=True`` (SR-GNN's published training; NARM's does not shuffle): the sessions are permuted by
    ``np.random.default_rng(seed)`` before they are cut into batches, anew at every iteration of the loader (the
    generator lives as long as the loader, so the epochs differ and one seed gives one run)."""

    def __init__(self, out_seqs, labels, batch_size, shuffle=False, seed=None):
        if len(out_seqs) != len(labels):
            raise ValueError("one label per session is needed")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be >= 1")
        self.batch_size = int(batch_size)
        self._lens = np.fromiter((len(s) for s in out_seqs), dtype=np.int64, count=len(out_seqs))
        if self._lens.size and int(self._lens.min()) < 1:
            raise ValueError("every session needs at least one item")
        self._flat = (np.concatenate([np.asarray(s, dtype=np.int64) for s in out_seqs]) if len(out_seqs)
                      else np.zeros(0, dtype=np.int64))
        self._start = np.concatenate([[0], np.cumsum(self._lens)[:-1]]).astype(np.int64) if len(out_seqs) else self._lens
        self._labels = np.asarray(labels, dtype=np.int64).reshape(-1)
        self.shuffle = bool(shuffle)
        self._rng = np.random.default_rng(seed) if self.shuffle else None

    def __len__(self):
        return (self._lens.size + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        perm = self._rng.permutation(self._lens.size) if self.shuffle else None
        for lo in range(0, self._lens.size, self.batch_size):
            hi = min(lo + self.batch_size, self._lens.size)
            if perm is None:
                order = lo + np.argsort(-self._lens[lo:hi], kind="stable")
            else:
                chunk = perm[lo:hi]
                order = chunk[np.argsort(-self._lens[chunk], kind="stable")]
            lens = self._lens[order]
            T = int(lens[0])
            pos = np.arange(T, dtype=np.int64)[None, :]
            real = pos < lens[:, None]
            padded = np.zeros((hi - lo, T), dtype=np.int64)
            padded[real] = self._flat[(self._start[order][:, None] + pos)[real]]
            yield (torch.from_numpy(np.ascontiguousarray(padded.T)), torch.from_numpy(self._labels[order].copy()),
                   lens.tolist())


# ---- session-parallel mini-batches for GRU4Rec (Hidasi et al., ICLR 2016, section 3.1) -------------------------------------
class SessionParallelLoader:
    """``batch_size`` slots each walk one session, one event per step; a step is ``(in_items [B], targets [B],
    reset [B] uint8, samples [n_sample])``.

    ``sessions``: a ragged list of id lists (ids in ``0 .. n_items - 1``, time order); sessions shorter than 2 are dropped
    with a warning.  Slots take the sessions in order.  A slot whose session has no next event takes the next unused
    session and sets ``reset`` for that step (every slot's first step has it set); the epoch ends when a slot cannot be
    refilled, so every step is full.  The walk is built on the host once: ``in_items``, ``targets``, ``reset`` are
    ``[n_steps, B]`` arrays.  The extra samples of an epoch, ``[n_steps, n_sample]``, are drawn with probability
    proportional to ``support ** sample_alpha`` from ``np.random.default_rng(seed + epoch)`` (``epoch`` counts the
    iterations of this loader).  The arrays are uploaded to ``device`` once per epoch and iterated as slices of them
    (``device=None``: host tensors; ``GRU4RecEngine.train_an_epoch`` sets the model's device on such a loader).

    ``support [n_items]``: events per item over the kept sessions; ``item_probs``: its share, which the engine's logQ
    shift reads."""

    def __init__(self, sessions, n_items, batch_size, n_sample, sample_alpha, seed=0, device=None):
        import warnings

        self.n_items, self.batch_size, self.n_sample = int(n_items), int(batch_size), int(n_sample)
        self.sample_alpha, self.seed, self.device = float(sample_alpha), int(seed), device
        if self.n_items < 1 or self.batch_size < 1 or self.n_sample < 0:
            raise ValueError("n_items and batch_size must be >= 1 and n_sample >= 0")
        kept = [np.asarray(s, dtype=np.int64).reshape(-1) for s in sessions]
        short = sum(1 for s in kept if s.size < 2)
        if short:
            warnings.warn(f"{short} sessions with fewer than 2 events were dropped")
        kept = [s for s in kept if s.size >= 2]
        if len(kept) < self.batch_size:
            raise ValueError(f"{len(kept)} sessions of 2 or more events cannot fill {self.batch_size} slots")
        events = np.concatenate(kept)
        if int(events.min()) < 0 or int(events.max()) >= self.n_items:
            raise IndexError(f"a session holds an item outside [0, {self.n_items})")
        self.support = np.bincount(events, minlength=self.n_items).astype(np.int64)
        self.item_probs = self.support / float(self.support.sum())
        weights = self.support.astype(np.float64) ** self.sample_alpha
        weights[self.support == 0] = 0.0      # 0 ** 0 = 1: an item without an event is never drawn
        self._cdf = np.cumsum(weights / weights.sum())
        self._last = int(np.flatnonzero(weights)[-1])      # where a draw beyond the rounded cdf's end lands
        B = self.batch_size
        sess = list(range(B))                 # the session of every slot
        at = [0] * B                          # the slot's input event inside it
        nxt = B
        fresh = [1] * B
        ins, tgts, rsts = [], [], []
        while True:
            for b in range(B):
                if at[b] + 1 >= kept[sess[b]].size:
                    if nxt >= len(kept):
                        nxt = -1
                        break
                    sess[b], at[b], fresh[b] = nxt, 0, 1
                    nxt += 1
            if nxt < 0:
                break
            ins.append([kept[sess[b]][at[b]] for b in range(B)])
            tgts.append([kept[sess[b]][at[b] + 1] for b in range(B)])
            rsts.append(list(fresh))
            at = [a + 1 for a in at]
            fresh = [0] * B
        self.in_items = np.asarray(ins, dtype=np.int64).reshape(-1, B)
        self.targets = np.asarray(tgts, dtype=np.int64).reshape(-1, B)
        self.reset = np.asarray(rsts, dtype=np.uint8).reshape(-1, B)
        self.samples = None                   # [n_steps, n_sample] of the epoch drawn last
        self.epoch = 0

    def __len__(self):
        return self.in_items.shape[0]

    def draw_samples(self, epoch):
        """The ``[n_steps, n_sample]`` extra samples of ``epoch``."""
        rng = np.random.default_rng(self.seed + int(epoch))
        u = rng.random((len(self), self.n_sample))
        return np.minimum(np.searchsorted(self._cdf, u, side="right"), self._last).astype(np.int64)

    def __iter__(self):
        self.samples = self.draw_samples(self.epoch)
        self.epoch += 1
        arrays = [torch.from_numpy(a) for a in (self.in_items, self.targets, self.reset, self.samples)]
        if self.device is not None:
            arrays = [a.to(self.device) for a in arrays]
        for t in range(len(self)):
            yield tuple(a[t] for a in arrays)

    def close(self):
        """Owns nothing."""


def hypergraph_laplacians(users, items, n_users, n_items):
    """The user and item hypergraph Laplacians of deprecated_data_base.py:420-452 as scipy CSR matrices:
    ``L_u = I - D_u^-1/2 H D_v^-1 H^T D_u^-1/2`` and the same with the roles swapped.  ``H`` is the binary incidence
    matrix (a repeated pair is one entry); the degrees count every interaction, repeated ones included, and are clamped
    from below as the reference clamps them (``max(sqrt(d), 1e-10)``, ``max(d, 1e-10)``)."""
    import scipy.sparse as sp

    users, items = np.asarray(users, dtype=np.int64).reshape(-1), np.asarray(items, dtype=np.int64).reshape(-1)
    if users.size != items.size:
        raise ValueError("users and items differ in length")
    if users.size and (users.min() < 0 or users.max() >= n_users or items.min() < 0 or items.max() >= n_items):
        raise ValueError("an interaction lies outside n_users x n_items")
    epsilon = 0.1 ** 10
    H = sp.csr_matrix((np.ones(users.size), (users, items)), shape=(n_users, n_items))
    H.data[:] = 1.0                                       # the constructor summed repeated pairs
    d_u = np.bincount(users, minlength=n_users).astype(np.float64)
    d_v = np.bincount(items, minlength=n_items).astype(np.float64)
    out = []
    for Hs, d_node, d_edge in ((H, d_u, d_v), (H.T.tocsr(), d_v, d_u)):
        D_n = sp.diags(1.0 / np.maximum(np.sqrt(d_node), epsilon))
        D_e = sp.diags(1.0 / np.maximum(d_edge, epsilon))
        out.append((sp.identity(Hs.shape[0]) - D_n @ Hs @ D_e @ Hs.T @ D_n).tocsr())
    return out


def graph_embeddings(users, items, n_users, n_items, cut_off):
    """``[P, Q]`` for ``LCFN``: the ``int(cut_off * n)`` lowest-frequency eigenvectors of the two hypergraph Laplacians
    (deprecated_data_base.py:411-467: ``eigsh(L, k, which="SM", tol=1e-5)``), as fp32 arrays ``[n_users, F_u]`` and
    ``[n_items, F_i]`` with ascending eigenvalues.  One-off host preprocessing; an eigenvector's sign is arbitrary."""
    from scipy.sparse.linalg import eigsh

    out = []
    for L, n in zip(hypergraph_laplacians(users, items, n_users, n_items), (n_users, n_items)):
        k = int(cut_off * n)
        if not 1 <= k < n:
            raise ValueError(f"cut_off {cut_off} keeps {k} of {n} frequencies: 1 .. n - 1 are possible")
        lam, vec = eigsh(L, k=k, which="SM", tol=0.1 ** 5)
        order = np.argsort(lam, kind="stable")
        out.append(np.ascontiguousarray(vec[:, order], dtype=np.float32))
    return out
