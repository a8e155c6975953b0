"""IndexTrie -- the prefix trie over the tuples of an index file, for the two consumers of an index: constrained generation (the
exact set of tokens that may follow a prefix) and the way back from a tuple to the catalogue items that hold it.

Beyond the reference, which keeps one set of allowed tokens per POSITION (data.py:67-89: on a 3 x 48 index of 3 000 items those
sets admit 48 * 48 * 47 tuples where the file holds 2 931) and has no tuple -> item lookup.  include/lcrec.h, lcrec_index_trie,
states the layout and the three rules; the device work is ops.trie_build, ops.trie_find and ops.trie_mask_logits_.
"""
import numpy as np
import torch

from . import ops


class IndexTrie:
    """The trie of an int64 [n, L] index matrix on a HIP device.  Arrays (device tensors, trimmed to what the build wrote):
    order [n], counts [L + 1] (also on the host as the list `nodes`), child: L rows, code: L rows, first [leaves + 1]."""

    def __init__(self, trie):
        self._trie = trie
        self.n, self.L, self.ks, self.device = trie.n, trie.L, list(trie.ks), trie.device
        a = trie.arrays
        self.nodes = [int(v) for v in a["counts"][:self.L + 1].tolist()]           # the one read of device data
        n, L = self.n, self.L
        self.order, self.counts = a["order"][:n], a["counts"][:L + 1]
        self.child = [a["child"][d * (n + 1):d * (n + 1) + (self.nodes[d] + 1 if n else 1)] for d in range(L)]
        self.code = [a["code"][d * n:d * n + self.nodes[d + 1]] for d in range(L)]
        self.first = a["first"][:self.nodes[L] + 1]
        self._host = None

    # ---- construction ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_indices(cls, idx, ks):
        """idx: int64 [n, L] on a HIP device (codes outside a level's range count as the nearest valid code, as everywhere)."""
        return cls(ops.trie_build(idx, ks))

    @classmethod
    def from_file(cls, path, ks, device="cuda:0"):
        """An `.index.json` through generate_indices.load_index_json (ValueError for a file that does not fit ks)."""
        from .generate_indices import load_index_json
        return cls.from_indices(torch.from_numpy(load_index_json(path, ks)).to(torch.device(device)), ks)

    # ---- device queries ------------------------------------------------------------------------------------------------------------
    def _rows(self, t, name):
        t = torch.as_tensor(t)
        if t.dtype != torch.int64:
            raise ValueError(f"{name} must be int64, got {t.dtype}")
        return t.to(self.device)

    def find(self, prefixes, depth=None, longest=False):
        """prefixes int64 [B, depth] (depth: its width): the node of depth `depth` every row leads to, -1 where there is none; with
        longest, (the deepest node on the row's path, its depth) instead.  Query codes outside [0, K) match nothing."""
        prefixes = self._rows(prefixes, "prefixes")
        if prefixes.dim() != 2:
            raise ValueError(f"prefixes must be [B, depth], got {tuple(prefixes.shape)}")
        depth = prefixes.shape[1] if depth is None else int(depth)
        return ops.trie_find(self._trie, prefixes, depth, longest=longest)

    def mask_logits_(self, logits, nodes, depth, token_ids=None, eos_token_id=-1):
        """In place: every logit of row b outside the tokens that may follow node nodes[b] of depth `depth` becomes -inf (at depth L,
        and at a dead node such as find's -1, eos alone may follow).  token_ids: int32 [ks[depth]], the token of every code of that
        level; None: the codes themselves.  Returns logits."""
        if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32:
            raise ValueError(f"logits must be a float32 tensor, got {getattr(logits, 'dtype', type(logits).__name__)}")
        if logits.device != self.device:
            raise ValueError(f"logits is on {logits.device} but the trie on {self.device}")
        if token_ids is not None:
            token_ids = torch.as_tensor(token_ids, dtype=torch.int32).to(self.device).contiguous()
        ops.trie_mask_logits_(self._trie, logits, self._rows(nodes, "nodes").contiguous(), depth, token_ids, int(eos_token_id))
        return logits

    def span(self, nodes, depth):
        """(lo, hi) int64 [B]: the positions of `order` under each node of depth `depth` -- down the child chain to the leftmost leaf
        of the node and of its right neighbour.  Nodes must be live."""
        lo = self._rows(nodes, "nodes")
        hi = lo + 1
        if self.n == 0:                                                            # (the root of an empty trie has no child row to follow)
            return torch.zeros_like(lo), torch.zeros_like(lo)
        for d in range(int(depth), self.L):
            lo, hi = self.child[d][lo], self.child[d][hi]
        return self.first[lo], self.first[hi]

    def lookup(self, tuples):
        """tuples int64 [B, L] -> (item_ids, offsets) in CSR form: row b's holders are item_ids[offsets[b]:offsets[b + 1]], ascending,
        none where no item holds the tuple."""
        leaf = self.find(tuples, self.L)
        B = leaf.shape[0]
        offsets = torch.zeros(B + 1, dtype=torch.int64, device=self.device)
        if B == 0 or self.n == 0:
            return self.order[:0], offsets
        hit = leaf >= 0
        at = torch.where(hit, leaf, torch.zeros_like(leaf))
        lo = self.first[at]
        size = torch.where(hit, self.first[at + 1] - lo, torch.zeros_like(lo))
        offsets[1:] = torch.cumsum(size, 0)
        total = int(offsets[-1])
        row = torch.repeat_interleave(torch.arange(B, device=self.device), size, output_size=total)
        pos = lo[row] + torch.arange(total, device=self.device) - offsets[row]
        return self.order[pos], offsets

    # ---- host side -------------------------------------------------------------------------------------------------------------------
    def host(self):
        """numpy copies of the arrays: dict(order, counts, child, code, first), made once"""
        if self._host is None:
            cpu = lambda t: t.cpu().numpy()
            self._host = {"order": cpu(self.order), "counts": np.array(self.nodes, dtype=np.int64), "child": [cpu(c) for c in self.child],
                          "code": [cpu(c) for c in self.code], "first": cpu(self.first)}
        return self._host

    def stats(self):
        """nodes per depth, the largest leaf (items on one tuple), mean and maximum children per depth"""
        h = self.host()
        leaf = np.diff(h["first"]) if self.n else np.zeros(0, np.int64)
        kids = [np.diff(c) if self.n else np.zeros(0, np.int64) for c in h["child"]]
        return {"items": int(self.n), "nodes": list(self.nodes), "largest_leaf": int(leaf.max()) if leaf.size else 0,
                "mean_children": [float(k.mean()) if k.size else 0.0 for k in kids],
                "max_children": [int(k.max()) if k.size else 0 for k in kids]}

    def prefix_allowed_tokens_fn(self, token_ids_per_level, eos_token_id, sep_ids):
        """The callable `generate(prefix_allowed_tokens_fn=...)` takes, with the signature and the prompt-separator search of the
        reference's (data.py:81-87), answering from the trie: after the i tokens that follow the last `sep_ids`, the tokens of the
        codes that continue that very prefix in the file -- not every code that occurs at position i.  After a whole tuple, and after
        a prefix no item holds, eos alone.  token_ids_per_level[l][c]: the token id of code c of level l.  Walks host copies."""
        h = self.host()
        tokens = [np.asarray(t, dtype=np.int64) for t in token_ids_per_level]
        if len(tokens) != self.L or any(len(t) < k for t, k in zip(tokens, self.ks)):
            raise ValueError(f"token_ids_per_level must hold {self.L} tables of at least {self.ks} ids")
        code_of = [{int(t): c for c, t in reversed(list(enumerate(tab[:k])))} for tab, k in zip(tokens, self.ks)]
        sep = [int(t) for t in sep_ids]
        rsep = sep[::-1]
        eos = [int(eos_token_id)]
        n = self.n

        def prefix_allowed_tokens_fn(batch_id, sentence):
            sentence = sentence.tolist()
            reversed_sent = sentence[::-1]
            for i in range(len(reversed_sent)):
                if reversed_sent[i:i + len(sep)] == rsep:
                    if i >= self.L or n == 0:
                        return list(eos) if i >= self.L else []
                    node = 0
                    for d, tok in enumerate(sentence[len(sentence) - i:]):
                        c = code_of[d].get(int(tok))
                        lo, hi = (int(h["child"][d][node]), int(h["child"][d][node + 1])) if c is not None else (0, 0)
                        k = lo + int(np.searchsorted(h["code"][d][lo:hi], c)) if c is not None else hi
                        if k >= hi or int(h["code"][d][k]) != c:
                            return list(eos)
                        node = k
                    lo, hi = int(h["child"][i][node]), int(h["child"][i][node + 1])
                    return [int(tokens[i][c]) for c in h["code"][i][lo:hi]]

        return prefix_allowed_tokens_fn
