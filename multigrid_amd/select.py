"""Selection on the device (include/mgx.h "SELECTION"): the k best of n by (score, index), as a list of fixed length with the count
kept on the device -- the beam cut of a search level, and with no scores a `nonzero` of fixed shape.  O(n), six launches with scores
and two without, no host round trip, capturable in a graph."""
from __future__ import annotations

import collections

import torch

#: what `Selector.select` returns: index int64 [k], count int32 [2] = (entries of `index` that are chosen, candidates there were)
Selection = collections.namedtuple("Selection", ("index", "count"))

_INT64 = (-(1 << 63), (1 << 63) - 1)


class Selector:
    """Selects among up to `n_max` items on `device`.  It owns the work buffer of the calls (include/mgx.h: mgx_select_work_bytes), so
    a `select(..., out=)` allocates nothing; one selector takes one call at a time (calls on one stream are ordered).

    backend: the launcher (`select` / `select_work_bytes`); product code leaves it None (= ops.SelectOps on a HIP device)."""

    def __init__(self, n_max: int, device, backend=None):
        if isinstance(n_max, bool) or not isinstance(n_max, int) or not 1 <= n_max < 2 ** 31:
            raise ValueError(f"Selector: n_max must be an int in [1, 2**31), got {n_max!r}")
        self.n_max = n_max
        self.device = torch.device(device)
        if backend is None:
            from .ops import SelectOps
            backend = SelectOps(self.device)
        self.backend = backend
        # (int64 elements: torch aligns an allocation far beyond the 16 bytes the entry point asks for)
        self.work = torch.empty((backend.select_work_bytes(n_max) + 7) // 8, dtype=torch.int64, device=self.device)

    def _arg(self, name: str, t, dtypes, shape):
        if t is None:
            return shape
        if not torch.is_tensor(t) or t.dtype not in dtypes or t.device != self.device or not t.is_contiguous():
            raise ValueError(f"select: {name} must be a contiguous {' or '.join(str(d).split('.')[-1] for d in dtypes)} tensor on "
                             f"{self.device}")
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"select: {name} must have the shape of the other inputs, {shape}, got {tuple(t.shape)}")
        return tuple(t.shape)

    def select(self, score: torch.Tensor | None = None, keep: torch.Tensor | None = None, *, k: int, values: torch.Tensor | None = None,
               fill: int = -1, out: Selection | None = None) -> Selection:
        """The `k` best of the items at which `keep` is set, by (score, flattened index), on the current stream (mgx_select): no host
        work, no synchronisation, capturable in a graph.  Returns Selection(index int64 [k], count int32 [2]).

        score    contiguous int32 tensor of any shape, smaller is better; None: the order is by index alone
        keep     contiguous bool or uint8 tensor of the same shape, non-zero = a candidate; None: every item is one
        values   contiguous int64 tensor of the same shape: `values[i]` is written in place of i
        At least one of score and keep is required; the inputs are flattened, and hold at most `n_max` items.

        With m = min(k, candidates), `index[:m]` holds the m best candidates in ASCENDING index -- the set `argsort(stable)[:m]`
        picks, sorted -- and `index[m:]` is `fill`; count = (m, candidates), so a cut shows as count[1] > count[0].  With score=None
        this is `nonzero(keep)` in a fixed shape.  out= takes a previous result of the same k to write into."""
        shape = self._arg("score", score, (torch.int32,), None)
        shape = self._arg("keep", keep, (torch.bool, torch.uint8), shape)
        if score is None and keep is None:
            raise ValueError("select: at least one of score and keep is required")
        self._arg("values", values, (torch.int64,), shape)
        n = 1
        for s in shape:
            n *= int(s)
        if n > self.n_max:
            raise ValueError(f"select: the inputs hold {n} items, this Selector takes at most n_max = {self.n_max}")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k < 2 ** 31:
            raise ValueError(f"select: k must be an int in [1, 2**31), got {k!r}")
        if isinstance(fill, bool) or not isinstance(fill, int) or not _INT64[0] <= fill <= _INT64[1]:
            raise ValueError(f"select: fill must be an int that fits int64, got {fill!r}")
        if out is None:
            out = Selection(torch.empty(k, dtype=torch.int64, device=self.device), torch.empty(2, dtype=torch.int32, device=self.device))
        else:
            if not isinstance(out, Selection):
                raise ValueError("select: out= must be a Selection that an earlier select returned")
            for name, t, dtype, want in (("index", out.index, torch.int64, (k,)), ("count", out.count, torch.int32, (2,))):
                if not torch.is_tensor(t) or t.dtype is not dtype or tuple(t.shape) != want or t.device != self.device \
                        or not t.is_contiguous():
                    raise ValueError(f"select: out=.{name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {want} on "
                                     f"{self.device}")
        self.backend.select(n, score, keep, values, k, fill, out.index, out.count, self.work)
        return out
