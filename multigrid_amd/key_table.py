"""Visited-state tables on the device (include/mgx.h "KEY TABLES"): a set of 64-bit keys with a stable entry id per key, visit
counts, and "which of these keys are new, and who holds each first" -- two launches per insert, one per lookup, constant memory, no
host round trip, capturable in a graph.  The keys are `state_key()` / `obs_key()` outputs or any int64 numbers of the caller's."""
from __future__ import annotations

import collections

import torch

from . import _lib

#: what `KeyTable.insert` returns; outputs not asked for are None
KeyInsert = collections.namedtuple("KeyInsert", ("entry", "is_new", "first", "visits"))
#: what `KeyTable.lookup` returns
KeyLookup = collections.namedtuple("KeyLookup", ("entry", "visits"))

_MEMBERS = ("keys", "tag", "born", "visits", "ctrl")


def _check_capacity(what: str, capacity) -> int:
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not _lib.KEY_MIN_CAPACITY <= capacity <= _lib.KEY_MAX_CAPACITY \
            or capacity & (capacity - 1):
        raise ValueError(f"{what}: capacity must be a power of two in [{_lib.KEY_MIN_CAPACITY}, 2**30], got {capacity!r}")
    return capacity


class KeyTable:
    """A table of `capacity` slots on `device`.  It maps a key to an ENTRY ID in [0, capacity) that stays the same until `clear()`:
    keep what you want per entry (best score, snapshot row, parent, depth) in tensors of your own indexed by that id.

    Placement is open addressing with linear probing inside a window of 1024 slots from the key's home; entries are never removed,
    and a table does not grow (make a bigger one and insert `old.keys[old.occupied()]`).  A key whose window is full is DROPPED:
    its entry is -1 and `dropped()` / `check_errors()` say so -- keep the load at a half or below.  The key 0 is stored and answered
    as the key 1.  One table takes one call at a time (calls on one stream are ordered; two streams must be ordered by the caller).

    The storage is ONE zero-initialised int64 buffer (24 * capacity + 32 bytes) and the five arrays of include/mgx.h's MgxKeyTable
    are views of it: `keys` int64 [capacity] (0 = empty), `tag` int64 [capacity], `born` int32 [capacity], `visits` int32
    [capacity], `ctrl` int32 [8].  All-zero storage is the empty table.

    backend: the launcher (`key_insert` / `key_lookup`); product code leaves it None (= ops.KeyTableOps on a HIP device)."""

    def __init__(self, capacity: int, device, backend=None):
        self.capacity = _check_capacity("KeyTable", capacity)
        self.device = torch.device(device)
        if backend is None:
            from .ops import KeyTableOps
            backend = KeyTableOps(self.device)
        self.backend = backend
        c = capacity
        self._buf = torch.zeros(3 * c + _lib.KEY_CTRL_WORDS // 2, dtype=torch.int64, device=self.device)
        self.keys, self.tag = self._buf[:c], self._buf[c:2 * c]
        self.born, self.visits = self._buf[2 * c:2 * c + c // 2].view(torch.int32), self._buf[2 * c + c // 2:3 * c].view(torch.int32)
        self.ctrl = self._buf[3 * c:].view(torch.int32)
        self.storage = {"capacity": c, **{m: getattr(self, m) for m in _MEMBERS}}

    # ------------------------------------------------------------------------------------------ arguments
    def _keys_arg(self, what: str, keys) -> torch.Tensor:
        if not torch.is_tensor(keys) or keys.dtype is not torch.int64 or keys.device != self.device or not keys.is_contiguous():
            raise ValueError(f"{what}: keys must be a contiguous int64 tensor on {self.device}")
        return keys

    def _out(self, what: str, name: str, prev, want: bool, shape, dtype):
        """output `name` of a call: None when not asked for, the tensor of `out=` when there is one, else a new one"""
        if not want:
            return None
        if prev is None:
            return torch.zeros(shape, dtype=dtype, device=self.device)
        if not torch.is_tensor(prev) or prev.dtype is not dtype or tuple(prev.shape) != tuple(shape) or prev.device != self.device \
                or not prev.is_contiguous():
            raise ValueError(f"{what}: out=.{name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {tuple(shape)} on "
                             f"{self.device}")
        return prev

    # ------------------------------------------------------------------------------------------ insert / lookup
    def insert(self, keys: torch.Tensor, *, is_new: bool = True, first: bool = False, visits: bool = False, count: bool = True,
               out: KeyInsert | None = None) -> KeyInsert:
        """Insert `keys` -- any contiguous int64 tensor on the table's device; `venv.obs_key()`'s [B, A] goes in as it is -- by TWO
        launches (mgx_key_insert) on the current stream: no host work, no synchronisation, capturable in a graph.  Returns
        KeyInsert(entry, is_new, first, visits), each of the shape of `keys`, those not asked for None.  Apart from the VALUES of
        `entry` the outputs are those of inserting the keys one after another in (flattened) index order:

        entry    int64: the id of the key's entry -- equal for equal keys, different for different keys, the same from every later
                 insert and lookup; -1 for a dropped key.  Which number an entry gets is not reproducible from run to run.
        is_new   bool: True at exactly one index per key the table did not hold before this call, the smallest
        first    int64: the smallest flattened index of this call that holds the same key (-1 for a dropped key)
        visits   int32: how often the key has been inserted in the table's life, this call included (0 for a dropped key)

        count=False inserts without counting (pure set semantics).  out= takes a previous result to write into, so a caller that
        inserts every step allocates nothing; it must hold a tensor for every output asked for."""
        keys = self._keys_arg("insert", keys)
        if out is not None and not isinstance(out, KeyInsert):
            raise ValueError("insert: out= must be a KeyInsert that an earlier insert returned")
        prev = out if out is not None else KeyInsert(None, None, None, None)
        if out is not None:
            for name, want in (("entry", True), ("is_new", is_new), ("first", first), ("visits", visits)):
                if want and getattr(prev, name) is None:
                    raise ValueError(f"insert: out= holds no `{name}` to write into")
        shape = tuple(keys.shape)
        res = KeyInsert(self._out("insert", "entry", prev.entry, True, shape, torch.int64),
                        self._out("insert", "is_new", prev.is_new, bool(is_new), shape, torch.bool),
                        self._out("insert", "first", prev.first, bool(first), shape, torch.int64),
                        self._out("insert", "visits", prev.visits, bool(visits), shape, torch.int32))
        self.backend.key_insert(self.storage, int(keys.numel()), keys, 0 if count else _lib.KEY_NO_COUNT, *res)
        return res

    def lookup(self, keys: torch.Tensor, *, visits: bool = False, out: KeyLookup | None = None) -> KeyLookup:
        """Look `keys` up by ONE read-only launch (mgx_key_lookup) on the current stream: KeyLookup(entry, visits) of the shape of
        `keys`; entry is -1 and visits 0 for a key the table does not hold.  `visits` is None unless asked for; out= as in insert."""
        keys = self._keys_arg("lookup", keys)
        if out is not None and not (isinstance(out, tuple) and len(out) == 2):
            raise ValueError("lookup: out= must be a KeyLookup that an earlier lookup returned")
        prev = KeyLookup(*out) if out is not None else KeyLookup(None, None)
        if out is not None and ((visits and prev.visits is None) or prev.entry is None):
            raise ValueError("lookup: out= holds no tensor for an output asked for")
        shape = tuple(keys.shape)
        res = KeyLookup(self._out("lookup", "entry", prev.entry, True, shape, torch.int64),
                        self._out("lookup", "visits", prev.visits, bool(visits), shape, torch.int32))
        self.backend.key_lookup(self.storage, int(keys.numel()), keys, *res)
        return res

    # ------------------------------------------------------------------------------------------ the table as a whole
    def clear(self):
        """Empty the table: a zero fill on the current stream, no synchronisation, capturable.  Entry ids start anew."""
        self._buf.zero_()

    def entries(self) -> int:
        """How many keys the table holds.  Synchronises, as `check_errors()` does."""
        return int(self.ctrl[_lib.KEY_CTRL_ENTRIES])

    def dropped(self) -> int:
        """How many inserted indices were dropped because their key's window was full, since the last `check_errors()` or
        `clear()`.  Synchronises."""
        return int(self.ctrl[_lib.KEY_CTRL_DROPPED])

    def check_errors(self):
        """Synchronises and raises ValueError if an insert dropped keys since the last check; the counter starts anew."""
        n = self.dropped()
        if n:
            self.ctrl[_lib.KEY_CTRL_DROPPED] = 0
            raise ValueError(f"KeyTable: {n} inserted key(s) were dropped: the {min(self.capacity, _lib.KEY_MAX_PROBE)} slots from their "
                             f"home were full (capacity {self.capacity}, {self.entries()} entries); their entry is -1")

    def occupied(self) -> torch.Tensor:
        """int64 [entries]: the entry ids in use, ascending -- the `nonzero` of the key array.  The size of the result depends on
        the data, so this synchronises and cannot be captured."""
        return torch.nonzero(self.keys).squeeze(1)

    def state_dict(self) -> dict:
        """Plain tensors: copies of the five arrays."""
        return {m: getattr(self, m).clone() for m in _MEMBERS}

    def load_state_dict(self, state: dict):
        if set(state) != set(_MEMBERS):
            raise ValueError(f"load_state_dict: expected the members {_MEMBERS}, got {tuple(sorted(state))}")
        for m in _MEMBERS:
            mine, t = getattr(self, m), state[m]
            if not torch.is_tensor(t) or t.dtype is not mine.dtype or tuple(t.shape) != tuple(mine.shape):
                raise ValueError(f"load_state_dict: {m} must be a {str(mine.dtype).split('.')[-1]} tensor of shape {tuple(mine.shape)} "
                                 f"(a table of capacity {self.capacity})")
        for m in _MEMBERS:
            getattr(self, m).copy_(state[m])
