"""The queries that read chosen rows of a state set (include/mgx.h: MgxEnvRows) -- state_key, action_mask, distance_field,
agent_distance -- written once, over a `RowSet`: a live batch (`BatchedMultiGridEnv._row_set`) or a snapshot
(`EnvSnapshot._row_set`).  The two sources differ in what they ask before a launch and say so there; from the row set on, a query is
the same launch through the same backend.  The public methods, their signatures and docstrings are in batched.py.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _lib


class RowSet(NamedTuple):
    what: str            # the public method's name, for messages
    env: object          # who launches: the env whose backend, index checks and `bad` words are used
    tensors: dict        # member -> tensor (missing: the set has no such member)
    rows: int            # the rows the set holds
    device: object
    index_name: str      # the index parameter's name, for messages: "env_ids" or "rows"

    def count(self, idx) -> int:
        """how many rows `idx` names (None: every row, in order)"""
        return self.rows if idx is None else int(self.env._index_arg(self.what, self.index_name, idx).shape[0])

    def members(self, *names) -> dict:
        return {m: self.tensors.get(m) for m in names}


def _key_args(what: str, salt, step_count, rng) -> tuple:
    """(flags, salt) of mgx_state_key / mgx_obs_key"""
    if isinstance(salt, bool) or not isinstance(salt, int) or not 0 <= salt < 2 ** 64:
        raise ValueError(f"{what}: salt must be an int in [0, 2**64)")
    return (_lib.KEY_STEP_COUNT if step_count else 0) | (_lib.KEY_RNG if rng else 0), salt


def _out(what: str, out, shape: tuple, dtype, fill, device) -> torch.Tensor:
    """the caller's out= tensor, checked, or a new one holding `fill` (what a row with a bad index keeps)"""
    shape = tuple(shape)
    if out is None:
        return torch.full(shape, fill, dtype=dtype, device=device)
    if not torch.is_tensor(out) or out.dtype is not dtype or tuple(out.shape) != shape or out.device != device or not out.is_contiguous():
        raise ValueError(f"{what}: out= must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {shape} on {device}")
    return out


_DIST_THROUGH = {"closed": _lib.DIST_THROUGH_CLOSED, "locked": _lib.DIST_THROUGH_LOCKED, "objects": _lib.DIST_THROUGH_OBJECTS}


def _dist_bits(what: str, name: str, values, below: int, why: str) -> int:
    """the bit mask of an iterable of small ints (enum members included)"""
    if isinstance(values, (str, bytes)) or torch.is_tensor(values):
        raise ValueError(f"{what}: {name} must be an iterable of ints")
    mask = 0
    try:
        items = list(values)
    except TypeError:
        raise ValueError(f"{what}: {name} must be an iterable of ints") from None
    for v in items:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < below:
            raise ValueError(f"{what}: {name} holds {v!r}: {why}")
        mask |= 1 << int(v)
    return mask


def _dist_query(what: str, spec, n: int, device, types=None, colors=None, agents=None, points=None, through=(), avoid_lava=False) -> dict:
    """The query of mgx_distance (include/mgx.h "DISTANCE FIELDS": MgxDistance) from the keyword arguments of distance_field() /
    agent_distance(): {type_mask, colour_mask, agent_mask, flags, points}."""
    A = spec.num_agents
    type_mask = 0 if types is None else _dist_bits(what, "types", types, 16, "a Type or an int in [0, 16)")
    colour_mask = 0xFF if colors is None else _dist_bits(what, "colors", colors, 8, "a Color or an int in [0, 8)")
    agent_mask = 0 if agents is None else _dist_bits(what, "agents", agents, A, f"an agent index must lie in [0, {A})")
    if colors is not None and types is None:
        raise ValueError(f"{what}: colors= narrows the cells that types= selects: pass types= with it")
    if isinstance(through, str):
        through = (through,)
    flags = _lib.DIST_AVOID_LAVA if avoid_lava else 0
    for w in through:
        if w not in _DIST_THROUGH:
            raise ValueError(f"{what}: through= holds {w!r}: it must be a subset of {sorted(_DIST_THROUGH)}")
        flags |= _DIST_THROUGH[w]
    if points is not None:
        if not torch.is_tensor(points) or points.dtype is not torch.int16 or points.dim() != 3 or int(points.shape[0]) != n \
                or int(points.shape[2]) != 2 or points.device != device or not points.is_contiguous():
            raise ValueError(f"{what}: points must be a contiguous int16 tensor of shape ({n}, P, 2) on {device}: (x, y) per output row")
        if int(points.shape[1]) == 0:
            points = None
    if not type_mask and not agent_mask and points is None:
        raise ValueError(f"{what}: the query names no source: pass types=, agents= or points=")
    return {"type_mask": type_mask, "colour_mask": colour_mask, "agent_mask": agent_mask, "flags": flags, "points": points}


def state_key(rs: RowSet, idx, salt, step_count, rng, out) -> torch.Tensor:
    n = rs.count(idx)
    flags, salt = _key_args(rs.what, salt, step_count, rng)
    keys = _out(rs.what, out, (n,), torch.int64, 0, rs.device)
    rs.env.backend.state_key(n, rs.members("cells", "agents", "rng", "step_count", "aux"), rs.rows, idx, flags, salt, keys,
                             rs.env._bad_words())
    return keys


def action_mask(rs: RowSet, idx, expand, out) -> torch.Tensor:
    n, A = rs.count(idx), rs.env.spec.num_agents
    shape, dtype = ((n, A, 7), torch.bool) if expand else ((n, A), torch.uint8)
    mask = _out(rs.what, out, shape, dtype, 0, rs.device)
    rs.env.backend.action_mask(n, rs.members("cells", "agents", "aux"), rs.rows, idx, _lib.MASK_EXPAND if expand else 0, mask,
                               rs.env._bad_words())
    return mask


def distance(rs: RowSet, idx, query: dict, out, field: bool) -> torch.Tensor:
    """distance_field (field) / agent_distance: `query` = their keyword arguments"""
    n, spec = rs.count(idx), rs.env.spec
    q = _dist_query(rs.what, spec, n, rs.device, **query)
    res = _out(rs.what, out, (n, spec.height, spec.width) if field else (n, spec.num_agents), torch.int16, -1, rs.device)
    rs.env.backend.distance(n, rs.members("cells", "agents"), rs.rows, idx, q, res if field else None, None if field else res,
                            rs.env._bad_words())
    return res
