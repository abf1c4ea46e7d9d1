"""What the sm_moe_route and sm_moe_gate tests share: the numpy restatement of the routing definition."""
import numpy as np


def route_ref(ids, top_k, groups):
    """include/sparsifyme.h, sm_moe_route, to the letter -- vectorised: a stable argsort with the dropped pairs behind every expert"""
    ids = np.asarray(ids, dtype=np.int64)
    Pn = len(ids)
    kept = (ids >= 0) & (ids < groups)
    V = int(kept.sum())
    order = np.argsort(np.where(kept, ids, groups), kind="stable")[:V]
    off = np.concatenate([[0], np.cumsum(np.bincount(ids[kept], minlength=groups))]).astype(np.int32)
    st, sp, pp = (np.full(Pn, -1, dtype=np.int32) for _ in range(3))
    sp[:V] = order
    st[:V] = order // top_k
    pp[order] = np.arange(V)
    return off, st, sp, pp
