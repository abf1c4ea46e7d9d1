"""sm_moe_route on the device: the router's expert ids to group_offsets, sorted_token, sorted_pair and pair_pos -- a stable counting sort
whose every output the definition fixes, so every comparison is of integers against the numpy restatement below.  Both forms (asserted
through sm_moe_route_form per case), top_k 1 / 2 / 8, 1 / 8 / 1024 experts, P at and around a chunk boundary of the multi form and at
the single form's limit, one expert taking everything, empty experts first / middle / last, ids outside [0, groups) (dropped: the tail
and pair_pos get -1), every pair dropped.  Every output sits between guard words; the workspace has exactly the reported size, a guard
behind it and garbage inside.  Two runs agree; a graph captured once and replayed under two id arrays equals each eager run."""
import numpy as np
import pytest
import torch
from linear24_testlib import DEV
from moe_route_testlib import route_ref

pytestmark = pytest.mark.gpu

GUARD = 8                  # int32 words before and behind every output
SENT = -77777
SINGLE_MAX, CHUNK = 4096, 4096


class Buffers:
    """the four outputs (and the workspace) inside guarded allocations"""

    def __init__(self, pkg, tokens, top_k, groups):
        self.pkg, self.tokens, self.top_k, self.groups = pkg, tokens, top_k, groups
        Pn = tokens * top_k
        self.sizes = [groups + 1, Pn, Pn, Pn]
        self.bufs = [torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV) for n in self.sizes]
        self.views = [b[GUARD:GUARD + n] for b, n in zip(self.bufs, self.sizes)]
        self.ws_bytes = pkg.moe_route_workspace_size(tokens, top_k, groups)
        assert self.ws_bytes % 4 == 0
        self.wbuf = torch.randint(-2 ** 31, 2 ** 31 - 1, (self.ws_bytes // 4 + GUARD,), dtype=torch.int32, device=DEV)
        self.wguard = self.wbuf[self.ws_bytes // 4:].clone()
        self.ws = self.wbuf[:self.ws_bytes // 4] if self.ws_bytes else None

    def run(self, ids):
        self.pkg.moe_route(ids, self.tokens, self.top_k, self.groups, *self.views, workspace=self.ws)

    def outputs(self):
        torch.cuda.synchronize()
        for b, n in zip(self.bufs, self.sizes):
            assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), "a guard word of an output was written"
        assert torch.equal(self.wbuf[self.ws_bytes // 4:], self.wguard), "the word behind the workspace was written"
        return [v.cpu().numpy().copy() for v in self.views]


def check(pkg, ids, tokens, top_k, groups, form):
    assert pkg.moe_route_form(tokens, top_k, groups) == form
    ids = np.asarray(ids, dtype=np.int32)
    assert len(ids) == tokens * top_k
    b = Buffers(pkg, tokens, top_k, groups)
    assert (b.ws_bytes == 0) == (form != "multi")
    d_ids = torch.from_numpy(ids).to(DEV)
    b.run(d_ids)
    got = b.outputs()
    want = route_ref(ids, top_k, groups)
    for name, g, w in zip(("group_offsets", "sorted_token", "sorted_pair", "pair_pos"), got, want):
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{name}: first mismatch at {bad[0]}: {g[bad[0]]} for {w[bad[0]]}, {bad.size} of {g.size}"
    if b.ws is not None:
        b.wbuf[:b.ws_bytes // 4].copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, (b.ws_bytes // 4,), dtype=torch.int32, device=DEV))   # other garbage
    b.run(d_ids)
    again = b.outputs()
    assert all(np.array_equal(x, y) for x, y in zip(got, again)), "two runs on the same ids differ"
    return got


def router_ids(rng, tokens, top_k, groups):
    """top_k DISTINCT experts per token where the expert count allows it, as a router gives them"""
    if groups >= top_k:
        return np.argsort(rng.random((tokens, groups)), axis=1)[:, :top_k].reshape(-1)
    return rng.integers(0, groups, tokens * top_k)


# (tokens, top_k, groups): the decode case, P at the single form's limit, 1024 experts of which most are empty
SINGLE = [(16, 8, 8), (1, 1, 1), (37, 2, 8), (4096, 1, 8), (512, 8, 1024), (2048, 2, 1), (100, 8, 1024), (63, 1, 8), (65, 3, 5)]
# P one above the single form's limit; at, one below and one above a chunk boundary; top_k 1 / 2 / 8; the largest case, about 2e4 pairs
MULTI = [(4097, 1, 8), (8192, 1, 8), (8191, 1, 1024), (8193, 1, 8), (4096, 2, 1), (1025, 8, 8), (2500, 8, 1024), (10001, 2, 64)]


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: "x".join(map(str, c)))
def test_single_form(gpu, case):
    tokens, top_k, groups = case
    assert tokens * top_k <= SINGLE_MAX
    check(gpu, router_ids(np.random.default_rng(2000 + SINGLE.index(case)), tokens, top_k, groups), tokens, top_k, groups, "single")


@pytest.mark.parametrize("case", MULTI, ids=lambda c: "x".join(map(str, c)))
def test_multi_form(gpu, case):
    tokens, top_k, groups = case
    assert tokens * top_k > SINGLE_MAX
    check(gpu, router_ids(np.random.default_rng(2100 + MULTI.index(case)), tokens, top_k, groups), tokens, top_k, groups, "multi")


@pytest.mark.parametrize("tokens,form", [(300, "single"), (3000, "multi")])
def test_skewed_and_empty_experts(gpu, tokens, form):
    pkg, top_k, groups = gpu, 2, 8
    Pn = tokens * top_k
    rng = np.random.default_rng(2200 + tokens)
    off = check(pkg, np.full(Pn, 5), tokens, top_k, groups, form)[0]                      # everything to one expert
    assert off.tolist() == [0] * 6 + [Pn] * 3
    ids = rng.choice(np.array([1, 2, 4, 6]), Pn)                                          # experts 0 (first), 3, 5 (middle), 7 (last) empty
    off = check(pkg, ids, tokens, top_k, groups, form)[0]
    assert off[1] == 0 and off[4] == off[3] and off[6] == off[5] and off[8] == off[7] == Pn
    ids = rng.permutation(np.concatenate([np.zeros(Pn - 7, dtype=np.int64), np.arange(1, 8)]))   # 90 %+ to expert 0, one pair each elsewhere
    check(pkg, ids, tokens, top_k, groups, form)


@pytest.mark.parametrize("tokens,form", [(150, "single"), (2100, "multi")])
def test_ids_outside_the_groups_are_dropped(gpu, tokens, form):
    pkg, top_k, groups = gpu, 8, 8
    Pn = tokens * top_k
    rng = np.random.default_rng(2300 + tokens)
    ids = rng.integers(-4, groups + 5, Pn)
    ids[::97] = -2 ** 31
    ids[5::101] = 2 ** 31 - 1
    off, st, sp, pp = check(pkg, ids, tokens, top_k, groups, form)
    V = int(off[-1])
    kept = (ids >= 0) & (ids < groups)
    assert 0 < V == int(kept.sum()) < Pn and np.all(sp[V:] == -1) and np.all(st[V:] == -1) and np.all(pp[~kept] == -1) and np.all(pp[kept] >= 0)
    off, st, sp, pp = check(pkg, np.where(rng.random(Pn) < 0.5, -1, groups), tokens, top_k, groups, form)     # every pair dropped
    assert not off.any() and np.all(sp == -1) and np.all(st == -1) and np.all(pp == -1)


def test_no_pairs_still_writes_the_offsets(gpu):
    """tokens == 0 or top_k == 0: the groups + 1 zeros are written, nothing else; groups == 0: nothing at all"""
    pkg = gpu
    for tokens, top_k in ((0, 2), (5, 0)):
        assert pkg.moe_route_form(tokens, top_k, 8) == "empty"
        off = torch.full((9 + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)
        other = torch.full((16,), SENT, dtype=torch.int32, device=DEV)
        pkg.moe_route(other[:0 + 1], tokens, top_k, 8, off[GUARD:GUARD + 9], other, other, other)
        torch.cuda.synchronize()
        assert off[GUARD:GUARD + 9].tolist() == [0] * 9 and bool((off[:GUARD] == SENT).all()) and bool((off[GUARD + 9:] == SENT).all())
        assert bool((other == SENT).all())
    off = torch.full((4,), SENT, dtype=torch.int32, device=DEV)
    ids = torch.zeros(8, dtype=torch.int32, device=DEV)
    pkg.moe_route(ids, 4, 2, 0, off, off, off, off)
    torch.cuda.synchronize()
    assert bool((off == SENT).all())


@pytest.mark.parametrize("tokens,form", [(64, "single"), (1200, "multi")])
def test_hipgraph_replays_follow_the_ids(gpu, tokens, form):
    """Captured once (one stream: a chain of kernel nodes, no parallel branches); the ids then change in device memory only."""
    pkg, top_k, groups = gpu, 8, 16
    assert pkg.moe_route_form(tokens, top_k, groups) == form
    rng = np.random.default_rng(2400 + tokens)
    routings = [router_ids(rng, tokens, top_k, groups).astype(np.int32), rng.integers(-1, groups + 1, tokens * top_k).astype(np.int32)]
    eager = []
    for r in routings:
        b = Buffers(pkg, tokens, top_k, groups)
        b.run(torch.from_numpy(r).to(DEV))
        eager.append(b.outputs())
        assert all(np.array_equal(x, y) for x, y in zip(eager[-1], route_ref(r, top_k, groups)))
    b = Buffers(pkg, tokens, top_k, groups)
    ids = torch.from_numpy(routings[0]).to(DEV)
    b.run(ids)                                       # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        b.run(ids)
    for r, want in list(zip(routings, eager)) + [(routings[0], eager[0])]:
        ids.copy_(torch.from_numpy(r).to(DEV))
        for v in b.views:
            v.fill_(SENT)
        graph.replay()
        got = b.outputs()
        for name, g, w in zip(("group_offsets", "sorted_token", "sorted_pair", "pair_pos"), got, want):
            # rows s >= V of the sorted arrays are written (-1) and dropped pairs' pair_pos too: the whole arrays are compared
            assert np.array_equal(g, w), f"replay: {name} differs from the eager run"
