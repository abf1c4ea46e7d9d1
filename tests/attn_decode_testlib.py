"""What the sm_attn_decode_* tests share: the definition of include/sparsifyme.h in numpy -- ONE function, evaluated in float64 (the
reference) or in float32 (the restatement: chunked, p rounded to the 16-bit type, the chunks combined in ascending order, exp as exp2f of
the argument times log2e) -- the bound the device is held to, the case table, the two exact classes (one-hot and uniform) and the cache
builder of the GPU test (operands at moved bases with pitches above their extents, NaN in all padding, in every slot at or beyond L of a
sequence's last page and in every page no table refers to, a NaN guard page in front of page 0 and behind the last page).  The block
table and the cache's place in its buffers are paged_kv_testlib's.

16-bit values travel as uint16 bit patterns; `ty` is "f16" or "bf16".  The chunk is a parameter everywhere: the tests pass the package's."""
import numpy as np

from guard_testlib import NAN16, Guarded, f32_of, rne16, seed   # noqa: F401  (re-exported)
from paged_kv_testlib import CacheLayout, PageTable

TYPES = ["f16", "bf16"]
MANT = {"f16": 10, "bf16": 7}
EMIN = {"f16": -14, "bf16": -126}
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}        # unit roundoff
LOG2E = np.float32(1.4426950408889634)
SALT = 0xA77D


def bits_of(x, ty):
    return rne16(np.asarray(x, dtype=np.float32), ty)


def ulp16(x, ty):
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** EMIN[ty])))
    return 2.0 ** (np.maximum(e, EMIN[ty]) - MANT[ty])


# ------------------------------------------------------------------------------------------------ the case table
# lens, max_pages: expressions in C (the chunk) and P (the page size).  absent: (sequence, table column, id) with id "lo" (-1) or "hi"
# (num_pages) planted inside the live range.  shared: the first `shared` table columns of sequence 1 are sequence 0's (prefix pages).
# raw: seq_lens as given to the call where they differ from the clamped lengths ("cap" = max_pages * P).
def case(ty, hd, group, kvh, ps, lens, max_pages, absent=(), shared=0, raw=None):
    return dict(ty=ty, hd=hd, group=group, kvh=kvh, ps=ps, lens=lens, max_pages=max_pages, absent=tuple(absent), shared=shared, raw=raw)


CASES = [
    case("bf16", 128, 4, 2, 16, ["1"], "4"),                                                # DIRECT: one token, one sequence
    case("f16", 64, 1, 1, 16, ["15", "16", "17"], "C//P"),                                  # DIRECT at max_pages * P == C; a tile's edge
    case("bf16", 128, 2, 3, 32, ["P-1", "P+1", "0", "C-1", "C"], "C//P", absent=[(3, 1, "lo"), (4, 0, "hi")]),   # DIRECT, 5 sequences, L = 0
    case("f16", 128, 5, 2, 16, ["C+1", "17", "2*C+3"], "(2*C+3)//P+2", absent=[(0, 3, "hi"), (2, "C//P", "lo")]),  # SPLIT, odd group
    case("bf16", 128, 8, 1, 128, ["5*C", "P+1", "C", "0", "C-1"], "5*C//P", absent=[(0, 1, "lo")]),   # SPLIT, 5 chunks, page = half a chunk
    case("f16", 128, 16, 1, 32, ["C+1"], "C//P+1"),                                         # the 16-row group class, SPLIT
    case("bf16", 64, 8, 2, 16, ["2*C+3", "P-1", "1"], "2*C//P+1"),                          # head_dim 64, the 16-row class
    case("bf16", 128, 16, 2, 16, ["16", "C"], "C//P", absent=[(1, 2, "lo"), (1, 5, "hi")]),  # the 16-row class, DIRECT, a full chunk
    case("f16", 64, 4, 3, 128, ["P-1", "C+1", "P+1"], "C//P+1"),                            # head_dim 64, page 128
    case("bf16", 128, 4, 1, 16, ["cap", "0", "17"], "C//P+2", raw=["cap+5", "-3", "17"]),   # seq_lens above the capacity and negative: clamped
    case("bf16", 128, 4, 2, 16, ["C+1", "C+17"], "C//P+2", shared=5),                       # two sequences share five prefix pages
    case("f16", 64, 2, 1, 32, ["5*C"], "5*C//P"),                                           # one long sequence, head_dim 64
    case("f16", 128, 1, 2, 16, ["C-1", "C+1", "1"], "C//P+1", absent=[(0, 0, "lo"), (1, "C//P", "hi")]),    # group 1; the second chunk's only page absent
    case("bf16", 64, 1, 3, 32, ["P+1"], "2", absent=[(0, 0, "hi"), (0, 1, "lo")]),          # every page absent: +0 and -inf
]


def case_id(c):
    return f"{c['ty']}-d{c['hd']}-g{c['group']}-kv{c['kvh']}-p{c['ps']}-" + "_".join(c["lens"]).replace("*", "x").replace("//", "d")


class Problem:
    """A case made concrete at a chunk size: lengths, the block table (paged_kv_testlib.PageTable), the set of live (page, slot) pairs."""

    def __init__(self, c, chunk, rng):
        self.c, self.chunk, self.ty = c, chunk, c["ty"]
        self.hd, self.group, self.kvh, self.ps = c["hd"], c["group"], c["kvh"], c["ps"]
        self.q_heads = self.group * self.kvh
        env = {"C": chunk, "P": self.ps}
        self.max_pages = int(eval(c["max_pages"], env))
        env["cap"] = self.cap = self.max_pages * self.ps
        self.lens = [int(eval(x, env)) for x in c["lens"]]
        self.raw_lens = [int(eval(x, env)) for x in (c["raw"] or c["lens"])]
        self.seqs = len(self.lens)
        pt = PageTable(self.lens, self.ps, self.max_pages, rng, [(s, int(eval(str(col), env)), which) for s, col, which in c["absent"]], c["shared"])
        self.table, self.num_pages = pt.table, pt.num_pages

    def tokens(self, s):
        """(t, page, slot) of the present tokens of sequence s, ascending t"""
        t = np.arange(self.lens[s])
        page = self.table[s, t // self.ps] if t.size else np.zeros(0, dtype=np.int32)
        ok = (page >= 0) & (page < self.num_pages)
        return t[ok], page[ok], (t % self.ps)[ok]

    def live(self):
        """[num_pages][page_size] bool: a sequence reads this slot"""
        m = np.zeros((self.num_pages, self.ps), dtype=bool)
        for s in range(self.seqs):
            _, page, slot = self.tokens(s)
            m[page, slot] = True
        return m


# ------------------------------------------------------------------------------------------------ the definition
def evaluate(pr, Q, K, V, scale, dtype, ty=None):
    """The definition on Q [seqs][q_heads][hd], K / V [num_pages][page_size][kv_heads][hd] (bit patterns), every operation in `dtype`:
    float32 -- the restatement, exp as exp2f(x * log2e) -- or float64 -- the reference, exp as exp.  Returns O [seqs][q_heads][hd] (in
    dtype, NOT rounded to the output type), lse, and for the bound A = sum p |v| / sum p, sabs = scale * max_t sum_d |q k|, T."""
    ty = ty or pr.ty
    f = np.dtype(dtype).type
    ex = (lambda x: np.exp2((x * LOG2E).astype(np.float32))) if dtype == np.float32 else np.exp
    O = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=dtype)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=dtype)
    A, sabs, T = np.zeros_like(O, dtype=np.float64), np.zeros((pr.seqs, pr.q_heads)), np.zeros(pr.seqs, dtype=np.int64)
    q_all, scale = f32_of(Q, ty).astype(dtype), f(scale)
    with np.errstate(all="ignore"):
        for s in range(pr.seqs):
            t, page, slot = pr.tokens(s)
            T[s] = t.size
            if t.size == 0:
                continue
            k = f32_of(K[page, slot], ty).astype(dtype)          # [T][kvh][hd]
            v = f32_of(V[page, slot], ty).astype(dtype)
            chunk_of = t // pr.chunk
            for h in range(pr.q_heads):
                kv = h // pr.group
                q = q_all[s, h]
                sc = (scale * (k[:, kv] * q[None, :]).sum(axis=1, dtype=dtype)).astype(dtype)
                sabs[s, h] = float(scale) * np.abs(k[:, kv].astype(np.float64) * q[None, :].astype(np.float64)).sum(axis=1).max()
                parts = []
                for cidx in range(-(-pr.lens[s] // pr.chunk)):       # every chunk the sequence has, ascending
                    sel = chunk_of == cidx
                    if not sel.any():
                        parts.append((f(-np.inf), f(0), np.zeros(pr.hd, dtype=dtype), np.zeros(pr.hd)))
                        continue
                    m_c = sc[sel].max()
                    p = f32_of(rne16(ex((sc[sel] - m_c).astype(dtype)).astype(np.float32), ty), ty).astype(dtype)
                    parts.append((m_c, p.sum(dtype=dtype), (p[:, None] * v[sel, kv]).sum(axis=0, dtype=dtype),
                                  (p[:, None].astype(np.float64) * np.abs(v[sel, kv]).astype(np.float64)).sum(axis=0)))
                m = max(pt[0] for pt in parts)
                l, acc, aabs = f(0), np.zeros(pr.hd, dtype=dtype), np.zeros(pr.hd)
                for m_c, l_c, acc_c, abs_c in parts:
                    w = ex(np.asarray(m_c - m, dtype=dtype)).astype(dtype)
                    l = f(l + f(w * l_c))
                    acc = (acc + (w * acc_c).astype(dtype)).astype(dtype)
                    aabs = aabs + float(w) * abs_c
                O[s, h] = (acc / l).astype(dtype)
                lse[s, h] = f(m + np.log(l).astype(dtype))
                A[s, h] = aabs / float(l)
    return O, lse, A, sabs, T


def restate32(pr, Q, K, V, scale):
    """the fp32 restatement: (O bits, lse float32)"""
    O, lse, _, _, _ = evaluate(pr, Q, K, V, scale, np.float32)
    return rne16(O, pr.ty), lse


def bound(pr, ref, got, A, sabs, T, scale):
    """Per element: half an ulp of the output type at max(|ref|, |O|) -- the one rounding -- plus (2 u + 2 delta + (T + head_dim + 16) 2^-24) A:
    u, the unit roundoff of the 16-bit type, for a p_t that rounds to the other neighbour on the device (one such p moves the numerator and the
    denominator by at most u p each); delta = (head_dim + 2) 2^-24 scale max_t sum_d |q_d k_t,d| for the scores (head_dim products and sums, the
    multiply by scale, the subtraction of m), which move every p by a factor e^(+-delta) in the numerator and in the denominator; T 2^-24 for
    the two fp32 sums over the tokens in any order, head_dim + 16 for exp2f, the combine and the division.  A = sum_t p_t |v_t,d| / sum_t p_t.
    An allowance derived from the definition, not a measurement."""
    delta = (pr.hd + 2) * 2.0 ** -24 * sabs
    return 0.5 * ulp16(np.maximum(np.abs(ref), np.abs(got)), pr.ty) + (2 * UNIT[pr.ty] + 2 * delta[..., None] + (T[:, None, None] + pr.hd + 16) * 2.0 ** -24) * A


def lse_bound(pr, ref_lse, sabs):
    return (pr.hd + 2) * 2.0 ** -24 * sabs + 8 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref_lse))


def worst_ratios(pr, got_bits, got_lse, Q, K, V, scale):
    """(worst |O - ref| / bound, worst |lse - ref| / bound) against the fp64 definition; -inf must sit exactly where the reference has it"""
    ref, rl, A, sabs, T = evaluate(pr, Q, K, V, scale, np.float64)
    got = f32_of(got_bits, pr.ty).astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), "a non-finite output on finite live data: a masked slot or an absent page was read"
    ro = float((np.abs(got - ref) / bound(pr, ref, got, A, sabs, T, scale)).max())
    gl = np.asarray(got_lse, dtype=np.float64)
    assert np.array_equal(np.isneginf(gl), np.isneginf(rl)) and not np.isnan(gl).any()
    fin = np.isfinite(rl)
    with np.errstate(invalid="ignore"):
        rlr = float((np.abs(gl - rl)[fin] / lse_bound(pr, rl, sabs)[fin]).max()) if fin.any() else 0.0
    return ro, rlr


# ------------------------------------------------------------------------------------------------ data
def general(pr, rng, sigma):
    Q = bits_of(rng.normal(0.0, 1.0, (pr.seqs, pr.q_heads, pr.hd)), pr.ty)
    K = bits_of(rng.normal(0.0, 1.0, (pr.num_pages, pr.ps, pr.kvh, pr.hd)), pr.ty)
    V = bits_of(rng.normal(0.0, sigma, (pr.num_pages, pr.ps, pr.kvh, pr.hd)), pr.ty)
    return Q, K, V


def v_codes(pr):
    """V whose bits encode (page, slot, kv head, dim): finite, normal, never -0"""
    p, s, k, d = np.meshgrid(np.arange(pr.num_pages), np.arange(pr.ps), np.arange(pr.kvh), np.arange(pr.hd), indexing="ij")
    hsh = p * 7919 + s * 131 + k * 37 + d * 3
    return (0x0400 + hsh % 0x3000 + ((hsh // 5) % 2) * 0x8000).astype(np.uint16)


def one_hot(pr, rng):
    """scale = 1; q of (s, h) has 8 entries of 4 on a support of its own inside its group (and across the sequences that share pages), K is zero
    except K[target] += q.  Returns Q, K, V, the targets [seqs][q_heads] as (page, slot) or None where the sequence has no present token, and
    the expected O bits and lse.  The premise -- the target scores 128 and every other present token 0, exactly -- is asserted."""
    sup = pr.hd // 8
    assert pr.group * (2 if pr.c["shared"] else 1) <= sup
    Q = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.float32)
    K = np.zeros((pr.num_pages, pr.ps, pr.kvh, pr.hd), dtype=np.float32)
    V = v_codes(pr)
    want = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=np.float32)
    targets = {}
    for s in range(pr.seqs):
        t, page, slot = pr.tokens(s)
        if t.size == 0:
            continue
        L, C, P = pr.lens[s], pr.chunk, pr.ps
        # the first and the last token, the last slot of a page and the first of the next, the last token of a chunk and the first of the next
        wanted = [0, L - 1, P - 1, P, C - 1, C, 2 * C - 1, 2 * C, L // 2, L - 2, 1]
        choice = [x for x in wanted if x in set(t.tolist())] or [int(t[0])]
        for h in range(pr.q_heads):
            g, kv = h % pr.group, h // pr.group
            u = (g + (s * pr.group if pr.c["shared"] else 0)) % sup
            Q[s, h, 8 * u:8 * u + 8] = 4.0
            tt = choice[(h + s) % len(choice)]
            i = int(np.flatnonzero(t == tt)[0])
            K[page[i], slot[i], kv] += Q[s, h]
            targets[(s, h)] = (int(page[i]), int(slot[i]), tt)
            want[s, h] = V[page[i], slot[i], kv]
            lse[s, h] = 128.0
    Qb, Kb = bits_of(Q, pr.ty), bits_of(K, pr.ty)
    for s in range(pr.seqs):                                   # the premise, in exact integer arithmetic
        t, page, slot = pr.tokens(s)
        for h in range(pr.q_heads if t.size else 0):
            sc = (f32_of(Kb[page, slot, h // pr.group], pr.ty).astype(np.float64) * f32_of(Qb[s, h], pr.ty).astype(np.float64)[None, :]).sum(axis=1)
            hot = np.flatnonzero(t == targets[(s, h)][2])
            assert sc[hot[0]] == 128.0 and np.count_nonzero(sc) == 1, "the one-hot premise"
    assert np.exp2(np.float32(-128.0) * LOG2E) == 0.0
    return Qb, Kb, V, targets, want, lse


def uniform(pr, rng):
    """Q = 0, so every p = 1 and every w = 1; V integers with |v| <= 7 and 7 L < 2^24: every partial sum is an exact integer in any order.
    Returns Q, K, V and the expected O bits = rne16(fp32(sum v) / fp32(T)) and lse = log(T)."""
    Q = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    K = bits_of(rng.normal(0.0, 1.0, (pr.num_pages, pr.ps, pr.kvh, pr.hd)), pr.ty)
    Vi = rng.integers(-7, 8, (pr.num_pages, pr.ps, pr.kvh, pr.hd))
    assert 7 * max(pr.lens + [1]) < 2 ** 24 and np.abs(Vi).max() <= 7
    want = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=np.float64)
    for s in range(pr.seqs):
        t, page, slot = pr.tokens(s)
        if t.size == 0:
            continue
        tot = Vi[page, slot].sum(axis=0).astype(np.float32)                     # [kvh][hd]
        o = rne16((tot / np.float32(t.size)).astype(np.float32), pr.ty)
        want[s] = np.repeat(o, pr.group, axis=0)
        lse[s] = np.log(float(t.size))
    return Q, K, bits_of(Vi, pr.ty), want, lse


# ------------------------------------------------------------------------------------------------ the layout builder (GPU test)
SENT16, SENT32 = 0x2BCD, 0xC640E400        # (-12345.0f as bits)


class Layout:
    """The call's operands on the device.  Inputs are NaN outside their live elements; outputs and their padding hold a sentinel."""

    def __init__(self, pr, Q, K, V, torch):
        import guard_testlib as gl
        self.pr, self.torch = pr, torch
        qh, hd, ty = pr.q_heads, pr.hd, pr.ty
        self.dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
        self.ldq, self.ldo, self.qbase, self.obase = qh * hd + 24, qh * hd + 8, 8, 16
        self.cache = cl = CacheLayout(pr.num_pages, pr.ps, pr.kvh * hd, pr.seqs, pr.max_pages)
        ar = np.arange
        iq = (self.qbase + ar(pr.seqs)[:, None] * self.ldq + ar(qh * hd)[None, :]).reshape(-1)
        self.Q = Guarded(self.qbase + pr.seqs * self.ldq + 16, NAN16[ty], np.uint16, self.qbase, idx=iq)
        self.Q.host[iq] = Q.reshape(-1)
        live = pr.live()
        self.K, self.V = (cl.cache_buffer(NAN16[ty], live) for _ in range(2))
        self.K.host[self.K.idx] = K.reshape(pr.num_pages, pr.ps, -1)[live].reshape(-1)
        self.V.host[self.V.idx] = V.reshape(pr.num_pages, pr.ps, -1)[live].reshape(-1)
        self.T = cl.table_buffer(pr.table)
        self.Ls = Guarded.around(np.array(pr.raw_lens, dtype=np.int32), 0x7FFFFFF0, 3, 5)
        self.io = (self.obase + ar(pr.seqs)[:, None] * self.ldo + ar(qh * hd)[None, :]).reshape(-1)
        self.O = Guarded(self.obase + pr.seqs * self.ldo + 16, SENT16, np.uint16, self.obase, idx=self.io)
        self.lse = Guarded(pr.seqs * qh + 13, SENT32, np.uint32, 6, size=pr.seqs * qh)
        for g in (self.Q, self.K, self.V, self.T, self.Ls, self.O, self.lse):
            g.to_device()
        self.gl = gl

    def tensors(self):
        pr, tv = self.pr, lambda g, dt: g.dev.view(dt)
        q = tv(self.Q, self.dt).as_strided((pr.seqs, pr.q_heads, pr.hd), (self.ldq, pr.hd, 1), self.qbase)
        o = tv(self.O, self.dt).as_strided((pr.seqs, pr.q_heads, pr.hd), (self.ldo, pr.hd, 1), self.obase)
        kv = [self.cache.cache_view(tv(g, self.dt), pr.kvh, pr.hd) for g in (self.K, self.V)]
        bt = self.cache.table_view(self.T.dev)
        sl = self.Ls.dev[3:3 + pr.seqs]
        lse = self.lse.dev.view(self.torch.float32)[6:6 + pr.seqs * pr.q_heads].view(pr.seqs, pr.q_heads)
        return q, kv[0], kv[1], bt, sl, o, lse

    def run(self, pkg, scale, form):
        """the call with a workspace of exactly the reported size between guards; asserts the form, that no input changed and that nothing
        outside the outputs was written; returns (O bits [seqs][q_heads][hd], lse float32 [seqs][q_heads])"""
        pr = self.pr
        assert pkg.attn_decode_form(pr.seqs, pr.q_heads, pr.kvh, pr.hd, pr.ps, pr.max_pages) == form
        need = pkg.attn_decode_workspace_size(pr.seqs, pr.q_heads, pr.hd, pr.ps, pr.max_pages)
        assert (need > 0) == (form == "split")
        ws = self.gl.Workspace(need, off=16) if need else None
        q, k, v, bt, sl, o, lse = self.tensors()
        self.O.dev.copy_(self.torch.from_numpy(self.O.host.view(np.int16)))
        self.lse.dev.copy_(self.torch.from_numpy(self.lse.host.view(np.int32)))
        pkg.attn_decode(q, k, v, bt, sl, scale=scale, out=o, lse=lse, workspace=ws.p[:need] if ws else None)
        self.torch.cuda.synchronize()
        for g, name in ((self.Q, "Q"), (self.K, "Kc"), (self.V, "Vc"), (self.T, "block_table"), (self.Ls, "seq_lens")):
            assert g.unchanged(), f"{name} was written"
        if ws:
            ws.check("attn_decode workspace")
        said = lambda what: (lambda n, first: f"{n} elements outside {what} were written, first at {first.tolist()}")
        ob = self.O.result(said("O")).reshape(pr.seqs, pr.q_heads, pr.hd)
        lb = self.lse.result(said("lse")).view(np.float32).reshape(pr.seqs, pr.q_heads)
        return ob.copy(), lb.copy()

    def twice(self, pkg, scale, form):
        a, b = self.run(pkg, scale, form), self.run(pkg, scale, form)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "two runs on the same operands differ"
        return a


def form_of(pr):
    return "direct" if pr.cap <= pr.chunk else "split"
