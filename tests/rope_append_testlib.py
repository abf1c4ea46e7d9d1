"""What the sm_rope_append_* tests share: the definition of include/sparsifyme.h in numpy -- ONE function (evaluate), run in float32 (the
restatement: every rounding of the definition, the bit-exact target of the device) or in float64 (the reference) --, the bound the
restatement is held to, the case table, the data classes (general, special values, the contraction witnesses) and the layout builder of
the GPU test: Q, K and V are column slices of one [tokens][(q_heads + 2 kv_heads) head_dim + pad] buffer at a moved base, every input
pitch is above its extent, the type's NaN fills all input padding and the rows of padding tokens, and Qo, Ko and the WHOLE cache hold a
sentinel -- unaddressed slots, unreferenced pages and a guard page in front of page 0 and behind the last page included -- so that an
unclamped kernel writes where the check sees it instead of faulting.

16-bit values travel as uint16 bit patterns; `ty` is "f16" or "bf16".  The page tables and the cache's place in its buffers are
paged_kv_testlib's."""
from fractions import Fraction

import numpy as np

import attn_decode_testlib as al
from guard_testlib import NAN16, SIGNED, Guarded, f32_of, is_nan16, rne16, seed   # noqa: F401  (re-exported)
from paged_kv_testlib import BAD32, CacheLayout, PageTable

TYPES = al.TYPES
SALT = 0x209E
SENT16 = al.SENT16
NEOX, INTERLEAVED = "neox", "interleaved"
FILL32 = BAD32                           # around the int32 operands: a position / id that addresses nothing near


def canon16(bits, ty):
    """16-bit patterns with every NaN turned into the type's quiet NaN: NaN is compared as NaN (by class), everything else -- the two
    zeros included -- bit for bit."""
    bits = np.asarray(bits, dtype=np.uint16)
    return np.where(is_nan16(bits, ty), np.uint16(NAN16[ty]), bits)


def table64(max_pos, rot, base=10000.0):
    """[max_pos][rot] float64: cos(p theta_j), j < rot / 2, then sin(p theta_j); theta_j = base^(-2 j / rot)"""
    half = rot // 2
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * (np.float64(base) ** (-2.0 * np.arange(half, dtype=np.float64) / max(rot, 1)))[None, :]
    return np.concatenate([np.cos(ang), np.sin(ang)], axis=1)


# ------------------------------------------------------------------------------------------------ the case table
# toks: the tokens as (sequence, position) pairs -- or, in the decode spellings, nothing: token i is sequence i at lens[i] - 1.
# lens: per sequence, how many slots the page-table builder gives it pages for (expressions in P, the page size); a token at or beyond
#   them meets a table column that holds -1 or num_pages.  absent: (sequence, column, "lo" | "hi") planted inside the live columns.
# spelling: "prefill" (positions and token_seq given), "decode" (both NULL: seq_lens[i] - 1), "decode_pos" (token_seq NULL, positions given),
#   "seq_only" (token_seq given, positions NULL: seq_lens[token_seq[i]] - 1; the positions of toks are not used).
# alias: "inplace" (Qo == Q, Ko == K), "out" (distinct buffers and pitches), "ko_null", "nocache" (Kc == Vc == NULL, Ko given).
def case(name, ty, qh, kvh, hd, rot, style, toks=None, lens=("1",), ps=16, max_pages="4", max_pos="4*P", spelling="prefill", alias="out", absent=(),
         data="general"):
    return dict(name=name, ty=ty, qh=qh, kvh=kvh, hd=hd, rot=rot, style=style, toks=toks, lens=list(lens), ps=ps, max_pages=max_pages, max_pos=max_pos,
                spelling=spelling, alias=alias, absent=tuple(absent), data=data)


def _shapes():
    out = []
    # head counts x head_dim x rot_dim x style x type: every head_dim meets rot 0, 16, head_dim / 2 (32 for 40) and head_dim (32 / 96 for 40 / 96)
    heads = [(1, 1), (5, 5), (8, 2), (32, 8), (3, 1)]
    rots = {64: (0, 16, 32, 64), 128: (0, 16, 64, 128), 256: (0, 16, 128, 256), 40: (0, 16, 32), 96: (0, 16, 48, 96)}
    n = 0
    for hd, rr in rots.items():
        for rot in rr:
            for style in (NEOX, INTERLEAVED):
                qh, kvh = heads[n % len(heads)]
                ty = TYPES[(n // 2) % 2]
                alias = ("inplace", "out")[n % 2]
                toks = [(0, 0), (1, 3), (0, 1), (1, 0), (0, 17)][: 1 + n % 5]
                out.append(case(f"shape{n}", ty, qh, kvh, hd, rot, style, toks=toks, lens=("P+2", "4"), alias=alias))
                n += 1
    return out


CASES = _shapes() + [
    # token counts: 1; 3, 4 and 5 (a partial, a full and a second WAVE workgroup -- at the shipped threshold these run BLOCK; the WAVE twins
    # are built by wave_twin() at BLOCK_MAX + 1 .. + 5 tokens)
    case("one-token", "bf16", 32, 8, 128, 128, NEOX, toks=[(0, 5)], lens=("6",)),
    case("three-tokens", "f16", 1, 1, 64, 64, NEOX, toks=[(0, 0), (0, 1), (0, 2)], lens=("3",)),
    case("four-tokens", "bf16", 1, 1, 64, 64, INTERLEAVED, toks=[(0, 0), (0, 1), (0, 2), (0, 3)], lens=("4",)),
    case("five-tokens", "f16", 1, 1, 64, 32, NEOX, toks=[(0, 0), (0, 1), (0, 2), (0, 3), (0, 4)], lens=("5",)),
    # positions: 0, page_size - 1, page_size, max_pos - 1
    case("positions", "bf16", 8, 2, 128, 128, NEOX, toks=[(0, 0), (0, "P-1"), (0, "P"), (0, "4*P-1")], lens=("4*P",), max_pages="4", max_pos="4*P"),
    case("positions-p32", "f16", 3, 1, 96, 48, INTERLEAVED, toks=[(0, 0), (0, "P-1"), (0, "P"), (0, "3*P-1")], lens=("3*P",), ps=32, max_pages="3", max_pos="3*P"),
    # a prefill of one sequence across two page boundaries, tokens shuffled; several sequences interleaved
    case("prefill-shuffled", "bf16", 8, 2, 128, 64, NEOX, toks="shuffled:2*P+3", lens=("2*P+3",)),
    case("prefill-interleaved", "f16", 5, 5, 64, 64, INTERLEAVED, toks="interleaved", lens=("P+1", "3", "2*P")),
    case("prefill-p128", "bf16", 3, 1, 40, 32, NEOX, toks="shuffled:P+2", lens=("P+2",), ps=128, max_pages="2", max_pos="2*P", alias="inplace"),
    # padding: pos -1 and max_pos; token_seq -1 and seqs (positions NULL); seq_lens 0 with positions NULL
    case("padding-pos", "bf16", 8, 2, 128, 128, NEOX, toks=[(0, 0), (0, -1), (1, "4*P"), (1, 1), (0, -7), (1, "4*P+9")], lens=("2", "2")),
    case("padding-seq", "f16", 3, 1, 64, 32, INTERLEAVED, toks=[(0, None), (-1, None), (2, None), (1, None), (-5, None), (7, None)], lens=("2", "0"),
         spelling="seq_only"),
    case("padding-rot0", "bf16", 5, 5, 64, 0, NEOX, toks=[(0, 0), (0, -1), (1, 1), (1, "9*P")], lens=("2", "2")),   # rot_dim 0: only pos < 0 pads
    # append refused, Q still written: pos >= max_pages * page_size with max_pos larger; page id -1 and num_pages in the live columns;
    # a sequence id out of range with a position given
    case("no-append-capacity", "bf16", 8, 2, 128, 128, NEOX, toks=[(0, 1), (0, "2*P"), (0, "2*P+5"), (0, "P")], lens=("2*P",), max_pages="2", max_pos="4*P"),
    case("no-append-absent", "f16", 8, 2, 64, 64, NEOX, toks=[(0, 0), (0, "P"), (0, "2*P+1"), (1, 1), (1, "P+1")], lens=("3*P", "2*P"),
         absent=[(0, 1, "lo"), (1, 1, "hi")]),
    case("no-append-seq", "bf16", 3, 1, 96, 96, INTERLEAVED, toks=[(0, 1), (-1, 2), (2, 3), (1, 0)], lens=("2", "1")),
    # the decode spellings
    case("decode", "bf16", 32, 8, 128, 128, NEOX, lens=("1", "P", "P+1", "0", "2*P+5"), spelling="decode", alias="inplace"),
    case("decode-positions", "f16", 8, 2, 64, 64, INTERLEAVED, lens=("3", "P+1", "2"), spelling="decode_pos"),
    # aliasing
    case("alias-inplace", "f16", 8, 2, 128, 64, NEOX, toks="interleaved", lens=("P+1", "3"), alias="inplace"),
    case("alias-inplace-i", "bf16", 5, 5, 40, 32, INTERLEAVED, toks="interleaved", lens=("P+1", "3"), alias="inplace"),
    case("alias-out", "bf16", 8, 2, 128, 128, INTERLEAVED, toks="interleaved", lens=("P+1", "3"), alias="out"),
    case("alias-ko-null", "f16", 8, 2, 128, 128, NEOX, toks="interleaved", lens=("P+1", "3"), alias="ko_null"),
    case("alias-nocache", "bf16", 8, 2, 128, 64, NEOX, toks="interleaved", lens=("P+1", "3"), alias="nocache"),
    # special values and the contraction witnesses
    case("special-bf16", "bf16", 8, 2, 128, 128, NEOX, toks="interleaved", lens=("P+1", "3"), data="special"),
    case("special-f16", "f16", 8, 2, 64, 64, INTERLEAVED, toks="interleaved", lens=("P+1", "3"), data="special"),
    case("special-bf16-i", "bf16", 3, 1, 96, 48, INTERLEAVED, toks="interleaved", lens=("P+1", "3"), data="special", alias="inplace"),
    case("witness-bf16", "bf16", 8, 2, 128, 128, NEOX, toks="interleaved", lens=("P+1", "3"), data="witness"),
    case("witness-f16", "f16", 8, 2, 64, 64, INTERLEAVED, toks="interleaved", lens=("P+1", "3"), data="witness"),
]


def case_id(c):
    return f"{c['name']}-{c['ty']}-q{c['qh']}-kv{c['kvh']}-d{c['hd']}-r{c['rot']}-{c['style']}-{c['alias']}"


def wave_twin(block_max, extra):
    """block_max + extra tokens of one sequence, one Q and one KV head of 64: the smallest case past the BLOCK / WAVE threshold"""
    n = block_max + extra
    return case(f"wave+{extra}", ("bf16", "f16")[extra % 2], 1, 1, 64, (64, 32)[extra % 2], (NEOX, INTERLEAVED)[(extra // 2) % 2], toks=f"shuffled:{n}", lens=(str(n),),
                ps=128, max_pages=str(-(-n // 128)), max_pos=str(n + 3), alias=("inplace", "out")[extra % 2])


class Problem:
    """A case made concrete: the tokens' sequence ids and positions as the call is given them, the page table (paged_kv_testlib.PageTable)
    and per token what the definition makes of it."""

    def __init__(self, c, rng):
        self.c, self.ty = c, c["ty"]
        self.qh, self.kvh, self.hd, self.rot, self.style, self.ps = c["qh"], c["kvh"], c["hd"], c["rot"], c["style"], c["ps"]
        self.half = self.rot // 2
        env = {"P": self.ps}
        ev = lambda x: x if x is None else int(eval(str(x), env))
        self.max_pages, self.max_pos = ev(c["max_pages"]), ev(c["max_pos"])
        lens = [ev(x) for x in c["lens"]]
        self.seqs = len(lens)
        pt = PageTable(lens, self.ps, self.max_pages, rng, c["absent"])
        self.table, self.num_pages, self.cap = pt.table, pt.num_pages, self.max_pages * self.ps
        self.cache = c["alias"] != "nocache"
        sp = c["spelling"]
        toks = c["toks"]
        if isinstance(toks, str) and toks.startswith("shuffled:"):
            n = ev(toks.split(":")[1])
            toks = [(0, int(p)) for p in rng.permutation(n)]
        elif toks == "interleaved":
            toks = [(s, p) for s in range(self.seqs) for p in range(lens[s])]
            toks = [toks[j] for j in rng.permutation(len(toks))]
        self.seq_lens = self.positions = self.token_seq = None
        if sp in ("decode", "decode_pos"):
            self.tokens = self.seqs
            self.seq_lens = np.array(lens, dtype=np.int32)
            if sp == "decode_pos":
                self.positions = np.array([L - 1 for L in lens], dtype=np.int32)
                self.seq_lens = None
        elif sp == "seq_only":                      # token_seq given, positions NULL: pos from seq_lens
            self.tokens = len(toks)
            self.token_seq = np.array([t[0] for t in toks], dtype=np.int32)
            self.seq_lens = np.array(lens, dtype=np.int32)
        else:
            self.tokens = len(toks)
            self.token_seq = np.array([t[0] for t in toks], dtype=np.int32)
            self.positions = np.array([ev(t[1]) for t in toks], dtype=np.int32)
        # the definition's s_i, pos_i, padding, and the slot
        self.s = np.arange(self.tokens) if self.token_seq is None else self.token_seq.astype(np.int64)
        s_ok = (self.s >= 0) & (self.s < self.seqs)
        if self.positions is not None:
            self.pos = self.positions.astype(np.int64)
        else:
            self.pos = np.where(s_ok, self.seq_lens[np.where(s_ok, self.s, 0)].astype(np.int64) - 1, -1)
        self.live = (self.pos >= 0) & ((self.pos < self.max_pos) if self.rot else True)          # not a padding token
        self.slot = [None] * self.tokens                                                        # (page, slot) where the append happens
        for i in range(self.tokens):
            if self.cache and self.live[i] and s_ok[i] and self.pos[i] < self.cap:
                pg = int(self.table[self.s[i], self.pos[i] // self.ps])
                if 0 <= pg < self.num_pages:
                    self.slot[i] = (pg, int(self.pos[i] % self.ps))
        named = [x for x in self.slot if x is not None]
        assert len(named) == len(set(named)), "two tokens of a case name the same slot"

    def pairs(self):
        """(a, b): the element indices of the rot_dim / 2 pairs"""
        j = np.arange(self.half)
        return (j, j + self.half) if self.style == NEOX else (2 * j, 2 * j + 1)


# ------------------------------------------------------------------------------------------------ the definition
def rotate(x, c, s, a, b, dtype):
    """The rotation of the definition on x [..., head_dim] (values in dtype) by c, s [..., half] (broadcast over the heads): every operation
    in dtype, each product rounded, then the subtraction / addition rounded.  Returns y (elements outside the pairs are x's) and, for the
    bound, |x_a c| + |x_b s| and |x_b c| + |x_a s| scattered to the elements."""
    x, c, s = x.astype(dtype), c.astype(dtype), s.astype(dtype)
    y, mag = x.copy(), np.zeros(x.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        ac, bs, bc, as_ = (x[..., a] * c).astype(dtype), (x[..., b] * s).astype(dtype), (x[..., b] * c).astype(dtype), (x[..., a] * s).astype(dtype)
        y[..., a] = (ac - bs).astype(dtype)
        y[..., b] = (bc + as_).astype(dtype)
        mag[..., a] = np.abs(ac.astype(np.float64)) + np.abs(bs.astype(np.float64))
        mag[..., b] = np.abs(bc.astype(np.float64)) + np.abs(as_.astype(np.float64))
    return y, mag


def evaluate(pr, Q, K, V, cs, dtype):
    """The definition on Q [tokens][q_heads][hd], K, V [tokens][kv_heads][hd] (bit patterns) and the table cs [max_pos][rot] (float32), every
    operation in `dtype`.  Returns a dict: q, k -- the rotated values [tokens][heads][hd] in dtype (not rounded to the 16-bit type; rows of
    padding tokens hold nothing meaningful), qmag, kmag for the bound, and for dtype float32 qbits, kbits: the values rounded once, the
    elements at or beyond rot_dim bit for bit the input's."""
    a, b = pr.pairs()
    out = {}
    for name, X in (("q", Q), ("k", K)):
        x = f32_of(X, pr.ty)
        y, mag = x.astype(dtype), np.zeros(x.shape)
        bits = np.array(X, dtype=np.uint16, copy=True)
        live = np.flatnonzero(pr.live)
        if pr.rot and live.size:
            rows = cs[pr.pos[live]]                                             # [live][rot]: the tokens' table rows
            y[live], mag[live] = rotate(x[live], rows[:, None, :pr.half], rows[:, None, pr.half:pr.rot], a, b, dtype)
        if dtype == np.float32 and pr.rot:
            rot_cols = np.concatenate([a, b])
            bits[:, :, rot_cols] = rne16(y[:, :, rot_cols], pr.ty)
        out[name], out[name + "mag"], out[name + "bits"] = y, mag, bits
    return out


def bound(pr, ref, got, mag):
    """Per element: half an ulp of the 16-bit type at max(|ref|, |y|) -- the one rounding to 16 bits -- plus 3 2^-24 (|x_a c| + |x_b s|): two
    rounded products and one rounded sum in fp32.  An allowance from the definition, not a measurement."""
    return 0.5 * al.ulp16(np.maximum(np.abs(ref), np.abs(got)), pr.ty) + 3 * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------------ data
def general(pr, rng):
    mk = lambda h: al.bits_of(rng.normal(0.0, 1.0, (pr.tokens, h, pr.hd)), pr.ty)
    return mk(pr.qh), mk(pr.kvh), mk(pr.kvh), table64(pr.max_pos, pr.rot).astype(np.float32)


def special(pr, rng):
    """x from +-0, +-inf, NaN, the largest finite value and the smallest subnormal of the type (and a few ordinary values); c and s from 0, +-1
    and 2^-120: fp32 subnormal products on bf16 inputs (2^-133 * 1, max * 2^-120 * ...), inf * 0, inf - inf."""
    big, tiny = {"f16": (0x7BFF, 0x0001), "bf16": (0x7F7F, 0x0001)}[pr.ty]
    one = int(al.bits_of(np.float32(1.0), pr.ty))
    pool = np.array([0x0000, 0x8000, 0x7C00 if pr.ty == "f16" else 0x7F80, 0xFC00 if pr.ty == "f16" else 0xFF80, NAN16[pr.ty], big, big | 0x8000, tiny,
                     tiny | 0x8000, one, one | 0x8000, int(al.bits_of(np.float32(0.333), pr.ty))], dtype=np.uint16)
    mk = lambda h: pool[rng.integers(0, pool.size, (pr.tokens, h, pr.hd))]
    cpool = np.array([0.0, 1.0, -1.0, 2.0 ** -120, -0.0], dtype=np.float32)
    cs = cpool[rng.integers(0, cpool.size, (pr.max_pos, pr.rot))]
    return mk(pr.qh), mk(pr.kvh), mk(pr.kvh), cs


def _f32_exact(fr):
    """a Fraction rounded ONCE to float32 (nearest even), or None where float64 does not hold it exactly (the candidate is dropped)"""
    f = float(fr)
    return np.float32(f) if Fraction(f) == fr else None


def find_witnesses(ty, rng, want=4):
    """Operands (x_a, x_b, c, s) at which a CONTRACTED evaluation differs from the definition in the rounded 16-bit output -- one list per
    contraction a compiler can make: y_a as fma(x_a, c, -(x_b s)) or fma(-x_b, s, x_a c), y_b as fma(x_b, c, x_a s) or fma(x_a, s, x_b c).
    The fused value is computed exactly (rationals) and rounded once; the premise is asserted.  Returns {kind: [(xa_bits, xb_bits, c, s)]}."""
    found = {k: [] for k in ("ya1", "ya2", "yb1", "yb2")}
    f64 = np.float64
    for _ in range(200):
        n = 1 << 16
        xa, xb = al.bits_of(rng.normal(0, 1, n), ty), al.bits_of(rng.normal(0, 1, n), ty)
        ang = rng.uniform(0, 2 * np.pi, n)
        c, s = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        fa, fb = f32_of(xa, ty), f32_of(xb, ty)
        ac, bs, bc, as_ = fa * c, fb * s, fb * c, fa * s
        plain = {"ya": rne16(ac - bs, ty), "yb": rne16(bc + as_, ty)}
        fused = {"ya1": (f64(fa) * f64(c) - f64(bs)), "ya2": (f64(ac) - f64(fb) * f64(s)), "yb1": (f64(fb) * f64(c) + f64(as_)), "yb2": (f64(fa) * f64(s) + f64(bc))}
        for kind, v in fused.items():
            for j in np.flatnonzero(rne16(v.astype(np.float32), ty) != plain[kind[:2]])[:want]:
                A, B, C, S = Fraction(float(fa[j])), Fraction(float(fb[j])), Fraction(float(c[j])), Fraction(float(s[j]))
                exact = {"ya1": A * C - Fraction(float(bs[j])), "ya2": Fraction(float(ac[j])) - B * S, "yb1": B * C + Fraction(float(as_[j])),
                         "yb2": A * S + Fraction(float(bc[j]))}[kind]
                r = _f32_exact(exact)
                if r is not None and rne16(r, ty) != plain[kind[:2]][j] and len(found[kind]) < want:
                    found[kind].append((int(xa[j]), int(xb[j]), float(c[j]), float(s[j])))
        if all(len(v) >= want for v in found.values()):
            break
    assert all(len(v) >= 1 for v in found.values()), "no contraction witness found: the premise of the test"
    return found


def witness(pr, rng):
    """general data with the witnesses planted: pair j of head 0 of Q and K of the first live tokens, with the table row's (c_j, s_j) replaced"""
    Q, K, V, cs = general(pr, rng)
    a, b = pr.pairs()
    w = [x for v in find_witnesses(pr.ty, rng).values() for x in v]
    live = np.flatnonzero(pr.live)
    used = set()
    k = 0
    for i in live:
        p = int(pr.pos[i])
        if p in used:
            continue                              # a table row is shared by the tokens at that position
        used.add(p)
        for j in range(pr.half):
            if k == len(w):
                break
            xa, xb, c, s = w[k]
            k += 1
            cs[p, j], cs[p, pr.half + j] = c, s
            for X in (Q, K):
                X[i, 0, a[j]], X[i, 0, b[j]] = xa, xb
    assert k == len(w), "the case is too small for the witnesses"
    # the premise at the planted places: the contracted value differs from the definition in the 16-bit output somewhere
    got = evaluate(pr, Q, K, V, cs, np.float32)["qbits"]
    f = lambda X: f32_of(X, pr.ty).astype(np.float64)
    differs = 0
    for i in live:
        row = cs[pr.pos[i]].astype(np.float64)
        c, s = row[:pr.half], row[pr.half:pr.rot]
        xa, xb = f(Q[i, 0, a]), f(Q[i, 0, b])
        fused_a = (xa * c - (xb.astype(np.float32) * s.astype(np.float32)).astype(np.float64)).astype(np.float32)
        differs += int(np.count_nonzero(rne16(fused_a, pr.ty) != got[i, 0, a]))
    assert differs > 0, "the planted witnesses do not separate a contracted kernel"
    return Q, K, V, cs


DATA = {"general": general, "special": special, "witness": witness}


def make(c, what="data"):
    rng = np.random.default_rng(seed(SALT, what, c["name"]))
    pr = Problem(c, rng)
    return pr, DATA[c["data"]](pr, rng)


# ------------------------------------------------------------------------------------------------ the layout builder (GPU test)
class Layout:
    """The call's operands on the device and, on the host, every buffer as the definition leaves it."""

    def __init__(self, pr, Q, K, V, cs, torch):
        self.pr, self.torch = pr, torch
        ty, qh, kvh, hd, T = pr.ty, pr.qh, pr.kvh, pr.hd, pr.tokens
        self.dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
        alias = pr.c["alias"]
        self.inplace = alias == "inplace"
        ar = np.arange
        # the fused QKV buffer: NaN everywhere but the live tokens' elements
        self.ld = (qh + 2 * kvh) * hd + 24
        self.base = 8
        self.col = {"q": 0, "k": qh * hd, "v": (qh + kvh) * hd}
        self.X = Guarded(self.base + T * self.ld + 16, NAN16[ty], np.uint16, self.base, size=0)
        live = np.flatnonzero(pr.live)
        self.ix = {}
        for name, src, h in (("q", Q, qh), ("k", K, kvh), ("v", V, kvh)):
            self.ix[name] = self.base + self.col[name] + ar(T)[:, None] * self.ld + ar(h * hd)[None, :]            # [tokens][h * hd]
            self.X.host[self.ix[name][live].reshape(-1)] = src.reshape(T, -1)[live].reshape(-1)
        # Qo, Ko: distinct buffers, distinct pitches, a sentinel
        self.ldqo, self.ldko, self.qobase, self.kobase = qh * hd + 8, kvh * hd + 16, 16, 8
        self.Qo = Guarded(self.qobase + T * self.ldqo + 16, SENT16, np.uint16, self.qobase, size=0)
        self.Ko = Guarded(self.kobase + T * self.ldko + 16, SENT16, np.uint16, self.kobase, size=0)
        self.iqo = self.qobase + ar(T)[:, None] * self.ldqo + ar(qh * hd)[None, :]
        self.iko = self.kobase + ar(T)[:, None] * self.ldko + ar(kvh * hd)[None, :]
        self.with_ko = alias in ("out", "nocache")
        # the cache: a sentinel everywhere, a guard page in front of page 0 and behind the last page
        self.cache = cl = CacheLayout(pr.num_pages, pr.ps, kvh * hd, pr.seqs, pr.max_pages)
        self.Kc, self.Vc = (cl.cache_buffer(SENT16) for _ in range(2))
        # the table, NaN in its padding, and the int32 operands between guards
        self.ldcs, self.csbase = pr.rot + 4, 4
        self.cs = Guarded(self.csbase + pr.max_pos * self.ldcs + 8, 0x7FC00000, np.uint32, self.csbase, size=0)
        if pr.rot:
            ics = self.csbase + ar(pr.max_pos)[:, None] * self.ldcs + ar(pr.rot)[None, :]
            self.cs.host[ics.reshape(-1)] = np.ascontiguousarray(cs[:, :pr.rot], dtype=np.float32).view(np.uint32).reshape(-1)
        self.T = cl.table_buffer(pr.table)
        wrap = lambda x: None if x is None else Guarded.around(x.astype(np.int32), FILL32, 3, 5)
        self.P, self.S, self.L = wrap(pr.positions), wrap(pr.token_seq), wrap(pr.seq_lens)
        self.bufs = {"qkv": self.X, "Qo": self.Qo, "Ko": self.Ko, "Kc": self.Kc, "Vc": self.Vc, "cs": self.cs, "block_table": self.T, "positions": self.P,
                     "token_seq": self.S, "seq_lens": self.L}
        for g in self.bufs.values():
            if g is not None:
                g.to_device()
        # what the definition leaves in every buffer, and where it writes (compared by NaN class there, bit for bit elsewhere)
        ev = evaluate(pr, Q, K, V, cs, np.float32)
        self.want = {k: g.host.copy() for k, g in self.bufs.items() if g is not None}
        self.written = {k: np.zeros(g.host.size, dtype=bool) for k, g in self.bufs.items() if g is not None}

        def put(buf, idx, bits):
            self.want[buf][idx] = bits
            self.written[buf][idx] = True
        flat = lambda bits: bits[live].reshape(-1)
        if self.inplace:
            put("qkv", self.ix["q"][live].reshape(-1), flat(ev["qbits"]))
            put("qkv", self.ix["k"][live].reshape(-1), flat(ev["kbits"]))
        else:
            put("Qo", self.iqo[live].reshape(-1), flat(ev["qbits"]))
            if self.with_ko:
                put("Ko", self.iko[live].reshape(-1), flat(ev["kbits"]))
        app = np.array([i for i in live if pr.slot[i] is not None], dtype=np.int64)
        if app.size:
            pg, sl = np.array([pr.slot[i] for i in app], dtype=np.int64).T
            at = cl.rows(pg, sl).reshape(-1)
            put("Kc", at, ev["kbits"][app].reshape(-1))
            put("Vc", at, V[app].reshape(-1))

    def args(self):
        pr, tv = self.pr, lambda g: g.dev.view(self.dt)
        sl3 = lambda name, h: tv(self.X).as_strided((pr.tokens, h, pr.hd), (self.ld, pr.hd, 1), self.base + self.col[name])
        q, k, v = sl3("q", pr.qh), sl3("k", pr.kvh), sl3("v", pr.kvh)
        kw = dict(rot_dim=pr.rot, style=pr.style)
        if self.inplace:
            kw.update(q_out=None, k_out=k)
        else:
            kw["q_out"] = tv(self.Qo).as_strided((pr.tokens, pr.qh, pr.hd), (self.ldqo, pr.hd, 1), self.qobase)
            if self.with_ko:
                kw["k_out"] = tv(self.Ko).as_strided((pr.tokens, pr.kvh, pr.hd), (self.ldko, pr.hd, 1), self.kobase)
        if pr.cache:
            kw["k_cache"], kw["v_cache"] = (self.cache.cache_view(tv(g), pr.kvh, pr.hd) for g in (self.Kc, self.Vc))
            kw["block_table"] = self.cache.table_view(self.T.dev)
        for name, g, n in (("positions", self.P, pr.tokens), ("token_seq", self.S, pr.tokens), ("seq_lens", self.L, pr.seqs)):
            if g is not None:
                kw[name] = g.dev[3:3 + n]
        csd = None
        if pr.rot:
            csd = self.cs.dev.view(self.torch.float32).as_strided((pr.max_pos, pr.rot), (self.ldcs, 1), self.csbase)
        return (q, k, v, csd), kw

    def run(self, pkg, form):
        """One call on freshly uploaded buffers.  Asserts the form; then compares EVERY buffer whole with what the definition leaves: the
        written elements by NaN class, everything else -- inputs, padding, unaddressed slots, the guard pages -- bit for bit.  Returns the
        buffers read back."""
        pr = self.pr
        assert pkg.rope_append_form(pr.tokens, pr.qh, pr.kvh, pr.hd, pr.rot) == form, (pkg.rope_append_form(pr.tokens, pr.qh, pr.kvh, pr.hd, pr.rot), form)
        for g in self.bufs.values():
            if g is not None:
                g.dev.copy_(self.torch.from_numpy(g.host.view(SIGNED[g.host.itemsize])))
        pos, kw = self.args()
        ret = pkg.rope_append(*pos, **kw)
        assert ret.data_ptr() == (pos[0] if self.inplace else kw["q_out"]).data_ptr()
        self.torch.cuda.synchronize()
        got = {}
        for name, g in self.bufs.items():
            if g is None:
                continue
            got[name] = h = g.read().copy()
            want, wr = self.want[name], self.written[name]
            if h.itemsize == 2:
                same = np.where(wr, canon16(h, pr.ty) == canon16(want, pr.ty), h == want)
            else:
                same = h == want
            bad = np.flatnonzero(~same)
            assert bad.size == 0, (f"{name}: {bad.size} elements differ from the definition, first at buffer index {bad[:6].tolist()} "
                                   f"(written there by the definition: {wr[bad[:6]].tolist()}; got {[hex(x) for x in h[bad[:6]]]}, want {[hex(x) for x in want[bad[:6]]]})")
        return got

    def twice(self, pkg, form):
        a, b = self.run(pkg, form), self.run(pkg, form)
        assert all(np.array_equal(a[k], b[k]) for k in a), "two runs on the same operands differ"
        return a


def form_of(pkg, pr):
    if pr.tokens == 0 or pr.qh + pr.kvh == 0:
        return "empty"
    return "block" if pr.tokens <= pkg.ROPE_APPEND_BLOCK_MAX_TOKENS else "wave"
