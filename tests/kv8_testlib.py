"""What the fp8 paged KV cache tests share (sm_rope_append_kv8_*, sm_attn_decode_kv8_*): the append restated -- rope_append_testlib's rotation,
then b8_testlib.ref_quant_rows per (token, head) --, the decode definition of include/sparsifyme.h on bytes and scales as ONE numpy function,
evaluated in float32 (the restatement) or float64 (the reference), the bound, the exact classes and the layout builders of the GPU tests:
NaN bytes (0x7f) and NaN scales in every dead slot and unreferenced page, a guard page in front of page 0 and behind the last page of the
bytes AND of the scales, sentinel-filled outputs.  Problem, CASES and the page tables are attn_decode_testlib's and rope_append_testlib's;
the cache's place in its buffers is paged_kv_testlib.CacheLayout with the 16-byte row rule of a byte cache.

fp8 values travel as uint8 bytes, scales as float32, 16-bit values as uint16 bit patterns; `fmt` is "e4m3" or "e5m2", `ty` "f16" or "bf16"."""
import numpy as np

import attn_decode_testlib as al
import b8_testlib as b8
import rope_append_testlib as rl
from guard_testlib import NAN16, SIGNED, Guarded, f32_of, rne16, seed   # noqa: F401  (re-exported)
from paged_kv_testlib import CacheLayout

FMTS = b8.FMTS
SALT = 0x8F8C
NAN8, NAN32 = 0x7F, 0x7FC00000           # a NaN byte of both formats; a quiet NaN scale
SENT8, SENT32 = 0x5A, al.SENT32          # outputs: a byte and a word no result equals by accident
# the relative step of the formats (the quantiser's header comment: 3 / 2 mantissa bits): what the accuracy record is expressed in
RSTEP = {"e4m3": 2.0 ** -4, "e5m2": 2.0 ** -3}


def each(cases, ident, check):
    """check(case) on every case; the failed assertions of ALL cases are reported together, each under its case's id: the GPU test files of
    the fp8 cache are a few test items that walk their case tables"""
    failed = []
    for c in cases:
        try:
            check(c)
        except AssertionError as e:
            failed.append(f"[{ident(c)}] {e}")
    assert not failed, f"{len(failed)} of {len(cases)} cases failed:\n" + "\n".join(failed)


def val32(a, fmt):
    """fp8 bytes -> their exact float32 values (torch's own conversion)"""
    return b8.val64_direct(a, fmt).astype(np.float32)


def finite_bytes(fmt):
    """every byte of the format that is a finite value, ascending"""
    a = np.arange(256, dtype=np.uint8)
    return a[np.isfinite(val32(a, fmt))]


class CacheLayout8(CacheLayout):
    """paged_kv_testlib.CacheLayout for a BYTE cache (rows 16-byte aligned: the page pitch and the base are multiples of 16 elements) and
    the scale arrays [num_pages][kv_heads][page_size] at a pitch above their extent, with a guard page in front and behind as well."""

    def __init__(self, num_pages, page_size, kv_heads, head_dim, seqs, max_pages):
        CacheLayout.__init__(self, num_pages, page_size, kv_heads * head_dim, seqs, max_pages)
        ar = np.arange
        self.kv_heads, self.head_dim = kv_heads, head_dim
        self.page_stride = page_size * self.ldkv + 16
        self.kbase = 16 + self.page_stride
        self.n_kv = self.kbase + (num_pages + 1) * self.page_stride + 16
        self.ikv = self.kbase + ar(num_pages)[:, None, None] * self.page_stride + ar(page_size)[None, :, None] * self.ldkv + ar(self.kv_width)[None, None, :]
        self.sps = kv_heads * page_size + 4
        self.sbase = 4 + self.sps
        self.n_sc = self.sbase + (num_pages + 1) * self.sps + 8
        self.isc = self.sbase + ar(num_pages)[:, None, None] * self.sps + ar(kv_heads)[None, :, None] * page_size + ar(page_size)[None, None, :]   # [page][head][slot]

    def bytes_buffer(self, fill, live=None):
        return Guarded(self.n_kv, fill, np.uint8, self.kbase, idx=self.ikv[np.zeros(self.ikv.shape[:2], dtype=bool) if live is None else live].reshape(-1))

    def scale_buffer(self, fill, live=None):
        """live [num_pages][page_size] bool, as for the bytes: the (page, slot) pairs whose kv_heads scales are logical elements"""
        m = np.zeros((self.num_pages, self.ps), dtype=bool) if live is None else live
        return Guarded(self.n_sc, fill, np.uint32, self.sbase, idx=self.isc.transpose(0, 2, 1)[m].reshape(-1))      # [page][slot][head] order

    def scale_at(self, page, slot):
        """[n][kv_heads]: buffer indices of the scales of the tokens (page[i], slot[i]); ids -1 and num_pages give what an unclamped kernel would address"""
        page, slot = np.asarray(page, dtype=np.int64), np.asarray(slot, dtype=np.int64)
        return self.sbase + page[:, None] * self.sps + np.arange(self.kv_heads)[None, :] * self.ps + slot[:, None]

    def scale_view(self, dev):
        return dev.as_strided((self.num_pages, self.kv_heads, self.ps), (self.sps, self.ps, 1), self.sbase)


# ------------------------------------------------------------------------------------------------ the append, restated
def quant_heads(bits, ty, fmt):
    """bits [n][heads][hd] (16-bit patterns) -> (bytes [n][heads][hd], scales float32 [n][heads]): sm_quantize_rows_fp8_* on every head row"""
    n, h, d = bits.shape
    q, sc = b8.ref_quant_rows(f32_of(bits.reshape(n * h, d), ty), fmt)
    return q.reshape(n, h, d).astype(np.uint8), sc.reshape(n, h).astype(np.float32)


def append_restated(pr, K, V, cs, fmt):
    """rope_append_testlib's float32 evaluation, then the per-row rule: (kbits, K bytes, K scales, V bytes, V scales), rows of every token"""
    ev = rl.evaluate(pr, np.zeros((pr.tokens, pr.qh, pr.hd), dtype=np.uint16), K, V, cs, np.float32)
    with np.errstate(all="ignore"):
        kq, ks = quant_heads(ev["kbits"], pr.ty, fmt)
        vq, vs = quant_heads(V, pr.ty, fmt)
    return ev["kbits"], kq, ks, vq, vs


def special_rows(pr, rng):
    """general data with the rows the per-row rule treats specially planted in head 0 (and the last head) of K and V of the first live tokens:
    all +0, all -0, one NaN among ordinary values, +inf and -inf among ordinary values, a row whose amax is subnormal in the 16-bit type"""
    Q, K, V, cs = rl.general(pr, rng)
    live = np.flatnonzero(pr.live)
    inf = {"f16": 0x7C00, "bf16": 0x7F80}[pr.ty]
    sub = np.array([0x0000, 0x0001, 0x0003, 0x8002, 0x8000, 0x0007], dtype=np.uint16)
    kinds = ["pzero", "nzero", "nan", "inf", "subnormal"]
    for n, i in enumerate(live[:2 * len(kinds)]):
        for X in (K, V):
            for g in {0, pr.kvh - 1}:
                kind = kinds[(n + g) % len(kinds)]
                if kind == "pzero":
                    X[i, g] = 0x0000
                elif kind == "nzero":
                    X[i, g] = 0x8000
                elif kind == "nan":
                    X[i, g, (3 * n + 5) % pr.hd] = NAN16[pr.ty]
                elif kind == "inf":
                    X[i, g, (7 * n + 1) % pr.hd], X[i, g, (7 * n + 9) % pr.hd] = inf, inf | 0x8000
                else:
                    X[i, g] = sub[rng.integers(0, sub.size, pr.hd)]
    return Q, K, V, cs


# ------------------------------------------------------------------------------------------------ the decode definition
def scales_at(S, page, slot):
    """S [num_pages][kv_heads][page_size] -> [T][kv_heads]"""
    return S[page, :, slot]


def evaluate(pr, Q, K8, V8, Ks, Vs, scale, fmt, dtype):
    """The definition on Q [seqs][q_heads][hd] (bit patterns), K8 / V8 [num_pages][page_size][kv_heads][hd] (bytes) and Ks / Vs [num_pages]
    [kv_heads][page_size] (float32), every operation in `dtype`: float32 -- the restatement, exp as exp2f(x * log2e) -- or float64 -- the
    reference.  Returns O (in dtype, NOT rounded), lse, and for the bound A = sum p |vs v8| / sum p, sabs = scale max_t |ks_t| sum_d |q k8|, T."""
    f = np.dtype(dtype).type
    ex = (lambda x: np.exp2((x * al.LOG2E).astype(np.float32))) if dtype == np.float32 else np.exp
    O = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=dtype)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=dtype)
    A, sabs, T = np.zeros_like(O, dtype=np.float64), np.zeros((pr.seqs, pr.q_heads)), np.zeros(pr.seqs, dtype=np.int64)
    q_all, scale = f32_of(Q, pr.ty).astype(dtype), f(scale)
    with np.errstate(all="ignore"):
        for s in range(pr.seqs):
            t, page, slot = pr.tokens(s)
            T[s] = t.size
            if t.size == 0:
                continue
            k = val32(K8[page, slot], fmt).astype(dtype)          # [T][kvh][hd]
            v = val32(V8[page, slot], fmt).astype(dtype)
            ks, vs = scales_at(Ks, page, slot).astype(dtype), scales_at(Vs, page, slot).astype(dtype)     # [T][kvh]
            chunk_of = t // pr.chunk
            for h in range(pr.q_heads):
                kv = h // pr.group
                q = q_all[s, h]
                dot = (k[:, kv] * q[None, :]).sum(axis=1, dtype=dtype).astype(dtype)
                sc = ((dot * ks[:, kv]).astype(dtype) * scale).astype(dtype)
                sabs[s, h] = float(scale) * (np.abs(ks[:, kv].astype(np.float64)) * np.abs(k[:, kv].astype(np.float64) * q[None, :].astype(np.float64)).sum(axis=1)).max()
                parts = []
                for cidx in range(-(-pr.lens[s] // pr.chunk)):       # every chunk the sequence has, ascending
                    sel = chunk_of == cidx
                    if not sel.any():
                        parts.append((f(-np.inf), f(0), np.zeros(pr.hd, dtype=dtype), np.zeros(pr.hd)))
                        continue
                    m_c = sc[sel].max()
                    p = f32_of(rne16(ex((sc[sel] - m_c).astype(dtype)).astype(np.float32), pr.ty), pr.ty).astype(dtype)
                    pv = (p * vs[sel, kv]).astype(dtype)             # one rounded multiply per token
                    parts.append((m_c, p.sum(dtype=dtype), (pv[:, None] * v[sel, kv]).sum(axis=0, dtype=dtype),
                                  (np.abs(pv[:, None].astype(np.float64)) * np.abs(v[sel, kv]).astype(np.float64)).sum(axis=0)))
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


def restate32(pr, Q, K8, V8, Ks, Vs, scale, fmt):
    O, lse, _, _, _ = evaluate(pr, Q, K8, V8, Ks, Vs, scale, fmt, np.float32)
    return rne16(O, pr.ty), lse


def bound(pr, ref, got, A, sabs, T, scale):
    """attn_decode_testlib.bound with A taken over |vs v8| and two further 2^-24 terms: the ks multiply moves every score by a relative
    2^-24, one more term of delta = (head_dim + 3) 2^-24 sabs (it enters twice, above and below the division); the p vs multiply moves every
    summand of the numerator by a relative 2^-24, one more 2^-24 in the A term.  Derived from the definition, not measured."""
    return al.bound(pr, ref, got, A, sabs, T, scale) + (2 * 2.0 ** -24 * sabs[..., None] + 2.0 ** -24) * A


def lse_bound(pr, ref_lse, sabs):
    return al.lse_bound(pr, ref_lse, sabs) + 2.0 ** -24 * sabs


def worst_ratios(pr, got_bits, got_lse, Q, K8, V8, Ks, Vs, scale, fmt):
    """(worst |O - ref| / bound, worst |lse - ref| / bound, A) against the fp64 definition; -inf must sit exactly where the reference has it"""
    ref, rl_, A, sabs, T = evaluate(pr, Q, K8, V8, Ks, Vs, scale, fmt, np.float64)
    got = f32_of(got_bits, pr.ty).astype(np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all(), "a non-finite output on finite live data: a masked slot or an absent page was read"
    ro = float((np.abs(got - ref) / bound(pr, ref, got, A, sabs, T, scale)).max())
    gl = np.asarray(got_lse, dtype=np.float64)
    assert np.array_equal(np.isneginf(gl), np.isneginf(rl_)) and not np.isnan(gl).any()
    fin = np.isfinite(rl_)
    with np.errstate(invalid="ignore"):
        rlr = float((np.abs(gl - rl_)[fin] / lse_bound(pr, rl_, sabs)[fin]).max()) if fin.any() else 0.0
    return ro, rlr


# ------------------------------------------------------------------------------------------------ data of the decode tests
def pow2_scales(pr, rng, lo, hi):
    """[num_pages][kv_heads][page_size] float32 powers of two 2^lo .. 2^hi"""
    return (2.0 ** rng.integers(lo, hi + 1, (pr.num_pages, pr.kvh, pr.ps))).astype(np.float32)


def general(pr, rng, sigma, fmt):
    """Q ~ N(0, 1); K and V as the quantiser leaves rows of N(0, 1) and N(0, sigma): bytes with per-row scales"""
    Q = al.bits_of(rng.normal(0.0, 1.0, (pr.seqs, pr.q_heads, pr.hd)), pr.ty)
    out = [Q]
    for sg in (1.0, sigma):
        x = al.bits_of(rng.normal(0.0, sg, (pr.num_pages * pr.ps, pr.kvh, pr.hd)), pr.ty)
        q, sc = quant_heads(x, pr.ty, fmt)
        out += [q.reshape(pr.num_pages, pr.ps, pr.kvh, pr.hd), np.ascontiguousarray(sc.reshape(pr.num_pages, pr.ps, pr.kvh).transpose(0, 2, 1))]
    Q, K8, Ks, V8, Vs = out
    return Q, K8, V8, Ks, Vs


def v_codes8(pr, fmt):
    """V bytes that encode (page, slot, kv head, dim) and run over every finite byte of the format"""
    fb = finite_bytes(fmt)
    p, s, k, d = np.meshgrid(np.arange(pr.num_pages), np.arange(pr.ps), np.arange(pr.kvh), np.arange(pr.hd), indexing="ij")
    return fb[(p * 7919 + s * 131 + k * 37 + d * 3) % fb.size]


def one_hot(pr, rng, fmt):
    """attn_decode_testlib.one_hot on the fp8 cache: K bytes are its K (entries 0 and 4, exact in both formats) with ks a power of two in
    1 .. 4 -- the target scores 128 ks >= 128, every other present token 0 --, V runs over every finite byte with vs a power of two in
    2^-2 .. 2^2.  Expected O = rne16(fp32(v8) vs) of the target row (a -0 product summed into +0 is +0) and lse = 128 ks, exactly."""
    Q, Kb, _, targets, _, _ = al.one_hot(pr, rng)
    kval = f32_of(Kb, pr.ty)
    K8 = b8.to8(kval, fmt)
    assert np.array_equal(val32(K8, fmt), kval), "the one-hot K is exact in the format"
    V8 = v_codes8(pr, fmt)
    Ks, Vs = pow2_scales(pr, rng, 0, 2), pow2_scales(pr, rng, -2, 2)
    want = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=np.float32)
    for (s, h), (pg, sl, _) in targets.items():
        kv = h // pr.group
        prod = (val32(V8[pg, sl, kv], fmt) * Vs[pg, kv, sl]).astype(np.float32)
        want[s, h] = rne16(prod + np.float32(0.0), pr.ty)
        lse[s, h] = np.float32(128.0) * Ks[pg, kv, sl]
    return Q, K8, V8, Ks, Vs, targets, want, lse


def uniform(pr, rng, fmt):
    """Q = 0, so every p = 1 and every w = 1; V integers |v| <= 7 (exact in both formats), vs a per-token power of two in 2^-2 .. 2^2: in
    units of 2^-2 every summand vs v is an integer, so every partial sum is exact in any order while 7 * 4 * L < 2^24 (asserted, in both
    units).  Expected O = rne16(fp32(sum vs v) / fp32(T)) and lse = log(T)."""
    Q = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    K8 = b8.finite_bytes(rng, (pr.num_pages, pr.ps, pr.kvh, pr.hd), fmt)
    Ks = pow2_scales(pr, rng, -2, 2)
    Vi = rng.integers(-7, 8, (pr.num_pages, pr.ps, pr.kvh, pr.hd))
    V8 = b8.to8(Vi.astype(np.float32), fmt)
    assert np.array_equal(val32(V8, fmt), Vi.astype(np.float32)), "integers up to 7 are exact in the format"
    Vs = pow2_scales(pr, rng, -2, 2)
    # in units of 2^-2 every summand is an integer of magnitude at most 7 * 16, and so is every partial sum: exact while 7 * 16 * L < 2^24
    assert 7 * 4 * max(pr.lens + [1]) < 2 ** 24 and 7 * 16 * max(pr.lens + [1]) < 2 ** 24 and np.abs(Vi).max() <= 7
    want = np.zeros((pr.seqs, pr.q_heads, pr.hd), dtype=np.uint16)
    lse = np.full((pr.seqs, pr.q_heads), -np.inf, dtype=np.float64)
    for s in range(pr.seqs):
        t, page, slot = pr.tokens(s)
        if t.size == 0:
            continue
        tot = (Vi[page, slot].astype(np.float64) * scales_at(Vs, page, slot).astype(np.float64)[:, :, None]).sum(axis=0)    # [kvh][hd], exact
        assert np.array_equal(tot.astype(np.float32).astype(np.float64), tot)
        o = rne16((tot.astype(np.float32) / np.float32(t.size)).astype(np.float32), pr.ty)
        want[s] = np.repeat(o, pr.group, axis=0)
        lse[s] = np.log(float(t.size))
    return Q, K8, V8, Ks, Vs, want, lse


# ------------------------------------------------------------------------------------------------ the decode layout builder (GPU test)
class DecodeLayout:
    """The call's operands on the device.  Inputs are NaN outside their live elements -- bytes 0x7f, scales NaN --; outputs hold a sentinel."""

    def __init__(self, pr, Q, K8, V8, Ks, Vs, fmt, torch):
        import guard_testlib as gl
        self.pr, self.torch, self.fmt, self.gl = pr, torch, fmt, gl
        qh, hd, ty = pr.q_heads, pr.hd, pr.ty
        self.dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
        self.ldq, self.ldo, self.qbase, self.obase = qh * hd + 24, qh * hd + 8, 8, 16
        self.cache = cl = CacheLayout8(pr.num_pages, pr.ps, pr.kvh, hd, pr.seqs, pr.max_pages)
        ar = np.arange
        iq = (self.qbase + ar(pr.seqs)[:, None] * self.ldq + ar(qh * hd)[None, :]).reshape(-1)
        self.Q = Guarded(self.qbase + pr.seqs * self.ldq + 16, NAN16[ty], np.uint16, self.qbase, idx=iq)
        self.Q.host[iq] = Q.reshape(-1)
        live = pr.live()
        self.K, self.V = (cl.bytes_buffer(NAN8, live) for _ in range(2))
        self.K.host[self.K.idx] = K8.reshape(pr.num_pages, pr.ps, -1)[live].reshape(-1)
        self.V.host[self.V.idx] = V8.reshape(pr.num_pages, pr.ps, -1)[live].reshape(-1)
        self.Ks, self.Vs = (cl.scale_buffer(NAN32, live) for _ in range(2))
        for g, S in ((self.Ks, Ks), (self.Vs, Vs)):
            g.host[g.idx] = np.ascontiguousarray(S.transpose(0, 2, 1), dtype=np.float32)[live].reshape(-1).view(np.uint32)
        self.T = cl.table_buffer(pr.table)
        self.Ls = Guarded.around(np.array(pr.raw_lens, dtype=np.int32), 0x7FFFFFF0, 3, 5)
        self.io = (self.obase + ar(pr.seqs)[:, None] * self.ldo + ar(qh * hd)[None, :]).reshape(-1)
        self.O = Guarded(self.obase + pr.seqs * self.ldo + 16, al.SENT16, np.uint16, self.obase, idx=self.io)
        self.lse = Guarded(pr.seqs * qh + 13, SENT32, np.uint32, 6, size=pr.seqs * qh)
        for g in (self.Q, self.K, self.V, self.Ks, self.Vs, self.T, self.Ls, self.O, self.lse):
            g.to_device()

    def tensors(self):
        pr, cl = self.pr, self.cache
        q = self.Q.dev.view(self.dt).as_strided((pr.seqs, pr.q_heads, pr.hd), (self.ldq, pr.hd, 1), self.qbase)
        o = self.O.dev.view(self.dt).as_strided((pr.seqs, pr.q_heads, pr.hd), (self.ldo, pr.hd, 1), self.obase)
        kv = [cl.cache_view(g.dev.view(b8.tdt(self.fmt)), pr.kvh, pr.hd) for g in (self.K, self.V)]
        sc = [cl.scale_view(g.dev.view(self.torch.float32)) for g in (self.Ks, self.Vs)]
        lse = self.lse.dev.view(self.torch.float32)[6:6 + pr.seqs * pr.q_heads].view(pr.seqs, pr.q_heads)
        return q, kv[0], kv[1], sc[0], sc[1], cl.table_view(self.T.dev), self.Ls.dev[3:3 + pr.seqs], o, lse

    def run(self, pkg, scale, form):
        """the call with a workspace of exactly the reported size between guards; asserts the form, that no input changed and that nothing
        outside the outputs was written; returns (O bits [seqs][q_heads][hd], lse float32 [seqs][q_heads])"""
        pr = self.pr
        assert pkg.attn_decode_form(pr.seqs, pr.q_heads, pr.kvh, pr.hd, pr.ps, pr.max_pages) == form
        need = pkg.attn_decode_workspace_size(pr.seqs, pr.q_heads, pr.hd, pr.ps, pr.max_pages)
        assert (need > 0) == (form == "split")
        ws = self.gl.Workspace(need, off=16) if need else None
        q, k, v, ks, vs, bt, sl, o, lse = self.tensors()
        self.O.dev.copy_(self.torch.from_numpy(self.O.host.view(np.int16)))
        self.lse.dev.copy_(self.torch.from_numpy(self.lse.host.view(np.int32)))
        pkg.attn_decode_kv8(q, k, v, ks, vs, bt, sl, scale=scale, out=o, lse=lse, workspace=ws.p[:need] if ws else None)
        self.torch.cuda.synchronize()
        for g, name in ((self.Q, "Q"), (self.K, "Kc8"), (self.V, "Vc8"), (self.Ks, "Ksc"), (self.Vs, "Vsc"), (self.T, "block_table"), (self.Ls, "seq_lens")):
            assert g.unchanged(), f"{name} was written"
        if ws:
            ws.check("attn_decode_kv8 workspace")
        said = lambda what: (lambda n, first: f"{n} elements outside {what} were written, first at {first.tolist()}")
        ob = self.O.result(said("O")).reshape(pr.seqs, pr.q_heads, pr.hd)
        lb = self.lse.result(said("lse")).view(np.float32).reshape(pr.seqs, pr.q_heads)
        return ob.copy(), lb.copy()

    def twice(self, pkg, scale, form):
        a, b = self.run(pkg, scale, form), self.run(pkg, scale, form)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "two runs on the same operands differ"
        return a


# ------------------------------------------------------------------------------------------------ the append cases and layout builder (GPU test)
def append_cases():
    """(case, fmt): every case of rope_append_testlib's table the fp8 call accepts (head_dim 64 / 128, with a cache) except the contraction
    witnesses (the rotation is shared code, held there), the formats alternating; then each type x format x style at rot_dim 0, the
    non-power-of-two item count (head_dim 64, rot_dim 32, NEOX: 6 lanes a head; 128 / 64: 12) and rot_dim == head_dim; a sequence id out of
    range with a position given; and the special rows of the per-row rule, rotated and not."""
    out = []
    for c in rl.CASES:
        if c["hd"] in (64, 128) and c["alias"] != "nocache" and c["data"] != "witness":
            out.append((c, FMTS[len(out) % 2]))
    toks = [(0, 0), (1, 3), (0, 1), (1, 0), (0, 17), (0, 15), (0, 16)]
    n = 0
    for ty in rl.TYPES:
        for fmt in FMTS:
            for hd, rot, style in ((64, 32, rl.NEOX), (128, 64, rl.NEOX), (64, 0, rl.INTERLEAVED), (128, 128, rl.INTERLEAVED), (64, 64, rl.NEOX), (128, 16, rl.NEOX)):
                heads = [(5, 5), (8, 2), (3, 1), (32, 8)][n % 4]
                out.append((rl.case(f"kv8-{n}", ty, heads[0], heads[1], hd, rot, style, toks=toks, lens=("P+2", "4"), alias=("out", "inplace", "ko_null")[n % 3]), fmt))
                n += 1
    out.append((rl.case("kv8-no-append-seq", "bf16", 3, 1, 64, 64, rl.INTERLEAVED, toks=[(0, 1), (-1, 2), (2, 3), (1, 0)], lens=("2", "1")), "e4m3"))
    for n, (ty, fmt, hd, rot, style) in enumerate((("f16", "e4m3", 64, 0, rl.NEOX), ("bf16", "e5m2", 128, 0, rl.INTERLEAVED), ("bf16", "e4m3", 64, 32, rl.NEOX),
                                                   ("f16", "e5m2", 128, 128, rl.NEOX))):
        out.append((rl.case(f"kv8-special-rows-{n}", ty, 8, 2, hd, rot, style, toks="interleaved", lens=("P+1", "11"), data="special_rows"), fmt))
    return out


def append_case_id(cf):
    return rl.case_id(cf[0]) + "-" + cf[1]


def make_append(c, what="data"):
    rng = np.random.default_rng(seed(SALT, what, c["name"]))
    pr = rl.Problem(c, rng)
    data = special_rows if c["data"] == "special_rows" else rl.DATA[c["data"]]
    return pr, data(pr, rng)


class AppendLayout(rl.Layout):
    """rope_append_testlib.Layout with the fp8 cache in the place of the 16-bit one: Kc8, Vc8 (bytes) and Ksc, Vsc (scales) hold a sentinel
    everywhere -- unaddressed slots, unreferenced pages and the guard pages included -- and `want` is what the restatement leaves there."""

    def __init__(self, pr, Q, K, V, cs, fmt, torch):
        assert pr.cache
        rl.Layout.__init__(self, pr, Q, K, V, cs, torch)
        self.fmt = fmt
        for name in ("Kc", "Vc"):                    # the 16-bit cache is not an operand of this call
            del self.bufs[name], self.want[name], self.written[name]
        self.cache8 = cl = CacheLayout8(pr.num_pages, pr.ps, pr.kvh, pr.hd, pr.seqs, pr.max_pages)
        self.Kc8, self.Vc8 = (cl.bytes_buffer(SENT8) for _ in range(2))
        self.Ksc, self.Vsc = (cl.scale_buffer(SENT32) for _ in range(2))
        for name, g in (("Kc8", self.Kc8), ("Vc8", self.Vc8), ("Ksc", self.Ksc), ("Vsc", self.Vsc)):
            g.to_device()
            self.bufs[name], self.want[name], self.written[name] = g, g.host.copy(), np.zeros(g.host.size, dtype=bool)
        _, kq, ks, vq, vs = append_restated(pr, K, V, cs, fmt)
        app = np.array([i for i in np.flatnonzero(pr.live) if pr.slot[i] is not None], dtype=np.int64)
        if app.size:
            pg, sl = np.array([pr.slot[i] for i in app], dtype=np.int64).T
            at, sat = cl.rows(pg, sl).reshape(-1), cl.scale_at(pg, sl).reshape(-1)
            for name, idx, val in (("Kc8", at, kq[app].reshape(-1)), ("Vc8", at, vq[app].reshape(-1)), ("Ksc", sat, ks[app].reshape(-1).view(np.uint32)),
                                   ("Vsc", sat, vs[app].reshape(-1).view(np.uint32))):
                self.want[name][idx] = val
                self.written[name][idx] = True

    def args(self):
        pos, kw = rl.Layout.args(self)
        cl, pr = self.cache8, self.pr
        kw.pop("k_cache"), kw.pop("v_cache")
        kw["k_cache"], kw["v_cache"] = (cl.cache_view(g.dev.view(b8.tdt(self.fmt)), pr.kvh, pr.hd) for g in (self.Kc8, self.Vc8))
        kw["k_scale"], kw["v_scale"] = (cl.scale_view(g.dev.view(self.torch.float32)) for g in (self.Ksc, self.Vsc))
        return pos, kw

    def run(self, pkg, form):
        """One call on freshly uploaded buffers; EVERY buffer compared whole with what the restatement leaves: Qo and Ko by NaN class where
        written, the bytes, the scales and everything else bit for bit.  Returns the buffers read back."""
        pr = self.pr
        assert pkg.rope_append_form(pr.tokens, pr.qh, pr.kvh, pr.hd, pr.rot) == form
        for g in self.bufs.values():
            if g is not None:
                g.dev.copy_(self.torch.from_numpy(g.host.view(SIGNED[g.host.itemsize])))
        pos, kw = self.args()
        ret = pkg.rope_append_kv8(*pos, **kw)
        assert ret.data_ptr() == (pos[0] if self.inplace else kw["q_out"]).data_ptr()
        self.torch.cuda.synchronize()
        got = {}
        for name, g in self.bufs.items():
            if g is None:
                continue
            got[name] = h = g.read().copy()
            want, wr = self.want[name], self.written[name]
            same = np.where(wr, rl.canon16(h, pr.ty) == rl.canon16(want, pr.ty), h == want) if h.itemsize == 2 else h == want
            bad = np.flatnonzero(~same)
            assert bad.size == 0, (f"{name}: {bad.size} elements differ from the restatement, first at buffer index {bad[:6].tolist()} "
                                   f"(written there by the definition: {wr[bad[:6]].tolist()}; got {[hex(x) for x in h[bad[:6]]]}, want {[hex(x) for x in want[bad[:6]]]})")
        return got

    def twice(self, pkg, form):
        a, b = self.run(pkg, form), self.run(pkg, form)
        assert all(np.array_equal(a[k], b[k]) for k in a), "two runs on the same operands differ"
        return a
