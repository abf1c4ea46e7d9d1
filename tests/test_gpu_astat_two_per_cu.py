"""The two A-stationary kernels of sm_spmma_fused_{f16,bf16} -- two workgroups per CU (k <= 256) and one per CU (every other
A-stationary call) -- bit for bit against sm_compress24_* + sm_spmma_* on the same operands (-m gpu).

Every case first asserts, through sm_spmma_fused_form, that the call reaches the A-stationary form.  C lies between two runs of
guard words and, with a strideC gap, around gap words; the whole buffer -- guards, gaps and result -- is compared, so a store
outside the logical result fails the case.  The gaps and the slack of A hold NaN: a row read from there shows in the product.
The cases: k / 64 = 1 .. 3 (two per CU at every grid size, 16-row C patches), k = 256 on both sides of its grid rule (small or
column-split grids: one per CU; panels525_k256, unsplit and above 7/4 workgroups per CU: two per CU with 8-row patches) and
k / 64 = 5 (one per CU), ragged rows and columns, single panels split 8 ways over the columns, batches that are not back to back,
grouped launches, and grids of more than 2 x CUs workgroups, on which CUs really hold two."""
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64           # elements before and after C (128 bytes: the logical C stays 16-byte aligned)
SENTINEL = 0x5A5A    # bits of every element of the C buffer before the call
DT_IDS = ["f16", "bf16"]

# (m, n, k, batch, count, gapA, gapC)
CASES = {
    "k64_tail": (130, 264, 64, 1, 1, 0, 0),
    "k128_tail_b2": (129, 264, 128, 2, 1, 0, 0),
    "k192_b3": (200, 520, 192, 3, 1, 0, 0),
    "k256_tight_lds": (257, 384, 256, 2, 1, 0, 0),
    "k320_one_per_cu": (130, 264, 320, 1, 1, 0, 0),
    "one_panel_nsplit8": (100, 2048, 256, 1, 1, 0, 0),
    "one_panel_nsplit8_ragged": (127, 1032, 256, 1, 1, 0, 0),
    "batches_apart_k128": (200, 264, 128, 3, 1, 64, 8),
    "batches_apart_k256": (257, 384, 256, 2, 1, 8, 24),
    "batches_apart_k320": (130, 264, 320, 2, 1, 64, 8),
    "grouped3": (200, 264, 128, 2, 3, 0, 0),
    "grouped3_k320": (200, 264, 320, 2, 3, 0, 0),
    "panels525_k256": (2100, 264, 256, 32, 1, 0, 0),
    "panels525_k128_grouped2": (2100, 264, 128, 32, 2, 0, 0),
}


def _sentinels(torch, numel):
    return torch.full((numel,), SENTINEL, dtype=torch.int16, device="cuda")


@pytest.mark.parametrize("bf", [False, True], ids=DT_IDS)
@pytest.mark.parametrize("case", list(CASES))
def test_astat_kernels_equal_staged(gpu, case, bf):
    import torch
    m, n, k, batch, count, gapA, gapC = CASES[case]
    dt = torch.bfloat16 if bf else torch.float16
    sA, sC = m * k + gapA, m * n + gapC
    assert gpu.spmma_fused_form(m, n, k, k, batch, count, sA, 0, sC) == "astat", f"{case} reaches another form"
    As, Bs, Cbufs, want = [], [], [], []
    for i in range(count):
        Ac = torch.empty(batch * m * k, dtype=dt, device="cuda")
        gpu.fill_uniform(Ac, 77 + 13 * i + m, -1.0, 1.0)
        B = torch.empty(k * n, dtype=dt, device="cuda")
        gpu.fill_uniform(B, 99 + 7 * i + n, -1.0, 1.0)
        # the padded A: NaN in the gaps between the batches and behind the last one
        A = torch.full((batch * sA + 64,), float("nan"), dtype=dt, device="cuda")
        A[:batch * sA].view(batch, sA)[:, :m * k] = Ac.view(batch, m * k)
        # compress + spmma on the compact copy: the bits the fused call must return
        blob = torch.empty(gpu.compress24_size(m, k, 2, batch), dtype=torch.uint8, device="cuda")
        gpu.compress24(Ac, m, k, k, batch, m * k, blob)
        Cref = torch.zeros(batch * m * n, dtype=dt, device="cuda")
        gpu.spmma(blob, B, Cref, m, n, k, batch, 0)
        w = _sentinels(torch, GUARD + batch * sC + GUARD)
        w[GUARD:GUARD + batch * sC].view(batch, sC)[:, :m * n] = Cref.view(torch.int16).view(batch, m * n)
        As.append(A); Bs.append(B); want.append(w)
        Cbufs.append(_sentinels(torch, GUARD + batch * sC + GUARD))
    Cs = [c.view(dt)[GUARD:] for c in Cbufs]
    assert all(c.data_ptr() % 16 == 0 for c in Cs) and all(a.data_ptr() % 16 == 0 for a in As)
    if count == 1:
        gpu.spmma_fused(As[0], Bs[0], Cs[0], m, n, k, batch=batch, strideA=sA, strideC=sC)
    else:
        gpu.spmma_fused_grouped(As, Bs, Cs, m, n, k, batch=batch, strideA=sA, strideC=sC)
    torch.cuda.synchronize()
    for i in range(count):
        if not torch.equal(Cbufs[i], want[i]):
            bad = torch.nonzero(Cbufs[i] != want[i]).flatten()
            first = int(bad[0].item()) - GUARD
            where = "a guard or gap word" if first < 0 or first >= batch * sC or first % sC >= m * n else \
                f"(batch, row, col) = ({first // sC}, {first % sC // n}, {first % sC % n})"
            pytest.fail(f"{case} {DT_IDS[bf]} problem {i}: {bad.numel()} elements differ from compress + spmma, first at {where}")
