/*
 * sparsifyme.h -- C ABI of libsparsifyme.so, the MI355X (gfx950) back end of the sparsify.me
 * hot path: prune to 2:4 -> compress -> sparse x dense matmul, measured against the library's
 * own dense batched GEMM.
 *
 * This is the drop-in boundary.  The reference (owensgroup/sparsify.me) is a header-only CUDA C++
 * template API; each entry point below replaces the vendor call(s) named next to it, and the
 * templates in include/sparsify.me/ *.hxx (same paths, namespace and signatures as the reference)
 * forward to these symbols.  Everything is `extern "C"`, plain pointers and sizes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - functions only enqueue work on `stream` (no allocation, no synchronisation), so a caller
 *     may capture them into a hipGraph (one exception, stated at sm_spmm_bell_batched_f32); they
 *     return SM_STATUS_* (0 = success) and never throw;
 *   - fp16 data are IEEE binary16 bit patterns (`_Float16` / `__half` / uint16_t storage).
 *
 * 2:4 compressed blob (produced by sm_compress24_*, consumed by sm_spmma_* / sm_decompress24_*),
 * for `batch` row-major m x k matrices, M = batch*m rows:
 *   kc       = k rounded up to a multiple of 64
 *   both sections are STAGE-major: plane s covers dense k 64s..64s+63 of every row
 *   values   : [kc/64][M][32] elements at byte 0 (kept pair of strip q of row R at
 *              [q/16][R][2(q%16)], [q/16][R][2(q%16)+1])
 *   metadata : [kc/64][M][8] bytes at byte round_up(M*(kc/2)*elt, 256); strip q's nibble
 *              (p0 | p1 << 2, p0 < p1 kept positions) in bits 4*(q&1).. of byte [q/16][R][(q%16)/2]
 *   size     = sm_compress24_size()
 */
#ifndef SPARSIFYME_H_
#define SPARSIFYME_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SM_STATUS_SUCCESS 0
#define SM_STATUS_INVALID_VALUE 1   /* bad pointer / size / flag                          */
#define SM_STATUS_NOT_SUPPORTED 2   /* valid request this build has no kernel for          */
#define SM_STATUS_LAUNCH_FAILED 3   /* HIP reported an error at launch                     */
#define SM_STATUS_NO_DEVICE 4       /* no gfx950 device visible                            */

#define SM_PRUNE_TILE 0   /* cusparseLtPruneAlg_t numbering used at spmma.hxx:86 */
#define SM_PRUNE_STRIP 1

#define SM_OP_N 0
#define SM_OP_T 1

typedef void* sm_stream_t; /* hipStream_t */

/* Library / device info (host). */
const char* sm_version(void);
/* 0 when a gfx950 device is usable by this process, else SM_STATUS_NO_DEVICE. */
int sm_device_check(void);
/* Message of the last failing call made by the calling thread ("" if none). */
const char* sm_last_error(void);

/* ---- (a1) positional sparsify: replaces the Thrust fill + transform of
 *      include/sparsify.me/sparsify.hxx:71-81 (sparsifyme::sparsify<BLK_M,BLK_N,type_t>).
 *      weights: m*n elements of elt_bytes (2, 4 or 8), zeroed in place; mask: m*n uint64
 *      (the reference's std::size_t mask), written in full. */
int sm_sparsify_positional(void* weights, uint64_t* mask, size_t m, size_t n, size_t elt_bytes,
                           size_t blk_m, size_t blk_n, float sparsity_factor, sm_stream_t stream);
int sm_sparsify_positional_f16(void* weights, uint64_t* mask, size_t m, size_t n,
                               float sparsity_factor, sm_stream_t stream);
int sm_sparsify_positional_f32(float* weights, uint64_t* mask, size_t m, size_t n,
                               float sparsity_factor, sm_stream_t stream);
int sm_sparsify_positional_f64(double* weights, uint64_t* mask, size_t m, size_t n,
                               float sparsity_factor, sm_stream_t stream);

/* ---- (a2) prune to 2:4: replaces cusparseLtSpMMAPrune (spmma.hxx:86-87).
 *      A_in / A_out row-major m x k, leading dimension ld elements; may alias (in place). */
int sm_prune24_f16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg,
                   sm_stream_t stream);
int sm_prune24_f32(const float* A_in, float* A_out, size_t m, size_t k, size_t ld, int alg,
                   sm_stream_t stream);

/* ---- (a2) prune check: replaces cusparseLtSpMMAPruneCheck (spmma.hxx:88).
 *      *d_valid (device int) = 0 iff every 1x4 strip has <= 2 non-zeros, else 1. */
int sm_prune24_check_f16(const void* A, size_t m, size_t k, size_t ld, int* d_valid,
                         sm_stream_t stream);
int sm_prune24_check_f32(const float* A, size_t m, size_t k, size_t ld, int* d_valid,
                         sm_stream_t stream);

/* ---- (a3) compress: replaces cusparseLtSpMMACompressedSize + cusparseLtSpMMACompress
 *      (spmma.hxx:100-103).  A: batch matrices, row-major m x k, ld, batch stride strideA
 *      elements.  Keeps the two largest |x| of every strip (STRIP rule), i.e. for an already
 *      pruned A exactly its non-zeros; so compress alone is also the fused prune+compress. */
int sm_compress24_size(size_t m, size_t k, size_t elt_bytes, size_t batch, size_t* bytes /*host*/);
int sm_compress24_f16(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                      void* blob, sm_stream_t stream);
int sm_compress24_f32(const float* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                      void* blob, sm_stream_t stream);
/* Inverse (test/debug aid; no reference counterpart). */
int sm_decompress24_f16(const void* blob, size_t m, size_t k, size_t ld, size_t batch,
                        size_t strideA, void* A, sm_stream_t stream);
int sm_decompress24_f32(const void* blob, size_t m, size_t k, size_t ld, size_t batch,
                        size_t strideA, float* A, sm_stream_t stream);

/* ---- (a2 + a3 in one pass) prune -> check -> compress as sparsifyme::spmma() runs them (spmma.hxx:82-104:
 *      cusparseLtSpMMAPrune in place, cusparseLtSpMMAPruneCheck, cusparseLtSpMMACompress): reads A_in once and writes
 *      the pruned operand to A_out (may alias A_in: in place; NULL: not wanted), the compressed blob (NULL: not wanted)
 *      and *d_valid (NULL: not wanted; 0 iff every strip written holds <= 2 non-zeros).  `batch` row-major m x k
 *      matrices strideA elements apart; a 4 x 4 TILE never straddles two of them.  alg = SM_PRUNE_TILE or
 *      SM_PRUNE_STRIP.  Same bytes as sm_prune24_* followed by sm_prune24_check_* and sm_compress24_* (which is what
 *      runs for shapes the one-pass kernel does not take: k % 64 != 0 or unaligned rows). */
int sm_prune24_compress24_f16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                              void* blob, int* d_valid, int alg, sm_stream_t stream);
int sm_prune24_compress24_bf16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                               void* blob, int* d_valid, int alg, sm_stream_t stream);
/* fp32 form (the type the reference's own driver instantiates, examples/spmma.cu:24): 2:4 on fp32 as everywhere in this
 * build; same bytes as sm_prune24_f32 + sm_prune24_check_f32 + sm_compress24_f32. */
int sm_prune24_compress24_f32(const float* A_in, float* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                              void* blob, int* d_valid, int alg, sm_stream_t stream);

/* ---- WHICH KERNEL a prune / check / compress / decompress / one-pass call runs: the dispatch rules of the entry points above as
 *      host-side queries -- each is the one function its entry point itself switches on, so the answer is what launches.  For tests (a
 *      test named for a kernel asserts that its call reaches it) and tools; no device work.  Arguments are the call's own sizes and
 *      strides, elt_bytes (2: f16 and bf16, which dispatch alike; 4: fp32), alg, and the operand POINTERS, which are taken as addresses
 *      only (alignment, null or not) and never dereferenced.  *form = _INVALID: the entry point returns SM_STATUS_INVALID_VALUE; _EMPTY:
 *      success, nothing launched.  Status: SM_STATUS_INVALID_VALUE for form == NULL or another elt_bytes.
 *
 *      sm_prune24_form / sm_prune24_check_form (SM_PRUNE24_FORM_*):
 *        STRIP and the check run one kernel with two flags: VEC -- both pointers 16-byte aligned and ld % 8 == 0 (fp32: ld % 4 == 0),
 *        16-byte accesses, else element accesses; FLAT -- ld == k and k % 8 == 0, rows back to back.
 *        TILE, 16-bit: _TILE2 -- k % 8 == 0, ld % 8 == 0, both pointers 16-byte aligned (two tiles per thread); _SPAN -- not _TILE2,
 *        ld == k, k <= 4096, both pointers 16-byte aligned: 8 .. 64 rows per workgroup through LDS (*span_rows, chosen by how the tile
 *        count fills the workgroup; span_rows may be NULL); _ELEMENT_VEC -- both pointers 8-byte aligned and ld % 4 == 0;
 *        _ELEMENT_SCALAR -- everything else.  TILE, fp32: _ELEMENT_VEC (16-byte aligned, ld % 4 == 0) or _ELEMENT_SCALAR.
 *      sm_compress24_form (SM_COMPRESS24_FORM_*): _FLAT -- A 16-byte aligned, ld == k, k % 64 == 0, strideA a multiple of 16 bytes,
 *        batches back to back (strideA == m * ld or batch == 1); _ROWSPAN -- 16-bit only, not _FLAT: A 16-byte aligned, batches back
 *        to back (strideA == m * ld or batch == 1), 32 * ld * 2 + 32 <= 48 KiB (ld <= 767), any ld >= k (nothing behind the last
 *        logical element, (M - 1) * ld + k, is read); _GENERAL_VEC (A 16-byte aligned, ld and strideA multiples of 16 bytes) / _GENERAL_SCALAR -- everything else.
 *      sm_decompress24_form (SM_DECOMPRESS24_FORM_*): _VEC (A 16-byte aligned, ld and strideA multiples of 16 bytes) / _SCALAR.
 *      sm_prune24_compress24_form (SM_PRUNE24_COMPRESS24_FORM_*): the one-pass kernel is taken when k % 64 == 0, ld and strideA are
 *        multiples of 16 bytes and A_in and a non-null A_out are 16-byte aligned: _ONEPASS_TILE, _ONEPASS_TILE_NOBLOB (16-bit, TILE,
 *        blob == NULL: the blob's re-selection compiled out) or _ONEPASS_STRIP; plan[0] = 1 for the FLAT instantiation (batch == 1, or
 *        batches back to back with m % 4 == 0), plan[1] = lpr_log2 (3 .. 6: lanes along k per tile row, the largest power of two
 *        <= 64 dividing k / 8), plan[2] = nj (passes per row, k / 8 >> lpr_log2), plan[3] = the grid, plan[4] = 1 when the grid was
 *        capped at 8 workgroups per compute unit (`cus`; 0: the current device's, 256 when none is visible; any other value makes the
 *        call host-only).  Otherwise the three launches: _FALLBACK_TALL_SPAN (16-bit TILE with A_out, the batch one tall matrix --
 *        batch == 1, or batches back to back and m % 4 == 0 -- that sm_prune24's span form takes: prune and flag in one pass),
 *        _FALLBACK_TALL (the batch as one tall matrix: back to back, and STRIP or m % 4 == 0), _FALLBACK_PER_BATCH (a prune and a
 *        check launch per batch matrix, at A + b * strideA); plan[5] = matrices the prune and check loops run over.  _NOT_SUPPORTED:
 *        TILE + blob without A_out off the one-pass kernel; the entry point returns SM_STATUS_NOT_SUPPORTED before anything -- the
 *        flag word included -- is touched.  plan: >= 6 unsigned, or NULL. */
#define SM_PRUNE24_FORM_INVALID 0
#define SM_PRUNE24_FORM_EMPTY 1
#define SM_PRUNE24_FORM_STRIP_SCALAR 2       /* prune_strip_kernel / prune_check_kernel, element accesses                */
#define SM_PRUNE24_FORM_STRIP_VEC 3          /* ... 16-byte accesses                                                      */
#define SM_PRUNE24_FORM_STRIP_FLAT_SCALAR 4  /* ... rows back to back, element accesses                                   */
#define SM_PRUNE24_FORM_STRIP_FLAT_VEC 5     /* ... rows back to back, 16-byte accesses                                   */
#define SM_PRUNE24_FORM_TILE2 6              /* prune_tile2_kernel                                                        */
#define SM_PRUNE24_FORM_SPAN 7               /* prune_tile_span_kernel                                                    */
#define SM_PRUNE24_FORM_ELEMENT_SCALAR 8     /* prune_tile_kernel, element accesses                                       */
#define SM_PRUNE24_FORM_ELEMENT_VEC 9        /* prune_tile_kernel, one 8-byte (16-bit) / 16-byte (fp32) access per tile row */
#define SM_COMPRESS24_FORM_INVALID 0
#define SM_COMPRESS24_FORM_EMPTY 1
#define SM_COMPRESS24_FORM_FLAT 2            /* compress_flat_kernel                                                      */
#define SM_COMPRESS24_FORM_ROWSPAN 3         /* compress_rowspan_f16_kernel                                               */
#define SM_COMPRESS24_FORM_GENERAL_SCALAR 4  /* compress_kernel, element loads                                            */
#define SM_COMPRESS24_FORM_GENERAL_VEC 5     /* compress_kernel, 16-byte loads                                            */
#define SM_DECOMPRESS24_FORM_INVALID 0
#define SM_DECOMPRESS24_FORM_EMPTY 1
#define SM_DECOMPRESS24_FORM_SCALAR 2
#define SM_DECOMPRESS24_FORM_VEC 3
#define SM_PRUNE24_COMPRESS24_FORM_INVALID 0
#define SM_PRUNE24_COMPRESS24_FORM_EMPTY 1
#define SM_PRUNE24_COMPRESS24_FORM_NOT_SUPPORTED 2
#define SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL_SPAN 3
#define SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL 4
#define SM_PRUNE24_COMPRESS24_FORM_FALLBACK_PER_BATCH 5
#define SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE 6
#define SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE_NOBLOB 7
#define SM_PRUNE24_COMPRESS24_FORM_ONEPASS_STRIP 8
int sm_prune24_form(const void* A_in, const void* A_out, size_t m, size_t k, size_t ld, size_t elt_bytes, int alg, int* form,
                    unsigned* span_rows);
int sm_prune24_check_form(const void* A, const void* d_valid, size_t m, size_t k, size_t ld, size_t elt_bytes, int* form);
int sm_compress24_form(const void* A, const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, size_t elt_bytes,
                       int* form);
int sm_decompress24_form(const void* blob, const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, size_t elt_bytes,
                         int* form);
int sm_prune24_compress24_form(const void* A_in, const void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                               const void* blob, size_t elt_bytes, int alg, size_t cus, int* form, unsigned* plan);

/* ---- (a2 + a4 without a blob, rounds 4 + 6) the whole call sequence of sparsifyme::spmma() (spmma.hxx:82-113: prune TILE in place,
 *      check, compress, multiply) with NO compressed blob: reads A_in, writes the pruned operand to A_out (A_in itself: in place, what
 *      the reference does; or a second buffer), raises *d_valid (NULL: not wanted; 0 iff every strip written holds <= 2 non-zeros,
 *      derived from the stored values) and computes C_b = alpha * prune24(A_b) * B_b + beta * C_b.  A_out is bit-identical to
 *      sm_prune24_*(A_in, alg) (per batch matrix when m % 4 != 0), C to sm_spmma_*(sm_compress24_*(A_out)).
 *      ONE kernel (A read once, written once) for n <= 128, n % 8 == 0, k % 64 == 0, m % 4 == 0 and 16-byte aligned rows.  Since round 6
 *      every other shape the EXACT fused kernels take -- n > 128 (k % 64 == 0, n % 8 == 0, 16-byte aligned rows), ragged k with
 *      n <= 128 on one contiguous A with a shared B (the span form), m % 4 != 0 -- runs as TWO launches inside the call: the prune + flag
 *      pass over A (sm_prune24_compress24_* with a null blob) and sm_spmma_fused_* on the pruned operand (its STRIP selection of a 2:4
 *      strip is what sm_compress24 stores for it); HBM bytes 2 A + C + B while the pruned A stays in the 256 MiB Infinity Cache between
 *      the two.  SM_STATUS_NOT_SUPPORTED -- decided BEFORE A is touched -- otherwise (n % 8 != 0, n < 8, unaligned operands): then
 *      sm_prune24_compress24_* + sm_spmma_*.  Any other failing status of the second launch (a refused LDS opt-in, a grid limit) is
 *      returned after A_out has been written. */
int sm_prune24_spmma_f16(const void* A_in, void* A_out, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda,
                         size_t batch, size_t strideA, size_t strideB, size_t strideC, int alg, int* d_valid, float alpha,
                         float beta, sm_stream_t stream);
int sm_prune24_spmma_bf16(const void* A_in, void* A_out, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda,
                          size_t batch, size_t strideA, size_t strideB, size_t strideC, int alg, int* d_valid, float alpha,
                          float beta, sm_stream_t stream);

/* ---- (a4) 2:4 sparse x dense matmul: replaces cusparseLtMatmul (spmma.hxx:112-113).
 *      C_b = alpha * A_b * B_b + beta * C_b, row-major, ld(B) = ld(C) = n (spmma.hxx:56-64);
 *      B_b = B + b*strideB (strideB = 0: one shared B), C_b = C + b*strideC (elements).
 *      fp16: v_smfmac_f32_16x16x64_f16, fp32 accumulate, one rounding to fp16. */
int sm_spmma_f16(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k,
                 size_t batch, size_t strideB, size_t strideC, float alpha, float beta,
                 sm_stream_t stream);
int sm_spmma_f32(const void* blob, const float* B, float* C, size_t m, size_t n, size_t k,
                 size_t batch, size_t strideB, size_t strideC, float alpha, float beta,
                 sm_stream_t stream);

/* ---- (f-1) fused prune -> compress -> matmul: C_b = alpha * prune24_strip(A_b) * B_b + beta * C_b from the
 *      DENSE row-major A (m x k, lda, batch stride strideA) without materialising the compressed blob the
 *      reference rebuilds on every call (spmma.hxx:100-113).  Bit-identical to
 *      sm_compress24_f16 + sm_spmma_f16.  Takes k % 64 == 0, n % 8 == 0 and 16-byte aligned rows; or (round 3, the span
 *      form) any k with n % 8 == 0, n <= 128, lda == k, the batches one contiguous tall matrix that ends on a 16-byte
 *      boundary and whose 128-row span + B fit the LDS (k = 147, the ResNets' stem layer); or (round 5, the THIN form) n < 8 with
 *      k <= 64, lda == k, the batches one contiguous tall matrix of a multiple of 16 bytes with a shared B -- the depthwise
 *      convolutions of MobileNet-type networks as im2col products (n = 1, k = 9 / 25) -- computed on the vector ALUs: that form is
 *      inside the tight bound of the exact product (one rounding + k fp32 accumulation steps) but NOT bit-identical to the staged
 *      pair, whose matrix instruction adds the same products in another order.  Returns SM_STATUS_NOT_SUPPORTED otherwise (use
 *      the staged pair). */
int sm_spmma_fused_f16(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda,
                       size_t batch, size_t strideA, size_t strideB, size_t strideC, float alpha,
                       float beta, sm_stream_t stream);

/* The matmul step on `count` same-shape compressed operands as ONE grid per 8 (extension, round 4): host arrays of device
 * pointers blobs[i], B[i], C[i]; the same kernels and the same C, bit for bit, as `count` calls of sm_spmma_f16.  What the
 * grouped form buys is the same as for the fused kernels below: a few-tile layer shape's last partial round of workgroups is
 * filled by the next instance of that shape. */
int sm_spmma_f16_grouped(size_t count, const void* const* blobs, const void* const* B, void* const* C, size_t m, size_t n, size_t k,
                         size_t batch, size_t strideB, size_t strideC, float alpha, float beta, sm_stream_t stream);
int sm_spmma_bf16_grouped(size_t count, const void* const* blobs, const void* const* B, void* const* C, size_t m, size_t n, size_t k,
                          size_t batch, size_t strideB, size_t strideC, float alpha, float beta, sm_stream_t stream);

/* Grouped form (extension; round 3): `count` same-shape problems -- host arrays of device pointers A[i], B[i], C[i], the way
 * the reference's batched::spmm takes its As / Cs (spmm.hxx:30-33) -- in one grid per 8 problems instead of one per problem:
 * the 3-6 instances of one layer shape in a network then share the chip (the last partial round of one instance is filled by
 * the next).  Same kernels and the same C, bit for bit, as `count` calls of sm_spmma_fused_f16; C operands 16-byte aligned. */
int sm_spmma_fused_f16_grouped(size_t count, const void* const* A, const void* const* B, void* const* C, size_t m, size_t n,
                               size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                               float alpha, float beta, sm_stream_t stream);
int sm_spmma_fused_bf16_grouped(size_t count, const void* const* A, const void* const* B, void* const* C, size_t m, size_t n,
                                size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                                float alpha, float beta, sm_stream_t stream);

/* The fused entry points with a WORKSPACE (extension, round 5): the library may then run the STREAM-K form of the fused kernel on
 * the shapes whose rounds of whole 256 x 256 tiles leave compute units idle (few row tiles, long K: 196 x 512 x 4608, 784 x 512 x 1024
 * at batch 32): the launch's 64-deep stage units are cut into one equal contiguous range per compute unit, a tile that lies inside one
 * range is computed and stored exactly as without a workspace (bit-identical), a tile cut by range borders is the sum of fp32 partial
 * sums added IN A FIXED ORDER (ascending k) by the workgroup that holds its first stages -- no atomics on data: repeated runs give
 * the same bits, and the result differs from the no-workspace result only in the order of those few fp32 additions (both within the
 * fp32-accumulation bound of the exact product).  Every other shape runs exactly as sm_spmma_fused_* does.
 * workspace: sm_spmma_fused_workspace_size bytes (4 KiB of flags + one 256 KiB slot per compute unit), 16-byte aligned, its first 4 KiB
 * ZERO before the first call; every call leaves them zero again (hipGraph replays need no memset; a non-zero word 1023 afterwards
 * means a fix-up wait gave up after ~0.3 s and the result is invalid -- it cannot happen with a zeroed flag page and one call at a time per workspace).  Calls that may run concurrently
 * (different streams) need a workspace each; the grouped form's launches share one.  Nothing is allocated or synchronised inside. */
int sm_spmma_fused_workspace_size(size_t* bytes);
/* State of a workspace's flag page after the stream has drained (blocks on `stream`; a 4 KiB read-back -- outside timed regions):
 * *state = 0 clean; 1 a fix-up timed out (word 1023 set: that launch's C is invalid and a late flag may still be raised); 2 flags raised
 * without a recorded timeout (a launch still running, or a page that was never zeroed).  After 1 or 2: zero the first 4096 bytes
 * (hipMemsetAsync) before the next call on this workspace -- a dirty page makes the next launch add a stale partial, silently. */
int sm_spmma_fused_workspace_state(const void* workspace, int* state, sm_stream_t stream);
/* What the workspace entry points do with `problems` same-shape problems of `rows` x n x k (rows = m * batch when the batches share B
 * and are stacked): *takes = 1 when they run the stream-K form, and the decomposition in plan[0 .. 24]: tg, wg, groups_full, tgl,
 * wgl, slots, longest slot range (stage units), cut[0 .. 8], cutl[0 .. 8] -- row panels (256 rows of a problem, in problem order) x
 * k / 64 stage units, groups of tg panels cut into wg slot ranges at cut[] (the last group: tgl panels, wgl slots, cutl[]); a tile
 * that lies inside one slot range is bit-identical to the no-workspace result.  For tests, bench.py and schedulers; no device work.
 * Answered for beta == 0 and a 16-byte aligned C with strideC % 8 == 0 (what the dispatch's A-stationary exception for n > 256,
 * k <= 512 requires): with another beta / C alignment those shapes may run stream-K although *takes = 0 here.  plan: >= 25 unsigned. */
int sm_spmma_fused_streamk_plan(size_t rows, size_t n, size_t k, size_t problems, int* takes, unsigned* plan);
/* WHICH FORM of the fused kernel a launch runs: the dispatch rule of sm_spmma_fused_{f16,bf16} and their _grouped / _ws / _ex forms as
 * a host-side query -- the one function the entry points themselves switch on, so the answer is what launches.  For tests (a test
 * named for a form asserts that its shape reaches it), bench.py-type tools and schedulers; no device work.
 *   m, n, k, lda, batch, strideA, strideB, strideC, beta: as passed to the entry point; count: the problems of ONE launch (1 for the
 *   plain entry points; the grouped ones launch 8 problems at a time, so 1 .. 8; 0: nothing to do).
 *   flags: SM_FUSED_FLAG_A_ALIGNED / _B_ALIGNED / _C_ALIGNED -- every problem's A / B / C starts on a 16-byte boundary (B and C are
 *   at least element-aligned); _WORKSPACE -- the _ws entry points with a 16-byte aligned workspace of sm_spmma_fused_workspace_size
 *   bytes; _EPILOGUE -- the _ex entry points with an epilogue that is not the plain one (a bias, an activation or a residual other
 *   than D), its residual -- where read, beta != 0 -- laid out like D: aligned as C is, strideR == strideD.  (_WORKSPACE and
 *   _EPILOGUE together: no entry point takes both.)
 *   cus: the compute units the rule is asked for (several choices compare how well tile counts fill the chip's rounds); 0: the
 *   current device's (256 when none is visible).  Any other value makes the call host-only.
 * *form: SM_FUSED_FORM_NOT_TAKEN -- the entry point returns SM_STATUS_NOT_SUPPORTED; _EMPTY -- success, nothing launched (a zero
 * extent or count); else the kernel family.  Every form but _THIN is bit-identical to sm_compress24 + sm_spmma.
 * Status: SM_STATUS_INVALID_VALUE for form == NULL, lda < k, count > 8, an unknown flag or _WORKSPACE with _EPILOGUE. */
#define SM_FUSED_FORM_NOT_TAKEN 0
#define SM_FUSED_FORM_EMPTY 1
#define SM_FUSED_FORM_THIN 2          /* n < 8, k <= 64: vector ALUs (spmma_f16_thin_kernel)                              */
#define SM_FUSED_FORM_SPAN 3          /* ragged k, one tall contiguous A, n <= 128 (spmma_f16_fused_span_kernel)           */
#define SM_FUSED_FORM_STREAMK 4       /* workspace given, few tiles x long K (spmma_f16_fused_sk_kernel)                   */
#define SM_FUSED_FORM_BIG 5           /* n > 128: 256 x 256 tiles (spmma_f16_fused_big_kernel)                             */
#define SM_FUSED_FORM_DIRECT64 6      /* n <= 64 (spmma_f16_fused_direct_kernel, 64 columns)                               */
#define SM_FUSED_FORM_DIRECT128 7     /* n <= 128 with k < 512, n <= 256 with k == 64: 128 columns, plain A loads          */
#define SM_FUSED_FORM_DIRECT128_NT 8  /* n <= 128 with k >= 512: 128 columns, non-temporal A loads                         */
#define SM_FUSED_FORM_ASTAT 9         /* n > 256, k <= 512, beta == 0, aligned C, no epilogue (spmma_f16_fused_astat_kernel) */
#define SM_FUSED_FORM_WIDEP 10        /* n > 128, k <= 1024, no epilogue: persistent wide (spmma_f16_fused_widep_kernel)    */
#define SM_FUSED_FORM_WIDE 11         /* n > 256: one workgroup per 128 x 256 tile (spmma_f16_fused_wide_kernel)           */
#define SM_FUSED_FORM_WIDE_NT 12      /* n <= 256: the same with non-temporal A loads                                      */
#define SM_FUSED_FLAG_A_ALIGNED 1u
#define SM_FUSED_FLAG_B_ALIGNED 2u
#define SM_FUSED_FLAG_C_ALIGNED 4u
#define SM_FUSED_FLAG_WORKSPACE 8u
#define SM_FUSED_FLAG_EPILOGUE 16u
int sm_spmma_fused_form(size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t count, size_t strideA, size_t strideB, size_t strideC,
                        float beta, unsigned flags, size_t cus, int* form);
/* The dense entry points with the same workspace: the dense twin of the stream-K form (the dense GEMM the 2:4 path is measured
 * against gets the tile economy the 2:4 path gets); same workspace contract, same bit-identity statement for uncut tiles. */
int sm_gemm_rowmajor_f16_ws(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                            size_t strideB, size_t strideC, float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_gemm_rowmajor_bf16_ws(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                             size_t strideB, size_t strideC, float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_gemm_batched_f16_ws(const void* const* A_ptrs, const void* const* B_ptrs, void* const* C_ptrs, size_t m, size_t n, size_t k, size_t batch,
                           int transpose_a, int transpose_b, float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_spmma_fused_f16_ws(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                          size_t strideB, size_t strideC, float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_spmma_fused_bf16_ws(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                           size_t strideB, size_t strideC, float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_spmma_fused_f16_grouped_ws(size_t count, const void* const* A, const void* const* B, void* const* C, size_t m, size_t n,
                                  size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                                  float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_spmma_fused_bf16_grouped_ws(size_t count, const void* const* A, const void* const* B, void* const* C, size_t m, size_t n,
                                   size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                                   float alpha, float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);

/* ---- Epilogues of the 16-bit 2:4 matmul (extension): the layer  activation(conv(x) + bias [+ shortcut])  in the matmul's own
 *      store instead of one or two more passes over the output.
 *
 *          D[i][j] = round_to_out( act( alpha * (A_2:4 . B)[i][j] + beta * R[i][j] + bias ) )
 *
 *      Everything between the fp32 accumulator and the final conversion is fp32 (alpha * acc + beta * R evaluated exactly as the
 *      plain entry points evaluate alpha * acc + beta * C; the bias is a separate addition after it); ONE rounding, to nearest
 *      even, to fp16 / bf16 at the end.
 *      R      the shortcut: a 16-bit matrix with the shape, the leading dimension (n) and the batch rule of D, given by its own
 *             pointer and batch stride (elements).  R == D (same pointer, same stride) is allowed: in place, what beta means in
 *             the plain entry points; any other overlap of R and D is undefined.  Not read when beta == 0 (may then be NULL).
 *      bias   fp32 device vector or NULL.  bias_dim = SM_BIAS_COL: n entries, one per output column (the output channel in this
 *             project's layout: A the im2col operand, B the weights); SM_BIAS_ROW: m entries indexed by row % m when batches are
 *             stacked (the rule row_scale follows in the fp8 product: the vendor orientation, sparse weights as A).
 *      act    SM_ACT_NONE; SM_ACT_RELU max(x, 0); SM_ACT_CLIPPED_RELU min(max(x, 0), act_arg) (ReLU6: act_arg = 6);
 *             SM_ACT_LEAKY_RELU x >= 0 ? x : act_arg * x; SM_ACT_HARDSWISH x * min(max(x + 3, 0), 6) * (1/6).  Plain fp32
 *             arithmetic.  NaN in, NaN out for every activation; max(-0, 0) is +0 (ReLU, clipped ReLU and the inner clamp of
 *             hardswish return +0 for every x <= 0 that is not NaN, -0 included; leaky ReLU returns -0 for -0).
 *             GELU / sigmoid are NOT offered here: the device erf / tanh they need would bring an error bound that has to be
 *             measured rather than derived.  SiLU is offered where the layer tables use it -- as the gate of a fused gate/up
 *             projection (datasets/linear_shapes.csv), with its bound derived: sm_linear24_glu_{f16,bf16,fp8} below.
 *      The struct is read during the call (host memory); a NULL struct pointer, or one that says "no bias, SM_ACT_NONE, R == D
 *      (or beta == 0)", IS the plain entry point: same kernels, same bits.
 *      Status, decided before any device work: unknown act / bias_dim, beta != 0 with R == NULL, a non-finite or negative
 *      act_arg for the clipped form: SM_STATUS_INVALID_VALUE; a shape the plain entry point does not take: what it returns.
 *      The calls only enqueue on `stream` (hipGraph-capturable).
 *      sm_spmma_*_ex takes every shape sm_spmma_* takes.  sm_spmma_fused_*_ex takes the EXACT forms of sm_spmma_fused_* (the
 *      shapes of the direct, big, wide, A-stationary and span kernels; with an epilogue the A-stationary and persistent-wide
 *      shapes run the wide kernel, whose store is the shared one: same bits) and is bit-identical to sm_compress24 + sm_spmma_*_ex;
 *      the span form additionally needs a 16-byte aligned R with strideR == m * n when it is read.  The THIN form (n < 8) with a
 *      non-trivial epilogue: SM_STATUS_NOT_SUPPORTED.
 *      Not covered yet (they share the routine and can follow): the grouped and _ws (stream-K) forms, sm_prune24_spmma_*,
 *      sm_conv_spmma_*, fp32, int8 and the fp8 matmuls (sm_spmma_fp8, sm_spmma_fused_fp8; the token-major fp8 layer
 *      sm_linear24_fp8 takes the struct). */
#define SM_BIAS_COL 0
#define SM_BIAS_ROW 1
#define SM_ACT_NONE 0
#define SM_ACT_RELU 1
#define SM_ACT_CLIPPED_RELU 2
#define SM_ACT_LEAKY_RELU 3
#define SM_ACT_HARDSWISH 4
typedef struct {
  const float* bias; /* device, fp32; NULL: none */
  int bias_dim;      /* SM_BIAS_COL / SM_BIAS_ROW */
  int act;           /* SM_ACT_* */
  float act_arg;     /* upper clip (SM_ACT_CLIPPED_RELU) / negative slope (SM_ACT_LEAKY_RELU) */
  const void* R;     /* device, the type of D; NULL allowed when beta == 0 */
  size_t strideR;    /* batch stride of R (elements) */
} sm_epilogue_t;
int sm_spmma_f16_ex(const void* blob, const void* B, void* D, size_t m, size_t n, size_t k, size_t batch, size_t strideB,
                    size_t strideD, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_spmma_bf16_ex(const void* blob, const void* B, void* D, size_t m, size_t n, size_t k, size_t batch, size_t strideB,
                     size_t strideD, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_spmma_fused_f16_ex(const void* A, const void* B, void* D, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                          size_t strideA, size_t strideB, size_t strideD, float alpha, float beta, const sm_epilogue_t* epilogue,
                          sm_stream_t stream);
int sm_spmma_fused_bf16_ex(const void* A, const void* B, void* D, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                           size_t strideA, size_t strideB, size_t strideD, float alpha, float beta, const sm_epilogue_t* epilogue,
                           sm_stream_t stream);

/* ---- 2:4 WEIGHT-sparse linear layer, token-major (extension: the reference has no linear layer; this is the documented case of
 *      the vendor libraries, torch.nn.functional.linear with W[out][in] pruned 2:4 along `in`).
 *
 *          Y[t][o] = round_to_out( act( alpha * sum_i W_2:4[o][i] * X[t][i] + beta * R[t][o] + bias ) )
 *
 *      blob   exactly what sm_compress24_{f16,bf16}(W, m = out_features, k = in_features, ld, batch = 1, ..) or
 *             sm_prune24_compress24_* writes: the weight is compressed once, the activations are fresh on every call.
 *      X      row-major tokens x in_features, leading dimension ldx >= in_features (elements); rows 16-byte aligned.
 *      Y      row-major tokens x out_features, leading dimension ldy >= out_features (elements): a fused QKV or gate/up output
 *             can be written as column slices of one buffer.  Columns at or beyond out_features are not touched.
 *      fp32 accumulation and ONE rounding at the end, the arithmetic of sm_spmma_*_ex: alpha * acc + beta * R, then the bias as an
 *      addition of its own, then the activation.
 *      epilogue  the sm_epilogue_t above, NULL = none, read in Y's coordinates: SM_BIAS_COL = one fp32 per out feature (the
 *             nn.Linear bias), SM_BIAS_ROW = one per token; R has Y's shape and ldy, R == Y is allowed (in place); strideR is ignored
 *             (there is no batch).  With a NULL struct beta != 0 reads Y; with a struct, beta != 0 and R == NULL is invalid.  The
 *             validity rules and the error text are those of sm_spmma_*_ex, checked before the shape.
 *      Forms  tokens <= 16 and out_features <= 16384: the decode form (a pure weight stream: the blob goes straight to registers, the
 *             waves of a workgroup split K and add their fp32 partial tiles in a fixed order); every other call: the tile form, which
 *             walks K in the order of
 *             sm_spmma_* and is bit-identical to sm_transpose(X) + sm_spmma_{f16,bf16}[_ex] + sm_transpose(C).  The decode form adds
 *             its K slices in another order: it agrees within the arithmetic's bound (as the THIN form of sm_spmma_fused_f16), not
 *             bit for bit.  Both forms give the same bits on every run (no atomics, no order that depends on arrival).
 *      Status, decided before any device work: invalid epilogue, null operand, blob not 16-byte aligned, ldx < in_features,
 *      ldy < out_features: SM_STATUS_INVALID_VALUE; in_features % 64 != 0, X rows not 16-byte aligned (pointer, ldx % 8), a
 *      dimension >= 2^31: SM_STATUS_NOT_SUPPORTED; tokens == 0 or out_features == 0: success, nothing enqueued.  Every tokens >= 1
 *      and out_features >= 1 is taken: Y (and R, when read) 8-byte aligned with out_features % 4 == 0 and ldy % 4 == 0 use 8-byte
 *      stores, everything else per-element stores.
 *      Enqueue only: no allocation, no synchronisation, no workspace, no memset node; capturable into a hipGraph.
 *      Not covered: int8 token-major output (fp8: sm_linear24_fp8 below), a batch dimension, in_features % 64 != 0. */
int sm_linear24_f16(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                    size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_bf16(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                     size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);

/* ---- The same layer on fp8 operands (W8A8, extension): the fp8 2:4 blob times fp8 tokens, token-major in and out, one launch.
 *
 *          Y[t][o] = round_to_out( act( s(o,t) * acc(o,t) + beta * R[t][o] + bias ) )
 *          acc(o,t) = sum_i W_2:4[o][i] * X[t][i]         fp32, v_smfmac_f32_16x16x128_<W>_<X>
 *          s(o,t)   = (alpha * w_scale[o]) * x_scale[t]   two fp32 multiplies in this order; a NULL scale is skipped
 *
 *      blob     exactly what sm_compress24_fp8(W, m = out_features, k = in_features, .., batch = 1) or
 *               sm_quantize_compress24_fp8_* writes (sm_compress24_size(out_features, in_features, 1, 1) bytes); fmt_w: its SM_FP8_*.
 *      X        fp8 (fmt_x), row-major tokens x in_features, leading dimension ldx >= in_features (bytes = elements); rows 16-byte
 *               aligned.  What sm_quantize_rows_fp8_* writes, as it is: no transpose.
 *      Y        row-major tokens x out_features, leading dimension ldy >= out_features (elements), of out_type SM_OUT_F32 / SM_OUT_F16 /
 *               SM_OUT_BF16.  Columns at or beyond out_features are not touched.
 *      w_scale  out_features floats (device) or NULL: the row_scale sm_quantize_compress24_fp8_* wrote for W.
 *      x_scale  tokens floats (device) or NULL: the row_scale sm_quantize_rows_fp8_* wrote for X.
 *      s * acc + beta * R is evaluated as sm_spmma_fp8 evaluates (alpha * row_scale[i]) * acc + beta * C; the bias is an addition of its
 *      own after it, then the activation, then ONE rounding to the output type.
 *      epilogue the sm_epilogue_t above, NULL = none, read in Y's coordinates as sm_linear24_{f16,bf16} read it: SM_BIAS_COL = one fp32
 *               per out feature, SM_BIAS_ROW = one per token; R has Y's shape, type and ldy, R == Y is allowed (in place); strideR is
 *               ignored.  With a NULL struct beta != 0 reads Y.  The validity rules and the error text are those of sm_spmma_*_ex,
 *               checked before everything else.
 *      Forms    sm_linear24_fp8_form below is the rule the entry point itself switches on.  The tile forms walk K in the order of
 *               sm_spmma_fp8, one matrix instruction per 128 k, and with x_scale == NULL and no epilogue struct are bit-identical to
 *               sm_spmma_fp8(blob, X, C, m = out_features, n = tokens, k = in_features, .., row_scale = w_scale) + sm_transpose(C).
 *               The decode form (few tokens: a pure weight stream; the waves of a workgroup split K and add their fp32 partial tiles
 *               in a fixed order) agrees within the arithmetic's bound, not bit for bit.  Every form gives the same bits on every run.
 *      Status, decided before any device work, in this order: invalid epilogue: SM_STATUS_INVALID_VALUE; null blob / X / Y, blob not
 *      16-byte aligned, fmt_w / fmt_x not SM_FP8_*, out_type not SM_OUT_*, ldx < in_features, ldy < out_features:
 *      SM_STATUS_INVALID_VALUE; a dimension >= 2^31, a tile
 *      grid beyond 2^31 - 1 workgroups, in_features % 64 != 0, X rows not 16-byte aligned (pointer, ldx % 16):
 *      SM_STATUS_NOT_SUPPORTED; tokens == 0 or out_features == 0: success, nothing enqueued.  Every tokens >= 1 and out_features >= 1
 *      is taken, odd out_features included: Y (and R, when read) aligned to four elements with out_features % 4 == 0 and ldy % 4 == 0
 *      use four-element stores, everything else per-element stores.
 *      Enqueue only: no allocation, no synchronisation, no workspace, no memset node; capturable into a hipGraph.
 *      Not covered: int8, quantising X inside the layer, a batch dimension, in_features % 64 != 0, split-K across workgroups. */
int sm_linear24_fp8(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                    size_t ldy, int fmt_w, int fmt_x, int out_type, float alpha, float beta, const float* w_scale, const float* x_scale,
                    const sm_epilogue_t* epilogue, sm_stream_t stream);
/* The form sm_linear24_fp8 runs for a shape -- the host-side statement of its dispatch rule, the one function the entry point
 * switches on.  cus: the compute units the tile rule is sized for; 0 = the current device's (256 when no device is visible); with
 * cus != 0 the call does no device work at all.
 *   NOT_TAKEN   a shape the entry point answers SM_STATUS_NOT_SUPPORTED to (in_features % 64 != 0, a dimension >= 2^31,
 *               a tile grid beyond 2^31 - 1 workgroups)
 *   EMPTY       tokens == 0 or out_features == 0: nothing is enqueued
 *   DECODE      tokens <= 16 and out_features <= 16384
 *   TILE128 / TILE128x64 / TILE64   out features x tokens per workgroup: the largest tile whose grid still has >= cus workgroups
 *               (128 x 128 needs tokens > 64 as well); 64 x 64 when neither larger tile does.
 * *form receives SM_LINEAR24_FORM_*; SM_STATUS_INVALID_VALUE when form is NULL. */
#define SM_LINEAR24_FORM_NOT_TAKEN 0
#define SM_LINEAR24_FORM_EMPTY 1
#define SM_LINEAR24_FORM_DECODE 2
#define SM_LINEAR24_FORM_TILE64 3
#define SM_LINEAR24_FORM_TILE128x64 4
#define SM_LINEAR24_FORM_TILE128 5
int sm_linear24_fp8_form(size_t tokens, size_t out_features, size_t in_features, size_t cus, int* form);

/* ---- The gated (GLU) form of the token-major layers (extension): a fused gate/up projection and its gate in ONE launch, so that the
 *      [tokens][2 hidden] intermediate is never written.
 *
 *          Y[t][h] = round_to_out( act(g) * u ),   g = s_g * acc(h, t) + bias[h],   u = s_u * acc(hidden + h, t) + bias[hidden + h]
 *
 *      blob     the UNCHANGED output of sm_compress24_*(W, m = 2 * hidden, k = in_features) for W[2 hidden][in]: rows 0 .. hidden-1 the
 *               gate projection, rows hidden .. 2 hidden - 1 the up projection (the concatenation datasets/linear_shapes.csv counts).
 *      X        as in the plain layers.
 *      Y        row-major tokens x hidden, ldy >= hidden (elements), of the plain layer's type (16-bit: X's; fp8: out_type).  Columns at
 *               or beyond hidden are not touched.
 *      bias     2 * hidden fp32 values (device), gate's then up's, or NULL.
 *      w_scale  2 * hidden floats or NULL; x_scale: tokens floats or NULL (fp8 only).
 *      g and u are computed in fp32 by the expression -- and the code -- of the plain layer before its activation, with alpha = 1,
 *      beta = 0: s = 1 (16-bit) or s = w_scale[row] * x_scale[t] (fp8, a NULL scale skipped), the bias as an addition of its own.  Then
 *      a = act(g), y = a * u as one fp32 multiply, ONE rounding to the output type; nothing is contracted from act onward.
 *      act      SM_GLU_ACT_NONE  a = g (bilinear); SM_GLU_ACT_RELU  a = max(g, 0) as SM_ACT_RELU computes it (max(-0, 0) = +0, NaN
 *               propagates); SM_GLU_ACT_SILU, defined to the operation: e = expf(-g) (the device library's, <= 1 ulp), d = 1 + e,
 *               a = g / d (correctly rounded division); when e is +inf (g below about -88.7, -inf included) a = -0.  NaN gives NaN,
 *               +inf gives +inf.  |a - silu(g)| <= 4 * 2^-24 |silu(g)| + 2^-120 (exp 2^-23, add 2^-24, divide 2^-24; the second term
 *               covers the cut to -0, where |silu| < 2.7e-37).  a * u is plain IEEE: 0 * inf = NaN.
 *      Forms    sm_linear24_glu_form(tokens, hidden, in, cus) is BY DEFINITION sm_linear24_fp8_form(tokens, 2 * hidden, in, cus), plus
 *               NOT_TAKEN for hidden > 0x3fffffff: the one function both entry points switch on (the 16-bit layer with cus = 256, fp8
 *               with the device's; cus = 0: the device's).  The kernels are the plain layers' own (gated instantiations): a tile holds
 *               the gate rows and the up rows of the same hidden features, so a lane ends with g and u of the same four outputs; g and
 *               u have the bits the plain layer gives columns h and hidden + h.  The decode limits are carried over, not measured.
 *      Status, decided before any device work, in this order: act not SM_GLU_ACT_*: SM_STATUS_INVALID_VALUE; null blob / X / Y, blob not
 *      16-byte aligned, (fp8: fmt / out_type unknown,) ldx < in_features, ldy < hidden: SM_STATUS_INVALID_VALUE; a dimension >= 2^31,
 *      hidden > 0x3fffffff, a tile grid beyond 2^31 - 1 workgroups: SM_STATUS_NOT_SUPPORTED; in_features % 64 != 0, X rows not 16-byte
 *      aligned: SM_STATUS_NOT_SUPPORTED; tokens == 0 or hidden == 0: success, nothing enqueued.  Every hidden >= 1 is taken, odd hidden
 *      included (the up rows then start at an odd blob row); the four-element store under the plain layer's conditions read on hidden.
 *      Enqueue only: no allocation, no synchronisation, no workspace, no memset node; capturable into a hipGraph; same bits on every run.
 *      Not covered: GELU / GeGLU, an fp8-quantised Y, interleaved gate/up layouts, alpha / beta / residual, a batch dimension. */
#define SM_GLU_ACT_NONE 0 /* bilinear: g * u */
#define SM_GLU_ACT_RELU 1 /* ReGLU:    max(g, 0) * u */
#define SM_GLU_ACT_SILU 2 /* SwiGLU:   g / (1 + exp(-g)) * u */
int sm_linear24_glu_f16(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                        int act, const float* bias, sm_stream_t stream);
int sm_linear24_glu_bf16(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                         int act, const float* bias, sm_stream_t stream);
int sm_linear24_glu_fp8(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                        int fmt_w, int fmt_x, int out_type, int act, const float* w_scale, const float* x_scale, const float* bias,
                        sm_stream_t stream);
int sm_linear24_glu_form(size_t tokens, size_t hidden, size_t in_features, size_t cus, int* form);

/* ---- The GROUPED forms of the token-major layers (extension): `groups` experts of ONE shape behind one launch -- the feed-forward
 *      block of a mixture-of-experts layer, whose per-expert token counts exist only on the device (they are the router's output).
 *
 *          for g in 0 .. groups-1, t in [lo_g, hi_g):   Y[t] = sm_linear24_*( blob of expert g, X[t] )      (plain or gated)
 *
 *      blob     the UNCHANGED output of sm_compress24_* / sm_prune24_compress24_* / sm_quantize_compress24_fp8_* for the stacked weight
 *               W[groups * out_features][in_features] (m = groups * out_features, or m = out_features with batch = groups: the same
 *               bytes).  Gated: W[groups][2 * hidden][in_features], each expert's gate rows followed by its up rows.
 *      X, Y     what the plain layers take: row-major, `tokens` rows, ldx / ldy; the tokens sorted by group.
 *      group_offsets  groups + 1 int32 values in DEVICE memory, read on the device only (the call never copies them to the host, so a
 *               captured graph stays valid when the routing changes).  Group g owns token rows [lo_g, hi_g),
 *               lo_g = clamp(off[g], 0, tokens), hi_g = clamp(off[g + 1], lo_g, tokens).  Whatever the array holds, no byte outside the
 *               `tokens` rows of X and Y (and R) and outside the blob is touched.  Rows of Y no group owns are not written.  Ranges that
 *               overlap because the offsets decrease give unspecified values in the overlap (the kernels hand the overlap to the
 *               earlier group); nothing else is affected.
 *      Per-out-feature vectors (an SM_BIAS_COL bias, w_scale): groups * out_features floats, expert-major; gated: groups * 2 * hidden,
 *      each expert's gate values then its up values.  Per-token vectors (an SM_BIAS_ROW bias, x_scale) and R: in Y's global rows.
 *      Arithmetic: the plain layer's own.  Group g's rows of Y have the bits sm_linear24_* (sm_linear24_glu_*) gives on that slice of
 *      X with expert g's own blob in a TILE form: the same K order, the one rounding, the same epilogue order (the kernels are the
 *      plain layers' tile kernels, GROUPED instantiations).  The same bits on every run.
 *      Forms    sm_linear24_grouped_form(tokens, groups, out_features, in_features, cus) is the one rule every grouped entry point
 *               switches on (16-bit with cus = 256, fp8 with the device's; cus = 0: the device's; gated: asked with
 *               out_features = 2 * hidden).  Never DECODE.  With mean = ceil(tokens / groups):
 *                 TILE128      mean > 64 and ceil(out / 128) * ceil(tokens / 128) >= cus
 *                 TILE128x64   else, when ceil(out / 128) * ceil(tokens / 64) >= cus
 *                 TILE64       else
 *                 NOT_TAKEN / EMPTY as in the statuses below.
 *               The thresholds are the plain rule's, carried over, NOT measured for the grouped launch.  The grid is tiles_m * slots
 *               workgroups, slots = min(tokens, ceil(tokens / BN) + groups - 1): an upper bound on sum_g ceil(count_g / BN) for every
 *               distribution (a non-empty group has ceil(c / BN) = floor((c - 1) / BN) + 1, so n non-empty groups of T tokens in all
 *               need <= floor((T - n) / BN) + n <= ceil(T / BN) + groups - 1 tiles; and ceil(c / BN) <= c).  A workgroup finds its
 *               group by walking group_offsets (scalar loads, at most 2 * groups of them); the real tiles run group by group in the
 *               plain layer's order, and a workgroup beyond the last real tile returns at once.  NOT_TAKEN's grid limit is read on
 *               this product.
 *      Status, decided before any device work, in this order: invalid epilogue (gated: act not SM_GLU_ACT_*): SM_STATUS_INVALID_VALUE;
 *      null blob / X / Y / group_offsets, blob not 16-byte aligned, (fp8: fmt / out_type unknown,) ldx < in_features,
 *      ldy < out_features: SM_STATUS_INVALID_VALUE; a dimension >= 2^31, groups > SM_LINEAR24_MAX_GROUPS, groups * out_features (gated:
 *      groups * 2 * hidden) > 2^31 - 1, a grid beyond 2^31 - 1 workgroups: SM_STATUS_NOT_SUPPORTED; in_features % 64 != 0, X rows not
 *      16-byte aligned: SM_STATUS_NOT_SUPPORTED; tokens == 0, out_features == 0 or groups == 0: success, nothing enqueued.
 *      Enqueue only: no allocation, no synchronisation, no workspace, no memset node; capturable into a hipGraph.
 *      Not covered: a grouped decode form (few tokens per expert run the 64 x 64 tile form: DESIGN.md 8), experts of differing shapes,
 *      an fp8-quantised Y; the plain layers' rules and kernels are unchanged.  (Un-permuted tokens: the _gather forms below; the top-k
 *      combine weight: sm_moe_combine_*.) */
#define SM_LINEAR24_MAX_GROUPS 1024
int sm_linear24_grouped_f16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t out_features,
                            size_t in_features, size_t ldx, size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t out_features,
                             size_t in_features, size_t ldx, size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t out_features,
                            size_t in_features, size_t ldx, size_t ldy, int fmt_w, int fmt_x, int out_type, float alpha, float beta,
                            const float* w_scale, const float* x_scale, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_glu_f16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t hidden,
                                size_t in_features, size_t ldx, size_t ldy, int act, const float* bias, sm_stream_t stream);
int sm_linear24_grouped_glu_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t hidden,
                                 size_t in_features, size_t ldx, size_t ldy, int act, const float* bias, sm_stream_t stream);
int sm_linear24_grouped_glu_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t hidden,
                                size_t in_features, size_t ldx, size_t ldy, int fmt_w, int fmt_x, int out_type, int act, const float* w_scale,
                                const float* x_scale, const float* bias, sm_stream_t stream);
int sm_linear24_grouped_form(size_t tokens, size_t groups, size_t out_features, size_t in_features, size_t cus, int* form);

/* ---- GATHERED X in the grouped layers (extension): the grouped entry points above with `const int* x_index, size_t x_rows` directly
 *      after group_offsets.  X stays in the caller's TOKEN order and is never copied into the sorted order:
 *
 *          row t of Y (a sorted row)  reads  row clamp(x_index[t], 0, x_rows - 1) of X          (X has x_rows rows)
 *
 *      x_index  `tokens` int32 values in DEVICE memory (sm_moe_route's sorted_token), read on the device only, once per workgroup,
 *               ahead of its first load of X.  Whatever the array holds, no byte outside the x_rows rows of X is touched.
 *      fp8      x_scale holds x_rows floats and is read at the same source row: the scale belongs to the token that was quantised.
 *      Y, R and an SM_BIAS_ROW bias stay in Y's sorted rows; group_offsets, the blob, the per-out-feature vectors and `tokens` (the
 *      row count of Y and of x_index) keep their meaning.  Rows no group owns are not written: with sm_moe_route's outputs that is
 *      every row s >= V of a routing with dropped pairs.
 *      Arithmetic: group g's rows are bit for bit what sm_linear24_grouped_* gives on the materialised X' = X[x_index] (the GATHER
 *      instantiations of the same tile kernels; only the source row of the X loads differs).  Form: sm_linear24_grouped_form.
 *      Status: the twin's list in its order; a null x_index or x_rows == 0 belongs to its first SM_STATUS_INVALID_VALUE test,
 *      x_rows >= 2^31 to its dimension test (SM_STATUS_NOT_SUPPORTED).  Enqueue only, capturable, as the twins. */
int sm_linear24_grouped_gather_f16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                   size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha,
                                   float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_gather_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                    size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha,
                                    float beta, const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_gather_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                   size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, int fmt_w,
                                   int fmt_x, int out_type, float alpha, float beta, const float* w_scale, const float* x_scale,
                                   const sm_epilogue_t* epilogue, sm_stream_t stream);
int sm_linear24_grouped_glu_gather_f16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                       size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act,
                                       const float* bias, sm_stream_t stream);
int sm_linear24_grouped_glu_gather_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                        size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act,
                                        const float* bias, sm_stream_t stream);
int sm_linear24_grouped_glu_gather_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                       size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int fmt_w,
                                       int fmt_x, int out_type, int act, const float* w_scale, const float* x_scale, const float* bias,
                                       sm_stream_t stream);

/* ---- MoE routing on the device (extension): from the router's ids to what the grouped layers and sm_moe_combine_* read.
 *      P = tokens * top_k pairs; pair p = t * top_k + j is token t's j-th choice, expert_ids[p] its expert (int32, device).
 *      The result is a STABLE COUNTING SORT of the pairs by expert id -- fully defined, the same integers from every form, every run:
 *        a pair whose id lies outside [0, groups) is DROPPED (padding, an expert of another rank);
 *        group_offsets[g]  (groups + 1 values) the number of kept pairs with id < g; V = group_offsets[groups] kept pairs in all;
 *        sorted_pair[s]    for s in [off[e], off[e + 1]): the (s - off[e])-th pair with id e in ascending p;  -1 for s in [V, P);
 *        sorted_token[s]   sorted_pair[s] / top_k (the x_index of the gathered layers);                       -1 for s in [V, P);
 *        pair_pos[p]       s for a kept pair, -1 for a dropped one (the inverse permutation sm_moe_combine_* reads).
 *      Forms (sm_moe_route_form; the entry point switches on it):
 *        SM_MOE_ROUTE_FORM_SINGLE  P <= SM_MOE_ROUTE_SINGLE_MAX_PAIRS: one launch, the whole sort in one workgroup's LDS; no
 *                                  workspace (size 0, NULL accepted).  The decode case.
 *        SM_MOE_ROUTE_FORM_MULTI   else: per chunk of SM_MOE_ROUTE_CHUNK pairs a histogram, one scan, a stable scatter per chunk
 *                                  (three launches); workspace = ceil(P / SM_MOE_ROUTE_CHUNK) * groups * 4 bytes
 *                                  (sm_moe_route_workspace_size), 4-byte aligned, contents irrelevant on entry.
 *        SM_MOE_ROUTE_FORM_EMPTY   P == 0 or groups == 0;  SM_MOE_ROUTE_FORM_INVALID  P > 2^31 - 1 or groups > SM_LINEAR24_MAX_GROUPS.
 *        The threshold is a choice (what one workgroup's LDS pass holds), NOT measured.
 *      Enqueue only: no allocation, no synchronisation, no memset node (the kernels zero what they count in); capturable into a
 *      hipGraph, and a captured graph stays valid when the ids change.  Nothing outside the four outputs and workspace_bytes of
 *      the workspace is written.
 *      Status, decided before any device work: a null pointer (a null workspace only when the size is non-zero) or
 *      workspace_bytes below the size: SM_STATUS_INVALID_VALUE; P > 2^31 - 1 or groups > SM_LINEAR24_MAX_GROUPS:
 *      SM_STATUS_NOT_SUPPORTED; groups == 0: success, nothing enqueued; tokens == 0 or top_k == 0: the groups + 1 zeros are written,
 *      nothing else.  Not covered: int64 ids, capacity limits that drop overflow tokens. */
#define SM_MOE_ROUTE_FORM_INVALID 0
#define SM_MOE_ROUTE_FORM_EMPTY 1
#define SM_MOE_ROUTE_FORM_SINGLE 2
#define SM_MOE_ROUTE_FORM_MULTI 3
#define SM_MOE_ROUTE_SINGLE_MAX_PAIRS 4096
#define SM_MOE_ROUTE_CHUNK 4096
int sm_moe_route_workspace_size(size_t tokens, size_t top_k, size_t groups, size_t* bytes);
int sm_moe_route(const int* expert_ids, size_t tokens, size_t top_k, size_t groups, int* group_offsets, int* sorted_token, int* sorted_pair,
                 int* pair_pos, void* workspace, size_t workspace_bytes, sm_stream_t stream);
int sm_moe_route_form(size_t tokens, size_t top_k, size_t groups, int* form);

/* ---- MoE combine (extension): the un-permute and the weighted sum over top_k, fp16 / bf16.
 *      Yp[rows_p][hidden] (ldp): one row per routed pair in sorted order (the down projection's output); pair_pos[P], P = tokens * top_k
 *      (sm_moe_route's); weights[P] fp32 in pair order, or NULL; R[tokens][hidden] (ldo) or NULL; out[tokens][hidden] (ldo).
 *      Per output element, all in fp32:  s = R[t][h], or +0 without R;  for j = 0 .. top_k - 1 ascending: pos = pair_pos[t * top_k + j],
 *      the pair is skipped when pos < 0 or pos >= rows_p, else q = w * y (q = y when weights is NULL), s = s + q;  then ONE rounding to
 *      nearest even to the output type.  q = w * y is one fp32 multiply and s = s + q one fp32 add, never contracted into an fma.  A
 *      token with every pair dropped gives R, or +0.  No atomics: the same bits on every run.  R == out is allowed (in place).
 *      Forms (sm_moe_combine_form; the entry points switch on it): SM_MOE_COMBINE_FORM_VEC, 16-byte accesses, when hidden % 8 == 0,
 *      ldp % 8 == 0, ldo % 8 == 0 and Yp, R and out are 16-byte aligned (a NULL R counts as aligned); _SCALAR otherwise; _EMPTY
 *      hidden == 0; _INVALID a null Yp or out, ldp < hidden, ldo < hidden or a dimension >= 2^31.
 *      Status: a null Yp, pair_pos or out, ldp < hidden or ldo < hidden: SM_STATUS_INVALID_VALUE; P or a dimension >= 2^31:
 *      SM_STATUS_NOT_SUPPORTED; tokens, top_k or hidden == 0: success, nothing enqueued.  Enqueue only, capturable.
 *      Not covered: an fp32 Yp, an fp8-quantised out. */
#define SM_MOE_COMBINE_FORM_INVALID 0
#define SM_MOE_COMBINE_FORM_EMPTY 1
#define SM_MOE_COMBINE_FORM_SCALAR 2
#define SM_MOE_COMBINE_FORM_VEC 3
int sm_moe_combine_f16(const void* Yp, const int* pair_pos, const float* weights, const void* R, void* out, size_t tokens, size_t top_k,
                       size_t hidden, size_t rows_p, size_t ldp, size_t ldo, sm_stream_t stream);
int sm_moe_combine_bf16(const void* Yp, const int* pair_pos, const float* weights, const void* R, void* out, size_t tokens, size_t top_k,
                        size_t hidden, size_t rows_p, size_t ldp, size_t ldo, sm_stream_t stream);
int sm_moe_combine_form(const void* Yp, const void* R, const void* out, size_t hidden, size_t ldp, size_t ldo, int* form);

/* ---- MoE gate (extension): the router's logits to top_k expert ids and fp32 weights per token, in one launch; fp16 / bf16 / fp32 logits.
 *      logits[tokens][experts], row pitch ld >= experts in elements, no alignment beyond the element's.  topk_ids (int32) and
 *      topk_weights (fp32) are [tokens][top_k], compact, in pair order p = t * top_k + j: what sm_moe_route reads as expert_ids and
 *      sm_moe_combine_* as weights.  select_bias: `experts` floats in DEVICE memory, or NULL; it takes part in the selection only, never
 *      in the weights (the sigmoid router's correction bias).  x_e is the logit converted exactly to fp32.
 *      Selection key:
 *        without a bias  key_e = x_e  (both scorings are monotone in x: no exp decides an id);
 *        with a bias (SM_MOE_SCORE_SIGMOID only)  q_e = 1 / (1 + expf(-x_e)), key_e = q_e + select_bias[e], one fp32 add;
 *        a NaN key counts as -inf.
 *      Selection: ids[j], j = 0 .. top_k - 1, are the experts in DESCENDING key order, equal keys in ASCENDING expert index.  Whatever
 *      the logits hold, the top_k ids of a token are distinct and in [0, experts).
 *      Weights, all in fp32:
 *        SM_MOE_SCORE_SOFTMAX with renormalize (only top_k exponentials):  m = x_{ids[0]};  e_j = expf(x_{ids[j]} - m);
 *          S = sum_j e_j in ascending j;  w_j = (e_j / S) * scale.
 *        SM_MOE_SCORE_SOFTMAX without renormalize:  m = the maximum over all experts;  S = the sum of expf(x_e - m) over all experts
 *          (its order is not fixed);  e_j and w_j as above.
 *        SM_MOE_SCORE_SIGMOID:  q_j = 1 / (1 + expf(-x_{ids[j]}));  w_j = q_j * scale, or (q_j / sum_j q_j) * scale with renormalize,
 *          the sum in ascending j.
 *        inf and NaN propagate through this arithmetic as IEEE has it: only the ids carry a guarantee.
 *      Forms (sm_moe_gate_form; the entry points switch on it): one wave per token, lane l holds experts l, l + 64, ...;
 *      SM_MOE_GATE_FORM_LANE{1,2,4,8,16} is the number of keys a lane holds, the least of them >= ceil(experts / 64); _EMPTY
 *      tokens == 0 or top_k == 0; _INVALID top_k > experts, experts > SM_LINEAR24_MAX_GROUPS, top_k > SM_MOE_GATE_MAX_TOP_K,
 *      tokens * top_k or tokens >= 2^31.
 *      Enqueue only: no allocation, no workspace, no synchronisation, no memset node; capturable into a hipGraph, and a captured graph
 *      stays valid when the logits change.  Nothing outside the two outputs is written.
 *      Status, decided before any device work, in this order: a null logits, topk_ids or topk_weights, ld < experts, top_k > experts,
 *      scoring not one of the two, or a bias with SM_MOE_SCORE_SOFTMAX: SM_STATUS_INVALID_VALUE; tokens * top_k, tokens * ld or a
 *      dimension >= 2^31, then experts > SM_LINEAR24_MAX_GROUPS, then top_k > SM_MOE_GATE_MAX_TOP_K: SM_STATUS_NOT_SUPPORTED (the text
 *      names the limit); tokens == 0 or top_k == 0: success, nothing enqueued.
 *      Not covered: group-limited selection, the router projection that produces the logits. */
#define SM_MOE_SCORE_SOFTMAX 0
#define SM_MOE_SCORE_SIGMOID 1
#define SM_MOE_GATE_MAX_TOP_K 32
#define SM_MOE_GATE_FORM_INVALID 0
#define SM_MOE_GATE_FORM_EMPTY 1
#define SM_MOE_GATE_FORM_LANE1 2
#define SM_MOE_GATE_FORM_LANE2 3
#define SM_MOE_GATE_FORM_LANE4 4
#define SM_MOE_GATE_FORM_LANE8 5
#define SM_MOE_GATE_FORM_LANE16 6
int sm_moe_gate_f16(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts,
                    size_t top_k, size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream);
int sm_moe_gate_bf16(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts,
                     size_t top_k, size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream);
int sm_moe_gate_f32(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts,
                    size_t top_k, size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream);
int sm_moe_gate_form(size_t tokens, size_t experts, size_t top_k, int* form);

/* ---- Residual add + RMSNorm (extension): the pre-norm in front of every layer, in one launch; fp16 / bf16, optional per-token fp8 output.
 *      H[tokens][hidden] (row pitch ldh, in elements) is the residual stream; D (ldd) the branch output to add, or NULL; gamma[hidden] the
 *      weight in the same 16-bit type, or NULL (= 1); res_out (pitch ldh) receives the updated stream, or NULL; N (ldn) the normalised
 *      16-bit output, or NULL; Q (row pitch ldq in bytes) with row_scale[tokens] the fp8 output in fmt (SM_FP8_E4M3 / SM_FP8_E5M2), or
 *      both NULL.  At least one of N and Q is given.
 *      Definition, per row, all in fp32:
 *        h_j = rne16(fp32(H_j) + fp32(D_j)): one fp32 add, one rounding to nearest even to the 16-bit type; without D, h_j = H_j
 *          unchanged.  This is what res_out receives, and everything below reads these ROUNDED values: the fused call is the composition
 *          of its parts.
 *        S = sum_j fp32(h_j)^2.  The order is not fixed by the definition; it is fixed per `hidden` by the kernel (the same bits on
 *          every run, whatever rows ride along).
 *        ms = S / fp32(hidden), one correctly rounded fp32 division.
 *        r = 1 / sqrtf(ms + eps): the add, the correctly rounded square root and the correctly rounded division are three separate
 *          operations; no rsq approximation.
 *        n_j = rne16((fp32(h_j) * r) * fp32(gamma_j)): two fp32 multiplies in this order, one rounding; without gamma one multiply.
 *        Q, row_scale: exactly the rule of sm_quantize_rows_fp8_* (below) applied to the rounded n_j -- amax over the finite elements
 *          with the 2^-100 floor, the two divisions, one multiply, rne to fmt, the non-finite bytes -- whether or not N is written.
 *        NaN and inf go through this arithmetic as IEEE has it: an inf in a row gives r = 0, hence zeros and NaN at the inf; an all-zero
 *          row with eps = 0 gives NaN.
 *      Aliasing allowed: res_out == H (the usual in-place update); N == D; N == H when res_out is NULL or == H (at equal pitches).  A
 *      lane reads every element it owns before it stores any.  Q and row_scale alias nothing.
 *      Forms (sm_rmsnorm_form; the entry points switch on it; a function of `hidden` only, so a row's bits do not depend on how many
 *      rows ride with it): SM_RMSNORM_FORM_LANES, hidden <= SM_RMSNORM_LANES_MAX_HIDDEN: 2^L lanes (8 .. 64) of one wave own a row, a wave
 *      holds several rows when hidden is short; _BLOCK: one 256-thread workgroup per row, the reductions cross waves through LDS;
 *      _EMPTY hidden == 0; _INVALID hidden > SM_RMSNORM_MAX_HIDDEN or hidden % 8 != 0.  Every row is read once and every output written
 *      once.  Enqueue only: no allocation, no workspace, no atomics, no memset node, no synchronisation; capturable into a hipGraph.
 *      Nothing outside the outputs is written.
 *      Status, decided before any device work, in this order: a null H, N and Q both null, exactly one of Q / row_scale null, Q with a
 *      fmt that is not SM_FP8_*, ldh, ldd (with D), ldn (with N) or ldq (with Q) below hidden, eps negative or NaN, or an aliasing not
 *      listed above (N == H with a distinct res_out, res_out == D, res_out == N, aliased operands at different pitches):
 *      SM_STATUS_INVALID_VALUE; then tokens, hidden or a pitch >= 2^31, then hidden > SM_RMSNORM_MAX_HIDDEN, then hidden % 8 != 0, then
 *      a 16-bit operand whose rows are not 16-byte aligned (pointer, pitch % 8): SM_STATUS_NOT_SUPPORTED (the text names the limit);
 *      tokens == 0 or hidden == 0: success, nothing enqueued.
 *      Not covered: LayerNorm, a 1 + gamma weight, an fp32 gamma, fp32 activations, hidden > 16384, the 2:4 compress of the output. */
#define SM_RMSNORM_MAX_HIDDEN 16384
#define SM_RMSNORM_LANES_MAX_HIDDEN 512
#define SM_RMSNORM_FORM_INVALID 0
#define SM_RMSNORM_FORM_EMPTY 1
#define SM_RMSNORM_FORM_LANES 2
#define SM_RMSNORM_FORM_BLOCK 3
int sm_rmsnorm_f16(const void* H, const void* D, const void* gamma, void* res_out, void* N, void* Q, float* row_scale, size_t tokens,
                   size_t hidden, size_t ldh, size_t ldd, size_t ldn, size_t ldq, float eps, int fmt, sm_stream_t stream);
int sm_rmsnorm_bf16(const void* H, const void* D, const void* gamma, void* res_out, void* N, void* Q, float* row_scale, size_t tokens,
                    size_t hidden, size_t ldh, size_t ldd, size_t ldn, size_t ldq, float eps, int fmt, sm_stream_t stream);
int sm_rmsnorm_form(size_t hidden, int* form);

/* ---- Paged-KV decode attention (extension): one query token per sequence over a paged KV cache, grouped query heads (GQA), the
 *      context split into chunks; fp16 / bf16.  All pitches are in elements.
 *      Q[seqs][q_heads][head_dim], row pitch ldq >= q_heads * head_dim (a column slice of a fused QKV projection's output, used as it
 *      is).  Kc and Vc are each [num_pages][page_size][kv_heads][head_dim]: token pitch ldkv >= kv_heads * head_dim, page pitch
 *      page_stride >= page_size * ldkv (token-major inside a page: appending a token is one row of the QKV projection).
 *      block_table[seqs][max_pages] (int32, DEVICE memory, pitch ldbt) and seq_lens[seqs] (int32, DEVICE memory).  O[seqs][q_heads]
 *      [head_dim], pitch ldo.  lse[seqs][q_heads] fp32, compact, or NULL.  Query head h reads KV head h / (q_heads / kv_heads).
 *      Definition, per (sequence s, query head h), all in fp32:
 *        L = clamp(seq_lens[s], 0, max_pages * page_size).  Token t < L lives in page block_table[s][t / page_size], slot
 *          t % page_size.  A page id outside [0, num_pages) makes that page's tokens ABSENT: they take no part in the maximum, the sum
 *          or the product, and no address is ever formed from such an id.  Table entries at or beyond ceil(L / page_size) are never
 *          read.  Slots at or beyond L in the last page take no part: they are masked by selection, not by a multiply (the cache may
 *          hold NaN there), and they are never loaded.
 *        s_t = scale * sum_d fp32(q_d) * fp32(k_t,d).  The order of the sum is not fixed by the definition.
 *        The context is cut into chunks of SM_ATTN_DECODE_CHUNK tokens (a multiple of every allowed page_size); chunk c holds tokens
 *          c * CHUNK .. and yields (m_c, l_c, acc_c) over its present tokens t < L:
 *        m_c = max_t s_t
 *        p_t = rne16(exp2f((s_t - m_c) * log2e)): log2e = 1.44269502f, one fp32 multiply, then exp2f as the hardware's v_exp_f32
 *          evaluates it (1 ulp; exp2f(0) = 1 exactly, and a result below 2^-126 is 0), then one rounding to nearest even to the
 *          operand's 16-bit type
 *        l_c = sum_t fp32(p_t), from the SAME rounded p_t that enter the product: the output is a convex combination of V rows
 *        acc_c,d = sum_t fp32(p_t) * fp32(v_t,d)
 *        A chunk without a present token has m_c = -inf, l_c = 0, acc_c = 0.  The order of the two sums inside a chunk is the
 *          kernel's, a function of the chunk alone.
 *        m = max_c m_c;  w_c = exp2f((m_c - m) * log2e);  l = sum_c w_c * l_c;  acc_d = sum_c w_c * acc_c,d: both sums in ASCENDING c
 *          over the ceil(L / CHUNK) chunks the sequence has.  With one chunk this is that chunk (w = 1).
 *        O_d = rne16(acc_d / l): one correctly rounded fp32 division, then one rounding.  lse = m + logf(l).
 *        L == 0, or every page absent: O = +0 and lse = -inf.
 *        NaN and inf in present tokens go through this arithmetic as IEEE has it (the maximum ignores a NaN); only memory safety
 *          and the masking above are guaranteed then.
 *      The chunk size does not depend on seqs, so a sequence's bits do not depend on which sequences ride along, and two runs on the
 *      same operands give the same bits.
 *      Forms (sm_attn_decode_form; the entry points switch on it): SM_ATTN_DECODE_FORM_DIRECT, max_pages * page_size <=
 *      SM_ATTN_DECODE_CHUNK: one launch, workspace may be NULL; _SPLIT: a partial kernel -- one workgroup per (sequence, kv head,
 *      chunk); one whose chunk starts at or beyond L returns at once -- then a combine kernel: two launches, no atomics, no memset
 *      node; the workspace (sm_attn_decode_workspace_size bytes: seqs * q_heads * ceil(max_pages * page_size / CHUNK) * (head_dim + 2)
 *      * 4; 4-byte aligned) holds acc, m and l per (sequence, query head, chunk), and the combine reads only the ceil(L / CHUNK)
 *      chunks a sequence has, so stale workspace bytes are never read; _EMPTY: seqs == 0 or q_heads == 0; _INVALID: what the entry
 *      points refuse by a limit below, kv_heads == 0 or q_heads % kv_heads != 0.
 *      Limits: head_dim is SM_ATTN_DECODE_MIN_HEAD_DIM (64) or SM_ATTN_DECODE_MAX_HEAD_DIM (128); page_size is a power of two from
 *      SM_ATTN_DECODE_MIN_PAGE_SIZE (16) to SM_ATTN_DECODE_MAX_PAGE_SIZE (128); q_heads % kv_heads == 0 and the group q_heads /
 *      kv_heads <= SM_ATTN_DECODE_MAX_GROUP (16: one 16-row matrix-instruction tile of query rows); max_pages * page_size <=
 *      SM_ATTN_DECODE_MAX_CONTEXT (2^31 - 1); rows of Q, Kc, Vc and O 16-byte aligned (pointer, ldq, ldkv, page_stride, ldo % 8 == 0).
 *      Status, decided before any device work, in this order: a null Q, Kc, Vc, block_table, seq_lens or O; a pitch below its
 *      extent; kv_heads == 0 with q_heads > 0; q_heads % kv_heads != 0; max_pages * page_size > CHUNK with a null, misaligned or short
 *      workspace; scale NaN: SM_STATUS_INVALID_VALUE; then a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or seqs *
 *      q_heads >= 2^31, then the limits above in the listed order: SM_STATUS_NOT_SUPPORTED (the text names the limit); seqs == 0 or
 *      q_heads == 0: success, nothing enqueued.
 *      Enqueue only: no allocation, no synchronisation; capturable into a hipGraph, and a captured graph stays valid when seq_lens
 *      and block_table change on the device.  Nothing outside O, lse and the workspace is written.
 *      Not covered: more than one query token per sequence, a sliding window, soft-capping, ALiBi, an fp8 cache, head dimensions
 *      other than the two, RoPE, the cache append, prefill. */
/* (An fp8 cache is sm_attn_decode_kv8_*, after the append below; RoPE and the cache append are sm_rope_append_*.) */
#define SM_ATTN_DECODE_CHUNK 256
#define SM_ATTN_DECODE_MIN_HEAD_DIM 64
#define SM_ATTN_DECODE_MAX_HEAD_DIM 128
#define SM_ATTN_DECODE_MIN_PAGE_SIZE 16
#define SM_ATTN_DECODE_MAX_PAGE_SIZE 128
#define SM_ATTN_DECODE_MAX_GROUP 16
#define SM_ATTN_DECODE_MAX_CONTEXT 2147483647
#define SM_ATTN_DECODE_FORM_INVALID 0
#define SM_ATTN_DECODE_FORM_EMPTY 1
#define SM_ATTN_DECODE_FORM_DIRECT 2
#define SM_ATTN_DECODE_FORM_SPLIT 3
int sm_attn_decode_f16(const void* Q, const void* Kc, const void* Vc, const int* block_table, const int* seq_lens, void* O, float* lse,
                       void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim,
                       size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t ldbt,
                       size_t ldo, float scale, sm_stream_t stream);
int sm_attn_decode_bf16(const void* Q, const void* Kc, const void* Vc, const int* block_table, const int* seq_lens, void* O, float* lse,
                        void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim,
                        size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t ldbt,
                        size_t ldo, float scale, sm_stream_t stream);
int sm_attn_decode_workspace_size(size_t seqs, size_t q_heads, size_t head_dim, size_t page_size, size_t max_pages, size_t* bytes);
int sm_attn_decode_form(size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t page_size, size_t max_pages, int* form);

/* ---- RoPE + paged KV-cache append (extension): the op between the QKV projection and sm_attn_decode_*, in one launch: rotate every Q
 *      and K head of a token by its row of a cos/sin table, and write K and V into the token's slot of the paged cache; fp16 / bf16.
 *      The same call is the decode step (one token per sequence) and the prefill (all tokens of several sequences).  All pitches are in
 *      elements.
 *      Q[tokens][q_heads][head_dim] (row pitch ldq), K[tokens][kv_heads][head_dim] (ldk) and V (ldv): the three column slices of one
 *      fused QKV output, used as they are.  Qo (ldqo) receives the rotated Q; it may be Q itself, at equal pitch.  Ko (ldko) receives the
 *      rotated K, or is NULL; it may be K itself, at equal pitch (what a framework attention needs at prefill).  Kc / Vc are the cache in
 *      exactly sm_attn_decode_*'s layout, [num_pages][page_size][kv_heads][head_dim] with token pitch ldkv and page pitch page_stride;
 *      both are given, or both are NULL, and with both NULL Ko is required.  cs[max_pos][rot_dim] is an fp32 table (row pitch ldcs): row
 *      p holds cos(p * theta_j) for j < rot_dim / 2, then sin(p * theta_j).  The table is the caller's: linear, NTK, YaRN or llama-3
 *      scaling is a matter of the table, not of this call.  positions[tokens], token_seq[tokens], seq_lens[seqs] and
 *      block_table[seqs][max_pages] (pitch ldbt) are int32 in DEVICE memory.
 *      Definition, per token i:
 *        s_i = token_seq ? token_seq[i] : i.  The NULL case is the decode step: token i is sequence i.
 *        pos_i = positions ? positions[i] : seq_lens[s_i] - 1.  The NULL case is the slot of the token the length already counts: the
 *          host bumps seq_lens, then this call and sm_attn_decode_* read the same array.  seq_lens is read only when 0 <= s_i < seqs;
 *          otherwise pos_i = -1.
 *        A token with pos_i outside [0, max_pos) is a PADDING token: nothing is read from its rows and nothing is written for it -- not
 *          Qo, Ko, Kc or Vc -- and no address is formed from its pos_i.  With rot_dim == 0 there is no table: cs may be NULL, max_pos is
 *          ignored, and a token is padding only when pos_i < 0.
 *        Rotation of every Q head and every K head: half = rot_dim / 2, c_j = cs[pos_i][j], s_j = cs[pos_i][half + j].  SM_ROPE_NEOX
 *          pairs (a, b) = (j, j + half); SM_ROPE_INTERLEAVED pairs (a, b) = (2j, 2j + 1).  All arithmetic is in fp32 and is NOT
 *          contracted:
 *        y_a = rne16(fp32(x_a) * c_j - fp32(x_b) * s_j)
 *        y_b = rne16(fp32(x_b) * c_j + fp32(x_a) * s_j)
 *          Each line is two fp32 multiplies, each rounded, then one fp32 subtract or add, then one rounding to nearest even to the
 *          16-bit type: never an fma.  Elements d >= rot_dim are copied bit for bit.  NaN, inf, -0 and subnormals go through this
 *          arithmetic as IEEE has it; fp32 subnormals are not flushed.
 *        Append: when 0 <= s_i < seqs, pos_i < max_pages * page_size and pg = block_table[s_i][pos_i / page_size] lies in
 *          [0, num_pages), the rotated K goes to Kc[pg][pos_i % page_size] and V goes bit for bit to the same slot of Vc.  Otherwise the
 *          token's Qo / Ko are still written, but the cache is not: no address is formed from an id out of range, and no table entry is
 *          read for a padding token.  The cache offset is 64-bit arithmetic (pg * page_stride exceeds 2^31 on real caches).
 *        Two tokens that name the same slot: either one's row ends up there, whole 16-byte pieces only; memory safe, not an error.
 *      Aliasing allowed: Qo == Q and Ko == K, at equal pitch.  A lane reads both elements of every pair it owns before it stores
 *      either.  Nothing else may alias.
 *      Forms (sm_rope_append_form; the entry points switch on it; the op is elementwise with fixed arithmetic, so both forms give the
 *      same bits): SM_ROPE_APPEND_FORM_BLOCK, tokens <= SM_ROPE_APPEND_BLOCK_MAX_TOKENS: one four-wave workgroup per token, the heads
 *      dealt over its waves (the decode regime); _WAVE: one wave per token, four tokens per workgroup (the prefill regime); _EMPTY:
 *      tokens == 0, q_heads + kv_heads == 0 or head_dim == 0; _INVALID: a head_dim or rot_dim the entry points refuse, a count or
 *      q_heads * head_dim, kv_heads * head_dim >= 2^31.
 *      Limits: head_dim % 8 == 0 and head_dim <= SM_ROPE_APPEND_MAX_HEAD_DIM (256); rot_dim <= head_dim and rot_dim %
 *      SM_ROPE_APPEND_ROT_DIM_MULTIPLE (16) == 0; with a cache, page_size within sm_attn_decode_*'s limits: a power of two from
 *      SM_ATTN_DECODE_MIN_PAGE_SIZE (16) to SM_ATTN_DECODE_MAX_PAGE_SIZE (128); style is SM_ROPE_NEOX or SM_ROPE_INTERLEAVED; rows of
 *      every 16-bit operand 16-byte aligned (pointer and pitches % 8 == 0); rows of cs 16-byte aligned (pointer, ldcs % 4 == 0) when a
 *      table is given.  What is not read is not checked: ldko without Ko; ldkv, page_stride, ldbt, num_pages, page_size and max_pages
 *      without a cache; cs, ldcs and max_pos with rot_dim == 0.
 *      Status, decided before any device work, in this order: a null Q, K, V or Qo; exactly one of Kc / Vc null; Kc null together
 *      with Ko null; a null block_table with a cache; positions and seq_lens both null; cs null with rot_dim > 0; style not one of the
 *      two; a pitch below its extent (ldq, ldqo >= q_heads * head_dim; ldk, ldv, ldko, ldkv >= kv_heads * head_dim; page_stride >=
 *      page_size * ldkv; ldcs >= rot_dim; ldbt >= max_pages); rot_dim > head_dim; token_seq null with tokens > seqs; an aliasing not
 *      listed above (two operands at one address other than Qo == Q and Ko == K, or those at different pitches):
 *      SM_STATUS_INVALID_VALUE; then a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or max_pages * page_size >= 2^31,
 *      then the limits above in the listed order: SM_STATUS_NOT_SUPPORTED (the text names the limit); tokens == 0, q_heads + kv_heads
 *      == 0 or head_dim == 0: success, nothing enqueued.
 *      Enqueue only: no allocation, no workspace, no atomics, no memset node, no synchronisation; capturable into a hipGraph, and a
 *      captured graph stays valid when positions, token_seq, seq_lens and block_table change on the device.  Nothing outside Qo, Ko and
 *      the addressed cache rows is written.
 *      Not covered: an fp8 cache (that is sm_rope_append_kv8_* below), multi-axis (M-RoPE) positions, per-head QK-norm, a 16-bit table, computing the table on the device,
 *      incrementing seq_lens, a cache layout other than sm_attn_decode_*'s. */
#define SM_ROPE_NEOX 0
#define SM_ROPE_INTERLEAVED 1
#define SM_ROPE_APPEND_MAX_HEAD_DIM 256
#define SM_ROPE_APPEND_ROT_DIM_MULTIPLE 16
#define SM_ROPE_APPEND_BLOCK_MAX_TOKENS 32768
#define SM_ROPE_APPEND_FORM_INVALID 0
#define SM_ROPE_APPEND_FORM_EMPTY 1
#define SM_ROPE_APPEND_FORM_BLOCK 2
#define SM_ROPE_APPEND_FORM_WAVE 3
int sm_rope_append_f16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc, void* Vc, const float* cs,
                       const int* positions, const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs,
                       size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size,
                       size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride,
                       size_t ldcs, size_t ldbt, int style, sm_stream_t stream);
int sm_rope_append_bf16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc, void* Vc, const float* cs,
                        const int* positions, const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs,
                        size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size,
                        size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride,
                        size_t ldcs, size_t ldbt, int style, sm_stream_t stream);
int sm_rope_append_form(size_t tokens, size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, int* form);

/* ---- The fp8 paged KV cache (extension): the cache of sm_attn_decode_* and sm_rope_append_* held in OCP fp8 with one fp32 scale per
 *      (token, kv head): half the cache bytes, twice the context in a given cache.  Written by sm_rope_append_kv8_*, read by
 *      sm_attn_decode_kv8_*.
 *      Bytes: Kc8 and Vc8 are fp8 bytes [num_pages][page_size][kv_heads][head_dim], token pitch ldkv, page pitch page_stride, both in
 *      elements (= bytes).  fmt is SM_FP8_E4M3 or SM_FP8_E5M2; one fmt covers both caches.
 *      Scales: Ksc and Vsc are fp32 [num_pages][kv_heads][page_size], page pitch scale_page_stride >= kv_heads * page_size: head-major
 *      inside a page, so that the 16 scales of 16 consecutive tokens of a head are 64 contiguous bytes.
 *      Meaning: element d of the token in (page, slot), kv head g, has the value fp32(byte) * Ksc[page][g][slot] (Vsc for V).
 *      block_table, seq_lens, the page sizes and the ABSENT rule are the 16-bit cache's: a page whose id lies outside [0, num_pages) has
 *      no bytes and no scales read or written, and no address is formed from its id.  head_dim is 64 or 128 in both calls: the reader
 *      accepts nothing else.  Rows are 16-byte aligned: the four pointers, ldkv % 16 == 0, page_stride % 16 == 0, scale_page_stride % 4
 *      == 0.
 *
 *      sm_rope_append_kv8_{f16,bf16}: sm_rope_append_* with the append going to the fp8 cache.  The arguments are sm_rope_append_*'s
 *      with Kc8, Vc8, Ksc, Vsc in the place of Kc, Vc -- all four required: without an fp8 cache the 16-bit call is the one to use --,
 *      scale_page_stride after page_stride and fmt after style.
 *      Definition: everything sm_rope_append_* states about tokens, padding tokens, positions, the rotation, Qo, Ko and aliasing holds
 *      unchanged; Qo and Ko are bit for bit what sm_rope_append_* writes.  Append, under sm_rope_append_*'s condition: let y[g][.] be
 *      the rotated K head g already rounded to the 16-bit type (the bits Ko receives).  The cache receives exactly what
 *      sm_quantize_rows_fp8_* gives for the row y[g][0 .. head_dim): Ksc[pg][g][pos_i % page_size] gets that row's row_scale and
 *      Kc8[pg][pos_i % page_size][g] that row's bytes -- amax = max(max |y| over the finite elements, 2^-100), row_scale = amax / FMAX
 *      and inv = FMAX / amax (two correctly rounded fp32 divisions), byte = rne_fmt(fp32(y) * inv) (one multiply), NaN -> 0x7f, +-inf ->
 *      0x7f (e4m3) / 0x7c | sign (e5m2) by a select on the source bits; an all-zero row has row_scale 2^-100 / FMAX and zero bytes (-0
 *      keeps its sign).  V is handled the same way from the bits of V (no rotation) into Vsc and Vc8.  A refused append (an absent page,
 *      pos_i >= max_pages * page_size, s_i out of range) writes neither bytes nor scales; a padding token writes nothing at all.
 *      Forms: sm_rope_append_form serves this call too (same rule, same threshold, same bits in both forms).
 *      Limits: head_dim is SM_ATTN_DECODE_MIN_HEAD_DIM (64) or SM_ATTN_DECODE_MAX_HEAD_DIM (128); rot_dim, page_size, style and the rows
 *      of Q, K, V, Qo, Ko and cs as in sm_rope_append_*; the rows of the byte and scale arrays as above.  What is not read is not
 *      checked: ldko without Ko; cs, ldcs and max_pos with rot_dim == 0.
 *      Status, decided before any device work, in this order: a null Q, K, V, Qo, Kc8, Vc8, Ksc or Vsc; a null block_table; positions
 *      and seq_lens both null; cs null with rot_dim > 0; style not one of the two; a pitch below its extent (sm_rope_append_*'s list);
 *      fmt not SM_FP8_E4M3 or SM_FP8_E5M2; scale_page_stride < kv_heads * page_size; rot_dim > head_dim; token_seq null with tokens >
 *      seqs; an aliasing other than Qo == Q and Ko == K at equal pitches (among Q, K, V, Qo, Ko, Kc8, Vc8, Ksc, Vsc):
 *      SM_STATUS_INVALID_VALUE; then a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or max_pages * page_size >= 2^31;
 *      head_dim not 64 or 128; rot_dim % SM_ROPE_APPEND_ROT_DIM_MULTIPLE != 0; page_size; the 16-byte rows of Q, K, V, Qo and Ko; the
 *      16-byte rows of Kc8, Vc8, Ksc and Vsc; the 16-byte rows of cs: SM_STATUS_NOT_SUPPORTED (the text names the limit); tokens == 0 or
 *      q_heads + kv_heads == 0: success, nothing enqueued.
 *      Enqueue only: one kernel node, no allocation, no workspace, no atomics, no memset node, no synchronisation; capturable into a
 *      hipGraph, and a captured graph stays valid when positions, token_seq, seq_lens and block_table change on the device.  Nothing
 *      outside Qo, Ko and the addressed cache rows and scales is written.
 *
 *      sm_attn_decode_kv8_{f16,bf16}: sm_attn_decode_* over the fp8 cache.  The arguments are sm_attn_decode_*'s with Ksc, Vsc after Vc8,
 *      scale_page_stride after page_stride and fmt after scale.  Q and O are 16-bit, lse fp32, as there.  The form and the workspace are
 *      functions of the geometry alone: sm_attn_decode_form and sm_attn_decode_workspace_size serve this call too.
 *      Definition: sm_attn_decode_*'s, with two lines changed (k8, v8 the cache bytes, ks_t, vs_t the scales of token t and the head):
 *        s_t = (dot_t * ks_t) * scale, with dot_t = sum_d fp32(q_d) * fp32(k8_t,d) in an order the definition does not fix, then the two
 *          fp32 multiplies in that order
 *        acc_c,d = sum_t (fp32(p_t) * vs_t) * fp32(v8_t,d): one rounded fp32 multiply per token, then the sum
 *        l_c still sums the rounded p_t themselves.
 *      The chunks, the rounding of p, the ascending combine, the masking by selection (the bytes AND the scales of a masked or absent
 *      token are never loaded; the cache may hold NaN bytes and NaN scales there), L == 0, the clamp and the NaN behaviour are as stated
 *      for sm_attn_decode_*.  The widening of a byte to Q's 16-bit type and to fp32 is exact: every e4m3 and e5m2 value is a value of
 *      fp16 and of bf16.
 *      Limits: sm_attn_decode_*'s, with the rows of the byte and scale arrays as above in the place of the rows of Kc and Vc.
 *      Status, decided before any device work, in this order: a null Q, Kc8, Vc8, Ksc, Vsc, block_table, seq_lens or O; a pitch below
 *      its extent; fmt not SM_FP8_E4M3 or SM_FP8_E5M2; scale_page_stride < kv_heads * page_size; kv_heads == 0 with q_heads > 0; q_heads
 *      % kv_heads != 0; max_pages * page_size > CHUNK with a null, misaligned or short workspace; scale NaN: SM_STATUS_INVALID_VALUE;
 *      then a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or seqs * q_heads >= 2^31; head_dim; page_size; the group; the
 *      context; the 16-byte rows of Q and O; the 16-byte rows of Kc8, Vc8, Ksc and Vsc: SM_STATUS_NOT_SUPPORTED (the text names the
 *      limit); seqs == 0 or q_heads == 0: success, nothing enqueued.
 *      Enqueue only, capturable, and a captured graph stays valid when seq_lens and block_table change on the device, as
 *      sm_attn_decode_*.  Nothing outside O, lse and the workspace is written.
 *      Not covered: prefill attention, fp8 Q or P on the 1-byte matrix instruction, per-tensor or calibrated static scales, different
 *      formats for K and V, head dimensions other than the two, converting a 16-bit cache in place. */
int sm_rope_append_kv8_f16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc8, void* Vc8, float* Ksc, float* Vsc,
                           const float* cs, const int* positions, const int* token_seq, const int* seq_lens, const int* block_table,
                           size_t tokens, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos,
                           size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko,
                           size_t ldkv, size_t page_stride, size_t scale_page_stride, size_t ldcs, size_t ldbt, int style, int fmt,
                           sm_stream_t stream);
int sm_rope_append_kv8_bf16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc8, void* Vc8, float* Ksc, float* Vsc,
                            const float* cs, const int* positions, const int* token_seq, const int* seq_lens, const int* block_table,
                            size_t tokens, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos,
                            size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko,
                            size_t ldkv, size_t page_stride, size_t scale_page_stride, size_t ldcs, size_t ldbt, int style, int fmt,
                            sm_stream_t stream);
int sm_attn_decode_kv8_f16(const void* Q, const void* Kc8, const void* Vc8, const float* Ksc, const float* Vsc, const int* block_table,
                           const int* seq_lens, void* O, float* lse, void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads,
                           size_t kv_heads, size_t head_dim, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv,
                           size_t page_stride, size_t scale_page_stride, size_t ldbt, size_t ldo, float scale, int fmt, sm_stream_t stream);
int sm_attn_decode_kv8_bf16(const void* Q, const void* Kc8, const void* Vc8, const float* Ksc, const float* Vsc, const int* block_table,
                            const int* seq_lens, void* O, float* lse, void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads,
                            size_t kv_heads, size_t head_dim, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv,
                            size_t page_stride, size_t scale_page_stride, size_t ldbt, size_t ldo, float scale, int fmt, sm_stream_t stream);

/* fp32 form: the STRIP rule applied to the A fragments in registers of the dense fp32 MFMA kernel (there is no fp32 sparse
 * matrix instruction).  Equals sm_gemm_rowmajor_f32 of the STRIP-pruned A bit for bit; agrees with sm_compress24_f32 +
 * sm_spmma_f32 to fp32 accumulation order.  Needs k % 32 == 0, n % 4 == 0, 16-byte aligned rows. */
int sm_spmma_fused_f32(const float* A, const float* B, float* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                       size_t strideA, size_t strideB, size_t strideC, float alpha, float beta, sm_stream_t stream);

/* fp32 operands on the SPARSE matrix instruction (extension, round 4; csrc/spmma_f32_split.hip): the same product -- the 2:4
 * STRIP selection made on the fp32 values, mask identical to sm_prune24_f32's -- computed by v_smfmac_f32_16x16x64_bf16 on
 * exact bfloat16 splits of both operands (x = x1 + x2 + x3, 8 + 8 + 8 significand bits) with fp32 accumulation:
 *   planes = 3: a1 b1 + a1 b2 + a2 b1 + a2 b2 + a1 b3 + a3 b1     |error| <= 2^-21 * sum |a| |b|  (+ fp32 accumulation)
 *   planes = 2: a1 b1 + a1 b2 + a2 b1                             |error| <= 2^-13 * sum |a| |b|
 * (north_star asks 1e-3 relative for fp32 products; cuSPARSELt, what spmma.hxx:106-114 calls, computes fp32 operands in
 * TF32 = 10 significand bits).  Not bit-identical to sm_spmma_fused_f32 -- which stays the exact form -- and several times
 * faster: bound by the HBM stream of A instead of the fp32 matrix rate.  `workspace` receives B's bfloat16 planes
 * (sm_spmma_fused_f32_split_workspace bytes, 16-byte aligned; a strided B must be packed, strideB == k * n).  Non-finite
 * operand values give NaN in the outputs they reach.  Needs k % 64 == 0, n % 8 == 0, 16-byte aligned rows of A, B and C (ldc = n);
 * a ragged k (the stem layer's 147) runs the span form when n <= 128, lda == k, B is shared and the batches are one tall contiguous
 * A (span + B's planes inside the LDS); everything else: SM_STATUS_NOT_SUPPORTED, use sm_spmma_fused_f32. */
/* sm_gemm_rowmajor_f32_split: the DENSE product C = alpha * A * B + beta * C by the same pieces (v_mfma_f32_16x16x32_bf16, same
 * workspace, same bounds with all of A's elements in the sums) -- the dense comparator the 2:4 split form is held against, and
 * 1.5-2 x faster than the fp32-MFMA sm_gemm_rowmajor_f32 in its own right. */
int sm_spmma_fused_f32_split_workspace(size_t n, size_t k, size_t batch, size_t strideB, int planes, size_t* bytes);
/* B's planes once (round 5): for a B that stays the same across calls (weights), sm_spmma_fused_f32_split_prepare splits it into `workspace`
 * (the same sm_spmma_fused_f32_split_workspace bytes) and sm_spmma_fused_f32_split_prepared multiplies from those planes: the same kernels and the
 * same C bit for bit as sm_spmma_fused_f32_split, without its per-call streaming pass over B. */
int sm_spmma_fused_f32_split_prepare(const float* B, size_t n, size_t k, size_t batch, size_t strideB, int planes, void* workspace, size_t workspace_bytes,
                                     sm_stream_t stream);
int sm_spmma_fused_f32_split_prepared(const float* A, const void* planes_workspace, float* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                                      size_t strideA, size_t strideB, size_t strideC, int planes, size_t workspace_bytes, float alpha, float beta,
                                      sm_stream_t stream);
int sm_spmma_fused_f32_split(const float* A, const float* B, float* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                             size_t strideA, size_t strideB, size_t strideC, int planes, void* workspace, size_t workspace_bytes,
                             float alpha, float beta, sm_stream_t stream);
int sm_gemm_rowmajor_f32_split(const float* A, const float* B, float* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                               size_t strideA, size_t strideB, size_t strideC, int planes, void* workspace, size_t workspace_bytes,
                               float alpha, float beta, sm_stream_t stream);

/* ---- (a5) dense batched GEMM: replaces cublas{H,S,D}gemmBatched (gemm.hxx:80-81, 133-134,
 *      186-187).  COLUMN-major, lda = m, ldb = k, ldc = m as the reference passes them;
 *      A_ptrs/B_ptrs/C_ptrs are device arrays of `batch` device pointers (examples/gemm.cu:65-90).
 *      ta / tb (gemm.hxx:33-34): SM_OP_N or SM_OP_T; a transposed operand is read as its stored k x m
 *      (n x k) form through the same leading dimension, which must cover a stored column (m >= k for
 *      ta = T, k >= n for tb = T; SM_STATUS_INVALID_VALUE otherwise, as the vendor BLAS).
 *      Precondition of every form (f16, f16_ws, f32, f64): every pointer in the arrays is 16-byte aligned (f64: 8-byte; what
 *      hipMalloc returns is).  The arrays live on the device, so the library cannot look at the bases before it picks a
 *      16-byte-chunk pipeline -- the f16 forms choose their 16-byte vector loads, the LDS-DMA kernel and the dense twin of the
 *      fused kernels from m and k alone -- and nothing checks them.
 *      sm_gemm_batched_f16_ws (declared with the other workspace entry points above) is sm_gemm_batched_f16 with the stream-K
 *      workspace of sm_spmma_fused_workspace_size: for non-transposed operands with 128 < m <= 256, m % 8 == 0, k % 64 == 0 and
 *      k >= 2048 it runs the stream-K dense twin where sm_spmma_fused_streamk_plan(n, m, k, batch) takes the launch and the
 *      workspace holds its slots; a null or too small workspace, and every other shape, runs exactly what sm_gemm_batched_f16
 *      runs.  Same workspace contract as sm_spmma_fused_*_ws (the first 4096 bytes zero before a call; they come back zero). */
int sm_gemm_batched_f16(const void* const* A_ptrs, const void* const* B_ptrs, void* const* C_ptrs,
                        size_t m, size_t n, size_t k, size_t batch, int ta, int tb, float alpha,
                        float beta, sm_stream_t stream);
int sm_gemm_batched_f32(const float* const* A_ptrs, const float* const* B_ptrs, float* const* C_ptrs,
                        size_t m, size_t n, size_t k, size_t batch, int ta, int tb, float alpha,
                        float beta, sm_stream_t stream);
int sm_gemm_batched_f64(const double* const* A_ptrs, const double* const* B_ptrs,
                        double* const* C_ptrs, size_t m, size_t n, size_t k, size_t batch, int ta,
                        int tb, double alpha, double beta, sm_stream_t stream);

/* Dense GEMM in the layout sm_spmma_* uses (row-major, strided batch): the like-for-like dense
 * denominator for the 2:4 kernel.  No reference counterpart (the reference's only dense GEMM is
 * the column-major pointer-array one above). */
int sm_gemm_rowmajor_f16(const void* A, const void* B, void* C, size_t m, size_t n, size_t k,
                         size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                         float alpha, float beta, sm_stream_t stream);
int sm_gemm_rowmajor_f32(const float* A, const float* B, float* C, size_t m, size_t n, size_t k,
                         size_t lda, size_t batch, size_t strideA, size_t strideB, size_t strideC,
                         float alpha, float beta, sm_stream_t stream);

/* ---- (a6) unstructured SpMM: replace cusparseSpMM on Blocked-ELL (spmm.hxx:57-67,107-110) and
 *      on strided-batch COO (spmm.hxx:164-187).  Column-major dense operands. */
int sm_spmm_bell_f32(const float* values, const uint64_t* column_indices, size_t rows, size_t cols,
                     size_t block_size, size_t ell_cols, const float* B, float* C, size_t n,
                     float alpha, float beta, sm_stream_t stream);
int sm_spmm_coo_f32(size_t A_num_rows, size_t A_num_cols, size_t A_nnz, size_t B_num_cols,
                    size_t num_batches, const int* rows, const int* cols, const float* vals,
                    const float* B, float* C, float alpha, float beta, sm_stream_t stream);

/* Blocked-ELL with a caller-provided workspace of sm_spmm_bell_workspace_size() bytes (reusable across the
 * batches of one stream): blocks are scattered into a dense A and multiplied on the fp32 matrix cores.
 * workspace == NULL behaves as sm_spmm_bell_f32 (slow gather kernel). */
int sm_spmm_bell_workspace_size(size_t rows, size_t cols, size_t* bytes /*host*/);
int sm_spmm_bell_f32_ws(const float* values, const uint64_t* column_indices, size_t rows, size_t cols,
                        size_t block_size, size_t ell_cols, const float* B, float* C, size_t n,
                        float alpha, float beta, void* workspace, sm_stream_t stream);

/* All batches of the reference's spmm() loop (spmm.hxx:90-101) in one submission: `values`, `column_indices` and `C`
 * are HOST arrays of `batch` device pointers (every A has the same rows/cols/block_size/ell_cols, B is shared --
 * exactly what the reference's driver builds).  Workspace: sm_spmm_bell_batched_workspace_size() bytes, required.
 * NOT hipGraph-capturable, unlike every other entry point: the three pointer tables are copied from the caller's HOST
 * arrays onto the stream (a synchronously staged copy from pageable memory); capture the per-matrix
 * sm_spmm_bell_f32_ws instead, or keep the host arrays alive and unchanged for the lifetime of the graph.
 * (The 16-bit forms below, sm_spmm_bell_batched_{f16,bf16}, pass their tables in the kernel arguments and can be captured.) */
int sm_spmm_bell_batched_workspace_size(size_t rows, size_t cols, size_t batch, size_t* bytes /*host*/);
int sm_spmm_bell_batched_f32(const float* const* values, const uint64_t* const* column_indices, size_t rows,
                             size_t cols, size_t block_size, size_t ell_cols, const float* B, float* const* C,
                             size_t n, size_t batch, float alpha, float beta, void* workspace, sm_stream_t stream);
/* Layout and meaning of the fp32 forms are those stated for the 16-bit forms below (any block_size >= 1, ragged rows and cols, an id >=
 * cols / block_size marks an empty block, whose values are not read).
 * Status: sm_spmm_bell_f32, sm_spmm_bell_f32_ws and sm_spmm_bell_batched_f32 return SM_STATUS_INVALID_VALUE for a null pointer
 * (sm_spmm_bell_batched_f32: a null workspace included), block_size == 0 or ell_cols % block_size != 0; then SM_STATUS_SUCCESS without work
 * when rows, n or batch is 0; then SM_STATUS_NOT_SUPPORTED for n > 8 * 65535 on sm_spmm_bell_f32 (the grid of its gather kernel), for
 * rows, cols or n beyond 2^31-1 on the two workspace forms and for batch > 65535 -- all decided before any HIP call. */

/* Blocked-ELL on the 16-bit matrix cores (fp16 / bfloat16 values, B and C; fp32 accumulation, one rounding of the result):
 * the operand types the reference's descriptors declare (CUDA_R_16F, spmm.hxx:57-67,107-110).  Same layout and meaning as
 * sm_spmm_bell_f32: values [rows][ell_cols] row-major, column_indices [ceil(rows/block_size)][ell_cols/block_size] (an id
 * >= cols/block_size, ~0 included, marks an empty block), B cols x n column-major (ldb = cols), C rows x n column-major
 * (ldc = rows); C is not read when beta == 0.  Any block_size >= 1 with ell_cols % block_size == 0; rows, cols and n need
 * not be multiples of anything.  The blocks are expanded inside the product (in LDS): no workspace, no device allocation, no
 * host synchronisation, deterministic.  A block row that stores its blocks in ascending order (every producer here does)
 * takes the fast path when ell_cols <= 65535 and the per-tile stage table (2 bytes per block row of a 128-row tile and per
 * 64 columns of A) fits in LDS beside the stage buffers: for n > 128, cols up to about 16 000 for block_size 1 and 32 000 for
 * block_size 2 (about 28 000 and 56 000 for n <= 64).
 * Any other order, and any larger shape, takes the generic path: the same C bit for bit, but every 64-column stage walks
 * whole rows of A, a cost that grows with cols * ell_cols.  A block column repeated within one block
 * row gives an unspecified result, as in the fp32 path.
 * The batched forms take HOST arrays of `batch` device pointers (one A and one C per entry, B shared), read during the call
 * and passed in the kernel arguments: the caller may free the arrays as soon as the call returns.
 * Status: SM_STATUS_INVALID_VALUE for a null pointer, block_size == 0 or ell_cols % block_size != 0;
 * SM_STATUS_NOT_SUPPORTED when rows, cols, n or ell_cols exceeds 2^31-1; SM_STATUS_SUCCESS without work when rows, n or
 * batch is 0 -- all decided before any HIP call.  Every one of these four entry points can be captured into a hipGraph. */
int sm_spmm_bell_f16(const void* values, const uint64_t* column_indices, size_t rows, size_t cols,
                     size_t block_size, size_t ell_cols, const void* B, void* C, size_t n,
                     float alpha, float beta, sm_stream_t stream);
int sm_spmm_bell_bf16(const void* values, const uint64_t* column_indices, size_t rows, size_t cols,
                      size_t block_size, size_t ell_cols, const void* B, void* C, size_t n,
                      float alpha, float beta, sm_stream_t stream);
int sm_spmm_bell_batched_f16(const void* const* values, const uint64_t* const* column_indices, size_t rows,
                             size_t cols, size_t block_size, size_t ell_cols, const void* B, void* const* C,
                             size_t n, size_t batch, float alpha, float beta, sm_stream_t stream);
int sm_spmm_bell_batched_bf16(const void* const* values, const uint64_t* const* column_indices, size_t rows,
                              size_t cols, size_t block_size, size_t ell_cols, const void* B, void* const* C,
                              size_t n, size_t batch, float alpha, float beta, sm_stream_t stream);

/* COO with a caller-provided workspace of sm_spmm_coo_workspace_size() bytes (the reference allocates its
 * cuSPARSE buffer inside the call, spmm.hxx:183): row-sorted input runs as CSR, row-parallel, without
 * atomics (bitwise reproducible); unsorted input falls back to the atomic kernel.  workspace == NULL
 * behaves as sm_spmm_coo_f32.
 * Status of the exact COO forms (sm_spmm_coo_f32, _ws, _packed): SM_STATUS_INVALID_VALUE for a null B or C, and for null rows, cols or vals
 * when A_nnz > 0; then SM_STATUS_SUCCESS without work when A_num_rows, B_num_cols or num_batches is 0; then SM_STATUS_NOT_SUPPORTED when
 * B_num_cols * num_batches > 65535 on sm_spmm_coo_f32 (also where another form is called without a workspace it can use), and on
 * sm_spmm_coo_f32_ws when A_nnz exceeds 2^31-1, num_batches exceeds 65535 or B_num_cols exceeds 16 * 65535 -- all decided before any HIP
 * call.  An entry whose row or column is out of range is skipped, never an error. */
int sm_spmm_coo_workspace_size(size_t A_num_rows, size_t* bytes /*host*/);
int sm_spmm_coo_f32_ws(size_t A_num_rows, size_t A_num_cols, size_t A_nnz, size_t B_num_cols,
                       size_t num_batches, const int* rows, const int* cols, const float* vals,
                       const float* B, float* C, float alpha, float beta, void* workspace,
                       sm_stream_t stream);

/* COO, packed form (replaces the same cusparseSpMM call, spmm.hxx:164-187): the rows of A are first copied, on the
 * device and once per call, into one stream of {LDS offset, value} entries padded per row, so that the product kernel
 * (csrc/spmm.hip: spmm_csr_packed_kernel) carries no per-entry predicates, clamps or scattered stores -- the work
 * cusparseSpMM does behind its buffer (spmm.hxx:178-183).  Workspace: sm_spmm_coo_packed_workspace_size(rows, nnz) bytes
 * (16-byte aligned), its size passed back in `workspace_bytes`.  Taken when the rows are sorted (decided on the device,
 * no synchronisation; unsorted input runs the atomic kernels) and (cols + 1) * 64 bytes fit the LDS (cols <= 2559);
 * otherwise, or with
 * a workspace that is too small (then treated as sm_spmm_coo_f32_ws's, or as none), sm_spmm_coo_f32_ws /
 * sm_spmm_coo_f32 produce the same result.  Bitwise reproducible on the sorted path; hipGraph-capturable. */
int sm_spmm_coo_packed_workspace_size(size_t A_num_rows, size_t A_nnz, size_t* bytes /*host*/);
int sm_spmm_coo_f32_packed(size_t A_num_rows, size_t A_num_cols, size_t A_nnz, size_t B_num_cols,
                           size_t num_batches, const int* rows, const int* cols, const float* vals,
                           const float* B, float* C, float alpha, float beta, void* workspace,
                           size_t workspace_bytes, sm_stream_t stream);

/* Dense-MFMA form of the same product (extension; what sparsifyme::batched::strided_coo tries first since round 4, with the exact
 * form as its fallback): the batches' dense operand is scaled by a power of two and rounded once to fp16, A is scattered dense,
 * scaled and split exactly into two fp16 planes, the product runs on the fp16 matrix instruction with fp32 accumulation and the
 * inverse scales are applied to the fp32 sums: 2-3 x faster than the exact forms at 90 % sparsity.
 * Scales (round 4, computed on the device: no synchronisation): 2^x that brings the largest |b| of a ~10^6-element sample of
 * the dense operand (1024 evenly spread runs of 1024 contiguous elements) into [2^12, 2^13) and 2^y that brings the largest |a| into [2^13, 2^14) -- so the error does not
 * depend on the operands' magnitude (1e-6-sized activations or 1e+6-sized ones convert alike).
 * Error: |C - exact| <= 2^-11 * |alpha| * sum|a||b|  (one fp16 rounding of b; 4.9e-4, inside the 1e-3 this build's fp32 products are
 * held to) + fp32 accumulation + 2^-37 * max|b| * |alpha| * sum|a| (elements of the dense operand more than 2^26 below its
 * largest one lose relative precision: they are rounded to a multiple of 2^-37 of the largest).
 * Range flag: the first int of the workspace is set != 0 on the device when an element does NOT convert -- non-finite, or more
 * than 8 x the sampled maximum (|x * scale| > 65504), or duplicates of A adding up beyond the range; the matrix kernel then
 * returns without touching C, so that the caller can run an exact entry point on the untouched operands:
 * sm_spmm_coo_fast_flag() copies the flag to the host (it synchronises the stream), which is what strided_coo does.
 * Duplicates add (in an unspecified order).  Needs A_num_cols % 64 == 0 (> 0), A_num_rows % 4 == 0 (>= 8), 16-byte aligned B and
 * C and sm_spmm_coo_fast_workspace_size bytes of workspace (SM_STATUS_NOT_SUPPORTED when the sizes overflow size_t);
 * SM_STATUS_NOT_SUPPORTED otherwise (use the exact entry points).
 * Round 5 -- the SPARSE matrix instruction for the same call: with beta == 0, A_num_rows % 4 == 0 and at most 20 % of A's entries present
 * (sm_spmm_coo_fast_form says which form a call gets: where both apply, this one for A_num_cols <= 128 and for matrices of at most 256 rows), A becomes a 2:4 image (per 1 x 4 strip its first two non-zeros, scaled and split hi + lo
 * as above; a random 10 %-dense A has a third non-zero in 0.4 % of its strips -- those entries are kept as fp32 values beside the image) and
 * the product runs on v_smfmac_f32_16x16x64_f16 with the dense operand converted inside the kernel's loader: no fp16 copy of B, any
 * A_num_cols (k % 64 != 0, k % 4 != 0 included).  Same error bound.  Flag, this form: A out of range, or a 32 x 64 block of A with more than
 * 64 third / fourth non-zeros -> nothing is written; an element of B out of range -> the 128 x 128 tiles of C that read it are not written, the
 * others are (beta == 0: the exact form overwrites all of C anyway). */
int sm_spmm_coo_fast_form(size_t A_num_rows, size_t A_num_cols, size_t A_nnz, size_t B_num_cols, size_t num_batches, float beta); /* 2: sparse matrix instruction, 1: dense-MFMA pipeline, 0: not taken */
int sm_spmm_coo_fast_workspace_size(size_t A_num_rows, size_t A_num_cols, size_t B_num_cols, size_t num_batches, size_t* bytes /*host*/);
int sm_spmm_coo_fast_flag(const void* workspace, int* host_flag, sm_stream_t stream);
int sm_spmm_coo_f32_fast(size_t A_num_rows, size_t A_num_cols, size_t A_nnz, size_t B_num_cols, size_t num_batches,
                         const int* rows, const int* cols, const float* vals, const float* B, float* C, float alpha,
                         float beta, void* workspace, size_t workspace_bytes, sm_stream_t stream);

/* ---- support: counter-based uniform fill (replaces the Thrust RNG transform of
 *      include/sparsify.me/util/gen.hxx:12-20); element i depends only on (seed, i). */
int sm_fill_uniform_f16(void* out, size_t count, uint64_t seed, float lo, float hi, sm_stream_t stream);
int sm_fill_uniform_f32(float* out, size_t count, uint64_t seed, float lo, float hi, sm_stream_t stream);

/* ---- support: plain streaming device-to-device copy (16-byte accesses; src, dst 16-byte aligned, bytes % 16 == 0).  No
 *      reference counterpart: the bandwidth yardstick bench.py times next to the step (roofline.yardstick), in-process. */
int sm_copy_bytes(const void* src, void* dst, size_t bytes, sm_stream_t stream);

/* ---- transposed operands of sparsifyme::spmma (spmma.hxx:30-31,67-69: transpose_a / transpose_b go to the vendor's matmul
 *      descriptor).  out[b][c * ld_out + r] = in[b][r * ld_in + c] for `batch` row-major rows x cols matrices of 2-, 4- or
 *      8-byte elements (out of place).  include/sparsify.me/spmma.hxx brings a transposed operand to the N form with
 *      it, prunes / compresses / multiplies there, and writes the pruned A back in its stored orientation. */
int sm_transpose(const void* in, void* out, size_t rows, size_t cols, size_t ld_in, size_t ld_out, size_t elt_bytes,
                 size_t batch, size_t stride_in, size_t stride_out, sm_stream_t stream);

/* ---- bfloat16 forms (extension; SURVEY.md 8(f) rank 2: the vendor call behind spmma.hxx:40-113 lists bf16 among its
 *      2:4 types, examples/libcusparse_lt/include/cusparseLt.h:164-169).  Same arguments, blob layout and rules as the
 *      _f16 entry points: the selection looks at magnitude bit patterns only, so prune (STRIP), check, compress and
 *      decompress ARE the fp16 kernels; the TILE rule (sums of magnitudes), the matmuls (v_smfmac_f32_16x16x64_bf16 /
 *      v_mfma_f32_16x16x32_bf16, fp32 accumulate) and the final round-to-nearest-even have their own code. */
int sm_prune24_bf16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, sm_stream_t stream);
int sm_prune24_check_bf16(const void* A, size_t m, size_t k, size_t ld, int* d_valid, sm_stream_t stream);
int sm_compress24_bf16(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob,
                       sm_stream_t stream);
int sm_decompress24_bf16(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A,
                         sm_stream_t stream);
int sm_spmma_bf16(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k, size_t batch,
                  size_t strideB, size_t strideC, float alpha, float beta, sm_stream_t stream);
int sm_spmma_fused_bf16(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                        size_t strideA, size_t strideB, size_t strideC, float alpha, float beta, sm_stream_t stream);
int sm_gemm_rowmajor_bf16(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda,
                          size_t batch, size_t strideA, size_t strideB, size_t strideC, float alpha, float beta,
                          sm_stream_t stream);
int sm_fill_uniform_bf16(void* out, size_t count, uint64_t seed, float lo, float hi, sm_stream_t stream);

/* ---- int8 forms (extension; SURVEY.md 8(f) rank 2, cusparseLt.h:164-169).  Elements are signed bytes; the rules
 *      act on |x| (|-128| = 128); same blob geometry with 1-byte elements (sm_compress24_size(m, k, 1, batch, ...)).
 *      sm_spmma_i8: C (int32, row-major m x n) = A_2:4 . B (+ C when
 *      accumulate != 0), exact integer arithmetic on v_smfmac_i32_16x16x128_i8; B is [n][k] -- K-CONTIGUOUS per output
 *      column ("TN", the layout int8 matrix cores are fed in), B_b = B + b * strideB (0 = shared).  Needs k % 64 == 0,
 *      an even m, a 16-byte aligned B; SM_STATUS_NOT_SUPPORTED otherwise. */
/* out[c][r] = in[r][c] for a row-major rows x cols byte matrix (out of place): turns the reference's row-major k x n B
 * (spmma.hxx:40-64) into the [n][k] operand of sm_spmma_i8; a one-off for the small, reused weight operand */
int sm_transpose_i8(const void* in, void* out, size_t rows, size_t cols, sm_stream_t stream);
int sm_prune24_i8(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, sm_stream_t stream);
int sm_prune24_check_i8(const void* A, size_t m, size_t k, size_t ld, int* d_valid, sm_stream_t stream);
int sm_compress24_i8(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob,
                     sm_stream_t stream);
int sm_decompress24_i8(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A,
                       sm_stream_t stream);
int sm_spmma_i8(const void* blob, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t batch,
                size_t strideB, size_t strideC, int accumulate, sm_stream_t stream);
/* the same product requantised on the way out: C (int8) = saturate(round_to_nearest_even(scale * acc)), one fp32
 * multiply of the int32 accumulator converted to fp32 */
int sm_spmma_i8_q(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k, size_t batch, size_t strideB,
                  size_t strideC, float scale, sm_stream_t stream);
/* prune (STRIP) + compress + matmul in one kernel straight from the dense int8 A (row-major, lda): bit-identical to
 * sm_compress24_i8 + sm_spmma_i8[_q], no blob.  Needs k % 64 == 0 and 16-byte aligned rows; SM_STATUS_NOT_SUPPORTED
 * otherwise (use the pair). */
int sm_spmma_fused_i8(const void* A, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                      size_t strideA, size_t strideB, size_t strideC, int accumulate, sm_stream_t stream);
int sm_spmma_fused_i8_q(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                        size_t strideA, size_t strideB, size_t strideC, float scale, sm_stream_t stream);
/* Dense int8 GEMM in the same layout, the like-for-like dense denominator of sm_spmma_i8: C (int32) = A . B (+ C when
 * accumulate != 0), or requantised as sm_spmma_i8_q, exact integer arithmetic on v_mfma_i32_16x16x64_i8.  A is row-major
 * m x k (lda, A_b = A + b * strideA), B [n][k] as for sm_spmma_i8 (strideB = 0: shared), C row-major m x n (strideC).
 * Shared B with contiguous A and C runs as one tall matrix.  Needs k % 64 == 0 and 16-byte aligned rows of A and B
 * (lda, strideA, strideB multiples of 16), each dimension below 2^31; any m (no even-m rule): SM_STATUS_NOT_SUPPORTED
 * otherwise.  A null operand or lda < k: SM_STATUS_INVALID_VALUE.  Both decided before any device work. */
int sm_gemm_rowmajor_i8(const void* A, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                        size_t strideA, size_t strideB, size_t strideC, int accumulate, sm_stream_t stream);
int sm_gemm_rowmajor_i8_q(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                          size_t strideA, size_t strideB, size_t strideC, float scale, sm_stream_t stream);

/* ---- OCP fp8 forms (extension).  Elements are bytes in one of the two OCP 8-bit float encodings (torch.float8_e4m3fn /
 *      torch.float8_e5m2; not the fnuz encodings), named by `fmt`.  The rules are the fp16 rules on the exact fp16 image of
 *      the bytes: the result of sm_prune24_fp8 is that of sm_prune24_f16 on the image, mapped back, bit for bit.  Keys are
 *      bits & 0x7f (-0 and +0 equal, NaN above every finite value and inf; an e5m2 NaN keys as its quieted image does:
 *      0x7d as 0x7f), ties keep the lower k; TILE adds the image's magnitudes in fp32 as sm_prune24_f16 does.  Dropped
 *      positions become 0x00, kept bytes are left as they are (NaN payloads included).  A byte is zero when
 *      (v & 0x7f) == 0: 0x80 (-0) is zero, NaN is not.  Same blob geometry as int8 (sm_compress24_size(m, k, 1, batch,
 *      ...)); the 2-bit codes of a strip are those sm_compress24_f16 stores for the image.
 *      sm_spmma_fp8: C_b = alpha * row_scale[i] * (A_2:4,b . B_b) + beta * C_b on v_smfmac_f32_16x16x128_<A>_<B>, fp32
 *      accumulation, one rounding to the output type at the end (beta reads C in that type; beta == 0 does not read C).
 *      A and B may be in different formats.  B is [n][k], K-CONTIGUOUS per output column as for sm_spmma_i8
 *      (sm_transpose_i8 turns a row-major k x n B into it), B_b = B + b * strideB (0 = shared); C is row-major m x n of
 *      out_type, C_b = C + b * strideC (elements).  row_scale: NULL (= 1) or a device array of m floats, the per-output-
 *      channel dequantisation scale of fp8 weights (a per-tensor scale folds into alpha).
 *      Needs k % 64 == 0, an even m, a 16-byte aligned B and strideB % 16 == 0 (the fused form also 16-byte aligned rows
 *      of A: lda % 16 == 0, strideA % 16 == 0), each dimension below 2^31: SM_STATUS_NOT_SUPPORTED otherwise, decided
 *      before any device work.  A null operand, a bad fmt / out_type / alg or ld < k: SM_STATUS_INVALID_VALUE.  Like every
 *      entry point here they only enqueue work, so they can be captured into a hipGraph. */
#define SM_FP8_E4M3 0 /* OCP e4m3 ("fn": no inf, NaN = 0x7f / 0xff), torch.float8_e4m3fn */
#define SM_FP8_E5M2 1 /* OCP e5m2 (IEEE-like: inf and NaN), torch.float8_e5m2 */
#define SM_OUT_F32 0
#define SM_OUT_F16 1
#define SM_OUT_BF16 2
/* A_in / A_out row-major m x k, ld; may alias (in place).  alg = SM_PRUNE_TILE or SM_PRUNE_STRIP; fmt matters to TILE only
 * for the magnitudes and to both for e5m2 NaN keys. */
int sm_prune24_fp8(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, int fmt, sm_stream_t stream);
/* *d_valid = 0 iff every strip holds <= 2 non-zeros ((v & 0x7f) != 0), else 1 (the same for both formats). */
int sm_prune24_check_fp8(const void* A, size_t m, size_t k, size_t ld, int* d_valid, sm_stream_t stream);
/* STRIP selection of the two largest keys per strip, as sm_compress24_i8 but with the fp8 keys of `fmt`; blob 16-byte aligned. */
int sm_compress24_fp8(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob, int fmt,
                      sm_stream_t stream);
int sm_decompress24_fp8(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A,
                        sm_stream_t stream);
int sm_spmma_fp8(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k, size_t batch, size_t strideB,
                 size_t strideC, int fmt_a, int fmt_b, int out_type, float alpha, float beta, const float* row_scale,
                 sm_stream_t stream);
/* prune (STRIP) + compress + matmul in one kernel straight from the dense fp8 A (row-major, lda, batch stride strideA):
 * C bit-identical to sm_prune24_fp8(STRIP) + sm_compress24_fp8 + sm_spmma_fp8, no blob. */
int sm_spmma_fused_fp8(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                       size_t strideA, size_t strideB, size_t strideC, int fmt_a, int fmt_b, int out_type, float alpha,
                       float beta, const float* row_scale, sm_stream_t stream);
/* Dense fp8 GEMM in the same layout, the like-for-like dense denominator of sm_spmma_fp8: C_b = alpha * row_scale[i] *
 * (A_b . B_b) + beta * C_b with the epilogue, formats, output types and statuses of sm_spmma_fused_fp8, on the full-rate
 * dense v_mfma_f32_16x16x128_f8f6f4 (fp32 accumulation).  A is row-major m x k (lda, A_b = A + b * strideA), every
 * element multiplied.  Any m (no even-m rule). */
int sm_gemm_rowmajor_fp8(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                         size_t strideA, size_t strideB, size_t strideC, int fmt_a, int fmt_b, int out_type, float alpha,
                         float beta, const float* row_scale, sm_stream_t stream);

/* ---- fp8 quantisation of 16-bit operands (extension): what produces the fp8 bytes and the row_scale of the entry points
 *      above.  Per row i of a row-major fp16 / bf16 A (rows x k, lda), FMAX = 448 (SM_FP8_E4M3) / 57344 (SM_FP8_E5M2):
 *        amax_i = max(max_j |a_ij| over the FINITE elements of the row, 2^-100)       exact
 *        row_scale_i = amax_i / FMAX,  inv_i = FMAX / amax_i                           two correctly rounded fp32 divisions
 *        q_ij = fp32(a_ij) * inv_i (one fp32 multiply) rounded to nearest even to fmt, subnormals of fmt included
 *      |fp32(a_ij) * inv_i| <= FMAX (1 + 2^-23), which rounds to FMAX: a finite row never overflows and the largest
 *      element of a non-zero row becomes 0x7e / 0x7b.  |a_ij - row_scale_i q_ij| <= R |a_ij| + S row_scale_i with
 *      R = 2^-4, S = 2^-10 (e4m3), R = 2^-3, S = 2^-17 (e5m2).  An all-zero row gives 0x00 (-0: 0x80).  Non-finite
 *      elements do not enter amax_i: NaN -> 0x7f (sign cleared), +-inf -> 0x7f (e4m3) / 0x7c | sign (e5m2).
 *      sm_quantize_rows_fp8_*: Q (row-major rows x k bytes, ldq) and row_scale[rows]; any k.
 *      sm_quantize_compress24_fp8_*: the same rule, then the STRIP selection on the quantised bytes, written as the blob
 *      of sm_compress24_size(rows, k, 1, 1) bytes -- identical in every byte to sm_quantize_rows_fp8_* followed by
 *      sm_compress24_fp8(Q, rows, k, k, 1, rows * k, blob, fmt) -- and the same row_scale; A is read once and no dense fp8
 *      A exists.  The blob is stage-major over all rows, so rows = batch * m stacked matrices give the blob of
 *      batch m x k matrices; with a shared B multiply them as ONE matrix, sm_spmma_fp8(blob, Bt, C, rows, n, k, 1, 0,
 *      rows * n, ..., row_scale, ...): sm_spmma_fp8 indexes row_scale by row % m, so per-row scales of stacked rows reach
 *      the epilogue only in that form (batch > 1 with a B per batch and per-row scales is not covered).
 *      sm_quantize_transpose_fp8_*: the weight operand, row-major k x n 16-bit B (ldb) -> the [n][k] fp8 operand of the
 *      1-byte kernels, q = rne_fmt(clamp(fp32(b) * inv_scale, -FMAX, FMAX)) with a per-tensor inv_scale given by the
 *      caller (its reciprocal folds into alpha); the non-finite rule above.
 *      A null operand, a bad fmt, lda < k, ldq < k, ldb < n or a blob that is not 16-byte aligned:
 *      SM_STATUS_INVALID_VALUE.  Rows of A that are not 16-byte aligned (pointer, lda % 8), k % 64 != 0 for the compress
 *      form, a dimension of 2^31 or more: SM_STATUS_NOT_SUPPORTED.  rows == 0 or k == 0 (n == 0): success.  All decided
 *      before any device work; the entry points only enqueue on `stream` (no allocation, no synchronisation). */
int sm_quantize_rows_fp8_f16(const void* A, size_t rows, size_t k, size_t lda, void* Q, size_t ldq, float* row_scale, int fmt,
                             sm_stream_t stream);
int sm_quantize_rows_fp8_bf16(const void* A, size_t rows, size_t k, size_t lda, void* Q, size_t ldq, float* row_scale, int fmt,
                              sm_stream_t stream);
int sm_quantize_compress24_fp8_f16(const void* A, size_t rows, size_t k, size_t lda, void* blob, float* row_scale, int fmt,
                                   sm_stream_t stream);
int sm_quantize_compress24_fp8_bf16(const void* A, size_t rows, size_t k, size_t lda, void* blob, float* row_scale, int fmt,
                                    sm_stream_t stream);
int sm_quantize_transpose_fp8_f16(const void* B, size_t k, size_t n, size_t ldb, float inv_scale, void* Bt, int fmt,
                                  sm_stream_t stream);
int sm_quantize_transpose_fp8_bf16(const void* B, size_t k, size_t n, size_t ldb, float inv_scale, void* Bt, int fmt,
                                   sm_stream_t stream);

/* ---- im2col front end (extension).  X: N x C x H x W activations (NCHW, contiguous).
 *      A: per image the row-major L x K operand of the layer's matmul, L = out_h * out_w rows (row oh * out_w + ow),
 *      K = C * kh * kw columns (column c * kh * kw + r * kw + u), images back to back -- the transpose of torch's
 *      unfold, i.e. the (m, k) = (L, C * kh * kw) operand of the reference's shape tables
 *      (datasets/get_shapes.py:30-40, 66-73).  out = floor((in + 2 pad - dilation (k - 1) - 1) / stride) + 1
 *      (get_shapes.py:19-20).  sm_im2col_compress24_* writes sm_compress24_*'s blob of that A (m = L, k = K,
 *      batch = N; size from sm_compress24_size) without ever materialising the dense A; same bytes as
 *      sm_im2col_* followed by sm_compress24_*. */
int sm_conv_out_size(size_t in, size_t kernel, size_t stride, size_t pad, size_t dilation, size_t* out /*host*/);
int sm_im2col_f16(const void* X, size_t N, size_t C, size_t H, size_t W, size_t kh, size_t kw, size_t stride, size_t pad,
                  size_t dilation, void* A, sm_stream_t stream);
int sm_im2col_bf16(const void* X, size_t N, size_t C, size_t H, size_t W, size_t kh, size_t kw, size_t stride, size_t pad,
                   size_t dilation, void* A, sm_stream_t stream);
int sm_im2col_compress24_f16(const void* X, size_t N, size_t C, size_t H, size_t W, size_t kh, size_t kw, size_t stride,
                             size_t pad, size_t dilation, void* blob, sm_stream_t stream);
int sm_im2col_compress24_bf16(const void* X, size_t N, size_t C, size_t H, size_t W, size_t kh, size_t kw, size_t stride,
                              size_t pad, size_t dilation, void* blob, sm_stream_t stream);

/* ---- implicit-GEMM form for convolution layers (extension; SURVEY.md 8(f) rank 3, datasets/get_shapes.py:30-40,66-73):
 *      C[i][l][:] = alpha * prune24_strip(A_i)[l][:] * B + beta * C[i][l][:] with A_i = the im2col operand of image i
 *      (sm_im2col_*'s layout: L = out_h * out_w rows, K = Cin * kh * kw columns), computed straight from the NCHW
 *      activations X: neither the dense A nor its blob is ever written to or read from HBM.  B: K x n_out row-major
 *      (shared by the images), C: N * L rows x n_out row-major.  Bit-identical to sm_im2col_compress24_* followed by
 *      sm_spmma_* (m = L, k = K, batch = N, strideB = 0).  Needs K % 64 == 0, n_out % 8 == 0, an even W of at most ~120
 *      columns and kh * kw <= 64; SM_STATUS_NOT_SUPPORTED otherwise (use the pair). */
int sm_conv_spmma_fused_f16(const void* X, const void* B, void* C, size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw,
                            size_t stride, size_t pad, size_t dilation, size_t n_out, float alpha, float beta, sm_stream_t stream);
int sm_conv_spmma_fused_bf16(const void* X, const void* B, void* C, size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw,
                             size_t stride, size_t pad, size_t dilation, size_t n_out, float alpha, float beta, sm_stream_t stream);
/* WHICH KERNEL CLASS sm_conv_spmma_fused_{f16,bf16} run for a layer, and the stage plan they run it with: the dispatch rule as a
 * host-side query -- the one function the entry points themselves switch on, so the answer is what launches.  For tests (a test
 * named for a class asserts that its layer reaches it) and schedulers; no device work.
 *   N .. n_out: as passed to the entry point.  flags: what the entry point reads off its pointers -- SM_CONV_FLAG_X_ALIGNED16 (X on a
 *   16-byte boundary; implies _X_ALIGNED4), _X_ALIGNED4 (X on a 4-byte boundary), _B_ALIGNED16 (B on a 16-byte boundary).
 * *form: SM_CONV_FORM_NOT_TAKEN -- the entry point returns SM_STATUS_NOT_SUPPORTED (sm_conv_spmma_* then needs its workspace);
 *   _EMPTY -- success, nothing launched (N, Cin or n_out zero); _V16 -- 16-byte patch DMAs (W % 8 == 0, a 16-byte aligned X, at most
 *   16 DMA instructions per stage); _SMALL4 / _LARGE4 -- 4-byte patch DMAs with at most 16 / at most 48 instructions per stage.
 *   Each class has a 64-column (n_out <= 64) and a 128-column kernel: plan[0].
 * plan (may be NULL; else SM_CONV_PLAN_WORDS unsigned), the numbers the kernel is launched with:
 *   [0] column tile (64 or 128)      [1] RI: patch rows per channel      [2] pitch: patch row pitch in halves (padl + W)
 *   [3] padl: zero halves in front of a row   [4] rpi: patch rows per DMA instruction   [5] nch: channels a 64-deep stage can touch
 *   [6] a_n: patch DMA instructions per stage  [7] patch_bytes: one stage's patch buffer   [8] dynamic LDS bytes of the launch
 *   [9] tiles_m: 128-pixel tiles per image     [10] tiles_n: column tiles
 *   _EMPTY: zeros.  _NOT_TAKEN: [0] and, as far as the rule got before it declined, [1] .. [7] of the 4-byte plan (zeros for a
 *   refusal that precedes the plan: n_out % 8, the alignments, K % 64, W, kh * kw); [8] .. [10] zero.  sm_last_error() then holds the
 *   words the entry point would leave, under this query's name.
 * Status: SM_STATUS_INVALID_VALUE for form == NULL, an unknown flag, and what the entry point answers so: a zero window extent,
 * stride or dilation, a window larger than the padded input. */
#define SM_CONV_FORM_NOT_TAKEN 0
#define SM_CONV_FORM_EMPTY 1
#define SM_CONV_FORM_V16 2
#define SM_CONV_FORM_SMALL4 3
#define SM_CONV_FORM_LARGE4 4
#define SM_CONV_FLAG_X_ALIGNED16 1u
#define SM_CONV_FLAG_X_ALIGNED4 2u
#define SM_CONV_FLAG_B_ALIGNED16 4u
#define SM_CONV_PLAN_WORDS 11
int sm_conv_spmma_fused_plan(size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw, size_t stride, size_t pad, size_t dilation,
                             size_t n_out, unsigned flags, int* form, unsigned* plan);
/* The same product by the faster of its two routes (round 4): the implicit-GEMM kernel, or -- small-spatial layers with a long K
 * (out_h * out_w <= 256 and K >= 2048: the 14 x 14 x 512-channel layers of a ResNet) -- sm_im2col_compress24_* into `workspace`
 * followed by sm_spmma_*.  Same C bit for bit either way.  sm_conv_spmma_workspace gives the bytes: the blob's size
 * (sm_compress24_size(out_h * out_w, Cin * kh * kw, 2, N)) for the layers the rule sends to the pair AND for every geometry the
 * implicit kernel cannot run (K % 64 != 0 such as a 7 x 7 x 3 stem, an odd or too wide W, kh * kw > 64, a patch beyond its DMA /
 * LDS limits), so that a caller who sizes the workspace with it never gets SM_STATUS_NOT_SUPPORTED for a geometry reason; 0 where
 * the implicit kernel is kept.  The query sees neither n_out nor the pointers: for n_out % 8 != 0 or a B / X that is not 16- /
 * 4-byte aligned size the workspace with sm_compress24_size.  With no workspace the implicit kernel runs wherever it can. */
int sm_conv_spmma_workspace(size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw, size_t stride, size_t pad, size_t dilation,
                            size_t* bytes);
int sm_conv_spmma_f16(const void* X, const void* B, void* C, size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw, size_t stride,
                      size_t pad, size_t dilation, size_t n_out, float alpha, float beta, void* workspace, size_t workspace_bytes,
                      sm_stream_t stream);
int sm_conv_spmma_bf16(const void* X, const void* B, void* C, size_t N, size_t Cin, size_t H, size_t W, size_t kh, size_t kw, size_t stride,
                       size_t pad, size_t dilation, size_t n_out, float alpha, float beta, void* workspace, size_t workspace_bytes,
                       sm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSIFYME_H_ */
