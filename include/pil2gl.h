/*
 * pil2gl.h -- C ABI of the MI355X (gfx950) STARK proving hot path for pil2-stark-js.
 *
 * One shared library (pil2-stark-js_amd/lib/libpil2gl.so), plain pointers and
 * sizes, no C++/torch types.  Each entry point replaces one JavaScript-level
 * operator of the reference (cited per function, paths relative to the
 * reference checkout); the Node.js addon (pil2-stark-js_amd/addon) and the
 * Python ctypes binding (pil2-stark-js_amd/python/pil2gl) are thin wrappers
 * over exactly these symbols.  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *  - Field elements are canonical little-endian u64 in [0,p), p = 2^64-2^32+1.
 *    Outputs are always canonical.  (The reference's WASM kernel may leave a
 *    digest word in [p,2^64), equal mod p -- src/helpers/glwasm.js:196-210;
 *    its JS twin src/helpers/hash/poseidon/poseidon.js is canonical, and so is this library.)
 *  - Matrices are row-major: element (row r, col c) at r*nCols + c
 *    (src/witness/witnessCalculator.js:113-141, src/helpers/fft/fft_worker.js:53-56).
 *  - Extension-field elements are 3 consecutive u64 (src/helpers/f3g.js:5-9).
 *  - Functions without suffix take HOST pointers (copy in, compute on the GPU,
 *    copy out): drop-in for the reference's BigUint64Array/BigBuffer calls.
 *    Functions with suffix _dev take DEVICE pointers (hipMalloc / pil2gl_dev_alloc /
 *    torch tensor.data_ptr()) plus a hipStream_t passed as void* (NULL = default
 *    stream), so buffers can stay resident in HBM across the prover's steps.
 *    Most of them only ENQUEUE work on that stream and return:
 *      interpolate / interpolate_cosets[_ws] / extend_cosets_unshifted / extend_coefs_brev[_cosets] / fft / ifft, linear_hash_rows, merkelize,
 *      merkelize_level, merkelize_digests, poseidon, fri_fold, fri_verify_fold, fri_transpose, build_x, geometric,
 *      x_div_x_sub_xi[_cosets], gprod, gsum, dev_zero, and their bn128_ twins; bn128_eval_program, bn128_poly_div_xk_sub and bn128_poly_eval (after staging: see there); bn128_batch_inverse, bn128_gprod, bn128_gsum and bn128_gsum_col; gsum_col; logup_sum and bn128_logup_sum; range_sum and bn128_range_sum; logup_cluster and bn128_logup_cluster; grand_prod and bn128_grand_prod; plookup_fold, plookup_prod and their bn128_ twins; the open of a lookup_session or range_session and their write with a null hostTotal; land_rows with a null hostFirstBad;
 *      wtns_adds and bn128_wtns_adds, wtns_gather and bn128_wtns_gather with a null hostFirstBad, conn_pols and bn128_conn_pols with a null hostFirstBad.
 *    dev_upload_async / dev_download_async / copy_after / copy_fence take no stream: they ENQUEUE on the library's own copy
 *    stream (or order it against the stream given) and return.
 *    The following _dev calls BLOCK until their work on the stream has finished, because they hand a result to the host or
 *    stage host-side tables in a scratch slot the next call reuses:
 *      eval_program (op-list and scalar pool are host temporaries), rows_dot_ext / rows_dot_ext_multi[_step] / cols_dot_ext /
 *      cols_dot_ext_multi / fri_combine / fri_combine_order (host-side weights), compute_evals (returns the evaluations),
 *      build_zhinv, build_one_row_zerofier_inv, build_frame_zerofier, compute_q_split[_brev], compute_q_stark, compute_fri_pol, build_lev (small host tables),
 *      h1h2 and bn128_h1h2 (the missing row comes back), conn_check and bn128_conn_check, tuple_check and bn128_tuple_check, lookup_mult and bn128_lookup_mult, range_mult and bn128_range_mult (the report comes back), the add of a lookup_session or range_session and their write with a hostTotal, synth_fibonacci, group_proof / group_proofs and bn128_group_proof / bn128_group_proofs (openings copied to host memory),
 *      land_rows, wtns_gather, bn128_wtns_gather, conn_pols and bn128_conn_pols with a hostFirstBad (the index comes back), dev_load_file / dev_save_file (the file is read / written
 *      when they return), copy_sync, and dev_upload / dev_download (synchronous copies of pageable memory).
 *    So do the host-pointer verifier calls roots_from_group_proofs and bn128_roots_from_group_proofs (roots copied to host memory).
 *    bn128_group_proof[s]_dev take no stream: their copies and their gather kernel run on the NULL stream, which orders them after work
 *    on BLOCKING streams only (the NULL stream itself, streams created with hipStreamDefault).  A tree built on a stream created
 *    hipStreamNonBlocking is not ordered against them: synchronise that stream first (pil2gl_sync).
 *    A whole config-3 proof keeps the GPU busy 99.3 % of its wall time with these.
 *  - Every function returns 0 on success, a negative PIL2GL_E* code otherwise;
 *    pil2gl_last_error() describes the failure (the reference throws Error /
 *    rejects the Promise; the addon converts the code back into a JS exception).
 *  - The library has no CPU fallback: without a HIP device every compute entry
 *    point fails with PIL2GL_ENODEV.  Calls that need no device say so where they are declared: merkle_num_nodes, add / mul /
 *    square, the jit_cache_ and precompile_ calls, wtns_adds_plan, conn_plan, conn_check_plan, tuple_check_plan, lookup_mult_plan, range_mult_plan, lookup_session_plan, range_session_plan, logup_sum_plan, range_sum_plan, logup_cluster_plan, grand_prod_plan, plookup_plan, the debug_ hooks.
 *  - Calls are not thread-safe against each other (the reference issues them
 *    sequentially from one JS thread: src/prover/prover.js, `await` on every step).
 */
#pragma once
#include <stdint.h>
#include "pil2gl_expr.h"
#include "pil2gl_bn_expr.h"
#ifdef __cplusplus
extern "C" {
#endif

#define PIL2GL_OK        0
#define PIL2GL_EINVAL   -1      /* bad argument (the reference would throw / assert) */
#define PIL2GL_ENODEV   -2      /* no usable HIP device */
#define PIL2GL_ENOMEM   -3      /* device or host allocation failed */
#define PIL2GL_EHIP     -4      /* a HIP runtime call failed */

/* ---- lifecycle ---------------------------------------------------------- */
int         pil2gl_init(int device);            /* select device, upload tables; idempotent */
void        pil2gl_shutdown(void);
const char *pil2gl_last_error(void);
int         pil2gl_version(void);
int         pil2gl_device_info(char *name, uint32_t nameLen, uint32_t *numCUs, uint64_t *totalMem);

/* ---- device buffers (for hosts without their own HIP allocator, e.g. Node) ---- */
int pil2gl_dev_alloc(uint64_t nWords, uint64_t **out);
int pil2gl_dev_free(uint64_t *p);
int pil2gl_dev_zero(uint64_t *p, uint64_t nWords, void *stream);
int pil2gl_dev_upload(uint64_t *dst, const uint64_t *hostSrc, uint64_t nWords);
int pil2gl_dev_download(uint64_t *hostDst, const uint64_t *src, uint64_t nWords);
int pil2gl_sync(void *stream);

/* ---- the host <-> HBM leg: pinned memory, asynchronous copies, file loaders (csrc/hostleg.hip) --------------------
 * How a witness or a constant tree reaches HBM when it starts in host memory or in a file, as the reference's does
 * (src/witness/witnessCalculator.js:145-214, src/prover/prover.js:24, merklehash_p.js:228-278).
 * pinned host memory (hipHostMalloc) for callers without a HIP allocator, and pinning of memory the caller owns */
int pil2gl_host_alloc(uint64_t nWords, uint64_t **out);
int pil2gl_host_free(uint64_t *p);
int pil2gl_host_register(uint64_t *p, uint64_t nWords);
int pil2gl_host_unregister(uint64_t *p);
/* Copies on a library-owned COPY stream (created non-blocking on first use, so it overlaps with the NULL stream; destroyed by
 * pil2gl_shutdown).  hostSrc / hostDst must be pinned or registered over the whole range, else PIL2GL_EINVAL: the copy never
 * degrades to a synchronous one.  (The runtime tells no extent of registered memory: the first and the last byte of the range are
 * what is checked; a range must lie in ONE pinned or registered block.)  These only enqueue.  Order them against compute streams with the two event calls:
 *   pil2gl_copy_after(s)   copies enqueued from now on start after the work now on s   (s may still be reading the target)
 *   pil2gl_copy_fence(s)   work enqueued on s from now on starts after the copies enqueued so far
 *   pil2gl_copy_sync()     the host waits for the copy stream
 * Double-buffered use: copy_after(s); dev_upload_async(next, ...); <proof k on s>; copy_fence(s); <proof k + 1 on s reads next>. */
int pil2gl_dev_upload_async(uint64_t *dst, const uint64_t *hostSrc, uint64_t nWords);
int pil2gl_dev_download_async(uint64_t *hostDst, const uint64_t *src, uint64_t nWords);
int pil2gl_copy_after(void *stream);
int pil2gl_copy_fence(void *stream);
int pil2gl_copy_sync(void);
/* The landing pass of words that came from outside, one read of each: *hostFirstBad = the smallest flat index into src of a
 * word that is not canonical (>= p), UINT64_MAX when all are -- a file is the one input nobody has checked, and every kernel
 * relies on canonical inputs.  The data is landed either way; the caller decides.  dstCols > srcCols: row r of dst = the srcCols
 * words of row r of src, then dstCols - srcCols zeros (writeToBigBuffer(buff, nCols), witnessCalculator.js:198-214); src and dst
 * must not overlap.  dstCols == srcCols: a copy, or with src == dst the check alone.  dstCols < srcCols: PIL2GL_EINVAL.
 * Pointers need 8-byte alignment only.  With hostFirstBad the call blocks until the answer is on the host; with NULL it only
 * enqueues and nothing is checked. */
int pil2gl_land_rows_dev(const uint64_t *src, uint64_t srcCols, uint64_t *dst, uint64_t dstCols, uint64_t nRows,
                         uint64_t *hostFirstBad, void *stream);
/* file <-> HBM through two pinned chunks of chunkWords (0 = 2^25 words = 256 MB, the reference's MaxBuffSize) on the copy
 * stream: one chunk is read from (written to) the file while the other is in flight.  Both block until done.
 * Both work on the COPY stream and order themselves against nothing else: when a compute stream may still write src (save)
 * or still read or write dst (load) -- most _dev calls only enqueue -- call pil2gl_copy_after(thatStream) first, or
 * synchronise it.  (The JS and Python wrappers do: DevBuffer.toFile / fromFile, io.save_pols_dev / load_pols_dev.)
 * dev_load_file: nRows x srcCols words from byteOffset land as nRows x dstCols (rules of land_rows; widening needs
 * chunkWords >= srcCols); hostFirstBad as above, flat index into the file's words, NULL = no check.  A file shorter than
 * byteOffset + 8*nRows*srcCols bytes fails with PIL2GL_EINVAL naming file, found and expected size before anything is copied.
 * dev_save_file: the file is created if missing, cut at byteOffset, and nWords words are appended there (a header first,
 * then each section at its offset in ascending order, writes a `.consttree`).  A byteOffset beyond the file's end is
 * PIL2GL_EINVAL (nothing is padded).  When a copy or a write fails midway the file is left holding the chunks written so far. */
int pil2gl_dev_load_file(const char *fileName, uint64_t byteOffset, uint64_t nRows, uint64_t srcCols,
                         uint64_t *dst, uint64_t dstCols, uint64_t chunkWords, uint64_t *hostFirstBad);
int pil2gl_dev_save_file(const char *fileName, uint64_t byteOffset, const uint64_t *src, uint64_t nWords, uint64_t chunkWords);

/* ---- NTT / LDE: src/helpers/fft/fft_p.js -------------------------------- */
/* interpolate(buffSrc,nPols,nBits,buffDst,nBitsExt)  fft_p.js:187-297:
 * per column, coefficients = iNTT_N(col), c_k *= 7^k, zero-pad to 2^nBitsExt, NTT ->
 * evaluations on the coset 7*<w_E> in natural order (== extendPol, polutils.js:18-30). */
int pil2gl_interpolate(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt);
int pil2gl_interpolate_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt, void *stream);
/* The same extension restricted to cosets j in [cosetBegin, cosetBegin+cosetCount) of the 2^(nBitsExt-nBits): dst is
 * 2^nBits x (cosetCount*nPols), element (pos, j - cosetBegin, c) = interpolate()'s row (pos << b) + j, column c.
 * One slice per GPU is the multi-GPU partition of extendAndMerkelize; the full range equals interpolate. */
int pil2gl_interpolate_cosets_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                  uint32_t cosetBegin, uint32_t cosetCount, void *stream);
/* The slice [cosetBegin, cosetBegin+cosetCount) of the PLAIN extension of the columns: src holds their evaluations on the
 * size-2^nBits subgroup, dst row (pos, j - cosetBegin) = row (pos << b) + j of fft(nBitsExt) applied to their zero-padded
 * coefficients (no coset shift).  This is how a rank extends its part of the split quotient (stark_gen_helpers.js:192). */
int pil2gl_extend_cosets_unshifted_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                       uint32_t cosetBegin, uint32_t cosetCount, void *stream);
/* The whole plain extension from COEFFICIENTS: coefBrev is 2^nBits x nPols with coefficient m of every column at row bitrev(m)
 * (pil2gl_compute_q_split_brev_dev writes that order); dst = fft(nBitsExt) of the zero-padded coefficient matrix, natural order
 * (stark_gen_helpers.js:192) -- without the padded 2^nBitsExt-row input and its first nBitsExt - nBits stages. */
int pil2gl_extend_coefs_brev_dev(const uint64_t *coefBrev, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt, void *stream);
/* The slice [cosetBegin, cosetBegin+cosetCount) of that extension, local-slice order (row (pos, j - cosetBegin) = row (pos << b) + j): how a
 * rank of a coset-split proof extends its part of the split quotient from the coefficients every rank holds (stark_gen_helpers.js:179-192),
 * without first turning them into evaluations and back. */
int pil2gl_extend_coefs_brev_cosets_dev(const uint64_t *coefBrev, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                        uint32_t cosetBegin, uint32_t cosetCount, void *stream);
/* Same with a caller-provided workspace of 2^nBits x nPols words for the coefficient matrix instead of the library's own
 * scratch; workspace == src is allowed (src is then overwritten): at config 5 a rank holds the 107 GB trace and its
 * 107 GB coset slice and nothing else. */
int pil2gl_interpolate_cosets_ws_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                     uint32_t cosetBegin, uint32_t cosetCount, uint64_t *workspace, void *stream);
/* fft / ifft (buffSrc,nPols,nBits,buffDst)  fft_p.js:178-184: in-order multi-column NTT / iNTT,
 * root F.w[nBits]; ifft = fft, index j -> (n-j) mod n, times 1/n (fft/fft.js:165-174). src may equal dst. */
int pil2gl_fft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst);
int pil2gl_ifft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst);
int pil2gl_fft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream);
int pil2gl_ifft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream);
/* The reference's worker-level operators, for a caller that keeps fft_p.js's own block loop (pool.exec sites fft_p.js:93,162,166);
 * the calls above replace that whole loop and are the product path.
 * fft_block(buff,start_pos,nPols,nBits,s,blockBits,layers)  fft_worker.js:21-67: buf = the 2^blockBits x nPols block standing at
 * row start_pos of a 2^nBits-row transform; `layers` butterfly stages ending at stage s, in place.  layers <= blockBits.
 * interpolatePrepareBlock(buff,width,start,inc,st_i,st_n)  fft_worker.js:6-19: row i of the height x width block times start*inc^i. */
int pil2gl_fft_block_dev(uint64_t *buf, uint64_t start_pos, uint64_t nPols, uint32_t nBits, uint32_t s, uint32_t blockBits, uint32_t layers, void *stream);
int pil2gl_interpolate_prepare_block_dev(uint64_t *buf, uint64_t width, uint64_t height, uint64_t start, uint64_t inc, void *stream);

/* ---- Poseidon / linear hash / Merkle tree -------------------------------- */
/* WASM export poseidon(pIn,nIn,pCap,nCap,pOut,nOut)  src/helpers/glwasm.js:216-426;
 * JS twin poseidon(inputs[8],capacity[4],nOuts)  hash/poseidon/poseidon.js:57.
 * `count` independent permutations: in = count x 8, cap = count x 4 (NULL = zeros), out = count x nOut. */
int pil2gl_poseidon(const uint64_t *in, const uint64_t *cap, uint64_t count, uint32_t nOut, uint64_t *out);
int pil2gl_poseidon_dev(const uint64_t *in, const uint64_t *cap, uint64_t count, uint32_t nOut, uint64_t *out, void *stream);
/* Transcript.put of a list (transcript.js:49-66): nBlocks full blocks of 8 elements absorbed one after the other, the
 * first with capacity hostCap, each next one with the previous output's first four words; hostOut12 = the last
 * permutation's twelve outputs.  One launch for the whole chain (twelve lanes share each permutation). */
int pil2gl_sponge_absorb(const uint64_t *hostBlocks, uint64_t nBlocks, const uint64_t hostCap[4], uint64_t hostOut12[12]);
/* worker linearHash(buffIn,width,st_i,st_n,splitLinearHash)  merklehash_worker.js:37-82
 * (= WASM multiLinearHash glwasm.js:1124-1218 / multiLinearHashGPU :1089-1122, with the
 * width<=4 raw copy of merklehash_worker.js:42-49): out = height x 4 digests. */
int pil2gl_linear_hash_rows(const uint64_t *in, uint64_t width, uint64_t height, int split, uint64_t *out);
int pil2gl_linear_hash_rows_dev(const uint64_t *in, uint64_t width, uint64_t height, int split, uint64_t *out, void *stream);
/* WASM merkelizeLevel(pIn,nOps,pOut)  glwasm.js:1220-1254: out[i] = Poseidon(in[8i..8i+7], cap=0)[0..3] */
int pil2gl_merkelize_level(const uint64_t *in, uint64_t nOps, uint64_t *out);
int pil2gl_merkelize_level_dev(const uint64_t *in, uint64_t nOps, uint64_t *out, void *stream);
/* MerkleHash._getNNodes(height*4)  merklehash_p.js:28-42: u64 words of tree.nodes */
uint64_t pil2gl_merkle_num_nodes(uint64_t height);
/* MerkleHash.merkelize(buff,width,height)  merklehash_p.js:44-133: nodes[0..4*height) = leaf digests,
 * then each level padded to an even node count with zero digests; root = last 4 words (:224-226). */
int pil2gl_merkelize(const uint64_t *elems, uint64_t width, uint64_t height, int split, uint64_t *nodes);
int pil2gl_merkelize_dev(const uint64_t *elems, uint64_t width, uint64_t height, int split, uint64_t *nodes, void *stream);
/* The upper part of merkelize (merklehash_p.js:87-103) alone: nodes[0..4*height) already holds the leaf digests (e.g.
 * gathered from the GPUs that hashed their own cosets); fills every higher level up to the root, zero padding included. */
int pil2gl_merkelize_digests_dev(uint64_t *nodes, uint64_t height, void *stream);
/* MerkleHash.getGroupProof(tree,idx)  merklehash_p.js:142-168: copies row idx (width words) to hostVals
 * and the sibling digest of every level (nLevels x 4 words) to hostSiblings; returns nLevels in *nLevels.
 * elems/nodes are DEVICE pointers (the tree stays in HBM); synchronises. */
int pil2gl_group_proof_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height,
                           uint64_t idx, uint64_t *hostVals, uint64_t *hostSiblings, uint32_t *nLevels);

/* the same for nIdx rows at once (fri.js:83-105 opens every tree at every query): hostOut receives, per index,
 * `width` row words followed by nLevels x 4 sibling words; one gather kernel, one device-to-host copy. */
int pil2gl_group_proofs_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height,
                            const uint64_t *hostIdxs, uint32_t nIdx, uint64_t *hostOut, uint32_t *nLevels);
/* verifier side: MerkleHash.calculateRootFromGroupProof  merklehash_p.js:169-203 for a batch of openings in
 * the packed layout pil2gl_group_proofs_dev writes (per opening: width values, then `levels` x 4 sibling words):
 * hostRoots[q] = the root the path of leaf hostIdxs[q] leads to; verifyGroupProof :212-215 is the comparison with the root. */
int pil2gl_roots_from_group_proofs(const uint64_t *hostProofs, uint64_t width, uint32_t levels, const uint64_t *hostIdxs, uint32_t nIdx,
                                   int splitLinearHash, uint64_t *hostRoots /* nIdx x 4 */);

/* ---- FRI: src/stark/fri.js ------------------------------------------------ */
/* FRI.fold(step>0, pol, challenge)  fri.js:22-61: pol has 2^polBits extension elements, out 2^outBits;
 * shiftInv = (1/7)^(2^(steps[0].nBits - polBits)) (fri.js:31-36, computed by the caller). */
int pil2gl_fri_fold(const uint64_t *pol, uint32_t polBits, uint32_t outBits, uint64_t shiftInv,
                    const uint64_t challenge[3], uint64_t *out);
int pil2gl_fri_fold_dev(const uint64_t *pol, uint32_t polBits, uint32_t outBits, uint64_t shiftInv,
                        const uint64_t challenge[3], uint64_t *out, void *stream);
/* FRI.verify, the per-query step of one layer for all queries at once  fri.js:121-127:
 * groups = 2^foldBits x (nQueries*3) row-major (row i = element i of every query's opened group),
 * sinv[q] = 1 / (shift * w_polBits^idx_q); out[q] = evalPol(ifft(group_q), challenge * sinv[q]). */
int pil2gl_fri_verify_fold(const uint64_t *groups, uint32_t foldBits, uint32_t nQueries, const uint64_t *sinv,
                           const uint64_t challenge[3], uint64_t *out /* nQueries x 3 */);
int pil2gl_fri_verify_fold_dev(const uint64_t *groups, uint32_t foldBits, uint32_t nQueries, const uint64_t *sinv,
                               const uint64_t challenge[3], uint64_t *out, void *stream);
/* getTransposedBuffer(pol, trasposeBits)  fri.js:187-202 */
int pil2gl_fri_transpose(const uint64_t *pol, uint32_t polBits, uint32_t transposeBits, uint64_t *out);
int pil2gl_fri_transpose_dev(const uint64_t *pol, uint32_t polBits, uint32_t transposeBits, uint64_t *out, void *stream);

/* ---- STARK step helpers: src/stark/stark_gen_helpers.js, src/helpers/polutils.js ---- */
/* x_n / x_ext tables  stark_gen_helpers.js:111-116,139-144: x[i] = shift * w[nBits]^i */
int pil2gl_build_x_dev(uint32_t nBits, uint64_t shift, uint64_t *x, void *stream);
/* out[i] = first * ratio^i, i < n: one coset's rows of x_ext (first = 7 w_E^j, ratio = w_N; stark_gen_helpers.js:139-144) or any other
 * table of powers, without building the whole 2^nBitsExt-row table (a rank of a coset-sharded proof holds its own cosets only) */
int pil2gl_geometric_dev(uint64_t first, uint64_t ratio, uint64_t n, uint64_t *out, void *stream);
/* buildZhInv(stark=true)  polutils.js:39-55 */
int pil2gl_build_zhinv_dev(uint32_t nBits, uint32_t nBitsExt, uint64_t *out, void *stream);
/* buildOneRowZerofierInv(stark=true)  polutils.js:57-71 */
int pil2gl_build_one_row_zerofier_inv_dev(uint32_t nBits, uint32_t nBitsExt, uint64_t rowIndex, uint64_t *out, void *stream);
/* buildFrameZerofierInv(stark=true)  polutils.js:74-102 (product of (x-root), not inverted) */
int pil2gl_build_frame_zerofier_dev(uint32_t nBits, uint32_t nBitsExt, uint64_t offsetMin, uint64_t offsetMax, uint64_t *out, void *stream);
/* computeQStark split/scale  stark_gen_helpers.js:179-190: qq2[i][p*qDim+k] = qq1[p*N+i][k] * (7^-N)^p, rows >= N zero */
int pil2gl_compute_q_split_dev(const uint64_t *qq1, uint32_t nBits, uint32_t nBitsExt, uint32_t qDim, uint32_t qDeg, uint64_t *qq2, void *stream);
/* the same pieces as the 2^nBits-row coefficient matrix alone, row bitrev(i) = coefficient i: coefBrev[bitrev(i)][p*qDim+k] = qq1[p*N+i][k] * (7^-N)^p */
int pil2gl_compute_q_split_brev_dev(const uint64_t *qq1, uint32_t nBits, uint32_t nBitsExt, uint32_t qDim, uint32_t qDeg, uint64_t *coefBrev, void *stream);
/* The quotient stage in one call (stark_gen_helpers.js:168-208): the constraint program, ifft, the split above and
 * pil2gl_extend_coefs_brev_dev; dstExt = 2^nBitsExt x (qDim*qDeg), the quotient stage's extended matrix.
 * ctx is the "ext" context of pil2gl_eval_program_dev (nBits = nBitsExt, primeShift = nBitsExt - nBits, every section a 2^nBitsExt-row
 * matrix); qSection is the section the program writes (width qDim): its ptr is ignored and may be NULL, the values live in the
 * library's scratch.  The program runs on the extended rows k * 2^s only, s = nBitsExt - nBits - ceil(log2 qDeg): deg Q < qDeg * N, so
 * those 2^(nBitsExt - s) values fix Q, and their inverse transform equals the first 2^(nBitsExt - s) rows of the full one word for word.
 * The evaluator sees a context of 2^(nBitsExt - s) rows whose sections have a row pitch of width * 2^s (same choice of kernel, same
 * optimiser); s = 0 is the full domain.  PIL2GL_EINVAL, before anything is launched or written: qDeg * 2^nBits > 2^nBitsExt, a program
 * that writes another section, a row offset that leaves the rows k * 2^s (none does when primeShift = nBitsExt - nBits).
 * For a SATISFIED AIR the result equals the full-domain sequence bit for bit.  For a witness that breaks a constraint Q has
 * coefficients above qDeg * N: the full-domain sequence drops them, this call folds them onto the low ones -- different matrices,
 * and neither proof verifies.  Constraint checking (calculateExps with debug) stays on the full domain.
 * Blocks like eval_program and compute_q_split_brev, whose host tables it stages; the extension is only enqueued. */
int pil2gl_compute_q_stark_dev(const glx_program *prog, const glx_ctx *ctx, uint32_t qSection, uint32_t nBits, uint32_t nBitsExt,
                               uint32_t qDim, uint32_t qDeg, uint64_t *dstExt, void *stream);
/* computeFRIStark xDivXSubXi  stark_gen_helpers.js:293-322: out[3*(k*nOpen+iOpen)+c] = (x_k / (x_k - xi))_c, x_k = 7 w_E^k.
 * A base-field xi = (7 w_E^k, 0, 0) is a row of the table: the reference throws "Division by zero" there (F.batchInverse), and
 * both forms return PIL2GL_EINVAL before anything is launched or written, whichever cosets are asked for. */
int pil2gl_x_div_x_sub_xi_dev(uint32_t nBitsExt, const uint64_t xi[3], uint64_t nOpen, uint64_t iOpen, uint64_t *out, void *stream);
/* the rows of cosets [cosetBegin, cosetBegin + cosetCount) of the 2^extBits only (one rank's slice of a coset-sharded proof), in
 * slice order: row pos * cosetCount + jl stands for extended row (pos << extBits) + cosetBegin + jl; cosetCount a power of two. */
int pil2gl_x_div_x_sub_xi_cosets_dev(uint32_t nBitsExt, uint32_t extBits, const uint64_t xi[3], uint64_t nOpen, uint64_t iOpen,
                                     uint32_t cosetBegin, uint32_t cosetCount, uint64_t *out, void *stream);
/* computeEvalsStark  stark_gen_helpers.js:216-264: lev = ifft_N(xi^k) (extension, N x 3), for every xi: at the N base-field roots of
 * unity xi = (w_N^j, 0, 0), where the closed form the library otherwise uses is 0 / 0, it is the unit vector at row j;
 * evals[e] = sum_k v_e[k << extendBits] * lev[k] for nEvals columns described by (buffer, width, offset, dim). */
int pil2gl_build_lev_dev(uint32_t nBits, const uint64_t xi[3], uint64_t *lev, void *stream);
typedef struct { const uint64_t *buf; uint64_t width; uint64_t offset; uint32_t dim; uint32_t levIndex; } pil2gl_eval_desc;
int pil2gl_compute_evals_dev(const pil2gl_eval_desc *descs, uint32_t nEvals, uint32_t nBits, uint32_t extendBits,
                             const uint64_t *const *levs, uint32_t nLevs, uint64_t *hostEvals /* nEvals x 3 */, void *stream);

/* ---- extension-weighted sums: the two steps that are matrix-vector products (csrc/dot.hip) ----
 * acc[r][o] (+)= sum_c buf[r][c] * coef[o][c]   (coef: host array nOut x width x 3, one extension constant per base
 * column; acc: device nRows x nOut x 3).  With coef = powers of vf2 this is the inner sum of the FRI polynomial
 * (friPolinomial.js:26-36) for every opening at once. */
int pil2gl_rows_dot_ext_dev(const uint64_t *buf, uint64_t width, uint64_t nRows, const uint64_t *hostCoef, uint32_t nOut,
                            uint64_t *acc, int accumulate, void *stream);
/* the same over nBufs matrices with the same rows -- the stage matrices and the constants the FRI polynomial walks
 * (friPolinomial.js:26-50): acc[r][o] (+)= sum_k sum_c bufs[k][r][c] * hostCoefs[k][o][c].  On the matrix cores: one pass over
 * all of them when their columns fit the kernel's staged row side by side (<= 112 columns in all, an odd width counted as the
 * next even one, <= 4 matrices); wider inputs in column windows packed into accumulating passes; three or four outputs as
 * two sweeps of two; matrices left with under 32 columns, and PIL2GL_ROWS_DOT_MFMA=0, on the vector kernels.  nOut: 1..4. */
int pil2gl_rows_dot_ext_multi_dev(const uint64_t *const *bufs, const uint64_t *widths, uint32_t nBufs, uint64_t nRows,
                                  const uint64_t *const *hostCoefs, uint32_t nOut, uint64_t *acc, int accumulate, void *stream);
/* the same sums over every 2^rowStepBits-th row: acc[r][o] (+)= sum_k sum_c bufs[k][r << rowStepBits][c] * hostCoefs[k][o][c], r < nRows,
 * acc dense (nRows x nOut x 3).  With rowStepBits = nBitsExt - nBits these are the rows of an extended matrix that lie on the coset
 * 7 <w_N>.  Same kernels and the same choice among them as the dense call (its rowStepBits = 0 case); rowStepBits: 0..20. */
int pil2gl_rows_dot_ext_multi_step_dev(const uint64_t *const *bufs, const uint64_t *widths, uint32_t nBufs, uint64_t nRows, uint32_t rowStepBits,
                                       const uint64_t *const *hostCoefs, uint32_t nOut, uint64_t *acc, int accumulate, void *stream);
/* host-only: how many launches this process has made of the three row-sum kernels behind the calls above -- out[0] the matrix-core
 * kernel, out[1] the streaming kernel, out[2] the column-tile kernel (a window of a wide matrix is a launch of its own).  The choice
 * among them hangs on widths, alignment, the device's LDS and two environment switches: the tests read the counts around a call and
 * assert which kernel took it.  Three host counters stepped at the launch sites; nothing on the device. */
int pil2gl_debug_rows_dot_launches(uint64_t out[3]);
/* f[r] = Horner in vf1 over the openings of (acc[r][o] - K_o) * xDivXSubXi[r][o]   (friPolinomial.js:38-50);
 * hostK: nOpen x 3 (K_o = sum_j ev_j vf2^(n_o - j)). */
int pil2gl_fri_combine_dev(const uint64_t *acc, const uint64_t *hostK, const uint64_t vf1[3], const uint64_t *xDivXSubXi,
                           uint32_t nOpen, uint64_t nRows, uint64_t *f, void *stream);
/* the same with the Horner order given: the k-th term is opening order[k] (host, a permutation of 0..nOpen-1; acc, hostK and
 * xDivXSubXi stay indexed by the opening's position in openingPoints).  The reference generates the terms in the order of
 * Object.keys(friExps) (friPolinomial.js:42-50): non-negative openings ascending, then negative ones as they first appear in
 * evMap -- with a previous-row opening ([-1, 0, 1]) that is 0, 1, -1, not the order of openingPoints. */
int pil2gl_fri_combine_order_dev(const uint64_t *acc, const uint64_t *hostK, const uint64_t vf1[3], const uint64_t *xDivXSubXi,
                                 uint32_t nOpen, const uint32_t *order, uint64_t nRows, uint64_t *f, void *stream);
/* The whole FRI polynomial (computeFRIStark, stark_gen_helpers.js:275-335) from the extended matrices, in one call:
 *     F(x) = Horner in vf1, in `order`, of  (sum_k sum_c bufs[k][x][c] * hostCoefs[k][o][c] - K_o) * x / (x - xi_o),   o < nOpen,
 * on all 2^nBitsExt rows of fExt (x 3).  bufs[k]: device 2^nBitsExt x widths[k]; hostCoefs[k]: nOpen x widths[k] x 3; hostK: nOpen x 3;
 * xis: nOpen x 3 (host); order: as in pil2gl_fri_combine_order_dev.
 * PRECONDITION: every column is a polynomial of degree < 2^nBits and K_o is built from the TRUE evaluations of those same columns at xi_o
 * (K_o = sum_c col_c(xi_o) * coef[o][c]).  Then each bracket vanishes at xi_o and F has degree < 2^nBits -- for any witness, satisfied
 * or not -- so F is fixed by its values on the extended rows k << (nBitsExt - nBits), the coset 7 <w_N>.  The call computes x / (x - xi),
 * the row sums and the combination on those 2^nBits rows only and extends the result (inverse transform, zero padding, plain forward
 * transform: one unshifted extension).  Exact field arithmetic, canonical words: fExt equals, word for word, what
 * x_div_x_sub_xi -> rows_dot_ext_multi -> fri_combine_order give on every row.  With any other K the two differ (F is then no polynomial
 * of that degree); the three entries above remain for that case.  nBitsExt == nBits is the full-domain sequence itself.
 * PIL2GL_EINVAL, before anything is launched or written: a base-field xi_o that is a row of the 2^nBitsExt-row domain (the rule of
 * pil2gl_x_div_x_sub_xi_dev, applied although only every 2^(nBitsExt - nBits)-th row is visited), nBitsExt < nBits, nOpen outside 1..4,
 * an order that is no permutation.  Blocks like rows_dot_ext_multi and fri_combine_order (host-side weights); the extension is only enqueued. */
int pil2gl_compute_fri_pol_dev(const uint64_t *const *bufs, const uint64_t *widths, uint32_t nBufs, const uint64_t *const *hostCoefs, uint32_t nOpen,
                               const uint64_t *hostK, const uint64_t vf1[3], const uint32_t *order, const uint64_t *xis,
                               uint32_t nBits, uint32_t nBitsExt, uint64_t *fExt, void *stream);
/* hostOut[l][c] = sum_k buf[k*rowStep][c] * levs[l][k]   (stark_gen_helpers.js:250-264 for every column of a buffer
 * and every opening at once; hostOut: nLev x width x 3, levs[l]: device nRows x 3). */
int pil2gl_cols_dot_ext_dev(const uint64_t *buf, uint64_t width, uint64_t nRows, uint64_t rowStep, const uint64_t *const *levs,
                            uint32_t nLev, uint64_t *hostOut, void *stream);
/* the same over nBufs (<= 8) matrices with the same rows in one sweep of the weights (computeEvalsStark walks every committed
 * stage and the constants, stark_gen_helpers.js:233-264): hostOuts[k] receives nLev x widths[k] x 3.  nLev: 1..64 (a sweep
 * weighs four opening points; more of them take more sweeps inside the call). */
int pil2gl_cols_dot_ext_multi_dev(const uint64_t *const *bufs, const uint64_t *widths, uint32_t nBufs, uint64_t nRows, uint64_t rowStep,
                                  const uint64_t *const *levs, uint32_t nLev, uint64_t *const *hostOuts, void *stream);
/* the same over the columns [colBegin[k], colBegin[k] + widths[k]) of matrices whose rows are strides[k] words long (colBegin null: from
 * column 0): a rank of a coset-sharded proof evaluates its share of the columns, and only those cells are read. */
int pil2gl_cols_dot_ext_range_dev(const uint64_t *const *bufs, const uint64_t *strides, const uint64_t *colBegin, const uint64_t *widths, uint32_t nBufs,
                                  uint64_t nRows, uint64_t rowStep, const uint64_t *const *levs, uint32_t nLev, uint64_t *const *hostOuts, void *stream);

/* ---- expression evaluator: src/prover/prover_helpers.js:23-259 ------------- */
/* callCalculateExps / calculateExps: run the op-list on every row of the domain.  Section pointers in
 * ctx are DEVICE pointers; prog/ctx structs themselves are host memory (copied at launch). */
int pil2gl_eval_program_dev(const glx_program *prog, const glx_ctx *ctx, void *stream);
/* ---- compile at setup, prove many times: code objects of the evaluator's run-time compiled kernels kept on disk (csrc/expr.hip) ----
 * Long programs on large domains run through a kernel hiprtc builds from the optimised op-list: 0.7 to 38 s for the programs of
 * LAB_NOTES.md 13, against 0.94 s for a whole config-3 proof.  The generated source holds no pointer, no scalar value and no row
 * count -- only the optimised op-list, the section widths, the row offsets and the form of its products -- so it is known at setup
 * and is the same for every proof.  With a cache directory set, the evaluator looks there before it compiles and stores what it
 * compiled; with none set (the default) nothing anywhere behaves differently.
 * ALL FOUR CALLS BELOW ARE HOST ONLY: they need no device, never initialise one, and run on a build host (the target is then gfx950).
 *
 * jit_cache_set_dir: NULL or "" switches the disk cache off.  Otherwise the directory is created (mode 0700) if missing; one that
 *   cannot be created or written is PIL2GL_EINVAL and the earlier setting stays.  Resets the counters.  Before the first call the
 *   setting is the environment variable PIL2GL_JIT_CACHE_DIR, read once at first use (unset: off).
 *   THE DIRECTORY HOLDS CODE THAT WILL RUN ON THE GPU: keep it private to the user who proves.  A file is only used when it belongs
 *   to geteuid(), is writable by nobody else, and passes the checks below; the library does not defend against that same user.
 * jit_cache_stats: counters since the library was loaded or the last set_dir --
 *   [0] kernels found in memory  [1] found on disk  [2] compiled  [3] files written  [4] files rejected  [5] writes that failed
 *   [6] total compile ms  [7] total ms spent looking on disk (open, read, compare, checksum)
 * One file per kernel, <dir>/<32 hex digits>.p2gl, the digits a 128-bit hash of: cache-format version, arch, the options handed to
 * hiprtcCompileProgram, hiprtcVersion, the source text.  Little-endian layout:
 *   0 magic "P2GLJIT\0"  8 u32 format version (1)  12 u32 header bytes = 64 + archLen + optsLen  16 u32 hiprtc major  20 u32 hiprtc minor
 *   24 u32 archLen  28 u32 optsLen  32 u64 srcLen  40 u64 codeLen  48 u64[2] checksum of the code bytes
 *   64 arch, options joined by '\n', the full source text, the code object
 * On a lookup every header field and the stored source must EQUAL what would be compiled now, the lengths must add up to the file's
 * size and the checksum must match; anything else counts as rejected, the kernel is compiled and the file replaced -- bytes that
 * fail a check never reach the module loader.  Files are written under a temporary name in the same directory and renamed, mode
 * 0600; a write that fails is counted and otherwise ignored (the evaluation succeeds, pil2gl_last_error is untouched).
 * Size: the source is about 25 KB of field arithmetic plus about 90 bytes per op, the code object 20-265 KB: 50 KB to 0.9 MB a kernel
 *   (119 KB for the 666-op constraint program of the bench AIR, 871 KB for a 200-slot FRI program).
 * Nothing is evicted: a directory serves one setup; delete it to start over.  pil2gl_shutdown forgets loaded modules, not files. */
int pil2gl_jit_cache_set_dir(const char *dir);
int pil2gl_jit_cache_stats(uint64_t out[8]);
/* Optimises the program for this context exactly as pil2gl_eval_program_dev does and applies the same choice of kernel (the compiled
 * one for >= 64 ops on >= 2^16 rows with <= 200 temporaries, PIL2GL_EXPR_JIT overriding); if the compiled kernel would run, makes sure
 * its code object is in the cache directory, compiling if need be.  Section pointers are not read and may be NULL; widths, nBits,
 * primeShift and the scalar pool must be what the later evaluation passes (equal scalars merge: placeholders must be pairwise
 * distinct where the real values will be -- js/prover_helpers.js precompileExps and pil2gl.stark.precompile see to that).
 * outInfo: [0] 0 interpreter / 1 compiled kernel  [1] 0 nothing to do / 1 compiled now / 2 already on disk  [2] code bytes  [3] temporaries.
 * PIL2GL_EINVAL with no cache directory set. */
int pil2gl_precompile_program(const glx_program *prog, const glx_ctx *ctx, uint32_t outInfo[4]);
/* the same for the program of pil2gl_compute_q_stark_dev, in the sub-domain context that call evaluates it in (one builder for both);
 * arguments and refusals as there, outInfo as above */
int pil2gl_precompile_q_stark(const glx_program *prog, const glx_ctx *ctx, uint32_t qSection, uint32_t nBits, uint32_t nBitsExt,
                              uint32_t qDim, uint32_t qDeg, uint32_t outInfo[4]);
/* calculateExps with debug = true (prover_helpers.js:46-70: a constraint evaluated on the rows [first, last) of its boundary, stopping
 * at the first row whose value is not zero): after the constraint's program has written its value to a column of `dim` (1 or 3) words
 * per row, *hostRow = the smallest such row (UINT64_MAX if the constraint holds on the whole range) and hostVal[0..dim) its value.
 * Blocks until the answer is on the host. */
int pil2gl_first_nonzero_row_dev(const uint64_t *col, uint32_t dim, uint64_t first, uint64_t last, uint64_t *hostRow, uint64_t *hostVal, void *stream);

/* ---- stage-2 witness hints (hints_helpers.js:91-114) ------------------------------------------------------------
 * calculateZ(F,num,den)  polutils.js:128-143: out[0] = 1, out[i] = out[i-1]*num[i-1]/den[i-1]   (num, den: n rows)
 * calculateS(F,num,den)  polutils.js:145-164: out[i] = out[i-1] + num/den[i]                    (num: ONE element)
 * dimNum/dimDen in {1,3} (base or cubic-extension columns, row-major); out has dimension 3 if either has, else 1.
 * A zero denominator yields 0 for that ratio (the reference's batchInverse would poison the whole column).
 * out must not overlap num or den. */
int pil2gl_gprod_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream);
int pil2gl_gsum_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream);
/* the grand sum with a COLUMN numerator (a pil2 gsum hint whose numerator is a multiplicity or a selector): num has n rows like den,
 * out[i] = out[i-1] + num[i]/den[i].  Dimensions, zeros, aliasing and limits as gsum's.  Only enqueues. */
int pil2gl_gsum_col_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream);
/* calculateH1H2(F,f,t)  polutils.js:105-126: the multiset f (every value must occur in t) merged into t; h1[i], h2[i] =
 * entries 2i, 2i+1 of the merged sequence.  f, t, h1, h2: n rows of dimension dim (1 or 3).  Returns PIL2GL_EINVAL with
 * the reference's "Number not included" message when some f[j] is missing from t (synchronises the stream).
 * h1 and h2 must not overlap f, t or each other. */
int pil2gl_h1h2_dev(const uint64_t *f, const uint64_t *t, uint64_t n, uint32_t dim, uint64_t *h1, uint64_t *h2, void *stream);
/* host-only, no device: how the three calls above run n rows (csrc/hint_plan.h).  outInfo[0] = lanes of a workgroup of the scan;
 * [1] = consecutive rows a lane takes (it inverts their denominators together); [2] = rows a block, [0] [1]; [3] = blocks of the first
 * pass, ceil(n / [2]); [4] = block totals a lane of the second pass (ONE workgroup) walks, ceil([3] / [0]); [5] = log2 of the capacity of
 * pil2gl_h1h2_dev's hash table, the smallest power of two >= 2 n and >= 2, or 0 for n > 2^30, which that call refuses.
 * PIL2GL_EINVAL: more than 2^31 - 1 blocks. */
int pil2gl_debug_hint_plan(uint64_t n, uint32_t *outInfo /* [6] */);
/* host-only, no device: the home slot of a key of pil2gl_h1h2_dev in a table of `capacity` slots (a power of two), from the one hash
 * function host and device share: words = dim CANONICAL 64-bit words.  UINT64_MAX for a dim other than 1 or 3, a capacity that is no
 * power of two, null words. */
uint64_t pil2gl_debug_h1h2_home(const uint64_t *words, uint32_t dim, uint64_t capacity);

/* ---- BN128 (BN254 scalar field) Merkle commitment: merklehash_bn128_p.js, merklehash_bn128_worker.js -------------
 * Field elements are 4 little-endian u64 words.  tree.nodes and leaf digests are in MONTGOMERY form (R = 2^256), exactly
 * what the reference's WASM leaves in memory (frm_toMontgomery, merklehash_bn128_worker.js:49,67,82), so files written
 * by writeToFile are interchangeable; poseidon / group proofs / roots cross the boundary in normal form like the JS
 * objects do (F.toObject, merklehash_bn128_p.js:167,241).  arity in {2,4,8,16}; Poseidon parameters for every
 * t = 2..17 are generated on first use (csrc/bn128.hip). */
/* circomlibjs poseidon(inputs[nIn], initState, nOut) -> out[nOut] for `count` independent calls (init may be NULL = 0) */
int pil2gl_bn128_poseidon(const uint64_t *in, const uint64_t *init, uint64_t count, uint32_t nIn, uint32_t nOut, uint64_t *out);
/* TranscriptBN128.put of a list (transcript.bn128.js:56-83): nBlocks full blocks of nIn elements (normal form, 4 words each)
 * absorbed one after the other, state element 0 = hostInit, then each permutation's output 0; hostOut = the nIn+1 outputs
 * of the last permutation.  One launch for the chain, 3*(nIn+1) lanes sharing each permutation. */
int pil2gl_bn128_sponge_absorb(const uint64_t *hostBlocks, uint64_t nBlocks, uint32_t nIn, const uint64_t hostInit[4], uint64_t *hostOut);
int pil2gl_bn128_poseidon_dev(const uint64_t *in, const uint64_t *init, uint64_t count, uint32_t nIn, uint32_t nOut, uint64_t *out, void *stream);
/* worker linearHash(buffIn,width,st_i,st_n,arity,custom)  merklehash_bn128_worker.js:13-100 -> height x 4 words */
int pil2gl_bn128_linear_hash_rows(const uint64_t *in, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *out);
int pil2gl_bn128_linear_hash_rows_dev(const uint64_t *in, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *out, void *stream);
/* worker merkelizeLevel(buffIn,st_i,st_n,arity)  merklehash_bn128_worker.js:104-144: arity*4 words in -> 4 words out per op */
int pil2gl_bn128_merkelize_level_dev(const uint64_t *in, uint64_t nOps, uint32_t arity, uint64_t *out, void *stream);
/* MerkleHash._getNNodes(height)  merklehash_bn128_p.js:31-45 (in nodes; tree.nodes has 4x as many u64 words) */
uint64_t pil2gl_bn128_merkle_num_nodes(uint64_t height, uint32_t arity);
/* MerkleHash.merkelize(buff,width,height)  merklehash_bn128_p.js:47-129 */
int pil2gl_bn128_merkelize(const uint64_t *elems, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *nodes);
int pil2gl_bn128_merkelize_dev(const uint64_t *elems, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *nodes, void *stream);
/* MerkleHash.getGroupProof(tree,idx)  merklehash_bn128_p.js:142-182: hostVals[width], hostSiblings[nLevels][arity][4] (normal form) */
int pil2gl_bn128_group_proof_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height, uint32_t arity,
                                 uint64_t idx, uint64_t *hostVals, uint64_t *hostSiblings, uint32_t *nLevels);
/* The same for a batch of rows in one launch (fri.js:83-105 opens every tree at every query): hostVals nIdx x width values, hostSiblings
 * nIdx x levels x arity field elements (4 words each, normal form), *nLevels = levels. */
int pil2gl_bn128_group_proofs_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height, uint32_t arity,
                                  const uint64_t *hostIdxs, uint32_t nIdx, uint64_t *hostVals, uint64_t *hostSiblings, uint32_t *nLevels);
/* verifier side: MerkleHash.calculateRootFromGroupProof  merklehash_bn128_p.js:184-232 with LinearHashBN.hash (linearhash.bn128.js:13-59)
 * for a batch of nIdx openings of one tree shape, all host pointers: hostVals nIdx x width Goldilocks words, hostSiblings nIdx x levels x
 * arity field elements (4 words each), hostRoots[q] = the root the path of leaf hostIdxs[q] leads to, normal form; verifyGroupProof
 * :234-237 is the comparison with the root.  Per opening: 3 words packed per element (the last may hold 1 or 2), no element -> 0, one ->
 * itself, else the sponge over chunks of `arity` (a short last chunk at t = nLast+1, or zero-padded when custom); per level the group of
 * `arity` siblings with position idx & (arity-1) replaced by the running value (what the proof holds there is not read), state 0, then
 * idx >>= log2(arity).  levels = 0 returns the leaf value.  Sibling words are any value < 2^256, reduced mod r (:218).
 * siblingsMontgomery = 1: the sibling words are in Montgomery form, as tree.nodes holds them (pil2gl_bn128_convert of what
 * pil2gl_bn128_group_proofs_dev returns, or a level's nodes read directly), so a prover can check openings against its own tree without
 * leaving that form; 0: normal form, as the group-proof entries above write them and as a proof carries them.
 * One launch for the whole batch, a wave per opening (csrc/bn128.hip bn_path_roots_kernel); blocks until the roots are on the host.
 * PIL2GL_EINVAL: arity not in {2,4,8,16}, levels > 40, a null buffer that would be read with nIdx > 0; nIdx = 0 is PIL2GL_OK. */
int pil2gl_bn128_roots_from_group_proofs(const uint64_t *hostVals, const uint64_t *hostSiblings, uint64_t width, uint32_t levels, uint32_t arity,
                                         int custom, int siblingsMontgomery, const uint64_t *hostIdxs, uint32_t nIdx, uint64_t *hostRoots /* nIdx x 4 */);
/* n elements between normal and Montgomery form (F.e / F.toObject); the host form is plain host arithmetic */
int pil2gl_bn128_convert(const uint64_t *in, uint64_t n, int toMontgomery, uint64_t *out);
int pil2gl_bn128_convert_dev(const uint64_t *in, uint64_t n, int toMontgomery, uint64_t *out, void *stream);

/* ---- BN254 Fr transforms: src/helpers/fft/fft_p.bn128.js, fft_worker.bn128.js (csrc/bn_ntt.hip) ----------------------------------
 * The multi-column NTT the fflonk prover runs over its committed polynomials (fflonk_prover_helpers.js:312,334, fflonk_setup.js:42).
 * An element is 4 little-endian u64 words of a * 2^256 mod r, MONTGOMERY form in and out (the bytes ffjavascript's Fr keeps in its
 * buffers, and the form of tree.nodes above).  Inputs must be canonical (< r); they are not validated.  Row-major: element (row j,
 * polynomial i) at word (j*nPols + i)*4 (test/fft_p.bn128.test.js:28).  Roots of unity are ffjavascript's Fr.w[]: w[28] =
 * 5^((r-1)/2^28), w[k] = w[k+1]^2.  nBits <= nBitsExt <= 28, else PIL2GL_EINVAL; nBits = 0 copies the row.  Argument errors are
 * reported before any device call; the compute entries return PIL2GL_ENODEV without a device.  The _dev forms take device pointers
 * (16-byte aligned) and only enqueue on the caller's stream; the others take host pointers and stage through device copies.
 * Two exceptions to "only enqueue", both on FIRST use: the twiddle tables of a size and direction are allocated and uploaded with a
 * synchronous copy, and the working buffer of a transform of more than 2^10 rows is (re)allocated, with a device synchronise, when it
 * has to grow -- make one call of the largest size before capturing a stream into a graph.  That working buffer is one per process, as
 * every scratch buffer of this library is (one caller at a time, any stream): two transforms of more than 2^10 rows must not be in flight
 * on different streams at once. */
/* fft(buffSrc, nPols, nBits, buffDst, Fr)  fft_p.bn128.js:178-223: dst[j] = sum_k src[k] w[nBits]^(jk), natural order in and out; dst may be src */
int pil2gl_bn128_fft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst);
/* ifft(...)  fft_p.bn128.js:58-71,178-223 (invBitReverse): dst[k] = 1/n sum_j src[j] w[nBits]^(-jk); dst may be src */
int pil2gl_bn128_ifft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst);
/* interpolate(buffSrc, nPols, nBits, buffDstCoefs, buffDst, nBitsExt, Fr)  fft_p.bn128.js:225-285: dstCoefs (2^nBits rows; may be NULL)
 * = ifft(src), scaled by 1/n (:265-266); dst (2^nBitsExt rows) = fft of the coefficients padded with zero rows.  NO coset shift
 * (fft_worker.bn128.js:15-22 never advances its factor).  dst and dstCoefs must not overlap each other or src. */
int pil2gl_bn128_interpolate(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dstCoefs, uint64_t *dst, uint32_t nBitsExt);
int pil2gl_bn128_fft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream);
int pil2gl_bn128_ifft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream);
int pil2gl_bn128_interpolate_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dstCoefs, uint64_t *dst, uint32_t nBitsExt, void *stream);
/* host-only, no device: the sweeps over global memory a transform of 2^nBits rows makes (the replacement of fft_p.bn128.js:200-221's
 * block loop): *nSweeps of them, layersPerSweep[i] butterfly layers in sweep i (room entries available; 3 always suffice), summing to
 * nBits.  A sweep of K layers keeps 2^K rows x min(nPols, tile_bytes / 32 >> K) columns in LDS; pil2gl_debug_bn128_fft_tile_bytes is that
 * limit.  nBits = 0 has no sweep; nBits > 28 is PIL2GL_EINVAL. */
int pil2gl_debug_bn128_fft_plan(uint32_t nBits, uint32_t *layersPerSweep, uint32_t room, uint32_t *nSweeps);
uint32_t pil2gl_debug_bn128_fft_tile_bytes(void);

/* ---- BN254 G1 multi-scalar multiplication: G1.toAffine(G1.multiExpAffine(bases, scalars)) (csrc/bn_msm.hip) ----------------------
 * The commitment step of the fflonk prover (commit(..., {multiExp: true}): fflonk_prover_helpers.js:185,336, fflonk_setup.js:52):
 * out = sum_i scalars[i] * bases[i] on y^2 = x^3 + 3 over Fq, generator (1, 2) of order r.  Byte formats are ffjavascript's:
 *   bases    n affine points, 8 little-endian u64 each: x then y, Fq MONTGOMERY form (a * 2^256 mod q), as ptau section 2 / zkey.pTau
 *            holds them.  Infinity is 64 zero bytes (G1.zeroAffine).  Coordinates must be canonical (< q); membership of the curve is NOT
 *            validated.
 *   scalars  element i is the 4 words at word 4 * i * scalarStride: a column of a row-major coefficient matrix of nPols columns commits
 *            with scalarStride = nPols and no gather (the copy loop of fflonk_prover_helpers.js:326-331).  scalarsMontgomery != 0: Fr
 *            Montgomery words, what pil2gl_bn128_ifft leaves (any value < 2^256, reduced mod r); 0: normal form, canonical (< r), what
 *            multiExpAffine itself takes after Fr.batchFromMontgomery.  A normal-form scalar >= r gives an unspecified point (no fault).
 *   out      one affine point in the format of bases; n = 0 and an empty sum give 64 zero bytes.
 * 0 <= n <= 2^28 and 1 <= scalarStride < 2^32, else PIL2GL_EINVAL; so is a null buffer (bases / scalars only with n > 0).  Argument
 * errors are reported before any device call; without a device the entries return PIL2GL_ENODEV (the host form with n = 0 needs none).
 * The _dev form takes device pointers (bases and scalars 16-byte aligned, out 8-byte), only enqueues on the caller's stream and writes
 * out on the device.  One exception, on FIRST use, as for the transforms above: the working buffer (pil2gl_debug_bn128_msm_plan's
 * scratchBytes) is (re)allocated, with a device synchronise, when it has to grow -- make one call of the largest n before capturing a
 * stream into a graph; it is one per process, so two MSMs must not be in flight on different streams at once.  The host form stages
 * bases, the scalars up to the last one read, and out through device copies. */
int pil2gl_bn128_g1_msm(const uint64_t *bases, const uint64_t *scalars, uint64_t n, uint64_t scalarStride, uint32_t scalarsMontgomery, uint64_t *out);
int pil2gl_bn128_g1_msm_dev(const uint64_t *bases, const uint64_t *scalars, uint64_t n, uint64_t scalarStride, uint32_t scalarsMontgomery,
                            uint64_t *out, void *stream);
/* host-only, no device: how an MSM of n points runs.  out[0] = c, the window width in bits; [1] = nWindows = ceil(255 / c); [2] = buckets
 * per window = 2^(c-1) (signed digits); [3] = windows whose point lists are built and accumulated per pass.  *scratchBytes = the working
 * buffer, at most 4 * clamp(8 n, 2^19, 2^30) + 96 MiB (0 for n = 0).  n > 2^28 is PIL2GL_EINVAL.  The batch of one polynomial. */
int pil2gl_debug_bn128_msm_plan(uint64_t n, uint32_t *out, uint64_t *scratchBytes);
/* ---- BN254 G1 stage commit: K packed polynomials over the same bases in one call (csrc/bn_msm.hip, csrc/bn_msm_batch.h) -----------
 * What fflonk's commit(stage, ...) computes for a stage (extendAndCommit, fflonk_prover_helpers.js:303-336; computeQFflonk's commit,
 * :185; fflonk_setup.js:52) straight from the row-major coefficient matrix pil2gl_bn128_ifft left: no packed copy of the polynomials is
 * built.  Packed polynomial k is fflonk's CPolynomial f_k(X) = sum_j X^j p_j(X^m): it has n_k = m_k * rows_k coefficients; coefficient
 * i sits in slot j = i mod m_k and row t = i div m_k, and is 0 when the slot is empty, else element
 * polys[k].first + t * rowStride + slot (elements of 4 words).  Polynomial k's m_k slots are the next m_k entries of `slots`, each a
 * column index below rowStride or PIL2GL_G1_EMPTY_SLOT.  out[8 k ..] = toAffine(sum_i coef_k[i] * bases[i]) in the format above, all
 * zero for the empty sum; every polynomial indexes bases from 0.  m = 1 with one slot is the strided MSM above; rowStride = 1, m = 1 and
 * different `first` commits pieces of one coefficient vector.  Formats of bases and scalars, scalarsMontgomery, the alignment of the
 * _dev form, its enqueue-only behaviour and the shared working buffer (pil2gl_debug_bn128_msm_batch_plan's scratchBytes) are those of
 * pil2gl_bn128_g1_msm.
 * Refused with PIL2GL_EINVAL before any device call, nothing written: K outside 1..16; m_k outside 1..64; sum m_k > 256;
 * n_k > nBases; sum n_k > 2^28; rowStride outside 1..2^32-1; first >= 2^58; a slot that is neither the marker nor below rowStride; a
 * null polys, slots or out, null bases with a point, null scalars with a slot in use.  rows_k = 0 is legal (the zero point); a batch
 * without any point needs no device in the host form.  The host form stages the bases up to the largest n_k, the scalars up to the last
 * element any descriptor reaches, and out through device copies; neither form can check how far bases and scalars extend. */
#define PIL2GL_G1_EMPTY_SLOT 0xFFFFFFFFu
typedef struct { uint64_t first, rows; uint32_t m, reserved; } pil2gl_g1_poly;
int pil2gl_bn128_g1_commit(const uint64_t *bases, uint64_t nBases, const uint64_t *scalars, uint64_t rowStride, uint32_t scalarsMontgomery,
                           const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t *out);
int pil2gl_bn128_g1_commit_dev(const uint64_t *bases, uint64_t nBases, const uint64_t *scalars, uint64_t rowStride, uint32_t scalarsMontgomery,
                               const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t *out, void *stream);
/* host-only, no device: how a batch of K MSMs of counts[k] points runs: out[0..3] as pil2gl_debug_bn128_msm_plan's, one window width for
 * the batch (from the largest count, lowered while K * out[1] * out[2] bucket points exceed 9 * 2^19) and out[3] windows per pass (from the
 * total count, K * out[3] * out[2] <= 2^18 histogram cells).  *scratchBytes = the working buffer, at most
 * 4 * clamp(8 N, 2^19, 2^30) + 96 MiB * min(K, 9), N the total count (0 for N = 0).  K = 1 equals pil2gl_debug_bn128_msm_plan.
 * K outside 1..16 or N > 2^28 is PIL2GL_EINVAL. */
int pil2gl_debug_bn128_msm_batch_plan(uint32_t K, const uint64_t *counts, uint32_t *out, uint64_t *scratchBytes);
/* host-only, no device: where point lane `lane` of a batch (described as for pil2gl_bn128_g1_commit) lies, by the code the kernels run:
 * out[0] = k, out[1] = i, out[2] = 1 and out[3] = the scalar's element offset, or out[2] = out[3] = 0 for an empty slot.  A lane at or
 * past sum n_k and every descriptor the commit refuses (n_k is checked against 2^28 only) is PIL2GL_EINVAL. */
int pil2gl_debug_bn128_commit_locate(const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t rowStride, uint64_t lane, uint64_t out[4]);
/* host-only, no device: the signed digits the kernels split a scalar into (normal form, below 2^254) for windows of c bits, least
 * significant first, by the code the kernels run: *nDigits = ceil(255 / c) of them (room entries available), each in
 * [-(2^(c-1) - 1), 2^(c-1)], sum_w digits[w] 2^(c w) = scalar.  c outside 4..16, a larger scalar or too little room: PIL2GL_EINVAL
 * (the count still comes back in the last case). */
int pil2gl_debug_bn128_msm_digits(const uint64_t scalar[4], uint32_t c, int32_t *digits, uint32_t room, uint32_t *nDigits);

/* ---- BN254 Fr expression evaluator: calculateExps over curve.Fr (csrc/bn_expr.hip, include/pil2gl_bn_expr.h) ----------------------
 * The row loop the fflonk final prover runs between two commitments (src/prover/prover.js:212-219; prover_helpers.js:31-72
 * calculateExps, :83-107 compileCode, :109-259 setRef / getRef / evalMap; fflonk_prover_worker.js:5-41): the op-list is evaluated for
 * every row i of a domain of 2^nBits rows, an operand with row offset `prime` at row (i + prime * 2^primeShift) mod 2^nBits.  Elements
 * are 4 little-endian u64 words, MONTGOMERY form and canonical (< r) in and out, never converted: what pil2gl_bn128_ifft leaves and
 * what pil2gl_bn128_fft / pil2gl_bn128_g1_msm(scalarsMontgomery = 1) take.  Inputs are not validated against r.  add / sub / mul / copy
 * on single elements; the operand classes, counted in elements, are in pil2gl_bn_expr.h.  Sections must not overlap each other.
 * Refused with PIL2GL_EINVAL before any device call: a null program, context, op-list, section table, or the null pointer of a section
 * or scalar pool that an op names; dim != 1; op above GLX_OP_COPY; a section, column, scalar or tmp out of range; a tmp read before it is
 * written; a scalar as destination; more than PIL2GL_BNX_MAX_SECTIONS sections; nBits or primeShift > 28; prime * 2^primeShift beyond 32
 * bits; a column that the program writes and also reads where any of those accesses has a non-zero row offset, or that it writes at two
 * different offsets (the reference's serial row loop makes that order-dependent; a lane per row would make it a race).  Reading and
 * writing one cell at offset 0 (x = x * x) is fine.  Without a device the compute entries then return PIL2GL_ENODEV.
 * The _dev form takes device sections (16-byte aligned).  Blocking behaviour: the op-list and the scalar pool are host temporaries; they
 * are staged with one pageable-memory copy on the caller's stream, which the runtime completes before the call returns (so it waits for
 * earlier work on that stream), and the kernel is only ENQUEUED: the call does not wait for it, and the next call on the same stream may
 * follow at once.  One exception, on FIRST use, as for the transforms: the working buffer (program, scalar pool, and temporaries when
 * more than the LDS limit are live) is (re)allocated, with a device synchronise, when it has to grow.  It is one per process: two
 * evaluations must not be in flight on different streams at once.  The host form stages the sections the program names through device
 * copies and copies back the ones it writes. */
int pil2gl_bn128_eval_program(const glx_program *prog, const bnx_ctx *ctx);
int pil2gl_bn128_eval_program_dev(const glx_program *prog, const bnx_ctx *ctx, void *stream);
/* calculateExps with debug = true over Fr (prover_helpers.js:46-70, fflonk_prover_worker.js:19-26): after a constraint's program has
 * written its value to column `column` of a device section `width` elements wide, *hostRow = the smallest row of [first, last) whose
 * element is not zero (all eight 32-bit words decide), hostVal[0..4) = that element (Montgomery words); UINT64_MAX and zeros if there is
 * none.  last <= 2^28.  Blocks until the answer is on the host. */
int pil2gl_bn128_first_nonzero_row_dev(const uint64_t *col, uint64_t width, uint64_t column, uint64_t first, uint64_t last,
                                       uint64_t *hostRow, uint64_t *hostVal, void *stream);
/* host-only, no device: how pil2gl_bn128_eval_program_dev would run the program, after the same checks.  outInfo[0] = temporary slots
 * after value numbering and live-range renumbering (each distinct cell loaded once, common sub-expressions merged), [1] = ops after
 * those passes, [2] = kernel form: 0 temporaries in LDS, 1 in the global working buffer, [3] = the LDS slot limit (form 0 up to and
 * including it), [4] = lanes of one launch (threads * resident workgroups: a larger domain takes the grid-stride loop again),
 * [5] = threads per workgroup. */
int pil2gl_debug_bn128_plan_program(const glx_program *prog, const bnx_ctx *ctx, uint32_t *outInfo /* [6] */);

/* ---- BN254 Fr polynomial division by x^k - beta and evaluation (csrc/bn_poly.hip) ---------------------------------------------------
 * The long-vector field work of the fflonk prover's last two steps: Q.divZh(N, 2^extendBits) of computeQFflonk
 * (fflonk_prover_helpers.js:147-148) and, in computeOpeningsFflonk's shplonkjs open (:212), the divisions by x^k - h^k and x - y and the
 * evaluations of the committed polynomials at their opening points.  For a coefficient vector c[0..n), k >= 1 and a field element beta,
 *     d[i] = c[i] + beta * d[i + k]     (d[j] = 0 for j >= n),   i.e.  d[i] = sum_{t >= 0} beta^t c[i + t k]:
 * d[k..n) is the quotient of c by x^k - beta, quotient coefficient m at position m + k, and d[0..k) is the remainder.  k = N, beta = 1 is
 * divZh: for a divisible polynomial the quotient, found from position N on, is the one the reference computes from the low end.  There is
 * no "not divisible" entry: the caller runs pil2gl_bn128_first_nonzero_row_dev(dst, stride, 0, 0, k) on the remainder positions (the
 * reference throws "Polynomial is not divisible").  k = 1, beta = z is division by x - z with d[0] = p(z); poly_eval computes only that,
 * out[p] = sum_i c[i] points[p]^i for nPoints points, and reads src only.
 *   Addressing  element i is the 4 words at word 4 * i * stride, for src and dst alike: a column of a row-major matrix is processed where
 *               it lies (as g1_msm's scalarStride), and the words between a strided destination's elements are left as they are.
 *   Aliasing    dst == src is allowed (position i depends on c[i] and on positions above it); any other overlap is not.
 *   beta, points  HOST pointers, 4 words per element, MONTGOMERY form and canonical (a challenge comes from the host transcript).
 *               Coefficients are Montgomery words, canonical in and out, never converted: what pil2gl_bn128_ifft leaves.
 *   Limits      0 <= n <= 2^28, 1 <= stride < 2^32, 1 <= k <= 2^28, 1 <= nPoints <= 64; anything else, and a null buffer (src / dst only
 *               with n > 0), is PIL2GL_EINVAL before any device call.  k >= n copies; n = 0 writes nothing, and poly_eval gives zeros.
 *               Without a device the compute entries return PIL2GL_ENODEV (the host forms with n = 0 need none).
 * The _dev forms take device pointers (16-byte aligned; out: nPoints elements on the device) and only ENQUEUE on the caller's stream,
 * after staging the levels' multipliers (powers of beta computed on the host, at most 16 KiB) with one pageable-memory copy on that
 * stream, which the runtime completes before the call returns.  One exception, on FIRST use, as for every BN254 block above: the working
 * buffer (pil2gl_debug_bn128_poly_plan's scratchBytes; poly_eval: 16 KiB + nPoints times the rest) is (re)allocated, with a device
 * synchronise, when it has to grow; it is one per process, so two of these calls must not be in flight on different streams at once.
 * The host forms stage src up to its last element, and a strided dst that is not src, through device copies. */
int pil2gl_bn128_poly_div_xk_sub(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t k, const uint64_t hostBeta[4], uint64_t *dst);
int pil2gl_bn128_poly_div_xk_sub_dev(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t k, const uint64_t hostBeta[4], uint64_t *dst, void *stream);
int pil2gl_bn128_poly_eval(const uint64_t *src, uint64_t n, uint64_t stride, const uint64_t *hostPoints, uint32_t nPoints, uint64_t *out);
int pil2gl_bn128_poly_eval_dev(const uint64_t *src, uint64_t n, uint64_t stride, const uint64_t *hostPoints, uint32_t nPoints, uint64_t *out, void *stream);
/* host-only, no device: how poly_div_xk_sub runs (n, k); poly_eval runs as (n, 1).  The k chains of M = ceil(n / k) links are cut into
 * segments, a lane each.  outInfo[0] = L, links per segment; [1] = S, segments per chain (L * S * k >= n); [2] = carry levels, the times
 * the same recurrence is applied to the segment values (0 when S = 1); [3] = threads per workgroup; [4] = the form: 0 a lane per chain
 * (M <= 32, or k >= 2^17 lanes), 1 segmented.  *scratchBytes = the working buffer: 16 KiB of multipliers, and the segment values of all
 * levels, below 9 MiB (none in form 0).  The carry-level count stops growing at n = 2^22.  n or k out of range: PIL2GL_EINVAL. */
int pil2gl_debug_bn128_poly_plan(uint64_t n, uint64_t k, uint32_t *outInfo /* [5] */, uint64_t *scratchBytes);

/* ---- BN254 Fr products with a sparse polynomial, scaled sums and the degree (csrc/bn_polymul.hip) -----------------------------------
 * What shplonkjs open (computeOpeningsFflonk, fflonk_prover_helpers.js:212) does on its longest vectors between the evaluations and the
 * divisions of the block above: the Polynomial class's add, sub, mulScalar, byXSubValue, byXNSubValue and degree, which build
 * W = sum_i alpha^i (f_i - r_i) Z_{T\S_i} and L = sum_i alpha^i Z_{T\S_i}(y) (f_i - r_i(y)) - Z_T(y) W.  One form covers the first five:
 *     acc[i] <- s * acc[i] + sum_{j < t} m[j] * src[i - e[j]]     for 0 <= i < nAcc,   src[x] = 0 for x < 0 or x >= nSrc,
 * the product of src by M(x) = sum_j m[j] x^e[j] added to the scaled accumulator.  add / sub: t = 1, m = 1 / r - 1, s = 1.  mulScalar:
 * t = 1, s = NULL, acc the same column as src.  byXSubValue(v): {(-v, 0), (1, 1)}; byXNSubValue(n, v): {(-v, 0), (1, n)}.  A zerofier
 * prod_j (x^k_j - beta_j) multiplied out on the host is ONE call instead of one per factor, and W += alpha^i Z f_i is one call.
 * poly_degree stores the largest i whose 32 bytes are not all zero, or UINT64_MAX for the zero polynomial and for n = 0.
 *   Addressing  element i of a column is the 4 words at word 4 * i * stride, acc and src each with a stride of its own; the words between a
 *               strided acc's elements are left as they are.  Montgomery words, canonical in and out, never converted, not validated.
 *   hostScale   a HOST pointer to 4 Montgomery words, or NULL: then acc is written and NEVER READ (it may hold anything).
 *   hostCoefs, hostExps   HOST pointers: t elements of 4 Montgomery words, and t exponents, strictly increasing.  Zero coefficients are
 *               dropped on the host; the kernel sees the compacted list.
 *   Aliasing    acc must share no element with src, by the rule of the scan block below (byte ranges apart, or two columns of one section).
 *               One exception: with t = 1 and e[0] = 0 the operation is elementwise and acc may be the SAME column as src.  A shifted
 *               product in place is refused: the caller alternates two buffers, as the reference's byXSubValue does with its new buffer.
 *   Limits      0 <= nAcc, nSrc <= 2^28, 1 <= stride < 2^32, 1 <= t <= 64, e[t-1] <= 2^28, and nSrc > 0 implies nSrc + e[t-1] <= nAcc (a
 *               product is never truncated); anything else, and a null buffer with a non-zero count (hostCoefs, hostExps, degree: always),
 *               is PIL2GL_EINVAL before any device call.  nAcc = 0 is PIL2GL_OK and needs no device; nSrc = 0 only scales, or zero-fills
 *               with hostScale NULL.  Without a device the entries return PIL2GL_ENODEV.
 * The _dev forms take device pointers (16-byte aligned; anything else is PIL2GL_EINVAL, also before any device call).  poly_fma_dev only
 * ENQUEUES one kernel on the caller's stream: the term list travels as kernel arguments, there is no copy, no readback and no working
 * buffer.  poly_degree_dev enqueues and BLOCKS for the 8-byte readback, as pil2gl_bn128_first_nonzero_row_dev does.  The host forms
 * stage every column up to its last element through device copies (columns whose ranges meet as one range). */
int pil2gl_bn128_poly_fma(uint64_t *acc, uint64_t nAcc, uint64_t accStride, const uint64_t *hostScale /* [4] or NULL */,
                          const uint64_t *src, uint64_t nSrc, uint64_t srcStride,
                          const uint64_t *hostCoefs /* [4 t] */, const uint64_t *hostExps /* [t] */, uint32_t t);
int pil2gl_bn128_poly_fma_dev(uint64_t *acc, uint64_t nAcc, uint64_t accStride, const uint64_t *hostScale /* [4] or NULL */,
                              const uint64_t *src, uint64_t nSrc, uint64_t srcStride,
                              const uint64_t *hostCoefs /* [4 t] */, const uint64_t *hostExps /* [t] */, uint32_t t, void *stream);
int pil2gl_bn128_poly_degree(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t *degree);
int pil2gl_bn128_poly_degree_dev(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t *degree, void *stream);

/* ---- BN254 Fr grand product, grand sum and batch inverse: the gprod / gsum hints over curve.Fr (csrc/bn_scan.hip) -----------------
 * What resolves the hints of a fflonk stage with a permutation, connection or lookup argument (src/prover/hints_helpers.js:92-113):
 * calculateZ and calculateS of src/helpers/polutils.js:132-164 with F = curve.Fr, each one F.batchInverse and a serial walk of n products.
 *     batch_inverse   dst[i] = src[i]^-1
 *     gprod           out[0] = 1 (Montgomery form), out[i] = out[i-1] * num[i-1] / den[i-1]          (calculateZ)
 *     gsum            out[i] = out[i-1] + num / den[i], out[0] = num / den[0]; num is ONE element      (calculateS)
 * The `result` field of a hint is out[n-1]: the caller copies those 32 bytes, there is no entry for it.
 *   Addressing  element i of a column is the 4 words at word 4 * i * stride, each column with a stride of its own: a column of a row-major
 *               section is read and written where it lies, and the words between a strided destination's elements are left as they are.
 *               Montgomery words, canonical in and out, never converted; inputs are not validated against r.
 *   Zeros       A stated choice: the reference's Fr is ffjavascript's wasm field, which the reference tree does not carry, so what its
 *               batchInverse makes of a zero cannot be pinned.  The convention of the Goldilocks hints above and of the MSM's Fq inversion
 *               holds: a zero inverts to ZERO and is kept out of every running product (it spoils no other row).  In gprod a zero
 *               denominator makes that row's ratio 0, so every later row is 0; in gsum the row adds 0.  A zero numerator is plain arithmetic.
 *   Aliasing    A column is (pointer, stride).  batch_inverse may run in place: dst the SAME column as src.  Otherwise an output must share
 *               no element with an input: columns whose byte ranges are apart, or columns of equal stride whose pointers differ by a
 *               multiple of 32 bytes that is no multiple of 32 * stride bytes (two columns of one section: the ranges interleave, no
 *               element is shared).  Ranges that meet in any other way -- different strides included -- are PIL2GL_EINVAL, a host check.
 *   hostNum     gsum's numerator: a HOST pointer to 4 Montgomery words in both forms.
 *   Limits      0 <= n <= 2^28, 1 <= stride < 2^32; anything else, and a null buffer with n > 0 (hostNum: always), is PIL2GL_EINVAL
 *               before any device call.  n = 0 is PIL2GL_OK, touches nothing and needs no device.  Without a device the entries return
 *               PIL2GL_ENODEV.
 * The _dev forms take device pointers (16-byte aligned) and only ENQUEUE on the caller's stream; nothing is staged.  One exception, on
 * FIRST use, as for every BN254 block above: the working buffer (pil2gl_debug_bn128_scan_plan's scratchBytes) is (re)allocated, with a
 * device synchronise, when it has to grow; it is one per process, so two of these calls must not be in flight on different streams at
 * once.  The host forms stage every column up to its last element (a strided destination too) through device copies. */
int pil2gl_bn128_batch_inverse(const uint64_t *src, uint64_t srcStride, uint64_t n, uint64_t *dst, uint64_t dstStride);
int pil2gl_bn128_batch_inverse_dev(const uint64_t *src, uint64_t srcStride, uint64_t n, uint64_t *dst, uint64_t dstStride, void *stream);
int pil2gl_bn128_gprod(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                       uint64_t *out, uint64_t outStride);
int pil2gl_bn128_gprod_dev(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                           uint64_t *out, uint64_t outStride, void *stream);
int pil2gl_bn128_gsum(const uint64_t hostNum[4], const uint64_t *den, uint64_t denStride, uint64_t n, uint64_t *out, uint64_t outStride);
int pil2gl_bn128_gsum_dev(const uint64_t hostNum[4], const uint64_t *den, uint64_t denStride, uint64_t n,
                          uint64_t *out, uint64_t outStride, void *stream);
/* gsum with a COLUMN numerator: out[i] = out[i-1] + num[i] / den[i], num a column of n elements like gprod's.  Addressing, zeros,
 * aliasing (out shares no element with num or den), limits and the two forms as gprod's. */
int pil2gl_bn128_gsum_col(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                          uint64_t *out, uint64_t outStride);
int pil2gl_bn128_gsum_col_dev(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                              uint64_t *out, uint64_t outStride, void *stream);
/* host-only, no device: how the three run on n rows.  op: 0 batch_inverse, 1 gprod, 2 gsum, 3 batch_inverse in place.  The rows are cut
 * into segments, a lane each; the segment totals are the same problem one level up, until a level has at most 64 items, which one lane
 * finishes (the inversion's single Fermat ladder is there).  outInfo[0] = L, rows per segment; [1] = S, segments (L * S >= n,
 * (S - 1) * L < n); [2] = levels (1 for n <= 64; first 2, 3, 4, 5 at n = 65, 1025, 16385, 262145; never more); [3] = threads per
 * workgroup; [4] = segments per workgroup (a workgroup's share is L times this many rows).  *scratchBytes = the working buffer: the levels
 * above the first, below 9 MiB, and 32 * n more for op 3 only (an inversion in place has nowhere else to keep its prefix products); 0 for
 * n = 0.  n > 2^28 or op > 3: PIL2GL_EINVAL. */
int pil2gl_debug_bn128_scan_plan(uint64_t n, uint32_t op, uint32_t *outInfo /* [5] */, uint64_t *scratchBytes);

/* ---- BN254 Fr plookup hint: calculateH1H2 over curve.Fr (csrc/bn_h1h2.hip) ---------------------------------------------------------
 * The last branch of resolveHint (src/prover/hints_helpers.js:115-121): calculateH1H2(F, f, t) of src/helpers/polutils.js:105-130, which
 * uses no field arithmetic.  f and t have n elements each.  Two elements are the same value exactly when their 32 bytes are equal (the
 * reference keys an object by the bytes).  With last(v) the largest i with t[i] = v, and cnt[i] = #{j : f[j] = t[i]} if i = last(t[i])
 * and 0 otherwise, the merged sequence s is t[0] repeated 1 + cnt[0] times, then t[1] repeated 1 + cnt[1] times, and so on: 2 n
 * elements; h1[i] = s[2i], h2[i] = s[2i+1].  (t = [a, b, a], f = [a, a, b]: s = a, b, b, a, a, a; h1 = [a, b, a], h2 = [b, a, a] -- the
 * counts of a duplicated value go to its LAST occurrence.)  The result does not depend on the order in which atomics land.
 *   Missing     If some f[j] is not in t the call returns PIL2GL_EINVAL with the message "Number not included: w:<j>", j the lowest such
 *               index, also stored through missingRow (which may be NULL, and holds UINT64_MAX on success and on every other refusal).
 *               Then no word of h1 or h2 has been written: the step that writes them is launched only after the check.
 *   Addressing  element i of a column is the 4 words at word 4 * i * stride, f, t, h1 and h2 each with a stride of its own; the words
 *               between a strided output's elements are left as they are.  Montgomery words as curve.Fr keeps them, expected canonical,
 *               not validated, never converted.
 *   Aliasing    An output must share no element with an input or with the other output, by the rule of the scan block above: byte ranges
 *               apart, or two columns of one section (equal strides, pointers a multiple of 32 bytes apart that is no multiple of
 *               32 * stride).  Any other overlap -- the same column included -- is PIL2GL_EINVAL, a host check.  f and t may be anything.
 *   Limits      0 <= n <= 2^28, 1 <= stride < 2^32; anything else, and a null buffer with n > 0, is PIL2GL_EINVAL before any device
 *               call.  n = 0 is PIL2GL_OK, touches nothing (missingRow aside) and needs no device.  Without a device: PIL2GL_ENODEV.
 * The _dev form takes device pointers (16-byte aligned; anything else is PIL2GL_EINVAL, also before any device call), enqueues on the
 * caller's stream and BLOCKS for the 8-byte readback of the missing cell; what writes h1 and h2 is enqueued after it and not waited
 * for.  As for every BN254 block above, the working buffer
 * (pil2gl_debug_bn128_h1h2_plan's scratchBytes) is (re)allocated, with a device synchronise, when it has to grow; it is one per process,
 * so two of these calls must not be in flight on different streams at once.  All of it is cleared or written by every call.  The host
 * form stages every column up to its last element (strided outputs too) through device copies. */
int pil2gl_bn128_h1h2(const uint64_t *f, uint64_t fStride, const uint64_t *t, uint64_t tStride, uint64_t n,
                      uint64_t *h1, uint64_t h1Stride, uint64_t *h2, uint64_t h2Stride, uint64_t *missingRow);
int pil2gl_bn128_h1h2_dev(const uint64_t *f, uint64_t fStride, const uint64_t *t, uint64_t tStride, uint64_t n,
                          uint64_t *h1, uint64_t h1Stride, uint64_t *h2, uint64_t h2Stride, uint64_t *missingRow, void *stream);
/* host-only, no device: how the hint runs on n rows.  outInfo[0] = the table's capacity in 4-byte slots, the power of two with
 * 2 n <= capacity < 4 n (2 for n <= 1); [1] = threads per workgroup; [2] = the scan chunk: groups (rows of t) per workgroup of the local
 * scan; [3] = that scan's workgroups, ceil(n / chunk); [4] = output rows per workgroup of the expand step; [5] = its workgroups.
 * *scratchBytes = the working buffer (table, counts / group starts, chunk totals, missing cell): below 20 n + n / 512 + 64 bytes for
 * every n, 3 GiB + 512 KiB + 16 bytes at n = 2^28; 0 for n = 0.  n > 2^28: PIL2GL_EINVAL. */
int pil2gl_debug_bn128_h1h2_plan(uint64_t n, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);

/* ---- recursion witness: the additions and the sMap gather of the *_exec step (csrc/wtns_exec.hip, csrc/wtns_plan.h) ---------------
 * compressorExec (src/compressor/compressor_exec.js:5-32) over Goldilocks and the loop of src/final/main_final_exec.js:50-67 over the
 * BN254 scalar field Fr (also test/plonk2pil/main_plonkexec.js) turn the circom witness w into the N x nCols trace:
 *   additions   for i = 0 .. nAdds - 1 in order: w[nWitness + i] = w[a_i] ca_i + w[b_i] cb_i in the field; a_i, b_i may name an earlier
 *               addition.  An operand >= nWitness + i is PIL2GL_EINVAL naming i (the reference would read `undefined`).
 *   gather      dst[i dstCols + j] = (s = sMap[i nCols + j]) ? w[s] : 0 for j < nCols, and 0 for nCols <= j < dstCols (the widening rule
 *               of land_rows above).  Index 0 means zero, not w[0].  nRows (the file's nSMap) rows are written.
 * An element is one u64 (Goldilocks) or four u64 (Fr); nW = nWitness + nAdds must stay below 2^32 (the reference's sMap is Uint32Array,
 * compressor18_setup.js:62).  Goldilocks: witness and coefficient words in [p, 2^64) count as their value mod p; outputs are canonical.
 * Fr: w holds NORMAL-form values, 32 bytes little-endian (what circom's calculator and a .wtns hold); the coefficients are Montgomery
 * words, as the exec file's section 4 holds them (final/exec_helpers.js:150-165); any 256-bit pattern counts as its value mod r; the
 * additions leave normal-form canonical values in w; the trace is written in Montgomery form when toMontgomery is non-zero (what
 * writeToBigBufferFr, src/prover/prover.js:27, leaves in cm1_n and fft_p_bn128 reads) and in normal form otherwise, canonical either way.
 *
 * pil2gl_wtns_adds_plan: host-only, no device.  Addition i has its operands at hostAddIdx[idxStride i], [idxStride i + 1] and its two
 * coefficients, coefWords (1 or 4) words each, at hostCoef[coefStride i ..] -- a compressor .exec: addsBuff, 4, addsBuff + 2, 4; a final
 * .exec: section 3, 2, section 4, 8.  level(i) = 0 when both operands are below nWitness, else 1 + the highest level among its operands
 * that are additions.  With every output NULL the call validates and returns *nLevels.  Otherwise outLevelStart (levelCap >= nLevels + 1
 * entries) and outAdds (4 nAdds words) receive the additions sorted by level, stable within a level, as (a, b, dst = nWitness + i, i),
 * level l being records [outLevelStart[l], outLevelStart[l + 1]); outCoef (2 coefWords nAdds words, may be NULL) the coefficients
 * permuted alike.  The device runs ONE LAUNCH PER LEVEL: a chain of depth D costs D launches (r1cs2plonk.js:49-67 reduces a linear
 * combination through a queue, so depth grows like log2 of the longest combination).
 * pil2gl_[bn128_]wtns_adds_dev: w (device, nW elements, the first nWitness filled), adds / coefs (device, the plan's outAdds / outCoef,
 * 16-byte aligned), hostLevelStart (HOST, checked: starts at 0, ascends, ends at nAdds).  Enqueues only.  A record whose a or b is >= nW or
 * whose dst is outside [nWitness, nW) writes nothing.  w overlapping a table is PIL2GL_EINVAL.
 * pil2gl_[bn128_]wtns_gather_dev: sMap32 = device, nRows x nCols 32-bit indices.  An index >= nW writes zero; with hostFirstBad the call
 * BLOCKS and reports the smallest flat cell index i nCols + j holding one, UINT64_MAX when clean (as land_rows); with NULL it only enqueues.
 * dstCols < nCols, nW >= 2^32, dst overlapping w or sMap: PIL2GL_EINVAL.  w and dst 8-byte (Fr: 16-byte) aligned.
 * pil2gl_[bn128_]wtns_exec: host pointers; plan, stage, compute, copy out.  The u64 tables as the files hold them: Goldilocks hostAddIdx
 * = the records (a, b, ca, cb) and hostAddCoef = hostAddIdx + 2 (strides 4); Fr hostAddIdx = 2 nAdds indices, hostAddCoef = 2 nAdds
 * elements.  hostSMap64 = nRows x nCols u64; a value >= nW is PIL2GL_EINVAL naming the cell.  hostDst = nRows x nCols elements.
 * Every refusal comes before the first device call; without a device the compute calls return PIL2GL_ENODEV.  nAdds = 0 and an empty
 * trace are PIL2GL_OK. */
int pil2gl_wtns_adds_plan(const uint64_t *hostAddIdx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, const uint64_t *hostCoef,
                          uint64_t coefStride, uint32_t coefWords, uint32_t *outAdds, uint64_t *outCoef, uint32_t *outLevelStart,
                          uint32_t levelCap, uint32_t *nLevels);
int pil2gl_wtns_adds_dev(uint64_t *w, uint64_t nWitness, const uint32_t *adds, const uint64_t *coefs, uint64_t nAdds,
                         const uint32_t *hostLevelStart, uint32_t nLevels, void *stream);
int pil2gl_bn128_wtns_adds_dev(uint64_t *w, uint64_t nWitness, const uint32_t *adds, const uint64_t *coefs, uint64_t nAdds,
                               const uint32_t *hostLevelStart, uint32_t nLevels, void *stream);
int pil2gl_wtns_gather_dev(const uint64_t *w, uint64_t nW, const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t *dst,
                           uint64_t dstCols, uint64_t *hostFirstBad, void *stream);
int pil2gl_bn128_wtns_gather_dev(const uint64_t *w, uint64_t nW, const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t *dst,
                                 uint64_t dstCols, int toMontgomery, uint64_t *hostFirstBad, void *stream);
int pil2gl_wtns_exec(const uint64_t *hostW, uint64_t nWitness, const uint64_t *hostAddIdx, const uint64_t *hostAddCoef, uint64_t nAdds,
                     const uint64_t *hostSMap64, uint64_t nRows, uint64_t nCols, uint64_t *hostDst);
int pil2gl_bn128_wtns_exec(const uint64_t *hostW, uint64_t nWitness, const uint64_t *hostAddIdx, const uint64_t *hostAddCoef, uint64_t nAdds,
                           const uint64_t *hostSMap64, uint64_t nRows, uint64_t nCols, uint64_t *hostDst, int toMontgomery);
/* host-only, no device: how the additions run.  outInfo[0] = levels, [1] = kernel launches of the additions (one per level), [2] = the
 * widest level, [3] = threads per workgroup, [4] = workgroups of the widest level's launch; outWidths[l] = additions of level l for
 * l < widthCap (may be NULL).  Refuses what pil2gl_wtns_adds_plan refuses. */
int pil2gl_debug_wtns_plan(const uint64_t *hostAddIdx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, uint32_t *outInfo /* [5] */,
                           uint32_t *outWidths, uint32_t widthCap);

/* ---- connection polynomials: the constant columns S of a recursion circuit from its sMap (csrc/conn_pols.hip, csrc/conn_plan.h) ----
 * The compressor and final setups build the copy-constraint permutation with two host loops (src/compressor/compressor12_setup.js:470-500,
 * compressor18_setup.js:534-560, src/final/final6_setup.js:243-270, final9_setup.js:264-290, finalfflonk_setup.js:136-163 over curve.Fr,
 * test/plonk2pil/plonksetup.js:79-105):
 *   S[j][i] = id(i, j) = w^i ks1[j] for i < N, j < nCols, with ks1[0] = 1 and ks1[j] = ks[j - 1] (w = F.w[nBits], ks = getKs(F, nCols - 1));
 *   for i < nRows, for j < nCols, s = sMap[j][i], s != 0: the first time s is seen its cell is remembered, every later time
 *   connect(S[first.col], first.row, S[j], i) swaps the two values (polutils.js:166).
 * The result has a closed form: with c_0 < c_1 < ... < c_k the cells of one signal in flat order i nCols + j, S[c_m] = id(c_{m-1}) for
 * m >= 1 and S[c_0] = id(c_k).  A zero cell, a signal seen once and every row at or past nRows keep id of themselves.  The library sorts
 * the cells by signal (stable, 8 bits a pass) and fills S from each cell's predecessor; the values equal the reference's, cell for cell.
 * An element is one u64 (Goldilocks: w and ks1 words in [p, 2^64) count as their value mod p, outputs canonical) or four u64 (Fr: w, ks1
 * and the output are MONTGOMERY words, what finalfflonk_setup.js leaves in constPols.Final.S through writeToBigBufferFr; any 256-bit pattern
 * counts as its value mod r, outputs canonical).  w (1 element) and ks1 (nCols elements, ks1[0] included) are HOST pointers in every form
 * and are read before the call returns; the library multiplies what it is given (getKs is pilcom's).
 *
 * pil2gl_conn_plan: host-only, no device.  outInfo[0] = digit passes of the sort, ceil(bits(nW - 1) / 8) (0 when no cell can name a signal);
 * [1] = threads per workgroup; [2] = cells per workgroup of a pass; [3] = workgroups of a pass's histogram and scatter; [4] = workgroups
 * of the histogram's scan; [5], [6] = bits of the low and high power tables (2^[5] entries a column, 2^[6] entries); [7] = kernel launches
 * of a call, 4 + 5 passes (2 without cells).  *scratchBytes = the working buffer, a multiple of 16: with cells = nRows nCols and
 * T = nCols 2^[5] + 2^[6], 16 + 8 elemWords T + 4 r16(4 cells) + 1024 [3] + r16(4 [4]) where r16 rounds up to 16 -- below
 * 16 cells + cells / 4 + cells / 16384 + 8 elemWords T + 2048 bytes; 0 for nCols = 0.  PIL2GL_EINVAL: nRows nCols >= 2^32, nW >= 2^32,
 * nRows > N, N no power of two or above 2^32, nCols > 64, elemWords not 1 or 4.
 * pil2gl_[bn128_]conn_pols_dev: sMap32 = device, nRows x nCols 32-bit indices, row-major (what pil2gl_wtns_gather_dev reads); scratch =
 * device, 16-byte aligned, scratchBytes >= the plan's; dst = device, element (i, j) at dst[(i dstStride + dstOffset + j) elemWords], the
 * column contract of csrc/bn_column.h applied to nCols adjacent columns of a row-major matrix dstStride elements wide, of which only those
 * nCols are written, N rows of them.  An index >= nW counts as zero (the cell keeps its identity); with hostFirstBad the call BLOCKS and
 * reports the smallest flat cell i nCols + j holding one, UINT64_MAX when clean; with NULL it only enqueues.  PIL2GL_EINVAL: what the plan
 * refuses, dstStride < dstOffset + nCols, dstStride >= 2^32, a scratch that is too small, dst overlapping sMap32 or the scratch, the
 * scratch overlapping sMap32, a null or misaligned buffer (dst 8-byte, Fr 16-byte).  nCols = 0 is PIL2GL_OK and needs no device.
 * pil2gl_[bn128_]conn_pols: host pointers; stage, compute, copy out N x nCols elements, row-major (hostDst[(i nCols + j) elemWords]).
 * sMapLayout PIL2GL_CONN_SMAP_ROWS_U64: hostSMap = nRows x nCols u64, row-major (an exec file's table); PIL2GL_CONN_SMAP_COLS_U32: nCols
 * arrays of N u32 one after the other (the setups' sMap[j][i] at hostSMap[j N + i]), of which rows below nRows are read.  A value >= nW is
 * PIL2GL_EINVAL naming the cell.  Every refusal comes before the first device call; without a device the compute calls return
 * PIL2GL_ENODEV. */
#define PIL2GL_CONN_SMAP_ROWS_U64 0
#define PIL2GL_CONN_SMAP_COLS_U32 1
int pil2gl_conn_plan(uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, uint32_t elemWords, uint32_t *outInfo /* [8] */, uint64_t *scratchBytes);
int pil2gl_conn_pols_dev(const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW, const uint64_t *hostKs1,
                         uint64_t *dst, uint64_t dstStride, uint64_t dstOffset, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostFirstBad,
                         void *stream);
int pil2gl_bn128_conn_pols_dev(const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                               const uint64_t *hostKs1, uint64_t *dst, uint64_t dstStride, uint64_t dstOffset, uint64_t *scratch, uint64_t scratchBytes,
                               uint64_t *hostFirstBad, void *stream);
int pil2gl_conn_pols(const void *hostSMap, int sMapLayout, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                     const uint64_t *hostKs1, uint64_t *hostDst);
int pil2gl_bn128_conn_pols(const void *hostSMap, int sMapLayout, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                           const uint64_t *hostKs1, uint64_t *hostDst);

/* ---- connection check: does a trace meet `{a[0 .. nCols)} connect {S[0 .. nCols)}` (csrc/conn_check.hip, csrc/conn_check_plan.h) ----
 * The reference checks a recursion circuit's witness with pilcom's verifyPil (src/compressor/main_compressor_pil_verify.js:36, which loads
 * the .const and .commit files); beyond polynomial identities the compressor and final PILs state one identity,
 * `{a[0], ..., a[n-1]} connect {S[0], ..., S[n-1]}` (src/compressor/compressor12.pil.ejs:352, compressor18.pil.ejs:374,
 * src/final/final6.pil.ejs:151, final9.pil.ejs:156, finalfflonk.pil.ejs:54).  pilcom is not part of the reference checkout; the statement checked here is this header's own:
 *   id(i, j) = w^i ks1[j] for i < N, j < nCols, ks1[0] = 1; cells in flat order c = i nCols + j; for every cell c, S[c] must equal id(c')
 *   of exactly one cell c' and a[c] must equal a[c'], both compared as field values.
 * hostReport[0] = the smallest failing flat cell, UINT64_MAX when the trace is clean; [1] = the cell its S names, UINT64_MAX when it names
 * none; [2] = the kind: 0 clean, 1 S names no cell, 2 the values differ, 3 the identities are not distinct (two cells share one id: a bad
 * ks1 or w) -- then [0] is the first cell, in flat order, whose id an earlier cell has, [1] the first cell with that id, and a and S are
 * not judged.  An element is one u64 (Goldilocks: words in [p, 2^64) count as their value mod p) or four u64 (Fr: MONTGOMERY words, any
 * 256-bit pattern counting as its value mod r), as pil2gl_[bn128_]conn_pols writes S and pil2gl_[bn128_]wtns_gather_dev the trace.
 * w (1 element) and ks1 (nCols elements, ks1[0] included) are HOST pointers in every form.
 *
 * pil2gl_conn_check_plan: host-only, no device.  outInfo[0] = log2 of the hash table's capacity, the smallest power of two >= 2 N nCols
 * and >= 16 (one 32-bit cell index a slot; the load factor never exceeds 1 / 2); [1] = threads per workgroup; [2], [3] = bits of the low
 * and high power tables (as pil2gl_conn_plan's [5], [6]); [4], [5] = workgroups of the build and of the check; [6] = lanes a cell of the
 * check (1, Fr 2); [7] = kernel launches of a call, 4.  *scratchBytes = the working buffer, a multiple of 16:
 * 64 + 4 2^[0] + r16(8 elemWords 2^[3]) + r16(8 elemWords nCols 2^[2]) where r16 rounds up to 16; 0 for nCols = 0.  PIL2GL_EINVAL:
 * N nCols >= 2^32, N no power of two or above 2^32, nCols > 64, elemWords not 1 or 4.
 * pil2gl_[bn128_]conn_check_dev: a, S = device; element (i, j) of either at ptr[(i stride + offset + j) elemWords], the column contract
 * of csrc/bn_column.h applied to nCols adjacent columns of a row-major matrix `stride` elements wide (where conn_pols_dev wrote S and
 * wtns_gather_dev the trace); a and S may be one matrix at different offsets, they are only read.  scratch = device, 16-byte aligned,
 * scratchBytes >= the plan's.  The call BLOCKS until the three words of hostReport are on the host (as pil2gl_bn128_h1h2_dev blocks for
 * its missing row).  PIL2GL_EINVAL: what the plan refuses, stride < offset + nCols or stride >= 2^32 for a or S, a scratch that is too
 * small or overlaps a or S, a null or misaligned buffer (a, S 8-byte, Fr 16-byte), a null hostReport.  nCols = 0 is PIL2GL_OK, clean,
 * and needs no device.
 * pil2gl_[bn128_]conn_check: host pointers, hostA and hostS N x nCols elements each, row-major; stage (every part on 16 bytes), compute.
 * Every refusal comes before the first device call; without a device the compute calls return PIL2GL_ENODEV. */
int pil2gl_conn_check_plan(uint64_t N, uint64_t nCols, uint32_t elemWords, uint32_t *outInfo /* [8] */, uint64_t *scratchBytes);
int pil2gl_conn_check_dev(const uint64_t *a, uint64_t aStride, uint64_t aOffset, const uint64_t *S, uint64_t sStride, uint64_t sOffset, uint64_t N,
                          uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1, uint64_t *scratch, uint64_t scratchBytes,
                          uint64_t *hostReport /* [3] */, void *stream);
int pil2gl_bn128_conn_check_dev(const uint64_t *a, uint64_t aStride, uint64_t aOffset, const uint64_t *S, uint64_t sStride, uint64_t sOffset, uint64_t N,
                                uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1, uint64_t *scratch, uint64_t scratchBytes,
                                uint64_t *hostReport /* [3] */, void *stream);
int pil2gl_conn_check(const uint64_t *hostA, const uint64_t *hostS, uint64_t N, uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1,
                      uint64_t *hostReport /* [3] */);
int pil2gl_bn128_conn_check(const uint64_t *hostA, const uint64_t *hostS, uint64_t N, uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1,
                            uint64_t *hostReport /* [3] */);
/* host-only, no device: the longest distance, in slots, between a key of the last call's hash table and its home slot (0: every key at
 * home, or no call yet) -- what shows that a test reached the probing past the home slot */
uint64_t pil2gl_debug_conn_check_probe(void);

/* ---- lookup and permutation checks: does a trace meet `selF {f0..fk-1} in selT {t0..tk-1}` (plookup) or `selF {f0..fk-1} is selT {t0..tk-1}`
 * (permutation) (csrc/tuple_check.hip, csrc/tuple_check_plan.h) ----
 * The two non-polynomial identity kinds of PIL beside `connect`.  Without this block a witness that breaks one is found in stage 2 only:
 * a permutation as the boundary constraint of Z at row N - 1, which names no row of f or t; a lookup as h1h2's missing row of the
 * challenge-compressed value, columns and selectors already folded into one element.  pilcom is not part of the reference checkout; the
 * statement checked here is this header's own (tests/tuple_check_ref.py restates it as one dictionary):
 *   n rows, k columns, 1 <= k <= 16.  f = k columns of a row-major matrix: element j of row i at f[(i fStride + hostFCols[j]) elemWords];
 *   the cols are element offsets within a row, need not be adjacent or increasing, and their order is the tuple's order.  t alike, with
 *   its own base, stride and cols.  selF, selT: one column (base, stride, col) of a matrix of its own each, or NULL.
 *   An element counts as its field value: one u64 (Goldilocks: words in [p, 2^64) count mod p) or four u64 (Fr: MONTGOMERY words, any
 *   256-bit pattern counting mod r), pil2gl_[bn128_]conn_pols' rule.  Two tuples are equal when all k values are equal, in order.  A row
 *   is SELECTED when its selector is NULL or its selector's value is non-zero; a selector value other than 0 or 1 is a polynomial
 *   identity's business and is not judged here.  A cubic-extension column is three columns to this block.
 *   cntF(v) = the selected rows of f with tuple v, cntT(v) = the selected rows of t with tuple v.
 *   mode 0, lookup (`in`): the trace fails when a selected row of f has cntT = 0; the row reported is the smallest such, the kind 1.
 *   mode 1, permutation (`is`): the trace fails when cntF(v) != cntT(v) for some v.  If any selected row of f has cntF > cntT the report
 *   is the smallest such row, kind 1 when cntT = 0 and 2 otherwise; if none has, it is the smallest selected row of t with cntT > cntF,
 *   kind 3.  A serial checker that walks f and decrements the counts of t would name the (cntT + 1)-th occurrence of an over-subscribed
 *   tuple; this block names the tuple's FIRST occurrence in f and gives both counts.  Both name the same tuple; the first occurrence
 *   needs no order of traversal to be defined, and cntF - cntT says how many occurrences are in excess, which the serial walk does not.
 * hostReport[0] = kind (0 clean); [1] = row; [2] = partner, the smallest selected row on the OTHER side (t for kinds 1 and 2, f for kind 3)
 * that holds the same tuple, UINT64_MAX when there is none; [3] = cntF and [4] = cntT of the reported row's tuple.  All five words
 * describe one tuple.  A clean trace gives (0, UINT64_MAX, UINT64_MAX, 0, 0).  The report does not depend on the order in which the
 * device's atomics land.
 *
 * pil2gl_tuple_check_plan: host-only, no device.  outInfo[0] = log2 of the hash table's capacity, the smallest power of two >= 4 n and
 * >= 16 (both sides' rows share one table: at most 2 n rows are inserted, so the load factor never exceeds 1 / 2 whatever the data);
 * [1] = threads per workgroup; [2] = workgroups of the build and of the judge; [3] = kernel launches of a call, 3; [4] = bytes of the
 * header, 64; [5] = bytes a slot, 16 (a 32-bit row index, the tuple's smallest f row, a 64-bit counter).  *scratchBytes = the working
 * buffer, 64 + 16 2^[0], every part on 16 bytes; 0 for n = 0.  PIL2GL_EINVAL: n > 2^28, k outside 1 .. 16, elemWords not 1 or 4, a mode
 * other than 0 or 1.
 * pil2gl_[bn128_]tuple_check_dev: f, t, selF, selT = device, 16-byte aligned, only read: they may overlap each other freely and one
 * matrix may serve both sides.  hostFCols, hostTCols = HOST pointers, k entries each.  scratch = device, 16-byte aligned,
 * scratchBytes >= the plan's.  The call BLOCKS until the five words of hostReport are on the host.  PIL2GL_EINVAL, before any device
 * call: what the plan refuses, a column >= its stride (f, t or a selector; a stride >= 2^32), a null f, t, cols, scratch or hostReport, a
 * misaligned device pointer, a scratch that is too small or overlaps f, t or a selector.  n = 0 is PIL2GL_OK, clean, and needs no device.
 * pil2gl_[bn128_]tuple_check: host pointers; each matrix is staged up to the last element touched ((n - 1) stride + the highest column + 1
 * elements, every part on 16 bytes) and the working buffer is taken inside.
 * Without a device the compute calls return PIL2GL_ENODEV. */
int pil2gl_tuple_check_plan(uint64_t n, uint64_t k, uint32_t elemWords, uint32_t mode, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_tuple_check_dev(const uint64_t *f, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *t, uint64_t tStride,
                           const uint64_t *hostTCols, const uint64_t *selF, uint64_t selFStride, uint64_t selFCol, const uint64_t *selT,
                           uint64_t selTStride, uint64_t selTCol, uint64_t n, uint64_t k, uint32_t mode, uint64_t *scratch,
                           uint64_t scratchBytes, uint64_t *hostReport /* [5] */, void *stream);
int pil2gl_bn128_tuple_check_dev(const uint64_t *f, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *t, uint64_t tStride,
                                 const uint64_t *hostTCols, const uint64_t *selF, uint64_t selFStride, uint64_t selFCol, const uint64_t *selT,
                                 uint64_t selTStride, uint64_t selTCol, uint64_t n, uint64_t k, uint32_t mode, uint64_t *scratch,
                                 uint64_t scratchBytes, uint64_t *hostReport /* [5] */, void *stream);
int pil2gl_tuple_check(const uint64_t *hostF, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *hostT, uint64_t tStride,
                       const uint64_t *hostTCols, const uint64_t *hostSelF, uint64_t selFStride, uint64_t selFCol, const uint64_t *hostSelT,
                       uint64_t selTStride, uint64_t selTCol, uint64_t n, uint64_t k, uint32_t mode, uint64_t *hostReport /* [5] */);
int pil2gl_bn128_tuple_check(const uint64_t *hostF, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *hostT, uint64_t tStride,
                             const uint64_t *hostTCols, const uint64_t *hostSelF, uint64_t selFStride, uint64_t selFCol,
                             const uint64_t *hostSelT, uint64_t selTStride, uint64_t selTCol, uint64_t n, uint64_t k, uint32_t mode,
                             uint64_t *hostReport /* [5] */);
/* host-only, no device: the home slot of a tuple in a table of `capacity` slots (a power of two), from the one hash function host and
 * device share: words = k elemWords CANONICAL 64-bit words (Goldilocks values below p; Fr Montgomery words below r), column after
 * column.  UINT64_MAX for k outside 1 .. 16, elemWords not 1 or 4, a capacity that is no power of two, null words. */
uint64_t pil2gl_debug_tuple_home(const uint64_t *words, uint64_t k, uint32_t elemWords, uint64_t capacity);
/* host-only, no device: the longest distance, in slots, between a tuple of the last call's hash table and its home slot (0: every tuple
 * at home, or no call yet) -- what shows that a test reached the probing past the home slot */
uint64_t pil2gl_debug_tuple_check_probe(void);

/* ---- lookup multiplicities: the logUp column m of `selF_s {f_s} in selT {t}`, s < nF (csrc/lookup_mult.hip, csrc/lookup_mult_plan.h) ----
 * pil2 states a lookup as a grand sum, sum selF / (f + gamma) - sum m / (t + gamma) = 0; m is a stage-1 witness column: m[j] = how often
 * the tuple of row j of t is looked up.  The block above says whether a lookup holds; this one produces the column that proves it, without
 * f and t leaving the device.  The statement is this header's own (tests/lookup_mult_ref.py restates it as one dictionary):
 *   n rows every side, n <= 2^28; k columns a tuple, 1 <= k <= 16; 1 <= nF <= 8 sides of f, so nF n <= 2^31 and a count fits 32 bits.
 *   One side is a pil2gl_tuple_side: k columns `hostCols` (element offsets within a row, in the tuple's order, a HOST pointer) of the
 *   row-major matrix (base, stride), and an optional selector column (sel, selStride, selCol) of a matrix of its own (sel NULL: none).
 *   Elements, equality of tuples and SELECTED rows are the block above's: an element counts as its field value (Goldilocks words in
 *   [p, 2^64) mod p, any 256-bit Fr Montgomery pattern mod r); a row is selected when its selector is NULL or non-zero.
 *   t is one side; f_0 .. f_{nF-1} are nF sides, each with its own matrix, columns and selector.
 *   cnt(v) = the sum over s of the selected rows of f_s with tuple v.
 *   m = column mCol of a matrix (m, mStride) of elemWords-word elements, written for EVERY row j < n:  m[j] = cnt(tuple of t[j]) when j is
 *   selected in t and is the smallest selected row of t with that tuple; m[j] = 0 otherwise.  The value is a canonical field element: one
 *   u64 below p, or the Montgomery form of the count, below r.
 * hostReport[0] = kind: 0 clean; 1 = some selected row of some f_s holds a tuple that no selected row of t holds.  [1] = side, [2] = row:
 * for kind 1 the lexicographically smallest failing (side, row); both UINT64_MAX when clean.  [3] = matched, the selected rows of all f
 * sides whose tuple t holds.  The sum of m over all rows is `matched`, always; on kind 1 m is still written in full and counts the rows
 * that matched.  Neither m nor the report depends on the order in which the device's atomics land.
 *
 * pil2gl_lookup_mult_plan: host-only, no device.  outInfo[0] = log2 of the hash table's capacity, the smallest power of two >= 2 n and
 * >= 16 (only t's selected rows are inserted: the load factor never exceeds 1 / 2); [1] = threads per workgroup; [2] = workgroups of the
 * build, of each count and of the write; [3] = kernel launches of a call, 3 + nF (init, build, one count a side of f, write); [4] = bytes
 * of the header, 64; [5] = bytes a slot, 8 (the tuple's smallest selected row of t, a 32-bit counter).  *scratchBytes = the working
 * buffer, 64 + 8 2^[0]; 0 for n = 0.  PIL2GL_EINVAL: n > 2^28, k outside 1 .. 16, nF outside 1 .. 8, elemWords not 1 or 4.
 * pil2gl_[bn128_]lookup_mult_dev: hostF (nF entries) and hostT are HOST pointers to sides whose base and sel are device pointers, 16-byte
 * aligned, only read; the read matrices may overlap each other freely and one matrix may serve several sides.  m = device, 16-byte
 * aligned.  Aliasing rule of m: m's span (from m to the end of row n - 1's element of column mCol) may meet the span of a matrix that is
 * read (t, an f, a selector's) only when it has that matrix's base and stride and mCol is none of the columns read of it -- m as one more
 * column of t's or of an f's matrix is the normal case.  scratch = device, 16-byte aligned, scratchBytes >= the plan's, meeting no
 * matrix, m's included.  The call BLOCKS until the four words of hostReport are on the host.  PIL2GL_EINVAL, before any device call: what
 * the plan refuses, a column >= its stride (t, an f, a selector or m), a stride >= 2^32 or n stride > 2^58 elements, a null side list,
 * cols, base, m, scratch or hostReport, a misaligned device pointer, a scratch that is too small or overlaps a matrix, an m that breaks
 * the aliasing rule.  A refused call leaves a clean report.  n = 0 is PIL2GL_OK, clean, writes nothing and needs no device.
 * pil2gl_[bn128_]lookup_mult: host pointers throughout; each matrix is staged up to the last element touched, every part on 16 bytes,
 * m's matrix (up to column mCol of row n - 1) goes up as it is and is downloaded again with the column written; the working buffer is
 * taken inside.  The aliasing rule holds for the host pointers alike.  Without a device the compute calls return PIL2GL_ENODEV. */
typedef struct pil2gl_tuple_side {
    const uint64_t *base;                /* the matrix: element j of row i at base[(i stride + hostCols[j]) elemWords] */
    uint64_t stride;
    const uint64_t *hostCols;            /* k element offsets, a HOST pointer in every form */
    const uint64_t *sel;                 /* the selector's matrix, or NULL */
    uint64_t selStride, selCol;
} pil2gl_tuple_side;
int pil2gl_lookup_mult_plan(uint64_t n, uint64_t k, uint64_t nF, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_lookup_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *m, uint64_t mStride,
                           uint64_t mCol, uint64_t n, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport /* [4] */,
                           void *stream);
int pil2gl_bn128_lookup_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *m, uint64_t mStride,
                                 uint64_t mCol, uint64_t n, uint64_t k, uint64_t *scratch, uint64_t scratchBytes,
                                 uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_lookup_mult(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *hostM, uint64_t mStride,
                       uint64_t mCol, uint64_t n, uint64_t k, uint64_t *hostReport /* [4] */);
int pil2gl_bn128_lookup_mult(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *hostM, uint64_t mStride,
                             uint64_t mCol, uint64_t n, uint64_t k, uint64_t *hostReport /* [4] */);
/* host-only, no device: the longest distance, in slots, between a tuple of the last call's hash table and its home slot */
uint64_t pil2gl_debug_lookup_mult_probe(void);

/* ---- range-check multiplicities: the logUp column m of `selF_s f_s in [lo, lo + size)`, s < nF (csrc/range_mult.hip, csrc/range_mult_plan.h) ----
 * The commonest lookup of a pil2 witness is a range check.  Its table is an arithmetic progression: the counter of a value v is v - lo, and
 * the block above would hash, probe and build for nothing -- and need the range materialised as a column t.  This block counts by direct
 * addressing and takes no t.  The statement is this header's own (tests/range_mult_ref.py restates it over Python integers):
 *   n rows, n <= 2^28; 1 <= nF <= 8 sides of f, each a pil2gl_tuple_side of which only hostCols[0] is read (k = 1); the optional selector,
 *   elements and SELECTED rows are the block above's (Goldilocks words in [p, 2^64) mod p, any 256-bit Fr Montgomery pattern mod r).
 *   The range is lo, a SIGNED 64-bit integer (negative allowed), and size, 1 <= size <= 2^28; its field elements are lo + j mod p|r, j < size.
 *   A value v is IN RANGE when (v - lo) mod p|r < size, the difference taken as a full field element (over Fr of the normal form, not of the
 *   Montgomery pattern).  cnt(j) = the selected rows, over all sides, whose value is lo + j.
 *   m = column mCol of a matrix (m, mStride) of elemWords-word elements, written for EVERY row i < n: cnt(i - row0) for
 *   row0 <= i < row0 + size, 0 elsewhere; row0 + size <= n.  The value is a canonical element as the block above writes it: one u64, or the
 *   Montgomery form of the count.
 * hostReport is the block above's four words: [0] = kind, 0 clean, 1 = some selected row is out of range; [1] = side, [2] = row: the
 * lexicographically smallest failing (side, row), both UINT64_MAX when clean; [3] = matched.  The sum of m is `matched`, always; on kind 1 m is
 * still written in full.  Neither m nor the report depends on the order in which the device's atomics land.
 * Equivalence: with row0 = 0 the result, m and report, is word for word what pil2gl_[bn128_]lookup_mult gives with k = 1 on the materialised
 * column t[i] = field(lo + min(i, size - 1)) -- the padding a fixed range column holds; the first-occurrence rule puts its count at row size - 1.
 * ONE range a call: several ranges stacked in one m column are out of scope; make one call per range, into separate columns.
 *
 * pil2gl_range_mult_plan: host-only, no device.  outInfo[0] = path: 0 = a workgroup counts in LDS counters of its own and flushes them once
 * (size <= the threshold, csrc/range_mult_plan.h), 1 = merged atomics on the global counters; [1] = threads a workgroup of a count launch;
 * [2] = workgroups of a count launch; [3] = kernel launches of a call, 2 + nF (init, one count a side, write); [4] = bytes of the header, 64;
 * [5] = counters a workgroup holds in LDS, 0 on path 1.  *scratchBytes = the working buffer, 64 + 4 size rounded up to 16; 0 for n = 0.
 * PIL2GL_EINVAL: n > 2^28, size outside 1 .. 2^28 or (n > 0) above n, nF outside 1 .. 8, elemWords not 1 or 4.
 * pil2gl_[bn128_]range_mult_dev: hostF (nF entries) is a HOST pointer to sides whose base and sel are device pointers, 16-byte aligned, only
 * read.  m = device, 16-byte aligned; its aliasing rule is the block above's: m may meet a matrix that is read only as that matrix (its base,
 * its stride) with a column that is not read.  scratch = device, 16-byte aligned, scratchBytes >= the plan's, meeting no matrix, m's
 * included.  The call BLOCKS until the four words of hostReport are on the host.  PIL2GL_EINVAL, before any device call: what the plan
 * refuses, row0 + size > n, a column >= its stride (an f, a selector or m), a stride >= 2^32 or n stride > 2^58 elements, a null side list,
 * cols, base, m, scratch or hostReport, a misaligned device pointer, a scratch that is too small or overlaps a matrix, an m that breaks the
 * aliasing rule.  A refused call leaves a clean report.  n = 0 is PIL2GL_OK, clean, writes nothing and needs no device.
 * pil2gl_[bn128_]range_mult: host pointers throughout; each matrix is staged up to the last element touched, every part on 16 bytes, m's
 * matrix goes up as it is and is downloaded again with the column written; the working buffer is taken inside.  Without a device the
 * compute calls return PIL2GL_ENODEV.
 * The two debug_ entries are the plan and the resident form with the count path given (0, 1, or 2 = the planner's choice; path 0 takes
 * size <= 8192), for the tests and tools/bench_range_mult.py; elemWords selects the field. */
int pil2gl_range_mult_plan(uint64_t n, uint64_t size, uint64_t nF, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride,
                          uint64_t mCol, uint64_t n, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_bn128_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m,
                                uint64_t mStride, uint64_t mCol, uint64_t n, uint64_t *scratch, uint64_t scratchBytes,
                                uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_range_mult(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *hostM, uint64_t mStride,
                      uint64_t mCol, uint64_t n, uint64_t *hostReport /* [4] */);
int pil2gl_bn128_range_mult(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *hostM,
                            uint64_t mStride, uint64_t mCol, uint64_t n, uint64_t *hostReport /* [4] */);
int pil2gl_debug_range_mult_plan(uint64_t n, uint64_t size, uint64_t nF, uint32_t elemWords, uint32_t path, uint32_t *outInfo /* [6] */,
                                 uint64_t *scratchBytes);
int pil2gl_debug_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m,
                                uint64_t mStride, uint64_t mCol, uint64_t n, uint64_t *scratch, uint64_t scratchBytes,
                                uint64_t *hostReport /* [4] */, void *stream, uint32_t elemWords, uint32_t path);

/* ---- multiplicity sessions: m of a table in an AIR of its own, counted over f sides of their own lengths (csrc/mult_session.hip, csrc/mult_session_plan.h) ----
 * The two blocks above state "n rows every side" and are one shot.  In a pil2 proof a table -- a U16 range, a fixed lookup table -- lives in
 * an AIR of its own and the rows that look values up lie in other AIRs, with other row counts, in many instances that arrive one at a time.
 * A session cuts the one call into three: OPEN makes the table, ADD counts f sides of any length, once per arriving instance, WRITE writes
 * m.  Between the calls the counters live in the caller's scratch.  The statement is this header's own (tests/mult_session_ref.py restates
 * it over Python integers and one dictionary):
 *   LOOKUP session: t is one pil2gl_tuple_side of nT <= 2^28 rows, k columns, 1 <= k <= 16.  open does what lookup_mult's init and build do,
 *   over t's selected rows.  t's matrix and selector must stay UNCHANGED AND RESIDENT until the session's last call: the table keeps row
 *   numbers and re-reads the keys.  hostT, nT and k are arguments of every call of the session.
 *   RANGE session: the range is (lo, size) with range_mult's meaning -- lo SIGNED, 1 <= size <= 2^28, the difference v - lo compared with
 *   size as a full field element.  open zeroes `size` counters.  lo and size are arguments of every later call; passing other values than at
 *   open is the caller's error and is not detected (a larger size reads past the counters: the scratch is checked against the size GIVEN).
 *   ADD: 1 <= nF <= 8 sides of f; side s has its OWN row count hostRows[s] <= 2^28, independent of nT and of size.  A side of 0 rows launches
 *   nothing and its pointers are not looked at.  Selected rows, element values (Goldilocks words in [p, 2^64), any Fr pattern), equality of
 *   tuples and IN RANGE are exactly the one-shot blocks'.  Every selected row whose tuple or value the table holds adds 1 to that counter.
 *   hostReport[4] describes THIS ADD ONLY: [0] = kind, 0 clean or 1; [1], [2] = the lexicographically smallest failing (side, row) of this
 *   add, both UINT64_MAX when clean; [3] = the matched rows of this add.  On kind 1 the rows that matched are still counted.  The call
 *   BLOCKS for the report.  Adds to one session must be stream-ordered; two adds in flight on one session are outside the statement.
 *   WRITE, lookup: m = column mCol of (m, mStride), written for every row j < nT: the count of t[j]'s tuple when j is selected in t and is
 *   the smallest selected row of t with that tuple, 0 otherwise.  WRITE, range: m is written for every row i < nM: cnt(i - row0) inside
 *   row0 .. row0 + size - 1, 0 outside; row0 + size <= nM <= 2^28.  The value is the canonical element of the accumulated count: one u64, or
 *   the Montgomery form over Fr.  hostTotal (one u64, may be NULL) receives the matched rows of the whole session, the integer sum of m;
 *   with NULL the call only enqueues, otherwise it BLOCKS.  write does not end the session: it may be called again after further adds and
 *   then shows the later state.  Nothing ends a session but the caller reusing the scratch.
 *   Counters are 64 bits wide.  Counts of 2^64 and above, or of p and above over Goldilocks, are outside the statement (2^33 full adds) and
 *   are not checked for.
 * Aliasing: m keeps lookup_mult's rule against t (it may be a spare column of t's matrix).  The scratch meets no matrix of any call.  The
 * matrices of f may overlap each other freely and one matrix may serve several sides; a side may start at a later row of a matrix, by a
 * base advanced by whole rows (still 16-byte aligned).
 * Equivalences: (1) one add whose sides all have hostRows[s] = nT (range: = nM, row0 as given), then write, gives m and the report word for
 * word as pil2gl_[bn128_]lookup_mult_dev / range_mult_dev give on the same input.  (2) m after a session depends only on the multiset of
 * selected rows offered, not on how they were cut into adds, sides and row ranges.
 *
 * pil2gl_lookup_session_plan / pil2gl_range_session_plan: host-only, no device.  outInfo[0] = log2 of the hash table's capacity (the smallest
 * power of two >= 2 nT and >= 16), or the range's count path (0 = LDS counters a workgroup, size <= the threshold of csrc/range_mult_plan.h;
 * 1 = merged atomics on the global counters); [1] = threads a workgroup of a count launch; [2] = workgroups of a count launch over a side of
 * 2^28 rows -- a launch takes its grid from ITS side's rows, never from the table; [3] = kernel launches of open, of an add with one side
 * (each further side with rows is one more) and of write, as open | add << 8 | write << 16: 2, 2, 1 for a lookup session (init, build; the
 * lane that closes the last add's report, count; write) and 1, 2, 1 for a range session; [4] = bytes of the header, 64; [5] = bytes a slot,
 * 16 (the tuple's smallest selected row of t, a 64-bit counter), or a counter, 8.  *scratchBytes = 64 + 16 2^[0] (0 for nT = 0), or
 * 64 + 8 size rounded up to 16.  PIL2GL_EINVAL: nT > 2^28, k outside 1 .. 16, size outside 1 .. 2^28, elemWords not 1 or 4.
 * The compute entries: hostT, hostF (nF entries) and hostRows (nF entries) are HOST pointers; base, sel, m and scratch are device pointers,
 * 16-byte aligned.  open only ENQUEUES.  PIL2GL_EINVAL, before any device call: what the plans refuse, nF outside 1 .. 8, a hostRows[s]
 * above 2^28, a column >= its stride, a stride >= 2^32 or rows stride > 2^58 elements -- each side checked against ITS OWN row count, t
 * against nT, m against nT or nM --, row0 + size > nM, a null hostT, hostF, hostRows, cols, base (of a side with rows), m, scratch or
 * hostReport, a misaligned device pointer, a scratch that is too small or overlaps a matrix of this call, an m that breaks the aliasing
 * rule.  A refused add leaves a clean report.  nT = 0 is PIL2GL_OK in all three lookup entries and does nothing.  Without a device the
 * compute entries return PIL2GL_ENODEV.  There are no host-pointer forms: a session's state is the device's.
 * The debug_ entries are for the tests and tools/bench_mult_session.py: the open forms with a seed, the u64 every counter starts from
 * (hostTotal of a later write is then NOT the sum of m: it counts matched rows only); the range plan and add with the count path given
 * (0, 1, or 2 = the planner's choice; path 0 takes size <= 8192), elemWords selecting the field; and pil2gl_debug_mult_session_grids, host-only: the
 * workgroups of the count launch of each of the 8 sides of the LAST add of this process, 0 for a side that launched nothing -- what lets a
 * test see that a launch took its grid from its side's rows. */
int pil2gl_lookup_session_plan(uint64_t nT, uint64_t k, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_range_session_plan(uint64_t size, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, void *stream);
int pil2gl_bn128_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes,
                                         void *stream);
int pil2gl_range_session_open_dev(uint64_t size, uint64_t *scratch, uint64_t scratchBytes, void *stream);
int pil2gl_lookup_session_add_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, const pil2gl_tuple_side *hostF, const uint64_t *hostRows,
                                  uint64_t nF, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_bn128_lookup_session_add_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, const pil2gl_tuple_side *hostF,
                                        const uint64_t *hostRows, uint64_t nF, uint64_t *scratch, uint64_t scratchBytes,
                                        uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF, uint64_t *scratch,
                                 uint64_t scratchBytes, uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_bn128_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF,
                                       uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport /* [4] */, void *stream);
int pil2gl_lookup_session_write_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *m, uint64_t mStride, uint64_t mCol,
                                    uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostTotal, void *stream);
int pil2gl_bn128_lookup_session_write_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *m, uint64_t mStride, uint64_t mCol,
                                          uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostTotal, void *stream);
int pil2gl_range_session_write_dev(uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride, uint64_t mCol, uint64_t nM, uint64_t *scratch,
                                   uint64_t scratchBytes, uint64_t *hostTotal, void *stream);
int pil2gl_bn128_range_session_write_dev(uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride, uint64_t mCol, uint64_t nM, uint64_t *scratch,
                                         uint64_t scratchBytes, uint64_t *hostTotal, void *stream);
int pil2gl_debug_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes,
                                         void *stream, uint32_t elemWords, uint64_t seed);
int pil2gl_debug_range_session_open_dev(uint64_t size, uint64_t *scratch, uint64_t scratchBytes, void *stream, uint64_t seed);
void pil2gl_debug_mult_session_grids(uint32_t *outGrids /* [8] */);
int pil2gl_debug_range_session_plan(uint64_t size, uint32_t elemWords, uint32_t path, uint32_t *outInfo /* [6] */, uint64_t *scratchBytes);
int pil2gl_debug_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF,
                                       uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport /* [4] */, void *stream, uint32_t elemWords,
                                       uint32_t path);

/* ---- lookup grand sum: the logUp column s of `selF_s {f_s} in selT {t}` from f, t and m (csrc/logup_sum_plan.h, hints.hip, bn_scan.hip) ----
 * The column that consumes the block above's m: the running sum of a pil2 lookup stated as  sum selF / (f + gamma) - sum m / (t + gamma),
 * in the shape pil2's std library gives a @gsum hint (a tuple Horner-compressed with std_alpha, first column highest, a bus id as the
 * last Horner term, + std_beta; the numerator a constant on the assume side and a multiplicity on the prove side), computed in one call
 * with the sides read where they lie.  The statement is this header's own (tests/logup_sum_ref.py restates it over Python integers):
 *   s[i] = s[i-1] + sum_{u < nTerms} coef_u w_u[i] / D_u[i]            s[-1] = 0,  i < n
 *   D_u[i] = ((..((v_0 alpha + v_1) alpha + v_2).. + v_{k_u-1}) alpha + busId_u) + beta
 *   n <= 2^28 rows; 1 <= nTerms <= 9 (eight f sides and t).  One term is a pil2gl_logup_term: a pil2gl_tuple_side, its k (1 .. 16, a
 *   term's own), coef and busId, HOST base-field elements: over Goldilocks word 0, canonical (else PIL2GL_EINVAL); over Fr four
 *   Montgomery words.  v_j = column hostCols[j] of the side's matrix at row i.  w_u[i] = the FIELD VALUE of the side's sel column at
 *   row i, 1 when sel is NULL: for a 0/1 selector that is the block above's "selected"; for t the sel column is m and coef is -1.
 *   Elements count as field values by the rules above (Goldilocks words in [p, 2^64) mod p, any Fr pattern mod r).
 *   alpha, beta: HOST pointers; over Goldilocks three words each, an element of the cubic extension (x^3 = x + 1, as the hints above),
 *   over Fr four Montgomery words each.
 *   out: column outCol of the matrix (out, outStride), written for every row.  Goldilocks: the matrix is rows of outStride u64 words
 *   and s[i] the three words outCol .. outCol + 2 of row i, canonical.  Fr: rows of outStride elements, s[i] one canonical Montgomery
 *   element.  Words between a strided destination's elements stay as they are.
 *   Zeros: the convention of the hints above.  A term whose D_u[i] is zero adds 0 at that row and spoils no other term or row.
 *   The hint's `result` is s[n-1]: the caller copies it, as with gsum.
 * pil2gl_logup_sum_plan: host-only, no device.  outInfo[0] = threads per workgroup of the first pass; [1] = rows a lane of it takes (8:
 * it inverts their denominators together; Fr 1); [2] = its workgroups; [3] = kernel launches of a call (Goldilocks 3: the fused first
 * pass, the block totals' scan, the fix-up; Fr 4 levels - 1: the compress, then bn128_gprod's inversion and gsum's scan); [4] =
 * Goldilocks: block totals a lane of the second pass walks, Fr: levels of pil2gl_debug_bn128_scan_plan; [5] = u64 words of an output
 * element's columns (3, or 1 element).  *workBytes = the working memory, taken from the library's own slots as gsum's is, growing with
 * neither nTerms nor k: Goldilocks 24 n + 24 ceil(n / 2048), what gsum takes; Fr the scan plan's bytes + 64 n (the product D of a row's
 * denominators and its numerator N).  PIL2GL_EINVAL: n > 2^28, nTerms outside 1 .. 9, elemWords not 1 or 4.
 * pil2gl_[bn128_]logup_sum_dev: hostTerms is a HOST pointer to terms whose side.base and side.sel are device pointers, 16-byte aligned,
 * only read; matrices may overlap each other freely and one matrix may serve several terms.  out = device, 16-byte aligned.  Aliasing
 * rule of out: lookup_mult's rule of m over each of out's word columns -- out may meet a read matrix (a term's, a numerator's) only with
 * that matrix's base and stride and with none of its read columns; s as spare columns of t's matrix is the normal case.  The call only
 * ENQUEUES on the caller's stream: the term table travels as a kernel argument, nothing is copied.  (On first use the working slots are
 * allocated, with a device synchronise when they grow; they are one per process.)  PIL2GL_EINVAL, before any device call: what the plan
 * refuses, k outside 1 .. 16, a column >= its stride (outCol + 2 over Goldilocks), a stride >= 2^32 or n stride > 2^58 elements, null
 * terms, cols, base, out, alpha or beta, a non-canonical Goldilocks coef or busId, a misaligned device pointer, an out that breaks the
 * aliasing rule.  n = 0 is PIL2GL_OK, touches nothing and needs no device.
 * pil2gl_[bn128_]logup_sum: host pointers throughout; each matrix staged up to the last element touched, every part on 16 bytes, out's
 * matrix goes up as it is and comes back with the column written.  Without a device the compute calls return PIL2GL_ENODEV. */
typedef struct pil2gl_logup_term {
    pil2gl_tuple_side side;              /* the tuple's columns; side.sel = the numerator column w, or NULL for 1 */
    uint64_t k;                          /* columns of this term's tuple, 1 .. 16 */
    uint64_t coef[4];                    /* Goldilocks: word 0, canonical.  Fr: 4 Montgomery words */
    uint64_t busId[4];
} pil2gl_logup_term;
int pil2gl_logup_sum_plan(uint64_t n, uint64_t nTerms, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *workBytes);
int pil2gl_logup_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha /* [3] */, const uint64_t *hostBeta /* [3] */,
                         uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_bn128_logup_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha /* [4] */, const uint64_t *hostBeta /* [4] */,
                               uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_logup_sum(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                     uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);
int pil2gl_bn128_logup_sum(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                           uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);

/* ---- range-check grand sum: the logUp column s of range checks from f, m and the ranges as NUMBERS (csrc/range_sum_plan.h, hints.hip, bn_scan.hip) ----
 * range_mult above takes no t; with logup_sum the argument as a whole still takes one, as the tuple column of m's term.  This block is
 * logup_sum with the table side of a range given as (lo, size, row0): no t column is made, uploaded or read.  nF = 0 is the range table's
 * own AIR in pil2's std library, whose @gsum holds only the -m_r / (t_r + gamma) terms, one per range.  The statement is this header's
 * own (tests/range_sum_ref.py restates it over Python integers):
 *   s[i] = s[i-1] + sum_{u < nF} coef_u w_u[i] / D_u[i]
 *                 + sum_{r < nR} coefR_r [row0_r <= i < row0_r + size_r] m_r[i] / E_r[i]            s[-1] = 0,  i < n
 *   D_u[i]  the block above's, of a pil2gl_logup_term: its own k in 1 .. 16, the sel column as numerator, busId, + beta
 *   E_r[i] = field(lo_r + (i - row0_r)) alpha + busId_r + beta
 *   n <= 2^28 rows; 0 <= nF <= 8, 1 <= nR <= 8, nF + nR <= 9.  One range is a pil2gl_range_term: the column mCol of the matrix (m, mStride)
 *   of elemWords-word elements; lo, a SIGNED 64-bit integer, size, 1 .. 2^28, and row0 with row0 + size <= n: field(lo + j) is range_mult's,
 *   lo + j mod p|r; coef (usually -1) and busId as in pil2gl_logup_term.
 *   Window: outside rows row0 .. row0 + size - 1 a range adds 0 and m is NOT READ there: whatever those rows of m hold does not change s.
 *   Inside it m_r[i] counts as its field value by the rules above (Goldilocks words in [p, 2^64) mod p, any Fr pattern mod r).
 *   Zeros: a zero E_r[i] or D_u[i] adds 0 at that row and spoils no other term or row.
 *   out, outStride, outCol, alpha and beta: the block above's (three words a row over Goldilocks, one element over Fr).
 * Equivalence: s is word for word what pil2gl_[bn128_]logup_sum gives when each range is replaced by a k = 1 term with the tuple column
 * t_r[i] = field(lo_r + clamp(i - row0_r, 0, size_r - 1)), the numerator column m_r zeroed outside the window, the same coef and busId.
 * pil2gl_range_sum_plan: host-only, no device.  outInfo and *workBytes are logup_sum_plan's, with its values for the same n: the working
 * memory grows with neither nF nor nR.  PIL2GL_EINVAL: n > 2^28, nR outside 1 .. 8, nF > 8, nF + nR > 9, elemWords not 1 or 4.
 * pil2gl_[bn128_]range_sum_dev: hostTerms (nF entries; may be NULL when nF = 0) and hostRanges (nR entries) are HOST pointers; side.base,
 * side.sel and m are device pointers, 16-byte aligned, only read.  out = device, 16-byte aligned; its aliasing rule is the block above's
 * with every m_r counted as a read column of its matrix (all n rows of it): s as spare columns of m's matrix is the normal case.  The call
 * only ENQUEUES on the caller's stream: both tables travel as the kernel argument, nothing is copied (working slots as the block above).
 * PIL2GL_EINVAL, before any device call: what the plan refuses; everything the block above refuses for the f terms and out; size outside
 * 1 .. 2^28; row0 + size > n (n > 0); mCol >= mStride, a stride >= 2^32 or n mStride > 2^58 elements; a null or misaligned m; a
 * non-canonical Goldilocks coef or busId of a range; null hostRanges, or null hostTerms with nF > 0; an out that breaks the aliasing rule.
 * n = 0 is PIL2GL_OK, touches nothing and needs no device.
 * pil2gl_[bn128_]range_sum: host pointers throughout; each matrix staged up to the last element touched (an m up to its window's last
 * row), every part on 16 bytes, out's matrix goes up as it is and comes back with the column written.  Without a device the compute calls
 * return PIL2GL_ENODEV. */
typedef struct pil2gl_range_term {
    const uint64_t *m;                   /* the multiplicities: element of row i at m[(i mStride + mCol) elemWords] */
    uint64_t mStride, mCol;
    int64_t lo;                          /* the range's first value, signed */
    uint64_t size;                       /* its values, 1 .. 2^28 */
    uint64_t row0;                       /* the row of m that counts lo; row0 + size <= n */
    uint64_t coef[4];                    /* Goldilocks: word 0, canonical.  Fr: 4 Montgomery words */
    uint64_t busId[4];
} pil2gl_range_term;
int pil2gl_range_sum_plan(uint64_t n, uint64_t nF, uint64_t nR, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *workBytes);
int pil2gl_range_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                         const uint64_t *hostAlpha /* [3] */, const uint64_t *hostBeta /* [3] */, uint64_t *out, uint64_t outStride, uint64_t outCol,
                         uint64_t n, void *stream);
int pil2gl_bn128_range_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                               const uint64_t *hostAlpha /* [4] */, const uint64_t *hostBeta /* [4] */, uint64_t *out, uint64_t outStride,
                               uint64_t outCol, uint64_t n, void *stream);
int pil2gl_range_sum(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostAlpha,
                     const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);
int pil2gl_bn128_range_sum(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                           const uint64_t *hostAlpha, const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);

/* ---- clustered logUp sum: the im columns and s in one call (csrc/logup_cluster_plan.h, hints.hip, bn_scan.hip) ----
 * An AIR that carries the s of the two blocks above states (s - 's (1 - L1)) prod D_u - sum .. = 0, of degree nTerms + 1.  pil2's std library
 * keeps it inside the degree bound by clustering: a cluster c of terms gets a committed stage-2 column im_c, and the sum constraint becomes
 * s - 's (1 - L1) = sum_c im_c + (the terms left direct).  This block writes s AND every im_c from the trace columns.  The statement is this
 * header's own (tests/logup_cluster_ref.py restates it over Python integers):
 *   terms: nF pil2gl_logup_term (D_u, coef_u, w_u of the lookup grand sum above), then nR pil2gl_range_term (E_r, its window, m_r of the block above);
 *          0 <= nF <= 8, 0 <= nR <= 8, 1 <= nF + nR <= 9
 *   cluster[u], u < nF + nR: a HOST array, f terms first; each entry 0 .. nIm - 1, or PIL2GL_LOGUP_DIRECT.  1 <= nIm <= 9 and every id
 *          0 .. nIm - 1 is the cluster of at least one term
 *   frac_u[i] = coef_u w_u[i] / D_u[i]                        an f term
 *             = [in window] coefR m_r[i] / E_r[i]             a range
 *             = 0                                             where the denominator is 0, and outside the window (m is NOT READ there)
 *   im_c[i]   = sum_{cluster[u] = c} frac_u[i]                                           c < nIm, every row i < n
 *   s[i]      = s[i-1] + sum_c im_c[i] + sum_{cluster[u] = DIRECT} frac_u[i]             s[-1] = 0
 * s goes to (out, outStride, outCol) as in the blocks above; im_c to (im[c].base, im[c].stride, im[c].col), an element of s's shape: three
 * canonical words a row over Goldilocks (col + 2 < stride), one canonical Montgomery element over Fr.  Words between strided elements stay
 * untouched.  Field arithmetic is exact, so, word for word: s is what pil2gl_[bn128_]logup_sum (nR = 0) or range_sum gives on the same
 * terms, whatever the clusters; and im_c[i] = s_c[i] - s_c[i-1] with s_c that call on cluster c's terms alone.
 * pil2gl_logup_cluster_plan: host-only, no device.  outInfo: threads a workgroup, rows a lane of the first pass, workgroups, launches, depth
 * (logup_sum_plan's), words of an output element; *workBytes: Goldilocks logup_sum's, Fr bn_scan's levels and 32 n -- neither grows with the
 * terms or with nIm.  PIL2GL_EINVAL: n > 2^28, nF > 8, nR > 8, nF + nR outside 1 .. 9, nIm outside 1 .. 9, elemWords not 1 or 4.
 * pil2gl_[bn128_]logup_cluster_dev: hostTerms, hostRanges, hostCluster and hostIm are HOST pointers (hostTerms may be NULL when nF = 0,
 * hostRanges when nR = 0); the matrices and every output are device pointers, 16-byte aligned.  The call only ENQUEUES on the caller's
 * stream: the tables travel as the kernel argument, working memory is the library's slots.  Aliasing: EVERY output, s and each im_c, obeys
 * the rule of out in the blocks above against every matrix read (each m_r counted over all n rows), and no two outputs share a word: two
 * outputs may meet only as different word columns of ONE matrix (the same base, the same stride) -- s and its im columns as neighbouring
 * stage-2 columns, possibly spare columns of t's matrix, is the normal case.
 * PIL2GL_EINVAL, before any device call: what the plan refuses; what the blocks above refuse for the terms, the ranges, the challenges and
 * out; a null cluster array, an id >= nIm that is not PIL2GL_LOGUP_DIRECT, a cluster without a term; null hostIm; for an im column: col + 2 >=
 * stride over Goldilocks (col >= stride over Fr), a stride >= 2^32, n stride > 2^58, a null or misaligned base; an output on a column that is
 * read; two outputs sharing a word.  n = 0 is PIL2GL_OK, touches nothing and needs no device.
 * pil2gl_[bn128_]logup_cluster: host pointers throughout; the read matrices staged as in the blocks above; every DISTINCT output matrix
 * (base, stride) goes up as it is, to the last word an output writes in it, and comes back with its columns written.  Without a device the
 * compute calls return PIL2GL_ENODEV. */
#define PIL2GL_LOGUP_DIRECT (~(uint64_t)0)           /* a cluster entry: the term stays in the sum constraint, in no im column */
typedef struct pil2gl_logup_im_col {
    uint64_t *base;                      /* im_c of row i at base[(i stride + col) elemWords]: words col .. col + 2 over Goldilocks */
    uint64_t stride, col;
} pil2gl_logup_im_col;
int pil2gl_logup_cluster_plan(uint64_t n, uint64_t nF, uint64_t nR, uint64_t nIm, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *workBytes);
int pil2gl_logup_cluster_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                             const uint64_t *hostCluster /* [nF + nR] */, const pil2gl_logup_im_col *hostIm, uint64_t nIm,
                             const uint64_t *hostAlpha /* [3] */, const uint64_t *hostBeta /* [3] */, uint64_t *out, uint64_t outStride, uint64_t outCol,
                             uint64_t n, void *stream);
int pil2gl_bn128_logup_cluster_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                                   const uint64_t *hostCluster, const pil2gl_logup_im_col *hostIm, uint64_t nIm,
                                   const uint64_t *hostAlpha /* [4] */, const uint64_t *hostBeta /* [4] */, uint64_t *out, uint64_t outStride,
                                   uint64_t outCol, uint64_t n, void *stream);
int pil2gl_logup_cluster(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                         const uint64_t *hostCluster, const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha,
                         const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);
int pil2gl_bn128_logup_cluster(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR,
                               const uint64_t *hostCluster, const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha,
                               const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);

/* ---- grand product: the column z of a permutation or a connection from the trace columns (csrc/grand_prod_plan.h, hints.hip, bn_scan.hip) ----
 * The sibling of the block above for the `gprod` hints (grandProductPermutation.js:121-126, grandProductConnection.js:131-136): z in one
 * call from the columns where they lie, without the two extension columns num and den (the hints' tmp fields) that gprod needs ready.
 * The statement is this header's own (tests/grand_prod_ref.py restates it over Python integers):
 *   z[0] = 1,   z[i] = z[i-1] R[i-1]                          i < n   (calculateZ, polutils.js:132-145: the EXCLUSIVE product)
 *   R[i]   = prod_{u: den_u = 0} D_u[i]  /  prod_{u: den_u = 1} D_u[i]          an empty product is 1
 *   D_u[i] = B_u[i] + idCoef_u id_u[i] + gamma                 (id NULL: no such summand)
 *   B_u[i] = H_u[i]                                           when the term's side has no selector
 *          = (H_u[i] - beta) sel_u[i] + beta                  when it has one: sel's FIELD VALUE, not "non-zero"
 *   H_u[i] = (..(v_0 alpha + v_1) alpha .. ) alpha + v_{k_u-1}  first column highest; there is no bus id
 *   n <= 2^28 rows; 1 <= nTerms <= 40; the k of all terms add up to at most 64.  One term is a pil2gl_grand_prod_term: a
 *   pil2gl_tuple_side, its k (1 .. 16), den (0: a factor of the numerator, 1: of the denominator), an optional id column -- column idCol
 *   of the matrix (id, idStride) -- and idCoef, a HOST element of the challenges' field: over Goldilocks three canonical words of a
 *   cubic-extension element (else PIL2GL_EINVAL), over Fr four Montgomery words.  alpha, beta, gamma: HOST pointers, three words each
 *   over Goldilocks (x^3 = x + 1), four Montgomery words over Fr; all three must be given even where no term uses them.
 *   Elements count as field values by the rules above (Goldilocks words in [p, 2^64) mod p, any Fr pattern mod r).
 *   out: the block above's -- column outCol of (out, outStride); Goldilocks the three canonical words outCol .. outCol + 2 of a row
 *   of u64 words, Fr one canonical Montgomery element.  Words between a strided destination's elements stay as they are.
 *   Zeros: gprod's convention (stage-2 hints and the Fr block).  If any den factor of row i is zero, R[i] = 0 and every later z is 0; a
 *   zero num factor is plain arithmetic.  The hint's `result` is z[n-1]: the caller copies it.
 *   Equivalence: the column is word for word what pil2gl_gprod_dev(num, 3, den, 3, ..) / pil2gl_bn128_gprod_dev give on the two
 *   materialised product columns.
 * How the reference's identities map:
 *   permutation (grandProductPermutation.js:35-48 the tuples' compression tExp = alpha tExp + e, 57-70 the same for f, 97 and 105
 *   (exp - beta) sel + beta and + gamma): one term den = 0 with pi.f and selF, one term den = 1 with pi.t and selT; alpha, beta, gamma =
 *   std_alpha, std_beta, std_gamma.  Several permutations share one z by listing more terms.
 *   connection (grandProductConnection.js:35-45 the ks of the columns, 59-85 numExp *= a_j + delta ks'_j x + gamma and denExp *= a_j +
 *   delta S_j + gamma): per column j of ci.pols one term den = 0 with k = 1, column a_j, id = the x column (over Goldilocks
 *   pil2gl_build_x_dev(nBits, 1, ..)'s; over Fr the caller's own) and idCoef = delta ks'_j (ks' = 1, ks[0], ks[1], .., made on the
 *   host), and one term den = 1 with column a_j, id = column S_j, idCoef = delta; gamma = std_gamma; alpha and beta are unused but must
 *   be non-null.  A 12-column compressor takes 24 terms, an 18-column one 36: hence the limit of 40.
 *   Out of scope: pil2 std's bus-id form of a product bus, a gamma per term, and pil2gl/stark.py's resolve_hints_info, which sees tmp
 *   fields and not the identity's structure and stays as it is.
 * pil2gl_grand_prod_plan: host-only, no device.  outInfo is logup_sum_plan's: [0] = threads per workgroup of the first pass; [1] = rows
 * a lane of it takes (8, Fr 1); [2] = its workgroups; [3] = kernel launches of a call (Goldilocks 3: the fused first pass, the block
 * totals' scan, the fix-up; Fr 4 levels - 1: the compress, then bn128_gprod's inversion and scan); [4] = Goldilocks: block totals a lane
 * of the second pass walks, Fr: levels; [5] = u64 words of an output element's columns (3, or 1 element).  *workBytes = the working
 * memory, from the library's own slots: Goldilocks gsum's 24 n + 24 ceil(n / 2048); Fr the scan plan's bytes + 64 n (N and D of every
 * row).  PIL2GL_EINVAL: n > 2^28, nTerms outside 1 .. 40, sumK outside nTerms .. min(64, 16 nTerms), elemWords not 1 or 4.
 * pil2gl_[bn128_]grand_prod_dev: hostTerms is a HOST pointer to terms whose side.base, side.sel and id are device pointers, 16-byte
 * aligned, only read; matrices may overlap each other freely.  out = device, 16-byte aligned; its aliasing rule is logup_sum's, with the
 * id and selector matrices counted as read matrices: z as spare columns of t's matrix is the normal case.  The call only ENQUEUES on the
 * caller's stream: the packed term table travels as a kernel argument, nothing is copied and the host does not wait.  (On first use the
 * working slots are allocated, with a device synchronise when they grow.)  PIL2GL_EINVAL, before any device call: what the plan refuses,
 * k outside 1 .. 16, den above 1, a column >= its stride (outCol + 2 over Goldilocks), a stride >= 2^32 or n stride > 2^58 elements,
 * null terms, cols, base, out, alpha, beta or gamma, a non-canonical Goldilocks idCoef, a misaligned device pointer, an out that breaks
 * the aliasing rule.  n = 0 is PIL2GL_OK, touches nothing and needs no device.
 * pil2gl_[bn128_]grand_prod: host pointers throughout; each matrix staged up to the last element touched, every part on 16 bytes, out's
 * matrix goes up as it is and comes back with the column written.  Without a device the compute calls return PIL2GL_ENODEV. */
typedef struct pil2gl_grand_prod_term {
    pil2gl_tuple_side side;              /* the tuple's columns and the optional selector */
    uint64_t k;                          /* columns of this term's tuple, 1 .. 16 */
    uint64_t den;                        /* 0: the term multiplies the numerator, 1: the denominator */
    const uint64_t *id;                  /* the id column's matrix, or NULL */
    uint64_t idStride, idCol;
    uint64_t idCoef[4];                  /* Goldilocks: 3 canonical words.  Fr: 4 Montgomery words */
} pil2gl_grand_prod_term;
int pil2gl_grand_prod_plan(uint64_t n, uint64_t nTerms, uint64_t sumK, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *workBytes);
int pil2gl_grand_prod_dev(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha /* [3] */, const uint64_t *hostBeta /* [3] */,
                          const uint64_t *hostGamma /* [3] */, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_bn128_grand_prod_dev(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha /* [4] */, const uint64_t *hostBeta /* [4] */,
                                const uint64_t *hostGamma /* [4] */, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_grand_prod(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                      const uint64_t *hostGamma, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);
int pil2gl_bn128_grand_prod(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                            const uint64_t *hostGamma, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n);

/* ---- plookup: pil1's lookup argument from the trace columns, h1 and h2 (csrc/plookup_plan.h, hints.hip, bn_scan.hip) ----
 * The third pil1 argument library, grandProductPlookup.js, beside the two of the block above: its stage-1 half (the two kept expressions
 * that the h1h2 hint merges) and its stage-2 half (the gprod hint's z) without the extension columns num and den.  The statement is this
 * header's own (tests/plookup_ref.py restates it over Python integers); alpha, beta = std_alpha, std_beta (grandProductPlookup.js:10-11),
 * gamma, delta = std_gamma, std_delta (:12-13):
 *   H_t[i] = (..(t_0 alpha + t_1) alpha ..) alpha + t_{kT-1}                          :42-50  (first column highest)
 *   T[i]   = H_t[i]                               without selT
 *          = (H_t[i] - beta) selT[i] + beta       with selT: its FIELD VALUE          :51-55
 *   H_f[i] likewise over the kF columns of f                                           :64-72
 *   F[i]   = H_f[i]                               without selF
 *          = (H_f[i] - T[i]) selF[i] + T[i]       with selF: blended towards T of the SAME row, not towards beta    :73-77
 *   g      = gamma (1 + delta)
 *   num[i] = (F[i] + gamma) (T[i] + delta T[i+1] + g) (1 + delta)                      :120-135
 *   den[i] = (h1[i] + delta h2[i] + g) (h2[i] + delta h1[i+1] + g)                     :143-164
 *   i+1 is taken mod n: row n - 1's neighbour is row 0
 *   z[0] = 1,  z[i] = z[i-1] num[i-1] / den[i-1]                                      (calculateZ, polutils.js:132-145)
 *   n <= 2^28 rows.  f and t are pil2gl_tuple_sides of kF and kT columns, each 1 .. 16 and not tied to each other.  Elements count as
 *   field values by the rules above (Goldilocks words in [p, 2^64) mod p, any Fr pattern mod r).  The challenges are HOST pointers: three
 *   words each over Goldilocks (x^3 = x + 1), canonical or not -- the entry canonicalises them -- or four Montgomery words over Fr.
 *   h1, h2: columns (ptr, stride, col) of hDim words an element, over Goldilocks hDim = 1 (a base column, word col of a row of `stride`
 *   words) or 3 (words col .. col + 2), over Fr hDim = 1: one element.  The reference makes h a base column exactly when kF = kT = 1 and
 *   there is no selT (:91, hDim = max(fDim, tDim)); the product takes hDim as given and does not enforce that.
 *   Zeros: gprod's convention.  If either factor of den[i] is zero, the ratio of row i is 0 and every later z is 0; a zero num is plain
 *   arithmetic.  No read goes past row n - 1 of any matrix.  num[n-1] / den[n-1] does not enter z (for a valid lookup it closes the
 *   product: z[n-1] num[n-1] / den[n-1] = 1).  The hint's `result` is z[n-1]: the caller copies it.
 *   Equivalence: z is word for word what pil2gl_gprod_dev(num, 3, den, 3, ..) / pil2gl_bn128_gprod_dev give on the two materialised columns.
 *   Out of scope: more than one plookup per z, and pil2gl/stark.py's resolve_hints_info, which sees tmp fields and stays as it is.
 * pil2gl_plookup_plan: host-only, no device.  outInfo is logup_sum_plan's, for the PRODUCT call: [0] threads per workgroup of the first
 * pass; [1] rows a lane of it takes (8, Fr 1); [2] its workgroups; [3] kernel launches (Goldilocks 3: the fused first pass, the block
 * totals' scan, the fix-up; Fr 4 levels - 1: the compress, then bn128_gprod's inversion and scan); [4] Goldilocks: block totals a lane of
 * the second pass walks, Fr: levels; [5] u64 words of an output element's columns (3, or 1 element).  *workBytes = the product's working
 * memory, from the library's own slots: Goldilocks gsum's 24 n + 24 ceil(n / 2048); Fr the scan plan's bytes + 64 n.  The fold is one
 * launch and takes no working memory.  PIL2GL_EINVAL: n > 2^28, kF or kT outside 1 .. 16, elemWords not 1 or 4.
 * pil2gl_[bn128_]plookup_fold[_dev], the stage-1 half: writes F into column colF of (outF, strideF) and T into column colT of (outT,
 * strideT), hDim words an element, canonical (Fr: one canonical Montgomery element).  Over Goldilocks hDim = 1 is PIL2GL_EINVAL unless
 * kF = kT = 1 and selT is NULL (alpha and beta are then unused but must be non-null); with hDim = 3 and dense outputs (stride 3, col 0)
 * they are what pil2gl_h1h2_dev takes; over Fr they are strided columns for pil2gl_bn128_h1h2_dev.  One kernel, a lane a row; the _dev
 * form only ENQUEUES.
 * pil2gl_[bn128_]plookup_prod[_dev], the stage-2 half: z into (out, outStride, outCol) as logup_sum writes s -- Goldilocks the three
 * canonical words outCol .. outCol + 2, Fr one canonical Montgomery element; words between a strided destination's elements stay as they
 * are.  The _dev form only ENQUEUES on the caller's stream: the job travels as a kernel argument, nothing is copied and the host does not
 * wait.  (On first use the working slots are allocated, with a device synchronise when they grow.)
 * Buffers: _dev pointers (side.base, side.sel, h1, h2, the outputs) are device pointers, 16-byte aligned; everything but the outputs is
 * only read and may overlap freely.  An output obeys logup_sum's aliasing rule with the selector and the h matrices counted as read
 * matrices: z as spare columns of t's matrix is the normal case; outF and outT may be distinct columns of one matrix.  PIL2GL_EINVAL,
 * before any device call: what the plan refuses, an hDim that is not allowed, a column >= its stride (col + 2 for three-word elements), a
 * stride >= 2^32 or n stride > 2^58 elements, a null side, cols, base, column, output or challenge, a misaligned device pointer, an
 * output that breaks the aliasing rule.  n = 0 is PIL2GL_OK, touches nothing and needs no device.
 * The forms without _dev take host pointers throughout; each matrix is staged up to the last element touched, every part on 16 bytes, an
 * output's matrix goes up as it is and comes back with the column written.  Without a device the compute calls return PIL2GL_ENODEV. */
int pil2gl_plookup_plan(uint64_t n, uint64_t kF, uint64_t kT, uint32_t elemWords, uint32_t *outInfo /* [6] */, uint64_t *workBytes);
int pil2gl_plookup_fold_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha /* [3] */,
                            const uint64_t *hostBeta /* [3] */, uint32_t hDim, uint64_t *outF, uint64_t strideF, uint64_t colF, uint64_t *outT, uint64_t strideT,
                            uint64_t colT, uint64_t n, void *stream);
int pil2gl_bn128_plookup_fold_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha /* [4] */,
                                  const uint64_t *hostBeta /* [4] */, uint32_t hDim, uint64_t *outF, uint64_t strideF, uint64_t colF, uint64_t *outT, uint64_t strideT,
                                  uint64_t colT, uint64_t n, void *stream);
int pil2gl_plookup_fold(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                        const uint64_t *hostBeta, uint32_t hDim, uint64_t *hostOutF, uint64_t strideF, uint64_t colF, uint64_t *hostOutT, uint64_t strideT,
                        uint64_t colT, uint64_t n);
int pil2gl_bn128_plookup_fold(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                              const uint64_t *hostBeta, uint32_t hDim, uint64_t *hostOutF, uint64_t strideF, uint64_t colF, uint64_t *hostOutT, uint64_t strideT,
                              uint64_t colT, uint64_t n);
int pil2gl_plookup_prod_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *h1, uint64_t h1Stride,
                            uint64_t h1Col, const uint64_t *h2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha /* [3] */,
                            const uint64_t *hostBeta /* [3] */, const uint64_t *hostGamma /* [3] */, const uint64_t *hostDelta /* [3] */, uint64_t *out,
                            uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_bn128_plookup_prod_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *h1, uint64_t h1Stride,
                                  uint64_t h1Col, const uint64_t *h2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha /* [4] */,
                                  const uint64_t *hostBeta /* [4] */, const uint64_t *hostGamma /* [4] */, const uint64_t *hostDelta /* [4] */, uint64_t *out,
                                  uint64_t outStride, uint64_t outCol, uint64_t n, void *stream);
int pil2gl_plookup_prod(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostH1, uint64_t h1Stride,
                        uint64_t h1Col, const uint64_t *hostH2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                        const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol,
                        uint64_t n);
int pil2gl_bn128_plookup_prod(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostH1, uint64_t h1Stride,
                              uint64_t h1Col, const uint64_t *hostH2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                              const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *hostOut, uint64_t outStride,
                              uint64_t outCol, uint64_t n);

/* ---- synthetic workload for bench.py / tests (not a reference operator) ----
 * witness of nPairs independent Fibonacci machines (test/state_machines/sm_fibonacci/sm_fibonacci.js:12-23):
 * cm is 2^nBits x (2*nPairs) row-major (l1_k, l2_k), hostInit = 2*nPairs canonical start values (host pointer). */
int pil2gl_synth_fibonacci_dev(uint32_t nBits, uint32_t nPairs, const uint64_t *hostInit, uint64_t *cm, void *stream);

/* ---- the WASM module's scalar exports (glwasm.js:47-96,1269-1275: add, mul, square of field elements) ------------
 * Host arithmetic, one element per call (the reference calls them from JS for twiddles and shifts); no device needed. */
uint64_t pil2gl_add(uint64_t a, uint64_t b);
uint64_t pil2gl_mul(uint64_t a, uint64_t b);
uint64_t pil2gl_square(uint64_t a);

/* ---- diagnostics used by the parity tests ---------------------------------- */
/* element-wise a*b, a+b, a-b on the device (n elements, host pointers) */
int pil2gl_selftest_field(const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *mul, uint64_t *add, uint64_t *sub);
/* host-only: the op-list after validation, value numbering (each distinct cell loaded once, common sub-expressions
 * merged) and live-range renumbering of temporaries, as the kernel runs it (without Horner-chain fusion).
 * outOps must hold 2*nOps+16 entries; outInfo[0] = temporaries needed, outInfo[1] = ops written. */
int pil2gl_debug_compact_program(const glx_program *prog, glx_op *outOps, uint32_t *outInfo);
/* host-only: run the optimiser, generate the straight-line kernel source of the program and compile it with hiprtc
 * (the path long programs take at run time); reports the code object size and the number of fused Horner terms. */
int pil2gl_debug_jit_compile(const glx_program *prog, const glx_ctx *ctx, uint64_t *codeBytes, uint32_t *fusedOps);
/* host-only: the program as pil2gl_eval_program_dev optimises it for this context, Horner fusion included: outInfo[0] = temporary
 * slots (what the choice between the compiled kernel and the two interpreter forms reads), [1] = ops, [2] = fused Horner terms */
int pil2gl_debug_plan_program(const glx_program *prog, const glx_ctx *ctx, uint32_t *outInfo);
/* host-only: how many times this process has launched the one-launch BN128 path kernel (pil2gl_bn128_roots_from_group_proofs); the tests
 * assert that a batch of openings went through it, once, and not through a permutation call per chunk and level */
uint64_t pil2gl_debug_bn128_path_launches(void);
/* host-only, no device: the kernel launches fft / ifft / interpolate / the extension from coefficients make for 2^nBits rows x nPols
 * columns (the two extensions: onto cosetCount of the 2^(nBitsExt - nBits) cosets, 0 = all; fft / ifft ignore both), as the
 * transforms plan them under the environment's test hooks (PIL2GL_NTT_KMAX, PIL2GL_NTT_GENERIC, PIL2GL_LDE_WIDEFWD).
 * Writes *nLaunches records of PIL2GL_PLAN_LAUNCH_WORDS words to out (room for maxLaunches; 64 always suffice), in launch order:
 *   [0] kind: 0 inverse DIF pass, 1 forward DIF pass, 2 DIT pass, 3 mid kernel (csrc/ntt.hip)   [1] lo, [2] k: index bits [lo, lo+k)
 *   [3] columns per slot group, [4] slot groups, [5] column chunks   [6] workgroup x (tile slots), [7] workgroup y
 *   [8] fixed-geometry instance: 0 (any-geometry), 15 or 16 slots   [9] mid kernel: rows per lane of the instance (passes: 0)
 *   [10] LDS bytes   [11] workgroups   [12] scatters to bit-reversed rows   [13] stores canonical values
 * A call of 2^0 rows (a copy / a broadcast) or of no columns has no launches. */
#define PIL2GL_PLAN_FFT 0
#define PIL2GL_PLAN_IFFT 1
#define PIL2GL_PLAN_INTERPOLATE 2
#define PIL2GL_PLAN_EXTEND_COEFS 3
#define PIL2GL_PLAN_LAUNCH_WORDS 14
int pil2gl_debug_plan_transform(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount,
                                uint32_t *out, uint32_t maxLaunches, uint32_t *nLaunches);
/* host-only, no device: how the launches of the same call (same arguments, same order) are dealt to workgroups.  A workgroup of a 16-slot
 * fixed-geometry instance owns one row tile and a run of up to W consecutive column chunks of it; every other instance has W = 1.
 * Per launch PIL2GL_PLAN_GRID_WORDS words:
 *   [0] workgroups launched   [1] W   [2] row tiles   [3] row tiles per outer index (hi)   [4] column chunks
 * so that [11] of pil2gl_debug_plan_transform, the tiles of the launch, is [2] x [4], and [0] = [2] x ceil([4] / [1]). */
#define PIL2GL_PLAN_GRID_WORDS 5
int pil2gl_debug_plan_transform_grid(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount,
                                     uint32_t *out, uint32_t maxLaunches, uint32_t *nLaunches);
/* the walk itself, from the function the kernels run: for workgroups [firstBlock, firstBlock + count) of launch number `launch` of that
 * call and steps s < W, out[((b - firstBlock) * W + s) * 3 + 0..2] = outer index hi, row tile gt within it, column chunk cc of the tile
 * the workgroup works on in step s; 0xffffffff thrice where it has no such step */
int pil2gl_debug_transform_walk(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount, uint32_t launch,
                                uint32_t firstBlock, uint32_t count, uint32_t *out);
/* every workgroup and step of that launch through the same function: counts[0] = tiles (hi, gt, cc) reached exactly once, [1] = tiles
 * never reached, [2] = visits beyond a tile's first or outside the launch */
int pil2gl_debug_transform_walk_cover(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount, uint32_t launch,
                                      uint64_t *counts);
/* the two hand-written Goldilocks products on n pairs of arbitrary u64 operands (host pointers): x[i] = a*b by the exact form
 * the transform kernels use (gl_field.cuh mul_lazy_x), pb[i] = a*b by the flagged form of the S-boxes (mul_lazy_b), both canonical;
 * flag[i] != 0 where the flagged form asks to be recomputed (its last subtraction borrowed: probability ~2^-32 on random operands) */
int pil2gl_selftest_products(const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *x, uint64_t *pb, uint64_t *flag);
/* `layers` consecutive Poseidon MDS layers (glwasm.js:428-440 matrix) applied to n 12-element states (host pointers,
 * any u64 representatives in, canonical out): mfma = 1 the matrix-core layer the hash kernels use, 0 the vector-ALU one */
int pil2gl_selftest_mds(const uint64_t *states, uint64_t n, uint32_t layers, int mfma, uint64_t *out);
/* the Poseidon-12 permutation (glwasm.js:216-426) of n 12-element states (host pointers, any u64 representatives in, canonical
 * out) in each of the library's statements of it: what = 0 the hash kernels' form (matrix-core MDS, rounds 4..25 four to a
 * linear layer), 1 matrix-core MDS with one layer per round, 2 vector ALU only; 3 / 4 = rounds 4..25 ALONE (folded-constant
 * form: lane 0 + c, x^7, MDS) in the forms of 0 / 1 -- arbitrary states reach the partial rounds' recombination that way */
int pil2gl_selftest_poseidon(const uint64_t *states, uint64_t n, int what, uint64_t *out);
/* diagnostics: the shader clock (MHz) under the Poseidon kernels' own load -- every workgroup of a chip-filling launch runs `iters`
   permutations between two readings of the shader-clock and the 100 MHz counters; mhz[3] = median, 5th, 95th percentile.
   (sysfs reports the nominal DPM level; under this load the MI355X runs near 1.9 GHz, which is what issue-cycle figures need) */
int pil2gl_selftest_clock(uint32_t iters, double *mhz);
/* extension a*b and 1/a on the device (n triples) */
int pil2gl_selftest_ext(const uint64_t *a, const uint64_t *b, uint64_t n, uint64_t *mul, uint64_t *inv);

#ifdef __cplusplus
}
#endif
