/*
 * ecamd_host.h -- host-side planning for the MI355X erasure-code backend (libecamd_host.so).
 *
 * Pure host C ABI (no HIP types): GF(2^16) arithmetic, the reference generator matrix, and the
 * "fragment maps" (which fragments to read, which to write, with which coefficients) that the
 * device kernels apply.  Each entry point restates a piece of the reference's built-in
 * liberasurecode_rs_vand codec:
 *
 *   ecamd_gf16_mul / ecamd_gf16_inv   rs_galois_mult / rs_galois_inverse
 *                                     (src/builtin/rs_vand/rs_galois.c:90-117)
 *   ecamd_rs_generator                make_systematic_matrix (liberasurecode_rs_vand.c:240-289)
 *   ecamd_gf16_invert                 gaussj_inversion (liberasurecode_rs_vand.c:293-334)
 *   ecamd_rs_decode_map               coefficient rows of liberasurecode_rs_vand_decode
 *                                     (liberasurecode_rs_vand.c:426-481); missing parity is
 *                                     expressed directly over the first k available fragments
 *   ecamd_rs_check_map                the same algebra for every surviving fragment beyond the first
 *                                     k: what the inputs imply it holds (no reference counterpart)
 *   ecamd_rs_locate_map               the check map with each column's ratios to its first row: which
 *                                     single fragment explains a syndrome (no reference counterpart)
 *   ecamd_rs_locate_pairs_map         the check map with, for every pair of columns of [A | I], two pivot
 *                                     rows and the rows' combinations of them: which two fragments
 *                                     explain a syndrome (no reference counterpart)
 *   ecamd_rs_correct_map              the check map with, per column and per pair of columns of [A | I],
 *                                     the pivot row(s) and the inverse that turn a located stripe's
 *                                     syndromes into error values (no reference counterpart)
 *   ecamd_rs_reconstruct_map          coefficient row of liberasurecode_rs_vand_reconstruct
 *                                     (liberasurecode_rs_vand.c:483-558)
 */
#ifndef ECAMD_HOST_H
#define ECAMD_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ecamd_gf16_mul(int a, int b);
int ecamd_gf16_inv(int a);

/* (k+m) x k row-major systematic generator into out; 0 on success. */
int ecamd_rs_generator(int k, int m, int *out);

/* Inverse of the n x n matrix a into inv; 0 on success, -1 if singular. */
int ecamd_gf16_invert(const int *a, int *inv, int n);

/* Decode map for a -1 terminated missing list.  inputs[k] receives the first k available
 * fragment indices; outputs[*nout] the rebuilt fragment indices (missing data, then missing
 * parity if rebuild_parity); coeff[*nout * k] the rows.  Returns -1 if more than m are missing. */
int ecamd_rs_decode_map(const int *G, int k, int m, const int *missing, int rebuild_parity,
                        int *inputs, int *outputs, int *coeff, int *nout);

/* Reconstruct map for one destination: inputs[*ninputs] and coeff[*ninputs]. */
int ecamd_rs_reconstruct_map(const int *G, int k, int m, const int *missing, int dest, int *inputs,
                             int *ninputs, int *coeff);

/* Check map (ecamd_rs_check, ecamd.h) for a -1 terminated missing list (NULL: none).
 * inputs[k]: first k available; checked[*ncheck]: the other available fragments, ascending;
 * coeff[*ncheck * k]: row i gives fragment checked[i] over the inputs.  With nothing missing the
 * rows are the generator's parity rows (the encode map); otherwise row f is G[f] * inv(G[inputs]),
 * the algebra ecamd_rs_decode_map uses for missing parity.  -1 if more than m missing; exactly m
 * missing leaves *ncheck 0. */
int ecamd_rs_check_map(const int *G, int k, int m, const int *missing, int *inputs, int *checked,
                       int *coeff, int *ncheck);

/* Locate map (ecamd_rs_locate, ecamd.h): what ecamd_rs_check_map returns, plus ratio[(*ncheck - 1) * k]
 * with ratio[(r - 1) * k + j] = coeff[r * k + j] / coeff[j] (nothing for *ncheck < 2; ratio may then be
 * NULL).  One bad input j leaves every word's syndrome S_r = coeff[r][j] * e, so it is the one j with
 * S_r == ratio[r - 1][j] * S_0 for all r >= 1; one bad checked fragment leaves every other row zero.
 * Every entry of a check map of this code is non-zero.  -1 if more than m missing. */
int ecamd_rs_locate_map(const int *G, int k, int m, const int *missing, int *inputs, int *checked,
                        int *coeff, int *ncheck, int *ratio);

/* Pair plan (ecamd_rs_locate_pairs, ecamd.h): what ecamd_rs_check_map returns, plus what names the TWO
 * bad fragments of a stripe.  The participants are the k inputs (0..k-1), then the *ncheck checked
 * rows (k..k+*ncheck-1); participant c has column c of the syndrome matrix [coeff | I].  With R =
 * *ncheck >= 4 there are *npairs = P(P-1)/2 pairs a < b of the P = k + R participants, in the order
 * (0,1), (0,2), ..., (P-2,P-1).  For pair i: pivots[2i], pivots[2i+1] = two rows (p, q) whose 2 x 2 minor
 * of columns a, b is non-singular, and L[(i*R + r)*2 + 0..1] with
 *     S_r == L[r][0] * S_p ^ L[r][1] * S_q   for every row r
 * exactly when the syndrome (S_0..S_{R-1}) of a word lies in the span of columns a and b; rows p and q
 * of L are (1,0) and (0,1).  A pair whose two columns are linearly dependent is never tested: its
 * pivots are (-1, -1) and its L rows zero.  *independent4 is 1 when any four columns of [coeff | I]
 * are linearly independent (every check map of this code that was tried; at most C(32,4) rank
 * computations): a word that needs two columns then lies in the span of no other pair, so the pair
 * that explains every dirty word of a stripe is unique.  With R < 4 there is no plan: *npairs 0,
 * *independent4 0, pivots and L (may be NULL) untouched.  -1 if more than m missing. */
int ecamd_rs_locate_pairs_map(const int *G, int k, int m, const int *missing, int *inputs, int *checked,
                              int *coeff, int *ncheck, int *npairs, int *pivots, int *L,
                              int *independent4);

/* Correction plan (ecamd_rs_correct, ecamd.h): what ecamd_rs_check_map returns, plus what turns the
 * syndromes of a LOCATED stripe into the error values of its bad fragment(s).  Participants as in the
 * pair plan: the k inputs (0..k-1), then the R = *ncheck checked rows.  With S_r = stored_r ^ sum_j
 * coeff[r][j] * input_j per 16-bit word:
 *   participant c: pivot[c] is a row where column c of [coeff | I] is non-zero -- row 0 for an input,
 *     its own row for a checked fragment -- and scale[c] the inverse of that entry (1 for a checked
 *     fragment); when c is the only bad fragment its error is e_c = scale[c] * S_pivot[c].
 *   pair i of a < b, in the pair plan's order (0,1), (0,2), ..., for R >= 2 (*npairs = P(P-1)/2):
 *     pair_pivots[2i], [2i+1] = rows (p, q) with a non-singular 2 x 2 minor of columns a, b -- where the
 *     pair plan exists (R >= 4) the very rows ecamd_rs_locate_pairs_map returns -- and minv[4i..4i+3]
 *     that minor's inverse, row-major:
 *         e_a = minv[0] * S_p ^ minv[1] * S_q,   e_b = minv[2] * S_p ^ minv[3] * S_q.
 *     Dependent columns: pivots (-1, -1) and a zero minv.
 * XORing the error value into the stored word gives the codeword that agrees with every other
 * participant -- what a decode with that fragment listed as missing writes.  R < 2: *npairs 0.  R == 0:
 * every pivot -1 and scale 0.  npairs, pair_pivots and minv may be NULL (singles only).  -1 if more
 * than m missing. */
int ecamd_rs_correct_map(const int *G, int k, int m, const int *missing, int *inputs, int *checked,
                         int *coeff, int *ncheck, int *pivot /* k+R */, int *scale /* k+R */,
                         int *npairs, int *pair_pivots /* 2 per pair */, int *minv /* 4 per pair */);

/* LDS split-table image for rows [row0,row0+width) x inputs [col0,col0+ncols) of the R x K
 * matrix coeff; width in {2,4,8}.  Returns the byte count written (ncols*512*width*2). */
int ecamd_split_tables(const int *coeff, int R, int K, int row0, int width, int col0, int ncols,
                       uint8_t *out);

/* ---- flat-XOR HD codes (src/builtin/xor_codes/) ---- */

/* Parity / data bitmaps of a supported (k, m, hd) code (include/xor_codes/xor_hd_code_defs.h);
 * -1 if the code is not one init_xor_hd_code accepts (xor_hd_code.c:664-693). */
int ecamd_xor_code_tables(int k, int m, int hd, unsigned int *parity_bms, unsigned int *data_bms);

/* Check / locate plan of a supported (k, m, hd) code (ecamd_xor_check, ecamd_xor_locate, ecamd.h):
 * sig[f], f < k+m, is the mask of parity rows whose syndrome S_p = stored parity p ^ XOR of the data
 * in parity bitmap p a bad fragment f disturbs -- for data fragment j the rows p with bit j in parity
 * bitmap p, for parity p the single bit 1 << p.  Every signature is non-zero and the k+m of a code
 * are distinct, so one bad fragment is always located: per 16-bit word, fragment f explains the word
 * iff all its non-zero syndromes are equal and the set of rows with a non-zero syndrome is sig[f].
 * The accepted codes have m in {3, 5, 6} and k <= 20.  -1 (sig untouched) if the code is not one
 * init_xor_hd_code accepts. */
int ecamd_xor_check_plan(int k, int m, int hd, unsigned int *sig /* k+m */);

/* The same plan for a stripe with fragments missing (ecamd_xor_check_degraded, ecamd_xor_locate_degraded,
 * ecamd_xor_correct_degraded, ecamd.h).  The m check rows start as fragment masks h_p = parity bitmap p
 * | 1 << (k+p) and are reduced by this rule, which callers may rely on:
 *   - the missing fragments are taken in ascending index order, whatever the order of the list;
 *   - for a missing fragment f the pivot is the lowest-index row still alive that has bit f;
 *   - the pivot is XORed into every other live row that has bit f, and is then retired;
 *   - if no live row has bit f, nothing happens.
 * rows[p] is the reduced row p, or 0 if row p was retired.  A surviving row p contains the stored
 * parity k+p and no missing fragment, so "row p" stays the check that parity p owns, with status bit
 * k+p.  sig[f] is the mask of p with bit f in rows[p]: 0 for a missing fragment and for an available
 * one that no surviving row contains.  *covered (may be NULL) is the mask of fragments with sig[f] != 0.
 * With nothing missing (missing NULL or {-1}) rows[p] = h_p and sig is ecamd_xor_check_plan's.
 * Signatures need not be distinct any more: fragments that share one cannot be told apart and are
 * located together.  With at most hd - 2 missing every available fragment is covered; at hd 4 with one
 * missing the signatures are still distinct.
 * Returns the number of surviving rows (0 is possible), or -1 with every output untouched for a code
 * init_xor_hd_code rejects, an index >= k+m, a repeated index, or more than m entries (`missing` ends
 * at its first negative entry). */
int ecamd_xor_check_plan_degraded(int k, int m, int hd, const int *missing /* -1 terminated, may be NULL */,
                                  unsigned int *rows /* m */, unsigned int *sig /* k+m */,
                                  unsigned int *covered /* may be NULL */);

/* Exact plan of a reference operation on k+m buffers: op 0 = xor_code_encode, 1 = xor_hd_decode
 * (arg = decode_parity), 2 = xor_reconstruct_one (arg = index).  outputs[*nout] are the buffers
 * the reference modifies, sources[i] the bitmask of ORIGINAL buffers whose XOR output i ends up
 * holding.  Returns the reference's return code (-100 for bad arguments). */
int ecamd_xor_plan(int op, int k, int m, int hd, const unsigned int *parity_bms,
                   const unsigned int *data_bms, const int *missing, int arg, int *outputs,
                   uint64_t *sources, int *nout);

/* The decode table of a supported (k, m, hd) code, as ecamd_xor_decode_masks (ecamd.h) uploads it: one
 * 16-byte entry per ascending list of fewer than hd lost fragments, the empty list included, at the rank
 * of the list's mask (csrc/hip/ecamd_xor_masks_plan.hpp: xor_masks_rank, and the entry's layout --
 * byte 0 the number of outputs, bytes 1-3 the output fragments, three uint32 source masks).  Entry by
 * entry it is ecamd_xor_plan(op 1, the list, decode_parity 1) with the outputs ascending and the bits of
 * the lost fragments dropped from every source: the bytes xor_hd_decode leaves when the lost slots were
 * zero-filled.  The outputs below k, unchanged, are the plan of decode_parity 0.
 * Returns the number of entries, sum of C(k+m, t) over t < hd (at most 2952, at (20,6,4)); the table is
 * written when it is not NULL and `capacity` (in entries) is at least that number.  -1 for a code
 * init_xor_hd_code rejects; -2, which no shipped code returns, if a plan does not have that form. */
int ecamd_xor_decode_masks_plan(int k, int m, int hd, void *table, int capacity);

/* The 80-byte fragment header the framed device calls stamp (ecamd_frame_encode, _reconstruct,
 * _reconstruct_masks in ecamd.h), from the text the device kernels run (csrc/hip/ecamd_frame_header.hpp):
 * add_fragment_metadata on a zeroed header for fragment idx of an object of obj_size bytes with payloads
 * of blocksize bytes.  payload_crc is stored when checksum is 2 (CRC32); any other type is stored, not
 * computed.  legacy != 0: the metadata checksum by liberasurecode_crc32_alt instead of zlib's crc32.
 * Returns 0; -1 for a null out or idx < 0. */
int ecamd_frame_header(int idx, uint32_t blocksize, uint64_t obj_size, int backend, int checksum,
                       uint32_t payload_crc, int legacy, uint8_t out[80]);

/* xor_hd_fragments_needed (xor_hd_code.c:209-412); needed ends with -1. */
int ecamd_xor_fragments_needed(int k, int m, int hd, const unsigned int *parity_bms,
                               const unsigned int *data_bms, const int *to_reconstruct,
                               const int *to_exclude, int *needed);

/* Batched planning: liberasurecode_fragments_needed for nstripes stripes at once.
 * Stripe s: to_reconstruct at recon + s*list_stride, to_exclude at excl + s*list_stride (each
 * -1 terminated within list_stride entries); its needed list (-1 terminated, padded with -1) at
 * needed + s*(k+m+1) and its return code at rcs[s].  backend 6 (rs_vand): the first k indices
 * neither missing nor excluded (src/backends/rs_vand/liberasurecode_rs_vand.c:119-145), rc -1 if
 * fewer remain; backend 3 (flat_xor_hd): xor_hd_fragments_needed.  Returns -1 on bad arguments. */
int ecamd_fragments_needed_batch(int backend, int k, int m, int hd, const int *recon,
                                 const int *excl, int list_stride, int nstripes, int *needed,
                                 int *rcs);

/* Devices the per-call path (ecamd_host_map_apply / ecamd_host_xor_apply) spreads calls over:
 * every one of ndev visible devices, or the comma-separated subset named by spec (the
 * ECAMD_PERCALL_DEVICES environment variable; NULL or "" = all; out-of-range or repeated ids are
 * dropped, and a spec naming none of them means all).  Writes up to max ids to devs, returns the
 * count.  Call n of a process goes to devs[n % count].  One process per GPU names its device
 * ("3": liberasurecode_amd/shard.py does so for its ranks); the spec "current" (not parsed here)
 * makes the per-call path use the device current on the thread of its first call, resolved once. */
int ecamd_percall_device_plan(int ndev, const char *spec, int *devs, int max);

/* Host copies of one per-call request (host/copy_pool.cpp): dst[i] <- src[i], len[i] bytes, i < n,
 * regions not overlapping.  Batches of 1 MiB or more are split into 256 KiB pieces shared by the
 * caller and ECAMD_COPY_THREADS helper threads (default 4, 0 = off; one request uses them at a
 * time, a caller that finds them busy copies alone).  Complete on return; 0, or ECAMD_EINVAL
 * (-22) for null arrays.  Used by the per-call staging (pack / unpack) and by liberasurecode.so.1
 * for its object <-> fragment copies. */
int ecamd_host_copy(int n, void *const *dst, const void *const *src, const int64_t *len);
/* The same with a second destination per copy: dst[i] <- src[i] and, when dst2 and dst2[i] are
 * not null, dst2[i] <- src[i], reading the source from DRAM once (each 256 KiB piece is copied to
 * dst2 and then from there, cache-resident, to dst).  Used by the per-call staging pack when the
 * frontend hands it an input tee (ecamd_percall_tee_arm, ecamd.h). */
int ecamd_host_copy2(int n, void *const *dst, void *const *dst2, const void *const *src,
                     const int64_t *len);

/* Bitsliced GF(2^16) maps (host/bitslice.hpp): the XOR network built for an R x K matrix
 * (R <= 8, K <= 32, at most `cap` shared temporaries per input) evaluated on 32 words per input
 * (in: K x 32, out: R x 32; *ops = VALU ops of the network per tile), and the HIP source of the
 * kernel specialised to it, inputs loaded into registers (depth 0) or through a per-wave LDS ring
 * of 2 or 4 inputs (returns the source length; writes up to size-1 bytes + NUL). */
int ecamd_bitslice_eval(const int *coeff, int R, int K, int cap, const uint16_t *in, uint16_t *out,
                        int *ops);
int64_t ecamd_bitslice_source(const int *coeff, int R, int K, int cap, int depth, char *buf,
                              int64_t size);
/* Test scaffolding (tests/test_bitslice_launch_forms.py), not part of the product API: what the
 * generator makes of a request, without a GPU or a compile.
 * Compile requests as libecamd writes them and ecamd_jitc reads them (bitslice_request): the text of
 * the plain one-wave form's request for an R x K matrix with the given option bits (kBsOpt*, 0:
 * none), the option bits a request text parses to (-1: not a request), and the source ecamd_jitc
 * compiles for a request text (-1: not a request).  Lengths and buffers as ecamd_bitslice_source. */
int64_t ecamd_bitslice_wave_request(const int *coeff, int R, int K, int cap, int opts, char *buf,
                                    int64_t size);
int ecamd_bitslice_request_opts(const char *request);
int64_t ecamd_bitslice_request_source(const char *request, char *buf, int64_t size);

#ifdef __cplusplus
}
#endif
#endif
