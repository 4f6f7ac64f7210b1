/*
 * ecamd.h -- MI355X device-resident erasure-code engine (libecamd.so), C ABI.
 *
 * This is the batched extension the reference does not have ("B2 ... A batched,
 * device-pointer extension API is new"): S independent stripes whose fragments already live in
 * HBM are encoded / decoded / reconstructed by one kernel launch.  The per-call drop-in ABIs of
 * the reference (liberasurecode_rs_vand.h, xor_code.h, erasurecode.h) are layered on top of it.
 *
 * All pointers named d_* are device pointers; `stream` is a hipStream_t (NULL = default stream).
 * Calls are asynchronous on `stream` unless stated.  Every entry point returns 0 on success and a
 * negative value on failure (ecamd_last_error() gives the reason).  There is no CPU fallback: with
 * no HIP device every call fails with ECAMD_ENODEV.
 *
 * Fragment layout ("strided"): fragment f of stripe s starts at
 *     base + s * stripe_stride + f * frag_stride
 * so both [S][k+m][F] (frag_stride = F, stripe_stride = (k+m)*F) and fragment-major
 * [k+m][S][F] layouts are expressible.  base, strides and offsets must be 16-byte aligned;
 * blocksize (bytes per fragment payload) may be any value >= 1.
 */
#ifndef ECAMD_H
#define ECAMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECAMD_ENODEV (-19)
#define ECAMD_EINVAL (-22)
#define ECAMD_ENOMEM (-12)
#define ECAMD_EHIP (-5)

/* 0 if a HIP device is usable, ECAMD_ENODEV otherwise. */
int ecamd_init(void);
int ecamd_device_count(void);
/* The calling thread's current HIP device (every call below works on it). */
int ecamd_get_device(int *dev);
int ecamd_set_device(int dev);
const char *ecamd_last_error(void);
/* Launch-geometry knobs for sweeps ("threads", "wgs_per_cu", "nt", "grid_mult", "tiles_per_slot",
 * "xor_tiles_per_slot", "bs_tiles_per_slot", "scatter_lanes", ...; every setting produces
 * bit-identical results, only the launch shape changes); 0 restores the default (for
 * xor_ / bs_tiles_per_slot 0 means one launch per pass, a negative value the default).  The list
 * of knobs, with each one's default and rule: csrc/host/tune.hpp (tune_knobs.def).  Safe to
 * call while other threads launch: each launch reads each knob once. */
int ecamd_tune(const char *key, int value);

/* Bitsliced 8-output passes (hip/ecamd_jit.hip): 1 if run-time compilation (hiprtc) is usable;
 * ecamd_bitslice_wait() blocks until every kernel compile started so far has finished and returns
 * how many failed (their maps keep using the LDS-table kernels); ecamd_bitslice_entries() is the
 * number of matrices held (bounded by the "bitslice_entries" knob, least recently used evicted and
 * their modules unloaded once no launch can still use them). */
int ecamd_bitslice_available(void);
int ecamd_bitslice_wait(void);
int ecamd_bitslice_entries(void);
/* Bitsliced kernel launches this process has enqueued (tests pin which kernel ran). */
long long ecamd_bitslice_launches(void);
/* ---- Development hooks: for the project's tests and tools, not part of the product API ---- */
/* Test scaffolding (tests/test_bitslice_launch_forms.py): the cache name (no directory, no ".co") of
 * the code object of a compile request text for target `arch`, as the shipped directory and the
 * per-user cache hold it: its length, < 0 on error. */
int ecamd_bitslice_object_name(const char *request, const char *arch, char *buf, int size);
/* Measurement hook (tools/launch_timeline.py; DESIGN.md §4 "Per-launch cost" says why it is a call and
 * not an environment variable): while `records` > 0, launches of the plain one-wave bitsliced kernel
 * -- from every thread of the process, so call it from a tool that launches from one -- run its
 * timeline form, which writes tile t's 32-byte record {start, end (64-bit ticks of the 100 MHz wall
 * clock), tile, XCC id, hardware id, 0} to buf + 32 t for t < records.  `buf` is device memory the
 * caller owns and keeps until those launches have finished; records 0 turns it off.  Results are
 * unchanged. */
int ecamd_bitslice_timeline(void *buf, unsigned records);

/* Which kernel an rs_vand operation's passes run on this process's current device, for fragments
 * of `blocksize` bytes: encode (missing NULL), decode of the -1 terminated `missing` (dest < 0;
 * rebuild_parity as ecamd_rs_decode) or single-destination reconstruct of `dest`.  Returns
 * ECAMD_FORM_TABLES (the LDS-table kernels serve it by shape or knob), ECAMD_FORM_BITSLICED (its
 * bitsliced kernel is loaded: shipped with the library, cached, or compiled), ECAMD_FORM_COMPILING
 * (being compiled; the LDS tables serve it meanwhile) or ECAMD_FORM_UNAVAILABLE (it would take the
 * bitsliced kernel but none can be had -- no shipped code object and no ecamd_jitc / libhiprtc, or
 * the compile failed: the LDS tables serve it, byte-identically); < 0 on error.  Asking starts the
 * compile of a map not seen before (knob "bitslice" 2: waits for it), as its first launch would. */
#define ECAMD_FORM_TABLES 0
#define ECAMD_FORM_BITSLICED 1
#define ECAMD_FORM_COMPILING 2
#define ECAMD_FORM_UNAVAILABLE 3
int ecamd_rs_kernel_form(int k, int m, const int *missing, int dest, int rebuild_parity, int64_t blocksize);

/* Build time, no GPU needed: compile the bitsliced kernels of one rs_vand operation (arguments as
 * ecamd_rs_kernel_form) for target `arch` ("gfx950") into `dir` -- the library's jit/ directory,
 * which the run time searches before the per-user cache -- under the names the run time looks up
 * with the current knobs.  Returns the number of code objects present (0: the operation takes no
 * bitsliced kernel), < 0 on error (ecamd_jitc missing or failed). */
int ecamd_bitslice_prebuild(int k, int m, const int *missing, int dest, int rebuild_parity, const char *arch,
                            const char *dir);
/* The same for the CHKSUM_CRC32 framed encode (ecamd_frame_encode) of a code (backend 6 rs_vand or 3
 * flat_xor_hd): its bitsliced codec-and-checksum kernel, one per code whatever the object size.
 * Returns 1 when present, 0 when that encode takes no bitsliced kernel, < 0 on error. */
int ecamd_frame_prebuild(int backend, int k, int m, int hd, const char *arch, const char *dir);

/* ---- GF(2^16) fragment maps: outputs[r] = sum_j coeff[r*K+j] * inputs[j] (16-bit LE words) ---- */
typedef struct ecamd_map ecamd_map;

/* Prepare the R x K coefficient matrix for the current device (split tables in HBM). */
int ecamd_map_create(const int *coeff, int R, int K, ecamd_map **out);
void ecamd_map_destroy(ecamd_map *map);

/* Input j of stripe s at in_base + s*in_stripe_stride + in_off[j] (K host-side offsets), output r
 * at out_base + s*out_stripe_stride + out_off[r] (R offsets). */
int ecamd_map_apply_strided(const ecamd_map *map, const void *in_base, int64_t in_stripe_stride,
                            const int64_t *in_off, void *out_base, int64_t out_stripe_stride,
                            const int64_t *out_off, int64_t blocksize, int nstripes, void *stream);
/* ecamd_map_apply_strided for ONE stripe, plus the CRC32 of every input and output fragment over its
 * `blocksize` bytes -- zlib's crc32, or the legacy liberasurecode_crc32_alt when legacy != 0 -- written
 * to crc_out[0 .. K + R) (inputs first; device or pinned host memory), all in ONE launch of the
 * small-launch kernel.  Returns 0 when done, 1 when the shape does not fuse (nothing launched: more
 * than 4096 16-byte chunks per fragment, several passes, tables and staged fragments over the LDS, ...;
 * the caller runs ecamd_map_apply_strided and ecamd_crc32), < 0 on error.  The per-call CHKSUM_CRC32
 * encode's checksums (src/erasurecode_postprocessing.c:37-69) without two more launches. */
int ecamd_map_apply_strided_crc(const ecamd_map *map, const void *in_base, const int64_t *in_off, void *out_base,
                                const int64_t *out_off, int64_t blocksize, int legacy, uint32_t *crc_out,
                                void *stream);
/* The same for a flat-XOR map (masks as ecamd_xor_apply_strided, at most 8 outputs): one launch of the
 * small-launch XOR kernel with the checksums folded in; 0 done, 1 not fused (nothing launched), < 0 error. */
int ecamd_xor_apply_strided_crc(const uint32_t *masks, int R, int K, const void *in_base, const int64_t *in_off,
                                void *out_base, const int64_t *out_off, int64_t blocksize, int legacy,
                                uint32_t *crc_out, void *stream);
/* Launches of ecamd_map_apply_strided_crc / ecamd_xor_apply_strided_crc that fused the checksums (tests
 * pin which path ran). */
long long ecamd_small_crc_launches(void);
/* Completion flag of the calling thread's next operation (the per-call path, host/hostio.cpp): when the
 * small-launch kernel that ends it runs (gf16_small_kernel), it stores `value` to *flag -- pinned host
 * memory -- after every output and checksum store of the operation is visible system-wide, so the host
 * can poll the flag instead of synchronizing the stream.  ecamd_done_flag_taken() says whether the
 * operation took it (1), posted it to the resident small server (2: wait with ecamd_small_server_wait,
 * not on the stream, which it never touched) or not (0: other kernels; synchronize as usual) and disarms. */
void ecamd_done_flag_arm(uint32_t *flag, uint32_t value);
int ecamd_done_flag_taken(void);
/* The same, and the operation may be posted to the calling thread's resident small server (small_server_kernel,
 * DESIGN.md §6) instead of launched when it is ONE small launch with staged inputs: mode 1 any such launch,
 * 2 only one with the checksums fused (a separate checksum pass would follow on the stream); 0 as
 * ecamd_done_flag_arm.  The caller guarantees nothing it enqueued earlier on the stream is still pending. */
void ecamd_done_flag_arm_server(uint32_t *flag, uint32_t value, int mode);
/* Waits for a served operation's flag; relaunches the server if it exited before the request (its idle
 * time).  0, or < 0 after 10 s or a HIP error. */
int ecamd_small_server_wait(const uint32_t *flag, uint32_t value);
/* Operations posted to small servers, and server kernels launched (first use, after idle exits, variant
 * switches, relaunches in ecamd_small_server_wait), in this process (tests pin which path ran). */
long long ecamd_small_server_posts(void);
long long ecamd_small_server_launches(void);
/* Posts that wrote a new argument block into one of the server's two slots (the others reused a cached one). */
long long ecamd_small_server_rewrites(void);
/* Posts that matched a cached slot in everything except the map's serial: another map of the same shape whose
 * table image sits at a recycled device address.  They rewrite the slot like any other new request (a map is
 * identified by the serial it got at creation, never by its tables' address). */
long long ecamd_small_server_stale_hits(void);
/* Stops the calling thread's server and waits for its kernel to exit (after a failed
 * ecamd_small_server_wait): nothing it was handed is in use afterwards, its cached argument blocks are
 * forgotten and its counters zeroed; the next post launches it again.  0 (also without a server), or < 0 when
 * its stream cannot be synchronized -- then memory a pending request points to must not be reused. */
int ecamd_small_server_quiesce(void);

/* Pointer tables in device memory: input j of stripe s is d_in_ptrs[s*in_row + in_col[j]],
 * output r is d_out_ptrs[s*out_row + out_col[r]] (in_col / out_col are host arrays). */
int ecamd_map_apply_ptrs(const ecamd_map *map, const void *const *d_in_ptrs, int in_row,
                         const int *in_col, void *const *d_out_ptrs, int out_row,
                         const int *out_col, int64_t blocksize, int nstripes, void *stream);

/* ---- GF(2) (flat XOR) fragment maps: outputs[r] = XOR of inputs j with bit j of mask[r] ---- */
int ecamd_xor_apply_strided(const uint32_t *masks, int R, int K, const void *in_base,
                            int64_t in_stripe_stride, const int64_t *in_off, void *out_base,
                            int64_t out_stripe_stride, const int64_t *out_off, int64_t blocksize,
                            int nstripes, void *stream);
int ecamd_xor_apply_ptrs(const uint32_t *masks, int R, int K, const void *const *d_in_ptrs,
                         int in_row, const int *in_col, void *const *d_out_ptrs, int out_row,
                         const int *out_col, int64_t blocksize, int nstripes, void *stream);

/* ---- liberasurecode_rs_vand on strided batches (maps cached per (k, m, pattern)) ---- */
/* Encode: parity fragments k..k+m-1 from data 0..k-1. */
int ecamd_rs_encode(int k, int m, void *base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, void *stream);
/* Decode: rebuild every fragment in the -1 terminated `missing` list in place (data, and parity
 * if rebuild_parity) from the first k available, as liberasurecode_rs_vand_decode does. */
int ecamd_rs_decode(int k, int m, const int *missing, int rebuild_parity, void *base,
                    int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                    void *stream);
/* Heterogeneous batch decode: stripe s has its own -1 terminated erasure list at
 * missing + s*missing_stride (at most missing_stride entries).  Stripes are grouped by erasure
 * set; each group is one launch over a device stripe list (a pointer table when k > 20 or a
 * stripe spans 2 GiB), so a batch of stripes that lost different fragments costs one launch per
 * distinct pattern, not per stripe. */
int ecamd_rs_decode_multi(int k, int m, const int *missing, int missing_stride,
                          int rebuild_parity, void *base, int64_t stripe_stride,
                          int64_t frag_stride, int64_t blocksize, int nstripes, void *stream);
/* Fragment placement across GPUs: fragment f of every stripe (frag_len bytes at
 * d_src + s*stripe_stride + f*frag_stride on the current device) goes to d_dst[f] +
 * s*dst_stride[f] on device dst_dev[f]: one strided DMA per fragment, over xGMI when dst_dev[f]
 * is a peer (peer access is enabled on first use).  Copies to different peers run at once on
 * per-destination copy lanes forked from and joined back into `stream`; every destination is
 * checked before anything is queued.  Asynchronous on `stream`. */
int ecamd_scatter_fragments(const void *d_src, int64_t stripe_stride, int64_t frag_stride,
                            int64_t frag_len, int nfrags, int nstripes, const int *dst_dev,
                            void *const *d_dst, const int64_t *dst_stride, void *stream);
/* The rs_* calls above cache one prepared map (device coefficient tables) per (device, k, m,
 * erasure pattern, destination), least recently used first out once the tables exceed `limit`
 * bytes: entries and bytes currently held. */
int ecamd_map_cache_stats(int64_t *entries, int64_t *bytes, int64_t *limit);
/* Reconstruct one destination, as liberasurecode_rs_vand_reconstruct does. */
int ecamd_rs_reconstruct(int k, int m, const int *missing, int dest, void *base,
                         int64_t stripe_stride, int64_t frag_stride, int64_t blocksize,
                         int nstripes, void *stream);

/* ---- stripe consistency check: do the fragments of a stripe still agree with each other? ----
 * Consistency of S stripes in place.  The first k fragments not in the -1 terminated `missing`
 * (NULL or empty: none) are the inputs, as in ecamd_rs_decode; every OTHER available fragment f is
 * "checked": d_status[s] gets bit f when any of its `blocksize` bytes differs from the value the
 * inputs imply.  Bits of inputs and of missing fragments are never set.  d_status (nstripes
 * uint32, device memory) is overwritten.  *checked (host, may be NULL) receives the mask of checked
 * fragments.  Nothing else is written; asynchronous on stream.
 * ECAMD_EINVAL: more than m missing, k+m > 32 (d_status is then untouched).  With exactly m missing
 * nothing is checked: status all zero, *checked 0.
 * Layout rules as for the other strided calls (16-byte aligned base and strides, any blocksize >= 1);
 * exactly `blocksize` bytes of each fragment are compared, bytes between blocksize and frag_stride
 * never influence the status.  Framed fragments (ecamd_frame_encode) are checked by passing
 * d_frags + 80 as `base`: the payload follows the 80-byte header, and 80 is a multiple of 16.
 * Reading the status: a single parity bit -- that parity fragment is bad; all checked bits -- an input
 * (or several fragments) is bad; re-check with a suspect listed as missing to isolate it, or let ecamd_rs_locate (below) name it in one pass.
 * Whole bitsliced tiles run one read-only fused kernel (the codec's XOR network over the K inputs and
 * the checked fragments; a consistent stripe causes no write); tails, small fragments, shapes the
 * bitsliced form declines, maps still compiling (knob "bitslice" 1) and knob "bitslice" 0 compute the
 * expected fragments into library-owned scratch of at most 64 MiB per (device, stream), stripe chunk
 * by stripe chunk, and compare (DESIGN.md "Consistency check"). */
int ecamd_rs_check(int k, int m, const int *missing, const void *base, int64_t stripe_stride,
                   int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                   uint32_t *checked, void *stream);
/* flat_xor_hd, all k+m fragments present: bit k+p when stored parity p differs from the XOR its
 * parity bitmap names (xor_code_encode).  Same layout rules; ECAMD_EINVAL (d_status untouched) when
 * (k, m, hd) is not a code init_xor_hd_code accepts.
 * Whole tiles run one read-only fused kernel (xor_check_kernel): 128-bit loads of all k+m fragments,
 * the m syndromes S_p = stored parity p ^ XOR of the data in bitmap p kept in registers, one status
 * atomic per wave that sees a non-zero syndrome and no write at all for a consistent tile.  Tiles are
 * 1 KiB (one-wave workgroups, the default: knob "xor_check_threads" 0 or 64) or 4 KiB (256-lane
 * workgroups: knob 256).  Long batches split into launches of "xor_tiles_per_slot" tiles per slot
 * with "xor_wgs" (0: 3) slots per CU; the knob counts 4 KiB tiles, so the one-wave form takes four
 * times as many of its 1 KiB tiles per slot -- the same bytes per launch.  The rest of each fragment,
 * fragments shorter than a tile, stripes whose last fragment ends 2 GiB or more past the first, and
 * everything with knob "xor_check_fused" 0 (default 1) take the scratch path described above.  Knob
 * "bitslice" does not affect flat XOR.  The results are the same on every path. */
int ecamd_xor_check(int k, int m, int hd, const void *base, int64_t stripe_stride,
                    int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                    void *stream);
/* Fused check launches enqueued by this process (tests pin which path ran): the bitsliced check form
 * (rs_vand), and xor_check_kernel's check form (flat XOR), each counted on its own. */
long long ecamd_check_fused_launches(void);
long long ecamd_xor_check_fused_launches(void);
/* Build time, as ecamd_bitslice_prebuild: the fused check kernel(s) of (k, m, missing).  Returns the
 * number of code objects present (0: the check takes no bitsliced form), < 0 on error. */
int ecamd_check_prebuild(int k, int m, const int *missing, const char *arch, const char *dir);

/* ---- locate and scrub: WHICH fragment of an inconsistent stripe is bad, and its repair ----
 * ecamd_rs_locate runs the check above (same inputs / checked fragments, same d_status words, same
 * *checked) and, in the same pass, fills d_suspects (nstripes uint32, device memory): 0 where
 * d_status[s] is 0; otherwise the mask of participating fragments (inputs and checked) that ALONE
 * explain every disagreement of stripe s.  Exactly one bit: that fragment is located -- list it as
 * missing and decode.  Zero: more than one fragment is bad.  Bits of missing fragments and bits
 * >= k+m are never set.  Only these two arrays are written; asynchronous on stream.
 * How much can be told depends on R, the number of checked fragments (m minus the missing ones):
 *   R >= 3  one bad fragment is located; any two bad fragments leave no suspect (with R >= 4,
 *           ecamd_rs_locate_pairs below names the two).
 *   R == 2  one bad fragment is located; two bad fragments can in principle be attributed to a
 *           third (a single suspect that is wrong) -- the code corrects one error with two checks
 *           and cannot also detect a second.
 *   R == 1  nothing can be told apart: every participating fragment is a suspect on a dirty stripe.
 *   R == 0  both words are 0.
 * The rule, per 16-bit word with syndromes S_r = stored_r ^ (what the inputs imply): input j explains
 * the word iff S_r == (A[r][j] / A[0][j]) * S_0 for every r >= 1, checked fragment c iff S_r == 0 for
 * every r != c; a stripe's suspects are the AND over its dirty words.
 * ECAMD_EINVAL as for the check, and also for an ODD blocksize (the trailing byte's product is cut
 * to 8 bits, so proportionality cannot be tested; the frontend and ecamd_frame_geometry only produce
 * even sizes).  On every ECAMD_EINVAL both arrays are untouched.
 * Whole bitsliced tiles with 2..8 checked fragments run the locate form of the fused check kernel (a
 * clean tile costs what the check costs; a wave that sees a non-zero syndrome tests every candidate
 * in registers and issues one atomic AND); everything else goes through the check's scratch path
 * with a compare kernel that applies the same rule (DESIGN.md "Locate and scrub"). */
int ecamd_rs_locate(int k, int m, const int *missing, const void *base, int64_t stripe_stride,
                    int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                    uint32_t *d_suspects, uint32_t *checked, void *stream);
/* ---- two bad fragments per stripe (rs_vand only) ----
 * ecamd_rs_locate_pairs does everything ecamd_rs_locate does -- d_status, d_suspects and *checked are
 * byte-identical to what that call writes for the same data -- and, in the same asynchronous call
 * (no host wait), fills d_pairs (nstripes uint32, device memory).  d_pairs[s] is 0 unless
 * d_status[s] != 0, d_suspects[s] == 0 and R >= 4; for such a stripe it has exactly the two bits
 * {a, b} when {a, b} is the ONE pair of participating fragments (inputs and checked) that explains
 * every dirty word, else 0.  A pair explains a word when the word's syndrome vector (S_0..S_{R-1})
 * lies in the span of columns a and b of the R x (K+R) syndrome matrix [A | I] (A: the check map of
 * ecamd_rs_check_map, ecamd_host.h).  Four checks determine two unknown error positions:
 *   R >= 5  two bad fragments are located; any three bad fragments leave no pair.
 *   R == 4  two bad fragments are located; three bad fragments can in principle be attributed to a
 *           pair (a pair that is wrong) -- the code corrects two errors with four checks and cannot
 *           also detect a third.  This is what R == 2 is to ecamd_rs_locate.
 *   R <  4  d_pairs is all zero.
 * The pair is unique because any four columns of [A | I] are linearly independent; the plan
 * (ecamd_rs_locate_pairs_map, ecamd_host.h) verifies that once per (k, m, missing) and keeps the
 * result with the cached check map.  For a map where it does not hold, d_pairs is all zero: uniqueness
 * would not be a theorem.  (It holds for every rs_vand map that was tried.)
 * ECAMD_EINVAL as for ecamd_rs_locate, an odd blocksize included, and also for a null d_pairs; all
 * three arrays are then untouched.  Exactly nstripes words of each array are written.
 * The pair stage runs after the locate, on its results and on the same stream: d_pairs set to 0 (by
 * the locate's own last kernel), locate_pairs_kernel, a finalize.  Its workgroups load d_status[s] and d_suspects[s] and go on only
 * for a dirty stripe without a suspect, whose K inputs and R checked fragments they read again -- no
 * scratch -- taking the syndromes by shift and xor: a clean batch costs two loads per workgroup, a
 * batch of damaged pairs several times its locate (DESIGN.md "Two bad fragments").  Knob
 * "pairs_grid" > 0 caps both grid dimensions (tests); like every knob it does not change results. */
int ecamd_rs_locate_pairs(int k, int m, const int *missing, const void *base, int64_t stripe_stride,
                          int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                          uint32_t *d_suspects, uint32_t *d_pairs, uint32_t *checked, void *stream);
/* Scrub FULL stripes in place, two bad fragments included (m >= 4, else ECAMD_EINVAL with the arrays
 * untouched): ecamd_rs_locate_pairs, a wait for `stream`, then ONE ecamd_rs_decode_multi
 * (missing_stride 3, rebuild_parity 1) with the list {f} for a stripe with exactly one suspect f,
 * {a, b} for a stripe with a pair, and the empty list for every other.  The counts (host, may be
 * NULL) are final on return: consistent stripes, stripes repaired from one suspect, stripes repaired
 * from a pair, and dirty stripes with neither, which are not written.  The repair launches are
 * enqueued on stream; the three arrays keep what the locate found.  At m == 4 a pair repair uses up
 * every check: nothing is left to notice a third bad fragment (see R == 4 above), as ecamd_rs_scrub
 * at m == 2. */
int ecamd_rs_scrub_pairs(int k, int m, void *base, int64_t stripe_stride, int64_t frag_stride,
                         int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                         uint32_t *d_pairs, int *n_clean, int *n_repaired, int *n_repaired_pairs,
                         int *n_unlocated, void *stream);
/* Launches of locate_pairs_kernel enqueued by this process (tests pin that it ran, or did not). */
long long ecamd_locate_pairs_launches(void);

/* flat_xor_hd, all fragments present: the same rule over the 0/1 parity bitmaps -- data fragment j
 * explains a word iff every parity that contains j has the same syndrome as the first one that does
 * and every other parity has none; parity p iff only its own syndrome is non-zero.  A flat XOR code
 * is not MDS: two bad fragments can leave a (wrong) single suspect.
 * As a lookup (ecamd_xor_check_plan, ecamd_host.h): fragment f explains a word iff all its non-zero
 * syndromes are equal and the set of rows with a non-zero syndrome is sig[f].  Whole tiles run the
 * locate form of the fused kernel of ecamd_xor_check (same tiles, same knobs): a clean tile costs what
 * the check costs; a wave that sees a non-zero syndrome applies the rule in registers and issues one
 * atomic OR and one atomic AND. */
int ecamd_xor_locate(int k, int m, int hd, const void *base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                     void *stream);
/* Scrub FULL stripes (nothing missing; m >= 2, else ECAMD_EINVAL) in place: ecamd_rs_locate, a wait
 * for `stream`, then ecamd_rs_decode_multi (rebuild_parity 1) with the list {f} for every stripe
 * that has exactly one suspect f and the empty list for every other.  The counts (host, may be NULL)
 * are final on return: consistent stripes, stripes being repaired, and dirty stripes with zero or
 * several suspects, which are not written.  The repair launches are enqueued on stream; d_status and
 * d_suspects keep what locate found.  With m == 2 a stripe with two bad fragments may be "repaired"
 * towards a third (see R == 2 above). */
int ecamd_rs_scrub(int k, int m, void *base, int64_t stripe_stride, int64_t frag_stride,
                   int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                   int *n_clean, int *n_repaired, int *n_unlocated, void *stream);
/* The same for flat_xor_hd: ecamd_xor_locate, a wait for `stream`, then ecamd_xor_decode_multi
 * (decode_parity 1) with the list {f} for every stripe that has exactly one suspect f and the empty
 * list for every other.  Counts and arrays as ecamd_rs_scrub.  ECAMD_EINVAL, both arrays untouched,
 * for a code init_xor_hd_code rejects and for an odd blocksize.
 * A flat XOR code is not MDS: two bad fragments f1 and f2 with the same error in the same word read
 * as the single fragment f3 whenever sig[f1] ^ sig[f2] == sig[f3] (ecamd_xor_check_plan; (3,3,3) has
 * such triples).  Scrub then "repairs" towards f3 and leaves a consistent stripe with both errors
 * in it, as ecamd_rs_scrub does at m == 2. */
int ecamd_xor_scrub(int k, int m, int hd, void *base, int64_t stripe_stride, int64_t frag_stride,
                    int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                    int *n_clean, int *n_repaired, int *n_unlocated, void *stream);

/* ---- correct on the device: locate, then repair the located words, all on `stream` ----
 * ecamd_rs_correct runs ecamd_rs_locate (d_pairs NULL) or ecamd_rs_locate_pairs (d_pairs given) --
 * d_status, d_suspects, d_pairs and *checked are byte-identical to what those calls write for the same
 * data; they keep what the locate found and are NOT re-evaluated after the correction -- and then, with
 * one more launch on the same stream, corrects in place every stripe with exactly one suspect and,
 * with d_pairs, every stripe without a suspect whose pair word has exactly two bits.  Every other
 * stripe is not written.  There is no host wait anywhere in the call: no stream synchronise, no copy
 * to the host, no launch whose shape depends on what the locate found.  (The first call for a (k, m,
 * missing) uploads its small tables before it enqueues anything, like every cached map.)
 * The rule: a located error is an error value.  With S_r = stored_r ^ (what the inputs imply for
 * checked row r), one bad checked fragment c has e = S_c, one bad input j has e = S_0 / A[0][j], and
 * a pair {a, b} has (e_a, e_b) = inv(M) (S_p, S_q) with M the 2 x 2 minor of the pair plan
 * (ecamd_rs_correct_map, ecamd_host.h).  correct_kernel reads the K inputs and the one or two pivot
 * rows of a stripe with work, XORs each non-zero error value into the stored 4-byte unit and writes
 * nothing else: the result is the fragment ecamd_rs_decode_multi would write, byte for byte, at the
 * cost of K+1 or K+2 fragment reads and stores to the damaged words only.  A clean stripe costs three
 * word loads per workgroup that visits it.
 * `missing` (-1 terminated, may be NULL) makes it work on degraded stripes: the slots of missing
 * fragments are never read or written, and the remaining bad fragment is located and corrected as far
 * as the R = m - |missing| checks allow -- the R == 2 and R == 4 caveats of ecamd_rs_locate and
 * ecamd_rs_locate_pairs apply word for word (a stripe with one bad fragment more than can be detected
 * may be "corrected" towards a wrong fragment or pair and ends consistent).  A non-NULL d_pairs with
 * R < 4 is not an error: d_pairs is zeroed and singles are still corrected.
 * d_counts (4 uint32, device memory, may be NULL) is overwritten with: stripes clean, corrected from
 * one suspect, corrected from a pair, dirty and not corrected.
 * ECAMD_EINVAL for everything the locate rejects (bad layout, null d_status / d_suspects, more than m
 * missing, k+m > 32, odd blocksize); the data, the arrays and d_counts are then untouched.  An empty
 * batch returns 0 and writes nothing.
 * Framed fragments (ecamd_frame_encode) are corrected by passing d_frags + 80 as `base`; a repaired
 * payload again matches the CRC32 its header holds, since the header is not touched and the payload
 * is the encode's again.
 * Knob "pairs_grid" > 0 caps both grid dimensions of correct_kernel as well (tests); results do not change. */
int ecamd_rs_correct(int k, int m, const int *missing, void *base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                     uint32_t *d_pairs /* may be NULL */, uint32_t *d_counts /* may be NULL */,
                     uint32_t *checked, void *stream);
/* The same over ecamd_xor_locate (flat_xor_hd, all fragments present): the kernel runs over the 0/1
 * parity bitmaps, fragment f's pivot row is the lowest bit of sig[f] (ecamd_xor_check_plan) and every
 * scale is 1.  ECAMD_EINVAL, everything untouched, for a code init_xor_hd_code rejects and for an odd
 * blocksize.  The caveat of ecamd_xor_scrub applies: two bad fragments that read as a third are
 * "corrected" towards it and leave a consistent stripe -- the same bytes ecamd_xor_scrub leaves. */
int ecamd_xor_correct(int k, int m, int hd, void *base, int64_t stripe_stride, int64_t frag_stride,
                      int64_t blocksize, int nstripes, uint32_t *d_status, uint32_t *d_suspects,
                      uint32_t *d_counts /* may be NULL */, void *stream);

/* ---- flat_xor_hd with fragments missing: check, locate and correct what is left ----
 * `missing` (-1 terminated, may be NULL) lists the lost fragments of every stripe of the batch; their
 * slots are never read and never written, on any path.  The checks are the rows of
 * ecamd_xor_check_plan_degraded (ecamd_host.h, where the reduction rule is stated): rows[p], the
 * surviving row that parity p owns, and sig[f], the surviving rows that contain fragment f.  Per
 * 16-bit word, S_p is the XOR of the stored fragments in rows[p].
 *   check    d_status[s] gets bit k+p when S_p is non-zero anywhere in stripe s, surviving rows only.
 *   locate   d_suspects[s] is 0 on a clean stripe, else the mask of covered fragments f such that in
 *            every dirty word the set of non-zero rows is exactly sig[f] and those syndromes are equal.
 *            Fragments that share a signature cannot be told apart and come back together (several
 *            bits).  Missing fragments and available ones that no surviving row contains (sig[f] == 0)
 *            never appear.  With one surviving row every fragment of that row is a suspect of a dirty
 *            stripe; with none both words are 0.
 *   correct  the locate, then on the same stream and with no host wait: a stripe with exactly one
 *            suspect f gets S_q XORed into fragment f, q the lowest bit of sig[f]; only the non-zero
 *            4-byte units are written, as ecamd_xor_correct does.  Every other stripe is not written.
 *            d_counts as ecamd_xor_correct; the arrays keep what the locate found.
 * *covered (host, may be NULL) is set to the mask of fragments with sig[f] != 0 -- the only ones whose
 * damage these calls can see -- for an empty batch too.
 * What can be told: with at most hd - 2 fragments missing every available fragment is covered; at
 * hd 4 with one missing the signatures are still distinct, so one bad fragment is located and
 * corrected; at hd 4 with two missing and at hd 3 with one missing some fragments share a signature and
 * come back as a set, which correct leaves alone.  With nothing missing the words are those of
 * ecamd_xor_check / ecamd_xor_locate / ecamd_xor_correct.
 * Losing fragments lowers the distance: a stripe with one bad fragment more than the remaining checks
 * can detect may read as a wrong single suspect and be "corrected" towards it, ending consistent -- the
 * caveat of R == 2 at ecamd_rs_locate and of (3,3,3) at ecamd_xor_scrub.
 * Whole tiles run the degraded form of the fused kernel (xor_check_kernel over slots: only the fragments of
 * the surviving rows are loaded, so a (10,6,4) stripe with one lost issues 15 loads per lane, not 16);
 * its launches count in ecamd_xor_check_fused_launches / ecamd_xor_locate_fused_launches.  Tails,
 * fragments shorter than a tile, knob xor_check_fused 0 and stripes the 32-bit offsets cannot span go
 * through the generic stage; the words are the same on every path.
 * ECAMD_EINVAL, with the data, the arrays, d_counts and *covered untouched, for everything the plan
 * rejects (a code init_xor_hd_code rejects, an index >= k+m, a repeated index, more than m entries),
 * for the layout errors of ecamd_xor_check and, on locate and correct, for an odd blocksize. */
int ecamd_xor_check_degraded(int k, int m, int hd, const int *missing, const void *base, int64_t stripe_stride,
                             int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                             uint32_t *covered, void *stream);
int ecamd_xor_locate_degraded(int k, int m, int hd, const int *missing, const void *base, int64_t stripe_stride,
                              int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                              uint32_t *d_suspects, uint32_t *covered, void *stream);
int ecamd_xor_correct_degraded(int k, int m, int hd, const int *missing, void *base, int64_t stripe_stride,
                               int64_t frag_stride, int64_t blocksize, int nstripes, uint32_t *d_status,
                               uint32_t *d_suspects, uint32_t *d_counts /* may be NULL */, uint32_t *covered,
                               void *stream);
/* Launches of correct_kernel enqueued by this process (one per call with a non-empty batch and at
 * least one checked fragment). */
long long ecamd_correct_launches(void);
/* Fused locate launches enqueued by this process (tests pin which path ran): the bitsliced locate
 * form (rs_vand), and xor_check_kernel's locate form (flat XOR), each counted on its own. */
long long ecamd_locate_fused_launches(void);
long long ecamd_xor_locate_fused_launches(void);
/* Build time, as ecamd_check_prebuild: the fused locate kernel of (k, m, missing).  Returns the number
 * of code objects present (0: no fused form -- fewer than 2 or more than 8 checked fragments, a shape
 * the bitsliced form declines, or a kernel that would need scratch), < 0 on error. */
int ecamd_locate_prebuild(int k, int m, const int *missing, const char *arch, const char *dir);

/* ---- decode from device masks: every stripe lost its own set of fragments, named on the device ----
 * The erasure counterpart of ecamd_rs_correct (rs_vand only).  d_lost (nstripes uint32, DEVICE memory)
 * holds one mask per stripe: bit f set when fragment f of stripe s is lost.  The word is read on the
 * device, in stream order; it may have been written by earlier work on the same stream
 * (ecamd_frame_status_masks below, a copy, a kernel of the caller's).  Per stripe, with L = d_lost[s]:
 *   L == 0                          nothing of the stripe is read or written; d_result[s] = 0.
 *   a bit >= k+m, or more than m    not recoverable: nothing of the stripe is written;
 *   bits                            d_result[s] = 0x80000000 | popcount(L).
 *   otherwise                       the inputs are the first k fragments not in L (ecamd_rs_decode's rule);
 *                                   the outputs are the lost data fragments, ascending, then -- with
 *                                   rebuild_parity -- the lost parity fragments, ascending.  The bytes
 *                                   written are exactly those ecamd_rs_decode_multi writes for the
 *                                   ascending list of L; d_result[s] = the number of fragments written.
 * Lost slots that are not rebuilt (lost parity without rebuild_parity, every slot of an unrecoverable
 * stripe) are never written, surviving fragments are never written, bytes between blocksize and
 * frag_stride are never written, and lost slots are never read: they may hold anything.
 * d_result (nstripes uint32, device memory, may be NULL).  d_counts (3 uint32, device memory, may be
 * NULL) is overwritten with the number of stripes left alone (result 0), rebuilt, and unrecoverable.
 * There is no host dependence inside the call: no stream synchronise, no copy to the host, no launch
 * whose shape depends on the masks, no map-cache entry, no bitsliced launch and no compile -- RS(20,8)
 * has 4.4 million patterns and each costs what any other costs.  The launches are fixed: a plan
 * kernel (one wave per stripe works out the stripe's coefficients from the code's generator by
 * Gauss-Jordan in shift-and-xor arithmetic: ecamd_masks_plan.hpp, the same text the host test checks
 * against ecamd_rs_decode_map), the data kernel (per stripe: nibble tables built in LDS from the
 * stripe's coefficients, 128-bit loads of the k inputs, 128-bit stores of the outputs; a stripe with
 * nothing to write costs one word load per workgroup that visits it; tiles of 4096 bytes, the last
 * partial 16-byte chunk byte-exact), and with d_counts a one-workgroup count.  The per-stripe plans
 * live in library-owned scratch per (device, stream), 560 bytes per stripe, which grows only when a
 * larger batch arrives (growing waits for the stream once, as the check's scratch does).  The first
 * call for a (k, m) on a device uploads that code's generator, once.
 * ECAMD_EINVAL, with the data and the arrays untouched, for a null d_lost or base, the layout errors
 * of the other strided calls (16-byte aligned base and strides, frag_stride >= blocksize >= 1),
 * k+m > 32, m > 8, and an ODD blocksize (as ecamd_rs_locate and ecamd_rs_correct; the frontend and
 * ecamd_frame_geometry only produce even sizes).  nstripes == 0 returns 0 and writes nothing.
 * Knob "pairs_grid" > 0 caps both grid dimensions of the data kernel as it does for correct_kernel
 * (tests); like every knob it does not change results.
 * When to prefer ecamd_rs_decode_multi: DESIGN.md "Decode from device masks", INTEGRATION.md. */
int ecamd_rs_decode_masks(int k, int m, const uint32_t *d_lost, int rebuild_parity, void *base,
                          int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                          uint32_t *d_result /* may be NULL */, uint32_t *d_counts /* 3 words, may be NULL */,
                          void *stream);
/* Launches of decode_masks_kernel (the data kernel) enqueued by this process: one per call with a
 * non-empty batch. */
long long ecamd_decode_masks_launches(void);

/* ---- flat_xor_hd on strided batches: the reference's xor_code_encode,
 * xor_hd_decode (decode_parity as its argument) and xor_reconstruct_one
 * (src/builtin/xor_codes/xor_code.c:180-314, xor_hd_code.c:574-662) replayed exactly per erasure
 * list, missing slots read as zero (the frontend's zero-filled buffers); (k, m, hd) one of the
 * codes init_xor_hd_code accepts.  encode overwrites the parity slots (the reference accumulates
 * into the zeroed parity the frontend allocates: the same bytes).  decode_multi groups stripes by
 * identical erasure lists and runs one stripe-list launch per group.  ECAMD_EINVAL for patterns
 * the code cannot recover. */
int ecamd_xor_encode(int k, int m, int hd, void *base, int64_t stripe_stride, int64_t frag_stride,
                     int64_t blocksize, int nstripes, void *stream);
int ecamd_xor_decode(int k, int m, int hd, const int *missing, int decode_parity, void *base,
                     int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                     void *stream);
int ecamd_xor_reconstruct(int k, int m, int hd, const int *missing, int dest, void *base,
                          int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                          void *stream);
int ecamd_xor_decode_multi(int k, int m, int hd, const int *missing, int missing_stride,
                           int decode_parity, void *base, int64_t stripe_stride, int64_t frag_stride,
                           int64_t blocksize, int nstripes, void *stream);
/* Launches of xor_stream_kernel enqueued by this process, with or without the copy-through (tests pin
 * which kernel ran: passes of at most "small_chunks" chunks take xor_small_kernel and do not count). */
long long ecamd_xor_stream_launches(void);

/* ---- flat_xor_hd decode from device masks: ecamd_rs_decode_masks' counterpart for the flat XOR codes ----
 * d_lost (nstripes uint32, DEVICE memory) holds one mask per stripe, bit f set when fragment f of stripe s
 * is lost; the word is read on the device, in stream order, exactly as ecamd_rs_decode_masks reads it.
 * Per stripe, with L = d_lost[s]:
 *   L == 0                          nothing of the stripe is read or written; d_result[s] = 0.
 *   a bit >= k+m, or hd or more     not recoverable -- the reference refuses every list of hd or more
 *   bits                            fragments (get_failure_pattern: GE_HD), whatever the code could solve:
 *                                   nothing of the stripe is written; d_result[s] = 0x80000000 | popcount(L).
 *   otherwise                       the outputs are the lost data fragments, ascending, then -- with
 *                                   decode_parity -- the lost parity fragments, ascending.  Each is the XOR
 *                                   of the surviving fragments that ecamd_xor_plan(op 1, the ascending list
 *                                   of L, decode_parity 1) names for it, the bits of lost fragments dropped:
 *                                   the bytes xor_hd_decode leaves when the lost slots were ZERO-FILLED,
 *                                   which is how the frontend calls it and what ecamd_xor_decode_multi
 *                                   documents.  d_result[s] = the number of fragments written (0 when only
 *                                   parity is lost and decode_parity is 0).
 * Lost slots are never read: they may hold anything.  Never written: surviving fragments, lost parity
 * without decode_parity, every slot of an unrecoverable stripe, the bytes between blocksize and frag_stride.
 * d_result (nstripes uint32, device memory, may be NULL).  d_counts (3 uint32, device memory, may be NULL)
 * is overwritten with the number of stripes left alone (result 0), rebuilt, and unrecoverable.
 * Any blocksize >= 1, odd ones included: XOR has no 16-bit word.
 * There is no host dependence inside the call: no stream synchronise, no copy to the host, no launch whose
 * shape depends on the masks, no map-cache entry, no xor_stream_kernel launch and no compile.  A code has
 * at most 2952 recoverable patterns ((20,6,4): the masks of fewer than hd bits), so its whole decode is one
 * table of 16-byte entries (ecamd_xor_decode_masks_plan, ecamd_host.h) indexed by the rank of the mask, and
 * nothing is solved on the device.  The launches are fixed: the data kernel (per stripe: the mask's rank and
 * entry as scalars, 128-bit loads of the union of the entry's sources -- each fragment once, however many
 * outputs it feeds --, 128-bit stores of the outputs; a stripe with nothing to write costs one word load
 * per workgroup that visits it; tiles of 4096 bytes, the last partial 16-byte chunk byte-exact; no LDS;
 * its first tile column writes d_result), and with d_counts a one-workgroup count.  The first call for a
 * (k, m, hd) on a device uploads that code's table, once; there is no per-stream scratch.
 * ECAMD_EINVAL, with the data and the arrays untouched, for a code init_xor_hd_code rejects, a null d_lost
 * or base, the layout errors of the other strided calls (16-byte aligned base and strides, frag_stride >=
 * blocksize >= 1) and nstripes < 0.  nstripes == 0 returns 0 and writes nothing.
 * Knob "pairs_grid" > 0 caps both grid dimensions of the data kernel as it does for decode_masks_kernel.
 * When to prefer ecamd_xor_decode_multi: DESIGN.md "Decode from device masks", INTEGRATION.md. */
int ecamd_xor_decode_masks(int k, int m, int hd, const uint32_t *d_lost, int decode_parity, void *base,
                           int64_t stripe_stride, int64_t frag_stride, int64_t blocksize, int nstripes,
                           uint32_t *d_result /* may be NULL */, uint32_t *d_counts /* 3 words, may be NULL */,
                           void *stream);
/* Launches of xor_decode_masks_kernel (the data kernel) enqueued by this process: one per call with a
 * non-empty batch. */
long long ecamd_xor_decode_masks_launches(void);

/* ---- synchronous host-buffer execution (used by the per-call drop-in ABIs) ----
 * Pooled pinned staging + two streams, chunked so host copies overlap PCIe and the kernel.
 * Calls are spread round-robin over the visible devices (or ECAMD_PERCALL_DEVICES, see
 * ecamd_percall_device_plan in ecamd_host.h), each with its own staging pool; the caller's
 * current device is restored on return.
 * ecamd_host_map_apply: out[r] = sum_j coeff[r*K+j] * in[j] over GF(2^16).
 * ecamd_host_xor_apply: out[r] = XOR of bufs[b] for bits b of sources[r] (nbuf <= 64, at most 32
 * distinct buffers referenced); outputs may alias bufs, every output sees the original inputs. */
int ecamd_host_map_apply(const int *coeff, int R, int K, const void *const *in, void *const *out,
                         int64_t blocksize);
int ecamd_host_xor_apply(const uint64_t *sources, int R, int nbuf, const void *const *bufs,
                         void *const *out, int64_t blocksize);

/* Per-call checksum handoff (used by liberasurecode.so.1 around encode / reconstruct): while armed
 * on the calling thread, the two calls above also compute the CRC32 (zlib, or the legacy
 * liberasurecode_crc32_alt when legacy != 0) of every input and output fragment on the GPU while
 * the bytes are resident; lookup returns 0 and the CRC for a (pointer, length) seen since arm. */
int ecamd_percall_crc_arm(int legacy);
int ecamd_percall_crc_lookup(const void *ptr, int64_t len, uint32_t *crc);
void ecamd_percall_crc_disarm(void);
/* Per-call execution status: the first failure (staging allocation, copy, launch) of the two
 * synchronous calls above on the calling thread since ecamd_percall_reset(), 0 if none.  The
 * reference codec cannot fail mid-call and its shims discard the codec's return code
 * (src/backends/rs_vand/liberasurecode_rs_vand.c:86-90); liberasurecode.so.1 reads this around
 * each codec call and fails the call (-EIO) instead of stamping unwritten fragments. */
void ecamd_percall_reset(void);
int ecamd_percall_status(void);
/* Per-call input tees (used by liberasurecode.so.1 around encode and decode): while armed on the
 * calling thread, the synchronous calls above pack input `key[i]` -- when it is one of their input
 * pointers -- by reading bytes [0, len[i]) from src[i] (the rest from key[i]) and writing them to
 * dst2[i] as well, so a host copy the frontend would make anyway (object -> data payloads on
 * encode, surviving data payloads -> decoded object on decode) rides on the staging pack instead of
 * reading its source a second time.  disarm writes into done[i] (may be NULL) how many of the
 * len[i] bytes were delivered to dst2[i] -- all of them or none -- and forgets the tees; the
 * caller copies whatever was not delivered.  n <= 64.  0, or ECAMD_EINVAL. */
int ecamd_percall_tee_arm(int n, const void *const *key, const void *const *src, void *const *dst2,
                          const int64_t *len);
void ecamd_percall_tee_disarm(int64_t *done);
/* Fault injection for tests: site "staging" makes the next `count` staging acquisitions of the
 * synchronous host-buffer calls fail with ECAMD_ENOMEM (0 disarms); site "server_wait" makes the next
 * `count` waits for a request posted to the resident small server report ECAMD_EHIP right after the post,
 * without waiting, as a timed-out ecamd_small_server_wait would (the request itself is not disturbed). */
int ecamd_fault_inject(const char *site, int count);

/* ---- on-device framing: the wire format of liberasurecode_encode, in HBM ----
 * backend 6 = liberasurecode_rs_vand, 3 = flat_xor_hd (hd used only there); checksum is the
 * ec_checksum_type_t of the instance (1 none, 2 CRC32; anything else is stored, not computed, as the
 * reference does).  Object s lives at d_obj + s*obj_stride (obj_size bytes, all stripes the same
 * size); fragment f of stripe s at d_frags + s*stripe_stride + f*frag_stride: the 80-byte
 * fragment_header_t followed by the payload.  frag_stride >= 80 + blocksize rounded up to 16, all
 * fragment addresses 16-byte aligned.  For full HBM rate put every payload on a 128-byte line:
 * frag_stride a multiple of 128 and d_frags = (128-aligned buffer) + 48, so each header sits at
 * offset 48 of its slot (packed fragments run 13-19% slower; DESIGN.md §4 "Payload alignment").
 * LIBERASURECODE_WRITE_LEGACY_CRC selects the legacy checksum exactly as in the reference.
 * Asynchronous on `stream`. */

/* blocksize = get_aligned_data_size(obj_size) / k; fragment_len = 80 + blocksize. */
int ecamd_frame_geometry(int backend, int k, int m, int hd, uint64_t obj_size, int64_t *blocksize,
                         int64_t *fragment_len);
/* liberasurecode_encode (src/erasurecode.c:383-477) for nstripes objects at once: split + pad,
 * parity, payload CRC32 and headers; fragments byte-identical to the reference's. */
int ecamd_frame_encode(int backend, int k, int m, int hd, int checksum, const void *d_obj,
                       int64_t obj_stride, uint64_t obj_size, void *d_frags, int64_t stripe_stride,
                       int64_t frag_stride, int nstripes, void *stream);
/* liberasurecode_decode (src/erasurecode.c:523-734) with fragments already in their index slots:
 * write the objects, rebuilding the missing (-1 terminated) data.  Surviving fragments are not
 * modified; the slots of missing ones may be overwritten (with their rebuilt payload). */
int ecamd_frame_decode(int backend, int k, int m, int hd, const int *missing, void *d_frags,
                       int64_t stripe_stride, int64_t frag_stride, int nstripes, void *d_obj,
                       int64_t obj_stride, uint64_t obj_size, void *stream);
/* liberasurecode_reconstruct_fragment (src/erasurecode.c:748-949): rebuild fragment `dest` of
 * every stripe in its slot, header and checksum included. */
int ecamd_frame_reconstruct(int backend, int k, int m, int hd, int checksum, const int *missing,
                            int dest, void *d_frags, int64_t stripe_stride, int64_t frag_stride,
                            uint64_t obj_size, int nstripes, void *stream);
/* Header / checksum audit of nfrag fragments per stripe: d_status[s*nfrag+f] bit 0 bad magic, 1 bad
 * metadata checksum (neither zlib nor legacy), 2 idx != f, 3 size != blocksize, 4 payload CRC32
 * mismatch (when the header says CRC32; `legacy` picks the machine).  d_crc (optional) receives the
 * computed payload CRCs. */
int ecamd_frame_verify(int nfrag, int64_t blocksize, int legacy, const void *d_frags,
                       int64_t stripe_stride, int64_t frag_stride, int nstripes, uint32_t *d_status,
                       uint32_t *d_crc, void *stream);
/* The glue from the audit to ecamd_rs_decode_masks (backend 6) and ecamd_xor_decode_masks (backend 3):
 * d_masks[s] (nstripes uint32, device memory) gets bit f when d_frag_status[s*nfrag + f] & bits is
 * non-zero; d_frag_status has the layout ecamd_frame_verify writes, nfrag <= 32.  One small kernel,
 * asynchronous on `stream`.  With it
 *   ecamd_frame_verify -> ecamd_frame_status_masks(bits = 1 << 4) -> ecamd_rs_decode_masks(base = d_frags + 80)
 *                                                                 or ecamd_xor_decode_masks(base = d_frags + 80)
 * heals payload damage of framed stripes on one stream with one wait at the end: the header still
 * holds the original payload's CRC32, so the rebuilt payload matches it again.  Fragments with a bad
 * HEADER (bits 0-3) -- a replaced disk, a slot of garbage -- need their header restamped as well: pass
 * bits = 0x1F and give the masks to ecamd_frame_reconstruct_masks (below) instead of the payload decode.
 * ECAMD_EINVAL (nothing written) for null arrays, nfrag < 1 or > 32, nstripes < 0. */
int ecamd_frame_status_masks(int nfrag, const uint32_t *d_frag_status, uint32_t bits, int nstripes,
                             uint32_t *d_masks, void *stream);
/* ---- whole fragments from device masks: ecamd_frame_reconstruct for batches in which every stripe lost
 * its own fragments, headers included ----
 * backend 6 (rs_vand) or 3 (flat_xor_hd); checksum and obj_size as for ecamd_frame_reconstruct; the layout
 * that of the other framed calls (blocksize from ecamd_frame_geometry).  d_lost (nstripes uint32, DEVICE
 * memory) holds one mask per stripe, bit f set when fragment f of stripe s is lost, header and payload;
 * the word is read on the device, in stream order, exactly as ecamd_rs_decode_masks reads it.  With
 *   ecamd_frame_verify -> ecamd_frame_status_masks(bits = 0x1F) -> ecamd_frame_reconstruct_masks
 * every kind of fragment damage the audit can see is healed on one stream with one wait at the end, and
 * a second audit comes back all zero.  Per stripe, with L = d_lost[s]:
 *   L == 0                          nothing of the stripe is read or written; d_result[s] = 0.
 *   not recoverable                 by the payload decode's rule and by no other -- a bit >= k+m, more than
 *                                   m bits (rs_vand), hd or more bits (flat_xor_hd): nothing of the stripe
 *                                   is written, header or payload; d_result[s] = 0x80000000 | popcount(L).
 *   otherwise                       every fragment f in L is rebuilt whole.  Its payload is what
 *                                   ecamd_rs_decode_masks(rebuild_parity 1) / ecamd_xor_decode_masks(
 *                                   decode_parity 1) writes at base = d_frags + 80; its header is what
 *                                   ecamd_frame_reconstruct stamps for dest = f: add_fragment_metadata on a
 *                                   zeroed header, the payload CRC32 stored when checksum == 2 (the machine
 *                                   LIBERASURECODE_WRITE_LEGACY_CRC selects), any other checksum type
 *                                   stored but not computed.  d_result[s] = popcount(L).  On a consistent
 *                                   stripe the fragment is the one liberasurecode_encode produced, byte
 *                                   for byte.
 * Never written: surviving fragments (header or payload), the bytes between 80 + blocksize and frag_stride,
 * anything in front of d_frags.  Never read: lost slots before they are rebuilt, and -- in the stamp stage --
 * the payload of any fragment that was not rebuilt.
 * d_result (nstripes uint32, device memory, may be NULL: library scratch then holds the words, which the
 * stamp stage reads -- whether a stripe is recoverable stays the decode kernel's decision).  d_counts (3
 * uint32, device memory, may be NULL): (left alone, rebuilt, unrecoverable) as ecamd_rs_decode_masks.
 * There is no host dependence inside the call: no stream synchronise, no copy to the host, no launch whose
 * shape depends on the masks, no map-cache entry, no compile, and no allocation beyond library scratch per
 * (device, stream) that grows only when a larger batch arrives.  The launches are fixed: the payload
 * decode's, then -- with checksum == 2 -- a masked CRC-partial kernel (one wave per (stripe, j, span), j <
 * min(m, 8) or hd - 1: a wave reads the stripe's result and mask words as scalars, takes the j-th lost
 * fragment and leaves on a scalar branch when there is none, so a stripe with nothing to stamp costs two
 * word loads per wave and no payload traffic; the span arithmetic, image and knobs are crc_partial_kernel's),
 * then one stamp kernel (one thread per (stripe, j): the fold of the span partials and tail bytes, the 80
 * header bytes as five 16-byte stores).  Neither grid nor the partials scale with k + m.
 * ECAMD_EINVAL, with everything untouched, for what the other framed calls reject (backend, code, 16-byte
 * aligned base and strides, frag_stride >= 80 + blocksize rounded up to 16), a null d_lost or d_frags,
 * nstripes < 0 and, for backend 6, m > 8 or k+m > 32 (ecamd_rs_decode_masks' limits).  nstripes == 0
 * returns 0 and writes nothing.
 * When to prefer ecamd_frame_reconstruct: DESIGN.md "Whole fragments from device masks", INTEGRATION.md. */
int ecamd_frame_reconstruct_masks(int backend, int k, int m, int hd, int checksum, const uint32_t *d_lost,
                                  void *d_frags, int64_t stripe_stride, int64_t frag_stride, uint64_t obj_size,
                                  int nstripes, uint32_t *d_result /* may be NULL */,
                                  uint32_t *d_counts /* 3 words, may be NULL */, void *stream);
/* Launches of frame_stamp_masks_kernel (the stamp kernel) enqueued by this process: one per call with a
 * non-empty batch. */
long long ecamd_frame_reconstruct_masks_launches(void);
/* zlib crc32(0, buf, len) (legacy = 0) or liberasurecode_crc32_alt(0, buf, len) (legacy = 1) of
 * every buffer d_base + s*stripe_stride + f*frag_stride, f < nfrag: d_crc[s*nfrag + f]. */
int ecamd_crc32(int legacy, const void *d_base, int64_t stripe_stride, int64_t frag_stride,
                int nfrag, int64_t len, int nstripes, uint32_t *d_crc, void *stream);

/* ---- synthetic data: splitmix64 stream per fragment, seed = seed_base ^ (s<<8) ^ f ---- */
int ecamd_fill_splitmix(void *base, int64_t stripe_stride, int64_t frag_stride, int nfrags,
                        int64_t blocksize, int nstripes, int stripe0, uint64_t seed_base,
                        void *stream);

/* ---- device memory helpers for C / ctypes callers ---- */
int ecamd_malloc(void **d_ptr, int64_t bytes);
/* Device memory the host may also write directly (the same address, through the PCIe BAR), uncached on the
 * GPU side; ECAMD_EINVAL where the platform does not map device memory for the host.  The per-call path
 * packs small calls' inputs there instead of staging them through a DMA. */
int ecamd_malloc_host_writable(void **d_ptr, int64_t bytes);
int ecamd_free(void *d_ptr);
int ecamd_memcpy_h2d(void *d_dst, const void *h_src, int64_t bytes);
int ecamd_memcpy_d2h(void *h_dst, const void *d_src, int64_t bytes);
int ecamd_memset(void *d_ptr, int value, int64_t bytes); /* synchronous: complete on return */
/* kind: 0 host->device, 1 device->host, 2 device->device; asynchronous on stream */
int ecamd_memcpy_async(void *dst, const void *src, int64_t bytes, int kind, void *stream);
int ecamd_host_alloc(void **h_ptr, int64_t bytes); /* pinned host memory */
int ecamd_host_free(void *h_ptr);
int ecamd_synchronize(void);
int ecamd_stream_create(void **stream);
/* Also releases the library's per-stream context of that stream (side stream, scratch). */
int ecamd_stream_destroy(void *stream);
/* hipStreamDestroy on the library's own HIP runtime WITHOUT releasing its context -- what a caller that
 * destroys a stream behind the library's back does (tests: the contexts stay bounded anyway). */
int ecamd_stream_destroy_unmanaged(void *stream);
int ecamd_stream_synchronize(void *stream);
/* 0 when all work on stream is complete, 1 while some is pending, ECAMD_EHIP on error. */
int ecamd_stream_query(void *stream);
/* Per-(device, stream) contexts the framed calls hold (side stream + events + CRC scratch): bounded --
 * released by ecamd_stream_destroy, and idle ones of other streams past a cap of 16 (diagnostics). */
int ecamd_stream_contexts(void);
/* HIP events for timing work on a stream (elapsed_ms waits for `stop`). */
int ecamd_event_create(void **ev);
int ecamd_event_destroy(void *ev);
int ecamd_event_record(void *ev, void *stream);
int ecamd_event_elapsed_ms(void *start, void *stop, float *ms);

#ifdef __cplusplus
}
#endif
#endif
