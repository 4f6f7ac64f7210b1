// ecamd_internal.hpp -- what the files of libecamd.so's device side take from each other, free of kernel
// argument types (those: ecamd_launch.hpp).  Each section names the file that defines it.
#pragma once
#include <vector>
#include <stddef.h>
#include <stdint.h>

#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <type_traits>

struct ecamd_map;

// The HIP call failed: its text becomes the thread's error text and the caller returns ECAMD_EHIP
// (needs <hip/hip_runtime.h> and ecamd.h where it is used).
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return ecamd::dev_fail(ECAMD_EHIP, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

namespace ecamd {

struct FragmentMap;

// ---- ecamd_runtime.hip ----
// The one writer of the thread's error text (ecamd_last_error): sets it and returns code.
int dev_fail(int code, const char* fmt, ...);

// "Upload a small table once and keep it": `bytes` of host words into device memory of their own, complete
// on return; the buffer is freed again when the copy fails.  ECAMD_EHIP with the text "<what>: <HIP's>".
// Where and for how long the pointer is cached is the caller's business.
int upload_table(const char* what, const void* host, size_t bytes, const void** dev);
// A device table made at most once and owned by whatever holds this (a cached map entry): made under
// `once` with upload_table, `rc` its result, `words` its length in 32-bit words; freed with the owner.
struct OnceTable {
    std::once_flag once;
    int rc = 0;
    const uint32_t* dev = nullptr;
    size_t words = 0;
    ~OnceTable();
};

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// The apply entry points' rule: both bases, both stripe strides and every fragment offset are multiples
// of 16 ("fragment addresses must be 16-byte aligned").
inline bool frags_aligned16(const void* in_base, const void* out_base, int64_t in_stride, int64_t out_stride,
                            const int64_t* in_off, int K, const int64_t* out_off, int R)
{
    bool ok = aligned16(in_base) && aligned16(out_base) && (in_stride % 16) == 0 && (out_stride % 16) == 0;
    for (int j = 0; j < K; j++) ok = ok && (in_off[j] % 16) == 0;
    for (int r = 0; r < R; r++) ok = ok && (out_off[r] % 16) == 0;
    return ok;
}

// Where a strided batch lies: fragment f of stripe s at base + s*stripe_stride + f*frag_stride, blocksize
// bytes each.  The two rules every entry point over such a batch starts with; the message, and the
// null tests of its other pointers, are the entry point's own.
struct StripeLayout {
    uint8_t* base;  // written only by the calls that say so (correct, decode_masks)
    int64_t stripe_stride, frag_stride, blocksize;
    int nstripes;
    bool sane() const { return base && nstripes >= 0 && blocksize >= 1 && frag_stride >= blocksize; }
    bool aligned16() const { return frags_aligned16(base, base, stripe_stride, stripe_stride, &frag_stride, 1, nullptr, 0); }
};

// f(std::integral_constant<int, N>{}) with N = groups held to [Lo, Hi]: the one place a count of
// four-fragment load groups picks the kernel<N> to launch.
template <int Lo, int Hi, class F>
void with_groups(int groups, F&& f)
{
    if constexpr (Lo < Hi) {
        if (groups > Lo) return with_groups<Lo + 1, Hi>(groups, f);
    }
    f(std::integral_constant<int, Lo>{});
}

// The device tables of one kind, one per code: made at the first call that asks for `key` -- (device,
// code...) --, by build(bytes) (0, or its own dev_fail) and upload_table(what), and kept for the life of
// the process.  A table that could not be made is tried again by the next call.
template <size_t N>
class CodeTables {
public:
    explicit CodeTables(const char* what) : what_(what) {}
    template <class Build>
    int get(const std::array<int, N>& key, Build&& build, const void** out)
    {
        const std::lock_guard<std::mutex> lk(mu_);
        const void*& slot = tables_[key];
        if (!slot) {
            std::vector<uint8_t> bytes;
            if (const int rc = build(bytes)) return rc;
            const void* d = nullptr;  // once per code, before anything of the call is enqueued
            if (const int rc = upload_table(what_, bytes.data(), bytes.size(), &d)) return rc;
            slot = d;
        }
        *out = slot;
        return 0;
    }

private:
    const char* what_;
    std::mutex mu_;
    std::map<std::array<int, N>, const void*> tables_;
};

// Asynchronous upload of a small host table (stripe list, pointer table) on `stream` through a
// ring of pinned slots per (device, stream); call end() after enqueuing the launches that read
// `dev`.
struct StagedSlot;
struct StagedRing;
struct StagedUpload {
    void* dev = nullptr;
    int begin(int device, void* stream, const void* src, size_t bytes);
    int end(void* stream);  // records the slot's event behind the launches and releases it
    ~StagedUpload() { end(stream_); }

private:
    StagedRing* ring_ = nullptr;
    StagedSlot* slot_ = nullptr;
    void* stream_ = nullptr;
};

// ---- ecamd_device.hip ----
// Strided flat-XOR apply (ecamd_xor_apply_strided) over the stripes listed in the device array
// d_list (logical stripe i is stripe d_list[i] of the layout); ECAMD_EINVAL when the stream
// kernel cannot take the shape.
int xor_apply_list(const uint32_t* masks, int R, int K, void* base, int64_t stripe_stride,
                   const int64_t* in_off, const int64_t* out_off, int64_t blocksize, int nstripes,
                   const int32_t* d_list, void* stream);

int dev_ensure(int* dev_out);                       // 0, or ECAMD_ENODEV / ECAMD_EHIP
int dev_cu_count(int dev);
// Stripes per launch of a strided pass split into launches of at most `limit` tiles per resident
// workgroup (`slots` of them), as even as the stripes allow; limit 0: one launch (for_each_launch in
// ecamd_device.hip, xor_check_fused in ecamd_check.hip).
int launch_stripes(int nstripes, uint64_t tiles_per_stripe, uint64_t slots, uint64_t limit);

// ---- ecamd_runtime.hip: the per-(device, stream) contexts ----
// Side stream of (dev, stream) for work beside the caller's launches (knob frame_tail_fork):
// side_fork orders it after everything issued to `stream` so far, side_join orders `stream` after
// everything issued to the side stream since.
// The side stream and the scratch slots live in a per-(dev, stream) context (ecamd_runtime.hip),
// bounded: ecamd_stream_destroy releases a stream's, and idle ones are released past a small cap.
int side_fork(int dev, void* stream, void** side);
int side_join(int dev, void* stream);
// Device scratch of `words` 32-bit words in slot 0..kStreamScratchSlots-1 of (dev, stream); calls
// on one stream are ordered, so reuse is safe (slot 1 holds values that must outlive a CRC pass on
// the same stream, whose partials use slot 0).
// Slot 4: the small-launch fused CRC's counter and partials (ecamd_map_apply_strided_crc).  A slot is
// zeroed when it is (re)allocated.  Slot 5: the fragments the checks and locates of ecamd_check.hip
// compute to compare the stored ones against (generic stage; at most kCheckScratchBytes).  Slot 6: the
// per-stripe records of ecamd_rs_decode_masks (ecamd_decode_masks.hip; 560 bytes per stripe of the
// largest batch seen).  Slots 7 and 8: ecamd_frame_reconstruct_masks (ecamd_frame_api.hip) -- the decode's
// result words when the caller passes none, and the span partials of its stamp stage; slots of their
// own, so that neither the decode's records (6), a check's fragments (5) nor a CRC pass's partials (0)
// enqueued around it on the same stream share a buffer with them.
constexpr int kStreamScratchSlots = 9;
constexpr int kSmallCrcScratchSlot = 4;
constexpr int kCheckScratchSlot = 5;
constexpr int kMasksPlanScratchSlot = 6;
constexpr int kFrameMasksResultSlot = 7;
constexpr int kFrameMasksPartialSlot = 8;
constexpr size_t kCheckScratchBytes = size_t(64) << 20;
int stream_scratch(int dev, void* stream, int slot, size_t words, uint32_t** out);
// A framed call in progress on (dev, stream): its context is not released until the call has
// returned and its work on the stream has completed.
int stream_use_begin(int dev, void* stream);
void stream_use_end(int dev, void* stream);
struct StreamUse {
    int dev;
    void* stream;
    StreamUse(int d, void* s) : dev(d), stream(s) { (void)stream_use_begin(d, s); }
    ~StreamUse() { stream_use_end(dev, stream); }
    StreamUse(const StreamUse&) = delete;
    StreamUse& operator=(const StreamUse&) = delete;
};
void stream_forget(void* stream);
int stream_contexts();

// ---- ecamd_rs.hip ----
// The one rs_vand planner: the FragmentMap (host/gf16.hpp) of kind 0 encode, 1 decode (`rebuild`: parity
// too), 2 reconstruct `dest`, 4 check (every surviving fragment beyond the first k) of the code (k, m)
// with `missing` (-1 terminated, may be null) lost.  Host only, no device.  ECAMD_EINVAL with the texts
// "bad k=.. m=..", "no generator for ..", "too many missing fragments (..)", "cannot reconstruct ..".
int rs_vand_plan(int kind, int k, int m, const int* missing, int dest, int rebuild, FragmentMap& fm);
// The cached check map of the rs_vand code (k, m) with `missing` (-1 terminated, may be null) lost:
// the first k available fragments are the inputs, every other available one is checked.  `hold` keeps
// the entry alive past its eviction from the map cache.  ECAMD_EINVAL for too many missing fragments.
// `pairs`, `correct`: the entry's attachments for the device tables of the pair and correct stages, which
// ecamd_check.hip makes on demand; they live and are freed with the entry (`hold`).
struct CheckMap {
    const std::vector<int>* inputs = nullptr;   // fragment indices of the K inputs
    const std::vector<int>* checked = nullptr;  // fragment indices of the R checked fragments
    const std::vector<int>* coeff = nullptr;    // R x K, row-major (null when R == 0)
    const ecamd_map* map = nullptr;             // the same map for the apply calls (null when R == 0)
    OnceTable* pairs = nullptr;
    OnceTable* correct = nullptr;
    std::shared_ptr<const void> hold;
};
int check_map(int k, int m, const int* missing, CheckMap& out);

// ---- ecamd_check.hip ----
// The grid of the kernels that go stripe by stripe (locate_pairs_kernel, correct_kernel,
// decode_masks_kernel): a chunk per 4096 units of a fragment, at most 64, by as many stripe slots as keep
// the grid within 4096 workgroups; knob pairs_grid > 0 caps both dimensions.
void stripe_grid(int64_t units, int nstripes, int& chunks, int& slots);

// ---- ecamd_check.hip: who takes part in a check, locate or correct call ----
// The K inputs, then the R checked rows (K + R <= 32): participant c of stripe s lies at base +
// s*stripe_stride + off[c] and is fragment bit[c]; mask has the bits of them all.
struct Participants {
    int K = 0, R = 0;
    int64_t off[32] = {};
    uint8_t bit[32] = {};
    uint32_t mask = 0;
};

// ---- ecamd_device.hip ----
// Fused stage of a check or, with d_suspects, of a locate: rows [row0, row0 + nrows) of the R x K
// matrix A as the syndrome map [A | I] through the check / locate form of the bitsliced kernel, over
// whole tiles of every stripe of `lay`, the inputs and checked rows where `p` has them.
// Returns the bytes of each fragment covered -- 0 when the shape, the knobs or a kernel still
// compiling decline, nothing launched -- or an error (< 0).
int64_t check_fused(int dev, const std::vector<int>& A, const Participants& p, int row0, int nrows, const StripeLayout& lay,
                    uint32_t* d_status, uint32_t* d_suspects, void* stream);
// Build time (no GPU): the code object check_fused will ask for over the same rows, into `dir`
// (bitslice_prebuild's result: 1 present, 0 no fused form under the current knobs, < 0 failed; -6
// from the locate form: every build needs scratch, so the run time declines it too).
int check_fused_prebuild(const std::vector<int>& A, int K, int row0, int nrows, bool locate, const char* arch,
                         const char* dir);

// ---- ecamd_copy.hip: copy-through launches of the framed calls ----
// rs_vand encode whose k data inputs are read from objects (input j of stripe s at
// obj + s*obj_stride + j*bs) and copied into payload j while the parity is computed
// (payload f of stripe s at payload0 + s*stripe_stride + f*frag_stride).  Objects of obj_size
// bytes (< 0: k*bs) are zero-padded past their end (prepare_fragments_for_encode).  16-byte aligned
// object base / stride and payloads; bs even (the object side may be read unaligned).  from > 0 (a
// multiple of 16): only bytes [from, bs) of every payload (the rest of a partly fused encode); to > 0:
// only bytes [from, to).
int rs_encode_copy(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                   int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size = -1, int64_t from = 0, int64_t to = -1);

// Framed flat-XOR decode with data lost, straight into the objects: data output r (outputs[r] < k) =
// XOR of the inputs (fragment indices) whose coeff[r*K + col] is 1; every data input is copied into
// its object chunk by the same launch (the RS decode-join with a 0 / 1 matrix).
int xor_decode_join(int k, const std::vector<int>& inputs, const std::vector<int>& outputs,
                    const std::vector<int>& coeff, const void* payload0, int64_t stripe_stride, int64_t frag_stride,
                    void* obj, int64_t obj_stride, int64_t bs, int nstripes, void* stream, int64_t obj_size);

// The same crc variant for a flat-XOR code (parity r = XOR of the data chunks in masks[r], run as a
// 0 / 1 coefficient matrix through the bitsliced generator).
int xor_encode_copy_crc_bs(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                           int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                           const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos = 1,
                           int64_t cover = -1);

// Framed flat-XOR encode, copy-through: bytes [0, cover) of every payload (cover a multiple of 4096,
// every object chunk at least that long) from objects of obj_stride bytes whose chunk j starts at j*bs
// (unaligned loads when bs % 16 != 0): the data payloads are written as the chunks stream through the
// XOR kernel, parity r = XOR of the chunks in masks[r].  ECAMD_EINVAL, nothing launched, when it
// does not apply.
int xor_encode_copy(const uint32_t* masks, int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                    int64_t stripe_stride, int64_t frag_stride, int64_t bs, int64_t cover, int nstripes, void* stream);

// rs_vand decode straight into objects: the missing data fragments (at least one, -1 terminated
// `missing`) are computed into their object positions (j*bs) and the available data inputs are
// copied there by the same launch (fragments_to_string without a separate join pass).
// Objects of obj_size bytes (< 0: k*bs): nothing is written past an object's end.
int rs_decode_join(int k, int m, const int* missing, const void* payload0, int64_t stripe_stride,
                   int64_t frag_stride, void* obj, int64_t obj_stride, int64_t bs, int nstripes,
                   void* stream, int64_t obj_size = -1);

// rs_encode_copy with the payload CRC32s folded into the same launch (ecamd_frame_fused.hip):
// d_img = build_fused_crc_image(machine, 8192) in device memory; r0 of range r (q ranges of
// bs/q bytes) of payload f of stripe s -> d_partial[(s*(k+m) + f)*q + r].  ECAMD_EINVAL, with
// nothing launched, when the shape does not fit (bs % 8192, q must divide bs/8192, one map pass).
int rs_encode_copy_crc(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                       int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                       const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int mb = 1,
                       bool nib = false);
size_t fused_crc_lds(int k, int m, int mb, bool nib = false);  // LDS bytes of the fused framed encode
// The same on the bitsliced kernel's crc variant (up to 4 outputs, 16 KiB tiles, q ranges of
// 16 KiB tiles per payload; d_img: the CRC image built for a 4096-byte chain step).  ECAMD_EINVAL,
// nothing launched, when it does not apply or the kernel is not compiled yet.
int rs_encode_copy_crc_bs(int k, int m, const void* obj, int64_t obj_stride, void* payload0,
                          int64_t stripe_stride, int64_t frag_stride, int64_t bs, int nstripes,
                          const uint32_t* d_img, uint32_t* d_partial, int q, void* stream, int crc_pos = 1,
                          int64_t cover = -1);  // cover: the first `cover` bytes of each payload only
// Build time (no GPU): the code object the CRC32 framed encode's crc variant (crc_pos flags as
// rs_encode_copy_crc_bs takes them) will ask for, for the rs_vand code (k, m) (masks null) or the
// flat-XOR code with parity masks `masks`, into `dir` (ecamd_frame_prebuild).  1: present, 0: this
// form takes no bitsliced kernel, < 0: failed.
int crc_encode_prebuild(int k, int m, const uint32_t* masks, int crc_pos, const char* arch, const char* dir);
// fused image words with byte tables for the first mb dwords of a piece, nibble tables after
constexpr int crc_fused_words(int mb = 1) { return mb * 1024 + (4 - mb) * 128 + 8 * 128; }

}  // namespace ecamd
