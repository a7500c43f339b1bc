// pdog_host.hpp — what the host side of the C ABI shares between its translation units (pawsome_dog.hip,
// pawsome_group.hip, pawsome_diag.hip, pdog_math.cpp): the thread's error text, the reference's Float64 host arithmetic
// (pdog_math.cpp, plain C++) and, for the units that hipcc compiles, the HIP-error macro and the owning buffer type.
// Two more headers are plain C++ and carry no HIP either: pdog_mailbox.hpp, the layout of the tracker's host-coherent mailbox,
// which the kernel headers and pawsome_dog.hip both include, and pdog_policy.hpp, the two adaptive policies of the roll batch
// path, which pawsome_dog.hip includes alone; the host compiler tests both (tests/policy_main.cpp).
//
// WHERE KERNELS LIVE.  The kernels of the tracker (dog_*.hpp) are templates or `static __global__` functions in headers, and
// raise_lds_limit is keyed on a kernel's address: a second translation unit that included one of those headers would get
// private copies whose LDS limit was never raised.  So every include of a dog_*.hpp header of the tracker, every launch of
// its kernels and every raise_lds_limit stay in pawsome_dog.hip (the *_inst.hip units only hold explicit instantiations);
// this header and pdog_math.cpp include no kernel header.  (pawsome_diag.hip, pawsome_group.hip, pawsome_peaks.hip,
// pawsome_exclusive.hip and pawsome_motion.hip launch their own kernels, dog_diag.hpp's, group_compact_kernel, dog_peaks.hpp's,
// dog_assign.hpp's and dog_motion.hpp's, which no other unit names; pawsome_predict.hip launches nothing itself: the predicted
// chain's kernels are instances of the tracker's own, launched by launch_predicted in pawsome_dog.hip.)  The one exception is dog_step.hpp, which
// pawsome_dog.hip and pawsome_clips.hip both include: its kernel uses no dynamic LDS, so no limit is ever raised for it and
// a private copy per unit is harmless.
#pragma once
#include "../../include/pawsome_dog.h"
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)
namespace pdog {

// ---- the thread's pdog_last_error() text ----
int fail(int code, const std::string &msg); // sets the text, returns code

// ---- Float64 host arithmetic, as the reference does it (pdog_math.cpp) ----
double sigma_of(double tw);                                  // src/PawsomeTracker.jl:30
int kernel_len_of_sigma(double s);                           // Kernel.DoG
void gaussian_1d(double s, int l, double *g);                // KernelFactors.gaussian: exp(-x²/2σ²) / sum
void dense_dog_kernel(const double *gp, const double *gm, int l, bool darker, double *K); // :41-43, column-major
struct ExactFactors { double sym_int, sym_sep, ring, rescan; };
ExactFactors exact_factors(const std::vector<double> &gp, const std::vector<double> &gm); // exact mode's FP32 error-bound factors
double dog_kernel_norm_up(const std::vector<double> &gp, const std::vector<double> &gm);  // ‖K‖₂ of the dense kernel, rounded up (dog_prune.hpp's bound)
// A frame table (include/pawsome_video.h) checked on the host, before anything is launched: every entry below n_frames,
// negative entries only as the tail of a row.  out_len[c] = steps of clip c (its row's leading non-negative entries),
// *max_len the longest.  PDOG_E_ARG in `who`'s name, outputs undefined, otherwise.
int chain_table_lengths(const char *who, const int32_t *h_table, int n_steps, int n_clips, int n_frames, int32_t *out_len, int *max_len);
// What the entry points of include/pawsome_exclusive.h refuse alike: sizes outside their ranges, a ratio outside [0, 1] or NaN.
int check_exclusive(const char *who, int n_groups, int n_targets, int k, double min_ratio);
// What the entry points of include/pawsome_motion.h refuse beyond that: a min_response that is negative, NaN or infinite, coast < 0.
int check_motion(const char *who, double min_response, int coast);
// The test the entry points share for a stack of frames (and `counts_ok`: the entry point's own sizes); PDOG_E_ARG in `who`'s name.
// Accepted layouts (include/pawsome_dog.h, "frame layouts"): rows fw … PDOG_MAX_ROW_STRIDE bytes apart, any non-negative
// frame stride (overlapping frames and 0 included), any base address.
inline int check_row_stride(const char *who, int fw, int64_t row_stride)
{
    if (row_stride < fw) return fail(PDOG_E_ARG, std::string(who) + ": bad size/stride (row_stride < frame width)");
    if (row_stride > PDOG_MAX_ROW_STRIDE)
        return fail(PDOG_E_ARG, std::string(who) + ": row_stride " + std::to_string((long long)row_stride) + " exceeds PDOG_MAX_ROW_STRIDE (" + std::to_string((long long)PDOG_MAX_ROW_STRIDE) + ")");
    return PDOG_OK;
}
inline int check_stack(const char *who, int fw, int n_frames, int64_t row_stride, int64_t frame_stride, bool counts_ok = true)
{
    if (!(counts_ok && n_frames > 0 && frame_stride >= 0)) return fail(PDOG_E_ARG, std::string(who) + ": bad size/stride");
    return check_row_stride(who, fw, row_stride);
}
void pack_tile_geo(const uint8_t *frame, int fh, int fw, int64_t row_stride, int fill, int L, int r1, int r2, int g1, int g2,
                   uint8_t *dst, int64_t pitch, bool stream = false);

} // namespace pdog
#pragma GCC visibility pop

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include <cstring>

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return pdog::fail(PDOG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));   \
    } while (0)

#pragma GCC visibility push(hidden)
namespace pdog {

// A typed, move-only buffer that owns device memory (kPinned = false) or pinned host memory (kPinned = true: with its
// hipHostMalloc flags and, where those map it, its device alias).  capacity() counts elements.  The destructor frees: the
// owner drains its streams before its buffers go.
template <typename T, bool kPinned>
class Buffer {
public:
    explicit Buffer(unsigned host_flags = hipHostMallocDefault) : flags_(host_flags) {}
    Buffer(Buffer &&o) noexcept : flags_(o.flags_) { swap(o); }
    Buffer &operator=(Buffer &&o) noexcept { if (this != &o) { release(); swap(o); } return *this; }
    Buffer(const Buffer &) = delete;
    Buffer &operator=(const Buffer &) = delete;
    ~Buffer() { release(); }

    T *get() const { return p_; }
    T *device() const { return kPinned ? dev_ : p_; } // the address kernels use (pinned: only where the flags map it)
    size_t capacity() const { return cap_; }

    // Room for `count` elements.  Nothing happens when the capacity suffices.  Otherwise: `*drain` (if given) is
    // synchronised — kernels queued there may still use the old memory —, the old memory is freed, new memory allocated
    // and, with zero_fill, cleared.  On failure the buffer is empty.  try_reserve returns HIP's own error.
    hipError_t try_reserve(size_t count, const hipStream_t *drain, bool zero_fill = false)
    {
        if (count <= cap_) return hipSuccess;
        hipError_t e = drain ? hipStreamSynchronize(*drain) : hipSuccess;
        if (e != hipSuccess) return e;
        release();
        const size_t bytes = sizeof(T) * count;
        if (kPinned) {
            e = hipHostMalloc((void **)&p_, bytes, flags_);
            if (e == hipSuccess && (flags_ & hipHostMallocMapped)) e = hipHostGetDevicePointer((void **)&dev_, p_, 0);
            if (e == hipSuccess && zero_fill) std::memset(p_, 0, bytes);
        } else {
            e = hipMalloc((void **)&p_, bytes);
            if (e == hipSuccess && zero_fill) e = hipMemset(p_, 0, bytes);
        }
        if (e != hipSuccess) release();
        else cap_ = count;
        return e;
    }
    int reserve(size_t count, const hipStream_t *drain, bool zero_fill = false)
    {
        const hipError_t e = try_reserve(count, drain, zero_fill);
        return e == hipSuccess ? PDOG_OK : fail(PDOG_E_HIP, std::string("buffer of ") + std::to_string(sizeof(T) * count) + " bytes: " + hipGetErrorString(e));
    }
    void release()
    {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = dev_ = nullptr;
        cap_ = 0;
    }

private:
    void swap(Buffer &o) { std::swap(p_, o.p_); std::swap(dev_, o.dev_); std::swap(cap_, o.cap_); std::swap(flags_, o.flags_); }
    T *p_ = nullptr, *dev_ = nullptr;
    size_t cap_ = 0;
    unsigned flags_;
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

// Host words on their way to the device: pinned staging, the device copy, and the event that tells when the last upload
// has left the staging.  Grow-only.  Two calls may follow each other without a synchronisation between them, so staging()
// waits for the previous upload before the caller overwrites the words; send() queues the copy and records the event.
template <typename T>
class StagedUpload {
public:
    ~StagedUpload() { if (ev_) (void)hipEventDestroy(ev_); } // (the owner has drained its stream)

    // Room for n words on both sides (`stream` is drained if the device copy, which kernels queued there may still read,
    // has to grow); *out = the staging, the caller's to fill.
    int staging(size_t n, hipStream_t stream, T **out)
    {
        if (pending_) HIP_TRY(hipEventSynchronize(ev_));
        pending_ = false;
        if (int rc = host_.reserve(n, nullptr)) return rc;
        if (int rc = dev_.reserve(n, &stream)) return rc;
        *out = host_.get();
        return PDOG_OK;
    }
    int send(size_t n, hipStream_t stream)
    {
        if (!ev_) HIP_TRY(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        HIP_TRY(hipMemcpyAsync(dev_.get(), host_.get(), sizeof(T) * n, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(ev_, stream));
        pending_ = true;
        return PDOG_OK;
    }
    const T *device() const { return dev_.get(); }

private:
    PinnedBuffer<T> host_;
    DeviceBuffer<T> dev_;
    hipEvent_t ev_ = nullptr;
    bool pending_ = false;
};

// What pdog_detect_peaks (pawsome_peaks.hip, a unit of its own with its own kernel) keeps on a tracker.  It is a member of
// pdog_tracker, so it goes after the tracker's destructor has drained the stream; peaks_state (pawsome_dog.hip) hands it out
// with the tracker's device and PDOG_MAP_MB filled in.
struct PeaksState {
    bool no_list = false;                   // pdog_set_tuning "peaks_no_list": the selection rounds scan the map (dog_peaks.hpp)
    int device = 0;
    size_t map_cap = 0;                     // PDOG_MAP_MB, bytes
    DeviceBuffer<float> d_map;              // the chunk's response maps when the caller gives no buffer
    DeviceBuffer<int32_t> d_ij1;            // [n][2] the detect kernels' positions: pick 1
    DeviceBuffer<unsigned long long> d_stat; // [0] windows served, [1] windows whose candidate list overflowed
};
PeaksState *peaks_state(pdog_tracker *t);

// What the exclusive step and walk (pawsome_exclusive.hip, a unit of its own with its own kernels) keep on a tracker: a member
// of pdog_tracker like PeaksState; exclusive_state (pawsome_dog.hip) hands it out with the tracker's device filled in.
struct ExclusiveState {
    int device = 0;
    DeviceBuffer<int32_t> d_words;  // per window: the current guess [n][2], the picks [n][k][2], the counts [n]
    DeviceBuffer<float> d_peak;     // [n][k] the picks' values
    StagedUpload<int32_t> table;    // the validated table by step, a frame per WINDOW [max_len][n], then the groups' lengths [G]
    std::vector<int32_t> len;       // steps per group of the table being served
    size_t table_words = 0;         // the most words `table` was asked for
    uint64_t steps = 0, grown = 0;  // pdog_get_exclusive_counts
};
ExclusiveState *exclusive_state(pdog_tracker *t);

// The same for the motion step and walk (pawsome_motion.hip, its own unit and kernels); motion_state (pawsome_dog.hip).
struct MotionState {
    bool lds = false;               // pdog_set_tuning "motion_lds": the kernel stages the lists in LDS (dog_motion.hpp)
    int device = 0;
    DeviceBuffer<int32_t> d_words;  // per window: the position [n][2], the guess [n][2], the walk's own mstate [n][4], the picks [n][k][2], the counts [n]
    DeviceBuffer<float> d_peak;     // [n][k] the picks' values
    StagedUpload<int32_t> table;    // as ExclusiveState's
    std::vector<int32_t> len;
    size_t table_words = 0;
    uint64_t steps = 0, grown = 0;  // pdog_get_motion_counts
};
MotionState *motion_state(pdog_tracker *t);

// The predicted chain (include/pawsome_predict.h; pawsome_predict.hip holds its entry points).  Its one-launch kernels are
// instances of the tracker's own chain kernels, so their launch stays in pawsome_dog.hip (see above): launch_predicted.
struct PredictState {
    int device = 0;
    std::vector<int32_t> len;       // steps per clip of the table being served
    size_t table_words = 0;         // the most words the staged table was asked for
    uint64_t fused = 0, persistent = 0, fallback = 0, grown = 0; // pdog_get_predict_counts
};
PredictState *predict_state(pdog_tracker *t);
// A validated walk (h_table's lengths in len, the longest max_len >= 1) on the kernel chain_path chooses.  *taken = 1: one
// launch of the fused kernel's predicted instance; 2: of the persistent chain kernel's; 0: nothing was launched or staged — the
// geometry is the tiled kernel's or the stepped walk's, or the kernel length has no instance — and the caller falls back.
struct PredictWalk {
    const uint8_t *d_frames;
    int64_t frame_stride, row_stride;
    const int32_t *h_table, *len;
    int max_len, n_steps, n_clips, first;
    float m;
    int coast;
    const int32_t *d_start;
    int32_t *d_out_ij, *d_out_state, *d_mstate;
};
int launch_predicted(pdog_tracker *t, const PredictWalk &w, int *taken);

} // namespace pdog
#pragma GCC visibility pop
#endif // __HIPCC__
