// pdog_host.hpp — what the host side of the C ABI shares between its translation units (pawsome_dog.hip,
// pawsome_group.hip, pawsome_diag.hip, pdog_math.cpp): the thread's error text, the reference's Float64 host arithmetic
// (pdog_math.cpp, plain C++) and, for the units that hipcc compiles, the HIP-error macro and the owning buffer type.
// Two more headers are plain C++ and carry no HIP either: pdog_mailbox.hpp, the layout of the tracker's host-coherent mailbox,
// which the kernel headers and pawsome_dog.hip both include, and pdog_policy.hpp, the two adaptive policies of the roll batch
// path, which pawsome_dog.hip includes alone; the host compiler tests both (tests/policy_main.cpp).  Two further ones carry the
// arithmetic around the kernels: dog_layout.hpp, the kernels' size formulas (LDS pitches and byte counts), which every kernel
// header includes and any host program may; and pdog_plan.hpp, the tracker's plan as a value (Switches, the variants' shapes,
// make_plan, path_for_batch, chain_path, the exact-mode thresholds), which includes dog_layout.hpp and dog_roll_range.hpp, no
// kernel header, and which pawsome_dog.hip and the host's test program (tests/plan_main.cpp) include.
//
// WHERE KERNELS LIVE.  The kernels of the tracker (dog_*.hpp) are templates or `static __global__` functions in headers, and
// raise_lds_limit is keyed on a kernel's address: a second translation unit that included one of those headers would get
// private copies whose LDS limit was never raised.  So every include of a dog_*.hpp header of the tracker, every launch of
// its kernels and every raise_lds_limit stay in pawsome_dog.hip (the *_inst.hip units only hold explicit instantiations);
// this header, pdog_walk.hpp, pdog_plan.hpp and pdog_math.cpp include no kernel header: what names no kernel and makes no HIP
// call — which variant, how many strips, which path, how much LDS — is pdog_plan.hpp's, and pawsome_dog.hip applies it
// (apply_plan: the limits a plan lists, the occupancy questions, then the assignment).  (pawsome_diag.hip, pawsome_group.hip, pawsome_peaks.hip,
// pawsome_exclusive.hip and pawsome_motion.hip launch their own kernels, dog_diag.hpp's, group_compact_kernel, dog_peaks.hpp's,
// dog_assign.hpp's and dog_motion.hpp's, which no other unit names; the last two hold nothing but those launches and their
// geometry: the walk around them — checks, scratch, staged table, the loop over pdog_detect_peaks — is pdog_walk.hpp's, which
// takes the rule's launch as a callable and so names no kernel.  pawsome_predict.hip launches nothing itself: the predicted
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
// The pre-pass's second stage (dog_prune.hpp, "the cell bound"): Σ K² of the box of the dense kernel that an output at offset
// (i, j) of its 8 × 8 cell takes from the input cell (dy, dx) cells further on, and the integer weights of the NS × NS input
// cells, NS = refine_span(l) (= prune_span(l), dog_roll_range.hpp), in units of ‖K‖₂ / 2¹², rounded up.
inline int refine_span(int l) { return (8 + l - 1 + 7) / 8; }
struct RefineBoxes {
    int ns;
    std::vector<double> A, B, C; // [d][i]: Σ g₊², Σ g₋², Σ g₊g₋ over the kernel rows [8d − i, 8d − i + 8) ∩ [0, l)
    RefineBoxes(const std::vector<double> &gp, const std::vector<double> &gm, bool f32); // f32: the taps rounded to float first
    double norm2(int dy, int i, int dx, int j) const;
};
std::vector<uint32_t> dog_refine_weights(const std::vector<double> &gp, const std::vector<double> &gm, double norm_up);
// A frame table (include/pawsome_video.h) checked on the host, before anything is launched: every entry below n_frames,
// negative entries only as the tail of a row.  out_len[c] = steps of clip c (its row's leading non-negative entries),
// *max_len the longest.  PDOG_E_ARG in `who`'s name, outputs undefined, otherwise.
int chain_table_lengths(const char *who, const int32_t *h_table, int n_steps, int n_clips, int n_frames, int32_t *out_len, int *max_len);
// One walk over a frame table, as every entry point that takes one describes it: the frame stack, the table's n_rows rows of
// n_steps entries, `windows` windows per row (a clip is one, a group its targets) and `first`.  n_strips > 0: the walk's steps
// go through pdog_detect_peaks, whose limit on a batch (n_rows * windows windows of n_strips strips) is judged here.
struct TableWalk {
    const char *who;
    int fw, n_frames;
    int64_t row_stride, frame_stride;
    const int32_t *h_table;
    int n_steps, n_rows, windows, first, n_strips;
    int max_len; // check_table_walk's: the longest row (0: no row has a step, nothing is to be done)
};
// The tests the table walks share, in the order they are refused: check_stack (the sizes positive, n_rows * windows * n_steps
// within 31 bits), the batch limit, first = 0 or 1, then the table itself; len grows to n_rows and receives the rows' lengths.
int check_table_walk(TableWalk &w, std::vector<int32_t> &len);
// The words a walk's table is staged as, and their arithmetic.  windows = 0: the rows as given, n_rows x n_steps — what the
// kernels that walk a clip themselves read.  windows = T >= 1: by step with a frame per WINDOW, [max_len][n_rows][T] (step s's
// cells are that batch's frame index); a row that has ended repeats its last frame (frame 0 if it has none).  The rows'
// lengths follow the cells either way.
struct TableShape { int n_steps, n_rows, max_len, windows; };
inline size_t table_cells(const TableShape &s) { return s.windows ? (size_t)s.max_len * s.n_rows * s.windows : (size_t)s.n_rows * s.n_steps; }
void fill_table(const int32_t *h_table, const int32_t *len, const TableShape &s, int32_t *out); // out: table_cells(s) + n_rows words
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

// A walk's validated table on its way to the device: the rows' lengths, the staged words (fill_table's layouts) and the most
// words any upload asked for.  Every family of walks keeps its own (the tracker's chains, the exclusive and the motion walk, the
// predicted chain), so a family's `grown` counts its own high-water marks alone.  Walks may follow each other on one stream
// without a synchronisation: staging() waits for the previous upload's event before the pinned words are overwritten, and the
// device copy is overwritten in stream order, behind the kernels that read it.
struct StagedTable {
    std::vector<int32_t> len; // steps per row of the table being served (check_table_walk)

    // h_table and len in `s`'s layout, queued on `stream`; ++*grown (if given) where that takes more words than ever before.
    int upload(const int32_t *h_table, const TableShape &s, hipStream_t stream, uint64_t *grown, const int32_t **d_cells, const int32_t **d_len)
    {
        const size_t cells = table_cells(s), n = cells + (size_t)s.n_rows;
        if (n > most_) { most_ = n; if (grown) ++*grown; }
        int32_t *hp = nullptr;
        if (int rc = words_.staging(n, stream, &hp)) return rc;
        fill_table(h_table, len.data(), s, hp);
        if (int rc = words_.send(n, stream)) return rc;
        *d_cells = words_.device();
        *d_len = words_.device() + cells;
        return PDOG_OK;
    }

private:
    StagedUpload<int32_t> words_;
    size_t most_ = 0;
};

// What a walk of groups keeps on a tracker — the exclusive walk and the motion walk, a member of pdog_tracker each like
// PeaksState (their units, pawsome_exclusive.hip and pawsome_motion.hip, have their own kernels); exclusive_state and
// motion_state (pawsome_dog.hip) hand them out with the tracker's device filled in, motion_lds the motion kernel's switch.
struct GroupWalkState {
    int device = 0;
    DeviceBuffer<int32_t> d_words;  // per window: what the rule carries from step to step, then the picks [n][k][2], the counts [n] (pdog_walk.hpp)
    DeviceBuffer<float> d_peak;     // [n][k] the picks' values
    StagedTable table;              // by step, a frame per window
    uint64_t steps = 0, grown = 0;  // pdog_get_exclusive_counts / pdog_get_motion_counts
};
GroupWalkState *exclusive_state(pdog_tracker *t);
GroupWalkState *motion_state(pdog_tracker *t);
bool motion_lds(const pdog_tracker *t); // pdog_set_tuning "motion_lds": the kernel stages the lists in LDS (dog_motion.hpp)

// The predicted chain (include/pawsome_predict.h; pawsome_predict.hip holds its entry points).  Its one-launch kernels are
// instances of the tracker's own chain kernels, so their launch stays in pawsome_dog.hip (see above): launch_predicted.
struct PredictState {
    int device = 0;
    StagedTable table;              // the rows as given
    uint64_t fused = 0, persistent = 0, fallback = 0, grown = 0; // pdog_get_predict_counts
};
PredictState *predict_state(pdog_tracker *t);
// A validated walk (its rows' lengths in the state's table, the longest walk.max_len >= 1) on the kernel chain_path chooses.
// *taken = 1: one launch of the fused kernel's predicted instance; 2: of the persistent chain kernel's; 0: nothing was launched
// or staged — the geometry is the tiled kernel's or the stepped walk's, or the kernel length has no instance — and the caller
// falls back.
struct PredictWalk {
    TableWalk walk;
    const uint8_t *d_frames;
    float m;
    int coast;
    const int32_t *d_start;
    int32_t *d_out_ij, *d_out_state, *d_mstate;
};
int launch_predicted(pdog_tracker *t, const PredictWalk &w, int *taken);

} // namespace pdog
#pragma GCC visibility pop
#endif // __HIPCC__
