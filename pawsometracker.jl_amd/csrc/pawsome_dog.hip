// pawsome_dog.hip — host side of the C ABI declared in include/pawsome_dog.h.
//
// Mirrors the `Tracker` constructor (/root/reference/src/PawsomeTracker.jl:39-52):
// σ and the two Gaussian factors of Kernel.DoG are built in Float64 on the host
// exactly as the reference builds them, rounded to f32 once, and kept on the
// device; the functor (:55-62) becomes kernel launches on a HIP stream.
// There is NO CPU fallback: without a gfx950 device pdog_create fails.
#include "pdog_host.hpp"
#include "pdog_mailbox.hpp"
#include "pdog_policy.hpp"
#include "pdog_plan.hpp"
#include "dog_kernels.hpp"
#include "dog_roll.hpp"
#include "dog_prune.hpp"
#include "dog_twopass.hpp"
#include "dog_fused.hpp"
#include "dog_exact.hpp"
#include "dog_tiled.hpp"
#include "dog_measure.hpp"
#include "dog_step.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

using namespace pdog;

// compile-time-length instances of the latency kernels: built in lat_inst.hip, one translation unit per length
namespace pdog {
#define PDOG_LAT_L(LT)                                                                                          \
    extern template __global__ void dog_fused_kernel<false, 0, LT>(const FusedGeo, const f2 *, const f2 *);    \
    extern template __global__ void dog_fused_kernel<true, 0, LT>(const FusedGeo, const f2 *, const f2 *);     \
    extern template __global__ void dog_tiled_kernel<false, LT>(const TiledGeo, const f2 *, const f2 *);       \
    extern template __global__ void dog_tiled_kernel<true, LT>(const TiledGeo, const f2 *, const f2 *);        \
    extern template __global__ void dog_fused_kernel<false, 0, LT, true>(const FusedTableGeo, const f2 *, const f2 *); \
    extern template __global__ void dog_tiled_kernel<false, LT, true>(const TiledTableGeo, const f2 *, const f2 *); \
    extern template __global__ void dog_fused_kernel<false, 0, LT, true, true>(const FusedPredictGeo, const f2 *, const f2 *);
#include "lat_lengths.def"
#undef PDOG_LAT_L
} // namespace pdog

// the roll kernels are instantiated in roll_inst.hip (one translation unit per set of lengths, built in parallel)
namespace pdog {
#define PDOG_ROLL_L(LT)                                                                                          \
    extern template __global__ void dog_roll_kernel<LT, false, 0>(const LaunchGeo, const f2 *, const f2 *);      \
    extern template __global__ void dog_roll_kernel<LT, true, 0>(const LaunchGeo, const f2 *, const f2 *);       \
    extern template __global__ void dog_roll_kernel<LT, false, 0, -1, true>(const LaunchGeo, const f2 *, const f2 *); \
    extern template __global__ void dog_thin_kernel<LT, false>(const LaunchGeo, const f2 *, const f2 *);         \
    extern template __global__ void dog_thin_kernel<LT, true>(const LaunchGeo, const f2 *, const f2 *);          \
    extern template __global__ void dog_chain_kernel<LT>(const ChainGeo, const f2 *, const f2 *);                \
    extern template __global__ void dog_chain_kernel<LT, true>(const ChainTableGeo, const f2 *, const f2 *);    \
    extern template __global__ void dog_chain_kernel<LT, true, true>(const ChainPredictGeo, const f2 *, const f2 *);
#include "roll_lengths.def"
#undef PDOG_ROLL_L
#define PDOG_EPI_CLASSES(X) X(10) X(2) X(16) X(14) X(6) X(4) X(0) X(1) X(3) X(5) X(7) X(8) X(9) X(11) X(12) X(13) X(15) X(17) // roll_inst.hip: every window-height class
#define PDOG_EPI_DECL(C) extern template __global__ void dog_roll_kernel<65, false, 0, C>(const LaunchGeo, const f2 *, const f2 *);
PDOG_EPI_CLASSES(PDOG_EPI_DECL)
#undef PDOG_EPI_DECL
} // namespace pdog

namespace {

// (struct Switches: pdog_plan.hpp.)  Read once, when a tracker is created, never on the launch path.
Switches read_switches()
{
    Switches w;
    if (const char *e = std::getenv("PDOG_SCRATCH_MB")) w.scratch_cap = (size_t)std::max(1, std::atoi(e)) << 20;
    if (const char *e = std::getenv("PDOG_MAP_MB")) w.map_cap = (size_t)std::max(0, std::atoi(e)) << 20;
    if (const char *e = std::getenv("PDOG_HOST_THREADS")) w.host_threads = std::max(1, std::min(64, std::atoi(e)));
    if (const char *e = std::getenv("PDOG_INGEST_CHUNK")) w.ingest_chunk = std::max(1, std::atoi(e));
#ifdef PDOG_ABLATIONS
    auto on = [](const char *n) { return std::getenv(n) != nullptr; };
    w.host_copy = on("PDOG_HOST_COPY");
    w.host_sync = on("PDOG_HOST_SYNC");
    w.host_trace = on("PDOG_HOST_TRACE");
    w.twopass_4l = on("PDOG_TWOPASS_4L");
    w.hpass16 = on("PDOG_HPASS16");
    w.ingest_no_nt = on("PDOG_INGEST_NO_NT");
    w.ingest_trace = on("PDOG_INGEST_TRACE");
    w.fused_diag = on("PDOG_FUSED_DIAG");
    w.no_tiled = on("PDOG_NO_TILED");
    w.no_fold = on("PDOG_NO_FOLD");
    w.fold_always = on("PDOG_FOLD_ALWAYS");
    w.no_pad_skip = on("PDOG_NO_PAD_SKIP");
    w.no_prune = on("PDOG_NO_PRUNE");
    w.no_range_end = on("PDOG_NO_RANGE_END");
    w.fenced_publish = on("PDOG_FENCED_PUBLISH");
    w.no_roll_map = on("PDOG_NO_ROLL_MAP");
    w.no_host_dc = on("PDOG_NO_HOST_DC");
    w.tiled_force = on("PDOG_TILED_FORCE");
    if (const char *e = std::getenv("PDOG_TILED_SUB")) w.tiled_sub = std::max(0, std::min(96, std::atoi(e)));
    if (const char *e = std::getenv("PDOG_TILED_BATCH")) w.tiled_batch = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("PDOG_V_AFTER")) w.v_after = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("PDOG_H1_U")) w.h1_u = std::atoi(e) == 8 ? 8 : 4;
    if (const char *e = std::getenv("PDOG_HP_U")) w.hp_u = std::atoi(e) == 16 ? 16 : 8;
    if (const char *e = std::getenv("PDOG_TP_P")) {
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && (a == 5 || a == 7 || a == 9 || a == 11 || a == 13 || a == 17) && (b == 5 || b == 7 || b == 9 || b == 13)) { w.tp_ph1 = a; w.tp_php = b; }
    }
    if (const char *e = std::getenv("PDOG_FUSED_P")) {
        int a = 0, b = 0;
        if (std::sscanf(e, "%d,%d", &a, &b) == 2 && (a == 3 || a == 4 || a == 5 || a == 6 || a == 8) &&
            (b == 2 || b == 3 || b == 4 || b == 6 || b == 8)) { w.fused_pr = a; w.fused_pc = b; }
    }
    if (const char *e = std::getenv("PDOG_LDS_PAD")) w.lds_pad = std::max(0, std::atoi(e));
#endif
    return w;
}

// MaxDynamicSharedMemorySize is a per-function (per-device) attribute shared by every tracker in the
// process: only ever raise it, so that a tracker with a small window cannot shrink the limit under a
// live tracker with a large one.
int raise_lds_limit(const void *fn, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> limit;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(PDOG_E_HIP, "hipGetDevice failed");
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = limit[{dev, fn}];
    if (bytes <= cur) return PDOG_OK;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(PDOG_E_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
    cur = bytes;
    return PDOG_OK;
}

// ---- compiled kernel specialisations: the kernels of kVariantShapes' rows (pdog_plan.hpp), row for row ----
typedef void (*kernel_fn)(const LaunchGeo, const f2 *, const f2 *);
typedef void (*chain_fn)(const ChainGeo, const f2 *, const f2 *);
typedef void (*chain_table_fn)(const ChainTableGeo, const f2 *, const f2 *);
typedef void (*chain_predict_fn)(const ChainPredictGeo, const f2 *, const f2 *);
struct VariantKernels {
    int id = -1;                              // the row of kVariantShapes these kernels are the instances of
    kernel_fn fn = nullptr, fn_resp = nullptr; // the batch kernel; fn_resp also writes the dense response (parity checks).  Null: two-pass and fused rows, whose kernels are picked per launch
    kernel_fn thin = nullptr, thin_resp = nullptr; // remainder-column kernel of the roll variants (may be null)
    chain_fn chain = nullptr;                 // persistent serial-chain kernel of the roll variants
    chain_table_fn chain_table = nullptr;     // … its instance that walks a frame table
    kernel_fn fn_prune = nullptr;             // the roll instance that honours kept ranges (dog_prune.hpp)
    chain_predict_fn chain_predict = nullptr; // the chain kernel's instance that walks a table as predicted chains
};
// the instance's template arguments are the row's numbers
constexpr bool shape_is(int id, Family family, int P, int XG, int Q, int CH, int LT, int NT, bool full_set)
{
    const VariantShape *s = find_variant(id);
    return s && s->family == family && s->P == P && s->XG == XG && s->Q == Q && s->CH == CH && s->LT == LT && s->NT == NT && s->full_set == full_set;
}
template <int ID, int P, int XG, int Q, int CH, int LT, int NT>
VariantKernels ring_kernels()
{
    static_assert(shape_is(ID, Family::Ring, P, XG, Q, CH, LT, NT, false), "kVariantShapes describes another instance under this id");
    VariantKernels k;
    k.id = ID;
    k.fn = (kernel_fn)dog_window_kernel<P, XG, Q, CH, LT, NT, false>;
    k.fn_resp = (kernel_fn)dog_window_kernel<P, XG, Q, CH, LT, NT, true>;
    return k;
}
template <int LT>
VariantKernels roll_kernels()
{
    constexpr int ID = LT == 65 ? 100 : 100 + LT;
    static_assert(shape_is(ID, Family::Roll, ROLL_P, ROLL_TW / ROLL_P, ROLL_CH, ROLL_CH, LT, 64, true), "kVariantShapes describes another instance under this id");
    VariantKernels k;
    k.id = ID;
    k.fn = (kernel_fn)dog_roll_kernel<LT, false>;
    k.fn_resp = (kernel_fn)dog_roll_kernel<LT, true>;
    k.thin = (kernel_fn)dog_thin_kernel<LT, false>;
    k.thin_resp = (kernel_fn)dog_thin_kernel<LT, true>;
    k.chain = dog_chain_kernel<LT>;
    k.chain_table = dog_chain_kernel<LT, true>;
    k.fn_prune = (kernel_fn)dog_roll_kernel<LT, false, 0, -1, true>;
    k.chain_predict = dog_chain_kernel<LT, true, true>;
    return k;
}
// a row whose kernels are picked per launch (two-pass, fused), or an ablation's strip kernels alone
VariantKernels bare_kernels(int id, kernel_fn fn = nullptr, kernel_fn fn_resp = nullptr)
{
    VariantKernels k;
    k.id = id;
    k.fn = fn;
    k.fn_resp = fn_resp;
    return k;
}

const VariantKernels kVariants[] = {
    // runtime-L (any target_width)
    ring_kernels<0, 4, 8, 8, 32, 0, 256>(),
    ring_kernels<1, 8, 8, 8, 32, 0, 256>(),
    ring_kernels<2, 11, 8, 8, 32, 0, 256>(),
    // l = 65 (target_width 25, the reference default)
    ring_kernels<10, 11, 8, 16, 32, 65, 256>(),
    ring_kernels<11, 11, 8, 8, 24, 65, 256>(),
    ring_kernels<12, 8, 8, 16, 32, 65, 256>(),
    ring_kernels<13, 8, 8, 8, 32, 65, 256>(),
    ring_kernels<14, 11, 8, 8, 32, 65, 256>(),
    // rolling-accumulator kernel: one instance per kernel length of roll_lengths.def
#define PDOG_ROLL_L(LT) roll_kernels<LT>(),
#include "roll_lengths.def"
#undef PDOG_ROLL_L
    bare_kernels(kPathTwoPass), // h1_kernel_for, hpass8_kernel_for
    bare_kernels(kPathFused),   // kLatInstances
#ifdef PDOG_ABLATIONS
    bare_kernels(101, (kernel_fn)dog_roll_kernel<65, false, 1>, (kernel_fn)dog_roll_kernel<65, true>),
    bare_kernels(102, (kernel_fn)dog_roll_kernel<65, false, 2>, (kernel_fn)dog_roll_kernel<65, true>),
    bare_kernels(103, (kernel_fn)dog_roll_kernel<65, false, 3>, (kernel_fn)dog_roll_kernel<65, true>),
    bare_kernels(104, (kernel_fn)dog_roll_kernel<65, false, 12>, (kernel_fn)dog_roll_kernel<65, true>),
    bare_kernels(105, (kernel_fn)dog_roll_kernel<65, false, 15>, (kernel_fn)dog_roll_kernel<65, true>),
    bare_kernels(106, (kernel_fn)dog_roll_kernel<65, false, 0>, (kernel_fn)dog_roll_kernel<65, false, 16>),
#endif
    // l = 29 (target_width 10, the reference test default)
    ring_kernels<20, 8, 8, 4, 32, 29, 256>(),
};
static_assert(sizeof(kVariants) / sizeof(kVariants[0]) == kNumVariants, "a row of kernels per row of kVariantShapes");
// (looked up once per plan, by apply_plan; the rows stand in the same order, and each names its shape)
const VariantKernels *kernels_of(const VariantShape &s)
{
    const VariantKernels &k = kVariants[&s - kVariantShapes];
    return k.id == s.id ? &k : nullptr;
}
// The fused kernel's interior staging path keeps 32-bit byte offsets from the tile's first pixel (dog_fused.hpp, rs32): at most
// (NA - 1) * row_stride + 4 * FUSED_NT.  A fused instance only runs where its tile of NA rows fits LDS (fused_lds_bytes >=
// fused_a_bytes = NA * pitch * 4, the pitch smallest for a one-column window under the shortest kernel, l = 5), which bounds NA;
// PDOG_MAX_ROW_STRIDE (check_row_stride) bounds the other factor.  Every other family forms its addresses in 64 bits.
constexpr long long kFusedMaxRows = (long long)(kMaxLds / (4 * (size_t)fused_pitch_a(1, 5)));
static_assert(fused_a_bytes(1, 1, 5) >= 5 * fused_pitch_a(1, 5) * 4 && fused_pitch_a(1, 5) <= fusedc_pitch_a(1, 5), "the tile's LDS bytes are at least rows * pitch * 4");
static_assert(kFusedMaxRows * (long long)PDOG_MAX_ROW_STRIDE + 4 * FUSED_NT < (1LL << 32), "PDOG_MAX_ROW_STRIDE: the fused kernel's 32-bit offsets would wrap");

// ---- what a kernel family keeps between launches (what make_plan derives per family: FusedPlan, TiledPlan, pdog_plan.hpp) ----
struct TiledRun {
    DeviceBuffer<int> d_ctl; // [cap][4]: current guess (2), partial arrivals, frame flag; then the abort word
    int ctl_cap() const { return (int)(d_ctl.capacity() / 4); }
    DeviceBuffer<unsigned long long> d_slots; // [clips][3][nsub][2] tagged partials of the tiled kernel's clips (dog_tiled.hpp): two sets by frame parity + the V set
    unsigned tag = 0;        // advanced by chain_len + 1 per clip launch: a frame's tag never repeats
};
// host-batch ingest (pdog_detect_batch_host): rotating pinned staging / device tile slots, created at the first call
struct Ingest {
    static constexpr int kSlots = 3;
    PinnedBuffer<uint8_t> h_stage[kSlots];
    DeviceBuffer<uint8_t> d_tiles[kSlots];
    DeviceBuffer<int32_t> d_guess, d_out;
    PinnedBuffer<int32_t> h_out;
    hipStream_t stream = nullptr;
    hipEvent_t ev_h2d[kSlots] = {nullptr, nullptr, nullptr}, ev_used[kSlots] = {nullptr, nullptr, nullptr};
};

} // namespace

struct pdog_tracker {
    int device = 0;
    Switches sw;                   // environment switches as they were when the tracker was created
    hipEvent_t ev_switch = nullptr; // orders a new stream behind the work queued on the previous one (pdog_set_stream)
    int fh = 0, fw = 0, r1 = 0, r2 = 0, n1 = 0, n2 = 0, L = 0, fill = 0, darker = 0;
    double tw = 0, sigma = 0;
    // Everything derived from the geometry, the switches and the pinned variant (pdog_plan.hpp); apply_plan alone assigns it,
    // with the kernels of plan.shape and what the device answered for the plan: the workgroups it keeps resident of the fused
    // kernel (the grid is capped there: a workgroup walks several windows; 0: launch_fused asks) and of the tiled kernel
    Plan plan;
    const VariantKernels *kern = nullptr;
    int fused_resident = 0, tiled_resident = 0;
    DeviceBuffer<int32_t> d_chain_tmp; // [2][n_clips][2]: current guesses / step results of multi-clip chains
    pdog::StagedTable table;       // chains over a frame table (pdog_detect_chains_indexed): the validated table as the path that runs wants it
    TiledRun tiled_run;
    // two-pass path scratch
    DeviceBuffer<f2> d_V;
    // exact mode on the batch kernels of short kernels (roll / ring): batches of HARD windows (noise only, ±1-level targets:
    // every window flagged) switch to the response-map refinement like the two-pass path — 81–206 ms per 4096 windows of
    // 257×257 without it (pdog_policy.hpp)
    MapPolicy map_policy;
    unsigned win_launched = 0;               // windows handed to finishing kernels so far
    // kept ranges on the roll family's batch path (dog_prune.hpp; pdog_policy.hpp)
    PrunePolicy prune_policy;
    double K_norm = 0;                       // ‖K‖₂ of the dense kernel, rounded up (dog_kernel_norm_up)
    DeviceBuffer<unsigned long long> d_prune_stat; // [0] kept, [1] total (slot, sub-chunk) pairs, [2] the pre-pass in flight: arrivals, jobs appended, pairs kept (dog_prune_publish.hpp)
    DeviceBuffer<uint32_t> d_refine_wq;      // the second stage's weights (dog_refine_weights), rows padded as dog_prune_kernel reads them
    int last_prune_n = 0, last_prune_nstrips = 0; // the last batch that ran the pre-pass (pdog_get_prune_jobs)
    DeviceBuffer<PruneJob> d_prune_jobs;     // the kept strips of the batch in flight: the header, then up to n·nstrips entries (dog_prune.hpp, "the job list")
    int last_n = 0, last_nslots = 0;         // windows and partial slots per window of the last launch_strips batch (pdog_get_batch_maxima)
    DeviceBuffer<float> d_map; // exact mode on the two-pass path: the batch's FP32 responses, where the refinement finds its candidates
    DeviceBuffer<int> d_dc;    // [cap] DC levels, then [cap] the windows' own V (exact mode)
    DeviceBuffer<int> d_counter; // [kLowLatMax] zero between launches: delivered column-pass partials per window (low-latency two-pass)
    hipStream_t own_stream = nullptr, stream = nullptr;
    // side stream + fork/join events: the thin-remainder kernel runs beside the strips (its waves fit in
    // the registers the 2-waves-per-SIMD roll kernel leaves free) instead of after them
    hipStream_t aux_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DeviceBuffer<f2> d_taps_row, d_taps_col;
    DeviceBuffer<f2> d_taps_roll; // paired column-tap table of dog_roll.hpp
    DeviceBuffer<f2> d_fold_r;    // [n][n1 + l − 1] row-pass outputs of a folded remainder column (LaunchGeo::fold_r)
    // the kernels' partials, [n][plan.part_slots] each (ensure_capacity)
    DeviceBuffer<float> d_part_val, d_part_sec;
    DeviceBuffer<unsigned long long> d_part_mask;
    DeviceBuffer<int> d_part_idx;
    // exact mode (dog_exact.hpp): windows whose two best FP32 responses lie within 2δ are re-decided in the
    // reference's own Float64 arithmetic
    bool exact = true;
    bool exact_all = false;           // pdog_set_exact(t, 2): refine every window with an infinite threshold (tests: the whole reference computation on the device)
    std::vector<double> h_gp, h_gm;   // the two Float64 Gaussians (host copy): the error bounds follow the kernels' operation order over THESE taps
    double F_sym_int = 0, F_sym_sep = 0, F_ring = 0, F_rescan = 0; // error-bound factors per kernel family (exact_factors)
    DeviceBuffer<double> d_K64;       // dir·(g₊⊗g₊ − g₋⊗g₋), l×l column-major, Float64 (:41-43)
    DeviceBuffer<double> d_g64;       // [2][l] the two normalised Gaussians in Float64 (the refinement's separable stage)
    DeviceBuffer<RefineParams> d_rp;  // {K64, g64, dir, T64} for the kernels that refine inline
    double exact_T64 = 0.0;           // 2δ64: separable Float64 against the reference's dense Float64
    DeviceBuffer<unsigned long long> d_ref_stat;
    // host-path staging (pdog_detect_host / chain seed)
    DeviceBuffer<uint8_t> d_frame;
    DeviceBuffer<int32_t> d_small; // [0..1] guess, [2..3] result
    PinnedBuffer<Mailbox> h_pinned{hipHostMallocMapped | hipHostMallocCoherent}; // one element (pdog_mailbox.hpp)
    int32_t ticket = 0;
    DeviceBuffer<float> d_resp;
    PinnedBuffer<uint8_t> h_tile{hipHostMallocMapped}; // the functor's window tile when the kernels read it in place
    Ingest ingest;
    pdog::PeaksState peaks; // pdog_detect_peaks (pawsome_peaks.hip): its scratch, switch and counters
    pdog::GroupWalkState exclusive; // the exclusive step and walk (pawsome_exclusive.hip): their scratch, table and counters
    pdog::GroupWalkState motion;    // the motion step and walk (pawsome_motion.hip): the same
    bool motion_lds = false;        // pdog_set_tuning "motion_lds": the motion kernel stages the lists in LDS (dog_motion.hpp)
    pdog::PredictState predict;     // the predicted chain (pawsome_predict.hip): its table and counters

    // Drains and destroys the streams and events; the buffers free themselves after that.
    ~pdog_tracker()
    {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipStream_t s : {ingest.stream, aux_stream})
            if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        for (int k = 0; k < Ingest::kSlots; ++k)
            for (hipEvent_t e : {ingest.ev_h2d[k], ingest.ev_used[k]})
                if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_fork, ev_join, ev_switch})
            if (e) (void)hipEventDestroy(e);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

pdog::PeaksState *pdog::peaks_state(pdog_tracker *t)
{
    t->peaks.device = t->device;
    t->peaks.map_cap = t->sw.map_cap;
    return &t->peaks;
}

pdog::GroupWalkState *pdog::exclusive_state(pdog_tracker *t)
{
    t->exclusive.device = t->device;
    return &t->exclusive;
}

pdog::GroupWalkState *pdog::motion_state(pdog_tracker *t)
{
    t->motion.device = t->device;
    return &t->motion;
}

bool pdog::motion_lds(const pdog_tracker *t) { return t->motion_lds; }

pdog::PredictState *pdog::predict_state(pdog_tracker *t)
{
    t->predict.device = t->device;
    return &t->predict;
}

namespace {

// The instances of the latency kernels (dog_fused.hpp, dog_tiled.hpp): a row per compile-time length of lat_lengths.def, then
// the row of the runtime-length instances (L = 0).  Per kernel: the plain instance, the one that also writes the response
// map, and the one that walks a frame table (no response map: a chain has none).
typedef void (*fused_fn_t)(const FusedGeo, const f2 *, const f2 *);
typedef void (*fused_table_fn_t)(const FusedTableGeo, const f2 *, const f2 *);
typedef void (*fused_predict_fn_t)(const FusedPredictGeo, const f2 *, const f2 *);
typedef void (*tiled_fn_t)(const TiledGeo, const f2 *, const f2 *);
enum { kLatPlain, kLatResp, kLatTable };
struct LatInstances { int L; const void *fused[3], *tiled[3]; fused_predict_fn_t fused_predict; }; // fused_predict: the table instance of the predicted chain
#define PDOG_LAT_L(LT)                                                                                                                \
    { LT, {(const void *)dog_fused_kernel<false, 0, LT>, (const void *)dog_fused_kernel<true, 0, LT>, (const void *)dog_fused_kernel<false, 0, LT, true>}, \
          {(const void *)dog_tiled_kernel<false, LT>, (const void *)dog_tiled_kernel<true, LT>, (const void *)dog_tiled_kernel<false, LT, true>}, \
          dog_fused_kernel<false, 0, LT, true, true> },
const LatInstances kLatInstances[] = {
#include "lat_lengths.def"
    PDOG_LAT_L(0)
};
#undef PDOG_LAT_L
// compile_time: the row of the tracker's own length where there is one
const LatInstances &lat_instances(int L, bool compile_time)
{
    const LatInstances &runtime_length = *(std::end(kLatInstances) - 1);
    if (!compile_time) return runtime_length;
    for (const LatInstances &row : kLatInstances)
        if (row.L == L) return row;
    return runtime_length;
}
const LatInstances &fused_instances(const pdog_tracker *t) { return lat_instances(t->L, t->plan.fused.c); }
const LatInstances &tiled_instances(const pdog_tracker *t) { return lat_instances(t->L, t->plan.tiled.c); }
int raise_lds_limits(const void *const (&fns)[3], size_t bytes)
{
    for (const void *fn : fns)
        if (int rc = raise_lds_limit(fn, bytes)) return rc;
    return PDOG_OK;
}

// (the two-pass kernels' LDS row pitches: twopass_pitch_q, twopass_pitch, dog_layout.hpp; their outputs per task: pick_h1_outputs,
// pick_hpass_outputs, pdog_plan.hpp)
typedef void (*tp_fn)(TwoPassGeo, const f2 *);
// flush: the blocked-accumulation instances (dog_twopass.hpp), for kernel lengths from TWOPASS_FLUSH_L on.  The product build
// holds the default block sizes only (row pass 4 taps, column pass 8); the diagnostic build adds the 8- / 16-tap instances.
tp_fn h1_kernel_for(int P, bool dcin, int U, bool flush)
{
#define PDOG_H1(PP, UU) (flush ? (dcin ? (tp_fn)dog_h1_kernel<PP, UU, true, true> : (tp_fn)dog_h1_kernel<PP, UU, false, true>) \
                               : (dcin ? (tp_fn)dog_h1_kernel<PP, UU, true, false> : (tp_fn)dog_h1_kernel<PP, UU, false, false>))
#ifdef PDOG_ABLATIONS
    if (U == 8) {
        switch (P) {
        case 5: return PDOG_H1(5, 8);
        case 7: return PDOG_H1(7, 8);
        case 9: return PDOG_H1(9, 8);
        case 11: return PDOG_H1(11, 8);
        case 17: return PDOG_H1(17, 8);
        default: return PDOG_H1(13, 8);
        }
    }
#endif
    (void)U;
    switch (P) {
    case 9: return PDOG_H1(9, 4);
    case 17: return PDOG_H1(17, 4);
    case 11: return PDOG_H1(11, 4);
    default: return PDOG_H1(13, 4);
    }
#undef PDOG_H1
}
tp_fn hpass8_kernel_for(int P, bool resp, bool fin, int U, bool flush)
{
#define PDOG_HP8F(PP, UU, FF) (fin ? (resp ? (tp_fn)dog_hpass_kernel<PP, UU, true, 8, true, FF> : (tp_fn)dog_hpass_kernel<PP, UU, false, 8, true, FF>) \
                                   : (resp ? (tp_fn)dog_hpass_kernel<PP, UU, true, 8, false, FF> : (tp_fn)dog_hpass_kernel<PP, UU, false, 8, false, FF>))
#define PDOG_HP8(PP, UU) (flush ? PDOG_HP8F(PP, UU, true) : PDOG_HP8F(PP, UU, false))
#ifdef PDOG_ABLATIONS
    if (U == 16) {
        switch (P) {
        case 5: return PDOG_HP8(5, 16);
        case 9: return PDOG_HP8(9, 16);
        default: return PDOG_HP8(7, 16);
        }
    }
#endif
    (void)U;
    switch (P) {
    case 5: return PDOG_HP8(5, 8);
    case 9: return PDOG_HP8(9, 8);
    case 13: return PDOG_HP8(13, 8);
    default: return PDOG_HP8(7, 8);
    }
#undef PDOG_HP8
#undef PDOG_HP8F
}
tp_fn h1_kernel(const pdog_tracker *t, bool dcin) { return h1_kernel_for(t->plan.tp_ph1, dcin, t->sw.h1_u, t->L >= TWOPASS_FLUSH_L); }
tp_fn hpass8_kernel(const pdog_tracker *t, bool resp, bool fin) { return hpass8_kernel_for(t->plan.tp_php, resp, fin, t->sw.hp_u, t->L >= TWOPASS_FLUSH_L); }
int ensure_capacity(pdog_tracker *t, int n);
ExactCtl exact_ctl(const pdog_tracker *t, KernelFamily fam);

// What a launch works on.  A caller sets the fields it uses; the rest keep these defaults.
struct Request {
    const uint8_t *frames = nullptr;
    int64_t frame_stride = 0, row_stride = 0;
    const int32_t *frame_index = nullptr;  // may stay null: window b looks at frame b
    ClipTable table{nullptr, nullptr, 0};  // chains over a frame table (index non-null): the kernels that walk a clip read it themselves
    const int32_t *guesses = nullptr;      // n x 2 (chains: the clips' start guesses)
    int n = 0;                             // windows, or clips of chain_len frames
    int chain_len = 1;
    int32_t *out_ij = nullptr;
    float *out_resp = nullptr;
    int fh = 0, fw = 0;                    // frame size as the kernels see it (0: the tracker's; the packed window tiles of the host paths differ)
    int32_t *done_flag = nullptr;          // published with done_value after the answer (single-window paths), or, with
    int32_t done_value = 0;                // `progress`, with k + 1 after frame k of a chain
    bool progress = false;
    int dc_host = -1;                      // the window's DC level where the host already sampled it
    const PredictCtl *predict = nullptr;   // chains over a table walked as predicted chains (launch_fused, launch_persistent)
};

// The LaunchGeo fields every path fills the same way; everything else is zero.  A path then sets what it uses: the
// partial arrays, ex, nstrips / nslots / nblocks and its own geometry.
LaunchGeo base_geo(const pdog_tracker *t, const Request &req)
{
    LaunchGeo g;
    std::memset(&g, 0, sizeof g);
    g.frames = req.frames;
    g.frame_stride = req.frame_stride;
    g.row_stride = req.row_stride;
    g.frame_index = req.frame_index;
    g.guesses = req.guesses;
    g.resp = req.out_resp;
    g.fh = req.fh ? req.fh : t->fh; g.fw = req.fw ? req.fw : t->fw;
    g.r1 = t->r1; g.r2 = t->r2; g.n1 = t->n1; g.n2 = t->n2;
    g.L = t->L; g.fill = t->fill; g.n = req.n;
    g.no_pad_skip = t->sw.no_pad_skip;
    return g;
}
void use_partials(const pdog_tracker *t, LaunchGeo &g)
{
    g.part_val = t->d_part_val.get();
    g.part_idx = t->d_part_idx.get();
    g.part_sec = t->d_part_sec.get();
    g.part_mask = t->d_part_mask.get();
}

// req.n windows (chain_len = 1: independent; ordinary launch) or req.n clips of chain_len frames (cooperative launch: the
// workgroups of a clip wait for each other's partials frame by frame).  *launched = false: not taken, the caller goes on.
int launch_tiled(pdog_tracker *t, const Request &req, bool *launched)
{
    *launched = false;
    const int n = req.n, chain_len = req.chain_len;
    if (!tiled_serves(t->plan, t->tiled_resident, n, chain_len)) return PDOG_OK;
    const TiledPlan &p = t->plan.tiled;
    TiledRun &run = t->tiled_run;
    const int nsub = p.ns1 * p.ns2;
    if (int rc = ensure_capacity(t, n)) return rc;
    // the kernel leaves its counters at zero; the last word is the abort word
    if (int rc = run.d_ctl.reserve(4 * (size_t)n + 1, &t->stream, true)) return rc;
    TiledTableGeo tg; // (an ordinary launch takes its TiledGeo part)
    std::memset(&tg, 0, sizeof tg);
    LaunchGeo &g = tg.g;
    g = base_geo(t, req);
    use_partials(t, g);
    g.ex = exact_ctl(t, kFamFused);
    g.nstrips = nsub; g.nslots = nsub; g.nblocks = n * nsub;
    tg.NA = t->n1 + t->L - 1;
    tg.TWin = t->n2 + t->L - 1;
    tg.sn1 = p.sn1; tg.sn2 = p.sn2; tg.ns1 = p.ns1; tg.ns2 = p.ns2;
    tg.pitchA = p.pitchA;
    tg.pitchV = p.pitchV;
    tg.cshift = p.cshift;
    tg.pr = p.pr;
    tg.pc = p.pc;
    tg.chain_len = chain_len;
    tg.out_ij = req.out_ij;
    tg.done_flag = req.done_flag;
    tg.done_value = req.done_value;
    tg.progress = req.progress ? 1 : 0;
    tg.rp = t->exact ? t->d_rp.get() : nullptr;
    tg.ref_cbw = p.ref_cbw;
    tg.ref_rows = p.ref_rows;
    tg.dc_host = req.dc_host;
    tg.cur = run.d_ctl.get();
    tg.sync = reinterpret_cast<unsigned *>(run.d_ctl.get() + 2 * (size_t)run.ctl_cap());
    tg.abort = reinterpret_cast<unsigned *>(run.d_ctl.get() + 4 * (size_t)run.ctl_cap());
    tg.fault_inject = t->sw.fault_inject ? 1 : 0;
    tg.tab = req.table;
    tg.slots = nullptr;
    tg.tag_base = 0;
    if (chain_len > 1) {
        if (int rc = run.d_slots.reserve((size_t)n * 3 * nsub * 2, &t->stream, true)) return rc; // zeroed: tag 0 is never a frame's
        tg.slots = run.d_slots.get();
        tg.tag_base = run.tag;
        run.tag += (unsigned)chain_len + 1u;
    }
    const void *fn = tiled_instances(t).tiled[req.table.index ? kLatTable : req.out_resp ? kLatResp : kLatPlain];
    const f2 *tr = t->d_taps_row.get(), *tc = t->d_taps_col.get();
    if (chain_len > 1) {
        void *args[] = {(void *)&tg, (void *)&tr, (void *)&tc};
        const hipError_t e = hipLaunchCooperativeKernel(fn, dim3(n * nsub), dim3(FUSED_NT), args, (unsigned)p.lds, t->stream);
        if (e != hipSuccess) { (void)hipGetLastError(); return PDOG_OK; } // refused: the caller's other paths
    } else {
        hipLaunchKernelGGL((tiled_fn_t)fn, dim3(n * nsub), dim3(FUSED_NT), p.lds, t->stream, static_cast<const TiledGeo &>(tg), tr, tc);
        HIP_TRY(hipGetLastError());
    }
    *launched = true;
    return PDOG_OK;
}

Geometry geometry_of(const pdog_tracker *t) { return Geometry{t->fh, t->fw, t->n1, t->n2, t->L}; }

// Makes `p` (make_plan's, for the switches `sw`) the tracker's plan: raises the LDS limit of every kernel the plan may launch
// — they only ever rise — and asks the device how many workgroups of the tiled kernel it keeps resident.  Only then are the
// plan, the switches it was made for and the device's answers assigned: a refusal leaves the tracker as it was.
int apply_plan(pdog_tracker *t, const Switches &sw, const Plan &p)
{
    const VariantKernels *k = kernels_of(*p.shape);
    if (!k) return fail(PDOG_E_ARG, "kVariants and kVariantShapes name different variants in a row");
    const bool flush = t->L >= TWOPASS_FLUSH_L;
    if (p.lds.fused)
        if (int rc = raise_lds_limits(lat_instances(t->L, p.fused.c).fused, p.lds.fused)) return rc;
    int tiled_resident = 0;
    if (p.lds.tiled) {
        const LatInstances &tiled = lat_instances(t->L, p.tiled.c);
        if (int rc = raise_lds_limits(tiled.tiled, p.lds.tiled)) return rc;
        int per_cu = 0, cus = 0, coop = 0; // chains need every workgroup of a clip resident at once: a cooperative launch, if the device has them
        if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, t->device) == hipSuccess && coop &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tiled.tiled[kLatPlain], FUSED_NT, p.lds.tiled) == hipSuccess && per_cu >= 1 &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) == hipSuccess)
            tiled_resident = per_cu * cus;
    }
    if (p.lds.tp_col16) { // (the three two-pass numbers are set together: small_twopass)
        for (const void *f : {(const void *)dog_hpass_kernel<13, 16, false>, (const void *)dog_hpass_kernel<13, 16, true>}) {
            if (int rc = raise_lds_limit(f, p.lds.tp_col16)) return rc;
        }
        for (bool resp : {false, true})
            for (bool fin : {false, true})
                if (int rc = raise_lds_limit((const void *)hpass8_kernel_for(p.tp_php, resp, fin, sw.hp_u, flush), p.lds.tp_col8)) return rc;
        for (bool dcin : {false, true})
            if (int rc = raise_lds_limit((const void *)h1_kernel_for(p.tp_ph1, dcin, sw.h1_u, flush), p.lds.tp_row)) return rc;
    }
    if (p.lds.thin)
        for (kernel_fn f : {k->thin, k->thin_resp}) {
            if (int rc = raise_lds_limit((const void *)f, p.lds.thin)) return rc;
        }
    if (p.lds.batch)
        for (kernel_fn f : {k->fn, k->fn_resp}) {
            if (int rc = raise_lds_limit((const void *)f, p.lds.batch)) return rc;
        }
    if (int rc = raise_lds_limit((const void *)dog_finish_kernel, p.lds.finish)) return rc;
    // (the count of resident workgroups stands while the instance and its LDS do; launch_fused asks again otherwise)
    if (!(p.fused.c == t->plan.fused.c && p.fused.lds == t->plan.fused.lds)) t->fused_resident = 0;
    t->tiled_resident = tiled_resident;
    t->kern = k;
    t->sw = sw;
    t->plan = p;
    return PDOG_OK;
}

// make_plan, then apply_plan: what pdog_create, pdog_set_variant and the pdog_set_tuning keys that change an input of the plan do.
int replan(pdog_tracker *t, const Switches &sw, int forced)
{
    Plan p;
    std::string why;
    if (int rc = make_plan(geometry_of(t), sw, forced, &p, &why)) return fail(rc, why);
    return apply_plan(t, sw, p);
}

// Room for the partials of n windows.  Growing drains the tracker's stream first, once (the four arrays grow together;
// a failure leaves the later ones empty, so the smallest capacity decides).
int ensure_capacity(pdog_tracker *t, int n)
{
    const size_t need = (size_t)n * t->plan.part_slots;
    if (need <= std::min({t->d_part_val.capacity(), t->d_part_sec.capacity(), t->d_part_idx.capacity(), t->d_part_mask.capacity()})) return PDOG_OK;
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (int rc = t->d_part_val.reserve(need, nullptr)) return rc;
    if (int rc = t->d_part_sec.reserve(need, nullptr)) return rc;
    if (int rc = t->d_part_idx.reserve(need, nullptr)) return rc;
    return t->d_part_mask.reserve(need, nullptr);
}

// ---- exact mode's FP32 error bounds per kernel family (exact_factors, pdog_math.cpp; twopass_factor and exact_thresholds, pdog_plan.hpp) ----
ExactCtl exact_ctl(const pdog_tracker *t, KernelFamily fam)
{
    ExactCtl x;
    x.stat = t->d_ref_stat.get();
    x.range_err = t->h_pinned.device() ? &t->h_pinned.device()->kernel : nullptr;
    const double F = family_factor(fam, t->F_sym_int, t->F_sym_sep, t->F_ring, t->plan, t->sw, t->h_gp, t->h_gm);
    const ExactThresholds th = exact_thresholds(F, t->F_rescan, t->exact_all);
    x.T = th.T;
    x.T_rescan = th.T_rescan;
    return x;
}

// The last kernel of a batch (dog_exact.hpp): strip combine, index map and clamp (:58-61) for every window — one
// workgroup each — and the refinement of exact mode for the windows that need it.  `slot_w`, `slot_last`: how the
// partial slots the main kernels wrote map to window columns (the refinement only rescans column blocks whose slot
// can hold a near-maximal pixel).  With done_flag set the kernel also publishes the host functor's ticket with
// window 0's final answer.
struct Finish {
    int slot_w = 0, slot_last = 1 << 30;
    bool use_mask = false;
    const float *map = nullptr; // the batch's FP32 responses (exact mode reads its candidates off them), or null
    const int *vmax = nullptr;  // the windows' own max |pixel − dc|, where the row pass collected it
    int32_t *out_ij = nullptr, *done_flag = nullptr;
    int32_t done_value = 0;
};
int launch_finish(pdog_tracker *t, const LaunchGeo &g, const Finish &f)
{
    FinishGeo fg;
    fg.g = g;
    fg.map = t->exact ? f.map : nullptr;
    fg.vmax = f.vmax;
    fg.K64 = t->exact ? t->d_K64.get() : nullptr;
    fg.g64 = t->d_g64.get();
    fg.dir = t->darker ? -1.0 : 1.0;
    fg.T64 = t->exact_T64;
    fg.cbw = t->plan.ref_cbw;
    fg.tile_rows = t->plan.ref_rows;
    fg.slot_w = f.slot_w;
    fg.slot_last = f.slot_last;
    fg.nmain = g.nslots - g.nthin;
    fg.thin_x0 = g.thin_x0;
    fg.use_mask = f.use_mask ? 1 : 0;
    fg.v_after = t->sw.v_after;
    fg.out_ij = f.out_ij;
    fg.done_flag = f.done_flag;
    fg.done_value = f.done_value;
    fg.seq_windows = (int)t->win_launched;
    t->win_launched += (unsigned)g.n;
    size_t lds = t->exact ? refine_lds_bytes(t->n1, t->L, t->plan.ref_cbw, t->plan.ref_rows) : 0;
    if (g.fold_r) { // the folded remainder column's R values, one slice per wave (a window each)
        lds = std::max(lds, (size_t)FINISH_WPB * (t->n1 + t->L - 1 + FOLD_GO) * sizeof(f2));
        if (int rc = raise_lds_limit((const void *)dog_finish_kernel, lds)) return rc;
    }
    hipLaunchKernelGGL(dog_finish_kernel, dim3((g.n + FINISH_WPB - 1) / FINISH_WPB), dim3(REFINE_NT), lds, t->stream, fg, (const f2 *)t->d_taps_row.get(),
                       (const f2 *)t->d_taps_col.get());
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

// One workgroup per window (chain_len = 1) or per clip (chain_len frames, frame k > 0 starts at frame k−1's answer).
int launch_fused(pdog_tracker *t, const Request &req)
{
    const int n = req.n, chain_len = req.chain_len;
    const FusedPlan &p = t->plan.fused;
    FusedPredictGeo fg; // (a launch without a table takes its FusedGeo part, one without prediction its FusedTableGeo part)
    fg.pred = req.predict ? *req.predict : PredictCtl{0.f, 0, nullptr, nullptr};
    fg.tab = req.table;
    fg.g = base_geo(t, req);
    LaunchGeo &g = fg.g;
    g.nstrips = 1; g.nslots = 1; g.nblocks = n;
    fg.NA = t->n1 + t->L - 1;
    fg.TWin = t->n2 + t->L - 1;
    fg.pitchA = p.pitchA;
    fg.pitchV = p.pitchV;
    fg.cshift = p.cshift;
    fg.pr = p.pr;
    fg.pc = p.pc;
    fg.chain_len = chain_len;
    fg.out_ij = req.out_ij;
    fg.done_flag = req.done_flag;
    fg.done_value = req.done_value;
    fg.progress = req.progress ? 1 : 0;
    fg.rp = t->exact ? t->d_rp.get() : nullptr;
    fg.ref_cbw = p.ref_cbw;
    fg.ref_rows = p.ref_rows;
    fg.dc_host = req.dc_host;
    g.ex = exact_ctl(t, kFamFused);
    const size_t lds = p.lds;
    fused_fn_t fn = (fused_fn_t)fused_instances(t).fused[req.out_resp ? kLatResp : kLatPlain];
    const f2 *tr = t->d_taps_row.get(), *tc = t->d_taps_col.get();
#ifdef PDOG_ABLATIONS
    if (req.out_resp && t->sw.fused_diag) { // phase stamps instead of the response (tools/fused_phases.py)
        fn = (p.c && t->L == 65) ? (fused_fn_t)dog_fused_kernel<true, 1, 65> : (fused_fn_t)dog_fused_kernel<true, 1>;
        if (int rc = raise_lds_limit((const void *)fn, lds)) return rc;
    }
    if (!req.out_resp && t->sw.fused_diag && chain_len > 8) { // a chain's steady state: stamps of every frame, the median printed per phase
        DeviceBuffer<float> d_st;
        std::vector<float> st(16 * (size_t)chain_len + 64);
        if (int rc = d_st.reserve(st.size(), nullptr)) return rc;
        fg.g.resp = d_st.get();
        fn = (p.c && t->L == 65) ? (fused_fn_t)dog_fused_kernel<true, 1, 65> : (fused_fn_t)dog_fused_kernel<true, 1>;
        if (int rc = raise_lds_limit((const void *)fn, lds)) return rc;
        hipLaunchKernelGGL(fn, dim3(n), dim3(FUSED_NT), lds, t->stream, fg, tr, tc);
        HIP_TRY(hipStreamSynchronize(t->stream));
        HIP_TRY(hipMemcpy(st.data(), d_st.get(), st.size() * sizeof(float), hipMemcpyDeviceToHost));
        static const int order[7] = {0, 4, 1, 2, 5, 6, 3};
        static const char *names[7] = {"samples", "barrier", "staged", "row pass", "col+peak(w0)", "barrier", "finalize"};
        std::fprintf(stderr, "fused chain phases (median over frames 8.., 100 MHz ticks → us):");
        int prev = -1;
        for (int q = 0; q < 7; ++q) {
            std::vector<float> d;
            for (int k = 8; k < chain_len; ++k) d.push_back(st[16 * k + 8 + order[q]] - (prev < 0 ? 0.f : st[16 * k + 8 + prev]));
            std::sort(d.begin(), d.end());
            std::fprintf(stderr, " %s %.2f;", names[q], d[d.size() / 2] / 100.0);
            prev = order[q];
        }
        std::fprintf(stderr, "\n");
        static const char *wn[4] = {"row pass done", "col tasks done", "wave peak done", "staged"};
        for (int i : {3, 0, 1, 2}) {
            std::fprintf(stderr, "  frame 20, cycles since frame start, %s, waves 0-15:", wn[i]);
            for (int w = 0; w < 16; ++w) std::fprintf(stderr, " %.0f", st[16 * (size_t)chain_len + 16 * i + w]);
            std::fprintf(stderr, "\n");
        }
        return PDOG_OK;
    }
#endif
    if (t->fused_resident <= 0) { // once per plan
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)fn, FUSED_NT, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus < 1) cus = 256;
        t->fused_resident = per_cu * cus;
    }
    const dim3 grid(std::min(n, t->fused_resident));
    if (req.predict) {
        const fused_predict_fn_t fp = fused_instances(t).fused_predict;
        if (int rc = raise_lds_limit((const void *)fp, lds)) return rc; // (here, not in apply_plan: a tracker that never predicts sets nothing up)
        hipLaunchKernelGGL(fp, grid, dim3(FUSED_NT), lds, t->stream, fg, tr, tc);
    } else if (req.table.index)
        hipLaunchKernelGGL((fused_table_fn_t)fused_instances(t).fused[kLatTable], grid, dim3(FUSED_NT), lds, t->stream, static_cast<const FusedTableGeo &>(fg), tr, tc);
    else hipLaunchKernelGGL(fn, grid, dim3(FUSED_NT), lds, t->stream, static_cast<const FusedGeo &>(fg), tr, tc);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

// The kernels of g write their FP32 responses to the tracker's map, where exact mode's refinement reads its candidates
// instead of recomputing them — unless g.n windows exceed PDOG_MAP_MB: g.resp then stays null.
int reserve_response_map(pdog_tracker *t, LaunchGeo &g)
{
    const size_t count = (size_t)g.n * t->n1 * t->n2;
    if (sizeof(float) * count > t->sw.map_cap) return PDOG_OK;
    if (int rc = t->d_map.reserve(count, &t->stream)) return rc;
    g.resp = t->d_map.get();
    return PDOG_OK;
}

// Small batches: fewer than ≈1000 strip-waves cannot fill 256 CUs × 8 waves; the two-pass kernels (dozens of workgroups per
// window, the intermediate in HBM) can.  `g` arrives as launch_detect filled it.
int launch_twopass(pdog_tracker *t, const Request &req, LaunchGeo g, bool *ticket_armed)
{
    const int n = req.n;
    const int hr = t->sw.hpass16 ? HP_ROWS : 8; // 8 RT rows per workgroup (32 KB LDS → 4 workgroups per CU): +3 % on cfg5 vs 16; env = tuning switch
    const int tp_slots = (t->n2 + hr - 1) / hr; // partial slots = hr-column blocks
    g.nstrips = tp_slots;
    g.nslots = tp_slots;
    g.nthin = 0;
    g.ex = exact_ctl(t, hr == 8 ? kFamTwoPass8 : kFamTwoPass16); // the two-pass kernels' own bound (blocked accumulation)
    // exact mode: the column pass also writes its responses (4 B per pixel), so that a window that needs the
    // refinement — every window, at the σ this path serves — reads its candidates off the map instead of recomputing them
    if (t->exact && !g.resp)
        if (int rc = reserve_response_map(t, g)) return rc;
    const bool want_resp = g.resp != nullptr;
    TwoPassGeo tg;
    tg.TWin = t->n2 + t->L - 1;
    tg.NA = t->n1 + t->L - 1;
    tg.h1blocks_per_win = (tg.NA + HP_ROWS - 1) / HP_ROWS;
    tg.hblocks_per_win = tp_slots;
    tg.pitchA = twopass_pitch_q(t->n2, t->L, 16 * t->plan.tp_ph1);
    tg.pitchV = hr == 8 ? twopass_pitch_q(t->n1, t->L, 32 * t->plan.tp_php) : twopass_pitch(t->n1, t->L, hr);
    const size_t per_win = (size_t)t->n2 * tg.NA; // f2 elements of HBM scratch for the transposed intermediate; larger batches go in chunks
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n, t->sw.scratch_cap / (per_win * sizeof(f2))));
    if (int rc = t->d_V.reserve(per_win * chunk, &t->stream)) return rc;
    if (int rc = t->d_dc.reserve(2 * (size_t)n, &t->stream)) return rc; // [cap] DC levels, then [cap] the windows' own V (exact mode)
    tg.g = g;
    tg.RT = t->d_V.get();
    tg.dc = t->d_dc.get();
    tg.vmax = nullptr;
    tg.counter = nullptr;
    tg.out_ij = req.out_ij;
    tg.done_flag = nullptr;
    tg.done_value = 0;
    tg.win0 = 0;
    const size_t l1 = (size_t)HP_ROWS * tg.pitchA * sizeof(float);
    const size_t l2 = (size_t)hr * tg.pitchV * sizeof(f2);
    const f2 *tr = t->d_taps_row.get(), *tc = t->d_taps_col.get();
    Finish fin;
    fin.slot_w = hr;
    fin.map = g.resp;
    fin.out_ij = req.out_ij;
    // A handful of windows (single-clip chains and functor calls with windows too large for the fused kernel,
    // the auto-detect pass): launches are what such a batch costs, so the DC level is derived inside the row pass
    // and the last column-pass workgroup of a window combines its partials — two launches instead of four.
    // (exact mode: the partials are combined by dog_finish_kernel, which also refines and publishes the ticket —
    // three launches; without it the last column-pass workgroup of a window combines them itself — two)
    constexpr int kLowLatMax = 16; // measured crossover (257×257 and 271×481 windows): 2 launches win up to 16 windows, 4 launches beyond
    if (n <= kLowLatMax && n <= chunk && hr == 8 && !t->sw.twopass_4l) {
        if (!t->exact) {
            if (!t->d_counter.get()) {
                if (int rc = t->d_counter.reserve(kLowLatMax, nullptr)) return rc;
                HIP_TRY(hipMemsetAsync(t->d_counter.get(), 0, sizeof(int) * kLowLatMax, t->stream));
            }
            tg.counter = t->d_counter.get();
            tg.done_flag = req.done_flag;
            tg.done_value = req.done_value;
        }
        if (ticket_armed) *ticket_armed = req.done_flag != nullptr;
        hipLaunchKernelGGL(h1_kernel(t, true), dim3(n * tg.h1blocks_per_win), dim3(256), l1, t->stream, tg, tr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hpass8_kernel(t, want_resp, !t->exact), dim3(n * tg.hblocks_per_win), dim3(256), l2, t->stream, tg, tc);
        HIP_TRY(hipGetLastError());
        if (!t->exact) return PDOG_OK;
        fin.done_flag = req.done_flag;
        fin.done_value = req.done_value;
        return launch_finish(t, g, fin);
    }
    // exact mode: the row pass collects each window's own V = max |pixel − dc| (the error bound is proportional to it) and the
    // finishing kernel flags with it; the two-pass kernels' own bound (blocked accumulation) replaces the one-chain bound
    if (t->exact && !t->exact_all && hr == 8 && t->L >= TWOPASS_FLUSH_L) tg.vmax = t->d_dc.get() + t->d_dc.capacity() / 2; // (the blocked-accumulation instances collect it)
    hipLaunchKernelGGL(dog_dc_kernel, dim3(n), dim3(64), 0, t->stream, g, t->d_dc.get(), tg.vmax);
    HIP_TRY(hipGetLastError());
    const tp_fn h1 = h1_kernel(t, false);
    const tp_fn hp = hr == 8 ? hpass8_kernel(t, want_resp, false) : want_resp ? (tp_fn)dog_hpass_kernel<13, 16, true> : (tp_fn)dog_hpass_kernel<13, 16, false>;
    for (int w0 = 0; w0 < n; w0 += chunk) {
        const int nw = std::min(chunk, n - w0);
        tg.win0 = w0;
        hipLaunchKernelGGL(h1, dim3(nw * tg.h1blocks_per_win), dim3(256), l1, t->stream, tg, tr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hp, dim3(nw * tg.hblocks_per_win), dim3(256), l2, t->stream, tg, tc);
        HIP_TRY(hipGetLastError());
    }
    fin.vmax = tg.vmax;
    return launch_finish(t, g, fin);
}

// ---- pruning policy (dog_prune.hpp; PrunePolicy, pdog_policy.hpp) ----
// Consecutive entries of the job list that go to one XCD (LaunchGeo::prune, prune_job_index): 1 deals the list out entry by
// entry.
#ifndef PDOG_PRUNE_XCD_GROUP
#define PDOG_PRUNE_XCD_GROUP 1
#endif
constexpr int kPruneXcdGroup = PDOG_PRUNE_XCD_GROUP;
static_assert(kPruneXcdGroup >= 1 && (kPruneXcdGroup & (kPruneXcdGroup - 1)) == 0, "a power of two");
constexpr size_t kPruneMaxLds = 64 * 1024; // (the pre-pass's dynamic LDS without raising the kernel's limit; larger windows stay dense)
bool use_pruning(pdog_tracker *t, bool want_resp, int nslots)
{
    // dense: the response-writing instances, pdog_set_exact(t, 2) (infinite thresholds), "no_prune", every other kernel family
    // (ahead of the policy: a launch that cannot prune is no observation)
    if (!t->kern->fn_prune || want_resp || t->exact_all || t->sw.no_prune || prune_lds(t->n1, t->n2, t->L, nslots).total > kPruneMaxLds) return false;
    return t->prune_policy.decide(__atomic_load_n(&t->h_pinned.get()->prune_pub, __ATOMIC_ACQUIRE));
}

// The tracker's batch kernel: one wave (roll) or workgroup (ring) per strip of every window, the thin remainder columns beside
// them, then the finishing kernel.  `g` arrives as launch_detect filled it.
int launch_strips(pdog_tracker *t, const Request &req, LaunchGeo g)
{
    const VariantShape &v = *t->plan.shape;
    const VariantKernels &k = *t->kern;
    const Plan &plan = t->plan;
    const bool roll = v.family == Family::Roll;
    const int n = req.n;
    int grid = round_up(g.nblocks, 8);
    // Exact mode: batches whose predecessors flagged many of their windows write their responses, and the finishing kernel
    // reads its candidates off that map (MapPolicy, pdog_policy.hpp).  The counts come through host-coherent memory: nothing
    // here waits for the GPU.
    if (t->exact && !t->exact_all) {
        const KernelWords &kw = t->h_pinned.get()->kernel;
        const uint32_t flagged = __atomic_load_n(&kw.flagged, __ATOMIC_ACQUIRE);
        t->map_policy.observe(flagged, __atomic_load_n(&kw.finished, __ATOMIC_ACQUIRE));
        if (!g.resp && t->map_policy.on() && !t->sw.no_roll_map)
            if (int rc = reserve_response_map(t, g)) return rc;
    }
    const bool want_resp = g.resp != nullptr;
    // A single remainder column (widths 64·k + 1: 257, 513, …) can be FOLDED into the last strip: its row pass rides in that
    // strip (a ninth output in the last lane group), its R values go through d_fold_r to the finishing kernel, which runs the
    // column's column pass — no second kernel re-reading a 65-column patch per window, no side stream.  The response-writing
    // instances (parity checks, the response-map refinement) and the other kernel lengths keep dog_thin_kernel.
    const int NA = t->n1 + t->L - 1;
    const size_t fold_wave_lds = (size_t)(NA + FOLD_GO) * sizeof(f2);
    // Measured (same-session A/B against dog_thin_kernel beside the strips): the folded strip is the slowest of its window (+6 %:
    // 49 packed instructions per sub-chunk) and the finishing kernel gains the column pass — +2.7 % per cfg3 step (4 strips per
    // window), −0.8 % per cfg4 step (8 strips).  A variant that kept the R column in the strip's LDS and ran the column pass in
    // the strip's own wave cost a wave per SIMD (12.9 KB per wave) and +5 %.  So: folded from 8 strips per window on.
    const bool prune = use_pruning(t, want_resp, g.nslots);
    const bool fold = roll && roll_folds(v.LT) && plan.nthin == 1 && !want_resp && !prune && !t->sw.no_fold && (plan.nstrips >= 8 || t->sw.fold_always) &&
                      (size_t)FINISH_WPB * fold_wave_lds <= kMaxLds - 1024;
    const f2 *tr = t->d_taps_row.get(), *tc = t->d_taps_col.get();
    if (prune) { // the pre-pass leaves every slot's kept range in part_mask, ahead of the strips and (through the fork) the thin kernel
        PruneGeo pg;
        pg.g = g;
        // (decided per launch: a batch whose arrivals, jobs or kept pairs could overflow their fields of the packed word keeps
        // the fenced publish; dog_prune_publish.hpp)
        const int nsub = (t->n1 + t->L - 1 + ROLL_CH - 1) / ROLL_CH;
        pg.g.prune = (t->sw.fenced_publish || !pp_fits(n, g.nstrips, g.nslots, nsub)) ? PRUNE_FENCED_PUBLISH : 0;
        pg.kinv = 255.0 / t->K_norm;
        pg.tmax = std::max(g.ex.T, g.ex.T_rescan);
        pg.darker = t->darker;
        pg.stat = t->d_prune_stat.get();
        pg.host = &t->h_pinned.device()->prune_pub;
        if (int rc = t->d_prune_jobs.reserve((size_t)g.nblocks + 1, &t->stream)) return rc;
        pg.jobs = t->d_prune_jobs.get();
        // the second stage, where its roots fit the pre-pass's LDS beside the rest (else the first stage alone, not a dense batch)
        const bool refine = !t->sw.no_refine && prune_span(t->L) <= PRUNE_REFINE_MAX_SPAN && prune_lds(t->n1, t->n2, t->L, g.nslots, true).total <= kPruneMaxLds;
        pg.wq = refine ? t->d_refine_wq.get() : nullptr;
        hipLaunchKernelGGL(t->fw < 8 ? dog_prune_kernel<true> : dog_prune_kernel<false>, dim3(n), dim3(PRUNE_NT), prune_lds(t->n1, t->n2, t->L, g.nslots, refine).total, t->stream, pg, tr, tc);
        t->last_prune_n = n;
        t->last_prune_nstrips = g.nstrips;
        HIP_TRY(hipGetLastError());
        static_assert((kPruneXcdGroup & ~PRUNE_GROUP_MASK) == 0, "the group size shares its word with PRUNE_NO_RANGE_END");
        g.prune = kPruneXcdGroup | (t->sw.no_range_end ? PRUNE_NO_RANGE_END : 0);
        grid = round_up(g.nblocks, 8 * kPruneXcdGroup); // (prune_job_index maps whole groups)
    }
    if (fold) {
        if (int rc = t->d_fold_r.reserve((size_t)n * NA, &t->stream)) return rc;
        g.fold_r = t->d_fold_r.get();
    } else if (plan.nthin) {
        // fork: the thin kernel only reads the frames and writes its own partial slots
        HIP_TRY(hipEventRecord(t->ev_fork, t->stream));
        HIP_TRY(hipStreamWaitEvent(t->aux_stream, t->ev_fork, 0));
        const size_t thin_lds = thin_lds_bytes(t->n1, t->L);
        hipLaunchKernelGGL(want_resp ? k.thin_resp : k.thin, dim3(round_up(n * plan.nthin, 8)), dim3(256), thin_lds, t->aux_stream, g, tr, tc);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(t->ev_join, t->aux_stream));
    }
    size_t lds_bytes = v.lds(t->L);
#ifdef PDOG_ABLATIONS
    if (t->sw.lds_pad) { // occupancy experiments: extra LDS per workgroup
        lds_bytes += (size_t)t->sw.lds_pad;
        (void)raise_lds_limit((const void *)(want_resp ? k.fn_resp : k.fn), lds_bytes);
    }
#endif
    kernel_fn fn = want_resp ? k.fn_resp : prune ? k.fn_prune : k.fn;
    if (!want_resp && !prune && roll && v.LT == 65 && v.id == 100) { // instances with statically shortened epilogue bodies for the common window heights
        const int cls = roll_epi_class(t->n1, 65);
#define PDOG_EPI_PICK(C) if (cls == C) fn = (kernel_fn)dog_roll_kernel<65, false, 0, C>;
        PDOG_EPI_CLASSES(PDOG_EPI_PICK)
#undef PDOG_EPI_PICK
    }
    {
        LaunchGeo gs = g; // (the finishing kernel reads fold_r: the job list is the strips' alone)
        if (prune) gs.jobs = t->d_prune_jobs.get();
        hipLaunchKernelGGL(fn, dim3(grid), dim3(v.NT), lds_bytes, t->stream, gs, tr, roll ? (const f2 *)t->d_taps_roll.get() : tc);
    }
    HIP_TRY(hipGetLastError());
    if (plan.nthin && !fold) HIP_TRY(hipStreamWaitEvent(t->stream, t->ev_join, 0)); // join before the strip combine
    // roll: 64-column strips over the first `covered` columns, the last one shifted left to stay inside; ring: tw() columns each
    const int covered = plan.nthin ? plan.thin_x0 : t->n2;
    t->last_n = n;
    t->last_nslots = g.nslots;
    Finish fin;
    fin.slot_w = v.tw();
    if (roll) fin.slot_last = std::max(0, covered - v.tw());
    fin.use_mask = roll;
    fin.map = g.resp;
    fin.out_ij = req.out_ij;
    return launch_finish(t, g, fin);
}

// req.n independent windows on the kernel family path_for_batch names.  *ticket_armed: the kernels that run will publish
// req.done_value at req.done_flag (the single-window paths).
int launch_detect(pdog_tracker *t, const Request &req, bool *ticket_armed = nullptr)
{
    const VariantShape &v = *t->plan.shape;
    const Plan &plan = t->plan;
    if (ticket_armed) *ticket_armed = false;
    const int path = path_for_batch(plan, t->sw, req.n);
    // windows that fit in LDS, in batches too small to fill the GPU any other way: the fused kernel, one workgroup per window,
    // one launch; one or a few windows too large for it: the tiled kernel, one launch (dog_tiled.hpp)
    if (path == kPathFused || path == kPathTiled) {
        Request one = req;
        if (req.n != 1) one.dc_host = -1; // the host samples the DC level of a single window only
        bool launched = true;
        if (path == kPathFused) {
            if (int rc = launch_fused(t, one)) return rc;
        } else if (int rc = launch_tiled(t, one, &launched)) return rc;
        if (launched) {
            if (ticket_armed) *ticket_armed = req.done_flag != nullptr;
            return PDOG_OK;
        }
    }
    LaunchGeo g = base_geo(t, req);
    use_partials(t, g);
    g.ex = exact_ctl(t, (v.family == Family::Roll ? kFamRoll : kFamRing));
    g.nstrips = plan.nstrips;
    g.RR = v.ring(t->L);
    g.pitchA = v.pa(t->L);
    g.nblocks = req.n * plan.nstrips;
    g.nslots = plan.nstrips + plan.nthin;
    g.thin_x0 = plan.thin_x0;
    g.nthin = plan.nthin;
    if (path == kPathTwoPass || path == kPathTiled) return launch_twopass(t, req, g, ticket_armed); // (a tiled launch that was not taken falls through to here)
    return launch_strips(t, req, g);
}

} // namespace

namespace {

// a device buffer of exactly the vector's size, filled from it (tracker construction: nothing is queued yet)
template <typename T>
int upload(DeviceBuffer<T> &d, const std::vector<T> &h)
{
    if (int rc = d.reserve(h.size(), nullptr)) return rc;
    HIP_TRY(hipMemcpy(d.get(), h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return PDOG_OK;
}

// The packed window tile of the host paths (pack_tile_geo): the window with its halo of l÷2 pixels, fill materialised.  On
// the device it is a frame of its own with the guess at its centre.
struct TileFrame {
    int hw, th, tw, pitch; // halo; rows, columns and row pitch of the tile
    int centre[2];         // the tile's guess
    explicit TileFrame(const pdog_tracker *t)
        : hw(t->L >> 1), th(t->n1 + 2 * hw), tw(t->n2 + 2 * hw), pitch(round_up(tw, 16)), centre{t->r1 + hw + 1, t->r2 + hw + 1} {}
    size_t bytes() const { return (size_t)th * pitch; }
    // The reference's PaddedView extends radii + l past the frame (:45-46) and the filter reads radii + l÷2 around the
    // guess: outside [-l÷2, sz + l÷2 + 1] it raises BoundsError.
    bool holds(const pdog_tracker *t, int g1, int g2) const { return g1 >= -hw && g1 <= t->fh + hw + 1 && g2 >= -hw && g2 <= t->fw + hw + 1; }
    // tile-local 1-based answer → padded-frame index → clamp (:60-61)
    void to_frame(const pdog_tracker *t, const int32_t *guess, const int32_t *local, int32_t *out) const
    {
        out[0] = std::min(std::max(guess[0] - centre[0] + local[0], 1), t->fh);
        out[1] = std::min(std::max(guess[1] - centre[1] + local[1], 1), t->fw);
    }
};

} // namespace

extern "C" {

int pdog_abi_version(void) { return PDOG_ABI_VERSION; }
int pdog_mode_u8_device(int device, const uint8_t *d_img, int h, int w, int64_t row_stride, void *hip_stream, int *out_mode)
{
    if (!d_img || !out_mode || h <= 0 || w <= 0 || row_stride < w || (long long)h * w >= 0xffffffffLL)
        return fail(PDOG_E_ARG, "pdog_mode_u8_device: bad argument");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)hip_stream;
    DeviceBuffer<unsigned> table; // [256] counts, [256] first positions
    if (int rc = table.reserve(512, nullptr)) return rc;
    unsigned *d_tab = table.get();
    unsigned tab[512];
    hipError_t e = hipMemsetAsync(d_tab, 0, sizeof(unsigned) * 512, stream);
    if (e == hipSuccess) {
        const int blocks = (int)std::min<long long>(1024, ((long long)h * w + 255) / 256);
        hipLaunchKernelGGL(dog_mode_kernel, dim3(blocks), dim3(256), 0, stream, d_img, h, w, (long long)row_stride, d_tab, d_tab + 256);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tab, d_tab, sizeof tab, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return fail(PDOG_E_HIP, std::string("pdog_mode_u8_device: ") + hipGetErrorString(e));
    int best = 0;
    for (int v = 1; v < 256; ++v)
        if (tab[v] > tab[best] || (tab[v] == tab[best] && tab[256 + v] < tab[256 + best])) best = v;
    *out_mode = best;
    return PDOG_OK;
}

int pdog_create(int device, int frame_h, int frame_w, double target_width, int win_h, int win_w,
                int darker_target, int fill, pdog_tracker **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_create: out is null");
    *out = nullptr;
    if (frame_h <= 0 || frame_w <= 0 || !(target_width > 0) || win_h < 0 || win_w < 0 || fill < 0 || fill > 255)
        return fail(PDOG_E_ARG, "pdog_create: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(PDOG_E_NODEV, "pdog_create: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(PDOG_E_ARG, "pdog_create: device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(PDOG_E_NODEV, std::string("pdog_create: device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    HIP_TRY(hipSetDevice(device));

    std::unique_ptr<pdog_tracker> owner(new pdog_tracker()); // a failure below destroys what was built so far
    pdog_tracker *t = owner.get();
    t->device = device;
    t->fh = frame_h; t->fw = frame_w;
    t->tw = target_width;
    t->sigma = sigma_of(target_width);             // :41
    t->darker = darker_target ? 1 : 0;             // :42
    t->L = kernel_len_of_sigma(t->sigma);          // :43
    t->r1 = win_h / 2; t->r2 = win_w / 2;          // :44
    t->n1 = 2 * t->r1 + 1; t->n2 = 2 * t->r2 + 1;  // :56
    t->fill = fill;                                // :47
    if ((long long)t->n1 * t->n2 > 0x3fffffffLL) return fail(PDOG_E_ARG, "pdog_create: window too large");

    if (int rc = replan(t, read_switches(), -1)) return rc;

    // taps: Float64 on the host, one rounding to f32
    std::vector<double> gp(t->L), gm(t->L);
    gaussian_1d(t->sigma, t->L, gp.data());
    gaussian_1d(t->sigma * std::sqrt(2.0), t->L, gm.data());
    const double s = (t->darker ? -1.0 : 1.0) / 255.0; // direction (:42) and N0f8 scale
    constexpr int kTapPad = 16; // zero taps past the end: kernels that request taps one block ahead read them
    std::vector<f2> tr(t->L + kTapPad, f2{0.f, 0.f}), tc(t->L + kTapPad, f2{0.f, 0.f});
    for (int k = 0; k < t->L; ++k) {
        tr[k] = f2{(float)gp[k], (float)gm[k]};
        tc[k] = f2{(float)(s * gp[k]), (float)(-s * gm[k])};
    }
    HIP_TRY(hipStreamCreateWithFlags(&t->own_stream, hipStreamNonBlocking));
    t->stream = t->own_stream;
    HIP_TRY(hipStreamCreateWithFlags(&t->aux_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&t->ev_switch, hipEventDisableTiming));
    if (int rc = upload(t->d_taps_row, tr)) return rc;
    if (int rc = upload(t->d_taps_col, tc)) return rc;
    {
        // roll_col_body's table: (Tc[t], Tc[t-1]) pairs per parity, T outside 0..l-1 is 0
        const int nqb = roll_col_blocks(t->L);
        std::vector<f2> tab((size_t)roll_col_table_len(t->L), f2{0.f, 0.f});
        auto tapc = [&](int c, int k) -> float {
            if (k < 0 || k >= t->L) return 0.f;
            return c ? tc[k].y : tc[k].x;
        };
        for (int qb = 0; qb < nqb; ++qb)
            for (int p = 0; p < 2; ++p)
                for (int c = 0; c < 2; ++c)
                    for (int m = 0; m < ROLL_QB; ++m) {
                        const int tt = p + 2 * (ROLL_QB * qb + m);
                        tab[((qb * 2 + p) * 2 + c) * ROLL_QB + m] = f2{tapc(c, tt), tapc(c, tt - 1)};
                    }
        if (int rc = upload(t->d_taps_roll, tab)) return rc;
    }
    if (int rc = t->d_small.reserve(4, nullptr)) return rc;
    if (int rc = t->h_pinned.reserve(1, nullptr, true)) return rc;
    {
        // exact mode (dog_exact.hpp): the reference's dense kernel in Float64, built exactly as :41-43 builds it
        // (K = dir·(g₊⊗g₊ − g₋⊗g₋), column-major), and the decision threshold T = 2δ, δ = u·(6l + 4) for |pixel − dc| ≤ 255
        std::vector<double> K((size_t)t->L * t->L);
        dense_dog_kernel(gp.data(), gm.data(), t->L, t->darker != 0, K.data());
        if (int rc = upload(t->d_K64, K)) return rc;
        t->h_gp = gp;
        t->h_gm = gm;
        {
            const ExactFactors ef = exact_factors(gp, gm);
            t->F_sym_int = ef.sym_int; t->F_sym_sep = ef.sym_sep; t->F_ring = ef.ring; t->F_rescan = ef.rescan;
        }
        t->K_norm = dog_kernel_norm_up(gp, gm);
        {
            const std::vector<uint32_t> wq = dog_refine_weights(gp, gm, t->K_norm);
            if ((int)wq.size() != prune_span(t->L) * prune_span(t->L)) return fail(PDOG_E_ARG, "pdog_create: the second stage's weight table has another span than the kernels");
            const int ns = prune_span(t->L), pitch = prune_refine_pitch(ns);
            std::vector<uint32_t> tab((size_t)ns * pitch + 4, 0u); // rows padded to whole groups of four, a group of zeros behind the last
            for (int dy = 0; dy < ns; ++dy) std::copy(wq.begin() + (size_t)dy * ns, wq.begin() + (size_t)(dy + 1) * ns, tab.begin() + (size_t)dy * pitch);
            if (int rc = upload(t->d_refine_wq, tab)) return rc;
        }
        if (int rc = t->d_prune_stat.reserve(4 + PRUNE_PHASES + 1, nullptr, true)) return rc; // [4 …]: phase cycles of the pre-pass and the workgroups that stamped (diagnostic build)
        if (int rc = t->d_ref_stat.reserve(16, nullptr, true)) return rc; // [4..7] unused, [8..15]: phase cycles of the refinement (diagnostic build)
        {
            std::vector<double> g2(2 * (size_t)t->L);
            std::copy(gp.begin(), gp.end(), g2.begin());
            std::copy(gm.begin(), gm.end(), g2.begin() + t->L);
            if (int rc = upload(t->d_g64, g2)) return rc;
        }
        // separable Float64 vs the reference's dense Float64 (l² sequential roundings): both within δ64 of the exact value
        t->exact_T64 = 2.0 * std::ldexp(1.0, -53) * (2.1 * t->L * t->L + 8.0 * t->L + 64.0);
        {
            RefineParams rp;
            rp.K64 = t->d_K64.get();
            rp.g64 = t->d_g64.get();
            rp.dir = t->darker ? -1.0 : 1.0;
            rp.T64 = t->exact_T64;
            if (int rc = upload(t->d_rp, std::vector<RefineParams>(1, rp))) return rc;
        }
        t->exact = exact_fits(geometry_of(t));
        if (!t->exact) // (success all the same: pdog_last_error carries the note, pdog_get_exact reports the state)
            (void)fail(PDOG_OK, "pdog_create: window too tall for the refinement's LDS block (n1 + l beyond ~9000 rows): exact mode is OFF for this tracker");
    }
    if (int rc = ensure_capacity(t, 1)) return rc;
    *out = owner.release();
    return PDOG_OK;
}

int pdog_destroy(pdog_tracker *t)
{
    delete t; // ~pdog_tracker drains and destroys the streams; the buffers free themselves
    return PDOG_OK;
}

int pdog_get_info(const pdog_tracker *t, pdog_info *o)
{
    if (!t || !o) return fail(PDOG_E_ARG, "pdog_get_info: null");
    o->frame_h = t->fh; o->frame_w = t->fw;
    o->radius_h = t->r1; o->radius_w = t->r2;
    o->win_h = t->n1; o->win_w = t->n2;
    o->kernel_len = t->L;
    o->fill = t->fill;
    o->darker_target = t->darker;
    o->n_strips = t->plan.nstrips;
    o->strip_w = t->plan.shape->tw();
    o->variant = t->plan.shape->id;
    o->sigma = t->sigma;
    o->target_width = t->tw;
    const int64_t th = t->n1 + t->L - 1, tw = t->n2 + t->L - 1;
    o->algorithmic_bytes_per_window = th * tw + 8;
    o->algorithmic_fma_per_window = 2LL * t->L * (th * t->n2 + (int64_t)t->n1 * t->n2);
    return PDOG_OK;
}

int pdog_kernel_for_batch(const pdog_tracker *t, int n, int *out_variant)
{
    if (!t || !out_variant || n < 0) return fail(PDOG_E_ARG, "pdog_kernel_for_batch: bad argument");
    *out_variant = path_for_batch(t->plan, t->sw, n);
    return PDOG_OK;
}

int pdog_set_fill(pdog_tracker *t, int fill)
{
    if (!t || fill < 0 || fill > 255) return fail(PDOG_E_ARG, "pdog_set_fill: bad argument");
    t->fill = fill;
    return PDOG_OK;
}

int pdog_set_stream(pdog_tracker *t, void *hip_stream)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_set_stream: null tracker");
    hipStream_t ns = (hipStream_t)hip_stream;
    if (ns == t->stream) return PDOG_OK;
    // The tracker's scratch (strip partials, two-pass intermediate, DC levels, counters, chain state) is per tracker,
    // not per stream: whatever is still queued on the previous stream must finish before work on the new one may
    // touch it.  Stream-ordered, no host wait.
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipEventRecord(t->ev_switch, t->stream));
    HIP_TRY(hipStreamWaitEvent(ns, t->ev_switch, 0));
    t->stream = ns;
    return PDOG_OK;
}

int pdog_get_stream(const pdog_tracker *t, void **out_hip_stream)
{
    if (!t || !out_hip_stream) return fail(PDOG_E_ARG, "pdog_get_stream: null pointer");
    *out_hip_stream = (void *)t->stream;
    return PDOG_OK;
}

int pdog_reserve(pdog_tracker *t, int max_windows)
{
    if (!t || max_windows <= 0) return fail(PDOG_E_ARG, "pdog_reserve: bad argument");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return ensure_capacity(t, max_windows);
}

int pdog_set_variant(pdog_tracker *t, int variant)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_set_variant: null tracker");
    if (variant >= 0 && !find_variant(variant)) return fail(PDOG_E_ARG, "pdog_set_variant: unknown variant id");
    HIP_TRY(hipSetDevice(t->device));
    return replan(t, t->sw, variant);
}

// Drain the tracker's stream and report what its kernels raised while they ran: every entry point that waits for the
// stream goes through here, so a fault surfaces at the first call that waits — not at a later, unrelated pdog_sync.
static int drain_and_check(pdog_tracker *t, const char *who)
{
    HIP_TRY(hipSetDevice(t->device)); // (group mode: the current device is whichever rank was touched last)
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (const int32_t raised = __atomic_load_n(&t->h_pinned.get()->kernel.raised, __ATOMIC_ACQUIRE)) { // raised by a kernel
        __atomic_store_n(&t->h_pinned.get()->kernel.raised, 0, __ATOMIC_RELEASE);
        if (raised == 2) { // a wait between resident workgroups gave up (wait_counter): the positions of that work are not valid
            if (t->tiled_run.d_ctl.get()) (void)hipMemset(t->tiled_run.d_ctl.get(), 0, sizeof(int) * t->tiled_run.d_ctl.capacity()); // counters, flags and the abort word
            return fail(PDOG_E_HIP, std::string(who) + ": a kernel gave up waiting for its other workgroups (device-side watchdog); the results of the work just finished are not valid");
        }
        // a device-resident guess was out of range
        return fail(PDOG_E_RANGE, std::string(who) + ": a guess of the work just finished lies outside the padded frame (reference: BoundsError, "
                                  "src/PawsomeTracker.jl:45-46); positions were computed with the fill value there");
    }
    return PDOG_OK;
}

int pdog_sync(pdog_tracker *t)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_sync: null tracker");
    return drain_and_check(t, "pdog_sync");
}

int pdog_set_exact(pdog_tracker *t, int on)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_set_exact: null tracker");
    if (on && !exact_fits(geometry_of(t)))
        return fail(PDOG_E_ARG, "pdog_set_exact: window too tall for the refinement's LDS block");
    HIP_TRY(hipStreamSynchronize(t->stream));
    t->exact = on != 0;
    t->exact_all = on == 2;
    return PDOG_OK;
}

int pdog_set_tuning(pdog_tracker *t, const char *key, int value)
{
    if (!t || !key) return fail(PDOG_E_ARG, "pdog_set_tuning: null pointer");
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipStreamSynchronize(t->stream));
    const std::string k(key);
    const bool on = value != 0;
    if (k == "host_copy") t->sw.host_copy = on;
    else if (k == "host_sync") t->sw.host_sync = on;
    else if (k == "twopass_4l") t->sw.twopass_4l = on;
    else if (k == "no_roll_map") t->sw.no_roll_map = on;
    else if (k == "no_fold") t->sw.no_fold = on;
    else if (k == "fold_always") t->sw.fold_always = on;
    else if (k == "no_pad_skip") t->sw.no_pad_skip = on;
    else if (k == "no_prune") t->sw.no_prune = on;
    else if (k == "no_refine") t->sw.no_refine = on;
    else if (k == "no_range_end") t->sw.no_range_end = on;
    else if (k == "fenced_publish") t->sw.fenced_publish = on;
    else if (k == "fault_inject") t->sw.fault_inject = on;
    else if (k == "measure_global") t->sw.measure_global = on;
    else if (k == "peaks_no_list") t->peaks.no_list = on; // include/pawsome_peaks.h
    else if (k == "motion_lds") t->motion_lds = on;       // include/pawsome_motion.h
    else if (k == "no_fused_c" || k == "no_tiled") { // inputs of the plan: the latency kernels' instances and tile layouts
        Switches sw = t->sw;
        (k == "no_tiled" ? sw.no_tiled : sw.no_fused_c) = on;
        return replan(t, sw, t->plan.forced ? t->plan.shape->id : -1);
    } else return fail(PDOG_E_ARG, "pdog_set_tuning: unknown key '" + k + "'");
    return PDOG_OK;
}

int pdog_get_exact_detail(pdog_tracker *t, uint64_t out[4])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_exact_detail: null pointer");
    if (int rc = drain_and_check(t, "pdog_get_exact_detail")) return rc;
    unsigned long long v[16];
    HIP_TRY(hipMemcpy(v, t->d_ref_stat.get(), sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = (uint64_t)v[i];
#ifdef PDOG_ABLATIONS
    std::fprintf(stderr, "pdog refine phases (shader cycles, thread 0): setup %llu, tile %llu, row32 %llu, col32 %llu, row64 %llu, cand64 %llu, verdict %llu\n",
                 v[8], v[9], v[10], v[11], v[12], v[13], v[14]);
#endif
    return PDOG_OK;
}

int pdog_get_prune_counts(pdog_tracker *t, uint64_t out[2])
{
    if (!t || !out) return fail(PDOG_E_ARG, "pdog_get_prune_counts: null pointer");
    if (int rc = drain_and_check(t, "pdog_get_prune_counts")) return rc;
    unsigned long long v[2];
    HIP_TRY(hipMemcpy(v, t->d_prune_stat.get(), sizeof v, hipMemcpyDeviceToHost));
    out[0] = (uint64_t)v[0];
    out[1] = (uint64_t)v[1];
#ifdef PDOG_ABLATIONS
    {
        unsigned long long ph[PRUNE_PHASES + 1];
        HIP_TRY(hipMemcpy(ph, t->d_prune_stat.get() + 4, sizeof ph, hipMemcpyDeviceToHost));
        const double wg = ph[PRUNE_PHASES] ? (double)ph[PRUNE_PHASES] : 1.0;
        std::fprintf(stderr, "pdog prune phases (cycles per workgroup, thread 0; %llu workgroups): dc %.0f, energy %.0f, straddle %.0f, cell+E %.0f, patch %.0f, row %.0f, "
                             "col %.0f, hull %.0f, publish %.0f\n",
                     ph[PRUNE_PHASES], ph[0] / wg, ph[1] / wg, ph[2] / wg, ph[3] / wg, ph[4] / wg, ph[5] / wg, ph[6] / wg, ph[7] / wg, ph[8] / wg);
    }
#endif
    return PDOG_OK;
}

int pdog_get_prune_jobs(pdog_tracker *t, int capacity, int32_t *h_out, int *count)
{
    if (!t || !count || capacity < 0 || (capacity > 0 && !h_out)) return fail(PDOG_E_ARG, "pdog_get_prune_jobs: bad argument");
    if (int rc = drain_and_check(t, "pdog_get_prune_jobs")) return rc;
    if (t->last_prune_n <= 0) return fail(PDOG_E_ARG, "pdog_get_prune_jobs: no batch of this tracker ran the bounding pass");
    PruneJob head;
    HIP_TRY(hipMemcpy(&head, t->d_prune_jobs.get(), sizeof head, hipMemcpyDeviceToHost));
    const long long room = (long long)t->last_prune_n * t->last_prune_nstrips;
    if (head.b < 0 || head.b > room) return fail(PDOG_E_RANGE, "pdog_get_prune_jobs: the list's count lies outside the list");
    *count = head.b;
    const int m = std::min(head.b, capacity);
    std::vector<PruneJob> jobs((size_t)m);
    if (m) HIP_TRY(hipMemcpy(jobs.data(), t->d_prune_jobs.get() + 1, sizeof(PruneJob) * (size_t)m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; ++i) {
        h_out[4 * i] = jobs[i].b;
        h_out[4 * i + 1] = jobs[i].s_dc & 0xffff;
        h_out[4 * i + 2] = jobs[i].ba;
        h_out[4 * i + 3] = jobs[i].bb;
    }
    return PDOG_OK;
}

int pdog_get_batch_maxima(pdog_tracker *t, int n, float *h_out)
{
    if (!t || !h_out || n <= 0) return fail(PDOG_E_ARG, "pdog_get_batch_maxima: bad argument");
    if (int rc = drain_and_check(t, "pdog_get_batch_maxima")) return rc;
    if (n != t->last_n || t->last_nslots <= 0) return fail(PDOG_E_ARG, "pdog_get_batch_maxima: the last batch on the strip kernels had another size (or there was none)");
    std::vector<float> pv((size_t)n * t->last_nslots);
    HIP_TRY(hipMemcpy(pv.data(), t->d_part_val.get(), sizeof(float) * pv.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b) h_out[b] = *std::max_element(pv.begin() + (size_t)b * t->last_nslots, pv.begin() + (size_t)(b + 1) * t->last_nslots);
    return PDOG_OK;
}

int pdog_get_exact(pdog_tracker *t, int *out_on, double *out_threshold, uint64_t *out_refined)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_get_exact: null tracker");
    if (out_on) *out_on = t->exact ? 1 : 0;
    if (out_threshold) { // 2δ of the tracker's batch kernel family (small batches may run another family with a tighter bound)
        *out_threshold = (double)exact_ctl(t, batch_family(*t->plan.shape)).T;
    }
    if (out_refined) {
        if (int rc = drain_and_check(t, "pdog_get_exact")) return rc;
        unsigned long long v = 0;
        HIP_TRY(hipMemcpy(&v, t->d_ref_stat.get(), sizeof v, hipMemcpyDeviceToHost));
        *out_refined = (uint64_t)v;
    }
    return PDOG_OK;
}

int pdog_detect_batch(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                      int n_frames, const int32_t *d_frame_index, const int32_t *d_guesses, int n,
                      int32_t *d_out_ij, float *d_out_resp)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_detect_batch: null tracker");
    if (n == 0) return PDOG_OK;
    if (!d_frames || !d_guesses || !d_out_ij) return fail(PDOG_E_ARG, "pdog_detect_batch: null pointer");
    if (int rc = check_stack("pdog_detect_batch", t->fw, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_detect_batch: more windows than frames and no frame index");
    if ((long long)n * t->plan.nstrips > 0x7ffffff0LL) return fail(PDOG_E_ARG, "pdog_detect_batch: batch too large");
    HIP_TRY(hipSetDevice(t->device));
    if (int rc = ensure_capacity(t, n)) return rc;
    Request req;
    req.frames = d_frames; req.frame_stride = frame_stride; req.row_stride = row_stride;
    req.frame_index = d_frame_index; req.guesses = d_guesses; req.n = n;
    req.out_ij = d_out_ij; req.out_resp = d_out_resp;
    return launch_detect(t, req);
}

// ---- response and sub-pixel position at tracked points (dog_measure.hpp) ----
int pdog_subpixel(const double resp5[5], const int32_t ij[2], double out_sub[2])
{
    if (!resp5 || !ij || !out_sub) return fail(PDOG_E_ARG, "pdog_subpixel: null pointer");
    subpixel_rule(resp5, ij[0], ij[1], out_sub);
    return PDOG_OK;
}

// Reads the tracker's geometry, fill and Float64 kernel table and nothing else: no workspace, no counter, no variant.
int pdog_measure(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride, int n_frames,
                 const int32_t *d_frame_index, const int32_t *d_ij, int n, double *d_out_resp5, double *d_out_sub)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_measure: null tracker");
    if (!d_frames || !d_ij) return fail(PDOG_E_ARG, "pdog_measure: null pointer");
    if (!d_out_resp5 && !d_out_sub) return fail(PDOG_E_ARG, "pdog_measure: both outputs are null");
    if (int rc = check_stack("pdog_measure", t->fw, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!d_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_measure: more positions than frames and no frame index");
    if (n == 0) return PDOG_OK;
    HIP_TRY(hipSetDevice(t->device));
    MeasureGeo g;
    g.frames = d_frames;
    g.frame_stride = frame_stride;
    g.row_stride = row_stride;
    g.frame_index = d_frame_index;
    g.ij = d_ij;
    g.n = n;
    g.fh = t->fh;
    g.fw = t->fw;
    g.fill = t->fill;
    g.L = t->L;
    g.K64 = t->d_K64.get();
    g.out_resp5 = d_out_resp5;
    g.out_sub = d_out_sub;
    // positions per wave: as many tiles as leave four workgroups per CU their LDS.  Below MEASURE_MIN_PPW tiles per wave
    // (l > 93) the kernel reads the frame itself: a wave of one tile (l = 293) keeps 5 lanes of a CU busy and measured
    // 45–72 ms per 4096 positions against 33 ms in place; 8 tiles per wave (l = 65) measured 2.5× faster than in place
    const size_t tile = (size_t)measure_tile_bytes(t->L);
    g.tile_pitch = measure_tile_pitch(t->L);
    g.tile_bytes = (int)tile;
    g.ppw = (int)std::min<size_t>(MEASURE_PPW, MEASURE_WG_LDS / tile);
    if (g.ppw < MEASURE_MIN_PPW || t->sw.measure_global) {
        g.ppw = MEASURE_PPW;
        g.tile_pitch = g.tile_bytes = 0;
    }
    const size_t lds = (size_t)g.ppw * g.tile_bytes;
    if (lds > 48 * 1024)
        if (int rc = raise_lds_limit((const void *)dog_measure_kernel, lds)) return rc;
    hipLaunchKernelGGL(dog_measure_kernel, dim3((n + g.ppw - 1) / g.ppw), dim3(MEASURE_NT), lds, t->stream, g);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

int pdog_detect_host(pdog_tracker *t, const uint8_t *h_frame, int64_t row_stride, const int32_t guess[2],
                     int32_t out_ij[2], float *h_resp)
{
    if (!t || !h_frame || !guess || !out_ij) return fail(PDOG_E_ARG, "pdog_detect_host: null pointer");
    if (int rc = check_row_stride("pdog_detect_host", t->fw, row_stride)) return rc;
    const TileFrame tile(t);
    if (!tile.holds(t, guess[0], guess[1])) return fail(PDOG_E_RANGE, "pdog_detect_host: guess outside the padded frame (reference: BoundsError)");
    HIP_TRY(hipSetDevice(t->device));
    if (h_resp)
        if (int rc = t->d_resp.reserve((size_t)t->n1 * t->n2, nullptr)) return rc;
    if (!t->sw.host_copy) {
        // Latency path: the tile is packed into pinned, device-mapped memory (fill materialised, as in
        // pdog_detect_batch_host) and the kernels read it in place over PCIe — no copy commands.  On the device the
        // tile is a frame of its own with the guess at its centre; the tile-local answer is mapped back and clamped
        // (:60-61) here.  Completion: the single-window kernels (fused, two-launch two-pass) publish a ticket right
        // after the answer (system-scope release into the host-coherent mailbox) and the host polls for it — the
        // answer is back before the kernel's end-of-grid bookkeeping, and the stream stays ordered for whatever is
        // queued next.  With a response copy, a pinned batch kernel that publishes no ticket, or a ticket that does
        // not show up in time (a failed launch), the stream is synchronised as usual.
        if (int rc = t->h_tile.reserve(tile.bytes(), nullptr)) return rc;
        Mailbox *mail = t->h_pinned.get(), *d_mail = t->h_pinned.device();
        const bool trace = t->sw.host_trace; // diagnostic: where a call's wall time goes
        const auto t0 = std::chrono::steady_clock::now();
        // cached stores: the functor's kernel reads this tile in place right away (non-temporal stores measured equal here)
        pack_tile_geo(h_frame, t->fh, t->fw, row_stride, t->fill, t->L, t->r1, t->r2, guess[0], guess[1], t->h_tile.get(), tile.pitch, false);
        mail->guess[0] = tile.centre[0];   // the guess is the tile's centre
        mail->guess[1] = tile.centre[1];
        const auto t1 = std::chrono::steady_clock::now();
        if (int rc = ensure_capacity(t, 1)) return rc;
        const int32_t ticket = t->ticket = t->ticket % 0x7fffffff + 1;   // 1 … 2^31 − 1, never the mailbox's initial 0
        bool armed = false;
        // the DC level from the tile just packed: the kernels' own 32×32 sample grid (dc_sample_sum / dc_from_sum), so the
        // fused and tiled kernels skip their sample loads and the reduction barrier (≈1.5 µs of a 10.8 µs frame)
        int dc_host;
        {
            int total = 0;
            for (int k = 0; k < 1024; ++k)
                total += t->h_tile.get()[(size_t)(int)(((long long)(k >> 5) * tile.th) >> 5) * tile.pitch + (size_t)(int)(((long long)(k & 31) * tile.tw) >> 5)];
            dc_host = (total + 512) >> 10;
            if (std::abs(dc_host - t->fill) <= 8) dc_host = t->fill;
        }
        Request req;
        req.frames = t->h_tile.device(); req.frame_stride = (int64_t)tile.bytes(); req.row_stride = tile.pitch;
        req.guesses = d_mail->guess; req.n = 1;
        req.out_ij = d_mail->result; req.out_resp = h_resp ? t->d_resp.get() : nullptr;
        req.fh = tile.th; req.fw = tile.tw;
        req.done_flag = &d_mail->ticket; req.done_value = ticket;
        req.dc_host = t->sw.no_host_dc ? -1 : dc_host;
        if (int rc = launch_detect(t, req, &armed)) return rc;
        if (h_resp) HIP_TRY(hipMemcpyAsync(h_resp, t->d_resp.get(), sizeof(float) * (size_t)t->n1 * t->n2, hipMemcpyDeviceToHost, t->stream));
        const auto t2 = std::chrono::steady_clock::now();
        bool done = false;
        if (armed && !h_resp && !t->sw.host_sync) {
            const auto deadline = t2 + std::chrono::microseconds(500);
            for (int spin = 0;; ++spin) {
                if (__atomic_load_n(&mail->ticket, __ATOMIC_ACQUIRE) == ticket) { done = true; break; }
                if ((spin & 63) == 63 && std::chrono::steady_clock::now() > deadline) break;
                __builtin_ia32_pause();
            }
        }
        if (!done) HIP_TRY(hipStreamSynchronize(t->stream));
        if (trace) {
            const auto t3 = std::chrono::steady_clock::now();
            auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            std::fprintf(stderr, "pdog functor: pack %.1f us, launch %.1f us, sync %.1f us\n", us(t0, t1), us(t1, t2), us(t2, t3));
        }
        tile.to_frame(t, guess, mail->result, out_ij);
        return PDOG_OK;
    }
    if (int rc = t->d_frame.reserve((size_t)t->fh * t->fw, nullptr)) return rc;
    if (int rc = ensure_capacity(t, 1)) return rc;
    Mailbox *mail = t->h_pinned.get();
    int32_t *d_small = t->d_small.get();
    {
        // Only the window's padded tile is read by the kernels (anything else they touch feeds masked
        // lanes), so only that rectangle of the frame crosses PCIe: 109×109 B instead of 2 MB for the
        // default 45×45 window on a 1080p frame.
        const int r_lo = std::max(0, guess[0] - t->r1 - 1 - tile.hw), r_hi = std::min(t->fh, guess[0] + t->r1 + tile.hw);
        const int c_lo = std::max(0, guess[1] - t->r2 - 1 - tile.hw), c_hi = std::min(t->fw, guess[1] + t->r2 + tile.hw);
        if (r_hi > r_lo && c_hi > c_lo)
            HIP_TRY(hipMemcpy2DAsync(t->d_frame.get() + (size_t)r_lo * t->fw + c_lo, t->fw, h_frame + (size_t)r_lo * row_stride + c_lo,
                                     row_stride, (size_t)(c_hi - c_lo), (size_t)(r_hi - r_lo), hipMemcpyHostToDevice, t->stream));
    }
    mail->guess[0] = guess[0];
    mail->guess[1] = guess[1];
    HIP_TRY(hipMemcpyAsync(d_small, mail->guess, sizeof(int32_t) * 2, hipMemcpyHostToDevice, t->stream));
    Request req;
    req.frames = t->d_frame.get(); req.frame_stride = (int64_t)t->fh * t->fw; req.row_stride = t->fw;
    req.guesses = d_small; req.n = 1;
    req.out_ij = d_small + 2; req.out_resp = h_resp ? t->d_resp.get() : nullptr;
    if (int rc = launch_detect(t, req)) return rc;
    HIP_TRY(hipMemcpyAsync(mail->result, d_small + 2, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, t->stream));
    if (h_resp) HIP_TRY(hipMemcpyAsync(h_resp, t->d_resp.get(), sizeof(float) * (size_t)t->n1 * t->n2, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    out_ij[0] = mail->result[0];
    out_ij[1] = mail->result[1];
    return PDOG_OK;
}

} // extern "C"

namespace {

int ingest_threads(const pdog_tracker *t)
{
    if (t->sw.host_threads) return t->sw.host_threads;
    const unsigned hc = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min(16u, hc ? hc : 1u));
}

} // namespace

// Frame ingest for batches: the frames are in HOST memory, as `read!(vid, trckr.img.data)`
// (:166) leaves them.  Only each window's padded tile crosses PCIe (cfg3: 103 KB instead of the 2 MB
// frame): host threads pack the tiles of a chunk into pinned staging, one async copy per chunk moves them
// on a copy stream, and the kernels of chunk c run beside the copy of chunk c+1 and the packing of c+2.
// On the device every tile is a frame of its own with the guess at its centre, so the kernels see exactly
// the pixel values the padded frame would give them; the tile-local result is mapped back and clamped to
// the frame (:60-61) on the host.
extern "C" int pdog_detect_batch_host(pdog_tracker *t, const uint8_t *h_frames, int64_t frame_stride, int64_t row_stride,
                                      int n_frames, const int32_t *h_frame_index, const int32_t *h_guesses, int n,
                                      int32_t *h_out_ij)
{
    if (!t) return fail(PDOG_E_ARG, "pdog_detect_batch_host: null tracker");
    if (n == 0) return PDOG_OK;
    if (!h_frames || !h_guesses || !h_out_ij) return fail(PDOG_E_ARG, "pdog_detect_batch_host: null pointer");
    if (int rc = check_stack("pdog_detect_batch_host", t->fw, n_frames, row_stride, frame_stride, n >= 0)) return rc;
    if (!h_frame_index && n > n_frames) return fail(PDOG_E_ARG, "pdog_detect_batch_host: more windows than frames and no frame index");
    const TileFrame tile(t);
    for (int b = 0; b < n; ++b) {
        if (!tile.holds(t, h_guesses[2 * b], h_guesses[2 * b + 1]))
            return fail(PDOG_E_RANGE, "pdog_detect_batch_host: guess outside the padded frame (reference: BoundsError)");
        if (h_frame_index && (h_frame_index[b] < 0 || h_frame_index[b] >= n_frames))
            return fail(PDOG_E_ARG, "pdog_detect_batch_host: frame index out of range");
    }
    HIP_TRY(hipSetDevice(t->device));
    const size_t tile_bytes = tile.bytes();
    // chunk: ≈32 MB of tiles, at least 64 windows (the batch kernels want ≥ 1000 strip-waves when they can get them)
    int chunk = (int)std::max<size_t>(64, ((size_t)32 << 20) / tile_bytes);
    if (t->sw.ingest_chunk) chunk = t->sw.ingest_chunk;
    chunk = std::min(chunk, n);
    constexpr int NS = Ingest::kSlots;
    Ingest &in = t->ingest;
    if (!in.stream) {
        HIP_TRY(hipStreamCreateWithFlags(&in.stream, hipStreamNonBlocking));
        for (int k = 0; k < NS; ++k) {
            HIP_TRY(hipEventCreateWithFlags(&in.ev_h2d[k], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&in.ev_used[k], hipEventDisableTiming));
        }
    }
    const size_t slot_bytes = tile_bytes * chunk;
    for (int k = 0; k < NS; ++k) {
        if (std::min(in.h_stage[k].capacity(), in.d_tiles[k].capacity()) < slot_bytes)
            HIP_TRY(hipStreamSynchronize(in.stream)); // copies queued into the old slot (reserve drains the tracker's stream)
        if (int rc = in.h_stage[k].reserve(slot_bytes, &t->stream)) return rc;
        if (int rc = in.d_tiles[k].reserve(slot_bytes, &t->stream)) return rc;
    }
    if (in.d_guess.capacity() < 2 * (size_t)chunk) { // every tile's guess is its centre
        if (int rc = in.d_guess.reserve(2 * (size_t)chunk, &t->stream)) return rc;
        std::vector<int32_t> centre(2 * (size_t)chunk);
        for (int b = 0; b < chunk; ++b) { centre[2 * b] = tile.centre[0]; centre[2 * b + 1] = tile.centre[1]; }
        HIP_TRY(hipMemcpy(in.d_guess.get(), centre.data(), sizeof(int32_t) * centre.size(), hipMemcpyHostToDevice));
    }
    if (int rc = in.d_out.reserve(2 * (size_t)n, &t->stream)) return rc;
    if (int rc = in.h_out.reserve(2 * (size_t)n, &t->stream)) return rc;
    if (int rc = ensure_capacity(t, chunk)) return rc;

    const int nchunks = (n + chunk - 1) / chunk;
    std::atomic<int> next{0}, submitted{0}, failed{0};
    std::vector<std::atomic<int>> packed(nchunks);
    for (auto &p : packed) p.store(0);
    auto worker = [&]() {
        (void)hipSetDevice(t->device);
        int waited_for = -1; // highest chunk whose slot this thread has seen released
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= n || failed.load()) return;
            const int c = b / chunk;
            if (c >= NS && waited_for < c) {
                // the slot was last used by chunk c - NS: wait until its copy has been enqueued, then done
                while (submitted.load(std::memory_order_acquire) <= c - NS) {
                    if (failed.load()) return;
                    std::this_thread::yield();
                }
                if (hipEventSynchronize(in.ev_h2d[c % NS]) != hipSuccess) { failed.store(1); return; }
                waited_for = c;
            }
            const int f = h_frame_index ? h_frame_index[b] : b;
            const bool nt_stores = !t->sw.ingest_no_nt;
            pack_tile_geo(h_frames + (int64_t)f * frame_stride, t->fh, t->fw, row_stride, t->fill, t->L, t->r1, t->r2,
                          h_guesses[2 * b], h_guesses[2 * b + 1], in.h_stage[c % NS].get() + (size_t)(b - c * chunk) * tile_bytes, tile.pitch, nt_stores);
            packed[c].fetch_add(1, std::memory_order_release);
        }
    };
    const int nthreads = std::min(ingest_threads(t), n);
    std::vector<std::thread> pool;
    for (int k = 0; k < nthreads; ++k) pool.emplace_back(worker);
    int rc = PDOG_OK;
    const bool trace = t->sw.ingest_trace; // diagnostic: where the wall time of a call goes
    const auto t_begin = std::chrono::steady_clock::now();
    double wait_pack_ms = 0;
    for (int c = 0; c < nchunks && rc == PDOG_OK; ++c) {
        const int w0 = c * chunk, nw = std::min(chunk, n - w0), slot = c % NS;
        const auto tw0 = std::chrono::steady_clock::now();
        while (packed[c].load(std::memory_order_acquire) < nw && !failed.load()) std::this_thread::yield();
        wait_pack_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
        if (failed.load()) { rc = fail(PDOG_E_HIP, "pdog_detect_batch_host: event wait failed in a packing thread"); break; }
        hipError_t e = hipSuccess;
        if (c >= NS) e = hipStreamWaitEvent(in.stream, in.ev_used[slot], 0); // kernels of chunk c - NS are done with the device slot
        if (e == hipSuccess) e = hipMemcpyAsync(in.d_tiles[slot].get(), in.h_stage[slot].get(), tile_bytes * nw, hipMemcpyHostToDevice, in.stream);
        if (e == hipSuccess) e = hipEventRecord(in.ev_h2d[slot], in.stream);
        submitted.store(c + 1, std::memory_order_release);
        if (e == hipSuccess) e = hipStreamWaitEvent(t->stream, in.ev_h2d[slot], 0);
        if (e != hipSuccess) { rc = fail(PDOG_E_HIP, std::string("pdog_detect_batch_host: ") + hipGetErrorString(e)); break; }
        Request req;
        req.frames = in.d_tiles[slot].get(); req.frame_stride = (int64_t)tile_bytes; req.row_stride = tile.pitch;
        req.guesses = in.d_guess.get(); req.n = nw;
        req.out_ij = in.d_out.get() + 2 * (size_t)w0;
        req.fh = tile.th; req.fw = tile.tw;
        rc = launch_detect(t, req);
        if (rc == PDOG_OK && hipEventRecord(in.ev_used[slot], t->stream) != hipSuccess)
            rc = fail(PDOG_E_HIP, "pdog_detect_batch_host: hipEventRecord failed");
    }
    if (rc != PDOG_OK) { failed.store(1); submitted.store(nchunks + NS); }
    for (auto &th_ : pool) th_.join();
    if (rc != PDOG_OK) { (void)hipStreamSynchronize(in.stream); (void)hipStreamSynchronize(t->stream); return rc; }
    const auto t_submitted = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(in.h_out.get(), in.d_out.get(), sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    if (trace) {
        const auto t_end = std::chrono::steady_clock::now();
        std::fprintf(stderr, "pdog ingest: %d windows, %d chunks of %d, %d threads: submit loop %.2f ms (waiting for packers %.2f ms), drain %.2f ms\n",
                     n, nchunks, chunk, nthreads, std::chrono::duration<double, std::milli>(t_submitted - t_begin).count(), wait_pack_ms,
                     std::chrono::duration<double, std::milli>(t_end - t_submitted).count());
    }
    for (int b = 0; b < n; ++b) tile.to_frame(t, h_guesses + 2 * b, in.h_out.get() + 2 * b, h_out_ij + 2 * b);
    return PDOG_OK;
}

namespace {

// A validated frame table (pdog_detect_chains_indexed, pdog_detect_chains_predicted) is the checked TableWalk: step k of
// row c looks at frame h_table[c*n_steps + k], `first` = 1 means that step 0 receives the start as given and the loop begins at
// step 1; row c has table.len[c] steps on the StagedTable that was checked with it.

// The persistent roll chain: one launch, a workgroup per clip (a wave per strip) walks the clip's req.chain_len frames,
// contiguous or over req.table.
int launch_persistent(pdog_tracker *t, const Request &req)
{
    const VariantShape &v = *t->plan.shape;
    const VariantKernels &k = *t->kern;
    const int strips = chain_strips(t->plan.geo);
    ChainPredictGeo cg; // (a launch without a table takes its ChainGeo part, one without prediction its ChainTableGeo part)
    cg.pred = req.predict ? *req.predict : PredictCtl{0.f, 0, nullptr, nullptr};
    cg.tab = req.table;
    cg.g = base_geo(t, req);
    LaunchGeo &g = cg.g;
    g.guesses = nullptr; // (the chain kernel takes its guesses from cg.start)
    g.nstrips = strips; g.nslots = strips; g.nblocks = req.n * strips;
    g.ex = exact_ctl(t, kFamRoll);
    cg.start = req.guesses; cg.out_ij = req.out_ij; cg.n_frames = req.chain_len;
    cg.rp = t->exact ? t->d_rp.get() : nullptr;
    cg.taps_col_plain = t->d_taps_col.get();
    // the strips' LDS doubles as the refinement's scratch
    const size_t lds = std::max((size_t)strips * roll_lds_bytes(v.LT), refine_lds_bytes(t->n1, t->L, 1, 8));
    fit_refine_scratch(t->plan.geo, t->plan.ref_cbw, lds, &cg.ref_cbw, &cg.ref_rows);
    if (int rc = raise_lds_limit(req.predict ? (const void *)k.chain_predict : req.table.index ? (const void *)k.chain_table : (const void *)k.chain, lds)) return rc;
    const f2 *tr = t->d_taps_row.get(), *troll = t->d_taps_roll.get();
    if (req.predict) hipLaunchKernelGGL(k.chain_predict, dim3(req.n), dim3(64 * strips), lds, t->stream, cg, tr, troll);
    else if (req.table.index) hipLaunchKernelGGL(k.chain_table, dim3(req.n), dim3(64 * strips), lds, t->stream, static_cast<const ChainTableGeo &>(cg), tr, troll);
    else hipLaunchKernelGGL(k.chain, dim3(req.n), dim3(64 * strips), lds, t->stream, static_cast<const ChainGeo &>(cg), tr, troll);
    HIP_TRY(hipGetLastError());
    return PDOG_OK;
}

// (What a chain runs on — a kernel that walks its clips itself, or the stepped walk below, a batch per step: chain_path, pdog_plan.hpp.)

// The stepped walk of ONE clip: a launch per step, stream order the only dependency — step k's guess is step k − 1's
// (clamped) answer, read straight from the output array (device or host-mapped), no host round trip per frame.  With a
// table the host names each step's frame itself.  With clip.done_flag every step publishes k + 1 there: by the kernels'
// own ticket where the launch arms one, by dog_publish_kernel behind them otherwise.
int walk_clip(pdog_tracker *t, const Request &clip, const TableWalk *ct)
{
    if (int rc = ensure_capacity(t, 1)) return rc;
    Request req = clip; // one independent window per launch
    req.n = 1; req.chain_len = 1; req.progress = false;
    req.table = ClipTable{nullptr, nullptr, 0};
    const int len = ct ? t->table.len[0] : clip.chain_len, first = ct ? ct->first : 0;
    if (first && len >= 1) { // the bootstrap's position, stored as given (:161); step 1 starts from the caller's copy of it
        HIP_TRY(hipMemcpyAsync(req.out_ij, clip.guesses, sizeof(int32_t) * 2, hipMemcpyDeviceToDevice, t->stream));
        req.out_ij += 2;
    }
    for (int k = first; k < len; ++k) {
        req.frames = clip.frames + (int64_t)(ct ? ct->h_table[k] : k) * clip.frame_stride;
        if (req.done_flag) req.done_value = k + 1;
        bool armed = false;
        if (int rc = launch_detect(t, req, req.done_flag ? &armed : nullptr)) return rc;
        if (req.done_flag && !armed) {
            hipLaunchKernelGGL(dog_publish_kernel, dim3(1), dim3(64), 0, t->stream, req.done_flag, k + 1);
            HIP_TRY(hipGetLastError());
        }
        req.guesses = req.out_ij;
        req.out_ij += 2;
    }
    return PDOG_OK;
}

// The stepped walk of SEVERAL clips: step k of all clips is one batch, and dog_step_kernel files its answers under [clip][k]
// and makes them the next guesses.  Contiguous: window c looks at frame c*n_steps + k, a batch whose frame stride is one
// clip.  Table: the batch's frame index is the table's column k; a clip that has ended rides along and stores nothing.
int walk_clips(pdog_tracker *t, const Request &clips, const TableWalk *ct)
{
    const int n_clips = clips.n, n_steps = clips.chain_len, blocks = (n_clips + 255) / 256;
    if (int rc = ensure_capacity(t, n_clips)) return rc;
    if (int rc = t->d_chain_tmp.reserve(4 * (size_t)n_clips, &t->stream)) return rc;
    int32_t *cur = t->d_chain_tmp.get(), *step = cur + 2 * (size_t)n_clips;
    Request batch;
    batch.frames = clips.frames; batch.row_stride = clips.row_stride;
    batch.guesses = cur; batch.n = n_clips;
    batch.out_ij = step;
    const int32_t *d_cols = nullptr, *d_len = nullptr;
    if (ct) {
        if (int rc = t->table.upload(ct->h_table, TableShape{n_steps, n_clips, ct->max_len, 1}, t->stream, nullptr, &d_cols, &d_len)) return rc;
        hipLaunchKernelGGL(dog_chain_table_init_kernel, dim3(blocks), dim3(256), 0, t->stream, clips.guesses, d_len, cur, clips.out_ij,
                           n_clips, n_steps, ct->first);
        HIP_TRY(hipGetLastError());
        batch.frame_stride = clips.frame_stride;
    } else {
        HIP_TRY(hipMemcpyAsync(cur, clips.guesses, sizeof(int32_t) * 2 * (size_t)n_clips, hipMemcpyDeviceToDevice, t->stream));
        batch.frame_stride = clips.frame_stride * n_steps;
    }
    for (int k = ct ? ct->first : 0; k < (ct ? ct->max_len : n_steps); ++k) {
        if (ct) batch.frame_index = d_cols + (size_t)k * n_clips;
        else batch.frames = clips.frames + (int64_t)k * clips.frame_stride;
        if (int rc = launch_detect(t, batch)) return rc;
        hipLaunchKernelGGL(dog_step_kernel, dim3(blocks), dim3(256), 0, t->stream, (const int32_t *)nullptr, d_len, n_clips, n_steps, k,
                           (const int32_t *)step, cur, clips.out_ij);
        HIP_TRY(hipGetLastError());
    }
    return PDOG_OK;
}

// clips.n clips of clips.chain_len steps each: contiguous (ct null: clip c's step k is frame c*chain_len + k) or over a table.
int run_chains(pdog_tracker *t, Request clips, const TableWalk *ct)
{
    if (t->sw.tiled_force && clips.n == 1 && !t->plan.forced && !ct && !clips.progress) { // experiment switch: the tiled kernel first
        bool launched = false;
        if (int rc = launch_tiled(t, clips, &launched)) return rc;
        if (launched) return PDOG_OK;
    }
    const ChainPath path = chain_path(t->plan, t->sw, t->tiled_resident, clips.n, clips.chain_len, ct != nullptr, clips.progress);
    if (ct && path != ChainPath::Stepped) { // the kernels that walk a clip themselves read the table's rows
        if (int rc = t->table.upload(ct->h_table, TableShape{clips.chain_len, clips.n, ct->max_len, 0}, t->stream, nullptr, &clips.table.index, &clips.table.len)) return rc;
        clips.table.first = ct->first;
    }
    switch (path) {
    case ChainPath::Fused: return launch_fused(t, clips);
    case ChainPath::Persistent: return launch_persistent(t, clips);
    case ChainPath::Tiled: {
        bool launched = false;
        if (int rc = launch_tiled(t, clips, &launched)) return rc;
        if (launched) return PDOG_OK;
        break; // not taken (the cooperative launch was refused): the stepped walk
    }
    case ChainPath::Stepped:
        break;
    }
    return clips.n == 1 ? walk_clip(t, clips, ct) : walk_clips(t, clips, ct);
}

} // namespace

extern "C" int pdog_detect_chains(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                  int n_frames, int n_clips, const int32_t *d_start_guesses, int32_t *d_out_ij)
{
    if (!t || !d_frames || !d_start_guesses || !d_out_ij) return fail(PDOG_E_ARG, "pdog_detect_chains: null pointer");
    if (int rc = check_stack("pdog_detect_chains", t->fw, n_frames, row_stride, frame_stride, n_clips > 0)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    Request clips;
    clips.frames = d_frames; clips.frame_stride = frame_stride; clips.row_stride = row_stride;
    clips.guesses = d_start_guesses; clips.n = n_clips; clips.chain_len = n_frames; clips.out_ij = d_out_ij;
    return run_chains(t, clips, nullptr);
}

// The chain over a frame table (include/pawsome_video.h).  The table is validated here, on the host, before anything is
// launched: no entry a kernel reads names a frame outside the stack.
extern "C" int pdog_detect_chains_indexed(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                          int n_frames, const int32_t *h_table, int n_steps, int n_clips, int first,
                                          const int32_t *d_start, int32_t *d_out_ij)
{
    if (!t || !d_frames || !h_table || !d_start || !d_out_ij) return fail(PDOG_E_ARG, "pdog_detect_chains_indexed: null pointer");
    TableWalk ct{"pdog_detect_chains_indexed", t->fw, n_frames, row_stride, frame_stride, h_table, n_steps, n_clips, 1, first, 0, 0};
    if (int rc = check_table_walk(ct, t->table.len)) return rc;
    if (ct.max_len == 0) return PDOG_OK; // no clip has a step
    HIP_TRY(hipSetDevice(t->device));
    Request clips;
    clips.frames = d_frames; clips.frame_stride = frame_stride; clips.row_stride = row_stride;
    clips.guesses = d_start; clips.n = n_clips; clips.chain_len = n_steps; clips.out_ij = d_out_ij;
    return run_chains(t, clips, &ct);
}

// The predicted chain's one-launch paths (pdog_host.hpp; pawsome_predict.hip validated the walk).
int pdog::launch_predicted(pdog_tracker *t, const PredictWalk &w, int *taken)
{
    *taken = 0;
    const TableWalk &tw = w.walk;
    const ChainPath path = chain_path(t->plan, t->sw, t->tiled_resident, tw.n_rows, tw.n_steps, true, false);
    if (path != ChainPath::Fused && !(path == ChainPath::Persistent && t->kern->chain_predict)) return PDOG_OK;
    HIP_TRY(hipSetDevice(t->device));
    Request clips;
    clips.frames = w.d_frames; clips.frame_stride = tw.frame_stride; clips.row_stride = tw.row_stride;
    clips.guesses = w.d_start; clips.n = tw.n_rows; clips.chain_len = tw.n_steps; clips.out_ij = w.d_out_ij;
    if (int rc = t->predict.table.upload(tw.h_table, TableShape{tw.n_steps, tw.n_rows, tw.max_len, 0}, t->stream, &t->predict.grown,
                                         &clips.table.index, &clips.table.len))
        return rc;
    clips.table.first = tw.first;
    const PredictCtl pc{w.m, w.coast, w.d_out_state, w.d_mstate};
    clips.predict = &pc;
    if (path == ChainPath::Fused) {
        ++t->predict.fused;
        *taken = 1;
        return launch_fused(t, clips);
    }
    ++t->predict.persistent;
    *taken = 2;
    return launch_persistent(t, clips);
}

extern "C" int pdog_detect_chain(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                 int n_frames, const int32_t start_guess[2], int32_t *d_out_ij)
{
    if (!t || !d_frames || !start_guess || !d_out_ij) return fail(PDOG_E_ARG, "pdog_detect_chain: null pointer");
    if (int rc = check_stack("pdog_detect_chain", t->fw, n_frames, row_stride, frame_stride)) return rc; // (before the start guess is queued)
    HIP_TRY(hipSetDevice(t->device));
    HIP_TRY(hipMemcpyAsync(t->d_small.get(), start_guess, sizeof(int32_t) * 2, hipMemcpyHostToDevice, t->stream));
    return pdog_detect_chains(t, d_frames, frame_stride, row_stride, n_frames, 1, t->d_small.get(), d_out_ij);
}


// ---- a chain whose positions can be consumed while it runs (the reference's Diagnose overlay,
// src/diagnose.jl:30-38, draws frame k as soon as ij[k] exists) ----
extern "C" int pdog_alloc_host(size_t bytes, void **out)
{
    if (!out || bytes == 0) return fail(PDOG_E_ARG, "pdog_alloc_host: bad argument");
    void *p = nullptr;
    HIP_TRY(hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable)); // portable: whichever device is current
    std::memset(p, 0, bytes);
    *out = p;
    return PDOG_OK;
}

extern "C" int pdog_free_host(void *p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return PDOG_OK;
}

extern "C" int pdog_detect_chain_progress(pdog_tracker *t, const uint8_t *d_frames, int64_t frame_stride, int64_t row_stride,
                                          int n_frames, const int32_t start_guess[2], int32_t *h_out_ij, int32_t *h_progress)
{
    if (!t || !d_frames || !start_guess || !h_out_ij || !h_progress) return fail(PDOG_E_ARG, "pdog_detect_chain_progress: null pointer");
    if (int rc = check_stack("pdog_detect_chain_progress", t->fw, n_frames, row_stride, frame_stride)) return rc;
    HIP_TRY(hipSetDevice(t->device));
    int32_t *d_out = nullptr, *d_prog = nullptr;
    if (hipHostGetDevicePointer((void **)&d_out, h_out_ij, 0) != hipSuccess || hipHostGetDevicePointer((void **)&d_prog, h_progress, 0) != hipSuccess)
        return fail(PDOG_E_ARG, "pdog_detect_chain_progress: h_out_ij / h_progress must come from pdog_alloc_host");
    __atomic_store_n(h_progress, 0, __ATOMIC_RELEASE);
    HIP_TRY(hipMemcpyAsync(t->d_small.get(), start_guess, sizeof(int32_t) * 2, hipMemcpyHostToDevice, t->stream));
    Request req; // one clip whose kernel publishes k + 1 after every frame
    req.frames = d_frames; req.frame_stride = frame_stride; req.row_stride = row_stride;
    req.guesses = t->d_small.get(); req.n = 1; req.chain_len = n_frames; req.out_ij = d_out;
    req.done_flag = d_prog; req.progress = true;
    return run_chains(t, req, nullptr);
}
