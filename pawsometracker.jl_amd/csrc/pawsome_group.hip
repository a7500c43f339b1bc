// pawsome_group.hip — several GPUs of one node behind one handle (include/pawsome_dog.h, pdog_group_*).
//
// The reference has no multi-device mode; the unit that shards is the functor applied to independent windows
// (/root/reference/src/PawsomeTracker.jl:55-62), and what comes back is the position list of :173.  One host
// process owns every device of the group (ncclCommInitAll): rank r keeps its shard of frames/guesses resident on
// its own device and runs the ordinary single-device path there (pdog_detect_batch through the public ABI — this
// file uses nothing else of pawsome_dog.hip); the results go to the root device with ONE ncclGather per batch,
// enqueued on each rank's tracker stream right behind its kernels (8 B per window: latency-bound over xGMI, no
// data-path collective).  Shards differ by at most one window, so the gather sends max-shard-sized blocks and a
// copy kernel on the root compacts them when n_total is not a multiple of the group size.
//
// The six collective calls go through a table (struct Rccl) that the group points to.  pdog_group_create installs librccl's;
// the test entry pdog_group_test_create_local installs a stand-in that keeps every rank on ONE device (below), so that the
// per-rank loop, the gather's protocol and the compaction run with ndev > 1 where there is one GPU.  Everything behind the
// create calls is the same code for both.
#include "pdog_host.hpp"
#include "pdog_dl.hpp"
#include <rccl/rccl.h>   // types and prototypes only: the library is opened when the first group is created (below)
#include <mutex>
#include <string>
#include <vector>

using pdog::fail;

namespace {

// RCCL is opened lazily, by pdog_group_create: a C or Julia host that only uses the single-device ABI can load this
// library on a machine (or loader path) without librccl, and no second RCCL copy enters a process that never asks for a
// group.  dlopen by SONAME: a librccl the process already holds (PyTorch-ROCm's) is the one that is used.
struct Rccl {
    void *handle = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};
Rccl &rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        pdog::DlLibrary lib;
        lib.open_first("librccl", std::initializer_list<const char *>{"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"});
        if (lib.handle) {
            r.CommInitAll = (decltype(r.CommInitAll))lib.symbol("librccl", "ncclCommInitAll");
            r.CommDestroy = (decltype(r.CommDestroy))lib.symbol("librccl", "ncclCommDestroy");
            r.GroupStart = (decltype(r.GroupStart))lib.symbol("librccl", "ncclGroupStart");
            r.GroupEnd = (decltype(r.GroupEnd))lib.symbol("librccl", "ncclGroupEnd");
            r.Gather = (decltype(r.Gather))lib.symbol("librccl", "ncclGather");
            r.GetErrorString = (decltype(r.GetErrorString))lib.symbol("librccl", "ncclGetErrorString");
        }
        r.handle = lib.handle;
        r.error = lib.error;
    });
    return r;
}
// a collective call through the group's table `net`: G_NCCL(net, GroupStart())
#define G_NCCL(net, call)                                                                                       \
    do {                                                                                                        \
        ncclResult_t r__ = (net)->call;                                                                         \
        if (r__ != ncclSuccess) return fail(PDOG_E_HIP, std::string("nccl" #call ": ") + (net)->GetErrorString(r__)); \
    } while (0)

// ---- the local transport: every rank on one device (pdog_group_test_create_local, tests only) ----
// What NCCL documents for a grouped gather on streams, and no more.  A communicator is a rank, the group's size and the state
// the group shares.  Gather is legal between GroupStart and GroupEnd, once per rank; every Gather of one group call carries
// the same count, root 0 and ncclInt32, and the root's recv is non-null — anything else is ncclInvalidUsage, from Gather or
// from GroupEnd.  At the outermost GroupEnd, for every rank r: an event is recorded on r's stream, the root's stream waits for
// it and copies r's block device-to-device into recv + r * count; then an event is recorded on the root's stream and every
// other rank's stream waits for it.  So the data is read after the sender's kernels, the root's later work (the compaction
// kernel, the next call) comes after all arrivals, and a sender's buffer is not overwritten by its next batch before it was
// read.  No host synchronisation anywhere; the events are created once per group and destroyed with its last communicator.
struct LocalShared {
    int size = 0, device = 0, alive = 0;
    std::vector<hipEvent_t> ev; // [r] rank r's work is queued, [size] the root has queued every copy
    struct Pending { bool have = false; const void *send = nullptr; void *recv = nullptr; size_t count = 0; hipStream_t stream = nullptr; };
    std::vector<Pending> pending;
    bool listed = false; // in local_open (below)
};
struct LocalComm { int rank, size; LocalShared *shared; };
// ncclGroupStart / ncclGroupEnd take no communicator: the open group is the calling thread's
thread_local int local_depth = 0;
thread_local std::vector<LocalShared *> local_open;

ncclResult_t local_comm_init_all(ncclComm_t *comm, int ndev, const int *devlist)
{
    if (!comm || ndev <= 0 || !devlist) return ncclInvalidArgument;
    for (int r = 1; r < ndev; ++r)
        if (devlist[r] != devlist[0]) return ncclInvalidArgument; // one device: that is what this transport is
    if (hipSetDevice(devlist[0]) != hipSuccess) return ncclUnhandledCudaError;
    LocalShared *s = new LocalShared();
    s->size = s->alive = ndev;
    s->device = devlist[0];
    s->pending.resize(ndev);
    for (int k = 0; k <= ndev; ++k) {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            for (hipEvent_t q : s->ev) (void)hipEventDestroy(q);
            delete s;
            return ncclUnhandledCudaError;
        }
        s->ev.push_back(e);
    }
    for (int r = 0; r < ndev; ++r) comm[r] = (ncclComm_t) new LocalComm{r, ndev, s};
    return ncclSuccess;
}

ncclResult_t local_comm_destroy(ncclComm_t comm)
{
    LocalComm *c = (LocalComm *)comm;
    if (!c) return ncclInvalidArgument;
    LocalShared *s = c->shared;
    delete c;
    if (--s->alive == 0) { // (the owner has drained every stream)
        for (auto it = local_open.begin(); it != local_open.end(); ++it)
            if (*it == s) { local_open.erase(it); break; }
        (void)hipSetDevice(s->device);
        for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
        delete s;
    }
    return ncclSuccess;
}

ncclResult_t local_group_start()
{
    ++local_depth;
    return ncclSuccess;
}

ncclResult_t local_gather(const void *sendbuff, void *recvbuff, size_t sendcount, ncclDataType_t datatype, int root, ncclComm_t comm, hipStream_t stream)
{
    LocalComm *c = (LocalComm *)comm;
    if (!c || !sendbuff) return ncclInvalidArgument;
    if (local_depth <= 0) return ncclInvalidUsage;                         // outside GroupStart … GroupEnd
    LocalShared *s = c->shared;
    LocalShared::Pending &p = s->pending[c->rank];
    if (p.have) return ncclInvalidUsage;                                   // twice for one rank
    if (datatype != ncclInt32 || root != 0) return ncclInvalidUsage;
    if (c->rank == 0 && !recvbuff) return ncclInvalidUsage;
    p.have = true; p.send = sendbuff; p.recv = recvbuff; p.count = sendcount; p.stream = stream;
    if (!s->listed) { s->listed = true; local_open.push_back(s); }
    return ncclSuccess;
}

// one group's gathers, checked and queued; its pending calls are forgotten either way
ncclResult_t local_flush(LocalShared *s)
{
    std::vector<LocalShared::Pending> p(s->size);
    p.swap(s->pending);
    s->listed = false;
    for (int r = 0; r < s->size; ++r)
        if (!p[r].have || p[r].count != p[0].count) return ncclInvalidUsage; // a rank is missing, or the ranks disagree
    const size_t bytes = p[0].count * sizeof(int32_t);
    hipStream_t root = p[0].stream;
    if (hipSetDevice(s->device) != hipSuccess) return ncclUnhandledCudaError;
    for (int r = 0; r < s->size; ++r) {
        if (r > 0) {
            if (hipEventRecord(s->ev[r], p[r].stream) != hipSuccess) return ncclUnhandledCudaError;
            if (hipStreamWaitEvent(root, s->ev[r], 0) != hipSuccess) return ncclUnhandledCudaError;
        }
        if (bytes && hipMemcpyAsync((char *)p[0].recv + r * bytes, p[r].send, bytes, hipMemcpyDeviceToDevice, root) != hipSuccess) return ncclUnhandledCudaError;
    }
    if (hipEventRecord(s->ev[s->size], root) != hipSuccess) return ncclUnhandledCudaError;
    for (int r = 1; r < s->size; ++r)
        if (hipStreamWaitEvent(p[r].stream, s->ev[s->size], 0) != hipSuccess) return ncclUnhandledCudaError;
    return ncclSuccess;
}

ncclResult_t local_group_end()
{
    if (local_depth <= 0) return ncclInvalidUsage;
    if (--local_depth > 0) return ncclSuccess; // a nested group: the outermost GroupEnd issues the calls
    std::vector<LocalShared *> open;
    open.swap(local_open);
    ncclResult_t first = ncclSuccess;
    for (LocalShared *s : open) {
        const ncclResult_t nr = local_flush(s);
        if (first == ncclSuccess) first = nr;
    }
    return first;
}

const char *local_error_string(ncclResult_t r)
{
    switch (r) {
    case ncclSuccess: return "no error (local transport)";
    case ncclUnhandledCudaError: return "unhandled HIP error (local transport)";
    case ncclInvalidArgument: return "invalid argument (local transport)";
    case ncclInvalidUsage: return "invalid usage (local transport)";
    default: return "error (local transport)";
    }
}

const Rccl &local_transport()
{
    static const Rccl t = [] {
        Rccl l;
        l.CommInitAll = local_comm_init_all;
        l.CommDestroy = local_comm_destroy;
        l.GroupStart = local_group_start;
        l.GroupEnd = local_group_end;
        l.Gather = local_gather;
        l.GetErrorString = local_error_string;
        return l;
    }();
    return t;
}

// Contiguous shards whose sizes differ by at most one: the first n_total % ndev ranks own one window more.
__host__ __device__ inline void shard_bounds(int n_total, int ndev, int rank, int &lo, int &hi)
{
    const int base = n_total / ndev, rem = n_total % ndev;
    lo = rank * base + (rank < rem ? rank : rem);
    hi = lo + base + (rank < rem ? 1 : 0);
}
// … and the inverse: which rank owns window w, and where in that rank's shard it sits.
__host__ __device__ inline void shard_owner(int n_total, int ndev, int w, int &rank, int &local)
{
    const int base = n_total / ndev, rem = n_total % ndev;
    const int cut = rem * (base + 1);
    rank = w < cut ? w / (base + 1) : rem + (w - cut) / (base > 0 ? base : 1);
    int lo, hi;
    shard_bounds(n_total, ndev, rank, lo, hi);
    local = w - lo;
}

// gathered[r][max_n][2] → out[lo_r + k][2], k < hi_r - lo_r (only needed when the shards are unequal)
__global__ void group_compact_kernel(const int32_t *__restrict__ gathered, int32_t *__restrict__ out, int n_total, int ndev, int max_n)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_total) return;
    int r, k;
    shard_owner(n_total, ndev, w, r, k);
    out[2 * w] = gathered[2 * ((long long)r * max_n + k)];
    out[2 * w + 1] = gathered[2 * ((long long)r * max_n + k) + 1];
}

} // namespace

struct pdog_group {
    int ndev = 0;
    const Rccl *net = nullptr; // the collective calls of this group: librccl's, or the local transport's
    std::vector<int> dev;
    std::vector<pdog_tracker *> tr;
    std::vector<ncclComm_t> comm;
    std::vector<pdog::DeviceBuffer<int32_t>> d_local; // per rank: max_n x 2 results of its shard
    pdog::DeviceBuffer<int32_t> d_gathered;           // root: ndev x max_n x 2 (unequal shards only)
};

// g->dev and g->net are set: a tracker per rank, then the communicators.  On failure g is destroyed.
static int group_finish_create(pdog_group *g, const char *who, int frame_h, int frame_w, double target_width, int win_h, int win_w,
                               int darker_target, int fill, pdog_group **out)
{
    const int ndev = g->ndev;
    g->tr.assign(ndev, nullptr);
    g->d_local.resize(ndev);
    for (int r = 0; r < ndev; ++r) {
        int rc = pdog_create(g->dev[r], frame_h, frame_w, target_width, win_h, win_w, darker_target, fill, &g->tr[r]);
        if (rc) { pdog_group_destroy(g); return rc; } // pdog_last_error() already holds pdog_create's text
    }
    g->comm.assign(ndev, nullptr);
    ncclResult_t nr = g->net->CommInitAll(g->comm.data(), ndev, g->dev.data());
    if (nr != ncclSuccess) {
        g->comm.clear();
        const std::string text = std::string(who) + ": ncclCommInitAll: " + g->net->GetErrorString(nr);
        pdog_group_destroy(g);
        return fail(PDOG_E_HIP, text);
    }
    *out = g;
    return PDOG_OK;
}

extern "C" {

int pdog_group_shard(const pdog_group *g, int n_total, int rank, int *lo, int *hi)
{
    if (!g) return fail(PDOG_E_ARG, "pdog_group_shard: null group");
    return pdog_shard_range(n_total, g->ndev, rank, lo, hi);
}

int pdog_shard_range(int n_total, int ndev, int rank, int *lo, int *hi)
{
    if (!lo || !hi || n_total < 0 || ndev <= 0 || rank < 0 || rank >= ndev) return fail(PDOG_E_ARG, "pdog_shard_range: bad argument");
    shard_bounds(n_total, ndev, rank, *lo, *hi);
    return PDOG_OK;
}

int pdog_shard_owner(int n_total, int ndev, int window, int *rank, int *local_index)
{
    if (!rank || !local_index || ndev <= 0 || window < 0 || window >= n_total) return fail(PDOG_E_ARG, "pdog_shard_owner: bad argument");
    shard_owner(n_total, ndev, window, *rank, *local_index);
    return PDOG_OK;
}

int pdog_group_destroy(pdog_group *g)
{
    if (!g) return PDOG_OK;
    for (int r = 0; r < (int)g->tr.size(); ++r)
        if (g->tr[r]) (void)pdog_sync(g->tr[r]);
    for (int r = 0; r < (int)g->comm.size(); ++r)
        if (g->comm[r]) (void)g->net->CommDestroy(g->comm[r]);
    for (int r = 0; r < (int)g->dev.size(); ++r) {
        (void)hipSetDevice(g->dev[r]);
        if (r < (int)g->d_local.size()) g->d_local[r].release();
        if (r == 0) g->d_gathered.release();
    }
    for (int r = 0; r < (int)g->tr.size(); ++r)
        if (g->tr[r]) (void)pdog_destroy(g->tr[r]);
    delete g;
    return PDOG_OK;
}

int pdog_group_create(int ndev, const int *devices, int frame_h, int frame_w, double target_width, int win_h, int win_w,
                      int darker_target, int fill, pdog_group **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_group_create: out is null");
    *out = nullptr;
    if (ndev <= 0 || ndev > 64) return fail(PDOG_E_ARG, "pdog_group_create: ndev must be 1 … 64");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have <= 0)
        return fail(PDOG_E_NODEV, "pdog_group_create: no HIP device (this library has no CPU path)");
    if (!rccl().error.empty() || !rccl().handle)
        return fail(PDOG_E_NODEV, "pdog_group_create: RCCL is not available: " + rccl().error + " — the single-device entry points do not need it");
    pdog_group *g = new pdog_group();
    g->ndev = ndev;
    g->net = &rccl();
    for (int r = 0; r < ndev; ++r) {
        const int d = devices ? devices[r] : r;
        if (d < 0 || d >= have) {
            delete g;
            return fail(PDOG_E_NODEV, "pdog_group_create: device ordinal " + std::to_string(d) + " requested, " + std::to_string(have) + " visible");
        }
        for (int q = 0; q < r; ++q)
            if (g->dev[q] == d) { delete g; return fail(PDOG_E_ARG, "pdog_group_create: a device appears twice (RCCL needs distinct devices)"); }
        g->dev.push_back(d);
    }
    return group_finish_create(g, "pdog_group_create", frame_h, frame_w, target_width, win_h, win_w, darker_target, fill, out);
}

int pdog_group_size(const pdog_group *g) { return g ? g->ndev : 0; }

int pdog_group_tracker(pdog_group *g, int rank, pdog_tracker **out)
{
    if (!g || !out || rank < 0 || rank >= g->ndev) return fail(PDOG_E_ARG, "pdog_group_tracker: bad argument");
    *out = g->tr[rank];
    return PDOG_OK;
}

int pdog_group_detect_batch(pdog_group *g, const uint8_t *const *d_frames, int64_t frame_stride, int64_t row_stride,
                            const int *n_frames, const int32_t *const *d_frame_index, const int32_t *const *d_guesses,
                            int n_total, int32_t *d_out_ij)
{
    if (!g) return fail(PDOG_E_ARG, "pdog_group_detect_batch: null group");
    if (n_total == 0) return PDOG_OK;
    if (!d_frames || !n_frames || !d_guesses || !d_out_ij || n_total < 0) return fail(PDOG_E_ARG, "pdog_group_detect_batch: bad argument");
    const Rccl *net = g->net;
    const int ndev = g->ndev;
    const int max_n = (n_total + ndev - 1) / ndev;
    const bool equal = n_total % ndev == 0;
    for (int r = 0; r < ndev; ++r) { // every shard's pointers are checked BEFORE anything is launched on any rank
        int lo, hi;
        shard_bounds(n_total, ndev, r, lo, hi);
        if (hi > lo && (!d_frames[r] || !d_guesses[r]))
            return fail(PDOG_E_ARG, "pdog_group_detect_batch: null frames / guesses pointer for rank " + std::to_string(r) + " (shard of " + std::to_string(hi - lo) + " windows)");
    }
    // (re)size the per-rank result blocks and the root's gather buffer; every stream is drained first
    const size_t need_local = 2 * (size_t)max_n, need_gathered = equal ? 0 : need_local * ndev;
    bool grow = g->d_gathered.capacity() < need_gathered;
    for (const auto &b : g->d_local) grow = grow || b.capacity() < need_local;
    if (grow) {
        for (int r = 0; r < ndev; ++r)
            if (int rc = pdog_sync(g->tr[r])) return rc;
        for (int r = 0; r < ndev; ++r) {
            HIP_TRY(hipSetDevice(g->dev[r]));
            if (int rc = g->d_local[r].reserve(need_local, nullptr, true)) return rc;
        }
        HIP_TRY(hipSetDevice(g->dev[0]));
        if (int rc = g->d_gathered.reserve(need_gathered, nullptr)) return rc;
    }
    // every rank: the ordinary single-device batch on its own shard
    std::vector<hipStream_t> st(ndev);
    for (int r = 0; r < ndev; ++r) {
        int lo, hi;
        pdog_group_shard(g, n_total, r, &lo, &hi);
        void *s = nullptr;
        if (int rc = pdog_get_stream(g->tr[r], &s)) return rc;
        st[r] = (hipStream_t)s;
        if (hi > lo) {
            int rc = pdog_detect_batch(g->tr[r], d_frames[r], frame_stride, row_stride, n_frames[r],
                                       d_frame_index ? d_frame_index[r] : nullptr, d_guesses[r], hi - lo, g->d_local[r].get(), nullptr);
            if (rc) return rc;
        }
    }
    // one gather of the (row, col) pairs to the root, each rank's part enqueued behind its own kernels
    int32_t *recv = equal ? d_out_ij : g->d_gathered.get();
    G_NCCL(net, GroupStart());
    for (int r = 0; r < ndev; ++r) {
        ncclResult_t nr = net->Gather(g->d_local[r].get(), recv, (size_t)2 * max_n, ncclInt32, 0, g->comm[r], st[r]);
        if (nr != ncclSuccess) {
            (void)net->GroupEnd();
            return fail(PDOG_E_HIP, std::string("pdog_group_detect_batch: ncclGather: ") + net->GetErrorString(nr));
        }
    }
    G_NCCL(net, GroupEnd());
    if (!equal) {
        HIP_TRY(hipSetDevice(g->dev[0]));
        hipLaunchKernelGGL(group_compact_kernel, dim3((n_total + 255) / 256), dim3(256), 0, st[0], (const int32_t *)g->d_gathered.get(), d_out_ij,
                           n_total, ndev, max_n);
        HIP_TRY(hipGetLastError());
    }
    return PDOG_OK;
}

int pdog_group_sync(pdog_group *g)
{
    if (!g) return fail(PDOG_E_ARG, "pdog_group_sync: null group");
    // EVERY rank is drained (and its raised flags cleared) whatever the others report; the first error is returned
    int first = PDOG_OK;
    std::string text;
    for (int r = 0; r < g->ndev; ++r) {
        const int rc = pdog_sync(g->tr[r]);
        if (rc && !first) { first = rc; text = "rank " + std::to_string(r) + ": " + pdog_last_error(); }
    }
    return first ? fail(first, text) : PDOG_OK;
}

// Test hook (tests/test_gpu_group.py): the copy kernel that compacts the gathered max-shard-sized blocks when the shards are
// unequal, on synthetic gathered buffers (with one rank the shards are always equal).
// d_gathered: int32[ndev][max_n][2] with max_n = ⌈n_total / ndev⌉; d_out: int32[n_total][2]; both on the current device.
int pdog_group_test_compact(const int32_t *d_gathered, int n_total, int ndev, int32_t *d_out)
{
    if (!d_gathered || !d_out || n_total <= 0 || ndev <= 0) return fail(PDOG_E_ARG, "pdog_group_test_compact: bad argument");
    const int max_n = (n_total + ndev - 1) / ndev;
    hipLaunchKernelGGL(group_compact_kernel, dim3((n_total + 255) / 256), dim3(256), 0, 0, d_gathered, d_out, n_total, ndev, max_n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    return PDOG_OK;
}

// Test hook (tests/test_gpu_group_ranks.py): a group of nranks trackers that all live on `device`, each with its own stream, over
// the local transport above — librccl is not opened.  Every other pdog_group_* call takes the handle as it takes
// pdog_group_create's.  Reachable through this entry alone: no environment variable and no tuning key selects the transport.
int pdog_group_test_create_local(int nranks, int device, int frame_h, int frame_w, double target_width, int win_h, int win_w,
                                 int darker_target, int fill, pdog_group **out)
{
    if (!out) return fail(PDOG_E_ARG, "pdog_group_test_create_local: out is null");
    *out = nullptr;
    if (nranks <= 0 || nranks > 64) return fail(PDOG_E_ARG, "pdog_group_test_create_local: nranks must be 1 … 64");
    int have = 0;
    if (hipGetDeviceCount(&have) != hipSuccess || have <= 0)
        return fail(PDOG_E_NODEV, "pdog_group_test_create_local: no HIP device (this library has no CPU path)");
    if (device < 0 || device >= have)
        return fail(PDOG_E_NODEV, "pdog_group_test_create_local: device ordinal " + std::to_string(device) + " requested, " + std::to_string(have) + " visible");
    pdog_group *g = new pdog_group();
    g->ndev = nranks;
    g->net = &local_transport();
    g->dev.assign(nranks, device);
    return group_finish_create(g, "pdog_group_test_create_local", frame_h, frame_w, target_width, win_h, win_w, darker_target, fill, out);
}

} // extern "C"
