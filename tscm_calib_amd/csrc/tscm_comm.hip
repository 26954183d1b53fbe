// tscm_comm.hip -- the exchange back-ends of the frame-sharded solve behind one interface (tscm_comm.h), and the
// tscm_comm_* entry points of the C ABI.  Whether a communicator can still be used (comm_usable) and how it stops being
// usable (retire) are decided here and nowhere else.
#include "tscm/tscm.h"
#include "tscm_comm.h"
#include "tscm_host.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <memory>
#include <string>
#include <thread>

using namespace tscm;

#define NCCL_TRY(expr)                                                                                 \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess)                                                                         \
            return tscm_set_error(TSCM_E_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));   \
    } while (0)

// Exchange backends of the frame-sharded solve.  RCCL: one process per GPU (the production path).  LOCAL: all ranks
// live in ONE process on ONE device and share a stream -- the all-reduce is a kernel that sums the ranks' buffers in
// rank order (tscm_comm_create_local / tscm_solver_solve_group): it runs every line of the sharded solver on a
// one-GPU box (RCCL refuses two ranks on one device) and serves hosts that drive several shards from one thread.
struct tscm_local_group {
    int world = 0, device = 0, refs = 0;
    hipStream_t stream = nullptr;
    double **d_ptrs = nullptr;           // [2 world] device array of the members' exchange buffers (comm_group_bind)
    DeviceMem mem;                       // owns d_ptrs
    ~tscm_local_group() { if (stream) (void)hipStreamDestroy(stream); }
};
// IPC: one process per rank like RCCL, but the exchange is this library's own one-shot all-reduce over memory the ranks
// map from each other (hipIpcMemHandle: the same device, or peers over xGMI).  Every rank owns a buffer of
// 2 (parity) x world (source rank) slots of max_doubles doubles and 2 x world arrival flags; an exchange is ONE
// single-workgroup kernel per rank: store my values into my slot of every rank's buffer, release, raise my flag there;
// wait for the world flags of my own buffer; sum the slots in rank order (the bits of the LOCAL backend, on every
// rank).  4 us where an RCCL all-reduce of 16-32 KB takes 15-25 -- and the only back-end that can put several rank
// PROCESSES on one device, which is how the multi-process path runs on a one-GPU box (tools/ipc_check.py,
// `bench.py --gpus N` with fewer devices than ranks).  Exercised between processes on ONE device only (no
// multi-GPU box in reach).  Across devices it is correct by construction since round 5 -- the buffer (slots and flags) is
// fine-grained device memory (hipExtMallocWithFlags: coherent for a peer's system-scope stores and loads), peer access is
// enabled explicitly at connect, and a rank whose buffer could only be had coarse-grained refuses peers on other devices --
// but unmeasured: RCCL stays the default.  A peer that does not arrive within the bound makes the communicator unusable
// (TSCM_E_PEER from then on, like an aborted RCCL communicator).
constexpr int kIpcMaxWorld = 16;
struct IpcPeers { double *base[kIpcMaxWorld]; };
struct tscm_ipc {
    int world = 0, rank = 0;
    size_t max_doubles = 0;             // per slot
    DeviceMem mem;                      // owns this rank's buffer and d_fault
    void *mapped[kIpcMaxWorld] = {};    // the ranks' buffers as mapped here (this rank's own at [rank])
    bool connected = false;
    long long count = 0;                // exchanges so far: parity and flag value of the next one
    int *d_fault = nullptr;             // raised by a kernel whose peers did not arrive within the bound
    bool fine = false;                  // the buffer is fine-grained memory (a peer on another device may use it)
    bool dead = false;                  // a peer fault or a failed solve: the ranks' exchange counters can no longer be trusted to agree
    size_t slot_doubles() const { return max_doubles; }
    size_t flags_offset() const { return 2 * (size_t)world * max_doubles; }        // in doubles (flags are 8-byte words)
    size_t total_bytes() const { return 8 * (flags_offset() + 2 * (size_t)world); }
};
struct tscm_comm {
    ncclComm_t comm = nullptr;           // RCCL backend; NULL again once aborted
    tscm_local_group *group = nullptr;   // LOCAL backend
    tscm_ipc *ipc = nullptr;             // IPC backend
    int rank = 0, world = 1, device = 0;
};

// ------------------------------------------------------------------------------------------------
// Per iteration the ranks exchange exactly two buffers, each with a sum all-reduce:
//   T        n_bids * 256 doubles   the Schur complement tiles, after k_T_reduce
//   H_stage  256 C + kScal + world  camera tiles, cost, model-cost / norm partials, failure flag, per-rank max slots
// ------------------------------------------------------------------------------------------------
__global__ void k_xchg_sum(double *const *bufs, int world, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    for (int r = 0; r < world; ++r) a += bufs[r][i];       // rank order: every member receives the same bits
    for (int r = 0; r < world; ++r) bufs[r][i] = a;
}

// the IPC backend's all-reduce: one workgroup of 1024 threads per rank (n <= max_doubles)
constexpr long long kIpcTimeoutTicks = 1000000000;      // 10 s of s_memrealtime (100 MHz): the start-up skew between rank processes (code-object loads of a first launch) included
__global__ __launch_bounds__(1024) void k_ipc_allreduce(double *buf, size_t n, IpcPeers peers, int rank, int world, size_t max_doubles, long long epoch, int *fault)
{
    // (a peer that has not arrived once is gone: the exchanges still enqueued behind the failed one do not wait for it again)
    if (__hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
    const int parity = (int)(epoch & 1);
    const size_t slot = ((size_t)parity * world + rank) * max_doubles, flags = 2 * (size_t)world * max_doubles;
    for (int p = 0; p < world; ++p) {
        double *dst = peers.base[p] + slot;
        for (size_t i = threadIdx.x; i < n; i += 1024) __builtin_nontemporal_store(buf[i], dst + i);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");            // (system scope: my stores are visible wherever the flag is)
    __syncthreads();
    if ((int)threadIdx.x < world) {
        long long *f = reinterpret_cast<long long *>(peers.base[threadIdx.x] + flags) + (size_t)parity * world + rank;
        __hip_atomic_store(f, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __shared__ int s_late;
    if (threadIdx.x == 0) s_late = 0;
    __syncthreads();
    if ((int)threadIdx.x < world) {
        const long long *f = reinterpret_cast<const long long *>(peers.base[rank] + flags) + (size_t)parity * world + threadIdx.x;
        const long long t0 = wall_clock64();
        while (__hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < epoch) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > kIpcTimeoutTicks) { s_late = 1; break; }
        }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    if (s_late) { if (threadIdx.x == 0) __hip_atomic_store(fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return; }
    const double *mine = peers.base[rank] + (size_t)parity * world * max_doubles;
    for (size_t i = threadIdx.x; i < n; i += 1024) {
        double a = 0.0;
        for (int r = 0; r < world; ++r) a += __builtin_nontemporal_load(mine + (size_t)r * max_doubles + i);     // rank order: every rank receives the same bits
        buf[i] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// what the solver asks (tscm_comm.h)
// ------------------------------------------------------------------------------------------------
CommKind comm_kind(const tscm_comm *c) { return !c ? kCommNone : c->world > 1 || c->group ? kCommShared : kCommOneRank; }
int comm_device(const tscm_comm *c) { return c->device; }
int comm_rank(const tscm_comm *c) { return c->rank; }
int comm_world(const tscm_comm *c) { return c->world; }
bool comm_is_local_group(const tscm_comm *c) { return c && c->group; }
bool comm_same_group(const tscm_comm *a, const tscm_comm *b) { return a && b && a->group && a->group == b->group; }

int comm_usable(const tscm_comm *c)
{
    if (c && !c->group && !c->ipc && !c->comm) return tscm_set_error(TSCM_E_RCCL, "the communicator was aborted by an earlier failure");
    if (c && c->ipc && c->ipc->dead) return tscm_set_error(TSCM_E_PEER, "the IPC communicator is unusable after an earlier failure (a peer that did not arrive, or a failed solve)");
    return 0;
}

// The only place a communicator becomes unusable.  RCCL: aborted and forgotten (unusable afterwards, like after any RCCL
// error), which the error text in place says from then on.  That does NOT unblock the peers by itself: they leave their next
// all-reduce through the watchdog of comm_wait (TSCM_E_RCCL), or are torn down by whoever started the ranks (bench.py's
// launcher ends all ranks as soon as one exits non-zero).  IPC: its exchange counter may be behind the peers' now.  A failed
// rank must not be re-used: start a fresh process.
static void retire(tscm_comm *c)
{
    if (c->ipc) c->ipc->dead = true;
    if (c->comm) {
        const std::string keep = tscm_last_error();
        (void)ncclCommAbort(c->comm);
        c->comm = nullptr;
        tscm_set_error(0, keep + " (communicator aborted)");
    }
}
void comm_fail(tscm_comm *c) { if (c && c->world > 1) retire(c); }

int comm_allreduce(tscm_comm *c, double *buf, size_t n, hipStream_t stream)
{
    if (c->ipc) {
        tscm_ipc *x = c->ipc;
        if (!x->connected) return tscm_set_error(TSCM_E_INVALID, "tscm_comm_ipc_connect has not been called");
        if (int rc = comm_usable(c)) return rc;
        IpcPeers peers{};
        for (int r = 0; r < x->world; ++r) peers.base[r] = static_cast<double *>(x->mapped[r]);
        for (size_t off = 0; off < n; off += x->max_doubles) {
            const size_t m = std::min(x->max_doubles, n - off);
            hipLaunchKernelGGL(k_ipc_allreduce, dim3(1), dim3(1024), 0, stream, buf + off, m, peers, x->rank, x->world, x->max_doubles, ++x->count, x->d_fault);
        }
        return 0;
    }
    NCCL_TRY(ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, c->comm, stream));
    return 0;
}

int comm_check(tscm_comm *c)
{
    if (!c || !c->ipc) return 0;
    int f = 0;
    HIP_TRY(hipMemcpy(&f, c->ipc->d_fault, sizeof(int), hipMemcpyDeviceToHost));
    if (f) { retire(c); return tscm_set_error(TSCM_E_PEER, "IPC exchange: a peer rank did not arrive within the bound (failed or gone); the communicator is unusable from here on"); }
    return 0;
}

// With a multi-rank RCCL communicator a peer that has failed (or died) leaves this rank's all-reduce kernel spinning for
// ever -- over the intra-node transports an ncclCommAbort on the FAILING rank does not reach the others -- so the wait is
// a poll with a watchdog: no completion within kCommWatchdogSeconds aborts the communicator locally and fails the call
// with TSCM_E_RCCL.  (A whole solve of the largest supported problem is well under a second of device time; the bound only
// has to exceed the start-up skew between the rank processes.)
constexpr double kCommWatchdogSeconds = 60.0;
int comm_wait(tscm_comm *c, hipStream_t stream)
{
    if (!c || c->group || !c->comm || c->world <= 1) { HIP_TRY(hipStreamSynchronize(stream)); return 0; }
    const double t0 = wall();
    for (;;) {
        const hipError_t q = hipStreamQuery(stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady) { HIP_TRY(q); }
        if (wall() - t0 > kCommWatchdogSeconds) {
            const int rc = tscm_set_error(TSCM_E_RCCL, "no progress on the solver stream within the watchdog interval: a peer rank has failed or is gone");
            retire(c);
            return rc;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

hipStream_t comm_group_stream(const tscm_comm *c) { return c->group->stream; }

int comm_group_bind(tscm_comm *c, const std::vector<double *> &ptrs)
{
    HIP_TRY(hipMemcpy(c->group->d_ptrs, ptrs.data(), sizeof(double *) * ptrs.size(), hipMemcpyHostToDevice));
    return 0;
}

void comm_group_sum(tscm_comm *c, bool t_buffer, size_t n)
{
    tscm_local_group *g = c->group;
    hipLaunchKernelGGL(k_xchg_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, g->stream, g->d_ptrs + (t_buffer ? 0 : g->world), g->world, n);
}

// ------------------------------------------------------------------------------------------------
// the C ABI's communicators
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(ncclUniqueId) <= TSCM_UNIQUE_ID_BYTES, "ncclUniqueId larger than the ABI buffer");

extern "C" int tscm_comm_unique_id(unsigned char id[TSCM_UNIQUE_ID_BYTES])
{
    if (!id) return tscm_set_error(TSCM_E_INVALID, "id is NULL");
    ncclUniqueId u;
    NCCL_TRY(ncclGetUniqueId(&u));
    std::memset(id, 0, TSCM_UNIQUE_ID_BYTES);
    std::memcpy(id, &u, sizeof(u));
    return 0;
}

extern "C" int tscm_comm_create(const unsigned char id[TSCM_UNIQUE_ID_BYTES], int rank, int world, int device, tscm_comm **out)
{
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return tscm_set_error(TSCM_E_INVALID, "bad communicator arguments");
    *out = nullptr;
    if (int rc = select_device(device, "tscm_comm_create")) return rc;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    std::unique_ptr<tscm_comm> c(new tscm_comm);
    c->rank = rank; c->world = world; c->device = device;
    NCCL_TRY(ncclCommInitRank(&c->comm, world, u, rank));
    *out = c.release();
    return 0;
}

extern "C" int tscm_comm_create_local(int world, int device, tscm_comm **out)
{
    if (!out || world < 1) return tscm_set_error(TSCM_E_INVALID, "bad communicator arguments");
    for (int r = 0; r < world; ++r) out[r] = nullptr;
    if (int rc = select_device(device, "tscm_comm_create_local")) return rc;
    std::unique_ptr<tscm_local_group> g(new tscm_local_group);
    g->world = world; g->device = device;
    HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
    if (g->mem.alloc(&g->d_ptrs, 2 * (size_t)world) != hipSuccess) return tscm_set_error(TSCM_E_NOMEM, "hipMalloc of the group's pointer table failed");
    for (int r = 0; r < world; ++r) {
        tscm_comm *c = new tscm_comm;
        c->rank = r; c->world = world; c->device = device; c->group = g.get();
        out[r] = c;
    }
    g->refs = world;
    g.release();
    return 0;
}

struct IpcIdent { int pci[3]; int fine; };
static_assert(sizeof(hipIpcMemHandle_t) + sizeof(IpcIdent) <= TSCM_IPC_HANDLE_BYTES, "hipIpcMemHandle_t + identity larger than the ABI buffer");

extern "C" int tscm_comm_ipc_open(int rank, int world, int device, size_t max_doubles, tscm_comm **out, unsigned char handle[TSCM_IPC_HANDLE_BYTES])
{
    if (!out || !handle || world < 1 || world > kIpcMaxWorld || rank < 0 || rank >= world || max_doubles == 0) return tscm_set_error(TSCM_E_INVALID, "bad communicator arguments (IPC: up to 16 ranks)");
    *out = nullptr;
    if (int rc = select_device(device, "tscm_comm_ipc_open")) return rc;
    std::unique_ptr<tscm_comm> c(new tscm_comm);
    std::unique_ptr<tscm_ipc> x(new tscm_ipc);
    c->rank = rank; c->world = world; c->device = device;
    x->rank = rank; x->world = world; x->max_doubles = (max_doubles + 1) & ~(size_t)1;
    if (x->mem.alloc(&x->d_fault, 1) != hipSuccess) return tscm_set_error(TSCM_E_NOMEM, "hipMalloc failed");
    hipIpcMemHandle_t h;
    // fine-grained first (what a peer on ANOTHER device needs for its system-scope flag stores and my loads of them to meet);
    // where that cannot be had or exported, ordinary device memory -- enough for ranks that share this device, and the handle
    // says so: a peer on another device then refuses to connect
    hipError_t e = hipErrorUnknown;
    char *own = nullptr;
    for (int attempt = 0; attempt < 2 && e != hipSuccess; ++attempt) {
        x->fine = attempt == 0;
        if (x->fine) {
            e = hipExtMallocWithFlags(reinterpret_cast<void **>(&own), x->total_bytes(), hipDeviceMallocFinegrained);
            if (e == hipSuccess) x->mem.adopt(own);
        } else {
            e = x->mem.alloc(&own, x->total_bytes());
        }
        if (e != hipSuccess) { (void)hipGetLastError(); continue; }
        e = hipMemset(own, 0, x->total_bytes());
        if (e == hipSuccess) e = hipMemset(x->d_fault, 0, sizeof(int));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipIpcGetMemHandle(&h, own);
        if (e != hipSuccess) { x->mem.release(own); (void)hipGetLastError(); }
    }
    if (e != hipSuccess) {
        return tscm_set_error(TSCM_E_HIP, std::string("IPC exchange buffer: ") + hipGetErrorString(e) + " (hipIpcGetMemHandle needs HSA_ENABLE_IPC_MODE_LEGACY=0 on hosts whose driver only supports dmabuf IPC)");
    }
    std::memset(handle, 0, TSCM_IPC_HANDLE_BYTES);
    std::memcpy(handle, &h, sizeof(h));
    {
        // behind the HIP handle: which device the buffer lives on (PCI address: ordinals differ between processes) and its kind
        IpcIdent id{};
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        id.pci[0] = prop.pciDomainID; id.pci[1] = prop.pciBusID; id.pci[2] = prop.pciDeviceID; id.fine = x->fine ? 1 : 0;
        std::memcpy(handle + sizeof(h), &id, sizeof(id));
    }
    x->mapped[rank] = own;
    tscm_set_error(0, x->fine ? "note: IPC exchange buffer in fine-grained device memory" : "note: IPC exchange buffer in ordinary device memory (ranks on this device only)");
    c->ipc = x.release();
    *out = c.release();
    return 0;
}

extern "C" int tscm_comm_ipc_connect(tscm_comm *c, const unsigned char *handles)
{
    if (!c || !c->ipc || !handles) return tscm_set_error(TSCM_E_INVALID, "not an IPC communicator");
    tscm_ipc *x = c->ipc;
    if (x->connected) return tscm_set_error(TSCM_E_INVALID, "already connected");
    HIP_TRY(hipSetDevice(c->device));
    IpcIdent me{};
    std::memcpy(&me, handles + (size_t)TSCM_IPC_HANDLE_BYTES * x->rank + sizeof(hipIpcMemHandle_t), sizeof(me));
    for (int r = 0; r < x->world; ++r) {
        if (r == x->rank) continue;
        hipIpcMemHandle_t h;
        IpcIdent id{};
        std::memcpy(&h, handles + (size_t)TSCM_IPC_HANDLE_BYTES * r, sizeof(h));
        std::memcpy(&id, handles + (size_t)TSCM_IPC_HANDLE_BYTES * r + sizeof(h), sizeof(id));
        if (std::memcmp(id.pci, me.pci, sizeof(id.pci)) != 0) {
            // a peer on another device: both buffers fine-grained, and peer access enabled here and now (not lazily)
            if (!id.fine || !x->fine) return tscm_set_error(TSCM_E_UNSUPPORTED, "IPC exchange across devices needs fine-grained exchange buffers on both ranks (one of them is ordinary device memory): put the ranks on one device or use RCCL");
            const int ndev = tscm_device_count();
            int peer = -1;
            for (int d = 0; d < ndev && peer < 0; ++d) {
                hipDeviceProp_t prop;
                HIP_TRY(hipGetDeviceProperties(&prop, d));
                if (prop.pciDomainID == id.pci[0] && prop.pciBusID == id.pci[1] && prop.pciDeviceID == id.pci[2]) peer = d;
            }
            if (peer < 0) return tscm_set_error(TSCM_E_UNSUPPORTED, "IPC exchange: a peer rank's device is not visible to this process (HIP_VISIBLE_DEVICES): no peer access");
            int can = 0;
            HIP_TRY(hipDeviceCanAccessPeer(&can, c->device, peer));
            if (!can) return tscm_set_error(TSCM_E_UNSUPPORTED, "IPC exchange: no peer access between this rank's device and a peer rank's");
            const hipError_t pe = hipDeviceEnablePeerAccess(peer, 0);
            if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled) { HIP_TRY(pe); }
            (void)hipGetLastError();
        }
        HIP_TRY(hipIpcOpenMemHandle(&x->mapped[r], h, hipIpcMemLazyEnablePeerAccess));
    }
    x->connected = true;
    return 0;
}

extern "C" int tscm_comm_info(const tscm_comm *c, int *rank, int *world, int *backend_ranks)
{
    if (!c) return tscm_set_error(TSCM_E_INVALID, "communicator is NULL");
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    if (backend_ranks) {
        int n = c->group ? c->group->world : c->ipc && c->ipc->connected ? c->ipc->world : 0;
        if (c->comm) NCCL_TRY(ncclCommCount(c->comm, &n));      // what RCCL itself reports for the communicator
        *backend_ranks = n;
    }
    return 0;
}

extern "C" void tscm_comm_destroy(tscm_comm *c)
{
    if (!c) return;
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->ipc) {
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        for (int r = 0; r < c->ipc->world; ++r) if (r != c->ipc->rank && c->ipc->mapped[r]) (void)hipIpcCloseMemHandle(c->ipc->mapped[r]);
        delete c->ipc;                  // (its DeviceMem frees the buffer and the fault word)
    }
    if (c->group && --c->group->refs == 0) {
        (void)hipSetDevice(c->group->device);
        (void)hipStreamSynchronize(c->group->stream);
        delete c->group;                // (frees the pointer table, destroys the stream)
    }
    delete c;
}
