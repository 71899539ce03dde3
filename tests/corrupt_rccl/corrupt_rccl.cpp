// corrupt_rccl.cpp -- TEST DOUBLE: a transport that damages ONE received piece, in front of another transport.
//
// Why: the exchange of mumemto_amd/csrc/dist.cpp verifies every message with digests because a library has
// been measured to deliver a piece with half its elements changed and no error.  A check that never sees a damaged piece
// shows nothing, so this shim exports the ten RCCL symbols dist.cpp binds, forwards every call to the library named by
// CORRUPT_RCCL_INNER (tests/fake_rccl/libfake_rccl.so) and, with
//     CORRUPT_RCCL_PLAN=rank:dtype:ordinal:mode
// damages one piece: on communicator rank `rank`, the `ordinal`-th ncclRecv (0-based) of datatype `dtype` (u8, u32, i64, u64)
// that has at least two elements.  The damage is done AFTER the inner call that completes the receive has returned -- the
// outermost ncclGroupEnd, or the ncclRecv itself outside a group (the inner transport is synchronous there) -- by a copy
// through the host.  Modes: flip = xor 1 into the lowest bit of the middle element; swap = exchange the first and the second
// half of the piece; zero_tail = zero the second half (the shape of the loss measured in round 6).  Without a plan the shim
// is transparent.  State is kept per communicator (rank, receives counted) and per thread (group depth, the piece to
// damage), as the inner double keeps its own: ranks may share a process, each on a thread of its own.
//
// Selected with MUMEMTO_RCCL_LIB=<path to this .so>.  Not a transport anybody should use for anything but tests.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

struct Inner {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

Inner* inner() {
    static Inner in;
    static std::once_flag once;
    std::call_once(once, [] {
        const char* path = std::getenv("CORRUPT_RCCL_INNER");
        void* h = path ? dlopen(path, RTLD_NOW | RTLD_LOCAL) : nullptr;
        if (!h) { std::fprintf(stderr, "corrupt rccl: cannot load CORRUPT_RCCL_INNER (%s): %s\n", path ? path : "unset", path ? dlerror() : ""); return; }
        bool all = true;
        auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) { std::fprintf(stderr, "corrupt rccl: the inner library lacks %s\n", n); all = false; } return p; };
        in.GetUniqueId = reinterpret_cast<decltype(in.GetUniqueId)>(sym("ncclGetUniqueId"));
        in.CommInitRank = reinterpret_cast<decltype(in.CommInitRank)>(sym("ncclCommInitRank"));
        in.CommDestroy = reinterpret_cast<decltype(in.CommDestroy)>(sym("ncclCommDestroy"));
        in.Broadcast = reinterpret_cast<decltype(in.Broadcast)>(sym("ncclBroadcast"));
        in.AllGather = reinterpret_cast<decltype(in.AllGather)>(sym("ncclAllGather"));
        in.Send = reinterpret_cast<decltype(in.Send)>(sym("ncclSend"));
        in.Recv = reinterpret_cast<decltype(in.Recv)>(sym("ncclRecv"));
        in.GroupStart = reinterpret_cast<decltype(in.GroupStart)>(sym("ncclGroupStart"));
        in.GroupEnd = reinterpret_cast<decltype(in.GroupEnd)>(sym("ncclGroupEnd"));
        in.GetErrorString = reinterpret_cast<decltype(in.GetErrorString)>(sym("ncclGetErrorString"));
        if (all) in.handle = h;
    });
    return in.handle ? &in : nullptr;
}

enum Mode { FLIP, SWAP, ZERO_TAIL };
struct Plan { bool on = false; int rank = 0; ncclDataType_t type = ncclUint8; size_t width = 1; uint64_t ordinal = 0; Mode mode = FLIP; };

const Plan& plan() {
    static const Plan p = [] {
        Plan q;
        const char* e = std::getenv("CORRUPT_RCCL_PLAN");
        if (!e || !*e) return q;
        char dtype[16] = {0}, mode[16] = {0};
        unsigned long long ordinal = 0;
        if (std::sscanf(e, "%d:%15[^:]:%llu:%15s", &q.rank, dtype, &ordinal, mode) != 4) {
            std::fprintf(stderr, "corrupt rccl: CORRUPT_RCCL_PLAN wants rank:dtype:ordinal:mode, got %s\n", e);
            std::abort();
        }
        const std::string d = dtype, m = mode;
        if (d == "u8") { q.type = ncclUint8; q.width = 1; }
        else if (d == "u32") { q.type = ncclUint32; q.width = 4; }
        else if (d == "i64") { q.type = ncclInt64; q.width = 8; }
        else if (d == "u64") { q.type = ncclUint64; q.width = 8; }
        else { std::fprintf(stderr, "corrupt rccl: dtype u8, u32, i64 or u64, got %s\n", dtype); std::abort(); }
        if (m == "flip") q.mode = FLIP;
        else if (m == "swap") q.mode = SWAP;
        else if (m == "zero_tail") q.mode = ZERO_TAIL;
        else { std::fprintf(stderr, "corrupt rccl: mode flip, swap or zero_tail, got %s\n", mode); std::abort(); }
        q.ordinal = ordinal; q.on = true;
        return q;
    }();
    return p;
}

// per communicator: its rank and the receives of the plan's datatype counted so far
struct CommState { int rank = 0; uint64_t seen = 0; };
std::mutex g_mu;
std::map<ncclComm_t, CommState> g_comms;

// per thread: the group it is in and the piece to damage when the group completes
struct Target { void* buf; size_t count; hipStream_t stream; int rank; };
thread_local int g_depth = 0;
thread_local std::vector<Target> g_pending;

ncclResult_t damage(const Target& t) {
    const Plan& p = plan();
    const size_t bytes = t.count * p.width, half = t.count / 2;
    std::vector<unsigned char> host(bytes);
    if (hipStreamSynchronize(t.stream) != hipSuccess) return ncclUnhandledCudaError;
    if (hipMemcpy(host.data(), t.buf, bytes, hipMemcpyDeviceToHost) != hipSuccess) return ncclUnhandledCudaError;
    if (p.mode == FLIP) host[half * p.width] ^= 1;                                 // (little endian: the element's lowest bit)
    else if (p.mode == SWAP) {
        std::vector<unsigned char> first(host.begin(), host.begin() + half * p.width);
        std::memcpy(host.data(), host.data() + half * p.width, half * p.width);
        std::memcpy(host.data() + half * p.width, first.data(), half * p.width);
    } else std::memset(host.data() + half * p.width, 0, bytes - half * p.width);
    if (hipMemcpy(t.buf, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return ncclUnhandledCudaError;
    std::fprintf(stderr, "corrupt rccl: rank %d: damaged a received piece of %zu bytes (%s)\n", t.rank, bytes,
                 p.mode == FLIP ? "flip" : p.mode == SWAP ? "swap" : "zero_tail");
    return ncclSuccess;
}

ncclResult_t damage_pending() {
    std::vector<Target> todo;
    todo.swap(g_pending);
    for (const Target& t : todo) { const ncclResult_t r = damage(t); if (r != ncclSuccess) return r; }
    return ncclSuccess;
}

}  // namespace

#define EXPORT extern "C" __attribute__((visibility("default")))
#define INNER_OR_FAIL Inner* in = inner(); if (!in) return ncclSystemError

EXPORT ncclResult_t ncclGetUniqueId(ncclUniqueId* id) { INNER_OR_FAIL; return in->GetUniqueId(id); }

EXPORT ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank) {
    INNER_OR_FAIL;
    const ncclResult_t r = in->CommInitRank(comm, nranks, id, rank);
    if (r == ncclSuccess) { std::lock_guard<std::mutex> lock(g_mu); CommState s; s.rank = rank; g_comms[*comm] = s; }
    return r;
}

EXPORT ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    INNER_OR_FAIL;
    { std::lock_guard<std::mutex> lock(g_mu); g_comms.erase(comm); }
    return in->CommDestroy(comm);
}

EXPORT ncclResult_t ncclSend(const void* buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t s) {
    INNER_OR_FAIL;
    return in->Send(buf, count, t, peer, comm, s);
}

EXPORT ncclResult_t ncclRecv(void* buf, size_t count, ncclDataType_t t, int peer, ncclComm_t comm, hipStream_t s) {
    INNER_OR_FAIL;
    const ncclResult_t r = in->Recv(buf, count, t, peer, comm, s);
    const Plan& p = plan();
    if (r != ncclSuccess || !p.on || t != p.type || count < 2) return r;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        auto it = g_comms.find(comm);
        if (it == g_comms.end() || it->second.rank != p.rank) return r;
        if (it->second.seen++ != p.ordinal) return r;
    }
    g_pending.push_back(Target{buf, count, s, p.rank});
    return g_depth > 0 ? r : damage_pending();
}

EXPORT ncclResult_t ncclBroadcast(const void* sendbuf, void* recvbuf, size_t count, ncclDataType_t t, int root, ncclComm_t comm, hipStream_t s) {
    INNER_OR_FAIL;
    return in->Broadcast(sendbuf, recvbuf, count, t, root, comm, s);
}

EXPORT ncclResult_t ncclAllGather(const void* sendbuf, void* recvbuf, size_t sendcount, ncclDataType_t t, ncclComm_t comm, hipStream_t s) {
    INNER_OR_FAIL;
    return in->AllGather(sendbuf, recvbuf, sendcount, t, comm, s);
}

EXPORT ncclResult_t ncclGroupStart() {
    INNER_OR_FAIL;
    const ncclResult_t r = in->GroupStart();
    if (r == ncclSuccess) g_depth++;
    return r;
}

EXPORT ncclResult_t ncclGroupEnd() {
    INNER_OR_FAIL;
    const ncclResult_t r = in->GroupEnd();
    if (g_depth > 0) g_depth--;
    if (r != ncclSuccess) { g_pending.clear(); return r; }
    return g_depth == 0 ? damage_pending() : r;
}

EXPORT const char* ncclGetErrorString(ncclResult_t r) {
    Inner* in = inner();
    return in ? in->GetErrorString(r) : "corrupt rccl: the inner library (CORRUPT_RCCL_INNER) could not be loaded";
}
