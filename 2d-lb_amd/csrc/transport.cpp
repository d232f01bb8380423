// transport.cpp -- what connects a slab handle to its neighbours: the RCCL loader and lb_comm_*, and the peer transport's set-up
// (lb_peer_export / lb_peer_connect).  The exchanges themselves: slab.cpp.
#include "host.h"

#include <dlfcn.h>
#include <unistd.h>

// ------------------------------------------------------------------------------------------
//  RCCL, loaded lazily so that single-GPU use never touches librccl (struct Rccl, NCCL_TRY: host.h)
// ------------------------------------------------------------------------------------------
Rccl g_rccl;

int rccl_load()
{
    if (g_rccl.lib) return LB_OK;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return fail(LB_ERR_COMM, "cannot load librccl.so: %s", dlerror());
#define SYM(field, name)                                                                     \
    *(void **)(&g_rccl.field) = dlsym(h, name);                                              \
    if (!g_rccl.field) return fail(LB_ERR_COMM, "librccl.so lacks %s", name)
    SYM(GetUniqueId, "ncclGetUniqueId");
    SYM(CommInitRank, "ncclCommInitRank");
    SYM(CommDestroy, "ncclCommDestroy");
    SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd");
    SYM(Send, "ncclSend");
    SYM(Recv, "ncclRecv");
    SYM(AllReduce, "ncclAllReduce");
    SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.lib = h;
    return LB_OK;
}

extern "C" {

// ---- RCCL --------------------------------------------------------------------------------
int lb_comm_available(void) { return rccl_load(); }

int lb_comm_unique_id(void *unique_id_128)
{
    if (!unique_id_128) return fail(LB_ERR_ARG, "null argument");
    int rc = rccl_load();
    if (rc) return rc;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    NCCL_TRY(g_rccl.GetUniqueId(&id));
    memcpy(unique_id_128, &id, sizeof(id));
    return LB_OK;
}

int lb_comm_init(lb_sim *s, const void *unique_id_128, int rank, int nranks)
{
    CPU_UNSUPPORTED(s, "lb_comm_init");
    SCALAR_UNSUPPORTED(s, "lb_comm_init");
    if (!s || !unique_id_128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(LB_ERR_ARG, "bad argument");
    int rc = rccl_load();
    if (rc) return rc;
    DeviceGuard guard(s->p.device);
    ncclUniqueId id;
    memcpy(&id, unique_id_128, sizeof(id));
    if ((rc = ensure_halo_buf(s))) return rc;
    // (RCCL's channel count.  Left alone, RCCL spreads the two sends and receives of an exchange -- 14 rows x 3 populations per direction,
    //  ~1.4 MB at 8192 columns -- over 59 workgroups of 256 threads with 20-37 KB of LDS each; k_deep's workgroups hold a CU's whole LDS
    //  in pairs, so those 59 trickle in as slots come free, sit on the SIMDs of an issue-bound kernel for most of a launch and take slots
    //  from the band launch behind them: one slab of four of an 8192^2 lattice 381 k MLUPS, with NCCL_MAX_NCHANNELS=2..16 438-450 k
    //  (profiles/r06c_slab_proxy_channels.txt, timeline profiles/r06c_slab_timeline_rccl_4.txt).  The per-communicator form of that cap,
    //  ncclConfig_t::maxCTAs through ncclCommInitRankConfig, is accepted and IGNORED by RCCL 2.26 / 2.27 (59 workgroups still:
    //  profiles/r06c_slab_timeline_rccl_4_cap8.txt), and the environment variable is read once per process at the first communicator's
    //  creation -- usually the caller's.  So the cap is the caller's to set before anything touches RCCL; neither this library nor
    //  bench.py sets it, and INTEGRATION.md explains why RCCL's default is left alone.)
    NCCL_TRY(g_rccl.CommInitRank(&s->comm, nranks, id, rank));
    if (!s->peer_connected()) s->transport = SLAB_RCCL;
    s->rank = rank;
    s->nranks = nranks;
    // Which fused kernels a slab can run depends on its height; neighbours must exchange in the same
    // rhythm, so the ranks agree on the smallest height once, here.
    {
        int *d = reinterpret_cast<int *>(s->halo_buf);
        HIP_TRY(hipMemcpyAsync(d, &s->H, sizeof(int), hipMemcpyHostToDevice, s->edge_stream));
        NCCL_TRY(g_rccl.AllReduce(d, d + 1, 1, ncclInt32, ncclMin, s->comm, s->edge_stream));
        HIP_TRY(hipMemcpyAsync(&s->min_h, d + 1, sizeof(int), hipMemcpyDeviceToHost, s->edge_stream));
        HIP_TRY(hipStreamSynchronize(s->edge_stream));
    }
    s->ghost_depth = 0;
    return LB_OK;
}

// ---- peer transport ----------------------------------------------------------------------
namespace {
struct PeerDesc {                      // what lb_peer_export hands out (<= LB_PEER_HANDLE_BYTES)
    uint32_t magic, version;
    int32_t pid, device;
    int32_t nx, ny, h, planar;
    int64_t pitch, rowp, plane, lat_floats;
    uint64_t self_lat[2], self_flags;  // the exporter's own pointers: meaningful inside the exporting process only
    hipIpcMemHandle_t lat[2], flags;
};
static_assert(sizeof(PeerDesc) <= LB_PEER_HANDLE_BYTES, "LB_PEER_HANDLE_BYTES too small");
constexpr uint32_t PEER_MAGIC = 0x4c425052u;    // "LBPR"
}  // namespace

int lb_peer_export(lb_sim *s, void *handle_out)
{
    CPU_UNSUPPORTED(s, "lb_peer_export");
    SCALAR_UNSUPPORTED(s, "lb_peer_export");
    if (!s || !handle_out) return fail(LB_ERR_ARG, "null argument");
    if (!s->multi_slab()) return fail(LB_ERR_STATE, "lb_peer_export needs a slab handle (LB_FLAG_HALO)");
    DeviceGuard guard(s->p.device);
    if (!s->peer_flags) {
        // fine-grained device memory: the neighbours' system-scope stores must become visible to a kernel that is already
        // running here (the bulk rows, ordinary coarse-grained memory, only have to be visible at kernel boundaries)
        void *f = nullptr;
        const size_t bytes = peer_flag_bytes;
        if (hipExtMallocWithFlags(&f, bytes, hipDeviceMallocFinegrained) == hipSuccess) s->peer_flags_fine = true;
        else {
            (void)hipGetLastError();
            HIP_TRY(hipMalloc(&f, bytes));
        }
        s->peer_flags = static_cast<unsigned long long *>(f);
        HIP_TRY(hipMemset(s->peer_flags, 0, bytes));
    }
    PeerDesc d;
    memset(&d, 0, sizeof(d));
    d.magic = PEER_MAGIC; d.version = LB_ABI_VERSION;
    d.pid = (int32_t)getpid(); d.device = s->p.device;
    d.nx = s->p.nx; d.ny = s->p.ny; d.h = s->H; d.planar = (s->p.flags & LB_FLAG_PLANAR) ? 1 : 0;
    d.pitch = s->pitch; d.rowp = s->rowp; d.plane = s->plane; d.lat_floats = s->lat_floats;
    d.self_lat[0] = (uint64_t)(uintptr_t)s->lat[0]; d.self_lat[1] = (uint64_t)(uintptr_t)s->lat[1];
    d.self_flags = (uint64_t)(uintptr_t)s->peer_flags;
    HIP_TRY(hipIpcGetMemHandle(&d.lat[0], s->lat[0]));
    HIP_TRY(hipIpcGetMemHandle(&d.lat[1], s->lat[1]));
    if (hipIpcGetMemHandle(&d.flags, s->peer_flags) != hipSuccess && s->peer_flags_fine) {
        // (a runtime that cannot export fine-grained memory: fall back to an ordinary allocation -- enough between processes
        //  that share one GPU, where the flags meet in that GPU's own memory)
        (void)hipGetLastError();
        (void)hipFree(s->peer_flags);
        s->peer_flags = nullptr;
        s->peer_flags_fine = false;
        void *f = nullptr;
        HIP_TRY(hipMalloc(&f, peer_flag_bytes));
        s->peer_flags = static_cast<unsigned long long *>(f);
        HIP_TRY(hipMemset(s->peer_flags, 0, peer_flag_bytes));
        d.self_flags = (uint64_t)(uintptr_t)s->peer_flags;
        HIP_TRY(hipIpcGetMemHandle(&d.flags, s->peer_flags));
    }
    memset(handle_out, 0, LB_PEER_HANDLE_BYTES);
    memcpy(handle_out, &d, sizeof(d));
    return LB_OK;
}

int lb_peer_connect(lb_sim *s, int rank, int nranks, const void *south_handle, const void *north_handle, int min_h)
{
    CPU_UNSUPPORTED(s, "lb_peer_connect");
    SCALAR_UNSUPPORTED(s, "lb_peer_connect");
    if (!s || nranks < 1 || rank < 0 || rank >= nranks || min_h < 1) return fail(LB_ERR_ARG, "bad argument");
    if (!s->peer_flags) return fail(LB_ERR_STATE, "lb_peer_connect before lb_peer_export");
    if (s->peer_connected() || s->comm) return fail(LB_ERR_STATE, "this handle already has a halo transport");
    DeviceGuard guard(s->p.device);
    const void *handles[2] = {south_handle, north_handle};
    PeerDesc d[2];
    for (int side = 0; side < 2; ++side) {
        if (!handles[side]) continue;
        memcpy(&d[side], handles[side], sizeof(PeerDesc));
        const PeerDesc &e = d[side];
        if (e.magic != PEER_MAGIC || e.version != LB_ABI_VERSION)
            return fail(LB_ERR_ARG, "not a peer descriptor of this library version");
        if (e.nx != s->p.nx || e.ny != s->p.ny || e.pitch != s->pitch || e.planar != ((s->p.flags & LB_FLAG_PLANAR) ? 1 : 0))
            return fail(LB_ERR_ARG, "the %s neighbour's lattice has another geometry or layout", side ? "north" : "south");
    }
    for (int side = 0; side < 2; ++side) {
        lb_sim::PeerNb &nb = s->peer_nb[side];
        if (!handles[side]) continue;
        const PeerDesc &e = d[side];
        nb.plane = e.plane; nb.rowp = e.rowp; nb.h = e.h;
        if (e.pid == (int32_t)getpid()) {              // exported by this process (a ring that closes on itself): use it in place
            nb.flags = reinterpret_cast<unsigned long long *>((uintptr_t)e.self_flags);
            nb.lat_raw[0] = reinterpret_cast<float *>((uintptr_t)e.self_lat[0]);
            nb.lat_raw[1] = reinterpret_cast<float *>((uintptr_t)e.self_lat[1]);
            continue;
        }
        if (side == 1 && handles[0] && d[0].pid == e.pid && d[0].self_flags == e.self_flags) {
            // two ranks in a periodic box: both neighbours are the same peer; one mapping serves both sides
            nb.flags = s->peer_nb[0].flags; nb.lat_raw[0] = s->peer_nb[0].lat_raw[0]; nb.lat_raw[1] = s->peer_nb[0].lat_raw[1];
            continue;
        }
        void *m = nullptr;
        HIP_TRY(hipIpcOpenMemHandle(&m, e.flags, hipIpcMemLazyEnablePeerAccess));
        nb.flags = static_cast<unsigned long long *>(m);
        nb.mapped = true;
        for (int w = 0; w < 2; ++w) {
            HIP_TRY(hipIpcOpenMemHandle(&m, e.lat[w], hipIpcMemLazyEnablePeerAccess));
            nb.lat_raw[w] = static_cast<float *>(m);
        }
    }
    {       // (lb_check's scratch and the launch-by-launch fallback share it with the RCCL path)
        int rc = ensure_halo_buf(s);
        if (rc) return rc;
    }
    double timeout_s = 20.0;
    if (const char *t = getenv("LB_PEER_TIMEOUT_S")) timeout_s = atof(t) > 0 ? atof(t) : timeout_s;
    s->peer_timeout_ticks = (unsigned long long)(timeout_s * 1e8);         // s_memrealtime: 100 MHz
    s->rank = rank;
    s->nranks = nranks;
    s->min_h = min_h;
    s->ghost_depth = 0;
    s->transport = SLAB_PEER;
    return LB_OK;
}

}  // extern "C"
