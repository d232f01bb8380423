// kernels_halo.h -- halo pack / unpack and the kernels of the peer transport (k_halo_pack, k_halo_unpack, k_peer_pre, k_peer_post,
// k_halo_push).  Included by slab.cpp only: its plain kernels must be emitted by exactly one translation unit.
#pragma once
#include "d2q9_cell.h"

namespace {

// Halo pack / unpack: the halo of one edge is 18 (3 rows deep), 45 (6 deep), 63 (8 deep) or 81 (10 deep) row segments scattered
// over the planes (HaloTables on the host side).  One tiny kernel gathers both edges into two contiguous
// buffers (so that an exchange is one send + one receive per neighbour), one scatters the received
// buffers into the ghost rows.  `neg` lists rows -D..-1 (leaves north, counted from row H / arrives
// south, counted from row 0), `pos` rows 0..D-1 (leaves south / arrives north).
struct HaloTable {
    signed char k[117], row[117];    // (D = 14: 9 x 14 - 9 row segments)
    int n;
};

// One wave moves 1 KiB of a row segment: 16 bytes per lane when nx is a multiple of 4 (row starts and buffer segments are
// then 16-byte aligned: pitch % 64 == 0), a dword per lane otherwise.  grid = (ceil(nx / (256 * V)), segments, 2 edges).
template <int V>
__global__ void k_halo_pack(const float *origin, long long plane, int pitch, int h, int nx, float *buf_n, float *buf_s,
                            const HaloTable neg, const HaloTable pos)
{
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * V, seg = blockIdx.y, north = (blockIdx.z == 0);
    if (x >= nx) return;
    float *buf = north ? buf_n : buf_s;
    if (!buf) return;
    const int k = north ? neg.k[seg] : pos.k[seg];
    const long long row = north ? h + neg.row[seg] : pos.row[seg];
    const float *src = origin + k * plane + row * pitch + x;
    float *dst = buf + (long long)seg * nx + x;
    if (V == 4) *reinterpret_cast<f4a *>(dst) = *reinterpret_cast<const f4a *>(src);
    else *dst = *src;
}

template <int V>
__global__ void k_halo_unpack(float *origin, long long plane, int pitch, int h, int nx, const float *buf_s,
                              const float *buf_n, const HaloTable neg, const HaloTable pos)
{
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * V, seg = blockIdx.y, north = (blockIdx.z == 0);
    if (x >= nx) return;
    const float *buf = north ? buf_n : buf_s;
    if (!buf) return;
    const int k = north ? pos.k[seg] : neg.k[seg];
    const long long row = north ? h + pos.row[seg] : neg.row[seg];
    float *dst = origin + k * plane + row * pitch + x;
    const float *src = buf + (long long)seg * nx + x;
    if (V == 4) *reinterpret_cast<f4a *>(dst) = *reinterpret_cast<const f4a *>(src);
    else *dst = *src;
}

// ---- peer transport (lb_peer_export / lb_peer_connect): halo rows stored straight into the neighbours' ghost rows -------
// Every rank owns a block of flags (fine-grained device memory, mapped by both neighbours); one 64-byte line per flag:
//   READY_FROM_SOUTH / _NORTH  written by that neighbour: 2 e + w = "exchange e may be stored into my lattice w"
//                              (its kernels that read the ghost rows of exchange e - 1 are complete)
//   DATA_FROM_SOUTH / _NORTH   written by that neighbour: e = "my rows of exchange e are in your ghost rows"
//   ERR                        local: a wait gave up (lb_sync reports it)
//   COUNT, WHICH_S, WHICH_N    local: the exchange counter; the lattice index each neighbour announced for this exchange
// An exchange on the edge stream: k_peer_pre (announce + wait for the neighbours' announcements), k_halo_push (the
// stores), k_peer_post (publish + wait for the neighbours' rows).  A rank signals before it waits, in both kernels, and every
// rank runs the same sequence of exchanges, so nobody waits for somebody who waits for him.  The bulk rows are ordinary
// stores made visible by the end of k_halo_push (stream order, kernel-boundary release) before k_peer_post publishes
// them; the kernels that read them start after k_peer_post has seen the flag.  Counters live on the device: the kernel
// arguments of a cycle never change, so a captured cycle can be replayed.
enum { PEER_READY_FROM_SOUTH = 0, PEER_READY_FROM_NORTH = 8, PEER_DATA_FROM_SOUTH = 16, PEER_DATA_FROM_NORTH = 24, PEER_ERR = 32,
       PEER_COUNT = 40, PEER_WHICH_S = 48, PEER_WHICH_N = 56, PEER_FLAG_WORDS = 64 };      // (uint64 indices: 64 bytes apart)

struct PeerArgs {
    unsigned long long *mine, *south, *north;      // flag blocks: my own, my neighbours' (nullptr = wall)
    unsigned long long timeout_ticks;              // of the 100 MHz clock
    int which;                                     // pre: the lattice of mine that receives this exchange
};

__device__ __forceinline__ void peer_signal(unsigned long long *flag, unsigned long long v)
{
    __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// spin until *flag >= want (shifted right by `shift` first); returns the value seen, or 0 after the timeout
__device__ __forceinline__ unsigned long long peer_wait(unsigned long long *flag, unsigned long long want, int shift,
                                                        unsigned long long timeout_ticks)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        const unsigned long long v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((v >> shift) >= want) return v;
        if (__builtin_amdgcn_s_memrealtime() - t0 > timeout_ticks) return 0;
        __builtin_amdgcn_s_sleep(16);
    }
}

__global__ void k_peer_pre(const PeerArgs p)
{
    if (threadIdx.x != 0) return;
    const unsigned long long e = p.mine[PEER_COUNT] + 1;
    p.mine[PEER_COUNT] = e;
    const unsigned long long v = 2 * e + (unsigned)p.which;
    if (p.south) peer_signal(p.south + PEER_READY_FROM_NORTH, v);       // (I am my southern neighbour's northern one)
    if (p.north) peer_signal(p.north + PEER_READY_FROM_SOUTH, v);
    if (p.south) {
        const unsigned long long r = peer_wait(p.mine + PEER_READY_FROM_SOUTH, e, 1, p.timeout_ticks);
        if (!r) p.mine[PEER_ERR] = e;
        p.mine[PEER_WHICH_S] = r & 1;
    }
    if (p.north) {
        const unsigned long long r = peer_wait(p.mine + PEER_READY_FROM_NORTH, e, 1, p.timeout_ticks);
        if (!r) p.mine[PEER_ERR] = e;
        p.mine[PEER_WHICH_N] = r & 1;
    }
}

__global__ void k_peer_post(const PeerArgs p)
{
    if (threadIdx.x != 0) return;
    const unsigned long long e = p.mine[PEER_COUNT];
    __threadfence_system();
    if (p.south) peer_signal(p.south + PEER_DATA_FROM_NORTH, e);
    if (p.north) peer_signal(p.north + PEER_DATA_FROM_SOUTH, e);
    if (p.south && !peer_wait(p.mine + PEER_DATA_FROM_SOUTH, e, 0, p.timeout_ticks)) p.mine[PEER_ERR] = e;
    if (p.north && !peer_wait(p.mine + PEER_DATA_FROM_NORTH, e, 0, p.timeout_ticks)) p.mine[PEER_ERR] = e;
}

// My edge rows -> the neighbours' ghost rows.  Same segment tables as k_halo_pack / k_halo_unpack (entry i of an OUT table
// pairs with entry i of the neighbour's IN table); the destination lattice of each neighbour is the one it announced.
struct PeerDst {
    float *lat[2];          // plane 0, row 0, x 0 of the neighbour's two lattices (mapped into this process); nullptr = wall
    long long plane, rowp;  // its strides
    int h;                  // its height (a southern neighbour's north ghost rows start at its row h)
};
template <int V>
__global__ void k_halo_push(const float *origin, long long plane, int pitch, int h, int nx, const unsigned long long *mine,
                            const PeerDst to_n, const PeerDst to_s, const HaloTable neg, const HaloTable pos)
{
    const int x = (blockIdx.x * blockDim.x + threadIdx.x) * V, seg = blockIdx.y, north = (blockIdx.z == 0);
    if (x >= nx) return;
    const PeerDst &d = north ? to_n : to_s;
    if (!d.lat[0]) return;
    const int w = (int)mine[north ? PEER_WHICH_N : PEER_WHICH_S];
    // north edge out = my rows h-D..h-1 (neg, +h) -> its south ghost rows -D..-1 (neg, +0);
    // south edge out = my rows 0..D-1 (pos) -> its north ghost rows (pos, + its h)
    const int k = north ? neg.k[seg] : pos.k[seg];
    const long long rs = north ? h + neg.row[seg] : pos.row[seg];
    const long long rd = north ? neg.row[seg] : d.h + pos.row[seg];
    const float *src = origin + k * plane + rs * pitch + x;
    float *dst = d.lat[w] + k * d.plane + rd * d.rowp + x;
    if (V == 4) *reinterpret_cast<f4a *>(dst) = *reinterpret_cast<const f4a *>(src);
    else *dst = *src;
}

}  // namespace
