// Mesh path report (include/gsim.h gsim_mesh_paths): hop distances over the
// mesh of one topic from up to 64 sources at once, with the peers of some
// classes not relaying (a read-only what-if).  The distances are those of the
// routers' eager push: a message goes to gs.mesh[topic], or from a publisher
// outside the topic to gs.fanout[topic] (gossipsub.go:975-1045), a hop a round.
//
// A level-synchronous, bit-parallel traversal.  Every local peer has three
// u64 words, bit s for source s: seen (a distance is known), cur (the frontier:
// expanded at this level) and nxt (what the level's expansion reached).  A
// level is two ordinary launches, no cooperative launch and no grid-wide spin:
//
// Push, over the owned rows by the heartbeat's row classes (row_classes), as
// the network report's mesh pass:
//   k_mp_push<W>       a lane group of W lanes per row of at most W
//                      connections, lane gl on edge row_ptr[i] + gl.  A row
//                      whose cur word is zero leaves after that one 8-byte
//                      load.  An active row reads its topic plane's bytes
//                      contiguously along the row, and col[e] with them (one
//                      wait); for every edge with the mesh bit (the fanout bit
//                      where the row does not announce the topic: a seed at
//                      level 0) sub[j] and seen[j] leave together (one wait)
//                      and atomicOr(&nxt[j], cur[i]) is issued unless j does
//                      not announce the topic or seen[j] already covers cur[i].
//   k_mp_push_hub      a block per row of more than 64 connections, 256 edges
//                      per step, the same per edge.
// OR is commutative, so nxt does not depend on scheduling.  No ballot, no LDS.
//
// Fold, over the local peers in order (coalesced 8-byte words):
//   k_mp_fold          new = nxt (| the bits other shards sent) & ~seen;
//                      seen |= new; cur = new, or 0 for a peer of a blocked
//                      class (level 0 keeps every seed: a source forwards its
//                      own publication); nxt = 0.  Per source bit present in
//                      the wave the new peers are counted by ballot and
//                      popcount, per class, into the block's LDS counters
//                      [64][4]; at block end one global atomic per non-zero
//                      counter into hist[level], reached_cls and max_hops
//                      (atomicMax).  reach_count / hop_sum: the peer's own
//                      thread adds, no atomic.  The OR of the block's cur words
//                      goes to the level's "frontier left" word with one
//                      atomicOr per block; the host reads that word (8 bytes,
//                      a counted synchronisation) to end the loop.  Level 0
//                      also counts the subscribers by class.
// cls[] is read (per peer, coalesced, never gathered along a row) only when
// there is more than one class.  A shard folds the peers it owns and clears
// the nxt words of its ghosts, which the host has read by then (shard.hip).
//
// Bytes per level: the push reads 8 bytes per owned row, and per active row
// its row_ptr / sub / smask words, 5 bytes per connection (plane byte, col)
// and 16 per mesh link (sub, seen of the neighbour) plus the atomic; the fold
// reads 16 and writes 8 to 24 bytes per peer.
//
// Every result is an integer count, a maximum or an OR: no dependence on
// scheduling.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch
// or spills; the ranges span the Dense / slot-plane instances (push) and the
// one-class / classes and level-0 instances (fold):
//   k_mp_push<16|32|64>  16-20 VGPRs, 38-44 SGPRs, no LDS, 8 waves/SIMD
//   k_mp_push_hub        14 VGPRs, 35-44 SGPRs, no LDS, 8 waves/SIMD
//   k_mp_fold            26-30 VGPRs, 60-70 SGPRs, 1032-1048 bytes of LDS, 8 waves/SIMD
//   k_mp_seed            11 VGPRs, 14 SGPRs, no LDS
// Measured: DESIGN.md §7.
#include <algorithm>
#include <cstring>
#include <vector>

#include "report_common.h"

namespace gsim {

// per source counters (u32), then the subscribers by class
enum : int {
    PA_HIST = 0,                               // [GSIM_REPORT_BINS]
    PA_RCLS = GSIM_REPORT_BINS,                // [GSIM_NET_CLASSES]
    PA_MAXH = PA_RCLS + GSIM_NET_CLASSES,
    kPA = 40,
    PA_MEMBERS = GSIM_PATH_SOURCES * kPA,      // [GSIM_NET_CLASSES]
    kPathAcc = PA_MEMBERS + GSIM_NET_CLASSES,
};
static_assert(PA_MAXH < kPA, "a source's counters fit its stride");

struct MeshPaths {
    uint64_t* d_words = nullptr;               // [3][n] seen, cur, nxt
    uint64_t* d_inc = nullptr;                 // [owned] bits from other shards (a shard only)
    uint32_t* d_acc = nullptr;                 // [kPathAcc]
    unsigned long long* d_any = nullptr;       // [2] by the level's parity
    uint32_t* d_pp = nullptr;                  // [2][n] reach_count, hop_sum
    // the call in progress (meshpaths_begin .. meshpaths_finish)
    int32_t topic = 0, nsrc = 0;
    uint32_t blocked = 0;
    bool per_peer = false;
};

struct PathArgs {
    const uint32_t *row_ptr, *col;
    const uint8_t *mflags, *cls;
    const uint64_t *smask, *sub;
    uint64_t *seen, *cur, *nxt;
    const uint64_t* inc;
    uint32_t* acc;
    unsigned long long* any;
    uint32_t *reach_count, *hop_sum;
    int64_t E, n;
    int32_t t, C, level, nsrc;
    uint32_t blocked, olo, ohi;
    int32_t sharded;
};

struct PathSources {
    uint32_t id[GSIM_PATH_SOURCES];
};

namespace {

constexpr int kPathBlock = 256;

// One edge of an active row: c = cur of the row, want = the plane bit followed.
template <bool Dense>
__device__ __forceinline__ void push_edge(const PathArgs& a, uint64_t m, uint32_t e, uint64_t c, uint8_t want)
{
    // the plane byte and the neighbour: independent loads, one wait
    const uint8_t fl = a.mflags[slot_idx_of<Dense>(m, a.t, a.E, (int64_t)e)];
    const uint32_t j = a.col[e];
    if (!(fl & want)) return;
    const uint64_t sj = a.sub[j], sn = a.seen[j];                  // ... and these two
    if (((sj >> a.t) & 1ull) && (c & ~sn)) atomicOr((unsigned long long*)&a.nxt[j], (unsigned long long)c);
}

template <int W, bool Dense>
__global__ __launch_bounds__(kPathBlock) void k_mp_push(PathArgs a, const uint32_t* rows, int64_t nrows, int64_t base)
{
    static_assert(W == 16 || W == 32 || W == 64, "a lane group per row");
    const int gl = (int)(threadIdx.x % W);
    for (int64_t x = ((int64_t)blockIdx.x * kPathBlock + threadIdx.x) / W; x < nrows;
         x += (int64_t)gridDim.x * kPathBlock / W) {
        const uint32_t i = rows ? rows[x] : (uint32_t)(base + x);
        const uint64_t c = a.cur[i];
        if (!c) continue;                                          // not on the frontier
        const uint32_t b = a.row_ptr[i], deg = a.row_ptr[i + 1] - b;
        const uint64_t m = Dense ? ~0ull : a.smask[i];
        const bool ann = (a.sub[i] >> a.t) & 1ull;
        if ((uint32_t)gl >= deg || !slot_has_of<Dense>(m, a.t)) continue;   // (rows of this class hold at most W edges)
        push_edge<Dense>(a, m, b + (uint32_t)gl, c, ann ? GSIM_TF_MESH : GSIM_TF_FANOUT);
    }
}

// Rows of more than 64 connections: a block per row.
template <bool Dense>
__global__ __launch_bounds__(kPathBlock) void k_mp_push_hub(PathArgs a, const uint32_t* rows, int64_t nrows)
{
    for (int64_t x = blockIdx.x; x < nrows; x += gridDim.x) {
        const uint32_t i = rows[x];
        const uint64_t c = a.cur[i];
        if (!c) continue;
        const uint32_t b = a.row_ptr[i], deg = a.row_ptr[i + 1] - b;
        const uint64_t m = Dense ? ~0ull : a.smask[i];
        const bool ann = (a.sub[i] >> a.t) & 1ull;
        if (!slot_has_of<Dense>(m, a.t)) continue;
        const uint8_t want = ann ? GSIM_TF_MESH : GSIM_TF_FANOUT;
        for (uint32_t e0 = threadIdx.x; e0 < deg; e0 += kPathBlock) push_edge<Dense>(a, m, b + e0, c, want);
    }
}

// Level 0: an announcing source is reached through its nxt bit (the fold
// counts it at distance 0); a fanout publisher only gets a frontier bit.
__global__ __launch_bounds__(GSIM_PATH_SOURCES) void k_mp_seed(PathArgs a, PathSources src)
{
    const int k = (int)threadIdx.x;
    if (k >= a.nsrc) return;
    const uint32_t s = src.id[k];
    if (s == 0xFFFFFFFFu || (int64_t)s >= a.n) return;
    const unsigned long long bit = 1ull << k;
    if ((a.sub[s] >> a.t) & 1ull) atomicOr((unsigned long long*)&a.nxt[s], bit);
    else atomicOr((unsigned long long*)&a.cur[s], bit);
}

template <bool CLS, bool L0>
__global__ __launch_bounds__(kPathBlock) void k_mp_fold(PathArgs a)
{
    static_assert(kPathBlock == GSIM_PATH_SOURCES * GSIM_NET_CLASSES, "a thread per (source, class) flushes");
    __shared__ uint32_t s_cnt[GSIM_PATH_SOURCES * GSIM_NET_CLASSES];
    __shared__ uint32_t s_mem[GSIM_NET_CLASSES];
    __shared__ unsigned long long s_any;
    s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < GSIM_NET_CLASSES) s_mem[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_any = 0ull;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t lvl = (uint32_t)a.level;
    for (int64_t p0 = (int64_t)blockIdx.x * kPathBlock; p0 < a.n; p0 += (int64_t)gridDim.x * kPathBlock) {   // block-uniform
        const int64_t p = p0 + threadIdx.x;
        const bool in = p < a.n, own = in && p >= (int64_t)a.olo && p < (int64_t)a.ohi;
        uint64_t nw = 0, co = 0;
        uint32_t cl = 0;
        bool ann = false;
        if (own) {
            // nxt, seen (the class, the level-0 words): independent loads, one wait
            uint64_t nx = a.nxt[p];
            const uint64_t sn = a.seen[p];
            if (a.inc) nx |= a.inc[p - (int64_t)a.olo];
            if (CLS) cl = a.cls[p];
            nw = nx & ~sn;
            if (nx) a.nxt[p] = 0ull;
            if (nw) a.seen[p] = sn | nw;
            if (L0) {
                ann = (a.sub[p] >> a.t) & 1ull;
                co = a.cur[p] | nw;                                // the seeds of the fanout publishers stay
                if (nw) a.cur[p] = co;
            } else {
                co = ((a.blocked >> cl) & 1u) ? 0ull : nw;         // a blocked peer is reached and never relays
                a.cur[p] = co;
            }
            if (nw && a.reach_count) {
                const uint32_t k = (uint32_t)__popcll(nw);
                a.reach_count[p] += k;
                a.hop_sum[p] += k * lvl;
            }
        } else if (in && a.sharded) {
            a.nxt[p] = 0ull;                                       // a ghost's bits went to its owner
        }
        if (L0) {
            for (int c = 0; c < a.C; ++c) {
                const uint32_t k = (uint32_t)__popcll(__ballot(ann && cl == (uint32_t)c));
                if (lane == 0 && k) atomicAdd(&s_mem[c], k);
            }
        }
        if (__ballot(co != 0ull)) {                                // wave-uniform
            const uint64_t w = wave_or(co);
            if (lane == 0) atomicOr(&s_any, (unsigned long long)w);
        }
        if (!__ballot(nw != 0ull)) continue;                       // wave-uniform
        for (uint64_t todo = wave_or(nw); todo; todo &= todo - 1) {   // the source bits present in the wave
            const int s = __builtin_ctzll(todo);
            const bool bit = (nw >> s) & 1ull;
            uint32_t val = 0;
            if (CLS) {
                for (int c = 0; c < a.C; ++c) {
                    const uint32_t k = (uint32_t)__popcll(__ballot(bit && cl == (uint32_t)c));
                    if (lane == c) val = k;
                }
            } else {
                const uint32_t k = (uint32_t)__popcll(__ballot(bit));
                if (lane == 0) val = k;
            }
            if (lane < GSIM_NET_CLASSES && val) atomicAdd(&s_cnt[s * GSIM_NET_CLASSES + lane], val);
        }
    }
    __syncthreads();
    {
        const uint32_t v = s_cnt[threadIdx.x];
        if (v) {
            uint32_t* r = a.acc + (threadIdx.x / GSIM_NET_CLASSES) * kPA;
            atomicAdd(&r[PA_HIST + (lvl < GSIM_REPORT_BINS - 1 ? lvl : GSIM_REPORT_BINS - 1)], v);
            atomicAdd(&r[PA_RCLS + threadIdx.x % GSIM_NET_CLASSES], v);
            atomicMax(&r[PA_MAXH], lvl);
        }
    }
    if (L0 && threadIdx.x < GSIM_NET_CLASSES && s_mem[threadIdx.x]) atomicAdd(&a.acc[PA_MEMBERS + threadIdx.x], s_mem[threadIdx.x]);
    if (threadIdx.x == 0) {
        if (s_any) atomicOr(&a.any[lvl & 1u], s_any);
        if (blockIdx.x == 0) a.any[(lvl + 1u) & 1u] = 0ull;        // the next level's word (read by the host before this launch)
    }
}

template <bool Dense>
void launch_push(gsim_handle* h, const PathArgs& a)
{
    launch_row_classes(h, kPathBlock, [&](auto w, dim3 grid, const uint32_t* rows, int64_t nrows, int64_t base) {
        constexpr int W = decltype(w)::value;
        if constexpr (W == 0)
            hipLaunchKernelGGL((k_mp_push_hub<Dense>), grid, dim3(kPathBlock), 0, h->stream, a, rows, nrows);
        else
            hipLaunchKernelGGL((k_mp_push<W, Dense>), grid, dim3(kPathBlock), 0, h->stream, a, rows, nrows, base);
    });
}

PathArgs path_args(gsim_handle* h)
{
    MeshPaths* r = h->mp;
    const size_t n = (size_t)h->n;
    PathArgs a{};
    a.row_ptr = h->d_row_ptr; a.col = h->d_col; a.mflags = h->d_mflags;
    a.C = netreport_classes(h, &a.cls);
    a.smask = h->d_smask; a.sub = h->d_sub;
    a.seen = r->d_words; a.cur = r->d_words + n; a.nxt = r->d_words + 2 * n;
    a.acc = r->d_acc; a.any = r->d_any;
    if (r->per_peer) { a.reach_count = r->d_pp; a.hop_sum = r->d_pp + n; }
    a.E = h->e; a.n = h->n;
    a.t = r->topic; a.nsrc = r->nsrc; a.blocked = r->blocked;
    a.olo = (uint32_t)h->olo(); a.ohi = (uint32_t)h->ohi();
    a.sharded = h->sh ? 1 : 0;
    return a;
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void meshpaths_release(gsim_handle* h)
{
    if (!h->mp) return;
    MeshPaths* r = h->mp;
    free_all({r->d_words, r->d_inc, r->d_acc, r->d_any, r->d_pp});
    delete r;
    h->mp = nullptr;
}

int meshpaths_begin(gsim_handle* h, int32_t topic, const uint32_t* src_local, int32_t n_sources, uint32_t blocked,
                    bool per_peer)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (!h->mp) h->mp = new MeshPaths;
    MeshPaths* r = h->mp;
    const size_t n = (size_t)std::max<int64_t>(h->n, 1), own = (size_t)std::max<int64_t>(h->ohi() - h->olo(), 1);
    int rc = alloc_once(h, "report", &r->d_words, (int64_t)(3 * n));
    if (!rc) rc = alloc_once(h, "report", &r->d_acc, kPathAcc);
    if (!rc) rc = alloc_once(h, "report", &r->d_any, 2);
    if (!rc && h->sh) rc = alloc_once(h, "report", &r->d_inc, (int64_t)own);
    if (!rc && per_peer) rc = alloc_once(h, "report", &r->d_pp, (int64_t)(2 * n));
    if (rc) return rc;
    r->topic = topic; r->nsrc = n_sources; r->blocked = blocked; r->per_peer = per_peer;
    hipError_t e = hipMemsetAsync(r->d_words, 0, sizeof(uint64_t) * 3 * n, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_acc, 0, sizeof(uint32_t) * kPathAcc, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_any, 0, sizeof(unsigned long long) * 2, h->stream);
    if (e == hipSuccess && per_peer) e = hipMemsetAsync(r->d_pp, 0, sizeof(uint32_t) * 2 * n, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_mesh_paths");
    PathSources src;
    for (int k = 0; k < GSIM_PATH_SOURCES; ++k) {
        uint32_t s = k < n_sources ? src_local[k] : 0xFFFFFFFFu;
        // a seed only on the peer's owner
        if (s != 0xFFFFFFFFu && ((int64_t)s < h->olo() || (int64_t)s >= h->ohi())) s = 0xFFFFFFFFu;
        src.id[k] = s;
    }
    hipLaunchKernelGGL(k_mp_seed, dim3(1), dim3(GSIM_PATH_SOURCES), 0, h->stream, path_args(h), src);
    return hip_check(h, hipGetLastError(), "gsim_mesh_paths");
}

int meshpaths_push(gsim_handle* h)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->ohi() <= h->olo() || h->e == 0) return GSIM_OK;
    const PathArgs a = path_args(h);
    if (h->d_smask) launch_push<false>(h, a); else launch_push<true>(h, a);
    return hip_check(h, hipGetLastError(), "gsim_mesh_paths");
}

int meshpaths_ghost_bits(gsim_handle* h, uint64_t* host)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    const uint64_t* nxt = h->mp->d_words + 2 * (size_t)h->n;
    const int64_t lo = h->olo(), hi = h->ohi();
    hipError_t e = hipSuccess;
    if (lo > 0) e = hipMemcpyAsync(host, nxt, sizeof(uint64_t) * (size_t)lo, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && hi < h->n)
        e = hipMemcpyAsync(host + hi, nxt + hi, sizeof(uint64_t) * (size_t)(h->n - hi), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    return hip_check(h, e, "gsim_mesh_paths");
}

int meshpaths_fold(gsim_handle* h, int32_t level, const uint64_t* inc, uint64_t* any)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    MeshPaths* r = h->mp;
    PathArgs a = path_args(h);
    a.level = level;
    hipError_t e = hipSuccess;
    if (inc && r->d_inc) {
        e = stream_copy(h, r->d_inc, inc, sizeof(uint64_t) * (size_t)(h->ohi() - h->olo()), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_check(h, e, "gsim_mesh_paths");
        a.inc = r->d_inc;
    }
    const dim3 grid((uint32_t)std::max<int64_t>(1, std::min<int64_t>((h->n + kPathBlock - 1) / kPathBlock, 2048)));
    const bool cls_on = a.cls != nullptr;
    if (level == 0) {
        if (cls_on) hipLaunchKernelGGL((k_mp_fold<true, true>), grid, dim3(kPathBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_mp_fold<false, true>), grid, dim3(kPathBlock), 0, h->stream, a);
    } else {
        if (cls_on) hipLaunchKernelGGL((k_mp_fold<true, false>), grid, dim3(kPathBlock), 0, h->stream, a);
        else hipLaunchKernelGGL((k_mp_fold<false, false>), grid, dim3(kPathBlock), 0, h->stream, a);
    }
    e = hipGetLastError();
    unsigned long long w = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&w, r->d_any + (level & 1), sizeof w, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);      // the level's one host read
    *any = (uint64_t)w;
    return hip_check(h, e, "gsim_mesh_paths");
}

int meshpaths_finish(gsim_handle* h, const uint32_t* sources, uint64_t truncated, struct gsim_mesh_path_row* rows,
                     uint32_t* reach_count, uint32_t* hop_sum)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    MeshPaths* r = h->mp;
    std::vector<uint32_t> acc(kPathAcc);
    hipError_t e = hipMemcpyAsync(acc.data(), r->d_acc, sizeof(uint32_t) * kPathAcc, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && r->per_peer && reach_count && h->n)
        e = hipMemcpyAsync(reach_count, r->d_pp, sizeof(uint32_t) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && r->per_peer && hop_sum && h->n)
        e = hipMemcpyAsync(hop_sum, r->d_pp + h->n, sizeof(uint32_t) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_mesh_paths");
    uint32_t subs = 0;
    for (int c = 0; c < GSIM_NET_CLASSES; ++c) subs += acc[PA_MEMBERS + c];
    for (int k = 0; k < r->nsrc; ++k) {
        const uint32_t* c = acc.data() + (size_t)k * kPA;
        gsim_mesh_path_row x{};
        x.source = sources[k];
        x.topic = (uint32_t)r->topic;
        x.subscribers = subs;
        x.max_hops = c[PA_MAXH];
        x.truncated = (truncated >> k) & 1ull ? 1u : 0u;
        for (int q = 0; q < GSIM_NET_CLASSES; ++q) { x.reached_cls[q] = c[PA_RCLS + q]; x.members_cls[q] = acc[PA_MEMBERS + q]; }
        for (int q = 0; q < GSIM_REPORT_BINS; ++q) { x.hist[q] = c[PA_HIST + q]; x.reached += c[PA_HIST + q]; }
        rows[k] = x;
    }
    return GSIM_OK;
}

extern "C" {

int gsim_mesh_paths(gsim_handle* h, int32_t topic, const uint32_t* sources, int32_t n_sources, uint32_t blocked,
                    int32_t max_hops, struct gsim_mesh_path_row* rows, uint32_t* reach_count, uint32_t* hop_sum)
{
    if (!h || !sources || !rows) return GSIM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->e == 0 && h->n == 0) { h->err = "no graph loaded (call gsim_load_graph first)"; return GSIM_ESTATE; }
    if (n_sources < 1 || n_sources > GSIM_PATH_SOURCES) { h->err = "gsim_mesh_paths: n_sources must lie in 1..64"; return GSIM_EINVAL; }
    if (topic < 0 || topic >= h->t) { h->err = "gsim_mesh_paths: topic out of range"; return GSIM_EINVAL; }
    for (int k = 0; k < n_sources; ++k)
        if ((int64_t)sources[k] >= h->n) { h->err = "gsim_mesh_paths: a source is not a peer"; return GSIM_EINVAL; }
    const uint8_t* d_cls;
    const int C = netreport_classes(h, &d_cls);
    if (blocked >> C) { h->err = "gsim_mesh_paths: a blocked bit is at or above the class count"; return GSIM_EINVAL; }
    if (max_hops < 0) { h->err = "gsim_mesh_paths: max_hops must not be negative"; return GSIM_EINVAL; }
    int rc = meshpaths_begin(h, topic, sources, n_sources, blocked, reach_count || hop_sum);
    if (rc) return rc;
    uint64_t any = 0, truncated = 0;
    int32_t level = 0;
    if ((rc = meshpaths_fold(h, 0, nullptr, &any))) return rc;
    while (any) {
        if (max_hops > 0 && level == max_hops) { truncated = any; break; }
        if ((rc = meshpaths_push(h))) return rc;
        ++level;
        if ((rc = meshpaths_fold(h, level, nullptr, &any))) return rc;
    }
    return meshpaths_finish(h, sources, truncated, rows, reach_count, hop_sum);
}

}  // extern "C"
