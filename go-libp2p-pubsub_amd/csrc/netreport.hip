// Network report (include/gsim.h gsim_net_report): mesh sizes, mesh links by
// the neighbour's class, fanout, and the score snapshot as histograms per
// (observer class, subject class), reduced on the device from the router's
// topic slot planes (mflags, edge order) and the per-record score state.  The
// reference shows these figures only per router (gs.mesh / gs.fanout,
// gossipsub.go:424-425; PeerScoreSnapshot, score.go:127-140); the report is
// their network-wide distribution.  No [T][E] view is built.
//
// Mesh pass: over the owned observers' rows, by the heartbeat's row classes
// (row_classes: rows of at most 16 / 32 / 64 connections, then the hubs).
//   k_net_mesh<W>      a lane group of W lanes per row, lane gl on edge
//                      row_ptr[i] + gl: per topic the group's lanes read one
//                      byte each of the topic's plane, contiguous along the
//                      row, and the row's counts are popcounts of the group's
//                      part of a ballot.  The wave walks only the topics some
//                      row of it holds (announced, fanout or slot), four
//                      topics' plane bytes in flight per lane.
//   k_net_mesh_hub     a block per row of more than 64 connections, 256 edges
//                      per step; per topic each wave adds its ballot popcounts
//                      to the row's LDS counters, which the block folds in
//                      once the row is walked.
// Both keep the report's counters per block in LDS, sized to the live T * C
// (kMF u32 per (topic, class): 196 bytes; 64 x 4 rows are 49 KB), one LDS atomic
// per lane for the row's handful of updates (lane k of the group carries update
// k), and flush the non-zero ones with one global atomic each (max_degree:
// atomicMax).  cls[col[e]] is gathered only when there is more than one class.
//
// Score pass: k_net_score over every local record r in record order (score[r],
// estate[r], owner[r] and col[r] coalesced): the subject is the row owner, the
// observer col[r]; a shard skips the records of observers it does not own
// (k_census's test).  Each lane has one key, (class pair, bin | NaN | retained);
// a wave counts by ballot over the distinct keys present and its leader lanes
// add to the block's LDS counters; connected is the row's hist + nan.  min and
// max are integer atomics on an order-preserving map of the f64 bits (the
// minimum kept as the maximum of the complement, so zero is both identities); a
// lane issues one only where it improves on what the block already holds.
// The edges arrive by value in the kernel argument.
//
// Every result is an integer count or a min / max: no dependence on scheduling.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch
// or spills; the ranges span the Dense / slot-plane and one-class / classes
// instances (LDS: the static part; the mesh kernels add 196 bytes per live
// (topic, class)):
//   k_net_mesh<16|32|64>  18-32 VGPRs, 86-91 SGPRs, 8 waves/SIMD
//   k_net_mesh_hub        20-24 VGPRs, 86-101 SGPRs, 1536 bytes of LDS, 7-8 waves/SIMD
//   k_net_score           14-16 VGPRs, 102-106 SGPRs, 1408 bytes of LDS, 7 waves/SIMD
// Measured: C3 after the default bench's ticks, two classes, the
// whole call 1.65 ms (mesh pass 1.33 ms over 512 MB of planes, score pass 0.34 ms
// over 544 MB): ballots and LDS atomics per (row, topic) bound it, not HBM.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "report_common.h"

namespace gsim {

// per (topic, class) counters of the mesh pass, u32 in LDS, u64 in global memory
enum : int {
    MF_MEMBERS = 0,
    MF_FANP,
    MF_MAXD,
    MF_OUTL,
    MF_FANL,
    MF_LINK,                                   // [GSIM_NET_CLASSES]
    MF_DEG = MF_LINK + GSIM_NET_CLASSES,       // [GSIM_NET_DEG_BINS]
    MF_OUT = MF_DEG + GSIM_NET_DEG_BINS,       // [GSIM_NET_OUT_BINS]
    kMF = MF_OUT + GSIM_NET_OUT_BINS,          // 49
};
// per class pair counters of the score pass
enum : int {
    SF_NAN = GSIM_NET_SCORE_BINS,              // after the bins
    SF_RET,
    kSFCount,                                  // 18 counts
    SF_MIN = kSFCount,                         // max of ~key
    SF_MAX,                                    // max of key
    kSF,                                       // 20
};
constexpr int kMaxPairs = GSIM_NET_CLASSES * GSIM_NET_CLASSES;
constexpr size_t kMeshAcc = (size_t)GSIM_MAX_TOPICS * GSIM_NET_CLASSES * kMF;
constexpr size_t kAccWords = kMeshAcc + (size_t)kMaxPairs * kSF;

struct NetReport {
    uint8_t* d_cls = nullptr;                  // [n] class of each local peer (nullptr: all 0)
    int C = 1;
    unsigned long long* d_acc = nullptr;       // [kAccWords] mesh counters, then score counters
};

struct NetArgs {
    const uint32_t *row_ptr, *col, *owner;
    const uint8_t *outbound, *mflags, *estate, *cls;
    const uint64_t *smask, *sub, *fan;
    const double* score;
    int64_t E;
    int32_t T, C;
    int32_t sharded;
    uint32_t olo, ohi;
    unsigned long long* acc;                   // this pass's counters
};

namespace {

constexpr int kNetBlock = 256;
constexpr int kTopicBatch = 4;             // k_net_mesh: plane bytes in flight per lane

// The block's counters to global memory: one atomic per non-zero entry.
__device__ __forceinline__ void mesh_flush(const uint32_t* s_acc, int nacc, unsigned long long* acc)
{
    for (int q = threadIdx.x; q < nacc; q += kNetBlock) {
        const uint32_t v = s_acc[q];
        if (!v) continue;
        if (q % kMF == MF_MAXD) atomicMax(&acc[q], (unsigned long long)v);
        else atomicAdd(&acc[q], (unsigned long long)v);
    }
}

// One (row, topic) into the block's counters, spread over the lanes k = 0..8
// of a lane group (or done by one thread, k running): d mesh or fanout edges,
// o of them outbound, nc[c] into class c.
__device__ __forceinline__ void mesh_update(uint32_t* s_row, int k, bool mem, bool fan, uint32_t d, uint32_t o,
                                            uint32_t nck)
{
    int idx = -1;
    uint32_t val = 0;
    if (mem) {
        switch (k) {
        case 0: idx = MF_MEMBERS; val = 1; break;
        case 1: idx = MF_DEG + (int)(d < GSIM_NET_DEG_BINS - 1 ? d : GSIM_NET_DEG_BINS - 1); val = 1; break;
        case 2: idx = MF_OUT + (int)(o < GSIM_NET_OUT_BINS - 1 ? o : GSIM_NET_OUT_BINS - 1); val = 1; break;
        case 3: idx = MF_OUTL; val = o; break;
        case 4: if (d) atomicMax(&s_row[MF_MAXD], d); break;
        default: idx = MF_LINK + (k - 5); val = nck; break;       // k = 5..8
        }
    } else {
        if (k == 0) { idx = MF_FANP; val = fan ? 1u : 0u; }
        else if (k == 1) { idx = MF_FANL; val = d; }
    }
    if (idx >= 0 && val) atomicAdd(&s_row[idx], val);
}

template <int W, bool Dense, bool CLS>
__global__ __launch_bounds__(kNetBlock) void k_net_mesh(NetArgs a, const uint32_t* rows, int64_t nrows, int64_t base)
{
    static_assert(W >= 16 && W <= 64, "lanes 0..8 of a group carry a row's updates");
    extern __shared__ uint32_t s_acc[];
    const int nacc = a.T * a.C * kMF;
    for (int q = threadIdx.x; q < nacc; q += kNetBlock) s_acc[q] = 0;
    __syncthreads();
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, gl = lane % W, gsh = lane - gl;
    const uint64_t gm = W == 64 ? ~0ull : ((1ull << W) - 1ull);
    const uint64_t tmask = a.T >= 64 ? ~0ull : ((1ull << a.T) - 1ull);
    const int64_t ngroups = (nrows + G - 1) / G * G;              // a wave's groups leave the loop together
    for (int64_t x = ((int64_t)blockIdx.x * kNetBlock + threadIdx.x) / W; x < ngroups;
         x += (int64_t)gridDim.x * kNetBlock / W) {
        const bool row_ok = x < nrows;
        const uint32_t i = row_ok ? (rows ? rows[x] : (uint32_t)(base + x)) : 0u;
        const uint32_t b = row_ok ? a.row_ptr[i] : 0u, deg = row_ok ? a.row_ptr[i + 1] - b : 0u;
        const bool on = (uint32_t)gl < deg;                       // (rows of this class hold at most W edges)
        const uint32_t e = b + (uint32_t)gl;
        const uint64_t m = Dense ? ~0ull : (row_ok ? a.smask[i] : 0ull);
        const uint64_t sb = row_ok ? a.sub[i] & tmask : 0ull;
        const uint64_t fn = row_ok && a.fan ? a.fan[i] & tmask & ~sb : 0ull;
        const uint32_t ci = CLS && row_ok ? a.cls[i] : 0u;
        bool ob = false;
        uint32_t cj = 0;
        if (on) {
            ob = a.outbound[e] != 0;
            if (CLS) cj = a.cls[a.col[e]];
        }
        const uint64_t need = (sb | fn | m) & tmask;
        for (int32_t t0 = 0; t0 < a.T; t0 += kTopicBatch) {
            // the batch's plane bytes are independent loads: issued together, one wait
            uint8_t flb[kTopicBatch];
#pragma unroll
            for (int u = 0; u < kTopicBatch; ++u) {
                const int32_t t = t0 + u;
                flb[u] = 0;
                if (t < a.T && on && slot_has_of<Dense>(m, t)) flb[u] = a.mflags[slot_idx_of<Dense>(m, t, a.E, (int64_t)e)];
            }
#pragma unroll
            for (int u = 0; u < kTopicBatch; ++u) {
                const int32_t t = t0 + u;
                if (t >= a.T || !__ballot((need >> t) & 1ull)) continue;   // no row of the wave holds t (wave-uniform)
                const bool mem = (sb >> t) & 1ull;
                const bool p = (flb[u] & (mem ? GSIM_TF_MESH : GSIM_TF_FANOUT)) != 0;
                const uint32_t d = (uint32_t)__popcll((__ballot(p) >> gsh) & gm);
                const uint32_t o = (uint32_t)__popcll((__ballot(p && ob) >> gsh) & gm);
                uint32_t nck = gl == 5 ? d : 0u;                  // one class: every link is into class 0
                if (CLS) {
                    for (int c = 0; c < a.C; ++c) {
                        const uint32_t n = (uint32_t)__popcll((__ballot(p && cj == (uint32_t)c) >> gsh) & gm);
                        if (gl == 5 + c) nck = n;
                    }
                }
                if (row_ok && gl < 9)
                    mesh_update(s_acc + ((int)t * a.C + (int)ci) * kMF, gl, mem, (fn >> t) & 1ull, d, o, nck);
            }
        }
    }
    __syncthreads();
    mesh_flush(s_acc, nacc, a.acc);
}

// Rows of more than 64 connections: a block per row.
template <bool Dense, bool CLS>
__global__ __launch_bounds__(kNetBlock) void k_net_mesh_hub(NetArgs a, const uint32_t* rows, int64_t nrows)
{
    extern __shared__ uint32_t s_acc[];
    __shared__ uint32_t s_row[GSIM_MAX_TOPICS][2 + GSIM_NET_CLASSES];     // d, o, links into each class
    const int nacc = a.T * a.C * kMF;
    for (int q = threadIdx.x; q < nacc; q += kNetBlock) s_acc[q] = 0;
    const int lane = threadIdx.x & 63;
    const uint64_t tmask = a.T >= 64 ? ~0ull : ((1ull << a.T) - 1ull);
    for (int64_t x = blockIdx.x; x < nrows; x += gridDim.x) {     // block-uniform
        for (int q = threadIdx.x; q < GSIM_MAX_TOPICS * (2 + GSIM_NET_CLASSES); q += kNetBlock) (&s_row[0][0])[q] = 0;
        __syncthreads();
        const uint32_t i = rows[x];
        const uint32_t b = a.row_ptr[i], deg = a.row_ptr[i + 1] - b;
        const uint64_t m = Dense ? ~0ull : a.smask[i];
        const uint64_t sb = a.sub[i] & tmask;
        const uint64_t fn = a.fan ? a.fan[i] & tmask & ~sb : 0ull;
        const uint32_t ci = CLS ? a.cls[i] : 0u;
        const uint64_t need = (sb | fn | m) & tmask;
        for (uint32_t e0 = 0; e0 < deg; e0 += kNetBlock) {
            const bool on = e0 + threadIdx.x < deg;
            const uint32_t e = b + e0 + threadIdx.x;
            bool ob = false;
            uint32_t cj = 0;
            if (on) {
                ob = a.outbound[e] != 0;
                if (CLS) cj = a.cls[a.col[e]];
            }
            for (uint64_t todo = need; todo; todo &= todo - 1) {
                const int32_t t = __builtin_ctzll(todo);
                const bool mem = (sb >> t) & 1ull;
                uint8_t fl = 0;
                if (on && slot_has_of<Dense>(m, t)) fl = a.mflags[slot_idx_of<Dense>(m, t, a.E, (int64_t)e)];
                const bool p = (fl & (mem ? GSIM_TF_MESH : GSIM_TF_FANOUT)) != 0;
                const uint64_t bp = __ballot(p);
                if (!bp) continue;                                // wave-uniform
                uint32_t val = lane == 0 ? (uint32_t)__popcll(bp) : 0u;
                const uint32_t o = (uint32_t)__popcll(__ballot(p && ob));
                if (lane == 1) val = o;
                if (CLS) {
                    for (int c = 0; c < a.C; ++c) {
                        const uint32_t n = (uint32_t)__popcll(__ballot(p && cj == (uint32_t)c));
                        if (lane == 2 + c) val = n;
                    }
                } else if (lane == 2) {
                    val = (uint32_t)__popcll(bp);
                }
                if (lane < 2 + GSIM_NET_CLASSES && val) atomicAdd(&s_row[t][lane], val);
            }
        }
        __syncthreads();
        if (threadIdx.x < GSIM_MAX_TOPICS && ((need >> threadIdx.x) & 1ull)) {
            const int32_t t = (int32_t)threadIdx.x;
            const bool mem = (sb >> t) & 1ull;
            uint32_t* r = s_acc + ((int)t * a.C + (int)ci) * kMF;
            for (int k = 0; k < 5 + a.C; ++k)
                mesh_update(r, k, mem, (fn >> t) & 1ull, s_row[t][0], s_row[t][1], k >= 5 ? s_row[t][2 + (k - 5)] : 0u);
        }
        __syncthreads();
    }
    __syncthreads();
    mesh_flush(s_acc, nacc, a.acc);
}

// (min / max: f64_key / key_f64, gsim_internal.h)
template <bool CLS>
__global__ __launch_bounds__(kNetBlock) void k_net_score(NetArgs a, ScoreEdges ed)
{
    __shared__ uint32_t s_cnt[kMaxPairs * kSFCount];
    __shared__ unsigned long long s_mm[kMaxPairs * 2];            // per pair: max of ~key, max of key
    for (int q = threadIdx.x; q < kMaxPairs * kSFCount; q += kNetBlock) s_cnt[q] = 0;
    if (threadIdx.x < kMaxPairs * 2) s_mm[threadIdx.x] = 0ull;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kNetBlock;
    for (int64_t r0 = (int64_t)blockIdx.x * kNetBlock; r0 < a.E; r0 += stride) {    // block-uniform
        const int64_t r = r0 + threadIdx.x;
        const bool valid = r < a.E;
        uint8_t st = valid ? a.estate[r] : (uint8_t)0;
        uint32_t obs = 0;
        if (valid && (CLS || a.sharded)) obs = a.col[r];
        if (a.sharded && (obs < a.olo || obs >= a.ohi)) st = 0;   // another shard's record
        const bool conn = (st & GSIM_ES_CONNECTED) != 0;
        const bool ret = !conn && (st & GSIM_ES_TRACKED) != 0;
        const bool act = conn || ret;
        // (unconditional loads: score, estate, col and owner leave together, then the two class bytes)
        const double sv = valid ? a.score[r] : 0.0;
        uint32_t pair = 0;
        if (CLS && valid) pair = (uint32_t)a.cls[obs] * (uint32_t)a.C + (uint32_t)a.cls[a.owner[r]];
        const double s = conn ? sv : 0.0;
        const bool isn = s != s;
        uint32_t bin = 0;
#pragma unroll
        for (int k = 0; k < GSIM_NET_SCORE_BINS - 1; ++k) bin += (k < ed.n && s >= ed.v[k]) ? 1u : 0u;
        const uint32_t key = pair * kSFCount + (conn ? (isn ? (uint32_t)SF_NAN : bin) : (uint32_t)SF_RET);
        count_keys(s_cnt, act, key, (int)(threadIdx.x & 63));      // the distinct keys present
        if (conn && !isn) {
            const unsigned long long kk = f64_key(s);
            volatile unsigned long long* mm = s_mm + pair * 2;
            if (~kk > mm[0]) atomicMax(&s_mm[pair * 2], ~kk);
            if (kk > mm[1]) atomicMax(&s_mm[pair * 2 + 1], kk);
        }
    }
    __syncthreads();
    const int npairs = a.C * a.C;
    for (int q = threadIdx.x; q < npairs * kSFCount; q += kNetBlock) {
        const uint32_t v = s_cnt[q];
        if (v) atomicAdd(&a.acc[(q / kSFCount) * kSF + q % kSFCount], (unsigned long long)v);
    }
    if ((int)threadIdx.x < npairs * 2) {
        const unsigned long long v = s_mm[threadIdx.x];
        if (v) atomicMax(&a.acc[(threadIdx.x >> 1) * kSF + SF_MIN + (threadIdx.x & 1)], v);
    }
}

template <bool Dense, bool CLS>
void launch_mesh(gsim_handle* h, const NetArgs& a)
{
    const size_t lds = sizeof(uint32_t) * (size_t)a.T * (size_t)a.C * kMF;
    launch_row_classes(h, kNetBlock, [&](auto w, dim3 grid, const uint32_t* rows, int64_t nrows, int64_t base) {
        constexpr int W = decltype(w)::value;
        if constexpr (W == 0)
            hipLaunchKernelGGL((k_net_mesh_hub<Dense, CLS>), grid, dim3(kNetBlock), lds, h->stream, a, rows, nrows);
        else
            hipLaunchKernelGGL((k_net_mesh<W, Dense, CLS>), grid, dim3(kNetBlock), lds, h->stream, a, rows, nrows, base);
    });
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void netreport_release(gsim_handle* h)
{
    if (!h->nr) return;
    free_all({h->nr->d_cls, h->nr->d_acc});
    delete h->nr;
    h->nr = nullptr;
}

int netreport_set_classes(gsim_handle* h, const uint8_t* cls, int C)
{
    int top = 0;
    if (cls)
        for (int64_t p = 0; p < h->n; ++p) {
            if (cls[p] >= GSIM_NET_CLASSES) { h->err = "peer class out of range (must be below GSIM_NET_CLASSES)"; return GSIM_EINVAL; }
            top = std::max<int>(top, cls[p]);
        }
    if (C <= 0) C = top + 1;
    if (C <= top || C > GSIM_NET_CLASSES) { h->err = "class count does not cover the classes given"; return GSIM_EINVAL; }
    if (!h->nr) h->nr = new NetReport;
    NetReport* r = h->nr;
    hipError_t e = hipStreamSynchronize(h->stream);               // no report in flight reads the old classes
    if (e == hipSuccess && cls && C > 1) {
        if (!r->d_cls) e = hipMalloc((void**)&r->d_cls, (size_t)std::max<int64_t>(h->n, 1));
        if (e == hipSuccess) e = stream_copy(h, r->d_cls, cls, (size_t)h->n, hipMemcpyHostToDevice);
    } else if (r->d_cls) {
        (void)hipFree(r->d_cls);
        r->d_cls = nullptr;
    }
    if (e != hipSuccess) return hip_check(h, e, "gsim_set_peer_classes");
    r->C = C;
    return GSIM_OK;
}

int netreport_classes(const gsim_handle* h, const uint8_t** d_cls)
{
    *d_cls = h->nr ? h->nr->d_cls : nullptr;
    return h->nr ? h->nr->C : 1;
}

extern "C" {

int gsim_set_peer_classes(gsim_handle* h, const uint8_t* cls)
{
    if (!h) return GSIM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->e == 0 && h->n == 0) { h->err = "no graph loaded (call gsim_load_graph first)"; return GSIM_ESTATE; }
    return netreport_set_classes(h, cls, 0);
}

int gsim_net_report(gsim_handle* h, const double* edges, int32_t n_edges, struct gsim_mesh_row* mesh, int64_t mesh_cap,
                    int64_t* n_mesh, struct gsim_score_row* scores, int64_t score_cap, int64_t* n_scores)
{
    if (!h || !n_mesh || !n_scores || mesh_cap < 0 || score_cap < 0) return GSIM_EINVAL;
    const int C = h->nr ? h->nr->C : 1;
    const int T = h->t;
    const int64_t nm = (int64_t)T * C, ns = (int64_t)C * C;
    *n_mesh = nm;
    *n_scores = ns;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->e == 0 && h->n == 0) { h->err = "no graph loaded (call gsim_load_graph first)"; return GSIM_ESTATE; }
    ScoreEdges ed{};
    if (int rc = score_edges(h, "gsim_net_report", edges, n_edges, &ed)) return rc;
    const bool want_mesh = mesh && mesh_cap > 0, want_scores = scores && score_cap > 0;
    if ((want_mesh && mesh_cap < nm) || (want_scores && score_cap < ns)) {
        h->err = "gsim_net_report: output buffer too small";
        return GSIM_ERANGE;
    }
    if (!want_mesh && !want_scores) return GSIM_OK;
    if (!h->nr) h->nr = new NetReport;
    NetReport* r = h->nr;
    if (int rc = alloc_once(h, "report", &r->d_acc, (int64_t)kAccWords)) return rc;
    const size_t mesh_words = (size_t)nm * kMF, score_words = (size_t)ns * kSF;
    hipError_t e = hipMemsetAsync(r->d_acc, 0, sizeof(unsigned long long) * kAccWords, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_net_report");

    NetArgs a{};
    a.row_ptr = h->d_row_ptr; a.col = h->d_col; a.owner = h->d_owner;
    a.outbound = h->d_outbound; a.mflags = h->d_mflags; a.estate = h->d_estate;
    a.cls = C > 1 ? r->d_cls : nullptr;
    a.smask = h->d_smask; a.sub = h->d_sub;
    FieldRef fr;
    a.fan = extra_field_ref(h, GSIM_F_FANOUT_TOPICS, &fr) ? (const uint64_t*)fr.ptr : nullptr;
    a.score = h->d_score;
    a.E = h->e; a.T = T; a.C = C;
    a.sharded = h->sh ? 1 : 0;
    a.olo = (uint32_t)h->olo(); a.ohi = (uint32_t)h->ohi();
    const bool cls_on = a.cls != nullptr;
    if (want_mesh && nm > 0 && h->ohi() > h->olo()) {
        a.acc = r->d_acc;
        if (h->d_smask) { if (cls_on) launch_mesh<false, true>(h, a); else launch_mesh<false, false>(h, a); }
        else { if (cls_on) launch_mesh<true, true>(h, a); else launch_mesh<true, false>(h, a); }
    }
    if (want_scores && h->e > 0) {
        a.acc = r->d_acc + kMeshAcc;
        const dim3 grid((uint32_t)std::max<int64_t>(1, std::min<int64_t>((h->e + 4 * kNetBlock - 1) / (4 * kNetBlock), 2048)));
        if (cls_on) hipLaunchKernelGGL(k_net_score<true>, grid, dim3(kNetBlock), 0, h->stream, a, ed);
        else hipLaunchKernelGGL(k_net_score<false>, grid, dim3(kNetBlock), 0, h->stream, a, ed);
    }
    std::vector<unsigned long long> acc(mesh_words + score_words);
    e = hipGetLastError();
    if (e == hipSuccess && want_mesh && mesh_words)
        e = hipMemcpyAsync(acc.data(), r->d_acc, sizeof(unsigned long long) * mesh_words, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && want_scores)
        e = hipMemcpyAsync(acc.data() + mesh_words, r->d_acc + kMeshAcc, sizeof(unsigned long long) * score_words,
                           hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_net_report");

    if (want_mesh)
        for (int64_t q = 0; q < nm; ++q) {
            const unsigned long long* c = acc.data() + (size_t)q * kMF;
            gsim_mesh_row x{};
            x.topic = (uint32_t)(q / C);
            x.cls = (uint32_t)(q % C);
            x.members = (uint32_t)c[MF_MEMBERS];
            x.max_degree = (uint32_t)c[MF_MAXD];
            x.fanout_peers = (uint32_t)c[MF_FANP];
            for (int k = 0; k < GSIM_NET_CLASSES; ++k) x.mesh_links[k] = c[MF_LINK + k];
            x.outbound_links = c[MF_OUTL];
            x.fanout_links = c[MF_FANL];
            for (int k = 0; k < GSIM_NET_DEG_BINS; ++k) x.deg_hist[k] = (uint32_t)c[MF_DEG + k];
            for (int k = 0; k < GSIM_NET_OUT_BINS; ++k) x.out_hist[k] = (uint32_t)c[MF_OUT + k];
            mesh[q] = x;
        }
    if (want_scores)
        for (int64_t q = 0; q < ns; ++q) {
            const unsigned long long* c = acc.data() + mesh_words + (size_t)q * kSF;
            gsim_score_row x{};
            x.obs_cls = (uint32_t)(q / C);
            x.subj_cls = (uint32_t)(q % C);
            uint64_t inb = 0;
            for (int k = 0; k < GSIM_NET_SCORE_BINS; ++k) { x.hist[k] = c[k]; inb += c[k]; }
            x.nan = c[SF_NAN];
            x.retained = c[SF_RET];
            x.connected = inb + x.nan;
            x.min = inb ? key_f64(~c[SF_MIN]) : std::numeric_limits<double>::infinity();
            x.max = inb ? key_f64(c[SF_MAX]) : -std::numeric_limits<double>::infinity();
            scores[q] = x;
        }
    return GSIM_OK;
}

}  // extern "C"
