// report_common.h — what the six device reports share (report.hip,
// netreport.hip, peerreport.hip, scorereport.hip, meshpaths.hip,
// relayreport.hip; none of it runs inside a tick).
//
// Device side:
//   k_select      the message selection: the slots published in a round window,
//                 compacted in slot order; the row written per slot is the
//                 caller's functor, the per-topic counts a compile-time choice
//   walk_keys     the distinct-key walk of a wave (lead_keys: its leader-lane
//                 form, count_keys: the leader adds to an LDS counter)
//   member_rank   a lane's place in a member-compacted slot; lane_cell: its cell
//   wave_max, wave_or
// Host side:
//   grow, alloc_once, free_all   device scratch and its one error text
//   launch_row_classes           a launch per heartbeat row class
//   ScoreEdges, score_edges      the callers' histogram edges, validated
#pragma once
#include <algorithm>
#include <initializer_list>
#include <string>
#include <type_traits>

#include "gsim_internal.h"

namespace gsim {

// ---- wave reductions (every lane gets the result) ------------------------------

__device__ __forceinline__ uint32_t wave_max(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t y = (uint32_t)__shfl_xor((int)x, off, 64);
        x = y > x ? y : x;
    }
    return x;
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// ---- the distinct-key walk -------------------------------------------------------

__device__ __forceinline__ uint32_t readlane_key(uint32_t key, int lead)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
}
__device__ __forceinline__ uint64_t readlane_key(uint64_t key, int lead)
{
    return (uint64_t)readlane_key((uint32_t)(key >> 32), lead) << 32 | readlane_key((uint32_t)key, lead);
}

// One key (u32 or u64) per lane of `on`.  Called by the whole wave: f(k, same,
// lead) runs once per distinct key present, on every lane, with the key, the
// ballot of the lanes holding it and the first of them (all wave-uniform).
template <typename K, typename F>
__device__ __forceinline__ void walk_keys(bool on, K key, F&& f)
{
    uint64_t todo = __ballot(on);
    while (todo) {                                             // wave-uniform
        const int lead = __builtin_ctzll(todo);
        const K k = readlane_key(key, lead);
        const uint64_t same = __ballot(on && key == k);
        f(k, same, lead);
        todo &= ~same;
    }
}

// ... f(k, count) on the key's leader lane alone.
template <typename K, typename F>
__device__ __forceinline__ void lead_keys(bool on, K key, int lane, F&& f)
{
    walk_keys(on, key, [&](K k, uint64_t same, int lead) {
        if (lane == lead) f(k, (uint32_t)__popcll(same));
    });
}

// ... the leader lanes add the popcounts to the block's LDS counters s_cnt[key].
__device__ __forceinline__ void count_keys(uint32_t* s_cnt, bool on, uint32_t key, int lane)
{
    lead_keys(on, key, lane, [&](uint32_t k, uint32_t c) { atomicAdd(&s_cnt[k], c); });
}

// ---- the lane's cell of a slot -----------------------------------------------------

// A wave owns the 64 peers of one member-bitmap word (Cells::word: its bits and
// the cell offset of its first member): whether the lane's peer has a cell in
// the topic's slots, and the cell's offset from the slot's base.
__device__ __forceinline__ void member_rank(uint64_t wbits, int64_t wpre, int lane, bool& has, int64_t& idx)
{
    has = (wbits >> lane) & 1ull;
    idx = wpre + __popcll(wbits & ((1ull << lane) - 1ull));
}

// one selected message as the walks read it: the peer report's row; the relay report's
// begins with the same fields (fill_sel and lane_cell take either)
struct SelMsg {
    uint64_t base;      // first cell of the slot
    uint32_t len;       // its cells (peers, or members of its topic)
    uint32_t pub;       // publication round
    uint32_t topic, origin;
};

template <typename Msg>
__device__ __forceinline__ void fill_sel(Msg& x, const ReportView& v, int m, int64_t pub)
{
    const int64_t base = (int64_t)v.cells.cbase[m];
    const int64_t end = (int64_t)m + 1 < v.ring ? (int64_t)v.cells.cbase[m + 1] : v.ncells;
    x.base = (uint64_t)base;
    x.len = (uint32_t)(end > base ? end - base : 0);
    x.pub = (uint32_t)pub;
    x.topic = v.mtopic[m];
    x.origin = v.morigin[m];
}

// the lane's cell of slot mm (kUnseen64: it has none); word is wave-uniform
template <typename Msg>
__device__ __forceinline__ uint64_t lane_cell(const Cells& cells, const Msg& mm, int64_t word, int lane, bool wave_on,
                                              bool active)
{
    const int32_t t = (int32_t)mm.topic;
    bool has = true;
    int64_t idx = word * 64 + lane;
    if ((cells.sparse >> t) & 1ull) {                          // wave-uniform
        uint64_t wbits = 0;
        int64_t wpre = 0;
        if (wave_on) cells.word(t, word, wbits, wpre);
        member_rank(wbits, wpre, lane, has, idx);
    }
    if (active && has && idx < (int64_t)mm.len) return cells.cell[(int64_t)mm.base + idx];
    return kUnseen64;
}

// ---- the message selection ---------------------------------------------------------

constexpr int kSelBlock = 1024;

// The slots whose message was published in [lo, hi), compacted in slot order
// (a block-wide prefix count per 1024 slots).  One block.  Fill::Row is the row
// type and Fill::fill(row, v, m, pub) writes rows[pos] of slot m and returns its
// topic.  cnt[0] = the selected slots.  TOPIC0 > 0: the words cnt[1 .. TOPIC0)
// (the caller's flags) are cleared and cnt[TOPIC0 + t] = the selected messages
// of topic t; TOPIC0 == 0: cnt[0] alone is written.
template <typename Fill, int TOPIC0>
__global__ __launch_bounds__(kSelBlock) void k_select(ReportView v, int64_t lo, int64_t hi, typename Fill::Row* rows,
                                                      uint32_t* cnt)
{
    __shared__ uint32_t s_w[kSelBlock / 64];
    __shared__ uint32_t s_base;
    __shared__ uint32_t s_nm[TOPIC0 ? GSIM_MAX_TOPICS : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_base = 0;
    if (TOPIC0 && tid < GSIM_MAX_TOPICS) s_nm[tid] = 0;
    __syncthreads();
    for (int m0 = 0; m0 < v.ring; m0 += kSelBlock) {
        const int m = m0 + tid;
        bool sel = false;
        int64_t pub = 0;
        if (m < v.ring && v.slot_last[m] >= 0) {               // published at least once
            pub = v.mpub[m];
            sel = pub >= lo && pub < hi;
        }
        const uint64_t b = __ballot(sel);
        if (lane == 0) s_w[w] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t pos = s_base + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        for (int q = 0; q < w; ++q) pos += s_w[q];
        if (sel) {
            const uint32_t topic = Fill::fill(rows[pos], v, m, pub);
            if (TOPIC0 && topic < (uint32_t)GSIM_MAX_TOPICS) atomicAdd(&s_nm[topic], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t tot = 0;
            for (int q = 0; q < kSelBlock / 64; ++q) tot += s_w[q];
            s_base += tot;
        }
        __syncthreads();
    }
    if (tid == 0) cnt[0] = s_base;
    if (TOPIC0) {
        if (tid > 0 && tid < TOPIC0) cnt[tid] = 0;
        if (tid < GSIM_MAX_TOPICS) cnt[TOPIC0 + tid] = s_nm[tid];
    }
}

// ---- host: device scratch ------------------------------------------------------------

// *p holds at least `need` elements afterwards (*cap: what it holds).  Growing
// waits for the stream, frees and allocates anew; the contents are not kept.
// `what` names the report in the error text.
template <typename T>
int grow(gsim_handle* h, const char* what, T** p, int64_t* cap, int64_t need)
{
    if (*cap >= need) return GSIM_OK;
    if (*p) {
        (void)hipStreamSynchronize(h->stream);
        (void)hipFree(*p);
    }
    *p = nullptr;
    *cap = 0;
    const hipError_t e = hipMalloc((void**)p, sizeof(T) * (size_t)need);
    if (e != hipSuccess) {
        h->err = std::string(what) + " scratch: " + hipGetErrorString(e);
        return GSIM_ENOMEM;
    }
    *cap = need;
    return GSIM_OK;
}

// a buffer of a fixed size n, allocated at the first call
template <typename T>
int alloc_once(gsim_handle* h, const char* what, T** p, int64_t n)
{
    int64_t cap = *p ? n : 0;
    return grow(h, what, p, &cap, n);
}

inline void free_all(std::initializer_list<void*> ps)
{
    for (void* p : ps)
        if (p) (void)hipFree(p);
}

// ---- host: a launch per heartbeat row class --------------------------------------------

// The owned rows by the heartbeat's row classes (row_classes): launch(W, grid,
// rows, nrows, base) once per class that holds rows, W an
// std::integral_constant of 16, 32 or 64 (a lane group of W lanes per row of at
// most W connections) or 0 (the hub rows, a block per row; only with lists).
template <typename F>
void launch_row_classes(gsim_handle* h, int block, F&& launch)
{
    RowClasses rc{};
    row_classes(h, &rc);
    auto grid = [](int64_t groups, int per_block) {
        return dim3((uint32_t)std::max<int64_t>(1, std::min<int64_t>((groups + per_block - 1) / per_block, 2048)));
    };
    const uint32_t* r = rc.rows;
    const int64_t b0 = r ? 0 : h->olo();
    // (without lists one class holds every owned row, in order from olo)
    if (rc.n16) launch(std::integral_constant<int, 16>{}, grid(rc.n16, block / 16), r, rc.n16, b0);
    if (rc.n32) launch(std::integral_constant<int, 32>{}, grid(rc.n32, block / 32), r ? r + rc.n16 : r, rc.n32, b0);
    if (rc.n64) launch(std::integral_constant<int, 64>{}, grid(rc.n64, block / 64), r ? r + rc.n16 + rc.n32 : r, rc.n64, b0);
    if (rc.nhub && r)
        launch(std::integral_constant<int, 0>{}, dim3((uint32_t)std::min<int64_t>(rc.nhub, 1024)),
               r + rc.n16 + rc.n32 + rc.n64, rc.nhub, b0);
}

// ---- host: histogram edges -------------------------------------------------------------

// the caller's edges of a score histogram, by value in a kernel argument
struct ScoreEdges {
    double v[GSIM_NET_SCORE_BINS - 1];
    int32_t n;
};

// 0..15 edges, strictly ascending, no NaN; fn: the calling function, for the error text
inline int score_edges(gsim_handle* h, const char* fn, const double* edges, int32_t n_edges, ScoreEdges* ed)
{
    if (n_edges < 0 || n_edges > GSIM_NET_SCORE_BINS - 1 || (n_edges > 0 && !edges)) {
        h->err = std::string(fn) + ": n_edges must lie in 0..15";
        return GSIM_EINVAL;
    }
    *ed = ScoreEdges{};
    ed->n = n_edges;
    for (int k = 0; k < n_edges; ++k) {
        if (edges[k] != edges[k] || (k > 0 && !(edges[k] > edges[k - 1]))) {
            h->err = std::string(fn) + ": the edges must be strictly ascending, without NaN";
            return GSIM_EINVAL;
        }
        ed->v[k] = edges[k];
    }
    return GSIM_OK;
}

}  // namespace gsim
