// Connection tags and the connection manager's trim (include/gsim.h
// gsim_conn_tags_config .. gsim_conn_trim): the tag
// tracer (tag_tracer.go) for every router at once.  Protection (direct peers,
// mesh peers) is read from the router planes; the decaying delivery tags are a
// u8 per (topic slot, connection) in edge order, bumped from the committed
// seen-set cells -- every cell names its first sender (gsim_internal.h) -- by a
// kernel of their own, once per refresh: nothing here runs inside a round, and
// no delivery, heartbeat or score kernel knows of the tags.
//
// Kernels (a lane owns a peer and a wave the 64 peers of one member-bitmap word
// in the fold, as k_relay_push; wave64 throughout):
//   k_select<TgFill>  grid 1: the published slots of the ring (the reports'
//                  shared selection), each with its verdict and the last round
//                  it was claimed in.
//   k_tag_fold     grid (peer blocks, ring slots).  A block past the selection's
//                  count (it stays on the device), or whose slot was not claimed
//                  since the cursor, or whose verdict is not accept, leaves at
//                  once.  The lane reads its cell, coalesced, through lane_cell
//                  (dense and member-compacted layouts); a committed
//                  cell first seen in [cursor, current round) of a peer that is
//                  not the origin and has joined the topic qualifies.  The lane
//                  finds the first sender in its own sorted row (a binary search
//                  over col) and bumps dtag[plane][e]: an atomicCAS loop on the
//                  aligned 32-bit word holding the byte, v -> min(v + bump, cap).
//                  (The slots of a peer run in different blocks and the four
//                  bytes of a word belong to neighbouring connections, possibly
//                  of two rows: hence the atomic, not a serialisation of the
//                  slots.)  A bump is a capped addition and the decay comes
//                  after the fold, so the result does not depend on order.
//   k_tag_decay    one pass over the planes as 32-bit words, zero words skipped:
//                  v -> max(0, v - amount * instants crossed).
//   k_tag_drop     per (connection, direction) of a list going down or up: its
//                  byte of every plane cleared and, going up, since = now.
//   k_tag_leave    per (leaving peer, topic): the row's bytes of that plane.
//   k_tag_trim<W>  per heartbeat row class (launch_row_classes): a lane group of
//                  W lanes per row of at most W connections, a lane per
//                  connection.  Its value is the sum of its planes, its key
//                  select_key(P_TRIM).  The group counts its connected lanes
//                  (__ballot); a trimming row ranks every candidate among the
//                  candidates by (value, key) with W shuffles and closes those
//                  of rank < connected - low.  (A rank instead of k rounds of the
//                  heartbeat's min-reduction: k is up to the row length here,
//                  the rank costs W steps whatever k is, and needs no order.)
//   k_tag_trim_hub a block per hub row, streamed in tiles of 256 positions
//                  through LDS: every thread ranks its position of a chunk
//                  against every tile; no scratch sized by the row.
//                  Both mark the connection's lower-to-higher edge in a bitmap
//                  over the edges, so a connection either end chose is listed
//                  once and the list comes out in (a, b) order.
//   k_tag_collect  the marked edges -> (a, b) pairs through a counter (the host
//                  sorts them, as gsim_px_connect does), marks cleared.
//   k_tag_view, k_tag_values   the read-outs (gsim_conn_tags_read, gsim_conn_values).
// The trim's closes go through gsim_set_connections itself.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): no kernel uses
// scratch memory or spills a register; all run at 8 waves/SIMD but k_tag_trim<64> (7):
//   k_tag_fold        12 VGPRs,  50 SGPRs, no LDS
//   k_tag_decay        7 VGPRs,  17 SGPRs
//   k_tag_drop         9 VGPRs,  23 SGPRs;  k_tag_leave 6 VGPRs, 22 SGPRs
//   k_tag_trim<16>    22 VGPRs,  96 SGPRs;  <32> the same;  <64> 26 VGPRs, 106 SGPRs
//   k_tag_trim_hub    30 VGPRs,  96 SGPRs, 3328 bytes of LDS
//   k_tag_collect     14 VGPRs,  40 SGPRs;  k_tag_view 10 / 32;  k_tag_values 14 / 54
//   k_tag_relayout    18 VGPRs,  32 SGPRs;  k_select<TgFill> 26 VGPRs, 53 SGPRs, 68 bytes of LDS
// Measured (profiles/conn_tags_c3.txt; C3, one MI355X): the fold of
// one tick's 6.5e7 first deliveries 7.60 ms (the first one after a config too; 8.5e9 per second; 22 % of the parent's
// tick, more than its whole refresh pass of 6.65 ms); one decay pass 0.27 ms; one
// forced trim (low 24, high 0) 1.8 ms count only.  With tags off the default bench
// is inside the parent's own spread and delivers the same counts.
#include <algorithm>
#include <string>
#include <vector>

#include "report_common.h"
#include "philox.h"

namespace gsim {

// one published slot as the fold reads it: SelMsg's fields (report_common.h), then its state
struct TgMsg {
    uint64_t base;      // first cell of the slot
    uint32_t len;       // its cells
    uint32_t pub;       // publication round
    uint32_t topic, origin;
    int32_t last;       // last round with a new claim or the publication (slot_last)
    uint32_t verdict;   // GSIM_VERDICT_*
};

struct TagArgs {
    Cells cells;
    const TgMsg* sel;
    int64_t n, E;
    int32_t T, S;
    int64_t cursor, cur;               // first-seen rounds [cursor, cur) are folded
    const uint32_t *row_ptr, *col, *owner;
    const uint64_t *sub, *smask;
    uint8_t* tag;                      // [S][E] edge order
    int64_t* since;                    // [E]
    uint32_t* flags;                   // [0] a first sender that is no connection of the receiver, [1] a row longer than its class
    int32_t bump, cap;
    // the trim and the read-outs
    const uint8_t *mflags, *rstate, *direct;
    uint64_t seed;
    uint32_t tick;
    int64_t now, grace;
    int32_t low, high;
    uint32_t* mark;                    // [E / 32] chosen connections (their lower-to-higher edge)
    const uint32_t* rev;
};

struct ConnTags {
    gsim_conn_tag_params p{};
    uint8_t* d_tag = nullptr;          // [S][E] (ensure_slots re-lays it out: read it per call)
    int64_t* d_since = nullptr;        // [E]
    size_t bytes = 0;                  // counted in bytes_allocated
    int64_t cursor = 0;                // first round not folded yet
    int64_t next_k = 1;                // the next decay instant is t0 + next_k * interval
    TgMsg* d_sel = nullptr;
    int64_t sel_cap = 0;
    uint32_t* d_cnt = nullptr;         // [4]: k_select's count, fold flags [2], the collect counter
    uint32_t* d_mark = nullptr;        // [ceil(E / 32)] zero between calls
    uint32_t* d_pairs = nullptr;       // the trim's list
    int64_t pairs_cap = 0;
};

namespace {

constexpr char kTgName[] = "connection tags";
constexpr int kTgBlock = 256;
constexpr int64_t kSinceOld = INT64_MIN / 4;      // a connection older than any grace period
enum : int { TC_NSEL = 0, TC_BADSENDER, TC_LONGROW, TC_NPAIRS, kTC };

struct TgFill {
    using Row = TgMsg;
    __device__ static uint32_t fill(Row& r, const ReportView& v, int m, int64_t pub)
    {
        TgMsg x;
        fill_sel(x, v, m, pub);
        x.last = v.slot_last[m];
        x.verdict = v.minv[m];
        r = x;
        return x.topic;
    }
};

__device__ __forceinline__ int32_t planes_of(const TagArgs& a, uint64_t m)
{
    return a.smask ? (int32_t)__popcll(m) : a.S;
}

__global__ __launch_bounds__(kTgBlock) void k_tag_fold(TagArgs a)
{
    if (blockIdx.y >= a.flags[TC_NSEL]) return;                                     // (the grid covers the ring)
    const TgMsg mm = a.sel[blockIdx.y];
    if ((int64_t)mm.last < a.cursor || mm.verdict != GSIM_VERDICT_ACCEPT) return;   // block-uniform
    const int tid = threadIdx.x, lane = tid & 63;
    const int32_t t = (int32_t)mm.topic;
    const int64_t word = (int64_t)blockIdx.x * (kTgBlock / 64) + (tid >> 6);        // wave-uniform
    const int64_t p = word * 64 + lane;
    const bool active = p < a.n;
    const bool wave_on = word * 64 < a.n;
    const uint64_t c = lane_cell(a.cells, mm, word, lane, wave_on, active);
    const uint32_t hi = (uint32_t)(c >> 32);
    if (hi & kClaim) return;                                   // unseen (all ones) or a claim
    if ((int64_t)hi < a.cursor || (int64_t)hi >= a.cur || (uint32_t)p == mm.origin) return;
    if (!((a.sub[p] >> t) & 1ull)) return;                     // no decaying tag registered (bumpDeliveryTag)
    const uint64_t m = smask_of(a.smask, (uint32_t)p);
    if (!slot_has(m, t)) return;
    const uint32_t from = (uint32_t)c & kPeerMask;
    uint32_t lo = a.row_ptr[p], hi_e = a.row_ptr[p + 1];
    const uint32_t end = hi_e;
    while (lo < hi_e) {
        const uint32_t mid = lo + (hi_e - lo) / 2;
        if (a.col[mid] < from) lo = mid + 1; else hi_e = mid;
    }
    if (lo >= end || a.col[lo] != from) { a.flags[TC_BADSENDER] = 1u; return; }
    const int64_t i = slot_idx(m, t, a.E, (int64_t)lo);
    // the aligned word holding byte i (the planes' allocation ends on a word boundary)
    uint32_t* w = reinterpret_cast<uint32_t*>(a.tag + (i & ~(int64_t)3));
    const int sh = (int)(i & 3) * 8;
    uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const uint32_t v = (old >> sh) & 0xFFu;
        const uint32_t nv = v + (uint32_t)a.bump < (uint32_t)a.cap ? v + (uint32_t)a.bump : (uint32_t)a.cap;
        if (nv == v) break;                                    // at the cap
        const uint32_t want = (old & ~(0xFFu << sh)) | (nv << sh);
        const uint32_t got = atomicCAS(w, old, want);
        if (got == old) break;
        old = got;
    }
}

// dec = amount * instants crossed, at most 255
__global__ __launch_bounds__(256) void k_tag_decay(uint32_t* w, int64_t nwords, uint32_t dec)
{
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < nwords; x += (int64_t)gridDim.x * 256) {
        const uint32_t v = w[x];
        if (!v) continue;
        uint32_t r = 0;
#pragma unroll
        for (int b = 0; b < 32; b += 8) {
            const uint32_t y = (v >> b) & 0xFFu;
            r |= (y > dec ? y - dec : 0u) << b;
        }
        w[x] = r;
    }
}

// One thread per (connection, direction).  The four bytes of a word may belong
// to four listed connections: each byte is cleared with an atomicAnd on its word.
__global__ __launch_bounds__(256) void k_tag_drop(TagArgs a, const uint32_t* edges, int32_t n2, int32_t up)
{
    const int32_t q = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (q >= n2) return;
    const uint32_t e = edges[q];
    if ((int64_t)e >= a.E) return;
    const int32_t np = planes_of(a, smask_of(a.smask, a.owner[e]));
    for (int32_t s = 0; s < np; ++s) {
        const int64_t i = (int64_t)s * a.E + e;
        if (a.tag[i]) atomicAnd(reinterpret_cast<uint32_t*>(a.tag + (i & ~(int64_t)3)), ~(0xFFu << ((int)(i & 3) * 8)));
    }
    if (up) a.since[e] = a.now;
}

// One wave per (peer, topic) pair of a Leave.
__global__ __launch_bounds__(64) void k_tag_leave(TagArgs a, const uint32_t* pairs, int32_t count)
{
    const int32_t q = (int32_t)blockIdx.x;
    if (q >= count) return;
    const uint32_t p = pairs[2 * q];
    const int32_t t = (int32_t)pairs[2 * q + 1];
    if ((int64_t)p >= a.n || t >= a.T) return;
    const uint64_t m = smask_of(a.smask, p);
    if (!slot_has(m, t)) return;
    const uint32_t b = a.row_ptr[p], en = a.row_ptr[p + 1];
    for (uint32_t e = b + threadIdx.x; e < en; e += 64) {
        const int64_t i = slot_idx(m, t, a.E, (int64_t)e);
        if (a.tag[i]) atomicAnd(reinterpret_cast<uint32_t*>(a.tag + (i & ~(int64_t)3)), ~(0xFFu << ((int)(i & 3) * 8)));
    }
}

__global__ __launch_bounds__(256) void k_tag_fill_i64(int64_t* p, int64_t n, int64_t v)
{
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (int64_t)gridDim.x * 256) p[x] = v;
}

// the planes under grown slot masks (engine.hip k_slot_relayout's rule; dst is zeroed)
__global__ __launch_bounds__(256) void k_tag_relayout(const uint8_t* src, uint8_t* dst, const uint32_t* owner,
                                                      const uint64_t* m0s, const uint64_t* m1s, int64_t E)
{
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < E; x += (int64_t)gridDim.x * 256) {
        const uint64_t m0 = smask_of(m0s, owner[x]), m1 = smask_of(m1s, owner[x]);
        int32_t p1 = 0;
        for (uint64_t b = m1; b; b &= b - 1, ++p1) {
            const int32_t t = __builtin_ctzll(b);
            if (slot_has(m0, t)) dst[(int64_t)p1 * E + x] = src[slot_idx(m0, t, E, x)];
        }
    }
}

__global__ __launch_bounds__(256) void k_tag_view(TagArgs a, int32_t t, uint8_t* out)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * 256) {
        const uint64_t m = smask_of(a.smask, a.owner[e]);
        out[e] = slot_has(m, t) ? a.tag[slot_idx(m, t, a.E, e)] : (uint8_t)0;
    }
}

// value(e) and GSIM_CONN_* of edge e of a row owner with slot mask m
__device__ __forceinline__ void edge_value(const TagArgs& a, uint64_t m, int64_t e, int32_t& value, uint32_t& fl)
{
    const int32_t np = planes_of(a, m);
    int32_t v = 0;
    bool prot = a.direct[e] != 0;
    for (int32_t s = 0; s < np; ++s) {
        v += a.tag[(int64_t)s * a.E + e];                      // (a plane of a topic the router left holds zeros)
        prot = prot || (a.mflags[(int64_t)s * a.E + e] & GSIM_TF_MESH);
    }
    value = v;
    fl = (a.rstate[e] & GSIM_ES_CONNECTED ? GSIM_CONN_CONNECTED : 0u) | (prot ? GSIM_CONN_PROTECTED : 0u) |
         (a.since[e] > a.now - a.grace ? GSIM_CONN_GRACE : 0u);
}

__global__ __launch_bounds__(256) void k_tag_values(TagArgs a, int32_t* value, uint8_t* flags)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * 256) {
        int32_t v;
        uint32_t fl;
        edge_value(a, smask_of(a.smask, a.owner[e]), e, v, fl);
        if (value) value[e] = v;
        if (flags) flags[e] = (uint8_t)fl;
    }
}

__device__ __forceinline__ bool trims(const TagArgs& a, int32_t nconn)
{
    return a.high > 0 ? nconn > a.high : nconn > a.low;
}

// the connection of edge e (row i, neighbour j) closes: its lower-to-higher edge is marked
__device__ __forceinline__ void mark_close(const TagArgs& a, uint32_t i, uint32_t j, uint32_t e)
{
    const uint32_t x = i < j ? e : a.rev[e];
    atomicOr(a.mark + (x >> 5), 1u << (x & 31));
}

__device__ __forceinline__ bool key_less(uint32_t v1, uint64_t k1, uint32_t v2, uint64_t k2)
{
    return v1 < v2 || (v1 == v2 && k1 < k2);
}

constexpr uint32_t kNoCand = 0xFFFFFFFFu;         // the value of a position that is no candidate (above every sum)

template <int W>
__global__ __launch_bounds__(kTgBlock) void k_tag_trim(TagArgs a, const uint32_t* rows, int64_t nrows, int64_t base)
{
    static_assert(W == 16 || W == 32 || W == 64, "a lane group per row");
    constexpr int G = 64 / W;
    const int lane = threadIdx.x & 63, gl = lane % W, gsh = lane - gl;
    const uint64_t gm = W == 64 ? ~0ull : ((1ull << W) - 1ull);
    const int64_t ngroups = (nrows + G - 1) / G * G;              // a wave's groups leave the loop together
    for (int64_t x = ((int64_t)blockIdx.x * kTgBlock + threadIdx.x) / W; x < ngroups;
         x += (int64_t)gridDim.x * kTgBlock / W) {
        const bool row_ok = x < nrows;
        const uint32_t i = row_ok ? (rows ? rows[x] : (uint32_t)(base + x)) : 0u;
        const uint32_t b = row_ok ? a.row_ptr[i] : 0u;
        uint32_t deg = row_ok ? a.row_ptr[i + 1] - b : 0u;
        if (deg > (uint32_t)W) { if (gl == 0) a.flags[TC_LONGROW] = 1u; deg = 0; }   // (not a row of this class)
        const bool on = (uint32_t)gl < deg;
        const uint32_t e = b + (uint32_t)gl;
        uint32_t val = kNoCand, fl = 0, j = 0;
        uint64_t key = 0;
        if (on) {
            int32_t v;
            edge_value(a, smask_of(a.smask, i), (int64_t)e, v, fl);
            j = a.col[e];
            if (fl == GSIM_CONN_CONNECTED) {                      // connected, not protected, out of grace
                val = (uint32_t)v;
                key = select_key(a.seed, a.tick, i, 0u, P_TRIM, j, (uint32_t)gl);
            }
        }
        const int32_t nconn = (int32_t)__popcll((__ballot(on && (fl & GSIM_CONN_CONNECTED)) >> gsh) & gm);
        const bool act = row_ok && trims(a, nconn);
        if (!__ballot(act)) continue;                             // wave-uniform
        const int32_t k = nconn - a.low;
        int32_t rank = 0;
        for (int s = 0; s < W; ++s) {
            const uint32_t ov = (uint32_t)__shfl((int)val, gsh + s, 64);
            const uint64_t ok = (uint64_t)__shfl((unsigned long long)key, gsh + s, 64);
            rank += ov != kNoCand && key_less(ov, ok, val, key);
        }
        if (act && val != kNoCand && rank < k) mark_close(a, i, j, e);
    }
}

// A block per hub row, any length: the thread ranks position c0 + tid against the
// row's candidates, a tile of kTgBlock positions at a time.
__global__ __launch_bounds__(kTgBlock) void k_tag_trim_hub(TagArgs a, const uint32_t* rows, int64_t nrows)
{
    __shared__ uint32_t s_val[kTgBlock];
    __shared__ uint64_t s_key[kTgBlock];
    const int tid = threadIdx.x;
    for (int64_t x = blockIdx.x; x < nrows; x += gridDim.x) {     // block-uniform
        const uint32_t i = rows[x];
        const uint32_t b = a.row_ptr[i], deg = a.row_ptr[i + 1] - b;
        const uint64_t m = smask_of(a.smask, i);
        int32_t nconn = 0;
        for (uint32_t q0 = 0; q0 < deg; q0 += kTgBlock)
            nconn += __syncthreads_count(q0 + tid < deg && (a.rstate[b + q0 + tid] & GSIM_ES_CONNECTED));
        if (!trims(a, nconn)) continue;
        const int32_t k = nconn - a.low;
        auto load = [&](uint32_t q, uint32_t& val, uint64_t& key) {
            val = kNoCand;
            key = 0;
            if (q >= deg) return;
            int32_t v;
            uint32_t fl;
            edge_value(a, m, (int64_t)(b + q), v, fl);
            if (fl != GSIM_CONN_CONNECTED) return;
            val = (uint32_t)v;
            key = select_key(a.seed, a.tick, i, 0u, P_TRIM, a.col[b + q], q);
        };
        for (uint32_t c0 = 0; c0 < deg; c0 += kTgBlock) {
            uint32_t val;
            uint64_t key;
            load(c0 + tid, val, key);
            int32_t rank = 0;
            for (uint32_t t0 = 0; t0 < deg; t0 += kTgBlock) {
                __syncthreads();                                  // the last tile was read
                load(t0 + tid, s_val[tid], s_key[tid]);
                __syncthreads();
                if (val != kNoCand)
                    for (int s = 0; s < kTgBlock; ++s) rank += s_val[s] != kNoCand && key_less(s_val[s], s_key[s], val, key);
            }
            if (val != kNoCand && rank < k) mark_close(a, i, a.col[b + c0 + tid], b + c0 + tid);
        }
        __syncthreads();
    }
}

// The marked edges as (row owner, neighbour) pairs, unordered; pairs == nullptr
// counts only.  clear: the marks go back to zero.
__global__ __launch_bounds__(256) void k_tag_collect(TagArgs a, int64_t nwords, uint32_t* pairs, int64_t cap, int32_t clear)
{
    for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * 256) {
        uint32_t bits = a.mark[w];
        if (!bits) continue;
        if (clear) a.mark[w] = 0u;
        const uint32_t k0 = atomicAdd(&a.flags[TC_NPAIRS], (uint32_t)__popc(bits));
        if (!pairs) continue;
        for (uint32_t k = k0; bits; bits &= bits - 1, ++k) {
            const int64_t e = w * 32 + (__ffs(bits) - 1);
            if ((int64_t)k < cap && e < a.E) { pairs[2 * k] = a.owner[e]; pairs[2 * k + 1] = a.col[e]; }
        }
    }
}

int tags_enter(gsim_handle* h, bool need_config)
{
    if (!h) return GSIM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->sh) { h->err = "connection tags run on a single engine, not on a shard of a group"; return GSIM_ESTATE; }
    if (h->e == 0 || !h->x) { h->err = "no graph loaded"; return GSIM_ESTATE; }
    if (!h->dl) { h->err = "gsim_msgs_init not called"; return GSIM_ESTATE; }
    if (need_config && !h->ct) { h->err = "gsim_conn_tags_config has not been called"; return GSIM_ESTATE; }
    return GSIM_OK;
}

// the planes' allocation ends on a word boundary: the kernels address a byte through its aligned 32-bit word
size_t plane_bytes(int32_t S, int64_t E)
{
    return ((size_t)std::max<int32_t>(S, 1) * (size_t)E + 3) & ~(size_t)3;
}
size_t plane_bytes(const gsim_handle* h) { return plane_bytes(h->S, h->e); }

TagArgs make_args(gsim_handle* h)
{
    ConnTags* c = h->ct;
    TagArgs a{};
    a.sel = c->d_sel;
    a.n = h->n; a.E = h->e; a.T = std::max(1, h->t); a.S = std::max<int32_t>(h->S, 1);
    a.row_ptr = h->d_row_ptr; a.col = h->d_col; a.owner = h->d_owner; a.rev = h->d_rev;
    a.sub = h->d_sub; a.smask = h->d_smask;
    a.tag = c->d_tag; a.since = c->d_since; a.flags = c->d_cnt;
    a.bump = c->p.bump; a.cap = c->p.cap;
    a.mflags = h->d_mflags; a.rstate = h->d_rstate; a.direct = h->d_direct;
    a.mark = c->d_mark;
    return a;
}

uint32_t grid_of(int64_t n) { return (uint32_t)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384)); }

}  // namespace
}  // namespace gsim

using namespace gsim;

void conntags_release(gsim_handle* h)
{
    ConnTags* c = h->ct;
    if (!c) return;
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_all({c->d_tag, c->d_since, c->d_sel, c->d_cnt, c->d_mark, c->d_pairs});
    h->bytes_allocated -= std::min(h->bytes_allocated, c->bytes);
    delete c;
    h->ct = nullptr;
}

int conntags_relayout(gsim_handle* h, const uint64_t* m0, const uint64_t* m1, int32_t S0, int32_t S1)
{
    ConnTags* c = h->ct;
    if (!c) return GSIM_OK;
    const size_t pb = plane_bytes(S1, h->e), old = plane_bytes(S0, h->e);
    uint8_t* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, pb);
    if (e != hipSuccess) { h->err = std::string("connection tags: ") + hipGetErrorString(e); return GSIM_ENOMEM; }
    e = hipMemsetAsync(q, 0, pb, h->stream);                  // (the bytes after the last plane too)
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tag_relayout, dim3(grid_of(h->e)), dim3(256), 0, h->stream, (const uint8_t*)c->d_tag, q,
                           (const uint32_t*)h->d_owner, m0, m1, h->e);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { (void)hipFree(q); return hip_check(h, e, "k_tag_relayout"); }
    (void)hipFree(c->d_tag);
    c->d_tag = q;
    c->bytes += pb - old;
    h->bytes_allocated += pb - old;
    return GSIM_OK;
}

int conntags_fold(gsim_handle* h)
{
    ConnTags* c = h->ct;
    if (!c) return GSIM_OK;
    int rc = deliver_flush(h);                     // the last round's claims become first-seen rounds
    if (rc) return rc;
    const int64_t cur = deliver_next_round(h);
    if (cur < c->cursor) c->cursor = cur;          // (gsim_msgs_init was called again: the rounds start over)
    if (cur <= c->cursor) return GSIM_OK;
    ReportView v{};
    if (!deliver_report_view(h, &v)) return GSIM_OK;
    rc = grow(h, kTgName, &c->d_sel, &c->sel_cap, (int64_t)std::max<int32_t>(v.ring, 1));
    if (rc) return rc;
    hipLaunchKernelGGL((k_select<TgFill, 0>), dim3(1), dim3(kSelBlock), 0, h->stream, v, (int64_t)0, cur, c->d_sel,
                       c->d_cnt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_check(h, e, "connection tags: selection");
    {
        // a block row per ring slot, the rows past the selection's count leave at once: no host read per tick
        TagArgs a = make_args(h);
        a.cells = v.cells;
        a.cursor = c->cursor; a.cur = cur;
        const int64_t words = (h->n + 63) >> 6;
        const dim3 grid((uint32_t)((words + kTgBlock / 64 - 1) / (kTgBlock / 64)), (uint32_t)std::max<int32_t>(v.ring, 1));
        hipLaunchKernelGGL(k_tag_fold, grid, dim3(kTgBlock), 0, h->stream, a);
        e = hipGetLastError();
        if (e != hipSuccess) return hip_check(h, e, "k_tag_fold");
    }
    c->cursor = cur;
    return GSIM_OK;
}

int conntags_publish(gsim_handle* h, int64_t round, int64_t guard)
{
    ConnTags* c = h->ct;
    if (!c || round - c->cursor < std::max<int64_t>(guard, 1)) return GSIM_OK;
    return conntags_fold(h);
}

int conntags_refresh(gsim_handle* h, int64_t now)
{
    ConnTags* c = h->ct;
    if (!c) return GSIM_OK;
    int rc = conntags_fold(h);
    if (rc) return rc;
    // the instants t0 + k * interval, k >= next_k, that `now` has reached
    if (now < c->p.t0_ns) return GSIM_OK;
    const int64_t reached = (now - c->p.t0_ns) / c->p.decay_interval_ns;
    if (reached < c->next_k) return GSIM_OK;
    const int64_t times = reached - c->next_k + 1;
    c->next_k = reached + 1;
    const uint32_t dec = (uint32_t)std::min<int64_t>(255, std::min<int64_t>(times, 255) * (int64_t)c->p.decay_amount);
    const int64_t nwords = (int64_t)(plane_bytes(h) / 4);
    hipLaunchKernelGGL(k_tag_decay, dim3(grid_of(nwords)), dim3(256), 0, h->stream, reinterpret_cast<uint32_t*>(c->d_tag),
                       nwords, dec);
    return hip_check(h, hipGetLastError(), "k_tag_decay");
}

int conntags_connections(gsim_handle* h, const uint32_t* d_edges, int32_t n2, int32_t up, int64_t now)
{
    if (!h->ct || n2 <= 0) return GSIM_OK;
    int rc = conntags_fold(h);
    if (rc) return rc;
    TagArgs a = make_args(h);
    a.now = now;
    hipLaunchKernelGGL(k_tag_drop, dim3((uint32_t)((n2 + 255) / 256)), dim3(256), 0, h->stream, a, d_edges, n2, up ? 1 : 0);
    return hip_check(h, hipGetLastError(), "k_tag_drop");
}

int conntags_leave(gsim_handle* h, const uint32_t* d_pairs, int32_t count)
{
    if (!h->ct || count <= 0) return GSIM_OK;
    TagArgs a = make_args(h);
    hipLaunchKernelGGL(k_tag_leave, dim3((uint32_t)count), dim3(64), 0, h->stream, a, d_pairs, count);
    return hip_check(h, hipGetLastError(), "k_tag_leave");
}

extern "C" {

int gsim_default_conn_tag_params(int64_t t0_ns, gsim_conn_tag_params* out)
{
    if (!out) return GSIM_EINVAL;
    *out = gsim_conn_tag_params{};
    out->bump = 1;                                 // GossipSubConnTagBumpMessageDelivery
    out->cap = 15;                                 // GossipSubConnTagMessageDeliveryCap
    out->decay_amount = 1;                         // GossipSubConnTagDecayAmount
    out->decay_interval_ns = 600000000000ll;       // GossipSubConnTagDecayInterval
    out->t0_ns = t0_ns;
    return GSIM_OK;
}

int gsim_conn_tags_config(gsim_handle* h, const gsim_conn_tag_params* p)
{
    int rc = tags_enter(h, false);
    if (rc) return rc;
    if (p && (p->cap < 1 || p->cap > 255 || p->bump < 1 || p->decay_amount < 1 || p->decay_interval_ns <= 0)) {
        h->err = "connection tags: cap in 1..255, bump >= 1, decay_amount >= 1 and decay_interval_ns > 0";
        return GSIM_EINVAL;
    }
    conntags_release(h);
    if (!p) return GSIM_OK;
    if (deliver_latency_on(h)) {
        // copies may be pending validation: they commit at their completion round, with near-first peers beside them
        h->err = "connection tags cannot be configured once a message with a validation latency (vdelay > 0) was published";
        return GSIM_ESTATE;
    }
    rc = deliver_flush(h);
    if (rc) return rc;
    ConnTags* c = new ConnTags();
    h->ct = c;
    c->p = *p;
    c->cursor = deliver_next_round(h);
    const size_t pb = plane_bytes(h), words = ((size_t)h->e + 31) / 32;
    hipError_t e = hipMalloc((void**)&c->d_tag, pb);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_since, sizeof(int64_t) * (size_t)h->e);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_cnt, sizeof(uint32_t) * kTC);
    if (e == hipSuccess) e = hipMalloc((void**)&c->d_mark, sizeof(uint32_t) * words);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_tag, 0, pb, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_cnt, 0, sizeof(uint32_t) * kTC, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_mark, 0, sizeof(uint32_t) * words, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tag_fill_i64, dim3(grid_of(h->e)), dim3(256), 0, h->stream, c->d_since, h->e, kSinceOld);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {                                     // the selection's rows: a slot of the ring each
        ReportView v{};
        (void)deliver_report_view(h, &v);
        c->sel_cap = std::max<int32_t>(v.ring, 1);
        e = hipMalloc((void**)&c->d_sel, sizeof(TgMsg) * (size_t)c->sel_cap);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        conntags_release(h);
        h->err = std::string("connection tags: ") + hipGetErrorString(e);
        return GSIM_ENOMEM;
    }
    c->bytes = pb + sizeof(int64_t) * (size_t)h->e + sizeof(uint32_t) * (kTC + words);
    h->bytes_allocated += c->bytes;
    return GSIM_OK;
}

// the fold's error flag: a committed cell names a first sender the receiver has no connection to
static int tags_check(gsim_handle* h)
{
    uint32_t fl[kTC] = {};
    const hipError_t e = stream_copy(h, fl, h->ct->d_cnt, sizeof fl, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "connection tags: flags");
    if (fl[TC_BADSENDER] || fl[TC_LONGROW])                    // reported once: the next call starts clean
        (void)hipMemsetAsync(h->ct->d_cnt + TC_BADSENDER, 0, 2 * sizeof(uint32_t), h->stream);
    if (fl[TC_BADSENDER]) {
        h->err = "connection tags: a committed cell names a first sender that is no connection of the receiver";
        return GSIM_ESTATE;
    }
    if (fl[TC_LONGROW]) { h->err = "connection tags: a row is longer than its row class"; return GSIM_ESTATE; }
    return GSIM_OK;
}

int gsim_conn_tags_read(gsim_handle* h, int32_t topic, uint8_t* out)
{
    int rc = tags_enter(h, true);
    if (rc) return rc;
    if (!out || topic < 0 || topic >= std::max(1, h->t)) { h->err = "gsim_conn_tags_read: topic out of range"; return GSIM_EINVAL; }
    rc = conntags_fold(h);
    if (rc) return rc;
    uint8_t* d_out = nullptr;
    hipError_t e = hipMalloc((void**)&d_out, (size_t)h->e);
    if (e != hipSuccess) { h->err = std::string("gsim_conn_tags_read: ") + hipGetErrorString(e); return GSIM_ENOMEM; }
    const TagArgs a = make_args(h);
    hipLaunchKernelGGL(k_tag_view, dim3(grid_of(h->e)), dim3(256), 0, h->stream, a, topic, d_out);
    e = hipGetLastError();
    if (e == hipSuccess) e = stream_copy(h, out, d_out, (size_t)h->e, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return hip_check(h, e, "gsim_conn_tags_read");
    return tags_check(h);
}

int gsim_conn_values(gsim_handle* h, int64_t now, int64_t grace_ns, int32_t* value, uint8_t* flags)
{
    int rc = tags_enter(h, true);
    if (rc) return rc;
    if (grace_ns < 0) { h->err = "gsim_conn_values: grace_ns >= 0"; return GSIM_EINVAL; }
    rc = conntags_fold(h);
    if (rc) return rc;
    if (!value && !flags) return tags_check(h);    // the fold alone
    int32_t* d_val = nullptr;
    uint8_t* d_fl = nullptr;
    hipError_t e = hipSuccess;
    if (value) e = hipMalloc((void**)&d_val, sizeof(int32_t) * (size_t)h->e);
    if (e == hipSuccess && flags) e = hipMalloc((void**)&d_fl, (size_t)h->e);
    if (e != hipSuccess) {
        free_all({d_val, d_fl});
        h->err = std::string("gsim_conn_values: ") + hipGetErrorString(e);
        return GSIM_ENOMEM;
    }
    TagArgs a = make_args(h);
    a.now = now; a.grace = grace_ns;
    hipLaunchKernelGGL(k_tag_values, dim3(grid_of(h->e)), dim3(256), 0, h->stream, a, d_val, d_fl);
    e = hipGetLastError();
    if (e == hipSuccess && value) e = stream_copy(h, value, d_val, sizeof(int32_t) * (size_t)h->e, hipMemcpyDeviceToHost);
    if (e == hipSuccess && flags) e = stream_copy(h, flags, d_fl, (size_t)h->e, hipMemcpyDeviceToHost);
    free_all({d_val, d_fl});
    if (e != hipSuccess) return hip_check(h, e, "gsim_conn_values");
    return tags_check(h);
}

int gsim_conn_trim(gsim_handle* h, uint64_t tick, int64_t now, int32_t low, int32_t high, int64_t grace_ns,
                   uint32_t* pairs, int64_t cap, int64_t* n)
{
    int rc = tags_enter(h, true);
    if (rc) return rc;
    if (!n || low < 0 || high < 0 || grace_ns < 0 || cap < 0 || (high > 0 && low > high)) {
        h->err = "gsim_conn_trim: 0 <= low, 0 <= high, grace_ns >= 0 and (high == 0 or low <= high)";
        return GSIM_EINVAL;
    }
    *n = 0;
    ConnTags* c = h->ct;
    rc = conntags_fold(h);
    if (rc) return rc;
    TagArgs a = make_args(h);
    a.seed = gsim_get_seed(h); a.tick = (uint32_t)tick;
    a.now = now; a.grace = grace_ns; a.low = low; a.high = high;
    const int64_t nwords = (h->e + 31) / 32;
    const bool want = pairs && cap > 0;
    // the marks are zero between calls: whatever ends the call before the listing pass cleared them clears them here
    bool marked = false;
    auto fail = [&](int code) {
        if (marked) (void)hipMemsetAsync(c->d_mark, 0, sizeof(uint32_t) * (size_t)nwords, h->stream);
        return code;
    };
    hipError_t e = hipMemsetAsync(c->d_cnt + TC_NPAIRS, 0, sizeof(uint32_t), h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_conn_trim");
    marked = true;
    launch_row_classes(h, kTgBlock, [&](auto w, dim3 grid, const uint32_t* rows, int64_t nrows, int64_t base) {
        constexpr int W = decltype(w)::value;
        if constexpr (W == 0)
            hipLaunchKernelGGL(k_tag_trim_hub, grid, dim3(kTgBlock), 0, h->stream, a, rows, nrows);
        else
            hipLaunchKernelGGL(k_tag_trim<W>, grid, dim3(kTgBlock), 0, h->stream, a, rows, nrows, base);
    });
    e = hipGetLastError();
    uint32_t cnt = 0;
    if (e == hipSuccess) {
        // the count first (without a buffer the pass clears the marks as it goes)
        hipLaunchKernelGGL(k_tag_collect, dim3(grid_of(nwords)), dim3(256), 0, h->stream, a, nwords, (uint32_t*)nullptr,
                           (int64_t)0, want ? 0 : 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = stream_copy(h, &cnt, c->d_cnt + TC_NPAIRS, sizeof cnt, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(hip_check(h, e, "gsim_conn_trim"));
    if (!want) marked = false;
    *n = cnt;
    rc = tags_check(h);
    if (rc) return fail(rc);
    if (!want || cnt == 0) return fail(GSIM_OK);
    if ((int64_t)cnt > cap) { h->err = "gsim_conn_trim: pair buffer too small"; return fail(GSIM_ERANGE); }
    rc = grow(h, kTgName, &c->d_pairs, &c->pairs_cap, 2 * (int64_t)cnt);
    if (rc) return fail(rc);
    e = hipMemsetAsync(c->d_cnt + TC_NPAIRS, 0, sizeof(uint32_t), h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tag_collect, dim3(grid_of(nwords)), dim3(256), 0, h->stream, a, nwords, c->d_pairs, (int64_t)cnt, 1);
        e = hipGetLastError();
    }
    std::vector<uint32_t> pv(2 * (size_t)cnt);
    if (e == hipSuccess) e = stream_copy(h, pv.data(), c->d_pairs, sizeof(uint32_t) * pv.size(), hipMemcpyDeviceToHost);
    // (a listing pass that ran cleared the marks; one that did not left them)
    if (e != hipSuccess) return fail(hip_check(h, e, "gsim_conn_trim pairs"));
    marked = false;
    std::vector<std::pair<uint32_t, uint32_t>> pr((size_t)cnt);
    for (size_t q = 0; q < cnt; ++q) pr[q] = {pv[2 * q], pv[2 * q + 1]};
    std::sort(pr.begin(), pr.end());
    for (size_t q = 0; q < cnt; ++q) { pairs[2 * q] = pr[q].first; pairs[2 * q + 1] = pr[q].second; }
    // every listed pair is a connection, marked once: the same path as a caller's list
    return gsim_set_connections(h, pairs, (int32_t)cnt, 0, now);
}

}  // extern "C"
