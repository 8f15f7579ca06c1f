// Relay report (include/gsim.h gsim_relay_report): the first-delivery forest of
// the messages still in the ring, read from the sender's side.  Every committed
// seen-set cell names the peer whose copy the receiver saw first (its low word,
// gsim_internal.h), so the tree that delivered a message is resident; this file
// counts, per sender, per (topic, class of the sender) and per message, the
// children every holder has, the depth of every holder and the rounds every hop
// took.  The reference has no such read-out; what is counted is the peer that
// markFirstMessageDelivery credits (score.go:919-946), summed at that peer.
//
// The selected slots (the reports' shared selection, k_select<RlFill>) are processed in
// batches of B.  The batch's scratch is cnt[B][n] (u32 children) and dep[B][n]
// (u16 depth code), indexed by the LOCAL PEER ID on the dense ring and on
// member-compacted sub-rings alike: a first sender is a local id, so a parent's
// entry needs no rank lookup, the fold needs no member bitmap, and on a sharded
// group a ghost's entry translates to its owner's by the peer id alone.  (The
// parent's CELL is found by member rank, Cells::at, for the orphan check.)
// B = budget / (6 n) (10 n on a group, which stages the ghosts' counts), the
// budget 256 MiB unless gsim_relay_report_budget says otherwise.
//
// Launches per batch (none per slot or per peer, no host loop over either); in
// every kernel a lane owns a peer, a wave the 64 peers of one member-bitmap word:
//   k_relay_push   grid (peer blocks, slots of the batch): the lane's cell of the
//                  block's slot, coalesced.  A committed non-origin cell does one
//                  non-returning atomicAdd on cnt[b][parent] (and, with more than
//                  one class, one on cto[parent][class of the child]), reads the
//                  parent's cell (orphan, delay) and stores its depth code:
//                  0xFFFF no committed cell, 0 the origin, 0x8000 an orphan,
//                  0x4000 | latency otherwise (depth pending).  Reached, orphans,
//                  the delay bins, the largest latency and the (sender class,
//                  child class) counts are reduced per wave (__ballot, __popcll)
//                  into block LDS, flushed with one global atomic per non-zero
//                  entry.
//   k_relay_fold   grid (peer blocks, parts of the batch): the lane walks the
//                  part's slots and reads cnt and dep: held, relayed messages,
//                  children, own children and the largest fan-out stay in
//                  registers and meet the peer's row in atomics; the fan-out bin
//                  of every (slot, holder) goes to the block's LDS counters, sized
//                  to the live T * C (33 words per (topic, class)), by the distinct
//                  (class, bin) keys of the wave, flushed with one global atomic
//                  per non-zero entry; a message's relays and its widest holder
//                  (lowest id on a tie: an atomicMax on children << 32 | ~peer)
//                  take one atomic per wave and slot.
//   k_relay_depth  only for message rows, level-synchronous by latency: pass L
//                  resolves the codes 0x4000 | L to depth[parent] + 1, which is
//                  final by then because a parent's round is strictly smaller.
//                  The passes of a batch are its largest latency, read with one
//                  8-byte host read.  A pass reads 2 bytes per (slot, peer) and
//                  the cell only of the lanes it resolves.
//   k_relay_bins   depth histogram and exact maximum per slot through block LDS.
// Everything is an integer: no result depends on order.
//
// An orphan (the parent holds no committed cell in the slot, or one with a round
// not smaller than the child's; a cell older than its publication) gets no
// depth and no delay and the call returns GSIM_ESTATE after writing the rows;
// its descendants take their depth from it as a root of depth 0.  A latency of
// 16383 rounds or more cannot be coded: with message rows asked for, GSIM_ERANGE.
//
// A shard walks the peers it owns (gsim_group_relay_report, shard.hip): the
// pushes of every shard, then the ghosts' cnt entries added into their owners'
// through the host, then the folds; a ghost parent's cell is not checked (its
// shard keeps it at tick granularity only).
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage): no kernel uses
// scratch memory or spills a register, all run at 8 waves/SIMD:
//   k_relay_push<false>   19 VGPRs, 69 SGPRs, 112 bytes of LDS
//   k_relay_push<true>    20 VGPRs, 72 SGPRs, 112 bytes of LDS
//   k_relay_fold<false>   30 VGPRs, 55 SGPRs, dynamic LDS only (132 bytes per live (topic, class))
//   k_relay_fold<true>    30 VGPRs, 57 SGPRs, likewise
//   k_relay_depth         12 VGPRs, 30 SGPRs, no LDS
//   k_relay_bins           6 VGPRs, 20 SGPRs, 132 bytes of LDS
//   k_select<RlFill>      30 VGPRs, 53 SGPRs, 324 bytes of LDS
//   k_relay_peers<CLS>   8-10 VGPRs, 22-26 SGPRs, no LDS;  k_relay_add 8 VGPRs, 20 SGPRs
// Measured (profiles/relay_report_c3.txt): C3 after the default
// bench's ticks, 1477 messages, 1.43e9 first deliveries, batches of 44 slots: the
// per-peer rows 96.0 ms, with the class rows 101.0, with the message rows 187.5
// (630 depth passes), against 6.6 ms for gsim_peer_report on the same cells
// (ratios 14.6, 15.3, 28.5); with two classes 155.7 / 162.1 / 248.6 against 14.1.
// The push pass and its memsets alone take 86.7 ms: at least 1.65e10 scattered
// u32 atomics per second, each beside a random 8-byte read of the parent's cell.
#include <algorithm>
#include <cstring>
#include <vector>

#include "report_common.h"

namespace gsim {

// one selected message as the walk reads it: SelMsg's fields (report_common.h), then the slot
struct RlMsg {
    uint64_t base;      // first cell of the slot
    uint32_t len;       // its cells
    uint32_t pub;       // publication round
    uint32_t topic, origin, slot, _pad;
};

// per selected message, u32 words on the device
enum : int {
    RM_REACHED = 0, RM_ORPHANS, RM_RELAYS, RM_LATMAX, RM_DEPTHMAX, RM_PAD,
    RM_MAXKEY,                                   // u64 (words 6-7): children << 32 | ~peer
    RM_DELAY = 8,                                // [8]
    RM_DEPTH = 16,                               // [GSIM_REPORT_BINS]
    kRM = RM_DEPTH + GSIM_REPORT_BINS,           // 48
};
// per (topic, class of the sender), u64 in global memory
enum : int {
    RC_PEERS = 0, RC_MAX,
    RC_CTO,                                      // [GSIM_NET_CLASSES] from the push
    RC_FAN = RC_CTO + GSIM_NET_CLASSES,          // [GSIM_REPORT_BINS] from the fold
    kRC = RC_FAN + GSIM_REPORT_BINS,             // 38
};
// the fold's LDS row per (topic, class), u32
enum : int { RL_FAN = 0, RL_MAX = GSIM_REPORT_BINS, kRL };   // 33
constexpr size_t kRlAcc = (size_t)GSIM_MAX_TOPICS * GSIM_NET_CLASSES * kRC;
// the call's flags; RF_BLAT (the batch's largest latency) and RF_BPAD (unused, zero) are the
// 8 bytes cleared before every push and read by the host before the depth passes
enum : int { RF_NSEL = 0, RF_BAD, RF_ORPH, RF_DEEP, RF_BLAT, RF_BPAD, RF_TOPIC, kRF = RF_TOPIC + GSIM_MAX_TOPICS };

constexpr uint16_t kDepNone = 0xFFFFu, kDepOrphan = 0x8000u, kDepPending = 0x4000u, kDepLatMax = 0x3FFFu;
constexpr int64_t kRlBudget = 256ll << 20;

struct RelayArgs {
    Cells cells;
    const RlMsg* sel;
    const uint8_t* cls;
    int32_t T, C;
    int64_t n;                                   // local peers
    int64_t rlo, rhi;                            // owned peers
    int64_t qlo, qhi;                            // peers the fold walks
    int64_t olo, ohi;                            // peers whose rows are written, rows[p - olo]
    uint32_t* cnt;                               // [B][n]
    uint16_t* dep;                               // [B][n]
    unsigned long long* cto;                     // [n][C], nullptr with one class
    unsigned long long* acc;                     // class counters (nullptr: none)
    uint32_t* macc;                              // [nsel][kRM]
    uint32_t* flags;                             // [kRF]
    gsim_relay_row* rows;
    int64_t k0;                                  // first selected message of the batch
    int32_t nb;                                  // its messages
    int32_t per;                                 // the fold: slots per part
    int32_t level;                               // the depth pass
    int32_t want_msgs;
};

struct RelayReport {
    RlMsg* d_sel = nullptr;
    uint32_t* d_flags = nullptr;
    unsigned long long* d_acc = nullptr;
    uint32_t* d_macc = nullptr;                  // [ring][kRM]
    int64_t sel_cap = 0, macc_cap = 0;           // entries of sel, words of macc
    uint32_t* d_cnt = nullptr;
    uint16_t* d_dep = nullptr;
    uint32_t* d_inc = nullptr;                   // a shard: the ghosts' counts from the other shards
    int64_t slots_cap = 0, dep_cap = 0, inc_cap = 0;   // entries of cnt, of dep, of inc
    unsigned long long* d_cto = nullptr;
    int64_t cto_cap = 0;
    gsim_relay_row* d_rows = nullptr;
    int64_t rows_cap = 0;
    int64_t budget = 0;                          // 0: kRlBudget
    int64_t last[4] = {0, 0, 0, 0};              // gsim_relay_report_launch
    // the call in progress (relay_begin .. relay_finish)
    ReportView v{};
    RelayArgs a{};
    uint32_t cs[kRF] = {};
    int64_t nsel = 0, B = 0;
    int C = 1;
    bool want_peers = false, want_cls = false, want_msgs = false;
};

namespace {

constexpr char kRlName[] = "relay report";      // (the scratch error text)
constexpr int kRlBlock = 256;                    // 4 waves, 256 consecutive peers
constexpr int64_t kRlFullWaves = 256;
constexpr int64_t kRlTargetWaves = 2048;

// The selected slot's row (k_select, report_common.h).
struct RlFill {
    using Row = RlMsg;
    __device__ static uint32_t fill(Row& r, const ReportView& v, int m, int64_t pub)
    {
        RlMsg x;
        fill_sel(x, v, m, pub);
        x.slot = (uint32_t)m;
        x._pad = 0;
        r = x;
        return x.topic;
    }
};
static_assert(RF_NSEL == 0, "k_select<RlFill, RF_TOPIC> writes the count and clears the flags before RF_TOPIC");

enum : int { PS_REACHED = 0, PS_ORPH, PS_LATMAX, PS_DEEP, PS_DELAY = 4, PS_CTO = 12, kPS = PS_CTO + GSIM_NET_CLASSES * GSIM_NET_CLASSES };

template <bool CLS>
__global__ __launch_bounds__(kRlBlock) void k_relay_push(RelayArgs a)
{
    __shared__ uint32_t s[kPS];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < kPS) s[tid] = 0;
    __syncthreads();
    const int b = (int)blockIdx.y;
    const RlMsg mm = a.sel[a.k0 + b];
    const int32_t t = (int32_t)mm.topic;
    const int64_t word = (a.rlo >> 6) + (int64_t)blockIdx.x * (kRlBlock / 64) + (tid >> 6);   // wave-uniform
    const int64_t p = word * 64 + lane;
    const bool active = p >= a.rlo && p < a.rhi;
    const bool wave_on = word * 64 < a.rhi;
    const uint64_t c = lane_cell(a.cells, mm, word, lane, wave_on, active);
    const uint32_t hi = (uint32_t)(c >> 32);
    const bool ok = !(hi & kClaim);                            // committed (unseen reads all ones, a claim has kClaim)
    const bool mine = ok && (uint32_t)p == mm.origin;
    bool other = ok && !mine;
    const uint32_t parent = (uint32_t)c & kPeerMask;
    const uint32_t mycls = CLS && active ? a.cls[p] : 0u;
    bool bad = false;
    if (other && (int64_t)parent >= a.n) { bad = true; other = false; }
    bool orphan = ok && !mine && (!other || hi < mm.pub);
    uint32_t delay = 0, sc = 0;
    bool timed = false;
    if (other) {
        atomicAdd(&a.cnt[(int64_t)b * a.n + parent], 1u);      // non-returning: one per first delivery
        if (CLS) {
            sc = a.cls[parent];
            atomicAdd(&a.cto[(int64_t)parent * a.C + mycls], 1ull);
        }
        if ((int64_t)parent >= a.rlo && (int64_t)parent < a.rhi) {   // (a ghost's cell is not its owner's)
            const int64_t pi = a.cells.at((int64_t)mm.base, t, parent);
            uint32_t phi = kClaim;
            if (pi >= 0 && pi - (int64_t)mm.base < (int64_t)mm.len) phi = (uint32_t)(a.cells.cell[pi] >> 32);
            if ((phi & kClaim) || phi >= hi) orphan = true;
            else if (!orphan) { delay = hi - phi; timed = true; }
        }
    }
    const uint32_t lat = ok && hi >= mm.pub ? hi - mm.pub : 0u;
    if (active) {
        uint16_t code = kDepNone;
        if (ok) code = mine ? (uint16_t)0 : orphan ? kDepOrphan : (uint16_t)(kDepPending | (lat < kDepLatMax ? lat : kDepLatMax));
        a.dep[(int64_t)b * a.n + p] = code;
    }
    const bool deep = ok && !mine && !orphan && lat >= kDepLatMax;

    // per wave, then per block, then one global atomic per non-zero entry
    const uint64_t b_ok = __ballot(ok), b_or = __ballot(orphan), b_deep = __ballot(deep), b_bad = __ballot(bad);
    const uint32_t wl = wave_max(lat);
    if (a.want_msgs) {
        const uint32_t bin = delay < 8 ? delay - 1 : 7;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint64_t m = __ballot(timed && bin == (uint32_t)k);
            if (lane == 0 && m) atomicAdd(&s[PS_DELAY + k], (uint32_t)__popcll(m));
        }
    }
    if (CLS) {
        const uint32_t key = sc * GSIM_NET_CLASSES + mycls;
        count_keys(s + PS_CTO, other, key, lane);               // the distinct (sender class, child class)
    } else {
        const uint64_t m = __ballot(other);
        if (lane == 0 && m) atomicAdd(&s[PS_CTO], (uint32_t)__popcll(m));
    }
    if (lane == 0) {
        if (b_ok) atomicAdd(&s[PS_REACHED], (uint32_t)__popcll(b_ok));
        if (b_or) atomicAdd(&s[PS_ORPH], (uint32_t)__popcll(b_or));
        if (wl) atomicMax(&s[PS_LATMAX], wl);
        if (b_deep) s[PS_DEEP] = 1u;
        if (b_bad) a.flags[RF_BAD] = 1u;
    }
    __syncthreads();
    if (tid >= kPS) return;
    const uint32_t v = s[tid];
    if (!v) return;
    uint32_t* mr = a.macc + (a.k0 + b) * kRM;
    if (tid == PS_REACHED) atomicAdd(&mr[RM_REACHED], v);
    else if (tid == PS_ORPH) {
        atomicAdd(&mr[RM_ORPHANS], v);
        atomicAdd(&a.flags[RF_ORPH], v);
    } else if (tid == PS_LATMAX) {
        atomicMax(&mr[RM_LATMAX], v);
        atomicMax(&a.flags[RF_BLAT], v);
    } else if (tid == PS_DEEP) a.flags[RF_DEEP] = 1u;
    else if (tid < PS_CTO) atomicAdd(&mr[RM_DELAY + (tid - PS_DELAY)], v);
    else if (a.acc && t < a.T) {
        const int key = tid - PS_CTO, scl = key / GSIM_NET_CLASSES, ccl = key % GSIM_NET_CLASSES;
        if (scl < a.C) atomicAdd(&a.acc[((int64_t)t * a.C + scl) * kRC + RC_CTO + ccl], (unsigned long long)v);
    }
}

template <bool CLS>
__global__ __launch_bounds__(kRlBlock) void k_relay_fold(RelayArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_acc[];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool classes = a.acc != nullptr;
    const int nacc = classes ? a.T * a.C * kRL : 0;
    for (int q = tid; q < nacc; q += kRlBlock) s_acc[q] = 0;
    __syncthreads();
    const int64_t word = (a.qlo >> 6) + (int64_t)blockIdx.x * (kRlBlock / 64) + (tid >> 6);   // wave-uniform
    const int64_t p = word * 64 + lane;
    const bool active = p >= a.qlo && p < a.qhi;
    const uint32_t mycls = CLS && active ? a.cls[p] : 0u;

    uint32_t nheld = 0, nrel = 0, maxc = 0;
    unsigned long long sumc = 0, ownc = 0;
    const int klo = (int)blockIdx.y * a.per;
    const int khi = klo + a.per < a.nb ? klo + a.per : a.nb;
    for (int b = klo; b < khi; ++b) {                          // block-uniform
        const RlMsg mm = a.sel[a.k0 + b];
        const int32_t t = (int32_t)mm.topic;
        uint32_t c = 0;
        uint16_t d = kDepNone;
        if (active) {
            c = a.cnt[(int64_t)b * a.n + p];
            d = a.dep[(int64_t)b * a.n + p];
        }
        const bool held = d != kDepNone;                       // (children without a cell of the peer's own: orphans)
        nheld += held;
        nrel += c > 0;
        sumc += c;
        if ((uint32_t)p == mm.origin) ownc += c;
        maxc = c > maxc ? c : maxc;
        if (a.want_msgs) {
            const uint64_t rel = __ballot(held && c > 0);
            if (__ballot(c > 0)) {
                const uint32_t wm = wave_max(c);
                const uint64_t top = __ballot(c == wm);
                if (lane == __builtin_ctzll(top)) {            // the wave's widest holder, the lowest id among equals
                    uint32_t* mr = a.macc + (a.k0 + b) * kRM;
                    if (rel) atomicAdd(&mr[RM_RELAYS], (uint32_t)__popcll(rel));
                    atomicMax(reinterpret_cast<unsigned long long*>(&mr[RM_MAXKEY]),
                              ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)p));
                }
            }
        }
        if (!classes || t >= a.T) continue;
        uint32_t* trow = s_acc + t * a.C * kRL;
        const uint32_t bin = c < GSIM_REPORT_BINS - 1 ? c : GSIM_REPORT_BINS - 1;
        const uint32_t key = mycls * GSIM_REPORT_BINS + bin;
        // (written out: through lead_keys the fold measured 1.2 % slower than before, outside the
        // spread of repeated runs)
        uint64_t todo = __ballot(held);
        while (todo) {                                         // wave-uniform: the distinct (class, fan-out bin) present
            const int lead = __builtin_ctzll(todo);
            const uint32_t kl = (uint32_t)__builtin_amdgcn_readlane((int)key, lead);
            const uint64_t same = __ballot(held && key == kl);
            if (lane == lead)
                atomicAdd(&trow[(kl / GSIM_REPORT_BINS) * kRL + RL_FAN + kl % GSIM_REPORT_BINS], (uint32_t)__popcll(same));
            todo &= ~same;
        }
        if (held && c >= GSIM_REPORT_BINS - 1) atomicMax(&trow[mycls * kRL + RL_MAX], c);   // the overflow bin alone needs the exact count
    }

    if (a.rows && p >= a.olo && p < a.ohi && (nheld || nrel)) {          // the parts and the batches meet on the zeroed row
        gsim_relay_row* row = a.rows + (p - a.olo);
        if (nheld) atomicAdd(&row->held, nheld);
        if (nrel) atomicAdd(&row->relayed_msgs, nrel);
        if (maxc) atomicMax(&row->max_children, maxc);
        if (sumc) atomicAdd(reinterpret_cast<unsigned long long*>(&row->children), sumc);
        if (ownc) atomicAdd(reinterpret_cast<unsigned long long*>(&row->own_children), ownc);
    }

    __syncthreads();
    for (int q = tid; q < nacc; q += kRlBlock) {               // one global atomic per non-zero entry
        const int k = q % kRL;
        uint32_t v = s_acc[q];
        unsigned long long* g = a.acc + (size_t)(q / kRL) * kRC;
        if (k == RL_MAX) {
            const uint32_t* fan = &s_acc[q - k + RL_FAN];       // the exact bins carry their own count
            for (int bb = GSIM_REPORT_BINS - 2; bb > 0 && !v; --bb) v = fan[bb] ? (uint32_t)bb : 0u;
            if (v) atomicMax(&g[RC_MAX], (unsigned long long)v);
        } else if (v) atomicAdd(&g[RC_FAN + k], (unsigned long long)v);
    }
}

// peers of each class announcing each topic, over [qlo, qhi)
template <bool CLS>
__global__ __launch_bounds__(kRlBlock) void k_relay_peers(RelayArgs a, const uint64_t* subs)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (a.qlo >> 6) * 64 + (int64_t)blockIdx.x * kRlBlock + threadIdx.x;
    const bool active = p >= a.qlo && p < a.qhi;
    const uint64_t sub = active ? subs[p] : 0ull;
    const uint32_t mycls = CLS && active ? a.cls[p] : 0u;
    for (int32_t t = 0; t < a.T; ++t) {
        // the classes present
        lead_keys((sub >> t) & 1ull, mycls, lane, [&](uint32_t cl, uint32_t cnt) {
            atomicAdd(&a.acc[((int64_t)t * a.C + cl) * kRC + RC_PEERS], (unsigned long long)cnt);
        });
    }
}

// pass `level`: the cells first seen `level` rounds after the publication
__global__ __launch_bounds__(kRlBlock) void k_relay_depth(RelayArgs a)
{
    const int lane = threadIdx.x & 63;
    const int b = (int)blockIdx.y;
    const int64_t word = (a.rlo >> 6) + (int64_t)blockIdx.x * (kRlBlock / 64) + (threadIdx.x >> 6);
    const int64_t p = word * 64 + lane;
    const bool active = p >= a.rlo && p < a.rhi;
    const uint16_t want = (uint16_t)(kDepPending | (uint32_t)a.level);
    const bool hit = active && a.dep[(int64_t)b * a.n + p] == want;
    if (!__ballot(hit)) return;                                // wave-uniform
    const RlMsg mm = a.sel[a.k0 + b];
    const uint64_t c = lane_cell(a.cells, mm, word, lane, word * 64 < a.rhi, hit);
    if (!hit) return;
    const uint32_t parent = (uint32_t)c & kPeerMask;           // (checked by the push: a local peer with an earlier cell)
    const uint16_t pv = a.dep[(int64_t)b * a.n + parent];
    const uint32_t pd = (pv & (kDepOrphan | kDepPending)) ? 0u : pv;
    a.dep[(int64_t)b * a.n + p] = (uint16_t)(pd + 1 < kDepLatMax ? pd + 1 : kDepLatMax - 1);
}

__global__ __launch_bounds__(kRlBlock) void k_relay_bins(RelayArgs a)
{
    __shared__ uint32_t s[GSIM_REPORT_BINS + 1];
    const int tid = threadIdx.x;
    if (tid <= GSIM_REPORT_BINS) s[tid] = 0;
    __syncthreads();
    const int b = (int)blockIdx.y;
    const int64_t p = (a.rlo >> 6) * 64 + (int64_t)blockIdx.x * kRlBlock + tid;
    if (p >= a.rlo && p < a.rhi) {
        const uint32_t d = a.dep[(int64_t)b * a.n + p];
        if (d < kDepPending) {
            atomicAdd(&s[d < GSIM_REPORT_BINS - 1 ? d : GSIM_REPORT_BINS - 1], 1u);
            if (d >= GSIM_REPORT_BINS - 1) atomicMax(&s[GSIM_REPORT_BINS], d);
        }
    }
    __syncthreads();
    if (tid > GSIM_REPORT_BINS) return;
    uint32_t v = s[tid];
    uint32_t* mr = a.macc + (a.k0 + b) * kRM;
    if (tid == GSIM_REPORT_BINS) {
        for (int k = GSIM_REPORT_BINS - 2; k > 0 && !v; --k) v = s[k] ? (uint32_t)k : 0u;
        if (v) atomicMax(&mr[RM_DEPTHMAX], v);
    } else if (v) atomicAdd(&mr[RM_DEPTH + tid], v);
}

// cnt[x] += inc[x]: the ghosts' counts of the other shards
__global__ __launch_bounds__(256) void k_relay_add(uint32_t* cnt, const uint32_t* inc, int64_t n)
{
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (int64_t)gridDim.x * 256) {
        const uint32_t v = inc[x];
        if (v) cnt[x] += v;
    }
}

inline uint32_t peer_blocks(int64_t lo, int64_t hi)
{
    const int64_t words = ((hi + 63) >> 6) - (lo >> 6);
    return (uint32_t)std::max<int64_t>(1, (words + kRlBlock / 64 - 1) / (kRlBlock / 64));
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void relayreport_release(gsim_handle* h)
{
    if (!h->rl) return;
    RelayReport* r = h->rl;
    free_all({r->d_sel, r->d_flags, r->d_acc, r->d_macc, r->d_cnt, r->d_dep, r->d_inc, r->d_cto, r->d_rows});
    delete r;
    h->rl = nullptr;
}

int64_t relay_budget(const gsim_handle* h) { return h->rl && h->rl->budget > 0 ? h->rl->budget : kRlBudget; }

// Commits the pending claims, selects, reads the counts: *nsel and *nc are set.
int relay_begin(gsim_handle* h, int64_t round_lo, int64_t round_hi, int64_t* nsel, int64_t* nc)
{
    const uint8_t* d_cls = nullptr;
    const int C = netreport_classes(h, &d_cls);
    *nc = (int64_t)h->t * C;
    *nsel = 0;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    ReportView v{};
    if (!deliver_report_view(h, &v)) { h->err = "gsim_msgs_init not called"; return GSIM_ESTATE; }
    int rc = deliver_flush(h);                     // the last round's claims become first-seen rounds
    if (rc) return rc;
    if (!h->rl) h->rl = new RelayReport;
    RelayReport* r = h->rl;
    const int64_t slots = std::max<int32_t>(v.ring, 1);
    rc = grow(h, kRlName, &r->d_sel, &r->sel_cap, slots);
    if (!rc) rc = grow(h, kRlName, &r->d_macc, &r->macc_cap, slots * kRM);
    if (!rc) rc = alloc_once(h, kRlName, &r->d_flags, kRF);
    if (!rc) rc = alloc_once(h, kRlName, &r->d_acc, (int64_t)kRlAcc);
    if (rc) return rc;
    hipLaunchKernelGGL((k_select<RlFill, RF_TOPIC>), dim3(1), dim3(kSelBlock), 0, h->stream, v, round_lo, round_hi, r->d_sel,
                       r->d_flags);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(r->cs, r->d_flags, sizeof(r->cs), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    r->v = v;
    r->C = C;
    r->nsel = r->cs[RF_NSEL];
    *nsel = r->nsel;
    RelayArgs a{};
    a.cells = v.cells; a.sel = r->d_sel; a.cls = C > 1 ? d_cls : nullptr;
    a.T = h->t; a.C = C; a.n = h->n; a.rlo = v.rlo; a.rhi = v.rhi;
    a.macc = r->d_macc; a.flags = r->d_flags;
    r->a = a;
    return GSIM_OK;
}

// Scratch for batches of B slots and the call's zeroed accumulators.  [olo, ohi):
// the owned local peers whose rows are wanted (empty: none); staged: a shard
// (the other shards' counts are added between the push and the fold).
int relay_prepare(gsim_handle* h, int64_t B, int64_t olo, int64_t ohi, bool want_cls, bool want_msgs, bool staged)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    RelayArgs& a = r->a;
    r->B = std::max<int64_t>(1, B);
    r->want_peers = ohi > olo;
    r->want_cls = want_cls;
    r->want_msgs = want_msgs;
    const int64_t ent = r->B * a.n;
    int rc = grow(h, kRlName, &r->d_cnt, &r->slots_cap, ent);
    if (!rc) rc = grow(h, kRlName, &r->d_dep, &r->dep_cap, ent);
    if (!rc && staged) rc = grow(h, kRlName, &r->d_inc, &r->inc_cap, ent);
    if (!rc && a.cls) rc = grow(h, kRlName, &r->d_cto, &r->cto_cap, a.n * a.C);
    if (!rc && r->want_peers) rc = grow(h, kRlName, &r->d_rows, &r->rows_cap, ohi - olo);
    if (rc) return rc;
    a.cnt = r->d_cnt; a.dep = r->d_dep;
    a.cto = a.cls ? r->d_cto : nullptr;
    a.acc = want_cls && (int64_t)a.T * a.C > 0 ? r->d_acc : nullptr;
    a.rows = r->want_peers ? r->d_rows : nullptr;
    a.olo = olo; a.ohi = ohi;
    // the class and message rows cover every owned peer; without them the range's owned peers are folded
    a.qlo = want_cls || want_msgs ? a.rlo : olo; a.qhi = want_cls || want_msgs ? a.rhi : ohi;
    a.want_msgs = want_msgs ? 1 : 0;
    hipError_t e = hipMemsetAsync(r->d_macc, 0, sizeof(uint32_t) * kRM * (size_t)std::max<int64_t>(r->nsel, 1), h->stream);
    if (e == hipSuccess && a.acc) e = hipMemsetAsync(r->d_acc, 0, sizeof(unsigned long long) * (size_t)a.T * a.C * kRC, h->stream);
    if (e == hipSuccess && a.cto) e = hipMemsetAsync(r->d_cto, 0, sizeof(unsigned long long) * (size_t)(a.n * a.C), h->stream);
    if (e == hipSuccess && a.rows) e = hipMemsetAsync(r->d_rows, 0, sizeof(gsim_relay_row) * (size_t)(ohi - olo), h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    if (a.acc && a.qhi > a.qlo) {
        const uint32_t gx = (uint32_t)((((a.qhi + 63) >> 6) * 64 - (a.qlo >> 6) * 64 + kRlBlock - 1) / kRlBlock);
        if (a.cls) hipLaunchKernelGGL(k_relay_peers<true>, dim3(gx), dim3(kRlBlock), 0, h->stream, a, r->v.sub);
        else hipLaunchKernelGGL(k_relay_peers<false>, dim3(gx), dim3(kRlBlock), 0, h->stream, a, r->v.sub);
    }
    r->last[0] = r->B; r->last[1] = 0; r->last[2] = 0; r->last[3] = r->nsel;
    return hip_check(h, hipGetLastError(), "gsim_relay_report");
}

int relay_push(gsim_handle* h, int64_t k0, int32_t nb)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    RelayArgs a = r->a;
    a.k0 = k0; a.nb = nb;
    hipError_t e = hipMemsetAsync(r->d_cnt, 0, sizeof(uint32_t) * (size_t)(nb * a.n), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_flags + RF_BLAT, 0, sizeof(uint32_t) * 2, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    r->last[1] += 1;
    if (a.rhi <= a.rlo) return GSIM_OK;
    const dim3 grid(peer_blocks(a.rlo, a.rhi), (uint32_t)nb);
    if (a.cls) hipLaunchKernelGGL(k_relay_push<true>, grid, dim3(kRlBlock), 0, h->stream, a);
    else hipLaunchKernelGGL(k_relay_push<false>, grid, dim3(kRlBlock), 0, h->stream, a);
    return hip_check(h, hipGetLastError(), "gsim_relay_report");
}

// the batch's counts of every local peer, [nb][n]; synchronizes
int relay_read_counts(gsim_handle* h, int32_t nb, uint32_t* host)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    return hip_check(h, stream_copy(h, host, r->d_cnt, sizeof(uint32_t) * (size_t)(nb * r->a.n), hipMemcpyDeviceToHost),
                     "gsim_relay_report");
}

// adds inc[nb][n] (a host array) to the batch's counts; synchronizes
int relay_add_counts(gsim_handle* h, int32_t nb, const uint32_t* inc)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    const int64_t ent = nb * r->a.n;
    hipError_t e = stream_copy(h, r->d_inc, inc, sizeof(uint32_t) * (size_t)ent, hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    hipLaunchKernelGGL(k_relay_add, dim3((uint32_t)std::min<int64_t>((ent + 255) / 256, 4096)), dim3(256), 0, h->stream,
                       r->d_cnt, r->d_inc, ent);
    return hip_check(h, hipGetLastError(), "gsim_relay_report");
}

int relay_fold(gsim_handle* h, int64_t k0, int32_t nb)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    RelayArgs a = r->a;
    a.k0 = k0; a.nb = nb;
    if (a.qhi <= a.qlo || (!a.rows && !a.acc && !a.want_msgs)) return GSIM_OK;
    const int64_t waves = ((a.qhi + 63) >> 6) - (a.qlo >> 6);
    int64_t parts = 1;
    if (waves < kRlFullWaves) parts = std::max<int64_t>(1, std::min<int64_t>((kRlTargetWaves + waves - 1) / waves, nb));
    a.per = (int32_t)((nb + parts - 1) / parts);
    parts = (nb + a.per - 1) / a.per;
    const dim3 grid(peer_blocks(a.qlo, a.qhi), (uint32_t)parts);
    const size_t lds = a.acc ? sizeof(uint32_t) * (size_t)a.T * a.C * kRL : 0;
    if (a.cls) hipLaunchKernelGGL(k_relay_fold<true>, grid, dim3(kRlBlock), lds, h->stream, a);
    else hipLaunchKernelGGL(k_relay_fold<false>, grid, dim3(kRlBlock), lds, h->stream, a);
    return hip_check(h, hipGetLastError(), "gsim_relay_report");
}

// the depth passes of the batch and its depth histograms (single engine)
int relay_depth(gsim_handle* h, int64_t k0, int32_t nb)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    RelayArgs a = r->a;
    a.k0 = k0; a.nb = nb;
    if (a.rhi <= a.rlo) return GSIM_OK;
    uint32_t bl[2] = {0, 0};                                   // the batch's largest latency (and RF_BPAD)
    hipError_t e = stream_copy(h, bl, r->d_flags + RF_BLAT, sizeof bl, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    const int32_t passes = (int32_t)std::min<uint32_t>(bl[0], kDepLatMax - 1);
    const dim3 grid(peer_blocks(a.rlo, a.rhi), (uint32_t)nb);
    for (int32_t L = 1; L <= passes; ++L) {
        a.level = L;
        hipLaunchKernelGGL(k_relay_depth, grid, dim3(kRlBlock), 0, h->stream, a);
    }
    r->last[2] += passes;
    const dim3 g2((uint32_t)((((a.rhi + 63) >> 6) * 64 - (a.rlo >> 6) * 64 + kRlBlock - 1) / kRlBlock), (uint32_t)nb);
    hipLaunchKernelGGL(k_relay_bins, g2, dim3(kRlBlock), 0, h->stream, a);
    return hip_check(h, hipGetLastError(), "gsim_relay_report");
}

// Reads the results; synchronizes.  peers: rows of the local peers [olo, ohi) of
// relay_prepare (children_to filled for the owned peers); cto: [n][C] the
// children by class of every local peer, ghosts included (a group adds the
// ghosts' to their owners' rows), or nullptr; classes: T * C rows; msgs: nsel rows.
int relay_finish(gsim_handle* h, struct gsim_relay_row* peers, uint64_t* cto, struct gsim_relay_class_row* classes,
                 struct gsim_relay_msg_row* msgs)
{
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    RelayReport* r = h->rl;
    const RelayArgs& a = r->a;
    const int64_t nc = (int64_t)a.T * a.C, np = a.ohi - a.olo;
    std::vector<unsigned long long> acc(classes ? (size_t)nc * kRC : 0);
    std::vector<uint32_t> macc(msgs ? (size_t)r->nsel * kRM : 0);
    std::vector<RlMsg> sel(msgs ? (size_t)r->nsel : 0);
    std::vector<unsigned long long> lcto;
    uint32_t fl[kRF] = {};
    hipError_t e = hipMemcpyAsync(fl, r->d_flags, sizeof fl, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && peers && np > 0)
        e = hipMemcpyAsync(peers, r->d_rows, sizeof(gsim_relay_row) * (size_t)np, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && !acc.empty())
        e = hipMemcpyAsync(acc.data(), r->d_acc, sizeof(unsigned long long) * acc.size(), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && a.cto && (cto || (peers && np > 0))) {
        if (cto) e = hipMemcpyAsync(cto, r->d_cto, sizeof(uint64_t) * (size_t)(a.n * a.C), hipMemcpyDeviceToHost, h->stream);
        else {
            lcto.resize((size_t)(np * a.C));
            e = hipMemcpyAsync(lcto.data(), r->d_cto + a.olo * a.C, sizeof(uint64_t) * lcto.size(), hipMemcpyDeviceToHost,
                               h->stream);
        }
    }
    if (e == hipSuccess && !macc.empty()) {
        e = hipMemcpyAsync(macc.data(), r->d_macc, sizeof(uint32_t) * macc.size(), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(sel.data(), r->d_sel, sizeof(RlMsg) * sel.size(), hipMemcpyDeviceToHost, h->stream);
    }
    std::vector<uint64_t> mid;
    std::vector<uint8_t> minv, mlat;
    if (e == hipSuccess && msgs && r->nsel) {
        const size_t ring = (size_t)r->v.ring;
        mid.resize(ring); minv.resize(ring); mlat.assign(ring, 0);
        e = hipMemcpyAsync(mid.data(), r->v.mid, sizeof(uint64_t) * ring, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(minv.data(), r->v.minv, ring, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && r->v.mlat) e = hipMemcpyAsync(mlat.data(), r->v.mlat, ring, hipMemcpyDeviceToHost, h->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_relay_report");
    if (peers)
        for (int64_t k = 0; k < np; ++k) {
            if (!a.cto) { peers[k].children_to[0] = peers[k].children; continue; }
            const uint64_t* src = cto ? cto + (a.olo + k) * a.C : (const uint64_t*)lcto.data() + k * a.C;
            for (int c = 0; c < a.C; ++c) peers[k].children_to[c] = src[c];
        }
    if (classes)
        for (int64_t q = 0; q < nc; ++q) {
            const unsigned long long* c = acc.data() + (size_t)q * kRC;
            gsim_relay_class_row x{};
            x.topic = (uint32_t)(q / a.C);
            x.cls = (uint32_t)(q % a.C);
            x.peers = (uint32_t)c[RC_PEERS];
            x.messages = r->cs[RF_TOPIC + x.topic];
            for (int k = 0; k < GSIM_REPORT_BINS; ++k) { x.fanout[k] = c[RC_FAN + k]; x.held += c[RC_FAN + k]; }
            x.relayed = x.held - x.fanout[0];
            x.max_children = (uint32_t)c[RC_MAX];
            for (int k = 0; k < GSIM_NET_CLASSES; ++k) { x.children_to[k] = c[RC_CTO + k]; x.children += c[RC_CTO + k]; }
            classes[q] = x;
        }
    if (msgs) {
        for (int64_t k = 0; k < r->nsel; ++k) {
            const uint32_t* m = macc.data() + (size_t)k * kRM;
            const RlMsg& s = sel[(size_t)k];
            gsim_relay_msg_row x{};
            x.id = mid[s.slot];
            x.pub_round = (int64_t)s.pub;
            x.slot = s.slot; x.topic = s.topic; x.origin = s.origin;
            x.reached = m[RM_REACHED];
            x.relays = m[RM_RELAYS];
            unsigned long long key;
            std::memcpy(&key, &m[RM_MAXKEY], sizeof key);
            x.max_children = (uint32_t)(key >> 32);
            x.max_children_peer = x.max_children ? 0xFFFFFFFFu - (uint32_t)key : 0u;
            x.depth_max = m[RM_DEPTHMAX];
            x.orphans = m[RM_ORPHANS];
            x.verdict = minv[s.slot];
            x.vdelay = mlat[s.slot];
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) x.depth_hist[q] = m[RM_DEPTH + q];
            for (int q = 0; q < 8; ++q) x.delay_hist[q] = m[RM_DELAY + q];
            msgs[k] = x;
        }
        // the device compacts in slot order: a stable sort by round gives (pub_round, slot)
        std::stable_sort(msgs, msgs + r->nsel, [](const gsim_relay_msg_row& x, const gsim_relay_msg_row& y) {
            return x.pub_round < y.pub_round;
        });
    }
    if (fl[RF_BAD]) {
        h->err = "gsim_relay_report: a committed cell of an owned peer names a first sender that is no local peer";
        return GSIM_ESTATE;
    }
    if (msgs && fl[RF_DEEP]) {
        h->err = "gsim_relay_report: a latency of 16383 rounds or more (the depth passes cannot code it)";
        return GSIM_ERANGE;
    }
    if (fl[RF_ORPH]) {
        h->err = "gsim_relay_report: a first sender holds no earlier committed cell of the message (orphans counted)";
        return GSIM_ESTATE;
    }
    return GSIM_OK;
}

extern "C" {

int gsim_relay_report(gsim_handle* h, int64_t round_lo, int64_t round_hi, int64_t peer_lo, int64_t peer_hi,
                      struct gsim_relay_row* peers, struct gsim_relay_class_row* classes, int64_t class_cap,
                      int64_t* n_classes, struct gsim_relay_msg_row* msgs, int64_t msg_cap, int64_t* n_msgs)
{
    if (!h || !n_classes || !n_msgs || class_cap < 0 || msg_cap < 0) return GSIM_EINVAL;
    *n_classes = 0;
    *n_msgs = 0;
    int64_t nsel = 0, nc = 0;
    int rc = relay_begin(h, round_lo, round_hi, &nsel, &nc);
    *n_classes = nc;
    *n_msgs = nsel;
    if (rc) return rc;
    if (peer_lo < 0 || peer_lo > peer_hi || peer_hi > h->n) {
        h->err = "gsim_relay_report: the peer range must satisfy 0 <= peer_lo <= peer_hi <= N";
        return GSIM_EINVAL;
    }
    if (h->sh && msgs && msg_cap > 0) {
        h->err = "gsim_relay_report: message rows are not offered on a shard";
        return GSIM_ESTATE;
    }
    RelayReport* r = h->rl;
    const bool want_cls = classes && class_cap > 0, want_msgs = msgs && msg_cap > 0;
    const bool want_peers = peers && peer_hi > peer_lo;
    if (want_cls && class_cap < nc) { h->err = "gsim_relay_report: class row buffer too small"; return GSIM_ERANGE; }
    if (want_msgs && msg_cap < nsel) { h->err = "gsim_relay_report: message row buffer too small"; return GSIM_ERANGE; }
    if (!want_cls && !want_msgs && !want_peers) return deliver_check_errors(h);
    const int64_t olo = std::min<int64_t>(std::max<int64_t>(peer_lo, r->v.rlo), peer_hi);
    const int64_t ohi = std::max<int64_t>(olo, std::min<int64_t>(peer_hi, r->v.rhi));
    const int64_t B = std::min<int64_t>(std::max<int64_t>(relay_budget(h) / (6 * std::max<int64_t>(h->n, 1)), 1),
                                        std::max<int64_t>(nsel, 1));
    rc = relay_prepare(h, B, want_peers ? olo : 0, want_peers ? ohi : 0, want_cls, want_msgs, false);
    for (int64_t k0 = 0; !rc && k0 < nsel; k0 += B) {
        const int32_t nb = (int32_t)std::min<int64_t>(B, nsel - k0);
        rc = relay_push(h, k0, nb);
        if (!rc) rc = relay_fold(h, k0, nb);
        if (!rc && want_msgs) rc = relay_depth(h, k0, nb);
    }
    if (rc) return rc;
    if (want_peers) {                              // the range's peers this engine does not own: empty rows
        std::memset(peers, 0, sizeof(gsim_relay_row) * (size_t)(olo - peer_lo));
        std::memset(peers + (ohi - peer_lo), 0, sizeof(gsim_relay_row) * (size_t)(peer_hi - ohi));
    }
    rc = relay_finish(h, want_peers ? peers + (olo - peer_lo) : nullptr, nullptr, want_cls ? classes : nullptr,
                      want_msgs ? msgs : nullptr);
    const int rc2 = deliver_check_errors(h);
    return rc ? rc : rc2;
}

int gsim_relay_report_budget(gsim_handle* h, int64_t bytes)
{
    if (!h || bytes < 0) return GSIM_EINVAL;
    if (!h->rl) h->rl = new RelayReport;
    h->rl->budget = bytes;
    return GSIM_OK;
}

int gsim_relay_report_launch(gsim_handle* h, int64_t* out4)
{
    if (!h || !out4) return GSIM_EINVAL;
    for (int k = 0; k < 4; ++k) out4[k] = h->rl ? h->rl->last[k] : 0;
    return GSIM_OK;
}

}  // extern "C"
