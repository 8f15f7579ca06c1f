// Router state (include/gsim.h gsim_router_state_*): the seen cache
// (timecache/, pubsub.go:986-995, 1150-1162) and the gossip tracer's promises
// (gossip_tracer.go:48-200) of externally driven routers, one of each per
// observer, as the CPU oracle restates them (orc_tcache_*, orc_gtracer_*).
//
// A batch runs in the score tracer's three stages (scoretracer.hip, DESIGN.md
// §4.11 and §4.13):
//   sort     a stable radix sort of (observer, index);
//   resolve  one thread per event: a PROMISE's edge (a binary search of the
//            observer's row), every check of the batch, the segment heads;
//   apply    one lane per observer segment walks its events in array order.
//
// Seen cache: one open-addressing table keyed (observer, id).  A slot is
// claimed by a device-scope CAS on its observer word and from then on read and
// written only by that observer's lane.  Nothing is ever deleted in place: the
// sweep rebuilds into a second table (as k_tracer_gc), so no tombstones exist
// and a probe may stop at the first empty slot.
//
// Promises: DRec / PeerEnt's shape.  A table keyed (observer, id) whose record
// heads a list of (edge, expire) through a bump-allocated pool; the edge is the
// observer's CSR edge to the promising peer, so edge order is (observer, peer)
// order.  fulfillPromise empties its record's list; broken and throttle are
// whole-table passes that rebuild table and pool from the surviving promises.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>

#include "gsim_internal.h"

namespace gsim {

constexpr uint32_t kSlotEmpty = 0xFFFFFFFFu;   // an unclaimed table slot's observer word
constexpr uint32_t kNoEnt = 0xFFFFFFFFu;       // end of a promise list / no slot
// why an event or a pair fails its call
enum : uint32_t { kRsBadKind = 1, kRsBadObserver, kRsBadEdge, kRsBadTime, kRsBadRange };
// d_cnt words: the live counters, then the per-call ones (cleared before each use)
enum : int { kRsSeenLive = 0, kRsPromLive, kRsPromRecs, kRsPromPool, kRsErr, kRsSeg, kRsFulfilled, kRsDropped,
             kRsWords = 8 };

struct SeenEnt {          // 24 bytes
    uint64_t mid;
    int64_t expiry;
    uint32_t obs;         // the claim word: kSlotEmpty or the owning observer
    uint32_t _pad;
};

struct PromRec {          // 24 bytes: promises[mid] of one observer
    uint64_t mid;
    uint32_t obs;         // the claim word
    uint32_t head;        // list of the peers' promises (pool index), kNoEnt: none
    uint32_t n;
    uint32_t _pad;
};

struct PromEnt {          // 16 bytes: promises[mid][peer] = expire
    int64_t expire;
    uint32_t edge;        // the observer's edge to the peer
    uint32_t next;
};

struct RouterState {
    int64_t seen_cap = 0, promises_cap = 0, ttl = 0, followup = 0;
    int32_t strategy = 0;
    uint32_t seen_slots = 0, prom_slots = 0;   // powers of two >= 2 cap
    SeenEnt *d_seen = nullptr, *d_seen2 = nullptr;      // the second of each: the rebuilds' other side,
    PromRec *d_prec = nullptr, *d_prec2 = nullptr;      // allocated at the first rebuild, swapped by each
    PromEnt *d_pool = nullptr, *d_pool2 = nullptr;
    uint32_t* d_cnt = nullptr;                 // [2][kRsWords]: the live counters, a rebuild's new ones
    unsigned long long* d_bad = nullptr;       // first offending index << 8 | why
    int64_t* d_last = nullptr;                 // [N] each observer's last router event time
    // host mirrors of the live counters; totals since config
    int64_t seen_live = 0, prom_live = 0, prom_recs = 0, prom_pool = 0;
    int64_t applied = 0, swept = 0, fulfilled = 0, broken = 0;
    // batch scratch, grow-only
    int64_t cap_ev = 0;
    gsim_router_event* d_ev = nullptr;
    uint32_t *d_key = nullptr, *d_key2 = nullptr, *d_idx = nullptr, *d_idx2 = nullptr, *d_edge = nullptr,
             *d_seg = nullptr;
    uint8_t* d_res = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
    // broken's scratch (allocated at the first call, sized by promises_cap)
    uint32_t *d_bkey = nullptr, *d_bkey2 = nullptr, *d_buniq = nullptr, *d_bcount = nullptr, *d_bruns = nullptr;
    gsim_broken_row* d_rows = nullptr;
    void* d_btmp = nullptr;
    size_t btmp_bytes = 0;
    // throttle's scratch: the pairs, their edges, one flag per edge (allocated at the first call)
    int64_t cap_pairs = 0;
    uint32_t *d_pairs = nullptr, *d_pedge = nullptr;
    uint8_t* d_thr = nullptr;
};

struct RsArgs {
    const gsim_router_event* ev;
    const uint32_t *key, *idx;        // sorted: observer (clamped to N) and event index of each position
    uint32_t *edge, *seg;             // [n] a PROMISE's edge (by index); first position of each segment
    uint8_t* res;                     // [n] the answers (by index)
    int64_t n, N;
    const uint32_t *row_ptr, *col;
    SeenEnt* seen;
    uint32_t smask;                   // seen_slots - 1
    PromRec* prec;
    uint32_t pmask;                   // prom_slots - 1
    PromEnt* pool;
    uint32_t pool_cap;
    uint32_t* cnt;
    unsigned long long* bad;
    int64_t* last;
    int64_t ttl, followup;
    int32_t strategy;
};

namespace {

// the observer's edge to `peer` (rows are sorted), kNoEnt: no connection
__device__ __forceinline__ uint32_t rs_find_edge(const uint32_t* row_ptr, const uint32_t* col, uint32_t o, uint32_t peer)
{
    uint32_t lo = row_ptr[o], hi = row_ptr[o + 1];
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (col[mid] < peer) lo = mid + 1; else hi = mid;
    }
    return lo < end && col[lo] == peer ? lo : kNoEnt;
}

__global__ __launch_bounds__(256) void k_rs_keys(const gsim_router_event* ev, int64_t n, uint32_t N, uint32_t* key,
                                                 uint32_t* idx)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t o = ev[k].observer;
    key[k] = o < N ? o : N;           // every observer out of range sorts last (and fails the batch)
    idx[k] = (uint32_t)k;
}

// One thread per sorted position: the event's checks, a PROMISE's edge, its segment.
__global__ __launch_bounds__(256) void k_rs_resolve(RsArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t k = a.idx[p], o = a.key[p];
    const gsim_router_event x = a.ev[k];
    const bool head = p == 0 || a.key[p - 1] != o;
    uint32_t why = 0, e = kNoEnt;
    if (x.kind > GSIM_RS_FULFILL) why = kRsBadKind;
    else if ((int64_t)x.observer >= a.N) why = kRsBadObserver;
    else if (x.kind == GSIM_RS_PROMISE) {
        if ((int64_t)x.peer < a.N) e = rs_find_edge(a.row_ptr, a.col, o, x.peer);
        if (e == kNoEnt) why = kRsBadEdge;
    }
    // an expiry is now + ttl or now + followup (both >= 0): it must fit an int64
    if (!why && x.now_ns > INT64_MAX - (a.ttl > a.followup ? a.ttl : a.followup)) why = kRsBadRange;
    if (!why) {
        // non-decreasing per observer: against the event before it in the
        // segment, the segment's first against the observer's last batch
        const int64_t prev = head ? a.last[o] : a.ev[a.idx[p - 1]].now_ns;
        if (x.now_ns < prev) why = kRsBadTime;
    }
    a.edge[k] = e;
    if (why) atomicMin(a.bad, ((unsigned long long)k << 8) | why);
    if (head && (int64_t)o < a.N) a.seg[atomicAdd(a.cnt + kRsSeg, 1u)] = (uint32_t)p;
}

__device__ __forceinline__ uint32_t rs_hash(uint32_t o, uint64_t mid)
{
    uint64_t x = mid ^ ((uint64_t)o * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return (uint32_t)x;
}

// The slot of (o, mid) in an open-addressing table (SeenEnt or PromRec).
//   Find && Claim   the observer's own slot of the key (found), else an empty
//                   slot claimed for it (Add, AddPromise);
//   Find only       the observer's own slot or kNoEnt (Has, fulfillPromise): a
//                   table without tombstones has no gap before a key it holds;
//   Claim only      a rebuild: every key is new and an observer's entries are
//                   moved by many threads, so no slot's other fields are read.
// kNoEnt with Claim: the table is full (the capacity checks keep half of it
// empty: not reached).
template <bool Find, bool Claim, class R>
__device__ uint32_t rs_slot(R* tab, uint32_t mask, uint32_t o, uint64_t mid, bool* found)
{
    uint32_t h = rs_hash(o, mid) & mask;
    *found = false;
    for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        uint32_t w = __hip_atomic_load(&tab[h].obs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == kSlotEmpty) {
            if (!Claim) return kNoEnt;
            w = atomicCAS(&tab[h].obs, kSlotEmpty, o);
            if (w == kSlotEmpty) return h;
        }
        // another observer's slot never becomes this one's; this observer's
        // slots are written by this lane only
        if (Find && w == o && tab[h].mid == mid) { *found = true; return h; }
    }
    return kNoEnt;
}

// first_seen_cache.go:47-56 / last_seen_cache.go:38-45
__device__ uint8_t rs_seen_add(const RsArgs& a, uint32_t o, const gsim_router_event& x)
{
    bool found;
    const uint32_t h = rs_slot<true, true>(a.seen, a.smask, o, x.mid, &found);
    if (h == kNoEnt) { atomicOr(a.cnt + kRsErr, 1u); return 0; }
    SeenEnt& s = a.seen[h];
    if (found) {
        if (a.strategy == 1) s.expiry = x.now_ns + a.ttl;
        return 0;
    }
    s.mid = x.mid;
    s.expiry = x.now_ns + a.ttl;
    atomicAdd(a.cnt + kRsSeenLive, 1u);
    return 1;
}

// first_seen_cache.go:37-45 / last_seen_cache.go:47-58
__device__ uint8_t rs_seen_has(const RsArgs& a, uint32_t o, const gsim_router_event& x)
{
    bool found;
    const uint32_t h = rs_slot<true, false>(a.seen, a.smask, o, x.mid, &found);
    if (!found) return 0;
    if (a.strategy == 1) a.seen[h].expiry = x.now_ns + a.ttl;
    return 1;
}

// gossip_tracer.go:48-77 with the id already picked
__device__ uint8_t rs_promise(const RsArgs& a, uint32_t o, uint32_t e, const gsim_router_event& x)
{
    bool found;
    const uint32_t h = rs_slot<true, true>(a.prec, a.pmask, o, x.mid, &found);
    if (h == kNoEnt) { atomicOr(a.cnt + kRsErr, 2u); return 0; }
    PromRec& r = a.prec[h];
    if (!found) {
        r.mid = x.mid;
        r.head = kNoEnt;
        r.n = 0;
        atomicAdd(a.cnt + kRsPromRecs, 1u);
    }
    uint32_t k = r.head;
    for (uint32_t q = 0; q < r.n && k != kNoEnt; ++q) {
        const PromEnt en = a.pool[k];
        if (en.edge == e) return 0;               // promised already: the expiry stays
        k = en.next;
    }
    k = atomicAdd(a.cnt + kRsPromPool, 1u);
    if (k >= a.pool_cap) { atomicOr(a.cnt + kRsErr, 4u); return 0; }   // (the capacity check: not reached)
    a.pool[k] = PromEnt{x.now_ns + a.followup, e, r.head};
    r.head = k;
    r.n += 1;
    atomicAdd(a.cnt + kRsPromLive, 1u);
    return 1;
}

// gossip_tracer.go:119-141: delete(promises, mid); the entries are reclaimed by the next rebuild
__device__ uint8_t rs_fulfill(const RsArgs& a, uint32_t o, const gsim_router_event& x)
{
    bool found;
    const uint32_t h = rs_slot<true, false>(a.prec, a.pmask, o, x.mid, &found);
    if (!found) return 0;
    PromRec& r = a.prec[h];
    const uint32_t c = r.n;
    if (!c) return 0;
    atomicAdd(a.cnt + kRsFulfilled, c);
    atomicSub(a.cnt + kRsPromLive, c);
    r.head = kNoEnt;
    r.n = 0;
    return (uint8_t)(c < 255u ? c : 255u);
}

// One lane per observer segment, its events in array order.
__global__ __launch_bounds__(256) void k_rs_apply(RsArgs a)
{
    const uint32_t nseg = a.cnt[kRsSeg];
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        int64_t p = a.seg[s];
        const uint32_t o = a.key[p];
        int64_t tlast = 0;
        for (; p < a.n && a.key[p] == o; ++p) {
            const uint32_t k = a.idx[p];
            const gsim_router_event x = a.ev[k];
            uint8_t r = 0;
            tlast = x.now_ns;
            switch (x.kind) {
            case GSIM_RS_SEEN_ADD: r = rs_seen_add(a, o, x); break;
            case GSIM_RS_SEEN_HAS: r = rs_seen_has(a, o, x); break;
            case GSIM_RS_PROMISE: r = rs_promise(a, o, a.edge[k], x); break;
            case GSIM_RS_FULFILL: r = rs_fulfill(a, o, x); break;
            default: break;                      // (a checked batch: not reached)
            }
            a.res[k] = r;
        }
        a.last[o] = tlast;
    }
}

// sweep: the entries that survive `now` move into a fresh table (cnt: the new
// counters; kRsDropped counts the swept entries).
__global__ __launch_bounds__(256) void k_rs_sweep(const SeenEnt* old, uint32_t nslots, SeenEnt* tab, uint32_t* cnt,
                                                  int64_t now)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
        const SeenEnt r = old[s];
        if (r.obs == kSlotEmpty) continue;
        if (r.expiry < now) { atomicAdd(cnt + kRsDropped, 1u); continue; }   // strict, timecache/util.go:31
        bool found;
        const uint32_t h = rs_slot<false, true>(tab, nslots - 1, r.obs, r.mid, &found);
        if (h == kNoEnt) { atomicOr(cnt + kRsErr, 1u); continue; }
        // (the claim stored obs already; the other fields are this thread's)
        tab[h].mid = r.mid;
        tab[h].expiry = r.expiry;
        atomicAdd(cnt + kRsSeenLive, 1u);
    }
}

// does the rebuild keep this promise?  (expire.Before(now), gossip_tracer.go:88; thr: ThrottlePeer's edges)
__device__ __forceinline__ bool rs_keeps(const PromEnt& en, int64_t now, const uint8_t* thr)
{
    return !(en.expire < now) && !(thr && thr[en.edge]);
}

// The promises that are neither broken at `now` nor flagged in thr (may be
// null) move into a fresh table and pool, each list in its order; a record
// without promises is not moved (cnt: the new counters; kRsDropped counts the
// dropped promises).
__global__ __launch_bounds__(256) void k_rs_prom_rebuild(const PromRec* old, uint32_t nslots, const PromEnt* opool,
                                                         PromRec* tab, PromEnt* pool, uint32_t pool_cap, uint32_t* cnt,
                                                         int64_t now, const uint8_t* thr)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
        const PromRec r = old[s];
        if (r.obs == kSlotEmpty || !r.n) continue;
        uint32_t keep = 0, k = r.head, q = 0;
        for (; q < r.n && k != kNoEnt; ++q) {
            const PromEnt en = opool[k];
            keep += rs_keeps(en, now, thr);
            k = en.next;
        }
        if (q != keep) atomicAdd(cnt + kRsDropped, q - keep);
        if (!keep) continue;
        bool found;
        const uint32_t h = rs_slot<false, true>(tab, nslots - 1, r.obs, r.mid, &found);
        if (h == kNoEnt) { atomicOr(cnt + kRsErr, 2u); continue; }
        const uint32_t base = atomicAdd(cnt + kRsPromPool, keep);
        if (base + keep > pool_cap) {            // (live promises never exceed the pool: not reached)
            atomicOr(cnt + kRsErr, 4u);
            tab[h].mid = r.mid; tab[h].head = kNoEnt; tab[h].n = 0;
            continue;
        }
        uint32_t c = 0;
        k = r.head;
        for (q = 0; q < r.n && k != kNoEnt; ++q) {
            const PromEnt en = opool[k];
            if (rs_keeps(en, now, thr)) {
                pool[base + c] = PromEnt{en.expire, en.edge, c + 1 < keep ? base + c + 1 : kNoEnt};
                ++c;
            }
            k = en.next;
        }
        tab[h].mid = r.mid; tab[h].head = base; tab[h].n = keep;
        atomicAdd(cnt + kRsPromLive, keep);
        atomicAdd(cnt + kRsPromRecs, 1u);
    }
}

// broken, first pass: the edge of every promise with expire < now (nothing changes yet)
__global__ __launch_bounds__(256) void k_rs_broken_keys(const PromRec* tab, uint32_t nslots, const PromEnt* pool,
                                                        int64_t now, uint32_t* keys, uint32_t cap, uint32_t* cnt)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
        const PromRec r = tab[s];
        if (r.obs == kSlotEmpty) continue;
        uint32_t k = r.head;
        for (uint32_t q = 0; q < r.n && k != kNoEnt; ++q) {
            const PromEnt en = pool[k];
            if (en.expire < now) {
                const uint32_t w = atomicAdd(cnt + kRsDropped, 1u);
                if (w < cap) keys[w] = en.edge;
            }
            k = en.next;
        }
    }
}

// broken: one row per run of the sorted edges; with apply, AddPenalty(peer, count)
// at the observer's peerScore (score.go:391-405), as k_tracer_apply's GSIM_EV_ADD_PENALTY
__global__ __launch_bounds__(256) void k_rs_broken_rows(const uint32_t* uniq, const uint32_t* count, uint32_t nruns,
                                                        const uint32_t* owner, const uint32_t* col, const uint32_t* rev,
                                                        const uint8_t* estate, double* bp, int32_t apply,
                                                        gsim_broken_row* rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nruns) return;
    const uint32_t e = uniq[i], c = count[i];
    rows[i] = gsim_broken_row{owner[e], col[e], c, 0u};
    if (apply) {
        const uint32_t pr = rev[e];
        if (estate[pr] & GSIM_ES_TRACKED) bp[pr] = bp[pr] + (double)c;
    }
}

// throttle: one thread per (observer, peer) pair: its edge and its checks
__global__ __launch_bounds__(256) void k_rs_pair_edges(const uint32_t* pairs, int64_t n, int64_t N,
                                                       const uint32_t* row_ptr, const uint32_t* col, uint32_t* edge,
                                                       unsigned long long* bad)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t o = pairs[2 * k], peer = pairs[2 * k + 1];
    uint32_t why = 0, e = kNoEnt;
    if ((int64_t)o >= N) why = kRsBadObserver;
    else {
        if ((int64_t)peer < N) e = rs_find_edge(row_ptr, col, o, peer);
        if (e == kNoEnt) why = kRsBadEdge;
    }
    edge[k] = e;
    if (why) atomicMin(bad, ((unsigned long long)k << 8) | why);
}

// (a checked pair list: every edge is in range; a pair named twice stores the same byte twice)
__global__ __launch_bounds__(256) void k_rs_flag_edges(const uint32_t* edge, int64_t n, uint8_t* flag, uint8_t v)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) flag[edge[k]] = v;
}

__global__ __launch_bounds__(256) void k_rs_fill_i64(int64_t* p, int64_t n, int64_t v)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) p[k] = v;
}

void rs_free(gsim_handle* h)
{
    RouterState* t = h->rs;
    if (!t) return;
    void* ptrs[] = {t->d_seen, t->d_seen2, t->d_prec, t->d_prec2, t->d_pool, t->d_pool2, t->d_cnt, t->d_bad, t->d_last,
                    t->d_ev, t->d_key, t->d_key2, t->d_idx, t->d_idx2, t->d_edge, t->d_seg, t->d_res, t->d_tmp,
                    t->d_bkey, t->d_bkey2, t->d_buniq, t->d_bcount, t->d_bruns, t->d_rows, t->d_btmp, t->d_pairs,
                    t->d_pedge, t->d_thr};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete t;
    h->rs = nullptr;
}

const char* rs_bad_text(uint32_t why)
{
    switch (why) {
    case kRsBadKind: return "unknown kind";
    case kRsBadObserver: return "observer out of range";
    case kRsBadEdge: return "the peer is not a connection of the observer";
    case kRsBadTime: return "time goes backwards for the observer";
    case kRsBadRange: return "time plus the lifetime exceeds the int64 range";
    default: return "invalid";
    }
}

int rs_enter(gsim_handle* h, bool need_config)
{
    if (!h) return GSIM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->sh) { h->err = "the router state runs on a single engine, not on a shard of a group"; return GSIM_ESTATE; }
    if (h->e == 0 || !h->x) { h->err = "no graph loaded"; return GSIM_ESTATE; }
    if (need_config && !h->rs) { h->err = "gsim_router_state_config has not been called"; return GSIM_ESTATE; }
    return GSIM_OK;
}

uint32_t rs_grid(int64_t work) { return (uint32_t)std::min<int64_t>((work + 255) / 256, 2048); }

// the batch scratch for n events
int rs_scratch(gsim_handle* h, int64_t n, int bits)
{
    RouterState* t = h->rs;
    size_t need = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(nullptr, need, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                      (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, bits,
                                                      h->stream);
    if (e != hipSuccess) return hip_check(h, e, "radix sort size");
    if (need > t->tmp_bytes) {
        if (t->d_tmp) { (void)hipFree(t->d_tmp); t->d_tmp = nullptr; t->tmp_bytes = 0; }
        e = hipMalloc(&t->d_tmp, need);
        if (e != hipSuccess) return hip_check(h, e, "radix sort scratch");
        t->tmp_bytes = need;
    }
    if (n <= t->cap_ev) return GSIM_OK;
    void** ptrs[] = {(void**)&t->d_ev, (void**)&t->d_key, (void**)&t->d_key2, (void**)&t->d_idx,
                     (void**)&t->d_idx2, (void**)&t->d_edge, (void**)&t->d_seg};
    for (void** p : ptrs)
        if (*p) { (void)hipFree(*p); *p = nullptr; }
    if (t->d_res) { (void)hipFree(t->d_res); t->d_res = nullptr; }
    t->cap_ev = 0;
    const int64_t cap = std::max<int64_t>(n, 1024);
    e = hipMalloc((void**)&t->d_ev, sizeof(gsim_router_event) * (size_t)cap);
    for (size_t q = 1; e == hipSuccess && q < sizeof(ptrs) / sizeof(ptrs[0]); ++q)
        e = hipMalloc(ptrs[q], sizeof(uint32_t) * (size_t)cap);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_res, (size_t)cap);
    if (e != hipSuccess) return hip_check(h, e, "event scratch");
    t->cap_ev = cap;
    return GSIM_OK;
}

// the live counters -> their host mirrors; cnt receives all words
int rs_read_counts(gsim_handle* h, uint32_t* cnt)
{
    RouterState* t = h->rs;
    const hipError_t e = stream_copy(h, cnt, t->d_cnt, sizeof(uint32_t) * kRsWords, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "router state counters");
    t->seen_live = cnt[kRsSeenLive];
    t->prom_live = cnt[kRsPromLive];
    t->prom_recs = cnt[kRsPromRecs];
    t->prom_pool = cnt[kRsPromPool];
    return GSIM_OK;
}

// Rebuild the promise table and pool without the promises broken at `now`
// (INT64_MIN: none) and those on the edges flagged in thr (null: none);
// *dropped their number.  Synchronizes.
int rs_prom_rebuild(gsim_handle* h, int64_t now, const uint8_t* thr, int64_t* dropped)
{
    RouterState* t = h->rs;
    uint32_t* ncnt = t->d_cnt + kRsWords;
    const size_t pool_n = (size_t)std::max<int64_t>(t->promises_cap, 1);
    hipError_t e = hipSuccess;
    if (!t->d_prec2) e = hipMalloc((void**)&t->d_prec2, sizeof(PromRec) * (size_t)t->prom_slots);
    if (e == hipSuccess && !t->d_pool2) e = hipMalloc((void**)&t->d_pool2, sizeof(PromEnt) * pool_n);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_prec2, 0xFF, sizeof(PromRec) * (size_t)t->prom_slots, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ncnt, 0, sizeof(uint32_t) * kRsWords, h->stream);
    if (e == hipSuccess) {
        ProfScope ps(h, GSIM_K_ROUTER_BROKEN);
        hipLaunchKernelGGL(k_rs_prom_rebuild, dim3(rs_grid(t->prom_slots)), dim3(256), 0, h->stream,
                           (const PromRec*)t->d_prec, t->prom_slots, (const PromEnt*)t->d_pool, t->d_prec2, t->d_pool2,
                           (uint32_t)t->promises_cap, ncnt, now, thr);
        e = hipGetLastError();
    }
    uint32_t nc[kRsWords] = {};
    if (e == hipSuccess) e = stream_copy(h, nc, ncnt, sizeof nc, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "router state: promise rebuild");
    if (nc[kRsErr]) { h->err = "router state: the rebuilt promise table overflowed"; return GSIM_ERANGE; }
    // the live table is replaced only once the rebuild has run
    e = hipMemcpyAsync(t->d_cnt + kRsPromLive, ncnt + kRsPromLive, 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice,
                       h->stream);
    if (e != hipSuccess) return hip_check(h, e, "router state: promise rebuild");
    std::swap(t->d_prec, t->d_prec2);
    std::swap(t->d_pool, t->d_pool2);
    t->prom_live = nc[kRsPromLive];
    t->prom_recs = nc[kRsPromRecs];
    t->prom_pool = nc[kRsPromPool];
    *dropped = nc[kRsDropped];
    return GSIM_OK;
}

// the first offending index of a checked list, read back; `what`: "event" / "pair"
int rs_check_bad(gsim_handle* h, const char* what, const char* where)
{
    unsigned long long bad = ~0ull;
    const hipError_t e = stream_copy(h, &bad, h->rs->d_bad, sizeof(bad), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, where);
    if (bad != ~0ull) {
        h->err = std::string(what) + " " + std::to_string(bad >> 8) + ": " + rs_bad_text((uint32_t)(bad & 0xFF));
        return GSIM_EINVAL;
    }
    return GSIM_OK;
}

// broken's scratch, sized by promises_cap
int rs_broken_scratch(gsim_handle* h, int bits)
{
    RouterState* t = h->rs;
    if (t->d_bkey) return GSIM_OK;
    const size_t cap = (size_t)std::max<int64_t>(t->promises_cap, 1);
    size_t s1 = 0, s2 = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, s1, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)cap,
                                                     0, bits, h->stream);
    if (e == hipSuccess)
        e = hipcub::DeviceRunLengthEncode::Encode(nullptr, s2, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                  (uint32_t*)nullptr, (uint32_t*)nullptr, (int)cap, h->stream);
    t->btmp_bytes = std::max<size_t>(std::max(s1, s2), 16);
    void** ptrs[] = {(void**)&t->d_bkey2, (void**)&t->d_buniq, (void**)&t->d_bcount, (void**)&t->d_bkey};
    for (size_t q = 0; e == hipSuccess && q < sizeof(ptrs) / sizeof(ptrs[0]); ++q)
        e = hipMalloc(ptrs[q], sizeof(uint32_t) * cap);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_bruns, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_rows, sizeof(gsim_broken_row) * cap);
    if (e == hipSuccess) e = hipMalloc(&t->d_btmp, t->btmp_bytes);
    if (e != hipSuccess) {
        // d_bkey is the marker: allocated last, so a failure leaves it null and the next call starts over
        void* all[] = {t->d_bkey2, t->d_buniq, t->d_bcount, t->d_bkey, t->d_bruns, t->d_rows, t->d_btmp};
        for (void* p : all)
            if (p) (void)hipFree(p);
        t->d_bkey = t->d_bkey2 = t->d_buniq = t->d_bcount = t->d_bruns = nullptr;
        t->d_rows = nullptr;
        t->d_btmp = nullptr;
        return hip_check(h, e, "router state: broken scratch");
    }
    return GSIM_OK;
}

int rs_edge_bits(const gsim_handle* h)
{
    int bits = 1;
    while (bits < 32 && (1ll << bits) < h->e) ++bits;       // keys 0..E-1
    return bits;
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void routerstate_release(gsim_handle* h) { gsim::rs_free(h); }

extern "C" {

int gsim_router_state_config(gsim_handle* h, int64_t seen_cap, int64_t promises_cap, int32_t strategy,
                             int64_t seen_ttl_ns, int64_t followup_ns)
{
    int rc = rs_enter(h, false);
    if (rc) return rc;
    if (seen_cap < 0 || promises_cap < 0 || (strategy != 0 && strategy != 1) || seen_ttl_ns < 0 || followup_ns < 0) {
        h->err = "router state: seen_cap >= 0, promises_cap >= 0, strategy 0 or 1, seen_ttl_ns >= 0 and followup_ns >= 0";
        return GSIM_EINVAL;
    }
    if (seen_cap > (1ll << 30) || promises_cap > (1ll << 30)) {
        h->err = "router state: at most 2^30 seen entries and 2^30 promises";
        return GSIM_ERANGE;
    }
    (void)hipStreamSynchronize(h->stream);
    rs_free(h);
    RouterState* t = new RouterState();
    h->rs = t;
    t->seen_cap = seen_cap;
    t->promises_cap = promises_cap;
    t->strategy = strategy;
    t->ttl = seen_ttl_ns ? seen_ttl_ns : 120000000000ll;      // TimeCacheDuration, pubsub.go:32
    t->followup = followup_ns ? followup_ns : h->gp.iwant_followup_time_ns;
    uint32_t ss = 16, ps = 16;
    while ((int64_t)ss < 2 * seen_cap) ss <<= 1;
    while ((int64_t)ps < 2 * promises_cap) ps <<= 1;
    t->seen_slots = ss;
    t->prom_slots = ps;
    hipError_t e = hipMalloc((void**)&t->d_seen, sizeof(SeenEnt) * (size_t)ss);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_prec, sizeof(PromRec) * (size_t)ps);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_pool, sizeof(PromEnt) * (size_t)std::max<int64_t>(promises_cap, 1));
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_cnt, sizeof(uint32_t) * 2 * kRsWords);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_last, sizeof(int64_t) * (size_t)h->n);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_seen, 0xFF, sizeof(SeenEnt) * (size_t)ss, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_prec, 0xFF, sizeof(PromRec) * (size_t)ps, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_cnt, 0, sizeof(uint32_t) * 2 * kRsWords, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rs_fill_i64, dim3((uint32_t)((h->n + 255) / 256)), dim3(256), 0, h->stream, t->d_last,
                           h->n, INT64_MIN);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        rs_free(h);
        return hip_check(h, e, "gsim_router_state_config");
    }
    return GSIM_OK;
}

int gsim_router_state_events(gsim_handle* h, const gsim_router_event* ev, int64_t n, uint8_t* result)
{
    int rc = rs_enter(h, true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !ev)) { h->err = "bad event list"; return GSIM_EINVAL; }
    if (n == 0) return GSIM_OK;
    if (n > 0x7FFFFFFFll) { h->err = "at most 2^31 - 1 events per batch"; return GSIM_ERANGE; }
    RouterState* t = h->rs;
    // host pre-scan: the seen entries and promises the batch could add
    int64_t want_seen = 0, want_prom = 0;
    for (int64_t k = 0; k < n; ++k) {
        want_seen += ev[k].kind == GSIM_RS_SEEN_ADD;
        want_prom += ev[k].kind == GSIM_RS_PROMISE;
    }
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= h->n) ++bits;      // keys 0..N
    rc = rs_scratch(h, n, bits);
    if (rc) return rc;

    RsArgs a{};
    a.ev = t->d_ev; a.key = t->d_key2; a.idx = t->d_idx2; a.edge = t->d_edge; a.seg = t->d_seg; a.res = t->d_res;
    a.n = n; a.N = h->n;
    a.row_ptr = h->d_row_ptr; a.col = h->d_col;
    a.seen = t->d_seen; a.smask = t->seen_slots - 1;
    a.pmask = t->prom_slots - 1; a.pool_cap = (uint32_t)t->promises_cap;
    a.cnt = t->d_cnt; a.bad = t->d_bad; a.last = t->d_last;
    a.ttl = t->ttl; a.followup = t->followup; a.strategy = t->strategy;

    const uint32_t grid = (uint32_t)((n + 255) / 256);
    hipError_t e = hipMemcpyAsync(t->d_ev, ev, sizeof(gsim_router_event) * (size_t)n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_bad, 0xFF, sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_cnt + kRsErr, 0, 4 * sizeof(uint32_t), h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_events");
    {
        ProfScope ps(h, GSIM_K_ROUTER_SORT);
        hipLaunchKernelGGL(k_rs_keys, dim3(grid), dim3(256), 0, h->stream, (const gsim_router_event*)t->d_ev, n,
                           (uint32_t)h->n, t->d_key, t->d_idx);
        e = hipGetLastError();
        size_t bytes = t->tmp_bytes;
        if (e == hipSuccess)
            e = hipcub::DeviceRadixSort::SortPairs(t->d_tmp, bytes, (const uint32_t*)t->d_key, t->d_key2,
                                                   (const uint32_t*)t->d_idx, t->d_idx2, (int)n, 0, bits, h->stream);
    }
    if (e == hipSuccess) {
        ProfScope ps(h, GSIM_K_ROUTER_RESOLVE);
        hipLaunchKernelGGL(k_rs_resolve, dim3(grid), dim3(256), 0, h->stream, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_events");
    rc = rs_check_bad(h, "event", "gsim_router_state_events");     // a bad batch fails before any change
    if (rc) return rc;
    if (t->seen_live + want_seen > t->seen_cap) {
        h->err = "the batch could add " + std::to_string(want_seen) + " seen entries, " +
                 std::to_string(t->seen_cap - t->seen_live) + " are free (gsim_router_state_config, gsim_router_state_sweep)";
        return GSIM_ERANGE;
    }
    if (t->prom_live + want_prom > t->promises_cap) {
        h->err = "the batch could add " + std::to_string(want_prom) + " promises, " +
                 std::to_string(t->promises_cap - t->prom_live) + " are free (gsim_router_state_config, gsim_router_state_broken)";
        return GSIM_ERANGE;
    }
    // the pool entries and records that fulfilled promises left behind: compacted when the batch needs their space
    if (t->prom_pool + want_prom > t->promises_cap || t->prom_recs + want_prom > t->promises_cap) {
        int64_t none = 0;
        rc = rs_prom_rebuild(h, INT64_MIN, nullptr, &none);
        if (rc) return rc;
    }
    a.prec = t->d_prec; a.pool = t->d_pool;
    {
        ProfScope ps(h, GSIM_K_ROUTER_APPLY);
        const int64_t segs = std::min<int64_t>(n, h->n);
        hipLaunchKernelGGL(k_rs_apply, dim3((uint32_t)std::min<int64_t>((segs + 255) / 256, 65536)), dim3(256), 0,
                           h->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess && result) e = hipMemcpyAsync(result, t->d_res, (size_t)n, hipMemcpyDeviceToHost, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "k_rs_apply");
    uint32_t cnt[kRsWords];
    rc = rs_read_counts(h, cnt);
    if (rc) return rc;
    if (cnt[kRsErr]) { h->err = "router state: a table overflowed"; return GSIM_ERANGE; }
    t->applied += n;
    t->fulfilled += cnt[kRsFulfilled];
    return GSIM_OK;
}

int gsim_router_state_sweep(gsim_handle* h, int64_t now_ns)
{
    int rc = rs_enter(h, true);
    if (rc) return rc;
    RouterState* t = h->rs;
    uint32_t* ncnt = t->d_cnt + kRsWords;
    hipError_t e = hipSuccess;
    if (!t->d_seen2) e = hipMalloc((void**)&t->d_seen2, sizeof(SeenEnt) * (size_t)t->seen_slots);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_seen2, 0xFF, sizeof(SeenEnt) * (size_t)t->seen_slots, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ncnt, 0, sizeof(uint32_t) * kRsWords, h->stream);
    if (e == hipSuccess) {
        ProfScope ps(h, GSIM_K_ROUTER_SWEEP);
        hipLaunchKernelGGL(k_rs_sweep, dim3(rs_grid(t->seen_slots)), dim3(256), 0, h->stream, (const SeenEnt*)t->d_seen,
                           t->seen_slots, t->d_seen2, ncnt, now_ns);
        e = hipGetLastError();
    }
    uint32_t nc[kRsWords] = {};
    if (e == hipSuccess) e = stream_copy(h, nc, ncnt, sizeof nc, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_sweep");
    if (nc[kRsErr]) { h->err = "router state: the rebuilt seen table overflowed"; return GSIM_ERANGE; }
    // the live table is replaced only once the rebuild has run
    e = hipMemcpyAsync(t->d_cnt + kRsSeenLive, ncnt + kRsSeenLive, sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_sweep");
    std::swap(t->d_seen, t->d_seen2);
    t->seen_live = nc[kRsSeenLive];
    t->swept += nc[kRsDropped];
    return GSIM_OK;
}

int gsim_router_state_throttle(gsim_handle* h, const uint32_t* pairs, int64_t n, int64_t* dropped)
{
    int rc = rs_enter(h, true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !pairs)) { h->err = "bad pair list"; return GSIM_EINVAL; }
    if (dropped) *dropped = 0;
    if (n == 0) return GSIM_OK;
    if (n > 0x3FFFFFFFll) { h->err = "at most 2^30 - 1 pairs per call"; return GSIM_ERANGE; }
    RouterState* t = h->rs;
    hipError_t e = hipSuccess;
    if (n > t->cap_pairs) {
        if (t->d_pairs) { (void)hipFree(t->d_pairs); t->d_pairs = nullptr; }
        if (t->d_pedge) { (void)hipFree(t->d_pedge); t->d_pedge = nullptr; }
        t->cap_pairs = 0;
        const int64_t cap = std::max<int64_t>(n, 1024);
        e = hipMalloc((void**)&t->d_pairs, sizeof(uint32_t) * 2 * (size_t)cap);
        if (e == hipSuccess) e = hipMalloc((void**)&t->d_pedge, sizeof(uint32_t) * (size_t)cap);
        if (e != hipSuccess) return hip_check(h, e, "router state: pair scratch");
        t->cap_pairs = cap;
    }
    if (!t->d_thr) {
        e = hipMalloc((void**)&t->d_thr, (size_t)h->e);
        if (e == hipSuccess) e = hipMemsetAsync(t->d_thr, 0, (size_t)h->e, h->stream);
        if (e != hipSuccess) return hip_check(h, e, "router state: edge flags");
    }
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    e = hipMemcpyAsync(t->d_pairs, pairs, sizeof(uint32_t) * 2 * (size_t)n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_bad, 0xFF, sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rs_pair_edges, dim3(grid), dim3(256), 0, h->stream, (const uint32_t*)t->d_pairs, n, h->n,
                           (const uint32_t*)h->d_row_ptr, (const uint32_t*)h->d_col, t->d_pedge, t->d_bad);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_throttle");
    rc = rs_check_bad(h, "pair", "gsim_router_state_throttle");
    if (rc) return rc;
    int64_t gone = 0;
    hipLaunchKernelGGL(k_rs_flag_edges, dim3(grid), dim3(256), 0, h->stream, (const uint32_t*)t->d_pedge, n, t->d_thr,
                       (uint8_t)1);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_throttle");
    rc = rs_prom_rebuild(h, INT64_MIN, t->d_thr, &gone);
    // the flags are cleared again whatever the rebuild returned
    hipLaunchKernelGGL(k_rs_flag_edges, dim3(grid), dim3(256), 0, h->stream, (const uint32_t*)t->d_pedge, n, t->d_thr,
                       (uint8_t)0);
    e = hipGetLastError();
    if (rc) return rc;
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_throttle");
    t->fulfilled += gone;
    if (dropped) *dropped = gone;
    return GSIM_OK;
}

int gsim_router_state_broken(gsim_handle* h, int64_t now_ns, int32_t apply_penalty, gsim_broken_row* out, int64_t cap,
                             int64_t* n)
{
    int rc = rs_enter(h, true);
    if (rc) return rc;
    if (!n || cap < 0 || (cap > 0 && !out)) { h->err = "bad row list"; return GSIM_EINVAL; }
    *n = 0;
    RouterState* t = h->rs;
    const int bits = rs_edge_bits(h);
    rc = rs_broken_scratch(h, bits);
    if (rc) return rc;
    const uint32_t kcap = (uint32_t)std::max<int64_t>(t->promises_cap, 1);
    hipError_t e = hipMemsetAsync(t->d_cnt + kRsDropped, 0, sizeof(uint32_t), h->stream);
    if (e == hipSuccess) {
        ProfScope ps(h, GSIM_K_ROUTER_BROKEN);
        hipLaunchKernelGGL(k_rs_broken_keys, dim3(rs_grid(t->prom_slots)), dim3(256), 0, h->stream,
                           (const PromRec*)t->d_prec, t->prom_slots, (const PromEnt*)t->d_pool, now_ns, t->d_bkey, kcap,
                           t->d_cnt);
        e = hipGetLastError();
    }
    uint32_t nb = 0;
    if (e == hipSuccess) e = stream_copy(h, &nb, t->d_cnt + kRsDropped, sizeof nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_broken");
    if (nb > kcap) { h->err = "router state: more broken promises than promises"; return GSIM_ERANGE; }
    uint32_t nruns = 0;
    if (nb) {
        {
            ProfScope ps(h, GSIM_K_ROUTER_BROKEN);
            size_t bytes = t->btmp_bytes;
            e = hipcub::DeviceRadixSort::SortKeys(t->d_btmp, bytes, (const uint32_t*)t->d_bkey, t->d_bkey2, (int)nb, 0,
                                                  bits, h->stream);
            bytes = t->btmp_bytes;
            if (e == hipSuccess)
                e = hipcub::DeviceRunLengthEncode::Encode(t->d_btmp, bytes, (const uint32_t*)t->d_bkey2, t->d_buniq,
                                                          t->d_bcount, t->d_bruns, (int)nb, h->stream);
        }
        if (e == hipSuccess) e = stream_copy(h, &nruns, t->d_bruns, sizeof nruns, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_broken");
    }
    *n = nruns;
    if ((int64_t)nruns > cap) {
        h->err = std::to_string(nruns) + " (observer, peer) rows, room for " + std::to_string(cap);
        return GSIM_ERANGE;
    }
    if (nruns) {
        if (apply_penalty) {
            rc = deliver_flush(h);                   // as a GSIM_EV_ADD_PENALTY batch: pending first deliveries come first
            if (rc) return rc;
        }
        {
            ProfScope ps(h, GSIM_K_ROUTER_BROKEN);
            hipLaunchKernelGGL(k_rs_broken_rows, dim3((nruns + 255) / 256), dim3(256), 0, h->stream,
                               (const uint32_t*)t->d_buniq, (const uint32_t*)t->d_bcount, nruns,
                               (const uint32_t*)h->d_owner, (const uint32_t*)h->d_col, (const uint32_t*)h->d_rev,
                               (const uint8_t*)h->d_estate, h->d_bp, apply_penalty, t->d_rows);
            e = hipGetLastError();
        }
        if (e == hipSuccess)
            e = stream_copy(h, out, t->d_rows, sizeof(gsim_broken_row) * (size_t)nruns, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_check(h, e, "gsim_router_state_broken");
    }
    int64_t gone = 0;
    rc = rs_prom_rebuild(h, now_ns, nullptr, &gone);
    if (rc) return rc;
    t->broken += gone;
    return GSIM_OK;
}

int gsim_router_state_stats(gsim_handle* h, int64_t* out6)
{
    int rc = rs_enter(h, true);
    if (rc) return rc;
    if (!out6) return GSIM_EINVAL;
    const RouterState* t = h->rs;
    out6[0] = t->seen_live;
    out6[1] = t->prom_live;
    out6[2] = t->applied;
    out6[3] = t->swept;
    out6[4] = t->fulfilled;
    out6[5] = t->broken;
    return GSIM_OK;
}

}  // extern "C"
