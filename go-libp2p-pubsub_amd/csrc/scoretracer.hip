// Score tracer events (include/gsim.h gsim_score_tracer_*; SURVEY.md §8(b)
// part 2): peerScore's RawTracer surface (trace.go:27-60, score.go:88) driven
// from outside.  A batch of ValidateMessage / DeliverMessage / RejectMessage /
// DuplicateMessage / Graft / Prune / AddPenalty calls, each addressed to one
// observer's peerScore, is applied to the record-order score planes and to the
// observers' delivery records (score.go:90-120, 693-877), which live here.
//
// A batch runs in three stages:
//   sort     a stable radix sort of (observer, index) groups the events by
//            observer and keeps each observer's array order;
//   resolve  one thread per event finds its edge (a binary search of the
//            observer's row, as k_churn_find), runs every check of the batch
//            and notes the first offending index; segment heads are listed;
//   apply    one lane per observer segment walks its events in order.  The
//            events of one observer are a dependency chain (each may read what
//            the one before wrote: the same record, the same counters), so the
//            parallelism is across observers.
//
// Delivery records: one open-addressing table keyed (observer, message id).
// A slot is claimed by a device-scope CAS on its observer word and is from
// then on read and written only by that observer's lane, so the other fields
// need no atomics.  deliveryRecord.peers is a list through a bump-allocated
// pool of (record index, next).  gsim_score_tracer_gc rebuilds table and pool
// from the surviving records, so collected space is free again.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "gsim_internal.h"

namespace gsim {

constexpr uint32_t kRecEmpty = 0xFFFFFFFFu;   // an unclaimed table slot's observer word
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;    // end of a peers list / no record
// deliveryRecord.status (score.go:104-112)
enum : uint32_t { kDrUnknown = 0, kDrValid, kDrInvalid, kDrIgnored, kDrThrottled };
// why an event fails the batch (k_tracer_resolve)
enum : uint32_t { kBadKind = 1, kBadReason, kBadObserver, kBadPeer, kBadEdge, kBadTopic, kBadJoin, kBadTime };
// d_cnt words
// (kCntErr, kCntSeg, kCntSettled are per batch: cleared together before each)
enum : int { kCntLive = 0, kCntPool, kCntPeers, kCntErr, kCntSeg, kCntSettled, kCntCollected, kCntWords = 8 };

struct DRec {             // 40 bytes
    uint64_t mid;
    int64_t validated;    // when status became valid
    int64_t expire;
    uint32_t obs;         // the claim word: kRecEmpty or the owning observer
    uint32_t head;        // peers list (pool index), kNoEntry: empty / released
    uint32_t npeers;
    uint32_t status;
};

struct PeerEnt {
    uint32_t rec;         // the peer's record index rev[e] (the observer's record about it)
    uint32_t next;
};

struct ScoreTracer {
    int64_t records_cap = 0, peers_cap = 0, ttl = 0;
    uint32_t nslots = 0;              // table slots, a power of two >= 2 records_cap
    DRec* d_rec = nullptr;
    PeerEnt* d_pool = nullptr;
    DRec* d_rec2 = nullptr;           // gc's other table and pool (allocated at the first gc, swapped by each)
    PeerEnt* d_pool2 = nullptr;
    uint32_t* d_cnt = nullptr;        // [2][kCntWords]: the live counters, gc's new ones
    unsigned long long* d_bad = nullptr;   // first offending index << 8 | why
    int64_t* d_last = nullptr;        // [N] each observer's last event time
    // host mirrors of the counters (read back after every batch and gc)
    int64_t live = 0, pool_used = 0, live_peers = 0, applied = 0, collected = 0;
    int64_t settled = 0;              // records whose pending mcnt increments an event settled (gsim_score_tracer_settled)
    // batch scratch, grow-only
    int64_t cap_ev = 0;
    gsim_score_event* d_ev = nullptr;
    uint32_t *d_key = nullptr, *d_key2 = nullptr, *d_idx = nullptr, *d_idx2 = nullptr, *d_edge = nullptr,
             *d_seg = nullptr;
    void* d_tmp = nullptr;
    size_t tmp_bytes = 0;
};

struct TracerArgs {
    const gsim_score_event* ev;
    const uint32_t *key, *idx;        // sorted: observer (clamped to N) and event index of each position
    uint32_t *edge, *seg;             // [n] edge of each event (by index); first position of each segment
    int64_t n, N, E;
    int32_t T, t_scored;              // topics of the views; topics with parameters (h->t)
    const gsim_topic_score_params* tp;
    const uint32_t *row_ptr, *col, *rev, *owner;
    const uint64_t *sub, *smask;
    double *first, *meshd, *fail, *invalid;
    uint8_t* mcnt;
    int64_t *graft, *mtime;
    uint8_t* tflags;
    double* bp;
    const uint8_t* estate;
    uint32_t* inv_live;
    DRec* rec;
    uint32_t mask;                    // nslots - 1
    PeerEnt* pool;
    uint32_t pool_cap;
    uint32_t* cnt;
    unsigned long long* bad;
    int64_t* last;
    int64_t ttl;
};

namespace {

__global__ __launch_bounds__(256) void k_tracer_keys(const gsim_score_event* ev, int64_t n, uint32_t N, uint32_t* key,
                                                     uint32_t* idx)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t o = ev[k].observer;
    key[k] = o < N ? o : N;           // every observer out of range sorts last (and fails the batch)
    idx[k] = (uint32_t)k;
}

// One thread per sorted position: the event's edge, its checks, its segment.
__global__ __launch_bounds__(256) void k_tracer_resolve(TracerArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t k = a.idx[p], o = a.key[p];
    const gsim_score_event x = a.ev[k];
    const bool head = p == 0 || a.key[p - 1] != o;
    uint32_t why = 0, e = 0xFFFFFFFFu;
    if (x.kind > GSIM_EV_ADD_PENALTY) why = kBadKind;
    else if (x.kind == GSIM_EV_REJECT && x.arg > GSIM_REJECT_SELF_ORIGIN) why = kBadReason;
    else if ((int64_t)x.observer >= a.N) why = kBadObserver;
    else if ((int64_t)x.peer >= a.N) why = kBadPeer;
    else {
        uint32_t lo = a.row_ptr[o], hi = a.row_ptr[o + 1];
        const uint32_t end = hi;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (a.col[mid] < x.peer) lo = mid + 1; else hi = mid;
        }
        if (lo < end && a.col[lo] == x.peer) e = lo;
        if (e == 0xFFFFFFFFu) why = kBadEdge;
        else if (x.kind != GSIM_EV_ADD_PENALTY) {
            if ((int32_t)x.topic >= a.T) why = kBadTopic;
            else if (!((a.sub[o] >> x.topic) & 1ull)) why = kBadJoin;
        }
    }
    if (!why) {
        // non-decreasing per observer: against the event before it in the
        // segment, the segment's first against the observer's last batch
        const int64_t prev = head ? a.last[o] : a.ev[a.idx[p - 1]].now_ns;
        if (x.now_ns < prev) why = kBadTime;
    }
    a.edge[k] = e;
    if (why) atomicMin(a.bad, ((unsigned long long)k << 8) | why);
    if (head && (int64_t)o < a.N) a.seg[atomicAdd(a.cnt + kCntSeg, 1u)] = (uint32_t)p;
}

// ---- the score records (record order: index r = rev[e], in the peer's row) ---

__device__ __forceinline__ bool tr_scored(const TracerArgs& a, int32_t t)
{
    return t < a.t_scored && const_tp(a.tp)[t].scored != 0;
}

// the plane index of record r's topic t; false: no peerStats, no score
// parameters, or the peer holds no slot for t (ensure_slots ran: not reached)
__device__ __forceinline__ bool tr_record(const TracerArgs& a, uint32_t r, int32_t t, int64_t* i)
{
    if (!(a.estate[r] & GSIM_ES_TRACKED) || !tr_scored(a, t)) return false;
    const uint64_t mj = smask_of(a.smask, a.owner[r]);
    if (!slot_has(mj, t)) return false;
    *i = slot_idx(mj, t, a.E, r);
    return true;
}

// meshMessageDeliveries += 1 up to the cap; the pending delivery increments
// are part of the counter and come first (apply_incs)
__device__ __forceinline__ void tr_meshd_inc(const TracerArgs& a, int64_t i, double cap)
{
    double md = a.meshd[i];
    const uint8_t pc = a.mcnt[i];
    if (pc) { md = apply_incs(md, pc, cap); a.mcnt[i] = 0; atomicAdd(a.cnt + kCntSettled, 1u); }
    double x = md + 1.0;
    if (x > cap) x = cap;
    a.meshd[i] = x;
}

// score.go:901-914
__device__ void tr_mark_invalid(const TracerArgs& a, uint32_t r, int32_t t)
{
    int64_t i;
    if (!tr_record(a, r, t, &i)) return;
    a.invalid[i] = a.invalid[i] + 1.0;
    *a.inv_live = 1u;                 // the refresh reads the invalid planes again
}

// score.go:919-946
__device__ void tr_mark_first(const TracerArgs& a, uint32_t r, int32_t t)
{
    int64_t i;
    if (!tr_record(a, r, t, &i)) return;
    const ctp_t tp = const_tp(a.tp) + t;
    double x = a.first[i] + 1.0;
    if (x > tp->first_message_deliveries_cap) x = tp->first_message_deliveries_cap;
    a.first[i] = x;
    if (!(a.tflags[i] & GSIM_TF_IN_MESH)) return;
    tr_meshd_inc(a, i, tp->mesh_message_deliveries_cap);
}

// score.go:951-981
__device__ void tr_mark_duplicate(const TracerArgs& a, uint32_t r, int32_t t, bool has_validated, int64_t validated,
                                  int64_t now)
{
    int64_t i;
    if (!tr_record(a, r, t, &i)) return;
    if (!(a.tflags[i] & GSIM_TF_IN_MESH)) return;
    const ctp_t tp = const_tp(a.tp) + t;
    if (has_validated && (now - validated) > tp->mesh_message_deliveries_window_ns) return;
    tr_meshd_inc(a, i, tp->mesh_message_deliveries_cap);
}

// score.go:649-667; lazy meshTime: graft = now, meshTime = 0
__device__ void tr_graft(const TracerArgs& a, uint32_t r, int32_t t, int64_t now)
{
    int64_t i;
    if (!tr_record(a, r, t, &i)) return;
    a.tflags[i] = (uint8_t)((a.tflags[i] | GSIM_TF_IN_MESH) & ~GSIM_TF_ACTIVE);
    a.graft[i] = now;
    a.mtime[i] = 0;
}

// score.go:669-691
__device__ void tr_prune(const TracerArgs& a, uint32_t r, int32_t t)
{
    int64_t i;
    if (!tr_record(a, r, t, &i)) return;
    const ctp_t tp = const_tp(a.tp) + t;
    const uint8_t fl = a.tflags[i];
    if (fl & GSIM_TF_ACTIVE) {
        double md = a.meshd[i];
        const uint8_t pc = a.mcnt[i];
        if (pc) {
            md = apply_incs(md, pc, tp->mesh_message_deliveries_cap);
            a.meshd[i] = md;
            a.mcnt[i] = 0;
            atomicAdd(a.cnt + kCntSettled, 1u);
        }
        const double thr = tp->mesh_message_deliveries_threshold;
        if (md < thr) {
            const double deficit = thr - md;
            a.fail[i] = a.fail[i] + deficit * deficit;
        }
    }
    if (fl & GSIM_TF_IN_MESH) {
        a.mtime[i] = 0;               // meshTime outside the mesh is 0
        a.tflags[i] = (uint8_t)(fl & ~GSIM_TF_IN_MESH);
    }
}

// ---- delivery records --------------------------------------------------------

__device__ __forceinline__ uint32_t tr_hash(uint32_t o, uint64_t mid)
{
    uint64_t x = mid ^ ((uint64_t)o * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return (uint32_t)x;
}

// Claim an empty slot of table `rec` for (o, mid), or find the observer's own.
// found: the slot held the key already.  kNoEntry: the table is full (the
// capacity check of the batch keeps half of it empty: not reached).
// Find = false (gc's rebuild: every key is new, and an observer's records are
// moved by many threads): claim only, no slot's other fields are read.
template <bool Find>
__device__ uint32_t tr_slot(DRec* rec, uint32_t mask, uint32_t o, uint64_t mid, bool* found)
{
    uint32_t h = tr_hash(o, mid) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe, h = (h + 1) & mask) {
        uint32_t w = __hip_atomic_load(&rec[h].obs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == kRecEmpty) {
            w = atomicCAS(&rec[h].obs, kRecEmpty, o);
            if (w == kRecEmpty) { *found = false; return h; }
        }
        // another observer's slot never becomes this one's; this observer's
        // slots are written by this lane only
        if (Find && w == o && rec[h].mid == mid) { *found = true; return h; }
    }
    return kNoEntry;
}

// score.go:840-861 getRecord
__device__ uint32_t tr_get_record(const TracerArgs& a, uint32_t o, uint64_t mid, int64_t now)
{
    bool found = false;
    const uint32_t h = tr_slot<true>(a.rec, a.mask, o, mid, &found);
    if (h == kNoEntry) { atomicOr(a.cnt + kCntErr, 1u); return h; }
    if (!found) {
        DRec& r = a.rec[h];
        r.mid = mid;
        r.validated = 0;
        r.expire = now + a.ttl;
        r.head = kNoEntry;
        r.npeers = 0;
        r.status = kDrUnknown;
        atomicAdd(a.cnt + kCntLive, 1u);
    }
    return h;
}

__device__ bool tr_has_peer(const TracerArgs& a, const DRec& r, uint32_t pr)
{
    uint32_t k = r.head;
    for (uint32_t q = 0; q < r.npeers && k != kNoEntry; ++q) {
        const PeerEnt x = a.pool[k];
        if (x.rec == pr) return true;
        k = x.next;
    }
    return false;
}

__device__ void tr_add_peer(const TracerArgs& a, DRec& r, uint32_t pr)
{
    const uint32_t k = atomicAdd(a.cnt + kCntPool, 1u);
    if (k >= a.pool_cap) { atomicOr(a.cnt + kCntErr, 2u); return; }   // (the capacity check: not reached)
    a.pool[k] = PeerEnt{pr, r.head};
    r.head = k;
    r.npeers += 1;
    atomicAdd(a.cnt + kCntPeers, 1u);
}

// drec.peers = nil: the entries are reclaimed by the next gc
__device__ void tr_release(const TracerArgs& a, DRec& r)
{
    if (r.npeers) atomicSub(a.cnt + kCntPeers, r.npeers);
    r.head = kNoEntry;
    r.npeers = 0;
}

// score.go:702-726
__device__ void tr_deliver(const TracerArgs& a, uint32_t o, uint32_t pr, const gsim_score_event& x)
{
    tr_mark_first(a, pr, x.topic);
    const uint32_t h = tr_get_record(a, o, x.mid, x.now_ns);
    if (h == kNoEntry) return;
    DRec& r = a.rec[h];
    if (r.status != kDrUnknown) return;
    r.status = kDrValid;
    r.validated = x.now_ns;
    uint32_t k = r.head;
    for (uint32_t q = 0; q < r.npeers && k != kNoEntry; ++q) {
        const PeerEnt en = a.pool[k];
        // the peers that forwarded it while it was validated: no window
        if (en.rec != pr) tr_mark_duplicate(a, en.rec, x.topic, false, 0, x.now_ns);
        k = en.next;
    }
}

// score.go:728-793
__device__ void tr_reject(const TracerArgs& a, uint32_t o, uint32_t pr, const gsim_score_event& x)
{
    switch (x.arg) {
    case GSIM_REJECT_MISSING_SIGNATURE: case GSIM_REJECT_INVALID_SIGNATURE: case GSIM_REJECT_UNEXPECTED_SIGNATURE:
    case GSIM_REJECT_UNEXPECTED_AUTH_INFO: case GSIM_REJECT_SELF_ORIGIN:
        tr_mark_invalid(a, pr, x.topic);
        return;
    case GSIM_REJECT_BLACKLISTED_PEER: case GSIM_REJECT_BLACKLISTED_SOURCE: case GSIM_REJECT_VALIDATION_QUEUE_FULL:
        return;
    default: break;
    }
    const uint32_t h = tr_get_record(a, o, x.mid, x.now_ns);
    if (h == kNoEntry) return;
    DRec& r = a.rec[h];
    if (r.status != kDrUnknown) return;
    if (x.arg == GSIM_REJECT_VALIDATION_THROTTLED) { r.status = kDrThrottled; tr_release(a, r); return; }
    if (x.arg == GSIM_REJECT_VALIDATION_IGNORED) { r.status = kDrIgnored; tr_release(a, r); return; }
    r.status = kDrInvalid;
    tr_mark_invalid(a, pr, x.topic);
    uint32_t k = r.head;
    for (uint32_t q = 0; q < r.npeers && k != kNoEntry; ++q) {
        const PeerEnt en = a.pool[k];
        tr_mark_invalid(a, en.rec, x.topic);
        k = en.next;
    }
    tr_release(a, r);
}

// score.go:795-827
__device__ void tr_duplicate(const TracerArgs& a, uint32_t o, uint32_t pr, const gsim_score_event& x)
{
    const uint32_t h = tr_get_record(a, o, x.mid, x.now_ns);
    if (h == kNoEntry) return;
    DRec& r = a.rec[h];
    if (tr_has_peer(a, r, pr)) return;           // already seen this duplicate
    switch (r.status) {
    case kDrUnknown:
        tr_add_peer(a, r, pr);
        break;
    case kDrValid:
        tr_add_peer(a, r, pr);
        tr_mark_duplicate(a, pr, x.topic, true, r.validated, x.now_ns);
        break;
    case kDrInvalid:
        tr_mark_invalid(a, pr, x.topic);
        break;
    default:                                     // throttled / ignored
        break;
    }
}

// One lane per observer segment, its events in array order.
__global__ __launch_bounds__(256) void k_tracer_apply(TracerArgs a)
{
    const uint32_t nseg = a.cnt[kCntSeg];
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        int64_t p = a.seg[s];
        const uint32_t o = a.key[p];
        int64_t tlast = 0;
        for (; p < a.n && a.key[p] == o; ++p) {
            const uint32_t k = a.idx[p];
            const gsim_score_event x = a.ev[k];
            const uint32_t e = a.edge[k];
            if ((int64_t)e >= a.E) continue;     // (a checked batch: not reached)
            const uint32_t pr = a.rev[e];
            tlast = x.now_ns;
            switch (x.kind) {
            case GSIM_EV_VALIDATE: (void)tr_get_record(a, o, x.mid, x.now_ns); break;
            case GSIM_EV_DELIVER: tr_deliver(a, o, pr, x); break;
            case GSIM_EV_REJECT: tr_reject(a, o, pr, x); break;
            case GSIM_EV_DUPLICATE: tr_duplicate(a, o, pr, x); break;
            case GSIM_EV_GRAFT: tr_graft(a, pr, x.topic, x.now_ns); break;
            case GSIM_EV_PRUNE: tr_prune(a, pr, x.topic); break;
            case GSIM_EV_ADD_PENALTY:                            // score.go:391-405
                if (a.estate[pr] & GSIM_ES_TRACKED) a.bp[pr] = a.bp[pr] + (double)x.arg;
                break;
            default: break;
            }
        }
        a.last[o] = tlast;
    }
}

// gc: the records that survive `now` move into a fresh table and pool
// (cnt: the new counters; kCntCollected counts the dropped records).
__global__ __launch_bounds__(256) void k_tracer_gc(const DRec* old, uint32_t nslots, const PeerEnt* opool, DRec* rec,
                                                   PeerEnt* pool, uint32_t pool_cap, uint32_t* cnt, int64_t now)
{
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < nslots; s += stride) {
        const DRec r = old[s];
        if (r.obs == kRecEmpty) continue;
        if (now > r.expire) { atomicAdd(cnt + kCntCollected, 1u); continue; }   // strict, score.go:869
        bool found = false;
        const uint32_t h = tr_slot<false>(rec, nslots - 1, r.obs, r.mid, &found);
        if (h == kNoEntry) { atomicOr(cnt + kCntErr, 1u); continue; }
        DRec q = r;
        q.head = kNoEntry;
        q.npeers = 0;
        if (r.npeers) {
            const uint32_t base = atomicAdd(cnt + kCntPool, r.npeers);
            if (base + r.npeers <= pool_cap) {
                uint32_t k = r.head, c = 0;
                for (; c < r.npeers && k != kNoEntry; ++c) {
                    const PeerEnt en = opool[k];
                    pool[base + c] = PeerEnt{en.rec, c + 1 < r.npeers ? base + c + 1 : kNoEntry};
                    k = en.next;
                }
                q.head = base;
                q.npeers = r.npeers;
                atomicAdd(cnt + kCntPeers, r.npeers);
            } else {
                atomicOr(cnt + kCntErr, 2u);
            }
        }
        // (the claim stored q.obs already; the other fields are this thread's)
        rec[h].mid = q.mid; rec[h].validated = q.validated; rec[h].expire = q.expire;
        rec[h].head = q.head; rec[h].npeers = q.npeers; rec[h].status = q.status;
        atomicAdd(cnt + kCntLive, 1u);
    }
}

void tracer_free(gsim_handle* h)
{
    ScoreTracer* t = h->st;
    if (!t) return;
    void* ptrs[] = {t->d_rec, t->d_pool, t->d_rec2, t->d_pool2, t->d_cnt, t->d_bad, t->d_last, t->d_ev, t->d_key, t->d_key2,
                    t->d_idx, t->d_idx2, t->d_edge, t->d_seg, t->d_tmp};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete t;
    h->st = nullptr;
}

__global__ __launch_bounds__(256) void k_tracer_fill_i64(int64_t* p, int64_t n, int64_t v)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) p[k] = v;
}

const char* bad_text(uint32_t why)
{
    switch (why) {
    case kBadKind: return "unknown kind";
    case kBadReason: return "reject reason above 10";
    case kBadObserver: return "observer out of range";
    case kBadPeer: return "peer out of range";
    case kBadEdge: return "the peer is not a connection of the observer";
    case kBadTopic: return "topic out of range";
    case kBadJoin: return "the observer has not announced the topic";
    case kBadTime: return "time goes backwards for the observer";
    default: return "invalid";
    }
}

int tracer_enter(gsim_handle* h, bool need_config)
{
    if (!h) return GSIM_EINVAL;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->sh) { h->err = "the score tracer runs on a single engine, not on a shard of a group"; return GSIM_ESTATE; }
    if (h->e == 0 || !h->x) { h->err = "no graph loaded"; return GSIM_ESTATE; }
    if (need_config && !h->st) { h->err = "gsim_score_tracer_config has not been called"; return GSIM_ESTATE; }
    return GSIM_OK;
}

// the batch scratch for n events
int tracer_scratch(gsim_handle* h, int64_t n, int bits)
{
    ScoreTracer* t = h->st;
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
    t->cap_ev = 0;
    const int64_t cap = std::max<int64_t>(n, 1024);
    e = hipMalloc((void**)&t->d_ev, sizeof(gsim_score_event) * (size_t)cap);
    for (size_t q = 1; e == hipSuccess && q < sizeof(ptrs) / sizeof(ptrs[0]); ++q)
        e = hipMalloc(ptrs[q], sizeof(uint32_t) * (size_t)cap);
    if (e != hipSuccess) return hip_check(h, e, "event scratch");
    t->cap_ev = cap;
    return GSIM_OK;
}

// the live counters -> their host mirrors
int tracer_read_counts(gsim_handle* h, uint32_t* cnt)
{
    hipError_t e = hipMemcpyAsync(cnt, h->st->d_cnt, sizeof(uint32_t) * kCntWords, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "score tracer counters");
    h->st->live = cnt[kCntLive];
    h->st->pool_used = cnt[kCntPool];
    h->st->live_peers = cnt[kCntPeers];
    return GSIM_OK;
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void scoretracer_release(gsim_handle* h) { gsim::tracer_free(h); }

extern "C" {

int gsim_score_tracer_config(gsim_handle* h, int64_t records_cap, int64_t peers_cap, int64_t seen_ttl_ns)
{
    int rc = tracer_enter(h, false);
    if (rc) return rc;
    if (records_cap <= 0 || peers_cap < 0 || seen_ttl_ns < 0) {
        h->err = "score tracer: records_cap > 0, peers_cap >= 0 and seen_ttl_ns >= 0";
        return GSIM_EINVAL;
    }
    if (records_cap > (1ll << 30) || peers_cap > 0xFFFFFFF0ll) {
        h->err = "score tracer: at most 2^30 records and 2^32 - 16 peers-list entries";
        return GSIM_ERANGE;
    }
    (void)hipStreamSynchronize(h->stream);
    tracer_free(h);
    ScoreTracer* t = new ScoreTracer();
    h->st = t;
    t->records_cap = records_cap;
    t->peers_cap = peers_cap;
    t->ttl = seen_ttl_ns ? seen_ttl_ns : 120000000000ll;      // TimeCacheDuration, pubsub.go:32
    uint32_t nslots = 16;
    while ((int64_t)nslots < 2 * records_cap) nslots <<= 1;
    t->nslots = nslots;
    hipError_t e = hipMalloc((void**)&t->d_rec, sizeof(DRec) * (size_t)nslots);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_pool, sizeof(PeerEnt) * (size_t)std::max<int64_t>(peers_cap, 1));
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_cnt, sizeof(uint32_t) * 2 * kCntWords);
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_bad, sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&t->d_last, sizeof(int64_t) * (size_t)h->n);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_rec, 0xFF, sizeof(DRec) * (size_t)nslots, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_cnt, 0, sizeof(uint32_t) * 2 * kCntWords, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tracer_fill_i64, dim3((uint32_t)((h->n + 255) / 256)), dim3(256), 0, h->stream, t->d_last,
                           h->n, INT64_MIN);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        tracer_free(h);
        return hip_check(h, e, "gsim_score_tracer_config");
    }
    return GSIM_OK;
}

int gsim_score_tracer_events(gsim_handle* h, const gsim_score_event* ev, int64_t n)
{
    int rc = tracer_enter(h, true);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !ev)) { h->err = "bad event list"; return GSIM_EINVAL; }
    if (n == 0) return GSIM_OK;
    if (n > 0x7FFFFFFFll) { h->err = "at most 2^31 - 1 events per batch"; return GSIM_ERANGE; }
    ScoreTracer* t = h->st;
    // host pre-scan: the records and peers-list entries the batch could need,
    // its earliest time, the topic slots its peers need (a topic
    // without score parameters has no record to hold: tr_record)
    int64_t want_rec = 0, want_peers = 0, tmin = INT64_MAX;
    const bool slots = !h->smask.empty();
    std::vector<uint64_t> need;
    for (int64_t k = 0; k < n; ++k) {
        const gsim_score_event& x = ev[k];
        tmin = std::min(tmin, x.now_ns);
        switch (x.kind) {
        case GSIM_EV_DUPLICATE: ++want_peers; ++want_rec; break;
        case GSIM_EV_VALIDATE: case GSIM_EV_DELIVER: ++want_rec; break;
        case GSIM_EV_REJECT:
            if (x.arg >= GSIM_REJECT_VALIDATION_THROTTLED && x.arg <= GSIM_REJECT_VALIDATION_IGNORED) ++want_rec;
            break;
        default: break;
        }
        if (slots && x.kind >= GSIM_EV_DELIVER && x.kind <= GSIM_EV_PRUNE && (int64_t)x.peer < h->n &&
            (int32_t)x.topic < h->t && h->tp[x.topic].scored && !((h->smask[x.peer] >> x.topic) & 1ull)) {
            if (need.empty()) need.assign((size_t)h->n, 0);
            need[x.peer] |= 1ull << x.topic;
        }
    }
    int bits = 1;
    while (bits < 32 && (1ll << bits) <= h->n) ++bits;      // keys 0..N
    rc = tracer_scratch(h, n, bits);
    if (rc) return rc;

    TracerArgs a{};
    a.ev = t->d_ev; a.key = t->d_key2; a.idx = t->d_idx2; a.edge = t->d_edge; a.seg = t->d_seg;
    a.n = n; a.N = h->n; a.E = h->e;
    a.T = std::max(1, h->t); a.t_scored = h->t;
    a.tp = h->d_tp;
    a.row_ptr = h->d_row_ptr; a.col = h->d_col; a.rev = h->d_rev; a.owner = h->d_owner;
    a.sub = h->d_sub;
    a.bp = h->d_bp; a.estate = h->d_estate;
    a.rec = t->d_rec; a.mask = t->nslots - 1; a.pool = t->d_pool; a.pool_cap = (uint32_t)t->peers_cap;
    a.cnt = t->d_cnt; a.bad = t->d_bad; a.last = t->d_last; a.ttl = t->ttl;

    const uint32_t grid = (uint32_t)((n + 255) / 256);
    hipError_t e = hipMemcpyAsync(t->d_ev, ev, sizeof(gsim_score_event) * (size_t)n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_bad, 0xFF, sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->d_cnt + kCntErr, 0, 3 * sizeof(uint32_t), h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_score_tracer_events");
    {
        ProfScope ps(h, GSIM_K_TRACER_SORT);
        hipLaunchKernelGGL(k_tracer_keys, dim3(grid), dim3(256), 0, h->stream, (const gsim_score_event*)t->d_ev, n,
                           (uint32_t)h->n, t->d_key, t->d_idx);
        e = hipGetLastError();
        size_t bytes = t->tmp_bytes;
        if (e == hipSuccess)
            e = hipcub::DeviceRadixSort::SortPairs(t->d_tmp, bytes, (const uint32_t*)t->d_key, t->d_key2,
                                                   (const uint32_t*)t->d_idx, t->d_idx2, (int)n, 0, bits, h->stream);
    }
    if (e == hipSuccess) {
        ProfScope ps(h, GSIM_K_TRACER_RESOLVE);
        hipLaunchKernelGGL(k_tracer_resolve, dim3(grid), dim3(256), 0, h->stream, a);
        e = hipGetLastError();
    }
    unsigned long long bad = ~0ull;
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, t->d_bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);   // a bad batch fails before any change
    if (e != hipSuccess) return hip_check(h, e, "gsim_score_tracer_events");
    if (bad != ~0ull) {
        h->err = "event " + std::to_string(bad >> 8) + ": " + bad_text((uint32_t)(bad & 0xFF));
        return GSIM_EINVAL;
    }
    if (t->live + want_rec > t->records_cap) {
        h->err = "the batch could need " + std::to_string(want_rec) + " delivery records, " +
                 std::to_string(t->records_cap - t->live) + " are free (gsim_score_tracer_config, gsim_score_tracer_gc)";
        return GSIM_ERANGE;
    }
    if (t->pool_used + want_peers > t->peers_cap) {
        h->err = "the batch could need " + std::to_string(want_peers) + " peers-list entries, " +
                 std::to_string(t->peers_cap - t->pool_used) + " are free (gsim_score_tracer_config, gsim_score_tracer_gc)";
        return GSIM_ERANGE;
    }
    rc = deliver_flush(h);                       // pending first deliveries of a simulated round come first
    // Graft stores meshTime 0 under lazy meshTime only for a time at or after the refresh
    if (!rc && h->mt_lazy && tmin < h->mt_R) rc = materialize_mtime(h, true);
    if (!rc && !need.empty()) rc = ensure_slots(h, need.data());
    if (rc) return rc;
    // (ensure_slots re-lays the planes out: their addresses are read after it)
    a.smask = h->d_smask;
    a.first = h->d_first; a.meshd = h->d_meshd; a.fail = h->d_fail; a.invalid = h->d_invalid;
    a.mcnt = h->d_mcnt; a.graft = h->d_graft; a.mtime = h->d_mtime; a.tflags = h->d_tflags;
    a.inv_live = h->d_inv_live + (h->inv_par & 1);
    {
        ProfScope ps(h, GSIM_K_TRACER_APPLY);
        const int64_t segs = std::min<int64_t>(n, h->n);
        hipLaunchKernelGGL(k_tracer_apply, dim3((uint32_t)std::min<int64_t>((segs + 255) / 256, 65536)), dim3(256), 0,
                           h->stream, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_check(h, e, "k_tracer_apply");
    uint32_t cnt[kCntWords];
    rc = tracer_read_counts(h, cnt);
    if (rc) return rc;
    if (cnt[kCntErr]) { h->err = "score tracer: the delivery record table overflowed"; return GSIM_ERANGE; }
    t->applied += n;
    t->settled += cnt[kCntSettled];
    return GSIM_OK;
}

int gsim_score_tracer_gc(gsim_handle* h, int64_t now_ns)
{
    int rc = tracer_enter(h, true);
    if (rc) return rc;
    ScoreTracer* t = h->st;
    uint32_t* ncnt = t->d_cnt + kCntWords;
    hipError_t e = hipSuccess;
    if (!t->d_rec2) e = hipMalloc((void**)&t->d_rec2, sizeof(DRec) * (size_t)t->nslots);
    if (e == hipSuccess && !t->d_pool2)
        e = hipMalloc((void**)&t->d_pool2, sizeof(PeerEnt) * (size_t)std::max<int64_t>(t->peers_cap, 1));
    DRec* nrec = t->d_rec2;
    PeerEnt* npool = t->d_pool2;
    if (e == hipSuccess) e = hipMemsetAsync(nrec, 0xFF, sizeof(DRec) * (size_t)t->nslots, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(ncnt, 0, sizeof(uint32_t) * kCntWords, h->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tracer_gc, dim3(std::min<uint32_t>((t->nslots + 255) / 256, 65536u)), dim3(256), 0,
                           h->stream, (const DRec*)t->d_rec, t->nslots, (const PeerEnt*)t->d_pool, nrec, npool,
                           (uint32_t)t->peers_cap, ncnt, now_ns);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    // the live table is replaced only once the rebuild has run
    if (e == hipSuccess)
        e = hipMemcpyAsync(t->d_cnt, ncnt, sizeof(uint32_t) * kCntWords, hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_score_tracer_gc");
    std::swap(t->d_rec, t->d_rec2);
    std::swap(t->d_pool, t->d_pool2);
    uint32_t cnt[kCntWords];
    rc = tracer_read_counts(h, cnt);
    if (rc) return rc;
    t->collected += cnt[kCntCollected];
    if (cnt[kCntErr]) { h->err = "score tracer: the rebuilt delivery record table overflowed"; return GSIM_ERANGE; }
    return GSIM_OK;
}

int gsim_score_tracer_settled(gsim_handle* h, int64_t* out2)
{
    int rc = tracer_enter(h, true);
    if (rc) return rc;
    if (!out2) return GSIM_EINVAL;
    out2[0] = h->st->settled;
    out2[1] = h->mcnt_dirty ? 1 : 0;
    return GSIM_OK;
}

int gsim_score_tracer_stats(gsim_handle* h, int64_t* out4)
{
    int rc = tracer_enter(h, true);
    if (rc) return rc;
    if (!out4) return GSIM_EINVAL;
    const ScoreTracer* t = h->st;
    out4[0] = t->live;
    out4[1] = t->live_peers;
    out4[2] = t->applied;
    out4[3] = t->collected;
    return GSIM_OK;
}

}  // extern "C"
