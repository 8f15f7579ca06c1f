// Score report (include/gsim.h gsim_score_report): the live score of every
// record decomposed into the reference's P1..P7 (score.go:265-342) -- ten
// parts per record: P1 P2 P3 P3b P4, the capped topic sum, P5 P6 P7 and the
// total -- as distributions per (observer class, subject class), with the
// dominant negative part per bin of the total and per-topic flag counts,
// under the engine's parameters or a caller's what-if set.  Reduced on the
// device in one read-only pass; no [T][E] view is built, no plane is written.
//
// k_score_report: one lane per record r in record order, mapped as
// k_refresh_score and k_net_score are (estate[r], owner[r], col[r], bp[r],
// p6[r] coalesced; the subject is the row owner, the observer col[r]; a shard
// skips the records of observers it does not own).  The topic loop reads the
// [S][E] planes at slot_idx_of(smask[owner[r]], t, E, r): a wave touches 64
// consecutive elements of each field.  A chunk of kChunk topics' fields is
// loaded before any is used (score_of_record's kScoreChunk); the invalid
// planes are skipped while *inv_live == 0.  Pending meshMessageDeliveries
// increments are applied in registers with the ENGINE's cap (tp_state), lazy
// meshTime is derived from the graft time (lazy_mtime); neither is stored.
// Topic parameters come through const_tp (scalar loads): a.tp is the engine's
// table or the what-if table uploaded into the report's own scratch.
//
// Reduction, k_net_score's scheme: a lane forms its keys -- per part (pair,
// bin | NaN), then (pair, bin of the total, cause) | retained -- a wave counts
// by ballot over the distinct keys present and its leader lanes add the
// popcounts to the block's LDS counters, sized to the live C^2 and T * C^2.  The
// eight topic flags: per topic one ballot per flag; lane l picks the ballot of
// flag l & 7 and counts in it the wave's lanes of class pair l >> 3 (kept per
// record batch), one LDS atomic on consecutive words for the wave.  min / max per
// (pair, part) are integer atomics on the order-preserving map of the f64 bits
// (f64_key, gsim_internal.h), issued only where a lane improves on the block's
// value.  The block flushes one global atomic per non-zero entry.  Every result
// is an integer count or a min / max: no dependence on scheduling.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch
// or spills (the histogram edges ride in the argument block and are re-read
// where they are used: passed as a second argument they stayed in 30 SGPRs
// across the loop and 30-37 SGPRs spilled to VGPR lanes); LDS is dynamic, 8 *
// 20 C^2 + 4 * 454 C^2 + 32 T C^2 bytes (2040 at T = 2 with one class, 64384 at
// T = 64 with four, the largest case, under a workgroup's 64 KB):
//   k_score_report<Dense, one class>   88 VGPRs, 82 SGPRs, 5 waves/SIMD
//   k_score_report<Dense, classes>     92 VGPRs, 93 SGPRs, 5 waves/SIMD
//   k_score_report<slots, one class>   92 VGPRs, 82 SGPRs, 5 waves/SIMD
//   k_score_report<slots, classes>     94 VGPRs, 93 SGPRs, 5 waves/SIMD
// Measured: C3 after the default bench's ticks, two classes, the whole
// call 10.8 ms over 18.2 GB (1.7 TB/s), 1.56x one k_refresh_score launch on the same
// state: the ten accumulators' arithmetic and the ballots and LDS atomics bound it, not HBM.
#include <algorithm>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "report_common.h"

namespace gsim {

// per class pair counters (u32 in LDS, u64 in global memory)
enum : int {
    kPartSlots = GSIM_SR_BINS + 1,                         // the bins, then NaN
    SP_CAUSE = GSIM_SR_PARTS * kPartSlots,                 // [GSIM_NET_SCORE_BINS][GSIM_SR_CAUSES]
    SP_RET = SP_CAUSE + GSIM_NET_SCORE_BINS * GSIM_SR_CAUSES,
    SP_CAPPED,
    kSP,                                                   // 454
};
constexpr int kTopicFlags = 8;                             // gsim_score_topic_row's counts, in its order
constexpr int kSrMaxPairs = GSIM_NET_CLASSES * GSIM_NET_CLASSES;
constexpr size_t kSrMaxWords =
    (size_t)kSrMaxPairs * kSP + (size_t)GSIM_MAX_TOPICS * kSrMaxPairs * kTopicFlags + (size_t)kSrMaxPairs * GSIM_SR_PARTS * 2;

struct ScoreReport {
    unsigned long long* d_acc = nullptr;                   // [kSrMaxWords] counters, topic flags, min / max keys
    gsim_topic_score_params* d_tp = nullptr;               // [T] what-if topic table
    int64_t tp_cap = 0;
};

struct SrArgs {
    const uint32_t *owner, *col;
    const uint8_t *estate, *cls, *tflags, *mcnt;
    const uint64_t* smask;
    const double *first, *meshd, *fail, *invalid, *bp, *p6, *p5;
    const int64_t *graft, *mtime;
    const gsim_topic_score_params* tp;                     // the parameters scored with
    const gsim_topic_score_params* tp_state;               // the engine's: the cap pending increments saw
    const uint32_t* inv_live;
    double topic_cap, w5, w6, bp_thr, w7;
    int64_t E, mt_R;
    int32_t T, C, sharded, mt_lazy;
    uint32_t olo, ohi;
    unsigned long long* acc;                               // [C^2 kSP] [T C^2 8] [C^2 10 2]
    ScoreEdges ed;                                          // the total's histogram edges, by value
};

namespace {

// Attribution builds (timing only, the rows are then incomplete): -DGSIM_SR_SKIP=1
// leaves out the topic flags' ballots, 2 the parts' and causes' key walks, 4 the
// min / max atomics
#ifndef GSIM_SR_SKIP
#define GSIM_SR_SKIP 0
#endif
constexpr int kSrBlock = 256;
#ifndef GSIM_SR_CHUNK
#define GSIM_SR_CHUNK 2
#endif
constexpr int kChunk = GSIM_SR_CHUNK;                      // topics whose record fields are loaded together

static_assert(sizeof(unsigned long long) * kSrMaxPairs * GSIM_SR_PARTS * 2 + sizeof(uint32_t) * kSrMaxPairs * kSP +
                      sizeof(uint32_t) * GSIM_MAX_TOPICS * kSrMaxPairs * kTopicFlags <= 65536,
              "the block's counters fit a workgroup's LDS at 64 topics and 4 classes");

// The fixed signed-log bin of a non-NaN value (include/gsim.h): integer
// arithmetic on the f64 bits.
__device__ __forceinline__ uint32_t sr_bin(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    const unsigned long long mag = u & 0x7FFFFFFFFFFFFFFFull;
    if (mag == 0) return 16u;
    const int k = (int)(mag >> 52) - 1023;                 // (a denormal reads -1023: below every edge all the same)
    int m = (k + 8) >> 1;
    m = m < 0 ? 0 : (m > 15 ? 15 : m);
    return (u >> 63) ? (uint32_t)(15 - m) : (uint32_t)(17 + m);
}

template <bool Dense, bool CLS>
__global__ __launch_bounds__(kSrBlock) void k_score_report(SrArgs a_)
{
    extern __shared__ unsigned long long s_mm[];           // [C^2][10][2]: max of ~key, max of key
    const int npairs = a_.C * a_.C, T = a_.T;
    const int n_mm = npairs * GSIM_SR_PARTS * 2, n_cnt = npairs * kSP, n_top = T * npairs * kTopicFlags;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_mm + n_mm);
    uint32_t* s_top = s_cnt + n_cnt;
    for (int q = threadIdx.x; q < n_mm; q += kSrBlock) s_mm[q] = 0ull;
    for (int q = threadIdx.x; q < n_cnt + n_top; q += kSrBlock) s_cnt[q] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kSrBlock;
    for (int64_t r0 = (int64_t)blockIdx.x * kSrBlock; r0 < a_.E; r0 += stride) {    // block-uniform
        const SrArgs& a = kernarg0(a_);                    // (re-read per batch: SGPR pressure)
        const int64_t r = r0 + threadIdx.x;
        const bool valid = r < a.E;
        uint8_t st = valid ? a.estate[r] : (uint8_t)0;
        const uint32_t obs = valid ? a.col[r] : 0u, subj = valid ? a.owner[r] : 0u;
        if (a.sharded && (obs < a.olo || obs >= a.ohi)) st = 0;   // another shard's record
        const bool conn = (st & GSIM_ES_CONNECTED) != 0;
        const bool ret = !conn && (st & GSIM_ES_TRACKED) != 0;
        const bool sc = conn && (st & GSIM_ES_TRACKED) != 0;      // has peerStats: its counters are read
        uint32_t pair = 0;
        if (CLS && valid) pair = (uint32_t)a.cls[obs] * (uint32_t)a.C + (uint32_t)a.cls[subj];
        // the per-record values leave with the first topics' fields
        const double bpv = sc ? a.bp[r] : 0.0, p6v = sc ? a.p6[r] : 0.0, p5v = sc ? a.p5[subj] : 0.0;
        const uint64_t mj = Dense ? ~0ull : (sc ? a.smask[subj] : 0ull);
        const bool inv_zero = a.inv_live && !*a.inv_live;   // no record holds an invalid delivery
        // the topic flags' lanes: lane l counts flag l & 7 of class pair l >> 3 (pairs 8..15
        // in a second word), so it keeps the wave's lanes of that pair
        uint64_t pmask0 = 0, pmask1 = 0;
        if (CLS) {
            walk_keys(conn, pair, [&](uint32_t k, uint64_t same, int) {   // the distinct pairs present
                if ((uint32_t)(lane >> 3) == (k & 7u)) {
                    if (k < 8u) pmask0 = same; else pmask1 = same;
                }
            });
        } else {
            const uint64_t all = __ballot(conn);
            if (lane < kTopicFlags) pmask0 = all;
        }

        double part[GSIM_SR_PARTS];
#pragma unroll
        for (int k = 0; k < GSIM_SR_PARTS; ++k) part[k] = 0.0;
        for (int32_t t0 = 0; t0 < T; t0 += kChunk) {       // wave-uniform: every lane walks every topic
            uint8_t fl[kChunk], mc[kChunk];
            double f[kChunk], md[kChunk], fa[kChunk], iv[kChunk];
            int64_t mt[kChunk];
            bool ok[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int32_t t = t0 + j;
                ok[j] = sc && t < T && (const_tp(a.tp) + t)->scored && slot_has_of<Dense>(mj, t);
                const int64_t i = slot_idx_of<Dense>(mj, t, a.E, r);
                fl[j] = ok[j] ? a.tflags[i] : (uint8_t)0;
                mc[j] = ok[j] ? a.mcnt[i] : (uint8_t)0;
                f[j] = ok[j] ? a.first[i] : 0.0;
                md[j] = ok[j] ? a.meshd[i] : 0.0;
                fa[j] = ok[j] ? a.fail[i] : 0.0;
                iv[j] = ok[j] && !inv_zero ? a.invalid[i] : 0.0;
                mt[j] = ok[j] ? (a.mt_lazy ? a.graft[i] : a.mtime[i]) : 0;
            }
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int32_t t = t0 + j;
                if (t >= T) break;
                const ctp_t tp = const_tp(a.tp) + t;
                if (!tp->scored) continue;                 // wave-uniform: its rows stay zero
                // (a record of a topic its subject holds no slot for reads as zeros, as in the ABI's view)
                const double meshd = apply_incs(md[j], mc[j], (const_tp(a.tp_state) + t)->mesh_message_deliveries_cap);
                const bool inm = (fl[j] & GSIM_TF_IN_MESH) != 0;
                int64_t mtv = mt[j];
                if (inm && a.mt_lazy)                      // lazy_mtime: the stored value where the Graft is newer
                    mtv = mtv <= a.mt_R ? a.mt_R - mtv : a.mtime[slot_idx_of<Dense>(mj, t, a.E, r)];
                double p1 = 0.0;
                if (inm && tp->time_in_mesh_quantum_ns != 0) p1 = (double)go_div(mtv, tp->time_in_mesh_quantum_ns);
                const bool p1cap = p1 > tp->time_in_mesh_cap;
                if (p1cap) p1 = tp->time_in_mesh_cap;
                p1 = inm ? p1 * tp->time_in_mesh_weight : 0.0;
                const double p2 = f[j] * tp->first_message_deliveries_weight;
                const bool actv = (fl[j] & GSIM_TF_ACTIVE) != 0;
                const bool def = actv && meshd < tp->mesh_message_deliveries_threshold;
                double p3 = 0.0;
                if (def) {
                    const double deficit = tp->mesh_message_deliveries_threshold - meshd;
                    p3 = (deficit * deficit) * tp->mesh_message_deliveries_weight;
                }
                const double p3b = fa[j] * tp->mesh_failure_penalty_weight;
                const double p4 = (iv[j] * iv[j]) * tp->invalid_message_deliveries_weight;
                const double ts = ((((0.0 + p1) + p2) + p3) + p3b) + p4;
                const double tw = tp->topic_weight, tsw = ts * tw;
                part[GSIM_SR_P1] += p1 * tw;
                part[GSIM_SR_P2] += p2 * tw;
                part[GSIM_SR_P3] += p3 * tw;
                part[GSIM_SR_P3B] += p3b * tw;
                part[GSIM_SR_P4] += p4 * tw;
                part[GSIM_SR_TOPICS] += tsw;
                uint32_t fb = (inm ? 1u : 0u) | (inm && p1cap ? 2u : 0u) |
                              (f[j] >= tp->first_message_deliveries_cap ? 4u : 0u) | (actv ? 8u : 0u) | (def ? 16u : 0u) |
                              (fa[j] != 0.0 ? 32u : 0u) | (iv[j] != 0.0 ? 64u : 0u) | (tsw < 0.0 ? 128u : 0u);
                if (!sc) fb = 0;
                if ((GSIM_SR_SKIP & 1) || !__ballot(fb != 0)) continue;   // wave-uniform
                // one ballot per flag, whatever the number of pairs: lane l picks its flag's
                // ballot and counts its pair's lanes in it; the counters of topic t are
                // [pair][flag], so the wave's adds are one LDS atomic on consecutive words
                uint64_t mb = 0;
#pragma unroll
                for (int b = 0; b < kTopicFlags; ++b) {
                    const uint64_t m = __ballot((fb >> b) & 1u);
                    if ((lane & 7) == b) mb = m;
                }
                uint32_t* top = s_top + (int)t * npairs * kTopicFlags;
                const uint32_t v0 = (uint32_t)__popcll(mb & pmask0);
                if (v0) atomicAdd(&top[lane], v0);
                if (CLS && npairs > 8) {
                    const uint32_t v1 = (uint32_t)__popcll(mb & pmask1);
                    if (v1) atomicAdd(&top[64 + lane], v1);
                }
            }
        }
        bool capped = false;
        if (a.topic_cap > 0 && part[GSIM_SR_TOPICS] > a.topic_cap) {
            part[GSIM_SR_TOPICS] = a.topic_cap;
            capped = sc;
        }
        part[GSIM_SR_P5] = sc ? p5v * a.w5 : 0.0;
        part[GSIM_SR_P6] = sc ? p6v * a.w6 : 0.0;
        if (sc && bpv > a.bp_thr) {
            const double excess = bpv - a.bp_thr;
            part[GSIM_SR_P7] = (excess * excess) * a.w7;
        }
        const double total = ((part[GSIM_SR_TOPICS] + part[GSIM_SR_P5]) + part[GSIM_SR_P6]) + part[GSIM_SR_P7];
        part[GSIM_SR_TOTAL] = total;

        // per part: (pair, bin | NaN), min / max
#pragma unroll
        for (int k = 0; k < GSIM_SR_PARTS; ++k) {
            const double v = part[k];
            const bool isn = v != v;
            if (!(GSIM_SR_SKIP & 2))
                count_keys(s_cnt, conn, pair * kSP + (uint32_t)k * kPartSlots + (isn ? (uint32_t)GSIM_SR_BINS : sr_bin(v)), lane);
            if (!(GSIM_SR_SKIP & 4) && conn && !isn) {
                const unsigned long long kk = f64_key(v);
                const int q = ((int)pair * GSIM_SR_PARTS + k) * 2;
                volatile unsigned long long* mm = s_mm + q;
                if (~kk > mm[0]) atomicMax(&s_mm[q], ~kk);
                if (kk > mm[1]) atomicMax(&s_mm[q + 1], kk);
            }
        }
        // (pair, bin of the total on the caller's edges, dominant negative part) | retained
        const int cidx[GSIM_SR_CAUSES - 1] = {GSIM_SR_P3, GSIM_SR_P3B, GSIM_SR_P4, GSIM_SR_P5, GSIM_SR_P6, GSIM_SR_P7};
        uint32_t cause = GSIM_SR_CAUSES - 1;               // NONE
        double worst = 0.0;
#pragma unroll
        for (int c = 0; c < GSIM_SR_CAUSES - 1; ++c) {
            const double v = part[cidx[c]];
            if (v < worst) { worst = v; cause = (uint32_t)c; }   // (NaN never; a tie keeps the earlier part)
        }
        uint32_t bin = 0;
#pragma unroll
        for (int k = 0; k < GSIM_NET_SCORE_BINS - 1; ++k) bin += (k < a.ed.n && total >= a.ed.v[k]) ? 1u : 0u;
        const bool tot_ok = conn && total == total;
        count_keys(s_cnt, tot_ok || ret,
                   pair * kSP + (ret ? (uint32_t)SP_RET : (uint32_t)SP_CAUSE + bin * GSIM_SR_CAUSES + cause), lane);
        count_keys(s_cnt, capped, pair * kSP + (uint32_t)SP_CAPPED, lane);
    }
    __syncthreads();
    const SrArgs& a = kernarg0(a_);
    for (int q = threadIdx.x; q < n_cnt + n_top; q += kSrBlock) {
        const uint32_t v = s_cnt[q];
        if (v) atomicAdd(&a.acc[q], (unsigned long long)v);
    }
    for (int q = threadIdx.x; q < n_mm; q += kSrBlock) {
        const unsigned long long v = s_mm[q];
        if (v) atomicMax(&a.acc[n_cnt + n_top + q], v);
    }
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void scorereport_release(gsim_handle* h)
{
    if (!h->sr) return;
    free_all({h->sr->d_acc, h->sr->d_tp});
    delete h->sr;
    h->sr = nullptr;
}

extern "C" {

int gsim_score_report(gsim_handle* h, const struct gsim_score_what_if* what_if, const double* edges, int32_t n_edges,
                      struct gsim_score_part_row* parts, int64_t part_cap, int64_t* n_parts,
                      struct gsim_score_cause_row* causes, int64_t cause_cap, int64_t* n_causes,
                      struct gsim_score_topic_row* topics, int64_t topic_cap, int64_t* n_topics)
{
    if (!h || !n_parts || !n_causes || !n_topics || part_cap < 0 || cause_cap < 0 || topic_cap < 0) return GSIM_EINVAL;
    const uint8_t* d_cls = nullptr;
    const int C = netreport_classes(h, &d_cls);
    const int T = h->t;
    const int npairs = C * C;
    const int64_t np = (int64_t)npairs * GSIM_SR_PARTS, nc = npairs, nt = (int64_t)T * npairs;
    *n_parts = np;
    *n_causes = nc;
    *n_topics = nt;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    if (h->e == 0 && h->n == 0) { h->err = "no graph loaded (call gsim_load_graph first)"; return GSIM_ESTATE; }
    ScoreEdges ed{};
    if (int rc = score_edges(h, "gsim_score_report", edges, n_edges, &ed)) return rc;
    // what-if parameters: validated as the engine's own were
    const gsim_peer_score_params* pp = &h->pp;
    const gsim_topic_score_params* wtp = nullptr;
    if (what_if) {
        if (what_if->topics && what_if->n_topics != T) {
            h->err = "gsim_score_report: the what-if topic table must hold one entry per topic";
            return GSIM_EINVAL;
        }
        wtp = what_if->topics;
        if (what_if->peer) pp = what_if->peer;
        char buf[256] = {0};
        // (a handle of gsim_create_unvalidated takes what-if sets unvalidated too, as its own parameters)
        if (h->validate && what_if->peer &&
            gsim_validate_peer_params(pp, wtp ? wtp : h->tp.data(), T, buf, sizeof buf)) {
            h->err = buf;
            return GSIM_EINVAL;
        }
        if (h->validate && wtp && !what_if->peer)
            for (int t = 0; t < T; ++t)
                if (wtp[t].scored && gsim_validate_topic_params(&wtp[t], buf, sizeof buf)) {
                    h->err = buf;
                    return GSIM_EINVAL;
                }
    }
    const bool want_parts = parts && part_cap > 0, want_causes = causes && cause_cap > 0, want_topics = topics && topic_cap > 0;
    if ((want_parts && part_cap < np) || (want_causes && cause_cap < nc) || (want_topics && topic_cap < nt)) {
        h->err = "gsim_score_report: output buffer too small";
        return GSIM_ERANGE;
    }
    if (!want_parts && !want_causes && !want_topics) return GSIM_OK;

    int rc = deliver_flush(h);                     // pending first deliveries are P2 credits
    if (rc) return rc;
    if (!h->sr) h->sr = new ScoreReport;
    ScoreReport* s = h->sr;
    rc = alloc_once(h, "report", &s->d_acc, (int64_t)kSrMaxWords);
    if (!rc && wtp) rc = grow(h, "report", &s->d_tp, &s->tp_cap, (int64_t)T);
    if (rc) return rc;
    const size_t n_cnt = (size_t)npairs * kSP, n_top = (size_t)nt * kTopicFlags, n_mm = (size_t)np * 2;
    const size_t words = n_cnt + n_top + n_mm;
    hipError_t e = hipMemsetAsync(s->d_acc, 0, sizeof(unsigned long long) * words, h->stream);
    // (the engine's d_tp is never written: the what-if table has its own)
    if (e == hipSuccess && wtp)
        e = hipMemcpyAsync(s->d_tp, wtp, sizeof(gsim_topic_score_params) * (size_t)T, hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_score_report");

    SrArgs a{};
    a.owner = h->d_owner; a.col = h->d_col;
    a.estate = h->d_estate; a.cls = C > 1 ? d_cls : nullptr; a.tflags = h->d_tflags; a.mcnt = h->d_mcnt;
    a.smask = h->d_smask;
    a.first = h->d_first; a.meshd = h->d_meshd; a.fail = h->d_fail; a.invalid = h->d_invalid;
    a.bp = h->d_bp; a.p6 = h->d_p6; a.p5 = h->d_p5;
    a.graft = h->d_graft; a.mtime = h->d_mtime;
    a.tp = wtp ? s->d_tp : h->d_tp;
    a.tp_state = h->d_tp;
    a.inv_live = h->d_inv_live ? h->d_inv_live + (h->inv_par & 1) : nullptr;
    a.topic_cap = pp->topic_score_cap; a.w5 = pp->app_specific_weight; a.w6 = pp->ip_colocation_factor_weight;
    a.bp_thr = pp->behaviour_penalty_threshold; a.w7 = pp->behaviour_penalty_weight;
    a.E = h->e; a.mt_R = h->mt_R;
    a.T = T; a.C = C;
    a.sharded = h->sh ? 1 : 0;
    a.mt_lazy = h->mt_lazy ? 1 : 0;
    a.olo = (uint32_t)h->olo(); a.ohi = (uint32_t)h->ohi();
    a.acc = s->d_acc;
    a.ed = ed;
    if (h->e > 0) {
        const size_t lds = sizeof(unsigned long long) * n_mm + sizeof(uint32_t) * (n_cnt + n_top);
        const dim3 grid((uint32_t)std::max<int64_t>(1, std::min<int64_t>((h->e + 4 * kSrBlock - 1) / (4 * kSrBlock), 2048)));
        const bool cls_on = a.cls != nullptr;
        if (h->d_smask) {
            if (cls_on) hipLaunchKernelGGL((k_score_report<false, true>), grid, dim3(kSrBlock), lds, h->stream, a);
            else hipLaunchKernelGGL((k_score_report<false, false>), grid, dim3(kSrBlock), lds, h->stream, a);
        } else {
            if (cls_on) hipLaunchKernelGGL((k_score_report<true, true>), grid, dim3(kSrBlock), lds, h->stream, a);
            else hipLaunchKernelGGL((k_score_report<true, false>), grid, dim3(kSrBlock), lds, h->stream, a);
        }
    }
    std::vector<unsigned long long> acc(words);
    e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(acc.data(), s->d_acc, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_score_report");

    const double inf = std::numeric_limits<double>::infinity();
    const unsigned long long* mm = acc.data() + n_cnt + n_top;
    if (want_parts)
        for (int64_t q = 0; q < np; ++q) {
            const int pair = (int)(q / GSIM_SR_PARTS), k = (int)(q % GSIM_SR_PARTS);
            const unsigned long long* c = acc.data() + (size_t)pair * kSP + (size_t)k * kPartSlots;
            gsim_score_part_row x{};
            x.obs_cls = (uint32_t)(pair / C);
            x.subj_cls = (uint32_t)(pair % C);
            x.part = (uint32_t)k;
            uint64_t inb = 0;
            for (int b = 0; b < GSIM_SR_BINS; ++b) { x.hist[b] = c[b]; inb += c[b]; }
            x.nan = c[GSIM_SR_BINS];
            x.min = inb ? key_f64(~mm[q * 2]) : inf;
            x.max = inb ? key_f64(mm[q * 2 + 1]) : -inf;
            parts[q] = x;
        }
    if (want_causes)
        for (int64_t q = 0; q < nc; ++q) {
            const unsigned long long* c = acc.data() + (size_t)q * kSP;
            gsim_score_cause_row x{};
            x.obs_cls = (uint32_t)(q / C);
            x.subj_cls = (uint32_t)(q % C);
            uint64_t inb = 0;
            for (int b = 0; b < GSIM_NET_SCORE_BINS; ++b)
                for (int k = 0; k < GSIM_SR_CAUSES; ++k) {
                    x.cause[b][k] = c[SP_CAUSE + b * GSIM_SR_CAUSES + k];
                    inb += x.cause[b][k];
                }
            x.nan = c[GSIM_SR_TOTAL * kPartSlots + GSIM_SR_BINS];
            x.connected = inb + x.nan;
            x.retained = c[SP_RET];
            x.capped = c[SP_CAPPED];
            causes[q] = x;
        }
    if (want_topics)
        for (int64_t q = 0; q < nt; ++q) {
            const unsigned long long* c = acc.data() + n_cnt + (size_t)q * kTopicFlags;
            const int pair = (int)(q % npairs);
            gsim_score_topic_row x{};
            x.topic = (uint32_t)(q / npairs);
            x.obs_cls = (uint32_t)(pair / C);
            x.subj_cls = (uint32_t)(pair % C);
            x.in_mesh = c[0]; x.p1_capped = c[1]; x.first_at_cap = c[2]; x.active = c[3];
            x.p3_deficit = c[4]; x.p3b_nonzero = c[5]; x.p4_nonzero = c[6]; x.negative = c[7];
            topics[q] = x;
        }
    return GSIM_OK;
}

}  // extern "C"
