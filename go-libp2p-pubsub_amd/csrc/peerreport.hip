// Peer delivery report (include/gsim.h gsim_peer_report): the propagation
// report (report.hip) transposed.  The same seen-set cells, streamed once, 8
// bytes each, reduced per peer and per (topic, class of the receiving peer):
// messages expected / received / missed, latencies, and the first deliveries
// by the class of the first sender, the low word of the committed cell.  The
// reference has no such read-out; what is counted is DeliverMessage's reach
// (score.go:702-726) as one router sees it, and whom it got each message from
// first (markFirstMessageDelivery's peer, score.go:919-946).
//
// Launches per call (none per slot or per peer, no host loop over either):
//   k_select<PrFill>  one block: the slots published in [round_lo, round_hi),
//                   the reports' shared selection (report_common.h), compacted in
//                   slot order with what the walk needs of each (cell base and
//                   count, publication round, topic, origin), and the selected
//                   messages per topic
//   k_peer_reduce   a lane owns a peer, a wave the 64 peers of one word of the
//                   member bitmaps, and walks the selected slots: 512 contiguous
//                   bytes per slot on the dense ring; on a member-compacted topic
//                   the run cbase[m] + mpre[t][w] + rank within mbits[t][w], the
//                   word and its prefix loaded once per topic (a sub-ring's slots
//                   are contiguous) and reused for all its slots.  kPrBatch slots'
//                   cells are in flight per lane, then their senders' class bytes
//                   (a gather, only with more than one class).
// Per-peer sums live in the lane's registers and are stored once.  Class rows:
// within a slot the topic is wave-uniform, so the wave walks the distinct
// (class, latency) and (class, sender class) keys present (__ballot of the lanes
// holding the leader's key, __popcll) and the leader adds the count to the
// block's LDS counters, sized to the live T * C (168 bytes per (topic, class):
// 43 KB at 64 x 4), flushed with one global atomic per non-zero entry.  Only
// the overflow bin adds its exact latencies to the row's sum and maximum in the
// walk; for the exact bins both follow from the histogram at the flush.
//
// Few peers and a large ring would leave the device idle with a grid over peers
// alone: with fewer peer waves than kPrFullWaves the selected slots are split
// over gridDim.y (pr_launch, a function of the owned peers walked and the
// selected messages) and the parts' per-peer sums meet in atomicAdd / atomicMax
// on the zeroed rows.  Everything is an integer: no dependence on order.
//
// A shard walks the peers it owns.  Their committed cells hold a local id of the
// first sender (owned or ghost: every claim writes owner[r], the local row owner
// of the receiver's record, in k_send_tm, listed_copy and k_xbits_deliver's fast
// path, and commit_claim keeps it; k_frontier_import and the bitmap import write
// ghosts' cells only, which no report counts), the origin's cell its own id.
// The class array covers ghosts (gsim_group_set_peer_classes).  A sender id
// that is no local peer sets a flag and the call returns GSIM_ESTATE.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch
// (LDS of k_peer_reduce: dynamic only, 168 bytes per live (topic, class)):
//   k_peer_reduce<false>  38 VGPRs, 94 SGPRs, no spills, 8 waves/SIMD
//   k_peer_reduce<true>   49 VGPRs, 106 SGPRs, 36 of them kept in lanes of one VGPR
//                         (kernel arguments), no VGPR spills, 7 waves/SIMD
//   k_select<PrFill>      28 VGPRs, 53 SGPRs, 324 bytes of LDS, 8 waves/SIMD
// Measured: C3 after the default bench's ticks, 1477 messages,
// 11.8 GB of cells: the per-peer rows alone 3.13 ms, both halves 6.56 ms with one
// class and 14.0 ms with two, against 2.20 ms for gsim_msg_report on the same
// state (ratios 1.4, 3.0, 6.3).  The class rows are bound by instruction issue
// (an LDS atomic per (slot, distinct key)), the two-class case by the gather.
#include <algorithm>
#include <cstring>
#include <vector>

#include "report_common.h"

namespace gsim {

using PrMsg = SelMsg;   // one selected message as the walk reads it (report_common.h)

// per (topic, class) counters: u32 words in LDS, u64 in global memory, the same index
enum : int {
    PL_LSUM = 0,        // u64 in LDS too (words 0-1); in LDS the overflow bin's part, the rest follows from hist
    PL_LMAX = 2,        // (likewise)
    PL_OWN,
    PL_STRAY,           // received cells of peers not announcing the topic
    PL_PEERS,
    PL_FF,              // [GSIM_NET_CLASSES]
    PL_HIST = PL_FF + GSIM_NET_CLASSES,
    kPL = PL_HIST + GSIM_REPORT_BINS,          // 42: every row starts 8-byte aligned
};
static_assert(kPL % 2 == 0, "the u64 latency sum of every LDS row must stay 8-byte aligned");
constexpr size_t kPrAcc = (size_t)GSIM_MAX_TOPICS * GSIM_NET_CLASSES * kPL;
enum : int { PC_NSEL = 0, PC_BAD, PC_TOPIC, kPC = PC_TOPIC + GSIM_MAX_TOPICS };

struct PeerReport {
    PrMsg* d_sel = nullptr;                    // [ring] the selected messages, slot order
    uint32_t* d_cnt = nullptr;                 // [kPC] selected, bad-sender flag, messages per topic
    unsigned long long* d_acc = nullptr;       // [kPrAcc]
    gsim_peer_row* d_rows = nullptr;           // [rows_cap]
    int64_t rows_cap = 0;
    int64_t ring = 0;
    int64_t last[3] = {0, 0, 0};               // gsim_peer_report_launch
};

struct PeerArgs {
    Cells cells;
    const PrMsg* sel;
    int64_t nsel, per;                         // selected messages; slots per part
    const uint64_t* sub;
    const uint8_t* cls;
    int32_t T, C;
    int64_t n;                                 // local peers (a first sender is one of them)
    int64_t w0;                                // first bitmap word walked
    int64_t qlo, qhi;                          // peers walked
    int64_t olo, ohi;                          // peers whose rows are written, rows[p - olo]
    gsim_peer_row* rows;
    unsigned long long* acc;                   // class counters (nullptr: the per-peer half alone)
    uint32_t* bad;
};

namespace {

constexpr int kPrBlock = 256;                  // 4 waves, 256 consecutive peers
constexpr int kPrBatch = 4;                    // slots whose cells a lane has in flight
constexpr int64_t kPrFullWaves = 256;          // one wave per CU: from here on peers alone fill the device
constexpr int64_t kPrTargetWaves = 2048;       // what a split grid aims at
constexpr int64_t kPrMinSlots = 2 * kPrBatch;  // a part walks at least two batches

// The selected slot's row (k_select, report_common.h).
struct PrFill {
    using Row = PrMsg;
    __device__ static uint32_t fill(Row& r, const ReportView& v, int m, int64_t pub)
    {
        PrMsg x;
        fill_sel(x, v, m, pub);
        r = x;
        return x.topic;
    }
};
static_assert(PC_NSEL == 0 && PC_BAD < PC_TOPIC, "k_select<PrFill, PC_TOPIC> writes the count and clears the flag");

template <bool CLS>
__global__ __launch_bounds__(kPrBlock) void k_peer_reduce(PeerArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_acc[];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool classes = a.acc != nullptr;
    const int nacc = classes ? a.T * a.C * kPL : 0;
    for (int q = tid; q < nacc; q += kPrBlock) s_acc[q] = 0;
    __syncthreads();

    const int64_t word = a.w0 + (int64_t)blockIdx.x * (kPrBlock / 64) + (tid >> 6);   // wave-uniform
    const int64_t p = word * 64 + lane;
    const bool active = p >= a.qlo && p < a.qhi;
    const bool wave_on = word * 64 < a.qhi;                    // (the grid's last block may hold idle waves)
    const uint64_t sub = active ? a.sub[p] : 0ull;
    const uint32_t mycls = CLS && active ? a.cls[p] : 0u;

    if (classes && blockIdx.y == 0) {                          // peers of each class announcing each topic
        for (int32_t t = 0; t < a.T; ++t) {
            // the classes present
            lead_keys((sub >> t) & 1ull, mycls, lane,
                      [&](uint32_t cl, uint32_t cnt) { atomicAdd(&s_acc[(t * a.C + (int)cl) * kPL + PL_PEERS], cnt); });
        }
    }

    uint32_t exp = 0, rec = 0, own = 0, rsub = 0, lmax = 0, ff0 = 0, ff1 = 0, ff2 = 0, ff3 = 0;
    uint64_t lsum = 0;
    bool bad = false;
    // the member word of the topic last walked (a member-compacted topic's slots are contiguous)
    int32_t wt = -1;
    uint64_t wbits = 0;
    int64_t wpre = 0;
    const int64_t klo = (int64_t)blockIdx.y * a.per;
    const int64_t khi = klo + a.per < a.nsel ? klo + a.per : a.nsel;
    for (int64_t k0 = klo; k0 < khi; k0 += kPrBatch) {         // block-uniform
        PrMsg mm[kPrBatch];
        uint64_t c[kPrBatch];
#pragma unroll
        for (int u = 0; u < kPrBatch; ++u) {                   // the batch's cells: independent loads
            const bool on = k0 + u < khi;
            mm[u] = a.sel[on ? k0 + u : khi - 1];
            const int32_t t = (int32_t)mm[u].topic;
            bool has = true;
            int64_t idx = p;
            if ((a.cells.sparse >> t) & 1ull) {                // wave-uniform
                if (t != wt) {
                    wt = t;
                    wbits = 0;
                    wpre = 0;
                    if (wave_on) a.cells.word(t, word, wbits, wpre);
                }
                member_rank(wbits, wpre, lane, has, idx);
            }
            c[u] = kUnseen64;
            if (on && active && has && idx < (int64_t)mm[u].len) c[u] = a.cells.cell[(int64_t)mm[u].base + idx];
        }
        uint32_t sc[kPrBatch];
#pragma unroll
        for (int u = 0; u < kPrBatch; ++u) {                   // the first senders' classes, gathered together
            sc[u] = 0;
            if (CLS) {
                const uint32_t hi = (uint32_t)(c[u] >> 32), from = (uint32_t)c[u] & kPeerMask;
                if (!(hi & kClaim) && (uint32_t)p != mm[u].origin) {
                    if ((int64_t)from < a.n) sc[u] = a.cls[from];
                    else bad = true;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kPrBatch; ++u) {
            if (k0 + u >= khi) break;                          // block-uniform
            const int32_t t = (int32_t)mm[u].topic;
            const uint32_t hi = (uint32_t)(c[u] >> 32);
            const bool ok = !(hi & kClaim);                    // committed (unseen reads all ones, a claim has kClaim)
            const uint32_t d = hi - mm[u].pub;
            const bool mine = ok && (uint32_t)p == mm[u].origin;
            const bool other = ok && !mine;
            const bool sb = (sub >> t) & 1ull;                 // (an inactive lane's sub is 0)
            exp += sb;
            rec += ok;
            own += mine;
            rsub += ok && sb;
            lsum += ok ? d : 0u;
            lmax = ok && d > lmax ? d : lmax;
            ff0 += other && sc[u] == 0;
            ff1 += other && sc[u] == 1;
            ff2 += other && sc[u] == 2;
            ff3 += other && sc[u] == 3;
            if (!classes || t >= a.T) continue;
            uint32_t* trow = s_acc + t * a.C * kPL;            // the topic's rows, one per class
            // (the three walks below stay written out: through lead_keys the one-class kernel
            // measured 2.8 % slower than before, outside the spread of repeated runs)
            uint64_t todo = __ballot(ok);
            while (todo) {                                     // wave-uniform: the distinct (class, latency) present
                const int lead = __builtin_ctzll(todo);
                const uint32_t dl = (uint32_t)__builtin_amdgcn_readlane((int)d, lead);
                const uint32_t cl = CLS ? (uint32_t)__builtin_amdgcn_readlane((int)mycls, lead) : 0u;
                const uint64_t same = __ballot(ok && d == dl && mycls == cl);
                if (lane == lead) {
                    uint32_t* r = trow + cl * kPL;
                    const uint32_t cnt = (uint32_t)__popcll(same);
                    atomicAdd(&r[PL_HIST + (dl < GSIM_REPORT_BINS - 1 ? dl : GSIM_REPORT_BINS - 1)], cnt);
                    if (dl >= GSIM_REPORT_BINS - 1) {           // the overflow bin alone needs its exact latencies
                        atomicAdd(reinterpret_cast<unsigned long long*>(&r[PL_LSUM]), (unsigned long long)dl * cnt);
                        atomicMax(&r[PL_LMAX], dl);
                    }
                }
                todo &= ~same;
            }
            const uint32_t fkey = mycls * GSIM_NET_CLASSES + sc[u];
            todo = __ballot(other);
            while (todo) {                                     // the distinct (class, sender class) present
                const int lead = __builtin_ctzll(todo);
                const uint32_t kl = CLS ? (uint32_t)__builtin_amdgcn_readlane((int)fkey, lead) : 0u;
                const uint64_t same = __ballot(other && fkey == kl);
                if (lane == lead)
                    atomicAdd(&trow[(kl / GSIM_NET_CLASSES) * kPL + PL_FF + kl % GSIM_NET_CLASSES], (uint32_t)__popcll(same));
                todo &= ~same;
            }
            if (mine) atomicAdd(&trow[mycls * kPL + PL_OWN], 1u);   // at most one lane of the whole grid per slot
            todo = __ballot(ok && !sb);                        // rare: a fanout publisher, a peer that left
            while (todo) {
                const int lead = __builtin_ctzll(todo);
                const uint32_t cl = CLS ? (uint32_t)__builtin_amdgcn_readlane((int)mycls, lead) : 0u;
                const uint64_t same = __ballot(ok && !sb && mycls == cl);
                if (lane == lead) atomicAdd(&trow[cl * kPL + PL_STRAY], (uint32_t)__popcll(same));
                todo &= ~same;
            }
        }
    }
    if (bad) *a.bad = 1u;

    if (a.rows && p >= a.olo && p < a.ohi) {
        gsim_peer_row* row = a.rows + (p - a.olo);
        if (gridDim.y == 1) {
            gsim_peer_row x;
            x.expected = exp; x.received = rec; x.own = own; x.missed = exp - rsub;
            x.lat_max = lmax; x._pad = 0; x.lat_sum = lsum;
            x.first_from[0] = ff0; x.first_from[1] = ff1; x.first_from[2] = ff2; x.first_from[3] = ff3;
            *row = x;
        } else {                                               // the parts' sums meet on the zeroed row
            if (exp) atomicAdd(&row->expected, exp);
            if (rec) atomicAdd(&row->received, rec);
            if (own) atomicAdd(&row->own, own);
            if (exp - rsub) atomicAdd(&row->missed, exp - rsub);
            if (lmax) atomicMax(&row->lat_max, lmax);
            if (lsum) atomicAdd(reinterpret_cast<unsigned long long*>(&row->lat_sum), (unsigned long long)lsum);
            if (ff0) atomicAdd(&row->first_from[0], ff0);
            if (ff1) atomicAdd(&row->first_from[1], ff1);
            if (ff2) atomicAdd(&row->first_from[2], ff2);
            if (ff3) atomicAdd(&row->first_from[3], ff3);
        }
    }

    __syncthreads();
    for (int q = tid; q < nacc; q += kPrBlock) {               // one global atomic per non-zero entry
        const int k = q % kPL;
        if (k == PL_LSUM + 1) continue;                        // the high word of the u64 sum
        const uint32_t* hist = &s_acc[q - k + PL_HIST];         // the exact bins carry their own latency
        if (k == PL_LSUM) {
            unsigned long long v = *reinterpret_cast<const unsigned long long*>(&s_acc[q]);
            for (int b = 1; b < GSIM_REPORT_BINS - 1; ++b) v += (unsigned long long)b * hist[b];
            if (v) atomicAdd(&a.acc[q], v);
            continue;
        }
        uint32_t v = s_acc[q];
        if (k == PL_LMAX && !v)
            for (int b = GSIM_REPORT_BINS - 2; b > 0 && !v; --b) v = hist[b] ? (uint32_t)b : 0u;
        if (!v) continue;
        if (k == PL_LMAX) atomicMax(&a.acc[q], (unsigned long long)v);
        else atomicAdd(&a.acc[q], (unsigned long long)v);
    }
}

// The launch rule, a function of the owned peers walked and the selected
// messages: peer waves, and the parts the slots are split into.
void pr_launch(int64_t peers_walked_words, int64_t nsel, int64_t* waves, int64_t* parts)
{
    *waves = peers_walked_words;
    *parts = 1;
    if (*waves >= kPrFullWaves || nsel < 2 * kPrMinSlots) return;
    const int64_t want = (kPrTargetWaves + *waves - 1) / std::max<int64_t>(*waves, 1);
    *parts = std::max<int64_t>(1, std::min<int64_t>(want, nsel / kPrMinSlots));
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void peerreport_release(gsim_handle* h)
{
    if (!h->pr) return;
    PeerReport* r = h->pr;
    free_all({r->d_sel, r->d_cnt, r->d_acc, r->d_rows});
    delete r;
    h->pr = nullptr;
}

static int peerreport_scratch(gsim_handle* h, int32_t ring, int64_t rows)
{
    if (!h->pr) h->pr = new PeerReport;
    PeerReport* r = h->pr;
    int rc = grow(h, "peer report", &r->d_sel, &r->ring, std::max<int64_t>(ring, 1));
    if (!rc) rc = alloc_once(h, "peer report", &r->d_cnt, kPC);
    if (!rc) rc = alloc_once(h, "peer report", &r->d_acc, (int64_t)kPrAcc);
    if (!rc) rc = grow(h, "peer report", &r->d_rows, &r->rows_cap, rows);
    return rc;
}

extern "C" {

int gsim_peer_report(gsim_handle* h, int64_t round_lo, int64_t round_hi, int64_t peer_lo, int64_t peer_hi,
                     struct gsim_peer_row* peers, struct gsim_peer_class_row* classes, int64_t class_cap,
                     int64_t* n_classes, int64_t* n_msgs)
{
    if (!h || !n_classes || !n_msgs || class_cap < 0) return GSIM_EINVAL;
    const uint8_t* d_cls = nullptr;
    const int C = netreport_classes(h, &d_cls);
    const int T = h->t;
    const int64_t nc = (int64_t)T * C;
    *n_classes = nc;
    *n_msgs = 0;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    ReportView v{};
    if (!deliver_report_view(h, &v)) { h->err = "gsim_msgs_init not called"; return GSIM_ESTATE; }
    if (peer_lo < 0 || peer_lo > peer_hi || peer_hi > h->n) {
        h->err = "gsim_peer_report: the peer range must satisfy 0 <= peer_lo <= peer_hi <= N";
        return GSIM_EINVAL;
    }
    const bool want_cls = classes && class_cap > 0;
    // the rows written on the device: the owned peers of the range
    const int64_t olo = std::min<int64_t>(std::max<int64_t>(peer_lo, v.rlo), peer_hi);
    const int64_t ohi = std::max<int64_t>(olo, std::min<int64_t>(peer_hi, v.rhi));
    const bool want_peers = peers && peer_hi > peer_lo;
    int rc = deliver_flush(h);                     // the last round's claims become first-seen rounds
    if (!rc) rc = peerreport_scratch(h, v.ring, want_peers ? ohi - olo : 0);
    if (rc) return rc;
    PeerReport* r = h->pr;
    hipLaunchKernelGGL((k_select<PrFill, PC_TOPIC>), dim3(1), dim3(kSelBlock), 0, h->stream, v, round_lo, round_hi, r->d_sel,
                       r->d_cnt);
    uint32_t cs[kPC] = {};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cs, r->d_cnt, sizeof(cs), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_peer_report");
    const int64_t nsel = cs[PC_NSEL];
    *n_msgs = nsel;
    if (want_cls && class_cap < nc) { h->err = "gsim_peer_report: class row buffer too small"; return GSIM_ERANGE; }
    if (!want_cls && !want_peers) return deliver_check_errors(h);

    // the class rows cover every owned peer; without them the range's owned peers are walked
    const int64_t qlo = want_cls ? (int64_t)v.rlo : olo, qhi = want_cls ? (int64_t)v.rhi : ohi;
    std::vector<unsigned long long> acc((size_t)nc * kPL);
    if (qhi > qlo) {
        PeerArgs a{};
        a.cells = v.cells; a.sel = r->d_sel; a.nsel = nsel;
        a.sub = v.sub; a.cls = C > 1 ? d_cls : nullptr;
        a.T = T; a.C = C; a.n = h->n;
        a.w0 = qlo >> 6; a.qlo = qlo; a.qhi = qhi;
        a.olo = olo; a.ohi = want_peers ? ohi : olo;
        a.rows = want_peers && ohi > olo ? r->d_rows : nullptr;
        a.acc = want_cls && nc > 0 ? r->d_acc : nullptr;
        a.bad = r->d_cnt + PC_BAD;
        int64_t waves = 0, parts = 1;
        pr_launch(((qhi + 63) >> 6) - (qlo >> 6), nsel, &waves, &parts);
        a.per = std::max<int64_t>(1, (nsel + parts - 1) / parts);
        parts = std::max<int64_t>(1, (nsel + a.per - 1) / a.per);
        r->last[0] = waves; r->last[1] = parts; r->last[2] = nsel;
        if (a.acc) e = hipMemsetAsync(r->d_acc, 0, sizeof(unsigned long long) * (size_t)nc * kPL, h->stream);
        if (e == hipSuccess && a.rows && parts > 1)
            e = hipMemsetAsync(r->d_rows, 0, sizeof(gsim_peer_row) * (size_t)(ohi - olo), h->stream);
        if (e != hipSuccess) return hip_check(h, e, "gsim_peer_report");
        const dim3 grid((uint32_t)((waves + kPrBlock / 64 - 1) / (kPrBlock / 64)), (uint32_t)parts);
        const size_t lds = a.acc ? sizeof(uint32_t) * (size_t)nc * kPL : 0;
        if (a.cls) hipLaunchKernelGGL(k_peer_reduce<true>, grid, dim3(kPrBlock), lds, h->stream, a);
        else hipLaunchKernelGGL(k_peer_reduce<false>, grid, dim3(kPrBlock), lds, h->stream, a);
        uint32_t bad = 0;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, r->d_cnt + PC_BAD, sizeof bad, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && a.acc)
            e = hipMemcpyAsync(acc.data(), r->d_acc, sizeof(unsigned long long) * acc.size(), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && a.rows)                           // straight into the caller's rows
            e = hipMemcpyAsync(peers + (olo - peer_lo), r->d_rows, sizeof(gsim_peer_row) * (size_t)(ohi - olo),
                               hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return hip_check(h, e, "gsim_peer_report");
        if (bad) {
            h->err = "gsim_peer_report: a committed cell of an owned peer names a first sender that is no local peer";
            return GSIM_ESTATE;
        }
    }
    if (want_peers) {                              // the range's peers this engine does not own: empty rows
        std::memset(peers, 0, sizeof(gsim_peer_row) * (size_t)(olo - peer_lo));
        std::memset(peers + (ohi - peer_lo), 0, sizeof(gsim_peer_row) * (size_t)(peer_hi - ohi));
    }
    if (want_cls)
        for (int64_t q = 0; q < nc; ++q) {
            const unsigned long long* c = acc.data() + (size_t)q * kPL;
            gsim_peer_class_row x{};
            x.topic = (uint32_t)(q / C);
            x.cls = (uint32_t)(q % C);
            x.peers = (uint32_t)c[PL_PEERS];
            x.messages = cs[PC_TOPIC + x.topic];
            x.expected = (uint64_t)x.peers * x.messages;
            for (int k = 0; k < GSIM_REPORT_BINS; ++k) { x.hist[k] = c[PL_HIST + k]; x.received += c[PL_HIST + k]; }
            x.own = c[PL_OWN];
            x.missed = x.expected - (x.received - c[PL_STRAY]);
            x.lat_sum = c[PL_LSUM];
            x.lat_max = (uint32_t)c[PL_LMAX];
            for (int k = 0; k < GSIM_NET_CLASSES; ++k) x.first_from[k] = c[PL_FF + k];
            classes[q] = x;
        }
    return deliver_check_errors(h);
}

int gsim_peer_report_launch(gsim_handle* h, int64_t* out3)
{
    if (!h || !out3) return GSIM_EINVAL;
    for (int k = 0; k < 3; ++k) out3[k] = h->pr ? h->pr->last[k] : 0;
    return GSIM_OK;
}

}  // extern "C"
