// Propagation report (include/gsim.h gsim_msg_report): per message still in
// the ring, how many peers it reached and a histogram of their latencies
// (first-seen round - publication round), reduced on the device straight from
// the seen-set cells.  The reference has no such read-out; what is counted is
// the reach of DeliverMessage (score.go:702-726) per message.
//
// A slot's cells are one contiguous range on both seen-set layouts (a cell per
// peer, or per member of the slot's topic; gsim_internal.h Cells), in peer
// order.  The report therefore needs no bitmap lookup per cell and no
// [ring][N] view: it streams cell[cbase[m] .. cbase[m + 1]) of the selected
// slots once, 8 bytes per cell, and keeps 32 counters per slot.  A shard
// counts the peers it owns: they are one sub-range of the slot's cells
// (base + rlo .. base + rhi, or the member counts before rlo and rhi on a
// member-compacted topic), so a ghost's cell, which repeats the round its
// owner exported, is counted once, by its owner.
//
// Launches per call (none per slot, no host loop over slots):
//   k_select<MsgFill> one block: the slots published in [round_lo, round_hi),
//                     compacted in slot order (report_common.h), each with its
//                     row header; the rows' slot fields are the slot list of the
//                     next launch
//   k_report_subs     subscribers per topic: a popcount pass over `sub` of the
//                     owned peers
//   k_report_reduce   block (x, y) reduces chunks x, x + gridDim.x, ... of
//                     slot row[y].slot's cell range
// Device scratch is ring rows (176 bytes each) and 65 counters.
//
// k_report_reduce: a lane reads two cells with one 16-byte load (a range that
// starts or ends on an odd cell leaves a head / tail cell, read with 8-byte
// loads by block x = 0), four loads in flight per lane.  Latencies cluster on a
// handful of values, so lanes never add to a counter themselves: per cell
// position the wave loops over the distinct bins present (__ballot of the
// lanes holding the leader's bin, __popcll), and lane b of the wave keeps the
// count of bin b in a register.  At the end each wave stores its 32 counts to
// its LDS histogram, the block sums its waves' and issues one global atomic
// per non-zero bin; max_latency is a per-lane maximum, reduced over the wave
// and the block, then one atomicMax.
//
// Resources (gfx950, -Rpass-analysis=kernel-resource-usage), none with scratch
// or spills, all at 8 waves/SIMD:
//   k_report_reduce  28 VGPRs, 54 SGPRs, 528 bytes of LDS
//   k_select<MsgFill>  24 VGPRs, 52 SGPRs, 68 bytes of LDS
//   k_report_subs    10 VGPRs, 22 SGPRs, 1024 bytes of LDS
// Measured: C3 after the default bench's ticks, 1477 messages,
// 11.8 GB of cells in 2.20 ms for the whole call: 5.4 TB/s.
#include <algorithm>
#include <vector>

#include "report_common.h"

namespace gsim {

struct Report {
    MsgReport* d_rows = nullptr;   // [ring] the selected rows, slot order
    uint32_t* d_cnt = nullptr;           // [0] selected rows, [1 + t] subscribers of topic t
    int64_t ring = 0;
};

namespace {

constexpr int kRpBlock = 256;            // k_report_reduce: 4 waves
constexpr int kRpBatch = 4;              // 16-byte loads in flight per lane
constexpr int kRpChunk = 2 * kRpBlock;   // cells a block reads per load step

// The selected slot's row header (k_select, report_common.h).
struct MsgFill {
    using Row = MsgReport;
    __device__ static uint32_t fill(Row& r, const ReportView& v, int m, int64_t pub)
    {
        r.id = v.mid[m];                                       // hist, reached, max_latency: zeroed by the caller
        r.pub_round = pub;
        r.slot = (uint32_t)m;
        r.topic = v.mtopic[m];
        r.origin = v.morigin[m];
        r.verdict = v.minv[m];
        r.vdelay = v.mlat[m];
        return r.topic;
    }
};

// Subscribers per topic among the owned peers: lane t of a wave counts topic t.
__global__ __launch_bounds__(256) void k_report_subs(const uint64_t* sub, int64_t rlo, int64_t rhi, int32_t T, uint32_t* out)
{
    __shared__ uint32_t s_c[4][64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t stride = (int64_t)gridDim.x * 256;
    uint32_t acc = 0;
    for (int64_t p0 = rlo + (int64_t)blockIdx.x * 256; p0 < rhi; p0 += stride) {
        const int64_t p = p0 + tid;
        const uint64_t s = p < rhi ? sub[p] : 0ull;
        for (int t = 0; t < T; ++t) {
            const uint32_t c = (uint32_t)__popcll(__ballot((s >> t) & 1ull));
            acc += lane == t ? c : 0u;
        }
    }
    s_c[w][lane] = acc;
    __syncthreads();
    if (tid < T) {
        const uint32_t c = s_c[0][tid] + s_c[1][tid] + s_c[2][tid] + s_c[3][tid];
        if (c) atomicAdd(&out[tid], c);
    }
}

// One cell position of the wave: lanes holding a committed cell (an unseen
// cell reads all ones, a claim has kClaim set; neither is counted) contribute
// their latency.  The wave walks the distinct bins present; lane b keeps bin b.
__device__ __forceinline__ void rp_add(uint32_t hi, uint32_t pub, int lane, uint32_t& acc, uint32_t& mx)
{
    const bool ok = !(hi & kClaim);
    const uint32_t d = hi - pub;
    const uint32_t bin = d < GSIM_REPORT_BINS - 1 ? d : GSIM_REPORT_BINS - 1;
    if (ok && d > mx) mx = d;
    walk_keys(ok, bin, [&](uint32_t b, uint64_t same, int) { acc += lane == (int)b ? (uint32_t)__popcll(same) : 0u; });
}

// members of topic t before peer p (a member-compacted topic; p <= n)
__device__ __forceinline__ int64_t members_before(const Cells& cs, int32_t t, int64_t p, int64_t n, int64_t all)
{
    if (p >= n) return all;
    uint64_t bits;
    int64_t pre, idx;
    bool has;
    cs.word(t, p >> 6, bits, pre);
    member_rank(bits, pre, (int)(p & 63), has, idx);            // (p itself need not be a member)
    return idx;
}

__global__ __launch_bounds__(kRpBlock) void k_report_reduce(ReportView v, MsgReport* rows)
{
    __shared__ uint32_t s_h[kRpBlock / 64][GSIM_REPORT_BINS];
    __shared__ uint32_t s_mx[kRpBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    MsgReport& row = rows[blockIdx.y];
    const uint32_t m = row.slot;
    const uint32_t pub = (uint32_t)v.mpub[m];
    // the owned peers' cells of the slot: [b, e)
    const int64_t base = (int64_t)v.cells.cbase[m];
    const int64_t end = (int64_t)m + 1 < v.ring ? (int64_t)v.cells.cbase[m + 1] : v.ncells;
    int64_t b = base, e = end;
    if (v.rlo != 0 || (int64_t)v.rhi != v.n) {
        const int32_t t = (int32_t)v.mtopic[m];
        if ((v.cells.sparse >> t) & 1ull) {
            b = base + members_before(v.cells, t, v.rlo, v.n, end - base);
            e = base + members_before(v.cells, t, v.rhi, v.n, end - base);
        } else {
            b = base + v.rlo;
            e = base + v.rhi;
        }
    }
    e = e < end ? e : end;
    b = b < e ? b : e;
    const uint64_t* cell = v.cells.cell;
    // 16-byte loads from the first 16-byte aligned cell on
    const int64_t b2 = b + (int64_t)((((uintptr_t)(cell + b)) >> 3) & 1);
    const int64_t np = b2 < e ? (e - b2) >> 1 : 0;             // whole pairs
    const ulonglong2* pair = reinterpret_cast<const ulonglong2*>(cell + b2);
    uint32_t acc = 0, mx = 0;
    const int64_t stride = (int64_t)gridDim.x * kRpBlock;
    for (int64_t q0 = (int64_t)blockIdx.x * kRpBlock; q0 < np; q0 += stride * kRpBatch) {
        uint32_t h0[kRpBatch], h1[kRpBatch];
#pragma unroll
        for (int u = 0; u < kRpBatch; ++u) {
            const int64_t q = q0 + (int64_t)u * stride + tid;
            const ulonglong2 c = pair[q < np ? q : np - 1];    // unconditional: the batch's loads issue together
            h0[u] = q < np ? (uint32_t)(c.x >> 32) : 0xFFFFFFFFu;
            h1[u] = q < np ? (uint32_t)(c.y >> 32) : 0xFFFFFFFFu;
        }
#pragma unroll
        for (int u = 0; u < kRpBatch; ++u) {
            rp_add(h0[u], pub, lane, acc, mx);
            rp_add(h1[u], pub, lane, acc, mx);
        }
    }
    if (blockIdx.x == 0 && w == 0) {                            // the unaligned head and the odd tail
        uint32_t hi = 0xFFFFFFFFu;
        if (lane == 0 && b < e && b2 > b) hi = (uint32_t)(cell[b] >> 32);
        if (lane == 1 && b2 + 2 * np < e) hi = (uint32_t)(cell[e - 1] >> 32);
        rp_add(hi, pub, lane, acc, mx);
    }
    mx = wave_max(mx);
    if (lane < GSIM_REPORT_BINS) s_h[w][lane] = acc;
    if (lane == 0) s_mx[w] = mx;
    __syncthreads();
    if (tid < GSIM_REPORT_BINS) {
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < kRpBlock / 64; ++q) c += s_h[q][tid];
        if (c) atomicAdd(&row.hist[tid], c);
    }
    if (tid == 0) {
        uint32_t x = 0;
#pragma unroll
        for (int q = 0; q < kRpBlock / 64; ++q) x = s_mx[q] > x ? s_mx[q] : x;
        if (x) atomicMax(&row.max_latency, x);
    }
}

}  // namespace
}  // namespace gsim

using namespace gsim;

void report_release(gsim_handle* h)
{
    if (!h->rp) return;
    free_all({h->rp->d_rows, h->rp->d_cnt});
    delete h->rp;
    h->rp = nullptr;
}

static int report_scratch(gsim_handle* h, int32_t ring)
{
    if (!h->rp) h->rp = new Report;
    Report* r = h->rp;
    int rc = grow(h, "report", &r->d_rows, &r->ring, (int64_t)ring);
    if (!rc) rc = alloc_once(h, "report", &r->d_cnt, 1 + GSIM_MAX_TOPICS);
    return rc;
}

extern "C" {

int gsim_msg_report(gsim_handle* h, int64_t round_lo, int64_t round_hi, struct gsim_msg_report* out, int64_t cap,
                    int64_t* n)
{
    if (!h || !n || cap < 0) return GSIM_EINVAL;
    *n = 0;
    if (hipSetDevice(h->device) != hipSuccess) return GSIM_EDEVICE;
    ReportView v{};
    if (!deliver_report_view(h, &v)) { h->err = "gsim_msgs_init not called"; return GSIM_ESTATE; }
    int rc = deliver_flush(h);                     // the last round's claims become first-seen rounds
    if (!rc) rc = report_scratch(h, v.ring);
    if (rc) return rc;
    Report* r = h->rp;
    const bool fill = out && cap > 0;
    hipError_t e = hipSuccess;
    if (fill) e = hipMemsetAsync(r->d_rows, 0, sizeof(MsgReport) * (size_t)v.ring, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->d_cnt, 0, sizeof(uint32_t) * (1 + GSIM_MAX_TOPICS), h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_msg_report");
    hipLaunchKernelGGL((k_select<MsgFill, 0>), dim3(1), dim3(kSelBlock), 0, h->stream, v, round_lo, round_hi, r->d_rows,
                       r->d_cnt);
    if (fill && v.rhi > v.rlo && v.T > 0)
        hipLaunchKernelGGL(k_report_subs, dim3((uint32_t)std::min<int64_t>(((int64_t)v.rhi - v.rlo + 255) / 256, 2048)),
                           dim3(256), 0, h->stream, v.sub, (int64_t)v.rlo, (int64_t)v.rhi, v.T, r->d_cnt + 1);
    uint32_t cs[1 + GSIM_MAX_TOPICS] = {};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cs, r->d_cnt, sizeof(cs), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return hip_check(h, e, "gsim_msg_report");
    const int64_t cnt = cs[0];
    *n = cnt;
    if (!fill) return deliver_check_errors(h);
    if (cap < cnt) { h->err = "output buffer too small for the selected messages"; return GSIM_ERANGE; }
    if (cnt) {
        // blocks per slot: chunks of kRpChunk cells, a few thousand blocks in all
        const int64_t longest = std::min<int64_t>((int64_t)v.rhi - v.rlo, v.ncells);
        const int64_t gx = std::max<int64_t>(1, std::min<int64_t>((longest + 16 * kRpChunk - 1) / (16 * kRpChunk),
                                                                  std::max<int64_t>(1, 8192 / cnt)));
        hipLaunchKernelGGL(k_report_reduce, dim3((uint32_t)gx, (uint32_t)cnt), dim3(kRpBlock), 0, h->stream, v, r->d_rows);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(out, r->d_rows, sizeof(MsgReport) * (size_t)cnt, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return hip_check(h, e, "gsim_msg_report");
        for (int64_t k = 0; k < cnt; ++k) {
            MsgReport& x = out[k];
            uint32_t s = 0;
            for (int q = 0; q < GSIM_REPORT_BINS; ++q) s += x.hist[q];
            x.reached = s;
            x.subscribers = x.topic < (uint32_t)GSIM_MAX_TOPICS ? cs[1 + x.topic] : 0;
        }
        // the device compacts in slot order: a stable sort by round gives (pub_round, slot)
        std::stable_sort(out, out + cnt, [](const MsgReport& a, const MsgReport& b) {
            return a.pub_round < b.pub_round;
        });
    }
    return deliver_check_errors(h);
}

}  // extern "C"
