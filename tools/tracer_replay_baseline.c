/* The CPU side of tools/tracer_events_times.py: the oracle's RawTracer
 * functions over a stream already grouped by observer, one observer per OpenMP
 * task, one orc_drecs per observer.  Built against oracle/liboracle.so by the
 * tool; test / measurement infrastructure, never shipped. */
#include <stdint.h>

#include "gsim.h"
#include "oracle.h"

/* ev: the grouped stream; edge[k]: the observer-row edge of event k;
 * seg[s] .. seg[s + 1]: the events of one observer */
void tracer_replay(orc_net* s, const gsim_score_event* ev, const int64_t* edge, const int64_t* seg, int64_t nseg)
{
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t q = 0; q < nseg; ++q) {
        orc_drecs* d = orc_drecs_new(0);
        for (int64_t k = seg[q]; k < seg[q + 1]; ++k) {
            const gsim_score_event* x = &ev[k];
            const int64_t e = edge[k];
            switch (x->kind) {
            case GSIM_EV_VALIDATE: orc_validate_message(s, d, x->mid, x->now_ns); break;
            case GSIM_EV_DELIVER: orc_deliver_message(s, d, e, x->mid, x->topic, x->now_ns); break;
            case GSIM_EV_REJECT: orc_reject_message(s, d, e, x->mid, x->topic, x->arg, x->now_ns); break;
            case GSIM_EV_DUPLICATE: orc_duplicate_message(s, d, e, x->mid, x->topic, x->now_ns); break;
            case GSIM_EV_GRAFT: orc_graft(s, e, x->topic, x->now_ns); break;
            case GSIM_EV_PRUNE: orc_prune(s, e, x->topic); break;
            case GSIM_EV_ADD_PENALTY: orc_add_penalty(s, e, x->arg); break;
            default: break;
            }
        }
        orc_drecs_free(d);
    }
}
