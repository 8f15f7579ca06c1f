/*
 * gsim.h — C ABI of the MI355X-native GossipSub scoring + heartbeat engine.
 *
 * This is the drop-in boundary for the reference's hot path.
 * Every entry point names the reference interface it replaces (file:line into
 * mouzzarr/go-libp2p-pubsub).  Conventions:
 *   - plain C types only; durations are int64 nanoseconds (Go time.Duration);
 *   - every function returns int: 0 = OK, negative errno-style on error;
 *     a human-readable message is available from gsim_last_error(h)
 *     (the reference returns Go `error`s with the same meaning);
 *   - no allocation crosses the boundary; callers own every buffer they pass,
 *     inputs are copied in, readbacks copy out (blocking);
 *   - a handle is single-threaded (the reference serializes all router and
 *     peerScore work on one event loop, pubsub.go:561-675);
 *   - topics cross as dense indices 0..T-1 (the Go shim maps topic strings to
 *     indices in sorted order); peers cross as dense indices 0..N-1.
 */
#ifndef GSIM_H
#define GSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
#define GSIM_OK        0
#define GSIM_EINVAL  (-22) /* invalid argument / parameter validation failed */
#define GSIM_ENOMEM  (-12) /* device or host allocation failed               */
#define GSIM_EDEVICE  (-5) /* HIP runtime error, or no gfx950 device           */
#define GSIM_ERANGE  (-34) /* size outside what the engine supports           */
#define GSIM_ESTATE  (-71) /* call out of order (e.g. step before load_graph)  */

/* ---- parameter blocks (field-for-field mirrors of the Go structs) ------- */

/* TopicScoreParams, score_params.go:117-170. */
typedef struct gsim_topic_score_params {
    int32_t skip_atomic_validation;
    int32_t scored;                 /* 1 if present in PeerScoreParams.Topics */
    double  topic_weight;
    /* P1 */
    double  time_in_mesh_weight;
    int64_t time_in_mesh_quantum_ns;
    double  time_in_mesh_cap;
    /* P2 */
    double  first_message_deliveries_weight;
    double  first_message_deliveries_decay;
    double  first_message_deliveries_cap;
    /* P3 */
    double  mesh_message_deliveries_weight;
    double  mesh_message_deliveries_decay;
    double  mesh_message_deliveries_cap;
    double  mesh_message_deliveries_threshold;
    int64_t mesh_message_deliveries_window_ns;
    int64_t mesh_message_deliveries_activation_ns;
    /* P3b */
    double  mesh_failure_penalty_weight;
    double  mesh_failure_penalty_decay;
    /* P4 */
    double  invalid_message_deliveries_weight;
    double  invalid_message_deliveries_decay;
} gsim_topic_score_params;

/* PeerScoreParams, score_params.go:66-115.  AppSpecificScore (a Go callback)
 * is replaced by a per-peer array set with gsim_set_app_score();
 * IPColocationFactorWhitelist (CIDR list) by a per-IP flag array set with
 * gsim_set_ip_whitelist(). */
typedef struct gsim_peer_score_params {
    int32_t skip_atomic_validation;
    int32_t has_app_specific_score;   /* AppSpecificScore != nil */
    double  topic_score_cap;
    double  app_specific_weight;
    double  ip_colocation_factor_weight;
    int32_t ip_colocation_factor_threshold;
    int32_t _pad0;
    double  behaviour_penalty_weight;
    double  behaviour_penalty_threshold;
    double  behaviour_penalty_decay;
    int64_t decay_interval_ns;
    double  decay_to_zero;
    int64_t retain_score_ns;
    int64_t seen_msg_ttl_ns;
} gsim_peer_score_params;

/* PeerScoreThresholds, score_params.go:12-35. */
typedef struct gsim_thresholds {
    int32_t skip_atomic_validation;
    int32_t _pad0;
    double  gossip_threshold;
    double  publish_threshold;
    double  graylist_threshold;
    double  accept_px_threshold;
    double  opportunistic_graft_threshold;
} gsim_thresholds;

/* GossipSubParams, gossipsub.go:63-205 (defaults gossipsub.go:244-275). */
typedef struct gsim_gossipsub_params {
    int32_t d, dlo, dhi, dscore, dout;
    int32_t history_length, history_gossip;
    int32_t dlazy;
    double  gossip_factor;
    int32_t gossip_retransmission;
    int32_t prune_peers;
    int64_t heartbeat_initial_delay_ns;
    int64_t heartbeat_interval_ns;
    double  slow_heartbeat_warning;
    int64_t fanout_ttl_ns;
    int64_t prune_backoff_ns;
    int64_t unsubscribe_backoff_ns;
    int32_t connectors;
    int32_t max_pending_connections;
    int64_t connection_timeout_ns;
    uint64_t direct_connect_ticks;
    int64_t direct_connect_initial_delay_ns;
    uint64_t opportunistic_graft_ticks;
    int32_t opportunistic_graft_peers;
    int32_t max_ihave_length;
    int64_t graft_flood_threshold_ns;
    int32_t max_ihave_messages;
    int32_t flood_publish;   /* router option WithFloodPublish (gossipsub.go:321-334); this fork's default is 0 */
    int64_t iwant_followup_time_ns;
    int32_t do_px;           /* router option WithPeerExchange (gossipsub.go:340-350): PRUNEs carry PX; default 0 */
    int32_t _pad_px;
} gsim_gossipsub_params;

/* ---- host-side parameter API (no device needed) ------------------------ */

/* DefaultGossipSubParams(), gossipsub.go:244-275. */
void gsim_default_gossipsub_params(gsim_gossipsub_params* out);

/* TopicScoreParams.validate(), score_params.go:236-398.  err may be NULL. */
int gsim_validate_topic_params(const gsim_topic_score_params* p, char* err, size_t errlen);
/* PeerScoreParams.validate(), score_params.go:173-234 (validates every scored
 * topic first, as the reference does). */
int gsim_validate_peer_params(const gsim_peer_score_params* p,
                              const gsim_topic_score_params* topics, int32_t n_topics,
                              char* err, size_t errlen);
/* PeerScoreThresholds.validate(), score_params.go:37-64. */
int gsim_validate_thresholds(const gsim_thresholds* p, char* err, size_t errlen);
/* NewMessageCache(gossip, history) panics if gossip > history, mcache.go:21-26;
 * here it is a GSIM_EINVAL from gsim_create. */

/* ScoreParameterDecay / ScoreParameterDecayWithBase, score_params.go:405-417. */
double gsim_score_parameter_decay(int64_t decay_ns);
double gsim_score_parameter_decay_with_base(int64_t decay_ns, int64_t base_ns, double decay_to_zero);

/* ---- engine lifecycle -------------------------------------------------- */

typedef struct gsim_handle gsim_handle;

/* Replaces WithPeerScore(params, thresholds) (gossipsub.go:278-319) +
 * WithGossipSubParams (gossipsub.go:398-411) + newPeerScore (score.go:183-195).
 * Validates like the reference (GSIM_EINVAL + message; the message is also
 * written to err when err != NULL since no handle exists on failure).
 * Also GSIM_EINVAL, before a device is asked for: HistoryGossip >
 * HistoryLength; D < 0, Dlo > D, D > Dhi, Dout > D (gossipsub.go:90), Dscore < 0
 * or Dlazy < 0 (the heartbeat restates the reference's loops for the
 * documented order of the degree parameters); PrunePeers < 1 with do_px (the
 * reference then lists every topic peer, gossipsub.go:1923).
 * device: HIP device ordinal. */
int gsim_create(const gsim_peer_score_params* params,
                const gsim_topic_score_params* topics, int32_t n_topics,
                const gsim_thresholds* thresholds,
                const gsim_gossipsub_params* gossip,
                int32_t device, gsim_handle** out, char* err, size_t errlen);
/* newPeerScore (score.go:183-195) without WithPeerScore's validation: the
 * reference's unit tests build peerScore this way with parameters validate()
 * would reject (e.g. decay 1.0).  Also disables validation in
 * gsim_set_topic_params for this handle. */
int gsim_create_unvalidated(const gsim_peer_score_params* params,
                            const gsim_topic_score_params* topics, int32_t n_topics,
                            const gsim_thresholds* thresholds,
                            const gsim_gossipsub_params* gossip,
                            int32_t device, gsim_handle** out, char* err, size_t errlen);
int gsim_destroy(gsim_handle* h);
const char* gsim_last_error(const gsim_handle* h);

/* Load the simulated network: a CSR of N observers.  Row i lists the peers i
 * is connected to (must be symmetric: j in row i <=> i in row j; rows sorted
 * ascending, no self loops, no duplicates).  outbound[e] = 1 if observer
 * row(e) initiated the connection to col[e] (gossipsub.go:525-552).
 * subscriptions[i] = bitmask of topics peer i subscribes to (T <= 64).
 * ip_ptr/ip_ids = per-peer CSR of IP ids as seen by its neighbours
 * (score.go:984-1024 getIPs; IPv6 /64 prefixes are just more ids).
 * Every edge starts tracked+connected (AddPeer, score.go:595-609) with zero
 * counters, nothing in any mesh.  Copies everything.  No row limit applies:
 * a peer may hold any number of connections (the reference has no degree
 * bound); the one bound is the uint32 edge index, E < 2^32. */
int gsim_load_graph(gsim_handle* h, int64_t n_peers,
                    const uint32_t* row_ptr, const uint32_t* col_idx,
                    const uint8_t* outbound, const uint64_t* subscriptions,
                    const uint32_t* ip_ptr, const uint32_t* ip_ids, uint32_t n_ips);

/* AppSpecificScore(p) for every peer (score_params.go:78) — host refreshes. */
int gsim_set_app_score(gsim_handle* h, const double* p5);
/* IPColocationFactorWhitelist (score_params.go:91): whitelisted[ip_id] = 1 if
 * any whitelisted CIDR contains that IP (host precomputes net.IPNet.Contains). */
int gsim_set_ip_whitelist(gsim_handle* h, const uint8_t* whitelisted);
/* WithDirectPeers (gossipsub.go:352-374): flags[e] != 0 when col[e] is in
 * the observer's direct set (E bytes, edge order; NULL clears).  Direct
 * peers are never grafted or gossiped to, GRAFTs from them are answered
 * with PRUNE (gossipsub.go:768-776), they receive every message of a topic
 * they joined (991-1003) and AcceptFrom accepts them whatever their score
 * (598-609).  The reconnect loop (directConnect) is not modelled. */
int gsim_set_direct_peers(gsim_handle* h, const uint8_t* flags);
/* SetTopicScoreParams (score.go:201-241, topic.go:44-82): validates, installs,
 * and recaps first/mesh counters when caps are lowered. */
int gsim_set_topic_params(gsim_handle* h, int32_t topic, const gsim_topic_score_params* p);

/* ---- hot path ---------------------------------------------------------- */

/* peerScore.refreshScores (score.go:504-565) for every observer at virtual
 * time now_ns, fused with peerScore.score (score.go:265-342) of every edge into
 * the score snapshot; P6 (score.go:344-388) is re-derived first when the
 * tracked set changed. */
int gsim_refresh_scores(gsim_handle* h, int64_t now_ns);
/* peerScore.score only (no decay) for every edge -> score snapshot. */
int gsim_compute_scores(gsim_handle* h);
/* ipColocationFactor (score.go:344-388) for every edge (segmented count over
 * each observer's neighbour IPs). */
int gsim_compute_ip_colocation(gsim_handle* h);

/* Seed of the Philox stream that replaces the reference's global math/rand
 * (gossipsub.go:1954-1973, gossip_tracer.go:53). */
int gsim_set_seed(gsim_handle* h, uint64_t seed);

/* GossipSubRouter.heartbeat (gossipsub.go:1345-1606) for every observer at
 * heartbeat tick `tick` (heartbeatTicks after its increment, so the first
 * heartbeat is tick 1) and virtual time now_ns: clearBackoff every 15 ticks,
 * per joined topic in ascending order: negative-score prune, Dlo graft, Dhi
 * score/random prune with the Dout rotation, Dout top-up, opportunistic graft
 * every OpportunisticGraftTicks; Graft/Prune traced into the score counters.
 * Uses the current score snapshot as the heartbeat's score cache
 * (gossipsub.go:1375-1383): call gsim_refresh_scores first.  GRAFT/PRUNE
 * records land in the receivers' control inbox for round 0.  No row limit
 * applies (rows of any length; the longest run on kernels that stream the row
 * in tiles).  Fails with the
 * previous tick's delivery error, if any (GSIM_ERANGE: the IWANT response
 * queue overflowed; GSIM_ESTATE: a slot was republished too early). */
int gsim_heartbeat(gsim_handle* h, uint64_t tick, int64_t now_ns);
/* Control-message round: every receiver handles the GRAFT/PRUNE records in
 * its inbox for `round` (handleGraft gossipsub.go:741-837, handlePrune
 * 839-871), senders in ascending peer order; PRUNE replies land in the inbox
 * of round+1. */
int gsim_handle_control(gsim_handle* h, int32_t round, int64_t now_ns);

/* Connections going down (up = 0) or up (up = 1) between two ticks, both
 * endpoints notified (handleDeadPeers pubsub.go:711-759; the new-peer case of
 * processLoop pubsub.go:575-595).  pairs = count (peer a, peer b) u32 pairs,
 * each an existing CSR connection, each at most once.
 *   down: router RemovePeer (gossipsub.go:554-567): out of every mesh without
 *         PRUNE, pending control dropped, backoff kept; score tracer
 *         RemovePeer (score.go:611-644): a positive live score is dropped,
 *         otherwise retained until now + RetainScore with P2 reset and the
 *         P3b penalty applied.
 *   up:   router AddPeer (gossipsub.go:525-552), peerScore.AddPeer
 *         (score.go:595-609): a retained record is reused, else a fresh one.
 * The removed peer's live score uses P6 over the tracked set as the batch
 * starts (re-derived if an up batch changed it).  GSIM_EINVAL if a
 * pair is not a connection or is listed twice (nothing is changed then). */
int gsim_set_connections(gsim_handle* h, const uint32_t* pairs, int32_t count, int32_t up, int64_t now_ns);

/* Peer exchange (WithPeerExchange: gsim_gossipsub_params.do_px).  PRUNEs
 * carry PX (makePrune, gossipsub.go:1866-1906: the heartbeat's Dhi prunes and
 * handleGraft's mesh-full replies); the pruned peer's handlePrune accepts it
 * from peers it scores at least acceptPXThreshold and pxConnect queues a
 * connection attempt to every listed peer it is not connected to
 * (gossipsub.go:860-869, 893-939).  This call is the connector
 * (gossipsub.go:941-973), run between ticks: every attempt whose peers know
 * each other's address (an edge of the loaded graph) and are not connected
 * becomes a connection, dialled by the peer that asked (outbound on its side;
 * the lower id when both asked), with AddPeer at both ends as in
 * gsim_set_connections.  pairs (optional, cap entries): the (dialer, peer)
 * pairs connected, sorted.  Single engines only. */
int gsim_px_connect(gsim_handle* h, int64_t now_ns, uint32_t* pairs, int64_t cap, int64_t* n_connected);

/* ---- connection tags and the connection manager's trim -- */
/* The tag tracer (tag_tracer.go) and the observable of go-libp2p's
 * BasicConnMgr that gossipsub_connmgr_test.go pins, for every router at once.
 * Per router i and connection e = (i, j):
 *   protected(e)  direct[e], or j in i's mesh of any topic (tagPeerIfDirect,
 *                 tagMeshPeer / untagMeshPeer: Protect / Unprotect by tag
 *                 name).  Derived from the router state, not stored.
 *   dtag[t][e]    u8, for every topic t that i has joined: DeliverMessage of an
 *                 ACCEPTED first delivery of a message of t whose ReceivedFrom
 *                 is j does v = min(v + bump, cap) (BumpSumBounded(0, cap)).
 *                 The origin's own cell bumps nothing; the verdicts reject /
 *                 ignore / throttle / bad signature bump nothing; a first
 *                 delivery pulled by IWANT bumps the advertiser.
 *   decay         DecayFixed(decay_amount) at the instants t0 + k * interval,
 *                 k >= 1: v = max(0, v - amount), applied by the first
 *                 gsim_refresh_scores(now) with now >= that instant, after
 *                 the bumps of everything delivered before that refresh; a
 *                 refresh that crosses several instants decrements as often.
 *   Leave         removes the router's tags of the topic (removeDeliveryTag);
 *                 a later Join starts at 0.
 *   down / up     a connection going down drops its tags at both ends; one
 *                 coming up (churn, PX) starts at 0 with since[e] = now (the
 *                 connection manager's firstSeen, for the grace period).
 *                 Connections present at gsim_conn_tags_config are out of grace.
 *   value(e)      the sum of dtag[t][e] over the router's joined topics.
 * Declared differences: the decayer's Resolution is the heartbeat; every
 * (router, topic) shares the phase t0 (a tag's own registration time is not
 * modelled); near-first credit (nearFirst, peers delivering while the first
 * copy validates) is not built: while tags are configured a publication with
 * vdelay > 0 is refused with GSIM_ESTATE (gsim_publish, gsim_step: nothing is
 * published).  The bumps are folded from the committed seen-set cells (first
 * sender, first-seen round) once per refresh and at the start of every call
 * below and of gsim_set_connections, gsim_px_connect, gsim_set_subscriptions.
 * A caller that runs rounds without any of these for as long as a ring slot
 * must rest before it is reused ((max(HistoryLength, HistoryGossip) + the
 * promise ticks + 2) * rounds) gets a fold at its next publication, before a
 * slot can be reset: no first delivery is lost between two folds.  An engine that never configures tags allocates and launches nothing.
 * Single engines only: every call returns GSIM_ESTATE on a shard of a group
 * and, but for the config, before gsim_conn_tags_config. */
typedef struct gsim_conn_tag_params {
    int32_t bump, cap, decay_amount;  /* GossipSubConnTagBumpMessageDelivery 1, ...MessageDeliveryCap 15, ...DecayAmount 1 */
    int32_t _pad;
    int64_t decay_interval_ns;        /* GossipSubConnTagDecayInterval, 10 min */
    int64_t t0_ns;                    /* phase of the decay instants */
} gsim_conn_tag_params;
/* The reference's values (tag_tracer.go:13-31) with phase t0_ns. */
int gsim_default_conn_tag_params(int64_t t0_ns, gsim_conn_tag_params* out);
/* After gsim_msgs_init (else GSIM_ESTATE), and refused with GSIM_ESTATE once a
 * message with vdelay > 0 was published on the handle (copies may be pending
 * validation; a later gsim_msgs_init starts over).  GSIM_EINVAL unless cap in 1..255,
 * bump >= 1, decay_amount >= 1, decay_interval_ns > 0.  Every tag starts at 0
 * and the first deliveries counted are those of the rounds not yet run.
 * Calling it again starts from zero tags; NULL turns the tags off and frees
 * their memory (u8 [S][E] topic slot planes and i64 [E]); so does a new graph. */
int gsim_conn_tags_config(gsim_handle* h, const gsim_conn_tag_params* p);
/* out[E], edge order: dtag[topic][e] (0 where the router has not joined). */
int gsim_conn_tags_read(gsim_handle* h, int32_t topic, uint8_t* out);
#define GSIM_CONN_CONNECTED 0x01
#define GSIM_CONN_PROTECTED 0x02
#define GSIM_CONN_GRACE     0x04   /* since + grace_ns > now_ns */
/* value[E] and flags[E] (GSIM_CONN_*), edge order; either may be NULL (both:
 * the pending bumps are folded and nothing is read). */
int gsim_conn_values(gsim_handle* h, int64_t now_ns, int64_t grace_ns, int32_t* value, uint8_t* flags);
/* TrimOpenConns / getConnsToClose restated, for every router at once on the
 * state before any close.  A router with connected > high trims (high == 0:
 * every router with connected > low, the forced trim).  Its candidates are its
 * connections that are connected, not protected and out of grace (since +
 * grace_ns <= now_ns), ordered ascending by (value, key), the key being
 * Philox(seed; tick, router, topic 0, purpose 19, neighbour id) above the row
 * position (the selection keys of DESIGN.md §3.4); it closes the first
 * connected - low of them, all of them if there are fewer.  The union over
 * the routers, as unique pairs (a < b) sorted ascending, is written to pairs
 * (*n of them) and applied as gsim_set_connections(pairs, *n, up = 0, now_ns):
 * a connection either end chose closes, so a router may end below low.
 * pairs NULL or cap 0: *n is counted and nothing closes; 0 < cap < *n:
 * GSIM_ERANGE, nothing closes.  GSIM_EINVAL unless 0 <= low, 0 <= high,
 * grace_ns >= 0 and (high == 0 or low <= high). */
int gsim_conn_trim(gsim_handle* h, uint64_t tick, int64_t now_ns, int32_t low, int32_t high, int64_t grace_ns,
                   uint32_t* pairs, int64_t cap, int64_t* n);

/* ---- message propagation ------------------------------ */
/* Rounds are numbered globally: round g belongs to heartbeat tick g / rounds
 * and happens at virtual time
 *   T(g) = t0 + (g / rounds) * heartbeat + (g % rounds + 1) * heartbeat / (rounds + 1).
 * The seen-set is a ring of `ring` message slots x N peers (u32 first-seen
 * round, 0xFFFFFFFF = unseen): the timecache (timecache/first_seen_cache.go)
 * restricted to messages that can still arrive.  Publishing into a slot ends
 * the propagation of its previous message; SeenMsgTTL and the ring must
 * outlast a message's propagation (they do for every reference configuration).
 *
 * Bounds of the clock (each checked on the host, before anything runs):
 *   rounds        >= 2 (GSIM_EINVAL from gsim_msgs_init).
 *   heartbeat_ns  > 0, and long enough for the promise ring: IWANT promises
 *                 are kept per heartbeat for IWantFollowupTime, so
 *                   (heartbeat_ns / (rounds + 1) + IWantFollowupTime) / heartbeat_ns + 2
 *                 (the promise ticks, integer division) must not exceed 64
 *                 (GSIM_EINVAL from gsim_msgs_init; with the default
 *                 IWantFollowupTime of 3 s and two rounds a tick: 48 ms at the least).
 *   round number  0 .. 2^31 - 2: a seen-set cell holds a first-seen round in 31
 *                 bits and 2^31 - 1 is not a round.  gsim_round and gsim_publish
 *                 of any other round, and a gsim_step whose last round would
 *                 pass it, return GSIM_ERANGE and change nothing.
 *   vdelay        0 .. GSIM_MAX_VDELAY (GSIM_EINVAL from gsim_publish).  A copy
 *                 arriving in round g completes in round g + vdelay, which its
 *                 cell must hold: a message with vdelay > 0 is refused
 *                 (GSIM_ERANGE) in a round above 2^31 - 2 - GSIM_MAX_VDELAY, and
 *                 once one was published gsim_round, gsim_step and gsim_publish
 *                 (of any message) refuse those rounds too.
 *   slot reuse    a slot may be republished reuse_guard = (max(HistoryLength,
 *                 HistoryGossip) + promise ticks + 2) * rounds rounds after its
 *                 message's last first delivery, not earlier (GSIM_ESTATE from
 *                 the next call that checks the error flags). */
/* Subscription changes between ticks (Topic.Subscribe / Cancel through
 * pubsub.go:1051-1079 announcements and the router's Join / Leave,
 * gossipsub.go:1047-1124), for (peer, topic) pairs.  join = 1: Join(topic):
 * the peer announces the topic; its fanout peers (score >= 0, no backoff)
 * become the mesh, topped up to D with getPeers (not direct, no backoff,
 * score >= 0), or D such peers without a fanout; tracer.Graft and a GRAFT to
 * each.  join = 0: Leave(topic): the announcement is withdrawn; every mesh
 * peer gets tracer.Prune, a PRUNE whose backoff is UnsubscribeBackoff and an
 * UnsubscribeBackoff of its own.  A change that is already in effect is a
 * no-op.  Scores are the snapshot; getPeers keys use `tick` (call before that
 * tick's refresh, as gsim_set_connections); the GRAFT/PRUNE are handled with
 * the heartbeat's in control round 0.  Peers that withdrew a topic drop its
 * messages (pubsub.go:1094-1098).  Leave's PRUNEs carry no peer exchange.
 * JOIN / LEAVE / GRAFT / PRUNE trace events.  Single engine.
 * A pair whose peer is not below n or whose topic is not below n_topics (as
 * unsigned numbers: 0xFFFFFFFF is no topic) fails the whole call with
 * GSIM_EINVAL before anything changes; so does gsim_load_graph for a
 * subscription bit at or beyond n_topics, and gsim_create takes at most 64
 * topics (GSIM_ERANGE). */
int gsim_set_subscriptions(gsim_handle* h, const uint32_t* pairs, int32_t count, int32_t join, uint64_t tick,
                           int64_t now_ns);

/* ---- peer gater (peer_gater.go) ------------------------------------------
 * WithPeerGater(params) (peer_gater.go:161-186): every router's AcceptFrom
 * adds the random-early-drop gate of peer_gater.go:320-363 behind the
 * graylist (gossipsub.go:598-609): once the router's validation throttles
 * (a message with GSIM_VERDICT_THROTTLE) and throttle/validate reaches
 * Threshold within Quiet of the last throttle, a message from a peer is
 * accepted with probability (1 + deliver) / (1 + weighted total) of its
 * IP's counters, else dropped (AcceptControl; the receiver's IWANT promises
 * from that peer are forgotten, gossip_tracer.go:182-200).  Field for field
 * PeerGaterParams (peer_gater.go:31-55); durations in ns.  Restatement
 * (DESIGN.md §3.9 step 7): the gate is drawn per message copy (Philox), a
 * round's tracer events are added to the counters at the end of the round,
 * TopicDeliveryWeights in 2^-16 units, decayStats at every score refresh
 * (DecayInterval must equal the heartbeat interval); single engine, no
 * validation latency. */
typedef struct gsim_peer_gater_params {
    double threshold;          /* Threshold: throttle / validate ratio that turns the gate on */
    double global_decay;       /* GlobalDecay (validate, throttle) */
    double source_decay;       /* SourceDecay (per-IP counters) */
    int64_t decay_interval_ns; /* DecayInterval */
    double decay_to_zero;      /* DecayToZero */
    int64_t retain_stats_ns;   /* RetainStats: an IP's stats after its last peer left */
    int64_t quiet_ns;          /* Quiet: the gate turns off this long after the last throttle */
    double duplicate_weight;   /* DuplicateWeight */
    double ignore_weight;      /* IgnoreWeight */
    double reject_weight;      /* RejectWeight */
} gsim_peer_gater_params;

/* PeerGaterParams.validate (peer_gater.go:57-90), the reference's messages. */
int gsim_validate_peer_gater_params(const gsim_peer_gater_params* p, char* err, size_t errlen);
/* NewPeerGaterParams(threshold, globalDecay, sourceDecay) defaults (peer_gater.go:99-111). */
int gsim_default_peer_gater_params(double threshold, double global_decay, double source_decay,
                                   gsim_peer_gater_params* out);
/* Turn the gater on for every router (after gsim_msgs_init).  topic_weights:
 * TopicDeliveryWeights per topic index ([T], 0 = 1.0; multiples of 2^-16),
 * or NULL.  GSIM_EINVAL: invalid params or weights; GSIM_ESTATE: a shard,
 * a message with validation latency published, or DecayInterval not the
 * heartbeat interval. */
int gsim_set_peer_gater(gsim_handle* h, const gsim_peer_gater_params* p, const double* topic_weights);
/* Message copies dropped by the gate (AcceptControl) so far. */
int gsim_gater_throttled(gsim_handle* h, int64_t* out);
/* The gater state (host buffers, each may be NULL): per router validate,
 * throttle [N] and lastThrottle [N] (INT64_MIN: never); per connection
 * e (edge order) the counters deliver, duplicate, ignore, reject [4][E],
 * connected [E] and expire [E] of its IP group, held at the group's
 * representative edge (the row's lowest position of that IP; other
 * positions read 0). */
int gsim_gater_read(gsim_handle* h, double* validate, double* throttle, int64_t* last, double* counters4,
                    int32_t* connected, int64_t* expire);

typedef struct gsim_msg_config {
    int32_t ring;            /* message slots (live-message window), 1..8192 */
    int32_t rounds;          /* propagation rounds per heartbeat, >= 2 */
    int64_t t0_ns;           /* virtual time of tick 0 */
    int64_t heartbeat_ns;    /* heartbeat interval (GossipSubParams.HeartbeatInterval), > 0; its lower
                                bound: "Bounds of the clock" above */
    int64_t max_frontier;    /* 0: default.  > 0: a memory bound on the round lists of member-compacted
                                layouts (topic_slots > 0): the claim list holds this many entries
                                (default max(4 N, 2^20)), each forwarder list half as many; a round
                                that overflows either is completed by the word scans (k_commit,
                                k_send_tm) -- the same results, slower.  A sharded group also sizes
                                its frontier export with it (gsim_group_msgs_init) */
    int64_t max_arrivals;    /* capacity of the IWANT response queue per tick (0: max(8 N, 2^20)) */
    int64_t topic_slots;     /* 0: one ring shared by every topic, a message's slot is id % ring, and
                                every slot keeps a seen-set cell per peer.  > 0: per-topic sub-rings
                                (ring = n_topics * topic_slots): topic t owns slots [t * topic_slots,
                                (t + 1) * topic_slots) and its messages take them in publication
                                order; each slot keeps cells only for the peers holding topic t (its
                                slot mask), so the seen-set scales with the topics'
                                members, not with the network (timecache, pubsub.go:987-995) */
} gsim_msg_config;

/* The validation verdict every receiver reaches for a message (validation
 * is instantaneous here, validation.go:282-407), with the score tracer's
 * handling of it (score.go:693-827) and the gossip tracer's (gossip_tracer.go
 * 148-170).  The origin publishes its message whatever the verdict. */
#define GSIM_VERDICT_ACCEPT    0  /* DeliverMessage: P2 / P3 credit, forwarded, mcache.Put           */
#define GSIM_VERDICT_REJECT    1  /* RejectValidationFailed: seen, P4 for the first and every later
                                     sender, not forwarded                                          */
#define GSIM_VERDICT_IGNORE    2  /* RejectValidationIgnored: seen, no credit and no penalty for any
                                     copy, not forwarded                                            */
#define GSIM_VERDICT_THROTTLE  3  /* RejectValidationThrottled: as IGNORE                           */
#define GSIM_VERDICT_SIGNATURE 4  /* RejectInvalidSignature (before markSeen, validation.go:282-290):
                                     every copy's sender gets P4, the message is never seen (so IWANT
                                     asks again) and the IWANT promise is not fulfilled            */

/* One published message (Topic.Publish, topic.go:217-283, at its origin). */
typedef struct gsim_msg {
    uint64_t id;             /* message id; slot = id % ring */
    uint32_t topic;          /* dense topic index */
    uint32_t origin;         /* publishing peer (must be subscribed) */
    uint8_t  verdict;        /* GSIM_VERDICT_* at every receiver */
    uint8_t  vdelay;         /* validation latency at every receiver, in rounds (0..GSIM_MAX_VDELAY):
                                async validation (validation.go:246-407) — a receiver that first sees
                                the message in round g marks it seen then, and its Deliver/Reject
                                verdict, mcache.Put and forwarding happen at round g + vdelay; copies
                                arriving meanwhile are pending duplicates (score.go:719-725, 806-809).
                                Needs the topic-major delivery on a single engine (not a shard). */
    uint8_t  _pad[6];
} gsim_msg;

#define GSIM_MAX_VDELAY 7

/* Allocate the message ring and seen-set (after load_graph). */
int gsim_msgs_init(gsim_handle* h, const gsim_msg_config* cfg);
/* Publish `count` messages in round g: each slot is reset, the origin marks
 * the message seen (markSeen, pubsub.go:987-995) and puts it in its mcache
 * (gossipsub.go:976); the origin forwards it in round g+1. */
int gsim_publish(gsim_handle* h, const gsim_msg* msgs, int32_t count, int64_t round);
/* Propagation round g for the whole network:
 *  1. every peer that saw a message for the first time in round g-1 (or
 *     published it then) forwards it to its current mesh except the sender
 *     and the origin (gossipsub.go:975-1045; receivers do not forward an
 *     invalid message);
 *  2. every receiver handles those copies: AcceptFrom graylist
 *     (gossipsub.go:598-609), seen-set check (pubsub.go:1118-1162), then
 *     DeliverMessage / DuplicateMessage / RejectMessage (score.go:693-827);
 *     of several same-round copies the lowest connection is the first;
 *  3. control inbox of round g % rounds (rounds 0 and 1 of a heartbeat). */
int gsim_round(gsim_handle* h, int64_t round);
/* Host synchronisations the library has made in this process (stream
 * synchronisations and blocking copies, every handle and group together):
 * read it around a tick to count the host round trips the tick paid. */
int gsim_host_sync_count(uint64_t* out);
/* n_ticks whole heartbeat ticks in one call (SURVEY.md §8(b) gsim_step; the
 * heartbeat timer loop, gossipsub.go:1320-1343): for tick k = tick ..
 * tick + n_ticks - 1 at now = t0 + k * heartbeat (gsim_msg_config):
 * gsim_refresh_scores, gsim_heartbeat, then the rounds g = k * rounds ..
 * k * rounds + rounds - 1, each with its publications (gsim_publish) and
 * gsim_round.  msgs / round_off: the publications of the call's rounds,
 * msgs[round_off[q] .. round_off[q + 1]) in round q of the call
 * (n_ticks * rounds + 1 offsets, round_off[0] = 0; both NULL: none), uploaded
 * once.  The same results as the calls it stands for; the error flags the
 * heartbeat checks (response-queue overflow, early slot reuse) are read once
 * per call, at its end (a tick after a failing one ran on flagged state).
 * Single engines only (a sharded group steps through gsim_group_*). */
int gsim_step(gsim_handle* h, uint64_t tick, int32_t n_ticks, const gsim_msg* msgs, const int64_t* round_off);
/* Cumulative totals since gsim_msgs_init: out4 = {msg-edge deliveries
 * (accepted arrivals, duplicates included), first deliveries, duplicates,
 * graylisted arrivals}.  Synchronizes.  GSIM_ERANGE if the IWANT response
 * queue overflowed, GSIM_ESTATE if a slot was republished while its message
 * could still be gossiped (results are then incomplete). */
int gsim_msg_stats(gsim_handle* h, int64_t* out4);

/* Propagation report: how far each message still in the ring got, and how
 * fast (the reach of DeliverMessage, score.go:702-726, per message).  One row
 * per message whose publication round lies in [round_lo, round_hi), ordered
 * by (pub_round, slot); never-published slots are left out and a republished
 * slot reports its current message only.  A peer's latency is its first-seen
 * round minus pub_round, the first-seen round being what GSIM_F_SEEN shows
 * (the high word of the committed seen-set cell): with vdelay > 0 that is the
 * round the receiver's validation completes, not the
 * round the copy arrived.  The origin's own cell falls in bin 0;
 * sum(hist) == reached.  The histograms are reduced on the device from the
 * seen-set cells (no [ring][N] view is built). */
#define GSIM_REPORT_BINS 32
struct gsim_msg_report {
    uint64_t id;            /* gsim_msg.id of the slot's message                          */
    int64_t  pub_round;     /* round it was published in                                  */
    uint32_t slot, topic;
    uint32_t origin;        /* peer id (global id on a group)                             */
    uint32_t reached;       /* peers with a committed cell, the origin included           */
    uint32_t subscribers;   /* peers announcing `topic` now (gs.p.topics), the denominator */
    uint32_t max_latency;   /* largest latency among the reached peers (exact, not binned) */
    uint8_t  verdict, vdelay, _pad[6];
    uint32_t hist[GSIM_REPORT_BINS]; /* hist[d], d < 31: peers with latency d; hist[31]: latency >= 31 */
};  /* 176 bytes, hist at offset 48.  A struct tag without a typedef: the call below has
       the same name, and C keeps typedef names and function names in one namespace */
/* *n is always set to the number of selected messages; out == NULL or
 * cap == 0 counts only; 0 < cap < *n: GSIM_ERANGE, nothing written.
 * GSIM_ESTATE before gsim_msgs_init.  Pending claims are committed first, so
 * the call may follow any round.  Synchronizes; returns gsim_msg_stats's
 * GSIM_ERANGE / GSIM_ESTATE (rows written) when the delivery error flags are
 * set. */
int gsim_msg_report(gsim_handle* h, int64_t round_lo, int64_t round_hi,
                    struct gsim_msg_report* out, int64_t cap, int64_t* n);

/* Per-peer behaviour flags for adversarial configurations:
 * GSIM_BEHAVE_IGNORE_IWANT = the peer advertises (IHAVE) but never answers
 * IWANT (gossipsub_spam_test.go:134-286), so the requesters' promises break
 * and P7 penalties follow (gossip_tracer.go:79-115, gossipsub.go:1620-1625). */
#define GSIM_BEHAVE_IGNORE_IWANT 0x01u
int gsim_set_peer_behaviour(gsim_handle* h, const uint8_t* flags);
/* Cumulative gossip totals: out4 = {(receiver, message) pairs handleIHave
 * examined for an unseen advertised id, IWANT ids sent, messages sent in
 * answer to IWANT, broken promises penalised}. */
int gsim_gossip_stats(gsim_handle* h, int64_t* out4);

/* Aggregate census of the state (the network-wide analogue of the
 * reference's score inspection, score.go:448-500): out8 = {connected scored
 * edge-topic records, of those inMesh, non-zero firstMessageDeliveries,
 * non-zero meshMessageDeliveries, non-zero meshFailurePenalty, non-zero
 * invalidMessageDeliveries, router mesh links, tracked edges}. */
int gsim_census(gsim_handle* h, int64_t* out8);

/* Network report: the meshes and the score snapshot as distributions by peer
 * class, reduced on the device from the topic slot planes and the per-edge
 * score state (no [T][E] view is built).
 *
 * gsim_set_peer_classes: one byte per peer, each < GSIM_NET_CLASSES; NULL:
 * every peer is class 0 (the default).  C = 1 + the largest class set.  A
 * value >= GSIM_NET_CLASSES: GSIM_EINVAL, the classes in force stay.  The
 * classes key the report and nothing else; a new graph resets them.
 *
 * Defined on the ABI's edge-order views: for edge e of observer i (row
 * owner) with neighbour j = col[e] and topic t,
 *   mesh rows   one per (t, class of i), ordered (topic, cls).  The
 *               GSIM_TF_MESH bits of GSIM_F_TFLAGS[t][e] count where i announces
 *               t, the GSIM_TF_FANOUT bits where it does not; connection state is
 *               not consulted.  sum(deg_hist) == sum(out_hist) == members and
 *               sum(mesh_links) == the members' mesh sizes summed.
 *   score rows  one per (class of i, class of j), ordered (obs_cls, subj_cls),
 *               over GSIM_F_SCORE[e] (the snapshot) and GSIM_F_ESTATE[e].  hist
 *               covers connected non-NaN scores s: bin 0 holds s < edges[0],
 *               bin k edges[k-1] <= s < edges[k], bin n_edges s >=
 *               edges[n_edges-1]; +-inf fall in the end bins and count for
 *               min / max. */
#define GSIM_NET_CLASSES    4
#define GSIM_NET_DEG_BINS   32
#define GSIM_NET_OUT_BINS   8
#define GSIM_NET_SCORE_BINS 16
struct gsim_mesh_row {
    uint32_t topic, cls;
    uint32_t members;                /* peers of cls announcing topic (sub bit)                         */
    uint32_t max_degree;             /* largest mesh size among them, exact                             */
    uint32_t fanout_peers;           /* peers of cls NOT announcing topic whose GSIM_F_FANOUT_TOPICS bit is set */
    uint32_t _pad;
    uint64_t mesh_links[GSIM_NET_CLASSES]; /* members' GSIM_TF_MESH edges, by the neighbour's class     */
    uint64_t outbound_links;         /* of those, edges with outbound = 1                               */
    uint64_t fanout_links;           /* GSIM_TF_FANOUT edges of the non-announcing peers of cls         */
    uint32_t deg_hist[GSIM_NET_DEG_BINS];  /* members by mesh size d < 31; [31]: >= 31                  */
    uint32_t out_hist[GSIM_NET_OUT_BINS];  /* members by outbound mesh links o < 7; [7]: >= 7           */
};  /* 232 bytes */
struct gsim_score_row {
    uint32_t obs_cls, subj_cls;
    uint64_t connected;              /* edges with GSIM_ES_CONNECTED                                    */
    uint64_t retained;               /* GSIM_ES_TRACKED without GSIM_ES_CONNECTED                       */
    uint64_t nan;                    /* connected edges whose snapshot score is NaN                     */
    double   min, max;               /* over connected non-NaN edges; +inf / -inf when there are none   */
    uint64_t hist[GSIM_NET_SCORE_BINS];
};  /* 176 bytes */
int gsim_set_peer_classes(gsim_handle* h, const uint8_t* cls);
/* *n_mesh = T * C and *n_scores = C * C are always set.  A NULL array or a
 * cap of 0 skips that half (both: the call only counts); a cap that is too
 * small: GSIM_ERANGE, nothing written.  n_edges in 0..15, edges strictly
 * ascending without NaN, else GSIM_EINVAL.  GSIM_ESTATE before
 * gsim_load_graph.  Changes no state; synchronizes. */
int gsim_net_report(gsim_handle* h, const double* edges, int32_t n_edges,
                    struct gsim_mesh_row* mesh, int64_t mesh_cap, int64_t* n_mesh,
                    struct gsim_score_row* scores, int64_t score_cap, int64_t* n_scores);

/* Peer delivery report: the propagation report transposed.  The same seen-set
 * cells, streamed once, reduced per peer and per (topic, class of the
 * receiving peer) instead of per message: how many of the messages it
 * subscribes to a peer received, how late, and who delivered them first (the
 * victims' delivery ratio and the attacker class's share of their first
 * deliveries are what eclipse, censorship and sybil studies read).  No
 * [ring][N] view is built.
 *
 * Defined on the ABI's views: for peer p and selected message m (ring slot s,
 * topic t, published in pub_round by origin),
 *   selection     the messages of gsim_msg_report(round_lo, round_hi): pub_round
 *                 in the window, never-published slots left out, a reused slot
 *                 its current message only.
 *   received      GSIM_F_SEEN[s][p] holds a round (a committed cell); the
 *                 latency is that round minus pub_round, as gsim_msg_report's
 *                 (with vdelay > 0 the round p's validation completes).
 *   expected      p announces t now (its sub bit, gs.p.topics); missed: it does
 *                 and the cell is not committed.  received + missed >= expected,
 *                 equal unless p holds a cell of a topic it does not announce
 *                 (a fanout publisher, a peer that left the topic).
 *   first sender  the low word of the committed cell, the peer whose copy p saw
 *                 first, counted by that peer's class (gsim_set_peer_classes;
 *                 every peer class 0 by default).  The origin's own cell has no
 *                 sender: it counts in `own` and in no first_from bin, so
 *                 sum(first_from) == received - own in every row.
 *   class rows    one per (t, class of p), ordered (topic, cls), over EVERY
 *                 peer whatever the peer range; expected == peers * messages;
 *                 sum(hist) == received. */
struct gsim_peer_row {
    uint32_t expected;   /* selected messages whose topic the peer announces now (sub bit)          */
    uint32_t received;   /* selected messages with a committed cell of this peer, its own included  */
    uint32_t own;        /* of those, the peer's own publications (origin == peer)                  */
    uint32_t missed;     /* selected messages whose topic it announces and for which it has no committed cell */
    uint32_t lat_max, _pad;
    uint64_t lat_sum;    /* sum over received of first-seen round - pub_round (own: 0)              */
    uint32_t first_from[GSIM_NET_CLASSES]; /* received - own, by the class of the first sender      */
};  /* 48 bytes */
struct gsim_peer_class_row {
    uint32_t topic, cls;
    uint32_t peers;      /* peers of cls announcing topic now                                      */
    uint32_t messages;   /* selected messages of topic                                             */
    uint64_t expected, received, own, missed, lat_sum;   /* expected == (u64)peers * messages      */
    uint32_t lat_max, _pad;
    uint64_t first_from[GSIM_NET_CLASSES];
    uint64_t hist[GSIM_REPORT_BINS];   /* received by latency d < 31; [31]: >= 31; sum == received  */
};  /* 352 bytes, first_from at offset 64, hist at 96 */
/* peers == NULL skips the per-peer half; otherwise peer_hi - peer_lo rows are
 * written for the peers [peer_lo, peer_hi); a range outside 0 <= peer_lo <=
 * peer_hi <= N: GSIM_EINVAL.  *n_classes = T * C (as gsim_net_report's mesh
 * rows) and *n_msgs, the number of selected messages, are always set.
 * classes == NULL or class_cap == 0 skips the class rows; 0 < class_cap <
 * T * C: GSIM_ERANGE, nothing written.  GSIM_ESTATE before gsim_msgs_init.
 * Pending claims are committed first, so the call may follow any round.
 * Changes no state; synchronizes; returns gsim_msg_stats's GSIM_ERANGE /
 * GSIM_ESTATE (rows written) when the delivery error flags are set. */
int gsim_peer_report(gsim_handle* h, int64_t round_lo, int64_t round_hi,
                     int64_t peer_lo, int64_t peer_hi, struct gsim_peer_row* peers,
                     struct gsim_peer_class_row* classes, int64_t class_cap,
                     int64_t* n_classes, int64_t* n_msgs);
/* Debug accessor: how the last gsim_peer_report that ran its reduction was
 * launched, out3 = {waves of 64 peers, parts the selected slots were split
 * into (1: every lane walks all of them and stores its row; > 1: the parts'
 * partial sums meet in atomics on the rows), selected messages}. */
int gsim_peer_report_launch(gsim_handle* h, int64_t* out3);

/* Relay report: the first-delivery forest read from the sender's side.  Every
 * committed seen-set cell names the peer whose copy the receiver saw first, so
 * the tree that actually delivered each message still in the ring is resident
 * on the device; this call counts who carried it (the quantity P2 rewards,
 * markFirstMessageDelivery, score.go:919-946, summed at the credited peer), how
 * wide and how deep the trees are and how many rounds each hop took.  No
 * [ring][N] view is built.
 *
 * Defined on the ABI's views.  Selection and pending claims as
 * gsim_peer_report's.  For a selected message m with origin o and a peer p
 * holding a committed cell:
 *   parent(p)      the cell's first sender; the origin's cell has none.
 *   children(q, m) the peers whose parent in m is q.
 *   depth(p)       depth(o) = 0, depth(p) = depth(parent(p)) + 1.  A parent's
 *                  first-seen round is strictly smaller than its child's (also
 *                  with vdelay: the cell stores the completion round, forwarding
 *                  happens a round later), so the structure is a tree.
 *   orphan         p's parent holds no committed cell in the slot, or one with a
 *                  round >= p's (or p's cell is older than the publication): p
 *                  counts in `orphans`, has no depth and no delay, and the call
 *                  returns GSIM_ESTATE after writing the rows.  Its descendants
 *                  take their depth from it as a root of depth 0.
 *   delay(p)       seen[p] - seen[parent(p)] >= 1; a hop of more than 1 + vdelay
 *                  rounds was pulled (IWANT) rather than pushed.
 * children counts reach ring * (a sender's degree), past 32 bits at the ABI's
 * limits (ring 8192, E < 2^30), so every sum of children is a u64; a single
 * message's children(q, m) is at most q's degree and stays a u32. */
struct gsim_relay_row {          /* one per peer q of [peer_lo, peer_hi): the sender's side */
    uint32_t held;               /* selected messages with a committed cell of q                 */
    uint32_t relayed_msgs;       /* of those, messages with children(q, m) > 0                   */
    uint32_t max_children;       /* largest children(q, m) of one message                        */
    uint32_t _pad;
    uint64_t children;           /* sum over m of children(q, m)                                 */
    uint64_t own_children;       /* of those, in messages q originated                           */
    uint64_t children_to[GSIM_NET_CLASSES]; /* children by the class of the receiving child; sum == children */
};  /* 64 bytes, children at offset 16, children_to at 32 */
struct gsim_relay_class_row {    /* one per (topic, class of the SENDER), ordered (topic, cls), over every peer */
    uint32_t topic, cls;
    uint32_t peers;              /* peers of cls announcing topic now                            */
    uint32_t messages;           /* selected messages of topic                                   */
    uint64_t held;               /* (q, m): q of cls holds a committed cell of m                 */
    uint64_t relayed;            /* of those, children(q, m) > 0                                 */
    uint64_t children;           /* first deliveries given by senders of cls                     */
    uint32_t max_children, _pad; /* largest children(q, m), exact                                */
    uint64_t children_to[GSIM_NET_CLASSES]; /* children by the child's class; sum == children     */
    uint64_t fanout[GSIM_REPORT_BINS]; /* holders by children(q, m) = k < 31; [31]: >= 31; leaves in [0]; sum == held */
};  /* 336 bytes, children_to at offset 48, fanout at 80 */
struct gsim_relay_msg_row {      /* one per selected message, ordered (pub_round, slot) */
    uint64_t id;
    int64_t  pub_round;
    uint32_t slot, topic;
    uint32_t origin;
    uint32_t reached;            /* peers with a committed cell, the origin included             */
    uint32_t relays;             /* holders with at least one child                              */
    uint32_t max_children;       /* the widest holder's children ...                             */
    uint32_t max_children_peer;  /* ... and its id, the lowest on a tie (0 when nobody relayed)  */
    uint32_t depth_max;          /* exact                                                        */
    uint32_t orphans;
    uint8_t  verdict, vdelay, _pad[2];
    uint32_t depth_hist[GSIM_REPORT_BINS]; /* depth d < 31 in [d], >= 31 in [31]; sum == reached - orphans */
    uint32_t delay_hist[8];      /* delays 1..7 in [0..6], >= 8 in [7]; sum == reached - 1 - orphans */
};  /* 216 bytes, depth_hist at offset 56, delay_hist at 184 */
/* Any of the three outputs may be NULL (or its cap 0) to skip that part; all
 * three skipped: the call only counts.  *n_classes = T * C and *n_msgs, the
 * selected messages, are always set; a cap that is too small: GSIM_ERANGE,
 * nothing written.  peers: peer_hi - peer_lo rows; a range outside 0 <= peer_lo
 * <= peer_hi <= N: GSIM_EINVAL.  GSIM_ESTATE before gsim_msgs_init.  The class
 * and message rows cover every peer whatever the peer range.  Message rows need
 * every latency below 16383 rounds (else GSIM_ERANGE, rows written).  A first
 * sender that is no local peer: GSIM_ESTATE.  Changes no state; synchronizes;
 * returns gsim_msg_stats's GSIM_ERANGE / GSIM_ESTATE (rows written) when the
 * delivery error flags are set. */
int gsim_relay_report(gsim_handle* h, int64_t round_lo, int64_t round_hi,
                      int64_t peer_lo, int64_t peer_hi, struct gsim_relay_row* peers,
                      struct gsim_relay_class_row* classes, int64_t class_cap, int64_t* n_classes,
                      struct gsim_relay_msg_row* msgs, int64_t msg_cap, int64_t* n_msgs);
/* Debug: the byte budget of the per-batch scratch (6 bytes per (slot of the
 * batch, peer); 0: the default, 256 MiB).  The results do not depend on it. */
int gsim_relay_report_budget(gsim_handle* h, int64_t bytes);
/* Debug accessor of the last gsim_relay_report that ran: out4 = {slots per
 * batch, batches, depth passes in all, selected messages}. */
int gsim_relay_report_launch(gsim_handle* h, int64_t* out4);

/* Score report: why a score is what it is.  The live score of every record
 * decomposed into the reference's P1..P7 (score.go:265-342) as distributions
 * per (observer class, subject class), reduced on the device in one read-only
 * pass over the topic slot planes; optionally under other parameters than the
 * engine's ("what if MeshMessageDeliveriesWeight were -0.5?").  No [T][E] view
 * is built and no state changes.
 *
 * Defined on the ABI's edge-order views: for every edge e of observer i with
 * subject j = col[e], on the CURRENT counters (not GSIM_F_SCORE, the snapshot
 * of the last refresh):
 *   counters    pending meshMessageDeliveries increments are applied with the
 *               ENGINE's MeshMessageDeliveriesCap (they are state, not scoring);
 *               meshTime is derived where the engine keeps it lazily; P6 is
 *               taken as last derived (GSIM_F_P6): the report does not recompute
 *               IP colocation.
 *   records     a GSIM_ES_CONNECTED record counts everywhere; a GSIM_ES_TRACKED
 *               record that is not connected counts in `retained` only; any other
 *               record counts nowhere.  (A connected record without
 *               GSIM_ES_TRACKED has no peerStats: every part of it is 0 and it
 *               counts in no topic row, as its score is 0.)
 *   per topic   with the parameters tp[t], pp (the engine's or the what-if
 *               ones), per scored topic in ascending t:
 *                 p1  = in_mesh ? min((double)(meshTime / quantum), cap) * w1 : 0
 *                       (0 when the quantum is 0)
 *                 p2  = first * w2
 *                 p3  = (active && meshd < thr) ? ((thr - meshd) * (thr - meshd)) * w3 : 0
 *                 p3b = fail * w3b
 *                 p4  = (invalid * invalid) * w4
 *                 ts  = ((((0 + p1) + p2) + p3) + p3b) + p4
 *   parts       P1..P4: part_k = sum_t (p_k * TopicWeight_t), from 0.0 in
 *               ascending t; TOPICS = sum_t ts * TopicWeight_t, then capped by
 *               TopicScoreCap when that is > 0; P5 = p5[j] * AppSpecificWeight;
 *               P6 = p6 * IPColocationFactorWeight; P7 = bp > thr7 ?
 *               ((bp - thr7) * (bp - thr7)) * w7 : 0; TOTAL = ((TOPICS + P5) + P6)
 *               + P7.  fp64, every operation rounded separately: TOTAL is bit for
 *               bit the live score (what gsim_refresh_scores would store now,
 *               decay aside).  The parts P1..P4 are sums of their own and need not
 *               add up to TOPICS or TOTAL in the last bits.
 *   hist        the bin of a part's value x, integer arithmetic on the f64 bits,
 *               no caller-chosen edges (the parts span ten orders of magnitude):
 *               zero of either sign: bin 16; otherwise k = floor(log2 |x|) (the
 *               unbiased binary exponent; a denormal's is below -1022) and m =
 *               clamp(floor((k + 8) / 2), 0, 15), +-inf: m = 15; x < 0: bin 15 - m,
 *               x > 0: bin 17 + m.  So bin 0 is x <= -2^22, bin 15 is -2^-6 < x <
 *               0, bin 17 is 0 < x < 2^-6, bin 32 is x >= 2^22, and in between bin
 *               17 + m is 2^(2m-8) <= x < 2^(2m-6).  NaN counts in `nan`, not in
 *               hist, min or max.
 *   cause       the dominant negative part of a record: the smallest of (P3, P3B,
 *               P4, P5, P6, P7) among those < 0 (NaN never qualifies, ties go to
 *               the first in that order), NONE when none is negative.
 *               cause[b][c] counts the connected records with a non-NaN TOTAL in
 *               bin b of `edges` (gsim_net_report's rule) and cause c: its sum
 *               over c is gsim_net_report's hist for the same edges while the
 *               live total equals the snapshot (right after gsim_refresh_scores).
 *   topic rows  flags of the connected tracked records per (topic, class pair);
 *               the rows of a topic that is not scored are zero. */
#define GSIM_SR_PARTS  10   /* P1 P2 P3 P3B P4 TOPICS P5 P6 P7 TOTAL, in this order */
#define GSIM_SR_BINS   33
#define GSIM_SR_CAUSES  7   /* P3 P3B P4 P5 P6 P7 NONE */
enum {
    GSIM_SR_P1 = 0, GSIM_SR_P2, GSIM_SR_P3, GSIM_SR_P3B, GSIM_SR_P4, GSIM_SR_TOPICS,
    GSIM_SR_P5, GSIM_SR_P6, GSIM_SR_P7, GSIM_SR_TOTAL
};
struct gsim_score_part_row {          /* one per (obs_cls, subj_cls, part), in that order */
    uint32_t obs_cls, subj_cls, part, _pad;
    uint64_t nan;                     /* connected records whose value of this part is NaN */
    double   min, max;                /* over connected non-NaN values; +inf / -inf when none */
    uint64_t hist[GSIM_SR_BINS];      /* fixed signed-log bins, above */
};  /* 304 bytes */
struct gsim_score_cause_row {         /* one per (obs_cls, subj_cls) */
    uint32_t obs_cls, subj_cls;
    uint64_t connected, retained;     /* as gsim_score_row */
    uint64_t nan;                     /* connected records whose TOTAL is NaN */
    uint64_t capped;                  /* connected records whose topic sum exceeded TopicScoreCap (> 0) */
    uint64_t cause[GSIM_NET_SCORE_BINS][GSIM_SR_CAUSES];
                                      /* [bin of TOTAL on the caller's edges, gsim_net_report's rule]
                                         [dominant negative part]; non-NaN totals only */
};  /* 936 bytes */
struct gsim_score_topic_row {         /* one per (topic, obs_cls, subj_cls); unscored topics: zeros */
    uint32_t topic, obs_cls, subj_cls, _pad;
    uint64_t in_mesh;                 /* GSIM_TF_IN_MESH */
    uint64_t p1_capped;               /* in mesh and (double)(meshTime / quantum) > TimeInMeshCap */
    uint64_t first_at_cap;            /* first >= FirstMessageDeliveriesCap */
    uint64_t active;                  /* GSIM_TF_ACTIVE */
    uint64_t p3_deficit;              /* active and meshd < MeshMessageDeliveriesThreshold */
    uint64_t p3b_nonzero, p4_nonzero; /* fail != 0, invalid != 0 */
    uint64_t negative;                /* ts * TopicWeight < 0 */
};  /* 80 bytes */
struct gsim_score_what_if {           /* NULL: the engine's own parameters */
    const gsim_peer_score_params*  peer;    /* NULL: the engine's */
    const gsim_topic_score_params* topics;  /* NULL: the engine's; else n_topics == T entries */
    int32_t n_topics, _pad;
};
/* *n_parts = C * C * 10, *n_causes = C * C and *n_topics = T * C * C are always
 * set (C: the classes of gsim_set_peer_classes).  A NULL array or a cap of 0
 * skips that third (all three: the call only counts); a cap that is too small:
 * GSIM_ERANGE, nothing written.  edges / n_edges as gsim_net_report's.  What-if
 * parameters pass gsim_validate_peer_params / gsim_validate_topic_params and
 * n_topics must equal T, else GSIM_EINVAL with the validator's text in
 * gsim_last_error; they are used by this call only.  GSIM_ESTATE before
 * gsim_load_graph.  Pending first deliveries are committed first (they are P2
 * credits), so the call may follow any round.  Changes no state; synchronizes. */
int gsim_score_report(gsim_handle* h, const struct gsim_score_what_if* what_if,
                      const double* edges, int32_t n_edges,
                      struct gsim_score_part_row*  parts,  int64_t part_cap,  int64_t* n_parts,
                      struct gsim_score_cause_row* causes, int64_t cause_cap, int64_t* n_causes,
                      struct gsim_score_topic_row* topics, int64_t topic_cap, int64_t* n_topics);

/* Mesh path report: the mesh of one topic as a graph.  Hop distances from up
 * to GSIM_PATH_SOURCES sources at once over the routers' mesh links, by a
 * level-synchronous traversal on the device (one bit per source in a 64-bit
 * word per peer), with a read-only what-if: the peers of some classes stop
 * relaying.  The distances are what eager push costs: a router forwards a
 * message to gs.mesh[topic] (and a publisher outside the topic to
 * gs.fanout[topic]), gossipsub.go:975-1045, one hop per round.
 *
 * Defined on the ABI's edge-order views, with gsim_net_report's convention:
 * for topic t the mesh digraph has an arc i -> j for edge e of row i with
 * col[e] = j iff GSIM_F_TFLAGS[t][e] & GSIM_TF_MESH, i announces t (sub bit)
 * and j announces t; connection state is not consulted.  A source that
 * announces t starts at hop 0 and expands over its arcs.  A source that does
 * not (a fanout publisher) expands once, at level 0, over its GSIM_TF_FANOUT
 * edges into peers that announce t, and is itself neither reached nor a
 * subscriber.  hops(s, p) is the BFS distance.
 *   blocked   a bit mask over the peer classes (gsim_set_peer_classes).  A peer
 *             whose class is in it is reached and counted but never expanded,
 *             unless it is the source itself (which forwards its own
 *             publication).  0: the plain distances.
 *   max_hops  0: until every frontier is empty.  > 0: that many levels; peers
 *             further away count as unreached and `truncated` is set in the
 *             rows whose frontier (the unblocked peers at distance max_hops)
 *             was not empty.
 * Duplicated sources are allowed; their rows are equal. */
#define GSIM_PATH_SOURCES 64
struct gsim_mesh_path_row {                 /* one per source, in the caller's order */
    uint32_t source, topic;
    uint32_t reached;                       /* peers announcing topic with a finite distance (the source if it announces) */
    uint32_t subscribers;                   /* peers announcing topic */
    uint32_t max_hops;                      /* largest finite distance, exact */
    uint32_t truncated;                     /* 1: max_hops stopped a non-empty frontier */
    uint32_t reached_cls[GSIM_NET_CLASSES]; /* reached, by the reached peer's class */
    uint32_t members_cls[GSIM_NET_CLASSES]; /* subscribers, by class */
    uint32_t hist[GSIM_REPORT_BINS];        /* hist[d], d < 31: peers at distance d; [31]: >= 31; sum == reached */
};  /* 184 bytes, reached_cls at offset 24, members_cls at 40, hist at 56 */
/* 1 <= n_sources <= GSIM_PATH_SOURCES.  GSIM_EINVAL: a source >= N, a topic
 * outside 0..T-1, a `blocked` bit at or above the class count, a negative
 * max_hops.  reach_count / hop_sum ([N] each, or NULL): per peer, how many of
 * the sources reach it and the sum of its finite distances (0 for a peer no
 * source reaches).  GSIM_ESTATE before gsim_load_graph.  Changes no state;
 * synchronizes (one counted host read per level). */
int gsim_mesh_paths(gsim_handle* h, int32_t topic, const uint32_t* sources, int32_t n_sources,
                    uint32_t blocked, int32_t max_hops, struct gsim_mesh_path_row* rows,
                    uint32_t* reach_count, uint32_t* hop_sum);

/* ---- trace export (pb/trace.proto, trace.go) ------ */
/* The events the routers [peer_lo, peer_hi) hand their tracer
 * (pubsubTracer, trace.go:70-530), one record each, in the order of
 * pb/trace.proto's TraceEvent.Type:
 *   PUBLISH_MESSAGE   the origin publishes (trace.go:70-91)
 *   REJECT_MESSAGE    first reception of a message that failed validation
 *                     (reason = the verdict), or every copy with a bad
 *                     signature (105-134)
 *   DUPLICATE_MESSAGE a copy of a message already seen (136-164)
 *   DELIVER_MESSAGE   first reception of an accepted message (166-194)
 *   ADD_PEER / REMOVE_PEER   connections made or lost (196-248)
 *   RECV_RPC / SEND_RPC  the message RPCs (trace.go:250-297): every copy a
 *                     router forwards is its own RPC (Publish -> sendRPC per
 *                     peer, gossipsub.go:1032-1044, 1195-1200), SEND_RPC at
 *                     the sender (other = the receiver) and RECV_RPC at the
 *                     receiver (other = the sender; handleIncomingRPC,
 *                     pubsub.go:1039, before AcceptFrom), reason 0; an
 *                     advertiser's IWANT answers to one requester in a round
 *                     are one RPC (handleIWant, gossipsub.go:700-739): reason
 *                     1, sent the round before they arrive, one record per
 *                     message (gsim_trace_encode joins them); reason 2:
 *                     handleIHave's IWANT request (HandleRPC -> sendRPC,
 *                     gossipsub.go:611-627), SEND_RPC at the requester in
 *                     control round 0 and RECV_RPC at the advertiser in round
 *                     1, one record per requested id (encoded as one
 *                     ControlMeta.iwant; ids in (topic, id) order).
 *                     Modelled difference: the reference's HandleRPC sends the
 *                     IWANT request, the IWANT answers and the PRUNEs of one
 *                     incoming RPC as ONE sendRPC (gossipsub.go:617-627); here
 *                     the request (control round 0) and the answers (round 1)
 *                     happen in different rounds, so they are separate RPCs
 *                     (no reference fixture pins this: parity unpinned).  The
 *                     heartbeat's control / IHAVE RPCs are traced from their
 *                     encoding (gsim_trace_rpc_encode, include/gsim_wire.h)
 *   JOIN / LEAVE      gsim_set_subscriptions (1047-1124)
 *   GRAFT / PRUNE     the router adds / drops a mesh link: heartbeat,
 *                     handleGraft, handlePrune (468-520)
 * Not produced: DROP_RPC (no outbound queue is modelled, so no RPC is
 * dropped: doDropRPC needs a full queue, gossipsub.go:1185-1200).  Copies
 * dropped by AcceptFrom produce no message event, as in pushMsg. */
#define GSIM_TRACE_PUBLISH_MESSAGE   0
#define GSIM_TRACE_REJECT_MESSAGE    1
#define GSIM_TRACE_DUPLICATE_MESSAGE 2
#define GSIM_TRACE_DELIVER_MESSAGE   3
#define GSIM_TRACE_ADD_PEER          4
#define GSIM_TRACE_REMOVE_PEER       5
#define GSIM_TRACE_RECV_RPC          6   /* a message RPC received: reason 0 a forwarded message, 1 an IWANT answer */
#define GSIM_TRACE_SEND_RPC          7   /* a message RPC sent (same reasons)                                     */
#define GSIM_TRACE_JOIN              9
#define GSIM_TRACE_LEAVE             10
#define GSIM_TRACE_GRAFT             11
#define GSIM_TRACE_PRUNE             12

typedef struct gsim_trace_event {
    int64_t  timestamp_ns;    /* TraceEvent.timestamp */
    uint64_t msg_id;          /* gsim_msg.id of message events */
    uint32_t peer;            /* TraceEvent.peerID: the router */
    uint32_t other;           /* receivedFrom (message events); the peer (ADD/REMOVE_PEER, GRAFT, PRUNE) */
    int32_t  topic;           /* message events, GRAFT, PRUNE; -1 otherwise */
    uint8_t  type;            /* GSIM_TRACE_* */
    uint8_t  reason;          /* REJECT_MESSAGE: GSIM_VERDICT_* */
    uint16_t _pad;
} gsim_trace_event;

/* Start tracing the routers [peer_lo, peer_hi) into a device buffer of cap
 * events (0: stop and free it).  A shard of a group: gsim_group_trace_config. */
int gsim_trace_config(gsim_handle* h, uint32_t peer_lo, uint32_t peer_hi, int64_t cap);

/* The events traced since the last call, sorted by (timestamp, peer, type,
 * other, reason, topic, msg_id); *n is their number (GSIM_ERANGE, nothing lost from
 * the buffer, when it exceeds cap; GSIM_ERANGE when the device buffer
 * overflowed). */
int gsim_trace_read(gsim_handle* h, gsim_trace_event* out, int64_t cap, int64_t* n);

/* ---- score tracer events: peerScore's RawTracer surface from outside ------
 * (trace.go:27-60, score.go:88; SURVEY.md §8(b) part 2).  A caller that owns
 * the routers -- an event-driven simulator, a replay of a TraceEvent stream, a
 * Go router bound through cgo -- hands the calls its routers' score tracers
 * would receive to the engine in batches; the engine keeps every router's
 * peerStats and delivery records (score.go:90-120) and scores as usual.
 *
 * Ordering: the events of one observer take effect in array order; observers
 * are independent (an observer's events touch only its own records about its
 * neighbours and its own delivery records), so the result does not depend on
 * how observers interleave in the array, which need not be grouped or sorted.
 *
 * Each event is the RawTracer method of its kind on the observer's peerScore,
 * as the CPU oracle restates it (oracle/oracle.c).  Changed: first / meshd /
 * fail / invalid / graft / meshTime, the score bits of GSIM_F_TFLAGS, and bp.
 * Router state (mesh flags, connections, backoff, the control inbox) is not
 * touched, nor are the peer gater, the IWANT promises and the trace export.
 * Connections still change through gsim_set_connections (AddPeer /
 * RemovePeer).  A peer without peerStats and a topic without score parameters
 * are the reference's silent returns (the delivery record is still updated). */
#define GSIM_EV_VALIDATE    0   /* ValidateMessage   score.go:693-700 */
#define GSIM_EV_DELIVER     1   /* DeliverMessage    score.go:702-726 */
#define GSIM_EV_REJECT      2   /* RejectMessage     score.go:728-793, arg = GSIM_REJECT_* */
#define GSIM_EV_DUPLICATE   3   /* DuplicateMessage  score.go:795-827 */
#define GSIM_EV_GRAFT       4   /* Graft             score.go:649-667 */
#define GSIM_EV_PRUNE       5   /* Prune             score.go:669-691 */
#define GSIM_EV_ADD_PENALTY 6   /* AddPenalty        score.go:391-405, arg = count */
/* RejectMessage reasons, in the order of tracer.go:28-38 */
#define GSIM_REJECT_BLACKLISTED_PEER      0
#define GSIM_REJECT_BLACKLISTED_SOURCE    1
#define GSIM_REJECT_MISSING_SIGNATURE     2
#define GSIM_REJECT_UNEXPECTED_SIGNATURE  3
#define GSIM_REJECT_UNEXPECTED_AUTH_INFO  4
#define GSIM_REJECT_INVALID_SIGNATURE     5
#define GSIM_REJECT_VALIDATION_QUEUE_FULL 6
#define GSIM_REJECT_VALIDATION_THROTTLED  7
#define GSIM_REJECT_VALIDATION_FAILED     8
#define GSIM_REJECT_VALIDATION_IGNORED    9
#define GSIM_REJECT_SELF_ORIGIN           10

typedef struct gsim_score_event {   /* 32 bytes */
    uint64_t mid;        /* message id (message events) */
    int64_t  now_ns;     /* time.Now() as the tracer saw it */
    uint32_t observer;   /* the router whose peerScore receives the call */
    uint32_t peer;       /* msg.ReceivedFrom / the grafted, pruned, penalised peer */
    uint16_t arg;        /* reject reason / penalty count */
    uint8_t  topic, kind;
    uint8_t  _pad[4];
} gsim_score_event;

/* Size the delivery records: room for records_cap records (one per (observer,
 * message id) alive at a time) and peers_cap entries of their peers lists
 * (deliveryRecord.peers); seen_ttl_ns is the records' lifetime (0:
 * TimeCacheDuration, 120 s).  Calling it again drops every record.  Needs a
 * graph (GSIM_ESTATE); a new graph drops the configuration.  A shard of a
 * group: GSIM_ESTATE (as the three calls below). */
int gsim_score_tracer_config(gsim_handle* h, int64_t records_cap, int64_t peers_cap, int64_t seen_ttl_ns);

/* Apply n events.  The whole batch is checked first: GSIM_EINVAL, with the
 * first offending index in gsim_last_error and nothing applied, on an unknown
 * kind, a reject reason above 10, an observer or peer >= N, a peer that is no
 * connection (CSR neighbour) of the observer, a topic >= T or one the observer
 * has not announced (every kind but ADD_PENALTY, which has no topic), or a
 * time that goes backwards for an observer (within the batch or against its
 * last event of an earlier batch).  GSIM_ERANGE, nothing applied, when the
 * batch could need more records or peers-list entries than are free: one
 * record per event that reaches getRecord (VALIDATE, DELIVER, DUPLICATE,
 * REJECT with a validation reason 7-9), one entry per DUPLICATE.  Entries of a
 * released list (RejectMessage) are free again after the next
 * gsim_score_tracer_gc.  GSIM_ESTATE before gsim_score_tracer_config.
 * Synchronizes. */
int gsim_score_tracer_events(gsim_handle* h, const gsim_score_event* ev, int64_t n);

/* gcDeliveryRecords (score.go:587-592, 863-877): drop every record with
 * now_ns > expire (strict); their space is reusable afterwards, and an id seen
 * again is a fresh record.  Per-observer times are non-decreasing and the TTL
 * is one constant, so expiry order is creation order: exactly the records the
 * reference's queue-head loop drops.  Synchronizes. */
int gsim_score_tracer_gc(gsim_handle* h, int64_t now_ns);

/* out4 = {live records, live peers-list entries, events applied, records
 * collected} since gsim_score_tracer_config. */
int gsim_score_tracer_stats(gsim_handle* h, int64_t* out4);

/* Diagnostic: out2 = {score records whose pending meshMessageDeliveries
 * increments (left by simulated rounds, not yet folded into the counter) an
 * event settled before it read or changed the counter, since
 * gsim_score_tracer_config; 1 while the engine holds such increments}. */
int gsim_score_tracer_settled(gsim_handle* h, int64_t* out2);

/* ---- router state: the seen cache and the IWANT promises from outside ------
 * The two id-keyed structures a router consults around the score tracer, for
 * the same callers (they own the routing; the engine keeps the state):
 *   the seen cache (timecache/, pubsub.go:986-995, 1150-1162,
 *   validation.go:307), which tells a ValidateMessage from a DuplicateMessage;
 *   the gossip tracer's promises (gossip_tracer.go:48-200), whose broken ones
 *   are the only source of P7 (gossipsub.go:1620-1625 -> AddPenalty).
 * Both are kept per observer, as the CPU oracle restates them (orc_tcache_*,
 * orc_gtracer_*).  The message cache is not here: it belongs with the
 * payloads, which the caller holds.
 *
 * Ordering: as for the score tracer.  The events of one observer take effect
 * in array order, observers are independent, the array need not be grouped,
 * result[k] belongs to ev[k].
 *
 * The engine's own seen-set, promise ring and trace (gsim_round) are neither
 * read nor written by these calls.  Single engines only: a shard of a group
 * returns GSIM_ESTATE from every call. */
#define GSIM_RS_SEEN_ADD 0   /* markSeen = TimeCache.Add: result 1 new, 0 already there */
#define GSIM_RS_SEEN_HAS 1   /* seenMessage = TimeCache.Has: result 1 there, 0 not */
#define GSIM_RS_PROMISE  2   /* gossipTracer.AddPromise(peer, ids) with the id already picked (the caller
                                draws rand.Intn): result 1 a new (id, peer) promise expiring at
                                now + followup, 0 it existed (its expiry is not renewed,
                                gossip_tracer.go:65-74) */
#define GSIM_RS_FULFILL  3   /* fulfillPromise(id) (gossip_tracer.go:119-141): every peer's promise of
                                that id at the observer is dropped; result = how many, saturating at 255 */

typedef struct gsim_router_event {   /* 32 bytes */
    uint64_t mid;        /* message id */
    int64_t  now_ns;     /* time.Now() as the router saw it */
    uint32_t observer;   /* the router whose seen cache / gossip tracer receives the call */
    uint32_t peer;       /* PROMISE: the peer that advertised the id; ignored otherwise */
    uint8_t  kind;       /* GSIM_RS_* */
    uint8_t  _pad[7];
} gsim_router_event;

typedef struct gsim_broken_row {     /* GetBrokenPromises: one (observer, peer) and its count */
    uint32_t observer, peer, count, _pad;
} gsim_broken_row;

/* Size both structures: room for seen_cap seen entries and promises_cap
 * promises alive at a time, over all observers.  strategy: 0 first-seen (the
 * expiry is fixed at the first Add), 1 last-seen (every Add and every
 * successful Has sets it to now + ttl).  seen_ttl_ns 0: TimeCacheDuration,
 * 120 s; followup_ns 0: the engine's IWantFollowupTime.  Calling it again
 * drops everything.  Needs a graph (GSIM_ESTATE); a new graph drops the
 * configuration. */
int gsim_router_state_config(gsim_handle* h, int64_t seen_cap, int64_t promises_cap, int32_t strategy,
                             int64_t seen_ttl_ns, int64_t followup_ns);

/* Apply n events; result[k] (may be NULL) receives ev[k]'s answer.  The whole
 * batch is checked first: GSIM_EINVAL, with the first offending index in
 * gsim_last_error and nothing applied, on an unknown kind, an observer >= N,
 * a PROMISE whose peer is no connection (CSR neighbour) of the observer (the
 * other kinds ignore peer), or a time that goes backwards for an observer,
 * within the batch or against its last router event (this clock is separate
 * from the score tracer's), or a time above INT64_MAX - max(seen_ttl_ns,
 * followup_ns): an expiry is now + lifetime and must fit an int64 (any other
 * time, negative ones included, is accepted).  GSIM_ERANGE, nothing applied, when the live seen
 * entries plus the batch's SEEN_ADD events exceed seen_cap, or the live
 * promises plus its PROMISE events exceed promises_cap.  Presence in the seen
 * cache never depends on the clock: only gsim_router_state_sweep removes
 * entries.  GSIM_ESTATE before gsim_router_state_config.  Synchronizes. */
int gsim_router_state_events(gsim_handle* h, const gsim_router_event* ev, int64_t n, uint8_t* result);

/* The time cache's background sweep (timecache/util.go:26-35): drop every seen
 * entry with expiry < now_ns (strict: expiry == now_ns stays).  Their space
 * is reusable afterwards, and an id added again is new.  Synchronizes. */
int gsim_router_state_sweep(gsim_handle* h, int64_t now_ns);

/* ThrottlePeer (gossip_tracer.go:182-200) for n (observer, peer) pairs
 * (pairs[2q], pairs[2q + 1]): every promise of that peer at that observer is
 * dropped; *dropped (may be NULL) their number.  GSIM_EINVAL, nothing dropped,
 * with the first offending pair in gsim_last_error, on an observer >= N or a
 * peer that is no connection of it.  Runs between batches (the reference
 * calls it from the control path, asynchronously to message events).
 * Synchronizes. */
int gsim_router_state_throttle(gsim_handle* h, const uint32_t* pairs, int64_t n, int64_t* dropped);

/* GetBrokenPromises (gossip_tracer.go:79-115) of every observer: the promises
 * with expire < now_ns (strict) are removed and counted, one row per
 * (observer, peer), sorted by (observer, peer).  *n is always set; when cap
 * is too small: GSIM_ERANGE and nothing is removed.  apply_penalty != 0: each
 * row also does what a GSIM_EV_ADD_PENALTY event of (observer, peer, count)
 * does to GSIM_F_BP, the silent return for a peer without peerStats included.
 * Space: the pool entries and table records of fulfilled, throttled and
 * broken promises are free again at once as far as the capacity check of
 * gsim_router_state_events goes (it counts live promises; a batch that needs
 * the space compacts table and pool first), and physically after every
 * throttle and broken call, which rebuild both.  Synchronizes. */
int gsim_router_state_broken(gsim_handle* h, int64_t now_ns, int32_t apply_penalty, gsim_broken_row* out, int64_t cap,
                             int64_t* n);

/* out6 = {live seen entries, live promises, events applied, seen entries
 * swept, promises fulfilled + throttled, promises broken} since
 * gsim_router_state_config. */
int gsim_router_state_stats(gsim_handle* h, int64_t* out6);

/* Copy the score snapshot (E doubles, edge order) to host. */
int gsim_read_scores(gsim_handle* h, double* out);

/* WithPeerScoreInspect's ExtendedPeerScoreInspectFn (score.go:127-180),
 * filled as inspectScoresExtended does (score.go:472-500) for every
 * connection of the observers [obs_lo, obs_hi): peers[x] for the x-th edge of
 * those rows (edge order), topics[x * T + t] its topic t.  Score is the live
 * score(p) (deliveries since the last refresh included); a topic without
 * events reads as a zero record; an untracked edge (no peerStats) has
 * tracked = 0 and zeros. */
typedef struct gsim_topic_score_snapshot {
    int64_t time_in_mesh_ns;            /* meshTime while inMesh, else 0 */
    double  first_message_deliveries;
    double  mesh_message_deliveries;
    double  invalid_message_deliveries;
} gsim_topic_score_snapshot;
typedef struct gsim_peer_score_snapshot {
    double   score;
    double   app_specific_score;
    double   ip_colocation_factor;       /* the P6 value before its weight */
    double   behaviour_penalty;
    uint32_t observer, peer;             /* peer ids (global ids on a shard) */
    int32_t  tracked;
    int32_t  _pad;
} gsim_peer_score_snapshot;
int gsim_read_snapshot(gsim_handle* h, int64_t obs_lo, int64_t obs_hi, gsim_peer_score_snapshot* peers,
                       gsim_topic_score_snapshot* topics);

/* refreshIPs (score.go:568-585): replace every peer's IP list (CSR as for
 * gsim_load_graph); P6 is re-derived before the next score.  The whitelist
 * stays if n_ips is unchanged, else it is cleared.  GSIM_ESTATE once the peer
 * gater is on (its per-IP groups are fixed by gsim_set_peer_gater). */
int gsim_set_ips(gsim_handle* h, const uint32_t* ip_ptr, const uint32_t* ip_ids, uint32_t n_ips);

/* ---- raw state access (tests, checkpoint/resume, golden fixtures) ------- */
typedef enum gsim_field {
    GSIM_F_FIRST = 0,     /* f64 [T][E] firstMessageDeliveries          score.go:49 */
    GSIM_F_MESHD,         /* f64 [T][E] meshMessageDeliveries           score.go:52 */
    GSIM_F_FAIL,          /* f64 [T][E] meshFailurePenalty              score.go:58 */
    GSIM_F_INVALID,       /* f64 [T][E] invalidMessageDeliveries        score.go:61 */
    GSIM_F_GRAFT_TIME,    /* i64 [T][E] graftTime (ns)                  score.go:42 */
    GSIM_F_MESH_TIME,     /* i64 [T][E] meshTime (ns)                   score.go:46 */
    GSIM_F_TFLAGS,        /* u8  [T][E] bit0 inMesh, bit1 meshMessageDeliveriesActive, bit2 mesh, bit3 fanout */
    GSIM_F_BP,            /* f64 [E]    behaviourPenalty                score.go:34 */
    GSIM_F_ESTATE,        /* u8  [E]    bit0 tracked (peerStats exists), bit1 connected */
    GSIM_F_EXPIRE,        /* i64 [E]    retention expiry (ns)           score.go:22 */
    GSIM_F_P6,            /* f64 [E]    ipColocationFactor value        */
    GSIM_F_SCORE,         /* f64 [E]    score snapshot                  */
    GSIM_F_BACKOFF,       /* i64 [T][E] prune backoff expiry, 0 = none gossipsub.go:432 */
    GSIM_F_CTL,           /* u8 [2][T][E] control inbox by round parity (receiver's edge) */
    GSIM_F_SEEN,          /* u32 [ring][N] first-seen round, 0xFFFFFFFF unseen (after msgs_init) */
    GSIM_F_LASTPUT,       /* i32 [T][N] tick of the newest mcache.Put, -1 none (after msgs_init) */
    GSIM_F_LASTPUB,       /* i64 [N][T] gs.lastpub[topic] (ns), 0 = none  gossipsub.go:426 (peer-major) */
    GSIM_F_FANOUT_TOPICS, /* u64 [N]    bit t: gs.fanout[topic t] exists  gossipsub.go:425 */
    GSIM_F__COUNT
} gsim_field;

#define GSIM_TF_IN_MESH   0x01u  /* topicStats.inMesh (score.go:39)               */
#define GSIM_TF_ACTIVE    0x02u  /* topicStats.meshMessageDeliveriesActive         */
#define GSIM_TF_MESH      0x04u  /* router membership: gs.mesh[topic][p] (gossipsub.go:424) */
#define GSIM_TF_FANOUT    0x08u  /* router fanout: gs.fanout[topic][p] (gossipsub.go:425) */
/* control inbox bits (GSIM_F_CTL), one byte per [parity][topic][receiver edge] */
#define GSIM_CTL_GRAFT    0x01u  /* ControlGraft  (pb/rpc.proto) */
#define GSIM_CTL_PRUNE    0x02u  /* ControlPrune with Backoff = PruneBackoff/1s */
#define GSIM_CTL_PX       0x04u  /* the PRUNE carries peer exchange (makePrune doPX, gossipsub.go:1878-1903) */
#define GSIM_CTL_IHAVE    0x08u  /* ControlIHave for this topic */
#define GSIM_CTL_UNSUB    0x10u  /* the PRUNE is Leave's (makePrune isUnsubscribe, gossipsub.go:1104-1124):
                                    Backoff = UnsubscribeBackoff/1s */
#define GSIM_ES_TRACKED   0x01u
#define GSIM_ES_CONNECTED 0x02u

/* Size in bytes of a field for the loaded graph. */
int gsim_field_bytes(gsim_handle* h, int32_t field, size_t* out);
int gsim_read_field(gsim_handle* h, int32_t field, void* dst, size_t bytes);
int gsim_write_field(gsim_handle* h, int32_t field, const void* src, size_t bytes);

/* ---- device timing on the engine's own stream (bench/profiling) -------- */
/* Record HIP event `slot` (0..511) on the engine stream. */
int gsim_event_record(gsim_handle* h, int32_t slot);
/* Milliseconds between two recorded events (synchronizes on `to`). */
int gsim_event_elapsed(gsim_handle* h, int32_t from, int32_t to, float* ms);
int gsim_synchronize(gsim_handle* h);
/* Per-kernel-class device time, measured with HIP events recorded on the
 * engine stream around each class's launches while profiling is enabled. */
typedef enum gsim_kernel_class {
    GSIM_K_REFRESH_SCORE = 0,  /* refreshScores (+ fused score) pass */
    GSIM_K_SCORE,              /* score-only pass */
    GSIM_K_IP_COLOCATION,      /* P6 segmented count */
    GSIM_K_HEARTBEAT,          /* mesh maintenance */
    GSIM_K_CONTROL,            /* GRAFT/PRUNE handling */
    GSIM_K_PUBLISH,            /* slot reset + origin self-delivery */
    GSIM_K_SEND,               /* mesh forwarding: AcceptFrom, seen-set claims, duplicate/invalid counters */
    GSIM_K_COMMIT,             /* seen commit + first-delivery credit */
    GSIM_K_ACCEPT,             /* AcceptFrom verdicts from a new score snapshot */
    GSIM_K_GOSSIP,             /* handleIHave/handleIWant + IWANT response delivery */
    GSIM_K_CHURN,              /* AddPeer/RemovePeer of gsim_set_connections */
    GSIM_K_TRACER_SORT,        /* gsim_score_tracer_events: grouping the batch by observer */
    GSIM_K_TRACER_RESOLVE,     /* ... the events' edges and the batch checks */
    GSIM_K_TRACER_APPLY,       /* ... the per-observer walk over the events */
    GSIM_K_ROUTER_SORT,        /* gsim_router_state_events: grouping the batch by observer */
    GSIM_K_ROUTER_RESOLVE,     /* ... the PROMISE events' edges and the batch checks */
    GSIM_K_ROUTER_APPLY,       /* ... the per-observer walk over the events */
    GSIM_K_ROUTER_SWEEP,       /* gsim_router_state_sweep: the seen table's rebuild */
    GSIM_K_ROUTER_BROKEN,      /* gsim_router_state_broken / _throttle: the promise kernels, sort and rebuild (device
                                  work only); also the compaction a batch of gsim_router_state_events runs first */
    GSIM_K__COUNT
} gsim_kernel_class;
/* Enable (1) or disable (0) recording; clears recorded totals. */
int gsim_profile(gsim_handle* h, int32_t enable);
/* Synchronize, then write per-class milliseconds and launch counts recorded
 * since the last read (n entries, indexed by gsim_kernel_class) and reset. */
int gsim_profile_read(gsim_handle* h, double* ms, int64_t* launches, int32_t n);
/* Select an implementation variant of a hot-path kernel for A/B timing in
 * one process.  Results are identical across variants (the GPU tests run
 * each).  which = 2: the delivery kernel; 3 (topic-major k_send_tm) is the
 * only one.  which = 3: the IHAVE walk's lane
 * group width (8, 16, 32 or 64 lanes per row; 0 = chosen from the row lengths).
 * which = 6: the topic-major kernel's blocks: 0 (default) shared out among
 * the topics by their subscribers, 1 the same number for every topic, >= 64
 * shared out by subscribers, this many in all. */
int gsim_set_kernel_variant(gsim_handle* h, int32_t which, int32_t variant);

/* ---- synthetic inputs -------------------------------- */
/* Random k-regular simple graph on n vertices (configuration model, bad
 * pairs repaired by random double-edge swaps), seeded.  row_ptr (n+1) and
 * col_idx (n*k) are caller-allocated; rows come out sorted.  outbound
 * (n*k, may be NULL) gets a Bernoulli(0.5) initiator per undirected edge. */
int gsim_gen_random_regular(int64_t n, int32_t k, uint64_t seed,
                            uint32_t* row_ptr, uint32_t* col_idx, uint8_t* outbound);
/* Chung-Lu power law (C5 inputs): expected degree of peer i proportional to
 * (i + i0)^(-1/(exponent-1)) scaled to `mean`, capped at max_degree; pairs
 * drawn by inverse CDF, self loops and repeats dropped, then accepted in
 * drawing order while both ends are below the cap.  Call with col_idx NULL
 * for the directed edge count (*n_edges), then with row_ptr (n+1), col_idx
 * and outbound (may be NULL) sized to it; rows come out sorted. */
int gsim_gen_power_law(int64_t n, double mean, double exponent, int32_t max_degree, double i0, uint64_t seed,
                       uint32_t* row_ptr, uint32_t* col_idx, uint8_t* outbound, int64_t* n_edges);
/* Fill every edge-topic record with seeded steady-state-like counters on the
 * device (mesh membership with probability p_mesh, graft times within the
 * last hour of now_ns); every edge tracked+connected.  Records of topics the
 * two endpoints do not both announce stay empty.  For benchmarking at sizes
 * where a host upload would dominate. */
int gsim_fill_synthetic(gsim_handle* h, uint64_t seed, int64_t now_ns, double p_mesh);

/* ---- graph sharding across GPUs -------- */
/* The reference simulates nothing across processes: one GossipSubRouter per
 * host, RPCs over libp2p streams (gossipsub.go:1138-1202 sendRPC).  Here one
 * network is split into contiguous peer ranges, one per shard (GPU); a shard
 * holds its peers' rows in full plus a "ghost" row per remote neighbour (that
 * neighbour's connections into the shard), so every record an owned observer
 * keeps is local.  Copies are pulled: each round every shard sends the
 * others its forwarders of the round (peer, first sender, slot), and a shard
 * walks the ghost rows of the remote forwarders itself, so each copy is
 * delivered by the receiver's shard.  GRAFT/PRUNE records, the router state
 * of cross edges (mesh / fanout bits, connected, direct, publish gate) and
 * gossip marks move the same way.  At most 2^24 - 2 peers per network. */
#define GSIM_MAX_SHARDS 64

/* Contiguous peer ranges for `shards` shards balanced by the sum of (row
 * length x joined topics): bounds[0] = 0 < bounds[1] < ... < bounds[shards]
 * = n, interior bounds multiples of 64.  sub may be NULL (one topic each). */
int gsim_shard_partition(int64_t n, const uint32_t* row_ptr, const uint64_t* sub, int32_t shards,
                         int64_t* bounds);

typedef struct gsim_shard_info {
    int32_t shard, shards;
    int64_t n_local, e_local;   /* local peers (owned + ghosts) and edges (owned rows + ghost rows) */
    int64_t own_lo, own_hi;     /* owned peers: local ids [own_lo, own_hi) = global [bounds[s], bounds[s+1]) */
    int64_t own_e_lo, own_e_hi; /* local edges of the owned rows */
    int64_t n_cross;            /* owned-row edges whose column belongs to another shard */
} gsim_shard_info;
int gsim_shard_layout_info(int64_t n, const uint32_t* row_ptr, const uint32_t* col, const int64_t* bounds,
                           int32_t shards, int32_t shard, gsim_shard_info* out);
/* The local graph of one shard (sizes from gsim_shard_layout_info; any output
 * may be NULL): gid[n_local] global id of each local peer (ascending);
 * row_ptr_l/col_l the local CSR; gidx[e_local] the global index of each local
 * edge; per other shard s, ghost_base[s]/ghost_count[s] the local edges of the
 * ghost rows of s's peers, and cross_count[s] owned-row edges into s, listed
 * in edge order one shard after the other in cross_out (n_cross entries).
 * Two shards enumerate their common cross edges in the same order:
 * cross_out of a into b, position q, is the edge ghost_base[a] + q of b. */
int gsim_shard_layout(int64_t n, const uint32_t* row_ptr, const uint32_t* col, const int64_t* bounds,
                      int32_t shards, int32_t shard, uint32_t* gid, uint32_t* row_ptr_l, uint32_t* col_l,
                      uint64_t* gidx, int64_t* ghost_base, int64_t* ghost_count, uint32_t* cross_out,
                      int64_t* cross_count);

/* A sharded network: a group of shards, each an engine handle over its
 * local graph.  gsim_group_create puts every shard in this process (shard s
 * on devices[s]; devices NULL: all on device 0), exchanging with device
 * copies.  gsim_group_create_rccl is one shard of a multi-process job (one
 * process per GPU): `unique_id` comes from gsim_rccl_unique_id on rank 0,
 * shared by the caller (128 bytes), and the exchanges run over RCCL. */
typedef struct gsim_group gsim_group;
int gsim_rccl_unique_id(void* out, size_t bytes);
int gsim_group_create(const gsim_peer_score_params* params, const gsim_topic_score_params* topics, int32_t n_topics,
                      const gsim_thresholds* thresholds, const gsim_gossipsub_params* gossip, int32_t shards,
                      const int32_t* devices, gsim_group** out, char* err, size_t errlen);
int gsim_group_create_rccl(const gsim_peer_score_params* params, const gsim_topic_score_params* topics,
                           int32_t n_topics, const gsim_thresholds* thresholds, const gsim_gossipsub_params* gossip,
                           int32_t shards, int32_t rank, int32_t device, const void* unique_id, gsim_group** out,
                           char* err, size_t errlen);
/* One shard of a multi-process job whose exchanges go through the caller's
 * own collectives over host memory (device -> pinned host -> callback ->
 * device): the one-shard-per-process code path of gsim_group_create_rccl
 * without RCCL (tests on one GPU with gloo; hosts without xGMI).  Callbacks
 * return 0 on success and are called by every rank in the same order.
 *   alltoallv: send[sdisp[d] .. + sbytes[d]) to rank d; recv[rdisp[s] .. +
 *              rbytes[s]) from rank s (sizes agreed beforehand; the rank's own
 *              entries are 0);
 *   allreduce: elementwise over `count` values of every rank, in place;
 *              dtype 0 = u32, 1 = i32, 2 = u64; op 0 = sum, 1 = max. */
typedef struct gsim_host_transport {
    void* ctx;
    int (*alltoallv)(void* ctx, const uint8_t* send, const uint64_t* sbytes, const uint64_t* sdisp, uint8_t* recv,
                     const uint64_t* rbytes, const uint64_t* rdisp);
    int (*allreduce)(void* ctx, void* buf, int64_t count, int32_t dtype, int32_t op);
} gsim_host_transport;
int gsim_group_create_host(const gsim_peer_score_params* params, const gsim_topic_score_params* topics,
                           int32_t n_topics, const gsim_thresholds* thresholds, const gsim_gossipsub_params* gossip,
                           int32_t shards, int32_t rank, int32_t device, const gsim_host_transport* transport,
                           gsim_group** out, char* err, size_t errlen);
int gsim_group_destroy(gsim_group* g);
const char* gsim_group_last_error(const gsim_group* g);
/* The handle of a shard hosted by this process (NULL otherwise): its state is
 * read and written through the gsim_*_field calls in the local view (owned
 * rows are edges [own_e_lo, own_e_hi) of gsim_shard_layout_info). */
gsim_handle* gsim_group_shard(gsim_group* g, int32_t shard);
int gsim_group_bounds(const gsim_group* g, int64_t* bounds);
/* The whole network's CSR and inputs, as for gsim_load_graph (every process
 * passes the same); bounds NULL: gsim_shard_partition. */
int gsim_group_load_graph(gsim_group* g, int64_t n_peers, const uint32_t* row_ptr, const uint32_t* col_idx,
                          const uint8_t* outbound, const uint64_t* subscriptions, const uint32_t* ip_ptr,
                          const uint32_t* ip_ids, uint32_t n_ips, const int64_t* bounds);
/* The single-handle calls over the whole network (global peer / edge
 * indexing; the per-round halo exchange happens inside). */
int gsim_group_set_app_score(gsim_group* g, const double* p5);
int gsim_group_set_ip_whitelist(gsim_group* g, const uint8_t* whitelisted);
int gsim_group_set_direct_peers(gsim_group* g, const uint8_t* flags);
int gsim_group_set_peer_behaviour(gsim_group* g, const uint8_t* flags);
int gsim_group_set_topic_params(gsim_group* g, int32_t topic, const gsim_topic_score_params* p);
int gsim_group_set_seed(gsim_group* g, uint64_t seed);
int gsim_group_fill_synthetic(gsim_group* g, uint64_t seed, int64_t now_ns, double p_mesh);
/* max_frontier > 0: the initial size of the per-shard forwarder lists
 * (default max(8 x owned peers, 65536) entries; they grow when a round needs
 * more). */
int gsim_group_msgs_init(gsim_group* g, const gsim_msg_config* cfg);
int gsim_group_refresh_scores(gsim_group* g, int64_t now_ns);
int gsim_group_heartbeat(gsim_group* g, uint64_t tick, int64_t now_ns);
int gsim_group_publish(gsim_group* g, const gsim_msg* msgs, int32_t count, int64_t round);
int gsim_group_round(gsim_group* g, int64_t round);
int gsim_group_set_connections(gsim_group* g, const uint32_t* pairs, int32_t count, int32_t up, int64_t now_ns);
/* gsim_px_connect over the shards (every rank calls it between ticks): PX
 * lists PRUNEs carried to other shards' peers are checked there
 * (acceptPXThreshold on the pruned peer's score, a known address, not
 * connected), every attempt is resolved once (the asker dials, the lower id
 * when both asked) and connected at both ends; pairs: the (dialer, peer)
 * global ids, sorted.  The same connections as one engine's gsim_px_connect. */
int gsim_group_px_connect(gsim_group* g, int64_t now_ns, uint32_t* pairs, int64_t cap, int64_t* n_connected);
/* gsim_set_subscriptions over the shards (global peer ids; every rank passes
 * the same list): the same Joins / Leaves as one engine. */
int gsim_group_set_subscriptions(gsim_group* g, const uint32_t* pairs, int32_t count, int32_t join, uint64_t tick,
                                 int64_t now_ns);
int gsim_group_set_ips(gsim_group* g, const uint32_t* ip_ptr, const uint32_t* ip_ids, uint32_t n_ips);
/* Router state (mesh / fanout flags, connection state, direct flags) was
 * written through gsim_write_field on a shard handle: the ghost rows are
 * refreshed from their owners before the next round. */
int gsim_group_state_written(gsim_group* g);
/* Totals of the whole job (summed over every shard, every process). */
int gsim_group_msg_stats(gsim_group* g, int64_t* out4);
int gsim_group_gossip_stats(gsim_group* g, int64_t* out4);
int gsim_group_census(gsim_group* g, int64_t* out8);
/* gsim_msg_report over a sharded network: every local shard reports the
 * peers it owns and the rows are merged by slot (hist, reached, subscribers
 * summed; max_latency the maximum); origin is the global id.  GSIM_ESTATE if
 * the shards disagree about a slot's message.  With one shard per process
 * (RCCL / host transports) the rows hold the local shards' partial sums, as
 * gsim_group_read_field holds a rank's rows, and origin is 0xFFFFFFFF where
 * the publishing peer is neither owned by nor a neighbour of the rank's
 * shard. */
int gsim_group_msg_report(gsim_group* g, int64_t round_lo, int64_t round_hi,
                          struct gsim_msg_report* out, int64_t cap, int64_t* n);
/* gsim_set_peer_classes / gsim_net_report over a sharded network: classes by
 * global peer id (ghosts carry their owner's class); every local shard
 * reports the observers it owns and the rows are merged: counts summed,
 * max_degree the maximum, min / max of the scores.  With one shard per
 * process the rows hold the local shards' part, as gsim_group_msg_report's. */
int gsim_group_set_peer_classes(gsim_group* g, const uint8_t* cls);
int gsim_group_net_report(gsim_group* g, const double* edges, int32_t n_edges,
                          struct gsim_mesh_row* mesh, int64_t mesh_cap, int64_t* n_mesh,
                          struct gsim_score_row* scores, int64_t score_cap, int64_t* n_scores);
/* gsim_peer_report over a sharded network: every local shard reports the
 * peers it owns (a ghost's cell is never counted).  Peer ranges and per-peer
 * rows are in global ids; the class rows are summed on the host (lat_max the
 * maximum) and parts that disagree about a row's (topic, cls), its messages or
 * the selected count are refused with GSIM_ESTATE.  A first sender owned by
 * another shard is a ghost of the receiver's shard and carries its owner's
 * class there (gsim_group_set_peer_classes).  With one shard per process the
 * class rows hold the local shards' part and the per-peer rows of peers no
 * local shard owns stay as the caller left them, as gsim_group_msg_report's
 * rows and gsim_group_read_field's. */
int gsim_group_peer_report(gsim_group* g, int64_t round_lo, int64_t round_hi,
                           int64_t peer_lo, int64_t peer_hi, struct gsim_peer_row* peers,
                           struct gsim_peer_class_row* classes, int64_t class_cap,
                           int64_t* n_classes, int64_t* n_msgs);
/* gsim_relay_report over a sharded network: peer rows (global ids) and class
 * rows only.  Every shard walks the cells of the peers it owns; a parent may be
 * a ghost, so between the push and the fold of a batch the ghosts' child counts
 * are read and added into their owners' scratch through the host, and every
 * owner folds the total children(q, m) of its own peers.  A ghost parent's cell
 * is not checked for orphans.  Class rows are merged on the host (sums,
 * max_children the maximum; disagreeing keys, messages or selected counts:
 * GSIM_ESTATE).  Needs every shard in this process; a group whose shards span
 * processes: GSIM_ESTATE. */
int gsim_group_relay_report(gsim_group* g, int64_t round_lo, int64_t round_hi,
                            int64_t peer_lo, int64_t peer_hi, struct gsim_relay_row* peers,
                            struct gsim_relay_class_row* classes, int64_t class_cap,
                            int64_t* n_classes, int64_t* n_msgs);
/* gsim_score_report over a sharded network: every local shard reports the
 * records of the observers it owns (a ghost subject carries its class and its
 * app-specific score), with the same what-if parameters; the rows are merged
 * on the host: counts summed, min / max taken, parts that disagree about a
 * row's key refused with GSIM_ESTATE.  With one shard per process the rows
 * hold the local shards' part, as gsim_group_net_report's. */
int gsim_group_score_report(gsim_group* g, const struct gsim_score_what_if* what_if,
                            const double* edges, int32_t n_edges,
                            struct gsim_score_part_row*  parts,  int64_t part_cap,  int64_t* n_parts,
                            struct gsim_score_cause_row* causes, int64_t cause_cap, int64_t* n_causes,
                            struct gsim_score_topic_row* topics, int64_t topic_cap, int64_t* n_topics);
/* gsim_mesh_paths over a sharded network: sources and the per-peer arrays in
 * global ids.  Every shard expands the frontier of the peers it owns over its
 * own rows; the bits that land on its ghosts go to their owners between the
 * levels (through the host: the ghost ranges are read, the ids translated, the
 * words ORed in before the owner's fold), every shard counts the new bits of
 * its owned peers and the rows are summed on the host (max_hops the maximum,
 * truncated the OR).  Needs every shard in this process (gsim_group_create,
 * or the host-staged transport in one process); a group whose shards span
 * processes: GSIM_ESTATE. */
int gsim_group_mesh_paths(gsim_group* g, int32_t topic, const uint32_t* sources, int32_t n_sources,
                          uint32_t blocked, int32_t max_hops, struct gsim_mesh_path_row* rows,
                          uint32_t* reach_count, uint32_t* hop_sum);
int gsim_group_synchronize(gsim_group* g);
/* WithPeerScoreInspect over a sharded network (score.go:152-180, 448-500):
 * the whole network's view, filled from the rows this process's shards own
 * (every shard with gsim_group_create; one rank's range with the RCCL / host
 * transports, the rest of dst left as it was).
 * gsim_group_field_bytes: the size of a field for the whole network (N peers,
 *   E edges; gsim_field_bytes's shapes).
 * gsim_group_read_field: gsim_read_field in global peer / edge order.
 * gsim_group_read_scores: the score snapshot, E doubles in global edge order.
 * gsim_group_read_snapshot: gsim_read_snapshot for the global observers
 *   [obs_lo, obs_hi): peers[x] for the x-th edge of those rows (global edge
 *   order from row_ptr[obs_lo]), topics[x * T + t]; observer and peer are
 *   global ids. */
int gsim_group_field_bytes(gsim_group* g, int32_t field, size_t* out);
int gsim_group_read_field(gsim_group* g, int32_t field, void* dst, size_t bytes);
int gsim_group_read_scores(gsim_group* g, double* out);
int gsim_group_read_snapshot(gsim_group* g, int64_t obs_lo, int64_t obs_hi, gsim_peer_score_snapshot* peers,
                             gsim_topic_score_snapshot* topics);
/* WithPeerGater over a sharded network (peer_gater.go:161-186): every
 * shard's routers; gsim_group_gater_throttled sums the drops over the job,
 * gsim_group_gater_read is gsim_gater_read in global peer / edge order (the
 * parts this process's shards own). */
int gsim_group_set_peer_gater(gsim_group* g, const gsim_peer_gater_params* p, const double* topic_weights);
int gsim_group_gater_throttled(gsim_group* g, int64_t* out);
int gsim_group_gater_read(gsim_group* g, double* validate, double* throttle, int64_t* last, double* counters4,
                          int32_t* connected, int64_t* expire);
/* gsim_trace_config / gsim_trace_read over a sharded network: the routers
 * [peer_lo, peer_hi) (global ids) that this process's shards own, every
 * event in global ids, sorted as gsim_trace_read sorts.  Needs the copy push
 * exchange (the default). */
int gsim_group_trace_config(gsim_group* g, uint32_t peer_lo, uint32_t peer_hi, int64_t cap);
int gsim_group_trace_read(gsim_group* g, gsim_trace_event* out, int64_t cap, int64_t* n);
/* Per-kernel-class time of this process's shards (summed). */
int gsim_group_profile(gsim_group* g, int32_t enable);
int gsim_group_profile_read(gsim_group* g, double* ms, int64_t* launches, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* GSIM_H */
