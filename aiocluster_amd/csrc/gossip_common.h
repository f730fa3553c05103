// gossip_common.h -- what more than one unit of libgossip_sim.so needs (gossip_sim.hip, gossip_census.hip,
// gossip_select.hip, gossip_probe.hip), and nothing else.  Everything here has internal linkage (the anonymous
// namespace) or is inline: each unit gets its own copy.
//
// This header is OUTSIDE the benchmark's kernel hash: bench.py's kernel_source_hash() covers gossip_sim.hip and
// include/gossip_sim.h only.  A change to a helper below that a timed kernel uses (k_pass1v, k_pack_slice,
// k_pack_heavy, k_settle, k_lite, k_liveness) calls for a fresh PMC profile (profiles/pmc_summary.json), even
// though bench.py cannot see the change.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include <type_traits>

#include "../../include/gossip_sim.h"

namespace {

constexpr uint32_t NONE = GS_NONE;
constexpr int WAVE = 64;
constexpr int LB = 256;  // liveness / elementwise workgroups
// native vectors: the nontemporal load / store builtins take them (not HIP's uint4 struct)
typedef unsigned int v4u_t __attribute__((ext_vector_type(4)));
typedef unsigned int v2u_t __attribute__((ext_vector_type(2)));
constexpr double TICK_S = 1.0 / 64.0;

struct Dev {
    uint32_t N, NP, K, KP, C, mtu, flags, W;
    // owner-column slice: this handle holds columns [col_lo, col_lo + ncol) of every observer row
    // (NP = ncol rounded to 64 is the row stride); shards = 1: the whole matrix
    uint32_t col_lo, ncol, shards, shard;
    uint32_t max_iv, tomb_grace, dead_grace, sched_delay, lb_min, sum_bits;
    uint32_t ablate;  // profiling only (env GS_ABLATE): 1 = skip packing, 2 = skip pass-1 stores (results invalid);
                      // A/B, results valid: 8 = k_pass1v without its slow-group slots
    double phi_thr, prior5;
    double prior5t;  // prior5 in ticks (x 64): the liveness sweep's division-free phi test
    float phi_thr_f, prior5t_f;  // the same in binary32: the sweep's first, full-rate test (2^-20 margin)
    uint16_t *hb;       // heartbeat mod 2^16 (hb_dec: exact while a view lags its owner by < 2^16)
    uint32_t *self_hb;  // [NP] each owner column's own heartbeat, full width
    uint32_t *gc;
    uint16_t *mv;  // max_version | MV_INEXACT (u16: versions <= K * (C - 1) <= 16,256)
    uint8_t *held;
    uint32_t *fd;       // sampling window: _sum in ticks | intervals appended since the last reset << sum_bits
    uint16_t *fd_last;  // _last_heartbeat tick mod 2^16 (decoded against the operation's tick: fd_get)
    uint8_t *fd_state;  // bits 0-1: 0 unknown, 1 live, 2 dead (_live_nodes / _dead_nodes); FD_WIN, FD_OLD
    uint32_t *tod;      // time of death of a dead pair (read only for rows whose row word 2 has passed)
    uint32_t *ts;
    uint16_t *ring;
    uint32_t *pos, *ord, *row;
    uint8_t *last_w;
    uint64_t *hist;  // version | meta << 32
    uint32_t *lat;   // [NC][KP] each key's latest write: version | DeltaPb bytes of its kv << 16 (prefix views)
    uint32_t *hist_vid;
    uint16_t *nid_size;
    uint8_t *key_len;
    uint32_t *stamp;
    unsigned long long *ctr;
    uint32_t *sbits;  // sharded phases: stale-owner bitmaps of both directions per exchange [e][2][NP/32]
    uint2 *cand;       // split phases: stale-owner records [e][dir][half][GS_CAND_CAP] (GS_R_CAND)
    uint32_t *cand_n;  // [e][dir][half] stale owners found (GS_R_CAND_N)
    // heartbeat reports of the current round not yet applied to the windows: one bit plane per phase
    // p (tick t_round + 1 + p) and observer row, [N][NPL][PW] u64 in quad-interleaved column order
    // (plane_word/plane_bit); a plane row is valid only if pstamp[o][p] holds that phase's tick
    uint64_t *pend;
    uint32_t *pstamp;  // [N][NPL]
    uint32_t PW;       // u64 words per plane row: NP rounded up to 256, / 64
    // plane base: the tick of the last gs_begin_round, or, once a round has run phases more than NPL
    // ticks after it (the planes were replayed into the windows mid-round), the tick before the
    // first phase after that replay; plane p holds the phase at tick t_round + 1 + p
    uint32_t t_round;
    // sub-phases (round 6): several phases at one tick -- every exchange select_nodes_for_gossip chose, however
    // many phases its hubs need (server.py:476-493).  Plane p of the base holds the phase of VIRTUAL tick
    // v_round + 1 + p (pstamp holds virtual ticks, unique over the handle's life) at real tick
    // min(t_round + 1 + p, t_cap) (plane_tick); vt = the virtual tick of the phase being launched (set per phase by
    // the host).  Without sub-phases v_round = t_round, vt = the phase's tick and t_cap = NONE: the round-5 layout.
    uint32_t v_round, vt, t_cap;
    // speculative max-version merge (canonical record phases): pass 1 already wrote
    // max(sender, receiver) into the receiver's max_version word of every recorded candidate whose two
    // views are prefix views; the packers restore the receiver's word of such a candidate when it is not
    // sent, and skip the store when it is sent whole.  Set per phase by the host (gs_run_phase /
    // gs_phase_count), identical in every kernel of the phase.
    uint32_t spec;
    uint4 *slot_stat;  // sliced phases: per (exchange, direction) {NodeDeltas, kvs, candidates, needs a pack}
    // sampled rings (gs_config.ring_rows): ring slot of each observer row (NONE: a compact row), GS_R_RING
    // then holds [ring_rows][NP][W]; nullptr otherwise
    uint32_t *ring_slot;
    // prefix views: each owner's writes by version, [NC][VL] (GS_R_VLOG): DeltaPb bytes of the kv field |
    // version of the next write of the same key (0xFFFF: none) << 16 -- a prefix candidate's NodeDelta
    // size from the entries (mr, ms] alone (pack_lite)
    uint32_t *vlog;
    uint32_t VL;
    uint32_t lite;  // this phase runs k_lite before the exact packer (set per phase by the host)
    uint32_t hb8;   // GS_HB8: hb holds u8 views (mod 2^8), else u16 (mod 2^16)
    uint32_t mv8;   // GS_MV8: mv holds u8 views (version mod 2^7 | inexact << 7), else u16 words
    uint32_t *self_mv;  // [NP] each owner column's own max_version (GS_R_SELF_MV)
    // GS_MV8: [NP] both owner values packed for pass 1 (self_pack): one 16-byte load per 4 columns decodes
    // both 8-bit views -- the heartbeat needs only R mod 2^8 and whether R is 0 (R < 2^15 kept exactly),
    // the max_version word only M (< 2^15)
    uint32_t *self_pk;
    // GS_MV8 (pass 1 of the record phases, k_pass1v): per 16-owner group, bits 0-15 = "owner j's own heartbeat
    // is < 2^8" (an 8-bit view of it stored as 0 is then the heartbeat 0), bits 16-31 = "owner j is hot": at the
    // last lag sweep some view of j lagged by >= HOT_HB heartbeats or HOT_MV versions (GS_R_P1FLAGS)
    uint32_t *p1flags;
    uint32_t pl16;  // report planes in the 16-column layout of k_pass1v (plane16_bit), else the ballot layout
    // the launch after a k_pass1v phase (k_pack_slice / k_settle<1>, set per launch by the host) first sets the
    // phase's responders' small bits (k_p1v_fix's work, round 5: one launch fewer per phase)
    uint32_t p1fix;
    // escaped owner columns (gs_config.esc_cols, k_pass1v handles): EC slots of 16-bit views [N][EC]; esc_slot[j] =
    // the slot of column j or NONE; esc_owner[s] = the column of slot s or NONE; esc_req = the sweep's scratch
    // (columns to escape, bitmap [NP/32], then the move count and list)
    uint16_t *esc16;
    uint32_t *esc_slot, *esc_owner, *esc_req;
    uint32_t EC;
    // event stream (gs_set_events): records {observer, owner, key | kind << 8, old version, new version,
    // tick, seq, phase}; kind 0 = on_key_change, 1 = node join, 2 = node leave; seq orders them, phase = ev_phase
    // in apply_delta's records and 0 in every other (gossip_sim.h, gs_set_events).  ev == nullptr: off
    uint32_t *ev, *ev_count;
    uint32_t ev_cap;
    uint32_t ev_phase;  // phases started on this handle since gs_set_events, this one included (1 = the first)
    // the exact packer's heavy slots (round 6): k_pack_slice lists a slot with more than heavy_t stale owners here
    // ([0] = count, then slot ids) instead of walking it, and k_pack_heavy packs it with a workgroup of its own;
    // nullptr: no hand-off (set per launch by the host, one-slice record phases only)
    uint32_t *heavy;
    uint32_t heavy_t;
    // one-slice prefix-view handles (round 6): sm[c] = the smallest possible NodeDelta of any owner column >= c --
    // min over j >= c of msgf(msgf(NodeIdPb bytes of j) + 2 + the smallest kv field j ever wrote, GS_R_VLOG entry
    // 0), a lower bound of every candidate's min1 -- rebuilt after every gs_owner_writes (k_sm_local, k_sm_fix); sm[ncol] =
    // 0xFFFF.  First-fit continuation stops as soon as the budget left is below sm at the next candidate's column:
    // no later candidate can add a NodeDelta (R only shrinks).  nullptr: not built (sliced handles: the chain's
    // later slices hold the other columns)
    uint16_t *sm;
    uint32_t ev_wseq;  // owner-write ops issued since gs_set_events (the seq of the next call's op 0)
    // cut exchanges (gs_run_phase_cut): legs[e] = messages delivered of exchange e; read by the CUT instantiations
    // of the phase kernels only, which the host launches when it is set (set per phase; nullptr otherwise)
    const uint8_t *legs;
};

__device__ inline size_t pix(const Dev &d, uint32_t o, uint32_t j) { return (size_t)o * d.NP + j; }

// FD_STATE byte: membership in bits 0-1 (FD_MEMB), FD_WIN = the pair has a sampling window (its
// _last_heartbeat is set), FD_OLD = that last report is >= FD_OLD_AGE ticks old (k_fd_age)
enum FdSt { FD_UNKNOWN = 0, FD_LIVE = 1, FD_DEAD = 2, FD_MEMB = 3, FD_WIN = 4, FD_OLD = 8 };
constexpr uint32_t FD_OLD_AGE = 1u << 15;

// One sampling window (SamplingWindow + BoundedArrayStats, failure_detector.py:12-53, 131-162) per pair
// in 6 bytes + 2 state bits: the _last_heartbeat tick mod 2^16 (GS_R_FD_LAST) and one word (GS_R_FD) =
// _sum in ticks (sum_bits wide, exact: every interval is a whole number of 1/64 s) | intervals appended
// since the last reset << sum_bits.  Decoding the tick against the operation's tick t is exact while the
// report is < 2^16 ticks old; k_fd_age marks windows FD_OLD once it is 2^15 old (the host runs it at
// least every 2^14 ticks), and an FD_OLD window's tick only ever enters as "more than max_interval
// ago" (no interval appended, gs_create: max_interval < 2^14) and "phi above the threshold" (gs_create:
// threshold x max(max_interval, prior) < 2^15), so it is decoded as t - 2^15.
struct Fd {
    uint32_t last, sum, cnt;  // last = NONE when there is no window
};
__device__ inline Fd fd_get(const Dev &d, uint32_t st, uint32_t l16, uint32_t sc, uint32_t t) {
    const uint32_t last = !(st & FD_WIN) ? NONE : (st & FD_OLD) ? t - FD_OLD_AGE : t - ((t - l16) & 0xFFFFu);
    return Fd{last, sc & ((1u << d.sum_bits) - 1u), sc >> d.sum_bits};
}

__device__ inline int lane_id() { return (int)__lane_id(); }

__device__ inline bool bit(const uint32_t *bm, uint32_t j) { return (bm[j >> 5] >> (j & 31u)) & 1u; }

__device__ inline uint32_t wave_incl_scan(uint32_t x) {
    const int l = lane_id();
#pragma unroll
    for (int dd = 1; dd < WAVE; dd <<= 1) {
        const uint32_t y = __shfl_up(x, dd, WAVE);
        if (l >= dd) x += y;
    }
    return x;
}

__device__ inline unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) x += __shfl_xor(x, dd, WAVE);
    return x;
}

// a max_version word less its MV_INEXACT bit (prefix views: gossip_sim.hip)
constexpr uint32_t MV_MASK = GS_MV_INEXACT - 1u;

// GS_MV8: a view's max_version in one byte, version mod 2^7 | MV_INEXACT >> 8, decoded against the owner's
// own max_version M (every view is <= M; exact while it lags M by < 2^7: k_hb_lag) into the u16 word form
// (version | MV_INEXACT) every consumer uses.  mv_word / mv_put: one view, either width.
__device__ __forceinline__ uint32_t mv_dec8(uint32_t s, uint32_t M) {
    return (M - ((M - (s & 0x7Fu)) & 0x7Fu)) | ((s & 0x80u) << 8);
}

__device__ __forceinline__ void ld4(const uint32_t *p, uint32_t (&v)[4]) {
    const uint4 x = *reinterpret_cast<const uint4 *>(p);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
}

constexpr uint32_t B7 = 0x80808080u, L7 = 0x7F7F7F7Fu;
// per-byte (x - y) mod 2^8
__device__ __forceinline__ uint32_t bsub(uint32_t x, uint32_t y) { return ((x | B7) - (y & L7)) ^ (~(x ^ y) & B7); }
// wave-wide inclusive prefix sum (DPP: row shifts, then the row broadcasts)
__device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return x;
}

struct GroupArgs;  // gs_run_phase_group's batched launches (gossip_sim.hip)

}  // namespace

struct gs_handle {
    gs_config cfg;
    Dev d;
    uint32_t N, NP, K, KP, C, W;
    uint32_t G, shard, col_lo, ncol;  // owner-column slice
    bool sliced;                      // phases take the sliced path (G > 1, or GS_SLICED with one slice)
    bool reports_pending;             // phases ran since the last gs_liveness
    bool round_open;                  // gs_begin_round ran and gs_liveness has not closed the round yet
    uint32_t last_phase_tick;
    // sub-phases (Dev::v_round): the last phase's virtual tick (monotonic over the handle's life); a phase has run
    // at last_phase_tick since the last round start / flush (a further phase at that tick is then a sub-phase);
    // the plane base still needs its virtual base (set by the base's first phase)
    uint32_t last_vt = 0;
    bool sub_ok = false;
    bool base_fresh = true;
    uint64_t plane_flushes;           // mid-round report replays (rounds with phases > 16 ticks after the base)
    uint64_t lag_sweeps = 0;          // k_hb_lag sweeps run (gs_counters.lag_sweeps)
    uint32_t hb_incs;                 // rounds + phases since the last heartbeat-lag check (gs_check_heartbeat_lag)
    uint32_t mv_incs = 0;             // GS_MV8: gs_owner_writes calls since the last lag check
    uint32_t age_tick = 0;            // tick of the last window-age sweep (k_fd_age)
    uint32_t max_tick = 0;            // latest tick of any operation (gs_latest_tick: decodes GS_R_FD_LAST)
    void *reg[GS_NUM_REGIONS];
    uint64_t bytes[GS_NUM_REGIONS];
    hipStream_t stream;
    uint32_t seq;
    bool booted;
    bool started = false;             // a round has begun (gs_set_ring_rows refuses from then on)
    // canonical unsliced handles run a phase on candidate records (k_pass1 + k_settle); env GS_FUSED=1
    // selects the single fused k_exchange (and, on sliced handles, the fused count pass) for A/B runs
    bool split;
    // record phases (env GS_PACK, A/B runs): 0 = k_pass1 with the speculative merge + k_settle (default),
    // 1 = "fused": k_pass1 packing in the same workgroup, 2 = "split": k_pass1 + k_pack_slice
    int pack_mode = 2;
    bool age_init = false;            // age_tick holds the first operation's tick (fd_age)
    // gs_set_timing: HIP events around each kernel launch of a kind (gs_ktimes), on the library's stream
    bool timing;
    uint32_t *heavy_buf = nullptr;  // k_pack_heavy's slot list (Dev::heavy): [0] = count, then up to N slot ids
    uint16_t *sm_buf = nullptr;     // Dev::sm (one-slice prefix-view handles)
    unsigned long long *vc_buf = nullptr;  // gs_view_census scratch: VC_NUM u64 accumulators, then the probes
    std::vector<uint64_t> vc_img;          // ... and its host image (the upload before, the read after the pass)
    unsigned long long *dc_buf = nullptr;  // gs_detect_census scratch: DC_NUM u64 accumulators
    unsigned long long *ac_buf = nullptr;  // gs_age_census scratch: AC_NUM u64 accumulators, then the floor u32 [ncol]
    unsigned long long *tc_buf = nullptr;  // gs_traffic_census scratch: NSHARD rows of TC_NUM u64 accumulators
    hipStream_t hside = nullptr;    // k_pack_heavy's stream (forked after the lite slot work, joined after the packer)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev[GS_KT_KINDS];
    std::vector<hipEvent_t> evpool;
    std::string err;
    // sliced phases driven by the library (gs_comm_init: RCCL across processes; gs_run_phase_group:
    // the slices of one process): device scratch for the gathered totals and chain states
    ncclComm_t comm = nullptr;
    struct {
        uint64_t *tot = nullptr, *tot_all = nullptr, *chain = nullptr, *chainc = nullptr, *chain_all = nullptr;
        uint64_t *pend = nullptr;  // device: the pending slots summed over the slices (sliced_phase's one read per step)
        uint64_t *pin = nullptr, *pin_dev = nullptr;  // pinned host pair {pending, count} the kernel writes directly
        uint32_t *list = nullptr;
        uint32_t cap = 0;  // exchanges the buffers hold
    } sc;
    // gs_run_phase_group: each slice's kernels of a step run on a stream of its own (forked from and joined
    // back into the group's stream around the step), so the slices' short launches overlap on the GPU
    hipStream_t side = nullptr, home = nullptr;
    hipEvent_t fj_fork = nullptr, fj_join = nullptr;
    // gs_run_phase_group's batched launches: the group's GroupArgs in device memory and its host image as last
    // uploaded (held by the group's first handle)
    GroupArgs *grp = nullptr;
    std::vector<uint8_t> grp_img;
};

namespace {

int fail(gs_handle *h, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf;
    return code;
}

#define HIPCHK(h, x)                                                                         \
    do {                                                                                     \
        hipError_t _e = (x);                                                                 \
        if (_e != hipSuccess) return fail((h), GS_E_HIP, "%s: %s", #x, hipGetErrorString(_e)); \
    } while (0)

uint32_t round_up(uint32_t x, uint32_t m) { return (x + m - 1) / m * m; }

}  // namespace
