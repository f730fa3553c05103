// gossip_select.hip -- peer selection, phase scheduling and cut drawing of libgossip_sim.so: gs_select_peers,
// gs_schedule_phases, gs_draw_cuts, gs_draw_cuts_zoned, gs_filter_targets_zoned.

#include "gossip_common.h"

namespace {

// ------------------------------------------------------------------ peer selection
// select_nodes_for_gossip (server.py:656-717) for every up node from its failure detector's
// live / dead sets and its known peers, as _gossip_multiple uses them at round start
// (server.py:442-469): F distinct peers sampled uniformly from the live set (from all known
// peers while the live set is empty), one dead node with probability dead / (live + 1), and one
// seed when no selected peer is a seed or live < seeds, with probability seeds / (live + dead)
// (1 if both are empty; always when live = 0).  Random numbers: Philox4x32-10 keyed by the run
// seed, counter (round, node, slot) -- reproducible, where the reference's Random() over set
// iteration order is not.  Slots 0..F-1 feed Floyd's sample, SEL_DEAD and SEL_SEED
// the two probes.  Restated on the CPU by oracle/peer_select.py.
constexpr uint32_t SEL_DEAD = 14, SEL_SEED = 15;

__host__ __device__ inline void philox4x32(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; i++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
__host__ __device__ inline void sel_rand(uint64_t seed, uint32_t round, uint32_t node, uint32_t slot, uint32_t (&c)[4]) {
    c[0] = round; c[1] = node; c[2] = slot; c[3] = 0u;
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__host__ __device__ inline uint32_t below(uint32_t x, uint32_t n) { return (uint32_t)(((uint64_t)x * n) >> 32); }
__host__ __device__ inline double unit53(uint32_t a, uint32_t b) {
    return (double)(((uint64_t)a << 21) ^ (uint64_t)(b >> 11)) * (1.0 / 9007199254740992.0);
}

// gs_draw_cuts: independent message loss, one thread per exchange.  Message m of the exchange is lost iff word m
// of Philox(key = seed, counter = (round, initiator, responder, phase)) is below loss_q32; legs = the messages
// delivered before the first lost one.  Restated on the CPU by aiocluster_amd/cuts.py.
__global__ __launch_bounds__(LB) void k_draw_cuts(const int32_t *ini, const int32_t *res, uint32_t n, uint64_t seed,
                                                  uint32_t round, uint32_t phase, uint32_t loss_q32, uint8_t *legs) {
    const uint32_t e = blockIdx.x * LB + threadIdx.x;
    if (e >= n) return;
    uint32_t c[4] = {round, (uint32_t)ini[e], (uint32_t)res[e], phase};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    legs[e] = c[0] < loss_q32 ? 0u : c[1] < loss_q32 ? 1u : c[2] < loss_q32 ? 2u : 3u;
}

// Zoned links (gs_draw_cuts_zoned, gs_filter_targets_zoned): link[x * Z + y] = the loss threshold of a message from a
// node of zone x to a node of zone y, GS_LINK_DOWN = the link carries nothing.  The matrix travels as a kernel
// argument (1 KiB) and is staged in LDS, where every lane looks up its own two entries.
struct ZoneLinks {
    uint32_t q[GS_MAX_ZONES * GS_MAX_ZONES];
};
static_assert(LB >= (int)(GS_MAX_ZONES * GS_MAX_ZONES), "one thread per link entry stages the matrix");
// the two thresholds of the pair a -> b (forward: Syn and Ack, backward: SynAck); false = the connect fails: an index
// or a zone byte out of range, or either direction down (asyncio.wait_for(open_coro), server.py:403-405, 424-431)
__device__ __forceinline__ bool zone_pair(const uint32_t *s_link, const uint8_t *zone, uint32_t N, uint32_t Z,
                                          uint32_t a, uint32_t b, uint32_t &fwd, uint32_t &bwd) {
    if (a >= N || b >= N) return false;
    const uint32_t za = zone[a], zb = zone[b];
    if (za >= Z || zb >= Z) return false;
    fwd = s_link[za * Z + zb];
    bwd = s_link[zb * Z + za];
    return fwd != GS_LINK_DOWN && bwd != GS_LINK_DOWN;
}
// gs_draw_cuts_zoned: k_draw_cuts with the threshold of each message's direction; a pair whose connect fails gets
// GS_LEGS_NO_CONNECT.  Restated on the CPU by aiocluster_amd/cuts.py (draw_cuts_zoned).
__global__ __launch_bounds__(LB) void k_draw_cuts_zoned(const int32_t *ini, const int32_t *res, uint32_t n, uint32_t N,
                                                        uint64_t seed, uint32_t round, uint32_t phase,
                                                        const uint8_t *zone, ZoneLinks lk, uint32_t Z, uint8_t *legs) {
    __shared__ uint32_t s_link[GS_MAX_ZONES * GS_MAX_ZONES];
    if (threadIdx.x < Z * Z) s_link[threadIdx.x] = lk.q[threadIdx.x];
    __syncthreads();
    const uint32_t e = blockIdx.x * LB + threadIdx.x;
    if (e >= n) return;
    const uint32_t a = (uint32_t)ini[e], b = (uint32_t)res[e];
    uint32_t fwd = 0u, bwd = 0u;
    if (!zone_pair(s_link, zone, N, Z, a, b, fwd, bwd)) {
        legs[e] = (uint8_t)GS_LEGS_NO_CONNECT;
        return;
    }
    uint32_t c[4] = {round, a, b, phase};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    legs[e] = c[0] < fwd ? 0u : c[1] < bwd ? 1u : c[2] < fwd ? 2u : 3u;
}
// gs_filter_targets_zoned: the selected targets (gs_select_peers: out[o * per + slot], -1 = none) whose connect
// would fail become -1; in may alias out (a thread reads and writes its own entry only).
__global__ __launch_bounds__(LB) void k_zone_filter(const int32_t *in, int32_t *out, uint32_t n_targets, uint32_t per,
                                                    uint32_t N, const uint8_t *zone, ZoneLinks lk, uint32_t Z,
                                                    uint32_t *dropped) {
    __shared__ uint32_t s_link[GS_MAX_ZONES * GS_MAX_ZONES];
    if (threadIdx.x < Z * Z) s_link[threadIdx.x] = lk.q[threadIdx.x];
    __syncthreads();
    const uint32_t e = blockIdx.x * LB + threadIdx.x;
    bool drop = false;
    if (e < n_targets) {
        const int32_t t = in[e];
        uint32_t fwd, bwd;
        drop = t >= 0 && !zone_pair(s_link, zone, N, Z, e / per, (uint32_t)t, fwd, bwd);
        out[e] = drop ? -1 : t;
    }
    const unsigned long long m = __ballot(drop);
    if (dropped && (threadIdx.x & 63) == 0 && m) atomicAdd(dropped, (uint32_t)__popcll(m));
}

// per row: live / dead / known-peer counts (observer up); SCNT[o] = {live, dead, peers, 0}
__global__ __launch_bounds__(LB) void k_sel_count(Dev d, const uint8_t *up, uint32_t *scnt) {
    const uint32_t o = blockIdx.x;
    if (!up[o]) return;
    const bool genm = !(d.flags & GS_CANONICAL);
    uint32_t L = 0, D = 0, P = 0;
    for (uint32_t j = threadIdx.x; j < d.ncol; j += LB) {
        const size_t p = pix(d, o, j);
        if (j == o || (genm && d.pos[p] == NONE)) continue;
        const uint32_t st = d.fd_state[p] & FD_MEMB;
        P++;
        L += st == 1u;
        D += st >= 2u;
    }
    __shared__ uint32_t s3[3][LB / WAVE];
    const uint32_t w = threadIdx.x >> 6;
    const unsigned long long l = wave_sum(L), dd = wave_sum(D), pp = wave_sum(P);
    if ((threadIdx.x & 63) == 0) { s3[0][w] = (uint32_t)l; s3[1][w] = (uint32_t)dd; s3[2][w] = (uint32_t)pp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0, c = 0;
        for (int i = 0; i < LB / WAVE; i++) { a += s3[0][i]; b += s3[1][i]; c += s3[2][i]; }
        scnt[o * 4 + 0] = a; scnt[o * 4 + 1] = b; scnt[o * 4 + 2] = c;
    }
}

// The seed probe (server.py:700-717) of row o and the resolved picks out: thread 0 of the resolve kernels.
__device__ void sel_seed_probe(const Dev &d, uint32_t o, uint32_t L, uint32_t D, uint32_t F, uint64_t seed,
                               uint32_t round, const int32_t *seeds, uint32_t n_seeds, const uint32_t *s_hit,
                               int32_t *oo, const uint32_t *pre = nullptr) {
    bool has_seed = false;
    uint32_t S = 0;
    for (uint32_t q = 0; q < n_seeds; q++) {
        if ((uint32_t)seeds[q] == o) continue;
        S++;
        for (uint32_t i = 0; i < F; i++) has_seed |= s_hit[i] == (uint32_t)seeds[q];
    }
    uint32_t pick = NONE;
    if (S && (!has_seed || L < S)) {
        uint32_t c[4];
        if (pre) {  // (drawn earlier by another lane: the same counter, the same values)
            for (int q = 0; q < 4; q++) c[q] = pre[q];
        } else {
            sel_rand(seed, round, o, SEL_SEED, c);
        }
        const double ps = (L + D) == 0u ? 1.0 : (double)S / (double)(L + D);
        if (L == 0u || unit53(c[0], c[1]) <= ps) {
            uint32_t k = below(c[2], S);
            for (uint32_t q = 0; q < n_seeds; q++) {
                if ((uint32_t)seeds[q] == o) continue;
                if (k-- == 0) { pick = (uint32_t)seeds[q]; break; }
            }
        }
    }
    for (uint32_t i = 0; i < F + 1; i++) oo[i] = s_hit[i] == NONE ? -1 : (int32_t)(d.col_lo + s_hit[i]);
    oo[F + 1] = pick == NONE ? -1 : (int32_t)pick;
}

// Canonical layout (every observer knows every owner, no dict positions): the same counts from 16 state
// bytes per thread and load -- live = membership 1, dead = membership 2 (bit 1), known = every column but
// the observer's own (whose state stays unknown: liveness skips it).
__device__ __forceinline__ uint32_t memb_live4(uint32_t w) {  // bytes whose membership bits are 01
    const uint32_t m = w & 0x03030303u;
    return m & ~(m >> 1) & 0x01010101u;
}
__device__ __forceinline__ uint32_t memb_dead4(uint32_t w) { return (w >> 1) & 0x01010101u; }
__global__ __launch_bounds__(LB) void k_sel_count16(Dev d, const uint8_t *up, uint32_t *scnt) {
    const uint32_t o = blockIdx.x;
    if (!up[o]) return;
    uint32_t L = 0, D = 0;
    const uint8_t *row = d.fd_state + (size_t)o * d.NP;
    for (uint32_t j0 = threadIdx.x * 16u; j0 < d.ncol; j0 += LB * 16u) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + j0);  // NP is a multiple of 64: in the row
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t jq = j0 + 4u * q;
            uint32_t keep = 0x01010101u;  // columns < ncol (the padding's state bytes are never written: 0)
            if (jq + 4u > d.ncol) keep = jq >= d.ncol ? 0u : (0x01010101u >> (8u * (jq + 4u - d.ncol)));
            const uint32_t js = o - d.col_lo - jq;  // the observer's own column is not a peer
            if (js < 4u) keep &= ~(0x01u << (8u * js));
            L += (uint32_t)__popc(memb_live4(w[q]) & keep);
            D += (uint32_t)__popc(memb_dead4(w[q]) & keep);
        }
    }
    __shared__ uint32_t s2[2][LB / WAVE];
    const uint32_t wv = threadIdx.x >> 6;
    const unsigned long long l = wave_sum(L), dd = wave_sum(D);
    if ((threadIdx.x & 63) == 0) { s2[0][wv] = (uint32_t)l; s2[1][wv] = (uint32_t)dd; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
        for (int i = 0; i < LB / WAVE; i++) { a += s2[0][i]; b += s2[1][i]; }
        scnt[o * 4 + 0] = a;
        scnt[o * 4 + 1] = b;
        scnt[o * 4 + 2] = d.ncol - (o - d.col_lo < d.ncol ? 1u : 0u);  // known: every column but o's own
    }
}

// Floyd's sample of k distinct ranks of [0, n) (n = L live, or P known when none is live) and the dead probe,
// by rank, into so[0..F] (NONE where absent: so[] starts all NONE)
// pre (optional): the draws of counters (round, o, slot) already made, pre[4 i + q] for slot i < F, then SEL_DEAD
__device__ inline void sel_ranks(uint32_t o, uint32_t L, uint32_t D, uint32_t P, uint32_t F, uint64_t seed,
                                 uint32_t round, uint32_t *so, const uint32_t *pre = nullptr) {
    const uint32_t n = L ? L : P, k = F < n ? F : n;
    uint32_t c[4];
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t t = n - k + i;
        if (pre) c[0] = pre[4 * i];
        else sel_rand(seed, round, o, i, c);
        uint32_t r = below(c[0], t + 1);
        for (uint32_t q = 0; q < i; q++)
            if (so[q] == r) { r = t; break; }
        so[i] = r;
    }
    if (D) {
        if (pre) {
            for (int q = 0; q < 4; q++) c[q] = pre[4 * F + q];
        } else {
            sel_rand(seed, round, o, SEL_DEAD, c);
        }
        const double pd = (double)D / (double)(L + 1u);
        if (pd > unit53(c[0], c[1])) so[F] = below(c[2], D);
    }
}
// Floyd's sample of k distinct ranks of [0, n) and the dead probe, by rank; targets resolved next.
// sel[o][0..F) = live (or peer) ranks, sel[o][F] = dead rank, NONE where absent.
__global__ __launch_bounds__(LB) void k_sel_pick(Dev d, const uint8_t *up, const uint32_t *scnt, uint32_t F,
                                                 uint64_t seed, uint32_t round, uint32_t *sel) {
    const uint32_t o = blockIdx.x * LB + threadIdx.x;
    if (o >= d.N) return;
    uint32_t *so = sel + (size_t)o * (F + 2);
    for (uint32_t i = 0; i < F + 2; i++) so[i] = NONE;
    if (!up[o]) return;
    sel_ranks(o, scnt[o * 4 + 0], scnt[o * 4 + 1], scnt[o * 4 + 2], F, seed, round, so);
}

// k-th set bit (k < popc(m)) of a 16-bit mask
__device__ __forceinline__ uint32_t nth_bit16(uint32_t m, uint32_t k) {
    for (uint32_t i = 0; i < k; i++) m &= m - 1u;
    return (uint32_t)__builtin_ctz(m);
}
// Canonical layout: k_sel_resolve with 16 columns per thread and step (one 16-byte state load); the pool
// (live, or every known node when none is live) and dead masks are ranked by a block scan of their
// popcounts, so a row takes ncol / 4096 steps instead of ncol / 256.
__global__ __launch_bounds__(LB) void k_sel_resolve16(Dev d, const uint8_t *up, const uint32_t *scnt, uint32_t F,
                                                      uint64_t seed, uint32_t round, const int32_t *seeds,
                                                      uint32_t n_seeds, const uint32_t *sel, int32_t *out) {
    __shared__ uint32_t s_w[LB / WAVE][2];
    __shared__ uint32_t s_rank[10], s_hit[10];
    const uint32_t o = blockIdx.x;
    int32_t *oo = out + (size_t)o * (F + 2);
    if (!up[o]) {
        for (uint32_t i = threadIdx.x; i < F + 2; i += LB) oo[i] = -1;
        return;
    }
    const uint32_t L = scnt[o * 4 + 0];
    const bool from_live = L != 0;
    if (threadIdx.x < F + 1) {
        s_rank[threadIdx.x] = sel[(size_t)o * (F + 2) + threadIdx.x];
        s_hit[threadIdx.x] = NONE;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint8_t *row = d.fd_state + (size_t)o * d.NP;
    uint32_t base_pool = 0, base_dead = 0;
    for (uint32_t b0 = 0; b0 < d.ncol; b0 += LB * 16u) {
        const uint32_t j0 = b0 + threadIdx.x * 16u;
        uint32_t mp = 0, md = 0;  // bit i: column j0 + i is in the pool / dead
        if (j0 < d.ncol) {
            const uint4 v = *reinterpret_cast<const uint4 *>(row + j0);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const uint32_t j = j0 + 4u * q + b;
                    const uint32_t st = (wd[q] >> (8 * b)) & FD_MEMB;
                    const bool valid = j < d.ncol && d.col_lo + j != o;
                    const bool live = valid && st == 1u, dead = valid && st >= 2u;
                    mp |= (uint32_t)(from_live ? live : valid) << (4 * q + b);
                    md |= (uint32_t)dead << (4 * q + b);
                }
            }
        }
        const uint32_t cp = (uint32_t)__popc(mp), cd = (uint32_t)__popc(md);
        const uint32_t ip = wave_incl_scan(cp), id = wave_incl_scan(cd);
        if (lane == 63) { s_w[w][0] = ip; s_w[w][1] = id; }
        __syncthreads();
        uint32_t op = base_pool + ip - cp, od = base_dead + id - cd, tp = 0, td = 0;
        for (uint32_t i = 0; i < LB / WAVE; i++) {
            if (i < w) { op += s_w[i][0]; od += s_w[i][1]; }
            tp += s_w[i][0];
            td += s_w[i][1];
        }
        for (uint32_t i = 0; i < F; i++) {
            const uint32_t r = s_rank[i];
            if (r != NONE && r >= op && r < op + cp) s_hit[i] = j0 + nth_bit16(mp, r - op);
        }
        {
            const uint32_t r = s_rank[F];
            if (r != NONE && r >= od && r < od + cd) s_hit[F] = j0 + nth_bit16(md, r - od);
        }
        base_pool += tp;
        base_dead += td;
        __syncthreads();
    }
    if (threadIdx.x == 0) sel_seed_probe(d, o, L, scnt[o * 4 + 1], F, seed, round, seeds, n_seeds, s_hit, oo);
}

// Canonical layout, ncol <= SEL_ROW_IT * 4096: k_sel_count16 + k_sel_pick + k_sel_resolve16 in one workgroup per
// row that reads the row's state bytes once -- each thread keeps its 16-column live / dead masks of every
// 4,096-column step in registers: the counts, the ranks (thread 0), then one block scan of all steps at once
// (one barrier instead of two per step)
constexpr uint32_t SEL_ROW_IT = 16;
__global__ __launch_bounds__(LB, 4) void k_sel_row16(Dev d, const uint8_t *up, uint32_t F, uint64_t seed, uint32_t round,
                                                  const int32_t *seeds, uint32_t n_seeds, uint32_t *scnt, int32_t *out) {
    // the live / dead masks of every step in LDS (16 KB: registers would hold the occupancy to 2 waves per SIMD)
    __shared__ uint16_t s_m[SEL_ROW_IT][2][LB];
    __shared__ uint32_t s_w[SEL_ROW_IT][LB / WAVE][2];
    __shared__ uint32_t s_rank[10], s_hit[10], s_cnt[2], s_rnd[10 * 4];
    const uint32_t o = blockIdx.x;
    int32_t *oo = out + (size_t)o * (F + 2);
    if (!up[o]) {
        for (uint32_t i = threadIdx.x; i < F + 2; i += LB) oo[i] = -1;
        return;
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (threadIdx.x < F + 2) {  // the row's Philox draws, one lane each (thread 0 only does the arithmetic)
        uint32_t c[4];
        sel_rand(seed, round, o, threadIdx.x < F ? threadIdx.x : threadIdx.x == F ? SEL_DEAD : SEL_SEED, c);
        for (int q = 0; q < 4; q++) s_rnd[4 * threadIdx.x + q] = c[q];
    }
    const uint8_t *row = d.fd_state + (size_t)o * d.NP;
    const uint32_t nit = (d.ncol + LB * 16u - 1u) / (LB * 16u);
    uint32_t L = 0, D = 0;
#pragma unroll
    for (uint32_t h = 0; h < SEL_ROW_IT; h += 8) {  // eight steps' loads in flight at a time
        uint4 v[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            // unconditional (a clamped address, masked below): loads under a branch would be waited for one by one
            const uint32_t j0 = (h + u) * LB * 16u + threadIdx.x * 16u;
            v[u] = *reinterpret_cast<const uint4 *>(row + min(j0, d.NP - 16u));
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            const uint32_t it = h + u, j0 = it * LB * 16u + threadIdx.x * 16u;
            const bool inrow = it < nit && j0 < d.ncol;
            const uint32_t wd[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t a = 0u, b = 0u;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t jq = j0 + 4u * q;
                uint32_t keep = inrow ? 0x01010101u : 0u;  // (k_sel_count16's column mask: in range, not o's own)
                if (jq + 4u > d.ncol) keep = jq >= d.ncol ? 0u : (keep >> (8u * (jq + 4u - d.ncol)));
                const uint32_t js = o - d.col_lo - jq;
                if (js < 4u) keep &= ~(0x01u << (8u * js));
                // bit 0 of each byte -> 4 adjacent bits: bytes 0..3 times 2^21, 2^14, 2^7, 1 land on bits 21..24
                a |= (((memb_live4(wd[q]) & keep) * 0x204081u) >> 21 & 0xFu) << (4 * q);
                b |= (((memb_dead4(wd[q]) & keep) * 0x204081u) >> 21 & 0xFu) << (4 * q);
            }
            s_m[it][0][threadIdx.x] = (uint16_t)a;
            s_m[it][1][threadIdx.x] = (uint16_t)b;
            L += (uint32_t)__popc(a);
            D += (uint32_t)__popc(b);
        }
    }
    {
        const unsigned long long l = wave_sum(L), dd = wave_sum(D);
        if (lane == 0) { s_w[0][w][0] = (uint32_t)l; s_w[0][w][1] = (uint32_t)dd; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t a = 0, b = 0;
            for (uint32_t i = 0; i < LB / WAVE; i++) { a += s_w[0][i][0]; b += s_w[0][i][1]; }
            const uint32_t P = d.ncol - (o - d.col_lo < d.ncol ? 1u : 0u);  // known: every column but o's own
            scnt[o * 4 + 0] = a;
            scnt[o * 4 + 1] = b;
            scnt[o * 4 + 2] = P;
            s_cnt[0] = a;
            s_cnt[1] = b;
            uint32_t so[10];
            for (uint32_t i = 0; i < F + 2; i++) so[i] = NONE;
            sel_ranks(o, a, b, P, F, seed, round, so, s_rnd);
            for (uint32_t i = 0; i < F + 1; i++) {
                s_rank[i] = so[i];
                s_hit[i] = NONE;
            }
        }
        __syncthreads();
    }
    L = s_cnt[0];
    const bool from_live = L != 0;
    // the pool (live, or every known column when none is live) and dead ranks of every step, one block scan
    auto pool = [&](uint32_t it) {
        if (from_live) return (uint32_t)s_m[it][0][threadIdx.x];
        const uint32_t j0 = it * LB * 16u + threadIdx.x * 16u;  // every valid column
        uint32_t m = j0 >= d.ncol ? 0u : d.ncol - j0 >= 16u ? 0xFFFFu : (1u << (d.ncol - j0)) - 1u;
        const uint32_t js = o - d.col_lo - j0;
        if (js < 16u) m &= ~(1u << js);
        return m;
    };
    uint32_t ex[SEL_ROW_IT];  // the wave-exclusive scans: pool | dead << 16 (each < 2^10)
#pragma unroll
    for (uint32_t it = 0; it < SEL_ROW_IT; it++) {
        const uint32_t c2 = (uint32_t)__popc(pool(it)) | ((uint32_t)__popc((uint32_t)s_m[it][1][threadIdx.x]) << 16);
        const uint32_t i2 = wave_scan_dpp(c2);  // (both halves at once: no carry out of the low one)
        ex[it] = i2 - c2;
        if (lane == 63) { s_w[it][w][0] = i2 & 0xFFFFu; s_w[it][w][1] = i2 >> 16; }
    }
    __syncthreads();
    uint32_t bp = 0, bd = 0;  // ranks before this step
#pragma unroll
    for (uint32_t it = 0; it < SEL_ROW_IT; it++) {  // (unrolled: ex[] stays in registers)
        uint32_t op = bp + (ex[it] & 0xFFFFu), od = bd + (ex[it] >> 16);
#pragma unroll
        for (uint32_t i = 0; i < LB / WAVE; i++) {
            const uint32_t xp = s_w[it][i][0], xd = s_w[it][i][1];
            if (i < w) { op += xp; od += xd; }
            bp += xp;
            bd += xd;
        }
        const uint32_t j0 = it * LB * 16u + threadIdx.x * 16u;
        const uint32_t mp = pool(it), md = s_m[it][1][threadIdx.x];
        const uint32_t cp = (uint32_t)__popc(mp), cd = (uint32_t)__popc(md);
        if (cp) {
            for (uint32_t i = 0; i < F; i++) {
                const uint32_t r = s_rank[i];
                if (r != NONE && r >= op && r < op + cp) s_hit[i] = j0 + nth_bit16(mp, r - op);
            }
        }
        const uint32_t r = s_rank[F];
        if (cd && r != NONE && r >= od && r < od + cd) s_hit[F] = j0 + nth_bit16(md, r - od);
    }
    __syncthreads();
    if (threadIdx.x == 0) sel_seed_probe(d, o, L, s_cnt[1], F, seed, round, seeds, n_seeds, s_hit, oo, s_rnd + 4 * (F + 1));
}

// Resolve ranks to node ids in column order (one workgroup per row), then the seed probe.
// out[o][0..F) live picks, out[o][F] dead pick, out[o][F+1] seed pick (NONE = none).
__global__ __launch_bounds__(LB) void k_sel_resolve(Dev d, const uint8_t *up, const uint32_t *scnt, uint32_t F,
                                                    uint64_t seed, uint32_t round, const int32_t *seeds,
                                                    uint32_t n_seeds, const uint32_t *sel, int32_t *out) {
    __shared__ uint32_t s_w[LB / WAVE][2];
    __shared__ uint32_t s_rank[10], s_hit[10];
    const uint32_t o = blockIdx.x;
    int32_t *oo = out + (size_t)o * (F + 2);
    if (!up[o]) {
        for (uint32_t i = threadIdx.x; i < F + 2; i += LB) oo[i] = -1;
        return;
    }
    const bool genm = !(d.flags & GS_CANONICAL);
    const uint32_t L = scnt[o * 4 + 0];
    const bool from_live = L != 0;
    if (threadIdx.x < F + 1) {
        s_rank[threadIdx.x] = sel[(size_t)o * (F + 2) + threadIdx.x];
        s_hit[threadIdx.x] = NONE;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t base_pool = 0, base_dead = 0;
    for (uint32_t j0 = 0; j0 < d.ncol; j0 += LB) {
        const uint32_t j = j0 + threadIdx.x;
        bool known = false, live = false, dead = false;
        if (j < d.ncol && j != o) {
            const size_t p = pix(d, o, j);
            known = !genm || d.pos[p] != NONE;
            if (known) {
                const uint32_t st = d.fd_state[p] & FD_MEMB;
                live = st == 1u;
                dead = st >= 2u;
            }
        }
        const bool inpool = from_live ? live : known;
        const unsigned long long mp = __ballot(inpool), md = __ballot(dead);
        if (lane == 0) { s_w[w][0] = (uint32_t)__popcll(mp); s_w[w][1] = (uint32_t)__popcll(md); }
        __syncthreads();
        uint32_t op = base_pool, od = base_dead, tp = 0, td = 0;
        for (uint32_t i = 0; i < LB / WAVE; i++) {
            if (i < w) { op += s_w[i][0]; od += s_w[i][1]; }
            tp += s_w[i][0];
            td += s_w[i][1];
        }
        const uint64_t lm = (1ull << lane) - 1ull;
        const uint32_t rp = op + (uint32_t)__popcll(mp & lm), rd = od + (uint32_t)__popcll(md & lm);
        for (uint32_t i = 0; i < F; i++)
            if (inpool && s_rank[i] == rp) s_hit[i] = j;
        if (dead && s_rank[F] == rd) s_hit[F] = j;
        base_pool += tp;
        base_dead += td;
        __syncthreads();
    }
    if (threadIdx.x == 0) sel_seed_probe(d, o, L, scnt[o * 4 + 1], F, seed, round, seeds, n_seeds, s_hit, oo);
}

// Conflict-free phases for the round's exchanges e = o * (F + 2) + slot (initiator o, responder
// out[e]; exchanges whose responder is down fail before any state change, as a refused
// connection does, and are not scheduled).  Per phase p, IT rounds of a deterministic Luby
// matching: an unscheduled exchange whose two endpoints are free in p takes p if its priority
// key is the smallest at both endpoints.  busy = one bit per phase and node for 64 phases at a time (bit p mod 64;
// the host clears it every 64 phases: a phase's bits are read only while it is being filled).  Up to
// GS_MAX_SCHED_PHASES phases (round 6: the hubs of the reference's selection -- every node picks a seed while its
// live set is empty -- need as many phases as their degree); exchanges left after the last are counted, not run.
__device__ inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__device__ inline bool luby_valid(const int32_t *out, const uint8_t *up, uint32_t e, uint32_t F, uint32_t &a,
                                  uint32_t &b) {
    const int32_t t = out[e];
    if (t < 0 || !up[t]) return false;
    a = e / (F + 2);
    b = (uint32_t)t;
    return true;
}
__device__ inline bool luby_active(const int32_t *out, const uint8_t *up, const uint32_t *eph,
                                   const unsigned long long *busy, uint32_t e, uint32_t F, uint32_t p, uint32_t &a,
                                   uint32_t &b) {
    if (eph[e] != NONE) return false;
    if (!luby_valid(out, up, e, F, a, b)) return false;
    return !((busy[a] >> (p & 63u)) & 1ull) && !((busy[b] >> (p & 63u)) & 1ull);
}
__device__ inline unsigned long long luby_key(uint64_t seed, uint32_t round, uint32_t e, uint32_t p, uint32_t it) {
    const uint32_t h = fmix32(e ^ fmix32((uint32_t)seed ^ fmix32(round * 0x9E3779B9u + p * 0x632BE5ABu + it)));
    return ((unsigned long long)h << 32) | e;
}
__global__ __launch_bounds__(LB) void k_luby_min(const int32_t *out, const uint8_t *up, const uint32_t *eph,
                                                 const unsigned long long *busy, unsigned long long *best, uint32_t E,
                                                 uint32_t F, uint64_t seed, uint32_t round, uint32_t p, uint32_t it) {
    const uint32_t e = blockIdx.x * LB + threadIdx.x;
    uint32_t a, b;
    if (e >= E || !luby_active(out, up, eph, busy, e, F, p, a, b)) return;
    const unsigned long long k = luby_key(seed, round, e, p, it);
    atomicMin(&best[a], k);
    atomicMin(&best[b], k);
}
__global__ __launch_bounds__(LB) void k_luby_pick(const int32_t *out, const uint8_t *up, uint32_t *eph,
                                                  unsigned long long *busy, const unsigned long long *best,
                                                  unsigned long long *best_next, uint32_t E, uint32_t N, uint32_t F,
                                                  uint64_t seed, uint32_t round, uint32_t p, uint32_t it,
                                                  uint32_t *pcount) {
    const uint32_t x = blockIdx.x * LB + threadIdx.x;
    if (x < N) best_next[x] = ~0ull;
    uint32_t a, b;
    if (x >= E || !luby_active(out, up, eph, busy, x, F, p, a, b)) return;
    const unsigned long long k = luby_key(seed, round, x, p, it);
    if (best[a] == k && best[b] == k) {
        eph[x] = p;
        atomicOr(&busy[a], 1ull << (p & 63u));
        atomicOr(&busy[b], 1ull << (p & 63u));
        atomicAdd(&pcount[p], 1u);
    }
}
// valid exchanges not scheduled yet
__global__ __launch_bounds__(LB) void k_luby_left(const int32_t *out, const uint8_t *up, const uint32_t *eph,
                                                  uint32_t E, uint32_t F, uint32_t *left) {
    const uint32_t e = blockIdx.x * LB + threadIdx.x;
    uint32_t a, b;
    const bool l = e < E && eph[e] == NONE && luby_valid(out, up, e, F, a, b);
    const unsigned long long m = __ballot(l);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(left, (uint32_t)__popcll(m));
}
// scatter the scheduled exchanges into per-phase (initiator, responder) arrays: each workgroup ranks its
// SCAT_PER x LB exchanges per phase in LDS and takes one range per phase with a single global atomic (a
// returning atomic per exchange, or per wave and phase, serialises on the 16 or so phase counters: 0.59 ms).
// Phases past the first 64 (hub exchanges only, a few per phase) take a global atomic each.
constexpr uint32_t SCAT_PER = 4;
__global__ __launch_bounds__(LB) void k_luby_scatter(const int32_t *out, const uint32_t *eph, uint32_t E, uint32_t F,
                                                     const uint32_t *poff, uint32_t *pfill, int32_t *ini,
                                                     int32_t *res) {
    __shared__ uint32_t s_cnt[GS_MAX_PHASES], s_base[GS_MAX_PHASES];
    if (threadIdx.x < GS_MAX_PHASES) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t p[SCAT_PER], loc[SCAT_PER];
#pragma unroll
    for (uint32_t k = 0; k < SCAT_PER; k++) {
        const uint32_t e = (blockIdx.x * SCAT_PER + k) * LB + threadIdx.x;
        p[k] = e < E ? eph[e] : NONE;
        loc[k] = p[k] < GS_MAX_PHASES ? atomicAdd(&s_cnt[p[k]], 1u) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < GS_MAX_PHASES && s_cnt[threadIdx.x])
        s_base[threadIdx.x] = atomicAdd(&pfill[threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SCAT_PER; k++) {
        if (p[k] == NONE) continue;
        const uint32_t e = (blockIdx.x * SCAT_PER + k) * LB + threadIdx.x;
        const uint32_t slot = poff[p[k]] + (p[k] < GS_MAX_PHASES ? s_base[p[k]] + loc[k] : atomicAdd(&pfill[p[k]], 1u));
        ini[slot] = (int32_t)(e / (F + 2));
        res[slot] = out[e];
    }
}

}  // namespace

extern "C" {

int gs_draw_cuts(gs_handle *h, const int32_t *ini, const int32_t *res, uint32_t n, uint64_t seed, uint32_t round,
                 uint32_t phase, uint32_t loss_q32, uint8_t *legs) {
    if (!h || (n && (!ini || !res || !legs))) return GS_E_INVALID;
    if (!n) return GS_OK;
    k_draw_cuts<<<(n + LB - 1) / LB, LB, 0, h->stream>>>(ini, res, n, seed, round, phase, loss_q32, legs);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
}

extern "C++" {
namespace {
// the checks gs_draw_cuts_zoned and gs_filter_targets_zoned share, and the matrix as a kernel argument
int zone_args(gs_handle *h, const char *fn, const uint8_t *zone, const uint32_t *link, uint32_t Z, ZoneLinks &lk) {
    if (!zone) return fail(h, GS_E_INVALID, "%s: zone is NULL", fn);
    if (!link) return fail(h, GS_E_INVALID, "%s: link is NULL", fn);
    if (Z < 1 || Z > GS_MAX_ZONES) return fail(h, GS_E_INVALID, "%s: %u zones (1..%u)", fn, Z, GS_MAX_ZONES);
    if (h->sliced || h->G > 1 || h->comm)
        return fail(h, GS_E_UNSUPPORTED, "%s: zoned links run on one-slice handles only, as cut exchanges do", fn);
    memset(&lk, 0, sizeof lk);
    memcpy(lk.q, link, (size_t)Z * Z * 4);
    return GS_OK;
}
}  // namespace
}

int gs_draw_cuts_zoned(gs_handle *h, const int32_t *ini, const int32_t *res, uint32_t n, uint64_t seed, uint32_t round,
                       uint32_t phase, const uint8_t *zone, const uint32_t *link, uint32_t Z, uint8_t *legs) {
    if (!h) return GS_E_INVALID;
    if (!ini || !res) return fail(h, GS_E_INVALID, "gs_draw_cuts_zoned: initiators or responders is NULL");
    if (!legs) return fail(h, GS_E_INVALID, "gs_draw_cuts_zoned: legs is NULL");
    ZoneLinks lk;
    if (const int rc = zone_args(h, "gs_draw_cuts_zoned", zone, link, Z, lk)) return rc;
    if (!n) return GS_OK;
    k_draw_cuts_zoned<<<(n + LB - 1) / LB, LB, 0, h->stream>>>(ini, res, n, h->N, seed, round, phase, zone, lk, Z, legs);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
}

int gs_filter_targets_zoned(gs_handle *h, const int32_t *targets_in, int32_t *targets_out, uint32_t n_targets,
                            const uint8_t *zone, const uint32_t *link, uint32_t Z, uint32_t *dropped) {
    if (!h) return GS_E_INVALID;
    if (!targets_in || !targets_out)
        return fail(h, GS_E_INVALID, "gs_filter_targets_zoned: targets_in or targets_out is NULL");
    ZoneLinks lk;
    if (const int rc = zone_args(h, "gs_filter_targets_zoned", zone, link, Z, lk)) return rc;
    if (!n_targets || n_targets % h->N)
        return fail(h, GS_E_INVALID, "gs_filter_targets_zoned: %u targets are not a whole number of slots for each of "
                    "%u nodes", n_targets, h->N);
    k_zone_filter<<<(n_targets + LB - 1) / LB, LB, 0, h->stream>>>(targets_in, targets_out, n_targets, n_targets / h->N,
                                                                  h->N, zone, lk, Z, dropped);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
}

int gs_select_peers(gs_handle *h, const uint8_t *up, uint32_t fanout, const int32_t *seeds, uint32_t n_seeds,
                    uint64_t seed, uint32_t round, int32_t *targets, void *scratch) {
    if (!h || !h->booted || !up || !targets || !scratch || fanout < 1 || fanout > 8 || (n_seeds && !seeds))
        return GS_E_INVALID;
    if (h->G > 1) return fail(h, GS_E_UNSUPPORTED, "gs_select_peers needs the whole matrix (one slice)");
    uint32_t *scnt = (uint32_t *)scratch;
    uint32_t *sel = scnt + (size_t)h->N * 4;
    const bool canon = (h->cfg.flags & GS_CANONICAL) != 0;
    if (canon && h->ncol <= SEL_ROW_IT * LB * 16u && !getenv("GS_SEL_SPLIT")) {  // one read of each row
        k_sel_row16<<<h->N, LB, 0, h->stream>>>(h->d, up, fanout, seed, round, seeds, n_seeds, scnt, targets);
        HIPCHK(h, hipGetLastError());
        return GS_OK;
    }
    if (canon) k_sel_count16<<<h->N, LB, 0, h->stream>>>(h->d, up, scnt);
    else k_sel_count<<<h->N, LB, 0, h->stream>>>(h->d, up, scnt);
    HIPCHK(h, hipGetLastError());
    k_sel_pick<<<(h->N + LB - 1) / LB, LB, 0, h->stream>>>(h->d, up, scnt, fanout, seed, round, sel);
    HIPCHK(h, hipGetLastError());
    if (canon) k_sel_resolve16<<<h->N, LB, 0, h->stream>>>(h->d, up, scnt, fanout, seed, round, seeds, n_seeds, sel, targets);
    else k_sel_resolve<<<h->N, LB, 0, h->stream>>>(h->d, up, scnt, fanout, seed, round, seeds, n_seeds, sel, targets);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
}

int gs_schedule_phases(gs_handle *h, const uint8_t *up, uint32_t fanout, const int32_t *targets, uint64_t seed,
                       uint32_t round, uint32_t iters, uint32_t max_phases, void *scratch, int32_t *initiators,
                       int32_t *responders, uint32_t *phase_offsets, uint32_t *unscheduled) {
    if (!h || !up || !targets || !scratch || !initiators || !responders || !phase_offsets || !unscheduled ||
        fanout < 1 || fanout > 8 || iters < 1 || max_phases < 1 || max_phases > GS_MAX_SCHED_PHASES)
        return GS_E_INVALID;
    const uint32_t N = h->N, E = N * (fanout + 2);
    // scratch (GS_SCHED_SCRATCH_BYTES): eph[E] | pcount[P] | pfill[P] | poff[P] | left[4] | busy[N] (u64) |
    // best[2][N] (u64)
    const uint32_t P = max_phases;
    uint32_t *eph = (uint32_t *)scratch;
    uint32_t *pcount = eph + E;
    uint32_t *pfill = pcount + P;
    uint32_t *poff = pfill + P;
    uint32_t *left = poff + P;
    unsigned long long *busy = (unsigned long long *)(((uintptr_t)(left + 4) + 15) & ~(uintptr_t)15);
    unsigned long long *best = busy + N;
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(eph, 0xFF, (size_t)E * 4, s));
    HIPCHK(h, hipMemsetAsync(pcount, 0, ((size_t)3 * P + 4) * 4, s));
    HIPCHK(h, hipMemsetAsync(busy, 0, (size_t)N * 8, s));
    HIPCHK(h, hipMemsetAsync(best, 0xFF, (size_t)N * 16, s));
    const uint32_t gE = (std::max(E, N) + LB - 1) / LB;
    // the two minimum buffers alternate by the GLOBAL iteration index, so each pick resets exactly
    // the buffer the next iteration (of this phase or the next) reduces into, whatever iters is
    uint32_t g = 0, nleft = 0;
    // phases in blocks: 16 first (a round's schedule needs about 15-17 at fanout 3), then 4 at a time (the last few
    // exchanges), each block followed by one count of the exchanges still without a phase
    for (uint32_t p0 = 0, p1; p0 < max_phases; p0 = p1) {
        p1 = std::min(max_phases, p0 + (p0 ? 4u : 16u));
        // busy holds bit p mod 64: a block starting a new window of 64 phases starts from clear bits (blocks are
        // 16 then 4 phases, so windows start at block boundaries)
        if (p0 && (p0 & 63u) == 0) HIPCHK(h, hipMemsetAsync(busy, 0, (size_t)N * 8, s));
        for (uint32_t p = p0; p < p1; p++)
            for (uint32_t it = 0; it < iters; it++, g++) {
                unsigned long long *b0 = best + (size_t)(g & 1) * N, *b1 = best + (size_t)((g + 1) & 1) * N;
                k_luby_min<<<(E + LB - 1) / LB, LB, 0, s>>>(targets, up, eph, busy, b0, E, fanout, seed, round, p,
                                                            it);
                k_luby_pick<<<gE, LB, 0, s>>>(targets, up, eph, busy, b0, b1, E, N, fanout, seed, round, p, it,
                                              pcount);
            }
        // stop once every valid exchange has a phase
        HIPCHK(h, hipMemsetAsync(left, 0, 4, s));
        k_luby_left<<<(E + LB - 1) / LB, LB, 0, s>>>(targets, up, eph, E, fanout, left);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(&nleft, left, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipStreamSynchronize(s));
        if (!nleft) break;
    }
    std::vector<uint32_t> cnt(max_phases);
    HIPCHK(h, hipMemcpyAsync(cnt.data(), pcount, (size_t)max_phases * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    std::vector<uint32_t> off(max_phases + 1);
    off[0] = 0;
    for (uint32_t p = 0; p < max_phases; p++) off[p + 1] = off[p] + cnt[p];
    HIPCHK(h, hipMemcpyAsync(poff, off.data(), max_phases * 4, hipMemcpyHostToDevice, s));
    k_luby_scatter<<<(E + SCAT_PER * LB - 1) / (SCAT_PER * LB), LB, 0, s>>>(targets, eph, E, fanout, poff, pfill,
                                                                        initiators, responders);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(s));
    memcpy(phase_offsets, off.data(), (max_phases + 1) * 4);
    *unscheduled = nleft;
    return GS_OK;
}

}  // extern "C"
