// gossip_census.hip -- the read-only censuses of libgossip_sim.so: gs_view_census (dissemination), gs_age_census
// with its write log (staleness in ticks) and gs_detect_census (failure detection).  None of it is on the gossip
// round's path; the failure detector's own k_fd_census and the traffic census (it instantiates the packer) are in
// gossip_sim.hip.

#include "gossip_common.h"

namespace {

// Dissemination census (gs_view_census): a read-only streaming pass over GS_R_MV (and, with GS_VC_HEARTBEATS,
// GS_R_HB) that counts, over the observer rows with up[o] != 0, the known / unknown / behind / inexact views, the
// version- and heartbeat-lag histograms and maxima, per owner column {behind, unknown, max version lag}, per
// observer row the columns it is behind on or does not know, and the reach of up to GS_VC_MAX_PROBES
// (owner, version) probes.
// One workgroup per (band of VC_BAND consecutive observer rows, column chunk of LB x PER columns), as k_hb_lag:
// one 16-byte non-temporal load per thread, row and region, VC_AHEAD rows in flight while one is reduced; the
// owners' own values, escape slots and the probes are loaded once per workgroup.  Everything a thread counts stays
// in registers over the band (per-owner counts, packed histogram fields of VC_HBITS bits), so a band costs at most
// one atomic per (column, plane), per histogram bucket and per row of the chunk, zeros skipped.  All results are
// integer sums and maxima: they do not depend on scheduling.
// VC_BAND = 256: 65,536 x 65,536 views in chunks of 4,096 columns make 256 x 16 = 4,096 workgroups (16 per CU).
constexpr uint32_t VC_BAND = 256;
constexpr uint32_t VC_HBITS = 13;  // a thread counts at most VC_BAND x 16 = 2^12 views per band
static_assert(VC_BAND * 16u < (1u << VC_HBITS), "packed histogram fields");
// gs_view_census's device scratch (gs_handle::vc_buf): u64 accumulators, then the probes as {local column, version}
enum VcSlot {
    VC_OBS = 0, VC_VIEWS, VC_UNK, VC_BEHIND, VC_INEX, VC_MAXV, VC_MAXH,
    VC_VH, VC_HH = VC_VH + GS_VC_BUCKETS, VC_REACH = VC_HH + GS_VC_BUCKETS, VC_NUM = VC_REACH + GS_VC_MAX_PROBES
};
struct VcArgs {
    const uint8_t *up;         // nullptr: every row counts
    uint32_t flags, n_probes;
    unsigned long long *acc;   // [VC_NUM], zeroed
    const uint32_t *probes;    // [n_probes][2] {local column or NONE, version}
    uint32_t *owners, *rows;   // optional outputs, zeroed
};
__device__ __forceinline__ uint32_t wave_sum32(uint32_t x) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) x += __shfl_xor(x, dd, WAVE);
    return x;
}
__device__ __forceinline__ uint32_t wave_max32(uint32_t x) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) x = max(x, (uint32_t)__shfl_xor(x, dd, WAVE));
    return x;
}
// lag bucket (GS_VC_BUCKETS): 0 for lag 0, else min(19, bit length)
__device__ __forceinline__ uint32_t vc_bucket(uint32_t lag) { return min(GS_VC_BUCKETS - 1u, 32u - (uint32_t)__clz(lag)); }
// bit 7 of each byte -> the whole byte
__device__ __forceinline__ uint32_t bytes7(uint32_t b7) { return (b7 >> 7) * 0xFFu; }
// per-byte maximum of two words whose bytes are all < 2^7
__device__ __forceinline__ uint32_t bmax7(uint32_t x, uint32_t y) {
    const uint32_t ge = bytes7(((x | B7) - y) & B7);  // bytes where x >= y
    return (x & ge) | (y & ~ge);
}
constexpr uint32_t VC_AHEAD = 3;  // rows in flight per thread: 16 waves per CU x 3 rows x 16 B per lane and region
template <bool SWAR>
__global__ __launch_bounds__(LB, 4) void k_view_census(Dev d, VcArgs a, uint32_t chunks) {
    constexpr uint32_t PER = SWAR ? 16u : 8u;  // views per thread and row: one 16-byte load of the widest region
    __shared__ uint32_t s_hist[2][GS_VC_BUCKETS];
    __shared__ uint32_t s_rows[VC_BAND];
    __shared__ uint32_t s_pi[GS_VC_MAX_PROBES];
    __shared__ uint32_t s_pn;
    // SWAR: an escaped column's own heartbeat mod 2^16 | slot << 16, per thread and column (read only for escaped
    // columns, so it lives here and not in registers)
    __shared__ uint32_t s_escpk[SWAR ? 16 : 1][LB];
    const bool genm = !(d.flags & GS_CANONICAL);
    const bool wantH = a.flags & GS_VC_HEARTBEATS;
    const uint32_t tid = threadIdx.x;
    const uint32_t rb = blockIdx.x / chunks, cb = blockIdx.x % chunks;
    const uint32_t c_lo = cb * LB * PER, j0 = c_lo + tid * PER;
    const uint32_t o0 = rb * VC_BAND, nrow = min(VC_BAND, d.N - o0);
    const bool act = j0 < d.ncol;
    const uint32_t nvt = act ? min(d.ncol - j0, PER) : 0u;  // this thread's real columns (padding is never counted)
    for (uint32_t i = tid; i < 2u * GS_VC_BUCKETS; i += LB) (&s_hist[0][0])[i] = 0u;
    for (uint32_t i = tid; i < VC_BAND; i += LB) s_rows[i] = 0u;
    if (tid == 0) s_pn = 0u;
    __syncthreads();
    // the probes whose owner column lies in this chunk (none: the probes cost this workgroup nothing more)
    if (tid < a.n_probes) {
        const uint32_t c = a.probes[2u * tid];
        if (c != NONE && c >= c_lo && c < c_lo + LB * PER) s_pi[atomicAdd(&s_pn, 1u)] = tid;
    }
    __syncthreads();
    const uint32_t npc = s_pn;
    uint32_t p_i = 0, p_c = 0, p_v = 0, p_M = 0, p_reach = 0;  // thread i < npc counts probe s_pi[i] over the band
    if (tid < npc) {
        p_i = s_pi[tid];
        p_c = a.probes[2u * p_i];
        p_v = a.probes[2u * p_i + 1u];
        p_M = d.self_mv[p_c];
    }
    // the owners' own values and escape slots: the same for every row of the band
    uint32_t own8v[4], owm7v[4], vm7v[4], esc7v[4];  // SWAR: four columns per word (k_hb_lag)
    uint32_t ownR[SWAR ? 1 : 8], ownM[SWAR ? 1 : 8], slot[SWAR ? 1 : 8];  // per column
    if constexpr (SWAR) {
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            const uint32_t jq = j0 + 4u * q;
            own8v[q] = owm7v[q] = vm7v[q] = esc7v[q] = 0u;
            if (jq >= d.ncol) continue;
            const uint4 pk = *reinterpret_cast<const uint4 *>(d.self_pk + jq);
            own8v[q] = (pk.x & 0xFFu) | ((pk.y & 0xFFu) << 8) | ((pk.z & 0xFFu) << 16) | (pk.w << 24);
            owm7v[q] = ((pk.x >> 16) & 0x7Fu) | (((pk.y >> 16) & 0x7Fu) << 8) | (((pk.z >> 16) & 0x7Fu) << 16) |
                       (((pk.w >> 16) & 0x7Fu) << 24);
            const uint32_t nv = min(d.ncol - jq, 4u);
            vm7v[q] = nv >= 4u ? B7 : B7 & ((1u << (8u * nv)) - 1u);  // bit 7 of the real columns
            if (d.EC && wantH) {
                uint32_t es[4], R[4];
                ld4(d.esc_slot + jq, es);
                ld4(d.self_hb + jq, R);
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    if (es[i] == NONE) continue;
                    esc7v[q] |= 0x80u << (8u * i);
                    s_escpk[4u * q + i][tid] = (R[i] & 0xFFFFu) | (es[i] << 16);  // (read back by this thread only)
                }
                esc7v[q] &= vm7v[q];
            }
        }
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 2u; q++) {
            const uint32_t jq = j0 + 4u * q;
            uint32_t R[4] = {0u, 0u, 0u, 0u}, M[4] = {0u, 0u, 0u, 0u}, es[4] = {NONE, NONE, NONE, NONE};
            if (jq < d.ncol) {
                ld4(d.self_hb + jq, R);
                ld4(d.self_mv + jq, M);
                if (d.EC) ld4(d.esc_slot + jq, es);
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) { ownR[4u * q + i] = R[i]; ownM[4u * q + i] = M[i]; slot[4u * q + i] = es[i]; }
        }
    }
    // one 16-byte load per region and row (8 bytes where this path's 8 views are bytes), VC_AHEAD rows ahead
    v4u_t bh[VC_AHEAD], bm[VC_AHEAD];
    auto ldv = [&](uint32_t o, v4u_t &nh, v4u_t &nm) {
        nh = nm = v4u_t{0u, 0u, 0u, 0u};
        if (!act) return;
        const size_t p0 = pix(d, o, j0);
        const uint8_t *m8 = reinterpret_cast<const uint8_t *>(d.mv), *h8 = reinterpret_cast<const uint8_t *>(d.hb);
        if (SWAR) {
            nm = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(m8 + p0));
            if (wantH) nh = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(h8 + p0));
            return;
        }
        if (d.mv8) {
            const v2u_t x = __builtin_nontemporal_load(reinterpret_cast<const v2u_t *>(m8 + p0));
            nm.x = x.x; nm.y = x.y;
        } else {
            nm = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.mv + p0));
        }
        if (!wantH) return;
        if (d.hb8) {
            const v2u_t x = __builtin_nontemporal_load(reinterpret_cast<const v2u_t *>(h8 + p0));
            nh.x = x.x; nh.y = x.y;
        } else {
            nh = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.hb + p0));
        }
    };
#pragma unroll
    for (uint32_t u = 0; u < VC_AHEAD; u++) ldv(o0 + min(u, nrow - 1u), bh[u], bm[u]);
    uint32_t t_views = 0, t_unk = 0, t_inex = 0, t_maxh = 0, n_obs = 0;
    // per owner column, over the band.  SWAR: behind counts as bytes (widened to 16-bit pairs every 128 rows: beh[2 q]
    // holds columns 4 q and 4 q + 2, beh[2 q + 1] columns 4 q + 1 and 4 q + 3), largest lags as bytes (mxv[q])
    uint32_t beh[8], unk[SWAR ? 1 : 8], mxv[SWAR ? 4 : 8];
    uint32_t beh8[4] = {0u, 0u, 0u, 0u};
    // histogram fields of VC_HBITS bits: buckets 1-4 and 5-8 (SWAR: every lag < 2^8); the other path keeps buckets
    // 1-4 here and sends the rare wider lags to the workgroup's LDS histogram
    unsigned long long vlo = 0ull, vhi = 0ull, hlo = 0ull, hhi = 0ull;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) beh[k] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < (SWAR ? 4u : 8u); k++) mxv[k] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < (SWAR ? 1u : 8u); k++) unk[k] = 0u;
    auto hadd = [&](unsigned long long &lo, unsigned long long &hi, uint32_t pl, uint32_t lag) {
        const uint32_t b = vc_bucket(lag) - 1u;  // lag != 0
        const unsigned long long inc = 1ull << (VC_HBITS * (b & 3u));
        if (b < 4u) lo += inc;
        else if (SWAR && b < 8u) hi += inc;
        else atomicAdd(&s_hist[pl][b + 1u], 1u);
    };
    // one row of the band: hr / mr = this thread's views of observer o
    auto row = [&](uint32_t r, const v4u_t hr, const v4u_t mr) {
        const uint32_t o = o0 + r;
        const bool counted = !a.up || a.up[o];
        if (counted) {
            n_obs++;
            uint32_t rowc = 0;  // this thread's columns the row is behind on or does not know
            if (act) {
                const uint32_t hw[4] = {hr.x, hr.y, hr.z, hr.w}, mw[4] = {mr.x, mr.y, mr.z, mr.w};
                if constexpr (SWAR) {
                    t_views += nvt;
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) {
                        const uint32_t vm7 = vm7v[q], vmask = bytes7(vm7);
                        t_inex += (uint32_t)__popc(mw[q] & vm7);
                        const uint32_t lagM = ((owm7v[q] | B7) - (mw[q] & L7)) & L7 & vmask;  // (own - view) mod 2^7
                        if (lagM) {  // only non-zero lags go one view at a time (the histogram)
                            const uint32_t nz = (lagM + L7) & B7;
                            beh8[q] += nz >> 7;
                            rowc += (uint32_t)__popc(nz);
                            mxv[q] = bmax7(mxv[q], lagM);
#pragma unroll
                            for (uint32_t i = 0; i < 4; i++) {
                                const uint32_t l = (lagM >> (8u * i)) & 0x7Fu;
                                if (l) hadd(vlo, vhi, 0u, l);
                            }
                        }
                        if (!wantH) continue;
                        const uint32_t esc7 = esc7v[q];
                        const uint32_t lagH = bsub(own8v[q], hw[q]) & vmask & ~bytes7(esc7);  // (own - view) mod 2^8
                        if (lagH) {
#pragma unroll
                            for (uint32_t i = 0; i < 4; i++) {
                                const uint32_t l = (lagH >> (8u * i)) & 0xFFu;
                                if (!l) continue;
                                t_maxh = max(t_maxh, l);
                                hadd(hlo, hhi, 1u, l);
                            }
                        }
                        if (esc7) {  // escaped columns: 16-bit views in GS_R_ESC16, one at a time
#pragma unroll
                            for (uint32_t i = 0; i < 4; i++) {
                                if (!((esc7 >> (8u * i + 7u)) & 1u)) continue;
                                const uint32_t pk = s_escpk[4u * q + i][tid];
                                const uint32_t l = (pk - d.esc16[(size_t)o * d.EC + (pk >> 16)]) & 0xFFFFu;
                                if (!l) continue;
                                t_maxh = max(t_maxh, l);
                                atomicAdd(&s_hist[1][vc_bucket(l)], 1u);
                            }
                        }
                    }
                } else {
                    const size_t p0 = pix(d, o, j0);
                    uint32_t ps[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                    if (genm) {
                        const uint4 x = *reinterpret_cast<const uint4 *>(d.pos + p0), y = *reinterpret_cast<const uint4 *>(d.pos + p0 + 4);
                        ps[0] = x.x; ps[1] = x.y; ps[2] = x.z; ps[3] = x.w; ps[4] = y.x; ps[5] = y.y; ps[6] = y.z; ps[7] = y.w;
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 8u; k++) {
                        if (k >= nvt) continue;
                        if (genm && ps[k] == NONE) {
                            unk[SWAR ? 0 : k]++;
                            t_unk++;
                            rowc++;
                            continue;
                        }
                        t_views++;
                        const uint32_t w = d.mv8 ? mv_dec8((mw[k >> 2] >> (8u * (k & 3u))) & 0xFFu, ownM[SWAR ? 0 : k])
                                                 : (mw[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
                        t_inex += w >> 15;
                        const uint32_t l = ownM[SWAR ? 0 : k] - (w & MV_MASK);
                        if (l) {
                            beh[k]++;
                            rowc++;
                            mxv[SWAR ? 0 : k] = max(mxv[SWAR ? 0 : k], l);
                            hadd(vlo, vhi, 0u, l);
                        }
                        if (!wantH) continue;
                        uint32_t lh;
                        const uint32_t R = ownR[SWAR ? 0 : k], sl = slot[SWAR ? 0 : k];
                        if (sl != NONE) lh = (R - d.esc16[(size_t)o * d.EC + sl]) & 0xFFFFu;
                        else if (d.hb8) lh = (R - ((hw[k >> 2] >> (8u * (k & 3u))) & 0xFFu)) & 0xFFu;
                        else lh = (R - ((hw[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu)) & 0xFFFFu;
                        if (lh) {
                            t_maxh = max(t_maxh, lh);
                            hadd(hlo, hhi, 1u, lh);
                        }
                    }
                }
            }
            if (a.rows && __ballot(rowc != 0u)) {  // one wave reduction; one global atomic per (row, chunk) below
                const uint32_t s = wave_sum32(rowc);
                if ((tid & 63u) == 0u && s) atomicAdd(&s_rows[r], s);
            }
            if (tid < npc) {
                const size_t p = pix(d, o, p_c);
                if (!genm || d.pos[p] != NONE) {
                    const uint32_t w = d.mv8 ? mv_dec8(reinterpret_cast<const uint8_t *>(d.mv)[p], p_M) : (uint32_t)d.mv[p];
                    p_reach += (w & MV_MASK) >= p_v;
                }
            }
        }
        if constexpr (SWAR) {
            if ((r & 127u) == 127u || r + 1u == nrow) {  // byte counters hold 128 rows: widen to 16-bit pairs
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    beh[2u * q] += beh8[q] & 0x00FF00FFu;
                    beh[2u * q + 1u] += (beh8[q] >> 8) & 0x00FF00FFu;
                    beh8[q] = 0u;
                }
            }
        }
    };
    for (uint32_t r0 = 0; r0 < nrow; r0 += VC_AHEAD) {
#pragma unroll
        for (uint32_t u = 0; u < VC_AHEAD; u++) {
            const uint32_t r = r0 + u;
            if (r >= nrow) break;
            const v4u_t hr = bh[u], mr = bm[u];
            ldv(o0 + min(r + VC_AHEAD, nrow - 1u), bh[u], bm[u]);  // (past the band: the last row again, unused)
            row(r, hr, mr);
        }
    }
    // the band's results: at most one atomic per (column, plane), zeros skipped
    uint32_t t_beh = 0, t_maxv = 0;
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        uint32_t bk, mk, uk = 0u;
        if constexpr (SWAR) {  // column k = 4 q + i: count in beh[2 q + (i & 1)], half i >> 1; lag in byte i of mxv[q]
            bk = (beh[2u * (k >> 2) + (k & 1u)] >> (16u * ((k >> 1) & 1u))) & 0xFFFFu;
            mk = (mxv[k >> 2] >> (8u * (k & 3u))) & 0xFFu;
        } else {
            bk = beh[k & 7u];
            mk = mxv[SWAR ? 0 : (k & 7u)];
            uk = unk[SWAR ? 0 : (k & 7u)];
        }
        t_beh += bk;
        t_maxv = max(t_maxv, mk);
        if (!a.owners || k >= nvt) continue;
        if (bk) atomicAdd(&a.owners[j0 + k], bk);
        if (uk) atomicAdd(&a.owners[d.ncol + j0 + k], uk);
        if (mk) atomicMax(&a.owners[2u * d.ncol + j0 + k], mk);
    }
#pragma unroll
    for (uint32_t b = 0; b < 4u; b++) {
        const uint32_t m = (1u << VC_HBITS) - 1u, sh = VC_HBITS * b;
        const uint32_t c0 = (uint32_t)(vlo >> sh) & m, c1 = (uint32_t)(vhi >> sh) & m;
        const uint32_t c2 = (uint32_t)(hlo >> sh) & m, c3 = (uint32_t)(hhi >> sh) & m;
        if (c0) atomicAdd(&s_hist[0][1u + b], c0);
        if (c1) atomicAdd(&s_hist[0][5u + b], c1);
        if (c2) atomicAdd(&s_hist[1][1u + b], c2);
        if (c3) atomicAdd(&s_hist[1][5u + b], c3);
    }
    {
        const uint32_t lane0 = (tid & 63u) == 0u;
        const unsigned long long sv = wave_sum(t_views), su = wave_sum(t_unk), sb = wave_sum(t_beh), si = wave_sum(t_inex);
        const uint32_t mv_ = wave_max32(t_maxv), mh_ = wave_max32(t_maxh);
        if (lane0) {
            if (sv) atomicAdd(&a.acc[VC_VIEWS], sv);
            if (su) atomicAdd(&a.acc[VC_UNK], su);
            if (sb) atomicAdd(&a.acc[VC_BEHIND], sb);
            if (si) atomicAdd(&a.acc[VC_INEX], si);
            if (mv_) atomicMax(&a.acc[VC_MAXV], (unsigned long long)mv_);
            if (mh_) atomicMax(&a.acc[VC_MAXH], (unsigned long long)mh_);
        }
    }
    if (cb == 0 && tid == 0 && n_obs) atomicAdd(&a.acc[VC_OBS], (unsigned long long)n_obs);
    if (tid < npc && p_reach) atomicAdd(&a.acc[VC_REACH + p_i], (unsigned long long)p_reach);
    __syncthreads();
    for (uint32_t i = tid; i < 2u * GS_VC_BUCKETS; i += LB) {
        const uint32_t c = (&s_hist[0][0])[i];
        if (c) atomicAdd(&a.acc[VC_VH + i], (unsigned long long)c);
    }
    if (a.rows)
        for (uint32_t i = tid; i < nrow; i += LB)
            if (s_rows[i]) atomicAdd(&a.rows[o0 + i], s_rows[i]);
}

// Age census (gs_age_census): k_view_census's streaming pass over GS_R_MV, in ticks.  The caller's write log
// wlog[ncol][WL] holds the tick at which each owner's max_version was first seen at each value (gs_note_writes); a
// counted view at version v < M (M = the owner's own max_version) is behind, and its age is tick - wlog[j][v + 1],
// the age of the oldest write its max_version does not cover (NONE there: counted in unlogged and nowhere else).
// A pair the observer does not know (general layout) is a view at version 0.
// The same workgroups as k_view_census: (band of VC_BAND rows, column chunk of LB x PER columns), one 16-byte
// non-temporal load per thread and row, VC_AHEAD rows in flight, the owners' own versions loaded once.  In the
// canonical 8-bit layout (SWAR) a row's 16 views are four words whose lags come out four at a time; a row with no
// lag costs nothing more.  Only a view that is behind gathers its log entry: a row's gathers are issued together,
// before any is used, and a chunk's log rows are shared by the whole band (and by the bands beside it), so they
// come from L2.  Over the band a thread keeps, per column, the largest lag (= the smallest version seen, the
// column's floor: one atomicMin per (band, column), none when it equals M), the age histogram as packed fields of
// VC_HBITS bits, and the maxima; a row's largest age takes one wave reduction and one atomic per (row, chunk).
// All results are integer sums, minima and maxima: they do not depend on scheduling.
enum AcSlot {
    AC_OBS = 0, AC_UNK, AC_BEHIND, AC_UNLOG, AC_MAXAGE, AC_SPREAD, AC_PENDING, AC_UNLOG_W, AC_MAXSPREAD, AC_MAXPEND,
    AC_AH, AC_SH = AC_AH + GS_VC_BUCKETS, AC_PH = AC_SH + GS_VC_BUCKETS, AC_NUM = AC_PH + GS_VC_BUCKETS
};
struct AcArgs {
    const uint8_t *up;         // nullptr: every row counts
    const uint32_t *wlog;      // [ncol][WL]
    uint32_t WL, tick;
    unsigned long long *acc;   // [AC_NUM], zeroed
    uint32_t *floor;           // [ncol], preset to the owners' own max_version
    uint32_t *rows;            // optional, zeroed
    uint32_t *done;            // optional, in/out (k_age_owners)
};
template <bool SWAR>
__global__ __launch_bounds__(LB, 4) void k_age_census(Dev d, AcArgs a, uint32_t chunks) {
    constexpr uint32_t PER = SWAR ? 16u : 8u;  // views per thread and row (k_view_census)
    __shared__ uint32_t s_hist[GS_VC_BUCKETS];
    __shared__ uint32_t s_rows[VC_BAND];
    __shared__ uint32_t s_M[SWAR ? 16 : 1][LB];  // SWAR: the owners' full max_version, read only for views behind
    const bool genm = !(d.flags & GS_CANONICAL);
    const uint32_t tid = threadIdx.x;
    const uint32_t rb = blockIdx.x / chunks, cb = blockIdx.x % chunks;
    const uint32_t j0 = cb * LB * PER + tid * PER;
    const uint32_t o0 = rb * VC_BAND, nrow = min(VC_BAND, d.N - o0);
    const bool act = j0 < d.ncol;
    const uint32_t nvt = act ? min(d.ncol - j0, PER) : 0u;  // this thread's real columns
    for (uint32_t i = tid; i < GS_VC_BUCKETS; i += LB) s_hist[i] = 0u;
    for (uint32_t i = tid; i < VC_BAND; i += LB) s_rows[i] = 0u;
    uint32_t owm7v[4], vm7v[4];   // SWAR: four columns per word
    uint32_t ownM[SWAR ? 1 : 8];  // per column
#pragma unroll
    for (uint32_t q = 0; q < PER / 4u; q++) {
        const uint32_t jq = j0 + 4u * q;
        uint32_t M[4] = {0u, 0u, 0u, 0u};
        if (jq < d.ncol) ld4(d.self_mv + jq, M);
        if constexpr (SWAR) {
            owm7v[q] = (M[0] & 0x7Fu) | ((M[1] & 0x7Fu) << 8) | ((M[2] & 0x7Fu) << 16) | ((M[3] & 0x7Fu) << 24);
            const uint32_t nv = jq < d.ncol ? min(d.ncol - jq, 4u) : 0u;
            vm7v[q] = nv >= 4u ? B7 : B7 & ((1u << (8u * nv)) - 1u);  // bit 7 of the real columns
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) s_M[4u * q + i][tid] = M[i];  // (read back by this thread only)
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; i++) ownM[4u * q + i] = M[i];
        }
    }
    __syncthreads();
    v4u_t bm[VC_AHEAD];
    auto ldv = [&](uint32_t o, v4u_t &nm) {
        nm = v4u_t{0u, 0u, 0u, 0u};
        if (!act) return;
        const size_t p0 = pix(d, o, j0);
        const uint8_t *m8 = reinterpret_cast<const uint8_t *>(d.mv);
        if (SWAR) {
            nm = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(m8 + p0));
        } else if (d.mv8) {
            const v2u_t x = __builtin_nontemporal_load(reinterpret_cast<const v2u_t *>(m8 + p0));
            nm.x = x.x; nm.y = x.y;
        } else {
            nm = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.mv + p0));
        }
    };
#pragma unroll
    for (uint32_t u = 0; u < VC_AHEAD; u++) ldv(o0 + min(u, nrow - 1u), bm[u]);
    uint32_t t_unk = 0, t_beh = 0, t_unlog = 0, t_maxage = 0, n_obs = 0;
    uint32_t mxl[SWAR ? 4 : 8];  // the largest lag per column over the band (SWAR: as bytes)
#pragma unroll
    for (uint32_t k = 0; k < (SWAR ? 4u : 8u); k++) mxl[k] = 0u;
    unsigned long long ah[5] = {0ull, 0ull, 0ull, 0ull, 0ull};  // bucket b: field b & 3 of ah[b >> 2]
    // the views of one row that are behind, lag[k] != 0: gather their log entries together, then count them
    auto ages = [&](const uint32_t (&lag)[PER], uint32_t &rowm) {
        uint32_t e[PER];
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            e[k] = NONE;
            if (!lag[k]) continue;
            uint32_t Mk;
            if constexpr (SWAR) Mk = s_M[k][tid];
            else Mk = ownM[k];
            const uint32_t w = Mk - lag[k] + 1u;  // the oldest write the view lacks (1 <= w <= M)
            if (w < a.WL) e[k] = a.wlog[(size_t)(j0 + k) * a.WL + w];
        }
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            if (!lag[k]) continue;
            t_beh++;
            if (e[k] == NONE) { t_unlog++; continue; }
            const uint32_t age = a.tick - e[k];
            rowm = max(rowm, age);
            const uint32_t b = vc_bucket(age);
            const unsigned long long inc = 1ull << (VC_HBITS * (b & 3u));
#pragma unroll
            for (uint32_t g = 0; g < 5u; g++) ah[g] += (b >> 2) == g ? inc : 0ull;
        }
    };
    auto row = [&](uint32_t r, const v4u_t mr) {
        const uint32_t o = o0 + r;
        if (a.up && !a.up[o]) return;
        n_obs++;
        uint32_t rowm = 0;  // this thread's largest age in the row
        if (act) {
            const uint32_t mw[4] = {mr.x, mr.y, mr.z, mr.w};
            uint32_t lag[PER];
            if constexpr (SWAR) {
                uint32_t lagM[4], any = 0u;
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    lagM[q] = ((owm7v[q] | B7) - (mw[q] & L7)) & L7 & bytes7(vm7v[q]);  // (own - view) mod 2^7
                    any |= lagM[q];
                }
                if (any) {
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++) {
                        mxl[q] = bmax7(mxl[q], lagM[q]);
#pragma unroll
                        for (uint32_t i = 0; i < 4; i++) lag[4u * q + i] = (lagM[q] >> (8u * i)) & 0x7Fu;
                    }
                    ages(lag, rowm);
                }
            } else {
                const size_t p0 = pix(d, o, j0);
                uint32_t ps[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
                if (genm) {
                    const uint4 x = *reinterpret_cast<const uint4 *>(d.pos + p0), y = *reinterpret_cast<const uint4 *>(d.pos + p0 + 4);
                    ps[0] = x.x; ps[1] = x.y; ps[2] = x.z; ps[3] = x.w; ps[4] = y.x; ps[5] = y.y; ps[6] = y.z; ps[7] = y.w;
                }
                uint32_t any = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 8u; k++) {
                    lag[k] = 0u;
                    if (k >= nvt) continue;
                    uint32_t v = 0u;  // a pair the observer does not know: a view at version 0
                    if (genm && ps[k] == NONE) {
                        t_unk++;
                    } else {
                        const uint32_t w = d.mv8 ? mv_dec8((mw[k >> 2] >> (8u * (k & 3u))) & 0xFFu, ownM[SWAR ? 0 : k])
                                                 : (mw[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
                        v = w & MV_MASK;
                    }
                    lag[k] = ownM[SWAR ? 0 : k] - v;
                    mxl[SWAR ? 0 : k] = max(mxl[SWAR ? 0 : k], lag[k]);
                    any |= lag[k];
                }
                if (any) ages(lag, rowm);
            }
        }
        t_maxage = max(t_maxage, rowm);
        if (a.rows && __ballot(rowm != 0u)) {  // one wave reduction; one global atomic per (row, chunk) below
            const uint32_t m = wave_max32(rowm);
            if ((tid & 63u) == 0u) atomicMax(&s_rows[r], m);
        }
    };
    for (uint32_t r0 = 0; r0 < nrow; r0 += VC_AHEAD) {
#pragma unroll
        for (uint32_t u = 0; u < VC_AHEAD; u++) {
            const uint32_t r = r0 + u;
            if (r >= nrow) break;
            const v4u_t mr = bm[u];
            ldv(o0 + min(r + VC_AHEAD, nrow - 1u), bm[u]);  // (past the band: the last row again, unused)
            row(r, mr);
        }
    }
    // the band's results: at most one atomicMin per column, none where no counted view is behind
#pragma unroll
    for (uint32_t k = 0; k < PER; k++) {
        if (k >= nvt) continue;
        uint32_t lk, Mk;
        if constexpr (SWAR) {
            lk = (mxl[k >> 2] >> (8u * (k & 3u))) & 0x7Fu;
            Mk = s_M[k][tid];
        } else {
            lk = mxl[SWAR ? 0 : k];
            Mk = ownM[SWAR ? 0 : k];
        }
        if (lk) atomicMin(&a.floor[j0 + k], Mk - lk);
    }
#pragma unroll
    for (uint32_t b = 0; b < GS_VC_BUCKETS; b++) {
        const uint32_t c = (uint32_t)(ah[b >> 2] >> (VC_HBITS * (b & 3u))) & ((1u << VC_HBITS) - 1u);
        if (c) atomicAdd(&s_hist[b], c);
    }
    {
        const unsigned long long su = wave_sum(t_unk), sb = wave_sum(t_beh), sl = wave_sum(t_unlog);
        const uint32_t ma = wave_max32(t_maxage);
        if ((tid & 63u) == 0u) {
            if (su) atomicAdd(&a.acc[AC_UNK], su);
            if (sb) atomicAdd(&a.acc[AC_BEHIND], sb);
            if (sl) atomicAdd(&a.acc[AC_UNLOG], sl);
            if (ma) atomicMax(&a.acc[AC_MAXAGE], (unsigned long long)ma);
        }
    }
    if (cb == 0 && tid == 0 && n_obs) atomicAdd(&a.acc[AC_OBS], (unsigned long long)n_obs);
    __syncthreads();
    for (uint32_t i = tid; i < GS_VC_BUCKETS; i += LB)
        if (s_hist[i]) atomicAdd(&a.acc[AC_AH + i], (unsigned long long)s_hist[i]);
    if (a.rows)
        for (uint32_t i = tid; i < nrow; i += LB)
            if (s_rows[i]) atomicMax(&a.rows[o0 + i], s_rows[i]);
}

// The owner pass of gs_age_census, one thread per owner column, after k_age_census (nothing with no counted observer).
// f = the column's floor, d0 = done[j] (f without done): the versions in (d0, f] have now reached every counted observer
// (credited once: done[j] = max(d0, f)); those in (max(d0, f), M] are not yet everywhere.
__global__ __launch_bounds__(LB) void k_age_owners(Dev d, AcArgs a) {
    __shared__ uint32_t s_h[2][GS_VC_BUCKETS];
    __shared__ uint32_t s_mx[2];
    for (uint32_t i = threadIdx.x; i < 2u * GS_VC_BUCKETS; i += LB) (&s_h[0][0])[i] = 0u;
    if (threadIdx.x < 2u) s_mx[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t j = blockIdx.x * LB + threadIdx.x;
    uint32_t n_spread = 0, n_pend = 0, n_unlog = 0;
    if (j < d.ncol && a.acc[AC_OBS]) {
        const uint32_t *wl = a.wlog + (size_t)j * a.WL;
        const uint32_t M = min(d.self_mv[j], a.WL - 1u), f = min(a.floor[j], M);
        const uint32_t d0 = a.done ? a.done[j] : f, top = max(d0, f);
        for (uint32_t w = d0 + 1u; w <= f; w++) {  // (runs only with done)
            const uint32_t e = wl[w];
            if (e == NONE) { n_unlog++; continue; }
            n_spread++;
            atomicAdd(&s_h[0][vc_bucket(a.tick - e)], 1u);
            atomicMax(&s_mx[0], a.tick - e);
        }
        if (a.done && f > d0) a.done[j] = f;
        for (uint32_t w = top + 1u; w <= M; w++) {
            const uint32_t e = wl[w];
            if (e == NONE) { n_unlog++; continue; }
            n_pend++;
            atomicAdd(&s_h[1][vc_bucket(a.tick - e)], 1u);
            atomicMax(&s_mx[1], a.tick - e);
        }
    }
    const unsigned long long ss = wave_sum(n_spread), sp = wave_sum(n_pend), su = wave_sum(n_unlog);
    if ((threadIdx.x & 63u) == 0u) {
        if (ss) atomicAdd(&a.acc[AC_SPREAD], ss);
        if (sp) atomicAdd(&a.acc[AC_PENDING], sp);
        if (su) atomicAdd(&a.acc[AC_UNLOG_W], su);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2u * GS_VC_BUCKETS; i += LB) {
        const uint32_t c = (&s_h[0][0])[i];
        if (c) atomicAdd(&a.acc[AC_SH + i], (unsigned long long)c);
    }
    if (threadIdx.x < 2u && s_mx[threadIdx.x]) atomicMax(&a.acc[AC_MAXSPREAD + threadIdx.x], (unsigned long long)s_mx[threadIdx.x]);
}

// gs_note_writes: the tick at which each owner's max_version was first seen at its current value
__global__ __launch_bounds__(LB) void k_note_writes(Dev d, uint32_t *wlog, uint32_t WL, uint32_t tick) {
    const uint32_t j = blockIdx.x * LB + threadIdx.x;
    if (j >= d.ncol) return;
    const uint32_t v = d.self_mv[j];
    if (!v || v >= WL) return;
    uint32_t *e = wlog + (size_t)j * WL + v;
    if (*e == NONE) *e = tick;
}

// Detection census (gs_detect_census): a read-only streaming pass over GS_R_FD_STATE -- and, with thresholds (PHI),
// over GS_R_FD_LAST and GS_R_FD -- that counts, over the pairs (observer o up, target j != o), the live / dead /
// unknown pairs by whether the target is up, the detection latencies (time of death - down_since), the ages of
// the undetected failures and of the false suspicions, and the pairs whose phi exceeds each swept threshold.
// k_view_census's access pattern: one workgroup per (band of DC_BAND observer rows, chunk of LB x 16 columns), one
// 16-byte non-temporal load of the state bytes per thread and row, rows in flight ahead of the one being reduced;
// rows that are not counted are neither loaded nor reduced (a wave-uniform choice).  The rows counted are those of
// DcArgs.obs, the targets' truth is DcArgs.up: gs_detect_census passes one array for both, gs_detect_census_for two
// (an observer set that is one side of a partition, against what that side can reach).  The chunk's up bytes become two
// byte masks per word (held in registers), down_since lives in LDS.
// State only: four pairs per 32-bit word -- live and dead bytes by two bit operations, masked by the targets'
// validity, accumulated in byte counters (widened every 128 rows).  The totals and the undetected ages follow from
// the per-column counts at the end of the band (the age depends on the column alone).  Dead pairs go one at a time:
// their time of death is loaded, bucketed into the workgroup's LDS histogram and folded into the column's
// smallest / largest time of death.
// PHI: per pair with a window, phi first in binary32 and division-free (numerator against threshold x denominator);
// a value clear of every threshold by 2^-10 relative (the binary32 error is below 2^-20) counts for all or none of
// them, any other is recomputed with k_phi_row's binary64
// expression and compared with each threshold.  All results are integer sums, minima and maxima.
constexpr uint32_t DC_BAND = 256;
enum DcSlot {
    DC_OBS = 0, DC_UP_PAIRS, DC_UP_LIVE, DC_UP_DEAD, DC_DN_PAIRS, DC_DN_LIVE, DC_DN_DEAD, DC_UP_WIN, DC_DN_WIN,
    DC_UP_PHI, DC_DN_PHI, DC_OLD, DC_EARLY, DC_MAX /* latency, undetected age, false age */, DC_HIST = DC_MAX + 3,
    DC_OVER = DC_HIST + 3 * GS_DC_BUCKETS, DC_NUM = DC_OVER + 2 * GS_DC_MAX_THRESHOLDS
};
struct DcArgs {
    const uint8_t *obs;          // the rows counted (gs_detect_census: obs == up)
    const uint8_t *up;           // the targets' truth
    const uint32_t *down_since;  // nullptr: no latency / undetected-age histograms
    uint32_t tick, tdec;         // tdec = the handle's latest tick: GS_R_FD_LAST decodes exactly against it
    uint32_t n_thr;
    float lo_all, hi_all;        // binary32 phi below lo_all: over no threshold; above hi_all: over every one
    double thr[GS_DC_MAX_THRESHOLDS];
    unsigned long long *acc;     // [DC_NUM], zeroed
    uint32_t *targets, *rows;    // optional outputs: planes 0, 1, 3 zeroed, plane 2 GS_NONE; rows zeroed
};
__device__ __forceinline__ uint32_t dc_bucket(uint32_t x) { return min(GS_DC_BUCKETS - 1u, 32u - (uint32_t)__clz(x)); }
// PHI holds 28 registers per row in flight: it is compiled for 2 workgroups per SIMD set (8 waves per CU x 2 rows x
// 112 B per lane in flight), the state-only pass for 4 as k_view_census
template <bool PHI>
__global__ __launch_bounds__(LB, PHI ? 2 : 4) void k_detect_census(Dev d, DcArgs a, uint32_t chunks) {
    constexpr uint32_t AHEAD = PHI ? 2u : 3u;  // rows in flight per thread (PHI: 112 B per row and lane)
    __shared__ uint32_t s_hist[3][GS_DC_BUCKETS];
    __shared__ uint32_t s_over[2][GS_DC_MAX_THRESHOLDS];
    __shared__ uint32_t s_rows[DC_BAND];  // up targets held dead | down targets held live << 16
    __shared__ uint32_t s_ds[16][LB];     // down_since of this thread's columns (read back by this thread only)
    __shared__ double s_thr[GS_DC_MAX_THRESHOLDS];  // read on the binary64 path only
    __shared__ uint32_t s_list[DC_BAND];  // the band's counted rows (up[o] != 0), in order: the loop runs over these
    __shared__ uint32_t s_wc[LB / WAVE];
    static_assert(DC_BAND == LB, "one thread per row of the band lists the counted rows");
    const uint32_t tid = threadIdx.x;
    const uint32_t rb = blockIdx.x / chunks, cb = blockIdx.x % chunks;
    const uint32_t j0 = (cb * LB + tid) * 16u;
    if (PHI && tid < GS_DC_MAX_THRESHOLDS) s_thr[tid] = a.thr[tid];
    const uint32_t o0 = rb * DC_BAND, nrow = min(DC_BAND, d.N - o0);
    const bool act = j0 < d.ncol;
    const uint32_t nvt = act ? min(d.ncol - j0, 16u) : 0u;  // this thread's real columns (padding is never counted)
    for (uint32_t i = tid; i < 3u * GS_DC_BUCKETS; i += LB) (&s_hist[0][0])[i] = 0u;
    for (uint32_t i = tid; i < 2u * GS_DC_MAX_THRESHOLDS; i += LB) (&s_over[0][0])[i] = 0u;
    s_rows[tid] = 0u;
    // rows of down observers are neither loaded nor reduced: every load of the loop below is unconditional, so the
    // compiler's wait for a row leaves the later rows in flight
    const bool cnt_row = tid < nrow && a.obs[o0 + tid];
    const unsigned long long cnt_b = __ballot(cnt_row);
    if ((tid & 63u) == 0u) s_wc[tid >> 6] = (uint32_t)__popcll(cnt_b);
    // the targets' truth: byte masks of the up and the down columns, four columns per word
    uint32_t upm[4] = {0u, 0u, 0u, 0u}, dnm[4] = {0u, 0u, 0u, 0u};
    uint32_t upcnt = 0, dncnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        uint32_t ds = 0u;
        if (k < nvt) {
            const uint32_t j = d.col_lo + j0 + k;
            if (a.up[j]) {
                upm[k >> 2] |= 1u << (8u * (k & 3u));
                upcnt++;
            } else {
                dnm[k >> 2] |= 1u << (8u * (k & 3u));
                dncnt++;
                if (a.down_since) ds = a.down_since[j];
            }
        }
        s_ds[k][tid] = ds;
    }
    __syncthreads();
    uint32_t nlist = 0;
    {
        uint32_t base = 0;
#pragma unroll
        for (uint32_t w = 0; w < LB / WAVE; w++) {
            if (w < (tid >> 6)) base += s_wc[w];
            nlist += s_wc[w];
        }
        if (cnt_row) s_list[base + (uint32_t)__popcll(cnt_b & ((1ull << (tid & 63u)) - 1ull))] = tid;
    }
    __syncthreads();
    nlist = __builtin_amdgcn_readfirstlane(nlist);
    const uint32_t jc = act ? j0 : 0u;  // a thread past the last column loads column 0's bytes: its masks are empty
    struct Row {
        v4u_t s;
        v4u_t l[PHI ? 2 : 1], f[PHI ? 4 : 1];
    };
    Row buf[AHEAD];
    auto row_of = [&](uint32_t i) { return o0 + (uint32_t)__builtin_amdgcn_readfirstlane(s_list[i]); };
    auto ldv = [&](uint32_t i, Row &r) {
        const size_t p0 = pix(d, row_of(i), jc);
        r.s = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.fd_state + p0));
        if constexpr (PHI) {
#pragma unroll
            for (uint32_t i = 0; i < 2u; i++)
                r.l[i] = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.fd_last + p0) + i);
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
                r.f[i] = __builtin_nontemporal_load(reinterpret_cast<const v4u_t *>(d.fd + p0) + i);
        }
    };
#pragma unroll
    for (uint32_t u = 0; u < AHEAD; u++)
        if (nlist) ldv(min(u, nlist - 1u), buf[u]);
    // per target column over the band: live / dead counts as bytes (widened to 16-bit pairs every 128 rows, as
    // k_view_census's beh), smallest and largest time of death
    uint32_t lv8[4] = {0u, 0u, 0u, 0u}, dd8[4] = {0u, 0u, 0u, 0u}, lv16[8], dd16[8], tmin[16], tmax[16];
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++) lv16[k] = dd16[k] = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) { tmin[k] = NONE; tmax[k] = 0u; }
    const uint32_t n_obs = nlist;
    uint32_t n_diag = 0, n_diag_dn = 0, t_early = 0, t_maxlat = 0, t_maxfalse = 0;
    uint32_t t_upwin = 0, t_dnwin = 0, t_upphi = 0, t_dnphi = 0, t_old = 0, t_upall = 0, t_dnall = 0;
    const uint32_t sum_mask = (1u << d.sum_bits) - 1u;
    auto row = [&](uint32_t r, const Row &rw) {
        const uint32_t o = row_of(r);
        {
            uint32_t rowc = 0;
            if (act) {
                uint32_t sw[4] = {rw.s.x, rw.s.y, rw.s.z, rw.s.w};
                const uint32_t dj = o - (d.col_lo + j0);  // the diagonal pair is not counted (wraps when o is below)
                if (dj < nvt) {
                    n_diag++;
#pragma unroll
                    for (uint32_t q = 0; q < 4u; q++)
                        if ((dj >> 2) == q) {  // (obs != up: a counted observer may itself be a down target)
                            sw[q] &= ~(0xFFu << (8u * (dj & 3u)));
                            n_diag_dn += (dnm[q] >> (8u * (dj & 3u))) & 1u;
                        }
                }
#pragma unroll
                for (uint32_t q = 0; q < 4u; q++) {
                    const uint32_t x = sw[q], vm = upm[q] | dnm[q];
                    const uint32_t lv = x & ~(x >> 1) & vm, dd = (x >> 1) & ~x & vm;
                    lv8[q] += lv;
                    dd8[q] += dd;
                    rowc += (uint32_t)__popc(dd & upm[q]) | ((uint32_t)__popc(lv & dnm[q]) << 16);
                    if (dd) {  // dead pairs, one at a time: the time of death
#pragma unroll
                        for (uint32_t i = 0; i < 4u; i++) {
                            if (!((dd >> (8u * i)) & 1u)) continue;
                            const uint32_t k = 4u * q + i;
                            const uint32_t tod = d.tod[pix(d, o, j0 + k)];
                            tmin[k] = min(tmin[k], tod);
                            tmax[k] = max(tmax[k], tod);
                            if ((upm[q] >> (8u * i)) & 1u) {  // a false suspicion: how long it has lasted
                                const uint32_t age = a.tick - tod;
                                t_maxfalse = max(t_maxfalse, age);
                                atomicAdd(&s_hist[2][dc_bucket(age)], 1u);
                            } else if (a.down_since) {
                                const uint32_t ds = s_ds[k][tid];
                                if (tod >= ds) {
                                    t_maxlat = max(t_maxlat, tod - ds);
                                    atomicAdd(&s_hist[0][dc_bucket(tod - ds)], 1u);
                                } else {
                                    t_early++;
                                }
                            }
                        }
                    }
                }
                if constexpr (PHI) {
                    const uint32_t lw[8] = {rw.l[0].x, rw.l[0].y, rw.l[0].z, rw.l[0].w, rw.l[1].x, rw.l[1].y, rw.l[1].z, rw.l[1].w};
                    const uint32_t fw[16] = {rw.f[0].x, rw.f[0].y, rw.f[0].z, rw.f[0].w, rw.f[1].x, rw.f[1].y, rw.f[1].z, rw.f[1].w,
                                             rw.f[2].x, rw.f[2].y, rw.f[2].z, rw.f[2].w, rw.f[3].x, rw.f[3].y, rw.f[3].z, rw.f[3].w};
#pragma unroll
                    for (uint32_t k = 0; k < 16u; k++) {
                        const uint32_t q = k >> 2, sh = 8u * (k & 3u);
                        const uint32_t st = (sw[q] >> sh) & 0xFFu;
                        const bool isup = (upm[q] >> sh) & 1u;
                        if (!(st & FD_WIN) || !(((upm[q] | dnm[q]) >> sh) & 1u)) continue;
                        if (isup) t_upwin++; else t_dnwin++;
                        const uint32_t sum = fw[k] & sum_mask, cnt = fw[k] >> d.sum_bits;
                        const uint32_t len = min(cnt, d.W);
                        if (!len) continue;  // phi is None
                        if (isup) t_upphi++; else t_dnphi++;
                        const uint32_t l16 = (lw[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
                        // the report's age at tick, through the handle's latest tick (exact there: fd_get); a window
                        // 2^15 ticks old or more is old, and decodes as tick - 2^15
                        uint32_t age = (a.tick - a.tdec) + ((a.tdec - l16) & 0xFFFFu);
                        if ((st & FD_OLD) || age >= FD_OLD_AGE) {
                            age = FD_OLD_AGE;
                            t_old++;
                        }
                        // phi = age (len + 5) / (sum + 5 prior), all in ticks: compared without dividing
                        const float num = (float)age * ((float)len + 5.0f), den = (float)sum + d.prior5t_f;
                        if (num < a.lo_all * den) continue;
                        if (num > a.hi_all * den) {
                            if (isup) t_upall++; else t_dnall++;
                            continue;
                        }
                        const double mean = ((double)sum * TICK_S + d.prior5) / ((double)len + 5.0);
                        const double phi = ((double)age * TICK_S) / mean;
                        for (uint32_t i = 0; i < a.n_thr; i++)
                            if (phi > s_thr[i]) atomicAdd(&s_over[isup ? 0 : 1][i], 1u);
                    }
                }
            }
            if (a.rows && __ballot(rowc != 0u)) {  // one wave reduction; one global atomic per (row, chunk, plane) below
                const uint32_t s = wave_sum32(rowc);
                if ((tid & 63u) == 0u && s) atomicAdd(&s_rows[o - o0], s);
            }
        }
        if ((r & 127u) == 127u || r + 1u == nlist) {  // byte counters hold 128 rows: widen to 16-bit pairs
#pragma unroll
            for (uint32_t q = 0; q < 4u; q++) {
                lv16[2u * q] += lv8[q] & 0x00FF00FFu;
                lv16[2u * q + 1u] += (lv8[q] >> 8) & 0x00FF00FFu;
                dd16[2u * q] += dd8[q] & 0x00FF00FFu;
                dd16[2u * q + 1u] += (dd8[q] >> 8) & 0x00FF00FFu;
                lv8[q] = dd8[q] = 0u;
            }
        }
    };
    for (uint32_t r0 = 0; r0 < nlist; r0 += AHEAD) {
#pragma unroll
        for (uint32_t u = 0; u < AHEAD; u++) {
            const uint32_t r = r0 + u;
            if (r >= nlist) break;
            const Row rw = buf[u];
            ldv(min(r + AHEAD, nlist - 1u), buf[u]);  // (past the list: the last row again, unused)
            row(r, rw);
        }
    }
    // the band's results: at most one atomic per (column, plane), zeros skipped; the totals and the undetected
    // ages (tick - down_since of the column) from the per-column counts
    uint32_t t_ul = 0, t_ud = 0, t_dl = 0, t_dd = 0, t_maxund = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16u; k++) {
        // column k = 4 q + i: counts in word 2 q + (i & 1), half i >> 1
        const uint32_t w = 2u * (k >> 2) + (k & 1u), sh = 16u * ((k >> 1) & 1u);
        const uint32_t lk = (lv16[w] >> sh) & 0xFFFFu, dk = (dd16[w] >> sh) & 0xFFFFu;
        if (k >= nvt) continue;
        if ((upm[k >> 2] >> (8u * (k & 3u))) & 1u) {
            t_ul += lk;
            t_ud += dk;
        } else {
            t_dl += lk;
            t_dd += dk;
            if (lk && a.down_since) {
                const uint32_t ds = s_ds[k][tid], age = a.tick >= ds ? a.tick - ds : 0u;
                t_maxund = max(t_maxund, age);
                atomicAdd(&s_hist[1][dc_bucket(age)], lk);
            }
        }
        if (!a.targets) continue;
        if (lk) atomicAdd(&a.targets[j0 + k], lk);
        if (dk) {
            atomicAdd(&a.targets[d.ncol + j0 + k], dk);
            atomicMin(&a.targets[2u * d.ncol + j0 + k], tmin[k]);
            atomicMax(&a.targets[3u * d.ncol + j0 + k], tmax[k]);
        }
    }
    {
        const uint32_t lane0 = (tid & 63u) == 0u;
        const uint32_t up_pairs = n_obs * upcnt - (n_diag - n_diag_dn), dn_pairs = n_obs * dncnt - n_diag_dn;
        const uint32_t v[12] = {up_pairs, t_ul, t_ud, dn_pairs, t_dl, t_dd, t_upwin, t_dnwin, t_upphi, t_dnphi, t_old, t_early};
#pragma unroll
        for (uint32_t i = 0; i < 12u; i++) {
            if (!PHI && i >= 6u && i < 11u) continue;
            const uint32_t s = wave_sum32(v[i]);
            if (lane0 && s) atomicAdd(&a.acc[DC_UP_PAIRS + i], (unsigned long long)s);
        }
        const uint32_t m[3] = {wave_max32(t_maxlat), wave_max32(t_maxund), wave_max32(t_maxfalse)};
#pragma unroll
        for (uint32_t i = 0; i < 3u; i++)
            if (lane0 && m[i]) atomicMax(&a.acc[DC_MAX + i], (unsigned long long)m[i]);
        if constexpr (PHI) {  // the pairs above every threshold
            const uint32_t su = wave_sum32(t_upall), sd = wave_sum32(t_dnall);
            if (lane0)
                for (uint32_t i = 0; i < a.n_thr; i++) {
                    if (su) atomicAdd(&s_over[0][i], su);
                    if (sd) atomicAdd(&s_over[1][i], sd);
                }
        }
    }
    if (cb == 0 && tid == 0 && n_obs) atomicAdd(&a.acc[DC_OBS], (unsigned long long)n_obs);
    __syncthreads();
    for (uint32_t i = tid; i < 3u * GS_DC_BUCKETS; i += LB) {
        const uint32_t c = (&s_hist[0][0])[i];
        if (c) atomicAdd(&a.acc[DC_HIST + i], (unsigned long long)c);
    }
    if (PHI)
        for (uint32_t i = tid; i < 2u * GS_DC_MAX_THRESHOLDS; i += LB) {
            const uint32_t c = (&s_over[0][0])[i];
            if (c) atomicAdd(&a.acc[DC_OVER + i], (unsigned long long)c);
        }
    if (a.rows)
        for (uint32_t i = tid; i < nrow; i += LB) {
            const uint32_t c = s_rows[i];
            if (c & 0xFFFFu) atomicAdd(&a.rows[o0 + i], c & 0xFFFFu);
            if (c >> 16) atomicAdd(&a.rows[d.N + o0 + i], c >> 16);
        }
}
// a target nobody holds dead has no largest time of death either (the plane was zeroed for atomicMax)
__global__ __launch_bounds__(LB) void k_detect_fix(uint32_t *targets, uint32_t ncol) {
    const uint32_t j = blockIdx.x * LB + threadIdx.x;
    if (j < ncol && !targets[ncol + j]) targets[3u * ncol + j] = NONE;
}

}  // namespace

extern "C" {

static_assert(sizeof(gs_view_totals) == 56 * 8, "gs_view_totals layout");
static_assert(sizeof(gs_probe) == 8, "gs_probe layout");

int gs_view_census(gs_handle *h, const uint8_t *up, uint32_t flags, const gs_probe *probes, uint32_t n_probes,
                   uint64_t *reach, uint32_t *owners, uint32_t *rows, gs_view_totals *out) {
    if (!h) return GS_E_INVALID;
    if (!out) return fail(h, GS_E_INVALID, "gs_view_census: out is NULL");
    if (flags & ~GS_VC_HEARTBEATS) return fail(h, GS_E_INVALID, "gs_view_census: unknown flags 0x%x", flags);
    if (n_probes > GS_VC_MAX_PROBES) return fail(h, GS_E_INVALID, "gs_view_census: %u probes (at most %u)", n_probes, GS_VC_MAX_PROBES);
    if (n_probes && (!probes || !reach)) return fail(h, GS_E_INVALID, "gs_view_census: probes without their arrays");
    for (uint32_t i = 0; i < n_probes; i++)
        if (probes[i].owner >= h->N) return fail(h, GS_E_INVALID, "gs_view_census: probe %u owner %u >= %u nodes", i, probes[i].owner, h->N);
    if (!h->booted) return fail(h, GS_E_INVALID, "gs_view_census: not booted");
    constexpr size_t WORDS = VC_NUM + GS_VC_MAX_PROBES;  // u64 accumulators, then {column, version} per probe
    if (!h->vc_buf) HIPCHK(h, hipMalloc(&h->vc_buf, WORDS * 8));
    h->vc_img.assign(WORDS, 0ull);
    for (uint32_t i = 0; i < n_probes; i++) {
        const uint32_t j = probes[i].owner;  // a probe of another slice's owner reaches nobody here
        const uint32_t c = j >= h->col_lo && j - h->col_lo < h->ncol ? j - h->col_lo : NONE;
        h->vc_img[VC_NUM + i] = (uint64_t)c | (uint64_t)probes[i].version << 32;
    }
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->vc_buf, h->vc_img.data(), WORDS * 8, hipMemcpyHostToDevice, s));
    if (owners) HIPCHK(h, hipMemsetAsync(owners, 0, (size_t)3 * h->ncol * 4, s));
    if (rows) HIPCHK(h, hipMemsetAsync(rows, 0, (size_t)h->N * 4, s));
    VcArgs a;
    a.up = up;
    a.flags = flags;
    a.n_probes = n_probes;
    a.acc = h->vc_buf;
    a.probes = reinterpret_cast<const uint32_t *>(h->vc_buf + VC_NUM);
    a.owners = owners;
    a.rows = rows;
    const Dev &d = h->d;
    const bool swar = (d.flags & GS_CANONICAL) && d.hb8 && d.mv8 && d.self_pk;
    const uint32_t per = swar ? 16u : 8u, chunks = (h->ncol + LB * per - 1) / (LB * per);
    const uint32_t grid = (h->N + VC_BAND - 1) / VC_BAND * chunks;
    if (swar)
        k_view_census<true><<<grid, LB, 0, s>>>(d, a, chunks);
    else
        k_view_census<false><<<grid, LB, 0, s>>>(d, a, chunks);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(h->vc_img.data(), h->vc_buf, (size_t)VC_NUM * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    const uint64_t *acc = h->vc_img.data();
    memset(out, 0, sizeof *out);
    out->observers = acc[VC_OBS];
    out->views = acc[VC_VIEWS];
    out->unknown = acc[VC_UNK];
    out->behind = acc[VC_BEHIND];
    out->inexact = acc[VC_INEX];
    out->max_version_lag = acc[VC_MAXV];
    out->max_heartbeat_lag = acc[VC_MAXH];
    // the kernel counts the non-zero lags: bucket 0 is the rest of the known views
    uint64_t nzv = 0, nzh = 0;
    for (uint32_t b = 1; b < GS_VC_BUCKETS; b++) {
        nzv += out->version_lag_hist[b] = acc[VC_VH + b];
        nzh += out->heartbeat_lag_hist[b] = acc[VC_HH + b];
    }
    out->version_lag_hist[0] = out->views - nzv;
    if (flags & GS_VC_HEARTBEATS) out->heartbeat_lag_hist[0] = out->views - nzh;
    for (uint32_t i = 0; i < n_probes; i++) reach[i] = acc[VC_REACH + i];
    return GS_OK;
}

static_assert(sizeof(gs_detect_totals) == 120 * 8, "gs_detect_totals layout");

extern "C++" {
namespace {
// gs_detect_census (obs == up) and gs_detect_census_for: `fn` names the entry point in gs_last_error
int detect_census(gs_handle *h, const char *fn, const uint8_t *obs, const uint8_t *up, const uint32_t *down_since,
                  uint32_t tick, const double *thresholds, uint32_t n_thresholds, uint32_t *targets, uint32_t *rows,
                  gs_detect_totals *out) {
    if (!h) return GS_E_INVALID;
    if (!obs) return fail(h, GS_E_INVALID, "%s: observers is NULL", fn);
    if (!up) return fail(h, GS_E_INVALID, "%s: up is NULL", fn);
    if (!out) return fail(h, GS_E_INVALID, "%s: out is NULL", fn);
    if (n_thresholds > GS_DC_MAX_THRESHOLDS)
        return fail(h, GS_E_INVALID, "%s: %u thresholds (at most %u)", fn, n_thresholds, GS_DC_MAX_THRESHOLDS);
    if (n_thresholds && !thresholds) return fail(h, GS_E_INVALID, "%s: thresholds is NULL", fn);
    // gs_create's bound on phi_threshold, for every swept threshold: a window silent for >= 2^15 ticks is above it
    const double widest = std::max((double)h->cfg.max_interval_ticks, h->cfg.prior_weighted / 5.0 * 64.0);
    double tmin = 0.0, tmax = 0.0;
    for (uint32_t i = 0; i < n_thresholds; i++) {
        const double x = thresholds[i];
        if (!(x >= 0.0) || !(x * widest < (double)FD_OLD_AGE))
            return fail(h, GS_E_INVALID, "%s: threshold %u = %g is NaN, negative or too large "
                        "(threshold x max(max_interval, prior) must stay below 2^15 ticks)", fn, i, x);
        tmin = i ? std::min(tmin, x) : x;
        tmax = i ? std::max(tmax, x) : x;
    }
    if ((int32_t)(tick - h->max_tick) < 0 || tick - h->max_tick >= FD_OLD_AGE)
        return fail(h, GS_E_INVALID, "%s: tick %u is before the handle's latest tick %u, or 2^15 or more "
                    "past it", fn, tick, h->max_tick);
    if (!h->booted) return fail(h, GS_E_INVALID, "%s: not booted", fn);
    if (!h->dc_buf) HIPCHK(h, hipMalloc(&h->dc_buf, (size_t)DC_NUM * 8));
    hipStream_t s = h->stream;
    HIPCHK(h, hipMemsetAsync(h->dc_buf, 0, (size_t)DC_NUM * 8, s));
    if (targets) {
        HIPCHK(h, hipMemsetAsync(targets, 0, (size_t)4 * h->ncol * 4, s));
        HIPCHK(h, hipMemsetAsync(targets + (size_t)2 * h->ncol, 0xFF, (size_t)h->ncol * 4, s));
    }
    if (rows) HIPCHK(h, hipMemsetAsync(rows, 0, (size_t)2 * h->N * 4, s));
    DcArgs a;
    a.obs = obs;
    a.up = up;
    a.down_since = down_since;
    a.tick = tick;
    a.tdec = h->max_tick;
    a.n_thr = n_thresholds;
    // binary32 phi carries a relative error below 2^-20: 2^-10 clear of every threshold decides all of them
    a.lo_all = (float)(tmin * (1.0 - 0x1p-10));
    a.hi_all = (float)(tmax * (1.0 + 0x1p-10));
    for (uint32_t i = 0; i < GS_DC_MAX_THRESHOLDS; i++) a.thr[i] = i < n_thresholds ? thresholds[i] : 0.0;
    a.acc = h->dc_buf;
    a.targets = targets;
    a.rows = rows;
    const uint32_t chunks = (h->ncol + LB * 16 - 1) / (LB * 16);
    const uint32_t grid = (h->N + DC_BAND - 1) / DC_BAND * chunks;
    if (n_thresholds)
        k_detect_census<true><<<grid, LB, 0, s>>>(h->d, a, chunks);
    else
        k_detect_census<false><<<grid, LB, 0, s>>>(h->d, a, chunks);
    HIPCHK(h, hipGetLastError());
    if (targets) {
        k_detect_fix<<<(h->ncol + LB - 1) / LB, LB, 0, s>>>(targets, h->ncol);
        HIPCHK(h, hipGetLastError());
    }
    uint64_t acc[DC_NUM];
    HIPCHK(h, hipMemcpyAsync(acc, h->dc_buf, sizeof acc, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->observers = acc[DC_OBS];
    out->up_pairs = acc[DC_UP_PAIRS];
    out->up_live = acc[DC_UP_LIVE];
    out->up_dead = acc[DC_UP_DEAD];
    out->up_unknown = out->up_pairs - out->up_live - out->up_dead;
    out->down_pairs = acc[DC_DN_PAIRS];
    out->down_live = acc[DC_DN_LIVE];
    out->down_dead = acc[DC_DN_DEAD];
    out->down_unknown = out->down_pairs - out->down_live - out->down_dead;
    out->up_windows = acc[DC_UP_WIN];
    out->down_windows = acc[DC_DN_WIN];
    out->up_phi = acc[DC_UP_PHI];
    out->down_phi = acc[DC_DN_PHI];
    out->old_windows = acc[DC_OLD];
    out->early_deaths = acc[DC_EARLY];
    out->max_detect_latency = acc[DC_MAX];
    out->max_undetected_age = acc[DC_MAX + 1];
    out->max_false_age = acc[DC_MAX + 2];
    for (uint32_t b = 0; b < GS_DC_BUCKETS; b++) {
        out->detect_latency_hist[b] = acc[DC_HIST + b];
        out->undetected_age_hist[b] = acc[DC_HIST + GS_DC_BUCKETS + b];
        out->false_age_hist[b] = acc[DC_HIST + 2 * GS_DC_BUCKETS + b];
    }
    for (uint32_t i = 0; i < n_thresholds; i++) {
        out->up_over[i] = acc[DC_OVER + i];
        out->down_over[i] = acc[DC_OVER + GS_DC_MAX_THRESHOLDS + i];
    }
    return GS_OK;
}
}  // namespace
}

int gs_detect_census(gs_handle *h, const uint8_t *up, const uint32_t *down_since, uint32_t tick, const double *thresholds,
                     uint32_t n_thresholds, uint32_t *targets, uint32_t *rows, gs_detect_totals *out) {
    if (h && !up) return fail(h, GS_E_INVALID, "gs_detect_census: up is NULL");
    return detect_census(h, "gs_detect_census", up, up, down_since, tick, thresholds, n_thresholds, targets, rows, out);
}

int gs_detect_census_for(gs_handle *h, const uint8_t *observers, const uint8_t *up, const uint32_t *down_since,
                         uint32_t tick, const double *thresholds, uint32_t n_thresholds, uint32_t *targets, uint32_t *rows,
                         gs_detect_totals *out) {
    return detect_census(h, "gs_detect_census_for", observers, up, down_since, tick, thresholds, n_thresholds, targets,
                         rows, out);
}

static_assert(sizeof(gs_age_totals) == 80 * 8, "gs_age_totals layout");

int gs_write_log_words(const gs_handle *h, uint32_t *wl) {
    if (!h || !wl) return GS_E_INVALID;
    *wl = round_up(h->K * (h->C - 1) + 1, 4);  // GS_R_VLOG's row: versions 1 .. K (C - 1)
    return GS_OK;
}

int gs_write_log_init(gs_handle *h, uint32_t *wlog) {
    if (!h) return GS_E_INVALID;
    if (!wlog) return fail(h, GS_E_INVALID, "gs_write_log_init: wlog is NULL");
    uint32_t WL = 0;
    gs_write_log_words(h, &WL);
    HIPCHK(h, hipMemsetAsync(wlog, 0xFF, (size_t)h->ncol * WL * 4, h->stream));
    return GS_OK;
}

int gs_note_writes(gs_handle *h, uint32_t tick, uint32_t *wlog) {
    if (!h) return GS_E_INVALID;
    if (!wlog) return fail(h, GS_E_INVALID, "gs_note_writes: wlog is NULL");
    if (!h->booted) return fail(h, GS_E_INVALID, "gs_note_writes: not booted");
    uint32_t WL = 0;
    gs_write_log_words(h, &WL);
    k_note_writes<<<(h->ncol + LB - 1) / LB, LB, 0, h->stream>>>(h->d, wlog, WL, tick);
    HIPCHK(h, hipGetLastError());
    return GS_OK;
}

int gs_age_census(gs_handle *h, const uint8_t *up, const uint32_t *wlog, uint32_t tick, uint32_t flags, uint32_t *floor,
                  uint32_t *rows, uint32_t *done, gs_age_totals *out) {
    if (!h) return GS_E_INVALID;
    if (!wlog) return fail(h, GS_E_INVALID, "gs_age_census: wlog is NULL");
    if (!out) return fail(h, GS_E_INVALID, "gs_age_census: out is NULL");
    if (flags) return fail(h, GS_E_INVALID, "gs_age_census: unknown flags 0x%x", flags);
    if ((int32_t)(tick - h->max_tick) < 0 || tick - h->max_tick >= FD_OLD_AGE)
        return fail(h, GS_E_INVALID, "gs_age_census: tick %u is before the handle's latest tick %u, or 2^15 or more "
                    "past it", tick, h->max_tick);
    if (!h->booted) return fail(h, GS_E_INVALID, "gs_age_census: not booted");
    const size_t bytes = (size_t)AC_NUM * 8 + (size_t)h->ncol * 4;
    if (!h->ac_buf) HIPCHK(h, hipMalloc(&h->ac_buf, bytes));
    hipStream_t s = h->stream;
    AcArgs a;
    a.up = up;
    a.wlog = wlog;
    gs_write_log_words(h, &a.WL);
    a.tick = tick;
    a.acc = h->ac_buf;
    a.floor = reinterpret_cast<uint32_t *>(h->ac_buf + AC_NUM);
    a.rows = rows;
    a.done = done;
    const Dev &d = h->d;
    HIPCHK(h, hipMemsetAsync(h->ac_buf, 0, (size_t)AC_NUM * 8, s));
    // a column's floor starts at the owner's own max_version: the value with no counted observer, or none behind
    HIPCHK(h, hipMemcpyAsync(a.floor, d.self_mv, (size_t)h->ncol * 4, hipMemcpyDeviceToDevice, s));
    if (rows) HIPCHK(h, hipMemsetAsync(rows, 0, (size_t)h->N * 4, s));
    const bool swar = (d.flags & GS_CANONICAL) && d.mv8;
    const uint32_t per = swar ? 16u : 8u, chunks = (h->ncol + LB * per - 1) / (LB * per);
    const uint32_t grid = (h->N + VC_BAND - 1) / VC_BAND * chunks;
    if (swar)
        k_age_census<true><<<grid, LB, 0, s>>>(d, a, chunks);
    else
        k_age_census<false><<<grid, LB, 0, s>>>(d, a, chunks);
    HIPCHK(h, hipGetLastError());
    k_age_owners<<<(h->ncol + LB - 1) / LB, LB, 0, s>>>(d, a);
    HIPCHK(h, hipGetLastError());
    if (floor) HIPCHK(h, hipMemcpyAsync(floor, a.floor, (size_t)h->ncol * 4, hipMemcpyDeviceToDevice, s));
    uint64_t acc[AC_NUM];
    HIPCHK(h, hipMemcpyAsync(acc, h->ac_buf, sizeof acc, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->observers = acc[AC_OBS];
    out->pairs = out->observers * h->ncol;
    out->unknown = acc[AC_UNK];
    out->behind = acc[AC_BEHIND];
    out->unlogged = acc[AC_UNLOG];
    out->max_age = acc[AC_MAXAGE];
    out->spread_writes = acc[AC_SPREAD];
    out->pending_writes = acc[AC_PENDING];
    out->unlogged_writes = acc[AC_UNLOG_W];
    out->max_spread_latency = acc[AC_MAXSPREAD];
    out->max_pending_age = acc[AC_MAXPEND];
    for (uint32_t b = 0; b < GS_AC_BUCKETS; b++) {
        out->age_hist[b] = acc[AC_AH + b];
        out->spread_hist[b] = acc[AC_SH + b];
        out->pending_age_hist[b] = acc[AC_PH + b];
    }
    return GS_OK;
}

}  // extern "C"
