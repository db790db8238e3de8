// dominance.hip — fast path of sortNondominated (deap/tools/emo.py:53-117)
// for 2..4 objectives and NaN-free fitnesses: the unique fitnesses' dominance
// relation over integer ranks, each unordered pair of 64-blocks computed once,
// and a front-peeling loop driven by the device.
//
// 1. Ranks.  Fitness.dominates (base.py:209-224) only asks, per objective,
//    whether x > y, x < y or neither; replacing every objective value by its
//    dense rank among the U unique values (-0.0 == 0.0, as Python compares)
//    preserves all three answers, so the O(M U^2) pass compares int32 ranks
//    (full-rate VALU compares) instead of fp64 values.  A NaN compares neither
//    way with anything and has no rank: populations holding one take the fp64
//    kernels of nsga2.hip.
// 2. Dominance.  Rows are ordered by objective 0 (q order), so a row can only
//    dominate the rows before it: tri_dom_kernel computes the lower triangle
//    only (section 2 below), D[a][b] one bit, with b's dominator count as
//    int16 partials per (A-group, b) summed by tri_count.  D is stored in
//    tiles of 64 rows x 16 words (tword): one 128-byte line per row and
//    1024-v segment.
// 3. Fronts.  Front 0 = count 0 in U order (nsga2.hip).  Then per front a
//    peel kernel reads the members' row lines (whole lines), transposes the
//    64 x 64-bit blocks with DPP / permlane moves (transpose.hpp) and
//    subtracts the dominator counts; a v whose count reaches zero joins the
//    next front's candidates with the key (last releasing position, U index).
//    One workgroup then orders the candidates by that key — the order the
//    reference's peel loop appends them in (emo.py:106-115, SURVEY.md
//    §8a-a21) — writes the front, its ranks and its individual count, and
//    decides termination on the device.  The host only checks a status word
//    every few fronts.
#include "bitdom.hpp"
#include "transpose.hpp"

namespace dm {

// ---------------------------------------------------------------------------
// 1. ranks in objective-0 order
// ---------------------------------------------------------------------------
// Unique fitness u gets the position q = pos[u] of its group in the
// population's lexicographic order (sigma[q] = u), so objective 0 ascends
// with q.  S[q] = int4 {rank_1, .., rank_{m-1}, rank_0, pad}: objective 0's
// dense rank is component m-1.
__global__ void lex_flags_kernel(const double* wv, int m, const int32_t* perm,
                                 const int32_t* segin, int64_t n, int32_t* fst, int32_t* f0) {
    DGRID_LOOP(j, n) {
        fst[j] = (j == 0 || segin[j] != 0) ? 1 : 0;
        f0[j] = (j == 0 || !(wv[(int64_t)perm[j] * m] == wv[(int64_t)perm[j - 1] * m])) ? 1 : 0;
    }
}
__global__ void lex_sigma_kernel(const int32_t* perm, const int32_t* uidx, const int32_t* fst,
                                 const int32_t* qex, const int32_t* f0, const int32_t* rex,
                                 int64_t n, int m, int32_t* sigma, int32_t* pos, int32_t* S) {
    DGRID_LOOP(j, n) {
        if (fst[j]) {
            const int32_t q = qex[j], u = uidx[perm[j]];
            sigma[q] = u;
            pos[u] = q;
            S[(int64_t)q * 4 + (m - 1)] = rex[j] + f0[j] - 1;
        }
    }
}
// Dense ranks of objectives 1..m-1 over the U unique fitnesses, batched:
// element j of segment g = j / U holds objective g + 1 of unique row j % U.
__global__ void rank_key_kernel(const double* ufit, int m, int64_t U, int64_t nb, uint64_t* keys,
                                int32_t* vals) {
    DGRID_LOOP(j, nb) {
        const int64_t g = j / U, u = j - g * U;
        keys[j] = ordered_key(ufit[u * m + g + 1]);
        vals[j] = (int32_t)u;
    }
}
__global__ void rank_flag_kernel(const uint64_t* keys, int64_t U, int64_t nb, int32_t* flag) {
    DGRID_LOOP(j, nb) flag[j] = (j % U != 0 && keys[j] != keys[j - 1]) ? 1 : 0;
}
// rank within the segment: the prefix count of new values since its start
__global__ void rank_scatter_kernel(const int32_t* vals, const int32_t* excl, const int32_t* flag,
                                    const int32_t* pos, int64_t U, int64_t nb, int32_t* S) {
    DGRID_LOOP(j, nb) {
        const int64_t g = j / U;
        S[(int64_t)pos[vals[j]] * 4 + g] = excl[j] + flag[j] - excl[g * U];
    }
}

// ---------------------------------------------------------------------------
// 2. dominance below the objective-0 diagonal
// ---------------------------------------------------------------------------
// a can dominate b only if rank_0(a) >= rank_0(b), i.e. (with ties aside)
// only for b before a in q order.  A wave owns an A-group of TD_WPW 64-row
// blocks (dominators a in the lanes, ranks in VGPRs) and sweeps the 64-v
// blocks B that the group's largest rank_0 can reach (v wave-uniform, ranks
// by scalar loads).  When every rank_0 of B is below every rank_0 of the
// group ("strict" block pair) objective 0 is decided, and a dominates b iff
// its other m-1 ranks are >= b's: m-1 compares whose wave masks are ANDed by
// the SALU.  Otherwise (the group's own blocks, rank_0 ties across blocks)
// the full test: min(x - y) >= 0 and max(x - y) > 0 over all m ranks.  The
// mask bit of lane a is shifted into a's word D[a][B] lane-locally
// (t = 2t + bit, one v_addc); the mask's popcount is b's dominator count
// contribution, parked in lane b%64 and stored as an int16 partial per
// (A-group, b).  Words above the reach of a group are never written (the
// peel skips them), so the matrix costs about half the bytes and compares of
// the symmetric pass and the strict inner step is m-1 compares + 1 add.
constexpr int TD_SEGS = 2;  // 8-block row segments (512 v) per task

// D layout: tword (dominance.hpp).  A wave's store of 4 words of its 64 rows
// is 64 pieces of 32 bytes that fill the tile's lines over four such stores;
// a peel read of a row segment is one whole line.

// nseg[g]: 8-block segments of v the rows of A-group g reach (every v whose
// rank_0 <= the group's largest); toff[g]: first task of g (TD_SEGS segments
// per task), toff[ngroups] = tasks.  One workgroup; nseg is nondecreasing.
// nseg[g] = the 512-v segments row group g (TD_WPW 64-row blocks) can
// reach: up to the last q whose rank_0 does not exceed the group's largest
// (rank_0 ascends with q).
__device__ __forceinline__ int32_t group_reach(const int4* S, int m, int64_t U, int64_t NG,
                                               int64_t g) {
    const int64_t last = std::min<int64_t>((g + 1) * TD_WPW * 64, U) - 1;
    const int32_t rmax = icomp(S[last], m - 1);
    int64_t lo = last, hi = U - 1;  // last q with rank_0 <= rmax
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (icomp(S[mid], m - 1) <= rmax) lo = mid;
        else hi = mid - 1;
    }
    return (int32_t)std::min<int64_t>(NG, (lo >> 9) + 1);
}
// the bitset path needs only nseg (no compare-kernel tile offsets): one
// thread per group over the whole grid instead of tri_plan_kernel's single
// workgroup (18.6 us at C5)
__global__ void group_reach_kernel(const int4* S, int m, int64_t U, int64_t NG, int64_t ngroups,
                                   int32_t* nseg) {
    DGRID_LOOP(g, ngroups) nseg[g] = group_reach(S, m, U, NG, g);
}

__global__ __launch_bounds__(1024) void tri_plan_kernel(const int4* S, int m, int64_t U,
                                                        int64_t NG, int64_t ngroups,
                                                        int32_t* nseg, int32_t* toff,
                                                        int32_t* counter) {
    __shared__ int32_t sh[1024];
    __shared__ int32_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) {
        carry = 0;
        *counter = 0;
    }
    __syncthreads();
    for (int64_t base = 0; base < ngroups; base += 1024) {
        const int64_t g = base + tid;
        int32_t nt = 0;
        if (g < ngroups) {
            const int32_t ns = group_reach(S, m, U, NG, g);
            nseg[g] = ns;
            nt = (ns + TD_SEGS - 1) / TD_SEGS;
        }
        sh[tid] = nt;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const int32_t add = tid >= off ? sh[tid - off] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        const int32_t c0 = carry;
        if (g < ngroups) toff[g] = c0 + sh[tid] - nt;
        __syncthreads();
        if (tid == 1023) carry = c0 + sh[1023];
        __syncthreads();
    }
    if (tid == 0) toff[ngroups] = carry;
}

// t + t + (bit `lane` of mask): one v_addc_co_u32 with the wave mask as the
// carry-in (lane-local "shift in the bit of this lane").
#ifndef DM_TD_ILP
#define DM_TD_ILP 1  // 0: the round-2 per-A-block order (A/B)
#endif
// Not volatile: a pure function of its operands, so the scheduler may
// interleave the independent shift-ins of the 4 A-blocks (a volatile asm kept
// them in program order, each waiting on its own compare -> s_and chain).
__device__ __forceinline__ uint32_t add2_carry(uint32_t t, uint32_t a, uint64_t mask) {
    uint32_t out;
    uint64_t cout;
#if DM_TD_ILP
    asm("v_addc_co_u32_e64 %0, %1, %2, %3, %4"
        : "=v"(out), "=s"(cout)
        : "v"(t), "v"(a), "s"(mask));
#else
    asm volatile("v_addc_co_u32_e64 %0, %1, %2, %3, %4"
                 : "=v"(out), "=s"(cout)
                 : "v"(t), "v"(a), "s"(mask));
#endif
    return out;
}

// v_writelane_b32 with an immediate lane: lane L of old <- the wave-uniform val
template <int L>
__device__ __forceinline__ int32_t writelane(int32_t old, int32_t val) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(val), "i"(L));
    return old;
}

// Dominator counts.  DM_TD_TCOUNT = 1 (default): after each 64-row block the
// group's words (lane a: bit j <-> a dominates row j of the block) are
// transposed across the wave (TransposerX, DPP / permlane moves) so that lane
// j holds the dominators of row j and counts them with v_bcnt — per block and
// A-block one transpose (~31 VALU) instead of 64 s_bcnt1 + s_add on the SALU
// and a v_writelane per row (r02: 1.16e9 SALU beside 1.36e9 VALU
// instructions per launch, profiles/r03b).  0: the per-row SALU count.
#ifndef DM_TD_TCOUNT
#define DM_TD_TCOUNT 1
#endif
// DM_TD_WQ = 1: the D words of 4 consecutive v blocks are kept and stored
// as two 16-B pieces per row; 0: one 8-B store per row and block.
#ifndef DM_TD_WQ
#define DM_TD_WQ 1
#endif
// DM_TD_SROWS = 1: the v block's ranks (wave-uniform) come by scalar loads
// into SGPRs instead of an LDS broadcast into VGPRs.
#ifndef DM_TD_SROWS
#define DM_TD_SROWS 1
#endif

// one row b (ranks y) against the group's lanes: shift the dominance bits
// into tw, return b's dominator count over the group (0 when counted by
// transposes)
template <int M, bool STRICT>
__device__ __forceinline__ int32_t td_row(const int4 y4, const int32_t (&x)[TD_WPW][M],
                                          uint32_t (&tw)[TD_WPW]) {
    int32_t y[M];
    y[0] = y4.x;
    y[1] = y4.y;
    if constexpr (M > 2) y[2] = y4.z;
    if constexpr (M > 3) y[3] = y4.w;
    int32_t cnt = 0;
    // all compares of the row first (independent wave masks), then the ANDs,
    // then the shift-ins: the VALU -> SALU -> VALU chains of the 4 A-blocks
    // overlap instead of running one after the other
    uint64_t msk[TD_WPW];
#pragma unroll
    for (int k = 0; k < TD_WPW; ++k) {
        if constexpr (STRICT) {
            msk[k] = __ballot(x[k][0] >= y[0]);
        } else {
            int32_t mn = x[k][0] - y[0], mx = mn;
#pragma unroll
            for (int o = 1; o < M; ++o) {
                const int32_t d = x[k][o] - y[o];
                mn = min(mn, d);
                mx = max(mx, d);
            }
            msk[k] = __ballot(mn >= 0) & __ballot(mx > 0);
        }
    }
    if constexpr (STRICT) {
#pragma unroll
        for (int o = 1; o < M - 1; ++o)
#pragma unroll
            for (int k = 0; k < TD_WPW; ++k) msk[k] &= __ballot(x[k][o] >= y[o]);
    }
#pragma unroll
    for (int k = 0; k < TD_WPW; ++k) {
        tw[k] = add2_carry(tw[k], tw[k], msk[k]);
#if !defined(DM_TD_NOCOUNT) && !DM_TD_TCOUNT
        cnt += __popcll(msk[k]);
#endif
    }
    return cnt;
}

// rows JTOP..JTOP-31 of a full block (descending: bit j of the word <-> row
// j); the block's ranks are in the wave's LDS buffer (broadcast reads), the
// next four rows read ahead
template <int M, bool STRICT, int JTOP, int J4 = 0>
__device__ __forceinline__ void td_half(const int4* L, const int32_t (&x)[TD_WPW][M],
                                        uint32_t (&tw)[TD_WPW], int32_t& cpark, const int4 (&cur)[4]) {
    int4 nxt[4];
    if constexpr (J4 + 4 < 32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) nxt[i] = L[JTOP - J4 - 4 - i];
    }
    if constexpr (DM_TD_TCOUNT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) (void)td_row<M, STRICT>(cur[i], x, tw);
    } else {
        cpark = writelane<JTOP - J4>(cpark, td_row<M, STRICT>(cur[0], x, tw));
        cpark = writelane<JTOP - J4 - 1>(cpark, td_row<M, STRICT>(cur[1], x, tw));
        cpark = writelane<JTOP - J4 - 2>(cpark, td_row<M, STRICT>(cur[2], x, tw));
        cpark = writelane<JTOP - J4 - 3>(cpark, td_row<M, STRICT>(cur[3], x, tw));
    }
    if constexpr (J4 + 4 < 32) td_half<M, STRICT, JTOP, J4 + 4>(L, x, tw, cpark, nxt);
}
template <int M, bool STRICT, int JTOP>
__device__ __forceinline__ void td_half(const int4* L, const int32_t (&x)[TD_WPW][M],
                                        uint32_t (&tw)[TD_WPW], int32_t& cpark) {
    int4 cur[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cur[i] = L[JTOP - i];
    td_half<M, STRICT, JTOP, 0>(L, x, tw, cpark, cur);
}

// the last, partial block (nb < 64 rows): rows past the end shift in zeros
template <int M, bool STRICT>
__device__ void td_partial_half(const int4* L, int jtop, int nb,
                                const int32_t (&x)[TD_WPW][M], uint32_t (&tw)[TD_WPW],
                                int32_t& cpark) {
    for (int j = jtop; j > jtop - 32; --j) {
        if (j >= nb) {
#pragma unroll
            for (int k = 0; k < TD_WPW; ++k) tw[k] += tw[k];
            continue;
        }
        const int32_t cnt = td_row<M, STRICT>(L[j], x, tw);
        if constexpr (!DM_TD_TCOUNT) cpark = (int)(threadIdx.x & 63) == j ? cnt : cpark;
    }
}

// Persistent: each wave takes tasks (A-group g, TD_SEGS segments of B) from
// an atomic counter until toff[ngroups] are done.
template <int M>
__global__ __launch_bounds__(256) void tri_dom_kernel(const int4* __restrict__ S, int64_t U,
                                                      int64_t NB, int64_t NQ, int64_t ngroups,
                                                      const int32_t* __restrict__ nseg,
                                                      const int32_t* __restrict__ toff,
                                                      int32_t* counter, uint64_t* __restrict__ D,
                                                      int16_t* __restrict__ part) {
#if !DM_TD_SROWS
    __shared__ int4 sbuf[4][64];  // per wave: the ranks of the current v block
    int4* Lw = sbuf[threadIdx.x >> 6];
#endif
    const int lane = threadIdx.x & 63;
    const TransposerX tr(lane);
    const int64_t Upad = NB * 64;
    const int32_t total = toff[ngroups];
    for (;;) {
        int32_t t = 0;
        if (lane == 0) t = atomicAdd(counter, 1);
        t = __builtin_amdgcn_readfirstlane(t);
        if (t >= total) break;
        int64_t lo = 0, hi = ngroups - 1;  // last g with toff[g] <= t
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (toff[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        const int64_t g = lo, c = t - toff[g];
        const int64_t A0 = g * TD_WPW;
        int32_t x[TD_WPW][M];
#pragma unroll
        for (int k = 0; k < TD_WPW; ++k) {
            const int64_t r = (A0 + k) * 64 + lane;
            const int4 xr = r < U ? S[r] : make_int4(-1, -1, -1, -1);  // past the end: no bits
            x[k][0] = xr.x;
            x[k][1] = xr.y;
            if constexpr (M > 2) x[k][2] = xr.z;
            if constexpr (M > 3) x[k][3] = xr.w;
        }
        const int32_t rmin = __builtin_amdgcn_readfirstlane(icomp(S[A0 * 64], M - 1));
        const int64_t B0 = c * TD_SEGS * 8;
        const int64_t B1 = std::min<int64_t>(std::min<int64_t>((int64_t)nseg[g], (c + 1) * TD_SEGS) * 8, NB);
#if !DM_TD_SROWS
        int4 nxt = B0 < B1 ? S[B0 * 64 + lane] : make_int4(0, 0, 0, 0);
#endif
        // words of 4 consecutive v blocks, stored together (whole 2 KB tiles)
        uint64_t wq[TD_WPW][4];
#pragma unroll
        for (int k = 0; k < TD_WPW; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) wq[k][i] = 0;
        for (int64_t B = B0; B < B1; ++B) {
            const int nb = (int)std::min<int64_t>(64, U - B * 64);
#if DM_TD_SROWS
            // the block's ranks are wave-uniform: scalar loads into SGPRs (no
            // LDS staging, no VGPRs for the rows in flight)
            const int4* L = S + B * 64;
            const bool strict = icomp(L[nb - 1], M - 1) < rmin;
#else
            int4* L = Lw;
            L[lane] = nxt;  // the previous block's reads were issued before (in-order LDS)
            if (B + 1 < B1) nxt = S[(B + 1) * 64 + lane];
            const bool strict = __builtin_amdgcn_readfirstlane(icomp(L[nb - 1], M - 1)) < rmin;
#endif
            uint32_t th[TD_WPW], tl[TD_WPW];
#pragma unroll
            for (int k = 0; k < TD_WPW; ++k) th[k] = tl[k] = 0;
            int32_t cpark = 0;
            if (nb == 64) {
                if (strict) {
                    td_half<M, true, 63>(L, x, th, cpark);
                    td_half<M, true, 31>(L, x, tl, cpark);
                } else {
                    td_half<M, false, 63>(L, x, th, cpark);
                    td_half<M, false, 31>(L, x, tl, cpark);
                }
            } else if (strict) {
                td_partial_half<M, true>(L, 63, nb, x, th, cpark);
                td_partial_half<M, true>(L, 31, nb, x, tl, cpark);
            } else {
                td_partial_half<M, false>(L, 63, nb, x, th, cpark);
                td_partial_half<M, false>(L, 31, nb, x, tl, cpark);
            }
            if constexpr (DM_TD_TCOUNT) {
                uint32_t lo[TD_WPW], hi[TD_WPW];
#pragma unroll
                for (int k = 0; k < TD_WPW; ++k) {
                    lo[k] = tl[k];
                    hi[k] = th[k];
                }
                tr.run<TD_WPW>(lo, hi);  // lane j: bit a <-> lane a dominates row j
                cpark = 0;
#pragma unroll
                for (int k = 0; k < TD_WPW; ++k) cpark += __popc(lo[k]) + __popc(hi[k]);
            }
            part[g * Upad + B * 64 + lane] = (int16_t)cpark;
#if !DM_TD_WQ
            // one 8-B word per row and block, stored at once (no VGPRs for the
            // 4-block line pieces; L2 merges the pieces of a line)
#pragma unroll
            for (int k = 0; k < TD_WPW; ++k)
                if (A0 + k < NB)
                    D[tword((A0 + k) * 64 + lane, B, NQ)] = ((uint64_t)th[k] << 32) | tl[k];
            continue;
#endif
            const int bq = (int)(B & 3);
#pragma unroll
            for (int k = 0; k < TD_WPW; ++k) {
                const uint64_t w = ((uint64_t)th[k] << 32) | tl[k];
#pragma unroll
                for (int i = 0; i < 4; ++i) wq[k][i] = bq == i ? w : wq[k][i];
            }
            if (bq == 3 || B + 1 == B1) {
#pragma unroll
                for (int k = 0; k < TD_WPW; ++k) {
                    if (A0 + k < NB) {
                        uint4* q = reinterpret_cast<uint4*>(D + tword((A0 + k) * 64 + lane, B & ~3ll, NQ));
                        const uint4 v0 = make_uint4((uint32_t)wq[k][0], (uint32_t)(wq[k][0] >> 32),
                                                    (uint32_t)wq[k][1], (uint32_t)(wq[k][1] >> 32));
                        const uint4 v1 = make_uint4((uint32_t)wq[k][2], (uint32_t)(wq[k][2] >> 32),
                                                    (uint32_t)wq[k][3], (uint32_t)(wq[k][3] >> 32));
                        // plain stores: the four 32-B pieces of a line merge in L2
                        // (nontemporal stores of the pieces measured 3x slower)
                        q[0] = v0;
                        q[1] = v1;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) wq[k][i] = 0;
                }
            }
        }
    }
}

// count[sigma[q]] (U order, front 0) = countq[q] (q order, the peel) = sum
// over the A-groups reaching q's segment of part[g][q].  The column sums are
// split over TC_CHUNKS ranges of g (grid y) so that enough loads are in
// flight (a column of segment 0 has ngroups partials): a thread sums 4
// adjacent q (one 8-byte load per g, 8 in flight) into tmp[chunk][q], and
// tri_count_sum_kernel adds the chunks.
constexpr int TC_CHUNKS = 4;
__global__ __launch_bounds__(256) void tri_count_part_kernel(const int16_t* __restrict__ part,
                                                             const int32_t* __restrict__ nseg,
                                                             int64_t U, int64_t Upad, int64_t ngroups,
                                                             int32_t* __restrict__ tmp) {
    const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (q0 >= U) return;
    const int32_t sq = (int32_t)(q0 >> 9);
    int64_t lo = 0, hi = ngroups;  // first g with nseg[g] > sq
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nseg[mid] > sq) hi = mid;
        else lo = mid + 1;
    }
    const int64_t ch = (ngroups + TC_CHUNKS - 1) / TC_CHUNKS;
    const int64_t g0 = std::max<int64_t>(lo, blockIdx.y * ch);
    const int64_t g1 = std::min<int64_t>(ngroups, (blockIdx.y + 1) * ch);
    int32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    const uint2* col = reinterpret_cast<const uint2*>(part + q0);  // Upad % 64 == 0: aligned
    const int64_t rs = Upad / 4;                                    // row stride in uint2
    auto add = [&](uint2 x) {
        c0 += (int16_t)(x.x & 0xFFFF);
        c1 += (int16_t)(x.x >> 16);
        c2 += (int16_t)(x.y & 0xFFFF);
        c3 += (int16_t)(x.y >> 16);
    };
    int64_t g = g0;
    for (; g + 8 <= g1; g += 8) {
        uint2 x[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = col[(g + i) * rs];
#pragma unroll
        for (int i = 0; i < 8; ++i) add(x[i]);
    }
    for (; g < g1; ++g) add(col[g * rs]);
    int32_t* out = tmp + blockIdx.y * U + q0;
    out[0] = c0;
    if (q0 + 1 < U) out[1] = c1;
    if (q0 + 2 < U) out[2] = c2;
    if (q0 + 3 < U) out[3] = c3;
}
__global__ void tri_count_sum_kernel(const int32_t* __restrict__ tmp, const int32_t* __restrict__ sigma,
                                     int64_t U, int32_t* __restrict__ count,
                                     int32_t* __restrict__ countq) {
    DGRID_LOOP(q, U) {
        int32_t cnt = 0;
#pragma unroll
        for (int c = 0; c < TC_CHUNKS; ++c) cnt += tmp[c * U + q];
        count[sigma[q]] = cnt;
        countq[q] = cnt;
    }
}

// ---------------------------------------------------------------------------
// 3. device-driven front peeling
// ---------------------------------------------------------------------------
struct FrontState {
    int32_t F;         // size of the current front (ulist[ustart, ustart + F))
    int32_t ustart;
    int32_t nfronts;   // fronts emitted after front 0
    int32_t done;
    int32_t overflow;  // candidates exceed the LDS sort: the host orders them
    int32_t ncand;     // candidates of the next front appended by the peel
    int64_t sorted;    // individuals in the emitted fronts
    int64_t pending;   // individuals of the released candidates (gsize sums)
    int64_t lastinds;  // individuals of the last emitted front
    int64_t N;         // min(n, k)
    int64_t U;
};

#ifndef DM_PEEL_WAVES
#define DM_PEEL_WAVES 8
#endif
constexpr int PEEL_WAVES = DM_PEEL_WAVES;  // waves of a peel workgroup (they split the front's members)
#ifndef DM_PEEL_BATCH
#define DM_PEEL_BATCH 2
#endif
constexpr int PEEL_BATCH = DM_PEEL_BATCH;  // member chunks per wave in flight
constexpr int PEEL_WORDS = TW;  // words of a row segment (one line)
// One workgroup (8 waves) owns one row segment s of D: PEEL_WORDS = 16 words,
// v in [1024 s, 1024 s + 1024) in q order, one 128-byte line of a row.  Its
// waves take interleaved 64-member chunks of the front, load each member's
// line (whole lines: the reads of a front's random rows fetch no bytes of
// other rows), transpose the 64 x 64-bit blocks, and the per-wave
// (dominators, last position) of each v are reduced in LDS.  v is written by
// this workgroup only, so countq needs no atomics; a v whose count reaches
// zero is released: its rank, its sort key (last releasing position, U index),
// its row and its individual count are recorded here, so the ordering kernel
// only sorts.  A row's reach (mrow.y) counts 512-v halves: the words of a half
// past it were never stored and read as zero.
// Slices of the front's members for segment s (grid y = K): a row reaches the
// segments up to its own, so segment s is read by about (1 - s/NS) of the
// members and the low segments carry the most work; they are split over up
// to K workgroups (at least PEEL_SLICE_MIN members each).
#ifndef DM_PEEL_SLICES
#define DM_PEEL_SLICES 4
#endif
constexpr int PEEL_SLICES = DM_PEEL_SLICES;
#ifndef DM_PEEL_SLICE_MIN
#define DM_PEEL_SLICE_MIN 1024
#endif
constexpr int64_t PEEL_SLICE_MIN = DM_PEEL_SLICE_MIN;
// the table peel's slices hold at least 2,048 members: its workgroups repeat
// the chunk's table loads and release per slice, and C5 measured 3.58 ms/gen
// with 2,048-8,192 against 3.69 with 1,024 (profiles/r03y)
#ifndef DM_PEEL_TAB_SLICE_MIN
#define DM_PEEL_TAB_SLICE_MIN 2048
#endif
__device__ __forceinline__ int64_t peel_slices(int64_t F, int64_t s, int64_t NS, int64_t K,
                                               int64_t smin = PEEL_SLICE_MIN) {
    const int64_t byload = (K * (NS - s) + NS - 1) / NS;
    return std::max<int64_t>(1, std::min<int64_t>(byload, F / smin));
}
// Data one phase of the persistent peel hands to another crosses workgroups
// on different XCDs, whose L2s are not coherent with each other: those
// accesses are agent-scope relaxed loads / stores (sc1, served coherently)
// when COH; plain otherwise (separate launches: the kernel boundary makes
// them visible).
template <bool COH, typename T>
__device__ __forceinline__ T cld(const T* p) {
    if constexpr (COH)
        return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        return *p;
}
template <bool COH, typename T>
__device__ __forceinline__ void cst(T* p, T v) {
    if constexpr (COH)
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}
template <bool COH>
__device__ __forceinline__ int2 cld2(const int2* p) {
    if constexpr (COH) {
        const unsigned long long x = __hip_atomic_load(
            reinterpret_cast<unsigned long long*>(const_cast<int2*>(p)), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT);
        return make_int2((int32_t)(uint32_t)x, (int32_t)(uint32_t)(x >> 32));
    } else {
        return *p;
    }
}
template <bool COH>
__device__ __forceinline__ void cst2(int2* p, int2 v) {
    if constexpr (COH)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(p),
                           (unsigned long long)(uint32_t)v.x | ((unsigned long long)(uint32_t)v.y << 32),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
        *p = v;
}

constexpr int PEEL_PV = PEEL_WORDS * 64;                 // v of a row segment
constexpr int PEEL_IT = PEEL_PV / (PEEL_WAVES * 64);      // v per thread
template <int PV>
struct PeelLdsT {
    int32_t sdec[PEEL_WAVES][PV];
    int32_t slast[PEEL_WAVES][PV];
};
template <int PV>
struct PeelSmallT {
    static constexpr int IT = PV / (PEEL_WAVES * 64);
    int32_t wcnt[IT][PEEL_WAVES];
    int64_t wgs[IT][PEEL_WAVES];
    int32_t sbase;
};
typedef PeelLdsT<PEEL_PV> PeelLds;
typedef PeelSmallT<PEEL_PV> PeelSmall;

// Per-v values a peel kernel may load in its prologue, long before the
// release needs them (the release's chain countq -> sigma -> gsize is then
// three dependent loads shorter): the count, the U index and the individual
// count of each v of the thread.
template <int IT>
struct PeelPre {
    int32_t cnt[IT], vu[IT], gs[IT];
};
template <bool COH, int PW>
__device__ void peel_release(const int32_t (&dec)[PW], const int32_t (&last)[PW], int64_t vbase,
                             const int32_t* __restrict__ gsize, const int32_t* __restrict__ sigma,
                             FrontState* st, int32_t* countq, unsigned long long* lastq,
                             uint64_t* ckey, int32_t* cq, int32_t* rankU, int64_t U, int32_t snf,
                             int64_t nsl, PeelLdsT<PW * 64>& L, PeelSmallT<PW * 64>& S,
                             const PeelPre<PeelSmallT<PW * 64>::IT>* pre = nullptr);

// Slice y of the nsl slices of row segment s for the front of sF unique
// fitnesses starting at sust in ulist / mrow (front number snf).
template <bool COH>
__device__ void peel_segment(const uint64_t* __restrict__ D, int64_t NQ, const int2* mrow,
                             const int32_t* __restrict__ gsize, const int32_t* __restrict__ sigma,
                             FrontState* st, int32_t* countq, unsigned long long* lastq,
                             uint64_t* ckey, int32_t* cq, int32_t* rankU, int64_t U, int32_t sF,
                             int32_t sust, int32_t snf, int64_t s, int64_t y, int64_t nsl,
                             PeelLds& L, PeelSmall& S) {
    constexpr int PW = PEEL_WORDS, PV = PEEL_PV;
    // members of this workgroup's slice [j0s, F)
    const int64_t slen = ((sF + nsl - 1) / nsl + 63) & ~63ll;
    const int64_t j0s = y * slen;
    const int64_t F = std::min<int64_t>(sF, j0s + slen);
    const int2* members = mrow + sust;  // (row in q order, 512-v halves it reaches)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TransposerX tr(lane);
    int32_t dec[PW], last[PW];
#pragma unroll
    for (int w = 0; w < PW; ++w) {
        dec[w] = 0;
        last[w] = -1;
    }
    constexpr int64_t STEP = PEEL_WAVES * 64;
    // member rows of the next batch are loaded one batch ahead
    int2 mr[PEEL_BATCH];
#pragma unroll
    for (int b = 0; b < PEEL_BATCH; ++b) {
        const int64_t j = j0s + (int64_t)wave * 64 + b * STEP + lane;
        mr[b] = j < F ? cld2<COH>(members + j) : make_int2(0, 0);
    }
    for (int64_t jb = j0s + (int64_t)wave * 64; jb < F; jb += STEP * PEEL_BATCH) {
        uint4 seg[PEEL_BATCH][PW / 2];
        bool has[PEEL_BATCH][2];
#pragma unroll
        for (int b = 0; b < PEEL_BATCH; ++b) {
            const uint4* q = reinterpret_cast<const uint4*>(D + tword(mr[b].x, s * PW, NQ));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                has[b][h] = 2 * s + h < mr[b].y;
#pragma unroll
                for (int i = 0; i < PW / 4; ++i)
                    seg[b][h * (PW / 4) + i] = has[b][h] ? q[h * (PW / 4) + i] : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int b = 0; b < PEEL_BATCH; ++b) {
            const int64_t j = jb + (PEEL_BATCH + b) * STEP + lane;
            mr[b] = j < F ? cld2<COH>(members + j) : make_int2(0, 0);
        }
#pragma unroll
        for (int b = 0; b < PEEL_BATCH; ++b) {
            const int64_t j0 = jb + b * STEP;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (__ballot(has[b][h]) == 0) continue;  // no member of the chunk reaches the half
                uint32_t lo[8], hi[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint4 x = seg[b][h * 4 + i];
                    lo[2 * i] = x.x;
                    hi[2 * i] = x.y;
                    lo[2 * i + 1] = x.z;
                    hi[2 * i + 1] = x.w;
                }
                tr.run<8>(lo, hi);  // lane v: bit i <-> member j0+i dominates v
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    dec[h * 8 + w] += __popc(lo[w]) + __popc(hi[w]);
                    const int32_t top = hi[w] ? 63 - __clz(hi[w]) : (lo[w] ? 31 - __clz(lo[w]) : -1);
                    if (top >= 0) last[h * 8 + w] = (int32_t)(j0 + top);
                }
            }
        }
    }
    peel_release<COH, PW>(dec, last, s * PV, gsize, sigma, st, countq, lastq, ckey, cq, rankU, U,
                          snf, nsl, L, S);
}

// The workgroup's (dominators, last releasing position) per v of its segment
// [vbase, vbase + 64 PW) (dec / last: word w of this thread = v 64 w + lane,
// per wave) are reduced in LDS and applied to countq; a v whose count reaches
// zero is released into the next front's candidates.
template <bool COH, int PW>
__device__ void peel_release(const int32_t (&dec)[PW], const int32_t (&last)[PW], int64_t vbase,
                             const int32_t* __restrict__ gsize, const int32_t* __restrict__ sigma,
                             FrontState* st, int32_t* countq, unsigned long long* lastq,
                             uint64_t* ckey, int32_t* cq, int32_t* rankU, int64_t U, int32_t snf,
                             int64_t nsl, PeelLdsT<PW * 64>& L, PeelSmallT<PW * 64>& S,
                             const PeelPre<PeelSmallT<PW * 64>::IT>* pre) {
    constexpr int PEEL_IT = PeelSmallT<PW * 64>::IT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < PW; ++w) {
        L.sdec[wave][w * 64 + lane] = dec[w];
        L.slast[wave][w * 64 + lane] = last[w];
    }
    __syncthreads();
    // release: one atomic per workgroup on the shared counters (a
    // same-address atomic per wave serialised ~6 ns each over thousands of
    // waves on the large fronts)
    bool fresh[PEEL_IT];
    int32_t lk[PEEL_IT], vu[PEEL_IT];
    unsigned long long fm[PEEL_IT];
#pragma unroll
    for (int it = 0; it < PEEL_IT; ++it) {
        const int t = threadIdx.x + it * PEEL_WAVES * 64;
        int32_t d = 0, l = -1;
#pragma unroll
        for (int wv = 0; wv < PEEL_WAVES; ++wv) {
            d += L.sdec[wv][t];
            l = max(l, L.slast[wv][t]);
        }
        const int64_t v = vbase + t;  // q order
        fresh[it] = false;
        if (v < U && d > 0) {
            if (nsl == 1) {
                const int32_t left = (pre ? pre->cnt[it] : cld<COH>(countq + v)) - d;
                cst<COH>(countq + v, left);
                fresh[it] = left == 0;
            } else {
                // several slices: publish the last position, then subtract;
                // the subtraction that reaches zero is ordered after every
                // slice's max (each waits for its max before subtracting)
                const unsigned long long key = ((unsigned long long)(snf + 1) << 32) | (uint32_t)l;
                __hip_atomic_fetch_max(lastq + v, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int32_t old = __hip_atomic_fetch_add(countq + v, -d, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (old == d) {
                    fresh[it] = true;
                    l = (int32_t)(uint32_t)__hip_atomic_fetch_max(lastq + v, key, __ATOMIC_RELAXED,
                                                                  __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        lk[it] = l;
        vu[it] = fresh[it] ? (pre ? pre->vu[it] : sigma[v]) : 0;
        fm[it] = __ballot(fresh[it]);
        int64_t gs = fresh[it] ? (pre ? pre->gs[it] : gsize[vu[it]]) : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) gs += __shfl_xor(gs, o, 64);
        if (lane == 0) {
            S.wcnt[it][wave] = __popcll(fm[it]);
            S.wgs[it][wave] = gs;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t tot = 0;
        int64_t gtot = 0;
        for (int it = 0; it < PEEL_IT; ++it)
            for (int wv = 0; wv < PEEL_WAVES; ++wv) {
                const int32_t c = S.wcnt[it][wv];
                S.wcnt[it][wv] = tot;
                tot += c;
                gtot += S.wgs[it][wv];
            }
        S.sbase = tot ? atomicAdd(&st->ncand, tot) : 0;
        if (gtot) atomicAdd((unsigned long long*)&st->pending, (unsigned long long)gtot);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < PEEL_IT; ++it) {
        if (!fresh[it]) continue;
        const int64_t v = vbase + threadIdx.x + it * PEEL_WAVES * 64;
        const int32_t slot = S.sbase + S.wcnt[it][wave] + __popcll(fm[it] & ((1ull << lane) - 1));
        cst<COH>(ckey + slot, ((uint64_t)(uint32_t)lk[it] << 32) | (uint32_t)vu[it]);
        cst<COH>(cq + slot, (int32_t)v);
        cst<COH>(rankU + vu[it], snf + 1);
    }
    __syncthreads();  // the LDS is reused by the caller's next task
}

#ifndef DM_PEEL_MINW
#define DM_PEEL_MINW 1  // min waves per SIMD (4: two 512-thread workgroups per CU)
#endif
__global__ __launch_bounds__(PEEL_WAVES * 64, DM_PEEL_MINW) void peel_owned_kernel(const uint64_t* __restrict__ D,
                                                         int64_t NQ,
                                                         const int2* __restrict__ mrow,
                                                         const int32_t* __restrict__ gsize,
                                                         const int32_t* __restrict__ sigma,
                                                         FrontState* st, int32_t* countq,
                                                         unsigned long long* lastq,
                                                         uint64_t* ckey, int32_t* cq,
                                                         int32_t* rankU) {
    __shared__ PeelLds L;
    __shared__ PeelSmall S;
    __shared__ int32_t sF, sust, sstop, snf;
    if (threadIdx.x == 0) {
        sF = st->F;
        sust = st->ustart;
        snf = st->nfronts;
        sstop = st->done | st->overflow;
    }
    __syncthreads();
    if (sstop) return;
    const int64_t s = blockIdx.x;
    const int64_t nsl = peel_slices(sF, s, gridDim.x, gridDim.y);
    if ((int64_t)blockIdx.y >= nsl) return;
    peel_segment<false>(D, NQ, mrow, gsize, sigma, st, countq, lastq, ckey, cq, rankU, st->U, sF,
                        sust, snf, s, blockIdx.y, nsl, L, S);
}

// Table-fed peel (the default with the bitset pass, 2-3 objectives): one
// workgroup per 512-v chunk c of the q order and member slice, as
// peel_owned_kernel, but each member's row bits over c are computed from the
// chunk's bitset tables (bd_row_words: a binary search of the chunk's sorted
// ranks in LDS and one 64-byte prefix-set read from the global table per
// objective; a workgroup reads only the sets its members need, mostly from
// L2) instead of read from a stored D, so the dominance matrix is never
// written.  Member rows, their ranks and tie spans
// are loaded two 64-member steps ahead (a row's ranks wait on its row index).
#ifndef DM_PEEL_TAB_MINW
#define DM_PEEL_TAB_MINW 4  // min waves per SIMD (4: two 512-thread workgroups per CU)
#endif
#ifdef DM_PEEL_PROF
// phase clocks of each table-peel workgroup (diagnostic builds only):
// {chunk, slice, F, t_start, t_tables, t_members, t_release, 0}
__device__ unsigned long long g_pprof[1 << 20];
__device__ unsigned int g_pprof_n;
#define PPROF_T(x) const unsigned long long x = wall_clock64()
#else
#define PPROF_T(x)
#endif
template <int F>
__global__ __launch_bounds__(PEEL_WAVES * 64, DM_PEEL_TAB_MINW) void peel_tab_kernel(
    const int4* __restrict__ S, const int2* __restrict__ span, const uint32_t* __restrict__ P,
    const int32_t* __restrict__ R, const uint16_t* __restrict__ BK, const int2* __restrict__ mrow,
    const int32_t* __restrict__ gsize,
    const int32_t* __restrict__ sigma, FrontState* st, int32_t* countq, unsigned long long* lastq,
    uint64_t* ckey, int32_t* cq, int32_t* rankU) {
    static_assert(PEEL_WAVES * 64 == BD_CW, "one thread per v of the chunk (sorted ranks, release)");
    constexpr int PW = BD_CW / 64;  // words of a chunk
    __shared__ int32_t sR[F][BD_RP];
    __shared__ uint16_t sB[F][BD_BKN];
    __shared__ PeelLdsT<BD_CW> L;
    __shared__ PeelSmallT<BD_CW> Sm;
    __shared__ int32_t sF, sust, sstop, snf;
    __shared__ int64_t sU;
    // grid x = NG rounded up to a multiple of 8: the slices y of chunk c (linear
    // workgroup ids c + y gridDim.x) land on one XCD, whose L2 then serves
    // the chunk's table slice to all of them
    PPROF_T(pt0);
    const int64_t c = blockIdx.x;
    const int64_t NG = (st->U + BD_CW - 1) / BD_CW;
    if (c >= NG) return;
    // loads that do not depend on the front go out first: the chunk's sorted
    // ranks, and this thread's v (count, U index, individual count)
    const int32_t* gR = R + c * F * BD_CW;
    int32_t rr[F];
#pragma unroll
    for (int f = 0; f < F; ++f) rr[f] = gR[f * BD_CW + threadIdx.x];
    if (threadIdx.x == 0) {
        sF = st->F;
        sust = st->ustart;
        snf = st->nfronts;
        sstop = st->done | st->overflow;
        sU = st->U;
    }
    __syncthreads();
    if (sstop) return;
    const int64_t nsl = peel_slices(sF, c, NG, gridDim.y, DM_PEEL_TAB_SLICE_MIN);
    if ((int64_t)blockIdx.y >= nsl) return;
    const int64_t U = sU;
    PeelPre<1> pre;
    {
        const int64_t v = c * BD_CW + threadIdx.x;
        pre.cnt[0] = v < U ? countq[v] : 0;
        pre.vu[0] = v < U ? sigma[v] : 0;
        pre.gs[0] = v < U ? gsize[pre.vu[0]] : 0;
    }
    const int64_t slen = ((sF + nsl - 1) / nsl + 63) & ~63ll;
    const int64_t j0s = blockIdx.y * slen;
    const int64_t Fm = std::min<int64_t>(sF, j0s + slen);
    const int2* members = mrow + sust;  // (row in q order, 512-v halves it reaches)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int STEP = PEEL_WAVES * 64;
    constexpr int WIN = 2048;       // 4 members per thread (8 spilled, and so did
                                    // loading the first window in the prologue)
    constexpr int WR = WIN / STEP;  // members per thread per window
    static_assert(WIN * sizeof(int2) <= sizeof(PeelLdsT<BD_CW>), "window list in the release's LDS");
#pragma unroll
    for (int f = 0; f < F; ++f) sR[f][bd_rpad(threadIdx.x)] = rr[f];
    bd_load_buckets<F>(BK, c, sB);
    const int sh = bd_bucket_shift(U);
    const BdGlobalSets sets{reinterpret_cast<const uint4*>(P + c * F * BD_K * 16)};
    const TransposerX tr(lane);
    int32_t dec[PW], last[PW];
#pragma unroll
    for (int w = 0; w < PW; ++w) {
        dec[w] = 0;
        last[w] = -1;
    }
    const int64_t v0 = c * BD_CW;
    // The slice is taken in windows of WIN members.  A window's members whose
    // row reaches chunk c are compacted, in front order, into LDS as (row,
    // front position) -- the release's LDS, not yet in use -- and processed
    // 64 at a time, so no group carries members that do not reach the chunk
    // (a front's members reach chunks up to their objective-0 position: in
    // front order about half of a group's lanes were idle on the high
    // chunks).  Positions rise within a group, so the top set bit of a
    // transposed word is its last dominator, read back by a lane shuffle.
    int2* sM = reinterpret_cast<int2*>(&L);
    PPROF_T(pt1);
    for (int64_t wb = j0s; wb < Fm; wb += WIN) {
        uint64_t bal[WR];
        int2 mr[WR];
        int nw = 0;
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            const int64_t j = wb + (int64_t)(wave * WR + r) * 64 + lane;
            mr[r] = j < Fm ? members[j] : make_int2(0, 0);
            bal[r] = __ballot(j < Fm && c < mr[r].y);
            nw += __popcll(bal[r]);
        }
        if (lane == 0) Sm.wcnt[0][wave] = nw;
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PEEL_WAVES; ++w) {
            const int x = Sm.wcnt[0][w];
            base += w < wave ? x : 0;
            total += x;
        }
        const uint64_t below = (1ull << lane) - 1;
#pragma unroll
        for (int r = 0; r < WR; ++r) {
            if ((bal[r] >> lane) & 1)
                sM[base + __popcll(bal[r] & below)] =
                    make_int2(mr[r].x, (int32_t)(wb - j0s + (int64_t)(wave * WR + r) * 64 + lane));
            base += __popcll(bal[r]);
        }
        __syncthreads();
        auto mget = [&](int g) { return g < total ? sM[g] : make_int2(0, -1); };
        int2 mA = mget(wave * 64 + lane);
        int4 suA = S[mA.x];
        int2 spA = span[mA.x];
        for (int g0 = wave * 64; g0 < total; g0 += STEP) {
            const int2 mB = mget(g0 + STEP + lane);
            const int4 suB = S[mB.x];
            const int2 spB = span[mB.x];
            const bool has = mA.y >= 0;
            const int32_t lim = (int32_t)std::max<int64_t>(-1, std::min<int64_t>((int64_t)spA.y - v0, BD_CW));
            int k[F];
            if (has && lim >= 0) {
                bd_row_k<F>(suA, sR, sB, sh, k);
            } else {
#pragma unroll
                for (int f = 0; f < F; ++f) k[f] = 0;
            }
            uint4 raw[F][4], w[4];
            bd_row_fetch<F>(sets, k, raw);
            bd_row_merge<F, false>(raw, lim, -1, w);
            uint32_t lo[8], hi[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo[2 * i] = w[i].x;
                hi[2 * i] = w[i].y;
                lo[2 * i + 1] = w[i].z;
                hi[2 * i + 1] = w[i].w;
            }
            tr.run<8>(lo, hi);  // lane v: bit i <-> group member i dominates v
            const int32_t posA = (int32_t)(j0s + mA.y);
#pragma unroll
            for (int w2 = 0; w2 < 8; ++w2) {
                dec[w2] += __popc(lo[w2]) + __popc(hi[w2]);
                const int32_t top = hi[w2] ? 63 - __clz(hi[w2]) : (lo[w2] ? 31 - __clz(lo[w2]) : 0);
                const int32_t pt = __shfl(posA, top);
                if (lo[w2] | hi[w2]) last[w2] = pt;
            }
            mA = mB;
            suA = suB;
            spA = spB;
        }
        __syncthreads();  // the window's list is read out before the next (or the release) reuses it
    }
    PPROF_T(pt2);
    peel_release<false, PW>(dec, last, v0, gsize, sigma, st, countq, lastq, ckey, cq, rankU, U,
                            snf, nsl, L, Sm, &pre);
#ifdef DM_PEEL_PROF
    PPROF_T(pt3);
    if (threadIdx.x == 0) {
        const unsigned int e = atomicAdd(&g_pprof_n, 1u);
        if (e < (1u << 17)) {
            unsigned long long* o = g_pprof + (size_t)e * 8;
            o[0] = c; o[1] = blockIdx.y; o[2] = sF; o[3] = pt0; o[4] = pt1; o[5] = pt2; o[6] = pt3; o[7] = 0;
        }
    }
#endif
}

constexpr int ORDER_CAP = 16384;  // candidates sorted in registers + LDS by one workgroup

// member i of a front: (its row in q order, the row segments it reaches)
__device__ __forceinline__ int2 member_row(int32_t u, const int32_t* pos, const int32_t* nseg) {
    const int32_t r = pos[u];
    return make_int2(r, nseg[r / (64 * TD_WPW)]);
}

template <int NT, int E, bool COH>
__device__ void order_sorted(const uint64_t* ckey, int32_t n, int32_t* out, int2* mout,
                             const int32_t* pos, const int32_t* nseg, uint64_t* lds) {
    uint64_t k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = threadIdx.x * E + e;
        k[e] = i < n ? cld<COH>(ckey + i) : ~0ull;
    }
    block_bitonic<NT, E>(k, lds);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = threadIdx.x * E + e;
        if (i < n) {
            const int32_t u = (int32_t)(uint32_t)k[e];
            cst<COH>(out + i, u);
            cst2<COH>(mout + i, member_row(u, pos, nseg));
        }
    }
}

template <int CAP>
union OrderLds {
    uint64_t keys[CAP];
    struct {
        int32_t base[CAP + 1];
        int32_t tmp[CAP];
    } cs;
};
struct OrderScalars {
    int32_t sn, sgo, snstart, sF, smax;
};

// Orders the released candidates by (last releasing position l, U index) and
// appends them to ulist / mrow as the next front, then updates the state
// (one workgroup of NT threads).  Counting sort: l < F (the current front's
// size), so the candidates are binned by l in LDS and ranked inside their bin
// by U index; a bin of more than ORDER_BIN_MAX candidates (or too many
// candidates) takes the bitonic sort of the whole key.  More than CAP
// candidates: overflow, the host's radix sort orders them (presorted: ckey
// already ordered).
constexpr int ORDER_BIN_MAX = 64;
// Exclusive prefix sum over the workgroup's threads: lane shuffles within
// each wave, one wave scans the wave totals (two barriers; a Hillis-Steele
// scan over 1,024 LDS slots took 20).  sh: NT / 64 ints of LDS.
template <int NT>
__device__ __forceinline__ int32_t block_excl_scan(int32_t v, int32_t* sh) {
    static_assert(NT % 64 == 0 && NT / 64 <= 64, "whole waves, at most 64");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int32_t w = lane < NT / 64 ? sh[lane] : 0;
#pragma unroll
        for (int o = 1; o < NT / 64; o <<= 1) {
            const int32_t y = __shfl_up(w, o, 64);
            if (lane >= o) w += y;
        }
        if (lane < NT / 64) sh[lane] = w;
    }
    __syncthreads();
    return x - v + (wave ? sh[wave - 1] : 0);
}

template <int NT, int CAP, bool COH>
__device__ void order_front(FrontState* st, const uint64_t* ckey, const int32_t* cq,
                            int32_t* ulist, int2* mrow, const int32_t* pos, const int32_t* nseg,
                            int32_t* fstarts, int presorted, OrderLds<CAP>& lds, int32_t* part,
                            OrderScalars& sc) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        const int32_t done = cld<COH>(&st->done), ovf = cld<COH>(&st->overflow);
        sc.sgo = !(done || (ovf && !presorted));
        sc.sn = cld<COH>(&st->ncand);
        sc.snstart = cld<COH>(&st->ustart) + cld<COH>(&st->F);
        sc.sF = cld<COH>(&st->F);
        sc.smax = 0;
    }
    __syncthreads();
    if (!sc.sgo) return;
    const int32_t n = sc.sn;
    if (n == 0) {  // nothing released: the reference's `if F2 == 0: break`
        if (tid == 0) cst<COH>(&st->done, 1);
        return;
    }
    if (!presorted && n > CAP) {
        if (tid == 0) cst<COH>(&st->overflow, 1);
        return;
    }
    int32_t* out = ulist + sc.snstart;
    int2* mout = mrow + sc.snstart;
    bool sorted_here = false;
    if (presorted) {
        for (int i = tid; i < n; i += NT) {
            const int32_t u = (int32_t)(uint32_t)cld<COH>(ckey + i);
            cst<COH>(out + i, u);
            cst2<COH>(mout + i, member_row(u, pos, nseg));
        }
        sorted_here = true;
    } else if (sc.sF <= CAP) {
        constexpr int E = CAP / NT;
        const int32_t Fr = sc.sF;
        for (int i = tid; i <= Fr; i += NT) lds.cs.base[i] = 0;
        __syncthreads();
        uint64_t key[E];
        int32_t qv[E], slot[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = tid + e * NT;
            if (i < n) {
                key[e] = cld<COH>(ckey + i);
                qv[e] = cld<COH>(cq + i);
                slot[e] = atomicAdd(&lds.cs.base[(int32_t)(key[e] >> 32)], 1);
            }
        }
        __syncthreads();
        // exclusive prefix of the bin counts: thread t owns C consecutive bins
        const int C = (Fr + NT - 1) / NT;
        const int b0 = tid * C, b1 = min(Fr, b0 + C);
        int32_t sum = 0, mx = 0;
        for (int b = b0; b < b1; ++b) {
            const int32_t c = lds.cs.base[b];
            sum += c;
            mx = max(mx, c);
        }
        if (mx > ORDER_BIN_MAX) atomicMax(&sc.smax, mx);
        int32_t run = block_excl_scan<NT>(sum, part);
        for (int b = b0; b < b1; ++b) {
            const int32_t c = lds.cs.base[b];
            lds.cs.base[b] = run;
            run += c;
        }
        if (tid == 0) lds.cs.base[Fr] = n;
        __syncthreads();
        if (sc.smax == 0) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = tid + e * NT;
                if (i < n) lds.cs.tmp[lds.cs.base[(int32_t)(key[e] >> 32)] + slot[e]] = (int32_t)(uint32_t)key[e];
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int i = tid + e * NT;
                if (i < n) {
                    const int32_t l = (int32_t)(key[e] >> 32), vu = (int32_t)(uint32_t)key[e];
                    const int32_t beg = lds.cs.base[l], end = lds.cs.base[l + 1];
                    int32_t r = beg;
                    for (int32_t j = beg; j < end; ++j) r += lds.cs.tmp[j] < vu ? 1 : 0;
                    cst<COH>(out + r, vu);
                    cst2<COH>(mout + r, make_int2(qv[e], nseg[qv[e] / (64 * TD_WPW)]));
                }
            }
            sorted_here = true;
        }
        __syncthreads();  // the bitonic fallback reuses the LDS
    }
    if (!sorted_here) {
        uint64_t* keys = lds.keys;
        if (n <= NT) {
            order_sorted<NT, 1, COH>(ckey, n, out, mout, pos, nseg, keys);
        } else if (n <= 2 * NT) {
            order_sorted<NT, 2, COH>(ckey, n, out, mout, pos, nseg, keys);
        } else if (n <= 4 * NT) {
            order_sorted<NT, 4, COH>(ckey, n, out, mout, pos, nseg, keys);
        } else if (n <= 8 * NT) {
            order_sorted<NT, 8, COH>(ckey, n, out, mout, pos, nseg, keys);
        } else {
            static_assert(CAP <= 16 * NT, "order capacity exceeds the bitonic sizes");
            order_sorted<NT, 16, COH>(ckey, n, out, mout, pos, nseg, keys);
        }
    }
    if (tid == 0) {
        const int32_t nstart = sc.snstart, r = cld<COH>(&st->nfronts);
        const int64_t pending = (int64_t)__hip_atomic_load(
            reinterpret_cast<unsigned long long*>(&st->pending), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT);
        const int64_t sorted = cld<COH>(&st->sorted) + pending;
        cst<COH>(&st->sorted, sorted);
        cst<COH>(&st->lastinds, pending);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(&st->pending), 0ull,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cst<COH>(&st->ustart, nstart);
        cst<COH>(&st->F, n);
        cst<COH>(&st->nfronts, r + 1);
        __hip_atomic_store(&st->ncand, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cst<COH>(&st->overflow, 0);
        cst<COH>(fstarts + r + 2, nstart + n);
        // emo.py:109: continue while pareto_sorted < N (and fronts remain)
        if (sorted >= cld<COH>(&st->N) || nstart + n >= cld<COH>(&st->U)) cst<COH>(&st->done, 1);
    }
}

__global__ __launch_bounds__(1024) void front_order_kernel(FrontState* st, const uint64_t* ckey,
                                                           const int32_t* cq, int32_t* ulist,
                                                           int2* mrow, const int32_t* pos,
                                                           const int32_t* nseg, int32_t* fstarts,
                                                           int presorted) {
    __shared__ OrderLds<ORDER_CAP> lds;
    __shared__ int32_t part[1024];
    __shared__ OrderScalars sc;
    order_front<1024, ORDER_CAP, false>(st, ckey, cq, ulist, mrow, pos, nseg, fstarts, presorted,
                                        lds, part, sc);
}

__global__ void member_rows_kernel(const int32_t* ulist, const int32_t* Fp, const int32_t* pos,
                                   const int32_t* nseg, int2* mrow) {
    const int64_t F = *Fp;
    DGRID_LOOP(j, F) mrow[j] = member_row(ulist[j], pos, nseg);
}

__global__ void front_init_kernel(FrontState* st, const int32_t* F0p, const int64_t* sorted0p,
                                  int64_t N, int64_t U, int32_t* fstarts) {
    const int32_t F0 = *F0p;
    const int64_t sorted0 = *sorted0p;
    st->F = F0;
    st->ustart = 0;
    st->nfronts = 0;
    st->done = (sorted0 >= N || F0 >= U || F0 == 0) ? 1 : 0;
    st->overflow = 0;
    st->ncand = 0;
    st->sorted = sorted0;
    st->lastinds = sorted0;
    st->pending = 0;
    st->N = N;
    st->U = U;
    fstarts[0] = 0;
    fstarts[1] = F0;
}

// ---------------------------------------------------------------------------
// host drivers (called from nsga2.hip)
// ---------------------------------------------------------------------------
// Workspace of the fast path: the buffers that live from the ranks to the
// last front, then the scratch shared by the rank sorts and the peel loop.
struct FastLayout {
    int64_t NB, NG, NQ, ngroups, Upad;  // NG: 512-v segments (tri_dom), NQ: TW-word lines (peel)
    size_t part, S, sigma, pos, nseg, toff, counter, mrow, countq, cq, work, total;
};
// elements of the rank pass's key / value buffers: the population (objective
// 0's q order) or the M-1 <= 3 objectives' unique values sorted as one batch
static int64_t ranks_elems(int64_t n, int64_t U) { return std::max<int64_t>(n, 3 * U); }
static size_t ranks_work_bytes(int64_t n, int64_t U) {
    const int64_t e = ranks_elems(n, U);
    return 2 * align_up((size_t)e * 8, 256) + 3 * align_up((size_t)e * 4, 256) +
           std::max(radix_sort_temp_bytes(n), radix_sort_batched_temp_bytes(3, U)) +
           scan_temp_bytes(e);
}
static size_t fronts_work_bytes(int64_t U) {
    return align_up(sizeof(FrontState), 256) + 3 * align_up((size_t)U * 8, 256) +
           2 * align_up((size_t)U * 4, 256) + 256 + radix_sort_temp_bytes(U);
}
static FastLayout fast_layout(int64_t n, int64_t U) {
    FastLayout L;
    L.NB = (U + 63) / 64;
    L.NG = (L.NB + 7) / 8;
    L.NQ = (L.NB + TW - 1) / TW;
    L.ngroups = (L.NB + TD_WPW - 1) / TD_WPW;
    L.Upad = L.NB * 64;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += align_up(std::max<size_t>(bytes, 1), 256);
        return o;
    };
    // the compare kernel's int16 partials, or the bitset pass's scratch
    L.part = take(std::max((size_t)L.ngroups * L.Upad * 2, bitdom_bytes(U, 4)));
    L.S = take((size_t)L.Upad * 16);
    L.sigma = take((size_t)U * 4);
    L.pos = take((size_t)U * 4);
    L.nseg = take((size_t)(L.ngroups + 1) * 4);
    L.toff = take((size_t)(L.ngroups + 1) * 4);
    L.counter = take(4);
    L.mrow = take((size_t)U * 8);
    L.countq = take((size_t)U * 4);
    L.cq = take((size_t)U * 4);
    L.work = take(std::max(ranks_work_bytes(n, U), fronts_work_bytes(U)));
    L.total = off;
    return L;
}
size_t fast_dom_bytes(int64_t n, int64_t U) { return fast_layout(n, U).total; }
int64_t fast_dom_words(int64_t U) {
    const int64_t NB = (U + 63) / 64, NQ = (NB + TW - 1) / TW;
    return NB * 64 * NQ * TW;
}

// Bitset tables (bitdom.hip) are the default dominance pass for 2 and 3
// objectives; four take the compare kernel: the m = 4 bitset kernels (three
// 33-KB tables, 104,640 B of LDS per workgroup) faulted on the GPU in the
// product build but not in a range-checked DM_BD_CHECK build, and a plain
// 104,640-B LDS kernel runs clean on the same boxes (tools_gpu/lds_probe.hip) —
// unresolved; DM_BD_MAXM=4 re-enables them for diagnosis.
// With the bitset pass the peel reads the tables, not a D matrix
// (peel_tab_kernel), unless the DM_DOM_PEEL_D cross-check asks for the D peel.
bool fast_bitset(const dm_ctx* ctx, int m) {
    return m >= 2 && m <= ctx->knobs.bd_maxm && ctx->dom_path != DM_DOM_COMPARE;
}
bool fast_table_peel(const dm_ctx* ctx, int m) {
    return fast_bitset(ctx, m) && ctx->dom_path != DM_DOM_PEEL_D;
}

// Ranks (objective 0 from the population's lexicographic order perm, whose
// group starts segin marks; uidx: U index of each group's representative),
// the dominance words D (fast_dom_words(U)) and count[U] (U order).
int fast_dom_build(dm_ctx* ctx, const double* wv, int m, int64_t n,
                   const int32_t* perm, const int32_t* segin, const int32_t* uidx,
                   const double* ufit, int64_t U, uint64_t* D, int32_t* count, char* ws) {
    hipStream_t s = ctx->stream;
    const int num_cus = ctx->num_cus;
    const FastLayout L = fast_layout(n, U);
    int4* S = (int4*)(ws + L.S);
    int32_t* sigma = (int32_t*)(ws + L.sigma);
    int32_t* pos = (int32_t*)(ws + L.pos);
    int32_t* nseg = (int32_t*)(ws + L.nseg);
    int32_t* toff = (int32_t*)(ws + L.toff);
    int32_t* counter = (int32_t*)(ws + L.counter);
    int16_t* part = (int16_t*)(ws + L.part);
    char* w = ws + L.work;
    const int64_t e = ranks_elems(n, U);
    uint64_t* keys = (uint64_t*)w;
    uint64_t* ktmp = (uint64_t*)(w + align_up((size_t)e * 8, 256));
    char* p = w + 2 * align_up((size_t)e * 8, 256);
    int32_t* vals = (int32_t*)p;
    int32_t* vtmp = (int32_t*)(p + align_up((size_t)e * 4, 256));
    int32_t* flag = (int32_t*)(p + 2 * align_up((size_t)e * 4, 256));
    void* rtemp = p + 3 * align_up((size_t)e * 4, 256);
    void* stemp = (char*)rtemp + std::max(radix_sort_temp_bytes(n), radix_sort_batched_temp_bytes(3, U));
    DM_HIP(hipMemsetAsync(S, 0, (size_t)L.Upad * 16, s));
    // objective 0 and the q order from the lexicographic order
    lex_flags_kernel<<<dg1(n), 256, 0, s>>>(wv, m, perm, segin, n, vals, vtmp);
    int rc;
    if ((rc = exclusive_scan_i32(s, vals, flag, n, nullptr, stemp))) return rc;
    if ((rc = exclusive_scan_i32(s, vtmp, (int32_t*)keys, n, nullptr, stemp))) return rc;
    lex_sigma_kernel<<<dg1(n), 256, 0, s>>>(perm, uidx, vals, flag, vtmp, (int32_t*)keys, n, m,
                                            sigma, pos, (int32_t*)S);
    // objectives 1..m-1: dense ranks by ONE batched sort of the unique values
    // (segment o - 1 = objective o), one flag pass, one scan, one scatter
    if (m > 1) {
        const int64_t nb = (int64_t)(m - 1) * U;
        rank_key_kernel<<<dg1(nb), 256, 0, s>>>(ufit, m, U, nb, keys, vals);
        if ((rc = radix_sort_pairs_batched(s, keys, vals, ktmp, vtmp, m - 1, U, 0, 64, rtemp)))
            return rc;
        rank_flag_kernel<<<dg1(nb), 256, 0, s>>>(keys, U, nb, flag);
        // the scan may not alias its input: the exclusive prefix goes to vtmp
        if ((rc = exclusive_scan_i32(s, flag, vtmp, nb, nullptr, stemp))) return rc;
        rank_scatter_kernel<<<dg1(nb), 256, 0, s>>>(vals, vtmp, flag, pos, U, nb, (int32_t*)S);
    }
    if (fast_bitset(ctx, m)) {  // bitset tables (bitdom.hip; DM_TIME_DOMINANCE: its count pass)
        group_reach_kernel<<<dg1(L.ngroups), 256, 0, s>>>(S, m, U, L.NG, L.ngroups, nseg);
        return bitdom_build(ctx, S, m, U, L.NQ, L.ngroups, nseg, sigma,
                            fast_table_peel(ctx, m) ? nullptr : D, count, (int32_t*)(ws + L.countq),
                            (char*)part);
    }
    tri_plan_kernel<<<1, 1024, 0, s>>>(S, m, U, L.NG, L.ngroups, nseg, toff, counter);
    const unsigned blocks = (unsigned)std::max(1, num_cus) * 8;
    timing_begin(ctx, DM_TIME_DOMINANCE);
    switch (m) {
        case 2: tri_dom_kernel<2><<<blocks, 256, 0, s>>>(S, U, L.NB, L.NQ, L.ngroups, nseg, toff, counter, D, part); break;
        case 3: tri_dom_kernel<3><<<blocks, 256, 0, s>>>(S, U, L.NB, L.NQ, L.ngroups, nseg, toff, counter, D, part); break;
        default: tri_dom_kernel<4><<<blocks, 256, 0, s>>>(S, U, L.NB, L.NQ, L.ngroups, nseg, toff, counter, D, part); break;
    }
    timing_end(ctx, DM_TIME_DOMINANCE);
    DM_LAUNCH_CHECK();
    // the rank sorts' keys / ktmp (2 n x 8 bytes) hold the TC_CHUNKS column sums
    static_assert(TC_CHUNKS * 4 <= 16, "tri_count scratch exceeds keys + ktmp");
    int32_t* ctmp = (int32_t*)keys;
    const int64_t cthreads = (U + 3) / 4;
    tri_count_part_kernel<<<dim3((unsigned)((cthreads + 255) / 256), TC_CHUNKS), 256, 0, s>>>(
        part, nseg, U, L.Upad, L.ngroups, ctmp);
    tri_count_sum_kernel<<<dg1(U), 256, 0, s>>>(ctmp, sigma, U, count, (int32_t*)(ws + L.countq));
    DM_LAUNCH_CHECK();
    return DM_OK;
}

// Integer crowding keys (selNSGA2's fast path): rk[o * T + j] = the dense rank
// of objective o (weighted-value order, equal values equal ranks) of the
// emitted individual order[j], from the ranks the dominance pass already
// holds (S in q order).  assignCrowdingDist's per-objective sorts then run on
// (front, rank) keys of ~26 bits — 4 radix passes instead of 8 + 1.
__global__ void rank_keys_kernel(const int4* S, const int32_t* pos, const int32_t* ui,
                                 const int32_t* order, int64_t T, int m, int32_t* rk) {
    DGRID_LOOP(j, T) {
        const int4 r = S[pos[ui[order[j]]]];
        for (int o = 0; o < m; ++o) rk[o * T + j] = icomp(r, o == 0 ? m - 1 : o - 1);
    }
}
int fast_rank_keys(dm_ctx* ctx, const char* ws, int64_t n, int64_t U, int m, const int32_t* ui,
                   const int32_t* order, int64_t T, int32_t* rk) {
    const FastLayout L = fast_layout(n, U);
    if (T <= 0) return DM_OK;
    rank_keys_kernel<<<dg1(T), 256, 0, ctx->stream>>>((const int4*)(ws + L.S),
                                                      (const int32_t*)(ws + L.pos), ui, order, T,
                                                      m, rk);
    DM_LAUNCH_CHECK();
    return DM_OK;
}

// Fronts 1.. after front 0 (ulist[0, *F0), rankU set): peel on the device,
// checking the status every few fronts.  F0 and sorted0 (front 0's unique
// fitnesses and individuals) stay on the device.  Fills ufront (front starts
// in ulist, host; fstarts on the device) and *sorted (individuals).  ws: the
// fast_dom_build workspace.
int fast_fronts(dm_ctx* ctx, const uint64_t* D, int m, int64_t n, int64_t U, const int32_t* F0,
                const int64_t* sorted0,
                int64_t N, const int32_t* gsize, int32_t* ulist, int32_t* rankU, int32_t* count,
                int32_t* fstarts, char* ws, std::vector<int32_t>& ufront, int64_t* sorted,
                int64_t* last_inds) {
    hipStream_t s = ctx->stream;
    const FastLayout L = fast_layout(n, U);
    const int32_t* sigma = (const int32_t*)(ws + L.sigma);
    const int32_t* pos = (const int32_t*)(ws + L.pos);
    const int32_t* nseg = (const int32_t*)(ws + L.nseg);
    int2* mrow = (int2*)(ws + L.mrow);
    int32_t* countq = (int32_t*)(ws + L.countq);
    int32_t* cq = (int32_t*)(ws + L.cq);
    char* p = ws + L.work;
    FrontState* st = (FrontState*)p;
    p += align_up(sizeof(FrontState), 256);
    uint64_t* ckey = (uint64_t*)p;
    p += align_up((size_t)U * 8, 256);
    uint64_t* ktmp = (uint64_t*)p;
    p += align_up((size_t)U * 8, 256);
    int32_t* vals = (int32_t*)p;
    p += align_up((size_t)U * 4, 256);
    int32_t* vtmp = (int32_t*)p;
    p += align_up((size_t)U * 4, 256);
    // sliced peels: per v the max (front + 1, last releasing position)
    unsigned long long* lastq = (unsigned long long*)p;
    p += align_up((size_t)U * 8, 256);
    // persistent peel: barrier counter and error flag
    unsigned* bar = (unsigned*)p;
    int32_t* perr = (int32_t*)(p + 192);  // bar[0]: arrivals, bar[16]: ordered front
    p += 256;
    void* rtemp = p;
    DM_HIP(hipMemsetAsync(lastq, 0, (size_t)U * 8, s));
    front_init_kernel<<<1, 1, 0, s>>>(st, F0, sorted0, N, U, fstarts);
    member_rows_kernel<<<dg1(U), 256, 0, s>>>(ulist, F0, pos, nseg, mrow);
    // status word and the first front starts come back together: when the
    // peel is done they are usually all that is needed (one round trip)
    char* hbuf = (char*)pinned(ctx, 2048);
    if (!hbuf) return DM_ERR_NOMEM;
    FrontState* hst = (FrontState*)hbuf;
    int32_t* hfs = (int32_t*)(hbuf + 256);
    const int64_t npre = std::min<int64_t>((2048 - 256) / 4, U + 2);
    // table-fed peel: the bitset pass's tables in the part region
    const bool tab = fast_table_peel(ctx, m);
    const BitdomLayout TL = bitdom_layout(U, m);
    const char* tws = ws + L.part;
    // launch pairs (peel, order) per front: first status check after as many
    // fronts as the previous call needed
    // (the previous call's front count + 1, so that a selection like the last
    // one needs a single status read; up to PEEL_BATCH_MAX launch pairs)
    constexpr int PEEL_BATCH_MAX = 96;
    // the hint counts only for a problem of about the same size
    const bool hinted = 4 * U >= 3 * ctx->peel_hint_U && 3 * U <= 4 * ctx->peel_hint_U &&
                        N == ctx->peel_hint_N;
    const int hint = hinted ? ctx->peel_hint : 4;
    int batch = std::max(2, std::min(hint + 1, PEEL_BATCH_MAX));
    for (;;) {
        for (int b = 0; b < batch; ++b) {
            if (tab) {
                const dim3 g((unsigned)((TL.NG + 7) & ~7ll), PEEL_SLICES);
                const int4* S = (const int4*)(ws + L.S);
                const int2* span = (const int2*)(tws + TL.span);
                const uint32_t* P = (const uint32_t*)(tws + TL.P);
                const int32_t* R = (const int32_t*)(tws + TL.R);
                const uint16_t* BK = (const uint16_t*)(tws + TL.BK);
                if (m == 2)
                    peel_tab_kernel<1><<<g, PEEL_WAVES * 64, 0, s>>>(S, span, P, R, BK, mrow, gsize, sigma,
                                                                     st, countq, lastq, ckey, cq, rankU);
                else if (m == 3)
                    peel_tab_kernel<2><<<g, PEEL_WAVES * 64, 0, s>>>(S, span, P, R, BK, mrow, gsize, sigma,
                                                                     st, countq, lastq, ckey, cq, rankU);
                else
                    peel_tab_kernel<3><<<g, PEEL_WAVES * 64, 0, s>>>(S, span, P, R, BK, mrow, gsize, sigma,
                                                                     st, countq, lastq, ckey, cq, rankU);
            } else {
                peel_owned_kernel<<<dim3((unsigned)L.NQ, PEEL_SLICES), PEEL_WAVES * 64, 0, s>>>(
                    D, L.NQ, mrow, gsize, sigma, st, countq, lastq, ckey, cq, rankU);
            }
            front_order_kernel<<<1, 1024, 0, s>>>(st, ckey, cq, ulist, mrow, pos, nseg, fstarts, 0);
        }
        DM_LAUNCH_CHECK();
        DM_HIP(hipMemcpyAsync(hst, st, sizeof(FrontState), hipMemcpyDeviceToHost, s));
        DM_HIP(hipMemcpyAsync(hfs, fstarts, (size_t)npre * 4, hipMemcpyDeviceToHost, s));
        DM_HIP(hipStreamSynchronize(s));
        if (hst->done) break;
        if (hst->overflow) {
            // a front too large for the LDS sort: the radix sort orders its keys
            const int32_t nc = hst->ncand;
            DM_HIP(hipMemsetAsync(vals, 0, (size_t)nc * 4, s));
            int rc = radix_sort_pairs(s, ckey, vals, ktmp, vtmp, nc, 0, 64, rtemp);
            if (rc) return rc;
            front_order_kernel<<<1, 1024, 0, s>>>(st, ckey, cq, ulist, mrow, pos, nseg, fstarts, 1);
            DM_LAUNCH_CHECK();
        }
        // next batch from what is left: fronts grow along the peel, so the
        // remaining individuals / the mean front size so far bounds the fronts
        // still needed (each launch past `done` returns at once but costs
        // ~10 us; each extra status check a round trip)
        const double mean = (double)hst->sorted / (double)(hst->nfronts + 1);
        const double left = (double)(hst->N - hst->sorted);
        int need = mean > 0 ? (int)std::ceil(left / mean) : 32;
        // the previous call's front count, when it had more fronts than done
        // so far, is the better estimate (later fronts are larger than the
        // mean so far); launches past `done` return at once but cost ~10 us
        if (hint > hst->nfronts) need = std::min(need, hint - hst->nfronts + 1);
        batch = std::max(2, std::min(need + 2, PEEL_BATCH_MAX));
    }
    const int32_t nf = hst->nfronts + 1;  // front 0 plus the peeled ones
    ctx->peel_hint = hst->nfronts;
    ctx->peel_hint_U = U;
    ctx->peel_hint_N = N;
    ufront.resize(nf + 1);
    if (nf + 1 <= npre) {
        std::copy(hfs, hfs + nf + 1, ufront.begin());
    } else {
        DM_HIP(hipMemcpyAsync(ufront.data(), fstarts, (size_t)(nf + 1) * 4, hipMemcpyDeviceToHost, s));
        DM_HIP(hipStreamSynchronize(s));
    }
    *sorted = hst->sorted;
    *last_inds = hst->lastinds;
    return DM_OK;
}

}  // namespace dm

#ifdef DM_PEEL_PROF
// diagnostic builds: copy out and reset the table-peel phase clocks
extern "C" int dm_debug_peel_prof(unsigned long long* host, int64_t cap) {
    unsigned int n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(dm::g_pprof_n), 4) != hipSuccess) return -1;
    n = std::min<unsigned int>(n, 1u << 17);
    const int64_t k = std::min<int64_t>(n, cap);
    if (k > 0 && hipMemcpyFromSymbol(host, HIP_SYMBOL(dm::g_pprof), (size_t)k * 64) != hipSuccess) return -1;
    const unsigned int z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(dm::g_pprof_n), &z, 4) != hipSuccess) return -1;
    return (int)k;
}
#endif
