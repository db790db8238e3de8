// pareto.hip — tools.ParetoFront.update (deap/tools/support.py:612-640) at
// population granularity for gfx950.
//
// The reference walks the population row by row against the hall.  For valid,
// NaN-free fitnesses and value-equality `similar` the result has a closed form
// (DESIGN.md §11), with H the archive in its order and P the
// population in row order:
//   1. a row of H u P survives iff no row of H u P dominates it;
//   2. a survivor is dropped iff an earlier survivor of the sequence (H, then
//      P by row) has equal fitness and an equal genome (element-wise ==);
//   3. order: lexicographic wvalues descending; among equal fitnesses the new
//      rows in descending population row, then the rows of H in their order.
// Pipeline: validity flag -> candidates C = P's own first front (the existing
// sortNondominated machinery) -> archive x C cross-dominance (the hot kernel)
// -> survivors laid out (C by descending row, then H) and sorted stably ->
// twins found inside (equal-fitness run, genome hash) groups -> compaction.
#include "sort.hpp"

namespace dm {

int validate_pop(const dm_pop* p, const char* what);

namespace {

struct PfBump {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(int64_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off += align_up((size_t)std::max<int64_t>(count, 1) * sizeof(T), 256);
        return p;
    }
};

dim3 pf_grid(int64_t n, int per_block = 256) {
    return dim3((unsigned)std::max<int64_t>(
        1, std::min<int64_t>((n + per_block - 1) / per_block, 65535)));
}

#define PF_LOOP(i, n)                                                         \
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); \
         i += (int64_t)gridDim.x * blockDim.x)

// scalars (int32 words of the `small` block)
enum { PF_BAD = 0, PF_NC = 1, PF_NS = 2, PF_NOUT = 3, PF_MAXKEY = 4 /* uint64: words 4-5 */ };

// *flag = 1 when a row is invalid or holds a NaN wvalue (idempotent stores)
__global__ void pf_invalid_kernel(const double* wv, const uint8_t* valid, int m, int64_t n,
                                  int32_t* flag) {
    PF_LOOP(i, n) {
        bool bad = valid[i] == 0;
        for (int o = 0; o < m; ++o) {
            const double x = wv[i * m + o];
            bad |= x != x;
        }
        if (bad) *flag = 1;
    }
}

// one objective: the front is the set of maximal rows
__global__ void pf_max_kernel(const double* wv, int64_t n, unsigned long long* maxkey) {
    unsigned long long best = 0;
    PF_LOOP(i, n) best = max(best, (unsigned long long)ordered_key(wv[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = max(best, other);
    }
    if ((threadIdx.x & 63) == 0) atomicMax(maxkey, best);
}
__global__ void pf_ismax_kernel(const double* wv, int64_t n, const unsigned long long* maxkey,
                                int32_t* flag) {
    const unsigned long long mk = *maxkey;
    PF_LOOP(i, n) flag[i] = ordered_key(wv[i]) == mk ? 1 : 0;
}
__global__ void pf_compact_rows_kernel(const int32_t* flag, const int32_t* pos, int64_t n,
                                       int32_t* rows) {
    PF_LOOP(i, n) if (flag[i]) rows[pos[i]] = (int32_t)i;
}

// Archive x candidates cross-dominance.  blockIdx.x: a tile of 256 candidates
// (one per thread, wvalues in registers); blockIdx.y: a chunk of archive
// tiles, staged 256 rows at a time in LDS (every lane reads the same archive
// row: broadcasts).  Both directions of Fitness.dominates (base.py:209-224)
// per pair; the flags are plain byte stores of 1 (idempotent: no atomics, no
// ordering between workgroups).  M = 0: any objective count (loop).
constexpr int PF_TILE = 256;
template <int M>
__global__ __launch_bounds__(PF_TILE) void pf_cross_kernel(
    const double* __restrict__ pwv, const int32_t* __restrict__ cand, int64_t nC,
    const double* __restrict__ awv, int64_t A, int m_rt, int64_t tiles_per_chunk,
    uint8_t* __restrict__ cand_dead, uint8_t* __restrict__ arch_dead) {
    constexpr int MM = M ? M : DM_MAX_OBJ;
    const int m = M ? M : m_rt;
    __shared__ double tile[PF_TILE * MM];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * PF_TILE + tid;
    const bool have = c < nC;
    double w[MM];
#pragma unroll
    for (int o = 0; o < MM; ++o) w[o] = 0.0;
    if (have) {
        const double* src = pwv + (int64_t)cand[c] * m;
#pragma unroll
        for (int o = 0; o < MM; ++o)
            if (o < m) w[o] = src[o];
    }
    const int64_t a0 = (int64_t)blockIdx.y * tiles_per_chunk * PF_TILE;
    const int64_t a1 = min(A, a0 + tiles_per_chunk * PF_TILE);
    bool dead = false;
    for (int64_t t = a0; t < a1; t += PF_TILE) {
        const int cnt = (int)min((int64_t)PF_TILE, a1 - t);
        __syncthreads();
        for (int k = tid; k < cnt * m; k += PF_TILE) tile[k] = awv[t * m + k];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            bool lt = false, gt = false;
#pragma unroll
            for (int o = 0; o < MM; ++o) {
                if (o < m) {
                    const double y = tile[j * m + o];
                    lt |= w[o] < y;
                    gt |= w[o] > y;
                }
            }
            dead |= lt && !gt;  // the archive row dominates the candidate
            if (__any(have && gt && !lt)) {  // a candidate of this wave dominates it
                if ((tid & 63) == 0) arch_dead[t + j] = 1;
            }
        }
    }
    if (have && dead) cand_dead[c] = 1;
}

// survivors' flags over the sequence: position j < N is population row
// N-1-j (descending row), position N+a is archive row a.  The population
// part is zeroed by the caller.
__global__ void pf_mark_kernel(const int32_t* cand, int64_t nC, const uint8_t* cand_dead,
                               const uint8_t* arch_dead, int64_t N, int64_t A, int32_t* seqflag) {
    PF_LOOP(i, nC + A) {
        if (i < nC) {
            if (!cand_dead[i]) seqflag[N - 1 - cand[i]] = 1;
        } else {
            const int64_t a = i - nC;
            seqflag[N + a] = arch_dead[a] ? 0 : 1;
        }
    }
}
// sid[s] = archive row (>= 0) or -(population row) - 1; swv[s] = its wvalues
__global__ void pf_layout_kernel(const int32_t* seqflag, const int32_t* seqpos, int64_t N,
                                 int64_t A, const double* pwv, const double* awv, int m,
                                 int32_t* sid, double* swv) {
    PF_LOOP(j, N + A) {
        if (!seqflag[j]) continue;
        const int64_t s = seqpos[j];
        const double* src;
        if (j < N) {
            const int64_t r = N - 1 - j;
            sid[s] = (int32_t)(-r - 1);
            src = pwv + r * m;
        } else {
            sid[s] = (int32_t)(j - N);
            src = awv + (j - N) * m;
        }
        for (int o = 0; o < m; ++o) swv[s * m + o] = src[o];
    }
}
// rf[i] = 1 when final position i starts a run of == wvalues (i > 0)
__global__ void pf_runflag_kernel(const double* swv, int m, const int32_t* perm, int64_t ns,
                                  int32_t* rf) {
    PF_LOOP(i, ns) {
        int32_t f = 0;
        if (i > 0) {
            const double* a = swv + (int64_t)perm[i] * m;
            const double* b = swv + (int64_t)perm[i - 1] * m;
            for (int o = 0; o < m; ++o)
                if (!(a[o] == b[o])) f = 1;
        }
        rf[i] = f;
    }
}

__device__ __forceinline__ uint64_t pf_mix(uint64_t x) {  // splitmix64 finaliser
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ const char* pf_row(const char* pg, const char* ag, int64_t stride,
                                              int32_t id) {
    return id >= 0 ? ag + (int64_t)id * stride : pg + (int64_t)(-(id + 1)) * stride;
}
// 64-bit genome hash, one wave per survivor (coalesced reads): the sum over
// the elements of mix(value bits ^ mix(position)), floats with -0.0 as 0.0.
// A row holding a NaN gene equals nothing: its hash is salted with its
// survivor index, so such rows do not pile up in one group.
__global__ void pf_hash_kernel(const char* pg, const char* ag, int64_t stride, int dim, int gtype,
                               const int32_t* sid, int64_t ns, uint64_t* hsh) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t s = wave; s < ns; s += nwaves) {
        const char* row = pf_row(pg, ag, stride, sid[s]);
        const int count = gtype == DM_BITS ? (dim + 63) / 64 : dim;
        uint64_t h = 0;
        int nan = 0;
        for (int e = lane; e < count; e += 64) {
            uint64_t bits;
            if (gtype == DM_BITS) {
                bits = reinterpret_cast<const uint64_t*>(row)[e];
            } else if (gtype == DM_F32) {
                float x = reinterpret_cast<const float*>(row)[e];
                if (x == 0.0f) x = 0.0f;
                nan |= x != x;
                uint32_t b;
                memcpy(&b, &x, 4);
                bits = b;
            } else {
                double x = reinterpret_cast<const double*>(row)[e];
                if (x == 0.0) x = 0.0;
                nan |= x != x;
                memcpy(&bits, &x, 8);
            }
            h += pf_mix(bits ^ pf_mix((uint64_t)e));
        }
        h = (uint64_t)group_sum_i<64>((int64_t)h);
        nan = __any(nan);
        if (nan) h = pf_mix(h ^ pf_mix((uint64_t)s));
        if (lane == 0) hsh[s] = h;
    }
}
__global__ void pf_key_hash_kernel(const uint64_t* hsh, const int32_t* perm, int64_t ns,
                                   uint64_t* keys, int32_t* vals) {
    PF_LOOP(i, ns) {
        keys[i] = hsh[perm[i]];
        vals[i] = (int32_t)i;
    }
}
// run id of final position vals[q] (rs: exclusive scan of rf)
__global__ void pf_key_run_kernel(const int32_t* rf, const int32_t* rs, const int32_t* vals,
                                  int64_t ns, uint64_t* keys) {
    PF_LOOP(q, ns) {
        const int32_t i = vals[q];
        keys[q] = (uint64_t)(uint32_t)(rs[i] + rf[i]);
    }
}

__device__ __forceinline__ bool pf_genome_eq(const char* a, const char* b, int dim, int gtype) {
    if (gtype == DM_BITS) {
        const uint64_t* x = reinterpret_cast<const uint64_t*>(a);
        const uint64_t* y = reinterpret_cast<const uint64_t*>(b);
        for (int e = 0; e < (dim + 63) / 64; ++e)
            if (x[e] != y[e]) return false;
        return true;
    }
    if (gtype == DM_F32) {
        const float* x = reinterpret_cast<const float*>(a);
        const float* y = reinterpret_cast<const float*>(b);
        for (int e = 0; e < dim; ++e)
            if (!(x[e] == y[e])) return false;
        return true;
    }
    const double* x = reinterpret_cast<const double*>(a);
    const double* y = reinterpret_cast<const double*>(b);
    for (int e = 0; e < dim; ++e)
        if (!(x[e] == y[e])) return false;
    return true;
}
// Sorted position q holds final position vals[q]; the groups (run, hash) keep
// the final order inside them.  A new row is dropped iff a later row of its
// group has an == genome (scan forward, stop at the first hit); archive rows
// always stay.  keep[] is written for every final position.
__global__ void pf_twin_kernel(const char* pg, const char* ag, int64_t stride, int dim, int gtype,
                               const int32_t* sid, const int32_t* perm, const uint64_t* hsh,
                               const uint64_t* runkeys, const int32_t* vals, int64_t ns,
                               int32_t* keep) {
    PF_LOOP(q, ns) {
        const int32_t i = vals[q];
        const int32_t s = perm[i];
        const int32_t id = sid[s];
        int32_t k = 1;
        if (id < 0) {
            const uint64_t run = runkeys[q], h = hsh[s];
            const char* mine = pf_row(pg, ag, stride, id);
            for (int64_t q2 = q + 1; q2 < ns; ++q2) {
                const int32_t s2 = perm[vals[q2]];
                if (runkeys[q2] != run || hsh[s2] != h) break;
                if (pf_genome_eq(mine, pf_row(pg, ag, stride, sid[s2]), dim, gtype)) {
                    k = 0;
                    break;
                }
            }
        }
        keep[i] = k;
    }
}
// kept final position i -> out row opos[i]: one wave per row, 16-B pieces
__global__ void pf_emit_kernel(const char* pg, const char* ag, const double* pwv,
                               const double* awv, int64_t stride, int m, const int32_t* sid,
                               const int32_t* perm, const int32_t* keep, const int32_t* opos,
                               int64_t ns, char* og, double* owv, uint8_t* ovalid, int32_t* src) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i = wave; i < ns; i += nwaves) {
        if (!keep[i]) continue;
        const int32_t id = sid[perm[i]];
        const int64_t o = opos[i];
        const uint4* from = reinterpret_cast<const uint4*>(pf_row(pg, ag, stride, id));
        uint4* to = reinterpret_cast<uint4*>(og + o * stride);
        for (int64_t p = lane; p < stride / 16; p += 64) to[p] = from[p];
        const double* w = id >= 0 ? awv + (int64_t)id * m : pwv + (int64_t)(-(id + 1)) * m;
        if (lane < m) owv[o * m + lane] = w[lane];
        if (lane == 0) {
            ovalid[o] = 1;
            if (src) src[o] = id;
        }
    }
}
__global__ void pf_iota_kernel(int32_t* v, int64_t n) {
    PF_LOOP(i, n) v[i] = (int32_t)i;
}

bool pf_overlap(const void* a, size_t alen, const void* b, size_t blen) {
    if (!a || !b || !alen || !blen) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + blen && y < x + alen;
}
bool pf_alias(const dm_pop* out, int64_t cap, const dm_pop* in) {
    const size_t m = (size_t)out->nobj;
    return pf_overlap(out->genes, (size_t)cap * out->stride, in->genes,
                      (size_t)in->n * in->stride) ||
           pf_overlap(out->wvalues, (size_t)cap * m * 8, in->wvalues, (size_t)in->n * m * 8) ||
           pf_overlap(out->valid, (size_t)cap, in->valid, (size_t)in->n);
}

template <int M>
void pf_launch_cross(dim3 grid, hipStream_t s, const double* pwv, const int32_t* cand, int64_t nC,
                     const double* awv, int64_t A, int m, int64_t tpc, uint8_t* cand_dead,
                     uint8_t* arch_dead) {
    pf_cross_kernel<M><<<grid, PF_TILE, 0, s>>>(pwv, cand, nC, awv, A, m, tpc, cand_dead,
                                                arch_dead);
}

}  // namespace
}  // namespace dm

using namespace dm;

extern "C" int dm_pareto_update(dm_ctx* ctx, const dm_pop* archive, const dm_pop* pop,
                                dm_pop* out, int64_t out_capacity, int64_t* n_out, int32_t* src) {
    DM_CHECK_ARG(ctx && archive && pop && out && n_out, "null argument");
    DM_CHECK_ARG(out_capacity >= 0, "negative out_capacity");
    int rc;
    if ((rc = validate_pop(archive, "archive")) || (rc = validate_pop(pop, "pop"))) return rc;
    dm_pop outc = *out;
    outc.n = out_capacity;
    if ((rc = validate_pop(&outc, "out"))) return rc;
    DM_CHECK_ARG(archive->gtype == pop->gtype && archive->dim == pop->dim &&
                     archive->stride == pop->stride && archive->nobj == pop->nobj,
                 "archive/pop layout mismatch");
    DM_CHECK_ARG(out->gtype == pop->gtype && out->dim == pop->dim && out->stride == pop->stride &&
                     out->nobj == pop->nobj,
                 "out/pop layout mismatch");
    const int64_t A = archive->n, N = pop->n, L = A + N;
    DM_CHECK_ARG(L < (1ll << 31), "archive + population too large");
    DM_CHECK_ARG(out_capacity >= L, "out_capacity %lld < archive + population rows %lld",
                 (long long)out_capacity, (long long)L);
    DM_CHECK_ARG(!pf_alias(&outc, out_capacity, archive) && !pf_alias(&outc, out_capacity, pop),
                 "out aliases an input");
    hipStream_t s = ctx->stream;
    const int m = pop->nobj;
    const int64_t stride = pop->stride;
    *n_out = 0;
    if (L == 0) {
        out->n = 0;
        return DM_OK;
    }
    if (N == 0) {  // nothing to add: the archive as it is
        outc.n = A;
        if ((rc = dm_gather(ctx, archive, nullptr, &outc))) return rc;
        if (src) pf_iota_kernel<<<pf_grid(A), 256, 0, s>>>(src, A);
        DM_LAUNCH_CHECK();
        DM_HIP(hipStreamSynchronize(s));
        *n_out = A;
        out->n = A;
        return DM_OK;
    }

    // ---- workspace: slot 5 (survives the inner sort's slots 0, 1, 3, 4),
    // sized for a power of two of rows so a growing archive seldom reallocates
    int64_t Lc = 1024;
    while (Lc < L + 2) Lc *= 2;
    const size_t rtb = radix_sort_temp_bytes(Lc), stb = scan_temp_bytes(Lc);
    const size_t a4 = align_up((size_t)Lc * 4, 256), a8 = align_up((size_t)Lc * 8, 256);
    const size_t need = 256 + 11 * a4 + 3 * a8 + align_up((size_t)Lc * m * 8, 256) + 2 * a4 +
                        align_up(rtb, 256) + align_up(stb, 256) + 4096;
    char* base = (char*)scratch_slot(ctx, 5, need);
    if (!base) return DM_ERR_NOMEM;
    int32_t* hostv = (int32_t*)pinned(ctx, 2048);
    if (!hostv) return DM_ERR_NOMEM;
    PfBump bp{base};
    int32_t* small = bp.take<int32_t>(64);
    int32_t* cand = bp.take<int32_t>(Lc);
    int32_t* fstart = bp.take<int32_t>(Lc);
    uint8_t* cand_dead = bp.take<uint8_t>(Lc);
    uint8_t* arch_dead = bp.take<uint8_t>(Lc);
    int32_t* seqflag = bp.take<int32_t>(Lc);
    int32_t* seqpos = bp.take<int32_t>(Lc);
    int32_t* sid = bp.take<int32_t>(Lc);
    double* swv = bp.take<double>(Lc * m);
    uint64_t* keys = bp.take<uint64_t>(Lc);
    uint64_t* ktmp = bp.take<uint64_t>(Lc);
    int32_t* perm = bp.take<int32_t>(Lc);
    int32_t* vtmp = bp.take<int32_t>(Lc);
    int32_t* rf = bp.take<int32_t>(Lc);
    int32_t* rs = bp.take<int32_t>(Lc);
    uint64_t* hsh = bp.take<uint64_t>(Lc);
    int32_t* vals = bp.take<int32_t>(Lc);
    void* rtemp = bp.take<char>((int64_t)rtb);
    void* stemp = bp.take<char>((int64_t)stb);
    if (bp.off > need) {
        set_error("internal workspace overflow");
        return DM_ERR_INVALID;
    }
    int32_t* keep = seqflag;  // free again after the layout
    int32_t* opos = seqpos;

    // ---- 1. validity: an invalid row or a NaN wvalue leaves the closed form
    DM_HIP(hipMemsetAsync(small, 0, 256, s));
    pf_invalid_kernel<<<pf_grid(N), 256, 0, s>>>(pop->wvalues, pop->valid, m, N, small + PF_BAD);
    if (A)
        pf_invalid_kernel<<<pf_grid(A), 256, 0, s>>>(archive->wvalues, archive->valid, m, A,
                                                     small + PF_BAD);
    DM_LAUNCH_CHECK();
    DM_HIP(hipMemcpyAsync(hostv, small, 4, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    if (hostv[0]) {
        set_error("ParetoFront closed form needs valid, NaN-free fitnesses");
        return DM_ERR_UNSUPPORTED;
    }

    // ---- 2. candidates: the population's own first front
    int64_t nC = 0;
    if (N == 1) {
        DM_HIP(hipMemsetAsync(cand, 0, 4, s));
        nC = 1;
    } else if (m == 1) {
        // the maximal rows (the sort's dominance matrix buys nothing here)
        unsigned long long* maxkey = (unsigned long long*)(small + PF_MAXKEY);
        pf_max_kernel<<<pf_grid(N), 256, 0, s>>>(pop->wvalues, N, maxkey);
        pf_ismax_kernel<<<pf_grid(N), 256, 0, s>>>(pop->wvalues, N, maxkey, seqflag);
        if ((rc = exclusive_scan_i32(s, seqflag, seqpos, N, small + PF_NC, stemp))) return rc;
        pf_compact_rows_kernel<<<pf_grid(N), 256, 0, s>>>(seqflag, seqpos, N, cand);
        DM_LAUNCH_CHECK();
        DM_HIP(hipMemcpyAsync(hostv, small + PF_NC, 4, hipMemcpyDeviceToHost, s));
        DM_HIP(hipStreamSynchronize(s));
        nC = hostv[0];
    } else {
        int64_t nsorted = 0;
        int32_t nfronts = 0;
        if ((rc = dm_sort_nondominated(ctx, pop, N, 1, cand, fstart, nullptr, &nsorted, &nfronts)))
            return rc;
        nC = nsorted;
    }
    if (nC < 1 || nC > N) {
        set_error("internal: first front of %lld rows", (long long)nC);
        return DM_ERR_INVALID;
    }

    // ---- 3. archive x candidates
    DM_HIP(hipMemsetAsync(cand_dead, 0, (size_t)nC, s));
    if (A) {
        DM_HIP(hipMemsetAsync(arch_dead, 0, (size_t)A, s));
        const int64_t gx = (nC + PF_TILE - 1) / PF_TILE, atiles = (A + PF_TILE - 1) / PF_TILE;
        // enough workgroups to fill the chip when C is small
        int64_t chunks = std::max<int64_t>(1, (4ll * ctx->num_cus + gx - 1) / gx);
        chunks = std::min<int64_t>(std::min<int64_t>(chunks, atiles), 65535);
        const int64_t tpc = (atiles + chunks - 1) / chunks;
        chunks = (atiles + tpc - 1) / tpc;
        const dim3 grid((unsigned)gx, (unsigned)chunks);
        switch (m) {
            case 1: pf_launch_cross<1>(grid, s, pop->wvalues, cand, nC, archive->wvalues, A, m, tpc, cand_dead, arch_dead); break;
            case 2: pf_launch_cross<2>(grid, s, pop->wvalues, cand, nC, archive->wvalues, A, m, tpc, cand_dead, arch_dead); break;
            case 3: pf_launch_cross<3>(grid, s, pop->wvalues, cand, nC, archive->wvalues, A, m, tpc, cand_dead, arch_dead); break;
            case 4: pf_launch_cross<4>(grid, s, pop->wvalues, cand, nC, archive->wvalues, A, m, tpc, cand_dead, arch_dead); break;
            default: pf_launch_cross<0>(grid, s, pop->wvalues, cand, nC, archive->wvalues, A, m, tpc, cand_dead, arch_dead); break;
        }
        DM_LAUNCH_CHECK();
    }

    // ---- 4. survivors in sequence layout, then the stable descending sort
    DM_HIP(hipMemsetAsync(seqflag, 0, (size_t)N * 4, s));
    pf_mark_kernel<<<pf_grid(nC + A), 256, 0, s>>>(cand, nC, cand_dead, arch_dead, N, A, seqflag);
    if ((rc = exclusive_scan_i32(s, seqflag, seqpos, L, small + PF_NS, stemp))) return rc;
    pf_layout_kernel<<<pf_grid(L), 256, 0, s>>>(seqflag, seqpos, N, A, pop->wvalues,
                                                archive->wvalues, m, sid, swv);
    DM_LAUNCH_CHECK();
    DM_HIP(hipMemcpyAsync(hostv, small + PF_NS, 4, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    const int64_t ns = hostv[0];
    if (ns < 1 || ns > L) {
        set_error("internal: %lld survivors", (long long)ns);
        return DM_ERR_INVALID;
    }
    if ((rc = lex_sort_rows(s, swv, m, ns, true, keys, ktmp, perm, vtmp, rtemp))) return rc;

    // ---- 5. twins: groups of (equal-fitness run, genome hash)
    const char* pg = (const char*)pop->genes;
    const char* ag = (const char*)archive->genes;
    pf_runflag_kernel<<<pf_grid(ns), 256, 0, s>>>(swv, m, perm, ns, rf);
    if ((rc = exclusive_scan_i32(s, rf, rs, ns, nullptr, stemp))) return rc;
    pf_hash_kernel<<<pf_grid(ns, 4), 256, 0, s>>>(pg, ag, stride, pop->dim, pop->gtype, sid, ns,
                                                  hsh);
    pf_key_hash_kernel<<<pf_grid(ns), 256, 0, s>>>(hsh, perm, ns, keys, vals);
    DM_LAUNCH_CHECK();
    if ((rc = radix_sort_pairs(s, keys, vals, ktmp, vtmp, ns, 0, 64, rtemp))) return rc;
    pf_key_run_kernel<<<pf_grid(ns), 256, 0, s>>>(rf, rs, vals, ns, keys);
    int bits = 8;
    while (bits < 32 && (1ll << bits) < ns) bits += 8;
    if ((rc = radix_sort_pairs(s, keys, vals, ktmp, vtmp, ns, 0, bits, rtemp))) return rc;
    pf_twin_kernel<<<pf_grid(ns), 256, 0, s>>>(pg, ag, stride, pop->dim, pop->gtype, sid, perm,
                                               hsh, keys, vals, ns, keep);

    // ---- 6. output
    if ((rc = exclusive_scan_i32(s, keep, opos, ns, small + PF_NOUT, stemp))) return rc;
    pf_emit_kernel<<<pf_grid(ns, 4), 256, 0, s>>>(pg, ag, pop->wvalues, archive->wvalues, stride,
                                                  m, sid, perm, keep, opos, ns, (char*)out->genes,
                                                  out->wvalues, out->valid, src);
    DM_LAUNCH_CHECK();
    DM_HIP(hipMemcpyAsync(hostv, small + PF_NOUT, 4, hipMemcpyDeviceToHost, s));
    DM_HIP(hipStreamSynchronize(s));
    *n_out = hostv[0];
    out->n = hostv[0];
    return DM_OK;
}
