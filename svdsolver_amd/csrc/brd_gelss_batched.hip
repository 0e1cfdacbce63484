// Batched least squares / pseudo-inverse from the batched SVD factors
// (DESIGN.md "Batched least squares"): per matrix
//
//     X = R diag(sigma+) (L^T B),   sigma+_j = 1 / sigma_j  if sigma_j > rcond sigma_1, else 0
//
// with L = U, R = V for min |A x - b| and L = V, R = U for the minimum-norm
// solution of A^T x = b; B == nullptr stands for the identity (X = R sigma+ L^T,
// the pseudo-inverse).  Everything is row-major.
//
// One launch, grid = (matrix, tile of 16 right-hand sides) linearised, 256
// threads = 4 waves.  No atomics, no communication between workgroups; every
// sum is taken in a fixed order, so the result is bit-reproducible.
//
//   phase 1  C = L^T B (n x 16): rows of L and B in chunks of KR rows staged
//            through LDS (zero-padded to a multiple of 16 columns there, never
//            in memory); wave w owns the 16-row blocks w and w + 4 of C and
//            walks every chunk in row order on the 16x16x4 MFMA.  With the
//            identity the tile is 16 rows of L transposed: nothing is summed.
//   phase 2  sigma+ into LDS (every tile recomputes the n compares), C scaled
//            by it on its way to LDS; workgroup (matrix, tile 0) writes rank.
//   phase 3  X = R C: rows of R in chunks of KR rows through the same LDS
//            block, one 16 x 16 block of X per wave and chunk, K = n on the
//            MFMA in two interleaved accumulators (even / odd k-steps), summed
//            at the end.
//
// Matrices with info == 2 (non-finite A) get NaN in X and rank -1.  Reads stay
// inside the n columns of the factors, the nrhs columns of B and the callers'
// rows; writes inside the nrhs columns and rows_r rows of X.
//
// LDS (elements): KR (NP + 4) + 16 KR + 16 NP + NP with NP = n rounded up to
// 16; KR = 32 rows (fp64) / 64 rows (fp32): at most 55,296 B / 46,592 B.
#include "brd_internal.h"

#include <limits>

namespace brd {
namespace {

constexpr int kLsThreads = 256;
constexpr int kLsWaves = kLsThreads / 64;
constexpr int kLsTile = 16;     // right-hand sides per workgroup = the MFMA's N
constexpr int kLsNmax = 128;    // columns of a factor
constexpr int kLsPad = 4;       // pitch of the factor chunk in LDS: NP + 4

// MFMA 16x16x4, one operand element per lane:
//   A operand lane l: A[m = l&15][k = l>>4],  B operand lane l: B[k = l>>4][n = l&15]
//   D register g of lane l: row crow(l>>4, g), column l&15
template <typename T> struct LsMf;
template <> struct LsMf<double> {
    typedef double v4 __attribute__((ext_vector_type(4)));
    static constexpr int KR = 32;
    static __device__ __forceinline__ v4 mma(double a, double b, v4 c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int crow(int q, int g) { return q + 4 * g; }
};
template <> struct LsMf<float> {
    typedef float v4 __attribute__((ext_vector_type(4)));
    static constexpr int KR = 64;
    static __device__ __forceinline__ v4 mma(float a, float b, v4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int crow(int q, int g) { return 4 * q + g; }
};

static inline size_t gelss_lds_elems(int n, int kr) {
    const int np = (n + 15) & ~15;
    return (size_t)kr * (np + kLsPad) + (size_t)kr * kLsTile + (size_t)np * kLsTile + np;
}

// rows [row0, row0 + rc) x columns [0, n) of F (leading dimension ld) into
// Fs (KR x NP at pitch NP + 4), zero beyond rc rows and n columns.  KR NP is a
// multiple of the block size, so every thread runs the same number of steps.
// The loads go out in groups of up to 16 per thread before the first of them
// is stored: one load per trip of a rolled loop would pay the memory latency
// KR NP / 256 times per chunk.
template <typename T, int G>
__device__ __forceinline__ void stage_group(T *Fs, const T *F, long ld, long row0, int rc, int n, int NP, int &r,
                                            int &c, int dr, int dc) {
    const int FP = NP + kLsPad;
    T v[G];
    int o[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
        v[u] = (r < rc && c < n) ? F[(row0 + r) * ld + c] : (T)0;
        o[u] = r * FP + c;
        r += dr;
        c += dc;
        if (c >= NP) {
            c -= NP;
            ++r;
        }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) Fs[o[u]] = v[u];
}

template <typename T, int KR>
__device__ __forceinline__ void stage_factor(T *Fs, const T *F, long ld, long row0, int rc, int n, int NP, int tid) {
    const int dr = kLsThreads / NP, dc = kLsThreads - dr * NP;
    int r = tid / NP, c = tid - r * NP;
    const int steps = KR * NP / kLsThreads;
    int it = 0;
    for (; it + 16 <= steps; it += 16) stage_group<T, 16>(Fs, F, ld, row0, rc, n, NP, r, c, dr, dc);
    for (; it + 4 <= steps; it += 4) stage_group<T, 4>(Fs, F, ld, row0, rc, n, NP, r, c, dr, dc);
    for (; it < steps; ++it) stage_group<T, 1>(Fs, F, ld, row0, rc, n, NP, r, c, dr, dc);
}

template <typename T>
__global__ __launch_bounds__(kLsThreads) void k_gelss_solve(const T *__restrict__ L, int rows_l, long ldl,
                                                            long stride_l, const T *__restrict__ R, int rows_r,
                                                            long ldr, long stride_r, const T *__restrict__ S, int n,
                                                            T rcond, const T *__restrict__ B, int nrhs, long ldb,
                                                            long stride_b, T *__restrict__ X, long ldx, long stride_x,
                                                            int *__restrict__ rank, const int *__restrict__ info,
                                                            int tiles)
{
    typedef LsMf<T> M;
    typedef typename M::v4 v4;
    constexpr int KR = M::KR;
    extern __shared__ __align__(16) unsigned char ls_smem[];

    const int NP = (n + 15) & ~15;
    const int FP = NP + kLsPad;
    T *Fs = (T *)ls_smem;            // KR x FP: a chunk of L, then of R
    T *Bs = Fs + KR * FP;            // KR x 16: a chunk of B
    T *Cs = Bs + KR * kLsTile;       // NP x 16: sigma+ (L^T B)
    T *sInv = Cs + NP * kLsTile;     // NP: sigma+

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long mat = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x - mat * tiles);
    const int t0 = tile * kLsTile;
    const int nt = nrhs - t0 < kLsTile ? nrhs - t0 : kLsTile;
    T *Xm = X + mat * stride_x;

    if (info[mat] == 2) {            // uniform over the workgroup
        const T nan = std::numeric_limits<T>::quiet_NaN();
        for (int r = wv; r < rows_r; r += kLsWaves)
            if (lane < nt) Xm[(long)r * ldx + t0 + lane] = nan;
        if (tile == 0 && tid == 0 && rank) rank[mat] = -1;
        return;
    }

    const T *Lm = L + mat * stride_l;
    const T *Rm = R + mat * stride_r;
    const T *Sm = S + mat * (long)n;

    // ---- phase 2 (first half): sigma+ and the rank -------------------------
    const T cut = rcond * Sm[0];
    for (int j = tid; j < NP; j += kLsThreads) {
        const T sj = j < n ? Sm[j] : (T)0;
        sInv[j] = (j < n && sj > cut) ? (T)1 / sj : (T)0;
    }
    if (tile == 0 && wv == 0 && rank) {
        int cnt = 0;
        for (int j0 = 0; j0 < NP; j0 += 64) {
            const int j = j0 + lane;
            cnt += __popcll(__ballot(j < n && Sm[j < n ? j : 0] > cut));
        }
        if (lane == 0) rank[mat] = cnt;
    }
    __syncthreads();

    // ---- phase 1: Cs = sigma+ (L^T B) ---------------------------------------
    const int q4 = lane >> 4, l16 = lane & 15;
    if (B) {
        const T *Bm = B + mat * stride_b;
        const int nb = NP >> 4;
        v4 acc[2];
        acc[0] = (v4)(0);
        acc[1] = (v4)(0);
        for (long row0 = 0; row0 < rows_l; row0 += KR) {
            const int rc = rows_l - row0 < KR ? (int)(rows_l - row0) : KR;
            T bv[KR * kLsTile / kLsThreads];
#pragma unroll
            for (int u = 0; u < KR * kLsTile / kLsThreads; ++u) {
                const int idx = tid + u * kLsThreads, r = idx >> 4, c = idx & 15;
                bv[u] = (r < rc && c < nt) ? Bm[(row0 + r) * ldb + t0 + c] : (T)0;
            }
            stage_factor<T, KR>(Fs, Lm, ldl, row0, rc, n, NP, tid);
#pragma unroll
            for (int u = 0; u < KR * kLsTile / kLsThreads; ++u) Bs[tid + u * kLsThreads] = bv[u];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int blk = wv + kLsWaves * q;
                if (blk < nb) {      // uniform over the wave
#pragma unroll 4
                    for (int k0 = 0; k0 < KR; k0 += 4) {
                        const T a = Fs[(k0 + q4) * FP + blk * 16 + l16];
                        const T b = Bs[(k0 + q4) * kLsTile + l16];
                        acc[q] = M::mma(a, b, acc[q]);
                    }
                }
            }
            __syncthreads();         // before the next chunk replaces Fs and Bs
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int blk = wv + kLsWaves * q;
            if (blk < nb) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int j = blk * 16 + M::crow(q4, g);
                    // rows beyond n are exact zeros whatever B holds
                    Cs[j * kLsTile + l16] = j < n ? acc[q][g] * sInv[j] : (T)0;
                }
            }
        }
    } else {
        // identity: column t of the tile is row t0 + t of L
        for (int t = wv; t < kLsTile; t += kLsWaves)
            for (int j = lane; j < NP; j += 64)
                Cs[j * kLsTile + t] = (j < n && t < nt) ? Lm[(long)(t0 + t) * ldl + j] * sInv[j] : (T)0;
    }
    __syncthreads();

    // ---- phase 3: X = R Cs ----------------------------------------------------
    for (long row0 = 0; row0 < rows_r; row0 += KR) {
        const int rc = rows_r - row0 < KR ? (int)(rows_r - row0) : KR;
        stage_factor<T, KR>(Fs, Rm, ldr, row0, rc, n, NP, tid);
        __syncthreads();
        if (wv < KR / 16) {          // uniform over the wave; KR / 16 row blocks per chunk
            v4 a0 = (v4)(0), a1 = (v4)(0);
            const T *Fr = Fs + (wv * 16 + l16) * FP + q4;
            const T *Cr = Cs + q4 * kLsTile + l16;
            for (int k0 = 0; k0 < NP; k0 += 8) {
                a0 = M::mma(Fr[k0], Cr[k0 * kLsTile], a0);
                a1 = M::mma(Fr[k0 + 4], Cr[(k0 + 4) * kLsTile], a1);
            }
            a0 += a1;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int r = wv * 16 + M::crow(q4, g);
                if (r < rc && l16 < nt) Xm[(row0 + r) * ldx + t0 + l16] = a0[g];
            }
        }
        __syncthreads();             // before the next chunk replaces Fs
    }
}

}  // namespace

template <typename T>
hipError_t launch_gelss_solve(const T *L, int rows_l, long ldl, long stride_l, const T *R, int rows_r, long ldr,
                              long stride_r, const T *S, int n, T rcond, const T *B, int nrhs, long ldb,
                              long stride_b, T *X, long ldx, long stride_x, int *rank, const int *info, int batch,
                              hipStream_t s)
{
    if (!L || !R || !S || !X || !info || batch < 1 || n < 1 || n > kLsNmax || rows_l < 1 || rows_r < 1)
        return hipErrorInvalidValue;
    if (!B) nrhs = rows_l;
    if (nrhs < 1 || ldl < n || ldr < n || ldx < nrhs || (B && ldb < nrhs)) return hipErrorInvalidValue;
    const long tiles = ((long)nrhs + kLsTile - 1) / kLsTile;
    if (tiles * batch > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = gelss_lds_elems(n, LsMf<T>::KR) * sizeof(T);
    hipLaunchKernelGGL((k_gelss_solve<T>), dim3((unsigned)(tiles * batch)), dim3(kLsThreads), lds, s, L, rows_l, ldl,
                       stride_l, R, rows_r, ldr, stride_r, S, n, rcond, B, nrhs, ldb, stride_b, X, ldx, stride_x,
                       rank, info, (int)tiles);
    return hipGetLastError();
}

template hipError_t launch_gelss_solve<double>(const double *, int, long, long, const double *, int, long, long,
                                               const double *, int, double, const double *, int, long, long, double *,
                                               long, long, int *, const int *, int, hipStream_t);
template hipError_t launch_gelss_solve<float>(const float *, int, long, long, const float *, int, long, long,
                                              const float *, int, float, const float *, int, long, long, float *,
                                              long, long, int *, const int *, int, hipStream_t);

}  // namespace brd
