// SVD of many mid-size matrices (65 .. 128 columns, n <= m <= 128) in one
// launch: one-sided Jacobi (Hestenes), the method of brd_svd_batched.hip step
// for step (tests/jacobi_model.py is the executable specification): coalesced
// load transposed into LDS with the largest |a| and a finiteness flag, the
// power-of-two scale, the round-robin schedule on n rounded up to even (slot 0
// skipped for odd n), the rotation threshold sqrt(m) eps sqrt(alpha) sqrt(beta),
// at most 30 sweeps ending when a sweep applies no rotation, the descending
// rank sort with ties broken by column index, sigma = 0 and a zero column of U
// for a zero column, NaN outputs and info = 2 for non-finite input.
// DESIGN.md "Batched mid-size SVD" has the design, the resource table and the
// measured times.
//
// The contract of this kernel (it runs beside anything else on the device):
// no communication between workgroups, no spin-waits, no atomics, every loop
// bounded (the sweep loop by kMidMaxSweeps, all others by the matrix sizes), no
// global state besides its arguments, A never written.  Every barrier sits in
// workgroup-uniform control flow.  Reductions use a fixed tree, so two runs
// are bit-identical.  No scratch.  All index arithmetic on batch * stride and
// rows * ld is in 64 bits.
//
// Geometry: one capacity class, 128 columns x 128 rows, one workgroup of 1024
// threads per matrix.  The 64 pair slots of a step x 32 lanes of the smaller
// classes would be 2048 threads, so a pair here is handled by L = 16 lanes
// (an aligned quarter of a wave) with 8 rows per lane: 64 slots x 16 lanes.
// Columns are offset by one group's width (pitch 128 + 16) as in the narrower
// classes of brd_svd_batched.  BRD_MID_LANES = 32 builds the rejected
// geometry for comparison: 32 slots x 32 lanes x 4 rows, pitch 128, each slot
// doing two (disjoint, independent) pairs per step, j = slot and slot + 32.
// It lost by 1.60 to 1.76x on the values classes and 1.25 to 1.43x with
// vectors.  BRD_MID_LANES = 8 (64 slots x 8 lanes x 16 rows, 512 threads) is
// faster on the values and slower with vectors (DESIGN.md has the figures).
//
// Where V lives.  fp32 with vectors: in LDS beside G, as in brd_svd_batched.
// fp64 with vectors: G alone is 128 KB, so the working copy of V is kept in
// device memory, in the caller's V block of the matrix, stored transposed: row
// j of the block (the n elements at V + mat * stride_v + j * ldv) holds column
// j of the working V, so a rotation's lanes read and write contiguous runs.
// It starts as the identity and is rotated in place by the lanes that rotate
// G; nothing outside the n x n entries is touched.  A run written by one wave
// is read by another wave of the same workgroup one step later; the per-step
// __syncthreads() orders that (workgroup scope, all waves on one CU).  That
// holds in the default compilation mode only: this file must not be compiled
// with threadgroup-split mode, V must not be read through a read-only or
// non-temporal path and is never declared __restrict__ or const.  After
// convergence and after U has left LDS the working copy is read into G's
// space, and the final V is written in sorted column order and proper
// orientation.
#include "brd_internal.h"

#include <cfloat>

#ifndef BRD_MID_LANES
#define BRD_MID_LANES 16
#endif

namespace brd {

constexpr int kMidMaxSweeps = 30;   // xGESVJ's cap

template <typename T> struct MidNum;
template <> struct MidNum<double> {
    static constexpr double eps = DBL_EPSILON, big = DBL_MAX;
    static constexpr int emax = 1022;
};
template <> struct MidNum<float> {
    static constexpr float eps = FLT_EPSILON, big = FLT_MAX;
    static constexpr int emax = 126;
};

enum { kMidNoV = 0, kMidVLds = 1, kMidVMem = 2 };

// Geometry of the 128 x 128 class with LN lanes per pair.
template <typename T, int LN, int VM>
struct MidCfg {
    static constexpr int NC = 128, MR = 128;
    static constexpr int L = LN;                  // lanes per pair
    static constexpr int SLOTS = L < 16 ? NC / 2 : 1024 / L;   // groups of L lanes
    static constexpr int BLOCK = SLOTS * L;
    static constexpr int PPS = (NC / 2) / SLOTS;  // pairs per slot and step
    static constexpr int RPL = MR / L;            // rows of G per lane
    static constexpr int VR = NC / L;             // rows of V per lane
    // column pitch: as in JacCfg, groups narrower than a half wave are offset
    static constexpr int GP = MR + (L < 32 ? L : 0);
    static constexpr int VP = NC + (L < 32 ? L / 2 : 0);
    static constexpr int GELEMS = NC * GP;
    static constexpr int VELEMS = VM == kMidVLds ? NC * VP : 0;
    static_assert(SLOTS * PPS == NC / 2 && (L & (L - 1)) == 0 && L <= 32 && L >= 8 && BLOCK <= 1024, "geometry");
    static_assert(GELEMS >= NC * NC, "the final V is staged in G's space");
};

template <typename T>
__device__ __forceinline__ T mid_group_sum(T v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T, int LN, int VM>
__global__ void __launch_bounds__((MidCfg<T, LN, VM>::BLOCK))
k_svd_mid_batched(const T *__restrict__ A, int m, int n, long lda, long stride_a, T *S, T *U, long ldu,
                  long stride_u, T *V, long ldv, long stride_v, int *info)
{
    using C = MidCfg<T, LN, VM>;
    constexpr int L = C::L, SLOTS = C::SLOTS, PPS = C::PPS, RPL = C::RPL, VR = C::VR, GP = C::GP, VP = C::VP;
    constexpr int BLOCK = C::BLOCK;
    __shared__ T sG[C::GELEMS];
    __shared__ T sV[VM == kMidVLds ? C::VELEMS : 1];
    __shared__ T sSig[C::NC];
    __shared__ int sInv[C::NC];
    __shared__ T sMax[BLOCK / 64];
    __shared__ int sBad[BLOCK / 64];
    __shared__ int sRot[2];

    const int t = threadIdx.x;
    const long mat = blockIdx.x;           // one workgroup per matrix
    const int slot = t / L;                // group of L lanes
    const int l = t % L;                   // lane within the group
    T *G = sG;
    T *Vm = VM == kMidVMem ? V + mat * stride_v : nullptr;   // working V, transposed, in memory

    // ---- load (coalesced row reads, transposed into LDS), largest |a|, finiteness
    T mx = (T)0;
    int bad = 0;
    {
        const T *Am = A + mat * stride_a;
        const int tot = m * n;
        for (int idx = t; idx < tot; idx += BLOCK) {
            const int r = idx / n, c = idx - r * n;
            const T v = Am[(long)r * lda + c];
            G[c * GP + r] = v;
            const T av = fabs(v);
            if (av <= MidNum<T>::big) mx = fmax(mx, av);
            else bad = 1;   // NaN or Inf
        }
        if (VM != kMidNoV)
            for (int idx = t; idx < n * n; idx += BLOCK) {
                const int c = idx / n, r = idx - c * n;
                const T e = r == c ? (T)1 : (T)0;
                if (VM == kMidVLds) sV[c * VP + r] = e;
                else Vm[(long)c * ldv + r] = e;
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o));
        bad |= __shfl_xor(bad, o);
    }
    if ((t & 63) == 0) {
        sMax[t >> 6] = mx;
        sBad[t >> 6] = bad;
    }
    if (t < 2) sRot[t] = 0;
    __syncthreads();
    mx = (T)0;
    bad = 0;
    for (int w = 0; w < BLOCK / 64; ++w) {
        mx = fmax(mx, sMax[w]);
        bad |= sBad[w];
    }
    // power-of-two scale: the largest entry lands in [1/2, 1), so the sums of
    // up to 128 squares neither overflow nor (for the large entries) underflow
    int ex = 0;
    if (mx > (T)0 && !bad) (void)frexp(mx, &ex);
    const int exs = ex > MidNum<T>::emax ? MidNum<T>::emax : (ex < -MidNum<T>::emax ? -MidNum<T>::emax : ex);
    if (!bad && exs != 0) {
        const T sc = ldexp((T)1, -exs);
        for (int c = slot; c < n; c += SLOTS)
            for (int r = l; r < m; r += L) G[c * GP + r] *= sc;
    }
    __syncthreads();

    // ---- sweeps
    const int np = (n + 1) & ~1;
    const int half = np >> 1;
    const bool odd = (n & 1) != 0;
    const T tol = sqrt((T)m) * MidNum<T>::eps;
    bool active = !bad;   // uniform over the workgroup
    for (int sweep = 0; sweep < kMidMaxSweeps && active; ++sweep) {
        bool rot = false;
        for (int k = 0; k < np - 1; ++k) {
#pragma unroll
            for (int pp = 0; pp < PPS; ++pp) {
                const int j = slot + pp * SLOTS;   // pair index of the step
                int p = 0, q = 0;
                bool work = j < half;
                if (work) {
                    if (j == 0) {
                        p = k;
                        q = np - 1;
                        work = !odd;
                    } else {
                        int a = k + j;
                        if (a >= np - 1) a -= np - 1;
                        int b = k - j;
                        if (b < 0) b += np - 1;
                        p = a < b ? a : b;
                        q = a < b ? b : a;
                    }
                }
                T x[RPL], y[RPL];
                T al = (T)0, be = (T)0, ga = (T)0;
                T *gp = G + p * GP, *gq = G + q * GP;
#pragma unroll
                for (int i = 0; i < RPL; ++i) {
                    const int r = l + i * L;
                    const bool in = work && r < m;
                    x[i] = in ? gp[r] : (T)0;
                    y[i] = in ? gq[r] : (T)0;
                    al = fma(x[i], x[i], al);
                    be = fma(y[i], y[i], be);
                    ga = fma(x[i], y[i], ga);
                }
                al = mid_group_sum(al, L);
                be = mid_group_sum(be, L);
                ga = mid_group_sum(ga, L);
                if (work && fabs(ga) > tol * sqrt(al) * sqrt(be)) {
                    const T zeta = (be - al) / ((T)2 * ga);
                    const T tt = copysign((T)1, zeta) / (fabs(zeta) + sqrt((T)1 + zeta * zeta));
                    const T cs = (T)1 / sqrt((T)1 + tt * tt);
                    const T sn = cs * tt;
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        const int r = l + i * L;
                        if (r < m) {
                            gp[r] = cs * x[i] - sn * y[i];
                            gq[r] = sn * x[i] + cs * y[i];
                        }
                    }
                    if (VM == kMidVLds) {
                        T *vp = sV + p * VP, *vq = sV + q * VP;
#pragma unroll
                        for (int i = 0; i < VR; ++i) {
                            const int r = l + i * L;
                            if (r < n) {
                                const T vx = vp[r], vy = vq[r];
                                vp[r] = cs * vx - sn * vy;
                                vq[r] = sn * vx + cs * vy;
                            }
                        }
                    }
                    if (VM == kMidVMem) {
                        // rows p and q of the transposed working copy; all loads first
                        T *vp = Vm + (long)p * ldv, *vq = Vm + (long)q * ldv;
                        T vx[VR], vy[VR];
#pragma unroll
                        for (int i = 0; i < VR; ++i) {
                            const int r = l + i * L;
                            vx[i] = r < n ? vp[r] : (T)0;
                            vy[i] = r < n ? vq[r] : (T)0;
                        }
#pragma unroll
                        for (int i = 0; i < VR; ++i) {
                            const int r = l + i * L;
                            if (r < n) {
                                vp[r] = cs * vx[i] - sn * vy[i];
                                vq[r] = sn * vx[i] + cs * vy[i];
                            }
                        }
                    }
                    rot = true;
                }
            }
            __syncthreads();
        }
        // workgroup-wide OR, double-buffered on the sweep's parity: the buffer
        // written here was cleared one sweep (>= 1 barrier) ago
        const int par = sweep & 1;
        if (rot) sRot[par] = 1;
        __syncthreads();
        active = sRot[par] != 0;
        if (t == 0) sRot[par ^ 1] = 0;
    }

    // ---- sigma_j = |g_j|, then the descending rank sort with ties broken by
    // column index; sInv[rank] = column
    for (int c = slot; c < n; c += SLOTS) {
        T a = (T)0;
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            const int r = l + i * L;
            const T v = (!bad && r < m) ? G[c * GP + r] : (T)0;
            a = fma(v, v, a);
        }
        a = mid_group_sum(a, L);
        if (l == 0) sSig[c] = sqrt(a);
    }
    __syncthreads();
    if (!bad && t < n) {
        const T sj = sSig[t];
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const T si = sSig[i];
            rank += (si > sj || (si == sj && i < t)) ? 1 : 0;
        }
        sInv[rank] = t;
    }
    __syncthreads();

    // ---- outputs: S with the scale undone, U = g_j / sigma_j, V; a non-finite
    // matrix gets NaN everywhere
    const T qnan = (T)NAN;
    for (int c = t; c < n; c += BLOCK) S[mat * n + c] = bad ? qnan : ldexp(sSig[sInv[c]], exs);
    if (VM != kMidNoV) {
        T *Um = U + mat * stride_u;
        const int tot = m * n;
        for (int idx = t; idx < tot; idx += BLOCK) {
            const int r = idx / n, c = idx - r * n;
            T v = qnan;
            if (!bad) {
                const int j = sInv[c];
                const T sg = sSig[j];
                v = sg > (T)0 ? G[j * GP + r] / sg : (T)0;
            }
            Um[(long)r * ldu + c] = v;
        }
        if (VM == kMidVLds) {
            T *Vo = V + mat * stride_v;
            for (int idx = t; idx < n * n; idx += BLOCK) {
                const int r = idx / n, c = idx - r * n;
                Vo[(long)r * ldv + c] = bad ? qnan : sV[sInv[c] * VP + r];
            }
        } else {
            // U has left LDS: stage the working copy (column c at row c of the
            // block) in G's space, then write V in place of it
            __syncthreads();
            if (!bad)
                for (int idx = t; idx < n * n; idx += BLOCK) {
                    const int c = idx / n, r = idx - c * n;
                    G[c * n + r] = Vm[(long)c * ldv + r];
                }
            __syncthreads();
            for (int idx = t; idx < n * n; idx += BLOCK) {
                const int r = idx / n, c = idx - r * n;
                Vm[(long)r * ldv + c] = bad ? qnan : G[sInv[c] * n + r];
            }
        }
    }
    if (t == 0) info[mat] = bad ? 2 : (active ? 1 : 0);
}

// fp64 with vectors keeps V in device memory (G alone fills the LDS), fp32
// with vectors keeps it in LDS.
template <typename T>
hipError_t launch_svd_mid_batched(const T *A, int batch, int m, int n, long lda, long stride_a, T *S, T *U, long ldu,
                                  long stride_u, T *V, long ldv, long stride_v, int *info, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || m > 128) return hipErrorInvalidValue;
    constexpr int LN = BRD_MID_LANES;
    constexpr int VM = sizeof(T) == 8 ? kMidVMem : kMidVLds;
    if (U && V)
        hipLaunchKernelGGL((k_svd_mid_batched<T, LN, VM>), dim3(batch), dim3(MidCfg<T, LN, VM>::BLOCK), 0, s, A, m, n, lda,
                           stride_a, S, U, ldu, stride_u, V, ldv, stride_v, info);
    else
        hipLaunchKernelGGL((k_svd_mid_batched<T, LN, kMidNoV>), dim3(batch), dim3(MidCfg<T, LN, kMidNoV>::BLOCK), 0, s, A, m, n,
                           lda, stride_a, S, (T *)nullptr, 0L, 0L, (T *)nullptr, 0L, 0L, info);
    return hipGetLastError();
}

template hipError_t launch_svd_mid_batched<double>(const double *, int, int, int, long, long, double *, double *, long,
                                                   long, double *, long, long, int *, hipStream_t);
template hipError_t launch_svd_mid_batched<float>(const float *, int, int, int, long, long, float *, float *, long,
                                                  long, float *, long, long, int *, hipStream_t);

}  // namespace brd
