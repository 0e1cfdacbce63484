// SVD of many small matrices in one launch: one-sided Jacobi (Hestenes).
//
// A workgroup owns one matrix (or 2 / 4 of the smallest class) entirely in
// LDS: G = A V (m x n, column-major, scaled by a power of two) and, when
// vectors are wanted, V (n x n).  Plane rotations orthogonalise pairs of
// columns of G until a whole sweep applies none; then sigma_j = |g_j|,
// u_j = g_j / sigma_j and V is the accumulated product of the rotations.
// DESIGN.md "Batched small SVD" has the design, the resource table and the
// measured times.
//
// The contract of this kernel (it runs beside anything else on the device):
// no communication between workgroups, no spin-waits, no atomics, every loop
// bounded (the sweep loop by kMaxSweeps, all others by the matrix sizes), no
// global state besides its arguments, A never written.  Every barrier sits in
// workgroup-uniform control flow.
//
// Pair schedule: round-robin tournament on np = n rounded up to even players;
// step k (0 .. np-2) pairs player np-1 with k and (k + j) with (k - j) mod
// (np - 1) for j = 1 .. np/2 - 1.  For odd n the dummy is player np-1, so the
// pair that meets it is slot 0 and is skipped.
//
// A pair is handled by L = MR/4 lanes (8 / 16 / 32, aligned groups of a wave):
// each lane keeps its <= 4 rows of both columns in registers, the three sums
// alpha = |g_p|^2, beta = |g_q|^2, gamma = g_p . g_q are reduced across the
// group by the fixed xor-shuffle tree (bit-reproducible), and the same lanes
// apply the rotation.  Norms are recomputed from the columns every time.
#include "brd_internal.h"

#include <cfloat>

namespace brd {

constexpr int kJacMaxSweeps = 30;   // xGESVJ's cap

template <typename T> struct JacNum;
template <> struct JacNum<double> {
    static constexpr double eps = DBL_EPSILON, big = DBL_MAX;
    static constexpr int emax = 1022;
};
template <> struct JacNum<float> {
    static constexpr float eps = FLT_EPSILON, big = FLT_MAX;
    static constexpr int emax = 126;
};

// Geometry of one capacity class: NC columns x MR rows.
template <typename T, int NC, int MR, bool WV>
struct JacCfg {
    static constexpr int L = MR / 4;                        // lanes per pair
    static constexpr int PAIRS = NC / 2;                    // pair slots per step
    static constexpr int TPM = PAIRS * L;                   // threads per matrix
    static constexpr int MPW = TPM >= 256 ? 1 : 256 / TPM;  // matrices per workgroup
    static constexpr int BLOCK = TPM * MPW;
    static constexpr int WPM = TPM / 64;                    // waves per matrix
    // column pitch: groups narrower than a half wave read several columns in one
    // LDS cycle, so consecutive columns are offset by one group's width (G) or
    // half of it (V: with the full width the fp64 64 x 64 class would exceed
    // half a CU's LDS by 872 bytes and run one workgroup per CU instead of two)
    static constexpr int GP = MR + (L < 32 ? L : 0);
    static constexpr int VP = NC + (L < 32 ? L / 2 : 0);
    static constexpr int VR = (NC + L - 1) / L;             // V rows per lane
    static constexpr int GELEMS = NC * GP;
    static constexpr int VELEMS = WV ? NC * VP : 0;
    static_assert(TPM % 64 == 0 && BLOCK <= 1024 && (L & (L - 1)) == 0 && L <= 32, "geometry");
};

template <typename T>
__device__ __forceinline__ T jac_group_sum(T v, int L) {
    for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T, int NC, int MR, bool WV>
__global__ void __launch_bounds__((JacCfg<T, NC, MR, WV>::BLOCK))
k_svd_batched(const T *__restrict__ A, int batch, int m, int n, long lda, long stride_a, T *__restrict__ S,
              T *__restrict__ U, long ldu, long stride_u, T *__restrict__ V, long ldv, long stride_v,
              int *__restrict__ info)
{
    using C = JacCfg<T, NC, MR, WV>;
    constexpr int L = C::L, TPM = C::TPM, MPW = C::MPW, GP = C::GP, VP = C::VP;
    __shared__ T sG[MPW * C::GELEMS];
    __shared__ T sV[WV ? MPW * C::VELEMS : 1];
    __shared__ T sSig[MPW * NC];
    __shared__ int sInv[MPW * NC];
    __shared__ T sMax[C::BLOCK / 64];
    __shared__ int sBad[C::BLOCK / 64];
    __shared__ int sRot[2][MPW];

    const int tid = threadIdx.x;
    const int ml = tid / TPM;              // matrix of this workgroup
    const int t = tid - ml * TPM;          // thread within the matrix
    const long mat = (long)blockIdx.x * MPW + ml;
    const bool valid = mat < batch;
    const int slot = t / L;                // pair slot
    const int l = t % L;                   // lane within the pair's group
    T *G = sG + ml * C::GELEMS;
    T *Vl = sV + (WV ? ml * C::VELEMS : 0);

    // ---- load (coalesced row reads, transposed into LDS), largest |a|, finiteness
    T mx = (T)0;
    int bad = 0;
    if (valid) {
        const T *Am = A + mat * stride_a;
        const int tot = m * n;
        for (int idx = t; idx < tot; idx += TPM) {
            const int r = idx / n, c = idx - r * n;
            const T v = Am[(long)r * lda + c];
            G[c * GP + r] = v;
            const T av = fabs(v);
            if (av <= JacNum<T>::big) mx = fmax(mx, av);
            else bad = 1;   // NaN or Inf
        }
        if (WV)
            for (int idx = t; idx < n * n; idx += TPM) {
                const int c = idx / n, r = idx - c * n;
                Vl[c * VP + r] = r == c ? (T)1 : (T)0;
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o));
        bad |= __shfl_xor(bad, o);
    }
    if ((tid & 63) == 0) {
        sMax[tid >> 6] = mx;
        sBad[tid >> 6] = bad;
    }
    if (tid < 2 * MPW) sRot[tid / MPW][tid % MPW] = 0;
    __syncthreads();
    mx = (T)0;
    bad = 0;
    for (int w = 0; w < C::WPM; ++w) {
        mx = fmax(mx, sMax[ml * C::WPM + w]);
        bad |= sBad[ml * C::WPM + w];
    }
    // power-of-two scale: the largest entry lands in [1/2, 1), so the sums of
    // up to 128 squares neither overflow nor (for the large entries) underflow
    int ex = 0;
    if (mx > (T)0 && !bad) (void)frexp(mx, &ex);
    const int exs = ex > JacNum<T>::emax ? JacNum<T>::emax : (ex < -JacNum<T>::emax ? -JacNum<T>::emax : ex);
    if (valid && !bad && exs != 0) {
        const T sc = ldexp((T)1, -exs);
        for (int c = slot; c < n; c += C::PAIRS)
            for (int r = l; r < m; r += L) G[c * GP + r] *= sc;
    }
    __syncthreads();

    // ---- sweeps
    const int np = (n + 1) & ~1;
    const int half = np >> 1;
    const bool odd = (n & 1) != 0;
    const T tol = sqrt((T)m) * JacNum<T>::eps;
    // bit j: matrix j of this workgroup still rotates (uniform over the workgroup)
    unsigned active = 0;
    for (int j = 0; j < MPW; ++j) {
        bool b = (long)blockIdx.x * MPW + j < batch;
        int bj = 0;
        for (int w = 0; w < C::WPM; ++w) bj |= sBad[j * C::WPM + w];
        if (b && !bj) active |= 1u << j;
    }
    for (int sweep = 0; sweep < kJacMaxSweeps && active != 0; ++sweep) {
        const bool mine = (active >> ml) & 1u;
        bool rot = false;
        for (int k = 0; k < np - 1; ++k) {
            int p = 0, q = 0;
            bool work = mine && slot < half;
            if (work) {
                if (slot == 0) {
                    p = k;
                    q = np - 1;
                    work = !odd;
                } else {
                    int a = k + slot;
                    if (a >= np - 1) a -= np - 1;
                    int b = k - slot;
                    if (b < 0) b += np - 1;
                    p = a < b ? a : b;
                    q = a < b ? b : a;
                }
            }
            T x[4], y[4];
            T al = (T)0, be = (T)0, ga = (T)0;
            T *gp = G + p * GP, *gq = G + q * GP;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = l + i * L;
                const bool in = work && r < m;
                x[i] = in ? gp[r] : (T)0;
                y[i] = in ? gq[r] : (T)0;
                al = fma(x[i], x[i], al);
                be = fma(y[i], y[i], be);
                ga = fma(x[i], y[i], ga);
            }
            al = jac_group_sum(al, L);
            be = jac_group_sum(be, L);
            ga = jac_group_sum(ga, L);
            if (work && fabs(ga) > tol * sqrt(al) * sqrt(be)) {
                const T zeta = (be - al) / ((T)2 * ga);
                const T tt = copysign((T)1, zeta) / (fabs(zeta) + sqrt((T)1 + zeta * zeta));
                const T cs = (T)1 / sqrt((T)1 + tt * tt);
                const T sn = cs * tt;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = l + i * L;
                    if (r < m) {
                        gp[r] = cs * x[i] - sn * y[i];
                        gq[r] = sn * x[i] + cs * y[i];
                    }
                }
                if (WV) {
                    T *vp = Vl + p * VP, *vq = Vl + q * VP;
#pragma unroll
                    for (int i = 0; i < C::VR; ++i) {
                        const int r = l + i * L;
                        if (r < n) {
                            const T vx = vp[r], vy = vq[r];
                            vp[r] = cs * vx - sn * vy;
                            vq[r] = sn * vx + cs * vy;
                        }
                    }
                }
                rot = true;
            }
            __syncthreads();
        }
        // workgroup-wide OR per matrix, double-buffered on the sweep's parity:
        // the buffer written here was cleared one sweep (>= 1 barrier) ago
        const int par = sweep & 1;
        if (rot) sRot[par][ml] = 1;
        __syncthreads();
        unsigned still = 0;
        for (int j = 0; j < MPW; ++j)
            if (sRot[par][j]) still |= 1u << j;
        active &= still;
        if (tid < MPW) sRot[par ^ 1][tid] = 0;
    }
    const bool live = valid && !bad;

    // ---- sigma_j = |g_j| (two columns per group), then the descending rank sort
    // with ties broken by column index; sInv[rank] = column
    T *sig = sSig + ml * NC;
    int *inv = sInv + ml * NC;
    for (int c = slot; c < n; c += C::PAIRS) {
        T a = (T)0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = l + i * L;
            const T v = (live && r < m) ? G[c * GP + r] : (T)0;
            a = fma(v, v, a);
        }
        a = jac_group_sum(a, L);
        if (l == 0) sig[c] = sqrt(a);
    }
    __syncthreads();
    if (live && t < n) {
        const T sj = sig[t];
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const T si = sig[i];
            rank += (si > sj || (si == sj && i < t)) ? 1 : 0;
        }
        inv[rank] = t;
    }
    __syncthreads();
    if (!valid) return;   // no barrier follows

    // ---- outputs: S with the scale undone, U = g_j / sigma_j, V; a non-finite
    // matrix gets NaN everywhere
    const T qnan = (T)NAN;
    for (int c = t; c < n; c += TPM) S[mat * n + c] = bad ? qnan : ldexp(sig[inv[c]], exs);
    if (WV) {
        T *Um = U + mat * stride_u, *Vm = V + mat * stride_v;
        const int tot = m * n;
        for (int idx = t; idx < tot; idx += TPM) {
            const int r = idx / n, c = idx - r * n;
            T v = qnan;
            if (!bad) {
                const int j = inv[c];
                const T sg = sig[j];
                v = sg > (T)0 ? G[j * GP + r] / sg : (T)0;
            }
            Um[(long)r * ldu + c] = v;
        }
        for (int idx = t; idx < n * n; idx += TPM) {
            const int r = idx / n, c = idx - r * n;
            Vm[(long)r * ldv + c] = bad ? qnan : Vl[inv[c] * VP + r];
        }
    }
    if (t == 0) info[mat] = bad ? 2 : (((active >> ml) & 1u) ? 1 : 0);
}

template <typename T, int NC, int MR>
static hipError_t jac_launch(const T *A, int batch, int m, int n, long lda, long stride_a, T *S, T *U, long ldu,
                             long stride_u, T *V, long ldv, long stride_v, int *info, hipStream_t s)
{
    if (U && V) {
        using C = JacCfg<T, NC, MR, true>;
        const int grid = (batch + C::MPW - 1) / C::MPW;
        hipLaunchKernelGGL((k_svd_batched<T, NC, MR, true>), dim3(grid), dim3(C::BLOCK), 0, s, A, batch, m, n, lda,
                           stride_a, S, U, ldu, stride_u, V, ldv, stride_v, info);
    } else {
        using C = JacCfg<T, NC, MR, false>;
        const int grid = (batch + C::MPW - 1) / C::MPW;
        hipLaunchKernelGGL((k_svd_batched<T, NC, MR, false>), dim3(grid), dim3(C::BLOCK), 0, s, A, batch, m, n, lda,
                           stride_a, S, (T *)nullptr, 0L, 0L, (T *)nullptr, 0L, 0L, info);
    }
    return hipGetLastError();
}

// Picks the capacity class: columns 16 / 32 / 64, rows 32 / 64 / 128 (n <= m,
// so 64 columns never meet 32 rows).  Sizes beyond 128 x 64 are the caller's
// to reject.
template <typename T>
hipError_t launch_svd_batched(const T *A, int batch, int m, int n, long lda, long stride_a, T *S, T *U, long ldu,
                              long stride_u, T *V, long ldv, long stride_v, int *info, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || n > 64 || m > 128) return hipErrorInvalidValue;
#define JAC_GO(NC, MR) \
    return jac_launch<T, NC, MR>(A, batch, m, n, lda, stride_a, S, U, ldu, stride_u, V, ldv, stride_v, info, s)
    if (n <= 16) {
        if (m <= 32) JAC_GO(16, 32);
        if (m <= 64) JAC_GO(16, 64);
        JAC_GO(16, 128);
    }
    if (n <= 32) {
        if (m <= 32) JAC_GO(32, 32);
        if (m <= 64) JAC_GO(32, 64);
        JAC_GO(32, 128);
    }
    if (m <= 64) JAC_GO(64, 64);
    JAC_GO(64, 128);
#undef JAC_GO
}

template hipError_t launch_svd_batched<double>(const double *, int, int, int, long, long, double *, double *, long,
                                               long, double *, long, long, int *, hipStream_t);
template hipError_t launch_svd_batched<float>(const float *, int, int, int, long, long, float *, float *, long, long,
                                              float *, long, long, int *, hipStream_t);

}  // namespace brd
