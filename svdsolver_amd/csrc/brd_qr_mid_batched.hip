// Batched QR of tall matrices with 65 .. 128 columns (m > 128) and its
// back-application: the 128-column class of the front end in
// brd_qr_batched.hip, which carries the mid-size Jacobi kernel
// (brd_svd_mid_batched.hip) to any number of rows.  A = Q R with R n x n,
// R = U_R S V^T by the Jacobi kernel, U = Q U_R.  The method is that of
// brd_qr_batched.hip step for step (tests/tall_model.py at a row block of 128
// is the executable specification); DESIGN.md "Batched tall mid-size SVD" has
// the layout, the resource table and the measured times.
//
// What differs from the narrower classes is where R lives.  [R; block] stacked
// in LDS no longer fits (128 columns x (128 + 64 + 1) x 8 B = 193 KB), and it
// does not have to: in a stacked step j only row j of R is touched.  So the
// LDS holds the row block alone (128 columns at pitch 129), the diagonal of R
// (every wave reads R[j][j] in step j) sits in a small LDS array, and the
// strict upper triangle of R lives in the workspace's R, in device memory.
// Only the wave that owns column c reads or writes R[j][c], one lane per
// column, and row j + 1 is fetched while step j computes.  The apply kernel
// keeps the running top n x n (W) the same way, in place in the workspace's
// U_R.
//
// k_qr_mid_factor: one workgroup per matrix streams row blocks of 128 rows
// through LDS.  The first block (>= n rows, since m >= n and n <= 128) is
// factored in LDS by Householder QR and hands R's strict upper triangle to the
// workspace; every further block B_k is folded in as the QR of the stacked
// [R; B_k] with reflectors [e_j; v_j].  With vectors the v_j go to the rows of
// U that block k occupies (first block: explicit form) and tau to the
// workspace, one scalar per column per block.  A is read once.
//
// k_qr_mid_apply: U = Q [U_R; 0], the blocks' reflectors in reverse order; a
// wave keeps its columns of the current block in registers and runs through
// the block's reflectors with no barrier.
//
// Scaling: as in brd_qr_batched.hip, a running power-of-two scale with the
// largest entry seen so far in [1/2, 1); when a block raises the exponent, R
// (workspace and diagonal) is rescaled exactly.  R leaves with the scale
// undone.
//
// Work split: 8 waves; wave w owns columns w, w + 8, ... (16 per wave); a lane
// owns rows lane and lane + 64 of the block.  Dot products are reduced by the
// fixed tree of qr_wave_sum, so every wave gets bit-identical norms of column
// j and two runs are bit-identical.
//
// Device memory written by one lane and read by another of the same workgroup
// (R and W between blocks, the rescale and the final un-scaling pass) follows
// the rules brd_svd_mid_batched.hip set for its memory-resident V: a
// __syncthreads() between the write and the read, plain loads, pointers
// neither const nor __restrict__, and this file is not to be built in
// threadgroup-split mode.
//
// The contract of these kernels (they run beside anything else on the device):
// no communication between workgroups, no spin-waits, no atomics, every loop
// bounded by the matrix sizes, no global state besides the arguments, A never
// written, no scratch, 64-bit index arithmetic on batch * stride and m * ld.
// Every barrier sits in workgroup-uniform control flow.
#include "brd_internal.h"

#include <cfloat>

namespace brd {

template <typename T> struct QmNum;
template <> struct QmNum<double> {
    static constexpr double big = DBL_MAX;
    static constexpr int emax = 1022;
};
template <> struct QmNum<float> {
    static constexpr float big = FLT_MAX;
    static constexpr int emax = 126;
};

constexpr int kQmBlock = 512;             // threads per workgroup
constexpr int kQmWaves = kQmBlock / 64;
constexpr int kQmNC = 128;                // columns of the class
constexpr int kQmRB = 128;                // rows per block
constexpr int kQmRPL = kQmRB / 64;        // rows per lane
constexpr int kQmCPW = kQmNC / kQmWaves;  // columns per wave
constexpr int kQmBP = kQmRB + 1;          // column pitch of the block in LDS (odd)

int qr_tall_mid_row_block(int) { return kQmRB; }

// The DPP moves and the fixed summation tree of brd_qr_batched.hip.
template <int CTRL>
__device__ __forceinline__ float qm_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ double qm_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

template <typename T, int N>
__device__ __forceinline__ void qm_wave_sum(T (&d)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qm_dpp<0xB1>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qm_dpp<0x4E>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qm_dpp<0x141>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qm_dpp<0x140>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += __shfl_xor(d[q], 16);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += __shfl_xor(d[q], 32);
}

// R, U and tau are written and (R) read back by other lanes of the workgroup:
// neither const nor __restrict__.
template <typename T, bool WV>
__global__ void __launch_bounds__(kQmBlock)
k_qr_mid_factor(const T *__restrict__ A, int m, int n, long lda, long stride_a, T *R, T *U, long ldu,
                long stride_u, T *tau)
{
    constexpr int RB = kQmRB, RPL = kQmRPL, CPW = kQmCPW, BP = kQmBP, NC = kQmNC;
    __shared__ T X[NC * BP];        // column c of the block at X + c * BP
    __shared__ T sDiag[NC];         // the diagonal of R
    __shared__ T sBeta[NC];
    __shared__ T sScal[NC];
    __shared__ T sMax[kQmWaves];
    __shared__ int sBad[kQmWaves];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const long mat = blockIdx.x;
    const T *Am = A + mat * stride_a;
    T *Rm = R + mat * (long)n * n;
    const int nblk = (m + RB - 1) / RB;
    const int myc = wv + kQmWaves * lane;   // the column whose R[j][.] this lane carries (lane < CPW)
    int e = -QmNum<T>::emax;        // exponent of the current scale
    int anybad = 0;

    for (int blk = 0; blk < nblk; ++blk) {
        const long row0 = (long)blk * RB;
        const int rb = (long)m - row0 < RB ? (int)(m - row0) : RB;
        const bool first = blk == 0;

        // ---- load (coalesced row reads, transposed into LDS; rows past the
        // end are zero), largest |a|, finiteness
        T mx = (T)0;
        int bad = 0;
        for (int idx = tid; idx < RB * n; idx += kQmBlock) {
            const int r = idx / n, c = idx - r * n;
            T v = (T)0;
            if (r < rb) {
                v = Am[(row0 + r) * lda + c];
                const T av = fabs(v);
                if (av <= QmNum<T>::big) mx = fmax(mx, av);
                else bad = 1;   // NaN or Inf
            }
            X[c * BP + r] = v;
        }
        for (int o = 32; o > 0; o >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, o));
            bad |= __shfl_xor(bad, o);
        }
        if (lane == 0) {
            sMax[wv] = mx;
            sBad[wv] = bad;
        }
        __syncthreads();            // also orders the previous block's writes of R before the reads below
        for (int w = 0; w < kQmWaves; ++w) {
            mx = fmax(mx, sMax[w]);
            anybad |= sBad[w];
        }
        int en = e;
        if (mx > (T)0) {
            int ek;
            (void)frexp(mx, &ek);
            ek = ek > QmNum<T>::emax ? QmNum<T>::emax : (ek < -QmNum<T>::emax ? -QmNum<T>::emax : ek);
            en = ek > e ? ek : e;
        }
        if (en != e && !first) {    // uniform over the workgroup
            for (int idx = tid; idx < n * n; idx += kQmBlock) {
                const int i = idx / n, c = idx - i * n;
                if (c > i) Rm[idx] = ldexp(Rm[idx], e - en);
            }
            if (tid < n) sDiag[tid] = ldexp(sDiag[tid], e - en);
        }
        e = en;
        {
            const T sc = ldexp((T)1, -e);
            for (int idx = tid; idx < rb * n; idx += kQmBlock) {   // the elements this thread stored
                const int r = idx / n, c = idx - r * n;
                X[c * BP + r] *= sc;
            }
        }
        __syncthreads();

        // ---- n reflectors.  Column j is final when step j starts; every wave
        // forms its norm itself (same tree, same bits) beside the dot products
        // with its own columns.  After the first block lane q < CPW of a wave
        // carries R[j][wv + 8 q]: rcur for step j, rnxt fetched for step j + 1
        // (step j touches row j only).
        T rcur = (T)0;
        if (!first && lane < CPW && myc < n && myc > 0) rcur = Rm[myc];
        for (int j = 0; j < n; ++j) {
            const int rlo = first ? j + 1 : 0;        // first block row of v_j
            T rnxt = (T)0;
            if (!first && j + 1 < n && lane < CPW && myc < n && myc > j + 1) rnxt = Rm[(long)(j + 1) * n + myc];
            T xj[RPL];
            T xc[CPW][RPL], d[CPW + 1];   // d[CPW]: |v_j|^2 before scaling
            d[CPW] = (T)0;
#pragma unroll
            for (int i = 0; i < RPL; ++i) {
                const int r = lane + 64 * i;
                xj[i] = r >= rlo ? X[j * BP + r] : (T)0;
                d[CPW] = fma(xj[i], xj[i], d[CPW]);
            }
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQmWaves * q;
                d[q] = (T)0;
                if (c > j && c < n) {
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        const int r = lane + 64 * i;
                        xc[q][i] = r >= rlo ? X[c * BP + r] : (T)0;
                        d[q] = fma(xj[i], xc[q][i], d[q]);
                    }
                }
            }
            qm_wave_sum(d);
            const T s2 = d[CPW];
            const T alpha = first ? X[j * BP + j] : sDiag[j];
            T beta = alpha, tj = (T)0, scal = (T)0;
            if (s2 != (T)0) {
                beta = -copysign(sqrt(fma(alpha, alpha, s2)), alpha);
                tj = (beta - alpha) / beta;
                scal = (T)1 / (alpha - beta);
            }
            T rnew = rcur;
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQmWaves * q;
                if (c > j && c < n) {
                    const T top = first ? X[c * BP + j] : __shfl(rcur, q);
                    const T tw = tj * fma(scal, d[q], top);
                    const T f = tw * scal;
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        const int r = lane + 64 * i;
                        if (r >= rlo) X[c * BP + r] = fma(-f, xj[i], xc[q][i]);
                    }
                    if (first) {
                        if (lane == 0) X[c * BP + j] = top - tw;
                    } else if (lane == q) {
                        rnew = top - tw;
                    }
                }
            }
            if (!first && lane < CPW && myc < n && myc > j) Rm[(long)j * n + myc] = rnew;
            rcur = rnxt;
            if (lane == 0 && (j & (kQmWaves - 1)) == wv) {
                sBeta[j] = beta;
                sScal[j] = scal;
                if (WV) tau[(mat * nblk + blk) * n + j] = tj;
            }
            __syncthreads();
        }

        // ---- the diagonal of R and, from the first block, its strict upper
        // triangle into place; the reflectors to U
        if (first)
            for (int idx = tid; idx < n * n; idx += kQmBlock) {
                const int i = idx / n, c = idx - i * n;
                if (c > i) Rm[idx] = X[c * BP + i];
            }
        if (tid < n) sDiag[tid] = sBeta[tid];
        if (WV) {
            T *Um = U + mat * stride_u;
            for (int idx = tid; idx < rb * n; idx += kQmBlock) {
                const int r = idx / n, c = idx - r * n;
                T v = X[c * BP + r] * sScal[c];
                if (first && r <= c) v = r == c ? (T)1 : (T)0;
                Um[(row0 + r) * ldu + c] = v;
            }
        }
        __syncthreads();
    }

    // ---- R with the scale undone; a non-finite matrix hands NaN to the SVD
    for (int idx = tid; idx < n * n; idx += kQmBlock) {
        const int i = idx / n, c = idx - i * n;
        T v = (T)0;
        if (c > i) v = ldexp(Rm[idx], e);
        else if (c == i) v = ldexp(sDiag[i], e);
        Rm[idx] = anybad ? (T)NAN : v;
    }
}

// UR is the running top n x n of Q [U_R; 0], updated in place.
template <typename T>
__global__ void __launch_bounds__(kQmBlock)
k_qr_mid_apply(T *UR, const T *tau, const int *info, int m, int n, T *U, long ldu, long stride_u)
{
    constexpr int RB = kQmRB, RPL = kQmRPL, CPW = kQmCPW, BP = kQmBP, NC = kQmNC;
    __shared__ T Vs[NC * BP];       // the block's reflectors, then its part of U
    __shared__ T sTau[NC];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const long mat = blockIdx.x;
    T *Um = U + mat * stride_u;
    if (info[mat] == 2) {           // non-finite input: NaN everywhere (uniform over the workgroup)
        for (long idx = tid; idx < (long)m * n; idx += kQmBlock) {
            const long r = idx / n;
            Um[r * ldu + (idx - r * n)] = (T)NAN;
        }
        return;
    }
    const int nblk = (m + RB - 1) / RB;
    T *Wm = UR + mat * (long)n * n;
    const int myc = wv + kQmWaves * lane;   // the column whose W[j][.] this lane carries (lane < CPW)

    for (int blk = nblk - 1; blk >= 0; --blk) {
        const long row0 = (long)blk * RB;
        const int rb = (long)m - row0 < RB ? (int)(m - row0) : RB;
        const bool first = blk == 0;
        for (int idx = tid; idx < RB * n; idx += kQmBlock) {
            const int r = idx / n, c = idx - r * n;
            Vs[c * BP + r] = r < rb ? Um[(row0 + r) * ldu + c] : (T)0;
        }
        if (tid < n) sTau[tid] = tau[(mat * nblk + blk) * n + tid];
        __syncthreads();            // also orders the previous block's writes of W before the reads below

        // this wave's columns of the block: [U_R; 0] for the first block (its
        // reflectors are explicit, the row of e_j included), zero otherwise
        // (e_j stands for row j of W)
        T cc[CPW][RPL];
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const int c = wv + kQmWaves * q;
#pragma unroll
            for (int i = 0; i < RPL; ++i) {
                const int r = lane + 64 * i;
                cc[q][i] = (first && c < n && r < n) ? Wm[(long)r * n + c] : (T)0;
            }
        }
        const bool mine = !first && lane < CPW && myc < n;
        T wcur = mine ? Wm[(long)(n - 1) * n + myc] : (T)0;
        for (int j = n - 1; j >= 0; --j) {
            const T wnxt = (mine && j > 0) ? Wm[(long)(j - 1) * n + myc] : (T)0;
            T vj[RPL], d[CPW];
#pragma unroll
            for (int i = 0; i < RPL; ++i) vj[i] = Vs[j * BP + lane + 64 * i];
            const T tj = sTau[j];
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                d[q] = (T)0;
#pragma unroll
                for (int i = 0; i < RPL; ++i) d[q] = fma(vj[i], cc[q][i], d[q]);
            }
            qm_wave_sum(d);
            T wnew = wcur;
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQmWaves * q;
                if (c < n) {
                    T w = d[q];
                    if (!first) {
                        const T top = __shfl(wcur, q);
                        w += top;
                        if (lane == q) wnew = top - tj * w;
                    }
                    const T tw = tj * w;
#pragma unroll
                    for (int i = 0; i < RPL; ++i) cc[q][i] = fma(-tw, vj[i], cc[q][i]);
                }
            }
            if (mine) Wm[(long)j * n + myc] = wnew;
            wcur = wnxt;
        }
        __syncthreads();            // every wave is done with the reflectors
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const int c = wv + kQmWaves * q;
            if (c < n) {
#pragma unroll
                for (int i = 0; i < RPL; ++i) Vs[c * BP + lane + 64 * i] = cc[q][i];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < rb * n; idx += kQmBlock) {
            const int r = idx / n, c = idx - r * n;
            Um[(row0 + r) * ldu + c] = Vs[c * BP + r];
        }
        __syncthreads();            // before the next block's reflectors replace Vs
    }
}

template <typename T>
hipError_t launch_qr_tall_mid_factor(const T *A, int batch, int m, int n, long lda, long stride_a, T *R, T *U,
                                     long ldu, long stride_u, T *tau, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || n > kQmNC || (U != nullptr) != (tau != nullptr)) return hipErrorInvalidValue;
    if (U)
        hipLaunchKernelGGL((k_qr_mid_factor<T, true>), dim3(batch), dim3(kQmBlock), 0, s, A, m, n, lda, stride_a, R, U,
                           ldu, stride_u, tau);
    else
        hipLaunchKernelGGL((k_qr_mid_factor<T, false>), dim3(batch), dim3(kQmBlock), 0, s, A, m, n, lda, stride_a, R,
                           (T *)nullptr, 0L, 0L, (T *)nullptr);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_qr_tall_mid_apply(T *UR, const T *tau, const int *info, int batch, int m, int n, T *U, long ldu,
                                    long stride_u, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || n > kQmNC) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_qr_mid_apply<T>), dim3(batch), dim3(kQmBlock), 0, s, UR, tau, info, m, n, U, ldu, stride_u);
    return hipGetLastError();
}

template hipError_t launch_qr_tall_mid_factor<double>(const double *, int, int, int, long, long, double *, double *,
                                                      long, long, double *, hipStream_t);
template hipError_t launch_qr_tall_mid_factor<float>(const float *, int, int, int, long, long, float *, float *, long,
                                                     long, float *, hipStream_t);
template hipError_t launch_qr_tall_mid_apply<double>(double *, const double *, const int *, int, int, int, double *,
                                                     long, long, hipStream_t);
template hipError_t launch_qr_tall_mid_apply<float>(float *, const float *, const int *, int, int, int, float *, long,
                                                    long, hipStream_t);

}  // namespace brd
