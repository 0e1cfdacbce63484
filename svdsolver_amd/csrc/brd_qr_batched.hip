// Batched QR of tall matrices (m > 128, n <= 64) and its back-application: the
// front end that carries the batched Jacobi SVD (brd_svd_batched.hip) to any
// number of rows.  A = Q R with R n x n, R = U_R S V^T by the Jacobi kernel,
// U = Q U_R.  DESIGN.md "Batched tall SVD" has the method, the resource table
// and the measured times.
//
// k_qr_tall_factor: one workgroup per matrix streams row blocks of RB rows
// through LDS.  The first block is factored by Householder QR (reflector j is
// e_j plus rows j+1.. of column j); every further block B_k is folded in as
// the QR of the stacked [R; B_k] with R upper triangular: reflector j is
// [e_j; v_j], so step j touches only row j of R and the block.  When vectors
// are wanted the v_j of block k go to the rows of U that block k occupies (for
// the first block in explicit form: zeros above the diagonal, one on it) and
// tau to the workspace, one scalar per column per block.  A is read once.
//
// k_qr_tall_apply: U = Q [U_R; 0].  The blocks' reflectors are applied in
// reverse order; the columns of the result are independent, so a wave keeps
// its columns of the current block in registers and runs through the block's
// reflectors with no barrier; each block of U overwrites the v's it was
// computed from.
//
// Scaling: the stacked [R; B_k] is kept scaled by a power of two such that the
// largest entry seen so far lies in [1/2, 1); when a block brings a larger
// entry, R is rescaled (exactly) to the new exponent.  R leaves with the scale
// undone.  No pass over A besides the one that factors it.
//
// Work split in both kernels: 4 waves; wave w owns columns w, w + 4, ...; a
// lane owns rows lane, lane + 64, ... of the block.  Dot products over the
// rows are reduced across the wave by one fixed tree (qr_wave_sum), so every
// wave gets bit-identical norms of column j and two runs are bit-identical.
//
// The contract of these kernels (they run beside anything else on the device):
// no communication between workgroups, no spin-waits, no atomics, every loop
// bounded by the matrix sizes, no global state besides the arguments, A never
// written.  Every barrier sits in workgroup-uniform control flow.
#include "brd_internal.h"

#include <cfloat>

namespace brd {

template <typename T> struct QrNum;
template <> struct QrNum<double> {
    static constexpr double big = DBL_MAX;
    static constexpr int emax = 1022;
};
template <> struct QrNum<float> {
    static constexpr float big = FLT_MAX;
    static constexpr int emax = 126;
};

constexpr int kQrBlock = 256;            // threads per workgroup
constexpr int kQrWaves = kQrBlock / 64;

int qr_tall_row_block(int n) { return n <= 32 ? 256 : 128; }

// Geometry of one column class: NC columns, row blocks of RB rows.
template <typename T, int NC>
struct QrCfg {
    static constexpr int RB = NC <= 32 ? 256 : 128;
    static constexpr int RPL = RB / 64;           // rows per lane
    static constexpr int CPW = NC / kQrWaves;     // columns per wave
    // column pitches (odd: the transposing loads and stores spread over the banks)
    static constexpr int XP = NC + RB + 1;        // factor: [R; B] stacked
    static constexpr int VP = RB + 1;             // apply: the block's reflectors
    static constexpr int WP = NC + 1;             // apply: the running top n x n
    static_assert(NC % kQrWaves == 0 && RB % 64 == 0, "geometry");
};

// Cross-lane moves inside a row of 16 lanes are DPP modifiers of a plain move
// (no LDS round trip): CTRL 0xB1 / 0x4E are quad_perm [1,0,3,2] / [2,3,0,1],
// i.e. lane ^ 1 and lane ^ 2; 0x141 / 0x140 mirror a half row / a row.
template <int CTRL>
__device__ __forceinline__ float qr_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ double qr_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// Sums of N values over the 64 lanes, the N trees interleaved.  The tree is
// fixed: pairs, quads, the two quads of a half row (mirrored: after the quad
// step every lane of a quad holds the same sum, so which lane of the other
// quad it meets does not matter), the two halves of a row, then rows 16 and 32
// lanes apart.  Every step adds the same two numbers in both partners, so all
// 64 lanes end with the same bits.
template <typename T, int N>
__device__ __forceinline__ void qr_wave_sum(T (&d)[N]) {
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qr_dpp<0xB1>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qr_dpp<0x4E>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qr_dpp<0x141>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += qr_dpp<0x140>(d[q]);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += __shfl_xor(d[q], 16);
#pragma unroll
    for (int q = 0; q < N; ++q) d[q] += __shfl_xor(d[q], 32);
}

template <typename T, int NC, bool WV>
__global__ void __launch_bounds__(kQrBlock)
k_qr_tall_factor(const T *__restrict__ A, int m, int n, long lda, long stride_a, T *__restrict__ R,
                 T *__restrict__ U, long ldu, long stride_u, T *__restrict__ tau)
{
    using C = QrCfg<T, NC>;
    constexpr int RB = C::RB, RPL = C::RPL, CPW = C::CPW, XP = C::XP;
    __shared__ T X[NC * XP];        // column c: rows 0 .. NC-1 of R, then the block
    __shared__ T sBeta[NC];
    __shared__ T sScal[NC];
    __shared__ T sMax[kQrWaves];
    __shared__ int sBad[kQrWaves];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const long mat = blockIdx.x;
    const T *Am = A + mat * stride_a;
    const int nblk = (m + RB - 1) / RB;
    int e = -QrNum<T>::emax;        // exponent of the current scale
    int anybad = 0;

    for (int blk = 0; blk < nblk; ++blk) {
        const long row0 = (long)blk * RB;
        const int rb = (long)m - row0 < RB ? (int)(m - row0) : RB;
        const bool first = blk == 0;

        // ---- load (coalesced row reads, transposed into LDS; rows past the
        // end are zero), largest |a|, finiteness
        T mx = (T)0;
        int bad = 0;
        for (int idx = tid; idx < RB * n; idx += kQrBlock) {
            const int r = idx / n, c = idx - r * n;
            T v = (T)0;
            if (r < rb) {
                v = Am[(row0 + r) * lda + c];
                const T av = fabs(v);
                if (av <= QrNum<T>::big) mx = fmax(mx, av);
                else bad = 1;   // NaN or Inf
            }
            X[c * XP + NC + r] = v;
        }
        for (int o = 32; o > 0; o >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, o));
            bad |= __shfl_xor(bad, o);
        }
        if (lane == 0) {
            sMax[wv] = mx;
            sBad[wv] = bad;
        }
        __syncthreads();
        for (int w = 0; w < kQrWaves; ++w) {
            mx = fmax(mx, sMax[w]);
            anybad |= sBad[w];
        }
        int en = e;
        if (mx > (T)0) {
            int ek;
            (void)frexp(mx, &ek);
            ek = ek > QrNum<T>::emax ? QrNum<T>::emax : (ek < -QrNum<T>::emax ? -QrNum<T>::emax : ek);
            en = ek > e ? ek : e;
        }
        if (en != e && !first)
            for (int idx = tid; idx < n * n; idx += kQrBlock) {
                const int i = idx / n, c = idx - i * n;
                if (c >= i) X[c * XP + i] = ldexp(X[c * XP + i], e - en);
            }
        e = en;
        {
            const T sc = ldexp((T)1, -e);
            for (int idx = tid; idx < rb * n; idx += kQrBlock) {   // the elements this thread stored
                const int r = idx / n, c = idx - r * n;
                X[c * XP + NC + r] *= sc;
            }
        }
        __syncthreads();

        // ---- n reflectors.  Column j is final when step j starts; every wave
        // forms its norm itself (same tree, same bits) beside the dot products
        // with its own columns.
        for (int j = 0; j < n; ++j) {
            const int rlo = first ? j + 1 : 0;        // first block row of v_j
            const int piv = first ? NC + j : j;       // the row e_j stands for
            T xj[RPL];
            T xc[CPW][RPL], d[CPW + 1];   // d[CPW]: |v_j|^2 before scaling
            d[CPW] = (T)0;
#pragma unroll
            for (int i = 0; i < RPL; ++i) {
                const int r = lane + 64 * i;
                xj[i] = r >= rlo ? X[j * XP + NC + r] : (T)0;
                d[CPW] = fma(xj[i], xj[i], d[CPW]);
            }
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQrWaves * q;
                d[q] = (T)0;
                if (c > j && c < n) {
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        const int r = lane + 64 * i;
                        xc[q][i] = r >= rlo ? X[c * XP + NC + r] : (T)0;
                        d[q] = fma(xj[i], xc[q][i], d[q]);
                    }
                }
            }
            qr_wave_sum(d);
            const T s2 = d[CPW];
            const T alpha = X[j * XP + piv];
            T beta = alpha, tj = (T)0, scal = (T)0;
            if (s2 != (T)0) {
                beta = -copysign(sqrt(fma(alpha, alpha, s2)), alpha);
                tj = (beta - alpha) / beta;
                scal = (T)1 / (alpha - beta);
            }
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQrWaves * q;
                if (c > j && c < n) {
                    const T top = X[c * XP + piv];
                    const T tw = tj * fma(scal, d[q], top);
                    const T f = tw * scal;
#pragma unroll
                    for (int i = 0; i < RPL; ++i) {
                        const int r = lane + 64 * i;
                        if (r >= rlo) X[c * XP + NC + r] = fma(-f, xj[i], xc[q][i]);
                    }
                    if (lane == 0) X[c * XP + piv] = top - tw;
                }
            }
            if (lane == 0 && (j & (kQrWaves - 1)) == wv) {
                sBeta[j] = beta;
                sScal[j] = scal;
                if (WV) tau[(mat * nblk + blk) * n + j] = tj;
            }
            __syncthreads();
        }

        // ---- the diagonal of R (and, after the first block, R itself) into
        // place; the reflectors to U
        if (first) {
            for (int idx = tid; idx < n * n; idx += kQrBlock) {
                const int i = idx / n, c = idx - i * n;
                if (c >= i) X[c * XP + i] = c == i ? sBeta[i] : X[c * XP + NC + i];
            }
        } else if (tid < n) {
            X[tid * XP + tid] = sBeta[tid];
        }
        if (WV) {
            T *Um = U + mat * stride_u;
            for (int idx = tid; idx < rb * n; idx += kQrBlock) {
                const int r = idx / n, c = idx - r * n;
                T v = X[c * XP + NC + r] * sScal[c];
                if (first && r <= c) v = r == c ? (T)1 : (T)0;
                Um[(row0 + r) * ldu + c] = v;
            }
        }
        __syncthreads();
    }

    // ---- R with the scale undone; a non-finite matrix hands NaN to the SVD
    T *Rm = R + mat * (long)n * n;
    for (int idx = tid; idx < n * n; idx += kQrBlock) {
        const int i = idx / n, c = idx - i * n;
        Rm[idx] = anybad ? (T)NAN : (c >= i ? ldexp(X[c * XP + i], e) : (T)0);
    }
}

template <typename T, int NC>
__global__ void __launch_bounds__(kQrBlock)
k_qr_tall_apply(const T *__restrict__ UR, const T *__restrict__ tau, const int *__restrict__ info, int m, int n,
                T *__restrict__ U, long ldu, long stride_u)
{
    using C = QrCfg<T, NC>;
    constexpr int RB = C::RB, RPL = C::RPL, CPW = C::CPW, VP = C::VP, WP = C::WP;
    __shared__ T Vs[NC * VP];       // the block's reflectors, then its part of U
    __shared__ T Ws[NC * WP];       // the top n x n of Q [U_R; 0] so far
    __shared__ T sTau[NC];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const long mat = blockIdx.x;
    T *Um = U + mat * stride_u;
    if (info[mat] == 2) {           // non-finite input: NaN everywhere (uniform over the workgroup)
        for (long idx = tid; idx < (long)m * n; idx += kQrBlock) {
            const long r = idx / n;
            Um[r * ldu + (idx - r * n)] = (T)NAN;
        }
        return;
    }
    const int nblk = (m + RB - 1) / RB;
    const T *URm = UR + mat * (long)n * n;
    for (int idx = tid; idx < n * n; idx += kQrBlock) {
        const int r = idx / n, c = idx - r * n;
        Ws[c * WP + r] = URm[idx];
    }

    for (int blk = nblk - 1; blk >= 0; --blk) {
        const long row0 = (long)blk * RB;
        const int rb = (long)m - row0 < RB ? (int)(m - row0) : RB;
        const bool first = blk == 0;
        for (int idx = tid; idx < RB * n; idx += kQrBlock) {
            const int r = idx / n, c = idx - r * n;
            Vs[c * VP + r] = r < rb ? Um[(row0 + r) * ldu + c] : (T)0;
        }
        if (tid < n) sTau[tid] = tau[(mat * nblk + blk) * n + tid];
        __syncthreads();

        // this wave's columns of the block: [U_R; 0] for the first block (its
        // reflectors are explicit, the row of e_j included), zero otherwise
        // (e_j stands for row j of Ws)
        T cc[CPW][RPL];
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const int c = wv + kQrWaves * q;
#pragma unroll
            for (int i = 0; i < RPL; ++i) {
                const int r = lane + 64 * i;
                cc[q][i] = (first && c < n && r < n) ? Ws[c * WP + r] : (T)0;
            }
        }
        for (int j = n - 1; j >= 0; --j) {
            T vj[RPL], d[CPW];
#pragma unroll
            for (int i = 0; i < RPL; ++i) vj[i] = Vs[j * VP + lane + 64 * i];
            const T tj = sTau[j];
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                d[q] = (T)0;
#pragma unroll
                for (int i = 0; i < RPL; ++i) d[q] = fma(vj[i], cc[q][i], d[q]);
            }
            qr_wave_sum(d);
#pragma unroll
            for (int q = 0; q < CPW; ++q) {
                const int c = wv + kQrWaves * q;
                if (c < n) {
                    T w = d[q];
                    if (!first) {
                        const T top = Ws[c * WP + j];
                        w += top;
                        if (lane == 0) Ws[c * WP + j] = top - tj * w;
                    }
                    const T tw = tj * w;
#pragma unroll
                    for (int i = 0; i < RPL; ++i) cc[q][i] = fma(-tw, vj[i], cc[q][i]);
                }
            }
        }
        __syncthreads();            // every wave is done with the reflectors
#pragma unroll
        for (int q = 0; q < CPW; ++q) {
            const int c = wv + kQrWaves * q;
            if (c < n) {
#pragma unroll
                for (int i = 0; i < RPL; ++i) Vs[c * VP + lane + 64 * i] = cc[q][i];
            }
        }
        __syncthreads();
        for (int idx = tid; idx < rb * n; idx += kQrBlock) {
            const int r = idx / n, c = idx - r * n;
            Um[(row0 + r) * ldu + c] = Vs[c * VP + r];
        }
        __syncthreads();            // before the next block's reflectors replace Vs
    }
}

template <typename T, int NC>
static hipError_t qr_factor_go(const T *A, int batch, int m, int n, long lda, long stride_a, T *R, T *U, long ldu,
                               long stride_u, T *tau, hipStream_t s)
{
    if (U)
        hipLaunchKernelGGL((k_qr_tall_factor<T, NC, true>), dim3(batch), dim3(kQrBlock), 0, s, A, m, n, lda, stride_a,
                           R, U, ldu, stride_u, tau);
    else
        hipLaunchKernelGGL((k_qr_tall_factor<T, NC, false>), dim3(batch), dim3(kQrBlock), 0, s, A, m, n, lda,
                           stride_a, R, (T *)nullptr, 0L, 0L, (T *)nullptr);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_qr_tall_factor(const T *A, int batch, int m, int n, long lda, long stride_a, T *R, T *U, long ldu,
                                 long stride_u, T *tau, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || n > 64 || (U != nullptr) != (tau != nullptr)) return hipErrorInvalidValue;
    if (n <= 16) return qr_factor_go<T, 16>(A, batch, m, n, lda, stride_a, R, U, ldu, stride_u, tau, s);
    if (n <= 32) return qr_factor_go<T, 32>(A, batch, m, n, lda, stride_a, R, U, ldu, stride_u, tau, s);
    return qr_factor_go<T, 64>(A, batch, m, n, lda, stride_a, R, U, ldu, stride_u, tau, s);
}

template <typename T>
hipError_t launch_qr_tall_apply(const T *UR, const T *tau, const int *info, int batch, int m, int n, T *U, long ldu,
                                long stride_u, hipStream_t s)
{
    if (batch < 1 || n < 1 || m < n || n > 64) return hipErrorInvalidValue;
    if (n <= 16)
        hipLaunchKernelGGL((k_qr_tall_apply<T, 16>), dim3(batch), dim3(kQrBlock), 0, s, UR, tau, info, m, n, U, ldu,
                           stride_u);
    else if (n <= 32)
        hipLaunchKernelGGL((k_qr_tall_apply<T, 32>), dim3(batch), dim3(kQrBlock), 0, s, UR, tau, info, m, n, U, ldu,
                           stride_u);
    else
        hipLaunchKernelGGL((k_qr_tall_apply<T, 64>), dim3(batch), dim3(kQrBlock), 0, s, UR, tau, info, m, n, U, ldu,
                           stride_u);
    return hipGetLastError();
}

template hipError_t launch_qr_tall_factor<double>(const double *, int, int, int, long, long, double *, double *, long,
                                                  long, double *, hipStream_t);
template hipError_t launch_qr_tall_factor<float>(const float *, int, int, int, long, long, float *, float *, long,
                                                 long, float *, hipStream_t);
template hipError_t launch_qr_tall_apply<double>(const double *, const double *, const int *, int, int, int, double *,
                                                 long, long, hipStream_t);
template hipError_t launch_qr_tall_apply<float>(const float *, const float *, const int *, int, int, int, float *, long,
                                                long, hipStream_t);

}  // namespace brd
